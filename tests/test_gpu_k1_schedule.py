"""The schedule of the tile stream (csrc/tiles.hip) does not show in a job's results: K1 of the first tiles is enqueued before the job sets up its consumers
(start_tile_stream), a tile goes to K2 at the end of its last phase 2 while its CRC pass still runs, and the kind of file is read from one sample of the first records
taken on the device. Counters, per-base depth and site counts equal the oracle's in every layout and switch setting of the stream; a set-up that fails behind the enqueued
K1 leaves the handle usable; the sample decides as the host's eight round trips did."""
import numpy as np
import pytest

import bamgen_lib as G
import hostprep as H
import oracle_lib as O
import k1sched_cases as K
from conftest import RESOURCES

pytestmark = pytest.mark.gpu
ngsqc = __import__("importlib").import_module("ngs-bits_amd")
OMIM = RESOURCES + "/hg38_440_omim_genes.bed"
SITES = [(0, p) for p in range(15_900_100, 15_925_000, 97)]


@pytest.fixture(scope="module")
def short_bam(tmp_path_factory):
    """a few thousand short reads, a BED inside the 25 kb they cover, and what the oracle makes of them"""
    d = tmp_path_factory.mktemp("k1sched")
    p = str(d / "short.bam"); G.write(p, n_reads=5000, seed=41, start_pos=15_900_000)
    bed = str(d / "roi.bed"); open(bed, "w").write("chr1\t15900500\t15905000\nchr1\t15910000\t15918000\n")
    ob = O.Bam(p)
    exp = O.mapping(ob, ngsqc.MODE_WGS, bed, merge_bed=False)
    exp_sites = O.site_pileup(ob, SITES, 1, 13, False)
    assert int(exp.depth.sum()) > 10000 and int(exp_sites.sum()) > 1000
    return p, bed, exp, exp_sites


def _job_and_check(h, bed, exp, exp_sites):
    out = K.job(ngsqc, h, bed, sites=SITES)
    K.assert_counters(out["counters"], exp)
    assert np.array_equal(h.depth(int(out["counters"][26])), exp.depth)
    assert np.array_equal(out["site_counts"][:, :6], exp_sites)


@pytest.mark.parametrize("env", [{}, {"NGSQC_TILE_MEMBERS": "2"}, {"NGSQC_PIPELINE": "0"}, {"NGSQC_PIPELINE": "0", "NGSQC_TILE_MEMBERS": "2"}, {"NGSQC_K1_SERIAL": "1"},
                                 {"NGSQC_K1_SERIAL": "1", "NGSQC_TILE_MEMBERS": "2"}, {"NGSQC_VERIFY_CRC": "0"}, {"NGSQC_VERIFY_CRC": "0", "NGSQC_TILE_MEMBERS": "2"}],
                         ids=lambda e: "-".join(f"{k[6:].lower()}{v}" for k, v in e.items()) or "default")
def test_same_results_in_every_schedule(short_bam, monkeypatch, env):
    p, bed, exp, exp_sites = short_bam
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h = ngsqc.Handle(path=p)
    _job_and_check(h, bed, exp, exp_sites)
    assert ("NGSQC_TILE_MEMBERS" in env) == (h.timings()["n_tiles"] > 1)
    h.close()


@pytest.mark.parametrize("drop", [True, False])
def test_two_jobs_on_one_handle(short_bam, drop):
    """the second job decodes again (drop_decoded) or visits the resident tile: start_tile_stream then enqueues nothing"""
    p, bed, exp, exp_sites = short_bam
    h = ngsqc.Handle(path=p)
    _job_and_check(h, bed, exp, exp_sites)
    first = h.timings()["members_inflated"]
    if drop:
        h.drop_decoded()
    _job_and_check(h, bed, exp, exp_sites)
    assert h.timings()["members_inflated"] == first == h.n_blocks
    h.close()


@pytest.mark.parametrize("tile_members", [None, "2"])
def test_setup_that_fails_behind_the_enqueued_k1(short_bam, monkeypatch, tile_members):
    """an unsorted region list is refused by the depth set-up, which now runs while K1 of the first tiles is already queued: the queued work is taken down, the
    error is the set-up's, and the next job on the same handle is a clean one"""
    p, bed, exp, exp_sites = short_bam
    if tile_members:
        monkeypatch.setenv("NGSQC_TILE_MEMBERS", tile_members)
    h = ngsqc.Handle(path=p)
    regs, _ = H.bed_regions(bed, h.refs, 3); tx, ty = H.xy_tids(h.refs)
    assert len(regs) == 2
    mp = dict(mode=ngsqc.MODE_WGS, regions=regs[::-1], min_mapq=1, tid_x=tx, tid_y=ty, nonspecial=H.nonspecial(h.refs))
    for _ in range(2):
        with pytest.raises(ngsqc.NgsqcError) as ei:
            h.run_job(mapping=mp, sites=SITES)
        assert "Merged and sorted BED file required" in str(ei.value) and ei.value.code == -3, (ei.value.code, str(ei.value))
    _job_and_check(h, bed, exp, exp_sites)
    h.close()


# walkers_per_member of the job at the parent of this change (one run on an MI355X; positive: walkers per member, negative: members per walker = long-read mode):
#   short 1, ont -16, few 1, short_then_long -16, header_only 1
def _kinds(tmp):
    return {
        "short": (lambda: G.generate(3000, seed=31, threads=2).tobytes(), OMIM, +1),
        "ont": (lambda: G.generate(300, seed=32, threads=2, mode=1, depth=40.0).tobytes(), OMIM, -1),
        "few": (lambda: K.records_bam([100] * 5, 33), tmp, +1),                            # fewer than the eight records of a sample
        "short_then_long": (lambda: K.records_bam([100] + [12000] * 10, 34), tmp, -1),     # the first record alone would say "short reads"
        "header_only": (lambda: K.bam([K.header()]), tmp, +1),                             # nothing to sample
    }


@pytest.mark.parametrize("kind", ["short", "ont", "few", "short_then_long", "header_only"])
def test_file_kind_sample(tmp_path, kind):
    bed = str(tmp_path / "roi.bed"); open(bed, "w").write(K.BED_TEXT)
    make, b, sign = _kinds(bed)[kind]
    p = str(tmp_path / (kind + ".bam")); open(p, "wb").write(make())
    ob = O.Bam(p)
    h = ngsqc.Handle(path=p)
    out = K.job(ngsqc, h, b)
    K.assert_counters(out["counters"], O.mapping(ob, ngsqc.MODE_WGS, b, merge_bed=False))
    w = int(h.timings()["walkers_per_member"])
    assert (w > 0) - (w < 0) == sign, w
    h.close()
