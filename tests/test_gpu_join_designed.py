"""The mate join on the GPU (csrc/join.h NameJoin: join_resolve_kernel, held_bytes_kernel, held_store_kernel and the two-pool hand-over, under the keys kernels
of csrc/pairs.hip, csrc/fastq.hip and csrc/downsample.hip) over the designed cases of tests/join_cases.py: every case through Handle.filter_pairs (all-pass
parameters and the defaults, which fail the designed MAPQ 10 records), Handle.to_fastq and Handle.downsample with names, at the default geometry, with one
BGZF member per tile, and with 2 and 4 hash bits. Records, counts and text must be the oracles'; the bytes must not depend on the geometry.

On the kernels before the name rule (a name ends at its first NUL) c_string_names fails, got / expected: BamFilter with all-pass parameters (3, 0) / (7, 0)
pairs passed and dropped; BamToFastq paired 3 / 7, unmatched 8 / 0, max_cached 8 / 5 (test_gpu_tofastq_designed.py::test_names_with_more_than_one_nul). Every
other case passed there."""
import os

import pytest

import bamdownsample_oracle as D
import bamfilter_oracle as F
import bamtofastq_oracle as Q
import join_cases as K
from test_gpu_bamtofastq import text_of, with_env

ngsqc = __import__("importlib").import_module("ngs-bits_amd")
pytestmark = pytest.mark.gpu

ALL_PASS = dict(min_mq=0, max_mm=-1, max_gap=-1)
GEOMETRIES = [{}, {"NGSQC_TILE_MEMBERS": "1"}, {"NGSQC_TILE_MEMBERS": "1", "NGSQC_NAME_HASH_BITS": "2"}, {"NGSQC_TILE_MEMBERS": "1", "NGSQC_NAME_HASH_BITS": "4"},
              {"NGSQC_NAME_HASH_BITS": "2"}]


def run_all(path, tmp, want_tiles=False):
    """every tool over the file with one handle: {tool: (result, output bytes ...)} and the tiles of the pass"""
    h = ngsqc.Handle(path=path)
    try:
        out = {}
        for label, kw in (("filter_all", ALL_PASS), ("filter_defaults", {})):
            o = os.path.join(tmp, label + ".bam")
            out[label] = (h.filter_pairs(o, **kw), open(o, "rb").read())
        o1, o2 = os.path.join(tmp, "o1.gz"), os.path.join(tmp, "o2.gz")
        out["tofastq"] = (h.to_fastq(o1, o2), open(o1, "rb").read(), open(o2, "rb").read())
        n_tiles = h.timings()["n_tiles"]
        o = os.path.join(tmp, "ds.bam")
        out["downsample"] = (h.downsample(o, 50, 7, want_names=True), open(o, "rb").read())
        return out, n_tiles
    finally:
        h.close()


@pytest.mark.parametrize("name", [f.__name__ for f in K.SMALL])
def test_case(tmp_path, name):
    case = getattr(K, name)()
    recs = case.records
    path = case.write(str(tmp_path / "in.bam"))
    ref, tiles = None, {}
    for env in GEOMETRIES:
        got, n_tiles = with_env(env, lambda: run_all(path, str(tmp_path)))
        tiles[env.get("NGSQC_TILE_MEMBERS", "")] = n_tiles
        if ref is None:
            ref = got
            for label, kw in (("filter_all", ALL_PASS), ("filter_defaults", {})):
                exp, passed, dropped = F.filter_pairs(recs, **kw)
                hdr, out = F.read_bam(got[label][1])
                print(name, label, "got", got[label][0], len(out), "expected", (passed, dropped), len(exp))
                assert got[label][0] == (passed, dropped) and hdr == K.header() and out == exp, label
            e1, e2, c = Q.to_fastq(recs)
            print(name, "tofastq got", got["tofastq"][0], "expected", c)
            assert got["tofastq"][0] == c
            assert text_of(str(tmp_path / "o1.gz")) == e1 and text_of(str(tmp_path / "o2.gz")) == e2
            exp, _, dc, names = D.downsample(recs, 50, 7)
            print(name, "downsample got", got["downsample"][0][0], "expected", dc)
            assert got["downsample"][0] == (dc, D.names_text(names))
            assert F.read_bam(got["downsample"][1])[1] == exp
            # the intended path: names open at the end and the largest cache are the reference cache's
            pairs, still, hs, peak = K.model(case, "tofastq")
            assert (c["paired"], c["unmatched"], c["max_cached"]) == (len(pairs), len(still), peak)
        else:
            assert got == ref, env   # counts, names and bytes do not depend on tiles or on collisions
    # one member per tile: the header's, every tile's (a tile longer than a member has members without a record start), the end marker's at most
    members = 1 + sum(max(1, -(-len(b"".join(t)) // 60000)) for t in case.tiles)
    assert members <= tiles["1"] <= members + 1 and tiles[""] < tiles["1"], tiles


def test_window_cuts(tmp_path):
    """BamFilter's gather and write_record under windows of one piece: every designed window end lies inside its probe pair (join_cases.window_cut_premises),
    the CG-tag openers (300 operations inline, 65 536 as placeholder with the tag moved to the end) included"""
    case = K.window_cuts_bam()
    kw = case.notes["kw"]
    exp, passed, dropped = F.filter_pairs(case.records, **kw)
    K.window_cut_premises(case, exp)
    path = case.write(str(tmp_path / "in.bam"))
    ref = None
    for env in ({"NGSQC_WRITE_WINDOW_PIECES": "1"}, {"NGSQC_WRITE_WINDOW_PIECES": "1", "NGSQC_TILE_MEMBERS": "1"}, {}):
        o = str(tmp_path / "o.bam")
        h = ngsqc.Handle(path=path)
        try:
            assert with_env(env, lambda: h.filter_pairs(o, **kw)) == (passed, dropped), env
        finally:
            h.close()
        b = open(o, "rb").read()
        if ref is None:
            hdr, out = F.read_bam(b)
            assert hdr == K.header()
            assert len(out) == len(exp) and [i for i in range(len(exp)) if out[i] != exp[i]] == []
            ref = b
        else:
            assert b == ref, env
