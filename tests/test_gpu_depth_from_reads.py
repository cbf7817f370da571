"""The first half of the depth path - reads to the difference array - on designed reads: Handle.scan_depth followed by Handle.depth against the plain model of
tests/readdepth_model.py, case by case of tests/readdepth_cases.py (qualities 0..255 under thresholds 1..1000, read positions and region edges on both sides of every
mask-word edge, CIGAR shapes around load_cigar4 and LONG_CIGAR, a pile, chunks that do and do not leave the LDS tile, sparse appends, the moves of the per-lane region
cache on a sorted and an unsorted file, every filter), by integer equality. tests/test_cpu_readdepth_model.py holds the model to the oracle, to the hand vectors and to
the cases' premises; tests/test_gpu_depth_products.py tests what reads the array.

The three implementations of BamAlignment::qualities (csrc/scan.hip) are reached through the library's path switches: baseq_tile_kernel behind the riding list
(default), baseq_decrements (NGSQC_BASEQ_RIDE=0, NGSQC_NO_FUSED_SCAN, a list that overflows under NGSQC_BQ_LIST_CAP), the mask loop of scan_long_kernel (the records of
65 operations and the CG records of cigar_shapes, on every path). One handle serves all parameter sets of a case: the call switches are read at every entry point.
A single-tile file stays decoded and indexed on its handle, and a later scan then runs a thread per record without any walk: Handle.drop_decoded() in front of a scan
makes it walk again. The path "resident" leaves that out - its first scan rides, the others meet the resident tile."""
import numpy as np
import pytest

import advbam as A
import hostprep as H
import oracle_lib as O
import readdepth_cases as RC
import readdepth_model as RM

pytestmark = pytest.mark.gpu
ngsqc = __import__("importlib").import_module("ngs-bits_amd")

PATHS = {"default": {}, "baseq_ride0": {"NGSQC_BASEQ_RIDE": "0"}, "no_fused_scan": {"NGSQC_NO_FUSED_SCAN": "1"}, "k2_general": {"NGSQC_K2_GENERAL": "1"},
         "tiles3k": {"NGSQC_TILE_MEMBERS": "1"}, "shards3": {}, "resident": {}}
SMALL_MEMBERS = (3000, 2900, 3100)
CAP_CASES = ("spill", "sparse_appends", "pile")
COUNT_CASES = ("region_cuts", "cache_moves", "cache_moves_unsorted", "filters")
SKIP_COUNTERS = {"half_depth", "bases_covered_half"}   # (ngsqc_depth_stats: compared through depth_stats)

_bams, _wants = {}, {}


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    """path of a case's file: members of whole records in the case's own sizes, as htslib writes them (the depth scan rides the chain walk), or the stream cut every
    3 KB or so, records across the cuts, as tests/test_gpu_adversarial.py does (the general path). Written once"""
    d = tmp_path_factory.mktemp("readdepth")

    def get(name, small=False):
        if (name, small) not in _bams:
            p = str(d / ("%s_%d.bam" % (name, small)))
            RC.case(name).write(p, member_sizes=SMALL_MEMBERS if small else None, whole_records=not small)
            _bams[name, small] = p
        return _bams[name, small]
    return get


def want(name, mq, bq, skip):
    """the model's depth: computed once, shared, never written to"""
    if (name, mq, bq, skip) not in _wants:
        c = RC.case(name)
        d = RM.depth_from_reads(c.records, c.regions, mq, bq, skip)
        d.setflags(write=False)
        _wants[name, mq, bq, skip] = d
    return _wants[name, mq, bq, skip]


def _mismatch(got, exp, regions):
    """the first position that differs, for the message"""
    bad = np.nonzero(got != exp)[0]
    if bad.size == 0:
        return None
    off = np.cumsum([0] + [e - s + 1 for _, s, e in regions])
    i = int(np.searchsorted(off, bad[0], side="right") - 1)
    return dict(n_bad=int(bad.size), region=regions[i], pos=int(regions[i][1] + bad[0] - off[i]), got=int(got[bad[0]]), expected=int(exp[bad[0]]))


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", RC.NAMES)
def test_depth_equals_model(bam, name, path, monkeypatch):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    c = RC.case(name)
    small = path in ("tiles3k", "shards3")
    n_shards = 3 if path == "shards3" else 1
    hs = [ngsqc.Handle(path=bam(name, small), shard=(i, n_shards)) for i in range(n_shards)] if n_shards > 1 else [ngsqc.Handle(path=bam(name, small))]
    try:
        for mq, bq, skip in c.params:
            exp = want(name, mq, bq, skip)
            if path != "resident":
                for h in hs:
                    h.drop_decoded()
            if n_shards > 1:
                ngsqc.scan_depth_sharded_local(hs, c.regions, min_mapq=mq, min_baseq=bq, skip_mismapped=skip)
            else:
                hs[0].scan_depth(c.regions, min_mapq=mq, min_baseq=bq, skip_mismapped=skip)
            got = hs[0].depth(exp.size)
            assert np.array_equal(got, exp), (mq, bq, skip, _mismatch(got, exp, c.regions))
            tm = hs[0].timings()
            if path == "default" and bq > 0:
                assert tm["tiles_scan_fused"] == tm["n_tiles"] >= 1, (mq, bq, tm["tiles_scan_fused"], tm["n_tiles"])   # the riding list, not a fallback
            if path == "no_fused_scan" or (path == "baseq_ride0" and bq > 0):   # (without min_baseq there is no list: NGSQC_BASEQ_RIDE changes nothing)
                assert tm["tiles_scan_fused"] == 0
            if path == "tiles3k":
                assert tm["n_tiles"] > 1
        assert any(want(name, *p).sum() > 0 for p in c.params)
        assert sum(h.n_records for h in hs) == len(c.records)
    finally:
        for h in hs:
            h.close()


@pytest.mark.parametrize("name", CAP_CASES)
def test_list_that_overflows(bam, name, monkeypatch):
    """NGSQC_BQ_LIST_CAP at the list's exact need, one block below it and at 1: the same depth whether the list holds or the tile is taken back and scanned record by
    record. The need is a whole number of blocks of 64 and is the library's own verdict (timings() does not report the count): the smallest cap under which the scan
    still rides, found by bisection - the need does not depend on the cap, the walk counts every block it asks for. The model bounds it from below: every list record
    takes a slot. Every probe of the search is compared with the model as well."""
    c = RC.case(name)
    mq, bq, skip = c.params[0]
    exp = want(name, mq, bq, skip)
    n_list = sum(e.listed for e in c.book(mq, bq, skip))
    lo = -(-n_list // RM.BQ_BLOCK)          # blocks: a lower bound of the need
    h = ngsqc.Handle(path=bam(name))
    try:
        def rides(blocks_or_cap, as_blocks=True):
            monkeypatch.setenv("NGSQC_BQ_LIST_CAP", str(blocks_or_cap * RM.BQ_BLOCK if as_blocks else blocks_or_cap))
            h.drop_decoded()
            h.scan_depth(c.regions, min_mapq=mq, min_baseq=bq, skip_mismapped=skip)
            got = h.depth(exp.size)
            assert np.array_equal(got, exp), (blocks_or_cap, as_blocks, _mismatch(got, exp, c.regions))
            tm = h.timings()
            return tm["tiles_scan_fused"] == tm["n_tiles"]
        assert lo >= 2 and not rides(lo - 1)                      # fewer slots than records: it must overflow
        hi = lo
        while not rides(hi):
            hi *= 2
            assert hi <= 64 * lo
        a, b = lo - 1, hi                                          # a overflows, b rides
        while b - a > 1:
            m = (a + b) // 2
            if rides(m):
                b = m
            else:
                a = m
        need = b
        assert rides(need) and not rides(need - 1) and not rides(1, as_blocks=False)
        assert need >= lo
    finally:
        h.close()


def test_depth_beside_a_mapping_scan(bam):
    """ngsqc_run_job: the depth scan as depth set 1 beside a WGS mapping scan over the same regions (set 0)"""
    name = "region_cuts"
    c = RC.case(name)
    tx, ty = H.xy_tids(A.REFS)
    h = ngsqc.Handle(path=bam(name))
    try:
        for mq, bq, skip in c.params:
            mp = dict(mode=ngsqc.MODE_WGS, regions=c.regions, min_mapq=1, tid_x=tx, tid_y=ty, nonspecial=H.nonspecial(A.REFS))
            h.drop_decoded()
            h.run_job(mapping=mp, depth=dict(regions=c.regions, min_mapq=mq, min_baseq=bq, skip_mismapped=skip))
            exp = want(name, mq, bq, skip)
            h.depth_select(1)
            got = h.depth(exp.size)
            assert np.array_equal(got, exp), (mq, bq, _mismatch(got, exp, c.regions))
            h.depth_select(0)
            assert np.array_equal(h.depth(exp.size), want(name, 1, 0, False))    # (these reads pass the ROI pass's filter and the coverage filter alike)
    finally:
        h.close()


@pytest.mark.parametrize("name", COUNT_CASES)
def test_region_read_counts(bam, name):
    """BedReadCount (MODE_COUNT): the same region search, without the cache"""
    c = RC.case(name)
    h = ngsqc.Handle(path=bam(name))
    try:
        for mq in (0, 1, 20):
            exp = RM.read_counts(c.records, c.regions, mq)
            assert h.region_read_counts(c.regions, mq).tolist() == exp.tolist(), mq
            assert exp.sum() > 0
    finally:
        h.close()


@pytest.mark.parametrize("name", ("cache_moves", "region_cuts"))
def test_wgs_roi_pass_shares_the_cache(bam, name, tmp_path):
    """scan_mapping(MODE_WGS, regions=...): the fused ROI pass searches with the same per-lane cache - every counter and the per-base depth against the oracle"""
    c = RC.case(name)
    bed = str(tmp_path / "roi.bed")
    open(bed, "w").write(c.bed())
    tx, ty = H.xy_tids(A.REFS)
    h = ngsqc.Handle(path=bam(name))
    try:
        for mq in (1, A.MIN_MAPQ):
            counters, _ = h.scan_mapping(ngsqc.MODE_WGS, regions=c.regions, min_mapq=mq, tid_x=tx, tid_y=ty, nonspecial=H.nonspecial(A.REFS))
            exp = O.mapping(O.Bam(bam(name)), O.MODE_WGS, bed, merge_bed=False, min_mapq=mq)
            for i, cname in enumerate(O.COUNTER_NAMES):
                if cname not in SKIP_COUNTERS:
                    assert int(counters[i]) == int(exp.counters[i]), (mq, cname, int(counters[i]), int(exp.counters[i]))
            assert np.array_equal(counters[32:], exp.counters[32:]), (mq, "insert-size histogram")
            roi_bases = int(counters[O.COUNTER_NAMES.index("roi_bases")])
            assert roi_bases == sum(e - s + 1 for _, s, e in c.regions)
            got = h.depth(roi_bases)
            assert np.array_equal(got, exp.depth), (mq, _mismatch(got, exp.depth, c.regions))
            assert exp["bases_usable_roi"] > 0
    finally:
        h.close()
