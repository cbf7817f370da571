"""The MappingQC record loops (csrc/scan.hip classify<MODE_ROI / MODE_NOROI / MODE_WGS>) on designed reads and target regions: Handle.scan_mapping against the plain model
of tests/mapping_model.py, case by case of tests/mapping_cases.py - every counter, the 1000 insert-size bins, the per-base depth, depth_stats and gc_reads. Integers by
equality. gc_reads: a bin fed only by reads over 1, 2, 4 .. 128 chunks is a sum of exactly representable terms and must equal the model's fraction exactly, whatever
the order of the atomics; a bin that also holds a read over 63 or 65 chunks gets the project's rtol = 1e-12. tests/test_cpu_mapping_model.py holds the model to the
oracle, to the hand vectors and to the cases' premises, and shows that the cases tell the model from each of its off-by-one variants.

classify is called from three kernels, reached through the library's path switches: walk_scan_kernel (default: the scan rides the chain walk), scan_kernel (a resident
tile, NGSQC_NO_FUSED_SCAN, NGSQC_K2_GENERAL, small tiles, shards) and scan_long_kernel (the records of 65 operations and the CG records on every path, every record
under NGSQC_LONG_READ_MODE). One handle per case and path serves all modes and parameter sets: the call switches are read at every entry point."""
from fractions import Fraction

import numpy as np
import pytest

import advbam as A
import hostprep as H
import mapping_cases as MC
import mapping_model as MM
import oracle_lib as O

pytestmark = pytest.mark.gpu
ngsqc = __import__("importlib").import_module("ngs-bits_amd")

PATHS = {"default": {}, "resident": {}, "no_fused_scan": {"NGSQC_NO_FUSED_SCAN": "1"}, "k2_general": {"NGSQC_K2_GENERAL": "1"}, "tiles3k": {"NGSQC_TILE_MEMBERS": "1"},
         "long_read": {"NGSQC_LONG_READ_MODE": "1"}, "shards3": {}}
SMALL_MEMBERS = (3000, 2900, 3100)
MODE_OF = {MM.MODE_ROI: ngsqc.MODE_ROI, MM.MODE_NOROI: ngsqc.MODE_NOROI, MM.MODE_WGS: ngsqc.MODE_WGS}
JOB_CASES = {MM.MODE_ROI: "overlap_window", MM.MODE_NOROI: "insert_sizes", MM.MODE_WGS: "gc_counts"}
HIST0 = 32              # counters[32:]: the insert-size bins
POW2 = {1, 2, 4, 8, 16, 32, 64, 128}
COUNTER_INDEX = {n: O.COUNTER_NAMES.index(n) for n in MM.COUNTERS}   # (half_depth and bases_covered_half: compared through depth_stats)

_bams, _wants, _dirs = {}, {}, {}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    if "d" not in _dirs:
        _dirs["d"] = str(tmp_path_factory.mktemp("mapping"))
    return _dirs["d"]


@pytest.fixture(scope="module")
def bam(workdir):
    """path of a case's file: members of whole records in the case's own sizes, as htslib writes them (the scan rides the chain walk), or the stream cut every 3 KB or
    so, records across the cuts (the general path). Written once"""
    def get(name, small=False):
        if (name, small) not in _bams:
            p = "%s/%s_%d.bam" % (workdir, name, small)
            MC.case(name).write(p, member_sizes=SMALL_MEMBERS if small else None, whole_records=not small)
            _bams[name, small] = p
        return _bams[name, small]
    return get


def bin_sets(c, mode, workdir):
    """[(what, the bins the library gets, the bins the model gets)]: the sparse FASTA's and, where the case has them, the hand-set ones"""
    if mode == MM.MODE_NOROI:
        return [("none", None, None)]
    fb = c.fasta_bins(mode, workdir)
    return [("fasta", fb, fb)] + ([("hand",) + c.bins(mode)] if c.hand_bins else [])


def want(c, mode, mq, yx, what, bins):
    """the model's result and its book: computed once, shared, never written to"""
    k = (c.name, mode, mq, yx, what)
    if k not in _wants:
        book = []
        r = c.run(mode, mq, yx, bins=bins, book=book)
        r.depth.setflags(write=False)
        _wants[k] = (r, book)
    return _wants[k]


def exact_bins(records, chunks, book, bins):
    """the bins whose reads all overlap a power-of-two number of chunks"""
    ns = {}
    for e in book:
        if e.gc_hits:
            r = records[e.k]
            for i, (t, s, en) in enumerate(chunks):
                if t == r.tid and s <= e.end1 and en >= e.start1 and bins[i] >= 0:
                    ns.setdefault(bins[i], set()).add(e.gc_n)
    return {b for b, n in ns.items() if n <= POW2}, ns


def check(what, counters, gc_reads, h, exp, records, chunks, mode, book, bins):
    for n, i in COUNTER_INDEX.items():
        assert int(counters[i]) == exp[n], (what, n, int(counters[i]), exp[n])
    bad = np.nonzero(np.asarray(counters[HIST0:]) != np.asarray(exp.hist))[0]
    assert bad.size == 0, (what, "insert-size bins", [(int(i), int(counters[HIST0 + i]), exp.hist[i]) for i in bad[:5]])
    if mode == MM.MODE_NOROI:
        assert not np.any(gc_reads), (what, "gc_reads")
        return
    roi_bases = exp["roi_bases"]
    got = h.depth(roi_bases)
    bad = np.nonzero(got != exp.depth)[0]
    assert bad.size == 0, (what, "per-base depth", int(bad.size), int(bad[0]), int(got[bad[0]]), int(exp.depth[bad[0]]))
    hist, cov = h.depth_stats(2499, exp.half_depth)
    assert np.array_equal(hist, np.bincount(np.minimum(exp.depth, 2499), minlength=2500)) and cov == exp.bases_covered_half, (what, "depth_stats", cov, exp.bases_covered_half)
    exact, ns = exact_bins(records, chunks, book, bins)
    for b in range(MM.N_BINS):
        w = float(exp.gc_reads[b])
        if b in exact or not exp.gc_reads[b]:
            assert Fraction(w) == exp.gc_reads[b] and gc_reads[b] == w, (what, "gc_reads, exact", b, gc_reads[b], w, sorted(ns.get(b, ())))
        else:
            assert abs(gc_reads[b] - w) <= 1e-12 * abs(w), (what, "gc_reads", b, gc_reads[b], w, sorted(ns.get(b, ())))
    return exact


def params_of(c, mode, mq, yx, bins):
    regs, chunks = c.tables(mode)
    tx, ty = H.xy_tids(A.REFS)
    return dict(regions=regs or None, min_mapq=mq, tid_x=tx, tid_y=ty if yx == "xy" else -1, nonspecial=H.nonspecial(A.REFS),
                gc_chunks=chunks if bins is not None else None, gc_bin=bins)


def open_handles(path, n_shards):
    return [ngsqc.Handle(path=path, shard=(i, n_shards)) for i in range(n_shards)] if n_shards > 1 else [ngsqc.Handle(path=path)]


def scan(hs, path, mode, kw):
    if path != "resident":
        for h in hs:
            h.drop_decoded()
    if len(hs) > 1:
        counters, gc_reads, _ = ngsqc.scan_mapping_sharded_local(hs, MODE_OF[mode], **kw)
    else:
        counters, gc_reads = hs[0].scan_mapping(MODE_OF[mode], **kw)
    tm = hs[0].timings()
    if path == "default":
        assert tm["tiles_scan_fused"] == tm["n_tiles"] >= 1, (tm["tiles_scan_fused"], tm["n_tiles"])   # the scan rode the walk
    if path == "no_fused_scan":
        assert tm["tiles_scan_fused"] == 0
    if path == "tiles3k":
        assert tm["n_tiles"] > 1
    return counters, gc_reads


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", MC.NAMES)
def test_mapping_equals_model(bam, workdir, name, path, monkeypatch):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    c = MC.case(name)
    small = path in ("tiles3k", "shards3")
    hs = open_handles(bam(name, small), 3 if path == "shards3" else 1)
    n_exact = n_fed = 0
    try:
        for mode in MC.MODES:
            for what, lib_bins, model_bins in bin_sets(c, mode, workdir):
                for mq, yx in c.params:
                    exp, book = want(c, mode, mq, yx, what, model_bins)
                    counters, gc_reads = scan(hs, path, mode, params_of(c, mode, mq, yx, lib_bins))
                    exact = check((name, path, mode, mq, yx, what), counters, gc_reads, hs[0], exp, c.records, c.tables(mode)[1], mode, book, model_bins)
                    n_exact += len(exact or ())
                    n_fed += sum(1 for x in exp.gc_reads if x)
        assert sum(h.n_records for h in hs) == len(c.records)
        assert n_fed > 0 and (name != "gc_counts" or 0 < n_exact < n_fed)     # gc_counts: bins of both kinds
    finally:
        for h in hs:
            h.close()


@pytest.mark.parametrize("mode", list(JOB_CASES), ids=["roi", "noroi", "wgs"])
def test_mapping_beside_a_depth_scan(bam, workdir, mode):
    """ngsqc_run_job: the mapping scan (depth set 0) with a depth scan over other regions (set 1) in one pass equals the single-purpose calls and the model"""
    c = MC.case(JOB_CASES[mode])
    what, lib_bins, model_bins = bin_sets(c, mode, workdir)[-1]
    mq, yx = c.params[-1]
    exp, book = want(c, mode, mq, yx, what, model_bins)
    dregs = [(A.T1, 900, 3100), (A.T1, 9000, 11000), (A.TX, 1, 2000)]
    h, h2 = ngsqc.Handle(path=bam(c.name)), ngsqc.Handle(path=bam(c.name))
    try:
        kw = params_of(c, mode, mq, yx, lib_bins)
        job = h.run_job(mapping=dict(kw, mode=MODE_OF[mode]), depth=dict(regions=dregs, min_mapq=mq, min_baseq=0))
        h.depth_select(0)
        check((c.name, "job", mode), job["counters"], job["gc_reads"], h, exp, c.records, c.tables(mode)[1], mode, book, model_bins)
        n = sum(e - s + 1 for _, s, e in dregs)
        h2.scan_depth(dregs, min_mapq=mq, min_baseq=0)
        alone = h2.depth(n)
        h.depth_select(1)
        assert np.array_equal(h.depth(n), alone) and alone.sum() > 0
        counters, gc_reads = h2.scan_mapping(MODE_OF[mode], **kw)
        assert np.array_equal(job["counters"], counters)
        check((c.name, "alone", mode), counters, gc_reads, h2, exp, c.records, c.tables(mode)[1], mode, book, model_bins)   # (gc_reads: both against the model - the doubles of 64 chunks and more are summed in any order)
    finally:
        h.close(); h2.close()


@pytest.mark.parametrize("path", [p for p in PATHS if p != "shards3"])
def test_isize_int32_min_is_a_huge_insert(workdir, path, monkeypatch):
    """The one record outside the reference's domain (abs(INT32_MIN) is undefined there): the product counts it as an insert of INT32_MAX - 1000 or more, no mate
    overlap (csrc/scan.hip abs_isize) - so no insert-size bin, count or sum moves, and every other counter is what the model gives with INT32_MAX in its place."""
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    c = MC.case("insert_sizes")
    g = MC.guarded_record()
    stand_in = MC.rec(g.name, g.pos, g.cigar, flag=g.flag, isize=2 ** 31 - 1)
    with_stand_in = sorted(c.records + [stand_in], key=MC.key)
    small = path == "tiles3k"
    p = "%s/int32min_%d.bam" % (workdir, small)
    c.write(p, member_sizes=SMALL_MEMBERS if small else None, whole_records=not small, records=sorted(c.records + [g], key=MC.key))
    h = ngsqc.Handle(path=p)
    try:
        for mode in MC.MODES:
            what, lib_bins, model_bins = bin_sets(c, mode, workdir)[0]
            without, _ = want(c, mode, 1, "xy", what, model_bins)
            book = []
            exp = c.run(mode, 1, bins=model_bins, records=with_stand_in, book=book)
            assert exp.hist == without.hist and all(exp[n] == without[n] for n in ("insert_size_read_count", "insert_size_sum")) and exp["al_total"] == without["al_total"] + 1
            counters, gc_reads = scan([h], path, mode, params_of(c, mode, 1, "xy", lib_bins))
            check((path, mode, "INT32_MIN"), counters, gc_reads, h, exp, with_stand_in, c.tables(mode)[1], mode, book, model_bins)
    finally:
        h.close()
