"""The kernels that READ the difference array (K6: the prefix sum of csrc/index.hip, csrc/depth.hip, their wrappers in csrc/jobs.hip) on designed depth profiles.

The scan that writes the array is tested elsewhere; here the array itself is the input. On a small carrier BAM ngsqc_scan_depth_partial lays out the regions,
ngsqc_depth_diff_set overwrites the difference array with tests/depth_model.py's diff_array of a designed profile, ngsqc_depth_finalize runs the prefix sum and marks
the spare slots, and every consumer (ngsqc_depth_copy, ngsqc_depth_stats, ngsqc_region_sums, ngsqc_lowhigh_runs, ngsqc_depth_reduce) is compared with the model, by
integer equality. The profiles hold what reads of ordinary coverage never give: depths of 255 and more, above every histogram cap and above 2^16, steps on lanes 63 and
0 of a 64-base step, line sums above 2^32, depth behind a contig's end; the layouts put region ends on scan tiles and go past every grid cap (256 and 512 scan tiles,
4096 * 256 slots, 4096 regions, 8192 lines). One leg goes through real reads (a pile of 66 000 reads), so that the scan's array and the injected one meet.
(ngsqc_scan_depth_partial takes a whole-file handle: no shard handle is needed.)"""
import ctypes as C

import numpy as np
import pytest

import advbam
import depth_model as M
import oracle_lib as O

pytestmark = pytest.mark.gpu
ngsqc = __import__("importlib").import_module("ngs-bits_amd")
RUN = np.dtype([("line", "<i8"), ("start", "<i4"), ("end", "<i4")])   # ngsqc_run
CAPS = (0, 1, 254, 2499, 16383, 16384, 30000)                         # 16384: the first cap whose bins need more than 64 KB of LDS (launch_depth_hist)


@pytest.fixture(scope="module")
def carrier(tmp_path_factory):
    """three references and a handful of ordinary reads: the injected array replaces whatever they pile up to"""
    path = str(tmp_path_factory.mktemp("carrier") / "carrier.bam")
    recs = [advbam.Record("r%d" % i, 0, tid, pos, [(advbam.M, 50)], "ACGTA" * 10, qual=[30] * 50) for i, (tid, pos) in
            enumerate([(0, 99), (0, 120), (0, 4000), (0, 1_999_900), (1, 0), (1, 240), (2, 10), (2, 49_940)])]
    M.write_bam(path, M.REFS, recs)
    return path


_cases = {}


def _case(layout, prof):
    """(regions, depths, lines) of tests/depth_model.py's case: made once, shared, never written to"""
    if (layout, prof) not in _cases:
        regs, depths, lines = M.case(layout, prof)
        for d in depths:
            d.setflags(write=False)
        _cases[layout, prof] = (regs, depths, lines)
    return _cases[layout, prof]


def _inject(path, regs, depths, finalize=True):
    h = ngsqc.Handle(path=path)
    assert h.refs == M.REFS
    h.scan_depth(regs, partial=True)
    assert h.depth_device()[1] == sum(e - s + 1 for _, s, e in regs) + len(regs)
    h.depth_diff_set(M.diff_array(regs, depths))
    if finalize:
        h.depth_finalize()
    return h


def _runs(h, lines, cutoff, is_high, sat):
    """ngsqc_lowhigh_runs called directly: the count-only call (runs = null) and the writing call report the same number"""
    L = ngsqc.lib()
    la = ngsqc.capi._regions_array(np.asarray(lines, dtype=np.int32)); n = C.c_int64(-1)
    assert L.ngsqc_lowhigh_runs(h.h, C.cast(la, C.c_void_p), len(lines), cutoff, int(is_high), int(sat), None, 0, C.byref(n)) == 0
    counted = n.value
    out = np.zeros(counted + 1, dtype=RUN); n = C.c_int64(-1)
    assert L.ngsqc_lowhigh_runs(h.h, C.cast(la, C.c_void_p), len(lines), cutoff, int(is_high), int(sat), out.ctypes.data, counted, C.byref(n)) == 0
    assert n.value == counted
    return out[:counted].tolist()


ALL_CASES = M.SMALL_CASES + M.LARGE_CASES
NOT_DEEP = [c for c in ALL_CASES if c[0] != "deep"]   # (deep is there for the prefix sum's third trip: test_depth and test_region_sums read it)


def test_the_edges_layout_puts_region_ends_on_scan_tiles():
    regs, _, _ = _case("edges", "steps")
    off = M.slot_offsets(regs)
    spare = off[1:] - 1
    assert (spare % M.SCAN_TILE == M.SCAN_TILE - 1).any() and (off[1:-1] % M.SCAN_TILE == 0).any()
    assert any(e - s + 2 == M.SCAN_TILE and o % M.SCAN_TILE == 0 for (_, s, e), o in zip(regs, off))     # len + 1 == 4096: one region is one tile, its spare slot the last
    assert [e - s + 1 for _, s, e in regs[1:10]] == list(M.EDGE_LENS)
    w, _, lines = _case("wide", "noise")
    assert M.slot_offsets(w)[-1] > M.SCAN_TILE * 256 and len(lines) > 8192
    assert M.slot_offsets(_case("deep", "noise")[0])[-1] > M.SCAN_TILE * 512 and len(_case("many", "steps")[0]) > 4096
    # every value of the steps profile occurs, and steps lie on both ends of a 64-base step
    d = np.concatenate(_case("edges", "steps")[1])
    assert set(M.VALUES) <= set(d.tolist())
    big = _case("edges", "steps")[1][-1]
    assert all(big[o - 1] != big[o] for o in M.OFFSETS[1:] + (big.size - 2, big.size - 1))


@pytest.mark.parametrize("layout,prof", ALL_CASES)
def test_depth(carrier, layout, prof):
    """prefix sum, spare marking and compaction: the depth comes back as designed"""
    regs, depths, _ = _case(layout, prof)
    h = _inject(carrier, regs, depths)
    try:
        want = np.concatenate(depths)
        assert np.array_equal(h.depth(want.size), want)
    finally:
        h.close()


@pytest.mark.parametrize("layout,prof", NOT_DEEP)
def test_depth_stats(carrier, layout, prof):
    regs, depths, _ = _case(layout, prof)
    cat = np.concatenate(depths)
    occurs = int(cat[cat.size // 2])
    h = _inject(carrier, regs, depths)
    try:
        for cap in CAPS:
            for half in (0, 1, occurs, occurs + 1, int(cat.max()) + 1):
                hist, cov = h.depth_stats(cap, half)
                assert np.array_equal(hist, M.hist(depths, cap)), (cap, half)
                assert cov == M.covered(depths, half), (cap, half)
                assert hist.sum() == cat.size                      # the spare slots are not counted
    finally:
        h.close()


@pytest.mark.parametrize("layout,prof", ALL_CASES)
def test_region_sums(carrier, layout, prof):
    regs, depths, lines = _case(layout, prof)
    want = M.line_sums(regs, depths, lines)
    if prof == "noise_big":
        assert want[0] == int(depths[0].sum()) and want[0] > 2 ** 32    # (line 0 is the first region whole)
    h = _inject(carrier, regs, depths)
    try:
        assert h.region_sums(np.asarray(lines, dtype=np.int32), n_lines=len(lines)).tolist() == want
    finally:
        h.close()


@pytest.mark.parametrize("layout,prof", NOT_DEEP)
def test_lowhigh_runs(carrier, layout, prof):
    regs, depths, lines = _case(layout, prof)
    h = _inject(carrier, regs, depths)
    try:
        for cutoff in M.CUTOFFS:
            for is_high in (False, True):
                for sat in (False, True):
                    got = _runs(h, lines, cutoff, is_high, sat)
                    assert got == M.runs(regs, depths, lines, cutoff, is_high, sat, M.REF_LENS), (cutoff, is_high, sat)
                    if cutoff == 255 and sat:     # no position of the sweep reaches 255: nothing is high, everything is low
                        assert got == ([] if is_high else [(i, s, e) for i, (_, s, e) in enumerate(lines)])
                    if cutoff == 0:               # no depth is below 0
                        assert got == ([(i, s, e) for i, (_, s, e) in enumerate(lines)] if is_high else [])
    finally:
        h.close()


def test_depth_behind_the_contigs_end(carrier):
    """chr2 has 300 bases, the region 250..330 holds depth 300 throughout: the sweep reads 0 behind the end, random access what is stored"""
    regs, depths, _ = _case("edges_tail", "tail")
    line = [r for r in regs if r[0] == 1]
    assert line == [(1, 250, 330)] and (depths[regs.index(line[0])] == 300).all()
    h = _inject(carrier, regs, depths)
    try:
        assert h.lowhigh_runs(line, 20, is_high=False, saturate254=True) == [(0, 301, 330)]
        assert h.lowhigh_runs(line, 20, is_high=True, saturate254=True) == [(0, 250, 300)]
        assert h.lowhigh_runs(line, 20, is_high=False, saturate254=False) == []
        assert h.lowhigh_runs(line, 20, is_high=True, saturate254=False) == [(0, 250, 330)]
        assert h.lowhigh_runs([(1, 301, 330), (1, 300, 301)], 255, is_high=True, saturate254=False) == [(0, 301, 330), (1, 300, 301)]
        assert h.region_sums(line).tolist() == [81 * 300]
    finally:
        h.close()


def test_depth_reduce(carrier):
    """two handles, the same regions, two arrays: a += b, then the prefix sum - b's array stays as it was set"""
    regs, da, _ = _case("wide", "noise")
    _, db, _ = _case("wide", "noise_big")
    a = _inject(carrier, regs, da, finalize=False); b = _inject(carrier, regs, db, finalize=False)
    try:
        a.depth_reduce([b])
        assert np.array_equal(b.depth_diff(), M.diff_array(regs, db))
        assert np.array_equal(a.depth_diff(), M.diff_array(regs, [x + y for x, y in zip(da, db)]))
        a.depth_finalize()
        want = np.concatenate(da) + np.concatenate(db)
        assert np.array_equal(a.depth(want.size), want)
        b.depth_finalize()
        assert np.array_equal(b.depth(want.size), np.concatenate(db))
    finally:
        a.close(); b.close()


def test_contract_errors(carrier):
    """each refusal carries the message of csrc/jobs.hip, and the handle goes on working"""
    regs, depths, lines = _case("edges", "steps")
    want = np.concatenate(depths)
    h = _inject(carrier, regs, depths, finalize=False)
    try:
        def refused(msg, f, *a, **kw):
            with pytest.raises(ngsqc.NgsqcError) as e:
                f(*a, **kw)
            assert e.value.message == msg
        refused("no depth array: run ngsqc_scan_depth first", h.lowhigh_runs, lines, 20)
        refused("no depth array: run ngsqc_scan_depth first", h.region_sums, lines)
        refused("no depth array: run ngsqc_scan_mapping / ngsqc_scan_depth first", h.depth, want.size)
        refused("no depth array: run ngsqc_scan_mapping / ngsqc_scan_depth first", h.depth_stats, 10, 1)
        refused("depth buffer size mismatch", h.depth_diff_set, M.diff_array(regs, depths)[:-1])
        assert np.array_equal(h.depth_diff(), M.diff_array(regs, depths))     # (the refused calls changed nothing)
        h.depth_finalize()
        refused("the depth array is already finalized (prefix-summed)", h.depth_diff_set, M.diff_array(regs, depths))
        refused("invalid histogram request", h.depth_stats, -1, 1)
        refused("invalid histogram request", h.depth_stats, 30001, 1)
        t, s, e = regs[2]
        for bad in [(t, s - 1, e), (t, s, e + 1), (t, regs[1][2], s), (2, 50_000, 50_001), (1, 301, 301)]:
            refused("line is not covered by the scanned regions", h.region_sums, [lines[0], bad])
            refused("line is not covered by the scanned regions", h.lowhigh_runs, [bad], 20)
        refused("depth buffer too small", h.depth, want.size - 1)
        assert np.array_equal(h.depth(want.size), want)
        assert h.region_sums(lines).tolist() == M.line_sums(regs, depths, lines)
    finally:
        h.close()


# ---- one leg through real reads ----
PILE_AT = 10_000   # chr3 position of the pile's first base


def _pile():
    """shoulder of 300, 253..257, a plateau of 66 000 over 1000 bases, 257..253: about 66 000 reads"""
    return np.concatenate([np.full(5000, 300), [253, 254, 255, 256, 257], np.full(1000, 66_000), [257, 256, 255, 254, 253]]).astype(np.int64)


@pytest.fixture(scope="module")
def pile(tmp_path_factory):
    d = tmp_path_factory.mktemp("pile")
    path = str(d / "pile.bam")
    prof = _pile()
    recs = M.pile_records(2, PILE_AT, prof)
    assert 60_000 < len(recs) < 80_000
    M.write_bam(path, M.REFS, recs)
    full = np.zeros(M.REF_LENS[2] + 2, dtype=np.int64); full[PILE_AT:PILE_AT + prof.size] = prof   # by 1-based position
    last = PILE_AT + prof.size - 1
    # two touching regions that cut through the plateau (the second ends inside it), and one that the pile overhangs by its last base
    regs = [(2, 9000, 15_500), (2, 15_501, 15_800), (2, last, last + 90)]
    assert full[15_500] == full[15_501] == full[15_800] == full[15_801] == 66_000 and full[last] == 253 and full[last + 1] == 0
    bed = str(d / "pile.bed"); open(bed, "w").write("".join("chr3\t%d\t%d\n" % (s - 1, e) for _, s, e in regs))
    return path, bed, regs, [full[s:e + 1].copy() for _, s, e in regs], len(recs)


def test_the_scan_and_the_injected_array_meet(pile):
    path, bed, regs, depths, n_records = pile
    lines = M.line_set(regs)
    h = ngsqc.Handle(path=path)
    try:
        assert h.n_records == n_records
        h.scan_depth(regs, min_mapq=1, min_baseq=0, partial=True)
        assert np.array_equal(h.depth_diff(), M.diff_array(regs, depths))       # the scan's +1 / -1, the "-1" in the spare slot included
        h.depth_finalize()
        want = np.concatenate(depths)
        assert np.array_equal(h.depth(want.size), want)
        assert h.region_sums(lines).tolist() == M.line_sums(regs, depths, lines)
        ob = O.Bam(path)
        cov, _, _ = O.avg_coverage(ob, bed, merge_bed=False, min_mapq=1, random_access=True)
        assert h.region_sums(regs).tolist() == cov.tolist()
        for is_high in (False, True):
            for ra in (True, False):
                got = _runs(h, lines, 255, is_high, not ra)
                assert got == M.runs(regs, depths, lines, 255, is_high, not ra, M.REF_LENS), (is_high, ra)
                exp = O.low_high_coverage(ob, bed, 255, 1, 0, is_high=is_high, random_access=ra, tool_merge=0)
                assert np.array_equal(exp["depth"], want if ra else np.minimum(want, 254))
                mine = M.merge_adjacent([("chr3", s, e) for _, s, e in _runs(h, regs, 255, is_high, not ra)])
                assert mine == [(f[0], int(f[1]) + 1, int(f[2])) for f in (ln.split("\t") for ln in exp["bed"].splitlines())], (is_high, ra)
    finally:
        h.close()
