"""The model of the depth products (tests/depth_model.py) against what the suite already trusts, without a GPU: the hand-derived vectors of tests/hand_vectors.py,
the oracle on a reference fixture, and its own per-base loop - so that tests/test_gpu_depth_products.py compares the kernels with something that was itself checked."""
import os

import numpy as np
import pytest

import depth_model as M
import hand_vectors as HV
import oracle_lib as O
from conftest import GOLDEN_IN


def _merged(bed):
    """merge(true, true) of a case's BED lines, as regions (1-based closed): what the tools scan"""
    out = []
    for s, e, _ in sorted(bed):
        if out and out[-1][2] >= s:
            out[-1] = (0, out[-1][1], max(out[-1][2], e))
        else:
            out.append((0, s + 1, e))
    return out


@pytest.mark.parametrize("name", list(HV.CASES))
def test_model_gives_the_hand_vectors(name):
    c = HV.CASES[name]
    regs = _merged(c["bed"])
    assert sum(e - s + 1 for _, s, e in regs) == len(c["depth"])
    depths, o = [], 0
    for _, s, e in regs:
        depths.append(np.array(c["depth"][o:o + e - s + 1], dtype=np.int64)); o += e - s + 1
    for ra in (True, False):
        for fn in (M.runs, M.runs_loop):
            got = fn(regs, depths, regs, c["cutoff"], c["is_high"], not ra, [ln for _, ln in HV.REFS])
            assert ["chr1\t%d\t%d" % (s - 1, e) for _, s, e in got] == [ln.rsplit("\t", 1)[0] for ln in HV.expected(name, ra)], (name, ra, fn.__name__)
    # the difference array sums back to the depth, and to 0 behind every region
    run = np.cumsum(M.diff_array(regs, depths).astype(np.int64))
    off = M.slot_offsets(regs)
    for i, d in enumerate(depths):
        assert np.array_equal(run[off[i]:off[i + 1] - 1], d) and run[off[i + 1] - 1] == 0


@pytest.fixture(scope="module")
def close_exons():
    bam, bed = os.path.join(GOLDEN_IN, "close_exons.bam"), os.path.join(GOLDEN_IN, "close_exons.bed")
    ob = O.Bam(bam)
    names = [n for n, _ in ob.refs]
    exp = O.low_high_coverage(ob, bed, 20, 1, 0, is_high=False, random_access=True, tool_merge=1)
    # the merged lines, from the oracle's own BED code
    regs = [(names.index(f[0]), int(f[1]) + 1, int(f[2])) for f in (ln.split("\t") for ln in O.bed_roundtrip(bed, 2).splitlines())]
    assert sum(e - s + 1 for _, s, e in regs) == exp["roi_bases"] == exp["depth"].size
    depths, o = [], 0
    for _, s, e in regs:
        depths.append(exp["depth"][o:o + e - s + 1].astype(np.int64)); o += e - s + 1
    return ob, bed, names, regs, depths


def test_model_gives_the_oracles_runs(close_exons):
    """the oracle's random-access depth fed to the model gives the oracle's output lines, random access and sweep, low and high"""
    ob, bed, names, regs, depths = close_exons
    ref_lens = [ln for _, ln in ob.refs]
    for is_high in (False, True):
        for ra in (True, False):
            exp = O.low_high_coverage(ob, bed, 20, 1, 0, is_high=is_high, random_access=ra, tool_merge=1)
            want = [(f[0], int(f[1]) + 1, int(f[2])) for f in (ln.split("\t") for ln in exp["bed"].splitlines())]
            for fn in (M.runs, M.runs_loop):
                got = fn(regs, depths, regs, 20, is_high, not ra, ref_lens)
                assert M.merge_adjacent([(names[regs[l][0]], s, e) for l, s, e in got]) == want, (is_high, ra, fn.__name__)   # (the oracle's final merge(true, true, true))


def test_model_gives_the_oracles_line_sums(close_exons):
    ob, bed, names, regs, depths = close_exons
    cov, _, _ = O.avg_coverage(ob, bed, merge_bed=False, min_mapq=1, random_access=True)
    lines = [(names.index(f[0]), int(f[1]) + 1, int(f[2])) for f in (ln.split("\t") for ln in O.bed_roundtrip(bed, 0).splitlines())]
    assert M.line_sums(regs, depths, lines) == cov.tolist()


@pytest.mark.parametrize("layout,prof", M.SMALL_CASES)
def test_loop_and_numpy_form_of_runs_agree(layout, prof):
    """on every small case of the GPU test, lines of up to 130 bases"""
    regs, depths, lines = M.case(layout, prof)
    lines = [ln for ln in lines if ln[2] - ln[1] < 130]
    if layout == "many":
        lines = lines[:1500]
    assert len(lines) > 100
    n = 0
    for cutoff in M.CUTOFFS:
        for is_high in (False, True):
            for sat in (False, True):
                a = M.runs(regs, depths, lines, cutoff, is_high, sat, M.REF_LENS)
                assert a == M.runs_loop(regs, depths, lines, cutoff, is_high, sat, M.REF_LENS), (cutoff, is_high, sat)
                n += len(a)
    assert n > 0


def test_reads_for_piles_up_to_the_profile():
    rng = np.random.default_rng(5)
    d = np.concatenate([rng.integers(0, 40, size=200), np.full(50, 300), [299, 301, 0, 0, 7], rng.integers(0, 5, size=100)])
    reads = M.reads_for(d)
    assert reads == sorted(reads, key=lambda r: r[0]) and all(n >= 1 for _, n in reads)
    got = np.zeros(d.size + 1, dtype=np.int64)
    for o, n in reads:
        got[o] += 1; got[o + n] -= 1
    assert np.array_equal(np.cumsum(got)[:-1], d) and o + n <= d.size
