"""The plain model of the depth products (K6, csrc/depth.hip and the prefix sum of csrc/index.hip): numpy and Python only, no GPU, no library.

The world is a list of merged, sorted regions (tid, start, end), 1-based closed as ngsqc_region, and per region an int64 array of its per-base depth. From these:
  diff_array   the int32 difference array in the library's slot layout (csrc/jobs.hip setup_regions): what ngsqc_depth_diff_set takes
  hist/covered the depth histogram and the half-depth count (depth_hist_kernel)
  line_sums    the sum of depth over each line (line_sums_kernel)
  runs         the runs of `depth >= cutoff` / `depth < cutoff` inside each line (the contract above line_runs_kernel), once as a per-base loop - the definition -
               and once in numpy for the large cases; tests/test_cpu_depth_model.py holds the two equal
  reads_for    mapped reads whose pile-up is a designed depth profile, and write_bam to put them (or anything else) into a BAM with a reference list of one's own
tests/test_gpu_depth_products.py injects diff_array through the C ABI and compares every product with this model, by integer equality."""
import numpy as np

import advbam
import cram_twin

VALUES = (0, 1, 19, 20, 21, 253, 254, 255, 256, 65535, 65536, 2_000_000)   # the depths of the `steps` profile: the cutoffs' neighbours, the sweep's 254, 2^16, a value no cap holds
OFFSETS = (0, 1, 62, 63, 64, 65, 127, 128)                                 # piece boundaries of `steps` (plus len - 2, len - 1): the lanes at both ends of a 64-base step


# ---- the slot layout ----
def diff_array(regions, depths):
    """region i owns len_i + 1 slots: depth[0], depth[j] - depth[j - 1], and the spare slot -depth[len - 1] (the running sum is 0 again at the next region)"""
    out = []
    for (tid, s, e), d in zip(regions, depths):
        d = np.asarray(d, dtype=np.int64)
        assert d.shape == (e - s + 1,) and d.min() >= 0
        x = np.empty(d.size + 1, dtype=np.int64)
        x[0] = d[0]; x[1:-1] = d[1:] - d[:-1]; x[-1] = -d[-1]
        out.append(x)
    x = np.concatenate(out)
    assert np.abs(x).max() < 2 ** 31
    return x.astype(np.int32)


def slot_offsets(regions):
    """first slot of every region (and, last, the number of slots)"""
    return np.concatenate([[0], np.cumsum([e - s + 2 for _, s, e in regions])]).astype(np.int64)


# ---- histogram ----
def hist(depths, cap):
    d = np.concatenate([np.asarray(x, dtype=np.int64) for x in depths])
    return np.bincount(np.minimum(d, cap), minlength=cap + 1).astype(np.int64)


def covered(depths, half):
    return sum(int((np.asarray(x, dtype=np.int64) >= half).sum()) for x in depths)


# ---- lines ----
def _locate(regions, lines):
    """per line: (index of the region that holds it, offset of its first base in that region)"""
    key = lambda t, s: (int(t) << 32) + int(s)
    rk = np.array([key(t, s) for t, s, _ in regions], dtype=np.int64)
    assert (np.diff(rk) > 0).all()
    ln = np.asarray(lines, dtype=np.int64).reshape(-1, 3)
    ri = np.searchsorted(rk, (ln[:, 0] << 32) + ln[:, 1], side="right") - 1
    rg = np.asarray(regions, dtype=np.int64).reshape(-1, 3)
    assert (ri >= 0).all() and (rg[ri, 0] == ln[:, 0]).all() and (rg[ri, 1] <= ln[:, 1]).all() and (ln[:, 2] <= rg[ri, 2]).all() and (ln[:, 1] <= ln[:, 2]).all()
    return ri, ln[:, 1] - rg[ri, 1]


def line_sums(regions, depths, lines):
    ri, off = _locate(regions, lines)
    return [int(np.asarray(depths[r][o:o + e - s + 1], dtype=np.int64).sum()) for (_, s, e), r, o in zip(lines, ri.tolist(), off.tolist())]   # (int64 holds 2^31 bases of depth 2^31)


def runs_loop(regions, depths, lines, cutoff, is_high, saturate254, ref_lens):
    """the definition: base by base. saturate254 is the sweep (an unsigned char per position of the contig that stops at 254, 0 behind the contig's end)"""
    ri, off = _locate(regions, lines)
    out = []
    for li, ((tid, s, e), r, o) in enumerate(zip(lines, ri.tolist(), off.tolist())):
        first = None
        for p in range(s, e + 1):
            v = int(depths[r][o + p - s])
            if saturate254:
                if p > ref_lens[tid]:
                    v = 0
                if v > 254:
                    v = 254
            hit = v >= cutoff if is_high else v < cutoff
            if hit and first is None:
                first = p
            if not hit and first is not None:
                out.append((li, first, p - 1)); first = None
        if first is not None:
            out.append((li, first, e))   # a run never leaves its line
    return out


def runs(regions, depths, lines, cutoff, is_high, saturate254, ref_lens):
    """the same in numpy: the predicate once per base of the regions, then every line's bases gathered side by side"""
    cat = np.concatenate([np.asarray(x, dtype=np.int64) for x in depths])
    base = np.concatenate([[0], np.cumsum([e - s + 1 for _, s, e in regions])]).astype(np.int64)
    if saturate254:
        pos = np.concatenate([np.arange(s, e + 1, dtype=np.int64) for _, s, e in regions])
        end = np.concatenate([np.full(e - s + 1, ref_lens[t], dtype=np.int64) for t, s, e in regions])
        cat = np.minimum(np.where(pos > end, 0, cat), 254)
    hit_all = cat >= cutoff if is_high else cat < cutoff
    ri, off = _locate(regions, lines)
    ln = np.asarray(lines, dtype=np.int64).reshape(-1, 3)
    n = ln[:, 2] - ln[:, 1] + 1
    at = np.concatenate([[0], np.cumsum(n)])             # where each line's bases begin in the gathered array
    k = np.arange(at[-1], dtype=np.int64)
    line_of = np.repeat(np.arange(len(ln), dtype=np.int64), n)
    j = k - at[line_of]                                   # offset inside the line
    hit = hit_all[(base[ri] + off)[line_of] + j]
    prev = np.concatenate([[False], hit[:-1]]) & (j > 0)
    nxt = np.concatenate([hit[1:], [False]]) & (j < n[line_of] - 1)
    st, en = hit & ~prev, hit & ~nxt
    p = ln[line_of, 1] + j
    return list(zip(line_of[st].tolist(), p[st].tolist(), p[en].tolist()))


def merge_adjacent(rows):
    """BedFile::merge(true, true, true) on runs given as (chromosome, start, end), 1-based closed: sorted, then touching and overlapping runs joined"""
    out = []
    for c, s, e in sorted(rows):
        if out and out[-1][0] == c and out[-1][2] + 1 >= s:
            out[-1] = (c, out[-1][1], max(out[-1][2], e))
        else:
            out.append((c, s, e))
    return out


# ---- profiles ----
def steps(rng, n, extra=0):
    """piecewise constant over n bases, values from VALUES, a boundary at every offset of OFFSETS and at n - 2, n - 1 that lies inside (plus `extra` random ones);
    neighbouring pieces differ, so every boundary is a step"""
    cuts = sorted({o for o in OFFSETS + (n - 2, n - 1) if 0 < o < n} | {int(x) for x in rng.integers(1, max(n, 2), size=extra) if 0 < x < n})
    d = np.empty(n, dtype=np.int64)
    last = None
    for a, b in zip([0] + cuts, cuts + [n]):
        v = VALUES[int(rng.integers(len(VALUES)))]
        while v == last:
            v = VALUES[int(rng.integers(len(VALUES)))]
        d[a:b] = v; last = v
    return d


def comb(n, cutoff, shift):
    """every other base at the cutoff, the rest one below"""
    return (cutoff - ((np.arange(n, dtype=np.int64) + shift) & 1)).astype(np.int64)


# ---- the designed cases of tests/test_gpu_depth_products.py (here, so that the CPU test can hold the two forms of runs() equal on the same profiles) ----
REFS = [("chr1", 2_000_000), ("chr2", 300), ("chr3", 50_000)]   # the carrier BAM's references
REF_LENS = [ln for _, ln in REFS]
CUTOFFS = (0, 1, 20, 254, 255)
SCAN_TILE = 4096                                                # slots per workgroup of the prefix sum (csrc/index.hip SCAN_TILE)
EDGE_LENS = (1, 2, 63, 64, 65, 4095, 4096, 4097, 8191)


def layout_edges(tail=False):
    """chr1: a first region whose length is nudged until the 4095-base region fills one scan tile with its spare slot as the tile's last, then regions of EDGE_LENS
    bases, 7 bases apart; chr2 whole (tail: 250..330, 30 bases behind the contig's end); chr3 whole"""
    for nudge in range(1, SCAN_TILE + 1):
        regs, p = [], 100
        for n in (nudge,) + EDGE_LENS:
            regs.append((0, p, p + n - 1)); p += n + 7
        off = slot_offsets(regs)
        if off[1 + EDGE_LENS.index(4095)] % SCAN_TILE == 0:
            break
    return regs + [(1, 250, 330) if tail else (1, 1, 300), (2, 1, 50_000)]


def layout_wide():
    """more than 256 scan tiles, more than 4096 * 256 slots; a short region behind it"""
    n = SCAN_TILE * 257 + 3
    return [(0, 11, 10 + n), (0, 10 + n + 5, 10 + n + 9)]


def layout_deep():
    """more than 512 scan tiles: the third trip of scan_tile_prefix's loop, the first that reads the carry the second trip left (the region runs past chr1's end)"""
    return [(0, 1, SCAN_TILE * 513), (2, 7, 11)]


def layout_many(rng):
    """4100 regions of 1 to 3 bases, 1 to 3 bases apart"""
    regs, p = [], 5
    for n, gap in zip(rng.integers(1, 4, size=4100).tolist(), rng.integers(1, 4, size=4100).tolist()):
        regs.append((0, p, p + n - 1)); p += n + gap
    return regs


def line_set(regions, rng=None, n_random=0):
    """every region whole, its first and its last base, lines of 1 / 63 / 64 / 65 / 129 bases at offsets 0, 1, 63, 64, nested lines and a duplicate; n_random lines of
    1 to 130 bases anywhere in the first region. In no particular order."""
    out = []
    for t, s, e in regions:
        out += [(t, s, e), (t, s, s), (t, e, e)]
        for n in (1, 63, 64, 65, 129):
            out += [(t, s + o, s + o + n - 1) for o in (0, 1, 63, 64) if s + o + n - 1 <= e]
        if e - s >= 130:
            out += [(t, s + 10, s + 120), (t, s + 20, s + 70), (t, s + 20, s + 70), (t, s + 64, s + 127)]
    if n_random:
        t, s, e = regions[0]
        a = rng.integers(s, e - 130, size=n_random); n = rng.integers(1, 131, size=n_random)
        out += [(t, int(x), int(x + k - 1)) for x, k in zip(a, n)]
    return out


def profile(name, regions, rng):
    """one depth array per region. steps | comb<cutoff> (the regions take turns with the pattern and the pattern shifted by a base) | flat<depth> |
    tail (steps, and depth 300 on the whole chr2 region) | noise (uniform in [0, 600)) | noise_big (noise, the first region's first 5000 bases uniform in [0, 3 000 000))"""
    lens = [e - s + 1 for _, s, e in regions]
    if name in ("steps", "tail"):
        d = [steps(rng, n, extra=20 if n > 1000 else 0) for n in lens]
        if name == "tail":
            d = [np.full(n, 300, dtype=np.int64) if t == 1 else x for (t, _, _), n, x in zip(regions, lens, d)]
        return d
    if name.startswith("comb"):
        return [comb(n, int(name[4:]), i & 1) for i, n in enumerate(lens)]
    if name.startswith("flat"):
        return [np.full(n, int(name[4:]), dtype=np.int64) for n in lens]
    d = [rng.integers(0, 600, size=n, dtype=np.int64) for n in lens]
    if name == "noise_big":
        d[0][:5000] = rng.integers(0, 3_000_000, size=5000, dtype=np.int64)
    else:
        assert name == "noise"
    return d


# (layout, profile) pairs: the small ones run every product and the loop form of runs(); wide and deep are for the GPU test alone
SMALL_CASES = [("edges", p) for p in ("steps", "comb1", "comb20", "comb254", "comb255", "flat0", "flat20", "flat300")] + [("edges_tail", "tail"), ("many", "steps"), ("many", "comb20")]
LARGE_CASES = [("wide", "noise"), ("wide", "noise_big"), ("wide", "flat300"), ("deep", "noise")]


def case(layout, prof, seed=20240607):
    """-> (regions, depths, lines) of a case, the same on every call"""
    rng = np.random.default_rng([seed, sum(map(ord, layout + prof))])
    regions = {"edges": layout_edges, "edges_tail": lambda: layout_edges(True), "wide": layout_wide, "deep": layout_deep, "many": lambda: layout_many(rng)}[layout]()
    depths = profile(prof, regions, rng)
    lines = line_set(regions, rng, 9000 if layout == "wide" else 0)
    return regions, depths, lines


# ---- reads ----
def reads_for(depth):
    """(offset, ref_len) of reads, sorted by offset, that pile up to `depth` (depth 0 outside): the rises of the profile open reads, the falls close them, first in
    first out, so the k-th read opened is the k-th closed"""
    d = np.concatenate([[0], np.asarray(depth, dtype=np.int64), [0]])
    step = np.diff(d)                                    # step[j]: depth[j] - depth[j - 1], step[n]: the fall to 0 behind the end
    idx = np.arange(step.size, dtype=np.int64)
    starts = np.repeat(idx, np.maximum(step, 0)); ends = np.repeat(idx, np.maximum(-step, 0))
    assert starts.size == ends.size and (ends > starts).all()
    return list(zip(starts.tolist(), (ends - starts).tolist()))


def write_bam(path, refs, records):
    """records: advbam.Record, coordinate-sorted by the caller"""
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs)
    for r in records:
        assert 0 <= r.tid < len(refs)
    cram_twin.write_bam(path, text, refs, [r.bytes() for r in records])


def pile_records(tid, pos1, depth):
    """the reads of reads_for as mapped records without SEQ (`*`, l_seq = 0), CIGAR <ref_len>M, MAPQ 60; pos1: 1-based position of depth[0]"""
    return [advbam.Record("p", 0, tid, pos1 - 1 + o, [(advbam.M, n)], "", mapq=60) for o, n in reads_for(depth)]
