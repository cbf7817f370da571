"""A plain model of MappingQC's three record loops over advbam.Record lists on advbam.REFS: every counter, the insert-size bins, the per-base depth and the
exact GC read fractions.

Written loop by loop from the reference's text, not from oracle/ and not from the kernels:
  Statistics::mapping(bed..)   src/cppNGS/Statistics.cpp:416-574     (ROI)
  Statistics::mapping(bam..)   src/cppNGS/Statistics.cpp:830-917     (NOROI)
  Statistics::mapping_wgs      src/cppNGS/Statistics.cpp:1068-1183   (WGS: the loop over the file, then one indexed pass per target region)
  Statistics::yxRatio          src/cppNGS/Statistics.cpp:2659-2691   (two indexed passes)
  ChromosomalIndex::matchingIndices: the lines of a chromosome with line.start <= end and line.end >= start
  an index query chr:start-end (BamReader::setRegion): the records of that reference with pos < end and bam_endpos > start - 1
It is a loop per record and per region, and a loop per base for the depth: slow, and meant to be. Regions and GC chunks are 1-based closed (tid, start, end)
tuples as the C ABI takes them; the depth comes back concatenated region by region, as Handle.depth() returns it; gc_reads are fractions.Fraction, one per bin
0..100: the value the reference's sum of doubles approximates.

Where the reference is undefined the oracle's documented choice is the contract (advbam's domain): a mapped record with a negative tid is on no chromosome
(never near a target, a special contig). Two inputs stay outside: a negative DP tag (it indexes bases_usable_dp out of range) and isize == INT32_MIN (abs()).

Rules: the reference's constants and comparisons, each of which a named variant (VARIANTS) gets wrong by one. tests/test_cpu_mapping_model.py shows that the designed
reads of tests/mapping_cases.py tell every variant from the model - the evidence that they would catch a kernel that is wrong in the same way.

The bookkeeping (book=[]: one Entry per record, in the order given) is what the premises of tests/mapping_cases.py are asserted on."""
import math
import struct
from fractions import Fraction

import numpy as np

import advbam as A

MODE_ROI, MODE_NOROI, MODE_WGS = 0, 1, 2
LONG_CIGAR = 64   # csrc/common.h: more operations -> the wave-per-record kernel
GC_NMAX = 64      # csrc/common.h: chunk counts below it are summed as integers, the others as doubles
N_BINS = 101
COUNTERS = ("al_total", "al_mapped", "al_ontarget", "al_neartarget", "al_dup", "al_proper_paired", "insert_size_read_count", "bases_trimmed", "bases_mapped",
            "bases_clipped", "insert_size_sum", "bases_usable", "bases_usable_no_overlap", "bases_usable_raw", "bases_usable_roi", "bases_usable_dp0",
            "bases_usable_dp1", "bases_usable_dp2", "bases_usable_dp3", "bases_usable_dp4", "dp_dist0", "dp_dist1", "dp_dist2", "dp_dist3", "max_length",
            "paired_end", "roi_bases", "reads_x", "reads_y", "yx_valid")


class Rules:
    """the reference's figures; a variant changes one of them"""
    near = 250            # Statistics.cpp:458
    strict = frozenset()  # comparisons of a region search taken as '<' where the reference has '<=': "<site>_lo" (line.end >= start), "<site>_hi" (line.start <= end)
    hist_bound = 1000     # :555 insert_size < 1000
    ovl_shift = 0         # :502 / :506 read_overlap_start
    ovl_from_span = False  # :494-502 al.length() is l_seq, not the reference span
    gc_binned_only = False  # :539 indices.count() counts the chunks without a bin too
    wgs_gc_once = False   # :1154-1173 a read is met once per target region it overlaps
    gc_lost_n = None      # (a product-side table of GC_NMAX columns: a read of that many chunks written to or read from a column that is not there)
    x_len_shift = 0       # index query: pos < len
    x_end_min = 0         # index query: endpos > 0
    dp_clamp = 4          # :472 / :483 std::min(dp, 4)

    def __init__(self, **kw):
        for k, v in kw.items():
            assert hasattr(Rules, k), k
            setattr(self, k, v)


REFERENCE = Rules()
SITES = ("near", "on", "ovl", "gc", "wgs")   # the region searches: near window, on target, read-overlap window, GC chunks, the indexed pass of mapping_wgs
VARIANTS = dict(
    [("near_249", Rules(near=249)), ("near_251", Rules(near=251))]
    + [("%s_%s_strict" % (s, side), Rules(strict=frozenset(["%s_%s" % (s, side)]))) for s in SITES for side in ("lo", "hi")]
    + [("hist_999", Rules(hist_bound=999)), ("hist_1001", Rules(hist_bound=1001)),
       ("ovl_start_minus1", Rules(ovl_shift=-1)), ("ovl_start_plus1", Rules(ovl_shift=1)), ("ovl_from_span", Rules(ovl_from_span=True)),
       ("gc_n_binned_only", Rules(gc_binned_only=True)), ("wgs_gc_once", Rules(wgs_gc_once=True)),
       ("gc_table_63", Rules(gc_lost_n=GC_NMAX - 1)), ("gc_table_65", Rules(gc_lost_n=GC_NMAX)),
       ("x_len_minus1", Rules(x_len_shift=-1)), ("x_len_plus1", Rules(x_len_shift=1)), ("x_end_min_minus1", Rules(x_end_min=-1)), ("x_end_min_plus1", Rules(x_end_min=1)),
       ("dp_clamp_3", Rules(dp_clamp=3)), ("dp_clamp_5", Rules(dp_clamp=5))])


class Entry:
    """what the model did with one record"""
    __slots__ = ("k", "counted", "start1", "end1", "near", "on_target", "regions", "usable", "gc_n", "gc_hits", "window", "window_regions", "ins_bin", "wave_path")

    def __init__(self, k):
        self.k, self.counted, self.start1, self.end1, self.near, self.on_target = k, False, 0, 0, False, False
        self.regions = []          # indices of the regions the read overlaps (ROI: on-target search; WGS: the indexed passes that met it)
        self.usable = False        # passed !duplicate && mapq >= min_mapq on a target
        self.gc_n = 0              # chunks the read overlaps, those without a bin included (0: no GC hit was made)
        self.gc_hits = 0           # how often the read was added to gc_reads (WGS: once per region)
        self.window = None         # (start, end) of the read-overlap window, ROI mode
        self.window_regions = []   # the regions the window was taken off
        self.ins_bin = None        # the insert-size bin the record was counted in
        self.wave_path = False     # the library hands the record to its wave-per-record kernel


class Result:
    def __init__(self, counters, hist, depth, gc_reads, half_depth, bases_covered_half):
        self.counters, self.hist, self.depth, self.gc_reads, self.half_depth, self.bases_covered_half = counters, hist, depth, gc_reads, half_depth, bases_covered_half

    def __getitem__(self, name):
        return self.counters[name]

    def outputs(self):
        """everything a comparison looks at, in one comparable value"""
        return (tuple(self.counters[n] for n in COUNTERS), tuple(self.hist), self.depth.tobytes(), tuple(self.gc_reads), self.half_depth, self.bases_covered_half)


def wave_path(r):
    """csrc/scan.hip scan_record: more than LONG_CIGAR operations, or a first operation that may be the placeholder of a CG:B,I tag"""
    c = r.cigar
    return len(c) > LONG_CIGAR or (len(c) > 0 and r.tid >= 0 and r.pos >= 0 and c[0] == (A.S, len(r.seq)))


def tag_int(aux, tag):
    """BamAlignment::tagi / bam_aux2i: the first tag of that name as an integer; 0 if it is absent or not of an integer type"""
    size = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4, "d": 8}
    fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}
    o = 0
    while o + 3 <= len(aux):
        name, t = aux[o:o + 2], chr(aux[o + 2]); o += 3
        if t in ("Z", "H"):
            n = aux.index(b"\0", o) - o + 1
        elif t == "B":
            n = 5 + size[chr(aux[o])] * struct.unpack_from("<I", aux, o + 1)[0]
        else:
            n = size[t]
        if name == tag:
            return struct.unpack_from(fmt[t], aux, o)[0] if t in fmt else 0
        o += n
    return 0


def span(r):
    """al.start(), al.end(): 1-based closed, bam_endpos of the effective CIGAR (an unmapped record, a record without reference length: its start)"""
    ref_len = 0 if r.flag & 4 else sum(ln for op, ln in r.effective_cigar() if op in A.REF_OPS)
    return r.pos + 1, r.pos + max(ref_len, 1)


def matching(table, tid, start, end, rules, site):
    """ChromosomalIndex::matchingIndices(chr, start, end) on a table of (tid, start, end) lines, ascending"""
    lo, hi = site + "_lo" in rules.strict, site + "_hi" in rules.strict
    out = []
    for i, (t, s, e) in enumerate(table):
        if t != tid:
            continue
        if (e > start if lo else e >= start) and (s < end if hi else s <= end):
            out.append(i)
    return out


def c_round(x):
    """std::round: halves away from zero"""
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def mapping(records, mode, regions=(), gc_chunks=(), gc_bins=(), min_mapq=1, tid_x=-1, tid_y=-1, nonspecial=None, refs=A.REFS, rules=REFERENCE, book=None):
    """records in file order -> Result. regions: of the mode (none in MODE_NOROI); gc_bins: -1 or 0..100 per chunk"""
    assert mode in (MODE_ROI, MODE_NOROI, MODE_WGS) and len(gc_chunks) == len(gc_bins) and all(-1 <= b <= 100 for b in gc_bins)
    if mode == MODE_NOROI:
        regions, gc_chunks, gc_bins = (), (), ()
    regions = list(regions)
    n_ref = len(refs)
    c = dict.fromkeys(COUNTERS, 0)
    hist = [0] * 1000
    dp_bases = [0] * (max(rules.dp_clamp, 4) + 1)
    depth = [np.zeros(e - s + 1, dtype=np.int32) for _, s, e in regions]
    gc_reads = [Fraction(0)] * N_BINS
    entries = [Entry(k) for k in range(len(records))]
    if book is not None:
        book.extend(entries)

    def gc_hit(ent, tid, start, end):
        ind = matching(gc_chunks, tid, start, end, rules, "gc")
        n = sum(1 for i in ind if gc_bins[i] >= 0) if rules.gc_binned_only else len(ind)
        ent.gc_n = len(ind)
        if ind:
            ent.gc_hits += 1
        for i in ind:
            if gc_bins[i] >= 0 and n != rules.gc_lost_n:
                gc_reads[gc_bins[i]] += Fraction(1, n)

    # ---- the loop over the file ----
    max_length, paired_end = 0, False
    for ent, r in zip(entries, records):
        f = r.flag
        ent.wave_path = wave_path(r)
        ent.start1, ent.end1 = span(r)
        if f & 0x100 or f & 0x800:
            continue
        ent.counted = True
        c["al_total"] += 1
        if f & 0x1:
            paired_end = True
        length = len(r.seq)
        max_length = max(max_length, length)
        spliced = False
        dup, passing = bool(f & 0x400), r.mapq >= min_mapq
        if not f & 0x4:
            c["al_mapped"] += 1
            start_pos, end_pos = ent.start1, ent.end1
            c["bases_mapped"] += length
            for op, ln in r.effective_cigar():
                if op in (A.S, A.H):
                    c["bases_clipped"] += ln
                elif op == A.N:
                    spliced = True
            on_chrom = 0 <= r.tid < n_ref
            if mode == MODE_ROI:
                if on_chrom and matching(regions, r.tid, start_pos - rules.near, end_pos + rules.near, rules, "near"):
                    c["al_neartarget"] += 1
                    ent.near = True
                    indices = matching(regions, r.tid, start_pos, end_pos, rules, "on")
                    if indices:
                        c["al_ontarget"] += 1
                        ent.on_target, ent.regions = True, indices
                        dp = tag_int(r.aux, b"DP")
                        assert dp >= 0, "a negative DP tag is outside the reference's domain"
                        if dp != 0:
                            c["dp_dist%d" % (min(min(dp, rules.dp_clamp), 4) - 1)] += 1   # Histogram(0.5, 4.5, 1): the bin of 4 holds what lies above it
                        if not dup and passing:
                            ent.usable = True
                            for i in indices:
                                _, s, e = regions[i]
                                ol_start, ol_end = max(s, start_pos), min(e, end_pos)
                                n = ol_end - ol_start + 1
                                c["bases_usable"] += n
                                dp_bases[min(dp, rules.dp_clamp)] += n
                                c["bases_usable_raw"] += n * (dp + 1)
                                for p in range(ol_start, ol_end + 1):
                                    depth[i][p - s] += 1
                                c["bases_usable_no_overlap"] += n
                            insert_size = abs(r.isize)
                            ln2 = end_pos - start_pos + 1 if rules.ovl_from_span else length
                            if f & 0x40 and f & 0x1 and f & 0x2 and not spliced and 2 * ln2 > insert_size:
                                overlap = 2 * ln2 - insert_size
                                o_start = (start_pos + ln2 - overlap if r.isize > 0 else start_pos) + rules.ovl_shift
                                o_end = o_start + overlap - 1
                                ent.window = (o_start, o_end)
                                for i in matching(regions, r.tid, o_start, o_end, rules, "ovl"):
                                    _, s, e = regions[i]
                                    c["bases_usable_no_overlap"] -= min(e, o_end) - max(s, o_start) + 1
                                    ent.window_regions.append(i)
                        gc_hit(ent, r.tid, start_pos, end_pos)
            else:
                if on_chrom and nonspecial[r.tid]:
                    c["al_ontarget"] += 1
                    ent.on_target = True
                    if not dup and passing:
                        ent.usable = True
                        c["bases_usable"] += length
                        if paired_end:
                            c["bases_usable_no_overlap"] += length
        if f & 0x1 and f & 0x2:
            c["al_proper_paired"] += 1
            if not spliced:
                insert_size = abs(r.isize)
                if insert_size < rules.hist_bound:
                    c["insert_size_read_count"] += 1
                    c["insert_size_sum"] += insert_size
                    if insert_size < 1000:
                        hist[insert_size] += 1
                    ent.ins_bin = insert_size
                    if mode != MODE_ROI and f & 0x40 and not dup and passing and 2 * length > insert_size:
                        c["bases_usable_no_overlap"] -= 2 * length - insert_size
        if length < max_length:
            c["bases_trimmed"] += max_length - length
        if dup:
            c["al_dup"] += 1
    if mode != MODE_ROI:
        c["bases_usable"] -= c["bases_clipped"]
    c["max_length"], c["paired_end"] = max_length, int(paired_end)

    # ---- mapping_wgs: one indexed pass per target region ----
    if mode == MODE_WGS:
        seen = set()
        for i, (t, s, e) in enumerate(regions):
            for ent, r in zip(entries, records):
                if r.tid != t or not (ent.end1 > s if "wgs_lo" in rules.strict else ent.end1 >= s) or not (ent.start1 < e if "wgs_hi" in rules.strict else ent.start1 <= e):
                    continue
                if r.flag & 0x100 or r.flag & 0x800 or r.flag & 0x4:
                    continue
                ent.regions.append(i)
                if not (rules.wgs_gc_once and ent.k in seen):
                    gc_hit(ent, r.tid, ent.start1, ent.end1)
                seen.add(ent.k)
                if not r.flag & 0x400 and r.mapq >= min_mapq:
                    ent.usable = True
                    c["bases_usable_roi"] += len(r.seq)
                    for p in range(max(ent.start1, s), min(ent.end1, e) + 1):
                        depth[i][p - s] += 1

    # ---- yxRatio: two indexed passes over the whole of chrY and chrX ----
    if 0 <= tid_x < n_ref and 0 <= tid_y < n_ref:
        for name, t in (("reads_y", tid_y), ("reads_x", tid_x)):
            for ent, r in zip(entries, records):
                if r.tid == t and r.pos < refs[t][1] + rules.x_len_shift and ent.end1 > rules.x_end_min and not (r.flag & 0x100 or r.flag & 0x800):
                    c[name] += 1
        c["yx_valid"] = int(c["reads_x"] != 0)

    for i in range(5):
        c["bases_usable_dp%d" % i] = dp_bases[i]
    c["roi_bases"] = sum(e - s + 1 for _, s, e in regions)
    d = np.concatenate(depth) if depth else np.zeros(0, dtype=np.int32)
    half = covered = 0
    if c["roi_bases"]:
        half = c_round(0.5 * ((c["bases_usable"] if mode == MODE_ROI else c["bases_usable_roi"]) / c["roi_bases"]))   # :607-608 / :1186-1187
        covered = int((d >= half).sum())
    return Result(c, hist, d, gc_reads, half, covered)
