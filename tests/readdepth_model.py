"""A plain model of the first half of the depth path: reads -> per-base depth of a set of regions, and the read counts of BedReadCount.

Written from the reference's text, not from oracle/ and not from the kernels:
  BamAlignment::qualities                 src/cppNGS/BamReader.cpp:210-255        (the min_baseq mask)
  WorkerLowOrHighCoverage::run            src/cppNGS/WorkerLowOrHighCoverage.cpp  (filter :47-49, the per-line depth loop)
  WorkerAverageCoverage::run              src/cppNGS/WorkerAverageCoverage.cpp:41-45 (the same filter plus skip_mismapped)
  BedReadCount                            src/BedReadCount/main.cpp:55-66
It works over advbam.Record lists and is a loop per record and per base: slow, and meant to be. Regions are 1-based closed (tid, start, end) tuples, sorted and without
overlap (touching is allowed), as the C ABI takes them; the depth comes back concatenated region by region, as Handle.depth() returns it.

The one place where the model, not the reference, is the judge: a read index at or behind l_seq masks nothing. The reference reads past the qualities there (a mapped
SEQ "*" record with M operations, advbam.SEQ_STAR_OOB); the product documents the clamp (csrc/scan.hip: "a CIGAR longer than SEQ").

The bookkeeping (book=[]: one Entry per record, in the order given) is what the premises of tests/readdepth_cases.py are asserted on."""
import struct

import numpy as np

import advbam as A

LONG_CIGAR = 64   # csrc/common.h: more operations -> the wave-per-record kernel
BQ_CHUNK, BQ_TILE, BQ_BLOCK = 256, 4096, 64   # csrc/scan.hip: records per chunk of baseq_tile_kernel, slots of its LDS tile, list entries per block


class Entry:
    """what the model did with one record"""
    __slots__ = ("k", "passed", "start1", "end1", "regions", "masked", "wave_path")

    def __init__(self, k):
        self.k, self.passed, self.start1, self.end1 = k, False, 0, 0
        self.regions = []      # indices of the overlapped regions
        self.masked = []       # (region index, 1-based position, read index) of every base the mask clears inside a region
        self.wave_path = False  # the library hands the record to its wave-per-record kernel (more than LONG_CIGAR operations, or a possible CG tag)

    @property
    def listed(self):
        """the riding walk puts the record on baseq_tile_kernel's list"""
        return self.passed and bool(self.regions) and not self.wave_path


def coverage_filter(r, min_mapq, skip_mismapped, n_ref):
    f = r.flag
    if f & 0x400 or f & 0x100 or f & 0x800 or f & 0x4 or r.mapq < min_mapq:
        return False
    if skip_mismapped and not f & 0x2 and r.mapq < 20:
        return False
    return 0 <= r.tid < n_ref


def span(r):
    """1-based closed [start, end] of the effective CIGAR (BamReader.h:80-94; a record without reference length covers its start)"""
    ref_len = 0 if r.flag & 4 else sum(ln for op, ln in r.effective_cigar() if op in A.REF_OPS)
    return r.pos + 1, r.pos + max(ref_len, 1)


def masked_bases(r, min_baseq):
    """BamAlignment::qualities, literally: [(offset from the record's start, read index)] of the bases the mask clears. Only M tests qualities; D / N advance the
    genome index, I / S the read index, '=' / 'X' / 'H' / 'P' neither (the reference has no branch for them)."""
    if min_baseq <= 0:
        return []
    l_seq = len(r.seq)
    qual = r.qual if r.qual is not None else [0xff] * l_seq
    out = []
    ai = gi = 0
    for op, ln in r.effective_cigar():
        if op == A.M:
            for _ in range(ln):
                if ai < l_seq and qual[ai] < min_baseq:   # (at or behind l_seq: nothing - the product's clamp)
                    out.append((gi, ai))
                ai += 1
                gi += 1
        elif op in (A.D, A.N):
            gi += ln
        elif op in (A.I, A.S):
            ai += ln
    return out


def slot_offsets(regions):
    """first slot of every region in the difference array (one spare slot behind each region), and the total"""
    off = [0]
    for _, s, e in regions:
        off.append(off[-1] + e - s + 2)
    return off


def _wave_path(r):
    c = r.cigar
    return len(c) > LONG_CIGAR or (len(c) > 0 and r.tid >= 0 and r.pos >= 0 and c[0] == (A.S, len(r.seq)))


def depth_from_reads(records, regions, min_mapq=1, min_baseq=0, skip_mismapped=False, n_ref=len(A.REFS), book=None):
    """per-base depth of the regions (int32, concatenated)"""
    depth = [np.zeros(e - s + 1, dtype=np.int32) for _, s, e in regions]
    for k, r in enumerate(records):
        ent = Entry(k)
        if book is not None:
            book.append(ent)
        if not coverage_filter(r, min_mapq, skip_mismapped, n_ref):
            continue
        ent.passed, ent.wave_path = True, _wave_path(r)
        start1, end1 = span(r)
        ent.start1, ent.end1 = start1, end1
        hit = [i for i, (t, s, e) in enumerate(regions) if t == r.tid and s <= end1 and e >= start1]
        if not hit:
            continue
        ent.regions = hit
        low = {start1 + g: ai for g, ai in masked_bases(r, min_baseq)}
        for i in hit:
            _, s, e = regions[i]
            for p in range(max(start1, s), min(end1, e) + 1):
                if p in low:
                    ent.masked.append((i, p, low[p]))
                else:
                    depth[i][p - s] += 1
    return np.concatenate(depth) if depth else np.zeros(0, dtype=np.int32)


def read_counts(records, regions, min_mapq=1, n_ref=len(A.REFS)):
    """BedReadCount: per region, the reads that are mapped, neither secondary nor supplementary, have MAPQ >= min_mapq and overlap it"""
    out = np.zeros(len(regions), dtype=np.int64)
    for r in records:
        if r.flag & 0x4 or r.flag & 0x100 or r.flag & 0x800 or r.mapq < min_mapq or not 0 <= r.tid < n_ref:
            continue
        start1, end1 = span(r)
        for i, (t, s, e) in enumerate(regions):
            if t == r.tid and s <= end1 and e >= start1:
                out[i] += 1
    return out


# ---- bookkeeping for the premises ----
def chunks(book):
    """the chunks of baseq_tile_kernel: 256 consecutive list records in file order (the radix sort by offset restores file order and puts every hole behind the records)"""
    listed = [e for e in book if e.listed]
    return [listed[i:i + BQ_CHUNK] for i in range(0, len(listed), BQ_CHUNK)]


def chunk_reach(chunk, regions):
    """the farthest masked slot of a chunk, counted from the chunk's lowest slot (the first slot any of its records covers): BQ_TILE and more -> the direct atomics"""
    off = slot_offsets(regions)
    base = min(off[e.regions[0]] + max(e.start1, regions[e.regions[0]][1]) - regions[e.regions[0]][1] for e in chunk)
    far = [off[i] + p - regions[i][1] - base for e in chunk for i, p, _ in e.masked]
    return max(far) if far else -1


def record_from_bytes(raw):
    """a BAM record (block_size included, SAM spec 4.2) as advbam.Record: tests/hand_vectors.py keeps its reads as bytes"""
    tid, pos, l_name, mapq, _, n_cigar, flag, l_seq, mtid, mpos, isize = struct.unpack_from("<iiBBHHHiiii", raw, 4)
    o = 36
    name = raw[o:o + l_name - 1].decode(); o += l_name
    cigar = [(c & 15, c >> 4) for c in struct.unpack_from("<%dI" % n_cigar, raw, o)]; o += 4 * n_cigar
    packed = raw[o:o + (l_seq + 1) // 2]; o += (l_seq + 1) // 2
    seq = "".join("=ACMGRSVTWYHKDBN"[(packed[i >> 1] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq))
    qual = list(raw[o:o + l_seq])
    return A.Record(name, flag, tid, pos, cigar, seq, mapq=mapq, qual=qual, isize=isize, mtid=mtid, mpos=mpos)
