"""A plain model of the site pileup and the indel windows (ngsqc_site_pileup / ngsqc_indel_windows / ngsqc_variant_details: pileup_kernel and pileup_long_kernel
of csrc/scan.hip, indel_kernel and indel_long_kernel of csrc/indel.hip).

Written from the reference's text, not from oracle/ and not from the kernels:
  BamReader::getPileup                    src/cppNGS/BamReader.cpp:809-885   (the read filters :829-836, SNP counts only)
  BamAlignment::extractBaseByCIGAR        src/cppNGS/BamReader.cpp:307-374   (the walk; cigarIsOnlyInsertion :90-100 looks at the core CIGAR)
  BamReader::getIndels                    src/cppNGS/BamReader.cpp:948-1125  (through tests/variant_oracle.py, which restates it and is left as it is)
It works over advbam.Record lists in file order, one record and one site or window at a time: slow, and meant to be. The records are read back from their bytes
by variant_oracle.reads, so the CIGAR is the CG-tag array exactly where htslib would take it (variant_oracle._cg_tag), whatever advbam believes.

Where the reference throws, the library's convention stands: a site gets a count in column 7 ("Unknown CIGAR operation", "Could not find position"), a window a
count in column 6 (the call then fails with a FormatError). A letter Pileup::inc would throw on is a count in column 6 of the site. The one place where the model,
not the reference, is the judge: a read index at or behind l_seq (a CIGAR longer than SEQ) - the reference reads past the record there, the library counts column 7.
A base quality is the raw byte (0xff stays 255), a deleted base has quality 255, and both are tested against min_baseq as they are.

The bookkeeping (book=[]: one Entry per record and site / window it meets) is what the premises of tests/pileup_cases.py are asserted on."""
import numpy as np

import advbam as A
import variant_oracle as V

LONG_CIGAR = 64           # csrc/common.h: more operations -> the wave-per-record kernels
PILEUP_BUCKET_SHIFT = 16  # csrc/postable.h: 64 kb buckets of the site and window tables (the table itself on the CPU: test_cpu_postable.py)
N_SITE_COLS, N_WIN_COLS = 8, 7
COL = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
W_MAPPED, W_MAPQ0, W_DEPTH, W_INS, W_DEL, W_MATCH, W_UNKNOWN = range(7)


class Entry:
    """what the model did with one record at one site (kind "site") or window (kind "win")"""
    __slots__ = ("kind", "k", "i", "branch", "op_index", "n_ops", "col", "ap", "events")

    def __init__(self, kind, k, i, branch, op_index=-1, n_ops=0, col=-1, ap=-1, events=()):
        self.kind, self.k, self.i, self.branch, self.op_index, self.n_ops, self.col, self.ap, self.events = kind, k, i, branch, op_index, n_ops, col, ap, list(events)

    @property
    def long(self):
        return self.n_ops > LONG_CIGAR


class _Image:
    """the records as variant_oracle.reads takes them: one inflated image and the offsets in it"""

    def __init__(self, records):
        raw = [r.bytes() for r in records]
        self._img = np.frombuffer(b"".join(raw) or b"\0", dtype=np.uint8)
        self._offs = np.cumsum([0] + [len(b) for b in raw])[:-1]

    def inflated(self):
        return self._img

    def record_offsets(self):
        return self._offs


def reads(records):
    """variant_oracle.Read per record, in the order given (the effective CIGAR in .cigar)"""
    return V.reads(_Image(records)) if records else []


def site_filter(rd, min_mapq, include_npp, n_ref):
    """BamReader.cpp:829-836, and a reference id the header has"""
    if rd.flag & (0x100 | 0x800 | 0x400 | 0x4):
        return False
    if not rd.flag & 0x2 and not include_npp:
        return False
    return rd.mapq >= min_mapq and 0 <= rd.tid < n_ref


def extract_base(rd, core_cigar, pos):
    """extractBaseByCIGAR: (branch, operation index, column or -1, quality, read index). Branches: only_ins, del, skip, softclip, base, other (a letter outside
    ACGTN), seq_oob (the model's clamp), unknown, notfound"""
    if all(op in (A.I, A.S) for op, _ in core_cigar):
        return "only_ins", -1, -1, -1, -1
    read_pos, genome_pos = 0, rd.start - 1
    for k, (op, ln) in enumerate(rd.cigar):
        if op in (A.M, A.EQ, A.X):
            genome_pos += ln; read_pos += ln
        elif op == A.I:
            read_pos += ln
        elif op == A.D:
            genome_pos += ln
            if genome_pos >= pos:
                return "del", k, 5, 255, -1
        elif op == A.N:
            genome_pos += ln
            if genome_pos >= pos:
                return "skip", k, -1, -1, -1
        elif op == A.S:
            read_pos += ln
            if read_pos >= rd.l_seq:
                return "softclip", k, -1, -1, -1
        elif op == A.H:
            pass
        else:
            return "unknown", k, 7, -1, -1
        if genome_pos >= pos:
            ap = read_pos - (genome_pos + 1 - pos)
            if ap < 0 or ap >= rd.l_seq:
                return "seq_oob", k, 7, -1, ap
            nib = (int(rd._img[rd._seq_off + (ap >> 1)]) >> (4 * (1 - (ap & 1)))) & 15
            q = int(rd._img[rd._seq_off + (rd.l_seq + 1) // 2 + ap])
            ch = V.SEQ_CODES[nib]
            return ("base", k, COL[ch], q, ap) if ch in COL else ("other", k, 6, q, ap)
    return "notfound", len(rd.cigar), 7, -1, -1


def site_counts(records, sites, min_mapq=1, min_baseq=13, include_npp=False, n_ref=len(A.REFS), book=None):
    """int64[n, 8]: A, C, G, T, N, deletion, other letter, thrown. sites: (tid, 1-based position) rows; a row given twice gets its counts twice"""
    out = np.zeros((len(sites), N_SITE_COLS), dtype=np.int64)
    by_tid = {}
    for i, (t, p) in enumerate(sites):
        by_tid.setdefault(t, []).append((p, i))
    for k, (r, rd) in enumerate(zip(records, reads(records))):
        if not site_filter(rd, min_mapq, include_npp, n_ref):
            continue
        for p, i in by_tid.get(rd.tid, ()):
            if not (rd.start - 1 < p and rd.end > p - 1):      # htslib: pos < site and bam_endpos > site - 1
                continue
            branch, op_index, col, q, ap = extract_base(rd, r.cigar, p)
            if col == 7 or (col >= 0 and q >= min_baseq):
                out[i, col] += 1
            if book is not None:
                book.append(Entry("site", k, i, branch, op_index, len(rd.cigar), col, ap))
    return out


def _walk_events(rd, start, end):
    """the I / D / N operations of a spanning read as getIndels sees them: (operation index, op, genome position, read position, counted)"""
    ev, gp, rp = [], rd.start, 0
    for k, (op, ln) in enumerate(rd.cigar):
        if op == A.I or op == A.D:
            ev.append((k, op, gp, rp, start <= gp <= end))
        elif op == A.N:
            ev.append((k, op, gp, rp, gp <= start and gp + ln >= end))
        if op in V.REF_OPS:
            gp += ln
        if op in (A.M, A.I, A.S, A.EQ, A.X):
            rp += ln
    return ev


def window_counts(records, windows, include_npp=False, ref_seq=None, book=None):
    """int64[n, 7]: the six NGSQC_W_* counters and the "unknown" flag (the reference's throw: the other six columns of such a row are 0).
    windows: (tid, start, end, kind, allele, ...) rows; ref_seq(tid, pos1, length) = FastaFileIndex::seq"""
    rds = reads(records)
    index = V.Index(rds)
    order = {id(rd): k for k, rd in enumerate(rds)}
    out = np.zeros((len(windows), N_WIN_COLS), dtype=np.int64)
    for i, w in enumerate(windows):
        tid, start, end, kind, allele = w[:5]
        allele = allele.decode("latin-1") if isinstance(allele, bytes) else (allele or "")
        try:
            out[i, :6] = V.window_counts(index, ref_seq, tid, start, end, kind, allele, include_npp)
        except ValueError:
            out[i, W_UNKNOWN] = 1
        if book is not None:
            for rd in index.region(tid, start, end):
                n = len(rd.cigar)
                if rd.flag & (0x400 | 0x100 | 0x800 | 0x4) or (not rd.flag & 0x2 and not include_npp):
                    branch, ev = "filtered", ()
                elif rd.mapq == 0:
                    branch, ev = "mapq0", ()
                elif rd.start > start or rd.end < end:
                    branch, ev = "not_spanning", ()
                elif not any(op in (A.I, A.D, A.N) for op, _ in rd.cigar):
                    branch, ev = "no_idn", ()
                else:
                    ev = _walk_events(rd, start, end)
                    branch = "unknown" if any(op == A.P or op > 8 for op, _ in rd.cigar) else "walked"
                book.append(Entry("win", order[id(rd)], i, branch, n_ops=n, events=ev))
    return out
