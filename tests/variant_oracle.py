"""BamReader::getIndels / getVariantDetails (src/cppNGS/BamReader.cpp:888-1125) restated over the records of oracle_lib.Bam: the checker of the indel
windows (ngsqc_indel_windows / ngsqc_variant_details). Plain Python, one record at a time, as the reference reads them."""
import bisect

import numpy as np

SEQ_CODES = "=ACMGRSVTWYHKDBN"
REF_OPS = (0, 2, 3, 7, 8)    # M D N = X consume the reference (bam_cigar2rlen)


class Read:
    __slots__ = ("tid", "start", "end", "mapq", "flag", "cigar", "_img", "_seq_off", "l_seq")

    def bases(self):
        """al.bases(): SEQ decoded"""
        a = self._img[self._seq_off:self._seq_off + (self.l_seq + 1) // 2]
        return "".join(SEQ_CODES[(a[i >> 1] >> (4 * (1 - (i & 1)))) & 15] for i in range(self.l_seq))


def _u32(a, o):
    return int(a[o]) | int(a[o + 1]) << 8 | int(a[o + 2]) << 16 | int(a[o + 3]) << 24


def _i32(a, o):
    v = _u32(a, o)
    return v - (1 << 32) if v >= 1 << 31 else v


def _cg_tag(img, aux, end, n_cig):
    """the payload of a CG:B,I tag with n_cig <= n < 2^29 entries (htslib bam_tag2cigar, the oracle's parse_rec), or None"""
    p = aux
    sizes = {ord("A"): 1, ord("c"): 1, ord("C"): 1, ord("s"): 2, ord("S"): 2, ord("i"): 4, ord("I"): 4, ord("f"): 4, ord("d"): 8}
    while p + 3 <= end:
        tag, t = bytes(img[p:p + 2]), int(img[p + 2])
        if tag == b"CG":
            if t == ord("B") and int(img[p + 3]) == ord("I"):
                n = _u32(img, p + 4)
                if n < n_cig or n >= 1 << 29:
                    return None
                return [(_u32(img, p + 8 + 4 * k) & 15, _u32(img, p + 8 + 4 * k) >> 4) for k in range(n)]
            return None
        if t in sizes:
            p += 3 + sizes[t]
        elif t in (ord("Z"), ord("H")):
            q = p + 3
            while q < end and img[q]:
                q += 1
            p = q + 1
        elif t == ord("B"):
            st, n = chr(img[p + 3]), _u32(img, p + 4)
            p += 8 + n * (1 if st in "cC" else 2 if st in "sS" else 4)
        else:
            return None
    return None


def reads(bam):
    """every record of the BAM in file order"""
    img, offs = bam.inflated(), bam.record_offsets()
    out = []
    for o in offs:
        o = int(o)
        bs, tid, pos = _u32(img, o), _i32(img, o + 4), _i32(img, o + 8)
        l_name, mapq = int(img[o + 12]), int(img[o + 13])
        n_cig, flag = int(img[o + 16]) | int(img[o + 17]) << 8, int(img[o + 18]) | int(img[o + 19]) << 8
        l_seq = _i32(img, o + 20)
        c0 = o + 36 + l_name
        cigar = [(_u32(img, c0 + 4 * k) & 15, _u32(img, c0 + 4 * k) >> 4) for k in range(n_cig)]
        seq_off = c0 + 4 * n_cig
        if n_cig and tid >= 0 and pos >= 0 and cigar[0] == (4, l_seq):
            cg = _cg_tag(img, seq_off + (l_seq + 1) // 2 + l_seq, o + 4 + bs, n_cig)
            if cg is not None:
                cigar = cg
        r = Read()
        rlen = 0 if flag & 0x4 else sum(n for op, n in cigar if op in REF_OPS)
        r.tid, r.start, r.end, r.mapq, r.flag, r.cigar = tid, pos + 1, pos + max(rlen, 1), mapq, flag, cigar   # al.start(), al.end() = bam_endpos
        r._img, r._seq_off, r.l_seq = img, seq_off, l_seq
        out.append(r)
    return out


class Index:
    """the reads of each reference sorted by start: what an indexed region query (BamReader::setRegion) returns"""

    def __init__(self, rds):
        self.by_tid = {}
        for r in rds:
            if r.tid >= 0:
                self.by_tid.setdefault(r.tid, []).append(r)
        self.starts, self.maxlen = {}, {}
        for t, lst in self.by_tid.items():
            lst.sort(key=lambda r: r.start)
            self.starts[t] = [r.start for r in lst]
            self.maxlen[t] = max(r.end - r.start + 1 for r in lst)

    def region(self, tid, start, end):
        """records overlapping [start, end] (1-based; htslib: pos < end and bam_endpos > start - 1)"""
        if tid not in self.by_tid:
            return []
        lst, st = self.by_tid[tid], self.starts[tid]
        lo = bisect.bisect_left(st, start - self.maxlen[tid])
        hi = bisect.bisect_right(st, end)
        return [r for r in lst[lo:hi] if r.start <= end and r.end >= start]


def get_indels(index, ref_seq, tid, start, end, include_npp=False):
    """BamReader::getIndels (:948-1125, count_fragments = false). ref_seq(tid, pos1, length) = FastaFileIndex::seq. Returns (indels, depth, reads_mapped,
    reads_mapq0)."""
    indels, depth, mapped, mapq0 = [], 0, 0, 0
    for al in index.region(tid, start, end):
        if al.flag & 0x400:                                  # :970
            continue
        if not (al.flag & 0x2) and not include_npp:          # :971
            continue
        if al.flag & (0x100 | 0x800):                        # :972
            continue
        if al.flag & 0x4:                                    # :973
            continue
        mapped += 1
        if al.mapq == 0:                                     # :976-980
            mapq0 += 1
            continue
        if al.start > start or al.end < end:                 # :984
            continue
        depth += 1
        if not any(op in (1, 2, 3) for op, _ in al.cigar):   # :990-1003
            continue
        read_pos, genome_pos = 0, al.start
        bases = None
        for op, n in al.cigar:                               # :1034-1086
            if op in (0, 7, 8):
                genome_pos += n; read_pos += n
            elif op == 1:
                if start <= genome_pos <= end:
                    if bases is None:
                        bases = al.bases()
                    indels.append("+" + bases[read_pos:read_pos + n])
                read_pos += n
            elif op == 2:
                if start <= genome_pos <= end:
                    indels.append("-" + ref_seq(tid, genome_pos, n))
                genome_pos += n
            elif op == 3:
                if genome_pos <= start and genome_pos + n >= end:
                    depth -= 1
                genome_pos += n
            elif op == 4:
                read_pos += n
            elif op == 5:
                pass
            else:
                raise ValueError("Unknown CIGAR operation")
    return indels, depth, mapped, mapq0


def window_counts(index, ref_seq, tid, start, end, kind, allele, include_npp=False):
    """the six NGSQC_W_* counters of one window"""
    indels, depth, mapped, mapq0 = get_indels(index, ref_seq, tid, start, end, include_npp)
    want = ("+" if kind == 1 else "-") + allele if kind in (1, 2) else None
    n_ins = sum(1 for x in indels if x[0] == "+")
    return np.array([mapped, mapq0, depth, n_ins, len(indels) - n_ins, indels.count(want) if want else 0], dtype=np.int64)


class Fasta:
    """FastaFileIndex::seq over an in-memory genome {name: sequence}; tid -> name by the BAM's reference list"""

    def __init__(self, path, ref_names):
        self.seqs, name, parts = {}, None, []
        for ln in open(path):
            ln = ln.rstrip("\n")
            if ln.startswith(">"):
                if name is not None:
                    self.seqs[name] = "".join(parts)
                name, parts = ln[1:].split()[0], []
            else:
                parts.append(ln)
        if name is not None:
            self.seqs[name] = "".join(parts)
        self.names = ref_names

    def seq(self, tid, pos1, length):
        s = self.seqs[self.names[tid]]
        return s[pos1 - 1:pos1 - 1 + length].upper()   # (truncated at the contig end, FastaFileIndex.cpp:89-94)

    def slice(self, tid, start, end, length):
        """the reference slice [start, end + length) of a deletion window, 0 behind the contig end"""
        s = self.seq(tid, start, end - start + length)
        return s.encode("ascii") + b"\0" * (end - start + length - len(s))


# ---- the variant side of getVariantDetails (VariantList.cpp:49-64, 273-291, 1283-1384; BamReader.cpp:900-958) ----
def normalize(start, ref, obs):
    """Variant::normalize(int&, Sequence&, Sequence&)"""
    def multi():
        return (len(ref) != 1 or len(obs) != 1) and ref and obs
    if multi() and ref[0] == obs[0]:
        ref, obs, start = ref[1:], obs[1:], start + 1
    while multi() and ref[-1] == obs[-1]:
        ref, obs = ref[:-1], obs[:-1]
    while multi() and ref[0] == obs[0]:
        ref, obs, start = ref[1:], obs[1:], start + 1
    return start, ref, obs


def min_block(seq):
    for size in range(1, len(seq) // 2 + 1):
        if len(seq) % size == 0 and seq[:size] * (len(seq) // size) == seq:
            return seq[:size]
    return seq


def indel_region(start, end, ref, obs, seq):
    """Variant::indelRegion; seq(pos1, length) = FastaFileIndex::seq of the chromosome"""
    ref, obs = ("" if ref == "-" else ref), ("" if obs == "-" else obs)
    start, ref, obs = normalize(start, ref, obs)
    if ref and obs:
        return start, end
    start0, end0 = start, end
    block = min_block(ref + obs); bl = len(block); rep = False
    end -= bl - 1
    while seq(end + bl, bl) == block:
        end += bl; rep = True
    if not ref:
        start += 1
    while seq(start - bl, bl) == block:
        start -= bl; rep = True
    return (start, end + bl - 1) if rep else (start0, end0)


def vcf_variant(pos, ref, alt):
    """Variant(const VcfLine&): normalize("-", true) -> (start, end, ref, obs)"""
    start, r, o = normalize(pos, ref.upper(), alt.upper())
    end = start + len(r) - 1
    if not r:
        r, end = "-", end + 1
    if not o:
        o = "-"
    if r == "-":
        start, end = start - 1, end - 1
    return start, end, r, o


def indel_details(index, ref_seq, tid, pos, ref, alt, include_npp=False):
    """getVariantDetails of an indel / complex VCF line: (depth, frequency)"""
    start, end, r, o = vcf_variant(pos, ref, alt)
    s, e = indel_region(start, end, r, o, lambda p, n: ref_seq(tid, p, n))
    indels, depth, _, _ = get_indels(index, ref_seq, tid, s - 1, e + 1, include_npp)
    _, rn, on = normalize(start, "" if r == "-" else r, "" if o == "-" else o)
    rn, on = rn or "-", on or "-"
    if rn != "-" and on != "-":
        n_ins = sum(1 for x in indels if x[0] == "+")
        obs = min(n_ins, len(indels) - n_ins)
    elif rn == "-":
        obs = indels.count("+" + on)
    else:
        obs = indels.count("-" + rn)
    return depth, (min(1.0, obs / depth) if depth else float("nan"))
