"""Adversarial but valid BAMs for the parity tests: a deterministic generator of records in the shapes the kernels have special branches for.

generate(seed) -> Catalogue: the reference list REFS, the records (coordinate-sorted, unplaced ones last) and, per shape class, how many records of it were
written (Catalogue.shapes). seed=None is the hand-ordered catalogue: every shape once, at fixed positions, no random filler. Catalogue.write(path, member_sizes)
lays the records into BGZF members of the chosen sizes (cram_twin._bgzf), so members of a few KB leave records straddling member boundaries.

Domain: every record is one that htslib's bam_read1 accepts (sam.c: l_qname >= 1 and NUL-terminated, the variable-length fields fit block_size - which is also
the product's record_fields_fit, csrc/common.h - and for a mapped record with SEQ, the query length of the effective CIGAR equals l_seq) and sam_read1 accepts
(-1 <= tid, mtid < n_ref). Where the reference is undefined the oracle's documented choice is the contract (a negative tid counts as a special contig,
oracle/stats.hpp pass1_noroi). Shapes the oracle itself cannot read are left out, by option (exclude=): see SEQ_STAR_OOB and QUAL_OOR below."""
import random
import struct

import cram_twin

# ---- references: chr1 / chrX / chrY / chrMT, one _random and one chrUn_ contig (special for nonspecial()), a contig of 1 base and one of a few hundred
REFS = [("chr1", 30000), ("chrX", 9000), ("chrY", 5000), ("chrMT", 700), ("chr1_KI270706v1_random", 1500), ("chrUn_GL000195v1", 1200), ("chr2", 1), ("chr3", 300)]
T1, TX, TY, TMT, TRND, TUN, TONE, TSHORT = range(len(REFS))
M, I, D, N, S, H, P, EQ, X = range(9)
QUERY_OPS, REF_OPS = (M, I, S, EQ, X), (M, D, N, EQ, X)
MIN_MAPQ = 20   # the min_mapq of the catalogue's MAPQ edges (0, 1, MIN_MAPQ - 1, MIN_MAPQ, 255)

# Shape classes that the oracle cannot read without going out of bounds; a test of that path builds its file with exclude= these:
#  - SEQ "*" (l_seq = 0) on a mapped record with M operations: BamAlignment::qualities reads al.qual[ai] without a bound (oracle/stats.hpp base_qual_mask),
#    extractBaseByCIGAR reads al.seq / al.qual at the site (stats.hpp extract_base_by_cigar). Min_baseq > 0 coverage and the site pileup.
SEQ_STAR_OOB = {"seq_star"}
#  - QUAL 0xff: StatisticsReads::update throws "Base quality > 100" (stats.hpp reads_qc): read QC compares it on its own.
QUAL_OOR = {"qual_ff"}
# (a CIGAR whose query length is larger than a nonzero l_seq would reach qualities() past the record in the oracle as in the reference; bam_read1 refuses such a
#  mapped record anyway, so the catalogue has none: the product's "CIGAR longer than SEQ" clamps are reached through SEQ "*" records only.)


class Record:
    __slots__ = ("name", "flag", "tid", "pos", "mapq", "cigar", "seq", "qual", "isize", "mtid", "mpos", "aux", "cg", "shapes")

    def __init__(self, name, flag, tid, pos, cigar, seq, mapq=60, qual=None, isize=0, mtid=-1, mpos=-1, aux=b"", cg=None, shapes=()):
        self.name, self.flag, self.tid, self.pos, self.mapq = name, flag, tid, pos, mapq
        self.cigar, self.seq, self.qual, self.isize, self.mtid, self.mpos = list(cigar), seq, qual, isize, mtid, mpos
        self.aux, self.cg, self.shapes = aux, cg, set(shapes)

    def effective_cigar(self):
        """the CIGAR after the oracle's CG rule (oracle/bamio.hpp parse_rec): self.cg = (tag bytes, ops or None)"""
        if self.cg is None or self.cg[1] is None:
            return self.cigar
        c = self.cigar
        if c and self.tid >= 0 and self.pos >= 0 and c[0] == (S, len(self.seq)) and len(self.cg[1]) >= len(c):
            return self.cg[1]
        return c

    def check(self):
        """bam_read1 / sam_read1 / record_fields_fit accept it"""
        assert -1 <= self.tid < len(REFS) and -1 <= self.mtid < len(REFS) and self.pos >= -1 and len(self.cigar) < 65536
        assert all(0 <= ln < 1 << 28 and 0 <= op <= 8 for op, ln in self.cigar)
        qlen = sum(ln for op, ln in self.effective_cigar() if op in QUERY_OPS)
        if self.seq and not self.flag & 4 and self.cigar:
            assert qlen == len(self.seq), (self.name, qlen, len(self.seq))
        assert self.qual is None or len(self.qual) == len(self.seq)

    def bytes(self):
        n = self.name.encode() + b"\0"
        l_seq = len(self.seq)
        codes = ["=ACMGRSVTWYHKDBN".index(ch) for ch in self.seq] + [0]
        packed = bytes(codes[i] << 4 | codes[i + 1] for i in range(0, l_seq, 2))
        qual = bytes(self.qual) if self.qual is not None else b"\xff" * l_seq
        aux = self.aux + (self.cg[0] if self.cg else b"")
        body = struct.pack("<iiBBHHHiiii", self.tid, self.pos, len(n), self.mapq, 4680, len(self.cigar), self.flag, l_seq, self.mtid, self.mpos, self.isize) + n
        body += b"".join(struct.pack("<I", ln << 4 | op) for op, ln in self.cigar) + packed + qual + aux
        return struct.pack("<I", len(body)) + body

    def end(self):
        """bam_endpos (0-based exclusive) of the effective CIGAR"""
        rl = 0 if self.flag & 4 else sum(ln for op, ln in self.effective_cigar() if op in REF_OPS)
        return self.pos + max(rl, 1)


def _tagi(tag, t, v):
    return tag + t.encode() + struct.pack({"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[t], v)


def _cg(ops, kind="BI", n_entries=None):
    """a CG tag of the given type; n_entries: the count written (the array holds that many ops)"""
    n = len(ops) if n_entries is None else n_entries
    words = b"".join(struct.pack("<I", ln << 4 | op) for op, ln in ops[:n])
    if kind == "Z":
        return b"CGZ" + "".join(f"{ln}{'MIDNSHP=X'[op]}" for op, ln in ops).encode() + b"\0"
    if kind == "BS":
        return b"CGBS" + struct.pack("<I", n) + b"".join(struct.pack("<H", ln << 4 | op) for op, ln in ops[:n] if ln < 4096)
    return b"CGB" + (b"I" if kind == "BI" else b"i") + struct.pack("<I", n) + words


class Catalogue:
    def __init__(self, records):
        def key(r):
            return (r.tid if r.tid >= 0 else len(REFS), r.pos)
        self.records = sorted(records, key=key)   # (stable: the hand order within a position)
        for r in self.records:
            r.check()
        self.shapes = {}
        for r in self.records:
            for s in r.shapes:
                self.shapes[s] = self.shapes.get(s, 0) + 1

    def header(self):
        text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in REFS)
        h = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(REFS))
        for n, ln in REFS:
            h += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", ln)
        return h

    def subset(self, exclude=()):
        return [r for r in self.records if not (r.shapes & set(exclude))]

    def write(self, path, member_sizes=(65280,), exclude=()):
        recs = self.subset(exclude)
        raw = self.header() + b"".join(r.bytes() for r in recs)
        out, o, k = [], 0, 0
        while o < len(raw):
            n = member_sizes[k % len(member_sizes)]; k += 1
            out.append(cram_twin._bgzf(raw[o:o + n])); o += n
        open(path, "wb").write(b"".join(out) + cram_twin._bgzf(b""))
        return recs


# ---- the catalogue ----
def _seq(rng, n, with_n=True):
    return "".join(rng.choice("ACGTN" if with_n and rng.random() < 0.1 else "ACGT") for _ in range(n))


def _qual(rng, n):
    return [rng.randrange(2, 42) for _ in range(n)]


def _long_cigar(n_ops, rng, with_n=False):
    """n_ops operations (S first and last), every kind of query / reference op between them; returns (ops, l_seq)"""
    body = [M, I, M, D, EQ, X, M] + ([N] if with_n else [])
    ops = [(S, 3)]
    k = 0
    while len(ops) < n_ops - 1:
        op = body[k % len(body)]; k += 1
        ops.append((op, 1 + rng.randrange(3) if op != N else 20))
    ops.append((S, 2))
    return ops, sum(ln for op, ln in ops if op in QUERY_OPS)


def _catalogue(rng, fixed):
    """every shape class; positions are fixed (seed None) or drawn"""
    out = []

    def pos(tid, lo=10, hi=None):
        hi = hi if hi is not None else REFS[tid][1] - 200
        return lo if fixed else rng.randrange(lo, max(lo + 1, hi))

    def add(name, flag, tid, p, cigar, shapes, l_seq=None, seq=None, **kw):
        if seq is None:
            l_seq = l_seq if l_seq is not None else sum(ln for op, ln in cigar if op in QUERY_OPS)
            seq = _seq(rng, l_seq)
        kw.setdefault("qual", _qual(rng, len(seq)))
        kw.setdefault("mtid", tid); kw.setdefault("mpos", p)
        kw.setdefault("mapq", 60)
        out.append(Record(f"{name}:{len(out)}", flag, tid, p, cigar, seq, shapes=shapes, **kw))
        return out[-1]

    PP = 0x1 | 0x2 | 0x40   # paired, proper, read 1
    base = pos(T1, 100, 20000)
    # CIGAR operations
    add("opN", PP, T1, base + 5, [(M, 20), (N, 300), (M, 15)], {"op_N"}, isize=400)
    add("opN_R2", 0x1 | 0x2 | 0x80 | 0x10, T1, base + 6, [(S, 2), (M, 18), (N, 50), (M, 10), (N, 7), (M, 5)], {"op_N"}, isize=-400)
    add("opP", PP, T1, base + 8, [(M, 12), (P, 3), (M, 12)], {"op_P"})
    add("opP2", PP, T1, base + 9, [(M, 6), (I, 2), (P, 1), (I, 1), (M, 9)], {"op_P"})
    add("zero", PP, T1, base + 10, [(M, 0), (M, 10), (I, 0), (D, 0), (M, 10), (N, 0), (S, 0)], {"zero_len"})
    add("zero2", PP, T1, base + 11, [(S, 0), (M, 25), (D, 0)], {"zero_len"})
    add("adjM", PP, T1, base + 12, [(M, 5), (M, 7), (I, 2), (I, 3), (M, 4), (D, 2), (D, 3), (M, 6)], {"adjacent_same"})
    add("adjS", PP, T1, base + 13, [(S, 2), (S, 3), (M, 20), (H, 1), (H, 2)], {"adjacent_same"})
    add("insStart", PP, T1, base + 14, [(I, 3), (M, 20)], {"indel_at_start"})
    add("insEnd", PP, T1, base + 15, [(M, 20), (I, 4)], {"indel_at_end"})
    add("delStart", PP, T1, base + 16, [(D, 3), (M, 20)], {"indel_at_start"})
    add("delEnd", PP, T1, base + 17, [(M, 20), (D, 2)], {"indel_at_end"})
    add("sInsStart", PP, T1, base + 18, [(S, 4), (I, 2), (M, 20), (I, 1), (S, 3)], {"indel_at_start", "indel_at_end"})
    add("eqx", PP, T1, base + 19, [(EQ, 8), (X, 1), (EQ, 5), (D, 1), (X, 3)], {"op_eqx"})
    add("hclip", PP, T1, base + 20, [(H, 5), (S, 3), (M, 22), (S, 4), (H, 6)], {"clips"})
    add("nOnly", PP, T1, base + 21, [(S, 4), (N, 10), (M, 6)], {"op_N"})
    # SEQ "*" (l_seq = 0) with a CIGAR: the kernels' "CIGAR longer than SEQ" clamps (bam_read1 checks the query length only when l_seq > 0)
    add("seqStar", PP, T1, base + 22, [(M, 30)], {"seq_star"}, seq="")
    add("seqStar2", PP, T1, base + 23, [(S, 3), (M, 10), (D, 2), (N, 30), (M, 8)], {"seq_star"}, seq="")
    add("seqStarNoCig", PP, T1, base + 24, [], {"seq_star", "no_cigar"}, seq="")
    # QUAL 0xff ("*")
    add("qualFF", PP, T1, base + 25, [(M, 30)], {"qual_ff"}, qual=None)
    add("qualFF2", 0x1 | 0x2 | 0x80 | 0x10, T1, base + 26, [(S, 5), (M, 25)], {"qual_ff"}, qual=None)
    # placement edges
    add("mappedNoPlace", 0x1 | 0x40, -1, -1, [(M, 20)], {"mapped_unplaced"}, mtid=-1, mpos=-1)
    add("mappedTidNeg", 0x1 | 0x2 | 0x40, -1, 500, [(M, 20)], {"mapped_unplaced"}, mtid=-1, mpos=-1)
    add("mappedPosNeg", 0x1 | 0x2 | 0x40, T1, -1, [(M, 20)], {"mapped_unplaced"})
    add("unmappedCig", 0x1 | 0x4 | 0x80, T1, base + 30, [(M, 25)], {"unmapped_cigar"})
    add("unmappedCigLong", 0x4, TX, pos(TX), [(S, 1), (M, 10), (D, 40), (M, 20)], {"unmapped_cigar"})
    add("unmapped", 0x4, -1, -1, [], {"unmapped"}, mtid=-1, mpos=-1)
    add("unmappedPlaced", 0x1 | 0x4 | 0x40, T1, base + 31, [], {"unmapped"})
    add("noCigar", PP, T1, base + 32, [], {"no_cigar"}, l_seq=25)
    add("rlen0", PP, T1, base + 33, [(S, 10), (I, 5)], {"rlen0"})
    add("rlen0H", PP, T1, base + 34, [(H, 3), (S, 6), (I, 2), (S, 1)], {"rlen0"})
    # contig ends: position 0, the last base, past the end; the contig of one base and the short one
    L1, Ls = REFS[T1][1], REFS[TSHORT][1]
    add("pos0", PP, T1, 0, [(M, 30)], {"pos0"})
    add("pos0del", PP, TSHORT, 0, [(D, 2), (M, 20)], {"pos0"})
    add("lastBase", PP, T1, L1 - 1, [(M, 1)], {"last_base"})
    add("lastBasePast", PP, TSHORT, Ls - 1, [(M, 25)], {"last_base", "past_end"})
    add("pastEnd", PP, T1, L1 - 10, [(M, 20), (D, 3), (M, 10)], {"past_end"})
    add("pastEndN", PP, TSHORT, Ls - 30, [(M, 20), (N, 100), (M, 10)], {"past_end", "op_N"})
    add("one", PP, TONE, 0, [(M, 1)], {"one_base_contig"})
    add("onePast", PP, TONE, 0, [(S, 2), (M, 30), (I, 2)], {"one_base_contig", "past_end"})
    add("mtPast", PP, TMT, REFS[TMT][1] - 5, [(M, 40)], {"past_end"})
    # special contigs, X / Y
    for t in (TRND, TUN, TX, TY):
        add(f"contig{t}", PP, t, pos(t), [(M, 40)], {"special_contig" if t in (TRND, TUN) else "sex_contig"})
        add(f"contigEnd{t}", PP, t, REFS[t][1] - 15, [(M, 30)], {"past_end"})
    # every flag bit alone and in combinations
    for b in range(12):
        add(f"flag{1 << b:x}", 1 << b, T1, base + 40 + b, [(M, 25)], {"flag_bit"}, isize=250 if b % 2 else -250)
    for f in (0x1 | 0x2 | 0x40 | 0x400, 0x1 | 0x2 | 0x80 | 0x100, 0x1 | 0x2 | 0x40 | 0x800, 0x1 | 0x40 | 0x8, 0x1 | 0x2 | 0x40 | 0x10 | 0x20,
              0x1 | 0x2 | 0x40 | 0x80, 0x2 | 0x400, 0xfff & ~0x4, 0xfff, 0x1 | 0x2 | 0x40 | 0x200, 0x1 | 0x2 | 0x80 | 0x400 | 0x10):
        add(f"flags{f:x}", f, T1, base + 60, [(S, 2), (M, 23)], {"flag_combo"}, isize=300)
    # MAPQ edges
    for q in (0, 1, MIN_MAPQ - 1, MIN_MAPQ, 255):
        add(f"mapq{q}", PP, T1, base + 70, [(M, 25)], {f"mapq_{q}"}, mapq=q, isize=200)
        add(f"mapqNP{q}", 0x1 | 0x40, T1, base + 71, [(M, 25)], {f"mapq_{q}"}, mapq=q, isize=200)
    # insert sizes (proper pairs, read 1 and read 2)
    for k, isz in enumerate((0, 999, -999, 1000, -1000, 12345, -12345, 2 ** 31 - 1, -(2 ** 31 - 1), 3, 49, -50)):
        add(f"isize{isz}", PP if k % 2 == 0 else 0x1 | 0x2 | 0x80 | 0x10, T1, base + 80, [(M, 25)], {"isize"}, isize=isz)
    # tags: NM / DP of every integer type, with f / Z / B tags and tags sharing a prefix in front of them
    types = ["c", "C", "s", "S", "i", "I"]
    for k, t in enumerate(types):
        front = [b"NAf" + struct.pack("<f", 3.5), b"XZZNM:i:7 DP:i:9\0", b"NBBc" + struct.pack("<I", 3) + b"\1\2\3", b"DQi" + struct.pack("<i", 77),
                 b"XBBI" + struct.pack("<I", 2) + struct.pack("<II", 5, 6)][k % 5:] + [b"MDZ10A14\0"]
        aux = b"".join(front) + _tagi(b"NM", t, 1 + k % 3) + _tagi(b"DP", types[(k + 2) % 6], k % 5)
        add(f"tags{t}", PP, T1, base + 90 + k, [(M, 10), (I, 1), (M, 14)], {"tags"}, aux=aux, isize=150)
    add("tagsF", PP, T1, base + 97, [(M, 25)], {"tags"}, aux=b"NMf" + struct.pack("<f", 2.0) + b"DPZ3\0", isize=150)
    add("tagsDP", PP, T1, base + 98, [(M, 25)], {"tags"}, aux=b"DPC" + b"\x07" + b"NMs" + struct.pack("<h", -3), isize=150)
    # CG edges. The inline CIGAR is htslib's placeholder "l_seq S, ref_len N"; the tag carries I and D so a CIGAR taken or not taken from it changes the
    # gap counts (BamFilter), the span and the depth
    cg_ops = [(S, 2), (M, 10), (I, 2), (M, 6), (D, 3), (M, 10), (N, 40), (M, 5)]
    cg_l = sum(ln for op, ln in cg_ops if op in QUERY_OPS)
    cg_r = sum(ln for op, ln in cg_ops if op in REF_OPS)
    ph = [(S, cg_l), (N, cg_r)]
    p0 = base + 100
    add("cgBI", PP, T1, p0, ph, {"cg_applied"}, l_seq=cg_l, cg=(_cg(cg_ops), cg_ops), isize=120)
    add("cgBIrev", 0x1 | 0x2 | 0x80 | 0x10, T1, p0 + 1, ph, {"cg_applied"}, l_seq=cg_l, cg=(_cg(cg_ops), cg_ops), isize=-120)
    add("cgBS", PP, T1, p0 + 2, ph, {"cg_BS"}, l_seq=cg_l, cg=(_cg(cg_ops, "BS"), None))
    add("cgBi", PP, T1, p0 + 3, ph, {"cg_Bi"}, l_seq=cg_l, cg=(_cg(cg_ops, "Bi"), None))
    add("cgZ", PP, T1, p0 + 4, ph, {"cg_Z"}, l_seq=cg_l, cg=(_cg(cg_ops, "Z"), None))
    add("cgShort", PP, T1, p0 + 5, [(S, cg_l), (N, 10), (M, 0)], {"cg_short"}, l_seq=cg_l, cg=(_cg(cg_ops[:2]), None))
    kne = [(S, cg_l - 1), (M, 1)]
    add("cgKne", PP, T1, p0 + 6, kne, {"cg_k_ne_lseq"}, l_seq=cg_l, cg=(_cg(cg_ops), None))
    add("cgTidNeg", 0x1 | 0x2 | 0x40, -1, p0, ph, {"cg_tid_neg"}, l_seq=cg_l, cg=(_cg(cg_ops), None), mtid=-1, mpos=p0)
    add("cgTidNeg", 0x1 | 0x2 | 0x80, -1, p0, ph, {"cg_tid_neg"}, l_seq=cg_l, cg=(_cg(cg_ops), None), mtid=-1, mpos=p0)   # (its mate: BamFilter pairs by name)
    out[-1].name = out[-2].name
    add("cgPosNeg", 0x1 | 0x2 | 0x40, T1, -1, ph, {"cg_pos_neg"}, l_seq=cg_l, cg=(_cg(cg_ops), None))
    add("cgPosNeg", 0x1 | 0x2 | 0x80, T1, -1, ph, {"cg_pos_neg"}, l_seq=cg_l, cg=(_cg(cg_ops), None))
    out[-1].name = out[-2].name
    add("cgUnmapped", 0x1 | 0x4 | 0x40, T1, p0 + 7, ph, {"cg_unmapped"}, l_seq=cg_l, cg=(_cg(cg_ops), cg_ops))
    long_cg, long_l = _long_cigar(300, rng, with_n=True)
    add("cgLong", PP, T1, p0 + 8, [(S, long_l), (N, sum(ln for op, ln in long_cg if op in REF_OPS))], {"cg_applied", "ops_300"}, l_seq=long_l,
        cg=(_cg(long_cg), long_cg))
    # long CIGARs around the LONG_CIGAR = 64 dispatch (csrc/common.h)
    for n_ops in (63, 64, 65, 300):
        for k, wn in enumerate((False, True)):
            ops, l_seq = _long_cigar(n_ops, rng, with_n=wn)
            add(f"ops{n_ops}", PP if k == 0 else 0x1 | 0x2 | 0x80 | 0x10, T1, base + 110 + k, ops, {f"ops_{n_ops}"}, isize=500 if k == 0 else -500)
    return out


def _filler(rng, n):
    """random proper pairs and single reads on every contig: depth under the catalogue"""
    out = []
    for k in range(n):
        tid = rng.choice([T1, T1, T1, T1, TX, TY, TMT, TRND, TUN, TSHORT])
        L = rng.randrange(20, 151)
        p = rng.randrange(0, max(1, REFS[tid][1] - 20))
        ops = [(M, L)]
        u = rng.random()
        if u < 0.15:
            a = rng.randrange(1, L - 1); ops = [(M, a), (I, 1), (M, L - a - 1)]
        elif u < 0.3:
            a = rng.randrange(1, L); ops = [(M, a), (D, rng.randrange(1, 4)), (M, L - a)]
        elif u < 0.4:
            a = rng.randrange(1, L); ops = [(S, a), (M, L - a)]
        elif u < 0.45:
            a = rng.randrange(1, L); ops = [(M, a), (N, rng.randrange(10, 300)), (M, L - a)]
        flag = rng.choice([0x1 | 0x2 | 0x40, 0x1 | 0x2 | 0x80 | 0x10, 0x1 | 0x40, 0x1 | 0x2 | 0x40 | 0x400, 0, 0x10, 0x1 | 0x2 | 0x80 | 0x100])
        isize = rng.choice([-1, 1]) * rng.randrange(0, 1300)
        aux = _tagi(b"NM", "C", rng.randrange(4)) if rng.random() < 0.5 else b""
        if rng.random() < 0.2:
            aux += _tagi(b"DP", rng.choice("cCsSiI"), rng.randrange(0, 6))
        out.append(Record(f"f{k}", flag, tid, p, ops, _seq(rng, L), mapq=rng.choice([0, 1, 19, 20, 37, 60, 255]), qual=_qual(rng, L), isize=isize,
                          mtid=tid, mpos=p + 50, aux=aux))
    return out


def generate(seed=None, n_filler=1500):
    """seed None: the hand-ordered catalogue alone. A seed: the catalogue at drawn positions (three copies) plus n_filler random reads."""
    if seed is None:
        return Catalogue(_catalogue(random.Random(0), fixed=True))
    rng = random.Random(seed)
    recs = []
    for _ in range(3):
        recs += _catalogue(rng, fixed=False)
    return Catalogue(recs + _filler(rng, n_filler))


REQUIRED_SHAPES = ("op_N", "op_P", "zero_len", "adjacent_same", "indel_at_start", "indel_at_end", "seq_star", "qual_ff", "mapped_unplaced", "unmapped_cigar",
                   "no_cigar", "rlen0", "pos0", "last_base", "past_end", "one_base_contig", "special_contig", "flag_bit", "flag_combo", "mapq_0", "mapq_1",
                   f"mapq_{MIN_MAPQ - 1}", f"mapq_{MIN_MAPQ}", "mapq_255", "isize", "tags", "cg_applied", "cg_BS", "cg_Bi", "cg_Z", "cg_short", "cg_k_ne_lseq",
                   "cg_tid_neg", "cg_pos_neg", "ops_63", "ops_64", "ops_65", "ops_300")
