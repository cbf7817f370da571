"""Designed CIGARs, site tables and window tables for the site pileup and the indel windows (csrc/scan.hip: pileup_kernel, the thread-per-record walk of at most
LONG_CIGAR operations, and pileup_long_kernel, the wave-per-record walk rebuilt from ballots and prefix sums over chunks of 64 operations; csrc/indel.hip:
indel_kernel and indel_long_kernel, the same pair for BamReader::getIndels).

Every case is a list of advbam.Record in FILE ORDER on REFS (advbam.REFS with a chr1 of 140 000 bases: two 64 kb bucket edges), a table of sites and / or windows
(sorted by reference, then position / start, as the C ABI takes them), the parameter sets it is run under and a premise over the bookkeeping of
tests/pileup_model.py: what the case is there for, asserted by tests/test_cpu_pileup_model.py so that a later edit cannot hollow the case out. The expected values
are the model's; nothing here knows them.

Records that no BAM writer would produce are marked by shape: "seq_short" (SEQ shorter than the CIGAR's query length: bam_read1 refuses it for a mapped record, the
library and the model do not), "seq_oob" (of those, the ones whose walk reaches a read index behind SEQ: the oracle reads past the record there, so a file for
the oracle leaves them out, as advbam.SEQ_STAR_OOB), "raw_ops" (an operation code above 8)."""
import random

import advbam as A
import cram_twin
import pileup_model as PM

M, I, D, N, S, H, P, EQ, X = A.M, A.I, A.D, A.N, A.S, A.H, A.P, A.EQ, A.X
OP9 = 9
T1, TX, TY, TMT = A.T1, A.TX, A.TY, A.TMT
REFS = [("chr1", 140000)] + list(A.REFS[1:])
PP = 0x1 | 0x2 | 0x40            # paired, proper, read 1
NPP = 0x1 | 0x40
ALLELE_NONE, ALLELE_INS, ALLELE_DEL = 0, 1, 2   # include/ngsqc.h
ORACLE_EXCLUDE = {"seq_oob"}
BUCKET = 1 << PM.PILEUP_BUCKET_SHIFT
LONG = PM.LONG_CIGAR
FORM_LENGTHS = (64, 65, 128, 129, 255, 256, 257, 260)
SMALL_MEMBERS = (3000, 2900, 3100)


class Genome:
    """the bases both sides take their deletions from: a fixed letter per position, the contigs as long as REFS says"""

    def seq(self, tid, pos1, length):
        end = min(pos1 - 1 + length, REFS[tid][1])
        return "".join("ACGT"[((p * 2654435761) >> 13 ^ tid * 97) & 3] for p in range(pos1 - 1, end))

    def slice(self, tid, start, end, length):
        s = self.seq(tid, start, end - start + length)
        return s.encode() + b"\0" * (end - start + length - len(s))


GENOME = Genome()


def header():
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, ln) for n, ln in REFS)
    h = b"BAM\1" + A.struct.pack("<i", len(text)) + text.encode() + A.struct.pack("<i", len(REFS))
    for n, ln in REFS:
        h += A.struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + A.struct.pack("<i", ln)
    return h


def qlen(cigar):
    return sum(ln for op, ln in cigar if op in A.QUERY_OPS)


def rlen(cigar):
    return sum(ln for op, ln in cigar if op in A.REF_OPS)


def draw(seed, n):
    rng = random.Random(seed)
    return "".join(rng.choice("ACGT") for _ in range(n))


def rec(name, pos, cigar, seq=None, qual=None, flag=PP, tid=T1, mapq=60, cg=False, l_seq=None, seed=None, shapes=()):
    """pos: 0-based. seq None: letters drawn from the seed (the name: forms of one alignment share a seed, and with it SEQ and QUAL); qual None: 30..39 in turn.
    cg: the CIGAR goes into a CG:B,I tag behind htslib's placeholder "l_seq S, ref_len N". l_seq: a SEQ cut short (or made longer) against the CIGAR"""
    cigar = list(cigar)
    if seq is None:
        seq = draw(seed if seed is not None else name, qlen(cigar))[:qlen(cigar) if l_seq is None else l_seq]
    if qual is None:
        qual = [30 + i % 10 for i in range(len(seq))]
    shapes = set(shapes)
    if len(seq) != qlen(cigar):
        shapes.add("seq_short")
    if any(op > 8 for op, _ in cigar):
        shapes.add("raw_ops")
    if cg:
        return A.Record(name, flag, tid, pos, [(S, len(seq)), (N, rlen(cigar))], seq, mapq=mapq, qual=list(qual), cg=(A._cg(cigar), cigar), shapes=shapes)
    return A.Record(name, flag, tid, pos, cigar, seq, mapq=mapq, qual=list(qual), shapes=shapes)


def split_m(cigar, n_ops):
    """the same alignment in n_ops operations: the longest M gives up one-base pieces from its front"""
    cigar = list(cigar)
    extra = n_ops - len(cigar)
    k = max((i for i, (op, _) in enumerate(cigar) if op == M), key=lambda i: cigar[i][1])
    assert 0 <= extra < cigar[k][1]
    return cigar[:k] + [(M, 1)] * extra + [(M, cigar[k][1] - extra)] + cigar[k + 1:]


PAD = LONG + 2   # one-base M operations in front of a padded twin: the interesting operations begin in the second chunk of 64


def padded(name, pos, cigar, seq=None, n=PAD, seed=None, l_seq=None, qual=None, **kw):
    """the alignment n bases further left behind n one-base M operations: SEQ and QUAL of rec(name, pos, cigar, ...) behind n bases of their own"""
    if seq is None:
        seq = draw(seed if seed is not None else name, qlen(cigar))[:qlen(cigar) if l_seq is None else l_seq]
    if qual is not None:
        qual = [40] * n + list(qual)
    return rec(name, pos - n, [(M, 1)] * n + list(cigar), seq="ACGT"[n % 4] * n + seq, qual=qual, **kw)


def key(r):
    return (r.tid if r.tid >= 0 else len(REFS), r.pos)


class Case:
    def __init__(self, name, records, premise, sites=(), windows=(), site_params=((1, 13, False),), win_params=(False,), member_sizes=(65280,), raises=False):
        self.name, self.premise, self.member_sizes, self.raises = name, premise, tuple(member_sizes), raises
        self.records = sorted(records, key=key)   # (stable: the order given within a position)
        self.sites = sorted(sites)                # (tid, pos); a row may stand twice
        self.windows = sorted(windows, key=lambda w: (w[0], w[1]))   # (tid, start, end, kind, allele, reference slice or None); stable
        self.site_params, self.win_params = list(site_params), list(win_params)
        for r in self.records:
            assert -1 <= r.tid < len(REFS) and r.pos >= -1 and len(r.cigar) < 65536 and (r.qual is None or len(r.qual) == len(r.seq)), r.name
            if not r.shapes & {"seq_short", "raw_ops"}:
                r.check()
        assert len({r.name for r in self.records}) == len(self.records)
        assert all(1 <= p for _, p in self.sites) and all(1 <= s <= e for _, s, e, *_ in self.windows)

    def subset(self, exclude=()):
        return [r for r in self.records if not (r.shapes & set(exclude))]

    def write(self, path, member_sizes=None, exclude=(), whole_records=True):
        """the twin of readdepth_cases.Case.write behind this module's header: BGZF members of whole records in the given sizes, as htslib writes them, or the
        stream cut wherever a size ends (the library's general path)"""
        recs = self.subset(exclude)
        sizes = member_sizes or self.member_sizes
        if whole_records:
            parts, cur = [header()], b""
            for r in recs:
                b = r.bytes()
                if cur and len(cur) + len(b) > sizes[(len(parts) - 1) % len(sizes)]:
                    parts.append(cur); cur = b""
                cur += b
            parts.append(cur)
        else:
            raw = header() + b"".join(r.bytes() for r in recs)
            parts, o = [], 0
            while o < len(raw):
                n = sizes[len(parts) % len(sizes)]
                parts.append(raw[o:o + n]); o += n
        open(path, "wb").write(b"".join(cram_twin._bgzf(p) for p in parts if p) + cram_twin._bgzf(b""))
        return recs

    def site_book(self, min_mapq=1, min_baseq=13, include_npp=False, exclude=()):
        b = []
        PM.site_counts(self.subset(exclude), self.sites, min_mapq, min_baseq, include_npp, n_ref=len(REFS), book=b)
        return b

    def win_book(self, include_npp=False):
        b = []
        PM.window_counts(self.records, self.windows, include_npp, GENOME.seq, book=b)
        return b

    def index_of(self, name):
        return next(k for k, r in enumerate(self.records) if r.name == name)


def span_sites(r, step=1):
    """every step-th position of the record's span (of the CIGAR htslib takes)"""
    c = r.effective_cigar()
    return [(r.tid, p) for p in range(r.pos + 1, r.pos + max(rlen(c), 1) + 1, step)]


def event_windows(r, pad=1, wrong=True):
    """windows around every I and D of the record, with its own allele (and, wrong=True, with one that differs in its last base)"""
    out, gp, rp = [], r.pos + 1, 0
    for op, ln in r.effective_cigar():
        s, e = max(1, gp - pad), gp + pad
        if op == I:
            a = r.seq[rp:rp + ln]
            out.append((r.tid, s, e, ALLELE_INS, a, None))
            if wrong and a:
                out.append((r.tid, s, e, ALLELE_INS, a[:-1] + ("A" if a[-1] != "A" else "C"), None))
        elif op == D:
            a = GENOME.seq(r.tid, gp, ln)
            out.append((r.tid, s, e, ALLELE_DEL, a, GENOME.slice(r.tid, s, e, len(a))))
        if op in A.REF_OPS:
            gp += ln
        if op in A.QUERY_OPS:
            rp += ln
    return out


def del_window(tid, s, e, allele):
    return (tid, s, e, ALLELE_DEL, allele, GENOME.slice(tid, s, e, len(allele)))


def _entries(book, case, name, kind="site"):
    k = case.index_of(name)
    return [e for e in book if e.k == k and e.kind == kind]


def _at(book, case, name, pos):
    """the entry of record `name` at the site(s) on position pos"""
    k = case.index_of(name)
    out = [e for e in book if e.k == k and case.sites[e.i][1] == pos]
    assert out, (name, pos)
    return out[0]


# ---- two_forms: one alignment in 64, 65, 128, 129, 255, 256, 257 and 260 operations, in the core and behind a CG tag ----
def _base_alignment():
    cyc = [(I, 2), (M, 4), (D, 3), (M, 3), (EQ, 2), (X, 1), (N, 7), (M, 5)]
    ops = [(H, 2), (S, 3), (M, 220)]
    while len(ops) < LONG - 1:
        ops.append(cyc[(len(ops) - 3) % len(cyc)])
    return ops + [(S, 2)]


def two_forms():
    base = _base_alignment()
    assert len(base) == LONG
    recs = []
    for n in FORM_LENGTHS:
        for cg in (False, True):
            recs.append(rec("form%d%s" % (n, "cg" if cg else ""), 1000, split_m(base, n), cg=cg, seed="form"))
    sites = span_sites(recs[0])
    windows = event_windows(recs[0]) + [(T1, 1100, 1101, ALLELE_NONE, "", None)]

    def premise(case):
        one = [Case("one", [r], None, case.sites, case.windows) for r in case.records]
        rows = [PM.site_counts(c.records, c.sites, 1, 13, False, n_ref=len(REFS)) for c in one]
        wrows = [PM.window_counts(c.records, c.windows, False, GENOME.seq) for c in one]
        assert all((x == rows[0]).all() for x in rows) and all((x == wrows[0]).all() for x in wrows)
        assert rows[0][:, :6].sum() > 300 and rows[0][:, 5].sum() >= 20 and wrows[0][:, PM.W_MATCH].sum() >= 10
        book = case.site_book()
        assert sorted({e.n_ops for e in book}) == sorted(FORM_LENGTHS)
        assert any(not e.long for e in book) and any(e.long for e in book)
        assert len(case.sites) == rlen(base) and {e.branch for e in book} >= {"base", "del", "skip"}
        wbook = case.win_book()
        assert {e.n_ops for e in wbook if e.branch == "walked"} == set(FORM_LENGTHS)
        assert sum(x[0] == (S, qlen(base)) for x in (r.cigar for r in case.records)) == len(FORM_LENGTHS)   # the placeholder of the CG forms
    return Case("two_forms", recs, premise, sites, windows, site_params=[(1, 13, False), (1, 35, False)])


# ---- ops_at_site: every operation at the site, once in at most 64 operations and once padded past 64 ----
# (name, operations, l_seq or None, [(1-based offset of the site from the record's first base, the branch that decides, its operation index)])
SCENARIOS = [
    ("m_d", [(M, 10), (D, 3), (M, 10)], None, [(10, "base", 0), (11, "del", 1), (13, "del", 1), (14, "base", 2)]),
    ("n", [(M, 10), (N, 20), (M, 10)], None, [(11, "skip", 1), (20, "skip", 1), (30, "skip", 1), (31, "base", 2)]),
    ("ins", [(M, 10), (I, 3), (M, 10)], None, [(10, "base", 0), (11, "base", 2)]),
    ("lead_s", [(S, 4), (M, 10)], None, [(1, "base", 1)]),
    ("lead_h", [(H, 4), (M, 10)], None, [(1, "base", 1)]),
    ("eqx", [(EQ, 5), (X, 2), (M, 5)], None, [(5, "base", 0), (6, "base", 1), (7, "base", 1), (8, "base", 2)]),
    ("p_front", [(M, 5), (P, 2), (M, 10)], None, [(5, "base", 0), (6, "unknown", 1), (15, "unknown", 1)]),
    ("op9_front", [(M, 5), (OP9, 2), (M, 10)], None, [(5, "base", 0), (6, "unknown", 1), (15, "unknown", 1)]),
    ("p_behind", [(M, 10), (P, 1), (D, 2), (M, 5)], None, [(1, "base", 0), (10, "base", 0), (11, "unknown", 1)]),
    ("s_exhausts", [(M, 10), (S, 5), (M, 10)], 12, [(10, "base", 0), (11, "softclip", 1), (15, "softclip", 1), (20, "softclip", 1)]),
    ("s_exhausts_d", [(M, 10), (S, 5), (D, 4), (M, 6)], 12, [(11, "softclip", 1), (14, "softclip", 1), (20, "softclip", 1)]),
    ("s_exhausts_p", [(M, 10), (S, 5), (P, 1), (M, 10)], 12, [(11, "softclip", 1), (20, "softclip", 1)]),
    ("p_then_s", [(M, 10), (P, 1), (S, 5), (M, 10)], 12, [(11, "unknown", 1), (20, "unknown", 1)]),
    ("cigar_longer", [(M, 20)], 12, [(12, "base", 0), (13, "seq_oob", 0), (20, "seq_oob", 0)]),
    ("seq_star", [(M, 20)], 0, [(1, "seq_oob", 0), (20, "seq_oob", 0)]),
]
OOB = ("cigar_longer", "seq_star")
SCEN_STEP = 400


def ops_at_site():
    recs, sites, expect = [], [], []
    for j, (name, ops, l_seq, exp) in enumerate(SCENARIOS):
        p = 2000 + SCEN_STEP * j
        sh = {"seq_oob"} if name in OOB else ()
        recs.append(rec(name, p, ops, l_seq=l_seq, seed=name, shapes=sh))
        recs.append(padded(name + "_long", p, ops, l_seq=l_seq, seed=name, shapes=sh))
        recs.append(padded(name + "_longcg", p, ops, l_seq=l_seq, seed=name, shapes=sh, cg=True))
        sites += [(T1, q) for q in range(p - PAD + 1, p + rlen(ops) + 3)]          # the pad, the span and two positions behind it
        for off, branch, k in exp:
            expect.append((name, p + off, branch, k))
            expect.append((name + "_long", p + off, branch, k + PAD))
            expect.append((name + "_longcg", p + off, branch, k + PAD))
    # a soft clip that exhausts SEQ in an earlier chunk of 64 than the site's operation: every later site counts nothing
    p = 2000 + SCEN_STEP * len(SCENARIOS)
    far = [(M, 10), (S, 5)] + [(M, 1)] * (2 * LONG) + [(D, 2), (M, 10)]
    recs.append(rec("s_far", p, far, l_seq=12, seed="s_far"))
    sites += [(T1, q) for q in range(p + 1, p + rlen(far) + 1)]
    expect += [("s_far", p + 10, "base", 0), ("s_far", p + 11, "softclip", 1), ("s_far", p + 10 + LONG, "softclip", 1), ("s_far", p + 10 + 2 * LONG + 1, "softclip", 1),
               ("s_far", p + rlen(far), "softclip", 1)]
    # reads of I and S operations only, and reads without reference length, each with a site on pos + 1
    p += SCEN_STEP
    recs.append(rec("only_is", p, [(S, 5), (I, 5)]))
    recs.append(rec("only_is_long", p, [(S, 1), (I, 1)] * 40))
    recs.append(rec("rlen0", p + 10, [(H, 2), (S, 3), (I, 2)]))
    recs.append(rec("rlen0_long", p + 10, [(H, 1)] * PAD + [(S, 3), (I, 2)]))
    recs.append(rec("rlen0_cg", p + 10, [(H, 1)] * PAD + [(S, 3), (I, 2)], cg=True))
    recs.append(rec("rlen0_s", p + 20, [(H, 2), (S, 5)]))                       # ... and one of them ends at a soft clip: nothing, not "Could not find position"
    recs.append(rec("rlen0_s_long", p + 20, [(H, 1)] * PAD + [(S, 5)]))
    sites += [(T1, p), (T1, p + 1), (T1, p + 2), (T1, p + 10), (T1, p + 11), (T1, p + 12), (T1, p + 20), (T1, p + 21), (T1, p + 22)]
    expect += [("rlen0_s", p + 21, "softclip", 1), ("rlen0_s_long", p + 21, "softclip", PAD),
               ("only_is", p + 1, "only_ins", -1), ("only_is_long", p + 1, "only_ins", -1), ("rlen0", p + 11, "notfound", 3), ("rlen0_long", p + 11, "notfound", PAD + 2),
               ("rlen0_cg", p + 11, "notfound", PAD + 2)]

    def premise(case):
        book = case.site_book()
        for name, pos, branch, k in expect:
            e = _at(book, case, name, pos)
            assert (e.branch, e.op_index) == (branch, k), (name, pos, e.branch, e.op_index, branch, k)
            assert e.long == (name.endswith(("_long", "_longcg", "_cg")) or name == "s_far"), name
        for name in ("only_is", "only_is_long", "rlen0", "rlen0_long", "rlen0_cg", "rlen0_s", "rlen0_s_long"):          # they meet the site on pos + 1 and no other
            assert len(_entries(book, case, name)) == 1, name
        assert {"base", "del", "skip", "softclip", "unknown", "seq_oob", "only_ins", "notfound"} == {e.branch for e in book if e.long} == {e.branch for e in book if not e.long}
        k = case.index_of("s_far")                                                             # the clip in chunk 0, sites decided (if it were not there) in chunks 0, 1 and 2
        assert len(case.records[k].cigar) > 2 * LONG and sum(e.branch == "softclip" for e in book if e.k == k) > 2 * LONG
        k = case.index_of("s_exhausts_long")                                                   # ... and in the chunk of the site's own operation
        assert {e.op_index // LONG for e in book if e.k == k and e.branch == "softclip"} == {1}
        assert all(r.shapes & {"seq_oob"} for r in case.records if r.name.startswith(OOB)) and len(case.subset(ORACLE_EXCLUDE)) == len(case.records) - 3 * len(OOB)
    return Case("ops_at_site", recs, premise, sites, site_params=[(1, 13, False), (1, 0, False)])


# ---- chunk_lanes: several sites per chunk of a long read ----
def chunk_lanes():
    # operation k covers two bases (M) or is an I / a D of one base: M I M D in turn
    def ops(n):
        return [((M, 2), (I, 1), (M, 2), (D, 1))[k % 4] for k in range(n - 1)] + [(M, 6)]
    n = 4 * LONG + 5
    whole = rec("whole", 10000, ops(n))
    far = rec("far", 12000, ops(n))                       # meets sites only where its fourth chunk lies
    far_cg = rec("far_cg", 12000, ops(n), cg=True, seed="far")
    first_ref = {}                                        # operation index -> the 1-based positions it decides
    gp = 0
    for k, (op, ln) in enumerate(ops(n)):
        if op in A.REF_OPS:
            first_ref[k] = list(range(gp + 1, gp + ln + 1)); gp += ln
    sites = [(T1, 10000 + q) for k in (0, LONG - 2, LONG - 1, LONG, 2 * LONG - 1, 2 * LONG, 3 * LONG + 4) if k in first_ref for q in first_ref[k]]
    sites += [(T1, 12000 + q) for k in range(3 * LONG, n) if k in first_ref for q in first_ref[k]]

    def premise(case):
        book = case.site_book()
        w = _entries(book, case, "whole")
        idx = [e.op_index for e in w]
        assert {0, LONG - 2, LONG - 1, LONG, 2 * LONG, 3 * LONG + 4} <= set(idx) and any(idx.count(k) == 2 for k in set(idx))   # lane 0, lane 63, lane 0 of the next chunk; two sites of one operation
        assert {e.branch for e in w} >= {"base", "del"}
        for name in ("far", "far_cg"):
            f = _entries(book, case, name)
            assert f and min(e.op_index for e in f) >= 3 * LONG and max(e.op_index for e in f) == n - 1 and all(e.long for e in f)
    return Case("chunk_lanes", [whole, far, far_cg], premise, sites)


# ---- bases_quals: every SEQ nibble at even and odd read indices, qualities around min_baseq, min_baseq up to 256 over deletions ----
BQ_VALUES = (0, 1, 13, 255, 256)
A_CODES = "=ACMGRSVTWYHKDBN"


def bases_quals():
    letters = (A_CODES + "A") * 5                      # 85 bases: every nibble at an even and at an odd index
    quals = [(0, 1, 12, 13, 14, 254, 255)[i % 7] for i in range(len(letters))]
    recs = [rec("nib", 20000, [(M, len(letters))], seq=letters, qual=quals),
            rec("nib_long", 20000, [(M, 1)] * len(letters), seq=letters, qual=quals),
            rec("del", 20030, [(M, 10), (D, 5), (M, 10)], qual=[13] * 20),
            padded("del_long", 20030, [(M, 10), (D, 5), (M, 10)], seed="del", qual=[13] * 20),
            padded("del_longcg", 20030, [(M, 10), (D, 5), (M, 10)], seed="del", qual=[13] * 20, cg=True),
            rec("qual_ff", 20000, [(M, 85)], qual=None)]
    recs[-1].qual = None                                # QUAL 0xff throughout
    sites = span_sites(recs[0])

    def premise(case):
        for bq in BQ_VALUES:
            book = case.site_book(min_baseq=bq)
            for name in ("nib", "nib_long"):
                e = _entries(book, case, name)
                other = [x for x in e if x.branch == "other"]
                assert len(e) == 85 and len(other) == 55
                for c in "=MRSVWYHKDB":                 # the letters Pileup::inc throws on, nibble 0 among them
                    assert {x.ap & 1 for x in other if case.records[x.k].seq[x.ap] == c} == {0, 1}, c
                for c in "ACGTN":
                    assert {x.ap & 1 for x in e if x.col == PM.COL[c]} == {0, 1}
            dels = [x for x in book if x.branch == "del"]
            assert {x.long for x in dels} == {False, True} and len(dels) == 15 and len({x.i for x in dels}) == 5
        want = {bq: PM.site_counts(case.records, case.sites, 1, bq, False, n_ref=len(REFS)) for bq in BQ_VALUES}
        assert want[255][:, 5].sum() == 15 and want[256][:, 5].sum() == 0 and want[256].sum() == 0          # a deleted base has quality 255
        assert want[0].sum() > want[1].sum() > want[13].sum() > want[255].sum() > 15                          # each threshold cuts between two of the qualities
        assert {q for r in case.records if r.name.startswith("nib") for q in r.qual} == {0, 1, 12, 13, 14, 254, 255}
    return Case("bases_quals", recs, premise, sites, site_params=[(1, bq, False) for bq in BQ_VALUES])


# ---- filters ----
def filters():
    ops = [(M, 10), (I, 2), (M, 10)]
    recs = []

    def both(name, pos, **kw):
        recs.append(rec(name, pos, ops, seed="f", **kw))
        recs.append(padded(name + "_long", pos, ops, seed="f", **kw))
    for f in (0x4, 0x100, 0x400, 0x800):
        both("flag%x" % f, 30100, flag=PP | f)
    both("proper", 30100)
    both("not_proper", 30100, flag=NPP)
    for mq in (0, 1, 19, 20):
        both("mapq%d" % mq, 30100, mapq=mq)
    both("no_ref", 30100, tid=-1)
    recs.append(rec("pos_neg", -1, [(M, 20)]))
    recs.append(rec("pos_neg_long", -1, [(M, 1)] * 70))
    sites = [(T1, p) for p in range(1, 75)] + [(T1, p) for p in range(30100 - PAD, 30125)]
    windows = event_windows(recs[0]) + [(T1, 1, 5, ALLELE_NONE, "", None)]

    def premise(case):
        names = {r.name for r in case.records}

        def seen(**kw):
            return {case.records[e.k].name for e in case.site_book(**kw)}
        out = {"flag4", "flag100", "flag400", "flag800", "no_ref"}
        out |= {n + "_long" for n in out}
        assert names - seen(min_mapq=0, include_npp=True) == out
        assert seen(min_mapq=0, include_npp=True) - seen(min_mapq=0) == {"not_proper", "not_proper_long"}
        assert seen(min_mapq=0) - seen(min_mapq=1) == {"mapq0", "mapq0_long"}
        assert seen(min_mapq=1) - seen(min_mapq=20) == {"mapq1", "mapq1_long", "mapq19", "mapq19_long"}
        assert {"mapq20", "mapq20_long", "pos_neg", "pos_neg_long"} <= seen(min_mapq=20)
        k = case.index_of("pos_neg")
        assert sorted(case.sites[e.i][1] for e in case.site_book() if e.k == k) == list(range(1, 20))      # pos -1: the span is 0..19, the table begins at 1
        i_ev = next(i for i, w in enumerate(case.windows) if w[3] == ALLELE_INS)
        wb = {(case.records[e.k].name, e.branch) for e in case.win_book() if e.i == i_ev}
        assert {("flag400", "filtered"), ("flag100_long", "filtered"), ("not_proper", "filtered"), ("mapq0", "mapq0"), ("mapq0_long", "mapq0"), ("mapq1", "walked"), ("proper_long", "walked")} <= wb
        assert not any(n.startswith("no_ref") for n, _ in wb)
        assert ("not_proper", "walked") in {(case.records[e.k].name, e.branch) for e in case.win_book(include_npp=True) if e.i == i_ev}
    params = [(mq, 13, npp) for mq in (0, 1, 19, 20) for npp in (False, True)]
    return Case("filters", recs, premise, sites, windows, site_params=params, win_params=(False, True))


# ---- site_table: bucket edges, record ends, a site twice, references with and without sites, a site behind the reference's end ----
def site_table():
    recs = []

    def both(name, pos, n, tid=T1):
        recs.append(rec(name, pos, [(M, n)], tid=tid))
        recs.append(rec(name + "_long", pos, [(M, 1)] * n, tid=tid))
    both("first", 0, 70)
    both("edge", BUCKET - 56, 100)                     # covers BUCKET - 55 .. BUCKET + 44
    both("edge_start", BUCKET - 1, 70)                 # its first base is position BUCKET
    both("edge_end", BUCKET - 70, 70)                  # its last base is position BUCKET
    both("edge2", 2 * BUCKET - 72, 100)                # covers 2 * BUCKET - 71 .. 2 * BUCKET + 28
    both("on_x", 500, 80, tid=TX)                      # a reference without a site, between two that have some
    both("on_y", 1000, 80, tid=TY)
    both("past_end", REFS[TY][1] - 10, 200, tid=TY)    # runs on behind the reference's end
    both("on_mt", 100, 80, tid=TMT)                    # a reference without a site behind the last that has some
    sites = [(T1, 1), (T1, 70), (T1, 71), (T1, BUCKET - 70), (T1, BUCKET - 69), (T1, BUCKET - 1), (T1, BUCKET), (T1, BUCKET), (T1, BUCKET + 1), (T1, BUCKET + 44),
             (T1, BUCKET + 45), (T1, BUCKET + 69), (T1, BUCKET + 70), (T1, 2 * BUCKET - 72), (T1, 2 * BUCKET - 71), (T1, 2 * BUCKET), (T1, 2 * BUCKET + 28), (T1, 2 * BUCKET + 29),
             (TY, 1000), (TY, 1001), (TY, 1080), (TY, 1081), (TY, REFS[TY][1]), (TY, REFS[TY][1] + 100), (TY, REFS[TY][1] + 190), (TY, REFS[TY][1] + 191)]

    def premise(case):
        book = case.site_book()
        met = {}
        for e in book:
            met.setdefault(case.sites[e.i], set()).add(case.records[e.k].name)
        assert {(T1, p) for p in (1, BUCKET - 1, BUCKET, BUCKET + 1, 2 * BUCKET)} <= set(met) and BUCKET == 65536
        assert met[T1, 70] == {"first", "first_long"} and (T1, 71) not in met and (T1, BUCKET - 70) not in met and (T1, 2 * BUCKET - 72) not in met   # the last base; one behind; one in front of the first
        assert met[T1, BUCKET - 69] == {"edge_end", "edge_end_long"} and met[T1, 2 * BUCKET - 71] == {"edge2", "edge2_long"} and "edge_start" not in met[T1, BUCKET - 1] and {"edge_start", "edge_end", "edge"} <= met[T1, BUCKET]
        assert "edge_end" not in met[T1, BUCKET + 1] and (T1, BUCKET + 70) not in met and met[T1, BUCKET + 69] == {"edge_start", "edge_start_long"}
        assert case.sites.count((T1, BUCKET)) == 2 and len({e.i for e in book if case.sites[e.i] == (T1, BUCKET)}) == 2
        assert (TY, REFS[TY][1] + 190) in met and (TY, REFS[TY][1] + 191) not in met and (TY, 1000) not in met and (TY, 1081) not in met
        assert not any(t in (TX, TMT) for t, _ in case.sites) and {r.tid for r in case.records} == {T1, TX, TY, TMT}
        assert {e.long for e in book} == {False, True}
    return Case("site_table", recs, premise, sites)


# ---- windows ----
def _w(tid, s, e, kind=ALLELE_NONE, allele=""):
    return del_window(tid, s, e, allele) if kind == ALLELE_DEL else (tid, s, e, kind, allele, None)


def windows():
    recs, wins, named = [], [], {}

    def add(name, w):
        named[name] = w
        wins.append(w)

    def both(name, pos, ops, **kw):
        recs.append(rec(name, pos, ops, **kw))
        recs.append(padded(name + "_long", pos, ops, seed=name, **kw))
        return recs[-2]
    # a window starting at 1
    r = rec("at1", 0, [(M, 1), (I, 2), (M, 20)]); recs.append(r)
    add("at1", _w(T1, 1, 3, ALLELE_INS, r.seq[1:3]))
    # window starts on both sides of a bucket edge: an I at BUCKET + 1, a D at BUCKET + 11
    r = both("edge", BUCKET - 36, [(M, 36), (I, 1), (M, 10), (D, 2), (M, 30)])
    for s in (BUCKET - 1, BUCKET, BUCKET + 1):
        add("edge%d" % (s - BUCKET), _w(T1, s, s + 2, ALLELE_INS, r.seq[36:37]))
        wins.append(_w(T1, s, BUCKET + 11, ALLELE_DEL, GENOME.seq(T1, BUCKET + 11, 2)))
    # one window 70 000 bases wide among one-base windows: tid_maxlen, and win_lower across a bucket
    add("wide", _w(T1, 1000, 70999))
    r = both("under_wide", 68990, [(M, 10), (D, 2), (M, 10)])
    add("one_base", _w(T1, 69001, 69001, ALLELE_DEL, GENOME.seq(T1, 69001, 2)))
    wins += [_w(T1, 69000, 69000), _w(T1, 69002, 69002), _w(T1, 70998, 70998)]
    # I and D at gp == start, gp == end and end + 1
    p = 3000
    both("gp", p, [(M, 10), (I, 2), (M, 10), (D, 2), (M, 10)])
    for nm, s, e in (("i_start", p + 11, p + 15), ("i_end", p + 5, p + 11), ("i_behind", p + 5, p + 10), ("d_start", p + 21, p + 22), ("d_end", p + 15, p + 21), ("d_behind", p + 15, p + 20)):
        add(nm, _w(T1, s, e))
    # a read that starts at start, one that starts at start + 1; MAPQ 0
    p = 3200
    recs.append(rec("starts_at", p, [(M, 10), (I, 1), (M, 10)]))
    recs.append(rec("starts_behind", p + 1, [(M, 9), (I, 1), (M, 10)]))
    recs.append(rec("ends_at", p - 10, [(M, 15), (I, 1), (M, 7)]))          # its last base is the window's end
    recs.append(rec("ends_before", p - 10, [(M, 15), (I, 1), (M, 6)]))
    recs.append(rec("mapq0", p, [(M, 10), (I, 1), (M, 10)], mapq=0))
    recs.append(rec("not_proper", p, [(M, 10), (I, 1), (M, 10)], flag=NPP))
    add("span", _w(T1, p + 1, p + 12))
    # an N with gp == start and gp + len == end, and one base shorter
    p = 3400
    both("n_spans", p, [(M, 10), (N, 5), (M, 10)])
    add("n_spans", _w(T1, p + 11, p + 16))
    both("n_short", p + 100, [(M, 10), (N, 4), (M, 11)])
    add("n_short", _w(T1, p + 111, p + 116))
    # two spanning N operations in one read over a one-base window: depth -1
    p = 3600
    both("two_n", p, [(M, 10), (N, 5), (I, 1), (N, 5), (M, 10)])
    add("two_n", _w(T1, p + 16, p + 16))
    # an insertion running past l_seq, with an allele equal to what is left of it; a read with l_seq = 0
    p = 3800
    r = both("ins_past", p, [(M, 10), (I, 5), (M, 10)], l_seq=13)
    add("ins_past", _w(T1, p + 10, p + 12, ALLELE_INS, r.seq[10:13]))
    wins.append(_w(T1, p + 10, p + 12, ALLELE_INS, r.seq[10:13] + "AA"))
    both("no_seq", p + 100, [(M, 10), (I, 2), (M, 10)], l_seq=0)
    add("no_seq", _w(T1, p + 110, p + 112, ALLELE_INS, ""))
    wins.append(_w(T1, p + 110, p + 112, ALLELE_INS, "AA"))
    # alleles: an INS allele that differs in its last base only; a DEL with the right length and wrong bases, with the right bases and a length off by one
    p = 4000
    r = both("alleles", p, [(M, 10), (I, 4), (M, 10), (D, 3), (M, 10)])
    ins = r.seq[10:14]
    add("ins_right", _w(T1, p + 10, p + 12, ALLELE_INS, ins))
    add("ins_last", _w(T1, p + 10, p + 12, ALLELE_INS, ins[:3] + ("A" if ins[3] != "A" else "C")))
    dele = GENOME.seq(T1, p + 21, 3)
    add("del_right", _w(T1, p + 20, p + 22, ALLELE_DEL, dele))
    add("del_wrong", _w(T1, p + 20, p + 22, ALLELE_DEL, dele[:2] + ("A" if dele[2] != "A" else "C")))
    add("del_longer", _w(T1, p + 20, p + 22, ALLELE_DEL, GENOME.seq(T1, p + 21, 4)))
    add("del_shorter", _w(T1, p + 20, p + 22, ALLELE_DEL, dele[:2]))
    # a deletion reaching past the contig end: a zero-padded slice
    L = REFS[TMT][1]
    both("past_end", L - 20, [(M, 15), (D, 10), (M, 5)], tid=TMT)
    add("past_end5", _w(TMT, L - 5, L - 3, ALLELE_DEL, GENOME.seq(TMT, L - 4, 10)))
    add("past_end10", _w(TMT, L - 5, L - 3, ALLELE_DEL, GENOME.seq(TMT, L - 4, 10) + "ACGTA"))
    # long records: an I at operation index 63 and a D at index 64; an I in the third chunk, its read position behind both carries
    p = 5000
    r = rec("chunk_edge", p, [(M, 2)] * (LONG - 1) + [(I, 2), (D, 3)] + [(M, 2)] * 10); recs.append(r)
    wins += event_windows(r)
    r = rec("third", p + 500, [(S, 3)] + [(M, 2), (I, 1)] * 70 + [(M, 5)]); recs.append(r)
    recs.append(rec("third_cg", p + 500, [(S, 3)] + [(M, 2), (I, 1)] * 70 + [(M, 5)], cg=True, seed="third"))
    third = [w for w in event_windows(r, wrong=False) if w[1] + 1 - (p + 501) in (2 * 64, 2 * 65, 2 * 69, 2 * 70)]
    wins += third
    # an unknown operation in a spanning read with no I, D or N: no error
    p = 6000
    both("p_plain", p, [(M, 10), (P, 1), (M, 10)])
    both("op9_plain", p, [(M, 10), (OP9, 1), (M, 10)])
    recs.append(rec("p_idn_not_spanning", p + 4, [(M, 6), (I, 1), (P, 1), (M, 10)]))
    recs.append(rec("p_idn_not_spanning_long", p + 4, [(M, 1)] * PAD + [(I, 1), (P, 1), (M, 10)]))
    add("p_plain", _w(T1, p + 2, p + 12))

    def premise(case):
        book = case.win_book(include_npp=True)
        want = PM.window_counts(case.records, case.windows, True, GENOME.seq)
        assert want[:, PM.W_UNKNOWN].sum() == 0

        def row(name):
            return want[case.windows.index(named[name])].tolist()

        def names(name, branch):
            i = case.windows.index(named[name])
            return {case.records[e.k].name for e in book if e.i == i and e.branch == branch}
        assert case.windows[0][1] == 1 and row("at1")[2:] == [1, 1, 0, 1, 0]
        assert [row("edge%d" % d)[PM.W_INS] for d in (-1, 0, 1)] == [2, 2, 2] and [named["edge%d" % d][1] for d in (-1, 0, 1)] == [65535, 65536, 65537]
        assert row("wide")[PM.W_MAPPED] > 20 and row("wide")[PM.W_DEPTH] == 0 and row("one_base")[2:] == [2, 0, 2, 2, 0]
        assert [row(n)[PM.W_INS] for n in ("i_start", "i_end", "i_behind")] == [2, 2, 0] and [row(n)[PM.W_DEL] for n in ("d_start", "d_end", "d_behind")] == [2, 2, 0]
        assert all(row(n)[PM.W_DEPTH] == 2 for n in ("i_start", "i_end", "i_behind", "d_start", "d_end", "d_behind"))
        assert names("span", "walked") == {"starts_at", "ends_at", "not_proper"} and names("span", "not_spanning") == {"starts_behind", "ends_before"} and names("span", "mapq0") == {"mapq0"}
        assert row("span") == [6, 1, 3, 3, 0, 0, 0]
        assert row("n_spans")[PM.W_DEPTH] == 0 and row("n_short")[PM.W_DEPTH] == 2 and row("two_n")[2:4] == [-2, 2]     # (a short and a padded read each: -1 apiece)
        assert row("ins_past")[3:6] == [2, 0, 2] and row("no_seq")[3:6] == [2, 0, 2]
        assert [row(n)[PM.W_MATCH] for n in ("ins_right", "ins_last", "del_right", "del_wrong", "del_longer", "del_shorter")] == [2, 0, 2, 0, 0, 0]
        assert row("past_end5")[4:6] == [2, 2] and row("past_end10")[4:6] == [2, 0] and len(GENOME.seq(TMT, L - 4, 10)) == 5   # FastaFileIndex::seq ends at the contig's end: "-" and five bases
        ce = [e for e in book if case.records[e.k].name == "chunk_edge" and e.branch == "walked"]
        assert {(k, op) for e in ce for k, op, _, _, counted in e.events if counted} == {(LONG - 1, I), (LONG, D)}
        th = [e for e in book if case.records[e.k].name == "third" and e.branch == "walked"]
        assert th and {k // LONG for e in th for k, op, _, _, counted in e.events if counted} == {2} and want[[case.windows.index(w) for w in third], PM.W_MATCH].tolist() == [2] * len(third)
        assert names("p_plain", "no_idn") == {"p_plain", "p_plain_long", "op9_plain", "op9_plain_long"} and names("p_plain", "not_spanning") == {"p_idn_not_spanning", "p_idn_not_spanning_long"}
        assert row("p_plain")[:3] == [6, 0, 4]
        long_walked = {case.records[e.k].name for e in book if e.branch == "walked" and e.long}
        assert len(long_walked) >= 12 and len({case.records[e.k].name for e in book if e.branch == "walked" and not e.long}) >= 12
    return Case("windows", recs, premise, windows=wins, win_params=(True, False))


def _unknown(name, long):
    def build():
        ops = [(M, 10), (I, 2), (P, 1), (M, 10)]
        mk = padded if long else rec
        recs = [mk("p_idn", 7000, ops), rec("plain", 7000, [(M, 10), (I, 2), (M, 11)])]
        wins = [_w(T1, 6000, 6001), _w(T1, 7005, 7015), _w(T1, 7018, 7022)]

        def premise(case):
            want = PM.window_counts(case.records, case.windows, False, GENOME.seq)
            assert want[:, PM.W_UNKNOWN].tolist() == [0, 1, 0]              # the spanned window throws; the one the read merely overlaps does not
            e = [x for x in case.win_book() if x.branch == "unknown"]
            assert len(e) == 1 and e[0].long == long and e[0].i == 1
        return Case(name, recs, premise, windows=wins, raises=True)
    build.__name__ = name
    return build


win_unknown_short, win_unknown_long = _unknown("win_unknown_short", False), _unknown("win_unknown_long", True)

BUILDERS = (two_forms, ops_at_site, chunk_lanes, bases_quals, filters, site_table, windows, win_unknown_short, win_unknown_long)
NAMES = tuple(b.__name__ for b in BUILDERS)
SITE_CASES = ("two_forms", "ops_at_site", "chunk_lanes", "bases_quals", "filters", "site_table")
WINDOW_CASES = ("two_forms", "filters", "windows")
RAISING = ("win_unknown_short", "win_unknown_long")
_made = {}


def case(name):
    """made once and shared: nobody writes to a case"""
    if name not in _made:
        _made[name] = BUILDERS[NAMES.index(name)]()
    return _made[name]
