"""Designed inputs for BamToFastq's kernels (csrc/fastq.hip over csrc/tofastq_visit.h and csrc/join.h): named runs, each the records in file order, the tile
every record lies in (one BGZF member per tile: run with NGSQC_TILE_MEMBERS=1), the options, and its premises as assertions. The expectations are
bamtofastq_oracle.to_fastq's. tests/test_cpu_tofastq_designed.py runs every record through the CPU build of the kernels' per-entry text,
tests/test_gpu_tofastq_designed.py every run through Handle.to_fastq."""
import bamtofastq_oracle as Q
from bamfilter_oracle import Rec
from join_cases import F1, F2, PIECE, Case, _search, collide, rec, _cg_record

REV = 0x10
NT16 = Q.NT16


def pack(seq):
    codes = [NT16.index(c) for c in seq] + ([0] if len(seq) & 1 else [])
    return bytes(codes[i] << 4 | codes[i + 1] for i in range(0, len(codes), 2))


def fq(name, flag, seq, qual=None, **kw):
    qual = qual if qual is not None else [20 + i % 50 for i in range(len(seq))]
    return rec(name, flag, l_seq=len(seq), seq=pack(seq), qual=bytes(qual), **kw)


class Run(Case):
    def __init__(self, name, tiles, kw=None, error=None, **notes):
        super().__init__(name, tiles, **notes)
        self.kw, self.error = kw or {}, error

    def expected(self):
        """(out1, out2, counts), or the base of the ComplementError"""
        try:
            return Q.to_fastq(self.records, **self.kw)
        except Q.ComplementError as e:
            return e.base


def pairs_of(probes):
    """every probe (name, flag bits, seq, qual) as a pair: the probe as read 1 and, mirrored to the other strand, as read 2"""
    out = []
    for nm, fl, seq, qual in probes:
        out += [fq(nm, F1 | fl, seq, qual), fq(nm, F2 | (fl ^ REV if all(c in "ACGTN" for c in seq) else fl), seq, qual)]
    return out


def bases():
    acgtn = "ACGTNNTGCAAN"
    probes = [("all16", 0, NT16, None), ("rev", REV, acgtn, None)]
    for n in (0, 1, 2, 3, 64, 65):   # (the nibble of base l_seq - 1 - k: both parities, an odd count's padding nibble)
        s = (acgtn * 6)[:n]
        probes += [("f%d" % n, 0, s, None), ("r%d" % n, REV, s, None)]
    r = Run("bases", [pairs_of(probes)])
    e1, e2, c = r.expected()
    assert b"@all16\n=ACMGRSVTWYHKDBN\n" in e1 and b"@rev\nNTTGCANNACGT\n" in e1 and b"@r0\n\n+\n\n" in e1 and c["paired"] == len(probes)
    assert b"@r65\n" + "".join(Q.COMP[ch] for ch in reversed((acgtn * 6)[:65])).encode() + b"\n" in e1
    return [r, Run("bases_single_end", r.tiles, dict(paired=False))]


def qualities():
    s = "ACGTACGT"
    probes = [("q0", 0, s, [0] * 8), ("q93", REV, s, [93] * 8), ("q222", 0, s, [222] * 8), ("wrap", 0, "ACGT" * 8, list(range(224, 256))), ("wrapr", REV, "ACGT" * 8, list(range(224, 256)))]
    for where, at in (("first", 0), ("mid", 4), ("last", 7)):
        q = [30 + k for k in range(8)]; q[at] = 223
        probes += [("nul_%s_f" % where, 0, s, q), ("nul_%s_r" % where, REV, s, q)]
    probes += [("two_nul", 0, s, [30, 223, 31, 223, 32, 33, 34, 35]), ("two_nul_r", REV, s, [30, 223, 31, 223, 32, 33, 34, 35]), ("plain", REV, s, None)]
    tiles = [pairs_of(probes)]
    runs = [Run("qualities_extend%d" % x, tiles, dict(extend=x)) for x in (0, 5, 8, 9, 12)]   # (l_seq 8: below, at, above; 32: below)
    e1, _, _ = runs[0].expected()
    assert b"@q0\nACGTACGT\n+\n!!!!!!!!\n" in e1 and b"@nul_first_f\nACGTACGT\n+\n\n" in e1 and b"@nul_last_r\nACGTACGT\n+\n\n" in e1
    assert b"@nul_first_r\nACGTACGT\n+\nFEDCBA@\n" in e1 and b"@wrap\n" + b"ACGT" * 8 + b"\n+\n" + bytes(range(1, 33)) + b"\n" in e1   # (224 + 33 wraps to 1)
    x1, _, _ = runs[4].expected()
    assert b"@nul_mid_f\nACGTACGTNNNN\n+\n?@AB\n" in x1 and b"@plain\nACGTACGTNNNN\n+\n" + bytes(33 + 20 + k for k in reversed(range(8))) + b"####\n" in x1
    return runs


def throws():
    ok = lambda nm, fl: fq(nm, fl, "ACGT")
    bad = lambda nm, fl, seq: fq(nm, fl | REV, seq)
    # output order is the order of the closing records, read 1 before read 2: pair y closes first (its read 2 throws 'R'), x's opener lies first in the file
    recs = [bad("x", F1, "AYCG"), ok("y", F1), bad("y", F2, "ARSG"), ok("x", F2), bad("z", F1, "AKCG"), ok("z", F2)]
    runs = [Run("throws_in_tile", [recs], error="S"), Run("throws_across_tiles", [recs[:2], recs[2:3], recs[3:]], error="S"),
            Run("throws_opener_from_held", [[recs[0], ok("w", F1)], [ok("w", F2)], [recs[3], recs[4], recs[5]]], error="Y"),
            Run("throws_e1_before_e2", [[bad("p", F2, "AMCG"), bad("p", F1, "AWCG")]], error="W"),
            Run("throws_e2_alone", [[ok("p", F1), ok("q", F1), ok("q", F2)], [bad("p", F2, "DACGB")]], error="B"),
            Run("throws_unmatched", [[bad("u", F1, "AYCG"), ok("v", F1)], [ok("v", F2)]]),
            Run("throws_single_end", [[ok("a", 0), bad("b", 0, "AHVG"), bad("c", 0, "AYCG")]], dict(paired=False), error="V"),
            Run("throws_0x900_is_skipped", [[bad("s", 0x100 | F1, "AYCG"), ok("s", F1), ok("s", F2)]])]
    for r in runs:
        e = r.expected()
        assert (e == r.error) if r.error else isinstance(e, tuple), r.name
    return runs


def fix():
    a, b, c = _search(b"fx%d", 3)
    f = lambda nm, fl, **kw: fq(nm + b"\0", fl, "ACGTA", **kw)
    T = [[f(a, F1), f(b, F1), f(c, F2), f(a, F2)],
         [f(b, F1), f(a, F1), f(c, F1), f(b, F2), f(b"un", 0), f(b"dup", F1 | 0x400), f(b"dup", F1), f(b"dup", F2)],
         [f(a, F1), f(c, F2), f(b"un", 0), f(c, F1), f(b, F2), f(b"dup", F1)]]
    assert collide(a, b) and collide(a, c)
    runs = [Run("fix", T, dict(fix=True)), Run("fix_remove_duplicates", T, dict(fix=True, remove_duplicates=True)), Run("fix_single_end", T, dict(fix=True, paired=False)),
            Run("no_fix", T)]
    c0, c1 = runs[0].expected()[2], runs[1].expected()[2]
    # (a, read 1) three times over three tiles; with -remove_duplicates the flagged first copy of dup never reaches the set, so the second stays and pairs
    assert c0["fixed"] == 9 and c0["unpaired"] == 1 and c1["duplicates"] == 1 and c1["fixed"] == 8 and c1["paired"] == c0["paired"] == 4
    return runs


def region():
    S, E = 1000, 2000   # 1-based closed
    m = lambda nm, pos, n, **kw: [fq(nm, fl, "ACGT" * 5, pos=pos, cigar=[n << 4] if n else [], **kw) for fl in (F1, F2)]
    cg = lambda nm, pos: [_cg_record(nm, fl, 60, pos=pos, n_len=1) for fl in (F1, F2)]   # (the placeholder alone would end at pos + 1)
    recs = (m("pos_end-1", E - 1, 20) + m("pos_end", E, 20) + m("endpos_start-1", S - 1 - 20, 20) + m("endpos_start", S - 20, 20)
            + [fq("um_out", fl | 4, "ACGT", pos=S - 2) for fl in (F1, F2)] + [fq("um_in", fl | 4, "ACGT", pos=S - 1) for fl in (F1, F2)]
            + cg("cg_in", S - 20) + cg("cg_out", S - 31) + m("other_tid", 1500, 20, tid=1) + m("no_cigar_out", S - 2, 0) + m("no_cigar_in", S - 1, 0)
            + [fq("in", F1 | 0x100, "ACGT", pos=1500), fq("in", F2 | 0x800, "ACGT", pos=1500)] + m("in", 1500, 20))
    runs = [Run("region", [recs[:9], recs[9:]], dict(region=(0, S, E))), Run("region_single_end", [recs], dict(region=(0, S, E), paired=False))]
    e1, _, c = runs[0].expected()
    names = [l[1:] for l in e1.split(b"\n")[0::4] if l]
    assert names == [b"pos_end-1", b"endpos_start", b"um_in", b"cg_in", b"no_cigar_in", b"in"] and c["unmatched"] == 0
    r = Rec(cg("cg_in", S - 20)[0])
    assert len(r.cg()[0]) == 60 and Q.endpos(r) == S - 20 + 30 and r.pos + (r.cigar[1] >> 4) == S - 19   # 30 M from the tag; the placeholder alone ends in front of the region
    return runs


def max_cached():
    o = lambda k: fq("m%d" % k, F1, "ACGT")
    c = lambda k: fq("m%d" % k, F2, "ACGT")
    inside = Run("max_cached_inside_a_tile", [[o(0)], [o(1), o(2), o(3), c(1), c(2), c(3)], [c(0)]])
    border = Run("max_cached_at_a_border", [[o(0), o(1), o(2), o(3)], [c(0), c(1), o(4), c(2)], [c(3), c(4)]])
    assert inside.expected()[2]["max_cached"] == 4 and border.expected()[2]["max_cached"] == 4
    return [inside, border]


def small_runs():
    return bases() + qualities() + throws() + fix() + region() + max_cached()


def _sized(nm_prefix, size, k):
    """(name, seq) of an entry of `size` bytes: "@" name "\\n" seq "\\n+\\n" qual "\\n" = len(name) + 2 l_seq + 6"""
    assert size >= 6
    l = (size - 6) // 2
    nl = size - 6 - 2 * l
    if l >= 8:   # room for a name that tells the probes apart
        tag = ("%s%d" % (nm_prefix, k)).encode()
        l -= (len(tag) + 1) // 2; nl = size - 6 - 2 * l
        name = tag + b"_" * (nl - len(tag))
    else:
        name = b"_" * nl
    assert len(name) == nl and len(name) + 2 * l + 6 == size
    return name, ("ACGTN" * (l // 5 + 1))[:l]


def format_cuts():
    """NGSQC_WRITE_WINDOW_PIECES=1. Part 1: entries of 6..13 and 255..262 bytes at every alignment mod 4 of their stream (a spacer in front gives the
    alignment). Part 2: probes cut by a window end `cut` bytes behind their start: cut = c for c = 1..7, and size - c for sizes 40..43 (the window ends are
    multiples of 4, so the cuts give every alignment of a probe's start and of its end); two filler pairs of about 16 000 bases reach each window end.
    Every pair is (entry as read 1, the same entry as read 2): both streams have one layout. notes: probes [(stream offset, size)], cuts [(offset, size, cut)]"""
    recs, probes, cuts, cur, k = [], [], [], 0, 0

    def add(name, seq, fl=0):
        nonlocal cur
        recs.extend([fq(name + b"\0", F1 | fl, seq), fq(name + b"\0", F2 | fl, seq)])
        cur += len(name) + 2 * len(seq) + 6

    for al in range(4):
        for size in list(range(6, 14)) + list(range(255, 263)):
            nl = (al - cur - 8) % 4 + 4   # a spacer "@name\nA\n+\nq\n" of nl + 8 bytes
            add(b"s%03d" % k + b"_" * (nl - 4), "A")
            assert cur % 4 == al
            name, seq = _sized("p", size, k)
            # (names repeat among the short probes: each pair closes before the next opens)
            probes.append((cur, size)); add(name, seq, REV if k % 3 == 0 else 0); k += 1
    plan = [(40, c) for c in range(1, 8)] + [(size, size - c) for size in (40, 41, 42, 43) for c in range(1, 8)]
    for size, cut in plan:
        need = (-(cur + cut)) % PIECE
        while need < 32000:
            need += PIECE
        half = need // 2
        for part in (half, need - half):
            name, seq = _sized("fill", part, k); k += 1
            add(name, seq)
        name, seq = _sized("c", size, k)
        cuts.append((cur, size, cut)); add(name, seq, REV if k % 2 else 0); k += 1
    add(b"tail", "ACGT")
    tiles, t, n = [], [], 0
    for i in range(0, len(recs), 2):   # tiles of about 50 KB of whole pairs
        if t and n > 50000:
            tiles.append(t); t, n = [], 0
        t += recs[i:i + 2]; n += len(recs[i]) + len(recs[i + 1])
    tiles.append(t)
    return Run("format_cuts", tiles, probes=probes, cuts=cuts)


def format_cut_premises(run, out1, out2):
    """out1 / out2: the oracle's texts. Every probe lies at its offset with its size, every designed window end inside its probe at the designed cut"""
    for out in (out1, out2):
        seen = set()
        for at, size in run.notes["probes"]:
            assert out[at:at + 1] == b"@" and out[at + size - 1:at + size + 1] == b"\n@" and out[at:at + size].count(b"\n") == 4, (at, size)
            seen.add((size, at % 4))
        assert seen == {(s, al) for s in list(range(6, 14)) + list(range(255, 263)) for al in range(4)}
        starts, ends = set(), set()
        for at, size, cut in run.notes["cuts"]:
            assert (at + cut) % PIECE == 0 and 0 < cut < size and out[at:at + 2] == b"@c" and out[at + size - 1:at + size + 1] == b"\n@", (at, size, cut)
            starts.add(at % 4); ends.add((at + size) % 4)
        assert starts == ends == {0, 1, 2, 3} and len(run.notes["cuts"]) == 35
    assert len(out1) == len(out2) and len(out1) < 4 << 20
