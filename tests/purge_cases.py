"""Designed read pairs for SeqPurge (tests/seqpurge_oracle.py is the model, src/SeqPurge/AnalysisWorker.cpp the reference): groups of pairs that share one set
of parameters, every pair with its premise - the plan columns it was built to produce. tests/test_cpu_seqpurge.py has the model assert every premise, so a
case that does not show what its name says fails there and not in the comparisons that use it. synthetic() is the input of the timing record."""
import random

import numpy as np

import seqpurge_oracle as M

A1, A2 = M.A1_DEFAULT, M.A2_DEFAULT
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
COL = {c: i for i, c in enumerate(M.PLAN_COLUMNS)}


def rc(s):
    return bytes(s).translate(_COMP)[::-1]


def rnd(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def other(c):
    return {65: 67, 67: 71, 71: 84, 84: 65}[c]


def mutate(s, positions):
    s = bytearray(s)
    for p in positions:
        s[p] = other(s[p])
    return bytes(s)


class Case:
    def __init__(self, name, r1, r2, q1=None, q2=None, h1=None, h2=None, premise=None, error=None):
        self.name, self.r1, self.r2 = name, bytes(r1), bytes(r2)
        self.q1 = bytes(q1) if q1 is not None else b"I" * len(r1)
        self.q2 = bytes(q2) if q2 is not None else b"I" * len(r2)
        self.h1, self.h2 = h1, h2
        self.premise = premise or {}    # plan column -> value
        self.error = error              # (kind, start of the message) of a pair that is refused


class Group:
    def __init__(self, name, params, out3=False):
        self.name, self.kw, self.out3, self.cases = name, params, out3, []

    def params(self):
        return M.Params(out3=self.out3, **self.kw)

    def add(self, *a, **k):
        self.cases.append(Case(*a, **k))

    def texts(self, crlf=False, final_newline=True):
        eol = b"\r\n" if crlf else b"\n"
        t = [[], []]
        for i, c in enumerate(self.cases):
            h1 = c.h1 if c.h1 is not None else b"@%s:%d" % (self.name.encode(), i)
            h2 = c.h2 if c.h2 is not None else h1
            t[0] += [h1, c.r1, b"+", c.q1]
            t[1] += [h2, c.r2, b"+", c.q2]
        out = [eol.join(x) + (eol if final_newline else b"") for x in t]
        return out[0], out[1]


def insert_pair(rng, len1, len2, offset, a1=A1, a2=A2, x1=0, x2=0):
    """a pair whose insert match is at `offset` (the fragment has len2 - offset bases), the adapters behind it with x1 / x2 substitutions in their first bases"""
    ins = len2 - offset
    frag = rnd(rng, ins)
    t1, t2 = mutate(a1, range(x1)) + rnd(rng, len1), mutate(a2, range(x2)) + rnd(rng, len2)
    return (frag + t1)[:len1], (rc(frag) + t2)[:len2]


def catalogue():
    rng = random.Random(20251)
    G = []
    base = dict(qcut=0, ncut=0, min_len=15)

    g = Group("plain", base)
    for n in (0, 1, 4, 63, 64, 65, 128, 129, 999):
        g.add("unrelated reads of length %d" % n, rnd(rng, n), rnd(rng, n), premise=dict(len1_in=n, len2_in=n, insert_offset=-1, adapter_fwd=-1, adapter_rev=-1, len1_out=n, len2_out=n))
    for n in (63, 64, 65, 128, 129, 999):
        r1, r2 = insert_pair(rng, n, n, 20)
        g.add("insert hit at offset 20, length %d" % n, r1, r2, premise=dict(insert_offset=20, len1_out=n - 20, len2_out=n - 20))
    for off in (1, 2, 3, 5, 6, 9):
        mm = 0 if off < 3 else 1 if off < 6 else 2
        r1, r2 = insert_pair(rng, 100, 100, off, x1=mm, x2=mm)
        g.add("offset %d, %d adapter mismatches on both sides: inside the budget" % (off, mm), r1, r2, premise=dict(insert_offset=off, len1_out=100 - off, len2_out=100 - off))
        r1, r2 = insert_pair(rng, 100, 100, off, x1=mm + 1, x2=mm + 1)
        g.add("offset %d, %d adapter mismatches on both sides: outside" % (off, mm + 1), r1, r2, premise=dict(insert_offset=-1))
        r1, r2 = insert_pair(rng, 100, 100, off, x1=mm + 1, x2=mm)
        g.add("offset %d, one side outside the budget, one inside" % off, r1, r2, premise=dict(insert_offset=off))
    for off in (10, 11):
        r1, r2 = insert_pair(rng, 100, 100, off, x1=2, x2=2)
        g.add("offset %d, tail(8,10)^2 <= mep: inside" % off, r1, r2, premise=dict(insert_offset=off))
        r1, r2 = insert_pair(rng, 100, 100, off, x1=3, x2=2)
        g.add("offset %d, tail(7,10) * tail(8,10) > mep: outside" % off, r1, r2, premise=dict(insert_offset=-1))
    # unequal lengths
    r1, r2 = insert_pair(rng, 80, 100, 30)
    g.add("len1 < len2, adapter visible in read 1", r1, r2, premise=dict(len1_in=80, len2_in=100, insert_offset=30, len1_out=70, len2_out=70))
    r1, r2 = insert_pair(rng, 100, 80, 30)
    g.add("len1 > len2", r1, r2, premise=dict(insert_offset=30, len1_out=50, len2_out=50))
    r1, r2 = insert_pair(rng, 50, 100, 20)
    g.add("len2 - offset lies beyond read 1: the adapter slice is empty", r1, r2, premise=dict(insert_offset=20, len1_out=50, len2_out=80))
    # N handling
    r1, r2 = insert_pair(rng, 100, 100, 25)
    r1n, r2n = bytearray(r1), bytearray(r2)
    for p in (3, 4, 40, 70):
        r1n[p] = 78
    for p in (10, 11, 60):
        r2n[p] = 78
    g.add("N at compared positions", r1n, r2n, premise=dict(insert_offset=25))
    g.add("read 1 all N", b"N" * 100, rnd(rng, 100), premise=dict(insert_offset=-1, adapter_fwd=-1, adapter_rev=-1, len1_out=100))
    g.add("both reads all N", b"N" * 100, b"N" * 100, premise=dict(insert_offset=-1, adapter_fwd=-1, adapter_rev=-1))
    r1o = bytearray(r1); r1o[5] = ord("R"); r1o[50] = ord("n")
    g.add("bytes outside ACGTN in read 1 are mismatches", r1o, r2, premise=dict(insert_offset=25))
    # adapter-only hits
    u = rnd(rng, 100)
    g.add("adapter 1 at offset 0", (A1 + rnd(rng, 100))[:100], u, premise=dict(insert_offset=-1, adapter_fwd=0, adapter_rev=-1, len1_out=0, len2_out=0))
    g.add("adapter 1 at offset 37", (rnd(rng, 37) + A1 + rnd(rng, 100))[:100], rnd(rng, 100), premise=dict(insert_offset=-1, adapter_fwd=37, adapter_rev=-1, len1_out=37, len2_out=37))
    g.add("adapter 2 at offset 41, read 2 only", rnd(rng, 100), (rnd(rng, 41) + A2 + rnd(rng, 100))[:100], premise=dict(insert_offset=-1, adapter_fwd=-1, adapter_rev=41, len1_out=41, len2_out=41))
    for k, hit in ((9, False), (10, True), (11, True)):
        body = rnd(rng, 100 - k - 1) + bytes([other(A1[0])])   # (the base in front is not the adapter's first: no window one to the left)
        g.add("adapter 1 as a partial window of %d bases at the end" % k, body + A1[:k], rnd(rng, 100), premise=dict(insert_offset=-1, adapter_fwd=(100 - k) if hit else -1))
    # headers
    r1, r2 = insert_pair(rng, 70, 70, 12)
    g.add("headers with /1 and /2", r1, r2, h1=b"@read/1", h2=b"@read/2", premise=dict(insert_offset=12))
    g.add("headers with comments", r1, r2, h1=b"@read 1:N:0:AAA", h2=b"@read 2:N:0:AAA", premise=dict(insert_offset=12))
    g.add("headers with /1, /2 and comments", r1, r2, h1=b"@read/1 x y", h2=b"@read/2 z", premise=dict(insert_offset=12))
    G.append(g)

    # every lane of the plan kernel's wave, and its second and third pass over the offsets
    g = Group("lanes", base)
    for off in list(range(10, 76)) + [127, 128, 129, 191, 192, 193]:
        for len1, len2 in ((230, 230),) if off % 3 else ((230, 230), (217, 230), (230, 211)):
            r1, r2 = insert_pair(rng, len1, len2, off)
            new = len2 - off
            g.add("insert hit at offset %d, lengths %d / %d" % (off, len1, len2), r1, r2, premise=dict(insert_offset=off, len1_out=min(len1, new), len2_out=new))
    G.append(g)

    # equal p: a read of period 7 against itself, adapters of the same period: every offset 7k matches everywhere, 4^-(700 - 7k) is 0.0 for both 7 and 14
    unit = b"ACGTTGC"
    g = Group("period", dict(a1=unit * 3, a2=rc(unit) * 3, **base))
    w = unit * 100
    g.add("two offsets with p = 0.0: the first is kept", w, rc(w), premise=dict(insert_offset=7, len1_out=693, len2_out=693))
    # the same at length 98, where offset 7 carries seven mismatches (seq2[7..14) is compared at offset 7 only): 14 has the smaller p
    w = unit * 14
    s2 = mutate(w, range(7, 14))
    g.add("a later offset with smaller p", w, rc(s2), premise=dict(insert_offset=14, len1_out=84, len2_out=84))
    G.append(g)

    g = Group("quality", dict(qcut=15, qwin=5, ncut=0, min_len=15))
    r = rnd(rng, 70)
    g.add("the whole read passes", r, rnd(rng, 70), premise=dict(len1_out=70, len2_out=70, flags=0))
    g.add("no window passes", r, rnd(rng, 70), q1=b"#" * 70, premise=dict(len1_out=0, len2_out=70, flags=1))
    g.add("the tail is stripped inside the window", r, rnd(rng, 70), q2=b"I" * 50 + b"#" * 20, premise=dict(len1_out=70, len2_out=50, flags=2))
    g.add("a low base inside, high bases behind it", r, rnd(rng, 70), q1=b"I" * 30 + b"#" + b"I" * 39, premise=dict(len1_out=70, flags=0))
    g.add("shorter than the window", rnd(rng, 4), rnd(rng, 4), q1=b"####", q2=b"####", premise=dict(len1_out=4, len2_out=4, flags=0))
    g.add("exactly one window, failing", rnd(rng, 5), rnd(rng, 5), q1=b"#####", q2=b"IIIII", premise=dict(len1_out=0, len2_out=5, flags=1))
    g.add("mean exactly at the cutoff", r, rnd(rng, 70), q1=b"#" * 65 + b"00000", premise=dict(len1_out=70, flags=0))
    g.add("more than 64 windows fail before one passes", rnd(rng, 200), rnd(rng, 200), q1=b"I" * 100 + b"#" * 100, premise=dict(len1_out=100, len2_out=200, flags=1))
    G.append(g)

    g = Group("nruns", dict(qcut=0, ncut=7, min_len=15))
    r = rnd(rng, 90)
    g.add("a run of ncut - 1", r[:20] + b"N" * 6 + r[26:], rnd(rng, 90), premise=dict(len1_out=90, flags=0))
    g.add("a run of ncut", r[:20] + b"N" * 7 + r[27:], rnd(rng, 90), premise=dict(len1_out=20, flags=4))
    g.add("a run at the start", rnd(rng, 90), b"N" * 7 + r[7:], premise=dict(len2_out=0, flags=8))
    g.add("a run at the end", r[:83] + b"N" * 7, rnd(rng, 90), premise=dict(len1_out=83, flags=4))
    g.add("a run behind position 64", rnd(rng, 150) + b"N" * 8 + rnd(rng, 10), rnd(rng, 168), premise=dict(len1_out=150, flags=4))
    g.add("shorter than ncut", b"NNNNNN", b"NNNNNN", premise=dict(len1_out=6, len2_out=6, flags=0))
    G.append(g)

    for out3 in (False, True):
        g = Group("route%d" % out3, dict(qcut=15, qwin=5, ncut=0, min_len=30), out3=out3)
        hi, lo = b"I" * 60, b"I" * 10 + b"#" * 50
        g.add("both long enough", rnd(rng, 60), rnd(rng, 60), q1=hi, q2=hi, premise=dict(len1_out=60, len2_out=60))
        g.add("only read 1 long enough", rnd(rng, 60), rnd(rng, 60), q1=hi, q2=lo, premise=dict(len1_out=60, len2_out=10))
        g.add("only read 2 long enough", rnd(rng, 60), rnd(rng, 60), q1=lo, q2=hi, premise=dict(len1_out=10, len2_out=60))
        g.add("neither", rnd(rng, 60), rnd(rng, 60), q1=lo, q2=lo, premise=dict(len1_out=10, len2_out=10))
        g.add("exactly min_len", rnd(rng, 60), rnd(rng, 60), q1=b"I" * 30 + b"#" * 30, q2=b"I" * 29 + b"#" * 31, premise=dict(len1_out=30, len2_out=29))
        G.append(g)

    g = Group("ec", dict(qcut=0, ncut=0, min_len=15, ec=True))
    r1, r2 = insert_pair(rng, 100, 100, 20)      # 80 bases overlap: position i of read 1 pairs with 79 - i of read 2
    bad = mutate(r1, [10, 30, 50])
    q1 = bytearray(b"5" * 100); q1[10], q1[30], q1[50] = ord("I"), ord("#"), ord("5")
    g.add("q1 > q2, q1 < q2 and q1 == q2", bad, r2, q1=q1, q2=b"5" * 100, premise=dict(insert_offset=20, len1_out=80, len2_out=80))
    r1, r2 = insert_pair(rng, 60, 100, 20)
    g.add("unequal lengths after truncation", mutate(r1, [5]), r2, q1=b"#" * 60, premise=dict(insert_offset=20, len1_out=60, len2_out=80))
    r1, r2 = insert_pair(rng, 100, 100, 20)
    g.add("no mismatch", r1, r2, premise=dict(insert_offset=20))
    G.append(g)
    return G


def error_cases():
    """(name, text1, text2, kind, pair, start of the message): runs that stop with an error; the first failing pair wins"""
    rng = random.Random(7)
    ok = Case("ok", rnd(rng, 50), rnd(rng, 50))

    def texts(cases):
        g = Group("err", {})
        g.cases = cases
        return g.texts()
    out = []
    out.append(("mismatching headers",) + texts([ok, Case("h", rnd(rng, 50), rnd(rng, 50), h1=b"@a/1 c", h2=b"@b/2 c")]) + (M.ERR_HEADER, 1, "Headers of reads do not match:\n@a\n@b"))
    out.append(("/1 without /2",) + texts([Case("h", rnd(rng, 50), rnd(rng, 50), h1=b"@a/1", h2=b"@a")]) + (M.ERR_HEADER, 0, "Headers of reads do not match:\n@a/1\n@a"))
    out.append(("a bad base in read 2",) + texts([ok, ok, Case("b", rnd(rng, 50), rnd(rng, 20) + b"x" + rnd(rng, 20) + b"R" + rnd(rng, 8))]) + (M.ERR_BASE, 2, "Could not convert base 'R' to complement!"))
    out.append(("length 1000",) + texts([ok, Case("l", rnd(rng, 1000), rnd(rng, 50))]) + (M.ERR_READLEN, 1, "Read length unsupported! A maximum read length of 1000 is supported!"))
    out.append(("bases and qualities differ",) + texts([Case("q", rnd(rng, 50), rnd(rng, 50), q2=b"I" * 49)]) + (M.ERR_LENGTHS, 0, "Differing length of bases (50) and qualities (49) in read 2 of pair 0"))
    out.append(("two failing pairs: the lowest wins",) + texts([ok, Case("l", rnd(rng, 50), rnd(rng, 1200)), Case("h", rnd(rng, 50), rnd(rng, 50), h1=b"@a", h2=b"@b")] + [ok] * 300 + [Case("b", rnd(rng, 9), b"ACGTU")])
               + (M.ERR_READLEN, 1, "Read length unsupported!"))
    out.append(("header in front of base in front of length within a pair",) + texts([Case("x", rnd(rng, 1000), rnd(rng, 30) + b"?", h1=b"@a", h2=b"@b")]) + (M.ERR_HEADER, 0, "Headers of reads do not match:"))
    out.append(("base in front of length within a pair",) + texts([Case("x", rnd(rng, 1000), rnd(rng, 30) + b"?")]) + (M.ERR_BASE, 0, "Could not convert base '?' to complement!"))
    return out


def _synthetic_block(rng, n, L, first):
    acgt = np.frombuffer(b"ACGT", np.uint8)
    W = 3 * L
    ins = np.clip(rng.normal(1.6 * L, 0.6 * L, n), 20, W).astype(np.int64)[:, None]
    codes = rng.integers(0, 4, (n, W), dtype=np.uint8)                            # the fragment, forward strand
    idx = np.arange(L, dtype=np.int64)[None, :]
    inside = idx < ins
    tails = [np.concatenate([np.frombuffer(a, np.uint8)[None, :].repeat(n, 0), acgt[rng.integers(0, 4, (n, L), dtype=np.uint8)]], axis=1) for a in (A1, A2)]
    behind = np.clip(idx - ins, 0, None)
    r1 = np.where(inside, acgt[np.take_along_axis(codes, np.where(inside, idx, 0), axis=1)], np.take_along_axis(tails[0], behind, axis=1))
    r2 = np.where(inside, acgt[3 - np.take_along_axis(codes, np.where(inside, ins - 1 - idx, 0), axis=1)], np.take_along_axis(tails[1], behind, axis=1))
    for r in (r1, r2):
        err = rng.random((n, L)) < 0.005
        r[err] = acgt[rng.integers(0, 4, int(err.sum()), dtype=np.uint8)]
    drop = rng.integers(L // 2, 2 * L, n)[:, None]
    q1 = np.where(idx >= drop, ord("+"), ord("I")).astype(np.uint8)
    q2 = np.where(idx >= drop - 10, ord("+"), ord("I")).astype(np.uint8)
    head = np.frombuffer(np.char.zfill(np.arange(first, first + n).astype("S9"), 9).tobytes(), np.uint8).reshape(n, 9)

    def text(r, qq):
        out = np.empty((n, 15 + 2 * L), np.uint8)
        out[:, 0] = ord("@"); out[:, 1:10] = head; out[:, 10] = 10
        out[:, 11:11 + L] = r; out[:, 11 + L] = 10; out[:, 12 + L] = ord("+"); out[:, 13 + L] = 10
        out[:, 14 + L:14 + 2 * L] = qq; out[:, 14 + 2 * L] = 10
        return out.tobytes()
    return text(r1, q1), text(r2, q2)


def synthetic(n_pairs, seed, length=151):
    """-> (text1, text2): n_pairs pairs of `length` bases. Fragment sizes come from a normal distribution (mean 1.6 lengths, sd 0.6 lengths, at least 20 bases),
    so that about a sixth of the pairs are shorter than a read and carry the default adapters; 0.5 % substitutions; qualities 40 with a tail of 10."""
    rng = np.random.default_rng(seed)
    t1, t2 = [], []
    for first in range(0, n_pairs, 100000):
        a, b = _synthetic_block(rng, min(100000, n_pairs - first), length, first)
        t1.append(a); t2.append(b)
    return b"".join(t1), b"".join(t2)
