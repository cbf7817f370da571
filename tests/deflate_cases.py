"""Named pieces for the BGZF encoder (csrc/deflate.hip), each built for one path of the encoder: deterministic generators, no committed data.

CASES: Case(name, path, gen, expect). gen() gives the bytes; path names the entry of PATHS (a predicate over the per-piece stats of tests/deflate_model.py at one
level) that the piece exists for; expect(stats_by_level), where given, is the finer claim of the case (which candidate a search ends at, which match a lazy step
keeps). REQUIRED_PATHS lists the paths the catalogue must reach; tests/test_cpu_deflate_model.py checks that each is hit and reports how often.

Reachability, as the kernel is written:
- HCLEN never reaches its floor of 4. Every used code length v in 1..15 is sent as code-length symbol v, which lies at position >= 4 of the 16, 17, 18, 0, 8, ...
  order; the distance code is complete over at most 30 symbols, so it holds a length <= 4 (position >= 11). HCLEN is therefore >= 12 for every input;
  the `> 4` bound of the trim is never what stops it. `hclen_floor` reaches 14 (UNREACHED below).
- `deep_codelen` (a code-length tree deeper than 7 before the limit) is reached: see _deep_codelen."""
import numpy as np

import deflate_model as M

PIECE = M.PIECE
SEG = M.SEGLEN


class Case:
    def __init__(self, name, path, gen, expect=None):
        self.name, self.path, self.gen, self.expect = name, path, gen, expect

    def data(self):
        return self.gen()


def rand(seed, n, lo=0, hi=256):
    return bytearray(np.random.default_rng(seed).integers(lo, hi, n, dtype=np.int64).astype(np.uint8).tobytes())


def h3(b, p):
    return ((b[p] << 16 | b[p + 1] << 8 | b[p + 2]) * 2654435761 & 0xffffffff) >> (32 - M.HBITS)


def avoid_hashes(b, hs, keep=(), protect=()):
    """redraws filler bytes of b until no position but those in keep has a 3-byte hash in hs (so that no chain passes through filler); bytes inside the
    protect ranges (start, end) and the trigrams at keep are never changed"""
    rng = np.random.default_rng(len(b))
    keep = set(keep)
    fixed = set()
    for k in keep:
        fixed.update((k, k + 1, k + 2))
    for s0, s1 in protect:
        fixed.update(range(s0, s1))
    bad = True
    while bad:
        bad = False
        for p in range(len(b) - 2):
            if p not in keep and h3(b, p) in hs:
                for j in (p, p + 1, p + 2):
                    if j not in fixed:
                        b[j] = int(rng.integers(0, 256))
                        bad = True
                        break
    return b


def clean(b, hs, keep):
    """no position but those in keep has a 3-byte hash in hs"""
    keep = set(keep)
    return all(p in keep or h3(b, p) not in hs for p in range(len(b) - 2))


def first_clean(make):
    """make(seed) -> (bytes, hs, keep) for seeds 0, 1, ... until the bytes are clean"""
    for seed in range(100):
        b, hs, keep = make(seed)
        if clean(b, hs, keep):
            return bytes(b)
    raise ValueError("no clean seed")


def copy(b, dst, dist, ln, breaker=True):
    """b[dst:dst + ln] = the ln bytes dist back (overlap allowed); the byte after differs from the one after the source"""
    for i in range(ln):
        b[dst + i] = b[dst + i - dist]
    if breaker and dst + ln < len(b):
        b[dst + ln] = (b[dst + ln - dist] + 1 + (b[dst + ln] % 200)) & 255
        if b[dst + ln] == b[dst + ln - dist]:
            b[dst + ln] ^= 1
    return b


def no_repeat_bytes(counts, seed=0):
    """bytes with counts[v] copies of every byte value v and no 3-byte sequence twice (a parse finds no match in them)"""
    rng = np.random.default_rng(seed)
    left = dict((v, c) for v, c in counts.items() if c)
    total = sum(left.values())
    for _ in range(200):
        rem, out, seen = dict(left), [], set()
        ok = True
        while len(out) < total:
            vals = [v for v, c in rem.items() if c]
            w = np.array([rem[v] for v in vals], float)
            order = rng.choice(len(vals), len(vals), replace=False, p=w / w.sum())
            for k in order:
                v = vals[k]
                if len(out) >= 2 and (out[-2], out[-1], v) in seen:
                    continue
                if len(out) >= 2:
                    seen.add((out[-2], out[-1], v))
                out.append(v); rem[v] -= 1
                break
            else:
                ok = False
                break
        if ok:
            return bytearray(out)
    raise ValueError("no arrangement without repeated trigrams")


def unique_trigrams(n, seed):
    """n random bytes in which no 3-byte string occurs twice (a parse finds no match in them)"""
    rng = np.random.default_rng(seed)
    b = rand(seed, n)
    seen = set()
    for i in range(2, n):
        while (b[i - 2], b[i - 1], b[i]) in seen:
            b[i] = int(rng.integers(0, 256))
        seen.add((b[i - 2], b[i - 1], b[i]))
    return b


# ---- sizes ----
def _sized(n):
    return lambda: bytes(rand(n + 1, n, 65, 69))


# ---- matches ----
def _zeros():
    return bytes(4 * SEG + 300)


def _period(p, n):
    def g():
        u = rand(p, p)
        return bytes((u * (n // p + 1))[:n])
    return g


def _too_far(d):
    def g():
        b = rand(d, d + 600)
        t = bytes([7, 201, 99])
        b[100:103] = t
        b[100 + d:103 + d] = t
        b[103 + d] = b[103] ^ 0x55
        return bytes(avoid_hashes(b, {h3(b, 100)}, keep=(100, 100 + d)))
    return g


def _collisions():
    """the trigram T at 40 and at 3000, seven other trigrams of T's hash in between (each in its own round): the chain of the second T passes through them"""
    t = (11, 22, 33)
    ht = h3(bytes(t), 0)
    coll = []
    for a in range(256):
        for c in range(256):
            x = (a, 5, c)
            if x != t and h3(bytes(x), 0) == ht:
                coll.append(x)
        if len(coll) >= 7:
            break
    b = rand(77, 3200)
    keep = [40, 3000] + [300 * (i + 1) + 40 for i in range(7)]
    b[40:43] = bytes(t); b[3000:3003] = bytes(t)
    copy(b, 3000, 2960, 12)
    for i, x in enumerate(coll[:7]):
        b[keep[2 + i]:keep[2 + i] + 3] = bytes(x)
    return bytes(avoid_hashes(b, {ht}, keep=keep))


def _lookback(gap):
    """a 6-byte string at 10 and at 10 + gap, inside round 0, and nowhere else"""
    def g():
        b = rand(gap, 600)
        copy(b, 10 + gap, gap, 6)
        return bytes(avoid_hashes(b, {h3(b, 10 + k) for k in range(4)}, keep=(10, 10 + gap, 11, 11 + gap, 12, 12 + gap, 13, 13 + gap)))
    return g


LONG = 23


def _chain_depth(k):
    """at P the trigram T with a 23-byte match far back, behind k decoys (T then another byte), one per round: the long match is the (k + 1)-th candidate"""
    P = 300 * (k + 2) + 40

    def make(seed):
        b = rand(1000 * seed + k, P + 200)
        t = bytes([3, 141, 59])
        ht = h3(t, 0)
        b[40:43] = t
        copy(b, P, P - 40, LONG)
        dec = [300 * (i + 1) + 40 for i in range(k)]
        for d in dec:
            b[d:d + 3] = t
            b[d + 3] = b[43] ^ 0x77
        keep = [40, P] + dec
        return avoid_hashes(b, {ht}, keep=keep, protect=[(40, 40 + LONG + 1), (P, P + LONG + 1)]), {ht}, keep
    return lambda: first_clean(make)


def _found_len(level, ln):
    return lambda sl: ln in set().union(*(s.len_values for s in sl[level]))


def _nice(ln):
    """at P: a match of ln bytes 300 back and one of 250 bytes 700 back"""
    P = 3 * SEG

    def make(seed):
        b = rand(1000 * seed + ln, P + SEG)
        copy(b, P, 700, 250)
        copy(b, P - 300, 400, ln, breaker=False)   # (the nearer source agrees with P on ln bytes)
        b[P - 300 + ln] = b[P + ln] ^ 0x3c
        hs = {h3(b, P)}
        return avoid_hashes(b, hs, keep=[P, P - 300, P - 700], protect=[(P - 700, P - 449), (P - 300, P - 299 + ln), (P, P + 251)]), hs, [P, P - 300, P - 700]
    return lambda: first_clean(make)


def _lazy(l0, l1):
    """at P a match of l0 bytes (source A); at P + 1 one of l1 bytes (source B)"""
    P = 3 * SEG + 5

    def make(seed):
        b = rand(1000 * seed + l0 * 100 + l1, P + 300)
        srcA, srcB = P - 1200, P + 1 - 600
        copy(b, P + 1, 600, l1)            # B: P + 1 .. P + l1 from srcB
        b[P] = b[srcA]                     # A: srcA .. srcA + l0 - 1 agrees with P .. P + l0 - 1
        for i in range(1, l0):
            b[srcA + i] = b[P + i]
        b[srcA + l0] = b[P + l0] ^ 0x21
        hs, keep = {h3(b, P), h3(b, P + 1)}, [P, P + 1, srcA, srcA + 1, srcB]
        return avoid_hashes(b, hs, keep=keep, protect=[(srcA, srcA + l0 + 1), (srcB, srcB + l1 + 1), (P, P + max(l0, l1 + 1) + 1)]), hs, keep
    return lambda: first_clean(make)


def _all_len_codes():
    """one match of every length base and every length code's largest length, each at the start of its own segment"""
    lens = sorted(set(M.LEN_BASE) | {M.LEN_BASE[c] + (1 << M.LEN_EXTRA[c]) - 1 for c in range(29)})
    b = rand(258, (len(lens) + 2) * SEG)
    for i, ln in enumerate(lens):
        copy(b, (i + 2) * SEG, SEG + 17 * i, ln)
    return bytes(b)


def _all_dist_codes():
    """one 12-byte match at every distance base and every distance code's largest distance: a fresh random string at dst - d and at dst, all the strings in
    places of their own, dst - d in an earlier round than dst (so that the look-back of 32 does not decide it)"""
    dists = sorted(set(M.DIST_BASE) | {M.DIST_BASE[c] + (1 << M.DIST_EXTRA[c]) - 1 for c in range(30)})
    n = M.WINDOW + 40 * SEG
    b = rand(30, n)
    used = bytearray(n)
    rng = np.random.default_rng(31)
    dst = 40
    for d in dists:
        dst = max(dst, d + 1)
        while True:
            ok = dst % SEG + 13 <= SEG and (d <= 32 or dst // M.NT != (dst - d) // M.NT) and not any(used[dst - d:dst - d + 13]) and not any(used[dst:dst + 13])
            if ok:
                break
            dst += 1
        z = bytes(rng.integers(0, 256, 12, dtype=np.int64).astype(np.uint8))
        for i in range(12):
            b[dst - d + i] = z[i]
        copy(b, dst, d, 12)
        used[dst - d:dst - d + 13] = b"\1" * 13; used[dst:dst + 13] = b"\1" * 13
        dst += 13
    return bytes(b[:dst + 100])


def _fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def _deep_litlen():
    """random filler (every byte value ~ 96 times) with planted copies of length codes 0..11 at Fibonacci counts 1, 1, 2, ..., 144 (largest for length 3)"""
    counts = _fib(12)[::-1]
    plan = [c for c, k in enumerate(counts) for _ in range(k)]
    np.random.default_rng(5).shuffle(plan)
    b = rand(12, PIECE)
    per = 3
    for i, c in enumerate(plan):
        s0 = (i // per) * SEG + (i % per) * 160 + 20
        ln = M.LEN_BASE[c]
        copy(b, s0, 3000 + 7 * i if ln > 3 else 1000 + i, ln)
    return bytes(b)


def _deep_dist():
    """distance codes 0..16 at Fibonacci counts (1597 for code 0 down to 1 for code 16), each a 3-byte match, in filler without repeated 3-byte strings"""
    counts = _fib(17)[::-1]
    plan = [c for c, k in enumerate(counts) for _ in range(k)]
    np.random.default_rng(6).shuffle(plan)
    b = unique_trigrams(8 * len(plan) + 2000, 6)
    p = 600
    for c in plan:
        if (p % SEG) + 12 > SEG:
            p += SEG - p % SEG + 1
        copy(b, p, M.DIST_BASE[c], 3)
        p += 8
    return bytes(b[:p + 20])


# code-length symbol counts of _deep_codelen, found by a search over literal count profiles with deflate_model.header_tables (no matches, so the literal counts
# are the byte counts): search_deep_codelen() repeats it
DEEP_CODELEN_SEED = 3


def _literal_profile(seed):
    rng = np.random.default_rng(seed)
    used = rng.choice(256, int(rng.integers(60, 200)), replace=False)
    return {int(v): max(1, int(np.exp(rng.normal(0, 1.6)) * 3)) for v in used}


def search_deep_codelen(tries=3000):
    for s in range(tries):
        f = [0] * 320
        for v, c in _literal_profile(s).items():
            f[v] = c
        st = M.PieceStats()
        M.header_tables(f, st)
        if st.depth_codelen > 7:
            return s
    return None


def _deep_codelen():
    return bytes(no_repeat_bytes(_literal_profile(DEEP_CODELEN_SEED), seed=DEEP_CODELEN_SEED))


def _zero_runs(runs):
    """every byte once, except that the gaps between present values are zero runs of the given lengths"""
    def g():
        vals, v = [], 0
        for r in runs:
            vals.append(v); v += r + 1
        vals.append(v)
        return bytes(no_repeat_bytes({x: 1 for x in vals if x < 256}, seed=len(runs)))
    return g


def _repeats():
    """groups of 3, 4, 5, 6, 7 and 8 consecutive byte values, one missing value between groups; 32 symbols of count 1 with EOB: every length is 5"""
    vals, v = [], 1
    for k in (3, 4, 5, 6, 7, 6):
        vals += list(range(v, v + k)); v += k + 1
    return bytes(no_repeat_bytes({x: 1 for x in vals}, seed=3))


def _hclen_floor():
    """code lengths only in 4..11: 16 distance codes used 4 times each (all of length 4), 64 matches of 5 bytes, filler without repeated 3-byte strings"""
    b = unique_trigrams(1600, 8)
    for i in range(64):
        copy(b, 200 + 20 * i, M.DIST_BASE[i % 16], 5)
    return bytes(b)


# near-stored pieces: random bytes with a run of zeros of length k; k found by search_near_stored() with the model (margin = ceil(bits / 8) - (n + 5))
NEAR_STORED_N = 2000


def _near(k):
    def g():
        b = rand(1, NEAR_STORED_N)
        b[500:500 + k] = bytes(k)
        return bytes(b)
    return g


def search_near_stored(margin):
    for k in range(0, 400):
        st = M.PieceStats()
        M.member(_near(k)(), None, st)
        if st.margin == margin:
            return k
    return None


NEAR_CODED_K, NEAR_STORED_K = 58, 57   # search_near_stored(-1), search_near_stored(0)


def _all_values():
    return bytes(range(256)) * 3 + bytes(range(255, -1, -1))


PATHS = {
    "sizes": lambda sl: True,
    "multi_member": lambda sl: len(sl) > 1,
    "stored": lambda sl: any(s.stored for s in sl),
    "near_stored_coded": lambda sl: any(s.margin == -1 for s in sl),
    "near_stored_stored": lambda sl: any(s.margin == 0 for s in sl),
    "len258_dist1": lambda sl: any(s.max_len == 258 and 1 in s.dist_values for s in sl),
    "segment_cut": lambda sl: any(s.segment_cut for s in sl),
    "dist_padded_2": lambda sl: any(s.pad_dist == 2 for s in sl),
    "dist_padded_1": lambda sl: any(s.pad_dist == 1 for s in sl),
    "dist_32768": lambda sl: any(M.WINDOW in s.dist_values for s in sl),
    "window_cut": lambda sl: any(s.window_cut for s in sl),
    "too_far_4096_kept": lambda sl: any(s.match3_4096 for s in sl),
    "too_far_4097_rejected": lambda sl: any(s.match3_4097 for s in sl),
    "hash_collision": lambda sl: any(s.collisions for s in sl),
    "lookback_32": lambda sl: any(s.lookback_32 for s in sl),
    "lookback_33": lambda sl: any(s.lookback_33 for s in sl),
    "chain_depth": lambda sl: True,   # (the cases' expect: the long match is found as the last candidate the level walks)
    "chain_exhausted": lambda sl: any(s.chain_exhausted for s in sl),
    "nice_stop": lambda sl: any(s.nice_stop for s in sl),
    "lazy_taken": lambda sl: any(s.lazy_taken for s in sl),
    "lazy_equal": lambda sl: any(s.lazy_equal for s in sl),
    "lazy_long": lambda sl: any(s.lazy_long for s in sl),
    "all_len_codes": lambda sl: set(M.LEN_BASE) | {M.LEN_BASE[c] + (1 << M.LEN_EXTRA[c]) - 1 for c in range(29)} <= set().union(*(s.len_values for s in sl)),
    "all_dist_codes": lambda sl: set(M.DIST_BASE) | {M.DIST_BASE[c] + (1 << M.DIST_EXTRA[c]) - 1 for c in range(30)} <= set().union(*(s.dist_values for s in sl)),
    "deep_litlen": lambda sl: any(s.depth_litlen > 15 for s in sl),
    "deep_dist": lambda sl: any(s.depth_dist > 15 for s in sl),
    "deep_codelen": lambda sl: any(s.depth_codelen > 7 for s in sl),
    "zero_run_3": lambda sl: any((17, 3) in s.rle_runs for s in sl),
    "zero_run_10": lambda sl: any((17, 10) in s.rle_runs for s in sl),
    "zero_run_11": lambda sl: any((18, 11) in s.rle_runs for s in sl),
    "zero_run_138": lambda sl: any(138 in s.zero_runs for s in sl),
    "zero_run_139": lambda sl: any(139 in s.zero_runs for s in sl),
    "zero_run_140": lambda sl: any(140 in s.zero_runs for s in sl),
    "repeat_3_to_7": lambda sl: any({3, 4, 5, 6, 7} <= s.rep_runs for s in sl),
    "hclen_floor": lambda sl: any(s.hclen <= 12 for s in sl),
    "all_byte_values": lambda sl: True,
}

CASES = [Case(f"size_{n}", "sizes", _sized(n)) for n in (0, 1, 2, 3, 4, 255, 256, 257, 509, 510, 511, PIECE - 1, PIECE)]
CASES += [Case(f"size_{n}", "multi_member", _sized(n)) for n in (PIECE + 1, 2 * PIECE + 3)]
CASES += [
    Case("zeros", "len258_dist1", _zeros),
    Case("zeros_segment_cut", "segment_cut", _zeros),
    Case("random", "stored", lambda: bytes(rand(2, 4000))),
    Case("no_match", "dist_padded_2", lambda: bytes(range(256))),
    Case("one_dist_code", "dist_padded_1", lambda: b"ACGT" * 50 + bytes(range(100, 200))),
    Case("period_32768", "dist_32768", _period(32768, 32768 + 3000)),
    Case("period_32769", "window_cut", _period(32769, 32769 + 3000)),
    Case("too_far_4096", "too_far_4096_kept", _too_far(4096)),
    Case("too_far_4097", "too_far_4097_rejected", _too_far(4097)),
    Case("hash_collisions", "hash_collision", _collisions, expect=lambda sl: 12 in sl[None][0].len_values and 12 not in sl[1][0].len_values),
    Case("lookback_32", "lookback_32", _lookback(32), expect=lambda sl: 6 in sl[None][0].len_values),
    Case("lookback_33", "lookback_33", _lookback(33), expect=lambda sl: not sl[None][0].len_values),
]
for chain_len, level in ((4, 1), (8, 2), (16, 3), (48, None)):
    CASES.append(Case(f"chain_{chain_len}_inside", "chain_depth", _chain_depth(chain_len - 1), expect=_found_len(level, LONG)))
    CASES.append(Case(f"chain_{chain_len}_outside", "chain_exhausted", _chain_depth(chain_len),
                      expect=lambda sl, level=level: LONG not in set().union(*(s.len_values for s in sl[level]))))
for ln, level, nice in ((31, 1, 32), (32, 1, 32), (33, 1, 32), (63, 2, 64), (64, 2, 64), (65, 3, 64), (127, None, 128), (128, None, 128), (129, None, 128)):
    CASES.append(Case(f"nice_{ln}", "nice_stop", _nice(ln), expect=_found_len(level, ln if ln >= nice else 250)))
CASES += [
    Case("lazy_longer", "lazy_taken", _lazy(5, 10), expect=_found_len(None, 10)),
    Case("lazy_equal", "lazy_equal", _lazy(6, 6), expect=_found_len(None, 6)),
    Case("lazy_long", "lazy_long", _lazy(32, 40), expect=lambda sl: 32 in sl[None][0].len_values and 40 not in sl[None][0].len_values),
    Case("all_len_codes", "all_len_codes", _all_len_codes),
    Case("all_dist_codes", "all_dist_codes", _all_dist_codes),
    Case("deep_litlen", "deep_litlen", _deep_litlen),
    Case("deep_dist", "deep_dist", _deep_dist),
    Case("deep_codelen", "deep_codelen", _deep_codelen),
    Case("zero_runs_3_10_11", "zero_run_3", _zero_runs((3, 10, 11, 4))),
    Case("zero_runs_10", "zero_run_10", _zero_runs((3, 10, 11, 4))),
    Case("zero_runs_11", "zero_run_11", _zero_runs((3, 10, 11, 4))),
    Case("zero_run_138", "zero_run_138", _zero_runs((138,))),
    Case("zero_run_139", "zero_run_139", _zero_runs((139,))),
    Case("zero_run_140", "zero_run_140", _zero_runs((140,))),
    Case("repeats_3_to_7", "repeat_3_to_7", _repeats),
    Case("hclen_floor", "hclen_floor", _hclen_floor),
    Case("all_byte_values", "all_byte_values", _all_values),
    Case("near_stored_coded", "near_stored_coded", lambda: _near(NEAR_CODED_K)()),
    Case("near_stored_stored", "near_stored_stored", lambda: _near(NEAR_STORED_K)()),
]

# paths with a case that does not reach them yet (the case stays in the catalogue: the device must still give the model's bytes on it)
UNREACHED = {
    "deep_dist": "distance codes 0..16 planted at Fibonacci counts give a distance tree of depth 10, not > 15: matches found elsewhere in the piece flatten the counts",
    "hclen_floor": "HCLEN 14 is the smallest this catalogue reaches (12 is the bound for any input, see the module's docstring)",
}
REQUIRED_PATHS = tuple(p for p in PATHS if p not in UNREACHED)
