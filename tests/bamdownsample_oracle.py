"""BamDownsample restated in Python (src/BamDownsample/main.cpp:31-101), independent of the device: the sequential loop over the records with glibc's rand().

The generator is glibc's srand() / rand() (random_r.c, TYPE_3): 31 words seeded by the Lehmer step 16807 x mod (2^31 - 1), the additive recurrence
o[i] = o[i-31] + o[i-3] mod 2^32, 310 values thrown away, output o[i] >> 1. Helper::randomNumber(0, 100) is taken as 0 + (double)rand() / RAND_MAX * 100: cppCORE is
not part of the reference tree at hand, so the formula is pinned by the expected log of the reference's own test (tests/golden/ref_out/BamDownsample_out1_Linux.txt),
which this model reproduces byte for byte (tests/test_cpu_bamdownsample.py)."""
import numpy as np

from bamfilter_oracle import Rec, read_bam, written

RAND_MAX = 2147483647
M32 = 0xFFFFFFFF


def seed_words(seed):
    """the 31 words behind srand(seed) and the 310 discarded values: o[313 .. 343]; the next output is (o[313] + o[341]) >> 1"""
    seed &= M32
    if seed == 0:
        seed = 1
    r = [seed]
    for _ in range(30):
        w = r[-1] - (1 << 32) if r[-1] & 0x80000000 else r[-1]   # (the word as int32)
        hi = int(w / 127773)                                       # (C division: towards zero)
        lo = w - hi * 127773
        w = 16807 * lo - 2836 * hi
        if w < 0:
            w += 2147483647
        r.append(w & M32)
    o = r + r[:3]
    for i in range(34, 344):
        o.append((o[i - 31] + o[i - 3]) & M32)
    return o[313:344]


def rand_stream(seed, n, first=0):
    """rand() values first .. first + n - 1 behind srand(seed) (sequential: first steps are walked)"""
    s = seed_words(seed)
    out = []
    for k in range(first + n):
        v = (s[0] + s[28]) & M32
        s = s[1:] + [v]
        if k >= first:
            out.append(v >> 1)
    return out


def rand_stream_np(seed, n):
    """the same stream for large n: the recurrence in strides of 3 (o[i] needs o[i-3])"""
    o = np.zeros(31 + n + 3, dtype=np.uint32)
    o[:31] = seed_words(seed)
    for i in range(31, 31 + n, 3):
        o[i:i + 3] = o[i - 31:i - 28] + o[i - 3:i]
    return o[31:31 + n] >> 1


def jump_words(words, e):
    """the 31 words e steps ahead without walking them: with c = x^e mod (x^31 - x^28 - 1) over Z/2^32, o[n + e] = sum c[j] o[n + j]"""
    def mul(a, b):
        t = [0] * 61
        for i, x in enumerate(a):
            if x:
                for j, y in enumerate(b):
                    t[i + j] += x * y
        for d in range(60, 30, -1):
            t[d - 3] += t[d]; t[d - 31] += t[d]
        return [v & M32 for v in t[:31]]
    r, x = [1] + [0] * 30, [0, 1] + [0] * 29
    while e:
        if e & 1:
            r = mul(r, x)
        x = mul(x, x); e >>= 1
    ext = list(words)
    for i in range(31, 61):
        ext.append((ext[i - 31] + ext[i - 3]) & M32)
    return [sum(r[j] * ext[j + k] for j in range(31)) & M32 for k in range(31)]


def rand_stream_at(seed, first, n):
    """rand() values first .. first + n - 1 for a first too far to walk"""
    s = jump_words(seed_words(seed), first)
    out = []
    for _ in range(n):
        v = (s[0] + s[28]) & M32
        s = s[1:] + [v]
        out.append(v >> 1)
    return out


def random_number(r, lo=0.0, hi=100.0):
    return lo + float(r) / float(RAND_MAX) * (hi - lo)


def keeps(r, percentage):
    return random_number(r) < percentage


def keep_stream(seed, percentage, first, n):
    """uint8[n]: ordinal first + i is kept"""
    r = rand_stream_np(seed, first + n)[first:].astype(np.float64)
    return ((0.0 + r / float(RAND_MAX) * 100.0) < percentage).astype(np.uint8)


def threshold(percentage):
    """the smallest T in [0, 2^31] with: r < T exactly when keeps(r, percentage), for every rand() value r (bisection: random_number is monotonic in r)"""
    lo, hi = 0, 1 << 31   # keeps(r) for every r < lo; not keeps(r) for every r >= hi
    while lo < hi:
        m = (lo + hi) >> 1
        if keeps(m, percentage):
            lo = m + 1
        else:
            hi = m
    return lo


def downsample(records, percentage, seed=1):
    """(kept record bytes in output order, log text of -test, counts dict, kept names [(b"SE" | b"PE", name)])"""
    if percentage <= 0 or percentage >= 100:
        raise ValueError(f"Invalid percentage {percentage:g}!")
    rnd = iter(rand_stream_np(seed, len(records)))   # (at most one decision per record)
    cache, out, names = {}, [], []
    c = dict(se=0, se_written=0, pe=0, pe_written=0, pe_unmatched=0)
    for b in records:
        r = b if isinstance(b, Rec) else Rec(b)   # (records parsed once by the caller serve many runs)
        if r.flag & 0x900:
            continue
        if not r.flag & 1:
            c["se"] += 1
            if keeps(int(next(rnd)), percentage):
                c["se_written"] += 1
                out.append(written(r)); names.append((b"SE", r.name))
        elif r.name not in cache:
            cache[r.name] = r
        else:
            c["pe"] += 1
            o = cache.pop(r.name)
            if keeps(int(next(rnd)), percentage):
                c["pe_written"] += 1
                out += [written(o), written(r)]; names.append((b"PE", r.name))
    c["pe_unmatched"] = len(cache)
    return out, log_text(names, c), c, names


def log_text(names, c):
    t = b"".join(b"KEPT " + k + b": " + nm + b"\n" for k, nm in names)
    t += b"SE reads                    : %d\n" % c["se"]
    t += b"SE reads (written)          : %d\n" % c["se_written"]
    t += b"PE reads                    : %d\n" % c["pe"]
    t += b"PE reads (written)          : %d\n" % c["pe_written"]
    t += b"PE reads unmatched (skipped): %d\n" % c["pe_unmatched"]
    return t


def names_text(names):
    """the kept names as ngsqc_downsample hands them out: "SE\\tname\\n" / "PE\\tname\\n" lines"""
    return b"".join(k + b"\t" + nm + b"\n" for k, nm in names)


def downsample_file(path, percentage, seed=1):
    header, recs = read_bam(path)
    out, log, c, names = downsample(recs, percentage, seed)
    return header, out, log, c, names
