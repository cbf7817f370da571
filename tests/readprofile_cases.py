"""The designed read profiles of test_cpu_readprofile.py (model == oracle, premises), test_gpu_reads_designed.py and test_gpu_prefix_fix.py: record lists
aimed at the internal boundaries of reads_kernel (64 lanes per pass, RQ_CYC = 320 register cycles, odd lengths, the per-wave run-length cache, the growing
length histogram, the rounding of the per-read mean) and of the order-dependent fix-ups (256-record chunks of the one-workgroup form, the switch to the
three-kernel form above 4096 records, its 1024-record blocks and the 256 blocks per trip of its seed kernel). Built with readprofile; CPU only."""
import functools

import numpy as np

import readprofile as RP

R1, R2 = 0x1 | 0x40, 0x1 | 0x80
SMALL_MEMBERS = (3000, 777, 5000)                                          # with NGSQC_TILE_MEMBERS=1: tiles of a few records, records straddle them


def _bases(i, r):
    return np.array([1, 2, 4, 8, 15], dtype=np.uint8)[(i + r) % 5]       # "ACGTN"[(i + r) % 5]


def _rec(flag, ln, r, mapq=None):
    i = np.arange(ln)
    t = (flag, _bases(i, r), ((7 * i + 3 * r) % 94).astype(np.uint8))
    return t if mapq is None else t + (mapq,)


def _const(flag, quals):
    q = np.asarray(quals, dtype=np.uint8)
    return (flag, _bases(np.arange(q.size), 0), q)


# ---- 1. length ladder ----
LADDER = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 319, 320, 321, 383, 384, 385, 641, 5001)


def ladder(lengths=LADDER, per_length=4):
    return [_rec(R1 if k % 2 == 0 else R2, ln, r) for r, (ln, k) in enumerate((ln, k) for ln in lengths for k in range(per_length))]


def ladder_closed_form(lengths=LADDER, per_length=4):
    """What the ladder must give, from the formulas of its bases and qualities alone (a grid over record x cycle; no record is looked at)."""
    ln = np.repeat(np.array(lengths, dtype=np.int64), per_length)
    r = np.arange(ln.size)[:, None]; i = np.arange(max(int(ln.max()), RP.N_CYC))[None, :]
    live = i < ln[:, None]
    fwd = (np.arange(ln.size) % per_length % 2 == 0)[:, None]
    q = (7 * i + 3 * r) % 94
    cyc = np.zeros((RP.N_CYC, 7), dtype=np.int64); bases = np.zeros(5, dtype=np.int64)
    for k in range(5):
        hit = live & ((i + r) % 5 == k)
        bases[k] = hit.sum(); cyc[:, k] = hit[:, :RP.N_CYC].sum(axis=0)
    cyc[:, 5] = (q * (live & fwd))[:, :RP.N_CYC].sum(axis=0); cyc[:, 6] = (q * (live & ~fwd))[:, :RP.N_CYC].sum(axis=0)
    return dict(bases_sequenced=int(ln.sum()), max_cycles=int(ln.max()), bases=bases, cycles=cyc, c_forward=int(fwd.sum()), c_reverse=int((~fwd).sum()),
                base_qualities=np.bincount(q[live], minlength=100).astype(np.int64))


# ---- 2. means on the rounding and clamp edges ----
def _mean_quals(ln, k, extra):
    """ln cycles of quality k, the first `extra` of them k + 1: sum = ln * k + extra"""
    q = np.full(ln, k, dtype=np.uint8); q[:extra] += 1
    return q


def means():
    """(records, notes): notes[ordinal] = (sum, length) where the case names a record's mean."""
    recs, notes = [], {}
    def add(flag, quals):
        q = np.asarray(quals, dtype=np.uint8)
        notes[len(recs)] = (int(q.astype(np.int64).sum()), int(q.size)); recs.append(_const(flag, q))
    for flag in (R1, R2):
        for q in range(99):
            add(flag, [q, q + 1])                                          # mean q + 1/2: read quality q + 1, bin min(q, 59)
        for k in (0, 19, 58, 59, 60, 98):
            add(flag, _mean_quals(64, k, 32))                              # 64 k + 32: k + 1/2 over exactly one wave
            add(flag, _mean_quals(321, k, 160))                            # 321 k + 160: the last mean below k + 1/2
            add(flag, _mean_quals(321, k, 161))                            # ... and the first above
        for k in (0, 20, 59, 60, 61, 99):
            add(flag, np.full(7, k))
            add(flag, np.full(321, k))
        add(flag, [60] * 999 + [59])                                       # sum 59999 over 1000 cycles: rounds to 60, bin 59
        add(flag, [60] * 999 + [61])                                       # just above the clamp
    return recs, notes


# ---- 3. run-length cache and histogram growth ----
def runs_equal():
    return [_rec(R1 if r % 2 == 0 else R2, 100, r) for r in range(300)]


def runs_alternating():
    return [_rec(R1 if r % 2 == 0 else R2, 37 if r % 2 == 0 else 91, r) for r in range(301)]


def runs_increasing():
    return [_rec(R1 if r % 3 else R2, 1 + r, r) for r in range(400)]


GROW_STEPS = ((50, 40), (101, 30), (150, 30), (250, 20), (2000, 9))         # (length, records): 50 -> 101 (> 2 x 50) -> 150 (<= 2 x 101: the histogram doubles to 202)
                                                                            # -> 250 (> 202, <= 404) -> 2000 (> 2 x 404)


def runs_growing():
    """(records, member_sizes): every step of GROW_STEPS fills one BGZF member exactly, so under NGSQC_TILE_MEMBERS=1 every tile brings a longer read."""
    recs = []
    for ln, cnt in GROW_STEPS:
        recs += [_rec(R1 if len(recs) % 2 == 0 else R2, ln, len(recs) + k) for k in range(cnt)]
    raw, off = RP.build_raw(recs)
    first = np.cumsum([0] + [cnt for _, cnt in GROW_STEPS])
    cuts = [0] + [int(off[k]) for k in first[1:-1]] + [len(raw)]
    sizes = tuple(b - a for a, b in zip(cuts, cuts[1:]))
    assert max(sizes) <= 60000
    return recs, sizes


def runs_longest_last():
    return [_rec(R1 if r % 2 == 0 else R2, 80, r) for r in range(200)] + [_rec(R2, 3000, 200)]


# ---- 4. flags ----
FLAG_BITS = (0x1, 0x40, 0x80, 0x100, 0x800, 0x4, 0x10)


def flag_combinations():
    out = []
    for m in range(1 << len(FLAG_BITS)):
        flag = sum(b for k, b in enumerate(FLAG_BITS) if m >> k & 1)
        out.append(_rec(flag, 10 + m % 7 + 64 * (m % 3), m))
    return out


def longest_is(flag_bit):
    recs = [_rec(R1 if r % 2 == 0 else R2, 100 - r % 3, r) for r in range(40)]
    recs.insert(17, _rec(R1 | flag_bit, 500, 99))
    return recs


def only_secondary():
    return [_rec((R1 if r % 2 == 0 else R2) | 0x100, 30 + r, r) for r in range(20)]


# ---- 5. few records ----
FEW = (0, 1, 3, 4, 5, 63, 257)


def few(n):
    return [_rec(R1 if r % 2 == 0 else R2, 30 + (7 * r) % 50, r) for r in range(n)]


# ---- 6. error counters ----
ERR_LEN = 401                                                               # odd: the last cycle is the high nibble of a half-used byte
ERR_AT = (0, 63, 64, 319, 320, ERR_LEN - 1)


def _err_file(values, field, multi_at=(5, 70, 200, 330)):
    """One bad record per (value, placement) between good records, then one record with several bad values in different 64-lane passes."""
    recs, bad = [], 0
    def good():
        recs.append(_rec(R1 if len(recs) % 2 == 0 else R2, ERR_LEN, len(recs)))
    for v in values:
        for at in ERR_AT:
            good()
            f, b, q = _rec(R2 if bad % 2 == 0 else R1, ERR_LEN, len(recs))
            b, q = b.copy(), q.copy(); (b if field == "base" else q)[at] = v
            recs.append((f, b, q)); bad += 1
    good()
    f, b, q = _rec(R1, ERR_LEN, len(recs)); b, q = b.copy(), q.copy()
    for k, at in enumerate(multi_at):
        (b if field == "base" else q)[at] = values[k % len(values)]
    recs.append((f, b, q)); bad += 1
    good()
    return recs, bad


def unknown_bases():
    return _err_file(RP.UNKNOWN, "base")


def bad_qualities():
    return _err_file((100, 255), "qual")


def reads_files():
    """name -> (records, member_sizes or None) of every read-QC file the oracle accepts."""
    out = {"ladder": (ladder(), None)}
    for ln in (63, 64, 320, 321):
        out[f"only_{ln}"] = (ladder((ln,), 6), None)
    out["means"] = (means()[0], None)
    out["runs_equal"] = (runs_equal(), None); out["runs_alternating"] = (runs_alternating(), None); out["runs_increasing"] = (runs_increasing(), None)
    out["runs_growing"] = runs_growing(); out["runs_longest_last"] = (runs_longest_last(), None)
    out["flags"] = (flag_combinations(), None)
    out["longest_secondary"] = (longest_is(0x100), None); out["longest_supplementary"] = (longest_is(0x800), None); out["only_secondary"] = (only_secondary(), None)
    for n in FEW:
        out[f"few_{n}"] = (few(n), None)
    return out


# ---- the fix-up files: short records, "full" = 150 ----
FULL = 150
KIND_DUP, KIND_UNMAPPED, KIND_MAPQ0 = 0, 1, 2


def _finish(flags, lens, mapq):
    """Columns with a base and a quality per cycle (their values do not matter to the mapping counters compared here)."""
    n = int(lens.sum())
    i = np.arange(n)
    return RP.Columns(flags.astype(np.int64), lens.astype(np.int64), np.array([1, 2, 4, 8], dtype=np.uint8)[i % 4], (20 + i % 20).astype(np.uint8), mapq.astype(np.int64))


def staircase(n, f, p, full=FULL, lo=20, hi=60, stair=None, sprinkle=True, on_stair=None):
    """n records; the first of length `full` is ordinal f, the first paired one ordinal p (None: no paired read). In front of f the lengths follow a slowly
    rising staircase lo..hi (`stair`: its own array) with records below the stair in between, so the running maximum changes inside the blocks. Behind f,
    two records in three are full. Duplicates, unmapped, MAPQ-0 and secondary records are sprinkled over the file (never on f or p)."""
    i = np.arange(n)
    st = lo + (i * (hi - lo)) // max(f, 1) if stair is None else stair
    st = np.minimum(st, hi)
    lens = np.maximum(st - (i * 7919) % 5, 1)
    if on_stair is not None:
        lens[on_stair] = st[on_stair]                                    # these records reach the stair: the maximum rises exactly there
    after = i > f
    lens[after & (i % 3 != 0)] = full
    if f < n:
        lens[f] = full
    flags = np.zeros(n, dtype=np.int64); mapq = np.full(n, 60)
    if p is not None:
        pr = (i >= p) & ((i == p) | (i % 5 != 0))
        flags[pr] |= np.where(i[pr] % 2 == 0, R1, R2)
    if sprinkle:
        keep = (i != f) & (i != (-1 if p is None else p))
        flags[keep & (i % 11 == 3)] |= 0x400
        flags[keep & (i % 13 == 5)] |= 0x4
        mapq[keep & (i % 17 == 7)] = 0
        sec = keep & (i % 19 == 9)
        flags[sec] |= 0x100; lens[sec] = np.minimum(lens[sec], hi)         # (a secondary record never is the first full-length one)
    return flags, lens, mapq


def first_full(f, p=2, n=None):
    n = n if n is not None else max(f, p or 0) + 700
    return _finish(*staircase(n, f, p))


FIRST_FULL = (0, 1, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 5119, 5120, 5121, 8191, 8192)
# (f, p): p << f, p >> f, p = f, p = f +- 1, no paired read; both orders of the two limits on both sides of 4096
FULL_PAIRED = ((3000, 3), (5000, 3), (100, 3000), (100, 6000), (5000, 9000), (4500, 6000), (2000, 2000), (4096, 4096), (4097, 4097), (4097, 4096), (4096, 4097),
               (4098, 4097), (1024, 1025), (1025, 1024), (300, None), (5000, None))


def quiet_records(f, at_151, edges):
    """Secondary / supplementary records of length 151 at the ordinals `at_151` in front of f: they must not move the maximum. Around every edge e of `edges`
    the records e - 1, e and e + 1 are a duplicate, an unmapped and a MAPQ-0 record (one of each kind on every edge, the order rotating from edge to edge),
    each LONGER than everything before it: counted for the running maximum, not passing for the length sum. Returns (columns, columns without the 151s)."""
    n = f + 700
    flags, lens, mapq = staircase(n, f, 7, sprinkle=False)
    for k, e in enumerate(edges):
        for side in (0, 1, 2):
            o = e - 1 + side; kind = (k + side) % 3
            assert 0 < o < f and o not in at_151
            lens[o] = int(lens[:o].max()) + 1
            if kind == KIND_DUP: flags[o] |= 0x400
            elif kind == KIND_UNMAPPED: flags[o] |= 0x4
            else: mapq[o] = 0
    assert int(lens[:f].max()) < FULL
    for k, o in enumerate(at_151):
        assert o < f
        flags[o] = (flags[o] & ~0x400) | (0x100 if k % 2 == 0 else 0x800); lens[o] = FULL + 1
    keep = lens != FULL + 1
    return _finish(flags, lens, mapq), _finish(flags[keep], lens[keep], mapq[keep])


QUIET = {"quiet_2500": (2500, (0, 1023, 1024), (256, 512, 768, 2048)),
         "quiet_6000": (6000, (0, 1023, 1024), (256, 512, 768, 2048, 3072, 4096, 5120)),
         "quiet_6000_b": (6000, (0, 2047, 2048), (1024, 3072, 4096, 4352, 5120))}


def stairs(kind):
    """steps_256 / steps_1024: the staircase rises exactly at the multiples of 256 / 1024. mid_block: it rises in the middle of every block of 1024 and again
    a record before its end, so no block's seed equals its maximum."""
    f = {"steps_256": 6000, "steps_1024": 8000, "mid_block": 8000}[kind]
    i = np.arange(f + 700)
    st = {"steps_256": 20 + i // 256, "steps_1024": 20 + 4 * (i // 1024), "mid_block": 20 + 2 * ((i + 512) // 1024) + (i % 1024 == 1022)}[kind]
    on = {"steps_256": i % 256 == 0, "steps_1024": i % 1024 == 0, "mid_block": (i % 1024 == 512) | (i % 1024 == 1022)}[kind]
    return _finish(*staircase(f + 700, f, 5000, stair=st, hi=70, sprinkle=False, on_stair=on))


BIG_F, BIG_N, BIG_P = 262_144 + 1025, 300_000, 200_000


def many_blocks():
    """3e5 records of 1..30 bases, the first 30 at ordinal 262 144 + 1025: 258 blocks of 1024 in front of it - a second trip of the seed kernel, and the
    maximum rises twice more (28, 29) inside the blocks of that second trip."""
    i = np.arange(BIG_N)
    st = np.minimum(1 + (i * 27) // (256 * 1024), 27) + (i >= 256 * 1024 + 300) + (i >= 256 * 1024 + 900)
    return _finish(*staircase(BIG_N, BIG_F, BIG_P, full=30, lo=1, hi=29, stair=st, on_stair=(i == 256 * 1024 + 300) | (i == 256 * 1024 + 900)))


TWO_STEP_F, TWO_STEP_F2, TWO_STEP_N = 5121, 9000 + 4097, 14000
TWO_STEP_SHORT, TWO_STEP_SPLIT = 8000, 8500                                # no record of 150 in [SHORT, F2); the second tile begins near SPLIT


def two_steps():
    """first_full(5121), and behind ordinal 9000 + 4097 a second, higher step: 200. From ordinal 8000 up to that step every record is shorter than 150, so in a
    second tile that begins there the running maximum is the carried 150 for more than four blocks of 1024: a lost carry changes bases_trimmed."""
    flags, lens, mapq = staircase(TWO_STEP_N, TWO_STEP_F, 2)
    i = np.arange(TWO_STEP_N)
    short = (i >= TWO_STEP_SHORT) & (i < TWO_STEP_F2) & (lens == FULL)
    lens[short] = 30 + (i[short] * 7919) % 29
    lens[(i > TWO_STEP_F2) & (lens == FULL)] = 200; lens[TWO_STEP_F2] = 200
    flags[TWO_STEP_F2] &= ~0x100 & ~0x400 & ~0x4
    return _finish(flags, lens, mapq)


def two_tile_layout(cols, member=50000, split=TWO_STEP_SPLIT):
    """(member_sizes, NGSQC_TILE_MEMBERS, records that begin in the first tile): two tiles, the first ends with the member that holds record `split`."""
    raw, off = RP.build_raw(cols)
    n_members = -(-len(raw) // member) + 1                                  # + the empty end-of-file member
    k = -(-int(off[split]) // member)
    assert n_members - k <= k                                               # what is left is one more tile
    return (member,), k, int(np.searchsorted(off, k * member))


@functools.lru_cache(maxsize=None)
def prefix_files():
    """name -> columns of every fix-up file but the large one (built once per process; nobody writes to them)."""
    out = {f"first_full_{f}": first_full(f) for f in FIRST_FULL}
    for f, p in FULL_PAIRED:
        out[f"full_{f}_paired_{p}"] = first_full(f, p, n=max(f, p or 0) + 700)
    for name, a in QUIET.items():
        out[name] = quiet_records(*a)[0]
    for kind in ("steps_256", "steps_1024", "mid_block"):
        out[kind] = stairs(kind)
    return out
