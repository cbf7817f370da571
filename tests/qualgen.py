"""Inputs for the tests of the device CRAM quality decoder (tests/test_cram_dev_emul.py on the CPU, tests/test_gpu_cram_quals.py on the GPU): BAM files whose SLICES
each carry one crafted quality distribution, written as CRAM by oracle/cram_encode.py with a chosen rANS order per slice - one file of a few hundred slices is a few
hundred jobs of cram_rans_lds_kernel. Everything is made from fixed seeds at test time; nothing is committed.

A file is a list of Slice(name, records, qs_method, gate): records = [(l_seq, quality bytes | None)] (None: no quality array, 0xff in the BAM), qs_method 4 = rANS
order 0, 41 = rANS order 1; gate names the reason a slice is EXPECTED to stay on the host (None: the device decodes it)."""
import os
import random
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import cram_encode as CE  # noqa: E402
import cram_twin  # noqa: E402

MIN_DEVICE_BYTES = 2048      # rans_plan: n_out >= 2048
MAX_DEVICE_SYMBOLS = 64      # rans_plan: at most 64 symbols (order 1: counting context 0)
MAX_RANS_BYTES = 400000      # the writer gzips larger blocks
PAYLOAD = 65280              # bytes of the BAM stream per stored BGZF member of the image


class Slice:
    def __init__(self, name, records, qs_method, gate=None, mapped=False):
        self.name, self.records, self.qs_method, self.gate, self.mapped = name, records, qs_method, gate, mapped

    def quals(self):
        return b"".join(q for n, q in self.records if n and q is not None)

    def expect_device(self):
        """the gates of cram.hip, from the data alone"""
        d = self.quals(); syms = set(d) | ({0} if self.qs_method == 41 else set())
        return len(d) >= MIN_DEVICE_BYTES and len(syms) <= MAX_DEVICE_SYMBOLS and len(d) <= MAX_RANS_BYTES and self.gate not in ("shared QS block", "lossy record")


def split(rng, q, k):
    """the quality bytes of a slice as k reads"""
    cuts = sorted(rng.sample(range(1, len(q)), k - 1)) if k > 1 else []
    return [(b - a, q[a:b]) for a, b in zip([0] + cuts, cuts + [len(q)])]


def uniform(rng, n, alphabet):
    """n bytes over the alphabet, every symbol at least once; the four quarters start with the first four symbols of the alphabet (different where it has as many)"""
    alphabet = list(alphabet); d = bytearray(rng.choices(alphabet, k=n)); q = n >> 2
    starts = {0, q, 2 * q, 3 * q} if n >= 8 + len(alphabet) else set()
    for s, at in zip(alphabet, [i for i in rng.sample(range(n), len(alphabet) + len(starts)) if i not in starts]): d[at] = s
    for j, at in enumerate(sorted(starts)): d[at] = alphabet[j % len(alphabet)]
    return bytes(d)


def rare_quads(rng, n, order):
    """one symbol of frequency ~4036 / 4096 and 60 symbols that occur four times each - in the four states of ONE round (order 0: four neighbours at a multiple of
    four; order 1: the same place in the four quarters): they normalise to frequency 1, a state that decodes one takes two renormalisation bytes when it is small"""
    d = bytearray([40]) * n; q = n >> 2
    rounds = rng.sample(range(8, q - 8, 2), 60)
    for k, r in enumerate(rounds):
        s = 41 + k if k < 30 else k - 29                 # 41..70 and 1..30
        for j in range(4): d[4 * r + j if order == 0 else j * q + r] = s
    return bytes(d)


def shapes(seed=3, big=True):
    """the distributions the issue names, each in both orders: -> [Slice]"""
    rng = random.Random(seed); out = []
    q41 = list(range(2, 43))

    def both(name, make, k=2, gate0=None, gate1=None):
        for m, gate in ((4, gate0), (41, gate1)):
            d = make(m); out.append(Slice("%s/order%d" % (name, 0 if m == 4 else 1), split(rng, d, k), m, gate))
    for n in (2047, 2048, 2049, 2050, 2051, 3000, 3001, 3002, 3003, 4093, 4094, 4095, 4096):
        g = "2047 bytes" if n < MIN_DEVICE_BYTES else None
        both("size %d" % n, lambda m, n=n: uniform(rng, n, q41), 3, g, g)
    for a in (1, 2, 3, 63, 64, 65):
        both("alphabet %d without quality 0" % a, lambda m, a=a: uniform(rng, 2600, range(1, a + 1)), 2, "65 symbols" if a > 64 else None, "65 symbols" if a + 1 > 64 else None)
    both("alphabet 64 with quality 0", lambda m: uniform(rng, 2600, range(0, 64)))
    both("alphabet 65 with quality 0", lambda m: uniform(rng, 2600, range(0, 65)), 2, "65 symbols", "65 symbols")
    both("quality 0 occurs", lambda m: uniform(rng, 2400, range(0, 41)))
    both("binned 4", lambda m: uniform(rng, 2300, (2, 12, 23, 37)))
    both("binned 8", lambda m: uniform(rng, 2300, (2, 6, 15, 22, 27, 33, 37, 40)))
    both("above 64", lambda m: uniform(rng, 2700, range(34, 94)))
    both("single symbol", lambda m: bytes([30]) * 2222, 1)
    def lonely(m):     # eight symbols that occur once (frequency 1) in a run of one other (frequency 4088): a small state that decodes one takes two bytes
        d = bytearray([35]) * 4501
        for k, at in enumerate(rng.sample(range(10, 4400, 7), 8)): d[at] = 3 + k
        return bytes(d)
    both("frequency 1 next to 4088", lonely, 1)
    both("rare quads", lambda m: rare_quads(rng, 20000 if big else 17000, 0 if m == 4 else 1), 4)
    # order 1 only: a context with exactly one successor (7 is always followed by 8), a symbol that is never a context (the last byte), quarters that start differently
    d = bytearray(uniform(rng, 2401, range(10, 30)))
    for i in range(0, 2390, 37): d[i] = 7; d[i + 1] = 8
    d[-1] = 50; qq = len(d) >> 2
    for j, s in enumerate((11, 7, 8, 29)): d[j * qq] = s
    d[qq + 1] = 8
    out.append(Slice("one successor, never a context/order1", split(rng, bytes(d), 2), 41))
    return out


def _name(i, ln=None):
    s = b"r%07d" % i
    return s if ln is None else (s + b"x" * ln)[:ln]


_NIBBLES = bytes(((1, 2, 4, 8)[(x >> 2) & 3] << 4) | (1, 2, 4, 8)[x & 3] for x in range(256))


def raw_record(name, l_seq, qual, rng, ref_id=-1, pos0=-1, mapq=0):
    r = rng.randbytes((l_seq + 1) // 2)
    packed = bytearray(r.translate(_NIBBLES))                      # two bases per byte, each one of A C G T (codes 1 2 4 8)
    if l_seq & 1: packed[-1] &= 0xf0
    q = b"\xff" * l_seq if qual is None else qual
    if ref_id < 0:
        body = struct.pack("<iiBBHHHiiii", -1, -1, len(name) + 1, 0, 4680, 0, 4, l_seq, -1, -1, 0) + name + b"\0" + bytes(packed) + q
    else:
        end = pos0 + l_seq; b = 0
        for sh, off in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
            if pos0 >> sh == (end - 1) >> sh: b = off + (pos0 >> sh); break
        body = struct.pack("<iiBBHHHiiii", ref_id, pos0, len(name) + 1, mapq, b, 1, 0, l_seq, -1, -1, 0) + name + b"\0" + struct.pack("<I", l_seq << 4) + bytes(packed) + q
    return struct.pack("<i", len(body)) + body


REFS = [("chrA", 500000), ("chrB", 400000)]
TEXT = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS)


def write(slices, directory, tag, **encode_kw):
    """-> dict(bam, cram, slices, n_device): the BAM and the CRAM of it (slice k of the file = slices[k]); reads of a slice marked `mapped` lie on the two contigs"""
    rng = random.Random(17); raws = []; counts = []; i = 0
    for k, s in enumerate(slices):
        for l_seq, q in s.records:
            if s.mapped: raws.append(raw_record(_name(i), l_seq, q, rng, (i // 3) % 2, 1000 + 7 * i, 30))
            else: raws.append(raw_record(s.names[len(raws) - sum(counts)] if hasattr(s, "names") else _name(i), l_seq, q, rng))
            i += 1
        counts.append(len(s.records))
    bam = os.path.join(directory, tag + ".bam"); cram = os.path.join(directory, tag + ".cram")
    cram_twin.write_bam(bam, TEXT, REFS, raws)
    CE.encode(bam, cram, None, slice_records=counts, rr=False, methods=[0, 1], qs_method=[s.qs_method for s in slices], **encode_kw)
    return dict(bam=bam, cram=cram, slices=slices, n_device=sum(s.expect_device() for s in slices))


def header_bytes():
    return 12 + len(TEXT) + sum(9 + len(n) for n, _ in REFS)


def record_shapes(seed=5, big=True):
    """reads against the 65280-byte payloads of the image: -> [Slice] (unmapped reads with chosen name lengths: a slice carries `names`)"""
    rng = random.Random(seed); out = []; at = header_bytes(); q41 = list(range(2, 43)); count = [0]

    def add(sl, l_seq, qual, ln=8):
        nonlocal at
        sl.names.append(_name(count[0], ln)); count[0] += 1; sl.records.append((l_seq, qual))
        start = at + 36 + ln + 1 + (l_seq + 1) // 2; at = start + l_seq
        return start

    def some(L): return uniform(rng, L, q41) if L >= 60 else bytes(rng.choice(q41) for _ in range(L))

    def add_ending_at_boundary(sl, about):
        """a read of about `about` bases whose LAST quality is the last byte of a payload (reads in front of it bring the stream close enough)"""
        lo = 36 + 9 + (about + 1) // 2 + about; hi = 36 + 200 + (about + 400) // 2 + about + 399
        while True:
            T = PAYLOAD - at % PAYLOAD
            if T < lo: T += PAYLOAD
            if T <= hi: break
            L = min(3000, max(1, (T - (lo + hi) // 2) * 2 // 3 - 40)); add(sl, L, some(L))
        for L in range(about, about + 400):
            for ln in range(8, 200):
                if (at + 36 + ln + 1 + (L + 1) // 2 + L) % PAYLOAD == 0: return add(sl, L, uniform(rng, L, q41), ln)
        raise AssertionError("no such read")

    def add_starting_at_boundary(sl, L):
        for ln in range(8, 250):
            if (at + 36 + ln + 1 + (L + 1) // 2) % PAYLOAD == 0: return add(sl, L, uniform(rng, L, q41), ln)
        return None

    def new(name, m): s = Slice(name, [], m); s.names = []; out.append(s); return s
    s = new("first read ends with a payload/order1", 41)
    add_ending_at_boundary(s, 43000)                                   # the FIRST record of the file: its qualities end at byte 65280 of the stream
    for l_seq, q in ((0, None), (1, b"\x05"), (2, b"\x06\x07"), (150, None), (0, None), (151, uniform(rng, 151, q41)), (100, None)): add(s, l_seq, q)
    s = new("tiny reads/order0", 4)
    for k in range(40):
        add(s, k % 3, None if k % 3 == 0 else bytes(rng.choice(q41) for _ in range(k % 3)))
        add(s, 120, None if k % 4 == 1 else uniform(rng, 120, q41))
    # a read of about 100 000 bases over two payload boundaries, in a block of a few hundred KB (order 1: large quarters); order 0: a read longer than a payload
    for m in (41, 4):
        s = new("long read/order%d" % (0 if m == 4 else 1), m)
        L = 100000 if m == 41 else 66000
        gap = lambda: (PAYLOAD - 20000 - (at + 45 + (L + 1) // 2) % PAYLOAD) % PAYLOAD   # the long read's qualities start 20 000 bytes in front of a boundary
        while gap() > 3000: add(s, 1200, uniform(rng, 1200, q41))
        add(s, L, uniform(rng, L, list(range(1, 61)) if m == 4 else q41))
        for _ in range(3): add(s, rng.randrange(100, 4000), None)   # (reads without a quality array between reads with one: no patch for them)
        if m == 41: add(s, 70000, uniform(rng, 70000, (2, 12, 23, 37)))
    s = new("read starts with a payload/order0", 4)
    while add_starting_at_boundary(s, 2500) is None: add(s, 700, uniform(rng, 700, q41))
    s = new("last read ends with the stream/order1", 41)
    add(s, 3000, uniform(rng, 3000, q41)); add(s, 90, None)
    add_ending_at_boundary(s, 2500)                                    # the LAST record of the file: the stream ends with it, the last member is full
    return out


def mapped_slices(seed=9, n_slices=4):
    """reads on two contigs (for multi-reference slices and for the writer's lossy-quality records)"""
    rng = random.Random(seed)
    return [Slice("mapped %d/order%d" % (k, k & 1), [(60, uniform(rng, 60, range(2, 43))) for _ in range(45)], 41 if k & 1 else 4, mapped=True) for k in range(n_slices)]


def many(n_slices, seed=21, distinct=48):
    """thousands of slices (more workgroups than the device has compute units) of `distinct` different contents, so that the writer codes each content once"""
    rng = random.Random(seed); base = []
    for k in range(distinct):
        n = 2048 + rng.randrange(0, 600); alpha = rng.choice([range(2, 43), (2, 12, 23, 37), range(0, 41), range(1, 64), range(30, 90)])
        base.append(split(rng, uniform(rng, n, alpha), 2))
    return [Slice("many %d/order%d" % (k, k & 1), base[(k // 2) % distinct], 41 if k & 1 else 4) for k in range(n_slices)]


class cached_rans:
    """with cached_rans(): the writer codes equal (data, order) once"""
    def __enter__(self):
        self.orig = CE.rans_encode; memo = {}
        def enc(data, order):
            key = (bytes(data), order)
            if key not in memo: memo[key] = self.orig(data, order)
            return memo[key]
        CE.rans_encode = enc
    def __exit__(self, *a):
        CE.rans_encode = self.orig
