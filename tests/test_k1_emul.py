"""The two K1 kernels (ngs-bits_amd/csrc/k1_kernels.h: the text libngsqc_hip.so compiles for gfx950) under the wave emulator
of tests/emul on the CPU, against zlib: every DEFLATE block type, ragged and empty members, overlapping matches, the token
budget of the library and the worst-case one, member queues longer than the grid, and damaged streams. No GPU needed; the
GPU runs of the same kernels are tests/test_gpu_inflate.py / test_gpu_parity.py."""
import ctypes as C
import os
import random
import zlib

import numpy as np
import pytest

import bamgen_lib
import emul_build

HERE = os.path.dirname(os.path.abspath(__file__))


class BD(C.Structure):
    _fields_ = [("cpos", C.c_uint64), ("upos", C.c_uint64), ("clen", C.c_uint32), ("usize", C.c_uint32)]


class BS(C.Structure):
    _fields_ = [("produced", C.c_uint32), ("error", C.c_uint32)]


@pytest.fixture(scope="module")
def emul():
    L = C.CDLL(emul_build.library("k1_emul.cpp"))
    L.k1_emul_inflate.argtypes = [C.c_char_p, C.POINTER(BD), C.c_int64, C.c_void_p, C.POINTER(BS), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
    return L


def run(L, img, mem, park=16, tok_mode=0, p1=0, p2=0, order=1):
    """mem: [(payload offset, payload bytes, inflated bytes)] -> (inflated stream, [(produced, error)], stats)"""
    n = len(mem); bd = (BD * n)(); up = 0
    for i, (cp, cl, us) in enumerate(mem):
        bd[i] = BD(cp, up, cl, us); up += us
    out = np.zeros(up + 64, np.uint8); st = (BS * n)(); stats = (C.c_uint64 * 16)()
    L.k1_emul_inflate(img + b"\0" * 64, bd, n, out.ctypes.data, st, park, tok_mode, p1, p2, order, stats)
    return out[:up].tobytes(), [(s.produced, s.error) for s in st], list(stats)


def deflate(data, level=6, mem=8, strat=zlib.Z_DEFAULT_STRATEGY, flushes=0):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strat); out = b""
    if flushes:
        step = max(1, len(data) // (flushes + 1))
        for i in range(0, len(data), step):
            out += c.compress(data[i:i + step]); out += c.flush(zlib.Z_FULL_FLUSH if (i // step) % 2 else zlib.Z_SYNC_FLUSH)
    else:
        out += c.compress(data)
    return out + c.flush()


def image(cases, rng):
    """payloads at arbitrary byte alignment, as in a BGZF file"""
    img = b""; mem = []
    for raw, comp in cases:
        img += bytes(rng.randrange(256) for _ in range(rng.randrange(0, 23)))
        mem.append((len(img), len(comp), len(raw))); img += comp
    return img, mem


def texty(rng, n):
    words = [bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(3, 12))) for _ in range(50)]
    out = b""
    while len(out) < n:
        out += rng.choice(words) + bytes([rng.randrange(33, 74)]) * rng.randrange(1, 5)
    return out[:n]


def shapes(rng):
    cs = [(b"", deflate(b"")), (b"", bytes([3, 0])), (b"A", deflate(b"A"))]   # empty members (bytes 03 00 = the BGZF EOF block)
    for n in (1, 2, 5, 300):                                              # tiny stored / fixed / dynamic members
        r = bytes(rng.randrange(256) for _ in range(n)); cs.append((r, deflate(r, 0)))
        r = texty(rng, n); cs.append((r, deflate(r, 6))); cs.append((r, deflate(r, 6, 8, zlib.Z_FIXED)))
    r = bytes(rng.randrange(256) for _ in range(20000)); cs.append((r, deflate(r)))                 # incompressible: stored blocks inside
    r = texty(rng, 30000); cs.append((r, deflate(r))); cs.append((r, deflate(r, 9))); cs.append((r, deflate(r, 1)))
    r = texty(rng, 20000); cs.append((r, deflate(r, 6, 8, zlib.Z_FIXED)))
    r = texty(rng, 20000); cs.append((r, deflate(r, 6, 1)))                                         # memLevel 1: many small dynamic blocks
    r = texty(rng, 20000); cs.append((r, deflate(r, 6, 8, zlib.Z_DEFAULT_STRATEGY, 7)))             # sync / full flushes: empty stored blocks between
    r = b"\0" * 65280; cs.append((r, deflate(r)))                                                    # one long run: overlapping matches (dist 1, len 258)
    r = (b"ab" * 40000)[:65535]; cs.append((r, deflate(r)))                                          # dist 2, the largest member size
    r = (b"abcde" * 3000) + texty(rng, 2000) + (b"xyz" * 900); cs.append((r, deflate(r, 9)))
    r = bytes(rng.choice(b"AB") for _ in range(20000)); cs.append((r, deflate(r, 6, 8, zlib.Z_HUFFMAN_ONLY)))   # more tokens than clen + 64 words
    r = bytes(rng.randrange(64, 80) for _ in range(8000)); cs.append((r, deflate(r, 6, 8, zlib.Z_RLE)))
    for _ in range(70):                                                                              # > 64 members: more than one wave, a second member per lane
        r = texty(rng, rng.randrange(1, 3000)); cs.append((r, deflate(r, rng.choice([1, 6, 9]))))
    return cs


def check(cases, got, st, allow_overflow):
    pos = 0
    for i, (raw, _) in enumerate(cases):
        if st[i][1] == 100 and allow_overflow:   # K1_ERR_TOKEN_OVERFLOW: the library inflates such a member again with the worst-case budget
            pos += len(raw); continue
        assert st[i] == (len(raw), 0), f"member {i}: {st[i]}"
        assert got[pos:pos + len(raw)] == raw, f"member {i} differs"
        pos += len(raw)


@pytest.mark.parametrize("variant", ["library_pool", "worst_case_pool", "small_pool", "no_parking", "park_all", "one_decoder_wave_three_resolver_waves", "file_order"])
def test_deflate_shapes(emul, variant):
    rng = random.Random(11)
    cases = shapes(rng); img, mem = image(cases, rng)
    kw = {"library_pool": {}, "worst_case_pool": dict(tok_mode=1), "small_pool": dict(tok_mode=150), "no_parking": dict(park=0), "park_all": dict(park=64),
          "one_decoder_wave_three_resolver_waves": dict(p1=1, p2=3), "file_order": dict(order=0)}[variant]
    got, st, stats = run(emul, img, mem, **kw)
    check(cases, got, st, allow_overflow=variant == "small_pool")
    overflow = [i for i, s in enumerate(st) if s[1] == 100]
    if variant == "small_pool":
        # a pool that runs out: the members that could not get a page report K1_ERR_TOKEN_OVERFLOW (the library repeats them with a
        # worst-case pool), every other member is complete and correct
        assert overflow and len(overflow) < len(cases) and stats[4] >= 150
    else:
        assert not overflow
    assert stats[2] <= 0.5 * stats[1]   # no-op words: lanes that waited inside a group, table groups


def test_synthetic_bam_members(emul):
    """members of the bench generator's BAM (one dynamic block each, ~14 k symbols): a decoding trip leaves ONE word (two literals | a literal and a
    match | a match), no-op words only where a lane waited (input, header) inside a group"""
    img = np.asarray(bamgen_lib.generate(n_reads=3000, seed=5)).tobytes()
    mem = _bgzf_members(img)
    ref = b"".join(zlib.decompress(img[cp:cp + cl], -15) for cp, cl, _ in mem)
    got, st, stats = run(emul, img, mem)
    assert all(s[1] == 0 for s in st) and got == ref
    assert stats[2] <= 0.05 * stats[1]
    assert 0.95 * stats[6] <= stats[1] - stats[2] <= stats[6]   # one word per decoding lane trip (a trip that only ends a block leaves none)


def test_member_whose_tokens_end_with_their_page(emul):
    """a member whose token groups fill the last page exactly has no page behind it: phase 2 must not follow that page's link word (whatever the pool
    held before - here 0xdeadbeef - is not a page). Literal-only members around 510 groups (two pages, two literals per word; the first page of a member is linked when
    the second one is taken, the last one never): some of them end exactly with the second page."""
    rng = random.Random(23); cases = []
    for n in range(3700, 4500):
        raw = bytes(rng.randrange(64, 96) for _ in range(n))
        cases.append((raw, deflate(raw, 6, 8, zlib.Z_HUFFMAN_ONLY)))
    img, mem = image(cases, rng)
    got, st, stats = run(emul, img, mem)
    check(cases, got, st, allow_overflow=False)
    assert stats[13] >= 1 and stats[4] >= 2 * len(cases)


def _random_payload(rng):
    kind = rng.randrange(8); n = rng.choice([rng.randrange(1, 300), rng.randrange(300, 5000), rng.randrange(5000, 65536), 65536, rng.randrange(60000, 65537)])
    if kind == 0: return bytes(rng.randrange(256) for _ in range(n))                      # incompressible: stored blocks
    if kind == 1: return texty(rng, n)
    if kind == 2: return bytes(rng.choice(b"ACGT") for _ in range(n))
    if kind == 3:                                                                          # runs of 1..400 equal bytes (distance-1 matches of every length)
        out = bytearray()
        while len(out) < n: out += bytes([rng.randrange(256)]) * rng.randrange(1, 400)
        return bytes(out[:n])
    if kind == 4:                                                                          # short periods
        base = bytes(rng.randrange(256) for _ in range(rng.randrange(1, 40))); return (base * (n // len(base) + 1))[:n]
    if kind == 5:                                                                          # copies at every distance up to 32 KiB
        out = bytearray(bytes(rng.randrange(64, 96) for _ in range(min(n, 2000))))
        while len(out) < n:
            d = rng.randrange(1, min(len(out), 32768) + 1); s = len(out) - d
            for i in range(rng.randrange(3, 259)): out.append(out[s + i])
        return bytes(out[:n])
    if kind == 6: return bytes(rng.randrange(33, 74) for _ in range(n))                    # quality-string alphabet
    return bytes([rng.randrange(4) * 40 + 33 for _ in range(n)])


@pytest.mark.parametrize("seed", [1])
def test_random_members_against_zlib(emul, seed):
    """random payloads x zlib level / memLevel / strategy / flush pattern x launch shapes (parking, pool size, grid sizes, queue order), inside the domain of BGZF
    (a member's payload is at most 65536 - 26 bytes: raw-run tokens address it with 16 bits). ~10 k such members ran clean while this was written; the test keeps a few hundred."""
    rng = random.Random(seed)
    for _ in range(2):
        cases = []
        for _ in range(rng.randrange(20, 70)):
            raw = _random_payload(rng)
            comp = deflate(raw, rng.choice([0, 1, 1, 3, 6, 6, 6, 9]), rng.choice([1, 4, 8, 9]),
                           rng.choice([zlib.Z_DEFAULT_STRATEGY] * 4 + [zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FILTERED]), rng.choice([0, 0, 0, 1, 3, 17]))
            if len(comp) <= 65510:
                cases.append((raw, comp))
        img, mem = image(cases, rng)
        worst = rng.random() < 0.4
        got, st, _ = run(emul, img, mem, park=rng.choice([0, 8, 16, 32, 64]), tok_mode=1 if worst else 0, p1=rng.choice([0, 0, 1, 2]), p2=rng.choice([0, 0, 1, 3]), order=rng.choice([0, 1]))
        check(cases, got, st, allow_overflow=not worst)


def test_members_made_of_hundreds_of_blocks(emul):
    """zlib flush markers every few bytes: a member of hundreds of DEFLATE blocks, each with its own literal table in the token pool. With enough of them that is
    more than two slots per output byte: a 3000-byte member with 1400 flushes reports K1_ERR_TOKEN_OVERFLOW with the second-chance pool (run once while this was
    written; a minute under the emulator) and decodes with the bound that holds for every valid member (k1_pool_pages_absolute, the library's third chance). Kept
    here: smaller members with the third-chance pool, and the arithmetic of that bound."""
    rng = random.Random(31); cases = []
    for n, flushes in ((1200, 400), (300, 150)):
        raw = texty(rng, n)
        comp = deflate(raw, 6, 8, zlib.Z_DEFAULT_STRATEGY, flushes)
        assert len(comp) <= 65510
        cases.append((raw, comp))
    img, mem = image(cases, rng)
    got, st, stats = run(emul, img, mem, tok_mode=-1)
    check(cases, got, st, allow_overflow=False)
    # the bound: 76 words per block at 0.8 blocks per payload byte stay below 64 words per payload byte
    assert 76 * 0.8 <= 64


def _bgzf_members(img):
    import struct
    pos = 0; mem = []
    while pos < len(img):
        bs = struct.unpack_from("<H", img, pos + 16)[0] + 1
        mem.append((pos + 18, bs - 26, struct.unpack_from("<I", img, pos + bs - 4)[0])); pos += bs
    return mem


@pytest.mark.parametrize("name", ["sry.bam", "BamReader_sr.bam", "MappingQC_in1.bam"])
def test_reference_fixture_bams(emul, name):
    """the BGZF members of the reference's own fixture BAMs (htslib / samtools streams: several deflate blocks per member, an EOF block)"""
    img = open(os.path.join(HERE, "golden", "ref_in", name), "rb").read()
    mem = _bgzf_members(img)
    ref = b"".join(zlib.decompress(img[cp:cp + cl], -15) for cp, cl, _ in mem)
    got, st, _ = run(emul, img, mem, tok_mode=1)
    assert all(s[1] == 0 for s in st) and got == ref and ref[:4] == b"BAM\x01"


def test_damaged_streams(emul):
    """bit flips, truncation, header damage, garbage: the kernels terminate, never report success with a wrong size, and agree with
    zlib on every stream zlib accepts (payload damage that leaves a valid stream is the CRC32 kernel's business)"""
    rng = random.Random(7)
    base = []
    for _ in range(5):
        r = texty(rng, rng.randrange(1000, 9000))
        base.append((r, deflate(r, rng.choice([1, 6, 9]), rng.choice([1, 8]), rng.choice([zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED]))))
    r = bytes(rng.randrange(256) for _ in range(2000)); base.append((r, deflate(r, 0)))
    cases = []
    for k in range(128):
        raw, comp = base[k % len(base)]; c = bytearray(comp); mode = k % 4
        if mode == 0:
            for _ in range(rng.randrange(1, 4)):
                c[rng.randrange(len(c))] ^= 1 << rng.randrange(8)
        elif mode == 1:
            c = c[:rng.randrange(1, len(c))]
        elif mode == 2:
            c[rng.randrange(min(40, len(c)))] ^= 1 << rng.randrange(8)
        else:
            c = bytearray(rng.randrange(256) for _ in range(rng.randrange(1, 400)))
        cases.append((raw, bytes(c)))
    img, mem = image(cases, rng)
    got, st, _ = run(emul, img, mem)
    pos = 0; rejected = 0
    for i, (raw, comp) in enumerate(cases):
        try:
            d = zlib.decompressobj(-15); z = d.decompress(comp); zok = d.eof and len(z) == len(raw)
        except zlib.error:
            zok, z = False, None
        if st[i][1] == 0:
            assert st[i][0] == len(raw)
            assert zok and got[pos:pos + len(raw)] == z, f"member {i}: accepted, but zlib {'differs' if zok else 'rejects it'}"
        else:
            rejected += 1
            assert not zok, f"member {i}: zlib accepts what the kernels reject ({st[i]})"
        pos += len(raw)
    assert rejected > 60
