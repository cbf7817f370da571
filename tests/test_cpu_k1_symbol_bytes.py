"""The symbol bytes of the K1 decoder (csrc/k1_kernels.h, len_byte / dist_byte): the header pass writes per length / distance symbol one byte that holds the
symbol's extra-bits count and a small multiplier, and a trip of the symbol loop makes length and distance from it with shifts. The catalogue of
tests/inflate_cases.py has every symbol at its smallest and largest extra value; here is every value in between and every place in a trip:
    (a) every match length 3..258, 258 both as symbol 284 + 31 and as symbol 285 - one member per length symbol, all its extra values;
    (b) every distance symbol 0..29 with its extra bits all zero, one, all ones and the two alternating patterns - one member per distance symbol (a stored
        block in front gives the far distances their output);
each in a dynamic block (complete codes over all 286 + 30 symbols, so both symbol tables of a lane are full) and in a fixed block, and with the match in the
three places it can take in a trip (a trip decodes up to two literal/length symbols and ends behind a match; the Huffman block starts a trip): first
symbol, behind one literal, behind two literals = first symbol of the next trip.
zlib's inflate of the same stream is the expectation, byte for byte, with status (usize, 0). The kernels' text runs under the wave emulator (tests/emul) with the
parking variants of test_k1_emul.py; the same members on the device: tests/test_gpu_k1_symbol_bytes.py."""
import random
import zlib

import pytest

import deflate_build as B
from inflate_cases import DL30, Member
from test_cpu_inflate_designed import check_named, layout, valid_members
from test_k1_emul import emul, run   # noqa: F401  (emul: the fixture that builds libk1.so)

LL286 = [8] * 226 + [9] * 60          # a complete code over all 286 literal/length symbols (inflate_cases._every_symbol)
PLACES = (0, 1, 2)                    # literals in front of every match of a member
PARKING = {"no_parking": dict(park=0), "default": {}, "park_all": dict(park=64)}


def extra_patterns(eb):
    """all zero, one, all ones, 0101.., 1010.. in eb bits (fewer where they coincide)"""
    mask = (1 << eb) - 1
    return sorted({0, 1 & mask, mask, 0x5555 & mask, 0xaaaa & mask})


def _member(name, kind, front, tokens):
    m = Member().stored(front)
    m = m.dyn(tokens, LL286, DL30, True) if kind == "dynamic" else m.fixed(tokens, True)
    return m.done(name)


def _length_member(i, kind, place, rng):
    """every length of length symbol 257 + i (symbol 284: 227..258, the last one as 284 + 31), at distances 1..16"""
    tokens = []
    for ex in range((1 << B.LEN_EXTRA[i]) if i < 28 else 1):
        tokens += [rng.randrange(256) for _ in range(place)] + [(B.LEN_BASE[i] + ex, 1 + rng.randrange(16), 257 + i)]
    return _member(f"length/{kind}/symbol_{257 + i}/behind_{place}_literals", kind, bytes(rng.randrange(256) for _ in range(16)), tokens)


def _distance_member(d, kind, place, rng):
    """distance symbol d with every pattern of extra_patterns() in its extra bits, at lengths 3..10"""
    eb = B.DIST_EXTRA[d]
    tokens = []
    for ex in extra_patterns(eb):
        tokens += [rng.randrange(256) for _ in range(place)] + [(3 + rng.randrange(8), B.DIST_BASE[d] + ex)]
    return _member(f"distance/{kind}/symbol_{d}/behind_{place}_literals", kind, bytes(rng.randrange(256) for _ in range(B.DIST_BASE[d] + (1 << eb) - 1)), tokens)


_cases = None


def cases():
    """[(name, raw, comp)], deterministic; built once and shared by the tests of both files"""
    global _cases
    if _cases is None:
        rng = random.Random(1951)
        _cases = [_length_member(i, kind, place, rng) for kind in ("dynamic", "fixed") for place in PLACES for i in range(29)]
        _cases += [_distance_member(d, kind, place, rng) for kind in ("dynamic", "fixed") for place in PLACES for d in range(30)]
    return _cases


def test_the_members_cover_what_they_claim():
    """every length 3..258 and both spellings of 258, every distance symbol with its patterns, in every place and both block types; zlib inflates each stream
    to the bytes the LZ77 model gives, and every member fits BGZF"""
    cs = cases()
    assert len(cs) == 2 * 3 * (29 + 30) and len({c[0] for c in cs}) == len(cs)
    lengths = sorted(B.LEN_BASE[i] + ex for i in range(28) for ex in range(1 << B.LEN_EXTRA[i]))
    assert lengths == sorted(list(range(3, 259)))   # 258 once as 284 + 31; symbol 285 is the 29th member of each set
    assert extra_patterns(0) == [0] and extra_patterns(1) == [0, 1] and extra_patterns(13) == [0, 1, 0x0aaa, 0x1555, 0x1fff]
    for name, raw, comp in cs:
        d = zlib.decompressobj(-15)
        assert d.decompress(comp) == raw and d.eof, name
        assert len(comp) <= 65510 and 1 <= len(raw) <= 65536, name


@pytest.mark.parametrize("what", ["length", "distance"])
@pytest.mark.parametrize("variant", sorted(PARKING))
def test_symbol_bytes_under_the_emulator(emul, variant, what):
    cs = [c for c in cases() if c[0].startswith(what)]
    expect = [(name, zlib.decompress(comp, -15), comp) for name, _, comp in cs]
    img, mem = layout(valid_members(expect))
    got, st, _ = run(emul, img, mem, **PARKING[variant])
    check_named(expect, got, st)
