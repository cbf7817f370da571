"""The catalogue of hand-built DEFLATE members for the K1 kernels (csrc/k1_kernels.h), shared by tests/test_cpu_inflate_designed.py (wave emulator,
sanitized stand-alone run) and tests/test_gpu_inflate_designed.py. Everything is deterministic. zlib is the judge of the catalogue: it must inflate every
valid case to `raw` and refuse every invalid one.

valid_cases()   -> [(name, raw, comp)]; the name's prefix is the group: shape/ (code shapes and header codings: phase 1), block/ (block structure),
                   geom/ (the resolver's geometry: phase 2), page/ (members whose tokens end near a page's end)
invalid_cases() -> [(name, comp, isize, codes)]: BlockStatus.error must be one of `codes`. Every ISIZE is at least 1: the library leaves members that claim
                   to be empty out of its member table (image.hip, walk_bgzf), so they never reach K1

In an image a member is followed by its BGZF trailer, CRC32 and ISIZE; the CRC field of an invalid member is 0 (INVALID_CRC). The two cases that cut a stream
inside a header / inside a symbol are built on that: zero bits behind the cut complete the header / the symbol, the decoder finishes the block cleanly and has
to notice on its own that it read past the payload (error 15)."""
import random
import zlib

import deflate_build as B

P2_BMAX, P2_IMAX, P2_HIST = 2032, 192, 16   # csrc/k1_kernels.h: output bytes / items per batch of the resolver, bytes of history kept in LDS
INVALID_CRC = 0

GEOM_DISTANCES = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 18, 31, 32, 33, 47, 48, 63, 64, 65, 127, 128, 129, 255, 256, 257, 2015, 2016, 2017, 2031, 2032, 2033,
                  2047, 2048, 2049, 4096, 32767, 32768]
GEOM_LENGTHS = [3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 18, 19, 20, 31, 32, 33, 34, 35, 36, 47, 48, 49, 64, 65, 130, 257, 258]
GEOM_GAPS = [0, 1, 2, 3, 5, 17]
PAGE_SIZES = range(3700, 4501)
N_VALID = {"shape": 43, "block": 9, "geom": 56, "page": 801}
N_INVALID = 30


class Member:
    """one raw DEFLATE stream under construction and the bytes it stands for"""

    def __init__(self):
        self.w, self.raw = B.BitWriter(), b""

    def stored(self, data, final=False):
        B.stored(self.w, data, final); self.raw += bytes(data); return self

    def fixed(self, tokens, final=False):
        B.fixed(self.w, tokens, final); self.raw = B.apply(tokens, self.raw); return self

    def dyn(self, tokens, llen, dlen, final=False, **kw):
        B.dynamic(self.w, tokens, llen, dlen, final, **kw); self.raw = B.apply(tokens, self.raw); return self

    def auto(self, tokens, final=False):
        B.auto_dynamic(self.w, tokens, final); self.raw = B.apply(tokens, self.raw); return self

    def done(self, name, tail=b""):
        return name, self.raw, self.w.bytes() + tail


def lens(d, n):
    """a list of n code lengths from {symbol: length}"""
    out = [0] * n
    for s, l in d.items():
        out[s] = l
    return out


def ladder(symbols):
    """lengths 1, 2, .. n - 1, n - 1 for the n symbols in the given order: a complete code whose longest length is n - 1"""
    n = len(symbols)
    return {s: min(i + 1, n - 1) for i, s in enumerate(symbols)}


def litlen_fields(llen):
    """per code length: (literals, symbols >= 256, literals in front, symbols >= 256 in front) - what the decoder's per-length words are made of"""
    out, pa, pb = {}, 0, 0
    for l in range(1, 16):
        nl = sum(1 for s, x in enumerate(llen) if x == l and s < 256); nn = sum(1 for s, x in enumerate(llen) if x == l and s >= 256)
        out[l] = (nl, nn, pa, pb); pa += nl; pb += nn
    return out


def all_ones_symbol(llen):
    """the symbol that owns the all-ones code: the last one of the longest length"""
    m = max(llen)
    return max(s for s, l in enumerate(llen) if l == m)


def _rand_bytes(rng, n):
    return bytes(rng.randrange(256) for _ in range(n))


DL2 = [1, 1]                                        # the smallest complete distance code
DL30 = [4, 4] + [5] * 28                            # a complete code over all 30 distance symbols


# ------------------------------------------------------------------------------------------------------------------ code shapes (phase 1)
def _all_ones_litlen():
    out = []
    # the two 15-bit codes: the larger symbol is the all-ones code
    lit = lens(ladder([256] + list(range(65, 80))), 257)
    assert all_ones_symbol(lit) == 79
    out.append(Member().dyn(list(range(65, 80)) * 2 + [79, 79, 78, 79], lit, DL2, True).done("shape/all_ones_15_literal"))
    eob = lens(ladder(list(range(65, 80)) + [256]), 257)
    assert all_ones_symbol(eob) == 256 and eob[256] == 15
    out.append(Member().dyn(list(range(65, 80)) * 2 + [79, 79], eob, DL2, True).done("shape/all_ones_15_eob"))
    ln = lens(ladder([256] + list(range(65, 79)) + [260]), 261)
    assert all_ones_symbol(ln) == 260 and ln[260] == 15 and ln[78] == 15
    toks = list(range(65, 79)) + [(6, 1), 78, (6, 2), (6, 14), 78, 78, (6, 1)]
    out.append(Member().dyn(toks, ln, _dl_for(toks), True).done("shape/all_ones_15_length"))
    return out


def _all_ones_distance():
    out = []
    dl = lens(ladder(list(range(16))), 16)             # distance symbols 0..14: 1..15 bits, 15: 15 bits and all ones (distances 193..256, 6 extra bits)
    toks = list(range(32, 96)) * 5 + [(9, 193), (3, 256), 33, (258, 224)] + [(4, B.DIST_BASE[s]) for s in range(15)] + [(5, 256)]
    lc, _ = B.token_counts(toks)
    out.append(Member().dyn(toks, B.build_lengths(lc[:286], 15)[0], dl, True).done("shape/all_ones_15_distance_symbol_15"))
    dl = lens(ladder(list(range(15)) + [29]), 30)      # the all-ones code on distance symbol 29 (13 extra bits)
    rng = random.Random(101)
    toks = [(3, 24577), 7, (4, 32768), (258, 32767), 9] + [(5, B.DIST_BASE[s]) for s in range(15)] + [(3, 30000)]
    lc, _ = B.token_counts(toks)
    out.append(Member().stored(_rand_bytes(rng, 33000)).dyn(toks, B.build_lengths(lc[:286], 15)[0], dl, True).done("shape/all_ones_15_distance_symbol_29"))
    return out


def _every_lmax():
    out = [Member().dyn([97] * 5, lens({97: 1, 256: 1}, 257), DL2, True).done("shape/lmax_01")]
    for lmax in range(2, 16):
        lits = list(range(65, 65 + lmax))
        # even: the all-ones code is EOB; odd: a literal
        ll = lens(ladder(lits + [256]) if lmax % 2 == 0 else ladder([256] + lits), 257)
        assert max(ll) == lmax and B.kraft(ll) == 32768 and all_ones_symbol(ll) == (256 if lmax % 2 == 0 else lits[-1])
        out.append(Member().dyn(lits + lits[::-1] + [lits[-1]] * 3, ll, DL2, True).done(f"shape/lmax_{lmax:02d}"))
    return out


def _every_symbol():
    """all 286 literal/length symbols and all 30 distance symbols in one block, each length / distance symbol at its smallest and largest extra-bits value"""
    ll = [8] * 226 + [9] * 60
    assert B.kraft(ll) == 32768 and B.kraft(DL30) == 32768
    toks = list(range(256))
    for i in range(29):
        s = 257 + i
        toks.append((B.LEN_BASE[i], 1 + i % 7, s))
        if i < 28:
            toks.append((B.LEN_BASE[i] + (1 << B.LEN_EXTRA[i]) - 1, 256 - i, s))   # (symbol 284 at 31 extra: 258)
    while len(B.apply(toks)) < 32768:
        toks.append((258, 255))
    for d in range(30):
        toks += [(3 + d % 5, B.DIST_BASE[d]), d, (4, B.DIST_BASE[d] + (1 << B.DIST_EXTRA[d]) - 1)]
    lc, dc = B.token_counts(toks)
    assert all(lc[:286]) and all(dc) and any(not isinstance(t, int) and t[1] == 32768 for t in toks)
    return [Member().dyn(toks, ll, DL30, True).done("shape/every_symbol")]


def _mixed_lengths():
    """code lengths that hold literals and symbols >= 256 side by side"""
    out = []
    ll = [7, 7] + [8] * 220 + [9] * 64             # length 9: literals 222..255 and all 30 symbols >= 256, behind 256 literals
    f = litlen_fields(ll)
    assert B.kraft(ll) == 32768 and f[9] == (34, 30, 222, 0) and f[9][0] + f[9][2] > 255
    rng = random.Random(202)
    toks = list(range(256)); rng.shuffle(toks)
    for i in range(29):
        toks += [(B.LEN_BASE[i], rng.randrange(1, 200)), rng.randrange(222, 256)]
    out.append(Member().dyn(toks, ll, DL30, True).done("shape/mixed_length_9_behind_256_literals"))
    # EOB among 255 literals of length 8 plus longer lengths shared by literals and length symbols
    ll = [8] * 200 + [9] * 56 + [8] + [9] * 10 + [10] * 19
    ll[199] = 9; ll[198] = 9; ll[197] = 10; ll[196] = 10; ll[195] = 10
    k = B.kraft(ll)
    i = 0
    while k < 32768:                                # shorten literals until the code is complete
        if ll[i] == 9 and k + 64 <= 32768:
            ll[i] = 8; k += 64
        i += 1
    f = litlen_fields(ll)
    assert B.kraft(ll) == 32768 and all(f[l][0] and f[l][1] for l in (8, 9, 10)) and f[10][2] + f[10][0] > 255
    toks = list(range(256)); rng.shuffle(toks)
    for i in range(29):
        toks += [rng.randrange(190, 256), (B.LEN_BASE[i] + (1 << B.LEN_EXTRA[i]) // 2, rng.randrange(1, 250))]
    out.append(Member().dyn(toks, ll, DL30, True).done("shape/mixed_lengths_8_9_10"))
    return out


def _random_skewed(seed):
    """a random skewed set of counts over all 286 + 30 symbols, Huffman lengths limited to 15, and random tokens over every symbol"""
    rng = random.Random(seed)
    ll = B.build_lengths([1 + int(20000 * rng.random() ** 9) for _ in range(286)], 15)[0]
    dl = B.build_lengths([1 + int(20000 * rng.random() ** 9) for _ in range(30)], 15)[0]
    toks = [rng.randrange(256) for _ in range(64)]; n = 64
    while n < 12000:
        if rng.random() < 0.5:
            toks.append(rng.randrange(256)); n += 1
        else:
            i = rng.randrange(29); ln = B.LEN_BASE[i] + rng.randrange(1 << B.LEN_EXTRA[i])
            d = rng.choice([s for s in range(30) if B.DIST_BASE[s] <= n]); dist = min(n, B.DIST_BASE[d] + rng.randrange(1 << B.DIST_EXTRA[d]))
            toks.append((ln, dist, 257 + i)); n += ln
    return Member().dyn(toks, ll, dl, True).done(f"shape/random_skewed_{seed}"), ll


def _incomplete():
    rng = random.Random(303)
    out = []
    toks = [65, 66, (5, 1), 67, (258, 1), (3, 1)]
    lc, _ = B.token_counts(toks)
    out.append(Member().dyn(toks, B.build_lengths(lc[:286], 15)[0], [1], True).done("shape/single_distance_code_symbol_0"))
    toks = [1, 2, (5, 24577), 3, (258, 32768), (3, 30000)]
    lc, _ = B.token_counts(toks)
    out.append(Member().stored(_rand_bytes(rng, 33000)).dyn(toks, B.build_lengths(lc[:286], 15)[0], [0] * 29 + [1], True).done("shape/single_distance_code_symbol_29"))
    out.append(Member().dyn([72, 73, 72, 74], lens({72: 1, 73: 2, 74: 3, 256: 3}, 257), [0], True).done("shape/no_distance_code_literals_only"))
    eob_only = lens({256: 1}, 257)
    out.append(Member().dyn([], eob_only, [0], True).done("shape/eob_only_member"))
    out.append(Member().fixed(list(b"front ")).dyn([], eob_only, [0]).fixed(list(b"back") + [(5, 9)], True).done("shape/eob_only_middle_block"))
    return out


def _length_258():
    toks = [88, (258, 1, 284), (258, 1), 89, (258, 259, 284), (257, 2, 284), (227, 3, 284)]
    lc, _ = B.token_counts(toks)
    out = [Member().dyn(toks, B.build_lengths(lc[:286], 15)[0], _dl_for(toks), True).done("shape/258_as_284_plus_31")]
    toks = [90, 91] + [(B.LEN_BASE[s - 257], 1 + s % 2, s) for s in range(280, 286)] + [(B.LEN_BASE[s - 257] + (1 << B.LEN_EXTRA[s - 257]) - 1, 2, s) for s in range(280, 285)]
    out.append(Member().fixed(toks, True).done("shape/fixed_symbols_280_285"))
    return out


def _dl_for(toks):
    dc = B.token_counts(toks)[1]
    for i in range(30):
        if sum(1 for x in dc if x) >= 2:
            break
        if not dc[i]:
            dc[i] = 1
    dl = B.build_lengths(dc, 15)[0]
    while len(dl) > 1 and not dl[-1]:
        dl.pop()
    return dl


def _longest_trip():
    """a 15-bit literal, a 15-bit length code with 5 extra bits, a 15-bit distance code with 13 extra bits: 63 bits in one trip of the symbol loop; then a
    15-bit literal in front of a length symbol and in front of EOB (the speculative second decode)"""
    rng = random.Random(404)
    ll = lens(ladder([256] + list(range(65, 78)) + [200, 284]), 285)
    dl = lens(ladder(list(range(15)) + [29]), 30)
    assert ll[200] == 15 and ll[284] == 15 and dl[29] == 15 and B.kraft(ll) == 32768 and B.kraft(dl) == 32768
    toks = [200, (258, 32768, 284), 200, (227, 24577, 284), 65, 200, (240, 32767, 284), 200, 200]
    return [Member().stored(_rand_bytes(rng, 33000)).dyn(toks, ll, dl, True).done("shape/longest_trip_63_bits")]


def _header_codings():
    out = []
    # every length 1..7 in the code-length alphabet, every one of its symbols in use
    ll = [7] * 3 + [8] * 246 + [9] * 8 + [0] * 3
    dl = [1, 0, 1] + [0] * 12
    cl = lens({8: 1, 0: 2, 18: 3, 7: 4, 9: 5, 1: 6, 17: 7, 16: 7}, 19)
    runs = B.rle(ll + dl)
    assert B.kraft(ll) == 32768 and B.kraft(cl) << 8 == 32768 << 8 and {s for s, _ in runs} == {0, 1, 7, 8, 9, 16, 17, 18} and sorted(x for x in cl if x) == [1, 2, 3, 4, 5, 6, 7, 7]
    out.append(Member().dyn(list(range(0, 256, 5)), ll, dl, True, cl_lens=cl).done("shape/header_code_lengths_1_to_7"))
    # the smallest HCLEN of a usable set: 16, 17, 18, 0 and 8
    ll = [8] * 255 + [0, 8]
    cl = lens({8: 1, 0: 2, 16: 2}, 19)
    out.append(Member().dyn(list(range(0, 255, 3)), ll, [0], True, cl_lens=cl, hclen=5).done("shape/header_hclen_5"))
    # EOB's length comes from inside a repeat
    ll = lens({10: 1, **{s: 4 for s in range(252, 260)}}, 260)
    runs = B.header_runs(ll + DL2, [(253, 6, 16)])
    assert B.kraft(ll) == 32768 and (16, 3) in runs
    out.append(Member().dyn([10, 252, 253, 254, 255, (3, 1), (4, 2), (5, 1), 10], ll, DL2, True, runs=runs).done("shape/header_16_run_over_eob"))
    # a repeat from the last literal/length symbol into the distance lengths
    ll = lens({97: 1, 255: 2, 256: 3, 257: 3}, 258); dl = [3] * 8
    runs = B.header_runs(ll + dl, [(257, 6, 16)])
    toks = [97] * 14 + [255] + [(3, d) for d in (1, 2, 3, 4, 5, 7, 9, 13)]
    out.append(Member().dyn(toks, ll, dl, True, runs=runs).done("shape/header_16_run_into_distances"))
    # an 18-run of 138 (the longest), and the longest 18-run that a valid header can end with: 59 zeros up to exactly HLIT + HDIST (a run of 138 cannot
    # end there: it would cover EOB)
    ll = lens({138: 2, 139: 2, 140: 2, 256: 2}, 286); dl = [0] * 30
    runs = B.header_runs(ll + dl, [(0, 138, 18), (257, 59, 18)])
    assert runs[0] == (18, 127) and runs[-1] == (18, 48)
    out.append(Member().dyn([138, 139, 140, 140, 139], ll, dl, True, runs=runs).done("shape/header_18_run_138_and_run_to_the_end"))
    # a 16 behind a 17 / an 18 repeats a zero
    ll = lens({6: 1, 7: 2, 40: 3, 256: 3}, 257)
    runs = B.header_runs(ll + DL2, [(0, 3, 17), (3, 3, 16), (8, 11, 18), (19, 6, 16), (25, 15, 18)])
    assert [r[0] for r in runs[:2]] == [17, 16]
    out.append(Member().dyn([6, 7, 40, 6, 6], ll, DL2, True, runs=runs).done("shape/header_16_behind_17_and_18"))
    return out


# ------------------------------------------------------------------------------------------------------------------ block structure
def _block_structure():
    rng = random.Random(505)
    out = []
    m = Member()
    toks = list(b"a Huffman block that ends off a byte boundary, ") + [(20, 30), (3, 1)]
    while True:
        w = B.BitWriter(); B.auto_dynamic(w, toks, False)
        if w.nacc not in (0, 5):                    # (5: the stored header's three bits would end on the boundary)
            break
        toks.append(33 + len(toks) % 7)
    m.auto(toks)
    for n in (0, 1, 255, 256, 257, 3000):
        m.stored(_rand_bytes(rng, n))
    n0 = len(m.raw)
    m.fixed([(50, 3000), (258, 3100), (16, 256), 120, 121, 122, (20, 10), (258, 5), (33, 3769), (3, n0)], True)
    out.append(m.done("block/stored_blocks_between_huffman_blocks"))
    m = Member()
    for _ in range(100):
        m.fixed([])
    out.append(m.fixed(list(b"behind a hundred empty blocks"), True).done("block/hundred_empty_fixed_blocks"))
    out.append(Member().fixed(list(b"then an empty stored block")).stored(b"", True).done("block/final_empty_stored_block"))
    out.append(Member().fixed(list(b"abcdefgh") + [(8, 8), 120, (17, 17), (258, 34), (3, 292)], True).done("block/distance_equals_position"))
    m = Member()
    m.dyn(list(b"abcdefgh" * 3), lens(ladder([256] + list(b"abcdefgh")), 257), DL2)
    toks = list(b"hgfedcbaXY") + [(30, 34), 88, (40, 5), (258, 60), (3, 1)]
    lc, _ = B.token_counts(toks)
    m.dyn(toks, lens(ladder(list(b"hgfedcbaXY") + [256] + sorted({s for s in range(257, 286) if lc[s]})), 286), _dl_for(toks))
    n1 = len(m.raw)
    toks = list(b"Q") + [(100, n1 + 1), (200, 150), 81, (17, 2)]
    m.auto(toks, True)
    out.append(m.done("block/matches_across_dynamic_blocks"))
    out.append(Member().fixed(list(b"bytes behind the final block are not read") + [(9, 4)], True).done("block/unused_bytes_behind_final_block", tail=b"\xff\x00\xaa\x55\xff"))
    out.append(Member().stored(b"", False).stored(b"x").stored(b"", False).fixed([120, (4, 2)]).stored(b"", True).done("block/empty_stored_blocks_everywhere"))
    m = Member().stored(_rand_bytes(rng, 700))
    m.auto([(258, 700), (258, 958), 1, (100, 1)]).stored(_rand_bytes(rng, 256)).auto([(256, 256), (3, 1772 - 200)], True)
    out.append(m.done("block/stored_dynamic_stored_dynamic"))
    out.append(Member().stored(_rand_bytes(rng, 65000), True).done("block/one_stored_block_of_65000"))
    return out


# ------------------------------------------------------------------------------------------------------------------ resolver geometry (phase 2)
def _geom_member(dist, seed, body):
    rng = random.Random(seed)
    toks = [rng.randrange(256) for _ in range(max(dist, 8))]; n = len(toks); end = n + body
    while n < end:
        g = rng.choice(GEOM_GAPS + [rng.randrange(301)] * 2)
        toks += [rng.randrange(256) for _ in range(g)]; n += g
        ln = rng.choice(GEOM_LENGTHS)
        d = dist if rng.random() < 0.85 else rng.choice([x for x in GEOM_DISTANCES if x <= n])
        toks.append((ln, d)); n += ln
    m = Member()
    if dist > 3000:
        head, toks = bytes(toks[:dist]), toks[dist:]   # (the random head as a stored block: the member has to fit BGZF)
        m.stored(head)
    return m.auto(toks, True).done(f"geom/distance_{dist:05d}")


def _geometry():
    out = [_geom_member(d, 600 + i, 20000 if d < 32767 else 16000) for i, d in enumerate(GEOM_DISTANCES)]
    rng = random.Random(707)
    for d in range(1, 16):
        out.append(Member().auto([rng.randrange(256) for _ in range(d)] + [(258, d)] * 253, True).done(f"geom/run_of_258_distance_{d:02d}"))
    m = Member().stored(_rand_bytes(rng, 32768)).auto([(258, 32768)] * 126 + [(4, 32768)], True)
    assert len(m.raw) == 65280
    out.append(m.done("geom/every_item_far_65280"))
    # sources 15, 16 and 17 bytes in front of a batch, and a match across the cut: literal batches are P2_BMAX bytes (no items), so the cuts are known
    toks = [rng.randrange(256) for _ in range(P2_BMAX - 100)] + [(258, 700), (33, P2_HIST + 1), (17, P2_HIST), (33, P2_HIST - 1)]
    toks += [rng.randrange(256) for _ in range(P2_BMAX)] + [(16, P2_HIST), (17, 17), (258, 15), (258, P2_BMAX), (258, P2_BMAX + 1), (258, P2_BMAX - 1)] * 40
    out.append(Member().auto(toks, True).done("geom/batch_cuts"))
    # the last token is a match that ends exactly where the member ends; it stays the last member of its image
    out.append(Member().auto(list(b"the last token is a match ") + [(258, 26), (35, 7), (258, 100)], True).done("geom/last_token_is_a_match"))
    return out


def _page_ends():
    """literal-only members of every size 3700..4500 from zlib's Z_HUFFMAN_ONLY: around 510 token groups, two pages; some end exactly with their page"""
    rng = random.Random(23); out = []
    for n in PAGE_SIZES:
        raw = bytes(rng.randrange(64, 96) for _ in range(n))
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
        out.append((f"page/literals_{n}", raw, c.compress(raw) + c.flush()))
    return out


_valid = None
_skewed_lens = []


def valid_cases():
    global _valid
    if _valid is None:
        cs = _all_ones_litlen() + _all_ones_distance() + _every_lmax() + _every_symbol() + _mixed_lengths()
        for seed in range(6):
            c, ll = _random_skewed(900 + seed); cs.append(c); _skewed_lens.append(ll)
        # (some of the random sets share three or more lengths between literals and symbols >= 256)
        assert any(sum(1 for v in litlen_fields(ll).values() if v[0] and v[1]) >= 3 for ll in _skewed_lens)
        cs += _incomplete() + _length_258() + _longest_trip() + _header_codings() + _block_structure() + _geometry() + _page_ends()
        for name, raw, comp in cs:
            assert len(comp) <= 65510 and len(raw) <= 65536, (name, len(comp), len(raw))
        assert len({c[0] for c in cs}) == len(cs)
        _valid = cs
    return _valid


def group(prefix):
    return [c for c in valid_cases() if c[0].startswith(prefix + "/")]


# ------------------------------------------------------------------------------------------------------------------ invalid members
def _hdr(w, hlit, hdist, hclen, final=1):
    w.put(final, 1); w.put(2, 2); w.put(hlit - 257, 5); w.put(hdist - 1, 5); w.put(hclen - 4, 4)


def _stream(fn):
    w = B.BitWriter(); fn(w)
    return w.bytes()


def invalid_cases():
    out = []
    pad = b"\x55" * 12   # bytes of the payload behind the point where a decoder must have given up

    def add(name, comp, isize, codes):
        out.append((name, comp, isize, tuple(codes)))

    add("block_type_3", _stream(lambda w: w.put(7, 3)) + pad, 10, [4])
    add("stored_len_nlen_mismatch", _stream(lambda w: B.stored(w, b"hello", True, nlen=0xfffb)), 5, [2])
    add("hlit_287", _stream(lambda w: (_hdr(w, 287, 1, 19), w.put(0, 64))) + pad, 10, [5])
    add("hdist_31", _stream(lambda w: (_hdr(w, 257, 31, 19), w.put(0, 64))) + pad, 10, [5])
    eob_only = lens({256: 1}, 257)
    ok_ll = lens({97: 1, 256: 1}, 257)
    add("code_length_code_over_subscribed", _stream(lambda w: B.dynamic(w, [], ok_ll, DL2, True, cl_lens=lens({0: 1, 1: 1, 18: 1}, 19), eob=False)) + pad, 1, [6])
    add("code_length_code_incomplete", _stream(lambda w: B.dynamic(w, [], ok_ll, DL2, True, cl_lens=lens({0: 2, 1: 2, 18: 2}, 19), eob=False)) + pad, 1, [6])
    add("code_length_code_single_code", _stream(lambda w: B.dynamic(w, [], [0] * 257, [0], True, cl_lens=lens({0: 1}, 19), runs=[(0, 0)] * 258, eob=False)) + pad, 1, [5, 6])
    add("repeat_as_first_symbol", _stream(lambda w: B.dynamic(w, [], ok_ll, DL2, True, cl_lens=lens({0: 2, 1: 2, 16: 2, 18: 2}, 19), runs=[(16, 0)] + B.rle(ok_ll + DL2), eob=False)) + pad, 1, [7])
    add("run_past_the_last_length", _stream(lambda w: B.dynamic(w, [], ok_ll, DL2, True, cl_lens=lens({0: 2, 1: 2, 17: 2, 18: 2}, 19), runs=B.rle(ok_ll) + [(1, 0), (17, 0)], eob=False)) + pad, 1, [8])
    add("no_code_for_eob", _stream(lambda w: B.dynamic(w, [97], lens({97: 1, 98: 1}, 257), DL2, True, eob=False)) + pad, 1, [5])
    add("literal_set_over_subscribed", _stream(lambda w: B.dynamic(w, [], lens({97: 1, 98: 1, 256: 1}, 257), DL2, True, eob=False)) + pad, 1, [5])
    add("literal_set_incomplete", _stream(lambda w: B.dynamic(w, [97], lens({97: 2, 256: 2}, 257), DL2, True)) + pad, 1, [5])
    add("distance_set_over_subscribed", _stream(lambda w: B.dynamic(w, [97], ok_ll, [1, 1, 1], True)) + pad, 1, [5])
    add("distance_set_incomplete", _stream(lambda w: B.dynamic(w, [97], ok_ll, [2, 2], True)) + pad, 1, [5])
    add("fixed_symbol_286", _stream(lambda w: B.fixed(w, [97, 98, 99, ("L", 286)], True)) + pad, 10, [10])
    add("fixed_symbol_287", _stream(lambda w: B.fixed(w, [97, ("L", 287)], True)) + pad, 10, [10])
    add("fixed_distance_symbol_30", _stream(lambda w: B.fixed(w, [97, 98, 99, ("L", 257), ("D", 30)], True)) + pad, 10, [12])
    add("fixed_distance_symbol_31", _stream(lambda w: B.fixed(w, [97, 98, ("L", 260), ("D", 31)], True)) + pad, 10, [12])
    ll = lens({97: 1, 256: 2, 257: 2}, 258)
    add("length_symbol_without_a_distance_code", _stream(lambda w: B.dynamic(w, [97, 97, ("L", 257), ("bits", 0, 8)], ll, [0], True)) + pad, 5, [12])
    add("length_symbol_and_the_missing_distance_code", _stream(lambda w: B.dynamic(w, [97, 97, (3, 1), ("L", 257), ("bits", 1, 1), ("bits", 0, 7)], ll, [1], True)) + pad, 8, [12])
    add("missing_code_of_an_eob_only_set", _stream(lambda w: B.dynamic(w, [("bits", 1, 1), ("bits", 0, 15)], eob_only, [0], True, eob=False)) + pad, 1, [10])
    add("distance_in_front_of_the_member", _stream(lambda w: B.fixed(w, [97, 98, 99, (3, 4)], True)), 6, [13])
    long_lit = _stream(lambda w: B.fixed(w, list(b"one byte too many"), True))
    add("output_longer_than_isize_literal", long_lit, 16, [3])
    add("output_longer_than_isize_match", _stream(lambda w: B.fixed(w, list(b"abc") + [(10, 3)], True)), 12, [3])
    add("output_longer_than_isize_stored", _stream(lambda w: B.stored(w, b"0123456789", True)), 9, [3])
    add("output_shorter_than_isize", long_lit, 18, [14])
    # cut inside a header: a literal in a fixed block, then an EOB-only dynamic block; the last four bits of its third 18-run's repeat count are behind the cut (they are zero)
    cl = lens({1: 1, 0: 2, 18: 2}, 19)
    full = _stream(lambda w: (B.fixed(w, [97], False), B.dynamic(w, [], [0] * 256 + [1], [1], True, cl_lens=cl, runs=[(18, 127), (18, 89), (18, 7), (1, 0), (1, 0)])))
    assert len(full) == 15 and B.judge(full) == b"a" and full[14] == 0
    add("cut_inside_a_header", full[:14], 1, [15])
    # cut inside a symbol: the fixed code's EOB is seven zero bits, two of them behind the cut
    full = _stream(lambda w: B.fixed(w, [97], True))
    assert len(full) == 3 and full[2] == 0 and B.judge(full) == b"a"
    add("cut_inside_a_symbol", full[:2], 1, [15])
    add("cut_inside_a_stored_run", _stream(lambda w: B.stored(w, bytes(range(100)), True))[:55], 100, [15])
    add("cut_inside_a_stored_run_second_token", _stream(lambda w: B.stored(w, bytes(600), True))[:5 + 300], 600, [15])
    assert len(out) == N_INVALID and len({c[0] for c in out}) == len(out)
    return out


# the invalid cases that meet the code an incomplete set does not have: what they decode to comes from table entries that only the header pass of that very block
# writes, so they are also run by a fresh process, where nothing an earlier block left in the lane's tables can stand in for it
FRESH_STATE_CASES = ("length_symbol_without_a_distance_code", "length_symbol_and_the_missing_distance_code", "missing_code_of_an_eob_only_set")
