"""A DEFLATE writer that takes orders (RFC 1951): it emits exactly the blocks, code lengths, header coding and tokens it is told to, legal or not.
tests/inflate_cases.py builds its catalogue of hand-made members with it; tests/deflate_model.py (the project's own encoder restated) lends the bit writer,
the canonical code assignment, the default run-length coding and the base tables.

A token is
    an int 0..255                      a literal
    (length, distance)                 a match, coded with the usual symbols
    (length, distance, length symbol)  a match whose length goes out under the given symbol (258 as 284 + 31)
    ("L", symbol)                      the bare code of a literal/length symbol (286, 287, or a length symbol nothing follows)
    ("D", symbol)                      the bare code of a distance symbol (30, 31)
    ("bits", value, count)             raw bits, LSB first
apply(tokens) is the LZ77 model, copied byte by byte: the output a decoder must produce (literals and matches only)."""
import heapq
import zlib

from deflate_model import CL_ORDER, DIST_BASE, DIST_CODE, DIST_EXTRA, LEN_BASE, LEN_CODE, LEN_EXTRA, RLE_EXTRA, BitWriter, build_lengths, canonical, rle

FIXED_LLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DLEN = [5] * 32


def apply(tokens, prefix=b""):
    """the bytes the tokens stand for, behind `prefix` (the output of earlier blocks); returns prefix + output"""
    out = bytearray(prefix)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            ln, d = t[0], t[1]
            assert isinstance(ln, int) and 3 <= ln <= 258 and 1 <= d <= len(out), t
            for _ in range(ln):
                out.append(out[-d])
    return bytes(out)


def huff_lengths(counts):
    """Huffman code lengths of the symbols with non-zero counts (ties: the lower symbol first); no limit - that is the caller's business. A single
    used symbol gets length 1."""
    used = [i for i, c in enumerate(counts) if c]
    lens = [0] * len(counts)
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    heap = [(counts[i], i, (i,)) for i in used]
    heapq.heapify(heap)
    tie = len(counts)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            lens[s] += 1
        heapq.heappush(heap, (a[0] + b[0], tie, a[2] + b[2])); tie += 1
    return lens


def kraft(lens):
    """the Kraft sum of a set of code lengths in units of 2^-15 (a complete code: 32768)"""
    return sum(1 << (15 - l) for l in lens if l)


def token_counts(tokens):
    """(288 literal/length counts with EOB counted once, 30 distance counts) of literal and match tokens"""
    lc, dc = [0] * 288, [0] * 30
    lc[256] = 1
    for t in tokens:
        if isinstance(t, int):
            lc[t] += 1
        else:
            lc[t[2] if len(t) > 2 else 257 + LEN_CODE[t[0]]] += 1; dc[DIST_CODE[t[1]]] += 1
    return lc, dc


def _put_tokens(w, tokens, llen, dlen, eob):
    lcode, dcode = canonical(llen), canonical(dlen)
    for t in tokens:
        if isinstance(t, int):
            assert llen[t], f"literal {t} has no code"
            w.put(lcode[t], llen[t])
        elif t[0] == "L":
            w.put(lcode[t[1]], llen[t[1]])
        elif t[0] == "D":
            w.put(dcode[t[1]], dlen[t[1]])
        elif t[0] == "bits":
            w.put(t[1], t[2])
        else:
            ln, d = t[0], t[1]
            ls = t[2] if len(t) > 2 else 257 + LEN_CODE[ln]
            ex = ln - LEN_BASE[ls - 257]
            assert 0 <= ex < (1 << LEN_EXTRA[ls - 257]) or (ex == 0 and LEN_EXTRA[ls - 257] == 0), t
            ds = DIST_CODE[d]
            assert llen[ls] and dlen[ds], f"{t}: no code for symbol {ls} / distance symbol {ds}"
            w.put(lcode[ls], llen[ls]); w.put(ex, LEN_EXTRA[ls - 257])
            w.put(dcode[ds], dlen[ds]); w.put(d - DIST_BASE[ds], DIST_EXTRA[ds])
    if eob:
        assert llen[256]
        w.put(lcode[256], llen[256])


def stored(w, data, final, nlen=None):
    """a stored block: aligns to the byte boundary, LEN / NLEN (nlen: a wrong complement, for the mismatch case), the bytes. LEN = 0 is allowed."""
    assert len(data) <= 65535
    w.put(1 if final else 0, 1); w.put(0, 2)
    if w.nacc:
        w.put(0, 8 - w.nacc)
    w.put(len(data), 16); w.put((~len(data) & 0xffff) if nlen is None else nlen, 16)
    for b in data:
        w.put(b, 8)


def fixed(w, tokens, final, eob=True):
    w.put(1 if final else 0, 1); w.put(1, 2)
    _put_tokens(w, tokens, FIXED_LLEN, FIXED_DLEN, eob)


def header_runs(seq, forced=()):
    """the run-length coding of a code-length sequence with runs at dictated places: forced = [(start, count, symbol 16 / 17 / 18)]; the stretches
    between them are coded by deflate_model.rle, each on its own (so no other run crosses a dictated one)"""
    out, pos = [], 0
    for start, count, sym in sorted(forced):
        assert start >= pos
        out += rle(seq[pos:start])
        lo = RLE_EXTRA[sym][1]; hi = lo + (1 << RLE_EXTRA[sym][0]) - 1
        assert lo <= count <= hi and start + count <= len(seq)
        v = seq[start]
        assert all(x == v for x in seq[start:start + count])
        assert (sym == 16 and start > 0 and seq[start - 1] == v) or (sym != 16 and v == 0)
        out.append((sym, count - lo)); pos = start + count
    return out + rle(seq[pos:])


def default_cl_lens(runs):
    """code lengths (limit 7) of the code-length alphabet for a run sequence, the counts padded to two symbols as the project's encoder does"""
    f = [0] * 19
    for s, _ in runs:
        f[s] += 1
    i = 0
    while sum(1 for x in f if x) < 2:
        if not f[i]:
            f[i] = 1
        i += 1
    return build_lengths(f, 7)[0]


def dynamic(w, tokens, llen, dlen, final, cl_lens=None, hclen=None, runs=None, eob=True):
    """a dynamic block with the given code lengths (llen: HLIT of them, dlen: HDIST of them; neither needs to come from the tokens, unused symbols may carry
    codes, and nothing is checked for being legal). Header coding: cl_lens = the 19 lengths of the code-length alphabet, hclen = how many of them are sent,
    runs = the run-length sequence [(symbol, extra)] for llen + dlen; each defaults to what a plain encoder would choose."""
    llen, dlen = list(llen), list(dlen)
    if runs is None:
        runs = rle(llen + dlen)
    if cl_lens is None:
        cl_lens = default_cl_lens(runs)
    if hclen is None:
        hclen = 19
        while hclen > 4 and not cl_lens[CL_ORDER[hclen - 1]]:
            hclen -= 1
    w.put(1 if final else 0, 1); w.put(2, 2)
    w.put((len(llen) - 257) & 31, 5); w.put((len(dlen) - 1) & 31, 5); w.put(hclen - 4, 4)
    for i in range(hclen):
        w.put(cl_lens[CL_ORDER[i]], 3)
    cc = canonical(cl_lens)
    for s, ex in runs:
        if cl_lens[s]:                       # (a symbol without a code cannot be written: only streams that are rejected before it have one)
            w.put(cc[s], cl_lens[s])
        if s >= 16:
            w.put(ex, RLE_EXTRA[s][0])
    _put_tokens(w, tokens, llen + [0] * (288 - len(llen)), dlen + [0] * (32 - len(dlen)), eob)


def auto_dynamic(w, tokens, final, limit=15):
    """a dynamic block whose two codes come from the tokens' own counts (Huffman, limited to `limit` bits); the distance code gets two symbols at least"""
    lc, dc = token_counts(tokens)
    for i in range(30):
        if sum(1 for x in dc if x) >= 2:
            break
        if not dc[i]:
            dc[i] = 1
    if sum(1 for x in lc if x) < 2:
        lc[0] = 1
    llen, dlen = build_lengths(lc[:286], limit)[0], build_lengths(dc, limit)[0]
    hl = 286
    while hl > 257 and not llen[hl - 1]:
        hl -= 1
    hd = 30
    while hd > 1 and not dlen[hd - 1]:
        hd -= 1
    dynamic(w, tokens, llen[:hl], dlen[:hd], final)


def judge(comp, isize=None):
    """zlib's verdict on a raw DEFLATE stream: the inflated bytes, or None when zlib raises, does not reach the end of the stream, or (isize given)
    returns another length"""
    try:
        d = zlib.decompressobj(-15); z = d.decompress(comp)
    except zlib.error:
        return None
    if not d.eof or (isize is not None and len(z) != isize):
        return None
    return z


__all__ = ["BitWriter", "apply", "huff_lengths", "kraft", "token_counts", "stored", "fixed", "header_runs", "default_cl_lens", "dynamic", "auto_dynamic", "judge",
           "FIXED_LLEN", "FIXED_DLEN", "LEN_BASE", "LEN_EXTRA", "DIST_BASE", "DIST_EXTRA", "LEN_CODE", "DIST_CODE", "CL_ORDER"]
