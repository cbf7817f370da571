"""The BGZF encoder of csrc/deflate.hip (bgzf_deflate_kernel) restated in plain Python: the specification of what the kernel computes, byte for byte.

compress(data, level=None) -> the bytes of ngsqc.bgzf_compress(data, level=level); compress_stats(data, level) -> (bytes, [PieceStats per member]).
The kernel's output does not depend on timing or the order of atomics, so it is a pure function of (data, level); every rule below is the kernel's, in its terms:

- Pieces of PIECE (0xff00) bytes, one BGZF member each, no EOF member. Header 1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, 'B' 'C' 2, BSIZE - 1; trailer CRC32, ISIZE.
- Level 0: stored members. Levels 1 / 2 / 3: greedy, 4 / 8 / 16 candidates, nice length 32 / 64 / 64. Levels 4-9 and None: 48 candidates, nice length 128, and
  the lazy step (for matches shorter than LAZY = 32).
- Hash of position p (only where p + 2 < n): ((b[p] << 16 | b[p+1] << 8 | b[p+2]) * 2654435761 mod 2^32) >> 20.
- Chain prev[p] (position + 1, 0: none), positions in rounds of 256; q = the last earlier position with p's hash: q itself if it lies in p's round at most LOOKBACK (32)
  positions back, the last position with that hash before the round if q lies in the round further back, else q (chain(); chain_rounds() is the round loop).
- Match search at p: limit min(segment end - p, 258); at most CHAIN candidates along prev, none more than WINDOW (32768) back; a candidate replaces the best only
  when strictly longer; the search stops at NICE or at the limit; a 3-byte match more than TOO_FAR (4096) back is none (zlib's TOO_FAR).
- Parse: 128 segments of 510 bytes, each greedy (with the lazy step where the level has one: a literal when the next position's match is strictly longer); a match
  never runs past its segment's end but may reach back anywhere in the piece.
- Huffman: freq[EOB] = 1; the distance counts padded to two used symbols from index 0 up. Symbols ranked by (count, symbol); Moffat-Katajainen lengths, then
  miniz's limit (counts per length, the ones past maxbits folded into maxbits, the Kraft sum repaired); the most frequent symbols take the shortest lengths;
  canonical codes. Limits 15 (lit/len), 15 (distance), 7 (code-length code). HLIT trimmed to >= 257, HDIST to >= 1; the lengths run-length coded as rle() does;
  the code-length counts padded to two symbols; HCLEN trimmed to >= 4 in CL_ORDER.
- One dynamic block, BFINAL = 1; the piece is stored instead when ceil(bits / 8) >= n + 5."""
import zlib

import numpy as np

PIECE = 0xff00
NT = 256                       # positions per round of the chain build (threads of a workgroup)
HBITS = 12
LOOKBACK = 32
NSEG, SEGLEN = 128, PIECE // 128
WINDOW = 32768
LAZY = 32
TOO_FAR = 4096
MAX_LEN = 258
DEFAULT = (48, 128, True)
FAST = {1: (4, 32, False), 2: (8, 64, False), 3: (16, 64, False)}

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
HEADER = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, ord("B"), ord("C"), 2, 0])


def _code_table(bases, top):
    t = [0] * (top + 1)
    for c, b in enumerate(bases):
        for v in range(b, top + 1):
            t[v] = c
    return t


LEN_CODE = _code_table(LEN_BASE, MAX_LEN)          # length 3..258 -> 0..28
DIST_CODE = _code_table(DIST_BASE, WINDOW)         # distance 1..32768 -> 0..29


def params(level):
    """(CHAIN, NICE, LAZY_STEP) of a level; None for level 0 (stored only)"""
    if level == 0:
        return None
    return FAST.get(level, DEFAULT)


class PieceStats:
    """the paths one piece took through the encoder"""
    FIELDS = ("stored", "margin", "depth_litlen", "depth_dist", "depth_codelen", "hlit", "hdist", "hclen", "pad_dist", "pad_codelen",
              "lazy_taken", "lazy_equal", "lazy_long", "too_far", "window_cut", "chain_exhausted", "nice_stop", "collisions", "segment_cut",
              "lookback_32", "lookback_33", "max_len", "max_dist", "match3_4096", "match3_4097")

    def __init__(self):
        for f in self.FIELDS:
            setattr(self, f, 0)
        self.rle_count = {16: 0, 17: 0, 18: 0}
        self.rle_max = {16: 0, 17: 0, 18: 0}
        self.len_codes, self.dist_codes = set(), set()
        self.len_values, self.dist_values = set(), set()
        self.rle_runs = set()                      # (16 / 17 / 18, the repeat count it codes)
        self.zero_runs, self.rep_runs = set(), set()   # lengths of the runs of zeros / of a nonzero length in the code-length sequence

    @property
    def limited(self):
        return self.depth_litlen > 15, self.depth_dist > 15, self.depth_codelen > 7

    def as_dict(self):
        d = {f: getattr(self, f) for f in self.FIELDS}
        d.update(rle_count=dict(self.rle_count), rle_max=dict(self.rle_max), len_codes=sorted(self.len_codes), dist_codes=sorted(self.dist_codes))
        return d


def hashes(b):
    """the 12-bit hash of every position p with p + 2 < len(b)"""
    a = np.frombuffer(bytes(b), np.uint8).astype(np.uint32)
    m = len(a) - 2
    if m <= 0:
        return np.zeros(0, np.uint32)
    return ((a[:m] << 16 | a[1:m + 1] << 8 | a[2:]) * np.uint32(2654435761)) >> np.uint32(32 - HBITS)


def chain(b):
    """prev[p] (position + 1 of p's predecessor, 0: none) for every position of piece b, without a loop over positions"""
    n = len(b)
    prev = np.zeros(n, np.int64)
    h = hashes(b).astype(np.int64)
    m = len(h)
    if m == 0:
        return prev
    order = np.lexsort((np.arange(m), h))          # by hash, then position
    hs, ps = h[order], order.astype(np.int64)
    idx = np.arange(m)
    same = np.zeros(m, bool)
    same[1:] = hs[1:] == hs[:-1]
    q = np.where(same, np.r_[-1, ps[:-1]], -1)     # the last earlier position with the same hash
    rnd = ps // NT
    new_group = ~same | (rnd != np.r_[-1, rnd[:-1]])
    gstart = np.maximum.accumulate(np.where(new_group, idx, 0))   # first entry of the (hash, round) group in sorted order
    gb = gstart - 1
    ok = gb >= 0
    gbc = np.maximum(gb, 0)
    head = np.where(ok & (hs[gbc] == hs), ps[gbc] + 1, 0)   # the last position with the hash before the round, + 1
    in_round = (q >= 0) & (q // NT == rnd)
    c = np.where(q < 0, 0, np.where(in_round, np.where(ps - q <= LOOKBACK, q + 1, head), q + 1))
    prev[ps] = c
    return prev


def chain_rounds(b):
    """chain(b) by the kernel's loop: rounds of NT positions, the look-back among the round's hashes, then the head table by maximum"""
    n = len(b)
    h = [int(x) for x in hashes(b)]
    prev, head = [0] * n, [0] * (1 << HBITS)
    for r0 in range(0, n, NT):
        rh = [h[p] if p < len(h) else None for p in range(r0, r0 + NT)]
        for t in range(NT):
            p = r0 + t
            if p >= n:
                break
            c = 0
            if rh[t] is not None:
                for j in range(t - 1, max(0, t - LOOKBACK) - 1, -1):
                    if rh[j] == rh[t]:
                        c = r0 + j + 1
                        break
                if not c:
                    c = head[rh[t]]
            prev[p] = c
        for t in range(NT):
            if rh[t] is not None:
                head[rh[t]] = max(head[rh[t]], r0 + t + 1)
    return prev


def _lookback_stats(b, st):
    h = hashes(b)
    m = len(h)
    for d, f in ((32, "lookback_32"), (33, "lookback_33")):
        if m > d:
            p = np.arange(d, m)
            # the nearest earlier same-hash position is exactly d back, inside p's round
            hit = (h[d:] == h[:-d]) & (p // NT == (p - d) // NT)
            for k in range(1, d):
                hit &= h[d:] != h[d - k:m - k]
            setattr(st, f, int(hit.sum()))


def _parse(b, prev, chain_len, nice, lazy, st):
    """the tokens of piece b: ints < 256 are literals, others -(len << 16 | dist)"""
    n = len(b)
    toks = []
    freq = [0] * 320                                   # lit/len symbols, then 32 distance symbols from 288
    c_tf = c_tf1 = c_win = c_exh = c_nice = c_col = 0

    def find(p, limit):
        nonlocal c_tf, c_tf1, c_win, c_exh, c_nice, c_col
        if limit < 3:
            return 0, 0
        if limit > MAX_LEN:
            limit = MAX_LEN
        best, bd, c, depth = 2, 0, prev[p], 0
        while c:
            if depth >= chain_len:
                c_exh += 1
                break
            depth += 1
            q = c - 1
            if p - q > WINDOW:
                c_win += 1
                break
            if b[q + best] == b[p + best] and b[q] == b[p]:
                if b[q + limit - 1] == b[p + limit - 1] and b[q:q + limit] == b[p:p + limit]:
                    ln = limit
                else:
                    ln = 1
                    while ln < limit and b[q + ln] == b[p + ln]:
                        ln += 1
                if ln > best:
                    best, bd = ln, p - q
                    if ln >= nice or ln == limit:
                        c_nice += ln >= nice
                        break
            elif b[q:q + 3] != b[p:p + 3]:
                c_col += 1
            c = prev[q]
        if best < 3:
            return 0, 0
        if best == 3 and bd > TOO_FAR:
            c_tf += 1
            c_tf1 += bd == TOO_FAR + 1
            return 0, 0
        return best, bd

    for s0 in range(0, n, SEGLEN):
        s1 = min(n, s0 + SEGLEN)
        p = s0
        ln, dist = find(p, s1 - p)
        while p < s1:
            if ln >= 3:
                if lazy and ln < LAZY and p + 1 < s1:
                    l1, d1 = find(p + 1, s1 - p - 1)
                    if l1 > ln:
                        toks.append(b[p]); freq[b[p]] += 1
                        st.lazy_taken += 1
                        p += 1; ln, dist = l1, d1
                        continue
                    st.lazy_equal += l1 == ln
                elif lazy and ln >= LAZY:
                    st.lazy_long += 1
                toks.append(-(ln << 16 | dist))
                lc, dc = LEN_CODE[ln], DIST_CODE[dist]
                freq[257 + lc] += 1; freq[288 + dc] += 1
                st.len_codes.add(lc); st.dist_codes.add(dc); st.len_values.add(ln); st.dist_values.add(dist)
                st.max_len, st.max_dist = max(st.max_len, ln), max(st.max_dist, dist)
                if ln == 3:
                    st.match3_4096 += dist == 4096
                if p + ln == s1 and s1 < n and b[s1] == b[s1 - dist]:
                    st.segment_cut += 1
                p += ln
            else:
                toks.append(b[p]); freq[b[p]] += 1
                p += 1
            ln, dist = find(p, s1 - p) if p < s1 else (0, 0)
    st.too_far, st.match3_4097, st.window_cut, st.chain_exhausted, st.nice_stop, st.collisions = c_tf, c_tf1, c_win, c_exh, c_nice, c_col
    return toks, freq


def build_lengths(f, maxbits):
    """code lengths of the symbols with counts f (at least two non-zero), limited to maxbits, and the depth the tree had before the limit"""
    n = len(f)
    lens = [0] * n
    rank = sorted((i for i in range(n) if f[i]), key=lambda i: (f[i], i))
    m = len(rank)
    A = [f[i] for i in rank]
    # Moffat & Katajainen, in place: A[i] becomes the code length of the i-th symbol in ascending order of count
    A[0] += A[1]
    root, leaf = 0, 2
    for nxt in range(1, m - 1):
        if leaf >= m or A[root] < A[leaf]:
            A[nxt] = A[root]; A[root] = nxt; root += 1
        else:
            A[nxt] = A[leaf]; leaf += 1
        if leaf >= m or (root < nxt and A[root] < A[leaf]):
            A[nxt] += A[root]; A[root] = nxt; root += 1
        else:
            A[nxt] += A[leaf]; leaf += 1
    A[m - 2] = 0
    for nxt in range(m - 3, -1, -1):
        A[nxt] = A[A[nxt]] + 1
    avbl, used, dpth, root, nxt = 1, 0, 0, m - 2, m - 1
    while avbl > 0:
        while root >= 0 and A[root] == dpth:
            used += 1; root -= 1
        while avbl > used:
            A[nxt] = dpth; nxt -= 1; avbl -= 1
        avbl, dpth, used = 2 * used, dpth + 1, 0
    depth = max(A[:m])
    # miniz's limit: counts per length, the longer ones folded into maxbits, the Kraft sum brought back to one
    cnt = [0] * 33
    for i in range(m):
        cnt[min(A[i], 32)] += 1
    for i in range(maxbits + 1, 33):
        cnt[maxbits] += cnt[i]; cnt[i] = 0
    total = sum(cnt[i] << (maxbits - i) for i in range(maxbits, 0, -1))
    while total != 1 << maxbits:
        cnt[maxbits] -= 1
        for i in range(maxbits - 1, 0, -1):
            if cnt[i]:
                cnt[i] -= 1; cnt[i + 1] += 2
                break
        total -= 1
    k = m - 1
    for ln in range(1, maxbits + 1):
        for _ in range(cnt[ln]):
            lens[rank[k]] = ln; k -= 1
    return lens, depth


def canonical(lens):
    """bit-reversed canonical codes of the lengths"""
    bl = [0] * 16
    for ln in lens:
        bl[ln] += 1
    bl[0] = 0
    nxt, c = [0] * 16, 0
    for b in range(1, 16):
        c = (c + bl[b - 1]) << 1
        nxt[b] = c
    codes = []
    for ln in lens:
        if ln:
            codes.append(int(format(nxt[ln], f"0{ln}b")[::-1], 2)); nxt[ln] += 1
        else:
            codes.append(0)
    return codes


def rle(seq):
    """the run-length coded code-length sequence: (symbol, extra) pairs"""
    out, i, ns = [], 0, len(seq)
    while i < ns:
        v, run = seq[i], 1
        while i + run < ns and seq[i + run] == v:
            run += 1
        if v == 0 and run >= 3:
            r = run
            while r >= 11:
                c = min(r, 138); out.append((18, c - 11)); r -= c
            if r >= 3:
                out.append((17, r - 3)); r = 0
            out.extend([(0, 0)] * r)
        elif v != 0 and run >= 4:
            out.append((v, 0))
            r = run - 1
            while r >= 3:
                c = min(r, 6); out.append((16, c - 3)); r -= c
            out.extend([(v, 0)] * r)
        else:
            out.extend([(v, 0)] * run)
        i += run
    return out


RLE_EXTRA = {16: (2, 3), 17: (3, 3), 18: (7, 11)}   # extra bits, the repeat count of extra 0


class BitWriter:
    def __init__(self):
        self.out, self.acc, self.nacc, self.nbits = bytearray(), 0, 0, 0

    def put(self, v, nb):
        self.acc |= v << self.nacc
        self.nacc += nb
        self.nbits += nb
        while self.nacc >= 8:
            self.out.append(self.acc & 255); self.acc >>= 8; self.nacc -= 8

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.nacc else b"")


def header_tables(freq, st=None):
    """everything of the dynamic block header from the symbol counts (freq: 288 lit/len + 32 distance slots, EOB not yet counted); st gets the stats"""
    st = st if st is not None else PieceStats()
    freq = list(freq)
    freq[256] = 1
    dist = freq[288:318]
    used = sum(1 for x in dist if x)
    i = 0
    while used < 2:
        if not dist[i]:
            dist[i] = 1; used += 1; st.pad_dist += 1
        i += 1
    llen, st.depth_litlen = build_lengths(freq[:286], 15)
    dlen, st.depth_dist = build_lengths(dist, 15)
    llen += [0, 0]
    hlit = 286
    while hlit > 257 and not llen[hlit - 1]:
        hlit -= 1
    hdist = 30
    while hdist > 1 and not dlen[hdist - 1]:
        hdist -= 1
    seq = llen[:hlit] + dlen[:hdist]
    i = 0
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        (st.rep_runs if seq[i] else st.zero_runs).add(j - i)
        i = j
    r = rle(seq)
    clfreq = [0] * 19
    for sym, ex in r:
        clfreq[sym] += 1
        if sym >= 16:
            st.rle_count[sym] += 1
            st.rle_max[sym] = max(st.rle_max[sym], ex + RLE_EXTRA[sym][1])
            st.rle_runs.add((sym, ex + RLE_EXTRA[sym][1]))
    cu = sum(1 for x in clfreq if x)
    i = 0
    while cu < 2:
        if not clfreq[i]:
            clfreq[i] = 1; cu += 1; st.pad_codelen += 1
        i += 1
    cllen, st.depth_codelen = build_lengths(clfreq, 7)
    hclen = 19
    while hclen > 4 and not cllen[CL_ORDER[hclen - 1]]:
        hclen -= 1
    st.hlit, st.hdist, st.hclen = hlit, hdist, hclen
    return llen, dlen, cllen, r, hlit, hdist, hclen


def _deflate_piece(b, level, st):
    """the raw DEFLATE bytes of one piece"""
    n = len(b)
    pr = params(level)
    if pr is not None:
        prev = chain(b).tolist()
        toks, freq = _parse(b, prev, pr[0], pr[1], pr[2], st)
        llen, dlen, cllen, r, hlit, hdist, hclen = header_tables(freq, st)
        lcode, dcode, clcode = canonical(llen), canonical(dlen), canonical(cllen)
        bits = 3 + 5 + 5 + 4 + 3 * hclen + sum(cllen[s] + (RLE_EXTRA[s][0] if s >= 16 else 0) for s, _ in r)
        for t in toks:
            if t >= 0:
                bits += llen[t]
            else:
                ln, d = (-t) >> 16, (-t) & 0xffff
                lc, dc = LEN_CODE[ln], DIST_CODE[d]
                bits += llen[257 + lc] + LEN_EXTRA[lc] + dlen[dc] + DIST_EXTRA[dc]
        bits += llen[256]
        st.margin = (bits + 7) // 8 - (n + 5)
        if st.margin < 0:
            w = BitWriter()
            w.put(1 | 2 << 1, 3)
            w.put(hlit - 257, 5); w.put(hdist - 1, 5); w.put(hclen - 4, 4)
            for i in range(hclen):
                w.put(cllen[CL_ORDER[i]], 3)
            for s, ex in r:
                w.put(clcode[s], cllen[s])
                if s >= 16:
                    w.put(ex, RLE_EXTRA[s][0])
            for t in toks:
                if t >= 0:
                    w.put(lcode[t], llen[t])
                else:
                    ln, d = (-t) >> 16, (-t) & 0xffff
                    lc, dc = LEN_CODE[ln], DIST_CODE[d]
                    w.put(lcode[257 + lc], llen[257 + lc]); w.put(ln - LEN_BASE[lc], LEN_EXTRA[lc])
                    w.put(dcode[dc], dlen[dc]); w.put(d - DIST_BASE[dc], DIST_EXTRA[dc])
            w.put(lcode[256], llen[256])
            assert w.nbits == bits
            return w.bytes()
    st.stored = 1
    return bytes([1, n & 255, n >> 8, ~n & 255, (~n >> 8) & 255]) + bytes(b)


def member(piece, level=None, st=None):
    """one BGZF member of a piece (at most PIECE bytes)"""
    st = st if st is not None else PieceStats()
    b = bytes(piece)
    if params(level) is not None:
        _lookback_stats(b, st)
    z = _deflate_piece(b, level, st)
    total = 18 + len(z) + 8
    return HEADER + (total - 1).to_bytes(2, "little") + z + zlib.crc32(b).to_bytes(4, "little") + len(b).to_bytes(4, "little")


def compress_stats(data, level=None):
    data = bytes(data)
    out, stats = [], []
    for o in range(0, len(data), PIECE):
        st = PieceStats()
        out.append(member(data[o:o + PIECE], level, st))
        stats.append(st)
    return b"".join(out), stats


def compress(data, level=None):
    """the bytes of ngsqc.bgzf_compress(data, level=level)"""
    return compress_stats(data, level)[0]
