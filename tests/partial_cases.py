"""Designed member geometry for the handles that do not see the whole file: shards (open_common of csrc/image.hip, the shard half of index_tile in
csrc/tiles.hip, ngsqc_plan_shard_fix of csrc/jobs.hip), virtual-offset ranges and heads (open_range_common). test_cpu_partial_model.py holds the premises,
test_gpu_partial_designed.py the library. Plain Python, no GPU, no library call.

A case is a k2geom_cases.Case (an explicit inflated stream plus explicit member cuts, written with cram_twin._bgzf at test time) and the runs it is opened
under: shard counts N with a tile layout (NGSQC_TILE_MEMBERS unset, 1, 2), tail settings (NGSQC_SHARD_TAIL_MEMBERS), virtual-offset ranges, head requests.
Which byte a shard border falls on depends on the COMPRESSED sizes, so the builders search the N that put a border where the case wants it, on the image
they have just written, and list what they found as the case's premises; the CPU test recomputes every premise with the model.

The sequential model (Model) reads the written file by its 18-byte member headers and the stream by one loop over block_size:
  member table  file offset, payload offset, inflated offset and size of every member; the library's table leaves members of ISIZE 0 out
  shard plan    first_member_at(s): the first member whose payload offset is >= int(n * s / N); a shard owns the records that start in [upos(m0), upos(m1))
                at or behind the first record; (n_records, first_abs, exit_abs), the local offsets (global - upos(m0)), the bytes inflated() returns
  tail need     the members behind m1 that the last owned record reaches into: NGSQC_SHARD_TAIL_MEMBERS below that must refuse
  range plan    the members walked for (beg_voff, end_voff), the owned records, and that a range that starts inside the header members never starts in
                front of the first record
  head plan     the member that holds the first record, own_end, the tail, the owned records
Three value-only mutations of the model (Model(mut=...)) are what the premises must tell apart from it: `le` (<= for < at the shard limit), `tail` (one
tail member less) and `member_start` (the target of first_member_at compared with the member's start instead of its payload's)."""
import struct

import numpy as np

import cram_twin
import k2geom_cases as K

EOF_BYTES = 28           # the empty member that ends the file
DEFAULT_TAIL = 64        # NGSQC_SHARD_TAIL_MEMBERS unset
E_FORMAT, E_ARG = -2, -3   # NGSQC_E_FORMAT, NGSQC_E_ARG of include/ngsqc.h (test_cpu_partial_model.py reads them from the header)
MSG_TAIL = "longer than the members read behind the shard (raise NGSQC_SHARD_TAIL_MEMBERS)"
MSG_BEHIND = "virtual offset behind the end of the file"
MSG_NO_BLOCK = "virtual offset does not name a BGZF block of this file"
MSG_JOIN = "but the previous shard's record chain ends at"


def image(c):
    """the bytes Case.write() writes"""
    return b"".join(cram_twin._bgzf(c.raw[lo:lo + n]) for lo, n in c.pieces()) + cram_twin._bgzf(b"")


def members(img):
    """(file offset, payload offset, inflated offset, inflated size) of every member, by the 18-byte headers"""
    out, off, u = [], 0, 0
    while off < len(img):
        assert img[off:off + 4] == b"\x1f\x8b\x08\x04" and img[off + 12:off + 16] == b"BC\x02\0"
        xlen, = struct.unpack_from("<H", img, off + 10)
        bsize = struct.unpack_from("<H", img, off + 16)[0] + 1
        isize, = struct.unpack_from("<I", img, off + bsize - 4)
        out.append((off, off + 12 + xlen, u, isize)); u += isize; off += bsize
    assert off == len(img)
    return out


class Model:
    def __init__(self, c, img, mut=None):
        assert mut in (None, "le", "tail", "member_start")
        self.c, self.img, self.n, self.mut = c, img, len(img), mut
        self.all = members(img)
        self.tab = [m for m in self.all if m[3] > 0]          # the library's member table
        self.by_off = {m[0]: k for k, m in enumerate(self.all)}
        self.offs = c.walk(); self.ends = np.append(self.offs[1:], len(c.raw))
        self.total, self.first_rec = len(c.raw), c.first_rec
        assert self.all[-1][3] == 0 and self.n - self.all[-1][0] == EOF_BYTES and sum(m[3] for m in self.all) == self.total

    def upos(self, m):
        return self.tab[m][2] if m < len(self.tab) else self.total

    # ---- shards ----
    def first_member_at(self, s, N):
        nb = len(self.tab)
        if s <= 0:
            return 0
        if s >= N:
            return nb
        target = int(self.n * s / N)
        col = 0 if self.mut == "member_start" else 1
        for m in range(nb):
            if self.tab[m][col] >= target:
                return m
        return nb

    def shard(self, s, N, tail=None):
        """what shard s of N owns and reports. kind: "empty" (no member), "header" (header bytes only: the handle drops its members), "plain"."""
        tail = DEFAULT_TAIL if tail is None else tail
        if self.mut == "tail":
            tail = max(tail - 1, 0)
        nb = len(self.tab)
        m0, m1 = self.first_member_at(s, N), self.first_member_at(s + 1, N)
        r = dict(m0=m0, m1=m1, kind="plain", n_blocks=0, inflated=(0, 0), own_bytes=0, need=0, refuses=False)
        none = dict(n_records=0, first_abs=-1, exit_abs=-1, owned=np.zeros(0, np.int64), local=np.zeros(0, np.int64))
        if m1 == m0:
            return dict(r, kind="empty", **none)
        u0, lim = self.upos(m0), self.upos(m1)
        if self.first_rec >= lim:
            return dict(r, kind="header", **none)
        m_end = min(nb, m1 + tail)
        u_all = self.upos(m_end)
        r.update(n_blocks=m_end - m0, inflated=(u0, u_all), own_bytes=lim - u0, u0=u0, lim=lim)
        mine = (self.offs >= u0) & ((self.offs <= lim) if self.mut == "le" else (self.offs < lim))
        owned = self.offs[mine]
        if owned.size == 0:
            return dict(r, **none)
        last_end = int(self.ends[mine][-1])
        need = sum(1 for m in range(m1, nb) if self.tab[m][2] < last_end)
        behind = self.offs[self.offs >= lim] if self.mut != "le" else self.offs[self.offs > lim]
        return dict(r, need=need, refuses=need > tail, n_records=int(owned.size), first_abs=int(owned[0]), exit_abs=int(behind[0]) if behind.size else self.total,
                    owned=owned, local=owned - u0)

    def shards(self, N, tail=None):
        return [self.shard(s, N, tail) for s in range(N)]

    def shard_borders(self, N):
        """inflated offsets of the borders between shards that both hold members"""
        nb = len(self.tab)
        return sorted({self.upos(m) for m in (self.first_member_at(s, N) for s in range(1, N)) if 0 < m < nb})

    # ---- virtual offsets ----
    def voff(self, o):
        """virtual offset of inflated offset o (of a byte that exists)"""
        for off, _, u, n in self.all:
            if u <= o < u + n:
                return off << 16 | (o - u)
        raise AssertionError(o)

    def _walked(self, co_beg, bound):
        return [m for m in self.all if co_beg <= m[0] < bound]

    def range(self, beg, end, own_end=0):
        """the handle over (beg, end): refuses = (code, message) or None; n_blocks, inflated = (lo, hi) global, owned, local; cut: the last owned record
        reaches behind the members walked (the library refuses with MSG_TAIL, shard 0)"""
        out = dict(refuses=None, n_blocks=0, inflated=(0, 0), owned=np.zeros(0, np.int64), local=np.zeros(0, np.int64), n_records=0, cut=False)
        if end <= beg:
            return out
        co_beg, co_end = beg >> 16, end >> 16
        if co_beg >= self.n or co_end > self.n:
            return dict(out, refuses=(E_ARG, MSG_BEHIND))
        if co_beg not in self.by_off:
            return dict(out, refuses=(E_ARG, MSG_NO_BLOCK))
        walked = [m for m in self._walked(co_beg, co_end + 1 if end & 0xffff else co_end) if m[3] > 0]
        if walked and walked[0][0] != co_beg and beg & 0xffff:
            return dict(out, refuses=(E_ARG, MSG_NO_BLOCK))
        if not walked:
            return out
        base, hi = walked[0][2], walked[-1][2] + walked[-1][3]
        if own_end:
            limit = next((m[2] for m in walked if m[0] >= own_end), hi)
        elif end & 0xffff == 0:
            limit = hi
        else:
            if walked[-1][0] != co_end:
                return dict(out, refuses=(E_ARG, MSG_NO_BLOCK))
            limit = walked[-1][2] + (end & 0xffff)
        first = max(base + (beg & 0xffff), self.first_rec)    # a range that starts inside the header members never starts in front of the first record
        mine = (self.offs >= first) & (self.offs < max(limit, first))
        owned = self.offs[mine]
        cut = bool(owned.size and self.ends[mine][-1] > hi)
        return dict(out, n_blocks=len(walked), inflated=(base, hi), owned=owned, local=owned - base, n_records=int(owned.size), cut=cut,
                    refuses=(E_FORMAT, MSG_TAIL) if cut else None)

    def head(self, n_members, tail=None):
        """the handle over the first n_members members from the one that holds the first record: plan = (beg, own_end, end) and the range's result"""
        tail = DEFAULT_TAIL if tail is None else tail
        a0 = next((k for k, m in enumerate(self.all) if m[3] > 0 and m[2] + m[3] > self.first_rec), None)
        if a0 is None:
            return dict(self.range(0, 0), plan=None)
        beg = self.all[a0][0] << 16 | (self.first_rec - self.all[a0][2])
        k1 = a0 + n_members
        o3 = self.all[k1][0] if k1 < len(self.all) else self.n
        own_end, end = 0, o3
        if o3 < self.n and tail > 0:
            own_end = o3
            k2 = k1 + tail
            end = self.all[k2][0] if k2 < len(self.all) else self.n
        return dict(self.range(beg, end << 16, own_end), plan=(beg, own_end, end))

    def rec_voff(self, i):
        return self.voff(int(self.offs[i])) if i < self.offs.size else self.n << 16


# ---- the cases ----
class PCase:
    """case: the k2geom Case; img: its file; shard_runs: [(N, tile_members)]; tails: [(N, tail)] runs under NGSQC_SHARD_TAIL_MEMBERS; ranges: [(tag, beg, end,
    tile_members)]; heads: [(tag, n_members, tail, tile_members)]; decoy: the case may refuse with NGSQC_E_FORMAT instead of the model's result"""

    def __init__(self, name, case, shard_runs=(), tails=(), ranges=(), heads=(), premises=None, decoy=None):
        self.name, self.case, self.img = name, case, image(case)
        self.shard_runs, self.tails, self.ranges, self.heads = list(shard_runs), list(tails), list(ranges), list(heads)
        self.premises, self.decoy = premises or {}, decoy
        assert len(self.img) < 1 << 20

    def model(self, mut=None):
        return Model(self.case, self.img, mut)

    def write(self, path):
        open(path, "wb").write(self.img)
        return path


def _noise(i, n, lo, span):
    """n bytes lo .. lo + span - 1 that deflate cannot shorten much"""
    return [lo + K._mix(i * 100003 + k) % span for k in range(n)]


def add_long(s, l_seq, tail_bytes=b""):
    """a mapped record of l_seq bases without optional fields whose bases and qualities do not compress (so that members cut from it are as large in the file
    as members of short records); tail_bytes: its last quality bytes. 42 + l_seq // 2 + l_seq (+ 1 for odd l_seq) bytes."""
    i = len(s.offs); h = K._mix(i); tid, pos = s.where()
    qual = _noise(i, l_seq - len(tail_bytes), 2, 40) + list(tail_bytes)
    seq = [(1, 2, 4, 8, 15)[x] for x in _noise(i + 7, l_seq, 0, 5)]
    r = K._pack(tid, pos, b"a\0", 60, [(0, l_seq)], 0x1 | 0x2 | 0x40 if h & 1 else 0, seq, qual, 300)
    s.mapped.append(i); s.offs.append(len(s.raw)); s.raw += r
    return i


def size_long(l_seq):
    return 42 + (l_seq + 1) // 2 + l_seq


def _cuts_hit(m, N):
    """bytes of a record in front of every shard border of N (0: a record's end, -1: header)"""
    return m.c.border_cuts(m.shard_borders(N))


def _search(m, want, n_range):
    """greedy: the N of n_range that add something to `want`: {key: predicate(m, N) -> bool}. Returns ([N], {key: N})"""
    chosen, found = [], {}
    n_range = list(n_range)
    for N in n_range:   # one N that does it all, if there is one
        if all(f(m, N) for f in want.values()):
            return [N], {k: N for k in want}
    for N in n_range:
        new = [k for k, f in want.items() if k not in found and f(m, N)]
        if new:
            chosen.append(N)
            found.update({k: N for k in new})
        if len(found) == len(want):
            break
    assert len(found) == len(want), sorted(set(want) - set(found), key=str)
    return chosen, found


def _layouts(ns, tms=(None, 1, 2)):
    return [(N, tm) for N in ns for tm in tms]


def _border_at(u):
    """predicate: a shard of N starts at inflated offset u"""
    return lambda m, N: u in m.shard_borders(N)


def case_shard_borders():
    """members of 24 records with their borders 1, 2, 3, 4, 20, 35 and 36 bytes into a record and at a record's end; the N are searched so that every one of
    these borders is a shard border"""
    s = K.Stream(x_from=160)
    cuts, at = [], {}
    s.fill(20)
    for d in K.CUT_AT:
        s.fill(23)
        i = s.add(44)
        cuts.append(s.offs[i] + d if d else s.end())
        at[d] = cuts[-1]
    s.fill(30)
    c = K.Case("shard_borders", s, cuts)
    p = PCase("shard_borders", c)
    m = p.model()
    ns, found = _search(m, {d: _border_at(u) for d, u in at.items()}, range(2, 200))
    p.premises = dict(cut_at=found, at=at)
    p.shard_runs = _layouts(ns)
    p.ranges = _generic_ranges(m)
    return p


def case_shard_header():
    """the header of 1500 references (75 KB) of k2geom's header_end in members of 20 000 bytes, the first record at a member start: shards that hold header bytes only, the shard
    in which the header ends (it knows its first record and starts in front of it), a shard that starts exactly at the first record"""
    c = K.get("header_end")
    p = PCase("shard_header", c)
    m = p.model()
    want = {
        "header_only": lambda m, N: any(x["kind"] == "header" for x in m.shards(N)),
        "header_ends_inside": lambda m, N: any(x["kind"] == "plain" and 0 < x["u0"] < m.first_rec < x["lim"] for x in m.shards(N)),
        "first_rec_at_start": lambda m, N: any(x["kind"] == "plain" and x["u0"] == m.first_rec for x in m.shards(N)),
    }
    ns, found = _search(m, want, range(2, 200))
    p.premises = dict(found)
    p.shard_runs = _layouts(ns, (None, 1))
    return p


TINY_RUN = (1, 2, 3, 0, 1, 1, 2, 3, 3, 0, 2, 1, 1)   # eleven tiny members (and two empty ones) inside one record


def case_shard_tiny():
    """empty members and members of 1 - 3 bytes: an empty member between two records, a member of one byte inside a block_size word, a run of eleven tiny
    members inside one record. N = members, members + 1 and 16 x members (every member start a shard border, the one inside block_size included), and the N
    at which one shard holds tiny members of the run alone"""
    s = K.Stream(x_from=150)
    cuts = []
    s.fill(12); cuts.append(s.end()); s.fill(12)
    empty_at = s.end()
    cuts += [s.end(), s.end()]
    s.fill(8)
    i = s.add(44); word = s.offs[i] + 2; cuts += [word, word + 1]    # a member of one byte: the third byte of block_size
    s.fill(10)
    i = s.add(44); cuts += [s.end(i - 1), s.offs[i] + 3]             # a member of three bytes: the first three bytes of block_size
    s.fill(10)
    i = s.add(44)
    o = s.offs[i] + 10; run_lo = o
    for n in TINY_RUN:
        cuts.append(o); o += n
    cuts.append(o); run_hi = o
    s.fill(12); cuts.append(s.end())
    s.fill(12)
    c = K.Case("shard_tiny", s, cuts)
    p = PCase("shard_tiny", c)
    m = p.model()
    nb = len(m.tab)
    inside_run = lambda x: x["kind"] == "plain" and x["m1"] - x["m0"] >= 2 and run_lo <= x["u0"] and x["lim"] <= run_hi and x["n_records"] == 0
    want = {"word_split": _border_at(word + 1), "tiny_shard": lambda m, N: any(inside_run(x) for x in m.shards(N))}
    ns, found = _search(m, want, [nb, nb + 1, 16 * nb] + list(range(2, 16 * nb)))
    p.premises = dict(found, members=nb, empty=[k for k, x in enumerate(m.all[:-1]) if x[3] == 0], word=word, run=(run_lo, run_hi), empty_at=empty_at)
    big = 16 * nb
    p.shard_runs = _layouts(sorted(set(ns) - {nb, nb + 1, big})) + [(N, tm) for N in (nb, nb + 1) for tm in (None, 1)] + [(big, None)]
    p.ranges = _generic_ranges(m, empty_at=empty_at)
    return p


def _long_file(name, plan, x_from):
    """records of 44 bytes in members of 24 and, for every (l_seq, [cut offsets into the record]) of plan, a long record cut there, ten records and a cut at a
    record end behind it. Returns (stream, cuts, [(record, [cut positions])])"""
    s = K.Stream(x_from=x_from)
    cuts, longs = [], []
    s.fill(24); cuts.append(s.end())
    for l_seq, at in plan:
        s.fill(14)
        i = add_long(s, l_seq)
        here = [s.offs[i] + a for a in at]
        assert all(a < size_long(l_seq) for a in at)
        cuts += here; longs.append((i, here))
        s.fill(10); cuts.append(s.end())
        s.fill(24); cuts.append(s.end())
    s.fill(20)
    return s, cuts, longs


def case_shard_long():
    """three long records that reach 1, 2 and 3 members behind the member they start in: with every member a shard of its own, the shard of each needs exactly
    T = 1, 2, 3 tail members, the second covers one whole shard and the third two. NGSQC_SHARD_TAIL_MEMBERS = T - 1 refuses that shard, T does not"""
    s, cuts, longs = _long_file("shard_long", [(1700, [900]), (2300, [900, 1800]), (2700, [900, 1800, 2700])], x_from=400)
    c = K.Case("shard_long", s, cuts)
    p = PCase("shard_long", c)
    m = p.model()
    borders = [u for _, here in longs for u in here] + [int(m.c.offs[i + 11]) for i, _ in longs]   # every cut of a long record, and the record end behind it
    ns, found = _search(m, {"single": lambda m, N: set(borders) <= set(m.shard_borders(N))}, range(len(m.tab), 40 * len(m.tab)))
    N = ns[0]
    p.premises = dict(N=N, longs=[i for i, _ in longs], need=[1, 2, 3], covered=[0, 1, 2])
    p.shard_runs = _layouts([N], (None, 1))
    p.tails = [(N, t) for t in (0, 1, 2, 3)]
    p.ranges = _generic_ranges(m, longs=longs)
    return p


def case_shard_last():
    """the file's last record straddles into a last member of one byte: the last shard owns only that member, and no record"""
    s = K.Stream(x_from=60)
    s.fill(16); cuts = [s.end()]
    s.fill(16)
    cuts.append(len(s.raw) - 1)
    c = K.Case("shard_last", s, cuts)
    p = PCase("shard_last", c)
    m = p.model()
    nb = len(m.tab)
    ns, found = _search(m, {"last_alone": lambda m, N: m.first_member_at(N - 1, N) == nb - 1}, range(2, 400))
    p.premises = dict(found, members=nb)
    p.shard_runs = _layouts(ns + [2])
    p.tails = [(ns[0], 0), (ns[0], 1)]
    return p


def case_shard_tiles():
    """a record of 4.6 KB cut every 900 bytes, and shards of several members that start at its second and at its third cut: under NGSQC_TILE_MEMBERS=1 the
    record covers the first two tiles (the first tile) of such a shard, under NGSQC_TILE_MEMBERS=2 the first tile - a shard whose first tile finds no record
    start has to keep guessing in the next one. (The number of members behind the record is the smallest that lets some N put its borders there.)"""
    def starts_at(u, k, end):   # a shard of more than k members whose first k members lie inside the record, and which owns records
        return lambda m, N: any(x["kind"] == "plain" and x["u0"] == u and x["m1"] - x["m0"] >= k + 1 and m.upos(x["m0"] + k) < end and x["n_records"] > 0 for x in m.shards(N))
    for behind in range(4, 40):
        s, cuts, longs = _long_file("shard_tiles", [(3050, [900, 1800, 2700, 3600])], x_from=300)
        for _ in range(behind):
            s.fill(24); cuts.append(s.end())
        s.fill(10)
        p = PCase("shard_tiles", K.Case("shard_tiles", s, cuts))
        m = p.model()
        (i, here), = longs
        end = int(m.c.offs[i + 1])
        try:
            ns, found = _search(m, {"two_tiles": starts_at(here[1], 2, end), "one_tile": starts_at(here[2], 1, end)}, range(2, 40))
        except AssertionError:
            continue
        p.premises = dict(found, record=i, cuts=here, members_behind=behind)
        p.shard_runs = _layouts(ns)
        p.ranges = [("tiles1", m.rec_voff(3), m.rec_voff(i + 5), 1), ("tiles2", m.rec_voff(3), m.rec_voff(i + 5), 2)]
        return p
    raise AssertionError("no N puts a shard border at the record's cuts")


N_DECOYS = 24


def case_decoy(dies):
    """a host record of 45 KB over three members whose last quality bytes are a verbatim chain of 24 records of 44 bytes on chrX (no true record lies there);
    the shard border falls inside the host record, in front of them, and no true record starts in that member. rejoin: the decoys run to the host record's
    last byte, their chain joins the true one; dies: ten other bytes follow them"""
    d = K.Stream(x_from=0)
    d.fill(N_DECOYS)
    decoys = bytes(d.raw[d.first_rec:])
    tail = decoys + (bytes([30] * 10) if dies else b"")
    s = K.Stream(x_from=1 << 60)
    s.fill(200)
    cuts = [s.end()]
    s.fill(100)
    host = add_long(s, 30000, tail_bytes=tail)
    o = s.offs[host]
    cuts += [o, o + 18000, o + 36000, s.end()]
    for _ in range(4):
        s.fill(250); cuts.append(s.end())
    s.fill(100)
    name = "shard_decoy_dies" if dies else "shard_decoy_rejoin"
    c = K.Case(name, s, cuts)
    p = PCase(name, c, decoy=dict(host=host, first=s.end(host) - len(tail), n=N_DECOYS, member_at=o + 36000))
    m = p.model()
    ns, found = _search(m, {"border": lambda m, N: any(x["kind"] == "plain" and x["u0"] == o + 36000 and x["n_records"] > 100 for x in m.shards(N))}, range(2, 60))
    p.premises = dict(found)
    p.shard_runs = _layouts(ns[:1])
    return p


def _generic_ranges(m, empty_at=None, longs=()):
    """the range cases a file allows; every beg and end is a record start (or the end of the file)"""
    nrec = m.offs.size
    out = []
    # beg and end inside one member: the second and the last record that start in the member that holds the most record starts
    k = max(range(len(m.tab)), key=lambda k: int(((m.offs >= m.tab[k][2]) & (m.offs < m.tab[k][2] + m.tab[k][3])).sum()))
    inside = np.nonzero((m.offs >= m.tab[k][2]) & (m.offs < m.tab[k][2] + m.tab[k][3]))[0]
    out.append(("one_member", m.rec_voff(int(inside[1])), m.rec_voff(int(inside[-1])), None))
    third = nrec // 3
    out.append(("from_voff0", 0, m.rec_voff(third), None))
    out.append(("from_first_record", m.rec_voff(0), m.rec_voff(third), None))
    # end at in-block offset 0 of a member that starts with a record; of the EOF member; at file_size << 16
    at0 = [k for k in range(1, len(m.tab)) if m.tab[k][2] in set(m.offs.tolist())]
    out.append(("end_member_start", m.rec_voff(third), m.tab[at0[-1]][0] << 16, None))
    out.append(("end_eof_member", m.rec_voff(third), (m.n - EOF_BYTES) << 16, None))
    out.append(("end_file_size", m.rec_voff(2 * third), m.n << 16, None))
    for tm in (1, 2):
        out.append((f"tiles{tm}", m.rec_voff(5), m.rec_voff(nrec - 7), tm))
    if empty_at is not None:
        e = next(x for x in m.all if x[3] == 0 and x[2] == empty_at)     # the empty member in front of the record at empty_at
        nxt = m.all[m.by_off[e[0]] + 1]
        assert nxt[3] > 0 and nxt[2] == empty_at and empty_at in set(m.offs.tolist())
        out.append(("beg_empty_member", e[0] << 16, m.rec_voff(nrec - 3), None))
        out.append(("end_empty_member", m.rec_voff(2), e[0] << 16, None))
        out.append(("empty_members_only", e[0] << 16, nxt[0] << 16, None))
    for i, here in longs:   # the last owned record spans len(here) member borders
        out.append((f"last_spans_{len(here)}", m.rec_voff(max(i - 20, 0)), m.rec_voff(i + 1), None))
    out.append(("refuse_behind", m.n << 16, (m.n << 16) + 1, None))
    out.append(("refuse_no_block", (m.tab[1][0] + 5) << 16, m.n << 16, None))
    return out


def split_ranges(m, k):
    """k consecutive ranges at record starts that together cover the file"""
    at = [0] + [m.rec_voff(int(i)) for i in np.linspace(0, m.offs.size, k + 1)[1:-1].astype(int)] + [m.n << 16]
    return list(zip(at, at[1:]))


def case_head(kind):
    """head requests on a header of 1500 references (75 KB). hdr8: the header is exactly the first eight members - the walk for the header ends where the header
    does, and the member of the first record is fetched by the extra branch of open_range_common; mid: the header over four members, the first record 16.5 KB
    into the fourth. Both: member borders that cut records, so that the last own record of a head of k members is cut at own_end"""
    refs = K.REFS + [(f"scaffold_{k:04d}", 1000 + k) for k in range(1498)]
    s = K.Stream(refs=refs, x_from=500)
    H = s.first_rec
    if kind == "hdr8":
        cuts = [9000 * k for k in range(1, 8)] + [H]
        s.fill(100); cuts.append(s.end() - 20); s.fill(100); cuts.append(s.end() - 30); s.fill(100)
        heads = [("one", 1, None, None), ("two_tail0", 2, 0, None), ("more_than_left", 50, None, None), ("two_tiles1", 2, None, 1)]
    else:
        cuts = [20000, 40000, 60000]
        s.fill(70); cuts.append(s.end() - 20)       # the first record starts H - 60000 bytes into the fourth member
        s.fill(120); cuts.append(s.end() - 7)
        s.fill(120); cuts.append(s.end())
        s.fill(120)
        heads = [("cut_tail0", 1, 0, None), ("cut_tail1", 1, 1, None), ("cut_default", 1, None, None), ("two", 2, 1, None), ("three_end", 3, 0, None),
                 ("more_than_left", 9, None, None), ("cut_tiles1", 2, None, 1), ("cut_tiles2", 2, 1, 2)]
    name = "head_" + kind
    c = K.Case(name, s, cuts)
    return PCase(name, c, heads=heads, premises=dict(header=H))


def _reuse(name, ns, tms):
    """a k2geom case under shards"""
    return lambda: PCase("k2_" + name, K.get(name), shard_runs=_layouts(ns, tms))


BUILDERS = {
    "shard_borders": case_shard_borders, "shard_header": case_shard_header, "shard_tiny": case_shard_tiny, "shard_long": case_shard_long,
    "shard_last": case_shard_last, "shard_tiles": case_shard_tiles,
    "shard_decoy_rejoin": lambda: case_decoy(False), "shard_decoy_dies": lambda: case_decoy(True),
    "k2_borders": _reuse("borders", (3, 7), (None, 1, 2)), "k2_degenerate": _reuse("degenerate", (5, 12), (None, 1)),
    "k2_header_mid": _reuse("header_mid", (2, 9), (None, 1)), "k2_carry_full": _reuse("carry_full", (2, 3), (None, 1)),
    "head_hdr8": lambda: case_head("hdr8"), "head_mid": lambda: case_head("mid"),
}
ALL = list(BUILDERS)
SHARD_CASES = [n for n in ALL if n.startswith(("shard_", "k2_"))]
DECOYS = ("shard_decoy_rejoin", "shard_decoy_dies")
RANGE_CASES = ("shard_borders", "shard_tiny", "shard_long", "shard_tiles")
HEAD_CASES = ("head_hdr8", "head_mid")
_BUILT = {}


def get(name):
    if name not in _BUILT:
        _BUILT[name] = BUILDERS[name]()
    return _BUILT[name]
