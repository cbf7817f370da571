"""Designed member and tile geometry for the record index (K2): test_cpu_k2geom.py (model == oracle, premises, constants, the guess on the aligned cases) and
test_gpu_k2geom.py (the library against model and oracle under every path switch). Plain Python, no GPU, no library call.

A case is an inflated BAM stream (header + small records of chosen sizes) and an explicit list of member cut positions; write() lays it into BGZF members with
cram_twin._bgzf and ends it with an empty member. The sequential model below gives what the library must find: the record offsets (one loop over block_size),
the tiles of a layout (NGSQC_TILE_MEMBERS over the members that hold bytes: walk_bgzf leaves members of ISIZE 0 out of the member table, csrc/image.hip), the
bytes carried from tile to tile, and - with a restatement of entry_range (csrc/common.h) - the records of every entry at every walker shift. Every case carries
the numbers it was built to produce (Case.premises); the CPU test recomputes them with the model.

Records: 44 bytes (name "a\\0", CIGAR 1M, one base), or longer by a longer name; flag, MAPQ, position, l_seq (1 mapped; 3 or 4 on unmapped records without a
CIGAR, same size) and insert size vary from record to record, positions ascend (two records per position), so a record that is counted twice, skipped or read
at a wrong offset changes the mapping counters, the insert-size histogram, the depth or a site."""
import struct

import numpy as np

import cram_twin

# ---- the three constants the geometry hangs on (test_cpu_k2geom.py reads them from csrc/common.h and csrc/index.hip) ----
K2_REL_STRIDE = 512   # u16 offsets kept per member for the write pass; an entry of a member cut into 2^ksh pieces owns K2_REL_STRIDE >> ksh
NAME_SHIFT = 12       # a record of the riding scan is named entry << NAME_SHIFT | k; the walk refuses an entry at record (1 << NAME_SHIFT) - 1
SCAN_TILE = 4096      # items per workgroup of the three-kernel scans of the entry counts
NAME_CAP = (1 << NAME_SHIFT) - 1   # the most records an entry of the riding scan may hold

REFS = [("chr1", 3_000_000), ("chrX", 1_000_000)]
MEMBER_MAX = 65280
PAIRED = (0x1 | 0x2 | 0x40, 0x1 | 0x2 | 0x80 | 0x10, 0x1 | 0x40, 0x1 | 0x2 | 0x40 | 0x400, 0x1 | 0x2 | 0x80 | 0x100, 0x1 | 0x80 | 0x20)
UNPAIRED = (0, 0x10, 0x400, 0x100, 0x800 | 0x10, 0x200)
MAPQS = (0, 1, 19, 20, 37, 60, 255)


def stride(ksh):
    """rel_stride (csrc/common.h): offsets kept per entry; none for a group of members"""
    return K2_REL_STRIDE >> ksh if ksh >= 0 else 0


def _mix(i):
    x = (i * 2654435761 + 0x9E3779B9) & 0xFFFFFFFF
    x ^= x >> 15; x = (x * 2246822519) & 0xFFFFFFFF; x ^= x >> 13
    return x


def header(refs=REFS):
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs)
    h = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(refs))
    for n, ln in refs:
        h += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", ln)
    return h


def _pack(tid, pos, name, mapq, cigar, flag, seq, qual, isize):
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(name), mapq, 4680, len(cigar), flag, len(seq), tid, pos + 7, isize) + name
    codes = list(seq) + [0]
    body += b"".join(struct.pack("<I", ln << 4 | op) for op, ln in cigar) + bytes(codes[k] << 4 | codes[k + 1] for k in range(0, len(seq), 2)) + bytes(qual)
    return struct.pack("<I", len(body)) + body


class Stream:
    """records in file order; add() gives the next record its position (ascending, two per position; tid 1 from record x_from on)"""

    def __init__(self, refs=REFS, x_from=1 << 60):
        self.refs, self.x_from = refs, x_from
        self.raw = bytearray(header(refs))
        self.first_rec = len(self.raw)
        self.offs, self.mapped = [], []

    def __len__(self):
        return len(self.offs)

    def where(self):
        i = len(self.offs)
        return (0, 100 + i // 2) if i < self.x_from else (1, 100 + (i - self.x_from) // 2)

    def add(self, size=44, paired=True, l_seq=None):
        """one record of `size` bytes (>= 44; the name grows), or - l_seq given - a mapped record of l_seq bases (CIGAR l_seq M). Returns its index."""
        i = len(self.offs); h = _mix(i); tid, pos = self.where()
        nm = lambda n: bytes(97 + (h >> (3 * k)) % 26 for k in range(n)) + b"\0"
        bases = lambda n: [(1, 2, 4, 8, 15)[(h >> k) % 5] for k in range(n)]
        quals = lambda n: [2 + (h >> (k % 20)) % 40 for k in range(n)]
        flags = PAIRED + UNPAIRED if paired else UNPAIRED
        mapq, isize = MAPQS[(h >> 5) % 7], (h >> 9) % 2601 - 1300
        if l_seq is not None:
            r = _pack(tid, pos, nm(1), mapq, [(0, l_seq)], flags[(h >> 3) % len(flags)], bases(l_seq), quals(l_seq), isize)
            self.mapped.append(i)
        else:
            assert 44 <= size <= 44 + 250
            v, extra = h % 4, size - 44
            if v < 2:     # mapped: name "a", 1M, one base
                r = _pack(tid, pos, nm(1 + extra), mapq, [(0, 1)], flags[(h >> 3) % len(flags)], bases(1), quals(1), isize)
                self.mapped.append(i)
            else:         # unmapped (placed with its mate), no CIGAR: name "ab" and 3 bases, or name "a" and 4 bases - the same size
                ln = 3 if v == 2 else 4
                f = 0x4 | ((0x1 | 0x40 | 0x8 * ((h >> 3) & 1)) if paired and (h >> 4) & 1 else 0)
                r = _pack(tid, pos, nm((2 if v == 2 else 1) + extra), mapq, [], f, bases(ln), quals(ln), isize)
            assert len(r) == size, (len(r), size)
        self.offs.append(len(self.raw)); self.raw += r
        return i

    def fill(self, n, size=44, paired=True):
        for _ in range(n):
            self.add(size, paired)

    def end(self, i=None):
        """offset behind record i (default: behind the last record)"""
        return len(self.raw) if i is None or i + 1 >= len(self.offs) else self.offs[i + 1]


class Case:
    """raw: the inflated stream; cuts: member borders (ascending offsets into raw, a repeated offset = an empty member); layouts: the (NGSQC_TILE_MEMBERS,
    NGSQC_CARRY_MAX) pairs the case is run under (None: unset); aligned: a record starts at every member's first byte and none straddles; premises: the numbers
    the case was built to produce; expect: what the GPU test asserts about the path taken; refuses: the library's message when it must refuse the file"""

    def __init__(self, name, stream, cuts, layouts=((None, None),), aligned=False, premises=None, expect=None, refuses=None):
        self.name, self.raw, self.refs, self.first_rec = name, bytes(stream.raw), stream.refs, stream.first_rec
        self.offs = np.array(stream.offs, dtype=np.int64)
        self.mapped = list(stream.mapped)
        self.cuts = sorted(cuts)
        assert all(0 < c < len(self.raw) for c in self.cuts)
        self.layouts, self.aligned, self.premises, self.expect, self.refuses = tuple(layouts), aligned, premises or {}, expect or {}, refuses

    # ---- the writer ----
    def pieces(self):
        b = [0] + self.cuts + [len(self.raw)]
        return [(b[k], b[k + 1] - b[k]) for k in range(len(b) - 1)]

    def write(self, path):
        out = []
        for lo, n in self.pieces():
            assert n <= MEMBER_MAX
            out.append(cram_twin._bgzf(self.raw[lo:lo + n]))
        open(path, "wb").write(b"".join(out) + cram_twin._bgzf(b""))
        return path

    # ---- inputs of the job ----
    def bed(self):
        n = len(self.offs)
        hi1 = 100 + n // 2
        lines = [("chr1", 90, 100 + n // 8), ("chr1", 100 + n // 6, min(100 + n // 6 + 700, hi1 + 50)), ("chr1", max(hi1 - 300, 100 + n // 6 + 700), hi1 + 40), ("chrX", 0, 400)]
        return "".join(f"{c}\t{s}\t{e}\n" for c, s, e in lines if e > s)

    def sites(self):
        """1-based (tid, pos) of about forty mapped records spread over the file, the base in front of and behind each"""
        pos = {}
        step = max(1, len(self.mapped) // 40)
        for i in self.mapped[::step] + self.mapped[-3:]:
            tid, p = struct.unpack_from("<ii", self.raw, int(self.offs[i]) + 4)
            for q in (p, p + 1, p + 2):
                if q >= 1:
                    pos[(tid, q)] = 1
        return sorted(pos)

    # ---- the sequential model ----
    def walk(self):
        """record offsets by one loop over block_size"""
        out, o = [], self.first_rec
        while o < len(self.raw):
            out.append(o); o += 4 + struct.unpack_from("<I", self.raw, o)[0]
        assert o == len(self.raw)
        return np.array(out, dtype=np.int64)

    def members(self):
        """(upos, usize) of the members that hold bytes: the library's member table"""
        return [(lo, n) for lo, n in self.pieces() if n > 0]

    def tiles(self, tile_members):
        m = self.members()
        k = tile_members or len(m)
        return [m[a:a + k] for a in range(0, len(m), k)]

    def tile_model(self, tile_members):
        """per tile: dict(u_lo, u_hi, prefix = bytes carried in, carry = bytes carried out, starts = tile-local offsets of the records that end in this tile,
        members = [(upos relative to the tile's first member, usize)])"""
        offs = self.walk(); ends = np.append(offs[1:], len(self.raw))
        out, prefix, prev_hi = [], 0, -1
        for tm in self.tiles(tile_members):
            u_lo, u_hi = tm[0][0], tm[-1][0] + tm[-1][1]
            mine = (ends > prev_hi) & (ends <= u_hi)
            cut = np.nonzero((offs < u_hi) & (ends > u_hi))[0]
            carry = int(u_hi - offs[cut[0]]) if cut.size else 0
            out.append(dict(u_lo=u_lo, u_hi=u_hi, prefix=prefix, carry=carry, starts=offs[mine] - u_lo + prefix, members=[(lo - u_lo, n) for lo, n in tm]))
            prefix, prev_hi = carry, u_hi
        return out

    def entries(self, tile, ksh):
        """[lo, hi) of every entry of a tile, tile-local"""
        nm = len(tile["members"])
        ne = (nm << ksh) + 1 if ksh >= 0 else ((nm + (1 << -ksh) - 1) >> -ksh) + 1
        return [entry_range(tile["members"], e, tile["prefix"], ksh, nm) for e in range(ne)]

    def entry_counts(self, tile_members, ksh):
        """per tile: the records that start in each entry (and end inside the tile: the walker of the entry counts them)"""
        out = []
        for t in self.tile_model(tile_members):
            his = np.array([hi for _, hi in self.entries(t, ksh)], dtype=np.int64)
            e = np.searchsorted(his, t["starts"], side="right")   # the first entry that ends behind the start (entries are contiguous, empty ones included)
            out.append(np.bincount(e, minlength=his.size))
        return out

    def name_of(self, i, tile_members, ksh):
        """(tile, entry, k) of record i: its name in the riding scan"""
        o = int(self.walk()[i]); ends = np.append(self.walk()[1:], len(self.raw))
        for ti, t in enumerate(self.tile_model(tile_members)):
            s = o - t["u_lo"] + t["prefix"]
            if ends[i] <= t["u_hi"] and s >= 0 and s in set(t["starts"].tolist()):
                his = np.array([hi for _, hi in self.entries(t, ksh)], dtype=np.int64)
                e = int(np.searchsorted(his, s, side="right"))
                first = np.searchsorted(his, t["starts"], side="right")
                return ti, e, int(np.nonzero(t["starts"][first == e] == s)[0][0])
        raise AssertionError(i)

    def border_cuts(self, borders):
        """for every border offset: how many bytes of a record lie in front of it (0: it is a record's end; -1: inside the header)"""
        offs = self.walk(); out = []
        for b in borders:
            k = int(np.searchsorted(offs, b, side="right")) - 1
            out.append(-1 if b < self.first_rec else int(b - offs[k]) if b > offs[k] else 0)
        return out

    def tile_borders(self, tile_members):
        return [t["u_hi"] for t in self.tile_model(tile_members)[:-1]]

    def member_borders(self):
        return [lo for lo, _ in self.members()[1:]]


def entry_range(blocks, e, prefix, ksh, nm):
    """entry_range of csrc/common.h: entry 0 is the carried prefix; entry e >= 1 is piece (e - 1) & (2^ksh - 1) of member (e - 1) >> ksh, or (ksh < 0) the group
    of 2^-ksh members from member (e - 1) << -ksh on. blocks: (upos relative to the tile's first member, usize)."""
    if e == 0:
        return 0, prefix
    if ksh >= 0:
        idx = e - 1; upos, usize = blocks[idx >> ksh]; j = idx & ((1 << ksh) - 1)
        return prefix + upos + ((usize * j) >> ksh), prefix + upos + ((usize * (j + 1)) >> ksh)
    m0 = (e - 1) << -ksh; m1 = min(m0 + (1 << -ksh), nm) - 1
    return prefix + blocks[m0][0], prefix + blocks[m1][0] + blocks[m1][1]


# ---- the cases ----
def _aligned_members(s, counts, size, paired=True, head=100):
    """members of counts[k] records of `size` bytes each; the first member holds the header and `head` records in front"""
    s.fill(head, size, paired)
    cuts = []
    for n in counts:
        cuts.append(s.end()); s.fill(n, size, paired)
    return cuts


# records per member of the stride files: (stride - 1, stride, stride + 1, stride + 8) x 2^ksh for ksh = 0..3 - an aligned member of c << ksh records has c in every piece
STRIDE_COUNTS = sorted({(c + d) << k for k in range(4) for c in (K2_REL_STRIDE >> k,) for d in (-1, 0, 1, 8)})
STRIDE_TARGETS = {k: [(K2_REL_STRIDE >> k) + d for d in (-1, 0, 1, 8)] for k in range(4)}


def case_stride(size):
    n_full = MEMBER_MAX // size
    counts = STRIDE_COUNTS + [n_full, 505, 456, 496, 480, 448, 509, 519]   # (505, 456: a last group of one offset with 1 and 8 walkers; 496, 480, 448: full groups of eight below the stride with 2, 4, 8 walkers; 509, 519: pieces that begin inside a record at every ksh > 0)
    s = Stream(x_from=7000)
    cuts = _aligned_members(s, counts, size)
    prem = dict(members=len(counts) + 1, max_count={0: n_full}, include=STRIDE_TARGETS, mod8={0: [0, 1, 7]})
    exp = dict(path="aligned")
    return Case(f"stride{size}", s, cuts, aligned=True, premises=prem, expect=exp)


def case_deep(later):
    """the file's longest read (30 bases; a second one of 30 follows) and its first paired read deep in a member of 1400 records: record k >= stride of its entry at
    every ksh. later: two members of unpaired one-base records in front and NGSQC_TILE_MEMBERS=2, so the two lie in the second tile."""
    s = Stream(x_from=3500)
    cuts = []
    if later:
        s.fill(300, 44, paired=False); cuts.append(s.end())
        s.fill(300, 44, paired=False); cuts.append(s.end())
    s.fill(690, 44, paired=False)
    longest = s.add(l_seq=30, paired=False)
    s.fill(4, 44, paired=False)
    first_paired = len(s)
    while True:   # (the records behind it may be paired: the first whose flag says so)
        i = s.add(44, paired=True)
        if struct.unpack_from("<H", s.raw, s.offs[i] + 18)[0] & 1:
            first_paired = i; break
    s.fill(1400 - (len(s) - (600 if later else 0)) - 1, 44)
    s.add(l_seq=30)
    cuts.append(s.end()); s.fill(700, 44); cuts.append(s.end()); s.fill(500, 44)
    prem = dict(longest=longest, first_paired=first_paired, tile=1 if later else 0)
    return Case("deep_later" if later else "deep_first", s, cuts, layouts=((2, None),) if later else ((None, None),), aligned=True, premises=prem, expect=dict(path="aligned"))


def case_names(kind):
    """groups of four members (NGSQC_LONG_READ_MODE=1, NGSQC_GROUP_SHIFT=2) of 4092 / 4095 / 4096 records; "drop": NGSQC_TILE_MEMBERS=4, one group per tile - one
    that fits, three that exceed the names, two that fit again"""
    per = {"4092": [[1023] * 4] * 3, "4095": [[1024, 1024, 1024, 1023]] * 3, "4096": [[1024] * 4] * 3,
           "drop": [[1023] * 4] + [[1024] * 4] * 3 + [[1024, 1024, 1024, 1023], [1000] * 4]}[kind]
    s = Stream(x_from=20000)
    cuts = []
    for g in per:
        for n in g:
            if len(s):
                cuts.append(s.end())
            s.fill(n, 44)
    groups = [sum(g) for g in per]
    prem = dict(groups=groups)
    exp = dict(path="names", fits=max(groups) <= NAME_CAP, drop=kind == "drop")
    return Case(f"names{kind}", s, cuts, layouts=((4, None),) if kind == "drop" else ((None, None),), aligned=True, premises=prem, expect=exp)


CUT_AT = (1, 2, 3, 4, 20, 35, 36, 0)   # bytes of a record in front of a border (0: the border is the record's end)


def case_borders():
    """member borders after 1, 2, 3, 4, 20, 35, 36 bytes of a record and at a record's end, twice with one plain border between the two runs, so that with
    NGSQC_TILE_MEMBERS=2 each of them is a tile border once; then a record of 900 bytes cut every 100 bytes: it spans five tiles of two members"""
    s = Stream(x_from=400)
    cuts = []
    sizes = (44, 45, 60, 44, 51)
    def some(n):
        for k in range(n):
            s.add(sizes[(len(s) + k) % 5])
    some(7)
    for rep in range(2):
        for d in CUT_AT:
            some(5)
            i = s.add(sizes[len(s) % 5])
            cuts.append(s.offs[i] + d if d else s.end())
        some(4); cuts.append(s.end())
    some(3)
    i = s.add(l_seq=573)   # 4 + 32 + 2 + 4 + 287 + 573 = 902 bytes
    cuts += [s.offs[i] + 100 * k for k in range(1, 9)]
    some(9)
    cuts.append(s.end()); some(6)
    prem = dict(cut_at=sorted(CUT_AT), long_record=i, long_spans={1: 9, 2: 5})
    return Case("borders", s, cuts, layouts=((None, None), (1, None), (2, None)), premises=prem)


def case_degenerate():
    """empty members, members of 1, 2 and 3 bytes (one of them splits a block_size), a run of eleven such members inside one record - with NGSQC_TILE_MEMBERS=4 a tile
    that holds nothing else - and a last member of one byte: the last tile ends the last record and starts none"""
    s = Stream(x_from=300)
    cuts = []
    s.fill(10, 44); cuts.append(s.end()); s.fill(10, 44)
    cuts += [s.end(), s.end()]                      # an empty member between two records
    s.fill(10, 45)
    i = s.add(60); cuts += [s.offs[i] + 2, s.offs[i] + 3]   # a member of one byte inside block_size
    s.fill(5, 44)
    i = s.add(44); cuts += [s.offs[i] + 30, s.offs[i] + 30, s.offs[i] + 32]   # an empty member and one of two bytes inside a record
    s.fill(8, 51)
    i = s.add(45); cuts += [s.end(i - 1), s.offs[i] + 3]    # a member of three bytes: the first three bytes of block_size
    s.fill(6, 44)
    i = s.add(80)
    o = s.offs[i] + 10
    for n in (1, 2, 3, 0, 1, 1, 2, 3, 3, 0, 2, 1, 1):        # eleven tiny members (and two empty ones) inside record i
        cuts.append(o); o += n
    cuts.append(o)
    for _ in range(3):
        s.fill(10, 44); cuts.append(s.end())
    s.fill(25, 45)
    cuts.append(len(s.raw) - 1)                              # the stream's last byte alone
    prem = dict(tiny_run=11, empty=4)
    return Case("degenerate", s, cuts, layouts=((None, None), (1, None), (4, None)), premises=prem)


def case_header(mid):
    """a header of 1500 references (69 KB) in members of 20 000 bytes: with NGSQC_TILE_MEMBERS=1 the first four tiles hold header bytes alone. mid False: the
    header ends exactly at a member end; True: the first record starts 5000 bytes into a member"""
    refs = REFS + [(f"scaffold_{k:04d}", 1000 + k) for k in range(1498)]
    s = Stream(refs=refs, x_from=900)
    H = s.first_rec
    cuts = [20000, 40000, 60000]
    if not mid:
        cuts.append(H)
    s.fill(400, 44); s.fill(300, 45)
    if mid:
        assert H - 5000 > 60000
        cuts.append(H - 5000)
    cuts.append(s.end()); s.fill(500, 44)
    prem = dict(header=H, header_tiles=4)
    return Case("header_mid" if mid else "header_end", s, cuts, layouts=((None, None), (1, None)), premises=prem)


def case_entries(n_members, mixed):
    """n_members members of one record each in one tile (mixed: of one to three records)"""
    s = Stream(x_from=1 << 60)
    cuts = []
    for k in range(n_members):
        if k:
            cuts.append(s.end())
        s.fill(1 + (_mix(k) % 3 if mixed else 0), 44)
    prem = dict(entries=n_members + 1)
    return Case(f"entries{n_members}{'m' if mixed else ''}", s, cuts, aligned=True, premises=prem, expect=dict(path="aligned"))


def case_pieces():
    """520 members of 16 to 24 records: with NGSQC_WALKERS=8 their pieces are 4161 entries"""
    s = Stream(x_from=9000)
    cuts = []
    for k in range(520):
        if k:
            cuts.append(s.end())
        s.fill(16 + _mix(k) % 9, 44)
    return Case("pieces520", s, cuts, aligned=True, premises=dict(entries={3: 520 * 8 + 1}), expect=dict(path="aligned"))


CARRY_MAX = 4096


def case_carry(over):
    """NGSQC_CARRY_MAX=4096, NGSQC_TILE_MEMBERS=1: a record of 6008 bytes starts 4096 (over: 4097) bytes in front of a member border and ends in the next member"""
    s = Stream(x_from=500)
    s.fill(50, 44)
    i = s.add(l_seq=3977)   # 4 + 32 + 2 + 4 + 1989 + 3977 = 6008 bytes
    cuts = [s.offs[i] + CARRY_MAX + over]
    s.fill(60, 45)
    cuts.append(s.end()); s.fill(40, 44)
    prem = dict(carry=[CARRY_MAX + over, 0, 0])
    return Case("carry_over" if over else "carry_full", s, cuts, layouts=((1, CARRY_MAX),), premises=prem,
                refuses="larger than the carry area" if over else None)


BUILDERS = {
    "stride44": lambda: case_stride(44), "stride45": lambda: case_stride(45), "deep_first": lambda: case_deep(False), "deep_later": lambda: case_deep(True),
    "names4092": lambda: case_names("4092"), "names4095": lambda: case_names("4095"), "names4096": lambda: case_names("4096"), "namesdrop": lambda: case_names("drop"),
    "borders": case_borders, "degenerate": case_degenerate, "header_end": lambda: case_header(False), "header_mid": lambda: case_header(True),
    "entries4095": lambda: case_entries(4095, False), "entries4096": lambda: case_entries(4096, False), "entries4097": lambda: case_entries(4097, False),
    "entries4093m": lambda: case_entries(4093, True), "entries4094m": lambda: case_entries(4094, True), "pieces520": case_pieces,
    "carry_full": lambda: case_carry(0), "carry_over": lambda: case_carry(1),
}
ALL = list(BUILDERS)
ALIGNED = [n for n in ALL if n.startswith(("stride", "deep", "names", "entries", "pieces"))]   # cases 1, 2, 3 and 7
_BUILT = {}


def get(name):
    """the case `name`, built once"""
    if name not in _BUILT:
        _BUILT[name] = BUILDERS[name]()
    return _BUILT[name]
