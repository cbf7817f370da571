"""Designed reads for the first half of the depth path (csrc/scan.hip: the region search of classify<MODE_DEPTH> / MODE_COUNT / the fused WGS ROI pass, and the three
implementations of the min_baseq mask: baseq_decrements, the mask loop of scan_long_kernel, baseq_tile_kernel behind the riding list).

Every case is a list of advbam.Record on advbam.REFS in FILE ORDER, a list of regions (1-based closed, sorted, no overlap; touching allowed), the parameter sets
(min_mapq, min_baseq, skip_mismapped) it is run under, the BGZF member sizes of its file and a premise over the bookkeeping of tests/readdepth_model.py: what the case
is there for, asserted by tests/test_cpu_readdepth_model.py so that a later edit cannot hollow the case out. The expected values are the model's; nothing here knows them.

Qualities: LOW = 5 and two high values, 40 and 210 (a byte with bit 7 set: "not below" for every threshold up to 127 by another term of the byte trick, and what
lets a threshold above 127 - the byte-by-byte path - still tell high from low)."""
import random

import advbam as A
import cram_twin
import readdepth_model as RM

M, I, D, N, S, H, P, EQ, X = A.M, A.I, A.D, A.N, A.S, A.H, A.P, A.EQ, A.X
T1, TX, TY, TMT = A.T1, A.TX, A.TY, A.TMT
LOW, HIGH, HIGH7 = 5, 40, 210
WORD_EDGES = (64, 128, 192, 256)   # the edges of the four mask words of BQ_BITS = 256 read positions


def high(i):
    return HIGH7 if i & 1 else HIGH


def rec(name, pos, cigar, qual=None, flag=0, tid=T1, mapq=60, shapes=(), cg=None, seq=None):
    """pos: 0-based. qual None: every base HIGH"""
    l_seq = sum(ln for op, ln in (cg[1] if cg else cigar) if op in A.QUERY_OPS)
    if seq is None:
        seq = "ACGT"[len(name) % 4] * l_seq
    if qual is None:
        qual = [HIGH] * len(seq)
    return A.Record(name, flag, tid, pos, cigar, seq, mapq=mapq, qual=list(qual), cg=cg, shapes=shapes)


def key(r):
    return (r.tid if r.tid >= 0 else len(A.REFS), r.pos)


class Case:
    def __init__(self, name, records, regions, params, premise, member_sizes=(65280,), is_sorted=True):
        self.name, self.regions, self.params, self.premise, self.member_sizes = name, list(regions), list(params), premise, tuple(member_sizes)
        self.records = sorted(records, key=key) if is_sorted else list(records)   # (stable: the order given within a position)
        self.is_sorted = is_sorted
        for r in self.records:
            r.check()
        assert all(a[0] != b[0] or a[2] < b[1] for a, b in zip(self.regions, self.regions[1:])) and all(1 <= s <= e for _, s, e in self.regions)

    def subset(self, exclude=()):
        return [r for r in self.records if not (r.shapes & set(exclude))]

    def bed(self):
        return "".join("%s\t%d\t%d\n" % (A.REFS[t][0], s - 1, e) for t, s, e in self.regions)

    def write(self, path, member_sizes=None, exclude=(), whole_records=True):
        """the records in their order behind Catalogue.header(), in BGZF members of at most the given sizes. whole_records: as htslib writes - the header in a member
        of its own, every other member begins with a record and none is cut (what lets the depth scan ride the library's chain walk); otherwise the stream is cut
        wherever a size ends, as advbam.Catalogue.write does (the library's general path)"""
        recs = self.subset(exclude)
        sizes = member_sizes or self.member_sizes
        if whole_records:
            parts, cur = [A.Catalogue([]).header()], b""
            for r in recs:
                b = r.bytes()
                if cur and len(cur) + len(b) > sizes[(len(parts) - 1) % len(sizes)]:
                    parts.append(cur); cur = b""
                cur += b
            parts.append(cur)
        else:
            raw = A.Catalogue([]).header() + b"".join(r.bytes() for r in recs)
            parts, o = [], 0
            while o < len(raw):
                n = sizes[len(parts) % len(sizes)]
                parts.append(raw[o:o + n]); o += n
        open(path, "wb").write(b"".join(cram_twin._bgzf(p) for p in parts if p) + cram_twin._bgzf(b""))
        return recs

    def book(self, min_mapq=1, min_baseq=20, skip_mismapped=False, exclude=()):
        b = []
        RM.depth_from_reads(self.subset(exclude), self.regions, min_mapq, min_baseq, skip_mismapped, book=b)
        return b


def _ai(e):
    return {ai for _, _, ai in e.masked}


# ---- quality_values: every quality a byte can hold, next to every other, under every kind of threshold ----
THRESHOLDS = (1, 2, 20, 64, 126, 127, 128, 129, 200, 255, 256, 1000)


def quality_values():
    recs = []
    for k, t in enumerate(THRESHOLDS):
        p = 100 + 300 * k
        recs.append(rec("up%d" % t, p, [(M, 256)], qual=list(range(256))))
        recs.append(rec("down%d" % t, p + 7, [(M, 256)], qual=list(range(255, -1, -1))))
        recs.append(rec("alt%d" % t, p + 13, [(M, 256)], qual=[min(t - 1 + (i & 1), 255) for i in range(256)]))
    regions = [(T1, 1, 4000)]

    def premise(case):
        for t in THRESHOLDS:
            book = case.book(min_baseq=t)
            for e in book:
                r = case.records[e.k]
                want = {i for i in range(256) if r.qual[i] < t}
                assert _ai(e) == want and len(e.masked) == len(want), (t, r.name)
                if r.name.startswith("up") and t <= 255:      # the mask ends exactly between quality t - 1 and quality t
                    assert t - 1 in want and t not in want
                if r.name == "alt%d" % t and t <= 255:
                    assert want == set(range(0, 256, 2))
        assert {q for r in case.records for q in r.qual} == set(range(256))
    return Case("quality_values", recs, regions, [(1, t, False) for t in THRESHOLDS], premise)


# ---- word_edges: read lengths and low qualities on both sides of every edge of the four mask words, and the byte tail behind them ----
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 600, 1500)
EDGE_POS = (0,) + tuple(range(62, 66)) + tuple(range(126, 130)) + tuple(range(190, 194)) + tuple(range(254, 258))


def _edge_set(length):
    return {x for x in EDGE_POS + (length - 1,) if x < length}


def word_edges():
    recs = []
    for length in LENGTHS:
        lo = _edge_set(length)
        recs.append(rec("edge%d" % length, 100, [(M, length)], qual=[LOW if i in lo else high(i) for i in range(length)]))
        recs.append(rec("comp%d" % length, 2000, [(M, length)], qual=[high(i) if i in lo else LOW for i in range(length)]))
    regions = [(T1, 1, 5000)]

    def premise(case):
        for t in (20,):
            book = case.book(min_baseq=t)
            for e in book:
                r = case.records[e.k]
                length = len(r.seq)
                lo = _edge_set(length)
                assert _ai(e) == (lo if r.name.startswith("edge") else set(range(length)) - lo), (t, r.name)
            both = set()
            for e in book:
                for w in WORD_EDGES:
                    if w - 1 in _ai(e) and w in _ai(e):
                        both.add(w)
            assert both == set(WORD_EDGES)
            assert any(max(_ai(e), default=0) >= 256 for e in book)                     # the byte tail behind BQ_BITS
        assert max(len(r.cigar) for r in case.records) <= RM.LONG_CIGAR and all(e.listed for e in case.book())
    return Case("word_edges", recs, regions, [(1, t, False) for t in (6, 20, 41, 127, 128, 200, 211)], premise)


# ---- region_cuts: region edges at every read position around the word edges ----
CUT_P = 5000   # 0-based position of every read: read position x lies at the 1-based position CUT_P + 1 + x
CUT_LEN = 300
# regions in read positions, [a_lo, a_hi): a_lo and a_hi each take every value of 63..65, 127..129, 191..193, 255..257
CUT_RANGES = ([(-50, 1), (10, 63), (63, 64), (64, 65), (65, 100)] + [(100, 127), (127, 128), (128, 129), (129, 150)]
              + [(160, 191), (191, 192), (192, 193), (193, 200)] + [(210, 255), (255, 256), (256, 257), (257, 280), (299, 350)])
CUT_VALUES = [w + d for w in WORD_EDGES for d in (-1, 0, 1)]


def region_cuts():
    regions = [(T1, CUT_P + 1 + a, CUT_P + b) for a, b in CUT_RANGES]
    firsts_lasts = {x for a, b in CUT_RANGES for x in (a, b - 1) if 0 <= x < CUT_LEN}
    rng = random.Random(11)
    recs = [rec("ends", CUT_P, [(M, CUT_LEN)], qual=[LOW if i in firsts_lasts else high(i) for i in range(CUT_LEN)]),
            rec("inner", CUT_P, [(M, CUT_LEN)], qual=[high(i) if i in firsts_lasts else LOW for i in range(CUT_LEN)]),
            rec("all", CUT_P, [(M, CUT_LEN)], qual=[LOW] * CUT_LEN)]
    for k in range(200):
        recs.append(rec("r%d" % k, CUT_P, [(M, CUT_LEN)], qual=[rng.choice((LOW, LOW, HIGH, HIGH7, 19, 20, 127, 128, 255)) for _ in range(CUT_LEN)]))

    def premise(case):
        book = case.book(min_baseq=20)
        e = book[0]
        assert case.records[0].name == "ends" and len(e.regions) == len(case.regions) >= 6
        cuts = [(max(e.start1, s) - e.start1, min(e.end1, en) - e.start1 + 1) for _, s, en in case.regions]
        assert set(CUT_VALUES) <= {a for a, _ in cuts} and set(CUT_VALUES) <= {b for _, b in cuts}
        assert (1, 1) in [(b - a, b) for a, b in cuts] and (CUT_LEN - 1, CUT_LEN) in cuts           # ends on the read's first base, starts on its last
        assert sum(1 for a, b in zip(case.regions, case.regions[1:]) if a[2] + 1 == b[1]) >= 8     # touching regions
        assert sum(1 for _, s, en in case.regions if s == en) >= 8                                  # one-base regions
        for i, (_, s, en) in enumerate(case.regions):                                               # a masked base on the first and on the last slot of every region
            hit = {p for j, p, _ in e.masked if j == i}
            assert max(s, e.start1) in hit and min(en, e.end1) in hit, i
    return Case("region_cuts", recs, regions, [(1, t, False) for t in (20, 127, 200)], premise)


# ---- cigar_shapes ----
def _n_ops(n):
    """n operations: M / I / M / D in turn, an M at the end"""
    body = [(M, 3), (I, 1), (M, 2), (D, 2)]
    return [body[k % 4] for k in range(n - 1)] + [(M, 4)]


CG_OPS = [(S, 2), (M, 30), (I, 2), (M, 16), (D, 3), (M, 40), (N, 20), (M, 25)]
SHAPES = [("ops1", [(M, 100)]), ("ops2", [(S, 10), (M, 90)]), ("ops3", [(M, 50), (I, 5), (M, 45)]), ("ops4", [(S, 5), (M, 40), (D, 10), (M, 55)]),
          ("ops5", [(S, 5), (M, 30), (I, 2), (D, 3), (M, 63)]), ("ops64", _n_ops(64)), ("ops65", _n_ops(65)),
          ("leadS", [(S, 7), (M, 100)]), ("leadI", [(I, 4), (M, 100)]), ("delFront", [(M, 20), (D, 60), (M, 100)]), ("skipFront", [(M, 20), (N, 70), (M, 80)]),
          ("eqx", [(EQ, 30), (X, 2), (M, 68)]), ("hp", [(H, 5), (M, 40), (P, 2), (M, 60), (H, 3)]),
          ("zero", [(M, 0), (S, 0), (M, 50), (I, 0), (D, 0), (M, 50), (N, 0)]), ("insEdge", [(M, 10), (I, 5), (M, 90)])]
SHAPE_REGIONS = [(T1, 900, 960), (T1, 1000, 1200), (T1, 1201, 1230), (T1, 1300, 1400), (T1, 1500, 1500)]
SHAPE_STARTS = (989, 940, 1130, 1290, 1420)   # 0-based; insEdge at 989: its I lies directly in front of the region start 1000


def cigar_shapes():
    rng = random.Random(5)

    def quals(n):
        return [rng.choice((3, 19, 20, 21, HIGH, 127, 128, 200, 255)) for _ in range(n)]
    recs = []
    for p in SHAPE_STARTS:
        for name, ops in SHAPES:
            lq = sum(ln for op, ln in ops if op in A.QUERY_OPS)
            recs.append(rec("%s@%d" % (name, p), p, ops, qual=quals(lq), shapes={name}))
        cg_l = sum(ln for op, ln in CG_OPS if op in A.QUERY_OPS); cg_r = sum(ln for op, ln in CG_OPS if op in A.REF_OPS)
        recs.append(rec("cg@%d" % p, p, [(S, cg_l), (N, cg_r)], qual=quals(cg_l), cg=(A._cg(CG_OPS), CG_OPS), shapes={"cg"}))
        recs.append(rec("seqStar@%d" % p, p, [(M, 100)], seq="", qual=[], shapes={"seq_star"}))

    def premise(case):
        book = case.book(min_baseq=20)
        by = {}
        for e in book:
            by.setdefault(next(iter(case.records[e.k].shapes)), []).append(e)
        for name in ("ops64", "ops65", "cg") + tuple(n for n, _ in SHAPES):      # every shape overlaps a region with masked bases
            assert any(e.masked for e in by[name]), name
        assert all(e.listed for e in by["ops64"]) and all(e.wave_path for e in by["ops65"] + by["cg"])
        assert [len(o) for n, o in SHAPES[:7]] == [1, 2, 3, 4, 5, 64, 65]
        assert all(e.regions and not e.masked for e in by["seq_star"])           # the clamp: counted, nothing masked
        # the '=' / 'X' quirk moves the mask: the M of "eqx" tests read positions 0.. (not 32..)
        assert any(ai < 32 for e in by["eqx"] for ai in _ai(e))
    params = [(1, t, False) for t in (1, 20, 128, 201)]
    return Case("cigar_shapes", recs, SHAPE_REGIONS, params, premise)


# ---- pile, spill, no_spill ----
def pile():
    q = [HIGH] * 150; q[10] = q[149] = LOW
    recs = [rec("p%d" % k, 500, [(M, 150)], qual=q) for k in range(300)]

    def premise(case):
        book = case.book(min_baseq=20)
        assert len(book) == 300 and all(_ai(e) == {10, 149} for e in book) and len(RM.chunks(book)) == 2
    return Case("pile", recs, [(T1, 400, 700)], [(1, 20, False), (1, 200, False)], premise)


def _row(step_of):
    rng = random.Random(3)
    return [rec("s%d" % k, step_of(k), [(M, 150)], qual=[LOW if rng.random() < 0.1 else high(i) for i in range(150)]) for k in range(600)]


def spill():
    """600 reads of 150 bases over one region of 30 000 bases, neighbouring starts 100 bases apart (chr1 has room for 298 starts: two or three reads share a start)"""
    recs = _row(lambda k: 100 * (k * 298 // 600))

    def premise(case):
        book = case.book(min_baseq=20)
        ch = RM.chunks(book)
        assert len(ch) == 3 and all(RM.chunk_reach(c, case.regions) >= RM.BQ_TILE for c in ch)
        starts = sorted({r.pos for r in case.records})
        assert all(b - a == 100 for a, b in zip(starts, starts[1:]))
    return Case("spill", recs, [(T1, 1, 30000)], [(1, 20, False), (1, 200, False)], premise)


def no_spill():
    recs = _row(lambda k: 5 * k)

    def premise(case):
        book = case.book(min_baseq=20)
        ch = RM.chunks(book)
        assert len(ch) == 3 and all(0 <= RM.chunk_reach(c, case.regions) < RM.BQ_TILE for c in ch)
    return Case("no_spill", recs, [(T1, 1, 30000)], [(1, 20, False), (1, 200, False)], premise)


# ---- sparse_appends: which lanes of a walking wave append, trip by trip ----
PERIODS = {1: 128, 2: 128, 63: 260, 64: 260, 65: 260}   # period -> records of its stretch
SPARSE_LEN, SPARSE_STEP = 20, 22


def sparse_appends():
    """per period p a stretch of records, 22 bases apart, of which every p-th lies on a region of its own (inside its span, out of its neighbours' reach) and passes;
    of the others every second one passes and meets no region, the rest fail a filter. Members of a few hundred bytes: a walker (a lane) has a handful of records,
    so the ballots of a wave's trips take every shape and the blocks of the list end in holes"""
    recs, regions = [], []
    rng = random.Random(17)
    x = 1000
    for p, n in PERIODS.items():
        for k in range(n):
            q = [LOW if rng.random() < 0.3 else high(i) for i in range(SPARSE_LEN)]
            q[6] = LOW
            if k % p == 0:
                recs.append(rec("a%d_%d" % (p, k), x, [(M, SPARSE_LEN)], qual=q))
                regions.append((T1, x + 5, x + 12))
            elif k % 2 == 0:
                recs.append(rec("n%d_%d" % (p, k), x, [(M, SPARSE_LEN)], qual=q))
            else:
                recs.append(rec("f%d_%d" % (p, k), x, [(M, SPARSE_LEN)], qual=q, flag=(0x400, 0x100, 0x800, 0x4)[(k // 2) % 4]))
            x += SPARSE_STEP

    def premise(case):
        book = case.book(min_baseq=20)
        o = 0
        for p, n in PERIODS.items():                                            # in file order: p - 1 records that do not append between two that do
            flags = "".join("x" if e.listed else "-" for e in book[o:o + n]); o += n
            assert flags.count("x") == (n + p - 1) // p and {len(g) for g in flags.split("x")[1:-1]} == ({p - 1} if flags.count("x") > 1 else set()), (p, flags)
        assert all(len(e.regions) == 1 and e.masked for e in book if e.listed)
        assert any(e.passed and not e.regions for e in book) and any(not e.passed for e in book)
        assert sum(e.listed for e in book) % RM.BQ_BLOCK != 0
    return Case("sparse_appends", recs, regions, [(1, 20, False), (1, 200, False)], premise, member_sizes=(300, 517, 1100, 409))


# ---- cache_moves: the per-lane cache of the region search must refresh, and must not ----
CACHE_REGIONS = [(T1, 1000, 1100), (T1, 1101, 1200), (T1, 2000, 2100), (T1, 5000, 5050), (TY, 100, 200), (TY, 1000, 1100), (TMT, 150, 160)]


def _cache_records():
    rng = random.Random(23)
    recs, k = [], 0
    for tid in (T1, TX, TY, TMT):                      # chrX has no region: between two references that have
        mine = [r for r in CACHE_REGIONS if r[0] == tid] or [(tid, 500, 600)]
        starts1 = [10, 400, mine[-1][2] + 300, A.REFS[tid][1] - 60]                                 # before the first region, behind the last
        for _, s, e in mine:
            starts1 += [s - 50, s - 49, s - 1, s, s + 1, e - 1, e, e + 1, e + 2]                     # a span that ends on s - 1 / on s; a start on e / on e + 1
        starts1 += [rng.randrange(1, A.REFS[tid][1] - 60) for _ in range(60)]
        for s1 in starts1:
            if 1 <= s1 <= A.REFS[tid][1] - 50:
                q = [LOW if rng.random() < 0.15 else high(i) for i in range(50)]
                recs.append(rec("c%d" % k, s1 - 1, [(M, 50)], qual=q, tid=tid)); k += 1
    return recs


def _cache_premise(case):
    book = case.book(min_baseq=20)
    st = {(case.records[e.k].tid, e.start1) for e in book if e.passed}
    for t, s, e in CACHE_REGIONS:
        assert {(t, e), (t, e + 1), (t, s - 50), (t, s - 49)} <= st
    assert any(case.records[e.k].tid == TX for e in book) and not any(e.regions for e in book if case.records[e.k].tid == TX)
    assert sum(bool(e.masked) for e in book) > 30
    keys = [key(r) for r in case.records]
    back = sum(b < a for a, b in zip(keys, keys[1:]))
    tid_back = sum(b[0] < a[0] for a, b in zip(keys, keys[1:]))
    assert (back == 0) if case.is_sorted else (back > 50 and tid_back > 10)   # the unsorted file really goes backwards, references included


def cache_moves():
    return Case("cache_moves", _cache_records(), CACHE_REGIONS, [(1, 20, False), (1, 0, False)], _cache_premise)


def cache_moves_unsorted():
    recs = _cache_records()
    random.Random(29).shuffle(recs)
    return Case("cache_moves_unsorted", recs, CACHE_REGIONS, [(1, 20, False), (1, 0, False)], _cache_premise, is_sorted=False)


# ---- filters ----
def filters():
    recs = []
    q = [LOW if i % 7 == 0 else high(i) for i in range(40)]
    for b in range(12):
        recs.append(rec("flag%x" % (1 << b), 1000 + b, [(M, 40)], qual=q, flag=1 << b))
    for mq in (0, 1, 19, 20):
        recs.append(rec("proper%d" % mq, 1020 + mq, [(M, 40)], qual=q, flag=0x1 | 0x2 | 0x40, mapq=mq))
        recs.append(rec("notProper%d" % mq, 1021 + mq, [(M, 40)], qual=q, flag=0x1 | 0x40, mapq=mq))
    recs.append(rec("noRef", 1000, [(M, 40)], qual=q, tid=-1))
    for k in range(60):                                     # plain reads that pass everything: depth under the others, and a file of more than one small tile
        recs.append(rec("plain%d" % k, 985 + k, [(M, 40)], qual=q, flag=0x1 | 0x2 | 0x40))

    def premise(case):
        def passed(**kw):
            return {case.records[e.k].name for e in case.book(**kw) if e.passed}
        everything = {r.name for r in case.records}
        assert sum(len(r.bytes()) for r in case.records) > 8000
        assert everything - passed(min_mapq=0) == {"flag4", "flag100", "flag400", "flag800", "noRef"}
        assert passed(min_mapq=0) - passed(min_mapq=1) == {"proper0", "notProper0"}
        assert passed(min_mapq=1) - passed(min_mapq=20) == {"proper1", "notProper1", "proper19", "notProper19"}
        assert passed(min_mapq=0) - passed(min_mapq=0, skip_mismapped=True) == {"notProper0", "notProper1", "notProper19"}
        assert "notProper20" in passed(min_mapq=20, skip_mismapped=True)
    params = [(mq, bq, skip) for mq in (0, 1, 20) for bq in (0, 20) for skip in (False, True)]
    return Case("filters", recs, [(T1, 990, 1030), (T1, 1031, 1100)], params, premise)


BUILDERS = (quality_values, word_edges, region_cuts, cigar_shapes, pile, spill, no_spill, sparse_appends, cache_moves, cache_moves_unsorted, filters)
NAMES = tuple(b.__name__ for b in BUILDERS)
_made = {}


def case(name):
    """made once and shared: nobody writes to a case"""
    if name not in _made:
        _made[name] = BUILDERS[NAMES.index(name)]()
    return _made[name]
