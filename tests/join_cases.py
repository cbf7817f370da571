"""Designed inputs for the mate join (csrc/join.h NameJoin over csrc/join_visit.h): named cases, each the records in file order, the tile every record lies in
(one BGZF member per tile: run with NGSQC_TILE_MEMBERS=1) and its premises as assertions. tests/test_cpu_join_designed.py runs them through the CPU build of
the join's own text, tests/test_gpu_join_designed.py through BamFilter, BamToFastq and BamDownsample on the device; the expectations are the oracles'.

name_hash / name_hash_mask restate csrc/join_visit.h (FNV-1a, then the splitmix64 finaliser); PINNED holds values the CPU build printed. With them a case
searches names that collide under NGSQC_NAME_HASH_BITS 2 and 4 and asserts that they do."""
import struct

import cram_twin
from bamfilter_oracle import Rec, written

M64 = (1 << 64) - 1
PIECE = 0xff00
F1, F2 = 0x41, 0x81   # paired, read 1 / read 2

TEXT = "@HD\tVN:1.6\n@SQ\tSN:c1\tLN:1000000\n@SQ\tSN:c2\tLN:1000000\n"
REFS = [("c1", 1000000), ("c2", 1000000)]


def header():
    h = b"BAM\1" + struct.pack("<i", len(TEXT)) + TEXT.encode() + struct.pack("<i", len(REFS))
    for nm, ln in REFS:
        h += struct.pack("<i", len(nm) + 1) + nm.encode() + b"\0" + struct.pack("<i", ln)
    return h


def name_hash(name):
    h = 0xcbf29ce484222325
    for c in name:
        h = ((h ^ c) * 0x100000001b3) & M64
    h ^= h >> 30; h = (h * 0xbf58476d1ce4e5b9) & M64
    h ^= h >> 27; h = (h * 0x94d049bb133111eb) & M64
    return h ^ (h >> 31)


def name_hash_mask(bits):
    return M64 >> 1 if bits >= 63 else (1 << bits) - 1


# name_hash as tests/emul/join_emul.cpp (join_name_hash) printed it: test_cpu_join_designed.py compares all three
PINNED = {b"": 0xf52a15e9a9b5e89b, b"ab": 0x9ffe50a657e4a147, b"r1": 0x15d7ff2b76197532, b"q17:4711": 0xc485a2fe421a7fe4, b"x" * 254: 0x21f19cca9f29a434}


def collide(a, b, bits=4):
    return (name_hash(a) ^ name_hash(b)) & name_hash_mask(bits) == 0


def rec(field, flag, l_seq=8, mapq=60, tid=0, pos=100, cigar=None, seq=None, qual=None, aux=b"", size=None):
    """a BAM record (block_size included). field: the name field as it lies in the record (str: the name, one NUL added; bytes: taken as they are).
    size: the record's whole size, reached by a padding Z tag"""
    n = field.encode() + b"\0" if isinstance(field, str) else field
    assert 1 <= len(n) <= 255
    cig = cigar if cigar is not None else ([l_seq << 4] if l_seq else [])
    seq = seq if seq is not None else bytes((0x12, 0x48)[i & 1] for i in range((l_seq + 1) // 2))
    qual = qual if qual is not None else bytes(30 + i % 10 for i in range(l_seq))
    assert len(seq) == (l_seq + 1) // 2 and len(qual) == l_seq

    def build(aux):
        body = struct.pack("<iiBBHHHiiii", tid, pos, len(n), mapq, 4680, len(cig), flag, l_seq, tid, pos + 100, 0) + n
        body += struct.pack(f"<{len(cig)}I", *cig) + seq + qual + aux
        return struct.pack("<I", len(body)) + body
    b = build(aux)
    if size is not None:
        k = size - len(b) - 4
        assert k >= 0, (size, len(b))
        b = build(aux + b"XPZ" + b"p" * k + b"\0")
        assert len(b) == size
    return b


class Case:
    def __init__(self, name, tiles, **notes):
        self.name, self.tiles, self.notes = name, tiles, notes

    @property
    def records(self):
        return [b for t in self.tiles for b in t]

    @property
    def tile_of(self):
        return [i for i, t in enumerate(self.tiles) for _ in t]

    def bam(self):
        """the file: the header in a member of its own, then every tile's bytes in members of their own (a tile longer than a member continues in members that
        hold no record start), then the EOF member"""
        out = cram_twin._bgzf(header())
        for t in self.tiles:
            raw = b"".join(t)
            for o in range(0, max(len(raw), 1), 60000):
                out += cram_twin._bgzf(raw[o:o + 60000])
        return out + cram_twin._bgzf(b"")

    def write(self, path):
        open(path, "wb").write(self.bam())
        return path


def takes_part(r, tool):
    """the record reaches the tool's mate cache (BamFilter: every primary record; BamDownsample and BamToFastq: the paired ones)"""
    return not r.flag & 0x900 and (tool == "filter" or bool(r.flag & 1))


def model(case, tool="filter"):
    """the reference's cache over the case, record by record: ([(opener index, closer index)], open indices at the end, H behind every tile, the largest
    cache size). Names by Rec.name."""
    cache, pairs, hs, peak, i = {}, [], [], 0, 0
    for t in case.tiles:
        for b in t:
            r = Rec(b)
            if takes_part(r, tool):
                if r.name in cache:
                    pairs.append((cache.pop(r.name), i))
                else:
                    cache[r.name] = i
                peak = max(peak, len(cache))
            i += 1
        hs.append(len(cache))
    return pairs, sorted(cache.values()), hs, peak


def _search(fmt, n, bits=4, start=0):
    """n names fmt % k, k >= start, whose hashes agree in their low bits"""
    want, out, k = None, [], start
    while len(out) < n:
        nm = fmt % k
        h = name_hash(nm) & name_hash_mask(bits)
        if want is None:
            want = h
        if h == want:
            out.append(nm)
        k += 1
        assert k < start + 100000
    return out


def run_lengths():
    """one name 1..7 times inside one tile, then spread over tiles; pairs are (1st, 2nd), (3rd, 4th), ..., an odd last record stays open"""
    tiles = [[] for _ in range(5)]
    for k in range(1, 8):
        tiles[0] += [rec("in%d" % k, F1 if c % 2 == 0 else F2, pos=100 + c) for c in range(k)]
    layouts = [(1, 0, 2, 2), (1, 1, 1), (3, 0, 0, 1), (2, 1, 0, 3), (0, 4, 3), (1, 2), (1, 0, 0, 0, 1), (2, 2, 2), (1, 6), (5, 1, 1)]
    for i, lay in enumerate(layouts):
        c = 0
        for t, k in enumerate(lay):
            for _ in range(k):
                tiles[t].append(rec("sp%d" % i, F1 if c % 2 == 0 else F2, pos=200 + c)); c += 1
    case = Case("run_lengths", tiles, layouts=layouts)
    pairs, still, hs, _ = model(case)
    recs = [Rec(b) for b in case.records]
    by_name = {}
    for i, r in enumerate(recs):
        by_name.setdefault(r.name, []).append(i)
    exp = sorted((v[k], v[k + 1]) for v in by_name.values() for k in range(0, len(v) - 1, 2))
    assert sorted(pairs) == exp and still == sorted(v[-1] for v in by_name.values() if len(v) & 1)
    assert sorted(len(v) for v in by_name.values())[-1] == 7 and {len(by_name[b"in%d" % k]) for k in range(1, 8)} == set(range(1, 8))
    assert any(hs[t] > hs[t + 1] for t in range(4)) and hs[0] > 0
    return case


def held_chain():
    """openers whose mates come 1, 2, 3 and 5 tiles later while other names open and close around them: H = 0 in front, then 8, 3, 8, 2, 5, 0 behind the
    tiles. "d3" does not pass BamFilter's defaults (MAPQ 10): it is held as its fixed part and name alone; the others are held whole. "far" is still
    compared in tile 5 when its own tile's buffer has been reused five times."""
    T = [[] for _ in range(6)]
    T[0] += [rec("far", F1, l_seq=40), rec("d3", F1, mapq=10, l_seq=33), rec("d1", F2), rec("d2", F1, l_seq=21)] + [rec("a%d" % k, F1) for k in range(4)]
    T[1] += [rec("d1", F1)] + [rec("a%d" % k, F2) for k in range(4)]
    T[2] += [rec("d2", F2)] + [rec("b%d" % k, F1, l_seq=k) for k in range(6)]
    T[3] += [rec("d3", F2)] + [rec("b%d" % k, F2) for k in range(6)] + [rec("e5", F2, mapq=10)]
    T[4] += [rec("c%d" % k, F1, mapq=(10 if k == 1 else 60)) for k in range(3)]
    T[5] += [rec("c%d" % k, F2) for k in range(3)] + [rec("far", F2), rec("e5", F1)]
    case = Case("held_chain", T)
    pairs, still, hs, peak = model(case)
    assert hs == [8, 3, 8, 2, 5, 0] and not still and peak == 8
    gaps = {Rec(case.records[o]).name: case.tile_of[c] - case.tile_of[o] for o, c in pairs}
    assert (gaps[b"d1"], gaps[b"d2"], gaps[b"d3"], gaps[b"far"]) == (1, 2, 3, 5)
    return case


def empty_tile():
    """a record of about 70 KB runs over two members: the second holds no record start (a tile with n == 0) while three names are open; the long record's
    mate and one of the open names close right behind it"""
    big = rec("big", F1, l_seq=46000, seq=bytes(23000), cigar=[46000 << 4])
    T = [[rec("o1", F1), rec("o2", F1, mapq=10), rec("o3", F2)], [big], [rec("big", F2), rec("o1", F2), rec("o2", F2)], [rec("o3", F1)]]
    case = Case("empty_tile", T, members_of_tile=[1, 2, 1, 1])
    assert 60000 < len(big) < 120000 and len(b"".join(T[1])[60000:]) > 0   # (the second member of tile 1 is the long record's tail alone)
    pairs, still, hs, _ = model(case)
    assert hs == [3, 4, 1, 0] and not still and len(pairs) == 4
    return case


def _colliding_pairs():
    """[(A, B)] whose hashes agree in their low 4 bits (so under 2 and 4 bits): different in the last byte alone, in length alone (r1 / r10), behind byte 200
    of 254 alone"""
    out = []
    k = 0
    while len(out) < 2:
        a, b = b"lb%da" % k, b"lb%db" % k
        if collide(a, b): out.append((a, b))
        k += 1
    k = 0
    while len(out) < 3:
        a, b = b"r%d" % k, b"r%d0" % k
        if collide(a, b): out.append((a, b))
        k += 1
    k = 0
    while len(out) < 5:
        a, b = b"L" * 200 + b"%054d" % k, b"L" * 200 + b"%054d" % (k + 100000)
        if collide(a, b): out.append((a, b))
        k += 1
    return out


def collisions():
    """runs of one hash (under 2 and 4 bits) that hold two names: A B A B, A B B A, A A B inside a tile, and held-A held-B in front of B A"""
    P = _colliding_pairs()
    f = lambda nm, fl, **kw: rec(nm + b"\0", fl, **kw)
    T = [[], []]
    (a, b) = P[0]; T[0] += [f(a, F1), f(b, F1), f(a, F2), f(b, F2)]
    (a, b) = P[1]; T[0] += [f(a, F1), f(b, F2), f(b, F1), f(a, F2)]
    (a, b) = P[2]; T[0] += [f(a, F1), f(a, F2), f(b, F1)]; T[1] += [f(b, F2, mapq=10)]
    (a, b) = P[3]; T[0] += [f(a, F1), f(b, F1), f(a, F2), f(b, F2)]
    (a, b) = P[4]; T[0] += [f(a, F1, mapq=10), f(b, F2)]; T[1] += [f(b, F1), f(a, F2)]
    # a run of 3 to 7 of one name that starts with a held entry, among held entries of other names of its hash
    names = _search(b"mix%d", 3)
    T[0] += [f(names[0], F1), f(names[1], F1), f(names[2], F1)]
    T[1] += [f(names[1], F2)] + [f(names[0], F2 if c % 2 == 0 else F1, pos=300 + c) for c in range(6)]
    case = Case("collisions", T, pairs_of_names=P, mixed=names)
    for a, b in P:
        assert a != b and collide(a, b, 4) and collide(a, b, 2)
    assert P[2][1] == P[2][0] + b"0" and len(P[3][0]) == 254 and P[3][0][:200] == P[3][1][:200] and P[0][0][:-1] == P[0][1][:-1]
    assert all(collide(names[0], n) for n in names)
    pairs, still, hs, _ = model(case)
    assert len(pairs) == 14 and len(still) == 2 and hs[0] == 6
    return case


def no_part():
    """0x100 / 0x800 records and unpaired records that carry open names, between opener and closer, in the tile and a tile later: BamDownsample and BamToFastq
    keep them out of the cache, BamFilter takes the unpaired ones in"""
    T = [[rec("n1", F1), rec("n1", F1 | 0x100), rec("n1", 0x800 | F2), rec("n1", 0), rec("n2", F1), rec("n2", 0x10), rec("n1", F2), rec("n3", F2)],
         [rec("n2", 0x100), rec("n3", 0x800 | F1), rec("n3", 0), rec("n2", F2), rec("n3", F1), rec("n4", 0x900 | F1), rec("n4", F2)]]
    case = Case("no_part", T)
    pf, sf, _, _ = model(case, "filter")
    pd, sd, _, _ = model(case, "downsample")
    assert pf != pd and len(pd) == 3 and len(sd) == 1 and len(pf) == 3 and len(sf) == 4
    return case


def c_string_names():
    """name fields that hold more than one NUL: the name is what lies in front of the first (BamAlignment::name); the empty name (l_read_name 1) twice; a name
    of 254 bytes"""
    long_name = bytes(65 + k % 26 for k in range(254))
    T = [[rec(b"ab\0", F1), rec(b"ab\0\0\0", F2), rec(b"cd\0ef\0", F1), rec(b"\0", F1), rec(long_name + b"\0", F1), rec(b"gh\0\0", F1, mapq=10), rec(b"ij\0xy\0", F1)],
         [rec(b"cd\0", F2), rec(b"\0", F2), rec(long_name + b"\0", F2), rec(b"gh\0zzzz\0", F2), rec(b"ij\0", F2), rec(b"ij\0xy\0", F1), rec(b"ij\0uv\0", F2)]]
    case = Case("c_string_names", T)
    recs = [Rec(b) for b in case.records]
    fields = [r.b[36:36 + r.l_name] for r in recs]
    pairs, still, _, _ = model(case)
    assert len(pairs) == 7 and not still
    assert sum(fields[o] != fields[c] for o, c in pairs) == 5   # (on the whole fields these would be different names: five pairs would stay open)
    assert all(recs[o].name == recs[c].name for o, c in pairs) and {recs[o].name for o, _ in pairs} == {b"ab", b"cd", b"", long_name, b"gh", b"ij"}
    return case


def _cg_record(name, flag, n_ops, pos=500, n_len=None):
    """a record whose CIGAR of n_ops operations lies in its CG tag (1M 1I alternating, l_seq = n_ops); n_len: the N of the placeholder, if not the real span"""
    ops = [(1 << 4) | (0 if k % 2 == 0 else 1) for k in range(n_ops)]
    l_seq = n_ops
    rlen = (n_ops + 1) // 2
    aux = b"NMC\0" + b"CGBI" + struct.pack("<I", n_ops) + struct.pack(f"<{n_ops}I", *ops) + b"RGZg\0"
    return rec(name, flag, l_seq=l_seq, pos=pos, cigar=[l_seq << 4 | 4, (n_len or rlen) << 4 | 3], aux=aux)


def window_cuts_bam():
    """NGSQC_WRITE_WINDOW_PIECES=1: filler pairs bring a multiple of 0xff00 of the output stream to a chosen offset of a probe pair (cut = the bytes of the
    pair in front of the window end). All-pass parameters with max_gap = -1 and max_mm = -1: every pair is written."""
    recs, cuts, stream = [], [], 0
    probes = []
    plain = lambda k: (rec("probe%d" % k, F1, l_seq=31), rec("probe%d" % k, F2, l_seq=30))
    o_size = len(plain(0)[0])
    for k, cut in enumerate([o_size, o_size + 1, o_size + 2, o_size + 3, o_size + 19, o_size + 36 + 3, 19, 36 + 2]):
        probes.append((plain(k), cut, "plain"))
    cg300 = lambda k: (_cg_record("cga%d" % k, F1, 300), rec("cga%d" % k, F2))
    w300 = written(Rec(cg300(0)[0]))
    for k, cut in enumerate([16, 17, 36 + 5 + 4 * 150 + 2, len(w300) - 3]):
        probes.append((cg300(k), cut, "cg300"))
    big = lambda k: (_cg_record("cgb%d" % k, F1, 65536), rec("cgb%d" % k, F2))
    wbig = written(Rec(big(0)[0]))
    tag_at = len(wbig) - (8 + 4 * 65536)
    for k, cut in enumerate([15, 36 + 5 + 2, 36 + 5 + 6, tag_at + 3, tag_at + 6, tag_at + 8 + 4 * 30000 + 1]):
        probes.append((big(k), cut, "cg65536"))
    for i, (pair, cut, kind) in enumerate(probes):
        # filler pair(s) so that (stream + filler + cut) is a multiple of the piece
        need = (-(stream + cut)) % PIECE
        while need < 200:
            need += PIECE
        half = need // 2
        fill = [rec("fill%d" % i, F1, size=half), rec("fill%d" % i, F2, size=need - half)]
        recs += fill + list(pair)
        stream += need
        cuts.append((stream, cut, kind))
        stream += sum(len(written(Rec(b))) for b in pair)
    raw = recs
    tiles, cur, n = [], [], 0
    for b in raw:   # tiles of about 40 KB; a record longer than that has a tile of its own
        if cur and n + len(b) > 40000:
            tiles.append(cur); cur, n = [], 0
        cur.append(b); n += len(b)
    tiles.append(cur)
    case = Case("window_cuts_bam", tiles, cuts=cuts, kw=dict(max_gap=-1, max_mm=-1))
    return case


def window_cut_premises(case, out_records):
    """out_records: the oracle's output records. Every designed boundary is a multiple of the piece and lies inside its probe pair at the designed offset"""
    starts, o = {}, 0
    for b in out_records:
        starts[o] = b; o += len(b)
    kinds = set()
    for at, cut, kind in case.notes["cuts"]:
        assert at in starts and (at + cut) % PIECE == 0, (at, cut, kind)
        opener = starts[at]
        closer = starts[at + len(opener)]
        assert Rec(opener).name == Rec(closer).name and 0 < cut < len(opener) + len(closer)
        kinds.add(kind)
        if kind == "cg300":
            assert Rec(opener).n_cigar == 300 and b"CGBI" not in opener
        if kind == "cg65536":
            assert Rec(opener).n_cigar == 2 and opener[-(8 + 4 * 65536):][:4] == b"CGBI" and len(opener) > 4 * PIECE
    assert kinds == {"plain", "cg300", "cg65536"}


SMALL = (run_lengths, held_chain, empty_tile, collisions, no_part, c_string_names)


def small_cases():
    return [f() for f in SMALL]
