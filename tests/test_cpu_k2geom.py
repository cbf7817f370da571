"""The designed member and tile geometry (tests/k2geom_cases.py) without a GPU: the oracle reads every case file and finds the model's records, every case
produces the numbers it was built for (records per entry at every walker shift, carried bytes per tile, entry counts - all from the sequential model, nothing
from the library), the restated constants are the source's, and on the aligned cases K2's guess (csrc/k2_guess.h through tests/emul/k2_guess_emul.cpp) finds
the true first record of every piece and group - the premise behind the path assertions of test_gpu_k2geom.py."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import emul_build
import k2geom_cases as K
import oracle_lib as O
from conftest import ROOT

CSRC = os.path.join(ROOT, "ngs-bits_amd", "csrc")
KSH = (0, 1, 2, 3)


def _flag(c, i):
    return struct.unpack_from("<H", c.raw, int(c.offs[i]) + 18)[0]


def _l_seq(c, i):
    return struct.unpack_from("<i", c.raw, int(c.offs[i]) + 20)[0]


# ---- constants ----
def test_constants_are_the_sources():
    common = open(os.path.join(CSRC, "common.h")).read()
    index = open(os.path.join(CSRC, "index.hip")).read()
    scan = open(os.path.join(CSRC, "scan.hip")).read()
    assert int(re.search(r"constexpr int K2_REL_STRIDE = (\d+);", common).group(1)) == K.K2_REL_STRIDE
    assert int(re.search(r"constexpr int NAME_SHIFT = (\d+);", common).group(1)) == K.NAME_SHIFT
    m = re.search(r"constexpr int SCAN_T = (\d+), SCAN_ITEMS = (\d+), SCAN_TILE = SCAN_T \* SCAN_ITEMS;", index)
    assert int(m.group(1)) * int(m.group(2)) == K.SCAN_TILE
    # the shapes the model restates: the stride of a piece, the walk's refusal at the last name, the walkers' range
    assert "return ksh >= 0 ? (uint32_t)K2_REL_STRIDE >> ksh : 0u;" in common
    assert "if (n >= (1u << NAME_SHIFT) - 1u) { res = -3; stop = true; break; }" in scan
    assert re.search(r"constexpr int K2_MAX_KSH = 3, K2_MIN_KSH = -4;", common)
    assert [K.stride(k) for k in (0, 1, 2, 3, -1, -2)] == [512, 256, 128, 64, 0, 0] and K.NAME_CAP == 4095


# ---- the oracle reads every file; the model's walk is the stream's ----
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("k2geom")
    made = {}

    def path(name):
        if name not in made:
            made[name] = K.get(name).write(str(d / f"{name}.bam"))
        return made[name]
    return path


@pytest.mark.parametrize("name", K.ALL)
def test_oracle_reads_the_case(files, name):
    c = K.get(name)
    offs = c.walk()
    assert np.array_equal(offs, c.offs) and offs[0] == c.first_rec
    b = O.Bam(files(name))
    assert b.count == offs.size and b.refs == c.refs and b.first_record_offset == c.first_rec
    assert np.array_equal(b.record_offsets(), offs)
    assert b.inflated().tobytes() == c.raw
    # what makes a miscounted record visible: the fields vary
    some = range(0, offs.size, max(1, offs.size // 3000))
    assert len({_flag(c, i) for i in some}) >= 8 and len({_l_seq(c, i) for i in some}) >= 3
    assert len({c.raw[int(c.offs[i]) + 13] for i in some}) >= 5 and len({struct.unpack_from("<i", c.raw, int(c.offs[i]) + 32)[0] for i in some}) >= 50   # MAPQ, insert size
    pos = [struct.unpack_from("<ii", c.raw, int(o) + 4) for o in offs]
    assert pos == sorted(pos)
    assert all(sz <= K.MEMBER_MAX for _, sz in c.pieces()) and len(c.raw) < 4 << 20
    assert len(c.sites()) >= 20 and c.bed()


def reference(c, path, d):
    """the oracle's answers for the job that test_gpu_k2geom.py runs on a case: MappingQC in WGS mode over the case's BED, and the pileup of its sites"""
    bed = os.path.join(str(d), c.name + ".bed")
    open(bed, "w").write(c.bed())
    b = O.Bam(path)
    sites = c.sites()
    return dict(bed=bed, sites=sites, mapping=O.mapping(b, O.MODE_WGS, bed, merge_bed=False), site_counts=O.site_pileup(b, sites, 1, 13, False))


@pytest.mark.parametrize("name", K.ALL)
def test_oracle_reference_sees_every_record(files, name, tmp_path):
    """the reference of the GPU test counts every record, and its order-dependent and per-base results are not trivially zero"""
    c = K.get(name)
    r = reference(c, files(name), tmp_path)
    m = r["mapping"]
    assert m["al_total"] == sum(1 for i in range(c.offs.size) if not _flag(c, i) & 0x900)
    assert m["al_mapped"] > 0 and m["bases_usable"] > 0 and m["insert_size_read_count"] > 0 and m["bases_trimmed"] > 0 and m["max_length"] >= 4
    assert m.depth.size == m["roi_bases"] > 0 and int(m.depth.sum()) > 0 and int(m.insert_hist.sum()) > 0
    assert int(r["site_counts"].sum()) > 0


# ---- premises ----
def _aligned(c):
    """a record starts at every member's first byte (the first member: the header) and none straddles a member"""
    starts = set(c.walk().tolist())
    return all(lo in starts for lo in c.member_borders())


@pytest.mark.parametrize("name", K.ALL)
def test_layouts_carry_what_the_model_says(name):
    """every tile's records, summed, are the file's; an aligned case carries nothing; the carried bytes fit the model's own account tile by tile"""
    c = K.get(name)
    assert _aligned(c) == c.aligned == (name in K.ALIGNED)
    for tm, _ in c.layouts:
        tiles = c.tile_model(tm)
        assert sum(t["starts"].size for t in tiles) == c.offs.size
        assert tiles[-1]["carry"] == 0 and tiles[0]["prefix"] == 0
        for a, b in zip(tiles, tiles[1:]):
            assert b["prefix"] == a["carry"] and b["u_lo"] == a["u_hi"]
        if c.aligned:
            assert all(t["carry"] == 0 for t in tiles)
        for ksh in KSH + (-1, -2):
            counts = c.entry_counts(tm, ksh)
            assert sum(int(x.sum()) for x in counts) == c.offs.size
            for t, x in zip(tiles, counts):   # entry 0 holds the carried record when it ends in this tile, and nothing else
                assert int(x[0]) == (1 if t["prefix"] and t["starts"].size and t["starts"][0] == 0 else 0)


@pytest.mark.parametrize("size", [44, 45])
def test_premise_stride(size):
    c = K.get(f"stride{size}")
    p = c.premises
    assert len(c.members()) == p["members"]
    inside = 0
    for ksh in KSH:
        (counts,) = c.entry_counts(None, ksh)
        pieces = counts[1:]
        s = K.stride(ksh)
        assert set(p["include"][ksh]) <= set(pieces.tolist()), (ksh, sorted(set(pieces.tolist())))
        assert p["include"][ksh] == [s - 1, s, s + 1, s + 8]
        assert (pieces > s).sum() >= 2 and (pieces == s).sum() >= 1 and (pieces < s).sum() >= 1
        below = {int(x) % 8 for x in pieces if 0 < x < s}
        assert {0, 1, 7} <= below, (ksh, below)          # full groups of eight, a group of one, a group of seven
        (tile,) = c.tile_model(None)
        starts = set(tile["starts"].tolist())
        inside += sum(1 for lo, hi in c.entries(tile, ksh)[1:] if hi > lo and lo not in starts and lo > c.first_rec)
    assert int(c.entry_counts(None, 0)[0].max()) == p["max_count"][0] == K.MEMBER_MAX // size
    assert inside >= 20   # pieces that begin inside a record: their start is a guess
    assert all((lo - c.first_rec) % size == 0 for lo in c.member_borders())


@pytest.mark.parametrize("name", ["deep_first", "deep_later"])
def test_premise_deep(name):
    c = K.get(name)
    p = c.premises
    (tm, _), = c.layouts
    lens = [_l_seq(c, i) for i in range(c.offs.size)]
    assert lens.index(max(lens)) == p["longest"] and lens.count(max(lens)) == 2        # the FIRST longest read: a second one follows
    assert [i for i in range(c.offs.size) if _flag(c, i) & 1][0] == p["first_paired"]
    for ksh in KSH:
        for i in (p["longest"], p["first_paired"]):
            tile, e, k = c.name_of(i, tm, ksh)
            assert tile == p["tile"] and k >= K.stride(ksh) and k < K.NAME_CAP, (ksh, i, tile, e, k)
    assert len(c.tile_model(tm)) == (3 if tm else 1)


@pytest.mark.parametrize("kind", ["4092", "4095", "4096", "drop"])
def test_premise_names(kind):
    c = K.get(f"names{kind}")
    (tm, _), = c.layouts
    groups = [int(x) for counts in c.entry_counts(tm, -2) for x in counts[1:]]
    assert groups == c.premises["groups"]
    assert c.expect["fits"] == (max(groups) <= K.NAME_CAP)
    assert {"4092": [4092] * 3, "4095": [4095] * 3, "4096": [4096] * 3, "drop": [4092, 4096, 4096, 4096, 4095, 4000]}[kind] == groups
    if kind == "drop":   # one group per tile: three tiles in a row exceed the names, the tiles behind them do not
        assert [len(x) for x in c.entry_counts(tm, -2)] == [2] * 6


def test_premise_borders():
    c = K.get("borders")
    p = c.premises
    assert set(c.border_cuts(c.member_borders())) >= set(p["cut_at"]) == {0, 1, 2, 3, 4, 20, 35, 36}
    for tm in (1, 2):
        assert set(c.border_cuts(c.tile_borders(tm))) >= set(p["cut_at"]), tm
        o, e = int(c.offs[p["long_record"]]), int(c.offs[p["long_record"] + 1])
        spans = sum(1 for t in c.tile_model(tm) if t["u_lo"] < e and t["u_hi"] > o)
        assert spans == p["long_spans"][tm] and spans >= 4
    # a record that ends exactly at a tile end, and tiles whose first bytes are a carried record's
    for tm in (1, 2):
        tiles = c.tile_model(tm)
        assert any(t["carry"] == 0 for t in tiles[:-1]) and sum(1 for t in tiles if t["prefix"]) >= 7
        assert {t["carry"] for t in tiles} >= {1, 2, 3, 4, 20, 35, 36}


def test_premise_degenerate():
    c = K.get("degenerate")
    p = c.premises
    sizes = [n for _, n in c.pieces()]
    assert sizes.count(0) == p["empty"] and {1, 2, 3} <= set(sizes)
    assert sum(1 for _, n in c.pieces()[1:-1] if 0 < n <= 3) >= p["tiny_run"] + 3
    cut_at = c.border_cuts(c.member_borders())
    assert {1, 2, 3} & set(cut_at) and 2 in cut_at and 3 in cut_at       # borders inside block_size
    for tm in (1, 4):
        tiles = c.tile_model(tm)
        # a tile that holds only tiny members, inside one record: nothing starts or ends in it
        assert any(t["starts"].size == 0 and t["prefix"] > 0 and t["carry"] == t["prefix"] + t["u_hi"] - t["u_lo"] and all(n <= 3 for _, n in t["members"]) for t in tiles), tm
        # the last tile: the last byte of the last record
        last = tiles[-1]
        assert last["u_hi"] - last["u_lo"] == 1 and last["starts"].tolist() == [0] and last["prefix"] == len(c.raw) - 1 - int(c.offs[-1])
    assert len(c.members()) % 4 == 1


@pytest.mark.parametrize("name", ["header_end", "header_mid"])
def test_premise_header(name):
    c = K.get(name)
    p = c.premises
    assert c.first_rec == p["header"] > 3 * 20000
    tiles = c.tile_model(1)
    head = [t for t in tiles if t["u_hi"] <= c.first_rec]
    assert len(head) == p["header_tiles"] >= 3 and all(t["starts"].size == 0 and t["carry"] == 0 for t in head)
    first = tiles[len(head)]
    assert c.first_rec - first["u_lo"] == (5000 if name == "header_mid" else 0)


@pytest.mark.parametrize("name", ["entries4095", "entries4096", "entries4097", "entries4093m", "entries4094m", "pieces520"])
def test_premise_entries(name):
    c = K.get(name)
    if name == "pieces520":
        (counts,) = c.entry_counts(None, 3)
        assert counts.size == c.premises["entries"][3] == 4161 > K.SCAN_TILE and len(c.members()) == 520
        return
    (counts,) = c.entry_counts(None, 0)
    assert counts.size == c.premises["entries"] == len(c.members()) + 1
    assert set(counts[1:].tolist()) == ({1, 2, 3} if name.endswith("m") else {1})
    assert abs(counts.size - K.SCAN_TILE) <= 2
    assert sorted(K.get(n).premises["entries"] for n in K.ALL if n.startswith("entries")) == [4094, 4095, 4096, 4097, 4098]


@pytest.mark.parametrize("name", ["carry_full", "carry_over"])
def test_premise_carry(name):
    c = K.get(name)
    (tm, cm), = c.layouts
    assert (tm, cm) == (1, K.CARRY_MAX)
    assert [t["carry"] for t in c.tile_model(tm)] == c.premises["carry"] == [K.CARRY_MAX + (name == "carry_over"), 0, 0]
    assert (c.refuses is not None) == (c.premises["carry"][0] > K.CARRY_MAX)


# ---- K2's guess on the aligned cases ----
@pytest.fixture(scope="module")
def guess():
    L = C.CDLL(emul_build.library("k2_guess_emul.cpp"))
    L.k2_guess_first.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    return L


@pytest.mark.parametrize("name", K.ALIGNED)
def test_guess_finds_the_first_record_of_every_piece(guess, name):
    """the first plausible record start of every piece (ksh 0..3) and of every group of members (ksh -1, -2) behind the tile's known first record is the piece's
    true first record, or none where none starts: no designed byte pattern looks like a record start"""
    c = K.get(name)
    n_checked = 0
    for tm, _ in c.layouts:
        for t in c.tile_model(tm):
            assert t["prefix"] == 0
            total = t["u_hi"] - t["u_lo"]
            infl = np.concatenate([np.frombuffer(c.raw[t["u_lo"]:t["u_hi"]], dtype=np.uint8), np.zeros(64, np.uint8)])   # (the tile buffers are padded as well)
            exp0 = max(c.first_rec - t["u_lo"], 0)
            starts = t["starts"]
            for ksh in KSH + (-1, -2):
                rng = [(lo, hi) for lo, hi in c.entries(t, ksh)[1:] if hi > lo and lo > exp0]
                lo = np.array([r[0] for r in rng], dtype=np.int64); hi = np.array([r[1] for r in rng], dtype=np.int64)
                got = np.zeros(lo.size, np.int64)
                guess.k2_guess_first(infl.ctypes.data, total, len(c.refs), lo.ctypes.data, hi.ctypes.data, lo.size, got.ctypes.data)
                j = np.searchsorted(starts, lo, side="left")
                want = np.where(j < starts.size, starts[np.minimum(j, starts.size - 1)], -1)
                want = np.where((want >= 0) & (want < hi), want, -1)
                bad = np.nonzero(got != want)[0]
                assert bad.size == 0, (tm, ksh, [(int(lo[i]), int(hi[i]), int(got[i]), int(want[i])) for i in bad[:5]])
                n_checked += lo.size
    assert n_checked > 20
