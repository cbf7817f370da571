"""The designed shard, range and head cases (tests/partial_cases.py) without a GPU: the oracle reads every case file, the sequential model recomputes every
case's premises (which border cuts which record after how many bytes, which shards own nothing, how many tail members a last record needs), the shards of
every N and consecutive ranges give the walk back - every record once, in order -, three value-only mutations of the model are each told apart by the
catalogue (the table prints under -s), and K2's guess (csrc/k2_guess.h on the CPU) accepts the first decoy record. test_gpu_partial_designed.py then holds
the library to the model."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import emul_build
import k2geom_cases as K
import oracle_lib as O
import partial_cases as P
from conftest import ROOT

CSRC = os.path.join(ROOT, "ngs-bits_amd", "csrc")


def test_constants_and_messages_are_the_sources():
    head = open(os.path.join(ROOT, "include", "ngsqc.h")).read()
    assert int(re.search(r"#define NGSQC_E_FORMAT\s+(-?\d+)", head).group(1)) == P.E_FORMAT
    assert int(re.search(r"#define NGSQC_E_ARG\s+(-?\d+)", head).group(1)) == P.E_ARG
    sw = open(os.path.join(CSRC, "switches.h")).read()
    assert int(re.search(r'env_int_clamped\("NGSQC_SHARD_TAIL_MEMBERS", (\d+),', sw).group(1)) == P.DEFAULT_TAIL
    tiles, image, jobs = (open(os.path.join(CSRC, f)).read() for f in ("tiles.hip", "image.hip", "jobs.hip"))
    assert P.MSG_TAIL in tiles and '"a record at the end of shard " + std::to_string(h->shard)' in tiles
    assert P.MSG_BEHIND in image and P.MSG_NO_BLOCK in image and P.MSG_JOIN in jobs
    assert len(P.cram_twin._bgzf(b"")) == P.EOF_BYTES


@pytest.mark.parametrize("name", P.ALL)
def test_oracle_reads_the_case(tmp_path, name):
    p = P.get(name)
    c, m = p.case, p.model()
    b = O.Bam(p.write(str(tmp_path / (name + ".bam"))))
    assert b.count == m.offs.size and b.first_record_offset == m.first_rec and np.array_equal(b.record_offsets(), m.offs)
    assert b.inflated().tobytes() == c.raw and b.n_blocks == len(m.all)     # (the oracle counts the empty members too)
    if not name.startswith("k2_") and name != "shard_header":   # (the reused k2geom files keep their own member sizes)
        assert max(x[3] for x in m.all) <= 20000
        sizes = {int(e - o) for o, e in zip(m.offs, m.ends)}
        assert sizes - {44} <= {int(m.ends[i] - m.offs[i]) for i in p.premises.get("longs", []) + [p.premises.get("record", -1), (p.decoy or {}).get("host", -1)] if i >= 0}
    pos = [struct.unpack_from("<ii", c.raw, int(o) + 4) for o in m.offs]
    assert pos == sorted(pos)


def _digest(m, p):
    """what a model says about every run of a case"""
    out = []
    for N in sorted({N for N, _ in p.shard_runs}):
        out.append(tuple((x["n_records"], x["first_abs"], x["exit_abs"], x["n_blocks"], x["kind"]) for x in m.shards(N)))
    for N, tail in p.tails:
        out.append(tuple((x["refuses"], x["n_blocks"]) for x in m.shards(N, tail)))
    return out


# ---- shards: every record once, in order ----
@pytest.mark.parametrize("name", P.SHARD_CASES)
def test_shards_give_the_walk(name):
    p = P.get(name); m = p.model()
    for N in sorted({N for N, _ in p.shard_runs} | set(range(1, 41))):
        sh = m.shards(N)
        owned = np.concatenate([x["owned"] for x in sh])
        assert np.array_equal(owned, m.offs), (name, N)
        assert sum(x["m1"] - x["m0"] for x in sh) == len(m.tab)
        cur = -1
        for x in sh:   # the chain rule of ngsqc_plan_shard_fix
            if x["first_abs"] >= 0:
                assert cur < 0 or x["first_abs"] == cur, (name, N)
                cur = x["exit_abs"]
        assert cur == m.total
        for x in sh:
            if x["kind"] == "plain":
                assert np.array_equal(x["local"], x["owned"] - m.upos(x["m0"])) and x["inflated"][1] - x["inflated"][0] >= x["own_bytes"] > 0
            assert not x["refuses"], (name, N, "the default tail suffices")


# ---- premises ----
def test_premise_shard_borders():
    p = P.get("shard_borders"); m = p.model()
    assert sorted(p.premises["cut_at"]) == sorted(K.CUT_AT) == [0, 1, 2, 3, 4, 20, 35, 36]
    for d, N in p.premises["cut_at"].items():
        assert N in {n for n, _ in p.shard_runs}
        assert d in P._cuts_hit(m, N), (d, N)
        u = p.premises["at"][d]
        s = next(s for s, x in enumerate(m.shards(N)) if x["kind"] == "plain" and x["u0"] == u)
        before, here = m.shard(s - 1, N), m.shard(s, N)
        k = int(np.searchsorted(m.offs, u, side="left"))
        if d:      # the record cut by the border is the previous shard's last one and needs this shard's first member
            assert before["owned"][-1] == m.offs[k - 1] == u - d and before["need"] >= 1 and here["first_abs"] == m.offs[k] == before["exit_abs"]
        else:
            assert here["first_abs"] == u == before["exit_abs"] and before["need"] == 0
    assert {tm for _, tm in p.shard_runs} == {None, 1, 2}


def test_premise_shard_header():
    p = P.get("shard_header"); m = p.model()
    for key, N in p.premises.items():
        sh = m.shards(N)
        if key == "header_only":
            x = next(x for x in sh if x["kind"] == "header")
            assert x["m1"] > x["m0"] and m.upos(x["m1"]) <= m.first_rec and x["n_blocks"] == 0 and (x["n_records"], x["first_abs"], x["exit_abs"]) == (0, -1, -1)
        elif key == "header_ends_inside":
            x = next(x for x in sh if x["kind"] == "plain" and 0 < x["u0"] < m.first_rec)
            assert x["first_abs"] == m.first_rec and x["local"][0] == m.first_rec - x["u0"] > 0
        else:
            x = next(x for x in sh if x["kind"] == "plain" and x["u0"] == m.first_rec)
            assert x["first_abs"] == m.first_rec and x["local"][0] == 0
    assert set(p.premises) == {"header_only", "header_ends_inside", "first_rec_at_start"}


def test_premise_shard_tiny():
    p = P.get("shard_tiny"); m = p.model()
    nb = p.premises["members"]
    assert nb == len(m.tab) and {nb, nb + 1, 16 * nb} <= {N for N, _ in p.shard_runs}
    sizes = [x[3] for x in m.all[:-1]]
    assert sizes.count(0) == 3 == len(p.premises["empty"]) and {1, 2, 3} <= set(sizes) and sum(1 for n in sizes if 0 < n <= 3) >= 11 + 2
    # a block_size word split across two shards: two bytes in one, two in the next
    word = p.premises["word"]
    N = p.premises["word_split"]
    assert word + 1 in m.shard_borders(N) and word - 2 in set(m.offs.tolist()) and 3 in P._cuts_hit(m, N)
    assert word + 1 in m.shard_borders(16 * nb) and word in m.shard_borders(16 * nb)
    # a shard of tiny members of the run alone: it owns nothing and reports (-1, -1)
    lo, hi = p.premises["run"]
    x = next(x for x in m.shards(p.premises["tiny_shard"]) if x["kind"] == "plain" and lo <= x["u0"] and x["lim"] <= hi)
    assert x["m1"] - x["m0"] >= 2 and (x["n_records"], x["first_abs"], x["exit_abs"]) == (0, -1, -1) and x["own_bytes"] < hi - lo
    k = int(np.searchsorted(m.offs, lo, side="right")) - 1
    assert m.offs[k] < lo and hi < m.ends[k]                          # ... inside one record
    # at 16 x members shards without a member exist, and most member starts are shard borders
    kinds = [x["kind"] for x in m.shards(16 * nb)]
    assert kinds.count("empty") > 10 * nb and len(m.shard_borders(16 * nb)) >= nb - 3


def test_premise_shard_long():
    p = P.get("shard_long"); m = p.model()
    N = p.premises["N"]
    sh = m.shards(N)
    needs, covered = [], []
    for i in p.premises["longs"]:
        s = next(s for s, x in enumerate(sh) if x["n_records"] and x["owned"][-1] == m.offs[i])
        needs.append(sh[s]["need"])
        inside = [x for x in sh if x["kind"] == "plain" and m.offs[i] < x["u0"] and x["lim"] <= m.ends[i]]
        assert all(x["n_records"] == 0 and x["first_abs"] == -1 for x in inside)
        covered.append(len(inside))
    assert needs == p.premises["need"] == [1, 2, 3] and covered == p.premises["covered"] == [0, 1, 2]
    for n, tail in p.tails:   # T - 1 refuses the shard that needs T, and only shards that need more than the tail
        assert n == N
        ref = [s for s, x in enumerate(m.shards(N, tail)) if x["refuses"]]
        assert ref == [s for s, x in enumerate(sh) if x["need"] > tail]
        assert len(ref) == max(3 - tail, 0)
    assert sorted(t for _, t in p.tails) == [0, 1, 2, 3]


def test_premise_shard_last():
    p = P.get("shard_last"); m = p.model()
    N = p.premises["last_alone"]
    sh = m.shards(N)
    assert m.tab[-1][3] == 1 and m.offs[-1] < m.tab[-1][2] < m.ends[-1] == m.total
    assert (sh[-1]["m0"], sh[-1]["m1"]) == (len(m.tab) - 1, len(m.tab)) and (sh[-1]["n_records"], sh[-1]["first_abs"], sh[-1]["exit_abs"]) == (0, -1, -1)
    prev = [x for x in sh if x["n_records"]][-1]
    assert prev["need"] == 1 and prev["exit_abs"] == m.total
    assert [x["refuses"] for x in m.shards(N, 0)].count(True) == 1 and not any(x["refuses"] for x in m.shards(N, 1))


def test_premise_shard_tiles():
    p = P.get("shard_tiles"); m = p.model()
    i, cuts = p.premises["record"], p.premises["cuts"]
    o, e = int(m.offs[i]), int(m.ends[i])
    assert all(o < u < e for u in cuts)
    for key, u, k in (("two_tiles", cuts[1], 2), ("one_tile", cuts[2], 1)):
        x = next(x for x in m.shards(p.premises[key]) if x["kind"] == "plain" and x["u0"] == u)
        # tiles of one member: the first k lie inside the record, nothing starts in them; the shard owns records all the same
        assert m.upos(x["m0"] + k) < e <= m.upos(x["m0"] + k + 1) and x["n_records"] > 0 and x["first_abs"] == e
        assert x["m1"] - x["m0"] > k
    assert {tm for _, tm in p.shard_runs} == {None, 1, 2}


@pytest.mark.parametrize("name", P.DECOYS)
def test_premise_decoy_geometry(name):
    p = P.get(name); m = p.model(); d = p.decoy
    host = d["host"]
    o, e = int(m.offs[host]), int(m.ends[host])
    assert 44000 < e - o < 46000
    spans = [x for x in m.tab if x[2] < e and x[2] + x[3] > o]
    assert len(spans) == 3 and spans[-1][2] == d["member_at"] and spans[-1][2] + spans[-1][3] == e     # three members; the last ends with the host record
    assert not ((m.offs >= d["member_at"]) & (m.offs < e)).any()                                          # no true record starts in that member
    N = p.premises["border"]
    x = next(x for x in m.shards(N) if x["kind"] == "plain" and x["u0"] == d["member_at"])
    assert x["first_abs"] == e and x["n_records"] > 100
    assert d["member_at"] < d["first"] and d["first"] + 44 * d["n"] == e - (10 if name.endswith("dies") else 0)
    # the decoys are real records on chrX, where no true record lies; some of them would be counted by the depth scan
    tids = {struct.unpack_from("<i", p.case.raw, int(q) + 4)[0] for q in m.offs}
    assert tids == {0}
    counted = 0
    for k in range(d["n"]):
        q = d["first"] + 44 * k
        bs, tid, pos, l_name, mapq, _, n_cig, flag = struct.unpack_from("<IiiBBHHH", p.case.raw, q)
        assert bs == 40 and tid == 1
        counted += n_cig == 1 and mapq >= 1 and not flag & (0x4 | 0x100 | 0x200 | 0x400 | 0x800)
    assert counted >= 5
    assert "chrX" in p.case.bed()


@pytest.fixture(scope="module")
def guess():
    L = C.CDLL(emul_build.library("k2_guess_emul.cpp"))
    L.k2_guess_classify.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    L.k2_guess_first.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    return L


@pytest.mark.parametrize("name", P.DECOYS)
def test_premise_decoy_passes_the_guess(guess, name):
    """plausible_chain accepts the first decoy record, and the first guess of the shard's first member is that record"""
    p = P.get(name); m = p.model(); d = p.decoy
    x = next(x for x in m.shards(p.premises["border"]) if x["kind"] == "plain" and x["u0"] == d["member_at"])
    lo, hi = x["inflated"]
    infl = np.concatenate([np.frombuffer(p.case.raw[lo:hi], dtype=np.uint8), np.zeros(64, np.uint8)])
    at = np.array([d["first"] - lo], dtype=np.int64); out = np.zeros(1, np.uint8)
    guess.k2_guess_classify(infl.ctypes.data, hi - lo, len(p.case.refs), at.ctypes.data, 1, out.ctypes.data)
    assert out[0] == 7
    member_hi = int(m.ends[d["host"]]) - lo
    a, b, got = np.array([0], np.int64), np.array([member_hi], np.int64), np.zeros(1, np.int64)
    guess.k2_guess_first(infl.ctypes.data, hi - lo, len(p.case.refs), a.ctypes.data, b.ctypes.data, 1, got.ctypes.data)
    assert got[0] == d["first"] - lo


# ---- ranges ----
@pytest.mark.parametrize("name", P.RANGE_CASES)
def test_consecutive_ranges_give_the_walk(name):
    p = P.get(name); m = p.model()
    for k in (1, 2, 3, 5, 8, 13):
        parts = [m.range(b, e) for b, e in P.split_ranges(m, k)]
        assert all(r["refuses"] is None for r in parts), (name, k)
        assert np.array_equal(np.concatenate([r["owned"] for r in parts]), m.offs), (name, k)


@pytest.mark.parametrize("name", P.RANGE_CASES)
def test_premise_ranges(name):
    p = P.get(name); m = p.model()
    got = {tag: m.range(b, e) for tag, b, e, _ in p.ranges}
    starts = set(m.offs.tolist())
    for tag, b, e, _ in p.ranges:
        r = got[tag]
        if tag.startswith("refuse"):
            assert r["refuses"] == (P.E_ARG, P.MSG_BEHIND if tag == "refuse_behind" else P.MSG_NO_BLOCK)
            continue
        assert r["refuses"] is None and not r["cut"], tag
        if tag != "empty_members_only":
            assert r["n_records"] > 0 and r["owned"][0] in starts and np.array_equal(r["local"], r["owned"] - r["inflated"][0])
    if name != "shard_tiles":
        assert got["one_member"]["n_blocks"] == 1 and got["one_member"]["n_records"] >= 2
        assert np.array_equal(got["from_voff0"]["owned"], got["from_first_record"]["owned"]) and got["from_voff0"]["owned"][0] == m.first_rec
        assert got["from_voff0"]["local"][0] == m.first_rec          # never in front of the first record
        for tag in ("end_member_start", "end_eof_member", "end_file_size"):
            b, e = next((b, e) for t, b, e, _ in p.ranges if t == tag)
            assert e & 0xffff == 0
        assert got["end_eof_member"]["owned"][-1] == got["end_file_size"]["owned"][-1] == m.offs[-1]
        assert got["end_member_start"]["inflated"][1] in starts
    if name == "shard_tiny":
        at = p.premises["empty_at"]
        assert got["beg_empty_member"]["owned"][0] == at and got["beg_empty_member"]["local"][0] == 0
        assert got["end_empty_member"]["owned"][-1] == m.offs[np.searchsorted(m.offs, at) - 1] and got["end_empty_member"]["inflated"][1] == at
        assert got["empty_members_only"]["n_blocks"] == 0 and got["empty_members_only"]["n_records"] == 0
    if name == "shard_long":
        for k, i in enumerate(p.premises["longs"]):
            r = got[f"last_spans_{k + 1}"]
            crossed = sum(1 for x in m.tab if m.offs[i] < x[2] < m.ends[i])
            assert r["owned"][-1] == m.offs[i] and crossed == k + 1 and m.ends[i] <= r["inflated"][1]
        assert any(r["n_records"] and m.ends[np.searchsorted(m.offs, r["owned"][-1])] == r["inflated"][1] for r in got.values())   # a last record that ends at a member end
    assert {tm for *_, tm in p.ranges} >= {1, 2}


# ---- heads ----
@pytest.mark.parametrize("name", P.HEAD_CASES)
def test_premise_heads(name):
    p = P.get(name); m = p.model()
    H = p.premises["header"]
    assert H == m.first_rec > 60000
    hold = [x for x in m.all if x[2] <= H < x[2] + x[3]]
    got = {tag: m.head(k, tail) for tag, k, tail, _ in p.heads}
    if name == "head_hdr8":
        assert [x[2] + x[3] for x in m.all[:8]][-1] == H and hold[0] == m.all[8]      # the header is exactly the first eight members
        assert got["one"]["plan"][0] == m.all[8][0] << 16 and got["one"]["local"][0] == 0
        assert got["two_tail0"]["refuses"] == (P.E_FORMAT, P.MSG_TAIL) and got["two_tiles1"]["refuses"] is None
        assert np.array_equal(got["more_than_left"]["owned"], m.offs) and got["more_than_left"]["plan"][1] == 0
    else:
        assert [x[2] for x in m.all[:4]] == [0, 20000, 40000, 60000] and hold[0] == m.all[3]     # over four members; the first record starts mid-member
        assert got["cut_default"]["plan"][0] == m.all[3][0] << 16 | (H - 60000)
        assert got["cut_tail0"]["refuses"] == (P.E_FORMAT, P.MSG_TAIL)
        for tag in ("cut_tail1", "cut_default", "cut_tiles1"):
            r = got[tag]
            assert r["refuses"] is None and r["n_records"] > 0
        # the last own record is cut at own_end: it starts in front of the boundary and ends behind it
        r = got["cut_tail1"]
        lim = m.all[4][2]
        assert r["owned"][-1] < lim < m.ends[np.searchsorted(m.offs, r["owned"][-1])] and r["n_blocks"] == 2
        assert np.array_equal(r["owned"], got["cut_default"]["owned"]) and got["cut_default"]["n_blocks"] > 2
        assert got["three_end"]["refuses"] is None                                                  # (that boundary is a record's end: no tail needed)
        assert np.array_equal(got["more_than_left"]["owned"], m.offs)
    for r in got.values():
        if r["refuses"] is None and r["n_records"]:
            assert r["owned"][0] == H


# ---- the mutations ----
def test_the_catalogue_tells_the_mutations_apart(capsys):
    rows = []
    for mut, aimed in (("le", "shard_borders"), ("tail", "shard_long"), ("member_start", "shard_tiny")):
        caught = [n for n in P.SHARD_CASES if _digest(P.get(n).model(), P.get(n)) != _digest(P.get(n).model(mut), P.get(n))]
        rows.append((mut, aimed, caught))
    with capsys.disabled():
        print("\nmutation        aimed at        caught by")
        for mut, aimed, caught in rows:
            print(f"{mut:15s} {aimed:15s} {', '.join(caught) or '-'}")
        print(f"{sum(1 for r in rows if r[2])} mutations caught")
    for mut, aimed, caught in rows:
        assert aimed in caught, (mut, caught)
