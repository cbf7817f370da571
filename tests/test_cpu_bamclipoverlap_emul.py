"""The device's visit of a read pair and the bytes of its two records (ngs-bits_amd/csrc/clip_visit.h - the text the GPU library compiles into the plan and
gather kernels of BamClipOverlap) on the CPU, against the literal Python restatement (tests/bamclipoverlap_oracle.py): the two-cursor merge against the lists
with '+' placeholders, the one-pass soft-clip rewrite against the per-base matrix, the patched bases and qualities, and the error codes, on designed pairs in
every mode and on a seeded random family. Plain integer code: held here without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import bamclipoverlap_oracle as O
import clip_cases as K
import emul_build
from conftest import ROOT

HEADER = O.read_bam(K.bam_bytes([], K.REFS))[0]
ALL_MODES = [(m, ii) for m in (0, O.MAPQ, O.REMOVE, O.BASEQ, O.BASEN) for ii in (False, True)]
SEED_PAIR = K.pair("seed", (K.F1, 100, "30M"), (K.R2, 110, "30M"))   # one clipped pair in front: reads_clipped is 2 at the pair behind it


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(emul_build.library("clip_emul.cpp"))
    L.clip_emul_pair.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
    L.clip_emul_joins.argtypes = [C.c_char_p]
    L.clip_emul_soft_clip.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return L


def emulate(L, a, b, mode, ii, parity):
    """-> (plan rows forward / reverse, (soft_clip, forward is opener, overlap), (err, a, b), [forward bytes, reverse bytes] or None)"""
    plan, info, err, n = np.zeros(12, np.int32), np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(2, np.int64)
    cap = len(a) + len(b) + 4096
    out = np.full(cap, 0xEE, np.uint8)
    wrote = L.clip_emul_pair(a + bytes(8), b + bytes(8), mode, int(ii), parity, plan.ctypes.data, info.ctypes.data, err.ctypes.data, out.ctypes.data, cap, n.ctypes.data)
    recs = None
    if wrote:
        assert np.all(out[int(n.sum()):] == 0xEE)   # nothing behind the two records
        recs = [out[:n[0]].tobytes(), out[n[0]:n[0] + n[1]].tobytes()]
    return [list(map(int, plan[:6])), list(map(int, plan[6:]))], tuple(map(int, info)), tuple(map(int, err)), recs


def restate(a, b, mode, ii, parity):
    """the restatement on the file [seed pair,] a, b -> (plan rows of a and b, written records of the pair or [] when removed, ClipError or None)"""
    recs = (list(SEED_PAIR[1:]) if parity else []) + [a, b]
    try:
        r = O.run(HEADER, recs, mode, ii, verbose=False)
    except O.ClipError as e:
        assert e.record == len(recs) - 1
        return None, None, e
    return r.plan[-2:], r.records[2 if parity else 0:], None


def compare(L, label, a, b, mode, ii, parity):
    """-> the error code, or 0"""
    rows, out, e = restate(a, b, mode, ii, parity)
    plan, info, err, got = emulate(L, a, b, mode, ii, parity)
    what = (label, mode, ii, parity)
    if e is not None:
        assert err == (e.code, e.a, e.b), what
        return e.code
    assert err == (0, 0, 0), what
    by_role = {r[0]: r for r in rows}
    assert plan[0] == by_role[O.FORWARD] and plan[1] == by_role[O.REVERSE], what
    soft = bool(plan[0][5] & O.V_CLIP_PAIR)
    assert info[0] == soft, what
    if not soft:
        assert got is None and out == ([a, b] if info[1] else [b, a]), what   # the pair leaves as it came, forward read first
    elif plan[0][5] & O.V_REMOVED:
        assert out == [] and got == [b"", b""], what
    else:
        assert got == out, what
    return 0


def test_designed_pairs_in_every_mode(lib):
    seen_bits = 0
    for label, a, b in K.designed_pairs():
        assert lib.clip_emul_joins(a + bytes(8)) == 1 and lib.clip_emul_joins(b + bytes(8)) == 1, label
        for mode, ii in ALL_MODES:
            for parity in (0, 1):
                assert compare(lib, label, a, b, mode, ii, parity) == 0, label
        seen_bits |= emulate(lib, a, b, O.BASEN, False, 0)[0][0][5]
    assert seen_bits & O.V_BASES and seen_bits & O.V_REWRITTEN


def test_designed_pairs_cover_the_branches(lib):
    """what the designed list is for is really there: both clip targets of has_indel, all-S mates, D-only CIGAR, leading shifts"""
    got = {}
    for label, a, b in K.designed_pairs():
        got[label] = [emulate(lib, a, b, 0, False, p) for p in (0, 1)]
    for at, inside in ((15, False), (16, True), (20, True), (24, True), (25, False)):
        for kind in ("ins", "del"):
            (p0, *_), (p1, *_) = got[f"{kind}_fwd_{at}"]
            assert ((p0[0][1], p0[1][1]) == (0, 20) and (p1[0][1], p1[1][1]) == (20, 0)) == inside, (kind, at)
    for at, inside in ((5, False), (6, True), (10, True), (14, True), (15, False)):
        (p0, *_), _ = got[f"ins_rev_{at}"]
        assert (p0[0][1], p0[1][1]) == ((0, 20) if inside else (10, 10)), at
    assert got["all_s_plain"][0][0][0][1] == 10 and got["all_s_plain"][0][3][0][36 + 14:36 + 18] == (10 << 4 | 4).to_bytes(4, "little")
    assert got["only_d_read"][1][3][0][36 + 14:36 + 18] == b"\xff\xff\xff\xff"
    assert got["apart"][0][1][0] == 0 and got["touching"][0][1][0] == 0 and got["one_base_both"][0][1] == (1, 1, 1)


def test_random_family(lib):
    pairs = K.random_pairs(2000)
    assert len(pairs) >= 2000
    n_err = n_soft = n_mm = 0
    for k, (label, a, b) in enumerate(pairs):
        mode, ii = ALL_MODES[k % len(ALL_MODES)]
        parity = (k // len(ALL_MODES)) & 1
        if not (lib.clip_emul_joins(a + bytes(8)) and lib.clip_emul_joins(b + bytes(8))):
            continue
        code = compare(lib, label, a, b, mode, ii, parity)
        n_err += code != 0
        if not code:
            bits = emulate(lib, a, b, mode, ii, parity)[0][0][5]
            n_soft += bool(bits & O.V_CLIP_PAIR); n_mm += bool(bits & O.V_MISMATCH)
    # the comparison is not hollow: at most a tenth of the pairs end in an error, most are clipped, many carry a mismatch
    assert n_err <= len(pairs) // 10 and n_err >= 5, n_err
    assert n_soft >= len(pairs) // 2 and n_mm >= 100, (n_soft, n_mm)


def test_error_pairs(lib):
    codes = set()
    for label, a, b, name, mode in K.error_pairs():
        want = getattr(O, name)
        for parity in (0, 1):
            assert compare(lib, label, a, b, mode, False, parity) == want, label
        codes.add(want)
    assert codes == {O.E_CIGAR_CHAR, O.E_LENGTH, O.E_SC_INDEX, O.E_SC_OP, O.E_BAD_BASE, O.E_UNSUPPORTED}
    # the length error carries the two lengths, also where the reverse list ends first
    by = {p[0]: p for p in K.error_pairs()}
    assert emulate(lib, *by["err_length_forward_short"][1:3], 0, False, 0)[2] == (O.E_LENGTH, 3, 4)
    assert emulate(lib, *by["err_length_reverse_ends_first"][1:3], 0, False, 0)[2] == (O.E_LENGTH, 3, 2)
    # the unstorable base matters under -overlap_mismatch_basen alone
    assert compare(lib, "err_bad_base", *by["err_bad_base"][1:3], O.BASEQ, False, 0) == 0


def test_unreachable_errors_are_unreachable():
    """E_ORIENT and three of softClipAlignment's failures: for every s1 <= e1, s2 <= e2 that overlap, a branch is taken and the clips fit the reads"""
    for s1 in range(1, 8):
        for e1 in range(s1, 9):
            for s2 in range(1, 8):
                for e2 in range(s2, 9):
                    if not ((s2 <= s1 <= e2) or (s2 <= e1 <= e2) or (s1 <= s2 and e1 >= e2)):
                        continue
                    for both in (False, True):
                        for read1 in (False, True):
                            if s1 <= s2 and e1 <= e2: ov = e1 - s2 + 1; cf = cr = ov // 2; odd = True
                            elif s1 > s2 and e1 > e2: ov = e2 - s1 + 1; cf = ov // 2 + e1 - e2; cr = ov // 2 + s1 - s2; odd = True
                            elif both and s1 >= s2 and e1 <= e2: ov = e1 - s1 + 1; cf = ov // 2; cr = ov // 2 + s1 - s2; odd = True
                            elif both and s1 <= s2 and e1 >= e2: ov = e2 - s2 + 1; cf = ov // 2 + e1 - e2; cr = ov // 2; odd = True
                            elif not both and s1 >= s2 and e1 <= e2: ov = e1 - s1 + 1; cf, cr, odd = ov, 0, False
                            elif not both and s1 <= s2 and e1 >= e2: ov = e2 - s2 + 1; cf, cr, odd = 0, ov, False
                            else: raise AssertionError("orientation not identified")
                            if odd and read1: cf += ov % 2
                            elif odd: cr += ov % 2
                            for c_f, c_r in ((cf, cr), (0, ov), (ov, 0)):   # (as computed, and moved to one mate by has_indel)
                                assert ov >= 1 and 0 <= c_f <= e1 - s1 + 1 and 0 <= c_r <= e2 - s2 + 1


def test_parity_over_a_sequence_with_removed_pairs(lib):
    """reads_clipped counts removed pairs too: the pair behind a removed one sends its clip to the other mate"""
    ind = K.pair("indel", (K.F1, 100, "20M1I10M"), (K.R2, 110, "10M1I20M"))   # (the same insertion in both mates: no mismatch)
    s = K.genome_seq(110, "30M")
    mm = K.pair("mismatch", (K.F1, 100, "30M"), (K.R2, 110, "30M", dict(seq=K.mutate(s, 4))))
    apart = K.pair("apart", (K.F1, 100, "30M"), (K.R2, 300, "30M"))
    seq = [ind, mm, ind, apart, ind, mm, mm, ind]
    recs = []
    for k, (label, a, b) in enumerate(seq):
        recs += [a, b]
    # (the names repeat: every name is closed before it comes again)
    r = O.run(HEADER, recs, O.REMOVE, False, verbose=False)
    assert r.counts[2] == 14 and r.counts[3] == 6 and len(r.records) == len(recs) - 6
    clipped_before = 0
    for k, (label, a, b) in enumerate(seq):
        plan, info, err, _ = emulate(lib, a, b, O.REMOVE, False, clipped_before & 1)
        assert plan == [r.plan[2 * k], r.plan[2 * k + 1]], (k, label)
        if label == "indel":
            assert (plan[0][1], plan[1][1]) == ((0, 20) if clipped_before % 2 == 0 else (20, 0)), k
        clipped_before += info[0]
    assert clipped_before == 7


def test_soft_clip_vectors_of_the_reference(lib):
    """NGSHelper_Test.cpp:77-123 through the one-pass rewrite"""
    recs = O.read_bam(os.path.join(ROOT, "tests", "golden", "ref_in", "BamClipOverlap", "bamclipoverlap.bam"))[1]

    def clip(b, start, end):
        words, n, pos = np.zeros(64, np.uint32), C.c_int(0), C.c_int(0)
        assert lib.clip_emul_soft_clip(b + bytes(8), start, end, words.ctypes.data, 64, C.byref(n), C.byref(pos)) == 0
        return "".join(f"{w >> 4}{O.CIGAR_CHR[w & 15]}" for w in words[:n.value].tolist()), pos.value + 1
    k = 17
    while O.Rec(recs[k]).flag & 4:
        k += 1
    assert clip(recs[k], 33038615, 33038624) == ("5H10S141M", 33038625)
    assert clip(recs[k + 2], 33038659, 33038668) == ("10S141M5H", 33038669)
