"""The two models of tests/readprofile.py against the oracle, and the premises of the designed files of tests/readprofile_cases.py (CPU only): before the
GPU kernels are compared with reads_model / carry_model, the models must equal the oracle's restatement of the reference on every designed file the oracle
accepts and on the fixture BAMs, and every file must really sit on the boundary it is named after."""
import os
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib as O
import readprofile as RP
import readprofile_cases as RC
from conftest import GOLDEN_IN as GI

FIXTURES = ["MappingQC_in1.bam", "MappingQC_in3.bam", "MappingQC_in5.bam", "BamReader_rna.bam", "BamReader_lr.bam", "Statistics_longread.bam",
            "BamReader_insert_only.bam", "sry.bam"]                        # the files of test_gpu_reads.py


@pytest.fixture(scope="module")
def reads_files():
    return RC.reads_files()


@pytest.fixture(scope="module")
def prefix_files():
    return RC.prefix_files()


def _oracle_bam(tmp_path, records, sizes=None):
    return O.Bam(RP.write(str(tmp_path / "f.bam"), records, sizes or (60000,)))


def _records_of(ob):
    """the record list of a BAM the oracle has loaded, in columnar form"""
    raw, offs = ob.inflated(), ob.record_offsets()
    flags, lens, bases, quals = [], [], [], []
    for o in offs.tolist():
        core = raw[o + 4:o + 36]
        l_name, n_cig, flag, l_seq = int(core[8]), int(core[12]) | int(core[13]) << 8, int(core[14]) | int(core[15]) << 8, int(core[16:20].view("<i4")[0])
        s = o + 36 + l_name + 4 * n_cig
        packed = raw[s:s + (l_seq + 1) // 2]
        bases.append(np.stack([packed >> 4, packed & 15], axis=1).reshape(-1)[:l_seq]); quals.append(raw[s + (l_seq + 1) // 2:s + (l_seq + 1) // 2 + l_seq])
        flags.append(flag); lens.append(l_seq)
    cat = lambda x: np.concatenate(x) if x else np.zeros(0, dtype=np.uint8)
    return RP.Columns(np.array(flags, dtype=np.int64), np.array(lens, dtype=np.int64), cat(bases), cat(quals), np.full(len(flags), 60))


# ---- reads_model == oracle ----
@pytest.mark.parametrize("single_end", [False, True])
@pytest.mark.parametrize("name", list(RC.reads_files()))
def test_reads_model_equals_oracle_on_designed_files(tmp_path, reads_files, name, single_end):
    records, sizes = reads_files[name]
    exp = O.reads_qc(_oracle_bam(tmp_path, records, sizes), single_end)
    got = RP.reads_model(records, single_end)
    assert got["n_unknown_base"] == 0 and got["n_quality_out_of_range"] == 0
    assert set(exp) <= set(got)                                              # every key the oracle reports is compared
    RP.assert_reads_equal(exp, got, what=name)


@pytest.mark.parametrize("single_end", [False, True])
@pytest.mark.parametrize("bam", FIXTURES)
def test_reads_model_equals_oracle_on_fixture_bams(bam, single_end):
    ob = O.Bam(os.path.join(GI, bam))
    exp, got = O.reads_qc(ob, single_end), RP.reads_model(_records_of(ob), single_end)
    assert set(exp) <= set(got)
    RP.assert_reads_equal(exp, got, what=bam)


def test_builder_writes_what_it_was_given(tmp_path):
    """every nibble and every quality byte, odd and even lengths, a record without bases: read back through the oracle's BAM reader"""
    rng = np.random.default_rng(3)
    recs = [(int(rng.integers(0, 1 << 12)) & ~0x2, rng.integers(0, 16, ln).astype(np.uint8), rng.integers(0, 256, ln).astype(np.uint8), int(rng.integers(0, 61)))
            for ln in (0, 1, 2, 3, 64, 65, 0, 321, 1000, 7)]
    ob = _oracle_bam(tmp_path, recs, (100, 333))
    assert ob.count == len(recs) and ob.refs == [("chr1", RP.REF_LEN)]
    back, want = _records_of(ob), RP.columns(recs)
    for a, b in zip(back[:4], want[:4]):
        assert np.array_equal(a, b)
    raw, offs = ob.inflated(), ob.record_offsets()
    pos = [int(raw[o + 8:o + 12].view("<i4")[0]) for o in offs]
    assert pos == sorted(pos) and len(set(pos)) == len(pos)
    assert [int(raw[o + 13]) for o in offs] == [r[3] for r in recs]         # MAPQ
    names = {bytes(raw[o + 36:o + 36 + int(raw[o + 12])]) for o in offs}
    assert len(names) == len(recs)


# ---- premises of the read-QC files ----
def test_ladder_closed_forms():
    """per-cycle counts and quality sums of the first 320 cycles, the totals with the tails, bases_sequenced and max_cycles from the formulas alone"""
    for lengths, per in ((RC.LADDER, 4), ((63,), 6), ((64,), 6), ((320,), 6), ((321,), 6)):
        recs = RC.ladder(lengths, per)
        assert sorted({len(r[1]) for r in recs}) == sorted(lengths)         # the lengths present: the whole pass sees only these
        assert {r[0] for r in recs} == {RC.R1, RC.R2}
        RP.assert_reads_equal(RC.ladder_closed_form(lengths, per), RP.reads_model(recs, False), what=str(lengths))
    m = RP.reads_model(RC.ladder(), False)
    assert m["read_lengths"][0] == 4 and m["read_lengths"].sum() == 4 * len(RC.LADDER)


def test_zero_length_reads_count_as_reads_only():
    """a zero-length read adds to c_forward / c_reverse and read_lengths[0], to nothing else"""
    z = np.zeros(0, dtype=np.uint8)
    m = RP.reads_model([(RC.R1, z, z), (RC.R2, z, z), (RC.R2, z, z)], False)
    assert (m["c_forward"], m["c_reverse"], m["max_cycles"]) == (1, 2, 0) and m["read_lengths"].tolist() == [3]
    assert all(int(np.sum(m[k])) == 0 for k in m if k not in ("c_forward", "c_reverse", "read_lengths"))


def test_means_sit_on_their_edges():
    recs, notes = RC.means()
    half = [o for o, (s, n) in notes.items() if Fraction(s, n).denominator == 2]
    assert len(half) == 2 * (99 + 6)                                         # the (q, q + 1) pairs and the 64-cycle reads, both directions
    for o in half:
        s, n = notes[o]; k = s // n
        one = RP.reads_model([recs[o]], False)
        assert Fraction(s, n) == k + Fraction(1, 2)
        assert one["read_qualities"][k + 1] == 1                             # half away from zero
        assert (one["qscore_dist_r1"] + one["qscore_dist_r2"])[min(k, 59)] == 1
    sums = {(s, n) for s, n in notes.values()}
    assert {(64 * k + 32, 64) for k in (0, 19, 58, 59, 60, 98)} <= sums and {(321 * k + 160, 321) for k in (0, 19, 58, 59, 60, 98)} <= sums
    assert {(7 * k, 7) for k in (0, 20, 59, 60, 61, 99)} <= sums and (59999, 1000) in sums
    m = RP.reads_model(recs, False)
    assert m["c_forward"] == m["c_reverse"] and np.array_equal(m["qscore_dist_r1"], m["qscore_dist_r2"]) and m["qscore_dist_r1"][59] > 40


def test_run_and_growth_premises():
    ln = lambda recs: [len(r[1]) for r in recs]
    assert set(ln(RC.runs_equal())) == {100}
    a = ln(RC.runs_alternating()); assert all(x != y for x, y in zip(a, a[1:])) and set(a) == {37, 91}
    c = ln(RC.runs_increasing()); assert all(y == x + 1 for x, y in zip(c, c[1:]))
    recs, sizes = RC.runs_growing()
    raw, off = RP.build_raw(recs)
    cuts = np.cumsum(sizes)
    assert cuts[-1] == len(raw) and all(int(c_) in set(off.tolist()) for c_ in cuts[:-1])          # every member ends where a record ends
    per_member = [sorted({len(recs[k][1]) for k in range(len(recs)) if lo <= off[k] < hi}) for lo, hi in zip([0] + cuts.tolist(), cuts.tolist())]
    assert per_member == [[s] for s, _ in RC.GROW_STEPS]
    cap, branches = -1, []
    for need, _ in RC.GROW_STEPS:                                            # ReadsState::tile: need > len_cap -> max(need, 2 len_cap)
        assert need > cap
        branches.append(cap >= 0 and need <= 2 * cap); cap = max(need, need if cap < 0 else 2 * cap)
    assert branches.count(True) >= 1 and branches[1:].count(False) >= 1
    e = ln(RC.runs_longest_last()); assert e[-1] == max(e) and e.count(max(e)) == 1


def test_flag_premises():
    recs = RC.flag_combinations()
    assert len({r[0] for r in recs}) == 128
    for bit, recs in ((0x100, RC.longest_is(0x100)), (0x800, RC.longest_is(0x800))):
        longest = max(recs, key=lambda r: len(r[1]))
        assert longest[0] & bit and len(longest[1]) == 500
        m = RP.reads_model(recs, False)
        assert m["max_cycles"] == 100 and len(m["read_lengths"]) == 101
    m = RP.reads_model(RC.only_secondary(), True)
    assert m["max_cycles"] == 0 and all(int(np.sum(v)) == 0 for v in m.values())


# ---- files the oracle rejects ----
def test_oracle_rejects_unknown_bases_and_qualities(tmp_path):
    recs, n_bad = RC.unknown_bases()
    assert n_bad == 11 * 6 + 1 and RP.reads_model(recs, False)["n_unknown_base"] == n_bad
    with pytest.raises(O.OracleError, match=r"Unknown base '0' in StatisticsReads::update!"):
        O.reads_qc(_oracle_bam(tmp_path, recs))
    recs, n_bad = RC.bad_qualities()
    assert n_bad == 2 * 6 + 1 and RP.reads_model(recs, False)["n_quality_out_of_range"] == n_bad
    with pytest.raises(O.OracleError, match=r"Base quality > 100 \(100\)\. This should not happen!"):
        O.reads_qc(_oracle_bam(tmp_path, recs))
    for v in RP.UNKNOWN:                                                     # each nibble on its own is rejected, at the last (half-byte) cycle too
        f, b, q = RC._rec(RC.R1, RC.ERR_LEN, 0); b = b.copy(); b[-1] = v
        with pytest.raises(O.OracleError, match=rf"Unknown base '{v}'"):
            O.reads_qc(_oracle_bam(tmp_path, [(f, b, q)]))


# ---- carry_model == oracle, premises of the fix-up files ----
def _carry_vs_oracle(tmp_path, cols, **kw):
    exp = O.mapping(O.Bam(RP.write(str(tmp_path / "c.bam"), cols, **kw)), O.MODE_NOROI)
    got = RP.carry_model(cols)
    for idx, key in RP.CARRY_COUNTERS:
        assert int(exp.counters[idx]) == got[key], (O.COUNTER_NAMES[idx], int(exp.counters[idx]), got[key])
    return got


def _firsts(cols):
    """(ordinal of the first record of the file's maximum length, ordinal of the first paired record) among the counted records"""
    rows = RP.carry_rows(cols)
    counted = rows[:, 1] == 1
    gmax = int(rows[counted, 0].max())
    full = np.flatnonzero(counted & (rows[:, 0] == gmax)); paired = np.flatnonzero(rows[:, 3] == 1)
    return gmax, int(full[0]), (int(paired[0]) if paired.size else None)


@pytest.mark.parametrize("name", list(RC.prefix_files()))
def test_carry_model_equals_oracle_on_fix_up_files(tmp_path, prefix_files, name):
    cols = prefix_files[name]
    got = _carry_vs_oracle(tmp_path, cols)
    assert got["gmax"] == RC.FULL and got["trimmed"] > 0 and int(cols.lens.max()) <= RC.FULL + 1


def test_first_full_and_first_paired_are_where_the_names_say(prefix_files):
    for f in RC.FIRST_FULL:
        assert _firsts(prefix_files[f"first_full_{f}"]) == (RC.FULL, f, 2)
    for f, p in RC.FULL_PAIRED:
        cols = prefix_files[f"full_{f}_paired_{p}"]
        assert _firsts(cols) == (RC.FULL, f, p)
        rows = RP.carry_rows(cols)
        runmax = np.maximum.accumulate(np.where(rows[:, 1] == 1, rows[:, 0], 0))
        if f >= 1024:                                                        # the running maximum changes inside the blocks, not only at their edges
            changes = np.flatnonzero(np.diff(runmax[:f]) > 0) + 1
            assert (changes % 256 != 0).sum() >= 10
    orders = {(f > 4096, (p or 10 ** 9) > 4096, f < (p or 10 ** 9)) for f, p in RC.FULL_PAIRED if p is not None and p != f}
    assert {(False, False, True), (False, False, False), (True, True, True), (True, False, False)} <= orders


def test_quiet_records_do_not_move_the_maximum(prefix_files):
    for name, (f, at_151, edges) in RC.QUIET.items():
        cols, without = RC.quiet_records(f, at_151, edges)
        assert all(int(cols.lens[o]) == 151 and int(cols.flags[o]) & 0x900 for o in at_151)
        a, b = RP.carry_model(cols), RP.carry_model(without)
        assert a == b and a["gmax"] == 150 and _firsts(cols)[1] == f
        rows = RP.carry_rows(cols)
        runmax = np.maximum.accumulate(np.where(rows[:, 1] == 1, rows[:, 0], 0))
        for e in edges:
            for o in (e - 1, e, e + 1):                                      # counted for the maximum (it rises there), not passing for the length sum
                assert rows[o, 1] == 1 and rows[o, 2] == 0 and runmax[o] == rows[o, 0] > runmax[o - 1]
            kinds = {(int(cols.flags[o]) & 0x404, int(cols.mapq[o])) for o in (e - 1, e, e + 1)}
            assert kinds == {(0x400, 60), (0x4, 60), (0, 0)}                 # one duplicate, one unmapped, one MAPQ-0 record on EVERY edge


def test_stairs_step_where_they_should(tmp_path):
    for kind, period in (("steps_256", 256), ("steps_1024", 1024)):
        cols = RC.stairs(kind); _carry_vs_oracle(tmp_path, cols)
        gmax, f, p = _firsts(cols)
        runmax = np.maximum.accumulate(RP.carry_rows(cols)[:, 0])
        changes = np.flatnonzero(np.diff(runmax[:f]) > 0) + 1
        assert changes.tolist() == list(range(period, f, period)) and (gmax, p) == (150, 5000)
    cols = RC.stairs("mid_block")
    gmax, f, p = _firsts(cols)
    runmax = np.maximum.accumulate(RP.carry_rows(cols)[:, 0])
    for b in range(1, f // 1024):                                            # block seed != block maximum, in every whole block in front of f
        assert runmax[1024 * b - 1] < runmax[1024 * (b + 1) - 1] and runmax[1024 * b] == runmax[1024 * b - 1]


def test_two_step_file(tmp_path):
    cols = RC.two_steps()
    got = _carry_vs_oracle(tmp_path, cols)
    rows = RP.carry_rows(cols)
    assert got["gmax"] == 200 and _firsts(cols)[1] == RC.TWO_STEP_F2
    assert int(np.flatnonzero((rows[:, 1] == 1) & (rows[:, 0] == 150))[0]) == RC.TWO_STEP_F
    sizes, k, n_first = RC.two_tile_layout(cols)
    assert RC.TWO_STEP_F + 64 < n_first and n_first + 4096 + 64 < RC.TWO_STEP_F2   # both tiles take the three-kernel form, the second with a carry of 150
    # the carry must matter: whichever record near the split the second tile begins with (a record that straddles the cut belongs to one of the two), the
    # running maxima over its prefix differ between a seed of 150 and a seed of 0 - by more than four blocks of 1024 records
    assert RC.TWO_STEP_SHORT + 64 < n_first
    for start in (n_first - 1, n_first, n_first + 1):
        prefix = rows[start:RC.TWO_STEP_F2].tolist()
        assert max(r[0] for r in prefix if r[1]) < 150
        with_carry, without = RP.sequential([[150, 1, 0, 0]] + prefix), RP.sequential([[0, 1, 0, 0]] + prefix)
        assert with_carry["trimmed"] - without["trimmed"] > 4096 * 50, (with_carry["trimmed"], without["trimmed"])


def test_many_blocks_file(tmp_path):
    cols = RC.many_blocks()
    _carry_vs_oracle(tmp_path, cols, level=1)
    assert _firsts(cols) == (30, RC.BIG_F, RC.BIG_P) and int(cols.lens.min()) == 1
    assert -(-RC.BIG_F // 1024) > 256                                        # more blocks than one trip of the seed kernel takes
    rows = RP.carry_rows(cols)
    runmax = np.maximum.accumulate(np.where(rows[:, 1] == 1, rows[:, 0], 0))
    assert runmax[256 * 1024 - 1] == 27 and runmax[257 * 1024 - 1] == 29 and runmax[RC.BIG_F - 1] == 29   # the maximum still rises behind the first trip
