"""The model of the reads -> depth half (tests/readdepth_model.py) and its catalogue of designed reads (tests/readdepth_cases.py) before three judges, and the bit
tricks of baseq_tile_kernel (ngs-bits_amd/csrc/baseq_bits.h) on the CPU, exhaustively. tests/test_gpu_depth_from_reads.py then holds the kernels to the model.

  * the oracle: O.low_high_coverage(random_access=True)["depth"], O.avg_coverage (the only oracle entry with skip_mismapped: per-line sums) and O.read_counts, on every
    case and parameter set the oracle can read - a sorted file (its random access stops at the first record behind a line) without the SEQ "*" record
    (advbam.SEQ_STAR_OOB: the reference reads past the qualities there). The tools merge touching lines; the concatenated depth stays what it was.
  * tests/hand_vectors.py: depths written out by hand from the reference's lines.
  * the premises of the cases: each case still reaches what it was built to reach."""
import subprocess

import numpy as np
import pytest

import advbam as A
import emul_build
import hand_vectors as HV
import hostprep as H
import oracle_lib as O
import readdepth_cases as RC
import readdepth_model as RM

SORTED = [n for n in RC.NAMES if RC.case(n).is_sorted]
COUNT_CASES = ("region_cuts", "cache_moves", "filters")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """per sorted case: (BAM without the SEQ "*" record, BED, the records in it)"""
    d = tmp_path_factory.mktemp("readdepth")
    out = {}
    for name in SORTED:
        c = RC.case(name)
        bam, bed = str(d / (name + ".bam")), str(d / (name + ".bed"))
        recs = c.write(bam, exclude=A.SEQ_STAR_OOB)
        open(bed, "w").write(c.bed())
        out[name] = (bam, bed, recs)
    return out


@pytest.mark.parametrize("name", RC.NAMES)
def test_premise(name):
    c = RC.case(name)
    assert 20 <= len(c.records) <= 5000
    c.premise(c)


@pytest.mark.parametrize("name", SORTED)
def test_model_equals_oracle_depth(files, name):
    c = RC.case(name)
    bam, bed, recs = files[name]
    ob = O.Bam(bam)
    assert ob.count == len(recs)
    n_checked = 0
    for mq, bq, skip in c.params:
        want = RM.depth_from_reads(recs, c.regions, mq, bq, skip)
        if not skip:
            exp = O.low_high_coverage(ob, bed, 1, mq, bq, is_high=False, random_access=True, tool_merge=1)
            assert exp["roi_bases"] == want.size and np.array_equal(exp["depth"], want), (mq, bq)
            n_checked += 1
        elif bq == 0:
            cov, _, _ = O.avg_coverage(ob, bed, merge_bed=False, min_mapq=mq, random_access=True, skip_mismapped=True)
            ends = np.cumsum([e - s + 1 for _, s, e in c.regions])
            assert cov.tolist() == [int(x.sum()) for x in np.split(want.astype(np.int64), ends[:-1])], (mq, "skip_mismapped")
            n_checked += 1
    assert n_checked >= len([p for p in c.params if not p[2]]) > 0


def test_unsorted_case_holds_the_sorted_records():
    a, b = RC.case("cache_moves"), RC.case("cache_moves_unsorted")
    assert sorted(r.bytes() for r in a.records) == sorted(r.bytes() for r in b.records) and a.regions == b.regions
    assert [r.bytes() for r in a.records] != [r.bytes() for r in b.records]
    for mq, bq, skip in a.params:   # (the order of the records is nothing to the model: the oracle's verdict on the sorted file holds for both)
        assert np.array_equal(RM.depth_from_reads(a.records, a.regions, mq, bq, skip), RM.depth_from_reads(b.records, b.regions, mq, bq, skip))


@pytest.mark.parametrize("name", COUNT_CASES)
def test_model_equals_oracle_read_counts(files, name):
    c = RC.case(name)
    bam, bed, recs = files[name]
    tm = H.tid_map(A.REFS)
    for mq in (0, 1, 20):
        exp, text = O.read_counts(O.Bam(bam), bed, mq)
        lines = [(tm[H.chr_num(f[0])], int(f[1]) + 1, int(f[2])) for f in (ln.split("\t") for ln in text.splitlines())]
        assert lines == c.regions                      # (merge(false): touching lines stay apart)
        assert np.array_equal(RM.read_counts(recs, lines, mq), exp), mq
        assert exp.sum() > 0


@pytest.mark.parametrize("name", sorted(HV.CASES))
def test_model_equals_hand_vectors(name):
    hv = HV.CASES[name]
    recs = [RM.record_from_bytes(raw) for raw in HV.READS]
    regions = [(0, s + 1, e) for s, e, _ in hv["bed"]]
    got = RM.depth_from_reads(recs, regions, 1, hv["min_baseq"], False, n_ref=len(HV.REFS))
    assert got.tolist() == hv["depth"]


def test_records_survive_the_byte_form():
    for r in RC.case("cigar_shapes").subset({"cg"}) + RC.case("filters").records:
        back = RM.record_from_bytes(r.bytes())
        assert back.bytes() == r.bytes() and back.cigar == r.cigar and (back.qual == r.qual or not r.seq)


# ---- the bit tricks ----
def test_bit_tricks_exhaustively(tmp_path):
    """tests/emul/baseq_bits_emul.cpp: every byte value against every threshold 1..127 in every byte lane, every `left`, every range [a_lo, b_hi) of 0..256 in every
    word - the header's text compiled by g++, against the obvious loops"""
    p = subprocess.run([emul_build.program("baseq_bits_emul.cpp", tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout + p.stderr
    counts = dict(kv.split("=") for kv in p.stdout.split()[1:])
    assert int(counts["dwords"]) >= 127 * 4 * 256 and int(counts["blocks"]) >= 127 * 65 and int(counts["words"]) >= 257 * 258 // 2
