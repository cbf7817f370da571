"""The model of MappingQC's record loops (tests/mapping_model.py) and its designed reads (tests/mapping_cases.py) before four judges; tests/test_gpu_mapping_designed.py
then holds the kernels to the model.

  * the oracle: oracle_lib.mapping on every case file in the three modes for min_mapq 1 and advbam.MIN_MAPQ, GC bins from the case's sparse FASTA - every integer equal,
    gc_reads within the project's rtol = 1e-12 of the model's fractions; the same on the adversarial catalogue (hand-ordered and one seed).
  * the premises of the cases: each case still reaches what it was built to reach.
  * the variants of the model (mapping_model.VARIANTS), each wrong by one in one comparison or constant: the designed set tells every one of them from the model.
    The test prints which cases caught which variant - the evidence that the set would catch a kernel that is wrong in the same way.
  * hand vectors: four reads whose counters are worked out below."""
import os
from fractions import Fraction

import numpy as np
import pytest

import advbam as A
import hostprep as H
import mapping_cases as MC
import mapping_model as MM
import oracle_lib as O

MODES = MC.MODES
SKIP_COUNTERS = {"half_depth", "bases_covered_half"}
# the ROI of tests/test_gpu_adversarial.py: inside the contigs, touching lines, a one-base contig
CATALOGUE_BED = "chr1\t0\t2000\nchr1\t2000\t2600\nchr1\t5000\t5001\nchr1\t8000\t29000\nchrX\t0\t9000\nchrY\t100\t4000\nchr2\t0\t1\nchr3\t10\t300\nchrMT\t0\t700\n"


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("mapping"))


def assert_equals_oracle(got, exp, what):
    for name in O.COUNTER_NAMES:
        if name not in SKIP_COUNTERS:
            assert got[name] == exp[name], (what, name, got[name], exp[name])
    assert list(got.hist) == exp.insert_hist.tolist(), (what, "insert-size histogram")
    assert np.array_equal(got.depth, exp.depth), (what, "per-base depth")
    if exp["roi_bases"]:
        assert (got.half_depth, got.bases_covered_half) == (exp["half_depth"], exp["bases_covered_half"]), what
    if exp.have_gc:
        have = np.zeros(MM.N_BINS); have[:exp.gc_reads.size] = exp.gc_reads
        assert np.allclose(have, [float(x) for x in got.gc_reads], rtol=1e-12, atol=0.0), (what, "gc_reads")


def test_counter_names():
    assert set(MM.COUNTERS) == set(O.COUNTER_NAMES) - SKIP_COUNTERS


@pytest.mark.parametrize("name", MC.NAMES)
def test_premise(name):
    c = MC.case(name)
    assert 20 <= len(c.records) <= 800
    c.premise(c)


@pytest.mark.parametrize("name", MC.NAMES)
def test_model_equals_oracle(workdir, name):
    c = MC.case(name)
    bam = os.path.join(workdir, name + ".bam")
    c.write(bam)
    bed, fasta = c.files(workdir)
    ob = O.Bam(bam)
    assert ob.count == len(c.records)
    fed = 0
    for mode in MODES:
        roi = mode != MM.MODE_NOROI
        bins = c.fasta_bins(mode, workdir) if roi else None
        for mq in (1, A.MIN_MAPQ):
            exp = O.mapping(ob, mode, bed if roi else None, merge_bed=c.merge and mode == MM.MODE_ROI, fasta=fasta if roi else None, min_mapq=mq)
            got = c.run(mode, mq, bins=bins)
            assert_equals_oracle(got, exp, (name, mode, mq))
            assert got["roi_bases"] == (sum(e - s + 1 for _, s, e in c.tables(mode)[0]) if roi else 0)
            fed += sum(1 for x in got.gc_reads if x) + int(got.depth.sum())
    assert fed > 0


@pytest.mark.parametrize("seed", [None, 1], ids=["catalogue", "seed1"])
def test_model_equals_oracle_on_the_catalogue(workdir, seed):
    cat = A.generate(seed)
    bam, bed = os.path.join(workdir, "adv%s.bam" % seed), os.path.join(workdir, "adv.bed")
    cat.write(bam)
    open(bed, "w").write(CATALOGUE_BED)
    fasta = H.sparse_fasta_for(bed, A.REFS, os.path.join(workdir, "adv.fa"), seed=5)
    ob = O.Bam(bam)
    tx, ty = H.xy_tids(A.REFS)
    for mode, merge in ((MM.MODE_ROI, 1), (MM.MODE_NOROI, 0), (MM.MODE_WGS, 3)):
        regs, chunks, bins = [], [], []
        if mode != MM.MODE_NOROI:
            regs, _ = H.bed_regions(bed, A.REFS, merge)
            chunks, bins = H.gc_inputs(bed, A.REFS, fasta, merge)
        for mq in (1, A.MIN_MAPQ):
            exp = O.mapping(ob, mode, bed if regs else None, merge_bed=(merge == 1), fasta=fasta if regs else None, min_mapq=mq)
            got = MM.mapping(cat.records, mode, regs, chunks, bins, min_mapq=mq, tid_x=tx, tid_y=ty, nonspecial=H.nonspecial(A.REFS))
            assert_equals_oracle(got, exp, (seed, mode, mq))


def test_every_variant_is_caught(workdir):
    """every off-by-one variant of the model changes a compared output (a counter, an insert-size bin, the depth, gc_reads, the half-depth pair) on the designed set"""
    runs = []    # (case, mode, min_mapq, yx, bins, the model's outputs)
    for name in MC.NAMES:
        c = MC.case(name)
        for mode in MODES:
            sets = [None] if mode == MM.MODE_NOROI else [c.fasta_bins(mode, workdir)] + ([c.bins(mode)[1]] if c.hand_bins else [])
            for bins in sets:
                for mq, yx in c.params:
                    runs.append((c, mode, mq, yx, bins, c.run(mode, mq, yx, bins=bins).outputs()))
    caught = {}
    for vname, rules in MM.VARIANTS.items():
        caught[vname] = sorted({c.name for c, mode, mq, yx, bins, ref in runs if c.run(mode, mq, yx, bins=bins, rules=rules).outputs() != ref})
    print()
    for vname, names in caught.items():
        print("variant %-22s caught by: %s" % (vname, ", ".join(names) or "NOTHING"))
    assert all(caught.values()), [v for v, n in caught.items() if not n]
    # each variant is caught where it was aimed at
    aimed = {"near": "near_window", "on": "near_window", "ovl": "overlap_window", "gc": "gc_counts", "wgs": "region_cuts", "hist": "insert_sizes", "x": "sex_contigs",
             "dp": "region_cuts"}
    for vname, names in caught.items():
        assert aimed[vname.split("_")[0]] in names, (vname, names)


# ---- hand vectors ----
# Regions [101, 200] and [301, 400] of chr1, each one GC chunk, bins 10 and 20; min_mapq 20. Four reads in file order:
#   r1  flag 0x43 (paired, proper, read 1)  [150, 249] 100M             isize  150  MAPQ 60  DP 2
#   r3  flag 0x93 (paired, proper, read 2)  [190, 309] 10S 120M         isize -150  MAPQ 19           l_seq 130
#   r2  flag 0                              [451, 500] 50M                          MAPQ 60
#   r4  flag 0x400 (duplicate)              [651, 700] 50M                          MAPQ 60
# Every loop: al_total 4, al_mapped 4, al_dup 1 (r4), al_proper_paired 2, bases_mapped 100 + 130 + 50 + 50 = 330, bases_clipped 10 (r3), max_length 130, paired_end 1.
#   insert sizes: r1 and r3, both 150 -> count 2, sum 300, bin 150 = 2. Trimmed: the running maximum is 100, 130, 130, 130 -> 0 + 0 + 80 + 80 = 160.
# Target-region loop:
#   near: r1 (on), r3 (on), r2 (451 - 250 = 201 <= 400) -> 3; r4: 651 - 250 = 401 > 400 -> not near. On target: r1, r3 -> 2.
#   r1: DP 2 -> dp_dist bin of 2 (the second) = 1. Usable: overlap with [101, 200] is [150, 200] = 51 bases -> bases_usable 51, bases_usable_dp2 51,
#       bases_usable_raw 51 * 3 = 153, depth 1 on 150..200. Overlap with its mate: 2 * 100 - 150 = 50 bases from 150 + 100 - 50 = 200 to 249; of these, position 200
#       lies on the target -> bases_usable_no_overlap 51 - 1 = 50. GC: one chunk -> gc_reads[10] += 1.
#   r3: MAPQ 19 < 20: not usable. GC: both chunks -> gc_reads[10] += 1/2, gc_reads[20] += 1/2.
#   gc_reads[10] = 3/2, gc_reads[20] = 1/2. half_depth = round(0.5 * 51 / 200) = 0 -> all 200 bases are covered at least half.
# Whole-genome loop (chr1 is not special): al_ontarget 4. Usable: r1 100 + r2 50 = 150, minus 10 clipped = 140. No overlap: 100 (r1; a paired read was seen) + 50 (r2)
#   - 50 (r1 is read 1, 2 * 100 - 150) = 100. The indexed passes: region 1 meets r1 and r3, region 2 meets r3 -> gc_reads[10] = 1 + 1/2 + 1/2 = 2, gc_reads[20] = 1/2 + 1/2 = 1;
#   bases_usable_roi = 100 (r1), depth 1 on 150..200. half_depth = round(0.5 * 100 / 200) = 0.
HAND_REGIONS = [(A.T1, 101, 200), (A.T1, 301, 400)]
HAND_COMMON = dict(al_total=4, al_mapped=4, al_dup=1, al_proper_paired=2, bases_mapped=330, bases_clipped=10, max_length=130, paired_end=1, insert_size_read_count=2,
                   insert_size_sum=300, bases_trimmed=160, reads_x=0, reads_y=0, yx_valid=0)
HAND_ROI = dict(HAND_COMMON, al_neartarget=3, al_ontarget=2, dp_dist1=1, bases_usable=51, bases_usable_dp2=51, bases_usable_raw=153, bases_usable_no_overlap=50, roi_bases=200)
HAND_WGS = dict(HAND_COMMON, al_ontarget=4, bases_usable=140, bases_usable_no_overlap=100, bases_usable_roi=100, roi_bases=200)
HAND_NOROI = dict(HAND_COMMON, al_ontarget=4, bases_usable=140, bases_usable_no_overlap=100)


def hand_reads():
    return [MC.rec("r1", 149, [(A.M, 100)], flag=0x43, isize=150, dp=2), MC.rec("r3", 189, [(A.S, 10), (A.M, 120)], flag=0x93, isize=-150, mapq=19),
            MC.rec("r2", 450, [(A.M, 50)]), MC.rec("r4", 650, [(A.M, 50)], flag=0x400)]


@pytest.mark.parametrize("mode,want,gc10,gc20", [(MM.MODE_ROI, HAND_ROI, Fraction(3, 2), Fraction(1, 2)), (MM.MODE_WGS, HAND_WGS, Fraction(2), Fraction(1)),
                                                 (MM.MODE_NOROI, HAND_NOROI, Fraction(0), Fraction(0))], ids=["roi", "wgs", "noroi"])
def test_hand_vectors(mode, want, gc10, gc20):
    tx, ty = H.xy_tids(A.REFS)
    got = MM.mapping(hand_reads(), mode, HAND_REGIONS, HAND_REGIONS, [10, 20], min_mapq=20, tid_x=tx, tid_y=ty, nonspecial=H.nonspecial(A.REFS))
    assert {n: got[n] for n in MM.COUNTERS} == {n: want.get(n, 0) for n in MM.COUNTERS}
    assert [i for i, v in enumerate(got.hist) if v] == [150] and got.hist[150] == 2
    gc = [Fraction(0)] * MM.N_BINS
    gc[10], gc[20] = gc10, gc20
    assert got.gc_reads == gc
    if mode == MM.MODE_NOROI:
        assert got.depth.size == 0
    else:
        depth = np.zeros(200, dtype=np.int32); depth[49:100] = 1
        assert np.array_equal(got.depth, depth) and (got.half_depth, got.bases_covered_half) == (0, 200)
