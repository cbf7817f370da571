"""The adversarial catalogue (tests/advbam.py) on the CPU side: every generated BAM opens in the oracle, the three readers of a record's effective CIGAR
(the oracle's parse_rec, bamfilter_oracle.Rec, variant_oracle.reads) agree on every record, and hand-derived values pin the oracle itself on the nastiest
records. The expected values below are written out by hand from the reference lines cited next to them; nothing here is computed by the code under test."""
import struct

import pytest

import advbam as A
import bamfilter_oracle as F
import oracle_lib as O
import variant_oracle as V

SEEDS = [None, 1, 2, 3]


@pytest.fixture(scope="module", params=SEEDS, ids=lambda s: "catalogue" if s is None else f"seed{s}")
def generated(request, tmp_path_factory):
    cat = A.generate(request.param)
    path = str(tmp_path_factory.mktemp("adv") / "adv.bam")
    recs = cat.write(path, member_sizes=(3000, 5000, 2500))
    return cat, recs, path


def test_opens_in_oracle_with_every_shape(generated):
    cat, recs, path = generated
    b = O.Bam(path)
    assert b.count == len(recs) and b.refs == A.REFS
    assert b.n_blocks > 3   # (members of a few KB: records straddle members)
    raw = cat.header() + b"".join(r.bytes() for r in recs)
    assert b.inflated().tobytes() == raw
    missing = [s for s in A.REQUIRED_SHAPES if cat.shapes.get(s, 0) == 0]
    assert not missing, missing
    for s in ("ops_64", "ops_65", "op_P", "op_N", "seq_star", "qual_ff", "past_end", "cg_applied", "cg_BS", "cg_Bi", "cg_Z", "cg_short", "cg_k_ne_lseq",
              "cg_tid_neg", "cg_pos_neg"):
        assert cat.shapes[s] >= 1, s
    for r in recs:   # (the long-CIGAR classes hold what their names say: LONG_CIGAR = 64 in csrc/common.h)
        for n in (63, 64, 65):
            if f"ops_{n}" in r.shapes:
                assert len(r.cigar) == n


def test_effective_cigar_agrees(generated):
    """the CG rule (htslib bam_tag2cigar as oracle/bamio.hpp parse_rec states it: n_cigar > 0, tid >= 0, pos >= 0, first op kS with k == l_seq, a CG:B,I tag of
    n_cigar <= n < 2^29 entries) read by the oracle, by the BamFilter / BamToFastq restatement and by the getIndels restatement"""
    cat, recs, path = generated
    b = O.Bam(path)
    _, raw = F.read_bam(path)
    vr = V.reads(b)
    assert len(raw) == len(vr) == len(recs)
    for i, r in enumerate(recs):
        exp = [ln << 4 | op for op, ln in r.effective_cigar()]
        assert b.effective_cigar(i) == exp, (r.name, "oracle")
        assert F.Rec(raw[i]).effective_cigar() == exp, (r.name, "bamfilter_oracle")
        assert [n << 4 | op for op, n in vr[i].cigar] == exp, (r.name, "variant_oracle")
        if r.shapes & {"cg_tid_neg", "cg_pos_neg", "cg_BS", "cg_Bi", "cg_Z", "cg_short", "cg_k_ne_lseq"}:
            assert exp == [ln << 4 | op for op, ln in r.cigar]      # not taken from the tag
        if "cg_applied" in r.shapes or "cg_unmapped" in r.shapes:
            assert exp == [ln << 4 | op for op, ln in r.cg[1]]      # taken from the tag (the unmapped flag plays no part in bam_tag2cigar)


# ---- hand-derived values on single records ----
def _bam(tmp_path, *records, name="one.bam"):
    path = str(tmp_path / name)
    A.Catalogue(list(records)).write(path)
    return path


PP = 0x1 | 0x2 | 0x40


def test_hand_P_operation(tmp_path):
    # 12M 3P 12M at 1-based 101 on chr1: P consumes neither read nor reference, so the span is 101..124 (bam_endpos, BamReader.h:91-94).
    # extractBaseByCIGAR (BamReader.cpp:307-374) walks 12M: genome_pos 100 -> 112; a site <= 112 is answered inside the first M (read index site - 101);
    # for a site >= 113 the walk reaches the P operation first and throws "Unknown CIGAR operation!".
    seq = "ACGTACGTACGTTTTTGGGGCCCC"
    r = A.Record("p", PP, A.T1, 100, [(A.M, 12), (A.P, 3), (A.M, 12)], seq, qual=[30] * 24)
    b = O.Bam(_bam(tmp_path, r))
    assert O.site_pileup(b, [(A.T1, 101)], 1, 13).tolist() == [[1, 0, 0, 0, 0, 0]]    # seq[0] = A
    assert O.site_pileup(b, [(A.T1, 112)], 1, 13).tolist() == [[0, 0, 0, 1, 0, 0]]    # seq[11] = T
    with pytest.raises(O.OracleError, match="Unknown CIGAR operation!"):
        O.site_pileup(b, [(A.T1, 113)], 1, 13)
    with pytest.raises(O.OracleError, match="Unknown CIGAR operation!"):
        O.site_pileup(b, [(A.T1, 124)], 1, 13)
    assert O.site_pileup(b, [(A.T1, 125)], 1, 13).tolist() == [[0] * 6]               # behind the span: not in the region query
    cov, _, _ = O.avg_coverage(b, _bed(tmp_path, "chr1\t100\t130\n"), random_access=True)
    assert cov.tolist() == [24]                                                        # bases 101..124


def _bed(tmp_path, text, name="r.bed"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_hand_zero_length_ops(tmp_path):
    # 0M 10M 0I 0D 10M 0N 0S at 1-based 101: zero-length operations add nothing, the span is 101..120. qlen = 20 = l_seq (bam_read1 accepts it).
    r = A.Record("z", PP, A.T1, 100, [(A.M, 0), (A.M, 10), (A.I, 0), (A.D, 0), (A.M, 10), (A.N, 0), (A.S, 0)], "A" * 20, qual=[30] * 20)
    b = O.Bam(_bam(tmp_path, r))
    cov, _, _ = O.avg_coverage(b, _bed(tmp_path, "chr1\t100\t130\n"), random_access=True)
    assert cov.tolist() == [20]
    n, _ = O.read_counts(b, _bed(tmp_path, "chr1\t119\t120\nchr1\t120\t130\n"), 1)   # 1-based [120,120] overlaps, [121,130] does not
    assert n.tolist() == [1, 0]
    # the site right behind the 0D: extractBaseByCIGAR returns '-' only when genome_pos >= pos after a D; a 0D leaves genome_pos at 110 < 111
    assert O.site_pileup(b, [(A.T1, 111)], 1, 13).tolist() == [[1, 0, 0, 0, 0, 0]]


def test_hand_seq_star(tmp_path):
    # SEQ "*" (l_seq = 0), 30M at 1-based 101, proper pair read 1, TLEN 0, MAPQ 60 on chr1 (not special):
    # Statistics::mapping(bam) (Statistics.cpp:830-916): al_total 1, al_mapped 1, bases_mapped += length() = 0, al_ontarget 1, bases_usable += 0;
    # proper pair, |isize| = 0 < 1000: insert_size_read_count 1, histogram bin 0; max_length 0.
    r = A.Record("s", PP, A.T1, 100, [(A.M, 30)], "", isize=0)
    b = O.Bam(_bam(tmp_path, r))
    m = O.mapping(b, O.MODE_NOROI)
    assert (m["al_total"], m["al_mapped"], m["al_ontarget"], m["bases_mapped"], m["bases_usable"], m["max_length"]) == (1, 1, 1, 0, 0, 0)
    assert (m["insert_size_read_count"], m["insert_size_sum"], int(m.insert_hist[0])) == (1, 0, 1)
    # the span comes from the CIGAR alone: depth 1 on 101..130 (min_baseq 0: qualities() is not asked)
    lh = O.low_high_coverage(b, _bed(tmp_path, "chr1\t95\t135\n"), 1, random_access=True, tool_merge=0)
    assert lh["depth"].tolist() == [0] * 5 + [1] * 30 + [0] * 5
    # StatisticsReads::update: cycles 0, no base, mean quality 0 / 0 = NaN is skipped (StatisticsReads.cpp:118-158)
    q = O.reads_qc(b)
    assert (q["c_forward"], q["bases_sequenced"], q["max_cycles"], int(q["read_qualities"].sum()), q["c_read_q20"]) == (1, 0, 0, 0, 0)


def test_hand_qual_ff(tmp_path):
    # QUAL 0xff: BamAlignment::qualities gives 255 per base. StatisticsReads::update throws at q >= 100 ("Base quality > 100 (255)...",
    # StatisticsReads.cpp:133-135); getPileup counts a base whose quality 255 >= min_baseq, even at min_baseq 255 (BamReader.cpp:866-870).
    r = A.Record("q", PP, A.T1, 100, [(A.M, 4)], "ACGT", qual=None)
    b = O.Bam(_bam(tmp_path, r))
    with pytest.raises(O.OracleError, match="Base quality > 100"):
        O.reads_qc(b)
    assert O.site_pileup(b, [(A.T1, 103)], 1, 255).tolist() == [[0, 0, 1, 0, 0, 0]]


def test_hand_read_past_contig_end(tmp_path):
    # chr3 has 300 bases; 25M at 1-based 300 spans 300..324 (bam_endpos does not look at the contig length).
    r = A.Record("e", PP, A.TSHORT, 299, [(A.M, 25)], "C" * 25, qual=[30] * 25)
    b = O.Bam(_bam(tmp_path, r))
    cov, _, _ = O.avg_coverage(b, _bed(tmp_path, "chr3\t294\t330\n"), random_access=True)   # a line past the contig end: [295, 330] overlaps 300..324
    assert cov.tolist() == [25]
    # the sweep keeps a depth array of contig length + 1 and stops at max_pos = 300 (WorkerLowOrHighCoverage.cpp:160-200): 1 at 300, 0 behind it
    lh = O.low_high_coverage(b, _bed(tmp_path, "chr3\t297\t303\n"), 1, random_access=False, tool_merge=0)
    assert lh["depth"].tolist() == [0, 0, 1, 0, 0, 0]
    n, _ = O.read_counts(b, _bed(tmp_path, "chr3\t320\t400\n"), 1)
    assert n.tolist() == [1]


CG_OPS = [(A.S, 2), (A.M, 10), (A.I, 2), (A.M, 6), (A.D, 3), (A.M, 10), (A.N, 40), (A.M, 5)]   # qlen 35, rlen 74


@pytest.mark.parametrize("case,tid,pos,first,tag,taken", [
    ("B,I", 0, 100, None, A._cg(CG_OPS), True),
    ("B,S", 0, 100, None, A._cg(CG_OPS, "BS"), False),            # not of type B,I
    ("B,i", 0, 100, None, A._cg(CG_OPS, "Bi"), False),            # (the oracle takes B,I only)
    ("Z", 0, 100, None, A._cg(CG_OPS, "Z"), False),
    ("fewer entries", 0, 100, None, A._cg(CG_OPS[:1]), False),    # 1 < n_cigar = 2
    ("k != l_seq", 0, 100, 34, A._cg(CG_OPS), False),             # first op 34S 1M: k != l_seq
    ("tid -1", -1, 100, None, A._cg(CG_OPS), False),
    ("pos -1", 0, -1, None, A._cg(CG_OPS), False),
], ids=["BI", "BS", "Bi", "Z", "fewer_entries", "k_ne_lseq", "tid_neg", "pos_neg"])
def test_hand_cg_edges(tmp_path, case, tid, pos, first, tag, taken):
    # htslib bam_tag2cigar as oracle/bamio.hpp parse_rec states it: n_cigar > 0 && tid >= 0 && pos >= 0, first op kS with k == l_seq, CG:B,I with
    # n_cigar <= n < 2^29 entries. Taken: the span is the tag's, 74 bases (10 + 6 + 3 + 10 + 40 + 5); not taken: the placeholder 35S 74N spans the same 74
    # bases (htslib writes it so), 34S 1M one base.
    cig = [(A.S, 35), (A.N, 74)] if first is None else [(A.S, first), (A.M, 35 - first)]
    r = A.Record("cg", PP, tid, pos, cig, "A" * 35, qual=[30] * 35, aux=tag)
    path = _bam(tmp_path, r)
    b = O.Bam(path)
    want = CG_OPS if taken else cig
    assert b.effective_cigar(0) == [ln << 4 | op for op, ln in want]
    _, raw = F.read_bam(path)
    g = F.Rec(raw[0]).effective_cigar()
    assert g == [ln << 4 | op for op, ln in want]
    if tid >= 0 and pos >= 0:
        cov, _, _ = O.avg_coverage(b, _bed(tmp_path, "chr1\t100\t110\n"), random_access=True)
        assert cov.tolist() == [1 if first else 10]   # (bases 101..110 of the span; 34S 1M: 101 alone)
    # BamFilter's alignment filter counts the gaps of the effective CIGAR (src/BamFilter/main.cpp): 2 (I, D) from the tag, none from the placeholder
    assert sum(1 for c in g if c & 15 in (1, 2)) == (2 if taken else 0)
