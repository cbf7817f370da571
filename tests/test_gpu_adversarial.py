"""The record kernels against the oracle on the adversarial catalogue (tests/advbam.py): three seeds plus the hand-ordered catalogue, every comparison exact,
under each of the library's path switches (README: NGSQC_TILE_MEMBERS with members of about 3 KB, NGSQC_NO_FUSED_SCAN, NGSQC_K2_GENERAL, NGSQC_BASEQ_RIDE=0,
NGSQC_NO_FUSED_PILEUP, NGSQC_LONG_READ_MODE) and, for the mapping and depth scans, over 3 local shards."""
import gzip
import os

import numpy as np
import pytest

import advbam as A
import bamfilter_oracle as F
import bamtofastq_oracle as Q
import hostprep as H
import oracle_lib as O
import variant_oracle as V
from test_gpu_variant_freq import HashGenome, _events, _windows

pytestmark = pytest.mark.gpu
ngsqc = __import__("importlib").import_module("ngs-bits_amd")

FILES = [None, 1, 2, 3]
SWITCHES = {"default": {}, "tiles3k": {"NGSQC_TILE_MEMBERS": "1"}, "no_fused_scan": {"NGSQC_NO_FUSED_SCAN": "1"}, "k2_general": {"NGSQC_K2_GENERAL": "1"},
            "baseq_ride0": {"NGSQC_BASEQ_RIDE": "0"}, "no_fused_pileup": {"NGSQC_NO_FUSED_PILEUP": "1"}, "long_read": {"NGSQC_LONG_READ_MODE": "1"}}
SKIP_COUNTERS = {"half_depth", "bases_covered_half"}   # (ngsqc_depth_stats: compared through depth_stats)

# ROI of the mapping scans: inside the contigs (FastaFileIndex::seq throws behind a contig end, in the reference too), touching lines, a one-base contig
ROI_BED = "chr1\t0\t2000\nchr1\t2000\t2600\nchr1\t5000\t5001\nchr1\t8000\t29000\nchrX\t0\t9000\nchrY\t100\t4000\nchr2\t0\t1\nchr3\t10\t300\nchrMT\t0\t700\n"
# coverage BED: nested, duplicate, touching and unsorted lines, lines at and past a contig's end (the coverage tools take them)
COV_BED = ("chr3\t250\t300\nchr1\t100\t900\nchr1\t200\t300\nchr1\t200\t300\nchr1\t900\t1500\nchrX\t8990\t9000\nchr1\t29950\t30040\nchr3\t280\t330\n"
           "chr1\t0\t5\nchr2\t0\t1\nchr2\t0\t3\nchrY\t4980\t5000\nchrMT\t650\t720\nchr1\t3000\t29000\nchr1_KI270706v1_random\t0\t1500\n")


class Files:
    """the BAMs of one catalogue: the whole catalogue in members of 64 KB and of about 3 KB, and the subsets the oracle can read for each path"""

    def __init__(self, seed, d):
        self.cat = A.generate(seed)
        self.d = d
        self.paths = {}
        self.bed_roi = self._text("roi.bed", ROI_BED)
        self.bed_cov = self._text("cov.bed", COV_BED)
        self.fasta = H.sparse_fasta_for(self.bed_roi, A.REFS, os.path.join(d, "genome.fa"), seed=5)
        self.cache = {}

    def _text(self, name, t):
        p = os.path.join(self.d, name)
        open(p, "w").write(t)
        return p

    def path(self, small, exclude=()):
        key = (small, tuple(sorted(exclude)))
        if key not in self.paths:
            p = os.path.join(self.d, f"adv_{int(small)}_{'_'.join(key[1]) or 'all'}.bam")
            self.cat.write(p, member_sizes=(3000, 2900, 3100) if small else (65280,), exclude=exclude)
            self.paths[key] = p
        return self.paths[key]

    def oracle(self, key, fn):
        if key not in self.cache:
            self.cache[key] = fn()
        return self.cache[key]


_FILES = {}


@pytest.fixture(params=FILES, ids=lambda s: "catalogue" if s is None else f"seed{s}")
def files(request, tmp_path_factory):
    if request.param not in _FILES:
        _FILES[request.param] = Files(request.param, str(tmp_path_factory.mktemp(f"adv{request.param}")))
    return _FILES[request.param]


def _setenv(monkeypatch, switch):
    for k, v in SWITCHES.get(switch, {}).items():
        monkeypatch.setenv(k, v)
    return switch == "tiles3k"


def _open(path, shards):
    return [ngsqc.Handle(path=path, shard=(i, shards)) for i in range(shards)] if shards > 1 else [ngsqc.Handle(path=path)]


def _close(hs):
    for h in hs:
        h.close()


# ---- MappingQC: ROI, NOROI and WGS ----
@pytest.mark.parametrize("switch", list(SWITCHES) + ["shards3"])
def test_mapping(files, switch, monkeypatch):
    small = _setenv(monkeypatch, switch) or switch == "shards3"
    path = files.path(small)
    refs = A.REFS
    tx, ty = H.xy_tids(refs)
    for mode, merge in ((ngsqc.MODE_ROI, 1), (ngsqc.MODE_NOROI, 0), (ngsqc.MODE_WGS, 3)):
        regs = gc = bins = None
        if mode != ngsqc.MODE_NOROI:
            regs, _ = H.bed_regions(files.bed_roi, refs, merge)
            gc, bins = H.gc_inputs(files.bed_roi, refs, files.fasta, merge)
        for mq in (1, A.MIN_MAPQ):
            kw = dict(regions=regs, min_mapq=mq, tid_x=tx, tid_y=ty, nonspecial=H.nonspecial(refs), gc_chunks=gc, gc_bin=bins)
            hs = _open(path, 3 if switch == "shards3" else 1)
            try:
                if len(hs) > 1:
                    counters, gc_reads, _ = ngsqc.scan_mapping_sharded_local(hs, mode, **kw)
                else:
                    counters, gc_reads = hs[0].scan_mapping(mode, **kw)
                exp = files.oracle(("map", mode, mq), lambda: O.mapping(O.Bam(files.path(False)), mode, files.bed_roi if regs else None, merge_bed=(merge == 1),
                                                                          fasta=files.fasta if regs else None, min_mapq=mq))
                for i, name in enumerate(O.COUNTER_NAMES):
                    if name not in SKIP_COUNTERS:
                        assert int(counters[i]) == int(exp.counters[i]), (mode, mq, name, int(counters[i]), int(exp.counters[i]))
                assert np.array_equal(counters[32:], exp.counters[32:]), (mode, mq, "insert-size histogram")
                if regs:
                    want = np.zeros(101); want[:exp.gc_reads.size] = exp.gc_reads
                    assert np.allclose(gc_reads, want, rtol=1e-12, atol=0.0), (mode, mq, "gc_reads")
                    roi_bases = int(counters[O.COUNTER_NAMES.index("roi_bases")])
                    assert np.array_equal(hs[0].depth(roi_bases), exp.depth), (mode, mq, "per-base depth")
                    hist, cov = hs[0].depth_stats(2499, exp["half_depth"])
                    assert np.array_equal(hist, np.bincount(np.minimum(exp.depth, 2499), minlength=2500)) and cov == exp["bases_covered_half"]
            finally:
                _close(hs)
    assert exp["al_total"] > 0 and exp["bases_usable"] != 0


# ---- the coverage tools: BedLowCoverage / BedHighCoverage, BedCoverage, BedReadCount ----
def _runs_merged(runs, regs):
    """the tools' final merge(true, true, true) on the raw runs"""
    merged = []
    for r in [(regs[l][0], s, e) for (l, s, e) in runs]:
        if merged and merged[-1][0] == r[0] and merged[-1][2] + 1 >= r[1]:
            merged[-1] = (r[0], merged[-1][1], max(merged[-1][2], r[2]))
        else:
            merged.append(r)
    return merged


@pytest.mark.parametrize("switch", list(SWITCHES) + ["shards3"])
def test_coverage(files, switch, monkeypatch):
    small = _setenv(monkeypatch, switch) or switch == "shards3"
    refs = A.REFS
    regs, _ = H.bed_regions(files.bed_cov, refs, 2)       # merge(true, true): the coverage tools' main
    lines, _ = H.bed_regions(files.bed_cov, refs, 0)      # BedCoverage: the lines as they are
    inside = np.concatenate([np.arange(s, e + 1) <= refs[t][1] for t, s, e in regs])   # (the sweep reads depth 0 behind a contig's end)
    tm = H.tid_map(refs)
    for mq in (0, 1, A.MIN_MAPQ):
        for bq, skip in ((0, False), (0, True), (20, False)):
            excl = A.SEQ_STAR_OOB if bq else ()
            path = files.path(small, excl)
            ob_path = files.path(False, excl)
            hs = _open(path, 3 if switch == "shards3" else 1)
            try:
                if len(hs) > 1:
                    ngsqc.scan_depth_sharded_local(hs, regs, min_mapq=mq, min_baseq=bq, skip_mismapped=skip)
                else:
                    hs[0].scan_depth(regs, min_mapq=mq, min_baseq=bq, skip_mismapped=skip)
                h = hs[0]
                if not skip:
                    for is_high in (False, True):
                        for ra in (True, False):
                            exp = files.oracle(("lh", mq, bq, is_high, ra), lambda: O.low_high_coverage(O.Bam(ob_path), files.bed_cov, 3, mq, bq, is_high=is_high,
                                                                                                          random_access=ra, tool_merge=1))
                            runs = h.lowhigh_runs(regs, 3, is_high=is_high, saturate254=not ra)
                            exp_runs = [(tm[H.chr_num(f[0])], int(f[1]) + 1, int(f[2])) for f in (ln.split("\t") for ln in exp["bed"].splitlines())]
                            assert _runs_merged(runs, regs) == exp_runs, (mq, bq, is_high, ra)
                            d = h.depth(exp["roi_bases"])
                            assert np.array_equal(d if ra else np.where(inside, np.minimum(d, 254), 0), exp["depth"]), (mq, bq, is_high, ra, "depth")
                if bq == 0:
                    cov, _, _ = files.oracle(("avg", mq, skip), lambda: O.avg_coverage(O.Bam(ob_path), files.bed_cov, merge_bed=False, min_mapq=mq,
                                                                                       random_access=True, skip_mismapped=skip))
                    assert np.array_equal(h.region_sums(lines), cov), (mq, skip)
                    assert cov.sum() > 0
            finally:
                _close(hs)
        # BedReadCount: the oracle merges the BED (merge(false)); its lines are the regions
        hs = _open(files.path(small), 1)
        try:
            exp, text = files.oracle(("rc", mq), lambda: O.read_counts(O.Bam(files.path(False)), files.bed_cov, mq))
            rregs = [(tm[H.chr_num(f[0])], int(f[1]) + 1, int(f[2])) for f in (ln.split("\t") for ln in text.splitlines())]
            assert np.array_equal(hs[0].region_read_counts(rregs, mq), exp), mq
            assert exp.sum() > 0
        finally:
            _close(hs)


# ---- site pileup ----
def _sites(recs):
    """every mapped record's start, end and end + 1, the positions inside its D and N operations and its I anchors (1-based)"""
    s = set()
    for r in recs:
        if r.flag & 4 or r.tid < 0:
            continue
        L = A.REFS[r.tid][1]
        s.update((r.tid, p) for p in (r.pos + 1, r.end(), r.end() + 1))
        g = r.pos
        for op, ln in r.effective_cigar():
            if op in (A.D, A.N):
                s.update((r.tid, g + k) for k in (1, 1 + ln // 2, ln))
            elif op == A.I:
                s.update(((r.tid, g), (r.tid, g + 1)))
            if op in A.REF_OPS:
                g += ln
        s.add((r.tid, L))
    return sorted((t, p) for t, p in s if p >= 1)


def _site_oracle(ob, sites, bq, npp):
    """per site: the oracle's six counts, or None where getPileup throws (a P operation or a CIGAR that never reaches the site)"""
    out = []
    for t, p in sites:
        try:
            out.append(O.site_pileup(ob, [(t, p)], 1, bq, npp)[0])
        except O.OracleError as e:
            assert "Unknown CIGAR operation" in str(e) or "Could not find position" in str(e), str(e)
            out.append(None)
    return out


@pytest.mark.parametrize("switch", list(SWITCHES))
def test_site_pileup(files, switch, monkeypatch):
    small = _setenv(monkeypatch, switch)
    recs = files.cat.subset(A.SEQ_STAR_OOB)
    sites = _sites(recs)
    h = ngsqc.Handle(path=files.path(small, A.SEQ_STAR_OOB))
    try:
        n_err = 0
        for bq in (13, 255):
            for npp in (False, True):
                exp = files.oracle(("pile", bq, npp), lambda: _site_oracle(O.Bam(files.path(False, A.SEQ_STAR_OOB)), sites, bq, npp))
                got = h.site_pileup(sites, 1, bq, npp)
                for i, e in enumerate(exp):
                    if e is None:
                        assert got[i, 7] >= 1, (sites[i], got[i].tolist())   # the product reports what the reference throws
                        n_err += 1
                    else:
                        assert got[i, :6].tolist() == e.tolist() and got[i, 6:].tolist() == [0, 0], (bq, npp, sites[i], got[i].tolist(), e.tolist())
                assert sum(int(e.sum()) for e in exp if e is not None) > 0
        assert n_err > 0   # (the P records: a P reached before the site)
    finally:
        h.close()


# ---- read QC ----
@pytest.mark.parametrize("switch", list(SWITCHES))
def test_read_qc(files, switch, monkeypatch):
    small = _setenv(monkeypatch, switch)
    for single_end in (False, True):
        exp = files.oracle(("qc", single_end), lambda: O.reads_qc(O.Bam(files.path(False, A.QUAL_OOR)), single_end))
        h = ngsqc.Handle(path=files.path(small, A.QUAL_OOR))
        try:
            got = h.scan_reads(single_end)
        finally:
            h.close()
        assert got["n_unknown_base"] == 0 and got["n_quality_out_of_range"] == 0
        for k in ("c_forward", "c_reverse", "bases_sequenced", "max_cycles"):
            assert got[k] == exp[k], (single_end, k, got[k], exp[k])
        for k in ("bases", "base_qualities", "read_qualities", "qscore_dist_r1", "qscore_dist_r2", "read_lengths", "cycles"):
            assert np.array_equal(got[k], exp[k]), (single_end, k)
    # with the QUAL 0xff records: the oracle throws "Base quality > 100", the product counts the qualities out of range
    with pytest.raises(O.OracleError, match="Base quality > 100"):
        O.reads_qc(O.Bam(files.path(False)))
    h = ngsqc.Handle(path=files.path(small))
    try:
        assert h.scan_reads(False)["n_quality_out_of_range"] > 0
    finally:
        h.close()


# ---- indel windows (getIndels) ----
@pytest.mark.parametrize("switch", list(SWITCHES))
def test_indel_windows(files, switch, monkeypatch):
    small = _setenv(monkeypatch, switch)
    excl = {"op_P"}   # (getIndels throws "Unknown CIGAR operation" on P: variant_oracle.get_indels)
    path = files.path(small, excl)
    ob = O.Bam(files.path(False, excl))
    rds = V.reads(ob)
    index = V.Index(rds)
    genome = HashGenome(A.REFS)
    wins = []
    for w in _windows(_events(rds), genome, 10 ** 6, seed=1):   # (a deletion behind the contig end: its allele is what the genome still holds)
        if w[3] == ngsqc.ALLELE_DEL:
            if not w[4]:
                continue
            w = w[:5] + (genome.slice(w[0], w[1], w[2], len(w[4])),)
        wins.append(w)
    for t, (_, L) in enumerate(A.REFS):   # contig ends
        wins += [(t, max(1, L - 3), L, ngsqc.ALLELE_NONE, "", None), (t, L, L, ngsqc.ALLELE_DEL, "A", genome.slice(t, L, L, 1))]
    wins = sorted(wins, key=lambda w: (w[0], w[1]))
    h = ngsqc.Handle(path=path)
    try:
        for npp in (False, True):
            exp = files.oracle(("indel", npp), lambda: np.array([V.window_counts(index, genome.seq, t, s, e, k, a, npp) for t, s, e, k, a, _ in wins]))
            got = h.indel_windows(wins, include_not_properly_paired=npp)
            bad = np.nonzero((got != exp).any(axis=1))[0]
            assert bad.size == 0, (npp, [(wins[i][:4], got[i].tolist(), exp[i].tolist()) for i in bad[:5]])
            assert exp[:, 3].sum() > 0 and exp[:, 4].sum() > 0
    finally:
        h.close()


# ---- BamToFastq and BamFilter ----
@pytest.mark.parametrize("switch", list(SWITCHES))
def test_fastq_and_filter(files, switch, monkeypatch, tmp_path):
    small = _setenv(monkeypatch, switch)
    path = files.path(small)
    _, recs = F.read_bam(path)
    h = ngsqc.Handle(path=path)
    try:
        for kw in (dict(), dict(fix=True, remove_duplicates=True, extend=40)):
            e1, e2, c = Q.to_fastq(recs, **kw)
            o1, o2 = str(tmp_path / "1.gz"), str(tmp_path / "2.gz")
            assert h.to_fastq(o1, o2, **kw) == c, kw
            assert gzip.decompress(open(o1, "rb").read()) == e1 and gzip.decompress(open(o2, "rb").read()) == e2, kw
            s1, _, sc = Q.to_fastq(recs, paired=False, **kw)
            assert h.to_fastq(o1, None, **kw) == sc and gzip.decompress(open(o1, "rb").read()) == s1, kw
        for kw in (dict(), dict(min_mq=0, max_gap=-1, max_mm=-1), dict(min_mq=A.MIN_MAPQ, max_gap=0)):
            out = str(tmp_path / "f.bam")
            got = h.filter_pairs(out, **kw)
            header, exp, passed, dropped = F.filter_file(path, **kw)
            hh, rr = F.read_bam(out)
            assert hh == header and rr == exp and got == (passed, dropped), kw
    finally:
        h.close()


# ---- the fused job equals the single-purpose calls ----
@pytest.mark.parametrize("switch", list(SWITCHES))
def test_fused_job(files, switch, monkeypatch):
    small = _setenv(monkeypatch, switch)
    refs = A.REFS
    regs, _ = H.bed_regions(files.bed_roi, refs, 3)
    dregs, _ = H.bed_regions(files.bed_cov, refs, 2)
    tx, ty = H.xy_tids(refs)
    sites = _sites(files.cat.records)
    mp = dict(mode=ngsqc.MODE_WGS, regions=regs, min_mapq=1, tid_x=tx, tid_y=ty, nonspecial=H.nonspecial(refs))
    for bq in (0, 20):
        h = ngsqc.Handle(path=files.path(small))
        try:
            job = h.run_job(mapping=mp, depth=dict(regions=dregs, min_mapq=1, min_baseq=bq), sites=sites, site_params=(1, 13, True), read_qc=dict(single_end=False))
            kw = dict(mp); mode = kw.pop("mode")
            counters, gc_reads = h.scan_mapping(mode, **kw)
            assert np.array_equal(job["counters"], counters) and np.array_equal(job["gc_reads"], gc_reads)
            assert np.array_equal(job["site_counts"], h.site_pileup(sites, 1, 13, True))
            reads = h.scan_reads(False)
            for k, v in reads.items():
                assert np.array_equal(job["reads"][k], v), k
        finally:
            h.close()
