"""Designed reads and target regions for the MappingQC record loops (csrc/scan.hip classify<MODE_ROI / MODE_NOROI / MODE_WGS>, called by scan_kernel,
walk_scan_kernel and scan_long_kernel): a read on both sides of every integer comparison that relates it to a region, a GC chunk, a contig end or a histogram bound.

Every case is a list of advbam.Record on advbam.REFS in file order (coordinate-sorted), a BED text, optionally hand-set GC bins, the parameter sets (min_mapq, "xy" or
"no_y": tid_y = -1) it is run under, the BGZF member sizes of its file and a premise over the bookkeeping of tests/mapping_model.py: what the case is there for,
asserted by tests/test_cpu_mapping_model.py so that a later edit cannot hollow the case out. The expected values are the model's; nothing here knows them.

Regions: Case.tables(mode) gives the region and GC chunk tables as the host layer (hostprep.bed_regions) makes them. A case with merge=True is loaded as MappingQC
loads it (BedFile::merge() in target-region mode, sort + merge in WGS mode; its BED is merged and sorted already, so both leave it as it is). region_cuts has
merge=False: its BED is sorted and free of overlaps, which is all Statistics::mapping asks for, and its touching lines stay two regions; no line is longer than
100 bases, so roi.chunk(100) leaves the lines as the chunks.

Inputs the reference leaves undefined - a negative DP tag, isize == INT32_MIN - are in no case (check_domain). guarded_record() is the one record with
isize == INT32_MIN: it goes to the product only, behind the guard of csrc/scan.hip abs_isize."""
import os
import tempfile

import advbam as A
import cram_twin
import hostprep as H
import mapping_model as MM

M, I, D, N, S, H_, P, EQ, X = A.M, A.I, A.D, A.N, A.S, A.H, A.P, A.EQ, A.X
T1, TX, TY, TSHORT = A.T1, A.TX, A.TY, A.TSHORT
PP1, PP2 = 0x1 | 0x2 | 0x40, 0x1 | 0x2 | 0x80 | 0x10
DUP = 0x400
LOW_MAPQ = A.MIN_MAPQ - 1
INT32_MIN = -2 ** 31
MODES = (MM.MODE_ROI, MM.MODE_NOROI, MM.MODE_WGS)
STD_PARAMS = ((1, "xy"), (A.MIN_MAPQ, "xy"))


def rec(name, pos, cigar, flag=0, tid=T1, mapq=60, isize=0, dp=None, dp_type="C", cg=None):
    """pos: 0-based. dp: the DP tag's value (None: no tag). cg: the operations a CG:B,I tag carries; cigar is then the placeholder"""
    ops = cg if cg else cigar
    l_seq = sum(ln for op, ln in ops if op in A.QUERY_OPS)
    aux = A._tagi(b"DP", dp_type, dp) if dp is not None else b""
    return A.Record(name, flag, tid, pos, cigar, "ACGT"[len(name) % 4] * l_seq, mapq=mapq, qual=[40] * l_seq, isize=isize, mtid=tid, mpos=max(pos, 0), aux=aux,
                    cg=(A._cg(cg), cg) if cg else None)


def at(start1, length):
    """an M-only read: (0-based pos, cigar) of the 1-based span [start1, start1 + length - 1]"""
    return start1 - 1, [(M, length)]


def key(r):
    return (r.tid if r.tid >= 0 else len(A.REFS), r.pos)


def dp_of(r):
    return MM.tag_int(r.aux, b"DP")


def check_domain(records):
    assert all(r.isize != INT32_MIN and dp_of(r) >= 0 for r in records)   # neither goes into a file the oracle reads


class Case:
    def __init__(self, name, aim, records, bed, premise, params=STD_PARAMS, member_sizes=(65280,), merge=True, hand_bins=None):
        self.name, self.aim, self.bed, self.premise, self.params, self.member_sizes, self.merge, self.hand_bins = name, aim, bed, premise, tuple(params), tuple(member_sizes), merge, hand_bins
        self.records = sorted(records, key=key)   # (stable: the order given within a position)
        for r in self.records:
            r.check()
        check_domain(self.records)
        assert len({r.name for r in self.records}) == len(self.records)
        self._tables = {}

    def write(self, path, member_sizes=None, whole_records=True, records=None):
        """the records in their order behind Catalogue.header(), in BGZF members of at most the given sizes. whole_records: as htslib writes - the header in a member
        of its own, every other member begins with a record and none is cut (what lets the scan ride the library's chain walk); otherwise the stream is cut
        wherever a size ends (the library's general path)"""
        recs = self.records if records is None else records
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

    def merge_mode(self, mode):
        """of hostprep.bed_regions / oracle_lib.gc_bins for this case in that mode"""
        return 0 if not self.merge else (1 if mode == MM.MODE_ROI else 3)

    def tables(self, mode):
        """(regions, GC chunks) of the mode: the host layer's BED handling"""
        if mode == MM.MODE_NOROI:
            return [], []
        mm = self.merge_mode(mode)
        if mm not in self._tables:
            with tempfile.TemporaryDirectory() as d:
                p = os.path.join(d, "roi.bed")
                open(p, "w").write(self.bed)
                regs, _ = H.bed_regions(p, A.REFS, mm)
                if self.merge:
                    chunks, _ = H.bed_regions(p, A.REFS, 4 if mm == 1 else 5)
                else:
                    assert all(e - s + 1 <= 100 for _, s, e in regs)   # chunk(100) leaves such lines alone
                    chunks = list(regs)
            self._tables[mm] = (regs, chunks)
        return self._tables[mm]

    def bins(self, mode):
        """the hand-set bins as the model takes them: what lies above 100 has no bin (mapping_setup)"""
        raw = self.hand_bins(self.tables(mode)[1])
        return raw, [b if b <= 100 else -1 for b in raw]

    def files(self, d):
        """BED and sparse FASTA of the case in directory d; returns (bed path, fasta path)"""
        bed, fasta = os.path.join(d, self.name + ".bed"), os.path.join(d, self.name + ".fa")
        if not os.path.exists(fasta):
            open(bed, "w").write(self.bed)
            H.sparse_fasta_for(bed, A.REFS, fasta, seed=5)
        return bed, fasta

    def fasta_bins(self, mode, d):
        """the bins of the mode's GC chunks from the case's sparse FASTA (Statistics.cpp:363-387, through the oracle)"""
        import oracle_lib as O
        bed, fasta = self.files(d)
        bins = [int(b) for b in O.gc_bins(fasta, bed, self.merge_mode(mode))]
        assert len(bins) == len(self.tables(mode)[1])
        return bins

    def run(self, mode, min_mapq=1, yx="xy", bins=None, rules=MM.REFERENCE, records=None, book=None):
        """the model on this case. bins None: no GC chunks"""
        regs, chunks = self.tables(mode)
        tx, ty = H.xy_tids(A.REFS)
        return MM.mapping(self.records if records is None else records, mode, regs, chunks if bins is not None else (), bins if bins is not None else (),
                          min_mapq=min_mapq, tid_x=tx, tid_y=ty if yx == "xy" else -1, nonspecial=H.nonspecial(A.REFS), rules=rules, book=book)

    def book(self, mode=MM.MODE_ROI, min_mapq=1, bins=None):
        b = []
        if bins is None and mode != MM.MODE_NOROI:
            bins = [0] * len(self.tables(mode)[1])   # (every chunk with a bin: the premises look at gc_n)
        self.run(mode, min_mapq, bins=bins, book=b)
        return {self.records[e.k].name: e for e in b}


# ---- near_window ----
NEAR_BED = "chr1\t5000\t5200\nchr1\t6000\t6200\n"    # 1-based [5001, 5200] and [6001, 6200]: 800 bases between them
NEAR_REGS = ((5001, 5200), (6001, 6200))
NEAR_D = (251, 250, 1, 0)
RLEN0 = [(S, 10), (I, 5)]                              # no reference length: the record covers its start


def near_window():
    recs = []
    for k, (s, e) in enumerate(NEAR_REGS):
        for d in NEAR_D:
            recs.append(rec("front%d_%d" % (k, d), *at(s - d - 49, 50)))         # ends d bases in front of the region start
            recs.append(rec("behind%d_%d" % (k, d), *at(e + d, 50)))             # starts d bases behind the region end
            recs.append(rec("zfront%d_%d" % (k, d), s - d - 1, RLEN0))
            recs.append(rec("zbehind%d_%d" % (k, d), e + d - 1, RLEN0))
    recs.append(rec("gap", *at(5440, 321)))                                       # [5440, 5760]: within 250 of both regions
    recs.append(rec("zgap", 5449, RLEN0))                                         # 5450: 250 behind the first region, 551 in front of the second
    recs.append(rec("noRegion", *at(101, 50), tid=TSHORT))
    recs.append(rec("zNoRegion", 100, RLEN0, tid=TSHORT))
    recs.append(rec("tidNeg", *at(5051, 50), tid=-1, flag=0x1 | 0x40))
    recs.append(rec("far", *at(9001, 50)))

    def premise(case):
        b = case.book()
        assert case.tables(MM.MODE_ROI)[0] == [(T1, s, e) for s, e in NEAR_REGS]
        for k in range(2):
            for z in ("", "z"):
                for side in ("front", "behind"):
                    got = [(b["%s%s%d_%d" % (z, side, k, d)].near, b["%s%s%d_%d" % (z, side, k, d)].on_target) for d in NEAR_D]
                    assert got == [(False, False), (True, False), (True, False), (True, True)], (k, z, side, got)
        assert b["gap"].near and not b["gap"].on_target and b["gap"].start1 - 250 <= 5200 and b["gap"].end1 + 250 >= 6001
        assert b["zgap"].near and b["zgap"].start1 == b["zgap"].end1 == 5450
        for n in ("noRegion", "zNoRegion", "tidNeg", "far"):
            assert not b[n].near and b[n].counted, n
        assert all(e.start1 == e.end1 for n, e in b.items() if n.startswith("z"))
    return Case("near_window", "the 250-base near window and the on-target edges, rlen == 0 records included; a reference without regions; tid = -1", recs, NEAR_BED, premise)


# ---- region_cuts ----
CUT_BED = "chr1\t5000\t5080\nchr1\t5080\t5150\nchr1\t5400\t5460\n"   # [5001, 5080] touching [5081, 5150]; [5401, 5460]
CUT_SPANS = {"cutStart": (4971, 5030), "cutEnd": (5420, 5500), "contains": (5390, 5470), "acrossTouch": (5060, 5100), "containsB": (5075, 5155),
             "allThree": (4990, 5470), "endsAtTouch": (5040, 5080), "startsAtTouch": (5081, 5120), "oneBaseIn": (4952, 5001), "oneBaseOut": (5461, 5500), "startsOnLast": (5150, 5190)}
CUT_DP = (None, 0, 1, 3, 4, 5, 255)


def region_cuts():
    recs = []
    for name, (s, e) in CUT_SPANS.items():
        for k, dp in enumerate(CUT_DP):
            recs.append(rec("%s_dp%s" % (name, dp), *at(s, e - s + 1), dp=dp, dp_type="CsiCSIc"[k] if dp != 255 else "C"))
        recs.append(rec("%s_dup" % name, *at(s, e - s + 1), dp=3, flag=DUP))
        recs.append(rec("%s_lowq" % name, *at(s, e - s + 1), dp=4, mapq=LOW_MAPQ))

    def premise(case):
        regs = case.tables(MM.MODE_ROI)[0]
        assert regs == [(T1, 5001, 5080), (T1, 5081, 5150), (T1, 5401, 5460)] == case.tables(MM.MODE_WGS)[0]   # unmerged: the touching lines stay apart
        with tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "roi.bed")
            open(p, "w").write(case.bed)
            assert H.bed_regions(p, A.REFS, 1)[0] == [(T1, 5001, 5150), (T1, 5401, 5460)]                        # BedFile::merge() would join them
        b = case.book()
        want = {"cutStart": [0], "cutEnd": [2], "contains": [2], "acrossTouch": [0, 1], "containsB": [0, 1], "allThree": [0, 1, 2], "endsAtTouch": [0],
                "startsAtTouch": [1], "oneBaseIn": [0], "oneBaseOut": [], "startsOnLast": [1]}
        for name, w in want.items():
            for suffix in ["dp%s" % dp for dp in CUT_DP] + ["dup", "lowq"]:
                e = b["%s_%s" % (name, suffix)]
                assert e.regions == w and e.on_target == bool(w), (name, suffix, e.regions)
                assert e.usable == (bool(w) and suffix != "dup"), (name, suffix)
        assert not any(e.usable for n, e in case.book(min_mapq=A.MIN_MAPQ).items() if n.endswith("_lowq"))
        assert b["oneBaseIn_dp1"].end1 == 5001 and b["oneBaseOut_dp1"].start1 == 5461 and b["oneBaseOut_dp1"].near
        assert {dp_of(r) for r in case.records} == {0, 1, 3, 4, 5, 255}
    return Case("region_cuts", "per-region sums of reads cut by, containing and spanning regions (touching ones), under every DP tag value, duplicates, low MAPQ", recs,
                CUT_BED, premise, merge=False)


# ---- overlap_window ----
OVL_BED = "chr1\t0\t100\nchr1\t10000\t10200\nchr1\t10300\t10400\nchr1\t12000\t12100\n"   # [1, 100], [10001, 10200], [10301, 10400], [12001, 12100]
# name -> (start1, l_seq of an M-only read, isize, window, regions the window is taken off)
OVL_READS = {
    "pos_inside": (10051, 100, 150, (10101, 10150), [1]), "pos_acrossStart": (9951, 100, 120, (9971, 10050), [1]), "pos_acrossEnd": (10151, 100, 130, (10181, 10250), [1]),
    "pos_two": (10151, 200, 210, (10161, 10350), [1, 2]), "pos_untouched": (10291, 100, 5, (10196, 10390), [1, 2]), "pos_endOnly": (10151, 100, 149, (10200, 10250), [1]),
    "neg_inside": (10051, 100, -150, (10051, 10100), [1]), "neg_acrossStart": (9951, 100, -120, (9951, 10030), [1]), "neg_acrossEnd": (10151, 100, -110, (10151, 10240), [1]),
    "neg_two_untouched": (10151, 100, -20, (10151, 10330), [1, 2]), "neg_startOnly": (10151, 100, -49, (10151, 10301), [1, 2]),
    "zero_inside": (10051, 40, 0, (10051, 10130), [1]), "zero_acrossStart": (9981, 40, 0, (9981, 10060), [1]), "zero_acrossEnd": (10151, 40, 0, (10151, 10230), [1]),
    "zero_two_untouched": (10151, 100, 0, (10151, 10350), [1, 2]),
    "belowOne": (1, 50, 10, (-39, 50), [0]),
    "ovl1_pos": (10051, 100, 199, (10150, 10150), [1]), "ovl1_neg": (10051, 100, -199, (10051, 10051), [1]),
}
OVL_NO_WINDOW = {"ovl0_pos": (10051, 100, 200, PP1), "ovl0_neg": (10051, 100, -200, PP1), "gate_read2": (10051, 100, 150, PP2), "gate_unpaired": (10051, 100, 150, 0x2 | 0x40),
                 "gate_notProper": (10051, 100, 150, 0x1 | 0x40), "gate_dup": (10051, 100, 150, PP1 | DUP)}
# reads whose l_seq is not their reference span: (cigar, isize, window) at start 10051
OVL_SHAPES = {"softclip": ([(S, 20), (M, 80)], 150, (10101, 10150)), "deletion": ([(M, 50), (D, 30), (M, 50)], 150, (10101, 10150)),
              "insertion": ([(M, 40), (I, 20), (M, 40)], -150, (10051, 10100)), "softclipZero": ([(S, 30), (M, 70)], 0, (10051, 10250))}


def overlap_window():
    recs = [rec(n, *at(s, ln), flag=PP1, isize=isz) for n, (s, ln, isz, _, _) in OVL_READS.items()]
    recs += [rec(n, *at(s, ln), flag=f, isize=isz) for n, (s, ln, isz, f) in OVL_NO_WINDOW.items()]
    recs += [rec(n, 10050, cig, flag=PP1, isize=isz) for n, (cig, isz, _) in OVL_SHAPES.items()]
    recs.append(rec("gate_spliced", 10050, [(M, 50), (N, 10), (M, 50)], flag=PP1, isize=150))
    recs.append(rec("gate_lowq", *at(10051, 100), flag=PP1, isize=150, mapq=LOW_MAPQ))

    def premise(case):
        b = case.book()
        assert case.tables(MM.MODE_ROI)[0] == [(T1, 1, 100), (T1, 10001, 10200), (T1, 10301, 10400), (T1, 12001, 12100)]
        for n, (s, ln, isz, win, regs) in OVL_READS.items():
            assert b[n].usable and b[n].window == win and b[n].window_regions == regs, (n, b[n].window, b[n].window_regions)
        for n in ("pos_untouched", "neg_two_untouched", "zero_two_untouched", "neg_startOnly"):
            assert set(b[n].window_regions) - set(b[n].regions), n                 # a region the read itself does not touch
        assert b["pos_endOnly"].window[0] == 10200 and b["neg_startOnly"].window[1] == 10301    # a window that meets a region in one base
        for n in list(OVL_NO_WINDOW) + ["gate_spliced"]:
            assert b[n].on_target and b[n].window is None, n
        assert b["gate_lowq"].window == (10101, 10150) and case.book(min_mapq=A.MIN_MAPQ)["gate_lowq"].window is None
        for n, (cig, isz, win) in OVL_SHAPES.items():
            r = next(x for x in case.records if x.name == n)
            assert b[n].window == win and len(r.seq) != b[n].end1 - b[n].start1 + 1, n
        assert b["belowOne"].window[0] < 1
    return Case("overlap_window", "the read-overlap window of target-region mode: its start and length from l_seq and isize, the regions it meets, every gate condition",
                recs, OVL_BED, premise)


# ---- gc_counts ----
GC_BED = "chr1\t10000\t23000\nchr1\t24000\t24100\n"   # 13 000 bases = 130 chunks of 100, and a second region of one chunk
GC_N = (1, 2, 4, 8, 16, 32, 63, 64, 65, 128)
GC_FIRST = {1: 5, 2: 7, 4: 10, 8: 20, 16: 40, 32: 60, 63: 2, 64: 30, 65: 62, 128: 1}   # first chunk of the read of n chunks
POW2 = (1, 2, 4, 8, 16, 32, 64, 128)


def lane_ops(n):
    """10M <k>N 10M over exactly n chunks, from the middle of a chunk (n = 1: 20M)"""
    return [(M, 20)] if n == 1 else [(M, 10), (N, (n - 1) * 100 - 19), (M, 10)]


def many_ops(span, spliced=True, clip=0):
    """65 operations (one more with a soft clip) over `span` reference bases"""
    front = [(S, clip)] if clip else []
    if spliced:
        return front + [(M, 1), (I, 1)] * 31 + [(M, 1), (N, span - 37), (M, 5)]
    return front + [(M, 1), (I, 1)] * 32 + [(M, span - 32)]


def few_ops(span, spliced=True, clip=0):
    """the same reference span, query length, clipped bases and splice flag in at most five operations"""
    front = [(S, clip)] if clip else []
    if spliced:
        return front + [(M, 31), (I, 31), (M, 1), (N, span - 37), (M, 5)]
    return front + [(M, 32), (I, 32), (M, span - 32)]


def hand_bins(chunks):
    return [(-1 if i % 10 == 3 else 100 if i % 10 == 6 else 101 if i % 10 == 8 else (i * 7) % 100) for i in range(len(chunks))]


def gc_counts():
    recs = []
    for n in GC_N:
        s = 10001 + 100 * GC_FIRST[n] + 50
        recs.append(rec("lane%d" % n, s - 1, lane_ops(n)))
        span = (n - 1) * 100 + 1 if n > 1 else 33
        recs.append(rec("wave%d" % n, s - 1, many_ops(span, spliced=n > 1)))
    recs.append(rec("lastBaseOfChunk", *at(10100, 20)))            # starts on a chunk's last base
    recs.append(rec("firstBaseOfChunk", *at(10182, 20)))           # ends on a chunk's first base
    recs.append(rec("wholeChunk", *at(10501, 100)))
    recs.append(rec("dup4", 10001 + 100 * 90 + 49, lane_ops(4), flag=DUP))
    recs.append(rec("lowq8", 10001 + 100 * 100 + 49, lane_ops(8), mapq=LOW_MAPQ))
    recs.append(rec("bothRegions", 22950, [(M, 10), (N, 1080), (M, 10)]))                    # [22951, 24050]: the last chunk of the first region and the second region
    recs.append(rec("bothRegionsWave", 22950, many_ops(1100)))
    recs.append(rec("secondOnly", *at(24041, 30)))

    def premise(case):
        for mode in (MM.MODE_ROI, MM.MODE_WGS):
            regs, chunks = case.tables(mode)
            assert regs == [(T1, 10001, 23000), (T1, 24001, 24100)]
            assert chunks == [(T1, 10001 + 100 * i, 10100 + 100 * i) for i in range(130)] + [(T1, 24001, 24100)]
        raw, bins = case.bins(MM.MODE_ROI)
        assert {-1, 100, 101} <= set(raw) and set(bins) <= set(range(-1, 101)) and bins.count(-1) == raw.count(-1) + raw.count(101)
        b = case.book()
        for n in GC_N:
            lane, wave = b["lane%d" % n], b["wave%d" % n]
            assert lane.gc_n == wave.gc_n == n and not lane.wave_path and wave.wave_path and lane.gc_hits == wave.gc_hits == 1, n
        assert (b["lastBaseOfChunk"].gc_n, b["firstBaseOfChunk"].gc_n, b["wholeChunk"].gc_n) == (2, 2, 1)
        assert b["dup4"].gc_n == 4 and not b["dup4"].usable and b["lowq8"].gc_n == 8
        w = case.book(MM.MODE_WGS)
        for n in ("bothRegions", "bothRegionsWave"):
            assert b[n].gc_hits == 1 and w[n].gc_hits == 2 and w[n].regions == [0, 1] and w[n].gc_n == 2, n
        assert w["bothRegionsWave"].wave_path and not w["bothRegions"].wave_path
        # reads over chunks of several bins, chunks without a bin among them
        first = 10001 + 100 * GC_FIRST[16] + 50
        under = [bins[i] for i, (_, s, e) in enumerate(case.tables(MM.MODE_ROI)[1]) if s <= first + 1500 and e >= first]
        assert len(under) == 16 and -1 in under and 100 in under and len(set(under)) > 5
    return Case("gc_counts", "GC hits: the chunk count n at 1..128 around GC_NMAX = 64 on the lane and the wave path, chunks without a bin, one hit per region in WGS mode",
                recs, GC_BED, premise, hand_bins=hand_bins)


# ---- sex_contigs ----
SEX_BED = "chr1\t5000\t5100\nchrX\t1000\t1100\n"
LX, LY = A.REFS[TX][1], A.REFS[TY][1]


def sex_contigs():
    recs = []
    for c, t, L in (("x", TX, LX), ("y", TY, LY)):
        recs += [rec(c + "PosNeg1M", -1, [(M, 1)], tid=t),            # end 0: not counted
                 rec(c + "PosNeg20M", -1, [(M, 20)], tid=t),          # end 19
                 rec(c + "First1M", 0, [(M, 1)], tid=t),              # end 1
                 rec(c + "Inside", 1040, [(M, 50)], tid=t, flag=PP1, isize=300),
                 rec(c + "Dup", 1050, [(M, 50)], tid=t, flag=PP1 | DUP, isize=300),
                 rec(c + "Unmapped", 1060, [], tid=t, flag=0x1 | 0x4 | 0x80),
                 rec(c + "UnmappedCigar", 1061, [(M, 30)], tid=t, flag=0x4),
                 rec(c + "Secondary", 1070, [(M, 50)], tid=t, flag=0x100),
                 rec(c + "Supplementary", 1080, [(M, 50)], tid=t, flag=0x800),
                 rec(c + "LowMapq", 1090, [(M, 50)], tid=t, mapq=0),
                 rec(c + "LastBase", L - 1, [(M, 20)], tid=t),        # pos == len - 1
                 rec(c + "PastEnd", L, [(M, 10)], tid=t),             # pos == len
                 rec(c + "PastEnd2", L + 1, [(M, 10)], tid=t)]
    recs += [rec("a%d" % k, 4990 + 7 * k, [(M, 50)], flag=PP1, isize=250) for k in range(8)]
    counted = ("PosNeg20M", "First1M", "Inside", "Dup", "Unmapped", "UnmappedCigar", "LowMapq", "LastBase")

    def premise(case):
        r = case.run(MM.MODE_ROI)
        assert r["reads_x"] == r["reads_y"] == len(counted) and r["yx_valid"] == 1
        r = case.run(MM.MODE_ROI, yx="no_y")
        assert r["reads_x"] == r["reads_y"] == r["yx_valid"] == 0
        b = case.book()
        assert b["xPosNeg1M"].end1 == 0 and b["xFirst1M"].end1 == 1 and b["xLastBase"].start1 == LX and b["yPastEnd"].start1 == LY + 1
        assert (1, "no_y") in case.params
    return Case("sex_contigs", "chrX / chrY read counts: both ends of the contig, duplicates, placed unmapped, secondary and supplementary reads; tid_y = -1", recs,
                SEX_BED, premise, params=STD_PARAMS + ((1, "no_y"),))


# ---- insert_sizes ----
INS_BED = "chr1\t1000\t3000\n"
INS_EDGES = (0, 1, 998, 999, 1000, 1001)
INS_PILE = 300


def insert_sizes():
    recs = []
    k = 0
    for v in INS_EDGES:
        for sign in (1, -1):
            for f in (PP1, PP2):
                recs.append(rec("edge%d_%d_%x" % (v, sign, f), 1100 + k, [(M, 50)], flag=f, isize=sign * v)); k += 1
    for j in range(INS_PILE):                       # the same two bins from every wave and workgroup
        recs.append(rec("pile0_%d" % j, 1200 + 5 * j, [(M, 50)], flag=PP1 if j % 2 else PP2, isize=0))
        recs.append(rec("pile999_%d" % j, 1202 + 5 * j, [(M, 50)], flag=PP1 if j % 3 else PP2, isize=999 if j % 2 else -999))
    recs.append(rec("spliced", 2800, [(M, 25), (N, 40), (M, 25)], flag=PP1, isize=500))
    recs.append(rec("notProper", 2801, [(M, 50)], flag=0x1 | 0x40, isize=500))
    recs.append(rec("unpaired", 2802, [(M, 50)], flag=0x2 | 0x40, isize=500))
    recs.append(rec("unmappedProper", 2803, [(M, 25), (N, 40), (M, 25)], flag=PP1 | 0x4, isize=500))   # (its N does not count: the CIGAR of an unmapped record is not read)
    for v in (100, 99, -100, -99):                  # read 1 of 50 bases: 2 * length - |isize| in {0, 1}
        recs.append(rec("mate%d" % v, 2810, [(M, 50)], flag=PP1, isize=v))
        recs.append(rec("mate%d_dup" % v, 2811, [(M, 50)], flag=PP1 | DUP, isize=v))
        recs.append(rec("mate%d_lowq" % v, 2812, [(M, 50)], flag=PP1, isize=v, mapq=LOW_MAPQ))
        recs.append(rec("mate%d_read2" % v, 2813, [(M, 50)], flag=PP2, isize=v))

    def premise(case):
        b = case.book(MM.MODE_WGS)
        for v in INS_EDGES:
            for n, e in b.items():
                if n.startswith("edge%d_" % v):
                    assert e.ins_bin == (v if v < 1000 else None), n
        r = case.run(MM.MODE_NOROI)
        assert r.hist[0] == INS_PILE + 4 and r.hist[999] == INS_PILE + 4 and r.hist[1] == r.hist[998] == 4
        for n in ("spliced", "notProper", "unpaired"):
            assert b[n].ins_bin is None, n
        assert b["unmappedProper"].ins_bin == 500
        assert sum(len(x.bytes()) for x in case.records) > 10 * max(case.member_sizes)     # the piles lie in many members
    return Case("insert_sizes", "the insert-size histogram at bins 0 and 999 from many waves, spliced and improper pairs, the read-1 overlap of the NOROI / WGS loops", recs,
                INS_BED, premise, member_sizes=(4000, 3500, 5000))


# ---- wave_path ----
WAVE_BED = "chr1\t5000\t5080\nchr1\t5100\t5150\nchr1\t5400\t5460\nchrX\t1000\t1100\n"   # [5001, 5080], [5101, 5150], [5401, 5460]; chrX [1001, 1100]
# name -> (start1, span, keyword arguments of the record); every one as a lane record, a record of 65 operations and a CG:B,I record
WAVE_TWINS = {
    "near250": (5001 - 250 - 99, 100, dict(spliced=False)),
    "cutStart": (4971, 60, dict(spliced=False, dp=3)),
    "allThree": (4990, 481, dict(dp=5)),
    "ovlAcrossEnd": (5021, 100, dict(spliced=False, flag=PP1, isize=140)),
    "splicedProper": (5030, 200, dict(flag=PP1, isize=300)),
    "bin999": (5040, 70, dict(spliced=False, flag=PP2, isize=-999)),
    "bin1000": (5041, 70, dict(spliced=False, flag=PP1, isize=1000)),
    "mateOverlap": (5042, 70, dict(spliced=False, flag=PP1, isize=100, dp=1)),
    "dup": (5050, 90, dict(spliced=False, flag=PP1 | DUP, isize=200, dp=4)),
    "lowq": (5060, 90, dict(spliced=False, mapq=LOW_MAPQ, dp=255)),
    "clipped": (5401, 60, dict(spliced=False, clip=7)),
    "onX": (1051, 120, dict(tid=TX)),
}
WAVE_KINDS = ("lane", "ops65", "cg")


def wave_path():
    recs = []
    for name, (s, span, kw) in WAVE_TWINS.items():
        kw = dict(kw)
        spliced, clip = kw.pop("spliced", True), kw.pop("clip", 0)
        few, many = few_ops(span, spliced, clip), many_ops(span, spliced, clip)
        l_seq = sum(ln for op, ln in few if op in A.QUERY_OPS)
        recs.append(rec("%s_lane" % name, s - 1, few, **kw))
        recs.append(rec("%s_ops65" % name, s - 1, many, **kw))
        recs.append(rec("%s_cg" % name, s - 1, [(S, l_seq), (N, span)], cg=few, **kw))

    def premise(case):
        by = {r.name: r for r in case.records}
        for mode in MODES:
            b = case.book(mode)
            for name in WAVE_TWINS:
                assert [b["%s_%s" % (name, k)].wave_path for k in WAVE_KINDS] == [False, True, True], name
                assert len(by[name + "_lane"].cigar) <= 6 and len(by[name + "_ops65"].cigar) in (65, 66) and by[name + "_cg"].effective_cigar() == by[name + "_lane"].cigar
                for mq in (1, A.MIN_MAPQ):      # each twin, alone in a file, contributes what its lane record contributes
                    bins = [i % 7 for i in range(len(case.tables(mode)[1]))]
                    alone = [case.run(mode, mq, bins=bins, records=[by["%s_%s" % (name, k)]]).outputs() for k in WAVE_KINDS]
                    assert alone[0] == alone[1] == alone[2], (mode, name, mq)
        b = case.book()
        assert b["near250_lane"].near and not b["near250_lane"].on_target and b["allThree_cg"].regions == [0, 1, 2] and b["ovlAcrossEnd_ops65"].window_regions == [0, 1]
        assert b["splicedProper_ops65"].ins_bin is None and b["bin999_cg"].ins_bin == 999 and b["bin1000_ops65"].ins_bin is None
    return Case("wave_path", "the same counters when scan_long_kernel classifies: records of 65 operations and CG:B,I records next to lane twins with the same sums", recs,
                WAVE_BED, premise)


def guarded_record():
    """isize == INT32_MIN, a proper read 1 on the target of insert_sizes: for the product alone (csrc/scan.hip abs_isize)"""
    return rec("isizeIntMin", 2820, [(M, 50)], flag=PP1, isize=INT32_MIN)


BUILDERS = (near_window, region_cuts, overlap_window, gc_counts, sex_contigs, insert_sizes, wave_path)
NAMES = tuple(b.__name__ for b in BUILDERS)
_made = {}


def case(name):
    """made once and shared: nobody writes to a case"""
    if name not in _made:
        _made[name] = BUILDERS[NAMES.index(name)]()
    return _made[name]
