"""Plain model of ReadQC's per-entry work: how a FASTQ text falls into entries (the rules of DESIGN.md for what the reference's line reader leaves open),
FastqEntry::validate (src/cppNGS/FastqFileStream.cpp:3-44), StatisticsReads::update(const FastqEntry&) (src/cppNGS/StatisticsReads.cpp:26-81) and the values of
StatisticsReads::getResult() (:160-442) that are numbers. The checker of csrc/fastqin.hip / csrc/fastq_visit.h and of the ReadQC tool: every field of
ngsqc_read_stats, the read-length histogram and the [320][7] cycle table."""
import math

import numpy as np

RQ_CYC = 320
OK, ERR_HEADER, ERR_HEADER2, ERR_LENGTH, ERR_BASE, ERR_QUALITY, ERR_EMPTY_HEADER = range(7)
_BASE_CLASS = np.full(256, 5, np.int64)
for _i, _c in enumerate(b"ACGTN"):
    _BASE_CLASS[_c] = _i


def lines_of(text):
    """The lines of a file: "\\n" and "\\r\\n" end a line, the last line need not be ended, lines at the end that are all empty are dropped."""
    text = bytes(text)
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()            # (what follows the last "\n" is no line when it is empty)
    lines = [l[:-1] if l.endswith(b"\r") else l for l in lines]
    while lines and lines[-1] == b"":
        lines.pop()
    return lines


def entries_of(text):
    """(header, bases, header2, qualities) per entry; the missing lines of an incomplete last entry are empty."""
    lines = lines_of(text)
    lines += [b""] * (-len(lines) % 4)
    return [tuple(lines[i:i + 4]) for i in range(0, len(lines), 4)]


def text_of(entries):
    """what -out1 / -out2 hold: every entry as its four lines, each followed by "\\n" (FastqOutfileStream::write)"""
    return b"".join(l + b"\n" for e in entries for l in e)


def quality_ok(c, long_read):
    return 33 <= c <= (126 if long_read else 74)


def validate(entry, long_read):
    """0, or the kind of the first check of FastqEntry::validate that fails; an entry with an empty header is not validated (FastqFileStream.cpp:151):
    kind 6 when update() cannot take it."""
    header, bases, header2, quals = entry
    bad_base = any(_BASE_CLASS[c] == 5 for c in bases)
    bad_qual = any(not quality_ok(c, long_read) for c in quals)
    if len(header) == 0:
        return ERR_EMPTY_HEADER if (len(bases) != len(quals) or bad_base or bad_qual) else OK
    if header[0:1] != b"@":
        return ERR_HEADER
    if len(header2) == 0 or header2[0:1] != b"+":
        return ERR_HEADER2
    if len(bases) != len(quals):
        return ERR_LENGTH
    if bad_base:
        return ERR_BASE
    if bad_qual:
        return ERR_QUALITY
    return OK


def message(entry, kind, long_read, index=0):
    """the text FastqEntry::validate throws (kind 6: ours)"""
    header, bases, header2, quals = (x.decode("latin-1") for x in entry)
    m = "Invalid Fastq file entry: "
    if kind == ERR_HEADER:
        return m + "First header line does not start with '@': '" + header + "'."
    if kind == ERR_HEADER2:
        return m + "Second header line does not start with '+': '" + header2 + "'."
    if kind == ERR_LENGTH:
        return m + "Differing length of bases (%d) and qualities string (%d) in sequence '%s'." % (len(bases), len(bases), header)
    if kind == ERR_BASE:
        c = next(x for x in bases if x not in "ACGTN")
        return m + "Invalid base '" + c + "' encountered in sequence '" + header + "'."
    if kind == ERR_QUALITY:
        c = next(x for x in quals if not quality_ok(ord(x), long_read))
        v = ord(c) - 256 if ord(c) > 127 else ord(c)
        return m + "Invalid " + ("nanopore " if long_read else "") + "quality character '" + c + "' with value '" + str(v) + "' encountered in sequence '" + header + "'."
    return m + "Entry %d has an empty header line and bases or qualities that cannot be counted (%d bases, %d qualities)." % (index, len(bases), len(quals))


def mean_bins(q_sum, cycles):
    """(bin of read_qualities_[std::round(mean)], bin of Histogram(0, 60, 1).inc(mean, true), mean)"""
    mean = q_sum / cycles                      # a double division, as :70
    r = int(mean)
    if mean - r >= 0.5:                        # std::round: halves away from zero (mean >= 0)
        r += 1
    v = 0.0 if mean < 0.0 else (60.0 if mean > 60.0 else mean)
    b = int(math.floor((v - 0.0) / (60.0 - 0.0) * 60.0))
    return r, max(0, min(59, b)), mean


class Stats:
    def __init__(self):
        self.c_forward = self.c_reverse = self.bases_sequenced = 0
        self.bases = np.zeros(5, np.int64)
        self.base_qualities = np.zeros(100, np.int64)
        self.read_qualities = np.zeros(100, np.int64)
        self.qscore_dist_r1 = np.zeros(60, np.int64)
        self.qscore_dist_r2 = np.zeros(60, np.int64)
        self.max_cycles = 0
        self.lengths = {}
        self.cycles = np.zeros((RQ_CYC, 7), np.int64)
        self.c_read_q20 = 0

    def update(self, entry, reverse):
        _, bases, _, quals = entry
        n = len(bases)
        if reverse:
            self.c_reverse += 1
        else:
            self.c_forward += 1
        self.bases_sequenced += n
        self.lengths[n] = self.lengths.get(n, 0) + 1
        self.max_cycles = max(self.max_cycles, n)
        if n == 0:
            return
        cls = _BASE_CLASS[np.frombuffer(bases, np.uint8)]
        q = np.frombuffer(quals, np.uint8).astype(np.int64) - 33
        self.bases += np.bincount(cls, minlength=5)[:5]
        self.base_qualities += np.bincount(q, minlength=100)
        w = min(n, RQ_CYC)
        self.cycles[np.arange(w), cls[:w]] += 1
        self.cycles[:w, 6 if reverse else 5] += q[:w]
        r, b, mean = mean_bins(int(q.sum()), n)
        self.read_qualities[r] += 1
        (self.qscore_dist_r2 if reverse else self.qscore_dist_r1)[b] += 1
        if mean >= 20.0:
            self.c_read_q20 += 1

    def length_hist(self):
        h = np.zeros(self.max_cycles + 1, np.int64)
        for l, c in self.lengths.items():
            h[l] = c
        return h

    def fields(self):
        """the fields of ngsqc_read_stats, the read-length histogram and the cycle table"""
        return {"c_forward": self.c_forward, "c_reverse": self.c_reverse, "bases_sequenced": self.bases_sequenced, "bases": self.bases, "base_qualities": self.base_qualities,
                "read_qualities": self.read_qualities, "qscore_dist_r1": self.qscore_dist_r1, "qscore_dist_r2": self.qscore_dist_r2, "max_cycles": self.max_cycles,
                "n_unknown_base": 0, "n_quality_out_of_range": 0, "read_lengths": self.length_hist(), "cycles": self.cycles}


def run(files, long_read=False):
    """files: [(text, reverse)] in the order ReadQC reads them. Returns (Stats, entries with a non-empty header per file, error): error is None or
    (file ordinal, entry, kind, message) of the first entry the reference throws on - the statistics are void then."""
    st = Stats()
    index = []
    for f, (text, reverse) in enumerate(files):
        n_headers = 0
        for i, e in enumerate(entries_of(text)):
            kind = validate(e, long_read)
            if kind:
                return st, index + [n_headers], (f, i, kind, message(e, kind, long_read, i))
            n_headers += len(e[0]) > 0
            st.update(e, reverse)
        index.append(n_headers)
    return st, index, None


def qc_values(st, single_end):
    """StatisticsReads::getResult(): the values that are numbers or text, as (name, text) in the reference's order; doubles with two decimals"""
    out = []
    total_reads = st.c_forward + st.c_reverse
    bases_total = int(st.bases.sum())
    c_base_n, c_base_gc = int(st.bases[4]), int(st.bases[1] + st.bases[2])
    c_base_q20, c_base_q30 = int(st.base_qualities[20:].sum()), int(st.base_qualities[30:].sum())
    keys = sorted(st.lengths)
    longest = keys[-1]
    out.append(("read count", str(total_reads)))
    out.append(("read length", ", ".join(map(str, keys)) if len(keys) < 4 else "%d-%d" % (keys[0], longest)))
    f2 = lambda x: "%.2f" % x
    out.append(("bases sequenced (MB)", f2(st.bases_sequenced / 1000000.0)))
    out.append(("Q20 read percentage", f2(100.0 * st.c_read_q20 / total_reads)))
    out.append(("Q20 base percentage", f2(100.0 * c_base_q20 / bases_total)))
    out.append(("Q30 base percentage", f2(100.0 * c_base_q30 / bases_total)))
    out.append(("no base call percentage", f2(100.0 * c_base_n / bases_total)))
    out.append(("gc content percentage", f2(100.0 * c_base_gc / (bases_total - c_base_n))))
    if single_end:
        bases, n50 = 0, 0
        for k in reversed(keys):
            bases += k * st.lengths[k]
            if bases > st.bases_sequenced // 2:
                n50 = k
                break
        out.append(("N50 read length (bp)", str(n50)))
        max_count, checked, mode_b, median_b = 0, 0, 0, -1
        for i in range(61):
            c = int(st.base_qualities[i])
            if c >= max_count:
                max_count = c
                if i < 50:
                    mode_b = i
            checked += c
            if median_b == -1 and checked * 2 >= st.bases_sequenced:
                median_b = i
        out += [("median base Q score", str(median_b)), ("mode base Q score", str(mode_b))]
        max_count, checked, mode_r, median_r = 0, 0, 0, -1
        for i in range(100):
            c = int(st.read_qualities[i])
            if c >= max_count:
                max_count, mode_r = c, i
            checked += c
            if median_r == -1 and checked * 2 >= st.c_forward:
                median_r = i
        out += [("median read Q score", str(median_r)), ("mode read Q score", str(mode_r))]
    return out
