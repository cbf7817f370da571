"""A plain Python model of SeqPurge (src/SeqPurge/AnalysisWorker.cpp:79-457 run, :19-77 correctErrors; src/cppNGS/FastqFileStream.cpp:52-117 trimQuality / trimN;
src/SeqPurge/OutputWorker.cpp:36-77 routing and statistics): what one read pair becomes, and the counters of a run. The binomial tail is exact (math.comb,
fractions) and rounded once to double. Test infrastructure: the CPU emulator of csrc/purge_visit.h and the GPU library are compared against it, and it is itself
held to the reference's expected outputs (tests/test_cpu_seqpurge.py)."""
import functools
import math
from fractions import Fraction

import numpy as np

A1_DEFAULT = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
A2_DEFAULT = b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"
MAXLEN = 1000
ADAPTER_OVERLAP = 10
# error kinds of a pair, in the order they are looked for (the lowest pair wins and, within it, the lowest kind)
ERR_LENGTHS, ERR_HEADER, ERR_BASE, ERR_READLEN = 1, 2, 3, 4
PLAN_COLUMNS = ("len1_in", "len2_in", "insert_offset", "adapter_fwd", "adapter_rev", "len1_out", "len2_out", "flags")
COUNTERS = ("read_num", "reads_trimmed_insert", "reads_trimmed_adapter", "reads_trimmed_q", "reads_trimmed_n", "reads_removed")
COMPLEMENT = {65: 84, 67: 71, 71: 67, 84: 65, 78: 78}


class PurgeError(Exception):
    def __init__(self, pair, kind, message):
        super().__init__(message)
        self.pair, self.kind, self.message = pair, kind, message


class Params:
    def __init__(self, a1=A1_DEFAULT, a2=A2_DEFAULT, match_perc=80.0, mep=1e-6, min_len=30, qcut=15, qwin=5, qoff=33, ncut=7, ec=False, out3=False):
        self.a1, self.a2 = bytes(a1), bytes(a2)
        self.match_perc, self.mep, self.min_len = float(match_perc), float(mep), int(min_len)
        self.qcut, self.qwin, self.qoff, self.ncut, self.ec, self.out3 = int(qcut), int(qwin), int(qoff), int(ncut), bool(ec), bool(out3)
        self.a_size = min(20, len(self.a1), len(self.a2))

    def kwargs(self):
        return dict(a1=self.a1, a2=self.a2, match_perc=self.match_perc, mep=self.mep, min_len=self.min_len, qcut=self.qcut, qwin=self.qwin, qoff=self.qoff,
                    ncut=self.ncut, ec=self.ec)


@functools.lru_cache(maxsize=None)
def tail_exact(k, n):
    """BasicStatistics::matchProbability(0.25, k, n): P(X >= k), X ~ Binomial(n, 1/4), as a fraction"""
    return Fraction(sum(math.comb(n, i) * 3 ** (n - i) for i in range(k, n + 1)), 4 ** n)


@functools.lru_cache(maxsize=None)
def tail(k, n):
    return float(tail_exact(k, n))


class Margin:
    """the smallest |p - mep| / mep over every probability that was compared with mep"""
    def __init__(self):
        self.value, self.n = math.inf, 0

    def see(self, p, mep):
        self.n += 1
        if mep > 0:
            self.value = min(self.value, abs(p - mep) / mep)


def parse_fastq(text):
    """the entries of a FASTQ text as the library reads it: '\\n' ends a line, one '\\r' in front of it is dropped, a missing final newline
    is supplied, empty lines at the end are ignored, the missing lines of an incomplete last entry are empty"""
    text = bytes(text)
    if text and not text.endswith(b"\n"):
        text += b"\n"
    lines = [l[:-1] if l.endswith(b"\r") else l for l in text.split(b"\n")[:-1]]
    while lines and lines[-1] == b"":
        lines.pop()
    lines += [b""] * (-len(lines) % 4)
    return [tuple(lines[i:i + 4]) for i in range(0, len(lines), 4)]


def revcomp(pair, r2):
    out = bytearray(len(r2))
    for i, c in enumerate(reversed(r2)):
        if c not in COMPLEMENT:
            raise PurgeError(pair, ERR_BASE, "Could not convert base '%s' to complement!" % chr(c))
        out[i] = COMPLEMENT[c]
    return bytes(out)


def header_token(h):
    return h.split(b" ")[0]


def count3(s, a):
    """matches, mismatches, invalid of s against the front of a (s is not longer than a)"""
    m = x = inv = 0
    for b1, b2 in zip(s, a):
        if b1 == 78 or b2 == 78:
            inv += 1
        elif b1 == b2:
            m += 1
        else:
            x += 1
    return m, x, inv


def insert_counts_literal(seq1, seq2, offset, min_len, match_perc):
    """the reference's loop with its early exit (:146-168)"""
    max_mm = int(math.ceil((1.0 - match_perc / 100.0) * (min_len - offset)))
    m = x = inv = 0
    for j in range(offset, min_len):
        b1, b2 = seq1[j - offset], seq2[j]
        if b1 == 78 or b2 == 78:
            inv += 1
        elif b1 == b2:
            m += 1
        else:
            x += 1
            if x > max_mm:
                break
    return m, x, inv


def _planes(s):
    pl = [0, 0, 0, 0, 0]
    for idx, c in enumerate(b"ACGTN"):
        v, start = 0, s.find(c)
        while start >= 0:
            v |= 1 << start
            start = s.find(c, start + 1)
        pl[idx] = v
    return pl


def insert_counts_planes(p1, p2, offset, min_len):
    """whole counts of an offset from bit planes (bit i: position i): seq1[i] against seq2[i + offset], i < min_len - offset"""
    mask = (1 << (min_len - offset)) - 1
    m = sum((p1[b] & (p2[b] >> offset) & mask).bit_count() for b in range(4))
    inv = ((p1[4] | (p2[4] >> offset)) & mask).bit_count()
    return m, (min_len - offset) - inv - m, inv


def perc_below(m, x, match_perc):
    """100.0*m/(m+x) < match_perc with the reference's doubles (0/0 is NaN: not below)"""
    return (m + x) != 0 and 100.0 * m / (m + x) < match_perc


def trim_quality(quals, cutoff, window, qoff):
    """FastqEntry::trimQuality: the new length"""
    count = len(quals)
    if count < window:
        return count
    q = [c - qoff for c in quals]
    s = 0.0
    for i in range(count - 1, count - window, -1):
        s += q[i]
    for i in range(count - window, -1, -1):
        s += q[i]
        if s / window >= cutoff:
            new = i + window
            while new > 0 and q[new - 1] < cutoff:
                new -= 1
            return new
        s -= q[i + window - 1]
    return 0


def trim_n(bases, num_n):
    """FastqEntry::trimN: the new length"""
    count = len(bases)
    if count < num_n:
        return count
    s = sum(1 for i in range(num_n - 1) if bases[i] == 78)
    for i in range(num_n - 1, count):
        s += bases[i] == 78
        if s == num_n:
            return i - num_n + 1
        s -= bases[i - num_n + 1] == 78
    return count


def adapter_scan(seq, adapter, a_size, P, margin):
    """the first offset at which the front of the adapter is found in seq (:309-353), or -1"""
    n = len(seq)
    for offset in range(n):
        m, x, _ = count3(seq[offset:offset + a_size], adapter)
        if perc_below(m, x, P.match_perc):
            continue
        p = tail(m, m + x)
        margin.see(p, P.mep)
        if p > P.mep:
            continue
        return offset
    return -1


class Stats:
    def __init__(self):
        self.counters = dict.fromkeys(COUNTERS, 0)
        self.bases_remaining = np.zeros(MAXLEN, np.int64)
        self.bases_perc_trim_sum = 0.0
        self.acons = np.zeros((2, 40, 5), np.int64)
        self.ec = np.zeros((3, MAXLEN), np.int64)    # mismatch_r1, mismatch_r2, errors_per_read


def process_pair(pair, e1, e2, P, stats, margin, literal=False):
    """-> (plan row, entry 1, entry 2) after every step; raises PurgeError"""
    h1, b1, g1, q1 = e1
    h2, b2, g2, q2 = e2
    if len(b1) != len(q1) or len(b2) != len(q2):
        which = 1 if len(b1) != len(q1) else 2
        bb, qq, hh = (b1, q1, h1) if which == 1 else (b2, q2, h2)
        raise PurgeError(pair, ERR_LENGTHS, "Differing length of bases (%d) and qualities (%d) in read %d of pair %d: '%s'." % (len(bb), len(qq), which, pair, hh.decode("latin-1")))
    t1, t2 = header_token(h1), header_token(h2)
    if t1.endswith(b"/1") and t2.endswith(b"/2"):
        t1, t2 = t1[:-2], t2[:-2]
    if t1 != t2:
        raise PurgeError(pair, ERR_HEADER, "Headers of reads do not match:\n%s\n%s" % (t1.decode("latin-1"), t2.decode("latin-1")))
    seq1, seq2 = b1, revcomp(pair, b2)
    len1, len2 = len(seq1), len(seq2)
    min_len, max_len = min(len1, len2), max(len1, len2)
    if max_len >= MAXLEN:
        raise PurgeError(pair, ERR_READLEN, "Read length unsupported! A maximum read length of %d is supported!" % MAXLEN)
    best_offset, best_p = -1, 1.0
    pl1, pl2 = (None, None) if literal else (_planes(seq1), _planes(seq2))
    for offset in range(1, min_len):
        if literal:
            m, x, _ = insert_counts_literal(seq1, seq2, offset, min_len, P.match_perc)
        else:
            m, x, _ = insert_counts_planes(pl1, pl2, offset, min_len)
            if x > int(math.ceil((1.0 - P.match_perc / 100.0) * (min_len - offset))):
                continue
        if (m + x) == 0 or perc_below(m, x, P.match_perc):
            continue
        p = tail(m, m + x)
        margin.see(p, P.mep)
        if p > P.mep:
            continue
        am1, ax1, _ = count3(seq1[len2 - offset:len2 - offset + ADAPTER_OVERLAP], P.a1)
        am2, ax2, _ = count3(b2[len2 - offset:len2 - offset + ADAPTER_OVERLAP], P.a2)
        if offset < 10:
            max_mm = 0 if offset < 3 else 1 if offset < 6 else 2
            if not (ax1 <= max_mm or ax2 <= max_mm):
                continue
        else:
            pp = tail(am1, am1 + ax1) * tail(am2, am2 + ax2)
            margin.see(pp, P.mep)
            if pp > P.mep:
                continue
        if p < best_p:
            best_p, best_offset = p, offset
    b1, q1, b2, q2 = bytearray(b1), bytearray(q1), bytearray(b2), bytearray(q2)
    fwd = rev = -1
    c = stats.counters
    if best_offset != -1:
        new_len = len2 - best_offset
        for k, ch in enumerate(seq1[new_len:new_len + 40]):
            if ch in b"ACGTN":
                stats.acons[0, k, b"ACGTN".index(ch)] += 1
        for k, ch in enumerate(bytes(b2[len2 - best_offset:len2 - best_offset + 40])):
            stats.acons[1, k, b"ACGTN".index(ch)] += 1
        del b1[new_len:], q1[new_len:], b2[new_len:], q2[new_len:]
        c["reads_trimmed_insert"] += 2
        if P.ec:
            count, mm = min(len(b1), len(b2)), 0
            for i in range(count):
                i2 = count - i - 1
                if b1[i] != COMPLEMENT[b2[i2]]:
                    mm += 1
                    v1, v2 = q1[i] - P.qoff, q2[i2] - P.qoff
                    if v1 > v2:
                        b2[i2] = COMPLEMENT.get(b1[i], 78); q2[i2] = q1[i]
                        stats.ec[1, i2] += 1
                    elif v1 < v2:
                        b1[i] = COMPLEMENT[b2[i2]]; q1[i] = q2[i2]
                        stats.ec[0, i] += 1
            if mm > 0:
                stats.ec[2, mm] += 1
    else:
        fwd = adapter_scan(seq1, P.a1, P.a_size, P, margin)
        rev = adapter_scan(bytes(b2), P.a2, P.a_size, P, margin)
        if fwd != -1 or rev != -1:
            c["reads_trimmed_adapter"] += 2
            cut1, cut2 = (fwd if fwd != -1 else rev), (rev if rev != -1 else fwd)
            del b1[cut1:], q1[cut1:], b2[cut2:], q2[cut2:]
    flags = 0
    if P.qcut > 0:
        for bit, (b, q) in enumerate(((b1, q1), (b2, q2))):
            new = trim_quality(q, P.qcut, P.qwin, P.qoff)
            if new < len(q):
                flags |= 1 << bit; c["reads_trimmed_q"] += 1
                del b[new:], q[new:]
    if P.ncut > 0:
        for bit, (b, q) in enumerate(((b1, q1), (b2, q2))):
            new = trim_n(b, P.ncut)
            if new < len(b):
                flags |= 4 << bit; c["reads_trimmed_n"] += 1
                del b[new:], q[new:]
    row = (len1, len2, best_offset, fwd, rev, len(b1), len(b2), flags)
    return row, (h1, bytes(b1), g1, bytes(q1)), (h2, bytes(b2), g2, bytes(q2))


def entry_text(e):
    return b"".join(l + b"\n" for l in e)


class Result:
    pass


def run(text1, text2, P, literal=False, name1="in1", name2="in2"):
    """a whole run over one file pair: .plan (n, 8) int32, .out [out1, out2, out3_R1, out3_R2] texts, .stats, .margin, .error (PurgeError or None: the outputs
    and statistics then hold the pairs in front of it)"""
    E1, E2 = parse_fastq(text1), parse_fastq(text2)
    r = Result()
    r.stats, r.margin, r.error = Stats(), Margin(), None
    rows, out = [], [[], [], [], []]
    c = r.stats.counters
    for i in range(min(len(E1), len(E2))):
        try:
            row, o1, o2 = process_pair(i, E1[i], E2[i], P, r.stats, r.margin, literal)
        except PurgeError as e:
            r.error = e
            break
        rows.append(row)
        l1, l2 = row[5], row[6]
        if l1 >= P.min_len and l2 >= P.min_len:
            out[0].append(entry_text(o1)); out[1].append(entry_text(o2))
        elif P.out3 and l1 >= P.min_len:
            c["reads_removed"] += 1; out[2].append(entry_text(o1))
        elif P.out3 and l2 >= P.min_len:
            c["reads_removed"] += 1; out[3].append(entry_text(o2))
        else:
            c["reads_removed"] += 2
        c["read_num"] += 2
        r.stats.bases_remaining[l1] += 1; r.stats.bases_remaining[l2] += 1
        if row[0] > 0:
            r.stats.bases_perc_trim_sum += (row[0] - l1) / row[0]
        if row[1] > 0:
            r.stats.bases_perc_trim_sum += (row[1] - l2) / row[1]
    if r.error is None and len(E1) != len(E2):
        a, b = (name2, name1) if len(E2) > len(E1) else (name1, name2)
        r.error = PurgeError(min(len(E1), len(E2)), 0, "File %s has more entries than %s!" % (a, b))
    r.plan = np.array(rows, np.int32).reshape(-1, 8)
    r.out = [b"".join(o) for o in out]
    return r


def _consensus(pile):
    s = b""
    for i in range(40):
        a, c, g, t, _ = (int(v) for v in pile[i])
        depth = a + c + g + t
        if depth < 20:
            break
        mx = max(a, c, g, t)
        if mx / depth <= 0.5:
            s += b"N"
        elif a == mx:
            s += b"A"
        elif c == mx:
            s += b"C"
        elif g == mx:
            s += b"G"
        else:
            s += b"T"
    return s.decode()


def _perc(x, n):
    return "nan" if n == 0 else "%.2f" % (100.0 * x / n)


def summary_text(stats, P):
    """TrimmingStatistics::writeStatistics (Auxilary.h:166-221) and, with -ec, ErrorCorrectionStatistics::writeStatistics (:238-269) - without the timestamped
    lines. A histogram that is all zero prints its heading and no rows (the reference walks below index 0 there)."""
    c, n = stats.counters, stats.counters["read_num"]
    out = ["Reads (forward + reverse): %d" % n, "",
           "Reads trimmed by insert match: %d" % c["reads_trimmed_insert"], "Reads trimmed by adapter match: %d" % c["reads_trimmed_adapter"],
           "Reads trimmed by quality: %d" % c["reads_trimmed_q"], "Reads trimmed by N stretches: %d" % c["reads_trimmed_n"]]
    trimmed = c["reads_trimmed_insert"] + c["reads_trimmed_adapter"]
    out += ["Trimmed reads: %d of %d (%s%%)" % (trimmed, n, _perc(trimmed, n)), "Removed reads: %d of %d (%s%%)" % (c["reads_removed"], n, _perc(c["reads_removed"], n)),
            "Removed bases: %s%%" % _perc(stats.bases_perc_trim_sum, n), "",
            "Forward adapter sequence (given)    : " + P.a1.decode(), "Forward adapter sequence (consensus): " + _consensus(stats.acons[0]),
            "Reverse adapter sequence (given)    : " + P.a2.decode(), "Reverse adapter sequence (consensus): " + _consensus(stats.acons[1]), "",
            "Read length distribution after trimming:"]

    def rows(hist, first):
        nz = np.nonzero(hist)[0]
        return ["%4d: %d" % (i, hist[i]) for i in range(first, int(nz[-1]) + 1)] if len(nz) else []
    out += rows(stats.bases_remaining, 0)
    if P.ec:
        for title, h in (("Read error per cycle (read 1):", stats.ec[0]), ("Read error per cycle (read 2):", stats.ec[1]), ("Read error count distribution:", stats.ec[2])):
            out += ["", title] + rows(h, 1)
    return "\n".join(out) + "\n"
