"""BamCleanHaloplex restated in Python (src/BamCleanHaloplex/main.cpp:27-69), independent of the device: the sequential loop of :41-62 over the records that
bamfilter_oracle.read_bam returns, the record bytes BamWriter::writeAlignment writes (bamfilter_oracle.written) and the three lines of :66-68.

A record is a candidate when it is none of unmapped, secondary, supplementary or duplicate (:44). The CIGAR is the one htslib hands out: a placed record (tid >= 0
and pos >= 0) whose first operation is "l_seq S" and whose CG:B,I tag holds at least n_cigar_op operations is judged on the tag's array (the CG rule of
oracle/bamio.hpp's parse_rec and advbam.Record.effective_cigar, restated in bamfilter_oracle.Rec.cg). Only operations of type M (0) count; '=' and 'X' do not (:51).
A candidate below min_match gets 0x4 and 0x100 set (src/cppNGS/BamReader.h:157-183: XOR where the bit is not yet set; a candidate has neither) and nothing else
changed. The reference's counters and its sum are `int`; Python's integers do not overflow, and the project counts in 64 bits."""
import struct

from bamfilter_oracle import Rec, read_bam, written  # noqa: F401

EXCLUDING = 0x4 | 0x100 | 0x400 | 0x800
FAIL_FLAGS = 0x4 | 0x100
NOT_CANDIDATE, KEPT, FAILED = 0, 1, 2


def sum_m(r):
    return sum(c >> 4 for c in r.effective_cigar() if c & 15 == 0)


def verdict(rec_bytes, min_match):
    r = Rec(rec_bytes)
    if r.flag & EXCLUDING:
        return NOT_CANDIDATE
    return FAILED if sum_m(r) < min_match else KEPT


def verdicts(records, min_match):
    return bytes(verdict(b, min_match) for b in records)


def with_flags(rec_bytes, mask):
    """the record with mask OR-ed into its flag word (bytes 18-19, block_size included)"""
    flag = struct.unpack_from("<H", rec_bytes, 18)[0] | mask
    return rec_bytes[:18] + struct.pack("<H", flag) + rec_bytes[20:]


def clean(records, min_match=30):
    """records: record bytes in file order -> (verdict bytes, output records, dict(reads, candidates, failed))"""
    vd = verdicts(records, min_match)
    out = [with_flags(written(Rec(b)), FAIL_FLAGS if v == FAILED else 0) for b, v in zip(records, vd)]
    return vd, out, dict(reads=len(records), candidates=sum(1 for v in vd if v), failed=sum(1 for v in vd if v == FAILED))


def percent(x, n):
    """QString::number(100.0 * x / n, 'f', 2); 0 / 0 prints as nan"""
    return "nan" if n == 0 else "%.2f" % (100.0 * x / n)


def log_text(c):
    n = c["reads"]
    return ("overall reads: %d\n" % n + "mapped reads : %d (%s%%)\n" % (c["candidates"], percent(c["candidates"], n))
            + "removed reads: %d (%s%%)\n" % (c["failed"], percent(c["failed"], n)))
