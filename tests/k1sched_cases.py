"""Inputs of the tile-schedule tests (test_gpu_k1_schedule.py, test_gpu_crc_late.py): small hand-built BAMs whose member layout and
record sizes are chosen by the test, and the job every one of those tests runs (MappingQC -wgs over a small BED)."""
import struct
import zlib

import numpy as np

import hostprep as H
import oracle_lib as O

SKIP = {O.COUNTER_NAMES.index("half_depth"), O.COUNTER_NAMES.index("bases_covered_half")}
BED_TEXT = "chr1\t900\t1500\nchr1\t1650\t1900\nchr1\t2500\t40000\n"
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def header():
    text = b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:248956422\n"
    return b"BAM\x01" + struct.pack("<I", len(text)) + text + struct.pack("<I", 1) + struct.pack("<I", 5) + b"chr1\0" + struct.pack("<I", 248956422)


def record(name, pos, l_seq, rng, flag=0, mapq=60):
    nm = name + b"\0"; cigar = struct.pack("<I", (l_seq << 4) | 0)
    qual = bytes(rng.integers(2, 41, l_seq, dtype=np.uint8)); seq = bytes((l_seq + 1) // 2)
    body = struct.pack("<iiBBHHHiiii", 0, pos, len(nm), mapq, 4680, 1, flag, l_seq, -1, -1, 0) + nm + cigar + seq + qual
    return struct.pack("<I", len(body)) + body


def member(payload, level=6):
    co = zlib.compressobj(level, zlib.DEFLATED, -15); comp = co.compress(payload) + co.flush()
    assert len(comp) + 26 <= 65536
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload)))


def bam(members, level=6):
    """the BGZF file of these payloads, one member each, plus the EOF member"""
    return b"".join(member(m, level) for m in members) + EOF_MEMBER


def records_bam(lengths, seed, level=6, per_member=None):
    """header in a member of its own, then the records (SEQ lengths as given, ascending positions); a member per record unless per_member says otherwise.
    Records longer than a member are cut into pieces of 60000 bytes (they then straddle members, as in a long-read file)."""
    rng = np.random.default_rng(seed)
    recs = [record(b"r%05d" % i, 1000 + 7 * i, n, rng) for i, n in enumerate(lengths)]
    members = [header()]
    step = per_member or 1
    for i in range(0, len(recs), step):
        blob = b"".join(recs[i:i + step])
        members += [blob[k:k + 60000] for k in range(0, len(blob), 60000)]
    return bam(members, level)


def job(ngsqc, h, bed_path, sites=None):
    regs, _ = H.bed_regions(bed_path, h.refs, 3); tx, ty = H.xy_tids(h.refs)
    mp = dict(mode=ngsqc.MODE_WGS, regions=regs, min_mapq=1, tid_x=tx, tid_y=ty, nonspecial=H.nonspecial(h.refs))
    return h.run_job(mapping=mp, sites=sites) if sites is not None else h.run_job(mapping=mp)


def assert_counters(counters, exp):
    for i in range(len(counters)):
        if i not in SKIP:
            assert int(counters[i]) == int(exp.counters[i]), (i, int(counters[i]), int(exp.counters[i]))
