"""Hand-built BAMs from a record list, and two sequential models of what the record list must give (CPU only).

build()        (flag, bases, quals[, mapq]) per record -> a coordinate-sorted BAM on chr1 (distinct names, tid 0, increasing pos, CIGAR `l_seq M`,
               none for l_seq = 0), laid into BGZF members of the chosen sizes (rebgzf of test_gpu_inflate). Any 4-bit base code and any quality byte
               can be written. The records are laid out with numpy (no per-record struct.pack), so 3e5 short records take well under a second.
reads_model()  StatisticsReads::update(const BamAlignment&) (src/cppNGS/StatisticsReads.cpp:83-158) restated from the record list, in the dict layout
               of Handle.scan_reads(). Integers only; the per-read mean is a fractions.Fraction, so "exactly .5" and "exactly 60" are decided exactly.
carry_model()  the two order-dependent carries of the mapping loop (running maximum read length behind bases_trimmed, Statistics.cpp:428-429,565-568;
               "a paired read has been seen" behind bases_usable_no_overlap, :879,:1115) as the sequential loop they are in the reference.

Columns is the same record list in columnar form (what the large files are generated as); every function here takes either."""
from collections import namedtuple
from fractions import Fraction

import numpy as np

REF_NAME, REF_LEN, POS0 = b"chr1", 248956422, 16_000_000
NIBBLE = {"A": 1, "C": 2, "G": 4, "T": 8, "N": 15}
KNOWN = (1, 2, 4, 8, 15)                                                   # baseIntegers(): every other nibble is "Unknown base"
UNKNOWN = tuple(x for x in range(16) if x not in KNOWN)
N_CYC = 320
L_NAME = 9                                                                 # 'r' + 7 digits + NUL
CARRY_COUNTERS = ((0, "n"), (7, "trimmed"), (12, "no_overlap"), (24, "gmax"), (25, "paired"))   # index in the mapping counters -> key of carry_model()

Columns = namedtuple("Columns", "flags lens bases quals mapq")            # bases / quals: all records' cycles in one flat array each


def columns(records):
    if isinstance(records, Columns):
        return records
    n = len(records)
    flags = np.fromiter((r[0] for r in records), dtype=np.int64, count=n)
    lens = np.fromiter((len(r[1]) for r in records), dtype=np.int64, count=n)
    mapq = np.fromiter((r[3] if len(r) > 3 else 60 for r in records), dtype=np.int64, count=n)
    for r in records:
        assert len(r[1]) == len(r[2]), "one quality per base"
    cat = lambda k: np.concatenate([np.asarray(r[k], dtype=np.uint8) for r in records]) if n else np.zeros(0, dtype=np.uint8)
    return Columns(flags, lens, cat(1), cat(2), mapq)


def _reg2bin(beg, end):
    end = end - 1
    out = np.zeros(beg.size, dtype=np.int64); done = np.zeros(beg.size, dtype=bool)
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        m = ~done & ((beg >> shift) == (end >> shift))
        out[m] = first + (beg[m] >> shift); done |= m
    return out


_FIXED = np.dtype([("block_size", "<i4"), ("tid", "<i4"), ("pos", "<i4"), ("l_name", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("n_cigar", "<u2"), ("flag", "<u2"),
                   ("l_seq", "<i4"), ("mtid", "<i4"), ("mpos", "<i4"), ("tlen", "<i4"), ("name", "u1", (L_NAME,))])


def build_raw(records, pos_step=3):
    """The uncompressed BAM stream and the offset of every record's block_size field in it."""
    c = columns(records)
    n = c.flags.size
    assert n < 10 ** 7 and c.bases.size == c.quals.size == int(c.lens.sum())
    text = b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:" + REF_NAME + b"\tLN:%d\n" % REF_LEN
    head = (b"BAM\x01" + np.int32(len(text)).tobytes() + text + np.int32(1).tobytes() + np.int32(len(REF_NAME) + 1).tobytes() + REF_NAME + b"\x00"
            + np.int32(REF_LEN).tobytes())
    lens = c.lens.astype(np.int64)
    has_cig = (lens > 0).astype(np.int64)
    seq_bytes = (lens + 1) // 2
    body = 32 + L_NAME + 4 * has_cig + seq_bytes + lens                    # what block_size says
    off = len(head) + np.concatenate([[0], np.cumsum(body + 4)])
    out = np.zeros(int(off[-1]), dtype=np.uint8)
    out[:len(head)] = np.frombuffer(head, dtype=np.uint8)
    off = off[:-1]
    if n == 0:
        return out.tobytes(), off
    idx = np.arange(n, dtype=np.int64)
    pos = POS0 + pos_step * idx
    fx = np.zeros(n, dtype=_FIXED)
    fx["block_size"] = body; fx["tid"] = 0; fx["pos"] = pos; fx["l_name"] = L_NAME; fx["mapq"] = c.mapq
    fx["bin"] = _reg2bin(pos, pos + np.maximum(lens, 1)); fx["n_cigar"] = has_cig; fx["flag"] = c.flags; fx["l_seq"] = lens
    fx["mtid"] = -1; fx["mpos"] = -1; fx["tlen"] = 0
    fx["name"][:, 0] = ord("r")
    fx["name"][:, 1:8] = (idx[:, None] // 10 ** np.arange(6, -1, -1)) % 10 + ord("0")
    w = _FIXED.itemsize
    out[off[:, None] + np.arange(w)] = fx.view(np.uint8).reshape(n, w)
    cig = np.flatnonzero(has_cig)
    out[(off[cig] + w)[:, None] + np.arange(4)] = (lens[cig] << 4).astype("<u4").view(np.uint8).reshape(-1, 4)       # op 0 = M
    # SEQ: two bases per byte, high nibble first; an odd length leaves the low nibble of its last byte zero
    seq0 = off + w + 4 * has_cig
    rec_of = np.repeat(idx, lens)
    cyc = np.arange(rec_of.size, dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
    nib0 = 2 * (np.cumsum(seq_bytes) - seq_bytes)
    nib = np.zeros(2 * int(seq_bytes.sum()), dtype=np.uint8)
    nib[nib0[rec_of] + cyc] = c.bases & 15
    byte_of = np.repeat(idx, seq_bytes)
    k = np.arange(byte_of.size, dtype=np.int64) - np.repeat(np.cumsum(seq_bytes) - seq_bytes, seq_bytes)
    out[seq0[byte_of] + k] = (nib[0::2] << 4) | nib[1::2]
    out[(seq0 + seq_bytes)[rec_of] + cyc] = c.quals
    return out.tobytes(), off


def build(records, member_sizes=(60000,), pos_step=3, **kw):
    """BGZF bytes of the BAM. member_sizes: uncompressed bytes per member, cycled (records straddle the members wherever a size says so)."""
    from test_gpu_inflate import rebgzf                                    # (here, not at the top: the models need neither the package nor the generator)
    raw, _ = build_raw(records, pos_step)
    return rebgzf(raw, list(member_sizes), **kw)


def write(path, records, member_sizes=(60000,), **kw):
    with open(path, "wb") as f:
        f.write(build(records, member_sizes, **kw))
    return path


# ---- StatisticsReads::update ----
def reads_model(records, single_end):
    """Dict in the layout of Handle.scan_reads() (plus the three q20 / q30 counters the oracle reports). Records with a nibble outside A, C, G, T, N
    or a quality >= 100 are COUNTED (n_unknown_base / n_quality_out_of_range: records, not bases) and left out of everything else: the reference throws
    on them, so the remaining counters are only defined - and only compared - for files that hold none."""
    c = columns(records)
    out = dict(c_forward=0, c_reverse=0, bases_sequenced=0, c_read_q20=0, c_base_q20=0, c_base_q30=0, max_cycles=0, n_unknown_base=0, n_quality_out_of_range=0)
    bases = [0] * 5
    base_q, read_q, qd = [0] * 100, [0] * 100, ([0] * 60, [0] * 60)
    lengths = {}
    cycles = np.zeros((N_CYC, 7), dtype=np.int64)
    start = 0
    for flag, ln, in zip(c.flags.tolist(), c.lens.tolist()):
        b = c.bases[start:start + ln].astype(np.int64); q = c.quals[start:start + ln].astype(np.int64); start += ln
        if flag & (0x100 | 0x800):                                         # :86
            continue
        bad_b, bad_q = bool(np.isin(b, UNKNOWN).any()), bool((q >= 100).any())
        out["n_unknown_base"] += bad_b; out["n_quality_out_of_range"] += bad_q
        if bad_b or bad_q:
            continue
        fwd = True if single_end else bool(flag & 0x40)                    # :90-106
        out["c_forward" if fwd else "c_reverse"] += 1
        out["bases_sequenced"] += ln
        lengths[ln] = lengths.get(ln, 0) + 1
        out["max_cycles"] = max(out["max_cycles"], ln)
        for k, code in enumerate(KNOWN):
            hit = b == code
            bases[k] += int(hit.sum())
            cycles[:min(ln, N_CYC), k] += hit[:N_CYC]
        cycles[:min(ln, N_CYC), 5 if fwd else 6] += q[:N_CYC]
        for v, cnt in zip(*np.unique(q, return_counts=True)):
            base_q[int(v)] += int(cnt)
        out["c_base_q20"] += int((q >= 20).sum()); out["c_base_q30"] += int((q >= 30).sum())
        if ln == 0:
            continue                                                       # mean = 0 / 0: nothing more is counted (zero-length reads)
        qsum = int(q.sum())
        mean = Fraction(qsum, ln)
        rounded = (2 * mean.numerator + mean.denominator) // (2 * mean.denominator)   # std::round: half away from zero (mean >= 0)
        read_q[rounded] += 1
        clamped = min(max(mean, Fraction(0)), Fraction(60))                # Histogram(0, 60, 1).inc(mean, true)
        qd[0 if fwd else 1][min(clamped.numerator // clamped.denominator, 59)] += 1
        out["c_read_q20"] += mean >= 20
    lens = np.zeros(out["max_cycles"] + 1, dtype=np.int64)
    for ln, cnt in lengths.items():
        lens[ln] = cnt
    out.update(bases=np.array(bases, dtype=np.int64), base_qualities=np.array(base_q, dtype=np.int64), read_qualities=np.array(read_q, dtype=np.int64),
               qscore_dist_r1=np.array(qd[0], dtype=np.int64), qscore_dist_r2=np.array(qd[1], dtype=np.int64), read_lengths=lens, cycles=cycles)
    return out


def assert_reads_equal(got, want, keys=None, what=""):
    """Key by key, exact. keys: default every key of `got` that `want` has."""
    for k in (keys or [k for k in got if k in want]):
        g, w = got[k], want[k]
        if isinstance(w, np.ndarray) or isinstance(g, np.ndarray):
            g, w = np.asarray(g), np.asarray(w)
            assert g.shape == w.shape, (what, k, g.shape, w.shape)
            bad = np.argwhere(g != w)
            assert bad.size == 0, (what, k, [(tuple(i), int(g[tuple(i)]), int(w[tuple(i)])) for i in bad[:5]])
        else:
            assert int(g) == int(w), (what, k, int(g), int(w))


# ---- the order-dependent carries ----
def sequential(recs):
    """recs: int array [n, 4] = (length, counted, passing, paired). Reference order semantics."""
    runmax, paired_seen, trimmed, no_overlap, n_counted = 0, False, 0, 0, 0
    for ln, counted, passing, paired in recs:
        if not counted:
            continue
        n_counted += 1
        runmax = max(runmax, ln)
        trimmed += runmax - ln
        if paired:
            paired_seen = True
        if passing and paired_seen:
            no_overlap += ln
    return dict(n=n_counted, trimmed=trimmed, no_overlap=no_overlap, gmax=runmax, paired=int(paired_seen))


def carry_rows(records, min_mapq=1, nonspecial=(True,)):
    """(length, counted, passing, paired) per record: counted = neither secondary nor supplementary; passing = mapped to a non-special chromosome,
    no duplicate, MAPQ >= min_mapq (every record here is on tid 0). No record of these files is a proper pair, so nothing is taken off for mate overlap."""
    c = columns(records)
    assert not (c.flags & 0x2).any()
    counted = (c.flags & (0x100 | 0x800)) == 0
    passing = counted & ((c.flags & 0x4) == 0) & bool(nonspecial[0]) & ((c.flags & 0x400) == 0) & (c.mapq >= min_mapq)
    paired = counted & ((c.flags & 0x1) != 0)
    return np.stack([c.lens, counted, passing, paired], axis=1).astype(np.int64)


def carry_model(records, min_mapq=1, nonspecial=(True,)):
    """n (al_total), trimmed (bases_trimmed), no_overlap (bases_usable_no_overlap), gmax (max_length), paired (paired_end): CARRY_COUNTERS."""
    return sequential(carry_rows(records, min_mapq, nonspecial).tolist())
