"""Designed and random read pairs for BamClipOverlap (tests/test_cpu_bamclipoverlap_emul.py compares ngs-bits_amd/csrc/clip_visit.h, compiled for the CPU, with
the literal restatement tests/bamclipoverlap_oracle.py on them; tests/test_gpu_bamclipoverlap.py the device on a BAM made of them).

designed_pairs() -> [(label, opener bytes, closer bytes)]: the six geometric branches, odd overlaps with read1 on either side, indels around the clip position,
insertions against matches and deletions, clips that end inside an I or a D, hard and soft clips at both ends, a mate clipped to all-S, one-base reads.
random_pairs(n, seed) -> the same triples: CIGARs of 1 to 12 operations over M, I, D, S, H, reads of 1 to 40 bases; a few carry what the reference throws on
(error_pairs() reaches every reachable error on purpose). designed_file() -> the records of a BAM of about 600 records for the device tests."""
import random
import struct

from rmvar_cases import NT16, OPS, bam_bytes, cigar_ops  # noqa: F401

REFS = [("chr1", 2_000_000), ("chr2", 2_000_000)]
_rng = random.Random(5)
GENOME = "".join(_rng.choice("ACGT") for _ in range(4000))   # the bases a clean read shows at a 0-based position


def record(name, flag, tid, pos, cigar, seq=None, qual=None, mtid=None, mpos=0, isize=0, aux=b"", mapq=60, cg=None, bin_=4680):
    """cigar: "20M2I18M" or [(length, operation number)]; seq None: the genome's bases along the CIGAR, insertions and soft clips 'T' / 'G'"""
    ops = cigar_ops(cigar) if isinstance(cigar, str) else list(cigar or [])
    if seq is None:
        seq, g = "", pos
        for n, o in ops:
            if o in (0, 7, 8): seq += GENOME[g:g + n]; g += n
            elif o in (2, 3): g += n
            elif o == 1: seq += "T" * n
            elif o == 4: seq += "G" * n
    if cg is not None:
        real = cigar_ops(cg) if isinstance(cg, str) else list(cg)
        aux = aux + b"CGBI" + struct.pack("<I", len(real)) + b"".join(struct.pack("<I", n << 4 | o) for n, o in real)
        ops = [(len(seq), 4), (sum(n for n, o in real if o in (0, 2, 3, 7, 8)) or 1, 3)]
    qual = bytes(20 + (i * 7 + len(name)) % 21 for i in range(len(seq))) if qual is None else qual
    nm = name.encode() + b"\0"
    nib = [NT16.index(c) for c in seq] + [0]
    sq = bytes(nib[i] << 4 | nib[i + 1] for i in range(0, len(seq), 2))
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(nm), mapq, bin_, len(ops), flag, len(seq), tid if mtid is None else mtid, mpos, isize) + nm
    body += b"".join(struct.pack("<I", (n << 4 | o) & 0xffffffff) for n, o in ops) + sq + qual + aux
    return struct.pack("<I", len(body)) + body


def mutate(seq, at, to=None):
    c = to or {"A": "C", "C": "G", "G": "T", "T": "A"}.get(seq[at], "A")
    return seq[:at] + c + seq[at + 1:]


def genome_seq(pos, cigar):
    r = record("x", 0, 0, pos, cigar)
    l_seq = struct.unpack_from("<i", r, 20)[0]
    o = 36 + r[12] + 4 * struct.unpack_from("<H", r, 16)[0]
    return "".join(NT16[(r[o + (i >> 1)] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq))


def pair(label, a, b, tid=0):
    """a / b: (flag bits beyond 'paired', pos, cigar[, keyword arguments of record()]) of the opener and the closer"""
    out = []
    for flag, pos, cigar, *kw in (a, b):
        out.append(record("d_" + label, 1 | flag, tid, pos, cigar, aux=b"NMC\1XSZab\0", **(kw[0] if kw else {})))
    return (label, out[0], out[1])


F1, R1, F2, R2 = 0x40, 0x40 | 0x10, 0x80, 0x80 | 0x10   # read1 / read2 on the forward / reverse strand


def designed_pairs():
    P = []
    # the six geometric branches (:137-192), and no overlap at all
    P.append(pair("left", (F1, 100, "30M"), (R2, 110, "30M")))
    P.append(pair("right", (F1, 110, "30M"), (R2, 100, "30M")))
    P.append(pair("fwd_in_rev", (F1, 105, "10M"), (R2, 100, "30M")))
    P.append(pair("rev_in_fwd", (F1, 100, "30M"), (R2, 105, "10M")))
    P.append(pair("same_opener_inside", (F1, 105, "10M"), (F2, 100, "30M")))
    P.append(pair("same_closer_inside", (R1, 100, "30M"), (R2, 105, "10M")))
    P.append(pair("apart", (F1, 100, "30M"), (R2, 200, "30M")))
    P.append(pair("touching", (F1, 100, "30M"), (R2, 130, "30M")))
    P.append(pair("closer_is_forward", (R1, 110, "30M"), (F2, 100, "30M")))
    P.append(pair("same_strand_left", (F1, 100, "30M"), (F2, 110, "30M")))
    P.append(pair("equal_spans", (F1, 100, "30M"), (R2, 100, "30M")))
    P.append(pair("equal_spans_same_strand", (F1, 100, "30M"), (F2, 100, "30M")))
    # odd overlaps: the odd base goes to read1, on either side and in every halving branch
    P.append(pair("odd_read1_forward", (F1, 100, "30M"), (R2, 119, "30M")))
    P.append(pair("odd_read1_reverse", (F2, 100, "30M"), (R1, 119, "30M")))
    P.append(pair("odd_right_read1_reverse", (F2, 111, "30M"), (R1, 100, "30M")))
    P.append(pair("odd_inside_read1_forward", (F1, 105, "11M"), (R2, 100, "30M")))
    P.append(pair("odd_inside_read1_reverse", (F2, 100, "30M"), (R1, 105, "11M")))
    # mismatches: one base, two bases of one byte, the first and the last base of the overlap, an N
    s = genome_seq(110, "30M")
    for label, seq in (("mm_one", mutate(s, 7)), ("mm_same_byte", mutate(mutate(s, 6), 7)), ("mm_edges", mutate(mutate(s, 0), 19)), ("mm_n", mutate(s, 5, "N")),
                       ("mm_ambiguous_patched", mutate(s, 5, "R")), ("mm_three_in_a_row", mutate(mutate(mutate(s, 9), 10), 11))):
        P.append(pair(label, (F1, 100, "30M"), (R2, 110, "30M", dict(seq=seq))))
    # an indel within +-4 of the clip position (forward clip position 120, reverse 120), and at exactly +-5
    for at in (15, 16, 20, 24, 25):
        P.append(pair(f"ins_fwd_{at}", (F1, 100, f"{at}M1I{30 - at}M"), (R2, 110, "30M")))
        P.append(pair(f"del_fwd_{at}", (F1, 100, f"{at}M1D{29 - at}M"), (R2, 110, "30M")))
    for at in (5, 6, 10, 14, 15):
        P.append(pair(f"ins_rev_{at}", (F1, 100, "30M"), (R2, 110, f"{at}M1I{30 - at}M")))
        P.append(pair(f"del_rev_{at}", (F1, 100, "30M"), (R2, 110, f"{at}M2D{28 - at}M")))
    P.append(pair("long_del_reaches_window", (F1, 100, "8M10D12M"), (R2, 110, "30M")))
    # insertion against match, deletion against insertion, the same insertion on both sides, an insertion on the overlap's first and last base
    P.append(pair("ins_vs_match", (F1, 100, "13M2I15M"), (R2, 110, "30M")))
    P.append(pair("match_vs_ins", (F1, 100, "30M"), (R2, 110, "3M2I25M")))
    P.append(pair("del_vs_ins", (F1, 100, "13M2D15M"), (R2, 110, "3M2I25M")))
    P.append(pair("ins_both", (F1, 100, "13M2I15M"), (R2, 110, "3M2I25M")))
    P.append(pair("ins_both_other_length", (F1, 100, "13M3I14M"), (R2, 110, "3M1I26M")))
    P.append(pair("del_both", (F1, 100, "13M2D15M"), (R2, 110, "3M2D25M")))
    P.append(pair("del_vs_match", (F1, 100, "13M2D15M"), (R2, 110, "30M")))
    P.append(pair("ins_at_overlap_start", (F1, 100, "10M2I18M"), (R2, 110, "30M")))
    P.append(pair("ins_at_overlap_start_rev", (F1, 100, "30M"), (R2, 110, "2I28M")))
    P.append(pair("ins_before_last_base", (F1, 100, "29M2I1M"), (R2, 110, "30M")))
    P.append(pair("ins_at_read_end", (F1, 100, "30M2I"), (R2, 110, "30M")))
    # clips that end inside a D or next to an I (the clean-up around S), with and without the indel detection
    P.append(pair("clip_ends_in_del_fwd", (F1, 100, "18M5D7M"), (R2, 110, "30M")))
    P.append(pair("clip_ends_in_del_rev", (F1, 100, "30M"), (R2, 110, "8M5D17M")))
    P.append(pair("clip_ends_at_ins_fwd", (F1, 100, "20M3I7M"), (R2, 110, "30M")))
    P.append(pair("clip_ends_at_ins_rev", (F1, 100, "30M"), (R2, 110, "10M3I17M")))
    P.append(pair("ins_del_in_front_of_clip", (F1, 100, "17M2I2D9M"), (R2, 110, "30M")))
    P.append(pair("del_at_read_start_rev", (F1, 100, "30M"), (R2, 110, "2S3D27M")))
    P.append(pair("split_matches_merge", (F1, 100, "10M5M15M"), (R2, 110, "12M0M18M")))
    # hard and soft clips in front and behind
    P.append(pair("hard_soft_both_ends", (F1, 100, "3H2S30M4S1H"), (R2, 110, "1H4S30M2S3H")))
    P.append(pair("soft_then_ins", (F1, 100, "2S28M2I"), (R2, 110, "2I28M2S")))
    P.append(pair("hard_only_ends", (F1, 100, "5H30M"), (R2, 110, "30M5H")))
    # a mate clipped to all-S (same strand, one inside the other), with indels and clips inside it
    P.append(pair("all_s_plain", (F1, 105, "10M"), (F2, 100, "30M")))
    P.append(pair("all_s_with_indels", (F1, 105, "2S3M1I2D4M2S1H"), (F2, 100, "30M")))
    P.append(pair("all_s_closer", (R1, 100, "30M"), (R2, 105, "1H3M2D5M")))
    P.append(pair("all_d_read", (F1, 105, "3H4D", dict(seq="")), (F2, 100, "30M")))
    P.append(pair("only_d_read", (F1, 105, "4D", dict(seq="")), (F2, 100, "30M")))
    # one-base reads, and a read of one reference base (start == end)
    P.append(pair("one_base_both", (F1, 100, "1M"), (R2, 100, "1M")))
    P.append(pair("one_base_in_long", (F1, 110, "1M"), (R2, 100, "30M")))
    P.append(pair("one_base_same_strand", (F1, 110, "1M"), (F2, 100, "30M")))
    P.append(pair("one_ref_base_with_ins", (F1, 110, "2I1M2I"), (R2, 100, "30M")))
    P.append(pair("reverse_clipped_to_one", (F1, 100, "30M"), (R2, 128, "3M")))
    # the CIGAR runs past the sequence (the reference reads behind its arrays; here: a base of its own)
    P.append(pair("cigar_longer_than_seq", (F1, 100, "30M", dict(seq=genome_seq(100, "25M"))), (R2, 110, "30M")))
    return P


def error_pairs():
    """(label, opener, closer, expected error code name, mode bits) - every reachable error"""
    return [pair("err_unknown_char_n", (F1, 100, "10M5N15M"), (R2, 110, "30M")) + ("E_CIGAR_CHAR", 0),
            pair("err_unknown_char_eq_reverse", (F1, 100, "30M"), (R2, 110, "10=20M")) + ("E_CIGAR_CHAR", 0),
            pair("err_unknown_char_p", (F1, 100, "10M1P20M"), (R2, 110, "10X20M")) + ("E_CIGAR_CHAR", 0),
            pair("err_length_forward_short", (F1, 105, "2H3I"), (R2, 100, "30M")) + ("E_LENGTH", 0),
            pair("err_length_reverse_ends_first", (F1, 100, "30M"), (R2, 105, "2H2I")) + ("E_LENGTH", 0),
            pair("err_index_out_of_boundary", (F1, 105, "2H1I"), (R2, 105, "1I3H")) + ("E_SC_INDEX", 0),
            pair("err_unsupported_type_zero_n", (F1, 100, "15M0N15M"), (R2, 110, "30M")) + ("E_SC_OP", 0),
            pair("err_bad_base", (F1, 100, "30M"), (R2, 110, "30M", dict(seq=mutate(mutate(genome_seq(110, "30M"), 3), 25, "R")))) + ("E_BAD_BASE", 8),
            pair("err_cg_tag", (F1, 100, None, dict(cg="12M18M", seq=genome_seq(100, "30M"))), (R2, 110, "30M")) + ("E_UNSUPPORTED", 0)]


def random_cigar(rng):
    """M, I, D, S, H in a shape an aligner could give (clips outside, S inside H), 1 to 12 operations, 1 to 40 read bases"""
    while True:
        n_mid = rng.randint(1, 8)
        mid = []
        for _ in range(n_mid):
            o = rng.choice((0, 0, 0, 1, 2))
            mid.append((rng.randint(1, 3) if o else rng.randint(1, 12), o))
        if rng.random() < 0.8 and mid[0][1] != 0: mid.insert(0, (rng.randint(1, 8), 0))
        if rng.random() < 0.8 and mid[-1][1] != 0: mid.append((rng.randint(1, 8), 0))
        lead = ([(rng.randint(1, 3), 5)] if rng.random() < 0.15 else []) + ([(rng.randint(1, 4), 4)] if rng.random() < 0.25 else [])
        tail = ([(rng.randint(1, 4), 4)] if rng.random() < 0.25 else []) + ([(rng.randint(1, 3), 5)] if rng.random() < 0.15 else [])
        ops = lead + mid + tail
        if rng.random() < 0.02: ops.insert(rng.randrange(len(ops) + 1), (0, rng.choice((0, 1, 2, 4))))          # an operation of length 0
        if rng.random() < 0.015: ops.insert(rng.randrange(1, len(ops) + 1), (rng.randint(0, 2), rng.choice((3, 7, 8))))  # what the reference throws on
        if rng.random() < 0.02: ops = [(2, 5), (rng.randint(1, 3), 1)]                                           # hard clip and insertion alone
        q = sum(n for n, o in ops if o in (0, 1, 4, 7, 8))
        if 1 <= len(ops) <= 12 and 1 <= q <= 40:
            return ops


def random_pairs(n=2000, seed=20):
    rng = random.Random(seed)
    out = []
    for k in range(n):
        ca, cb = random_cigar(rng), random_cigar(rng)
        pa = rng.randint(100, 3000)
        pb = pa + rng.randint(-15, 15) if rng.random() < 0.9 else pa + rng.choice((-60, 60))
        strands = rng.choice(((0, 0x10), (0x10, 0), (0, 0), (0x10, 0x10), (0, 0x10), (0x10, 0)))
        first = rng.choice((0x40, 0x80))
        recs = []
        for pos, ops, st, rd in ((pa, ca, strands[0], first), (pb, cb, strands[1], first ^ 0xc0)):
            r = record(f"r{k:04d}", 1 | st | rd, 0, pos, ops, isize=rng.randint(-300, 300), mpos=rng.randint(0, 3000), aux=b"NMC\0" if k % 3 else b"XZZ" + b"q" * 70 + b"\0")
            if rng.random() < 0.5:   # mutations, one of them sometimes a base setBases cannot store
                seq = genome_seq(pos, ops)
                for _ in range(rng.randint(1, 3)):
                    seq = mutate(seq, rng.randrange(len(seq)), "R" if rng.random() < 0.03 else None)
                r = record(f"r{k:04d}", 1 | st | rd, 0, pos, ops, seq=seq, isize=rng.randint(-300, 300), mpos=rng.randint(0, 3000))
            recs.append(r)
        out.append((f"r{k:04d}", recs[0], recs[1]))
    return out


def good_random_pairs(n, seed=21):
    """random pairs that no mode fails on: known operations of at least one base, a reference base in both reads, storable bases"""
    out = []
    for label, a, b in random_pairs(4 * n, seed):
        ok = True
        for r in (a, b):
            n_cigar, l_name = struct.unpack_from("<H", r, 16)[0], r[12]
            ops = struct.unpack_from(f"<{n_cigar}I", r, 36 + l_name)
            ok = ok and all(c & 15 in (0, 1, 2, 4, 5) and c >> 4 for c in ops) and any(c & 15 in (0, 2) for c in ops) and "R" not in genome_seq_of(r)
        if ok:
            out.append(("g" + label, a, b))
        if len(out) == n:
            break
    return out


def genome_seq_of(r):
    l_seq = struct.unpack_from("<i", r, 20)[0]
    o = 36 + r[12] + 4 * struct.unpack_from("<H", r, 16)[0]
    return "".join(NT16[(r[o + (i >> 1)] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq))


def designed_file(good_pairs):
    """about 600 records from error-free pairs [(label, opener, closer)]: the first third of the pairs as neighbours, the openers of the rest in front of all
    their closers (open across tiles, and closed in another order than opened), between them records that pass through, a name with three records, names that
    stay open, and records whose CIGAR sits in a CG tag (written through, and as a pair that does not overlap)"""
    third = len(good_pairs) // 3
    recs = []
    g100 = genome_seq(100, "30M")
    extra = [record("x_unpaired", 0, 0, 100, "30M"), record("x_secondary", 0x141, 0, 100, "30M"), record("x_supplementary", 0x841, 0, 100, "30M"),
             record("x_unmapped", 0x45, 0, 100, [], seq=g100), record("x_mate_unmapped", 0x49, 0, 100, "30M"), record("x_other_chr", 0x41, 0, 100, "30M", mtid=1),
             record("x_only_ins", 0x41, 0, 100, "3S27I", seq=g100), record("x_cg_alone", 0, 0, 100, None, cg="10M2D20M", seq=g100),
             record("x_no_cigar", 0x41, 0, 100, [], seq=g100)]
    for k, (_, a, b) in enumerate(good_pairs[:third]):
        recs += [a, b]
        if k % 7 == 0: recs.append(extra[(k // 7) % len(extra)])
    late = good_pairs[third:]
    recs += [a for _, a, _ in late]
    recs += [record("x_three", 0x41, 0, 100, "30M"), record("x_left_open_1", 0x41, 0, 500, "30M"), record("x_cgpair", 0x41, 0, 100, None, cg="15M15M", seq=g100)]
    recs += extra
    order = list(range(len(late)))
    random.Random(3).shuffle(order)
    recs += [late[i][2] for i in order]
    recs += [record("x_three", 0x91, 0, 110, "30M"), record("x_three", 0x41, 0, 120, "30M"), record("x_cgpair", 0x91, 0, 900, None, cg="14M14M2S", seq=g100),
             record("x_left_open_2", 0x91, 0, 100, "30M")]
    return recs
