"""Designed inputs for BamRemoveVariants: a BAM of a few hundred records and a VCF whose lines sit on every boundary of the CIGAR walks, of the look-up of the
overlapping lines and of the pair rules (tests/test_gpu_bamremovevariants.py compares the device with tests/bamremovevariants_oracle.py on them;
tests/test_cpu_bamremovevariants_emul.py the device's per-record text compiled for the CPU). No reference genome is involved: a line's REF is whatever the case needs."""
import gzip
import random
import struct

import cram_twin

REFS = [("chr1", 2_000_000), ("chr2", 2_000_000), ("chr3", 2_000_000)]
OPS = "MIDNSHP=X"
NT16 = "=ACMGRSVTWYHKDBN"


def cigar_ops(text):
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append((int(n), OPS.index(ch))); n = ""
    return out


def record(name, flag, tid, pos, cigar, seq, aux=b"", cg=None, mapq=60):
    """cigar / cg: "20M2I18M" or a list of (length, operation number); cg: the real CIGAR goes into a CG:B,I tag behind the placeholder"""
    ops = cigar_ops(cigar) if isinstance(cigar, str) else list(cigar or [])
    if cg is not None:
        real = cigar_ops(cg) if isinstance(cg, str) else list(cg)
        aux = aux + b"CGBI" + struct.pack("<I", len(real)) + b"".join(struct.pack("<I", n << 4 | o) for n, o in real)
        ops = [(len(seq), 4), (sum(n for n, o in real if o in (0, 2, 3, 7, 8)) or 1, 3)]
    nm = name.encode() + b"\0"
    nib = [NT16.index(c) for c in seq] + [0]
    sq = bytes(nib[i] << 4 | nib[i + 1] for i in range(0, len(seq), 2))
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(nm), mapq, 4680, len(ops), flag, len(seq), tid, max(pos, 0), 0) + nm
    body += b"".join(struct.pack("<I", n << 4 | o) for n, o in ops) + sq + bytes(30 + i % 10 for i in range(len(seq))) + aux
    return struct.pack("<I", len(body)) + body


def seq_with(n, subs, fill="A"):
    s = [fill] * n
    for i, c in subs.items():
        s[i] = c
    return "".join(s)


def bam_bytes(recs, refs=REFS, member=4000):
    text = "@HD\tVN:1.6\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs)
    hdr = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(refs))
    for n, ln in refs:
        hdr += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", ln)
    raw = hdr + b"".join(recs)
    return b"".join(cram_twin._bgzf(raw[o:o + member]) for o in range(0, len(raw), member)) + cram_twin._bgzf(b"")


def vcf_text(lines):
    """lines: (chromosome, POS, REF, ALT[, INFO]) in any order; sorted by chromosome (first appearance) and POS, ties in the order given"""
    chroms = []
    for ln in lines:
        if ln[0] not in chroms:
            chroms.append(ln[0])
    rows = sorted(enumerate(lines), key=lambda t: (chroms.index(t[1][0]), t[1][1], t[0]))
    body = "".join(f"{ln[0]}\t{ln[1]}\t.\t{ln[2]}\t{ln[3]}\t.\tPASS\t{ln[4] if len(ln) > 4 else '.'}\n" for _, ln in rows)
    return "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n" + body


def write_vcf(path, text, index=True):
    with gzip.open(path, "wb") as f:
        f.write(text.encode())
    if index:   # (the tool asks for the index's existence alone)
        open(path + ".tbi", "wb").close()


def designed(seed=11):
    """(records, vcf lines): every case is a name of its own; `first` records come first in the file, their mates (clean reads on chr2 unless the case says
    otherwise) behind all of them, so that openers wait across tiles"""
    rng = random.Random(seed)
    first, second, lines = [], [], []
    slot = [0]

    def place():
        slot[0] += 1
        return 10_000 + 3_000 * slot[0]   # 0-based start of the case's read on chr1; cases lie 3 kb apart

    def case(label, rec_args, mate_args=None):
        name = f"c{len(first):03d}_{label}"
        first.append(record(name, 0x41, *rec_args))
        second.append(record(name, 0x81, *(mate_args or (1, 500 + 10 * len(first), "40M", "A" * 40))))

    # SNVs on the first and on the last aligned base; even and odd read index; the last base of an odd-length read
    P = place(); case("first_base", (0, P, "40M", seq_with(40, {0: "C"}))); lines.append(("chr1", P + 1, "A", "C"))
    P = place(); case("last_base_odd_index", (0, P, "40M", seq_with(40, {39: "C"}))); lines.append(("chr1", P + 40, "A", "C"))
    P = place(); case("last_base_odd_length", (0, P, "41M", seq_with(41, {40: "G"}))); lines.append(("chr1", P + 41, "T", "G"))
    P = place(); case("not_carried", (0, P, "40M", seq_with(40, {7: "G"}))); lines.append(("chr1", P + 8, "A", "C"))
    # inside a deletion, inside a skip, next to soft clips, H = X operations
    P = place(); case("in_deletion", (0, P, "20M5D20M", "C" * 40)); lines.append(("chr1", P + 22, "A", "C"))
    P = place(); case("in_skip", (0, P, "20M100N20M", "C" * 40)); lines.append(("chr1", P + 50, "A", "C"))
    P = place(); case("behind_leading_clip", (0, P, "5S35M", seq_with(40, {5: "T"}))); lines.append(("chr1", P + 1, "A", "T"))
    P = place(); case("before_trailing_clip", (0, P, "35M5S", seq_with(40, {34: "T", 35: "T"}))); lines += [("chr1", P + 35, "A", "T"), ("chr1", P + 36, "A", "T")]
    P = place(); case("hard_eq_diff", (0, P, "3H10=1X29M2H", seq_with(40, {10: "G"}))); lines.append(("chr1", P + 11, "A", "G"))
    P = place(); case("insertion_only", (0, P, "40I", "C" * 40)); lines.append(("chr1", P + 1, "A", "C"))
    P = place(); case("all_clipped", (0, P, "40S", "C" * 40)); lines.append(("chr1", P + 1, "A", "C"))
    P = place(); case("clip_reaches_length", (0, P, "10M30S", "C" * 40)); lines.append(("chr1", P + 10, "AT", "AG"))   # (the SNV's start lies behind the 10 aligned bases: the clip ends the walk)
    # an unmapped record placed at its mate, an SNV on its position
    P = place(); case("mate_of_unmapped", (0, P, "40M", seq_with(40, {3: "G"})), (0, P, [], "C" * 40)); lines.append(("chr1", P + 1, "A", "C"))
    second[-1] = record(f"c{len(first) - 1:03d}_mate_of_unmapped", 0x85, 0, P, [], "C" * 40)
    # two and three carried SNVs; a carried indel line between two carried SNVs
    P = place(); case("two_snvs", (0, P, "40M", seq_with(40, {4: "C", 5: "G"}))); lines += [("chr1", P + 5, "A", "C"), ("chr1", P + 6, "A", "G")]
    P = place(); case("three_snvs", (0, P, "41M", seq_with(41, {0: "T", 20: "C", 40: "G"}))); lines += [("chr1", P + 1, "A", "T"), ("chr1", P + 21, "G", "C"), ("chr1", P + 41, "C", "G")]
    P = place(); case("indel_between_snvs", (0, P, "20M2I18M", seq_with(40, {2: "C", 30: "C"})))
    lines += [("chr1", P + 3, "A", "C"), ("chr1", P + 10, "A", "ATT"), ("chr1", P + 29, "A", "C")]
    # two lines on one base: the second sees what the first wrote; a base set and set back; REF equal to ALT
    P = place(); case("second_sees_first", (0, P, "40M", seq_with(40, {9: "C"}))); lines += [("chr1", P + 10, "A", "C"), ("chr1", P + 10, "G", "A")]
    P = place(); case("set_and_set_back", (0, P, "40M", seq_with(40, {9: "C", 12: "T"}))); lines += [("chr1", P + 10, "A", "C"), ("chr1", P + 10, "C", "A"), ("chr1", P + 13, "T", "T")]
    P = place(); case("ref_equals_alt", (0, P, "40M", "A" * 40)); lines.append(("chr1", P + 2, "A", "A"))
    # I and D exactly 50 and 51 bases from the normalised start, on both sides; POS is one in front of the start
    for op in "ID":
        for d in (-51, -50, 50, 51):
            P = place(); case(f"{op}_{d}", (0, P, f"100M{'1I' if op == 'I' else '3D'}100M", "A" * (201 if op == "I" else 200)))
            lines.append(("chr1", P + 101 + d - 1, "AC", "A"))   # the operation's genome position is P + 101; the line's start POS + 1
    # a line that reaches the read only with the tail of its REF: an indel line with and without an indel in the read, an SNV whose start is in front of the read
    P = place(); case("tail_no_indel", (0, P, "40M", "A" * 40)); lines.append(("chr1", P - 5, "A" * 10, "A"))
    P = place(); case("tail_indel", (0, P, "5M1D35M", "A" * 40)); lines.append(("chr1", P - 5, "A" * 10, "A"))
    P = place(); case("snv_in_front_of_read", (0, P, "40M", "T" * 40)); lines.append(("chr1", P - 2, "ACAA", "TCAA"))
    P = place(); case("snv_in_front_lands_in_clip", (0, P, "5S35M", seq_with(40, {2: "T"}))); lines.append(("chr1", P - 2, "ACAA", "TCAA"))
    P = place(); case("snv_start_behind_pos", (0, P, "40M", seq_with(40, {0: "T"}))); lines.append(("chr1", P - 1, "AAC", "AAT"))
    P = place(); case("end_from_info", (0, P + 10, "40M", "C" * 40)); lines.append(("chr1", P + 1, "A", "C", "DP=9;END=" + str(P + 30)))
    # <NON_REF> is no SNV: an indel line
    P = place(); case("non_ref_plain", (0, P, "40M", "C" * 40)); lines.append(("chr1", P + 5, "A", "<NON_REF>"))
    P = place(); case("non_ref_deletion", (0, P, "20M2D20M", "C" * 40)); lines.append(("chr1", P + 21, "A", "<NON_REF>"))
    # a line no record visits may be invalid; chromosomes the BAM does not have
    lines += [("chr1", 1_900_000, "A", "C,G"), ("chr9", 100, "A", "C"), ("chr9", 200, "ACGT", "A")]
    # the reads-modified rule: an opener that fails, a closer that would be modified; a closer that fails behind a modified opener; both modified
    P = place(); case("opener_fails", (0, P, "20M1I19M", "A" * 40), (0, P + 500, "40M", seq_with(40, {1: "C"})))
    lines += [("chr1", P + 21, "A", "ATT"), ("chr1", P + 502, "A", "C")]
    P = place(); case("closer_fails", (0, P, "40M", seq_with(40, {1: "C"})), (0, P + 500, "20M1D20M", seq_with(40, {0: "G"})))
    lines += [("chr1", P + 2, "A", "C"), ("chr1", P + 501, "A", "G"), ("chr1", P + 521, "AC", "A")]
    P = place(); case("both_modified", (0, P, "40M", seq_with(40, {1: "C"})), (0, P + 500, "40M", seq_with(40, {38: "G", 39: "G"})))
    lines += [("chr1", P + 2, "A", "C"), ("chr1", P + 539, "A", "G"), ("chr1", P + 540, "T", "G")]
    # a name seen three times: the third record opens again and never closes
    P = place(); case("three_times", (0, P, "40M", "A" * 40)); first.append(record(f"c{len(first) - 1:03d}_three_times", 0x41, 0, P, "40M", seq_with(40, {6: "C"})))
    second.append(record("lonely", 0x41, 1, 900, "40M", "A" * 40)); lines.append(("chr1", P + 7, "A", "C"))
    # secondary and supplementary copies of a carried read
    P = place(); case("with_copies", (0, P, "40M", seq_with(40, {0: "C"}))); lines.append(("chr1", P + 1, "A", "C"))
    first.append(record(f"c{len(first) - 1:03d}_with_copies", 0x141, 0, P, "40M", seq_with(40, {0: "C"}))); second.append(record(f"c{len(first) - 2:03d}_with_copies", 0x881, 0, P, "40M", seq_with(40, {0: "C"})))
    # no chromosome
    first.append(record("nowhere", 0x4d, -1, -1, [], "C" * 40)); second.append(record("nowhere", 0x8d, -1, -1, [], "C" * 40))
    # more than LONG_CIGAR operations: carried SNVs around a carried indel line; the same read with the real CIGAR in a CG tag
    long_ops = [(3, 0), (1, 1)] * 34 + [(3, 0)]   # 69 operations, 139 bases, 105 reference bases
    long_seq = seq_with(139, {0: "C", 1: "G", 8: "T", 138: "C"})   # read index 8 is the M base at reference offset 6; 138 the last base (offset 104)
    for label, kw in (("long_cigar", dict(cigar=long_ops)), ("long_cigar_cg", dict(cigar=None, cg=long_ops))):
        P = place(); case(label, (0, P, kw["cigar"], long_seq, b"", kw.get("cg")))
        lines += [("chr1", P + 1, "A", "C"), ("chr1", P + 2, "A", "G"), ("chr1", P + 7, "A", "T"), ("chr1", P + 105, "A", "C")]
        P = place(); case(label + "_indel", (0, P, kw["cigar"], long_seq, b"", kw.get("cg")))
        lines += [("chr1", P + 1, "A", "C"), ("chr1", P + 60, "AG", "A"), ("chr1", P + 105, "A", "C")]
    P = place(); case("short_cg", (0, P, None, seq_with(41, {2: "C", 40: "C"}), b"XAZx\0", "20M2I19M")); lines += [("chr1", P + 3, "A", "C"), ("chr1", P + 39, "A", "C")]
    # a 10 kb REF in front of 200 SNV lines: the first candidate comes from the running maximum of end, not from end
    lines.append(("chr3", 1_000, "A" * 10_000, "A"))
    lines += [("chr3", 5_000 + i, "A", "CGT"[i % 3]) for i in range(200)]
    for label, pos, seq in (("dense_all_c", 5_049, "C" * 40), ("dense_mixed", 5_120, "".join("CGTA"[(i * 7) % 4] for i in range(41))), ("dense_edge", 5_190, "C" * 40),
                            ("long_ref_only", 7_000, "C" * 40), ("long_ref_tail", 10_990, "C" * 40), ("behind_long_ref", 11_000, "C" * 40), ("in_front_of_all", 900, "C" * 40)):
        case(label, (2, pos, f"{len(seq)}M", seq))
    case("dense_deletion", (2, 5_010, "20M2D20M", "C" * 40))
    # filler pairs over a handful of random lines
    for k in range(90):
        P = 1_000_000 + 37 * k
        sq = "".join(rng.choice("ACGT") for _ in range(50))
        case(f"fill{k}", (0, P, "25M1I24M" if k % 9 == 0 else "50M", sq), (0, P + 200, "50M", "".join(rng.choice("ACGT") for _ in range(50))))
    lines += [("chr1", 1_000_000 + rng.randrange(0, 3600), "A", rng.choice("CGT")) for _ in range(60)]
    lines += [("chr1", 1_000_000 + 400 * k, "AT", "A") for k in range(1, 8)]
    return first + second, lines


def picked_lines(records, ref_names, seed=5, n_snv=34, n_indel=6):
    """VCF lines read off the records of a BAM by a seeded picker: SNVs at positions inside reads with the read's own base as ALT (so that they ARE carried), and
    indel lines where reads have an I or a D operation"""
    from bamfilter_oracle import Rec
    rng = random.Random(seed)
    lines, tries = [], 0
    cand = [i for i in range(len(records))]
    rng.shuffle(cand)
    with_indel = []
    for i in cand:
        r = Rec(records[i])
        if r.flag & 4 or r.tid < 0 or not r.cigar:
            continue
        ops = [(c >> 4, c & 15) for c in r.effective_cigar()]
        gp, rp, spots, indels = r.pos + 1, 0, [], []
        for n, op in ops:
            if op in (0, 7, 8):
                k = rng.randrange(n); spots.append((gp + k, rp + k)); gp += n; rp += n
            elif op in (1, 4):
                if op == 1:
                    indels.append(gp)
                rp += n
            elif op in (2, 3):
                if op == 2:
                    indels.append(gp)
                gp += n
        if indels and len(with_indel) < n_indel:
            g = rng.choice(indels) + rng.randrange(-20, 21)
            with_indel.append((ref_names[r.tid], max(1, g - 1), "AC", "A") if len(with_indel) % 2 else (ref_names[r.tid], max(1, g), "A", "ATT"))
        if spots and sum(1 for ln in lines if len(ln[2]) == 1) < n_snv:
            g, p = rng.choice(spots)
            b = NT16[(records[i][r.seq_off + (p >> 1)] >> (4 if p % 2 == 0 else 0)) & 15]
            if b in "ACGT":
                lines.append((ref_names[r.tid], g, rng.choice([c for c in "ACGT" if c != b]), b))
        tries += 1
        if len(with_indel) >= n_indel and len(lines) >= n_snv:
            break
    lines += with_indel
    order = {n: t for t, n in enumerate(ref_names)}
    return sorted(lines, key=lambda ln: (order[ln[0]], ln[1]))


def device_layout(rows):
    """the table as the library lays it out: the rows (bamremovevariants_oracle.table) with a tid, grouped by tid in file order; the running maximum of end;
    the first row of every tid. Returns (rows, maxend, tid_first builder taking n_ref, index of every row in the input)"""
    keep = sorted((i for i, r in enumerate(rows) if r[0] >= 0), key=lambda i: (rows[i][0], i))
    out, maxend = [rows[i] for i in keep], []
    for k, r in enumerate(out):
        maxend.append(r[2] if k == 0 or out[k - 1][0] != r[0] else max(maxend[-1], r[2]))
    return out, maxend, keep
