"""BamClipOverlap restated in Python (src/BamClipOverlap/main.cpp:43-554, NGSHelper::softClipAlignment NGSHelper.cpp:670-810, the BamAlignment setters of
BamReader.cpp), literally: the overlap lists, the '+' placeholders and the per-base matrix are built as the reference builds them. BAMs are read with Python's
gzip (bamfilter_oracle).

run(header, records, mode, ignore_indels) -> Result: the written record bytes in the reference's order, the six counters, the three summary lines, the whole
-v log and the plan (one row of six integers per input record, what ngsqc_clip_overlap_plan gives). Raises ClipError where the reference throws.

Where the reference leaves something open, this file says what the project does:
  - the entries still in the name map at the end are written in QHash order there; here in file order;
  - the insertion correction reads reverse_overlap.cigar[i] behind the end of a shorter list (undefined there): reported as the length mismatch, with the two
    lengths at that moment;
  - a CIGAR that walks past the end of the sequence reads behind the arrays there: here such an index gives the base and quality NUL and is never patched;
  - a pair that is clipped and whose CIGAR lives in a CG tag (or would need more than 65535 operations) is refused (E_UNSUPPORTED).
Errors that cannot be reached, by the code's own arithmetic: "Read orientation ... was not identified" (with end >= start on both reads the four comparisons
of s1/s2 and e1/e2 always land in one of the six branches), and softClipAlignment's "End position is smaller than start position", "Start position ... not within
alignment", "End position ... not within alignment" (a clip is at least 1 and at most the read's reference length in every branch). They are restated all the
same. "Unsupported CIGAR type" is reached by an operation of length 0 alone: any base of N, =, X, P already throws "Unknown CIGAR character" in the walk."""
import gzip
import os
import struct

from bamfilter_oracle import Rec, read_bam, written  # noqa: F401

MAPQ, REMOVE, BASEQ, BASEN = 1, 2, 4, 8                     # mode bits
PASS, FORWARD, REVERSE, LEFTOVER = 0, 1, 2, 3               # plan column 0
V_CLIP_PAIR, V_MISMATCH, V_REMOVED, V_MAPQ0, V_QUAL, V_BASES, V_REWRITTEN = 1, 2, 4, 8, 16, 32, 64   # plan column 5
(E_ORIENT, E_CIGAR_CHAR, E_LENGTH, E_SC_ORDER, E_SC_START, E_SC_END, E_SC_INDEX, E_SC_OP, E_BAD_BASE, E_UNSUPPORTED) = range(1, 11)
NT16 = "=ACMGRSVTWYHKDBN"
CIGAR_CHR = "MIDNSHP=XB??????"
M, I, D, N_, S, H = 0, 1, 2, 3, 4, 5


def golden_log(k):
    """the reference's expected log data_out/BamClipOverlap_out<k>.log, byte for byte (kept gzip-compressed under tests/golden/ref_out)"""
    here = os.path.dirname(os.path.abspath(__file__))
    return gzip.open(os.path.join(here, "golden", "ref_out", f"BamClipOverlap_out{k}.log.gz"), "rb").read()


class ClipError(Exception):
    def __init__(self, code, message, a=0, b=0):
        super().__init__(message)
        self.code, self.message, self.a, self.b, self.record = code, message, a, b, -1


def ref_names_of(header):
    o = 8 + struct.unpack_from("<I", header, 4)[0]
    n = struct.unpack_from("<I", header, o)[0]; o += 4
    out = []
    for _ in range(n):
        ln = struct.unpack_from("<I", header, o)[0]
        out.append(header[o + 4:o + 4 + ln - 1].decode("latin-1")); o += 8 + ln
    return out


class Aln:
    """a BamAlignment as bam_read1 leaves it: the CIGAR of a CG tag is in place, and the copy can be changed"""

    def __init__(self, b):
        r = Rec(b)
        self.raw, self.rec, self.cg = b, r, r.cg() is not None
        self.tid, self.pos, self.mapq, self.bin, self.flag, self.l_seq, self.mtid, self.mpos, self.isize = r.tid, r.pos, r.mapq, r.bin, r.flag, r.l_seq, r.mtid, r.mpos, r.isize
        self.name = r.name
        self.cigar = list(r.effective_cigar())
        sq = b[r.seq_off:r.seq_off + (r.l_seq + 1) // 2]
        self.seq = [(sq[i >> 1] >> (0 if i & 1 else 4)) & 15 for i in range(r.l_seq)]
        self.qual = list(b[r.seq_off + (r.l_seq + 1) // 2:r.aux_off])
        self.aux = b[r.aux_off:]
        self.changed = False

    # --- BamReader.h ---
    def start(self):
        return self.pos + 1

    def end(self):   # bam_endpos
        rlen = 0 if self.flag & 4 else sum(c >> 4 for c in self.cigar if (0x3C1A7 >> ((c & 15) << 1)) & 2)
        return self.pos + (rlen or 1)

    def bases(self):
        return "".join(NT16[x] for x in self.seq)

    def qualities(self):
        return "".join(chr((q + 33) & 255) for q in self.qual)

    def cigar_string(self, expand=False):
        if expand:
            return "".join(CIGAR_CHR[c & 15] * (c >> 4) for c in self.cigar)
        return "".join(f"{c >> 4}{CIGAR_CHR[c & 15]}" for c in self.cigar)

    def cigar_is_only_insertion(self):
        return all(c & 15 in (I, S) for c in self.cigar)

    def set_bases(self, text):   # BamReader.cpp:133-181
        for i, ch in enumerate(text):
            k = {"A": 1, "C": 2, "G": 4, "T": 8, "N": 15}.get(ch.upper())
            if k is None:
                raise ClipError(E_BAD_BASE, f"Cannot store character '{ch}' in BAM/CRAM file. Only A,C,G,T,N are allowed!", ord(ch))
            self.seq[i] = k
        self.changed = True

    def set_qualities(self, text):
        self.qual = [(ord(c) - 33) & 255 for c in text]
        self.changed = True

    def add_tag(self, tag, type_, value):
        self.aux += tag + type_ + value + b"\0"
        self.changed = True

    def bytes(self):
        if not self.changed:
            return written(self.rec)
        sq = self.seq + [0]
        body = struct.pack("<iiBBHHHiiii", self.tid, self.pos, len(self.name) + 1, self.mapq, self.bin, len(self.cigar), self.flag, self.l_seq, self.mtid, self.mpos, self.isize)
        body += self.name + b"\0" + struct.pack(f"<{len(self.cigar)}I", *self.cigar)
        body += bytes(sq[i] << 4 | sq[i + 1] for i in range(0, self.l_seq, 2)) + bytes(self.qual) + self.aux
        return struct.pack("<I", len(body)) + body


def soft_clip_alignment(al, start_ref_pos, end_ref_pos):
    """NGSHelper::softClipAlignment (NGSHelper.cpp:670-810)"""
    al.add_tag(b"BS", b"Z", al.cigar_string().encode())
    if start_ref_pos > end_ref_pos:
        raise ClipError(E_SC_ORDER, "End position is smaller than start position.")
    if start_ref_pos < al.start() or start_ref_pos > al.end():
        raise ClipError(E_SC_START, f"Start position {start_ref_pos} not within alignment ({al.start()}:{al.end()}).", start_ref_pos)
    if end_ref_pos < al.start() or end_ref_pos > al.end():
        raise ClipError(E_SC_END, f"End position {end_ref_pos} not within alignment ({al.start()}:{al.end()}).", end_ref_pos)
    matrix = []
    for c in al.cigar:
        op = c & 15
        if op not in (D, S, M, I, H):
            raise ClipError(E_SC_OP, f"Unsupported CIGAR type '{CIGAR_CHR[op]}'", ord(CIGAR_CHR[op]))
        for _ in range(c >> 4):
            matrix.append([op, op])
    j, cur = 0, al.start()
    while cur <= al.end():
        if j >= len(matrix):
            raise ClipError(E_SC_INDEX, "Index out of boundary!")
        if matrix[j][0] != H:
            if start_ref_pos <= cur <= end_ref_pos:
                matrix[j][1] = S
            if matrix[j][0] in (D, M):
                cur += 1
        j += 1
    new, tmp_char, tmp_count = [], -1, 0
    for first, second in matrix:
        if first == D and second == S:
            continue
        if second != tmp_char:
            if tmp_char != -1:
                new.append([tmp_char, tmp_count])
            tmp_char, tmp_count = second, 0
        tmp_count += 1
    new.append([tmp_char, tmp_count])
    i = 1
    while i < len(new):
        redo = False
        if new[i - 1][0] == S and new[i][0] == D:
            del new[i]; redo = True
        elif new[i - 1][0] == D and new[i][0] == S:
            del new[i - 1]; redo = True
        elif new[i - 1][0] == S and new[i][0] == I:
            new[i - 1][1] += new[i][1]; del new[i]; redo = True
        elif new[i - 1][0] == I and new[i][0] == S:
            new[i][1] += new[i - 1][1]; del new[i - 1]; redo = True
        if redo:
            i -= 1
        i += 1
    k = 0
    while k < len(matrix) and matrix[k][1] == H:
        k += 1
    if matrix[k][1] == S:
        offset = 0
        while k < len(matrix) and matrix[k][1] == S:
            if matrix[k][0] in (M, D):
                offset += 1
            k += 1
        al.pos = al.start() + offset - 1
    al.cigar = [((n << 4) | (t & 0xffffffff)) & 0xffffffff for t, n in new]   # bam_cigar_gen
    if len(al.cigar) > 65535:
        raise ClipError(E_UNSUPPORTED, "BamClipOverlap: a clipped CIGAR of more than 65535 operations is not supported")


class Overlap:
    def __init__(self):
        self.genome_pos, self.read_pos, self.base, self.quality, self.cigar = [], [], [], [], []

    def append(self, base, cigar, quality, genome_pos, read_pos):
        self.base.append(base); self.cigar.append(cigar); self.quality.append(quality); self.genome_pos.append(genome_pos); self.read_pos.append(read_pos)

    def insert(self, at, base, cigar, quality, genome_pos, read_pos):
        self.base.insert(at, base); self.cigar.insert(at, cigar); self.quality.insert(at, quality); self.genome_pos.insert(at, genome_pos); self.read_pos.insert(at, read_pos)

    def length(self):
        return len(self.read_pos)


class Result:
    pass


def _i32(x):
    return (x + 2 ** 31) % 2 ** 32 - 2 ** 31


def fmt_pct(a, b):
    """QString::number((double)a / (double)b * 100, 'f', 2)"""
    if b == 0:
        return "nan" if a == 0 else "inf"
    return "%.2f" % (a / b * 100)


def run(header, records, mode=0, ignore_indels=False, verbose=True):
    refs = ref_names_of(header)
    log, out, plan = [], [], [None] * len(records)
    reads_count = reads_saved = reads_clipped = reads_mismatch = 0
    bases_count = bases_clipped = 0
    al_map = {}   # name -> (Aln, ordinal); insertion-ordered: the leftovers leave in file order
    removed = []

    def chrom(tid):
        return refs[tid]

    def say(s):
        if verbose:
            log.append(s)

    def own_row(a, role):
        return [role, 0, a.pos, len(a.cigar), a.isize, 0]

    for ordinal, b in enumerate(records):
        al = Aln(b)
        reads_count += 1
        bases_count += al.l_seq
        skip_al = False
        if (not al.flag & 1 or al.flag & 0x900 or al.flag & 4 or al.flag & 8 or al.tid != al.mtid or al.cigar_is_only_insertion()):
            out.append(al.bytes()); plan[ordinal] = own_row(al, PASS); reads_saved += 1
            continue
        if al.name not in al_map:
            al_map[al.name] = (al, ordinal); plan[ordinal] = own_row(al, LEFTOVER)
            continue
        mate, mate_ord = al_map.pop(al.name)
        try:
            forward_read, reverse_read, f_ord, r_ord = mate, al, mate_ord, ordinal
            both_strands = False
            if bool(forward_read.flag & 16) != bool(reverse_read.flag & 16):
                both_strands = True
                if not reverse_read.flag & 16:
                    forward_read, reverse_read, f_ord, r_ord = reverse_read, forward_read, r_ord, f_ord
            s1, e1, s2, e2 = forward_read.start(), forward_read.end(), reverse_read.start(), reverse_read.end()
            soft_clip = False
            if forward_read.tid == reverse_read.tid:
                if s2 <= s1 <= e2: soft_clip = True
                elif s2 <= e1 <= e2: soft_clip = True
                elif s1 <= s2 and e1 >= e2: soft_clip = True
            bits = 0
            clip_forward_read = clip_reverse_read = 0
            if soft_clip:
                bits |= V_CLIP_PAIR
                if forward_read.cg or reverse_read.cg:
                    raise ClipError(E_UNSUPPORTED, "BamClipOverlap: clipping a read whose CIGAR is stored in a CG tag is not supported (read '" + al.name.decode("latin-1") + "')")
                if s1 <= s2 and e1 <= e2:
                    overlap = e1 - s2 + 1; overlap_start = s2 - 1; overlap_end = e1
                    clip_forward_read = clip_reverse_read = overlap // 2
                    if forward_read.flag & 64: clip_forward_read += overlap % 2
                    else: clip_reverse_read += overlap % 2
                elif s1 > s2 and e1 > e2:
                    overlap = e2 - s1 + 1; overlap_start = s1 - 1; overlap_end = e2
                    clip_forward_read = overlap // 2 + (e1 - e2); clip_reverse_read = overlap // 2 + (s1 - s2)
                    if forward_read.flag & 64: clip_forward_read += overlap % 2
                    else: clip_reverse_read += overlap % 2
                elif both_strands and s1 >= s2 and e1 <= e2:
                    overlap = e1 - s1 + 1; overlap_start = s1 - 1; overlap_end = e1
                    clip_forward_read = overlap // 2; clip_reverse_read = overlap // 2 + (s1 - s2)
                    if forward_read.flag & 64: clip_forward_read += overlap % 2
                    else: clip_reverse_read += overlap % 2
                elif both_strands and s1 <= s2 and e1 >= e2:
                    overlap = e2 - s2 + 1; overlap_start = s2 - 1; overlap_end = e2
                    clip_forward_read = overlap // 2 + (e1 - e2); clip_reverse_read = overlap // 2
                    if forward_read.flag & 64: clip_forward_read += overlap % 2
                    else: clip_reverse_read += overlap % 2
                elif not both_strands and s1 >= s2 and e1 <= e2:
                    overlap = e1 - s1 + 1; overlap_start = s1 - 1; overlap_end = e1
                    clip_forward_read, clip_reverse_read = overlap, 0
                elif not both_strands and s1 <= s2 and e1 >= e2:
                    overlap = e2 - s2 + 1; overlap_start = s2 - 1; overlap_end = e2
                    clip_forward_read, clip_reverse_read = 0, overlap
                else:
                    fn, rn = forward_read.name.decode("latin-1"), reverse_read.name.decode("latin-1")
                    a, c = ("forward read ", "reverse read ") if both_strands else ("read1 ", "read2 ")
                    raise ClipError(E_ORIENT, f"Read orientation of {a}{fn} ({chrom(forward_read.tid)}:{s1}-{e1}) and {c}{rn} ({chrom(reverse_read.tid)}:{s2}-{e2}) was not identified.")
                for tag, r in (("forward", forward_read), ("reverse", reverse_read)):
                    say(f"{tag} read: name - {r.name.decode('latin-1')}, region - {chrom(r.tid)}:{r.start() - 1}-{r.end()}, insert size: {r.isize} bp; mate: {r.mpos + 1}, CIGAR {r.cigar_string()}, overlap: {overlap} bp")
                for tag, r in (("forward", forward_read), ("reverse", reverse_read)):
                    say(f"{tag} read bases {r.bases()}"); say(f"{tag} read qualities {r.qualities()}"); say(f"{tag} CIGAR {r.cigar_string(True)}")
                say(f"  clip forward read from position {e1 - clip_forward_read + 1} to {e1}")
                say(f"  clip reverse read from position {s2} to {s2 - 1 + clip_reverse_read}")
                say(f"  overlap found from {overlap_start} to {overlap_end}")
                has_indel = False
                surrounding_nuc = 5
                lists = []
                for tag, r, clip_position in (("forward", forward_read, e1 - clip_forward_read), ("reverse", reverse_read, s2 - 1 + clip_reverse_read)):
                    genome_pos, read_pos = r.start() - 1, 0
                    ov = Overlap()
                    rb, rq = r.bases(), r.qualities()
                    for ch in r.cigar_string(True):
                        if overlap_start <= genome_pos < overlap_end and ch != "H" and ch != "S":
                            cb = rb[read_pos] if read_pos < len(rb) else "\0"
                            cq = rq[read_pos] if read_pos < len(rq) else "\0"
                            if ch == "D": cb = "-"
                            ov.append(cb, ch, cq, genome_pos, read_pos)
                        if not ignore_indels and clip_position - surrounding_nuc < genome_pos < clip_position + surrounding_nuc:
                            if ch in "ID":
                                has_indel = True
                        if ch == "H": continue
                        elif ch == "S": read_pos += 1
                        elif ch == "M": genome_pos += 1; read_pos += 1
                        elif ch == "D": genome_pos += 1
                        elif ch == "I": read_pos += 1
                        else:
                            raise ClipError(E_CIGAR_CHAR, f"Unknown CIGAR character '{ch}'", ord(ch))
                    say(f"  finished reading overlap {tag} bases {''.join(ov.base)}")
                    say(f"  finished reading overlap {tag} cigar {''.join(ov.cigar)}")
                    lists.append(ov)
                fo, ro = lists

                def length_error():
                    return ClipError(E_LENGTH, f"Length mismatch between forward/reverse overlap - forward:{fo.length()} reverse:{ro.length()} in read with name '{al.name.decode('latin-1')}'", fo.length(), ro.length())
                i = 0
                while i < fo.length():
                    if i >= ro.length():
                        raise length_error()   # (the reference reads behind the reverse list here)
                    if fo.cigar[i] != ro.cigar[i] and fo.cigar[i] == "I" and fo.base[i] != "+":
                        ro.insert(i, "+", "I", "0", ro.genome_pos[i], ro.read_pos[i])
                    if fo.cigar[i] != ro.cigar[i] and ro.cigar[i] == "I" and ro.base[i] != "+":
                        fo.insert(i, "+", "I", "0", fo.genome_pos[i], fo.read_pos[i])
                    i += 1
                for tag, ov in (("forward", fo), ("reverse", ro)):
                    say(f"  finished indel correction {tag} bases {''.join(ov.base)}")
                    say(f"  finished indel correction {tag} cigar {''.join(ov.cigar)}")
                if fo.length() != ro.length():
                    raise length_error()
                mm_pos = []
                for i in range(fo.length()):
                    if fo.base[i] != ro.base[i]:
                        first, second = fo.read_pos[i], ro.read_pos[i]
                        if fo.base[i] in "-+": first = -1
                        if ro.base[i] in "-+": second = -1
                        mm_pos.append((first, second))
                if verbose and mm_pos:
                    say(f"  overlap mismatch for read pair {forward_read.name.decode('latin-1')} - {''.join(fo.base)} != {''.join(ro.base)}!")
                map_, rem, base, basen = mode & MAPQ, mode & REMOVE, mode & BASEQ, mode & BASEN
                if base or rem or map_ or basen:
                    if mm_pos and map_:
                        forward_read.mapq = reverse_read.mapq = 0; forward_read.changed = reverse_read.changed = True
                        reads_mismatch += 2; bits |= V_MISMATCH | V_MAPQ0
                        say("  Set mapping quality to 0.")
                    elif mm_pos and rem:
                        reads_mismatch += 2; skip_al = True; bits |= V_MISMATCH | V_REMOVED
                        say("   Removed pair.")
                    elif mm_pos and base:
                        reads_mismatch += 2; bits |= V_MISMATCH | V_QUAL
                        orig_for, orig_rev = forward_read.qualities(), reverse_read.qualities()
                        new_for, new_rev = list(orig_for), list(orig_rev)
                        for first, second in mm_pos:
                            if 0 <= first < len(new_for): new_for[first] = "!"
                            if 0 <= second < len(new_rev): new_rev[second] = "!"
                        forward_read.set_qualities("".join(new_for)); reverse_read.set_qualities("".join(new_rev))
                        say(f"   changed forward base qualities from {orig_for} to {forward_read.qualities()}")
                        say(f"   changed reverse base qualities from {orig_rev} to {reverse_read.qualities()}")
                    elif mm_pos and basen:
                        reads_mismatch += 2; bits |= V_MISMATCH | V_BASES
                        orig_for, orig_rev = forward_read.bases(), reverse_read.bases()
                        new_for, new_rev = list(orig_for), list(orig_rev)
                        for first, second in mm_pos:
                            if 0 <= first < len(new_for): new_for[first] = "N"
                            if 0 <= second < len(new_rev): new_rev[second] = "N"
                        forward_read.set_bases("".join(new_for)); reverse_read.set_bases("".join(new_rev))
                        say(f"   changed forward sequences from {orig_for} to {forward_read.bases()}")
                        say(f"   changed reverse sequences from {orig_rev} to {reverse_read.bases()}")
                    else:
                        say(f"  no overlap mismatch for read pair {forward_read.name.decode('latin-1')}")
                if has_indel:
                    if reads_clipped % 4 == 0:
                        clip_forward_read, clip_reverse_read = 0, overlap
                    else:
                        clip_forward_read, clip_reverse_read = overlap, 0
                if clip_forward_read > 0:
                    soft_clip_alignment(forward_read, forward_read.end() - clip_forward_read + 1, forward_read.end())
                if clip_reverse_read > 0:
                    soft_clip_alignment(reverse_read, reverse_read.start(), reverse_read.start() - 1 + clip_reverse_read)
                forward_end, reverse_end = forward_read.end(), reverse_read.end()
                if reverse_read.start() == reverse_read.end(): reverse_end -= 1
                if forward_read.start() == forward_read.end(): forward_end -= 1
                forward_read.isize = _i32(reverse_end - forward_read.start() + 1)
                forward_read.mpos = reverse_read.start() - 1
                reverse_read.isize = _i32(forward_read.start() - reverse_end - 1)
                reverse_read.mpos = forward_read.start() - 1
                forward_read.changed = reverse_read.changed = True
                for tag, r, e in (("forward", forward_read, forward_end), ("reverse", reverse_read, reverse_end)):
                    say(f"  clipped {tag} read: name - {r.name.decode('latin-1')}, region - {chrom(r.tid)}:{r.start() - 1}-{e}, insert size: {r.isize} bp; mate: {r.mpos + 1}, CIGAR {r.cigar_string()}, overlap: {overlap} bp")
                say("")
                bases_clipped += overlap
                reads_clipped += 2
        except ClipError as e:
            e.record = ordinal
            raise
        plan[f_ord] = [FORWARD, clip_forward_read, forward_read.pos, len(forward_read.cigar), forward_read.isize, bits | (V_REWRITTEN if clip_forward_read > 0 else 0)]
        plan[r_ord] = [REVERSE, clip_reverse_read, reverse_read.pos, len(reverse_read.cigar), reverse_read.isize, bits | (V_REWRITTEN if clip_reverse_read > 0 else 0)]
        reads_saved += 2
        if skip_al:
            removed.append(al.name)
            continue
        out.append(forward_read.bytes()); out.append(reverse_read.bytes())
    for a, _ in al_map.values():
        out.append(a.bytes()); reads_saved += 1
    if reads_saved != reads_count:
        raise ClipError(0, f"Lost Reads: {reads_count - reads_saved}/{reads_count}")
    # the counters other than bases_* are `int`
    res = Result()
    res.records, res.plan, res.removed = out, plan, removed
    res.counts = [_i32(reads_count), _i32(reads_saved), _i32(reads_clipped), _i32(reads_mismatch), bases_count, bases_clipped]
    res.summary = summary_lines(res.counts)
    res.log = "".join(s + "\n" for s in log + res.summary)
    return res


def summary_lines(c):
    return [f"Overlap mismatch filtering was used for {c[3]} of {c[0]} reads ({fmt_pct(c[3], c[0])} %).",
            f"Softclipped {c[2]} of {c[0]} reads ({fmt_pct(c[2], c[0])} %).",
            f"Softclipped {c[5]} of {c[4]} basepairs ({fmt_pct(c[5], c[4])} %)."]


def run_file(path, mode=0, ignore_indels=False, verbose=True):
    header, recs = read_bam(path)
    return run(header, recs, mode, ignore_indels, verbose)
