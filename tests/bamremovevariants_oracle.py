"""BamRemoveVariants restated in Python (src/BamRemoveVariants/main.cpp:34-278 over BamReader / BamWriter / TabixIndexedFile / Variant), independent of the
device: BAMs are read with Python's gzip (bamfilter_oracle), the VCF.GZ with gzip too.

parse_vcf(text) -> [Line]: every data line with the span tabix gives it and what Variant(VcfLine(chr, POS, REF, [ALT])) makes of it (SNV / OTHER / INVALID).
table(lines, ref_names) -> the rows (tid, beg, end, start, kind, ref, obs) the library takes.
run(records, lines, ref_names, mask, single_end, keep_indels) -> (written record bytes, counts); raises RmError where the reference throws.
verdicts(records, lines, ref_names, mask, keep_indels) -> one byte per record: bit 0 passes, bit 1 modified, bit 2 skipped, bit 3 error.

Where the reference's behaviour is undefined this file says what the project does: a read index outside [0, l_seq) (extractBaseByCIGAR reads in front of or
behind the sequence there) gives no base; a record with tid < 0 (chrs_[-1]) or pos < 0 overlaps nothing; CIGAR operations the walks throw on (P, B) are stepped over."""
import gzip
import struct

from bamfilter_oracle import Rec, read_bam, written  # noqa: F401

SNV, OTHER, INVALID = 0, 1, 2
ERR_INVALID_LINE, ERR_POS_NOT_FOUND, ERR_BAD_BASE = 1, 2, 3
NT16 = "=ACMGRSVTWYHKDBN"
_special = {}


def chrom_num(name):
    """Chromosome::num() (src/cppNGS/Chromosome.cpp)"""
    t = name.strip().upper()
    if t.startswith("CHR"):
        t = t[3:]
    if t == "M":
        t = "MT"
    if not t:
        return 0
    if t in ("X", "Y", "MT"):
        return {"X": 1001, "Y": 1002, "MT": 1003}[t]
    if t[0] != "0" and t.isdigit() and len(t) <= 9 and 0 < int(t) <= 1000:
        return int(t)
    return _special.setdefault(t, 1004 + len(_special))


def normalize(start, ref, obs):
    """Variant::normalize(start, ref, obs) (VariantList.cpp:1283-1307)"""
    def multi():
        return (len(ref) != 1 or len(obs) != 1) and ref and obs
    if multi() and ref[0] == obs[0]:
        ref, obs, start = ref[1:], obs[1:], start + 1
    while multi() and ref[-1] == obs[-1]:
        ref, obs = ref[:-1], obs[:-1]
    while multi() and ref[0] == obs[0]:
        ref, obs, start = ref[1:], obs[1:], start + 1
    return start, ref, obs


def only_acgt(s):
    return bool(s) and all(c in "ACGT" for c in s)


class Line:
    def __init__(self, chrom, pos, ref, alt, info=None):
        self.chr, self.pos, self.ref, self.alt = chrom, pos, ref, alt
        self.beg, self.end = pos, pos + len(ref) - 1
        if info is not None:   # htslib's tbx_parse1: INFO END=<n> moves the end when it lies behind POS - 1
            s = 4 if info.startswith("END=") else (info.find(";END=") + 5 if ";END=" in info else -1)
            if s >= 0 and s < len(info) and info[s] != ".":
                digits = ""
                for c in info[s:]:
                    if not (c.isdigit() or (c == "-" and not digits)):
                        break
                    digits += c
                e = int(digits) if digits not in ("", "-") else 0
                if e > pos - 1:
                    self.end = e
        # Variant(const VcfLine&) (VariantList.cpp:49-64): VcfLine::isValid (VcfLine.cpp:405-425) with the ALT column as ONE allele, then normalize("-", true)
        self.message = ""
        if chrom_num(chrom) <= 0 or pos < 0 or not only_acgt(ref) or not (only_acgt(alt) or alt == "<NON_REF>"):
            self.kind, self.start, self.vref, self.vobs = INVALID, pos, "", ""
            self.message = f"Cannot convert invalid VCF variant to GSvar variant: {chrom}:{pos} {ref}>{alt}"
            return
        start, r, o = normalize(pos, ref, alt)
        if not r:
            start -= 1   # (GSvar format: an insertion sits on the base in front of it)
        self.start, self.vref, self.vobs = start, r or "-", o or "-"
        self.kind = SNV if len(self.vref) == 1 and len(self.vobs) == 1 and self.vref != "-" and self.vobs != "-" else OTHER


class VcfOrderError(Exception):
    pass


def parse_vcf(text):
    lines, seen, prev = [], [], None
    for raw in text.split("\n"):
        if not raw or raw[0] == "#":
            continue
        c = raw.split("\t")
        try:
            pos = int(c[1]) if c[1].strip() == c[1] else 0
        except ValueError:
            pos = 0
        if prev is None or prev[0] != c[0]:
            if c[0] in seen:
                raise VcfOrderError(f"chromosome {c[0]} comes again")
            seen.append(c[0])
        elif pos < prev[1]:
            raise VcfOrderError(f"position {pos} behind {prev[1]}")
        prev = (c[0], pos)
        lines.append(Line(c[0], pos, c[3], c[4], c[7] if len(c) > 7 else None))
    return lines


def load_vcf(path):
    return parse_vcf(gzip.open(path, "rb").read().decode("latin-1"))


def line_tids(lines, ref_names):
    """tid per line: of the VCF's names with one Chromosome::num() the last one named is looked up (TabixIndexedFile.cpp:40-45); its lines go to the first
    reference of the BAM with that number, every other line gets -1"""
    names = []
    for ln in lines:
        if ln.chr not in names:
            names.append(ln.chr)
    name_of_num = {chrom_num(n): n for n in names}
    tid_of_num = {}
    for t, n in enumerate(ref_names):
        tid_of_num.setdefault(chrom_num(n), t)
    return [tid_of_num.get(chrom_num(ln.chr), -1) if name_of_num[chrom_num(ln.chr)] == ln.chr else -1 for ln in lines]


def table(lines, ref_names):
    return [(t, ln.beg, ln.end, ln.start, ln.kind, ln.vref.encode() if ln.kind == SNV else 0, ln.vobs.encode() if ln.kind == SNV else 0)
            for t, ln in zip(line_tids(lines, ref_names), lines)]


class RmError(Exception):
    def __init__(self, code, variant, message):
        super().__init__(message)
        self.code, self.variant, self.message, self.record = code, variant, message, -1


class Aln:
    """a record with its sequence as a mutable list of nibbles"""
    def __init__(self, b, rec=None):
        self.r = r = rec or Rec(b)
        self.cigar = [(c & 15, c >> 4) for c in r.effective_cigar()]
        raw = b[r.seq_off:r.seq_off + (r.l_seq + 1) // 2]
        self.seq = [int(c, 16) for c in raw.hex()[:r.l_seq]]   # (a nibble per base, the even index in the high half)
        self.seq0, self.bad = list(self.seq), None
        self.start = r.pos + 1
        rlen = 0 if r.flag & 4 else sum(n for op, n in self.cigar if op in (0, 2, 3, 7, 8))
        self.end = r.pos + max(1, rlen)   # bam_endpos

    def bytes(self):
        if self.seq == self.seq0:
            return self.r.b
        r, b = self.r, bytearray(self.r.b)
        for i in range(r.l_seq):
            if self.seq[i] != self.seq0[i]:
                o = r.seq_off + i // 2
                b[o] = (b[o] & 0x0f) | self.seq[i] << 4 if i % 2 == 0 else (b[o] & 0xf0) | self.seq[i]
        return bytes(b)

    def written(self):
        """what BamWriter::writeAlignment writes for the record as it is now"""
        return written(self.r if self.seq == self.seq0 else Rec(self.bytes()))

    def extract_base(self, pos):
        """extractBaseByCIGAR (BamReader.cpp:307-374) -> (base character, read index or -1); None where it throws 'Could not find position'"""
        if all(op in (1, 4) for op, _ in self.cigar):
            return "~", -1
        rp, gp = 0, self.start - 1
        for op, n in self.cigar:
            if op in (0, 7, 8):
                gp += n; rp += n
            elif op == 1:
                rp += n
            elif op == 2:
                gp += n
                if gp >= pos:
                    return "-", -1
            elif op == 3:
                gp += n
                if gp >= pos:
                    return "~", -1
            elif op == 4:
                rp += n
                if rp >= self.r.l_seq:
                    return "~", -1
            if gp >= pos:
                ap = rp - (gp + 1 - pos)
                return (NT16[self.seq[ap]], ap) if 0 <= ap < self.r.l_seq else ("~", -1)
        return None

    def has_indel(self, pos, window=50):
        """extractIndelsByCIGAR(pos, 50) is non-empty (BamReader.cpp:376-439)"""
        gp = self.start
        for op, n in self.cigar:
            if op in (0, 7, 8, 3):
                gp += n
            elif op in (1, 2):
                if pos - window <= gp <= pos + window:
                    return True
                if op == 2:
                    gp += n
            if gp > pos + window:
                break
        return False


def matches(a, lines, tids):
    """getMatchingLines(chr, start, end) (TabixIndexedFile.cpp:96-129): the lines of the record's chromosome that meet [start, end], in file order"""
    if a.r.tid < 0 or a.r.pos < 0:
        return []
    return [(i, ln) for i, (ln, t) in enumerate(zip(lines, tids)) if t == a.r.tid and ln.beg <= a.end and ln.end >= a.start]


def visit(a, lines, tids, mask, keep_indels):
    """alignment_pass (:34-66) / mask_alignment (:68-110): passes; a.seq is rewritten under mask"""
    for i, ln in matches(a, lines, tids):
        if ln.kind == INVALID:
            raise RmError(ERR_INVALID_LINE, i, ln.message)
        if ln.kind == SNV:
            got = a.extract_base(ln.start)
            if got is None:
                raise RmError(ERR_POS_NOT_FOUND, i, f"Could not find position {ln.start} in read {a.r.name.decode()} with start position {a.start}!")
            base, idx = got
            if base == ln.vobs:
                if not mask:
                    return False
                if a.bad is None:   # setBases (BamReader.cpp:161-168) rewrites the whole read; what it refuses is never a base that was set
                    a.bad = [j for j, v in enumerate(a.seq0) if v not in (1, 2, 4, 8, 15)]
                if a.bad:
                    raise RmError(ERR_BAD_BASE, a.bad[0], f"Cannot store character '{NT16[a.seq0[a.bad[0]]]}' in BAM/CRAM file. Only A,C,G,T,N are allowed!")
                a.seq[idx] = NT16.index(ln.vref)
        elif a.has_indel(ln.start):
            return keep_indels if mask else False
    return True


def verdicts(records, lines, ref_names, mask=False, keep_indels=False):
    tids, out = line_tids(lines, ref_names), bytearray()
    for b in records:
        a = Aln(b)
        if a.r.flag & 0x900:
            out.append(4); continue
        try:
            ok = visit(a, lines, tids, mask, keep_indels)
            out.append((1 if ok else 0) | (2 if a.seq != a.seq0 else 0))
        except RmError:
            out.append(8)
    return bytes(out)


def run(records, lines, ref_names, mask=False, single_end=False, keep_indels=False):
    tids = line_tids(lines, ref_names)
    out, cache = [], {}
    c = dict(passed=0, dropped=0, modified=0, skipped=0)

    def evaluate(k, b, r):
        a = Aln(b, r)
        try:
            return a, visit(a, lines, tids, mask, keep_indels)
        except RmError as e:
            e.record = k
            raise

    for k, b in enumerate(records):
        r = Rec(b)
        if r.flag & 0x900:
            c["skipped"] += 1; continue
        if single_end:
            a, ok = evaluate(k, b, r)
            if ok:
                out.append(a.written()); c["passed"] += 1
                c["modified"] += a.seq != a.seq0
            else:
                c["dropped"] += 1
        elif r.name not in cache:
            a, ok = evaluate(k, b, r)
            cache[r.name] = (a, ok)
            c["modified"] += a.seq != a.seq0
        else:
            o, o_ok = cache.pop(r.name)
            if not o_ok:   # (the closer is not looked at, :218 / :251)
                c["dropped"] += 1; continue
            a, ok = evaluate(k, b, r)
            c["modified"] += a.seq != a.seq0
            if ok:
                out += [o.written(), a.written()]; c["passed"] += 1
            else:
                c["dropped"] += 1
    return out, c


def run_file(bam_path, vcf_path, ref_names, **kw):
    header, recs = read_bam(bam_path)
    out, c = run(recs, load_vcf(vcf_path), ref_names, **kw)
    return header, out, c


def ref_names_of(header):
    """the reference names of a BAM header (read_bam's header bytes)"""
    o = 4
    o += 4 + struct.unpack_from("<I", header, o)[0]
    n = struct.unpack_from("<I", header, o)[0]; o += 4
    names = []
    for _ in range(n):
        ln = struct.unpack_from("<I", header, o)[0]
        names.append(header[o + 4:o + 4 + ln - 1].decode()); o += 4 + ln + 4
    return names
