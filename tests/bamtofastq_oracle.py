"""BamToFastq restated in Python (src/BamToFastq/main.cpp:77-196 over BamReader, Sequence and FastqOutfileStream), independent of the device: BAMs are read
with bamfilter_oracle.read_bam.

to_fastq(records, ...) -> (out1 text, out2 text or None, counts). The text is what gzread gives back of the reference's gzip files: every entry is written with
gzputs, so a quality that became NUL (q = 223) ends its line early. A reverse-strand record whose reversed sequence holds a base other than ACGTN raises
ComplementError with the base, as Sequence::complement does, for the first such entry in output order."""
import glob
import os
import re
import struct
import tempfile

from bamfilter_oracle import Rec, read_bam

NT16 = "=ACMGRSVTWYHKDBN"
COMP = {"A": "T", "C": "G", "T": "A", "G": "C", "N": "N"}
COUNT_FIELDS = ("paired", "unpaired", "unmatched", "single_end", "duplicates", "fixed", "max_cached")


_joined = {}


def fixture(path):
    """a fixture file; one larger than a committed file may be is kept as <name>.part0, .part1, ... and joined into a temporary directory on first use"""
    if os.path.exists(path):
        return path
    if path not in _joined:
        parts = sorted(glob.glob(path + ".part*"))
        assert parts, path
        d = tempfile.mkdtemp(prefix="ngsqc_fixture_")
        out = os.path.join(d, os.path.basename(path))
        with open(out, "wb") as f:
            for q in parts:
                f.write(open(q, "rb").read())
        _joined[path] = out
    return _joined[path]


class ComplementError(Exception):
    def __init__(self, base):
        super().__init__(f"Could not convert base '{base}' to complement!")
        self.base = base


class RegionError(Exception):
    pass


def bases(r):
    s = r.b[r.seq_off:r.seq_off + (r.l_seq + 1) // 2]
    return "".join(NT16[(s[i >> 1] >> (4 - 4 * (i & 1))) & 15] for i in range(r.l_seq))


def quals(r):
    q = r.b[r.seq_off + (r.l_seq + 1) // 2:r.aux_off]
    return bytes((x + 33) & 255 for x in q)


def entry(r, extend=0):
    """the bytes one FASTQ entry leaves in the file (alignmentToFastq, then FastqOutfileStream::write)"""
    b, q = bases(r), quals(r)
    if r.flag & 0x10:
        b = b[::-1]
        for c in b:
            if c not in COMP:
                raise ComplementError(c)
        b = "".join(COMP[c] for c in b)
        q = q[::-1]
    if extend > 0 and len(b) < extend:
        q += b"#" * (extend - len(b))
        b += "N" * (extend - len(b))
    q = q.split(b"\0", 1)[0]   # gzputs writes up to the first NUL
    return b"@" + r.name + b"\n" + b.encode() + b"\n+\n" + q + b"\n"


def endpos(r):
    """bam_endpos: pos + reference length of the effective CIGAR, one base for an unmapped record or an empty span"""
    rlen = 0 if r.flag & 4 else sum(c >> 4 for c in r.effective_cigar() if c & 15 in (0, 2, 3, 7, 8))
    return r.pos + max(rlen, 1)


def in_region(r, region):
    """htslib's iterator (sam_itr_queryi(idx, tid, start - 1, end)): region = (tid, start, end), 1-based closed"""
    tid, start, end = region
    return r.tid == tid and r.pos < end and endpos(r) > start - 1


def to_fastq(records, paired=True, remove_duplicates=False, extend=0, fix=False, region=None):
    c = dict.fromkeys(COUNT_FIELDS, 0)
    out1, out2 = [], [] if paired else None
    cache, seen = {}, set()
    for b in records:
        r = Rec(b)
        if region is not None and not in_region(r, region):
            continue
        if r.flag & 0x900:
            continue
        if remove_duplicates and r.flag & 0x400:
            c["duplicates"] += 1
            continue
        if fix:
            k = (r.name, bool(r.flag & 0x40))
            if k in seen:
                c["fixed"] += 1
                continue
            seen.add(k)
        if paired:
            if not r.flag & 1:
                c["unpaired"] += 1
                continue
            if r.name in cache:
                mate = cache.pop(r.name)
                first, second = (r, mate) if r.flag & 0x40 else (mate, r)
                out1.append(entry(first, extend)); out2.append(entry(second, extend))
                c["paired"] += 1
            else:
                cache[r.name] = r
            c["max_cached"] = max(c["max_cached"], len(cache))
        else:
            out1.append(entry(r, extend))
            c["single_end"] += 1
    c["unmatched"] = len(cache) if paired else 0
    return b"".join(out1), (b"".join(out2) if paired else None), c


def to_fastq_file(path, **kw):
    _, recs = read_bam(path)
    return to_fastq(recs, **kw)


def stdout_lines(c, paired, remove_duplicates=False, fix=False):
    """main()'s report without its last line (the elapsed time)"""
    if paired:
        s = [f"Pair reads (written)            : {c['paired']}", f"Unpaired reads (skipped)        : {c['unpaired']}",
             f"Unmatched paired reads (skipped): {c['unmatched']}"]
    else:
        s = [f"Reads (written)                 : {c['single_end']}"]
    if remove_duplicates:
        s.append(f"Duplicate tagged reads (skipped): {c['duplicates']}")
    if fix:
        s.append(f"Duplicate name reads (skipped)  : {c['fixed']}")
    return s + ["", f"Maximum cached reads            : {c['max_cached']}"]


def parse_region(s):
    """BedLine::fromString (src/cppNGS/BedFile.cpp:37-70) -> (chromosome, start, end); RegionError where the line is not valid"""
    t = re.sub("[ ]+", "\t", s.replace(":", "\t").replace("-", "\t"))
    parts = t.split("\t")
    if len(parts) < 3:
        raise RegionError(s)
    try:
        start, end = (_to_int(p.replace(",", "")) for p in parts[1:3])
    except ValueError:
        raise RegionError(s)
    chrom = parts[0].strip()
    if not _chr_valid(chrom) or start < 0 or start > end:
        raise RegionError(s)
    return chrom, start, end


def _to_int(p):
    """Helper::toInt: QString::toInt on the trimmed text"""
    p = p.strip()
    if not re.fullmatch(r"[+-]?[0-9]+", p):
        raise ValueError(p)
    v = int(p)
    if not -2 ** 31 <= v < 2 ** 31:
        raise ValueError(p)
    return v


def _chr_valid(c):
    """Chromosome::isValid: a non-empty name once a leading 'chr' is taken off"""
    c = c.strip()
    if c.lower().startswith("chr"):
        c = c[3:]
    return c != ""


def make_record(name, flag, seq, qual, tid=0, pos=100, mapq=60, cigar=None):
    """a BAM record (block_size included) for hand cases: seq a string over NT16, qual a list of raw values"""
    n = name.encode() + b"\0"
    l_seq = len(seq)
    cig = cigar if cigar is not None else ([l_seq << 4] if l_seq else [])
    codes = [NT16.index(ch) for ch in seq]
    if len(codes) & 1:
        codes.append(0)
    packed = bytes(codes[i] << 4 | codes[i + 1] for i in range(0, len(codes), 2))
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(n), mapq, 4680, len(cig), flag, l_seq, tid, pos + 100, 0) + n
    body += struct.pack(f"<{len(cig)}I", *cig) + packed + bytes(qual)
    return struct.pack("<I", len(body)) + body
