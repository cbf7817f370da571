"""BamFilter restated in Python (src/BamFilter/main.cpp:35-134 over BamReader / BamWriter), independent of the device: BAMs are read with Python's gzip.

filter_pairs(records, **thresholds) -> (kept record bytes in output order, pairs passed, pairs dropped). A record whose CIGAR comes from its CG tag is written as
htslib's bam_write1 writes what bam_read1 made of it (from memory of htslib's sam.c, bam_tag2cigar / bam_write1): up to 65535 operations inline without the tag,
more as the placeholder "l_seq S, ref_len N" with CG:B,I appended behind the other tags; bin recomputed from the real span in both cases."""
import gzip
import struct

DEFAULTS = dict(min_mq=30, max_mq=256, max_mm=4, max_gap=1, min_dup=0, max_is=-1)


def read_bam(path_or_bytes):
    """(header bytes, [record bytes, block_size included]) of a BAM"""
    raw = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else open(path_or_bytes, "rb").read()
    d = gzip.decompress(raw)
    assert d[:4] == b"BAM\x01"
    o = 4
    l_text = struct.unpack_from("<I", d, o)[0]; o += 4 + l_text
    n_ref = struct.unpack_from("<I", d, o)[0]; o += 4
    for _ in range(n_ref):
        l_name = struct.unpack_from("<I", d, o)[0]; o += 4 + l_name + 4
    header, recs = d[:o], []
    while o < len(d):
        bs = struct.unpack_from("<I", d, o)[0]
        recs.append(d[o:o + 4 + bs]); o += 4 + bs
    return header, recs


class Rec:
    def __init__(self, b):
        self.b = b
        (self.bs, self.tid, self.pos, self.l_name, self.mapq, self.bin, self.n_cigar, self.flag, self.l_seq, self.mtid, self.mpos,
         self.isize) = struct.unpack_from("<IiiBBHHHiiii", b, 0)
        # BamAlignment::name() (src/cppNGS/BamReader.h:69-72): bam_get_qname read as a C string - the bytes of the name field in front of its first NUL
        self.name = b[36:36 + self.l_name].split(b"\0", 1)[0]
        self.cig_off = 36 + self.l_name
        self.cigar = list(struct.unpack_from(f"<{self.n_cigar}I", b, self.cig_off))
        self.seq_off = self.cig_off + 4 * self.n_cigar
        self.aux_off = self.seq_off + (self.l_seq + 1) // 2 + self.l_seq

    def aux(self):
        """[(tag, type, value bytes start, end)] of the optional fields"""
        out, b, o = [], self.b, self.aux_off
        sizes = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4, "d": 8}
        while o + 3 <= len(b):
            tag, t = b[o:o + 2], chr(b[o + 2]); v = o + 3
            if t in sizes:
                e = v + sizes[t]
            elif t in "ZH":
                e = b.index(b"\0", v) + 1
            elif t == "B":
                st, n = chr(b[v]), struct.unpack_from("<I", b, v + 1)[0]
                e = v + 5 + n * (1 if st in "cC" else 2 if st in "sS" else 4)
            else:
                break
            out.append((tag, t, o, e)); o = e
        return out

    def tagi(self, tag):
        """BamAlignment::tagi (bam_aux2i): integer types as integers, anything else and a missing tag 0"""
        for tg, t, o, _ in self.aux():
            if tg == tag:
                fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}.get(t)
                return struct.unpack_from(fmt, self.b, o + 3)[0] if fmt else 0
        return 0

    def cg(self):
        """(ops, tag start, tag end) when the CIGAR comes from the CG tag (htslib bam_tag2cigar, as the oracle's parse_rec: a placed record, tid >= 0 and pos >= 0), else None"""
        if not self.cigar or self.tid < 0 or self.pos < 0:
            return None
        if self.cigar[0] & 15 != 4 or self.cigar[0] >> 4 != self.l_seq:
            return None
        for tg, t, o, e in self.aux():
            if tg == b"CG":
                if t != "B" or chr(self.b[o + 3]) != "I":
                    return None
                n = struct.unpack_from("<I", self.b, o + 4)[0]
                if n < self.n_cigar or n >= 1 << 29:
                    return None
                return list(struct.unpack_from(f"<{n}I", self.b, o + 8)), o, e
        return None

    def effective_cigar(self):
        g = self.cg()
        return g[0] if g else self.cigar


def alignment_pass(r, min_mq, max_mq, max_mm, max_gap, min_dup, max_is):
    n_gaps = indel = 0
    for c in r.effective_cigar():
        if c & 15 in (1, 2):
            indel += c >> 4; n_gaps += 1
    mm = r.tagi(b"NM") - indel
    dup = r.tagi(b"DP")
    return (not r.flag & 4 and bool(r.flag & 1) and not r.flag & 8 and min_mq <= r.mapq <= max_mq and (max_gap == -1 or n_gaps <= max_gap)
            and (max_mm == -1 or mm <= max_mm) and dup >= min_dup and (max_is == -1 or r.isize <= max_is))


def reg2bin(beg, end):
    end -= 1
    for shift, off in ((14, ((1 << 15) - 1) // 7), (17, ((1 << 12) - 1) // 7), (20, ((1 << 9) - 1) // 7), (23, ((1 << 6) - 1) // 7), (26, ((1 << 3) - 1) // 7)):
        if beg >> shift == end >> shift:
            return off + (beg >> shift)
    return 0


def written(r):
    """the bytes BamWriter::writeAlignment writes for the record"""
    g = r.cg()
    if not g:
        return r.b
    ops, t0, t1 = g
    b = r.b
    rlen = sum(c >> 4 for c in ops if c & 15 in (0, 2, 3, 7, 8))
    end = r.pos + (1 if (r.flag & 4) or rlen == 0 else rlen)
    inline = len(ops) <= 65535
    cig = struct.pack(f"<{len(ops)}I", *ops) if inline else struct.pack("<II", r.l_seq << 4 | 4, rlen << 4 | 3)
    body = b[r.seq_off:t0] + b[t1:] + (b"" if inline else b[t0:t1])
    core = bytearray(b[:36])
    struct.pack_into("<HH", core, 14, reg2bin(r.pos, end), len(ops) if inline else 2)
    out = bytes(core) + b[36:36 + r.l_name] + cig + body
    return struct.pack("<I", len(out) - 4) + out[4:]


def filter_pairs(records, **kw):
    p = dict(DEFAULTS); p.update(kw)
    cache, out, passed, dropped = {}, [], 0, 0
    for b in records:
        r = Rec(b)
        if r.flag & 0x900:
            continue
        if r.name not in cache:
            cache[r.name] = (r, alignment_pass(r, **p))
        else:
            o, ok = cache.pop(r.name)
            if ok and alignment_pass(r, **p):
                out += [written(o), written(r)]; passed += 1
            else:
                dropped += 1
    return out, passed, dropped


def filter_file(path, **kw):
    header, recs = read_bam(path)
    out, passed, dropped = filter_pairs(recs, **kw)
    return header, out, passed, dropped
