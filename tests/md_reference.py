"""A local reference FASTA rebuilt from the reads of a BAM: aligned read bases, with the MD tag's mismatches and ^DEL runs applied. The fixture BAMs carry MD
tags, so the tool tests need no hg38: only the contigs asked for are written, each cut off a few kb behind its last covered base, positions no read covers
are N (as are the reads whose MD tag no longer matches their CIGAR), and every position is checked to be the same in all reads that cover it."""
import re

import variant_oracle as V

MD_TOKEN = re.compile(r"(\d+)|(\^[A-Za-z]+)|([A-Za-z])")


def _md(img, aux, end):
    p = aux
    sizes = {ord("A"): 1, ord("c"): 1, ord("C"): 1, ord("s"): 2, ord("S"): 2, ord("i"): 4, ord("I"): 4, ord("f"): 4, ord("d"): 8}
    while p + 3 <= end:
        tag, t = bytes(img[p:p + 2]), int(img[p + 2])
        if t in (ord("Z"), ord("H")):
            q = p + 3
            while q < end and img[q]:
                q += 1
            if tag == b"MD":
                return bytes(img[p + 3:q]).decode()
            p = q + 1
        elif t in sizes:
            p += 3 + sizes[t]
        elif t == ord("B"):
            st, n = chr(img[p + 3]), V._u32(img, p + 4)
            p += 8 + n * (1 if st in "cC" else 2 if st in "sS" else 4)
        else:
            return None
    return None


def rebuild(bam, contigs, tail=5000):
    """{contig: sequence} for the contigs named (reference names of the BAM)"""
    refs = [n for n, _ in bam.refs]
    want = {refs.index(c) for c in contigs}
    img, offs = bam.inflated(), bam.record_offsets()
    known = {t: {} for t in want}
    for r, o in zip(V.reads(bam), offs):
        if r.tid not in want or r.flag & 0x4 or r.l_seq == 0:
            continue
        o = int(o)
        aux = r._seq_off + (r.l_seq + 1) // 2 + r.l_seq
        md = _md(img, aux, o + 4 + V._u32(img, o))
        if md is None:
            continue
        seq = r.bases()
        # reference positions in MD order: aligned bases (with the read's base) and deleted bases (None)
        cols, gp, rp = [], r.start, 0
        for op, n in r.cigar:
            if op in (0, 7, 8):
                cols += [(gp + k, seq[rp + k]) for k in range(n)]; gp += n; rp += n
            elif op == 2:
                cols += [(gp + k, None) for k in range(n)]; gp += n
            elif op == 3:
                gp += n
            elif op in (1, 4):
                rp += n
        toks = MD_TOKEN.findall(md)
        if sum(int(a) if a else (len(d) - 1 if d else 1) for a, d, _ in toks) != len(cols):
            continue   # (an MD tag written before bases were soft-clipped - overlap clipping - no longer describes the alignment)
        k = 0
        for num, dele, mis in toks:
            if num:
                for _ in range(int(num)):
                    pos, b = cols[k]; k += 1
                    _put(known[r.tid], pos, b.upper())
            elif dele:
                for b in dele[1:]:
                    pos, _ = cols[k]; k += 1
                    _put(known[r.tid], pos, b.upper())
            else:
                pos, _ = cols[k]; k += 1
                _put(known[r.tid], pos, mis.upper())
    out = {}
    for t in want:
        kn = known[t]
        n = (max(kn) if kn else 0) + tail
        s = ["N"] * n
        for pos, b in kn.items():
            s[pos - 1] = b
        out[refs[t]] = "".join(s)
    return out


def _put(d, pos, b):
    old = d.get(pos)
    if old is None or old == "N":
        d[pos] = b
    elif b != "N":
        assert old == b, f"reads disagree on the reference base at {pos}: {old} / {b}"


def write(bam, contigs, path, line=60):
    """writes path (FASTA) and path.fai; returns the genome as {contig: sequence}"""
    g = rebuild(bam, contigs)
    with open(path, "w") as f, open(path + ".fai", "w") as fai:
        for name in contigs:
            s = g[name]
            fai.write(f"{name}\t{len(s)}\t{f.tell() + len(name) + 2}\t{line}\t{line + 1}\n")
            f.write(f">{name}\n")
            for i in range(0, len(s), line):
                f.write(s[i:i + line] + "\n")
    return g
