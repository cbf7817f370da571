"""Plain model of the per-entry FASTQ-to-FASTQ tools of the reference - FastqTrim (src/FastqTrim/main.cpp:47-73), FastqConvert (src/FastqConvert/main.cpp:33-41),
FastqExtract (src/FastqExtract/main.cpp:39-90) and FastqExtractUMI (src/FastqExtractUMI/main.cpp:48-74) - written as the tools are: an entry is four byte strings
that are cut, joined and written. What it is judged by: the reference's own 13 test methods (tests/test_cpu_fastqtools.py). What it then judges: the plan records
and output text of csrc/fqedit_visit.h on the CPU and of csrc/fqedit.hip on the GPU. How a text falls into entries and how an entry is validated are
tests/fastq_model.py's."""
import numpy as np

import fastq_model as F

PLAN_COLUMNS = ("keep", "ins_at", "ins_len", "b_off", "b_len", "q_off", "q_len", "q_delta")
NO_LENGTH, ABSENT = -1, -2


class EditError(Exception):
    def __init__(self, entry, kind, message):
        super().__init__(message)
        self.entry, self.kind = entry, kind


class Result:
    """plan: (n, 8) int32, (n, 2, 8) for the paired tool; out: the text of each output; stats: what ngsqc_fqedit_stats counts; error: None or EditError"""

    def __init__(self, plan, out, entries, error=None):
        self.plan, self.out, self.error = plan, out, error
        self.stats = dict(entries=entries, written=[int(p[..., 0].sum()) if p.size else 0 for p in self._sides()], bytes=[len(o) for o in out] + [0] * (2 - len(out)))
        self.stats["written"] += [0] * (2 - len(self.stats["written"]))

    def _sides(self):
        return [self.plan] if self.plan.ndim == 2 else [self.plan[:, 0], self.plan[:, 1]]


def _row(keep, entry, b_off, b_len, q_off, q_len, ins_at=0, ins_len=0, q_delta=0):
    if not keep:   # a dropped entry: the whole lines
        return [0, 0, 0, 0, len(entry[1]), 0, len(entry[3]), 0]
    return [1, ins_at, ins_len, b_off, b_len, q_off, q_len, q_delta]


def _write(entry):
    return b"".join(l + b"\n" for l in entry)


def _finish(rows, out, n, shape):
    plan = np.array(rows, np.int32).reshape(shape)
    return Result(plan, [b"".join(o) for o in out], n)


def trim(text, start=0, end=0, len_=0, max_len=0):
    """no line grows: where the reference's resize() would lengthen the quality line with unspecified bytes, the line stays as it is"""
    rows, out = [], []
    entries = F.entries_of(text)
    for e in entries:
        header, bases, header2, quals = e
        if max_len > 0 and len(bases) >= max_len:
            rows.append(_row(1, e, 0, len(bases), 0, len(quals))); out.append(_write(e))
            continue
        b_off = q_off = 0
        if start > 0 or end > 0:
            n = len(bases)
            if n <= start + end:
                rows.append(_row(0, e, 0, 0, 0, 0))
                continue
            q_off = min(start, len(quals))
            bases, quals, b_off = bases[start:n - end], quals[start:n - end], start   # QByteArray::mid(start, n - start - end)
        if len_ > 0 and len(bases) > len_:
            bases, quals = bases[:len_], quals[:len_]
        rows.append(_row(1, e, b_off, len(bases), q_off, len(quals))); out.append(_write((header, bases, header2, quals)))
    return _finish(rows, [out], len(entries), (-1, 8))


def convert(text):
    rows, out = [], []
    entries = F.entries_of(text)
    for e in entries:
        quals = bytes((c - 31) & 255 for c in e[3])
        rows.append(_row(1, e, 0, len(e[1]), 0, len(quals), q_delta=-31)); out.append(_write((e[0], e[1], e[2], quals)))
    return _finish(rows, [out], len(entries), (-1, 8))


def to_int(text):
    """Helper::toInt: QString::toInt on the trimmed text; None when it is no int"""
    t = text.strip(b" \t\n\v\f\r")
    body = t[1:] if t[:1] in (b"+", b"-") else t
    if not body or not body.isdigit() or not all(48 <= c <= 57 for c in body):
        return None
    v = int(t)
    return v if -2 ** 31 <= v < 2 ** 31 else None


def parse_ids(text):
    """the id file (main.cpp:41-52) -> ([id], [length]) in file order, -1 for an id without a length; raises ValueError with Helper::toInt's message"""
    names, lengths = [], []
    for line in bytes(text).split(b"\n"):
        line = line.strip(b" \t\n\v\f\r")
        if not line or line[:1] == b"#":
            continue
        parts = line.split(b"\t")
        length = NO_LENGTH
        if len(parts) > 1:
            length = to_int(parts[1])
            if length is None:
                raise ValueError("Could not convert length value '%s' to integer" % parts[1].decode("latin-1"))
        names.append(parts[0]); lengths.append(length)
    return names, lengths


def entry_id(header):
    i = header.strip(b" \t\n\v\f\r")[1:]
    sp = i.find(b" ")
    return i if sp < 0 else i[:sp]


def extract(text, names, lengths=None, invert=False, long_read=False):
    ids = {}
    for k, n in enumerate(names):
        ids[bytes(n)] = NO_LENGTH if lengths is None or lengths[k] is None else int(lengths[k])   # (QHash::insert: the last one wins)
    rows, out = [], []
    entries = F.entries_of(text)
    error = None
    for i, e in enumerate(entries):
        if len(e[0]):   # (FastqFileStream.cpp:151: an entry with an empty header is not validated)
            kind = F.validate(e, long_read)
            if kind:
                error = EditError(i, kind, F.message(e, kind, long_read))
                break
        length = ids.get(entry_id(e[0]), ABSENT)
        header, bases, header2, quals = e
        if length == ABSENT:
            keep = invert
        elif length == NO_LENGTH:
            keep = not invert
        elif length >= 1:
            keep = not invert
            if keep:
                bases, quals = bases[:length], quals[:length]   # (a length beyond the read keeps the whole read: FastqExtract_out4)
        else:
            keep = False
        rows.append(_row(keep, e, 0, len(bases), 0, len(quals)))
        if keep:
            out.append(_write((header, bases, header2, quals)))
    r = _finish(rows, [out], len(rows), (-1, 8))
    r.error = error
    return r


def umi(text1, text2, cut1=0, cut2=0):
    """the UMI of a read shorter than its cut is the bases that exist"""
    e1, e2 = F.entries_of(text1), F.entries_of(text2)
    n = min(len(e1), len(e2))
    rows, out = [], [[], []]
    for a, b in zip(e1[:n], e2[:n]):
        barcode = b":%d,%d:" % (cut1, cut2) + a[1][:cut1] + b"," + b[1][:cut2]
        for k, (e, cut) in enumerate(((a, cut1), (b, cut2))):
            parts = e[0].split(b" ")
            at = len(parts[0])
            parts[0] += barcode
            bases, quals = e[1][cut:], e[3][cut:]
            rows.append(_row(1, e, min(cut, len(e[1])), len(bases), min(cut, len(e[3])), len(quals), ins_at=at, ins_len=len(barcode)))
            out[k].append(_write((b" ".join(parts), bases, e[2], quals)))
    return _finish(rows, out, n, (-1, 2, 8))


def run(op, text1, text2=None, ids=None, **kw):
    """one entry point with the library's parameter names: op "trim" / "extract" / "umi" / "convert" """
    if op == "trim":
        return trim(text1, kw.get("start", 0), kw.get("end", 0), kw.get("len", 0), kw.get("max_len", 0))
    if op == "convert":
        return convert(text1)
    if op == "umi":
        return umi(text1, text2, kw.get("cut1", 0), kw.get("cut2", 0))
    names, lengths = ids if ids is not None else ([], None)
    return extract(text1, names, lengths, kw.get("invert", False), kw.get("long_read", False))
