"""Plain model of four more per-entry FASTQ tools of the reference - FastqExtractBarcode (src/FastqExtractBarcode/main.cpp:44-60), FastqAddBarcode
(src/FastqAddBarcode/main.cpp:44-73), FastqDownsample (src/FastqDownsample/main.cpp:51-85) and FastqConcat (src/FastqConcat/main.cpp:40-51) - written as the
tools are: an entry is four byte strings that are cut, joined and written. What it is judged by: the reference's own seven test methods
(tests/test_cpu_fastqtools2.py). What it then judges: the plan records and output text of csrc/fqedit_visit.h on the CPU (tests/test_cpu_fqedit2_emul.py) and
of csrc/fqedit.hip on the GPU. Entries and plan rows are tests/fastq_model.py's and tests/fqedit_oracle.py's; the rand() stream is tests/bamdownsample_oracle.py's.

mutate: a named mistake built into the model, for the tests that show that the designed cases tell it from the model (None: the model itself)."""
import numpy as np

import bamdownsample_oracle as D
import fastq_model as F
from fqedit_oracle import Result, _finish, _row, _write

MUTATIONS = ("index range off by one", "ins_len one short at two digits", "keep bit of ordinal + 1")


def barcode_cut(text, cut=0, mutate=None):
    """plan (n, 2, 8): the main stream, then the index stream. QByteArray(read1.bases, cut) reads behind a shorter line in the reference: here the bytes that
    exist are taken, each line cut on its own."""
    entries = F.entries_of(text)
    rows, out = [], [[], []]
    icut = cut + 1 if mutate == MUTATIONS[0] else cut
    for e in entries:
        header, bases, header2, quals = e
        main = (header, bases[cut:], header2, quals[cut:])
        index = (header, bases[:icut], header2, quals[:icut])
        rows.append(_row(1, e, min(cut, len(bases)), len(main[1]), min(cut, len(quals)), len(main[3])))
        rows.append(_row(1, e, 0, len(index[1]), 0, len(index[3])))
        out[0].append(_write(main)); out[1].append(_write(index))
    return _finish(rows, out, len(entries), (-1, 2, 8))


def barcode_add(files, mutate=None):
    """files: [(text 1, text 2, barcode text)], one triple per position of the three file lists; every triple ends at its shortest file"""
    rows, out, n = [], [[], []], 0
    for t1, t2, t3 in files:
        e1, e2, e3 = F.entries_of(t1), F.entries_of(t2), F.entries_of(t3)
        m = min(len(e1), len(e2), len(e3))
        n += m
        for a, b, c in zip(e1[:m], e2[:m], e3[:m]):
            barcode = b":%d,0:" % len(c[1]) + c[1] + b","
            for k, e in enumerate((a, b)):
                parts = e[0].split(b" ")
                at = len(parts[0])
                parts[0] += barcode
                ins = len(barcode) - (1 if mutate == MUTATIONS[1] and len(c[1]) >= 10 else 0)
                rows.append(_row(1, e, 0, len(e[1]), 0, len(e[3]), ins_at=at, ins_len=ins))
                out[k].append(_write((b" ".join(parts), e[1], e[2], e[3])))
    return _finish(rows, out, n, (-1, 2, 8))


def downsample(text1, text2, seed=1, percentage=20.0, mutate=None):
    """one rand() per pair, in file order. Result.kept_headers: what -test prints behind "KEPT PAIR: ", each followed by a line feed; Result.side_entries: the
    entries of the two files, for "File a has more entries than b!" """
    if percentage <= 0 or percentage >= 100:
        raise ValueError("Invalid percentage %g!" % percentage)
    e1, e2 = F.entries_of(text1), F.entries_of(text2)
    n = min(len(e1), len(e2))
    shift = 1 if mutate == MUTATIONS[2] else 0
    keep = D.keep_stream(seed, percentage, 0, n + shift)[shift:]
    rows, out, headers = [], [[], []], []
    for a, b, k in zip(e1[:n], e2[:n], keep):
        for s, e in enumerate((a, b)):
            rows.append(_row(int(k), e, 0, len(e[1]), 0, len(e[3])))
            if k:
                out[s].append(_write(e))
        if k:
            headers.append(a[0] + b"\n")
    r = _finish(rows, out, n, (-1, 2, 8))
    r.kept_headers, r.side_entries = b"".join(headers), [len(e1), len(e2)]
    return r


def downsample_log(r):
    """STDOUT of the tool under -test"""
    kept = r.kept_headers.split(b"\n")[:-1]
    return b"".join(b"KEPT PAIR: " + h + b"\n" for h in kept) + b"PE reads read   : %d\nPE reads written: %d\n" % (r.stats["entries"], len(kept))


def concat(texts):
    """the files one after the other; every file ends on its own (line structure of DESIGN.md §14 at the end of each)"""
    rows, out, n = [], [], 0
    for t in texts:
        for e in F.entries_of(t):
            rows.append(_row(1, e, 0, len(e[1]), 0, len(e[3]))); out.append(_write(e)); n += 1
    return _finish(rows, [out], n, (-1, 8))
