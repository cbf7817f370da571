"""The device's visit of a record to its variant lines (ngs-bits_amd/csrc/rmvar_visit.h - the text the GPU library compiles into the verdict and gather kernels
of BamRemoveVariants) on the CPU, against the Python restatement: the verdict byte of every record and, under -mask, the bytes of its sequence, on the designed
BAM (tests/rmvar_cases.py) and on the reference's fixture with lines picked from its own reads. Plain integer code: held here without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import bamremovevariants_oracle as R
import emul_build
import rmvar_cases as K
from conftest import ROOT

ngsqc = __import__("importlib").import_module("ngs-bits_amd")
IN1 = os.path.join(ROOT, "tests", "golden", "ref_in", "BamRemoveVariants", "BamRemoveVariants_in1.bam")


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(emul_build.library("rmvar_emul.cpp"))
    L.rmvar_emul.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def emulate(L, recs, lines, refs, mask, keep):
    rows, maxend, _ = K.device_layout(R.table(lines, refs))
    arr, n = ngsqc.capi._variants_buffer(rows)
    tid_first = np.zeros(len(refs) + 1, np.int32)
    for t in range(len(refs) + 1):
        tid_first[t] = sum(1 for r in rows if r[0] < t)
    me = np.array(maxend + [0], np.int32)
    infl = np.frombuffer(b"".join(recs) + bytes(64), np.uint8)
    off = np.cumsum([0] + [len(b) for b in recs[:-1]]).astype(np.int64)
    vd, ev, patched = np.zeros(len(recs), np.uint8), np.zeros(len(recs), np.int32), np.zeros(len(infl), np.uint8)
    L.rmvar_emul(infl.ctypes.data, off.ctypes.data, len(recs), C.addressof(arr), me.ctypes.data, tid_first.ctypes.data, len(refs), mask, keep, vd.ctypes.data, ev.ctypes.data, patched.ctypes.data)
    out = [patched[o:o + len(b)].tobytes() for o, b in zip(off, recs)]
    return bytes(vd & 15), out


def check(L, recs, lines, refs):
    """-> the restatement's verdict bytes per mode"""
    tids, seen = R.line_tids(lines, refs), {}
    for mask, keep in ((0, 0), (1, 0), (1, 1)):
        vd, out = emulate(L, recs, lines, refs, mask, keep)
        exp = bytearray()
        for k, b in enumerate(recs):
            a = R.Aln(b)
            if a.r.flag & 0x900:
                exp.append(4); assert out[k] == b; continue
            try:
                ok = R.visit(a, lines, tids, mask, keep)
            except R.RmError:
                exp.append(8); assert out[k] == b; continue
            exp.append((1 if ok else 0) | (2 if a.seq != a.seq0 else 0))
            assert out[k] == a.bytes(), (mask, keep, k, a.r.name)
        assert vd == bytes(exp), (mask, keep)
        seen[(mask, keep)] = bytes(exp)
    return seen


def test_designed_records(lib):
    recs, raw = K.designed()
    check(lib, recs, R.parse_vcf(K.vcf_text(raw)), [n for n, _ in K.REFS])


def test_fixture_records_with_picked_lines(lib):
    header, recs = R.read_bam(IN1)
    refs = R.ref_names_of(header)
    raw = K.picked_lines(recs, refs)
    assert sum(1 for ln in raw if len(ln[2]) == 1 and len(ln[3]) == 1) >= 30 and sum(1 for ln in raw if len(ln[2]) != len(ln[3])) >= 4
    lines = R.parse_vcf(K.vcf_text(raw))
    recs = recs[::5]   # (an amplicon panel: every locus keeps hundreds of reads; the restatement is slow)
    vd = check(lib, recs, lines, refs)[(1, 0)]
    assert sum(1 for v in vd if v & 2) >= 30 and sum(1 for v in vd if not v & 1) >= 4   # the picked lines ARE carried


def test_errors(lib):
    refs = ["chr1"]
    rec = [K.record("e", 0x41, 0, 1000, "40M", K.seq_with(40, {39: "G", 7: "M"}))]
    for text, mask, code in (("chr1\t1040\t.\tAT\tAG\t.\t.\t.\n", 0, R.ERR_POS_NOT_FOUND), ("chr1\t1010\t.\ta\tc\t.\t.\t.\n", 0, R.ERR_INVALID_LINE),
                             ("chr1\t1040\t.\tA\tG\t.\t.\t.\n", 1, R.ERR_BAD_BASE)):
        lines = R.parse_vcf(text)
        assert emulate(lib, rec, lines, refs, mask, 0)[0] == bytes([8]) == R.verdicts(rec, lines, refs, mask, 0)
        with pytest.raises(R.RmError) as e:
            R.run(rec, lines, refs, mask=bool(mask))
        assert e.value.code == code and e.value.record == 0
    # the same lines where no visit reaches them: behind a carried line (default mode), or away from every read
    lines = R.parse_vcf("chr1\t1001\t.\tA\tA\t.\t.\t.\nchr1\t1010\t.\ta\tc\t.\t.\t.\nchr1\t5000\t.\tA\tC,G\t.\t.\t.\n")
    assert emulate(lib, rec, lines, refs, 0, 0)[0] == bytes([0]) == R.verdicts(rec, lines, refs, 0, 0)
