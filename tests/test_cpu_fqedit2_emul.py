"""The per-entry text of FastqExtractBarcode, FastqAddBarcode, FastqDownsample and FastqConcat (ngs-bits_amd/csrc/fqedit_visit.h - what the GPU library compiles
into the kernels of csrc/fqedit.hip) on the CPU, against the Python model (tests/fqedit2_oracle.py): the plan row for row, every output text and the text of
kept headers byte for byte on the designed cases (tests/fqedit2_cases.py) and on the reference's inputs, the same text as a stand-alone program under
AddressSanitizer and UBSan, and three mistakes built into the model that the designed cases must tell from it. The keep bytes handed to the emulator are
tests/bamdownsample_oracle.py's: the generator itself is device code and is held to the same stream on the GPU."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import bamdownsample_oracle as D
import emul_build
import fqedit2_cases as K2
import fqedit2_oracle as M2
from test_cpu_fastqtools2 import REF_TESTS2, inputs2, ref_run2
from test_cpu_seqpurge_emul import prepared


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(emul_build.library("fqedit2_emul.cpp"))
    L.fqedit2_emul.restype = C.c_int32
    L.fqedit2_emul.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.fqedit2_format.restype = C.c_int64
    L.fqedit2_format.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64]
    L.fqedit2_headers.restype = C.c_int64
    L.fqedit2_headers.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
    return L


def keep_bytes(case, first, n):
    """the decisions of the pair ordinals [first, first + n) of a downsample case"""
    return D.keep_stream(case.kw["seed"], case.kw["percentage"], first, n) if case.op == "downsample" else np.zeros(0, np.uint8)


def emulate(L, case):
    """every file of the case as one feed that ends a file, as the accumulator sees them: the plans and texts one behind the other"""
    op, streams = K2.OPS[case.op], K2.STREAMS[case.op]
    plans, texts, headers, sides, done = [], [b""] * streams, b"", np.zeros(3, np.int64), 0
    for f in case.files:
        t = [np.frombuffer(prepared(x, True), np.uint8).copy() for x in f]
        ptr = (C.c_void_p * 3)(*[x.ctypes.data for x in t]); ln = (C.c_int64 * 3)(*[len(x) for x in t])
        cap = max(len(x) for x in t) // 4 + 2
        plan, out = np.zeros((cap, streams, 8), np.int32), np.zeros(4, np.uint64)
        keep = np.ascontiguousarray(keep_bytes(case, done, cap))
        assert L.fqedit2_emul(ptr, ln, op, case.kw.get("cut1", 0), keep.ctypes.data, plan.ctypes.data, cap, out.ctypes.data) == 0
        n = int(out[0])
        buf = np.zeros(2 * sum(len(x) for x in t) + 128 * n + 64, np.uint8)
        for k in range(streams):
            got = L.fqedit2_format(ptr, ln, op, plan.ctypes.data, n, k, buf.ctypes.data, len(buf))
            assert got >= 0
            texts[k] += buf[:got].tobytes()
        if case.op == "downsample":
            got = L.fqedit2_headers(ptr, ln, op, plan.ctypes.data, n, buf.ctypes.data, len(buf))
            assert got >= 0
            headers += buf[:got].tobytes()
        plans.append(plan[:n]); done += n; sides += out[1:4].astype(np.int64)
    plan = np.concatenate(plans) if plans else np.zeros((0, streams, 8), np.int32)
    return dict(plan=plan if streams == 2 else plan[:, 0], out=texts, headers=headers, sides=sides[:K2.SIDES[case.op]].tolist())


def differs(got, r):
    """what of an emulator run is not the model's: a list of names, empty when they agree"""
    bad = []
    if got["plan"].shape != r.plan.shape or not np.array_equal(got["plan"], r.plan):
        bad.append("plan")
    if got["out"] != r.out:
        bad.append("out")
    if hasattr(r, "kept_headers") and (got["headers"] != r.kept_headers or got["sides"] != r.side_entries):
        bad.append("headers")
    return bad


@pytest.mark.parametrize("name", [c.name for c in K2.catalogue()])
def test_catalogue(lib, name):
    c = K2.by_name(name)
    assert differs(emulate(lib, c), c.model()) == []


@pytest.mark.parametrize("name", sorted(REF_TESTS2))
def test_reference_inputs(lib, name):
    tool, t = REF_TESTS2[name][0], inputs2(name)
    case = {"FastqExtractBarcode": lambda: K2.Case(name, "barcode_cut", dict(cut1=10), [(t[0],)]), "FastqAddBarcode": lambda: K2.Case(name, "barcode_add", {}, [tuple(t)]),
            "FastqDownsample": lambda: K2.Case(name, "downsample", dict(seed=1, percentage=20.0), [tuple(t)]), "FastqConcat": lambda: K2.Case(name, "copy", {}, [(x,) for x in t])}[tool]()
    assert differs(emulate(lib, case), ref_run2(name)) == []


@pytest.mark.parametrize("mutation", M2.MUTATIONS)
def test_a_mistake_in_the_model_is_told_apart(lib, mutation):
    """a designed case exists whose emulator run differs from the model with the mistake built in, while no case differs from the model itself
    (test_catalogue): the catalogue can see an index range off by one, an insertion one byte short from two digits on, and a keep bit of the next ordinal"""
    told = [c.name for c in K2.catalogue() if differs(emulate(lib, c), c.model(mutate=mutation))]
    assert told, mutation
    expect = {M2.MUTATIONS[0]: "cut-", M2.MUTATIONS[1]: "add-", M2.MUTATIONS[2]: "downsample-"}[mutation]
    assert all(n.startswith(expect) for n in told)
    if mutation == M2.MUTATIONS[1]:
        assert "add-digits" in told and "add-headers" not in told   # nine bases and fewer are not touched by it: the border decides


def test_stand_alone_under_sanitizers(tmp_path):
    """the same text as a program of its own, built with AddressSanitizer and UBSan, over every file of every case of the catalogue: the texts lie in heap
    buffers of exactly their size, and every output text and the kept headers in buffers of exactly the size the plan announces, so a read outside a line
    or a write behind an entry ends the run; its plan equals the model's"""
    exe = emul_build.program("fqedit2_emul_main.cpp", tmp_path, sanitize=True)
    for c in K2.catalogue():
        streams = K2.STREAMS[c.op]
        for f in c.files:   # (every file is a case of its own here: ordinals start at 0)
            one = K2.Case(c.name, c.op, c.kw, [f])
            r = one.model()
            paths = []
            for k, x in enumerate(f):
                paths.append(str(tmp_path / ("t%d" % k)))
                (tmp_path / ("t%d" % k)).write_bytes(prepared(x, True))
            keep = "-"
            if c.op == "downsample":
                keep = str(tmp_path / "keep")
                (tmp_path / "keep").write_bytes(keep_bytes(one, 0, r.stats["entries"] + 1).tobytes())
            p = subprocess.run([exe, str(K2.OPS[c.op]), str(c.kw.get("cut1", 0)), keep] + paths, capture_output=True, text=True)
            assert p.returncode == 0, (c.name, p.stderr[-2000:])
            lines = p.stdout.splitlines()
            rows = r.plan.reshape(-1, 8).tolist()
            assert [[int(v) for v in l.split()] for l in lines[:len(rows)]] == rows, c.name
            tail = ["stream %d: %d bytes" % (k, len(r.out[k])) for k in range(streams)] + (["headers: %d bytes" % len(r.kept_headers)] if c.op == "downsample" else [])
            assert lines[len(rows):] == tail, c.name
