"""The Python model of SeqPurge (tests/seqpurge_oracle.py) against the reference's own expected outputs: the ten test methods of src/tools-TEST/SeqPurge_Test.cpp
with their arguments, every output file, every entry - the singleton files of test_07 and the error correction of test_10 included. What the model is then used
for (the CPU emulator of csrc/purge_visit.h, the GPU library) rests on this."""
import gzip
import os

import pytest

import seqpurge_oracle as M
from conftest import ROOT

GI = os.path.join(ROOT, "tests", "golden", "ref_in", "SeqPurge")
GO = os.path.join(ROOT, "tests", "golden", "ref_out", "SeqPurge")
NEXTERA = b"CTGTCTCTTATACACATCT"
# name: (in1, in2, out1, out2, out3 prefix or None, parameters) - SeqPurge_Test.cpp:100-208
REF_TESTS = {
    "test_01": (1, 2, 1, 2, None, dict(ncut=0, qcut=0, min_len=15)),
    "test_02": (3, 4, 3, 4, None, dict(ncut=0, qcut=0, min_len=15)),
    "test_03": (5, 6, 5, 6, None, dict(ncut=0, qcut=0, min_len=15)),
    "test_04": (7, 8, 7, 8, None, dict(a1=NEXTERA, a2=NEXTERA, ncut=0, qcut=0, min_len=15)),
    "test_05": (1, 2, 9, 10, None, dict(qcut=15, ncut=0, min_len=15)),
    "test_06": (1, 2, 11, 12, None, dict(ncut=7, qcut=0, min_len=15)),
    "test_07": (1, 2, 13, 14, 15, dict(qcut=25)),
    "test_08": (9, 10, 16, 17, None, dict(min_len=15)),
    "test_09": (11, 12, 18, 19, None, dict(min_len=15)),
    "test_10": (1, 2, 20, 21, None, dict(ncut=0, qcut=0, ec=True, min_len=15)),
}
_runs = {}


def read_in(i):
    with gzip.open(os.path.join(GI, "SeqPurge_in%d.fastq.gz" % i), "rb") as f:
        return f.read()


def read_out(name):
    with gzip.open(os.path.join(GO, "SeqPurge_out%s.fastq.gz" % name), "rb") as f:
        return f.read()


def ref_run(name):
    """the model's run of a reference test method, computed once"""
    if name not in _runs:
        in1, in2, _, _, out3, kw = REF_TESTS[name]
        _runs[name] = M.run(read_in(in1), read_in(in2), M.Params(out3=out3 is not None, **kw))
    return _runs[name]


def expected_outputs(name):
    _, _, o1, o2, o3, _ = REF_TESTS[name]
    exp = [read_out(str(o1)), read_out(str(o2))]
    if o3 is not None:
        exp += [read_out("%d_R1" % o3), read_out("%d_R2" % o3)]
    return exp


@pytest.mark.parametrize("name", sorted(REF_TESTS))
def test_model_reproduces_reference_outputs(name):
    r = ref_run(name)
    assert r.error is None, r.error
    exp = expected_outputs(name)
    for k, e in enumerate(exp):
        got_entries, exp_entries = M.parse_fastq(r.out[k]), M.parse_fastq(e)
        assert len(got_entries) == len(exp_entries), (name, k)
        for i, (g, x) in enumerate(zip(got_entries, exp_entries)):
            assert g == x, (name, k, i)
        assert r.out[k] == e, (name, k)
    if len(exp) == 2:
        assert r.out[2] == b"" and r.out[3] == b""


def test_literal_loop_and_whole_counts_agree_on_reference_input():
    """the model's two ways of counting an offset - the reference's loop with its early exit, and whole counts with the mismatch budget - give the same plan"""
    t1, t2 = read_in(11), read_in(12)
    P = M.Params(min_len=15)
    a, b = M.run(t1, t2, P, literal=True), M.run(t1, t2, P, literal=False)
    assert a.error is None and b.error is None
    assert (a.plan == b.plan).all() and a.out == b.out


def test_margin_record():
    """Record, not a gate: how near any probability compared with mep came to mep on the reference's inputs (DESIGN.md quotes the value). The only thing
    asserted is that no decision sat on mep itself."""
    worst = min(ref_run(n).margin.value for n in sorted(REF_TESTS))
    print("smallest |p - mep| / mep over the reference inputs: %.6g" % worst)
    assert worst > 0.0


def test_catalogue_premises_hold():
    """every designed pair (tests/purge_cases.py) produces, in the model with the reference's literal loop, the plan columns it was built for; every designed
    error stops the run at its pair with its kind and message"""
    import purge_cases as K
    n = 0
    for g in K.catalogue():
        t1, t2 = g.texts()
        r = M.run(t1, t2, g.params(), literal=True)
        assert r.error is None, (g.name, r.error)
        assert len(r.plan) == len(g.cases)
        for c, row in zip(g.cases, r.plan):
            n += 1
            for k, v in c.premise.items():
                assert int(row[K.COL[k]]) == v, (g.name, c.name, k, v, row.tolist())
    assert n >= 200
    for name, t1, t2, kind, pair, msg in K.error_cases():
        e = M.run(t1, t2, M.Params()).error
        assert e is not None and (e.kind, e.pair) == (kind, pair) and e.message.startswith(msg), (name, e)


def test_unequal_entry_counts():
    import purge_cases as K
    g = K.catalogue()[1]
    t1, t2 = g.texts()
    cut = t2[:t2.rindex(b"@")]
    e = M.run(t1, cut, g.params(), name1="a.fastq.gz", name2="b.fastq.gz").error
    assert e.message == "File a.fastq.gz has more entries than b.fastq.gz!" and e.pair == len(g.cases) - 1
    e = M.run(cut, t1, g.params(), name1="a.fastq.gz", name2="b.fastq.gz").error
    assert e.message == "File b.fastq.gz has more entries than a.fastq.gz!"
