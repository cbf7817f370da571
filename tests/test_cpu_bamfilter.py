"""BamFilter without a device: the Python restatement (tests/bamfilter_oracle.py) against the reference's expected BAMs (src/tools-TEST/BamFilter_Test.cpp), and
the tool's argument errors, which come before a device is opened."""
import os
import subprocess

import pytest

import bamfilter_oracle as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GI = os.path.join(ROOT, "tests", "golden", "ref_in", "BamFilter")   # (a folder of their own: the tools' fixture loops over ref_in stay as they were)
GO = os.path.join(ROOT, "tests", "golden", "ref_out")
TOOL = os.path.join(ROOT, "ngs-bits_amd", "bin", "BamFilter")

CASES = [   # BamFilter_Test.cpp: no_filtering, mq_filter, max_mq_filter
    ("BamFilter_in1.bam", {}, "BamFilter_out1.bam"),
    ("BamFilter_in2.bam", {"min_mq": 50}, "BamFilter_out2.bam"),
    ("BamFilter_in2.bam", {"max_mq": 50}, "BamFilter_out3.bam"),
]


@pytest.mark.parametrize("inp,kw,exp", CASES)
def test_restatement_reproduces_reference_outputs(inp, kw, exp):
    header, out, passed, dropped = F.filter_file(os.path.join(GI, inp), **kw)
    eh, erecs = F.read_bam(os.path.join(GO, exp))
    assert header == eh
    assert out == erecs
    assert passed == len(erecs) // 2


def test_pairing_rules():
    import struct

    def rec(name, flag, mapq=60):
        n = name.encode() + b"\0"
        body = struct.pack("<iiBBHHHiiii", 0, 100, len(n), mapq, 4680, 1, flag, 1, 0, 200, 150) + n + struct.pack("<I", 1 << 4) + b"\x10" + b"\x1e"
        return struct.pack("<I", len(body)) + body
    recs = [rec("a", 1), rec("b", 1), rec("a", 1 | 0x100), rec("a", 1), rec("a", 1 | 0x800), rec("a", 1), rec("c", 1), rec("a", 1), rec("a", 1 | 4), rec("a", 1)]
    out, passed, dropped = F.filter_pairs(recs)
    # the non-skipped a records pair (0,3), (5,7), (8,9); the last pair holds an unmapped record; b and c stay open
    assert passed == 2 and dropped == 1
    assert out == [recs[0], recs[3], recs[5], recs[7]]


@pytest.mark.parametrize("out,msg", [("x.sam", "File extension has to be '.bam' or '.cram'."), ("x.cram", "CRAM output is not supported")])
def test_tool_argument_errors(tmp_path, out, msg):
    if not os.path.exists(TOOL):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ngs-bits_amd", "host"), "-s"])
    r = subprocess.run([TOOL, "-in", os.path.join(GI, "BamFilter_in1.bam"), "-out", str(tmp_path / out)], capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode != 0
    assert msg in r.stdout + r.stderr
    assert not (tmp_path / out).exists()
