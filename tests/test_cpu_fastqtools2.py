"""The Python model of FastqExtractBarcode, FastqAddBarcode, FastqDownsample and FastqConcat (tests/fqedit2_oracle.py) against the reference's own expected
outputs: the seven test methods of src/tools-TEST/FastqExtractBarcode_Test.cpp (3), FastqAddBarcode_Test.cpp (1), FastqDownsample_Test.cpp (1) and
FastqConcat_Test.cpp (2) with their arguments, every output byte for byte after decompression. What the model is then used for (the CPU emulator of
csrc/fqedit_visit.h, the GPU library, the four tools) rests on this. The fixtures lie under tests/golden/<Tool>/."""
import os

import pytest

import fqedit2_oracle as M2
from conftest import ROOT
from test_cpu_fastqtools import text_of

GOLDEN = os.path.join(ROOT, "tests", "golden")
# name: (tool, inputs, expected outputs in the order of the model's streams, the reference's arguments in front of the files, does the expected text carry CR)
REF_TESTS2 = {
    "barcode_test_01": ("FastqExtractBarcode", ["FastqExtractBarcode_in1.fastq.gz"], ["FastqExtractBarcode_out2.fastq.gz", "FastqExtractBarcode_out1.fastq.gz"], ["-cut", "10"], False),
    "barcode_test_02": ("FastqExtractBarcode", ["FastqExtractBarcode_in2.fastq.gz"], ["FastqExtractBarcode_out4.fastq.gz", "FastqExtractBarcode_out3.fastq.gz"], ["-cut", "10"], False),
    "barcode_test_03": ("FastqExtractBarcode", ["FastqExtractBarcode_in2.fastq.gz"], ["FastqExtractBarcode_out4.fastq.gz", "FastqExtractBarcode_out3.fastq.gz"], ["-cut", "10"], False),
    "addbarcode_test_01": ("FastqAddBarcode", ["FastqExtractBarcode_in1.fastq.gz", "FastqExtractBarcode_in2.fastq.gz", "FastqAddBarcode_in.fastq.gz"],
                           ["FastqAddBarcode_out1.fastq.gz", "FastqAddBarcode_out2.fastq.gz"], [], False),
    "downsample_paired_end": ("FastqDownsample", ["FastqDownsample_in1.fastq.gz", "FastqDownsample_in2.fastq.gz"], ["FastqDownsample_out1_Linux.txt"], ["-percentage", "20", "-test"], False),
    "concat_default_test": ("FastqConcat", ["FastqConcat_in1.fastq.gz", "FastqConcat_in2.fastq.gz", "FastqConcat_in3.fastq.gz"], ["FastqConcat_out.fastq.gz"], [], True),
    "concat_long_test": ("FastqConcat", ["FastqConcat_in4.fastq.gz", "FastqConcat_in5.fastq.gz"], ["FastqConcat_out2.fastq.gz"], ["-long_read"], False),
}
_runs = {}


def golden(tool, f):
    """FastqAddBarcode reads the inputs of FastqExtractBarcode"""
    p = os.path.join(GOLDEN, tool, f)
    return p if os.path.exists(p) else os.path.join(GOLDEN, f.split("_")[0], f)


def inputs2(name):
    return [text_of(golden(REF_TESTS2[name][0], f)) for f in REF_TESTS2[name][1]]


def expected2(name):
    """the expected texts. FastqConcat_out.fastq.gz carries CRLF at the end of every line (its inputs were written on another system); this project drops
    CR from the end of a line and ends every line with a line feed, so that one file is compared after taking its CR out."""
    tool, _, outs, _, has_cr = REF_TESTS2[name]
    exp = [text_of(golden(tool, f)) for f in outs]
    return [x.replace(b"\r", b"") for x in exp] if has_cr else exp


def ref_run2(name):
    """the model's run of a reference test method, computed once"""
    if name not in _runs:
        tool, t = REF_TESTS2[name][0], inputs2(name)
        if tool == "FastqExtractBarcode":
            _runs[name] = M2.barcode_cut(t[0], cut=10)
        elif tool == "FastqAddBarcode":
            _runs[name] = M2.barcode_add([tuple(t)])
        elif tool == "FastqDownsample":
            _runs[name] = M2.downsample(t[0], t[1], seed=1, percentage=20.0)
        else:
            _runs[name] = M2.concat(t)
    return _runs[name]


@pytest.mark.parametrize("name", sorted(REF_TESTS2))
def test_model_reproduces_reference_outputs(name):
    r = ref_run2(name)
    exp = expected2(name)
    if REF_TESTS2[name][0] == "FastqDownsample":   # the test method compares the log, not the FASTQ files
        assert M2.downsample_log(r) == exp[0]
        assert r.stats["entries"] == 271 and r.stats["written"] == [51, 51] and r.side_entries == [271, 271]
        return
    assert len(r.out) == len(exp)
    for k, (got, want) in enumerate(zip(r.out, exp)):
        assert got == want, (name, k, len(got), len(want))
    assert r.stats["bytes"][:len(exp)] == [len(x) for x in exp]


def test_the_concat_fixture_really_carries_cr_and_the_others_do_not():
    """the premise of the one comparison that is not byte for byte"""
    raw = text_of(golden("FastqConcat", "FastqConcat_out.fastq.gz"))
    assert raw.count(b"\r\n") == raw.count(b"\n") > 0
    for name in REF_TESTS2:
        if not REF_TESTS2[name][4]:
            assert all(b"\r" not in text_of(golden(REF_TESTS2[name][0], f)) for f in REF_TESTS2[name][2])
    assert text_of(golden("FastqExtractBarcode", "FastqExtractBarcode_in2.fastq.gz"))[:1] == b"@"   # plain text under a .gz name: the readers take both


def test_the_barcode_text_is_five_bytes_the_digits_and_the_bases():
    r = M2.barcode_add([(b"@a 1\nAC\n+\nII\n", b"@a 2\nGT\n+\nII\n", b"@b\nACGTACGTAC\n+\nIIIIIIIIII\n")])
    assert r.out[0].split(b"\n")[0] == b"@a:10,0:ACGTACGTAC, 1" and r.plan[0, 0, 1:3].tolist() == [2, 5 + 2 + 10]
