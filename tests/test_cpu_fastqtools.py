"""The Python model of the per-entry FASTQ tools (tests/fqedit_oracle.py) against the reference's own expected outputs: the 13 test methods of
src/tools-TEST/FastqTrim_Test.cpp (6), FastqExtract_Test.cpp (4), FastqConvert_Test.cpp (1) and FastqExtractUMI_Test.cpp (2, two files each) with their
arguments, every output file byte for byte after decompression. What the model is then used for (the CPU emulator of csrc/fqedit_visit.h, the GPU library,
the four tools) rests on this. Also here: the rules of FastqExtract's id file."""
import gzip
import os

import pytest

import fqedit_oracle as M
from conftest import ROOT

GI = os.path.join(ROOT, "tests", "golden", "ref_in")
GO = os.path.join(ROOT, "tests", "golden", "ref_out")
# name: (tool, op, inputs, id file or None, expected outputs, the reference's arguments, the model's parameters)
REF_TESTS = {
    "trim_start": ("FastqTrim", "trim", ["FastqTrim_in1.fastq.gz"], None, ["FastqTrim_out1.fastq.gz"], ["-start", 5], dict(start=5)),
    "trim_start_end": ("FastqTrim", "trim", ["FastqTrim_in1.fastq.gz"], None, ["FastqTrim_out2.fastq.gz"], ["-start", 5, "-end", 5], dict(start=5, end=5)),
    "trim_start_len": ("FastqTrim", "trim", ["FastqTrim_in1.fastq.gz"], None, ["FastqTrim_out3.fastq.gz"], ["-start", 5, "-len", 50], dict(start=5, len=50)),
    "trim_max_len": ("FastqTrim", "trim", ["FastqTrim_in1.fastq.gz"], None, ["FastqTrim_out4.fastq.gz"], ["-end", 5, "-max_len", 80], dict(end=5, max_len=80)),
    "trim_all": ("FastqTrim", "trim", ["FastqTrim_in1.fastq.gz"], None, ["FastqTrim_out5.fastq.gz"], ["-len", 50, "-start", 5, "-end", 5, "-max_len", 80], dict(len=50, start=5, end=5, max_len=80)),
    "trim_long_read": ("FastqTrim", "trim", ["FastqTrim_in2.fastq.gz"], None, ["FastqTrim_out6.fastq.gz"], ["-long_read", "-len", 1000], dict(long_read=True, len=1000)),
    "extract_test_01": ("FastqExtract", "extract", ["FastqExtract_in1.fastq.gz"], "FastqExtract_in1.txt", ["FastqExtract_out1.fastq.gz"], [], dict()),
    "extract_test_02": ("FastqExtract", "extract", ["FastqExtract_in2.fastq.gz"], "FastqExtract_in2.txt", ["FastqExtract_out2.fastq.gz"], [], dict()),
    "extract_option_v": ("FastqExtract", "extract", ["FastqExtract_in1.fastq.gz"], "FastqExtract_in1.txt", ["FastqExtract_out3.fastq.gz"], ["-v"], dict(invert=True)),
    "extract_long_read": ("FastqExtract", "extract", ["FastqExtract_in3.fastq.gz"], "FastqExtract_in3.txt", ["FastqExtract_out4.fastq.gz"], ["-long_read"], dict(long_read=True)),
    "convert_test_01": ("FastqConvert", "convert", ["FastqConvert_in1.fastq.gz"], None, ["FastqConvert_out1.fastq.gz"], [], dict()),
    "umi_test_01": ("FastqExtractUMI", "umi", ["FastqExtractBarcode_in1.fastq.gz", "FastqExtractBarcode_in2.fastq.gz"], None, ["FastqExtractUMI_out1.fastq.gz", "FastqExtractUMI_out2.fastq.gz"],
                    ["-cut1", 12], dict(cut1=12)),
    "umi_test_02": ("FastqExtractUMI", "umi", ["FastqExtractBarcode_in1.fastq.gz", "FastqExtractBarcode_in2.fastq.gz"], None, ["FastqExtractUMI_out3.fastq.gz", "FastqExtractUMI_out4.fastq.gz"],
                    ["-cut1", 8, "-cut2", 8], dict(cut1=8, cut2=8)),
}
_runs = {}


def text_of(path):
    """gzip or plain text, as the reference's reader takes both"""
    raw = open(path, "rb").read()
    return gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw


def in_path(name, f):
    return os.path.join(GI, REF_TESTS[name][0], f)


def inputs(name):
    return [text_of(in_path(name, f)) for f in REF_TESTS[name][2]]


def ids_of(name):
    f = REF_TESTS[name][3]
    return None if f is None else M.parse_ids(open(in_path(name, f), "rb").read())


def expected(name):
    return [text_of(os.path.join(GO, REF_TESTS[name][0], f)) for f in REF_TESTS[name][4]]


def ref_run(name):
    """the model's run of a reference test method, computed once"""
    if name not in _runs:
        t = inputs(name)
        _runs[name] = M.run(REF_TESTS[name][1], t[0], t[1] if len(t) > 1 else None, ids=ids_of(name), **REF_TESTS[name][6])
    return _runs[name]


@pytest.mark.parametrize("name", sorted(REF_TESTS))
def test_model_reproduces_reference_outputs(name):
    r = ref_run(name)
    assert r.error is None
    exp = expected(name)
    assert len(r.out) == len(exp)
    for k, (got, want) in enumerate(zip(r.out, exp)):
        assert got == want, (name, k, len(got), len(want))
    assert r.stats["bytes"][:len(exp)] == [len(x) for x in exp]


def test_the_long_read_lengths_lie_beyond_the_reads():
    """FastqExtract_in3.txt lists lengths above its reads' (one above in six of seven lines), and FastqExtract_out4 holds the whole reads: a length beyond the
    read keeps the whole read - the reference's fixture decides this, not this project"""
    names, lengths = ids_of("extract_long_read")
    reads = {M.entry_id(e[0]): len(e[1]) for e in M.F.entries_of(inputs("extract_long_read")[0])}
    over = [lengths[k] - reads[n] for k, n in enumerate(names)]
    assert len(over) == 7 and all(d >= 1 for d in over) and sorted(over)[:6] == [1] * 6
    r = ref_run("extract_long_read")
    kept = r.plan[r.plan[:, 0] == 1]
    assert len(kept) == 7 and sorted(kept[:, 4].tolist()) == sorted(reads[n] for n in names)


def test_convert_fixture_turns_a_quality_into_a_line_feed_or_not():
    """quality ')' (41) - 31 is a line feed; whether the fixture holds one or not, the model writes what the arithmetic gives"""
    assert M.convert(b"@a\nAC\n+\n)h\n").out[0] == b"@a\nAC\n+\n\nI\n"


def test_id_file_rules():
    names, lengths = M.parse_ids(b"  a \n\n# comment\n#b\t3\nb\t 7 \nc\t-1\nd\t-2\na\t4\r\ne f\t+2\n\tg\t9\n")
    assert names == [b"a", b"b", b"c", b"d", b"a", b"e f", b"g"] and lengths == [-1, 7, -1, -2, 4, 2, 9]
    for bad in (b"x\tabc\n", b"x\t\t3\n", b"x\t1.5\n", b"x\t99999999999\n", b"x\t3 4\n"):
        with pytest.raises(ValueError) as e:
            M.parse_ids(bad)
        assert str(e.value).startswith("Could not convert length value '") and str(e.value).endswith("' to integer")
    # a later duplicate replaces the earlier one; -1 behaves as "no length", -2 as "not listed"; 0 and below -2 drop in both modes
    text = b"".join(b"@%s x\nACGTAC\n+\nIIIIII\n" % n for n in (b"a", b"b", b"c", b"d", b"z", b"n", b"m"))
    ids = ([b"a", b"b", b"c", b"d", b"a", b"n", b"m"], [-1, 7, -1, -2, 4, 0, -3])
    r = M.run("extract", text, ids=ids)
    assert r.plan[:, 0].tolist() == [1, 1, 1, 0, 0, 0, 0] and r.plan[:, 4].tolist() == [4, 6, 6, 6, 6, 6, 6]
    r = M.run("extract", text, ids=ids, invert=True)
    assert r.plan[:, 0].tolist() == [0, 0, 0, 1, 1, 0, 0]
