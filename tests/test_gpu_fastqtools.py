"""The four per-entry FASTQ tools (ngs-bits_amd/host/Fastq{Trim,Extract,ExtractUMI,Convert}.cpp over ngsqc_fqedit_*) on the reference's 13 test methods
(src/tools-TEST/Fastq*_Test.cpp) with the reference's arguments: every output's decompressed text equals the expected file's. And the tools' messages: an invalid
-compression_level, a length column that is no integer, and FastqExtract's validation."""
import gzip
import os
import subprocess

import pytest

from conftest import ROOT
from test_cpu_fastqtools import GO, REF_TESTS, in_path, text_of

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "ngs-bits_amd", "bin")
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def tool(name, *args):
    return subprocess.run([os.path.join(BIN, name)] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def io_args(name, tmp_path):
    """the -in / -ids / -out arguments of a reference test method, and the output paths"""
    t, _, ins, ids, outs, _, _ = REF_TESTS[name]
    if len(ins) == 2:
        paths = [tmp_path / "o1.fastq.gz", tmp_path / "o2.fastq.gz"]
        return ["-in1", in_path(name, ins[0]), "-in2", in_path(name, ins[1]), "-out1", paths[0], "-out2", paths[1]], paths
    args = ["-in", in_path(name, ins[0])] + (["-ids", in_path(name, ids)] if ids else [])
    return args + ["-out", tmp_path / "o.fastq.gz"], [tmp_path / "o.fastq.gz"]


@pytest.mark.parametrize("name", sorted(REF_TESTS))
def test_reference_test_method(tmp_path, name):
    args, paths = io_args(name, tmp_path)
    p = tool(REF_TESTS[name][0], *args, *REF_TESTS[name][5])
    assert p.returncode == 0, p.stderr
    for path, exp in zip(paths, REF_TESTS[name][4]):
        assert gzip.open(path, "rb").read() == text_of(os.path.join(GO, REF_TESTS[name][0], exp)), (name, exp)
        assert open(path, "rb").read()[-28:] == EOF_MEMBER


@pytest.mark.parametrize("level", [0, 9])
def test_compression_levels_change_no_text(tmp_path, level):
    args, paths = io_args("trim_all", tmp_path)
    p = tool("FastqTrim", *args, *REF_TESTS["trim_all"][5], "-compression_level", level)
    assert p.returncode == 0, p.stderr
    assert gzip.open(paths[0], "rb").read() == text_of(os.path.join(GO, "FastqTrim", "FastqTrim_out5.fastq.gz"))


@pytest.mark.parametrize("name,level", [("trim_start", 10), ("extract_test_01", -1), ("convert_test_01", 10), ("umi_test_01", 11)])
def test_invalid_compression_level(tmp_path, name, level):
    args, paths = io_args(name, tmp_path)
    p = tool(REF_TESTS[name][0], *args, *REF_TESTS[name][5], "-compression_level", level)
    assert p.returncode != 0
    assert "ArgumentException: Invalid gzip compression level '%d' given for FASTQ file '%s'!" % (level, paths[0]) in p.stderr


def test_length_column_that_is_no_integer(tmp_path):
    (tmp_path / "ids.txt").write_bytes(b"#id\tlength\nNG-5232_4_1_1022_17823#0/1\t12\nother\tabc\n")
    p = tool("FastqExtract", "-in", in_path("extract_test_01", "FastqExtract_in1.fastq.gz"), "-ids", tmp_path / "ids.txt", "-out", tmp_path / "o.fastq.gz")
    assert p.returncode != 0 and "Could not convert length value 'abc' to integer" in p.stderr


def test_validation_message_of_fastqextract(tmp_path):
    (tmp_path / "ids.txt").write_bytes(b"a\n")
    (tmp_path / "in.fastq").write_bytes(b"@a\nACGT\n+\nIIII\n@b x\nACGU\n+\nIIII\n")
    p = tool("FastqExtract", "-in", tmp_path / "in.fastq", "-ids", tmp_path / "ids.txt", "-out", tmp_path / "o.fastq.gz")
    assert p.returncode != 0 and "Invalid Fastq file entry: Invalid base 'U' encountered in sequence '@b x'." in p.stderr
    (tmp_path / "in.fastq").write_bytes(b"@a\nACGT\n+\nIII~\n")
    p = tool("FastqExtract", "-in", tmp_path / "in.fastq", "-ids", tmp_path / "ids.txt", "-out", tmp_path / "o.fastq.gz")
    assert p.returncode != 0 and "Invalid quality character '~' with value '126' encountered in sequence '@a'." in p.stderr
    p = tool("FastqExtract", "-in", tmp_path / "in.fastq", "-ids", tmp_path / "ids.txt", "-out", tmp_path / "o.fastq.gz", "-long_read")
    assert p.returncode == 0 and gzip.open(tmp_path / "o.fastq.gz", "rb").read() == b"@a\nACGT\n+\nIII~\n"
