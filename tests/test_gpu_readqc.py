"""The ReadQC tool (ngs-bits_amd/host/ReadQC.cpp over ngsqc_fastq_*) on the reference's seven test methods (src/tools-TEST/ReadQC_Test.cpp): outputs compared with the
expected files after the reference's own REMOVE_LINES; the merged FASTQ outputs gunzip to the inputs' text; the tool's error messages; and one of this project's
own BamToFastq outputs read back."""
import gzip
import os
import re
import subprocess
from decimal import Decimal, InvalidOperation

import pytest

import fastq_cases as K
import fastq_model as M
from conftest import GOLDEN_IN as BAM_IN, ROOT

pytestmark = pytest.mark.gpu
GI = os.path.join(ROOT, "tests", "golden", "ref_in", "ReadQC")
GO = os.path.join(ROOT, "tests", "golden", "ref_out", "ReadQC")
BIN = os.path.join(ROOT, "ngs-bits_amd", "bin")
STRIP = re.compile(r"creation |<binary>")


def fq(k):
    return os.path.join(GI, "ReadQC_in%d.fastq.gz" % k)


def tool(name, *args):
    return subprocess.run([os.path.join(BIN, name)] + list(args), capture_output=True, text=True, timeout=300)


def run(*args):
    p = tool("ReadQC", *args)
    assert p.returncode == 0, p.stderr
    return p


def _lines(path):
    return [ln for ln in open(path, encoding="latin-1").read().splitlines() if not STRIP.search(ln)]


@pytest.mark.parametrize("args,expected", [
    (["-in1", fq(1), "-in2", fq(2)], "ReadQC_out1.qcML"),                                    # base_test
    (["-in1", fq(1), "-in2", fq(2), "-txt"], "ReadQC_out2.txt"),                             # with_txt_parameter
    (["-in1", fq(1)], "ReadQC_out3.qcML"),                                                   # single_end
    (["-in1", fq(1), fq(3), "-in2", fq(2), fq(4)], "ReadQC_out5.qcML"),                      # multiple_input_files
    (["-in1", fq(5), "-long_read"], "ReadQC_out7.qcML"),                                     # long_read_test
])
def test_readqc_matches_reference_expected_output(tmp_path, args, expected):
    out = str(tmp_path / expected)
    run(*args, "-out", out)
    got, exp = _lines(out), _lines(os.path.join(GO, expected))
    assert got == exp, [(g, e) for g, e in zip(got, exp) if g != e][:5]


def same_within(a, b, delta):
    """COMPARE_FILES_DELTA(..., delta, false, '"'): the lines split at the quote; parts that are numbers may differ by delta (absolute, on the printed decimals)"""
    pa, pb = a.split('"'), b.split('"')
    if len(pa) != len(pb):
        return False
    for x, y in zip(pa, pb):
        if x == y:
            continue
        try:
            if abs(Decimal(x) - Decimal(y)) > Decimal(delta):
                return False
        except InvalidOperation:
            return False
    return True


def test_different_read_lengths(tmp_path):
    """compared as the reference compares it: 125 000 bases are the tie 0.125 MB, printed 0.13 by the reference (ReadQC_Test.cpp:36 allows 0.01)"""
    out = str(tmp_path / "ReadQC_out4.qcML")
    run("-in1", fq(3), "-in2", fq(4), "-out", out)
    got, exp = _lines(out), _lines(os.path.join(GO, "ReadQC_out4.qcML"))
    assert len(got) == len(exp)
    bad = [(g, e) for g, e in zip(got, exp) if not same_within(g, e, "0.01")]
    assert not bad, bad[:5]
    assert sum(g != e for g, e in zip(got, exp)) <= 1


def test_with_fastq_output(tmp_path):
    """-out1 / -out2: the decompressed text is the input's (the reference compares the gunzipped files), merged over the input files; in3 / in4 end without a newline"""
    o1, o2 = str(tmp_path / "R1.fastq.gz"), str(tmp_path / "R2.fastq.gz")
    run("-in1", fq(1), "-in2", fq(2), "-out1", o1, "-out2", o2, "-out", str(tmp_path / "o.qcML"))
    assert gzip.open(o1).read() == gzip.open(fq(1)).read() and gzip.open(o2).read() == gzip.open(fq(2)).read()
    raw = open(o1, "rb").read()
    assert raw[3] & 4 and raw[12:14] == b"BC" and raw.endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))   # BGZF with its EOF member
    run("-in1", fq(3), fq(1), "-in2", fq(4), fq(2), "-out1", o1, "-out2", o2, "-out", str(tmp_path / "o.qcML"), "-compression_level", "9")
    assert gzip.open(o1).read() == gzip.open(fq(3)).read() + b"\n" + gzip.open(fq(1)).read()
    assert gzip.open(o2).read() == gzip.open(fq(4)).read() + b"\n" + gzip.open(fq(2)).read()
    # the tool's values are those of the same run without the outputs
    a, b = str(tmp_path / "a.txt"), str(tmp_path / "b.txt")
    run("-in1", fq(3), "-in2", fq(4), "-out", a, "-txt", "-out1", o1)
    run("-in1", fq(3), "-in2", fq(4), "-out", b, "-txt")
    assert open(a).read() == open(b).read() and gzip.open(o1).read() == gzip.open(fq(3)).read() + b"\n"


def test_designed_text_through_the_tool(tmp_path):
    """CRLF, blank lines at the end, entries without a header: the tool's TXT values are the model's, and -out1 holds the entries as the reference writes them"""
    text = K.designed(True)
    for name, v in K.variants(text).items():
        p = tmp_path / (name + ".fastq.gz")
        p.write_bytes(gzip.compress(v, 1))
        out, o1 = str(tmp_path / (name + ".txt")), str(tmp_path / (name + ".out.fastq.gz"))
        run("-in1", str(p), "-long_read", "-txt", "-out", out, "-out1", o1)
        st, _, err = M.run([(v, False)], True)
        assert err is None and open(out).read() == "".join("%s: %s\n" % nv for nv in M.qc_values(st, True)), name
        assert gzip.open(o1).read() == M.text_of(M.entries_of(v)) == text, name


def test_error_messages(tmp_path):
    p = tool("ReadQC", "-in1", fq(1), fq(3), "-in2", fq(2))
    assert p.returncode != 0 and "Input file lists 'in1' and 'in2' differ in counts!" in p.stderr
    p = tool("ReadQC", "-in1", fq(1), "-in2", fq(4))
    assert p.returncode != 0 and "Differing number of reads in file '%s' and '%s'!" % (fq(1), fq(4)) in p.stderr
    # validation: the reference's message, offending character included; the first error is in1's although in2 fails earlier in its file
    cases = {c[0]: c for c in K.error_cases()}
    a, b = tmp_path / "a.fastq.gz", tmp_path / "b.fastq"
    a.write_bytes(gzip.compress(cases["kind5-above"][1]))
    b.write_bytes(cases["first-entry"][1])
    p = tool("ReadQC", "-in1", str(a), "-in2", str(b))
    assert p.returncode != 0 and "Invalid Fastq file entry: Invalid quality character 'K' with value '75' encountered in sequence '@e7'." in p.stderr, p.stderr
    p = tool("ReadQC", "-in1", str(b), "-in2", str(a))
    assert p.returncode != 0 and "First header line does not start with '@': 'Ae0'." in p.stderr
    p = tool("ReadQC", "-in1", str(a), "-long_read")      # 'K' (42) is a nanopore quality
    assert p.returncode == 0, p.stderr
    p = tool("ReadQC", "-in1", str(tmp_path / "missing.fastq.gz"))
    assert p.returncode != 0 and "missing.fastq.gz' given for parameter 'in1' does not exist." in p.stderr


def test_bamtofastq_output_is_read_back(tmp_path):
    """BamToFastq writes FASTQ.GZ (BGZF) here; ReadQC reads it: its values are the model's on the decompressed text"""
    o1, o2 = str(tmp_path / "r1.fastq.gz"), str(tmp_path / "r2.fastq.gz")
    p = tool("BamToFastq", "-in", os.path.join(BAM_IN, "BamToFastq", "BamToFastq_in1.bam"), "-out1", o1, "-out2", o2)
    assert p.returncode == 0, p.stderr
    out = str(tmp_path / "qc.txt")
    run("-in1", o1, "-in2", o2, "-txt", "-out", out)
    st, index, err = M.run([(gzip.open(o1).read(), False), (gzip.open(o2).read(), True)])
    assert err is None and index[0] == index[1] > 0
    assert open(out).read() == "".join("%s: %s\n" % nv for nv in M.qc_values(st, False))
