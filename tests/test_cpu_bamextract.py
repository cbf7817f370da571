"""BamExtract without a device: the Python restatement (tests/bamextract_oracle.py) on the reference's fixture (src/tools-TEST/BamExtract_Test.cpp: its expected
output, fed back as input with its own ID list, must come out whole), the ID file's parsing rules, the new symbols, and what the library and the tool refuse
before a device is opened."""
import ctypes as C
import os
import subprocess

import pytest

import bamextract_oracle as X

ngsqc = __import__("importlib").import_module("ngs-bits_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = os.path.join(ROOT, "tests", "golden", "ref_in", "BamExtract", "BamExtract_ids.txt")   # (a folder of its own: the tools' fixture loops over ref_in stay as they were)
GO = os.path.join(ROOT, "tests", "golden", "ref_out")
OUT1 = os.path.join(GO, "BamExtract_out1.bam")
TOOL = os.path.join(ROOT, "ngs-bits_amd", "bin", "BamExtract")
NO_DEVICE = dict(os.environ, HIP_VISIBLE_DEVICES="-1")


def tool(*args, **kw):
    if not os.path.exists(TOOL):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ngs-bits_amd", "host"), "-s"])
    return subprocess.run([TOOL] + list(args), capture_output=True, text=True, timeout=120, **kw)


def test_restatement_on_the_reference_vector():
    ids = X.parse_ids(open(IDS, "rb").read())
    header, recs = X.read_bam(OUT1)
    out, out2, c = X.extract(recs, ids, True)
    assert c == dict(out=2260, out2=0, names=1117)
    assert out == recs and out2 == []   # every input record lands in out, byte for byte
    log = open(os.path.join(GO, "BamExtract_out1.log")).read().splitlines(True)
    assert X.log_text(c, True) == log[0] + log[1] + "Reads written to 'out2': 0\n"
    assert X.log_text(c, False) == log[0] + log[1]
    assert {X.name_of(b) for b in recs} == ids
    assert sum(1 for b in recs if X.Rec(b).flag & 0x900) == 26 and max(len(i) for i in ids) == 44


def test_parse_ids_rules():
    data = (b"a\r\n" b"  b \t\n" b"\tc d\t\r\n" b"#x\n" b"  #x\n" b"\n" b"   \r\n" b"a\n" b"c d\n" b"\v\fe\f\v\n" b"x#y\n" b"last")
    assert X.parse_ids(data) == {b"a", b"b", b"c d", b"e", b"x#y", b"last"}
    assert X.parse_ids(b"") == set() and X.parse_ids(b"\n\n# only a comment") == set()
    assert X.parse_ids(b"q\0r\n") == {b"q\0r"}   # (read as bytes: a NUL is no blank)


def test_name_ends_at_the_first_nul():
    rec = bytearray(40)
    rec[12] = 6
    assert X.name_of(bytes(rec[:36]) + b"ab\0cd\0") == b"ab"
    rec[12] = 1
    assert X.name_of(bytes(rec[:36]) + b"\0") == b""
    rec[12] = 0
    assert X.name_of(bytes(rec[:36])) == b""


def test_new_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ngsqc.h")).read()
    assert "ngsqc_extract_reads(" in hdr and "ngsqc_match_names(" in hdr and "ngsqc_extract_counts;" in hdr
    assert {"ngsqc_extract_reads", "ngsqc_match_names"} <= set(ngsqc.capi.EXPORTS)
    assert callable(ngsqc.Handle.extract) and callable(ngsqc.Handle.match_names)
    assert [f for f, _ in ngsqc.ExtractCounts._fields_] == list(ngsqc.EXTRACT_COUNT_NAMES) == ["out", "out2", "names"]


def test_argument_errors_come_before_the_device():
    L = ngsqc.lib()
    cnt = ngsqc.ExtractCounts()
    lens = (C.c_int32 * 1)(1)
    out = (C.c_uint8 * 4)()
    E_ARG = -3
    fake = C.c_void_p(8)   # (never dereferenced: every call below is refused on its arguments alone)
    assert L.ngsqc_extract_reads(None, b"a", lens, 1, b"o.bam", None, C.byref(cnt)) == E_ARG
    assert L.ngsqc_extract_reads(fake, b"a", lens, 1, None, None, C.byref(cnt)) == E_ARG
    assert L.ngsqc_extract_reads(fake, b"a", lens, 1, b"o.bam", None, None) == E_ARG
    assert L.ngsqc_extract_reads(fake, None, lens, 1, b"o.bam", None, C.byref(cnt)) == E_ARG
    assert L.ngsqc_extract_reads(fake, b"a", None, 1, b"o.bam", None, C.byref(cnt)) == E_ARG
    assert L.ngsqc_extract_reads(fake, b"a", lens, -1, b"o.bam", None, C.byref(cnt)) == E_ARG
    assert L.ngsqc_match_names(None, b"a", lens, 1, out, 4) == E_ARG
    assert L.ngsqc_match_names(fake, None, lens, 1, out, 4) == E_ARG
    assert L.ngsqc_match_names(fake, b"a", lens, -1, out, 4) == E_ARG
    assert L.ngsqc_match_names(fake, b"a", lens, 1, None, 4) == E_ARG
    assert L.ngsqc_match_names(fake, b"a", lens, 1, out, -1) == E_ARG
    assert not os.path.exists("o.bam")


@pytest.mark.parametrize("out,out2,msg", [("x.cram", None, "CRAM output is not supported"), ("x.txt", None, "File extension has to be '.bam' or '.cram'."),
                                          ("x.bam", "y.cram", "CRAM output is not supported"), ("x.bam", "y.txt", "File extension has to be '.bam' or '.cram'.")])
def test_tool_refuses_outputs_before_the_device(tmp_path, out, out2, msg):
    args = ["-in", OUT1, "-ids", IDS, "-out", str(tmp_path / out)] + (["-out2", str(tmp_path / out2)] if out2 else [])
    r = tool(*args, env=NO_DEVICE)
    assert r.returncode == 1 and msg in r.stderr and "no CPU fallback" not in r.stderr
    assert "Read IDs" not in r.stdout
    assert os.listdir(tmp_path) == []


def test_tool_without_a_device_prints_the_id_count_and_fails(tmp_path):
    ids = tmp_path / "ids.txt"
    ids.write_bytes(b"a\r\n  b \n#c\n\na\nlast")
    r = tool("-in", OUT1, "-ids", str(ids), "-out", str(tmp_path / "o.bam"), "-out2", str(tmp_path / "o2.bam"), env=NO_DEVICE)
    assert r.returncode == 1 and r.stdout == "Read IDs: 3\n" and "no CPU fallback" in r.stderr, (r.stdout, r.stderr)
    r = tool("-in", OUT1, "-ids", IDS, "-out", str(tmp_path / "o.bam"), env=NO_DEVICE)
    assert r.returncode == 1 and r.stdout == "Read IDs: 1117\n" and "no CPU fallback" in r.stderr


def test_tool_missing_id_file(tmp_path):
    """the tool layer checks an input file when it parses the command line, as the reference's ToolBase does for addInfile: the ID file is never opened"""
    missing = str(tmp_path / "nope.txt")
    r = tool("-in", OUT1, "-ids", missing, "-out", str(tmp_path / "o.bam"), env=NO_DEVICE)
    assert r.returncode == 1 and "Input file '" + missing + "' given for parameter 'ids' does not exist." in r.stderr
    assert r.stdout == "" and os.listdir(tmp_path) == []


def test_tool_unreadable_id_file(tmp_path):
    """a path that exists and cannot be read as a file (a directory: QFile::open fails on it) passes the command line's check and gets the host layer's message
    for a file that does not open, before "Read IDs" and before a device"""
    d = tmp_path / "ids.d"
    d.mkdir()
    r = tool("-in", OUT1, "-ids", str(d), "-out", str(tmp_path / "o.bam"), env=NO_DEVICE)
    assert r.returncode == 1 and "Could not open file for reading: '" + str(d) + "'!" in r.stderr and "no CPU fallback" not in r.stderr, (r.stdout, r.stderr)
    assert r.stdout == "" and os.listdir(tmp_path) == ["ids.d"]


def test_tool_help_and_changelog():
    r = tool("--help")
    assert r.returncode == 0 and "Extract reads from BAM/CRAM by read name." in r.stdout
    for flag, text in (("-in", "Input BAM/CRAM file."), ("-ids", "Input text file containing read names (one per line)."), ("-out", "Output BAM/CRAM file with matching reads."),
                       ("-out2", "Output BAM/CRAM file with not matching reads."), ("-ref", "Reference genome for CRAM support (mandatory if CRAM is used).")):
        assert f"  {flag}" in r.stdout and text in r.stdout, flag
    r = tool("--changelog")
    assert r.returncode == 0 and "2023-11-30" in r.stdout and "Initial implementation." in r.stdout
