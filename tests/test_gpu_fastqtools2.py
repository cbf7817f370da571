"""FastqExtractBarcode, FastqAddBarcode, FastqDownsample and FastqConcat (ngs-bits_amd/host/<tool>.cpp over ngsqc_fqedit_*) on the reference's seven test methods
(src/tools-TEST/Fastq{ExtractBarcode,AddBarcode,Downsample,Concat}_Test.cpp) with the reference's arguments: every output's decompressed text equals the
expected file's (FastqConcat's default_test after the CR of the expected text is taken out: tests/test_cpu_fastqtools2.py says why), FastqDownsample's STDOUT
equals the expected log. And the tools' messages, and their help texts, which restate the parameters of the reference's setup()."""
import gzip
import os
import subprocess

import pytest

import fqedit2_oracle as M2
from conftest import ROOT
from test_cpu_fastqtools2 import REF_TESTS2, expected2, golden, inputs2, ref_run2

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "ngs-bits_amd", "bin")
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
SPECIAL = """
Special parameters:
  --help	Shows this help and exits.
  --version	Prints version and exits.
  --changelog	Prints changeloge and exits.
  --tdx	Writes a Tool Definition Xml file. The file name is the application name with the suffix '.tdx'.
  --settings [file]	Settings override file (no other settings files are used).
"""
LEVEL = "  -compression_level <int>	Output FASTQ compression level from 1 (fastest) to 9 (best compression).\n		Default value: '1'\n"
# the help text behind the line with the tool's name and version: description, parameters, types, defaults and their order as in the reference's setup()
HELP = {
    "FastqExtractBarcode": """
Cuts bases from the beginning of reads and stores them in an additional fastq.

Mandatory parameters:
  -in <infile>	input fastq file1.
  -out_main <string>	output filename for main fastq.

Optional parameters:
  -out_index <string>	output filename for index fastq.
		Default value: 'index.fastq.gz'
  -cut <int>	number of bases from the beginning of reads to use as barcodes.
		Default value: '0'
""" + LEVEL + SPECIAL,
    "FastqAddBarcode": """
Adds barcodes from separate FASTQ file to read headers.

Mandatory parameters:
  -in1 <infilelist>	Input FASTQ file 1.
  -in2 <infilelist>	Input FASTQ file 2.
  -in_barcode <infilelist>	Input barcode file.
  -out1 <outfile>	Output filename for read 1 FASTQ.
  -out2 <outfile>	Output filename for read 2 FASTQ.

Optional parameters:
""" + LEVEL + SPECIAL,
    "FastqDownsample": """
Downsamples paired-end FASTQ files.

Mandatory parameters:
  -in1 <infile>	Forward input gzipped FASTQ file(s).
  -in2 <infile>	Reverse input gzipped FASTQ file(s).
  -percentage <float>	Percentage of reads to keep.
  -out1 <outfile>	Forward output gzipped FASTQ file.
  -out2 <outfile>	Reverse output gzipped FASTQ file.

Optional parameters:
  -test	Test mode: fix random number generator seed and write kept read names to STDOUT.
		Default value: 'false'
""" + LEVEL + SPECIAL,
    "FastqConcat": """
Concatinates several FASTQ files into one output FASTQ file.

Mandatory parameters:
  -in <infilelist>	Input (gzipped) FASTQ files.
  -out <outfile>	Output gzipped FASTQ file.

Optional parameters:
""" + LEVEL + """  -long_read	Support long reads (> 1kb).
		Default value: 'false'
""" + SPECIAL,
}


def tool(name, *args):
    return subprocess.run([os.path.join(BIN, name)] + [str(a) for a in args], capture_output=True, timeout=300)


def io_args(name, tmp_path):
    """the input and output arguments of a reference test method, and the output paths in the order of the expected files"""
    t, ins, _, _, _ = REF_TESTS2[name]
    p = [golden(t, f) for f in ins]
    o = [tmp_path / "o1.fastq.gz", tmp_path / "o2.fastq.gz"]
    if t == "FastqExtractBarcode":
        return ["-in", p[0], "-out_main", o[0], "-out_index", o[1]], o
    if t == "FastqAddBarcode":
        return ["-in1", p[0], "-in2", p[1], "-in_barcode", p[2], "-out1", o[0], "-out2", o[1]], o
    if t == "FastqDownsample":
        return ["-in1", p[0], "-in2", p[1], "-out1", o[0], "-out2", o[1]], o
    return ["-in"] + p + ["-out", o[0]], o[:1]


def is_bgzf(path):
    raw = open(path, "rb").read()
    return raw[:2] == b"\x1f\x8b" and raw[-28:] == EOF_MEMBER


@pytest.mark.parametrize("name", sorted(REF_TESTS2))
def test_reference_test_method(tmp_path, name):
    args, paths = io_args(name, tmp_path)
    p = tool(REF_TESTS2[name][0], *args, *REF_TESTS2[name][3])
    assert p.returncode == 0, p.stderr
    r, exp = ref_run2(name), expected2(name)
    if REF_TESTS2[name][0] == "FastqDownsample":
        assert p.stdout == exp[0]                                             # the reference compares the log ...
        assert [gzip.open(q, "rb").read() for q in paths] == r.out            # ... and the files hold the pairs the log names
    else:
        assert [gzip.open(q, "rb").read() for q in paths] == exp
    assert all(is_bgzf(q) for q in paths)


def test_downsample_with_one_file_longer(tmp_path):
    t1, t2 = inputs2("downsample_paired_end")
    cut = t2.index(b"\n@", len(t2) // 2) + 1
    (tmp_path / "a.fastq").write_bytes(t1); (tmp_path / "b.fastq").write_bytes(t2[:cut])
    n = len(M2.F.entries_of(t2[:cut]))
    assert 0 < n < 271
    for first, second, msg in (("a", "b", "File %s has more entries than %s!" % (tmp_path / "a.fastq", tmp_path / "b.fastq")), ("b", "a", "File %s has more entries than %s!" % (tmp_path / "a.fastq", tmp_path / "b.fastq"))):
        p = tool("FastqDownsample", "-in1", tmp_path / (first + ".fastq"), "-in2", tmp_path / (second + ".fastq"), "-out1", tmp_path / "o1.gz", "-out2", tmp_path / "o2.gz", "-percentage", 20, "-test")
        assert p.returncode != 0 and msg in p.stderr.decode() and b"PE reads read" not in p.stdout
        r = M2.downsample(t1, t2[:cut]) if first == "a" else M2.downsample(t2[:cut], t1)
        assert p.stdout == M2.downsample_log(r).split(b"PE reads read")[0]   # the kept pairs were named before the ends were compared
        assert r.stats["entries"] == n


@pytest.mark.parametrize("args,msg", [(["-percentage", "0"], "Invalid percentage 0!"), (["-percentage", "100"], "Invalid percentage 100!"), (["-percentage", "-2.5"], "Invalid percentage -2.5!"),
                                      (["-percentage", "20", "-compression_level", "10"], "Invalid gzip compression level '10' given for FASTQ file '")])
def test_downsample_refusals(tmp_path, args, msg):
    a, _ = io_args("downsample_paired_end", tmp_path)
    p = tool("FastqDownsample", *a, *args)
    assert p.returncode != 0 and msg in p.stderr.decode()


def test_barcode_refusals(tmp_path):
    a, paths = io_args("barcode_test_01", tmp_path)
    p = tool("FastqExtractBarcode", *a, "-cut", -1)
    assert p.returncode != 0 and "must not be negative!" in p.stderr.decode()
    p = tool("FastqExtractBarcode", *a, "-cut", 10, "-compression_level", 11)
    assert p.returncode != 0 and "ArgumentException: Invalid gzip compression level '11' given for FASTQ file '%s'!" % paths[0] in p.stderr.decode()
    f = golden("FastqAddBarcode", "FastqAddBarcode_in.fastq.gz")
    p = tool("FastqAddBarcode", "-in1", f, f, "-in2", f, f, "-in_barcode", f, "-out1", tmp_path / "x1.gz", "-out2", tmp_path / "x2.gz")
    assert p.returncode != 0 and "must have the same number of files (2, 2 and 1 given)!" in p.stderr.decode()


def test_lists_of_files_and_plain_text_under_a_gz_name(tmp_path):
    """FastqAddBarcode over two triples equals the model's; FastqExtractBarcode_in2.fastq.gz is plain text"""
    f1, f2, f3 = (golden("FastqExtractBarcode", "FastqExtractBarcode_in1.fastq.gz"), golden("FastqExtractBarcode", "FastqExtractBarcode_in2.fastq.gz"), golden("FastqAddBarcode", "FastqAddBarcode_in.fastq.gz"))
    assert open(f2, "rb").read(1) == b"@"
    p = tool("FastqAddBarcode", "-in1", f1, f2, "-in2", f2, f1, "-in_barcode", f3, f3, "-out1", tmp_path / "x1.gz", "-out2", tmp_path / "x2.gz")
    assert p.returncode == 0, p.stderr
    t = inputs2("addbarcode_test_01")
    r = M2.barcode_add([(t[0], t[1], t[2]), (t[1], t[0], t[2])])
    assert [gzip.open(tmp_path / q, "rb").read() for q in ("x1.gz", "x2.gz")] == r.out
    p = tool("FastqConcat", "-in", f1, "-out", tmp_path / "c.gz", "-compression_level", 9)
    assert p.returncode == 0 and gzip.open(tmp_path / "c.gz", "rb").read() == M2.concat([t[0]]).out[0] and is_bgzf(tmp_path / "c.gz")   # (the input lacks its final line feed)


@pytest.mark.parametrize("name", sorted(HELP))
def test_help_text(name):
    p = tool(name, "--help")
    assert p.returncode == 0
    first, rest = p.stdout.decode().split("\n", 1)
    assert first.startswith(name + " (") and rest == HELP[name]   # (the first line carries this project's version)
