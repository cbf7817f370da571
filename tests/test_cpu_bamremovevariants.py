"""BamRemoveVariants without a device: the Python restatement (tests/bamremovevariants_oracle.py) turns the reference's fixture input into its expected output
(src/tools-TEST/BamRemoveVariants_Test.cpp), the host's VCF-to-table loader (ngs-bits_amd/host/RmVariants.hpp behind bin/libngsqc_hostapi.so) agrees with the
restatement's classification on a hand-written VCF, and the new symbols and what the tool refuses before a device is opened."""
import ctypes as C
import gzip
import os
import subprocess

import pytest

import bamremovevariants_oracle as R

ngsqc = __import__("importlib").import_module("ngs-bits_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GI = os.path.join(ROOT, "tests", "golden", "ref_in", "BamRemoveVariants")   # (a folder of its own: the tools' fixture loops over ref_in stay as they were)
IN1, VCF1 = os.path.join(GI, "BamRemoveVariants_in1.bam"), os.path.join(GI, "BamRemoveVariants_in1.vcf.gz")
OUT1 = os.path.join(ROOT, "tests", "golden", "ref_out", "BamRemoveVariants_out1.bam")
TOOL = os.path.join(ROOT, "ngs-bits_amd", "bin", "BamRemoveVariants")
NO_DEVICE = dict(os.environ, HIP_VISIBLE_DEVICES="-1")


def tool(*args, **kw):
    if not os.path.exists(TOOL):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ngs-bits_amd", "host"), "-s"])
    return subprocess.run([TOOL] + list(args), capture_output=True, text=True, timeout=120, **kw)


def hostapi():
    so = os.path.join(ROOT, "ngs-bits_amd", "bin", "libngsqc_hostapi.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ngs-bits_amd", "host"), "-s", os.path.join("..", "bin", "libngsqc_hostapi.so")])
    L = C.CDLL(so)
    L.ngsbits_rm_variants.restype = C.c_longlong
    L.ngsbits_rm_variants.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_int), C.c_longlong, C.c_char_p, C.c_int]
    return L


def host_table(path, ref_names, cap=4096):
    """(rows, None) or (None, message) from loadRmVariants"""
    names = (C.c_char_p * max(len(ref_names), 1))(*[n.encode() for n in ref_names])
    out, err = (C.c_int * (7 * cap))(), C.create_string_buffer(512)
    n = hostapi().ngsbits_rm_variants(path.encode(), names, len(ref_names), out, cap, err, 512)
    if n < 0:
        return None, err.value.decode()
    assert n <= cap
    return [tuple(out[7 * i:7 * i + 7]) for i in range(n)], None


def as_ints(rows):
    return [(t, b, e, s, k, r[0] if r else 0, o[0] if o else 0) for t, b, e, s, k, r, o in rows]


def test_restatement_turns_the_fixture_input_into_the_fixture_output():
    header, recs = R.read_bam(IN1)
    assert len(recs) == 29132
    h, out, c = R.run_file(IN1, VCF1, R.ref_names_of(header))
    eh, erecs = R.read_bam(OUT1)
    assert c == dict(passed=7933, dropped=2653, modified=0, skipped=0)
    assert h == eh                                   # the input's header, no @PG line
    assert len(out) == 15866 and out == erecs        # byte for byte per record


def test_restatement_modes_on_a_small_case():
    # one pair, the opener carries A>C at 101 and an insertion near 130; the closer carries G>T at 205
    import struct

    def rec(name, pos, cigar, seq, flag):
        nib = [R.NT16.index(c) for c in seq] + [0]
        sq = bytes(nib[i] << 4 | nib[i + 1] for i in range(0, len(seq), 2))
        body = struct.pack("<iiBBHHHiiii", 0, pos, len(name) + 1, 60, 0, len(cigar), flag, len(seq), 0, 0, 0) + name + b"\0"
        body += b"".join(struct.pack("<I", n << 4 | "MIDNSHP=X".index(op)) for n, op in cigar) + sq + b"\x1e" * len(seq)
        return struct.pack("<I", len(body)) + body
    a = rec(b"p", 100, [(30, "M"), (2, "I"), (8, "M")], "C" + "A" * 39, 0x41)
    b = rec(b"p", 200, [(9, "M")], "AAAAGAAAA", 0x81)
    lines = R.parse_vcf("chr1\t101\t.\tA\tC\t.\t.\t.\nchr1\t130\t.\tA\tAGG\t.\t.\t.\nchr1\t205\t.\tG\tT\t.\t.\t.\n")
    assert [ln.kind for ln in lines] == [R.SNV, R.OTHER, R.SNV] and lines[1].start == 130
    refs = ["chr1"]
    assert R.run([a, b], lines, refs) == ([], dict(passed=0, dropped=1, modified=0, skipped=0))
    assert R.run([a, b], lines, refs, mask=True)[1] == dict(passed=0, dropped=1, modified=1, skipped=0)   # the opener fails on the insertion: the closer is not looked at
    out, c = R.run([a, b], lines, refs, mask=True, keep_indels=True)
    assert c == dict(passed=1, dropped=0, modified=1, skipped=0) and R.Aln(out[0]).seq[0] == 1 and out[1] == b
    assert R.verdicts([a, b], lines, refs, mask=True) == bytes([2, 1]) and R.verdicts([a, b], lines, refs) == bytes([0, 1])
    out, c = R.run([a, b], lines, refs, mask=True, single_end=True)
    assert c == dict(passed=1, dropped=1, modified=0, skipped=0) and out == [b]   # (modified counts written records only)


HAND = (
    "##fileformat=VCFv4.2\n"
    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
    "1\t100\t.\tA\tC\t.\t.\t.\n"                       # SNV; the name "1" loses to "chr1" below
    "chr1\t100\t.\tA\tC\t.\t.\t.\n"                    # SNV
    "chr1\t100\t.\tA\tATT\t.\t.\t.\n"                  # insertion: GSvar start stays on the base in front
    "chr1\t110\t.\tACG\tA\t.\t.\t.\n"                  # deletion: start moves behind the common first base
    "chr1\t120\t.\tAC\tGT\t.\t.\t.\n"                  # MNP
    "chr1\t130\t.\tAT\tAG\t.\t.\t.\n"                  # an SNV behind a common first base: start 131
    "chr1\t140\t.\tA\t<NON_REF>\t.\t.\t.\n"            # valid, and never an SNV
    "chr1\t150\t.\tA\tC,G\t.\t.\t.\n"                  # the ALT column is one allele: invalid
    "chr1\t160\t.\ta\tc\t.\t.\t.\n"                    # lower case: invalid on this path
    "chr1\t170\t.\tA\tC\t.\t.\tDP=3;END=180\n"         # tabix takes the end from INFO
    "chr1\t200\t.\t" + "A" * 10000 + "\tA\t.\t.\t.\n"  # a 10 kb REF
    "chr1\t201\t.\tN\tA\t.\t.\t.\n"                    # REF not ACGT: invalid
    "chr7\t5\t.\tG\tT\t.\t.\t.\n"                      # a chromosome the BAM does not have
    "chrX\t7\t.\tG\tT\t.\t.\t.\n"
)


def test_host_loader_agrees_with_the_restatement(tmp_path):
    p = str(tmp_path / "hand.vcf.gz")
    with gzip.open(p, "wb") as f:
        f.write(HAND.encode())
    refs = ["chr1", "1", "chrX", "chrUn_x"]   # ("1" has chr1's number: the first reference with it takes the lines)
    lines = R.parse_vcf(HAND)
    exp = as_ints(R.table(lines, refs))
    rows, err = host_table(p, refs)
    assert err is None and rows == exp
    kinds = [r[4] for r in rows]
    assert kinds == [R.SNV, R.SNV, R.OTHER, R.OTHER, R.OTHER, R.SNV, R.OTHER, R.INVALID, R.INVALID, R.SNV, R.OTHER, R.INVALID, R.SNV, R.SNV]
    assert [r[0] for r in rows] == [-1] + [0] * 11 + [-1, 2]
    assert rows[2][3] == 100 and rows[3][3] == 111 and rows[5][3] == 131 and rows[5][5:] == (ord("T"), ord("G"))
    assert rows[9][1:3] == (170, 180) and rows[10][1:3] == (200, 10199)
    assert lines[7].message == "Cannot convert invalid VCF variant to GSvar variant: chr1:150 A>C,G"


@pytest.mark.parametrize("body", ["chr1\t100\t.\tA\tC\t.\t.\t.\nchr1\t99\t.\tA\tC\t.\t.\t.\n",
                                  "chr1\t100\t.\tA\tC\t.\t.\t.\nchr2\t5\t.\tA\tC\t.\t.\t.\nchr1\t200\t.\tA\tC\t.\t.\t.\n"])
def test_host_loader_refuses_an_unsorted_file(tmp_path, body):
    p = str(tmp_path / "bad.vcf.gz")
    with gzip.open(p, "wb") as f:
        f.write(body.encode())
    rows, err = host_table(p, ["chr1", "chr2"])
    assert rows is None and "not sorted" in err
    with pytest.raises(R.VcfOrderError):
        R.parse_vcf(body)


def test_new_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ngsqc.h")).read()
    for s in ("ngsqc_remove_variants(", "ngsqc_variant_verdicts(", "} ngsqc_rm_variant;", "} ngsqc_rm_params;", "} ngsqc_rm_counts;"):
        assert s in hdr
    assert "ngsqc_remove_variants" in ngsqc.capi.EXPORTS and "ngsqc_variant_verdicts" in ngsqc.capi.EXPORTS
    assert C.sizeof(ngsqc.RmVariant) == 20 and C.sizeof(ngsqc.RmParams) == 12 and C.sizeof(ngsqc.RmCounts) == 48
    assert hasattr(ngsqc.Handle, "remove_variants") and hasattr(ngsqc.Handle, "variant_verdicts")
    L = ngsqc.lib()
    assert L.ngsqc_abi_version() == 6
    # null arguments are refused before a device is touched
    assert L.ngsqc_remove_variants(None, None, 0, None, None, None) != 0 and L.ngsqc_variant_verdicts(None, None, 0, None, None, 0) != 0


def test_tool_refuses_before_a_device_is_opened(tmp_path):
    r = tool("-in", IN1, "-vcf", VCF1, "-out", str(tmp_path / "o.cram"), env=NO_DEVICE)
    assert r.returncode != 0 and "CRAM output is not supported" in r.stdout + r.stderr
    r = tool("-in", IN1, "-vcf", VCF1, "-out", str(tmp_path / "o.txt"), env=NO_DEVICE)
    assert r.returncode != 0 and "File extension has to be '.bam' or '.cram'" in r.stdout + r.stderr
    lone = str(tmp_path / "lone.vcf.gz")
    with open(lone, "wb") as f:
        f.write(open(VCF1, "rb").read())
    r = tool("-in", IN1, "-vcf", lone, "-out", str(tmp_path / "o.bam"), env=NO_DEVICE)
    assert r.returncode != 0 and "Could not determine tabix index of file " + lone in r.stdout + r.stderr
    r = tool("--help")
    assert r.returncode == 0 and "Removes reads which contain the provided variants" in r.stdout and "-keep_indels" in r.stdout and "-single_end" in r.stdout
