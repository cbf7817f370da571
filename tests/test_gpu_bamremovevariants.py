"""BamRemoveVariants on the device against the Python restatement (tests/bamremovevariants_oracle.py): the tool on the reference's case
(src/tools-TEST/BamRemoveVariants_Test.cpp), the fixture BAM with lines picked from its own reads in every flag combination and tile geometry, a designed BAM
whose records and lines sit on every boundary of the walks (tests/rmvar_cases.py), the errors and what the tool refuses.

<NON_REF>: the issue behind this tool expected "Invalid read position" for a <NON_REF> line over a deletion under -mask. The reference cannot give that: isSNV()
asks for an ALT of one character (src/cppNGS/VariantList.h:183-186), so main.cpp:55 and :89 never see "<NON_REF>", and such a line is an indel line. The
reachable errors are checked instead: a line Variant(VcfLine) refuses, "Could not find position" (BamReader.cpp:373) and setBases' "Cannot store character"."""
import os
import struct
import subprocess

import pytest

import bamremovevariants_oracle as R
import rmvar_cases as K

ngsqc = __import__("importlib").import_module("ngs-bits_amd")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GI = os.path.join(ROOT, "tests", "golden", "ref_in", "BamRemoveVariants")
IN1, VCF1 = os.path.join(GI, "BamRemoveVariants_in1.bam"), os.path.join(GI, "BamRemoveVariants_in1.vcf.gz")
OUT1 = os.path.join(ROOT, "tests", "golden", "ref_out", "BamRemoveVariants_out1.bam")
TOOL = os.path.join(ROOT, "ngs-bits_amd", "bin", "BamRemoveVariants")
COMBOS = [dict(mask=m, keep_indels=k, single_end=s) for m, k in ((False, False), (True, False), (True, True)) for s in (False, True)]


def run_tool(*args, env=None):
    return subprocess.run([TOOL] + list(args), capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})))


def flags(kw):
    return [f for f, on in (("-mask", kw.get("mask")), ("-keep_indels", kw.get("keep_indels")), ("-single_end", kw.get("single_end"))) if on]


def with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


def device_run(path, out, rows, env=None, **kw):
    def go():
        h = ngsqc.Handle(path=path)
        try:
            return h.remove_variants(out, rows, **kw)
        finally:
            h.close()
    return with_env(env or {}, go)


def device_verdicts(path, rows, env=None, **kw):
    def go():
        h = ngsqc.Handle(path=path)
        try:
            return h.variant_verdicts(rows, **kw)
        finally:
            h.close()
    return with_env(env or {}, go)


def reopen_ok(path, n_expected):
    h = ngsqc.Handle(path=path)   # (ngsqc_open checks every member's CRC)
    try:
        assert h.n_records == n_expected
    finally:
        h.close()


# ---- (a) the tool on the reference case ----
def test_tool_reference_case(tmp_path):
    out = str(tmp_path / "out.bam")
    r = run_tool("-in", IN1, "-vcf", VCF1, "-out", out)
    assert r.returncode == 0, r.stderr
    h, recs = R.read_bam(out)
    eh, erecs = R.read_bam(OUT1)
    assert h == eh and len(recs) == 15866 and recs == erecs
    assert r.stdout == "pairs passed: 7933\npairs dropped: 2653\nreads modified: 0\nskipped reads: 0\n"
    reopen_ok(out, 15866)


# ---- (b) the fixture BAM with lines picked from its own reads ----
@pytest.fixture(scope="module")
def picked():
    header, recs = R.read_bam(IN1)
    refs = R.ref_names_of(header)
    lines = R.parse_vcf(K.vcf_text(K.picked_lines(recs, refs)))
    exp = [R.run(recs, lines, refs, **kw) for kw in COMBOS]
    assert exp[2][1]["modified"] > 1000 and exp[2][1]["dropped"] > 100 and exp[0][1]["passed"] > 0   # the lines ARE carried, by SNV and by indel
    return dict(header=header, recs=recs, refs=refs, lines=lines, rows=R.table(lines, refs), exp=exp)


@pytest.mark.parametrize("env", [{}, {"NGSQC_TILE_MEMBERS": "8"}, {"NGSQC_NAME_HASH_BITS": "4"}, {"NGSQC_WRITE_WINDOW_PIECES": "1"}],
                         ids=["plain", "tiles_of_8_members", "hash_of_4_bits", "one_piece_windows"])
def test_fixture_with_picked_lines(tmp_path, picked, env):
    for i, kw in enumerate(COMBOS):
        out = str(tmp_path / f"o{i}.bam")
        got = device_run(IN1, out, picked["rows"], env, **kw)
        exp_recs, exp_counts = picked["exp"][i]
        h, recs = R.read_bam(out)
        assert h == picked["header"], kw
        assert len(recs) == len(exp_recs) and recs == exp_recs, kw
        assert got == exp_counts, kw
    if not env:
        assert device_verdicts(IN1, picked["rows"], mask=True) == R.verdicts(picked["recs"], picked["lines"], picked["refs"], True, False)


# ---- (c) the designed BAM ----
@pytest.fixture(scope="module")
def designed(tmp_path_factory):
    d = tmp_path_factory.mktemp("rmvar")
    recs, raw = K.designed()
    refs = [n for n, _ in K.REFS]
    path, vcf = str(d / "designed.bam"), str(d / "designed.vcf.gz")
    open(path, "wb").write(K.bam_bytes(recs))
    K.write_vcf(vcf, K.vcf_text(raw))
    lines = R.load_vcf(vcf)
    header, back = R.read_bam(path)
    assert back == recs and 200 <= len(recs) <= 400
    return dict(path=path, vcf=vcf, header=header, recs=recs, refs=refs, lines=lines, rows=R.table(lines, refs))


@pytest.mark.parametrize("env", [{}, {"NGSQC_TILE_MEMBERS": "1"}, {"NGSQC_TILE_MEMBERS": "1", "NGSQC_NAME_HASH_BITS": "4"}],
                         ids=["plain", "one_member_tiles", "one_member_tiles_hash_of_4_bits"])
def test_designed_matches_restatement(tmp_path, designed, env):
    D = designed
    for i, kw in enumerate(COMBOS):
        exp_recs, exp_counts = R.run(D["recs"], D["lines"], D["refs"], **kw)
        out = str(tmp_path / f"o{i}.bam")
        got = device_run(D["path"], out, D["rows"], env, **kw)
        h, recs = R.read_bam(out)
        assert h == D["header"], kw
        for k, (a, b) in enumerate(zip(recs, exp_recs)):
            assert a == b, (kw, k, R.Rec(b).name)
        assert len(recs) == len(exp_recs), kw
        assert got == exp_counts, kw
        if not kw["single_end"]:
            vd = device_verdicts(D["path"], D["rows"], env, **kw)
            exp_vd = R.verdicts(D["recs"], D["lines"], D["refs"], kw["mask"], kw["keep_indels"])
            assert vd == exp_vd, (kw, [(k, R.Rec(D["recs"][k]).name, vd[k], exp_vd[k]) for k in range(len(vd)) if vd[k] != exp_vd[k]][:8])


def test_designed_through_the_tool(tmp_path, designed):
    D = designed
    for i, kw in enumerate(COMBOS):
        exp_recs, c = R.run(D["recs"], D["lines"], D["refs"], **kw)
        out = str(tmp_path / f"t{i}.bam")
        r = run_tool("-in", D["path"], "-vcf", D["vcf"], "-out", out, *flags(kw))
        assert r.returncode == 0, r.stderr
        assert r.stdout == f"pairs passed: {c['passed']}\npairs dropped: {c['dropped']}\nreads modified: {c['modified']}\nskipped reads: {c['skipped']}\n", kw
        assert R.read_bam(out) == (D["header"], exp_recs), kw
        reopen_ok(out, len(exp_recs))


# ---- (d) errors ----
def small_case(tmp_path, name, recs, vcf_lines):
    refs = [("chr1", 100000)]
    path, vcf = str(tmp_path / (name + ".bam")), str(tmp_path / (name + ".vcf.gz"))
    open(path, "wb").write(K.bam_bytes(recs, refs))
    K.write_vcf(vcf, K.vcf_text(vcf_lines))
    return path, vcf, R.load_vcf(vcf), ["chr1"]


def pair(name, *a, **kw):
    return [K.record(name, 0x41, *a, **kw), K.record(name, 0x81, 0, 50000, "40M", "A" * 40)]


def test_non_ref_over_a_deletion_is_an_indel_line(tmp_path):
    recs = pair("d", 0, 1000, "20M2D20M", "C" * 40)
    path, vcf, lines, refs = small_case(tmp_path, "nonref", recs, [("chr1", 1021, "A", "<NON_REF>")])
    assert lines[0].kind == R.OTHER
    for kw, text in ((dict(mask=True), "pairs passed: 0\npairs dropped: 1\nreads modified: 0\nskipped reads: 0\n"),
                     (dict(mask=True, keep_indels=True), "pairs passed: 1\npairs dropped: 0\nreads modified: 0\nskipped reads: 0\n")):
        out = str(tmp_path / "o.bam")
        r = run_tool("-in", path, "-vcf", vcf, "-out", out, *flags(kw))
        assert r.returncode == 0 and r.stdout == text, (kw, r.stdout, r.stderr)
        assert R.run(recs, lines, refs, **kw)[0] == R.read_bam(out)[1]


def test_invalid_line_fails_only_when_visited(tmp_path):
    recs = pair("v", 0, 1000, "40M", "C" * 40) + pair("w", 0, 3000, "40M", "C" * 40)
    # no record visits it: far from every read, and behind a carried line of a default-mode visit
    path, vcf, lines, refs = small_case(tmp_path, "unvisited", recs, [("chr1", 1001, "A", "C"), ("chr1", 1010, "A", "C,G"), ("chr1", 2000, "a", "c")])
    out = str(tmp_path / "o.bam")
    r = run_tool("-in", path, "-vcf", vcf, "-out", out)
    assert r.returncode == 0 and r.stdout == "pairs passed: 1\npairs dropped: 1\nreads modified: 0\nskipped reads: 0\n", r.stderr
    # -mask goes on behind the carried SNV and reaches it
    r = run_tool("-in", path, "-vcf", vcf, "-out", out, "-mask")
    assert r.returncode != 0 and "Cannot convert invalid VCF variant to GSvar variant: chr1:1010 A>C,G" in r.stdout + r.stderr
    # the same line moved under the second pair's read: the first pair is fine, the second fails the run
    path, vcf, lines, refs = small_case(tmp_path, "visited", recs, [("chr1", 3010, "a", "c")])
    r = run_tool("-in", path, "-vcf", vcf, "-out", out)
    assert r.returncode != 0 and "Cannot convert invalid VCF variant to GSvar variant: chr1:3010 a>c" in r.stdout + r.stderr
    with pytest.raises(R.RmError) as e:
        R.run(recs, lines, refs)
    assert (e.value.code, e.value.record, e.value.variant) == (R.ERR_INVALID_LINE, 2, 0)
    with pytest.raises(ngsqc.NgsqcError) as d:
        device_run(path, out, R.table(lines, refs))
    assert d.value.rm_error == (2, ngsqc.RMERR_INVALID_LINE, 0)
    assert device_verdicts(path, R.table(lines, refs)) == bytes([1, 1, 8, 1])


def test_walk_and_base_errors(tmp_path):
    # an SNV whose start lies behind the read's last base: the walk does not find it (BamReader.cpp:373); the earliest record in file order decides
    recs = pair("p", 0, 1000, "40M", "A" * 40) + pair("q", 0, 2000, "40M", "A" * 40)
    path, vcf, lines, refs = small_case(tmp_path, "notfound", recs, [("chr1", 1040, "AT", "AG"), ("chr1", 2040, "AT", "AG")])
    out = str(tmp_path / "o.bam")
    r = run_tool("-in", path, "-vcf", vcf, "-out", out)
    assert r.returncode != 0 and "Could not find position 1041 in read p with start position 1001!" in r.stdout + r.stderr
    # a closer whose opener failed is not visited: its error does not count
    recs = [K.record("z", 0x41, 0, 1000, "40M", "C" + "A" * 39), K.record("z", 0x81, 0, 2000, "40M", "A" * 40)]
    path, vcf, lines, refs = small_case(tmp_path, "unvisited_closer", recs, [("chr1", 1001, "A", "C"), ("chr1", 2040, "AT", "AG")])
    r = run_tool("-in", path, "-vcf", vcf, "-out", out)
    assert r.returncode == 0 and r.stdout == "pairs passed: 0\npairs dropped: 1\nreads modified: 0\nskipped reads: 0\n", r.stderr
    assert R.run(recs, lines, refs)[1] == dict(passed=0, dropped=1, modified=0, skipped=0)
    r = run_tool("-in", path, "-vcf", vcf, "-out", out, "-single_end")
    assert r.returncode != 0 and "Could not find position 2041 in read z with start position 2001!" in r.stdout + r.stderr
    # setBases stores A, C, G, T, N alone: a masked read with another base
    recs = pair("m", 0, 1000, "40M", K.seq_with(40, {0: "C", 17: "R", 30: "M"}))
    path, vcf, lines, refs = small_case(tmp_path, "badbase", recs, [("chr1", 1001, "A", "C")])
    r = run_tool("-in", path, "-vcf", vcf, "-out", out, "-mask")
    assert r.returncode != 0 and "Cannot store character 'R' in BAM/CRAM file. Only A,C,G,T,N are allowed!" in r.stdout + r.stderr
    r = run_tool("-in", path, "-vcf", vcf, "-out", out)
    assert r.returncode == 0 and r.stdout.startswith("pairs passed: 0\npairs dropped: 1\n")


def test_unsorted_table_is_refused(tmp_path):
    recs = pair("u", 0, 1000, "40M", "A" * 40)
    path = str(tmp_path / "u.bam")
    open(path, "wb").write(K.bam_bytes(recs, [("chr1", 100000)]))
    with pytest.raises(ngsqc.NgsqcError) as e:
        device_run(path, str(tmp_path / "o.bam"), [(0, 2000, 2000, 2000, 0, b"A", b"C"), (0, 1000, 1000, 1000, 0, b"A", b"C")])
    assert "not sorted" in str(e.value)


# ---- (e) what the tool refuses ----
def test_tool_refusals(tmp_path):
    r = run_tool("-in", IN1, "-vcf", VCF1, "-out", str(tmp_path / "o.cram"))
    assert r.returncode != 0 and "CRAM output is not supported" in r.stdout + r.stderr
    lone = str(tmp_path / "lone.vcf.gz")
    open(lone, "wb").write(open(VCF1, "rb").read())
    r = run_tool("-in", IN1, "-vcf", lone, "-out", str(tmp_path / "o.bam"))
    assert r.returncode != 0 and "Could not determine tabix index of file " + lone in r.stdout + r.stderr
    # a shard of the file cannot be paired
    h = ngsqc.Handle(path=IN1, shard=(0, 2))
    try:
        with pytest.raises(ngsqc.NgsqcError):
            h.remove_variants(str(tmp_path / "s.bam"), [])
    finally:
        h.close()
