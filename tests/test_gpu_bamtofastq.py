"""BamToFastq on the GPU (ngsqc_bam_to_fastq: csrc/fastq.hip over csrc/join.h and csrc/deflate.hip; bin/BamToFastq) against the reference's expected FASTQ
files (src/tools-TEST/BamToFastq_Test.cpp) and the Python restatement (tests/bamtofastq_oracle.py). The contract is the decompressed text; every output is also
checked member by member as BGZF and must end with the EOF member."""
import gzip
import os
import random
import struct
import subprocess
import zlib

import pytest

import bamgen_lib as G
import bamtofastq_oracle as Q
import cram_twin
from bamfilter_oracle import read_bam
from test_cpu_bamtofastq import CASES, IN1, IN3, golden, region_of

ngsqc = __import__("importlib").import_module("ngs-bits_amd")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "ngs-bits_amd", "bin", "BamToFastq")
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def text_of(path):
    """the decompressed text, after checking every BGZF member (CRC32, ISIZE, BSIZE) and the EOF member at the end"""
    z = open(path, "rb").read()
    assert z.endswith(EOF_MEMBER)
    out, o = [], 0
    while o < len(z):
        assert z[o:o + 4] == b"\x1f\x8b\x08\x04" and z[o + 12:o + 16] == b"BC\x02\x00", o
        bsize = struct.unpack_from("<H", z, o + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", z, o + bsize - 8)
        d = zlib.decompressobj(-15)
        piece = d.decompress(z[o + 18:o + bsize - 8]) + d.flush()
        assert d.eof and not d.unused_data and len(piece) == isize and zlib.crc32(piece) == crc, o
        assert isize <= 0xff00
        out.append(piece); o += bsize
    t = b"".join(out)
    assert gzip.decompress(z) == t
    return t


def with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


def write_bam(path, header, recs, member=4000):
    """a BAM of the records in members of `member` bytes (many tiles under NGSQC_TILE_MEMBERS)"""
    raw = header + b"".join(recs)
    open(path, "wb").write(b"".join(cram_twin._bgzf(raw[o:o + member]) for o in range(0, len(raw), member)) + cram_twin._bgzf(b""))


def tool_args(name, kw):
    a = ["-in", IN3 if name == "single_end" else IN1]
    if kw.get("fix"): a.append("-fix")
    if kw.get("remove_duplicates"): a.append("-remove_duplicates")
    if "region" in kw: a += ["-reg", kw["region"]]
    if "extend" in kw: a += ["-extend", str(kw["extend"])]
    return a


def device(path, out1, out2, **kw):
    h = ngsqc.Handle(path=path)
    try:
        return h.to_fastq(out1, out2, **kw)
    finally:
        h.close()


@pytest.mark.parametrize("name,kw,e1,e2", CASES, ids=[c[0] for c in CASES])
def test_tool_reference_cases(tmp_path, name, kw, e1, e2):
    args = tool_args(name, kw)
    if name == "fix":   # the reference test's input: every record twice
        header, recs = read_bam(IN1)
        doubled = str(tmp_path / "doubled.bam"); write_bam(doubled, header, recs + recs, member=60000)
        args[1] = doubled
    o1, o2 = str(tmp_path / "o1.fastq.gz"), str(tmp_path / "o2.fastq.gz")
    r = subprocess.run([TOOL] + args + ["-out1", o1] + (["-out2", o2] if e2 else []) + ["-write_buffer_size", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert text_of(o1) == golden(e1)
    if e2:
        assert text_of(o2) == golden(e2)
    else:
        assert not os.path.exists(o2)
    _, _, c = __import__("test_cpu_bamtofastq").run_case(name, kw)
    lines = r.stdout.split("\n")
    exp = Q.stdout_lines(c, e2 is not None, kw.get("remove_duplicates", False), kw.get("fix", False))
    assert lines[:len(exp)] == exp and lines[len(exp)].startswith("Time elapsed                    : ")


@pytest.mark.parametrize("name,kw,e1,e2", [c for c in CASES if c[0] != "fix"], ids=[c[0] for c in CASES if c[0] != "fix"])
def test_handle_reference_cases(tmp_path, name, kw, e1, e2):
    header, _ = read_bam(IN3 if name == "single_end" else IN1)
    kw = dict(kw); paired = kw.pop("paired", True)
    if "region" in kw:
        kw["region"] = region_of(header, kw["region"])
    o1, o2 = str(tmp_path / "o1.fastq.gz"), (str(tmp_path / "o2.fastq.gz") if paired else None)
    got = device(IN3 if name == "single_end" else IN1, o1, o2, **kw)
    _, _, c = Q.to_fastq(read_bam(IN3 if name == "single_end" else IN1)[1], paired=paired, **kw)
    assert got == c
    assert text_of(o1) == golden(e1)
    if paired:
        assert text_of(o2) == golden(e2)


@pytest.fixture(scope="module")
def shuffled(tmp_path_factory):
    """in1's records twice, shuffled (mates and name repeats tiles apart), with hand records: q = 223, 0xff qualities, l_seq = 0, unpaired"""
    header, recs = read_bam(IN1)
    rng = random.Random(3)
    extra = [Q.make_record("h1", 0x1 | 0x40 | 0x10, "ACGTNACGT", [30, 223, 31, 32, 223, 33, 34, 35, 36]), Q.make_record("h1", 0x1 | 0x80, "AC", [255, 255]),
             Q.make_record("h2", 0x1 | 0x80 | 0x4, "", []), Q.make_record("h2", 0x1 | 0x40 | 0x4, "", []), Q.make_record("h3", 0, "ACGT", [223, 1, 2, 3])]
    recs = recs + recs + extra
    rng.shuffle(recs)
    path = str(tmp_path_factory.mktemp("shuf") / "shuf.bam")
    write_bam(path, header, recs)
    return path, recs


KWS = [dict(), dict(fix=True), dict(remove_duplicates=True, extend=160), dict(fix=True, remove_duplicates=True)]


def test_multi_tile_matches_restatement(tmp_path, shuffled):
    path, recs = shuffled
    for i, kw in enumerate(KWS):
        e1, e2, c = Q.to_fastq(recs, **kw)
        ref = None
        for env in ({}, {"NGSQC_TILE_MEMBERS": "2"}, {"NGSQC_NAME_HASH_BITS": "4", "NGSQC_TILE_MEMBERS": "3"}, {"NGSQC_WRITE_WINDOW_PIECES": "1"},
                    {"NGSQC_WRITE_WINDOW_PIECES": "3", "NGSQC_TILE_MEMBERS": "2"}):
            o1, o2 = str(tmp_path / f"{i}_1.gz"), str(tmp_path / f"{i}_2.gz")
            got = with_env(env, lambda: device(path, o1, o2, **kw))
            assert got == c, (kw, env)
            b = (open(o1, "rb").read(), open(o2, "rb").read())
            if ref is None:
                assert text_of(o1) == e1 and text_of(o2) == e2, kw
                ref = b
            else:
                assert b == ref, (kw, env)   # the bytes do not depend on tiles, windows or hash collisions
        o1 = str(tmp_path / f"{i}_se.gz")
        s1, _, sc = Q.to_fastq(recs, paired=False, **kw)
        assert with_env({"NGSQC_TILE_MEMBERS": "2", "NGSQC_NAME_HASH_BITS": "4"}, lambda: device(path, o1, None, **kw)) == sc
        assert text_of(o1) == s1


def test_bamgen_multi_tile(tmp_path):
    src = str(tmp_path / "g.bam")
    G.write(src, n_reads=300_000, flavor=8)   # (flavor bit 3: mates share read names)
    _, recs = read_bam(src)
    e1, e2, c = Q.to_fastq(recs)
    o1, o2 = str(tmp_path / "o1.gz"), str(tmp_path / "o2.gz")
    assert with_env({"NGSQC_TILE_MEMBERS": "64"}, lambda: device(src, o1, o2)) == c
    assert c["paired"] > 100_000
    assert text_of(o1) == e1 and text_of(o2) == e2


def test_levels_give_the_same_text(tmp_path):
    e1, e2, _ = Q.to_fastq(read_bam(IN1)[1])
    sizes = []
    for level in range(10):
        o1, o2 = str(tmp_path / f"l{level}_1.gz"), str(tmp_path / f"l{level}_2.gz")
        device(IN1, o1, o2, compression_level=level)
        assert text_of(o1) == e1 and text_of(o2) == e2, level
        sizes.append(os.path.getsize(o1))
    assert sizes[0] > sizes[1] > sizes[6] and sizes[4] == sizes[9]


def test_cram_input_equals_bam_twin(tmp_path):
    import cram_encode as CE
    t = cram_twin.make_twin(os.path.join(ROOT, "tests", "golden", "ref_in", "MappingQC_in2.bam"), str(tmp_path), max_records=20000)
    cram = str(tmp_path / "twin.cram"); CE.encode(t["bam"], cram, t["genome"])
    a = (str(tmp_path / "b1.gz"), str(tmp_path / "b2.gz")); b = (str(tmp_path / "c1.gz"), str(tmp_path / "c2.gz"))
    ga = device(t["bam"], *a)
    ngsqc.set_reference(t["fasta"])
    try:
        gb = device(cram, *b)
    finally:
        ngsqc.set_reference(None)
    assert ga == gb and ga["paired"] > 0
    assert text_of(a[0]) == text_of(b[0]) and text_of(a[1]) == text_of(b[1])
    e1, e2, c = Q.to_fastq(read_bam(t["bam"])[1])
    assert ga == c and text_of(a[0]) == e1


def test_complement_error(tmp_path):
    header, recs = read_bam(IN1)
    bad = [Q.make_record("zz", 0x1 | 0x40 | 0x10, "ACGRTY", [30] * 6), Q.make_record("zz", 0x1 | 0x80, "ACGT", [30] * 4)]
    path = str(tmp_path / "bad.bam"); write_bam(path, header, recs[:500] + bad + recs[500:], member=60000)
    r = subprocess.run([TOOL, "-in", path, "-out1", str(tmp_path / "o1.gz"), "-out2", str(tmp_path / "o2.gz")], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "ProgrammingException: Could not convert base 'Y' to complement!" in r.stderr
    with pytest.raises(ngsqc.NgsqcError) as e:
        device(path, str(tmp_path / "p1.gz"), str(tmp_path / "p2.gz"))
    assert e.value.code == -2 and "Could not convert base 'Y' to complement!" in str(e.value)
    # an unmatched record is never written: no error
    path2 = str(tmp_path / "bad2.bam"); write_bam(path2, header, recs + bad[:1], member=60000)
    device(path2, str(tmp_path / "q1.gz"), str(tmp_path / "q2.gz"))


def test_shard_handle_is_refused(tmp_path):
    h = ngsqc.Handle(path=IN1, shard=(0, 2))
    try:
        with pytest.raises(ngsqc.NgsqcError):
            h.to_fastq(str(tmp_path / "x.gz"), str(tmp_path / "y.gz"))
    finally:
        h.close()
