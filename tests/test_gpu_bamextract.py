"""BamExtract on the GPU (ngsqc_extract_reads / ngsqc_match_names: csrc/extract.hip over csrc/join.h, csrc/recwrite.h and csrc/deflate.hip; bin/BamExtract)
against the reference's fixture (src/tools-TEST/BamExtract_Test.cpp: its expected output, fed back as input with its own ID list, must come out whole) and the
Python restatement (tests/bamextract_oracle.py). Outputs are read back with Python's gzip, and through ngsqc_open, whose K1 checks every member's CRC."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import bamextract_oracle as X
import cram_twin
from bamfilter_oracle import read_bam

ngsqc = __import__("importlib").import_module("ngs-bits_amd")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GI = os.path.join(ROOT, "tests", "golden", "ref_in")
GO = os.path.join(ROOT, "tests", "golden", "ref_out")
IDS = os.path.join(GI, "BamExtract", "BamExtract_ids.txt")
OUT1 = os.path.join(GO, "BamExtract_out1.bam")
TOOL = os.path.join(ROOT, "ngs-bits_amd", "bin", "BamExtract")
FOREIGN = sorted(X.parse_ids(open(IDS, "rb").read()))   # 1117 names that occur in no other golden BAM
GOLDEN = sorted(f for f in os.listdir(GI) if f.endswith(".bam"))


def with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


def reopen_ok(path, n_expected):
    h = ngsqc.Handle(path=path)
    try:
        assert h.n_records == n_expected
    finally:
        h.close()


def device_extract(path, out, names, out2=None):
    h = ngsqc.Handle(path=path)
    try:
        return h.extract(out, names, out2)
    finally:
        h.close()


def device_match(path, names):
    h = ngsqc.Handle(path=path)
    try:
        return h.match_names(names)
    finally:
        h.close()


def third_of_names(recs, seed):
    names = sorted({X.name_of(b) for b in recs} - {b""})
    return random.Random(seed).sample(names, (len(names) + 2) // 3)


def usable(ids):
    """the listed names a record can carry (1 to 254 bytes, no NUL): the library leaves the others out of the lookup and still counts them"""
    return {i for i in ids if 1 <= len(i) <= 254 and b"\0" not in i}


def check_against_oracle(header, recs, ids, out, out2, got, what):
    e1, e2, counts = X.extract(recs, usable(ids), out2 is not None)
    counts["names"] = len(set(ids))
    h1, r1 = read_bam(out)
    assert h1 == header and len(r1) == len(e1) and r1 == e1, what
    assert got == counts, (what, got, counts)
    reopen_ok(out, len(e1))
    if out2 is not None:
        h2, r2 = read_bam(out2)
        assert h2 == header and len(r2) == len(e2) and r2 == e2, what
        reopen_ok(out2, len(e2))
    return e1, e2


# ---- 1. the reference's vector ----
def test_tool_reference_vector(tmp_path):
    out, out2 = str(tmp_path / "o.bam"), str(tmp_path / "o2.bam")
    r = subprocess.run([TOOL, "-in", OUT1, "-ids", IDS, "-out", out, "-out2", out2], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    log = open(os.path.join(GO, "BamExtract_out1.log")).read().splitlines(True)
    assert log[:2] == ["Read IDs: 1117\n", "Reads written to 'out': 2260\n"]
    assert r.stdout == log[0] + log[1] + "Reads written to 'out2': 0\n"
    header, recs = read_bam(OUT1)
    assert read_bam(out) == (header, recs)
    assert read_bam(out2) == (header, [])   # the header and no record
    reopen_ok(out, 2260); reopen_ok(out2, 0)
    # without -out2: the same file, and no third line
    r = subprocess.run([TOOL, "-in", OUT1, "-ids", IDS, "-out", str(tmp_path / "p.bam")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout == log[0] + log[1]
    assert open(str(tmp_path / "p.bam"), "rb").read() == open(out, "rb").read()


# ---- 2. every golden BAM ----
@pytest.mark.parametrize("bam", GOLDEN)
def test_golden_bams_match_restatement(tmp_path, bam):
    src = os.path.join(GI, bam)
    header, recs = read_bam(src)
    ids = third_of_names(recs, 11) + FOREIGN
    out, out2, solo = str(tmp_path / "o.bam"), str(tmp_path / "o2.bam"), str(tmp_path / "s.bam")
    h = ngsqc.Handle(path=src)
    try:
        got2 = h.extract(out, ids, out2)
        got1 = h.extract(solo, ids)
    finally:
        h.close()
    e1, e2 = check_against_oracle(header, recs, ids, out, out2, got2, bam)
    check_against_oracle(header, recs, ids, solo, None, got1, bam)
    assert got1 == dict(got2, out2=0) and got2["names"] == len(set(ids))
    # out and out2 together hold every input record exactly once, each in file order
    assert len(e1) + len(e2) == len(recs) and 0 < len(e1) < len(recs)
    r1, r2 = read_bam(out)[1], read_bam(out2)[1]
    i1 = i2 = 0
    for b in recs:
        w = X.written(X.Rec(b))
        if i1 < len(r1) and r1[i1] == w: i1 += 1
        else: assert i2 < len(r2) and r2[i2] == w; i2 += 1
    assert (i1, i2) == (len(r1), len(r2))


def cg_record(name, l_seq=40):
    """a long-read style record: the real CIGAR in CG:B,I, the placeholder "l_seq S, ref_len N" in its place (no golden BAM holds one)"""
    real = [(l_seq - 4, 0), (2, 1), (2, 0), (3, 2)]
    ops = [(l_seq, 4), (l_seq - 2 + 3, 3)]
    aux = b"NMC\1" + b"CGBI" + struct.pack("<I", len(real)) + b"".join(struct.pack("<I", l << 4 | o) for l, o in real) + b"RGZgrp\0"
    body = struct.pack("<iiBBHHHiiii", 0, 5000, len(name) + 1, 60, 4680, len(ops), 0, l_seq, -1, -1, 0) + name + b"\0"
    body += b"".join(struct.pack("<I", l << 4 | o) for l, o in ops) + b"\x12" * ((l_seq + 1) // 2) + b"\x1e" * l_seq + aux
    return struct.pack("<I", len(body)) + body


def test_cg_tag_records_are_written_as_bam_write1_writes_them(tmp_path):
    recs = [record(b"plain1\0"), cg_record(b"cg-listed"), record(b"plain2\0"), cg_record(b"cg-other"), record(b"plain3\0")]
    assert [bool(X.Rec(b).cg()) for b in recs] == [False, True, False, True, False]
    assert X.written(X.Rec(recs[1])) != recs[1]
    src = str(tmp_path / "cg.bam")
    write_bam(src, recs)
    header = read_bam(src)[0]
    ids = [b"cg-listed", b"plain3"]
    out, out2 = str(tmp_path / "o.bam"), str(tmp_path / "o2.bam")
    got = device_extract(src, out, ids, out2)
    check_against_oracle(header, recs, ids, out, out2, got, "cg")
    assert got == dict(out=2, out2=3, names=2)


# ---- 3. CRAM input through the existing reader ----
def test_cram_input_equals_bam_twin(tmp_path):
    import cram_encode as CE
    t = cram_twin.make_twin(os.path.join(GI, "MappingQC_in2.bam"), str(tmp_path), max_records=5000)
    cram = str(tmp_path / "twin.cram"); CE.encode(t["bam"], cram, t["genome"])
    header, recs = read_bam(t["bam"])
    ids = third_of_names(recs, 3)
    a, a2, b, b2 = (str(tmp_path / n) for n in ("a.bam", "a2.bam", "b.bam", "b2.bam"))
    ga = device_extract(t["bam"], a, ids, a2)
    ngsqc.set_reference(t["fasta"])
    try:
        gb = device_extract(cram, b, ids, b2)
    finally:
        ngsqc.set_reference(None)
    assert ga == gb and ga["out"] > 0 and ga["out2"] > 0
    assert read_bam(a)[1] == read_bam(b)[1] and read_bam(a2)[1] == read_bam(b2)[1]
    check_against_oracle(header, recs, ids, a, a2, ga, "twin")


# ---- 4. independence of geometry ----
def test_geometry_does_not_change_the_files(tmp_path):
    src = os.path.join(GI, "MappingQC_in2.bam")
    header, recs = read_bam(src)
    ids = third_of_names(recs, 5)
    assert 300 < len(ids) < 5000   # (NGSQC_NAME_HASH_BITS=4 probes linearly: the list stays in the low thousands)
    out, out2 = str(tmp_path / "o.bam"), str(tmp_path / "o2.bam")
    got = device_extract(src, out, ids, out2)
    e1, e2 = check_against_oracle(header, recs, ids, out, out2, got, "default")
    ref1, ref2 = open(out, "rb").read(), open(out2, "rb").read()
    assert len(ref2) > 2 * 0xff00 // 4   # (several pieces of output)
    for env in ({"NGSQC_TILE_MEMBERS": "2"}, {"NGSQC_TILE_MEMBERS": "3"}, {"NGSQC_WRITE_WINDOW_PIECES": "1"}, {"NGSQC_WRITE_WINDOW_PIECES": "3"},
                {"NGSQC_WRITE_WINDOW_PIECES": "1", "NGSQC_TILE_MEMBERS": "2"}):
        a, a2 = str(tmp_path / "a.bam"), str(tmp_path / "a2.bam")
        assert with_env(env, lambda: device_extract(src, a, ids, a2)) == got, env
        assert open(a, "rb").read() == ref1 and open(a2, "rb").read() == ref2, env
    a, a2 = str(tmp_path / "c.bam"), str(tmp_path / "c2.bam")
    assert with_env({"NGSQC_NAME_HASH_BITS": "4"}, lambda: device_extract(src, a, ids, a2)) == got
    assert read_bam(a) == (header, e1) and read_bam(a2) == (header, e2)
    assert np.array_equal(with_env({"NGSQC_NAME_HASH_BITS": "4"}, lambda: device_match(src, ids)), device_match(src, ids))


# ---- 5. designed names through the lookup alone ----
def record(field, flag=0, l_seq=12):
    """a record whose name FIELD is the given bytes (l_read_name = len(field), terminator included by the caller)"""
    tid, pos = (-1, -1) if flag & 4 else (0, 100)
    ops = [] if flag & 4 else [(l_seq, 0)]
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(field), 60, 4681, len(ops), flag, l_seq, -1, -1, 0) + field
    body += b"".join(struct.pack("<I", l << 4 | o) for l, o in ops) + b"\x11" * ((l_seq + 1) // 2) + b"\x1e" * l_seq
    return struct.pack("<I", len(body)) + body


def write_bam(path, recs, member=60000):
    text = "@HD\tVN:1.6\n@SQ\tSN:c1\tLN:1000000\n"
    raw = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", 1) + struct.pack("<i", 3) + b"c1\0" + struct.pack("<i", 1000000) + b"".join(recs)
    open(path, "wb").write(b"".join(cram_twin._bgzf(raw[o:o + member]) for o in range(0, len(raw), member)) + cram_twin._bgzf(b""))
    return len(raw) - len(b"".join(recs))   # the header's bytes


def expected_match(recs, ids):
    ids = usable(ids)
    return np.array([1 if X.name_of(b) in ids else 0 for b in recs], dtype=np.uint8)


def name_of_length(n, last):
    return (b"L%03d" % n + b"abcdefghijklmnopqrstuvwxyz0123456789" * 8)[:n - 1] + last if n > 1 else last


LENGTHS = (1, 7, 8, 9, 63, 64, 65, 254)


@pytest.fixture(scope="module")
def designed(tmp_path_factory):
    fields = [b"a\0", b"ab\0", b"abc\0",                                  # prefixes of each other
              b"tail-A\0", b"tail-B\0", b"A-head\0", b"B-head\0",           # the last byte, the first byte
              b"\x80\xff\xfe\0", b"\x80\xff\xfd\0", b"caf\xc3\xa9\0",       # bytes of 0x80 and above
              b"ab\0cd\0", b"zz\0ab\0", b"\0", b"\0ab\0"]                   # a NUL inside the field; l_read_name = 1; an empty name in front of bytes
    for n in LENGTHS:
        fields += [name_of_length(n, b"x") + b"\0", name_of_length(n, b"y") + b"\0"]
    recs = [record(f) for f in fields]
    recs += [record(b"quad\0", fl) for fl in (0, 0x100, 0x800, 4)]         # primary, secondary, supplementary, unmapped
    path = str(tmp_path_factory.mktemp("designed") / "d.bam")
    write_bam(path, recs)
    return path, recs


@pytest.mark.parametrize("ids", [
    [b"ab"],                                                                # a, abc, zz stay out; the field ab\0cd\0 matches
    [b"ab\0cd", b"cd", b"abcd"],                                            # what no record's name can be
    [b"tail-A", b"B-head"],
    [b"\x80\xff\xfe", b"caf\xc3\xa9"],
    [name_of_length(n, b"x") for n in LENGTHS],
    [name_of_length(n, b"y") for n in LENGTHS] + [name_of_length(255, b"x"), b""],
    [b"quad"],
    [b"", b"\0", b"x" * 255, b"x" * 300],                                   # ignored for matching
], ids=lambda v: "ids%d" % len(v))
def test_designed_names(designed, ids):
    path, recs = designed
    exp = expected_match(recs, ids)
    got = device_match(path, ids)
    assert got.dtype == np.uint8 and np.array_equal(got, exp), (ids, got.tolist(), exp.tolist())


def test_designed_names_counts_and_outputs(tmp_path, designed):
    path, recs = designed
    header = read_bam(path)[0]
    ids = [b"quad", b"ab", b"", b"x" * 255, b"p\0q", b"ab", b"x" * 255, name_of_length(254, b"x")]
    out, out2 = str(tmp_path / "o.bam"), str(tmp_path / "o2.bam")
    got = device_extract(path, out, ids, out2)
    assert got["names"] == 6   # quad, ab, the empty name, 255 x, p\0q, the 254-byte name: what cannot match still counts once
    e1, _ = check_against_oracle(header, recs, ids, out, out2, got, "designed")
    assert [X.Rec(b).flag for b in e1 if X.name_of(b) == b"quad"] == [0, 0x100, 0x800, 4]   # all four, in file order
    assert got["out"] == 4 + 2 + 1


@pytest.fixture(scope="module")
def placed(tmp_path_factory):
    """3000 records of unique names in members of 4000 bytes: with NGSQC_TILE_MEMBERS=2 a tile ends every 8000 inflated bytes"""
    recs = [record(b"f%d:%s\0" % (i, b"n" * (i % 23)), l_seq=12 + i % 40) for i in range(3000)]
    path = str(tmp_path_factory.mktemp("placed") / "p.bam")
    hdr = write_bam(path, recs, member=4000)
    starts = np.cumsum([hdr] + [len(b) for b in recs])[:-1]
    return path, recs, starts


def test_matches_at_wave_and_tile_edges(placed):
    path, recs, starts = placed
    ends = starts + np.array([len(b) for b in recs])
    carried, first, last = [], [], []
    for edge in range(8000, int(ends[-1]), 8000):
        i = int(np.searchsorted(starts, edge, side="right")) - 1   # the record that holds the byte in front of which the tile ends
        if starts[i] == edge: first.append(i); last.append(i - 1)
        else: carried.append(i); first.append(min(i + 1, len(recs) - 1)); last.append(i - 1)
    assert len(carried) > 10
    for picks in ([0, 63, 64, 127, 128, len(recs) - 1], carried, first, last, sorted(set(carried + first + last + [0, len(recs) - 1]))):
        ids = [X.name_of(recs[i]) for i in picks]
        exp = expected_match(recs, ids)
        assert int(exp.sum()) == len(set(picks))
        for env in ({}, {"NGSQC_TILE_MEMBERS": "2"}, {"NGSQC_TILE_MEMBERS": "3"}):
            got = with_env(env, lambda: device_match(path, ids))
            assert np.array_equal(got, exp), (env, picks[:8], np.flatnonzero(got != exp)[:8].tolist())


# ---- 6. set sizes ----
def test_no_names_everything_goes_to_out2(tmp_path, placed):
    path, recs, _ = placed
    header = read_bam(path)[0]
    ids = tmp_path / "ids.txt"; ids.write_bytes(b"# nothing\n\n")
    out, out2 = str(tmp_path / "o.bam"), str(tmp_path / "o2.bam")
    r = subprocess.run([TOOL, "-in", path, "-ids", str(ids), "-out", out, "-out2", out2], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "Read IDs: 0\nReads written to 'out': 0\nReads written to 'out2': 3000\n"
    assert read_bam(out) == (header, []) and read_bam(out2) == (header, recs)
    reopen_ok(out, 0); reopen_ok(out2, 3000)
    assert not device_match(path, []).any()


@pytest.mark.parametrize("n_names", [1, 1023, 1024, 1025])   # (the table doubles behind 1024 names)
def test_set_sizes_around_a_table_step(tmp_path, placed, n_names):
    path, recs, _ = placed
    own = [X.name_of(recs[i]) for i in range(0, 3000, 7)][:n_names // 2 + 1]
    ids = own + [b"other:%d" % i for i in range(n_names - len(own))]
    assert len(set(ids)) == n_names
    exp = expected_match(recs, ids)
    assert np.array_equal(device_match(path, ids), exp) and int(exp.sum()) == len(own)
    out = str(tmp_path / "o.bam")
    got = device_extract(path, out, ids)
    assert got == dict(out=len(own), out2=0, names=n_names)
    assert read_bam(out)[1] == [b for b, m in zip(recs, exp) if m]


def test_large_set_and_duplicates(tmp_path, placed):
    path, recs, _ = placed
    own = [X.name_of(recs[i]) for i in range(5, 3000, 11)]
    ids = [b"gen:%d:%d" % (i, i * 2654435761 % 1000003) for i in range(200_000 - len(own))] + own
    random.Random(9).shuffle(ids)
    exp = expected_match(recs, own)
    assert np.array_equal(device_match(path, ids), exp)
    out, dup = str(tmp_path / "o.bam"), str(tmp_path / "d.bam")
    got = device_extract(path, out, ids)
    assert got == dict(out=len(own), out2=0, names=200_000)
    # every name twice: the loaded count is that of the single list, the file the same
    assert device_extract(path, dup, ids + ids[::-1]) == got
    assert open(dup, "rb").read() == open(out, "rb").read()
    assert read_bam(out)[1] == [b for b, m in zip(recs, exp) if m]


# ---- 7. determinism ----
def test_two_runs_give_identical_files(tmp_path):
    src = os.path.join(GI, "MappingQC_in1.bam")
    ids = third_of_names(read_bam(src)[1], 2) + FOREIGN
    files = []
    for k in range(2):
        out, out2 = str(tmp_path / f"o{k}.bam"), str(tmp_path / f"p{k}.bam")
        device_extract(src, out, ids, out2)
        files.append((open(out, "rb").read(), open(out2, "rb").read()))
    assert files[0] == files[1]


# ---- errors ----
def test_partial_handles_are_refused(tmp_path):
    src = os.path.join(GI, "BamDownsample", "BamDownsample_in1.bam")
    h = ngsqc.Handle(path=src)
    name, ln = h.refs[0]
    h.close()
    for kw in (dict(regions=[(name, 1, ln)]), dict(shard=(0, 2))):
        h = ngsqc.Handle(path=src, **kw)
        try:
            for call in (lambda: h.extract(str(tmp_path / "x.bam"), [b"a"]), lambda: h.match_names([b"a"])):
                with pytest.raises(ngsqc.NgsqcError) as e:
                    call()
                assert e.value.code == -3 and "BamExtract needs a handle on the whole file (not a shard, a range or regions)" in str(e.value)
        finally:
            h.close()
    assert not os.path.exists(str(tmp_path / "x.bam"))


def test_cram_output_is_refused(tmp_path):
    out = str(tmp_path / "o.cram")
    r = subprocess.run([TOOL, "-in", OUT1, "-ids", IDS, "-out", out], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "CRAM output is not supported: " + out + ". Write a '.bam' file." in r.stderr and not os.path.exists(out)
