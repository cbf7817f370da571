"""BamFilter on the GPU (ngsqc_filter_pairs: csrc/pairs.hip + csrc/deflate.hip; bin/BamFilter) against the reference's expected BAMs
(src/tools-TEST/BamFilter_Test.cpp) and against the Python restatement (tests/bamfilter_oracle.py). Outputs are read back with Python's gzip, and through
ngsqc_open, whose K1 checks every member's CRC."""
import glob
import os
import random
import struct
import subprocess

import pytest

import bamfilter_oracle as F
import bamgen_lib as G
import cram_twin

ngsqc = __import__("importlib").import_module("ngs-bits_amd")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GI = os.path.join(ROOT, "tests", "golden", "ref_in")
GO = os.path.join(ROOT, "tests", "golden", "ref_out")
GBF = os.path.join(GI, "BamFilter")   # BamFilter_Test.cpp's inputs
TOOL = os.path.join(ROOT, "ngs-bits_amd", "bin", "BamFilter")
SWEEP = [{}, {"min_mq": 0}, {"min_mq": 60}, {"max_mq": 50}, {"max_mm": -1}, {"max_mm": 0}, {"max_gap": -1}, {"max_gap": 0}, {"max_gap": 3},
         {"min_dup": 1}, {"max_is": -1}, {"max_is": 300}]


def reopen_ok(path, n_expected):
    h = ngsqc.Handle(path=path)
    try:
        assert h.n_records == n_expected
    finally:
        h.close()


def device_filter(path, out, **kw):
    h = ngsqc.Handle(path=path)
    try:
        return h.filter_pairs(out, **kw)
    finally:
        h.close()


def assert_equal_to_oracle(src, out, got, **kw):
    header, exp, passed, dropped = F.filter_file(src, **kw)
    h, recs = F.read_bam(out)
    assert h == header
    assert len(recs) == len(exp) and recs == exp, (src, kw)
    assert got == (passed, dropped), (src, kw, got, passed, dropped)


@pytest.mark.parametrize("inp,args,exp", [("BamFilter_in1.bam", [], "BamFilter_out1.bam"), ("BamFilter_in2.bam", ["-minMQ", "50"], "BamFilter_out2.bam"),
                                          ("BamFilter_in2.bam", ["-maxMQ", "50"], "BamFilter_out3.bam")])
def test_tool_reference_cases(tmp_path, inp, args, exp):
    out = str(tmp_path / "out.bam")
    r = subprocess.run([TOOL, "-in", os.path.join(GBF, inp), "-out", out] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    h, recs = F.read_bam(out)
    eh, erecs = F.read_bam(os.path.join(GO, exp))
    assert h == eh and recs == erecs
    kw = {"min_mq": 50} if "-minMQ" in args else {"max_mq": 50} if "-maxMQ" in args else {}
    _, _, passed, dropped = F.filter_file(os.path.join(GBF, inp), **kw)
    assert r.stdout == f"pairs passed: {passed}\npairs dropped: {dropped}\n"
    reopen_ok(out, len(erecs))


@pytest.mark.parametrize("bam", sorted(os.path.relpath(p, GI) for p in glob.glob(os.path.join(GI, "*.bam")) + glob.glob(os.path.join(GBF, "*.bam"))))
def test_filter_pairs_matches_restatement(tmp_path, bam):
    src = os.path.join(GI, bam)
    h = ngsqc.Handle(path=src)
    try:
        for i, kw in enumerate(SWEEP):
            out = str(tmp_path / f"o{i}.bam")
            got = h.filter_pairs(out, **kw)
            assert_equal_to_oracle(src, out, got, **kw)
    finally:
        h.close()


# ---- an adversarial BAM ----
def _aux_int(tag, t, v):
    return tag + t.encode() + struct.pack({"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[t], v)


def _record(rng, name, flag, tid, pos, mapq, cigar, l_seq, isize, aux, cg_ops=None):
    n = name.encode() + b"\0"
    seq = bytes(rng.randrange(256) for _ in range((l_seq + 1) // 2)); qual = bytes(rng.randrange(2, 41) for _ in range(l_seq))
    ops = [(l_seq, 4), (sum(l for l, o in cg_ops if o in (0, 2, 3, 7, 8)) or 1, 3)] if cg_ops else cigar
    if cg_ops:
        aux = aux + b"CGBI" + struct.pack("<I", len(cg_ops)) + b"".join(struct.pack("<I", l << 4 | o) for l, o in cg_ops)
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(n), mapq, 4680, len(ops), flag, l_seq, tid, pos + 100, isize) + n
    body += b"".join(struct.pack("<I", l << 4 | o) for l, o in ops) + seq + qual + aux
    return struct.pack("<I", len(body)) + body


def adversarial_records(seed=3, n_names=1500):
    rng = random.Random(seed)
    recs = []
    nm_types = ["c", "C", "s", "S", "i", "I", "f", None]
    for k in range(n_names):
        name = f"q{k}:{rng.randrange(10**6)}" + ("x" * rng.randrange(0, 40))
        for c in range(rng.choice([1, 2, 2, 2, 3, 4, 5])):
            flag = 1 | (0x40 if c % 2 == 0 else 0x80)
            u = rng.random()
            if u < 0.05: flag |= 4
            elif u < 0.10: flag |= 8
            elif u < 0.13: flag &= ~1
            if rng.random() < 0.08: flag |= rng.choice([0x100, 0x800])
            l_seq = rng.randrange(20, 160)
            ins, dl = rng.randrange(0, 3), rng.randrange(0, 3)
            cigar = [(l_seq - ins - 5, 0)] + ([(ins, 1)] if ins else []) + ([(dl, 2)] if dl else []) + [(5, 0)]
            aux = b""
            t = rng.choice(nm_types)
            if t == "f": aux += b"NMf" + struct.pack("<f", 1.0)
            elif t: aux += _aux_int(b"NM", t, rng.randrange(0, 7))
            aux += b"RGZgrp\0"
            t = rng.choice(nm_types)
            if t == "f": aux += b"DPf" + struct.pack("<f", 2.0)
            elif t: aux += _aux_int(b"DP", t, rng.randrange(0, 3))
            isize = rng.choice([-1, 1]) * rng.randrange(0, 600)
            cg = None
            if rng.random() < 0.04:   # a long-read style record: the real CIGAR in CG:B,I
                cg = [(l_seq - 4, 0), (2, 1), (2, 0), (rng.randrange(1, 4), 2)]
            recs.append(_record(rng, name, flag, rng.randrange(2), rng.randrange(1, 900000), rng.choice([0, 20, 30, 45, 60, 255]), cigar, l_seq, isize, aux, cg))
    rng.shuffle(recs)   # mates lie tiles apart
    return recs


@pytest.fixture(scope="module")
def adversarial(tmp_path_factory):
    d = tmp_path_factory.mktemp("adv")
    path = str(d / "adv.bam")
    # members of a few KB: many tiles under NGSQC_TILE_MEMBERS
    recs = adversarial_records()
    text = "@HD\tVN:1.6\n@SQ\tSN:c1\tLN:1000000\n@SQ\tSN:c2\tLN:1000000\n"
    hdr = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", 2)
    for nm in ("c1", "c2"):
        hdr += struct.pack("<i", 3) + nm.encode() + b"\0" + struct.pack("<i", 1000000)
    raw = hdr + b"".join(recs)
    out = b"".join(cram_twin._bgzf(raw[o:o + 4000]) for o in range(0, len(raw), 4000)) + cram_twin._bgzf(b"")
    open(path, "wb").write(out)
    return path


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


def test_adversarial_matches_restatement(tmp_path, adversarial):
    _, recs = F.read_bam(adversarial)
    assert any(F.Rec(r).cg() for r in recs)
    for kw in ({}, {"min_mq": 0, "max_mm": -1, "max_gap": -1}, {"min_dup": 1, "max_is": 300}):
        out = str(tmp_path / "a.bam")
        assert_equal_to_oracle(adversarial, out, device_filter(adversarial, out, **kw), **kw)
        out4 = str(tmp_path / "a4.bam")
        got4 = _with_env({"NGSQC_NAME_HASH_BITS": "4"}, lambda: device_filter(adversarial, out4, **kw))
        assert_equal_to_oracle(adversarial, out4, got4, **kw)
        assert open(out, "rb").read() == open(out4, "rb").read()


def test_tiles_give_identical_bytes(tmp_path, adversarial):
    kw = {"min_mq": 0, "max_mm": -1, "max_gap": -1}
    one = str(tmp_path / "one.bam")
    got = device_filter(adversarial, one, **kw)
    assert_equal_to_oracle(adversarial, one, got, **kw)
    reopen_ok(one, 2 * got[0])
    for k in ("2", "3"):
        out = str(tmp_path / f"t{k}.bam")
        assert _with_env({"NGSQC_TILE_MEMBERS": k}, lambda: device_filter(adversarial, out, **kw)) == got
        assert open(out, "rb").read() == open(one, "rb").read(), k


def test_cram_input_equals_bam_twin(tmp_path):
    import cram_encode as CE
    t = cram_twin.make_twin(os.path.join(GI, "MappingQC_in2.bam"), str(tmp_path), max_records=20000)
    cram = str(tmp_path / "twin.cram"); CE.encode(t["bam"], cram, t["genome"])
    a, b = str(tmp_path / "from_bam.bam"), str(tmp_path / "from_cram.bam")
    kw = {"min_mq": 0, "max_mm": -1}
    ga = device_filter(t["bam"], a, **kw)
    ngsqc.set_reference(t["fasta"])
    try:
        gb = device_filter(cram, b, **kw)
    finally:
        ngsqc.set_reference(None)
    assert ga == gb and ga[0] > 0
    assert F.read_bam(a)[1] == F.read_bam(b)[1]


def test_shard_handle_is_refused(tmp_path):
    h = ngsqc.Handle(path=os.path.join(GI, "MappingQC_in2.bam"), shard=(0, 2))
    try:
        with pytest.raises(ngsqc.NgsqcError) as e:
            h.filter_pairs(str(tmp_path / "x.bam"))
        assert "whole file" in str(e.value)
    finally:
        h.close()


def test_bamgen_million_reads(tmp_path):
    src = str(tmp_path / "g.bam")
    G.write(src, n_reads=1_000_000, flavor=8)   # (flavor bit 3: mates share read names)
    out = str(tmp_path / "o.bam")
    got = device_filter(src, out)
    assert got[0] > 100_000
    assert_equal_to_oracle(src, out, got)
    reopen_ok(out, 2 * got[0])


def test_small_output_windows_give_identical_bytes(tmp_path, adversarial):
    """the writer's windows of the output stream (NGSQC_WRITE_WINDOW_PIECES: pieces of 0xff00 bytes) do not change a byte, alone and with many tiles"""
    kw = {"min_mq": 0, "max_mm": -1, "max_gap": -1}
    one = str(tmp_path / "one.bam")
    got = device_filter(adversarial, one, **kw)
    ref = open(one, "rb").read()
    assert len(ref) > 3 * 0xff00 // 4   # (several pieces of output)
    for env in ({"NGSQC_WRITE_WINDOW_PIECES": "1"}, {"NGSQC_WRITE_WINDOW_PIECES": "3"}, {"NGSQC_WRITE_WINDOW_PIECES": "1", "NGSQC_TILE_MEMBERS": "2"}):
        out = str(tmp_path / "w.bam")
        assert _with_env(env, lambda: device_filter(adversarial, out, **kw)) == got
        assert open(out, "rb").read() == ref, env


def test_bamgen_small_windows(tmp_path):
    src = str(tmp_path / "g.bam")
    G.write(src, n_reads=200_000, flavor=8)
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    got = device_filter(src, a)
    assert got[0] > 20_000
    assert _with_env({"NGSQC_WRITE_WINDOW_PIECES": "2"}, lambda: device_filter(src, b)) == got
    assert open(a, "rb").read() == open(b, "rb").read()


def _single_bam(path, recs):
    text = "@HD\tVN:1.6\n@SQ\tSN:c1\tLN:1000000\n"
    raw = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", 1) + struct.pack("<i", 3) + b"c1\0" + struct.pack("<i", 1000000) + b"".join(recs)
    open(path, "wb").write(b"".join(cram_twin._bgzf(raw[o:o + 60000]) for o in range(0, len(raw), 60000)) + cram_twin._bgzf(b""))


def test_cg_cigar_of_more_than_65535_operations(tmp_path):
    """a kept record with a CG-tag CIGAR of 65540 operations is written as the placeholder "l_seq S, ref_len N" with CG:B,I behind the other tags;
    its mate, with 4 operations, inline without the tag"""
    rng = random.Random(9)
    long_ops = [(1, 0), (1, 2)] * 32770            # 65540 operations: 32770 bases, 65540 reference bases
    short_ops = [(46, 0), (2, 1), (2, 0), (3, 2)]   # 50 bases
    aux = _aux_int(b"NM", "C", 0)
    recs = [_record(rng, "long1", 0x41, 0, 1000, 60, None, 32770, 300, aux, long_ops),
            _record(rng, "long1", 0x81, 0, 1200, 60, None, 50, -300, aux, short_ops),
            _record(rng, "long2", 0x41, 0, 5000, 60, None, 50, 300, aux, short_ops),
            _record(rng, "long2", 0x81, 0, 5200, 60, None, 32770, -300, aux, long_ops)]
    src = str(tmp_path / "cg.bam"); _single_bam(src, recs)
    out = str(tmp_path / "o.bam")
    kw = {"max_mm": -1, "max_gap": -1}
    got = device_filter(src, out, **kw)
    assert got == (2, 0)
    assert_equal_to_oracle(src, out, got, **kw)
    _, written = F.read_bam(out)
    for b in written:
        r = F.Rec(b)
        if r.l_seq == 32770:
            assert r.n_cigar == 2 and r.cigar == [32770 << 4 | 4, 65540 << 4 | 3]
            assert r.aux()[-1][0] == b"CG" and r.cg() is not None and len(r.cg()[0]) == 65540
        else:
            assert r.n_cigar == 4 and all(t != b"CG" for t, _, _, _ in r.aux())
    reopen_ok(out, 4)


def test_cram_selection_handle_is_refused(tmp_path):
    import cram_encode as CE
    t = cram_twin.make_twin(os.path.join(GI, "MappingQC_in2.bam"), str(tmp_path), max_records=5000)
    cram = str(tmp_path / "twin.cram"); CE.encode(t["bam"], cram, t["genome"])
    name, ln = t["refs"][0]
    ngsqc.set_reference(t["fasta"])
    try:
        h = ngsqc.Handle(path=cram, regions=[(name, 1, min(ln, 1000))])
        try:
            with pytest.raises(ngsqc.NgsqcError) as e:
                h.filter_pairs(str(tmp_path / "x.bam"))
            assert "whole file" in str(e.value)
        finally:
            h.close()
    finally:
        ngsqc.set_reference(None)
