"""The mate join's own text (ngs-bits_amd/csrc/join_visit.h - what the GPU library compiles into join_resolve_kernel, held_bytes_kernel and the keys kernels of
BamFilter, BamToFastq, BamDownsample, BamRemoveVariants and BamClipOverlap) on the CPU over the designed cases (tests/join_cases.py): tests/emul/join_emul.cpp
plays the tiles, the held set and the two pools; pairs, counts, open records and held bytes must be the reference cache's (join_cases.model, itself held
against the three oracles). The same driver runs as a stand-alone program under AddressSanitizer and UBSan, and three value-only mutations of a scratch copy
of the header must each be caught by a named case.

The name rule is judged by the reference: BamAlignment::name() is bam_get_qname read as a C string (src/cppNGS/BamReader.h:69-72), DESIGN.md "What a name is"."""
import ctypes as C
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

import bamdownsample_oracle as D
import bamfilter_oracle as F
import bamtofastq_oracle as Q
import emul_build
import join_cases as K
from conftest import ROOT

CSRC = os.path.join(ROOT, "ngs-bits_amd", "csrc")
GI = os.path.join(ROOT, "tests", "golden", "ref_in")
BITS = (2, 4, 63)
TOOLS = ("filter", "downsample", "tofastq")


def load(so):
    L = C.CDLL(so)
    L.join_name_hash.restype = C.c_uint64; L.join_name_hash.argtypes = [C.c_char_p, C.c_int32]
    L.join_name_hash_mask.restype = C.c_uint64; L.join_name_hash_mask.argtypes = [C.c_int32]
    L.join_name_len.restype = C.c_int32; L.join_name_len.argtypes = [C.c_char_p, C.c_uint32]
    L.join_name_hash_z.restype = C.c_uint64; L.join_name_hash_z.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_int32)]
    L.join_same_name.restype = C.c_int32; L.join_same_name.argtypes = [C.c_char_p, C.c_char_p]
    L.join_emul.restype = C.c_int64
    L.join_emul.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 6
    return L


@pytest.fixture(scope="module")
def lib():
    return load(emul_build.library("join_emul.cpp", include=[CSRC]))


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in K.small_cases()}


def inputs(case, tool):
    """(records blob, offsets, tiles, part, pass) as the driver takes them; pass: BamFilter's defaults for "filter", every record for the other tools"""
    recs = case.records
    parsed = [F.Rec(b) for b in recs]
    off = np.cumsum([0] + [len(b) for b in recs]).astype(np.int64)
    part = np.array([K.takes_part(r, tool) for r in parsed], np.uint8)
    ok = np.array([F.alignment_pass(r, **F.DEFAULTS) if tool == "filter" else True for r in parsed], np.uint8)
    return np.frombuffer(b"".join(recs), np.uint8), off, np.array(case.tile_of, np.int32), part, ok, parsed


def emulate(L, case, tool, bits):
    blob, off, tiles, part, ok, _ = inputs(case, tool)
    n, nt = len(part), len(case.tiles)
    opener, kept = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.uint8)
    h_after, pool_after, open_idx, counts = np.zeros(nt + 1, np.int64), np.zeros(nt + 1, np.int64), np.zeros(n + 1, np.int64), np.zeros(4, np.uint64)
    H = L.join_emul(blob.ctypes.data, off.ctypes.data, tiles.ctypes.data, n, nt, part.ctypes.data, ok.ctypes.data, L.join_name_hash_mask(bits), opener.ctypes.data,
                    kept.ctypes.data, h_after.ctypes.data, pool_after.ctypes.data, open_idx.ctypes.data, counts.ctypes.data)
    assert H >= 0, ("held order", case.name, tool, bits, H)
    pairs = [(int(opener[i]), i, int(kept[i])) for i in range(n) if opener[i] >= 0]
    return dict(pairs=pairs, h=h_after[:nt].tolist(), pool=pool_after[:nt].tolist(), open=sorted(open_idx[:H].tolist()), counts=(int(counts[0]), int(counts[1])))


def expected(case, tool):
    _, _, _, _, ok, parsed = inputs(case, tool)
    pairs, still, hs, _ = K.model(case, tool)
    exp = [(o, c, int(ok[o] and ok[c])) for o, c in pairs]
    # what the held set keeps behind every tile: the whole record of an opener that passes, 36 + l_read_name bytes of one that does not
    pool, opened, i = [], {}, 0
    close_at = {o: c for o, c in pairs}
    for t in case.tiles:
        i += len(t)
        held = [o for o in list(close_at) + still if o < i and close_at.get(o, 1 << 60) >= i]
        pool.append(sum(len(case.records[o]) if ok[o] else 36 + parsed[o].l_name for o in held))
    kept = sum(k for _, _, k in exp)
    return dict(pairs=sorted(exp, key=lambda p: p[1]), h=hs, pool=pool, open=still, counts=(kept, len(exp) - kept))


def differences(L, case):
    """every (tool, bits, field) at which the driver and the reference cache differ, got / expected"""
    out = []
    for tool in TOOLS:
        exp = expected(case, tool)
        for bits in BITS:
            got = emulate(L, case, tool, bits)
            out += [(tool, bits, k, got[k], exp[k]) for k in exp if got[k] != exp[k]]
    return out


def test_hash_is_pinned(lib):
    for nm, v in K.PINNED.items():
        assert lib.join_name_hash(nm, len(nm)) == v == K.name_hash(nm), nm
    for bits in (1, 2, 4, 62, 63, 64):
        assert lib.join_name_hash_mask(bits) == K.name_hash_mask(bits)


def test_name_rule(lib, cases):
    fields = [b"ab\0", b"ab\0\0\0", b"ab\0cd\0", b"\0", b"a\0", b"abc", bytes(range(1, 255)) + b"\0", b"\0ab\0"]
    for f in fields:
        assert lib.join_name_len(f, len(f)) == len(f.split(b"\0", 1)[0])
    assert lib.join_name_len(b"abc", 0) == 0 and lib.join_name_len(b"abc", 2) == 2
    recs = [K.rec(f, K.F1) for f in fields]
    for a in recs:
        for b in recs:
            assert bool(lib.join_same_name(a, b)) == (F.Rec(a).name == F.Rec(b).name), (a[36:44], b[36:44])
    for c in cases.values():
        for b in c.records:
            r = F.Rec(b)
            assert lib.join_name_len(b[36:36 + r.l_name], r.l_name) == len(r.name)


def test_the_word_walks_are_the_byte_walks(lib):
    """name_len and name_hash_z read eight bytes a load: on fields of every length with the first NUL at every place (and bytes of every kind behind it, 0x80 and
    0x01 next to the NUL among them) they are the byte-wise definitions, and same_name is the comparison of the names"""
    import random
    rng = random.Random(11)
    fields = []
    for l in list(range(0, 40)) + [63, 64, 65, 254, 255]:
        for z in sorted({0, 1, 7, 8, 9, 15, 16, 17, l - 2, l - 1, l} & set(range(l + 1))):
            body = bytes(rng.choice([1, 0x80, 0xff, 0x41, 0x7f, 0x81]) for _ in range(z))
            tail = bytes(rng.choice([0, 0, 1, 0x80, 0x41]) for _ in range(max(0, l - z - 1)))
            fields.append((body + (b"\0" + tail if z < l else b""))[:l])
    n = C.c_int32()
    for f in fields:
        name = f.split(b"\0", 1)[0]
        pad = f + b"\x01" * 16   # (what lies behind the field is not NUL: a read past l_read_name would change the answer)
        assert lib.join_name_len(pad, len(f)) == len(name), f
        assert lib.join_name_hash_z(pad, len(f), C.byref(n)) == K.name_hash(name) and n.value == len(name), f
    recs = [K.rec(f, K.F1) for f in fields if 1 <= len(f)]
    for a in recs[::3]:
        for b in recs[::2]:
            assert bool(lib.join_same_name(a, b)) == (F.Rec(a).name == F.Rec(b).name)


@pytest.mark.parametrize("name", [f.__name__ for f in K.SMALL])
def test_case_through_the_join(lib, cases, name):
    assert differences(lib, cases[name]) == []


@pytest.mark.parametrize("name", [f.__name__ for f in K.SMALL])
def test_the_model_is_the_oracles(cases, name):
    """join_cases.model against the three restated tools: counts, the written pairs in order, the open names"""
    case = cases[name]
    recs = case.records
    pairs, still, _, peak = K.model(case, "filter")
    out, passed, dropped = F.filter_pairs(recs)
    ok = [F.alignment_pass(F.Rec(b), **F.DEFAULTS) for b in recs]
    kept = [(o, c) for o, c in pairs if ok[o] and ok[c]]
    assert (passed, dropped) == (len(kept), len(pairs) - len(kept))
    assert out == [F.written(F.Rec(recs[i])) for o, c in sorted(kept, key=lambda p: p[1]) for i in (o, c)]
    pairs, still, _, peak = K.model(case, "tofastq")
    _, _, c = Q.to_fastq(recs)
    assert (c["paired"], c["unmatched"], c["max_cached"]) == (len(pairs), len(still), peak)
    _, _, dc, names = D.downsample(recs, 99.999, 1)
    assert (dc["pe"], dc["pe_unmatched"]) == (len(pairs), len(still))


def test_window_cuts_lie_where_designed():
    case = K.window_cuts_bam()
    out, passed, dropped = F.filter_pairs(case.records, **case.notes["kw"])
    assert dropped == 0 and passed == len(case.records) // 2
    K.window_cut_premises(case, out)
    assert len(b"".join(out)) < 4 << 20


def test_golden_names_hold_no_nul():
    """the rule changes nothing on the reference's files: every name field there is its name and one NUL"""
    n = 0
    for p in sorted(glob.glob(os.path.join(GI, "**", "*.bam"), recursive=True)):
        for b in F.read_bam(p)[1]:
            l = b[12]
            assert b[36 + l - 1] == 0 and 0 not in b[36:36 + l - 1], p
            n += 1
    assert n > 1000


def test_stand_alone_under_sanitizers(tmp_path, lib, cases):
    """the same driver as a program of its own under AddressSanitizer and UBSan: tiles, pools and inputs in heap buffers of exactly their size, freed when the
    device would reuse them; its output equals the library's"""
    exe = emul_build.program("join_emul_main.cpp", tmp_path, include=[CSRC], sanitize=True)
    for case in cases.values():
        for tool in ("filter", "tofastq"):
            blob, off, tiles, part, ok, _ = inputs(case, tool)
            for nm, a in (("recs", blob), ("offs", off), ("tiles", tiles), ("part", part), ("pass", ok)):
                (tmp_path / nm).write_bytes(a.tobytes())
            for bits in (2, 63):
                r = subprocess.run([exe] + [str(tmp_path / nm) for nm in ("recs", "offs", "tiles", "part", "pass")] + [str(bits)], capture_output=True, text=True, timeout=120)
                assert r.returncode == 0, (case.name, tool, bits, r.stderr[-2000:])
                got = emulate(lib, case, tool, bits)
                lines = ["pair %d %d %d" % p for p in got["pairs"]] + ["tile %d held %d bytes %d" % (t, h, b) for t, (h, b) in enumerate(zip(got["h"], got["pool"]))]
                assert r.stdout.split("\n")[:len(lines)] == lines, (case.name, tool, bits)
                assert r.stdout.rstrip("\n").split("\n")[-1] == "counts %d %d" % got["counts"]


# value-only mutations of the header's text (no address moves): (label, text, replacement, the cases that must notice)
MUTATIONS = [
    ("a run pairs one entry short", "for (; q + 1 < e; q += 2)", "for (; q + 2 < e; q += 2)", {"run_lengths", "held_chain", "empty_tile", "collisions", "no_part", "c_string_names"}),
    ("a closed entry is matched again", "if (o.st[r] == 1 && same_name(", "if (same_name(", {"collisions"}),
    ("a held name loses its last byte", "36ull + s[12]", "35ull + s[12]", {"held_chain", "empty_tile", "collisions", "c_string_names"}),
]


def test_mutations_are_caught(tmp_path, cases):
    text = open(os.path.join(CSRC, "join_visit.h")).read()
    table = {}
    for k, (label, old, new, must) in enumerate(MUTATIONS):
        d = tmp_path / ("m%d" % k); d.mkdir()
        assert text.count(old) == 1, label
        (d / "join_visit.h").write_text(text.replace(old, new))
        shutil.copy(os.path.join(CSRC, "rec.h"), d / "rec.h")
        L = load(emul_build.library("join_emul.cpp", d / "libjoin_mut.so", include=[d]))
        caught = {name for name, case in cases.items() if differences(L, case)}
        table[label] = sorted(caught)
        assert must <= caught, (label, sorted(caught))
    print(table)
