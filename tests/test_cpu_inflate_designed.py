"""The K1 kernels (csrc/k1_kernels.h) on the catalogue of hand-built DEFLATE members (tests/inflate_cases.py, written with tests/deflate_build.py): legal
streams that zlib's encoder never emits - distances up to 32768, 15-bit codes with the all-ones code on a literal / EOB / a length symbol, incomplete codes
that zlib accepts, 258 as 284 + 31, dictated header run-length codings, block sequences, matches laid on the resolver's batch / item / history cuts - and one
damaged stream per check of the decoder. zlib judges the catalogue; the kernels' text runs under the wave emulator (tests/emul) in five launch shapes, with
every phase-1 case at all 16 alignments of its payload, and once more as a stand-alone program built with -fsanitize=address,undefined: there every member
but the page-end ones, of which it takes every 40th (sanitized_batches). No GPU needed; the same catalogue on the device: tests/test_gpu_inflate_designed.py."""
import struct
import subprocess
import zlib

import pytest

import deflate_build as B
import emul_build
import inflate_cases as IC
from test_k1_emul import emul, run   # noqa: F401  (emul: the fixture that builds libk1.so)

VARIANTS = {"library_pool": {}, "worst_case_pool": dict(tok_mode=1), "no_parking": dict(park=0), "park_all": dict(park=64), "file_order": dict(order=0)}


def layout(members, align=None):
    """members [(comp, usize, crc)] laid out as in a BGZF file: bytes in front (align: the payload starts at that offset mod 16; None: as
    emul/k1_emul_main.cpp places them), the payload, CRC32, ISIZE -> (image, [(payload offset, payload bytes, inflated bytes)])"""
    img = bytearray(); mem = []
    for i, (comp, usize, crc) in enumerate(members):
        img += b"\xa5" * (18 + (i * 7) % 16)
        if align is not None:
            img += b"\xa5" * ((align - len(img)) % 16)
        mem.append((len(img), len(comp), usize)); img += comp + struct.pack("<II", crc, usize)
    return bytes(img), mem


def valid_members(cases):
    return [(comp, len(raw), zlib.crc32(raw)) for _, raw, comp in cases]


def check_named(cases, got, st):
    pos = 0
    for i, (name, raw, _) in enumerate(cases):
        assert st[i] == (len(raw), 0), f"{name}: (produced, error) = {st[i]}"
        assert got[pos:pos + len(raw)] == raw, f"{name}: the inflated bytes differ"
        pos += len(raw)


def test_catalogue_counts():
    """nothing was dropped to fit a size limit, and every member fits BGZF"""
    for g, n in IC.N_VALID.items():
        assert len(IC.group(g)) == n, g
    assert len(IC.valid_cases()) == sum(IC.N_VALID.values()) and len(IC.invalid_cases()) == IC.N_INVALID
    for name, raw, comp in IC.valid_cases():
        assert len(comp) <= 65510 and len(raw) <= 65536, name
    for name, comp, isize, codes in IC.invalid_cases():
        assert len(comp) <= 65510 and 1 <= isize <= 65536 and codes and all(2 <= c <= 18 for c in codes), name


def test_zlib_accepts_every_valid_case():
    for name, raw, comp in IC.valid_cases():
        d = zlib.decompressobj(-15)
        assert d.decompress(comp) == raw and d.eof, name


def test_zlib_refuses_every_invalid_case():
    """the rule of test_k1_emul.py::test_damaged_streams: zlib raises, or does not reach the end of the stream, or returns another length than ISIZE"""
    for name, comp, isize, _ in IC.invalid_cases():
        assert B.judge(comp, isize) is None, name


def test_the_cut_cases_continue_with_zero_bits():
    """the two cut streams are prefixes of valid ones whose remaining bits are zero: behind the cut the decoder reads the zero CRC field"""
    cases = {c[0]: c for c in IC.invalid_cases()}
    assert B.judge(cases["cut_inside_a_header"][1] + b"\0") == b"a" and B.judge(cases["cut_inside_a_symbol"][1] + b"\0") == b"a"


@pytest.mark.parametrize("group", ["shape+block", "geom", "page"])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_valid_cases(emul, variant, group):
    cases = [c for g in group.split("+") for c in IC.group(g)]
    img, mem = layout(valid_members(cases))
    got, st, stats = run(emul, img, mem, **VARIANTS[variant])
    check_named(cases, got, st)
    if group == "page":
        assert stats[13] >= 1   # members whose token groups fill their last page exactly


def test_phase1_cases_at_every_alignment(emul):
    """every code-shape and block-structure case with its payload at each offset mod 16 (the decoder reads its input in aligned 16-byte pieces), in one launch"""
    cases = IC.group("shape") + IC.group("block")
    img = bytearray(); mem = []; order = []
    for a in range(16):
        for name, raw, comp in cases:
            img += b"\xa5" * (18 + (a - len(img) - 18) % 16)
            mem.append((len(img), len(comp), len(raw))); order.append((f"{name} at {a}", raw, comp)); img += comp + struct.pack("<II", zlib.crc32(raw), len(raw))
    assert [sum(1 for m in mem if m[0] & 15 == a) for a in range(16)] == [len(cases)] * 16
    got, st, _ = run(emul, bytes(img), mem)
    check_named(order, got, st)


def invalid_image():
    """every invalid member between two valid ones -> (members for layout(), cases in member order: (name, raw or None, codes))"""
    good = [c for c in IC.group("shape") + IC.group("block") if len(c[1]) < 3000]
    members, order = [], []
    for i, (name, comp, isize, codes) in enumerate(IC.invalid_cases()):
        g = good[i % len(good)]
        members.append((g[2], len(g[1]), zlib.crc32(g[1]))); order.append((g[0], g[1], None))
        members.append((comp, isize, IC.INVALID_CRC)); order.append((name, None, codes))
    g = good[-1]
    members.append((g[2], len(g[1]), zlib.crc32(g[1]))); order.append((g[0], g[1], None))
    return members, order


def check_invalid(order, mem, got, st):
    pos = 0
    for i, (name, raw, codes) in enumerate(order):
        if raw is None:
            assert st[i][1] in codes, f"{name}: error {st[i][1]}, expected one of {codes}"
        else:
            assert st[i] == (len(raw), 0) and got[pos:pos + len(raw)] == raw, f"{name} (beside an invalid member): {st[i]}"
        pos += mem[i][2]


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_invalid_cases(emul, variant):
    members, order = invalid_image()
    img, mem = layout(members)
    got, st, _ = run(emul, img, mem, **VARIANTS[variant])
    check_invalid(order, mem, got, st)


def test_distance_in_front_of_the_member_does_not_read_the_previous_member(emul):
    """the bytes of the previous member lie directly in front in the output buffer: the match must be refused, not served from them"""
    prev = next(c for c in IC.group("block") if c[0] == "block/distance_equals_position")
    bad = next(c for c in IC.invalid_cases() if c[0] == "distance_in_front_of_the_member")
    img, mem = layout([(prev[2], len(prev[1]), zlib.crc32(prev[1])), (bad[1], bad[2], 0)])
    got, st, _ = run(emul, img, mem)
    assert st[0] == (len(prev[1]), 0) and got[:len(prev[1])] == prev[1] and st[1][1] == 13


def _fnv(chunks):
    h = 1469598103934665603
    for c in chunks:
        for b in c:
            h = ((h ^ b) * 1099511628211) & 0xffffffffffffffff
    return h


SANITIZED_PAGE_STEP = 40   # the one sample of the sanitized run: every 40th of the 801 page-end members


def sanitized_batches():
    """what the sanitized program runs, one process per batch -> [(members for layout(), cases in member order)]: every invalid member between valid ones and
    EVERY code-shape, block-structure and geometry member; of the page-end members (literal-only, one code shape, 801 sizes) every SANITIZED_PAGE_STEP-th.
    (The batches are cut by running time: the hundred empty blocks are 64 000 wave iterations of the header passes, a minute under AddressSanitizer, which pays
    for every fiber switch, and the geometry group is two and a half minutes in one process; the page group would be several more.)"""
    geom, block = IC.group("geom"), IC.group("block")
    slow = [c for c in block if c[0] == "block/hundred_empty_fixed_blocks"]
    assert len(slow) == 1 and geom[-1][0] == "geom/last_token_is_a_match"
    members, order = invalid_image()
    batches = [(members, order)]
    # (geom[3::4] ends with the member whose last token is a match: it stays the last member of its image)
    for cases in (IC.group("shape") + [c for c in block if c not in slow], slow, IC.group("page")[::SANITIZED_PAGE_STEP], geom[0::4], geom[1::4], geom[2::4], geom[3::4]):
        batches.append((valid_members(cases), [(n, raw, None) for n, raw, _ in cases]))
    assert batches[-1][1][-1][0] == "geom/last_token_is_a_match"
    ran = [n for _, o in batches[1:] for n, _, _ in o]
    assert sorted(ran) == sorted(c[0] for c in IC.group("shape") + block + geom + IC.group("page")[::SANITIZED_PAGE_STEP])
    assert {c[0] for c in IC.invalid_cases()} <= {n for n, _, _ in order}
    return batches


def write_case_file(path, members):
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(members)))
        for comp, usize, _ in members:
            f.write(struct.pack("<II", len(comp), usize) + comp)


def test_sanitized_stand_alone_run(emul, tmp_path):
    """the emulator as a program of its own under AddressSanitizer and UndefinedBehaviorSanitizer (nothing is loaded into python) on the members of
    sanitized_batches(): exit status 0, the statuses of the shared library, the same bytes.
    (Before its Kraft sums were written without a shift of a negative value this run ended in CodeShape::add: "left shift of negative value".)"""
    exe = emul_build.program("k1_emul_main.cpp", tmp_path, sanitize=True)
    batches = sanitized_batches()
    procs = []
    for b, (members, _) in enumerate(batches):   # the batches side by side, each a process of its own
        write_case_file(tmp_path / f"cases{b}.bin", members)
        out, err = open(tmp_path / f"out{b}.txt", "w"), open(tmp_path / f"err{b}.txt", "w")
        procs.append((subprocess.Popen([exe, str(tmp_path / f"cases{b}.bin")], stdout=out, stderr=err), out, err))
    codes = []
    for pr, out, err in procs:
        codes.append(pr.wait()); out.close(); err.close()
    for b, (members, order) in enumerate(batches):
        assert codes[b] == 0, (tmp_path / f"err{b}.txt").read_text()[-3000:]
        lines = (tmp_path / f"out{b}.txt").read_text().split("\n")
        st_prog = [tuple(int(x) for x in ln.split()) for ln in lines[:len(members)]]
        img, mem = layout([(c, u, 0) for c, u, _ in members])   # (the program writes a zero CRC field behind every member)
        got, st, _ = run(emul, img, mem)
        assert st_prog == st, b
        check_invalid(order, mem, got, st)
        pos, ok = 0, []
        for i, m in enumerate(mem):
            if st[i][1] == 0:
                ok.append(got[pos:pos + m[2]])
            pos += m[2]
        assert lines[len(members)] == f"fnv {_fnv(ok):016x}", b
    # a process of its own per case that depends on what the header pass leaves in the lane's tables: no earlier block has been there
    case_file = tmp_path / "cases.bin"
    for name, comp, isize, codes in (c for c in IC.invalid_cases() if c[0] in IC.FRESH_STATE_CASES):
        write_case_file(case_file, [(comp, isize, 0)])
        p = subprocess.run([exe, str(case_file)], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        assert int(p.stdout.split()[1]) in codes, f"{name}: {p.stdout.splitlines()[0]}"
