"""Phase 2 of K1 (csrc/k1_kernels.h, lz77_groups_kernel: the text the library compiles) under the wave emulator of tests/emul on the designed members of
tests/k1_resolve_cases.py: every item length as a far and as a near item, long matches whose last item overlaps its predecessor, sources on every side of a
batch start (the P2_HIST edge), sources over a literal, a far item and a near item, dependency chains of depth 0..8 inside one near step and a chain across
near steps, distance-1 runs and self-overlapping distances, batches cut by each of the three limits, a table switch and stored blocks inside a member, last
batches with 0..7 odd bytes, members of 0 and 1 byte. zlib's inflate is the reference, byte for byte, with `produced` and `error` of every member.
No GPU needed; the same members on the device: tests/test_gpu_k1_resolve_designed.py."""
import zlib

import pytest

import deflate_build as B
import k1_resolve_cases as KC
from test_cpu_inflate_designed import check_named, layout, valid_members
from test_k1_emul import emul, run   # noqa: F401  (emul: the fixture that builds libk1.so)

VARIANTS = {"library_pool": {}, "worst_case_pool": dict(tok_mode=1), "three_resolver_waves": dict(p2=3), "file_order_no_parking": dict(order=0, park=0)}


def test_zlib_is_the_reference_of_every_case():
    names = [c[0] for c in KC.valid_cases()]
    for prefix in ("far", "near", "raw", "edge", "span", "chain", "kind", "cut", "block", "tail", "size"):
        assert KC.group(prefix), prefix
    assert {f"chain/depth_{d}" for d in range(9)} <= set(names) and {f"tail/last_batch_with_{r}_odd_bytes" for r in range(8)} <= set(names)
    for name, raw, comp in KC.valid_cases():
        d = zlib.decompressobj(-15)
        assert d.decompress(comp) == raw and d.eof, name
        assert len(raw) <= 8192 and len(comp) <= 8192, name
    assert [len(c[1]) for c in KC.group("size")] == [0, 1]
    name, comp, isize, _, code = KC.error_cases()[0]
    assert B.judge(comp, isize) is None and code == 13
    name, comp, raw, crc, code = KC.error_cases()[1]
    assert B.judge(comp, len(raw)) == raw and crc != zlib.crc32(raw) and code == 20


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_designed_members(emul, variant):
    cases = KC.valid_cases()
    img, mem = layout(valid_members(cases))
    got, st, _ = run(emul, img, mem, **VARIANTS[variant])
    check_named(cases, got, st)


def test_each_member_alone(emul):
    """a launch of its own per member: nothing a neighbour left in the staging bytes or the literal table can stand in for a missing byte"""
    for case in KC.valid_cases():
        img, mem = layout(valid_members([case]))
        got, st, _ = run(emul, img, mem)
        check_named([case], got, st)


@pytest.mark.parametrize("depth", KC.CHAIN_DEPTHS)
def test_chain_depth_is_the_number_of_rounds(emul, depth):
    """a chain of depth d in one near step takes d + 1 rounds: every round completes the items whose sources are complete, and whether another
    round is needed is known at the end of a round (stats: 9 = near steps, 11 = rounds, 12 = batches)"""
    case = next(c for c in KC.valid_cases() if c[0] == f"chain/depth_{depth}")
    img, mem = layout(valid_members([case]))
    got, st, stats = run(emul, img, mem)
    check_named([case], got, st)
    assert (stats[12], stats[9], stats[11]) == (1, 1, depth + 1)


def test_chain_across_near_steps(emul):
    case = next(c for c in KC.valid_cases() if c[0] == "chain/across_near_steps")
    img, mem = layout(valid_members([case]))
    got, st, stats = run(emul, img, mem)
    check_named([case], got, st)
    assert stats[12] == 1 and stats[9] == 3 and stats[11] == 180   # one batch, 180 near items in three near steps, every item a round of its own


def test_the_cuts_are_met(emul):
    """each cut case needs more batches than its other two limits alone would ask for"""
    want = {"cut/by_2032_bytes": lambda n: n * 2032 < 80 * 32, "cut/by_192_items_far": lambda n: n * 192 < 420, "cut/by_192_items_near": lambda n: n * 192 < 420,
            "cut/by_64_groups": lambda n: n * 64 * 8 < 1500, "cut/groups_of_four_258_byte_matches": lambda n: n * 2032 < 13 * 258}
    for name, too_few in want.items():
        case = next(c for c in KC.valid_cases() if c[0] == name)
        img, mem = layout(valid_members([case]))
        got, st, stats = run(emul, img, mem)
        check_named([case], got, st)
        assert not too_few(stats[12]), (name, stats[12])


def test_error_cases(emul):
    """the damaged member between two valid ones: error 13 (a match that reaches in front of the member), the neighbours unharmed. The member with the wrong
    CRC32 field is the CRC kernel's business (tests/test_gpu_k1_resolve_designed.py): the K1 kernels inflate it, bytes and `produced` as zlib says"""
    good = KC.group("edge")[:2]
    (n0, comp0, isize0, crc0, code0), (n1, comp1, raw1, crc1, _) = KC.error_cases()
    members = [(good[0][2], len(good[0][1]), zlib.crc32(good[0][1])), (comp0, isize0, crc0), (good[1][2], len(good[1][1]), zlib.crc32(good[1][1])), (comp1, len(raw1), crc1)]
    img, mem = layout(members)
    got, st, _ = run(emul, img, mem)
    assert st[1][1] == code0, st[1]
    for i, raw in ((0, good[0][1]), (2, good[1][1]), (3, raw1)):
        pos = sum(m[2] for m in mem[:i])
        assert st[i] == (len(raw), 0) and got[pos:pos + len(raw)] == raw, (i, st[i])
