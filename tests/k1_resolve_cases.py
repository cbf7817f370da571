"""Designed members for phase 2 of K1, the LZ77 resolve (csrc/k1_kernels.h, lz77_groups_kernel), shared by tests/test_cpu_k1_resolve_designed.py (wave emulator)
and tests/test_gpu_k1_resolve_designed.py (the library). Every member is written token by token with tests/deflate_build.py, is a few KB at most, and is
judged by zlib. Deterministic.

What the resolver makes of a token stream (the terms of the cases below):
  batch   up to 64 token groups (four words each), cut to <= 2032 output bytes and <= 192 items. A new DEFLATE block starts with a table group, which ENDS the
          batch in front of it: the first byte of a Huffman block that follows another block is the first byte of a batch - that is how the cases put a source
          at a known place relative to a batch start
  item    a match (or the raw run of a stored block) in pieces of at most 16 bytes; the last piece of a match longer than 16 overlaps its predecessor
  far     an item whose source ends at or in front of the batch start (loaded from the member's output), near: any other (copied inside the staging bytes, in
          dependency rounds, 64 near items per near step); the 16 bytes in front of the batch stay in the staging bytes (P2_HIST)
  kinds   a distance-1 match repeats the byte in front of it; a match with a distance of 2..15 below an item's length overlaps its own source

Items of one and two bytes only come from stored blocks (a match has three bytes at least) and a raw run is never near: as near items the lengths are 3..16.

valid_cases()  -> [(name, raw, comp)]
error_cases()  -> [(name, comp, raw (or the ISIZE a damaged stream claims), CRC32 field, the error number)]"""
import random
import zlib

import deflate_build as B
from inflate_cases import Member

P2_BMAX, P2_IMAX, P2_GROUPS, P2_HIST = 2032, 192, 64, 16   # csrc/k1_kernels.h
HEAD = 2200           # bytes of the literal block in front of the designed block: more than a batch holds, so a distance of HEAD reaches behind any batch start
ITEM_LENGTHS = list(range(1, 17))
LONG_LENGTHS = [17, 18, 31, 32, 33, 34, 47, 48, 49, 64, 65, 257, 258]
CHAIN_DEPTHS = list(range(9))


class Toks:
    """the tokens of a block that starts `base` bytes into the member; p = bytes of the block so far"""

    def __init__(self, rng, base):
        self.rng, self.base, self.t, self.p = rng, base, [], 0

    def lit(self, n=1):
        self.t += [self.rng.randrange(256) for _ in range(n)]; self.p += n; return self

    def m(self, length, dist):
        assert 3 <= length <= 258 and 1 <= dist <= self.base + self.p and dist <= 32768, (length, dist, self.base, self.p)
        self.t.append((length, dist)); self.p += length; return self

    def back(self, length, k):
        """a match whose source starts k bytes in front of the block (= of the batch, when the block is the second of its member)"""
        return self.m(length, self.p + k)


def _two_blocks(name, seed, fill, head=HEAD):
    """a block of `head` random literals, then the designed block: its first byte starts a batch"""
    rng = random.Random(seed)
    m = Member().auto([rng.randrange(256) for _ in range(head)])
    t = Toks(rng, head); fill(t)
    return m.auto(t.t, True).done(name)


def _one_block(name, seed, fill):
    rng = random.Random(seed)
    t = Toks(rng, 0); fill(t)
    return Member().auto(t.t, True).done(name)


def _far_lengths(t):
    for ln in range(3, 17):           # every source wholly in front of the batch, at odd and even addresses
        t.lit(ln % 3).m(ln, t.p + 100 + ln).m(ln, HEAD + t.p)
    for ln in LONG_LENGTHS:
        t.lit(1).m(ln, t.p + 300 + ln)


def _near_lengths(t):
    t.lit(20)
    for ln in range(3, 17):           # source in the batch: adjacent, a few bytes back, and as far back as the batch goes
        t.lit(ln + 2).m(ln, ln + 2).m(ln, ln).lit(1).m(ln, t.p)
    for ln in LONG_LENGTHS:           # (distance >= length: no item overlaps its own source; the last item overlaps its predecessor's place. The source is the block's
        t.lit(2).m(ln, t.p)           # first byte: near only while the batch that began there lasts, far behind its cut - the near long matches up to 258 are _near_long's)
        if t.p > 1500:
            break


def _near_long(t):
    t.lit(300)
    for ln in LONG_LENGTHS:
        t.lit(1).m(ln, 300)


def _hist_edge(t):
    # the first token of the batch and later ones: sources that END at the batch start (far), and that START 1, 15 and 16 bytes in front of it
    for ln in (3, 4, 8, 9, 16):
        t.back(ln, ln).lit(1)                         # [-ln, 0)
    for k in (1, 15, 16):
        for ln in (3, 4, 9, 15, 16, 17, 31, 40):      # k = 16: the first item of a long match is far, its next one near (it starts 15 in front at the latest)
            t.lit(2).back(ln, k)
    t.back(16, 15).back(3, 2).back(258, 16)


def _hist_edge_first_token(k, ln):
    return lambda t: t.back(ln, k).lit(3).back(ln, k)


def _spanning(t):
    # [far item A, 8 bytes] [literal] [near item B, 8 bytes] then matches whose source spans the end of A, the literal and the start of B
    for ln in (3, 5, 8, 12):
        t.lit(24)
        a = t.p; t.m(8, HEAD + 7).lit(1).m(8, 20)
        t.m(ln, t.p - (a + 8 - (ln // 2 if ln < 12 else 3)))
    # a long match over literals, far items and near items
    t.lit(5).m(40, 60).m(100, 120)


def _chain(depth, ln=8):
    def fill(t):
        t.lit(ln)
        for _ in range(depth + 1):    # each match copies the one before it: the (depth + 1)-th waits for `depth` others
            t.m(ln, ln)
    return fill


def _chains_all(t):
    for depth in CHAIN_DEPTHS:
        for ln in (3, 4, 7, 9, 16):
            t.lit(ln)
            for _ in range(depth + 1):
                t.m(ln, ln)
            if t.p > 1700:
                return


def _chain_across_steps(t):
    t.lit(4)
    for _ in range(150):              # 150 near items in one batch (three near steps), each waiting for its predecessor
        t.m(4, 4)
    t.lit(3)
    for _ in range(30):
        t.m(3, 3)


def _runs(t):
    for ln in list(range(3, 18)) + [31, 32, 33, 258]:
        t.lit(2).m(ln, 1)
    t.lit(1).m(258, 1).m(258, 1).m(20, 1)             # a run that goes on over several matches


def _self_overlap(t):
    for d in range(2, 16):
        for ln in (d + 1, 16, 17, 35):
            if ln > d:
                t.lit(d).m(ln, d)
        if t.p > 1600:
            t.lit(400)                                # (a new batch sooner or later: the periods also cross a cut)


def _cut_by_bytes(t):
    for _ in range(80):               # groups of four 32-byte matches: 128 bytes and 8 items a group - 2032 bytes are reached first
        t.m(32, HEAD)
    t.lit(3)


def _cut_by_items(t):
    for i in range(420):              # groups of four 5-byte matches: 20 bytes and 4 items a group - 192 items are reached first
        t.m(5, HEAD - 3 * (i % 7))


def _cut_by_items_near(t):
    t.lit(6)
    for i in range(420):
        t.m(5, 6 + (i % 5))


def _cut_by_groups(t):
    t.lit(1500)                       # eight bytes a group: 64 groups are reached first


def _groups_of_258(t):
    for _ in range(3):
        t.m(258, HEAD).m(258, 700).m(258, 258).m(258, 1)   # 1032 bytes and 68 items a group: one group per batch
    t.m(258, 5).lit(1)


def _odd_tail(r):
    return lambda t: t.lit(20).m(9, 20).m(11 + r, 7) if r else t.lit(24).m(16, 24)


def _stored_between(name, seed, sizes):
    rng = random.Random(seed)
    m = Member().auto([rng.randrange(256) for _ in range(300)] + [(30, 200), (5, 1)])
    for n in sizes:
        m.stored(bytes(rng.randrange(256) for _ in range(n)))
    n0 = len(m.raw)
    t = Toks(rng, n0)
    t.back(16, 16).back(17, 15).lit(1).m(40, 9).m(9, n0).lit(2).back(258, sum(sizes))
    return m.auto(t.t, True).done(name)


def _raw_lengths(seed):
    """stored blocks of every length 1..16 (items of one and two bytes exist only here), 17, 33, 256 and 300 (two raw runs), Huffman blocks between them"""
    rng = random.Random(seed)
    m = Member().auto([rng.randrange(256) for _ in range(40)])
    for n in ITEM_LENGTHS + [17, 33, 256, 300]:
        m.stored(bytes(rng.randrange(256) for _ in range(n)))
        if n % 3 == 0:
            m.auto([rng.randrange(256), (min(n, 258), n), (4, 2)])
    return m.auto([(3, 1), 7], True).done("raw/stored_blocks_of_every_item_length")


_valid = None


def valid_cases():
    global _valid
    if _valid is None:
        cs = [_two_blocks("far/every_item_length_and_long_matches", 1, _far_lengths),
              _two_blocks("near/every_item_length_and_long_matches", 2, _near_lengths),
              _one_block("near/every_item_length_first_batch", 3, _near_lengths),
              _one_block("near/long_matches_from_300_back", 4, _near_long),
              _raw_lengths(5),
              _two_blocks("edge/sources_around_the_batch_start", 6, _hist_edge),
              _two_blocks("edge/sources_around_the_batch_start_short_head", 7, _hist_edge, head=40)]
        for k, ln in ((16, 16), (15, 16), (16, 17), (1, 3), (15, 3), (16, 258)):
            cs.append(_two_blocks(f"edge/first_token_{k}_in_front_length_{ln}", 10 + k + ln, _hist_edge_first_token(k, ln)))
        cs.append(_two_blocks("span/literal_far_item_near_item", 30, _spanning))
        for depth in CHAIN_DEPTHS:
            cs.append(_one_block(f"chain/depth_{depth}", 40 + depth, _chain(depth)))
        cs += [_one_block("chain/every_depth_several_lengths", 50, _chains_all),
               _two_blocks("chain/every_depth_behind_a_block", 51, _chains_all),
               _one_block("chain/across_near_steps", 52, _chain_across_steps),
               _one_block("kind/distance_1_runs", 60, _runs),
               _two_blocks("kind/distance_1_runs_behind_a_block", 61, _runs),
               _one_block("kind/self_overlap_distances_2_to_15", 62, _self_overlap),
               _two_blocks("cut/by_2032_bytes", 70, _cut_by_bytes),
               _two_blocks("cut/by_192_items_far", 71, _cut_by_items),
               _one_block("cut/by_192_items_near", 72, _cut_by_items_near),
               _one_block("cut/by_64_groups", 73, _cut_by_groups),
               _two_blocks("cut/groups_of_four_258_byte_matches", 74, _groups_of_258),
               _two_blocks("block/table_switch_in_the_middle", 80, lambda t: t.back(16, 16).lit(1).back(40, 7).m(3, 1).m(258, HEAD)),
               _stored_between("block/stored_block_between_huffman_blocks", 81, [100]),
               _stored_between("block/stored_blocks_of_1_2_3_bytes_between_huffman_blocks", 82, [1, 2, 3, 17])]
        for r in range(8):
            cs.append(_one_block(f"tail/last_batch_with_{r}_odd_bytes", 90 + r, _odd_tail(r)))
        cs.append(Member().auto([], True).done("size/member_of_0_bytes"))
        cs.append(Member().auto([201], True).done("size/member_of_1_byte"))
        for name, raw, comp in cs:
            assert len(raw) <= 8192 and len(comp) <= 8192, (name, len(raw), len(comp))
            assert B.judge(comp, len(raw)) == raw, name
        assert len({c[0] for c in cs}) == len(cs)
        _valid = cs
    return _valid


def group(prefix):
    return [c for c in valid_cases() if c[0].startswith(prefix + "/")]


def error_cases():
    """(name, comp, raw or the ISIZE a damaged stream claims, CRC32 field, BlockStatus.error)
    - a match that reaches in front of the member: error 13 from the decoder (the resolver is never asked for it)
    - an intact stream whose CRC32 field is wrong: the K1 kernels inflate it (error 0), the CRC kernel of the library refuses it (K1_ERR_CRC = 20)
    The two numbers are written down here, not computed: 13 is what the parent's kernels give this member under the wave emulator (and what the catalogue of
    tests/inflate_cases.py expects of its own such member), 20 is K1_ERR_CRC of csrc/k1_types.h."""
    rng = random.Random(99)
    w = B.BitWriter(); B.auto_dynamic(w, [rng.randrange(256) for _ in range(30)] + [(5, 30), (9, 36)], True)
    m = Member().auto([rng.randrange(256) for _ in range(50)] + [(16, 50), (3, 1), (40, 7)], True)
    _, raw, comp = m.done("x")
    return [("error/match_in_front_of_the_member", w.bytes(), 30 + 5 + 9, 0, 13),
            ("error/wrong_crc", comp, raw, zlib.crc32(raw) ^ 0x00100000, 20)]
