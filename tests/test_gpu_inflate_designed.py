"""K1 on the device against the catalogue of hand-built DEFLATE members (tests/inflate_cases.py; judged by zlib and run under the wave emulator in
tests/test_cpu_inflate_designed.py): streams no encoder of this suite emits - distances up to 32768, 15-bit codes, incomplete codes, dictated header
codings, block sequences, matches on the resolver's cuts - and one damaged member per check of the decoder. The members reach K1 as the payload of one
oversized unmapped BAM record behind a zlib-made preamble (header, the record's fixed part, 300 KB of filler: the designed members lie behind what an open
inflates for the header). Valid images must inflate byte for byte under the K1 switches; every damaged member must be refused with the reference's read
error, naming that member and one of the codes the catalogue allows, with and without the CRC kernel.
One case is CPU-only: shape/eob_only_member inflates to nothing, and the library leaves members of ISIZE 0 out of its member table (image.hip, walk_bgzf), so
on the device it is in the image but never reaches K1; the EOB-only block reaches K1 here as shape/eob_only_middle_block alone."""
import re
import struct
import zlib

import numpy as np
import pytest

import inflate_cases as IC
from test_gpu_inflate import EOF_MEMBER, member

pytestmark = pytest.mark.gpu
ngsqc = __import__("importlib").import_module("ngs-bits_amd")

BAM_HEADER = b"BAM\x01" + struct.pack("<i", 0) + struct.pack("<i", 1) + struct.pack("<i", 5) + b"chr1\x00" + struct.pack("<i", 1000000)
FILLER = 300000
SWITCHES = {"default": {}, "no_park": {"NGSQC_P1_PARK": "0"}, "tiles_of_2": {"NGSQC_TILE_MEMBERS": "2"},
            "second_chance": {"NGSQC_TILE_MEMBERS": "8", "NGSQC_TOKEN_POOL_FACTOR": "0.01"}}


def bgzf_member(comp, crc, isize):
    bsize = 18 + len(comp) + 8
    assert bsize <= 65536
    return b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize - 1) + comp + struct.pack("<II", crc & 0xffffffff, isize)


_filler = None


def filler():
    global _filler
    if _filler is None:
        rng = np.random.default_rng(41)
        _filler = (rng.integers(0, 6, FILLER, dtype=np.uint8) * 7 + 48).tobytes()
    return _filler


def bam_image(members):
    """members: [(comp, raw, crc)] - raw: the bytes a valid member inflates to, or the ISIZE an invalid one claims -> (BGZF image, the inflated stream it stands
    for (zeros where an invalid member sits), index of the first of the members). The stream is a BAM header and ONE unmapped record whose variable part is the
    filler and everything the members inflate to; header, fixed part and filler are zlib-made members of 30 000 bytes."""
    sizes = [len(r) if isinstance(r, bytes) else r for _, r, _ in members]
    var = b"r\x00" + filler()
    block_size = 32 + len(var) + sum(sizes)
    pre = BAM_HEADER + struct.pack("<i", block_size) + struct.pack("<iiBBHHHiiii", -1, -1, 2, 0, 4680, 0, 4, 0, -1, -1, 0) + var
    front = [member(pre[i:i + 30000]) for i in range(0, len(pre), 30000)]
    assert len(front) > 8
    body = [bgzf_member(comp, crc, n) for (comp, _, crc), n in zip(members, sizes)]
    stream = pre + b"".join(r if isinstance(r, bytes) else bytes(r) for _, r, _ in members)
    return b"".join(front + body) + EOF_MEMBER, stream, len(front)


def valid_members(cases):
    return [(comp, raw, zlib.crc32(raw)) for _, raw, comp in cases]


@pytest.fixture(scope="module")
def images():
    return {g: bam_image(valid_members([c for p in g.split("+") for c in IC.group(p)])) for g in ("shape+block", "geom", "page")}


def test_catalogue_is_whole():
    for g, n in IC.N_VALID.items():
        assert len(IC.group(g)) == n, g
    assert len(IC.invalid_cases()) == IC.N_INVALID


@pytest.mark.parametrize("switch", sorted(SWITCHES))
@pytest.mark.parametrize("group", ["shape+block", "geom", "page"])
def test_valid_members(images, group, switch, monkeypatch):
    for k, v in SWITCHES[switch].items():
        monkeypatch.setenv(k, v)
    image, stream, first = images[group]
    if group == "geom":
        assert IC.group("geom")[-1][0] == "geom/last_token_is_a_match"   # (the last data member of its image)
    h = ngsqc.Handle(data=np.frombuffer(image, dtype=np.uint8))
    try:
        h.decode()
        got = h.inflated()
        assert got.size == len(stream)
        want = np.frombuffer(stream, dtype=np.uint8)
        if not np.array_equal(got, want):
            at = int(np.flatnonzero(got != want)[0]); pos = len(stream) - sum(len(c[1]) for p in group.split("+") for c in IC.group(p))
            for name, raw, _ in (c for p in group.split("+") for c in IC.group(p)):
                if at < pos + len(raw):
                    raise AssertionError(f"{name}: first wrong byte at {at - pos} of {len(raw)}")
                pos += len(raw)
            raise AssertionError(f"first wrong byte at {at}, in the preamble")
        assert h.n_records == 1
        if switch == "second_chance":
            assert h.timings()["members_second_chance"] > 0
    finally:
        h.close()


def _neighbours():
    good = {c[0]: c for c in IC.group("shape") + IC.group("block")}
    return valid_members([good[n] for n in ("shape/all_ones_15_length", "block/distance_equals_position", "shape/header_16_run_over_eob", "block/final_empty_stored_block")])


@pytest.mark.parametrize("crc", ["crc_on", "crc_off"])
@pytest.mark.parametrize("case", IC.invalid_cases(), ids=lambda c: c[0])
def test_invalid_member_is_refused(case, crc, monkeypatch):
    """the damaged member between valid ones: the error names it and carries a code the catalogue allows; the same with the CRC kernel off, so it is the decoder that refuses"""
    if crc == "crc_off":
        monkeypatch.setenv("NGSQC_VERIFY_CRC", "0")
    name, comp, isize, codes = case
    nb = _neighbours()
    image, _, first = bam_image(nb[:2] + [(comp, isize, IC.INVALID_CRC)] + nb[2:])
    with pytest.raises(ngsqc.NgsqcError) as ei:
        h = ngsqc.Handle(data=np.frombuffer(image, dtype=np.uint8))
        try:
            h.decode()
        finally:
            h.close()
    m = re.search(r"BGZF inflate failed in block (\d+), code (\d+)", str(ei.value))
    assert m and ei.value.code == -2 and "Could not read next alignment" in str(ei.value), str(ei.value)
    assert int(m.group(1)) == first + 2 and int(m.group(2)) in codes, (name, str(ei.value), codes)


def test_the_neighbours_alone_are_accepted():
    """the image of the invalid cases without its damaged member inflates: the errors above are the damaged members'"""
    image, stream, _ = bam_image(_neighbours())
    h = ngsqc.Handle(data=np.frombuffer(image, dtype=np.uint8))
    try:
        h.decode()
        assert np.array_equal(h.inflated(), np.frombuffer(stream, dtype=np.uint8)) and h.n_records == 1
    finally:
        h.close()
