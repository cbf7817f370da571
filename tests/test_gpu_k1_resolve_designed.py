"""Phase 2 of K1 on the device against the designed members of tests/k1_resolve_cases.py (judged by zlib and run under the wave emulator in
tests/test_cpu_k1_resolve_designed.py): every item length far and near, long matches, sources around a batch start, dependency chains inside and across
near steps, runs and self-overlapping distances, batches cut by each limit, table switches and stored blocks inside a member, odd tails, members of 0 and
1 byte. The members reach K1 as the payload of one oversized unmapped BAM record (tests/test_gpu_inflate_designed.py, bam_image); the inflated stream must
be zlib's, byte for byte, under the K1 switches. The two error members must be refused with the reference's read error: the match that reaches in front
of its member with K1's error 13, the intact stream with a wrong CRC32 field as a CRC32 mismatch - each naming exactly that member.
(The member of 0 bytes is in the image, but the library leaves members of ISIZE 0 out of its member table: it reaches K1 only on the CPU.)"""
import re
import zlib

import numpy as np
import pytest

import k1_resolve_cases as KC
from test_gpu_inflate_designed import SWITCHES, bam_image, valid_members

pytestmark = pytest.mark.gpu
ngsqc = __import__("importlib").import_module("ngs-bits_amd")


@pytest.fixture(scope="module")
def image():
    return bam_image(valid_members(KC.valid_cases()))


def _inflate(img):
    h = ngsqc.Handle(data=np.frombuffer(img, dtype=np.uint8))
    try:
        h.decode()
        return h.inflated(), h.n_records
    finally:
        h.close()


@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_designed_members(image, switch, monkeypatch):
    for k, v in SWITCHES[switch].items():
        monkeypatch.setenv(k, v)
    img, stream, first = image
    got, n_records = _inflate(img)
    assert got.size == len(stream)
    want = np.frombuffer(stream, dtype=np.uint8)
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0]); pos = len(stream) - sum(len(c[1]) for c in KC.valid_cases())
        for name, raw, _ in KC.valid_cases():
            if at < pos + len(raw):
                raise AssertionError(f"{name}: first wrong byte at {at - pos} of {len(raw)}")
            pos += len(raw)
        raise AssertionError(f"first wrong byte at {at}, in the preamble")
    assert n_records == 1


def _error_image(k):
    good = valid_members(KC.group("edge")[:2] + KC.group("chain")[:2])
    name, comp, raw, crc, code = KC.error_cases()[k]
    return bam_image(good[:2] + [(comp, raw, crc)] + good[2:]), code


@pytest.mark.parametrize("crc", ["crc_on", "crc_off"])
def test_match_in_front_of_the_member_is_refused(crc, monkeypatch):
    if crc == "crc_off":
        monkeypatch.setenv("NGSQC_VERIFY_CRC", "0")
    (img, _, first), code = _error_image(0)
    with pytest.raises(ngsqc.NgsqcError) as ei:
        _inflate(img)
    m = re.search(r"BGZF inflate failed in block (\d+), code (\d+)", str(ei.value))
    assert m and ei.value.code == -2 and "Could not read next alignment" in str(ei.value), str(ei.value)
    assert (int(m.group(1)), int(m.group(2))) == (first + 2, code) and code == 13, str(ei.value)


def test_wrong_crc_is_refused(monkeypatch):
    (img, stream, first), code = _error_image(1)
    assert code == 20
    with pytest.raises(ngsqc.NgsqcError) as ei:
        _inflate(img)
    assert "Could not read next alignment" in str(ei.value) and f"CRC32 mismatch in block {first + 2}" in str(ei.value) and ei.value.code == -2, str(ei.value)
    # the stream itself is intact: without the check it inflates to zlib's bytes
    monkeypatch.setenv("NGSQC_VERIFY_CRC", "0")
    got, n_records = _inflate(img)
    assert np.array_equal(got, np.frombuffer(stream, dtype=np.uint8)) and n_records == 1
    assert zlib.crc32(KC.error_cases()[1][2]) != KC.error_cases()[1][3]
