"""The members of tests/test_cpu_k1_symbol_bytes.py - every match length 3..258 (258 in both spellings), every distance symbol with its extra-bits patterns,
in a dynamic and in a fixed block, the match in each of the three places of a trip - on the device: one BGZF image through the library, the way
tests/test_gpu_inflate_designed.py feeds its catalogue, byte for byte against zlib's inflate of the same streams."""
import zlib

import numpy as np
import pytest

from test_cpu_k1_symbol_bytes import cases
from test_gpu_inflate_designed import bam_image

pytestmark = pytest.mark.gpu
ngsqc = __import__("importlib").import_module("ngs-bits_amd")

SWITCHES = {"default": {}, "no_park": {"NGSQC_P1_PARK": "0"}}


@pytest.fixture(scope="module")
def image():
    expect = [(name, zlib.decompress(comp, -15), comp) for name, _, comp in cases()]
    return expect, bam_image([(comp, raw, zlib.crc32(raw)) for _, raw, comp in expect])


@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_symbol_bytes_on_the_device(image, switch, monkeypatch):
    for k, v in SWITCHES[switch].items():
        monkeypatch.setenv(k, v)
    expect, (img, stream, first) = image
    h = ngsqc.Handle(data=np.frombuffer(img, dtype=np.uint8))
    try:
        h.decode()
        got = h.inflated()
        assert got.size == len(stream)
        want = np.frombuffer(stream, dtype=np.uint8)
        if not np.array_equal(got, want):
            at = int(np.flatnonzero(got != want)[0]); pos = len(stream) - sum(len(raw) for _, raw, _ in expect)
            for name, raw, _ in expect:
                if at < pos + len(raw):
                    raise AssertionError(f"{name}: first wrong byte at {at - pos} of {len(raw)}")
                pos += len(raw)
            raise AssertionError(f"first wrong byte at {at}, in the preamble")
        assert h.n_records == 1
    finally:
        h.close()
