"""The device CRAM quality decoder (csrc/cram_dev_kernels.h) on the GPU, on the generated files of tests/qualgen.py - the ones tests/test_cram_dev_emul.py runs under
the wave emulator: crafted quality distributions in both rANS orders, reads against the 65280-byte payloads of the image, multi-reference slices, and a file of a few
thousand jobs (more workgroups than the device has compute units). A handle on the CRAM (device path, the default) against the handle on the BAM the CRAM was written
from and against the host path (NGSQC_CRAM_DEVICE_QUALS=0): the BAM stream byte for byte, the record count, and a depth scan with a base-quality threshold so that the
bytes are also seen through a kernel. The number of blocks the device decoded must be the number the gates of cram.hip let through, computed from the data - a gate
that moved cannot hide behind the host fallback. No damaged input here (tests/test_cram_dev_emul.py runs that on the CPU)."""
import os
import re

import numpy as np
import pytest

import qualgen
from conftest import GOLDEN_IN as GI
from test_cram_dev_emul import FIXTURE_JOBS

pytestmark = pytest.mark.gpu
ngsqc = __import__("importlib").import_module("ngs-bits_amd")

LINE = re.compile(r"cram: (\d+) quality blocks \((\d+) bytes, (\d+) records\) decoded on the device")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("qualgen")); out = {}
    out["shapes"] = qualgen.write(qualgen.shapes(), d, "shapes")
    out["records"] = qualgen.write(qualgen.record_shapes(), d, "records", slices_per_container=3)
    out["multi_ref"] = qualgen.write(qualgen.mapped_slices(n_slices=12), d, "mapped", multi_ref=True)
    with qualgen.cached_rans():
        out["many"] = qualgen.write(qualgen.many(3000), d, "many", slices_per_container=5)
    return out


def _open(capfd, monkeypatch, device, **kw):
    """-> (handle, quality blocks decoded on the device as the library reports them)"""
    monkeypatch.setenv("NGSQC_TIMING", "1"); monkeypatch.setenv("NGSQC_CRAM_NO_REFERENCE", "1")
    if device: monkeypatch.delenv("NGSQC_CRAM_DEVICE_QUALS", raising=False)
    else: monkeypatch.setenv("NGSQC_CRAM_DEVICE_QUALS", "0")
    capfd.readouterr(); ngsqc.set_reference(None)
    h = ngsqc.Handle(**kw)
    m = LINE.search(capfd.readouterr().err)
    return h, (int(m.group(1)), int(m.group(2)), int(m.group(3))) if m else (0, 0, 0)


@pytest.mark.parametrize("name", ["shapes", "records", "multi_ref", "many"])
def test_generated_files_decode_on_the_device(name, files, capfd, monkeypatch):
    made = files[name]; dev = [s for s in made["slices"] if s.expect_device()]
    a, blocks = _open(capfd, monkeypatch, True, path=made["cram"])
    b = ngsqc.Handle(path=made["bam"])
    c, none = _open(capfd, monkeypatch, False, path=made["cram"])
    m, blocks_m = _open(capfd, monkeypatch, True, data=np.fromfile(made["cram"], dtype=np.uint8))
    try:
        # decided as intended: every slice the gates let through was decoded on the device, no other
        assert blocks == blocks_m == (len(dev), sum(len(s.quals()) for s in dev), sum(1 for s in dev for n, q in s.records if n and q is not None)) and none == (0, 0, 0)
        assert {s.qs_method for s in dev} == {4, 41} and len(dev) == made["n_device"] > 0
        if name == "many": assert len(dev) == 3000
        assert a.n_records == b.n_records == c.n_records == m.n_records == sum(len(s.records) for s in made["slices"])
        want = b.inflated()
        for h in (a, c, m): assert np.array_equal(h.inflated(), want)                       # the BAM stream, byte for byte
        if name == "multi_ref":                                                             # the qualities through a kernel: depth of bases of quality >= 20
            regs = [(0, 1, 30000), (1, 1, 30000)]; n = 60000; got = []
            for h in (a, b, c):
                h.scan_depth(regs, min_mapq=1, min_baseq=20); got.append(h.depth(n).copy())
            b.scan_depth(regs, min_mapq=1, min_baseq=0); every = b.depth(n).copy()
            assert np.array_equal(got[0], got[1]) and np.array_equal(got[2], got[1]) and 0 < int(got[1].sum()) < int(every.sum())
    finally:
        for h in (a, b, c, m): h.close()


@pytest.mark.parametrize("name", list(FIXTURE_JOBS))
def test_fixture_blocks_go_to_the_device(name, capfd, monkeypatch):
    """the reference's own CRAM files (htslib's writer): their large quality blocks are decoded on the device - as many as the plan of the CPU test holds - and the
    stream equals the host path's"""
    src = os.path.join(GI, name)
    a, blocks = _open(capfd, monkeypatch, True, path=src)
    c, none = _open(capfd, monkeypatch, False, path=src)
    try:
        assert blocks[0] == FIXTURE_JOBS[name] > 0 and none[0] == 0
        assert a.n_records == c.n_records > 0 and np.array_equal(a.inflated(), c.inflated())
    finally:
        a.close(); c.close()
