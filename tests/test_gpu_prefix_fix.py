"""The order-dependent fix-ups (csrc/scan.hip: prefix_fix_kernel, its parallel form prefix_fix_max_kernel -> prefix_fix_seed_kernel -> prefix_fix_sum_kernel,
prefix_capture_kernel; driven by ScanState::tile and ngsqc_scan_mapping_finish in csrc/jobs.hip) on the designed files of readprofile_cases.py: the first
full-length and the first paired record sit on the edges of the kernels' own blocks. bases_trimmed, bases_usable_no_overlap, max_length, paired_end and
al_total are compared with readprofile.carry_model (the reference's sequential loop; test_cpu_readprofile.py holds it against the oracle), every other
counter with the oracle. All comparisons are exact integers.

Which kernel a file reaches (launch_prefix_fix): the tile-local prefix is upto = max(first full-length ordinal, first paired ordinal) when the tile's
longest read beats the running maximum / holds the file's first paired read. ScanState::tile passes scratch, so upto <= 4096 runs the one-workgroup kernel
(chunks of 256 records) and upto > 4096 the three-kernel form (blocks of PF_BLK = 1024 records, 256 block maxima per trip of the seed kernel). In the default
layout these files are ONE tile (asserted), so the tile-local ordinal is the file ordinal. ngsqc_scan_mapping_finish passes no scratch: as two shards the
one-workgroup kernel walks prefixes of any length, on the head words prefix_capture_kernel kept.

What a wrong kernel would trip over (argued from the code; the two mutations were not run):
* `upto <= 4096` -> `upto <= 4095` with an off-by-one in block_seed: first_full_4096 and the (4096, p <= 4096) pairs then take the three-kernel form, and a seed
  read from the neighbouring block changes A_FIX_TRIM wherever two neighbouring blocks differ in their maximum - every file with f > 4096 here (the rising
  staircase, steps_1024, mid_block, the large file), fused and unfused.
* `threadIdx.x ? sh[threadIdx.x - 1] : 0` -> `sh[threadIdx.x]` in prefix_fix_sum_kernel: a thread's four records then all run at the maximum INCLUDING themselves, so
  the sum changes wherever the maximum rises on the 2nd..4th record of a thread: every first_full / full_paired / quiet / mid_block file with f > 4096, the first
  tile of the two-tile file and the large file. By design not steps_256 / steps_1024 (their rises fall on multiples of 4) and not the second tile of the two-tile
  file (its maximum is the constant carry); those are there for the seeds and for A_FIX_CARRY."""
import time

import numpy as np
import pytest

import hostprep as H
import oracle_lib as O
import readprofile as RP
import readprofile_cases as RC
from test_gpu_shard import SKIP, _sharded_vs_oracle

pytestmark = pytest.mark.gpu
ngsqc = __import__("importlib").import_module("ngs-bits_amd")
BED = "chr1\t16000100\t16003000\tA\nchr1\t16010000\t16030000\tB\nchr1\t16050000\t16050400\tC\n"


def _check_handle(path, cols, bed, n_tiles):
    """NOROI against carry_model and the oracle, then one WGS and one ROI call on the three-line BED; returns the handle's timings"""
    ob = O.Bam(path)
    want = RP.carry_model(cols)
    h = ngsqc.Handle(path=path)
    try:
        for mode, b, mm in ((ngsqc.MODE_NOROI, None, 0), (ngsqc.MODE_WGS, bed, 3), (ngsqc.MODE_ROI, bed, 1)):
            if b is None and mode != ngsqc.MODE_NOROI:
                continue
            regs = H.bed_regions(b, h.refs, mm)[0] if b else None
            counters, _ = h.scan_mapping(mode, regions=regs, nonspecial=H.nonspecial(h.refs))
            if mode == ngsqc.MODE_NOROI:
                got = {key: int(counters[idx]) for idx, key in RP.CARRY_COUNTERS}
                assert got == want, (got, want)
            exp = O.mapping(ob, mode, b, merge_bed=(mm == 1))
            bad = [(O.COUNTER_NAMES[i] if i < 32 else i, int(counters[i]), int(exp.counters[i])) for i in range(len(counters)) if i not in SKIP and int(counters[i]) != int(exp.counters[i])]
            assert not bad, (mode, bad[:5])
        tm = h.timings()
    finally:
        h.close()
    if n_tiles is not None:
        assert tm["n_tiles"] == n_tiles, tm["n_tiles"]
    return tm


def _every_setting(tmp_path, monkeypatch, cols):
    path = RP.write(str(tmp_path / "designed.bam"), cols)
    bed = tmp_path / "chr1.bed"; bed.write_text(BED)
    monkeypatch.delenv("NGSQC_TILE_MEMBERS", raising=False)
    _check_handle(path, cols, str(bed), 1)                                   # default layout: one tile, fused scan
    monkeypatch.setenv("NGSQC_NO_FUSED_SCAN", "1")
    _check_handle(path, cols, None, 1)                                       # K2 and the scan as two kernels: the unfused key / ordinal path
    monkeypatch.delenv("NGSQC_NO_FUSED_SCAN")
    _sharded_vs_oracle(path, None, ngsqc.MODE_NOROI, 0, 2)                   # two shards: ngsqc_scan_mapping_finish on the captured head
    # (the sharded run against carry_model too: _sharded_vs_oracle compares with the oracle, which test_cpu_readprofile.py holds equal to the model)


@pytest.fixture(scope="module")
def files():
    return RC.prefix_files()


@pytest.mark.parametrize("f", RC.FIRST_FULL)
def test_first_full_on_the_block_edges(tmp_path, monkeypatch, files, f):
    """first full-length record at ordinal f, on both sides of the 256-record chunks, the 1024-record blocks and the 4096 switch: f <= 4096 takes
    the one-workgroup kernel, f > 4096 the three-kernel form (launch_prefix_fix, see the module docstring); the staircase in front rises inside the blocks"""
    _every_setting(tmp_path, monkeypatch, files[f"first_full_{f}"])


@pytest.mark.parametrize("f,p", RC.FULL_PAIRED)
def test_first_paired_independent_of_first_full(tmp_path, monkeypatch, files, f, p):
    """p << f, p >> f, p = f, p = f +- 1, no paired read at all (the whole file counts); both orders of the two limits on both sides of 4096"""
    _every_setting(tmp_path, monkeypatch, files[f"full_{f}_paired_{p}"])


@pytest.mark.parametrize("name", list(RC.QUIET))
def test_records_that_must_not_move_the_maximum(tmp_path, monkeypatch, name):
    """secondary / supplementary records of 151 bases in front of f (ordinals 0, 1023, 1024 / 0, 2047, 2048): the maximum stays 150, bases_trimmed is what
    the file without them gives; a duplicate, an unmapped and a MAPQ-0 record around every block edge raise the running maximum but add nothing to the length sum"""
    cols, without = RC.quiet_records(*RC.QUIET[name])
    assert RP.carry_model(cols) == RP.carry_model(without) and RP.carry_model(cols)["gmax"] == 150
    _every_setting(tmp_path, monkeypatch, cols)


@pytest.mark.parametrize("kind", ["steps_256", "steps_1024", "mid_block"])
def test_staircase_steps_on_the_block_edges(tmp_path, monkeypatch, files, kind):
    """the maximum rises exactly at every multiple of 256 / of 1024; mid_block: it rises inside every block of 1024 (block seed != block maximum everywhere)"""
    _every_setting(tmp_path, monkeypatch, files[kind])


def test_more_than_256_blocks(tmp_path, monkeypatch):
    """3e5 records of 1..30 bases, first full-length record at 262 144 + 1025: 258 blocks, so the seed kernel makes a second trip and its carry crosses
    the trips (the maximum still rises in blocks 256 and 257). One tile, default layout only.
    File generation, the model and the oracle take 1.4 s of this test on a CPU; the whole test prints its wall time (run with -s), which has not been
    recorded on an MI355X yet."""
    t0 = time.perf_counter()
    monkeypatch.delenv("NGSQC_TILE_MEMBERS", raising=False)
    cols = RC.many_blocks()
    path = RP.write(str(tmp_path / "big.bam"), cols, level=1)
    ob = O.Bam(path)
    want = RP.carry_model(cols)
    exp = O.mapping(ob, O.MODE_NOROI)
    h = ngsqc.Handle(path=path)
    try:
        counters, _ = h.scan_mapping(ngsqc.MODE_NOROI, nonspecial=H.nonspecial(h.refs))
        assert h.timings()["n_tiles"] == 1
    finally:
        h.close()
    got = {key: int(counters[idx]) for idx, key in RP.CARRY_COUNTERS}
    assert got == want, (got, want)
    bad = [(i, int(counters[i]), int(exp.counters[i])) for i in range(len(counters)) if i not in SKIP and int(counters[i]) != int(exp.counters[i])]
    assert not bad, bad[:5]
    print(f"more_than_256_blocks: {time.perf_counter() - t0:.2f} s")


def test_two_tiles_with_long_prefixes(tmp_path, monkeypatch):
    """first_full(5121) and a second, higher step (200) at 9000 + 4097, as two tiles of more than 4096 records each: both tiles take the three-kernel form, and
    A_FIX_CARRY enters the second one non-zero (150). No record of the second tile in front of the 200 reaches 150, so its running maximum IS the carry
    there: a carry that is lost (a seed of 0) changes bases_trimmed (test_cpu_readprofile.py::test_two_step_file asserts that of the file)"""
    cols = RC.two_steps()
    sizes, tile_members, n_first = RC.two_tile_layout(cols)
    assert RC.TWO_STEP_F < n_first and RC.TWO_STEP_F2 - n_first > 4096
    path = RP.write(str(tmp_path / "two.bam"), cols, sizes)
    bed = tmp_path / "chr1.bed"; bed.write_text(BED)
    monkeypatch.setenv("NGSQC_TILE_MEMBERS", str(tile_members))
    _check_handle(path, cols, str(bed), 2)
    monkeypatch.setenv("NGSQC_NO_FUSED_SCAN", "1")
    _check_handle(path, cols, None, 2)
