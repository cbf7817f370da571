"""The record index on designed member and tile geometry (tests/k2geom_cases.py; premises: test_cpu_k2geom.py), one test per case. Every case runs under each
of its tile layouts (NGSQC_TILE_MEMBERS / NGSQC_CARRY_MAX) and each path switch of K2: the walkers per member, the separate scan, the host-verified chain, the
eager offsets, long-read groups of two and four members. For every run:
 * a fresh handle's record count, record offsets and inflated bytes are the model's (one loop over block_size), exactly;
 * one job (MappingQC in WGS mode over the case's BED, riding K2's walk where the switches allow, and a site pileup) gives the ORACLE's counters, insert-size
   histogram, per-base depth and site counts - never compared with another run of the library first; all runs of a case then also agree with each other;
 * the record offsets asked for AFTER that job (the lazily expanded ones of a single-tile file) are the model's as well;
 * timings() says the path the case was built for was taken: aligned cases pass the chain check on the device and ride the walk in every tile with the set
   number of walkers; groups of up to 4095 records pass as groups of four members, groups of 4096 do not, and three such tiles in a row end long-read mode.
The one refusal: a record that leaves one byte more than NGSQC_CARRY_MAX to carry (decided on the host before any copy)."""
import contextlib
import os

import numpy as np
import pytest

import hostprep as H
import k2geom_cases as K
import oracle_lib as O
from test_cpu_k2geom import reference

pytestmark = pytest.mark.gpu
ngsqc = __import__("importlib").import_module("ngs-bits_amd")

SWITCH_SETS = [("default", {}), ("walkers2", {"NGSQC_WALKERS": "2"}), ("walkers4", {"NGSQC_WALKERS": "4"}), ("walkers8", {"NGSQC_WALKERS": "8"}),
               ("no_fused_scan", {"NGSQC_NO_FUSED_SCAN": "1"}), ("k2_general", {"NGSQC_K2_GENERAL": "1"}), ("eager_recoff", {"NGSQC_EAGER_RECOFF": "1"}),
               ("groups2", {"NGSQC_LONG_READ_MODE": "1", "NGSQC_GROUP_SHIFT": "1"}), ("groups4", {"NGSQC_LONG_READ_MODE": "1", "NGSQC_GROUP_SHIFT": "2"})]
WALKERS = {"default": 1, "walkers2": 2, "walkers4": 4, "walkers8": 8}
ALL_SWITCHES = ("NGSQC_WALKERS", "NGSQC_NO_FUSED_SCAN", "NGSQC_K2_GENERAL", "NGSQC_EAGER_RECOFF", "NGSQC_LONG_READ_MODE", "NGSQC_GROUP_SHIFT", "NGSQC_TILE_MEMBERS",
                "NGSQC_CARRY_MAX")
SKIP_COUNTERS = {"half_depth", "bases_covered_half"}   # (ngsqc_depth_stats: they come from depth_stats)


@contextlib.contextmanager
def _env(**kw):
    keep = {k: os.environ.get(k) for k in ALL_SWITCHES}
    try:
        for k in ALL_SWITCHES:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in kw.items() if v is not None})
        yield
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


_MADE = {}


def _case(name, tmp_path_factory):
    """the case, its file and the oracle's reference: made once"""
    if name not in _MADE:
        c = K.get(name)
        d = tmp_path_factory.mktemp("k2geom_" + name)
        path = c.write(str(d / (name + ".bam")))
        _MADE[name] = (c, path, reference(c, path, d))
    return _MADE[name]


def _job_inputs(c, ref):
    regs, _ = H.bed_regions(ref["bed"], c.refs, 3)
    tx, ty = H.xy_tids(c.refs)
    return dict(mode=ngsqc.MODE_WGS, regions=regs, min_mapq=1, tid_x=tx, tid_y=ty, nonspecial=H.nonspecial(c.refs))


def _check_job(c, ref, job, depth, tag):
    exp = ref["mapping"]
    for i, name in enumerate(O.COUNTER_NAMES):
        if name not in SKIP_COUNTERS:
            assert int(job["counters"][i]) == int(exp.counters[i]), (c.name, tag, name, int(job["counters"][i]), int(exp.counters[i]))
    assert np.array_equal(job["counters"][32:], exp.counters[32:]), (c.name, tag, "insert-size histogram")
    assert np.array_equal(depth, exp.depth), (c.name, tag, "per-base depth")
    assert np.array_equal(job["site_counts"][:, :6], ref["site_counts"]) and not job["site_counts"][:, 6:].any(), (c.name, tag, "site counts")


def _check_path(c, tag, sw, tm_set, t):
    """the path the case was built for (timings() of the job)"""
    exp = c.expect
    nt = t["n_tiles"]
    assert nt == len(c.tile_model(tm_set)), (c.name, tag, nt)
    if c.aligned and sw in WALKERS:
        assert t["tiles_chain_on_device"] == nt == t["tiles_scan_fused"] and t["walkers_per_member"] == WALKERS[sw], (c.name, tag, t)
    if exp.get("path") == "names" and sw == "groups4":
        if exp["fits"]:
            assert t["tiles_chain_on_device"] == nt == t["tiles_scan_fused"] and t["walkers_per_member"] == -4, (c.name, tag, t)
        else:
            assert t["tiles_chain_on_device"] < nt, (c.name, tag, t)
        if exp["drop"]:   # the first tile rode the walk as a group; three refused tiles ended long-read mode: the tiles behind them are walked member by member
            assert t["tiles_scan_fused"] == 1 and t["walkers_per_member"] == 1, (c.name, tag, t)


def _run_case(name, tmp_path_factory):
    c, path, ref = _case(name, tmp_path_factory)
    offs = c.walk()
    raw = np.frombuffer(c.raw, dtype=np.uint8)
    mp = _job_inputs(c, ref)
    first, seen = None, []
    for tm_set, carry_max in c.layouts:
        for sw, env in SWITCH_SETS:
            tag = (tm_set, carry_max, sw)
            with _env(NGSQC_TILE_MEMBERS=None if tm_set is None else str(tm_set), NGSQC_CARRY_MAX=None if carry_max is None else str(carry_max), **env):
                if c.refuses:
                    h = ngsqc.Handle(path=path)
                    try:
                        with pytest.raises(ngsqc.NgsqcError, match=c.refuses):
                            h.n_records
                        with pytest.raises(ngsqc.NgsqcError, match=c.refuses):
                            h.run_job(mapping=mp, sites=ref["sites"])
                    finally:
                        h.close()
                    continue
                # the record index of a fresh handle
                h = ngsqc.Handle(path=path)
                try:
                    assert h.n_records == offs.size, (name, tag, h.n_records, offs.size)
                    got = h.record_offsets()
                    assert np.array_equal(got, offs), (name, tag, "record offsets", int(np.nonzero(got != offs)[0][0]))
                    assert np.array_equal(h.inflated(), raw), (name, tag, "inflated bytes")
                finally:
                    h.close()
                # the job on a handle of its own (its scan rides the first walk of the tiles), the path it took, the offsets behind it
                h = ngsqc.Handle(path=path)
                try:
                    job = h.run_job(mapping=mp, sites=ref["sites"])
                    t = h.timings()
                    depth = h.depth(int(job["counters"][O.COUNTER_NAMES.index("roi_bases")]))
                    _check_job(c, ref, job, depth, tag)
                    assert t["n_records"] == offs.size, (name, tag, t["n_records"])
                    _check_path(c, tag, sw, tm_set, t)
                    got = h.record_offsets()
                    assert np.array_equal(got, offs), (name, tag, "record offsets behind the job", int(np.nonzero(got != offs)[0][0]))
                finally:
                    h.close()
                seen.append((tag, {k: t[k] for k in ("n_tiles", "tiles_chain_on_device", "tiles_scan_fused", "walkers_per_member")}))
                res = (job["counters"].copy(), depth.copy(), job["site_counts"].copy())
                if first is None:
                    first = res
                assert all(np.array_equal(a, b) for a, b in zip(first, res)), (name, tag, "differs from the case's first run")
    print(name, seen)   # (pytest -s: the paths taken)
    assert c.refuses or len(seen) == len(c.layouts) * len(SWITCH_SETS)


@pytest.mark.parametrize("name", K.ALL)
def test_case(name, tmp_path_factory):
    _run_case(name, tmp_path_factory)
