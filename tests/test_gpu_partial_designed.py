"""Shard, range and head handles on designed member geometry (tests/partial_cases.py; premises: test_cpu_partial_model.py), one test per case.

Shards: one test per (case, N), every tile layout of that N, handles opened by path and from memory (the exchange of summaries once per layout: both cut the
same member table). Per shard a fresh handle's record count, local record offsets, inflated
bytes and member count are the sequential model's; scan_mapping_partial reports the model's (n_records, first_abs, exit_abs) - (-1, -1) for a shard that owns
no record -, ngsqc_plan_shard_fix accepts the summaries, and the protocol gives the ORACLE's counters, insert-size histogram and depth for the whole file;
the partial depth scans, reduced and finalized, give the oracle's depth. Under NGSQC_SHARD_TAIL_MEMBERS exactly the shards whose last record needs more
tail members refuse, naming the shard and the switch.

Ranges and heads: the same four facts against the model, and the depth and read counts of the handle against the oracle's over a file of the owned records
alone. Once per file: write_bai() and a region handle on each of about forty records' positions against the oracle's depth and read counts of the whole file.

Refusals: every run goes through _Ledger. Outside the decoy cases and the designed tail, head and range refusals no refusal is allowed - each test ends by
asserting that the ledger holds exactly the designed ones. A decoy case has two allowed outcomes per entry point: the model's / oracle's result, or
NGSQC_E_FORMAT; a number that differs from the oracle's fails."""
import contextlib
import os

import numpy as np
import pytest

import cram_twin
import hostprep as H
import oracle_lib as O
import partial_cases as P

pytestmark = pytest.mark.gpu
ngsqc = __import__("importlib").import_module("ngs-bits_amd")
dist_mod = __import__("importlib").import_module("ngs-bits_amd.dist")

SWITCHES = ("NGSQC_TILE_MEMBERS", "NGSQC_SHARD_TAIL_MEMBERS", "NGSQC_CARRY_MAX", "NGSQC_WALKERS", "NGSQC_K2_GENERAL", "NGSQC_LONG_READ_MODE", "NGSQC_GROUP_SHIFT",
            "NGSQC_NO_FUSED_SCAN", "NGSQC_EAGER_RECOFF")
SKIP_COUNTERS = {"half_depth", "bases_covered_half"}   # (they come from ngsqc_depth_stats)


@contextlib.contextmanager
def _env(tile_members=None, tail=None):
    keep = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        if tile_members is not None:
            os.environ["NGSQC_TILE_MEMBERS"] = str(tile_members)
        if tail is not None:
            os.environ["NGSQC_SHARD_TAIL_MEMBERS"] = str(tail)
        yield
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


class _Ledger:
    """every library call of a test runs through here: `expect` = None (must succeed), (code, [message parts]) (must refuse so) or "either" (a decoy: the
    exact result or NGSQC_E_FORMAT)"""

    def __init__(self):
        self.refused, self.ran = [], 0

    def run(self, tag, expect, fn):
        self.ran += 1
        try:
            out = fn()
        except ngsqc.NgsqcError as e:
            assert expect is not None, ("refused where no refusal is allowed", tag, e.code, e.message)
            if expect == "either":
                assert e.code == P.E_FORMAT, (tag, e.code, e.message)
            else:
                assert e.code == expect[0] and all(part in e.message for part in expect[1]), (tag, e.code, e.message, expect)
            self.refused.append(tag)
            return None
        assert expect is None or expect == "either", ("did not refuse", tag, expect)
        return out


_MADE = {}


def _sub_bam(c, owned, ends, path):
    """a BAM of the header and the owned records alone"""
    raw = c.raw[:c.first_rec] + b"".join(c.raw[int(o):int(e)] for o, e in zip(owned, ends))
    open(path, "wb").write(b"".join(cram_twin._bgzf(raw[k:k + 60000]) for k in range(0, len(raw), 60000)) + cram_twin._bgzf(b""))
    return path


def _oracle(bam, bed, mapping=False):
    b = O.Bam(bam)
    out = dict(cov=O.low_high_coverage(b, bed, 20, 1, 0, is_high=False, random_access=True, tool_merge=1), counts=O.read_counts(b, bed, 1))
    if mapping:
        out["mapping"] = O.mapping(b, O.MODE_WGS, bed, merge_bed=False)
    return out


def _case(name, tmp_path_factory):
    """the case, its model, its file, and the oracle's answers over the whole file: made once"""
    if name not in _MADE:
        p = P.get(name)
        d = tmp_path_factory.mktemp("partial_" + name)
        path = p.write(str(d / (name + ".bam")))
        bed = str(d / (name + ".bed")); open(bed, "w").write(p.case.bed())
        refs = p.case.refs
        tm = H.tid_map(refs)
        ref = _oracle(path, bed, mapping=True)
        ref.update(bed=bed, dir=d, regs3=H.bed_regions(bed, refs, 3)[0], regs2=H.bed_regions(bed, refs, 2)[0],
                   lines=[(tm[H.chr_num(f[0])], int(f[1]) + 1, int(f[2])) for f in (ln.split("\t") for ln in ref["counts"][1].splitlines())])
        tx, ty = H.xy_tids(refs)
        ref["mp"] = dict(regions=ref["regs3"], min_mapq=1, tid_x=tx, tid_y=ty, nonspecial=H.nonspecial(refs))
        _MADE[name] = (p, p.model(), path, np.fromfile(path, dtype=np.uint8), ref)
    return _MADE[name]


def _check_index(h, x, raw, tiled, tag):
    """a fresh handle against the model: records, local offsets, members, inflated bytes (a tiled shard stops at the tile of the next shard's first record: its
    own bytes are compared)"""
    lo, hi = x["inflated"]
    assert h.n_records == x["n_records"], (tag, h.n_records, x["n_records"])
    got = h.record_offsets()
    assert np.array_equal(got, x["local"]), (tag, "record offsets", got[:4], x["local"][:4])
    assert h.n_blocks == x["n_blocks"] and h.inflated_size == hi - lo, (tag, h.n_blocks, x["n_blocks"], h.inflated_size, hi - lo)
    k = x["own_bytes"] if tiled and "own_bytes" in x else hi - lo
    assert np.array_equal(h.inflated()[:k], raw[lo:lo + k]), (tag, "inflated bytes")


def _check_counters(counters, exp, tag):
    for i, name in enumerate(O.COUNTER_NAMES):
        if name not in SKIP_COUNTERS:
            assert int(counters[i]) == int(exp.counters[i]), (tag, name, int(counters[i]), int(exp.counters[i]))
    assert np.array_equal(counters[32:], exp.counters[32:]), (tag, "insert-size histogram")


def _close(hs):
    for h in hs:
        h.close()


BIG_N = 40   # above it only the shards that hold a member, some of the empty shards behind them and the last shard are opened (the other empty ones hold nothing to run)


def _opened(exp, N):
    if N <= BIG_N:
        return list(range(N))
    full = [s for s, x in enumerate(exp) if x["kind"] != "empty"]
    return sorted(set(full) | {s + 1 for s in full[::4] if s + 1 < N} | {N - 1})


def _shard_run(p, m, path, data, ref, N, tm, tail, by_path, protocol, led):
    exp = m.shards(N, tail)
    raw = np.frombuffer(p.case.raw, dtype=np.uint8)
    src = "path" if by_path else "data"
    open_ = (lambda s: ngsqc.Handle(path=path, shard=(s, N))) if by_path else (lambda s: ngsqc.Handle(data=data, shard=(s, N)))
    either = "either" if p.decoy else None
    which = _opened(exp, N)
    mp = dict(ref["mp"], mode=ngsqc.MODE_WGS)
    with _env(tm, tail):
        if tail is not None:
            # ---- under NGSQC_SHARD_TAIL_MEMBERS: every entry point of a shard whose last record needs more members refuses, the other shards are exact ----
            for s in which:
                x = exp[s]
                tag = (p.name, N, tm, tail, src, s)
                want = (P.E_FORMAT, [P.MSG_TAIL, f"shard {s} "]) if x["refuses"] else None
                h = open_(s)
                try:
                    led.run(tag + ("index",), want, lambda: _check_index(h, x, raw, False, tag))
                    led.run(tag + ("summary",), want, lambda: _check_summary(h.scan_mapping_partial(**mp), x, tag))
                    led.run(tag + ("depth",), want, lambda: h.scan_depth(ref["regs2"], min_mapq=1, partial=True))
                finally:
                    h.close()
            return
        # ---- per shard the index of a fresh handle; then, on the same handles, the coverage tools' path: partial depth scans, reduced and finalized ----
        hs = []
        try:
            for s in which:
                x = exp[s]
                tag = (p.name, N, tm, src, s)
                hs.append(open_(s))
                if p.decoy and x.get("u0") == p.decoy["member_at"]:
                    continue      # (the shard that starts in front of the decoys: alone it cannot know; what the exchange makes of it is checked below)
                led.run(tag + ("index",), either, lambda: _check_index(hs[-1], x, raw, tm is not None, tag))

            def depth():
                for h in hs:
                    h.scan_depth(ref["regs2"], min_mapq=1, partial=True)
                hs[0].depth_reduce(hs[1:])
                hs[0].depth_finalize()
                assert np.array_equal(hs[0].depth(ref["cov"]["roi_bases"]), ref["cov"]["depth"]), (p.name, N, tm, src, "depth of the reduced scans")
            led.run((p.name, N, tm, src, "depth_reduce"), either, depth)
        finally:
            _close(hs)
        if not protocol:
            return
        # ---- the mapping protocol on fresh handles: summaries, ngsqc_plan_shard_fix, the oracle's counters, histogram and depth ----
        def mapping():
            hs = [open_(s) for s in which]
            try:
                counters, _, summaries = dist_mod.scan_mapping_sharded_local(hs, ngsqc.MODE_WGS, **ref["mp"])
                for k, s in enumerate(which):
                    _check_summary(summaries[k], exp[s], (p.name, N, tm, src, s))
                _check_counters(counters, ref["mapping"], (p.name, N, tm, src))
                assert np.array_equal(hs[0].depth(int(counters[O.COUNTER_NAMES.index("roi_bases")])), ref["mapping"].depth), (p.name, N, tm, src, "depth of the mapping scan")
            finally:
                _close(hs)
        led.run((p.name, N, tm, src, "protocol"), either, mapping)
        if p.decoy:
            def job():
                hs = [open_(s) for s in which]
                try:
                    jobs = [h.run_job(mapping=mp, depth=dict(regions=ref["regs2"], min_mapq=1), partial=True) for h in hs]
                    summaries = np.stack([j["summary"] for j in jobs])
                    parts = [h.scan_mapping_finish(ngsqc.plan_shard_fix(summaries, i)) for i, h in enumerate(hs)]
                    _check_counters(ngsqc.combine_counters_local([c for c, _ in parts]), ref["mapping"], (p.name, N, tm, src, "job"))
                finally:
                    _close(hs)
            led.run((p.name, N, tm, src, "run_job"), either, job)


def _check_summary(sm, x, tag):
    assert (int(sm[0]), int(sm[1]), int(sm[2])) == (x["n_records"], x["first_abs"], x["exit_abs"]), (tag, [int(v) for v in sm[:3]], (x["n_records"], x["first_abs"], x["exit_abs"]))


SHARD_RUNS = [(n, N) for n in P.SHARD_CASES if n not in P.DECOYS for N in sorted({N for N, _ in P.get(n).shard_runs})]


@pytest.mark.parametrize("name,N", SHARD_RUNS, ids=[f"{n}-N{N}" for n, N in SHARD_RUNS])
def test_shards(name, N, tmp_path_factory):
    p, m, path, data, ref = _case(name, tmp_path_factory)
    led = _Ledger()
    layouts = [tm for n, tm in p.shard_runs if n == N]
    for tm in layouts:
        for by_path in (True, False):
            _shard_run(p, m, path, data, ref, N, tm, None, by_path, by_path, led)      # (the exchange once per layout: from memory and by path the same member table is cut)
    assert led.refused == [] and led.ran >= 5 * len(layouts)               # no refusal outside the designed ones
    tails = [t for n, t in p.tails if n == N]
    for tail in tails:
        _shard_run(p, m, path, data, ref, N, None, tail, True, False, led)
    designed = [(name, N, None, tail, "path", s, what) for tail in tails for s, x in enumerate(m.shards(N, tail)) if x["refuses"] for what in ("index", "summary", "depth")]
    assert led.refused == designed and (not tails or designed)


@pytest.mark.parametrize("name", P.DECOYS)
def test_decoy(name, tmp_path_factory):
    """a guess is never trusted: every shard entry point gives the model's / the oracle's result or refuses with NGSQC_E_FORMAT"""
    p, m, path, data, ref = _case(name, tmp_path_factory)
    assert ref["cov"]["depth"][-400:].sum() == 0 and ref["cov"]["depth"].sum() > 0     # the oracle has no depth on chrX: a counted decoy shows
    led = _Ledger()
    for N, tm in p.shard_runs:
        for by_path in (True, False):
            _shard_run(p, m, path, data, ref, N, tm, None, by_path, True, led)
    print(name, "refused:", sorted({t[-1] for t in led.refused}), len(led.refused), "of", led.ran)


# ---- ranges and heads ----
def _check_selection(p, m, ref, r, open_, tm, tag, led, want):
    """a range or head handle against the model, and its depth and read counts against the oracle's over the owned records alone"""
    raw = np.frombuffer(p.case.raw, dtype=np.uint8)

    def index():
        h = open_()
        try:
            _check_index(h, dict(r, own_bytes=int(r["owned"][-1] - r["inflated"][0]) if r["n_records"] else 0), raw, tm is not None, tag)
        finally:
            h.close()
    led.run(tag + ("index",), want, index)
    if want is not None:
        return
    sub = _sub_bam(p.case, r["owned"], m.ends[np.searchsorted(m.offs, r["owned"])], str(ref["dir"] / "sub.bam"))
    exp = _oracle(sub, ref["bed"])

    def products():
        h = open_()
        try:
            h.scan_depth(ref["regs2"], min_mapq=1)
            assert np.array_equal(h.depth(exp["cov"]["roi_bases"]), exp["cov"]["depth"]), (tag, "depth")
            assert np.array_equal(h.region_read_counts(ref["lines"], 1), exp["counts"][0]), (tag, "read counts")
        finally:
            h.close()
    led.run(tag + ("products",), None, products)


@pytest.mark.parametrize("name", P.RANGE_CASES)
def test_ranges(name, tmp_path_factory):
    p, m, path, data, ref = _case(name, tmp_path_factory)
    led = _Ledger()
    designed = []
    for tag, beg, end, tm in p.ranges:
        r = m.range(beg, end)
        if r["refuses"]:
            designed.append((name, tag, "index"))
        with _env(tm):
            _check_selection(p, m, ref, r, lambda: ngsqc.Handle(path=path, voff_range=(beg, end)), tm, (name, tag), led, (r["refuses"][0], [r["refuses"][1]]) if r["refuses"] else None)
    assert led.refused == designed and len(designed) == 2 * (name != "shard_tiles")


@pytest.mark.parametrize("name", P.HEAD_CASES)
def test_heads(name, tmp_path_factory):
    p, m, path, data, ref = _case(name, tmp_path_factory)
    led = _Ledger()
    designed = []
    for tag, k, tail, tm in p.heads:
        r = m.head(k, tail)
        if r["refuses"]:
            designed.append((name, tag, "index"))
        with _env(tm, tail):
            _check_selection(p, m, ref, r, lambda: ngsqc.Handle(path=path, head_members=k), tm, (name, tag), led, (r["refuses"][0], [r["refuses"][1], "shard 0 "]) if r["refuses"] else None)
    assert led.refused == designed and len(designed) == 1


@pytest.mark.parametrize("name", P.RANGE_CASES)
def test_region_handles_on_single_records(name, tmp_path_factory):
    """write_bai() on the whole file, then a region handle on the position of each of about forty records spread over the file: its depth and read count at
    that position are the oracle's over the whole file"""
    p, m, path, data, ref = _case(name, tmp_path_factory)
    c = p.case
    whole = ngsqc.Handle(path=path)
    try:
        whole.write_bai()
    finally:
        whole.close()
    where = sorted({tuple(int(v) for v in np.frombuffer(c.raw[int(o) + 4:int(o) + 12], dtype=np.int32)) for o in m.offs[::max(1, m.offs.size // 40)]})
    bed = str(ref["dir"] / "records.bed")
    open(bed, "w").write("".join(f"{c.refs[tid][0]}\t{pos}\t{pos + 1}\n" for tid, pos in where))     # (0-based pos -> the 1-based position pos + 1)
    b = O.Bam(path)
    depth = O.low_high_coverage(b, bed, 20, 1, 0, is_high=False, random_access=True, tool_merge=1)["depth"]
    counts, text = O.read_counts(b, bed, 1)
    assert depth.size == len(where) == len(text.splitlines()) and depth.sum() > 0
    led = _Ledger()
    for j, (tid, pos) in enumerate(where):
        def one():
            h = ngsqc.Handle(path=path, regions=[(c.refs[tid][0], pos + 1, pos + 1)])
            try:
                h.scan_depth([(tid, pos + 1, pos + 1)], min_mapq=1)
                assert int(h.depth(1)[0]) == int(depth[j]), (name, tid, pos, "depth")
                assert int(h.region_read_counts([(tid, pos + 1, pos + 1)], 1)[0]) == int(counts[j]), (name, tid, pos, "read count")
            finally:
                h.close()
        led.run((name, tid, pos), None, one)
    assert led.refused == []
