"""The library of FastqExtractBarcode, FastqAddBarcode, FastqDownsample and FastqConcat (include/ngsqc.h ngsqc_fqedit_*, ops 4 to 7; csrc/fqedit.hip) on the
designed cases (tests/fqedit2_cases.py) against the Python model (tests/fqedit2_oracle.py): the plan row for row, and the decompressed outputs, the statistics,
the entries of every side and the kept headers - whole, under feeds cut at every byte with a different cut on every side, with one side hundreds of entries
ahead, with a barcode read longer than a BGZF piece, with the decision stream cut before, on and behind a chunk border, and with files following one another
in one accumulator. Every comparison is exact: bytes or integers."""
import gzip
import importlib
import random

import numpy as np
import pytest

import bamdownsample_oracle as D
import fqedit2_cases as K2
import fqedit2_oracle as M2
from fqedit_cases import entry

pytestmark = pytest.mark.gpu
ngsqc = importlib.import_module("ngs-bits_amd")
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
_model = {}


def model(c):
    if c.name not in _model:
        _model[c.name] = c.model()
    return _model[c.name]


def file_feeds(c):
    """every file of the case whole, as one feed that ends it"""
    return [tuple(f) + (None,) * (3 - len(f)) + (True,) for f in c.files]


def pieces(file, sizes):
    """one file (a text per side) in pieces of sizes[k] bytes on side k, and an empty feed that ends it"""
    n = max((len(t) + s - 1) // s for t, s in zip(file, sizes))
    feeds = [tuple(t[s * i:s * i + s] for t, s in zip(file, sizes)) + (None,) * (3 - len(file)) + (False,) for i in range(n)]
    return feeds + [tuple(b"" for _ in file) + (None,) * (3 - len(file)) + (True,)]


def run_edit(lib_kw, feeds, tmp_path=None, tag="o", level=1, want_headers=False):
    """feeds: [(text 1, text 2 or None, text 3 or None, last)]. With tmp_path the outputs are written: -> dict(out, stats, sides, headers); without: -> dict(plan, ...)"""
    kw = dict(lib_kw, want_headers=True) if want_headers else lib_kw
    e = ngsqc.FastqEdit(**kw)
    try:
        paths = []
        if tmp_path is not None:
            paths = [str(tmp_path / ("%s.o%d.gz" % (tag, k + 1))) for k in range(e.streams)]
            e.outputs(paths[0], paths[1] if e.streams == 2 else None, compression_level=level)
        for a, b, c, last in feeds:
            e.feed(a, b, c, last=last)
        got = dict(stats=e.result(), sides=e.side_entries())
        if tmp_path is None:
            got["plan"] = e.plan()
        if want_headers:
            got["headers"] = e.kept_headers()
    finally:
        e.close()
    for p in paths:
        assert open(p, "rb").read()[-28:] == EOF_MEMBER
    got["out"] = [gzip.open(p, "rb").read() for p in paths]
    return got


def same_as_model(got, r):
    st = got["stats"]
    assert got["out"] == r.out
    assert st["entries"] == r.stats["entries"] and st["written"] == r.stats["written"] and st["bytes"] == r.stats["bytes"] and st["err_entry"] == -1
    if "headers" in got:
        assert got["headers"] == r.kept_headers
    if hasattr(r, "side_entries"):
        assert got["sides"] == r.side_entries


def same_plan(got, r):
    assert got["plan"].shape == r.plan.shape
    bad = np.nonzero((got["plan"] != r.plan).any(axis=tuple(range(1, r.plan.ndim))))[0]
    assert len(bad) == 0, [(int(i), got["plan"][i].tolist(), r.plan[i].tolist()) for i in bad[:5]]
    assert got["stats"]["written"] == r.stats["written"] and got["stats"]["bytes"] == r.stats["bytes"]   # (counted with or without outputs)


NAMES = [c.name for c in K2.catalogue()]


@pytest.mark.parametrize("name", NAMES)
def test_plan_row_for_row(name):
    c = K2.by_name(name)
    same_plan(run_edit(c.lib_kw(), file_feeds(c)), model(c))


@pytest.mark.parametrize("name", NAMES)
def test_outputs_and_statistics_whole(tmp_path, name):
    c = K2.by_name(name)
    same_as_model(run_edit(c.lib_kw(), file_feeds(c), tmp_path, want_headers=c.op == "downsample"), model(c))


def test_fastq_edit_plan_takes_a_third_text():
    c = K2.by_name("add-digits")
    assert np.array_equal(ngsqc.fastq_edit_plan(*c.files[0][:2], text3=c.files[0][2], op="barcode_add"), model(c).plan)
    c = K2.by_name("cut-1")
    assert np.array_equal(ngsqc.fastq_edit_plan(c.files[0][0], op="barcode_cut", cut1=1), model(c).plan)


def test_cut_at_every_byte(tmp_path):
    c = K2.by_name("cut-len-1")
    assert len(c.files[0][0]) <= 300
    same_as_model(run_edit(c.lib_kw(), pieces(c.files[0], (1,)), tmp_path), model(c))


@pytest.mark.parametrize("sizes", [(1, 7, 3), (7, 3, 1), (3, 1, 7)])
def test_cut_at_every_byte_with_a_different_cut_on_every_side(tmp_path, sizes):
    c = K2.by_name("add-headers")
    assert all(len(t) <= 300 for t in c.files[0])
    same_as_model(run_edit(c.lib_kw(), pieces(c.files[0], sizes), tmp_path), model(c))


@pytest.mark.parametrize("ahead", [0, 1, 2])
def test_one_side_hundreds_of_entries_ahead(tmp_path, ahead):
    rng = random.Random(11)
    t = [K2.text([entry(rng, "p%d" % i, 10 + (i * (k + 3)) % 40, header=("@p%d %d:N" % (i, k + 1)).encode()) for i in range(600)]) for k in range(3)]
    c = K2.Case("add-many", "barcode_add", {}, [tuple(t)])
    lag = [k for k in range(3) if k != ahead]
    cuts = [[0, 1000, 1001, len(t[k]) // 3, len(t[k]) // 2 + 5, len(t[k])] for k in range(3)]
    feeds = []
    for i in range(5):   # the whole of one side at once, the others in five pieces cut anywhere
        f = [b"", b"", b""]
        f[ahead] = t[ahead] if i == 0 else b""
        for k in lag:
            f[k] = t[k][cuts[k][i]:cuts[k][i + 1]]
        feeds.append(tuple(f) + (i == 4,))
    same_as_model(run_edit(c.lib_kw(), feeds, tmp_path), model(c))


def test_a_barcode_read_longer_than_a_piece_straddles_windows(tmp_path, monkeypatch):
    """a barcode read of 70 000 bases, windows of one BGZF piece (0xff00 bytes): the two headers it goes into, and so the two output entries, are written by
    several launches of the format kernel"""
    monkeypatch.setenv("NGSQC_WRITE_WINDOW_PIECES", "1")
    rng = random.Random(13)
    e1 = [entry(rng, "s%d" % i, 100, header=("@s%d 1" % i).encode()) for i in range(120)]
    e2 = [entry(rng, "s%d" % i, 80, header=("@s%d 2" % i).encode()) for i in range(120)]
    e3 = [entry(rng, "b%d" % i, 8) for i in range(120)]
    e3[60] = entry(rng, "big", 70000)
    c = K2.Case("add-big", "barcode_add", {}, [(K2.text(e1), K2.text(e2), K2.text(e3))])
    r = c.model()
    assert r.plan[60, 0, 2] == 5 + 5 + 70000 > 0xff00 and min(len(x) for x in r.out) > 70000 + 10000   # one header alone is longer than a window
    same_plan(run_edit(c.lib_kw(), file_feeds(c)), r)
    same_as_model(run_edit(c.lib_kw(), file_feeds(c), tmp_path, "whole"), r)
    same_as_model(run_edit(c.lib_kw(), pieces(c.files[0], (50000, 3000, 40000)), tmp_path, "pieces", level=0), r)


def test_decisions_across_feeds_cut_around_a_chunk_border(tmp_path):
    """2 CHUNK + 1 pairs in pieces whose borders fall one pair before, on and one pair behind a chunk border of the generator: the decisions are those of
    the one sequential stream, the kept headers the model's, and the plan is the plan of the same input fed whole"""
    n, seed, p = 2 * K2.CHUNK + 1, 12345, 20.0
    c = K2.by_name("downsample-%d-seed%d-%g" % (n, seed, p))
    r = model(c)
    t1, t2 = c.files[0]
    starts = [[0], [0]]
    for k, t in enumerate((t1, t2)):
        at = 0
        for _ in range(n):
            at = t.index(b"\n", t.index(b"\n+\n", at) + 3) + 1
            starts[k].append(at)
        assert at == len(t)
    borders = [0, K2.CHUNK - 1, K2.CHUNK, K2.CHUNK + 1, 2 * K2.CHUNK, n]
    feeds = [(t1[starts[0][a]:starts[0][b]], t2[starts[1][a]:starts[1][b]], None, False) for a, b in zip(borders, borders[1:])] + [(b"", b"", None, True)]
    got = run_edit(c.lib_kw(), feeds, want_headers=True)
    assert np.array_equal(got["plan"][:, 0, 0], D.keep_stream(seed, p, 0, n)) and np.array_equal(got["plan"][:, 1, 0], got["plan"][:, 0, 0])
    same_plan(got, r)
    assert got["headers"] == r.kept_headers
    whole = run_edit(c.lib_kw(), file_feeds(c))
    assert np.array_equal(whole["plan"], got["plan"])
    same_as_model(run_edit(c.lib_kw(), feeds, tmp_path, want_headers=True), r)


def test_a_feed_behind_the_last_piece_of_a_file_carries_on(tmp_path):
    c = K2.by_name("copy-first-lacks-final-newline")
    r = model(c)
    e = ngsqc.FastqEdit("copy")
    e.feed(c.files[0][0], last=True)
    assert e.side_entries() == [3]
    e.feed(c.files[1][0][:9])                 # the second file begins: a piece that ends inside its first entry
    e.feed(c.files[1][0][9:], last=True)
    e.feed(c.files[2][0], last=True)
    assert e.side_entries() == [r.stats["entries"]]
    assert np.array_equal(e.plan(), r.plan) and np.array_equal(e.plan(first=3, n=2), r.plan[3:5])
    e.close()
    same_as_model(run_edit(c.lib_kw(), file_feeds(c)[:1] + pieces(c.files[1], (9,)) + file_feeds(c)[2:], tmp_path), r)


def test_refusals(tmp_path):
    def refused(call, msg):
        with pytest.raises(ngsqc.NgsqcError) as x:
            call()
        assert x.value.code == -3 and msg in str(x.value), str(x.value)
    a = b"@a\nAC\n+\nII\n"
    e = ngsqc.FastqEdit("barcode_add")
    refused(lambda: e.feed(a, a), "three inputs")
    refused(lambda: e.outputs(str(tmp_path / "a")), "out2 is needed")
    e.close()
    for op in ("trim", "copy", "barcode_cut"):
        e = ngsqc.FastqEdit(op)
        refused(lambda: e.feed(a, None, a), "one input")
        refused(lambda: e.feed(a, a, a), "one input")
        refused(lambda: e.downsample(1, 20.0), "only FastqDownsample")
        e.close()
    e = ngsqc.FastqEdit("umi")
    refused(lambda: e.feed(a, a, a), "two inputs")
    e.close()
    e = ngsqc.FastqEdit("copy")
    refused(lambda: e.outputs(str(tmp_path / "a"), str(tmp_path / "b")), "one output")
    e.close()
    e = ngsqc.FastqEdit("barcode_cut")
    refused(lambda: e.outputs(str(tmp_path / "a")), "out2 is needed")
    e.close()
    refused(lambda: ngsqc.FastqEdit("barcode_cut", cut1=-1), "must not be negative!")
    for p in (0, 100, -1.5, 100.5):
        refused(lambda: ngsqc.FastqEdit("downsample", seed=1, percentage=p), "Invalid percentage %g!" % p)
    e = ngsqc.FastqEdit("downsample")
    refused(lambda: e.feed(a, a, last=True), "ngsqc_fqedit_downsample comes before the first feed")
    refused(lambda: e.outputs(str(tmp_path / "a")), "out2 is needed")
    e.downsample(1, 20.0)
    refused(lambda: e.downsample(1, 20.0), "set once, before the first feed")
    e.feed(a, a, last=True)
    refused(lambda: e.downsample(2, 30.0), "set once, before the first feed")
    e.result()
    refused(lambda: e.kept_headers(), "only when ngsqc_fqedit_downsample asked for them")
    e.close()
    e = ngsqc.FastqEdit("downsample", seed=1, percentage=20.0, want_headers=True)
    e.feed(a, a, last=True)
    refused(lambda: e.kept_headers(), "ngsqc_fqedit_result comes first")
    e.close()
