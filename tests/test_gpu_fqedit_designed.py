"""The library of the per-entry FASTQ tools (include/ngsqc.h ngsqc_fqedit_*, csrc/fqedit.hip) on the designed entries (tests/fqedit_cases.py) against the Python
model (tests/fqedit_oracle.py): the plan row for row through fastq_edit_plan, and the decompressed outputs and the statistics through FastqEdit - whole, under
feeds cut at every byte, with differing cuts on the two sides and one side hundreds of entries ahead, with every probe of the id table colliding, and with one
entry longer than a BGZF piece straddling output windows. Every comparison is exact: bytes or integers."""
import gzip
import importlib
import random

import numpy as np
import pytest

import fqedit_cases as K
import fqedit_oracle as M

pytestmark = pytest.mark.gpu
ngsqc = importlib.import_module("ngs-bits_amd")
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
_model = {}


def model(g):
    if g.name not in _model:
        _model[g.name] = g.texts() + (g.model(),)
    return _model[g.name]


def gunzip(path):
    with gzip.open(path, "rb") as f:
        return f.read()


def run_edit(lib_kw, ids, tmp_path, feeds, tag, level=1):
    """feeds: [(piece 1, piece 2 or None)]; the last one ends the input. -> ([texts of the outputs], statistics)"""
    e = ngsqc.FastqEdit(**lib_kw)
    try:
        if ids is not None:
            e.ids(*ids)
        paths = [str(tmp_path / ("%s.o%d.gz" % (tag, k + 1))) for k in range(e.sides)]
        e.outputs(paths[0], paths[1] if e.sides == 2 else None, compression_level=level)
        for i, (a, b) in enumerate(feeds):
            e.feed(a, b, last=i == len(feeds) - 1)
        st = e.result()
    finally:
        e.close()
    for p in paths:
        assert open(p, "rb").read()[-28:] == EOF_MEMBER
    return [gunzip(p) for p in paths], st


def same_as_model(out, st, r):
    assert out == r.out
    assert st["entries"] == r.stats["entries"] and st["written"] == r.stats["written"] and st["bytes"] == r.stats["bytes"] and st["err_entry"] == -1


def both(t1, t2, size1, size2=None):
    """the two texts in pieces of size1 / size2 bytes, and an empty last feed"""
    if t2 is None:
        return [(t1[i:i + size1], None) for i in range(0, len(t1), size1)] + [(b"", None)]
    n = max((len(t1) + size1 - 1) // size1, (len(t2) + size2 - 1) // size2)
    return [(t1[size1 * i:size1 * i + size1], t2[size2 * i:size2 * i + size2]) for i in range(n)] + [(b"", b"")]


@pytest.mark.parametrize("gi", range(len(K.catalogue())))
def test_plan_row_for_row(gi):
    g = K.catalogue()[gi]
    t1, t2, r = model(g)
    got = ngsqc.fastq_edit_plan(t1, t2, ids=g.ids, **g.lib_kw())
    assert got.shape == r.plan.shape
    bad = np.nonzero((got != r.plan).any(axis=tuple(range(1, got.ndim))))[0]
    assert len(bad) == 0, [(g.entries[i][0], got[i].tolist(), r.plan[i].tolist()) for i in bad[:5]]


@pytest.mark.parametrize("gi", range(len(K.catalogue())))
def test_outputs_and_statistics_whole(tmp_path, gi):
    g = K.catalogue()[gi]
    t1, t2, r = model(g)
    same_as_model(*run_edit(g.lib_kw(), g.ids, tmp_path, [(t1, t2)], "w"), r)


@pytest.mark.parametrize("name", ["trim-lines-differ", "convert", "umi-headers", "extract"])
def test_line_structure(tmp_path, name):
    g = K.by_name(name)
    _, _, r = model(g)
    blank = tuple(None if t is None else t + b"\n\r\n\n" for t in g.texts())
    for tag, (t1, t2) in (("crlf", g.texts(crlf=True)), ("nonl", g.texts(final_newline=False)), ("blank", blank)):
        same_as_model(*run_edit(g.lib_kw(), g.ids, tmp_path, [(t1, t2)], tag), r)


@pytest.mark.parametrize("name", ["extract", "extract-v", "extract-many", "extract-many-v", "extract-long-read"])
def test_every_probe_collides(tmp_path, monkeypatch, name):
    """NGSQC_NAME_HASH_BITS=4: sixteen hash values for all ids, so nearly every probe meets other ids first and is decided by comparing the bytes"""
    monkeypatch.setenv("NGSQC_NAME_HASH_BITS", "4")
    g = K.by_name(name)
    t1, t2, r = model(g)
    assert np.array_equal(ngsqc.fastq_edit_plan(t1, t2, ids=g.ids, **g.lib_kw()), r.plan)
    same_as_model(*run_edit(g.lib_kw(), g.ids, tmp_path, both(t1, None, 4001), "h"), r)


@pytest.mark.parametrize("name", ["trim-thresholds", "extract"])
def test_cut_at_every_byte(tmp_path, name):
    g = K.by_name(name)
    t1, _, r = model(g)
    same_as_model(*run_edit(g.lib_kw(), g.ids, tmp_path, both(t1, None, 1), "b"), r)


def test_cut_at_every_byte_with_differing_cuts_on_the_two_sides(tmp_path):
    """side 1 byte by byte while side 2 comes in pieces of 7 bytes, and the other way round"""
    g = K.by_name("umi-headers")
    t1, t2, r = model(g)
    same_as_model(*run_edit(g.lib_kw(), None, tmp_path, both(t1, t2, 1, 7), "a"), r)
    same_as_model(*run_edit(g.lib_kw(), None, tmp_path, both(t1, t2, 7, 1), "b"), r)


@pytest.mark.parametrize("ahead", [0, 1])
def test_one_side_hundreds_of_entries_ahead(tmp_path, ahead):
    rng = random.Random(5)
    e1 = [K.entry(rng, "p%d" % i, 20 + i % 50, header=("@p%d 1:N" % i).encode()) for i in range(600)]
    e2 = [K.entry(rng, "p%d" % i, 10 + i % 70, header=("@p%d 2:N" % i).encode()) for i in range(600)]
    g = K.Group("umi-many", "umi", dict(cut1=9, cut2=11), e1, e2)
    t1, t2, r = model(g)
    t = [t1, t2]
    lead, lag = t[ahead], t[1 - ahead]
    cuts = [0, 1000, 1001, len(lag) // 3, len(lag) // 2 + 5, len(lag)]
    feeds = []
    for i in range(len(cuts) - 1):
        a = lead if i == 0 else b""            # the whole of one side at once, the other in five pieces cut anywhere
        b = lag[cuts[i]:cuts[i + 1]]
        feeds.append((a, b) if ahead == 0 else (b, a))
    same_as_model(*run_edit(g.lib_kw(), None, tmp_path, feeds, "s%d" % ahead), r)


@pytest.mark.parametrize("op", ["trim", "extract", "convert", "umi"])
def test_an_entry_longer_than_a_piece_straddles_windows(tmp_path, monkeypatch, op):
    """one entry of 70 000 bases in about 200 KB of text, windows of one BGZF piece (0xff00 bytes): the entry is written by several launches of the format kernel"""
    monkeypatch.setenv("NGSQC_WRITE_WINDOW_PIECES", "1")
    _, t = K.big()
    kw, ids, t2 = dict(trim=(dict(long_read=True, start=7, end=9, len=69000), None, None), extract=(dict(long_read=True), ([b"big", b"s3", b"t59", b"s100"], [69999, None, 7, 0]), None),
                       convert=(dict(), None, None), umi=(dict(cut1=12, cut2=5), None, t[:len(t) // 2 + 40000]))[op]
    r = M.run(op, t, t2, ids=ids, **kw)
    assert r.error is None and max(len(x) for x in r.out) > 2 * 0xff00 and r.plan.reshape(-1, 8)[:, 4].max() > 0xff00
    if op != "umi":
        assert np.array_equal(ngsqc.fastq_edit_plan(t, ids=ids, op=op, **kw), r.plan)
    for tag, size, level in (("whole", 1 << 30, 1), ("pieces", 50000, 0)):
        same_as_model(*run_edit(dict(op=op, **kw), ids, tmp_path, both(t, t2, size, size), tag, level=level), r)


def test_first_failing_entry():
    for name, text, long_read, kind, entry, msg in K.error_cases():
        e = ngsqc.FastqEdit("extract", long_read=long_read)
        with pytest.raises(ngsqc.NgsqcError) as x:
            e.feed(text, last=True)
        assert x.value.code == -2 and msg in str(x.value), (name, str(x.value))
        assert e.error == (entry, kind), name
        e.close()


def test_first_failing_entry_when_two_fail_in_different_pieces(tmp_path):
    rng = random.Random(3)
    ok = lambda n: K.entry(rng, n, 30)[1]
    es = [ok("a"), ok("b"), (b"@c", b"ACGT", b"+", b"II I"), ok("d"), ok("e"), (b"f", b"A", b"+", b"I"), ok("g")]
    text = b"".join(l + b"\n" for e in es for l in e)
    cut1, cut2 = text.index(b"\n@c\n") + 1, text.index(b"\n@e\n") + 5
    e = ngsqc.FastqEdit("extract")
    e.ids([b"a"])
    e.outputs(str(tmp_path / "o.gz"))
    e.feed(text[:cut1])                                   # two good entries
    with pytest.raises(ngsqc.NgsqcError) as x:
        e.feed(text[cut1:cut2])                           # the piece with entry 2
    assert e.error == (2, 5) and "Invalid quality character ' ' with value '32' encountered in sequence '@c'." in str(x.value)
    with pytest.raises(ngsqc.NgsqcError) as x:
        e.feed(text[cut2:], last=True)                    # the piece with entry 5: the accumulator is void, the first error stays
    assert x.value.code == -2 and e.error == (2, 5) and "'@c'" in str(x.value)
    e.close()


def test_small_feeds_empty_input_and_everything_dropped(tmp_path):
    g = K.by_name("trim-kept-sizes")
    t1, _, r = model(g)
    # feeds that complete no entry: pieces without a line end, then three lines of the first entry
    first = t1.index(b"\n", t1.index(b"\n+\n") + 3) + 1
    feeds = [(t1[:3], None), (t1[3:5], None), (t1[5:first - 1], None), (t1[first - 1:], None), (b"", None)]
    same_as_model(*run_edit(g.lib_kw(), None, tmp_path, feeds, "n"), r)
    # an empty input
    out, st = run_edit(dict(op="convert"), None, tmp_path, [(b"", None)], "e")
    assert out == [b""] and st["entries"] == 0 and st["written"] == [0, 0] and st["bytes"] == [0, 0]
    out, st = run_edit(dict(op="umi", cut1=3), None, tmp_path, [(b"", b"\n\n")], "e2")
    assert out == [b"", b""] and st["entries"] == 0
    # every entry dropped: an empty but valid gzip file
    out, st = run_edit(dict(op="trim", start=1000), None, tmp_path, [(t1, None)], "d")
    assert out == [b""] and st["entries"] == len(g.entries) and st["written"] == [0, 0] and st["bytes"] == [0, 0]
    assert ngsqc.fastq_edit_plan(t1, op="trim", start=1000)[:, 0].tolist() == [0] * len(g.entries)
    out, st = run_edit(dict(op="extract"), ([], None), tmp_path, [(t1, None)], "x")
    assert out == [b""] and st["entries"] == len(g.entries)


def test_refusals(tmp_path):
    for kw, msg in ((dict(op="trim", start=-1), "must not be negative"), (dict(op="trim", max_len=-5), "must not be negative"), (dict(op="umi", cut2=-1), "must not be negative")):
        with pytest.raises(ngsqc.NgsqcError) as x:
            ngsqc.FastqEdit(**kw)
        assert x.value.code == -3 and msg in str(x.value)
    e = ngsqc.FastqEdit("trim")
    for call, msg in ((lambda: e.ids([b"a"]), "only FastqExtract takes ids"), (lambda: e.outputs(str(tmp_path / "a"), str(tmp_path / "b")), "one output"),
                      (lambda: e.outputs(str(tmp_path / "a"), compression_level=10), "compression level 10 is not in 0..9"), (lambda: e.feed(b"@a\n", b"@a\n"), "one input")):
        with pytest.raises(ngsqc.NgsqcError) as x:
            call()
        assert x.value.code == -3 and msg in str(x.value)
    e.close()
    e = ngsqc.FastqEdit("umi")
    with pytest.raises(ngsqc.NgsqcError) as x:
        e.outputs(str(tmp_path / "a"))
    assert x.value.code == -3 and "out2 is needed" in str(x.value)
    e.close()
