"""The SeqPurge library (include/ngsqc.h ngsqc_purge_*, csrc/purge.hip) on the designed pairs (tests/purge_cases.py) against the Python model
(tests/seqpurge_oracle.py): the plan row for row, and the outputs and counters of the accumulator under feeds cut at every byte, at differing cuts on the two
sides and with one side hundreds of entries ahead."""
import gzip
import importlib

import numpy as np
import pytest

import purge_cases as K
import seqpurge_oracle as M

pytestmark = pytest.mark.gpu
ngsqc = importlib.import_module("ngs-bits_amd")
_model = {}


def model(g):
    if g.name not in _model:
        t1, t2 = g.texts()
        _model[g.name] = (t1, t2, M.run(t1, t2, g.params(), literal=True))
    return _model[g.name]


def gunzip(path):
    with gzip.open(path, "rb") as f:
        return f.read()


def run_purge(g, tmp_path, feeds, tag):
    """feeds: [(piece 1, piece 2)]; the last one ends the file pair. -> ([out1, out2, out3_R1, out3_R2] texts, statistics)"""
    p = ngsqc.Purge(**g.params().kwargs())
    o3 = str(tmp_path / (tag + "o3")) if g.out3 else None
    p.outputs(str(tmp_path / (tag + "o1.gz")), str(tmp_path / (tag + "o2.gz")), o3, compression_level=1)
    for i, (a, b) in enumerate(feeds):
        p.feed(a, b, last=i == len(feeds) - 1)
    st = p.result()
    p.close()
    out = [gunzip(tmp_path / (tag + "o1.gz")), gunzip(tmp_path / (tag + "o2.gz"))]
    out += [gunzip(o3 + "_R1.fastq.gz"), gunzip(o3 + "_R2.fastq.gz")] if o3 else [b"", b""]
    return out, st


def same_as_model(out, st, r):
    assert out == r.out
    for k, v in r.stats.counters.items():
        assert int(st[k]) == v, k
    assert st["pairs"] == len(r.plan) and st["err_pair"] == -1
    assert st["bases_perc_trim_sum"] == r.stats.bases_perc_trim_sum
    assert np.array_equal(st["bases_remaining"], r.stats.bases_remaining)
    assert np.array_equal(st["acons"], r.stats.acons)
    assert np.array_equal(np.stack([st["ec_mismatch_r1"], st["ec_mismatch_r2"], st["ec_errors_per_read"]]), r.stats.ec)


@pytest.mark.parametrize("gi", range(len(K.catalogue())))
def test_plan_row_for_row(gi):
    g = K.catalogue()[gi]
    t1, t2, r = model(g)
    got = ngsqc.purge_plan(t1, t2, **g.params().kwargs())
    assert got.shape == r.plan.shape
    bad = np.nonzero((got != r.plan).any(axis=1))[0]
    assert len(bad) == 0, [(g.cases[i].name, got[i].tolist(), r.plan[i].tolist()) for i in bad[:5]]


@pytest.mark.parametrize("gi", range(len(K.catalogue())))
def test_outputs_and_counters_whole(tmp_path, gi):
    g = K.catalogue()[gi]
    t1, t2, r = model(g)
    same_as_model(*run_purge(g, tmp_path, [(t1, t2)], "w"), r)


def test_line_structure(tmp_path):
    g = K.catalogue()[0]
    _, _, r = model(g)
    for tag, (t1, t2) in (("crlf", g.texts(crlf=True)), ("nonl", g.texts(final_newline=False)), ("blank", tuple(t + b"\n\r\n\n" for t in g.texts()))):
        same_as_model(*run_purge(g, tmp_path, [(t1, t2)], tag), r)


def test_cut_at_every_byte(tmp_path):
    """a small file pair: fed byte by byte on side 1 while side 2 comes in pieces of 7 bytes, and the other way round"""
    g = [x for x in K.catalogue() if x.name == "ec"][0]
    t1, t2, r = model(g)
    n = max(len(t1), (len(t2) + 6) // 7)
    feeds = [(t1[i:i + 1], t2[7 * i:7 * i + 7]) for i in range(n)] + [(b"", b"")]
    same_as_model(*run_purge(g, tmp_path, feeds, "a"), r)
    n = max((len(t1) + 6) // 7, len(t2))
    feeds = [(t1[7 * i:7 * i + 7], t2[i:i + 1]) for i in range(n)] + [(b"", b"")]
    same_as_model(*run_purge(g, tmp_path, feeds, "b"), r)


@pytest.mark.parametrize("ahead", [0, 1])
def test_one_side_hundreds_of_entries_ahead(tmp_path, ahead):
    g = [x for x in K.catalogue() if x.name == "lanes"][0]
    t1, t2, r = model(g)
    t = [t1, t2]
    lead, lag = t[ahead], t[1 - ahead]
    cuts = [0, 1000, 1001, len(lag) // 3, len(lag) // 2 + 5, len(lag)]
    feeds = []
    for i in range(len(cuts) - 1):
        a = lead if i == 0 else b""            # the whole of one side at once, the other in five pieces cut anywhere
        b = lag[cuts[i]:cuts[i + 1]]
        feeds.append((a, b) if ahead == 0 else (b, a))
    same_as_model(*run_purge(g, tmp_path, feeds, "s%d" % ahead), r)


def test_errors():
    for name, t1, t2, kind, pair, msg in K.error_cases():
        p = ngsqc.Purge()
        with pytest.raises(ngsqc.NgsqcError) as e:
            p.feed(t1, t2, last=True)
        assert e.value.code == -2 and msg in str(e.value), (name, str(e.value))
        assert p.error == (pair, kind), name
        p.close()


def test_create_refuses():
    for kw, msg in ((dict(a1=b"ACGT"), "Forward adapter ACGT too short!"), (dict(a2=b"ACGTACGTACGTAC"), "Reverse adapter ACGTACGTACGTAC too short!"),
                    (dict(a1=b"ACGTACGTACGTACGU"), "only A, C, G, T and N"), (dict(qwin=0), "qwin")):
        with pytest.raises(ngsqc.NgsqcError) as e:
            ngsqc.Purge(**kw)
        assert e.value.code == -3 and msg in str(e.value)
