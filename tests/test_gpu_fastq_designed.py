"""FastqStats (include/ngsqc.h ngsqc_fastq_*: the line index and the entry kernel of csrc/fastqin.hip, the carry of the accumulator) against the Python model
(tests/fastq_model.py) on the designed texts of tests/fastq_cases.py: field for field, every value an integer. Fed whole and in pieces of 1, 7 and 4096 bytes and of
one entry, forward and reverse, with and without long_read; the (entry, kind) and the message of every error case."""
import importlib

import numpy as np
import pytest

import fastq_cases as K
import fastq_model as M

ngsqc = importlib.import_module("ngs-bits_amd")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def designed():
    out = {}
    for long_read in (False, True):
        text = K.designed(long_read)
        out[long_read] = (text, {rev: M.run([(text, rev)], long_read) for rev in (False, True)})
    return out


def same(got, exp):
    assert sorted(got) == sorted(exp)
    for k in exp:
        assert np.array_equal(np.asarray(got[k]), np.asarray(exp[k])), k


def pieces(text, size):
    if size == "entry":
        cuts = [i + 1 for i, c in enumerate(text) if c == 10][3::4]
        return [text[a:b] for a, b in zip([0] + cuts, cuts + [len(text)])]
    return [text[i:i + size] for i in range(0, len(text), size)] or [b""]


def feed(files, long_read=False, size=None):
    """files: [(text, reverse)]; every file is ended with last. Returns the FastqStats."""
    f = ngsqc.FastqStats(long_read=long_read)
    for text, rev in files:
        ps = [text] if size is None else pieces(text, size)
        for i, p in enumerate(ps):
            f.feed(p, int(rev), last=i == len(ps) - 1)
    return f


@pytest.mark.parametrize("long_read", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
def test_designed_text_whole(designed, long_read, reverse):
    text, exp = designed[long_read]
    st, index, err = exp[reverse]
    assert err is None
    f = feed([(text, reverse)], long_read)
    same(f.result(), st.fields())
    assert f.report["entries"] == index[0] and f.report["files"] == 1 and f.report["err_kind"] == 0 and f.report["err_entry"] == -1


@pytest.mark.parametrize("size,long_read,reverse", [(1, False, False), (7, False, True), (7, True, False), (4096, False, False), (4096, True, True), ("entry", False, True), ("entry", True, False)])
def test_designed_text_in_pieces(designed, size, long_read, reverse):
    text, exp = designed[long_read]
    st, index, _ = exp[reverse]
    f = feed([(text, reverse)], long_read, size)
    same(f.result(), st.fields())
    assert f.report["entries"] == index[0]


def test_sizes_line_endings_and_file_ends(designed):
    for name, text in K.size_cases().items():
        st, index, err = M.run([(text, False)])
        for size in (None, 7):
            f = feed([(text, False)], size=size)
            same(f.result(), st.fields())
            assert f.report["entries"] == index[0], name
    text, exp = designed[False]
    for name, v in K.variants(text).items():
        for size in (None, 7, 4096):
            f = feed([(v, False)], size=size)
            same(f.result(), exp[False][0].fields())
            assert f.report["entries"] == exp[False][1][0], (name, size)


def test_files_in_a_row_forward_and_reverse(designed):
    """ReadQC's loop: in1[0], in2[0], in1[1], ... into one accumulator; `last` resets the line phase (the first file ends inside an entry's worth of blank lines)"""
    a, b = designed[False][0], K.sized(3 * K.B)
    files = [(a + b"\n\n", False), (b[:-1], True), (K.size_cases()["one-entry"], False), (b"", True)]
    st, index, err = M.run(files)
    assert err is None and index[3] == 0
    for size in (None, 4096):
        f = ngsqc.FastqStats()
        for k, (text, rev) in enumerate(files):
            ps = [text] if size is None else pieces(text, size)
            for i, p in enumerate(ps):
                f.feed(p, int(rev), last=i == len(ps) - 1)
            f.result()
            assert f.report["entries"] == index[k] and f.report["files"] == k + 1
        same(f.result(), st.fields())


def test_reads_longer_than_the_dense_length_histogram():
    """lengths of 2^20 and more leave the histogram through a list (FQ_LEN_DENSE in csrc/fastq_visit.h)"""
    rng = np.random.default_rng(5)
    b = K.Builder()
    for n in ((1 << 20) - 1, 1 << 20, (1 << 20) + 5, 100, 1 << 20):
        b.add(K._bases(rng, n), K._quals(rng, n, 2, 90))
    text = b.text()
    st, index, err = M.run([(text, False)], True)
    assert err is None
    for size in (None, 1 << 20):
        f = feed([(text, False)], True, size)
        got = f.result()
        same(got, st.fields())
        assert got["read_lengths"][1 << 20] == 2


@pytest.mark.parametrize("long_read", [False, True])
def test_error_cases(long_read):
    for name, text, expect, cut in K.error_cases(long_read):
        _, _, err = M.run([(text, False)], long_read)
        assert (err[1], err[2]) == expect
        ways = [[text], pieces(text, 7), pieces(text, 4096)] + ([[text[:cut], text[cut:]]] if cut is not None else [])
        for ps in ways:
            f = ngsqc.FastqStats(long_read=long_read)
            with pytest.raises(ngsqc.NgsqcError) as e:
                for i, p in enumerate(ps):
                    f.feed(p, 0, last=i == len(ps) - 1)
            assert e.value.code == -2 and str(e.value).endswith(err[3]), (name, str(e.value), err[3])
            assert (f.report["err_file"], f.report["err_entry"], f.report["err_kind"]) == (0, expect[0], expect[1]), name


def test_error_in_the_second_file():
    good = K.size_cases()["B+1"]
    name, text, expect, _ = K.error_cases()[0]
    f = ngsqc.FastqStats()
    f.feed(good, 0, last=True)
    with pytest.raises(ngsqc.NgsqcError):
        f.feed(text, 1, last=True)
    assert (f.report["err_file"], f.report["err_entry"], f.report["err_kind"]) == (1, expect[0], expect[1])
    with pytest.raises(ngsqc.NgsqcError):      # the accumulator is void from the first error on
        f.feed(good, 0, last=True)
