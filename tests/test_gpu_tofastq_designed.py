"""BamToFastq's kernels on the GPU (csrc/fastq.hip: fq_keys_kernel, fq_fix_kernel / fq_fix_store_kernel, fq_pair_sizes_kernel, fq_format_kernel over
csrc/tofastq_visit.h and csrc/join.h) over the designed runs of tests/tofastq_cases.py through Handle.to_fastq, at the default geometry, with one BGZF member
per tile, and with 2 and 4 hash bits; the format cuts also with windows of one piece. Text and counts must be bamtofastq_oracle's - for a run that throws, the
base of the first throwing entry in output order - and the bytes must not depend on the geometry."""
import pytest

import tofastq_cases as K
from test_gpu_bamtofastq import text_of, with_env

ngsqc = __import__("importlib").import_module("ngs-bits_amd")
pytestmark = pytest.mark.gpu

GEOMETRIES = [{}, {"NGSQC_TILE_MEMBERS": "1"}, {"NGSQC_TILE_MEMBERS": "1", "NGSQC_NAME_HASH_BITS": "2"}, {"NGSQC_TILE_MEMBERS": "1", "NGSQC_NAME_HASH_BITS": "4"}]


def device(path, o1, o2, kw):
    kw = dict(kw); paired = kw.pop("paired", True)
    h = ngsqc.Handle(path=path)
    try:
        c = h.to_fastq(o1, o2 if paired else None, **kw)
        return c, open(o1, "rb").read(), (open(o2, "rb").read() if paired else None)
    finally:
        h.close()


def check(tmp_path, run, geometries):
    path = run.write(str(tmp_path / (run.name + ".bam")))
    o1, o2 = str(tmp_path / "o1.gz"), str(tmp_path / "o2.gz")
    exp = run.expected()
    ref = None
    for env in geometries:
        if run.error:
            with pytest.raises(ngsqc.NgsqcError) as e:
                with_env(env, lambda: device(path, o1, o2, run.kw))
            assert e.value.code == -2 and "Could not convert base '%s' to complement!" % run.error in str(e.value), (run.name, env, str(e.value))
            continue
        got = with_env(env, lambda: device(path, o1, o2, run.kw))
        if ref is None:
            e1, e2, c = exp
            print(run.name, "got", got[0], "expected", c)
            assert got[0] == c, run.name
            assert text_of(o1) == e1, run.name
            if e2 is not None:
                assert text_of(o2) == e2, run.name
            ref = got
        else:
            assert got == ref, (run.name, env)


@pytest.mark.parametrize("group", ["bases", "qualities", "throws", "fix", "region", "max_cached"])
def test_designed_runs(tmp_path, group):
    for run in getattr(K, group)():
        check(tmp_path, run, GEOMETRIES)


def test_names_with_more_than_one_nul(tmp_path):
    """the "@" line ends where gzputs ends it: at the name's first NUL"""
    import join_cases as J
    tiles = J.c_string_names().tiles
    for kw in (dict(), dict(fix=True), dict(paired=False)):
        check(tmp_path, K.Run("c_string_names", tiles, kw), GEOMETRIES)
    # with -fix, "ab\0" and "ab\0\0\0" as read 1 are one (name, read 1): the second is skipped
    twice = K.Run("c_string_fix", [[K.fq(b"ab\0", K.F1, "ACGT")], [K.fq(b"ab\0\0\0", K.F1, "ACGT"), K.fq(b"ab\0cd\0", K.F2, "ACGT")]], dict(fix=True))
    assert twice.expected()[2]["fixed"] == 1 and twice.expected()[2]["paired"] == 1
    check(tmp_path, twice, GEOMETRIES)


def test_format_cuts(tmp_path):
    run = K.format_cuts()
    e1, e2, _ = run.expected()
    K.format_cut_premises(run, e1, e2)
    check(tmp_path, run, [{"NGSQC_WRITE_WINDOW_PIECES": "1"}, {"NGSQC_WRITE_WINDOW_PIECES": "1", "NGSQC_TILE_MEMBERS": "1"}, {}, {"NGSQC_WRITE_WINDOW_PIECES": "2", "NGSQC_NAME_HASH_BITS": "2"}])
