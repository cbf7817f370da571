"""The BAM-output path the six record-rewriting tools share (csrc/recwrite.h open_bam, csrc/join.h BgzfStream::put_host / place / close) on a header that is
larger than two output windows at NGSQC_WRITE_WINDOW_PIECES=1: every tool writes the same bytes with the default window and with windows of one piece, the
inflated output begins with the input's header bytes, and its records and counts are those of the tool's Python restatement."""
import gzip
import os
import struct

import pytest

import bamcleanhaloplex_oracle as HX
import bamclipoverlap_oracle as CL
import bamdownsample_oracle as DS
import bamextract_oracle as EX
import bamfilter_oracle as F
import bamremovevariants_oracle as RM
import cram_twin

ngsqc = __import__("importlib").import_module("ngs-bits_amd")

PIECE = 0xff00
N_SQ = 4000
LISTED = b"pair1"


def _record(name, flag, pos, mpos, isize, seed):
    """a mapped 50M read on c0000 with its mate at mpos; bases of A, C, G, T alone"""
    n = name + b"\0"
    l_seq = 50
    seq = bytes(((1 << ((seed + 2 * i) % 4)) << 4) | (1 << ((seed + 2 * i + 1) % 4)) for i in range(l_seq // 2))
    qual = bytes(20 + (seed + i) % 20 for i in range(l_seq))
    aux = b"NMC" + bytes([0])
    body = struct.pack("<iiBBHHHiiii", 0, pos, len(n), 60, 4680, 1, flag, l_seq, 0 if flag & 1 else -1, mpos, isize) + n + struct.pack("<I", l_seq << 4) + seq + qual + aux
    return struct.pack("<I", len(body)) + body


def input_records():
    """two proper pairs (the mates overlap by 20 bases) and one single-end read"""
    return [_record(b"pair1", 0x63, 1000, 1030, 80, 0), _record(b"pair1", 0x93, 1030, 1000, -80, 1), _record(b"single", 0x0, 2000, -1, 0, 2),
            _record(b"pair2", 0x63, 3000, 3030, 80, 3), _record(b"pair2", 0x93, 3030, 3000, -80, 0)]


def input_bam_bytes():
    text = "@HD\tVN:1.6\n" + "".join(f"@SQ\tSN:c{i:04d}\tLN:1000\n" for i in range(N_SQ))
    raw = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", N_SQ)
    raw += b"".join(struct.pack("<i", 6) + f"c{i:04d}".encode() + b"\0" + struct.pack("<i", 1000) for i in range(N_SQ))
    raw += b"".join(input_records())
    return b"".join(cram_twin._bgzf(raw[o:o + 60000]) for o in range(0, len(raw), 60000)) + cram_twin._bgzf(b"")


# per tool: (the call on a handle -> (counts, [output paths]), the restatement -> (counts in the call's shape, [records per output]))
def _filter_expected(header, recs):
    out, passed, dropped = F.filter_pairs(recs, **OPEN_LIMITS)
    return (passed, dropped), [out]


def _downsample_expected(header, recs):
    out, _, c, _ = DS.downsample(recs, 99, 1)
    return c, [out]


def _extract_expected(header, recs):
    e1, e2, c = EX.extract(recs, {LISTED}, True)
    return c, [e1, e2]


def _rmvar_expected(header, recs):
    out, c = RM.run(recs, [], RM.ref_names_of(header))
    return c, [out]


def _clip_expected(header, recs):
    r = CL.run(header, recs, 0, False, False)
    return dict(zip(ngsqc.CLIP_COUNT_NAMES, r.counts)), [r.records]


def _haloplex_expected(header, recs):
    _, out, c = HX.clean(recs, 0)
    return c, [out]


OPEN_LIMITS = dict(min_mq=0, max_mq=256, max_mm=-1, max_gap=-1, min_dup=0, max_is=-1)
TOOLS = {
    "BamFilter": (lambda h, o: (h.filter_pairs(o[0], **OPEN_LIMITS), o[:1]), _filter_expected),
    "BamDownsample": (lambda h, o: (h.downsample(o[0], 99, 1), o[:1]), _downsample_expected),
    "BamExtract": (lambda h, o: (h.extract(o[0], [LISTED], o[1]), o), _extract_expected),
    "BamRemoveVariants": (lambda h, o: (h.remove_variants(o[0], []), o[:1]), _rmvar_expected),
    "BamClipOverlap": (lambda h, o: (h.clip_overlap(o[0], 0), o[:1]), _clip_expected),
    "BamCleanHaloplex": (lambda h, o: (h.clean_haloplex(o[0], 0), o[:1]), _haloplex_expected),
}


def test_restatements_keep_records():
    """the chosen parameters leave every output of every tool non-empty (no device: the restatements alone)"""
    header, recs = F.read_bam(input_bam_bytes())
    assert len(header) > 2 * PIECE and len(recs) == 5
    for tool, (_, expected) in TOOLS.items():
        assert all(len(out) > 0 for out in expected(header, recs)[1]), tool


@pytest.fixture(scope="module")
def big_header(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("hdrwin") / "in.bam")
    open(path, "wb").write(input_bam_bytes())
    header, recs = F.read_bam(path)   # (Python's gzip and struct on the input file, not the library)
    assert len(header) > 2 * PIECE
    return dict(path=path, header=header, recs=recs)


def _run(tool, src, outs, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    h = ngsqc.Handle(path=src)
    try:
        return TOOLS[tool][0](h, outs)
    finally:
        h.close()
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


@pytest.mark.gpu
@pytest.mark.parametrize("tool", sorted(TOOLS))
def test_header_of_three_windows(tmp_path, big_header, tool):
    D = big_header
    exp_counts, exp_outs = TOOLS[tool][1](D["header"], D["recs"])
    got, paths = _run(tool, D["path"], [str(tmp_path / "a.bam"), str(tmp_path / "a2.bam")], {})
    got1, paths1 = _run(tool, D["path"], [str(tmp_path / "w.bam"), str(tmp_path / "w2.bam")], {"NGSQC_WRITE_WINDOW_PIECES": "1"})
    assert got == exp_counts and got1 == exp_counts, (got, got1, exp_counts)
    assert len(paths) == len(exp_outs)
    for p, p1, exp in zip(paths, paths1, exp_outs):
        data = open(p, "rb").read()
        assert data == open(p1, "rb").read()
        assert gzip.decompress(data).startswith(D["header"])
        header, recs = F.read_bam(data)
        assert header == D["header"] and len(exp) > 0 and recs == exp
