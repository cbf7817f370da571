"""The library's NGSQC_* environment switches are read in ONE file, ngs-bits_amd/csrc/switches.h (host-only C++): where they are read, which names exist, and how each value
is parsed. The parsing rules asserted here were read off the call sites the table replaced (one getenv + atoi + clamp per site); they are written out below by hand and are
not produced by the code under test. tests/emul/switches_dump.cpp, compiled by g++, prints both structs of switches.h under the environment it is started with."""
import glob
import os
import re
import subprocess

import pytest

import emul_build
from conftest import ROOT

CSRC = os.path.join(ROOT, "ngs-bits_amd", "csrc")
HOST = os.path.join(ROOT, "ngs-bits_amd", "host")
NAME = re.compile(r"NGSQC_[A-Z0-9_]+")
REMOVED = ["NGSQC_P1_PRIO", "NGSQC_P2_PRIO", "NGSQC_P1_WAVES", "NGSQC_P1_STREAMS", "NGSQC_K1_CHUNK_WAVES", "NGSQC_K1_CHUNK_DIV", "NGSQC_GUESS_WAVES"]


def _read(path):
    with open(path, errors="replace") as f:
        return f.read()


def _getenv_names(text):
    return set(re.findall(r'"(NGSQC_[A-Z0-9_]+)"', text))


def test_getenv_only_in_switches_h():
    hits = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(CSRC, "*"))) if os.path.isfile(p) and not p.endswith(".o") and "getenv" in _read(p)]
    assert hits == ["switches.h"]
    includes = re.findall(r'#include\s*[<"]([^>"]+)', _read(os.path.join(CSRC, "switches.h")))
    assert includes and not any("hip" in i.lower() for i in includes)   # host-only: a plain g++ compiles it


def test_names_of_the_table_the_readme_and_the_tests():
    table = _getenv_names(_read(os.path.join(CSRC, "switches.h")))
    readme = _read(os.path.join(ROOT, "README.md"))
    a = readme.index("### Environment switches of the library"); b = readme.index("### Environment switches of the host tools")
    listed = set(re.findall(r"^- `(NGSQC_[A-Z0-9_]+)`", readme[a:b], re.M))
    assert table == listed and len(table) == 40
    # what the tests and the benchmark put into the environment is read by the library's table or by the host tools
    host = set()
    for p in glob.glob(os.path.join(HOST, "*.[ch]pp")):
        host |= set(re.findall(r'getenv\("(NGSQC_[A-Z0-9_]+)"\)', _read(p)))
    used = set()
    for p in sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))) + [os.path.join(ROOT, "bench.py")]:
        if os.path.basename(p) == "test_cpu_switches.py":
            continue
        used |= set(NAME.findall(_read(p)))
    used = {n for n in used if not re.match(r"NGSQC_(BENCH_|E_|W_|SW_)", n)}
    assert used <= table | host, sorted(used - table - host)
    assert not set(REMOVED) & (table | host)


def test_removed_switches_are_gone_everywhere():
    """In the project's sources: the files at the root and everything under include/, ngs-bits_amd/, oracle/, tests/ and tools/ - outside the documents (*.md) and
    tools/dev (the probe scripts that produced the recorded profiles: kept as they ran)."""
    skip_dirs = {"dev", "__pycache__", "_ref", "bin", "variants"}
    paths = [os.path.join(ROOT, f) for f in os.listdir(ROOT) if os.path.isfile(os.path.join(ROOT, f))]
    for top in ("include", "ngs-bits_amd", "oracle", "tests", "tools"):
        for d, dirs, files in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [x for x in dirs if x not in skip_dirs]
            paths += [os.path.join(d, f) for f in files]
    found = []
    for p in paths:
        if p.endswith((".md", ".so", ".o", ".a", ".pyc", ".bam", ".cram", ".bai", ".gz", ".npy", ".bin")) or os.path.abspath(p) == os.path.abspath(__file__) or os.path.getsize(p) > (4 << 20):
            continue
        t = _read(p)
        found += [(os.path.relpath(p, ROOT), n) for n in REMOVED if re.search(n + r"(?![A-Z0-9_])", t)]
    assert len(paths) > 100 and not found, found


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = emul_build.program("switches_dump.cpp", tmp_path_factory.mktemp("switches"), flags=["-O0"])

    def run(env):
        out = subprocess.run([exe], env=env, capture_output=True, text=True, check=True).stdout
        return dict(line.split("=", 1) for line in out.splitlines())
    return run


DEFAULTS = {
    "open.tile_members": "0", "open.tile_chunks": "0", "open.token_slots": "8", "open.token_pool_factor": "1", "open.carry_max": str(64 << 20), "open.comp_slots": "0",
    "open.h2d_threads": "4", "open.h2d_piece_mb": "64", "open.h2d_delay_us": "0", "open.walk_threads": "8", "open.stream_image": "unset", "open.stream_image_min_mb": "4096",
    "open.shard_tail_members": "64", "open.async_h2d": "1", "open.async_plan": "1", "open.verify_crc": "1", "open.p1_park": "32",
    "open.cram_threads": "0", "open.cram_device_quals": "1", "open.cram_ignore_md5": "0", "open.cram_no_reference": "0", "open.cram_plan_dump": "", "open.reference": "",
    "open.debug": "0", "open.timing": "0",
    "call.pipeline": "1", "call.k1_serial": "0", "call.no_fused_scan": "0", "call.no_fused_pileup": "0", "call.k2_general": "0", "call.eager_recoff": "0",
    "call.baseq_ride": "1", "call.bq_list_cap": "0", "call.walker_shift": "0", "call.group_shift": "unset", "call.walk_waves": "unset", "call.long_read_mode": "unset",
    "call.crc_chains": "4", "call.name_hash_bits": "63", "call.write_window_pieces": "16384", "call.debug": "0", "call.timing": "0",
}


def test_defaults_with_an_empty_environment(dump):
    assert dump({}) == DEFAULTS


def _rows():
    rows = []

    def row(name, field, *pairs):
        rows.extend((name, v, field, exp) for v, exp in pairs)
    # presence-only: on when set to any value, "0" included
    for n, f in (("NO_FUSED_SCAN", "call.no_fused_scan"), ("NO_FUSED_PILEUP", "call.no_fused_pileup"), ("K2_GENERAL", "call.k2_general"), ("EAGER_RECOFF", "call.eager_recoff")):
        row(n, f, ("0", "1"), ("1", "1"), ("", "1"))
    for n in ("DEBUG", "TIMING"):
        for s in ("open", "call"):
            row(n, f"{s}.{n.lower()}", ("0", "1"), ("1", "1"))
    # on unless atoi == 0
    for n, f in (("PIPELINE", "call.pipeline"), ("BASEQ_RIDE", "call.baseq_ride")):
        row(n, f, ("0", "0"), ("1", "1"), ("2", "1"), ("x", "0"))   # (atoi("x") == 0)
    # atoi != 0
    for n, f in (("K1_SERIAL", "call.k1_serial"), ("VERIFY_CRC", "open.verify_crc"), ("CRAM_NO_REFERENCE", "open.cram_no_reference"), ("CRAM_IGNORE_MD5", "open.cram_ignore_md5")):
        row(n, f, ("0", "0"), ("1", "1"), ("-1", "1"))
    # clamped integers and factors: below, inside, above
    row("TOKEN_SLOTS", "open.token_slots", ("1", "2"), ("2", "2"), ("5", "5"), ("8", "8"), ("9", "8"))
    row("TILE_CHUNKS", "open.tile_chunks", ("0", "1"), ("-3", "1"), ("3", "3"))
    row("TILE_MEMBERS", "open.tile_members", ("0", "1"), ("-5", "1"), ("11", "11"), ("200", "200"))
    row("TOKEN_POOL_FACTOR", "open.token_pool_factor", ("0", "0.01"), ("0.001", "0.01"), ("0.01", "0.01"), ("0.5", "0.5"), ("3", "3"))
    row("CARRY_MAX", "open.carry_max", ("-1", "0"), ("0", "0"), ("4096", "4096"), (str(1 << 33), str(1 << 33)))
    row("COMP_SLOTS", "open.comp_slots", ("0", "2"), ("1", "2"), ("2", "2"), ("5", "5"), ("100", "100"))   # (min(chunks, .) is the layout's)
    row("H2D_PIECE_MB", "open.h2d_piece_mb", ("0", "1"), ("1", "1"), ("16", "16"))
    row("H2D_THREADS", "open.h2d_threads", ("0", "1"), ("-2", "1"), ("2", "2"), ("16", "16"))
    row("H2D_DELAY_US", "open.h2d_delay_us", ("-1", "0"), ("0", "0"), ("4000", "4000"))
    row("WALK_THREADS", "open.walk_threads", ("0", "1"), ("1", "1"), ("16", "16"), ("64", "64"), ("65", "64"))
    row("STREAM_IMAGE_MIN_MB", "open.stream_image_min_mb", ("-1", "0"), ("0", "0"), ("100", "100"))
    row("SHARD_TAIL_MEMBERS", "open.shard_tail_members", ("-1", "0"), ("0", "0"), ("3", "3"))
    row("CRAM_THREADS", "open.cram_threads", ("0", "1"), ("-4", "1"), ("7", "7"))
    row("BQ_LIST_CAP", "call.bq_list_cap", ("0", "1"), ("-1", "1"), ("7", "7"), ("50", "50"))   # (min(cap, .) is the scan's)
    # enumerated
    row("CRC_CHAINS", "call.crc_chains", ("1", "1"), ("2", "2"), ("3", "4"), ("4", "4"), ("0", "4"), ("8", "4"))
    row("WALKERS", "call.walker_shift", ("0", "0"), ("1", "0"), ("2", "1"), ("3", "1"), ("4", "2"), ("7", "2"), ("8", "3"), ("100", "3"))
    row("GROUP_SHIFT", "call.group_shift", ("-1", "0"), ("0", "0"), ("1", "1"), ("2", "2"), ("8", "8"), ("9", "8"))
    row("WALK_WAVES", "call.walk_waves", ("0", "0"), ("3", "3"), ("4", "4"), ("5", "5"), ("-1", "-1"))
    row("P1_PARK", "open.p1_park", ("0", "0"), ("1", "1"), ("63", "63"), ("300", "300"))   # (& 255 at launch)
    row("LONG_READ_MODE", "call.long_read_mode", ("0", "0"), ("1", "1"), ("2", "1"))
    # as the code had them
    row("NAME_HASH_BITS", "call.name_hash_bits", ("0", "1"), ("1", "1"), ("8", "8"), ("63", "63"), ("64", "63"))
    row("WRITE_WINDOW_PIECES", "call.write_window_pieces", ("0", "1"), ("-1", "1"), ("3", "3"), ("20000", "20000"))
    row("STREAM_IMAGE", "open.stream_image", ("0", "0"), ("1", "1"), ("2", "1"))
    row("ASYNC_H2D", "open.async_h2d", ("0", "0"), ("1", "1"))
    row("ASYNC_PLAN", "open.async_plan", ("0", "0"), ("1", "1"))
    row("CRAM_DEVICE_QUALS", "open.cram_device_quals", ("0", "0"), ("1", "1"))
    row("CRAM_PLAN_DUMP", "open.cram_plan_dump", ("/tmp/plan.bin", "/tmp/plan.bin"))
    row("REFERENCE", "open.reference", ("/data/genome.fa", "/data/genome.fa"), ("", ""))
    return rows


@pytest.mark.parametrize("name,value,field,expected", _rows(), ids=[f"{r[0]}={r[1]}" for r in _rows()])
def test_parsing_rule(dump, name, value, field, expected):
    got = dump({"NGSQC_" + name: value})
    want = dict(DEFAULTS); want[field] = expected
    if name in ("DEBUG", "TIMING"):   # read at open (what ngsqc_open* and its threads print) and per call
        want["open." + name.lower()] = want["call." + name.lower()] = expected
    assert got == want
