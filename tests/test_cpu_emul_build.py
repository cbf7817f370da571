"""tests/emul_build.py itself, on a source of three lines in tmp_path: a.cpp includes one.h, one.h includes two.h, two.h holds the value - the header reached
only through another header is what a hand-written list of sources misses."""
import ctypes as C
import os
import subprocess

import pytest

import emul_build


def value(so, tmp_path, k):
    """what a_value() of the library returns (a copy is loaded: one path is mapped once per process)"""
    copy = tmp_path / ("loaded%d.so" % k)
    copy.write_bytes(open(so, "rb").read())
    return C.CDLL(str(copy)).a_value()


def later(path, than):
    """path just younger than `than`, and older than anything built from now on"""
    t = os.stat(than).st_mtime_ns + 1000
    os.utime(path, ns=(t, t))


def test_library_is_rebuilt_exactly_when_it_is_stale(tmp_path):
    src, one, two, out = tmp_path / "a.cpp", tmp_path / "one.h", tmp_path / "two.h", str(tmp_path / "liba.so")
    src.write_text('#include "one.h"\nextern "C" int a_value() { return VALUE; }\n')
    one.write_text('#include "two.h"\n')
    two.write_text("#define VALUE 1\n")

    def build(*flags):
        assert emul_build.library(str(src), out, flags=flags) == out
        return os.stat(out).st_mtime_ns
    first = build()                                            # 1. a first call builds
    assert value(out, tmp_path, 1) == 1
    assert build() == first                                    # 2. a second call does not
    two.write_text("#define VALUE 2\n"); later(two, out)       # 3. a header behind a header changed
    third = build()
    assert third != first and value(out, tmp_path, 3) == 2
    fourth = build("-DUNUSED")                                 # 4. another flag
    assert fourth != third and build("-DUNUSED") == fourth
    two.unlink(); one.write_text("#define VALUE 5\n"); later(one, out)   # 5. a header the last build read is gone
    assert build("-DUNUSED") != fourth and value(out, tmp_path, 5) == 5


def test_failed_build_raises_and_leaves_nothing(tmp_path):
    src, out = tmp_path / "a.cpp", tmp_path / "liba.so"
    src.write_text("int a_value() { return nothing; }\n")
    with pytest.raises(subprocess.CalledProcessError):
        emul_build.library(str(src), str(out))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["a.cpp"]   # 6. no output, no temporary, no dependency file
