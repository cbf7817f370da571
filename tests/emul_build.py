"""The one recipe for the CPU builds of the device text (tests/emul/*.cpp): library() for a shared library that a test loads, program() for a stand-alone
program, sanitized or not. The compiler names what a build read (-MMD), so a library is rebuilt when anything it was made from changed - a header reached
only through another header included - or when its command line did. Nothing sanitized is ever loaded into python: the sanitizers get programs of their own."""
import os
import shlex
import subprocess

EMUL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul")
BASE = ["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _source(src):
    return src if os.path.isabs(src) else os.path.join(EMUL, src)


def _includes(include):
    return [w for d in include for w in ("-I", str(d))]


def _fresh(out, line):
    """out is younger than every file its dependency file names, and that file begins with this command line"""
    try:
        built = os.stat(out).st_mtime_ns
        with open(out + ".d") as f:
            first, rules = f.read().split("\n", 1)
        deps = rules.replace("\\\n", " ").split(": ", 1)[1].split()
        return first == "# " + line and all(os.stat(p).st_mtime_ns <= built for p in deps)
    except (OSError, ValueError, IndexError):   # no output, no or a torn dependency file, a file it names is gone
        return False


def library(src, out=None, include=(), flags=()):
    """-> the path of the shared library of one source (a name under tests/emul/, or a path), by default tests/emul/lib<name minus _emul>.so; built only when
    it is not fresh. The new file is written beside the old one and moved into place, so no half-written library ever carries the name."""
    src = _source(src)
    out = os.path.abspath(out or os.path.join(EMUL, "lib" + os.path.basename(src)[:-len(".cpp")].replace("_emul", "") + ".so"))
    cmd = BASE + ["-O2", "-shared", "-fPIC", *flags, *_includes(include), "-o", out, src]
    line = shlex.join(cmd)
    if not _fresh(out, line):
        tmp = "%s.%d.tmp" % (out, os.getpid())
        try:
            subprocess.check_call(cmd[:-2] + [tmp, "-MMD", "-MF", tmp + ".d", src])
            with open(tmp + ".d") as f:
                rules = f.read()
            with open(tmp + ".d", "w") as f:
                f.write("# " + line + "\n" + rules)
            os.replace(tmp + ".d", out + ".d")
            os.replace(tmp, out)
        finally:
            for p in (tmp, tmp + ".d"):
                if os.path.exists(p):
                    os.remove(p)
    return out


_programs = {}


def program(src, outdir, include=(), flags=(), sanitize=False):
    """-> the path of the program of one source (it has a main), built into outdir; once per process for the same source and flags. sanitize: under
    AddressSanitizer and UBSan with the runtimes linked statically - such a program starts whatever else the environment preloads into it, where a shared
    AddressSanitizer runtime refuses to run unless it comes first among the libraries. Only where that link fails are the shared runtimes linked."""
    src = _source(src)
    opts = (SANITIZE if sanitize else ["-O2"]) + [*flags]
    key = (src, *opts, *_includes(include))
    if key not in _programs or not os.path.exists(_programs[key]):
        exe = os.path.join(str(outdir), os.path.basename(src)[:-len(".cpp")])
        subprocess.check_call(BASE + opts + _includes(include) + ["-c", "-o", exe + ".o", src])
        link = BASE[:1] + opts + ["-o", exe, exe + ".o"]
        if not sanitize or subprocess.run(link + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
            subprocess.check_call(link)
        _programs[key] = exe
    return _programs[key]
