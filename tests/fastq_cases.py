"""Designed FASTQ texts for the device's FASTQ reader (csrc/fastqin.hip): what its line index, its entry kernel and its validation can get wrong. The expected
values come from tests/fastq_model.py; this file only builds texts. B is the block of the line index (FQ_BLOCK in csrc/fastq_visit.h): a newline's place relative
to a multiple of B decides which lane, wave and workgroup finds it."""
import numpy as np

B = 4096
LENGTHS = [0, 1, 63, 64, 65, 319, 320, 321, 20011]   # around the wave (64) and the per-cycle window (320), and one read across five blocks


def _bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), n, p=[0.27, 0.22, 0.23, 0.26, 0.02]))


def _quals(rng, n, lo, hi):
    return bytes((rng.integers(lo, hi + 1, n) + 33).astype(np.uint8))


class Builder:
    def __init__(self):
        self.parts, self.n, self.k = [], 0, 0

    def add(self, bases, quals, header=None, header2=b"+"):
        if header is None:
            header = b"@r%d" % self.k
        self.k += 1
        e = header + b"\n" + bases + b"\n" + header2 + b"\n" + quals + b"\n"
        self.parts.append(e)
        self.n += len(e)

    def add_aligned(self, bases, quals, which, target, header2=b"+"):
        """an entry whose line `which` (0 header .. 3 qualities) ends with its newline at an offset = target (mod B): the header is padded to that"""
        extra = [0, 1 + len(bases), 2 + len(bases) + len(header2), 3 + len(bases) + len(header2) + len(quals)][which]
        hl = (target - self.n - extra) % B
        if hl < 8:
            hl += B
        at = self.n + hl + extra
        self.add(bases, quals, header=(b"@a%d_" % self.k).ljust(hl, b"x")[:hl], header2=header2)
        assert at % B == target % B and self.text()[at:at + 1] == b"\n"

    def text(self):
        return b"".join(self.parts)


def designed(long_read=False, seed=7):
    """One good text: every designed length and quality, newlines at the first and the last byte of a block, entries with an empty header."""
    rng = np.random.default_rng(seed)
    qmax = 93 if long_read else 41
    b = Builder()
    for n in LENGTHS:
        b.add(_bases(rng, n), _quals(rng, n, 2, 40))
    for q in (0, qmax):                                     # the quality characters at both ends of the range
        for n in (1, 65, 321):
            b.add(_bases(rng, n), bytes([q + 33]) * n)
    # means exactly at x.5, at 20.0 and (where the range has it) at 60
    b.add(b"AC", bytes([20 + 33, 21 + 33]))
    b.add(b"ACGT", bytes([0 + 33, 1 + 33, 0 + 33, 1 + 33]))
    b.add(b"ACGTNA", bytes([19 + 33, 20 + 33, 21 + 33] * 2))
    b.add(_bases(rng, 100), bytes([20 + 33]) * 100)
    b.add(_bases(rng, 7), bytes([19 + 33] * 3 + [20 + 33] * 4))            # just below 20
    b.add(_bases(rng, 64), bytes([40 + 33, 41 + 33] * 32))
    if long_read:
        b.add(_bases(rng, 10), bytes([60 + 33]) * 10)
        b.add(_bases(rng, 2), bytes([59 + 33, 60 + 33]))
        b.add(_bases(rng, 3), bytes([93 + 33]) * 3)
    # quality lines that begin with '@' and with '+', a second header that repeats the name
    b.add(b"ACGTACGT", b"@" + _quals(rng, 7, 2, 40))
    b.add(b"ACGTACGT", b"+" + _quals(rng, 7, 2, 40))
    b.add(b"ACGT", b"@@@@", header2=b"+r again")
    b.add(b"ACGT", b"++++")
    # entries with an empty header: counted, not indexed; one of them all empty
    b.add(b"ACGTN", b"IIIII", header=b"")
    b.add(b"", b"", header=b"", header2=b"")
    # newlines at the last and the first byte of a block, for each of the four lines; some ordinary reads in between
    for which in range(4):
        for target in (B - 1, 0):
            n = int(rng.integers(90, 160))
            b.add_aligned(_bases(rng, n), _quals(rng, n, 2, 40), which, target)
            for _ in range(3):
                n = int(rng.integers(1, 152))
                b.add(_bases(rng, n), _quals(rng, n, 2, 40))
    return b.text()


def newline_offsets_hit(text):
    """{offset mod B} of the text's newlines (the design claims 0 and B - 1)"""
    a = np.frombuffer(text, np.uint8)
    return set((np.nonzero(a == 10)[0] % B).tolist())


def sized(total, seed=3):
    """a good text of exactly `total` bytes (total 0, or >= 24)"""
    if total == 0:
        return b""
    rng = np.random.default_rng(seed + total)
    b = Builder()
    while total - b.n > 400:
        n = int(rng.integers(1, 152))
        b.add(_bases(rng, n), _quals(rng, n, 2, 40))
    rest = total - b.n            # header + 2 n + 5 bytes
    n = (rest - 5 - 4) // 2
    hl = rest - 5 - 2 * n
    b.add(_bases(rng, n), _quals(rng, n, 2, 40), header=b"@".ljust(hl, b"s"))
    assert b.n == total
    return b.text()


def size_cases():
    return {"empty": b"", "one-entry": b"@one\nACGTN\n+\nIIII#\n", "B-1": sized(B - 1), "B": sized(B), "B+1": sized(B + 1), "3B": sized(3 * B)}


def variants(text):
    """the same entries under other line endings and file ends"""
    return {"crlf": text.replace(b"\n", b"\r\n"), "no-final-newline": text[:-1], "blank-lines-behind": text + b"\n\n\n\n\n", "blank-crlf-behind": text + b"\r\n\n\r\n",
            "crlf-no-final-newline": text.replace(b"\n", b"\r\n")[:-2]}


def _plain(n_entries=40, length=100, seed=11):
    rng = np.random.default_rng(seed)
    return [[b"@e%d" % i, _bases(rng, length), b"+", _quals(rng, length, 2, 40)] for i in range(n_entries)]


def _join(entries):
    return b"".join(l + b"\n" for e in entries for l in e)


def error_cases(long_read=False):
    """[(name, text, (entry, kind), cut)]: the first error the reference meets; cut: an offset at which the text should also be fed in two pieces (or None)"""
    out = []
    bad_q = bytes([127 if long_read else 75])

    def case(name, edits, expect, cut_entry=None, tail=None):
        es = _plain()
        for k, f in edits:
            f(es[k])
        text = _join(es) if tail is None else _join(es[:tail[0]]) + tail[1]
        cut = len(_join(es[:cut_entry])) if cut_entry is not None else None
        out.append((name, text, expect, cut))

    def sub(line, at, c):
        def f(e):
            e[line] = e[line][:at] + c + e[line][at + 1:]
        return f

    def put(line, v):
        def f(e):
            e[line] = v
        return f
    case("kind1-header", [(7, sub(0, 0, b"X"))], (7, 1))
    case("kind2-header2-empty", [(7, put(2, b""))], (7, 2))
    case("kind2-header2-char", [(7, put(2, b"x+"))], (7, 2))
    case("kind3-short-qualities", [(7, lambda e: e.__setitem__(3, e[3][:-1]))], (7, 3))
    case("kind3-long-qualities", [(0, lambda e: e.__setitem__(3, e[3] + b"I"))], (0, 3))
    case("kind4-lowercase", [(39, sub(1, 99, b"a"))], (39, 4))
    case("kind4-first-base", [(7, sub(1, 0, b"-"))], (7, 4))
    case("kind5-below", [(7, sub(3, 64, b" "))], (7, 5))
    case("kind5-above", [(7, sub(3, 63, bad_q))], (7, 5))
    case("kind5-tab", [(7, sub(3, 0, b"\t"))], (7, 5))
    case("kind6-empty-header-base", [(7, put(0, b"")), (7, sub(1, 5, b"X"))], (7, 6))
    case("kind6-empty-header-lengths", [(7, put(0, b"")), (7, put(3, b"II"))], (7, 6))
    case("two-kinds-2-and-4", [(7, put(2, b"-")), (7, sub(1, 3, b"x"))], (7, 2))
    case("two-kinds-4-and-5", [(7, sub(1, 70, b"x")), (7, sub(3, 2, b" "))], (7, 4))
    case("two-kinds-1-and-3", [(7, sub(0, 0, b">")), (7, put(3, b"I"))], (7, 1))
    case("two-entries-far-apart", [(5, sub(3, 9, b" ")), (35, sub(0, 0, b"X"))], (5, 5))
    case("two-entries-later-has-lower-kind", [(36, sub(0, 0, b"X")), (4, sub(3, 9, b" "))], (4, 5))
    case("behind-a-piece-boundary", [(20, sub(1, 0, b"x"))], (20, 4), cut_entry=20)
    case("first-entry", [(0, sub(0, 0, b"A"))], (0, 1), cut_entry=1)
    case("incomplete-two-lines", [], (10, 2), tail=(10, b"@last\nACGT\n"))
    case("incomplete-three-lines", [], (10, 3), tail=(10, b"@last\nACGT\n+"))
    case("incomplete-header-only", [], (10, 2), tail=(10, b"@last"))
    return out
