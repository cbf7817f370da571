#!/usr/bin/env python3
"""Synthetic FASTQ for timing ReadQC and the FASTQ kernels (DESIGN.md §5 "FASTQ input"): reads of one length with Illumina-like qualities, written as plain text
or as gzip. A block of reads (--block-reads) is generated once and repeated until --bytes of text are reached, so a gigabyte is made in seconds; the gzip form is the
deflated block repeated as gzip members (a valid multi-member file). Deterministic for a seed.
    python tools/fastqgen.py --bytes 1073741824 --out /tmp/reads.fastq.gz"""
import argparse
import gzip

import numpy as np


def block(n_reads, length, seed):
    rng = np.random.default_rng(seed)
    bases = rng.choice(np.frombuffer(b"ACGTN", np.uint8), (n_reads, length), p=[0.27, 0.23, 0.23, 0.265, 0.005])
    q = np.clip(rng.normal(36, 4, (n_reads, length)).astype(np.int64) - (rng.random((n_reads, length)) < 0.03) * 25, 2, 41).astype(np.uint8) + 33
    parts = []
    for i in range(n_reads):
        parts += [b"@SIM:1:FC:1:%d:%d:%d 1:N:0:ACGT\n" % (1101 + i // 10000, 1000 + i % 9973, 2000 + i % 7919), bases[i].tobytes(), b"\n+\n", q[i].tobytes(), b"\n"]
    return b"".join(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30, help="text bytes (rounded up to whole blocks)")
    ap.add_argument("--length", type=int, default=151)
    ap.add_argument("--block-reads", type=int, default=50000)
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--out", required=True, help="*.gz: gzip members, else plain text")
    a = ap.parse_args()
    b = block(a.block_reads, a.length, a.seed)
    n = -(-a.bytes // len(b))
    data = gzip.compress(b, a.level) if a.out.endswith(".gz") else b
    with open(a.out, "wb") as f:
        for _ in range(n):
            f.write(data)
    print("%s: %d reads, %d text bytes, %d file bytes" % (a.out, n * a.block_reads, n * len(b), n * len(data)))


if __name__ == "__main__":
    main()
