#!/usr/bin/env python3
"""Feeds a plain FASTQ text (tools/fastqgen.py) to FastqStats in pieces and prints the HIP-event sums of its copies and kernels (DESIGN.md §5 "FASTQ input").
    python tools/dev/fastq_rate.py reads.fastq [piece MiB]"""
import importlib
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
ngsqc = importlib.import_module("ngs-bits_amd")

path, piece = sys.argv[1], (int(sys.argv[2]) if len(sys.argv) > 2 else 32) << 20
text = open(path, "rb").read()
for rep in range(3):
    f = ngsqc.FastqStats()
    t0 = time.time()
    for o in range(0, len(text), piece):
        f.feed(text[o:o + piece], 0, last=o + piece >= len(text))
    st = f.result()
    r = f.report
    print("run %d: %d text bytes, %d reads, pieces of %d MiB: wall %.1f ms, H2D %.1f ms (%.1f GB/s), kernels %.1f ms (%.1f GB/s of text), host waited %.1f ms" % (
        rep, len(text), st["c_forward"], piece >> 20, (time.time() - t0) * 1e3, r["h2d_ms"], len(text) / r["h2d_ms"] / 1e6, r["kernels_ms"], len(text) / r["kernels_ms"] / 1e6, r["wait_ms"]), flush=True)
    f.close()
