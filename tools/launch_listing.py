#!/usr/bin/env python3
"""Diagnostics: the launch listing of a -DZH_TRACE_LAUNCH build (tools/build_variant.sh <name> -DZH_TRACE_LAUNCH): every launch with its grid and block, on stderr, in the
order the host enqueues them — to be compared between two builds with diff (grep '^launch\\|^== batch'). One build per process.
usage: python tools/launch_listing.py <lib.so> blocks|files 2> listing.txt
blocks: 13 MiB at 64 KiB max-blocks, three runs, one context — text twice (the second batch goes out without chain kernels and without overflow forms), then tables and
        near-copies (the batch is run again).
files:  64 inputs of 4 KiB, two batches; run with ZULTRA_HIP_STREAMS=2 ZULTRA_HIP_FILES_RUN_GRAPHS=0 (the trace build waits around every launch: not through graph capture)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import corpus  # noqa: E402
from zultra_amd._ffi import Lib  # noqa: E402

so, mode = sys.argv[1], sys.argv[2]
L = Lib(so)


def mark(k):
    sys.stderr.write("== batch %d\n" % k)
    sys.stderr.flush()


if mode == "blocks":
    n, bs = 13 << 20, 65536
    plain = corpus.text_like(n, 31)
    chains = np.concatenate([corpus.table_like(n // 2, 9), corpus.duplicated(n - n // 2, 4, 900)])
    nb = (n + bs - 1) // bs
    blocks = [(b * bs - (32768 if b else 0), 32768 if b else 0, min(bs, n - b * bs)) for b in range(nb)]
    ctx = L.context(bs, nb)
    for k, d in enumerate((plain, plain, chains)):
        mark(k)
        ctx.compress_blocks(d, blocks)
        st = ctx.stats()
        print("batch", k, "runs", st["runs"], "rerun", st["batches_rerun"], "without chain kernels", st["runs_without_chain_kernels"], flush=True)
else:
    size, nf = 4096, 64
    host = np.concatenate([corpus.json_like(size, 5 + k) for k in range(nf)])
    ctx = L.files_context(size, nf)
    offs = np.arange(nf, dtype=np.uint64) * np.uint64(size)
    sizes = np.full(nf, size, dtype=np.uint32)
    for k in range(2):
        mark(k)
        fo = ctx.compress_files(host, offs, sizes)
        print("files batch", k, "bytes out", int(fo[-1]), "runs", ctx.stats()["runs"], flush=True)
ctx.close()
