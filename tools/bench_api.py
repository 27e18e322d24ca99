#!/usr/bin/env python3
"""The drop-in entry as lzbench would call it: zultra_memory_compress on a host buffer (PCIe-inclusive, pageable memory).
Reported next to bench.py's HBM-resident number; never the headline value.

usage: python tools/bench_api.py [bytes] [--lib PATH] [--leg latency|memory|stream]

Without --leg: the table of framings and max-block sizes, best of three calls each. With --leg: one end-to-end figure of the host layer as one JSON
line (A/B of two builds of the library: every leg and every build in a process of its own) —
  latency  zultra_memory_compress of the 39 680-byte file of bench.py's configuration 1, raw deflate, default block size: median of 200 calls after 20
  memory   [bytes] (100 MB) of text through zultra_memory_compress, gzip, 64 KiB max-blocks: median of 5 calls after 2
  stream   the same through the stream API in chunks of 1 MiB: median of 5 calls after 2
--lib: a build of the library other than the package's (as tools/ab_lib.py and tools/inflate_time.py take one)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import corpus  # noqa: E402
import zultra_amd  # noqa: E402
from zultra_amd._ffi import Lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("size", nargs="?", type=int, default=100_000_000)
ap.add_argument("--lib")
ap.add_argument("--leg", choices=["latency", "memory", "stream"])
args = ap.parse_args()
size = args.size
L = Lib(args.lib) if args.lib else zultra_amd.lib()


def timed(call, warmup, reps):
    """call() -> compressed bytes written; the median wall time of `reps` calls after `warmup`, and that byte count."""
    for _ in range(warmup):
        n = call()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        n = call()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), n


def stream_call(d, out, flags, bs, chunk):
    """The whole of d through one stream, `chunk` bytes per call, into `out` (large enough for all of it)."""
    s = L.stream(flags, bs)
    st = s.s
    st.next_out, st.avail_out = out.ctypes.data, len(out)
    for pos in range(0, len(d), chunk):
        st.next_in, st.avail_in = d.ctypes.data + pos, min(chunk, len(d) - pos)
        final = pos + chunk >= len(d)
        while True:
            rc = L.L.zultra_stream_compress(C.byref(st), 1 if final else 0)
            if rc != 0 or st.avail_in == 0:
                break
        assert rc == (1 if final else 0), rc
    n = int(st.total_out)
    s.end()
    return n


if args.leg:
    if args.leg == "latency":
        d, flags, bs, warmup, reps = corpus.bootstrap_js(), 0, 0, 20, 200
        assert len(d) == 39680
    else:
        d, flags, bs, warmup, reps = corpus.text_like_fast(size, 1000), 2, 65536, 2, 5
    out = np.empty(L.memory_bound(len(d), flags, bs) + 16, dtype=np.uint8)
    if args.leg == "stream":
        med, best, n = timed(lambda: stream_call(d, out, flags, bs, 1 << 20), warmup, reps)
    else:
        med, best, n = timed(lambda: L.memory_compress_into(d, flags, bs, out), warmup, reps)
    assert n, "the call failed"
    print(json.dumps({"leg": args.leg, "lib": os.path.basename(os.path.dirname(os.path.abspath(L.path))) + "/" + os.path.basename(L.path), "in_bytes": len(d), "out_bytes": n,
                      "crc32": "%08x" % (zlib.crc32(out[:n].tobytes()) & 0xFFFFFFFF), "median_ms": round(med * 1e3, 4), "min_ms": round(best * 1e3, 4),
                      "calls": reps, "warmup": warmup}), flush=True)
    sys.exit(0)

d = corpus.text_like_fast(size, 1000)
for flags, bs in ((2, 65536), (1, 65536), (0, 65536), (2, 0), (1, 32768)):
    best = None
    for it in range(3):
        t0 = time.perf_counter()
        out = L.memory_compress(d, flags, bs)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    print("zultra_memory_compress flags=%d max_block=%d: %.1f MB/s (%d -> %d bytes)" % (flags, bs, size / best / 1e6, size, len(out)), flush=True)
