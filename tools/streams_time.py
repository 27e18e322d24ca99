#!/usr/bin/env python3
"""Wall time of a ZIP archive of large files through the grouped assembly (zultra_memory_compress_zip_streams), next to what a caller
had to do before it existed, for the same files (default 64 files of 4 MiB of corpus text, max-blocks of 1 MiB):

  (a) zultra_memory_compress_zip_streams: the files as streams of max-blocks in shared device batches, the archive written on the device;
  (b) one zultra_memory_compress call per file (raw deflate): one batch and one synchronisation per file — the records of an archive would still be the
      caller's to write on the host, which is not timed;
  (c) the kernel times of one grouped assembly of the same batch, from HIP events on the context's stream: scan, fold, frame kernel.

--repeat times each (default 3, after one warm-up call of each), every run printed.

    python tools/streams_time.py [--files 64] [--file-size 4194304] [--max-block 1048576] [--repeat 3] [--out profiles/stream_groups_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import corpus  # noqa: E402
import zultra_amd  # noqa: E402


def fmt(v):
    return "%s   (min %.1f, max %.1f)" % (" ".join("%.1f" % x for x in v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--file-size", type=int, default=4 << 20)
    ap.add_argument("--max-block", type=int, default=1 << 20)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = zultra_amd.lib()
    n, size, mb = a.files, a.file_size, a.max_block
    data = np.ascontiguousarray(np.resize(corpus.text_like_fast(min(n * size, 64 << 20), 7), n * size))
    inputs = [(i * size, size) for i in range(n)]
    names = [b"dir%02d/file%04d.txt" % (i % 8, i) for i in range(n)]
    out = np.empty(lib.memory_bound(size, 0, mb) + 16, dtype=np.uint8)
    lines = ["library: %s" % lib.path, "%d files of %d bytes of corpus text, max-blocks of %d bytes" % (n, size, mb)]

    archive_ms, per_file_ms, archive_bytes, per_file_bytes = [], [], 0, 0
    for k in range(a.repeat + 1):
        t0 = time.perf_counter()
        got = lib.memory_compress_zip_streams(data, inputs, names, 0, mb)
        t1 = time.perf_counter()
        assert got is not None
        archive_bytes = len(got)
        per_file_bytes = 0
        for off, sz in inputs:
            r = lib.memory_compress_into(data[off: off + sz], 0, mb, out)
            assert r is not None
            per_file_bytes += r
        t2 = time.perf_counter()
        if k:   # (the first round warms both: contexts are created and cached)
            archive_ms.append(1e3 * (t1 - t0))
            per_file_ms.append(1e3 * (t2 - t1))
    mbytes = n * size / 1e6
    lines.append("(a) zultra_memory_compress_zip_streams, ms                 : %s   -> %d bytes, %.0f MB/s at the median" %
                 (fmt(archive_ms), archive_bytes, mbytes / (float(np.median(archive_ms)) / 1e3)))
    lines.append("(b) one zultra_memory_compress per file, ms in all         : %s   -> %d bytes of streams, %.0f MB/s at the median" %
                 (fmt(per_file_ms), per_file_bytes, mbytes / (float(np.median(per_file_ms)) / 1e3)))
    lines.append("    (b) / (a), medians                                     : %.2f" % (float(np.median(per_file_ms)) / float(np.median(archive_ms))))

    # (c) the assembly's own launches, on one batch of all the files
    per = (size + mb - 1) // mb
    blocks, first = [], []
    for i in range(n):
        first.append(len(blocks))
        for k in range(per):
            prev = min(32768, k * mb)
            blocks.append((i * size + k * mb - prev, prev, min(mb, size - k * mb)))
    ctx = lib.context(mb, len(blocks))
    ctx.compress_blocks(data, blocks)
    scan, fold, frame = [], [], []
    for k in range(a.repeat + 1):
        rc, mem, total = ctx.frame_streams(first, 2)
        assert rc == 0
        if k:
            ms = ctx.streams_ms()
            scan.append(ms[0]), fold.append(ms[1]), frame.append(ms[2])
    lines.append("(c) one grouped assembly of %d streams, %d max-blocks (gzip), kernel ms:" % (n, len(blocks)))
    lines.append("    zh_stitch_scan_streams (with the upload of the grouping): %s" % " ".join("%.3f" % v for v in scan))
    lines.append("    zh_fold_streams                                         : %s" % " ".join("%.3f" % v for v in fold))
    lines.append("    zh_frame_members over the streams                       : %s" % " ".join("%.3f" % v for v in frame))
    lines.append("    the batch's compress time, ms                           : %.1f" % ctx.timing()["total_ms"])
    ctx.close()
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
