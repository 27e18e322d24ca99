#!/usr/bin/env python3
"""Device time of laying a batch out as ZIP entries on the device (zultra_hip_zip_members) on

  * a files batch (default 65 536 inputs of 4 KiB);
  * a batch of max-blocks (default 1 500 blocks of 64 KiB of text).

Per batch, --repeat times each (default 5), every run printed:

  (a) the three launches from HIP events on the context's stream: zh_zip_scan, zh_zip_records, zh_zip_copy;
  (b) the yardstick of the copy: ONE device-to-device hipMemcpyAsync of the same local_bytes, out of the zip buffer, between two events, in the same
      process right behind each call. The library does not hand out its stream, so the copy runs on a stream of this tool's; the device does nothing else
      at the time;
  (c) the batch's compress time (timing()["total_ms"] of its compress call), which the three launches are given as a share of.

    python tools/zip_time.py [--files 65536] [--file-size 4096] [--blocks 1500] [--block-size 65536] [--repeat 5]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import corpus  # noqa: E402
import zultra_amd  # noqa: E402


class Hip:
    """The few calls of the HIP runtime the yardstick needs."""

    def __init__(self):
        self.L = None
        for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
            try:
                self.L = C.CDLL(name)
                break
            except OSError:
                continue
        assert self.L is not None, "HIP runtime not found"
        self.stream = C.c_void_p()
        self.ev = [C.c_void_p(), C.c_void_p()]
        assert self.L.hipStreamCreate(C.byref(self.stream)) == 0
        for e in self.ev:
            assert self.L.hipEventCreate(C.byref(e)) == 0
        self.L.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        self.L.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.L.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.L.hipStreamSynchronize.argtypes = [C.c_void_p]
        self.L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.L.hipFree.argtypes = [C.c_void_p]

    def copy_ms(self, dst, src, nbytes):
        ms = C.c_float(0)
        assert self.L.hipEventRecord(self.ev[0], self.stream) == 0
        assert self.L.hipMemcpyAsync(dst, src, nbytes, 3, self.stream) == 0
        assert self.L.hipEventRecord(self.ev[1], self.stream) == 0
        assert self.L.hipStreamSynchronize(self.stream) == 0
        assert self.L.hipEventElapsedTime(C.byref(ms), self.ev[0], self.ev[1]) == 0
        return float(ms.value)


def fmt(v):
    return "%s   (min %.3f, max %.3f)" % (" ".join("%.3f" % x for x in v), min(v), max(v))


def measure(hip, ctx, n, repeat, name, compress_ms):
    names = [b"dir%02d/file%06d.bin" % (i % 50, i) for i in range(n)]
    scan, records, copy, memcpy = [], [], [], []
    rc, ent, local, central, central_at = ctx.zip_members(names)          # (the first call allocates)
    assert rc == 0, rc
    dst = C.c_void_p()
    assert hip.L.hipMalloc(C.byref(dst), local) == 0
    hip.copy_ms(dst, ctx.zip_ptr()[0], local)
    for _ in range(repeat):
        rc, ent, local, central, central_at = ctx.zip_members(names)
        assert rc == 0, rc
        ms = ctx.last_zip_ms()
        scan.append(ms[0]), records.append(ms[1]), copy.append(ms[2])
        memcpy.append(hip.copy_ms(dst, ctx.zip_ptr()[0], local))
    hip.L.hipFree(dst)
    comp = np.array([int(e["comp_size"]) for e in ent])
    three = [a + b + c for a, b, c in zip(scan, records, copy)]
    print("%s: %d entries, streams of %d .. %d bytes, local part %d bytes, central part %d bytes" % (name, n, comp.min(), comp.max(), local, central))
    print("  (a) zh_zip_scan, ms                                   : %s" % fmt(scan))
    print("  (a) zh_zip_records, ms                                : %s" % fmt(records))
    print("  (a) zh_zip_copy, ms                                   : %s" % fmt(copy))
    print("  (b) hipMemcpyAsync of local_bytes, device to device   : %s" % fmt(memcpy))
    print("      zh_zip_copy / memcpy, medians                     : %.2f" % (float(np.median(copy)) / float(np.median(memcpy))))
    print("  (c) the batch's compress time, ms                     : %.3f" % compress_ms)
    print("      the three launches, share of it, median           : %.2f %%" % (100.0 * float(np.median(three)) / compress_ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=65536)
    ap.add_argument("--file-size", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=1500)
    ap.add_argument("--block-size", type=int, default=65536)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    lib = zultra_amd.lib()
    print("library: %s" % lib.path)
    hip = Hip()
    text = corpus.text_like_fast(min(max(a.files * a.file_size, a.blocks * a.block_size, 1), 64 << 20), 7)[:64 << 20]
    if a.files:
        data = np.resize(text, a.files * a.file_size)
        sizes = np.full(a.files, a.file_size, dtype=np.uint32)
        offsets = (np.arange(a.files, dtype=np.uint64) * a.file_size)
        ctx = lib.files_context(a.file_size, a.files)
        ctx.compress_files(data, offsets, sizes)          # (warm: the graph is captured)
        ctx.compress_files(data, offsets, sizes)
        measure(hip, ctx, a.files, a.repeat, "files batch", ctx.timing()["total_ms"])
        ctx.close()
    if a.blocks:
        n = a.block_size
        data = np.resize(text, a.blocks * n)
        blocks = [(i * n, 0, n) for i in range(a.blocks)]
        ctx = lib.context(n, a.blocks)
        ctx.compress_blocks(data, blocks)
        ctx.compress_blocks(data, blocks)
        compress_ms = ctx.timing()["total_ms"]
        ctx.stitch_files()                                # (the plain assembly, so that the calls below launch the three kernels only)
        measure(hip, ctx, a.blocks, a.repeat, "batch of %d KiB max-blocks" % (n >> 10), compress_ms)
        ctx.close()


if __name__ == "__main__":
    main()
