#!/usr/bin/env python3
"""Device and wall time of framing a batch on the device (zultra_hip_frame_members) on

  * a files batch (default 65 536 inputs of 4 KiB, gzip members);
  * a BGZF batch (default 1 500 blocks of 65 280 bytes of text, with the end marker).

Per batch, --repeat times each (default 5), every run printed:

  (a) the plain assembly of the batch, zultra_hip_stitch_files assembling again (memset + scan + mover with head = tail = 0, timing()["stitch_ms"]).
      With --lib PATH the same figure is taken from ANOTHER build of the library — the parent commit's — on the same input: the two sets of five and
      their spreads say what the scan's head / tail arithmetic costs the existing path.
  (b) the framed assembly's launches from HIP events on the context's stream: scan + clearing, mover, frame kernel.
  (c) wall time from the batch's end to framed bytes on the host: frame_members + one stream_read, against the route without the frame kernel —
      stitch_files, one stream_read, then the members put together on the host in C (a header, memcpy of the stream, zultra_crc32_append, ISIZE per
      member; the helper below is compiled with the system's C compiler when the tool starts). The two results are compared byte for byte.

    python tools/frame_time.py [--files 65536] [--file-size 4096] [--blocks 1500] [--repeat 5] [--lib other/libzultra_amd.so]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import corpus  # noqa: E402
import zultra_amd  # noqa: E402
from zultra_amd._ffi import Lib  # noqa: E402

GZIP, BGZF = 2, 4
NEW_EXPORTS = ("zultra_hip_frame_members", "zultra_hip_last_frame_ms", "zultra_memory_bound_bgzf", "zultra_memory_compress_bgzf", "zultra_memory_compress_batch")

HOST_FRAMING_C = r"""
#include <stdint.h>
#include <string.h>
typedef uint32_t (*append_t)(uint32_t, uint32_t, size_t);
/* the route without the frame kernel: members put together from the plain layout, on the host */
size_t frame_on_host(const uint8_t *stream, const uint64_t *off, const uint32_t *crc_lin, const uint32_t *n, uint32_t count, int bgzf, append_t append, uint8_t *out) {
   static const uint8_t gz[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 2, 255};
   static const uint8_t bg[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0};
   static const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
   size_t w = 0;
   for (uint32_t i = 0; i < count; i++) {
      const size_t len = (size_t)(off[i + 1] - off[i]);
      if (bgzf) {
         const uint32_t bsize = (uint32_t)(18 + len + 8 - 1);
         memcpy(out + w, bg, 16);
         out[w + 16] = (uint8_t)bsize;
         out[w + 17] = (uint8_t)(bsize >> 8);
         w += 18;
      }
      else {
         memcpy(out + w, gz, 10);
         w += 10;
      }
      memcpy(out + w, stream + off[i], len);
      w += len;
      const uint32_t crc = append(0, crc_lin[i], n[i]);
      for (int k = 0; k < 4; k++) out[w + k] = (uint8_t)(crc >> (8 * k));
      for (int k = 0; k < 4; k++) out[w + 4 + k] = (uint8_t)(n[i] >> (8 * k));
      w += 8;
   }
   if (bgzf) {
      memcpy(out + w, eof, 28);
      w += 28;
   }
   return w;
}
"""


def build_host_framing(tmp):
    src, so = os.path.join(tmp, "frame_on_host.c"), os.path.join(tmp, "frame_on_host.so")
    with open(src, "w") as f:
        f.write(HOST_FRAMING_C)
    subprocess.run([os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", "-o", so, src], check=True)
    h = C.CDLL(so)
    h.frame_on_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
    h.frame_on_host.restype = C.c_size_t
    return h


def fmt(v):
    return "%s   (min %.3f, max %.3f, spread %.3f)" % (" ".join("%.3f" % x for x in v), min(v), max(v), max(v) - min(v))


def stitch_files_raw(lib, ctx, n):
    """zultra_hip_stitch_files through the C ABI (a build from before HipContext.stitch_files has the export all the same)."""
    out = np.zeros(n + 1, dtype=np.uint64)
    f = lib.L.zultra_hip_stitch_files
    f.argtypes = [C.c_void_p, C.c_void_p]
    assert f(ctx.h, out.ctypes.data) == 0
    return out


def measure_plain(lib, ctx, n, repeat):
    """(a): the plain assembly, launched again by every call (the assembly of another kind in between drops what a files batch brought with it)."""
    ms = []
    for _ in range(repeat + 1):
        invalidate(lib, ctx)
        stitch_files_raw(lib, ctx, n)
        ms.append(ctx.timing()["stitch_ms"])
    return ms[1:]          # (the first run pays for the allocation of file_off in a context of max-blocks)


def invalidate(lib, ctx):
    """A files batch brings its assembly with it and stitch_files then launches nothing: any assembly of another kind in between makes the next call
    assemble again. zultra_hip_stitch_device at phase 0 is such a one, in every build."""
    try:
        ctx.stitch_device(-1, 0)
    except Exception:
        pass


def measure(lib, host, ctx, sizes, framing, eof, repeat, name):
    n = len(sizes)
    sizes32 = np.ascontiguousarray(sizes, dtype=np.uint32)
    plain = measure_plain(lib, ctx, n, repeat)
    scan, mover, frame, wall_dev, wall_host = [], [], [], [], []
    lib.L.zultra_crc32_append.argtypes = [C.c_uint32, C.c_uint32, C.c_size_t]
    lib.L.zultra_crc32_append.restype = C.c_uint32
    append = C.cast(lib.L.zultra_crc32_append, C.c_void_p)
    framed = np.empty(int(sizes32.sum()) + 64 * n + 1024, dtype=np.uint8)
    stream = np.empty(len(framed), dtype=np.uint8)
    byhost = np.empty(len(framed), dtype=np.uint8)
    for _ in range(repeat):
        t0 = time.perf_counter()
        rc, mem, total = ctx.frame_members(framing, eof)
        ctx.stream_read(total, out=framed)
        wall_dev.append(1e3 * (time.perf_counter() - t0))
        assert rc == 0, rc
        ms = ctx.frame_ms()
        scan.append(ms[0]), mover.append(ms[1]), frame.append(ms[2])
        t0 = time.perf_counter()
        off = stitch_files_raw(lib, ctx, n)
        ctx.stream_read(int(off[-1]), out=stream)
        crc = ctx.block_crc32()
        w = host.frame_on_host(stream.ctypes.data, off.ctypes.data, crc.ctypes.data, sizes32.ctypes.data, n, 1 if framing == BGZF else 0, append, byhost.ctypes.data)
        wall_host.append(1e3 * (time.perf_counter() - t0))
        assert w == total and (byhost[:w] == framed[:w]).all(), "the host route and the device disagree"
    print("%s: %d members, %d framed bytes" % (name, n, total))
    print("  (a) plain assembly, memset + scan + mover, ms        : %s" % fmt(plain))
    print("  (b) framed: scan + clearing, ms                      : %s" % fmt(scan))
    print("  (b) framed: mover, ms                                : %s" % fmt(mover))
    print("  (b) framed: frame kernel, ms                         : %s" % fmt(frame))
    print("  (c) wall, frame_members + read, ms                   : %s" % fmt(wall_dev))
    print("  (c) wall, stitch_files + read + framing in C on host : %s" % fmt(wall_host))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=65536)
    ap.add_argument("--file-size", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=1500)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--lib", default=None, help="another build of libzultra_amd.so (the parent commit's): only (a) is measured")
    a = ap.parse_args()
    other = a.lib is not None
    lib = Lib(a.lib, allow_missing=NEW_EXPORTS) if other else zultra_amd.lib()
    print("library: %s" % lib.path)
    text = corpus.text_like(min(max(a.files * a.file_size, a.blocks * 65280, 1), 64 << 20), 7)
    with tempfile.TemporaryDirectory() as tmp:
        host = None if other else build_host_framing(tmp)
        if a.files:
            data = np.resize(text, a.files * a.file_size)
            sizes = np.full(a.files, a.file_size, dtype=np.uint32)
            offsets = (np.arange(a.files, dtype=np.uint64) * a.file_size)
            ctx = lib.files_context(a.file_size, a.files)
            ctx.compress_files(data, offsets, sizes)
            if other:
                print("files batch: %d inputs\n  (a) plain assembly, memset + scan + mover, ms        : %s" % (a.files, fmt(measure_plain(lib, ctx, a.files, a.repeat))))
            else:
                measure(lib, host, ctx, sizes, GZIP, False, a.repeat, "files batch")
            ctx.close()
        if a.blocks:
            n = 65280
            data = np.resize(text, a.blocks * n)
            ctx = lib.context(n, a.blocks)
            ctx.compress_blocks(data, [(i * n, 0, n) for i in range(a.blocks)])
            if other:
                print("BGZF batch: %d blocks\n  (a) plain assembly, memset + scan + mover, ms        : %s" % (a.blocks, fmt(measure_plain(lib, ctx, a.blocks, a.repeat))))
            else:
                measure(lib, host, ctx, [n] * a.blocks, BGZF, True, a.repeat, "BGZF batch")
            ctx.close()


if __name__ == "__main__":
    main()
