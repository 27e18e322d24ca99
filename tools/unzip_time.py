"""Times zultra_hip_unzip on the MI355X and writes profiles/unzip_time.txt:

  * the five kernel times (index, local headers, inflate, copy, check) of a 100 000-entry archive of 4 KiB records and of one of 1000 x 200 KiB, from and
    to device memory, five runs each;
  * the index (zultra_hip_zip_index) with the tile size swept from 4 KiB to the whole directory, two figures per row: zh_uz_tiles + zh_uz_resolve alone
    (no dirents asked for), and those two with zh_uz_entries, the third pass whose time depends on the tile size (one lane walks each tile). The LAST row is
    the serial one-lane walk — one tile, nothing to speculate —, which is what the tiled index is compared against.

Archives come from Python's zipfile (stored and deflated entries alternate) and are built once, into a temporary file. Every row is a process of its own, run
under its own time limit; a row that fails ends the run.

    python tools/unzip_time.py [--out profiles/unzip_time.txt]
    python tools/unzip_time.py --row KIND TILE FILE     (one row, printed: what the parent starts)
"""
import argparse
import ctypes as C
import io
import os
import struct
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KINDS = {"records": (100000, 4096), "large": (1000, 200 * 1024)}


def archive(kind):
    n, size = KINDS[kind]
    rs = np.random.RandomState(5)
    words = [bytes(rs.randint(97, 123, size=int(k)).astype(np.uint8)) for k in rs.randint(2, 10, size=4000)]
    text = b" ".join(words[int(i)] for i in rs.randint(0, len(words), size=size // 3))[:size].ljust(size, b".")
    out = io.BytesIO()
    with zipfile.ZipFile(out, "w") as z:
        for i in range(n):
            info = zipfile.ZipInfo("dir%03d/entry%06d.txt" % (i % 500, i))
            info.compress_type = zipfile.ZIP_DEFLATED if i & 1 else zipfile.ZIP_STORED
            z.writestr(info, text[i % 97:] + text[:i % 97], compresslevel=1)
    return out.getvalue()


def directory(buf):
    """-> (position, size) of the central directory, from the end records zipfile writes (no archive comment)"""
    size_dir, off_dir = struct.unpack_from("<II", buf, len(buf) - 22 + 12)
    if off_dir == 0xFFFFFFFF or size_dir == 0xFFFFFFFF:   # (more than 65 535 entries: zipfile writes the ZIP64 records in front)
        size_dir, off_dir = struct.unpack_from("<QQ", buf, len(buf) - 22 - 20 - 56 + 40)
    return off_dir, size_dir


def hip():
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    raise RuntimeError("the HIP runtime is not there")


def row(kind, tile, path):
    import zultra_amd
    lib = zultra_amd.lib()
    buf = np.fromfile(path, dtype=np.uint8)
    off, size = directory(buf)
    n, total = KINDS[kind][0], KINDS[kind][0] * KINDS[kind][1]
    h = hip()
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    src, dst = C.c_void_p(), C.c_void_p()
    assert h.hipMalloc(C.byref(src), len(buf)) == 0 and h.hipMalloc(C.byref(dst), total) == 0
    assert h.hipMemcpy(src, buf.ctypes.data, len(buf), 1) == 0
    chain, index, whole = [], [], []
    for cap, times in ((0, chain), (n, index)) * 5:
        rc, res, dirents, ms = lib.zip_index(src.value, len(buf), off, size, cap)
        assert rc == 0 and res.stop == 0 and res.entries == n and len(dirents) == cap, (rc, res.stop, res.entries)
        times.append(ms)
    if tile == 0:
        for _ in range(5):
            rc, res, _, _, ms = lib.unzip(src.value, len(buf), off, size, 0, dst.value, total, None)
            assert rc == 0 and res.out_size == total, (rc, res.stop)
            whole.append(ms)
    h.hipFree(src)
    h.hipFree(dst)
    print("ROW %s tile %d directory %d entries %d tiles %d rewalked %d tiles+resolve_ms %s with_entries_ms %s"
          % (kind, tile, size, res.entries, res.tiles, res.tiles_rewalked, " ".join("%.4f" % v for v in chain), " ".join("%.4f" % v for v in index)))
    for ms in whole:
        print("ROW %s unzip_ms index %.4f locals %.4f inflate %.4f copy %.4f check %.4f  (%d -> %d bytes)" % ((kind,) + tuple(ms) + (len(buf), total)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unzip_time.txt"))
    ap.add_argument("--row", nargs=3)
    a = ap.parse_args()
    if a.row:
        return row(a.row[0], int(a.row[1]), a.row[2])
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        for kind in KINDS:
            buf = archive(kind)
            size = directory(buf)[1]
            path = os.path.join(tmp, kind + ".zip")
            with open(path, "wb") as f:
                f.write(buf)
            del buf
            tiles = [0] + [t for t in (4096, 8192, 16384, 32768, 65536, 262144, 1048576, 4194304) if t < size] + [max(size, 32)]
            for t in tiles:   # 0: the default tile, with the five kernel times; the last: the serial walk
                env = dict(os.environ)
                env.pop("ZULTRA_HIP_INDEX_TILE", None)
                if t:
                    env["ZULTRA_HIP_INDEX_TILE"] = str(t)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--row", kind, str(t), path], env=env, capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    sys.stderr.write(r.stdout + r.stderr)
                    return 1
                rows = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("ROW ")]
                lines += rows
                print("\n".join(rows), flush=True)
    with open(a.out, "w") as f:
        f.write("tools/unzip_time.py: zultra_hip_unzip and zultra_hip_zip_index on the MI355X, HIP event times in ms, five runs per row.\n"
                "tile 0 = the default (ZH_UZ_TILE, 16 KiB); the last tile of a kind is the whole directory: the serial one-lane walk.\n"
                "tiles+resolve_ms: zh_uz_tiles and zh_uz_resolve (no dirents asked for); with_entries_ms: the same and zh_uz_entries.\n"
                "The first figure of a row holds the process's first launches.\n\n" + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
