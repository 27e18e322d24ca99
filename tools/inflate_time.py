#!/usr/bin/env python3
"""Times the batched inflate kernel (zh_inflate_streams, zultra_hip_inflate_streams) on a files batch of BASELINE.json configuration 5's shape:
the batch is compressed on the device and inflated from the context's stream buffer into device memory, nothing leaves HBM. Next to it the
verification kernel (zultra_hip_verify_device) on the same batch — the same decoder without an output path — and host zlib inflating the same
streams on one core. Then the dictionary leg: the same records compressed by host zlib against one preset dictionary (zdict: the library's files
mode has none) and inflated by zh_inflate_streams_dict (zultra_hip_inflate_streams_dict), next to the plain kernel on the same records compressed
by host zlib without a dictionary, and host zlib with zdict on one core. Then the members leg: the library's own raw streams of the first batch with
gzip framing put around them on the host, and as a second variant with zlib framing, inflated and CHECKED device to device by
zultra_hip_inflate_members (zh_frame_heads, the inflate kernel, zh_check_members: three kernel times), next to zultra_hip_inflate_streams on the
bare streams and host zlib.crc32 / zlib.adler32 over the output on one core, all in one process. Then the file leg: the first --bgzf-bytes of the
corpus as ONE BGZF file built on the host (payloads of 65 280 bytes, host zlib level 6), indexed, inflated and checked device to device by
zultra_hip_inflate_file (four kernel times: index, frame, inflate, check) with ZULTRA_HIP_INDEX_TILE swept over 64 KiB .. 4 MiB, next to the route
without the index in the same process: a host walk of BSIZE over a host copy of the file, then zultra_hip_inflate_members over those items. Then the
range leg (--only range; no part of the whole run): bytes of 64 KiB, 1 MiB and 16 MiB from the middle of the same file by zultra_hip_inflate_range, device
to device (five kernel times: index, select + items, frame, inflate, check + edges), next to the route to the same bytes without it in the same process:
zultra_hip_inflate_file of the whole file. One JSON line.

    python tools/inflate_time.py [--files N] [--file-size BYTES] [--reps N] [--dict-size BYTES] [--step-timeout SECONDS] [--lib PATH]

The steps run in this order, every GPU step in a process of its own under its own time limit; a step that fails ends the run:
    1. zultra_hip_inflate_streams from the device stream buffer (the output is read back once and compared with the input)
    2. zultra_hip_verify_device on the same batch
    3. host zlib, one core, over the same streams (this process: it touches no GPU)
    4. zultra_hip_inflate_streams_dict over the zdict streams, then zultra_hip_inflate_streams over the streams without a dictionary, device to
       device (both outputs are read back once and compared with the records)
    5. host zlib with zdict, one core, over the streams of step 4 (this process), every output compared with its record
    6. zultra_hip_inflate_members over the gzip members, then over the zlib members, device to device; zultra_hip_inflate_streams over the bare
       streams; zlib.crc32 and zlib.adler32 over the output on one core (the outputs are read back once and compared with the input)
    7. zultra_hip_inflate_file over the BGZF file per tile size, then the host walk and zultra_hip_inflate_members (the output is read back once
       and compared with the input)
    range (--only range). zultra_hip_inflate_range per range size, then zultra_hip_inflate_file of the whole file (every range is read back once and
       compared with the input)
--lib: another build of the library (an A/B of the plain kernel against an older build); steps 4 and 5 are left out where it has no dictionary kernel,
step 6 where it has no members call, step 7 where it has no file call."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def library(args):
    import zultra_amd
    if not args.lib:
        return zultra_amd.lib()
    from zultra_amd._ffi import Lib
    return Lib(args.lib, allow_missing=("zultra_memory_decompress_dict", "zultra_hip_inflate_streams_dict", "zultra_memory_decompress_batch", "zultra_hip_inflate_members",
                                        "zultra_hip_index_members", "zultra_hip_inflate_file", "zultra_memory_decompress_members",
                                        "zultra_hip_inflate_range", "zultra_memory_index_gzi", "zultra_memory_decompress_range"))


def batch(args):
    import numpy as np

    import corpus
    L = library(args)
    if L.device_count() < 1:
        raise RuntimeError("no HIP device visible: nothing can be timed")
    L.is_emulator = False
    d = np.ascontiguousarray(corpus.json_files(0, args.files, args.file_size), dtype=np.uint8)
    offs, sizes = np.arange(args.files, dtype=np.uint64) * args.file_size, np.full(args.files, args.file_size, dtype=np.uint32)
    ctx = L.files_context(args.file_size, args.files)
    file_off = ctx.compress_files(d, offs, sizes)
    return L, ctx, d, file_off


def child_inflate(args):
    import numpy as np

    import inflate_cases as I
    import verify_cases as V
    L, ctx, d, file_off = batch(args)
    n, fs = args.files, args.file_size
    items = np.stack([file_off[:-1], file_off[1:] - file_off[:-1], np.arange(n, dtype=np.uint64) * fs, np.full(n, fs, dtype=np.uint64)], axis=1)
    dst = V.DeviceCopy(L, np.zeros(n * fs, dtype=np.uint8))
    times, calls = [], []
    for it in range(2 + args.reps):   # (two warm-up calls)
        t0 = time.perf_counter()
        rc, res, ms = L.inflate_streams(ctx.stream_ptr(), int(file_off[-1]), dst.ptr, n * fs, items)
        calls.append(1e3 * (time.perf_counter() - t0))
        assert rc == 0, (rc, res[res["reason"] != 0][:4])
        if it >= 2:
            times.append(ms)
    assert I.device_read(L, dst, n * fs).tobytes() == d.tobytes(), "the inflated batch differs from the input"
    np.savez(args.stream_file, stream=ctx.stream_read(int(file_off[-1])), file_off=file_off)
    dst.free()
    ctx.close()
    print(json.dumps({"inflate_kernel_ms": {"min": min(times), "median": float(np.median(times)), "all": times},
                      "inflate_call_ms": {"min": min(calls[2:]), "all": calls[2:]}, "stream_bytes": int(file_off[-1]), "blocks": int(res["blocks"].sum())}), flush=True)
    return 0


def child_verify(args):
    import numpy as np
    L, ctx, d, file_off = batch(args)
    times = []
    for it in range(2 + args.reps):
        r = ctx.verify()
        assert r["rc"] == 0 and r["verified_bytes"] == len(d), r
        if it >= 2:
            times.append(r["verify_ms"])
    ctx.close()
    print(json.dumps({"verify_kernel_ms": {"min": min(times), "median": float(np.median(times)), "all": times}}), flush=True)
    return 0


def records_and_dictionary(args):
    """The records of configuration 5's generator and a dictionary of further records of it (so that every record finds its keys there)."""
    import numpy as np

    import corpus
    d = np.ascontiguousarray(corpus.json_files(0, args.files, args.file_size), dtype=np.uint8)
    more = (args.dict_size + args.file_size - 1) // args.file_size
    dictionary = np.ascontiguousarray(corpus.json_files(args.files, more, args.file_size), dtype=np.uint8)[-args.dict_size:]
    return d, dictionary.tobytes()


def zlib_records(d, n, fs, dictionary):
    """Every record as a raw deflate stream of host zlib (level 6), against the dictionary or without one -> (streams back to back, offsets[n + 1])."""
    import numpy as np
    raw = d.tobytes()
    base = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY, zdict=dictionary) if dictionary else zlib.compressobj(6, zlib.DEFLATED, -15, 9)
    parts = []
    for i in range(n):
        c = base.copy()
        parts.append(c.compress(raw[i * fs: (i + 1) * fs]) + c.flush())
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), off


def child_dict(args):
    import numpy as np

    import inflate_cases as I
    import verify_cases as V
    L = library(args)
    if L.device_count() < 1:
        raise RuntimeError("no HIP device visible: nothing can be timed")
    L.is_emulator = False
    n, fs = args.files, args.file_size
    d, dictionary = records_and_dictionary(args)
    out = {"dict_size": len(dictionary)}
    hist = V.DeviceCopy(L, np.frombuffer(dictionary, dtype=np.uint8).copy())
    for leg, zdict in (("dict", dictionary), ("nodict", None)):
        stream, off = zlib_records(d, n, fs, zdict)
        items = np.stack([off[:-1], off[1:] - off[:-1], np.arange(n, dtype=np.uint64) * fs, np.full(n, fs, dtype=np.uint64)], axis=1)
        src, dst = V.DeviceCopy(L, stream), V.DeviceCopy(L, np.zeros(n * fs, dtype=np.uint8))
        times = []
        for it in range(2 + args.reps):   # (two warm-up calls)
            if zdict:
                rc, res, ms = L.inflate_streams_dict(src.ptr, len(stream), dst.ptr, n * fs, hist.ptr, len(dictionary), items)
            else:
                rc, res, ms = L.inflate_streams(src.ptr, len(stream), dst.ptr, n * fs, items)
            assert rc == 0, (leg, rc, res[res["reason"] != 0][:4])
            if it >= 2:
                times.append(ms)
        assert I.device_read(L, dst, n * fs).tobytes() == d.tobytes(), "the inflated batch differs from the records (%s)" % leg
        src.free()
        dst.free()
        out["zlib_%s_stream_bytes" % leg] = int(off[-1])
        out["%s_inflate_kernel_ms" % leg] = {"min": min(times), "median": float(np.median(times)), "all": times}
        if zdict:
            np.savez(args.stream_file, stream=stream, file_off=off)
    hist.free()
    print(json.dumps(out), flush=True)
    return 0


def child_members(args):
    import numpy as np

    import inflate_cases as I
    import verify_cases as V
    L, ctx, d, file_off = batch(args)
    n, fs = args.files, args.file_size
    raw = d.tobytes()
    stream = ctx.stream_read(int(file_off[-1])).tobytes()
    bare = np.stack([file_off[:-1], file_off[1:] - file_off[:-1], np.arange(n, dtype=np.uint64) * fs, np.full(n, fs, dtype=np.uint64)], axis=1)
    dst = V.DeviceCopy(L, np.zeros(n * fs, dtype=np.uint8))
    out, times = {}, []
    for it in range(2 + args.reps):   # (two warm-up calls)
        rc, res, ms = L.inflate_streams(ctx.stream_ptr(), int(file_off[-1]), dst.ptr, n * fs, bare)
        assert rc == 0, (rc, res[res["reason"] != 0][:4])
        if it >= 2:
            times.append(ms)
    out["bare_inflate_kernel_ms"] = {"min": min(times), "median": float(np.median(times)), "all": times}
    ctx.close()
    for leg, framing, head in (("gzip", 2, b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03"), ("zlib", 1, b"\x78\x9c")):
        parts, sums = [], []
        for i in range(n):
            rec = raw[i * fs: (i + 1) * fs]
            sums.append(zlib.crc32(rec) if framing == 2 else zlib.adler32(rec))
            foot = sums[-1].to_bytes(4, "little") + fs.to_bytes(4, "little") if framing == 2 else sums[-1].to_bytes(4, "big")
            parts.append(head + stream[int(file_off[i]): int(file_off[i + 1])] + foot)
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(p) for p in parts])
        members = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
        items = np.stack([off[:-1], off[1:] - off[:-1], np.arange(n, dtype=np.uint64) * fs, np.full(n, fs, dtype=np.uint64)], axis=1)
        src = V.DeviceCopy(L, members)
        assert V._Hip.lib().hipMemset(C.c_void_p(dst.ptr), 0, C.c_size_t(n * fs)) == 0
        times = []
        for it in range(2 + args.reps):
            rc, res, ms = L.inflate_members(src.ptr, len(members), dst.ptr, n * fs, None, 0, framing, items)
            assert rc == 0, (leg, rc, res[res["reason"] != 0][:4])
            if it >= 2:
                times.append(ms)
        assert (res["check"] == np.array(sums, dtype=np.uint32)).all() and (res["src_used"] == items[:, 1]).all(), leg
        assert I.device_read(L, dst, n * fs).tobytes() == raw, "the inflated batch differs from the input (%s)" % leg
        src.free()
        med = [float(np.median([t[k] for t in times])) for k in range(3)]
        out["%s_members_kernel_ms" % leg] = {"frame": med[0], "inflate": med[1], "check": med[2], "all": times}
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            f = zlib.crc32 if framing == 2 else zlib.adler32
            got = [f(raw[i * fs: (i + 1) * fs]) for i in range(n)]
            host.append(1e3 * (time.perf_counter() - t0))
        assert got == sums
        out["%s_host_checksum_one_core_ms" % leg] = {"min": min(host), "all": host}
        out["%s_frame_and_check_over_inflate" % leg] = (med[0] + med[2]) / med[1]
        out["%s_frame_and_check_over_bare_inflate" % leg] = (med[0] + med[2]) / out["bare_inflate_kernel_ms"]["median"]
        out["%s_host_checksum_over_frame_and_check" % leg] = min(host) / (med[0] + med[2])
    dst.free()
    print(json.dumps(out), flush=True)
    return 0


FILE_TILES = [64 << 10, 128 << 10, 256 << 10, 512 << 10, 1 << 20, 2 << 20, 4 << 20]


def child_file(args):
    import numpy as np

    import corpus
    import inflate_cases as I
    import inflate_file_cases as F
    import verify_cases as V
    L = library(args)
    if L.device_count() < 1:
        raise RuntimeError("no HIP device visible: nothing can be timed")
    L.is_emulator = False
    nrec = (args.bgzf_bytes + args.file_size - 1) // args.file_size
    raw = np.ascontiguousarray(corpus.json_files(0, nrec, args.file_size), dtype=np.uint8).tobytes()[:args.bgzf_bytes]
    buf = b"".join(F.bgzf(raw[at: at + 65280]) for at in range(0, len(raw), 65280)) + F.EOF_MARKER
    src, dst = V.DeviceCopy(L, np.frombuffer(buf, dtype=np.uint8).copy()), V.DeviceCopy(L, np.zeros(len(raw), dtype=np.uint8))
    out = {"bgzf_input_bytes": len(raw), "bgzf_file_bytes": len(buf), "file_kernel_ms_by_tile": {}}
    for tile in FILE_TILES:
        os.environ["ZULTRA_HIP_INDEX_TILE"] = str(tile)   # (read per call)
        times, calls = [], []
        for it in range(2 + args.reps):   # (two warm-up calls)
            t0 = time.perf_counter()
            rc, res, _, ms = L.inflate_file(src.ptr, len(buf), dst.ptr, len(raw), None)
            calls.append(1e3 * (time.perf_counter() - t0))
            assert rc == 0 and res.stop == 0 and res.out_size == len(raw), (tile, rc, res.stop, res.out_size)
            if it >= 2:
                times.append(ms)
        med = [float(np.median([t[k] for t in times])) for k in range(4)]
        out["file_kernel_ms_by_tile"][str(tile)] = {"index": med[0], "frame": med[1], "inflate": med[2], "check": med[3], "call_ms_min": min(calls[2:]), "members": res.members,
                                                    "tiles": res.tiles, "tiles_rewalked": res.tiles_rewalked}
    del os.environ["ZULTRA_HIP_INDEX_TILE"]
    assert I.device_read(L, dst, len(raw)).tobytes() == raw, "the inflated file differs from the input"
    assert V._Hip.lib().hipMemset(C.c_void_p(dst.ptr), 0, C.c_size_t(len(raw))) == 0
    # the route without the index: the host walks BSIZE over a host copy of the file, zultra_hip_inflate_members takes the items
    walks, times, calls = [], [], []
    for it in range(2 + args.reps):
        t0 = time.perf_counter()
        items, stop, at, total = F.walk(buf)
        walks.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        rc, mres, ms = L.inflate_members(src.ptr, len(buf), dst.ptr, len(raw), None, 0, 2, items)
        calls.append(1e3 * (time.perf_counter() - t0))
        assert rc == 0 and stop == 0 and total == len(raw)
        if it >= 2:
            times.append(ms)
    assert I.device_read(L, dst, len(raw)).tobytes() == raw, "the inflated file differs from the input (members route)"
    med = [float(np.median([t[k] for t in times])) for k in range(3)]
    out["file_members_route"] = {"host_walk_python_ms_min": min(walks), "frame": med[0], "inflate": med[1], "check": med[2], "call_ms_min": min(calls[2:]), "members": len(items)}
    best = min(out["file_kernel_ms_by_tile"].items(), key=lambda kv: kv[1]["index"])
    out["file_best_tile"] = int(best[0])
    out["file_index_over_inflate_at_best_tile"] = best[1]["index"] / best[1]["inflate"]
    src.free()
    dst.free()
    print(json.dumps(out), flush=True)
    return 0


RANGE_SIZES = [64 << 10, 1 << 20, 16 << 20]


def child_range(args):
    import numpy as np

    import corpus
    import inflate_cases as I
    import inflate_file_cases as F
    import verify_cases as V
    L = library(args)
    if L.device_count() < 1:
        raise RuntimeError("no HIP device visible: nothing can be timed")
    L.is_emulator = False
    nrec = (args.bgzf_bytes + args.file_size - 1) // args.file_size
    raw = np.ascontiguousarray(corpus.json_files(0, nrec, args.file_size), dtype=np.uint8).tobytes()[:args.bgzf_bytes]
    buf = b"".join(F.bgzf(raw[at: at + 65280]) for at in range(0, len(raw), 65280)) + F.EOF_MARKER
    src, dst = V.DeviceCopy(L, np.frombuffer(buf, dtype=np.uint8).copy()), V.DeviceCopy(L, np.zeros(len(raw), dtype=np.uint8))
    out = {"bgzf_input_bytes": len(raw), "bgzf_file_bytes": len(buf), "range_kernel_ms_by_size": {}}
    names = ("index", "select_items", "frame", "inflate", "check_edges")
    for size in RANGE_SIZES:
        first = len(raw) // 2 - size // 2 + 12345   # (no member boundary: both ends straddle)
        times, calls = [], []
        for it in range(2 + args.reps):   # (two warm-up calls)
            t0 = time.perf_counter()
            rc, res, _, ms = L.inflate_range(src.ptr, len(buf), first, size, dst.ptr, size, None)
            calls.append(1e3 * (time.perf_counter() - t0))
            assert rc == 0 and res.stop == 0 and res.out_size == size, (size, rc, res.stop, res.out_size)
            if it >= 2:
                times.append(ms)
        assert I.device_read(L, dst, size).tobytes() == raw[first: first + size], "the range differs from the input (%d)" % size
        row = {name: float(np.median([t[k] for t in times])) for k, name in enumerate(names)}
        row.update({"call_ms_min": min(calls[2:]), "first_member": res.first_member, "range_members": res.range_members, "members": res.members, "tiles": res.tiles})
        out["range_kernel_ms_by_size"][str(size)] = row
    # the route without the range call: the whole file inflated, the bytes a slice of it
    times, calls = [], []
    for it in range(2 + args.reps):
        t0 = time.perf_counter()
        rc, res, _, ms = L.inflate_file(src.ptr, len(buf), dst.ptr, len(raw), None)
        calls.append(1e3 * (time.perf_counter() - t0))
        assert rc == 0 and res.stop == 0 and res.out_size == len(raw)
        if it >= 2:
            times.append(ms)
    med = [float(np.median([t[k] for t in times])) for k in range(4)]
    out["range_whole_file_route"] = {"index": med[0], "frame": med[1], "inflate": med[2], "check": med[3], "call_ms_min": min(calls[2:]), "members": res.members}
    for size in RANGE_SIZES:
        row = out["range_kernel_ms_by_size"][str(size)]
        row["index_share_of_kernels"] = row["index"] / sum(row[name] for name in names)
        row["select_and_edges_over_inflate"] = (row["select_items"] + row["check_edges"]) / row["inflate"]
        row["call_over_whole_file_call"] = row["call_ms_min"] / out["range_whole_file_route"]["call_ms_min"]
    src.free()
    dst.free()
    print(json.dumps(out), flush=True)
    return 0


def gpu_step(name, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--files", str(args.files), "--file-size", str(args.file_size), "--reps", str(args.reps),
           "--dict-size", str(args.dict_size), "--bgzf-bytes", str(args.bgzf_bytes), "--stream-file", args.stream_file] + (["--lib", args.lib] if args.lib else [])
    r = subprocess.run(cmd, timeout=args.step_timeout, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        sys.exit("step %s failed with status %d: nothing more is started" % (name, r.returncode))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=65536)
    ap.add_argument("--file-size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds every GPU step may take")
    ap.add_argument("--dict-size", type=int, default=32768, help="bytes of the dictionary leg's preset dictionary")
    ap.add_argument("--bgzf-bytes", type=int, default=100 * 1000 * 1000, help="bytes of the corpus the file leg frames as one BGZF file")
    ap.add_argument("--only", default="", help="run only this step (e.g. file) and print its JSON line")
    ap.add_argument("--lib", default="", help="another build of libzultra_amd.so to time instead of the tree's")
    ap.add_argument("--child", choices=["inflate", "verify", "dict", "members", "file", "range"], help="(internal) the process that opens the GPU")
    ap.add_argument("--stream-file", default="", help="(internal) where the inflate step leaves the streams for host zlib")
    args = ap.parse_args()
    if args.child:
        sys.exit({"inflate": child_inflate, "verify": child_verify, "dict": child_dict, "members": child_members, "file": child_file, "range": child_range}[args.child](args))
    import numpy as np
    if args.only:
        print(json.dumps(gpu_step(args.only, args)), flush=True)
        return
    with tempfile.TemporaryDirectory() as tmp:
        args.stream_file = os.path.join(tmp, "streams.npz")
        out = {"files": args.files, "file_size": args.file_size, "input_bytes": args.files * args.file_size}
        out.update(gpu_step("inflate", args))
        out.update(gpu_step("verify", args))
        z = np.load(args.stream_file)
        stream, file_off = z["stream"].tobytes(), z["file_off"]
        with_dict = not args.lib or hasattr(library(args).L, "zultra_hip_inflate_streams_dict")   # (loading the library opens no device)
        if with_dict:
            out.update(gpu_step("dict", args))
            z = np.load(args.stream_file)
            dstream, dict_off = z["stream"].tobytes(), z["file_off"]
        with_members = not args.lib or hasattr(library(args).L, "zultra_hip_inflate_members")
        if with_members:
            out.update(gpu_step("members", args))
        if not args.lib or hasattr(library(args).L, "zultra_hip_inflate_file"):
            out.update(gpu_step("file", args))
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        total = sum(len(zlib.decompress(stream[int(file_off[i]):int(file_off[i + 1])], -15)) for i in range(args.files))
        host.append(1e3 * (time.perf_counter() - t0))
    assert total == out["input_bytes"]
    out["zlib_inflate_one_core_ms"] = {"min": min(host), "all": host}
    out["inflate_over_verify"] = out["inflate_kernel_ms"]["median"] / out["verify_kernel_ms"]["median"]
    out["zlib_over_inflate"] = min(host) / out["inflate_kernel_ms"]["median"]
    out["inflate_GBps_of_output"] = out["input_bytes"] / out["inflate_kernel_ms"]["median"] / 1e6
    if with_dict:
        d, dictionary = records_and_dictionary(args)
        raw, fs, host = d.tobytes(), args.file_size, []
        for rep in range(3):
            t0 = time.perf_counter()
            outs = [zlib.decompressobj(-15, zdict=dictionary).decompress(dstream[int(dict_off[i]):int(dict_off[i + 1])]) for i in range(args.files)]
            host.append(1e3 * (time.perf_counter() - t0))
            if rep == 0:
                assert all(o == raw[i * fs: (i + 1) * fs] for i, o in enumerate(outs)), "host zlib with zdict differs from the records"
        out["zlib_zdict_inflate_one_core_ms"] = {"min": min(host), "all": host}
        out["dict_over_nodict"] = out["dict_inflate_kernel_ms"]["median"] / out["nodict_inflate_kernel_ms"]["median"]
        out["zlib_zdict_over_dict_inflate"] = min(host) / out["dict_inflate_kernel_ms"]["median"]
        out["dict_inflate_GBps_of_output"] = out["input_bytes"] / out["dict_inflate_kernel_ms"]["median"] / 1e6
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
