#!/usr/bin/env python3
"""Times the verification kernel (zh_verify_subblocks, zultra_hip_verify_device) on a benchmark configuration's batch, next to the batch's own
step time from the same context and to host zlib inflating the same stream on one core — the check the reference tool offers. One JSON line.

    python tools/verify_time.py [--config 1|2|3|4|5] [--size BYTES] [--reps N] [--lib PATH]

Configurations 2-4 are one stream of max-blocks (4: 256 MiB of its GiB unless --size says otherwise), 1 is the one small file as one max-block, 5 one
batch of 65 536 inputs of 4 KiB in files mode. The exit status is 1 when the kernel is not faster than host zlib's inflate — the acceptance of the check.
--lib: another build of the library (an A/B of the kernel against an older build, as in tools/inflate_time.py); the line then names it as "lib".

The process that is started touches no GPU: like bench.py it hands the work to a child process, and only the child opens the device."""
import argparse
import json
import os
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def child(args):
    import ctypes as C

    import numpy as np

    import bench
    import zultra_amd
    files = args.config == 5
    if args.config == 1:
        import corpus
        bs, corp, note = 1 << 20, None, "bootstrap.min.js (tests/golden), one max-block"
        d = corpus.bootstrap_js()
    elif files:
        import corpus
        bs, corp, note = 4096, None, "65 536 JSON-like inputs of 4 KiB (tests/gen/zgen.c), each a stream of its own"
        nfiles = (args.size or (65536 * 4096)) // 4096
        d = corpus.json_files(0, nfiles)
    elif args.config == 2:
        bs, size = 65536, args.size or 100_000_000
        corp, note = bench.text_corpus(1, size)
    elif args.config == 3:
        bs, size = 32768, args.size or 51_220_480
        corp, note = bench.binary_corpus(1, size)
    else:
        bs, size = 65536, args.size or (1 << 28)
        size -= size % (1 << 20)
        corp, note = bench.MixedConfig4(), "synthetic mixed-entropy corpus (tests/gen/zgen.c)"
    if corp is not None:
        _, d = corp.shard(0, size)
    d = np.ascontiguousarray(d, dtype=np.uint8)
    nb = (len(d) + bs - 1) // bs
    blocks = [(b * bs - (32768 if b else 0), 32768 if b else 0, min(bs, len(d) - b * bs)) for b in range(nb)]
    if args.lib:
        from zultra_amd._ffi import Lib
        L = Lib(args.lib, allow_missing=("zultra_memory_decompress_dict", "zultra_hip_inflate_streams_dict"))
    else:
        L = zultra_amd.lib()
    if L.device_count() < 1:
        raise RuntimeError("no HIP device visible: nothing can be timed")
    hip = None
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            hip = C.CDLL(name)
            break
        except OSError:
            continue
    if hip is None:
        raise RuntimeError("HIP runtime (libamdhip64.so) not found")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    ctx = L.files_context(bs, nb) if files else L.context(bs, nb)
    offs, sizes = np.arange(nb, dtype=np.uint64) * bs, np.full(nb, bs, dtype=np.uint32)
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), len(d)) == 0 and hip.hipMemcpy(dev, d.ctypes.data, len(d), 1) == 0
    steps, verifies, rep = [], [], None
    for it in range(2 + args.reps):   # (two warm-up batches)
        if files:
            file_off = ctx.compress_files(dev.value, offs, sizes, data_on_device=True, data_size=len(d))
            end_bit = 8 * int(file_off[-1])
        else:
            ctx.stitch_with_batch(nb - 1, 0)
            ctx.compress_blocks(dev.value, blocks, data_on_device=True, data_size=len(d))
            end_bit, _ = ctx.stitch_device(nb - 1, 0)
        rep = ctx.verify()
        if it >= 2:
            steps.append(ctx.timing()["total_ms"])
            verifies.append(rep["verify_ms"])
    stream = ctx.stream_read((end_bit + 7) // 8).tobytes()
    st = ctx.stats()
    ctx.close()
    hip.hipFree(dev)
    inflate = []
    for _ in range(3):
        t0 = time.perf_counter()
        if files:
            out = b"".join(zlib.decompress(stream[int(file_off[i]):int(file_off[i + 1])], -15) for i in range(nb))
        else:
            out = zlib.decompress(stream, -15)
        inflate.append(1e3 * (time.perf_counter() - t0))
    assert out == d.tobytes(), "host zlib does not inflate the device's stream to the input"
    below = float(np.median(verifies)) < min(inflate)
    print(json.dumps({
        "config": args.config, "corpus": note, "input_bytes": len(d), "stream_bytes": len(stream), "max_block": bs, "max_blocks": nb, "subblocks": st["subblocks"],
        "verify_rc": rep["rc"], "verified_bytes": rep["verified_bytes"],
        "verify_kernel_ms": {"min": min(verifies), "median": float(np.median(verifies)), "all": verifies},
        "step_ms": {"min": min(steps), "median": float(np.median(steps)), "all": steps},
        "zlib_inflate_one_core_ms": {"min": min(inflate), "all": inflate},
        "verify_over_step": float(np.median(verifies)) / float(np.median(steps)),
        "verify_below_zlib_inflate": below,
        "csrc_digest": zultra_amd.csrc_digest(), "lib": args.lib or "this tree",
    }), flush=True)
    return 0 if below and rep["rc"] == 0 else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2, choices=[1, 2, 3, 4, 5])
    ap.add_argument("--size", type=int, default=0, help="bytes (default: the configuration's own; configuration 4: 256 MiB)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default="", help="another build of libzultra_amd.so to time instead of the tree's")
    ap.add_argument("--child", action="store_true", help="(internal) the process that opens the GPU")
    args = ap.parse_args()
    if args.child:
        sys.exit(child(args))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:], timeout=1500)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
