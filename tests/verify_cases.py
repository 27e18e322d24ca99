"""Shared by tests/test_verify_emu.py (CPU emulator build) and tests/test_verify_gpu.py (product library on the MI355X): the inputs, the
batch builder and the checks of zultra_hip_verify_device. Both files run the same generators; the emulator takes smaller windows."""
import ctypes as C
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":   # (the recorder at the end of the file: no conftest has set the path up)
    sys.path[:0] = [os.path.dirname(HERE), os.path.join(HERE, "emu")]

import corpus
from zultra_amd._ffi import Block

HISTORY = 32768
FLIP_REPORTS = os.path.join(HERE, "golden", "verify_flip_reports.json")


def many_splits(stretch):
    """The pattern of test_gpu_parity.py::test_many_sub_blocks_in_one_max_block: 64 stretches over 16 byte values each, neighbours in different bins
    of the splitter's statistics (41 sub-blocks at 32 KiB per stretch in one 2 MiB max-block)."""
    parts = []
    for k in range(64):
        r = corpus.noise(stretch, 500 + k)
        parts.append(((((k >> 2) & 3) << 6) | ((r & 15) << 2) | (k & 3)).astype(np.uint8))
    return np.concatenate(parts)


def text_noise_text(n_text, n_noise):
    t = corpus.text_like(2 * n_text, 5)
    return np.concatenate([t[:n_text], corpus.noise(n_noise, 3), t[n_text:]])


# (name, generator, bytes per max-block of the stream, max-block size the context is created with)
CLEAN_GPU = [
    ("text", lambda: corpus.text_like(200000, 3), 65536, 65536),
    ("mixed", lambda: corpus.mixed(98304, 5), 32768, 32768),
    ("json", lambda: corpus.json_like(100000, 3), 32768, 32768),
    ("noise", lambda: corpus.noise(40000, 1), 32768, 32768),
    ("noise_multi_piece", lambda: corpus.noise(150000, 2), 1 << 20, 1 << 20),
    ("constant", lambda: corpus.constant(70000), 65536, 65536),
    ("periodic", lambda: corpus.periodic(50000, 3), 32768, 32768),
    ("selftest2", lambda: corpus.selftest_data(49152, 123, 2, 0.5), 32768, 32768),
    ("selftest15", lambda: corpus.selftest_data(49152, 123, 15, 0.5), 32768, 32768),
    ("selftest256", lambda: corpus.selftest_data(49152, 123, 256, 0.0), 32768, 32768),
    ("fibonacci", lambda: corpus.fibonacci_bytes(22), 65536, 65536),
    ("one", lambda: corpus.text_like(1, 1), 32768, 32768),
    ("three", lambda: corpus.text_like(3, 1), 32768, 32768),
    ("ten", lambda: corpus.text_like(10, 1), 32768, 32768),
    ("many_splits", lambda: many_splits(32768), 2 << 20, 2 << 20),
    ("text_noise_text", lambda: text_noise_text(45000, 33000), 32768, 32768),
    ("text_1m", lambda: corpus.text_like(1300000, 6), 1 << 20, 1 << 20),
    ("text_odd_block", lambda: corpus.text_like(150000, 7), 50001, 50001),
]
CLEAN_EMU = [
    ("text", lambda: corpus.text_like(9000, 3), 4000, 32768),
    ("mixed", lambda: corpus.mixed(98304, 5)[56000:64000], 4000, 32768),   # (two-symbol segment, then text: the first 36 KB are one byte value)
    ("json", lambda: corpus.json_like(6000, 3), 3000, 32768),
    ("noise", lambda: corpus.noise(3000, 1), 2000, 32768),
    ("constant", lambda: corpus.constant(6000), 3000, 32768),
    ("periodic", lambda: corpus.periodic(2500, 3), 2500, 32768),
    ("selftest2", lambda: corpus.selftest_data(5000, 5, 2, 0.3), 3000, 32768),
    ("selftest15", lambda: corpus.selftest_data(6000, 77, 15, 0.5), 3000, 32768),
    ("selftest256", lambda: corpus.selftest_data(4000, 9, 256, 0.0), 4000, 32768),
    ("fibonacci", lambda: corpus.fibonacci_bytes(19), 10945, 32768),
    ("one", lambda: corpus.text_like(1, 1), 32768, 32768),
    ("three", lambda: corpus.text_like(3, 1), 32768, 32768),
    ("ten", lambda: corpus.text_like(10, 1), 32768, 32768),
    ("many_splits", lambda: many_splits(600), 38400, 65536),
    ("text_noise_text", lambda: text_noise_text(3000, 1500), 2501, 32768),
]

# single-bit flips: (name, generator, bytes per max-block, context max-block, flips, held to the 5 % cap of benign flips)
FLIPS_GPU = [
    ("text", lambda: corpus.text_like(65536, 3), 32768, 32768, 200, True),
    ("mixed", lambda: corpus.mixed(98304, 5), 32768, 32768, 200, True),
    ("json", lambda: corpus.json_like(4096, 3), 32768, 32768, 200, True),
    ("noise", lambda: corpus.noise(40000, 1), 32768, 32768, 200, True),
    ("constant", lambda: corpus.constant(70000), 65536, 65536, 100, False),
]
FLIPS_EMU = [
    ("text", lambda: corpus.text_like(5000, 3), 2500, 32768, 40, True),
    ("mixed", lambda: corpus.mixed(98304, 5)[58000:63000], 2500, 32768, 40, True),
    ("json", lambda: corpus.json_like(3000, 3), 3000, 32768, 40, True),
    ("noise", lambda: corpus.noise(2500, 1), 1500, 32768, 40, True),
    ("constant", lambda: corpus.constant(6000), 3000, 32768, 40, False),
]
BENIGN_CAP = 0.05


def stream_blocks(total, per_block):
    """Consecutive max-blocks over one buffer, history from the buffer: [(win_off, prev, n)]."""
    blocks, off = [], 0
    while off < total:
        n = min(per_block, total - off)
        prev = min(HISTORY, off)
        blocks.append((off - prev, prev, n))
        off += n
    return blocks


class _Hip:
    """hipMalloc / hipMemcpy of the HIP runtime the product library is linked against (no torch: it cannot initialise HIP behind the library)."""
    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
                try:
                    cls._lib = C.CDLL(name)
                    break
                except OSError:
                    continue
            assert cls._lib is not None, "HIP runtime not found"
            cls._lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            cls._lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            cls._lib.hipFree.argtypes = [C.c_void_p]
        return cls._lib


class DeviceCopy:
    """A device copy of `data` for data_on_device == 1. Under the emulator device memory is host memory: the array itself. Which of the two `lib`
    is, its fixture says (lib.is_emulator)."""

    def __init__(self, lib, data):
        self.emu = bool(lib.is_emulator)
        self.data = data
        if self.emu:
            self.ptr = data.ctypes.data
        else:
            p = C.c_void_p()
            assert _Hip.lib().hipMalloc(C.byref(p), max(len(data), 1)) == 0
            assert _Hip.lib().hipMemcpy(p, data.ctypes.data, len(data), 1) == 0
            self.ptr = p.value

    def free(self):
        if not self.emu and self.ptr:
            _Hip.lib().hipFree(self.ptr)
            self.ptr = None


def compress(lib, ctx, data, blocks, mode=0):
    """zultra_hip_compress_blocks with data_on_device = mode (0 host, 1 device pointer, 2 pageable host staged run by run). Returns what keeps the
    input alive until the verify call."""
    arr = (Block * len(blocks))(*[Block(int(o), int(p), int(n)) for (o, p, n) in blocks])
    keep = DeviceCopy(lib, data) if mode == 1 else None
    ptr = keep.ptr if mode == 1 else data.ctypes.data
    n = lib.L.zultra_hip_compress_blocks(ctx.h, ptr, len(data), mode, arr, len(blocks))
    assert n > 0, lib.L.zultra_hip_last_error(ctx.h).decode()
    return keep


def plan(subs, max_block, phase=0):
    """The stitcher's rule (zh_stitch_step) in Python: first header bit of every sub-block, and the end bit."""
    cap = 1 + max_block + 5 * (max_block // 65535 + 1)
    bit, base, cur, out = phase, 0, None, []
    for sb in subs:
        if sb.block != cur:
            cur, base = sb.block, bit >> 3
        out.append(bit)
        nacc = bit & 7
        o0 = ((bit >> 3) - base) + ((nacc + 3) >> 3)
        body = (((nacc + 3) & 7) + sb.nbits) >> 3
        if not sb.failed and body <= sb.size and o0 + body <= cap:
            bit += 3 + sb.nbits
        else:
            rem = sb.size
            while rem:
                piece = min(rem, 65535)
                bit = (bit + 3 + 7) & ~7
                bit += 32 + 8 * piece
                rem -= piece
    return out, bit


def inflates_to(stream, want):
    """Host zlib's verdict on a raw deflate stream: inflates without error, reaches the end, gives `want`."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(bytes(stream))
    except zlib.error:
        return False
    return d.eof and out == want


def check_clean(lib, name, gen, per_block, max_block, phase=0, final=True, mode=0):
    """One stream stitched on the device and verified: the return value, the report, and — at phase 0 with BFINAL — host zlib on the same bytes."""
    data = np.ascontiguousarray(gen(), dtype=np.uint8)
    blocks = stream_blocks(len(data), per_block)
    ctx = lib.context(max_block, len(blocks))
    keep = None
    try:
        keep = compress(lib, ctx, data, blocks, mode)
        end_bit, _ = ctx.stitch_device(len(blocks) - 1 if final else -1, phase)
        r = ctx.verify()
        assert r["rc"] == 0 and r["bad_subblocks"] == 0, (name, r)
        assert r["verified_bytes"] == len(data), (name, r)
        assert r["first_bad"] == 0xFFFFFFFF
        if phase == 0 and final:
            stream = ctx.stream_read((end_bit + 7) // 8).tobytes()
            assert zlib.decompress(stream, -15) == data.tobytes(), name
        return r
    finally:
        if keep:
            keep.free()
        ctx.close()


def targeted_bits(subs, starts, end_bit):
    """Bits worth flipping on purpose: {label: bit}. Needs a stream with a dynamic and a stored sub-block and at least three sub-blocks."""
    t = {}
    nxt = starts[1:] + [end_bit]
    mid = len(subs) // 2
    t["bfinal_middle"] = starts[mid]
    t["bfinal_last"] = starts[-1]
    t["btype_lo"] = starts[mid] + 1
    t["btype_hi"] = starts[mid] + 2
    for k, sb in enumerate(subs):
        bits = nxt[k] - starts[k]
        stored = bits >= 8 * sb.size + 32
        if not stored and sb.is_dynamic and "hlit" not in t:
            t["hlit"] = starts[k] + 3 + 2
            t["hdist"] = starts[k] + 8 + 1
            t["hclen"] = starts[k] + 13 + 1
        if stored and "stored_len" not in t:
            byte0 = (starts[k] + 3 + 7) >> 3
            t["stored_len"] = byte0 * 8 + 3
            t["stored_nlen"] = byte0 * 8 + 16 + 5
            t["stored_byte"] = (byte0 + 4 + sb.size // 2) * 8 + 6
    t["last_valid_bit"] = end_bit - 1
    return t


def check_flips(lib, name, gen, per_block, max_block, nflips, capped, seed, targeted=False):
    """Single-bit flips of a phase-0 final stream, one per verify call: verify says 1 exactly when host zlib does not inflate the mutated stream to
    the input, and then names the sub-block whose bits hold the flip. Returns (flips, benign flips)."""
    data = np.ascontiguousarray(gen(), dtype=np.uint8)
    want = data.tobytes()
    blocks = stream_blocks(len(data), per_block)
    ctx = lib.context(max_block, len(blocks))
    try:
        compress(lib, ctx, data, blocks, 0)
        end_bit, _ = ctx.stitch_device(len(blocks) - 1, 0)
        subs, _, cnt = ctx.subblocks()
        starts, planned_end = plan(subs, max_block, 0)
        assert planned_end == end_bit
        nbytes = (end_bit + 7) // 8
        clean = ctx.stream_read(nbytes).copy()
        assert inflates_to(clean, want)
        assert ctx.verify()["rc"] == 0
        rs = np.random.RandomState(seed)
        bits = [(("flip%d" % i), int(b)) for i, b in enumerate(rs.randint(0, end_bit, size=nflips))]
        if targeted:
            t = targeted_bits(subs, starts, end_bit)
            assert {"hlit", "stored_len", "bfinal_middle"} <= set(t), sorted(t)
            bits += sorted(t.items())
        benign = 0
        for label, bit in bits:
            byte = clean[bit >> 3: (bit >> 3) + 1].copy()
            byte[0] ^= 1 << (bit & 7)
            mutated = clean.copy()
            mutated[bit >> 3] = byte[0]
            ok = inflates_to(mutated, want)
            ctx.stream_write(byte, bit >> 3)
            r = ctx.verify()
            ctx.stream_write(clean[bit >> 3: (bit >> 3) + 1], bit >> 3)
            print("%s %s bit %d: zlib %s verify rc %d reason %d first_bad %d" % (name, label, bit, "ok" if ok else "bad", r["rc"], r["reason"], r["first_bad"] if r["rc"] else -1))
            assert r["rc"] == (0 if ok else 1), (name, label, bit, ok, r)
            if ok:
                benign += 1 if label.startswith("flip") else 0
            else:
                holder = max(k for k in range(cnt) if starts[k] <= bit)
                assert r["first_bad"] == holder, (name, label, bit, holder, r)
        assert ctx.verify()["rc"] == 0   # (the buffer is restored)
        if capped:
            assert benign <= BENIGN_CAP * nflips, "%s: %d of %d flips still inflate to the input: the case tests little" % (name, benign, nflips)
        return len(bits), benign
    finally:
        ctx.close()


def check_files(lib, nrecords):
    """Files mode: 4 KiB json records plus inputs of 1, 2 and 8191 bytes, each a stream of its own; then one file's bytes corrupted."""
    sizes = [4096] * nrecords + [1, 2, 8191]
    parts = [corpus.json_like(4096, 10 + i) for i in range(nrecords)] + [corpus.text_like(1, 2), corpus.text_like(2, 3), corpus.json_like(8191, 4)]
    data = np.concatenate(parts)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    ctx = lib.files_context(8191, len(sizes))
    try:
        file_off = ctx.compress_files(data, offsets, sizes)
        r = ctx.verify()
        assert r["rc"] == 0 and r["bad_subblocks"] == 0 and r["verified_bytes"] == sum(sizes), r
        for i in range(len(sizes)):
            raw = ctx.stream_read(int(file_off[i + 1] - file_off[i]), int(file_off[i])).tobytes()
            assert zlib.decompress(raw, -15) == parts[i].tobytes()
        victim = nrecords // 2
        at = int(file_off[victim] + file_off[victim + 1]) // 2
        old = ctx.stream_read(1, at).copy()
        ctx.stream_write(old ^ np.uint8(0xFF), at)
        r = ctx.verify()
        assert r["rc"] == 1 and r["first_bad"] == victim and r["bad_subblocks"] == 1 and r["block"] == victim, r
        assert r["verified_bytes"] == sum(sizes) - sizes[victim], r
        ctx.stream_write(old, at)
        assert ctx.verify()["rc"] == 0
    finally:
        ctx.close()


def _flip_rows(ctx, subs, starts, end_bit, seed):
    """The fixed list of single-bit flips of flip_reports over the stitched stream in `ctx`, one verify call each:
    [[bit, rc, reason, first_bad, block, input_off, stream_bit]] and the clean stream's CRC-32."""
    nbytes = (end_bit + 7) // 8
    clean = ctx.stream_read(nbytes).copy()
    assert ctx.verify()["rc"] == 0
    assert nbytes > 8 and starts[-1] + 24 <= end_bit
    bits = sorted(targeted_bits(subs, starts, end_bit).values())
    bits += [int(b) for b in np.random.RandomState(seed).randint(0, end_bit, size=200)]
    bits += range(8 * (nbytes - 8), 8 * nbytes)      # the end of the data (the pad bits of the last byte included) ...
    bits += range(starts[-1], starts[-1] + 24)       # ... and the last sub-block's header: where the order of the decoder's verdicts shows
    rows = []
    for bit in bits:
        at = bit >> 3
        ctx.stream_write(clean[at: at + 1] ^ np.uint8(1 << (bit & 7)), at)
        r = ctx.verify()
        ctx.stream_write(clean[at: at + 1], at)
        rows.append([bit] + [r[k] for k in ("rc", "reason", "first_bad", "block", "input_off", "stream_bit")])
    assert ctx.verify()["rc"] == 0   # (the buffer is restored)
    return {"end_bit": end_bit, "crc32": zlib.crc32(clean.tobytes()), "rows": rows}


def flip_reports(lib):
    """The whole report of zultra_hip_verify_device — not only its verdict — for a fixed, seeded list of single-bit flips of two small streams: the one
    of test_targeted_flips_get_zlibs_verdict in the emulator's size (dynamic and stored sub-blocks) and a files batch of two 4 KiB records and inputs
    of 1, 2 and 8191 bytes. -> {stream name: {"end_bit", "crc32" of the clean stream, "rows"}}; tests/golden/verify_flip_reports.json holds what the
    decoder said before zh_deflate_dec.h was shared between the verify and the inflate kernels."""
    out = {}
    data = np.ascontiguousarray(text_noise_text(2000, 2000), dtype=np.uint8)
    blocks = stream_blocks(len(data), 2000)
    ctx = lib.context(32768, len(blocks))
    try:
        compress(lib, ctx, data, blocks, 0)
        end_bit, _ = ctx.stitch_device(len(blocks) - 1, 0)
        subs, _, cnt = ctx.subblocks()
        starts, planned_end = plan(subs, 32768, 0)
        assert planned_end == end_bit and cnt >= 3
        assert {"hlit", "stored_len"} <= set(targeted_bits(subs, starts, end_bit))
        out["targeted"] = _flip_rows(ctx, subs, starts, end_bit, 20260117)
    finally:
        ctx.close()
    sizes = [4096, 4096, 1, 2, 8191]
    data = np.concatenate([corpus.json_like(4096, 10), corpus.json_like(4096, 11), corpus.text_like(1, 2), corpus.text_like(2, 3), corpus.json_like(8191, 4)])
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    ctx = lib.files_context(8191, len(sizes))
    try:
        file_off = ctx.compress_files(data, offsets, sizes)
        subs, _, cnt = ctx.subblocks()
        starts = []
        for f in range(len(sizes)):   # every file is a stream of its own, from a byte boundary
            s, end = plan([sb for sb in subs if sb.block == f], 8191, 0)
            starts += [8 * int(file_off[f]) + b for b in s]
            assert int(file_off[f]) + (end + 7) // 8 == int(file_off[f + 1])
        assert len(starts) == cnt
        out["files"] = _flip_rows(ctx, subs, starts, 8 * int(file_off[-1]), 20260118)
    finally:
        ctx.close()
    return out


def check_flip_reports(lib):
    """The build under test gives the recorded reports, field for field."""
    with open(FLIP_REPORTS) as f:
        want = json.load(f)["streams"]
    got = flip_reports(lib)
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert (got[name]["end_bit"], got[name]["crc32"]) == (want[name]["end_bit"], want[name]["crc32"]), "%s: the compressor's stream is another one" % name
        assert len(got[name]["rows"]) == len(want[name]["rows"])
        for g, w in zip(got[name]["rows"], want[name]["rows"]):
            assert g == w, "%s: bit, rc, reason, first_bad, block, input_off, stream_bit: got %s, recorded %s" % (name, g, w)


if __name__ == "__main__":
    # python tests/verify_cases.py --record PATH [SOURCE]: the reports of this tree's emulator build, written as the golden file. SOURCE says which
    # commit the tree is (the file is recorded from the commit BEFORE a change to the decoder, never from the code under test).
    assert len(sys.argv) in (3, 4) and sys.argv[1] == "--record", "usage: verify_cases.py --record PATH [SOURCE]"
    import build_emu
    from zultra_amd._ffi import Lib
    emu = Lib(build_emu.build())
    emu.is_emulator = True
    streams = flip_reports(emu)
    with open(sys.argv[2], "w") as f:
        f.write('{"recorded_from": %s,\n "row": ["bit", "rc", "reason", "first_bad", "block", "input_off", "stream_bit"],\n "streams": {\n' % json.dumps(sys.argv[3] if len(sys.argv) == 4 else "unnamed tree"))
        for i, name in enumerate(sorted(streams)):
            s = streams[name]
            f.write('  %s: {"end_bit": %d, "crc32": %d, "rows": [\n' % (json.dumps(name), s["end_bit"], s["crc32"]))
            f.write(",\n".join("   " + json.dumps(r) for r in s["rows"]))
            f.write("]}%s\n" % ("," if i + 1 < len(streams) else ""))
        f.write(" }}\n")
    print("%s: %s" % (sys.argv[2], ", ".join("%s %d rows" % (k, len(v["rows"])) for k, v in sorted(streams.items()))))
