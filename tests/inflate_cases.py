"""Shared by tests/test_inflate_emu.py (CPU emulator build) and tests/test_inflate_gpu.py (product library on the MI355X): the streams, the batch
runner and the checks of zultra_hip_inflate_streams (zultra_amd/csrc/zh_inflate_out.h) and zultra_memory_decompress. The yardstick is Python's zlib
on the host. Both files run the same cases; the emulator takes the smaller sizes."""
import ctypes as C
import bisect
import gzip
import io
import os
import pickle
import random
import subprocess
import sys
import zlib

import numpy as np

import corpus
import verify_cases as V

CANARY = 16          # bytes between two destination ranges
CANARY_BYTE = 0xA5   # ... and what the whole destination holds before the call

# reasons (include/zultra_hip.h)
OK, HEADER, CODELENS, SYMBOL, DISTANCE, STORED_LEN, STREAM_END, DST_FULL = 0, 1, 2, 3, 4, 7, 12, 13


# ---- running a batch ----------------------------------------------------------------------------------------------------------------------
def device_read(lib, dc, n):
    """The first n bytes behind a verify_cases.DeviceCopy, as a host array (under the emulator device memory is the array itself)."""
    if dc.emu:
        return dc.data[:n]
    out = np.empty(max(n, 1), dtype=np.uint8)
    assert V._Hip.lib().hipMemcpy(out.ctypes.data, dc.ptr, n, 2) == 0
    return out[:n]


def check_canaries(back, items, res):
    """Nothing outside [dst_off, dst_off + out_size) of any item has been written."""
    mask = np.ones(len(back), dtype=bool)
    for (_, _, doff, cap), r in zip(items, res):
        assert int(r["out_size"]) <= cap, (doff, cap, r)
        mask[doff: doff + int(r["out_size"])] = False
    assert (back[mask] == CANARY_BYTE).all(), "bytes outside the items' output were written at %s" % np.nonzero(mask & (back != CANARY_BYTE))[0][:8]


def run_streams(lib, streams, caps, on_device=True, src_sizes=None):
    """The streams packed back to back (source offsets of every residue mod 4), the destination ranges `caps` long and CANARY bytes apart.
    on_device: both buffers in device memory, used in place; else host arrays, staged by the call. src_sizes: what the items give as src_size
    instead of the streams' lengths (truncation). -> (rc, [(reason, blocks, out_size, src_used, output bytes)])."""
    src = np.frombuffer(b"".join(bytes(s) for s in streams) + b"\0", dtype=np.uint8).copy()[:-1]
    items, soff, doff = [], 0, CANARY
    for k, s in enumerate(streams):
        items.append((soff, len(s) if src_sizes is None else src_sizes[k], doff, caps[k]))
        soff += len(s)
        doff += caps[k] + CANARY
    dst = np.full(doff, CANARY_BYTE, dtype=np.uint8)
    if on_device:
        s, d = V.DeviceCopy(lib, src), V.DeviceCopy(lib, dst)
        try:
            rc, res, _ = lib.inflate_streams(s.ptr, len(src), d.ptr, len(dst), items)
            back = device_read(lib, d, len(dst)).copy()
        finally:
            s.free()
            d.free()
    else:
        rc, res, _ = lib.inflate_streams(src, len(src), dst, len(dst), items)
        back = dst
    assert rc >= 0, "zultra_hip_inflate_streams failed"
    assert rc == int((res["reason"] != 0).sum())
    check_canaries(back, items, res)
    return rc, [(int(r["reason"]), int(r["blocks"]), int(r["out_size"]), int(r["src_used"]), back[it[2]: it[2] + int(r["out_size"])].tobytes()) for it, r in zip(items, res)]


def host_verdict(stream):
    """Host zlib on a raw deflate stream -> (inflates without error and reaches the end, output, bytes of the stream used)."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(bytes(stream))
    except zlib.error:
        return False, b"", 0
    return bool(d.eof), out, len(stream) - len(d.unused_data)


def check_good(lib, named, on_device=True):
    """Every (name, stream, want) decodes to `want`, uses the whole stream, and host zlib agrees."""
    for name, s, want in named:
        ok, out, used = host_verdict(s)
        assert ok and out == want and used == len(s), name
    rc, res = run_streams(lib, [s for _, s, _ in named], [len(w) for _, _, w in named], on_device)
    for (name, s, want), (reason, blocks, out_size, src_used, out) in zip(named, res):
        assert reason == OK, (name, reason, out_size, src_used)
        assert out_size == len(want) and out == want, (name, out_size, len(want))
        assert src_used == len(s), (name, src_used, len(s))
        assert blocks >= 1
    assert rc == 0
    return res


# ---- 1. foreign streams: what this library's coder never emits -------------------------------------------------------------------------------
VARIANTS = [("l0", 0, zlib.Z_DEFAULT_STRATEGY), ("l1", 1, zlib.Z_DEFAULT_STRATEGY), ("l6", 6, zlib.Z_DEFAULT_STRATEGY), ("l9", 9, zlib.Z_DEFAULT_STRATEGY),
            ("fixed", 6, zlib.Z_FIXED), ("huffman", 6, zlib.Z_HUFFMAN_ONLY), ("rle", 6, zlib.Z_RLE)]
FOREIGN = {   # name -> generator of the input
    "text": lambda: corpus.text_like(9000, 3),
    "json": lambda: corpus.json_like(6000, 3),
    "noise": lambda: corpus.noise(3000, 1),
    "constant": lambda: corpus.constant(5000, 7),
    "periodic": lambda: corpus.periodic(4000, 3),
}
FOREIGN_GPU_ONLY = {"text300k": lambda: corpus.text_like(300000, 4)}


def zlib_raw(data, level, strategy, flush_every=0):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    data = bytes(data)
    if not flush_every:
        return c.compress(data) + c.flush()
    out = b""
    for at in range(0, len(data), flush_every):
        out += c.compress(data[at: at + flush_every]) + c.flush(zlib.Z_SYNC_FLUSH)
    return out + c.flush()


def foreign_streams(gen):
    d = np.ascontiguousarray(gen(), dtype=np.uint8).tobytes()
    return [(name, zlib_raw(d, level, strategy), d) for name, level, strategy in VARIANTS]


def check_foreign(lib, gen):
    check_good(lib, foreign_streams(gen), on_device=False)


def check_sync_flushes(lib):
    """Z_SYNC_FLUSH every 1000 bytes: an empty stored block behind every piece, and two in a row at the end."""
    d = corpus.text_like(9000, 5).tobytes()
    s = zlib_raw(d, 6, zlib.Z_DEFAULT_STRATEGY, flush_every=1000) + b""
    res = check_good(lib, [("sync", s, d), ("sync_l0", zlib_raw(d, 0, zlib.Z_DEFAULT_STRATEGY, flush_every=1000), d)])
    assert res[0][1] >= 18, res[0][1]   # (nine pieces, each a block and an empty stored block)


def check_stored_pieces(lib):
    d = corpus.noise(70000, 9).tobytes()
    res = check_good(lib, [("noise_l0", zlib_raw(d, 0, zlib.Z_DEFAULT_STRATEGY), d)])
    assert res[0][1] >= 2


# ---- 2. hand-written token streams: a fixed-Huffman bit writer ----------------------------------------------------------------------------------
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_XBITS = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_XBITS = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]


class BitWriter:
    """RFC 1951 by hand: stored blocks, and fixed-Huffman blocks from literals, (len, dist) tokens, raw symbols and block ends."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):           # LSB first (header fields, extra bits)
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, nbits):          # Huffman codes go in from their most significant bit: one put of the code's bits reversed
        self.put(int(format(value & ((1 << nbits) - 1), "0%db" % nbits)[::-1], 2) if nbits else 0, nbits)

    def begin_fixed(self, final):
        self.put(1 if final else 0, 1)
        self.put(1, 2)

    def begin_btype(self, final, btype):
        self.put(1 if final else 0, 1)
        self.put(btype, 2)

    def sym(self, s):                      # literal / length symbol 0..287 of the fixed code (RFC 1951 3.2.6)
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def lits(self, data):
        for b in bytes(data):
            self.sym(b)

    def dist_sym(self, ds):
        self.code(ds, 5)

    def match(self, length, dist):
        li = max(k for k in range(29) if LEN_BASE[k] <= length) if length < 258 else 28
        self.sym(257 + li)
        self.put(length - LEN_BASE[li], LEN_XBITS[li])
        di = max(k for k in range(30) if DIST_BASE[k] <= dist)
        self.dist_sym(di)
        self.put(dist - DIST_BASE[di], DIST_XBITS[di])

    def eob(self):
        self.sym(256)

    def stored(self, data, final):
        self.put(1 if final else 0, 1)
        self.put(0, 2)
        if self.n:
            self.put(0, 8 - self.n)
        data = bytes(data)
        assert len(data) <= 65535
        self.out += len(data).to_bytes(2, "little") + (len(data) ^ 0xFFFF).to_bytes(2, "little") + data

    def bytes(self):
        if self.n:
            self.put(0, 8 - self.n)
        return bytes(self.out)


def _pattern(n, seed=0):
    return bytes(((i * 7 + 3 + seed * 31) ^ (i >> 5)) & 255 for i in range(n))


def _with_zlib(name, stream):
    ok, out, used = host_verdict(stream)
    assert ok and used == len(stream), name
    return (name, stream, out)


def hand_matches():
    """dist 1, 2, 3, 63, 64, 65 with len 3, 64, 65, 257, 258, each behind exactly `dist` literals and followed by two more tokens."""
    out = []
    for dist in (1, 2, 3, 63, 64, 65):
        for length in (3, 64, 65, 257, 258):
            w = BitWriter()
            w.begin_fixed(True)
            w.lits(_pattern(dist, dist))
            w.match(length, dist)
            w.lits(b"ok")
            w.match(4, 2)
            w.eob()
            out.append(_with_zlib("d%d_l%d" % (dist, length), w.bytes()))
    return out


def hand_after_literals():
    """A match right behind 1, 63, 64 (and 130) literals whose source lies inside those literals: they are still in the lanes when it arrives."""
    out = []
    for nlit, dist, length in ((1, 1, 10), (63, 63, 70), (63, 5, 9), (63, 1, 258), (64, 64, 64), (64, 1, 3), (64, 33, 100), (130, 3, 11), (130, 66, 258)):
        w = BitWriter()
        w.begin_fixed(True)
        w.lits(_pattern(nlit, nlit + dist))
        w.match(length, dist)
        w.eob()
        out.append(_with_zlib("n%d_d%d_l%d" % (nlit, dist, length), w.bytes()))
    return out


def hand_far():
    """dist 32768 with len 258 at output position exactly 32768 (zlib never produces this distance, this library does): 32768 literals in stored
    blocks, then one fixed block."""
    w = BitWriter()
    d = corpus.text_like(32768, 11).tobytes()
    w.stored(d[:20000], False)
    w.stored(d[20000:], False)
    w.begin_fixed(True)
    w.match(258, 32768)
    w.lits(b"end")
    w.match(258, 32768)
    w.eob()
    name, s, want = _with_zlib("far", w.bytes())
    assert want == d + d[:258] + b"end" + d[261: 261 + 258]
    return [(name, s, want)]


def hand_bad():
    """-> [(name, stream, reason)]: streams host zlib rejects as well."""
    out = []
    for produced in (0, 1, 63, 64, 100):      # dist = produced + 1: one byte in front of the item's output
        w = BitWriter()
        w.begin_fixed(True)
        w.lits(_pattern(produced))
        w.match(5, produced + 1)
        w.lits(b"tail of the stream")
        w.eob()
        out.append(("before_start_%d" % produced, w.bytes(), DISTANCE))
    for s in (286, 287):
        w = BitWriter()
        w.begin_fixed(True)
        w.lits(b"abc")
        w.sym(s)
        w.dist_sym(0)
        w.lits(b"tail of the stream")
        w.eob()
        out.append(("length_symbol_%d" % s, w.bytes(), SYMBOL))
    for ds in (30, 31):
        w = BitWriter()
        w.begin_fixed(True)
        w.lits(b"abc")
        w.sym(257)
        w.dist_sym(ds)
        w.lits(b"tail of the stream")
        w.eob()
        out.append(("distance_symbol_%d" % ds, w.bytes(), DISTANCE))
    w = BitWriter()
    w.begin_fixed(False)
    w.lits(b"abc")
    w.eob()
    w.begin_btype(True, 3)
    w.put(0, 29)
    out.append(("btype3", w.bytes(), HEADER))
    for name, s, _ in out:
        assert not host_verdict(s)[0], name
    return out


def check_hand_good(lib):
    check_good(lib, hand_matches() + hand_after_literals() + hand_far())


def check_hand_bad(lib):
    bad = hand_bad()
    rc, res = run_streams(lib, [s for _, s, _ in bad], [600] * len(bad))
    assert rc == len(bad)
    for (name, s, want), (reason, blocks, out_size, src_used, out) in zip(bad, res):
        assert reason == want, (name, reason, want)
    # what was written before the failure is what the stream said: the three literals of the symbol cases
    assert res[5][4] == b"abc" and res[7][4] == b"abc", (res[5], res[7])


# ---- 3. own streams, device to device ---------------------------------------------------------------------------------------------------------
FILE_SIZES = [1, 2, 63, 64, 65, 100, 4095, 4096, 8191]


def check_own_files(lib, nfiles):
    """A files batch compressed on the device and inflated from the context's stream buffer into device memory: every input comes back."""
    sizes = [FILE_SIZES[i % len(FILE_SIZES)] for i in range(nfiles)]
    gens = (corpus.json_like, corpus.text_like)
    parts = [gens[i & 1](n, 100 + i) for i, n in enumerate(sizes)]
    data = np.concatenate(parts)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    ctx = lib.files_context(8191, nfiles)
    d = None
    try:
        file_off = ctx.compress_files(data, offsets, sizes)
        items, doff = [], CANARY
        for i, n in enumerate(sizes):
            items.append((int(file_off[i]), int(file_off[i + 1] - file_off[i]), doff, n))
            doff += n + CANARY
        dst = np.full(doff, CANARY_BYTE, dtype=np.uint8)
        d = V.DeviceCopy(lib, dst)
        rc, res, ms = lib.inflate_streams(ctx.stream_ptr(), int(file_off[-1]), d.ptr, len(dst), items)
        back = device_read(lib, d, len(dst)).copy()
        assert rc == 0, (rc, res[res["reason"] != 0][:4])
        check_canaries(back, items, res)
        for i, (it, r) in enumerate(zip(items, res)):
            assert int(r["out_size"]) == sizes[i] and int(r["src_used"]) == it[1], (i, r, it)
            assert back[it[2]: it[2] + sizes[i]].tobytes() == parts[i].tobytes(), i
        assert {it[0] & 3 for it in items} == {0, 1, 2, 3}
        return ms
    finally:
        if d:
            d.free()
        ctx.close()


def check_own_files_strided(lib_path, is_emulator, nfiles):
    """The same batch in a process of its own with ZULTRA_HIP_GRID_CAP=8: eight waves stride over the batch."""
    tests = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import inflate_cases as I\nfrom zultra_amd._ffi import Lib\nL = Lib(%r)\nL.is_emulator = %r\n"
            "I.check_own_files(L, %d)\nprint('strided ok')\n") % (os.path.dirname(tests), tests, lib_path, bool(is_emulator), nfiles)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ZULTRA_HIP_GRID_CAP="8"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "strided ok" in r.stdout, r.stdout + r.stderr


def check_own_blocks(lib, size, max_block):
    """One blocks-mode stream of the library's own coder, raw framing (its matches reach back 32768 bytes)."""
    d = corpus.text_like(size, 21)
    s = lib.memory_compress(d, 0, max_block)
    assert s is not None
    check_good(lib, [("own", s, d.tobytes())])


# ---- 4. bounds --------------------------------------------------------------------------------------------------------------------------------
def check_bounds(lib):
    # back to back, in an order that starts an item at every residue mod 4
    pool = foreign_streams(lambda: corpus.text_like(3001, 8)) + hand_after_literals() + hand_matches()[:6]
    named, seen, at = [], set(), 0
    while pool and (len(named) < 8 or len(seen) < 4):
        fresh = [c for c in pool if (at + len(c[1])) & 3 not in seen | {at & 3}]
        pick = fresh[0] if fresh else pool[0]
        pool.remove(pick)
        named.append(pick)
        seen.add(at & 3)
        at += len(pick[1])
    streams = [s for _, s, _ in named]
    wants = [w for _, _, w in named]
    offs = np.cumsum([0] + [len(s) for s in streams[:-1]])
    assert {int(o) & 3 for o in offs} == {0, 1, 2, 3}, offs
    # dst_cap exact: ok (run_streams looks at the canaries between the ranges)
    rc, res = run_streams(lib, streams, [len(w) for w in wants])
    assert rc == 0 and all(r[0] == OK and r[4] == w for r, w in zip(res, wants))
    # one byte short: reason 13, nothing past dst_cap, and what was written is a prefix of the output
    rc, res = run_streams(lib, streams, [len(w) - 1 for w in wants])
    assert rc == len(streams)
    for r, w in zip(res, wants):
        assert r[0] == DST_FULL and r[2] <= len(w) - 1 and r[4] == w[: r[2]], r[:4]
    # ... mixed with items that fit, and an item without any room
    caps = [len(w) - (k & 1) for k, w in enumerate(wants)]
    caps[2] = 0
    rc, res = run_streams(lib, streams, caps)
    for k, (r, w) in enumerate(zip(res, wants)):
        assert r[0] == (OK if caps[k] == len(w) else DST_FULL), (k, r[:4])


def check_bad_arguments(lib):
    s = zlib_raw(b"hello hello hello", 6, zlib.Z_DEFAULT_STRATEGY)
    src = np.frombuffer(s, dtype=np.uint8).copy()
    dst = np.zeros(200, dtype=np.uint8)
    n = len(src)
    assert lib.inflate_streams(src, n, dst, 200, [(0, n, 0, 100), (0, n, 100, 100)])[0] == 0
    assert lib.inflate_streams(src, n, dst, 200, [(0, n, 0, 100), (0, n, 99, 100)])[0] == -1      # destination ranges overlap
    assert lib.inflate_streams(src, n, dst, 200, [(0, n, 50, 100), (0, n, 0, 51)])[0] == -1       # ... in either order
    assert lib.inflate_streams(src, n, dst, 200, [(1, n, 0, 100)])[0] == -1                        # an item past src_size
    assert lib.inflate_streams(src, n, dst, 200, [(n + 1, 0, 0, 100)])[0] == -1
    assert lib.inflate_streams(src, n, dst, 200, [(0, n, 101, 100)])[0] == -1                      # ... past dst_size
    assert lib.inflate_streams(src, n, dst, 200, np.zeros((0, 4), dtype=np.uint64))[0] == -1       # n == 0
    assert (dst[:17].tobytes(), dst[100:117].tobytes()) == (b"hello hello hello",) * 2


# ---- 5. corruption against zlib's verdict -------------------------------------------------------------------------------------------------------
def corruption_streams():
    return [(c + "/" + name, s, d) for c in ("text", "json", "noise") for name, s, d in foreign_streams(FOREIGN[c])]


def check_flips(lib, nflips, seed):
    """One flipped bit per stream, nflips streams in one batch: reason 0 exactly where host zlib inflates the mutated stream without error and
    reaches its end — then with zlib's bytes and zlib's count of stream bytes used. -> (flips, flips that still inflate)."""
    base = corruption_streams()
    rs = np.random.RandomState(seed)
    muts, labels = [], []
    for i in range(nflips):
        name, s, d = base[i % len(base)]
        bit = int(rs.randint(0, 8 * len(s)))
        m = bytearray(s)
        m[bit >> 3] ^= 1 << (bit & 7)
        muts.append(bytes(m))
        labels.append("%s bit %d" % (name, bit))
    caps = [len(base[i % len(base)][2]) + 1024 for i in range(nflips)]
    return nflips, judge_mutants(lib, labels, muts, caps)


def judge_mutants(lib, labels, muts, caps, verbose=True):
    """The rule of check_flips on one batch of mutated streams. -> mutants that host zlib still inflates to the end (and that fit their cap)."""
    rc, res = run_streams(lib, muts, caps)
    benign = 0
    for label, m, cap, (reason, blocks, out_size, src_used, out) in zip(labels, muts, caps, res):
        ok, want, used = host_verdict(m)
        if verbose:
            print("%s: zlib %s (%d bytes) device reason %d out_size %d src_used %d" % (label, "ok" if ok else "bad", len(want), reason, out_size, src_used))
        if ok and len(want) > cap:
            assert reason == DST_FULL, (label, reason)
            continue
        assert (reason == OK) == ok, (label, reason, ok)
        if ok:
            benign += 1
            assert out == want and src_used == used, (label, out_size, len(want), src_used, used)
    return benign


def check_truncations(lib, seed):
    """Every stream cut short at 10 points (one batch: the items share the streams' bytes): reason 12, and what was written is a prefix."""
    base = corruption_streams()
    rs = np.random.RandomState(seed)
    src = np.frombuffer(b"".join(s for _, s, _ in base), dtype=np.uint8).copy()
    items, wants, soff, doff = [], [], 0, CANARY
    for name, s, d in base:
        for cut in sorted(set([0, 1, len(s) - 1] + [int(c) for c in rs.randint(2, len(s) - 1, size=7)])):
            items.append((soff, cut, doff, len(d)))
            wants.append((name, cut, d))
            doff += len(d) + CANARY
        soff += len(s)
    dst = np.full(doff, CANARY_BYTE, dtype=np.uint8)
    s_dev, d_dev = V.DeviceCopy(lib, src), V.DeviceCopy(lib, dst)
    try:
        rc, res, _ = lib.inflate_streams(s_dev.ptr, len(src), d_dev.ptr, len(dst), items)
        back = device_read(lib, d_dev, len(dst)).copy()
    finally:
        s_dev.free()
        d_dev.free()
    assert rc == len(items), rc
    check_canaries(back, items, res)
    for (name, cut, d), it, r in zip(wants, items, res):
        assert int(r["reason"]) == STREAM_END, (name, cut, r)
        assert not host_verdict(src[it[0]: it[0] + cut].tobytes())[0]
        assert back[it[2]: it[2] + int(r["out_size"])].tobytes() == d[: int(r["out_size"])], (name, cut)
    return len(items)


# ---- 6. the host API --------------------------------------------------------------------------------------------------------------------------
def check_host_api(lib, size):
    d = corpus.text_like(size, 31)
    raw = d.tobytes()
    packed = {}
    for f in (0, 1, 2):
        packed[f] = lib.memory_compress(d, f, 32768)
        assert packed[f] is not None
        assert lib.memory_decompress(packed[f], f, len(raw)) == raw, f
        assert lib.memory_decompress(packed[f], f, len(raw) + 100) == raw, f
        assert lib.memory_decompress(packed[f], f, len(raw) - 1) is None, f        # nMaxOut one byte short
        assert lib.memory_decompress(packed[f] + b"\0", f, len(raw) + 100) is None, f   # a trailing byte
    # what other tools write
    assert lib.memory_decompress(zlib.compress(raw, 9), 1, len(raw)) == raw
    buf = io.BytesIO()
    with gzip.GzipFile(filename="a.txt", mode="wb", fileobj=buf, mtime=1) as g:
        g.write(raw)
    member = buf.getvalue()
    assert member[3] & 8                                                            # FNAME
    assert lib.memory_decompress(member, 2, len(raw)) == raw
    extra = bytearray(member)                                                       # ... plus FEXTRA, FCOMMENT and FHCRC, by hand
    extra[3] |= 4 | 16 | 2
    name_end = member.index(b"\0", 10) + 1
    head = bytes(extra[:10]) + b"\x05\x00extra" + member[10:name_end] + b"a comment\0"
    head += (zlib.crc32(head) & 0xFFFF).to_bytes(2, "little")
    assert lib.memory_decompress(head + member[name_end:], 2, len(raw)) == raw
    # one flipped checksum bit, a wrong ISIZE, FDICT, a wrong framing
    for f, at in ((1, -1), (1, -4), (2, -5), (2, -8)):
        bad = bytearray(packed[f])
        bad[at] ^= 0x10
        assert lib.memory_decompress(bytes(bad), f, len(raw)) is None, (f, at)
    for at in (-1, -4):                                                             # ISIZE
        bad = bytearray(packed[2])
        bad[at] ^= 1
        assert lib.memory_decompress(bytes(bad), 2, len(raw)) is None, at
    fdict = bytearray(packed[1])
    fdict[1] |= 0x20
    fdict[1] = (fdict[1] & 0xE0) | (31 - ((fdict[0] << 8 | (fdict[1] & 0xE0)) % 31)) % 31   # (FCHECK right again: FDICT alone is the reason)
    assert (fdict[0] << 8 | fdict[1]) % 31 == 0
    assert lib.memory_decompress(bytes(fdict), 1, len(raw)) is None
    assert lib.memory_decompress(packed[2], 1, len(raw)) is None
    assert lib.memory_decompress(packed[1], 2, len(raw)) is None
    assert lib.memory_decompress(packed[0][:-1], 0, len(raw)) is None               # a stream cut short
    assert lib.memory_decompress(b"", 0, 10) is None


# ---- 7. dynamic-Huffman headers written by hand ------------------------------------------------------------------------------------------------
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]   # RFC 1951 3.2.7
CL_XBITS = {16: 2, 17: 3, 18: 7}
FIXED_LIT_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST_LENS = [5] * 32


def canonical_codes(lens):
    """RFC 1951 3.2.2: code lengths -> {symbol: (code, bits)}. An over-subscribed set gets codes too (cut to their length when written)."""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[s] = (nxt[n], n)
            nxt[n] += 1
    return out


def balanced_lens(symbols, n):
    """A complete code over `symbols` (two or more) in an alphabet of n: every length is floor(log2) or one more."""
    symbols = sorted(set(symbols))
    assert len(symbols) >= 2
    k = len(symbols).bit_length() - 1
    short = (2 << k) - len(symbols)          # this many codes of k bits, the rest of k + 1
    lens = [0] * n
    for i, s in enumerate(symbols):
        lens[s] = k if i < short else k + 1
    return lens


def ladder_lens(symbols, n):
    """Lengths 1, 2, .., m - 1, m - 1 over the m <= 16 symbols in the order given: complete, the two longest codes of up to 15 bits."""
    assert 2 <= len(symbols) <= 16
    lens = [0] * n
    for i, s in enumerate(symbols):
        lens[s] = min(i + 1, len(symbols) - 1)
    return lens


def rle_ops(lens):
    """The length sequence as operations, greedily with symbols 16, 17 and 18 (a run crosses from the literal lengths into the distance lengths
    wherever the values allow it)."""
    ops, i = [], 0
    while i < len(lens):
        run = 1
        while i + run < len(lens) and lens[i + run] == lens[i]:
            run += 1
        if lens[i] == 0 and run >= 3:
            take = min(run, 138)
            ops.append((18, take - 11) if take >= 11 else (17, take - 3))
        elif i and lens[i] == lens[i - 1] and run >= 3:
            take = min(run, 6)
            ops.append((16, take - 3))
        else:
            take = 1
            ops.append((lens[i], 0))
        i += take
    return ops


def token_symbols(length, dist):
    """-> (length symbol, distance symbol) as every compressor writes them (258 as symbol 285)."""
    return 257 + (bisect.bisect_right(LEN_BASE, length) - 1 if length < 258 else 28), bisect.bisect_right(DIST_BASE, dist) - 1


class DynWriter(BitWriter):
    """... plus dynamic-Huffman blocks: the header as given (wrong ones included), tokens in the block's own canonical codes."""

    def begin_fixed(self, final):
        BitWriter.begin_fixed(self, final)
        self.lit_codes, self.dist_codes = canonical_codes(FIXED_LIT_LENS), canonical_codes(FIXED_DIST_LENS)

    def begin_dynamic(self, final, lit_lens, dist_lens, cl_lens=None, ops=None, hlit=None, hdist=None, ncl=None):
        """ops: the length sequence as [(symbol, extra)] (extra used by 16, 17, 18), default one symbol per length. cl_lens: the 19 lengths of
        the code length code, default a complete code over the symbols of ops. hlit / hdist / ncl: the header fields' values (HLIT, HDIST) and
        the number of code length code lengths written, where they are not to follow from the lengths."""
        if ops is None:
            ops = [(n, 0) for n in list(lit_lens) + list(dist_lens)]
        if cl_lens is None:
            used = sorted({s for s, _ in ops})
            if len(used) < 2:                # (zlib takes no incomplete code length code, not even a single code)
                used.append(next(s for s in (0, 18, 17) if s not in used))
            cl_lens = balanced_lens(used, 19)
        if ncl is None:
            ncl = max([4] + [i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]])
        self.put(1 if final else 0, 1)
        self.put(2, 2)
        self.put(len(lit_lens) - 257 if hlit is None else hlit, 5)
        self.put(len(dist_lens) - 1 if hdist is None else hdist, 5)
        self.put(ncl - 4, 4)
        for i in range(ncl):
            self.put(cl_lens[CL_ORDER[i]], 3)
        cl = canonical_codes(cl_lens)
        for s, extra in ops:
            self.code(*cl[s])
            if s in CL_XBITS:
                self.put(extra, CL_XBITS[s])
        self.lit_codes, self.dist_codes = canonical_codes(lit_lens), canonical_codes(dist_lens)

    def dsym(self, s):
        self.code(*self.lit_codes[s])

    def dlits(self, data):
        for b in bytes(data):
            self.code(*self.lit_codes[b])

    def ddist_sym(self, ds):
        self.code(*self.dist_codes[ds])

    def dmatch(self, length, dist):
        ls, di = token_symbols(length, dist)
        li = ls - 257
        self.dsym(ls)
        self.put(length - LEN_BASE[li], LEN_XBITS[li])
        self.ddist_sym(di)
        self.put(dist - DIST_BASE[di], DIST_XBITS[di])

    def deob(self):
        self.dsym(256)


def _hclen(stream):
    """The number of code length code lengths a stream's first block (a dynamic one) announces."""
    return 4 + ((stream[1] | stream[2] << 8) >> 5 & 15)


def _lens_of(pairs, n):
    lens = [0] * n
    for s, bits in pairs:
        lens[s] = bits
    return lens


LADDER_LIT = [ord("a"), ord("b"), 257, ord("c"), 256, ord("d"), ord("e"), ord("f"), ord("g"), 280, ord("h"), ord("i"), ord("j"), ord("k"), ord("z"), 285]
LADDER_DIST_LOW = [14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0, 15]            # 1 bit on symbol 14 .. 14 bits on 1, 15 bits on 0 and 15
LADDER_DIST_SPREAD = [28, 26, 24, 23, 22, 21, 20, 19, 14, 12, 8, 4, 1, 0, 17, 29]    # ... 9 bits on 14, 10 on 12, 15 bits on 17 and 29
SMALL_LIT = _lens_of([(ord("a"), 2), (ord("b"), 2), (256, 2), (257, 2)], 258)        # a complete little set: a, b, end of block, length 3


def _ladder(name, dist_order, far):
    """The 15-bit literal z, the 15-bit length symbol 285 and a 15-bit distance code; every code of more than 9 / 8 bits takes zh_d_sym's walk."""
    w = DynWriter()
    dist_lens = ladder_lens(dist_order, max(dist_order) + 1)
    w.begin_dynamic(True, ladder_lens(LADDER_LIT, 286), dist_lens)
    w.dlits(b"a")
    w.dmatch(3, 1)
    w.dlits(b"bz")
    w.dmatch(258, 2)
    w.dlits((b"abcdefghijkz" * 6)[:70])
    w.dmatch(3, 70)
    w.dmatch(130, far)
    if 17 in dist_order:
        w.dmatch(3, 400)
    w.deob()
    assert {n for _, n in w.lit_codes.values()} == set(range(1, 16)) and w.lit_codes[ord("z")][1] == w.lit_codes[285][1] == 15
    assert w.dist_codes[17 if 17 in dist_order else 0][1] == 15 and w.dist_codes[14][1] in (1, 9)
    return (name, w.bytes(), 1)


def dynamic_good():
    """-> [(name, stream, blocks)]: headers no compressor writes, all of which host zlib accepts."""
    out = [_ladder("ladder_low", LADDER_DIST_LOW, 193), _ladder("ladder_spread", LADDER_DIST_SPREAD, 129)]
    w = DynWriter()                                   # a single distance code of one bit
    lit = balanced_lens([ord("a"), ord("b"), 256, 257, 285], 286)
    w.begin_dynamic(True, lit, [1], ops=rle_ops(lit + [1]))
    w.dlits(b"b")
    w.dmatch(3, 1)
    w.dlits(b"a")
    w.dsym(285)                                       # (258, 1)
    w.ddist_sym(0)
    w.deob()
    out.append(("one_distance_code", w.bytes(), 1))
    w = DynWriter()                                   # no distance code at all: HDIST 0 and that one length zero
    w.begin_dynamic(True, SMALL_LIT, [0], ops=rle_ops(SMALL_LIT + [0]))
    w.dlits(b"abba")
    w.deob()
    out.append(("no_distance_code", w.bytes(), 1))
    w = DynWriter()                                   # only the end-of-block code, one bit
    eob_only = _lens_of([(256, 1)], 257)
    w.begin_dynamic(False, eob_only, [0], ops=rle_ops(eob_only + [0]))
    w.put(0, 1)
    w.begin_fixed(True)
    w.lits(b"after the empty block")
    w.eob()
    out.append(("eob_only", w.bytes(), 2))
    w = DynWriter()                                   # 286 and 30 codes, written with 16-runs
    full_lit, full_dist = [8] * 226 + [9] * 60, [4] * 2 + [5] * 28
    ops = rle_ops(full_lit + full_dist)
    assert sum(1 for s, _ in ops if s == 16) > 50 and all(s in (4, 5, 8, 9, 16) for s, _ in ops)
    w.begin_dynamic(True, full_lit, full_dist, ops=ops)
    w.dlits(bytes(range(256)))
    w.dmatch(258, 256)
    w.dmatch(3, 1)
    w.dmatch(100, 200)
    w.deob()
    out.append(("full_alphabets", w.bytes(), 1))
    # runs that start in the literal lengths and end in the distance lengths, with distance lengths behind them that the tokens use
    lit = SMALL_LIT + [0] * 12                        # an 18-run: literal lengths 258..269 and distance lengths 0..3
    dist = [0, 0, 0, 0, 2, 2, 2, 2]
    w = DynWriter()
    w.begin_dynamic(True, lit, dist, ops=rle_ops(SMALL_LIT) + [(18, 16 - 11)] + [(2, 0)] * 4)
    w.dlits(b"abbab")
    w.dmatch(3, 5)
    w.dmatch(3, 7)
    w.deob()
    out.append(("run18_crosses", w.bytes(), 1))
    lit, dist = SMALL_LIT + [0, 0], [0, 0, 0, 1, 1]   # a 17-run: literal lengths 258, 259 and distance lengths 0..2
    w = DynWriter()
    w.begin_dynamic(True, lit, dist, ops=rle_ops(SMALL_LIT) + [(17, 5 - 3), (1, 0), (1, 0)])
    w.dlits(b"abbab")
    w.dmatch(3, 4)
    w.dmatch(3, 5)
    w.deob()
    out.append(("run17_crosses", w.bytes(), 1))
    lit = _lens_of([(ord("a"), 3), (256, 3), (257, 2), (258, 2), (259, 2)], 260)   # a 16-run: literal lengths 258, 259 and distance lengths 0, 1
    dist = [2, 2, 1]
    w = DynWriter()
    w.begin_dynamic(True, lit, dist, ops=rle_ops(lit[:258]) + [(16, 4 - 3), (1, 0)])
    w.dlits(b"aaa")
    w.dmatch(3, 1)
    w.dmatch(4, 2)
    w.dmatch(5, 3)
    w.deob()
    out.append(("run16_crosses", w.bytes(), 1))
    # HCLEN. Four code length code lengths reach the symbols 16, 17, 18 and 0 only: every length is zero, the end-of-block code is missing, and no
    # such block is accepted (dynamic_bad has it). The least that can be accepted is five (symbol 8: 256 codes of eight bits, no distance code).
    lit = [8] * 255 + [0, 8]
    w = DynWriter()
    w.begin_dynamic(True, lit, [0], cl_lens=_lens_of([(16, 2), (0, 2), (8, 1)], 19), ops=rle_ops(lit + [0]))
    w.dlits(b"five lengths")
    w.deob()
    out.append(("hclen_5", w.bytes(), 1))
    assert _hclen(out[-1][1]) == 5
    w = DynWriter()                                   # (the HCLEN field at the value 4: eight lengths, symbols 8, 7, 9 and 6 behind the first four)
    lit = _lens_of([(ord("a"), 6), (ord("b"), 6)] + [(s, 6) for s in range(200, 230)] + [(256, 7), (257, 7)] + [(s, 7) for s in range(260, 262)] + [(s, 8) for s in range(100, 200)] + [(s, 8) for s in range(230, 246)] + [(s, 9) for s in range(8)], 262)
    w.begin_dynamic(True, lit, [0], cl_lens=_lens_of([(0, 1), (6, 3), (7, 3), (8, 3), (9, 4), (16, 5), (17, 6), (18, 6)], 19), ops=rle_ops(lit + [0]), ncl=8)
    w.dlits(b"ab\x00\x07\x64ba")
    w.deob()
    out.append(("hclen_8", w.bytes(), 1))
    assert _hclen(out[-1][1]) == 8
    w = DynWriter()                                   # nineteen: the last of them, symbol 15's, zero
    w.begin_dynamic(True, SMALL_LIT, [1, 1], ops=rle_ops(SMALL_LIT + [1, 1]), ncl=19)
    w.dlits(b"ab")
    w.dmatch(3, 2)
    w.dmatch(3, 1)
    w.deob()
    out.append(("hclen_19", w.bytes(), 1))
    assert _hclen(out[-1][1]) == 19
    w = DynWriter()                                   # length 258 as symbol 284 with all five extra bits set (BitWriter.match writes 285)
    w.begin_fixed(True)
    w.lits(b"xy")
    w.sym(284)
    w.put(31, 5)
    w.dist_sym(1)
    w.eob()
    out.append(("len258_as_284", w.bytes(), 1))
    named = []
    for name, s, blocks in out:
        name, s, want = _with_zlib(name, s)
        named.append((name, s, want, blocks))
    by = {name: want for name, _, want, _ in named}
    assert by["one_distance_code"] == b"b" * 4 + b"a" * 259 and by["no_distance_code"] == b"abba" and by["eob_only"] == b"after the empty block"
    assert by["len258_as_284"] == b"xy" * 130 and by["hclen_5"] == b"five lengths" and by["hclen_19"] == b"ababaaaa"
    assert by["full_alphabets"][:514] == bytes(range(256)) + bytes(range(256)) + b"\x00\x01" and len(by["full_alphabets"]) == 256 + 258 + 3 + 100
    assert by["run16_crosses"] == b"a" * 15 and by["run17_crosses"] == b"abbab" + b"bba" + b"abb" and by["run18_crosses"] == b"abbab" + b"abb" + b"bba"
    assert len(by["ladder_low"]) == 1 + 3 + 2 + 258 + 70 + 3 + 130 and len(by["ladder_spread"]) == len(by["ladder_low"]) + 3
    return named


def _small_block(w, lit=None, dist=None, tokens=True, tail=4, **kw):
    """A little dynamic block around one wrong thing, and `tail` bytes behind it (so that no verdict is the stream's end)."""
    lit = SMALL_LIT if lit is None else lit
    dist = [1, 1] if dist is None else dist
    if "ops" not in kw:
        kw["ops"] = rle_ops(list(lit) + list(dist))
    w.begin_dynamic(True, lit, dist, **kw)
    if tokens:
        w.dlits(b"ab")
        w.deob()
    for _ in range(tail):
        w.put(0x55, 8)
    return w.bytes()


def dynamic_bad():
    """-> [(name, stream, reason, output written before the failure or None)]: host zlib rejects every one of them with an error."""
    out = []
    for v in (30, 31):
        out.append(("hlit_%d" % v, _small_block(DynWriter(), hlit=v), HEADER, None))
        out.append(("hdist_%d" % v, _small_block(DynWriter(), hdist=v), HEADER, None))
    c = ord("c")
    out.append(("lit_over", _small_block(DynWriter(), lit=_lens_of([(97, 2), (98, 2), (c, 2), (256, 2), (257, 2)], 258)), CODELENS, None))
    out.append(("lit_incomplete", _small_block(DynWriter(), lit=_lens_of([(97, 2), (98, 2), (256, 2)], 258)), CODELENS, None))
    out.append(("dist_over", _small_block(DynWriter(), dist=[1, 1, 1]), CODELENS, None))
    out.append(("dist_incomplete", _small_block(DynWriter(), dist=[2, 2, 2]), CODELENS, None))
    out.append(("dist_single_two_bit", _small_block(DynWriter(), dist=[2]), CODELENS, None))
    out.append(("no_eob", _small_block(DynWriter(), lit=_lens_of([(97, 2), (98, 2), (c, 2), (257, 2)], 258), tokens=False), CODELENS, None))
    out.append(("cl_single", _small_block(DynWriter(), cl_lens=_lens_of([(0, 1)], 19), ops=[(0, 0)] * 20, tokens=False), CODELENS, None))
    out.append(("cl_over", _small_block(DynWriter(), cl_lens=_lens_of([(0, 1), (2, 1), (18, 1)], 19), ops=[(0, 0)] * 20, tokens=False), CODELENS, None))
    out.append(("cl_incomplete", _small_block(DynWriter(), cl_lens=_lens_of([(0, 2), (2, 2), (18, 2)], 19), ops=[(0, 0)] * 20, tokens=False), CODELENS, None))
    out.append(("cl_all_zero", _small_block(DynWriter(), cl_lens=[0] * 19, ops=[], tokens=False, tail=40), CODELENS, None))   # (zlib reads 260 lengths of one bit first)
    out.append(("hclen_4", _small_block(DynWriter(), cl_lens=_lens_of([(0, 1), (18, 1)], 19), ops=[(18, 127), (18, 260 - 138 - 11)], ncl=4, tokens=False), CODELENS, None))
    out.append(("repeat_first", _small_block(DynWriter(), ops=[(16, 0)] + rle_ops(SMALL_LIT[3:] + [1, 1]), tokens=False), CODELENS, None))
    out.append(("run_past_end", _small_block(DynWriter(), ops=rle_ops(SMALL_LIT + [1]) + [(17, 0)], tokens=False), CODELENS, None))
    w = DynWriter()                                   # the one-bit distance set addressed with the bit that is no code
    w.begin_dynamic(True, SMALL_LIT, [1], ops=rle_ops(SMALL_LIT + [1]))
    w.dlits(b"ab")
    w.dsym(257)
    w.put(1, 1)
    w.put(0x55555555, 32)
    out.append(("one_distance_code_other_bit", w.bytes(), DISTANCE, b"ab"))
    w = DynWriter()                                   # a length symbol where there are no distance codes
    w.begin_dynamic(True, SMALL_LIT, [0], ops=rle_ops(SMALL_LIT + [0]))
    w.dlits(b"ba")
    w.dsym(257)
    w.put(0x55555555, 32)
    out.append(("length_without_distance_codes", w.bytes(), DISTANCE, b"ba"))
    w = DynWriter()                                   # the end-of-block-only set addressed with the bit that is no code
    w.begin_fixed(False)
    w.lits(b"abc")
    w.eob()
    eob_only = _lens_of([(256, 1)], 257)
    w.begin_dynamic(True, eob_only, [0], ops=rle_ops(eob_only + [0]))
    w.put(1, 1)
    w.put(0x55555555, 32)
    out.append(("eob_only_other_bit", w.bytes(), SYMBOL, b"abc"))
    for name, s, _, _ in out:
        d = zlib.decompressobj(-15)
        try:
            d.decompress(s)
        except zlib.error:
            continue
        raise AssertionError("host zlib takes " + name)
    return out


def check_dynamic_good(lib):
    named = dynamic_good()
    res = check_good(lib, [c[:3] for c in named])
    for (name, _, _, blocks), r in zip(named, res):
        assert r[1] == blocks, (name, r[1], blocks)
    return len(named)


def check_dynamic_bad(lib):
    bad = dynamic_bad()
    rc, res = run_streams(lib, [c[1] for c in bad], [600] * len(bad))
    assert rc == len(bad)
    for (name, s, want, written), (reason, blocks, out_size, src_used, out) in zip(bad, res):
        assert reason == want, (name, reason, want)
        if written is not None:
            assert out == written, (name, out, written)
    return len(bad)


def check_dynamic_cuts(lib):
    """Every accept case cut at every byte, one batch: the copies lie back to back, so what follows an item's end is the stream's own next byte
    (never the zeros a cut-off stream reads as). Reason 12, a prefix of the output, and host zlib does not reach the end either."""
    streams, sizes, caps, wants = [], [], [], []
    for name, s, want, _ in dynamic_good():
        for cut in range(len(s)):
            streams.append(s)
            sizes.append(cut)
            caps.append(len(want))
            wants.append((name, cut, want))
    rc, res = run_streams(lib, streams, caps, src_sizes=sizes)
    assert rc == len(streams)
    for (name, cut, want), s, (reason, blocks, out_size, src_used, out) in zip(wants, streams, res):
        assert reason == STREAM_END, (name, cut, reason)
        assert out == want[:out_size] and src_used <= cut, (name, cut, out_size, src_used)
        assert not host_verdict(s[:cut])[0], (name, cut)
    return len(streams)


def check_dynamic_flips(lib):
    """Every bit of every accept case of at most 60 bytes flipped, one batch, dst_cap 1200: check_flips' rule. -> (mutants, those zlib accepts)."""
    muts, labels = [], []
    for name, s, want, _ in dynamic_good():
        if len(s) > 60:
            continue
        for bit in range(8 * len(s)):
            m = bytearray(s)
            m[bit >> 3] ^= 1 << (bit & 7)
            muts.append(bytes(m))
            labels.append("%s bit %d" % (name, bit))
    benign = judge_mutants(lib, labels, muts, [1200] * len(muts), verbose=False)
    assert benign > 0, "no mutant is accepted by zlib: accepted mutants were not compared at all"
    return len(muts), benign


# ---- 8. seeded token streams aimed at `synced`, the literal stretches and the stored copy ---------------------------------------------------------
class ListWriter(DynWriter):
    """DynWriter that keeps (value, bits) and packs them in one numpy pass: for streams of many thousands of tokens."""

    def __init__(self):
        self.v, self.k, self.total = [], [], 0

    def put(self, value, nbits):
        self.v.append(value)
        self.k.append(nbits)
        self.total += nbits

    @staticmethod
    def tables(lit_lens, dist_lens):
        rev = lambda codes, n: ([int(format(codes[s][0], "0%db" % codes[s][1])[::-1], 2) if s in codes else None for s in range(n)], [codes[s][1] if s in codes else 0 for s in range(n)])
        return rev(canonical_codes(lit_lens), len(lit_lens)) + rev(canonical_codes(dist_lens), len(dist_lens))

    def set_codes(self, lit_lens, dist_lens):
        self.lit_rev, self.lit_bits, self.dist_rev, self.dist_bits = self.tables(lit_lens, dist_lens)

    def begin_fixed(self, final):
        BitWriter.begin_fixed(self, final)
        self.lit_rev, self.lit_bits, self.dist_rev, self.dist_bits = FIXED_TABLES

    def begin_dynamic(self, final, lit_lens, dist_lens, **kw):
        DynWriter.begin_dynamic(self, final, lit_lens, dist_lens, **kw)
        self.set_codes(lit_lens, dist_lens)

    def dsym(self, s):
        self.put(self.lit_rev[s], self.lit_bits[s])

    def dlits(self, data):
        self.v.extend(map(self.lit_rev.__getitem__, data))
        self.k.extend(map(self.lit_bits.__getitem__, data))
        self.total += sum(map(self.lit_bits.__getitem__, data))

    def ddist_sym(self, ds):
        self.put(self.dist_rev[ds], self.dist_bits[ds])

    def stored(self, data, final):
        self.put(1 if final else 0, 1)
        self.put(0, 2)
        self.put(0, -self.total & 7)
        self.put(len(data), 16)
        self.put(len(data) ^ 0xFFFF, 16)
        self.v.extend(data)
        self.k.extend([8] * len(data))
        self.total += 8 * len(data)

    def bytes(self):
        v, k = np.array(self.v, dtype=np.uint32), np.array(self.k, dtype=np.int64)
        start = np.cumsum(k) - k
        within = np.arange(int(k.sum()), dtype=np.int64) - np.repeat(start, k)
        return np.packbits(((np.repeat(v, k) >> within.astype(np.uint32)) & 1).astype(np.uint8), bitorder="little").tobytes()


FIXED_TABLES = ListWriter.tables(FIXED_LIT_LENS, FIXED_DIST_LENS)
DIST_CLASSES = ("1_2_3", "63_64_65", "to_start", "to_previous_match", "to_previous_match_pm1", "into_last_stored", "uniform")
LEN_CLASSES = (3, 4, 63, 64, 65, 66, 128, 129, 257, 258, "random")
HAZARDS = ("chain", "straddles_synced", "ends_at_synced", "starts_at_synced", "below_synced", "stored_then_match")


def random_token_streams(seed, nstreams, ntokens):
    """-> ([(name, stream, blocks)], stats): blocks = [("stored", bytes) | ("fixed" | "dynamic", [bytes | (len, dist)])], stats = how often every
    distance class, length class and hazard was drawn. The generator follows the kernel's `synced` (the output position at the last match whose
    source reached past it) to aim matches below, at and across it."""
    rs = random.Random(seed)
    stats = {c: 0 for c in DIST_CLASSES + LEN_CLASSES + HAZARDS}
    ri = lambda lo, hi: lo + int(rs.random() * (hi - lo + 1))

    def draw_len():
        c = LEN_CLASSES[ri(0, len(LEN_CLASSES) - 1)]
        stats[c] += 1
        return ri(3, 258) if c == "random" else c

    out = []
    for k in range(nstreams):
        blocks, p, q, synced, stored_at, left = [], 0, 0, 0, None, ntokens   # q: output position at the previous match; stored_at: (lo, hi) of the last stored block

        def match(length, dist):
            nonlocal p, q, synced
            assert 1 <= dist <= min(p, 32768) and 3 <= length <= 258
            src_hi = p - dist + min(dist, length)
            stats["below_synced"] += src_hi < synced
            stats["ends_at_synced"] += src_hi == synced
            stats["starts_at_synced"] += p - dist == synced
            stats["straddles_synced"] += p - dist < synced < src_hi
            if src_hi > synced:
                synced = p
            q = p
            p += length
            return (length, dist)

        def draw_match():
            length = draw_len()
            for _ in range(50):
                c = DIST_CLASSES[ri(0, len(DIST_CLASSES) - 1)]
                if c == "1_2_3":
                    dist = ri(1, 3)
                elif c == "63_64_65":
                    dist = ri(63, 65)
                elif c == "to_start":
                    dist = p
                elif c == "to_previous_match":
                    dist = p - q
                elif c == "to_previous_match_pm1":
                    dist = p - q + (1, -1)[ri(0, 1)]
                elif c == "into_last_stored":
                    dist = p - ri(stored_at[0], stored_at[1] - 1) if stored_at and stored_at[1] > stored_at[0] else 0
                else:
                    dist = ri(1, min(p, 32768))
                if 1 <= dist <= min(p, 32768):
                    stats[c] += 1
                    return match(length, dist)
            return match(length, 1)

        while left > 0 or not blocks:
            kind = ("stored", "fixed", "dynamic", "dynamic")[ri(0, 3)]
            if kind == "stored":
                n = (0, 1, 63, 64, 65, ri(0, 300), ri(0, 300))[ri(0, 6)]
                blocks.append(("stored", rs.randbytes(n)))
                stored_at = (p, p + n)
                p += n
                left -= 1
                continue
            tokens = []
            if stored_at and stored_at[1] == p and stored_at[1] > stored_at[0] and ri(0, 1):   # a match into the stored block right in front
                stats["stored_then_match"] += 1
                tokens.append(match(draw_len(), p - ri(stored_at[0], stored_at[1] - 1)))
            for _ in range(ri(1, 60)):
                what = ri(0, 9) if p else 0
                if what < 4:
                    n = (1, 1, 1, 63, 64, 65, ri(1, 20), ri(1, 20), ri(1, 20), ri(1, 150))[ri(0, 9)]
                    tokens.append(rs.randbytes(n) if kind == "fixed" else bytes(rs.choices(b"etaoin shr", k=n)))
                    p += n
                elif what < 8:
                    tokens.append(draw_match())
                elif what == 8:                          # a chain: every match sources from the bytes of the match in front of it
                    stats["chain"] += 1
                    length = draw_len()
                    tokens.append(match(length, ri(1, min(p, 300))))
                    for _ in range(ri(2, 6)):
                        nxt = draw_len()
                        tokens.append(match(nxt, ri(1, length)))
                        length = nxt
                elif synced:                             # a match whose source reaches across `synced`, ends at it or starts at it
                    length, how = draw_len(), ri(0, 3)
                    below = (ri(1, min(length - 1, synced)), length, 0)[max(how - 1, 0)]
                    if below <= synced and 1 <= p - synced + below <= 32768:
                        tokens.append(match(length, p - synced + below))
                left -= 1
            blocks.append((kind, tokens))
        w = ListWriter()
        for i, (kind, body) in enumerate(blocks):
            final = i == len(blocks) - 1
            if kind == "stored":
                w.stored(body, final)
                continue
            if kind == "fixed":
                w.begin_fixed(final)
            else:
                pairs = [token_symbols(*t) for t in body if isinstance(t, tuple)]
                lit_used = sorted({256} | {b for t in body if isinstance(t, bytes) for b in t} | {a for a, _ in pairs})
                dist_used = sorted({b for _, b in pairs})
                shape = lambda used, n: ladder_lens(rs.sample(used, len(used)), n) if len(used) <= 16 and ri(0, 1) else balanced_lens(used, n)
                lit_lens = shape(lit_used, lit_used[-1] + 1 if lit_used[-1] > 256 else 257) if len(lit_used) > 1 else _lens_of([(256, 1)], 257)
                dist_lens = shape(dist_used, dist_used[-1] + 1) if len(dist_used) > 1 else _lens_of([(d, 1) for d in dist_used], (dist_used or [0])[-1] + 1)
                w.begin_dynamic(final, lit_lens, dist_lens, ops=rle_ops(lit_lens + dist_lens) if ri(0, 3) else None)
            for t in body:
                if isinstance(t, bytes):
                    w.dlits(t)
                else:
                    w.dmatch(*t)
            w.deob()
        out.append(("fuzz%d" % k, w.bytes(), blocks))
    return out, stats


def replay(blocks):
    """What the token list says, in plain Python."""
    out = bytearray()
    for kind, body in blocks:
        for t in ([body] if kind == "stored" else body):
            if isinstance(t, bytes):
                out += t
                continue
            length, dist = t
            piece = bytes(out[len(out) - dist: len(out) - dist + length])
            out += (piece * (length // len(piece) + 1))[:length]
    return bytes(out)


def check_token_fuzz(lib, seed, nstreams, ntokens, copies=1, made=None):
    """One batch of nstreams generated streams, every one `copies` times (each copy an item with a destination of its own: the batch keeps that
    many more waves busy than streams had to be generated). made: what random_token_streams gave another process. -> made."""
    streams, stats = made or random_token_streams(seed, nstreams, ntokens)
    empty = [c for c, n in stats.items() if n == 0]
    assert not empty, "never drawn with seed %d: %s" % (seed, empty)
    named = [(name, s, replay(blocks)) for name, s, blocks in streams]
    for name, s, want in named:                     # host zlib against the replay first, then the device
        assert host_verdict(s) == (True, want, len(s)), name
    res = check_good(lib, named * copies)
    for (name, _, blocks), r in zip(streams * copies, res):
        assert r[1] == len(blocks), (name, r[1], len(blocks))
    return streams, stats


def check_token_fuzz_strided(lib_path, is_emulator, made, copies, tmp_path):
    """The same batch in a process of its own with ZULTRA_HIP_GRID_CAP=8."""
    tests = os.path.dirname(os.path.abspath(__file__))
    handed = os.path.join(str(tmp_path), "token_streams.pickle")
    with open(handed, "wb") as f:
        pickle.dump(made, f)
    code = ("import pickle, sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import inflate_cases as I\nfrom zultra_amd._ffi import Lib\nL = Lib(%r)\nL.is_emulator = %r\n"
            "I.check_token_fuzz(L, 0, 0, 0, %d, pickle.load(open(%r, 'rb')))\nprint('strided ok')\n") % (os.path.dirname(tests), tests, lib_path, bool(is_emulator), copies, handed)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ZULTRA_HIP_GRID_CAP="8"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "strided ok" in r.stdout, r.stdout + r.stderr


# ---- 9. buffers that start inside a dword -----------------------------------------------------------------------------------------------------------
def check_unaligned(lib):
    """The source pointer 1, 2 and 3 bytes into a dword (0xFF in front of the buffer and behind it: nothing outside it may count), one call per
    stream, so that every stream meets both edge dwords; then the destination pointer likewise. Every result is that of the aligned run."""
    named = hand_matches()[:8] + [c[:3] for c in dynamic_good()]
    aligned = check_good(lib, named)
    for lead in (1, 2, 3):
        for (name, s, want), ref in zip(named, aligned):
            src = V.DeviceCopy(lib, np.frombuffer(b"\xff" * lead + s + b"\xff" * 8, dtype=np.uint8).copy())
            dst = V.DeviceCopy(lib, np.full(len(want) + 2 * CANARY, CANARY_BYTE, dtype=np.uint8))
            try:
                items = [(0, len(s), CANARY, len(want))]
                rc, res, _ = lib.inflate_streams(src.ptr + lead, len(s), dst.ptr, len(want) + 2 * CANARY, items)
                back = device_read(lib, dst, len(want) + 2 * CANARY).copy()
            finally:
                src.free()
                dst.free()
            check_canaries(back, items, res)
            r = res[0]
            got = (int(r["reason"]), int(r["blocks"]), int(r["out_size"]), int(r["src_used"]), back[CANARY: CANARY + int(r["out_size"])].tobytes())
            assert rc == 0 and got == ref, (name, lead, got[:4], ref[:4])
    src_arr = np.frombuffer(b"".join(s for _, s, _ in named), dtype=np.uint8).copy()
    for lead in (1, 2, 3):
        items, soff, doff = [], 0, CANARY
        for name, s, want in named:
            items.append((soff, len(s), doff, len(want)))
            soff += len(s)
            doff += len(want) + CANARY
        src, dst = V.DeviceCopy(lib, src_arr), V.DeviceCopy(lib, np.full(lead + doff, CANARY_BYTE, dtype=np.uint8))
        try:
            rc, res, _ = lib.inflate_streams(src.ptr, len(src_arr), dst.ptr + lead, doff, items)
            back = device_read(lib, dst, lead + doff).copy()
        finally:
            src.free()
            dst.free()
        assert rc == 0 and (back[:lead] == CANARY_BYTE).all(), (lead, rc)
        check_canaries(back[lead:], items, res)
        for (name, _, _), it, r, ref in zip(named, items, res, aligned):
            got = (int(r["reason"]), int(r["blocks"]), int(r["out_size"]), int(r["src_used"]), back[lead + it[2]: lead + it[2] + int(r["out_size"])].tobytes())
            assert got == ref, (name, lead, got[:4], ref[:4])


# ---- 10. stored blocks by hand ----------------------------------------------------------------------------------------------------------------------
def check_stored_edges(lib):
    rc, res = run_streams(lib, [bytes.fromhex("010000ffff")], [0])           # an empty stream into no room at all
    assert rc == 0 and res[0] == (OK, 1, 0, 5, b""), res[0]
    named = []
    w = BitWriter()
    w.stored(corpus.noise(65535, 5).tobytes(), True)
    named.append(_with_zlib("stored_65535", w.bytes()))
    for nine in range(8):      # a fixed block of 10 + 8 * literals + `nine` bits in front: the stored header starts at every bit of a byte, the pad is 0..7 bits
        w = BitWriter()
        w.begin_fixed(False)
        w.lits(b"pad" + bytes([200 + i for i in range(nine)]))
        w.eob()
        assert w.n == (2 + nine) & 7
        at = w.n
        w.stored(_pattern(70, nine), True)
        named.append(_with_zlib("stored_at_bit_%d" % at, w.bytes()))
    w = BitWriter()            # an empty stored block between two fixed blocks whose literals lie in one 64-byte stretch
    w.begin_fixed(False)
    w.lits(b"ten bytes,")
    w.eob()
    w.stored(b"", False)
    w.begin_fixed(True)
    w.lits(b" ten more.")
    w.eob()
    named.append(_with_zlib("empty_stored_between", w.bytes()))
    res = check_good(lib, named)
    assert res[-1][1] == 3 and res[-1][4] == b"ten bytes, ten more." and all(r[1] == 2 for r in res[1:9])
    w = BitWriter()            # a stored block one byte larger than the room left: nothing of it is written
    w.begin_fixed(False)
    w.lits(b"abcde")
    w.eob()
    w.stored(_pattern(20), True)
    assert host_verdict(w.bytes())[0]
    rc, res = run_streams(lib, [w.bytes()], [5 + 19])
    assert rc == 1 and res[0][0] == DST_FULL and res[0][2] == 5 and res[0][4] == b"abcde", res[0]
    w = BitWriter()
    w.stored(b"wrong NLEN", True)
    bad = bytearray(w.bytes())
    bad[3] ^= 0x40
    assert not host_verdict(bytes(bad))[0]
    rc, res = run_streams(lib, [bytes(bad)], [100])
    assert rc == 1 and res[0][0] == STORED_LEN and res[0][2] == 0, res[0]
