"""Shared by tests/test_inflate_emu.py (CPU emulator build) and tests/test_inflate_gpu.py (product library on the MI355X): the streams, the batch
runner and the checks of zultra_hip_inflate_streams (zultra_amd/csrc/zh_inflate_out.h) and zultra_memory_decompress. The yardstick is Python's zlib
on the host. Both files run the same cases; the emulator takes the smaller sizes."""
import ctypes as C
import gzip
import io
import os
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

    def code(self, value, nbits):          # Huffman codes go in from their most significant bit
        for k in range(nbits - 1, -1, -1):
            self.put((value >> k) & 1, 1)

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
    rc, res = run_streams(lib, muts, caps)
    benign = 0
    for label, m, cap, (reason, blocks, out_size, src_used, out) in zip(labels, muts, caps, res):
        ok, want, used = host_verdict(m)
        print("%s: zlib %s (%d bytes) device reason %d out_size %d src_used %d" % (label, "ok" if ok else "bad", len(want), reason, out_size, src_used))
        if ok and len(want) > cap:
            assert reason == DST_FULL, (label, reason)
            continue
        assert (reason == OK) == ok, (label, reason, ok)
        if ok:
            benign += 1
            assert out == want and src_used == used, (label, out_size, len(want), src_used, used)
    return nflips, benign


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
