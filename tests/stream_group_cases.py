"""Shared by tests/test_stream_groups_emu.py (CPU emulator build) and tests/test_stream_groups_gpu.py (product library on the MI355X): the cases and the
checks of the GROUPED assembly — a batch that holds several deflate streams, each a run of consecutive max-blocks: zultra_hip_frame_streams and
zultra_hip_zip_streams (zh_stitch_scan_streams and zh_fold_streams of zultra_amd/csrc/zh_streams.h in front of the writers of zh_frame.h and zh_zip.h),
zultra_memory_compress_streams, zultra_memory_compress_zip_streams and the tool's -a with -b. The expected bytes never come from the code under test:
the reference's memory_compress (the `checker` fixture) for whole members and raw streams, binascii.crc32 / zlib.adler32, want_archive of
tests/zip_cases.py fed the reference's streams; Python's gzip, zlib and zipfile decode what comes out. Every case uses the smallest max-block, 32768."""
import binascii
import ctypes as C
import gzip
import os
import subprocess
import zlib

import numpy as np

import frame_member_cases as M
import inflate_file_cases as F
import verify_cases as V
import zip_cases as Z
from inflate_cases import device_read

MB = 32768
RAW, ZLIB, GZIP, BGZF = M.RAW, M.ZLIB, M.GZIP, M.BGZF
HEAD, TAIL = M.HEAD, M.TAIL
u8 = M.u8


def long_text(n, seed):
    """n bytes of text, n above what F.text has: windows of it one behind the other."""
    return b"".join(F.text(min(150000, n - at), seed + at // 150000) for at in range(0, n, 150000))


def describe(parts, mb=MB):
    """The inputs one behind the other as streams of max-blocks of mb bytes -> (data, blocks [(win_off, prev, n)], stream_first)."""
    blocks, first, at = [], [], 0
    for p in parts:
        first.append(len(blocks))
        for k in range(0, len(p), mb):
            prev = min(32768, k)
            blocks.append((at + k - prev, prev, min(mb, len(p) - k)))
        at += len(p)
    return b"".join(parts), blocks, first


def compress(ctx, parts, mb=MB):
    data, blocks, first = describe(parts, mb)
    ctx.compress_blocks(u8(data), blocks)
    return blocks, first


def grouped(ctx, checker, parts, first, framing, mb=MB):
    """frame_streams over the context's last batch (= parts as streams) held to the reference member by member, members[] and total_bytes to the bytes.
    -> (the buffer's bytes, members)."""
    rc, mem, total = ctx.frame_streams(first, framing)
    assert rc == 0, (framing, rc, ctx.lib.L.zultra_hip_last_error(ctx.h))
    buf = ctx.stream_read(total).tobytes()
    at = 0
    for i, (p, m) in enumerate(zip(parts, mem)):
        want = M.want_member(checker, p, framing, mb)
        assert (int(m["off"]), int(m["size"]), int(m["flags"])) == (at, len(want), 0), (framing, i, m, len(want))
        assert buf[at: at + len(want)] == want, (framing, i, len(p))
        assert int(m["check"]) == M.check_value(p, framing), (framing, i)
        at += len(want)
    assert at == total == len(buf), (framing, at, total)
    return buf, mem


class Batch:
    """A context and the batch it has compressed: `parts` as streams of max-blocks of 32768 bytes. Shared by the checks of a test module — the emulator
    compresses a kilobyte per second, so a batch is compressed once."""

    def __init__(self, lib, parts, spare_blocks=0):
        self.lib, self.parts = lib, parts
        self.data, self.blocks, self.first = describe(parts)
        self.ctx = lib.context(MB, len(self.blocks) + spare_blocks)
        self.ctx.compress_blocks(u8(self.data), self.blocks)

    def close(self):
        self.ctx.close()


# ---- 1: parity per framing ------------------------------------------------------------------------------------------------------------------------
def parity_parts():
    return [F.text(1, 1),
            F.text(32769, 2),                                           # the last block is 1 byte
            F.text(100, 3),
            F.text(65536, 4),                                           # the last block is full
            F.text(MB, 5) + F.noise(MB, 6) + F.text(MB, 7),             # a stored max-block in the middle: its LEN aligns from a carried phase
            F.text(8192, 8),
            F.noise(65537, 9),                                          # stored throughout
            F.text(3 * MB + 5000, 10)]


def small_parts():
    """What the emulator takes for the checks that share one batch: a stream of two max-blocks between two of one."""
    return [F.text(500, 20), F.text(MB + 300, 21), F.text(2000, 22)]


def check_parity(batch, checker):
    ctx, parts, first = batch.ctx, batch.parts, batch.first
    for framing in (RAW, ZLIB, GZIP):
        buf, mem = grouped(ctx, checker, parts, first, framing)
        v = ctx.verify()
        assert v["rc"] == 0 and v["verified_bytes"] == sum(len(p) for p in parts), (framing, v)
        if framing == GZIP:
            assert gzip.decompress(buf) == b"".join(parts)
        if framing == ZLIB:
            assert b"".join(zlib.decompress(buf[int(m["off"]): int(m["off"] + m["size"])]) for m in mem) == b"".join(parts)
    return len(parts)


# ---- 2: every carried phase ------------------------------------------------------------------------------------------------------------------------
def carried_phases(batch):
    """The bit phase at every interior max-block boundary of every stream of the batch, from the HOST stitcher (zultra_hip_stitch with out == NULL) over
    that stream's descriptors, max-block by max-block."""
    from zultra_amd._ffi import BitState
    ctx, blocks, first = batch.ctx, batch.blocks, batch.first
    raw = u8(batch.data)
    subs, p, cnt = ctx.subblocks()
    size = C.c_size_t()
    payload = ctx.lib.L.zultra_hip_payload(ctx.h, C.byref(size))
    offs = (C.c_uint64 * len(blocks))(*[o + pv for o, pv, _ in blocks])
    start = {}
    for k, s in enumerate(subs):
        start.setdefault(s.block, k)
    start[len(blocks)] = cnt
    phases = []
    bounds = list(first) + [len(blocks)]
    for s in range(len(first)):
        st = BitState(0, 0)
        for b in range(bounds[s], bounds[s + 1] - 1):     # (behind the last block there is no boundary to carry over)
            k0, k1 = start[b], start[b + 1]
            w = ctx.lib.L.zultra_hip_stitch(C.byref(st), C.byref(p[k0]), k1 - k0, payload, raw.ctypes.data, offs, MB, -1, None, 0)
            assert w != C.c_size_t(-1).value
            phases.append(int(st.nacc))
    return phases


PHASE_SEEDS = (19, 23)   # (phases 2 and 7, which the parity batch's nine boundaries — 3 6 4 0 0 0 6 1 5 — miss)


def phase_parts():
    """Two-block streams of text: next to the parity batch's boundaries, theirs carry every phase 0 .. 7 (the seeds were chosen by their phase; a set that
    misses one fails the test that asks for all eight)."""
    return [F.text(MB + 40, seed) for seed in PHASE_SEEDS]


# ---- 3: degenerate groupings ----------------------------------------------------------------------------------------------------------------------
def check_single_blocks(lib, checker):
    """Every stream a single max-block: frame_members byte for byte, and the plain form stitch_files'."""
    parts = [F.text(n, 300 + i) for i, n in enumerate((1, 63, 4096, 100))] + [F.noise(500, 310), F.text(3000, 311)]
    ctx = lib.context(MB, len(parts))
    try:
        M.compress(ctx, parts)
        every = list(range(len(parts)))
        file_off = [int(v) for v in ctx.stitch_files()]
        plain = ctx.stream_read(file_off[-1]).tobytes()
        for framing in (RAW, ZLIB, GZIP):
            rc, mem, total = ctx.frame_members(framing)
            assert rc == 0
            want = ctx.stream_read(total).tobytes()
            rc, smem, stotal = ctx.frame_streams(every, framing)
            assert rc == 0 and stotal == total and ctx.stream_read(total).tobytes() == want, framing
            assert smem.tobytes() == mem.tobytes(), framing
            assert ctx.verify()["rc"] == 0
            if framing == RAW:
                assert want == plain and [int(m["off"]) for m in smem] == file_off[:-1]
    finally:
        ctx.close()


def check_one_stream(lib, checker, size):
    """One stream over the whole batch: the plain form is stitch_device's from phase 0 with the last block final, padded to a byte."""
    one = F.text(size, 320)
    batch = Batch(lib, [one])
    try:
        ctx = batch.ctx
        assert batch.first == [0] and len(batch.blocks) == (size + MB - 1) // MB >= 2
        end_bit, _ = ctx.stitch_device(len(batch.blocks) - 1)
        want = ctx.stream_read((end_bit + 7) // 8).tobytes()
        rc, mem, total = ctx.frame_streams([0], RAW)
        assert rc == 0 and total == len(want) and ctx.stream_read(total).tobytes() == want
        assert want == M.want_member(checker, one, RAW, MB)
    finally:
        batch.close()


# ---- 4: the device scan equals the host planner -----------------------------------------------------------------------------------------------------
def check_scan_equals_planner(batch, stored=True):
    ctx, first = batch.ctx, batch.first
    for framing in (RAW, ZLIB, GZIP):
        rc, mem, total = ctx.frame_streams(first, framing)
        assert rc == 0
        got = ctx.stitch_items()
        rc, want, file_off, end_bit = ctx.plan_streams(first, framing)
        assert rc == 0 and len(got) == len(want) >= len(batch.blocks)
        for k, (g, w) in enumerate(zip(got, want)):
            assert tuple(int(g[f]) for f in ("dst_bit", "stored", "is_final")) == tuple(int(w[f]) for f in ("dst_bit", "stored", "is_final")), (framing, k, g, w)
        assert [int(m["off"]) + HEAD[framing] for m in mem] == [int(v) for v in file_off[:-1]] and int(file_off[-1]) - HEAD[framing] == total == end_bit // 8
        assert sum(int(g["is_final"]) for g in got) == len(first) and (not stored or any(int(g["stored"]) for g in got))


# ---- 5: more blocks than scan threads ---------------------------------------------------------------------------------------------------------------
def many_parts(n, multi):
    """n small inputs of 30 .. 90 bytes, and streams of 2 and 3 max-blocks put in at the part indices of `multi` {index: blocks}."""
    parts = M.small_inputs(n)
    for k, (at, nb) in enumerate(sorted(multi.items())):
        parts.insert(at, F.text((nb - 1) * MB + 77 + k, 400 + k))
    return parts


def check_many(lib, checker, n, multi, chunk):
    """chunk: max-blocks per thread of the scan at this batch size (2 for 1025 .. 2048): the long streams start at odd and at even block indices, so that
    they start, end and straddle chunk boundaries. With ZULTRA_HIP_GRID_CAP in the environment a wave of zh_fold_streams folds several streams."""
    checker = checker or M.make_checker()
    parts = many_parts(n, multi)
    data, blocks, first = describe(parts)
    assert (len(blocks) + 1023) // 1024 == chunk
    starts = {first[i] % 2 for i, p in enumerate(parts) if len(p) > MB}
    assert chunk == 1 or starts == {0, 1}, starts
    ctx = lib.context(MB, len(blocks))
    try:
        ctx.compress_blocks(u8(data), blocks)
        for framing in (GZIP, RAW):
            buf, mem = grouped(ctx, checker, parts, first, framing)
            assert ctx.verify()["rc"] == 0
        names = [b"f%05d" % i for i in range(len(parts))]
        zipped(ctx, checker, parts, first, names)
    finally:
        ctx.close()
    return len(blocks)


MANY_GPU = (1090, {3: 2, 200: 3, 401: 2, 702: 3, 1000: 3})   # (part indices; the block indices come out odd and even: check_many asserts it)


# ---- 6: the fold across lanes -----------------------------------------------------------------------------------------------------------------------
def check_fold(lib, nblocks_long):
    """One stream of nblocks_long max-blocks — above 64 a lane of zh_fold_streams folds two — next to a stream of 2: checksums and sizes against Python's."""
    parts = [long_text(nblocks_long * MB, 500), F.text(MB + 1, 501)]
    ctx = lib.context(MB, nblocks_long + 2)
    try:
        blocks, first = compress(ctx, parts)
        assert first == [0, nblocks_long]
        for framing, fn in ((GZIP, binascii.crc32), (ZLIB, zlib.adler32)):
            rc, mem, total = ctx.frame_streams(first, framing)
            assert rc == 0
            assert [int(m["check"]) for m in mem] == [fn(p) for p in parts], framing
            buf = ctx.stream_read(total).tobytes()
            if framing == GZIP:
                assert gzip.decompress(buf) == b"".join(parts)
            else:
                assert [zlib.decompress(buf[int(m["off"]): int(m["off"] + m["size"])]) for m in mem] == parts
            assert ctx.verify()["rc"] == 0
    finally:
        ctx.close()


# ---- 7: flipped bits ----------------------------------------------------------------------------------------------------------------------------------
def check_flipped_bits(batch, checker):
    ctx, parts, first = batch.ctx, batch.parts, batch.first
    bounds = list(first) + [len(batch.blocks)]
    s = max(range(len(first)), key=lambda i: bounds[i + 1] - bounds[i])       # the stream of the most max-blocks
    nb = bounds[s + 1] - bounds[s]
    assert nb >= 2
    inner = bounds[s] + (nb - 1) // 2                                         # a block that does not end it: the middle one of three
    buf, mem = grouped(ctx, checker, parts, first, GZIP)
    items = ctx.stitch_items()
    subs = ctx.subblocks()[0]
    assert ctx.verify()["rc"] == 0

    def flipped(at, bit):
        ctx.stream_write(bytes([buf[at] ^ (1 << bit)]), at)
        v = ctx.verify()
        ctx.stream_write(bytes([buf[at]]), at)
        return v

    k = next(k for k, sb in enumerate(subs) if sb.block == inner)
    v = flipped(int(items[k]["dst_bit"]) // 8 + 30, 4)
    assert v["rc"] == 1 and v["block"] == inner, v
    # the last byte of the stream's deflate data (its bit 0 belongs to the stream, however few of its bits do)
    v = flipped(int(mem[s]["off"] + mem[s]["size"]) - TAIL[GZIP] - 1, 0)
    assert v["rc"] == 1 and v["block"] == bounds[s + 1] - 1, v
    # BFINAL set on the first sub-block of a block that does not end its stream
    assert int(items[k]["is_final"]) == 0
    bit = int(items[k]["dst_bit"])
    v = flipped(bit // 8, bit % 8)
    assert v["rc"] == 1 and v["reason"] == 11 and v["block"] == inner, v
    assert ctx.verify()["rc"] == 0


# ---- 8: refusals --------------------------------------------------------------------------------------------------------------------------------------
def _marked(lib, ctx, first, names, data_len):
    """Marks in both buffers, and the check that a refused call has left them alone."""
    rc, ent, local, central, central_at = ctx.zip_streams(first, names)
    assert rc == 0
    mark_s, mark_z = bytes((i * 7 + 3) & 255 for i in range(data_len + 256)), bytes((i * 11 + 5) & 255 for i in range(central_at + central))
    ctx.stream_write(mark_s)
    Z._zip_write(lib, ctx, mark_z)

    def refused(what, first_, rc_want=-1, framing=GZIP):
        assert ctx.frame_streams(first_, framing)[0] == rc_want, what
        if framing != BGZF:
            assert ctx.zip_streams(first_, names[:max(len(first_), 1)])[0] == rc_want, what
        assert ctx.stream_read(len(mark_s)).tobytes() == mark_s, "a refused call has written the stream buffer: " + what
        assert ctx.zip_read(len(mark_z)).tobytes() == mark_z, "a refused call has written the zip buffer: " + what
    return refused


def check_refused_groupings(batch):
    """On a batch of streams of 1, 2 and 1 max-blocks (small_parts)."""
    ctx, first = batch.ctx, batch.first
    assert first == [0, 1, 3] and len(batch.blocks) == 4
    refused = _marked(batch.lib, ctx, first, ["a", "bb", "ccc"], len(batch.data))
    refused("stream_first[0] != 0", [1, 3])
    refused("a non-increasing index", [0, 3, 3])
    refused("an index past the batch", [0, 1, 4])
    refused("a stream's first block with history", [0, 1, 2])
    refused("BGZF", first, framing=BGZF)
    refused("nstreams == 0", [])
    rc, mem, total = ctx.frame_streams(first, GZIP)
    assert rc == 0 and gzip.decompress(ctx.stream_read(total).tobytes()) == batch.data


def check_refused_descriptors(lib, checker):
    """Max-blocks that do not continue their predecessor; before any batch; and a stored-only stream, held to the reference's verdict: -2 where it fails
    with ZULTRA_ERROR_DST (no such input is known: two max-blocks of noise fit the reference's buffer, and then the member must be the reference's)."""
    parts = small_parts()
    data, blocks, first = describe(parts)
    ctx = lib.context(MB, 4)
    try:
        assert ctx.frame_streams([0], GZIP)[0] == -1                                  # before any batch
        ctx.compress_blocks(u8(data), blocks)
        refused = _marked(lib, ctx, first, ["a", "bb", "ccc"], len(data))
        ok = blocks[2]
        for what, bad in (("a continuation with a wrong prev", (ok[0] + 100, ok[1] - 100, ok[2])), ("a non-contiguous window", (ok[0] + 1, ok[1], ok[2] - 1))):
            ctx.compress_blocks(u8(data), blocks[:2] + [bad] + blocks[3:])
            refused(what, first)
        short = [blocks[0], (blocks[1][0], 0, 20000), (blocks[1][0], 20000, len(parts[1]) - 20000), blocks[3]]
        ctx.compress_blocks(u8(data), short)
        refused("a short predecessor", first)
    finally:
        ctx.close()
    # stored-only streams: where the reference fails with ZULTRA_ERROR_DST the call returns -2, where it does not the member is the reference's
    noise = F.noise(2 * MB, 710)
    batch = Batch(lib, [noise])
    try:
        want = checker.memory_compress(u8(noise), GZIP, MB)
        rc, mem, total = batch.ctx.frame_streams([0], GZIP)
        assert rc == (-2 if want is None else 0), (rc, want is None)
        if want is not None:
            assert batch.ctx.stream_read(total).tobytes() == want
    finally:
        batch.close()


# ---- 9: behind and in front of the other assemblies -------------------------------------------------------------------------------------------------
def check_next_to_the_others(batch, checker):
    ctx, parts, first, blocks = batch.ctx, batch.parts, batch.first, batch.blocks
    names = ["n%d" % i for i in range(len(parts))]
    # what each old call gives alone
    alone_files = [int(v) for v in ctx.stitch_files()]
    alone_files_bytes = ctx.stream_read(alone_files[-1]).tobytes()
    alone_end, alone_phase = ctx.stitch_device(len(blocks) - 1)
    alone_stream = ctx.stream_read((alone_end + 7) // 8).tobytes()
    ctx.lib.L.zultra_hip_stitch_phase_table.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]

    def phase_table():
        ends, mask = (C.c_uint64 * 8)(), C.c_uint32()
        assert ctx.lib.L.zultra_hip_stitch_phase_table(ctx.h, ends, C.byref(mask)) == 0
        return list(ends), mask.value
    alone_table = phase_table()
    assert ctx.frame_members(GZIP)[0] == -1
    olds = (("stitch_files", lambda: ([int(v) for v in ctx.stitch_files()], ctx.stream_read(alone_files[-1]).tobytes()) == (alone_files, alone_files_bytes)),
            ("frame_members", lambda: ctx.frame_members(GZIP)[0] == -1 and ctx.frame_members(RAW)[0] == -1),
            ("stitch_device", lambda: ctx.stitch_device(len(blocks) - 1) == (alone_end, alone_phase) and ctx.stream_read(len(alone_stream)).tobytes() == alone_stream),
            ("stitch_phase_table", lambda: phase_table() == alone_table),
            ("zip_members", lambda: ctx.zip_members(["b%d" % i for i in range(len(blocks))])[0] == -1))
    for what, old in olds:
        grouped(ctx, checker, parts, first, GZIP)
        assert old(), "behind a grouped assembly: " + what
        grouped(ctx, checker, parts, first, ZLIB)              # ... and a grouped assembly behind it
        v = ctx.verify()
        assert v["rc"] == 0 and v["verified_bytes"] == sum(len(p) for p in parts), what
    # zip_streams behind framed streams assembles the plain form itself; behind the plain form it gathers from what it finds
    grouped(ctx, checker, parts, first, GZIP)
    zipped(ctx, checker, parts, first, names)
    assert ctx.verify()["rc"] == 0
    plain, _ = grouped(ctx, checker, parts, first, RAW)
    zipped(ctx, checker, parts, first, names)
    assert ctx.stream_read(len(plain)).tobytes() == plain and ctx.verify()["rc"] == 0


# ---- 10: ZIP --------------------------------------------------------------------------------------------------------------------------------------------
def zipped(ctx, checker, parts, first, names, base_off=0, dos=0):
    """zip_streams over the context's last batch — the non-empty parts as streams — held to the expected local and central part (zip_cases.want_parts
    with the reference's streams at max-blocks of 32768) and entries[] to both. -> (entries, local part, central part)."""
    names = Z.enc(names)
    es = None
    if any(len(p) == 0 for p in parts):
        es, k = [], 0
        for p in parts:
            es.append(k if len(p) else Z.EMPTY)
            k += 1 if len(p) else 0
    rc, ent, local, central, central_at = ctx.zip_streams(first, names, es, base_off, dos)
    assert rc == 0, (rc, ctx.lib.L.zultra_hip_last_error(ctx.h))
    want_local, want_central, offs, streams = Z.want_parts(checker, parts, names, MB, base_off, dos or Z.DOS_DEFAULT)
    assert (local, central) == (len(want_local), len(want_central)) and central_at % 16 == 0 and central_at >= local, (local, central, central_at)
    for i, e in enumerate(ent):
        got = tuple(int(e[k]) for k in ("local_off", "comp_size", "size", "crc32", "name_len"))
        assert got == (offs[i], len(streams[i]), len(parts[i]), binascii.crc32(parts[i]) if len(parts[i]) else 0, len(names[i])), (i, got)
    got_local, got_central = ctx.zip_read(local).tobytes(), ctx.zip_read(central, central_at).tobytes()
    assert got_local == want_local and got_central == want_central
    return ent, got_local, got_central


def zip_parts():
    """The non-empty entries of the archive of check_zip, in order."""
    return [F.text(5000, 900), F.text(70000, 901), F.text(3 * MB + 1, 902), F.noise(40000, 903)]


def check_zip(batch, checker, empty_at=(1, 4)):
    """The batch's streams and, at the entry indices empty_at, an empty file and a directory."""
    lib, ctx, first = batch.lib, batch.ctx, batch.first
    parts = list(batch.parts)
    names = ["e%d/file %d.txt" % (i % 2, i) for i in range(len(parts))]
    for at, name in zip(empty_at, ("empty.bin", "dir/")):
        parts.insert(at, b"")
        names.insert(at, name)
    sizes = [len(p) for p in parts]
    dst_off = [0] + [int(v) for v in np.cumsum(sizes)]
    plain = b"".join(parts)
    base_off = 1000003
    d = V.DeviceCopy(lib, np.zeros(len(plain) + 16, dtype=np.uint8))
    try:
        ent, local, central = zipped(ctx, checker, parts, first, names)
        buf = local + central + Z.want_end_records(len(parts), len(local), len(central))
        assert buf == Z.want_archive(checker, parts, Z.enc(names), MB)
        z = Z.check_zipfile(buf, Z.enc(names), parts)
        assert z.getinfo("dir/").is_dir()
        out, info, n = lib.memory_decompress_zip(buf, len(plain), len(parts))
        assert out == plain and n == len(parts) and [int(i["nStatus"]) for i in info] == [0] * len(parts)
        # inflate the entries where they stand in the zip buffer
        ent, local, central = zipped(ctx, checker, parts, first, names, base_off=base_off, dos=0x5b54a825)
        items = [(int(e["local_off"]) - base_off + 30 + int(e["name_len"]), int(e["comp_size"]), dst_off[i], sizes[i]) for i, e in enumerate(ent) if sizes[i]]
        rc, results, _ = lib.inflate_streams(ctx.zip_ptr()[0], len(local), d.ptr, len(plain), items)
        assert rc == 0 and [int(r["reason"]) for r in results] == [0] * len(items), (rc, results)
        assert device_read(lib, d, len(plain)).tobytes() == plain
        v = ctx.verify()
        assert v["rc"] == 0 and v["verified_bytes"] == len(plain), v
    finally:
        d.free()


# ---- 11: the host API -----------------------------------------------------------------------------------------------------------------------------------
def api_parts(huge):
    return [F.text(100, 1000), F.text(9000, 1001), F.text(40000, 1002), F.text(100000, 1003)] + ([long_text(2097153, 1004)] if huge else [])


def check_api(lib, checker, max_block, parts, framings=(GZIP, RAW, ZLIB), short_caps=True):
    """max_block as the caller passes it (0: the default, 1 MiB). short_caps: also with a byte of room too few (each such call compresses again)."""
    checker = checker or M.make_checker()
    mb = max_block or 1048576
    lead = b"\xee" * 3
    data = lead + b"".join(parts)
    offs = [len(lead) + int(v) for v in np.concatenate([[0], np.cumsum([len(p) for p in parts])[:-1]])]
    inputs = [(o, len(p)) for o, p in zip(offs, parts)]
    for flags in framings:
        lib.set_verify(1)
        try:
            v0 = lib.verified_bytes()
            out, off = lib.memory_compress_streams(data, inputs, flags, max_block)
            assert out is not None and lib.verified_bytes() - v0 == sum(len(p) for p in parts)
        finally:
            lib.set_verify(0)
        assert off[0] == 0 and off[-1] == len(out) and len(off) == len(parts) + 1
        for i, p in enumerate(parts):
            assert out[off[i]: off[i + 1]] == M.want_member(checker, p, flags, mb), (flags, i)
        if flags == GZIP:
            assert gzip.decompress(out) == b"".join(parts)
            assert not short_caps or lib.memory_compress_streams(data, inputs, flags, max_block, cap=len(out) - 1) == (None, None)      # one byte short
    assert lib.memory_compress_streams(data, inputs[:2] + [(5, 0)], GZIP, max_block) == (None, None)                   # an empty input
    assert lib.memory_compress_streams(data, [(len(data) - 10, 11)], GZIP, max_block) == (None, None)                  # past the end
    assert lib.memory_compress_streams(data, inputs, 3, max_block) == (None, None)                                     # two framings
    names = ["n%d" % i for i in range(len(parts))] + ["empty", "d/"]
    zparts = parts + [b"", b""]
    lib.set_verify(1)
    try:
        got = lib.memory_compress_zip_streams(data, inputs + [(0, 0), (0, 0)], names, 0, max_block)
    finally:
        lib.set_verify(0)
    want = Z.want_archive(checker, zparts, Z.enc(names), mb)
    assert got is not None and got == want, (None if got is None else len(got), len(want))
    Z.check_zipfile(got, Z.enc(names), zparts)
    assert not short_caps or lib.memory_compress_zip_streams(data, inputs + [(0, 0), (0, 0)], names, 0, max_block, cap=len(got) - 1) is None
    return len(parts)


def check_api_small_batches(lib, checker):
    """With ZULTRA_HIP_BATCH_BLOCKS=4 in the environment (a process of its own: the knob is read per call, the cached contexts are per process): the streams
    of 1, 1, 2 and 4 max-blocks are spread over several batches; an input of five is refused."""
    assert os.environ.get("ZULTRA_HIP_BATCH_BLOCKS") == "4"
    n = check_api(lib, checker, MB, api_parts(False))
    five = F.text(4 * MB + 1, 1010)
    assert lib.memory_compress_streams(five, [(0, len(five))], GZIP, MB) == (None, None)
    assert lib.memory_compress_zip_streams(five, [(0, len(five))], ["five"], 0, MB) is None
    return n


# ---- 12: the tool -----------------------------------------------------------------------------------------------------------------------------------------
def check_cli(cli, lib, tmp_path, checker):
    parts = [F.text(5000, 1100), long_text(2097153, 1101)]
    names = ["one.txt", "huge"]
    for name, p in zip(names, parts):
        with open(os.path.join(str(tmp_path), name), "wb") as f:
            f.write(p)
    r = subprocess.run([cli, "-c", "-v", "-a", "out.zip", "-b", "32768"] + names, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0 and "verified %d bytes" % sum(len(p) for p in parts) in r.stdout, r.stdout + r.stderr
    got = open(os.path.join(str(tmp_path), "out.zip"), "rb").read()
    assert got == lib.memory_compress_zip_streams(b"".join(parts), [(0, 5000), (5000, 2097153)], names, 0, MB)
    Z.check_zipfile(got, Z.enc(names), parts)
    r = subprocess.run([cli, "-x", "-a", "out.zip", "back"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    for name, p in zip(names, parts):
        assert open(os.path.join(str(tmp_path), "back", name), "rb").read() == p, name
    r = subprocess.run([cli, "-c", "-v", "-a", "out2.zip"] + names, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode != 0 and "huge" in r.stderr, r.stdout + r.stderr


# ---- 13: the stand-alone program ------------------------------------------------------------------------------------------------------------------------
def sanitizer_case(checker, parts):
    """The case file of tests/emu/stream_groups_main.cpp: u64 n, the data; u64 blocks, their (win_off, prev, n) as u64 each; u64 streams, their first blocks
    as u64; then per framing 0, 1, 2: u64 size and the bytes the stream buffer must hold (the reference's members back to back)."""
    u64 = lambda v: int(v).to_bytes(8, "little")
    data, blocks, first = describe(parts)
    out = u64(len(data)) + data + u64(len(blocks)) + b"".join(u64(a) + u64(b) + u64(c) for a, b, c in blocks) + u64(len(first)) + b"".join(u64(v) for v in first)
    for framing in (RAW, ZLIB, GZIP):
        want = b"".join(M.want_member(checker, p, framing, MB) for p in parts)
        out += u64(len(want)) + want
    return out
