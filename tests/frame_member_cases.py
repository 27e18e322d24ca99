"""Shared by tests/test_frame_members_emu.py (CPU emulator build) and tests/test_frame_members_gpu.py (product library on the MI355X): the cases and
the checks of framed members written on the device — zultra_hip_frame_members (zh_stitch_scan with head and tail, zh_frame_clear and zh_frame_members
of zultra_amd/csrc/zh_frame.h), zultra_memory_compress_bgzf, zultra_memory_compress_batch and the tool's -f bgzf. The expected bytes never come from
the code under test: the reference's memory_compress (the `checker` fixture) for whole gzip / zlib members and for the raw stream inside a BGZF
member, binascii.crc32, and the bgzf() / EOF_MARKER helpers of tests/inflate_file_cases.py for BGZF's header and trailer; Python's gzip and zlib
decode what comes out."""
import binascii
import gzip
import os
import subprocess
import zlib

import numpy as np

import inflate_file_cases as F
import verify_cases as V
from inflate_cases import device_read

RAW, ZLIB, GZIP, BGZF = 0, 1, 2, 4
HEAD = {RAW: 0, ZLIB: 2, GZIP: 10, BGZF: 18}
TAIL = {RAW: 0, ZLIB: 4, GZIP: 8, BGZF: 8}
_WANT = {}


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def make_checker():
    """What conftest's `checker` fixture hands out, for a check that runs in a process of its own (run_child)."""
    import zlibs
    return zlibs.RefStages() if zlibs.have_ref() else zlibs.Oracle()


def want_member(checker, data, framing, max_block):
    """The member the reference writes for `data` (BGZF: its raw stream between the header and trailer the format defines), computed once per case."""
    key = (bytes(data), framing, max_block)
    if key not in _WANT:
        if framing == BGZF:
            _WANT[key] = F.bgzf(data, raw=want_member(checker, data, RAW, max_block))
        else:
            _WANT[key] = checker.memory_compress(u8(data), framing, max_block)
    return _WANT[key]


def check_value(data, framing):
    return 0 if framing == RAW else zlib.adler32(data) if framing == ZLIB else binascii.crc32(data)


def compress(ctx, parts):
    sizes = [len(p) for p in parts]
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    ctx.compress_blocks(u8(b"".join(parts)), [(int(o), 0, n) for o, n in zip(offs, sizes)])


def framed(ctx, checker, parts, framing, max_block, eof=False):
    """frame_members over the context's last batch (= parts) held to the reference member by member, and members[] / total_bytes to the bytes.
    -> (the buffer's bytes, members)."""
    rc, mem, total = ctx.frame_members(framing, eof)
    assert rc == 0, (framing, rc)
    buf = ctx.stream_read(total).tobytes()
    at = 0
    for i, (p, m) in enumerate(zip(parts, mem)):
        want = want_member(checker, p, framing, max_block)
        assert (int(m["off"]), int(m["size"]), int(m["flags"])) == (at, len(want), 0), (framing, i, m, len(want))
        assert buf[at: at + len(want)] == want, (framing, i, len(p))
        assert int(m["check"]) == check_value(p, framing), (framing, i)
        at += len(want)
    if eof and framing == BGZF:
        assert buf[at:] == F.EOF_MARKER
        at += len(F.EOF_MARKER)
    assert at == total == len(buf), (framing, at, total)
    return buf, mem


# ---- 1: parity per framing ------------------------------------------------------------------------------------------------------------------------
def parity_blocks():
    return [F.text(1, 1), F.text(2, 2), F.text(100, 3), F.text(4095, 4), F.text(8191, 5), F.text(8192, 6),
            F.text(16000, 7) + F.noise(12000, 8) + F.text(12000, 9),        # several sub-blocks, a stored one among them
            F.text(65280, 10), F.noise(65280, 11), F.text(65536, 12)]       # ..., stored, BGZF's largest ISIZE


def check_parity(lib, checker):
    parts = parity_blocks()
    ctx = lib.context(65536, len(parts))
    try:
        compress(ctx, parts)
        subs = ctx.subblocks()[0]
        mixed = [s for s in subs if s.block == 6]
        assert len(mixed) >= 3, len(mixed)
        for framing in (ZLIB, GZIP, BGZF):
            buf, mem = framed(ctx, checker, parts, framing, 65536, eof=framing == BGZF)
            assert {int(m["off"]) & 3 for m in mem} == {0, 1, 2, 3}, (framing, [int(m["off"]) & 3 for m in mem])
            assert ctx.verify()["rc"] == 0, framing
            if framing == GZIP:
                assert gzip.decompress(buf) == b"".join(parts)
        # the stream of the 40000-byte case holds a stored sub-block: its noise lies in the member byte for byte
        assert F.noise(12000, 8)[5000:6000] in want_member(checker, parts[6], GZIP, 65536)
    finally:
        ctx.close()
    return len(parts)


# ---- 2: more blocks than the scan has threads ---------------------------------------------------------------------------------------------------
def small_inputs(n):
    return [F.text(30 + (i * 37) % 61, 200 + i) for i in range(n)]


def check_many_small(lib, checker, n):
    """n inputs of 30 .. 90 bytes in a files context: above 1024 a thread of zh_stitch_scan walks a chunk of several max-blocks, and with
    ZULTRA_HIP_GRID_CAP in the environment a lane of zh_frame_members frames several members."""
    checker = checker or make_checker()
    parts = small_inputs(n)
    sizes = [len(p) for p in parts]
    assert min(sizes) == 30 and max(sizes) == 90
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    ctx = lib.files_context(8191, n)
    try:
        ctx.compress_files(u8(b"".join(parts)), offsets, sizes)
        for framing in (GZIP, BGZF, ZLIB):
            buf, mem = framed(ctx, checker, parts, framing, 32768, eof=True)
            assert ctx.verify()["rc"] == 0
        assert b"".join(zlib.decompress(buf[int(m["off"]): int(m["off"] + m["size"])]) for m in mem) == b"".join(parts)
    finally:
        ctx.close()
    return n


# ---- 3: both kinds of context; the plain files layout before and after ----------------------------------------------------------------------------
def check_both_contexts(lib, checker):
    parts = [F.text(n, 300 + i) for i, n in enumerate((1, 63, 64, 65, 4096, 8191, 100))] + [F.noise(500, 310)]
    sizes = [len(p) for p in parts]
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    raw = b"".join(want_member(checker, p, RAW, 32768) for p in parts)
    raw_off = [0] + list(np.cumsum([len(want_member(checker, p, RAW, 32768)) for p in parts]))
    seen = {}
    for kind in ("files", "blocks"):
        ctx = lib.files_context(8191, len(parts)) if kind == "files" else lib.context(32768, len(parts))
        try:
            if kind == "files":
                before = ctx.compress_files(u8(b"".join(parts)), offsets, sizes)     # (its assembly comes with the batch, from the captured graph)
            else:
                compress(ctx, parts)
                before = ctx.stitch_files()
            assert [int(v) for v in before] == raw_off and ctx.stream_read(len(raw)).tobytes() == raw, kind
            for framing in (RAW, ZLIB, GZIP, BGZF):
                buf, mem = framed(ctx, checker, parts, framing, 32768, eof=True)
                assert seen.setdefault(framing, buf) == buf, (kind, framing)
            after = ctx.stitch_files()
            assert [int(v) for v in after] == raw_off and ctx.stream_read(len(raw)).tobytes() == raw, kind
            assert ctx.verify()["rc"] == 0
        finally:
            ctx.close()


# ---- 4: round trip on the device ------------------------------------------------------------------------------------------------------------------
def check_round_trip(lib, checker):
    parts = [F.text(3000, 400), F.text(1, 401), F.noise(700, 402), F.text(20000, 403) + F.noise(9000, 404), F.text(65280, 405), F.text(77, 406)]
    sizes = [len(p) for p in parts]
    dst_off = [0] + [int(v) for v in np.cumsum(sizes)]
    plain = b"".join(parts)
    ctx = lib.context(65280, len(parts))
    d = V.DeviceCopy(lib, np.zeros(len(plain) + 16, dtype=np.uint8))
    try:
        compress(ctx, parts)
        for framing in (BGZF, GZIP, ZLIB):
            buf, mem = framed(ctx, checker, parts, framing, 65280, eof=True)
            items = [(int(m["off"]), int(m["size"]), dst_off[i], sizes[i]) for i, m in enumerate(mem)]
            if framing == BGZF:
                marker = (len(buf) - 28, 28, len(plain), 0)
                rc, res, got, _ = lib.index_members(ctx.stream_ptr(), len(buf), len(parts) + 1)
                assert rc == 0 and res.stop == 0 and [tuple(int(v) for v in r) for r in got] == items + [marker]
                rc, res, results, _ = lib.inflate_file(ctx.stream_ptr(), len(buf), d.ptr, len(plain), len(parts) + 1)
                assert rc == 0 and res.members == len(parts) + 1 and res.out_size == len(plain)
            else:
                rc, results, _ = lib.inflate_members(ctx.stream_ptr(), len(buf), d.ptr, len(plain), None, 0, framing, items)
                assert rc == 0
            assert [int(r["reason"]) for r in results] == [0] * len(results), framing
            assert device_read(lib, d, len(plain)).tobytes() == plain, framing
            assert [int(r["check"]) for r in results][:len(parts)] == [int(m["check"]) for m in mem]
            if framing == ZLIB:
                assert b"".join(zlib.decompress(buf[o: o + n]) for o, n, _, _ in items) == plain
            else:
                assert gzip.decompress(buf) == plain
            v = ctx.verify()
            assert v["rc"] == 0 and v["verified_bytes"] == len(plain), v
            # one flipped bit inside member 0's deflate body
            at = int(mem[0]["off"]) + HEAD[framing] + 40
            ctx.stream_write(bytes([buf[at] ^ 0x10]), at)
            v = ctx.verify()
            assert v["rc"] == 1 and v["block"] == 0, v
    finally:
        d.free()
        ctx.close()


# ---- 5: refusals ------------------------------------------------------------------------------------------------------------------------------------
def check_refusals(lib):
    ctx = lib.context(131072, 2)
    try:
        assert ctx.frame_members(GZIP, blocks=1)[0] == -1                         # before any batch
        big = F.noise(131072, 500)
        compress(ctx, [big])
        mark = bytes((i * 7 + 3) & 255 for i in range(131072 + 64))               # (what the members and the marker would take, and more)
        ctx.stream_write(mark)
        rc, mem, total = ctx.frame_members(BGZF, True)
        assert rc == -3 and int(mem[0]["flags"]) & 1, (rc, mem)
        assert ctx.stream_read(len(mark)).tobytes() == mark, "a refused call has written"
        for framing in (3, 5, 8):
            assert ctx.frame_members(framing)[0] == -1, framing
        buf, mem = framed_gzip_of_big(ctx, big)
        # a block with history is no member
        ctx.compress_blocks(u8(big), [(0, 0, 40000), (40000 - 32768, 32768, 50000)])
        assert ctx.frame_members(GZIP)[0] == -1
        assert ctx.frame_members(RAW)[0] == -1
    finally:
        ctx.close()


def check_oversize_member(lib):
    """The other way to -3: an input of 65536 bytes, which ISIZE can hold, whose member cannot be a BGZF member — noise is stored as pieces of 65535 and 1
    bytes at the least (10 bytes of headers), 18 + 65546 + 8 bytes or more in all. Next to it a member that fits: only the large one is flagged, nothing is written."""
    parts = [F.text(500, 510), F.noise(65536, 511)]
    ctx = lib.context(65536, 2)
    try:
        compress(ctx, parts)
        mark = bytes((i * 5 + 1) & 255 for i in range(66400))
        ctx.stream_write(mark)
        rc, mem, total = ctx.frame_members(BGZF, True)
        assert rc == -3 and [int(m["flags"]) for m in mem] == [0, 1] and 65536 < int(mem[1]["size"]) <= 18 + 65547 + 8, (rc, mem)
        assert ctx.stream_read(len(mark)).tobytes() == mark, "a refused call has written"
        rc, mem, total = ctx.frame_members(GZIP)
        assert rc == 0 and gzip.decompress(ctx.stream_read(total).tobytes()) == b"".join(parts)
    finally:
        ctx.close()


def check_batch_after_framing(lib, checker):
    """A context that has framed a batch compresses the next one: the plain layout the batch brings with it (a files context's captured graph, the stitch
    armed with a batch of max-blocks) verifies, and so does the framed one behind it — the gap of the last framing is not remembered."""
    first = [F.text(n, 900 + i) for i, n in enumerate((700, 64, 3000))]
    second = [F.text(n, 910 + i) for i, n in enumerate((100, 2500, 33, 4000))]
    ctx = lib.files_context(8191, 4)
    try:
        for parts, framing in ((first, GZIP), (second, BGZF), (first, ZLIB)):
            sizes = [len(p) for p in parts]
            offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
            file_off = ctx.compress_files(u8(b"".join(parts)), offsets, sizes)
            v = ctx.verify()
            assert v["rc"] == 0 and v["verified_bytes"] == sum(sizes), (framing, v)
            assert ctx.stream_read(int(file_off[-1])).tobytes() == b"".join(want_member(checker, p, RAW, 32768) for p in parts)
            framed(ctx, checker, parts, framing, 32768, eof=True)
            assert ctx.verify()["rc"] == 0
    finally:
        ctx.close()
    ctx = lib.context(32768, 4)
    try:
        compress(ctx, first)
        framed(ctx, checker, first, GZIP, 32768)
        ctx.stitch_with_batch(len(second) - 1)
        compress(ctx, second)
        ctx.stitch_device(len(second) - 1)
        assert ctx.verify()["rc"] == 0
    finally:
        ctx.close()


def framed_gzip_of_big(ctx, big):
    """(the same batch is a sound gzip member: only BGZF has a size limit)"""
    rc, mem, total = ctx.frame_members(GZIP)
    assert rc == 0 and int(mem[0]["flags"]) == 0
    buf = ctx.stream_read(total).tobytes()
    assert gzip.decompress(buf) == big and int(mem[0]["check"]) == binascii.crc32(big)
    return buf, mem


# ---- 6: the host API --------------------------------------------------------------------------------------------------------------------------------
def bgzf_file(checker, data, block):
    max_block = max(block, 32768)
    return b"".join(want_member(checker, data[at: at + block], BGZF, max_block) for at in range(0, len(data), block)) + F.EOF_MARKER


def mixed_input():
    return F.text(90000, 600) + F.noise(30000, 601) + F.text(80000, 602)


def check_bgzf_api(lib, checker):
    d = mixed_input()
    assert len(d) == 200000
    cases = [(d, 0), (d, 4096), (d[:3 * 4096], 4096), (d[:1], 0), (b"", 0)]
    for data, block in cases:
        want = bgzf_file(checker, data, block or 65280)
        got = lib.memory_compress_bgzf(data, block)
        assert got == want, (len(data), block, None if got is None else len(got), len(want))
        assert gzip.decompress(got) == data
        assert lib.memory_decompress_members(got, len(data)) == (data, len(F.walk(want)[0]))
        assert lib.memory_bound_bgzf(len(data), block) >= len(got)
        assert lib.memory_compress_bgzf(data, block, cap=len(got) - 1) is None
    assert lib.memory_compress_bgzf(b"", 0) == F.EOF_MARKER and len(F.EOF_MARKER) == 28
    assert lib.memory_compress_bgzf(d[:100], 65281) is None                       # above bgzip's block size
    return len(cases)


def check_batch_api(lib, checker):
    parts = [F.text(100, 700), F.text(9000, 701), F.text(8191, 702), F.text(8192, 703), F.noise(50, 704), F.text(1, 705), F.text(20000, 706), F.text(5000, 707)]
    lead = b"\xee" * 3
    data = lead + b"".join(parts)
    offs = [len(lead) + int(v) for v in np.concatenate([[0], np.cumsum([len(p) for p in parts])[:-1]])]
    inputs = [(o, len(p)) for o, p in zip(offs, parts)]
    max_block = 32768          # (the call's context of max-blocks is as large as its largest input)
    for flags in (RAW, ZLIB, GZIP):
        lib.set_verify(1)
        try:
            v0 = lib.verified_bytes()
            out, off = lib.memory_compress_batch(data, inputs, flags)
            assert lib.verified_bytes() - v0 == sum(len(p) for p in parts)
        finally:
            lib.set_verify(0)
        assert out is not None and off[0] == 0 and off[-1] == len(out)
        for i, p in enumerate(parts):
            assert out[off[i]: off[i + 1]] == want_member(checker, p, flags, max_block), (flags, i)
        rc, outs = lib.memory_decompress_batch(out, [(off[i], off[i + 1] - off[i]) for i in range(len(parts))], flags, [len(p) for p in parts])
        assert rc == 0 and outs == parts, flags
        if flags == GZIP:
            assert lib.memory_compress_batch(data, inputs, flags, cap=len(out) - 1) == (None, None)
    assert lib.memory_compress_batch(data, inputs[:2] + [(5, 0)], GZIP) == (None, None)       # an empty input
    assert lib.memory_compress_batch(data, [(len(data) - 10, 11)], GZIP) == (None, None)      # past the end
    assert lib.memory_compress_batch(data, inputs, 3) == (None, None)                         # two framings


def check_bgzf_api_verifies(lib):
    d = mixed_input()[80000:100000]
    lib.set_verify(1)
    try:
        v0 = lib.verified_bytes()
        assert lib.memory_compress_bgzf(d, 0) is not None
        assert lib.verified_bytes() - v0 == len(d)
    finally:
        lib.set_verify(0)


# ---- 7: the tool ------------------------------------------------------------------------------------------------------------------------------------
def check_cli(cli, tmp_path, checker):
    data = F.text(65280, 800) + F.noise(65280, 801)[:65280] + F.text(1234, 802)
    src, mid, back = (os.path.join(str(tmp_path), n) for n in ("three.in", "three.gz", "three.out"))
    with open(src, "wb") as f:
        f.write(data)
    r = subprocess.run([cli, "-f", "bgzf", "-c", "-v", src, mid], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "verified %d bytes" % len(data) in r.stdout, r.stdout + r.stderr
    got = open(mid, "rb").read()
    assert got == bgzf_file(checker, data, 65280) and len(F.walk(got)[0]) == 4
    r = subprocess.run([cli, "-x", "-m", "-f", "gzip", mid, back], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and open(back, "rb").read() == data, r.stdout + r.stderr
    r = subprocess.run([cli, "-f", "bgzf", "-b", "70000", src, mid], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "65280" in r.stderr, r.stdout + r.stderr
    r = subprocess.run([cli, "-f", "bgzf", "-b", "20000", src, mid], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and open(mid, "rb").read() == bgzf_file(checker, data, 20000), r.stdout + r.stderr
