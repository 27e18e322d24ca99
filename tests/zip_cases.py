"""Shared by tests/test_zip_emu.py (CPU emulator build) and tests/test_zip_gpu.py (product library on the MI355X): the cases and the checks of ZIP
archives written on the device — zultra_hip_zip_members (zh_zip_scan, zh_zip_records and zh_zip_copy of zultra_amd/csrc/zh_zip.h),
zultra_zip_end_records, zultra_memory_compress_zip and the tool's -a. The expected archive never comes from the code under test: struct.pack per
the layouts of APPNOTE.TXT around the reference's raw deflate stream (the `checker` fixture's memory_compress) with binascii.crc32; Python's zipfile
opens every archive."""
import binascii
import ctypes as C
import io
import os
import struct
import subprocess
import zipfile

import numpy as np

import frame_member_cases as M
import inflate_file_cases as F
import verify_cases as V
from inflate_cases import device_read

EMPTY = 0xFFFFFFFF
DOS_DEFAULT = 0x00210000      # 1980-01-01 00:00:00
LIMIT = 0xFFFFFFFF
_STREAM = {}
u8 = M.u8


# ---- the expected bytes ---------------------------------------------------------------------------------------------------------------------------
def want_stream(checker, data, max_block):
    key = (bytes(data), max_block)
    if key not in _STREAM:
        _STREAM[key] = bytes(checker.memory_compress(u8(data), 0, max_block))
    return _STREAM[key]


def _common(name, data, stream, dos):
    """What a local and a central header share: version needed .. extra length."""
    empty = len(data) == 0
    return struct.pack("<HHHHHIIIHH", 10 if empty else 20, 0x0800, 0 if empty else 8, dos & 0xFFFF, dos >> 16, binascii.crc32(data) if not empty else 0,
                       len(stream), len(data), len(name), 0)


def want_parts(checker, parts, names, max_block, base_off=0, dos=DOS_DEFAULT):
    """-> (local part, central part, [offset of every local header in the archive], [the streams]) of the entries (names[i], parts[i]); max_block: one
    for all, or one per entry."""
    local, central, offs, streams = b"", b"", [], []
    for i, (p, name) in enumerate(zip(parts, names)):
        mb = max_block[i] if isinstance(max_block, (list, tuple)) else max_block
        stream = want_stream(checker, p, mb) if len(p) else b""
        offs.append(base_off + len(local))
        streams.append(stream)
        common = _common(name, p, stream, dos)
        local += struct.pack("<I", 0x04034b50) + common + name + stream
        central += struct.pack("<IH", 0x02014b50, 20) + common + struct.pack("<HHHII", 0, 0, 0, 0, offs[-1]) + name
    return local, central, offs, streams


def want_end_records(n, central_off, central_size):
    out = b""
    if n > 65535:
        out += struct.pack("<IQHHIIQQQQ", 0x06064b50, 44, 45, 45, 0, 0, n, n, central_size, central_off)
        out += struct.pack("<IIQI", 0x07064b50, 0, central_off + central_size, 1)
    return out + struct.pack("<IHHHHIIH", 0x06054b50, 0, 0, min(n, 0xFFFF), min(n, 0xFFFF), central_size, central_off, 0)


def want_archive(checker, parts, names, max_block, dos=DOS_DEFAULT):
    local, central, _, _ = want_parts(checker, parts, names, max_block, 0, dos)
    return local + central + want_end_records(len(parts), len(local), len(central))


def check_zipfile(buf, names, parts):
    """Python's zipfile reads the archive: sound, these names, these contents; an empty entry is stored."""
    z = zipfile.ZipFile(io.BytesIO(buf))
    assert z.testzip() is None
    assert z.namelist() == [n.decode("utf-8") for n in names]
    for info, name, p in zip(z.infolist(), names, parts):
        assert z.read(info) == p, name
        assert (info.file_size, info.compress_type) == (len(p), zipfile.ZIP_DEFLATED if len(p) else zipfile.ZIP_STORED), name
    return z


def enc(names):
    return [n.encode("utf-8") if isinstance(n, str) else bytes(n) for n in names]


def compress_files(ctx, parts):
    sizes = [len(p) for p in parts]
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    return ctx.compress_files(u8(b"".join(parts)), offsets, sizes)


def zipped(ctx, checker, parts, names, max_block, base_off=0, dos=0):
    """zip_members over the context's last batch — the non-empty parts, in order — held to the expected local and central part and entries[] to both.
    -> (entries, local part, central part)."""
    names = enc(names)
    eb = None
    if any(len(p) == 0 for p in parts):
        eb, k = [], 0
        for p in parts:
            eb.append(k if len(p) else EMPTY)
            k += 1 if len(p) else 0
    rc, ent, local, central, central_at = ctx.zip_members(names, eb, base_off, dos)
    assert rc == 0, (rc, ctx.lib.L.zultra_hip_last_error(ctx.h))
    want_local, want_central, offs, streams = want_parts(checker, parts, names, max_block, base_off, dos or DOS_DEFAULT)
    assert (local, central) == (len(want_local), len(want_central)) and central_at % 16 == 0 and central_at >= local, (local, central, central_at)
    for i, e in enumerate(ent):
        got = tuple(int(e[k]) for k in ("local_off", "comp_size", "size", "crc32", "name_len"))
        assert got == (offs[i], len(streams[i]), len(parts[i]), binascii.crc32(parts[i]) if len(parts[i]) else 0, len(names[i])), (i, got)
    got_local, got_central = ctx.zip_read(local).tobytes(), ctx.zip_read(central, central_at).tobytes()
    if got_local != want_local:
        at = next(k for k in range(len(want_local)) if got_local[k] != want_local[k])
        raise AssertionError("the local part differs at byte %d of %d (entry %d)" % (at, len(want_local), max(i for i, o in enumerate(offs) if o - base_off <= at)))
    assert got_central == want_central
    return ent, got_local, got_central


# ---- 1: every source and destination alignment ----------------------------------------------------------------------------------------------------
def _sized_stream(checker, size):
    """An input whose raw deflate stream has exactly `size` bytes, searched with the checker: short windows of text."""
    tries = 0
    for n in range(size - 8, size + 24):
        for seed in range(60):
            if n < 1 or tries >= 2000:
                continue
            tries += 1
            p = F.text(n, 1000 + seed)
            if len(want_stream(checker, p, 32768)) == size:
                return p
    return None


_GRID = {}


def alignment_grid(checker):
    """About 45 inputs of 1 .. 3000 bytes — text, noise, zeros — and their names, ordered and named so that over the batch a stream starts at every source
    address mod 16 (the inputs are picked from a pool by the size of the reference's stream) and at every destination address mod 16 (the name
    lengths: 1 .. 17 first, then whatever moves the stream to the residue wanted next). -> (parts, names, notes)."""
    if _GRID:
        return _GRID["v"]
    fixed = [F.text(1, 1), F.text(2, 2), F.noise(1, 3)]
    notes = []
    for size in (16, 32):
        p = _sized_stream(checker, size)
        if p is None:
            notes.append("no input with a stream of exactly %d bytes found in 2000 tries: that sub-case is skipped" % size)
        else:
            fixed.append(p)
    sizes = [3, 5, 9, 17, 31, 33, 47, 64, 100, 129, 200, 255, 300, 411, 512, 700, 901, 1024, 1333, 1500, 1777, 2048, 2500, 3000]
    pool = [F.text(n, 20 + i) for i, n in enumerate(sizes)] + [F.noise(n, 50 + i) for i, n in enumerate(sizes[::2])] + [bytes(n) for n in sizes[1::3]] + \
           [F.text(40 + 7 * i, 90 + i) for i in range(16)]
    parts, src, seen = [], 0, set()
    for p in fixed:
        parts.append(p)
        seen.add(src % 16)
        src += len(want_stream(checker, p, 32768))
    while pool and len(parts) < 48:
        # the next input: one behind which the following stream starts at a residue not seen yet, if the pool has one
        seen.add(src % 16)
        k = next((k for k, p in enumerate(pool) if (src + len(want_stream(checker, p, 32768))) % 16 not in seen), 0)
        p = pool.pop(k)
        parts.append(p)
        src += len(want_stream(checker, p, 32768))
    names, at = [], 0
    alphabet = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"
    for i, p in enumerate(parts):
        if i < 17:
            n = i + 1
        else:
            n = 1 + ((i % 16) - (at + 30 + 1)) % 16 + (16 if i % 5 == 0 else 0)     # the stream starts at residue i mod 16
        names.append((alphabet[i] + "n" * (n - 1)).encode())
        at += 30 + n + len(want_stream(checker, p, 32768))
    _GRID["v"] = (parts, names, notes)
    return _GRID["v"]


def check_alignment_grid(lib, checker):
    parts, names, notes = alignment_grid(checker)
    for note in notes:
        print(note)
    assert 40 <= len(parts) <= 48 and {len(n) for n in names} >= set(range(1, 18))
    ctx = lib.files_context(8191, len(parts))
    try:
        file_off = compress_files(ctx, parts)
        ent, local, central = zipped(ctx, checker, parts, names, 32768)
        assert {int(v) % 16 for v in file_off[:-1]} == set(range(16)), sorted({int(v) % 16 for v in file_off[:-1]})
        assert {(int(e["local_off"]) + 30 + int(e["name_len"])) % 16 for e in ent} == set(range(16))
        comp = [int(e["comp_size"]) for e in ent]
        assert min(comp) < 16 and (notes or (16 in comp and 32 in comp)), comp
        buf = local + central + want_end_records(len(parts), len(local), len(central))
        assert buf == want_archive(checker, parts, names, 32768)
        check_zipfile(buf, names, parts)
    finally:
        ctx.close()
    return len(parts)


# ---- 2: more entries than the scan has threads ----------------------------------------------------------------------------------------------------
def check_many(lib, checker, n):
    """n inputs of 30 .. 90 bytes in a files context: above 1024 a thread of zh_zip_scan walks a chunk of several entries; with ZULTRA_HIP_GRID_CAP in
    the environment a lane of zh_zip_records writes several entries' records and a wave of zh_zip_copy copies several streams."""
    checker = checker or M.make_checker()
    parts = M.small_inputs(n)
    names = [("dir%d/f%05d.txt" % (i % 7, i)).encode() for i in range(n)]
    ctx = lib.files_context(8191, n)
    try:
        compress_files(ctx, parts)
        ent, local, central = zipped(ctx, checker, parts, names, 32768, base_off=12345, dos=(((2026 - 1980) << 9 | 10 << 5 | 20) << 16) | (13 << 11 | 37 << 5 | 4))
        _, local0, central0 = zipped(ctx, checker, parts, names, 32768)
        check_zipfile(local0 + central0 + want_end_records(n, len(local0), len(central0)), names, parts)
    finally:
        ctx.close()
    return n


# ---- 3: a large entry -------------------------------------------------------------------------------------------------------------------------------
def check_large(lib, checker, noise_size, text_size):
    """One entry of noise (the stored form) and one of text in a context of max-blocks: several slices of zh_zip_copy each, at a capped grid too."""
    text = (F.text(100000, 5) + F.text(100000, 11) + F.text(100000, 23))[:text_size]
    parts, names = [F.noise(noise_size, 77), text], [b"noise.bin", b"text/long name with spaces.txt"]
    max_block = max(32768, noise_size, text_size)
    ctx = lib.context(max_block, 2)
    try:
        M.compress(ctx, parts)
        ent, local, central = zipped(ctx, checker, parts, names, max_block)
        assert int(ent[0]["comp_size"]) > noise_size and F.noise(noise_size, 77)[1000:2000] in local
        check_zipfile(local + central + want_end_records(2, len(local), len(central)), names, parts)
        return [int(e["comp_size"]) for e in ent]
    finally:
        ctx.close()


# ---- 4, 5: the host API -----------------------------------------------------------------------------------------------------------------------------
def api_archive(lib, checker, parts, names, dos=0, verify=False):
    """zultra_memory_compress_zip over (names[i], parts[i]) held to the expected archive and to zipfile. -> the archive."""
    names = enc(names)
    lead = b"\xee" * 5
    data = lead + b"".join(parts)
    offs = np.concatenate([[0], np.cumsum([len(p) for p in parts])[:-1]]) + len(lead)
    inputs = [(int(o), len(p)) for o, p in zip(offs, parts)]
    if verify:
        lib.set_verify(1)
    try:
        v0 = lib.verified_bytes()
        got = lib.memory_compress_zip(data, inputs, names, dos)
        if verify:
            assert lib.verified_bytes() - v0 == sum(len(p) for p in parts)
    finally:
        lib.set_verify(0)
    large = max([len(p) for p in parts if len(p) >= 8192] or [0])
    max_block = [32768 if len(p) < 8192 else max(32768, large) for p in parts]
    want = want_archive(checker, parts, names, max_block, dos or DOS_DEFAULT)
    assert got is not None and len(got) == len(want) and got == want, (None if got is None else len(got), len(want))
    check_zipfile(got, names, parts)
    assert lib.memory_bound_zip(sum(len(p) for p in parts), sum(len(n) for n in names), len(parts)) >= len(got)
    assert lib.memory_compress_zip(data, inputs, names, dos, cap=len(got) - 1) is None                  # one byte short
    return got


def check_api_mixed(lib, checker, large_size, small_size):
    """Small, large, small: a files batch, a batch of max-blocks, a files batch, base_off carried from one to the next; a name that is not ASCII and one of 300 bytes."""
    parts = [F.text(100, 700), F.text(small_size // 2, 701), F.noise(50, 702), F.text(large_size, 703), F.noise(8192, 704), F.text(small_size, 705), F.text(1, 706)]
    names = ["a.txt", "grüße/日本語.txt", "n" * 296 + ".bin", "big/one.txt", "big/two.txt", "z/last but one", "z/last"]
    assert len(enc(names)[2]) == 300 and len(enc(names)[1]) > len(names[1])
    api_archive(lib, checker, parts, names, verify=True)
    return len(parts)


def check_api_empty_entries(lib, checker):
    """Empty entries first, last, two adjacent, a directory, between two batches of different kinds; and an archive of empty entries only."""
    parts = [b"", F.text(300, 710), b"", b"", F.text(77, 711), b"", F.text(9000, 712), b"", F.text(20, 713), b""]
    names = ["empty first", "one.txt", "d/", "d/empty", "d/two.txt", "between/", "large.txt", "behind large", "three.txt", "empty last"]
    z = check_zipfile(api_archive(lib, checker, parts, names, dos=0x5b54a825), enc(names), parts)
    assert z.getinfo("d/").is_dir() and z.getinfo("one.txt").date_time == (2025, 10, 20, 21, 1, 10)
    only = [b"", b"", b""]
    api_archive(lib, checker, only, ["x/", "x/y/", "x/y/nothing"])


def check_api_refusals(lib):
    big = bytes(2097153)
    assert lib.memory_compress_zip(big, [(0, len(big))], ["too large"]) is None                       # above one max-block
    assert lib.memory_compress_zip(big, [(0, 100)], [""]) is None                                     # a name of length 0
    assert lib.memory_compress_zip(big, [(0, 100)], ["n" * 65536]) is None
    assert lib.memory_compress_zip(big, [(len(big) - 10, 11)], ["past the end"]) is None


# ---- 6, 7: round trip on the device; the stream buffer is untouched -------------------------------------------------------------------------------
def check_round_trip(lib, checker, scale):
    """scale: the size of the texts, in units of 500 bytes (the emulator takes the small ones)."""
    parts = [F.text(500 * scale, 400), F.text(1, 401), F.noise(700, 402), F.text(1500 * scale, 403) + F.noise(9000, 404), F.text(3000 * scale, 405), F.text(77, 406)]
    names = ["r/%d" % i + "x" * i for i in range(len(parts))]
    sizes = [len(p) for p in parts]
    dst_off = [0] + [int(v) for v in np.cumsum(sizes)]
    plain = b"".join(parts)
    base_off = 1000003
    ctx = lib.context(65536, len(parts))
    d = V.DeviceCopy(lib, np.zeros(len(plain) + 16, dtype=np.uint8))
    try:
        M.compress(ctx, parts)
        gzip_before, _ = M.framed(ctx, checker, parts, M.GZIP, 65536)
        raw_off = ctx.stitch_files()
        raw = ctx.stream_read(int(raw_off[-1])).tobytes()
        ent, local, central = zipped(ctx, checker, parts, names, 65536, base_off=base_off)
        # inflate the entries where they stand in the zip buffer
        items = [(int(e["local_off"]) - base_off + 30 + int(e["name_len"]), int(e["comp_size"]), dst_off[i], sizes[i]) for i, e in enumerate(ent)]
        rc, results, _ = lib.inflate_streams(ctx.zip_ptr()[0], len(local), d.ptr, len(plain), items)
        assert rc == 0 and [int(r["reason"]) for r in results] == [0] * len(parts), (rc, results)
        assert device_read(lib, d, len(plain)).tobytes() == plain
        # the stream buffer is as the plain assembly left it: it reads the same, verifies, and frames as it did before
        assert ctx.stream_read(len(raw)).tobytes() == raw
        v = ctx.verify()
        assert v["rc"] == 0 and v["verified_bytes"] == len(plain), v
        assert [int(x) for x in ctx.stitch_files()] == [int(x) for x in raw_off]
        gzip_after, _ = M.framed(ctx, checker, parts, M.GZIP, 65536)
        assert gzip_after == gzip_before
        # ... and behind framed members the call assembles the plain layout itself
        zipped(ctx, checker, parts, names, 65536)
        assert ctx.verify()["rc"] == 0 and ctx.stream_read(len(raw)).tobytes() == raw
    finally:
        d.free()
        ctx.close()


# ---- 8: refusals ------------------------------------------------------------------------------------------------------------------------------------
def _zip_write(lib, ctx, data):
    ptr = ctx.zip_ptr()[0]
    if lib.is_emulator:
        C.memmove(ptr, data, len(data))
    else:
        keep = u8(data)
        assert V._Hip.lib().hipMemcpy(ptr, keep.ctypes.data, len(keep), 1) == 0


def check_refusals(lib, checker):
    parts = [F.text(500, 800), F.noise(300, 801), F.text(2000, 802)]
    names = ["a", "bb", "ccc"]
    ctx = lib.context(32768, 4)
    try:
        assert ctx.zip_members(names)[0] == -1 and ctx.zip_ptr()[0] is None                         # before any batch
        M.compress(ctx, parts)
        ent, local, central = zipped(ctx, checker, parts, names, 32768)
        total = len(local) + len(central)
        zipped(ctx, checker, parts, names, 32768, base_off=LIMIT - total - 1)      # one byte below the limit is an archive
        room = ctx.zip_ptr()[1] + len(central)
        mark_s, mark_z = bytes((i * 7 + 3) & 255 for i in range(len(local) + 64)), bytes((i * 11 + 5) & 255 for i in range(room))
        ctx.stream_write(mark_s)
        _zip_write(lib, ctx, mark_z)

        def untouched(what):
            assert ctx.stream_read(len(mark_s)).tobytes() == mark_s, "a refused call has written the stream buffer: " + what
            assert ctx.zip_read(len(mark_z)).tobytes() == mark_z, "a refused call has written the zip buffer: " + what

        refused = [("a name of length 0", (["a", "", "ccc"],), -1), ("a max-block twice", (names, [0, 1, 1]), -1), ("a max-block skipped", (names, [0, 2, EMPTY]), -1),
                   ("out of order", (names, [1, 0, 2]), -1), ("a max-block missing", (names, [0, 1, EMPTY]), -1), ("a max-block past the batch", (names + ["d"], [0, 1, 2, 3]), -1),
                   ("fewer entries than max-blocks", (names[:2],), -1), ("more entries than max-blocks", (names + ["d"],), -1),
                   ("the total reaches the limit", (names, None, LIMIT - total), -2), ("base_off beyond it", (names, None, 1 << 33), -2)]
        for what, args, rc in refused:
            assert ctx.zip_members(*args)[0] == rc, what
            untouched(what)
        # a max-block with history
        ctx.compress_blocks(u8(F.noise(12000, 803)), [(0, 0, 6000), (0, 6000, 6000)])
        assert ctx.zip_members(["a", "b"])[0] == -1
        untouched("a max-block with history")
    finally:
        ctx.close()


# ---- 9: the end records -----------------------------------------------------------------------------------------------------------------------------
def check_end_records(lib):
    for n in (0, 1, 65535, 65536, 1000000):
        for off, size in ((0, 0), (123456789, 46 * 3 + 10), (LIMIT - 1, LIMIT - 1)):
            want = want_end_records(n, off, size)
            assert len(want) == (98 if n > 65535 else 22)
            assert lib.zip_end_records(n, off, size) == want, (n, off, size)
            assert lib.zip_end_records(n, off, size, cap=len(want)) == want
            assert lib.zip_end_records(n, off, size, cap=len(want) - 1) is None                   # the buffer one byte short
    assert lib.zip_end_records(1, LIMIT, 10) is None and lib.zip_end_records(1, 10, LIMIT) is None and lib.zip_end_records(70000, 1 << 32, 10) is None


def check_zip64_end(lib):
    """65 537 inputs of 8 bytes: two files batches at the least, and the ZIP64 end records."""
    n = 65537
    rs = np.random.RandomState(9)
    data = rs.randint(97, 123, size=8 * n).astype(np.uint8)
    names = [b"%05x" % i for i in range(n)]
    got = lib.memory_compress_zip(data, [(8 * i, 8) for i in range(n)], names)
    assert got is not None
    z = zipfile.ZipFile(io.BytesIO(got))
    assert len(z.namelist()) == n and z.testzip() is None
    for i in (0, n // 2, n - 1):
        assert z.read(names[i].decode()) == data[8 * i: 8 * i + 8].tobytes(), i
    central_size = sum(46 + len(s) for s in names)
    end = want_end_records(n, len(got) - 98 - central_size, central_size)
    assert got[-98:] == end


# ---- 10: the tool -----------------------------------------------------------------------------------------------------------------------------------
def check_cli(cli, lib, tmp_path, checker):
    parts = [F.text(5000, 900), b"", F.text(70000, 901)]
    names = ["one.txt", "empty.bin", "sub/three.txt"]
    os.makedirs(os.path.join(str(tmp_path), "sub"))
    for name, p in zip(names, parts):
        with open(os.path.join(str(tmp_path), name), "wb") as f:
            f.write(p)
    r = subprocess.run([cli, "-c", "-v", "-a", "out.zip"] + names, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0 and "verified %d bytes" % sum(len(p) for p in parts) in r.stdout, r.stdout + r.stderr
    got = open(os.path.join(str(tmp_path), "out.zip"), "rb").read()
    data = b"".join(parts)
    assert got == lib.memory_compress_zip(data, [(0, 5000), (5000, 0), (5000, 70000)], names)
    assert got == want_archive(checker, parts, enc(names), [32768, 32768, 70000])
    check_zipfile(got, enc(names), parts)
    with open(os.path.join(str(tmp_path), "huge"), "wb") as f:
        f.write(bytes(2097153))
    r = subprocess.run([cli, "-a", "out2.zip", "one.txt", "huge"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode != 0 and "huge" in r.stderr, r.stdout + r.stderr
    # the old forms with a wrong count of arguments: the usage, 100
    for args in (["one.txt"], ["-x", "one.txt"], ["-x", "-m", "one.txt"], ["-f", "bgzf", "one.txt"], ["one.txt", "a", "b"], ["-a", "out3.zip"], []):
        r = subprocess.run([cli] + args, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert r.returncode == 100 and "usage:" in r.stderr, (args, r.stdout + r.stderr)
