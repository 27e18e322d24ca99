"""Shared by tests/test_inflate_file_emu.py (CPU emulator build) and tests/test_inflate_file_gpu.py (product library on the MI355X): the files, the
runners and the checks of the member index (zh_ix_tiles, zh_ix_resolve and zh_ix_items, zultra_amd/csrc/zh_inflate_index.h), of
zultra_hip_index_members, zultra_hip_inflate_file and zultra_memory_decompress_members. The yardstick of the index is `walk` below, the serial walk
DESIGN.md 3.11 defines; of the bytes Python's gzip.decompress / zlib.decompressobj(wbits=31), member by member; of the per-member results
zultra_hip_inflate_members given the walker's items. BGZF files are built by hand: a deflate stream, an 18-byte header in front, CRC-32 and ISIZE
behind. The tile size comes from the environment (ZULTRA_HIP_INDEX_TILE), so every tile size but the default runs in a process of its own."""
import ctypes
import gzip
import os
import subprocess
import sys
import zlib

import numpy as np

import corpus
import inflate_cases as I
import verify_cases as V
from inflate_cases import CANARY, CANARY_BYTE

GZIP = 2
DEFAULT_TILE = 256 * 1024
TILES = (32, 100, 256, 4096)
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


# ---- the yardstick: the serial walk ---------------------------------------------------------------------------------------------------------
def _le(buf, at, n):
    return int.from_bytes(buf[at: at + n], "little")


def probe(buf, p):
    """-> (None, L, ISIZE) where a hinted member starts at p, else (stop kind, 0, 0)."""
    S = len(buf)
    if p == S:
        return 0, 0, 0
    if S - p < 12 or buf[p: p + 3] != b"\x1f\x8b\x08":
        return 3, 0, 0
    if not buf[p + 3] & 4:
        return 1, 0, 0
    xlen = _le(buf, p + 10, 2)
    if p + 12 + xlen > S:
        return 1, 0, 0
    at, end = p + 12, p + 12 + xlen
    while end - at >= 4:
        slen = _le(buf, at + 2, 2)
        if at + 4 + slen > end:
            break
        if buf[at: at + 2] == b"BC" and slen == 2:
            L = _le(buf, at + 4, 2) + 1
            if L < 12 + xlen + 8 or p + L > S:
                return 2, 0, 0
            return None, L, _le(buf, p + L - 4, 4)
        at += 4 + slen
    return 1, 0, 0


def walk(buf):
    """-> (items [(src_off, src_size, dst_off, dst_cap)], stop kind, stop position, output bytes)."""
    buf = bytes(buf)
    p = out = 0
    items = []
    while True:
        kind, L, isize = probe(buf, p)
        if kind is not None:
            return items, kind, p, out
        items.append((p, L, out, isize))
        out += isize
        p += L


# ---- members by hand ------------------------------------------------------------------------------------------------------------------------
def stored(data):
    """One final stored block: the payload lies in the stream byte for byte."""
    assert len(data) <= 65535
    return b"\x01" + len(data).to_bytes(2, "little") + (len(data) ^ 0xFFFF).to_bytes(2, "little") + bytes(data)


def deflated(data, level=6):
    return I.zlib_raw(data, level, zlib.Z_DEFAULT_STRATEGY)


def bgzf(data, raw=None, before=b"", after=b"", flg=0, name=b"name", comment=b"c", bsize_delta=0, isize=None, bc=True, level=6):
    """A member with the `BC` subfield between the subfields `before` and `after` of its extra field; flg: FNAME / FCOMMENT / FHCRC on top of
    FEXTRA. bsize_delta: what BSIZE lies by; isize: what ISIZE says instead of the truth; bc False: no BC subfield at all."""
    data = bytes(data)
    raw = deflated(data, level) if raw is None else raw
    flg |= 4
    extra_len = len(before) + (6 if bc else 0) + len(after)
    tail = (name + b"\0" if flg & 8 else b"") + (comment + b"\0" if flg & 16 else b"")
    total = 12 + extra_len + len(tail) + (2 if flg & 2 else 0) + len(raw) + 8
    sub = b"BC\x02\x00" + ((total - 1 + bsize_delta) & 0xFFFF).to_bytes(2, "little") if bc else b""
    h = b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\x00\xff" + extra_len.to_bytes(2, "little") + before + sub + after + tail
    if flg & 2:
        h += (zlib.crc32(h) & 0xFFFF).to_bytes(2, "little")
    m = h + raw + zlib.crc32(data).to_bytes(4, "little") + ((len(data) if isize is None else isize) & 0xFFFFFFFF).to_bytes(4, "little")
    assert len(m) == total and total <= 65536
    return m


def sub(si, data):
    return si + len(data).to_bytes(2, "little") + data


_TEXT = []


def text(n, seed):
    """n bytes of text: a window, chosen by `seed`, into one generated text (corpus.text_like builds a vocabulary per call)."""
    if not _TEXT:
        _TEXT.append(corpus.text_like(200000, 1).tobytes())
    at = (seed * 7919) % (len(_TEXT[0]) - n + 1)
    return _TEXT[0][at: at + n]


def noise(n, seed):
    return corpus.noise(n, seed).tobytes()


def filler(length, seed):
    """A member of exactly `length` bytes (>= 31): noise in a stored block."""
    return bgzf(noise(length - 31, seed), raw=stored(noise(length - 31, seed)))


def pad_to(target, seed=0):
    """Members whose lengths add up to exactly `target` (0, or >= 31)."""
    out, left = [], target
    while left > 60031 + 31:
        out.append(filler(60031, seed + len(out)))
        left -= 60031
    if left > 60031:
        out.append(filler(left // 2, seed + len(out)))
        left -= left // 2
    if left:
        out.append(filler(left, seed + len(out)))
    return out


# ---- the files of the index cases -------------------------------------------------------------------------------------------------------------
def header_files():
    body = text(700, 1)
    out = [("bc_alone", bgzf(body)),
           ("bc_behind", bgzf(body, before=sub(b"XY", b"abcde"))),
           ("bc_in_front", bgzf(body, after=sub(b"XY", b"abc"))),
           ("slen0_in_front", bgzf(body, before=sub(b"ZZ", b""))),
           ("bc_wrong_slen_first", bgzf(body, before=sub(b"BC", b"abc"))),
           ("with_name_comment_hcrc", bgzf(body, flg=8 | 16 | 2) + bgzf(body[:50], flg=2) + bgzf(body[:9], flg=16)),
           ("eof_marker", EOF_MARKER),
           ("member_and_eof", bgzf(body) + EOF_MARKER)]
    for n in (0, 1, 65280, 65536):
        d = text(n, n & 7)
        out.append(("isize_%d" % n, bgzf(d) + EOF_MARKER))
    for count in (1, 2, 63, 64, 65, 257):
        out.append(("count_%d" % count, b"".join(bgzf(text(1 + (k * 37) % 90, k)) for k in range(count))))
    assert EOF_MARKER == bgzf(b"", raw=b"\x03\x00") and len(EOF_MARKER) == 28
    return out


def boundary_files(T):
    """A member that starts exactly on the boundary B of two tiles, one byte before it and one byte after it; members longer than several tiles and
    many to a tile come with the tile sizes."""
    B = T * (31 // T + 1)
    out = []
    for delta in (-1, 0, 1):
        ms = pad_to(B + delta, 3) + [bgzf(text(200, 4)), bgzf(text(40, 5)), EOF_MARKER]
        out.append(("boundary%+d" % delta, b"".join(ms)))
    sizes = [0, 1, 5, 300, 3000, 20000, 7, 7, 7, 65280, 2, 900]
    out.append(("mixed_sizes", b"".join(bgzf(text(n, k)) if k & 1 else bgzf(noise(n, k), raw=stored(noise(n, k))) for k, n in enumerate(sizes)) + EOF_MARKER))
    out.append(("eof_markers_5000", EOF_MARKER * 5000))
    return out


def fake_header(L):
    """A complete hinted header that says its member is L bytes long."""
    return b"\x1f\x8b\x08\x04\0\0\0\0\x00\xff\x06\x00BC\x02\x00" + ((L - 1) & 0xFFFF).to_bytes(2, "little")


def decoy_member(offset, T, fake, cut=0):
    """A member for position `offset` whose stored payload ends with `fake` (less its last `cut` bytes), the fake lying exactly on the next tile
    boundary that leaves the member 23 bytes of head room: it is the first candidate of that tile, and the member ends in the same tile."""
    B = T * ((offset + 23) // T + 1)
    payload = noise(B - offset - 23, 9).replace(b"\x1f\x8b\x08", b"\x1f\x8b\x09") + fake[: len(fake) - cut]
    m = bgzf(payload, raw=stored(payload))
    assert m[B - offset: B - offset + len(fake) - cut] == fake[: len(fake) - cut]
    return m


def decoy_files(T):
    """-> [(name, file, tiles_rewalked must be > 0, == 0, or None for whatever the walker's result needs)]."""
    B = T * (2 * 60031 // T + 2)                   # (far enough for two tiles in front under every tile size but the default)
    lead = pad_to(B - 23 - min(T, 20000), 11)      # the decoy member then starts min(T, 20000) + 23 bytes in front of a boundary
    at = sum(len(m) for m in lead)
    rest = [bgzf(text(300, 12)), bgzf(text(30, 13)), EOF_MARKER]
    out = []
    for name, fake, cut, rewalked in (("a_first_candidate_is_fake", fake_header(40), 0, True), ("b_chain_rejoins", fake_header(26), 0, True),
                                      ("c_bsize_past_the_end", fake_header(65536), 0, False), ("d_cut_by_the_member_end", fake_header(40), 4, None)):
        ms = lead + [decoy_member(at, T, fake, cut)] + (rest if name[0] != "c" else rest[:1])
        out.append((name, b"".join(ms), rewalked))
    B1 = T * (31 // T + 1)
    out.append(("e_guess_is_right", b"".join(pad_to(B1, 14) + rest), False))   # the first candidate of the second tile used IS the chain's entry
    return out


def stop_files():
    body = text(90, 20)
    a, b, c = bgzf(body), bgzf(body[:60]), bgzf(body[:75])
    plain = gzip.compress(body, 6, mtime=0)
    out = [("plain_first", plain + a + b), ("plain_middle", a + plain + b), ("plain_last", a + b + plain),
           ("fextra_without_bc", a + bgzf(body, bc=False, before=sub(b"XY", b"abcdef")) + b),
           ("slen_past_xlen", a + bgzf(body, before=b"XY\x40\x00") + b),
           ("bsize_past_the_end", a + bgzf(body, bsize_delta=1)),
           ("bsize_past_the_end_middle", a + bgzf(body, bsize_delta=2000) + b),
           ("bsize_short", a + bgzf(body, bsize_delta=-(len(bgzf(body)) - 25)) + b),
           ("bsize_short_by_one_of_minimum", a + fake_header(25) + b"\0" * 30),
           ("bsize_minimum", a + fake_header(26) + b"\0" * 8),
           ("trailing_garbage", a + b + b"garbage behind the last member"),
           ("trailing_zeros", a + b + b"\0" * 40),
           ("xlen_past_the_end", a + b"\x1f\x8b\x08\x04\0\0\0\0\x00\xff\xff\xffBC\x02\x00\x20\x00")]
    three = a + b + c
    assert 80 <= len(a) <= 140
    out += [("cut_%d" % n, three[:n]) for n in range(1, len(three))]
    return out


def index_files(T):
    return header_files() + boundary_files(T) + [f[:2] for f in decoy_files(T)] + stop_files()


# ---- the index --------------------------------------------------------------------------------------------------------------------------------
def check_index(lib, name, buf, on_device=False, lead=0):
    """zultra_hip_index_members over `buf`: items and totals are the walker's; the query form (items NULL) agrees; one item too few is stop 4."""
    want_items, stop, at, out = walk(buf)
    if on_device:
        held = V.DeviceCopy(lib, np.frombuffer(b"\xee" * lead + bytes(buf) + b"\xee" * 7, dtype=np.uint8).copy())
        src = held.ptr + lead
    else:
        held, src = None, np.frombuffer(bytes(buf) + b"\0", dtype=np.uint8).copy()[:-1]
    try:
        rc, res, items, _ = lib.index_members(src, len(buf), len(want_items) + 1)
        assert rc == 0 and (res.members, res.stop, res.src_used, res.out_size) == (len(want_items), stop, at, out), (name, rc, res.members, res.stop, res.src_used, res.out_size, stop, at, out)
        assert [tuple(int(v) for v in row) for row in items] == want_items, name
        assert 0 < res.tiles and res.tiles_rewalked <= res.tiles, name
        rc, q, _, _ = lib.index_members(src, len(buf), 0)
        assert rc == 0 and (q.members, q.stop, q.src_used, q.out_size, q.tiles, q.tiles_rewalked) == (res.members, stop, at, out, res.tiles, res.tiles_rewalked), name
        if len(want_items) > 1:
            rc, q, items, _ = lib.index_members(src, len(buf), len(want_items) - 1)
            assert rc == -1 and len(items) == 0 and (q.stop, q.members, q.out_size) == (4, len(want_items), out), name
    finally:
        if held:
            held.free()
    return res


def tile_size():
    t = int(os.environ.get("ZULTRA_HIP_INDEX_TILE", "0") or 0)
    return t if t >= 32 else DEFAULT_TILE


def check_index_files(lib):
    """Every file of cases 1 to 4 under the tile size of this process. -> files."""
    T = tile_size()
    files = index_files(T)
    for k, (name, buf) in enumerate(files):
        check_index(lib, name, buf, on_device=bool(k & 1), lead=k % 4)
    for name, buf, rewalked in decoy_files(T):
        res = check_index(lib, name, buf)
        if rewalked is not None:
            assert (res.tiles_rewalked > 0) == rewalked, (name, T, res.tiles, res.tiles_rewalked)
    kinds = {walk(buf)[1] for _, buf in files}
    assert kinds == {0, 1, 2, 3}
    return len(files)


def run_child(lib_path, is_emulator, call, env):
    """`call` (an expression over this module as F and the library as L) in a process of its own with `env` on top of the environment."""
    tests = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import inflate_file_cases as F\nfrom zultra_amd._ffi import Lib\nL = Lib(%r)\nL.is_emulator = %r\n"
            "print('child result', %s)\n") % (os.path.dirname(tests), tests, lib_path, bool(is_emulator), call)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "child result" in r.stdout, r.stdout + r.stderr
    return r.stdout


# ---- whole files ------------------------------------------------------------------------------------------------------------------------------
def run_file(lib, buf, on_device=True, src_lead=0, dst_lead=0, short=0, results=True):
    """zultra_hip_inflate_file over `buf` with exactly the room the walker counts, less `short`, canaries in front and behind.
    -> (rc, index result, [member results as tuples], the destination's bytes)."""
    items, stop, at, out = walk(buf)
    room = out - short
    if on_device:
        s = V.DeviceCopy(lib, np.frombuffer(b"\xee" * src_lead + bytes(buf) + b"\xee" * 7, dtype=np.uint8).copy())
        d = V.DeviceCopy(lib, np.full(dst_lead + CANARY + room + CANARY, CANARY_BYTE, dtype=np.uint8))
        try:
            rc, res, mem, ms = lib.inflate_file(s.ptr + src_lead, len(buf), d.ptr + dst_lead + CANARY, room, len(items) if results else None)
            back = I.device_read(lib, d, dst_lead + 2 * CANARY + room).copy()[dst_lead:]
        finally:
            s.free()
            d.free()
    else:
        src = np.frombuffer(bytes(buf) + b"\0", dtype=np.uint8).copy()[:-1]
        back = np.full(2 * CANARY + room, CANARY_BYTE, dtype=np.uint8)
        rc, res, mem, ms = lib.inflate_file(src, len(buf), back[CANARY:], room, len(items) if results else None)
    assert (back[:CANARY] == CANARY_BYTE).all() and (back[CANARY + room:] == CANARY_BYTE).all(), "a canary was written"
    assert len(ms) == 4
    return rc, res, [tuple(int(v) for v in r) for r in mem], back[CANARY: CANARY + room]


def members_path(lib, buf, on_device=True):
    """zultra_hip_inflate_members over the walker's items. -> (rc, [member results as tuples], the destination's bytes)."""
    items, stop, at, out = walk(buf)
    src = np.frombuffer(bytes(buf) + b"\0", dtype=np.uint8).copy()[:-1]
    dst = np.full(max(out, 1), CANARY_BYTE, dtype=np.uint8)
    if on_device:
        s, d = V.DeviceCopy(lib, src), V.DeviceCopy(lib, dst)
        try:
            rc, mem, _ = lib.inflate_members(s.ptr, len(buf), d.ptr, out, None, 0, GZIP, items)
            back = I.device_read(lib, d, len(dst)).copy()
        finally:
            s.free()
            d.free()
    else:
        rc, mem, _ = lib.inflate_members(src, len(buf), dst, out, None, 0, GZIP, items)
        back = dst
    return rc, [tuple(int(v) for v in r) for r in mem], back[:out]


def check_file(lib, name, buf, want=None, **kw):
    """The index result is the walker's, the per-member results and the bytes those of the members path; want: the bytes, where every member is sound."""
    items, stop, at, out = walk(buf)
    rc, res, mem, back = run_file(lib, buf, **kw)
    assert (res.members, res.stop, res.src_used, res.out_size) == (len(items), stop, at, out), (name, res.members, res.stop, res.src_used, res.out_size)
    if items:
        rc0, mem0, back0 = members_path(lib, buf, kw.get("on_device", True))
        assert rc == rc0 and mem == (mem0 if kw.get("results", True) else []), (name, rc, rc0, [(a, b) for a, b in zip(mem, mem0) if a != b][:3])
        mem = mem0
        for it, r in zip(items, mem):
            assert (back[it[2]: it[2] + r[2]] == back0[it[2]: it[2] + r[2]]).all(), (name, it)
        if not kw.get("on_device", True):   # of a host destination nothing but the members' out_size bytes is written
            mask = np.ones(out, dtype=bool)
            for it, r in zip(items, mem):
                mask[it[2]: it[2] + r[2]] = False
            assert (back[mask] == CANARY_BYTE).all(), name
    else:
        assert rc == 0 and mem == [], name
    if want is not None:
        assert rc == 0 and back.tobytes() == want, name
    return rc, res, mem, back


def whole_files(big):
    """Text, noise and zeros in members of 1 .. 65280 bytes of payload. -> [(name, file, the bytes)]"""
    out = []
    sizes = [1, 2, 255, 256, 257, 4000, 16384, 16385, 65280] if big else [1, 2, 255, 256, 257, 4000, 16385]
    for kind, gen in (("text", text), ("noise", noise), ("zeros", lambda n, seed: b"\0" * n)):
        parts = [gen(n, k + 3) for k, n in enumerate(sizes)]
        out.append((kind, b"".join(bgzf(p, level=(0 if kind == "noise" and k & 1 else 6)) for k, p in enumerate(parts)) + EOF_MARKER, b"".join(parts)))
    return out


def check_whole_files(lib, big):
    n = 0
    for name, buf, want in whole_files(big):
        assert gzip.decompress(buf) == want
        for kw in (dict(), dict(on_device=False), dict(src_lead=1, dst_lead=3), dict(src_lead=2, dst_lead=2), dict(src_lead=3, dst_lead=1), dict(results=False)):
            rc, res, mem, _ = check_file(lib, name, buf, want, **kw)
            assert res.stop == 0 and rc == 0
            n += 1
    # a stop of 1..3 is no error: the indexed prefix is decoded
    parts = [text(500, 40), text(77, 41)]
    prefix = bgzf(parts[0]) + bgzf(parts[1])
    for tail, kind in ((gzip.compress(b"plain", 6, mtime=0), 1), (b"garbage", 3), (bgzf(parts[0])[:-3], 2)):
        rc, res, mem, _ = check_file(lib, "stop%d" % kind, prefix + tail, b"".join(parts))
        assert rc == 0 and res.stop == kind and res.src_used == len(prefix)
    rc, res, mem, _ = check_file(lib, "nothing indexed", gzip.compress(b"plain", 6, mtime=0))
    assert (rc, res.members, res.stop, res.src_used) == (0, 0, 1, 0)
    return n


def check_large_file(lib):
    """128 members of 64 KiB of output each: the default tile is crossed many times."""
    assert tile_size() == DEFAULT_TILE
    parts = [(noise(65536, k) if k % 3 == 0 else text(65536, k)) for k in range(128)]
    parts = [p if k % 3 else p[:65280] for k, p in enumerate(parts)]
    buf = b"".join(bgzf(p, level=1) if k % 3 else bgzf(p, raw=stored(p)) for k, p in enumerate(parts)) + EOF_MARKER
    want = b"".join(parts)
    assert len(buf) > 8 * DEFAULT_TILE
    rc, res, mem, back = check_file(lib, "large", buf, want)
    assert res.members == 129 and res.tiles >= 8 and res.stop == 0
    check_index(lib, "large", buf, on_device=True, lead=1)


def check_damage(lib):
    """Member k of 9 damaged in four ways, with a device and with a host destination (of the latter check_file holds every byte outside the
    members' out_size bytes to the canary): only the members path's verdicts, every other member's bytes right where they belong; one byte short
    of room is stop 4 with nothing written."""
    parts = [text(300 + 50 * k, 60 + k) for k in range(9)]
    ms = [bgzf(p, raw=stored(p)) if k == 4 else bgzf(p) for k, p in enumerate(parts)]
    k = 4
    start = sum(len(m) for m in ms[:k])
    seen = set()
    for what, at, delta in (("payload", start + 18 + 5 + 100, 0x20), ("crc", start + len(ms[k]) - 8, 1), ("isize_up", start + len(ms[k]) - 4, 1), ("isize_down", start + len(ms[k]) - 4, -1)):
        buf = bytearray(b"".join(ms))
        buf[at] = (buf[at] + delta) & 255 if what.startswith("isize") else buf[at] ^ delta
        items = walk(buf)[0]
        for dev in (True, False):
            rc, res, mem, back = check_file(lib, what, bytes(buf), on_device=dev)
            assert rc == 1 and [r[0] for j, r in enumerate(mem) if j != k] == [0] * 8 and mem[k][0] in (13, 15, 16), (what, dev, [r[0] for r in mem])
            seen.add(mem[k][0])
            for j, (it, p) in enumerate(zip(items, parts)):
                if j != k:
                    assert back[it[2]: it[2] + len(p)].tobytes() == p, (what, dev, j)
    assert seen == {13, 15, 16}, seen
    buf = b"".join(ms)
    for dev in (True, False):
        rc, res, mem, back = run_file(lib, buf, on_device=dev, short=1)
        assert rc == -1 and res.stop == 4 and res.out_size == sum(len(p) for p in parts) and res.members == 9 and mem == []
        assert (back == CANARY_BYTE).all(), "a refused call has written"


def check_own_files(lib, nfiles):
    """A files batch of the library's coder framed as BGZF by the test and inflated as one file, device to device."""
    sizes = [I.FILE_SIZES[i % len(I.FILE_SIZES)] for i in range(nfiles)]
    parts = [(corpus.json_like, corpus.text_like)[i & 1](n, 100 + i).tobytes() for i, n in enumerate(sizes)]
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    ctx = lib.files_context(8191, nfiles)
    try:
        file_off = ctx.compress_files(np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), offsets, sizes)
        stream = ctx.stream_read(int(file_off[-1])).tobytes()
    finally:
        ctx.close()
    buf = b"".join(bgzf(p, raw=stream[int(file_off[i]): int(file_off[i + 1])]) for i, p in enumerate(parts)) + EOF_MARKER
    assert gzip.decompress(buf) == b"".join(parts)
    rc, res, mem, back = check_file(lib, "own files", buf, b"".join(parts))
    assert res.members == nfiles + 1 and rc == 0
    return nfiles


# ---- the host API, the command-line tool, arguments ----------------------------------------------------------------------------------------------
def check_host_api(lib):
    parts = [text(3000, 70), text(10, 71), noise(500, 72), b"", text(20000, 73), text(1, 74)]
    plain = gzip.compress(parts[2], 6, mtime=0)
    buf = bgzf(parts[0]) + bgzf(parts[1]) + plain + bgzf(parts[3]) + bgzf(parts[4]) + bgzf(parts[5]) + EOF_MARKER
    want = gzip.decompress(buf)
    assert want == b"".join(parts)
    assert lib.memory_decompress_members(buf, len(want)) == (want, 7)
    assert lib.memory_decompress_members(buf, len(want) + 100) == (want, 7)
    assert lib.memory_decompress_members(plain, 500) == (lib.memory_decompress(plain, GZIP, 500), 1) == (parts[2], 1)
    assert lib.memory_decompress_members(plain + plain, 1000) == (parts[2] * 2, 2)
    assert lib.memory_decompress_members(buf + b"garbage", len(want)) == (None, 0)         # a garbage tail
    assert lib.memory_decompress_members(buf + b"\0" * 12, len(want)) == (None, 0)         # trailing zeros
    assert lib.memory_decompress_members(plain + b"\0", 500) == (None, 0)
    bad = bytearray(buf)
    bad[len(bgzf(parts[0])) - 6] ^= 1                                                      # a damaged member (its CRC)
    assert lib.memory_decompress_members(bytes(bad), len(want)) == (None, 0)
    bad = bytearray(buf)
    bad[len(buf) - len(EOF_MARKER) - 40] ^= 1                                              # ... behind the plain member
    assert lib.memory_decompress_members(bytes(bad), len(want)) == (None, 0)
    assert lib.memory_decompress_members(buf, len(want) - 1) == (None, 0)                  # one byte short
    assert lib.memory_decompress_members(plain, 499) == (None, 0)
    assert lib.memory_decompress_members(buf[:-5], len(want)) == (None, 0)                 # the last member cut off
    assert lib.memory_decompress_members(b"", 10) == (None, 0)                             # an empty input


def check_cli(cli, tmp_path):
    parts = [text(5000, 80), text(100, 81), text(70000, 82)[:65280]]
    buf = b"".join(bgzf(p) for p in parts)
    src, dst = os.path.join(str(tmp_path), "three.gz"), os.path.join(str(tmp_path), "three.out")
    with open(src, "wb") as f:
        f.write(buf)
    r = subprocess.run([cli, "-x", "-m", "-v", "-f", "gzip", src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(dst, "rb").read() == gzip.decompress(buf) == b"".join(parts)
    assert "3 members" in r.stdout and "rewalked" in r.stdout, r.stdout
    mixed = buf + gzip.compress(parts[1], 6, mtime=0)   # the whole file does not index: the buffer grows
    with open(src, "wb") as f:
        f.write(mixed)
    r = subprocess.run([cli, "-x", "-m", "-f", "gzip", src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and open(dst, "rb").read() == gzip.decompress(mixed), r.stdout + r.stderr
    r = subprocess.run([cli, "-x", "-f", "gzip", src, dst], capture_output=True, text=True, timeout=120)   # plain -x: one member, as before
    assert r.returncode != 0 and open(dst, "rb").read() == b""
    r = subprocess.run([cli, "-x", "-m", "-f", "zlib", src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0, "-m is for gzip"


def check_bad_arguments(lib):
    buf = bgzf(text(100, 90)) + EOF_MARKER
    src = np.frombuffer(buf, dtype=np.uint8).copy()
    dst = np.zeros(200, dtype=np.uint8)
    n = len(src)
    f = lib.L.zultra_hip_index_members
    assert lib.index_members(src, n, 2)[0] == 0
    assert lib.index_members(None, n, 2)[0] == -1                   # src NULL
    assert lib.index_members(src, 0, 2)[0] == -1                    # src_size 0
    assert lib.index_members(src, n, 2, device=-1)[0] == -1
    assert lib.index_members(src, n, 2, device=lib.device_count())[0] == -1
    assert f(0, src.ctypes.data, n, 0, None, 3, None, None) == -1   # res NULL
    res = type(lib.index_members(src, n, 2)[1])()
    assert f(0, src.ctypes.data, n, 0, None, 3, ctypes.byref(res), None) == -1   # items NULL with cap 3
    assert lib.inflate_file(src, n, dst, 200, 2)[0] == 0 and dst[:100].tobytes() == text(100, 90)
    dst[:] = 0
    assert lib.inflate_file(None, n, dst, 200, 2)[0] == -1
    assert lib.inflate_file(src, 0, dst, 200, 2)[0] == -1
    assert lib.inflate_file(src, n, None, 200, 2)[0] == -1
    assert lib.inflate_file(src, n, dst, 200, 2, device=-1)[0] == -1
    assert lib.inflate_file(src, n, dst, 200, 2, device=lib.device_count())[0] == -1
    g = lib.L.zultra_hip_inflate_file
    assert g(0, src.ctypes.data, n, 0, dst.ctypes.data, 200, 0, None, None, 0, None) == -1   # res NULL
    rc, r, mem, _ = lib.inflate_file(src, n, dst, 200, 1)            # room for one result, two members
    assert rc == -1 and r.stop == 4 and r.members == 2
    rc, r, mem, _ = lib.inflate_file(src, n, dst, 99, 2)
    assert rc == -1 and r.stop == 4 and r.out_size == 100
    assert not dst.any(), "a refused call has written"
    assert lib.memory_decompress_members(buf, 100) == (text(100, 90), 2)   # (sets the prototype)
    h = lib.L.zultra_memory_decompress_members
    assert h(None, 10, dst.ctypes.data, 200, None) == h(src.ctypes.data, 0, dst.ctypes.data, 200, None) == h(src.ctypes.data, n, None, 200, None) == 2 ** 64 - 1
    assert lib.memory_decompress_members(buf, 100) == (text(100, 90), 2)
