"""Shared by tests/test_unzip_emu.py (CPU emulator build) and tests/test_unzip_gpu.py (product library on the MI355X): the archives, the runners and the
checks of ZIP archives READ on the device — zh_uz_tiles, zh_uz_resolve, zh_uz_entries, zh_uz_locals and zh_uz_copy of zultra_amd/csrc/zh_unzip.h, the ZIP
form of zh_check_members, zultra_hip_zip_index, zultra_hip_unzip, zultra_zip_find_end, zultra_memory_decompress_zip and the tool's -x -a.
The expectation never comes from the code under test. For the directory the yardstick is `walk` below, the serial walk of exactly the probe rule DESIGN.md
3.14 states, and `expected_tiles`, which tiles the chain enters and which of them start from a wrong guess; for the bytes Python's zipfile / zlib; for the
reasons, which field a hand-made struct.pack archive lies in. The tile size comes from the environment (ZULTRA_HIP_INDEX_TILE) and the grid cap too
(ZULTRA_HIP_GRID_CAP), so every value of either but the default runs in a process of its own (inflate_file_cases.run_child)."""
import binascii
import ctypes as C
import io
import os
import struct
import subprocess
import zipfile
import zlib

import numpy as np

import frame_member_cases as M
import inflate_file_cases as F
import verify_cases as V
import zip_cases as Z
from inflate_cases import CANARY_BYTE, device_read

SIG_C, SIG_L, SIG_E = b"PK\x01\x02", b"PK\x03\x04", b"PK\x05\x06"
TILES = F.TILES
DEFAULT_TILE = 16 * 1024   # ZH_UZ_TILE: a directory's default, where the gzip index's is 256 KiB
PAD = 64   # canary bytes around a destination and around a dirent array
UNSUPPORTED, BAD_FRAME, BAD_CHECK, BAD_SIZE, STREAM_END, DST_FULL = 17, 14, 15, 16, 12, 13
DIRENT_FIELDS = ("central_at", "local_off", "dst_off", "comp_size", "size", "crc32", "name_len", "method", "flags", "extra_len", "comment_len")


def tile_size():
    """The tile size of this process, as the library reads it."""
    t = int(os.environ.get("ZULTRA_HIP_INDEX_TILE", "0") or 0)
    return t if t >= 32 else DEFAULT_TILE


# ---- the yardstick: the serial walk ------------------------------------------------------------------------------------------------------------------
def probe(buf, D1, p):
    """-> (None, length) where a record starts at p, else (stop kind, 0)."""
    if p == D1:
        return 0, 0
    if D1 - p < 46 or buf[p: p + 4] != SIG_C:
        return 1, 0
    n, m, k = struct.unpack_from("<HHH", buf, p + 28)
    if p + 46 + n + m + k > D1:
        return 2, 0
    return None, 46 + n + m + k


def walk(buf, D0, D1):
    """-> (dirents as tuples in DIRENT_FIELDS' order, stop kind, stop position, sum of the sizes)."""
    buf = bytes(buf)
    p, out, ents = D0, 0, []
    while True:
        kind, L = probe(buf, D1, p)
        if kind is not None:
            return ents, kind, p, out
        _, _, flags, method, _, _, crc, comp, size, n, m, k, _, _, _, off = struct.unpack_from("<HHHHHHIIIHHHHHII", buf, p + 4)
        ents.append((p, off, out, comp, size, crc, n, method, flags, m, k))
        out += size
        p += L


def first_candidate(buf, D1, lo, hi):
    """The first position in [lo, hi) that starts a record, or None: a tile's guess."""
    p = lo
    while True:
        p = buf.find(SIG_C, p, hi + 3)
        if p < 0 or p >= hi:
            return None
        if probe(buf, D1, p)[0] is None:
            return p
        p += 1


def expected_tiles(buf, D0, D1, T, addr=0):
    """The three passes on paper -> dict: tiles the chain enters, those of them whose guess is not the chain's entry, whether a record straddles a tile end,
    whether the chain jumps over whole tiles, and whether the signature of a tile's guess lies across a lane's 16-byte window / across the 1024-byte round of
    a wave (addr: the address of buf[0])."""
    buf = bytes(buf)
    ents, stop, at, _ = walk(buf, D0, D1)
    chain = [e[0] for e in ents] + [at]   # (at: the stop position, D1 for a complete chain)
    facts = dict(tiles=0, rewalked=0, jumped=False, across16=False, across1024=False)
    facts["straddles"] = any((a - D0) // T != (b - 1 - D0) // T for a, b in zip(chain, chain[1:]))
    i, last = 0, -1
    while chain[i] < D1:
        e = chain[i]
        k = (e - D0) // T
        lo = D0 + k * T
        end = lo + T if D1 - lo > T else D1 + 1
        guess = D0 if k == 0 else first_candidate(buf, D1, lo, min(lo + T, D1))
        facts["tiles"] += 1
        facts["rewalked"] += guess != e
        facts["jumped"] |= k > last + 1
        last = k
        if k and guess is not None:
            off = guess - lo + ((addr + lo) & 15)   # from the start of the scan's first window, which is 16-byte aligned in memory
            facts["across16"] |= off % 16 >= 13
            facts["across1024"] |= off % 1024 >= 1021
        while i < len(ents) and chain[i] < end:   # the walk from e: on to the first position at or behind the tile's end, or to the stop
            i += 1
        if chain[i] < end:
            break
    return facts


def end_of(buf, comment_len=0, prefix=0):
    """Where the test itself put the directory: (D0, size) from the end record it knows to stand comment_len + 22 bytes in front of the end."""
    size, off = struct.unpack_from("<II", buf, len(buf) - 22 - comment_len + 12)
    return prefix + off, size


# ---- placing buffers -----------------------------------------------------------------------------------------------------------------------------------
def place(lib, buf, lead=0):
    """A device copy of buf whose first byte stands `lead` bytes behind an allocation's start -> (the DeviceCopy, the pointer)."""
    held = V.DeviceCopy(lib, np.frombuffer(b"\xee" * lead + bytes(buf) + b"\xee" * 7, dtype=np.uint8).copy())
    return held, held.ptr + lead


def host(buf):
    return np.frombuffer(bytes(buf) + b"\0", dtype=np.uint8).copy()[:-1]


def rows(dirents):
    return [tuple(int(d[f]) for f in DIRENT_FIELDS) for d in dirents]


# ---- 1: the index equals the serial walk -----------------------------------------------------------------------------------------------------------------
def tlv(data, tag=0x7a7a):
    """One well-formed extra subfield (zipfile refuses extras that are not a chain of them)."""
    return struct.pack("<HH", tag, len(data)) + data


DECOY_RECORD = SIG_C + struct.pack("<HHHHHHIIIHHHHHII", 20, 20, 0, 0, 0, 0x21, 0x11111111, 7, 9, 0, 0, 0, 0, 0, 0, 5)   # complete and plausible: n = m = k = 0


def index_archive(lead_name=1, decoys=True):
    """About 40 entries from zipfile: names of 1 .. 300 bytes, extras of 0 .. 5000, comments; with `decoys`, PK\\1\\2 inside names, comments and extras and
    a complete 46-byte record inside an extra. One record is sized so that the next starts 1010 bytes into a tile of 4096: behind the first round of that
    tile's scan, its signature across the round's end for three of the sixteen source alignments. lead_name: the first entry's name length, which moves
    the directory's start. -> the archive."""
    rs = np.random.RandomState(4)
    specs = []
    for i in range(40):
        n = [lead_name, 300, 1, 2, 17, 255][i] if i < 6 else int(rs.randint(3, 60))
        name = ("%02d" % i + "n" * 300)[:n] if n >= 2 else "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"[i]
        m = [0, 5000, 9, 1100, 0, 2500][i] if i < 6 else int(rs.choice([0, 0, 4, 40, 300, 700]))
        extra = tlv(bytes(rs.randint(0, 256, size=m - 4).astype(np.uint8)).replace(b"PK", b"pk")) if m >= 4 else b""
        comment = bytes(rs.randint(97, 123, size=int(rs.choice([0, 0, 3, 30, 200]))).astype(np.uint8))
        if decoys and i % 5 == 2:
            name = name[:1] + "PK\x01\x02" + name[1:]
            comment = comment[:2] + SIG_C + comment[2:]
        if decoys and i % 7 == 3:
            extra += tlv(b"\0" * (i % 5) + DECOY_RECORD + b"tail" * (i % 3))
        if decoys and i % 7 == 5:
            extra += tlv(SIG_C + bytes(rs.randint(0, 4, size=50).astype(np.uint8)))   # small lengths: a "record" that fits the directory
        specs.append([name, extra, comment, F.text(5 + 3 * i, i), zipfile.ZIP_DEFLATED if i & 1 else zipfile.ZIP_STORED])
    # the steering record: a filler comment that ends 1010 bytes into a tile of 4096 (positions relative to the directory's start)
    pos = [0]
    for name, extra, comment, _, _ in specs:
        pos.append(pos[-1] + 46 + len(name.encode()) + len(extra) + len(comment))
    s = 20
    target = 4096 * (pos[s] // 4096 + 1) + 1010
    specs[s][2] = b"\x55" * (target - pos[s] - 46 - len(specs[s][0].encode()) - len(specs[s][1]))   # (the comment: it stands in the directory only)
    out = io.BytesIO()
    with zipfile.ZipFile(out, "w") as z:
        for name, extra, comment, data, method in specs:
            info = zipfile.ZipInfo(name)
            info.extra, info.comment, info.compress_type = extra, comment, method
            z.writestr(info, data)
    buf = out.getvalue()
    with zipfile.ZipFile(io.BytesIO(buf)) as z:   # zipfile still opens it, decoys and all
        assert z.testzip() is None and len(z.infolist()) == 40 and len(z.infolist()[0].filename) == lead_name
    return buf


def check_index(lib, name, buf, D0, size, lead=0, on_device=True, T=None):
    """zultra_hip_zip_index over the directory buf[D0 .. D0 + size): dirents and totals are the walker's, tiles and tiles_rewalked what the three passes
    give on paper; the query form (dirents NULL) agrees. -> (the result, the facts)."""
    want, stop, at, out = walk(buf, D0, D0 + size)
    held, src = place(lib, buf, lead) if on_device else (None, host(buf))
    facts = None
    try:
        rc, res, dirents, _ = lib.zip_index(src, len(buf), D0, size, len(want) + 1)
        got = (res.entries, res.stop, res.dir_used, res.out_size)
        assert rc == 0 and got == (len(want), stop, at - D0, out), (name, rc, got, (len(want), stop, at - D0, out))
        assert rows(dirents) == want, (name, [(a, b) for a, b in zip(rows(dirents), want) if a != b][:2])
        if T:
            facts = expected_tiles(buf, D0, D0 + size, T, src if on_device else 0)
            assert (res.tiles, res.tiles_rewalked) == (facts["tiles"], facts["rewalked"]), (name, T, res.tiles, res.tiles_rewalked, facts)
        rc, q, _, _ = lib.zip_index(src, len(buf), D0, size, 0)
        assert rc == 0 and (q.entries, q.stop, q.dir_used, q.out_size, q.tiles, q.tiles_rewalked) == got + (res.tiles, res.tiles_rewalked), name
    finally:
        if held:
            held.free()
    return res, facts


def check_index_tiles(lib):
    """Case 1 under the tile size of this process: the decoy archive at every source address mod 16, its directory starting at every address mod 16 (the
    first entry's name length), and the archive without decoys. -> the number of index runs."""
    T = tile_size()
    seen = dict(straddles=False, jumped=False, across16=False, across1024=False, rewalked=0)
    runs = 0
    buf = index_archive()
    D0, size = end_of(buf)
    assert 8000 < size < 40000 and max(e[9] for e in walk(buf, D0, D0 + size)[0]) >= 5000
    starts = set()
    for lead in range(16):
        res, facts = check_index(lib, "decoys lead %d" % lead, buf, D0, size, lead=lead, T=T)
        for k in seen:
            seen[k] = seen[k] + facts[k] if k == "rewalked" else seen[k] or facts[k]
        runs += 1
    for lead_name in range(2, 18):
        b = index_archive(lead_name)
        d0, sz = end_of(b)
        starts.add(d0 % 16)
        check_index(lib, "decoys name %d" % lead_name, b, d0, sz, lead=0, T=T)
        runs += 1
    starts.add(D0 % 16)
    assert starts == set(range(16)), sorted(starts)
    check_index(lib, "decoys from the host", buf, D0, size, on_device=False, T=T)
    plain = index_archive(decoys=False)
    check_index(lib, "no decoys", plain, *end_of(plain), lead=5, T=T)
    if T in TILES:
        assert seen["straddles"] and seen["across16"], (T, seen)
        assert (seen["jumped"] and seen["rewalked"] > 0) or T == 4096, (T, seen)
        assert seen["across1024"] == (T == 4096), (T, seen)
    else:
        assert T == DEFAULT_TILE < size < 2 * T and seen["straddles"]   # two tiles, a record across their border: held to the paper model above
    return runs + 2


# ---- archives by hand ------------------------------------------------------------------------------------------------------------------------------------
class Entry:
    """One entry of a hand-made archive. `raw`: the bytes that stand behind the local header (default: data stored, or deflated at `level`). Every field of
    the two headers can lie: c_* for the central record, l_* for the local header (default: the truth)."""

    def __init__(self, name, data=b"", method=8, level=6, raw=None, extra=b"", l_extra=None, comment=b"", flags=0, **lies):
        self.name = name if isinstance(name, bytes) else name.encode()
        self.data = bytes(data)
        self.method = method
        self.raw = bytes(raw) if raw is not None else (self.data if method == 0 else F.deflated(self.data, level))
        self.extra, self.l_extra, self.comment, self.flags = extra, extra if l_extra is None else l_extra, comment, flags
        self.lies = lies

    def field(self, where, key, truth):
        return self.lies.get(where + "_" + key, self.lies.get(key, truth))

    def local(self):
        name = self.field("l", "name", self.name)
        return SIG_L + struct.pack("<HHHHHIIIHH", 20, self.field("l", "flags", self.flags), self.field("l", "method", self.method), 0, 0x21, self.field("l", "crc", binascii.crc32(self.data)),
                                   self.field("l", "comp", len(self.raw)), self.field("l", "size", len(self.data)), self.field("l", "name_len", len(name)), len(self.l_extra)) + name + self.l_extra

    def central(self, local_off):
        return SIG_C + struct.pack("<HHHHHHIIIHHHHHII", 20, 20, self.field("c", "flags", self.flags), self.field("c", "method", self.method), 0, 0x21, self.field("c", "crc", binascii.crc32(self.data)),
                                   self.field("c", "comp", len(self.raw)), self.field("c", "size", len(self.data)), len(self.name), len(self.extra), len(self.comment), 0, 0, 0,
                                   self.field("c", "off", local_off)) + self.name + self.extra + self.comment


def hand_archive(entries, base=0, directory_first=False):
    """-> (the archive without end records, D0, size of the directory, [position of every local header]). base: what the central records' offsets count from
    on top of the position in the buffer (the caller passes local_delta = -base). directory_first: the directory in front of the local part."""
    sizes = [len(e.local()) + len(e.raw) for e in entries]
    dir_size = sum(46 + len(e.name) + len(e.extra) + len(e.comment) for e in entries)
    at, offs = dir_size if directory_first else 0, []
    for s in sizes:
        offs.append(at)
        at += s
    local = b"".join(e.local() + e.raw for e in entries)
    central = b"".join(e.central(o + base) for e, o in zip(entries, offs))
    assert len(central) == dir_size
    return (central + local, 0, dir_size, offs) if directory_first else (local + central, len(local), dir_size, offs)


def want_results(lib, buf, D0, size, local_delta):
    """What a sound archive's results must be, from the directory and the local headers as struct reads them: reason 0, out_size = size, src_used =
    comp_size, head_size, check = the CRC-32 of zlib's / the stored bytes; blocks from zultra_hip_inflate_streams over the same streams (0 for stored).
    -> ([(reason, blocks, out_size, src_used, head_size, check)], [the bytes of every entry])."""
    ents = walk(buf, D0, D0 + size)[0]
    out, datas, items, where, total = [], [], [], [], 0
    for (p, off, dst_off, comp, sz, crc, n, method, flags, m, k) in ents:
        lp = off + local_delta
        ln, lm = struct.unpack_from("<HH", buf, lp + 26)
        raw = bytes(buf[lp + 30 + ln + lm: lp + 30 + ln + lm + comp])
        data = raw if method == 0 else zlib.decompressobj(-15).decompress(raw)
        assert len(data) == sz and binascii.crc32(data) == crc, "the test's archive is not sound"
        datas.append(data)
        out.append([0, 0, sz, comp, 30 + ln + lm, crc])
        if method == 8:
            items.append((lp + 30 + ln + lm, comp, total, sz))
            where.append(len(out) - 1)
        total += sz
    if items:
        rc, res, _ = lib.inflate_streams(host(buf), len(buf), np.zeros(max(total, 1), dtype=np.uint8), total, items)
        assert rc == 0
        for w, r in zip(where, res):
            out[w][1] = int(r["blocks"])
    return [tuple(o) for o in out], datas


def run_unzip(lib, buf, D0, size, local_delta=0, on_device=True, src_lead=0, dst_lead=0, short=0, room=None, src_size=None, cap=None):
    """zultra_hip_unzip with exactly the room the walker counts, less `short`, canaries around the destination.
    -> (rc, index result, dirents, [results as tuples], the destination's bytes)."""
    ents, stop, at, out = walk(buf, D0, D0 + size)
    room = (out if room is None else room) - short
    cap = len(ents) if cap is None else cap
    n = len(buf) if src_size is None else src_size
    if on_device:
        s, sp = place(lib, buf, src_lead)
        d = V.DeviceCopy(lib, np.full(dst_lead + PAD + room + PAD, CANARY_BYTE, dtype=np.uint8))
        try:
            rc, res, dirents, results, ms = lib.unzip(sp, n, D0, size, local_delta, d.ptr + dst_lead + PAD, room, cap)
            back = device_read(lib, d, dst_lead + 2 * PAD + room).copy()[dst_lead:]
        finally:
            s.free()
            d.free()
    else:
        back = np.full(2 * PAD + room, CANARY_BYTE, dtype=np.uint8)
        rc, res, dirents, results, ms = lib.unzip(host(buf)[:n], n, D0, size, local_delta, back[PAD:], room, cap)
    assert (back[:PAD] == CANARY_BYTE).all() and (back[PAD + room:] == CANARY_BYTE).all(), "a canary around the destination was written"
    assert len(ms) == 5
    return rc, res, dirents, [tuple(int(v) for v in r) for r in results], back[PAD: PAD + room]


def check_sound(lib, name, buf, D0, size, local_delta=0, **kw):
    """A sound archive: every byte and every result field, and the dirents."""
    want, datas = want_results(lib, buf, D0, size, local_delta)
    rc, res, dirents, results, back = run_unzip(lib, buf, D0, size, local_delta, **kw)
    ents, stop, at, out = walk(buf, D0, D0 + size)
    assert rc == 0 and (res.entries, res.stop, res.out_size, res.dir_used) == (len(ents), 0, out, size), (name, rc, res.entries, res.stop, res.out_size)
    if kw.get("cap") != 0:   # (0: dirents and results passed as NULL)
        assert rows(dirents) == ents, name
        assert results == want, (name, [(i, a, b) for i, (a, b) in enumerate(zip(results, want)) if a != b][:3])
    assert back.tobytes() == b"".join(datas), name
    return len(ents)


# ---- 2: stops ------------------------------------------------------------------------------------------------------------------------------------------
def check_stops(lib):
    entries = [Entry("e%d" % i + "x" * i, F.text(40 + i, i), method=8 if i & 1 else 0, extra=tlv(b"e" * i), comment=b"c" * (i % 3)) for i in range(7)]
    buf, D0, size, _ = hand_archive(entries)
    ents = walk(buf, D0, D0 + size)[0]
    assert len(ents) == 7
    kinds = set()
    cases = [("whole", buf, size, 0)]
    for j in (0, 3, 6):
        rel = ents[j][0] - D0
        cases.append(("cut %d: fewer than 46 bytes left" % j, buf, rel + 30, 1))
        cases.append(("cut %d: the lengths overrun" % j, buf, rel + 46 + 1, 2))
        bad = bytearray(buf)
        bad[ents[j][0] + 2] ^= 4
        cases.append(("signature %d" % j, bytes(bad), size, 1))
    for name, b, sz, kind in cases:
        res, _ = check_index(lib, name, b, D0, sz, lead=len(name) % 16, T=tile_size())
        assert res.stop == kind, (name, res.stop)
        kinds.add(res.stop)
        if kind:   # a stop of 1 or 2 is an error of zultra_hip_unzip: nothing is decoded
            rc, res, dirents, results, back = run_unzip(lib, b, D0, sz, room=300)
            assert rc == -1 and res.stop == kind and (back == CANARY_BYTE).all(), name
    assert kinds == {0, 1, 2}
    # cap one short: 4, and nothing written — the dirents stand between canaries
    held, src = place(lib, buf, 3)
    try:
        arr = np.full(PAD + 48 * 7 + PAD, CANARY_BYTE, dtype=np.uint8)
        res = type(lib.zip_index(src, len(buf), D0, size, 0)[1])()
        f = lib.L.zultra_hip_zip_index
        assert f(0, src, len(buf), 1, D0, size, arr.ctypes.data + PAD, 6, C.byref(res), None) == -1 and (res.stop, res.entries, res.out_size) == (4, 7, sum(e[4] for e in ents))
        assert (arr == CANARY_BYTE).all(), "a refused call has written dirents"
        assert f(0, src, len(buf), 1, D0, size, arr.ctypes.data + PAD, 7, C.byref(res), None) == 0 and res.stop == 0
        assert (arr[:PAD] == CANARY_BYTE).all() and (arr[PAD + 48 * 7:] == CANARY_BYTE).all() and not (arr[PAD: PAD + 48 * 7] == CANARY_BYTE).all()
    finally:
        held.free()
    for dev in (True, False):
        rc, res, dirents, results, back = run_unzip(lib, buf, D0, size, on_device=dev, cap=6)
        assert rc == -1 and (res.stop, res.entries) == (4, 7) and (back == CANARY_BYTE).all()
        rc, res, dirents, results, back = run_unzip(lib, buf, D0, size, on_device=dev, short=1)   # one byte short of room: the same
        assert rc == -1 and (res.stop, res.out_size) == (4, sum(e[4] for e in ents)) and (back == CANARY_BYTE).all()
    # arguments
    assert lib.zip_index(host(buf), len(buf), D0, size + 1, 0)[0] == -1 and lib.zip_index(host(buf), len(buf), len(buf) + 1, 0, 0)[0] == -1   # a directory outside src
    assert lib.zip_index(None, len(buf), D0, size, 0)[0] == -1 and lib.zip_index(host(buf), 0, 0, 0, 0)[0] == -1
    assert lib.zip_index(host(buf), len(buf), D0, size, 0, device=lib.device_count())[0] == -1
    rc, res, _, _ = lib.zip_index(host(buf), len(buf), D0, 0, 0)   # an empty directory is a complete chain
    assert rc == 0 and (res.entries, res.stop, res.tiles) == (0, 0, 0)
    return len(cases)


# ---- 3: what other producers write -------------------------------------------------------------------------------------------------------------------------
class Unseekable(io.RawIOBase):
    """A stream zipfile can only append to: flag bit 3, sizes 0 in the local headers, data descriptors behind the data."""

    def __init__(self):
        self.out = bytearray()

    def writable(self):
        return True

    def write(self, b):
        self.out += bytes(b)
        return len(b)


def foreign_entries(noise_size, many):
    out = [("stored.txt", F.text(700, 1), zipfile.ZIP_STORED, None, b"", b""), ("level1.txt", F.text(3000, 2), zipfile.ZIP_DEFLATED, 1, b"", b"a comment"),
           ("level6.txt", F.text(5000, 3), zipfile.ZIP_DEFLATED, 6, tlv(b"extra bytes"), b""), ("dir/level9.txt", F.text(4000, 4), zipfile.ZIP_DEFLATED, 9, tlv(b"x" * 33), b"both"),
           ("empty", b"", zipfile.ZIP_STORED, None, b"", b""), ("dir/", b"", zipfile.ZIP_STORED, None, b"", b""), ("deflated empty", b"", zipfile.ZIP_DEFLATED, 6, b"", b""),
           ("grüße/日本語.txt", F.text(333, 5), zipfile.ZIP_DEFLATED, 6, b"", "Kommentar ä".encode()), ("noise.bin", F.noise(noise_size, 6), zipfile.ZIP_STORED, None, b"", b""),
           ("zeros", bytes(9000), zipfile.ZIP_DEFLATED, 6, b"", b""), ("one", b"1", zipfile.ZIP_STORED, None, b"", b"")]
    for i in range(many):
        out.append(("many/%04d%s" % (i, "y" * (i % 23)), F.text(30 + i % 61, 100 + i), zipfile.ZIP_DEFLATED if i % 3 else zipfile.ZIP_STORED, 6, b"", b""))
    return out


def foreign_archives(noise_size, many):
    """-> [(name, archive)]: a seekable one, with one entry written with force_zip64 (a ZIP64 extra in its LOCAL header only), and an unseekable one."""
    entries = foreign_entries(noise_size, many)
    seek, stream = io.BytesIO(), Unseekable()
    for target in (seek, stream):
        with zipfile.ZipFile(target, "w") as z:
            for name, data, method, level, extra, comment in entries:
                info = zipfile.ZipInfo(name)
                info.extra, info.comment, info.compress_type = extra, comment, method
                z.writestr(info, data, compresslevel=level)
            if target is seek:
                with z.open(zipfile.ZipInfo("forced zip64"), "w", force_zip64=True) as f:
                    f.write(F.text(1234, 7))
    a, b = seek.getvalue(), bytes(stream.out)
    la = zipfile.ZipFile(io.BytesIO(a)).getinfo("forced zip64").header_offset
    assert struct.unpack_from("<HH", a, la + 26) == (12, 20) and a[la + 42: la + 46] == b"\x01\x00\x10\x00", "no ZIP64 extra in the local header"
    lb = zipfile.ZipFile(io.BytesIO(b)).getinfo("level1.txt")
    assert lb.flag_bits & 8 and struct.unpack_from("<III", b, lb.header_offset + 14) == (0, 0, 0), "no data descriptor"
    for buf in (a, b):
        z = zipfile.ZipFile(io.BytesIO(buf))
        assert z.testzip() is None and [z.read(i) for i in z.infolist()][:len(entries)] == [e[1] for e in entries]
    return [("seekable", a), ("unseekable", b)]


def check_foreign(lib, noise_size, many, full=True):
    n = 0
    for name, buf in foreign_archives(noise_size, many):
        D0, size = end_of(buf)
        n += check_sound(lib, name, buf, D0, size, src_lead=3, dst_lead=5)
        if full:
            check_sound(lib, name + " host", buf, D0, size, on_device=False)
            check_sound(lib, name + " no results", buf, D0, size, cap=0)
    return n


# ---- 4: stored-copy alignment ----------------------------------------------------------------------------------------------------------------------------
def alignment_archive():
    """Stored entries whose data start and whose destination together take all 16 x 16 residue pairs mod 16: the sizes move the destination on, the name
    lengths the data (zip_cases.alignment_grid steers the writer's the same way). -> (archive, D0, directory size, the pairs in entry order)."""
    sizes = [0, 1, 15, 16, 17, 31, 33, 300, 257]
    missing = {(s, d) for s in range(16) for d in range(16)}
    entries, pairs, at, dst, i = [], [], 0, 0, 0
    while (missing or i < len(sizes)) and i < 2000:
        s = min((p[0] for p in missing if p[1] == dst % 16), default=0)
        n = 1 + (s - (at + 30 + 1)) % 16 + (16 if i % 5 == 0 else 0)
        # the size whose successor's destination residue still misses most pairs; ties go round the list
        size = sizes[i] if i < len(sizes) else max(sizes[i % len(sizes):] + sizes[:i % len(sizes)], key=lambda z: sum(1 for p in missing if p[1] == (dst + z) % 16 and p != (s, dst % 16)))
        entries.append(Entry(("%03d" % i + "n" * 40)[:n] if n >= 3 else "ab"[:n], b"" if not size else F.noise(size, i) if i & 1 else F.text(size, i), method=0))
        pair = ((at + 30 + n) % 16, dst % 16)
        pairs.append(pair)
        missing.discard(pair)
        at += 30 + n + size
        dst += size
        i += 1
    assert not missing and {len(e.data) for e in entries} == set(sizes), (len(missing), i)
    return hand_archive(entries)[:3] + (pairs,)


def check_copy_alignment(lib):
    """With the source and the destination at allocation starts (16-byte aligned) the pairs are address residues; and once more with both moved."""
    buf, D0, size, pairs = alignment_archive()
    assert len(set(pairs)) == 256
    n = check_sound(lib, "alignment grid", buf, D0, size)
    check_sound(lib, "alignment grid, moved", buf, D0, size, src_lead=7, dst_lead=11)
    return n


# ---- 5: reasons ------------------------------------------------------------------------------------------------------------------------------------------
def check_reasons(lib):
    """One hand-made archive per cause: the entry in question gets exactly that reason, its neighbours 0 and their bytes."""
    a, c = F.text(900, 31), F.noise(500, 33)
    v = F.text(1200, 32)
    stored_deflate = F.deflated(v, 0)   # stored blocks: a flipped payload bit decodes, to other bytes
    assert len(stored_deflate) == len(v) + 5

    def flip(raw, at):
        b = bytearray(raw)
        b[at] ^= 0x10
        return bytes(b)

    causes = [("method 9", Entry("v", v, method=9, raw=F.deflated(v)), UNSUPPORTED), ("flag bit 0", Entry("v", v, flags=1), UNSUPPORTED), ("flag bit 6", Entry("v", v, flags=0x40), UNSUPPORTED),
              ("flag bit 5", Entry("v", v, flags=0x20), UNSUPPORTED), ("comp_size 0xFFFFFFFF", Entry("v", v, c_comp=0xFFFFFFFF), UNSUPPORTED),
              ("local_off 0xFFFFFFFF", Entry("v", v, c_off=0xFFFFFFFF), UNSUPPORTED),
              ("local signature", Entry("v", v), BAD_FRAME), ("local name differs by one byte", Entry("name", v, l_name=b"nbme"), BAD_FRAME),
              ("local name differs by length", Entry("name", v, l_name=b"name2"), BAD_FRAME), ("local method differs", Entry("v", v, l_method=0), BAD_FRAME),
              ("local_off outside src", Entry("v", v, c_off=0x7FFFFFF0), BAD_FRAME), ("stored with comp_size != size", Entry("v", v, method=0, c_size=len(v) - 1), BAD_FRAME),
              ("a deflate stream cut short", Entry("v", v, c_comp=len(F.deflated(v)) - 3), STREAM_END), ("size one too small", Entry("v", v, c_size=len(v) - 1), DST_FULL),
              ("size one too large", Entry("v", v, c_size=len(v) + 1), BAD_SIZE), ("a data bit flipped, stored", Entry("v", v, method=0, raw=flip(v, 77)), BAD_CHECK),
              ("a data bit flipped, deflated", Entry("v", v, raw=flip(stored_deflate, 5 + 77)), BAD_CHECK), ("central CRC wrong", Entry("v", v, c_crc=binascii.crc32(v) ^ 1), BAD_CHECK),
              ("local CRC and sizes wrong: not looked at", Entry("v", v, l_crc=5, l_comp=6, l_size=7), 0), ("flag bit 3 and 11: not looked at", Entry("v", v, flags=0x808), 0)]
    seen = set()
    for k, (what, victim, reason) in enumerate(causes):
        entries = [Entry("first", a), victim, Entry("last", c, method=0)]
        buf, D0, size, offs = hand_archive(entries)
        if what == "local signature":
            buf = flip(buf, offs[1] + 1)
        for dev in (True, False):
            rc, res, dirents, results, back = run_unzip(lib, buf, D0, size, on_device=dev, src_lead=k % 16, dst_lead=(3 * k) % 16)
            got = [r[0] for r in results]
            assert got == [0, reason, 0] and rc == (1 if reason else 0), (what, dev, rc, got)
            assert back[:len(a)].tobytes() == a and back[len(back) - len(c):].tobytes() == c, (what, dev)
            if reason in (UNSUPPORTED, BAD_FRAME):
                assert results[1] == (reason, 0, 0, 0, 0, 0), (what, results[1])
                assert (back[len(a): len(back) - len(c)] == CANARY_BYTE).all(), what   # nothing of such an entry is written
            if reason == BAD_SIZE:
                assert results[1][2:4] == (len(v), len(F.deflated(v))) and results[1][5] == binascii.crc32(v), (what, results[1])
            if reason == BAD_CHECK:
                assert results[1][2] == len(v) and results[1][5] == binascii.crc32(back[len(a): len(a) + len(v)].tobytes()), (what, results[1])
            if reason == DST_FULL:
                assert results[1][2] <= len(v) - 1 and results[1][5] == 0, (what, results[1])
            if not dev and reason:   # of a host destination nothing but what entries wrote comes back
                written = results[1][2]
                assert (back[len(a) + written: len(back) - len(c)] == CANARY_BYTE).all(), what
        seen.add(reason)
    assert seen == {0, UNSUPPORTED, BAD_FRAME, STREAM_END, DST_FULL, BAD_SIZE, BAD_CHECK}
    # a size of 0xFFFFFFFF: the last entry, so that the others' destinations are not moved by it; the destination is SAID to be as large as the directory's
    # sum (device memory: nothing of the entry is written or summed)
    entries = [Entry("first", a), Entry("last", c, method=0), Entry("v", v, c_size=0xFFFFFFFF)]
    buf, D0, size, _ = hand_archive(entries)
    s, sp = place(lib, buf)
    d = V.DeviceCopy(lib, np.full(len(a) + len(c) + PAD, CANARY_BYTE, dtype=np.uint8))
    try:
        rc, res, dirents, results, _ = lib.unzip(sp, len(buf), D0, size, 0, d.ptr, len(a) + len(c) + 0xFFFFFFFF, 3)
        assert rc == 1 and [int(r["reason"]) for r in results] == [0, 0, UNSUPPORTED] and res.out_size == len(a) + len(c) + 0xFFFFFFFF
        back = device_read(lib, d, len(a) + len(c) + PAD)
        assert back[:len(a) + len(c)].tobytes() == a + c and (back[len(a) + len(c):] == CANARY_BYTE).all()
        rc, res, _, _, _ = lib.unzip(sp, len(buf), D0, size, 0, d.ptr, len(a) + len(c), 3)   # the zip-bomb gate: the sum is known before a byte is inflated
        assert rc == -1 and res.stop == 4
    finally:
        s.free()
        d.free()
    # data past the source's end: the directory in front, the victim's data last, the source one byte short
    entries = [Entry("first", a), Entry("last", c, method=0), Entry("v", v)]
    buf, D0, size, _ = hand_archive(entries, directory_first=True)
    for cut, reason in ((0, 0), (1, BAD_FRAME)):
        rc, res, dirents, results, back = run_unzip(lib, buf, D0, size, src_size=len(buf) - cut, src_lead=9)
        assert [r[0] for r in results] == [0, 0, reason] and back[:len(a) + len(c)].tobytes() == a + c, (cut, results)
    rc, res, dirents, results, back = run_unzip(lib, buf, D0, size, src_size=len(buf) - len(F.deflated(v)) - 30)   # ... and with the local header itself cut
    assert [r[0] for r in results] == [0, 0, BAD_FRAME]
    # a local header in front of the source after local_delta
    entries = [Entry("first", a), Entry("v", v, c_off=50), Entry("last", c, method=0)]
    buf, D0, size, _ = hand_archive(entries, base=100)
    rc, res, dirents, results, back = run_unzip(lib, buf, D0, size, local_delta=-100)
    assert [r[0] for r in results] == [0, BAD_FRAME, 0], results
    # two entries whose data ranges overlap: the second one's local header and data stand inside the first one's stored data
    inner = Entry("inner", F.text(300, 40))
    outer = Entry("outer", b"lead" + inner.local() + inner.raw + b"trail", method=0)
    buf, D0, size, offs = hand_archive([outer, Entry("x", a)])
    central = outer.central(0) + inner.central(30 + 5 + 4) + Entry("x", a).central(offs[1])
    buf = buf[:D0] + central
    assert check_sound(lib, "overlap", buf, D0, len(central)) == 3
    return len(causes)


# ---- 6: round trip without leaving the device ------------------------------------------------------------------------------------------------------------
def check_device_round_trip(lib, checker, scale):
    """A files batch with empty entries, and a batch of max-blocks with one in stored form, through zultra_hip_zip_members(base_off = 1000003) and back
    through zultra_hip_unzip reading the zip buffer where it stands: the output equals the inputs, and neither the stream buffer nor the zip buffer changes."""
    base_off = 1000003
    small = [F.text(400 * scale, 500), b"", F.noise(300, 501), F.text(1, 502), b"", b"", F.text(2000 * scale, 503), F.text(77, 504), b""]
    large = [F.text(8500 * scale, 505), F.noise(9000 * scale, 506), F.text(300, 507)]
    for kind, parts in (("files", small), ("max-blocks", large)):
        names = ["%s/%d" % (kind, i) + "x" * i for i in range(len(parts))]
        plain = b"".join(parts)
        ctx = lib.files_context(8191, len(parts)) if kind == "files" else lib.context(65536, len(parts))
        d = V.DeviceCopy(lib, np.full(len(plain) + PAD, CANARY_BYTE, dtype=np.uint8))
        try:
            live = [p for p in parts if len(p)]
            if kind == "files":
                Z.compress_files(ctx, live)
            else:
                M.compress(ctx, live)
            ent, local, central = Z.zipped(ctx, checker, parts, names, 32768 if kind == "files" else 65536, base_off=base_off)
            if kind == "max-blocks":
                assert int(ent[1]["comp_size"]) > len(parts[1])   # noise: stored blocks inside a method-8 entry
            ptr, central_at = ctx.zip_ptr()
            stream_before = ctx.stream_read(len(local) + 64).tobytes()
            zip_before = ctx.zip_read(central_at + len(central)).tobytes()
            rc, res, dirents, results, ms = lib.unzip(ptr, central_at + len(central), central_at, len(central), -base_off, d.ptr, len(plain), len(parts))
            assert rc == 0 and (res.entries, res.stop, res.out_size) == (len(parts), 0, len(plain)), (kind, rc, res.entries, res.stop, [int(r["reason"]) for r in results])
            back = device_read(lib, d, len(plain) + PAD)
            assert back[:len(plain)].tobytes() == plain and (back[len(plain):] == CANARY_BYTE).all(), kind
            for e, r, w, p in zip(ent, results, dirents, parts):
                assert (int(w["local_off"]), int(w["comp_size"]), int(w["size"]), int(w["crc32"]), int(w["method"])) == \
                       (int(e["local_off"]), int(e["comp_size"]), len(p), binascii.crc32(p) if p else 0, 8 if p else 0)
                assert (int(r["reason"]), int(r["out_size"]), int(r["src_used"]), int(r["check"])) == (0, len(p), int(e["comp_size"]), binascii.crc32(p) if p else 0)
            assert ctx.stream_read(len(stream_before)).tobytes() == stream_before and ctx.zip_read(len(zip_before)).tobytes() == zip_before, kind
        finally:
            d.free()
            ctx.close()


# ---- 7: the host API and the end records -----------------------------------------------------------------------------------------------------------------
def check_api_archive(lib, buf, names, parts, what):
    total = sum(len(p) for p in parts)
    got, info, n = lib.memory_decompress_zip(buf, total, len(parts))
    assert got == b"".join(parts) and n == len(parts), (what, None if got is None else len(got), n)
    at = 0
    for i, (name, p) in enumerate(zip(names, parts)):
        o = info[i]
        assert bytes(buf[int(o["nNameAt"]): int(o["nNameAt"]) + int(o["nNameLen"])]) == name, (what, i)
        assert (int(o["nSize"]), int(o["nOutOff"]), int(o["nCrc32"]), int(o["nStatus"])) == (len(p), at, binascii.crc32(p) if p else 0, 0), (what, i)
        at += len(p)
    size, info2, n2 = lib.memory_decompress_zip(buf, 0, len(parts), list_only=True)   # list only
    assert size == total and n2 == n and info2.tobytes() == info.tobytes(), what
    if total:
        got, info3, _ = lib.memory_decompress_zip(buf, total - 1, len(parts))               # the output one byte short
        assert got is None and [int(o["nSize"]) for o in info3] == [len(p) for p in parts], what
    got, info4, n4 = lib.memory_decompress_zip(buf, total, len(parts) - 1)                  # one info short
    assert got is None and n4 == len(parts) and len(info4) == len(parts) - 1, what
    return len(parts)


def check_host_api(lib, large_size, small_size):
    # the library's own archives: zip_cases' mixed and empty-entry inputs
    mixed = [F.text(100, 700), F.text(small_size // 2, 701), F.noise(50, 702), F.text(large_size, 703), F.noise(8192, 704), F.text(small_size, 705), F.text(1, 706)]
    mixed_names = Z.enc(["a.txt", "grüße/日本語.txt", "n" * 296 + ".bin", "big/one.txt", "big/two.txt", "z/last but one", "z/last"])
    empty = [b"", F.text(300, 710), b"", b"", F.text(77, 711), b"", F.text(large_size, 712), b"", F.text(20, 713), b""]
    empty_names = Z.enc(["empty first", "one.txt", "d/", "d/empty", "d/two.txt", "between/", "large.txt", "behind large", "three.txt", "empty last"])
    for what, parts, names in (("mixed", mixed, mixed_names), ("empty entries", empty, empty_names), ("only empty", [b"", b""], [b"x/", b"x/nothing"])):
        offs = np.concatenate([[0], np.cumsum([len(p) for p in parts])[:-1]])
        buf = lib.memory_compress_zip(b"".join(parts) + b"\0", [(int(o), len(p)) for o, p in zip(offs, parts)], names)
        assert buf is not None
        check_api_archive(lib, buf, names, parts, what)
    # zipfile's, behind a 45-byte prefix (a self-extractor's stub: the offsets do not count it) and with an archive comment that holds an end signature
    parts = [F.text(2000, 720), b"", F.noise(600, 721), F.text(50, 722)]
    names = [b"p/one", b"p/empty", b"p/noise", b"two"]
    out = io.BytesIO()
    with zipfile.ZipFile(out, "w", zipfile.ZIP_DEFLATED) as z:
        for name, p in zip(names, parts):
            z.writestr(name.decode(), p)
    plain = out.getvalue()
    check_api_archive(lib, b"#!stub" + b"s" * 39 + plain, names, parts, "prefix")
    assert zipfile.ZipFile(io.BytesIO(b"#!stub" + b"s" * 39 + plain)).testzip() is None
    comment = b"see " + SIG_E + b"\0" * 18 + b" above"   # a whole end record's worth inside the comment, whose comment length (0) does not reach the end
    for comment in (b"an archive comment", comment):   # (zipfile itself takes the last signature it finds, so only the first is held to it)
        with_comment = plain[:-2] + struct.pack("<H", len(comment)) + comment
        assert SIG_E in comment or zipfile.ZipFile(io.BytesIO(with_comment)).comment == comment
        check_api_archive(lib, with_comment, names, parts, "archive comment")
    # an end record whose count differs from the chain
    for delta in (-1, 1):
        bad = bytearray(plain)
        struct.pack_into("<HH", bad, len(bad) - 22 + 8, 4 + delta, 4 + delta)
        assert lib.memory_decompress_zip(bytes(bad), 4000, 8)[0] is None, delta
    # a damaged entry fails the call and says which
    bad = bytearray(plain)
    bad[30 + 5 + 40] ^= 1
    got, info, n = lib.memory_decompress_zip(bytes(bad), 4000, 8)
    assert got is None and n == 4 and int(info[0]["nStatus"]) != 0 and [int(o["nStatus"]) for o in info[1:]] == [0, 0, 0]
    assert lib.memory_decompress_zip(b"PK", 10, 1)[0] is None and lib.memory_decompress_zip(plain[:-1], 4000, 8)[0] is None


def check_find_end(lib):
    """zultra_zip_find_end against zip_cases.want_end_records, the writer's yardstick."""
    for n in (0, 1, 65535, 65536):
        for off, size, prefix in ((0, 46 * n, 0), (123456, 46 * n + 10, 0), (1000, 46 * n + 3, 45)):
            records = Z.want_end_records(n, off, size)
            assert len(records) == (98 if n > 65535 else 22)
            archive_size = prefix + off + size + len(records)
            lead = b"\xab" * min(300, archive_size - len(records))   # some of the directory in front, as a caller's tail holds
            # an archive comment; one with an end signature too close to the end to be a record; one with a whole record's worth whose own comment length
            # (0) does not reach the end
            for comment in (b"", b"has " + SIG_E + b" inside", b"see " + SIG_E + b"\0" * 18 + b" above"):
                tail = records[:-2] + struct.pack("<H", len(comment)) + comment
                end = lib.zip_find_end(lead + tail, archive_size + len(comment))
                assert end is not None, (n, off, size, prefix, comment)
                got = (end.nEntries, end.nCentralOff, end.nCentralSize, end.nPrefix, end.nZip64)
                assert got == (n, off, size, prefix, 1 if n > 65535 else 0), (n, off, size, prefix, comment, got)
            if n > 65535:
                assert lib.zip_find_end(records[56:], archive_size) is None                        # the locator, and its record not in the tail
                # the locator missing: the end record alone says 0xFFFF entries, which is what 65535 entries look like too (want_end_records(65535)): the
                # reader cannot tell, and zultra_memory_decompress_zip's count check can
                end = lib.zip_find_end(records[:56] + b"\0" * 20 + records[76:], archive_size)
                assert end is not None and (end.nEntries, end.nZip64) == (65535, 0)
                bad = bytearray(records)
                bad[56 + 16] = 2                                                                    # two disks in all
                assert lib.zip_find_end(bytes(bad), archive_size) is None
            for at, what in ((4, "this disk"), (6, "the directory's disk")):
                bad = bytearray(records)
                bad[len(records) - 22 + at] = 1
                assert lib.zip_find_end(bytes(bad), archive_size) is None, what
            assert lib.zip_find_end(records[-21:], archive_size) is None                           # a tail shorter than 22 bytes
    # a size or an offset of 0xFFFFFFFF with the locator missing
    for rec in (struct.pack("<IHHHHIIH", 0x06054b50, 0, 0, 3, 3, 0xFFFFFFFF, 10, 0), struct.pack("<IHHHHIIH", 0x06054b50, 0, 0, 3, 3, 10, 0xFFFFFFFF, 0)):
        assert lib.zip_find_end(b"\0" * 100 + rec, 1 << 33) is None
    assert lib.zip_find_end(Z.want_end_records(3, 100, 50), 100 + 50 + 22 - 1) is None           # a negative prefix
    assert lib.zip_find_end(b"\0" * 64, 64) is None                                             # no end record


def check_zip64_archive(lib):
    """The 65 537-entry archive of zip_cases.check_zip64_end read back: ZIP64 end records, and a directory of several default tiles."""
    n = 65537
    rs = np.random.RandomState(9)
    data = rs.randint(97, 123, size=8 * n).astype(np.uint8)
    names = [b"%05x" % i for i in range(n)]
    buf = lib.memory_compress_zip(data, [(8 * i, 8) for i in range(n)], names)
    assert buf is not None
    end = lib.zip_find_end(buf[-98:], len(buf))
    assert (end.nEntries, end.nCentralSize, end.nPrefix, end.nZip64) == (n, 51 * n, 0, 1)
    got, info, entries = lib.memory_decompress_zip(buf, 8 * n, n)
    assert got == data.tobytes() and entries == n and not info["nStatus"].any()
    rc, res, _, _ = lib.zip_index(host(buf), len(buf), end.nCentralOff, end.nCentralSize, 0)
    assert rc == 0 and (res.entries, res.stop, res.out_size) == (n, 0, 8 * n) and res.tiles == (51 * n + DEFAULT_TILE - 1) // DEFAULT_TILE, (res.tiles, res.tiles_rewalked)
    facts = expected_tiles(buf, end.nCentralOff, end.nCentralOff + end.nCentralSize, DEFAULT_TILE)
    assert facts["straddles"] and res.tiles_rewalked == facts["rewalked"]


# ---- 8: the tool -------------------------------------------------------------------------------------------------------------------------------------------
def check_cli(cli, tmp_path):
    root = str(tmp_path)
    parts = {"one.txt": F.text(5000, 900), "empty.bin": b"", "sub/three.txt": F.text(70000, 901), "sub/deeper/four": F.noise(3000, 902)}
    os.makedirs(os.path.join(root, "sub", "deeper"))
    for name, p in parts.items():
        with open(os.path.join(root, name), "wb") as f:
            f.write(p)
    r = subprocess.run([cli, "-a", "out.zip"] + list(parts), capture_output=True, text=True, timeout=120, cwd=root)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([cli, "-x", "-v", "-a", "out.zip", "unpacked"], capture_output=True, text=True, timeout=120, cwd=root)
    assert r.returncode == 0 and "4 entries" in r.stdout and "rewalked" in r.stdout and "sub/three.txt" in r.stdout, r.stdout + r.stderr
    for name, p in parts.items():
        assert open(os.path.join(root, "unpacked", name), "rb").read() == p, name
    # zipfile's, with a directory entry
    with zipfile.ZipFile(os.path.join(root, "py.zip"), "w", zipfile.ZIP_DEFLATED) as z:
        z.writestr("d/", b"")
        z.writestr("d/e/f.txt", parts["one.txt"])
        z.writestr(zipfile.ZipInfo("stored"), parts["sub/deeper/four"])
    r = subprocess.run([cli, "-x", "-a", "py.zip", "py"], capture_output=True, text=True, timeout=120, cwd=root)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.isdir(os.path.join(root, "py", "d")) and open(os.path.join(root, "py", "d/e/f.txt"), "rb").read() == parts["one.txt"]
    assert open(os.path.join(root, "py", "stored"), "rb").read() == parts["sub/deeper/four"]
    # names that would leave the directory: the whole archive is refused and nothing is created
    for k, evil in enumerate(("../evil", "/abs", "a\\b", "ok/../../evil")):
        with zipfile.ZipFile(os.path.join(root, "evil%d.zip" % k), "w") as z:
            z.writestr("good.txt", b"good")
            info = zipfile.ZipInfo("placeholder")
            info.filename = evil   # (the constructor would tidy the name)
            z.writestr(info, b"evil")
        r = subprocess.run([cli, "-x", "-a", "evil%d.zip" % k, "evil%d" % k], capture_output=True, text=True, timeout=120, cwd=root)
        assert r.returncode != 0 and not os.path.exists(os.path.join(root, "evil%d" % k)) and not os.path.exists(os.path.join(root, "evil")), (evil, r.stdout + r.stderr)
        assert not os.path.exists("/abs")
    bad = bytearray(open(os.path.join(root, "py.zip"), "rb").read())
    bad[30 + 2 + 30 + 9 + 20] ^= 0x55   # (inside the second entry's deflate stream, behind "d/" and its own header)
    with open(os.path.join(root, "bad.zip"), "wb") as f:
        f.write(bad)
    r = subprocess.run([cli, "-x", "-a", "bad.zip", "bad"], capture_output=True, text=True, timeout=120, cwd=root)
    assert r.returncode != 0, "a damaged archive"
    # wrong counts of arguments: the usage, 100
    for args in (["-x", "-a", "out.zip"], ["-x", "-a", "out.zip", "a", "b"], ["-x", "-a"], ["-x", "-m", "-a", "out.zip", "d"], ["-a", "out3.zip"], ["-x", "one.txt"], []):
        r = subprocess.run([cli] + args, capture_output=True, text=True, timeout=120, cwd=root)
        assert r.returncode == 100 and "usage:" in r.stderr, (args, r.stdout + r.stderr)
