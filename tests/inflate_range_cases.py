"""Shared by tests/test_inflate_range_emu.py (CPU emulator build) and tests/test_inflate_range_gpu.py (product library on the MI355X): the files, the
runners and the checks of zultra_hip_inflate_range (zh_rg_select, zh_rg_items and zh_rg_edges, zultra_amd/csrc/zh_inflate_range.h), of
zultra_memory_index_gzi and zultra_memory_decompress_range. The yardstick of the bytes is gzip.decompress(file)[lo:hi] — for a file whose
index stops early, of the walker's prefix —; of the per-member results zultra_hip_inflate_file's for the same members; of first_member / range_members and
of the .gzi pairs the serial walk of tests/inflate_file_cases.py, whose file builders these cases use."""
import gzip
import os
import subprocess

import numpy as np

import corpus
import inflate_cases as I
import inflate_file_cases as F
import verify_cases as V
from inflate_cases import CANARY, CANARY_BYTE

U64 = 2 ** 64 - 1
BAD_CHECK = 15


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------------------
class Case:
    """A file with what the walker and Python say of it. want: the output of the indexed prefix where the file itself is damaged (the sound file's)."""

    def __init__(self, name, buf, want=None):
        self.name, self.buf = name, bytes(buf)
        self.items, self.stop, self.at, self.out = F.walk(self.buf)
        self.want = (gzip.decompress(self.buf[: self.at]) if self.at else b"") if want is None else want
        assert len(self.want) == self.out, name
        self._file = None

    def clip(self, first, nbytes):
        return min(first, self.out), min(first + nbytes, U64, self.out)

    def members(self, lo, hi):
        """-> (m0, m1) of the walker's items for bytes [lo, hi), lo < hi."""
        holds = lambda x: next(k for k, it in enumerate(self.items) if it[3] and it[2] <= x < it[2] + it[3])
        return holds(lo), holds(hi - 1)

    def file_results(self, lib):
        """zultra_hip_inflate_file's per-member results for the whole file (host to host), once."""
        if self._file is None:
            src = np.frombuffer(self.buf + b"\0", dtype=np.uint8).copy()[:-1]
            rc, res, mem, _ = lib.inflate_file(src, len(self.buf), np.zeros(max(self.out, 1), dtype=np.uint8), self.out, len(self.items))
            assert rc >= 0 and res.members == len(self.items), self.name
            self._file = [tuple(int(v) for v in r) for r in mem]
        return self._file


class Held:
    """The source of a case where the calls read it: a device copy `lead` bytes into an allocation, or a host array."""

    def __init__(self, lib, case, on_device=True, lead=0):
        self.lib, self.case, self.on_device = lib, case, on_device
        if on_device:
            self.dc = V.DeviceCopy(lib, np.frombuffer(b"\xee" * lead + case.buf + b"\xee" * 7, dtype=np.uint8).copy())
            self.src = self.dc.ptr + lead
        else:
            self.dc, self.src = None, np.frombuffer(case.buf + b"\0", dtype=np.uint8).copy()[:-1]

    def free(self):
        if self.dc:
            self.dc.free()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def run_range(held, first, nbytes, dst_on_device=True, dst_lead=0, extra=0, short=0, results=True, results_short=0):
    """zultra_hip_inflate_range with out_size + extra - short bytes of room between canaries, room for range_members - results_short results.
    -> (rc, RangeResult, [member results as tuples], the room's bytes)."""
    lib, case = held.lib, held.case
    lo, hi = case.clip(first, nbytes)
    n = 0
    if hi > lo:
        m0, m1 = case.members(lo, hi)
        n = m1 - m0 + 1
    room = hi - lo + extra - short
    cap = (n - results_short) if results else None
    if dst_on_device:
        d = V.DeviceCopy(lib, np.full(dst_lead + CANARY + room + CANARY, CANARY_BYTE, dtype=np.uint8))
        try:
            rc, res, mem, ms = lib.inflate_range(held.src, len(case.buf), first, nbytes, d.ptr + dst_lead + CANARY, room, cap)
            back = I.device_read(lib, d, dst_lead + 2 * CANARY + room).copy()[dst_lead:]
        finally:
            d.free()
    else:
        back = np.full(dst_lead + 2 * CANARY + room, CANARY_BYTE, dtype=np.uint8)[dst_lead:]
        rc, res, mem, ms = lib.inflate_range(held.src, len(case.buf), first, nbytes, back[CANARY:], room, cap)
    assert (back[:CANARY] == CANARY_BYTE).all() and (back[CANARY + room:] == CANARY_BYTE).all(), "a canary was written"
    assert len(ms) == 5
    return rc, res, [tuple(int(v) for v in r) for r in mem], back[CANARY: CANARY + room]


def check_range(held, first, nbytes, **kw):
    """One range against the yardsticks. -> (rc, RangeResult)."""
    lib, case = held.lib, held.case
    lo, hi = case.clip(first, nbytes)
    tag = (case.name, first, nbytes, kw)
    rc, res, mem, back = run_range(held, first, nbytes, **kw)
    assert (res.members, res.stop, res.src_used, res.file_size, res.out_size) == (len(case.items), case.stop, case.at, case.out, hi - lo), (tag, res.members, res.stop, res.src_used, res.file_size, res.out_size)
    assert 0 < res.tiles and res.tiles_rewalked <= res.tiles, tag
    if hi == lo:
        assert rc == 0 and res.range_members == 0 and mem == [] and (back == CANARY_BYTE).all(), tag
        return rc, res
    m0, m1 = case.members(lo, hi)
    assert (res.first_member, res.range_members) == (m0, m1 - m0 + 1), (tag, res.first_member, res.range_members, m0, m1)
    want_mem = case.file_results(lib)[m0: m1 + 1]
    assert rc == sum(1 for r in want_mem if r[0]), (tag, rc)
    if kw.get("results", True):
        assert mem == want_mem, (tag, [(a, b) for a, b in zip(mem, want_mem) if a != b][:3])
    got, want = back[: hi - lo], np.frombuffer(case.want, dtype=np.uint8)[lo: hi]
    sound = np.ones(hi - lo, dtype=bool)
    for k, r in enumerate(want_mem):   # a failed member's own part is unspecified
        if r[0]:
            it = case.items[m0 + k]
            sound[max(it[2], lo) - lo: max(min(it[2] + it[3], hi), lo) - lo] = False
    assert (got[sound] == want[sound]).all(), (tag, np.nonzero(sound & (got != want))[0][:8])
    assert (back[hi - lo:] == CANARY_BYTE).all(), (tag, "bytes behind out_size were written")
    return rc, res


def boundary_points(case):
    """Every member boundary of the output, one byte before it and one behind it, inside [0, F + 1]."""
    pts = set()
    for it in case.items:
        for b in (it[2], it[2] + it[3]):
            pts.update(p for p in (b - 1, b, b + 1) if 0 <= p <= case.out + 1)
    return sorted(pts)


def boundary_ranges(case, reach=None):
    """(first, nbytes) from every boundary point to every later one (reach: only to the next `reach` points and to the last)."""
    pts = boundary_points(case)
    out = []
    for i, a in enumerate(pts):
        for j in range(i + 1, len(pts)):
            if reach is None or j - i <= reach or j == len(pts) - 1:
                out.append((a, pts[j] - a))
    return out


# ---- 1. every range of a tiny file ------------------------------------------------------------------------------------------------------------------
def tiny_case():
    parts = [b"abc", b"", b"defgh", b"i", b"", b"jklm"]
    buf = b"".join(F.bgzf(p, raw=F.stored(p)) if k & 1 else F.bgzf(p) for k, p in enumerate(parts)) + F.EOF_MARKER
    case = Case("tiny", buf)
    assert case.out == 13 and len(case.items) == 7 and case.stop == 0
    return case


def check_tiny(lib):
    case = tiny_case()
    n = 0
    for on_device in (True, False):
        with Held(lib, case, on_device=on_device, lead=1) as held:
            for first in range(0, 15):
                for nbytes in range(0, 16):
                    check_range(held, first, nbytes, dst_on_device=on_device, dst_lead=(first + nbytes) & 3, extra=nbytes & 1)
                    n += 1
            for first in (0, 5, 12, 13, U64 - 3, U64):   # first + nbytes wraps 2^64: the sum saturates
                rc, res = check_range(held, first, U64, dst_on_device=on_device)
                assert res.out_size == max(13 - first, 0)
                n += 1
    return n


# ---- 2. edges at real sizes ---------------------------------------------------------------------------------------------------------------------------
_SIZES = []


def sizes_case():
    """Payloads of 1, 100, 65280 (stored) and 65536 bytes — a BGZF member of at most 65536 bytes holds 65536 bytes of payload only deflated — and a member
    of zeros whose ISIZE is 1 MiB under a stream of about 1 KiB: an edge member far above 64 KiB."""
    if not _SIZES:
        zeros = b"\0" * (1 << 20)
        parts = [F.text(1, 1), F.text(100, 2), F.noise(65280, 3), F.text(65536, 4), zeros, F.text(300, 5)]
        ms = [F.bgzf(parts[0]), F.bgzf(parts[1]), F.bgzf(parts[2], raw=F.stored(parts[2])), F.bgzf(parts[3]), F.bgzf(zeros, level=9), F.bgzf(parts[5])]
        assert len(ms[4]) < 1200
        _SIZES.append(Case("sizes", b"".join(ms) + F.EOF_MARKER, b"".join(parts)))
    return _SIZES[0]


def check_sizes(lib, reach=None):
    case = sizes_case()
    n = 0
    with Held(lib, case) as held:
        for first, nbytes in boundary_ranges(case, reach):
            check_range(held, first, nbytes, dst_lead=first & 3)
            n += 1
        for at in (0, 1, 100, 101, 65381, 65382, 65381 + 65536 + 12345, case.out - 1):   # single bytes
            check_range(held, at, 1)
            n += 1
        rc, res, mem, back = run_range(held, 0, case.out)   # the whole file: what zultra_hip_inflate_file writes
        frc, fres, fmem, fback = F.run_file(lib, case.buf)
        assert rc == frc == 0 and mem == fmem[:6] and back.tobytes() == fback.tobytes() == case.want   # (the end marker holds no byte of the range)
        assert (res.first_member, res.range_members) == (0, 6)
    return n + 1


# ---- 3. tiles (a process of its own per tile size) --------------------------------------------------------------------------------------------------
def check_tiles(lib):
    """Under the tile size of this process: ranges over many tiles, members longer than several tiles (unused tiles between the selected ones), both ends
    in one tile, and the decoy files: a rewalked tile in front of the range and inside it."""
    T = F.tile_size()
    n = 0
    mixed = Case("mixed_sizes", dict(F.boundary_files(T))["mixed_sizes"])
    with Held(lib, mixed, lead=3) as held:
        rc, res = check_range(held, 0, mixed.out)
        assert res.tiles < (len(mixed.buf) + T - 1) // T, "no tile was jumped over"
        for first, nbytes in boundary_ranges(mixed, reach=1):
            check_range(held, first, nbytes, dst_lead=first & 3)
            n += 1
        a, b, c = mixed.items[6: 9]   # the three members of 7 bytes, some 40 bytes each: with tiles of 100 bytes and more, two neighbours start in one tile
        if T >= 100:
            assert a[0] // T == b[0] // T or b[0] // T == c[0] // T
        check_range(held, a[2] + 3, 9)
        check_range(held, b[2] + 1, 9)
        n += 2
    for name, buf, rewalked in F.decoy_files(T):
        case = Case(name, buf)
        d = next((it for it in case.items if it[0] + it[1] > T * (2 * 60031 // T + 2) - 23), None)   # the member with the fake header (file e has none)
        ranges = [(case.items[1][2] + 11, case.out), (case.out - 150, 100)]
        if d:   # behind it, from its end, around it, inside it
            ranges += [(d[2] + d[3] + 5, 200), (d[2] + d[3], case.out), (d[2] - 100, d[3] + 150), (d[2] + 7, d[3] - 9)]
        with Held(lib, case) as held:
            for first, nbytes in ranges:
                rc, res = check_range(held, first, nbytes)
                if rewalked is not None:
                    assert (res.tiles_rewalked > 0) == rewalked, (name, T)
                n += 1
    return n


# ---- 4. placement -------------------------------------------------------------------------------------------------------------------------------------
def check_placement(lib):
    parts = [F.text(n, 30 + k) for k, n in enumerate((700, 33, 4001, 0, 520, 1000))]
    case = Case("placement", b"".join(F.bgzf(p) for p in parts) + F.EOF_MARKER, b"".join(parts))
    n = 0
    for src_dev in (True, False):
        with Held(lib, case, on_device=src_dev, lead=2) as held:
            for dst_dev in (True, False):
                for dst_lead in range(4):
                    # lo inside member 0, so that members 1.. lie at dst_off - lo of either parity; the last range is exactly members 1..4
                    for first, nbytes in ((1, 5000), (2, 5000), (350, case.out), (700, 33 + 4001 + 520), (699, 2), (734, 4000)):
                        check_range(held, first, nbytes, dst_on_device=dst_dev, dst_lead=dst_lead)   # exactly out_size bytes between the canaries
                        n += 1
                    check_range(held, 1, 5000, dst_on_device=dst_dev, dst_lead=dst_lead, extra=37)
    return n


# ---- 5. only the covered members ----------------------------------------------------------------------------------------------------------------------
def check_only_covered(lib):
    parts = [F.text(300 + 50 * k, 60 + k) for k in range(9)]
    ms = [F.bgzf(p) for p in parts]
    want = b"".join(parts)
    starts = [sum(len(m) for m in ms[:k]) for k in range(10)]
    offs = [sum(len(p) for p in parts[:k]) for k in range(10)]

    def damaged(*members):
        buf = bytearray(b"".join(ms))
        for k in members:
            buf[starts[k + 1] - 8] ^= 1   # its CRC-32
        return Case("crc of %s" % (members,), bytes(buf), want)

    first, nbytes = offs[4] + 20, offs[6] + 30 - (offs[4] + 20)   # from inside member 4 to inside member 6
    with Held(lib, damaged(1)) as held:
        for dev in (True, False):
            rc, res = check_range(held, first, nbytes, dst_on_device=dev)
            assert rc == 0 and (res.first_member, res.range_members) == (4, 3)
        rc, res = check_range(held, offs[2], offs[9] - offs[2])   # from a boundary: no edge member at all
        assert rc == 0
        rc, res = check_range(held, offs[1] + 1, 10)
        assert rc == 1
    for k in (5, 4, 6):   # an interior member, the head edge, the tail edge
        case = damaged(1, k)
        with Held(lib, case) as held:
            for dev in (True, False):
                rc, res, mem, back = run_range(held, first, nbytes, dst_on_device=dev)
                assert rc == 1 and [r[0] for r in mem] == [BAD_CHECK if 4 + j == k else 0 for j in range(3)], (k, dev, mem)
                check_range(held, first, nbytes, dst_on_device=dev)   # (every other member's bytes in place)
    return 4


# ---- 6. stops -----------------------------------------------------------------------------------------------------------------------------------------
def stop_case():
    parts = [F.text(400 + 10 * k, 80 + k) for k in range(6)]
    ms = [gzip.compress(p, 6, mtime=0) if k == 3 else F.bgzf(p) for k, p in enumerate(parts)]
    case = Case("plain at 3 of 6", b"".join(ms))
    assert case.stop == 1 and len(case.items) == 3 and case.want == b"".join(parts[:3])
    return case


def check_stops(lib):
    case = stop_case()
    with Held(lib, case) as held:
        rc, res = check_range(held, 100, 900)   # members 0..2
        assert rc == 0 and res.stop == 1 and res.out_size == 900
        rc, res = check_range(held, 1000, 5000)   # past the prefix: clipped to it
        assert rc == 0 and res.stop == 1 and res.out_size == case.out - 1000
        rc, res = check_range(held, case.out, 10)
        assert rc == 0 and res.out_size == 0
    assert lib.memory_decompress_range(case.buf, 100, 900) == case.want[100:1000]
    assert lib.memory_decompress_range(case.buf, 100, case.out - 100) == case.want[100:]
    assert lib.memory_decompress_range(case.buf, 1000, 5000) is None   # what lies behind the prefix is unknown
    assert lib.memory_decompress_range(case.buf, 100, case.out - 99) is None
    for tail, kind in ((b"garbage", 3), (F.bgzf(F.text(50, 1))[:-3], 2)):
        c = Case("stop%d" % kind, case.buf[: case.at] + tail)
        assert c.stop == kind
        with Held(lib, c, on_device=False) as held:
            rc, res = check_range(held, 5, c.out, dst_on_device=False)
            assert rc == 0 and res.stop == kind
    with Held(lib, Case("nothing indexed", gzip.compress(b"plain", 6, mtime=0))) as held:
        rc, res = check_range(held, 0, 10)
        assert (rc, res.members, res.stop, res.out_size) == (0, 0, 1, 0)


# ---- 7. room, bad arguments ---------------------------------------------------------------------------------------------------------------------------
def check_room(lib):
    case = sizes_case()
    first, nbytes = 50, 65381 + 1000   # members 1..3: two edges
    with Held(lib, case) as held:
        for dev in (True, False):
            rc, res, mem, back = run_range(held, first, nbytes, dst_on_device=dev, short=1)
            assert rc == -1 and (res.stop, res.out_size, res.first_member, res.range_members, res.members, res.file_size) == (4, nbytes, 1, 3, 7, case.out) and mem == []
            assert (back == CANARY_BYTE).all(), "a refused call has written"
            rc, res, mem, back = run_range(held, first, nbytes, dst_on_device=dev, results_short=1)
            assert rc == -1 and (res.stop, res.out_size, res.range_members) == (4, nbytes, 3) and (back == CANARY_BYTE).all()
            check_range(held, first, nbytes, dst_on_device=dev, results=False)   # results == NULL
            check_range(held, 0, case.out, dst_on_device=dev, results=False)


def check_bad_arguments(lib):
    buf = F.bgzf(F.text(100, 90)) + F.EOF_MARKER
    src = np.frombuffer(buf, dtype=np.uint8).copy()
    dst = np.zeros(200, dtype=np.uint8)
    n = len(src)
    rc, res, mem, _ = lib.inflate_range(src, n, 10, 50, dst, 200, 2)
    assert rc == 0 and dst[:50].tobytes() == F.text(100, 90)[10:60] and not dst[50:].any()
    dst[:] = 0
    assert lib.inflate_range(None, n, 10, 50, dst, 200, 2)[0] == -1
    assert lib.inflate_range(src, 0, 10, 50, dst, 200, 2)[0] == -1
    assert lib.inflate_range(src, n, 10, 50, None, 200, 2)[0] == -1
    assert lib.inflate_range(src, n, 10, 50, dst, 200, 2, device=-1)[0] == -1
    assert lib.inflate_range(src, n, 10, 50, dst, 200, 2, device=lib.device_count())[0] == -1
    g = lib.L.zultra_hip_inflate_range
    assert g(0, src.ctypes.data, n, 0, 10, 50, dst.ctypes.data, 200, 0, None, None, 0, None) == -1   # res NULL
    assert not dst.any(), "a refused call has written"
    assert lib.memory_decompress_range(buf, 10, 50) == F.text(100, 90)[10:60]   # (sets the prototypes)
    assert lib.memory_index_gzi(buf) == gzi_of(Case("one", buf))
    h, x = lib.L.zultra_memory_decompress_range, lib.L.zultra_memory_index_gzi
    p = src.ctypes.data
    assert h(None, n, 0, 5, dst.ctypes.data, 200, None, 0) == h(p, 0, 0, 5, dst.ctypes.data, 200, None, 0) == h(p, n, 0, 5, None, 200, None, 0) == h(p, n, 0, 5, dst.ctypes.data, 200, None, 8) == U64
    assert h(p, n, 0, 50, dst.ctypes.data, 49, None, 0) == U64   # too little room
    assert x(None, n, None, 0) == x(p, 0, None, 0) == U64
    assert not dst.any()


# ---- 8. the .gzi index --------------------------------------------------------------------------------------------------------------------------------
def gzi_of(case, keep=lambda k: True):
    """The pairs of the walker: every member but the first (those of them that `keep` keeps)."""
    pairs = [(it[0], it[2]) for k, it in enumerate(case.items[1:]) if keep(k)]
    return len(pairs).to_bytes(8, "little") + b"".join(c.to_bytes(8, "little") + u.to_bytes(8, "little") for c, u in pairs)


def check_gzi(lib, big):
    own = lib.memory_compress_bgzf(F.text(3000, 7), 1000)
    cases = [tiny_case(), sizes_case(), Case("own", own)]
    assert len(cases[2].items) == 4 and cases[2].want == F.text(3000, 7)
    for case in cases:
        gzi = gzi_of(case)
        assert lib.memory_index_gzi(case.buf) == gzi, case.name
        assert lib.memory_index_gzi(case.buf, query=True) == len(gzi) == 8 + 16 * (len(case.items) - 1)
        assert lib.memory_index_gzi(case.buf, cap=len(gzi) - 1) is None
        assert lib.memory_index_gzi(case.buf, cap=len(gzi) + 9) == gzi
    for c in (stop_case(), Case("garbage", tiny_case().buf + b"garbage"), Case("cut", tiny_case().buf[:-3])):
        assert c.stop in (1, 2, 3) and lib.memory_index_gzi(c.buf) is None and lib.memory_index_gzi(c.buf, query=True) is None
    # with the index as without, over the boundary ranges; a sparse index — every fourth pair, as another writer may keep — as well
    for case in (cases[0], cases[1]):
        gzi, sparse = gzi_of(case), gzi_of(case, lambda k: k % 4 == 3)
        ranges = boundary_ranges(case, None if case.out < 100 else (1 if not big else 3))
        for first, nbytes in ranges:
            lo, hi = case.clip(first, nbytes)
            plain = lib.memory_decompress_range(case.buf, first, nbytes)
            assert plain == case.want[lo:hi], (case.name, first, nbytes)
            assert lib.memory_decompress_range(case.buf, first, nbytes, gzi=gzi) == plain, (case.name, first, nbytes)
            assert lib.memory_decompress_range(case.buf, first, nbytes, gzi=sparse) == plain, (case.name, first, nbytes)
        assert lib.memory_decompress_range(case.buf, 3, 0, gzi=gzi) == b"" and lib.memory_decompress_range(case.buf, case.out + 5, 9, gzi=gzi) == b""
        assert lib.memory_decompress_range(case.buf, 1, case.out, gzi=gzi) == case.want[1:]   # short at the end of the file
        assert lib.memory_decompress_range(case.buf, 1, 10, max_out=9, gzi=gzi) is None
    # the bytes outside the window are never read: noise there changes nothing
    case = sizes_case()
    gzi = gzi_of(case)
    first, nbytes = 50, 40   # inside member 1: the window is that member
    c0, c1 = case.items[1][0], case.items[2][0]
    noisy = np.frombuffer(F.noise(len(case.buf), 99), dtype=np.uint8).copy()
    noisy[c0:c1] = np.frombuffer(case.buf[c0:c1], dtype=np.uint8)
    assert lib.memory_decompress_range(noisy, first, nbytes, gzi=gzi) == case.want[first: first + nbytes]
    assert lib.memory_decompress_range(noisy, first, nbytes) is None
    first = case.items[5][2] + 5   # inside the last member with payload: the window runs to the end of the input
    noisy = np.frombuffer(F.noise(len(case.buf), 98), dtype=np.uint8).copy()
    noisy[case.items[5][0]:] = np.frombuffer(case.buf[case.items[5][0]:], dtype=np.uint8)
    assert lib.memory_decompress_range(noisy, first, 1000, gzi=gzi) == case.want[first:]
    # an index that is malformed, or lies
    pairs = [(it[0], it[2]) for it in case.items[1:]]

    def enc(ps, n=None):
        return (len(ps) if n is None else n).to_bytes(8, "little") + b"".join(c.to_bytes(8, "little") + u.to_bytes(8, "little") for c, u in ps)

    def refused(g, first=50, nbytes=40):
        return lib.memory_decompress_range(case.buf, first, nbytes, gzi=g) is None

    assert not refused(enc(pairs))
    assert refused(gzi[:-1]) and refused(gzi + b"\0") and refused(gzi[:7]) and refused(b"")          # a size that is not 8 + 16 N
    assert refused(enc(pairs, len(pairs) + 1)) and refused(enc(pairs, len(pairs) - 1))                 # N disagrees with the size
    assert refused(enc([pairs[1], pairs[0]] + pairs[2:])) and refused(enc([pairs[0], pairs[0]] + pairs[1:]))   # offsets out of order
    assert refused(enc(pairs[:2] + [(pairs[2][0], pairs[1][1] - 1)] + pairs[3:]))                      # an uncompressed offset that decreases
    assert refused(enc([(0, 0)] + pairs))                                                              # a compressed offset of 0
    assert refused(enc(pairs + [(len(case.buf), case.out)])) and refused(enc(pairs + [(len(case.buf) + 5, case.out)]))   # at or past nIn
    assert refused(enc([(pairs[0][0] + 1, pairs[0][1])] + pairs[1:]))                                  # (c0) no member start
    assert refused(enc([pairs[0], (pairs[1][0] - 1, pairs[1][1])] + pairs[2:]))                        # (c1) no member start
    assert refused(enc([(pairs[0][0], pairs[0][1] - 1)] + pairs[1:]))                                  # u0 off by one: the window's size gives it away
    assert refused(enc([pairs[0], (pairs[1][0], pairs[1][1] + 1)] + pairs[2:]))                        # u1 off by one


# ---- 9. GPU only: larger ------------------------------------------------------------------------------------------------------------------------------
def check_large_file(lib):
    """128 members of 64 KiB of output: the default tile is crossed many times."""
    assert F.tile_size() == F.DEFAULT_TILE
    parts = [(F.noise(65536, k) if k % 3 == 0 else F.text(65536, k)) for k in range(128)]
    parts = [p if k % 3 else p[:65280] for k, p in enumerate(parts)]
    buf = b"".join(F.bgzf(p, level=1) if k % 3 else F.bgzf(p, raw=F.stored(p)) for k, p in enumerate(parts)) + F.EOF_MARKER
    case = Case("large", buf, b"".join(parts))
    assert len(buf) > 8 * F.DEFAULT_TILE
    across = next(it for it in case.items if it[0] + it[1] > 3 * F.DEFAULT_TILE)   # the member that crosses a boundary of two default tiles
    with Held(lib, case, lead=1) as held:
        for first, nbytes in ((case.out // 2, 1), (case.out // 2 - 77, 1 << 20), (across[2] - 70000, 140000 + across[3]), (0, case.out), (case.out - 5, 100)):
            rc, res = check_range(held, first, nbytes, dst_lead=1)
            assert rc == 0 and res.tiles >= 8 and res.members == 129
    with Held(lib, case, on_device=False) as held:
        check_range(held, case.out // 3, 300000, dst_on_device=False)


def check_own_files(lib, nfiles):
    """A files batch of the library's coder framed as BGZF by the test, and a range cut from it, device to device."""
    sizes = [I.FILE_SIZES[i % len(I.FILE_SIZES)] for i in range(nfiles)]
    parts = [(corpus.json_like, corpus.text_like)[i & 1](n, 100 + i).tobytes() for i, n in enumerate(sizes)]
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    ctx = lib.files_context(8191, nfiles)
    try:
        file_off = ctx.compress_files(np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), offsets, sizes)
        stream = ctx.stream_read(int(file_off[-1])).tobytes()
    finally:
        ctx.close()
    case = Case("own files", b"".join(F.bgzf(p, raw=stream[int(file_off[i]): int(file_off[i + 1])]) for i, p in enumerate(parts)) + F.EOF_MARKER, b"".join(parts))
    with Held(lib, case) as held:
        for first, nbytes in ((case.out // 3, case.out // 2), (1, 1), (case.out - 4000, 10000)):
            rc, res = check_range(held, first, nbytes)
            assert rc == 0


# ---- 10. the command-line tool ------------------------------------------------------------------------------------------------------------------------
def check_cli(cli, tmp_path):
    data = F.text(150000, 5) + F.noise(50000, 6)
    raw, gz, gzi, out = (os.path.join(str(tmp_path), n) for n in ("data.bin", "data.gz", "data.gz.gzi", "slice.out"))
    with open(raw, "wb") as f:
        f.write(data)
    r = subprocess.run([cli, "-f", "bgzf", "-i", gzi, raw, gz], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    case = Case("cli", open(gz, "rb").read())
    assert case.want == data and open(gzi, "rb").read() == gzi_of(case)
    for first, length in ((0, 10), (65279, 3), (100000, 70000), (199990, 500), (300000, 5)):
        for index in ((), ("-i", gzi)):
            r = subprocess.run([cli, "-x", "-m", "-v", "-f", "gzip", "-r", "%d:%d" % (first, length)] + list(index) + [gz, out], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stdout + r.stderr
            assert open(out, "rb").read() == data[first: first + length], (first, length, index)
            if first < len(data):
                assert "first member" in r.stdout and "tiles" in r.stdout, r.stdout
    r = subprocess.run([cli, "-x", "-m", "-f", "gzip", "-r", "12", gz, out], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0, "-r takes first:length"
