"""Shared by tests/test_inflate_members_emu.py (CPU emulator build) and tests/test_inflate_members_gpu.py (product library on the MI355X): the members,
the batch runner and the checks of zultra_hip_inflate_members (zh_frame_heads and zh_check_members, zultra_amd/csrc/zh_inflate_check.h, around the
inflate kernels of zh_inflate_out.h) and zultra_memory_decompress_batch. One framing serves every item of a call. The yardstick is Python's zlib:
decompressobj(wbits=31), decompressobj(wbits=15[, zdict=]), zlib.crc32 and zlib.adler32; accept means that `eof` is set and no error was raised.
The writers and the runner's pattern are those of tests/inflate_cases.py and tests/inflate_dict_cases.py."""
import gzip
import itertools
import os
import subprocess
import sys
import zlib

import numpy as np

import corpus
import inflate_cases as I
import inflate_dict_cases as D
import verify_cases as V
from inflate_cases import CANARY, CANARY_BYTE, DISTANCE, OK, STREAM_END

RAW, ZLIB, GZIP = 0, 1, 2
BAD_FRAME, BAD_CHECK, BAD_ISIZE = 14, 15, 16
WBITS = {RAW: -15, ZLIB: 15, GZIP: 31}
SMALL_MAX = 64 * 256   # zh_check_members: items with at most this much room lie several to a workgroup


# ---- running a batch ----------------------------------------------------------------------------------------------------------------------
def run_members(lib, members, caps, framing, dictionary=None, on_device=True, src_sizes=None, src_lead=0, dst_lead=0, dict_lead=0):
    """The members packed back to back (source offsets of every residue mod 4), the destination ranges `caps` long and CANARY bytes apart.
    on_device: source, destination and dictionary in device memory, each *_lead bytes behind an allocation's start (0xFF in front of the source
    and the dictionary and behind them, canaries around the destination); else host arrays, staged by the call. src_sizes: what the items give
    as src_size instead of the members' lengths. -> (rc, [(reason, blocks, out_size, src_used, head_size, check, output bytes)])."""
    packed = b"".join(bytes(m) for m in members)
    items, soff, doff = [], 0, CANARY
    for k, m in enumerate(members):
        items.append((soff, len(m) if src_sizes is None else src_sizes[k], doff, caps[k]))
        soff += len(m)
        doff += caps[k] + CANARY
    n = 0 if dictionary is None else len(dictionary)
    if on_device:
        src = np.frombuffer(b"\xff" * src_lead + packed + b"\xff" * 8, dtype=np.uint8).copy()
        dst = np.full(dst_lead + doff, CANARY_BYTE, dtype=np.uint8)
        held = np.frombuffer(b"\xff" * dict_lead + bytes(dictionary or b"") + b"\xff" * 8, dtype=np.uint8).copy()
        s, d, h = V.DeviceCopy(lib, src), V.DeviceCopy(lib, dst), V.DeviceCopy(lib, held)
        try:
            assert (s.ptr + src_lead) & 3 == src_lead & 3 and (d.ptr + dst_lead) & 3 == dst_lead & 3 and (h.ptr + dict_lead) & 3 == dict_lead & 3
            rc, res, _ = lib.inflate_members(s.ptr + src_lead, len(packed), d.ptr + dst_lead, doff, None if dictionary is None else h.ptr + dict_lead, n, framing, items)
            back = I.device_read(lib, d, len(dst)).copy()
        finally:
            s.free()
            d.free()
            h.free()
        assert (back[:dst_lead] == CANARY_BYTE).all()
        back = back[dst_lead:]
    else:
        src = np.frombuffer(packed + b"\0", dtype=np.uint8).copy()[:-1]
        back = np.full(doff, CANARY_BYTE, dtype=np.uint8)
        arr = None if dictionary is None else np.frombuffer(bytes(dictionary) + b"\0", dtype=np.uint8).copy()[:-1]
        rc, res, _ = lib.inflate_members(src, len(src), back, doff, arr, n, framing, items)
    assert rc >= 0, "zultra_hip_inflate_members failed"
    assert rc == int((res["reason"] != 0).sum())
    I.check_canaries(back, items, res)
    return rc, [(int(r["reason"]), int(r["blocks"]), int(r["out_size"]), int(r["src_used"]), int(r["head_size"]), int(r["check"]),
                 back[it[2]: it[2] + int(r["out_size"])].tobytes()) for it, r in zip(items, res)]


def zlib_verdict(member, framing, dictionary=None):
    """Host zlib on one member -> (inflates without error and reaches the end, output, bytes of the member used)."""
    d = zlib.decompressobj(WBITS[framing], zdict=bytes(dictionary)) if dictionary and framing != GZIP else zlib.decompressobj(WBITS[framing])
    try:
        out = d.decompress(bytes(member))
    except zlib.error:
        return False, b"", 0
    return bool(d.eof), out, len(member) - len(d.unused_data)


def checksum(framing, data):
    return {RAW: 0, ZLIB: zlib.adler32(data), GZIP: zlib.crc32(data)}[framing] & 0xFFFFFFFF


def hold_to_zlib(lib, labels, members, framing, cap, dictionary=None, reject_reason=None, **kw):
    """One batch: reason 0 exactly where host zlib accepts the member, then with zlib's bytes, its count of bytes used and its checksum;
    reject_reason: what every reject must be. -> (results, accepted)."""
    rc, res = run_members(lib, members, [cap] * len(members), framing, dictionary, **kw)
    accepted = 0
    for label, m, r in zip(labels, members, res):
        ok, want, used = zlib_verdict(m, framing, dictionary)
        assert not (ok and len(want) > cap), label
        assert (r[0] == OK) == ok, (label, r[:6], ok)
        if ok:
            accepted += 1
            assert r[6] == want and r[3] == used and r[5] == checksum(framing, want), (label, r[:6], len(want), used)
        elif reject_reason is not None:
            assert r[0] == reject_reason, (label, r[:6])
    return res, accepted


# ---- members ----------------------------------------------------------------------------------------------------------------------------------
BODY_TEXT = b"a fixed body, a fixed body: the body of every hand-built member. " * 2
BODY = I.zlib_raw(BODY_TEXT, 6, zlib.Z_DEFAULT_STRATEGY)


def gzip_trailer(data):
    return zlib.crc32(data).to_bytes(4, "little") + (len(data) & 0xFFFFFFFF).to_bytes(4, "little")


def gzip_header(flg, extra=b"", name=b"", comment=b"", hcrc_ok=True, cm=8, magic=b"\x1f\x8b"):
    """RFC 1952 2.3 by hand: what `flg` announces is written, whatever the bits are."""
    h = magic + bytes([cm, flg]) + (1234567).to_bytes(4, "little") + b"\x02\x03"
    if flg & 4:
        h += len(extra).to_bytes(2, "little") + extra
    if flg & 8:
        h += name + b"\0"
    if flg & 16:
        h += comment + b"\0"
    if flg & 2:
        h += ((zlib.crc32(h) & 0xFFFF) ^ (0 if hcrc_ok else 0x100)).to_bytes(2, "little")
    return h


def gzip_member(header, raw_stream=BODY, data=BODY_TEXT):
    return header + raw_stream + gzip_trailer(data)


def zlib_member(data, level=6, dictionary=None):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, zlib.Z_DEFAULT_STRATEGY, zdict=dictionary) if dictionary else zlib.compressobj(level, zlib.DEFLATED, 15)
    return c.compress(data) + c.flush()


def gzip_header_cases():
    """-> [(name, header)]: every combination of FEXTRA / FNAME / FCOMMENT / FHCRC with XLEN 0, 1 and 300 and empty and 1-byte names, a right and
    a wrong FHCRC; each reserved FLG bit; CM = 7; wrong magic bytes."""
    out = []
    for fextra, fname, fcomment, fhcrc in itertools.product((0, 1), repeat=4):
        flg = 4 * fextra | 8 * fname | 16 * fcomment | 2 * fhcrc
        for xlen in ((0, 1, 300) if fextra else (0,)):
            for name in ((b"", b"n") if fname else (b"",)):
                for ok in ((True, False) if fhcrc else (True,)):
                    h = gzip_header(flg, extra=I._pattern(xlen, 5), name=name, comment=b"c!", hcrc_ok=ok)
                    out.append(("flg%02x_x%d_n%d_%s" % (flg, xlen, len(name), "ok" if ok else "badhcrc"), h))
    for bit in (0x20, 0x40, 0x80):
        out.append(("reserved_%02x" % bit, gzip_header(bit)))
        out.append(("reserved_%02x_with_name" % bit, gzip_header(bit | 8, name=b"n")))
    out.append(("cm7", gzip_header(0, cm=7)))
    out.append(("magic0", gzip_header(0, magic=b"\x1e\x8b")))
    out.append(("magic1", gzip_header(0, magic=b"\x1f\x8a")))
    out.append(("magic_swapped", gzip_header(0, magic=b"\x8b\x1f")))
    return out


def check_gzip_headers(lib):
    cases = gzip_header_cases()
    members = [gzip_member(h) for _, h in cases]
    for dev in (True, False):
        res, accepted = hold_to_zlib(lib, [c[0] for c in cases], members, GZIP, len(BODY_TEXT), reject_reason=BAD_FRAME, on_device=dev)
        for (name, h), m, r in zip(cases, members, res):
            if r[0] == OK:
                assert r[4] == len(h) and r[3] == len(m), (name, r[:6])
            else:
                assert r[2:6] == (0, 0, 0, 0) and ("bad" in name or "reserved" in name or "cm7" in name or "magic" in name), (name, r[:6])
        assert accepted == sum(1 for n, _ in cases if n.startswith("flg") and n.endswith("ok")) >= 30
    return len(cases)


def accept_cases(big):
    """-> [(name, framing, member, head_size, dictionary)]: the members the flips and the cuts start from. big: with the XLEN 300 headers."""
    out = [(name, GZIP, gzip_member(h), len(h), None) for name, h in gzip_header_cases() if name.startswith("flg") and name.endswith("ok") and (big or len(h) < 60)]
    if not big:
        out.append(next((name, GZIP, gzip_member(h), len(h), None) for name, h in gzip_header_cases() if name == "flg1e_x300_n1_ok"))
    out.append(("zlib_l6", ZLIB, zlib_member(BODY_TEXT), 2, None))
    out.append(("zlib_l0", ZLIB, zlib_member(BODY_TEXT, 0), 2, None))
    dictionary = BODY_TEXT[:40] + b"some more of a dictionary"
    out.append(("zlib_fdict", ZLIB, zlib_member(BODY_TEXT, 6, dictionary), 6, dictionary))
    return out


def check_header_flips(lib, big):
    """Every bit of every accept case's header flipped, one batch per case, one item per bit: zlib's accept / reject verdict; where both accept,
    bytes and src_used are equal. -> (mutants, those zlib accepts)."""
    total = benign = 0
    for name, framing, m, head, dictionary in accept_cases(big):
        muts = []
        for bit in range(8 * head):
            x = bytearray(m)
            x[bit >> 3] ^= 1 << (bit & 7)
            muts.append(bytes(x))
        labels = ["%s bit %d" % (name, b) for b in range(8 * head)]
        if dictionary:   # (a flipped FDICT bit: zlib then ignores the dictionary, this call does not — the documented difference, held apart)
            keep = [i for i, x in enumerate(muts) if x[1] & 0x20]
            muts, labels = [muts[i] for i in keep], [labels[i] for i in keep]
        _, ok = hold_to_zlib(lib, labels, muts, framing, len(BODY_TEXT) + 600, dictionary)
        total += len(muts)
        benign += ok
    assert benign > 0
    return total, benign


# ---- zlib headers -------------------------------------------------------------------------------------------------------------------------------
def check_zlib_headers(lib):
    """CINFO 0..8, every FLG without FDICT for CINFO 7 (those that pass the mod-31 check and those that fail it), the passing ones and one failing
    one for the other CINFO values."""
    members, labels = [], []
    tail = BODY + zlib.adler32(BODY_TEXT).to_bytes(4, "big")
    for cinfo in range(9):
        cmf = cinfo << 4 | 8
        passing = [f for f in range(256) if not f & 0x20 and (cmf << 8 | f) % 31 == 0]
        assert len(passing) >= 3
        for flg in ([f for f in range(256) if not f & 0x20] if cinfo == 7 else passing + [passing[0] ^ 1]):
            members.append(bytes([cmf, flg]) + tail)
            labels.append("cinfo%d_flg%02x" % (cinfo, flg))
    members.append(bytes([0x77, next(f for f in range(256) if not f & 0x20 and (0x77 << 8 | f) % 31 == 0)]) + tail)   # CM = 7 with a right check
    labels.append("cm7")
    res, accepted = hold_to_zlib(lib, labels, members, ZLIB, len(BODY_TEXT), reject_reason=BAD_FRAME)
    assert accepted >= 8 * 3 and all(r[4] == 2 for r in res if r[0] == OK)
    assert all(r[0] == BAD_FRAME for lab, r in zip(labels, res) if lab.startswith("cinfo8"))
    return len(members)


def check_zlib_fdict(lib, dict_size, leads=(0,)):
    """FDICT with the right dictionary (host pointer, then device pointers at every lead of `leads`), a wrong one, none; a dictionary given and no
    FDICT; raw and gzip items that need the dictionary."""
    dictionary = D.dictionary_of(corpus.text_like, dict_size)
    data = dictionary[-1:] * 4 + dictionary[-300:] + corpus.text_like(2000, 3).tobytes()
    m = zlib_member(data, 6, dictionary)
    assert m[1] & 0x20 and int.from_bytes(m[2:6], "big") == zlib.adler32(dictionary)
    plain = zlib_member(data, 6)
    for kw in [dict(on_device=False)] + [dict(dict_lead=lead) for lead in leads]:
        res, accepted = hold_to_zlib(lib, ["fdict", "fdict again"], [m, m], ZLIB, len(data), dictionary, **kw)
        assert accepted == 2 and all(r[4] == 6 for r in res), res
        wrong = dictionary[:-1] + bytes([dictionary[-1] ^ 1])
        other_order = dictionary[1:] + dictionary[:1] if dict_size > 1 else b"\x00"
        for d in (wrong, other_order, None):
            rc, res = run_members(lib, [m], [len(data)], ZLIB, d, **kw)
            assert res[0][0] == BAD_FRAME and res[0][2] == 0, (dict_size, res[0][:6])
        rc, res = run_members(lib, [plain, m], [len(data)] * 2, ZLIB, dictionary, **kw)   # a dictionary given and no FDICT: the documented difference
        assert (res[0][0], res[1][0]) == (BAD_FRAME, OK) and zlib_verdict(plain, ZLIB, dictionary)[0]
        rc, res = run_members(lib, [plain], [len(data)], ZLIB, None, **kw)
        assert res[0][0] == OK and res[0][6] == data
    # raw and gzip items that need the dictionary (its last 32768 bytes are the history)
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY, zdict=dictionary)
    raw = c.compress(data) + c.flush()
    gz = gzip_member(gzip_header(8, name=b"d"), raw, data)
    for framing, member, head in ((RAW, raw, 0), (GZIP, gz, 12)):
        rc, res = run_members(lib, [member], [len(data)], framing, dictionary, dict_lead=dict_size & 3)
        assert res[0][:5] == (OK, res[0][1], len(data), len(member), head) and res[0][6] == data and res[0][5] == checksum(framing, data), res[0][:6]
        if dict_size >= 3:   # (zlib's match finder does not reach into a shorter one)
            rc, res = run_members(lib, [member], [len(data)], framing, None)
            assert res[0][0] == DISTANCE, res[0][:6]


# ---- verdicts and edges -------------------------------------------------------------------------------------------------------------------------
def check_cuts(lib, big):
    """Every accept case cut at every byte (the copies lie back to back: what follows an item's end is the member's own next byte): 14 below
    head_size, else 12; a prefix is written. -> cuts."""
    total = 0
    for name, framing, m, head, dictionary in accept_cases(big):
        ok, want, used = zlib_verdict(m, framing, dictionary)
        assert ok and used == len(m), name
        cuts = list(range(len(m)))
        rc, res = run_members(lib, [m] * len(cuts), [len(want)] * len(cuts), framing, dictionary, src_sizes=cuts)
        assert rc == len(cuts)
        for cut, r in zip(cuts, res):
            assert r[0] == (BAD_FRAME if cut < head else STREAM_END), (name, cut, r[:6])
            assert r[6] == want[:r[2]] and r[3] <= cut, (name, cut, r[:6])
            assert not zlib_verdict(m[:cut], framing, dictionary)[0], (name, cut)
        rc, res = run_members(lib, [m, m + b"trailing bytes"], [len(want)] * 2, framing, dictionary)   # bytes behind the trailer are not an error
        assert rc == 0 and res[0][:6] == res[1][:6] and res[1][3] == len(m), (name, res[0][:6], res[1][:6])
        total += len(cuts)
    return total


def check_trailers(lib):
    """Every trailer byte flipped: gzip 15 for the CRC-32's bytes and 16 for ISIZE's, zlib 15; both wrong is 15. A payload byte of a stored block
    flipped: it decodes, 15, and `check` is the checksum of what was written. Then check_host_gaps."""
    for framing, m, foot in ((GZIP, gzip_member(gzip_header(0)), 8), (ZLIB, zlib_member(BODY_TEXT), 4)):
        muts = []
        for i in range(foot):
            x = bytearray(m)
            x[len(m) - foot + i] ^= 0x10
            muts.append(bytes(x))
        both = bytearray(m)
        both[-1] ^= 1
        both[-foot] ^= 1
        rc, res = run_members(lib, muts + [bytes(both), m], [len(BODY_TEXT)] * (foot + 2), framing)
        assert rc == foot + 1 and res[-1][0] == OK
        for i, r in enumerate(res[:-1]):
            assert r[0] == (BAD_ISIZE if framing == GZIP and 4 <= i < 8 else BAD_CHECK), (framing, i, r[:6])
            assert r[6] == BODY_TEXT and r[5] == checksum(framing, BODY_TEXT) and r[3] == len(m), (framing, i, r[:6])
            assert not zlib_verdict(muts[i] if i < foot else bytes(both), framing)[0]
    data = corpus.noise(700, 3).tobytes()
    for framing, m, head in ((GZIP, gzip_member(gzip_header(0), I.zlib_raw(data, 0, zlib.Z_DEFAULT_STRATEGY), data), 10), (ZLIB, zlib_member(data, 0), 2)):
        x = bytearray(m)
        x[head + 5 + 333] ^= 0x40   # (behind the stored block's five header bytes)
        wrote = bytearray(data)
        wrote[333] ^= 0x40
        rc, res = run_members(lib, [bytes(x)], [len(data)], framing)
        assert res[0][0] == BAD_CHECK and res[0][6] == bytes(wrote) and res[0][5] == checksum(framing, bytes(wrote)), res[0][:6]
    check_host_gaps(lib)


def check_host_gaps(lib):
    """A host destination whose ranges lie CANARY bytes apart (run_members), in both framings: an item without room, one whose stream breaks part-way
    (its second block is of type 3: the first block's bytes are written), one with a byte too little room, the others filling their ranges
    exactly. run_members holds every byte in front of, between and behind the items' out_size bytes to the canary; here the verdicts, what was
    written of the damaged items, and the sound items' bytes."""
    datas = [corpus.text_like(n, 90 + k).tobytes() for k, n in enumerate((300, 450, 0, 700, 380, 520))]
    for framing in (GZIP, ZLIB):
        members = [member_of(framing, d, 6) for d in datas]
        c = zlib.compressobj(6, zlib.DEFLATED, WBITS[framing])
        first = c.compress(datas[3][:333]) + c.flush(zlib.Z_FULL_FLUSH)   # (ends on a byte boundary: the next block's header is the next byte's low bits)
        broken = bytearray(first + c.compress(datas[3][333:]) + c.flush())
        assert zlib_verdict(bytes(broken), framing)[:2] == (True, datas[3])
        broken[len(first)] |= 6
        members[3] = bytes(broken)
        caps = [len(d) for d in datas]
        caps[1] = 0
        caps[4] -= 1
        rc, res = run_members(lib, members, caps, framing, on_device=False)
        assert rc == 3 and [r[0] == OK for r in res] == [True, False, True, False, False, True], [r[:6] for r in res]
        assert res[1][2] == 0 and res[3][2] == 333 and res[3][6] == datas[3][:333], [r[:6] for r in res]
        assert res[4][2] <= caps[4] and res[4][6] == datas[4][:res[4][2]], res[4][:6]
        for k in (0, 2, 5):
            assert res[k][6] == datas[k] and res[k][2] == caps[k] and res[k][5] == checksum(framing, datas[k]), (framing, k, res[k][:6])


EDGE_SIZES = [0, 1, 255, 256, 257, 65535, 65536, 65537, 3 * 65536 + 1]


def member_of(framing, data, level):
    if framing == ZLIB:
        return zlib_member(data, level)
    return gzip_member(gzip_header(0), I.zlib_raw(data, level, zlib.Z_DEFAULT_STRATEGY), data)


def edge_members(framing):
    """Stored and compressed members of random bytes and of 0xFF bytes (Adler-32's modular worst case) at the sizes where the slices and the
    rounds of zh_check_members change."""
    out = []
    for n in EDGE_SIZES:
        for kind, data in (("random", corpus.noise(n, n & 255).tobytes()), ("ff", b"\xff" * n)):
            for level in (0, 6):
                out.append(("%s_%d_l%d" % (kind, n, level), member_of(framing, data, level), data))
    return out


def check_checksum_edges(lib, framing):
    """Items with exactly the room they need (those up to 16384 bytes lie several to a workgroup, the others take one each), then all of them with
    the largest room (every one takes a workgroup of its own)."""
    named = edge_members(framing)
    for caps in ([len(d) for _, _, d in named], [EDGE_SIZES[-1]] * len(named)):
        rc, res = run_members(lib, [m for _, m, _ in named], caps, framing)
        for (name, m, d), r in zip(named, res):
            assert r[0] == OK and r[6] == d and r[3] == len(m) and r[5] == checksum(framing, d), (name, r[:6], checksum(framing, d))
        assert rc == 0
    return len(named)


def mixed_members(framing):
    """Many outputs of 0 .. 600 bytes and three large ones: both forms of zh_check_members in one launch."""
    out = []
    for n in list(range(0, 601, 7)) + [599, 600, 256, 512]:
        d = (corpus.text_like if n & 1 else corpus.noise)(n, n).tobytes()
        out.append(("m%d" % n, member_of(framing, d, 6), d))
    for k, n in enumerate((SMALL_MAX + 1, 40001, 65536 + 300)):
        d = corpus.text_like(n, 50 + k).tobytes()
        out.insert(20 * k + 5, ("large%d" % n, member_of(framing, d, 6), d))
    return out


def check_mixed(lib):
    for framing in (GZIP, ZLIB):
        named = mixed_members(framing)
        rc, res = run_members(lib, [m for _, m, _ in named], [len(d) for _, _, d in named], framing)
        for (name, m, d), r in zip(named, res):
            assert r[0] == OK and r[6] == d and r[3] == len(m) and r[5] == checksum(framing, d), (name, r[:6])
        bad = [bytearray(m) for _, m, _ in named]   # ... and every trailer's checksum wrong
        for x in bad:
            x[-1 if framing == ZLIB else -5] ^= 1
        rc, res = run_members(lib, bad, [len(d) for _, _, d in named], framing)
        assert rc == len(named) and all(r[0] == BAD_CHECK for r in res)
    return len(named)


def check_mixed_strided(lib_path, is_emulator):
    """The same batches in a process of its own with ZULTRA_HIP_GRID_CAP=8: the workgroups of both forms (and the inflate kernel's waves) stride."""
    tests = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import inflate_member_cases as M\nfrom zultra_amd._ffi import Lib\nL = Lib(%r)\nL.is_emulator = %r\n"
            "M.check_mixed(L)\nprint('strided ok')\n") % (os.path.dirname(tests), tests, lib_path, bool(is_emulator))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ZULTRA_HIP_GRID_CAP="8"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "strided ok" in r.stdout, r.stdout + r.stderr


def check_alignment(lib):
    """Source, destination and device dictionary 1, 2 and 3 bytes into a dword: the results of the aligned run."""
    dictionary = D.dictionary_of(corpus.text_like, 1000)
    data = dictionary[-200:] + corpus.text_like(1500, 7).tobytes()
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY, zdict=dictionary)
    raw = c.compress(data) + c.flush()
    big = corpus.text_like(40000, 8).tobytes()
    sets = [(GZIP, None, [gzip_member(gzip_header(0)), gzip_member(gzip_header(0), I.zlib_raw(big, 6, zlib.Z_DEFAULT_STRATEGY), big), gzip_member(gzip_header(2 | 8, name=b"name"))]),
            (ZLIB, None, [zlib_member(BODY_TEXT), zlib_member(big), zlib_member(big[:257], 0)]),
            (ZLIB, dictionary, [zlib_member(data, 6, dictionary), zlib_member(data[:300], 6, dictionary)]),
            (GZIP, dictionary, [gzip_member(gzip_header(0), raw, data)])]
    for framing, d, members in sets:
        caps = [len(zlib_verdict(m, framing, d)[1]) if framing != GZIP or d is None else len(data) for m in members]
        rc0, ref = run_members(lib, members, caps, framing, d)
        assert rc0 == 0 and all(r[5] == checksum(framing, r[6]) and r[2] == cap for r, cap in zip(ref, caps)), [r[:6] for r in ref]
        for lead in (1, 2, 3):
            for kw in (dict(src_lead=lead), dict(dst_lead=lead), dict(dict_lead=lead), dict(src_lead=lead, dst_lead=4 - lead, dict_lead=(lead + 1) & 3)):
                assert run_members(lib, members, caps, framing, d, **kw) == (rc0, ref), (framing, lead, kw)


def check_concatenated(lib):
    """Five gzip members in one buffer, walked with src_used, one call per member: the joined output is gzip.decompress of the buffer."""
    parts = [corpus.text_like(n, n).tobytes() for n in (1, 3000, 0, 20000, 700)]
    buf = b"".join(gzip.compress(p, 6, mtime=k) for k, p in enumerate(parts))
    want = gzip.decompress(buf)
    src = np.frombuffer(buf, dtype=np.uint8).copy()
    dst = np.zeros(len(want) + 1, dtype=np.uint8)
    at = written = calls = 0
    while at < len(buf):
        rc, res, _ = lib.inflate_members(src, len(src), dst, len(dst), None, 0, GZIP, [(at, len(buf) - at, written, len(want) - written)])
        assert rc == 0 and int(res[0]["src_used"]) > 0, (calls, res[0])
        at += int(res[0]["src_used"])
        written += int(res[0]["out_size"])
        calls += 1
    assert calls == 5 and dst[:written].tobytes() == want == b"".join(parts)


def check_equivalence(lib):
    """framing == 0: the results and the bytes of zultra_hip_inflate_streams and zultra_hip_inflate_streams_dict, accept and reject cases alike, and
    head_size = check = 0."""
    streams = [s for _, s, _ in I.hand_matches() + I.hand_after_literals()] + [c[1] for c in I.dynamic_good()] + [c[1] for c in I.hand_bad()] + [c[1] for c in I.dynamic_bad()]
    caps = [600 + (k & 1) * 700 for k in range(len(streams))]
    caps[3] = 10   # (reason 13)
    for dev in (True, False):
        rc0, plain = I.run_streams(lib, streams, caps, dev)
        rc, res = run_members(lib, streams, caps, RAW, None, on_device=dev)
        assert rc == rc0 and [r[:4] + (0, 0) + r[6:] for r in res] == [p[:4] + (0, 0) + p[4:] for p in plain] and all(r[4:6] == (0, 0) for r in res)
    assert {p[0] for p in plain} >= {0, 1, 2, 3, 4, 13}
    n = len(streams)
    for h, group in D.by_history(D.hand_streams())[-2:]:
        ds = [s for _, _, s, _ in group] + [s[:-1] for _, _, s, _ in group]
        caps = [len(w) for _, _, _, w in group] * 2
        rc0, plain = D.run_dict(lib, ds, caps, h, dict_lead=1)
        rc, res = run_members(lib, ds, caps, RAW, h, dict_lead=1)
        assert rc == rc0 == len(group) and [r[:4] + r[6:] for r in res] == plain and all(r[4:6] == (0, 0) for r in res)
        n += len(ds)
    return n


# ---- the library's own output, the host API, arguments -------------------------------------------------------------------------------------------
def check_own_files(lib, nfiles):
    """A files batch of the library's coder framed as gzip and as zlib on the host, uploaded, inflated and checked device to device."""
    sizes = [I.FILE_SIZES[i % len(I.FILE_SIZES)] for i in range(nfiles)]
    parts = [(corpus.json_like, corpus.text_like)[i & 1](n, 100 + i).tobytes() for i, n in enumerate(sizes)]
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    ctx = lib.files_context(8191, nfiles)
    try:
        file_off = ctx.compress_files(np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), offsets, sizes)
        stream = ctx.stream_read(int(file_off[-1])).tobytes()
    finally:
        ctx.close()
    raws = [stream[int(file_off[i]): int(file_off[i + 1])] for i in range(nfiles)]
    for framing in (GZIP, ZLIB):
        if framing == GZIP:
            members = [gzip_member(gzip_header(8 if i & 1 else 0, name=b"f%d" % i), r, p) for i, (r, p) in enumerate(zip(raws, parts))]
        else:
            members = [b"\x78\x9c" + r + zlib.adler32(p).to_bytes(4, "big") for r, p in zip(raws, parts)]
        assert all(zlib_verdict(m, framing)[:2] == (True, p) for m, p in list(zip(members, parts))[:20])
        rc, res = run_members(lib, members, sizes, framing)
        assert rc == 0, [r[:6] for r in res if r[0]][:4]
        for i, (m, p, r) in enumerate(zip(members, parts, res)):
            assert r[6] == p and r[3] == len(m) and r[5] == checksum(framing, p), (i, r[:6])
    return nfiles


def check_host_api(lib, size):
    """zultra_memory_decompress_batch in the three framings against zultra_memory_decompress member by member; one bad member among good ones;
    trailing bytes fail a member."""
    datas = [corpus.text_like(size, 31).tobytes(), corpus.json_like(size // 3, 32).tobytes(), b"x", corpus.noise(700, 33).tobytes()]
    for f in (RAW, ZLIB, GZIP):
        packed = [lib.memory_compress(np.frombuffer(d, dtype=np.uint8), f, 32768) for d in datas]
        assert all(p is not None for p in packed)
        bad = bytearray(packed[1])
        bad[len(bad) // 2] ^= 4
        if f == RAW:   # (nothing checks a raw stream's bytes: cut short instead)
            bad = bad[:-1]
        blob = [packed[0], bytes(bad), packed[2], packed[3], packed[3] + b"\0"]
        caps = [len(datas[0]), len(datas[1]) + 50, 1, 700, 700]
        members, at = [], 0
        for b in blob:
            members.append((at, len(b)))
            at += len(b)
        rc, outs = lib.memory_decompress_batch(b"".join(blob), members, f, caps)
        single = [lib.memory_decompress(b, f, cap) for b, cap in zip(blob, caps)]
        assert outs == single and outs[0] == datas[0] and outs[2] == b"x" and outs[3] == datas[3] and outs[4] is None, (f, rc)
        assert outs[1] is None and rc == 2, (f, rc)
        rc, outs = lib.memory_decompress_batch(b"".join(blob), members, f, [c - 1 if k == 0 else c for k, c in enumerate(caps)])   # one byte short of room
        assert rc == 3 and outs[0] is None and outs[2] == b"x"
    dictionary = D.dictionary_of(corpus.text_like, 5000, 34)
    data = dictionary[-100:] + datas[1]
    for f in (RAW, ZLIB, GZIP):
        p = lib.memory_compress(np.frombuffer(data, dtype=np.uint8), f, 32768, dictionary=dictionary)
        rc, outs = lib.memory_decompress_batch(p + p, [(0, len(p)), (len(p), len(p))], f, [len(data)] * 2, dictionary)
        assert rc == 0 and outs == [data, data] == [lib.memory_decompress_dict(p, f, len(data), dictionary)] * 2, (f, rc)
        rc, outs = lib.memory_decompress_batch(p, [(0, len(p))], f, [len(data)], None)
        assert rc == 1 and outs == [None], f
    assert lib.memory_decompress_batch(b"abc", [], RAW, [])[0] == -1                       # n == 0
    assert lib.memory_decompress_batch(b"abc", [(0, 3)], ZLIB | GZIP, [10])[0] == -1       # both framings
    assert lib.memory_decompress_batch(b"abc", [(1, 3)], RAW, [10])[0] == -1               # a member past nIn


def check_bad_arguments(lib):
    m = gzip_member(gzip_header(0))
    src = np.frombuffer(m, dtype=np.uint8).copy()
    dst = np.zeros(400, dtype=np.uint8)
    n, cap = len(src), len(BODY_TEXT)
    call = lambda items, framing=GZIP, d=None, dn=0: lib.inflate_members(src, n, dst, 400, d, dn, framing, items)[0]
    assert call([(0, n, 0, cap)], ZLIB | GZIP) == -1                                  # both framing bits
    for framing in (4, 8, 5, 6, 0x100, 0x80000000):
        assert call([(0, n, 0, cap)], framing) == -1                                  # any other bit
    assert call(np.zeros((0, 4), dtype=np.uint64)) == -1                              # n == 0
    assert call([(0, n, 0, cap), (0, n, cap - 1, cap)]) == -1                         # destination ranges overlap
    assert call([(0, n, 50, cap), (0, n, 0, 51)]) == -1
    assert call([(1, n, 0, cap)]) == -1                                               # an item past src_size
    assert call([(0, n, 401 - cap, cap)]) == -1                                       # ... past dst_size
    assert call([(0, n, 0, cap)], GZIP, None, 40) == -1                               # a NULL dictionary of 40 bytes
    assert not dst.any(), "a refused call has written"
    h = D.history(40, 14)
    buf = V.DeviceCopy(lib, np.frombuffer(b"\0" * 200 + h + b"\0" * 200, dtype=np.uint8).copy())   # a device dictionary inside a device destination range
    dsrc = V.DeviceCopy(lib, src)
    try:
        on_dev = lambda dst_off, dict_at: lib.inflate_members(dsrc.ptr, n, buf.ptr, 440, buf.ptr + dict_at, 40, GZIP, [(0, n, dst_off, cap)])[0]
        assert on_dev(239, 200) == -1 and on_dev(201 - cap, 200) == -1
        assert I.device_read(lib, buf, 440).tobytes() == b"\0" * 200 + h + b"\0" * 200, "a refused call has written"
        assert on_dev(240, 200) == 0 and on_dev(200 - cap, 200) == 0
        back = I.device_read(lib, buf, 440).tobytes()
        assert back[240:240 + cap] == BODY_TEXT and back[200 - cap:200] == BODY_TEXT and back[200:240] == h
    finally:
        buf.free()
        dsrc.free()
    assert call([(0, n, 0, cap), (0, n, cap, cap)]) == 0 and dst[:cap].tobytes() == dst[cap:2 * cap].tobytes() == BODY_TEXT
