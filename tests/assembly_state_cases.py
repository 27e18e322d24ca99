"""Shared by tests/test_assembly_state_emu.py (CPU emulator build) and tests/test_assembly_state_gpu.py (product library on the MI355X): what the
context remembers of the stream buffer's content between the calls that assemble the last batch (the assembly record of zultra_amd/csrc/zh_device.hip,
DESIGN.md 3.7). Every assembling call is run alone behind a fresh batch and held to a reference that is not the code under test — the host stitcher
and host zlib for one stream, the reference's members (the `checker` fixture) for the files form, the framed members and the ZIP entries, the
stitcher's rule in Python for the phase table —, then behind every other call, where it must give the same bytes and leave a buffer that verifies."""
import ctypes as C

import numpy as np

import frame_member_cases as M
import inflate_file_cases as F
import verify_cases as V
import zip_cases as Z
from zultra_amd._ffi import BitState, ZultraError

MAX_BLOCK = 32768
NAMES = [b"a", b"bb.txt", b"d/c", b"noise.bin"]
KINDS = ("files", "blocks")
_PARTS, _SOLO = [], {}


def parts():
    if not _PARTS:
        _PARTS.extend([F.text(700, 950), F.text(64, 951), F.text(3000, 952), F.noise(500, 953)])
    return _PARTS


def total():
    return sum(len(p) for p in parts())


def open_ctx(lib, kind):
    return lib.files_context(8191, 4) if kind == "files" else lib.context(MAX_BLOCK, 4)


def batch(ctx, kind):
    """A fresh batch of the four parts. -> the offsets a files context's batch brings with it (None for a context of max-blocks)."""
    if kind == "files":
        return Z.compress_files(ctx, parts())
    M.compress(ctx, parts())
    return None


def raw_layout(checker):
    """The plain files form per the reference: (the streams end to end, where each starts)."""
    streams = [M.want_member(checker, p, M.RAW, MAX_BLOCK) for p in parts()]
    return b"".join(streams), [0] + [int(v) for v in np.cumsum([len(s) for s in streams])]


# ---- the operations: run(ctx, checker) -> what the call returned and the bytes it left ---------------------------------------------------------------
def _stitch(phase, final):
    def run(ctx, checker):
        end_bit, nacc = ctx.stitch_device(final, phase)
        return (end_bit, nacc, ctx.stream_read((end_bit + 7) // 8).tobytes())
    return run


def _stitch_files(ctx, checker):
    off = ctx.stitch_files()
    return (tuple(int(v) for v in off), ctx.stream_read(int(off[-1])).tobytes())


def _framed(framing):
    def run(ctx, checker):
        buf, mem = M.framed(ctx, checker, parts(), framing, MAX_BLOCK, eof=framing == M.BGZF)     # (held to the reference member by member)
        return (buf, mem.tobytes())
    return run


def _phase_table(ctx, checker):
    ends, failed = (C.c_uint64 * 8)(), C.c_uint32(7)
    f = ctx.lib.L.zultra_hip_stitch_phase_table
    f.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    assert f(ctx.h, ends, C.byref(failed)) == 0
    return (tuple(int(v) for v in ends), int(failed.value))


def _zipped(ctx, checker):
    ent, local, central = Z.zipped(ctx, checker, parts(), NAMES, MAX_BLOCK)     # (held to the expected local and central part)
    return (ent.tobytes(), local, central)


STITCH0, STITCH3 = (0, 3), (3, -1)      # (phase, final block) of the two stitches: at phase 0 with the final block, at phase 3 and open
OPS = {
    "stitch0": (("blocks",), _stitch(*STITCH0)),
    "stitch3": (("blocks",), _stitch(*STITCH3)),
    "files": (KINDS, _stitch_files),
    "gzip": (KINDS, _framed(M.GZIP)),
    "bgzf": (KINDS, _framed(M.BGZF)),
    "table": (("blocks",), _phase_table),
    "zip": (KINDS, _zipped),
}


def ops_of(kind):
    return [name for name, (kinds, _) in OPS.items() if kind in kinds]


def run(name, ctx, checker):
    return OPS[name][1](ctx, checker)


def check_verifies(ctx, after):
    """verify() behind `after`: the whole input, no bad sub-block — but a refusal behind the phase table, which rewrites the items and moves no bit."""
    if after == "table":
        try:
            ctx.verify()
        except ZultraError:
            return
        raise AssertionError("verify() took the items of a phase-table call for a stitched batch")
    v = ctx.verify()
    assert v["rc"] == 0 and v["bad_subblocks"] == 0 and v["verified_bytes"] == total(), (after, v)


# ---- each operation alone, against its reference ------------------------------------------------------------------------------------------------------
def _check_stitch(ctx, got, phase, final):
    data = b"".join(parts())
    offs = [0] + [int(v) for v in np.cumsum([len(p) for p in parts()])[:-1]]
    want, st = ctx.stitch(M.u8(data), offs, MAX_BLOCK, final, state=BitState(0, phase), finish=False)      # (the serial host stitcher)
    end_bit, nacc, buf = got
    full = len(want)
    assert nacc == st.nacc and (end_bit + 7) // 8 == full + (1 if st.nacc else 0) and buf[:full] == want, (phase, end_bit, full, st.nacc)
    if st.nacc:
        assert buf[full] == st.acc & 0xff, phase
    if phase == 0 and final >= 0:
        assert V.inflates_to(buf, data)


def solo(lib, checker, kind):
    """name -> the result of every operation valid on a context of `kind`, each alone behind a fresh batch and held to its reference. Computed once."""
    key = (lib.path, kind)
    if key in _SOLO:
        return _SOLO[key]
    raw, raw_off = raw_layout(checker)
    out = {}
    ctx = open_ctx(lib, kind)
    try:
        for name in ops_of(kind):
            batch(ctx, kind)
            got = out[name] = run(name, ctx, checker)
            if name in ("stitch0", "stitch3"):
                _check_stitch(ctx, got, *(STITCH0 if name == "stitch0" else STITCH3))
            elif name == "files":
                assert got == (tuple(raw_off), raw), kind
            elif name == "table":
                subs = ctx.subblocks()[0]
                assert got == (tuple(V.plan(subs, MAX_BLOCK, p)[1] for p in range(8)), 0), got
            check_verifies(ctx, name)
        if kind == "blocks":
            assert (out["table"][0][0], out["table"][0][3]) == (out["stitch0"][0], out["stitch3"][0])
    finally:
        ctx.close()
    _SOLO[key] = out
    return out


def check_solo(lib, checker, kind):
    return len(solo(lib, checker, kind))


# ---- every ordered pair ---------------------------------------------------------------------------------------------------------------------------
def check_pairs(lib, checker, kind, first):
    """One batch, then for every B valid on the context: `first`, B — B's result is its solo result byte for byte and the buffer verifies behind it."""
    want = solo(lib, checker, kind)
    ctx = open_ctx(lib, kind)
    try:
        batch(ctx, kind)
        for second in ops_of(kind):
            assert run(first, ctx, checker) == want[first], (kind, first, "before " + second)
            assert run(second, ctx, checker) == want[second], (kind, first, second)
            check_verifies(ctx, second)
    finally:
        ctx.close()
    return len(ops_of(kind))


# ---- what a batch brings with it ------------------------------------------------------------------------------------------------------------------
def check_armed_stitch(lib, checker, armed):
    """A batch of max-blocks whose stitch was armed (zultra_hip_stitch_with_batch) at STITCH0 or STITCH3: it verifies as it comes, the stitch_device call with the
    same arguments hands out that stitch without a launch (the batch's stitch_ms stands), the other one stitches again."""
    want = solo(lib, checker, "blocks")
    name, other = ("stitch0", "stitch3") if armed == 0 else ("stitch3", "stitch0")
    phase, final = STITCH0 if armed == 0 else STITCH3
    assert phase == armed
    ctx = open_ctx(lib, "blocks")
    try:
        ctx.stitch_with_batch(final, phase)
        batch(ctx, "blocks")
        check_verifies(ctx, name)
        ms = ctx.timing()["stitch_ms"]
        assert run(name, ctx, checker) == want[name], armed
        assert ctx.timing()["stitch_ms"] == ms, "the call that takes the batch's stitch has stitched again"
        check_verifies(ctx, name)
        assert run(other, ctx, checker) == want[other], armed
        check_verifies(ctx, other)
        assert run(name, ctx, checker) == want[name], armed
        # (one batch only: the next one comes without)
        batch(ctx, "blocks")
        try:
            ctx.verify()
            raise AssertionError("a batch without a stitch verified")
        except ZultraError:
            pass
        assert run(name, ctx, checker) == want[name], armed
    finally:
        ctx.close()


def check_files_batch_brings_its_offsets(lib, checker):
    want = solo(lib, checker, "files")
    raw, raw_off = raw_layout(checker)
    ctx = open_ctx(lib, "files")
    try:
        brought = batch(ctx, "files")
        assert [int(v) for v in brought] == raw_off
        check_verifies(ctx, "files")
        assert run("files", ctx, checker) == want["files"] == (tuple(raw_off), raw)
        assert run("gzip", ctx, checker) == want["gzip"]
        assert ctx.stream_read(len(raw)).tobytes() != raw
        assert run("files", ctx, checker) == want["files"]          # (the same offsets, the plain bytes back)
        check_verifies(ctx, "files")
    finally:
        ctx.close()


# ---- the buffer overwritten behind the library's back ---------------------------------------------------------------------------------------------
def marker(n):
    return bytes((i * 13 + 7) & 255 for i in range(n))


def check_explicit_assembly_is_redone(lib, checker):
    want = solo(lib, checker, "blocks")
    ctx = open_ctx(lib, "blocks")
    try:
        batch(ctx, "blocks")
        assert run("files", ctx, checker) == want["files"]
        mark = marker(len(want["files"][1]) + 64)
        ctx.stream_write(mark)
        assert ctx.stream_read(len(mark)).tobytes() == mark
        assert run("files", ctx, checker) == want["files"], "an explicit assembly asked for again was handed out, not redone"
        check_verifies(ctx, "files")
    finally:
        ctx.close()


def check_zip_reuses_the_assembled_buffer(lib, checker, kind):
    """zip_members behind the plain files form — a files batch's own, an explicit stitch_files on a context of max-blocks — gathers from the buffer as it
    stands: with a marker written over it the local part carries the marker's bytes in every entry's data range and the solo result's everywhere else."""
    want = solo(lib, checker, kind)
    _, raw_off = raw_layout(checker)
    ent, solo_local, solo_central = want["zip"]
    ctx = open_ctx(lib, kind)
    try:
        batch(ctx, kind)
        if kind == "blocks":
            assert run("files", ctx, checker) == want["files"]
        mark = marker(raw_off[-1] + 64)
        ctx.stream_write(mark)
        rc, got_ent, local, central, central_at = ctx.zip_members(NAMES)
        assert rc == 0 and got_ent.tobytes() == ent and (local, central) == (len(solo_local), len(solo_central))
        got, expect, at = ctx.zip_read(local).tobytes(), bytearray(solo_local), 0
        for i, name in enumerate(NAMES):
            at += 30 + len(name)
            n = raw_off[i + 1] - raw_off[i]
            assert solo_local[at: at + n] != mark[raw_off[i]: raw_off[i + 1]]
            expect[at: at + n] = mark[raw_off[i]: raw_off[i + 1]]
            at += n
        assert at == local and got == bytes(expect), kind
        assert ctx.zip_read(central, central_at).tobytes() == solo_central
    finally:
        ctx.close()
