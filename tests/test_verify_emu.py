"""CPU (no GPU needed): zultra_hip_verify_device — the inflate-and-compare kernel of zultra_amd/csrc/zh_verify.h — in the lock-step emulator
build of the product's sources: clean streams verify, corrupted streams get host zlib's verdict and the right sub-block, and the host API
verifies every batch when asked. tests/test_verify_gpu.py runs the same cases, larger, on the MI355X."""
import os
import sys
import zlib

import numpy as np
import pytest

import corpus
import verify_cases as V

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def emu():
    import build_emu
    from zultra_amd._ffi import Lib
    L = Lib(build_emu.build())
    L.is_emulator = True    # (verify_cases.DeviceCopy: device memory is host memory)
    return L


@pytest.mark.parametrize("case", V.CLEAN_EMU, ids=lambda c: c[0])
def test_clean_streams_verify(emu, case):
    V.check_clean(emu, *case)


@pytest.mark.parametrize("phase", range(8))
def test_every_start_phase_with_and_without_bfinal(emu, phase):
    d = lambda: V.text_noise_text(1500, 700)
    V.check_clean(emu, "phase%d" % phase, d, 1300, 32768, phase=phase, final=True)
    V.check_clean(emu, "phase%d/open" % phase, d, 1300, 32768, phase=phase, final=False)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_input_is_reachable_in_every_data_mode(emu, mode):
    V.check_clean(emu, "mode%d" % mode, lambda: corpus.text_like(5000, 8), 2000, 32768, mode=mode)


def test_stitch_armed_with_the_batch_is_verified(emu):
    data = corpus.text_like(5000, 12)
    blocks = V.stream_blocks(len(data), 2000)
    ctx = emu.context(32768, len(blocks))
    try:
        ctx.stitch_with_batch(len(blocks) - 1, 3)
        V.compress(emu, ctx, data, blocks)
        r = ctx.verify()   # (no stitch call in between: the batch brought its stitch)
        assert r["rc"] == 0 and r["verified_bytes"] == len(data), r
    finally:
        ctx.close()


def test_nothing_stitched_is_an_error_not_a_verdict(emu):
    from zultra_amd._ffi import ZultraError
    data = corpus.text_like(3000, 2)
    ctx = emu.context(32768, 1)
    try:
        with pytest.raises(ZultraError):
            ctx.verify()
        V.compress(emu, ctx, data, [(0, 0, len(data))])
        with pytest.raises(ZultraError):
            ctx.verify()   # (compressed, not stitched)
        ctx.stitch_device(0, 0)
        assert ctx.verify()["rc"] == 0
        import ctypes as C
        tab = (C.c_uint64 * 8)()
        assert emu.L.zultra_hip_stitch_phase_table(C.c_void_p(ctx.h), tab, None) == 0
        with pytest.raises(ZultraError):
            ctx.verify()   # (the phase table rewrote the items)
    finally:
        ctx.close()


def test_preset_dictionary_through_the_host_api(emu):
    d = corpus.text_like(6000, 4)
    dic = corpus.text_like(3000, 4)
    emu.set_verify(0)
    plain = emu.memory_compress(d, 0, 32768, dictionary=dic)
    emu.set_verify(1)
    try:
        before = emu.verified_bytes()
        got = emu.memory_compress(d, 0, 32768, dictionary=dic)
        assert got == plain
        assert emu.verified_bytes() - before == len(d)
        o = zlib.decompressobj(-15, zdict=dic.tobytes())
        assert o.decompress(got) == d.tobytes()
    finally:
        emu.set_verify(0)


def test_files_mode(emu):
    V.check_files(emu, 2)


@pytest.mark.parametrize("case", V.FLIPS_EMU, ids=lambda c: c[0])
def test_single_bit_flips_get_zlibs_verdict(emu, case):
    V.check_flips(emu, *case, seed=20260117)


def test_targeted_flips_get_zlibs_verdict(emu):
    """BFINAL of a middle and of the last sub-block, both BTYPE bits, HLIT / HDIST / HCLEN, a stored LEN and NLEN bit, a stored byte, the last valid bit."""
    n, _ = V.check_flips(emu, "text_noise_text", lambda: V.text_noise_text(2000, 2000), 2000, 32768, 4, False, seed=7, targeted=True)
    assert n >= 4 + 11


def test_flip_reports_are_the_recorded_ones(emu):
    """reason, sub-block, input offset and stream bit of every report for the fixed flips of verify_cases.flip_reports (the end of the data and the
    last sub-block's header among them) are those of tests/golden/verify_flip_reports.json, recorded before the decoder was shared with the inflate
    kernels."""
    V.check_flip_reports(emu)


def test_host_api_verifies_every_batch(emu, monkeypatch):
    d = corpus.mixed(9000, 3)
    emu.set_verify(0)
    before = emu.verified_bytes()
    plain = emu.memory_compress(d, 2, 32768)
    assert emu.verified_bytes() == before          # off: the counter does not move
    emu.set_verify(1)
    try:
        assert emu.memory_compress(d, 2, 32768) == plain
        assert emu.verified_bytes() - before == len(d)
        # the stream API in uneven chunks
        before = emu.verified_bytes()
        s = emu.stream(2, 32768)
        out = b""
        for lo, hi in ((0, 1), (1, 4000), (4000, 4001), (4001, len(d))):
            st, o = s.compress(d[lo:hi], hi == len(d))
            out += o
        s.end()
        assert out == plain and emu.verified_bytes() - before == len(d)
        # the host stitcher's path: the batch is stitched on the device as well, for the check
        monkeypatch.setenv("ZULTRA_HIP_HOST_STITCH", "1")
        monkeypatch.setenv("ZULTRA_HIP_MEMORY_LANES", "0")
        before = emu.verified_bytes()
        assert emu.memory_compress(d, 2, 32768) == plain
        assert emu.verified_bytes() - before == len(d)
    finally:
        emu.set_verify(0)


def test_environment_variable_turns_it_on(emu, tmp_path):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import corpus\nfrom zultra_amd._ffi import Lib\nL = Lib(%r)\n"
            "d = corpus.text_like(3000, 1)\nassert L.memory_compress(d, 2, 32768) is not None\nprint(L.verified_bytes())\n") % (root, os.path.join(root, "tests"), emu.path)
    for val, want in (("1", "3000"), ("0", "0")):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ZULTRA_HIP_VERIFY=val), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.strip() == want, r.stdout + r.stderr
