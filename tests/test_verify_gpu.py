"""GPU (MI355X): zultra_hip_verify_device — the inflate-and-compare kernel of zultra_amd/csrc/zh_verify.h — in the product library: clean streams
verify, corrupted streams get host zlib's verdict and the right sub-block, the host API and the command-line tool verify every batch when asked.
The cases are those of tests/test_verify_emu.py at full size (tests/verify_cases.py)."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import corpus
import verify_cases as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import zultra_amd
    L = zultra_amd.lib()            # raises if the .so is missing: no fallback
    assert L.device_count() >= 1, "no HIP device visible"
    L.is_emulator = False   # (verify_cases.DeviceCopy: device memory comes from hipMalloc)
    return L


@pytest.mark.parametrize("case", V.CLEAN_GPU, ids=lambda c: c[0])
def test_clean_streams_verify(gpu, case):
    V.check_clean(gpu, *case)


@pytest.mark.parametrize("phase", range(8))
def test_every_start_phase_with_and_without_bfinal(gpu, phase):
    d = lambda: V.text_noise_text(45000, 33000)
    V.check_clean(gpu, "phase%d" % phase, d, 32768, 32768, phase=phase, final=True)
    V.check_clean(gpu, "phase%d/open" % phase, d, 32768, 32768, phase=phase, final=False)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_input_is_reachable_in_every_data_mode(gpu, mode):
    V.check_clean(gpu, "mode%d" % mode, lambda: corpus.text_like(300000, 8), 65536, 65536, mode=mode)


def test_stitch_armed_with_the_batch_is_verified(gpu):
    data = corpus.text_like(200000, 12)
    blocks = V.stream_blocks(len(data), 65536)
    ctx = gpu.context(65536, len(blocks))
    try:
        ctx.stitch_with_batch(len(blocks) - 1, 3)
        V.compress(gpu, ctx, data, blocks)
        r = ctx.verify()   # (no stitch call in between: the batch brought its stitch)
        assert r["rc"] == 0 and r["verified_bytes"] == len(data), r
    finally:
        ctx.close()


def test_nothing_stitched_is_an_error_not_a_verdict(gpu):
    from zultra_amd._ffi import ZultraError
    data = corpus.text_like(30000, 2)
    ctx = gpu.context(32768, 1)
    try:
        with pytest.raises(ZultraError):
            ctx.verify()
        V.compress(gpu, ctx, data, [(0, 0, len(data))])
        with pytest.raises(ZultraError):
            ctx.verify()   # (compressed, not stitched)
        ctx.stitch_device(0, 0)
        assert ctx.verify()["rc"] == 0
    finally:
        ctx.close()


def test_preset_dictionary_through_the_host_api(gpu):
    d = corpus.text_like(100000, 4)
    dic = corpus.text_like(20000, 4)
    gpu.set_verify(0)
    plain = gpu.memory_compress(d, 0, 32768, dictionary=dic)
    gpu.set_verify(1)
    try:
        before = gpu.verified_bytes()
        got = gpu.memory_compress(d, 0, 32768, dictionary=dic)
        assert got == plain
        assert gpu.verified_bytes() - before == len(d)
        o = zlib.decompressobj(-15, zdict=dic.tobytes())
        assert o.decompress(got) == d.tobytes()
    finally:
        gpu.set_verify(0)


def test_files_mode(gpu):
    V.check_files(gpu, 61)


@pytest.mark.parametrize("case", V.FLIPS_GPU, ids=lambda c: c[0])
def test_single_bit_flips_get_zlibs_verdict(gpu, case):
    V.check_flips(gpu, *case, seed=20260117)


def test_targeted_flips_get_zlibs_verdict(gpu):
    """BFINAL of a middle and of the last sub-block, both BTYPE bits, HLIT / HDIST / HCLEN, a stored LEN and NLEN bit, a stored byte, the last valid bit."""
    n, _ = V.check_flips(gpu, "text_noise_text", lambda: V.text_noise_text(65536, 32768), 32768, 32768, 20, False, seed=7, targeted=True)
    assert n >= 20 + 11


def test_flip_reports_are_the_recorded_ones(gpu):
    """reason, sub-block, input offset and stream bit of every report for the fixed flips of verify_cases.flip_reports (the end of the data and the
    last sub-block's header among them) are those of tests/golden/verify_flip_reports.json, recorded before the decoder was shared with the inflate
    kernels."""
    V.check_flip_reports(gpu)


def _uneven_stream(lib, d, flags, bs):
    s = lib.stream(flags, bs)
    out, at = b"", 0
    for step in (1, 70001, 65536, 1 << 20, 3, len(d)):
        hi = min(len(d), at + step)
        st, o = s.compress(d[at:hi], hi == len(d))
        out += o
        at = hi
        if at == len(d):
            break
    s.end()
    return out


def test_host_api_memory_compress(gpu):
    d = corpus.mixed(3 << 20, 3)
    gpu.set_verify(0)
    before = gpu.verified_bytes()
    plain = gpu.memory_compress(d, 2, 65536)
    assert gpu.verified_bytes() == before          # off: the counter does not move
    gpu.set_verify(1)
    try:
        assert gpu.memory_compress(d, 2, 65536) == plain
        assert gpu.verified_bytes() - before == len(d)
    finally:
        gpu.set_verify(0)
    assert zlib.decompress(plain, 31) == d.tobytes()


def test_host_api_stream_in_uneven_chunks(gpu):
    d = corpus.mixed(3 << 20, 3)
    gpu.set_verify(0)
    plain = _uneven_stream(gpu, d, 2, 65536)
    gpu.set_verify(1)
    try:
        before = gpu.verified_bytes()
        assert _uneven_stream(gpu, d, 2, 65536) == plain
        assert gpu.verified_bytes() - before == len(d)
    finally:
        gpu.set_verify(0)


def test_host_api_two_lanes(gpu, monkeypatch):
    d = corpus.mixed(3 << 20, 3)
    gpu.set_verify(0)
    plain = gpu.memory_compress(d, 2, 65536)
    monkeypatch.setenv("ZULTRA_HIP_MEMORY_LANES", "2")
    gpu.set_verify(1)
    try:
        before = gpu.verified_bytes()
        assert gpu.memory_compress(d, 2, 65536) == plain
        assert gpu.verified_bytes() - before == len(d)
    finally:
        gpu.set_verify(0)


def test_host_stitch_path_is_verified_too(gpu, monkeypatch):
    d = corpus.mixed(1 << 20, 4)
    gpu.set_verify(0)
    plain = gpu.memory_compress(d, 2, 65536)
    monkeypatch.setenv("ZULTRA_HIP_HOST_STITCH", "1")
    monkeypatch.setenv("ZULTRA_HIP_MEMORY_LANES", "0")
    gpu.set_verify(1)
    try:
        before = gpu.verified_bytes()
        assert gpu.memory_compress(d, 2, 65536) == plain
        assert gpu.verified_bytes() - before == len(d)
    finally:
        gpu.set_verify(0)


def test_cli_verifies(gpu, tmp_path):
    import zultra_amd
    cli = os.path.join(os.path.dirname(zultra_amd.LIB_PATH), "zultra_amd_cli")
    d = corpus.text_like(500000, 9)
    src, dst = tmp_path / "in.bin", tmp_path / "out.gz"
    src.write_bytes(d.tobytes())
    r = subprocess.run([cli, "-c", "-v", "-b", "65536", str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "verified %d bytes on the device" % len(d) in r.stdout, r.stdout
    assert zlib.decompress(dst.read_bytes(), 31) == d.tobytes()
    r = subprocess.run([cli, "-v", "-b", "65536", str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "verified" not in r.stdout
