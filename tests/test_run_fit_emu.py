"""CPU (no GPU needed): the one function that decides how many staggered runs a batch is cut into (zultra_hip_runs_for), against the rule as its comment states
it, and an emulator batch whose run count is what it was: the emulator build creates its streams like the product and never looks at queues."""
import os
import sys

import numpy as np
import pytest

import corpus

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

MIB = 1 << 20
MAX_RUNS = 8   # ZH_MAX_RUNS


@pytest.fixture(scope="module")
def emu():
    import build_emu
    from zultra_amd._ffi import Lib
    return Lib(build_emu.build())


def rule(batch_bytes, nblocks, setting):
    """The comment of zultra_hip_runs_for, restated: what is wanted, then what the batch can feed. It is the formula zh_plan_runs had inline before."""
    want = min(setting, MAX_RUNS) if setting > 0 else (4 if batch_bytes >= 256 * MIB else 3)   # the setting; else three, four from 256 MiB on
    return max(1, min(want, nblocks // 4, batch_bytes // (4 * MIB)))                            # a run has at least four max-blocks and 4 MiB


SIZES = [r * 4 * MIB - d for r in (1, 2, 3, 4) for d in (1, 0)] + [100_000_000, 256 * MIB - 1, 256 * MIB, 1 << 30]


@pytest.mark.parametrize("setting", [0, 1, 3])
def test_runs_for_table(emu, setting):
    for batch_bytes in SIZES:
        for nblocks in (3, 4, 8, 1526):
            assert emu.runs_for(batch_bytes, nblocks, setting) == rule(batch_bytes, nblocks, setting), (batch_bytes, nblocks, setting)


def test_runs_for_spot_values(emu):
    """A few values by hand, so that the table does not only compare two copies of one formula."""
    assert emu.runs_for(100_000_000, 1526, 0) == 3
    assert emu.runs_for(100_000_000, 1526, 1) == 1 and emu.runs_for(100_000_000, 1526, 2) == 2
    assert emu.runs_for(100_000_000, 1526, 8) == 8 and emu.runs_for(100_000_000, 1526, 99) == 8
    assert emu.runs_for(1 << 30, 16384, 0) == 4 and emu.runs_for(256 * MIB - 1, 16384, 0) == 3
    assert emu.runs_for(12 * MIB - 1, 1526, 0) == 2 and emu.runs_for(12 * MIB, 1526, 0) == 3
    assert emu.runs_for(100_000_000, 8, 0) == 2 and emu.runs_for(100_000_000, 3, 0) == 1
    assert emu.runs_for(8 * 65536, 8, 0) == 1 and emu.runs_for(8 * 65536, 8, 3) == 1


def test_the_emulators_run_count_is_unchanged(emu, checker, monkeypatch):
    """Three max-blocks of 32 KiB are one run, as ever, and the stream is the checker's; a files batch under ZULTRA_HIP_STREAMS=3 is still three runs."""
    monkeypatch.delenv("ZULTRA_HIP_STREAMS", raising=False)
    bs, d = 32768, corpus.text_like(2 * 32768 + 300, 31)
    blocks = [(b * bs - (bs if b else 0), bs if b else 0, min(bs, len(d) - b * bs)) for b in range(3)]
    ctx = emu.context(bs, 3)
    try:
        ctx.compress_blocks(d, blocks)
        end_bit, _ = ctx.stitch_device(2, phase=0)
        st = ctx.stats()
        assert (st["runs"], st["runs_fitted"], st["stream_collisions"]) == (1, 1, 0)
        assert ctx.stream_read((end_bit + 7) // 8).tobytes() == checker.memory_compress(d, 0, bs)
    finally:
        ctx.close()
    monkeypatch.setenv("ZULTRA_HIP_STREAMS", "3")
    sizes = [4096, 1500, 1, 3000, 777, 4000, 2048, 12, 3500, 4096, 100, 2500]
    ctx = emu.files_context(4096, len(sizes))
    try:
        ctx.compress_files(np.concatenate([corpus.json_like(n, 60 + i) for i, n in enumerate(sizes)]), np.cumsum([0] + sizes[:-1]), sizes)
        assert ctx.stats()["runs"] == 3
    finally:
        ctx.close()
