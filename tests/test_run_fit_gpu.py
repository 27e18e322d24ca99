"""GPU: a context creates the streams a batch keeps busy first and reports what hardware queues they got (zh_need_run_streams, zh_look_at_streams; the run count
itself: zultra_hip_runs_for, which the look does not enter).

Every case is a fresh child process that initialises HIP through torch before the library is loaded — the library's own hint for the number of hardware queues then
comes too late, and GPU_MAX_HW_QUEUES in the child's environment decides how many the process has. The batch is the smallest that is cut into three runs (13 MiB at
64 KiB max-blocks: a run needs 4 MiB and four max-blocks); the bytes are the checker's in every case, computed once for all of them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import corpus
from frame_member_cases import make_checker

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BS = 65536

WORKER = r'''
import json, sys
import numpy as np
import torch
torch.zeros(1).cuda()                      # HIP is up before the library is loaded: its GPU_MAX_HW_QUEUES hint comes too late
sys.path.insert(0, %(root)r); sys.path.insert(0, %(here)r)
import corpus, zultra_amd
L = zultra_amd.lib()
bs, contexts, size, want = %(bs)d, int(sys.argv[1]), int(sys.argv[2]), open(sys.argv[3], "rb").read()
d = np.concatenate([corpus.text_like_fast(9 << 20, 3), corpus.indented(4 << 20, 5)])[:size]
nb = (len(d) + bs - 1) // bs
blocks = [(b * bs - (32768 if b else 0), 32768 if b else 0, min(bs, len(d) - b * bs)) for b in range(nb)]
ctxs = [L.context(bs, nb) for _ in range(contexts)]   # (the second is created while the first lives)
out = []
for ctx in ctxs:
    ctx.compress_blocks(d, blocks)
    end_bit, _ = ctx.stitch_device(nb - 1, phase=0)
    st = ctx.stats()
    st["bytes_equal"] = ctx.stream_read((end_bit + 7) // 8).tobytes() == want
    out.append(st)
for ctx in ctxs:
    ctx.close()
print("STATS " + json.dumps(out))
''' % {"root": ROOT, "here": HERE, "bs": BS}


def _data(size):
    return np.concatenate([corpus.text_like_fast(9 << 20, 3), corpus.indented(4 << 20, 5)])[:size]


@pytest.fixture(scope="module")
def case_files(tmp_path_factory):
    """The worker's script and the checker's raw deflate stream of both batches, written once."""
    d = tmp_path_factory.mktemp("run_fit")
    (d / "worker.py").write_text(WORKER)
    checker = make_checker()
    for name, size in (("large", 13 << 20), ("small", 8 * BS)):
        (d / (name + ".deflate")).write_bytes(checker.memory_compress(_data(size), 0, BS))
    return d


def _child(case_files, queues, contexts=1, batch="large", streams=None):
    env = {k: v for k, v in os.environ.items() if k not in ("ZULTRA_HIP_STREAMS", "ZULTRA_HIP_SPREAD_STREAMS", "ZULTRA_HIP_SPREAD_SCOPE")}
    env["GPU_MAX_HW_QUEUES"] = str(queues)
    if streams:
        env["ZULTRA_HIP_STREAMS"] = str(streams)
    size = (13 << 20) if batch == "large" else 8 * BS
    r = subprocess.run([sys.executable, str(case_files / "worker.py"), str(contexts), str(size), str(case_files / (batch + ".deflate"))],
                       env=env, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("STATS ")]
    assert r.returncode == 0 and lines, r.stdout[-1500:] + r.stderr[-1500:]
    stats = json.loads(lines[-1][6:])
    print(queues, streams, [(s["runs"], s["runs_fitted"], s["stream_collisions"]) for s in stats])
    assert len(stats) == contexts and all(s["bytes_equal"] for s in stats), stats
    return stats


def _consistent(st):
    """What the two figures mean, whatever the streams got: a look of R = 3 -> 2 -> 1 that stops where nothing shared."""
    assert 1 <= st["runs_fitted"] <= 3
    assert (st["stream_collisions"] == 0) == (st["runs_fitted"] == 3)   # (the collisions are those of the first look, at three runs)


def test_four_queues_the_first_contexts_runs_have_queues_of_their_own(case_files):
    """The runtime's default of four queues, the benchmark's setting: the context creates the streams of its three runs before any other, a process has one normal
    and one high-priority queue for each, and the look finds them apart. A second context created behind the first keeps the run count whatever its look says:
    the figures report, they do not decide (one run alone is slower than three that wait for each other, profiles/run_fit_time.txt)."""
    first, second = _child(case_files, 4, contexts=2)
    _consistent(first), _consistent(second)
    assert (first["runs"], first["runs_fitted"], first["stream_collisions"]) == (3, 3, 0)
    assert second["runs"] == 3


def test_two_queues_keep_the_run_count(case_files):
    """Three runs' streams cannot lie apart on two queues; the batch is three runs all the same, as it was before the look existed."""
    (st,) = _child(case_files, 2)
    _consistent(st)
    assert st["runs"] == 3 and st["runs_fitted"] < 3 and st["stream_collisions"] > 0


def test_eight_queues_nothing_shares(case_files):
    (st,) = _child(case_files, 8)
    assert (st["runs"], st["runs_fitted"], st["stream_collisions"]) == (3, 3, 0)


def test_an_explicit_setting_wins_and_does_not_look(case_files):
    (st,) = _child(case_files, 4, streams=3)
    assert (st["runs"], st["runs_fitted"], st["stream_collisions"]) == (3, 3, 0)
    (st,) = _child(case_files, 4, streams=2)
    assert (st["runs"], st["runs_fitted"], st["stream_collisions"]) == (2, 2, 0)


def test_a_context_of_one_run_does_not_look(case_files):
    """Eight max-blocks can only be one run: nothing is probed, the figure is still reported."""
    (st,) = _child(case_files, 4, batch="small")
    assert (st["runs"], st["runs_fitted"], st["stream_collisions"]) == (1, 1, 0)
