"""Shared cases of tests/test_lane_order_emu.py and tests/test_lane_order_gpu.py: the bundles zh_parse_lanes takes (zh_parse.h: up to T consecutive
tasks of ONE sub-block, listed by zh_list_huge in classes by their longest piece, handed out longest class first) must not change a byte. Every case is
run with ZULTRA_HIP_LANE_ORDER 0 and 1 and ZULTRA_HIP_LANE_TASKS 1, 2, 3 (odd on purpose) and 8 — a window of a few max-blocks otherwise always gets
T = 1 — and compares with the checker stage by stage (parity_util.check_window) or on whole streams. `small`: the emulator's sizes (it takes ten
seconds for 32 KiB of noise and fifty for 32 KiB of text); the windows keep their shape — the number of tasks per sub-block, which tasks are listed —
and lose bytes only."""
import numpy as np

import corpus
from parity_util import check_window

COMBOS = [(order, tasks) for order in ("0", "1") for tasks in ("1", "2", "3", "8")]
COMBO_IDS = ["order%s-T%s" % c for c in COMBOS]
TASK = 2048   # ZH_TASK: a sub-block of n bytes has ceil(n / 2048) tasks


def set_switches(monkeypatch, lib, combo, **more):
    """The two switches of this file plus the case's own, read when a context is created: cached contexts are dropped and not used."""
    order, tasks = combo
    monkeypatch.setenv("ZULTRA_HIP_LANE_ORDER", order)
    monkeypatch.setenv("ZULTRA_HIP_LANE_TASKS", tasks)
    monkeypatch.setenv("ZULTRA_HIP_CACHE", "0")
    for k, v in more.items():
        monkeypatch.setenv("ZULTRA_HIP_" + k, str(v))
    lib.L.zultra_release_cached_contexts()


def one_bin_stretch(n, k):
    """n bytes over 16 byte values that fall into one bin of the splitter's statistics (test_many_sub_blocks_in_one_max_block): stretch k and
    stretch k + 1 fall into different bins, so the splitter cuts between them and not inside."""
    r = corpus.noise(n, 500 + k)
    return ((((k >> 2) & 3) << 6) | ((r & 15) << 2) | (k & 3)).astype(np.uint8)


def bundle_sizes(lib, checker, monkeypatch, combo, small):
    """A sub-block of one task (a bundle of one whatever T is); a sub-block of T + 1 tasks (a full bundle and a last bundle of one); and one max-block
    cut into several sub-blocks of five tasks each (T = 2: bundles of 2, 2, 1; T = 3: 3, 2; T = 8: every sub-block one short bundle)."""
    set_switches(monkeypatch, lib, combo)
    T = int(combo[1])
    st = {}
    check_window(lib, checker, corpus.text_like(2500, 3), 1000, 1500, tag="one_task", stats_out=st)
    assert (st["subblocks"], st["tasks"]) == (1, 1), st
    st = {}
    n = (T + 1) * TASK - 300
    check_window(lib, checker, corpus.noise(n, 5), 0, n, tag="T_plus_one", stats_out=st)   # (noise: nothing for the splitter to cut at)
    assert (st["subblocks"], st["tasks"]) == (1, T + 1), st
    st = {}
    many = np.concatenate([one_bin_stretch(5 * TASK - 100, k) for k in range(3 if small else 12)])
    check_window(lib, checker, many, 0, len(many), max_block=1 << 20, tag="five_task_subblocks", stats_out=st)
    assert st["subblocks"] >= (3 if small else 10) and st["tasks"] >= 5 * (3 if small else 12), st


def mixed_classes(lib, checker, monkeypatch, combo, small):
    """Tasks with barrier-free pieces of many hundred positions (near-copies with an edit every 900 bytes, byte runs, table rows) beside tasks of text
    and noise, whose pieces are the minimum of 128: bundles of several length classes in one run. ZULTRA_HIP_COOP_SMALL=1536 keeps every piece of up
    to ZH_COOP_MIN positions on the quads, as a large batch does."""
    set_switches(monkeypatch, lib, combo, COOP_SMALL=1536)
    k = 1 if small else 4
    d = np.concatenate([corpus.text_like(1500 * k, 3), corpus.duplicated(5000 * k, 3, 900), corpus.noise(2100 * k, 2), corpus.indented(2500 * k, 11),
                        corpus.table_like(3000 * k, 9), corpus.text_like(1200 * k, 5)])
    check_window(lib, checker, d, 1000, len(d) - 1000, max_block=65536, tag="mixed_classes")


def single_class(lib, checker, monkeypatch, combo, small):
    """Noise has a barrier at every position: every task's pieces are 128 positions, every bundle falls into the last class, the other lists stay empty."""
    set_switches(monkeypatch, lib, combo, COOP_SMALL=1536)
    n = 7000 if small else 40000
    check_window(lib, checker, corpus.noise(n, 1), 0, n, max_block=65536, tag="single_class")


def listed_tasks(lib, checker, monkeypatch, combo, small, wide):
    """Table-like text is mostly barrier-free runs: its tasks are cut into speculative segments (parsed in the segment workgroups or by zh_parse_chain:
    ZULTRA_HIP_SEG_WIDE both ways, as test_chain_tasks_are_cut_into_speculative_segments) or listed as whole chains. With a little text at either end
    the run has bundles in which every task is listed — no entry, no ticket — and bundles in which one or two are not."""
    set_switches(monkeypatch, lib, combo, SEG_WIDE=wide, SEG_WHOLE=0)
    st = {}
    if small:
        # (the emulator build cuts every 512 positions; noise over 16 byte values has matches everywhere and few barriers: cut tasks for a fifth of
        # the time table-like text of the size that has any would take it)
        d = one_bin_stretch(9 * TASK - 300, 5)
        d[:600] = corpus.text_like(600, 4)
        check_window(lib, checker, d, 0, len(d), tag="listed/" + wide, stats_out=st)
    else:
        d = np.concatenate([corpus.table_like(98304, 9), corpus.text_like(3000, 8)])
        check_window(lib, checker, d, 32768, 65536 + 3000, 1 << 20, tag="listed/" + wide, stats_out=st)
    assert st["cut_tasks"] + st["huge_tasks"] >= 1 and st["tasks"] > st["cut_tasks"] + st["huge_tasks"], st


def settled_subblocks(lib, checker, monkeypatch, combo, small):
    """The windows of test_settled_subblocks_keep_their_parse: a sub-block that settles after pass 0, 1 or 2 is skipped from then on — in ordered bundles
    too the skipped tasks keep their parse entries and their histogram slots (the stages equal the checker's after the last pass)."""
    set_switches(monkeypatch, lib, combo)
    for name, d, prev, n, skipped in (("zeros", corpus.constant(3000), 500, 2500, 3), ("noise", corpus.noise(3000, 1), 0, 3000, 2),
                                      ("selftest", corpus.selftest_data(6000, 77, 15, 0.5), 1000, 5000, 1)):
        st = {}
        check_window(lib, checker, d, prev, n, tag="settled/" + name, stats_out=st)
        assert st["subblocks"] == 1 and st["settled_passes"] == skipped, (name, st)
    if not small:
        st = {}
        check_window(lib, checker, corpus.noise(40000, 1), 0, 40000, max_block=65536, tag="settled/noise40k", stats_out=st)
        assert st["settled_passes"] >= 1, st


def bundles_off(lib, checker, monkeypatch, combo, small):
    """ZULTRA_HIP_LANE_BUNDLES=0: no lists are kept and zh_parse_lanes takes T consecutive tasks of the task list per ticket, across sub-blocks, as it did before
    bundles (files mode still does): a max-block of several sub-blocks, chain tasks among the others."""
    set_switches(monkeypatch, lib, combo, LANE_BUNDLES=0)
    many = np.concatenate([one_bin_stretch(5 * TASK - 100, k) for k in range(3 if small else 12)])
    many[-1900:] = corpus.constant(1900, 66)
    st = {}
    check_window(lib, checker, many, 0, len(many), max_block=1 << 20, tag="bundles_off", stats_out=st)
    assert st["subblocks"] >= 3, st


def overflow_form(lib, checker, monkeypatch, combo, small):
    """ZULTRA_HIP_GRID_CAP=2: all tasks but two are visited by the strided <true> form of zh_list_huge, which has to fill the same lists."""
    set_switches(monkeypatch, lib, combo, GRID_CAP=2)
    many = np.concatenate([one_bin_stretch(9000, k) for k in range(3 if small else 8)])
    many[:500] = corpus.text_like(500, 2)
    st = {}
    check_window(lib, checker, many, 0, len(many), max_block=1 << 20, tag="overflow_form", stats_out=st)
    assert st["subblocks"] >= 3 and st["tasks"] > 4, st


def _stream_data(n, seed, small):
    """n bytes: text (a little for the emulator), noise, byte runs, near-copies — a chain task or two among ordinary ones."""
    if not small:
        d = corpus.text_like_fast(n, seed)
        d[20000:29000] = corpus.noise(9000, seed)
        d[50000:58000] = corpus.indented(8000, seed)
        d[n - 30000:n - 18000] = corpus.duplicated(12000, seed, 900)
        return d
    d = corpus.noise(n, seed)
    d[:1500] = corpus.text_like(1500, seed)
    d[9000:17000] = corpus.constant(8000, 32 + seed)
    d[32768 - 700:32768 + 800] = corpus.text_like(1500, seed + 1)
    if n >= 37000:
        d[34000:37000] = corpus.indented(3000, seed)
    return d


def staggered_runs(lib, checker, monkeypatch, combo, small):
    """Two and three staggered runs (ZULTRA_HIP_STREAMS) over a handful of max-blocks of 32 and 64 KiB, raw, zlib and gzip framing: each run lists its own
    bundles in its own lists and takes its own tickets. (The emulator: three runs of one 32 KiB max-block each and two runs over two, the framing
    going round with the combination.)"""
    k = COMBOS.index(combo)
    if small:
        todo = [("3", 32768, 2 * 32768 + 300, k % 3), ("2", 32768, 32768 + 5000, (k + 1) % 3)]
    else:
        todo = [(runs, bs, 5 * bs + 777, flags) for runs in ("2", "3") for bs in (32768, 65536) for flags in (0, 1, 2)]
    for runs, bs, n, flags in todo:
        set_switches(monkeypatch, lib, combo, STREAMS=runs)
        d = _stream_data(n, 30 + flags, small)
        assert lib.memory_compress(d, flags, bs) == checker.memory_compress(d, flags, bs), (runs, bs, flags)


def files_mode(lib, checker, monkeypatch, combo, small):
    """Files mode keeps its hand-out (consecutive tasks of the task list, no lists): a dozen 4 KiB inputs, then inputs of unequal sizes — also
    in three runs — are the checker's streams whatever the switches say."""
    for runs, sizes in ((None, [4096] * 12), ("3", [4096, 1500, 1, 3000, 777, 4000, 2048, 12, 3500, 4096, 100, 2500])):
        set_switches(monkeypatch, lib, combo, **({"STREAMS": runs} if runs else {}))
        makers = (corpus.json_like, corpus.noise) if small else (corpus.json_like, corpus.text_like, corpus.indented)
        files = [makers[i % len(makers)](n, 60 + i) for i, n in enumerate(sizes)]
        ctx = lib.files_context(4096, len(files))
        try:
            fo = ctx.compress_files(np.concatenate(files), np.cumsum([0] + sizes[:-1]), sizes)
            stream = ctx.stream_read(int(fo[-1]))
            for i, f in enumerate(files):
                assert stream[int(fo[i]):int(fo[i + 1])].tobytes() == checker.memory_compress(f, 0, 32768), (runs, i, sizes[i])
        finally:
            ctx.close()
