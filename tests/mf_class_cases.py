"""Shared cases of tests/test_mf_classes_emu.py and tests/test_mf_classes_gpu.py: the bigram classes that zh_mf_group does not refine in LDS
(zultra_amd/csrc/zh_mf_group_lds.h). A class of `cap` entries or more — cap: the chunk size, ZULTRA_HIP_MF_CAP or what the layout leaves — is NOTED
behind the segment's run table and refined by zh_mf_group_big; a class that is neither refined nor noted leaves its part of the 6-gram order unwritten,
and zh_mf_frontier then walks garbage. The note table was 29 entries whatever the chunk size; it is sized by the chunk size now (zh_mfl_max_notes).
The data is corpus.phrase_edits: `period` deep classes, all of one size, so that the number of notes a window needs is known before it is run. Every
case first asserts that number in numpy (noted_classes, expect_noted) — a case must not quietly stop exercising the table — and then compares every
stage with the checker (parity_util.check_window) or whole streams."""
import os
import re
import zlib

import numpy as np

import corpus
from parity_util import check_window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def constants():
    """ZH_SEG_WINDOW, ZH_HISTORY, ZH_MAX_MATCH, ZH_MIN_BLOCK as the product's zh_common.h defines them."""
    txt = open(os.path.join(ROOT, "zultra_amd", "csrc", "zh_common.h")).read()
    out = {}
    for name in ("ZH_SEG_WINDOW", "ZH_HISTORY", "ZH_MAX_MATCH", "ZH_MIN_BLOCK"):
        out[name] = int(re.search(r"^#define\s+%s\s+(\d+)u?\b" % name, txt, flags=re.M).group(1))
    return out


def noted_classes(win, prev, n, cap, tail=0):
    """Sizes of the bigram classes of a segment window (prev bytes of history, n of the block, `tail` of look-ahead) over the positions that start a
    trigram — the min(prev + n, W - 2) entries of zh_mf_group's bigram order. `cap` is not used to count: the caller compares. The data must have no
    byte runs (their interior positions leave the order)."""
    W = prev + n + tail
    win = np.asarray(win[:W], dtype=np.uint8)
    assert len(win) == W
    assert not ((win[1:-2] == win[:-3]) & (win[2:-1] == win[:-3]) & (win[3:] == win[:-3])).any(), "byte runs: the count below would not be the order's"
    m3 = min(prev + n, W - 2)
    keys = win[:m3].astype(np.uint32) | (win[1:m3 + 1].astype(np.uint32) << 8)
    sizes = np.bincount(keys, minlength=65536)
    return sizes[sizes > 0]


def expect_noted(win, prev, n, cap, expect, at_least=False, tail=0, band=True):
    """The case's precondition: every class is at most 0.8 x cap or at least 1.2 x cap (so that the number at or above cap does not hang on an entry or
    two), and that number is `expect` (or at least that). -> the number."""
    sizes = noted_classes(win, prev, n, cap, tail)
    if band:
        mid = sizes[(sizes > 0.8 * cap) & (sizes < 1.2 * cap)]
        assert mid.size == 0, "classes of %s entries: too close to the chunk size %d" % (mid.tolist(), cap)
    noted = int((sizes >= cap).sum())
    assert (noted >= expect) if at_least else (noted == expect), "%d classes of %d entries or more, the case needs %s%d" % (noted, cap, ">= " if at_least else "", expect)
    return noted


def set_cap(monkeypatch, lib, cap):
    """ZULTRA_HIP_MF_CAP is read when a context is created: cached contexts are dropped and not used. cap None: the library's default."""
    if cap is None:
        monkeypatch.delenv("ZULTRA_HIP_MF_CAP", raising=False)
    else:
        monkeypatch.setenv("ZULTRA_HIP_MF_CAP", str(cap))
    monkeypatch.setenv("ZULTRA_HIP_CACHE", "0")
    lib.L.zultra_release_cached_contexts()


def context_cap(lib, max_block, window, noted=0):
    """The chunk size a context of this library takes for a window of `window` bytes (zultra_hip_mf_chunk); its note table holds `noted` classes."""
    ctx = lib.context(max_block, 1)
    try:
        cap, room = ctx.mf_chunk(window)
    finally:
        ctx.close()
    assert room >= noted, "the note table holds %d classes, the window has %d to note" % (room, noted)
    return cap


def _mixed(size):
    half = size // 2
    return np.concatenate([corpus.phrase_edits(half, 7, period=40), corpus.text_like(size - half, 3)])


# name -> (data, prev, n, ZULTRA_HIP_MF_CAP, classes to note, "at least")
TABLE = {
    "notes_28": (lambda: corpus.phrase_edits(8000, 1, period=28), 0, 8000, 64, 28, False),
    "notes_29": (lambda: corpus.phrase_edits(8000, 1, period=29), 0, 8000, 64, 29, False),          # the table of before: exactly full
    "notes_30": (lambda: corpus.phrase_edits(8000, 1, period=30), 0, 8000, 64, 30, False),          # ... the first one past it
    "notes_64": (lambda: corpus.phrase_edits(8000, 1, period=64), 0, 8000, 64, 64, False),
    "notes_64_hist": (lambda: corpus.phrase_edits(8000, 2, period=64), 3000, 5000, 64, 64, False),  # rows only from `prev` on
    "notes_200_cap16": (lambda: corpus.phrase_edits(8000, 1, period=200), 0, 8000, 16, 200, False),  # 40 per class
    # noted and refined classes interleaved in the order: where a later chunk's entries go depends on the entries of every class noted before it
    "notes_mixed": (lambda: _mixed(12000), 0, 12000, 64, 40, True),
}
TABLE_IDS = list(TABLE)


def _mixed_precondition(win, prev, n, cap, expect):
    """notes_mixed: text has bigram classes of every size, some of them near any chunk size, so the band holds for the phrase's classes only — each of
    them at least 1.2 x cap: `expect` notes for certain, the text adds some — and the case is about the order: walking the bigram order (byte 0, then
    byte 1), noted and refined classes take turns many times. -> the number of classes at or above cap."""
    m3 = min(prev + n, len(win) - 2)
    keys = win[:m3].astype(np.uint32) | (win[1:m3 + 1].astype(np.uint32) << 8)
    sizes = np.bincount(keys, minlength=65536)
    half = np.bincount(keys[:m3 // 2 - 1], minlength=65536)
    phrase = np.argsort(half)[-expect:]                     # the phrase's bigrams: the `expect` most frequent of the first half
    assert (half[phrase] >= 1.2 * cap).all() and (sizes[phrase] >= 1.2 * cap).all()
    present = np.flatnonzero(sizes)
    order = present[np.lexsort((present >> 8, present & 0xff))]
    is_noted = sizes[order] >= cap
    turns = int((is_noted[1:] != is_noted[:-1]).sum())
    assert turns >= expect, "noted and refined classes take turns %d times in the order" % turns
    return int(is_noted.sum())


def table_case(lib, checker, monkeypatch, name):
    gen, prev, n, cap, expect, at_least = TABLE[name]
    win = gen()
    noted = expect_noted(win, prev, n, cap, expect, at_least, band=name != "notes_mixed")
    if name == "notes_mixed":
        assert _mixed_precondition(win, prev, n, cap, expect) == noted
    set_cap(monkeypatch, lib, cap)
    assert context_cap(lib, 32768, prev + n, noted) == cap
    check_window(lib, checker, win, prev, n, tag=name)


def _follows_phrase(d, period, lo, hi):
    """No edit in d[lo:hi]: the bytes are the tiled phrase's (every byte equals the one a period before)."""
    return bool((d[lo:hi] == d[lo - period:hi - period]).all())


def window_end_tail0(lib, checker, monkeypatch):
    """The last five positions of a window are in no 6-gram order: a noted class's entry count is its size less those of them that are its own
    (zh_mf_group_body_lds, `nv`), and the chunks behind it are written from there on. A window that ends inside the phrase — its last positions belong
    to noted classes —, the max-block its own segment: no look-ahead, the five positions are block positions."""
    period, cap, n = 64, 64, 8000
    win = corpus.phrase_edits(n, 5, period=period)
    assert _follows_phrase(win, period, n - 12, n)
    noted = expect_noted(win, 0, n, cap, period)
    set_cap(monkeypatch, lib, cap)
    assert context_cap(lib, 32768, n, noted) == cap
    check_window(lib, checker, win, 0, n, tag="window_end_tail0")


def window_end_lookahead(lib, checker, monkeypatch):
    """The same with a look-ahead tail: a max-block of more than ZH_SEG_WINDOW bytes is cut into segments of ZH_SEG_WINDOW - ZH_HISTORY - ZH_MAX_MATCH
    positions, each but the last with ZH_MAX_MATCH bytes of the next behind it. The last five positions of such a window are look-ahead, none of them is
    in the bigram order, and a noted class has as many entries as positions. Both segments' windows end inside the phrase."""
    k = constants()
    period, cap = 64, 64
    seg_n = k["ZH_SEG_WINDOW"] - k["ZH_HISTORY"] - k["ZH_MAX_MATCH"]
    n = k["ZH_SEG_WINDOW"] + 1000                       # the smallest max-blocks that are cut: two segments
    win = corpus.phrase_edits(n, 2, period=period)
    w0 = seg_n + k["ZH_MAX_MATCH"]                      # the first segment's window: no history, seg_n positions, the look-ahead
    assert _follows_phrase(win, period, w0 - 12, w0) and _follows_phrase(win, period, n - 12, n)
    noted = expect_noted(win, 0, seg_n, cap, period, tail=k["ZH_MAX_MATCH"])
    hist = k["ZH_HISTORY"]
    noted = max(noted, expect_noted(win[seg_n - hist:], hist, n - seg_n, cap, period))
    set_cap(monkeypatch, lib, cap)
    assert context_cap(lib, 1 << 20, k["ZH_SEG_WINDOW"], noted) == cap
    check_window(lib, checker, win, 0, n, max_block=1 << 20, tag="window_end_lookahead")


def default_cap_sibling(lib, checker, monkeypatch):
    """The emulator build's compiled chunk size (512) on a window of 24 KB: 36 classes of about 650 entries, more than the 29 notes of before. (The
    recorded input's shape at a size that takes the emulator tens of seconds; recorded_shape is the input itself.)"""
    set_cap(monkeypatch, lib, None)
    prev, n = 8000, 16384
    cap = context_cap(lib, 32768, prev + n)
    win = corpus.phrase_edits(prev + n, 3, period=36)
    noted = expect_noted(win, prev, n, cap, 36)
    assert context_cap(lib, 32768, prev + n, noted) == cap
    check_window(lib, checker, win, prev, n, tag="default_cap_sibling")


def recorded_shape(lib, checker, monkeypatch):
    """profiles/compress_host_refactor.txt's input: one 64-byte phrase with a changed byte every 40 to 90 positions, 70000 bytes as a gzip stream of
    32 KiB max-blocks. The second max-block's window is 64 KiB: 64 classes of about 1000 entries against the emulator's chunks of 512."""
    set_cap(monkeypatch, lib, None)
    d = corpus.phrase_edits(70000, 1)
    got = lib.memory_compress(d, 2, 32768)
    assert got is not None and zlib.decompress(got, 31) == d.tobytes()
    assert got == checker.memory_compress(d, 2, 32768)


def full_window_default_cap(lib, checker, monkeypatch):
    """The product's own edge: the largest segment window (ZH_SEG_WINDOW: the largest max-block that is one segment behind a full history) leaves the
    smallest chunks, and 24 classes that reach them is what the 29 notes of the default table are for. Period 24, an edit every 1500 to 2500 bytes: every
    class keeps more entries than a chunk holds. If the window grows or the layout's chunks shrink, the count asserted here is the first thing to move."""
    k = constants()
    set_cap(monkeypatch, lib, None)
    prev, n = k["ZH_HISTORY"], k["ZH_SEG_WINDOW"] - k["ZH_HISTORY"]
    ctx = lib.context(n, 1)
    try:
        cap, room = ctx.mf_chunk(prev + n)
    finally:
        ctx.close()
    win = corpus.phrase_edits(prev + n, 4, period=24, gap=(1500, 2500))
    sizes = noted_classes(win, prev, n, cap)
    assert int((sizes >= cap).sum()) == 24 and int(np.sort(sizes)[-24:].min()) >= 1.02 * cap, (cap, np.sort(sizes)[-26:].tolist())
    assert room >= 24, (cap, room)
    check_window(lib, checker, win, prev, n, max_block=n, tag="full_window_default_cap")


def helpers(lib, checker, monkeypatch, cap, period, flags=2):
    """Workgroups of zh_mf_frontier without a segment of their own join the unfinished ones (`steal`): a batch of four max-blocks of the smallest size,
    every one's window with `period` classes of 1.3 to 2.7 chunks each, as a whole stream."""
    k = constants()
    bs = k["ZH_MIN_BLOCK"]
    d = corpus.phrase_edits(3 * bs + 9000, 8, period=period)
    set_cap(monkeypatch, lib, cap)
    most = 0
    for b in range(4):
        prev = min(b * bs, k["ZH_HISTORY"])
        n = min(bs, len(d) - b * bs)
        c = context_cap(lib, bs, prev + n)
        assert cap is None or c == cap
        most = max(most, expect_noted(d[b * bs - prev:], prev, n, c, period))
    context_cap(lib, bs, bs + k["ZH_HISTORY"], most)
    got = lib.memory_compress(d, flags, bs)
    assert got is not None and zlib.decompress(got, 31 if flags == 2 else 15 if flags == 1 else -15) == d.tobytes()
    assert got == checker.memory_compress(d, flags, bs)
