"""Shared by tests/test_inflate_dict_emu.py (CPU emulator build) and tests/test_inflate_dict_gpu.py (product library on the MI355X): the streams, the
batch runner and the checks of zultra_hip_inflate_streams_dict (zh_inflate_streams_dict, zultra_amd/csrc/zh_inflate_out.h) and
zultra_memory_decompress_dict. One preset dictionary serves every item of a call; its last min(size, 32768) bytes are the history in front of every
item's output. The yardstick is Python's zlib with `zdict`. The writers and the runner's pattern are those of tests/inflate_cases.py."""
import os
import pickle
import random
import subprocess
import sys
import zlib

import numpy as np

import corpus
import inflate_cases as I
import verify_cases as V
from inflate_cases import CANARY, CANARY_BYTE, DISTANCE, DST_FULL, OK, STREAM_END, BitWriter, ListWriter

WINDOW = 32768
DICT_SIZES = [1, 2, 3, 63, 64, 65, 257, 258, 259, 32767, 32768, 32769, 70000]


# ---- running a batch ----------------------------------------------------------------------------------------------------------------------
def run_dict(lib, streams, caps, dictionary, on_device=True, src_sizes=None, dict_lead=0):
    """inflate_cases.run_streams with a dictionary (bytes; None: a NULL pointer and size 0). on_device: source, destination and dictionary in device
    memory, the dictionary dict_lead bytes behind an allocation's start (0xFF around it); else host arrays, staged by the call.
    -> (rc, [(reason, blocks, out_size, src_used, output bytes)])."""
    src = np.frombuffer(b"".join(bytes(s) for s in streams) + b"\0", dtype=np.uint8).copy()[:-1]
    items, soff, doff = [], 0, CANARY
    for k, s in enumerate(streams):
        items.append((soff, len(s) if src_sizes is None else src_sizes[k], doff, caps[k]))
        soff += len(s)
        doff += caps[k] + CANARY
    dst = np.full(doff, CANARY_BYTE, dtype=np.uint8)
    n = 0 if dictionary is None else len(dictionary)
    if on_device:
        held = np.frombuffer(b"\xff" * dict_lead + bytes(dictionary or b"") + b"\xff" * 8, dtype=np.uint8).copy()
        s, d, h = V.DeviceCopy(lib, src), V.DeviceCopy(lib, dst), V.DeviceCopy(lib, held)
        try:
            assert (h.ptr + dict_lead) & 3 == dict_lead & 3
            rc, res, _ = lib.inflate_streams_dict(s.ptr, len(src), d.ptr, len(dst), None if dictionary is None else h.ptr + dict_lead, n, items)
            back = I.device_read(lib, d, len(dst)).copy()
        finally:
            s.free()
            d.free()
            h.free()
    else:
        arr = None if dictionary is None else np.frombuffer(bytes(dictionary) + b"\0", dtype=np.uint8).copy()[:-1]
        rc, res, _ = lib.inflate_streams_dict(src, len(src), dst, len(dst), arr, n, items)
        back = dst
    assert rc >= 0, "zultra_hip_inflate_streams_dict failed"
    assert rc == int((res["reason"] != 0).sum())
    I.check_canaries(back, items, res)
    return rc, [(int(r["reason"]), int(r["blocks"]), int(r["out_size"]), int(r["src_used"]), back[it[2]: it[2] + int(r["out_size"])].tobytes()) for it, r in zip(items, res)]


def host_verdict(stream, dictionary):
    """Host zlib with zdict on a raw deflate stream -> (inflates without error and reaches the end, output, bytes of the stream used)."""
    d = zlib.decompressobj(-15, zdict=bytes(dictionary)) if dictionary else zlib.decompressobj(-15)
    try:
        out = d.decompress(bytes(stream))
    except zlib.error:
        return False, b"", 0
    return bool(d.eof), out, len(stream) - len(d.unused_data)


def check_good(lib, named, dictionary, on_device=True, dict_lead=0, copies=1):
    """Every (name, stream, want) decodes to `want` against the dictionary, uses the whole stream, and host zlib with zdict agrees first."""
    for name, s, want in named:
        assert host_verdict(s, dictionary) == (True, want, len(s)), name
    named = named * copies
    rc, res = run_dict(lib, [s for _, s, _ in named], [len(w) for _, _, w in named], dictionary, on_device, dict_lead=dict_lead)
    for (name, s, want), (reason, blocks, out_size, src_used, out) in zip(named, res):
        assert reason == OK, (name, reason, out_size, src_used)
        assert out_size == len(want) and out == want, (name, out_size, len(want))
        assert src_used == len(s) and blocks >= 1, (name, src_used, len(s), blocks)
    assert rc == 0
    return res


# ---- 1. zlib's own streams, compressed with zdict ---------------------------------------------------------------------------------------------
VARIANTS = [("l1", 1, zlib.Z_DEFAULT_STRATEGY), ("l6", 6, zlib.Z_DEFAULT_STRATEGY), ("l9", 9, zlib.Z_DEFAULT_STRATEGY), ("fixed", 6, zlib.Z_FIXED), ("rle", 6, zlib.Z_RLE)]
INPUTS = {"text": (corpus.text_like, 3000), "json": (corpus.json_like, 2500)}


def dictionary_of(gen, size, seed=40):
    return gen(size, seed).tobytes()


def zlib_streams(size):
    """-> (dictionary, [(name, stream, input)]). The dictionary comes from the input's generator (another seed: the same words and keys). The input
    starts by quoting the dictionary's end — its last byte four times (what Z_RLE, which looks one byte back only, takes from the dictionary, and
    all that can be taken from a dictionary of one or two bytes, which zlib does not hash), then its last up to 300 bytes — so that matches reach
    into dictionaries of every size."""
    out = []
    dictionary = dictionary_of(corpus.text_like, size)
    for kind, (gen, n) in sorted(INPUTS.items()):
        d = dictionary[-1:] * 4 + dictionary[-300:] + gen(n, 3).tobytes()
        for name, level, strategy in VARIANTS:
            c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy, zdict=dictionary)
            out.append(("%s/%s/%d" % (kind, name, size), c.compress(d) + c.flush(), d))
    return dictionary, out


def check_zlib_streams(lib, size, leads):
    """Host pointers, then device pointers with the dictionary `lead` bytes into a dword for every lead of `leads`; and without the dictionary at
    least one stream of the size must fail (host zlib: invalid distance too far back; the plain call: reason 4)."""
    dictionary, named = zlib_streams(size)
    check_good(lib, named, dictionary, on_device=False)
    for lead in leads:
        check_good(lib, named, dictionary, on_device=True, dict_lead=lead)
    rc, res = I.run_streams(lib, [s for _, s, _ in named], [len(w) for _, _, w in named])
    need = 0
    for (name, s, want), r in zip(named, res):
        ok = I.host_verdict(s)[0]
        assert (r[0] == OK) == ok and r[0] in (OK, DISTANCE), (name, r[:4], ok)
        need += not ok
    assert need >= 1, "no stream of dictionary size %d needs its dictionary" % size
    if size > WINDOW:   # the last 32768 bytes alone are the same history
        check_good(lib, named, dictionary[-WINDOW:], on_device=True)
    return need


# ---- 2. hand-written token streams ---------------------------------------------------------------------------------------------------------------
def replay(blocks, history=b""):
    """What the token list says over history + output, byte by byte in plain Python. blocks = [("stored", bytes) | (kind, [bytes | (len, dist)])]."""
    h = bytes(history)[-WINDOW:]
    out = bytearray(h)
    for kind, body in blocks:
        for t in ([body] if kind == "stored" else body):
            if isinstance(t, bytes):
                out += t
                continue
            length, dist = t
            assert 1 <= dist <= len(out), (length, dist, len(out))
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out[len(h):])


def write_fixed(blocks):
    """Stored and fixed-Huffman blocks from a token list, with inflate_cases.BitWriter."""
    w = BitWriter()
    for i, (kind, body) in enumerate(blocks):
        final = i == len(blocks) - 1
        if kind == "stored":
            w.stored(body, final)
            continue
        w.begin_fixed(final)
        for t in body:
            if isinstance(t, bytes):
                w.lits(t)
            else:
                w.match(*t)
        w.eob()
    return w.bytes()


def history(n, seed):
    return I._pattern(n, seed)


def hand_cases():
    """-> [(name, history, blocks)]: the smallest shapes at which the source select, the wrap and `synced` can go wrong. Every case ends with two
    literals and a match into what the case itself has written."""
    tail = [b"ok", (4, 2)]
    full, h32767 = history(WINDOW, 1), history(WINDOW - 1, 2)
    out = []
    for n in (1, 100):
        out.append(("p0_d1_l258_h%d" % n, history(n, 3), [("fixed", [(258, 1)] + tail)]))
    for n in (7, 300):
        for length in (3, 258):
            out.append(("p0_dhist_l%d_h%d" % (length, n), history(n, 4), [("fixed", [(length, n)] + tail)]))
    for length in (3, 258):
        out.append(("p0_d32768_l%d" % length, full, [("fixed", [(length, WINDOW)] + tail)]))
    out.append(("p1_d32768_h32767", h32767, [("fixed", [b"x", (258, WINDOW), (3, WINDOW)] + tail)]))
    for n in (3, 10):
        for length in (3, 5, 6, 258):   # p = 2, dist = 5: three bytes of history, two of the output, then round again
            out.append(("straddle_l%d_h%d" % (length, n), history(n, 5), [("fixed", [b"ab", (length, 5)] + tail)]))
    for n in (7, 40):   # three literals still held in the lanes: the source is history, those literals, and wraps
        out.append(("lits_then_d10_l20_h%d" % n, history(n, 6), [("fixed", [b"xyz", (20, 10)] + tail)]))
    out.append(("behind_stored", history(50, 7), [("stored", b"ten bytes."), ("fixed", [(8, 14), (30, 12), (258, 60)] + tail)]))
    out.append(("behind_stored_at_start", history(9, 7), [("stored", b""), ("fixed", [(9, 9)]), ("stored", b"abc"), ("fixed", [(7, 12 + 9)] + tail)]))
    lits65 = I._pattern(65, 9)
    out.append(("65_literals_then_straddle", history(5, 8), [("fixed", [lits65, (10, 65 + 3), (258, 65 + 10 + 5)] + tail)]))
    out.append(("64_literals_then_straddle", history(5, 8), [("fixed", [lits65[:64], (70, 64 + 1)] + tail)]))
    out.append(("history_then_its_output", history(20, 10), [("fixed", [(6, 10), (8, 6), (5, 14), (258, 19 + 20)] + tail)]))
    return out


def hand_streams():
    """-> [(name, history, stream, want)], host zlib with zdict checked against the replay."""
    out = []
    for name, h, blocks in hand_cases():
        s, want = write_fixed(blocks), replay(blocks, h)
        assert host_verdict(s, h) == (True, want, len(s)), name
        out.append((name, h, s, want))
    return out


def by_history(cases):
    """Cases grouped by their history: one call serves one dictionary."""
    groups = {}
    for c in cases:
        groups.setdefault(c[1], []).append(c)
    return sorted(groups.items(), key=lambda g: (len(g[0]), g[0]))


def check_hand(lib):
    n = 0
    for h, group in by_history(hand_streams()):
        named = [(name, s, want) for name, _, s, want in group]
        check_good(lib, named, h, on_device=True, dict_lead=n & 3)
        check_good(lib, named, h, on_device=False)
        n += len(named)
    return n


# ---- 3. rejects ------------------------------------------------------------------------------------------------------------------------------------
def check_too_far(lib):
    """dist = p + hist_len + 1: reason 4, and what was written is the literals in front of the match."""
    n = 0
    for hist_len, ps in ((0, (0, 5)), (1, (0, 5)), (100, (0, 5, 64)), (WINDOW - 1, (0,))):
        h = history(hist_len, 11)
        streams, lits = [], []
        for p in ps:
            lit = I._pattern(p, p)
            s = write_fixed([("fixed", [lit] * (p > 0) + [(5, p + hist_len + 1), b"tail of the stream"])])
            assert not host_verdict(s, h)[0], (hist_len, p)
            streams.append(s)
            lits.append(lit)
        for dev in (True, False):
            rc, res = run_dict(lib, streams, [600] * len(streams), h if hist_len else None, on_device=dev)
            assert rc == len(streams)
            for p, lit, r in zip(ps, lits, res):
                assert r[0] == DISTANCE and r[4] == lit, (hist_len, p, r)
        if hist_len:   # one byte more of history, the same streams: accepted
            rc, res = run_dict(lib, streams, [600] * len(streams), b"q" + h)
            assert rc == 0, (hist_len, res)
        n += len(streams)
    return n


def check_plain_call_rejects(lib):
    """Every accept case of hand_streams needs its dictionary: reason 4 through zultra_hip_inflate_streams."""
    cases = hand_streams()
    rc, res = I.run_streams(lib, [c[2] for c in cases], [len(c[3]) for c in cases])
    assert rc == len(cases)
    for (name, _, s, _), r in zip(cases, res):
        assert r[0] == DISTANCE and not I.host_verdict(s)[0], (name, r[:4])
    return len(cases)


def check_dst_cap(lib):
    """dst_cap exact and one byte short on the straddling matches (no tail behind them): one short is reason 13 with the bytes before the match."""
    h = history(10, 5)
    streams, wants = [], []
    for length in (3, 5, 6, 258):
        blocks = [("fixed", [b"ab", (length, 5)])]
        streams.append(write_fixed(blocks))
        wants.append(replay(blocks, h))
    for dev in (True, False):
        rc, res = run_dict(lib, streams, [len(w) for w in wants], h, on_device=dev)
        assert rc == 0 and [r[4] for r in res] == wants
        rc, res = run_dict(lib, streams, [len(w) - 1 for w in wants], h, on_device=dev)   # (run_dict looks at the canaries)
        assert rc == len(streams)
        for r in res:
            assert r[0] == DST_FULL and r[2] == 2 and r[4] == b"ab", r


# ---- 4. equivalence with the plain call ----------------------------------------------------------------------------------------------------------
def check_equivalence(lib):
    """Streams that never reach in front of their output: with dict_size == 0 (NULL and non-NULL pointer) and with a dictionary present the results
    and the bytes are those of zultra_hip_inflate_streams."""
    named = [c for name in sorted(I.FOREIGN) for c in I.foreign_streams(I.FOREIGN[name])] + I.hand_matches()
    streams, caps = [s for _, s, _ in named], [len(w) for _, _, w in named]
    rc0, plain = I.run_streams(lib, streams, caps)
    assert rc0 == 0 and [r[4] for r in plain] == [w for _, _, w in named]
    for dictionary, dev in ((None, True), (None, False), (b"", True), (b"", False), (history(1000, 12), True), (history(WINDOW + 5, 13), False)):
        rc, res = run_dict(lib, streams, caps, dictionary, on_device=dev)
        assert (rc, res) == (rc0, plain), (None if dictionary is None else len(dictionary), dev)
    return len(named)


# ---- 5. seeded token fuzz ------------------------------------------------------------------------------------------------------------------------
FUZZ_HISTORY = 5000
CLASSES = ("all_history", "ends_at_history_end", "straddles", "straddles_and_wraps", "output_below_synced", "output_across_synced", "chain", "from_history_start")
LENS = (3, 4, 63, 64, 65, 66, 128, 129, 257, 258, "random")


def random_token_streams(seed, nstreams, ntokens, hist_len=FUZZ_HISTORY):
    """-> ([(name, stream, blocks)], stats, history). Stored, fixed and dynamic blocks; the matches are aimed at the history (all of the source in it,
    ending at its end, straddling into the output with and without a wrap, starting at its first byte), at `synced` as the kernel keeps it (the
    output position at the last match whose source in the output reached past it) and at the match in front (chains). stats counts what every
    emitted match IS, whatever it was drawn as."""
    rs = random.Random(seed)
    hist = bytes(rs.randbytes(hist_len))
    stats = {c: 0 for c in CLASSES}
    ri = lambda lo, hi: lo + int(rs.random() * (hi - lo + 1))
    draw_len = lambda: (lambda c: ri(3, 258) if c == "random" else c)(LENS[ri(0, len(LENS) - 1)])
    out = []
    for k in range(nstreams):
        blocks, p, synced, left = [], 0, 0, ntokens

        def match(length, dist):
            nonlocal p, synced
            assert 1 <= dist <= min(p + hist_len, WINDOW) and 3 <= length <= 258, (length, dist, p)
            lo = p - dist
            hi = lo + min(dist, length)
            if hi < 0:
                stats["all_history"] += 1
            elif hi == 0:
                stats["ends_at_history_end"] += 1
            elif lo < 0:
                stats["straddles_and_wraps" if dist < length else "straddles"] += 1
            else:
                stats["output_across_synced" if hi > synced else "output_below_synced"] += 1
            stats["from_history_start"] += lo == -hist_len
            if hi > synced:
                synced = p
            p += length
            return (length, dist)

        def draw_match(near_start):
            length = draw_len()
            for _ in range(50):
                c = ri(0, 4) if near_start else ri(0, 9)
                lo = None
                if c == 0 and hist_len > length:                       # all of the source in the history
                    lo = ri(-hist_len, -length - 1)
                elif c == 1 and hist_len >= length:                    # ... ending at its end
                    lo = -length
                elif c == 2 and p >= 1 and length > 1:                 # from the history into the output
                    lo = ri(-min(length - 1, hist_len), min(-1, p - length))
                elif c == 3 and p <= length - 2:                       # ... and round again
                    lo = ri(max(-hist_len, p - length + 1), -1)
                elif c == 4:                                           # the first byte of the history
                    lo = -hist_len
                elif c == 5 and synced:                                # the output below `synced`
                    lo = ri(0, max(0, synced - length))
                    if lo + min(p - lo, length) > synced:
                        lo = None
                elif c == 6 and synced:                                # ... across it, ending at it, starting at it
                    lo = ri(max(0, synced - length), synced)
                elif c == 7:
                    lo = p - ri(1, 3)
                elif c >= 8:
                    lo = p - ri(1, min(p + hist_len, WINDOW))
                if lo is not None and 1 <= p - lo <= min(p + hist_len, WINDOW):
                    return match(length, p - lo)
            return match(length, 1 if p + hist_len >= 1 else None)

        while left > 0 or not blocks:
            kind = ("stored", "fixed", "dynamic", "dynamic")[ri(0, 3)]
            if kind == "stored":
                n = (0, 1, 63, 64, 65, ri(0, 300), ri(0, 300))[ri(0, 6)]
                blocks.append(("stored", rs.randbytes(n)))
                p += n
                left -= 1
                continue
            tokens = []
            for _ in range(ri(1, 60)):
                what = ri(0, 9)
                near_start = p < 300
                if what < (2 if near_start else 4):
                    n = (1, 1, 1, 2, 3, 63, 64, 65, ri(1, 20), ri(1, 150))[ri(0, 4 if near_start else 9)]
                    tokens.append(rs.randbytes(n) if kind == "fixed" else bytes(rs.choices(b"etaoin shr", k=n)))
                    p += n
                elif what < 9:
                    tokens.append(draw_match(near_start))
                else:                                      # a chain: every match sources from the bytes of the match in front of it
                    stats["chain"] += 1
                    length = draw_len()
                    tokens.append(match(length, ri(1, min(p + hist_len, 300))))
                    for _ in range(ri(2, 6)):
                        nxt = draw_len()
                        tokens.append(match(nxt, ri(1, length)))
                        length = nxt
                left -= 1
            blocks.append((kind, tokens))
        w = ListWriter()
        for i, (kind, body) in enumerate(blocks):
            final = i == len(blocks) - 1
            if kind == "stored":
                w.stored(body, final)
                continue
            if kind == "fixed":
                w.begin_fixed(final)
            else:
                pairs = [I.token_symbols(*t) for t in body if isinstance(t, tuple)]
                lit_used = sorted({256} | {b for t in body if isinstance(t, bytes) for b in t} | {a for a, _ in pairs})
                dist_used = sorted({b for _, b in pairs})
                shape = lambda used, n: I.ladder_lens(rs.sample(used, len(used)), n) if len(used) <= 16 and ri(0, 1) else I.balanced_lens(used, n)
                lit_lens = shape(lit_used, lit_used[-1] + 1 if lit_used[-1] > 256 else 257) if len(lit_used) > 1 else I._lens_of([(256, 1)], 257)
                dist_lens = shape(dist_used, dist_used[-1] + 1) if len(dist_used) > 1 else I._lens_of([(d, 1) for d in dist_used], (dist_used or [0])[-1] + 1)
                w.begin_dynamic(final, lit_lens, dist_lens, ops=I.rle_ops(lit_lens + dist_lens) if ri(0, 3) else None)
            for t in body:
                if isinstance(t, bytes):
                    w.dlits(t)
                else:
                    w.dmatch(*t)
            w.deob()
        out.append(("dictfuzz%d" % k, w.bytes(), blocks))
    return out, stats, hist


def check_token_fuzz(lib, seed, nstreams, ntokens, copies=1, made=None):
    """One batch of the generated streams, each `copies` times with a destination of its own. made: what random_token_streams gave another
    process. -> made."""
    streams, stats, hist = made or random_token_streams(seed, nstreams, ntokens)
    empty = [c for c, n in stats.items() if n == 0]
    assert not empty, "never drawn with seed %d: %s" % (seed, empty)
    named = [(name, s, replay(blocks, hist)) for name, s, blocks in streams]
    res = check_good(lib, named, hist, on_device=True, dict_lead=1, copies=copies)   # (host zlib with zdict against the replay first)
    for (name, _, blocks), r in zip(streams * copies, res):
        assert r[1] == len(blocks), (name, r[1], len(blocks))
    return streams, stats, hist


def check_token_fuzz_strided(lib_path, is_emulator, made, copies, tmp_path):
    """The same batch in a process of its own with ZULTRA_HIP_GRID_CAP=8: eight waves stride over it."""
    tests = os.path.dirname(os.path.abspath(__file__))
    handed = os.path.join(str(tmp_path), "dict_token_streams.pickle")
    with open(handed, "wb") as f:
        pickle.dump(made, f)
    code = ("import pickle, sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import inflate_dict_cases as D\nfrom zultra_amd._ffi import Lib\nL = Lib(%r)\nL.is_emulator = %r\n"
            "D.check_token_fuzz(L, 0, 0, 0, %d, pickle.load(open(%r, 'rb')))\nprint('strided ok')\n") % (os.path.dirname(tests), tests, lib_path, bool(is_emulator), copies, handed)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ZULTRA_HIP_GRID_CAP="8"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "strided ok" in r.stdout, r.stdout + r.stderr


# ---- 6. every bit flipped, cut at every byte ------------------------------------------------------------------------------------------------------
MUTANT_CAP = 1200


def check_flips(lib):
    """Every stream of hand_streams with every single bit flipped, one batch per dictionary: reason 0 exactly where host zlib with zdict inflates
    the mutant to its end, then with zlib's bytes and its count of stream bytes used. -> (mutants, those zlib accepts)."""
    total = benign = 0
    for h, group in by_history(hand_streams()):
        muts, labels = [], []
        for name, _, s, _ in group:
            for bit in range(8 * len(s)):
                m = bytearray(s)
                m[bit >> 3] ^= 1 << (bit & 7)
                muts.append(bytes(m))
                labels.append("%s bit %d" % (name, bit))
        rc, res = run_dict(lib, muts, [MUTANT_CAP] * len(muts), h)
        for label, m, (reason, blocks, out_size, src_used, out) in zip(labels, muts, res):
            ok, want, used = host_verdict(m, h)
            if ok and len(want) > MUTANT_CAP:
                assert reason == DST_FULL, (label, reason)
                continue
            assert (reason == OK) == ok, (label, reason, ok)
            if ok:
                benign += 1
                assert out == want and src_used == used, (label, out_size, len(want), src_used, used)
        total += len(muts)
    assert benign > 0
    return total, benign


def check_cuts(lib):
    """... and cut at every byte (the copies lie back to back: what follows an item's end is the stream's own next byte): reason 12, a prefix of the
    output, and host zlib does not reach the end either. -> cuts."""
    total = 0
    for h, group in by_history(hand_streams()):
        streams, sizes, caps, wants = [], [], [], []
        for name, _, s, want in group:
            for cut in range(len(s)):
                streams.append(s)
                sizes.append(cut)
                caps.append(len(want))
                wants.append((name, cut, want))
        rc, res = run_dict(lib, streams, caps, h, src_sizes=sizes)
        assert rc == len(streams)
        for (name, cut, want), s, (reason, blocks, out_size, src_used, out) in zip(wants, streams, res):
            assert reason == STREAM_END, (name, cut, reason)
            assert out == want[:out_size] and src_used <= cut, (name, cut, out_size, src_used)
            assert not host_verdict(s[:cut], h)[0], (name, cut)
        total += len(streams)
    return total


# ---- 7. bad arguments ------------------------------------------------------------------------------------------------------------------------------
def check_bad_arguments(lib):
    h = history(40, 14)
    s = write_fixed([("fixed", [(30, 35), b"!"])])
    want = replay([("fixed", [(30, 35), b"!"])], h)
    src = np.frombuffer(s, dtype=np.uint8).copy()
    hist = np.frombuffer(h, dtype=np.uint8).copy()
    dst = np.zeros(200, dtype=np.uint8)
    n = len(src)
    call = lambda items, d=hist, dn=len(h): lib.inflate_streams_dict(src, n, dst, 200, d, dn, items)[0]
    assert call([(0, n, 0, 100)], None, 40) == -1                                   # a NULL dictionary of 40 bytes
    assert call([(0, n, 0, 100), (0, n, 99, 100)]) == -1                             # what the plain call refuses: destination ranges overlap
    assert call([(0, n, 50, 100), (0, n, 0, 51)]) == -1
    assert call([(1, n, 0, 100)]) == -1                                              # an item past src_size
    assert call([(0, n, 101, 100)]) == -1                                            # ... past dst_size
    assert call(np.zeros((0, 4), dtype=np.uint64)) == -1                             # n == 0
    assert not dst.any(), "a refused call has written"
    # a device dictionary inside a device destination range, at its first and at its last byte, and right in front of it and behind it
    buf = V.DeviceCopy(lib, np.frombuffer(b"\0" * 100 + h + b"\0" * 200, dtype=np.uint8).copy())
    dsrc = V.DeviceCopy(lib, src)
    try:
        on_dev = lambda dst_off, cap, dict_at: lib.inflate_streams_dict(dsrc.ptr, n, buf.ptr, 340, buf.ptr + dict_at, 40, [(0, n, dst_off, cap)])[0]
        assert on_dev(139, 50, 100) == -1 and on_dev(60, 41, 100) == -1 and on_dev(0, 340, 100) == -1
        assert (I.device_read(lib, buf, 340).tobytes() == b"\0" * 100 + h + b"\0" * 200), "a refused call has written"
        assert on_dev(140, 50, 100) == 0 and on_dev(60, 40, 100) == 0
        back = I.device_read(lib, buf, 340).tobytes()
        assert back[140:171] == want and back[60:91] == want and back[100:140] == h
    finally:
        buf.free()
        dsrc.free()
    assert call([(0, n, 0, 100), (0, n, 100, 100)]) == 0 and (dst[:31].tobytes(), dst[100:131].tobytes()) == (want, want)


# ---- 8. the host API -------------------------------------------------------------------------------------------------------------------------------
def check_host_round_trip(lib, size, dict_size):
    """zultra_memory_compress_dict -> zultra_memory_decompress_dict in the three framings; the stream needs its dictionary."""
    raw = corpus.text_like(size, 31).tobytes()
    dictionary = dictionary_of(corpus.text_like, dict_size, 32)
    raw = dictionary[-min(dict_size, 200):] * 2 + raw[:size - 2 * min(dict_size, 200)]   # (the input quotes the dictionary's end: see zlib_streams)
    for f in (0, 1, 2):
        packed = lib.memory_compress(np.frombuffer(raw, dtype=np.uint8), f, 32768, dictionary=dictionary)
        assert packed is not None
        assert zlib.decompressobj({0: -15, 1: 15, 2: 31}[f], zdict=dictionary).decompress(packed) == raw if f < 2 else True
        assert lib.memory_decompress_dict(packed, f, len(raw), dictionary) == raw, f
        assert lib.memory_decompress_dict(packed, f, len(raw) + 100, dictionary) == raw, f
        assert lib.memory_decompress_dict(packed, f, len(raw) - 1, dictionary) is None, f
        if dict_size > WINDOW and f != 1:     # raw and gzip: the last 32768 bytes are all there is to a dictionary
            assert lib.memory_decompress_dict(packed, f, len(raw), dictionary[-WINDOW:]) == raw, f
        if dict_size >= 3:                    # (the match finder does not reach into a shorter one)
            assert lib.memory_decompress(packed, f, len(raw)) is None, f
            assert lib.memory_decompress_dict(packed, f, len(raw), None) is None, f
        other = bytes(b ^ 1 for b in dictionary)
        assert lib.memory_decompress_dict(packed, f, len(raw), other) is None or f != 1 or dict_size == 0, f   # zlib: the DICTID check


def check_host_zlib_framing(lib, size):
    raw = corpus.json_like(size, 33).tobytes()
    for dict_size in (258, 70000):
        dictionary = dictionary_of(corpus.json_like, dict_size, 34)
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_DEFAULT_STRATEGY, zdict=dictionary)
        packed = c.compress(raw) + c.flush()
        assert packed[1] & 0x20 and int.from_bytes(packed[2:6], "big") == zlib.adler32(dictionary)
        assert lib.memory_decompress_dict(packed, 1, len(raw), dictionary) == raw, dict_size         # a stream made by zlib with zdict
        wrong = dictionary[:-1] + bytes([dictionary[-1] ^ 1])
        assert lib.memory_decompress_dict(packed, 1, len(raw), wrong) is None                          # the DICTID check
        assert lib.memory_decompress_dict(packed, 1, len(raw), dictionary[1:]) is None
        assert lib.memory_decompress_dict(packed, 1, len(raw), None) is None                           # FDICT and no dictionary
        assert lib.memory_decompress_dict(packed, 1, len(raw), b"") is None
        assert lib.memory_decompress(packed, 1, len(raw)) is None                                      # zultra_memory_decompress keeps rejecting FDICT
        bad = bytearray(packed)                                                                        # a DICTID that is not the dictionary's
        bad[5] ^= 1
        assert lib.memory_decompress_dict(bytes(bad), 1, len(raw), dictionary) is None
        bad = bytearray(packed)                                                                        # the Adler-32 of the output is still checked
        bad[-1] ^= 1
        assert lib.memory_decompress_dict(bytes(bad), 1, len(raw), dictionary) is None
        plain = zlib.compress(raw, 6)                                                                  # no FDICT: the dictionary is not looked at
        assert not plain[1] & 0x20
        assert lib.memory_decompress_dict(plain, 1, len(raw), dictionary) == raw
        assert lib.memory_decompress_dict(plain, 1, len(raw), None) == raw
    # raw framing: a stream made by zlib against the last 32768 bytes decodes with the whole dictionary
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY, zdict=dictionary[-WINDOW:])
    packed = c.compress(raw) + c.flush()
    assert lib.memory_decompress_dict(packed, 0, len(raw), dictionary) == raw
    assert lib.memory_decompress_dict(packed + b"\0", 0, len(raw), dictionary) is None                 # a trailing byte


# ---- 9. the command-line tool ----------------------------------------------------------------------------------------------------------------------
def check_cli(cli, tmp_path):
    raw = corpus.text_like(100000, 9).tobytes()
    dictionary = dictionary_of(corpus.text_like, 20000, 35)
    raw = dictionary[-300:] + raw
    src, dic, other, back = tmp_path / "in.bin", tmp_path / "dict.bin", tmp_path / "other.bin", tmp_path / "back.bin"
    src.write_bytes(raw)
    dic.write_bytes(dictionary)
    other.write_bytes(dictionary_of(corpus.text_like, 20000, 36))
    run = lambda *a: subprocess.run([cli] + [str(x) for x in a], capture_output=True, text=True, timeout=300)
    for framing, wbits in (("gzip", 31), ("zlib", 15)):
        packed = tmp_path / ("out." + framing)
        r = run("-b", "65536", "-f", framing, "-D", dic, src, packed)
        assert r.returncode == 0, r.stdout + r.stderr
        assert zlib.decompressobj(wbits, zdict=dictionary).decompress(packed.read_bytes()) == raw if framing == "zlib" else True
        r = run("-x", "-f", framing, "-D", dic, packed, back)
        assert r.returncode == 0 and back.read_bytes() == raw, r.stdout + r.stderr
        r = run("-x", "-f", framing, packed, back)                     # no dictionary: zlib by FDICT, gzip by the first match into it
        assert r.returncode != 0, framing
        r = run("-x", "-f", framing, "-D", other, packed, back)        # another dictionary: zlib by the DICTID, gzip by its CRC-32
        assert r.returncode != 0, framing
    plain = tmp_path / "plain.gz"                                      # a run without -D is what it was
    assert run("-b", "65536", src, plain).returncode == 0
    assert zlib.decompress(plain.read_bytes(), 31) == raw
    assert run("-x", plain, back).returncode == 0 and back.read_bytes() == raw
    assert run("-D", tmp_path / "missing.bin", src, plain).returncode != 0
