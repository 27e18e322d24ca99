"""Histograms for the code-building kernels (zh_sb_init, zh_sb_build: zultra_amd/csrc/zh_encode.h over zh_huffman.h), and what the tests do with them.

The kernels are run on made-up sub-blocks by zultra_hip_entropy_probe (include/zultra_hip.h) and compared, record for record and header byte for header byte,
with the `checker` of tests/conftest.py: the compiled reference driven by oracle/ref_probe.c where it is there, the restatement oracle/zultra_oracle.c otherwise
(tests/test_oracle_vs_ref.py pins the one to the other over every case of this file).

A case is a name and 320 counts: 288 literal/length symbols WITHOUT the end-of-block symbol (the kernels add it) and 32 distance symbols. Every case keeps
sum(distance counts) == sum(counts of the length symbols 257..287), so that it is the histogram of a token list (tokens_of) and can go through zh_sb_init too,
and sum(literal/length counts) <= 2**21: a sub-block of the largest max-block — the sort keys are count << 9 | symbol in 32 bits, larger counts cannot occur.

What the cases reach is not taken on trust: reference_facts() asks the compiled reference for the UNLIMITED lengths of each alphabet a case builds and runs
them through limit_trace(), a plain model of the repair of huffencoder.c:310-341 (clamp, Kraft sum, the two loops). The model's trajectory depends on the
multiset of lengths only, so it needs no tie rule. tests/test_oracle_vs_ref.py asserts the coverage and that no case lets the repair's last loop run off the end
of its symbol list: there the reference reads a slot it never wrote, and the device fails the sub-block. Such histograms are not cases.
"""
import functools

import numpy as np

NLIT, NDIST, NSYM, EOB = 288, 32, 320, 256
MAX_SUM = 1 << 21
INIT_TOKENS = 1 << 16                                   # token lists of the init mode stay below this ...
INIT_WHOLE = ("fib_dist24", "fib_dist28")               # ... except those of these cases
RANDOM_KINDS = ("pareto", "pow2", "geometric", "ties", "loguniform")


def fib(k):
    """F(1)..F(k) = 1, 1, 2, 3, 5, ..."""
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def _balance(h, rs):
    """Make sum(dist) == sum(length symbols) with the least damage to either shape: a lighter distance side is scaled by a whole factor (a Fibonacci chain stays
    one) and its largest count takes the rest; a lighter length side gets the difference on one length symbol."""
    L, D = int(h[257:NLIT].sum()), int(h[NLIT:].sum())
    if L == D:
        return h
    if D < L:
        if D == 0:
            h[NLIT + int(rs.randint(0, 30))] = L
        else:
            h[NLIT:] *= L // D
            h[NLIT + int(np.argmax(h[NLIT:]))] += L - int(h[NLIT:].sum())
    else:
        used = np.flatnonzero(h[257:286])
        s = 257 + (int(used[rs.randint(len(used))]) if len(used) and rs.randint(2) else int(rs.randint(0, 29)))
        h[s] += D - L
    return h


def _place(counts, rs, symbols):
    h = np.zeros(NSYM, dtype=np.int64)
    h[rs.permutation(symbols)[:len(counts)]] = counts
    return h


_NOT_EOB = np.array([s for s in range(286) if s != EOB])


def _fixed_cases():
    out = []
    # Fibonacci counts with the end-of-block symbol as the first 1: F(2)..F(k) and the kernel's own 1 are F(1)..F(k), a chain of depth k - 1
    for k in (16, 17, 18, 20, 24, 28, 29):
        rs = np.random.RandomState(100 + k)
        out.append(("fib_lit%d" % k, _balance(_place(fib(k)[1:], rs, _NOT_EOB), rs)))
    for k in (17, 20, 24, 28):
        rs = np.random.RandomState(200 + k)
        h = np.zeros(NSYM, dtype=np.int64)
        h[rs.permutation(256)[:40]] = 3
        h[NLIT + rs.permutation(30)[:k]] = fib(k)
        total, lens = sum(fib(k)), 257 + rs.permutation(29)[:3]
        h[lens] = [total // 2, total // 3, total - total // 2 - total // 3]
        out.append(("fib_dist%d" % k, h))
    # the tied variant: F(1)..F(k) next to the end-of-block symbol's 1 — three counts of 1, and two interleaved chains of half the depth
    for k in (20, 28):
        rs = np.random.RandomState(300 + k)
        out.append(("fib_tied%d" % k, _balance(_place(fib(k), rs, _NOT_EOB), rs)))
    # n equal counts: across the rank-sort / bitonic switch (64 keys) and the network's 128 / 256 / 512 entries (with the end-of-block symbol: n + 1 keys)
    for n in (1, 2, 3, 64, 65, 128, 129, 255, 256, 257, 285):
        rs = np.random.RandomState(400 + n)
        out.append(("flat%d" % n, _balance(_place([7] * n, rs, _NOT_EOB), rs)))
    for n in (62, 63, 126, 127):   # n + 1 keys = 63, 64, 127, 128: the last rank sort and the last network of 128, on literals alone
        rs = np.random.RandomState(400 + n)
        out.append(("flat_lit%d" % n, _place([7] * n, rs, np.arange(256))))

    def edge(name, lit=(), dist=()):
        h = np.zeros(NSYM, dtype=np.int64)
        for s, c in lit:
            h[s] = c
        for s, c in dist:
            h[NLIT + s] = c
        assert h[257:NLIT].sum() == h[NLIT:].sum(), name
        out.append((name, h))

    text = [(s, 1 + (s * 7) % 23) for s in range(97, 123)]
    edge("empty")
    edge("one_literal", [(65, 1)])
    edge("one_literal_many", [(200, 5000)])
    edge("two_literals", [(0, 1), (255, 1)])
    edge("no_distance", text)
    edge("one_distance_0", text + [(257, 9)], [(0, 9)])
    edge("one_distance_5", text + [(260, 9)], [(5, 9)])
    edge("one_distance_29", text + [(270, 9)], [(29, 9)])
    edge("two_distances", text + [(258, 9), (266, 4)], [(3, 12), (17, 1)])
    edge("two_distances_0_1", text + [(258, 9)], [(0, 5), (1, 4)])
    edge("last_symbols", text + [(285, 6), (257, 3)], [(29, 2), (0, 7)])
    edge("low_literals", [(s, 1 + (s * 5) % 11) for s in range(0, 144, 3)])
    edge("symbol_287", text + [(287, 1)], [(4, 1)])   # nlit = 288: zultra_block_deflate refuses the header, the device fails the sub-block
    return out


def _random_case(kind, idx):
    rs = np.random.RandomState(10000 * (kind + 1) + idx)
    n = int(rs.randint(2, 286))
    if kind == 0:
        c = np.floor(rs.pareto(0.7, n) * 3 + 1)
    elif kind == 1:
        c = 2.0 ** rs.randint(0, 18, n)
    elif kind == 2:
        c = np.floor(1.6 ** np.arange(n % 30 + 2))
    elif kind == 3:
        c = rs.randint(1, 4, n).astype(np.float64)
    else:
        c = np.floor(np.exp(rs.uniform(0, 13, n)))
    c = np.minimum(c, 1 << 19).astype(np.int64)
    while c.sum() > (1 << 20):
        c = (c + 1) // 2
    nd = int(rs.randint(0, 31))
    if rs.randint(3):
        dc = np.floor(np.exp(rs.uniform(0, 12, nd))).astype(np.int64)
    else:
        dc = np.array(fib(min(nd, 27)), dtype=np.int64)
    while dc.sum() > (1 << 19):
        dc = (dc + 1) // 2
    if len(dc) == 0:
        return _place(c[:256], rs, np.arange(256))   # no distance symbol: no length symbol either
    h = _place(c, rs, _NOT_EOB)
    h[NLIT + rs.permutation(30)[:len(dc)]] = dc
    return _balance(h, rs)


@functools.lru_cache(maxsize=None)
def cases(per_kind):
    """[(name, counts)]: the fixed families and per_kind random histograms of each of the five kinds. A smaller list is a subset of a larger one."""
    out = _fixed_cases()
    for idx in range(per_kind):
        for kind, kname in enumerate(RANDOM_KINDS):
            out.append(("%s_%d" % (kname, idx), _random_case(kind, idx)))
    for name, h in out:
        assert h.min() >= 0 and h[EOB] == 0 and h[:NLIT].sum() < MAX_SUM and h[257:NLIT].sum() == h[NLIT:].sum() and h[NLIT + 30:].sum() == 0, name
    return [(name, h.astype(np.uint32)) for name, h in out]


FULL = 1000     # per kind: 5 000 random cases and the fixed ones — the oracle-vs-reference leg, where the coverage is asserted
GPU = 300       # the GPU test: a few hundred per kind
EMU = 24        # the emulator test (tests/test_entropy_emu.py says what that costs)


def hist_of(case_list):
    return np.stack([h for _, h in case_list])


def split_rows(hist, ntasks, seed=5):
    """hist[n, 320] -> hist_part[n, ntasks, 320]: every count cut at random into ntasks parts (what the tasks of a sub-block leave for zh_sb_build)."""
    rs = np.random.RandomState(seed)
    part = np.zeros((len(hist), ntasks, NSYM), dtype=np.uint32)
    left = hist.astype(np.int64)
    for j in range(ntasks - 1):
        take = np.floor(rs.random_sample(left.shape) * (left + 1)).astype(np.int64)
        part[:, j] = take
        left = left - take
    part[:, ntasks - 1] = left
    assert (part.sum(axis=1, dtype=np.int64) == hist).all()
    return part


def init_hist(name, h):
    """The histogram the init mode gets for a case: the case's own if its token list stays below INIT_TOKENS (or is one of INIT_WHOLE), halved until it does otherwise."""
    h = h.astype(np.int64)
    if name in INIT_WHOLE:
        return h
    rs = np.random.RandomState(7)
    while h[:NLIT].sum() > INIT_TOKENS:
        h = _balance((h + 1) // 2, rs)
    return h


def tokens_of(h, seed):
    """A token list whose histogram is h: one uint16 per token, symbol | distance symbol << 9; a length token carries a distance symbol, and which one it carries is
    drawn at random (only the two histograms matter)."""
    rs = np.random.RandomState(seed)
    lit = np.repeat(np.arange(257, dtype=np.uint16), h[:257].astype(np.int64))
    lens = np.repeat(np.arange(257, NLIT, dtype=np.uint16), h[257:NLIT].astype(np.int64))
    dsym = np.repeat(np.arange(NDIST, dtype=np.uint16), h[NLIT:].astype(np.int64))
    assert len(lens) == len(dsym)
    tok = np.concatenate([lit, lens | (rs.permutation(dsym) << 9)]).astype(np.uint16)
    return rs.permutation(tok)


def init_input(case_list):
    """-> (tok_info, tok_off) of the init mode for a case list"""
    toks = [tokens_of(init_hist(name, h), i) for i, (name, h) in enumerate(case_list)]
    off = np.zeros(len(toks) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(t) for t in toks])
    return (np.concatenate(toks) if toks else np.zeros(0, dtype=np.uint16)), off


# ---- comparing ---------------------------------------------------------------------------------------------------------------------------------------------

def normalised(recs):
    """The record with what it leaves undefined set to zero: the code of a symbol without a length (the kernels store whatever their workspace held), the padding."""
    r = recs.copy()
    r["lit_code"][r["lit_len"] == 0] = 0
    r["dist_code"][r["dist_len"] == 0] = 0
    r["reserved"] = 0
    return r


def assert_same(got, want, names, what):
    """Exact equality of the whole record and of the whole header slot, case by case; the message names the first case and field that differ."""
    (grec, gslot), (wrec, wslot) = got, want
    grec, wrec = normalised(grec), normalised(wrec)
    assert len(grec) == len(wrec) == len(names)
    if grec.tobytes() == wrec.tobytes() and np.array_equal(gslot, wslot):
        return
    for i, name in enumerate(names):
        for f in grec.dtype.names:
            assert np.array_equal(grec[i][f], wrec[i][f]), "%s: case %s (%d), field %s: got %s, want %s" % (what, name, i, f, grec[i][f], wrec[i][f])
        nb = (int(wrec[i]["hdr_bits"]) + 7) // 8
        assert np.array_equal(gslot[i], wslot[i]), "%s: case %s (%d): header bytes differ (%d bits): got %s, want %s" % (
            what, name, i, int(wrec[i]["hdr_bits"]), gslot[i][:nb + 4].tobytes().hex(), wslot[i][:nb + 4].tobytes().hex())


def changed_lengths(lens):
    """lens[n, 320] -> a copy with ONE length per row changed so that it differs after the defaults for unused symbols (9 / 6 bits) are in: the row's symbol walks
    through both alphabets and every stride of the wave."""
    out = lens.copy()
    for i in range(len(out)):
        s = (i * 37) % (NSYM - 2)     # (never the distance symbols 30, 31)
        eff = int(out[i, s]) or (9 if s < NLIT else 6)
        out[i, s] = eff % 15 + 1
    return out


def lengths_of(recs):
    return np.concatenate([recs["lit_len"], recs["dist_len"]], axis=1)


_memo = {}


def _once(key, make):
    """The inputs and the checker's answers are computed once per case list and shared by the tests that need them (they are never written to)."""
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def check_build(dev, checker, per_kind, ntasks, grid):
    """zh_sb_build on every case of cases(per_kind): pass 0 with the lengths it is about to build in force (settled, three passes saved each), pass 0 with one of
    them changed (not settled), pass 3 (distance-code fix, alternative, header). grid None: every sub-block through the one-per-workgroup form."""
    case_list = cases(per_kind)
    names, hist = [n for n, _ in case_list], hist_of(case_list)
    part = _once(("part", per_kind, ntasks), lambda: split_rows(hist, ntasks))
    same = _once(("same", id(checker), per_kind), lambda: lengths_of(checker.entropy_build(hist, 0, np.zeros((len(hist), NSYM), dtype=np.uint8))[0]))
    for in_force, settled in ((same, 1), (changed_lengths(same), 0)):
        want = _once(("pass0", id(checker), per_kind, settled), lambda: checker.entropy_build(hist, 0, in_force))
        assert (want[0]["settled"] == settled).all() and not want[0]["failed"].any()
        recs, slots, counters = dev.entropy_probe(grid, hist_part=part, in_force=in_force, pass_=0)
        assert_same((recs, slots), want, names, "pass 0, %d task rows, settled %d" % (ntasks, settled))
        assert counters == (3 * settled * len(names), 3 * settled * len(names))
    want = _once(("pass3", id(checker), per_kind), lambda: checker.entropy_build(hist, 3, same))
    recs, slots, counters = dev.entropy_probe(grid, hist_part=part, in_force=same, pass_=3)
    assert_same((recs, slots), want, names, "pass 3, %d task rows" % ntasks)
    assert counters == (0, 0)
    failed = [n for n, r in zip(names, want[0]) if r["failed"]]
    assert failed == [n for n in names if n == "symbol_287"], failed


def check_init(dev, checker, per_kind, grid):
    """zh_sb_init on the token lists of every case of cases(per_kind)"""
    case_list = cases(per_kind)
    names = [n for n, _ in case_list]
    tok_info, tok_off = _once(("tokens", per_kind), lambda: init_input(case_list))
    want = _once(("init", id(checker), per_kind), lambda: checker.entropy_init(tok_info, tok_off))
    recs, slots, _ = dev.entropy_probe(grid, tok_info=tok_info, tok_off=tok_off)
    assert_same((recs, slots), want, names, "init")
    assert not want[0]["failed"].any() and want[0]["is_dynamic"].any() and not want[0]["is_dynamic"].all()   # (both block types are among the cases)


# ---- what the cases reach, from the reference side alone ---------------------------------------------------------------------------------------------------

def limit_trace(lens, maxbits):
    """The repair of huffencoder.c:310-341 on the multiset of non-zero lengths -> (limited?, last loop active?, last loop runs off the list?)"""
    ls = sorted(int(l) for l in lens if l)
    if not ls or ls[-1] <= maxbits:
        return (False, False, False)
    full = 1 << maxbits
    ls = [min(l, maxbits) for l in ls]
    k = sum(full >> l for l in ls)
    i = len(ls) - 1
    while k > full and i >= 0:
        while ls[i] < maxbits and k > full:
            ls[i] += 1
            k -= full >> ls[i]
        i -= 1
    third = k < full
    i = 0
    while k < full:
        if i >= len(ls):
            return (True, third, True)
        while k + (full >> ls[i]) <= full:
            k += full >> ls[i]
            ls[i] -= 1
        i += 1
    return (True, third, False)


@functools.lru_cache(maxsize=None)
def _ref_tools(ref):
    import ctypes as C

    L = ref.lib

    class Enc(C.Structure):   # zultra_huffman_encoder_t (huffman/huffencoder.h)
        _fields_ = [("nSymbols", C.c_int), ("nMax", C.c_int), ("ent", C.c_int * 288), ("cw", C.c_uint * 288), ("cl", C.c_int * 288)]

    def enc(freq, nsym, maxbits):
        e = Enc()
        L.zultra_huffman_encoder_init(C.byref(e), nsym, maxbits, 0)
        for i, f in enumerate(freq):
            e.ent[i] = int(f)
        return e

    def trace(freq, nsym, maxbits):
        e = enc(freq, nsym, maxbits)
        L.zultra_huffman_encoder_estimate_dynamic_codelens(C.byref(e))
        return limit_trace([e.cl[i] for i in range(nsym)], maxbits)

    return C, L, Enc, enc, trace


def init_facts(ref, h):
    """-> (lit, dist): limit_trace of the two alphabets zh_sb_init builds for the histogram h (no distance-code fix there)"""
    _, _, _, _, trace = _ref_tools(ref)
    lit = [int(x) for x in h[:NLIT]]
    lit[EOB] += 1
    return trace(lit, 288, 15), trace([int(x) for x in h[NLIT:]], 32, 15)


def reference_facts(ref, h):
    """What the last pass of a case goes through, asked of the compiled reference's own functions (ref = zlibs.Ref): a dict of
    lit / dist / alt / cl -> limit_trace of the unlimited lengths of that alphabet (cl: any of the twenty masks), past -> some repair would run off its list
    (nothing further is asked then), alt_won, mask (the winning one), hclen."""
    C, L, Enc, enc, trace = _ref_tools(ref)
    lit, dist = [int(x) for x in h[:NLIT]], [int(x) for x in h[NLIT:]]
    lit[EOB] += 1
    used = [i for i in range(30) if dist[i]][:2]
    if len(used) == 0:
        dist[0] = dist[1] = 1
    elif len(used) == 1:
        dist[1 if dist[0] else 0] = 1
    facts = {"lit": trace(lit, 288, 15), "dist": trace(dist, 32, 15), "alt": (False, False, False), "cl": (False, False, False), "past": False}
    if facts["lit"][2] or facts["dist"][2]:
        facts["past"] = True
        return facts
    el, ed = enc(lit, 288, 15), enc(dist, 32, 15)
    L.zultra_huffman_encoder_build_dynamic_codewords(C.byref(el))
    L.zultra_huffman_encoder_build_dynamic_codewords(C.byref(ed))
    ol, od = Enc.from_buffer_copy(el), Enc.from_buffer_copy(ed)
    cur, opt = C.c_int(0), C.c_int(0)
    L.zultra_block_evaluate_dynamic_cost(C.byref(ol), C.byref(od), C.byref(cur))
    tmp = (C.c_int * 320)()
    L.zultra_huffman_encoder_optimize_for_rle(288, ol.ent, tmp)
    L.zultra_huffman_encoder_optimize_for_rle(32, od.ent, tmp)
    ta, tb = trace(list(ol.ent), 288, 15), trace(list(od.ent)[:32], 32, 15)
    facts["alt"] = tuple(a or b for a, b in zip(ta, tb))
    if facts["alt"][2]:
        facts["past"] = True
        return facts
    L.zultra_huffman_encoder_build_dynamic_codewords(C.byref(ol))
    L.zultra_huffman_encoder_build_dynamic_codewords(C.byref(od))
    L.zultra_block_evaluate_dynamic_cost(C.byref(ol), C.byref(od), C.byref(opt))
    facts["alt_won"] = opt.value < cur.value
    if facts["alt_won"]:
        el, ed = ol, od
    nl = L.zultra_huffman_encoder_get_defined_var_lengths_count(C.byref(el), 257)
    nd = L.zultra_huffman_encoder_get_defined_var_lengths_count(C.byref(ed), 1)
    lens = (C.c_int * 320)(*([el.cl[i] for i in range(nl)] + [ed.cl[i] for i in range(nd)]))
    best, best_mask, best_hclen, m = None, -1, 0, 0
    while m <= 31:
        t = Enc()
        L.zultra_huffman_encoder_init(C.byref(t), 19, 7, 0)
        L.zultra_huffman_encoder_update_var_lengths_entropy(C.byref(t), nl + nd, lens, m)
        tr = trace([t.ent[i] for i in range(19)], 19, 7)
        facts["cl"] = tuple(a or b for a, b in zip(facts["cl"], tr))
        if tr[2]:
            facts["past"] = True
            return facts
        L.zultra_huffman_encoder_build_dynamic_codewords(C.byref(t))
        c = L.zultra_huffman_encoder_get_var_lengths_size(C.byref(t), nl + nd, lens, m)
        if best_mask == -1 or best >= c:
            best, best_mask, best_hclen = c, m, L.zultra_huffman_encoder_get_raw_table_size(C.byref(t))
        m = m + 2 if m >= 7 else m + 1
    facts["mask"], facts["hclen"] = best_mask, best_hclen
    return facts


def coverage(ref, case_list):
    """-> (table: alphabet -> [cases limited, cases with an active last loop], alt_won count, {mask: count}, {hclen: count}, cases whose repair runs off its list)"""
    table = {a: [0, 0] for a in ("lit", "dist", "cl", "alt")}
    masks, hclens, past, alt_won = {}, {}, [], 0
    for name, h in case_list:
        f = reference_facts(ref, h)
        if f["past"]:
            past.append(name)
            continue
        for a in table:
            table[a][0] += f[a][0]
            table[a][1] += f[a][1]
        alt_won += f["alt_won"]
        masks[f["mask"]] = masks.get(f["mask"], 0) + 1
        hclens[f["hclen"]] = hclens.get(f["hclen"], 0) + 1
    return table, alt_won, masks, hclens, past
