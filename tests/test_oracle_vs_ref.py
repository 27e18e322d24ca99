"""CPU: pin the oracle against the reference itself, stage by stage and on whole streams, over seeded inputs covering the
reference's self-test grid (tool/zultra.c:529-534) and the edge cases of SURVEY.md Appendix A.

Every case records what one side computes — match rows, split offsets, sub-block costs, bits, final parse and code lengths,
whole streams, checksums — as a list of values and digests. The reference's records are stored in tests/golden/ref_answers.json
(written by tests/golden/make_golden.py from the compiled reference, oracle/_ref); the oracle's must equal them. Where oracle/_ref
is present the reference is also run live and its records compared with the stored ones."""
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

import corpus
import zlibs

ANSWERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_answers.json")


def _h(x):
    b = x if isinstance(x, bytes) else np.ascontiguousarray(x).tobytes()
    return hashlib.sha256(b).hexdigest()


class _OracleSide:
    """The oracle behind the interface of zlibs.Ref that the cases use."""

    class Probe:
        def __init__(self, o, win, prev, n):
            self.o, self.win, self.prev, self.n = o, win, prev, n
            self.m = o.find_matches(win, prev, n)

        def __enter__(self):
            return self

        def __exit__(self, *a):
            pass

        def matches(self):
            return self.m

        def split(self):
            return self.o.split(self.win, self.m, self.prev, self.n)

        def costs(self, start, size):
            return self.o.costs(self.win, self.m, self.prev, start, size)

        def deflate(self, start, size, is_dynamic):
            r = self.o.deflate(self.win, self.m, self.prev, start, size, is_dynamic)
            assert r[0] == 0, "oracle deflate failed at %d+%d" % (start, size)
            return r

    def __init__(self, oracle):
        self.o = oracle

    def probe(self, max_block, win, prev, n):
        return _OracleSide.Probe(self.o, win, prev, n)

    def memory_compress(self, data, flags, max_block, dictionary=None, cap=None):
        return self.o.memory_compress(data, flags, max_block, dictionary, cap=cap)

    def checksum(self, data, flags, start):
        return self.o.crc32(data, start) if flags == 2 else self.o.adler32(data, start)


def _stages(side, win, prev, n, max_block=65536):
    win = np.ascontiguousarray(win, dtype=np.uint8)
    with side.probe(max_block, win, prev, n) as P:
        rec = [["matches", _h(P.matches())]]
        sr = P.split()
        rec.append(["split", sr])
        at = prev
        for e in sr:
            size = e - at
            rec.append(["costs %d+%d" % (at, size), list(P.costs(at, size))])
            for dyn in (0, 1):
                r = P.deflate(at, size, dyn)
                rec.append(["deflate %d+%d dynamic=%d" % (at, size, dyn), [int(r[1]), _h(r[2]), _h(r[3]), _h(r[4]), _h(r[5])]])
            at = e
    return rec


def _stream(side, data, flags, bs, d=None, cap=None):
    out = side.memory_compress(data, flags, bs, d, cap=cap)
    if out is not None and cap is None:
        wb = {0: -15, 1: 15, 2: 31}[flags]
        dec = zlib.decompressobj(wb, zdict=bytes(d)) if (d is not None and flags != 2) else zlib.decompressobj(wb)
        assert dec.decompress(out) == bytes(np.ascontiguousarray(data, dtype=np.uint8).tobytes())
    return [["stream flags=%d bs=%d n=%d" % (flags, bs, len(data)), None if out is None else [len(out), _h(out)]]]


# ---- the cases: key -> side -> record --------------------------------------------------------------------------------------

def _case_stages_text_with_history(side):
    return _stages(side, corpus.text_like(98304, 3), 32768, 65536)


def _case_stages_text_first_block(side):
    return _stages(side, corpus.text_like(65536, 4), 0, 65536)


def _case_stages_selftest_grid(side, alphabet, prob):
    return _stages(side, corpus.selftest_data(24576, 123, alphabet, prob), 8192, 16384, 32768)


def _case_stages_degenerate(side):
    return (_stages(side, corpus.constant(40000), 4464, 35536) + _stages(side, corpus.periodic(30000, 3), 0, 30000)
            + _stages(side, corpus.noise(20000, 1), 0, 20000) + _stages(side, corpus.sparse_ones(40000), 8000, 32000)
            + _stages(side, corpus.text_like(10, 1), 0, 10) + _stages(side, corpus.text_like(3, 1), 0, 3) + _stages(side, corpus.text_like(1, 1), 0, 1))


def _case_stream_text(side, flags, bs):
    return _stream(side, corpus.text_like(250000, 9), flags, bs)


def _case_stream_phase_dependent_stored_fallback(side):
    t = corpus.text_like(150000, 7)
    d = np.concatenate([t[:70000], corpus.noise(140000, 3), t[70000:]])
    return sum((_stream(side, d, flags, bs) for flags, bs in [(2, 65536), (0, 32768), (1, 1 << 20)]), [])


def _case_stream_dictionary(side):
    t = corpus.text_like(140000, 7)
    return _stream(side, t[40000:], 1, 65536, t[:32768]) + _stream(side, t[40000:90000], 0, 65536, t[100:5000])


def _case_stream_small_and_ragged(side):
    t = corpus.text_like(70000, 2)
    rec = sum((_stream(side, t[:n], 2, 32768) for n in (1, 2, 3, 4, 100, 32768, 32769, 65535, 65536, 65537)), [])
    return rec + [["empty input", side.memory_compress(t[:0], 2, 0) is None]]


def _case_stream_output_too_small(side):
    t = corpus.text_like(4096, 2)
    return sum((_stream(side, t, 1, 0, cap=cap) for cap in range(0, 12)), [])


def _case_fuzz_streams(side):
    rs = np.random.RandomState(2024)
    rec = []
    for it in range(12):
        n = int(rs.randint(1, 120000))
        kind = it % 4
        if kind == 0:
            d = corpus.mixed(n, 100 + it)
        elif kind == 1:
            d = corpus.selftest_data(n, 200 + it, corpus.SELFTEST_ALPHABETS[it % 12], [0.0, 0.3, 0.7, 0.995][it % 4])
        elif kind == 2:
            d = corpus.text_like(n, 300 + it)
        else:
            d = np.concatenate([corpus.json_like(n // 2, it), corpus.noise(n - n // 2, it)])
        rec += _stream(side, d, int(rs.randint(0, 3)), [0, 32768, 65536][it % 3])
    return rec


def _case_checksums(side):
    d = corpus.text_like(100003, 5)
    return [["crc32", int(side.checksum(d, 2, 0))], ["adler32", int(side.checksum(d, 1, 1))]]


GRID_ALPHABETS = [1, 2, 15, 96, 256]
GRID_PROBS = [0.0, 0.5, 0.995]
STREAM_TEXT = [(2, 65536), (1, 32768), (0, 0)]

CASES = {"stages_text_with_history": (_case_stages_text_with_history, ()), "stages_text_first_block": (_case_stages_text_first_block, ()),
         "stages_degenerate": (_case_stages_degenerate, ()),
         "stream_phase_dependent_stored_fallback": (_case_stream_phase_dependent_stored_fallback, ()),
         "stream_dictionary": (_case_stream_dictionary, ()), "stream_small_and_ragged": (_case_stream_small_and_ragged, ()),
         "stream_output_too_small": (_case_stream_output_too_small, ()), "fuzz_streams": (_case_fuzz_streams, ()), "checksums": (_case_checksums, ())}
CASES.update({"stages_selftest_grid %d %r" % (a, p): (_case_stages_selftest_grid, (a, p)) for a in GRID_ALPHABETS for p in GRID_PROBS})
CASES.update({"stream_text %d %d" % fb: (_case_stream_text, fb) for fb in STREAM_TEXT})


def record(side, key):
    fn, args = CASES[key]
    return json.loads(json.dumps(fn(side, *args)))


def record_reference(path=ANSWERS):
    """Writes the compiled reference's records of every case (tests/golden/make_golden.py)."""
    ref = zlibs.Ref()
    with open(path, "w") as f:
        json.dump({key: record(ref, key) for key in CASES}, f, indent=0, sort_keys=True)
        f.write("\n")


# ---- the tests ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def answers():
    with open(ANSWERS) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def live_ref():
    """The compiled reference where it was built (oracle/_ref), else None: the stored records stand for it."""
    return zlibs.Ref() if zlibs.have_ref() else None


def _verify(key, oracle, answers, live_ref):
    want = answers[key]
    if live_ref is not None:
        assert record(live_ref, key) == want, "the compiled reference no longer gives the stored records: rerun tests/golden/make_golden.py"
    got = record(_OracleSide(oracle), key)
    assert len(got) == len(want), key
    for g, w in zip(got, want):
        assert g == w, "%s: %s" % (key, w[0])


def test_stages_text_with_history(oracle, answers, live_ref):
    _verify("stages_text_with_history", oracle, answers, live_ref)


def test_stages_text_first_block(oracle, answers, live_ref):
    _verify("stages_text_first_block", oracle, answers, live_ref)


@pytest.mark.parametrize("alphabet", GRID_ALPHABETS)
@pytest.mark.parametrize("prob", GRID_PROBS)
def test_stages_selftest_grid(oracle, answers, live_ref, alphabet, prob):
    _verify("stages_selftest_grid %d %r" % (alphabet, prob), oracle, answers, live_ref)


def test_stages_degenerate(oracle, answers, live_ref):
    _verify("stages_degenerate", oracle, answers, live_ref)


@pytest.mark.parametrize("flags,bs", STREAM_TEXT)
def test_stream_text(oracle, answers, live_ref, flags, bs):
    _verify("stream_text %d %d" % (flags, bs), oracle, answers, live_ref)


def test_stream_phase_dependent_stored_fallback(oracle, answers, live_ref):
    _verify("stream_phase_dependent_stored_fallback", oracle, answers, live_ref)


def test_stream_dictionary(oracle, answers, live_ref):
    _verify("stream_dictionary", oracle, answers, live_ref)


def test_stream_small_and_ragged(oracle, answers, live_ref):
    _verify("stream_small_and_ragged", oracle, answers, live_ref)
    assert oracle.memory_compress(corpus.text_like(10, 2)[:0], 2, 0) is None


def test_stream_output_too_small_fails_like_reference(oracle, answers, live_ref):
    _verify("stream_output_too_small", oracle, answers, live_ref)
    assert all(w[1] is None for w in answers["stream_output_too_small"])


def test_fuzz_streams(oracle, answers, live_ref):
    _verify("fuzz_streams", oracle, answers, live_ref)


def test_checksums(oracle, answers, live_ref):
    _verify("checksums", oracle, answers, live_ref)


# ---- the entropy stage on chosen histograms (tests/entropy_cases.py): the two oracle calls the emulator and GPU tests may be checked with, pinned to the
# compiled reference over every case, and what the cases reach, asserted from the reference side alone ----------------------------------------------------

def _entropy_ref(ref):
    if not ref.has_entropy:
        pytest.skip("this build of the compiled reference (oracle/_ref) is from before oracle/ref_probe.c had the entropy probes, and the sources to make it again are not here")
    return ref


def test_entropy_oracle_matches_reference_on_every_case(oracle, ref):
    import entropy_cases as ec
    ref = _entropy_ref(ref)
    case_list = ec.cases(ec.FULL)
    names, hist = [n for n, _ in case_list], ec.hist_of(case_list)
    zeros = np.zeros((len(hist), ec.NSYM), dtype=np.uint8)
    same = ec.lengths_of(ref.entropy_build(hist, 0, zeros)[0])
    for in_force, settled in ((zeros, None), (same, 1), (ec.changed_lengths(same), 0)):
        want = ref.entropy_build(hist, 0, in_force)
        assert settled is None or (want[0]["settled"] == settled).all()
        ec.assert_same(oracle.entropy_build(hist, 0, in_force), want, names, "oracle, pass 0")
    want = ref.entropy_build(hist, 3, zeros)
    ec.assert_same(oracle.entropy_build(hist, 3, zeros), want, names, "oracle, pass 3")
    assert [n for n, r in zip(names, want[0]) if r["failed"]] == ["symbol_287"]
    assert (want[0]["hdr_bits"][want[0]["failed"] == 0] > 14 + 3 * 4).all()
    for i in range(0, len(case_list), 256):   # (token lists of up to 64 Ki entries each: a few at a time)
        tok_info, tok_off = ec.init_input(case_list[i:i + 256])
        want = ref.entropy_init(tok_info, tok_off)
        ec.assert_same(oracle.entropy_init(tok_info, tok_off), want, names[i:i + 256], "oracle, init")
        assert not want[0]["failed"].any()


def test_entropy_cases_reach_the_limiter_and_never_run_off_its_list(ref):
    """Observed (5 000 random cases and the fixed ones): profiles/entropy_probe.txt."""
    import entropy_cases as ec
    case_list = ec.cases(ec.FULL)   # (asked of the reference's encoder functions, which every build of it has)
    table, alt_won, masks, hclens, past = ec.coverage(ref, case_list)
    print("coverage of %d cases: %r, alternative won %d, masks %r, hclen %r" % (len(case_list), table, alt_won, sorted(masks.items()), sorted(hclens.items())))
    assert past == [], "cases where the reference's repair reads past its symbol list are not cases: %s" % past
    for alphabet, (limited, third) in table.items():
        assert limited > 0 and third > 0, (alphabet, limited, third)
    assert 0 < alt_won < len(case_list)
    assert len(masks) >= 8 and 0 in masks and 31 in masks, sorted(masks)
    assert 19 in hclens and min(hclens) == 16, sorted(hclens.items())   # (16: the smallest HCLEN the reference writes for any of the cases)
    # the init mode builds from the same histograms (halved where the token list would be long), without the distance-code fix
    init = [ec.init_facts(ref, ec.init_hist(n, h)) for n, h in case_list]
    assert not any(lit[2] or dist[2] for lit, dist in init)
    assert sum(lit[0] for lit, _ in init) > 0 and sum(dist[0] for _, dist in init) > 0 and sum(lit[1] for lit, _ in init) > 0 and sum(dist[1] for _, dist in init) > 0
    # the smaller lists of the emulator and GPU tests are parts of this one
    full = {n: h.tobytes() for n, h in case_list}
    for part in (ec.EMU, ec.GPU):
        assert all(full.get(n) == h.tobytes() for n, h in ec.cases(part))
