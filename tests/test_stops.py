"""Stop sequences matched inside the decode step, on the GPU.

The match kernel through its hook, generate and decode sessions, all against ``dsocr.stops.first_stop`` on the ids
the same call produces without stops: a stop never changes a selection, so the stopped ids are a prefix of the plain
ones and ``first_stop`` says where it ends.  Tiny config, the pages and prompt of tests/test_logit_bias.py.
"""
import ctypes as C
import os

import numpy as np
import pytest

from dsocr import DecodeParameters, DsocrError, ModelLoadArgs, Page, VisionSettings, build_prompt_tokens, load_model
from dsocr._lib import (MAX_STOP_LEN, MAX_STOP_SEQS, SESSION_LOGIT_BIAS, SESSION_LOGPROBS, SESSION_PER_REQUEST,
                        SESSION_STOP, lib)
from dsocr.stops import StopSet, first_stop
from dsocr.synth import SyntheticTokenizer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, "deepseek-ocr.rs_amd", "dsocr", "configs", "tiny.json")
TINY_VS = VisionSettings(256, 128, True)
SEED = 7
PROMPT = "<image>\nConvert the document to markdown."
SIZES = [(300, 420), (256, 256), (500, 140)]
N = 32  # max_new_tokens of the generate tests


def _set(*seqs):
    return StopSet(tuple(tuple(int(t) for t in q) for q in seqs), tuple(range(len(seqs))), ())


# ------------------------------------------------------------------ the kernel through its hook
def k_stop_match(seq_rows, tokens, emit, out0, out_len0, done0, seen0, hit0, out_cap):
    """dsocr_k_stop_match on host rows: per step (done, seen, hit, out_len), each [steps][B(, 2)]."""
    B, steps = len(seq_rows), len(tokens)
    n_seq = np.asarray([len(r) for r in seq_rows], np.int32)
    lens = np.zeros((B, MAX_STOP_SEQS), np.int32)
    ids = np.zeros((B, MAX_STOP_SEQS * MAX_STOP_LEN), np.int64)
    for b, r in enumerate(seq_rows):
        flat = [t for q in r for t in q]
        lens[b, :len(r)] = [len(q) for q in r]
        ids[b, :len(flat)] = flat
    tokens = np.ascontiguousarray(tokens, np.int32)
    emit = np.ascontiguousarray(emit, np.uint8)
    out = np.zeros((B, out_cap), np.int32)
    for b, o in enumerate(out0):
        out[b, :len(o)] = o
    out_len, done, seen = (np.asarray(a, np.int32).copy() for a in (out_len0, done0, seen0))
    hit = np.asarray(hit0, np.int32).reshape(B, 2).copy()
    rec = [np.zeros((steps, B), np.int32), np.zeros((steps, B), np.int32), np.zeros((steps, B, 2), np.int32),
           np.zeros((steps, B), np.int32)]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    st = lib().dsocr_k_stop_match(B, steps, out_cap, p(n_seq), p(lens), p(ids), p(tokens), p(emit), p(out), p(out_len),
                                  p(done), p(seen), p(hit), p(rec[0]), p(rec[1]), p(rec[2]), p(rec[3]))
    assert st == 0, lib().dsocr_last_error()
    return rec


def test_kernel_hook(gpu):
    """B = 8 rows over 12 steps, every step's done / seen / hit against first_stop on the row's stream so far."""
    r = np.random.default_rng(5)
    steps, cap, S = 12, 64, 0x5A5A5A5A
    stream = r.integers(600, 900, (8, cap)).astype(np.int32)  # what each row would emit, position by position
    start = np.zeros(8, np.int32)                             # tokens already in the row before step 0
    seqs = [[] for _ in range(8)]
    emit = np.ones((steps, 8), np.uint8)
    done0 = np.zeros(8, np.int32)
    # 0: a length-1 sequence matching the very first token
    seqs[0] = [(int(stream[0, 0]),)]
    # 1: a length-32 sequence completing exactly at out_len == 32 (26 tokens in the row, the 6th step completes it)
    start[1] = 26
    seqs[1] = [tuple(stream[1, :32])]
    # 2: a length-32 sequence while out_len < 32: its last 12 ids are the row's whole output, nothing below out[0]
    seqs[2] = [tuple(r.integers(100, 200, 20)) + tuple(stream[2, :12])]
    # 3: two sequences completing on the same step: the lower index is recorded
    seqs[3] = [(1, 2, 3), tuple(stream[3, 2:5]), tuple(stream[3, 4:5]), (4,)]
    # 4: a sequence that occurs in the stream, but only after a step in which the row selected EOS
    seqs[4] = [tuple(stream[4, 5:7])]
    emit[3, 4] = 0
    # 5: a row that is already done (its tail even equals its sequence: nothing is examined)
    start[5] = 9
    seqs[5] = [tuple(stream[5, 7:9]), tuple(stream[5, 9:10])]
    done0[5] = 1
    # 6: 16 sequences, only the last one matching
    seqs[6] = [tuple(r.integers(100, 200, 1 + i % 5)) for i in range(15)] + [tuple(stream[6, 6:10])]
    # 7: no stop set: done, seen and hit hold sentinels that must survive bit for bit
    done0[7] = S
    seen0 = start.copy()
    seen0[7] = S
    hit0 = np.tile(np.asarray([-1, 0], np.int32), (8, 1))
    hit0[7] = [S, S + 1]
    tokens = np.zeros((steps, 8), np.int32)
    want = []      # per step: (done, seen, hit, out_len) from first_stop and the rules of the final selection kernels
    done, olen = [int(d) for d in done0], [int(s) for s in start]
    seen, hit = [int(s) for s in seen0], [list(map(int, h)) for h in hit0]
    pos = olen[:]  # the next position of the row's stream
    for t in range(steps):
        for b in range(8):
            tokens[t, b] = stream[b, min(pos[b], cap - 1)]
            if done[b]:
                continue
            if not emit[t, b]:
                done[b] = 1
                continue
            pos[b] += 1
            olen[b] += 1
            if not seqs[b]:
                continue
            seen[b] = olen[b]
            fs = first_stop(stream[b, :olen[b]], seqs[b])
            if fs is not None and fs[0] == olen[b]:
                done[b], hit[b] = 1, [fs[1], len(seqs[b][fs[1]])]
        want.append(([*done], [*seen], [list(h) for h in hit], [*olen]))
    rec = k_stop_match(seqs, tokens, emit, [stream[b, :start[b]] for b in range(8)], start, done0, seen0, hit0, cap)
    for t in range(steps):
        for k in range(4):
            assert rec[k][t].tolist() == want[t][k], (t, k)
    d, s, h, n = (a[-1] for a in rec)
    assert h[0].tolist() == [0, 1] and n[0] == 1                       # the first token
    assert h[1].tolist() == [0, 32] and n[1] == 32                     # completes at out_len == 32
    assert h[2].tolist() == [-1, 0] and n[2] == 12 and d[2] == 0       # longer than the output: no match
    assert h[3].tolist() == [1, 3] and n[3] == 5                       # sequences 1 and 2 both end at token 5
    assert h[4].tolist() == [-1, 0] and d[4] == 1 and n[4] == 3 and s[4] == 3   # EOS at step 3: never examined again
    assert h[5].tolist() == [-1, 0] and s[5] == 9 and n[5] == 9        # already done
    assert h[6].tolist() == [15, 4] and n[6] == 10
    assert (int(d[7]), int(s[7]), h[7].tolist()) == (S, S, [S, S + 1])  # untouched
    assert rec[0][:, 7].tolist() == [S] * steps


# ------------------------------------------------------------------ generate
@pytest.fixture(scope="module")
def engine(gpu):
    eng = load_model(ModelLoadArgs(config_path=TINY, synthetic_seed=SEED, dtype="f16"))
    yield eng
    eng.close()


def _img(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def pages():
    tok = SyntheticTokenizer(512)
    out = []
    for i, hw in enumerate(SIZES):
        page = Page(_img(100 + i, *hw), TINY_VS)
        ids, mask = build_prompt_tokens(tok, PROMPT, [page.n_image_tokens])
        out.append((ids, mask, page))
    return out


def _steps(L, max_new):
    """decode_steps of a generate whose last page ended at token L (include/dsocr.h, dsocr_generate_stop): the done
    words are polled before the first step and after steps 8, 16, ... and max_new - 1."""
    return 0 if L == 1 else min(max_new - 1, -(-(L - 1) // 8) * 8)


def _stop_sets(plain):
    """(stop set, the expected (end, seq)) for the four cases, each asserted on the plain ids."""
    assert len(plain) == N
    cases = []
    t = plain[5]
    cases.append((_set((t,)), (plain.index(t) + 1, 0)))                 # a single id
    run = tuple(plain[4:7])
    fs = first_stop(plain, [run])
    assert fs is not None and 3 <= fs[0] <= 7 and plain[fs[0] - 3:fs[0]] == list(run)
    cases.append((_set(run), fs))                                       # a 3-id run
    cases.append((_set((999999 % 400 + 20, 3), (plain[0],)), (1, 1)))   # completes at token 1 (as sequence 1)
    cases.append((_set(tuple(plain)), (N, 0)))                          # completes at token 32 = max_new_tokens
    for ss, want in cases:
        assert first_stop(plain, ss.seqs) == want
    return cases


@pytest.mark.parametrize("kw", [{}, dict(do_sample=True, temperature=0.8, top_p=0.9, seed=11),
                                dict(repetition_penalty=1.3)], ids=["greedy", "sampled", "penalty"])
def test_generate_stops_where_first_stop_says(engine, pages, kw):
    p = DecodeParameters(max_new_tokens=N, **kw)
    req = (*pages[0], None)
    plain, hits = engine.generate_stops([req], [None], p, ignore_eos=True)
    plain = plain[0]
    assert hits == [(-1, 0)] and engine.last_timings()["decode_steps"] == N - 1
    assert plain == engine.generate_batch([req], p, ignore_eos=True)[0]
    for ss, (end, seq) in _stop_sets(plain):
        before = engine.stop_launches()
        got, hits = engine.generate_stops([req], [ss], p, ignore_eos=True)
        steps = engine.last_timings()["decode_steps"]
        print(f"end {end} seq {seq}: n_out {len(got[0])} hit {hits[0]} decode_steps {steps}")
        assert got[0] == plain[:end]
        assert hits[0] == (seq, len(ss.seqs[seq]))
        assert steps == _steps(end, N)
        assert engine.stop_launches() == before + 1 + steps  # the prefill's selection and every step


def test_generate_stops_with_logprobs(engine, pages):
    """top_k log-probabilities: the entries of the stopped run equal the plain run's prefix bit for bit."""
    p = DecodeParameters(max_new_tokens=N)
    req = (*pages[0], None)
    plain, _, lp, ti, tl = engine.generate_stops([req], [None], p, ignore_eos=True, top_k=3)
    assert len(lp[0]) == N
    for ss, (end, seq) in _stop_sets(plain[0]):
        got, hits, glp, gti, gtl = engine.generate_stops([req], [ss], p, ignore_eos=True, top_k=3)
        assert got[0] == plain[0][:end] and hits[0] == (seq, len(ss.seqs[seq]))
        assert len(glp[0]) == end
        assert glp[0].tobytes() == lp[0][:end].tobytes()
        assert gti[0].tobytes() == ti[0][:end].tobytes() and gtl[0].tobytes() == tl[0][:end].tobytes()


def test_generate_stop_stream_sees_tokens_as_emitted(engine, pages):
    """One page with its stream callback: every token arrives as it is emitted, the matched ones included, and the
    done word is polled after every step, so the engine runs exactly end - 1 decode steps."""
    p = DecodeParameters(max_new_tokens=N)
    req = (*pages[0], None)
    plain = engine.generate_stops([req], [None], p, ignore_eos=True)[0][0]
    for ss, (end, seq) in _stop_sets(plain):
        seen = []
        got, hit = engine.generate_stop_stream(req, ss, p, lambda n, t: seen.append((n, list(t))), ignore_eos=True)
        assert got == plain[:end] and hit == (seq, len(ss.seqs[seq]))
        assert seen == [(n, plain[:n]) for n in range(1, end + 1)]
        assert engine.last_timings()["decode_steps"] == end - 1
    seen = []
    got, hit = engine.generate_stop_stream(req, None, p, lambda n, t: seen.append(n), ignore_eos=True)
    assert got == plain and hit == (-1, 0) and seen == list(range(1, N + 1))


def test_generate_mixed_batch(engine, pages):
    """Three pages, one with stops: the two without produce what they produce in the batch without stops."""
    p = DecodeParameters(max_new_tokens=N)
    reqs = [(*pg, None) for pg in pages]
    plain, _ = engine.generate_stops(reqs, [None] * 3, p, ignore_eos=True)
    ss = _set(tuple(plain[2][:6]))
    got, hits = engine.generate_stops(reqs, [None, None, ss], p, ignore_eos=True)
    assert got[0] == plain[0] and got[1] == plain[1] and got[2] == plain[2][:6]
    assert hits == [(-1, 0), (-1, 0), (0, 6)]


# ------------------------------------------------------------------ sessions
FLAGS = [dict(), dict(per_request=True, logprobs=True, logit_bias=True)]
FLAG_BITS = [SESSION_STOP, SESSION_STOP | SESSION_PER_REQUEST | SESSION_LOGPROBS | SESSION_LOGIT_BIAS]


def _P(m):
    return DecodeParameters(max_new_tokens=m)


def _adm(flags, m):
    return dict(params=_P(m)) if flags.get("per_request") else dict(max_new_tokens=m)


@pytest.fixture(scope="module")
def single(engine, pages):
    """Every page decoded alone for 20 tokens, once."""
    return [engine.generate(*pg, None, _P(20)) for pg in pages]


@pytest.mark.parametrize("flags,bits", list(zip(FLAGS, FLAG_BITS)), ids=["stop", "all-flags"])
def test_session_mixed_batch_and_mid_burst(engine, pages, single, flags, bits):
    """Slots {none, none, stops}: the stop fires in the middle of the first 8-step burst and leaves out_len at the
    match; the two other pages produce bit for bit what they produce alone."""
    assert all(len(s) == 20 for s in single)
    ss = _set((7, 8, 9), tuple(single[2][:5]))
    assert first_stop(single[2], ss.seqs) == (5, 1)
    need = max(len(pg[0]) for pg in pages) + 21 + 8
    before = engine.stop_launches()
    with engine.open_session(3, need, _P(20), stops=True, **flags) as sess:
        assert sess.info()["flags"] == bits
        assert sess.admit(*pages[0], **_adm(flags, 20)) == 0
        sess.step(2)
        assert engine.stop_launches() == before          # no active page carries a stop set yet
        assert sess.admit(*pages[1], **_adm(flags, 20)) == 1
        assert sess.admit(*pages[2], stops=ss, **_adm(flags, 20)) == 2
        assert sess.stop_hit(2) == (-1, 0)
        st = sess.step(8)
        assert engine.stop_launches() == before + 1 + 8  # the admission's selection, then one per step
        assert st[2].done and st[2].out_len == 5 and not st[0].done and st[0].out_len == 11
        assert sess.stop_hit(2) == (1, 5) and sess.stop_hit(0) == (-1, 0)
        ids2, _ = sess.retire(2)
        sess.step(8)
        sess.step(8)
        assert all(s.done for s in sess.poll())
        ids1, _ = sess.retire(1)
        ids0, _ = sess.retire(0)
    assert ids2 == single[2][:5] and ids1 == single[1] and ids0 == single[0]


@pytest.mark.parametrize("flags", FLAGS, ids=["stop", "all-flags"])
def test_session_stop_follows_the_compaction(engine, pages, single, flags):
    """The page with stops is moved into a retired lower slot before its stop fires: it fires at the same token and
    the hit is read at the page's new slot."""
    ss = _set(tuple(single[2][:7]))
    assert first_stop(single[2], ss.seqs) == (7, 0)
    short = engine.generate(*pages[0], None, _P(4))
    need = max(len(pg[0]) for pg in pages) + 21 + 8
    with engine.open_session(2, need, _P(20), stops=True, **flags) as sess:
        sess.admit(*pages[0], **_adm(flags, 4))
        sess.admit(*pages[2], stops=ss, **_adm(flags, 20))
        st = sess.step(3)
        assert st[0].done and st[1].out_len == 4 and not st[1].done
        ids0, moved = sess.retire(0)
        assert moved == 1 and ids0 == short
        assert sess.stop_hit(0) == (-1, 0) and sess.slot_stops(0) == (ss, False)
        st = sess.step(8)
        assert st[0].done and st[0].out_len == 7
        assert sess.stop_hit(0) == (0, 7)
        res, _ = sess.retire_stopped(0, lambda ids: " ".join(map(str, ids)))
    assert res.tokens == single[2][:0] and res.stop_reason == 0  # the whole output was the stop: trimmed by match_len


def test_session_staged_set_is_consumed_once(engine, pages, single):
    """A staged set is consumed by the next admission call whether that call succeeds or not."""
    ss = _set((single[1][0],))
    need = len(pages[1][0]) + 21 + 8
    with engine.open_session(2, need, _P(20), stops=True) as sess:
        sess._stage_stops((ss, False))
        with pytest.raises(DsocrError):
            sess.admit(*pages[1], max_new_tokens=10 ** 6)       # refused: the staged set goes with it
        assert sess.info()["active"] == 0
        assert sess.admit(*pages[1], max_new_tokens=20) == 0    # no stop set: the whole run
        sess.step(8), sess.step(8), sess.step(8)
        assert sess.stop_hit(0) == (-1, 0)
        assert sess.retire(0)[0] == single[1]
        sess._stage_stops((ss, False))
        assert sess.admit(*pages[1], max_new_tokens=20) == 0    # consumed by the call that succeeds
        assert sess.poll()[0].done and sess.stop_hit(0) == (0, 1)
        assert sess.retire(0)[0] == single[1][:1]
        assert sess.admit(*pages[1], max_new_tokens=20) == 0    # ... once
        assert not sess.poll()[0].done


def test_session_admission_forms(engine, pages, single):
    """The same set through admit, admit_prefix and admit_begin / advance with 32-row chunks, a length-1 stop on the
    admission's first selection included; admit_cancel drops the staged set."""
    ids, mask, page = pages[0]
    want = single[0]
    ss = _set(tuple(want[:6]))
    assert first_stop(want, ss.seqs) == (6, 0)
    one = _set((want[0],))
    rows = max(i for i, m in enumerate(mask) if m) + 1
    assert len(ids) > 32
    got, first = {}, {}

    def run(sess):
        sess.step(8)
        sess.step(8)
        hit = sess.stop_hit(0)
        return sess.retire(0)[0], hit

    with engine.open_session(2, len(ids) + 21 + 8, _P(20), stops=True) as sess:
        assert sess.admit(ids, mask, page, max_new_tokens=20, stops=ss) == 0
        handle = sess.keep_prefix(0, rows)
        got["admit"] = run(sess)
        assert sess.admit_prefix(handle, ids, mask, max_new_tokens=20, stops=ss) == 0
        got["prefix"] = run(sess)
        sess.admit_begin(ids, mask, page, chunk_rows=32, max_new_tokens=20, stops=ss)
        sess.admit_advance()
        sess.admit_cancel()
        assert sess.admit(*pages[1], max_new_tokens=20) == 0     # begun with stops, cancelled: this page has none
        sess.step(8), sess.step(8), sess.step(8)
        got["after_cancel"] = (sess.retire(0)[0], None)
        for name, stops in (("chunked", ss), ("chunked_first", one)):
            sess.admit_begin(ids, mask, page, chunk_rows=32, max_new_tokens=20, stops=stops)
            done, slices = False, 0
            while not done:
                done, slot = sess.admit_advance()
                slices += 1
            assert slot == 0 and slices >= 3
            first[name] = sess.poll()[0]
            got[name] = run(sess)
        assert sess.admit_prefix(handle, ids, mask, max_new_tokens=20, stops=one) == 0
        first["prefix_first"] = sess.poll()[0]
        got["prefix_first"] = run(sess)
    for name in ("admit", "prefix", "chunked"):
        assert got[name] == (want[:6], (0, 6)), name
    assert got["after_cancel"][0] == single[1]
    for name in ("chunked_first", "prefix_first"):
        assert first[name].done and first[name].out_len == 1, name
        assert got[name] == (want[:1], (0, 1)), name


def test_off_means_off(engine, pages, single):
    """No stop set anywhere: no match launch, and the ids of a session opened without the flag."""
    before = engine.stop_launches()
    assert engine.generate(*pages[0], None, _P(20)) == single[0]
    assert engine.generate_stops([(*pages[0], None)], [None], _P(20))[0][0] == single[0]
    out = []
    for flag in (False, True):
        with engine.open_session(2, len(pages[0][0]) + 21 + 8, _P(20), stops=flag) as sess:
            assert sess.info()["flags"] == (SESSION_STOP if flag else 0)
            sess.admit(*pages[0], max_new_tokens=20)
            sess.admit(*pages[1], max_new_tokens=20)
            sess.step(8), sess.step(8), sess.step(8)
            out.append([sess.retire(1)[0], sess.retire(0)[0]])
    assert out[0] == out[1] == [single[1], single[0]]
    assert engine.stop_launches() == before


def _einval(fn, *a, **kw):
    with pytest.raises(DsocrError) as ei:
        fn(*a, **kw)
    assert ei.value.status == 1, ei.value


def test_refusals(engine, pages, single):
    ss = _set((single[0][3],))
    req = (*pages[0], None)
    _einval(engine.generate_stops, [req], [ss], DecodeParameters(max_new_tokens=4, use_cache=False))
    old = os.environ.get("DSOCR_PERSIST")
    os.environ["DSOCR_PERSIST"] = "1"
    try:
        _einval(engine.generate_stops, [req], [ss], _P(4))
    finally:
        if old is None:
            os.environ.pop("DSOCR_PERSIST", None)
        else:
            os.environ["DSOCR_PERSIST"] = old
    for bad in (_set(*[(i + 20,) for i in range(17)]), _set(tuple(range(20, 53))), _set(()), _set((engine.vocab,)),
                _set((5, 6), (5, 6))):
        _einval(engine.generate_stops, [req], [bad], _P(4))
    from dsocr.engine import _stop_c
    keep = []
    rec = _stop_c(ss, keep)
    assert lib().dsocr_session_stage_stop(engine._h, C.byref(rec)) == 1      # no session open
    with engine.open_session(2, len(pages[0][0]) + 21 + 8, _P(20)) as sess:  # opened without the flag
        sess.admit(*pages[1], max_new_tokens=20)
        sess.step(2)
        assert lib().dsocr_session_stage_stop(engine._h, C.byref(rec)) == 1
        _einval(sess.admit, *pages[0], max_new_tokens=20, stops=ss)
        assert sess.info()["active"] == 1
        sess.step(8), sess.step(8), sess.step(8)
        assert sess.retire(0)[0] == single[1]                               # the running slot is as it was
    assert engine.generate(*pages[0], None, _P(20)) == single[0]            # nothing was left behind
