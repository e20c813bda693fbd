"""Guided decoding on the GPU: a per-request token automaton in the decode step.

The two kernels through their hooks against NumPy, bit for bit; the engine against the CPU oracle, whose
``select_token_id`` is patched here to mask its ``logits`` argument with ``TokenAutomaton.mask_row`` in the state
that ``TokenAutomaton.walk`` gives for the generated part of the context (the semantics restated, statelessly:
nothing under ``oracle/`` changes); decode sessions against the same page decoded alone.  Tiny config (vocab 512,
EOS 1), the pages and prompt of tests/test_session.py.

The logits trace cannot be asked for together with an automaton (the trace entry takes none), so there is no such
refusal to test.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from dsocr import DecodeParameters, DsocrError, ModelLoadArgs, Page, VisionSettings, build_prompt_tokens, load_model
from dsocr._lib import SESSION_GUIDED, GuidedC, lib
from dsocr.constraint import merge_constraint
from dsocr.engine import _guided_c
from dsocr.guided import TokenAutomaton, automaton_from_sequences
from dsocr.ngram_window import NgramWindow
from dsocr.penalties import Penalties
from dsocr.stops import StopSet
from dsocr.synth import SyntheticTokenizer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, "deepseek-ocr.rs_amd", "dsocr", "configs", "tiny.json")
TINY_VS = VisionSettings(256, 128, True)
SEED = 7
EOS = 1
PROMPT = "<image>\nConvert the document to markdown."
SIZES = [(300, 420), (256, 256), (500, 140)]
# test_logprobs.py's bound for a log-probability against float64 NumPy: LP_C * 2**-23 * max(1, max|l - m|)
LP_C = 32.3
EPS = 2.0 ** -23
NAN_BITS = np.uint32(0x7FC12345)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _mask_ld(V):
    return ((V + 31) // 32 + 3) // 4 * 4


# ------------------------------------------------------------------ the kernels through their hooks
def _mask_automaton(V):
    """Five states: 0 one edge; 1 edges on the word boundaries 0, 31, 32, V - 1 (accepting); 2 a spread of ids (not
    accepting); 3 every eighth id from 8 on (accepting: whole mask bytes with one bit); 4 terminal."""
    edges = [[5], sorted({0, 31, 32, V - 1}), sorted({2, 7, 8, 15, 16, V // 2, V - 2}), list(range(8, V, 8)), []]
    eos = 3
    edges = [[t for t in e if t != eos] for e in edges]
    row_ptr = np.cumsum([0] + [len(e) for e in edges]).tolist()
    tok = [t for e in edges for t in e]
    return TokenAutomaton(5, 0, (0, 1, 0, 1, 0), row_ptr, tok, [4] * len(tok)), eos


@pytest.mark.parametrize("V,ld,off", [(37, 40, 0), (1003, 1008, 1), (4104, 4104, 3), (129280, 129280, 0)])
def test_mask_hook(gpu, V, ld, off):
    """B = 3 with the middle row's flag 0, each of the states 0..3 in turn for rows 0 and 2 (row 2 one state ahead).
    Kept logits keep their bits, the others are -inf, the flag-0 row and the columns [V, ld) keep a NaN pattern."""
    aut, eos = _mask_automaton(V)
    aut.validate(V, eos)
    r = np.random.default_rng(V + off)
    B, mld = 3, _mask_ld(V)
    keep = []
    rec = _guided_c(aut, keep)
    on = np.asarray([1, 0, 1], np.int32)
    done = np.zeros(B, np.int32)
    want_mask = np.zeros((aut.n_states, mld), np.uint32)
    for s in range(aut.n_states):
        for t in np.nonzero(aut.mask_row(s, V, eos))[0]:
            want_mask[s, t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    for s0 in range(4):
        state = np.asarray([s0, 2, (s0 + 1) % 4], np.int32)
        logits = r.standard_normal((B, ld)).astype(np.float32)
        logits[r.random((B, ld)) < 0.05] = -np.inf
        bits = logits.view(np.uint32)
        bits[:, V:] = NAN_BITS
        bits[1, :] = NAN_BITS
        got = logits.copy()
        mask = np.full((aut.n_states, mld), 0xDEADBEEF, np.uint32)
        st = lib().dsocr_k_guided_mask(B, V, ld, off, _p(got), C.byref(rec), eos, _p(on), _p(state), _p(done), _p(mask))
        assert st == 0, lib().dsocr_last_error()
        assert np.array_equal(mask, want_mask)
        want = logits.copy()
        for b in (0, 2):
            want[b, :V][~aut.mask_row(int(state[b]), V, eos)] = -np.inf
        assert got.tobytes() == want.tobytes()
    # a done row and a violated row (state -1) are left alone
    state = np.asarray([0, 0, -1], np.int32)
    done = np.asarray([1, 0, 0], np.int32)
    logits = r.standard_normal((B, ld)).astype(np.float32)
    got = logits.copy()
    st = lib().dsocr_k_guided_mask(B, V, ld, off, _p(got), C.byref(rec), eos, _p(on), _p(state), _p(done), _p(mask))
    assert st == 0, lib().dsocr_last_error()
    assert got.tobytes() == logits.tobytes()


def test_advance_hook(gpu):
    """A scripted 12-step run over B = 4 (row 3: flag 0).  State 0 has 200 edges (the binary search), state 1 has 3
    (the strided compare), state 2 exactly 64 and state 3 exactly 65 (both sides of the threshold), state 4 is
    terminal.  Rows: 0 walks 0 -> 1 -> 2 -> 3 -> 4 (complete) with a step in which nothing is appended; 1 takes a
    token without an edge from state 1 (violated); 2 loops in state 0 and never ends."""
    e0 = list(range(10, 410, 2))            # 200 edges: 10 -> 0 (loop), 408 (the last) -> 1, the others -> 0
    e1 = [3, 50, 400]                       # 50 -> 2
    e2 = list(range(100, 164))              # 64 edges: 163 (the last lane) -> 3
    e3 = list(range(200, 265))              # 65 edges: 200 (the first) -> 4
    edges = [e0, e1, e2, e3, []]
    nxt = [[1 if t == 408 else 0 for t in e0], [2 if t == 50 else 1 for t in e1], [3 if t == 163 else 2 for t in e2],
           [4 if t == 200 else 3 for t in e3], []]
    row_ptr = np.cumsum([0] + [len(e) for e in edges]).tolist()
    aut = TokenAutomaton(5, 0, (0, 0, 0, 0, 1), row_ptr, [t for e in edges for t in e], [n for e in nxt for n in e])
    aut.validate(512, EOS)
    B, steps = 4, 12
    on = np.asarray([1, 1, 1, 0], np.int32)
    script = {
        0: [(408, 1), (3, 1), (0, 0), (50, 1), (100, 1), (163, 1), (264, 1), (200, 1), (10, 1), (10, 1), (10, 1), (10, 1)],
        1: [(12, 1), (408, 1), (400, 1), (51, 1), (10, 1), (10, 1), (10, 1), (10, 1), (10, 1), (10, 1), (10, 1), (10, 1)],
        2: [(10, 1), (406, 1), (10, 0), (12, 1), (10, 1), (10, 1), (10, 1), (10, 1), (10, 1), (10, 1), (10, 1), (10, 1)],
        3: [(7, 1)] * 12,
    }
    tokens = np.asarray([[script[b][i][0] for b in range(B)] for i in range(steps)], np.int32)
    emit = np.asarray([[script[b][i][1] for b in range(B)] for i in range(steps)], np.uint8)
    out = np.full((steps, B, 4), -7, np.int32)
    keep = []
    rec = _guided_c(aut, keep)
    st = lib().dsocr_k_guided_advance(B, steps, C.byref(rec), _p(on), _p(tokens), _p(emit), _p(out))
    assert st == 0, lib().dsocr_last_error()
    # the reference: TokenAutomaton.step on what the row appended
    state, seen, status, done = [0, 0, 0, 0], [0] * B, [0] * B, [0] * B
    for i in range(steps):
        for b in range(B):
            if on[b] and not done[b] and emit[i, b] and state[b] >= 0:
                seen[b] += 1
                state[b], status[b] = aut.step(state[b], int(tokens[i, b]))
                done[b] = int(status[b] != 0)
            want = [state[b], seen[b], status[b], done[b]] if on[b] else [0, 0, 0, 0]
            assert out[i, b].tolist() == want, (i, b, out[i, b].tolist(), want)
    assert out[-1, 0].tolist() == [4, 7, 1, 1] and out[-1, 1].tolist() == [-1, 4, 2, 1] and out[-1, 2, 3] == 0


# ------------------------------------------------------------------ the engine against the oracle
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


class Oracle:
    """The CPU oracle on page 0, with ``oracle.model.select_token_id`` patched per call to apply the automaton."""

    def __init__(self):
        import oracle.model as om
        from oracle.weights import Weights
        self.om = om
        self.model = om.OracleModel(json.load(open(TINY)), Weights(seed=SEED, dtype="f16"))
        self.emb, _ = self.model.image_embeddings(_img(100, *SIZES[0]), 256, 128, True)

    def generate(self, ids, mask, max_new, aut=None, **kw):
        om, real = self.om, self.om.select_token_id
        P = len(ids)

        def select(logits, context, repetition_penalty=1.0, no_repeat_ngram_size=None, **sel):
            l = np.asarray(logits, np.float32)
            if aut is not None:
                state, status = aut.walk(int(c) for c in list(context)[P:])
                if status == 0:
                    l = np.where(aut.mask_row(state, l.shape[-1], EOS), l, np.float32(-np.inf)).astype(np.float32)
            return real(l, context, repetition_penalty, no_repeat_ngram_size, **sel)

        om.select_token_id = select
        try:
            out, _ = self.model.generate(ids, mask, self.emb, max_new, eos_token_id=EOS, **kw)
        finally:
            om.select_token_id = real
        out = [int(t) for t in out]
        if aut is not None:  # the device ends the page where the automaton completes (or is violated)
            for n in range(1, len(out) + 1):
                if aut.walk(out[:n])[1] != 0:
                    return out[:n]
        return out


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


@pytest.fixture(scope="module")
def plain(engine, pages):
    """The unconstrained greedy run of page 0 (24 tokens), shared."""
    return engine.generate(*pages[0], None, DecodeParameters(max_new_tokens=24))


def _trie(plain):
    """Four choices of 3..6 tokens: two start with the unconstrained run's first token, all continue with ids it
    never emits."""
    never = [t for t in range(2, 512) if t not in plain]
    a = plain[0]
    return [[a, never[0], never[1]], [a, never[0], never[2], never[3]], [never[4], never[5], never[6], never[7], never[8]],
            [never[9], never[10], never[11], never[12], never[13], never[14]]]


def _cyclic():
    """Two states, 16 allowed ids each, no terminal: even-numbered edges stay, odd ones cross."""
    a, b = list(range(100, 116)), list(range(200, 216))
    return TokenAutomaton(2, 0, (0, 0), (0, 16, 32), a + b, [i % 2 for i in range(16)] + [(i + 1) % 2 for i in range(16)])


def _guided(engine, req, aut, params, **kw):
    got = engine.generate_guided([(*req, None)], [aut], params, **kw)
    return (got[0][0], got[2][0], *got[3:])


def test_engine_greedy_trie(engine, pages, oracle, plain):
    ids, mask, page = pages[0]
    choices = _trie(plain)
    aut = automaton_from_sequences(choices)
    p = DecodeParameters(max_new_tokens=24)
    assert plain == oracle.generate(ids, mask, 24)
    got, (state, status) = _guided(engine, pages[0], aut, p)
    assert got == oracle.generate(ids, mask, 24, aut=aut)
    assert got != plain[:len(got)] and got in choices and status == 1
    assert (state, status) == aut.walk(got)


def test_engine_sampled_trie(engine, pages, oracle, plain):
    ids, mask, page = pages[0]
    aut = automaton_from_sequences(_trie(plain))
    kw = dict(do_sample=True, temperature=0.8, top_p=0.9, seed=11)
    got, (state, status) = _guided(engine, pages[0], aut, DecodeParameters(max_new_tokens=24, **kw))
    assert got == oracle.generate(ids, mask, 24, aut=aut, **kw)
    assert (state, status) == aut.walk(got) and status == 1


def test_engine_cyclic_under_ngram_ban(engine, pages, oracle):
    ids, mask, page = pages[0]
    aut = _cyclic()
    got, (state, status) = _guided(engine, pages[0], aut, DecodeParameters(max_new_tokens=24, no_repeat_ngram_size=3))
    assert got == oracle.generate(ids, mask, 24, aut=aut, no_repeat_ngram_size=3)
    assert len(got) == 24 and set(got) <= set(aut.edge_tok) and status == 0 and (state, status) == aut.walk(got)


def _lp_ref(l, K):
    """float64 log-softmax of one row over its finite entries: (lp [V], the K best ids, the bound's scale)."""
    fin = np.isfinite(l)
    l64 = l.astype(np.float64)
    m = l64[fin].max()
    lp = np.where(fin, l64 - m - np.log(np.sum(np.exp(l64[fin] - m))), -np.inf)
    order = np.argsort(-np.where(fin, l64, -np.inf), kind="stable")[:K]
    return lp, order, max(1.0, float(np.abs(l64[fin] - m).max()))


def test_engine_logprobs_and_mixed_batch(engine, pages):
    """Pages {1 guided by the cyclic automaton, 0 not} with K = 5 alternatives.  The guided page's step-0 entry and
    alternatives equal NumPy's log-softmax of the traced unconstrained logits masked by the start state, at
    tests/test_logit_bias.py's bound.  The unguided page's ids equal its run alone, and its ids and entries are
    bit-equal to the same two pages decoded without any automaton: the kernels touch nothing of a row whose flag is 0.
    (Against the one-page run the entries are not bit-equal with the feature off either: the lm_head of a two-page
    batch rounds differently from the one-page one.  The test prints that difference, 9.5e-7 on an MI355X in both
    cases, which is the engine's and not this feature's.)"""
    K = 5
    p = DecodeParameters(max_new_tokens=8)
    aut = _cyclic()
    _, logits = engine.generate_trace([(*pages[1], None)], p)
    l0 = np.where(aut.mask_row(0, engine.vocab, EOS), logits[0][0], np.float32(-np.inf)).astype(np.float32)
    reqs = [(*pages[1], None), (*pages[0], None)]
    ids, _, gres, lp, ti, tl = engine.generate_guided(reqs, [aut, None], p, top_k=K)
    alone = engine.generate_logprobs([reqs[1]], K, p)
    both = engine.generate_logprobs(reqs, K, p)
    d_off = np.abs(np.asarray(both[1][1], np.float64) - np.asarray(alone[1][0], np.float64)).max()
    d_on = np.abs(np.asarray(lp[1], np.float64) - np.asarray(alone[1][0], np.float64)).max()
    print(f"unguided page, entries against its one-page run: feature off (two pages, no automaton) max |diff| {d_off:.3e}, "
          f"beside a guided page {d_on:.3e}")
    assert ids[1] == alone[0][0] == both[0][1] and gres[1] == (0, 0)
    for a, b in zip((lp[1], ti[1], tl[1]), (both[1][1], both[2][1], both[3][1])):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    assert set(ids[0]) <= set(aut.edge_tok) and set(int(t) for t in np.asarray(ti[0]).reshape(-1)) <= set(aut.edge_tok)
    ref, order, scale = _lp_ref(l0, K)
    tol = LP_C * EPS * scale
    err0, errk = abs(lp[0][0] - ref[ids[0][0]]), np.abs(np.asarray(tl[0][0]) - ref[order]).max()
    print(f"guided step-0 entry: |err| {err0:.3e}, alternatives {errk:.3e}, bound {tol:.3e}")
    assert np.array_equal(np.asarray(ti[0][0]), order)
    assert err0 <= tol and errk <= tol


def _einval(fn, *a, **kw):
    with pytest.raises(DsocrError) as ei:
        fn(*a, **kw)
    assert ei.value.status == 1, ei.value


def test_engine_refuses(engine, pages, plain, monkeypatch):
    aut = _cyclic()
    req = [(*pages[0], None)]
    _einval(engine.generate_guided, req, [aut], DecodeParameters(max_new_tokens=4, use_cache=False))
    monkeypatch.setenv("DSOCR_PERSIST", "1")
    _einval(engine.generate_guided, req, [aut], DecodeParameters(max_new_tokens=4))
    monkeypatch.delenv("DSOCR_PERSIST")
    # the EOS rule is the engine's own check (the Python side does not know the request's EOS id)
    _einval(engine.generate_guided, req, [TokenAutomaton(2, 0, (0, 1), (0, 1, 1), (EOS,), (1,))], DecodeParameters(max_new_tokens=4))
    # ... and every rule through the C call: the Python check is taken out of the way, so the record reaches
    # dsocr_generate_guided as it is
    import dsocr.engine as de
    from test_guided_host import RULES, _ok
    monkeypatch.setattr(de, "_guided", lambda a, vocab: a)
    for rule, change in sorted(RULES.items()):
        bad = TokenAutomaton(**dict(_ok(), **change))
        with pytest.raises(DsocrError) as ei:
            engine.generate_guided(req, [bad], DecodeParameters(max_new_tokens=4))
        assert ei.value.status == 1 and "token automaton" in str(ei.value), rule
    monkeypatch.undo()
    assert engine.generate(*pages[0], None, DecodeParameters(max_new_tokens=24)) == plain


# ------------------------------------------------------------------ decode sessions
def test_session_admission_forms(engine, pages, plain):
    """The same guided request through admit, admit_prefix and admit_begin (the prompt in 2 chunks): the same ids,
    first token included, and the final state.  A cancelled chunked admission leaves no automaton behind, and a
    staged automaton is consumed by one admission."""
    ids, mask, page = pages[0]
    aut = automaton_from_sequences(_trie(plain))
    p = DecodeParameters(max_new_tokens=10)
    want, wres = _guided(engine, pages[0], aut, p)
    plain1 = engine.generate(*pages[1], None, p)
    rows = max(i for i, m in enumerate(mask) if m) + 1
    chunk = max(32, (len(ids) + 1) // 2)
    got, res = {}, {}
    with engine.open_session(2, len(ids) + 11 + 8, p, guided=True) as sess:
        assert sess.info()["flags"] == SESSION_GUIDED
        assert sess.admit(ids, mask, page, max_new_tokens=10, guided=aut) == 0
        handle = sess.keep_prefix(0, rows)
        sess.step(8)
        sess.step(8)
        assert sess.head_steps()["screened"] == 0
        res["admit"] = sess.guided_state(0)
        got["admit"], _ = sess.retire(0)
        assert sess.admit_prefix(handle, ids, mask, max_new_tokens=10, guided=aut) == 0
        sess.step(8)
        sess.step(8)
        res["prefix"] = sess.guided_state(0)
        got["prefix"], _ = sess.retire(0)
        sess.admit_begin(ids, mask, page, chunk_rows=chunk, max_new_tokens=10, guided=aut)
        sess.admit_advance()
        sess.admit_cancel()
        # the next page carries none: the staged automaton was consumed by the cancelled admission
        assert sess.admit(*pages[1], max_new_tokens=10) == 0
        sess.step(8)
        sess.step(8)
        assert sess.guided_state(0) == (0, 0)
        got["after_cancel"], _ = sess.retire(0)
        sess.admit_begin(ids, mask, page, chunk_rows=chunk, max_new_tokens=10, guided=aut)
        done = False
        while not done:
            done, slot = sess.admit_advance()
        sess.step(8)
        sess.step(8)
        res["chunked"] = sess.guided_state(slot)
        got["chunked"], _ = sess.retire(slot)
    assert got["admit"] == got["prefix"] == got["chunked"] == want
    assert res["admit"] == res["prefix"] == res["chunked"] == wres and wres[1] == 1
    assert got["after_cancel"] == plain1


def test_all_controls_agree_across_entry_points(engine, pages):
    """Page 0 under all five controls at once (deny / bias list, stop set, frequency / presence penalties, windowed
    2-gram ban, the cyclic automaton) with K = 2 log-probability alternatives: generate_guided alone, a session opened
    with every feature through admit, and the same session through admit_begin / admit_advance (the page is staged in
    slot 1 and moves to slot 0) give the same ids, stop hit, automaton (state, status) and log-probability entries,
    bit for bit (the page runs alone, at n = 1, every time).  The chunked admission takes the prompt as one chunk:
    in two, the chunk attention rounds the cache rows differently from the one-pass prefill and entry 3 moves by one
    ulp, with or without controls (ids, hit and state still agree).  Then two pages: slot 0 retires mid-run, the controlled
    page moves into it with every record and finishes with the same ids.  The stop is the run's own 2-gram at
    positions 5, 6 (the windowed ban makes that its first occurrence), so it fires at 7 tokens, after the move."""
    ids, mask, page = pages[0]
    K, M = 2, 12
    aut = _cyclic()
    con = merge_constraint(logit_bias={101: 1.5, 203: -1.0}, banned_token_ids=[100, 200])
    pen, win = Penalties(0.8, 0.4, 0.0), NgramWindow(2, 6)
    p = DecodeParameters(max_new_tokens=M)

    def alone(ss):
        got = engine.generate_guided([(ids, mask, page, None)], [aut], p, top_k=K, constraints=[con], stop_sets=[ss],
                                     penalties=[pen], ngram_windows=[win])
        return [g[0] for g in got]

    base = alone(None)[0]
    assert len(base) == M and set(base) <= set(aut.edge_tok) - {100, 200}
    ss = StopSet(((base[5], base[6]), (7, 8, 9)), (0, 1), ())
    want = alone(ss)
    assert want[0] == base[:7] and want[1] == (0, 2) and want[2] == aut.walk(base[:7])
    kw = dict(params=p, logprobs=K, stops=ss, frequency_penalty=pen.frequency, presence_penalty=pen.presence,
              min_p=pen.min_p, ngram_window=win, guided=aut, **con.kwargs())
    need = max(len(pages[i][0]) for i in (0, 1)) + M + 1 + 8
    got = {}

    def finish(sess, key, slot):
        st = sess.step(8)
        sess.step(8)
        assert st[slot].done and st[slot].out_len == 7
        got[key] = [None, sess.stop_hit(slot), sess.guided_state(slot), *sess.logprobs(slot, 0, 7, K)]
        got[key][0] = sess.retire(slot)[0]

    with engine.open_session(2, need, p, per_request=True, logprobs=True, logit_bias=True, stops=True, penalties=True,
                             ngram_window=True, guided=True) as sess:
        assert sess.admit(ids, mask, page, **kw) == 0
        finish(sess, "admit", 0)
        sess.admit_begin(ids, mask, page, chunk_rows=max(32, len(ids)), **kw)
        done = False
        while not done:
            done, slot = sess.admit_advance()
        assert slot == 0
        finish(sess, "chunked", 0)
        # two pages: the plain one (3 tokens) leaves first and the controlled page moves from slot 1 to slot 0
        assert sess.admit(*pages[1], params=DecodeParameters(max_new_tokens=3)) == 0
        assert sess.admit(ids, mask, page, **kw) == 1
        assert sess.step(3)[0].done
        assert sess.retire(0)[1] == 1
        sess.step(8)
        moved = [sess.stop_hit(0), sess.guided_state(0)]
        moved.insert(0, sess.retire(0)[0])
    for key in ("admit", "chunked"):
        assert got[key][:3] == want[:3], key
        for a, b in zip(got[key][3:], want[3:]):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), key
    assert moved == want[:3]


def test_session_compaction(engine, pages):
    """Three pages {plain, plain, guided by the cyclic automaton}; slot 0 finishes first and the guided page moves
    into it in the middle of its run: its ids equal the single-page run, and so do the others'."""
    aut = _cyclic()
    P = lambda m: DecodeParameters(max_new_tokens=m, no_repeat_ngram_size=3)
    max_new = {0: 6, 1: 20, 2: 20}
    single = {i: engine.generate(*pages[i], None, P(m)) for i, m in list(max_new.items())[:2]}
    single[2], sres = _guided(engine, pages[2], aut, P(20))
    need = max(len(pages[i][0]) + m + 1 for i, m in max_new.items())
    with engine.open_session(3, need + 8, P(20), per_request=True, guided=True) as sess:
        assert sess.admit(*pages[0], params=P(6)) == 0
        assert sess.admit(*pages[1], params=P(20)) == 1
        assert sess.admit(*pages[2], params=P(20), guided=aut) == 2
        st = sess.step(6)
        assert st[0].done
        ids0, moved = sess.retire(0)
        assert moved == 2
        sess.step(8)
        sess.step(8)
        assert all(s.done for s in sess.poll())
        assert sess.guided_state(0) == sres and sess.guided_state(1) == (0, 0)
        ids1, _ = sess.retire(1)
        ids2, _ = sess.retire(0)
    assert ids0 == single[0] and ids1 == single[1] and ids2 == single[2]
    assert set(ids2) <= set(aut.edge_tok) and len(ids2) == 20


def test_session_without_flag_and_feature_off(engine, pages, oracle, plain):
    """Staging without the flag is EINVAL; with the feature unused a generate and a session give the oracle's ids,
    the plain run's step count, the screened head and a clear flag bit."""
    ids, mask, page = pages[0]
    p = DecodeParameters(max_new_tokens=24)
    assert engine.generate(ids, mask, page, None, p) == plain
    steps = engine.last_timings()["decode_steps"]
    _guided(engine, pages[0], _cyclic(), p)
    assert engine.generate(ids, mask, page, None, p) == plain and engine.last_timings()["decode_steps"] == steps
    got = engine.generate_guided([(ids, mask, page, None)], [None], p)
    assert got[0][0] == plain and got[2][0] == (0, 0)
    keep = []
    rec = _guided_c(_cyclic(), keep)
    with engine.open_session(2, len(ids) + 25, p) as sess:
        assert sess.info()["flags"] & SESSION_GUIDED == 0
        _einval(sess.admit, ids, mask, page, max_new_tokens=24, guided=_cyclic())
        assert lib().dsocr_session_stage_guided(engine._h, C.byref(rec)) == 1
        assert sess.info()["active"] == 0
        sess.admit(ids, mask, page, max_new_tokens=24)
        for _ in range(3):
            sess.step(8)
        assert sess.head_steps()["exact"] == 0
        assert sess.retire(0)[0] == plain
    assert plain == oracle.generate(ids, mask, 24)


def test_scheduler_shares_the_session(engine, pages, plain):
    """``BatchScheduler(guided=True)``: a guided and a plain request share the running session; the guided page's
    ids and status equal its run alone, the plain one's today's decode.  Without the flag the guided request runs
    exclusively, with the same result."""
    from dsocr.scheduler import BatchScheduler
    tok = SyntheticTokenizer(512)
    aut = automaton_from_sequences(_trie(plain))
    p = DecodeParameters(max_new_tokens=10)
    want, wres = _guided(engine, pages[0], aut, p)
    plain1 = engine.generate(*pages[1], None, p)
    need = max(len(pages[i][0]) for i in (0, 1)) + 11 + 8
    with BatchScheduler(engine, tok, 2, need, p, TINY_VS, guided=True) as s:
        f1 = s.submit(PROMPT, [_img(101, *SIZES[1])])
        f0 = s.submit(PROMPT, [_img(100, *SIZES[0])], guided=aut)
        o0, o1 = f0.result(timeout=60), f1.result(timeout=60)
        assert s.exclusive_runs == 0
    assert [int(t) for t in o0.generated_tokens] == want and o0.guided_status == "complete" and wres[1] == 1
    assert [int(t) for t in o1.generated_tokens] == plain1 and o1.guided_status is None
    with BatchScheduler(engine, tok, 2, need, p, TINY_VS) as s:
        o0 = s.submit(PROMPT, [_img(100, *SIZES[0])], guided=aut).result(timeout=60)
        assert s.exclusive_runs == 1
    assert [int(t) for t in o0.generated_tokens] == want and o0.guided_status == "complete"
