"""Frequency / presence penalties and min-p on the GPU.

The penalty kernel through its hook against ``dsocr.penalties.apply`` (NumPy f32, bit for bit: one multiply, one add
and one subtract, each rounded); the sampler through its hook, and the engine, against the CPU oracle, whose
``select_token_id`` is restated here with the two new steps in their places (repetition penalty, then frequency /
presence over the generated ids, then the n-gram ban; min-p on ``logit / T`` before top-k: nothing under ``oracle/``
changes); decode sessions against the same page decoded alone.  Tiny config, the pages and prompt of
tests/test_session.py.
"""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import dsocr
from dsocr import DecodeParameters, DsocrError, ModelLoadArgs, Page, VisionSettings, build_prompt_tokens, load_model
from dsocr._lib import SESSION_PENALTIES, SESSION_PER_REQUEST, PenaltiesC, check, lib
from dsocr.constraint import merge_constraint
from dsocr.penalties import Penalties, apply, ln_min_p, min_p_keep
from dsocr.synth import SyntheticTokenizer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, "deepseek-ocr.rs_amd", "dsocr", "configs", "tiny.json")
TINY_VS = VisionSettings(256, 128, True)
SEED = 7
PROMPT = "<image>\nConvert the document to markdown."
SIZES = [(300, 420), (256, 256), (500, 140)]
SENTINEL = np.float32(-12345.5)
STEPS = 20
# the engine cases' records; the values are chosen on the CPU oracle so that its penalised ids differ from its plain
# ids on page 0 within STEPS tokens (every test asserts that on the oracle before it looks at the engine)
FREQ = Penalties(0.8, 0.4, 0.0)
MINP = Penalties(0.0, 0.0, 0.1)
# (the tiny model's logits span about 1.5: at temperature 0.2 ln(0.1) = -2.3 cuts into them, at 1.0 it would not)
MINP_KW = dict(do_sample=True, temperature=0.2, seed=11)
# a record small enough that the page still repeats ids (on the oracle: 204, 348, 322 in a loop up to step 16): the
# emitted ids whose logits the penalty kernel has rewritten, for the log-probability entries
REP = Penalties(0.01, 0.01, 0.0)
# test_logprobs.py's bound for a log-probability against float64 NumPy: LP_C * 2**-23 * max(1, max|l - m|)
LP_C, EPS = 32.3, 2.0 ** -23


# ------------------------------------------------------------------ select_token_id with the two steps added
def select_with_penalties(logits, context, n_prompt, pen, repetition_penalty=1.0, no_repeat_ngram_size=None,
                          do_sample=False, temperature=0.0, top_k=None, top_p=None, rng=None):
    """oracle.decoder.select_token_id restated, with DESIGN 4.19's steps: the generated ids are context[n_prompt:]."""
    from oracle.decoder import argmax_first, banned_ngram_tokens
    from oracle.sampling import apply_top_k, apply_top_p, sample_from_logits
    logits = np.asarray(logits, np.float32)
    adjusted = logits.copy()
    if repetition_penalty > 0.0 and abs(repetition_penalty - 1.0) > np.finfo(np.float32).eps:
        rp = np.float32(repetition_penalty)
        for t in dict.fromkeys(int(c) for c in context):
            if 0 <= t < len(adjusted):
                adjusted[t] = adjusted[t] / rp if adjusted[t] > 0 else adjusted[t] * rp
    adjusted = apply(adjusted, context[n_prompt:], pen.frequency, pen.presence)
    filtered = adjusted.copy()
    if no_repeat_ngram_size is not None and no_repeat_ngram_size > 1:
        for t in banned_ngram_tokens([int(c) for c in context], no_repeat_ngram_size):
            if 0 <= t < len(filtered):
                filtered[t] = -np.inf
    if not np.any(np.isfinite(filtered)):
        filtered = adjusted
    if do_sample and temperature > 0.0:
        lg = [float(v) / temperature for v in filtered]
        fin = [i for i, v in enumerate(lg) if math.isfinite(v)]
        if fin and pen.min_p > 0:
            keep = min_p_keep([lg[i] for i in fin], ln_min_p(pen.min_p))
            for i, k in zip(fin, keep):
                if not k:
                    lg[i] = -math.inf
        if top_k is not None and 0 < top_k < len(lg):
            apply_top_k(lg, top_k)
        if top_p is not None and 0.0 <= top_p < 1.0:
            apply_top_p(lg, top_p)
        tok = sample_from_logits(lg, rng)
        if tok is not None:
            return tok
    for arr in (filtered, adjusted, logits):
        idx = argmax_first(arr)
        if idx is not None:
            return idx
    return 0


# ------------------------------------------------------------------ the penalty kernel through its hook
@pytest.mark.parametrize("recs", [[(0.5, 0.25), (0.0, 0.0), (0.7, 0.0)], [(0.0, 0.0), (0.0, -1.5), (0.7, -0.375)]],
                         ids=["frequency_only", "negative_presence"])
@pytest.mark.parametrize("V,ld", [(1003, 1008), (4104, 4104)])
def test_penalty_kernel_hook(gpu, V, ld, recs):
    """One call of the hook: B = 3, out_cap = 640, out_len = [0, 1, 600], one (frequency, presence) per row; one row's
    record is off in either set and its bytes must be unchanged.  Row 2 holds one id at positions 3 and 590 (first
    occurrence and repeat in different blocks and grid strides: 128 positions per block, 3 blocks), ids 0 and V - 1,
    an id seven times, an id whose logit is -inf, and ids outside [0, V), which are skipped.  (0.7 * 7 is inexact in
    f32, so with a presence beside it a fused multiply-add would show in the last bit.)"""
    B, cap = 3, 640
    r = np.random.default_rng(V)
    x = np.full((B, ld), SENTINEL, np.float32)
    x[:, :V] = (r.standard_normal((B, V)) * 4).astype(np.float32)
    out = r.integers(1, V - 1, (B, cap)).astype(np.int32)
    lens = np.array([0, 1, 600], np.int32)
    twice, seven, ninf = 17, 23, 31
    row = out[2]
    row[np.isin(row, (twice, seven, ninf, 0, V - 1))] = 40
    row[3] = row[590] = twice
    row[[5, 130, 131, 257, 400, 511, 599]] = seven
    row[10], row[300], row[200], row[201] = 0, V - 1, ninf, ninf
    row[50], row[51] = -1, V
    row[600:] = seven                      # behind out_len: never counted
    x[2, ninf] = -np.inf
    got = x.copy()
    pen = (PenaltiesC * B)(*[PenaltiesC(f, p, 0.0) for f, p in recs])
    check(lib().dsocr_k_out_penalty(B, V, ld, got.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), cap,
                                    lens.ctypes.data_as(C.c_void_p), pen))
    assert got[0].tobytes() == x[0].tobytes()                  # out_len 0 (and, in the second set, the record off)
    assert np.all(got[:, V:] == SENTINEL)                      # columns [V, ld) are not written
    for b in (1, 2):
        f, p = recs[b]
        if f == 0 and p == 0:
            assert got[b].tobytes() == x[b].tobytes()          # record off: the row's bytes
        else:                                                  # NumPy f32, bit for bit
            assert got[b, :V].tobytes() == apply(x[b, :V], out[b, :lens[b]], f, p).tobytes()
    f, p = np.float32(recs[2][0]), np.float32(recs[2][1])
    assert got[2, ninf] == -np.inf
    assert got[2, seven] == np.float32(x[2, seven] - np.float32(np.float32(f * np.float32(7)) + p))
    assert got[2, twice] == np.float32(x[2, twice] - np.float32(np.float32(f * np.float32(2)) + p))
    assert got[2, 0] != x[2, 0] and got[2, V - 1] != x[2, V - 1]
    if recs[1][1] < 0:                                         # a negative presence raises the one generated id
        assert got[1, out[1, 0]] == np.float32(x[1, out[1, 0]] + np.float32(1.5))


def test_penalty_kernel_rows_longer_than_a_tile(gpu):
    """out_cap = 2600: rows of 2500 ids (two LDS tiles of 2048, staged per grid-stride iteration) and of exactly 2048
    (one tile, staged once), ids from a small range so that every id repeats, one id at positions 5 and 2100 (first
    occurrence and repeat in different tiles)."""
    B, V, ld, cap = 2, 1003, 1008, 2600
    r = np.random.default_rng(5)
    x = np.full((B, ld), SENTINEL, np.float32)
    x[:, :V] = (r.standard_normal((B, V)) * 4).astype(np.float32)
    out = r.integers(0, 300, (B, cap)).astype(np.int32)
    out[0][out[0] == 777] = 1
    out[0, 5] = out[0, 2100] = 777
    lens = np.array([2500, 2048], np.int32)
    recs = [(0.3, 0.125), (0.2, -0.5)]
    got = x.copy()
    pen = (PenaltiesC * B)(*[PenaltiesC(f, p, 0.0) for f, p in recs])
    check(lib().dsocr_k_out_penalty(B, V, ld, got.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), cap,
                                    lens.ctypes.data_as(C.c_void_p), pen))
    for b in range(B):
        assert got[b, :V].tobytes() == apply(x[b, :V], out[b, :lens[b]], *recs[b]).tobytes()
    assert np.all(got[:, V:] == SENTINEL)
    assert got[0, 777] == np.float32(x[0, 777] - np.float32(np.float32(np.float32(0.3) * np.float32(2)) + np.float32(0.125)))


# ------------------------------------------------------------------ the sampler through its hook
SV, ST, SDRAWS, SSEED, SCAP = 1003, 0.7, 8, 4321, 64


@pytest.fixture(scope="module")
def sampler_rows():
    """Two rows of V = 1003 logits (a -inf, a NaN, ties of the maximum in row 1) and a context whose last token has
    been followed by each row's maximum: under no_repeat_ngram_size = 2 the maximum is banned."""
    r = np.random.default_rng(99)
    logits = (r.standard_normal((2, SV)) * 3).astype(np.float32)
    logits[0, 5] = -np.inf
    logits[1, 7] = np.nan
    logits[1, 100:103] = np.nanmax(logits[1]) + np.float32(0.5)  # three tied maxima
    top = [int(np.nanargmax(logits[b])) for b in range(2)]
    ctx = np.zeros((2, SCAP), np.int32)
    lens = np.array([9, 9], np.int32)
    for b in range(2):
        ctx[b, :9] = [3, 4, 900, top[b], 8, 9, 10, 11, 900]  # (900, top) occurred: top is banned behind 900
    return logits, ctx, lens, top


def _oracle_draws(logits, ctx, ngram, k, p, mp):
    from oracle.sampling import StdRng
    rng = StdRng(SSEED)
    return [select_with_penalties(logits, ctx, len(ctx), Penalties(0.0, 0.0, mp), 1.0, ngram if ngram > 1 else None,
                                  do_sample=True, temperature=ST, top_k=k if k else None,
                                  top_p=p if 0.0 <= p < 1.0 else None, rng=rng) for _ in range(SDRAWS)]


def _k_min_p(rows, ngram, k, p, mp):
    from _dev import Dev
    logits, ctx, lens, _ = rows
    dl, dc, dn = Dev(logits), Dev(ctx), Dev(lens)
    dt = Dev.zeros(SDRAWS * 2, np.int32)
    ln = np.full(2, ln_min_p(mp), np.float64)
    check(lib().dsocr_k_sample_stoch_min_p(2, SV, dl.ptr, dc.ptr, SCAP, dn.ptr, ngram, 1.0, ST, k, p,
                                           ln.ctypes.data_as(C.c_void_p), SSEED, SDRAWS, dt.ptr))
    return dt.get().reshape(SDRAWS, 2)


def test_sampler_min_p_zero_is_todays(gpu, sampler_rows):
    """ln_min_p = -inf: draw for draw the ids of dsocr_k_sample_stoch, in every mode."""
    from _dev import Dev
    logits, ctx, lens, _ = sampler_rows
    for ngram, k, p in [(0, 0, -1.0), (0, 5, -1.0), (0, 0, 0.9), (2, 0, -1.0)]:
        dl, dc, dn = Dev(logits), Dev(ctx), Dev(lens)
        dt = Dev.zeros(SDRAWS * 2, np.int32)
        check(lib().dsocr_k_sample_stoch(2, SV, dl.ptr, dc.ptr, SCAP, dn.ptr, ngram, 1.0, ST, k, p, SSEED, SDRAWS, dt.ptr))
        assert _k_min_p(sampler_rows, ngram, k, p, 0.0).tolist() == dt.get().reshape(SDRAWS, 2).tolist()


@pytest.mark.parametrize("mp", [0.05, 1.0])
@pytest.mark.parametrize("ngram,k,p", [(0, 0, -1.0), (0, 5, -1.0), (0, 0, 0.9), (2, 0, -1.0)],
                         ids=["alone", "top_k5", "top_p0.9", "ngram_bans_max"])
def test_sampler_min_p_matches_oracle(gpu, sampler_rows, mp, ngram, k, p):
    logits, ctx, lens, top = sampler_rows
    got = _k_min_p(sampler_rows, ngram, k, p, mp)
    for b in range(2):
        ref = _oracle_draws(logits[b], ctx[b, :lens[b]].tolist(), ngram, k, p, mp)
        assert got[:, b].tolist() == ref, (b, got[:, b].tolist(), ref)
        if ngram:  # qmax comes from the unbanned set: the banned maximum is never drawn, its runner-ups are
            assert top[b] not in ref
        if mp == 1.0 and not ngram:  # exactly the ties of the maximum
            assert set(ref) <= ({100, 101, 102} if b == 1 else {top[0]})


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
    """The CPU oracle on page 0 with ``oracle.model.select_token_id`` replaced per call by the restatement above
    (plus an optional dense logit bias in front of it).  Runs are cached: a reference is computed once."""

    def __init__(self):
        import oracle.model as om
        from oracle.weights import Weights
        self.om = om
        self.model = om.OracleModel(json.load(open(TINY)), Weights(seed=SEED, dtype="f16"))
        self.emb, _ = self.model.image_embeddings(_img(100, *SIZES[0]), 256, 128, True)
        self.cache = {}

    def generate(self, ids, mask, max_new, pen=None, dense=None, **kw):
        key = (max_new, pen, None if dense is None else dense.tobytes(), tuple(sorted(kw.items())))
        if key in self.cache:
            return self.cache[key]
        om, real, n_prompt = self.om, self.om.select_token_id, len(ids)
        pn = pen or Penalties()

        def select(logits, context, repetition_penalty=1.0, no_repeat_ngram_size=None, **sel):
            l = np.asarray(logits, np.float32)
            if dense is not None:
                l = l + dense
            return select_with_penalties(l, context, n_prompt, pn, repetition_penalty, no_repeat_ngram_size, **sel)

        om.select_token_id = select
        try:
            out, _ = self.model.generate(ids, mask, self.emb, max_new, eos_token_id=1, **kw)
        finally:
            om.select_token_id = real
        self.cache[key] = [int(t) for t in out]
        return self.cache[key]


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def _penalised(engine, req, pen, params, **kw):
    return engine.generate_penalties([(*req, None)], [pen], params, **kw)[0][0]


def test_oracle_restatement_is_the_oracle(oracle, pages):
    """With every record off the restated select_token_id gives the oracle's own ids, greedy and sampled."""
    import oracle.model as om
    ids, mask, _ = pages[0]
    for kw in ({}, dict(repetition_penalty=1.3, no_repeat_ngram_size=3), dict(top_p=0.9, **MINP_KW)):
        real, _ = oracle.model.generate(ids, mask, oracle.emb, 12, eos_token_id=1, **kw)
        assert oracle.generate(ids, mask, 12, **kw) == [int(t) for t in real]
    assert om.select_token_id.__module__ == "oracle.decoder"


def test_engine_greedy(engine, pages, oracle):
    ids, mask, page = pages[0]
    p = DecodeParameters(max_new_tokens=STEPS)
    plain, want = oracle.generate(ids, mask, STEPS), oracle.generate(ids, mask, STEPS, FREQ)
    assert want != plain, "the record changes nothing on this page: pick another"
    assert engine.generate(ids, mask, page, None, p) == plain
    assert _penalised(engine, pages[0], FREQ, p) == want


def test_engine_greedy_with_repetition_penalty_and_ngram(engine, pages, oracle):
    ids, mask, page = pages[0]
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=3)
    plain, want = oracle.generate(ids, mask, STEPS, **kw), oracle.generate(ids, mask, STEPS, FREQ, **kw)
    assert want != plain, "the record changes nothing on this page: pick another"
    assert _penalised(engine, pages[0], FREQ, DecodeParameters(max_new_tokens=STEPS, **kw)) == want


def test_engine_sampled_min_p(engine, pages, oracle):
    ids, mask, page = pages[0]
    plain, want = oracle.generate(ids, mask, STEPS, **MINP_KW), oracle.generate(ids, mask, STEPS, MINP, **MINP_KW)
    assert want != plain, "min_p changes nothing under this seed: pick another"
    assert _penalised(engine, pages[0], MINP, DecodeParameters(max_new_tokens=STEPS, **MINP_KW)) == want
    # a greedy row ignores min_p
    assert _penalised(engine, pages[0], MINP, DecodeParameters(max_new_tokens=STEPS)) == oracle.generate(ids, mask, STEPS)


def test_engine_with_bias_and_logprobs(engine, pages, oracle):
    """Penalties with a logit bias and log-probabilities: the ids are the oracle's, and the entries are those of the
    bias-constrained distribution, which the penalties do not enter: bit for bit the entries of the same ids' steps
    where the unpenalised run emitted the same prefix."""
    ids, mask, page = pages[0]
    plain = oracle.generate(ids, mask, STEPS)
    con = merge_constraint(banned_token_ids=list(dict.fromkeys(plain))[:2], vocab=engine.vocab)
    dense = con.dense(engine.vocab)
    base, want = oracle.generate(ids, mask, STEPS, dense=dense), oracle.generate(ids, mask, STEPS, FREQ, dense=dense)
    assert want != base, "the record changes nothing under this constraint: pick another"
    p = DecodeParameters(max_new_tokens=STEPS)
    got, _, lp, ti, tl = engine.generate_penalties([(*pages[0], None)], [FREQ], p, top_k=5, constraints=[con])
    assert got[0] == want
    g0, lp0, ti0, tl0 = engine.generate_constrained([(*pages[0], None)], [con], p, top_k=5)
    assert g0[0] == base
    same = next(i for i in range(STEPS) if want[i] != base[i])  # steps [0, same] saw the same prefix: the same logits
    assert same > 0
    assert np.asarray(ti[0][:same + 1]).tobytes() == np.asarray(ti0[0][:same + 1]).tobytes()
    assert np.asarray(tl[0][:same + 1]).tobytes() == np.asarray(tl0[0][:same + 1]).tobytes()
    assert np.asarray(lp[0][:same]).tobytes() == np.asarray(lp0[0][:same]).tobytes()
    assert not set(con.ids) & set(got[0])


def _check_repeat_entries(ids, lp, ti, tl, raw, n_raw):
    """Entries of a page whose record rewrote logits at repeated ids: every emitted id that is among its step's 20
    alternatives has exactly that alternative's log-probability (both are l_raw - M - log S of the same row), at
    least one of them is a repeat, and the first n_raw entries equal float64 NumPy on the raw logits ``raw``."""
    repeats = 0
    for i, t in enumerate(ids):
        k = [j for j in range(len(ti[i])) if int(ti[i][j]) == t]
        if k:
            assert np.float32(lp[i]).tobytes() == np.float32(tl[i][k[0]]).tobytes(), (i, t, lp[i], tl[i][k[0]])
            repeats += t in ids[:i]
    assert repeats >= 3, "no emitted repeat among the alternatives: pick another record"
    for i in range(n_raw):
        l = np.asarray(raw[i], np.float32)
        fin = np.isfinite(l)
        l64 = l.astype(np.float64)
        m = l64[fin].max()
        want = l64[ids[i]] - m - np.log(np.sum(np.exp(l64[fin] - m)))
        tol = LP_C * EPS * max(1.0, float(np.abs(l64[fin] - m).max()))
        assert abs(float(lp[i]) - want) <= tol, (i, ids[i], float(lp[i]), want, tol)


def test_logprobs_of_repeated_ids(engine, pages, oracle):
    """Log-probabilities stay those of the unpenalised distribution where the penalty kernel has rewritten the emitted
    id's logit: repetition_penalty = 1, so only the frequency / presence penalty can have touched it.  Through
    generate_penalties, and through a session with fixed parameters (LOGPROBS | PENALTIES, not PER_REQUEST).  The raw
    logits come from the logits trace of the plain run, which emits the same ids up to the first difference."""
    ids, mask, page = pages[0]
    p = DecodeParameters(max_new_tokens=STEPS)
    plain, want = oracle.generate(ids, mask, STEPS), oracle.generate(ids, mask, STEPS, REP)
    same = next((i for i in range(STEPS) if want[i] != plain[i]), STEPS)   # steps [0, same] saw the same prefix
    assert want != plain and len(set(want[:same + 1])) < same + 1, "no repeat under this record: pick another"
    traced, logits = engine.generate_trace([(*pages[0], None)], p)
    assert traced[0] == plain
    raw = logits[0]
    n_raw = min(same + 1, STEPS)
    got, _, lp, ti, tl = engine.generate_penalties([(*pages[0], None)], [REP], p, top_k=20)
    assert got[0] == want
    _check_repeat_entries(want, lp[0], ti[0], tl[0], raw, n_raw)
    with engine.open_session(2, len(ids) + STEPS + 1 + 8, p, logprobs=True, penalties=True) as sess:
        assert not sess.info()["flags"] & SESSION_PER_REQUEST
        assert sess.admit(ids, mask, page, max_new_tokens=STEPS, **_pkw(REP)) == 0
        for _ in range(3):
            sess.step(8)
        slp, sti, stl = sess.logprobs(0, 0, STEPS, 20)
        assert sess.retire(0)[0] == want
    _check_repeat_entries(want, slp, sti, stl, raw, n_raw)


def _einval(fn, *a, **kw):
    with pytest.raises(DsocrError) as ei:
        fn(*a, **kw)
    assert ei.value.status == 1, ei.value


def test_engine_refuses(engine, pages, monkeypatch):
    p4 = DecodeParameters(max_new_tokens=4)
    _einval(_penalised, engine, pages[0], FREQ, DecodeParameters(max_new_tokens=4, use_cache=False))
    for bad in (Penalties(float("nan"), 0.0, 0.0), Penalties(0.0, float("inf"), 0.0), Penalties(0.0, 0.0, -0.1),
                Penalties(0.0, 0.0, 1.5), Penalties(0.0, 0.0, float("nan"))):
        _einval(_penalised, engine, pages[0], bad, p4)
    # the logits trace: the C form takes no record, so the engine's check is reached through the shared body only
    # with use_cache = 0 above; the persistent step is refused on its switch
    monkeypatch.setenv("DSOCR_PERSIST", "1")
    _einval(_penalised, engine, pages[0], FREQ, p4)
    monkeypatch.delenv("DSOCR_PERSIST")
    # nothing was left behind: the plain call still runs, and a record that is off is the plain call
    a = engine.generate(*pages[0], None, p4)
    assert len(a) == 4 and _penalised(engine, pages[0], None, p4) == a and _penalised(engine, pages[0], Penalties(), p4) == a


# ------------------------------------------------------------------ sessions
def _pkw(pen):
    return {} if pen is None else dict(frequency_penalty=pen.frequency, presence_penalty=pen.presence, min_p=pen.min_p)


def test_session_mixed_batch(engine, pages, oracle):
    """3 slots {plain, penalised greedy, sampled min_p}: every page equals its single-page run.  Slot 0 retires
    mid-run, so the sampled page moves into slot 0 with its record; then slot 0 again, so the penalised page moves.
    (The plain row against a session without the flag, bit for bit: the next test.)"""
    P = lambda m, **kw: DecodeParameters(max_new_tokens=m, **kw)
    prm = {0: P(6), 1: P(STEPS), 2: P(STEPS, **MINP_KW)}
    pen = {0: None, 1: FREQ, 2: MINP}
    single = {i: (engine.generate(*pages[i], None, prm[i]) if pen[i] is None else _penalised(engine, pages[i], pen[i], prm[i]))
              for i in prm}
    assert single[1] != engine.generate(*pages[1], None, prm[1])
    need = max(len(pages[i][0]) + prm[i].max_new_tokens + 1 for i in prm) + 8

    def run():
        with engine.open_session(3, need, P(STEPS), per_request=True, logprobs=True, penalties=True) as sess:
            assert sess.info()["flags"] & SESSION_PENALTIES
            assert sess.admit(*pages[0], params=prm[0]) == 0
            assert sess.admit(*pages[1], params=prm[1], **_pkw(pen[1])) == 1
            assert sess.admit(*pages[2], params=prm[2], **_pkw(pen[2])) == 2
            sess.step(8)
            ids0, moved = sess.retire(0)
            assert moved == 2
            sess.step(4)
            # compaction once more: the sampled page (slot 0) leaves early, the penalised page moves from 1 to 0
            part2, moved = sess.retire(0)
            assert moved == 1
            sess.step(8)
            sess.step(8)
            ids1, _ = sess.retire(0)
            return ids0, ids1, part2

    ids0, ids1, part2 = run()
    assert ids0 == single[0] and ids1 == single[1]
    assert part2 == single[2][:len(part2)] and len(part2) >= 12


def test_session_plain_row_is_bit_for_bit(engine, pages):
    """The plain row of a batch whose other rows carry records, against a session without the flag: ids and
    log-probability entries bit for bit.  A row's last bits depend on what the other rows of the batch emit, feature
    or no feature: without the flag, row 0's third token_lp entry is -5.6640034 or -5.6640043 depending on the seed
    of a sampled row 2 (moe_down_grp_kernel cuts its K axis by the batch's number of distinct experts).
    So the other two rows carry records that are on and provably change no id: a
    frequency of 1e-30 (l - 1e-30 * c == l in f32 for every logit of this model) and min_p = 1e-300 (ln = -690.8,
    far below (min - max) / T of a logits row that spans about 1.5).  The exact head, the penalty launch's
    read-modify-write and the sampler's min-p pass all run; only row 0's isolation is left to show."""
    P = lambda m, **kw: DecodeParameters(max_new_tokens=m, **kw)
    prm = {0: P(6), 1: P(STEPS), 2: P(STEPS, **MINP_KW)}
    pen = {0: None, 1: Penalties(1e-30, 0.0, 0.0), 2: Penalties(0.0, 0.0, 1e-300)}
    need = max(len(pages[i][0]) + prm[i].max_new_tokens + 1 for i in prm) + 8

    def run(flag):
        kw = {"penalties": True} if flag else {}
        with engine.open_session(3, need, P(STEPS), per_request=True, logprobs=True, **kw) as sess:
            for i in range(3):
                sess.admit(*pages[i], params=prm[i], **(_pkw(pen[i]) if flag else {}))
            sess.step(8)
            lp = [sess.logprobs(i, 0, 6, 5) for i in range(3)]
            ids = [sess.retire(i)[0] for i in (2, 1, 0)][::-1]
        return ids, lp

    ids_f, lp_f = run(True)
    ids_p, lp_p = run(False)
    assert ids_f == ids_p                       # (the records change no id: the premise of the comparison)
    for a, b in zip(lp_f[0], lp_p[0]):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_session_admission_forms(engine, pages):
    """The same penalised request through admit, admit_prefix and admit_begin (the prompt in 2 chunks): the same ids.
    A chunked admission cancelled before its last slice leaves no record behind."""
    ids, mask, page = pages[0]
    p = DecodeParameters(max_new_tokens=STEPS)
    want = _penalised(engine, pages[0], FREQ, p)
    assert want != engine.generate(ids, mask, page, None, p)
    plain1 = engine.generate(*pages[1], None, p)
    rows = max(i for i, m in enumerate(mask) if m) + 1
    chunk = max(32, (len(ids) + 1) // 2)
    assert chunk < len(ids)
    got = {}

    def finish(sess):
        for _ in range(3):
            sess.step(8)
        return sess.retire(0)[0]

    with engine.open_session(2, len(ids) + STEPS + 1 + 8, p, penalties=True) as sess:
        assert sess.info()["flags"] == SESSION_PENALTIES
        assert sess.admit(ids, mask, page, max_new_tokens=STEPS, **_pkw(FREQ)) == 0
        handle = sess.keep_prefix(0, rows)
        got["admit"] = finish(sess)
        assert sess.admit_prefix(handle, ids, mask, max_new_tokens=STEPS, **_pkw(FREQ)) == 0
        got["prefix"] = finish(sess)
        sess.admit_begin(ids, mask, page, chunk_rows=chunk, max_new_tokens=STEPS, **_pkw(FREQ))
        sess.admit_advance()
        sess.admit_cancel()
        assert sess.admit(*pages[1], max_new_tokens=STEPS) == 0
        got["after_cancel"] = finish(sess)
        sess.admit_begin(ids, mask, page, chunk_rows=chunk, max_new_tokens=STEPS, **_pkw(FREQ))
        done = False
        while not done:
            done, slot = sess.admit_advance()
        assert slot == 0
        got["chunked"] = finish(sess)
        hs = sess.head_steps()
        assert hs["exact"] == 3 * 24  # the three penalised pages' bursts; the plain page's ran as a session without the flag does
    assert got["admit"] == got["prefix"] == got["chunked"] == want
    assert got["after_cancel"] == plain1


def test_session_refuses_without_flag(engine, pages):
    need = len(pages[0][0]) + 9
    with engine.open_session(2, need, DecodeParameters(max_new_tokens=8)) as sess:
        _einval(sess.admit, *pages[0], max_new_tokens=8, **_pkw(FREQ))
        rec = PenaltiesC(0.5, 0.0, 0.0)
        assert lib().dsocr_session_stage_penalties(engine._h, C.byref(rec)) == 1   # DSOCR_EINVAL
        off = PenaltiesC(0.0, 0.0, 0.0)
        assert lib().dsocr_session_stage_penalties(engine._h, C.byref(off)) == 0   # an off record asks for nothing
        assert sess.info()["active"] == 0
        assert sess.admit(*pages[0], max_new_tokens=8) == 0
    with engine.open_session(2, need, DecodeParameters(max_new_tokens=8), penalties=True) as sess:
        _einval(sess.admit, *pages[0], max_new_tokens=8, min_p=2.0)
        bad = PenaltiesC(float("nan"), 0.0, 0.0)
        assert lib().dsocr_session_stage_penalties(engine._h, C.byref(bad)) == 1
        assert sess.info()["active"] == 0


def test_feature_off_is_unchanged(engine, pages, oracle):
    """No flag, no record: the ids of the plain paths against the oracle and each other, the step count included."""
    p = DecodeParameters(max_new_tokens=12)
    a = engine.generate(*pages[0], None, p)
    assert a == oracle.generate(pages[0][0], pages[0][1], STEPS)[:12]
    steps = engine.last_timings()["decode_steps"]
    _penalised(engine, pages[0], FREQ, p)
    assert engine.generate(*pages[0], None, p) == a and engine.last_timings()["decode_steps"] == steps
    with engine.open_session(2, len(pages[0][0]) + 13, p) as sess:
        assert sess.info()["flags"] == 0
        sess.admit(*pages[0], max_new_tokens=12)
        sess.step(8)
        sess.step(8)
        assert sess.head_steps()["exact"] == 0
        assert sess.retire(0)[0] == a
    # a session with the flag and no record on: the screened head still runs, and the ids are the same
    with engine.open_session(2, len(pages[0][0]) + 13, p, penalties=True) as sess:
        sess.admit(*pages[0], max_new_tokens=12)
        sess.step(8)
        sess.step(8)
        assert sess.head_steps()["exact"] == 0
        assert sess.retire(0)[0] == a


def test_engine_that_never_saw_a_record(engine, pages):
    """A fresh engine that never saw a record against the module's engine after penalised calls, records off in
    both: the ids and the log-probability entries (the logits-derived outputs) byte for byte."""
    p = DecodeParameters(max_new_tokens=12)
    _penalised(engine, pages[0], FREQ, p)
    fresh = load_model(ModelLoadArgs(config_path=TINY, synthetic_seed=SEED, dtype="f16"))
    try:
        outs = []
        for eng in (fresh, engine):
            ids = eng.generate(*pages[0], None, p)
            g, lp, ti, tl = eng.generate_logprobs([(*pages[0], None)], 5, p)
            outs.append((ids, g[0], np.asarray(lp[0]).tobytes(), np.asarray(ti[0]).tobytes(), np.asarray(tl[0]).tobytes()))
    finally:
        fresh.close()
    assert outs[0] == outs[1]

