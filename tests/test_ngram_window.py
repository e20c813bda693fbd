"""The windowed no-repeat n-gram ban with a whitelist on the GPU.

The kernel through its hook against ``dsocr.ngram_window.apply`` (NumPy, byte for byte on the whole logit matrix); the
identity "unbounded window, no whitelist == the selection kernels' plain ban" through ``dsocr_k_select_rows``; the
engine against the CPU oracle, whose ``select_token_id`` is restated here with the windowed ban in the plain ban's place
(nothing under ``oracle/`` changes); decode sessions against the same page decoded alone.  Tiny config, the pages and
prompt of tests/test_session.py.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import dsocr
from dsocr import DecodeParameters, DsocrError, ModelLoadArgs, Page, VisionSettings, build_prompt_tokens, load_model
from dsocr._lib import SESSION_NGRAM_WINDOW, NgramWindowC, RowParamsC, check, lib
from dsocr.constraint import merge_constraint
from dsocr.ngram_window import UNBOUNDED, NgramWindow, apply, candidates
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
# The engine cases.  An allow-only bias onto ALLOW keeps the page inside five ids, so n-grams repeat within a few
# steps; the records are chosen on the CPU oracle so that the windowed ids differ both from the plain-ban ids (same g,
# whole context) and from the no-ban ids within STEPS tokens (every test asserts that on the oracle before it looks at
# the engine).  WHITE's whitelist changes the ids of WIN again.
ALLOW = [204, 348, 322, 77, 401]
WIN = NgramWindow(2, 6)
WHITE = NgramWindow(2, 6, (204,))
SAMPLE_KW = dict(do_sample=True, temperature=0.7, seed=11)


# ------------------------------------------------------------------ the kernel through its hook
def _recs_c(recs, keep):
    ptrs = []
    for r in recs:
        if r is None:
            ptrs.append(C.POINTER(NgramWindowC)())
            continue
        arr = (C.c_int32 * max(len(r.whitelist), 1))(*r.whitelist)
        rec = NgramWindowC(r.ngram_size, r.window, C.cast(arr, C.POINTER(C.c_int32)), len(r.whitelist))
        keep += [arr, rec]
        ptrs.append(C.pointer(rec))
    return (C.POINTER(NgramWindowC) * len(recs))(*ptrs)


def k_window(logits, ctx, lens, recs, plain=0):
    """The hook on host rows; returns the logit matrix it leaves."""
    B, ld = logits.shape
    V = k_window.V
    got = np.ascontiguousarray(logits, np.float32).copy()
    ctx = np.ascontiguousarray(ctx, np.int32)
    lens = np.ascontiguousarray(lens, np.int32)
    keep = []
    check(lib().dsocr_k_ngram_window(B, V, ld, got.ctypes.data_as(C.c_void_p), ctx.ctypes.data_as(C.c_void_p),
                                     ctx.shape[1], lens.ctypes.data_as(C.c_void_p), _recs_c(recs, keep), plain))
    return got


k_window.V = 1003
KV, KLD = 1003, 1011


def _check_rows(x, ctx, lens, recs):
    """One launch on the batch against NumPy, byte for byte on the whole matrix (columns [V, ld) included)."""
    got = k_window(x, ctx, lens, recs)
    want = x.copy()
    for b, r in enumerate(recs):
        want[b, :KV] = apply(x[b, :KV], ctx[b, :lens[b]], r)
    assert got.tobytes() == want.tobytes(), [b for b in range(len(recs)) if got[b].tobytes() != want[b].tobytes()]
    return got


def _logits(B, seed):
    r = np.random.default_rng(seed)
    x = np.full((B, KLD), SENTINEL, np.float32)
    x[:, :KV] = (r.standard_normal((B, KV)) * 4).astype(np.float32)
    return x


def _ctx(rows, cap):
    ctx = np.full((len(rows), cap), 999, np.int32)  # (behind ctx_len: never read)
    for b, row in enumerate(rows):
        ctx[b, :len(row)] = row
    return ctx, np.array([len(r) for r in rows], np.int32)


def test_kernel_short_and_exact_contexts(gpu):
    """n < g: nothing.  n == g with the one admissible start (0) matching: a run of one id.  Matches at the last
    starts n - g - 1 and n - g, which overlap the suffix.  One match in the middle of a row."""
    rows = [[5, 6], [7, 7, 7], [1, 2, 9, 9, 9, 9], [3, 4, 5, 8, 4, 5]]
    recs = [NgramWindow(3, 50), NgramWindow(3, 50), NgramWindow(3, 50), NgramWindow(3, 50)]
    ctx, lens = _ctx(rows, 16)
    x = _logits(4, 1)
    got = _check_rows(x, ctx, lens, recs)
    assert got[0].tobytes() == x[0].tobytes()                          # n < g
    assert got[1, 7] == -np.inf and np.isfinite(got[1, :KV]).sum() == KV - 1   # n == g, start 0: (7,7) -> 7
    assert got[2, 9] == -np.inf                                        # starts 2 and 3 (= n - g) overlap the suffix
    assert got[3, 8] == -np.inf and np.isfinite(got[3, :KV]).sum() == KV - 1   # (4,5) -> 8 at start 1


def test_kernel_window_edge(gpu):
    """Two rows equal except for w and w + 1, where the only match starts at n - w - 1: the first row is unchanged."""
    g, n = 3, 40
    row = list(range(100, 100 + n))
    row[-2:] = [500, 501]
    start = 12
    row[start:start + 3] = [500, 501, 77]
    w = n - start - 1
    ctx, lens = _ctx([row, row], 64)
    x = _logits(2, 2)
    x[1] = x[0]
    got = _check_rows(x, ctx, lens, [NgramWindow(g, w), NgramWindow(g, w + 1)])
    assert got[0].tobytes() == x[0].tobytes()
    assert got[1, 77] == -np.inf and np.isfinite(got[1, :KV]).sum() == KV - 1


def test_kernel_bigrams_long_suffix_and_batch_with_record_off(gpu):
    """g = 2; a g whose suffix (1200 ids) is longer than a block and than the LDS copy; a whitelisted candidate beside
    a banned one; context ids of -1 and >= V; a logit that is already -inf; a record off (None and g = 0) in the batch."""
    r = np.random.default_rng(3)
    big = r.integers(0, 50, 1200).tolist()
    long_row = big + [321] + [11, 12] + big                    # start 0 repeats the 1200-id suffix: 321 follows it
    near = big[:-1] + [49 if big[-1] != 49 else 48]            # (a near miss that fails on the last suffix id)
    bi = [9, 40, 3, 9, 41, 9, -1, 9, KV, 9, KV + 7, 9, 42, 9]  # 9 is followed by 40, 41, -1, V, V + 7, 42
    rows = [bi, long_row, bi, bi, near + [600] + big]
    recs = [NgramWindow(2, 100, (41,)), NgramWindow(1201, UNBOUNDED), None, NgramWindow(0, 5), NgramWindow(1201, UNBOUNDED)]
    ctx, lens = _ctx(rows, 2500)
    x = _logits(5, 4)
    x[0, 42] = -np.inf
    got = _check_rows(x, ctx, lens, recs)
    assert got[0, 40] == -np.inf and got[0, 42] == -np.inf and got[0, 41] == x[0, 41]
    assert np.isfinite(got[0, :KV]).sum() == KV - 2
    assert got[1, 321] == -np.inf and np.isfinite(got[1, :KV]).sum() == KV - 1
    assert got[2].tobytes() == x[2].tobytes() and got[3].tobytes() == x[3].tobytes()
    assert got[4].tobytes() == x[4].tobytes()
    # the same batch with plain = 2: the rows whose record is off take the plain bigram ban over the whole context
    plain = k_window(x, ctx, lens, recs, plain=2)
    for b in (2, 3):
        assert plain[b, :KV].tobytes() == apply(x[b, :KV], bi, NgramWindow(2, UNBOUNDED)).tobytes()
        assert plain[b, 40] == -np.inf and plain[b, 41] == -np.inf
    assert plain[0].tobytes() == got[0].tobytes() and plain[1].tobytes() == got[1].tobytes()


def test_kernel_long_context(gpu):
    """About 3000 context ids over a small alphabet with w = 2500: grid strides are crossed, many starts match, and a
    match just outside the window does not count."""
    r = np.random.default_rng(5)
    n, w, g = 3001, 2500, 3
    row = r.integers(0, 12, n)
    row[-2:] = [3, 4]
    row[100:103] = [3, 4, 700]                                   # outside the window (n - w = 501)
    row[501:504] = [3, 4, 701]                                   # the first admissible start
    rows = [row.tolist(), row.tolist()]
    ctx, lens = _ctx(rows, 3008)
    x = _logits(2, 6)
    got = _check_rows(x, ctx, lens, [NgramWindow(g, w, (5, 6)), NgramWindow(g, w - 1)])
    assert got[0, 700] == x[0, 700] and got[0, 701] == -np.inf and got[1, 701] == x[1, 701]
    assert len(candidates(rows[0], g, w)) > 10
    assert got[0, 5] == x[0, 5] and got[0, 6] == x[0, 6]


def test_kernel_fallback(gpu):
    """The ban is dropped when it would leave no finite logit: two finite logits, both banned (unchanged); the same
    plus one finite survivor (applied); three finite logits and five matches of one id (applied: more matches than
    finite logits, yet two survive)."""
    a, b_, c = 30, 600, 1002
    both = [8, a, 8, b_, 8]
    five = [8, a] * 5 + [8]
    ctx, lens = _ctx([both, both, five, both], 16)
    x = np.full((4, KLD), SENTINEL, np.float32)
    x[:, :KV] = -np.inf
    x[0, [a, b_]] = [1.5, -2.0]
    x[1, [a, b_, c]] = [1.5, -2.0, 0.25]
    x[2, [a, b_, c]] = [1.5, -2.0, 0.25]
    x[3, [a, b_]] = [np.nan, np.inf]                             # (NaN and +inf are not finite either: nothing to keep)
    x[3, 7] = 1.0
    got = _check_rows(x, ctx, lens, [NgramWindow(2, 10)] * 4)
    assert got[0].tobytes() == x[0].tobytes()
    assert got[1, a] == -np.inf and got[1, b_] == -np.inf and got[1, c] == np.float32(0.25)
    assert got[2, a] == -np.inf and got[2, b_] == np.float32(-2.0)
    assert got[3, a] == -np.inf and got[3, b_] == -np.inf and got[3, 7] == 1.0


# ------------------------------------------------------------------ identity with the selection kernels' plain ban
@pytest.mark.parametrize("g", [2, 3, 5])
def test_identity_with_plain_ban(gpu, g):
    """Random repetitive contexts over a small alphabet: the hook with an unbounded window and no whitelist, then
    dsocr_k_select_rows with ngram = 0, picks the ids of dsocr_k_select_rows with ngram = g alone.  Rows 0..2 greedy,
    row 3 sampled (8 draws)."""
    from _dev import Dev
    B, V, cap, draws = 4, 1003, 256, 8
    r = np.random.default_rng(100 + g)
    x = (r.standard_normal((B, V)) * 3).astype(np.float32)
    lens = np.array([200, 37, g, 256], np.int32)
    ctx = r.integers(0, 3, (B, cap)).astype(np.int32)
    x[:, :3] += 6.0                                              # the alphabet's ids lead: the ban decides the argmax
    seeds = (C.c_uint64 * B)(1, 2, 3, 4)

    def select(logits, ngram):
        rows = (RowParamsC * B)()
        for b in range(B):
            rows[b] = RowParamsC(1 if b == 3 else 0, 0.8, 0.95, 0, 1.0, ngram, -1)
        dl, dc, dn = Dev(logits), Dev(ctx), Dev(lens)
        dt = Dev.zeros(draws * B, np.int32)
        check(lib().dsocr_k_select_rows(B, V, dl.ptr, dc.ptr, cap, dn.ptr, rows, seeds, draws, dt.ptr))
        return dt.get().reshape(draws, B)

    k_window.V = V
    try:
        banned = k_window(x, ctx, lens, [NgramWindow(g, UNBOUNDED)] * B)
    finally:
        k_window.V = KV
    assert (banned != x).any()
    want, got, free = select(x, g), select(banned, 0), select(x, 0)
    assert got.tolist() == want.tolist()
    assert want.tolist() != free.tolist()                        # (the ban decides something: the case shows the identity)


# ------------------------------------------------------------------ select_token_id with the windowed ban
def select_with_window(logits, context, rec, repetition_penalty=1.0, no_repeat_ngram_size=None, do_sample=False,
                       temperature=0.0, top_k=None, top_p=None, rng=None):
    """oracle.decoder.select_token_id restated with DESIGN 4.20's step: a record that is on takes the plain ban's
    place (``apply`` carries the has_valid_logits fallback); off, the plain ban runs as in the oracle."""
    import math

    from oracle.decoder import argmax_first, banned_ngram_tokens
    from oracle.sampling import apply_top_k, apply_top_p, sample_from_logits
    logits = np.asarray(logits, np.float32)
    adjusted = logits.copy()
    if repetition_penalty > 0.0 and abs(repetition_penalty - 1.0) > np.finfo(np.float32).eps:
        rp = np.float32(repetition_penalty)
        for t in dict.fromkeys(int(c) for c in context):
            if 0 <= t < len(adjusted):
                adjusted[t] = adjusted[t] / rp if adjusted[t] > 0 else adjusted[t] * rp
    if rec is not None and not rec.off:
        filtered = apply(adjusted, context, rec)
    else:
        filtered = adjusted.copy()
        if no_repeat_ngram_size is not None and no_repeat_ngram_size > 1:
            for t in banned_ngram_tokens([int(c) for c in context], no_repeat_ngram_size):
                if 0 <= t < len(filtered):
                    filtered[t] = -np.inf
        if not np.any(np.isfinite(filtered)):
            filtered = adjusted
    if do_sample and temperature > 0.0:
        lg = [float(v) / temperature for v in filtered]
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

    def generate(self, ids, mask, max_new, rec=None, dense=None, **kw):
        key = (max_new, rec, None if dense is None else dense.tobytes(), tuple(sorted(kw.items())))
        if key in self.cache:
            return self.cache[key]
        om, real = self.om, self.om.select_token_id

        def select(logits, context, repetition_penalty=1.0, no_repeat_ngram_size=None, **sel):
            l = np.asarray(logits, np.float32)
            if dense is not None:
                l = l + dense
            return select_with_window(l, context, rec, repetition_penalty, no_repeat_ngram_size, **sel)

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


@pytest.fixture(scope="module")
def allow(engine):
    con = merge_constraint(allowed_token_ids=ALLOW, vocab=engine.vocab)
    return con, con.dense(engine.vocab)


def _windowed(engine, req, rec, params, **kw):
    return engine.generate_ngram_window([(*req, None)], [rec], params, **kw)[0][0]


def _three(oracle, pages, dense, rec, **kw):
    """(windowed, plain ban of the same size, no ban) on the oracle, asserted pairwise different."""
    ids, mask, _ = pages[0]
    want = oracle.generate(ids, mask, STEPS, rec, dense=dense, **kw)
    plain = oracle.generate(ids, mask, STEPS, dense=dense, no_repeat_ngram_size=rec.ngram_size, **kw)
    free = oracle.generate(ids, mask, STEPS, dense=dense, **kw)
    assert want != plain and want != free, "the window changes nothing on this page: pick another record"
    return want, plain, free


def test_oracle_restatement_is_the_oracle(oracle, pages):
    """With the record off the restated select_token_id gives the oracle's own ids, greedy and sampled."""
    import oracle.model as om
    ids, mask, _ = pages[0]
    for kw in ({}, dict(repetition_penalty=1.3, no_repeat_ngram_size=3), dict(top_p=0.9, **SAMPLE_KW)):
        real, _ = oracle.model.generate(ids, mask, oracle.emb, 12, eos_token_id=1, **kw)
        assert oracle.generate(ids, mask, 12, **kw) == [int(t) for t in real]
    assert om.select_token_id.__module__ == "oracle.decoder"


def test_engine_greedy(engine, pages, oracle, allow):
    """The record replaces the plain ban: params still carry no_repeat_ngram_size (and, in the second run, a
    repetition penalty in front of the ban)."""
    con, dense = allow
    want, plain, free = _three(oracle, pages, dense, WIN)
    p = DecodeParameters(max_new_tokens=STEPS, no_repeat_ngram_size=WIN.ngram_size)
    assert engine.generate_constrained([(*pages[0], None)], [con], p)[0] == plain
    assert _windowed(engine, pages[0], WIN, p, constraints=[con]) == want
    assert _windowed(engine, pages[0], None, p, constraints=[con]) == plain      # a NULL record: the plain call
    kw = dict(repetition_penalty=1.3)
    ids, mask, _ = pages[0]
    want_rp = oracle.generate(ids, mask, STEPS, WIN, dense=dense, **kw)
    got = _windowed(engine, pages[0], WIN, DecodeParameters(max_new_tokens=STEPS, no_repeat_ngram_size=20, **kw), constraints=[con])
    assert got == want_rp


def test_engine_whitelist_changes_the_result(engine, pages, oracle, allow):
    con, dense = allow
    want, _, _ = _three(oracle, pages, dense, WHITE)
    assert want != oracle.generate(pages[0][0], pages[0][1], STEPS, WIN, dense=dense), "the whitelist changes nothing: pick another"
    assert _windowed(engine, pages[0], WHITE, DecodeParameters(max_new_tokens=STEPS), constraints=[con]) == want


def test_engine_sampled(engine, pages, oracle, allow):
    con, dense = allow
    want, _, _ = _three(oracle, pages, dense, WIN, **SAMPLE_KW)
    assert _windowed(engine, pages[0], WIN, DecodeParameters(max_new_tokens=STEPS, **SAMPLE_KW), constraints=[con]) == want


def test_engine_batch_and_logprobs(engine, pages, oracle, allow):
    """A generate call of two pages, one windowed and one on the plain ban of the call's parameters (which the window
    launch applies for it), with log-probabilities: the ids are the oracle's and the single-page runs', and the
    entries are those of the bias-constrained distribution, which the ban does not enter: bit for bit the entries of
    the steps of the same batch without a record that saw the same prefix."""
    con, dense = allow
    want, plain, _ = _three(oracle, pages, dense, WIN)
    p = DecodeParameters(max_new_tokens=STEPS, no_repeat_ngram_size=WIN.ngram_size)
    reqs = [(*pages[0], None), (*pages[0], None)]
    got, _, lp, ti, tl = engine.generate_ngram_window(reqs, [WIN, None], p, top_k=5, constraints=[con, con])
    assert got[0] == want and got[1] == plain
    # the same batch without a record (a row's last bits depend on the batch it runs in, DESIGN 4.19's closing note, so
    # the comparison is between batches of two, and ends where row 0's emissions part: steps [0, same] saw the same
    # prefixes in both rows)
    g0, lp0, ti0, tl0 = engine.generate_constrained(reqs, [con, con], p, top_k=5)
    assert g0[0] == plain and g0[1] == plain
    same = next(i for i in range(STEPS) if want[i] != plain[i])
    assert same > 0
    for row in (0, 1):
        assert np.asarray(ti[row][:same + 1]).tobytes() == np.asarray(ti0[row][:same + 1]).tobytes()
        assert np.asarray(tl[row][:same + 1]).tobytes() == np.asarray(tl0[row][:same + 1]).tobytes()
        assert np.asarray(lp[row][:same]).tobytes() == np.asarray(lp0[row][:same]).tobytes()
        assert all(np.isfinite(np.asarray(lp[row])))               # an emitted id is never one the kernel rewrote


def _einval(fn, *a, **kw):
    with pytest.raises(DsocrError) as ei:
        fn(*a, **kw)
    assert ei.value.status == 1, ei.value


def test_engine_refuses(engine, pages, monkeypatch):
    p4 = DecodeParameters(max_new_tokens=4)
    _einval(_windowed, engine, pages[0], WIN, DecodeParameters(max_new_tokens=4, use_cache=False))
    for bad in (NgramWindow(2, 0), NgramWindow(3, -5), NgramWindow(2, 5, (engine.vocab,)), NgramWindow(2, 5, tuple(range(33)))):
        _einval(_windowed, engine, pages[0], bad, p4)
    monkeypatch.setenv("DSOCR_PERSIST", "1")
    _einval(_windowed, engine, pages[0], WIN, p4)
    monkeypatch.delenv("DSOCR_PERSIST")
    # nothing was left behind: the plain call still runs, and a record that is off is the plain call
    a = engine.generate(*pages[0], None, p4)
    assert len(a) == 4 and _windowed(engine, pages[0], None, p4) == a and _windowed(engine, pages[0], NgramWindow(0, 5), p4) == a
    assert _windowed(engine, pages[0], NgramWindow(2, 1), p4) == engine.generate(
        *pages[0], None, DecodeParameters(max_new_tokens=4, no_repeat_ngram_size=0))   # w < g never matches


# ------------------------------------------------------------------ sessions
def _ckw(con):
    return dict(allowed_token_ids=list(con.ids)) if con is not None else {}


@pytest.mark.parametrize("per_request", [True, False], ids=["per_request", "fixed"])
def test_session_mixed_batch(engine, pages, allow, per_request):
    """3 slots {windowed, plain ban, plain ban / no ban}: every page equals its single-page run through two
    compactions.  Per request the third page runs without a ban; with fixed parameters every page shares the
    session's no_repeat_ngram_size, the selections of a windowed burst run at ngram 0 and the window launch bans for
    the plain rows, and the burst after the windowed page has left runs the exact head once more."""
    con, _ = allow
    g = WIN.ngram_size
    P = lambda m, n=g: DecodeParameters(max_new_tokens=m, no_repeat_ngram_size=n)
    prm = {0: P(6), 1: P(STEPS), 2: P(STEPS, 0 if per_request else g)}
    rec = {0: None, 1: WIN, 2: None}
    single = {i: _windowed(engine, pages[i], rec[i], prm[i], constraints=[con]) for i in prm}
    assert single[1] != engine.generate_constrained([(*pages[1], None)], [con], prm[1])[0], "the window changes nothing on page 1"
    assert single[2] != _windowed(engine, pages[2], None, P(STEPS, 0 if not per_request else g), constraints=[con]), \
        "the plain ban changes nothing on page 2"
    need = max(len(pages[i][0]) + prm[i].max_new_tokens + 1 for i in prm) + 8
    with engine.open_session(3, need, P(STEPS), per_request=per_request, logit_bias=True, ngram_window=True) as sess:
        assert sess.info()["flags"] & SESSION_NGRAM_WINDOW
        kw = (lambda i: dict(params=prm[i])) if per_request else (lambda i: dict(max_new_tokens=prm[i].max_new_tokens))
        assert sess.admit(*pages[0], **kw(0), **_ckw(con)) == 0
        assert sess.admit(*pages[1], **kw(1), **_ckw(con), ngram_window=rec[1]) == 1
        assert sess.admit(*pages[2], **kw(2), **_ckw(con)) == 2
        sess.step(8)
        ids0, moved = sess.retire(0)
        assert moved == 2
        sess.step(4)
        part2, moved = sess.retire(0)                  # the windowed page moves from 1 to 0 with its record
        assert moved == 1
        sess.step(8)
        ids1, _ = sess.retire(0)
        # a plain page after the windowed one has left: the plain ban is back in the selection
        assert sess.admit(*pages[2], **kw(2), **_ckw(con)) == 0
        for _ in range(3):
            sess.step(8)
        again, _ = sess.retire(0)
    assert ids0 == single[0] and ids1 == single[1]
    assert part2 == single[2][:len(part2)] and len(part2) >= 12
    assert again == single[2]


def test_session_head_returns_to_screened(engine, pages):
    """Fixed parameters, no bias: a plain page shares two bursts with a windowed page that then leaves.  The windowed
    bursts ran every selection at ngram 0, so the ban lists a screened head reads are stale: one more exact burst
    writes them again, then the screened head is back, and the plain page's ids are those of a session without the
    flag."""
    g = 2
    p = DecodeParameters(max_new_tokens=STEPS, no_repeat_ngram_size=g)
    need = max(len(pages[i][0]) for i in range(2)) + STEPS + 1 + 8
    with engine.open_session(2, need, p) as sess:
        sess.admit(*pages[0], max_new_tokens=STEPS)
        for _ in range(5):
            sess.step(4)
        screened_all = sess.head_steps()["exact"] == 0
        want = sess.retire(0)[0]
    assert want != engine.generate(*pages[0], None, DecodeParameters(max_new_tokens=STEPS, no_repeat_ngram_size=0)), \
        "the plain ban changes nothing on page 0"
    with engine.open_session(2, need, p, ngram_window=True) as sess:
        sess.admit(*pages[0], max_new_tokens=STEPS)
        sess.admit(*pages[1], max_new_tokens=6, ngram_window=NgramWindow(3, 4))
        sess.step(4)
        sess.step(4)
        assert sess.head_steps() == {"exact": 8, "screened": 0}
        sess.retire(1)
        sess.step(4)
        hs = sess.head_steps()
        assert hs["exact"] == 12                          # the ban lists are written again
        sess.step(4)
        sess.step(4)
        if screened_all:
            assert sess.head_steps() == {"exact": 12, "screened": 8}
        assert sess.retire(0)[0] == want


def test_session_plain_row_is_bit_for_bit(engine, pages):
    """The plain row of a per-request batch whose other rows carry records, against a session without the flag: ids
    and log-probability entries bit for bit.  Other rows' emissions move a row's last bits (the note at the end of
    DESIGN 4.19), so the other two rows carry records that are on and change no id: g = 400 is longer than any context
    here, so n < g and nothing is ever banned.  The exact head and the window launch run; only row 0's isolation is
    left to show."""
    P = lambda m, **kw: DecodeParameters(max_new_tokens=m, **kw)
    prm = {0: P(6), 1: P(STEPS), 2: P(STEPS, **SAMPLE_KW)}
    assert max(len(pg[0]) for pg in pages) + STEPS < 400
    rec = {0: None, 1: NgramWindow(400, 90), 2: NgramWindow(400, 500, (3, 4))}
    need = max(len(pages[i][0]) + prm[i].max_new_tokens + 1 for i in prm) + 8
    # (the records switch rows 1 and 2's plain ban off: without the flag they run without one)
    off = {i: P(prm[i].max_new_tokens, no_repeat_ngram_size=0, **(SAMPLE_KW if i == 2 else {})) for i in (1, 2)}

    def run(flag):
        kw = {"ngram_window": True} if flag else {}
        with engine.open_session(3, need, P(STEPS), per_request=True, logprobs=True, **kw) as sess:
            sess.admit(*pages[0], params=prm[0])
            for i in (1, 2):
                if flag:
                    sess.admit(*pages[i], params=prm[i], ngram_window=rec[i])
                else:
                    sess.admit(*pages[i], params=off[i])
            sess.step(8)
            lp = [sess.logprobs(i, 0, 6, 5) for i in range(3)]
            ids = [sess.retire(i)[0] for i in (2, 1, 0)][::-1]
        return ids, lp

    ids_f, lp_f = run(True)
    ids_p, lp_p = run(False)
    assert ids_f == ids_p
    for a, b in zip(lp_f[0], lp_p[0]):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_session_admission_forms(engine, pages, allow):
    """The same windowed request through admit, admit_prefix and admit_begin (the prompt in 2 chunks): the same ids.
    A chunked admission cancelled before its last slice leaves no record behind."""
    con, _ = allow
    ids, mask, page = pages[0]
    p = DecodeParameters(max_new_tokens=STEPS, no_repeat_ngram_size=WIN.ngram_size)
    want = _windowed(engine, pages[0], WIN, p, constraints=[con])
    plain0 = engine.generate_constrained([(*pages[0], None)], [con], p)[0]
    assert want != plain0
    rows = max(i for i, m in enumerate(mask) if m) + 1
    chunk = max(32, (len(ids) + 1) // 2)
    assert chunk < len(ids)
    got = {}
    ckw = _ckw(con)

    def finish(sess):
        for _ in range(3):
            sess.step(8)
        return sess.retire(0)[0]

    with engine.open_session(2, len(ids) + STEPS + 1 + 8, p, logit_bias=True, ngram_window=True) as sess:
        assert sess.admit(ids, mask, page, max_new_tokens=STEPS, ngram_window=WIN, **ckw) == 0
        handle = sess.keep_prefix(0, rows)
        got["admit"] = finish(sess)
        assert sess.admit_prefix(handle, ids, mask, max_new_tokens=STEPS, ngram_window=WIN, **ckw) == 0
        got["prefix"] = finish(sess)
        sess.admit_begin(ids, mask, page, chunk_rows=chunk, max_new_tokens=STEPS, ngram_window=WIN, **ckw)
        sess.admit_advance()
        sess.admit_cancel()
        assert sess.admit(ids, mask, page, max_new_tokens=STEPS, **ckw) == 0
        got["after_cancel"] = finish(sess)
        sess.admit_begin(ids, mask, page, chunk_rows=chunk, max_new_tokens=STEPS, ngram_window=WIN, **ckw)
        done = False
        while not done:
            done, slot = sess.admit_advance()
        assert slot == 0
        got["chunked"] = finish(sess)
    assert got["admit"] == got["prefix"] == got["chunked"] == want
    assert got["after_cancel"] == plain0


def test_session_refuses_without_flag(engine, pages):
    need = len(pages[0][0]) + 9
    arr = (C.c_int32 * 1)(3)
    with engine.open_session(2, need, DecodeParameters(max_new_tokens=8)) as sess:
        _einval(sess.admit, *pages[0], max_new_tokens=8, ngram_window=WIN)
        rec = NgramWindowC(2, 6, C.cast(arr, C.POINTER(C.c_int32)), 1)
        assert lib().dsocr_session_stage_ngram_window(engine._h, C.byref(rec)) == 1   # DSOCR_EINVAL
        off = NgramWindowC(0, 0, None, 0)
        assert lib().dsocr_session_stage_ngram_window(engine._h, C.byref(off)) == 0   # an off record asks for nothing
        assert sess.info()["active"] == 0
        assert sess.admit(*pages[0], max_new_tokens=8) == 0
    with engine.open_session(2, need, DecodeParameters(max_new_tokens=8), ngram_window=True) as sess:
        _einval(sess.admit, *pages[0], max_new_tokens=8, ngram_window=NgramWindow(2, 0))
        bad = NgramWindowC(2, 6, C.cast(arr, C.POINTER(C.c_int32)), 40)
        assert lib().dsocr_session_stage_ngram_window(engine._h, C.byref(bad)) == 1
        assert sess.info()["active"] == 0


def test_feature_off_is_unchanged(engine, pages, oracle):
    """No flag, no record: the ids of the plain paths against the oracle and each other; a session with the flag and
    no record on still runs the screened head, and its ids are the same."""
    p = DecodeParameters(max_new_tokens=12)
    ids, mask, _ = pages[0]
    a = engine.generate(*pages[0], None, p)
    assert a == oracle.generate(ids, mask, 12)
    steps = engine.last_timings()["decode_steps"]
    _windowed(engine, pages[0], WIN, p)
    assert engine.generate(*pages[0], None, p) == a and engine.last_timings()["decode_steps"] == steps
    heads = []
    for kw in ({}, {"ngram_window": True}):
        with engine.open_session(2, len(ids) + 13, p, **kw) as sess:
            assert sess.info()["flags"] == (SESSION_NGRAM_WINDOW if kw else 0)
            sess.admit(*pages[0], max_new_tokens=12)
            sess.step(8)
            sess.step(8)
            heads.append(sess.head_steps())
            assert sess.retire(0)[0] == a
    assert heads[0] == heads[1]


def test_engine_that_never_saw_a_record(engine, pages):
    """A fresh engine that never saw a record against the module's engine after windowed calls, records off in both:
    the ids and the log-probability entries (the logits-derived outputs) byte for byte."""
    p = DecodeParameters(max_new_tokens=12)
    _windowed(engine, pages[0], WIN, p)
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
