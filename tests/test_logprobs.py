"""Per-token log-probabilities on the GPU: the two kernels through their hook, the engine against its own logits
trace, decode sessions against the single-page run.

The reference for every number is NumPy in float64 on the same f32 logits: ``l64 - max - log(sum(exp(l64 - max)))``
over the finite entries, and a stable argsort of the negated logits for the alternatives (largest first, the lower id
on equal values).  Alternative ids must match exactly; log-probabilities within
``LP_C * 2**-23 * max(1, max_v |l[v] - m|)``.
"""
import ctypes as C
import os

import numpy as np
import pytest

from dsocr import DecodeParameters, ModelLoadArgs, Page, VisionSettings, build_prompt_tokens, load_model
from dsocr._lib import MAX_TOP_LOGPROBS, lib
from dsocr.synth import SyntheticTokenizer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, "deepseek-ocr.rs_amd", "dsocr", "configs", "tiny.json")
TINY_VS = VisionSettings(256, 128, True)
PROMPT = "<image>\nConvert the document to markdown."
SIZES = [(300, 420), (256, 256), (500, 140), (130, 130)]

# The bound's constant.  The order of the f32 sum and expf's error are the kernel's own choice, so the worst error of
# this file's hook cases against the float64 reference was measured on an MI355X, in units of
# 2**-23 * max(1, max|l - m|): 7.346 at V = 1003 (the flat row: lp = -log V = -6.9 at scale 1, so the unit is a
# quarter of the result's own ulp), 4.508 at V = 129280, 0.818 at V = 8, 0.178 at V = 512; the same at every B and K.
# The engine-against-trace cases (tiny model, scale ~ 1..3): 8.063 at worst (3 pages, sampled).
# LP_C is four times the worst figure of all of them.
LP_C = 32.3
EPS = 2.0 ** -23
KINDS = ["normal4", "flat", "dominant", "pm1e4", "ties", "nonfinite", "tok_nan", "tok_ninf", "all_nonfinite"]
CHUNK = 2048  # the partial kernel's chunk of the row: ties straddle its boundary


def ref_logprobs(l, tok, K):
    """float64 reference of one row: (lp of tok, alternative ids [K], their lps [K], the bound's scale)."""
    l = np.asarray(l, np.float32)
    fin = np.isfinite(l)
    ids = np.full(K, -1, np.int64)
    lps = np.full(K, -np.inf)
    if not fin.any():
        return -np.inf, ids, lps, 1.0
    l64 = l.astype(np.float64)
    m = l64[fin].max()
    lse = np.log(np.sum(np.exp(l64[fin] - m)))
    order = np.argsort(-np.where(fin, l64, -np.inf), kind="stable")[:min(K, int(fin.sum()))]
    ids[:len(order)] = order
    lps[:len(order)] = l64[order] - m - lse
    lp = l64[tok] - m - lse if fin[tok] else -np.inf
    return lp, ids, lps, max(1.0, float(np.abs(l64[fin] - m).max()))


def make_row(kind, V, seed):
    """One row of logits [V] f32 and the token to score."""
    r = np.random.default_rng(seed)
    x = (r.standard_normal(V) * 4).astype(np.float32)
    tok = int(r.integers(0, V))
    b0 = CHUNK - 1 if V > CHUNK else V // 2 - 1  # the last index of a chunk (or of the first half of a short row)
    if kind == "flat":
        x[:] = np.float32(0.37)
    elif kind == "dominant":
        x[:] = np.float32(-100.0)
        x[V // 3] = np.float32(100.0)
        tok = V // 3
    elif kind == "pm1e4":
        x = (np.where(r.random(V) < 0.5, 1e4, -1e4) + r.standard_normal(V)).astype(np.float32)
    elif kind == "ties":
        x = np.minimum(x, np.float32(3.0))
        for i in (0, b0, b0 + 1, V - 1):
            x[i] = np.float32(5.0)
        x[1] = x[V - 2] = np.float32(4.5)
        tok = V - 1
    elif kind in ("nonfinite", "tok_nan", "tok_ninf"):
        x[r.choice(V, max(1, V // 5), replace=False)] = -np.inf
        i_nan, i_inf = (1, 6) if V == 8 else (V // 2 + 1, V - 3)
        x[i_nan] = np.nan
        x[i_inf] = np.inf
        x[2] = np.float32(1.5)
        x[3] = -np.inf
        tok = {"nonfinite": 2, "tok_nan": i_nan, "tok_ninf": 3}[kind]
    elif kind == "all_nonfinite":
        x[:] = -np.inf
        x[0] = np.nan
        x[V - 1] = np.inf
    return x, tok


def k_logprobs(logits, tok, K, emit=None, ctx=None, ctx_len=None, penalty=None, sentinel=-7.0):
    """The hook on host rows: (lp [B], alternative ids [B][K], their lps [B][K]); rows start at the sentinel."""
    logits = np.ascontiguousarray(logits, np.float32)
    B, V = logits.shape
    tok = np.ascontiguousarray(tok, np.int32)
    emit = np.ones(B, np.uint8) if emit is None else np.ascontiguousarray(emit, np.uint8)
    lp = np.full(B, sentinel, np.float32)
    ti = np.full((B, max(K, 1)), int(sentinel), np.int64)
    tl = np.full((B, max(K, 1)), sentinel, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    if ctx is None:
        st = lib().dsocr_k_logprobs(B, V, K, p(logits), V, p(tok), p(emit), p(lp), p(ti), p(tl))
    else:
        ctx = np.ascontiguousarray(ctx, np.int32)
        ctx_len = np.ascontiguousarray(ctx_len, np.int32)
        st = lib().dsocr_k_logprobs_penalty(B, V, K, p(logits), V, p(tok), p(emit), p(ctx), ctx.shape[1], p(ctx_len),
                                            float(penalty), p(lp), p(ti), p(tl))
    assert st == 0, lib().dsocr_last_error()
    return lp, ti.reshape(B, -1)[:, :K], tl.reshape(B, -1)[:, :K]


_ROWS = {}


def rows_of(V):
    """Every row kind at this V, built once and never changed: (logits [kinds][V], tok [kinds])."""
    if V not in _ROWS:
        rows = [make_row(k, V, 1000 + 17 * i + V) for i, k in enumerate(KINDS)]
        x, t = np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], np.int32)
        x.setflags(write=False)
        _ROWS[V] = (x, t)
    return _ROWS[V]


def check_row(got_lp, got_ids, got_tl, l, tok, K, what):
    """One entry against the float64 reference; returns the worst error in units of 2**-23 * scale."""
    lp, ids, lps, scale = ref_logprobs(l, tok, K)
    assert np.array_equal(got_ids, ids), (what, got_ids, ids)
    worst = 0.0
    for g, r in [(float(got_lp), lp)] + list(zip(got_tl.astype(np.float64), lps)):
        if np.isinf(r):
            assert g == r, (what, g, r)
            continue
        assert np.isfinite(g), (what, g, r)
        worst = max(worst, abs(g - r) / (EPS * scale))
    return worst


@pytest.mark.parametrize("K", [0, 1, 5, 20])
@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("V", [8, 512, 1003, 129280])
def test_kernel_against_float64(gpu, V, B, K):
    x, tok = rows_of(V)
    worst = 0.0
    for r0 in range(0, len(KINDS), B):  # every kind in every (V, B, K): the kinds in calls of B rows (the last wraps)
        sel = [(r0 + i) % len(KINDS) for i in range(B)]
        lp, ti, tl = k_logprobs(x[sel], tok[sel], K)
        for j, r in enumerate(sel):
            worst = max(worst, check_row(lp[j], ti[j], tl[j], x[r], tok[r], K, (KINDS[r], V, B, K)))
    print(f"logprob worst error V={V} B={B} K={K}: {worst:.3f} x 2^-23 x scale")
    assert worst <= LP_C


def test_kernel_expected_values(gpu):
    """The closed forms: a flat row is -log V everywhere, a dominant logit has lp ~ 0 and finite alternatives whose
    exp underflows, a non-finite token and an all-non-finite row are -inf with padded alternatives."""
    V = 1003
    x, tok = rows_of(V)
    lp, ti, tl = k_logprobs(x, tok, 20)
    k = {n: i for i, n in enumerate(KINDS)}
    assert abs(lp[k["flat"]] + np.log(V)) < 1e-5 and np.array_equal(ti[k["flat"]], np.arange(20))
    assert np.allclose(tl[k["flat"]], -np.log(V), atol=1e-5)
    d = k["dominant"]
    assert lp[d] == 0.0 and ti[d][0] == V // 3 and np.all(tl[d][1:] == -200.0) and np.array_equal(ti[d][1:], np.arange(19))
    assert lp[k["tok_nan"]] == -np.inf and lp[k["tok_ninf"]] == -np.inf and np.isfinite(lp[k["nonfinite"]])
    a = k["all_nonfinite"]
    assert lp[a] == -np.inf and np.all(ti[a] == -1) and np.all(tl[a] == -np.inf)
    t = k["ties"]
    assert list(ti[t][:6]) == [0, V // 2 - 1, V // 2, V - 1, 1, V - 2]
    # V = 8 with K = 20: the row's finite entries, then (-1, -inf)
    x8, t8 = rows_of(8)
    lp8, ti8, tl8 = k_logprobs(x8[:1], t8[:1], 20)
    assert np.all(ti8[0][8:] == -1) and np.all(tl8[0][8:] == -np.inf) and sorted(ti8[0][:8]) == list(range(8))


@pytest.mark.parametrize("V", [1003, 129280])
def test_kernel_rows_are_independent(gpu, V):
    """Row r of a B = 8 call equals the B = 1 call on that row bit for bit, in forward and reversed row order; rows
    with emit = 0 keep the sentinel."""
    x, tok = rows_of(V)
    sel = list(range(8))
    one = [k_logprobs(x[[r]], tok[[r]], 20) for r in sel]
    for order in (sel, sel[::-1]):
        lp, ti, tl = k_logprobs(x[order], tok[order], 20)
        for j, r in enumerate(order):
            assert lp[j].tobytes() == one[r][0][0].tobytes(), (V, r)
            assert np.array_equal(ti[j], one[r][1][0]) and tl[j].tobytes() == one[r][2][0].tobytes(), (V, r)
    emit = np.array([1, 0, 1, 0, 0, 1, 1, 0], np.uint8)
    lp, ti, tl = k_logprobs(x[sel], tok[sel], 20, emit=emit, sentinel=-7.0)
    for j in sel:
        if emit[j]:
            assert lp[j].tobytes() == one[j][0][0].tobytes() and np.array_equal(ti[j], one[j][1][0])
        else:
            assert lp[j] == -7.0 and np.all(ti[j] == -7) and np.all(tl[j] == -7.0)


@pytest.mark.parametrize("V", [512, 129280])
def test_kernel_penalty_path(gpu, V):
    """With a context row and penalty 1.3 between the two launches the entry is bit-equal to the call without a
    penalty on the same raw logits: tok in the context at a positive and at a negative raw logit, and outside it."""
    r = np.random.default_rng(V)
    x = (r.standard_normal((3, V)) * 4).astype(np.float32)
    pos, neg, out = V - 5, 7, V // 2
    x[0, pos], x[1, neg] = np.float32(2.75), np.float32(-3.25)
    cap = 40
    ctx = r.integers(0, V, (3, cap)).astype(np.int32)
    ctx[ctx == out] = out + 1
    ctx[0, 9] = ctx[0, 30] = pos      # twice in the context: the first match is the one the penalty applied at
    ctx[1, 0] = neg
    ctx_len = np.array([cap, 33, 21], np.int32)
    tok = np.array([pos, neg, out], np.int32)
    base = k_logprobs(x, tok, 20)
    pen = k_logprobs(x, tok, 20, ctx=ctx, ctx_len=ctx_len, penalty=1.3)
    for a, b in zip(base, pen):
        assert a.tobytes() == b.tobytes()
    for j in range(3):
        check_row(pen[0][j], pen[1][j], pen[2][j], x[j], tok[j], 20, ("penalty", V, j))


# ------------------------------------------------------------------ the engine against its own trace
@pytest.fixture(scope="module")
def engine(gpu):
    eng = load_model(ModelLoadArgs(config_path=TINY, synthetic_seed=7, dtype="f16"))
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def pages():
    tok = SyntheticTokenizer(512)
    out = []
    for i, hw in enumerate(SIZES):
        img = np.random.default_rng(100 + i).integers(0, 256, (*hw, 3), dtype=np.uint8)
        page = Page(img, TINY_VS)
        ids, mask = build_prompt_tokens(tok, PROMPT, [page.n_image_tokens])
        out.append((ids, mask, page, None))
    return out


def _against_trace(engine, reqs, params, K=20):
    plain = engine.generate_batch(reqs, params)
    ids, lp, ti, tl = engine.generate_logprobs(reqs, K, params)
    tids, logits = engine.generate_trace(reqs, params)
    assert ids == plain == tids
    worst = 0.0
    for i in range(len(reqs)):
        assert len(lp[i]) == len(ids[i]) == ti[i].shape[0] == tl[i].shape[0]  # entry count == n_out
        for t, tok in enumerate(ids[i]):
            worst = max(worst, check_row(lp[i][t], ti[i][t], tl[i][t], logits[i][t], tok, K, ("engine", i, t)))
    print(f"engine logprob worst error over {len(reqs)} page(s): {worst:.3f} x 2^-23 x scale")
    assert worst <= LP_C
    return ids, lp


@pytest.mark.parametrize("n", [1, 3])
def test_engine_greedy(engine, pages, n):
    ids, _ = _against_trace(engine, pages[:n], DecodeParameters(max_new_tokens=24))
    assert all(len(x) > 0 for x in ids)


@pytest.mark.parametrize("n", [1, 3])
def test_engine_eos_midway(engine, pages, n):
    """EOS set to an id page 0 emits mid-way: no entry for it and none after it (in a batch the other pages stop
    where they emit that id, or run on)."""
    p = DecodeParameters(max_new_tokens=24)
    full = engine.generate_batch(pages[:n], p)
    cut = next(t for t in range(3, len(full[0])) if full[0][t] not in full[0][:t])
    eos0 = engine.eos_token_id
    engine.eos_token_id = eos = int(full[0][cut])
    try:
        ids, lp = _against_trace(engine, pages[:n], p)
    finally:
        engine.eos_token_id = eos0
    for i in range(n):
        want = full[i][:full[i].index(eos)] if eos in full[i] else full[i]
        assert ids[i] == want and len(lp[i]) == len(want)
    assert len(lp[0]) == cut


@pytest.mark.parametrize("n", [1, 3])
def test_engine_repetition_penalty(engine, pages, n):
    _against_trace(engine, pages[:n], DecodeParameters(max_new_tokens=24, repetition_penalty=1.3))
    if n == 1:
        _against_trace(engine, pages[:1], DecodeParameters(max_new_tokens=24, repetition_penalty=1.3), K=0)


@pytest.mark.parametrize("n", [1, 3])
def test_engine_sampled(engine, pages, n):
    _against_trace(engine, pages[:n], DecodeParameters(max_new_tokens=24, do_sample=True, temperature=0.8, top_p=0.9,
                                                       seed=11))


def _einval(fn, *a, **kw):
    """The call is refused with DSOCR_EINVAL (status 1)."""
    from dsocr import DsocrError
    with pytest.raises(DsocrError) as ei:
        fn(*a, **kw)
    assert ei.value.status == 1, ei.value


def test_engine_refuses(engine, pages):
    _einval(engine.generate_logprobs, pages[:1], 3, DecodeParameters(max_new_tokens=4, use_cache=False))
    _einval(engine.generate_logprobs, pages[:1], MAX_TOP_LOGPROBS + 1, DecodeParameters(max_new_tokens=4))


# ------------------------------------------------------------------ sessions
def _single_lp(engine, pages, i, max_new, **kw):
    """The single-page run: (ids, lp [n], alternative ids [n][20], their lps [n][20], the bound's scale per entry
    [n] from the page's traced logits)."""
    p = DecodeParameters(max_new_tokens=max_new, **kw)
    ids, lp, ti, tl = engine.generate_logprobs([pages[i]], 20, p)
    _, logits = engine.generate_trace([pages[i]], p)
    scale = np.array([ref_logprobs(logits[0][t], ids[0][t], 0)[3] for t in range(len(ids[0]))])
    return ids[0], lp[0], ti[0], tl[0], scale


def _close(a, b, scale):
    """Two runs of the same page whose logits differ in the last bits (another n: another GEMV form): every entry
    within the kernel bound at its own scale."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    sc = scale if a.ndim == 1 else scale[:, None]
    ratio = float((np.abs(a - b) / (EPS * sc)).max()) if a.size else 0.0
    print(f"session logprob difference: {ratio:.3f} x 2^-23 x scale")
    return ratio <= LP_C


def test_session_logprobs(engine, pages):
    """3 slots.  Page 0 (5 tokens) runs alone, wholly at n = 1: bit-equal to its single-page run.  Pages 1, 2 then
    join (n = 3); page 0 retires, so page 2 moves to slot 0 with a half-filled row; page 3 is admitted late.  Pages
    1-3 step at n = 2..3: entry 0 (the admission's own selection, a single-page prefill) is bit-equal, the rest is
    held within the bound."""
    max_new = {0: 5, 1: 20, 2: 12, 3: 10}
    single = {i: _single_lp(engine, pages, i, m) for i, m in max_new.items()}
    need = max(len(pages[i][0]) + m + 1 for i, m in max_new.items())
    got = {}
    with engine.open_session(3, need + 16, DecodeParameters(max_new_tokens=20), logprobs=True) as sess:
        assert sess.info()["flags"] == 2

        def read(slot, key, n):
            got[key] = sess.logprobs(slot, 0, n, 20)

        assert sess.admit(*pages[0][:3], max_new_tokens=5, logprobs=20) == 0
        st = sess.step(8)
        assert st[0].done and st[0].out_len == 5
        assert sess.admit(*pages[1][:3], max_new_tokens=20) == 1
        assert sess.admit(*pages[2][:3], max_new_tokens=12) == 2
        sess.step(4)
        mid = sess.logprobs(1, 1, 3, 5)  # a range read mid-run
        _einval(sess.logprobs, 1, 3, 4, 5)    # out_len is 5: [3, 7) passes it
        _einval(sess.logprobs, 1, 6, 0, 5)
        _einval(sess.logprobs, 1, 0, 1, 21)
        read(0, 0, 5)
        ids0, moved = sess.retire(0)
        assert moved == 2 and ids0 == single[0][0]
        half = sess.logprobs(0, 0, 5, 20)  # page 2, now in slot 0, with the entries it brought along
        assert sess.admit(*pages[3][:3], max_new_tokens=10) == 2
        owner = {0: 2, 1: 1, 2: 3}
        sess.step(8)   # page 2 done (12), page 3 has 9, page 1 has 13
        sess.step(8)
        st = sess.poll()
        assert all(s.done for s in st)
        end = sess.logprobs(1, 1, 3, 5)
        for a, b in zip(mid, end):
            assert a.tobytes() == b.tobytes()
        for slot, key in owner.items():
            read(slot, key, max_new[key])
        for a, b in zip(half, got[2]):
            assert a.tobytes() == b[:5].tobytes()
        ids = {}
        for slot in (2, 1, 0):
            ids[owner[slot]], _ = sess.retire(slot)
        hs = sess.head_steps()
        assert hs["screened"] == 0 and hs["exact"] > 0
    for a, b in zip(got[0], single[0][1:4]):
        assert a.tobytes() == b.tobytes()          # page 0: every step at n = 1
    for key in (1, 2, 3):
        sid, slp, sti, stl, sc = single[key]
        assert ids[key] == sid
        lp, ti, tl = got[key]
        assert lp[0].tobytes() == slp[0].tobytes() and np.array_equal(ti[0], sti[0]) and tl[0].tobytes() == stl[0].tobytes()
        assert _close(lp, slp, sc) and _close(tl, stl, sc)


def test_session_without_flag(engine, pages):
    """A session opened without the flag: reading is EINVAL, and an all-greedy workload runs no exact step."""
    need = len(pages[0][0]) + 8 + 1
    with engine.open_session(2, need, DecodeParameters(max_new_tokens=8)) as sess:
        assert sess.info()["flags"] == 0
        sess.admit(*pages[0][:3], max_new_tokens=8)
        sess.step(8)
        _einval(sess.logprobs, 0, 0, 1, 0)
        _einval(sess.admit, *pages[1][:3], max_new_tokens=8, logprobs=3)
        hs = sess.head_steps()
        assert hs["exact"] == 0


def test_session_per_request_logprobs(engine, pages):
    """The flag with DSOCR_SESSION_PER_REQUEST: one greedy and one sampled slot (n = 2)."""
    greedy = DecodeParameters(max_new_tokens=10)
    sampled = DecodeParameters(max_new_tokens=10, do_sample=True, temperature=0.8, top_p=0.9, seed=5)
    s0 = _single_lp(engine, pages, 0, 10)
    s1 = _single_lp(engine, pages, 1, 10, do_sample=True, temperature=0.8, top_p=0.9, seed=5)
    need = max(len(pages[i][0]) for i in (0, 1)) + 11
    with engine.open_session(2, need, greedy, per_request=True, logprobs=True) as sess:
        assert sess.info()["flags"] == 3
        sess.admit(*pages[0][:3], params=greedy)
        sess.admit(*pages[1][:3], params=sampled)
        sess.step(8)
        sess.step(8)
        g0, g1 = sess.logprobs(0, 0, 10, 20), sess.logprobs(1, 0, 10, 20)
        ids1, _ = sess.retire(1)
        ids0, _ = sess.retire(0)
        assert sess.head_steps()["screened"] == 0
    assert ids0 == s0[0] and ids1 == s1[0]
    for got, ref in ((g0, s0), (g1, s1)):
        assert got[0][0].tobytes() == ref[1][0].tobytes()
        assert _close(got[0], ref[1], ref[4]) and _close(got[2], ref[3], ref[4])


def test_nothing_moves_with_the_flag_off(engine, pages):
    """generate without log-probabilities: the same ids and decode steps before and after a log-probability call."""
    p = DecodeParameters(max_new_tokens=12)
    a = engine.generate(*pages[0], p, ignore_eos=True)
    steps_a = engine.last_timings()["decode_steps"]
    engine.generate_logprobs(pages[:1], 20, p)
    b = engine.generate(*pages[0], p, ignore_eos=True)
    assert a == b and steps_a == engine.last_timings()["decode_steps"] == 11
