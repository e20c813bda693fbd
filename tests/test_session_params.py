"""Per-request decode parameters in a decode session (DSOCR_SESSION_PER_REQUEST) on the GPU.

Contract: every page's ids equal ``engine.generate`` of that page alone with that page's parameters and seed,
whatever else is in the batch, whichever lm_head + selection head a burst ran under.  Every expected value is
computed outside any session.  Tiny config, the pages and prompt of tests/test_session.py.
"""
import ctypes as C
import os

import numpy as np
import pytest

from dsocr import DecodeParameters, DsocrError, ModelLoadArgs, Page, VisionSettings, build_prompt_tokens, load_model
from dsocr._lib import RowParamsC, check, lib
from dsocr.scheduler import BatchScheduler
from dsocr.synth import SyntheticTokenizer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, "deepseek-ocr.rs_amd", "dsocr", "configs", "tiny.json")
TINY_VS = VisionSettings(256, 128, True)
SEED = 7
PROMPT = "<image>\nConvert the document to markdown."
SIZES = [(300, 420), (256, 256), (500, 140), (130, 130), (120, 500)]

# the parameter sets of the mixed cases (beside the default greedy one)
GREEDY_PEN = dict(repetition_penalty=1.3, no_repeat_ngram_size=3)
GREEDY_BAN = dict(no_repeat_ngram_size=2)
TOPK = dict(do_sample=True, temperature=0.7, top_k=5)
TOPP = dict(do_sample=True, temperature=1.3, top_p=0.9)


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


_SINGLES = {}


def _single(engine, pages, i, max_new, **kw):
    """engine.generate of page i alone: computed once per (page, parameters), outside any session."""
    key = (i, max_new, tuple(sorted(kw.items())))
    if key not in _SINGLES:
        ids, mask, page = pages[i]
        _SINGLES[key] = engine.generate(ids, mask, page, None, DecodeParameters(max_new_tokens=max_new, **kw))
    return _SINGLES[key]


def _differs_from_default(engine, pages, i, max_new, **kw):
    """The precondition of the mixed cases: page i's own parameters change its stream (else the case shows nothing)."""
    if _single(engine, pages, i, max_new, **kw) == _single(engine, pages, i, max_new):
        pytest.fail(f"pick other parameters: page {i} with {kw} decodes like default greedy")


def _need(pages, idx, max_new):
    return max(len(pages[i][0]) + m + 1 for i, m in zip(idx, max_new))


def _retire_done(sess, status, owner, out):
    for st in sorted(status, key=lambda s: -s.slot):
        if st.done:
            ids, moved = sess.retire(st.slot)
            out[owner[st.slot]] = ids
            last = len(owner) - 1
            assert moved == (-1 if st.slot == last else last)
            if moved >= 0:
                owner[st.slot] = owner[last]
            owner.pop()


def _drain(sess, owner, out, burst=8):
    """Steps until every active page is retired.  owner[slot] = page key; retires at every burst boundary."""
    guard = 0
    while owner:
        _retire_done(sess, sess.step(burst), owner, out)
        guard += 1
        assert guard < 200
    return out


# ------------------------------------------------------------------ 1. the kernel hook: per row against scalar
def _hook_rows():
    rng = np.random.default_rng(517)
    V, cap = 517, 32
    lens = [0, 5, 31, 12, 9]
    B = len(lens)
    logits = (rng.standard_normal((B, V)) * 3).astype(np.float32)
    logits[2, 5] = -np.inf
    logits[3, 7] = np.nan
    ctx = np.zeros((B, cap), np.int32)
    for b in range(B - 1):
        base = rng.integers(0, 40, 3)
        seq = np.tile(base, 12)[: lens[b]]
        ctx[b, : lens[b]] = seq
        logits[b, seq] += 4.0  # the repeated tokens are the likely picks: the ban and the penalty matter
    # the last row: everything non-finite but one token, and the n-gram ban (size 2 after ... 7) bans that one
    ctx[4, :9] = [7, 9, 7, 9, 7, 9, 7, 9, 7]
    logits[4, :] = -np.inf
    logits[4, 100:120] = np.nan
    logits[4, 9] = 1.0
    rows = [
        dict(do_sample=0, temperature=0.0, top_p=-1.0, top_k=0, pen=1.0, ngram=0),
        dict(do_sample=0, temperature=0.0, top_p=-1.0, top_k=0, pen=1.3, ngram=3),
        dict(do_sample=1, temperature=0.7, top_p=-1.0, top_k=5, pen=1.0, ngram=2),
        dict(do_sample=1, temperature=1.3, top_p=0.9, top_k=0, pen=1.1, ngram=0),
        dict(do_sample=0, temperature=0.0, top_p=-1.0, top_k=0, pen=1.0, ngram=2),
    ]
    seeds = [0, 0, 4242, 777, 0]
    return V, cap, logits, ctx, np.array(lens, np.int32), rows, seeds


@pytest.fixture(scope="module")
def hook_reference(gpu):
    """Every row alone (B = 1) through the scalar hooks: [draws] ids per row, computed once."""
    from _dev import Dev
    V, cap, logits, ctx, lens, rows, seeds = _hook_rows()
    draws, L, ref = 3, lib(), []
    for b, r in enumerate(rows):
        dl, dc, dn = Dev(logits[b:b + 1]), Dev(ctx[b:b + 1]), Dev(lens[b:b + 1])
        if r["do_sample"]:
            dt = Dev.zeros(draws, np.int32)
            check(L.dsocr_k_sample_stoch(1, V, dl.ptr, dc.ptr, cap, dn.ptr, r["ngram"], r["pen"], r["temperature"],
                                         r["top_k"], r["top_p"], seeds[b], draws, dt.ptr))
            ref.append(dt.get().tolist())
        else:
            dt = Dev.zeros(1, np.int32)
            check(L.dsocr_k_sample_greedy(1, V, dl.ptr, dc.ptr, cap, dn.ptr, r["ngram"], r["pen"], dt.ptr))
            ref.append(dt.get().tolist() * draws)
    return ref


@pytest.mark.parametrize("order", [[0, 1, 2, 3, 4], [4, 3, 2, 1, 0]], ids=["forward", "reversed"])
def test_select_rows_equals_the_scalar_hooks(gpu, hook_reference, order):
    from _dev import Dev
    V, cap, logits, ctx, lens, rows, seeds = _hook_rows()
    B, draws = len(order), 3
    assert hook_reference[4] == [9] * draws  # the all-banned row: the final kernel's fallback ignores the ban
    assert len(set(hook_reference[2])) > 1 or len(set(hook_reference[3])) > 1  # the draws do move
    rp = (RowParamsC * B)()
    sd = (C.c_uint64 * B)()
    for j, b in enumerate(order):
        r = rows[b]
        rp[j] = RowParamsC(r["do_sample"], r["temperature"], r["top_p"], r["top_k"], r["pen"], r["ngram"], -1)
        sd[j] = seeds[b]
    dl, dc, dn = Dev(logits[order]), Dev(ctx[order]), Dev(lens[order])
    dt = Dev.zeros(draws * B, np.int32)
    check(lib().dsocr_k_select_rows(B, V, dl.ptr, dc.ptr, cap, dn.ptr, rp, sd, draws, dt.ptr))
    got = dt.get().reshape(draws, B)
    for j, b in enumerate(order):
        assert got[:, j].tolist() == hook_reference[b], (j, b, got[:, j].tolist(), hook_reference[b])


# ------------------------------------------------------------------ 2. a mixed session equals the singles
def test_mixed_session_equals_singles(engine, pages):
    idx, max_new = [0, 1, 2, 3], [16, 40, 24, 32]
    kws = [dict(), GREEDY_PEN, dict(seed=11, **TOPK), dict(seed=12, **TOPP)]
    singles = [_single(engine, pages, i, m, **kw) for i, m, kw in zip(idx, max_new, kws)]
    for i, m, kw in zip(idx[1:], max_new[1:], kws[1:]):
        _differs_from_default(engine, pages, i, m, **kw)
    with engine.open_session(4, _need(pages, idx, max_new), DecodeParameters(max_new_tokens=40),
                             per_request=True) as sess:
        for n, (i, m, kw) in enumerate(zip(idx, max_new, kws)):
            assert sess.admit(*pages[i], params=DecodeParameters(max_new_tokens=m, **kw)) == n
        first = sess.poll()
        assert [s.new_tokens for s in first] == [s[:1] for s in singles]
        out = _drain(sess, list(range(4)), {})
        hs = sess.head_steps()
        assert hs["screened"] + hs["exact"] == sess.info()["steps"]
    assert [out[k] for k in range(4)] == singles


# ------------------------------------------------------------------ 3. the head follows the traffic
def _fixed_greedy_is_screened(engine, pages):
    with engine.open_session(1, _need(pages, [3], [4]), DecodeParameters(max_new_tokens=4, **GREEDY_BAN)) as sess:
        sess.admit(*pages[3], max_new_tokens=4)
        sess.step(1)
        return sess.head_steps()["screened"] == 1


def test_head_switch_hands_the_ban_list_over(engine, pages):
    """Greedy A, B run screened; a sampled page C joins: exact; C and A leave (B moves into slot 0): screened again.
    B's n-gram ban list crosses both switches."""
    screenable = _fixed_greedy_is_screened(engine, pages)
    idx, max_new = [0, 1, 2], [12, 40, 6]
    kws = [GREEDY_BAN, GREEDY_BAN, dict(seed=5, **TOPP)]
    singles = [_single(engine, pages, i, m, **kw) for i, m, kw in zip(idx, max_new, kws)]
    for i, m, kw in zip(idx, max_new, kws):
        _differs_from_default(engine, pages, i, m, **kw)
    if any(len(s) < m for s, m in zip(singles, max_new)):
        pytest.fail("the tiny pages are expected to run to max_new (no early eos): pick other pages")
    out, owner = {}, [0, 1]
    with engine.open_session(3, _need(pages, idx, max_new), DecodeParameters(max_new_tokens=40),
                             per_request=True) as sess:
        for i in (0, 1):
            sess.admit(*pages[i], params=DecodeParameters(max_new_tokens=max_new[i], **kws[i]))
        assert not any(s.done for s in sess.step(5))
        assert sess.head_steps() == ({"screened": 5, "exact": 0} if screenable else {"screened": 0, "exact": 5})
        assert sess.admit(*pages[2], params=DecodeParameters(max_new_tokens=6, **kws[2])) == 2
        owner.append(2)
        st = sess.step(8)  # C has 1 + 8 >= 6 tokens, A 1 + 13 >= 12, B 14 of 40
        assert [s.done for s in st] == [True, False, True]
        assert sess.head_steps()["exact"] == (8 if screenable else 13)
        _retire_done(sess, st, owner, out)  # C leaves slot 2, then A leaves slot 0 and B moves into it
        assert owner == [1] and sess.info()["active"] == 1
        _drain(sess, owner, out)
        hs, steps = sess.head_steps(), sess.info()["steps"]
        assert hs["screened"] + hs["exact"] == steps
        assert hs["exact"] == (8 if screenable else steps)
    assert [out[k] for k in range(3)] == singles


# ------------------------------------------------------------------ 4. a slot move carries the row and the RNG
def test_move_carries_the_row(engine, pages):
    idx, max_new = [0, 1, 2], [6, 30, 30]
    kws = [dict(), GREEDY_PEN, dict(seed=21, **TOPK)]
    singles = [_single(engine, pages, i, m, **kw) for i, m, kw in zip(idx, max_new, kws)]
    _differs_from_default(engine, pages, 2, 30, **kws[2])
    if any(len(s) < m for s, m in zip(singles, max_new)):
        pytest.fail("the tiny pages are expected to run to max_new (no early eos): pick other pages")
    out = {}
    with engine.open_session(3, _need(pages, idx, max_new), DecodeParameters(max_new_tokens=30),
                             per_request=True) as sess:
        for i, m, kw in zip(idx, max_new, kws):
            sess.admit(*pages[i], params=DecodeParameters(max_new_tokens=m, **kw))
        st = sess.step(5)
        assert [s.done for s in st] == [True, False, False]
        ids, moved = sess.retire(0)
        assert (ids, moved) == (singles[0], 2)  # the sampled page now lives in slot 0
        _drain(sess, [2, 1], out)
    assert [out[1], out[2]] == singles[1:]


# ------------------------------------------------------------------ 5. eos per request
def test_eos_per_request(engine, pages):
    max_new = 20
    plain = [_single(engine, pages, i, max_new) for i in (0, 1)]
    # a token page 1's own stream emits mid-stream for the first time
    j = next((k for k in range(2, len(plain[1]) - 1) if plain[1][k] not in plain[1][:k]), None)
    if j is None:
        pytest.fail("pick another page: its stream has no first occurrence mid-stream")
    eos = plain[1][j]
    if len(plain[0]) < max_new:
        pytest.fail("the tiny pages are expected to run to max_new (no early eos): pick other pages")
    saved = engine.eos_token_id
    try:
        engine.eos_token_id = eos
        ids, mask, page = pages[1]
        stopped = engine.generate(ids, mask, page, None, DecodeParameters(max_new_tokens=max_new))
    finally:
        engine.eos_token_id = saved
    assert stopped == plain[1][:j]
    out = {}
    with engine.open_session(2, _need(pages, [0, 1], [max_new] * 2), DecodeParameters(max_new_tokens=max_new),
                             per_request=True) as sess:
        # page 0 would stop at its own third token if that eos counted
        sess.admit(*pages[0], params=DecodeParameters(max_new_tokens=max_new), eos_token_id=plain[0][2], ignore_eos=True)
        sess.admit(*pages[1], params=DecodeParameters(max_new_tokens=max_new), eos_token_id=eos)
        _drain(sess, [0, 1], out)
    assert out[0] == plain[0] and out[1] == stopped


# ------------------------------------------------------------------ 6. errors
def test_errors(engine, pages):
    idx, max_new = [0, 1], [20, 16]
    singles = [_single(engine, pages, 0, 20), _single(engine, pages, 1, 16)]
    screenable = _fixed_greedy_is_screened(engine, pages)
    out = {}
    # a fixed session refuses foreign parameters and its running slots go on
    with engine.open_session(3, _need(pages, [0, 1, 2], [20, 16, 24]), DecodeParameters(max_new_tokens=24)) as sess:
        sess.admit(*pages[0], max_new_tokens=20)
        assert sess.admit(*pages[1], params=DecodeParameters(max_new_tokens=16, seed=3)) == 1  # only max_new / seed
        sess.step(3)
        with pytest.raises(DsocrError) as e:
            sess.admit(*pages[2], params=DecodeParameters(max_new_tokens=8, do_sample=True, temperature=0.7))
        assert e.value.status == 1 and "fixed" in e.value.message
        assert sess.info()["active"] == 2
        _drain(sess, [0, 1], out)
    assert [out[0], out[1]] == singles
    out = {}
    with engine.open_session(2, _need(pages, idx, max_new), DecodeParameters(max_new_tokens=20),
                             per_request=True) as sess:
        sess.admit(*pages[0], params=DecodeParameters(max_new_tokens=20))
        steps = sess.info()["steps"]
        with pytest.raises(DsocrError) as e:  # above the session's output capacity: before any launch
            sess.admit(*pages[1], params=DecodeParameters(max_new_tokens=21))
        assert e.value.status == 1 and "max_new_tokens" in e.value.message
        with pytest.raises(DsocrError) as e:
            sess.admit(*pages[1], params=DecodeParameters(max_new_tokens=16, use_cache=False))
        assert e.value.status == 1
        assert sess.info()["active"] == 1 and sess.info()["steps"] == steps
        # do_sample without a temperature is greedy (sampling.rs:67)
        sess.admit(*pages[1], params=DecodeParameters(max_new_tokens=16, do_sample=True, temperature=0.0, seed=9))
        _drain(sess, [0, 1], out)
        if screenable:  # greedy traffic without a penalty never leaves the screened head
            assert sess.head_steps()["exact"] == 0
    assert [out[0], out[1]] == singles


# ------------------------------------------------------------------ 7. the scheduler
def test_scheduler_admits_mixed_parameters(engine, pages):
    tok = SyntheticTokenizer(512)
    max_new = [12, 20, 8, 16, 10]
    kws = [dict(), GREEDY_PEN, dict(seed=31, **TOPK), dict(), dict(seed=32, **TOPP)]
    singles = [_single(engine, pages, i, m, **kw) for i, (m, kw) in enumerate(zip(max_new, kws))]
    imgs = [_img(100 + i, *hw) for i, hw in enumerate(SIZES)]
    need = _need(pages, range(5), max_new)
    with BatchScheduler(engine, tok, 2, need, DecodeParameters(max_new_tokens=20), TINY_VS,
                        per_request_params=True) as sched:
        futs = [sched.submit(PROMPT, [im], params=DecodeParameters(max_new_tokens=m, **kw))
                for im, m, kw in zip(imgs, max_new, kws)]
        outs = [f.result(timeout=120) for f in futs]
        assert sched.max_active == 2 and sched.exclusive_runs == 0
        assert all(n <= 2 for n, _ in sched.bursts)
    assert [o.generated_tokens for o in outs] == singles
