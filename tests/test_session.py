"""Decode sessions on the GPU: pages join and leave a running batch between decode steps.

Contract: every page's ids equal ``engine.generate`` of that page alone with the same parameters and seed, whatever
joined, left or moved around it; ``session_slot_move`` copies one slot's state bit for bit and writes nothing else.
Tiny config, the pages and prompt of tests/test_gpu_model.py.
"""
import ctypes as C
import os

import numpy as np
import pytest

from dsocr import DecodeParameters, DsocrError, ModelLoadArgs, Page, VisionSettings, build_prompt_tokens, load_model
from dsocr._lib import check, lib
from dsocr.scheduler import BatchScheduler
from dsocr.synth import SyntheticTokenizer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, "deepseek-ocr.rs_amd", "dsocr", "configs", "tiny.json")
TINY_VS = VisionSettings(256, 128, True)
SEED = 7
PROMPT = "<image>\nConvert the document to markdown."
SIZES = [(300, 420), (256, 256), (500, 140), (130, 130), (120, 500)]


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


def _need(pages, idx, max_new):
    return max(len(pages[i][0]) + m + 1 for i, m in zip(idx, max_new))


def _drain(sess, owner, out, burst=8):
    """Steps until every active page is retired.  owner[slot] = page key; retires at every burst boundary."""
    guard = 0
    while owner:
        status = sess.step(burst)
        for st in sorted(status, key=lambda s: -s.slot):
            if st.done:
                ids, moved = sess.retire(st.slot)
                out[owner[st.slot]] = ids
                last = len(owner) - 1
                assert moved == (-1 if st.slot == last else last)
                if moved >= 0:
                    owner[st.slot] = owner[last]
                owner.pop()
        guard += 1
        assert guard < 200
    return out


# ------------------------------------------------------------------ the move kernel alone
@pytest.mark.parametrize("kv_len", [1, 17, 40])
def test_slot_move_kernel(gpu, kv_len):
    layers, S, kvh, hd, cap = 2, 3, 2, 128, 40
    ctx_cap, out_cap, ban_ld, rng_words, H = 48, 12, 49, 80, 96
    rng = np.random.default_rng(kv_len)
    L = lib()
    host = {
        "kc": rng.standard_normal((layers, S, kvh, cap, hd)).astype(np.float32),
        "vc": rng.standard_normal((layers, S, kvh, cap, hd)).astype(np.float32),
        "kv_len": np.array([5, 9, kv_len], np.int32),
        "kv_pos": np.array([4, 8, kv_len - 1], np.int32),
        "ctx": rng.integers(0, 500, (S, ctx_cap)).astype(np.int32),
        "ctx_len": np.array([11, 12, 13], np.int32),
        "out": rng.integers(0, 500, (S, out_cap)).astype(np.int32),
        "out_len": np.array([1, 2, 3], np.int32),
        "done": np.array([1, 0, 0], np.int32),
        "tok": np.array([7, 8, 9], np.int32),
        "rng": rng.integers(0, 2 ** 32, (S, rng_words), dtype=np.uint64).astype(np.uint32),
        "ban": rng.integers(0, 500, (S, ban_ld)).astype(np.int32),
        "x": rng.standard_normal((S, H)).astype(np.float32),
    }
    dev = {}
    try:
        for k, a in host.items():
            p = C.c_void_p()
            check(L.dsocr_dev_alloc(a.nbytes, C.byref(p)))
            dev[k] = p
            check(L.dsocr_memcpy_h2d(p, a.ctypes.data_as(C.c_void_p), a.nbytes))
        d = dev
        check(L.dsocr_k_session_slot_move(layers, S, kvh, cap, hd, d["kc"], d["vc"], d["kv_len"], d["kv_pos"], d["ctx"],
                                          ctx_cap, d["ctx_len"], d["out"], out_cap, d["out_len"], d["done"], d["tok"],
                                          d["rng"], rng_words, d["ban"], ban_ld, d["x"], H, 2, 0))
        got = {}
        for k, a in host.items():
            got[k] = np.empty_like(a)
            check(L.dsocr_memcpy_d2h(got[k].ctypes.data_as(C.c_void_p), dev[k], a.nbytes))
        # the same slot twice and a slot outside the session are refused before any launch
        for src, dst in ((1, 1), (3, 0), (0, -1)):
            assert L.dsocr_k_session_slot_move(layers, S, kvh, cap, hd, d["kc"], d["vc"], d["kv_len"], d["kv_pos"],
                                               d["ctx"], ctx_cap, d["ctx_len"], d["out"], out_cap, d["out_len"],
                                               d["done"], d["tok"], d["rng"], rng_words, d["ban"], ban_ld, d["x"], H,
                                               src, dst) == 1
    finally:
        for p in dev.values():
            L.dsocr_dev_free(p)
    for k in ("kc", "vc"):
        assert np.array_equal(got[k][:, 0, :, :kv_len], host[k][:, 2, :, :kv_len]), k   # moved rows
        assert np.array_equal(got[k][:, 0, :, kv_len:], host[k][:, 0, :, kv_len:]), k   # rows past kv_len untouched
        assert np.array_equal(got[k][:, 1:], host[k][:, 1:]), k                         # slot 1 and the source
    for k in ("kv_len", "kv_pos", "ctx", "ctx_len", "out", "out_len", "done", "tok", "rng", "ban", "x"):
        assert np.array_equal(got[k][0], host[k][2]), k
        assert np.array_equal(got[k][1:], host[k][1:]), k


# ------------------------------------------------------------------ sessions
def test_session_equals_single(engine, pages):
    idx, max_new = [0, 1, 2, 3], [8, 24, 40, 16]
    singles = [_single(engine, pages, i, m) for i, m in zip(idx, max_new)]
    with engine.open_session(4, _need(pages, idx, max_new), DecodeParameters(max_new_tokens=40)) as sess:
        info = sess.info()
        assert (info["slots"], info["active"], info["out_cap"]) == (4, 0, 40)
        assert info["kv_cap"] == info["max_context"] + info["burst_cap"]
        for n, (i, m) in enumerate(zip(idx, max_new)):
            assert sess.admit(*pages[i], max_new_tokens=m) == n
        assert sess.info()["active"] == 4
        first = sess.poll()
        assert [s.new_tokens for s in first] == [s[:1] for s in singles]
        out = _drain(sess, list(range(4)), {})
        assert sess.info()["active"] == 0
    assert [out[k] for k in range(4)] == singles


def test_late_admit(engine, pages):
    """Prefill into a live cache; the step graphs for n = 2, 3, 4."""
    idx, max_new = [0, 1, 2, 3], [24, 30, 20, 16]
    singles = [_single(engine, pages, i, m) for i, m in zip(idx, max_new)]
    out = {}
    with engine.open_session(4, _need(pages, idx, max_new), DecodeParameters(max_new_tokens=30)) as sess:
        sess.admit(*pages[0], max_new_tokens=24)
        sess.admit(*pages[1], max_new_tokens=30)
        assert not any(s.done for s in sess.step(5))
        assert sess.admit(*pages[2], max_new_tokens=20) == 2
        assert not any(s.done for s in sess.step(3))
        assert sess.admit(*pages[3], max_new_tokens=16) == 3
        _drain(sess, [0, 1, 2, 3], out)
    assert [out[k] for k in range(4)] == singles


@pytest.mark.parametrize("max_new", [[6, 30, 30], [6, 12, 30]])
def test_retire_and_compact(engine, pages, max_new):
    """Slot 0 finishes first: slot 2 moves into it and n = 2; in the second case n then drops to 1 and the one-page
    kernels finish the last page."""
    idx = [0, 1, 2]
    singles = [_single(engine, pages, i, m) for i, m in zip(idx, max_new)]
    if any(len(s) < m for s, m in zip(singles, max_new)):
        pytest.fail("the tiny pages are expected to run to max_new (no early eos): pick other pages")
    out, owner = {}, [0, 1, 2]
    with engine.open_session(3, _need(pages, idx, max_new), DecodeParameters(max_new_tokens=30)) as sess:
        for i, m in zip(idx, max_new):
            sess.admit(*pages[i], max_new_tokens=m)
        st = sess.step(5)  # 1 + 5 tokens: page 0 (max_new 6) is done
        assert [s.done for s in st] == [True, False, False]
        ids, moved = sess.retire(0)
        assert (ids, moved) == (singles[0], 2)
        assert sess.info()["active"] == 2
        owner = [2, 1]
        seen_active = set()
        while owner:
            status = sess.step(8)
            seen_active.add(len(status))
            for s in sorted(status, key=lambda s: -s.slot):
                if s.done:
                    got, mv = sess.retire(s.slot)
                    out[owner[s.slot]] = got
                    if mv >= 0:
                        owner[s.slot] = owner[mv]
                    owner.pop()
        assert seen_active == ({2} if max_new[1] == max_new[2] else {1, 2})
    assert [out[1], out[2]] == singles[1:]


def test_slot_reuse_through_scheduler(engine, pages):
    tok = SyntheticTokenizer(512)
    max_new = [12, 20, 8, 16, 10]
    singles = [_single(engine, pages, i, m) for i, m in enumerate(max_new)]
    imgs = [_img(100 + i, *hw) for i, hw in enumerate(SIZES)]
    need = _need(pages, range(5), max_new)
    with BatchScheduler(engine, tok, 2, need, DecodeParameters(max_new_tokens=20), TINY_VS) as sched:
        futs = [sched.submit(PROMPT, [im], params=DecodeParameters(max_new_tokens=m)) for im, m in zip(imgs, max_new)]
        outs = [f.result(timeout=120) for f in futs]
        assert sched.max_active == 2
        assert all(n <= 2 for n, _ in sched.bursts)
    assert [o.generated_tokens for o in outs] == singles
    # the scheduler closed its session: the engine serves generate again
    assert _single(engine, pages, 0, 12) == engine.generate(*pages[0], None, DecodeParameters(max_new_tokens=12))


def test_sampling_with_seeds(engine, pages):
    kw = dict(do_sample=True, temperature=0.7, top_p=0.9, top_k=40)
    idx, max_new, seeds = [0, 1, 2], [12, 20, 16], [11, 12, 13]
    singles = [_single(engine, pages, i, m, seed=s, **kw) for i, m, s in zip(idx, max_new, seeds)]
    out = {}
    with engine.open_session(3, _need(pages, idx, max_new), DecodeParameters(max_new_tokens=20, **kw)) as sess:
        for i, m, s in zip(idx, max_new, seeds):
            sess.admit(*pages[i], max_new_tokens=m, seed=s)
        _drain(sess, [0, 1, 2], out)
    assert [out[k] for k in range(3)] == singles


def test_streaming_two_requests(engine, pages):
    tok = SyntheticTokenizer(512)
    max_new = [9, 14]
    singles = [_single(engine, pages, i, m) for i, m in enumerate(max_new)]
    imgs = [_img(100 + i, *SIZES[i]) for i in range(2)]
    seen = [[], []]
    with BatchScheduler(engine, tok, 2, _need(pages, [0, 1], max_new), DecodeParameters(max_new_tokens=14),
                        TINY_VS) as sched:
        futs = [sched.submit(PROMPT, [imgs[i]], params=DecodeParameters(max_new_tokens=max_new[i]),
                             on_token=lambda n, ids, i=i: seen[i].append((n, list(ids)))) for i in range(2)]
        outs = [f.result(timeout=120) for f in futs]
        assert all(b == 1 for _, b in sched.bursts)
    for i in range(2):
        assert outs[i].generated_tokens == singles[i]
        assert [n for n, _ in seen[i]] == list(range(1, len(singles[i]) + 1))
        assert all(ids == singles[i][:n] for n, ids in seen[i])


def test_errors_leave_the_running_slots_alone(engine, pages):
    idx, max_new = [0, 1], [20, 24]
    singles = [_single(engine, pages, i, m) for i, m in zip(idx, max_new)]
    before = _single(engine, pages, 2, 8)
    out = {}
    sess = engine.open_session(3, _need(pages, idx, max_new), DecodeParameters(max_new_tokens=24))
    try:
        with pytest.raises(DsocrError) as e:
            engine.open_session(2, 64, DecodeParameters(max_new_tokens=8))
        assert e.value.status == 1
        sess.admit(*pages[0], max_new_tokens=20)
        sess.admit(*pages[1], max_new_tokens=24)
        sess.step(4)
        ids, mask, page = pages[2]
        bad = list(mask)
        bad[-1] = 1  # one extra <image> slot
        with pytest.raises(DsocrError) as e:
            sess.admit(ids, bad, page, max_new_tokens=8)
        assert e.value.status == 1 and "mismatch" in e.value.message
        bad_ids = list(ids)
        bad_ids[-1] = engine.vocab
        with pytest.raises(DsocrError) as e:
            sess.admit(bad_ids, mask, page, max_new_tokens=8)
        assert e.value.status == 1 and "out of bounds" in e.value.message
        with pytest.raises(DsocrError) as e:
            engine.generate(ids, mask, page, None, DecodeParameters(max_new_tokens=8))
        assert e.value.status == 1 and "session" in e.value.message
        assert sess.info()["active"] == 2
        _drain(sess, [0, 1], out)
    finally:
        sess.close()
    assert [out[0], out[1]] == singles
    ids, mask, page = pages[2]
    assert engine.generate(ids, mask, page, None, DecodeParameters(max_new_tokens=8)) == before


def test_capacity(engine, pages):
    """One row short is EINVAL at admit; max_context exactly the largest need, burst 8, completes."""
    idx, max_new = [0, 1, 2], [10, 21, 13]
    singles = [_single(engine, pages, i, m) for i, m in zip(idx, max_new)]
    need = _need(pages, idx, max_new)
    out = {}
    with engine.open_session(3, need - 1, DecodeParameters(max_new_tokens=21)) as sess:
        big = max(idx, key=lambda i: len(pages[i][0]) + max_new[i])
        with pytest.raises(DsocrError) as e:
            sess.admit(*pages[big], max_new_tokens=max_new[big])
        assert e.value.status == 1 and "context" in e.value.message
        assert sess.info()["active"] == 0
    with engine.open_session(3, need, DecodeParameters(max_new_tokens=21)) as sess:
        for i, m in zip(idx, max_new):
            sess.admit(*pages[i], max_new_tokens=m)
        _drain(sess, [0, 1, 2], out, burst=8)
    assert [out[k] for k in range(3)] == singles
