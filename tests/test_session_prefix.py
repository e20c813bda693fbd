"""Page prefix cache on the GPU: the copy kernel through its hook, prefix admission against plain admission, the
life cycle of entries and slots, the statistics, every refusal, and the scheduler.

Tiny config; the page is prepared at base 512 / tiles 256, which gives it 177 image rows: its prefix (BOS + the image
rows, 178 rows) spans two 128-key pieces of launch_attention_past and six of its 32-key waves.

Prefix admission against plain admission of the same prompt (test_prefix_admission_equals_plain): the emitted ids are
equal over all 24 steps, and the token log-probabilities agree within LP_BAR.  The two differ only in the prefill of
the suffix rows (attention over key pieces of 32 with a combine, against the causal prefill's order; GEMMs on 7 rows
against 185), so the bar is measured, not guessed: the worst |delta| over this test's three suffixes on an MI355X was
4.768e-7 (WORST_MEASURED: two ulps of a log-probability near -2), and LP_BAR = 1.907e-6 is four times that (DESIGN
4.12's convention); both are far below the project's 2e-3 logit bar.  Before ids are compared the plain run's
top-1 / top-2 gap is asserted to exceed LP_BAR at every step (its smallest over the three suffixes was 5.5e-4), so no
step's argmax can turn on a difference the bar allows.

"The same entry bytes" (test_keep_after_decoding) is checked through what the bytes determine: two admissions of one
prompt, behind an entry kept right after the admission and behind one kept from the same slot ten steps later, give
bit-equal log-probability rows."""
import ctypes as C
import os

import numpy as np
import pytest

from _dev import Dev
from dsocr import DecodeParameters, DsocrError, ModelLoadArgs, Page, VisionSettings, build_prompt_tokens, load_model
from dsocr._lib import EINVAL, check, lib
from dsocr.scheduler import BatchScheduler
from dsocr.synth import SyntheticTokenizer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, "deepseek-ocr.rs_amd", "dsocr", "configs", "tiny.json")
VS = VisionSettings(512, 256, True)
PROMPTS = ["<image>\nConvert the document to markdown.", "<image>\nFree OCR.", "<image>\nParse the figure.",
           "<image>\nLocate the title in the image."]
MAX_NEW = 24
WORST_MEASURED = 4.768e-7    # worst |delta logprob| of the three suffixes on an MI355X (see the docstring)
LP_BAR = 4 * WORST_MEASURED  # 1.907e-6: four times the measured worst, far below the project's 2e-3 logit bar


@pytest.fixture(scope="module")
def engine(gpu):
    eng = load_model(ModelLoadArgs(config_path=TINY, synthetic_seed=7, dtype="f16"))
    yield eng
    eng.close()


def _img(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def docs():
    """Two pages, each with the four prompts: docs[page][prompt] = (ids, mask), and the pages' prefix rows."""
    tok = SyntheticTokenizer(512)
    out = []
    for i, hw in enumerate([(300, 420), (500, 500)]):
        page = Page(_img(100 + i, *hw), VS)
        prompts = [build_prompt_tokens(tok, p, [page.n_image_tokens]) for p in PROMPTS]
        rows = max(j for j, m in enumerate(prompts[0][1]) if m) + 1
        assert rows > 128 and all(len(ids) > rows for ids, _ in prompts)
        out.append(dict(page=page, prompts=prompts, rows=rows))
    return out


def _einval(fn, *a, **kw):
    with pytest.raises(DsocrError) as ei:
        fn(*a, **kw)
    assert ei.value.status == EINVAL, ei.value


def _run_slot(sess, slot, steps=MAX_NEW):
    """Steps until `slot` has `steps` tokens or is done; returns its ids so far (every slot of the session steps)."""
    for _ in range(8):
        st = {s.slot: s for s in sess.poll()}
        if st[slot].done or st[slot].out_len >= steps:
            break
        sess.step(8)
    return st[slot].out_len


# ------------------------------------------------------------------ the copy kernel alone
@pytest.mark.parametrize("rows", [1, 3, 12])
def test_prefix_copy_kernel(gpu, rows):
    layers, S, kvh, hd, cap, slot = 2, 3, 2, 32, 12, 1
    rng = np.random.default_rng(rows)
    kc = rng.standard_normal((layers, S, kvh, cap, hd)).astype(np.float32)
    vc = rng.standard_normal((layers, S, kvh, cap, hd)).astype(np.float32)
    n = layers * kvh * rows * hd
    L = lib()
    # slot -> entry: a NaN-filled entry with a tail the copy must not reach
    dk, dv = Dev(kc), Dev(vc)
    de = Dev(np.full(2 * n + 64, np.nan, np.float32))
    check(L.dsocr_k_session_prefix_copy(layers, S, kvh, cap, hd, dk.ptr, dv.ptr, slot, rows, de.ptr, 0))
    e = de.get()
    want = np.concatenate([kc[:, slot, :, :rows].ravel(), vc[:, slot, :, :rows].ravel()])
    assert np.array_equal(e[:2 * n].view(np.uint32), want.view(np.uint32)) and np.isnan(e[2 * n:]).all()
    assert np.array_equal(dk.get(), kc) and np.array_equal(dv.get(), vc)
    # entry -> slot: NaN-filled caches; only rows [0, rows) of the slot are written
    nk, nv = Dev(np.full_like(kc, np.nan)), Dev(np.full_like(vc, np.nan))
    check(L.dsocr_k_session_prefix_copy(layers, S, kvh, cap, hd, nk.ptr, nv.ptr, slot, rows, de.ptr, 1))
    for got, src in ((nk.get(), kc), (nv.get(), vc)):
        assert np.array_equal(got[:, slot, :, :rows].view(np.uint32), src[:, slot, :, :rows].view(np.uint32))
        assert np.isnan(got[:, slot, :, rows:]).all()
        assert np.isnan(got[:, [0, 2]]).all()
    assert np.array_equal(de.get().view(np.uint32), e.view(np.uint32))
    for bad in ((slot, 0), (slot, cap + 1), (S, 1), (-1, 1)):
        assert L.dsocr_k_session_prefix_copy(layers, S, kvh, cap, hd, nk.ptr, nv.ptr, bad[0], bad[1], de.ptr, 1) == EINVAL


# ------------------------------------------------------------------ prefix admission == plain admission
def _admit_and_read(sess, admit):
    slot = admit()
    n = _run_slot(sess, slot)
    lp, ti, tl = sess.logprobs(slot, 0, n, 2)
    ids, _ = sess.retire(slot)
    return ids, lp.copy(), tl.copy()


def test_prefix_admission_equals_plain(engine, docs):
    d = docs[0]
    need = max(len(ids) for ids, _ in d["prompts"]) + MAX_NEW + 1
    worst, min_gap, runs = 0.0, np.inf, []
    with engine.open_session(2, need, DecodeParameters(max_new_tokens=MAX_NEW), ignore_eos=True,
                             logprobs=True) as sess:
        ids0, mask0 = d["prompts"][0]
        assert sess.admit(ids0, mask0, d["page"]) == 0
        h = sess.keep_prefix(0, d["rows"])
        sess.retire(0)  # the entry outlives its source slot; every run below is alone in the session (n = 1)
        for ids, mask in d["prompts"][1:]:
            plain = _admit_and_read(sess, lambda: sess.admit(ids, mask, d["page"]))
            pre = _admit_and_read(sess, lambda: sess.admit_prefix(h, ids, mask))
            assert len(plain[0]) == MAX_NEW
            gap = float(np.min(plain[2][:, 0] - plain[2][:, 1]))
            delta = float(np.max(np.abs(plain[1].astype(np.float64) - pre[1][:len(plain[1])])))
            print(f"prefix admission: worst |d logprob| {delta:.3e}, smallest top-1/top-2 gap of the plain run {gap:.3e}")
            worst, min_gap = max(worst, delta), min(min_gap, gap)
            runs.append((gap, delta, plain[0], pre[0]))
        print(f"prefix admission over 3 suffixes: worst {worst:.3e}, smallest gap {min_gap:.3e}, bar {LP_BAR:.3e}")
        for gap, delta, plain_ids, pre_ids in runs:
            assert gap > LP_BAR, gap
            assert pre_ids == plain_ids
            assert delta <= LP_BAR, delta
        st = sess.prefix_stats()
        assert st["admissions"] == 3 and st["rows_reused"] == 3 * d["rows"] and st["entries"] == 1
    assert LP_BAR == pytest.approx(4 * WORST_MEASURED) and LP_BAR <= 2e-3


def test_keep_after_decoding(engine, docs):
    d = docs[0]
    ids0, mask0 = d["prompts"][0]
    ids1, mask1 = d["prompts"][1]
    need = len(ids0) + MAX_NEW + 1
    with engine.open_session(2, need, DecodeParameters(max_new_tokens=MAX_NEW), ignore_eos=True,
                             logprobs=True) as sess:
        sess.admit(ids0, mask0, d["page"])
        early = sess.keep_prefix(0, d["rows"])
        sess.step(8)
        sess.step(2)   # ten steps later
        late = sess.keep_prefix(0, d["rows"])
        short = sess.keep_prefix(0, 1)  # a one-row entry holds 1 / rows of the bytes
        st = sess.prefix_stats()
        assert st["entries"] == 3 and st["bytes"] > 0
        sess.drop_prefix(short)
        per = sess.prefix_stats()["bytes"]
        assert per < st["bytes"] and per % 2 == 0
        sess.retire(0)
        a = _admit_and_read(sess, lambda: sess.admit_prefix(early, ids1, mask1))
        b = _admit_and_read(sess, lambda: sess.admit_prefix(late, ids1, mask1))
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
        sess.drop_prefix(early)
        assert sess.prefix_stats()["bytes"] == per // 2
        sess.drop_prefix(late)
        st = sess.prefix_stats()
        assert st["bytes"] == 0 and st["entries"] == 0 and st["admissions"] == 2 and st["rows_reused"] == 2 * d["rows"]


# ------------------------------------------------------------------ slots and entries
def test_entry_outlives_its_slot_and_serves_two_slots_at_once(engine, docs):
    """Per-request session, 3 slots.  The entry is kept from slot 0, which is then retired: the other page moves into
    slot 0 (compaction).  Two requests are admitted from the one entry, one greedy and one sampled with a seed, and
    run together; then a third into the reused slot.  Every stream equals the plain admission of that prompt (vision + full prefill), run alone."""
    a, b = docs
    greedy = DecodeParameters(max_new_tokens=MAX_NEW)
    sampled = DecodeParameters(max_new_tokens=MAX_NEW, do_sample=True, temperature=0.8, top_p=0.9, seed=11)
    need = max(len(p[0]) for d in docs for p in d["prompts"]) + MAX_NEW + 1

    def plain(d, j, params):
        """The prompt's own plain admission (vision + full prefill), alone in a session of the same kind."""
        with engine.open_session(1, need, greedy, per_request=True) as s:
            assert s.admit(*d["prompts"][j], d["page"], params=params) == 0
            for _ in range(3):
                s.step(8)
            return s.retire(0)[0]

    ref = {"b0": plain(b, 0, greedy), "a1": plain(a, 1, greedy), "a2": plain(a, 2, sampled), "a3": plain(a, 3, greedy)}
    got = {}
    with engine.open_session(3, need, greedy, per_request=True) as sess:
        assert sess.admit(*a["prompts"][0], a["page"], params=greedy) == 0
        assert sess.admit(*b["prompts"][0], b["page"], params=greedy) == 1
        h = sess.keep_prefix(0, a["rows"])
        _, moved = sess.retire(0)
        assert moved == 1                                   # page b now lives in the entry's source slot
        assert sess.admit_prefix(h, *a["prompts"][1], params=greedy) == 1
        assert sess.admit_prefix(h, *a["prompts"][2], params=sampled) == 2
        owner = ["b0", "a1", "a2"]
        for _ in range(4):
            sess.step(8)
        assert all(s.done for s in sess.poll())
        for slot in (2, 1, 0):
            got[owner[slot]], _ = sess.retire(slot)
        assert sess.admit_prefix(h, *a["prompts"][3], params=greedy) == 0   # the reused slot
        for _ in range(3):
            sess.step(8)
        got["a3"], _ = sess.retire(0)
        st = sess.prefix_stats()
        assert st["admissions"] == 3 and st["rows_reused"] == 3 * a["rows"]
    assert got == ref


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_running_slot_alone(engine, docs):
    d = docs[0]
    ids0, mask0 = d["prompts"][0]
    ids1, mask1 = d["prompts"][1]
    rows, P1 = d["rows"], len(ids1)
    p = DecodeParameters(max_new_tokens=40)
    ref = engine.generate(ids0, mask0, d["page"], None, p)
    C_ = P1 + 20 + 1  # max_context: prompt 1 fits with max_new_tokens 20 exactly
    assert len(ids0) + 8 + 1 <= C_
    with engine.open_session(2, C_, p) as sess:
        run_new = C_ - len(ids0) - 1
        assert sess.admit(ids0, mask0, d["page"], max_new_tokens=run_new) == 0
        _einval(sess.keep_prefix, 0, 0)
        _einval(sess.keep_prefix, 0, len(ids0) + 1)
        _einval(sess.keep_prefix, 1, 1)                       # not an active slot
        h = sess.keep_prefix(0, rows)
        sess.step(3)
        _einval(sess.admit_prefix, h, ids1[:rows], mask1[:rows], max_new_tokens=4)       # no new row
        bad = list(ids1)
        bad[rows // 2] += 1
        _einval(sess.admit_prefix, h, bad, mask1, max_new_tokens=4)                      # an id inside the prefix
        bad = list(mask1)
        bad[rows] = 1
        _einval(sess.admit_prefix, h, ids1, bad, max_new_tokens=4)                       # a mask bit behind it
        bad = list(mask1)
        bad[rows - 1] = 0
        _einval(sess.admit_prefix, h, ids1, bad, max_new_tokens=4)                       # the mask inside it
        _einval(sess.admit_prefix, 9999, ids1, mask1, max_new_tokens=4)                  # unknown handle
        gone = sess.keep_prefix(0, 2)
        sess.drop_prefix(gone)
        _einval(sess.admit_prefix, gone, ids1, mask1, max_new_tokens=4)                  # dropped handle
        _einval(sess.drop_prefix, gone)
        _einval(sess.admit_prefix, h, ids1, mask1, max_new_tokens=21)                    # one row too many
        more = [sess.keep_prefix(0, 1) for _ in range(63)]                               # 64 entries in all
        _einval(sess.keep_prefix, 0, 1)                                                  # the 65th
        for m in more:
            sess.drop_prefix(m)
        assert sess.info()["active"] == 1
        assert sess.admit_prefix(h, ids1, mask1, max_new_tokens=20) == 1                 # accepted at the bound
        _einval(sess.admit_prefix, h, ids1, mask1, max_new_tokens=4)                     # no free slot
        assert sess.prefix_stats()["admissions"] == 1
        owner, out = ["running", "admitted"], {}
        for _ in range(8):  # finished slots leave at every burst boundary (the capacity invariant)
            if not owner:
                break
            for s in sorted(sess.step(8), key=lambda s: -s.slot):
                if s.done:
                    out[owner[s.slot]], moved = sess.retire(s.slot)
                    if moved >= 0:
                        owner[s.slot] = owner[moved]
                    owner.pop()
        assert not owner
    assert out["running"] == ref[:run_new] and len(out["admitted"]) > 0


# ------------------------------------------------------------------ the scheduler
def test_scheduler_hits_and_equal_outcomes(engine, docs):
    img = _img(100, 300, 420)
    tok = SyntheticTokenizer(512)
    need = max(len(p[0]) for p in docs[0]["prompts"]) + 12 + 1
    outs = {}
    for n in (0, 4):
        with BatchScheduler(engine, tok, 2, need, DecodeParameters(max_new_tokens=12), VS, prefix_cache=n) as s:
            first = s.submit(PROMPTS[0], [img]).result(timeout=120)
            second = s.submit(PROMPTS[1], [img.copy()]).result(timeout=120)
            outs[n] = (first.generated_tokens, second.generated_tokens)
            assert (s.prefix_hits, s.prefix_misses) == ((1, 1) if n else (0, 0))
    assert outs[0] == outs[4] and len(outs[0][1]) > 0
