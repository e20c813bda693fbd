"""Chunked admission on the GPU (Session.admit_begin / admit_advance / admit_cancel, BatchScheduler(admit_chunk=...)):
an admission in slices equals the plain admission, the running slots are untouched by it, retiring and cancelling
while one is pending, every refusal, and the scheduler.

Tiny config; the image page of test_session_prefix.py (base 512 / tiles 256: 177 image rows, a 178-row prefix) and a
text-only prompt.  chunk_rows 32 and 50 put several chunk boundaries inside the image rows (50 off a multiple of 32),
10 000 gives one chunk.

Chunked against plain (test_chunked_equals_plain): the emitted ids are equal at all 24 steps and the token
log-probabilities agree within LP_BAR.  The two differ only in the prefill (GEMMs on a chunk's rows against the whole
prompt's, attention_chunk's key order against the causal prefill's), so the bar is measured: LP_BAR is four times the
worst |delta| measured on an MI355X over this test's runs (WORST_MEASURED; DESIGN 4.12's convention).  Before ids are
compared the plain run's smallest top-1 / top-2 gap is asserted to exceed LP_BAR at every step."""
import json
import os

import numpy as np
import pytest

from dsocr import DecodeParameters, DsocrError, ModelLoadArgs, Page, VisionSettings, build_prompt_tokens, load_model
from dsocr._lib import EINVAL, SESSION_ADMIT_PENDING
from dsocr.scheduler import BatchScheduler
from dsocr.synth import SyntheticTokenizer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, "deepseek-ocr.rs_amd", "dsocr", "configs", "tiny.json")
VS = VisionSettings(512, 256, True)
PROMPTS = ["<image>\nFree OCR.", "<image>\nConvert the document to markdown.", "<image>\nParse the figure.",
           "<image>\nLocate the title in the image."]
TEXT = "Convert the document to markdown. " * 12
MAX_NEW = 24
VISION_SLICES = 3            # SAM, CLIP, projector + the image-row plan
_CFG = json.load(open(TINY))
LAYERS = int((_CFG.get("language_config") or _CFG)["num_hidden_layers"])  # decoder layers of the tiny config
WORST_MEASURED = 9.537e-7    # worst |delta logprob| chunked against plain on an MI355X (see the docstring)
LP_BAR = 4 * WORST_MEASURED


@pytest.fixture(scope="module")
def engine(gpu):
    eng = load_model(ModelLoadArgs(config_path=TINY, synthetic_seed=7, dtype="f16"))
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def reqs():
    """Four image requests on one page and one text-only request: (ids, mask, page)."""
    tok = SyntheticTokenizer(512)
    page = Page(np.random.default_rng(100).integers(0, 256, (300, 420, 3), dtype=np.uint8), VS)
    out = [(*build_prompt_tokens(tok, p, [page.n_image_tokens]), page) for p in PROMPTS]
    out.append((*build_prompt_tokens(tok, TEXT, []), None))
    assert max(j for j, m in enumerate(out[0][1]) if m) + 1 == 178
    assert len(out[4][0]) > 70 and not any(out[4][1])
    return out


def _need(reqs):
    return max(len(r[0]) for r in reqs) + MAX_NEW + 1


def _open(engine, reqs, slots, extra=0):
    return engine.open_session(slots, _need(reqs) + extra, DecodeParameters(max_new_tokens=MAX_NEW), ignore_eos=True,
                               logprobs=True)


def _einval(fn, *a, **kw):
    with pytest.raises(DsocrError) as ei:
        fn(*a, **kw)
    assert ei.value.status == EINVAL, ei.value


def _chunked(sess, rq, chunk, between=None):
    """A whole admission in slices; `between(i)` runs after slice i.  Returns (slot, slices)."""
    sess.admit_begin(rq[0], rq[1], rq[2], chunk_rows=chunk)
    n = 0
    while True:
        done, slot = sess.admit_advance()
        n += 1
        if done:
            return slot, n
        assert slot == -1
        if between:
            between(n)


def _finish(sess, slot):
    """Steps until `slot` has MAX_NEW tokens; (ids, log-probabilities, top-2 log-probabilities), then retires it."""
    for _ in range(MAX_NEW):
        st = {s.slot: s for s in sess.poll()}
        if st[slot].out_len >= MAX_NEW:
            break
        sess.step(8)
    lp, _, tl = sess.logprobs(slot, 0, MAX_NEW, 2)
    ids, _ = sess.retire(slot)
    return ids, lp.copy(), tl.copy()


@pytest.fixture(scope="module")
def singles(engine, reqs):
    """Every request alone in a session through the plain admission: (ids, lp, top-2)."""
    out = []
    with _open(engine, reqs, 1) as sess:
        for rq in reqs:
            out.append(_finish(sess, sess.admit(*rq)))
    return out


def test_chunked_equals_plain(engine, reqs, singles):
    worst, min_gap = 0.0, np.inf
    with _open(engine, reqs, 2) as sess:
        for i in (1, 4):  # the image prompt and the text-only one
            rq, plain = reqs[i], singles[i]
            P = len(rq[0])
            gap = float(np.min(plain[2][:, 0] - plain[2][:, 1]))
            min_gap = min(min_gap, gap)
            for chunk in (32, 50, 10000):
                seen, vis = [], VISION_SLICES if rq[2] is not None else 0
                before = sess.admit_progress()["chunk_attn_launches"]
                slot, slices = _chunked(sess, rq, chunk, lambda n: seen.append(sess.admit_progress()))
                assert slot == 0 and slices == vis + -(-P // chunk)
                assert all(p["pending"] and p["rows_total"] == P for p in seen)
                assert [p["rows_done"] for p in seen] == [min(chunk * max(0, k - vis), P) for k in range(1, slices)]
                assert [p["vision_stage"] for p in seen] == [2, 3, 0][:vis] + [0] * (slices - 1 - vis)
                # every chunk behind a past attends through launch_attention_chunk, once per layer
                assert sess.admit_progress()["chunk_attn_launches"] - before == LAYERS * (-(-P // chunk) - 1)
                assert not sess.admit_progress()["pending"] and not sess.info()["flags"] & SESSION_ADMIT_PENDING
                got = _finish(sess, slot)
                delta = float(np.max(np.abs(plain[1].astype(np.float64) - got[1])))
                print(f"chunked admission: request {i} chunk {chunk}: worst |d logprob| {delta:.3e}, smallest "
                      f"top-1/top-2 gap of the plain run {gap:.3e}")
                worst = max(worst, delta)
                assert len(plain[0]) == MAX_NEW and got[0] == plain[0], (i, chunk)
    print(f"chunked admission: worst |d logprob| {worst:.3e} (bar {LP_BAR:.3e}), smallest gap {min_gap:.3e}")
    assert min_gap > LP_BAR, min_gap
    assert worst <= LP_BAR, worst


def _trace(sess, steps, hook=None):
    """`steps` one-step bursts; hook(i) runs before burst i.  Returns per slot the ids and log-probabilities read
    after every burst: [(active, [ids per slot], [lp per slot])]."""
    out = []
    for i in range(steps):
        if hook:
            hook(i)
        st = sess.step(1)
        row = []
        for s in st:
            n = min(s.out_len, MAX_NEW)
            row.append((n, sess.logprobs(s.slot, 0, n, 0)[0].copy()))
        out.append((len(st), row))
    return out


def test_running_slots_are_untouched(engine, reqs, singles):
    """Two slots decode while a third page is admitted with one advance per one-step burst (n == S - 1: the page stays
    in the staging slot)."""
    STEPS = 12
    with _open(engine, reqs, 3, extra=8) as sess:
        sess.admit(*reqs[0]); sess.admit(*reqs[2])
        base = _trace(sess, STEPS)
    state = {"at": None}
    with _open(engine, reqs, 3, extra=8) as sess:
        sess.admit(*reqs[0]); sess.admit(*reqs[2])
        sess.admit_begin(*reqs[1], chunk_rows=32)

        def hook(i):
            if state["at"] is None:
                assert sess.info()["flags"] & SESSION_ADMIT_PENDING
                done, slot = sess.admit_advance()
                if done:
                    assert slot == 2
                    state["at"] = i
        got = _trace(sess, STEPS, hook)
        at = state["at"]
        assert at == 8  # three vision slices and six chunks of a 185-row prompt: active from burst 8 on
        for i in range(at):
            assert got[i][0] == 2
            for b in range(2):
                assert got[i][1][b][0] == base[i][1][b][0]
                assert np.array_equal(got[i][1][b][1].view(np.uint32), base[i][1][b][1].view(np.uint32)), (i, b)
        assert got[at][0] == 3
        chunked_ids = [_finish(sess, b)[0] for b in (2, 1, 0)][::-1]
    # a session that admits plainly at that step
    with _open(engine, reqs, 3, extra=8) as sess:
        sess.admit(*reqs[0]); sess.admit(*reqs[2])
        _trace(sess, STEPS, lambda i: sess.admit(*reqs[1]) if i == at else None)
        plain_ids = [_finish(sess, b)[0] for b in (2, 1, 0)][::-1]
    assert chunked_ids == plain_ids
    assert chunked_ids == [singles[0][0], singles[2][0], singles[1][0]]


@pytest.mark.parametrize("slots", [4, 3])
def test_retire_while_pending(engine, reqs, singles, slots):
    """slots 4: three active, slot 0 retired while the fourth page is pending (slot 2 moves to 0), the page then moves
    from the staging slot 3 to slot 2.  slots 3: two active, slot 0 retired, the page moves from slot 2 to slot 1."""
    active = [0, 2, 3][:slots - 1]
    with _open(engine, reqs, slots, extra=8) as sess:
        for i in active:
            sess.admit(*reqs[i])
        sess.step(2)
        sess.admit_begin(*reqs[1], chunk_rows=50)
        assert sess.admit_advance() == (False, -1)
        sess.step(1)
        assert sess.admit_advance() == (False, -1)
        ids0, moved = sess.retire(0)
        assert moved == len(active) - 1 and ids0 == singles[active[0]][0][:len(ids0)]
        sess.step(1)
        while True:
            done, slot = sess.admit_advance()
            if done:
                break
            sess.step(1)
        assert slot == len(active) - 1 and sess.info()["active"] == len(active)
        order = [active[-1]] + active[1:-1] + [1]  # slot -> request after the compaction and the admission
        for b in range(len(order) - 1, -1, -1):
            assert _finish(sess, b)[0] == singles[order[b]][0], b


def test_cancel(engine, reqs, singles):
    with _open(engine, reqs, 3, extra=8) as sess:
        assert sess.admit(*reqs[0]) == 0
        sess.admit_begin(*reqs[1], chunk_rows=32)
        assert sess.admit_advance() == (False, -1)      # the first vision slice (SAM)
        sess.admit_cancel()
        sess.admit_begin(*reqs[1], chunk_rows=32)
        for _ in range(VISION_SLICES):                  # ... and after all of the vision
            assert sess.admit_advance() == (False, -1)
        assert sess.admit_progress()["vision_stage"] == 0 and sess.admit_progress()["rows_done"] == 0
        sess.admit_cancel()
        assert not sess.admit_progress()["pending"] and sess.info()["active"] == 1
        sess.step(1)
        sess.admit_begin(*reqs[3], chunk_rows=32)
        for _ in range(VISION_SLICES + 2):              # vision and two chunks: cancelled in the middle of the prompt
            assert sess.admit_advance() == (False, -1)
            sess.step(1)
        assert sess.admit_progress()["rows_done"] == 64
        sess.admit_cancel()
        assert sess.admit(*reqs[1]) == 1                # a plain admission into the slot after the running one
        assert sess.admit(*reqs[4]) == 2                # ... and into the slot the cancelled page was staged in
        for b in (2, 1, 0):
            assert _finish(sess, b)[0] == singles[[0, 1, 4][b]][0], b


def test_errors(engine, reqs):
    with _open(engine, reqs, 2) as sess:
        _einval(sess.admit_advance)
        _einval(sess.admit_cancel)
        _einval(sess.admit_begin, *reqs[1], chunk_rows=31)
        _einval(sess.admit_begin, *reqs[1], chunk_rows=32, max_new_tokens=MAX_NEW + 1)      # one of admit's own checks
        assert not sess.admit_progress()["pending"]      # a refused begin changes nothing
        assert sess.admit(*reqs[0]) == 0
        sess.admit_begin(*reqs[1], chunk_rows=32)
        _einval(sess.admit_begin, *reqs[2], chunk_rows=32)
        _einval(sess.admit, *reqs[2])
        h = sess.keep_prefix(0, 178)                     # keeping a prefix of an active slot stays legal
        _einval(sess.admit_prefix, h, reqs[2][0], reqs[2][1])
        p = sess.admit_progress()
        p.pop("chunk_attn_launches")
        assert p == {"pending": True, "rows_done": 0, "rows_total": len(reqs[1][0]), "slices": 0, "vision_stage": 1}
        sess.admit_cancel()
        assert sess.admit(*reqs[2]) == 1
        _einval(sess.admit_begin, *reqs[1], chunk_rows=32)   # no free slot
        assert not sess.admit_progress()["pending"] and sess.info()["active"] == 2
    with _open(engine, reqs, 2) as sess:                 # close while pending
        sess.admit_begin(*reqs[1], chunk_rows=32)
        sess.admit_advance()
    with _open(engine, reqs, 1) as sess:                 # the engine is as usable as before
        assert sess.admit(*reqs[4]) == 0


@pytest.mark.parametrize("stream", [False, True])
def test_scheduler(engine, reqs, stream):
    """Four requests for three slots: the first is admitted with nothing running (slices back to back), the others
    while slots decode (a burst after every slice), the fourth once a slot is free."""
    tok = SyntheticTokenizer(512)
    img = np.random.default_rng(100).integers(0, 256, (300, 420, 3), dtype=np.uint8)
    params = DecodeParameters(max_new_tokens=MAX_NEW)
    seen = []
    with BatchScheduler(engine, tok, 3, _need(reqs), params, VS, admit_chunk=32) as s:
        futs = [s.submit(p, [img], on_token=(lambda n, t: seen.append(n)) if stream and i == 0 else None)
                for i, p in enumerate(PROMPTS)]
        outs = [f.result(timeout=120) for f in futs]
        events = list(s.events)
        assert s.chunked_admissions == 4 and s.admit_slices == 4 * 9  # three vision slices + six chunks of 185 rows
    with BatchScheduler(engine, tok, 1, _need(reqs), params, VS) as ref:
        for p, o in zip(PROMPTS, outs):
            assert o.generated_tokens == ref.submit(p, [img]).result(timeout=120).generated_tokens, p
        assert ref.events == [] and ref.admit_slices == 0
    kinds = [e[0] for e in events]
    assert kinds[:9] == ["slice"] * 9 and [e[1] for e in events[:9]] == ["vision"] * 3 + ["prefill"] * 6
    for a, b in zip(events, events[1:]):
        if a[0] == "slice" and a[2] > 0:  # a slot is running after the slice: a burst before the next slice
            assert b[0] == "burst" and b[1] == a[2], (a, b)
    assert any(x == ("burst", "slice", "burst") for x in zip(kinds, kinds[1:], kinds[2:]))
    sizes = [e[2] for e in events if e[0] == "burst"]
    if stream:
        first_done = len(seen)
        assert seen == list(range(1, first_done + 1)) and first_done >= 1
        assert all(k == 1 for k in sizes[:first_done - 1])  # one step per burst while the streaming request runs
    else:
        assert set(sizes) == {8}
