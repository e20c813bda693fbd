"""Per-request logit bias and token allow / deny sets on the GPU.

The kernels through their hook against NumPy's ``l + b`` (bit for bit: a sum of two f32 values is exact in any
order); the engine against the CPU oracle, whose ``select_token_id`` is patched here to add the dense bias to its
``logits`` argument (the semantics restated: nothing under ``oracle/`` changes); decode sessions against the same
page decoded alone.  Tiny config, the pages and prompt of tests/test_session.py.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import dsocr
from dsocr import DecodeParameters, DsocrError, ModelLoadArgs, Page, VisionSettings, build_prompt_tokens, load_model
from dsocr._lib import SESSION_LOGIT_BIAS, SESSION_LOGPROBS, lib
from dsocr.constraint import merge_constraint
from dsocr.synth import SyntheticTokenizer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, "deepseek-ocr.rs_amd", "dsocr", "configs", "tiny.json")
TINY_VS = VisionSettings(256, 128, True)
SEED = 7
PROMPT = "<image>\nConvert the document to markdown."
SIZES = [(300, 420), (256, 256), (500, 140)]
CHUNK = 2048     # the add kernel's chunk of the row
SENTINEL = np.float32(-12345.5)
# test_logprobs.py's bound for a log-probability against float64 NumPy: LP_C * 2**-23 * max(1, max|l - m|)
LP_C = 32.3
EPS = 2.0 ** -23
# case (b): 16 allowed ids under no_repeat_ngram_size = 3.  A greedy run of this model over 16 ids does not exhaust a
# two-token prefix within 700 tokens (tried on the CPU oracle with 16 lists), so the prompt is chosen with the list:
# behind the usual prompt it carries (a, b, t) for every allowed t and ends in (a, b), a and b the first two allowed
# ids.  The first selection then finds all 16 ids banned and select_token_id falls back to the unfiltered row; the
# test asserts on the oracle alone that this happens.
ALLOW_B = list(range(100, 116))
ALLOW_B_STEPS = 24


# ------------------------------------------------------------------ the kernels through their hook
def k_logit_bias(logits, lists, flags, allow_only, offset):
    """The hook on host rows [B][ld] (V given by the caller's sentinel columns): (logits after the add, dense rows)."""
    logits = np.ascontiguousarray(logits, np.float32)
    B, ld = logits.shape
    V = k_logit_bias.V
    first, count, ids, vals = [], [], [], []
    for lst in lists:
        first.append(len(ids))
        count.append(len(lst))
        ids += [int(t) for t, _ in lst]
        vals += [float(v) for _, v in lst]
    ids = np.asarray(ids or [0], np.int64)
    vals = np.asarray(vals or [0], np.float32)
    first, count = np.asarray(first, np.int32), np.asarray(count, np.int32)
    flags, allow_only = np.asarray(flags, np.int32), np.asarray(allow_only, np.int32)
    dld = (V + 3) // 4 * 4
    dense = np.full((B, dld), SENTINEL, np.float32)
    out = logits.copy()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    st = lib().dsocr_k_logit_bias(B, V, ld, offset, p(out), p(ids), p(vals), p(first), p(count), p(flags), p(allow_only),
                                  p(dense), dld)
    assert st == 0, lib().dsocr_last_error()
    return out, dense


@pytest.mark.parametrize("V,ld,offset", [(1003, 1008, 1), (1003, 1008, 0), (4104, 4104, 0), (4104, 4104, 3)])
def test_kernel_hook(gpu, V, ld, offset):
    """B = 3 rows {none, bias list, allow-only}.  V = 1003 in ld = 1008 behind an odd offset (the scalar path) and
    aligned (the vector path with a 3-element scalar tail); V = 4104: two full chunks and an 8-element tail.  The
    lists hit the first and the last element, both sides of a chunk boundary and both sides of a 16-byte boundary."""
    k_logit_bias.V = V
    r = np.random.default_rng(V + offset)
    x = np.full((3, ld), SENTINEL, np.float32)
    x[:, :V] = (r.standard_normal((3, V)) * 4).astype(np.float32)
    edge = [0, V - 1, 3, 4]                                  # first, last, the two sides of a 16-byte boundary
    edge += [CHUNK - 1, CHUNK] if V > CHUNK else [V // 2 - 1, V // 2]
    if V > 2 * CHUNK:
        edge += [2 * CHUNK - 1, 2 * CHUNK]
    vals = [1.5, -2.25, -np.inf, 30.0, -np.inf, 0.125, 7.0, -100.0]
    bias_list = [(t, vals[i]) for i, t in enumerate(edge)] + [(int(t), float(v)) for t, v in
                                                               zip(r.choice(np.arange(8, V - 8), 20, replace=False) | 1,
                                                                   r.standard_normal(20))
                                                               if int(t) not in edge and int(t) not in (CHUNK - 1, CHUNK)]
    bias_list = list({t: v for t, v in bias_list}.items())
    allow_list = [(t, 0.0) for t in edge] + [(V // 3, 2.5)]
    got, dense = k_logit_bias(x, [[], bias_list, allow_list], [0, 1, 1], [0, 0, 1], offset)
    b1 = np.zeros(V, np.float32)
    b2 = np.full(V, -np.inf, np.float32)
    for t, v in bias_list:
        b1[t] = np.float32(v)
    for t, v in allow_list:
        b2[t] = np.float32(v)
    want = x.copy()
    want[1, :V] = x[1, :V] + b1
    want[2, :V] = x[2, :V] + b2
    assert got[0].tobytes() == x[0].tobytes()                       # the unconstrained row: byte-identical
    assert got[1:, :V].tobytes() == want[1:, :V].tobytes()          # numpy l + b, bit for bit
    assert np.all(got[:, V:] == SENTINEL)                           # columns [V, ld) keep the sentinel
    assert np.all(dense[0] == 0)                                    # (no flag: the hook's zero row, never built)
    assert dense[1, :V].tobytes() == b1.tobytes() and dense[2, :V].tobytes() == b2.tobytes()
    assert np.all(dense[1:, V:] == 0)
    assert np.isneginf(got[2, :V]).sum() == V - len(allow_list)


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
    """The CPU oracle on page 0, with ``oracle.model.select_token_id`` patched per call to add a dense bias."""

    def __init__(self):
        import oracle.model as om
        from oracle.weights import Weights
        self.om = om
        self.model = om.OracleModel(json.load(open(TINY)), Weights(seed=SEED, dtype="f16"))
        self.emb, _ = self.model.image_embeddings(_img(100, *SIZES[0]), 256, 128, True)
        self.fallbacks = 0

    def generate(self, ids, mask, max_new, dense=None, allowed=None, **kw):
        from oracle.decoder import banned_ngram_tokens
        om, real = self.om, self.om.select_token_id
        self.fallbacks = 0

        def select(logits, context, repetition_penalty=1.0, no_repeat_ngram_size=None, **sel):
            l = np.asarray(logits, np.float32)
            if dense is not None:
                l = l + dense
            if allowed is not None and no_repeat_ngram_size and no_repeat_ngram_size > 1:
                if set(allowed) <= banned_ngram_tokens([int(c) for c in context], no_repeat_ngram_size):
                    self.fallbacks += 1  # every allowed id is banned: the unfiltered row decides
            return real(l, context, repetition_penalty, no_repeat_ngram_size, **sel)

        om.select_token_id = select
        try:
            out, _ = self.model.generate(ids, mask, self.emb, max_new, eos_token_id=1, **kw)
        finally:
            om.select_token_id = real
        return [int(t) for t in out]


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def _constrained(engine, req, con, params):
    return engine.generate_constrained([(*req, None)], [con], params)[0]


def _prompt_b(pages):
    """Page 0's prompt followed by (a, b, t) for every allowed t, then (a, b)."""
    ids, mask, page = pages[0]
    a, b = ALLOW_B[:2]
    tail = [x for t in ALLOW_B for x in (a, b, t)] + [a, b]
    return list(ids) + tail, list(mask) + [0] * len(tail), page


def test_engine_deny(engine, pages, oracle):
    """(a) deny the unconstrained run's first three distinct tokens."""
    ids, mask, page = pages[0]
    p = DecodeParameters(max_new_tokens=16)
    plain = engine.generate(ids, mask, page, None, p)
    assert plain == oracle.generate(ids, mask, 16)
    deny = list(dict.fromkeys(plain))[:3]
    con = merge_constraint(banned_token_ids=deny, vocab=engine.vocab)
    got = _constrained(engine, pages[0], con, p)
    assert got == oracle.generate(ids, mask, 16, dense=con.dense(engine.vocab))
    assert got != plain and not set(got) & set(deny)


def test_engine_allow_with_ngram_fallback(engine, pages, oracle):
    """(b) an allow list of 16 ids under no_repeat_ngram_size = 3: the ban exhausts the list and the fallback runs
    (asserted on the oracle), and every emitted id is still an allowed one."""
    ids, mask, page = req = _prompt_b(pages)
    allow = ALLOW_B
    con = merge_constraint(allowed_token_ids=allow, vocab=engine.vocab)
    want = oracle.generate(ids, mask, ALLOW_B_STEPS, dense=con.dense(engine.vocab), allowed=allow, no_repeat_ngram_size=3)
    assert oracle.fallbacks > 0, "the chosen list never exhausts under the ban: pick another"
    got = _constrained(engine, req, con, DecodeParameters(max_new_tokens=ALLOW_B_STEPS, no_repeat_ngram_size=3))
    assert got == want and set(got) <= set(allow) and len(got) == ALLOW_B_STEPS


def test_engine_bias_with_penalty(engine, pages, oracle):
    """(c) +30 on one id with repetition penalty 1.3: the bias goes in before the penalty."""
    ids, mask, page = pages[0]
    p = DecodeParameters(max_new_tokens=16, repetition_penalty=1.3)
    plain = engine.generate(ids, mask, page, None, p)
    t = next(i for i in range(2, engine.vocab) if i not in plain)
    con = merge_constraint(logit_bias={t: 30.0}, vocab=engine.vocab)
    got = _constrained(engine, pages[0], con, p)
    assert got == oracle.generate(ids, mask, 16, dense=con.dense(engine.vocab), repetition_penalty=1.3)
    assert t in got


def test_engine_allow_sampled(engine, pages, oracle):
    """(d) the allow list under sampling with a fixed seed."""
    ids, mask, page = pages[0]
    allow = ALLOW_B
    con = merge_constraint(allowed_token_ids=allow, vocab=engine.vocab)
    kw = dict(do_sample=True, temperature=0.8, top_p=0.9, seed=11)
    got = _constrained(engine, pages[0], con, DecodeParameters(max_new_tokens=16, **kw))
    assert got == oracle.generate(ids, mask, 16, dense=con.dense(engine.vocab), **kw)
    assert set(got) <= set(allow)


def _einval(fn, *a, **kw):
    with pytest.raises(DsocrError) as ei:
        fn(*a, **kw)
    assert ei.value.status == 1, ei.value


def test_engine_refuses(engine, pages):
    con = merge_constraint(banned_token_ids=[5])
    _einval(_constrained, engine, pages[0], con, DecodeParameters(max_new_tokens=4, use_cache=False))
    from dsocr.constraint import LogitConstraint
    for bad in (LogitConstraint((engine.vocab,), (0.0,)), LogitConstraint((3, 3), (0.0, 1.0)),
                LogitConstraint((3,), (float("nan"),)), LogitConstraint((3,), (float("inf"),)),
                LogitConstraint((), (), True), LogitConstraint((-1,), (0.0,))):
        _einval(_constrained, engine, pages[0], bad, DecodeParameters(max_new_tokens=4))
    # nothing was left behind: the plain call still runs
    assert len(engine.generate(*pages[0], None, DecodeParameters(max_new_tokens=4))) == 4


# ------------------------------------------------------------------ sessions
def _cons(engine, pages):
    """{page: constraint} of the mixed batch: none, a deny list, an allow list."""
    p = DecodeParameters(max_new_tokens=16)
    plain1 = engine.generate(*pages[1], None, p)
    plain2 = engine.generate(*pages[2], None, p)
    deny = merge_constraint(banned_token_ids=list(dict.fromkeys(plain1))[:3], vocab=engine.vocab)
    allow = merge_constraint(allowed_token_ids=sorted(set(plain2))[:2] + list(range(40, 54)), vocab=engine.vocab)
    return {0: None, 1: deny, 2: allow}


def _kw(con):
    return {} if con is None else con.kwargs()


def test_session_mixed_batch(engine, pages):
    """3 slots {none, deny, allow}: every page equals the same page decoded alone with its constraint, the
    unconstrained one today's decode.  Slot 0 retires mid-run, so the allow-list page moves into slot 0 and must
    go on honouring its list.  Screened steps before the first constrained admission, exact ones after it (the
    session is opened per request as well: with fixed parameters a 3-slot session of the tiny model, whose
    vocabulary the 3..8-page screened head does not take, runs the exact head throughout)."""
    cons = _cons(engine, pages)
    max_new = {0: 6, 1: 20, 2: 20}
    single = {i: (engine.generate(*pages[i], None, DecodeParameters(max_new_tokens=m)) if cons[i] is None else
                  _constrained(engine, pages[i], cons[i], DecodeParameters(max_new_tokens=m)))
              for i, m in max_new.items()}
    need = max(len(pages[i][0]) + m + 1 for i, m in max_new.items())
    P = lambda m: DecodeParameters(max_new_tokens=m)
    with engine.open_session(3, need + 8, P(20), per_request=True, logit_bias=True) as sess:
        assert sess.info()["flags"] == SESSION_LOGIT_BIAS | 1
        assert sess.admit(*pages[0], params=P(6)) == 0
        sess.step(2)
        hs = sess.head_steps()
        assert hs["screened"] == 2 and hs["exact"] == 0
        assert sess.admit(*pages[1], params=P(20), **_kw(cons[1])) == 1
        assert sess.admit(*pages[2], params=P(20), **_kw(cons[2])) == 2
        st = sess.step(4)
        assert st[0].done
        ids0, moved = sess.retire(0)
        assert moved == 2 and ids0 == single[0]
        sess.step(8)
        sess.step(8)
        assert all(s.done for s in sess.poll())
        hs = sess.head_steps()
        assert hs["screened"] == 2 and hs["exact"] == 20
        ids1, _ = sess.retire(1)
        ids2, _ = sess.retire(0)
        # a page admitted without a constraint behind them: the flag of the reused slot is clear again
        assert sess.admit(*pages[0], params=P(6)) == 0
        sess.step(8)
        again, _ = sess.retire(0)
        assert sess.head_steps()["screened"] == 2 + 8
    assert ids1 == single[1] and ids2 == single[2] and again == single[0]
    assert set(ids2) <= set(cons[2].ids) and len(ids2) == 20
    assert not set(ids1) & set(cons[1].ids)


def test_session_admission_forms(engine, pages):
    """The same constrained request through admit, admit_prefix and admit_begin (the prompt in 2 chunks): the same
    ids, first token included.  A cancelled chunked admission leaves no constraint behind."""
    ids, mask, page = pages[0]  # (the longest prompt: two chunks of at least 32 rows)
    first = engine.generate(ids, mask, page, None, DecodeParameters(max_new_tokens=10))
    con = merge_constraint(banned_token_ids=list(dict.fromkeys(first))[:3], vocab=engine.vocab)
    want = _constrained(engine, pages[0], con, DecodeParameters(max_new_tokens=10))
    assert want != first
    plain1 = engine.generate(*pages[1], None, DecodeParameters(max_new_tokens=10))
    rows = max(i for i, m in enumerate(mask) if m) + 1
    chunk = max(32, (len(ids) + 1) // 2)
    assert chunk < len(ids)
    got = {}
    with engine.open_session(2, len(ids) + 11 + 8, DecodeParameters(max_new_tokens=10), logit_bias=True) as sess:
        assert sess.admit(ids, mask, page, max_new_tokens=10, **con.kwargs()) == 0
        handle = sess.keep_prefix(0, rows)
        sess.step(8)
        sess.step(8)
        got["admit"], _ = sess.retire(0)
        assert sess.admit_prefix(handle, ids, mask, max_new_tokens=10, **con.kwargs()) == 0
        sess.step(8)
        sess.step(8)
        got["prefix"], _ = sess.retire(0)
        # begun with a constraint, then cancelled: the next page (no constraint) decodes as it does today
        sess.admit_begin(ids, mask, page, chunk_rows=chunk, max_new_tokens=10, **con.kwargs())
        sess.admit_advance()
        sess.admit_cancel()
        assert sess.admit(*pages[1], max_new_tokens=10) == 0
        sess.step(8)
        sess.step(8)
        got["after_cancel"], _ = sess.retire(0)
        sess.admit_begin(ids, mask, page, chunk_rows=chunk, max_new_tokens=10, **con.kwargs())
        done, slices = False, 0
        while not done:
            done, slot = sess.admit_advance()
            slices += 1
        assert slot == 0 and slices >= 3
        sess.step(8)
        sess.step(8)
        got["chunked"], _ = sess.retire(0)
    assert got["admit"] == got["prefix"] == got["chunked"] == want
    assert got["after_cancel"] == plain1


def test_session_refuses_without_flag(engine, pages):
    con = merge_constraint(banned_token_ids=[5])
    need = len(pages[0][0]) + 9
    with engine.open_session(2, need, DecodeParameters(max_new_tokens=8)) as sess:
        _einval(sess.admit, *pages[0], max_new_tokens=8, **con.kwargs())
        assert sess.info()["active"] == 0


def _lp_ref(l, K):
    """float64 log-softmax of one row over its finite entries: (lp [V], the K best ids, the bound's scale)."""
    fin = np.isfinite(l)
    l64 = l.astype(np.float64)
    m = l64[fin].max()
    lp = np.where(fin, l64 - m - np.log(np.sum(np.exp(l64[fin] - m))), -np.inf)
    order = np.argsort(-np.where(fin, l64, -np.inf), kind="stable")[:K]
    return lp, order, max(1.0, float(np.abs(l64[fin] - m).max()))


def test_session_logprobs_under_a_constraint(engine, pages):
    """LOGPROBS | LOGIT_BIAS: the entries are those of the constrained distribution (step 0 against NumPy on the
    traced unconstrained logits + b), a denied id is never an alternative, and the unconstrained row of the batch is
    bit-identical to a session without the bias flag."""
    K = 20
    p = DecodeParameters(max_new_tokens=8)
    _, logits = engine.generate_trace([(*pages[1], None)], p)
    l0 = logits[0][0]
    deny = [int(t) for t in np.argsort(-l0, kind="stable")[:3]]   # the three likeliest first tokens
    con = merge_constraint(banned_token_ids=deny, vocab=engine.vocab)
    need = max(len(pages[i][0]) for i in (0, 1)) + 9 + 8

    def run(bias):
        kw = {"logit_bias": True} if bias else {}
        with engine.open_session(2, need, p, logprobs=True, **kw) as sess:
            assert sess.info()["flags"] == SESSION_LOGPROBS | (SESSION_LOGIT_BIAS if bias else 0)
            sess.admit(*pages[0], max_new_tokens=8)
            sess.admit(*pages[1], max_new_tokens=8, **(con.kwargs() if bias else {}))
            sess.step(8)
            out = [sess.logprobs(s, 0, 8, K) for s in (0, 1)]
            ids = [sess.retire(s)[0] for s in (1, 0)][::-1]
        return ids, out

    ids_b, lp_b = run(True)
    ids_p, lp_p = run(False)
    assert ids_b[0] == ids_p[0]
    for a, b in zip(lp_b[0], lp_p[0]):
        assert a.tobytes() == b.tobytes()
    lp, ti, tl = lp_b[1]
    assert not set(deny) & set(int(t) for t in ti.reshape(-1)) and not set(deny) & set(ids_b[1])
    ref, order, scale = _lp_ref(l0 + con.dense(engine.vocab), K)
    tol = LP_C * EPS * scale
    print(f"constrained step-0 entry: |err| {abs(lp[0] - ref[ids_b[1][0]]):.3e}, alternatives "
          f"{np.abs(tl[0] - ref[order]).max():.3e}, bound {tol:.3e}")
    assert np.array_equal(ti[0], order)
    assert abs(lp[0] - ref[ids_b[1][0]]) <= tol and np.abs(tl[0] - ref[order]).max() <= tol


def test_feature_off_is_unchanged(engine, pages):
    """No flag, no constraint: the ids of the plain paths, asserted once here against the oracle and each other."""
    p = DecodeParameters(max_new_tokens=12)
    a = engine.generate(*pages[0], None, p)
    steps = engine.last_timings()["decode_steps"]
    _constrained(engine, pages[0], merge_constraint(banned_token_ids=[a[0]]), p)
    assert engine.generate(*pages[0], None, p) == a and engine.last_timings()["decode_steps"] == steps
    assert engine.generate_constrained([(*pages[0], None)], [None], p)[0] == a
    with engine.open_session(2, len(pages[0][0]) + 13, p) as sess:
        assert sess.info()["flags"] == 0
        sess.admit(*pages[0], max_new_tokens=12)
        sess.step(8)
        sess.step(8)
        assert sess.head_steps()["exact"] == 0
        assert sess.retire(0)[0] == a
