"""One engine walked across the modes that share its decode rows (the engine's DecodeRows record).

generate, a session and profile_decode reserve and read the same record, with different capacities, optional rows and
hand-off sizing.  On one engine, in order: generate at B = 3, a 2-slot session, a sampled generate at B = 1,
profile_decode, generate at B = 3 again, then a second session.  Contract: every call's ids equal the ids the same
call gives as the first call on a freshly loaded engine.  The shapes cross the paths that differ: B = 1 (the fused
one-page launch and both hand-off copies), 2 (fused norm), 3 (matrix-core forms), and sessions whose slot count
differs from the generate before them.
"""
import math
import os

import numpy as np
import pytest

from dsocr import DecodeParameters, ModelLoadArgs, Page, VisionSettings, build_prompt_tokens, load_model
from dsocr.synth import SyntheticTokenizer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, "deepseek-ocr.rs_amd", "dsocr", "configs", "tiny.json")
TINY_VS = VisionSettings(256, 128, True)
SEED = 7
PROMPT = "<image>\nConvert the document to markdown."
SIZES = [(300, 420), (256, 256), (500, 140)]
GREEDY = DecodeParameters(max_new_tokens=10)
SAMPLED = DecodeParameters(max_new_tokens=10, do_sample=True, temperature=0.7, top_p=0.9, top_k=40, seed=11)
SESSION_NEW = [10, 7]  # the two admitted pages' max_new_tokens: they finish in different bursts


def _pages():
    tok = SyntheticTokenizer(512)
    out = []
    for i, (h, w) in enumerate(SIZES):
        page = Page(np.random.default_rng(100 + i).integers(0, 256, (h, w, 3), dtype=np.uint8), TINY_VS)
        ids, mask = build_prompt_tokens(tok, PROMPT, [page.n_image_tokens])
        out.append((ids, mask, page))
    return out


def _load():
    return load_model(ModelLoadArgs(config_path=TINY, synthetic_seed=SEED, dtype="f16"))


def _batch3(eng, pages):
    return eng.generate_batch([(ids, mask, page, None) for ids, mask, page in pages], GREEDY, ignore_eos=True)


def _sampled1(eng, pages):
    ids, mask, page = pages[0]
    return eng.generate(ids, mask, page, None, SAMPLED, ignore_eos=True)


def _session(eng, pages, slots):
    """Pages 0 and 1 through a session of `slots` slots, stepped to completion: their ids, by page."""
    need = max(len(pages[i][0]) + m + 1 for i, m in enumerate(SESSION_NEW))
    out, owner = {}, [0, 1]
    with eng.open_session(slots, need, DecodeParameters(max_new_tokens=max(SESSION_NEW)), ignore_eos=True) as sess:
        for i, m in enumerate(SESSION_NEW):
            assert sess.admit(*pages[i], max_new_tokens=m) == i
        for _ in range(8):
            for st in sorted(sess.step(4), key=lambda s: -s.slot):
                if st.done:
                    ids, moved = sess.retire(st.slot)
                    out[owner[st.slot]] = ids
                    if moved >= 0:
                        owner[st.slot] = owner[moved]
                    owner.pop()
            if not owner:
                break
        assert not owner
    return [out[0], out[1]]


@pytest.fixture(scope="module")
def fresh(gpu):
    """Each call as the first call on an engine of its own: computed once, never changed."""
    pages = _pages()
    ref = {}
    for name, call in (("batch3", _batch3), ("sampled1", _sampled1), ("session", lambda e, p: _session(e, p, 2))):
        eng = _load()
        try:
            ref[name] = call(eng, pages)
        finally:
            eng.close()
    assert [len(x) for x in ref["batch3"]] == [10, 10, 10] and [len(x) for x in ref["session"]] == SESSION_NEW
    return pages, ref


def test_one_engine_across_generate_session_profile(fresh):
    pages, ref = fresh
    eng = _load()
    try:
        assert _batch3(eng, pages) == ref["batch3"]
        assert _session(eng, pages, 2) == ref["session"]
        assert _sampled1(eng, pages) == ref["sampled1"]
        prof = eng.profile_decode(1)
        assert prof["tokens"] == 1
        timed = [k for k, v in prof.items() if isinstance(v, dict) and v["launches"] > 0]
        assert {"attention", "lm_head", "qkv", "o_proj"} <= set(timed)
        for k in timed:
            assert math.isfinite(prof[k]["avg_us"]) and prof[k]["avg_us"] > 0, (k, prof[k])
        assert _batch3(eng, pages) == ref["batch3"]
        # a second session, with more slots than the first and than the generate before it: it reserves its rows again
        # and nothing grows once they are frozen (a growth is an EINTERNAL error from the admission or the step)
        assert _session(eng, pages, 3) == ref["session"]
    finally:
        eng.close()
