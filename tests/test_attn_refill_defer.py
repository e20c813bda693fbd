"""Deferred sentinel refill of the one-page fused q/k/v + attention launch (dec_qkv_attn).

Two hand-off copies alternate by layer: launch l polls copy l & 1, leaves the q / k / v and record words it read
as they are, and the next launch's projection blocks write the sentinel over them (the last launch of a step
refills its own copy).  Invariant: at every step boundary every word of both copies holds the sentinel.

* kernel level (dsocr_k_qkv_attention_layers; 128-dim MHA heads, 2 heads, hidden 256): sequences of 1..4 launches
  with 1 / 63 / 64 / 65 / 129 cached keys give bitwise the context rows and appended K / V rows of the in-launch
  refill (whose arithmetic test_gpu_kernels.py checks against f64 math), leave both copies sentinel-filled and the
  give-up flag 0.  The 3- and 4-launch sequences poll a copy that another launch cleaned.
* engine level: a 3-layer model on which the fused launch runs (the tiny config with two 128-dim heads): 16 greedy
  tokens of a page alone, and of the same page in a session that a second page joins and leaves (one-page steps,
  two-page steps, one-page steps again), equal the ids of a process started with DSOCR_ATT_REFILL_DEFER=0 and
  the oracle's.
"""
import ctypes as C
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # the DSOCR_ATT_REFILL_DEFER=0 child of test_three_layers_and_session_handover
    for _p in (ROOT, os.path.join(ROOT, "deepseek-ocr.rs_amd"), os.path.join(ROOT, "tests")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

from _dev import Dev, f16_bits
from dsocr._lib import check, lib

pytestmark = pytest.mark.gpu

SENT = 0x7FBADBAD  # DSOCR_HANDOFF_SENTINEL
H, HEADS, HD = 256, 2, 128
MAX_LEN = 131      # 3 chunks of 64 keys: at 1 cached key two of them leave at once, at 129 all three run
LAYERS = [1, 2, 3, 4]
CACHED = [1, 63, 64, 65, 129]


@functools.lru_cache(maxsize=None)
def _inputs(cached):
    """Weights, rows and caches of four layers with `cached` keys each (the slots from `cached` on hold NaN)."""
    from types import SimpleNamespace
    from oracle.decoder import rope_tables
    rng = np.random.default_rng(1000 + cached)
    n = max(LAYERS)
    x = rng.standard_normal((n, H)).astype(np.float32)
    nw = (1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32)
    w = f16_bits(rng.standard_normal((n, 3 * H, H)) * 0.05)
    kc = rng.standard_normal((n, HEADS, MAX_LEN, HD)).astype(np.float32)
    vc = rng.standard_normal((n, HEADS, MAX_LEN, HD)).astype(np.float32)
    kc[:, :, cached:] = np.nan
    vc[:, :, cached:] = np.nan
    cos, sin = rope_tables(SimpleNamespace(rope_theta=10000.0), MAX_LEN, HD)
    return x, nw, w, kc, vc, cos, sin


@functools.lru_cache(maxsize=None)
def _run(layers, cached, defer):
    """One sequence of `layers` fused launches, every one decoding position `cached` of its own layer's cache:
    (context rows, K caches, V caches, both q/k/v copies, both record copies, give-up flag)."""
    x, nw, w, kc, vc, cos, sin = _inputs(cached)
    pos = np.full(layers, cached, np.int32)
    dx, dn, dw, dcos, dsin, dp = Dev(x), Dev(nw), Dev(w), Dev(cos), Dev(sin), Dev(pos)
    dk, dv, do = Dev(kc), Dev(vc), Dev.zeros((layers, H))
    pw = HEADS * ((MAX_LEN + 63) // 64) * (HD + 4)
    rows, parts, err = np.zeros((2, 3 * H), np.uint32), np.zeros((2, pw), np.uint32), C.c_int(-1)
    check(lib().dsocr_k_qkv_attention_layers(defer, layers, H, HEADS, HD, MAX_LEN, 1.0 / math.sqrt(HD), 1e-6, dx.ptr,
                                             dn.ptr, dw.ptr, 1, dcos.ptr, dsin.ptr, dk.ptr, dv.ptr, dp.ptr, do.ptr,
                                             rows.ctypes.data_as(C.c_void_p), parts.ctypes.data_as(C.c_void_p),
                                             C.byref(err)))
    return do.get(), dk.get(), dv.get(), rows, parts, err.value


@pytest.mark.parametrize("cached", CACHED)
@pytest.mark.parametrize("layers", LAYERS)
def test_deferred_equals_in_launch_refill(gpu, layers, cached):
    _, _, _, kc, vc, _, _ = _inputs(cached)
    o1, k1, v1 = _run(layers, cached, 1)[:3]
    o0, k0, v0 = _run(layers, cached, 0)[:3]
    assert np.all(np.isfinite(o1)), "a sentinel or a stale slot reached a context row"
    assert np.array_equal(o1.view(np.uint32), o0.view(np.uint32))
    for got, ref, src in ((k1, k0, kc), (v1, v0, vc)):
        new = got[:layers, :, cached]
        assert np.all(np.isfinite(new))
        assert np.array_equal(new.view(np.uint32), ref[:layers, :, cached].view(np.uint32))
        # nothing else in any cache was written: the launched layers' other slots, the layers not launched
        keep = np.ones(got.shape[:3], bool)
        keep[:layers, :, cached] = False
        assert np.array_equal(got.view(np.uint32)[keep], src.view(np.uint32)[keep])


@pytest.mark.parametrize("defer", [1, 0])
@pytest.mark.parametrize("cached", CACHED)
@pytest.mark.parametrize("layers", LAYERS)
def test_both_copies_end_sentinel_filled(gpu, layers, cached, defer):
    rows, parts, err = _run(layers, cached, defer)[3:]
    assert err == 0, "a polling block gave up"
    for c in range(2):
        assert np.all(rows[c] == SENT), f"q/k/v copy {c}: {int(np.sum(rows[c] != SENT))} words are not the sentinel"
        assert np.all(parts[c] == SENT), f"record copy {c}: {int(np.sum(parts[c] != SENT))} words are not the sentinel"


# ------------------------------------------------------------------ engine level
SEED, N_NEW, N_NEW_GUEST = 7, 16, 4
PROMPT = "<image>\nConvert the document to markdown."


def _config(path):
    """The tiny config with two 128-dim heads (hidden 256): 3 decoder layers on the fused one-page launch."""
    import dsocr
    cfg = json.load(open(dsocr.TINY_CONFIG))
    cfg["language_config"].update(hidden_size=H, num_attention_heads=HEADS, num_key_value_heads=HEADS)
    cfg["projector_config"]["n_embed"] = H
    assert cfg["language_config"]["num_hidden_layers"] == 3
    with open(path, "w") as f:
        json.dump(cfg, f)
    return cfg


def _images():
    return [np.random.default_rng(s).integers(0, 256, hw + (3,), dtype=np.uint8) for s, hw in ((0, (300, 420)), (1, (256, 256)))]


def _prompt_ids(n_image_tokens):
    from dsocr import build_prompt_tokens
    from dsocr.synth import SyntheticTokenizer
    return build_prompt_tokens(SyntheticTokenizer(512), PROMPT, [n_image_tokens])


def _scenario(config_path):
    """ids of the host page alone, of the guest page alone, and of both from a session: host admitted, 3 one-page
    steps, guest admitted (two-page steps), guest retired when done, one-page steps to the end."""
    from dsocr import DecodeParameters, ModelLoadArgs, Page, VisionSettings, load_model
    eng = load_model(ModelLoadArgs(config_path=config_path, synthetic_seed=SEED, dtype="f16", device=0))
    try:
        vs = VisionSettings(256, 128, True)
        reqs = []
        for img in _images():
            page = Page(img, vs)
            reqs.append(_prompt_ids(page.n_image_tokens) + (page,))
        new = [N_NEW, N_NEW_GUEST]
        out = {"single": [eng.generate(ids, mask, page, None, DecodeParameters(max_new_tokens=m))
                          for (ids, mask, page), m in zip(reqs, new)]}
        need = max(len(r[0]) + m + 1 for r, m in zip(reqs, new))
        got, owner = {}, [0]
        with eng.open_session(2, need, DecodeParameters(max_new_tokens=N_NEW)) as sess:
            sess.admit(*reqs[0], max_new_tokens=new[0])
            sess.step(3)
            sess.admit(*reqs[1], max_new_tokens=new[1])
            owner.append(1)
            for _ in range(N_NEW + 2):
                if not owner:
                    break
                for st in sorted(sess.step(3), key=lambda s: -s.slot):
                    if st.done:
                        ids, moved = sess.retire(st.slot)
                        got[owner[st.slot]] = ids
                        if moved >= 0:
                            owner[st.slot] = owner[moved]
                        owner.pop()
            assert not owner
        out["session"] = [got[0], got[1]]
        return out
    finally:
        eng.close()


def test_three_layers_and_session_handover(gpu, tmp_path):
    from dsocr import Page, VisionSettings
    from oracle.model import OracleModel
    from oracle.weights import Weights
    path = str(tmp_path / "tiny_hd128.json")
    cfg = _config(path)
    # the fused launch is what runs at this shape (else both settings would take the same two launches)
    x, nw, w, kc, vc, cos, sin = _inputs(1)
    d = [Dev(a) for a in (x, nw, w, cos, sin, kc, vc, np.array([1], np.int32), np.full(3 * H, SENT, np.uint32),
                          np.zeros(H, np.float32))]
    used = C.c_int(-1)
    check(lib().dsocr_k_qkv_attention(1, 1, H, HEADS, HD, MAX_LEN, 1.0 / math.sqrt(HD), 1e-6, d[0].ptr, d[1].ptr,
                                      d[2].ptr, 1, d[3].ptr, d[4].ptr, d[5].ptr, d[6].ptr, d[7].ptr, d[8].ptr, d[9].ptr,
                                      C.byref(used)))
    assert used.value == 1
    assert os.environ.get("DSOCR_ATT_REFILL_DEFER", "1") != "0", "this test compares the default with the switch at 0"
    deferred = _scenario(path)
    env = dict(os.environ, DSOCR_ATT_REFILL_DEFER="0")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True,
                           timeout=300)
    assert child.returncode == 0, child.stderr[-2000:]
    in_launch = json.loads(child.stdout.strip().splitlines()[-1])
    assert deferred == in_launch
    orc = OracleModel(cfg, Weights(seed=SEED, dtype="f16"))
    for img, m, single, sess in zip(_images(), [N_NEW, N_NEW_GUEST], deferred["single"], deferred["session"]):
        emb, _ = orc.image_embeddings(img, 256, 128, True)
        ids, mask = _prompt_ids(Page(img, VisionSettings(256, 128, True)).n_image_tokens)
        ref, _ = orc.generate(ids, mask, emb, m, eos_token_id=1)
        assert single == ref
        assert sess == ref
    assert len(deferred["single"][0]) == N_NEW, "the host page is expected to run all 16 steps (no early eos)"


if __name__ == "__main__":
    print(json.dumps(_scenario(sys.argv[1])))
