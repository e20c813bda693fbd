"""f16 KV cache with its own decode attention kernel (DSOCR_LOAD_KV_F16, decode_attn16.hip):
K / V rounded once at append (nearest even, clamped to +-65504), all else f32, the step's own key / value unrounded."""
import json
import math
from types import SimpleNamespace

import numpy as np
import pytest

from _dev import Dev
from dsocr import DecodeParameters, ModelLoadArgs, Page, VisionSettings, build_prompt_tokens, load_model
from dsocr._lib import DsocrError, check, lib
from dsocr.synth import SyntheticTokenizer
from oracle.decoder import Decoder, apply_rope, rope_tables
from oracle.model import OracleModel
from oracle.weights import Weights
from test_dsq import SEED, TINY256
from test_dsq_packed import _text_prompts
from test_fp8_experts import N_NEW, _load

f32, f16, f64 = np.float32, np.float16, np.float64
NAN16 = 0x7E00
SHAPES = [(128, 2, 2), (128, 4, 2), (64, 2, 2), (32, 4, 4)]  # (hd, heads, kv_heads)
LANG = SimpleNamespace(rope_theta=10000.0)


def _rotated(qkv, pos, heads, kvh, hd, cos, sin):
    """The q | k columns of each row rotated at the row's position (numpy), v as it is."""
    rot, n = qkv.copy(), (heads + kvh) * hd
    for b, p in enumerate(pos):
        rot[b, :n] = apply_rope(qkv[b, :n].reshape(heads + kvh, hd), cos[p][None], sin[p][None], False).reshape(-1)
    return rot


def _call(fn, B, heads, kvh, hd, max_len, qkv, cos, sin, kc, vc, pos, prerot):
    """One decode-attention hook call on host arrays: (o, k cache, v cache) afterwards."""
    d = [Dev(a) for a in (qkv, cos, sin, kc, vc, np.asarray(pos, np.int32))]
    do = Dev.zeros((B, heads * hd))
    check(fn(B, heads, kvh, hd, hd, max_len, 1.0 / math.sqrt(hd), *[x.ptr for x in d], do.ptr, prerot))
    return do.get(), d[3].get(), d[4].get()


@pytest.mark.gpu
@pytest.mark.parametrize("prerot", [1, 0])
@pytest.mark.parametrize("hd", [128, 32])
def test_append_rounds_once(gpu, hd, prerot):
    """prerot = 1 (no device arithmetic on k): row pos of both caches is np.float16 of the clamped row bit for bit,
    with an exact tie (1 + 2^-11 -> 1, 1 + 3 2^-11 -> 1 + 2^-9), an f16 subnormal, +-1e6 (-> +-65504) and +-0 planted;
    every other row keeps its bits.  prerot = 0: the device rotates in f32, so k is within one f16 ulp."""
    B, heads, kvh, max_len, pos = 2, 2, 2, 200, [5, 130]
    rng = np.random.default_rng(hd + prerot)
    qkv = rng.standard_normal((B, (heads + 2 * kvh) * hd)).astype(f32)
    plant = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 3e-6, 1e6, -1e6, 0.0, -0.0], f32)
    for h in range(2 * kvh):  # every k and v head row
        qkv[:, (heads + h) * hd + 3:(heads + h) * hd + 3 + len(plant)] = plant
    cos, sin = rope_tables(LANG, max_len, hd)
    kc0 = rng.standard_normal((B, kvh, max_len, hd)).astype(f16).view(np.uint16)
    vc0 = rng.standard_normal((B, kvh, max_len, hd)).astype(f16).view(np.uint16)
    rot = _rotated(qkv, pos, heads, kvh, hd, cos, sin)
    _, gk, gv = _call(lib().dsocr_k_decode_attention_kv16, B, heads, kvh, hd, max_len, rot if prerot else qkv, cos, sin,
                      kc0, vc0, pos, prerot)
    want = np.clip(rot[:, heads * hd:], -65504, 65504).astype(f16).reshape(B, 2, kvh, hd)
    for b, p in enumerate(pos):
        assert np.array_equal(gv[b, :, p], want[b, 1].view(np.uint16))
        if prerot:
            assert np.array_equal(gk[b, :, p], want[b, 0].view(np.uint16))
        else:
            got, w64 = gk[b, :, p].view(f16).astype(f64), want[b, 0].astype(f64)
            ulp = np.maximum(np.spacing(np.abs(w64).astype(f32)).astype(f64) * 2.0 ** 13, 2.0 ** -24)  # f16 spacing
            assert np.all(np.abs(got - w64) <= ulp)
        others = np.arange(max_len) != p
        assert np.array_equal(gk[b][:, others], kc0[b][:, others]) and np.array_equal(gv[b][:, others], vc0[b][:, others])


def _ref64(q, K, V, scale):
    s = (K.astype(f64) @ q.astype(f64)) * scale
    p = np.exp(s - s.max())
    return (p / p.sum()) @ V.astype(f64)


@pytest.mark.gpu
@pytest.mark.parametrize("lens", [(1, 128, 300), (127, 129, 300)])
@pytest.mark.parametrize("prerot", [0, 1])
@pytest.mark.parametrize("hd,heads,kvh", SHAPES)
def test_attention_against_f64(gpu, hd, heads, kvh, prerot, lens):
    """Three pages in one launch (a single key, a full 128-key chunk, the own position first in a new chunk, ragged
    chunks; max_len 400 leaves whole chunks past every length; rows at and past pos enter as f16 NaN), then a second
    launch one position on over the caches the first left.  Reference: f64 softmax attention over the f16 rows read
    back, the new k / v unrounded.  Bar: 4 x the error of dsocr_k_decode_attention on f32 caches holding the same
    rows (both sum exact products in f32 in another order), (len + hd) 2^-24 max|v| where that error is 0."""
    B, max_len, scale = 3, 400, 1.0 / math.sqrt(hd)
    rng = np.random.default_rng(hd + heads + prerot + lens[0])
    cos, sin = rope_tables(LANG, max_len, hd)
    pos = np.array(lens) - 1
    kc = rng.standard_normal((B, kvh, max_len, hd)).astype(f16).view(np.uint16)
    vc = rng.standard_normal((B, kvh, max_len, hd)).astype(f16).view(np.uint16)
    for b in range(B):
        kc[b, :, pos[b]:] = vc[b, :, pos[b]:] = NAN16
    for step in range(2):
        qkv = rng.standard_normal((B, (heads + 2 * kvh) * hd)).astype(f32)
        rot = _rotated(qkv, pos, heads, kvh, hd, cos, sin)
        args = (B, heads, kvh, hd, max_len, rot if prerot else qkv, cos, sin)
        k32, v32 = kc.view(f16).astype(f32), vc.view(f16).astype(f32)
        o16, kc, vc = _call(lib().dsocr_k_decode_attention_kv16, *args, kc, vc, pos, prerot)
        o32, _, _ = _call(lib().dsocr_k_decode_attention, *args, k32, v32, pos, prerot)
        assert not np.isnan(o16).any()
        ref = np.zeros((B, heads * hd))
        for b, p in enumerate(pos):
            for h in range(heads):
                g = h // (heads // kvh)
                K, V = k32[b, g, :p + 1].copy(), v32[b, g, :p + 1].copy()
                K[p] = rot[b, (heads + g) * hd:(heads + g + 1) * hd]
                V[p] = qkv[b, (heads + kvh + g) * hd:(heads + kvh + g + 1) * hd]
                ref[b, h * hd:(h + 1) * hd] = _ref64(rot[b, h * hd:(h + 1) * hd], K, V, scale)
        e16, e32 = float(np.max(np.abs(o16 - ref))), float(np.max(np.abs(o32 - ref)))
        floor = (int(pos.max()) + 1 + hd) * 2.0 ** -24 * max(np.nanmax(np.abs(v32)), np.max(np.abs(qkv[:, (heads + kvh) * hd:])))
        print(f"kv16 hd {hd} heads {heads}/{kvh} prerot {prerot} lens {(pos + 1).tolist()}: {e16:.3e}, f32 kernel {e32:.3e}")
        assert e16 <= 4 * (e32 if e32 > 0 else floor), (step, e16, e32)
        pos = pos + 1


class _RoundedCacheDecoder(Decoder):
    """The oracle decoder storing f16(K) / f16(V): prefill and a step's own row unrounded, the stored rows rounded."""

    def attention(self, li, x):
        out = super().attention(li, x)
        self.k_cache[li] = np.clip(self.k_cache[li], -65504, 65504).astype(f16).astype(f32)
        self.v_cache[li] = np.clip(self.v_cache[li], -65504, 65504).astype(f16).astype(f32)
        return out


@pytest.mark.gpu
def test_engine_matches_oracle_with_rounded_cache(gpu):
    """tiny256 (hd 128), test_fp8_mm's seed, prompts, N_NEW and 2e-3 logit bar (no id flipped, so no other seed was
    needed): greedy ids at 1, 3 and 8 prompts and an image page equal the oracle's with a rounded cache; the cache is
    2 bytes per element and half the f32 engine's bytes for the same requests; a session is refused."""
    cfg, params, prompts = json.load(open(TINY256)), DecodeParameters(max_new_tokens=N_NEW), _text_prompts(8)
    reqs = lambda n: [(p, None, None, None) for p in prompts[:n]]
    img = np.random.default_rng(5).integers(0, 256, (300, 260, 3), dtype=np.uint8)
    page = Page(img, VisionSettings(256, 128, True))
    pids, pmask = build_prompt_tokens(SyntheticTokenizer(512), "<image>\nConvert the document to markdown.",
                                      [page.n_image_tokens])
    eng = _load(dtype="f16", kv_dtype="f16")
    try:
        assert eng.kv_info() == {"elem_bytes": 2, "cache_bytes": 0}
        with pytest.raises(DsocrError, match="EINVAL.*f32 KV cache"):
            eng.open_session(2, 64, params)
        got_page = eng.generate(pids, pmask, page, None, params)
        trace = {n: eng.generate_trace(reqs(n), params, ignore_eos=True) for n in (1, 3, 8)}
        got = {n: eng.generate_batch(reqs(n), params, ignore_eos=True) for n in (1, 3, 8)}
        bytes16 = eng.kv_info()["cache_bytes"]
        assert eng.profile_decode(1)["tokens"] == 8  # (the profile's save / restore of the slot at pos - 1)
    finally:
        eng.close()
    for kv in ("f32", None):
        eng = _load(dtype="f16", kv_dtype=kv)
        try:
            assert eng.kv_info()["elem_bytes"] == 4
            if kv:
                eng.generate_batch(reqs(8), params, ignore_eos=True)
                assert eng.kv_info()["cache_bytes"] == 2 * bytes16 > 0
        finally:
            eng.close()
    oracle = OracleModel(cfg, Weights(seed=SEED, dtype="f16"))
    oracle.dec = _RoundedCacheDecoder(cfg, oracle.W)
    emb, _ = oracle.image_embeddings(img, 256, 128, True)
    assert got_page == oracle.generate(pids, pmask, emb, N_NEW, eos_token_id=1, no_repeat_ngram_size=20)[0]
    refs = [oracle.generate(p, np.zeros(len(p), np.uint8), None, N_NEW, eos_token_id=None, ignore_eos=True,
                            record_logits=True) for p in prompts]
    for n, (ids, lg) in trace.items():
        assert ids == got[n] == [r[0] for r in refs[:n]], (n, ids)
        err = max(float(np.max(np.abs(lg[i, s] - refs[i][1][s]))) for i in range(n) for s in range(N_NEW))
        print(f"f16 KV engine vs oracle with a rounded cache, {n} prompt(s): max abs logit diff {err:.3e}")
        assert err < 2e-3, (n, err)


def test_kv_dtype_refused():
    with pytest.raises(DsocrError, match="kv_dtype"):
        load_model(ModelLoadArgs(config_path=TINY256, kv_dtype="f8"))


@pytest.mark.gpu
def test_kv16_hook_refuses_other_head_dims(gpu):
    z = np.zeros(1, f32)
    with pytest.raises(DsocrError, match="EINVAL"):
        _call(lib().dsocr_k_decode_attention_kv16, 1, 2, 2, 48, 64, z, z, z, z, z, [0], 1)
