"""n samples of one page (generate_n; decode_attn_shared.hip): the decode rows share the prompt's
K/V in page 0 and each owns only its tail."""
import json
import math

import numpy as np
import pytest

from _dev import Dev
from dsocr import DecodeParameters, Page, VisionSettings, build_prompt_tokens, server
from dsocr._lib import DsocrError, check, lib
from dsocr.synth import SyntheticTokenizer
from oracle.decoder import rope_tables
from oracle.model import OracleModel
from oracle.weights import Weights
from test_dsq import SEED, TINY256
from test_fp8_experts import N_NEW, _load
from test_kv_f16 import LANG, SHAPES, _ref64, _rotated

f32, f64 = np.float32, np.float64
OFFSETS = [0, 1, 127, 128, 129, 200, 255, 256]  # row b decodes at shared_len + OFFSETS[b]


def _call(B, heads, kvh, hd, max_len, qkv, cos, sin, kc, vc, pos, prerot, shared=None):
    """One decode-attention hook call on host arrays (shared: the shared-prompt hook): (o, k cache, v cache) afterwards."""
    d = [Dev(a) for a in (qkv, cos, sin, kc, vc, np.asarray(pos, np.int32))]
    do = Dev.zeros((B, heads * hd))
    head = (B, heads, kvh, hd, hd, max_len, 1.0 / math.sqrt(hd), *[x.ptr for x in d])
    if shared is None:
        check(lib().dsocr_k_decode_attention(*head, do.ptr, prerot))
    else:
        check(lib().dsocr_k_decode_attention_shared(*head, shared, do.ptr, prerot))
    return do.get(), d[3].get(), d[4].get()


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 127, 128, 129, 300])
@pytest.mark.parametrize("B", [2, 5, 8])
@pytest.mark.parametrize("prerot", [0, 1])
@pytest.mark.parametrize("hd,heads,kvh", SHAPES)
def test_attention_against_f64(gpu, hd, heads, kvh, prerot, B, P):
    """Ragged rows (row 0 at shared_len: no own key but the step's; own chunks empty, full, starting at the own
    position), max_len 600.  Rows [0, P) of pages 1 .. B - 1 and every row at or past a row's position enter as NaN:
    no NaN in the output proves only page 0's prompt rows are read.  A second launch one position on over the caches
    the first left covers the append; every row but the appended one keeps its bits.  Reference: f64 softmax attention
    over page 0's prompt rows + the row's own rows + the unrounded new key / value.  Bar: 4 x the error of
    dsocr_k_decode_attention on caches with the prompt rows copied into every page (both sum exact f32 products in
    another order), (len + hd) 2^-24 max|v| where that error is 0."""
    max_len, scale = 600, 1.0 / math.sqrt(hd)
    rng = np.random.default_rng(hd + heads + prerot + 7 * B + P)
    cos, sin = rope_tables(LANG, max_len, hd)
    pos = P + np.array(OFFSETS[:B])
    kc = rng.standard_normal((B, kvh, max_len, hd)).astype(f32)
    vc = rng.standard_normal((B, kvh, max_len, hd)).astype(f32)
    for b in range(B):
        kc[b, :, pos[b]:] = vc[b, :, pos[b]:] = np.nan
    kf, vf = kc.copy(), vc.copy()  # the f32 kernel's caches: the prompt rows in every page
    kf[1:, :, :P], vf[1:, :, :P] = kc[0, :, :P], vc[0, :, :P]
    kc[1:, :, :P] = vc[1:, :, :P] = np.nan
    for step in range(2):
        qkv = rng.standard_normal((B, (heads + 2 * kvh) * hd)).astype(f32)
        rot = _rotated(qkv, pos, heads, kvh, hd, cos, sin)
        args = (B, heads, kvh, hd, max_len, rot if prerot else qkv, cos, sin)
        o, k1, v1 = _call(*args, kc, vc, pos, prerot, shared=P)
        o32, kf, vf = _call(*args, kf, vf, pos, prerot)
        assert not np.isnan(o).any()
        ref = np.zeros((B, heads * hd))
        for b, p in enumerate(pos):
            knew, vnew = rot[b, heads * hd:(heads + kvh) * hd].reshape(kvh, hd), qkv[b, (heads + kvh) * hd:].reshape(kvh, hd)
            keep = np.arange(max_len) != p
            assert np.array_equal(k1[b][:, keep].view(np.uint32), kc[b][:, keep].view(np.uint32))
            assert np.array_equal(v1[b][:, keep].view(np.uint32), vc[b][:, keep].view(np.uint32))
            assert np.array_equal(v1[b, :, p], vnew)
            assert np.array_equal(k1[b, :, p], knew) if prerot else np.allclose(k1[b, :, p], knew, rtol=0, atol=1e-6)
            for h in range(heads):
                g = h // (heads // kvh)
                K = np.concatenate([kc[0, g, :P], kc[b, g, P:p], knew[g][None]])
                V = np.concatenate([vc[0, g, :P], vc[b, g, P:p], vnew[g][None]])
                ref[b, h * hd:(h + 1) * hd] = _ref64(rot[b, h * hd:(h + 1) * hd], K, V, scale)
        e, e32 = float(np.max(np.abs(o - ref))), float(np.max(np.abs(o32 - ref)))
        floor = (int(pos.max()) + 1 + hd) * 2.0 ** -24 * max(np.nanmax(np.abs(vc)), np.max(np.abs(qkv[:, (heads + kvh) * hd:])))
        print(f"shared hd {hd} heads {heads}/{kvh} prerot {prerot} B {B} P {P} step {step}: {e:.3e}, f32 kernel {e32:.3e}, "
              f"ratio {e / e32 if e32 else float('nan'):.2f}")
        assert e <= 4 * (e32 if e32 > 0 else floor), (step, e, e32)
        kc, vc, pos = k1, v1, pos + 1


def _page_request():
    img = np.random.default_rng(5).integers(0, 256, (300, 260, 3), dtype=np.uint8)
    page = Page(img, VisionSettings(256, 128, True))
    ids, mask = build_prompt_tokens(SyntheticTokenizer(512), "<image>\nConvert the document to markdown.",
                                    [page.n_image_tokens])
    return img, page, ids, mask


@pytest.mark.gpu
def test_engine_greedy_rows_equal_generate(gpu):
    """tiny256, the image page of test_engine_matches_oracle_with_rounded_cache: every row of generate_n at n = 2, 3, 8
    (sampling off) equals the oracle's ids, which are generate's; generate and generate_batch afterwards return what
    they returned before (the shared-prompt mode was cleared)."""
    img, page, ids, mask = _page_request()
    params = DecodeParameters(max_new_tokens=N_NEW)
    eng = _load(dtype="f16")
    try:
        one = eng.generate(ids, mask, page, None, params)
        bat = eng.generate_batch([(ids, mask, page, None)] * 3, params)
        got = {n: eng.generate_n(ids, mask, page, n, params) for n in (2, 3, 8)}
        assert eng.generate(ids, mask, page, None, params) == one
        assert eng.generate_batch([(ids, mask, page, None)] * 3, params) == bat == [one] * 3
    finally:
        eng.close()
    oracle = OracleModel(json.load(open(TINY256)), Weights(seed=SEED, dtype="f16"))
    emb, _ = oracle.image_embeddings(img, 256, 128, True)
    ref = oracle.generate(ids, mask, emb, N_NEW, eos_token_id=1, no_repeat_ngram_size=20)[0]
    assert one == ref
    for n, rows in got.items():
        assert rows == [ref] * n, (n, rows)


@pytest.mark.gpu
def test_engine_sampled_rows_equal_generate_with_their_seed(gpu):
    """n = 3 at test_sampling's parameters: sample i equals generate of the page alone with seed i (the two paths
    differ only in the attention's summation order)."""
    _, page, ids, mask = _page_request()
    seeds = [5, 6, 7]
    eng = _load(dtype="f16")
    try:
        for T, k, p in [(0.9, None, 0.95), (1.5, 20, 1.0)]:
            prm = lambda s: DecodeParameters(max_new_tokens=24, do_sample=True, temperature=T, top_k=k, top_p=p, seed=s)
            want = [eng.generate(ids, mask, page, None, prm(s)) for s in seeds]
            assert eng.generate_n(ids, mask, page, 3, prm(0), seeds=seeds) == want
            assert eng.generate_n(ids, mask, page, 3, prm(5)) == want  # no seeds: params.seed + i
        assert len({tuple(w) for w in want}) > 1  # (the seeds do draw different samples)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("hd,P,pos", [(48, 4, [4, 5]), (64, 0, [1, 2]), (64, 4, [4, 3])])
def test_hook_refusals(gpu, hd, P, pos):
    z = np.zeros(4, f32)
    with pytest.raises(DsocrError, match="EINVAL"):
        _call(2, 2, 2, hd, 64, z, z, z, z, z, pos, 1, shared=P)


@pytest.mark.gpu
def test_generate_n_refusals(gpu):
    _, page, ids, mask = _page_request()
    for kv, ns in (("f16", (2,)), (None, (1, 9))):
        eng = _load(dtype="f16", kv_dtype=kv)
        try:
            for n in ns:
                with pytest.raises(DsocrError, match="EINVAL"):
                    eng.generate_n(ids, mask, page, n, DecodeParameters(max_new_tokens=4))
        finally:
            eng.close()


@pytest.mark.parametrize("extra", [{"n": 9}, {"n": 0}, {"n": 2, "stream": True}])
def test_server_refuses_n(extra):
    from starlette.testclient import TestClient
    st = server.ServerState(None, SyntheticTokenizer(512), "deepseek-ocr", VisionSettings(256, 128, True),
                            DecodeParameters(max_new_tokens=8))
    r = TestClient(server.create_app(st)).post("/v1/chat/completions", json={
        "model": "deepseek-ocr", "messages": [{"role": "user", "content": "OCR"}], **extra})
    assert r.status_code == 400 and r.json()["error"]["type"] == "invalid_request_error", r.text
