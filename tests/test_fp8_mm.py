"""FP8 expert weights on the matrix cores at 3..8 decode tokens (DSOCR_LOAD_FP8_EXPERTS_MM, decode_f8mm.hip; DESIGN.md
section 4.4.4).  Same contract as test_fp8_experts: the fp16 engine on W8 = 2^e_r e4m3(code), up to summation order.
"""
import ctypes as C
import json

import numpy as np
import pytest

from test_dsq import SEED, TINY256
from test_dsq_packed import _text_prompts
from test_fp8_experts import N_NEW, _W8Snapshot, _expert_tables, _load, f8_ref, planted

f32 = np.float32
MM_SHAPES = [(16, 64), (40, 192), (16, 1280)]  # one tile / one step; ragged last tile, odd steps; 20 steps, K split
MM_MOE_CASES = [(3, 256, 16, 6, 256, 1, False), (5, 256, 16, 6, 64, 2, True), (8, 256, 8, 3, 64, 1, False),
                (8, 1280, 64, 6, 896, 2, True), (1, 256, 8, 3, 64, 1, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 3, 8])
@pytest.mark.parametrize("rows,cols", MM_SHAPES)
def test_mm_rows_dot(gpu, rows, cols, T):
    """One-hot x returns W8 exactly (-0 == +0); random x is within the f32 accumulation bound
    (K + 2) 2^-24 sum_k |W8 x| of the f64 sum over the same codes."""
    from _dev import Dev
    from dsocr._lib import check, lib
    _, (e, q, w8) = planted(rows, cols, "subnormal")
    dq, de = Dev(q), Dev(e)

    def dot(x):
        dx, dy = Dev(x), Dev.zeros((T, rows), f32)
        check(lib().dsocr_k_fp8_mm_rows_dot(rows, cols, dq.ptr, de.ptr, T, dx.ptr, dy.ptr))
        return dy.get()
    # the ends plus an odd stride: every lane group (8 codes), both halves of a block, the first and last step
    pick = sorted(set(range(16)) | set(range(cols - 16, cols)) | set(range(0, cols, 41)))
    for i in range(0, len(pick), T):
        c = pick[i:i + T]
        x = np.zeros((T, cols), f32)
        x[np.arange(len(c)), c] = 1.0
        assert np.array_equal(dot(x)[:len(c)].T, w8[:, c]), c
    x = np.random.default_rng(cols + T).standard_normal((T, cols)).astype(f32)
    w64, x64 = w8.astype(np.float64), x.astype(np.float64)
    ratio = np.max(np.abs(dot(x) - x64 @ w64.T) / ((cols + 2) * 2.0 ** -24 * (np.abs(x64) @ np.abs(w64).T)))
    print(f"fp8 mm_rows_dot {rows}x{cols} T={T}: largest error / bound {ratio:.3f}")
    assert ratio <= 1.0, ratio


def _moe_mm(T, H, E, topk, I, ns, norm):
    """dsocr_k_moe_fp8_mm on test_fp8_experts' layer; returns (status, inputs, outputs)."""
    from _dev import Dev
    from dsocr._lib import lib
    rng = np.random.default_rng(700 + T + H + I)
    x = rng.standard_normal((T, H)).astype(f32)
    router = (rng.standard_normal((E, H)) * 0.1).astype(np.float16)
    nw = (1.0 + 0.05 * rng.standard_normal(H)).astype(f32)
    out0 = rng.standard_normal((T, H)).astype(f32)
    gu, dn, sgu, sd = _expert_tables(H, E, I, ns)
    dev = [Dev(a.view(np.uint16)) for a in (router, gu.reshape(-1, H), dn.reshape(-1, I), sgu, sd)]
    dx, dnw, dout = Dev(x), Dev(nw), Dev(out0)
    ids, wts = np.zeros(T * topk, np.int32), np.zeros(T * topk, f32)
    st = lib().dsocr_k_moe_fp8_mm(T, H, E, topk, I, I * ns, dx.ptr, dnw.ptr if norm else None, 1e-6, *[d.ptr for d in dev],
                                  0, 1.0, dout.ptr, ids.ctypes.data_as(C.c_void_p), wts.ctypes.data_as(C.c_void_p))
    return st, (x, router, nw, out0, gu, dn, sgu, sd), (dout.get(), ids.reshape(T, topk))


@pytest.mark.gpu
@pytest.mark.parametrize("case", MM_MOE_CASES)
def test_moe_fp8_mm_matches_f64_layer_on_w8(gpu, case):
    from dsocr._lib import check
    from oracle.decoder import rms_norm, softmax
    T, H, E, topk, I, ns, norm = case
    Is = I * ns
    st, (x, router, nw, out0, gu, dn, sgu, sd), (got, ids) = _moe_mm(*case)
    check(st)
    xin = rms_norm(x, nw, 1e-6) if norm else x
    scores = softmax(xin @ router.astype(f32).T)
    assert all(len(np.unique(s)) == E for s in scores)  # no ties: an id mismatch can only be the kernel's
    order = np.argsort(-scores, axis=-1, kind="stable")[:, :topk]
    w8 = lambda w: f8_ref(w)[2].astype(np.float64)
    silu = lambda v: v / (1.0 + np.exp(-v))
    x64 = xin.astype(np.float64)
    s_gu, s_d = w8(sgu), w8(sd)
    ref = out0.astype(np.float64) + (silu(x64 @ s_gu[:Is].T) * (x64 @ s_gu[Is:].T)) @ s_d.T
    for t in range(T):
        for e_ in order[t]:
            g = w8(gu[e_])
            ref[t] += float(scores[t, e_]) * (w8(dn[e_]) @ (silu(g[:I] @ x64[t]) * (g[I:] @ x64[t])))
    assert np.array_equal(ids, order)
    err = float(np.max(np.abs(got - ref)))
    print(f"moe_fp8_mm {case}: max abs err {err:.3e}")
    assert err < 1e-4, err


@pytest.mark.gpu
def test_moe_fp8_mm_rejects_misfit(gpu):
    from dsocr._lib import DsocrError, check
    with pytest.raises(DsocrError, match="EINVAL"):  # I = 32 is no whole 64-code step
        check(_moe_mm(3, 256, 8, 3, 32, 1, False)[0])


@pytest.mark.gpu
def test_fp8_mm_engine_matches_oracle_on_w8(gpu):
    """tiny256, the synthetic seed and text prompts of test_fp8_engine_matches_oracle_on_w8 (no id flipped, so no other
    seed was needed): mode 2, greedy ids at 3 and 8 prompts equal the oracle's on W8, traced logits within 2e-3, the
    matrix-core kernels at 8 prompts and the VALU pair at 1; expert_fp8=True stays mode 1 with the VALU pair at 8."""
    from dsocr import DecodeParameters
    from oracle.model import OracleModel
    from oracle.weights import Weights
    cfg = json.load(open(TINY256))
    params = DecodeParameters(max_new_tokens=N_NEW)
    prompts = _text_prompts(8)
    reqs = lambda n: [(p, None, None, None) for p in prompts[:n]]
    names = lambda prof: (prof["moe_gateup_kernel"], prof["moe_down_kernel"])
    eng = _load(dtype="f16", expert_fp8="mm")
    try:
        assert eng.fp8_mode() == 2 and eng.fp8_info()["fp8_layers"] > 0
        trace = {n: eng.generate_trace(reqs(n), params, ignore_eos=True) for n in (3, 8)}
        got = {n: eng.generate_batch(reqs(n), params, ignore_eos=True) for n in (3, 8)}
        assert names(eng.profile_decode(1)) == ("moe_gateup_f8mm_kernel", "moe_down_f8mm_kernel")
        eng.generate_batch(reqs(1), params, ignore_eos=True)
        assert names(eng.profile_decode(1)) == ("moe_gateup_f8_kernel", "moe_down_f8_kernel")
    finally:
        eng.close()
    eng = _load(dtype="f16", expert_fp8=True)
    try:
        assert eng.fp8_mode() == 1
        eng.generate_batch(reqs(8), params, ignore_eos=True)
        assert names(eng.profile_decode(1)) == ("moe_gateup_f8_kernel", "moe_down_f8_kernel")
    finally:
        eng.close()
    oracle = OracleModel(cfg, Weights(seed=SEED, dtype="f16", snapshot=_W8Snapshot(cfg, Weights(seed=SEED, dtype="f16"))))
    refs = [oracle.generate(p, np.zeros(len(p), np.uint8), None, N_NEW, eos_token_id=None, ignore_eos=True,
                            record_logits=True) for p in prompts]
    for n, (ids, lg) in trace.items():
        assert ids == got[n]
        for i in range(n):
            assert ids[i] == refs[i][0], (n, i, ids[i], refs[i][0])
        err = max(float(np.max(np.abs(lg[i, s] - refs[i][1][s]))) for i in range(n) for s in range(N_NEW))
        print(f"fp8 mm engine vs oracle on W8, {n} prompt(s): max abs logit diff {err:.3e}")
        assert err < 2e-3, (n, err)
