"""FP8 (E4M3) expert weights for the decode MoE (DSOCR_LOAD_FP8_EXPERTS, decode_f8.hip).

Contract: per expert row one exponent e_r (the smallest with amax 2^-e_r <= 448, clamped to >= -15) and the E4M3
round-to-nearest-even codes of the exactly scaled fp16 weights; the FP8 path is the fp16 engine on
W8 = 2^e_r e4m3(code).  The quantiser is checked bit for bit against a numpy / torch.float8_e4m3fn restatement, the
row dots against W8 (one-hot, exact) and its f64 sums, the layer against the f64 layer on W8, the engine against the
CPU oracle reading W8 through a snapshot-like object.
"""
import ctypes as C
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_dsq import SEED, TINY256
from test_dsq_packed import MOE_CASES, ROOT, _text_prompts

f32 = np.float32
SHAPES = [(4, 16), (5, 96), (3, 1280)]
PLANTS = ["zero", "amax448", "amax448_ulp", "tie", "subnormal", "clamp"]
N_NEW = 12


def f8_ref(w16):
    """The contract's quantiser: exponents (int8), codes (uint8) and W8 (f32) of fp16 rows."""
    import torch
    w = w16.astype(f32)
    amax = np.abs(w).max(axis=1)
    m, ex = np.frexp(amax)  # amax = m 2^ex, m in [0.5, 1); 448 = 0.875 * 2^9
    e = np.where(amax == 0, 0, np.maximum(ex - 9 + (m > 0.875), -15)).astype(np.int32)
    t8 = torch.from_numpy(np.ldexp(w, -e[:, None])).to(torch.float8_e4m3fn)
    return e.astype(np.int8), t8.view(torch.uint8).numpy(), np.ldexp(t8.to(torch.float32).numpy(), e[:, None])


@functools.lru_cache(maxsize=None)
def planted(rows, cols, plant):
    """Seeded N(0, 0.05) fp16 rows; row 0 is the planted one (amax 7 = 448 * 2^-6 unless said otherwise)."""
    w = (np.random.default_rng(rows * cols).standard_normal((rows, cols)) * 0.05).astype(np.float16)
    w[0, 3] = 7.0
    if plant == "zero":
        w[0, :] = 0
    elif plant == "amax448_ulp":
        w[0, 3] = np.nextafter(np.float16(7), np.float16(8))
    elif plant == "tie":  # scaled by 64: 1.0625 and -1.1875, halfway between 1 | 1.125 and 1.125 | 1.25
        w[0, 5], w[0, 6] = 1.0625 / 64, -1.1875 / 64
    elif plant == "subnormal":  # scaled by 64: 3, 2.5 (tie -> 2), 0.5 (tie -> 0) and -0.5 (-> -0) times 2^-9
        w[0, 8:12] = np.array([3, 2.5, 0.5, -0.5]) * 2.0 ** -15
    elif plant == "clamp":  # amax 3 * 2^-24 < 2^-21: e would be -31
        w[0, :] = (np.arange(cols) % 7 - 3) * 2.0 ** -24
    return w, f8_ref(w)


@pytest.mark.gpu
@pytest.mark.parametrize("plant", PLANTS)
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_quantiser_bit_exact(gpu, rows, cols, plant):
    from _dev import Dev
    from dsocr._lib import check, lib
    w, (e, q, _) = planted(rows, cols, plant)
    dw, dq, de = Dev(w.view(np.uint16)), Dev.zeros(w.shape, np.uint8), Dev.zeros((rows,), np.int8)
    check(lib().dsocr_k_fp8_quantize_rows(rows, cols, dw.ptr, dq.ptr, de.ptr))
    assert np.array_equal(de.get(), e)
    zero = lambda c: np.where(c == 0x80, 0, c)  # -0 and +0 are one value
    assert np.array_equal(zero(dq.get()), zero(q)), np.argwhere(zero(dq.get()) != zero(q))[:5]


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 3, 8])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_rows_dot(gpu, rows, cols, T):
    """One-hot x returns W8 exactly (-0 == +0); random x is within the f32 accumulation bound
    (K + 2) 2^-24 sum_k |W8 x| of the f64 sum over the same codes."""
    from _dev import Dev
    from dsocr._lib import check, lib
    _, (e, q, w8) = planted(rows, cols, "subnormal")
    dq, de = Dev(q), Dev(e)

    def dot(x):
        dx, dy = Dev(x), Dev.zeros((T, rows), f32)
        check(lib().dsocr_k_fp8_rows_dot(rows, cols, dq.ptr, de.ptr, T, dx.ptr, dy.ptr))
        return dy.get()
    pick = range(cols) if cols <= 96 else sorted(set(range(16)) | set(range(cols - 16, cols)) | set(range(0, cols, 41)))
    pick = list(pick)
    for i in range(0, len(pick), T):
        c = pick[i:i + T]
        x = np.zeros((T, cols), f32)
        x[np.arange(len(c)), c] = 1.0
        assert np.array_equal(dot(x)[:len(c)].T, w8[:, c]), c
    x = np.random.default_rng(cols + T).standard_normal((T, cols)).astype(f32)
    w64, x64 = w8.astype(np.float64), x.astype(np.float64)
    ratio = np.max(np.abs(dot(x) - x64 @ w64.T) / ((cols + 2) * 2.0 ** -24 * (np.abs(x64) @ np.abs(w64).T)))
    print(f"fp8 rows_dot {rows}x{cols} T={T}: largest error / bound {ratio:.3f}")
    assert ratio <= 1.0, ratio


@functools.lru_cache(maxsize=None)
def _expert_tables(H, E, I, ns):
    """fp16 expert tables of one layer, uniform in +-1/16: routed [E][2I][H], [E][H][I]; shared [2Is][H], [H][Is]."""
    rng = np.random.default_rng(H + E + I)
    tab = lambda *s: (rng.integers(-2048, 2048, s, dtype=np.int16).astype(np.float16) * np.float16(2.0 ** -15))
    return tab(E, 2 * I, H), tab(E, H, I), tab(2 * I * ns, H), tab(H, I * ns)


@pytest.mark.gpu
@pytest.mark.parametrize("case", MOE_CASES)
def test_moe_fp8_matches_f64_layer_on_w8(gpu, case):
    from _dev import Dev
    from dsocr._lib import check, lib
    from oracle.decoder import rms_norm, softmax
    T, H, E, topk, I, ns, norm = case
    Is = I * ns
    rng = np.random.default_rng(700 + T + H + I)  # the activations, router and residual of test_dsq_packed's case
    x = rng.standard_normal((T, H)).astype(f32)
    router = (rng.standard_normal((E, H)) * 0.1).astype(np.float16)
    nw = (1.0 + 0.05 * rng.standard_normal(H)).astype(f32)
    out0 = rng.standard_normal((T, H)).astype(f32)
    gu, dn, sgu, sd = _expert_tables(H, E, I, ns)
    xin = rms_norm(x, nw, 1e-6) if norm else x
    scores = softmax(xin @ router.astype(f32).T)
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
    dev = [Dev(a.view(np.uint16)) for a in (router, gu.reshape(-1, H), dn.reshape(-1, I), sgu, sd)]
    dx, dnw, dout = Dev(x), Dev(nw), Dev(out0)
    ids, wts = np.zeros(T * topk, np.int32), np.zeros(T * topk, f32)
    check(lib().dsocr_k_moe_fp8(T, H, E, topk, I, Is, dx.ptr, dnw.ptr if norm else None, 1e-6, *[d.ptr for d in dev],
                                0, 1.0, dout.ptr, ids.ctypes.data_as(C.c_void_p), wts.ctypes.data_as(C.c_void_p)))
    assert np.array_equal(ids.reshape(T, topk), order)
    err = float(np.max(np.abs(dout.get() - ref)))
    print(f"moe_fp8 {case}: max abs err {err:.3e}")
    assert err < 1e-4, err


class _W8Snapshot:
    """What Weights asks of a snapshot, answering W8 for the expert matrices of every MoE layer and nothing else."""

    def __init__(self, cfg, base):
        from oracle import dsq
        self.shape = {n: (o, i) for n, o, i, _ in dsq.discover_linears(cfg) if ".mlp.experts." in n or ".mlp.shared_experts." in n}
        self.base = base

    def has(self, name):
        return name in self.shape

    def weight(self, name):
        return f8_ref(self.base.get(name, self.shape[name]).astype(np.float16))[2]

    def bias_for(self, name):
        return None


def _load(**kw):
    from dsocr import ModelLoadArgs, load_model
    return load_model(ModelLoadArgs(config_path=TINY256, synthetic_seed=SEED, **kw))


@pytest.mark.gpu
def test_fp8_engine_matches_oracle_on_w8(gpu):
    """tiny256, the synthetic seed and text prompts of test_dsq_packed (no id flipped, so no other seed was needed):
    greedy ids at 1, 3 and 8 prompts equal the oracle's on W8; the traced logits are within 2e-3 of the oracle's
    per-step logits and differ from the unflagged engine's."""
    from dsocr import DecodeParameters
    from oracle.model import OracleModel
    from oracle.weights import Weights
    cfg = json.load(open(TINY256))
    params = DecodeParameters(max_new_tokens=N_NEW)
    prompts = _text_prompts(8)
    reqs = lambda n: [(p, None, None, None) for p in prompts[:n]]
    eng = _load(dtype="f16", expert_fp8=True)
    try:
        info = eng.fp8_info()
        assert info["fp8_layers"] == info["moe_layers"] > 0 and info["fp8_bytes"] > 0, info
        assert eng.packed_info()["packed_layers"] == 0 and eng.packed_mode() == 0
        got = {n: eng.generate_batch(reqs(n), params, ignore_eos=True) for n in (1, 3, 8)}
        trace = {n: eng.generate_trace(reqs(n), params, ignore_eos=True) for n in (1, 3, 8)}
        eng.generate_batch(reqs(1), params, ignore_eos=True)  # both engines profile the state of a one-prompt run
        prof = eng.profile_decode(1)
    finally:
        eng.close()
    eng = _load(dtype="f16", expert_fp8=False)
    try:
        assert eng.fp8_info()["fp8_layers"] == 0
        _, lg16 = eng.generate_trace(reqs(1), params, ignore_eos=True)
        prof16 = eng.profile_decode(1)
    finally:
        eng.close()
    assert prof["moe_gateup_kernel"] == "moe_gateup_f8_kernel" and prof["moe_down_kernel"] == "moe_down_f8_kernel", prof
    for k in ("moe_gateup", "moe_down"):
        assert prof[k]["bytes"] < prof16[k]["bytes"], (k, prof[k]["bytes"], prof16[k]["bytes"])
    snap = _W8Snapshot(cfg, Weights(seed=SEED, dtype="f16"))
    name = next(iter(snap.shape))
    assert np.array_equal(snap.weight(name).astype(np.float16).astype(f32), snap.weight(name))  # round_f16 is the identity
    oracle = OracleModel(cfg, Weights(seed=SEED, dtype="f16", snapshot=snap))
    refs = [oracle.generate(p, np.zeros(len(p), np.uint8), None, N_NEW, eos_token_id=None, ignore_eos=True,
                            record_logits=True) for p in prompts]
    for n, ids in got.items():
        for i in range(n):
            assert ids[i] == refs[i][0], (n, i, ids[i], refs[i][0])
    for n, (ids, lg) in trace.items():
        assert ids == got[n]
        err = max(float(np.max(np.abs(lg[i, s] - refs[i][1][s]))) for i in range(n) for s in range(N_NEW))
        print(f"fp8 engine vs oracle on W8, {n} prompt(s): max abs logit diff {err:.3e}")
        assert err < 2e-3, (n, err)
    assert float(np.max(np.abs(trace[1][1][0, 0] - lg16[0, 0]))) > 0


@pytest.mark.gpu
def test_fp8_switches_and_rejections(gpu, tmp_path):
    from _dev import Dev
    from dsocr._lib import DsocrError, check, lib
    from test_dsq import make_tiny256_snapshot
    snap = str(tmp_path / "t.dsq")
    make_tiny256_snapshot(snap)
    with pytest.raises(DsocrError, match="EINVAL"):
        _load(dtype="f16", snapshot_path=snap, snapshot_packed=True, expert_fp8=True)
    with pytest.raises(DsocrError, match="EINVAL"):
        _load(dtype="f32", expert_fp8=True)
    buf, x, y = Dev(np.zeros(4096, np.uint8)), Dev.zeros((9, 48), f32), Dev.zeros((9, 4), f32)
    with pytest.raises(DsocrError, match="EINVAL"):  # cols % 16 != 0
        check(lib().dsocr_k_fp8_quantize_rows(4, 40, buf.ptr, buf.ptr, buf.ptr))
    with pytest.raises(DsocrError, match="EINVAL"):
        check(lib().dsocr_k_fp8_rows_dot(4, 40, buf.ptr, buf.ptr, 1, x.ptr, y.ptr))
    with pytest.raises(DsocrError, match="EINVAL"):  # T > 8
        check(lib().dsocr_k_fp8_rows_dot(4, 48, buf.ptr, buf.ptr, 9, x.ptr, y.ptr))
    # the environment switch through dsocr_engine_load, in a fresh process
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from dsocr import ModelLoadArgs, load_model\n"
            "e = load_model(ModelLoadArgs(config_path=%r, synthetic_seed=%d, dtype='f16'))\n"
            "print('FP8_LAYERS', e.fp8_info()['fp8_layers']); e.close()\n"
            % (ROOT, os.path.join(ROOT, "deepseek-ocr.rs_amd"), TINY256, SEED))
    for env_val, want in (("1", True), (None, False)):
        env = dict(os.environ)
        env.pop("DSOCR_EXPERT_FP8", None)
        if env_val:
            env["DSOCR_EXPERT_FP8"] = env_val
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        n = int(re.search(r"FP8_LAYERS (\d+)", r.stdout).group(1))
        assert (n > 0) == want, (env_val, n)
