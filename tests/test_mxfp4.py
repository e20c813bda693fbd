"""MXFP4 expert weights on the matrix cores at 1..8 decode tokens (DSOCR_LOAD_MXFP4_EXPERTS, decode_f4mm.hip; DESIGN.md
section 4.4.5).

Contract: per row an exponent e_r, per block of 32 a down-shift d_b in 0..12, per weight an E2M1 code; the MXFP4 path is
the fp16 engine on W4 = 2^(e_r - d_b) e2m1(code), up to summation order.  f4_ref restates it in numpy; the quantiser is
checked bit for bit, the row dots against W4 (one-hot, exact) and its f64 sums, the layer against the f64 layer on W4,
the engine against the CPU oracle reading W4 through a snapshot-like object.
"""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest

from test_dsq import SEED, TINY256
from test_dsq_packed import ROOT, _text_prompts
from test_fp8_experts import N_NEW, _expert_tables, _load

f32 = np.float32
GRID = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6])  # the E2M1 magnitudes by code
NEW_SYMBOLS = ["dsocr_engine_fp4_info", "dsocr_k_mxfp4_quantize_rows", "dsocr_k_mxfp4_mm_rows_dot", "dsocr_k_moe_mxfp4",
               "dsocr_k_mxfp4_dequant_rows"]
Q_SHAPES = [(16, 128), (5, 256), (3, 1280)]
PLANTS = ["zero_row", "zero_block", "amax6", "amax6_ulp", "tie", "shift_clamp", "subnormal", "top"]
MM_SHAPES = [(16, 128), (40, 384), (16, 1280)]  # one tile / one block; ragged last tile, odd blocks; ten blocks, K split
MOE_CASES = [(1, 256, 8, 3, 128, 1, True), (3, 256, 16, 6, 256, 1, False), (5, 256, 16, 6, 128, 2, True),
             (8, 256, 8, 3, 128, 1, False), (8, 1280, 64, 6, 896, 2, True),
             (1, 256, 8, 1, 128, 2, False)]  # (the last: one routed slot, so one group: the down launch's direct add)


def _e2m1_codes(a, s):
    """Code magnitudes 0..7 of the scaled magnitudes a (f32, on the grid 2^s): to nearest, ties to the even code."""
    grid = GRID.astype(f32)
    c = sum((a >= g).astype(np.int8) for g in grid[1:])  # the largest grid value <= a, then up if the next one is nearer
    lo, hi = grid[c], grid[np.minimum(c + 1, 7)]
    c = c + ((c < 7) & ((a - lo > hi - a) | ((a - lo == hi - a) & (c % 2 == 1))))  # ... or as near and the even code
    return np.where(np.ldexp(grid[c], s) > 65504, c - 1, c)  # top of the range: the next code down


def f4_ref(w16):
    """The contract's quantiser: (e_r int8 [R], d uint8 [R][K/32], packed codes uint8 [R][K/2], W4 f32 [R][K])."""
    R, K = w16.shape
    w = w16.astype(f32).reshape(R, K // 32, 32)
    amax = np.abs(w).max(axis=2)
    m, ex = np.frexp(amax)  # amax = m 2^ex, m in [0.5, 1): 6 = 0.75 * 2^3
    eb = np.where(amax > 0, ex - 3 + (m > 0.75), -1000)
    er = eb.max(axis=1)
    er = np.where(er == -1000, 0, np.maximum(er, -11))
    d = np.where(amax > 0, np.minimum(er[:, None] - eb, 12), 12)
    s = er[:, None] - d
    # a table of codes per distinct block scale over the 31744 finite fp16 magnitudes (the scaling by 2^-s is exact)
    scales, which = np.unique(s, return_inverse=True)
    mags = np.arange(0x7c00, dtype=np.uint16).view(np.float16).astype(f32)
    lut = np.stack([_e2m1_codes(np.ldexp(mags, -int(sv)), int(sv)) for sv in scales])
    c = lut[which.reshape(R, -1, 1), (w16.view(np.uint16) & 0x7fff).reshape(w.shape)]
    neg = np.signbit(w)
    w4 = np.ldexp(np.where(neg, -GRID[c], GRID[c]), s[:, :, None])
    nib = (c | (neg << 3)).astype(np.uint8).reshape(R, K)
    return er.astype(np.int8), d.astype(np.uint8), nib[:, 0::2] | (nib[:, 1::2] << 4), w4.reshape(R, K).astype(f32)


@functools.lru_cache(maxsize=None)
def planted(rows, cols, plant):
    """Seeded N(0, 0.05) fp16 rows; row 0 is the planted one (block 0's amax 0.375 = 6 * 2^-4 = 1.5 * 2^-2 unless said
    otherwise, so its grid is 2^-4 and "amax6" is also the significand-exactly-1.5 case)."""
    w = (np.random.default_rng(rows * cols).standard_normal((rows, cols)) * 0.05).astype(np.float16)
    w[0, 3] = 0.375
    if plant == "zero_row":
        w[0, :] = 0
    elif plant == "zero_block":
        w[0, 32:64] = 0
    elif plant == "amax6_ulp":
        w[0, 3] = np.nextafter(np.float16(0.375), np.float16(1))
    elif plant == "tie":  # halfway between two codes: the even one is below (2.5, 1.25, 5, 0.25) and above (the rest)
        w[0, 8:16] = np.array([2.5, 1.25, 1.75, 3.5, 0.75, 5, 0.25, -0.25]) / 16
    elif plant == "shift_clamp":  # block 1 is 2^-20 below the row's largest (d would be 20: every code rounds to zero),
        w[0, 32:64] = (np.arange(32) % 7 - 3) * 2.0 ** -23  # block 2 2^-15 below (d would be 15): grid 2^-16, values k / 4
        w[0, 64:96] = (np.arange(32) % 7 - 3) * 2.0 ** -18
    elif plant == "subnormal":  # amax 3 * 2^-24: e_r would be -25; clamped to -11, d = 12, values k / 2
        w[0, :] = (np.arange(cols) % 7 - 3) * 2.0 ** -24
    elif plant == "top":  # 65504 rounds to 4 * 2^14 = 65536, 57344 ties up to it: both take 3 * 2^14
        w[0, 3:6] = [65504, -57344, 40960]
    return w, f4_ref(w)


def test_c_abi_exports_the_mxfp4_symbols():
    header = open(os.path.join(ROOT, "include", "dsocr.h")).read()
    declared = set(re.findall(r"\b(dsocr_[a-z0-9_]+)\s*\(", header))
    from dsocr import ModelLoadArgs
    from dsocr._lib import EXPORTS, LIB_PATH, LOAD_MXFP4_EXPERTS
    L = C.CDLL(LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared and s in EXPORTS and hasattr(L, s), s
    assert LOAD_MXFP4_EXPERTS == 32 and "#define DSOCR_LOAD_MXFP4_EXPERTS 32u" in header
    assert ModelLoadArgs().expert_fp4 is None


@pytest.mark.gpu
@pytest.mark.parametrize("plant", PLANTS)
@pytest.mark.parametrize("rows,cols", Q_SHAPES)
def test_quantiser_bit_exact(gpu, rows, cols, plant):
    from _dev import Dev
    from dsocr._lib import check, lib
    w, (e, d, q, w4) = planted(rows, cols, plant)
    assert np.all(np.isfinite(w4.astype(np.float16))) and np.array_equal(w4.astype(np.float16).astype(f32), w4)
    dw, dq = Dev(w.view(np.uint16)), Dev.zeros(q.shape, np.uint8)
    dd, de = Dev.zeros(d.shape, np.uint8), Dev.zeros((rows,), np.int8)
    check(lib().dsocr_k_mxfp4_quantize_rows(rows, cols, dw.ptr, dq.ptr, dd.ptr, de.ptr))
    assert np.array_equal(de.get(), e)
    assert np.array_equal(dd.get(), d), np.argwhere(dd.get() != d)[:5]
    assert np.array_equal(dq.get(), q), np.argwhere(dq.get() != q)[:5]
    d16 = Dev.zeros(w.shape, np.uint16)  # the write-back over the fp16 rows: W4, value for value (-0 == +0)
    check(lib().dsocr_k_mxfp4_dequant_rows(rows, cols, dq.ptr, dd.ptr, de.ptr, d16.ptr))
    assert np.array_equal(d16.get().view(np.float16).astype(f32), w4)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 3, 8])
@pytest.mark.parametrize("rows,cols", MM_SHAPES)
def test_mm_rows_dot(gpu, rows, cols, T):
    """One-hot x returns W4 exactly (-0 == +0); random x is within the f32 accumulation bound
    (K + 2) 2^-24 sum_k |W4 x| of the f64 sum over the same codes."""
    from _dev import Dev
    from dsocr._lib import check, lib
    _, (e, d, q, w4) = planted(rows, cols, "shift_clamp")
    dq, dd, de = Dev(q), Dev(d), Dev(e)

    def dot(x):
        dx, dy = Dev(x), Dev.zeros((T, rows), f32)
        check(lib().dsocr_k_mxfp4_mm_rows_dot(rows, cols, dq.ptr, dd.ptr, de.ptr, T, dx.ptr, dy.ptr))
        return dy.get()
    # the ends plus an odd stride: every lane group (8 codes), every dword of a lane, every byte select, both nibbles
    pick = sorted(set(range(16)) | set(range(cols - 16, cols)) | set(range(0, cols, 41)))
    for i in range(0, len(pick), T):
        c = pick[i:i + T]
        x = np.zeros((T, cols), f32)
        x[np.arange(len(c)), c] = 1.0
        assert np.array_equal(dot(x)[:len(c)].T, w4[:, c]), c
    x = np.random.default_rng(cols + T).standard_normal((T, cols)).astype(f32)
    w64, x64 = w4.astype(np.float64), x.astype(np.float64)
    ratio = np.max(np.abs(dot(x) - x64 @ w64.T) / ((cols + 2) * 2.0 ** -24 * (np.abs(x64) @ np.abs(w64).T)))
    print(f"mxfp4 mm_rows_dot {rows}x{cols} T={T}: largest error / bound {ratio:.3f}")
    assert ratio <= 1.0, ratio


def _moe(T, H, E, topk, I, ns, norm):
    """dsocr_k_moe_mxfp4 on test_fp8_experts' layer; returns (status, inputs, outputs)."""
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
    st = lib().dsocr_k_moe_mxfp4(T, H, E, topk, I, I * ns, dx.ptr, dnw.ptr if norm else None, 1e-6, *[d.ptr for d in dev],
                                 0, 1.0, dout.ptr, ids.ctypes.data_as(C.c_void_p), wts.ctypes.data_as(C.c_void_p))
    return st, (x, router, nw, out0, gu, dn, sgu, sd), (dout.get(), ids.reshape(T, topk))


@pytest.mark.gpu
@pytest.mark.parametrize("case", MOE_CASES)
def test_moe_mxfp4_matches_f64_layer_on_w4(gpu, case):
    from dsocr._lib import check
    from oracle.decoder import rms_norm, softmax
    T, H, E, topk, I, ns, norm = case
    Is = I * ns
    st, (x, router, nw, out0, gu, dn, sgu, sd), (got, ids) = _moe(*case)
    check(st)
    xin = rms_norm(x, nw, 1e-6) if norm else x
    scores = softmax(xin @ router.astype(f32).T)
    assert all(len(np.unique(s)) == E for s in scores)  # no ties: an id mismatch can only be the kernel's
    order = np.argsort(-scores, axis=-1, kind="stable")[:, :topk]
    w4 = lambda w: f4_ref(w)[3].astype(np.float64)
    silu = lambda v: v / (1.0 + np.exp(-v))
    x64 = xin.astype(np.float64)
    s_gu, s_d = w4(sgu), w4(sd)
    ref = out0.astype(np.float64) + (silu(x64 @ s_gu[:Is].T) * (x64 @ s_gu[Is:].T)) @ s_d.T
    used = {e_: (w4(gu[e_]), w4(dn[e_])) for e_ in np.unique(order)}
    for t in range(T):
        for e_ in order[t]:
            g, dw = used[e_]
            ref[t] += float(scores[t, e_]) * (dw @ (silu(g[:I] @ x64[t]) * (g[I:] @ x64[t])))
    assert np.array_equal(ids, order)
    err = float(np.max(np.abs(got - ref)))
    print(f"moe_mxfp4 {case}: max abs err {err:.3e}")
    assert err < 1e-4, err


@pytest.mark.gpu
def test_moe_mxfp4_rejects_misfit(gpu):
    from dsocr._lib import DsocrError, check
    with pytest.raises(DsocrError, match="EINVAL"):  # I = 64 is no whole 128-code block
        check(_moe(3, 256, 8, 3, 64, 1, False)[0])


class _W4Snapshot:
    """What Weights asks of a snapshot, answering W4 for the expert matrices of every MoE layer and nothing else."""

    def __init__(self, cfg, base):
        from oracle import dsq
        self.shape = {n: (o, i) for n, o, i, _ in dsq.discover_linears(cfg) if ".mlp.experts." in n or ".mlp.shared_experts." in n}
        self.base = base

    def has(self, name):
        return name in self.shape

    def weight(self, name):
        return f4_ref(self.base.get(name, self.shape[name]).astype(np.float16))[3]

    def bias_for(self, name):
        return None


@pytest.mark.gpu
def test_mxfp4_engine_matches_oracle_on_w4(gpu):
    """tiny256, the synthetic seed and text prompts of test_fp8_engine_matches_oracle_on_w8 (no id flipped, so no other
    seed was needed): greedy ids at 1, 3 and 8 prompts equal the oracle's on W4, traced logits within 2e-3, the
    matrix-core pair named at 1 and at 8 prompts."""
    from dsocr import DecodeParameters
    from oracle.model import OracleModel
    from oracle.weights import Weights
    cfg = json.load(open(TINY256))
    params = DecodeParameters(max_new_tokens=N_NEW)
    prompts = _text_prompts(8)
    reqs = lambda n: [(p, None, None, None) for p in prompts[:n]]
    names = {}
    eng = _load(dtype="f16", expert_fp4=True)
    try:
        info = eng.fp4_info()
        assert info["fp4_layers"] == info["moe_layers"] > 0 and info["fp4_bytes"] > 0, info
        assert eng.fp8_mode() == 0 and eng.packed_mode() == 0 and eng.fp8_info()["fp8_layers"] == 0
        trace = {n: eng.generate_trace(reqs(n), params, ignore_eos=True) for n in (1, 3, 8)}
        for n in (8, 1):
            got = eng.generate_batch(reqs(n), params, ignore_eos=True)
            assert got == trace[n][0]
            prof = eng.profile_decode(1)
            names[n] = (prof["moe_gateup_kernel"], prof["moe_down_kernel"])
    finally:
        eng.close()
    assert names[1] == names[8] == ("moe_gateup_f4mm_kernel", "moe_down_f4mm_kernel"), names
    oracle = OracleModel(cfg, Weights(seed=SEED, dtype="f16", snapshot=_W4Snapshot(cfg, Weights(seed=SEED, dtype="f16"))))
    refs = [oracle.generate(p, np.zeros(len(p), np.uint8), None, N_NEW, eos_token_id=None, ignore_eos=True,
                            record_logits=True) for p in prompts]
    for n, (ids, lg) in trace.items():
        for i in range(n):
            assert ids[i] == refs[i][0], (n, i, ids[i], refs[i][0])
        err = max(float(np.max(np.abs(lg[i, s] - refs[i][1][s]))) for i in range(n) for s in range(N_NEW))
        print(f"mxfp4 engine vs oracle on W4, {n} prompt(s): max abs logit diff {err:.3e}")
        assert err < 2e-3, (n, err)


@pytest.mark.gpu
def test_mxfp4_switches_and_rejections(gpu, tmp_path):
    from dsocr import ModelLoadArgs, load_model
    from dsocr._lib import DsocrError
    from test_dsq import make_tiny256_snapshot
    snap = str(tmp_path / "t.dsq")
    make_tiny256_snapshot(snap)
    refused = [dict(snapshot_path=snap, snapshot_packed=True), dict(snapshot_path=snap, snapshot_packed="int8"),
               dict(expert_fp8=True), dict(expert_fp8="mm")]
    for kw in refused:
        with pytest.raises(DsocrError, match="EINVAL"):
            _load(dtype="f16", expert_fp4=True, **kw)
    with pytest.raises(DsocrError, match="EINVAL"):
        _load(dtype="f32", expert_fp4=True)
    tiny = os.path.join(os.path.dirname(TINY256), "tiny.json")  # moe_intermediate_size 32: no layer fits
    with pytest.raises(DsocrError, match="EINVAL"):
        load_model(ModelLoadArgs(config_path=tiny, synthetic_seed=SEED, dtype="f16", expert_fp4=True))
    eng = _load(dtype="f16", expert_fp4=True, kv_dtype="f16")
    try:
        assert eng.fp4_info()["fp4_layers"] > 0 and eng.kv_info()["elem_bytes"] == 2
    finally:
        eng.close()
    eng = _load(dtype="f16", expert_fp4=False)
    try:
        assert eng.fp4_info()["fp4_layers"] == 0
    finally:
        eng.close()
