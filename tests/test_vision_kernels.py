"""The vision tower's kernels (SAM -> CLIP -> projector, the OCR-2 encoder's row ops) in the forms the engine
launches them, through the kernel-level entry points, against numpy in f64 or exact integer / bit moves.

Poison rule: every output buffer enters filled with one NaN bit pattern; whatever the contract says is not written
(ld padding columns, rows whose scatter index is -1 or that no index names, rows of done pages) must come back
bit-identical.  Input padding columns hold NaN as well: a kernel that reads them spoils its result.

Tolerances:
  f32a GEMM  |got - ref| <= 2e-5 * sum_k |a_k w_k| + 1e-6 (doubled under an activation) + 1e-5 |ref|
             (test_gpu_kernels.py's per-element bound)
  norms      1e-5 relative, as test_layernorm / test_rmsnorm
  attention  2e-5 absolute without bias, 5e-5 with the rel-pos bias, on standard-normal q / k / v
  rel-pos    hd * 2^-23 * sum_d |q_d r_d| per entry (an fmaf chain of hd terms)
  ocr2 rope  3 * 2^-24 * (|x1 c| + |x2 s|) per element (three roundings, which the compiler may fuse)
  scatter invariance, data movement: bit for bit.

Which kernel a case reaches (launch_gemm_f32a / launch_splitk_reduce / launch_attention / launch_sam_relbias):
  GEMM   splits 1: the GEMM's own epilogue scatters; splits > 1 and N % 4 == 0 and M <= 65535: splitk_reduce4_kernel;
         otherwise splitk_reduce_kernel (N = 770 / 130, M = 65537)
  attn   hd 64, bidirectional, uniform L: attention_split_kernel<REL>; hd 128: attention_fwd2_kernel<128, false>;
         hd 32: attention_fwd_kernel<32>
  bias   hd 64: sam_relbias2_kernel<64> (tables in LDS); hd 32: sam_relbias_kernel
"""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from _dev import Dev, bf16_round, bf16_to_f32, f16_bits
from dsocr import ModelLoadArgs, Page, VisionSettings, load_model
from dsocr import _lib as L
from dsocr._lib import check, lib
from oracle.model import OracleModel
from oracle.vision import conv2d_nhwc
from oracle.weights import Weights
from test_gpu_kernels import ACTS, _attn_ref, _bound, _weights

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY64 = os.path.join(ROOT, "deepseek-ocr.rs_amd", "dsocr", "configs", "tiny64.json")
POISON = 0x7FA5C3E1  # a NaN no kernel here produces


def _poison(shape):
    return np.full(shape, POISON, np.uint32).view(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _padded(a, ld):
    """rows of a in a buffer of row stride ld, NaN in the padding columns"""
    out = np.full((a.shape[0], ld), np.nan, np.float32)
    out[:, :a.shape[1]] = a
    return out


def _window_maps(n, g, W):
    nw = -(-g // W)
    t2w = np.empty(n * g * g, np.int32)
    w2t = np.empty(n * nw * nw * W * W, np.int32)
    check(lib().dsocr_window_maps(n, g, W, t2w.ctypes.data_as(C.c_void_p), w2t.ctypes.data_as(C.c_void_p)))
    return t2w, w2t


def _row_map(rng, rows, cap, kind):
    """None; 'perm': a permutation of cap == rows targets; 'drop': injective into cap rows, ~1/8 of the rows dropped"""
    if kind is None:
        return None
    if kind == "perm":
        assert cap == rows
        return rng.permutation(rows).astype(np.int32)
    m = rng.permutation(cap)[:rows].astype(np.int32)
    m[rng.random(rows) < 0.125] = -1
    m[0] = -1
    return m


# ================================================================================ f32a GEMM, engine form
def _gemm_ex(a, bits, wdt, bias, c0, c_rows, act, acc, variant, splits, lda=None):
    """C0 [c_cap][ldc] -> (C after the call, split count used)"""
    M, K = a.shape
    N = bits.shape[0]
    lda = lda or K
    dA, dW, dB, dC = Dev(_padded(a, lda)), Dev(bits), Dev(bias), Dev(c0)
    dR = Dev(c_rows) if c_rows is not None else None
    used = C.c_int(-1)
    check(lib().dsocr_k_gemm_f32a_ex(M, N, K, dA.ptr, lda, dW.ptr, wdt, dB.ptr, dC.ptr, c0.shape[1],
                                     dR.ptr if dR else None, c0.shape[0], act, acc, variant, splits, C.byref(used)))
    return dC.get(), used.value


def _gemm_case(M, N, K, wdt, act, acc, variant, splits, lda_pad, ldc_pad, rows_kind, c_rows=None, c_cap=None,
               nan_dropped=False):
    rng = np.random.default_rng(M * 7 + N + K + splits)
    a = rng.standard_normal((M, K)).astype(np.float32)
    bits, w = _weights(rng, N, K, wdt)
    bias = rng.standard_normal(N).astype(np.float32) * 0.1
    if c_rows is None:
        c_cap = M if rows_kind in (None, "perm") else M + 20
        c_rows = _row_map(rng, M, c_cap, rows_kind)
    dst = np.arange(M) if c_rows is None else c_rows
    kept = dst >= 0
    if nan_dropped:  # a dropped row's product must go nowhere
        a[~kept] = np.nan
    c0 = _poison((c_cap, N + ldc_pad))
    if acc:
        c0[dst[kept], :N] = rng.standard_normal((int(kept.sum()), N)).astype(np.float32)
    got, used = _gemm_ex(a, bits, wdt, bias, c0, c_rows, act, acc, variant, splits, K + lda_pad)
    ak = a[kept]
    ref = ACTS[act]((ak.astype(np.float64) @ w.T.astype(np.float64)).astype(np.float32) + bias)
    if acc:
        ref = ref + c0[dst[kept], :N]
    bound = _bound(ak, w) * (2.0 if act else 1.0) + 1e-5 * np.abs(ref)
    err = np.abs(got[dst[kept], :N].astype(np.float64) - ref)
    print(f"gemm_f32a M={M} N={N} K={K} wdt={wdt} act={act} acc={acc} variant={variant} splits={splits}->{used} "
          f"max err {err.max():.3e} max err/bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound), (np.max(err), np.max(err / bound))
    # not written: the padding columns of written rows, every row no index names
    want = c0.copy()
    want[dst[kept], :N] = got[dst[kept], :N]
    assert _same_bits(got, want), "a dropped row or a padding column of C was written"
    return used


@pytest.mark.parametrize("N", [768, 770])
def test_gemm_f32a_sam_proj_form(gpu, N):
    """A SAM window block's proj + residual: the 784 window rows of one 16 x 16 grid (256 kept, 528 padding rows
    dropped) scattered through win2tok into x, bias, accumulate, the engine's split count (> 1 here), so the scatter,
    the bias and the residual add all run in the split-K reduce: four columns per thread at N = 768, the scalar
    kernel at N = 770."""
    _, w2t = _window_maps(1, 16, 14)
    assert w2t.size == 784 and int((w2t >= 0).sum()) == 256
    used = _gemm_case(784, N, 768, 0, 0, 1, 0, 0, 0, 0, "win2tok", c_rows=w2t, c_cap=256, nan_dropped=True)
    assert used > 1


def test_gemm_f32a_forced_splits_two_reduce_batches(gpu):
    """9 slices (more than one batch of 8 in splitk_reduce4_kernel), c_rows a permutation, GELU, accumulate"""
    assert _gemm_case(300, 512, 1152, 0, 1, 1, 0, 9, 0, 0, "perm") == 9


def test_gemm_f32a_rows_beyond_grid_y(gpu):
    """M = 65537 > 65535 rows: the reduce cannot take one row per grid.y and falls back to the scalar kernel"""
    assert _gemm_case(65537, 64, 64, 0, 0, 1, 0, 2, 0, 0, "perm") == 2


@pytest.mark.parametrize("M,N,K,wdt,act,acc,variant,splits,lda_pad,ldc_pad,rows_kind", [
    (300, 130, 96, 0, 0, 1, 0, 1, 0, 0, "drop"),     # one slice: the GEMM's own epilogue scatters
    (300, 130, 96, 0, 1, 0, 0, 1, 4, 3, None),       # lda = K + 4, ldc = N + 3, no reduce
    (300, 132, 96, 0, 0, 1, 0, 3, 4, 3, "drop"),     # ... through splitk_reduce4_kernel
    (300, 130, 96, 0, 2, 1, 0, 3, 4, 3, "perm"),     # ... through splitk_reduce_kernel
    (129, 256, 1280, 1, 3, 1, 0, 0, 0, 0, "drop"),   # f16 weights, the engine's count (16: two reduce batches)
    (77, 130, 64, 1, 0, 0, 0, 1, 4, 0, None),        # f16 weights, one slice
    (300, 512, 256, 0, 0, 1, 2, 1, 0, 0, "drop"),    # variant 2 (two LDS stages), one slice
    (300, 512, 256, 0, 1, 0, 2, 4, 4, 3, "perm")])   # variant 2, four slices
def test_gemm_f32a_forms(gpu, M, N, K, wdt, act, acc, variant, splits, lda_pad, ldc_pad, rows_kind):
    used = _gemm_case(M, N, K, wdt, act, acc, variant, splits, lda_pad, ldc_pad, rows_kind)
    assert used == (splits if splits else 16)


@pytest.mark.parametrize("N,wdt,splits", [(128, 0, 1), (128, 0, 4), (130, 0, 3), (128, 1, 2), (128, 0, 0)])
def test_gemm_f32a_scatter_invariance(gpu, N, wdt, splits):
    """The run with c_rows equals, bit for bit, the run without it at the same split count scattered on the host;
    the rows of C no index names are unchanged."""
    M, K, cap = 300, 256, 320
    rng = np.random.default_rng(N + wdt + splits)
    a = rng.standard_normal((M, K)).astype(np.float32)
    bits, _ = _weights(rng, N, K, wdt)
    bias = rng.standard_normal(N).astype(np.float32) * 0.1
    res = rng.standard_normal((M, N)).astype(np.float32)
    rows = _row_map(rng, M, cap, "drop")
    kept = rows >= 0
    plain, used0 = _gemm_ex(a, bits, wdt, bias, res.copy(), None, 1, 1, 0, splits)
    c0 = _poison((cap, N))
    c0[rows[kept]] = res[kept]
    got, used1 = _gemm_ex(a, bits, wdt, bias, c0, rows, 1, 1, 0, splits)
    assert used0 == used1 and (splits == 0 or used1 == splits)
    want = c0.copy()
    want[rows[kept]] = plain[kept]
    assert _same_bits(got, want)


def test_gemm_fallback_row_scatter(gpu):
    """Engine::linear's fallback (K % 32 != 0: launch_gemm) with a row scatter that drops rows"""
    M, N, K, cap = 150, 72, 40, 170
    rng = np.random.default_rng(40)
    a = rng.standard_normal((M, K)).astype(np.float32)
    bits, w = _weights(rng, N, K, 0)
    bias = rng.standard_normal(N).astype(np.float32) * 0.1
    rows = _row_map(rng, M, cap, "drop")
    kept = rows >= 0
    c0 = _poison((cap, N))
    c0[rows[kept]] = rng.standard_normal((int(kept.sum()), N)).astype(np.float32)
    dA, dW, dB, dC, dR, dO = Dev(a), Dev(bits), Dev(bias), Dev(c0), Dev(rows), Dev(np.array([0, M], np.int32))
    check(lib().dsocr_k_gemm_grouped(M, N, K, dA.ptr, K, None, dW.ptr, 0, 0, dB.ptr, 0, dC.ptr, N, dR.ptr, 0, 1, dO.ptr,
                                     1, M, 0))
    got = dC.get()
    ref = (a[kept].astype(np.float64) @ w.T.astype(np.float64)).astype(np.float32) + bias + c0[rows[kept]]
    assert np.all(np.abs(got[rows[kept]] - ref) <= _bound(a[kept], w) + 1e-5 * np.abs(ref))
    want = c0.copy()
    want[rows[kept]] = got[rows[kept]]
    assert _same_bits(got, want)


# ================================================================================ norms
def _ln_ref(x, w, b, eps):
    x = x.astype(np.float64)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * w.astype(np.float64) + b.astype(np.float64)


def _rms_ref(x, w, eps):
    x = x.astype(np.float64)
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * w.astype(np.float64)


def _layernorm_ex(x, ldx, w, b, eps, y0, out_rows=None, inplace=False):
    rows, cols = x.shape
    dx, dw, db = Dev(_padded(x, ldx)), Dev(w), Dev(b)
    dy = dx if inplace else Dev(y0)
    dr = Dev(out_rows) if out_rows is not None else None
    ldy, yrows = (ldx, rows) if inplace else (y0.shape[1], y0.shape[0])
    check(lib().dsocr_k_layernorm_ex(rows, cols, dx.ptr, ldx, dw.ptr, db.ptr, eps, dy.ptr, ldy, dr.ptr if dr else None,
                                     yrows))
    return dy.get()


def _ln_inputs(rows, cols, offset=False):
    rng = np.random.default_rng(rows * 131 + cols)
    x = (100 + rng.standard_normal((rows, cols)) if offset else rng.standard_normal((rows, cols)) * 3 + 1)
    return rng, x.astype(np.float32), rng.standard_normal(cols).astype(np.float32), rng.standard_normal(cols).astype(np.float32)


def _norm_close(got, ref):
    err = np.max(np.abs(got - ref))
    print(f"norm max err {err:.3e} of {1e-5 * (1 + np.max(np.abs(ref))):.3e}")
    return err <= 1e-5 * (1 + np.max(np.abs(ref)))


@pytest.mark.parametrize("form", ["strided", "inplace", "scatter", "offset"])
@pytest.mark.parametrize("rows", [1, 5, 257])
@pytest.mark.parametrize("cols", [64, 260, 768, 1024])
def test_layernorm_forms(gpu, cols, rows, form):
    """strided: ldx = cols + 4, ldy = cols + 8, eps 1e-5 (CLIP); inplace: y == x at ldx = cols + 4, eps 1e-6 (the neck,
    the CLIP pre-norm); scatter: out_rows with -1 entries into a larger buffer; offset: rows with mean >> standard
    deviation (x = 100 + N(0, 1)), which a one-pass variance would lose."""
    rng, x, w, b = _ln_inputs(rows, cols, form == "offset")
    eps = 1e-5 if form == "strided" else 1e-6
    ref = _ln_ref(x, w, b, eps)
    if form == "inplace":
        got = _layernorm_ex(x, cols + 4, w, b, eps, None, inplace=True)
        assert _norm_close(got[:, :cols], ref)
        assert np.all(np.isnan(got[:, cols:])), "the padding columns were written"
        return
    if form == "scatter":
        cap = rows + 3
        m = rng.permutation(cap)[:rows].astype(np.int32)
        if rows > 1:
            m[rows // 2] = -1
        y0 = _poison((cap, cols + 8))
        got = _layernorm_ex(x, cols, w, b, eps, y0, out_rows=m)
        kept = m >= 0
        assert _norm_close(got[m[kept], :cols], ref[kept])
        want = y0.copy()
        want[m[kept], :cols] = got[m[kept], :cols]
        assert _same_bits(got, want)
        plain = _layernorm_ex(x, cols, w, b, eps, _poison((rows, cols)))
        assert _same_bits(got[m[kept], :cols], plain[kept]), "the scattered rows differ from the unscattered run"
        return
    y0 = _poison((rows, cols + 8))
    got = _layernorm_ex(x, cols + 4, w, b, eps, y0)
    assert _norm_close(got[:, :cols], ref)
    assert _same_bits(got[:, cols:], y0[:, cols:])


@pytest.mark.parametrize("cols", [128, 768])
def test_layernorm_window_partition(gpu, cols):
    """norm1 of a SAM window block: the 256 token rows of a 16 x 16 grid scattered through tok2win into the zeroed
    784-row window buffer; the 528 padding rows stay zero."""
    t2w, _ = _window_maps(1, 16, 14)
    rng, x, w, b = _ln_inputs(256, cols)
    got = _layernorm_ex(x, cols, w, b, 1e-6, np.zeros((784, cols), np.float32), out_rows=t2w)
    assert _norm_close(got[t2w], _ln_ref(x, w, b, 1e-6))
    pad = np.ones(784, bool)
    pad[t2w] = False
    assert pad.sum() == 528 and not _bits(got[pad]).any()
    plain = _layernorm_ex(x, cols, w, b, 1e-6, _poison((256, cols)))
    assert _same_bits(got[t2w], plain)


@pytest.mark.parametrize("form", ["strided", "inplace"])
@pytest.mark.parametrize("rows", [1, 5, 706])
@pytest.mark.parametrize("cols", [64, 260, 896, 1280])
def test_rmsnorm_forms(gpu, cols, rows, form):
    rng = np.random.default_rng(rows * 17 + cols)
    x = (rng.standard_normal((rows, cols)) * 0.5).astype(np.float32)
    w = (1 + rng.standard_normal(cols) * 0.05).astype(np.float32)
    ref = _rms_ref(x, w, 1e-6)
    ldx = cols + 4
    dx, dw = Dev(_padded(x, ldx)), Dev(w)
    if form == "inplace":
        check(lib().dsocr_k_rmsnorm_ex(rows, cols, dx.ptr, ldx, dw.ptr, 1e-6, dx.ptr, ldx))
        got = dx.get()
        assert np.all(np.isnan(got[:, cols:]))
    else:
        y0 = _poison((rows, cols + 8))
        dy = Dev(y0)
        check(lib().dsocr_k_rmsnorm_ex(rows, cols, dx.ptr, ldx, dw.ptr, 1e-6, dy.ptr, cols + 8))
        got = dy.get()
        assert _same_bits(got[:, cols:], y0[:, cols:])
    assert np.max(np.abs(got[:, :cols] - ref)) <= 1e-5 * np.max(np.abs(ref))


# ================================================================================ attention on the fused buffer
def _rel_tables(rng, gh, gw, hd):
    return (rng.standard_normal((2 * gh - 1, hd)).astype(np.float32) * 0.2,
            rng.standard_normal((2 * gw - 1, hd)).astype(np.float32) * 0.2)


def _rel_gather(tab, g):
    """[2g-1][hd] -> R[q][k] = tab[q - k + g - 1]"""
    i = np.arange(g)
    return tab[i[:, None] - i[None, :] + g - 1].astype(np.float64)


def _fused_attention_case(n_seq, L, heads, hd, grid, ld_pad):
    rng = np.random.default_rng(L * heads + hd + ld_pad)
    Cw = heads * hd
    ld, o_ld = 3 * Cw + ld_pad, Cw + 4
    qkv = rng.standard_normal((n_seq * L, 3 * Cw)).astype(np.float32)   # every (sequence, head) its own q / k / v
    o0 = _poison((n_seq * L, o_ld))
    dq, do = Dev(_padded(qkv, ld)), Dev(o0)
    scale = 1.0 / math.sqrt(hd)
    if grid:
        gh, gw = grid
        th, tw = _rel_tables(rng, gh, gw, hd)
        dh, dw = Dev(th), Dev(tw)
        check(lib().dsocr_k_attention_fused(n_seq, L, heads, hd, scale, dq.ptr, ld, do.ptr, o_ld, dh.ptr, dw.ptr, gh, gw))
        Rh, Rw = _rel_gather(th, gh), _rel_gather(tw, gw)
    else:
        check(lib().dsocr_k_attention_fused(n_seq, L, heads, hd, scale, dq.ptr, ld, do.ptr, o_ld, None, None, 0, 0))
    got = do.get()
    assert _same_bits(got[:, Cw:], o0[:, Cw:]), "the padding columns of o were written"
    worst = 0.0
    for s in range(n_seq):
        for h in range(heads):
            sl = slice(s * L, (s + 1) * L)
            q, k, v = (qkv[sl, i * Cw + h * hd:i * Cw + (h + 1) * hd] for i in range(3))
            bias = None
            if grid:
                qg = q.reshape(gh, gw, hd).astype(np.float64)
                rel_h = np.einsum("hwc,hkc->hwk", qg, Rh)
                rel_w = np.einsum("hwc,wkc->hwk", qg, Rw)
                bias = (rel_h[:, :, :, None] + rel_w[:, :, None, :]).reshape(L, L)
            ref = _attn_ref(q, k, v, scale, False, bias)
            err = np.max(np.abs(got[sl, h * hd:(h + 1) * hd] - ref))
            worst = max(worst, err)
            assert err < (5e-5 if grid else 2e-5), (s, h, err)
    print(f"attention n_seq={n_seq} L={L} hd={hd} grid={grid} ld_pad={ld_pad}: max err {worst:.3e}")


@pytest.mark.parametrize("ld_pad", [0, 8])
@pytest.mark.parametrize("n_seq,L,grid", [(4, 196, (14, 14)),   # SAM windows
                                          (2, 256, (16, 16)),   # SAM global block of a 256 px view
                                          (3, 5, None), (3, 17, None), (3, 257, None)])  # CLIP
def test_attention_fused_hd64(gpu, n_seq, L, grid, ld_pad):
    """The production towers' attention (attention_split_kernel) as Engine::vision_pass launches it: q | k | v views
    of one buffer of row stride 3C (+ 8), several sequences, a rel-pos table per (sequence, head)."""
    _fused_attention_case(n_seq, L, 2, 64, grid, ld_pad)


@pytest.mark.parametrize("hd,L,grid", [(128, 100, None), (32, 196, (14, 14))])
def test_attention_fused_other_head_dims(gpu, hd, L, grid):
    _fused_attention_case(2, L, 2, hd, grid, 8)


@pytest.mark.parametrize("hd", [64, 32])
def test_sam_relbias_table(gpu, hd):
    """launch_sam_relbias on the q columns of a fused buffer, a 10 x 14 grid (gh != gw), 3 sequences, 2 heads"""
    n_seq, gh, gw, heads = 3, 10, 14, 2
    Lq, Cw, R = gh * gw, heads * hd, gh + gw
    rng = np.random.default_rng(hd)
    qkv = rng.standard_normal((n_seq * Lq, 3 * Cw)).astype(np.float32)
    th, tw = _rel_tables(rng, gh, gw, hd)
    dq, dh, dw, dout = Dev(qkv), Dev(th), Dev(tw), Dev(_poison((n_seq, heads, Lq, R)))
    check(lib().dsocr_k_sam_relbias(n_seq, gh, gw, heads, hd, dq.ptr, 3 * Cw, dh.ptr, dw.ptr, dout.ptr))
    got = dout.get().astype(np.float64)
    q = qkv[:, :Cw].reshape(n_seq, gh, gw, heads, hd).astype(np.float64)
    Rh, Rw = _rel_gather(th, gh), _rel_gather(tw, gw)
    ref_h = np.einsum("shwnc,hkc->snhwk", q, Rh)
    ref_w = np.einsum("shwnc,wkc->snhwk", q, Rw)
    mag_h = np.einsum("shwnc,hkc->snhwk", np.abs(q), np.abs(Rh))
    mag_w = np.einsum("shwnc,wkc->snhwk", np.abs(q), np.abs(Rw))
    ref = np.concatenate([ref_h, ref_w], -1).reshape(n_seq, heads, Lq, R)
    bound = hd * 2.0 ** -23 * np.concatenate([mag_h, mag_w], -1).reshape(n_seq, heads, Lq, R)
    assert np.all(np.abs(got - ref) <= bound), np.max(np.abs(got - ref) / bound)


# ================================================================================ data movement
def _vis(op, dims, bufs):
    d = (C.c_longlong * len(dims))(*dims)
    p = (C.c_void_p * len(bufs))(*[b.ptr.value for b in bufs])
    check(lib().dsocr_k_vision_op(op, d, len(dims), p, len(bufs)))


@pytest.mark.parametrize("n,H,W", [(2, 64, 64), (1, 32, 64), (6, 512, 512)])
def test_patch_im2col(gpu, n, H, W):
    """(6, 512, 512) has more elements than 16384 blocks x 256 threads: the grid-stride loop's second trip"""
    ps = 16
    gh, gw = H // ps, W // ps
    img = np.random.default_rng(H + W).standard_normal((n, 3, H, W)).astype(np.float32)
    assert (n, H) != (6, 512) or img.size > 16384 * 256
    dimg, dcols = Dev(img), Dev(_poison((n * gh * gw, 3 * ps * ps)))
    _vis(L.VIS_PATCH_IM2COL, [n, H, W, ps], [dimg, dcols])
    # oracle.vision.Sam.forward's patch rows
    ref = img.reshape(n, 3, gh, ps, gw, ps).transpose(0, 2, 4, 1, 3, 5).reshape(n * gh * gw, 3 * ps * ps)
    assert _same_bits(dcols.get(), ref)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("H,W,Cc", [(16, 16, 8), (15, 15, 12), (10, 14, 4)])
def test_conv_im2col_nhwc(gpu, H, W, Cc, stride):
    n, k, pad = 2, 3, 1
    x = np.random.default_rng(H * W + Cc).standard_normal((n, H, W, Cc)).astype(np.float32)
    oh, ow = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    K = k * k * Cc
    # the cols conv2d_nhwc builds, read out through an identity weight: out = cols @ I (every sum is one value + zeros)
    eye = np.eye(K, dtype=np.float32).reshape(K, k, k, Cc).transpose(0, 3, 1, 2)
    ref = conv2d_nhwc(x, eye, stride, pad).reshape(n * oh * ow, K)
    dx, dcols = Dev(x), Dev(_poison((n * oh * ow, K)))
    _vis(L.VIS_CONV_IM2COL_NHWC, [n, H, W, Cc, k, k, stride, pad], [dx, dcols])
    assert np.array_equal(dcols.get(), ref)


def test_add_broadcast(gpu):
    rng = np.random.default_rng(3)
    rows, cols, reps = 37, 24, 3
    x = rng.standard_normal((reps, rows, cols)).astype(np.float32)
    t = rng.standard_normal((rows, cols)).astype(np.float32)
    dt, dx = Dev(t), Dev(x)
    _vis(L.VIS_ADD_BROADCAST, [rows, cols, reps], [dt, dx])
    assert _same_bits(dx.get(), x + t[None])


def test_clip_embed(gpu):
    rng = np.random.default_rng(4)
    n, S, Cw = 2, 16, 64
    sam = rng.standard_normal((n, S, Cw)).astype(np.float32)
    cls = rng.standard_normal(Cw).astype(np.float32)
    pos = rng.standard_normal((S + 1, Cw)).astype(np.float32)
    dsam, dcls, dpos, dout = Dev(sam), Dev(cls), Dev(pos), Dev(_poison((n, S + 1, Cw)))
    _vis(L.VIS_CLIP_EMBED, [n, S, Cw], [dsam, dcls, dpos, dout])
    ref = np.concatenate([np.broadcast_to(cls, (n, 1, Cw)), sam], 1) + pos[None]
    assert _same_bits(dout.get(), ref)


def test_concat_clip_sam(gpu):
    rng = np.random.default_rng(5)
    n, S, C1, C2 = 2, 16, 64, 32
    clip = rng.standard_normal((n, S + 1, C1)).astype(np.float32)
    sam = rng.standard_normal((n, S, C2)).astype(np.float32)
    dclip, dsam, dout = Dev(clip), Dev(sam), Dev(_poison((n, S, C1 + C2)))
    _vis(L.VIS_CONCAT_CLIP_SAM, [n, S, C1, C2], [dclip, dsam, dout])
    assert _same_bits(dout.get(), np.concatenate([clip[:, 1:], sam], -1))


def _table(rng, rows, H, dt):
    t = rng.standard_normal((rows, H)).astype(np.float32)
    if dt == 0:
        bits = bf16_round(t)
        return bits, bf16_to_f32(bits)
    bits = f16_bits(t)
    return bits, bits.view(np.float16).astype(np.float32)


@pytest.mark.parametrize("dt", [0, 1])
def test_assemble_rows(gpu, dt):
    """all five kinds in one call, H = 200 in rows of stride 208"""
    rng = np.random.default_rng(6 + dt)
    rows, H, ld = 41, 200, 208
    bits, tab = _table(rng, 50, H, dt)
    srcA = rng.standard_normal((20, H)).astype(np.float32)
    srcB = rng.standard_normal((10, H)).astype(np.float32)
    vecA, vecB = (rng.standard_normal(H).astype(np.float32) for _ in range(2))
    kind = np.concatenate([np.arange(5), rng.integers(0, 5, rows - 5)]).astype(np.int32)
    index = np.array([rng.integers(0, (50, 20, 10, 1, 1)[k]) for k in kind], np.int32)
    dst0 = _poison((rows, ld))
    bufs = [Dev(kind), Dev(index), Dev(bits), Dev(srcA), Dev(srcB), Dev(vecA), Dev(vecB), Dev(dst0)]
    _vis(L.VIS_ASSEMBLE_ROWS, [rows, H, dt, ld], bufs)
    want = dst0.copy()
    for r in range(rows):
        want[r, :H] = (tab[index[r]], srcA[index[r] % 20], srcB[index[r] % 10], vecA, vecB)[kind[r]]
    assert _same_bits(bufs[-1].get(), want)


@pytest.mark.parametrize("dt", [0, 1])
def test_embed_tokens(gpu, dt):
    rng = np.random.default_rng(8 + dt)
    n, H, ld = 9, 200, 208
    bits, tab = _table(rng, 50, H, dt)
    ids = rng.integers(0, 50, n).astype(np.int32)
    out0 = _poison((n, ld))
    dtab, dids, dout = Dev(bits), Dev(ids), Dev(out0)
    _vis(L.VIS_EMBED_TOKENS, [n, H, dt, ld], [dtab, dids, dout])
    want = out0.copy()
    want[:, :H] = tab[ids]
    assert _same_bits(dout.get(), want)


def test_trace_logits(gpu):
    """three pages: one running (its row lands at trace[0][out_len]), one done, one with out_len >= steps; V beyond
    one trip of the 64 x 256 grid, rows of stride ld > V"""
    rng = np.random.default_rng(9)
    B, V, ld, steps = 3, 20000, 20008, 4
    logits = rng.standard_normal((B, V)).astype(np.float32)
    out_len = np.array([1, 2, 4], np.int32)
    done = np.array([0, 1, 0], np.int32)
    tr0 = _poison((B, steps, V))
    dl, dn, dd, dt = Dev(_padded(logits, ld)), Dev(out_len), Dev(done), Dev(tr0)
    _vis(L.VIS_TRACE_LOGITS, [B, V, ld, steps], [dl, dn, dd, dt])
    want = tr0.copy()
    want[0, 1] = logits[0]
    assert _same_bits(dt.get(), want)


def test_ocr2_build_seq_and_take_queries(gpu):
    rng = np.random.default_rng(10)
    n, P, D = 2, 16, 64
    feat = rng.standard_normal((n, P, D)).astype(np.float32)
    query = rng.standard_normal((P, D)).astype(np.float32)
    dfeat, dquery, dseq = Dev(feat), Dev(query), Dev(_poison((n, 2 * P, D)))
    _vis(L.VIS_OCR2_BUILD_SEQ, [n, P, D], [dfeat, dquery, dseq])
    seq = np.concatenate([feat, np.broadcast_to(query, (n, P, D))], 1)
    assert _same_bits(dseq.get(), seq)
    src = rng.standard_normal((n, 2 * P, D)).astype(np.float32)
    dsrc, ddst = Dev(src), Dev(_poison((n, P, D)))
    _vis(L.VIS_OCR2_TAKE_QUERIES, [n, P, D], [dsrc, ddst])
    assert _same_bits(ddst.get(), src[:, P:])


@pytest.mark.parametrize("hd", [32, 64])
def test_ocr2_rope(gpu, hd):
    """the first 3 of 5 heads' worth of columns rotated at position row % L, the rest untouched"""
    rng = np.random.default_rng(hd)
    Lr, n_heads, half = 32, 3, hd // 2
    rows, ld = 2 * Lr, 5 * hd
    x = rng.standard_normal((rows, ld)).astype(np.float32)
    cos, sin = (rng.uniform(-1, 1, (Lr, hd)).astype(np.float32) for _ in range(2))
    dcos, dsin, dx = Dev(cos), Dev(sin), Dev(x)
    _vis(L.VIS_OCR2_ROPE, [rows, Lr, n_heads, hd, ld], [dcos, dsin, dx])
    got = dx.get()
    assert _same_bits(got[:, n_heads * hd:], x[:, n_heads * hd:])
    pos = np.arange(rows) % Lr
    xh = x[:, :n_heads * hd].reshape(rows, n_heads, hd).astype(np.float64)
    c, s = cos[pos][:, None, :].astype(np.float64), sin[pos][:, None, :].astype(np.float64)
    x1, x2 = xh[..., :half], xh[..., half:]
    ref = np.concatenate([x1 * c[..., :half] - x2 * s[..., :half], x2 * c[..., half:] + x1 * s[..., half:]], -1)
    mag = np.concatenate([np.abs(x1 * c[..., :half]) + np.abs(x2 * s[..., :half]),
                          np.abs(x2 * c[..., half:]) + np.abs(x1 * s[..., half:])], -1)
    err = np.abs(got[:, :n_heads * hd].reshape(rows, n_heads, hd) - ref)
    assert np.all(err <= 3 * 2.0 ** -24 * mag), np.max(err / mag)


# ================================================================================ the engine on tiny64.json
TINY64_VS = VisionSettings(256, 128, True)


@pytest.fixture(scope="module")
def tiny64_engine(gpu):
    eng = load_model(ModelLoadArgs(config_path=TINY64, synthetic_seed=7, dtype="f16"))
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def tiny64_oracle():
    return OracleModel(json.load(open(TINY64)), Weights(seed=7, dtype="f16"))


@pytest.mark.parametrize("hw", [(300, 420), (256, 256), (100, 90)])
def test_tiny64_image_embeddings(tiny64_engine, tiny64_oracle, hw):
    """test_tiny_image_embeddings on towers of head dim 64: the engine path through attention_split_kernel (windows of
    196 rows over grids of 16 and 8, both padded; the global blocks; CLIP) and, with K = 128, a split-K proj with the
    win2tok scatter in the reduce."""
    img = np.random.default_rng(hw[0] + hw[1]).integers(0, 256, (*hw, 3), dtype=np.uint8)
    page = Page(img, TINY64_VS)
    got = tiny64_engine.image_embeddings([page])[0]
    ref, crop = tiny64_oracle.image_embeddings(img, 256, 128, True)
    assert page.crop_shape == crop
    assert got.shape == ref.shape
    assert np.max(np.abs(got - ref)) < 1e-3 * max(1.0, np.max(np.abs(ref)))
