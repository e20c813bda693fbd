"""Kernel-level tests of the dots.ocr tower's bf16 GEMM (gemm_bf16.hip) and row ops (dots_ops.hip): one launch
through dsocr_k_gemm_bf16 / dsocr_k_dots_op against numpy references with f64 sums, at the smallest shapes
that reach each path (partial tiles, scalar tails, the short-K prologue, the fused epilogues, the scalar
fallbacks of the row kernels).

Every output buffer is pre-filled with the bf16 pattern SENT (2.9e38, no kernel output gets near it), has
ldc > N where the kernel allows it and rows past M: the pattern must survive wherever the kernel may not write.

GEMM reference (out_bf16): s = A64 @ W64^T, v1 = rnd(s), v2 = rnd(v1 + b) with a bias, v3 = rnd(C0 + v2) under
accumulate (rnd = one RNE rounding to bf16).  Two assertions per launch:
  hard bound, every element: |got - ref| <= (2e-5 (|A| @ |W|^T) + 1e-6 + 2^-7 (|v1| + |v2| + |v3|)) (1 + 2^-6)
      (test_gpu_kernels' f32-accumulation bound, plus one bf16 step per rounding step applied);
  flip cap: the share of elements not bit-equal to ref is <= 1e-3.  A dropped or doubled rounding step moves
      several percent of the elements; the f32 accumulation order alone moves < 1e-4 of them
      (test_gemm_reference_margin, which needs no GPU).
Why a whole step and not half of one per rounding: the kernel and the reference both round.  With
d_i = |g_i - v_i| between the kernel's chain g and the reference's v, and half a step of y at most 2^-8 |y|,
d_i <= d_(i-1) + 2^-8 (|g_i| + |v_i|) <= d_(i-1) + 2^-8 (2 |v_i| + d_i), so d_n <= (d_0 + 2^-7 sum |v_i|) /
(1 - 2^-8)^n.  Half a step per rounding (2^-8 sum |v_i|) is not a bound: in page_tail, element (85, 193) has
s = -0.52539066, 5.7e-8 past the tie -0.525390625 on which the f32 accumulator (16-wide blocks, on the CPU) lands
exactly, so rnd gives -0.52734375 for s and -0.5234375 for the accumulator; with b = 0.0905 the chains end at
-0.4375 and -0.43359375, 2^-8 apart, where 2^-8 (|v1| + |v2|) plus the accumulation term is 0.003887.  The
MI355X result is that accumulator chain's, bit for bit.
"""
import functools
import math

import numpy as np
import pytest

from _dev import Dev, bf16_round, bf16_to_f32
from dsocr._lib import (DOTS_BF16_TO_F32, DOTS_GELU, DOTS_LAYERNORM, DOTS_RMSNORM, DOTS_ROPE_QK, DOTS_SWIGLU, DOTS_TO_BF16,
                        EINVAL, check, lib)
from oracle.dots import DotsVision, bf16, gelu_bf16, layer_norm, rms_norm, silu_bf16

gpu_test = pytest.mark.gpu
F32, F64 = np.float32, np.float64
SENT = np.uint16(0x7F5A)   # 2.9e38 as bf16
EPS = 1e-5                 # rms_norm_eps of dsocr/configs/dots-ocr.json
NT1, NT2, PP = 0, 2, 3     # dsocr_k_gemm_bf16 variants; 0 is the 128 x 128 one-stage kernel below 256 ping-pong tiles
KNAME = {NT1: "nt<1>", NT2: "nt<2>", PP: "ping-pong"}


def rnd64(x):
    """f64 -> nearest bf16 in one RNE rounding, returned as f32 (values in the f32 normal range)."""
    u = np.ascontiguousarray(x, F64).view(np.uint64)
    u = ((u + np.uint64((1 << 44) - 1) + ((u >> np.uint64(45)) & np.uint64(1))) >> np.uint64(45)) << np.uint64(45)
    return u.view(F64).astype(F32)


def bits_of(v):
    """bf16-valued f32 -> uint16 bits."""
    return (np.ascontiguousarray(v, F32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_step(v, d):
    """bf16-valued f32 moved d bf16 steps along the number line (+-0 are one point)."""
    b = bits_of(v).astype(np.int32)
    key = np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF) + d
    out = np.where(key < 0, 0x8000 | -key, key).astype(np.uint16)
    return bf16_to_f32(out)


def sentinel(rows, cols):
    return np.full((rows, cols), SENT, np.uint16)


def ptr(d):
    return d.ptr if d is not None else None


def gemm(M, N, K, dA, lda, dW, ldw, dB, dC, ldc, acc=0, variant=0, group_m=-1, swiglu=0, cos=None, sin=None, rope_cols=0):
    return lib().dsocr_k_gemm_bf16(M, N, K, dA.ptr, lda, dW.ptr, ldw, ptr(dB), dC.ptr, ldc, 1, acc, variant, group_m, swiglu,
                                   ptr(cos), ptr(sin), rope_cols)


def dots_op(op, rows, cols, y, x=None, aux=0, ld=0, p0=None, p1=None, eps=0.0):
    return lib().dsocr_k_dots_op(op, rows, cols, aux, ld, ptr(x), ptr(p0), ptr(p1), eps, y.ptr)


# ----------------------------------------------------------------------------- GEMM against f64
# id -> (M, N, K, bias, accumulate, ldc, kernels).  The path each case reaches:
GEMM_CASES = {
    # one nt k-step, two ping-pong k-tiles (the short prologue); ragged both ways, N % 8 != 0
    "k64_ragged": (70, 130, 64, 1, 0, 144, (NT1, NT2, PP)),
    # wave row 1 entirely past M; the gcol + 8 > N scalar tail under accumulate; columns 196..199 keep SENT
    "tail_accumulate": (100, 196, 128, 1, 1, 200, (PP, NT1, NT2)),
    # a second M tile of one row, a second N tile of 8 columns (three of its wave columns out of range), six k-tiles
    "one_row_tile": (257, 264, 192, 0, 1, 272, (PP, NT1)),
    # the 68-row tail of the 2044 px page (21316 = 83 * 256 + 68)
    "page_tail": (324, 256, 320, 1, 0, 264, (PP, NT1)),
    # the tower's proj and fc2 depths
    "proj_depth": (300, 200, 1536, 1, 1, 208, (NT1, PP)),
    "fc2_depth": (260, 264, 4224, 1, 1, 272, (NT1, PP)),
}
PATCH_CASE = (100, 192, 588, 640)  # M, N, the patch embed's K = 3 * 14 * 14 and its padding to a multiple of 64


def chain64(s, bias, c0):
    """The f64 reference chain on the exact product sums s -> (ref, sum of |v| over the steps applied)."""
    v = rnd64(s)
    mag = np.abs(v).astype(F64)
    if bias is not None:
        v = rnd64(v.astype(F64) + bias.astype(F64))
        mag += np.abs(v)
    if c0 is not None:
        v = rnd64(c0.astype(F64) + v.astype(F64))
        mag += np.abs(v)
    return v, mag


def hard_bound(a, w, mag):
    return (2e-5 * (np.abs(a).astype(F64) @ np.abs(w).T.astype(F64)) + 1e-6 + 2.0 ** -7 * mag) * (1 + 2.0 ** -6)


def chain_blocks16(a, w, bias, c0):
    """The kernels' arithmetic: an f32 accumulator over ascending 16-wide k blocks (one MFMA each, the block's
    products summed exactly), then the f32 epilogue rounding to bf16 after every op."""
    acc = np.zeros((a.shape[0], w.shape[0]), F32)
    for k in range(0, a.shape[1], 16):
        acc = (acc.astype(F64) + a[:, k:k + 16].astype(F64) @ w[:, k:k + 16].T.astype(F64)).astype(F32)
    v = bf16(acc)
    if bias is not None:
        v = bf16(v + bias)
    if c0 is not None:
        v = bf16(c0 + v)
    return v


@functools.lru_cache(maxsize=None)
def gemm_case(name):
    if name == "patch_embed":
        M, N, K0, K = PATCH_CASE
        has_bias, acc, ldc = 1, 0, 200
    else:
        M, N, K, has_bias, acc, ldc, _ = GEMM_CASES[name]
        K0 = K
    rng = np.random.default_rng([M, N, K])
    x = rng.standard_normal((M, K0)).astype(F32)          # the patch case feeds these f32 rows to the to_bf16 op
    a = np.zeros((M, K), F32)
    a[:, :K0] = bf16(x)
    w = np.zeros((N, K), F32)
    w[:, :K0] = bf16((0.03 * rng.standard_normal((N, K0))).astype(F32))
    bias = (0.1 * rng.standard_normal(N)).astype(F32) if has_bias else None
    c0 = bf16(rng.standard_normal((M, N)).astype(F32)) if acc else None
    ref, mag = chain64(a.astype(F64) @ w.T.astype(F64), bias, c0)
    bound = hard_bound(a, w, mag)
    for arr in (x, a, w, bias, c0, ref, bound):
        if arr is not None:
            arr.setflags(write=False)
    return dict(M=M, N=N, K=K, K0=K0, x=x, a=a, w=w, bias=bias, c0=c0, ldc=ldc, ref=ref, bound=bound)


def c_buffer(c, rows_past=3):
    buf = sentinel(c["M"] + rows_past, c["ldc"])
    if c["c0"] is not None:
        buf[:c["M"], :c["N"]] = bits_of(c["c0"])
    return buf


def check_gemm(c, buf, what):
    """Sentinel, hard bound and flip cap of one launch's output buffer; returns the result bits [M][N]."""
    M, N = c["M"], c["N"]
    assert np.all(buf[M:] == SENT), f"{what}: rows past M written"
    assert np.all(buf[:M, N:] == SENT), f"{what}: columns past N written"
    got = buf[:M, :N]
    assert not np.any(got == SENT), f"{what}: {int((got == SENT).sum())} elements never written"
    err = np.abs(bf16_to_f32(got).astype(F64) - c["ref"])
    share = float(np.mean(got != bits_of(c["ref"])))
    print(f"{what}: flip share {share:.2e}, max err / bound {float(np.max(err / c['bound'])):.3f}")
    assert np.all(err <= c["bound"]), f"{what}: {int((err > c['bound']).sum())} elements past the hard bound"
    assert share <= 1e-3, f"{what}: flip share {share:.2e}"
    return got


def run_gemm_case(c, dA, kernels, name):
    dW, dB = Dev(bits_of(c["w"])), (Dev(c["bias"]) if c["bias"] is not None else None)
    outs = {}
    for v in kernels:
        dC = Dev(c_buffer(c))
        check(gemm(c["M"], c["N"], c["K"], dA, c["K"], dW, c["K"], dB, dC, c["ldc"], acc=int(c["c0"] is not None), variant=v))
        outs[v] = check_gemm(c, dC.get(), f"{name} {KNAME[v]}")
    first = kernels[0]
    for v in kernels[1:]:
        assert np.array_equal(outs[v], outs[first]), f"{name}: {KNAME[v]} and {KNAME[first]} differ in " \
                                                     f"{int((outs[v] != outs[first]).sum())} elements"


@gpu_test
@pytest.mark.parametrize("name", list(GEMM_CASES))
def test_gemm_bf16_vs_f64(gpu, name):
    """Each case on each of its kernels against the f64 chain, and the kernels against each other bit for bit
    (the ping-pong kernel runs the 128 x 128 kernel's MFMA sequence per element).
    Measured on an MI355X, flip share against the f64 chain (the same on every kernel of a case, and the CPU
    emulation's of test_gemm_reference_margin): k64_ragged 0, tail_accumulate 0, one_row_tile 1.47e-5,
    page_tail 3.62e-5, proj_depth 0, fc2_depth 1.02e-4."""
    c = gemm_case(name)
    run_gemm_case(c, Dev(bits_of(c["a"])), GEMM_CASES[name][6], name)


@gpu_test
def test_gemm_bf16_patch_embed_form(gpu):
    """(100, 192, 640) with lda = 640 on the default dispatch and the ping-pong kernel: A comes from the to_bf16 op
    on f32 rows of 588 columns (its 52 padding columns must be zero), W is zero-padded as the engine pads it.
    Measured flip share on an MI355X: 1.04e-4 (2 of 19200) on both kernels."""
    c = gemm_case("patch_embed")
    M, K0, K = c["M"], c["K0"], c["K"]
    dA = Dev(sentinel(M + 1, K))
    check(dots_op(DOTS_TO_BF16, M, K0, dA, x=Dev(c["x"]), aux=K, ld=K0))
    a = dA.get()
    assert np.array_equal(a[:M], bits_of(c["a"])) and np.all(a[M:] == SENT)
    run_gemm_case(c, dA, (NT1, PP), "patch_embed")


def test_gemm_reference_margin():
    """No GPU: the kernels' accumulation order (f32 over ascending 16-wide k blocks) with the f32 epilogue moves at
    most 1e-4 of the elements of the cases above off the f64 chain (pooled: the smaller cases have fewer than 1e4
    elements, where one flip is already more), a tenth of the cap each launch is held to.  Per case: 0, 0, 1, 2, 1,
    5 and 2 elements, 11 of 326332."""
    flips = total = 0
    for name in list(GEMM_CASES) + ["patch_embed"]:
        c = gemm_case(name)
        emu = chain_blocks16(c["a"], c["w"], c["bias"], c["c0"])
        n = int((bits_of(emu) != bits_of(c["ref"])).sum())
        print(f"{name}: 16-block emulation moves {n} of {emu.size} elements ({n / emu.size:.2e})")
        assert n / emu.size <= 1e-3, name
        flips, total = flips + n, total + emu.size
    assert flips / total <= 1e-4, (flips, total)


@gpu_test
def test_gemm_bf16_tile_raster(gpu):
    """(1300, 520, 64) with bias: 6 x 3 ping-pong tiles under group_m 1 / 4 / 8 (groups of 4 + 2 and of 6 bands) and
    11 x 5 tiles of 128 under group_m 1 / 8 (8 + 3).  A raster that is no bijection leaves a tile unwritten: no
    sentinel may remain inside M x N, and all five results are the same bits (measured flip share against the f64
    chain: 7.4e-6)."""
    M, N, K, ldc = 1300, 520, 64, 528
    rng = np.random.default_rng(1300)
    a = bf16(rng.standard_normal((M, K)).astype(F32))
    w = bf16((0.03 * rng.standard_normal((N, K))).astype(F32))
    bias = (0.1 * rng.standard_normal(N)).astype(F32)
    ref, mag = chain64(a.astype(F64) @ w.T.astype(F64), bias, None)
    c = dict(M=M, N=N, K=K, ref=ref, c0=None, ldc=ldc, bound=hard_bound(a, w, mag))
    dA, dW, dB = Dev(bits_of(a)), Dev(bits_of(w)), Dev(bias)
    outs = []
    for v, gm in [(PP, 1), (PP, 4), (PP, 8), (NT1, 1), (NT1, 8)]:
        dC = Dev(c_buffer(c))
        check(gemm(M, N, K, dA, K, dW, K, dB, dC, ldc, variant=v, group_m=gm))
        outs.append(check_gemm(c, dC.get(), f"raster {KNAME[v]} group_m={gm}"))
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])


@gpu_test
def test_gemm_bf16_rejects_bad_shapes(gpu):
    """The launchers' EINVAL comes back as a status and nothing is written."""
    M, N, K = 64, 128, 128
    dA, dW = Dev(np.zeros((M, K), np.uint16)), Dev(np.zeros((N, K), np.uint16))
    dC = Dev(sentinel(M, N))
    assert gemm(M, N, 96, dA, K, dW, K, None, dC, N) == EINVAL                      # K % 64
    assert b"EINVAL" in lib().dsocr_last_error()
    assert gemm(M, 96, K, dA, K, dW, K, None, dC, 48, swiglu=1) == EINVAL          # SwiGLU pair: N % 64
    assert gemm(M, N, K, dA, K, dW, K, None, dC, N + 4, variant=PP) == EINVAL      # ping-pong: ldc % 8
    assert gemm(M, N, K, dA, K, dW, K, None, dC, N, variant=1) == EINVAL
    assert np.all(dC.get() == SENT)


# ----------------------------------------------------------------------------- fused epilogues
def pair32(v, I):
    """[fc1 | fc3] rows (or bias entries) -> per 32: fc1 32b..32b+31, then fc3 32b..32b+31 (DotsVision's pair32)."""
    f1, f3 = v[:I].reshape(I // 32, 32, -1), v[I:].reshape(I // 32, 32, -1)
    return np.ascontiguousarray(np.stack([f1, f3], 1).reshape(v.shape))


@gpu_test
@pytest.mark.parametrize("has_bias", [0, 1])
@pytest.mark.parametrize("M", [100, 257])
@pytest.mark.parametrize("I", [96, 160])
def test_gemm_bf16_swiglu_pair(gpu, I, M, has_bias):
    """The SwiGLU-pair epilogue (N = 2 I = 192: wave column 3 of the tile is out of range and returns early; 320:
    two tiles) against the 128 x 128 GEMM of [fc1 | fc3] followed by the swiglu op: the same bits, rows past M
    untouched."""
    K, N = 128, 2 * I
    rng = np.random.default_rng(I * 1000 + M * 2 + has_bias)
    a = bits_of(bf16(rng.standard_normal((M, K)).astype(F32)))
    w = bits_of(bf16((0.03 * rng.standard_normal((N, K))).astype(F32)))
    bias = (0.1 * rng.standard_normal(N)).astype(F32)
    dA = Dev(a)
    dGU, dH = Dev(sentinel(M + 2, N)), Dev(sentinel(M + 2, I))
    check(gemm(M, N, K, dA, K, Dev(w), K, Dev(bias) if has_bias else None, dGU, N, variant=NT1))
    check(dots_op(DOTS_SWIGLU, M, I, dH, x=dGU))
    dF = Dev(sentinel(M + 2, I))
    check(gemm(M, N, K, dA, K, Dev(pair32(w, I)), K, Dev(pair32(bias, I)) if has_bias else None, dF, I, swiglu=1))
    unfused, fused = dH.get(), dF.get()
    assert np.all(dGU.get()[M:] == SENT) and np.all(unfused[M:] == SENT) and np.all(fused[M:] == SENT)
    assert not np.any(unfused[:M] == SENT)
    assert np.array_equal(fused[:M], unfused[:M]), int((fused[:M] != unfused[:M]).sum())


def rotary_tables(rng, n, hd):
    tower = DotsVision({"embed_dim": hd, "num_attention_heads": 1, "rms_norm_eps": EPS, "spatial_merge_size": 2}, None)
    return tower.rotary(rng.integers(0, 146, (n, 2)))  # any positions of a 2044 px page's 146 x 146 grid


@gpu_test
@pytest.mark.parametrize("M", [100, 257])
def test_gemm_bf16_rotary_epilogue(gpu, M):
    """The rotary epilogue (two heads of 128, q | k | v = 768 columns, rope_cols = 512) against the 128 x 128 GEMM
    followed by the rope op: the same bits on the q | k columns, and the v columns are the plain GEMM's."""
    D, K, hd = 256, 128, 128
    N = 3 * D
    rng = np.random.default_rng(7000 + M)
    a = bits_of(bf16(rng.standard_normal((M, K)).astype(F32)))
    w = bits_of(bf16((0.03 * rng.standard_normal((N, K))).astype(F32)))
    bias = (0.1 * rng.standard_normal(N)).astype(F32)
    cos, sin = rotary_tables(rng, M, hd)
    dA, dW, dB, dcos, dsin = Dev(a), Dev(w), Dev(bias), Dev(cos), Dev(sin)
    dQ, dR, dF = Dev(sentinel(M + 2, N)), Dev(sentinel(M + 2, N)), Dev(sentinel(M + 2, N))
    check(gemm(M, N, K, dA, K, dW, K, dB, dQ, N, variant=NT1))
    check(dots_op(DOTS_ROPE_QK, M, hd, dR, x=dQ, aux=D // hd, p0=dcos, p1=dsin))
    check(gemm(M, N, K, dA, K, dW, K, dB, dF, N, cos=dcos, sin=dsin, rope_cols=2 * D))
    plain, roped, fused = dQ.get(), dR.get(), dF.get()
    assert np.all(fused[M:] == SENT) and np.all(roped[M:] == SENT) and not np.any(fused[:M] == SENT)
    assert np.array_equal(fused[:M, :2 * D], roped[:M, :2 * D]), int((fused[:M, :2 * D] != roped[:M, :2 * D]).sum())
    assert np.array_equal(fused[:M, 2 * D:], plain[:M, 2 * D:])
    assert not np.array_equal(roped[:M, :2 * D], plain[:M, :2 * D])  # the rotation did something


# ----------------------------------------------------------------------------- row ops
def finite_bf16():
    """Every finite bf16 value, 65280 of them, as bits."""
    b = np.arange(0x10000, dtype=np.uint32)
    return b[(b & 0x7F80) != 0x7F80].astype(np.uint16)


def gelu_moved(x, d):
    """oracle.dots.gelu_bf16 with its one rounded transcendental, rnd(tanh(.)), moved d bf16 steps."""
    c, k = bf16(np.asarray(0.044715, F32)), bf16(np.asarray(math.sqrt(2.0 / math.pi), F32))
    alpha = bf16(x + bf16(c * bf16(bf16(x * x) * x)))
    t = bf16_step(bf16(np.tanh(bf16(k * alpha))), d)
    return bf16(bf16(F32(0.5) * x) * bf16(F32(1.0) + t))


def silu_moved(x, d):
    """oracle.dots.silu_bf16 with rnd(exp(-x)) moved d bf16 steps."""
    return bf16(x / bf16(F32(1.0) + bf16_step(bf16(np.exp(-x)), d)))


def assert_oracle_or_moved(got, exact, moved, cap, what):
    """got equals the oracle, or the oracle with its transcendental one bf16 step up or down; at most cap do."""
    off = got != bits_of(exact)
    ok = ~off
    for m in moved:
        ok |= got == bits_of(m)
    print(f"{what}: {int(off.sum())} of {got.size} elements needed the moved transcendental")
    assert np.all(ok), f"{what}: {int((~ok).sum())} elements match neither the oracle nor a moved one"
    assert int(off.sum()) <= cap, f"{what}: {int(off.sum())} moved elements"


@gpu_test
def test_gelu_every_finite_bf16(gpu):
    """dots_gelu on all 65280 finite bf16 values against oracle.dots.gelu_bf16.  A device tanhf that differs from
    numpy's in the last f32 bits may move rnd(tanh(.)) by one bf16 step and nothing else: every element equals the
    oracle or the oracle with that step, and at most 64 need it (the oracle with an f64 tanh differs from the f32
    one in 0 elements; measured on an MI355X: 0 elements need it).  +inf gives +inf and -inf gives NaN (-inf * rnd(1 + -1)), in the oracle and the kernel."""
    xb = finite_bf16()
    x = bf16_to_f32(xb)
    buf = np.concatenate([xb, np.array([0x7F80, 0xFF80], np.uint16), np.full(6, SENT)])
    dX = Dev(buf)
    check(dots_op(DOTS_GELU, 1, xb.size + 2, dX))
    got = dX.get()
    assert np.all(got[-6:] == SENT)
    with np.errstate(all="ignore"):
        assert_oracle_or_moved(got[:xb.size], gelu_bf16(x), [gelu_moved(x, -1), gelu_moved(x, 1)], 64, "gelu")
        inf = gelu_bf16(np.array([np.inf, -np.inf], F32))
    assert inf[0] == np.inf and np.isnan(inf[1])
    assert got[xb.size] == 0x7F80 and np.isnan(bf16_to_f32(got[xb.size + 1:xb.size + 2]))[0]


@gpu_test
@pytest.mark.parametrize("N,I,cap", [(255, 256, 64), (7, 20, 1)])
def test_swiglu_every_finite_bf16(gpu, N, I, cap):
    """dots_swiglu8 (I = 256, N = 255: g runs over all 65280 finite bf16 values) and the scalar dots_swiglu
    (I = 20, N = 7: 140 of them, the largest and smallest included) with random u, against
    bf16(silu_bf16(g) * u); rnd(exp(-g)) may sit one bf16 step off in at most 64 of 65280 elements (1e-3; one
    element for the 140).  The oracle with an f64 exp differs from the f32 one in 1 element of 65280; measured on an
    MI355X: 0 elements need the step in either case."""
    rng = np.random.default_rng(N * I)
    gb = finite_bf16()
    if N * I < gb.size:
        pick = np.sort(rng.choice(gb.size, N * I - 4, replace=False))
        gb = np.concatenate([gb[pick], np.array([0x0001, 0x7F7F, 0x8001, 0xFF7F], np.uint16)])
    g = bf16_to_f32(gb).reshape(N, I)
    u = bf16(rng.standard_normal((N, I)).astype(F32))
    dH = Dev(sentinel(N + 1, I))
    check(dots_op(DOTS_SWIGLU, N, I, dH, x=Dev(bits_of(np.concatenate([g, u], 1)))))
    got = dH.get()
    assert np.all(got[N:] == SENT)
    with np.errstate(all="ignore"):
        exact = bf16(silu_bf16(g) * u)
        moved = [bf16(silu_moved(g, d) * u) for d in (-1, 1)]
    assert_oracle_or_moved(got[:N], exact, moved, cap, f"swiglu I={I}")


@gpu_test
@pytest.mark.parametrize("heads,hd,N", [(12, 128, 5), (4, 32, 3)])
def test_rope_qk(gpu, heads, hd, N):
    """dots_rope8 computes x cos + rot sin in f32 with contraction off, as numpy's f32 does: bitwise equal to
    bf16(t * cos + r * sin).  (12, 128, 5): 384 threads of 8 dims, the second block partly out of range.  The v
    columns of out are not the kernel's to write."""
    D = heads * hd
    rng = np.random.default_rng(D + N)
    qkv = bf16(rng.standard_normal((N, 3 * D)).astype(F32))
    cos, sin = rotary_tables(rng, N, hd)
    dO = Dev(sentinel(N + 1, 3 * D))
    check(dots_op(DOTS_ROPE_QK, N, hd, dO, x=Dev(bits_of(qkv)), aux=heads, p0=Dev(cos), p1=Dev(sin)))
    got = dO.get()
    t = qkv[:, :2 * D].reshape(N, 2 * heads, hd)
    r = np.concatenate([-t[..., hd // 2:], t[..., :hd // 2]], -1)
    ref = bf16((t * cos[:, None, :]) + (r * sin[:, None, :])).reshape(N, 2 * D)
    assert np.array_equal(got[:N, :2 * D], bits_of(ref)), int((got[:N, :2 * D] != bits_of(ref)).sum())
    assert np.all(got[:N, 2 * D:] == SENT) and np.all(got[N:] == SENT)


@gpu_test
def test_rope_qk_rejects_head_dim_24(gpu):
    dO = Dev(sentinel(2, 3 * 48))
    z = Dev(np.zeros((2, 3 * 48), np.uint16))
    t = Dev(np.zeros((2, 24), F32))
    assert dots_op(DOTS_ROPE_QK, 2, 24, dO, x=z, aux=2, p0=t, p1=t) == EINVAL
    assert dots_op(99, 2, 24, dO, x=z) == EINVAL
    assert np.all(dO.get() == SENT)


ROWS = 33


def norm_rows(rng, D, spread):
    """33 rows with per-row scales spread over exp(spread * randn)."""
    return (rng.standard_normal((ROWS, D)) * np.exp(spread * rng.standard_normal((ROWS, 1)))).astype(F32)


@gpu_test
@pytest.mark.parametrize("D,in_f32,in_place", [(8, 0, 0), (1536, 0, 1), (2056, 0, 0), (4096, 0, 0),   # dots_rmsnorm8
                                               (100, 0, 0), (4104, 0, 0), (1536, 1, 0)])            # dots_rmsnorm
def test_dots_rmsnorm(gpu, D, in_f32, in_place):
    """dots_rmsnorm8 (D % 8 == 0, D <= 4096; 2056 leaves the second register chunk partly used; one case in place
    as the tower runs it) and the scalar dots_rmsnorm (D % 8 != 0, D > 4096, f32 input).  With den64 from an f64
    sum and delta = D 2^-24 (the worst-case f32 summation error, which also covers the kernel's four other f32
    roundings from D = 8 on), every element lies between bf16(x / (den64 (1 + delta)) w) and
    bf16(x / (den64 (1 - delta)) w), never more than one bf16 step apart, and at most 1e-3 of them differ from
    the den64 value.  Measured on an MI355X: 7.4e-6 at D = 4096, 1.48e-5 at D = 4104, 0 elsewhere, each the same as
    oracle.dots.rms_norm in f32 gives against the den64 value."""
    rng = np.random.default_rng(D * 2 + in_f32)
    x = norm_rows(rng, D, 2.0)
    if not in_f32:
        x = bf16(x)
    w = (1.0 + 0.1 * rng.standard_normal(D)).astype(F32)
    buf = sentinel(ROWS + 1, D)
    if in_place:
        buf[:ROWS] = bits_of(x)
    dY = Dev(buf)
    dX = dY if in_place else Dev(x if in_f32 else bits_of(x))
    check(dots_op(DOTS_RMSNORM, ROWS, D, dY, x=dX, aux=in_f32, p0=Dev(w), eps=EPS))
    got = dY.get()
    assert np.all(got[ROWS:] == SENT)
    got = bf16_to_f32(got[:ROWS])
    x64, delta = x.astype(F64), D * 2.0 ** -24
    den = np.sqrt((x64 * x64).mean(-1, keepdims=True) + EPS)
    a, b, mid = (rnd64(x64 / (den * f) * w) for f in (1 + delta, 1 - delta, 1.0))
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    assert np.all(np.abs(bits_of(hi).astype(np.int32) - bits_of(lo).astype(np.int32)) <= 1)  # the window: one step
    assert np.all((got >= lo) & (got <= hi)), int(((got < lo) | (got > hi)).sum())
    share = float(np.mean(bits_of(got) != bits_of(mid)))
    f32_share = float(np.mean(bits_of(bf16(rms_norm(x, w, EPS))) != bits_of(mid)))
    print(f"rmsnorm D={D} in_f32={in_f32}: share off the den64 value {share:.2e} (f32 oracle {f32_share:.2e})")
    assert share <= 1e-3, share


@gpu_test
@pytest.mark.parametrize("D", [1536, 100, 4104])
def test_dots_layernorm(gpu, D):
    """dots_layernorm against y = (x - mu) / den * w + b with f64 sums: |got - y| <= 2^-8 |y| (the output
    rounding) + D 2^-24 (|t| + |w| mean|x| / den + |b|) (the f32 sums of the mean and the variance and the f32
    ops on t, the mean and b), and at most 1e-3 of the elements differ from rnd(y).  Measured on an MI355X: 3.95e-5
    (D = 1536), 3.03e-4 (D = 100: 1 of 3300), 6.65e-5 (D = 4104), each the same as oracle.dots.layer_norm in f32
    gives; largest error / bound 0.98."""
    rng = np.random.default_rng(D)
    x = bf16(norm_rows(rng, D, 1.0) + rng.standard_normal((ROWS, 1)).astype(F32))
    w = (1.0 + 0.1 * rng.standard_normal(D)).astype(F32)
    b = (0.1 * rng.standard_normal(D)).astype(F32)
    dY = Dev(sentinel(ROWS + 1, D))
    check(dots_op(DOTS_LAYERNORM, ROWS, D, dY, x=Dev(bits_of(x)), p0=Dev(w), p1=Dev(b), eps=1e-6))
    got = dY.get()
    assert np.all(got[ROWS:] == SENT)
    got = bf16_to_f32(got[:ROWS])
    x64 = x.astype(F64)
    mu = x64.mean(-1, keepdims=True)
    den = np.sqrt(((x64 - mu) ** 2).mean(-1, keepdims=True) + 1e-6)
    t = (x64 - mu) / den * w
    y = t + b
    bound = 2.0 ** -8 * np.abs(y) + D * 2.0 ** -24 * (np.abs(t) + np.abs(w) * np.abs(x64).mean(-1, keepdims=True) / den
                                                      + np.abs(b))
    err = np.abs(got - y)
    share = float(np.mean(bits_of(got) != bits_of(rnd64(y))))
    f32_share = float(np.mean(bits_of(bf16(layer_norm(x, w, b, 1e-6))) != bits_of(rnd64(y))))
    print(f"layernorm D={D}: max err / bound {float(np.max(err / bound)):.3f}, share off rnd(y) {share:.2e} "
          f"(f32 oracle {f32_share:.2e})")
    assert np.all(err <= bound), int((err > bound).sum())
    assert share <= 1e-3, share


@gpu_test
def test_to_bf16_and_back_exact(gpu):
    """dots_to_bf16 rounds to nearest even (ties both ways, a carry into the next exponent, overflow to inf,
    subnormals), reads rows of ldi > D and zero-fills columns D..ldo; dots_bf16_to_f32 is exact on all 65536 bit
    patterns."""
    N, D, ldi, ldo = 5, 13, 17, 24
    rng = np.random.default_rng(5)
    x = rng.standard_normal((N, ldi)).astype(F32)
    x[0, :8] = np.array([0x3FFFFFFF, 0x3F808000, 0x3F818000, 0xBF808001, 0x7F7FFFFF, 0x00008000, 0x80018000, 0x7F800000],
                        np.uint32).view(F32)  # -> 2.0 (next exponent), tie down, tie up, above a tie, inf, 0, -2 steps, inf
    dY = Dev(sentinel(N + 1, ldo))
    check(dots_op(DOTS_TO_BF16, N, D, dY, x=Dev(x), aux=ldo, ld=ldi))
    got = dY.get()
    assert list(got[0, :8]) == [0x4000, 0x3F80, 0x3F82, 0xBF81, 0x7F80, 0x0000, 0x8002, 0x7F80]
    assert np.array_equal(got[:N, :D], bf16_round(x[:, :D]))
    assert np.all(got[:N, D:] == 0) and np.all(got[N:] == SENT)
    allb = np.arange(0x10000, dtype=np.uint32).astype(np.uint16).reshape(256, 256)
    dF = Dev(np.full((257, 256), 0x7F5A7F5A, np.uint32))
    check(dots_op(DOTS_BF16_TO_F32, 256, 256, dF, x=Dev(allb)))
    f = dF.get()
    assert np.array_equal(f[:256], allb.astype(np.uint32) << 16) and np.all(f[256:] == 0x7F5A7F5A)
