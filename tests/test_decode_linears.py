"""The decode linears in every form the engine launches them (launch_dec_gemv and the kernels it picks in
decode_gemv.hip / decode_mm.hip, launch_mm_swizzle, launch_silu_mul) on MI355X (gfx950), one launch at a time.

Reference of every linear: act((xn . W^T in f64) -> f32 + bias) (+ y0), xn the oracle's f32 rms_norm when a norm
weight is given.  Tolerance (the project's bound for f32 sums in another order, tests/test_gpu_kernels.py):
  |got - ref| <= 2e-5 * sum_k |xn_k w_k| (x 2 when act != 0) + 1e-6 + 1e-6 * |ref|
Every case asserts the kernel kind the dispatch reports (the CPU table test in test_host_cpu.py pins that report),
so no case passes on another kernel.  x, W and y carry padding columns: NaN in x and W (a read past K poisons the
output), a bit pattern in y that must come back unchanged.
"""
import ctypes as C
import zlib

import numpy as np
import pytest

from _dev import Dev, bf16_round, f16_bits  # noqa: F401  (bf16_round / f16_bits: through _weights)
from dsocr._lib import EINVAL, DsocrError, check, lib
from oracle.decoder import rms_norm
from test_gpu_kernels import ACTS, _weights

pytestmark = pytest.mark.gpu

F32 = np.float32
Y_PAD = np.uint32(0xC0DEFACE)                     # y's padding columns
W_NAN = {0: np.uint16(0x7FC0), 1: np.uint16(0x7E00)}  # bf16 / f16 quiet NaN
EPS = 1e-6


def _rows(rng, M, K, rows):
    """Token rows.  "unit": unit normal.  "wide" (M >= 3): per-row scales exp(3 randn) — the f16 plane split rescales
    each row by a power of two — row 1 all zero (mx == 0), row 2 1e-3-scale values with a single 1e4 outlier."""
    x = rng.standard_normal((M, K))
    if rows == "wide":
        x *= np.exp(3.0 * rng.standard_normal((M, 1)))
        x[1] = 0.0
        x[2] = 1e-3 * rng.standard_normal(K)
        x[2, int(rng.integers(K))] = 1e4
    return x.astype(F32)


def _launch(M, N, K, x, ldx, nw, bits, ldw, wdt, bias, y0, ldy, act, swizzle, dW=None):
    """One launch through dsocr_k_gemv_ex on padded buffers -> (y [M][N], kind).  x's and W's padding columns hold
    NaN, y's a bit pattern that must come back unchanged; y starts from y0 (accumulate) or NaN."""
    xb = np.full((M, ldx), np.nan, F32)
    xb[:, :K] = x
    if dW is None:
        wb = np.full((N, ldw), W_NAN[wdt], np.uint16)
        wb[:, :K] = bits
        dW = Dev(wb)
    yb = np.full((M, ldy), Y_PAD, np.uint32).view(F32)
    yb[:, :N] = np.nan if y0 is None else y0
    dx, dy, db = Dev(xb), Dev(yb), Dev(bias)
    dn = Dev(nw) if nw is not None else None
    kind = C.c_char_p()
    check(lib().dsocr_k_gemv_ex(M, N, K, dx.ptr, ldx, dn.ptr if dn else None, EPS, dW.ptr, ldw, wdt, db.ptr, dy.ptr, ldy,
                                act, int(y0 is not None), int(swizzle), C.byref(kind)))
    got = dy.get()
    assert np.all(got[:, N:].view(np.uint32) == Y_PAD), "y padding overwritten"
    return got[:, :N].copy(), kind.value.decode()


class Case:
    """Host data of one linear, its f64-based reference and the per-element bound (computed once per case)."""

    def __init__(self, name, M, N, K, wdt, norm, act, acc, rows="unit", padx=8, padw=8, pady=4):
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        self.M, self.N, self.K, self.wdt, self.act, self.acc = M, N, K, wdt, act, acc
        self.ldx, self.ldw, self.ldy = K + padx, K + padw, N + pady
        self.x = _rows(rng, M, K, rows)
        self.bits, w = _weights(rng, N, K, wdt)
        self.nw = (1.0 + 0.05 * rng.standard_normal(K)).astype(F32) if norm else None
        self.bias = (0.1 * rng.standard_normal(N)).astype(F32)
        self.y0 = rng.standard_normal((M, N)).astype(F32) if acc else None
        xn = rms_norm(self.x, self.nw, EPS) if norm else self.x
        dot = np.empty((M, N), F32)
        mag = np.empty((M, N), np.float64)
        xd, xa = xn.astype(np.float64), np.abs(xn).astype(np.float64)
        for n0 in range(0, N, 8192):  # in row blocks: the f64 copy of a 70007-row W is 700 MB
            wd = w[n0:n0 + 8192].astype(np.float64)
            dot[:, n0:n0 + 8192] = (xd @ wd.T).astype(F32)
            mag[:, n0:n0 + 8192] = xa @ np.abs(wd).T
        pre = dot + self.bias
        with np.errstate(over="ignore"):
            self.ref = ACTS[act](pre).astype(F32)
        if acc:
            self.ref = self.ref + self.y0
        self.mag = mag
        scale = 2.0 if act else 1.0
        self.bound = 2e-5 * mag * scale + 1e-6 + 1e-6 * np.abs(self.ref)
        # The bound is not vacuous.  At unit scale its sum term is 2e-5 * K * E|x| E|w| against a linear output of
        # root mean square sqrt(K) * sd(x) sd(w), i.e. scale * 2e-5 * (2 / pi) * sqrt(K) of the typical output:
        # 4.6e-4 (9.1e-4 with an activation) at K = 1280, below 1e-3 up to K = 1540 even when doubled; the two long-K
        # cases of the dispatch table sit above it by construction (K = 1544: 1.0e-3, K = 6848: 2.1e-3).
        self.slack = float(np.median(self.bound) / np.sqrt(np.mean(pre.astype(np.float64) ** 2)))
        if rows == "unit":
            assert self.slack < 1.1 * scale * 2e-5 * (2 / np.pi) * np.sqrt(K) + 2e-5, (name, self.slack)
            assert self.slack < 1e-3 or K > 1280, (name, self.slack)
        self._dW = None

    def run(self, swizzle):
        """The case's launch, row-major (ldw as given) or on the fragment-ordered copy (ldw == K) -> (y, kind)."""
        ldw = self.K if swizzle else self.ldw
        if ldw == self.K and self._dW is None:  # one upload for the row-major and the fragment-ordered launch
            self._dW = Dev(self.bits)
        return _launch(self.M, self.N, self.K, self.x, self.ldx, self.nw, self.bits, ldw, self.wdt, self.bias, self.y0,
                       self.ldy, self.act, swizzle, self._dW if ldw == self.K else None)

    def check(self, got, label):
        err = np.abs(got.astype(np.float64) - self.ref)
        ratio = float(np.max(err / self.bound)) if np.all(np.isfinite(got)) else float("inf")
        print(f"{label}: max |got - ref| / bound = {ratio:.4f}")
        assert np.all(err <= self.bound), (label, ratio)


def _rows_per_launch(c, swizzle=0):
    k, r = C.c_char_p(), C.c_int(-1)
    check(lib().dsocr_k_gemv_kind(c.M, c.N, c.K, c.ldw, c.wdt, int(c.nw is not None), 0, swizzle, C.byref(k), C.byref(r)))
    return r.value


# ---------------------------------------------------------------- a. dec_mm, row-major and fragment-ordered
# K = 1280 is the only K inside dec_mm_ok.  With it a wave's k range holds one batch (WK 8: 5 steps, PF 5) or four
# (WR 8: 40 steps, PF 10), so the `nch & 1` hand-over of dec_mm_kernel (an odd batch count with several tiles per
# block) cannot be reached through the dispatch and has no case here.
# (M, N, wdt (0 bf16, 1 f16), norm, act, accumulate, rows, padded ldw for the row-major launch)
MM_CASES = [
    (3, 16, 1, 0, 0, 1, "wide", 1), (4, 16, 0, 1, 1, 0, "unit", 1), (5, 16, 1, 1, 3, 0, "wide", 0), (8, 16, 0, 0, 0, 1, "unit", 0),
    (3, 40, 0, 1, 3, 1, "unit", 1), (4, 40, 1, 0, 1, 0, "wide", 0), (5, 40, 0, 0, 0, 0, "unit", 0), (8, 40, 1, 1, 0, 1, "wide", 1),
    (3, 200, 1, 1, 0, 0, "wide", 0), (4, 200, 0, 0, 3, 1, "unit", 0), (5, 200, 1, 0, 1, 1, "wide", 1), (8, 200, 0, 1, 0, 0, "unit", 0),
    (3, 1280, 0, 0, 1, 0, "unit", 0), (4, 1280, 1, 1, 3, 1, "wide", 0), (5, 1280, 0, 1, 0, 1, "unit", 1), (8, 1280, 1, 0, 0, 0, "wide", 0),
    # the engine's o_proj and q/k/v at unit scale with f16 weights
    (8, 1280, 1, 0, 0, 1, "unit", 0), (3, 3840, 1, 1, 0, 0, "unit", 1),
    # the WR 8 block shape (N >= 16384): residual read from global memory, ragged last tile, 3 and 5 staged rows
    (8, 16400, 1, 0, 0, 1, "wide", 1), (5, 16400, 0, 0, 3, 1, "unit", 0), (3, 16384, 1, 1, 1, 0, "wide", 0),
    (8, 70007, 0, 1, 0, 0, "unit", 0),
]


@pytest.mark.parametrize("M,N,wdt,norm,act,acc,rows,padw", MM_CASES)
def test_dec_mm(gpu, M, N, wdt, norm, act, acc, rows, padw):
    """dec_mm_kernel from row-major weights and from the fragment-ordered copy the engine keeps at 3..8 pages
    (dec_mm_kernel<.., SWZ = true> on launch_mm_swizzle's output), both against f64, and against each other bit for
    bit: the two instantiations feed the same fragments to the same MFMA sequence, only the load addresses differ.

    M = 3 and 5 leave staged token rows unwritten (their columns must not leak), N = 40 / 200 / 16400 / 70007 end in
    a partial tile (row clamp min(n, N - 1), store guard nn < N), accumulate off starts from a NaN-filled y.
    f16 weights take the "wide" rows of _rows: the all-zero row must give exactly act(bias) (+ y0).

    N = 70007 (4376 row tiles, 547 blocks of WR 8 tiles): the launch is capped at the resident block count; a block
    has 512 threads, 3 * 8 * (1280 + 16) * 2 B = 62208 B of dynamic LDS plus 8.3 KB static, so at most 2 fit a CU's
    160 KB, and 547 > 2 * 256 CUs: some blocks walk a second tile group (the `more` / `nxt` path), the last one ragged.
    (Derived from the code, not measured: with one block per CU every block walks two or three groups instead.)"""
    K = 1280
    c = Case(f"mm-{M}-{N}-{wdt}-{norm}-{act}-{acc}-{rows}", M, N, K, wdt, norm, act, acc, rows, padw=8 if padw else 0)
    shape = "wr8" if N >= 16384 else "wk8"
    assert _rows_per_launch(c) == 12 and _rows_per_launch(c, 1) == 12  # one launch
    label = f"dec_mm M={M} N={N} {'f16' if wdt else 'bf16'} norm={norm} act={act} acc={acc} {rows}"
    got_rm, kind = c.run(swizzle=0)
    assert kind == f"dec_mm_{shape}"
    c.check(got_rm, f"{label} [{kind}]")
    got_sw, kind = c.run(swizzle=1)
    assert kind == f"dec_mm_{shape}_swz"
    c.check(got_sw, f"{label} [{kind}]")
    assert np.array_equal(got_rm.view(np.uint32), got_sw.view(np.uint32)), "fragment-ordered != row-major, bitwise"
    if rows == "wide":
        zero = ACTS[act](c.bias).astype(F32) + (c.y0[1] if acc else 0)
        if act == 0:  # no dot product term at all: bias (+ y0), bit for bit
            assert np.array_equal(got_sw[1].view(np.uint32), zero.astype(F32).view(np.uint32))
        else:  # the device's own erff / expf: within the bound's floor (its sum term is zero for this row)
            assert np.all(c.mag[1] == 0) and np.all(np.abs(got_sw[1] - zero) <= 1e-6 + 1e-6 * np.abs(zero))


@pytest.mark.parametrize("wdt,N,acc", [(0, 200, 1), (1, 200, 0), (1, 16400, 1), (0, 16400, 0)])
def test_dec_mm_exact_on_integers(gpu, wdt, N, acc):
    """The tolerance above leaves room for a lost low plane (2^-17 of an element), so one check is exact: integer
    inputs whose every partial sum is an integer below 2^24 give the integer result in any summation order, bit
    for bit.  Weights are -1 / 0 / 1; a token row holds odd integers below 2^11 and two entries of 23 significant
    bits in [2^22, 1.5 * 2^22) — more than two 8-bit bf16 planes or two 11-bit f16 planes hold, so the third plane
    must arrive, and for f16 the row scale 2^-8 must come back exactly.  Largest partial sum: 2 * 1.5 * 2^22 +
    1278 * 2047 + bias 8 + residual 100 = 15.2e6 < 2^24 = 16.8e6.  Row 0 has no large entry (another row scale)."""
    M, K = 5, 1280
    rng = np.random.default_rng(1000 * N + 10 * wdt + acc)
    xi = (2 * rng.integers(0, 1024, (M, K)) + 1) * rng.choice([-1, 1], (M, K))
    for m in range(1, M):
        k1, k2 = rng.choice(K, 2, replace=False)
        xi[m, k1] = (2 ** 22 + 2 * rng.integers(0, 2 ** 20) + 1) * rng.choice([-1, 1])
        xi[m, k2] = (2 ** 22 + 2 * rng.integers(0, 2 ** 20) + 1) * rng.choice([-1, 1])
    wi = rng.integers(-1, 2, (N, K))
    bi = rng.integers(-8, 9, N)
    yi = rng.integers(-100, 101, (M, N)) if acc else None
    ref = xi @ wi.T + bi + (yi if acc else 0)
    assert int((np.abs(xi) @ np.abs(wi).T).max()) + 108 < 2 ** 24  # every partial sum of every order is exact
    bits = bf16_round(wi.astype(F32)) if wdt == 0 else f16_bits(wi.astype(F32))
    x, bias, y0 = xi.astype(F32), bi.astype(F32), (yi.astype(F32) if acc else None)
    assert np.array_equal(x.astype(np.int64), xi)
    shape = "wr8" if N >= 16384 else "wk8"
    for swizzle in (0, 1):
        got, kind = _launch(M, N, K, x, K + 8, None, bits, K if swizzle else K + 8, wdt, bias, y0, N + 4, 0, swizzle)
        assert kind == f"dec_mm_{shape}" + ("_swz" if swizzle else "")
        assert np.array_equal(got.astype(np.float64), ref.astype(np.float64)), (kind, np.max(np.abs(got - ref)))


def test_swizzle_refused_outside_dec_mm(gpu):
    """dsocr_k_gemv_ex never runs another kernel when asked for the fragment-ordered form."""
    for M, N, K in [(2, 1280, 1280), (9, 1280, 1280), (8, 8, 1280), (8, 1280, 256)]:
        c = Case(f"refuse-{M}-{N}-{K}", M, N, K, 1, 0, 0, 0)
        with pytest.raises(DsocrError) as e:
            c.run(swizzle=1)
        assert e.value.status == EINVAL


# ---------------------------------------------------------------- b. launch_mm_swizzle's layout
@pytest.mark.parametrize("N,K", [(16, 32), (40, 64), (1280, 1280)])
def test_mm_swizzle_layout(gpu, N, K):
    """[ceil(N/16) tiles][K/32 steps][64 lanes][8]: lane l of step t of tile T holds
    W[min(16 T + (l & 15), N - 1)][32 t + 8 (l >> 4) .. + 7], exact on the 16-bit patterns (N = 40: rows past N
    repeat row N - 1).  W holds a different value at every (row, column) a transposed lane map could confuse."""
    n, k = np.arange(N, dtype=np.int64)[:, None], np.arange(K, dtype=np.int64)[None, :]
    w = ((n * K + k + 7919 * n) % 65536).astype(np.uint16)
    T = (N + 15) // 16
    rows = np.minimum(16 * np.arange(T)[:, None] + np.arange(16)[None, :], N - 1)  # [T][16]
    ref = w[rows].reshape(T, 16, K // 32, 4, 8).transpose(0, 2, 3, 1, 4).reshape(T, K // 32, 64, 8)  # lane = 16 g + r
    dw, do = Dev(w), Dev(np.full(ref.shape, 0xFFFF, np.uint16))
    check(lib().dsocr_k_mm_swizzle(N, K, dw.ptr, do.ptr))
    assert np.array_equal(do.get(), ref)


# ---------------------------------------------------------------- c. the other branches of the dispatch
# (M, N, K, wdt, norm, act, accumulate, kind, token rows per launch)
GEMV_CASES = [
    (1, 130, 64, 1, 1, 1, 1, "dec_gemv_rb1", 16),
    (2, 16400, 256, 0, 0, 3, 0, "dec_gemv_stream", 16),
    (1, 16400, 1544, 1, 1, 3, 1, "dec_gemv_rb4", 10),
    (3, 16400, 256, 0, 1, 1, 1, "dec_gemv_rb2", 16),
    (16, 16400, 64, 0, 0, 3, 0, "dec_gemv_rb2", 16),
    (4, 200, 512, 1, 1, 1, 1, "dec_gemv_lds_r1", 16),
    (8, 2600, 256, 0, 1, 3, 0, "dec_gemv_lds_r2", 16),
    (3, 64, 6848, 1, 0, 1, 1, "dec_gemv_rb1", 2),  # K = 6848 stages 2 rows per launch: two launches (2 rows, 1 row)
]


@pytest.mark.parametrize("M,N,K,wdt,norm,act,acc,kind,per", GEMV_CASES)
def test_dec_gemv_branches(gpu, M, N, K, wdt, norm, act, acc, kind, per):
    """dec_gemv_kernel at 1 / 2 / 4 weight rows per wave, the stream kernel, dec_gemv_lds at 1 / 2 rows per wave
    and the row-chunk loop of launch_dec_gemv, each with bias, an activation and padded ldx / ldw / ldy."""
    c = Case(f"gemv-{M}-{N}-{K}-{wdt}", M, N, K, wdt, norm, act, acc)
    assert _rows_per_launch(c) == per
    got, k = c.run(swizzle=0)
    assert k == kind
    c.check(got, f"dec_gemv M={M} N={N} K={K} {'f16' if wdt else 'bf16'} norm={norm} act={act} acc={acc} [{k}, {per} rows]")


# ---------------------------------------------------------------- d. launch_silu_mul
@pytest.mark.parametrize("rows,I,padg,padh", [(3, 6848, 0, 0), (5, 20, 4, 4)])
def test_silu_mul(gpu, rows, I, padg, padh):
    """h = silu(g) * u on [gate | up] rows (the dense MLP between its two matrix-core launches at 3..8 pages) vs
    candle's g / (1 + exp(-g)) * u in f64 rounded to f32, within 4 ulp of f32 (expf and the division are each
    within about 1 ulp; the margin covers the product).  Gate values include +-30 and 0."""
    rng = np.random.default_rng(rows * 100003 + I)
    ldg, ldh = 2 * I + padg, I + padh
    g = (3.0 * rng.standard_normal((rows, I))).astype(F32)
    u = (rng.standard_normal((rows, I)) * np.exp(rng.standard_normal((rows, I)))).astype(F32)
    g[:, 0], g[:, 1], g[:, 2], g[0, 3] = 30.0, -30.0, 0.0, -0.0
    gb = np.full((rows, ldg), np.nan, F32)
    gb[:, :I], gb[:, I:2 * I] = g, u
    hb = np.full((rows, ldh), Y_PAD, np.uint32).view(F32)
    hb[:, :I] = np.nan
    dg, dh = Dev(gb), Dev(hb)
    check(lib().dsocr_k_silu_mul(rows, I, dg.ptr, ldg, dh.ptr, ldh))
    out = dh.get()
    assert np.all(out[:, I:].view(np.uint32) == Y_PAD), "h padding overwritten"
    got = out[:, :I]
    g64, u64 = g.astype(np.float64), u.astype(np.float64)
    ref = (g64 / (1.0 + np.exp(-g64)) * u64).astype(F32)
    assert np.all(np.isfinite(got))
    ulps = np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref))
    print(f"silu_mul rows={rows} I={I}: max error {float(np.max(ulps)):.2f} ulp")
    assert np.all(ulps <= 4.0), float(np.max(ulps))
    assert np.all(got[:, 2] == 0)
