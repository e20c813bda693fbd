"""The numpy model of the screened lm_head (lmhead.hip) that tests/test_screened_head.py compares the kernels
against, and its own checks (no GPU).

Model (every formula is the one in lmhead.hip's header comments, in f64 on the 16-bit rows):
  load time   s = max|w| / 127 in f32 (1 for a zero row), q = clip(rint(w / s), +-127) with the f32 division,
              E = ||w - s q||, bound = E + g (||w|| + s ||q||) with g = 2 K u, u = 2^-24, qnorm = s ||q||
  one token   A = s (x . q), half-width e = ||x|| bound
  3..8 tokens x~ = t1 Xh + t2 Xl (t1 = max|x| / 127, Xh = rint(x / t1), t2 = t1 / 254, Xl = rint((x - t1 Xh) / t2)),
              A = s (t1 Xh.q + t2 Xl.q), e = ||x|| bound + qnorm ||x - x~||
  fragments   q[v][k] at [v / 16][k / 64][v % 16 + 16 ((k % 64) / 16)][k % 16], a zero last tile past V
"""
import os
import re

import numpy as np
import pytest

from _dev import bf16_round, bf16_to_f32, f16_bits
from oracle.decoder import rms_norm

U = 2.0 ** -24
BF16, F16 = 0, 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- 16-bit storage
def round16(x, wdt):
    """f32 -> the storage type's bits (round to nearest even)."""
    return bf16_round(x) if wdt == BF16 else f16_bits(x)


def bits_to_f32(bits, wdt):
    bits = np.ascontiguousarray(bits, np.uint16)
    return bf16_to_f32(bits) if wdt == BF16 else bits.view(np.float16).astype(np.float32)


# ---------------------------------------------------------------- load-time quantisation
def quant_model(bits, wdt):
    """-> q int8 [V][K], scale f32 [V], bound f64 [V], qnorm f64 [V] (the two f64 ones before any rounding up)."""
    w = bits_to_f32(bits, wdt)
    K = w.shape[1]
    mx = np.abs(w).max(axis=1)
    s = np.where(mx > 0, mx / np.float32(127.0), np.float32(1.0)).astype(np.float32)
    with np.errstate(over="ignore"):
        q = np.clip(np.rint(w / s[:, None]), -127.0, 127.0).astype(np.float32)
    w64, s64, q64 = w.astype(np.float64), s.astype(np.float64), q.astype(np.float64)
    e2 = ((w64 - s64[:, None] * q64) ** 2).sum(axis=1)
    w2 = (w64 * w64).sum(axis=1)
    q2 = (q64 * q64).sum(axis=1)
    g = 2.0 * K * U
    bound = np.sqrt(e2) + g * (np.sqrt(w2) + s64 * np.sqrt(q2))
    return q.astype(np.int8), s, bound, s64 * np.sqrt(q2)


def frag_index(v, k, K):
    """Flat index of q[v][k] in the fragment-ordered copy."""
    v, k = np.asarray(v, np.int64), np.asarray(k, np.int64)
    kk = k & 63
    return (((v >> 4) * (K >> 6) + (k >> 6)) * 64 + (v & 15) + 16 * (kk >> 4)) * 16 + (kk & 15)


def frag_model(q):
    V, K = q.shape
    out = np.zeros((V + 15) // 16 * 16 * K, np.int8)
    v, k = np.meshgrid(np.arange(V), np.arange(K), indexing="ij")
    out[frag_index(v, k, K)] = q
    return out


# ---------------------------------------------------------------- per-step intervals
def planes_model(xn):
    """The matrix-core form's two int8 planes of one normalised row (f32) -> t1, t2 (f32), Xh, Xl (f64 integers)."""
    xn = np.asarray(xn, np.float32)
    mx = np.float32(np.abs(xn).max()) if np.isfinite(xn).any() else np.float32(0)
    t1 = np.float32(mx / np.float32(127.0)) if mx > 0 else np.float32(1.0)
    t2 = np.float32(t1 / np.float32(254.0))
    h = np.clip(np.rint(xn / t1), -127.0, 127.0).astype(np.float32)
    r = (xn.astype(np.float64) - np.float64(t1) * h.astype(np.float64)).astype(np.float32)  # fmaf(-t1, h, x)
    lo = np.clip(np.rint(r / t2), -127.0, 127.0).astype(np.float32)
    return t1, t2, h.astype(np.float64), lo.astype(np.float64)


def intervals_model(xn, q, s, bound, qnorm, matrix_core):
    """-> A, e (f64 [V]) for one normalised row: the interval [A - e, A + e] the screened lm_head gives row v."""
    x64 = np.asarray(xn, np.float32).astype(np.float64)
    q64, s64 = q.astype(np.float64), s.astype(np.float64)
    nrm = np.sqrt((x64 * x64).sum())
    if not matrix_core:
        return s64 * (q64 @ x64), nrm * bound
    t1, t2, h, lo = planes_model(xn)
    xt = np.float64(t1) * h + np.float64(t2) * lo
    errn = np.sqrt(((x64 - xt) ** 2).sum())
    A = s64 * (np.float64(t1) * (q64 @ h) + np.float64(t2) * (q64 @ lo))
    return A, nrm * bound + qnorm * errn


# ---------------------------------------------------------------- the near-tie ensemble
M_ENS = 64


def ensemble_positions(V, B, m=M_ENS):
    """m row indices per token row at the kernels' edges: row 0 and row V - 1, and pairs (8 t + 7, 8 t + 8) - the
    single-token kernel's group edge, every second one also the 16-row tile edge - spread evenly over the whole
    vocabulary (at the model's size that puts them in every wave's first and later groups and tiles)."""
    pairs = [(0, V - 1)] + [(8 * t + 7, 8 * t + 8) for t in range((V - 9) // 8 + 1) if 8 * t + 8 < V - 1]
    assert len(pairs) >= B * (m // 2), (V, B, len(pairs))
    out = []
    for b in range(B):
        mine = [p for i, p in enumerate(pairs) if (i + i // B) % B == b]  # (rotated: both edge parities per row)
        sel = np.unique(np.linspace(0, len(mine) - 1, m // 2).astype(np.int64))
        assert len(sel) == m // 2
        out.append(np.array(sorted(i for j in sel for i in mine[j]), np.int64))
    return out


def near_tie_rows(xn_row, wdt, rng, m=M_ENS):
    """m rows round16(0.5 u + N(0, (2e-5)^2)), u = xn / ||xn||: exact logits closer than the int8 error."""
    u = (xn_row.astype(np.float64) / np.linalg.norm(xn_row.astype(np.float64)))
    rows = 0.5 * u[None, :] + rng.standard_normal((m, len(u))) * 2e-5
    return round16(rows.astype(np.float32), wdt)


def near_tie_case(B, V, K, wdt, seed, fill=True):
    """x [B][K], norm weight, the oracle's normalised rows, W bits [V][K] (fill=False: zeros outside the
    ensembles - the ensemble rows are all the host checks read) and every token row's ensemble positions."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, K)).astype(np.float32)
    nw = (1.0 + 0.05 * rng.standard_normal(K)).astype(np.float32)
    xn = rms_norm(x, nw, 1e-6)
    pos = ensemble_positions(V, B)
    ens = [near_tie_rows(xn[b], wdt, rng) for b in range(B)]
    bits = np.zeros((V, K), np.uint16)
    if fill:
        step = 8192
        for v0 in range(0, V, step):
            n = min(step, V - v0)
            bits[v0:v0 + n] = round16((rng.standard_normal((n, K)) * 0.02).astype(np.float32), wdt)
    for b in range(B):
        bits[pos[b]] = ens[b]
    return x, nw, xn, bits, pos


# (B, K) of the near-tie selection tests at V = 2043, each with bf16 and f16 rows; the seed of a case is SEEDS[...]
# where the default (its K + 17 B + wdt) does not meet the precondition below
SMALL_V = 2043
SELECT_CASES = ([(B, K, wdt) for B in (1, 2) for K in (256, 1024, 1280, 1536) for wdt in (BF16, F16)] +
                [(B, K, wdt) for B in (3, 8) for K in (768, 1024, 1280, 1536) for wdt in (BF16, F16)])
BIG_V, BIG_K, BIG_B, BIG_SEED = 129280, 1280, 8, 5
SEEDS = {}


def case_seed(B, K, wdt):
    return SEEDS.get((B, K, wdt), K + 17 * B + wdt)


def flipped_rows(xn, bits, pos, wdt, matrix_core):
    """Token rows whose int8 argmax differs from the exact (f64) argmax over their ensemble; also asserts that the
    model's interval of every ensemble row contains the f64 logit."""
    out = []
    for b in range(len(pos)):
        rows = bits[pos[b]]
        q, s, bound, qnorm = quant_model(rows, wdt)
        A, e = intervals_model(xn[b], q, s, bound, qnorm, matrix_core)
        L = bits_to_f32(rows, wdt).astype(np.float64) @ xn[b].astype(np.float64)
        assert np.all(np.abs(L - A) <= e), (b, float(np.max(np.abs(L - A) - e)))
        # the intervals overlap: the model keeps the whole ensemble
        assert np.all(A + e >= np.max(A - e))
        if int(np.argmax(A)) != int(np.argmax(L)):
            out.append(b)
    return out


# ================================================================ checks of the model itself
@pytest.mark.parametrize("wdt", [BF16, F16])
@pytest.mark.parametrize("K", [16, 256, 1280])
def test_quant_model_reconstructs_rows(wdt, K):
    """|w - s q| <= s / 2 per element (plus the f32 quotient's rounding, half an ulp of at most 127), the largest element maps to +-127, a zero row to scale 1 and q = 0, and the
    bound dominates the f64 error of the int8 dot product for random x."""
    rng = np.random.default_rng(K + wdt)
    bits = round16((rng.standard_normal((37, K)) * 0.05).astype(np.float32), wdt)
    bits[3] = 0
    bits[5] = round16(-np.abs(bits_to_f32(bits[5], wdt)) - np.float32(0.01), wdt)  # largest element negative
    q, s, bound, qnorm = quant_model(bits, wdt)
    w = bits_to_f32(bits, wdt).astype(np.float64)
    assert np.all(np.abs(w - s[:, None].astype(np.float64) * q) <= s[:, None] * (0.5 + 127 * U))
    assert np.all(np.abs(q).max(axis=1)[np.arange(37) != 3] == 127)
    assert s[3] == 1.0 and not q[3].any() and bound[3] == 0.0 and qnorm[3] == 0.0
    assert q[5].min() == -127 and q[5].max() <= 0
    x = rng.standard_normal((4, K)).astype(np.float32)
    for xr in x:
        A, e = intervals_model(xr, q, s, bound, qnorm, False)
        assert np.all(np.abs(w @ xr.astype(np.float64) - A) <= e)


@pytest.mark.parametrize("V,K", [(5, 64), (17, 128), (48, 1280), (2043, 256)])
def test_frag_index_is_the_stated_layout(V, K):
    """frag_index equals the 4-d layout [v / 16][k / 64][v % 16 + 16 ((k % 64) / 16)][k % 16] built by reshapes, maps
    the padded matrix one to one, and leaves the rows past V zero."""
    rng = np.random.default_rng(V + K)
    q = rng.integers(-127, 128, (V, K)).astype(np.int8)
    q[q == 0] = 1
    T = (V + 15) // 16
    pad = np.zeros((T * 16, K), np.int8)
    pad[:V] = q
    # [T][v % 16][k / 64][(k % 64) / 16][k % 16] -> [T][k / 64][(k % 64) / 16][v % 16][k % 16]
    ref = pad.reshape(T, 16, K // 64, 4, 16).transpose(0, 2, 3, 1, 4).reshape(-1)
    got = frag_model(q)
    assert np.array_equal(got, ref)
    v, k = np.meshgrid(np.arange(T * 16), np.arange(K), indexing="ij")
    assert len(np.unique(frag_index(v, k, K))) == T * 16 * K
    assert np.count_nonzero(got) == V * K


@pytest.mark.parametrize("K", [768, 1536])
def test_planes_model_error(K):
    """The two planes represent x to t2 / 2 per element (t2 = max|x| / (127 * 254)) and stay inside int8."""
    rng = np.random.default_rng(K)
    xn = (rng.standard_normal(K) * np.exp(rng.standard_normal())).astype(np.float32)
    t1, t2, h, lo = planes_model(xn)
    assert np.abs(h).max() == 127 and np.abs(lo).max() <= 127
    err = np.abs(xn.astype(np.float64) - (np.float64(t1) * h + np.float64(t2) * lo))
    assert err.max() <= 0.5 * t2 * (1 + 1e-5)
    t1z, t2z, hz, lz = planes_model(np.zeros(K, np.float32))
    assert t1z == 1.0 and not hz.any() and not lz.any()


def test_ensemble_positions_cover_the_edges():
    for V, B in [(SMALL_V, 1), (SMALL_V, 8), (BIG_V, BIG_B)]:
        pos = ensemble_positions(V, B)
        flat = np.concatenate(pos)
        assert len(np.unique(flat)) == B * M_ENS and flat.min() == 0 and flat.max() == V - 1
        for p in pos:
            assert len(p) == M_ENS
            assert np.any(p % 8 == 7) and np.any(p % 8 == 0) and np.any(p % 16 == 15) and np.any(p % 16 == 0)
            assert p.max() > V // 2  # spread over the vocabulary: later groups / tiles of a wave at the model's size


@pytest.mark.parametrize("B,K,wdt", SELECT_CASES)
def test_near_tie_precondition(B, K, wdt):
    """Every case the GPU tests run: the model's intervals hold the f64 logit, and for at least one token row the
    int8 argmax is NOT the exact argmax - a head that trusted A alone, or a bound too small, picks a wrong token."""
    x, nw, xn, bits, pos = near_tie_case(B, SMALL_V, K, wdt, case_seed(B, K, wdt))
    w = bits_to_f32(bits, wdt).astype(np.float64)
    for b in range(B):  # the fill rows stay far below the ensemble
        L = w @ xn[b].astype(np.float64)
        rest = np.ones(SMALL_V, bool)
        rest[pos[b]] = False
        assert L[rest].max() < L[pos[b]].min() - 1.0
    assert flipped_rows(xn, bits, pos, wdt, B >= 3), "precondition: choose another seed"


@pytest.mark.parametrize("B", [1, 2, 3, 8])
def test_near_tie_precondition_model_vocabulary(B):
    """The same at V = 129280 (the ensembles' rows only: the host never forms the whole matrix)."""
    x, nw, xn, bits, pos = near_tie_case(BIG_B, BIG_V, BIG_K, BF16, BIG_SEED, fill=False)
    assert flipped_rows(xn[:B], bits, pos[:B], BF16, B >= 3), "precondition: choose another seed"


def test_screen_steps_struct_matches_the_header():
    """ScreenStepsC lists the fields of dsocr_screen_steps in the header's order."""
    from dsocr._lib import ScreenStepsC
    header = open(os.path.join(ROOT, "include", "dsocr.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} dsocr_screen_steps;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        parts = decl.split(",")
        for i, p in enumerate(parts):
            names.append(re.findall(r"[A-Za-z_][A-Za-z0-9_]*", p)[-1])
    assert names == [f[0] for f in ScreenStepsC._fields_]
