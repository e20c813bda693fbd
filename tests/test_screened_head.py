"""The screened lm_head (lmhead.hip + dec_screen_final_kernel) on MI355X, part by part, through
dsocr_k_lmhead_screen_steps: the load-time quantisation, the intervals and kept lists of one step, the token, and
the final kernel's branches (ban chain, bookkeeping, embedding hand-off).

References.  A logit: the exact kernel, dsocr_k_gemv on the same rows (the head's contract names it); numpy f64 on
the 16-bit weights checks that reference with the term the bound reserves for it, |L_gemv - L_f64| <= 2 K u ||x||
||W_v||, u = 2^-24 (g in lmhead_quantize_kernel).  Selection and bookkeeping: oracle.decoder.select_token_id in a
plain Python loop.  The interval model: tests/test_screened_head_host.py.

Tolerances and the constants in the code they come from:
  bound, qnorm in [f64 formula, formula (1 + 1e-5) + 2e-30]: lmhead_quantize_kernel multiplies by (1 + 1e-6), adds
      1e-30 (bound only) and rounds up to f32 once (2^-23 relative); 1e-5 keeps a vacuous bound from passing.
  cand_hi - L <= 2 e_model (1 + 1e-3) + 1e-6 |L|: the kernels widen e_model by ||x|| rounded up (single token:
      sqrt(1 + 1e-4) (1 + 1e-6) in nrm_s; matrix cores: 1 + 1e-9), bound / qnorm as above, (1 + 4.8e-7) resp.
      (1 + 1e-6) on e, and add |A| 3.6e-7 resp. |A| 1e-12: together below e_model 1e-3 + 1e-6 |L|.
  cand_hi >= A_model + e_model (1 - 1e-9) - acc - 1e-6 |A|: the kernels' e is the model's rounded up; acc = 0 for
      the matrix-core form (A is exact integers scaled in f64), K u ||x|| s||Q|| for the single-token form (the
      bound of its K-term f32 dot product).  This side fails when a term of the bound is missing.
  xn_out: the row dec_gemv stages (its own xn_out, returned by the entry): bitwise, in both forms.
"""
import ctypes as C

import numpy as np
import pytest

from _dev import Dev
from dsocr._lib import EINVAL, RowParamsC, ScreenStepsC, check, lib
from oracle.decoder import banned_ngram_tokens, select_token_id
from test_screened_head_host import (BF16, BIG_B, BIG_K, BIG_SEED, BIG_V, F16, SELECT_CASES, SMALL_V, U, bits_to_f32,
                                     case_seed, frag_model, intervals_model, near_tie_case, near_tie_rows, quant_model,
                                     round16)

pytestmark = pytest.mark.gpu
EPS = 1e-6
LQ_BANS, LM_BANS, SP_LIST, SP_PM, E_REGS = 256, 128, 1024, 256, 16  # lmhead.hip / decode_sample.hip


# ---------------------------------------------------------------- the entry
def grid(B, V, K):
    nblk, slot, mm = C.c_int(), C.c_longlong(), C.c_int()
    check(lib().dsocr_k_lmhead_screen_grid(B, V, K, C.byref(nblk), C.byref(slot), C.byref(mm)))
    return nblk.value, slot.value, bool(mm.value)


class Run:
    pass


def screen_steps(bits, wdt, x=None, nw=None, ctx=None, ctx_len=None, ngram=0, eos=-1, rows=None, ban=None, out_cap=16,
                 table=None, table_dt=BF16, probe=0, want_frag=None):
    """One call of dsocr_k_lmhead_screen_steps; x [steps][B][K] (None: quantise only).  -> Run with every output."""
    V, K = bits.shape
    s, r, keep = ScreenStepsC(), Run(), []

    def ptr(a):
        keep.append(a)
        return a.ctypes.data_as(C.c_void_p)

    def out(name, shape, dtype):
        a = np.zeros(shape, dtype)
        setattr(r, name, a)
        setattr(s, name, ptr(a))

    bits = np.ascontiguousarray(bits, np.uint16)
    s.V, s.K, s.wdtype, s.W = V, K, wdt, ptr(bits)
    s.B, s.steps = 1, 0
    frag = K % 64 == 0 if want_frag is None else want_frag
    out("q", (V, K), np.int8); out("scale", V, np.float32); out("bound", V, np.float32)
    if frag:
        out("qnorm", V, np.float32); out("qfrag", (V + 15) // 16 * 16 * K, np.int8)
    if x is not None:
        x = np.ascontiguousarray(x, np.float32)
        steps, B, _ = x.shape
        s.B, s.steps, s.probe, s.x, s.ldx = B, steps, probe, ptr(x), K
        s.norm_w, s.eps = ptr(np.ascontiguousarray(nw, np.float32)), EPS
        if ctx is None:
            ctx, ctx_len = np.zeros((B, 8), np.int32), np.zeros(B, np.int32)
        ctx = np.ascontiguousarray(ctx, np.int32)
        cap = ctx.shape[1]
        s.ctx, s.ctx_cap, s.ctx_len = ptr(ctx), cap, ptr(np.ascontiguousarray(ctx_len, np.int32))
        s.ngram, s.eos, s.out_cap = ngram, eos, out_cap
        if rows is not None:
            arr = (RowParamsC * B)()
            for b, (g, e) in enumerate(rows):
                arr[b].no_repeat_ngram_size, arr[b].eos_token_id, arr[b].repetition_penalty = g, e, 1.0
            keep.append(arr)
            s.rows = C.cast(arr, C.POINTER(RowParamsC))
        s.ban_ld = cap + 1
        if ban is not None:
            full = np.zeros((B, cap + 1), np.int32)
            for b, lst in enumerate(ban):
                full[b, 0] = len(lst)
                full[b, 1:1 + len(lst)] = lst
            s.ban = ptr(full)
        nblk, slot, mm = grid(B, V, K)
        r.nblk, r.slot, r.mm = nblk, slot, mm
        out("out_tok", (steps, B), np.int32); out("ban_out", (steps, B, cap + 1), np.int32)
        out("ctx_out", (steps, B, cap), np.int32); out("ctx_len_out", (steps, B), np.int32)
        out("out_ids", (steps, B, out_cap), np.int32)
        for n in ("out_len", "done", "kv_pos", "kv_len"):
            out(n, (steps, B), np.int32)
        out("blk_cnt", (B, nblk), np.int32); out("blk_t", (B, nblk), np.float32)
        out("cand", (B, slot, nblk), np.int32); out("cand_hi", (B, slot, nblk), np.float32)
        out("xn_out", (B, K), np.float32); out("xn_gemv", (B, K), np.float32)
        if table is not None:
            table = np.ascontiguousarray(table, np.uint16)
            s.table, s.table_dt, s.H = ptr(table), table_dt, table.shape[1]
            out("x_next", (steps, B, table.shape[1]), np.float32)
    check(lib().dsocr_k_lmhead_screen_steps(C.byref(s)))
    return r


def gemv_logits(x, nw, bits, wdt, dW=None):
    """The exact head: dsocr_k_gemv (fused RMSNorm) -> f32 [B][V]."""
    B, K = x.shape
    V = bits.shape[0]
    dx, dn, dW, dy = Dev(x), Dev(nw), dW or Dev(bits), Dev.zeros((B, V))
    check(lib().dsocr_k_gemv(B, V, K, dx.ptr, dn.ptr, EPS, dW.ptr, wdt, None, dy.ptr, 0, 0))
    return dy.get()


def rms_norm64(x, nw):
    x64 = x.astype(np.float64)
    return x64 / np.sqrt((x64 * x64).mean(axis=-1, keepdims=True) + EPS) * nw.astype(np.float64)


def check_gemv_reference(L, xn, bits, wdt, rows=None):
    """|L_gemv - L_f64| <= 2 K u ||x|| ||W_v|| (the g term of the bound), xn the staged rows [B][K]; rows: the
    vocabulary rows to check (default all)."""
    rows = np.arange(bits.shape[0]) if rows is None else rows
    w = bits_to_f32(bits[rows], wdt).astype(np.float64)
    K = w.shape[1]
    wn = np.sqrt((w * w).sum(axis=1))
    for b in range(len(xn)):
        x64 = xn[b].astype(np.float64)
        ref = w @ x64
        lim = 2.0 * K * U * np.linalg.norm(x64) * wn
        assert np.all(np.abs(L[b][rows] - ref) <= lim), (b, float(np.max(np.abs(L[b][rows] - ref) - lim)))


def first_argmax(L, banned=()):
    row = np.where(np.isfinite(L), L, -np.inf).astype(np.float32)
    row[list(banned)] = -np.inf
    return int(np.argmax(row))


def check_invariants(r, L, bits, wdt, banned=None):
    """The layout-independent properties of one step's kept lists: L [B][V] the exact logits, banned the lists
    the step read."""
    B, V = L.shape
    for b in range(B):
        ban = set(banned[b]) if banned else set()
        ok = np.ones(V, bool)
        ok[list(ban)] = False
        cnt = r.blk_cnt[b]
        assert cnt.min() >= 0 and cnt.max() <= r.slot
        T = float(r.blk_t[b].max())
        assert T <= L[b][ok].max(), (b, T, L[b][ok].max())
        kept, hi = [], []
        for j in np.nonzero(cnt)[0]:
            kept.append(r.cand[b, :cnt[j], j])
            hi.append(r.cand_hi[b, :cnt[j], j])
        kept, hi = np.concatenate(kept), np.concatenate(hi)
        assert kept.min() >= 0 and kept.max() < V
        assert len(np.unique(kept)) == len(kept), "a row kept twice"
        assert not ban & set(kept.tolist()), "a banned row kept"
        must = np.nonzero(ok & (L[b] >= T))[0]
        assert np.isin(must, kept).all(), (b, must[~np.isin(must, kept)][:8])
        assert np.all(hi >= L[b][kept]), (b, float(np.min(hi - L[b][kept])))
        q, s, bound, qnorm = quant_model(bits[kept], wdt)
        A, e = intervals_model(r.xn_out[b], q, s, bound, qnorm, r.mm)
        # ... and no narrower than the model's interval: cand_hi >= A + e.  The matrix-core form's A is exact integer
        # arithmetic scaled in f64 (its 1e-12 |A| fudge and the f32 round-up are far below 1e-6 |A|); the
        # single-token form accumulates A in f32, at most K u ||x|| s||Q|| away from the model's (the standard
        # bound of a K-term f32 dot product), plus one rounding of s * sum
        nrm = np.linalg.norm(r.xn_out[b].astype(np.float64))
        acc = 0.0 if r.mm else bits.shape[1] * U * nrm * qnorm
        floor = A + e * (1 - 1e-9) - acc - 1e-6 * np.abs(A)
        assert np.all(hi >= floor), (b, float(np.min(hi - floor)))
        slack = 2.0 * e * (1 + 1e-3) + 1e-6 * np.abs(L[b][kept])
        assert np.all(hi - L[b][kept] <= slack), (b, float(np.max(hi - L[b][kept] - slack)))


def check_xn(r, x, nw):
    """The staged row against the exact kernel's: both forms run dec_gemv's staging arithmetic, bit for bit; and
    that row is near the f64 RMSNorm."""
    ulp = np.spacing(np.abs(r.xn_gemv))
    d = np.abs(r.xn_out.astype(np.float64) - r.xn_gemv.astype(np.float64)) / ulp
    print("xn_out vs dec_gemv's staged row: max %.2f ulp (matrix cores: %s)" % (d.max(), r.mm))
    assert np.array_equal(r.xn_out.view(np.uint32), r.xn_gemv.view(np.uint32)), float(d.max())
    ref = rms_norm64(x, nw)
    assert np.all(np.abs(r.xn_gemv - ref) <= 4e-7 * np.abs(ref))  # three f32 roundings and the f32 sum of squares


# ================================================================ quantisation
def _quant_rows(V, K, wdt):
    rng = np.random.default_rng(V * 31 + K + wdt)
    w = (rng.standard_normal((V, K)) * np.exp(rng.standard_normal((V, 1)))).astype(np.float32) * np.float32(0.03)
    bits = round16(w, wdt)
    bits[1] = 0                                                            # a zero row
    bits[2] = round16(-np.abs(bits_to_f32(bits[2], wdt)) - np.float32(1e-3), wdt)  # the largest element negative
    bits[3, K // 2] = 0x7F7F if wdt == BF16 else 0x7BFF                    # the type's largest finite value
    bits[4, 0] = 0xFF7F if wdt == BF16 else 0xFBFF                         # ... and its negative
    return bits


@pytest.mark.parametrize("wdt", [BF16, F16])
@pytest.mark.parametrize("V", [5, 17, 2043, 2048])
@pytest.mark.parametrize("K", [16, 256, 768, 1024, 1280, 1536])
def test_quantisation(gpu, V, K, wdt):
    """q and scale equal the model exactly; bound and qnorm are the f64 formula rounded up by no more than the
    kernel's own factors; qfrag is the fragment permutation of q with a zero tail tile."""
    bits = _quant_rows(V, K, wdt)
    r = screen_steps(bits, wdt)
    q, s, bound, qnorm = quant_model(bits, wdt)
    assert np.array_equal(r.scale, s)
    assert np.array_equal(r.q, q)
    b64 = r.bound.astype(np.float64)
    assert np.all(b64 >= bound) and np.all(b64 <= bound * (1 + 1e-5) + 2e-30), float(np.max(b64 / np.maximum(bound, 1e-300)))
    if K % 64 == 0:
        n64 = r.qnorm.astype(np.float64)
        assert np.all(n64 >= qnorm) and np.all(n64 <= qnorm * (1 + 1e-5))
        assert np.array_equal(r.qfrag, frag_model(q))  # (frag_model leaves the tail tile's rows past V zero)


def test_entry_refuses_shapes_outside_the_contract(gpu):
    bits = np.zeros((32, 24), np.uint16)
    s = ScreenStepsC()
    s.B, s.V, s.K, s.W = 1, 32, 24, bits.ctypes.data_as(C.c_void_p)
    assert lib().dsocr_k_lmhead_screen_steps(C.byref(s)) == EINVAL          # K % 16
    n, sl, mm = C.c_int(), C.c_longlong(), C.c_int()
    for B, V, K in [(1, 32, 1552), (3, 32, 256), (9, 32, 1280), (3, 8, 1280), (1, 32, 8)]:
        assert lib().dsocr_k_lmhead_screen_grid(B, V, K, C.byref(n), C.byref(sl), C.byref(mm)) == EINVAL, (B, V, K)
    assert grid(2, 2043, 1536)[2] is False and grid(3, 2043, 1536)[2] is True


# ================================================================ near ties: intervals + token
def _near_tie_check(B, V, K, wdt, x, nw, bits, pos, L=None, ban_winner=False, ref_rows=None):
    L = gemv_logits(x, nw, bits, wdt) if L is None else L
    banned = None
    if ban_winner:  # the ensemble's exact winner of every token row is banned: the runner-up must win
        banned = [[first_argmax(L[b])] for b in range(B)]
    r = screen_steps(bits, wdt, x[None], nw, ban=banned)
    check_gemv_reference(L, r.xn_gemv, bits, wdt, ref_rows)
    check_invariants(r, L, bits, wdt, banned)
    for b in range(B):
        want = first_argmax(L[b], banned[b] if banned else ())
        assert r.out_tok[0, b] == want, (b, int(r.out_tok[0, b]), want)
        assert want in pos[b]
        if ban_winner:
            assert want != banned[b][0]
    return r


@pytest.mark.parametrize("B,K,wdt", SELECT_CASES)
def test_near_tie_selection(gpu, B, K, wdt):
    """64 rows per token whose exact logits differ by less than the int8 error, placed at group / tile edges: the
    token is the exact kernel's first-index argmax, and the kept lists obey the interval invariants.  (The host
    file asserts that the int8 argmax alone would pick another row in every one of these cases.)"""
    x, nw, xn, bits, pos = near_tie_case(B, SMALL_V, K, wdt, case_seed(B, K, wdt))
    r = _near_tie_check(B, SMALL_V, K, wdt, x, nw, bits, pos)
    assert r.mm == (B >= 3)
    for b in range(B):  # the whole ensemble survives to the rescoring
        kept = np.concatenate([r.cand[b, :r.blk_cnt[b, j], j] for j in range(r.nblk)])
        assert np.isin(pos[b], kept).all()


@pytest.mark.parametrize("B,K,wdt", SELECT_CASES)
def test_staged_row_is_the_exact_kernels(gpu, B, K, wdt):
    """xn_out, the row the rescoring reads, is the row dec_gemv stages from the same input (the entry returns both),
    bit for bit, in both forms.  (Before the sum of squares became one helper with contraction off, and the
    matrix-core form summed it in dec_gemv's order, 11 of these 32 cases were 2 to 4 ulp apart.)"""
    x, nw, xn, bits, pos = near_tie_case(B, SMALL_V, K, wdt, case_seed(B, K, wdt))
    check_xn(screen_steps(bits, wdt, x[None], nw), x, nw)


@pytest.mark.parametrize("B,K", [(1, 1280), (2, 256), (3, 1280), (8, 768)])
def test_near_tie_winner_banned(gpu, B, K):
    x, nw, xn, bits, pos = near_tie_case(B, SMALL_V, K, BF16, case_seed(B, K, BF16))
    _near_tie_check(B, SMALL_V, K, BF16, x, nw, bits, pos, ban_winner=True)


@pytest.fixture(scope="module")
def big_case():
    x, nw, xn, bits, pos = near_tie_case(BIG_B, BIG_V, BIG_K, BF16, BIG_SEED)
    return x, nw, bits, pos, Dev(bits)


@pytest.mark.parametrize("B", [1, 2, 3, 8])
def test_near_tie_selection_model_vocabulary(gpu, big_case, B):
    """V = 129280, K = 1280: a wave walks several groups / tiles; one weight matrix for the four row counts.  (More
    lm_head blocks than the final kernel has threads does not happen here: the grid is capped by the resident
    blocks, 768 on MI355X; test_more_blocks_than_final_threads reaches that branch.)"""
    x, nw, bits, pos, dW = big_case
    L = gemv_logits(x[:B], nw, bits, BF16, dW)  # the exact head as it runs for B rows
    # (the f64 check of the reference on every ensemble row and every 97th row of the rest)
    ref_rows = np.unique(np.concatenate(pos + [np.arange(0, BIG_V, 97)]))
    r = _near_tie_check(B, BIG_V, BIG_K, BF16, x[:B], nw, bits, pos[:B], L=L, ref_rows=ref_rows)
    if r.mm:
        tile = pos[0] // 16
        assert np.any(tile % (r.slot // 16) >= 8), "no ensemble row in a wave's second tile"
    else:
        group = pos[0] // 8
        assert np.any(group >= 4 * r.nblk), "no ensemble row in a wave's second group"


def test_stream_and_row_kernels_stage_the_same_row(gpu, big_case):
    """The exact lm_head at the model's vocabulary is dec_gemv_stream, which has no xn_out to return; the row the
    staged-row test compares with comes from dec_gemv_kernel.  Their per-row arithmetic is the same, so their logits
    on the same weight rows are bitwise equal exactly when their staged rows are: checked for one and two tokens."""
    x, nw, bits, pos, dW = big_case
    n = 4096
    for B in (1, 2):
        kinds = []
        for N in (BIG_V, n):
            k = C.c_char_p()
            check(lib().dsocr_k_gemv_kind(B, N, BIG_K, BIG_K, BF16, 1, 0, 0, C.byref(k), None))
            kinds.append(k.value.decode())
        assert kinds == ["dec_gemv_stream", "dec_gemv_rb1"], kinds
        big = gemv_logits(x[:B], nw, bits, BF16, dW)[:, :n]
        small = gemv_logits(x[:B], nw, bits[:n], BF16)
        assert np.array_equal(big.view(np.uint32), small.view(np.uint32)), float(np.max(np.abs(big - small)))


# ================================================================ final-kernel branches
@pytest.mark.parametrize("far_first", [False, True])
def test_more_blocks_than_final_threads(gpu, far_first):
    """V = 1 050 000 at K = 16: the block lists are bounded by LQ_LIST rows, so the single-token grid has more than
    1024 blocks and the final kernel's threads each reduce a second block (threshold and kept rows).  The winner
    sits in a block past the 1024th with the runner-up in block 0, and the other way round."""
    V, K = 1050000, 16
    rng = np.random.default_rng(11)
    x = rng.standard_normal((1, K)).astype(np.float32)
    nw = np.ones(K, np.float32)
    bits = round16((rng.standard_normal((V, K)) * 0.02).astype(np.float32), BF16)
    nblk, slot, mm = grid(1, V, K)
    assert nblk > 1024 and not mm, nblk
    u = (rms_norm64(x, nw)[0] / np.linalg.norm(rms_norm64(x, nw)[0])).astype(np.float32)
    near, far = 3, 8 * (4 * (nblk - 1) + 2) + 5   # rows of block 0 and of the last block (group 4 j + wave)
    assert far < V
    bits[far if far_first else near] = round16(0.5 * u, BF16)
    bits[near if far_first else far] = round16(0.45 * u, BF16)
    L = gemv_logits(x, nw, bits, BF16)
    r = screen_steps(bits, BF16, x[None], nw)
    assert r.nblk == nblk
    want = first_argmax(L[0])
    assert want == (far if far_first else near)
    assert r.out_tok[0, 0] == want, (int(r.out_tok[0, 0]), want)
    check_invariants(r, L, bits, BF16)
    blocks = {int(j) for j in range(nblk) for v in r.cand[0, :r.blk_cnt[0, j], j] if v in (near, far)}
    assert 0 in blocks and max(blocks) >= 1024, blocks


@pytest.mark.parametrize("B,K,wdt", [(1, 256, BF16), (2, 1280, F16), (3, 1280, BF16)])
def test_more_survivors_than_the_list(gpu, B, K, wdt):
    """Every row identical: all V > SP_LIST rows survive and are rescored from the block slots; token 0.  With rows
    0..k banned through a list longer than LQ_BANS / LM_BANS (read from global memory): the first unbanned row."""
    V = 4100
    rng = np.random.default_rng(K + B)
    x = rng.standard_normal((B, K)).astype(np.float32)
    nw = (1.0 + 0.05 * rng.standard_normal(K)).astype(np.float32)
    bits = np.tile(round16((rng.standard_normal(K) * 0.05).astype(np.float32), wdt), (V, 1))
    L = gemv_logits(x, nw, bits, wdt)
    assert V > SP_LIST
    nban = max(LQ_BANS, LM_BANS) + 44
    ctx, n = np.zeros((B, nban + 20), np.int32), np.zeros(B, np.int32)
    for banned in (None, [list(range(nban))[::-1] if b % 2 else list(range(nban)) for b in range(B)]):
        r = screen_steps(bits, wdt, x[None], nw, ctx=ctx, ctx_len=n, ban=banned)
        check_invariants(r, L, bits, wdt, banned)
        assert np.all(r.out_tok[0] == (nban if banned else 0)), r.out_tok[0]
        assert r.blk_cnt.sum() == B * (V - (nban if banned else 0))
        if not r.mm:
            assert r.blk_cnt.max() > E_REGS  # entries past the final kernel's preloaded 16 per block


@pytest.mark.parametrize("B,K", [(2, 256), (3, 1280)])
def test_non_finite_rows(gpu, B, K):
    """An input row holding Inf or NaN: the token of the exact head on the same input (dsocr_k_sample_greedy on
    dsocr_k_gemv's logits) and of select_token_id on those logits; the finite rows beside it are unaffected."""
    V = 600
    rng = np.random.default_rng(K)
    x = rng.standard_normal((B, K)).astype(np.float32)
    x[0, 5] = np.inf
    if B > 2:
        x[1, K - 1] = np.nan
    nw = (1.0 + 0.05 * rng.standard_normal(K)).astype(np.float32)
    bits = round16((rng.standard_normal((V, K)) * 0.02).astype(np.float32), BF16)
    L = gemv_logits(x, nw, bits, BF16)
    dl, dc, dn, dt = Dev(L), Dev.zeros((B, 8), np.int32), Dev.zeros(B, np.int32), Dev.zeros(B, np.int32)
    check(lib().dsocr_k_sample_greedy(B, V, dl.ptr, dc.ptr, 8, dn.ptr, 0, 1.0, dt.ptr))
    exact = dt.get()
    r = screen_steps(bits, BF16, x[None], nw)
    for b in range(B):
        oracle = select_token_id(L[b], [], 1.0, None)
        assert exact[b] == oracle, (b, exact[b], oracle)
        assert r.out_tok[0, b] == oracle, (b, int(r.out_tok[0, b]), oracle)
    assert not np.isfinite(L[0]).all() and np.isfinite(L[B - 1]).all()


def _chain_case(B, K, seed):
    """Six dominant rows (graded, far apart against the int8 error) and contexts that repeat them, so the n-gram ban
    decides most steps; x differs a little from step to step."""
    V, steps, cap = 600, 8, 320
    rng = np.random.default_rng(seed)
    nw = (1.0 + 0.05 * rng.standard_normal(K)).astype(np.float32)
    x0 = rng.standard_normal((B, K)).astype(np.float32)
    x = (x0[None] + 0.02 * rng.standard_normal((steps, B, K))).astype(np.float32)
    bits = round16((rng.standard_normal((V, K)) * 0.01).astype(np.float32), BF16)
    dom = [7, 8, 15, 16, 599, 0]
    mean_dir = rms_norm64(x0, nw).mean(axis=0)
    u = mean_dir / np.linalg.norm(mean_dir)
    for j, t in enumerate(dom):
        bits[t] = round16(((0.5 - 0.03 * j) * u).astype(np.float32), BF16)
    return V, steps, cap, x, nw, bits, dom


def _ban_list(seq, g):
    """The next step's banned ids with their multiplicity (banned_ngram_tokens keeps the set)."""
    if g <= 1 or len(seq) < g - 1:
        return []
    pre = seq[len(seq) - (g - 1):]
    return [seq[i + g - 1] for i in range(len(seq) - g + 1) if seq[i:i + g - 1] == pre]


def _chain_reference(Ls, ctx0, params, out_cap, cap):
    """select_token_id + the step bookkeeping of decode_sample.hip's final kernels, one page: per step the token,
    ban list, context, output, done, or None where the page had finished before the step (its slots are unread)."""
    seq, outs, done, kv, rec = list(ctx0), [], 0, len(ctx0), []
    g, eos = params
    for L in Ls:
        live = not done
        tok = select_token_id(L, seq, 1.0, g if g > 1 else None) if live else None
        if live:
            if eos >= 0 and tok == eos:
                done = 1
            else:
                if len(outs) < out_cap:
                    outs.append(tok)
                if len(outs) >= out_cap:
                    done = 1
                if len(seq) < cap:
                    seq.append(tok)
        kv += 1
        took = live and not (eos >= 0 and tok == eos)
        rec.append(dict(tok=tok, ban=sorted(_ban_list(seq, g)) if took else None, seq=list(seq), outs=list(outs),
                        done=done, kv=kv))
    return rec


def _chain_compare(r, b, rec, g):
    for t, e in enumerate(rec):
        if e["tok"] is not None:
            assert r.out_tok[t, b] == e["tok"], (t, b, int(r.out_tok[t, b]), e["tok"])
        if e["ban"] is not None:
            n = r.ban_out[t, b, 0]
            assert n == len(e["ban"]) and sorted(r.ban_out[t, b, 1:1 + n].tolist()) == e["ban"], (t, b, n, e["ban"])
            assert set(e["ban"]) == banned_ngram_tokens(e["seq"], g)
        assert r.ctx_len_out[t, b] == len(e["seq"]) and r.ctx_out[t, b, :len(e["seq"])].tolist() == e["seq"], (t, b)
        assert r.out_len[t, b] == len(e["outs"]) and r.out_ids[t, b, :len(e["outs"])].tolist() == e["outs"], (t, b)
        assert r.done[t, b] == e["done"], (t, b)
        assert r.kv_pos[t, b] == e["kv"] and r.kv_len[t, b] == e["kv"], (t, b)


CHAIN = [  # (B, K, ngram, context lengths, eos, out_cap, a page finishes)
    (2, 256, 2, [280, 12], 599, 16, True),    # ngram 2: every position a prefix match; 280 > SP_PM: the rescan; EOS
    (2, 256, 3, [40, 300], -1, 5, True),      # the fast path; out_cap reached at step 5
    (2, 1280, 20, [3, 60], 16, 16, False),    # a context shorter than ngram - 1 beside one with 19-token matches
    (3, 1280, 3, [41, 290, 1], 15, 6, True),  # the matrix-core form; EOS or out_cap
    (3, 1280, 2, [300, 2, 0], -1, 16, False),  # ... more than SP_PM matches, an empty context
]


def _chain_inputs(case):
    B, K, g, lens, eos, out_cap = case[:6]
    V, steps, cap, x, nw, bits, dom = _chain_case(B, K, K + g + B)
    ctx = np.zeros((B, cap), np.int32)
    for b, n in enumerate(lens):
        ctx[b, :n] = np.tile(np.array(dom[:5 - b % 2], np.int32), cap // 4 + 1)[b:b + n]
    Ls = np.stack([gemv_logits(x[t], nw, bits, BF16) for t in range(steps)])
    return V, steps, cap, x, nw, bits, ctx, np.array(lens, np.int32), Ls


@pytest.mark.parametrize("case", CHAIN, ids=lambda c: "B%d-K%d-g%d" % c[:3])
def test_ngram_chain_and_bookkeeping(gpu, case):
    """8 consecutive steps, each reading the ban list the step before wrote: tokens, ban lists (as multisets),
    context, output, done (EOS and out_cap) and the KV counters equal a Python loop over select_token_id on the
    exact logits; the same through per-row records equals each row alone."""
    B, K, g, lens, eos, out_cap, finishes = case
    V, steps, cap, x, nw, bits, ctx, n0, Ls = _chain_inputs(case)
    ban0 = [_ban_list(ctx[b, :n0[b]].tolist(), g) for b in range(B)]
    if g == 2:
        assert max(lens) > SP_PM
    r = screen_steps(bits, BF16, x, nw, ctx=ctx, ctx_len=n0, ngram=g, eos=eos, ban=ban0, out_cap=out_cap, probe=3)
    finished = bans = 0
    for b in range(B):
        rec = _chain_reference(Ls[:, b], ctx[b, :n0[b]].tolist(), (g, eos), out_cap, cap)
        _chain_compare(r, b, rec, g)
        finished += rec[-1]["done"]
        bans += bool(ban0[b]) + sum(1 for e in rec if e["ban"])
    assert bans, "the ban never applied"
    assert bool(finished) == finishes, "the done branches: a page finishes in the cases marked so"
    # the probe step's lists against that step's exact logits and the ban list it read (the one step 2 wrote)
    banned = [r.ban_out[2, b, 1:1 + r.ban_out[2, b, 0]].tolist() for b in range(B)]
    check_invariants(r, Ls[3], bits, BF16, banned)


@pytest.mark.parametrize("B,K", [(2, 256), (3, 1280)])
def test_per_row_records_equal_each_row_alone(gpu, B, K):
    """The ROWS instantiations: every row with its own ngram / eos equals the Python loop with that row's
    parameters and the same row run alone with them as launch arguments."""
    case = (B, K, 0, [44, 290, 9][:B], -1, 6)
    V, steps, cap, x, nw, bits, ctx, n0, Ls = _chain_inputs(case)
    params = [(2, -1), (3, 15), (20, 599)][:B]
    ban0 = [_ban_list(ctx[b, :n0[b]].tolist(), params[b][0]) for b in range(B)]
    r = screen_steps(bits, BF16, x, nw, ctx=ctx, ctx_len=n0, rows=params, ban=ban0, out_cap=6)
    for b in range(B):
        rec = _chain_reference(Ls[:, b], ctx[b, :n0[b]].tolist(), params[b], 6, cap)
        _chain_compare(r, b, rec, params[b][0])
        one = screen_steps(bits, BF16, x[:, b:b + 1], nw, ctx=ctx[b:b + 1], ctx_len=n0[b:b + 1], ngram=params[b][0],
                           eos=params[b][1], ban=ban0[b:b + 1], out_cap=6)
        live = np.concatenate([[True], one.done[:-1, 0] == 0])
        assert np.array_equal(one.out_tok[live, 0], r.out_tok[live, b])
        for name in ("ctx_out", "ctx_len_out", "out_ids", "out_len", "done", "kv_pos", "kv_len"):
            assert np.array_equal(getattr(one, name)[:, 0], getattr(r, name)[:, b]), (b, name)


@pytest.mark.parametrize("table_dt", [BF16, F16])
@pytest.mark.parametrize("H", [256, 1280, 100])
def test_embedding_hand_off(gpu, table_dt, H):
    """x_next[b] is table row out_tok[b], bit for bit: row 0 has one dominant row (one survivor: the prefetch hits),
    row 1 the 64-row near-tie ensemble (more survivors than waves: the gather).  H = 100: no prefetch at all."""
    B, V, K = 2, SMALL_V, 256
    x, nw, xn, bits, pos = near_tie_case(B, V, K, BF16, case_seed(B, K, BF16))
    rng = np.random.default_rng(H + table_dt)
    bits[pos[0]] = round16((rng.standard_normal((len(pos[0]), K)) * 0.02).astype(np.float32), BF16)
    bits[pos[0][5]] = near_tie_rows(xn[0], BF16, rng, 1)[0]
    table = round16(rng.standard_normal((V, H)).astype(np.float32), table_dt)
    r = screen_steps(bits, BF16, x[None], nw, table=table, table_dt=table_dt)
    L = gemv_logits(x, nw, bits, BF16)
    survivors = []
    for b in range(B):
        assert r.out_tok[0, b] == first_argmax(L[b])
        T = r.blk_t[b].max()
        survivors.append(sum(int(np.count_nonzero(r.cand_hi[b, :r.blk_cnt[b, j], j] >= T)) for j in range(r.nblk)))
        assert np.array_equal(r.x_next[0, b].view(np.uint32), bits_to_f32(table[r.out_tok[0, b]], table_dt).view(np.uint32))
    assert survivors[0] == 1 and survivors[1] > 16, survivors
    assert r.out_tok[0, 0] == pos[0][5]
