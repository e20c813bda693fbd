"""launch_attention_chunk (attention_past.hip) through dsocr_k_attention_chunk: the attention of a prefill chunk
behind a cached past, tiled over the queries, in the form Engine::layer_forward_prefill launches it for a sliced
admission (RoPE at the shifted positions + KV append + attention into pages [page0, page0 + B) of a session cache).

Reference: float64 numpy softmax attention on the f32 inputs the kernel itself reads: the rotated q rows and the K
cache are read back from the device after the launch (launch_rope_kv is the same launch in both hooks, so both
kernels see bit-equal q and K), V is the input's.

Cases: every (past, n_q) of {0, 1, 31, 33, 130} x {1, 31, 32, 33, 70} as one ragged call of 25 sequences, for every
hd in {32, 64, 128} and (heads, kv_heads) in {(4, 4), (4, 2)}; a call of two ragged sequences; a cache with
kv_page0 > 0 and a slot stride above the rows used.  Every cache row at or behind past + n_q is NaN on entry, every
output word a NaN sentinel: a read past a sequence's keys and an unwritten row both show.

Bar, per (past, n_q) case: the worst |o - f64| of attention_chunk is at most twice that of attention_past
(dsocr_k_prefill_attention_past) on the same inputs: both sum the same f32 terms in another order.  past == 0 is held
to the same bar against the causal prefill (dsocr_k_prefill_attention) too."""
import ctypes as C
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest

from _dev import Dev
from dsocr._lib import EINVAL, check, lib
from oracle.decoder import rope_tables

pytestmark = pytest.mark.gpu

SENT = 0x7FBADBAD  # a NaN pattern no kernel produces
PASTS = (0, 1, 31, 33, 130)
NQS = (1, 31, 32, 33, 70)
GRID = tuple((p, n) for p in PASTS for n in NQS)
CAP = 208  # >= 130 + 70, not a multiple of 32


@functools.lru_cache(maxsize=None)
def _inputs(hd, heads, kvh, seqs, cap, pages, page0, seed=3):
    """qkv rows of the new rows, the caches on entry (past rows of random K / V, NaN elsewhere), shared read-only."""
    rng = np.random.default_rng(seed)
    H, KVH = heads * hd, kvh * hd
    cos, sin = rope_tables(SimpleNamespace(rope_theta=10000.0), cap, hd)
    k0 = np.full((pages, kvh, cap, hd), np.nan, np.float32)
    v0 = np.full((pages, kvh, cap, hd), np.nan, np.float32)
    for b, (past, _) in enumerate(seqs):
        k0[page0 + b, :, :past] = rng.standard_normal((kvh, past, hd)).astype(np.float32)
        v0[page0 + b, :, :past] = rng.standard_normal((kvh, past, hd)).astype(np.float32)
    qkv = rng.standard_normal((sum(n for _, n in seqs), H + 2 * KVH)).astype(np.float32)
    for a in (qkv, cos, sin, k0, v0):
        a.setflags(write=False)
    return SimpleNamespace(qkv=qkv, cos=cos, sin=sin, k0=k0, v0=v0, scale=1.0 / math.sqrt(hd))


def _run(kind, inp, hd, heads, kvh, seqs, cap, pages, page0):
    """kind: "chunk" | "past" | "causal".  Returns (rotated qkv, K cache, V cache, o) read back from the device."""
    B, T = len(seqs), sum(n for _, n in seqs)
    dqkv, dcos, dsin = Dev(inp.qkv), Dev(inp.cos), Dev(inp.sin)
    dk, dv = Dev(inp.k0), Dev(inp.v0)
    do = Dev(np.full((T, heads * hd), SENT, np.uint32))
    hp = (C.c_int * B)(*[p for p, _ in seqs])
    hl = (C.c_int * B)(*[n for _, n in seqs])
    off = page0 * kvh * cap * hd * 4  # the older hooks take the first sequence's page
    kp, vp = C.c_void_p(dk.ptr.value + off), C.c_void_p(dv.ptr.value + off)
    L = lib()
    if kind == "chunk":
        check(L.dsocr_k_attention_chunk(B, heads, kvh, hd, hd, 0, cap, inp.scale, hp, hl, dqkv.ptr, dcos.ptr, dsin.ptr,
                                        dk.ptr, dv.ptr, do.ptr, page0, pages))
    elif kind == "past":
        check(L.dsocr_k_prefill_attention_past(B, heads, kvh, hd, hd, 0, cap, inp.scale, hp, hl, dqkv.ptr, dcos.ptr,
                                               dsin.ptr, kp, vp, do.ptr))
    else:
        assert all(p == 0 for p, _ in seqs)
        check(L.dsocr_k_prefill_attention(B, heads, kvh, hd, hd, 0, cap, inp.scale, hl, dqkv.ptr, dcos.ptr, dsin.ptr,
                                          kp, vp, do.ptr, 1))
    return dqkv.get(), dk.get(), dv.get(), do.get()


def _errors(hd, heads, kvh, seqs, page0, got_qkv, gk, gv, go_bits):
    """Worst |o - f64| per sequence, the f64 attention computed on the f32 q / K / V the kernel read."""
    H = heads * hd
    assert not np.any(go_bits == SENT), "part of o was never written"
    go = go_bits.view(np.float32).astype(np.float64)
    errs, r0 = [], 0
    for b, (past, n) in enumerate(seqs):
        tot = past + n
        q = got_qkv[r0:r0 + n, :H].reshape(n, heads, hd).astype(np.float64)
        worst = 0.0
        for h in range(heads):
            g = h // (heads // kvh)
            k = gk[page0 + b, g, :tot].astype(np.float64)
            v = gv[page0 + b, g, :tot].astype(np.float64)
            assert np.isfinite(k).all() and np.isfinite(v).all()
            s = (q[:, h] @ k.T) / math.sqrt(hd)
            s[np.arange(tot)[None, :] > (past + np.arange(n))[:, None]] = -np.inf
            p = np.exp(s - s.max(-1, keepdims=True))
            ref = (p / p.sum(-1, keepdims=True)) @ v
            d = np.abs(go[r0:r0 + n, h * hd:(h + 1) * hd] - ref)
            assert np.isfinite(d).all(), (b, h)  # a NaN: a read past the sequence's rows
            worst = max(worst, float(d.max()))
        errs.append(worst)
        r0 += n
    return errs


def _untouched(inp, seqs, page0, gk, gv):
    """Rows [0, past) bit-unchanged, rows from past + n on and every other page still NaN."""
    used = set()
    for b, (past, n) in enumerate(seqs):
        pg = page0 + b
        used.add(pg)
        assert np.array_equal(gk[pg, :, :past].view(np.uint32), inp.k0[pg, :, :past].view(np.uint32)), b
        assert np.array_equal(gv[pg, :, :past].view(np.uint32), inp.v0[pg, :, :past].view(np.uint32)), b
        assert np.isnan(gk[pg, :, past + n:]).all() and np.isnan(gv[pg, :, past + n:]).all(), b
    for pg in range(gk.shape[0]):
        if pg not in used:
            assert np.isnan(gk[pg]).all() and np.isnan(gv[pg]).all(), pg


def _compare(hd, heads, kvh, seqs, cap, pages=None, page0=0, causal=False):
    pages = len(seqs) + page0 if pages is None else pages
    inp = _inputs(hd, heads, kvh, seqs, cap, pages, page0)
    args = (hd, heads, kvh, seqs, cap, pages, page0)
    c = _run("chunk", inp, *args)
    p = _run("past", inp, *args)
    # the same rotation and append in both hooks: both kernels read bit-equal q and K
    assert np.array_equal(c[0].view(np.uint32), p[0].view(np.uint32))
    assert np.array_equal(c[1].view(np.uint32), p[1].view(np.uint32), ) and np.array_equal(c[2].view(np.uint32), p[2].view(np.uint32))
    _untouched(inp, seqs, page0, c[1], c[2])
    ec = _errors(hd, heads, kvh, seqs, page0, *c)
    ep = _errors(hd, heads, kvh, seqs, page0, *p)
    for (past, n), a, b in zip(seqs, ec, ep):
        print(f"attention_chunk hd {hd} heads {heads}/{kvh} past {past} n_q {n}: chunk {a:.3e} past-kernel {b:.3e}")
    print(f"attention_chunk hd {hd} heads {heads}/{kvh}: worst chunk {max(ec):.3e}, worst past-kernel {max(ep):.3e}")
    if causal:
        z = tuple(s for s in seqs if s[0] == 0)
        zi = _inputs(hd, heads, kvh, z, cap, len(z), 0)
        za = (hd, heads, kvh, z, cap, len(z), 0)
        cz, pz = _run("chunk", zi, *za), _run("causal", zi, *za)
        assert np.array_equal(cz[0].view(np.uint32), pz[0].view(np.uint32))
        ecz, epz = _errors(hd, heads, kvh, z, 0, *cz), _errors(hd, heads, kvh, z, 0, *pz)
        dd = float(np.max(np.abs(cz[3].view(np.float32) - pz[3].view(np.float32))))
        print(f"attention_chunk hd {hd} heads {heads}/{kvh} past 0 vs causal prefill: chunk {max(ecz):.3e} "
              f"causal {max(epz):.3e} max|do| {dd:.3e}")
        for (past, n), a, b in zip(z, ecz, epz):
            assert a <= 2 * b, ("causal", past, n, a, b)
    for (past, n), a, b in zip(seqs, ec, ep):
        assert a <= 2 * b, (past, n, a, b)


@pytest.mark.parametrize("heads,kvh", [(4, 4), (4, 2)])
@pytest.mark.parametrize("hd", [32, 64, 128])
def test_every_past_and_row_count(gpu, hd, heads, kvh):
    _compare(hd, heads, kvh, GRID, CAP, causal=True)


def test_two_ragged_sequences(gpu):
    _compare(128, 4, 2, ((130, 33), (31, 70)), CAP)


def test_more_key_tiles_than_waves(gpu):
    """Up to 200 keys every wave of the workgroup owns at most one 32-key tile; behind 300 and 610 rows a wave visits
    two and three, so its running (m, l, O) is rescaled between tiles (the sizes of a chunk behind a page's rows)."""
    _compare(128, 4, 2, ((300, 33), (610, 70), (255, 2)), 700)
    _compare(32, 4, 4, ((257, 31), (610, 70)), 700)


def test_page0_and_a_slot_stride_above_the_rows(gpu):
    """Pages [2, 4) of a five-page cache with 300 rows per head: the other pages and every row from past + n_q on are
    NaN on entry and on exit, and no output is NaN."""
    _compare(64, 4, 2, ((33, 70), (130, 31)), 300, pages=5, page0=2)


def test_refuses_shapes_outside_the_contract(gpu):
    """EINVAL before any launch: nothing is rotated, appended or written."""
    heads = kvh = 2
    cap = 8
    L = lib()

    def call(heads, kvh, hd, past, n, page0=0, pages=1):
        qkv = np.ones((2, (heads + 2 * kvh) * hd), np.float32)
        cos, sin = rope_tables(SimpleNamespace(rope_theta=10000.0), cap, hd)
        k0 = np.full((1, kvh, cap, hd), np.nan, np.float32)
        k0[:, :, :3] = 1.0
        dqkv, dcos, dsin, dk, dv = Dev(qkv), Dev(cos), Dev(sin), Dev(k0), Dev(k0)
        do = Dev(np.full((2, heads * hd), SENT, np.uint32))
        st = L.dsocr_k_attention_chunk(1, heads, kvh, hd, hd, 0, cap, 1.0, (C.c_int * 1)(past), (C.c_int * 1)(n),
                                       dqkv.ptr, dcos.ptr, dsin.ptr, dk.ptr, dv.ptr, do.ptr, page0, pages)
        assert np.array_equal(dqkv.get(), qkv) and np.all(do.get() == SENT)
        assert np.array_equal(dk.get().view(np.uint32), k0.view(np.uint32))
        return st

    assert call(heads, kvh, 48, 3, 2) == EINVAL      # head dim outside {32, 64, 128}
    assert call(heads, kvh, 16, 3, 2) == EINVAL
    assert call(3, 2, 64, 3, 2) == EINVAL            # heads % kv_heads
    assert call(heads, kvh, 64, 3, 0) == EINVAL      # no new row
    assert call(heads, kvh, 64, -1, 2) == EINVAL     # a negative past
    assert call(heads, kvh, 64, 7, 2) == EINVAL      # past + new rows beyond cap
    assert call(heads, kvh, 64, 3, 2, page0=1) == EINVAL  # the page outside the cache
