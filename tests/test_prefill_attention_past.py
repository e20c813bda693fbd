"""The decoder prefill behind a cached past (a prompt suffix admitted through a page prefix entry): RoPE at the
shifted positions + KV append + launch_attention_past, in the form the engine launches them
(Engine::layer_forward_prefill with `past`, through dsocr_k_prefill_attention_past).  Every sequence brings n new
rows behind `past` cached ones; new row i sits at position past + i and sees keys [0, past + i].

Reference: f64 numpy over the full past + n rows of every sequence (the rows [past, past + n) of its causal
attention).  The cache enters holding rows [0, past) of the reference's rotated K (rounded to f32) and V, NaN
everywhere else; o enters full of a NaN sentinel and the piece workspace full of NaN, so a read past a sequence's
keys, a row nobody wrote and a record the combine should not have read all show.

Bounds are test_prefill_attention's own (same arithmetic, same input distribution): rotated q and appended k within
1e-5, o within 2e-5 max-abs, appended v bit-equal, nothing written outside [past, past + n), rows [0, past) of the
cache bit-unchanged.  Worst errors measured on MI355X over the cases below, per head dim (q / k / o):
hd 32: 2.4e-7 / 4.8e-7 / 3.4e-7; hd 64: 4.8e-7 / 2.4e-7 / 3.7e-7; hd 128: 4.8e-7 / 2.4e-7 / 8.3e-7; the no-past
sequence equals the causal prefill bit for bit (max|do| 0)."""
import ctypes as C
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest

from _dev import Dev
from dsocr._lib import EINVAL, check, lib
from oracle.decoder import apply_rope, rope_tables

pytestmark = pytest.mark.gpu

SENT = 0x7FBADBAD  # a NaN pattern no kernel produces
# (past, n) per sequence, the longest not first: new rows across a 128-key piece boundary; ending exactly at cap; one
# row behind one row; two query tiles, the second with one row; no past at all
RAGGED = ((127, 2), (300, 20), (1, 1), (128, 33), (0, 5))

# (past, n) per sequence, cap, heads, kv_heads, hd, rope_dim, use_mla
SHAPES = {
    "hd128": (RAGGED, 320, 2, 2, 128, 128, 0),                        # production head dim
    "gqa64": (RAGGED, 320, 4, 2, 64, 64, 0),                          # grouped-query form at hd 64
    "onekv": (((299, 1), (127, 40)), 300, 4, 1, 128, 128, 0),         # all q heads on one kv head, cap == past + n
    "hd32": (((40, 3), (129, 31), (0, 7), (95, 34)), 160, 4, 4, 32, 32, 0),  # the tiny model's head dim
    "mla": (RAGGED, 320, 2, 2, 128, 128, 1),                          # even/odd regroup before the rotation
    "partial": (RAGGED, 320, 2, 2, 128, 64, 0),                       # rotary on the first hd / 2 dims
}


def _attn_ref(q, k, v, scale):
    s = (q @ k.T) * scale
    s = s + np.triu(np.full(s.shape, -1e9), 1)
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(-1, keepdims=True)
    return p @ v


def _rope_ref(x, cos, sin, rope_dim, use_mla):
    """x [len][n][hd] f64, cos / sin [len][rope_dim]: whole-head rotary is the oracle's apply_rope; partial rotary
    rotates the first rope_dim dims and passes the rest through."""
    hd = x.shape[-1]
    cs, sn = cos[:, None, :], sin[:, None, :]
    if rope_dim == hd:
        return apply_rope(x, cs, sn, bool(use_mla)).astype(np.float64)
    assert not use_mla
    head, half = x[..., :rope_dim], rope_dim // 2
    rot = np.concatenate([-head[..., half:], head[..., :half]], -1)
    return np.concatenate([head * cs + rot * sn, x[..., rope_dim:]], -1)


@functools.lru_cache(maxsize=None)
def _reference(name, seed=1):
    """Inputs and the f64 reference of one shape, computed once and shared read-only."""
    seqs, cap, heads, kvh, hd, rope_dim, use_mla = SHAPES[name]
    rng = np.random.default_rng(seed)
    H, KVH = heads * hd, kvh * hd
    cos, sin = rope_tables(SimpleNamespace(rope_theta=10000.0), cap, rope_dim)
    scale = 1.0 / math.sqrt(hd)
    B = len(seqs)
    k0 = np.full((B, kvh, cap, hd), np.nan, np.float32)   # the cache on entry
    v0 = np.full((B, kvh, cap, hd), np.nan, np.float32)
    qkv_new, q_ref, k_ref, v_new, o_ref = [], [], [], [], []
    for b, (past, n) in enumerate(seqs):
        tot = past + n
        full = rng.standard_normal((tot, H + 2 * KVH)).astype(np.float32)
        x = full.astype(np.float64)
        q = _rope_ref(x[:, :H].reshape(tot, heads, hd), cos[:tot], sin[:tot], rope_dim, use_mla)
        k = _rope_ref(x[:, H:H + KVH].reshape(tot, kvh, hd), cos[:tot], sin[:tot], rope_dim, use_mla)
        v = x[:, H + KVH:].reshape(tot, kvh, hd)
        o = np.empty((tot, heads, hd))
        for h in range(heads):
            g = h // (heads // kvh)
            o[:, h] = _attn_ref(q[:, h], k[:, g], v[:, g], scale)
        k0[b, :, :past] = k[:past].transpose(1, 0, 2).astype(np.float32)
        v0[b, :, :past] = full[:past, H + KVH:].reshape(past, kvh, hd).transpose(1, 0, 2)
        qkv_new.append(full[past:])
        q_ref.append(q[past:].reshape(n, H))
        k_ref.append(k[past:].transpose(1, 0, 2))          # [kvh][n][hd], the cache's layout
        v_new.append(full[past:, H + KVH:].reshape(n, kvh, hd).transpose(1, 0, 2))
        o_ref.append(o[past:].reshape(n, H))
    out = SimpleNamespace(qkv=np.concatenate(qkv_new), cos=cos, sin=sin, scale=scale, k0=k0, v0=v0,
                          q_ref=np.concatenate(q_ref), k_ref=k_ref, v_new=v_new, o_ref=np.concatenate(o_ref))
    for a in (out.qkv, cos, sin, k0, v0, out.q_ref, out.o_ref, *k_ref, *v_new):
        a.setflags(write=False)
    return out


def _launch(name, ref):
    seqs, cap, heads, kvh, hd, rope_dim, use_mla = SHAPES[name]
    T = sum(n for _, n in seqs)
    dqkv, dcos, dsin = Dev(ref.qkv), Dev(ref.cos), Dev(ref.sin)
    dk, dv = Dev(ref.k0), Dev(ref.v0)
    do = Dev(np.full((T, heads * hd), SENT, np.uint32))
    hp = (C.c_int * len(seqs))(*[p for p, _ in seqs])
    hl = (C.c_int * len(seqs))(*[n for _, n in seqs])
    check(lib().dsocr_k_prefill_attention_past(len(seqs), heads, kvh, hd, rope_dim, use_mla, cap, ref.scale, hp, hl,
                                               dqkv.ptr, dcos.ptr, dsin.ptr, dk.ptr, dv.ptr, do.ptr))
    return dqkv.get(), dk.get(), dv.get(), do.get()


def _verify(name, ref, got_qkv, gk, gv, go_bits):
    seqs, cap, heads, kvh, hd, rope_dim, use_mla = SHAPES[name]
    H, KVH = heads * hd, kvh * hd
    go = go_bits.view(np.float32)
    eq = np.max(np.abs(got_qkv[:, :H] - ref.q_ref))
    eo = np.max(np.abs(go - ref.o_ref))
    ek = max(np.max(np.abs(gk[b, :, p:p + n] - ref.k_ref[b])) for b, (p, n) in enumerate(seqs))
    print(f"prefill_attention_past {name}: hd {hd} max|dq| {eq:.3e} max|dk| {ek:.3e} max|do| {eo:.3e}")
    assert eq < 1e-5, eq
    assert ek < 1e-5, ek
    for b, (p, n) in enumerate(seqs):
        assert np.array_equal(gv[b, :, p:p + n].view(np.uint32), ref.v_new[b].view(np.uint32)), b
        # the append writes rows [past, past + n) only: the past is bit-unchanged, the rest is still NaN
        assert np.array_equal(gk[b, :, :p].view(np.uint32), ref.k0[b, :, :p].view(np.uint32)), b
        assert np.array_equal(gv[b, :, :p].view(np.uint32), ref.v0[b, :, :p].view(np.uint32)), b
        assert np.isnan(gk[b, :, p + n:]).all() and np.isnan(gv[b, :, p + n:]).all(), b
    assert np.array_equal(got_qkv[:, H + KVH:].view(np.uint32), ref.qkv[:, H + KVH:].view(np.uint32))
    assert not np.any(go_bits == SENT), "part of o was never written"
    err = np.max(np.abs(go - ref.o_ref), axis=1)  # NaN (a read past a sequence, an unwritten record) fails too
    assert np.all(err < 2e-5), (int(np.argmax(~(err < 2e-5))), eo)


@pytest.mark.parametrize("name", list(SHAPES))
def test_prefill_attention_past(gpu, name):
    ref = _reference(name)
    _verify(name, ref, *_launch(name, ref))


def test_no_past_agrees_with_the_causal_prefill(gpu):
    """The (0, 5) sequence of the ragged case has no past: launch_attention_past on it must also agree with the
    causal prefill (dsocr_k_prefill_attention, with and without the key-piece workspace) on the same rows."""
    name = "hd128"
    seqs, cap, heads, kvh, hd, rope_dim, use_mla = SHAPES[name]
    ref = _reference(name)
    b = [i for i, (p, _) in enumerate(seqs) if p == 0][0]
    r0 = sum(n for _, n in seqs[:b])
    n = seqs[b][1]
    rows = ref.qkv[r0:r0 + n]
    go = _launch(name, ref)[3].view(np.float32)[r0:r0 + n]
    for use_part in (1, 0):
        dqkv, dcos, dsin = Dev(rows), Dev(ref.cos), Dev(ref.sin)
        dk = Dev(np.full((1, kvh, cap, hd), np.nan, np.float32))
        dv = Dev(np.full((1, kvh, cap, hd), np.nan, np.float32))
        do = Dev(np.full((n, heads * hd), SENT, np.uint32))
        check(lib().dsocr_k_prefill_attention(1, heads, kvh, hd, rope_dim, use_mla, cap, ref.scale, (C.c_int * 1)(n),
                                              dqkv.ptr, dcos.ptr, dsin.ptr, dk.ptr, dv.ptr, do.ptr, use_part))
        want = do.get().view(np.float32)
        d = np.max(np.abs(go - want))
        print(f"prefill_attention_past vs causal prefill (part {use_part}): max|do| {d:.3e}")
        assert d < 2e-5, d


def test_refuses_head_dim_48(gpu):
    """hd 48 is outside the contract: EINVAL before any launch (nothing is rotated, appended or written)."""
    heads = kvh = 2
    hd, cap = 48, 8
    qkv = np.ones((2, (heads + 2 * kvh) * hd), np.float32)
    cos, sin = rope_tables(SimpleNamespace(rope_theta=10000.0), cap, hd)
    dqkv, dcos, dsin = Dev(qkv), Dev(cos), Dev(sin)
    k0 = np.full((1, kvh, cap, hd), np.nan, np.float32)
    k0[:, :, :3] = 1.0
    dk, dv = Dev(k0), Dev(k0)
    do = Dev(np.full((2, heads * hd), SENT, np.uint32))
    st = lib().dsocr_k_prefill_attention_past(1, heads, kvh, hd, hd, 0, cap, 1.0, (C.c_int * 1)(3), (C.c_int * 1)(2),
                                              dqkv.ptr, dcos.ptr, dsin.ptr, dk.ptr, dv.ptr, do.ptr)
    assert st == EINVAL
    assert np.array_equal(dqkv.get(), qkv) and np.all(do.get() == SENT)
    assert np.array_equal(dk.get().view(np.uint32), k0.view(np.uint32))
    # past + new rows beyond cap is refused the same way
    st = lib().dsocr_k_prefill_attention_past(1, heads, kvh, 64, 64, 0, cap, 1.0, (C.c_int * 1)(7), (C.c_int * 1)(2),
                                              dqkv.ptr, dcos.ptr, dsin.ptr, dk.ptr, dv.ptr, do.ptr)
    assert st == EINVAL and np.array_equal(dqkv.get(), qkv)
