"""The decoder prefill's RoPE + KV append + causal attention in the form the engine launches it
(Engine::layer_forward_prefill through dsocr_k_prefill_attention): a ragged batch packed row after row, q read
from the q|k|v buffer at per-sequence offsets, k / v read back from the paged cache, the grid sized by the
longest sequence and every sequence bounded by its own length; with the key-piece workspace (one block per
128-query block and 128-key piece + the piece combine, the workspace handed over full of NaN) and without it
(one block per query block), against f64 numpy math.

Bounds: rotated q and cached k within 1e-5 (test_decode_attention's bound for the same arithmetic), attention
rows within 2e-5 max-abs (test_attention's bound at the same input distribution and longer L), v bit-equal.
The cache enters full of NaN and o full of a sentinel, so a read past a sequence's length or a row nobody
wrote shows.  Worst errors measured on MI355X over the cases below, per head dim (q / k / o):
hd 32: 2.4e-7 / 2.4e-7 / 5.5e-7; hd 64: 4.8e-7 / 4.8e-7 / 8.7e-7; hd 128: 4.8e-7 / 4.8e-7 / 1.8e-6."""
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
RAGGED = (129, 300, 1, 128, 257)  # 1, exactly one block, one past a block, one past two; the longest not first

# lens, cap, heads, kv_heads, hd, rope_dim, use_mla
SHAPES = {
    "hd128": (RAGGED, 320, 2, 2, 128, 128, 0),            # production head dim
    "gqa64": (RAGGED, 320, 4, 2, 64, 64, 0),              # grouped-query form at hd 64
    "onekv": ((300, 127), 300, 4, 1, 128, 128, 0),        # all q heads on one kv head, cap == max_len
    "single": ((257,), 300, 2, 2, 128, 128, 0),           # one page: the uniform test's path through the cache layout
    "hd32": ((40, 130, 7), 160, 4, 4, 32, 32, 0),         # the tiny model's kernel with ragged offsets
    "mla": (RAGGED, 320, 2, 2, 128, 128, 1),              # even/odd regroup before the rotation
    "partial": (RAGGED, 320, 2, 2, 128, 64, 0),           # rotary on the first hd / 2 dims, tables [cap][rope_dim]
    "widest": ((3,), 4, 32, 32, 128, 128, 0),             # (heads + kv_heads) * hd == 8192: rope_kv's last accepted row
}
CASES = [(n, p) for n in ("hd128", "gqa64", "onekv", "single") for p in (1, 0)] + [
    ("hd32", 1), ("mla", 1), ("partial", 1), ("widest", 1)]


def _attn_ref(q, k, v, scale):
    s = (q @ k.T) * scale
    s = s + np.triu(np.full(s.shape, -1e9), 1)
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(-1, keepdims=True)
    return p @ v


def _rope_ref(x, cos, sin, rope_dim, use_mla):
    """x [len][n][hd] f64, cos / sin [len][rope_dim].  Whole-head rotary: the oracle's apply_rope.  Partial:
    out[:rope_dim] = x[:rope_dim] * cos + rotate_half(x[:rope_dim]) * sin, the rest passes through."""
    hd = x.shape[-1]
    cs, sn = cos[:, None, :], sin[:, None, :]
    if rope_dim == hd:
        return apply_rope(x, cs, sn, bool(use_mla)).astype(np.float64)
    assert not use_mla
    head, half = x[..., :rope_dim], rope_dim // 2
    rot = np.concatenate([-head[..., half:], head[..., :half]], -1)
    return np.concatenate([head * cs + rot * sn, x[..., rope_dim:]], -1)


@functools.lru_cache(maxsize=None)
def _reference(name, seed):
    """Inputs and the f64 reference of one shape, computed once and shared read-only."""
    lens, cap, heads, kvh, hd, rope_dim, use_mla = SHAPES[name]
    rng = np.random.default_rng(seed)
    T, H, KVH = sum(lens), heads * hd, kvh * hd
    qkv = rng.standard_normal((T, H + 2 * KVH)).astype(np.float32)
    cos, sin = rope_tables(SimpleNamespace(rope_theta=10000.0), cap, rope_dim)
    scale = 1.0 / math.sqrt(hd)
    q_ref = np.empty((T, heads, hd))
    k_ref, o_ref = [], np.empty((T, heads, hd))
    r0 = 0
    for n in lens:
        rows = slice(r0, r0 + n)
        x = qkv[rows].astype(np.float64)
        q = _rope_ref(x[:, :H].reshape(n, heads, hd), cos[:n], sin[:n], rope_dim, use_mla)
        k = _rope_ref(x[:, H:H + KVH].reshape(n, kvh, hd), cos[:n], sin[:n], rope_dim, use_mla)
        v = x[:, H + KVH:].reshape(n, kvh, hd)
        for h in range(heads):
            g = h // (heads // kvh)
            o_ref[rows, h] = _attn_ref(q[:, h], k[:, g], v[:, g], scale)
        q_ref[rows] = q
        k_ref.append(k.transpose(1, 0, 2))  # [kvh][n][hd], the cache's layout
        r0 += n
    out = SimpleNamespace(qkv=qkv, cos=cos, sin=sin, scale=scale, q_ref=q_ref.reshape(T, H), k_ref=k_ref,
                          o_ref=o_ref.reshape(T, H))
    for a in (qkv, cos, sin, out.q_ref, out.o_ref, *k_ref):
        a.setflags(write=False)
    return out


def _nan_cache(B, kvh, cap, hd):
    return Dev(np.full((B, kvh, cap, hd), np.nan, np.float32))


def _launch(name, ref, dk, dv, use_part):
    lens, cap, heads, kvh, hd, rope_dim, use_mla = SHAPES[name]
    T = sum(lens)
    dqkv, dcos, dsin = Dev(ref.qkv), Dev(ref.cos), Dev(ref.sin)
    do = Dev(np.full((T, heads * hd), SENT, np.uint32))
    hl = (C.c_int * len(lens))(*lens)
    check(lib().dsocr_k_prefill_attention(len(lens), heads, kvh, hd, rope_dim, use_mla, cap, ref.scale, hl, dqkv.ptr,
                                          dcos.ptr, dsin.ptr, dk.ptr, dv.ptr, do.ptr, use_part))
    return dqkv.get(), dk.get(), dv.get(), do.get()


def _verify(name, ref, got_qkv, gk, gv, go_bits, tag):
    lens, cap, heads, kvh, hd, rope_dim, use_mla = SHAPES[name]
    H, KVH = heads * hd, kvh * hd
    go = go_bits.view(np.float32)
    eq = np.max(np.abs(got_qkv[:, :H] - ref.q_ref))
    eo = np.max(np.abs(go - ref.o_ref))
    ek = max(np.max(np.abs(gk[b, :, :n] - ref.k_ref[b])) for b, n in enumerate(lens))
    print(f"prefill_attention {tag}: hd {hd} max|dq| {eq:.3e} max|dk| {ek:.3e} max|do| {eo:.3e}")
    assert eq < 1e-5, eq
    assert ek < 1e-5, ek
    r0 = 0
    for b, n in enumerate(lens):
        v = ref.qkv[r0:r0 + n, H + KVH:].reshape(n, kvh, hd).transpose(1, 0, 2)
        assert np.array_equal(gv[b, :, :n].view(np.uint32), v.view(np.uint32)), b
        assert np.isnan(gk[b, :, n:]).all() and np.isnan(gv[b, :, n:]).all(), b  # the append writes nothing else
        r0 += n
    assert np.array_equal(got_qkv[:, H + KVH:].view(np.uint32), ref.qkv[:, H + KVH:].view(np.uint32))
    assert not np.any(go_bits == SENT), "part of o was never written"
    err = np.max(np.abs(go - ref.o_ref), axis=1)  # NaN (a read past a sequence, an unwritten record) fails too
    assert np.all(err < 2e-5), (int(np.argmax(~(err < 2e-5))), eo)


@pytest.mark.parametrize("name,use_part", CASES, ids=[f"{n}-part{p}" for n, p in CASES])
def test_prefill_attention(gpu, name, use_part):
    lens, cap, heads, kvh, hd, rope_dim, use_mla = SHAPES[name]
    ref = _reference(name, 1)
    dk, dv = _nan_cache(len(lens), kvh, cap, hd), _nan_cache(len(lens), kvh, cap, hd)
    _verify(name, ref, *_launch(name, ref, dk, dv, use_part), f"{name}-part{use_part}")


def test_prefill_attention_back_to_back(gpu):
    """Two prefills on the same cache, fresh q|k|v the second time: no stale cache row and no leftover piece
    record may reach the second result."""
    name = "hd128"
    lens, cap, heads, kvh, hd, rope_dim, use_mla = SHAPES[name]
    dk, dv = _nan_cache(len(lens), kvh, cap, hd), _nan_cache(len(lens), kvh, cap, hd)
    first, second = _reference(name, 1), _reference(name, 2)
    _verify(name, first, *_launch(name, first, dk, dv, 1), "back-to-back-1")
    _verify(name, second, *_launch(name, second, dk, dv, 1), "back-to-back-2")


def test_rope_kv_refuses_wide_rows(gpu):
    """(heads + kv_heads) * hd > 8192 is past what rope_kv keeps per thread: EINVAL before any launch."""
    heads = kvh = 33
    hd, cap = 128, 4
    assert (heads + kvh) * hd > 8192
    qkv = np.ones((1, (heads + 2 * kvh) * hd), np.float32)
    cos, sin = rope_tables(SimpleNamespace(rope_theta=10000.0), cap, hd)
    dqkv, dcos, dsin = Dev(qkv), Dev(cos), Dev(sin)
    dk, dv = _nan_cache(1, kvh, cap, hd), _nan_cache(1, kvh, cap, hd)
    do = Dev(np.full((1, heads * hd), SENT, np.uint32))
    st = lib().dsocr_k_prefill_attention(1, heads, kvh, hd, hd, 0, cap, 1.0, (C.c_int * 1)(1), dqkv.ptr, dcos.ptr,
                                         dsin.ptr, dk.ptr, dv.ptr, do.ptr, 1)
    assert st == EINVAL
    assert b"8192" in lib().dsocr_last_error()
    assert np.array_equal(dqkv.get(), qkv) and np.isnan(dk.get()).all() and np.all(do.get() == SENT)
