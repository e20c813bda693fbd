"""Bit-for-bit A/B of the f32 MFMA attention kernels across two builds: fixed-seed inputs through the
C hooks of attention_fwd2 (+ merge), attention_prefix, attention_past (+ merge) and attention_chunk at the shapes the
tests use, every output array written to an .npz.

    python tools/attention_ab.py --out a.npz                  # in a checkout of the older commit, built there
    python tools/attention_ab.py --out b.npz --against a.npz  # in this tree: exits 1 on any differing byte

_lib.py loads the library beside itself, so each checkout measures its own build.  Run each in a fresh process.
DSOCR_ATTN_SPLIT=0 in the environment sends the SAM / CLIP shapes of dsocr_k_attention to attention_fwd2 (they run the
bf16-plane kernel otherwise); the causal shapes reach attention_fwd2 either way.
"""
import argparse
import ctypes as C
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "deepseek-ocr.rs_amd")]

# tests/test_gpu_kernels.py: n_seq, L, heads, hd, causal
ATTENTION = [(2, 257, 16, 64, 0), (3, 101, 4, 32, 0), (1, 706, 10, 128, 1), (5, 196, 12, 64, 0), (2, 33, 2, 128, 1),
             (3, 300, 4, 64, 1), (1, 1217, 10, 128, 1), (2, 20, 4, 64, 0), (1, 97, 3, 64, 0)]
SAM_GRIDS = (14, 16, 40, 64)  # rel-pos bias, 2 heads of 64
# tests/test_prefill_attention.py: lens, cap, heads, kv_heads, hd, rope_dim, use_mla
RAGGED0 = (129, 300, 1, 128, 257)
PREFILL = {
    "hd128": (RAGGED0, 320, 2, 2, 128, 128, 0), "gqa64": (RAGGED0, 320, 4, 2, 64, 64, 0),
    "onekv": ((300, 127), 300, 4, 1, 128, 128, 0), "single": ((257,), 300, 2, 2, 128, 128, 0),
    "hd32": ((40, 130, 7), 160, 4, 4, 32, 32, 0), "mla": (RAGGED0, 320, 2, 2, 128, 128, 1),
    "partial": (RAGGED0, 320, 2, 2, 128, 64, 0), "widest": ((3,), 4, 32, 32, 128, 128, 0)}
PREFILL_NO_PART = ("hd128", "gqa64", "onekv", "single")
# tests/test_prefill_attention_past.py: (past, n) per sequence, cap, heads, kv_heads, hd, rope_dim, use_mla
RAGGED = ((127, 2), (300, 20), (1, 1), (128, 33), (0, 5))
GRID = tuple((p, n) for p in (0, 1, 31, 33, 130) for n in (1, 31, 32, 33, 70))  # tests/test_attention_chunk.py
PAST = {
    "hd128": (RAGGED, 320, 2, 2, 128, 128, 0), "gqa64": (RAGGED, 320, 4, 2, 64, 64, 0),
    "onekv": (((299, 1), (127, 40)), 300, 4, 1, 128, 128, 0),
    "hd32": (((40, 3), (129, 31), (0, 7), (95, 34)), 160, 4, 4, 32, 32, 0), "mla": (RAGGED, 320, 2, 2, 128, 128, 1),
    "partial": (RAGGED, 320, 2, 2, 128, 64, 0),
    "grid32": (GRID, 208, 4, 2, 32, 32, 0), "grid64": (GRID, 208, 4, 2, 64, 64, 0), "grid128": (GRID, 208, 4, 4, 128, 128, 0),
    "past610": (((610, 6), (610, 70)), 700, 2, 2, 128, 128, 0)}  # more than 8 key tiles per wave of attention_chunk
# tests/test_ocr2_gpu.py: n_seq, prefix, L, heads, kv_heads, hd
PREFIX = [(1, 144, 288, 14, 2, 64), (2, 256, 512, 14, 2, 64), (3, 5, 37, 4, 2, 32), (1, 31, 64, 4, 2, 64),
          (1, 32, 64, 4, 2, 64), (1, 33, 64, 4, 2, 64), (1, 0, 33, 2, 1, 64), (1, 40, 40, 7, 1, 64), (2, 33, 34, 4, 4, 64)]
SENT = 0x7FBADBAD


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--against")
    a = ap.parse_args()
    from dsocr._lib import check, lib
    L = lib()
    live = []

    def dev(x):
        x = np.ascontiguousarray(x)
        p = C.c_void_p()
        check(L.dsocr_dev_alloc(max(x.nbytes, 16), C.byref(p)))
        check(L.dsocr_memcpy_h2d(p, x.ctypes.data_as(C.c_void_p), x.nbytes))
        live.append(p)
        return p

    def get(p, shape, dtype=np.uint32):
        out = np.empty(shape, dtype)
        check(L.dsocr_memcpy_d2h(out.ctypes.data_as(C.c_void_p), p, out.nbytes))
        return out

    def free_all():
        for p in live:
            L.dsocr_dev_free(p)
        live.clear()

    out = {}
    rng = np.random.default_rng(20240)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
    for n_seq, Ls, heads, hd, causal in ATTENTION:
        q, k, v = (f32(n_seq * Ls, heads * hd) for _ in range(3))
        do = dev(np.full((n_seq * Ls, heads * hd), SENT, np.uint32))
        check(L.dsocr_k_attention(n_seq, Ls, heads, hd, 1.0 / math.sqrt(hd), causal, dev(q), dev(k), dev(v), do, None,
                                  None, 0, 0))
        out[f"attention/{n_seq}x{Ls}x{heads}x{hd}c{causal}"] = get(do, (n_seq * Ls, heads * hd))
        free_all()
    for g in SAM_GRIDS:
        Ls, heads, hd = g * g, 2, 64
        q, k, v = (f32(Ls, heads * hd) for _ in range(3))
        th, tw = f32(2 * g - 1, hd) * 0.2, f32(2 * g - 1, hd) * 0.2
        do = dev(np.full((Ls, heads * hd), SENT, np.uint32))
        check(L.dsocr_k_attention(1, Ls, heads, hd, 1.0 / math.sqrt(hd), 0, dev(q), dev(k), dev(v), do, dev(th), dev(tw),
                                  g, g))
        out[f"attention/sam{g}"] = get(do, (Ls, heads * hd))
        free_all()

    def rope(cap, rope_dim):
        ang = np.arange(cap)[:, None] * (10000.0 ** (-np.arange(rope_dim // 2) * 2.0 / rope_dim))[None, :]
        return (dev(np.concatenate([np.cos(ang), np.cos(ang)], 1).astype(np.float32)),
                dev(np.concatenate([np.sin(ang), np.sin(ang)], 1).astype(np.float32)))

    def behind_past(tag, seqs, cap, heads, kvh, hd, rope_dim, use_mla, hook, page0=0, extra=()):
        # the caches hold random rows below every past and NaN from there on; q|k|v rows of the new rows; o a sentinel
        B, pages = len(seqs), len(seqs) + page0
        T = sum(n for _, n in seqs)
        kc, vc = f32(pages, kvh, cap, hd), f32(pages, kvh, cap, hd)
        for b, (p, _) in enumerate(seqs):
            kc[page0 + b, :, p:] = np.nan
            vc[page0 + b, :, p:] = np.nan
        kc[:page0] = np.nan
        vc[:page0] = np.nan
        W = (heads + 2 * kvh) * hd
        dq, dk, dv = dev(f32(T, W)), dev(kc), dev(vc)
        do = dev(np.full((T, heads * hd), SENT, np.uint32))
        dc, ds = rope(cap, rope_dim)
        hp = (C.c_int * B)(*[p for p, _ in seqs])
        hl = (C.c_int * B)(*[n for _, n in seqs])
        hook(B, heads, kvh, hd, rope_dim, use_mla, cap, 1.0 / math.sqrt(hd), hp, hl, dq, dc, ds, dk, dv, do, *extra)
        out[tag + "/qkv"] = get(dq, (T, W))
        out[tag + "/k"] = get(dk, kc.shape)
        out[tag + "/v"] = get(dv, vc.shape)
        out[tag + "/o"] = get(do, (T, heads * hd))
        free_all()

    for name, (lens, cap, heads, kvh, hd, rd, mla) in PREFILL.items():
        for part in (1, 0) if name in PREFILL_NO_PART else (1,):
            behind_past(f"prefill/{name}-part{part}", tuple((0, n) for n in lens), cap, heads, kvh, hd, rd, mla,
                        lambda B, h, kv, d, r, m, c, sc, hp, hl, *p, part=part: check(
                            L.dsocr_k_prefill_attention(B, h, kv, d, r, m, c, sc, hl, *p, part)))
    for name, (seqs, cap, heads, kvh, hd, rd, mla) in PAST.items():
        behind_past(f"past/{name}", seqs, cap, heads, kvh, hd, rd, mla,
                    lambda *p: check(L.dsocr_k_prefill_attention_past(*p)))
        behind_past(f"chunk/{name}", seqs, cap, heads, kvh, hd, rd, mla,
                    lambda *p: check(L.dsocr_k_attention_chunk(*p)), extra=(0, len(seqs)))
    seqs, cap, heads, kvh, hd, rd, mla = PAST["gqa64"]  # a session cache: kv_page0 > 0
    behind_past("chunk/gqa64-page2", seqs, cap, heads, kvh, hd, rd, mla,
                lambda *p: check(L.dsocr_k_attention_chunk(*p)), page0=2, extra=(2, len(seqs) + 2))
    for n_seq, P, Ls, heads, kvh, hd in PREFIX:
        q, k, v = f32(n_seq * Ls, heads * hd), f32(n_seq * Ls, kvh * hd), f32(n_seq * Ls, kvh * hd)
        do = dev(np.full((n_seq * Ls, heads * hd), SENT, np.uint32))
        check(L.dsocr_k_attention_prefix(n_seq, Ls, P, heads, kvh, hd, 1.0 / math.sqrt(hd), dev(q), dev(k), dev(v), do))
        out[f"prefix/{n_seq}x{P}x{Ls}x{heads}x{kvh}x{hd}"] = get(do, (n_seq * Ls, heads * hd))
        free_all()

    np.savez(a.out, **out)
    nbytes = sum(x.nbytes for x in out.values())
    unwritten = sum(int(np.any(x == SENT)) for n, x in out.items() if n.endswith("/o") or "/" not in n[n.index("/") + 1:])
    print(f"attention_ab: {len(out)} arrays, {nbytes} bytes -> {a.out} ({unwritten} output arrays with unwritten words)")
    if not a.against:
        return 0
    ref = np.load(a.against)
    bad = sorted(set(ref.files) ^ set(out))
    for n in sorted(set(ref.files) & set(out)):
        if ref[n].shape != out[n].shape or not np.array_equal(ref[n], out[n]):
            bad.append(n)
    split = os.environ.get("DSOCR_ATTN_SPLIT", "1")
    print(f"attention_ab: DSOCR_ATTN_SPLIT={split}: {len(out) - len(bad)} of {len(out)} arrays byte-identical to "
          f"{os.path.basename(a.against)}" + ("".join("\n  differs: " + n for n in bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
