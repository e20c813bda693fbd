"""launch_attention_chunk beside launch_attention_past on the same inputs at the full-size shape,
for a kernel trace: one sequence of NEW new rows behind a past of 128, 384 and 640 rows (10 heads, head dim 128),
each kernel REPS times per shape through its hook.  --new also runs other row counts (the crossover).

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/chunk_kernels.py [--new 128,32,6]

The trace's per-dispatch grid sizes tell the shapes apart: attention_chunk_kernel runs ceil(new / 32) x 10
workgroups of 512 threads, attention_past_kernel ceil((past + new) / 128) x 10 x ceil(new / 32) of 256.
"""
import argparse
import ctypes as C
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "deepseek-ocr.rs_amd")]

REPS = 20
PASTS = (128, 384, 640)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", default="128")
    ap.add_argument("--only", default="chunk,past", help="which kernels run")
    a = ap.parse_args()
    from dsocr._lib import check, lib
    L = lib()

    def dev(x):
        x = np.ascontiguousarray(x)
        p = C.c_void_p()
        check(L.dsocr_dev_alloc(x.nbytes, C.byref(p)))
        check(L.dsocr_memcpy_h2d(p, x.ctypes.data_as(C.c_void_p), x.nbytes))
        return p

    rng = np.random.default_rng(0)
    heads, hd, cap = 10, 128, 1232
    ang = np.arange(cap)[:, None] * (10000.0 ** (-np.arange(hd // 2) * 2.0 / hd))[None, :]
    dc = dev(np.concatenate([np.cos(ang), np.cos(ang)], 1).astype(np.float32))
    ds = dev(np.concatenate([np.sin(ang), np.sin(ang)], 1).astype(np.float32))
    kc = rng.standard_normal((heads, cap, hd)).astype(np.float32)
    dk, dv = dev(kc), dev(kc)
    scale = 1.0 / math.sqrt(hd)
    for n in [int(x) for x in a.new.split(",")]:
        qkv = rng.standard_normal((n, 3 * heads * hd)).astype(np.float32)
        do = dev(np.zeros((n, heads * hd), np.float32))
        for past in PASTS:
            hp, hl = (C.c_int * 1)(past), (C.c_int * 1)(n)
            for kind in a.only.split(","):
                for _ in range(REPS):
                    dq = dev(qkv)  # (the hooks rotate q in place)
                    if kind == "chunk":
                        check(L.dsocr_k_attention_chunk(1, heads, heads, hd, hd, 0, cap, scale, hp, hl, dq, dc, ds, dk, dv,
                                                        do, 0, 1))
                    else:
                        check(L.dsocr_k_prefill_attention_past(1, heads, heads, hd, hd, 0, cap, scale, hp, hl, dq, dc, ds,
                                                               dk, dv, do))
                    L.dsocr_dev_free(dq)
            print(f"{REPS} x [{a.only}] past {past}, {n} new rows, {heads} heads, hd {hd}")
        L.dsocr_dev_free(do)
    for p in (dc, ds, dk, dv):
        L.dsocr_dev_free(p)


if __name__ == "__main__":
    main()
