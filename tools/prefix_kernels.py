"""launch_attention_past and launch_session_prefix_copy alone at the full-size shape, for a kernel
trace: one sequence of 6 new rows behind a past of 700 (10 heads, head dim 128), and a copy of 700 rows of the
full-size cache (12 layers, 10 kv heads) out of a slot and back into it.  Each runs REPS times through its hook.

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/prefix_kernels.py
"""
import ctypes as C
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "deepseek-ocr.rs_amd")]

REPS = 20


def main():
    from dsocr._lib import check, lib
    L = lib()

    def dev(a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        check(L.dsocr_dev_alloc(a.nbytes, C.byref(p)))
        check(L.dsocr_memcpy_h2d(p, a.ctypes.data_as(C.c_void_p), a.nbytes))
        return p

    rng = np.random.default_rng(0)
    heads, hd, past, n, cap, layers, slots = 10, 128, 700, 6, 1232, 12, 2
    qkv = rng.standard_normal((n, 3 * heads * hd)).astype(np.float32)
    ang = np.arange(cap)[:, None] * (10000.0 ** (-np.arange(hd // 2) * 2.0 / hd))[None, :]
    cos = np.concatenate([np.cos(ang), np.cos(ang)], 1).astype(np.float32)
    sin = np.concatenate([np.sin(ang), np.sin(ang)], 1).astype(np.float32)
    kc = rng.standard_normal((heads, cap, hd)).astype(np.float32)
    dq, dc, ds, dk, dv = dev(qkv), dev(cos), dev(sin), dev(kc), dev(kc)
    do = dev(np.zeros((n, heads * hd), np.float32))
    for _ in range(REPS):
        check(L.dsocr_k_prefill_attention_past(1, heads, heads, hd, hd, 0, cap, 1.0 / math.sqrt(hd), (C.c_int * 1)(past),
                                               (C.c_int * 1)(n), dq, dc, ds, dk, dv, do))
    cache = np.zeros((layers, slots, heads, cap, hd), np.float32)
    ck, cv = dev(cache), dev(cache)
    entry = dev(np.zeros(2 * layers * heads * past * hd, np.float32))
    for i in range(REPS):
        check(L.dsocr_k_session_prefix_copy(layers, slots, heads, cap, hd, ck, cv, i % 2, past, entry, i % 2))
    for p in (dq, dc, ds, dk, dv, do, ck, cv, entry):
        L.dsocr_dev_free(p)
    print(f"{REPS} x attention_past (past {past}, {n} new rows, {heads} heads, hd {hd}); {REPS} x prefix copy of {past} rows, "
          f"{2 * layers * heads * past * hd * 4 / 1e6:.1f} MB each")


if __name__ == "__main__":
    main()
