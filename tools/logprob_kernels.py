"""The two log-probability launches at the full vocabulary, for a kernel trace.

Runs dsocr_k_logprobs REPS times on B random rows (V = 129280, K = 20 by default), so that

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/logprob_kernels.py --B 8

reports the durations of dec_lp_partial_kernel and dec_lp_final_kernel at that B (one run per B: the kernel names
do not carry it).  The first call is a warm-up that the statistics include (1 of REPS + 1).
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "deepseek-ocr.rs_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1)
    ap.add_argument("--V", type=int, default=129280)
    ap.add_argument("--K", type=int, default=20)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    from dsocr._lib import check, lib
    r = np.random.default_rng(a.B)
    x = (r.standard_normal((a.B, a.V)) * 4).astype(np.float32)
    tok = r.integers(0, a.V, a.B).astype(np.int32)
    emit = np.ones(a.B, np.uint8)
    lp = np.zeros(a.B, np.float32)
    ti = np.zeros((a.B, max(a.K, 1)), np.int64)
    tl = np.zeros((a.B, max(a.K, 1)), np.float32)
    p = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
    for _ in range(a.reps + 1):
        check(lib().dsocr_k_logprobs(a.B, a.V, a.K, p(x), a.V, p(tok), p(emit), p(lp), p(ti), p(tl)))
    print(f"B={a.B} V={a.V} K={a.K} reps={a.reps} lp[0]={lp[0]:.4f} top0={int(ti[0][0]) if a.K else -1}")


if __name__ == "__main__":
    main()
