// Fused decode-step kernels (B pages x 1 token).  One decode step of the reference
// (model/mod.rs:1977-2034 -> block.rs:124-191 x 12 -> lm_head -> select_token_id)
// becomes 7 launches per layer instead of 15:
//   dec_gemv (RMSNorm fused) -> dec_attn (RoPE + KV append + flash-decoding + combine)
//   -> dec_gemv (o_proj + residual) -> dec_gemv (router, norm fused)
//   -> moe_route (softmax top-k + grouping, one block) -> moe_gateup2 (routed + shared)
//   -> moe_down2 (routed + shared + weighted combine + residual)
// Every reduction keeps the reference's f32 order where it is observable
// (top-k weighted sum in top-k order, then + shared, then the residual add).
//
// One unit per stage: decode_gemv.hip, decode_attn.hip (q/k/v + RoPE, attention, their fused launch),
// decode_route.hip, decode_moe.hip, decode_sample.hip; the matrix-core forms are in decode_mm.hip.  This header
// is private to those units: the x-row staging helpers they share, the residency queries and the two helpers
// every launch picks its kernel instantiation with.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <stdexcept>
#include <type_traits>

#include "dev_common.hpp"
#include "kernels.hpp"

namespace dsocr {

// ------------------------------------------------------------------ helpers
// Dynamic LDS of the GEMV-type kernels: [XS_RED floats of row partial sums][M][K staged rows].
constexpr int XS_RED = 128;  // >= M * (blockDim / 64)

// Sum of the squares of one float4, every product and sum rounded on its own.  The compiler contracts the plain
// expression into fused multiply-adds differently from one kernel to the next, which moved the RMSNorm divisor by
// an ulp between kernels that claim the same staged row (dec_gemv's forms, the screened lm_head's rescoring).
__device__ __forceinline__ float sumsq4(const float4 v) {
#pragma clang fp contract(off)
    return (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
}

// Block-wide: stage M rows of x (row m = rows ? rows[m] : m, stride ldx) into LDS, RMS-normalised
// when nw != null (rms_norm_slow, block.rs:24-29: x / sqrt(mean(x^2) + eps) * w).  Every
// thread of the block must call it (two barriers).
__device__ __forceinline__ void stage_rows(const float* x, long ldx, const int* rows, int M, int K, const float* nw,
                                           float eps, float* smem) {
    float* red = smem;
    float* xs = smem + XS_RED;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwv = blockDim.x >> 6;
    const int step = blockDim.x * 4;
    if (nw) {
        for (int m = 0; m < M; ++m) {
            const float* xr = x + (long)(rows ? rows[m] : m) * ldx;
            float q = 0.f;
            for (int k = tid * 4; k < K; k += step) {
                const float4 v = *reinterpret_cast<const float4*>(xr + k);
                q = __fadd_rn(q, sumsq4(v));
            }
            q = wave_sum(q);
            if (lane == 0) red[m * nwv + wave] = q;
        }
        __syncthreads();
    }
    for (int m = 0; m < M; ++m) {
        const float* xr = x + (long)(rows ? rows[m] : m) * ldx;
        float den = 1.f;
        if (nw) {
            float q = 0.f;
            for (int w = 0; w < nwv; ++w) q += red[m * nwv + w];
            den = sqrtf(q / (float)K + eps);
        }
        for (int k = tid * 4; k < K; k += step) {
            float4 v = *reinterpret_cast<const float4*>(xr + k);
            if (nw) {
                const float4 w = *reinterpret_cast<const float4*>(nw + k);
                v.x = (v.x / den) * w.x;
                v.y = (v.y / den) * w.y;
                v.z = (v.z / den) * w.z;
                v.w = (v.w / den) * w.w;
            }
            *reinterpret_cast<float4*>(xs + m * K + k) = v;
        }
    }
    __syncthreads();
}

// Two-phase staging for the hot kernels.  vmcnt is in-order on CDNA: a load issued after
// the weight stream can only be consumed once every weight load has landed.  So the
// activation rows (and the norm weight) are loaded into registers FIRST (xload), the weight
// stream is issued next, and xstage then normalises / writes LDS waiting only for the
// activation loads.  XR float4 per thread per row covers K <= XR * 4 * blockDim.
template <int MT, int XR>
struct XRegs {
    float4 v[MT][XR];
    float4 w[XR];
};

template <int MT, int XR>
__device__ __forceinline__ void xload(XRegs<MT, XR>& r, const float* x, long ldx, const int* rows, int M, int K,
                                      const float* nw) {
    const int tid = threadIdx.x, nt = blockDim.x;
    // unconditional loads from clamped addresses (a predicated load becomes an exec-masked
    // branch plus a vmcnt(0) drain in hipcc's output); lanes past K / M are ignored by xstage
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int mm = min(m, M - 1);
        const float* xr = x + (long)(rows ? rows[mm] : mm) * ldx;
#pragma unroll
        for (int i = 0; i < XR; ++i) {
            const int k = min((tid + i * nt) * 4, K - 4);
            r.v[m][i] = *reinterpret_cast<const float4*>(xr + k);
        }
    }
    const float* nwp = nw ? nw : x;
#pragma unroll
    for (int i = 0; i < XR; ++i) {
        const int k = min((tid + i * nt) * 4, K - 4);
        r.w[i] = *reinterpret_cast<const float4*>(nwp + k);
    }
}

template <int MT, int XR>
__device__ __forceinline__ void xstage(const XRegs<MT, XR>& r, int M, int K, bool norm, float eps, float* smem) {
    float* red = smem;
    float* xs = smem + XS_RED;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nt = blockDim.x, nwv = nt >> 6;
    if (norm) {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (m < M) {
                float q = 0.f;
#pragma unroll
                for (int i = 0; i < XR; ++i) {
                    const float4 v = r.v[m][i];
                    if ((tid + i * nt) * 4 < K) q = __fadd_rn(q, sumsq4(v));
                }
                q = wave_sum(q);
                if (lane == 0) red[m * nwv + wave] = q;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        if (m < M) {
            float den = 1.f;
            if (norm) {
                float q = 0.f;
                for (int w = 0; w < nwv; ++w) q += red[m * nwv + w];
                den = sqrtf(q / (float)K + eps);
            }
#pragma unroll
            for (int i = 0; i < XR; ++i) {
                const int k = (tid + i * nt) * 4;
                if (k < K) {
                    float4 v = r.v[m][i];
                    if (norm) {
                        const float4 w = r.w[i];
                        v.x = (v.x / den) * w.x;
                        v.y = (v.y / den) * w.y;
                        v.z = (v.z / den) * w.z;
                        v.w = (v.w / den) * w.w;
                    }
                    *reinterpret_cast<float4*>(xs + m * K + k) = v;
                }
            }
        }
    }
    __syncthreads();
}

// 8 consecutive f32 (LDS or global) into registers
__device__ __forceinline__ void ld_x8(const float* xs, float* o) {
    const float4 a = *reinterpret_cast<const float4*>(xs);
    const float4 b = *reinterpret_cast<const float4*>(xs + 4);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}

inline size_t stage_bytes(int M, int K) { return sizeof(float) * (XS_RED + (size_t)M * K); }
constexpr size_t STAGE_LDS_MAX = 64 * 1024;

// ------------------------------------------------------------------ host: residency queries
// CUs of the current device (asked once per process; 0: the query failed) and the blocks of 256 threads of
// `kernel` one CU holds at `lds` dynamic bytes (0: the query failed).  Callers cache the product themselves.
inline int device_cus() {
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 0;
    }
    return cus;
}
template <typename K>
int blocks_per_cu(K kernel, size_t lds) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, lds) != hipSuccess) return 0;
    return per_cu;
}

// ------------------------------------------------------------------ host: template selection
// A launch picks its kernel instantiation in one place each: the weight element type as a value
// (f(bf16_t{}) or f(f16_t{}); in the lambda: using WT = decltype(wt)) ...
template <typename F>
auto with_wt(int wdtype, F&& f) {
    if (wdtype == WDT_BF16) return f(bf16_t{});
    return f(f16_t{});
}
// ... and a compile-time int out of the listed ones (a staged-row template, a head size, a top-k) as a
// std::integral_constant (in the lambda: constexpr int MT = decltype(mt)::value).  Only the listed values are
// instantiated; any other is a dispatch bug and throws, it never takes the last branch.
template <int... Vs, typename F>
void with_rows(int v, F&& f) {
    if (!((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...))
        throw std::runtime_error("EINTERNAL: decode dispatch: no kernel template for this value");
}

}  // namespace dsocr
