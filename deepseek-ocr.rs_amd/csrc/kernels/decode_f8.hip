// FP8 (OCP E4M3) expert weights for the decode MoE at T = 1..8 tokens (DSOCR_LOAD_FP8_EXPERTS).  Contract:
// DESIGN.md section 4.4.3.  Every expert row keeps one power-of-two exponent e_r and one E4M3 code per weight:
// W8[r][k] = 2^e_r * e4m3(code[r][k]), an fp16 value by construction, and the launches compute
// y[t][r] = 2^e_r * sum_k e4m3(code[r][k]) * x[t][k] in f32 (fmaf, fixed order), the scale applied once per row.
//
// Kernels:
//   fp8_quantize_rows  load time, one wave per row: amax over the row (DPP), e_r from the float's exponent and
//                      significand, codes by v_cvt_pk_fp8_f32 of the exactly scaled values.
//   moe_gateup_f8      grid (row chunks, expert records + shared).  The block stages its record's token rows in
//                      LDS as f32 once; every 8 lanes own one gate row and its up row (32 row pairs per block).
//   moe_down_f8        one block per 4 output rows, 16 lanes per row; its 4 waves split the layer's items (expert
//                      records, then the shared expert cut into pieces of I columns so that the items are of one
//                      length); the per-wave sums meet in LDS and are added to the residual in a fixed order.
//   fp8_dequant_rows   load time: W8 written over the layer's fp16 rows, so that prefill and batches above 8 run on
//                      the same weights as the FP8 launches.
//   fp8_rows_dot       parity hook: y[T][rows] = x . W8^T through the same row walk.
//
// Row walk (F8Stream).  Lane k of a GW-lane group owns codes [16 (GW s + k), +16) of the row at step s: one
// nontemporal dwordx4.  load() issues the loads of up to CH steps back to back (the whole row in the MoE
// launches) before fma() consumes the first; per dword two v_cvt_pk_f32_fp8 (low and high word) give four f32
// weights, each one fmaf per token against the token row (LDS broadcast in gate/up, L2 in down).  The GW x 8
// (lane, token) partials of a row are summed transposed on DPP at the row's end, so that lane k ends with token k.
#include <hip/hip_fp16.h>

#include <algorithm>
#include <cstdint>
#include <stdexcept>

#include "dev_common.hpp"
#include "kernels.hpp"

namespace dsocr {

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// 2^e as an f32 (|e| <= 126)
__device__ __forceinline__ float pow2i(int e) { return __uint_as_float((uint32_t)(127 + e) << 23); }

// four E4M3 codes of one dword -> f32 (byte j -> o[j])
__device__ __forceinline__ void e4m3x4(uint32_t w, float* o) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    o[0] = lo.x; o[1] = lo.y; o[2] = hi.x; o[3] = hi.y;
}
__device__ __forceinline__ void e4m3x16(const uint4 q, float* o) {
    e4m3x4(q.x, o); e4m3x4(q.y, o + 4); e4m3x4(q.z, o + 8); e4m3x4(q.w, o + 12);
}

// Transposed sum of the GW x 8 (lane, token) partials of a group (GW = 8 or 16): lane k ends with the sum over the
// group's lanes of v[k & 7], every select on a compile-time register index (7 DPP exchanges per 8 lanes; at
// GW = 16 a row mirror folds the two halves first, and both halves end with the same totals).
template <int GW>
__device__ __forceinline__ float group_transpose_sum(const float* v, int k) {
    float f[8], a[4], b[2];
#pragma unroll
    for (int t = 0; t < 8; ++t) f[t] = GW == 16 ? v[t] + dpp_f<DPP_ROW_MIRROR>(0.f, v[t]) : v[t];
    const bool h4 = k & 4, h2 = k & 2, h1 = k & 1;
#pragma unroll
    for (int u = 0; u < 4; ++u)  // partner 7 - k: the lanes with bit 2 clear keep tokens 0..3
        a[u] = (h4 ? f[4 + u] : f[u]) + dpp_f<DPP_ROW_HALF_MIRROR>(0.f, h4 ? f[u] : f[4 + u]);
#pragma unroll
    for (int u = 0; u < 2; ++u)  // partner k ^ 2
        b[u] = (h2 ? a[2 + u] : a[u]) + dpp_f<DPP_QUAD_XOR2>(0.f, h2 ? a[u] : a[2 + u]);
    return (h1 ? b[1] : b[0]) + dpp_f<DPP_QUAD_XOR1>(0.f, h1 ? b[0] : b[1]);
}

// ------------------------------------------------------------------ load-time quantiser
// smallest e with amax 2^-e <= 448 (= 0.875 * 2^9), clamped to e >= -15; amax = m 2^ex, m in [0.5, 1)
__device__ __forceinline__ int row_exponent(float amax) {
    if (amax == 0.f) return 0;
    const uint32_t b = __float_as_uint(amax);
    const int ex = (int)(b >> 23) - 126;  // (an fp16 value widened: always a normal f32)
    const int e = ex - 9 + ((b & 0x7fffffu) > 0x600000u ? 1 : 0);
    return max(e, -15);
}

__global__ __launch_bounds__(256) void fp8_quantize_rows_kernel(long rows, int cols, const uint16_t* w, uint8_t* codes,
                                                                 int8_t* exps) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;  // wave-uniform
    const uint16_t* wr = w + r * cols;
    const int chunks = cols >> 3;  // 8 fp16 per 16-byte load
    float amax = 0.f;
    for (int c = lane; c < chunks; c += 64) {
        float v[8];
        unpack8<f16_t>(*reinterpret_cast<const uint4*>(wr + 8 * c), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
    }
    amax = wave_max(amax);
    const int e = row_exponent(amax);
    const float inv = pow2i(-e);  // exact: the conversion below is the only rounding
    for (int c = lane; c < chunks; c += 64) {
        float v[8];
        unpack8<f16_t>(*reinterpret_cast<const uint4*>(wr + 8 * c), v);
        int lo = 0, hi = 0;
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[0] * inv, v[1] * inv, lo, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[2] * inv, v[3] * inv, lo, true);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[4] * inv, v[5] * inv, hi, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[6] * inv, v[7] * inv, hi, true);
        *reinterpret_cast<uint2*>(codes + r * cols + 8 * c) = make_uint2((uint32_t)lo, (uint32_t)hi);
    }
    if (lane == 0) exps[r] = (int8_t)e;
}

// W8 as fp16 (exact: 2^e_r e4m3(code) is an fp16 value): what prefill and batches above 8 read for an FP8 layer
__global__ __launch_bounds__(256) void fp8_dequant_rows_kernel(long rows, int cols, const uint8_t* codes, const int8_t* exps,
                                                                uint16_t* out) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float sc = pow2i(exps[r]);
    for (int c = lane; c < (cols >> 3); c += 64) {
        const uint2 q = *reinterpret_cast<const uint2*>(codes + r * cols + 8 * c);
        float v[8];
        e4m3x4(q.x, v);
        e4m3x4(q.y, v + 4);
        uint32_t h[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const _Float16 lo = (_Float16)(v[2 * j] * sc), hi = (_Float16)(v[2 * j + 1] * sc);
            uint16_t bl, bh;
            __builtin_memcpy(&bl, &lo, 2);
            __builtin_memcpy(&bh, &hi, 2);
            h[j] = (uint32_t)bl | ((uint32_t)bh << 16);
        }
        *reinterpret_cast<uint4*>(out + r * cols + 8 * c) = make_uint4(h[0], h[1], h[2], h[3]);
    }
}

// ------------------------------------------------------------------ the row walk
template <int GW, int NR, int CH>
struct F8Stream {
    static constexpr int SPAN = GW * 16;  // codes of one row a group takes per step
    uint4 q[CH][NR];

    // issue the loads of steps [s0, s0 + CH) of the NR rows; lanes past the row's end read its first granule
    __device__ __forceinline__ void load(const uint8_t* const* row, int in_dim, int s0) {
        const int k = threadIdx.x & (GW - 1), steps = (in_dim + SPAN - 1) / SPAN;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            if (s0 + c < steps) {  // group-uniform
                const int off = (s0 + c) * SPAN + 16 * k;
#pragma unroll
                for (int r = 0; r < NR; ++r) q[c][r] = ldg_nt16(row[r] + (off < in_dim ? off : 0));
            }
        }
    }

    // acc[r][t] += the lane's codes of those steps . x[xoff[t] + column], for the tokens of tmask
    __device__ __forceinline__ void fma(int in_dim, int s0, const float* x, const int* xoff, int tmask, float (*acc)[8]) const {
        const int k = threadIdx.x & (GW - 1), steps = (in_dim + SPAN - 1) / SPAN;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            if (s0 + c < steps) {
                const int off = (s0 + c) * SPAN + 16 * k;
                const bool in = off < in_dim;
                const int offc = in ? off : 0;
                float w[NR][16];
#pragma unroll
                for (int r = 0; r < NR; ++r)  // (a lane past the row's end multiplies by code 0)
                    e4m3x16(in ? q[c][r] : make_uint4(0u, 0u, 0u, 0u), w[r]);
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    if ((tmask >> t) & 1) {  // wave-uniform
                        const float4* xp = reinterpret_cast<const float4*>(x + xoff[t] + offc);
                        const float4 x0 = xp[0], x1 = xp[1], x2 = xp[2], x3 = xp[3];
                        const float xv[16] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w,
                                              x2.x, x2.y, x2.z, x2.w, x3.x, x3.y, x3.z, x3.w};
#pragma unroll
                        for (int r = 0; r < NR; ++r)
#pragma unroll
                            for (int j = 0; j < 16; ++j) acc[r][t] = fmaf(w[r][j], xv[j], acc[r][t]);
                    }
                }
            }
        }
    }
};

// ------------------------------------------------------------------ y = x . W8^T (parity hook)
constexpr int DOT_CH = 4;
__global__ __launch_bounds__(256) void fp8_rows_dot_kernel(F8Mat m, long rows, int cols, int T, const float* x, float* y) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    for (int i = threadIdx.x * 4; i < T * cols; i += 1024) *reinterpret_cast<float4*>(xs + i) = *reinterpret_cast<const float4*>(x + i);
    __syncthreads();
    const int k = threadIdx.x & 7;
    const long r = (long)blockIdx.x * 32 + (threadIdx.x >> 3);
    const long rc = r < rows ? r : rows - 1;
    const uint8_t* row[1] = {m.q + rc * cols};
    int xoff[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) xoff[t] = t * cols;
    float acc[1][8];
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[0][t] = 0.f;
    F8Stream<8, 1, DOT_CH> st;
    const int steps = (cols + 127) / 128;
    for (int s0 = 0; s0 < steps; s0 += DOT_CH) {
        st.load(row, cols, s0);
        st.fma(cols, s0, xs, xoff, (1 << T) - 1, acc);
    }
    const float v = group_transpose_sum<8>(acc[0], k) * pow2i(m.e[rc]);  // lane k: token k
    if (k < T && r < rows) y[(long)k * rows + r] = v;
}

// ------------------------------------------------------------------ gate/up
constexpr int GU_GW = 8, GU_RPB = 256 / GU_GW;  // lanes per row pair, row pairs per block
constexpr int GU_CH = 12;                       // steps of 128 codes held in flight: a whole row of H <= 1536
constexpr int GU_XR = 2;                        // float4 per thread per token row: H <= 2048

__global__ __launch_bounds__(256) void moe_gateup_f8_kernel(MoeF8Args a) {
    WaveSpan span_(a.span);
    extern __shared__ __attribute__((aligned(16))) float xs[];
    const int item = blockIdx.y, tid = threadIdx.x;
    const bool routed = item < a.slots;
    const int* rec = a.grp + MOE_GRP_REC * (1 + item);
    int n = a.T, e = 0;
    if (routed) {
        if (item >= a.grp[0] || blockIdx.x * GU_RPB >= a.I) return;  // block-uniform, before any barrier
        e = rec[0];
        n = min(rec[1], 8);
    } else if (blockIdx.x * GU_RPB >= a.Is) {
        return;
    }
    const int rows_I = routed ? a.I : a.Is;
    const F8Mat& m = routed ? a.Wgu : a.sWgu;
    // 1. the record's token rows into registers (token = h row / topk for a routed pick)
    // (unconditional loads from clamped rows: a predicated load would keep the rows in scratch)
    float4 xr[8][GU_XR];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int tc = min(t, n - 1);
        const float* xp = a.x + (long)(routed ? rec[2 + tc] / a.topk : tc) * a.H;
#pragma unroll
        for (int i = 0; i < GU_XR; ++i) xr[t][i] = *reinterpret_cast<const float4*>(xp + min((tid + i * 256) * 4, a.H - 4));
    }
    // 2. the whole gate row and up row of the group, issued before anything is consumed
    const int k = tid & (GU_GW - 1);
    const int i = blockIdx.x * GU_RPB + tid / GU_GW;
    const long r0 = (long)e * 2 * rows_I + min(i, rows_I - 1);  // (shared: e = 0)
    const uint8_t* row[2] = {m.q + r0 * a.H, m.q + (r0 + rows_I) * a.H};
    F8Stream<GU_GW, 2, GU_CH> st;
    st.load(row, a.H, 0);
    const int eg = m.e[r0], eu = m.e[r0 + rows_I];
    // 3. stage the token rows (waits for the activation loads only)
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        if (t < n) {
#pragma unroll
            for (int j = 0; j < GU_XR; ++j) {
                const int c = (tid + j * 256) * 4;
                if (c < a.H) *reinterpret_cast<float4*>(xs + t * a.H + c) = xr[t][j];
            }
        }
    }
    __syncthreads();
    int xoff[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) xoff[t] = t * a.H;
    float acc[2][8];
#pragma unroll
    for (int t = 0; t < 8; ++t) { acc[0][t] = 0.f; acc[1][t] = 0.f; }
    st.fma(a.H, 0, xs, xoff, (1 << n) - 1, acc);
    // lane k of the group hands over token k
    const float gs = group_transpose_sum<GU_GW>(acc[0], k) * pow2i(eg), us = group_transpose_sum<GU_GW>(acc[1], k) * pow2i(eu);
    if (k < n && i < rows_I) {
        float hv = (gs / (1.0f + expf(-gs))) * us;  // silu (candle: x / (1 + exp(-x)))
        if (routed) a.h[(long)rec[2 + k] * a.I + i] = hv * __int_as_float(rec[10 + k]);
        else a.hs[(long)k * a.Is + i] = hv;
    }
}

// ------------------------------------------------------------------ down + combine + residual
constexpr int DN_GW = 16, DN_ROWS = 64 / DN_GW;  // lanes per row, output rows per block (every wave walks the same rows)
constexpr int DN_CH = 8;                         // steps of 256 codes in flight: a whole item of up to 2048 columns

__global__ __launch_bounds__(256) void moe_down_f8_kernel(MoeF8Args a) {
    WaveSpan span_(a.span);
    __shared__ float part[4][DN_ROWS][8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / DN_GW, k = lane & (DN_GW - 1);
    const int j0 = blockIdx.x * DN_ROWS;
    const int j = min(j0 + g, a.H - 1);  // rows past H repeat the last one (never written)
    const int ng = min(a.grp[0], a.slots);
    const int np = a.Is > 0 ? (a.Is + a.I - 1) / a.I : 0;  // the shared expert as pieces of I columns
    float tot = 0.f;  // token (k & 7) of row j over the wave's items
    for (int item = wave; item < ng + np; item += 4) {  // wave-uniform
        int xoff[8], tmask = 0, in_dim, ej;
        const uint8_t* row[1];
        const float* x;
        if (item < ng) {
            const int* rec = a.grp + MOE_GRP_REC * (1 + item);
            const int e = rec[0], n = min(rec[1], 8);
#pragma unroll
            for (int t = 0; t < 8; ++t) xoff[t] = 0;
            for (int q = 0; q < n; ++q) {
                const int hrow = rec[2 + q], tk = hrow / a.topk;
#pragma unroll
                for (int t = 0; t < 8; ++t)
                    if (t == tk) { xoff[t] = hrow * a.I; tmask |= 1 << t; }
            }
            const long r = (long)e * a.H + j;
            row[0] = a.Wd.q + r * a.I;
            ej = a.Wd.e[r];
            in_dim = a.I;
            x = a.h;
        } else {
            const int c0 = (item - ng) * a.I;
#pragma unroll
            for (int t = 0; t < 8; ++t) xoff[t] = t * a.Is + c0;
            tmask = (1 << a.T) - 1;
            row[0] = a.sWd.q + (long)j * a.Is + c0;
            ej = a.sWd.e[j];
            in_dim = min(a.I, a.Is - c0);
            x = a.hs;
        }
        float acc[1][8];
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[0][t] = 0.f;
        F8Stream<DN_GW, 1, DN_CH> st;
        const int steps = (in_dim + DN_GW * 16 - 1) / (DN_GW * 16);
        for (int s0 = 0; s0 < steps; s0 += DN_CH) {
            st.load(row, in_dim, s0);
            st.fma(in_dim, s0, x, xoff, tmask, acc);
        }
        tot += group_transpose_sum<DN_GW>(acc[0], k) * pow2i(ej);  // (a token outside the item adds its zero)
    }
    if (k < 8) part[wave][g][k] = tot;
    __syncthreads();
    const int rr = threadIdx.x >> 3, t = threadIdx.x & 7;
    if (rr < DN_ROWS && j0 + rr < a.H && t < a.T) {
        const float v = ((part[0][rr][t] + part[1][rr][t]) + part[2][rr][t]) + part[3][rr][t];
        float* o = a.out + (long)t * a.H + j0 + rr;
        *o = *o + v;
    }
}

}  // namespace

// ------------------------------------------------------------------ host side
bool fp8_rows_ok(long cols) { return cols > 0 && cols % 16 == 0; }

void launch_fp8_quantize_rows(long rows, long cols, const void* w_f16, uint8_t* codes, int8_t* exps, hipStream_t s) {
    if (rows <= 0 || !fp8_rows_ok(cols) || cols > (1L << 30) || !w_f16 || !codes || !exps)
        throw std::runtime_error("EINVAL: fp8_quantize_rows takes rows of a multiple of 16 fp16 values");
    hipLaunchKernelGGL(fp8_quantize_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, rows, (int)cols,
                       reinterpret_cast<const uint16_t*>(w_f16), codes, exps);
}

void launch_fp8_dequant_rows(long rows, long cols, const F8Mat& m, void* w8_f16, hipStream_t s) {
    if (rows <= 0 || !fp8_rows_ok(cols) || cols > (1L << 30) || !m.q || !m.e || !w8_f16)
        throw std::runtime_error("EINVAL: fp8_dequant_rows takes rows of a multiple of 16 codes");
    hipLaunchKernelGGL(fp8_dequant_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, rows, (int)cols, m.q, m.e,
                       reinterpret_cast<uint16_t*>(w8_f16));
}

void launch_fp8_rows_dot(const F8Mat& m, long rows, long cols, int T, const float* x, float* y, hipStream_t s) {
    if (rows <= 0 || !fp8_rows_ok(cols) || !m.q || !m.e || !x || !y)
        throw std::runtime_error("EINVAL: fp8_rows_dot takes rows of a multiple of 16 codes");
    if (T < 1 || T > 8) throw std::runtime_error("EINVAL: fp8_rows_dot takes 1..8 token rows");
    const size_t lds = sizeof(float) * (size_t)T * cols;
    if (lds > 64 * 1024) throw std::runtime_error("EINVAL: fp8_rows_dot rows too wide for LDS staging");
    hipLaunchKernelGGL(fp8_rows_dot_kernel, dim3((unsigned)((rows + 31) / 32)), dim3(256), lds, s, m, rows, (int)cols, T, x, y);
}

bool moe_f8_ok(const MoeF8Args& a) {
    if (a.T < 1 || a.T > 8 || a.topk < 1 || a.topk > 8 || a.T * a.topk > 64 || a.slots < 1) return false;
    if (!a.x || !a.h || !a.out || !a.grp || !a.Wgu.q || !a.Wgu.e || !a.Wd.q || !a.Wd.e) return false;
    if (a.H % 16 || a.I % 16 || a.I <= 0 || a.H <= 0 || a.H > GU_CH * GU_GW * 16 || a.H > GU_XR * 1024) return false;
    if (a.Is > 0 && (a.Is % 16 || !a.hs || !a.sWgu.q || !a.sWgu.e || !a.sWd.q || !a.sWd.e)) return false;
    return (long)a.T * a.topk * a.I < (1L << 31) && sizeof(float) * 8 * (size_t)a.H <= 64 * 1024;
}

void launch_moe_gateup_f8(const MoeF8Args& a, hipStream_t s) {
    if (!moe_f8_ok(a)) throw std::runtime_error("EINVAL: FP8 decode MoE outside its range");
    const int rows = std::max(a.I, a.Is);
    const dim3 grid((unsigned)((rows + GU_RPB - 1) / GU_RPB), (unsigned)(a.slots + (a.Is > 0 ? 1 : 0)));
    DSOCR_LAUNCH(moe_gateup_f8_kernel, grid, dim3(256), sizeof(float) * 8 * (size_t)a.H, s, a);
}

void launch_moe_down_f8(const MoeF8Args& a, hipStream_t s) {
    if (!moe_f8_ok(a)) throw std::runtime_error("EINVAL: FP8 decode MoE outside its range");
    DSOCR_LAUNCH(moe_down_f8_kernel, dim3((unsigned)((a.H + DN_ROWS - 1) / DN_ROWS)), dim3(256), 0, s, a);
}

}  // namespace dsocr
