// Decode MoE from packed DSQ blocks (Q4_K / Q8_0) for T = 1..8 tokens: the expert rows stay quantised on
// the device and are decoded in registers by the decoder the load-time dequantiser uses (dsq_decode.hpp).
// Every weight is the fp16 value dequant-on-load would have stored, widened to f32; products and sums are
// f32 (fmaf), so the packed path differs from the fp16 kernels only in summation order.
//
// Packed layout (QMat, made by launch_dsq_repack from record-layout payloads; the decoded values do not change):
//   Q4_K  the 144-byte super-blocks as recorded, rows concatenated: 144 = 9 x 16, so in a 16-byte-aligned
//         buffer every header {d, dmin, scales[12]} is one dwordx4 and every lane's quant word is aligned
//   Q8_0  the 34-byte blocks split into an int8 plane [rows][in_dim] (rows 32-byte aligned) followed by a
//         scale plane f16 [rows][in_dim / 32]
// Lane mapping of one row (qrow_unpack): Q4_K — a half-wave per super-block, lane l of 32 decodes the quant
// word 4l..4l+3 of the block (4 low-nibble + 4 high-nibble values), two super-blocks per wave iteration;
// Q8_0 — lane l decodes 8 consecutive codes, 512 values (16 blocks) per wave iteration.
//
// Launches (both in grouped form: an expert picked by several tokens is decoded once and applied to all of
// them; the records are the router launch's, MOE_GRP_* layout):
//   moe_gateup_q  grid (row chunks, expert slots + shared): a wave decodes QG_RW gate rows and their up rows
//                 and dots them with the group's normalised token rows (read from xn through L1 / L2);
//                 SwiGLU, the routing weight folded into h (as the fp16 kernels do)
//   moe_down_q    one block per QD_R output rows; its 4 waves split the layer's items (expert groups + the shared
//                 expert), each decoding its items' down rows once for all the item's tokens; the partial
//                 sums meet in LDS and the block adds them to the residual stream in a fixed order (no
//                 cross-workgroup reduction, no polled hand-off)
#include <hip/hip_fp16.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#include "dev_common.hpp"
#include "dsq_decode.hpp"
#include "kernels.hpp"

namespace dsocr {

namespace {

__device__ __forceinline__ uint32_t ldg_nt_u32(const void* p) {
    return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p));
}

// 8 weights of row `row` for this lane at wave iteration `it`: o[0..3] are elements oa..oa+3 of the row,
// o[4..7] elements ob..ob+3.  False (nothing loaded) when the lane's elements lie past in_dim.
template <int QT>
__device__ __forceinline__ bool qrow_unpack(const QMat& m, long row, int in_dim, int it, int lane, float* o, int& oa,
                                            int& ob) {
    if (QT == DSQ_Q4K) {
        const int nb = in_dim >> 8, sb = 2 * it + (lane >> 5), l32 = lane & 31;
        oa = sb * 256 + q4k_lane_off(l32);
        ob = oa + 32;
        if (sb >= nb) return false;
        const uint8_t* blk = reinterpret_cast<const uint8_t*>(m.q) + (row * nb + sb) * 144;
        const uint4 hdr = ldg_nt16(blk);
        const uint32_t qs = ldg_nt_u32(blk + 16 + 4 * l32);
        q4k_unpack8(hdr, qs, l32, o);
        return true;
    } else {
        oa = it * 512 + lane * 8;
        ob = oa + 4;
        if (oa >= in_dim) return false;
        const int nb = in_dim >> 5;
        const uint8_t* q = reinterpret_cast<const uint8_t*>(m.q) + row * in_dim + oa;
        const uint32_t q0 = ldg_nt_u32(q), q1 = ldg_nt_u32(q + 4);
        const uint16_t db = reinterpret_cast<const uint16_t*>(m.d)[row * nb + (oa >> 5)];
        q8_0_unpack8(f16_bits_to_f32(db), q0, q1, o);
        return true;
    }
}
template <int QT>
__device__ __forceinline__ int qrow_iters(int in_dim) {
    return QT == DSQ_Q4K ? ((in_dim >> 8) + 1) >> 1 : (in_dim + 511) >> 9;
}

__device__ __forceinline__ void ld_x8q(const float* x, int oa, int ob, float* v) {
    const float4 a = *reinterpret_cast<const float4*>(x + oa);
    const float4 b = *reinterpret_cast<const float4*>(x + ob);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// ------------------------------------------------------------------ repack
__global__ __launch_bounds__(256) void dsq_repack_q8_0_kernel(const uint8_t* __restrict__ src, long nblocks,
                                                              uint8_t* __restrict__ q, uint16_t* __restrict__ d) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nblocks * 32; i += (long)gridDim.x * 256) {
        const long b = i >> 5;
        const int k = (int)(i & 31);
        const uint8_t* blk = src + b * 34;
        q[i] = blk[2 + k];
        if (k == 0) d[b] = (uint16_t)blk[0] | ((uint16_t)blk[1] << 8);
    }
}

// ------------------------------------------------------------------ y = x . W^T (parity hook)
// One wave per row.  Terms with x == 0 are skipped and every sum starts from -0 (the identity of IEEE
// addition), so a one-hot x returns the decoded weight itself, the sign of a zero included.
template <int QT>
__global__ __launch_bounds__(256) void dsq_rows_dot_kernel(QMat m, long rows, int in_dim, int T, const float* x, float* y) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = -0.0f;
    const int iters = qrow_iters<QT>(in_dim);
    for (int it = 0; it < iters; ++it) {
        float w[8];
        int oa, ob;
        const bool ok = qrow_unpack<QT>(m, row, in_dim, it, lane, w, oa, ob);
        if (ok) {
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                if (t < T) {
                    float xv[8];
                    ld_x8q(x + (long)t * in_dim, oa, ob, xv);
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (xv[j] != 0.f) acc[t] = fmaf(xv[j], w[j], acc[t]);
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        if (t < T) {
            // (wave_sum's DPP fill value is +0: -0 + +0 = +0 would lose the sign, so a plain butterfly here)
            float v = acc[t];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0) y[(long)t * rows + row] = v;
        }
    }
}

// ------------------------------------------------------------------ gate/up
constexpr int QG_RW = 2;  // gate/up row pairs per wave

template <int QT>
__device__ __forceinline__ void gateup_q_body(const MoeQArgs& a, const QMat& m, long row0, int rows_I, int i0, int n,
                                              const int* xrow, const int* orow, const float* ow, float* hout) {
    const int lane = threadIdx.x & 63;
    float acc[QG_RW][2][8];
#pragma unroll
    for (int r = 0; r < QG_RW; ++r)
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int t = 0; t < 8; ++t) acc[r][g][t] = 0.f;
    const int iters = qrow_iters<QT>(a.H);
    for (int it = 0; it < iters; ++it) {
        float w[QG_RW][2][8];
        int oa = 0, ob = 0;
        bool ok = false;
#pragma unroll
        for (int r = 0; r < QG_RW; ++r) {
            const int i = min(i0 + r, rows_I - 1);
#pragma unroll
            for (int g = 0; g < 2; ++g) ok = qrow_unpack<QT>(m, row0 + (long)g * rows_I + i, a.H, it, lane, w[r][g], oa, ob);
        }
        if (ok) {
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                if (t < n) {
                    float xv[8];
                    ld_x8q(a.x + (long)xrow[t] * a.H, oa, ob, xv);
#pragma unroll
                    for (int r = 0; r < QG_RW; ++r)
#pragma unroll
                        for (int g = 0; g < 2; ++g)
#pragma unroll
                            for (int j = 0; j < 8; ++j) acc[r][g][t] = fmaf(xv[j], w[r][g][j], acc[r][g][t]);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < QG_RW; ++r) {
        const int i = i0 + r;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            if (t < n) {
                const float gs = wave_sum(acc[r][0][t]);
                const float us = wave_sum(acc[r][1][t]);
                if (lane == 0 && i < rows_I) {
                    float hv = (gs / (1.0f + expf(-gs))) * us;  // silu (candle: x / (1 + exp(-x)))
                    if (ow) hv = hv * ow[t];
                    hout[(long)orow[t] * rows_I + i] = hv;
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void moe_gateup_q_kernel(MoeQArgs a) {
    WaveSpan span_(a.span);
    const int wave = threadIdx.x >> 6;
    const int item = blockIdx.y, i0 = (blockIdx.x * 4 + wave) * QG_RW;
    int xrow[8], orow[8];
    float ow[8];
    if (item < a.slots) {
        if (item >= a.grp[0] || i0 >= a.I) return;
        const int* rec = a.grp + MOE_GRP_REC * (1 + item);
        const int e = rec[0], n = min(rec[1], 8);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int hr = t < n ? rec[2 + t] : 0;
            orow[t] = hr;
            xrow[t] = hr / a.topk;
            ow[t] = t < n ? __int_as_float(rec[10 + t]) : 0.f;
        }
        const long row0 = (long)e * 2 * a.I;
        if (a.Wgu.qtype == DSQ_Q4K) gateup_q_body<DSQ_Q4K>(a, a.Wgu, row0, a.I, i0, n, xrow, orow, ow, a.h);
        else gateup_q_body<DSQ_Q8_0>(a, a.Wgu, row0, a.I, i0, n, xrow, orow, ow, a.h);
    } else {
        if (i0 >= a.Is) return;
#pragma unroll
        for (int t = 0; t < 8; ++t) xrow[t] = orow[t] = t;
        if (a.sWgu.qtype == DSQ_Q4K) gateup_q_body<DSQ_Q4K>(a, a.sWgu, 0, a.Is, i0, a.T, xrow, orow, nullptr, a.hs);
        else gateup_q_body<DSQ_Q8_0>(a, a.sWgu, 0, a.Is, i0, a.T, xrow, orow, nullptr, a.hs);
    }
}

// ------------------------------------------------------------------ down + combine + residual
constexpr int QD_R = 4;  // output rows per block

// one item (an expert group or the shared expert): acc[r][t] += W[row0 + r][:] . hsrc[hr[t]][:] for the
// tokens t with hr[t] >= 0
template <int QT>
__device__ __forceinline__ void down_q_item(const QMat& m, long row0, int rmax, int in_dim, const float* hsrc,
                                            const int* hr, float (*acc)[8]) {
    const int lane = threadIdx.x & 63;
    const int iters = qrow_iters<QT>(in_dim);
    for (int it = 0; it < iters; ++it) {
        float w[QD_R][8];
        int oa = 0, ob = 0;
        bool ok = false;
#pragma unroll
        for (int r = 0; r < QD_R; ++r) ok = qrow_unpack<QT>(m, row0 + min(r, rmax), in_dim, it, lane, w[r], oa, ob);
        if (ok) {
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                if (hr[t] >= 0) {
                    float xv[8];
                    ld_x8q(hsrc + (long)hr[t] * in_dim, oa, ob, xv);
#pragma unroll
                    for (int r = 0; r < QD_R; ++r)
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[r][t] = fmaf(xv[j], w[r][j], acc[r][t]);
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void moe_down_q_kernel(MoeQArgs a) {
    WaveSpan span_(a.span);
    __shared__ float red[4][QD_R][8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * QD_R;
    const int rmax = min(QD_R - 1, a.H - 1 - r0);  // rows past H repeat the last one (never written)
    float acc[QD_R][8];
#pragma unroll
    for (int r = 0; r < QD_R; ++r)
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[r][t] = 0.f;
    const int ng = min(a.grp[0], a.slots);
    const int items = ng + (a.Is > 0 ? 1 : 0);
    for (int item = wave; item < items; item += 4) {
        int hr[8];
        if (item < ng) {
            const int* rec = a.grp + MOE_GRP_REC * (1 + item);
            const int e = rec[0], n = min(rec[1], 8);
#pragma unroll
            for (int t = 0; t < 8; ++t) hr[t] = -1;
            for (int k = 0; k < n; ++k) {
                const int row = rec[2 + k], tk = row / a.topk;
#pragma unroll
                for (int t = 0; t < 8; ++t)
                    if (t == tk) hr[t] = row;
            }
            const long row0 = (long)e * a.H + r0;
            if (a.Wd.qtype == DSQ_Q4K) down_q_item<DSQ_Q4K>(a.Wd, row0, rmax, a.I, a.h, hr, acc);
            else down_q_item<DSQ_Q8_0>(a.Wd, row0, rmax, a.I, a.h, hr, acc);
        } else {
#pragma unroll
            for (int t = 0; t < 8; ++t) hr[t] = t < a.T ? t : -1;
            if (a.sWd.qtype == DSQ_Q4K) down_q_item<DSQ_Q4K>(a.sWd, r0, rmax, a.Is, a.hs, hr, acc);
            else down_q_item<DSQ_Q8_0>(a.sWd, r0, rmax, a.Is, a.hs, hr, acc);
        }
    }
#pragma unroll
    for (int r = 0; r < QD_R; ++r)
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const float v = wave_sum(acc[r][t]);
            if (lane == 0) red[wave][r][t] = v;
        }
    __syncthreads();
    const int r = threadIdx.x >> 3, t = threadIdx.x & 7;
    if (r < QD_R && r0 + r < a.H && t < a.T) {
        const float v = ((red[0][r][t] + red[1][r][t]) + red[2][r][t]) + red[3][r][t];
        float* o = a.out + (long)t * a.H + r0 + r;
        *o = *o + v;
    }
}

void check_qmat(const QMat& m, long in_dim, const char* what) {
    if (!m.q || !dsq_packed_ok(m.qtype, in_dim) || (m.qtype == DSQ_Q8_0 && !m.d))
        throw std::runtime_error(std::string("EINVAL: packed ") + what + " is not a Q4_K / Q8_0 table of this width");
}

}  // namespace

// ------------------------------------------------------------------ host side
bool dsq_packed_ok(int qtype, long in_dim) {
    if (in_dim <= 0) return false;
    if (qtype == DSQ_Q4K) return in_dim % 256 == 0;
    if (qtype == DSQ_Q8_0) return in_dim % 32 == 0;
    return false;
}

size_t dsq_packed_bytes(int qtype, long rows, long in_dim) {
    if (!dsq_packed_ok(qtype, in_dim) || rows <= 0) return 0;
    if (qtype == DSQ_Q4K) return (size_t)rows * (in_dim / 256) * 144;
    return (size_t)rows * in_dim + (size_t)rows * (in_dim / 32) * 2;
}

QMat dsq_packed_view(int qtype, const void* packed, long rows, long in_dim) {
    QMat m;
    m.qtype = qtype;
    m.q = packed;
    if (qtype == DSQ_Q8_0) m.d = reinterpret_cast<const uint8_t*>(packed) + (size_t)rows * in_dim;
    return m;
}

void launch_dsq_repack(const QMat& dst, long dst_row0, const void* payload, long rows, long in_dim, hipStream_t s) {
    if (!dsq_packed_ok(dst.qtype, in_dim)) throw std::runtime_error("EINVAL: repack needs Q4_K / Q8_0 rows of whole blocks");
    if (rows <= 0) return;
    if (dst.qtype == DSQ_Q4K) {
        const size_t rb = (size_t)(in_dim / 256) * 144;
        uint8_t* q = const_cast<uint8_t*>(reinterpret_cast<const uint8_t*>(dst.q)) + (size_t)dst_row0 * rb;
        if (hipMemcpyAsync(q, payload, (size_t)rows * rb, hipMemcpyDeviceToDevice, s) != hipSuccess)
            throw std::runtime_error("EDEVICE: packed Q4_K copy failed");
        return;
    }
    const long nb = rows * (in_dim / 32);
    uint8_t* q = const_cast<uint8_t*>(reinterpret_cast<const uint8_t*>(dst.q)) + (size_t)dst_row0 * in_dim;
    uint16_t* d = const_cast<uint16_t*>(reinterpret_cast<const uint16_t*>(dst.d)) + (size_t)dst_row0 * (in_dim / 32);
    const long blocks = std::min<long>((nb * 32 + 255) / 256, 65536);
    hipLaunchKernelGGL(dsq_repack_q8_0_kernel, dim3((unsigned)blocks), dim3(256), 0, s,
                       reinterpret_cast<const uint8_t*>(payload), nb, q, d);
}

void launch_dsq_rows_dot(const QMat& m, long rows, long in_dim, int T, const float* x, float* y, hipStream_t s) {
    check_qmat(m, in_dim, "matrix");
    if (T < 1 || T > 8 || rows <= 0) throw std::runtime_error("EINVAL: rows_dot takes 1..8 token rows");
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (m.qtype == DSQ_Q4K) hipLaunchKernelGGL(dsq_rows_dot_kernel<DSQ_Q4K>, grid, dim3(256), 0, s, m, rows, (int)in_dim, T, x, y);
    else hipLaunchKernelGGL(dsq_rows_dot_kernel<DSQ_Q8_0>, grid, dim3(256), 0, s, m, rows, (int)in_dim, T, x, y);
}

bool moe_q_ok(const MoeQArgs& a) {
    if (a.T < 1 || a.T > 8 || a.topk < 1 || a.topk > 8 || a.T * a.topk > 64 || a.slots < 1) return false;
    if (!a.x || !a.h || !a.out || !a.grp) return false;
    if (!a.Wgu.q || !a.Wd.q || !dsq_packed_ok(a.Wgu.qtype, a.H) || !dsq_packed_ok(a.Wd.qtype, a.I)) return false;
    if (a.Is > 0 && (!a.hs || !a.sWgu.q || !a.sWd.q || !dsq_packed_ok(a.sWgu.qtype, a.H) || !dsq_packed_ok(a.sWd.qtype, a.Is)))
        return false;
    return true;
}

void launch_moe_gateup_q(const MoeQArgs& a, hipStream_t s) {
    if (!moe_q_ok(a)) throw std::runtime_error("EINVAL: packed decode MoE outside its range");
    check_qmat(a.Wgu, a.H, "gate|up");
    if (a.Is > 0) check_qmat(a.sWgu, a.H, "shared gate|up");
    const int rows = std::max(a.I, a.Is), per_block = 4 * QG_RW;
    const dim3 grid((unsigned)((rows + per_block - 1) / per_block), (unsigned)(a.slots + (a.Is > 0 ? 1 : 0)));
    DSOCR_LAUNCH(moe_gateup_q_kernel, grid, dim3(256), 0, s, a);
}

void launch_moe_down_q(const MoeQArgs& a, hipStream_t s) {
    if (!moe_q_ok(a)) throw std::runtime_error("EINVAL: packed decode MoE outside its range");
    check_qmat(a.Wd, a.I, "down");
    if (a.Is > 0) check_qmat(a.sWd, a.Is, "shared down");
    const dim3 grid((unsigned)((a.H + QD_R - 1) / QD_R));
    DSOCR_LAUNCH(moe_down_q_kernel, grid, dim3(256), 0, s, a);
}

}  // namespace dsocr
