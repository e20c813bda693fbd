// Integer-dot decode MoE from packed DSQ blocks (DSOCR_LOAD_PACKED_INT8_DOT) for T = 1..8 tokens: the
// activations are quantised to 8-bit blocks (Q8_K for Q4_K rows, Q8_0 for Q8_0 rows, the ggml reference
// quantisers) and every block dot is taken in int32 by v_dot4c_i32_i8 — one instruction per four weights
// per token.  A Q4_K quant word masked with 0x0F0F0F0F is already four int8 operands, so no weight is ever
// rebuilt as a float.  Contract: DESIGN.md section 4.4.2; the packed tables are decode_q.hip's (QMat).
//
// Launches of one layer (4: two quantisers, gate/up, down; the records are the router launch's, MOE_GRP_*):
//   q8_quantize     one wave per 256 activations (a Q8_K block, or eight Q8_0 blocks), 4 per lane; the codes,
//                   the block scales d and (Q8_K) the 32-value code sums bs go to planes in global memory.
//                   Once over xn before gate/up, once over h and hs before down.
//   moe_gateup_qdot grid (row chunks, expert slots + shared).  The block stages its group's code rows in LDS
//                   once; every 8 lanes own one gate row and its up row, so a wave streams 8 row pairs.
//   moe_down_qdot   one block per 8 output rows; its 4 waves split the layer's items (expert groups + the
//                   shared expert), each staging an item's code rows in a wave-private LDS region; the
//                   partial sums meet in LDS and are added to the residual stream in a fixed order.
//
// Row walk (qdot_rows).  Lane k of an 8-lane group reads 16 bytes of the row per step (nontemporal dwordx4).
//   Q4_K  a step is one super-block: the 16-byte header {d, dmin, scales} and quant bytes [16k, 16k + 16),
//         whose low nibbles are values 64c + 16hh + b and high nibbles values 64c + 32 + 16hh + b (c = k >> 1,
//         hh = k & 1).  In LDS the 16-byte code granules of a block are stored with the two low bits of their
//         index swapped, so the lane's low and high codes are the 32 contiguous bytes at 32k and the eight
//         lanes of a group read 256 contiguous bytes: no bank conflict; the 8 groups read the same addresses.
//         Per token: 8 dot4, then p = sc_2c * isum_lo + sc_2c+1 * isum_hi (int32).  The 8 x 8 (lane, token)
//         partials are reduced transposed on DPP (7 exchanges) so that lane k ends with token k's exact
//         sum S1 = sum_j sc_j isum_j; it takes S2 = sum_j m_j bs_j from the staged bs plane and adds
//         d_x * (d_w * S1 - dmin_w * S2) to its one f32 accumulator.  At the row's end lane k holds token k:
//         no reduction at all.
//   Q8_0  a step is 128 values (4 blocks, 2 lanes each).  Per token 4 dot4; one DPP exchange leaves the even
//         lane with the block's isum of tokens 0..3 and the odd lane with tokens 4..7; acc += (d_w * d_x) * isum.
//         At the row's end the 4 block slots are summed by a quad DPP and a ds_swizzle (xor 4).
// Integer accumulators per lane: 8 per row stream (16 in gate/up, 8 in down), f32 accumulators 1 or 4 per stream.
#include <hip/hip_fp16.h>

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "dev_common.hpp"
#include "dsq_decode.hpp"
#include "kernels.hpp"

namespace dsocr {

namespace {

__device__ __forceinline__ int dot4(uint32_t a, uint32_t b, int c) {
    return __builtin_amdgcn_sdot4((int)a, (int)b, c, false);
}
__device__ __forceinline__ int dot16(const uint4 a, const uint4 b) {
    return dot4(a.w, b.w, dot4(a.z, b.z, dot4(a.y, b.y, dot4(a.x, b.x, 0))));
}

// ------------------------------------------------------------------ activation quantiser
struct QuantJob {
    const float* x = nullptr;
    int rows = 0, in_dim = 0, kind = 0;  // kind: the weight table's qtype (DSQ_Q4K -> Q8_K, DSQ_Q8_0 -> Q8_0)
    Q8Planes o;
};

// max over the lanes of an 8-lane group
__device__ __forceinline__ float group8_max(float v) {
    v = fmaxf(v, dpp_f<DPP_QUAD_XOR1>(0.f, v));
    v = fmaxf(v, dpp_f<DPP_QUAD_XOR2>(0.f, v));
    return fmaxf(v, dpp_f<DPP_ROW_HALF_MIRROR>(0.f, v));
}

__device__ __forceinline__ uint32_t pack4(const int* q) {
    return (uint32_t)(q[0] & 0xFF) | ((uint32_t)(q[1] & 0xFF) << 8) | ((uint32_t)(q[2] & 0xFF) << 16) |
           ((uint32_t)(q[3] & 0xFF) << 24);
}

__global__ __launch_bounds__(256) void q8_quantize_kernel(QuantJob j0, QuantJob j1) {
    const int lane = threadIdx.x & 63;
    long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long w0 = (long)j0.rows * ((j0.in_dim + 255) >> 8);
    const bool second = w >= w0;
    const QuantJob& j = second ? j1 : j0;
    if (second) w -= w0;
    const int per_row = (j.in_dim + 255) >> 8;
    if (w >= (long)j.rows * per_row) return;
    const int row = (int)(w / per_row), e0 = (int)(w % per_row) * 256 + lane * 4;
    const bool in = e0 < j.in_dim;  // (Q8_0 rows of whole 32-blocks: a lane's 4 values are all in or all out)
    float x[4] = {0.f, 0.f, 0.f, 0.f};
    if (in) {
        const float4 v = *reinterpret_cast<const float4*>(j.x + (long)row * j.in_dim + e0);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    }
    int q[4];
    if (j.kind == DSQ_Q4K) {
        // Q8_K: the signed element of largest magnitude, the first on ties (key: element index, then sign)
        float bv = fabsf(x[0]);
        int bi = 0;
#pragma unroll
        for (int i = 1; i < 4; ++i)
            if (fabsf(x[i]) > bv) { bv = fabsf(x[i]); bi = i; }
        bi = ((lane * 4 + bi) << 1) | (x[bi] < 0.f ? 1 : 0);
        wave_argmax(bv, bi);
        const float mx = (bi & 1) ? -bv : bv;
        float d = 0.f;
        q[0] = q[1] = q[2] = q[3] = 0;
        if (bv != 0.f) {
            const float iscale = __fdiv_rn(-128.f, mx);
#pragma unroll
            for (int i = 0; i < 4; ++i) q[i] = min(127, (int)rintf(__fmul_rn(iscale, x[i])));
            d = __fdiv_rn(1.f, iscale);
        }
        int s = (q[0] + q[1]) + (q[2] + q[3]);  // 32-value sums: 8 lanes
        s += dpp_i<DPP_QUAD_XOR1>(0, s);
        s += dpp_i<DPP_QUAD_XOR2>(0, s);
        s += dpp_i<DPP_ROW_HALF_MIRROR>(0, s);
        const long blk = (long)row * per_row + e0 / 256;
        if (lane == 0) j.o.d[blk] = d;
        if ((lane & 7) == 0) j.o.bs[blk * 8 + (lane >> 3)] = (int16_t)s;
    } else {
        const float amax = group8_max(fmaxf(fmaxf(fabsf(x[0]), fabsf(x[1])), fmaxf(fabsf(x[2]), fabsf(x[3]))));
        const float d = __fdiv_rn(amax, 127.f);
        const float id = d != 0.f ? __fdiv_rn(1.f, d) : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = (int)roundf(__fmul_rn(x[i], id));
        // d as f16 (RNE), held widened
        if (in && (lane & 7) == 0) j.o.d[(long)row * (j.in_dim >> 5) + (e0 >> 5)] = f16_bits_to_f32(to_f16_rne(d));
    }
    if (in) *reinterpret_cast<uint32_t*>(j.o.q + (long)row * j.in_dim + e0) = pack4(q);
}

// ------------------------------------------------------------------ code rows in LDS
// One item's region: codes [8][in_dim] | d [8][nblk] f32 | bs [8][in_dim / 32] i16 (Q4_K only); slot t of 8
// holds global code row rows[t] (< 0: absent, left unwritten and never read).
__host__ __device__ inline int qdot_nblk(int qt, int in_dim) { return qt == DSQ_Q4K ? in_dim >> 8 : in_dim >> 5; }
__host__ __device__ inline size_t qdot_item_lds(int qt, int in_dim) {
    return (size_t)8 * in_dim + (size_t)8 * qdot_nblk(qt, in_dim) * 4 + (qt == DSQ_Q4K ? (size_t)8 * (in_dim >> 5) * 2 : 0);
}

template <int QT>
__device__ __forceinline__ void stage_codes(uint8_t* lds, const Q8Planes& p, const int* rows, int in_dim, int tid, int nthr) {
    const int gran = in_dim >> 4, nblk = qdot_nblk(QT, in_dim), nbs = in_dim >> 5;
    float* ld = reinterpret_cast<float*>(lds + 8 * in_dim);
    int16_t* lb = reinterpret_cast<int16_t*>(lds + 8 * in_dim + 8 * nblk * 4);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        if (rows[t] < 0) continue;
        const long r = rows[t];
        for (int g = tid; g < gran; g += nthr) {
            const uint4 v = *reinterpret_cast<const uint4*>(p.q + r * in_dim + 16 * g);
            const int gd = QT == DSQ_Q4K ? (g & ~3) | ((g & 1) << 1) | ((g >> 1) & 1) : g;
            *reinterpret_cast<uint4*>(lds + t * in_dim + 16 * gd) = v;
        }
        for (int b = tid; b < nblk; b += nthr) ld[t * nblk + b] = p.d[r * nblk + b];
        if (QT == DSQ_Q4K)
            for (int b = tid; b < nbs; b += nthr) lb[t * nbs + b] = p.bs[r * nbs + b];
    }
}

// ------------------------------------------------------------------ the row walk
// 8 x 8 transposed sum: lane k of every 8-lane group ends with sum over the group's lanes of v[k]
__device__ __forceinline__ int group8_transpose_sum(const int* v, int k) {
    int a[4], b[2];
    const bool h4 = k & 4, h2 = k & 2, h1 = k & 1;
#pragma unroll
    for (int u = 0; u < 4; ++u)  // partner 7 - k: the lanes with bit 2 clear keep tokens 0..3
        a[u] = (h4 ? v[4 + u] : v[u]) + dpp_i<DPP_ROW_HALF_MIRROR>(0, h4 ? v[u] : v[4 + u]);
#pragma unroll
    for (int u = 0; u < 2; ++u)  // partner k ^ 2
        b[u] = (h2 ? a[2 + u] : a[u]) + dpp_i<DPP_QUAD_XOR2>(0, h2 ? a[u] : a[2 + u]);
    return (h1 ? b[1] : b[0]) + dpp_i<DPP_QUAD_XOR1>(0, h1 ? b[0] : b[1]);
}

template <int QT>
struct RowAcc {
    float v[QT == DSQ_Q4K ? 1 : 4];
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (float& f : v) f = 0.f;
    }
};

// acc[r] += W[row[r]][:] . codes of the staged tokens (tmask: bit t = slot t present).  Q4_K: acc[r].v[0] is
// the sum of token (lane & 7); Q8_0: acc[r].v[u] is the partial of token 4 (lane & 1) + u over the lane's blocks.
template <int QT, int NR>
__device__ __forceinline__ void qdot_rows(const QMat& m, const long* row, int in_dim, const uint8_t* lds, int tmask,
                                          RowAcc<QT>* acc) {
    const int k = threadIdx.x & 7;
    const int nblk = qdot_nblk(QT, in_dim);
    const float* ld = reinterpret_cast<const float*>(lds + 8 * in_dim);
    if constexpr (QT == DSQ_Q4K) {
        const int16_t* lb = reinterpret_cast<const int16_t*>(lds + 8 * in_dim + 8 * nblk * 4);
        const bool mine = (tmask >> k) & 1;
        uint4 hdr[NR], qs[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const uint8_t* blk = reinterpret_cast<const uint8_t*>(m.q) + row[r] * nblk * 144;
            hdr[r] = ldg_nt16(blk);
            qs[r] = ldg_nt16(blk + 16 + 16 * k);
        }
        for (int sb = 0; sb < nblk; ++sb) {
            uint4 lo[NR], hi[NR];
            uint4 h[NR];
            int sc0[NR], sc1[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                h[r] = hdr[r];
                lo[r] = make_uint4(qs[r].x & 0x0F0F0F0Fu, qs[r].y & 0x0F0F0F0Fu, qs[r].z & 0x0F0F0F0Fu, qs[r].w & 0x0F0F0F0Fu);
                hi[r] = make_uint4((qs[r].x >> 4) & 0x0F0F0F0Fu, (qs[r].y >> 4) & 0x0F0F0F0Fu, (qs[r].z >> 4) & 0x0F0F0F0Fu,
                                   (qs[r].w >> 4) & 0x0F0F0F0Fu);
                if (sb + 1 < nblk) {  // the next super-block's loads fly over this one's arithmetic
                    const uint8_t* blk = reinterpret_cast<const uint8_t*>(m.q) + (row[r] * nblk + sb + 1) * 144;
                    hdr[r] = ldg_nt16(blk);
                    qs[r] = ldg_nt16(blk + 16 + 16 * k);
                }
                int mm;
                scale_min_k4_words(k & 6, h[r].y, h[r].z, h[r].w, sc0[r], mm);
                scale_min_k4_words((k & 6) + 1, h[r].y, h[r].z, h[r].w, sc1[r], mm);
            }
            int p[NR][8];
#pragma unroll
            for (int t = 0; t < 8; ++t) {
#pragma unroll
                for (int r = 0; r < NR; ++r) p[r][t] = 0;
                if ((tmask >> t) & 1) {
                    const uint8_t* c = lds + t * in_dim + sb * 256 + 32 * k;
                    const uint4 ca = *reinterpret_cast<const uint4*>(c), cb = *reinterpret_cast<const uint4*>(c + 16);
#pragma unroll
                    for (int r = 0; r < NR; ++r) p[r][t] = __mul24(sc0[r], dot16(lo[r], ca)) + __mul24(sc1[r], dot16(hi[r], cb));
                }
            }
            int4 b0 = make_int4(0, 0, 0, 0);
            float dx = 0.f;
            if (mine) {
                b0 = *reinterpret_cast<const int4*>(lb + k * (in_dim >> 5) + sb * 8);
                dx = ld[k * nblk + sb];
            }
            const int bw[4] = {b0.x, b0.y, b0.z, b0.w};
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const int s1 = group8_transpose_sum(p[r], k);
                int s2 = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    int sc, mj;
                    scale_min_k4_words(j, h[r].y, h[r].z, h[r].w, sc, mj);
                    const int bsj = (j & 1) ? (bw[j >> 1] >> 16) : (int)(int16_t)(bw[j >> 1] & 0xFFFF);
                    s2 += __mul24(mj, bsj);
                }
                const float dw = f16_bits_to_f32(h[r].x & 0xffffu), dmin = f16_bits_to_f32(h[r].x >> 16);
                const float blk = __fmul_rn(dx, __fsub_rn(__fmul_rn(dw, (float)s1), __fmul_rn(dmin, (float)s2)));
                if (mine) acc[r].v[0] = __fadd_rn(acc[r].v[0], blk);
            }
        }
    } else {
        const int steps = (in_dim + 127) >> 7;
        for (int it = 0; it < steps; ++it) {
            const int off = it * 128 + 16 * k;
            const bool in = off < in_dim;
            const int offc = in ? off : 0;
            uint4 q[NR];
            float dw[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                q[r] = ldg_nt16(reinterpret_cast<const uint8_t*>(m.q) + row[r] * in_dim + offc);
                dw[r] = f16_bits_to_f32(reinterpret_cast<const uint16_t*>(m.d)[row[r] * nblk + (offc >> 5)]);
            }
            int p[NR][8];
#pragma unroll
            for (int t = 0; t < 8; ++t) {
#pragma unroll
                for (int r = 0; r < NR; ++r) p[r][t] = 0;
                if ((tmask >> t) & 1) {
                    const uint4 ca = *reinterpret_cast<const uint4*>(lds + t * in_dim + offc);
#pragma unroll
                    for (int r = 0; r < NR; ++r) p[r][t] = dot16(q[r], ca);
                }
            }
            const bool odd = k & 1;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int tt = 4 * (k & 1) + u;
                const bool on = in && ((tmask >> tt) & 1);
                const float dx = on ? ld[tt * nblk + (offc >> 5)] : 0.f;
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    const int isum = (odd ? p[r][4 + u] : p[r][u]) + dpp_i<DPP_QUAD_XOR1>(0, odd ? p[r][u] : p[r][4 + u]);
                    const float blk = __fmul_rn(__fmul_rn(dw[r], dx), (float)isum);
                    if (on) acc[r].v[u] = __fadd_rn(acc[r].v[u], blk);
                }
            }
        }
    }
}

// Row-end hand-over: tok[t] (t < 8) valid on the lane out_lane(t) of the group
//   Q4_K  lane t holds token t;  Q8_0  lanes 0 / 1 hold tokens 0..3 / 4..7 after the block slots are summed
template <int QT>
__device__ __forceinline__ void row_finish(RowAcc<QT>& a) {
    if constexpr (QT == DSQ_Q8_0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float v = a.v[u];
            v = __fadd_rn(v, dpp_f<DPP_QUAD_XOR2>(0.f, v));
            v = __fadd_rn(v, __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), (4 << 10) | 0x1f)));
            a.v[u] = v;
        }
    }
}
// f(token, value) for every token this lane hands over
template <int QT, typename F>
__device__ __forceinline__ void row_tokens(const RowAcc<QT>& a, int k, F&& f) {
    if constexpr (QT == DSQ_Q4K) {
        f(k, a.v[0]);
    } else {
        if (k < 2)
#pragma unroll
            for (int u = 0; u < 4; ++u) f(4 * k + u, a.v[u]);
    }
}

// ------------------------------------------------------------------ y = codes . W^T (parity hook)
template <int QT>
__global__ __launch_bounds__(256) void dsq_rows_dot_q8_kernel(QMat m, long rows, int in_dim, int T, Q8Planes p, float* y) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    int src[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) src[t] = t < T ? t : -1;
    stage_codes<QT>(smem, p, src, in_dim, threadIdx.x, 256);
    __syncthreads();
    const int k = threadIdx.x & 7;
    const long r = (long)blockIdx.x * 32 + (threadIdx.x >> 3);
    const long row[1] = {r < rows ? r : rows - 1};
    RowAcc<QT> acc[1];
    acc[0].zero();
    qdot_rows<QT, 1>(m, row, in_dim, smem, (1 << T) - 1, acc);
    row_finish<QT>(acc[0]);
    row_tokens<QT>(acc[0], k, [&](int t, float v) {
        if (t < T && r < rows) y[(long)t * rows + r] = v;
    });
}

// ------------------------------------------------------------------ gate/up
// rec: the group's record (its h rows and routing weights), or null for the shared expert (h row = token)
template <int QT>
__device__ __forceinline__ void gateup_qdot_body(const MoeQArgs& a, const QMat& m, long row0, int rows_I, int n,
                                                 const int* xrow, const int* rec, float* hout, uint8_t* smem) {
    stage_codes<QT>(smem, a.qx, xrow, a.H, threadIdx.x, 256);
    __syncthreads();
    const int k = threadIdx.x & 7;
    const int i = blockIdx.x * 32 + (threadIdx.x >> 3);
    const int ic = min(i, rows_I - 1);
    const long row[2] = {row0 + ic, row0 + rows_I + ic};
    RowAcc<QT> acc[2];
    acc[0].zero();
    acc[1].zero();
    qdot_rows<QT, 2>(m, row, a.H, smem, (1 << n) - 1, acc);
    row_finish<QT>(acc[0]);
    row_finish<QT>(acc[1]);
    float us[4];
    int ui = 0;
    row_tokens<QT>(acc[1], k, [&](int, float v) { us[ui++] = v; });
    ui = 0;
    row_tokens<QT>(acc[0], k, [&](int t, float gs) {
        const float u = us[ui++];
        if (t < n && i < rows_I) {
            float hv = (gs / (1.0f + expf(-gs))) * u;  // silu (candle: x / (1 + exp(-x)))
            if (rec) hv = hv * __int_as_float(rec[10 + t]);
            hout[(long)(rec ? rec[2 + t] : t) * rows_I + i] = hv;
        }
    });
}

__global__ __launch_bounds__(256) void moe_gateup_qdot_kernel(MoeQArgs a) {
    WaveSpan span_(a.span);
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int item = blockIdx.y;
    int xrow[8];
    if (item < a.slots) {
        if (item >= a.grp[0] || blockIdx.x * 32 >= a.I) return;  // block-uniform, before any barrier
        const int* rec = a.grp + MOE_GRP_REC * (1 + item);
        const int e = rec[0], n = min(rec[1], 8);
#pragma unroll
        for (int t = 0; t < 8; ++t) xrow[t] = t < n ? rec[2 + t] / a.topk : -1;
        const long row0 = (long)e * 2 * a.I;
        if (a.Wgu.qtype == DSQ_Q4K) gateup_qdot_body<DSQ_Q4K>(a, a.Wgu, row0, a.I, n, xrow, rec, a.h, smem);
        else gateup_qdot_body<DSQ_Q8_0>(a, a.Wgu, row0, a.I, n, xrow, rec, a.h, smem);
    } else {
        if (blockIdx.x * 32 >= a.Is) return;
#pragma unroll
        for (int t = 0; t < 8; ++t) xrow[t] = t < a.T ? t : -1;
        if (a.sWgu.qtype == DSQ_Q4K) gateup_qdot_body<DSQ_Q4K>(a, a.sWgu, 0, a.Is, a.T, xrow, nullptr, a.hs, smem);
        else gateup_qdot_body<DSQ_Q8_0>(a, a.sWgu, 0, a.Is, a.T, xrow, nullptr, a.hs, smem);
    }
}

// ------------------------------------------------------------------ down + combine + residual
constexpr int QDOT_DR = 8;  // output rows per block (one per 8-lane group of every wave)

template <int QT>
__device__ __forceinline__ void down_qdot_item(const QMat& m, long row, int in_dim, const Q8Planes& p, const int* hr,
                                               uint8_t* lds, float (*red)[8]) {
    const int lane = threadIdx.x & 63, k = lane & 7, g = lane >> 3;
    int tmask = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) tmask |= hr[t] >= 0 ? 1 << t : 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();  // the previous item's reads of this wave's region and its sums are done
    stage_codes<QT>(lds, p, hr, in_dim, lane, 64);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    RowAcc<QT> acc[1];
    acc[0].zero();
    const long rows[1] = {row};
    qdot_rows<QT, 1>(m, rows, in_dim, lds, tmask, acc);
    row_finish<QT>(acc[0]);
    // the wave's own [row][token] partials: every (g, t) cell has one writer per item
    row_tokens<QT>(acc[0], k, [&](int t, float v) {
        if ((tmask >> t) & 1) red[g][t] = __fadd_rn(red[g][t], v);
    });
}

// the wave's share of the expert groups (items wave, wave + 4, ...)
template <int QT>
__device__ __forceinline__ void down_qdot_routed(const MoeQArgs& a, int ng, int wave, int r, uint8_t* lds, float (*red)[8]) {
    for (int item = wave; item < ng; item += 4) {
        const int* rec = a.grp + MOE_GRP_REC * (1 + item);
        const int e = rec[0], n = min(rec[1], 8);
        int hr[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) hr[t] = -1;
        for (int q = 0; q < n; ++q) {
            const int row = rec[2 + q], tk = row / a.topk;
#pragma unroll
            for (int t = 0; t < 8; ++t)
                if (t == tk) hr[t] = row;
        }
        down_qdot_item<QT>(a.Wd, (long)e * a.H + r, a.I, a.qh, hr, lds, red);
    }
}

__global__ __launch_bounds__(256) void moe_down_qdot_kernel(MoeQArgs a, int item_lds) {
    WaveSpan span_(a.span);
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ float red[4][QDOT_DR][8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * QDOT_DR;
    const int r = min(r0 + (lane >> 3), a.H - 1);  // rows past H repeat the last one (never written)
    red[wave][lane >> 3][lane & 7] = 0.f;
    uint8_t* lds = smem + (size_t)wave * item_lds;
    const int ng = min(a.grp[0], a.slots);
    if (a.Wd.qtype == DSQ_Q4K) down_qdot_routed<DSQ_Q4K>(a, ng, wave, r, lds, red[wave]);
    else down_qdot_routed<DSQ_Q8_0>(a, ng, wave, r, lds, red[wave]);
    if (a.Is > 0 && wave == (ng & 3)) {  // the shared expert: the item after the last group
        int hr[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) hr[t] = t < a.T ? t : -1;
        if (a.sWd.qtype == DSQ_Q4K) down_qdot_item<DSQ_Q4K>(a.sWd, r, a.Is, a.qhs, hr, lds, red[wave]);
        else down_qdot_item<DSQ_Q8_0>(a.sWd, r, a.Is, a.qhs, hr, lds, red[wave]);
    }
    __syncthreads();
    const int rr = threadIdx.x >> 3, t = threadIdx.x & 7;
    if (rr < QDOT_DR && r0 + rr < a.H && t < a.T) {
        const float v = ((red[0][rr][t] + red[1][rr][t]) + red[2][rr][t]) + red[3][rr][t];
        float* o = a.out + (long)t * a.H + r0 + rr;
        *o = *o + v;
    }
}

size_t planes_bytes(long rows, long in_dim) {
    auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
    return up((size_t)rows * in_dim) + up((size_t)rows * (in_dim / 32) * 4) + up((size_t)rows * (in_dim / 32) * 2);
}
Q8Planes planes_carve(uint8_t*& p, long rows, long in_dim) {
    auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
    Q8Planes o;
    o.q = reinterpret_cast<int8_t*>(p);
    p += up((size_t)rows * in_dim);
    o.d = reinterpret_cast<float*>(p);
    p += up((size_t)rows * (in_dim / 32) * 4);
    o.bs = reinterpret_cast<int16_t*>(p);
    p += up((size_t)rows * (in_dim / 32) * 2);
    return o;
}

QuantJob quant_job(const float* x, int rows, int in_dim, int kind, const Q8Planes& o) {
    QuantJob j;
    j.x = x; j.rows = rows; j.in_dim = in_dim; j.kind = kind; j.o = o;
    return j;
}
void launch_quant_jobs(const QuantJob& j0, const QuantJob& j1, hipStream_t s) {
    const long waves = (long)j0.rows * ((j0.in_dim + 255) / 256) + (long)j1.rows * ((j1.in_dim + 255) / 256);
    if (waves <= 0) return;
    hipLaunchKernelGGL(q8_quantize_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, j0, j1);
}

size_t down_item_lds(const MoeQArgs& a) {
    size_t b = qdot_item_lds(a.Wd.qtype, a.I);
    if (a.Is > 0) b = std::max(b, qdot_item_lds(a.sWd.qtype, a.Is));
    return (b + 15) & ~(size_t)15;
}

}  // namespace

// ------------------------------------------------------------------ host side
size_t moe_qdot_ws_bytes(int T, int topk, int H, int I, int Is) {
    return planes_bytes(T, H) + planes_bytes((long)T * topk, I) + (Is > 0 ? planes_bytes(T, Is) : 0);
}

void moe_qdot_planes(void* ws, int T, int topk, int H, int I, int Is, Q8Planes* qx, Q8Planes* qh, Q8Planes* qhs) {
    uint8_t* p = reinterpret_cast<uint8_t*>(ws);
    *qx = planes_carve(p, T, H);
    *qh = planes_carve(p, (long)T * topk, I);
    *qhs = Is > 0 ? planes_carve(p, T, Is) : Q8Planes();
}

void launch_q8_quantize(int kind, int rows, int in_dim, const float* x, const Q8Planes& o, hipStream_t s) {
    if (!dsq_packed_ok(kind, in_dim) || rows <= 0 || !x || !o.q || !o.d || (kind == DSQ_Q4K && !o.bs))
        throw std::runtime_error("EINVAL: q8_quantize takes Q8_K rows of whole 256-blocks or Q8_0 rows of whole 32-blocks");
    launch_quant_jobs(quant_job(x, rows, in_dim, kind, o), QuantJob(), s);
}

void launch_dsq_rows_dot_q8(const QMat& m, long rows, long in_dim, int T, const Q8Planes& p, float* y, hipStream_t s) {
    if (!m.q || !dsq_packed_ok(m.qtype, in_dim) || (m.qtype == DSQ_Q8_0 && !m.d))
        throw std::runtime_error("EINVAL: packed matrix is not a Q4_K / Q8_0 table of this width");
    if (T < 1 || T > 8 || rows <= 0 || !p.q || !p.d || (m.qtype == DSQ_Q4K && !p.bs) || !y)
        throw std::runtime_error("EINVAL: rows_dot_q8 takes 1..8 code rows");
    const size_t lds = qdot_item_lds(m.qtype, (int)in_dim);
    if (lds > 64 * 1024) throw std::runtime_error("EINVAL: rows_dot_q8 row too wide for LDS staging");
    const dim3 grid((unsigned)((rows + 31) / 32));
    if (m.qtype == DSQ_Q4K) hipLaunchKernelGGL(dsq_rows_dot_q8_kernel<DSQ_Q4K>, grid, dim3(256), lds, s, m, rows, (int)in_dim, T, p, y);
    else hipLaunchKernelGGL(dsq_rows_dot_q8_kernel<DSQ_Q8_0>, grid, dim3(256), lds, s, m, rows, (int)in_dim, T, p, y);
}

bool moe_qdot_ok(const MoeQArgs& a) {
    if (!moe_q_ok(a) || !a.qx.q || !a.qh.q || (a.Is > 0 && !a.qhs.q)) return false;
    if (a.Is > 0 && a.sWgu.qtype != a.Wgu.qtype) return false;  // xn is quantised once, to one block kind
    return qdot_item_lds(a.Wgu.qtype, a.H) <= 64 * 1024 && (a.Is <= 0 || qdot_item_lds(a.sWgu.qtype, a.H) <= 64 * 1024) &&
           4 * down_item_lds(a) + sizeof(float) * 4 * QDOT_DR * 8 <= 64 * 1024;
}

void launch_moe_gateup_qdot(const MoeQArgs& a, hipStream_t s) {
    if (!moe_qdot_ok(a)) throw std::runtime_error("EINVAL: integer-dot decode MoE outside its range");
    launch_quant_jobs(quant_job(a.x, a.T, a.H, a.Wgu.qtype, a.qx), QuantJob(), s);
    const size_t lds = qdot_item_lds(a.Wgu.qtype, a.H);
    const int rows = std::max(a.I, a.Is);
    const dim3 grid((unsigned)((rows + 31) / 32), (unsigned)(a.slots + (a.Is > 0 ? 1 : 0)));
    DSOCR_LAUNCH(moe_gateup_qdot_kernel, grid, dim3(256), lds, s, a);
}

void launch_moe_down_qdot(const MoeQArgs& a, hipStream_t s) {
    if (!moe_qdot_ok(a)) throw std::runtime_error("EINVAL: integer-dot decode MoE outside its range");
    launch_quant_jobs(quant_job(a.h, a.T * a.topk, a.I, a.Wd.qtype, a.qh),
                      a.Is > 0 ? quant_job(a.hs, a.T, a.Is, a.sWd.qtype, a.qhs) : QuantJob(), s);
    const int item = (int)down_item_lds(a);
    const dim3 grid((unsigned)((a.H + QDOT_DR - 1) / QDOT_DR));
    DSOCR_LAUNCH(moe_down_qdot_kernel, grid, dim3(256), (size_t)4 * item, s, a, item);
}

}  // namespace dsocr
