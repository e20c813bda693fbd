// Decode MoE: gate/up and down in their 2 / slot / shared / mix / grouped forms and the layer dispatch.
#include "decode_common.hpp"

namespace dsocr {

// One wave: greedy top-k of E router logits (softmax or sigmoid scores, stable: ties -> lower
// expert id, block.rs:1271-1301); returns the `want`-th pick (e, its score) and the sum of the
// top-k scores (for norm_topk_prob).  Results are wave-uniform.
__device__ __forceinline__ void topk_select(const float* lg, int E, int K, int softmax_scoring, int want, int& e_out,
                                            float& v_out, float& wsum) {
    const int lane = threadIdx.x & 63;
    float sc[4];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = lane + 64 * j;
        sc[j] = e < E ? lg[e] : -INFINITY;
        mx = fmaxf(mx, sc[j]);
    }
    if (softmax_scoring) {
        mx = wave_max(mx);
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = lane + 64 * j;
            sc[j] = e < E ? expf(sc[j] - mx) : 0.f;
            sum += sc[j];
        }
        sum = wave_sum(sum);
#pragma unroll
        for (int j = 0; j < 4; ++j) sc[j] = (lane + 64 * j) < E ? sc[j] / sum : -INFINITY;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) sc[j] = (lane + 64 * j) < E ? 1.0f / (1.0f + expf(-sc[j])) : -INFINITY;
    }
    wsum = 0.f;
    e_out = 0;
    v_out = 0.f;
    for (int k = 0; k < K; ++k) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = lane + 64 * j;
            if (e < E && (sc[j] > bv || (sc[j] == bv && e < bi))) { bv = sc[j]; bi = e; }
        }
        wave_argmax(bv, bi);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (lane + 64 * j == bi) sc[j] = -INFINITY;
        wsum += bv;
        if (k == want) { e_out = bi; v_out = bv; }
    }
}

// ------------------------------------------------------------------ MoE gate/up (routed + shared)
// blocks [0, slots*units_r): routed expert active[s] (rows I); the rest: the shared
// experts (rows Is, all T tokens).  h = silu(x.Wg) * (x.Wu) with x = rmsnorm(X) staged in
// LDS; routed rows are pre-multiplied by their routing weight (aw, sorted order) so that
// the down kernel reduces every expert of a token into ONE accumulator.
template <typename WT, int MT>
__global__ __launch_bounds__(256) void moe_gateup2_kernel(MoeDec2Args a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int RB = 2, U = 3;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int units_r = (a.I + 4 * RB - 1) / (4 * RB);
    const int bid = blockIdx.x;
    __shared__ int sel_e;
    __shared__ float sel_w;
    const WT* Wg;
    const WT* Wu;
    int rows_I, u, p0, cnt;
    float* hout;
    const int* rowmap;
    const float* xb = a.x;    // rows come from xb[rowmap[p]] (grouped) or xb[t0 + m]
    float slot_w = 1.f;       // slot mode: routing weight of this (token, k) slot
    constexpr int XR = 2;
    const bool fast = a.K <= XR * 4 * 256;
    XRegs<MT, XR> xr;
    bool xpre = false;        // slot mode loads its activation row before routing itself
    if (bid < a.slots * units_r && a.slot_mode) {
        // slot mode (T <= 8): block (s = t*topk + k, unit) picks its own expert from the router
        // logits (the same greedy top-k as moe_route), no grouping pass
        const int sl = bid / units_r, t = sl / a.topk, k = sl % a.topk;
        u = bid % units_r;
        if (fast) {
            xload<MT, XR>(xr, a.x + (long)t * a.K, a.K, nullptr, 1, a.K, a.norm_w);
            xpre = true;
        }
        if (wave == 0) {
            int e;
            float v, wsum;
            topk_select(a.logits + (long)t * a.E, a.E, a.topk, a.softmax_scoring, k, e, v, wsum);
            if (a.topk > 1 && a.norm_topk) v = v / (wsum + 1e-20f);
            if (a.scaling != 1.0f) v = v * a.scaling;
            if (lane == 0) {
                sel_e = e;
                sel_w = v;
                if (u == 0) { a.ids_out[sl] = e; a.w_out[sl] = v; }
            }
        }
        __syncthreads();
        const int e = sel_e;
        slot_w = sel_w;
        rows_I = a.I;
        Wg = reinterpret_cast<const WT*>(a.Wgu) + (long)e * 2 * a.I * a.K;
        Wu = Wg + (long)a.I * a.K;
        p0 = sl;
        cnt = 1;
        hout = a.h;
        rowmap = nullptr;
        xb = a.x + (long)t * a.K;
    } else if (bid < a.slots * units_r) {
        const int s = bid / units_r;
        if (s >= *a.n_active) return;
        const int e = a.active[s];
        u = bid % units_r;
        rows_I = a.I;
        Wg = reinterpret_cast<const WT*>(a.Wgu) + (long)e * 2 * a.I * a.K;
        Wu = Wg + (long)a.I * a.K;
        p0 = a.eoff[e];
        cnt = a.eoff[e + 1] - p0;
        hout = a.h;
        rowmap = a.arow;
    } else {
        if (!a.sWgu) return;
        u = bid - a.slots * units_r;
        rows_I = a.Is;
        Wg = reinterpret_cast<const WT*>(a.sWgu);
        Wu = Wg + (long)a.Is * a.K;
        p0 = 0;
        cnt = a.T;
        hout = a.hs;
        rowmap = nullptr;
    }
    const int i0 = (u * 4 + wave) * RB;
    const bool active = i0 < rows_I;
    const int chunks = a.K >> 3;
    const float* xs = smem + XS_RED;
    for (int t0 = 0; t0 < cnt; t0 += MT) {
        const int tn = min(MT, cnt - t0);
        if (fast && !xpre) {
            if (rowmap) xload<MT, XR>(xr, xb, a.K, rowmap + p0 + t0, tn, a.K, a.norm_w);
            else xload<MT, XR>(xr, xb + (long)t0 * a.K, a.K, nullptr, tn, a.K, a.norm_w);
        }
        xpre = false;
        uint4 qg[U][RB], qu[U][RB];
#pragma unroll
        for (int uu = 0; uu < U; ++uu) {
            const int c = uu * 64 + lane;
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int i = min(i0 + r, rows_I - 1);
                const int cc = min(c, chunks - 1);
                qg[uu][r] = ldg_nt16(Wg + (long)i * a.K + (cc << 3));
                qu[uu][r] = ldg_nt16(Wu + (long)i * a.K + (cc << 3));
            }
        }
        if (t0 > 0) __syncthreads();  // previous group's LDS rows fully consumed
        if (fast) xstage<MT, XR>(xr, tn, a.K, a.norm_w != nullptr, a.eps, smem);
        else if (rowmap) stage_rows(xb, a.K, rowmap + p0 + t0, tn, a.K, a.norm_w, a.eps, smem);
        else stage_rows(xb + (long)t0 * a.K, a.K, nullptr, tn, a.K, a.norm_w, a.eps, smem);
        if (!active) continue;
        float ag[RB][MT], au[RB][MT];
#pragma unroll
        for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int m = 0; m < MT; ++m) { ag[r][m] = 0.f; au[r][m] = 0.f; }
        for (int base = 0;;) {
#pragma unroll
            for (int uu = 0; uu < U; ++uu) {
                const int c = base + uu * 64 + lane;
                if (c >= chunks) continue;
#pragma unroll
                for (int r = 0; r < RB; ++r) {
                    float wg[8], wu[8];
                    unpack8<WT>(qg[uu][r], wg);
                    unpack8<WT>(qu[uu][r], wu);
#pragma unroll
                    for (int m = 0; m < MT; ++m) {
                        if (m < tn) {
                            float xv[8];
                            ld_x8(xs + m * a.K + (c << 3), xv);
#pragma unroll
                            for (int j = 0; j < 8; ++j) {
                                ag[r][m] = fmaf(xv[j], wg[j], ag[r][m]);
                                au[r][m] = fmaf(xv[j], wu[j], au[r][m]);
                            }
                        }
                    }
                }
            }
            base += 64 * U;
            if (base >= chunks) break;
#pragma unroll
            for (int uu = 0; uu < U; ++uu) {
                const int c = base + uu * 64 + lane;
#pragma unroll
                for (int r = 0; r < RB; ++r) {
                    const int i = min(i0 + r, rows_I - 1);
                    const int cc = min(c, chunks - 1);
                    qg[uu][r] = ldg_nt16(Wg + (long)i * a.K + (cc << 3));
                    qu[uu][r] = ldg_nt16(Wu + (long)i * a.K + (cc << 3));
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const float gs = wave_sum(ag[r][m]);
                const float us = wave_sum(au[r][m]);
                const int i = i0 + r;
                if (lane == 0 && m < tn && i < rows_I) {
                    float hv = (gs / (1.0f + expf(-gs))) * us;  // silu (candle: x / (1 + exp(-x)))
                    if (rowmap) hv = hv * a.aw[p0 + t0 + m];
                    else if (hout == a.h) hv = hv * slot_w;
                    hout[(long)(p0 + t0 + m) * rows_I + i] = hv;
                }
            }
    }
}

// Slot-mode gate/up (T <= 8, the decode configurations): straight-line code so that the
// in-order vmcnt accounting stays exact (activation loads -> [routing] -> weight stream ->
// stage -> FMA).  Blocks [0, T*topk*units_r) are (token, pick) slots that route themselves;
// the rest are the shared experts over all T tokens (MT >= T).
template <typename WT, int MT, int RB = 2>
__device__ __forceinline__ void gateup_slot_body(const MoeDec2Args& a, const int bid, float* smem) {
    __shared__ int sel_e;
    __shared__ float sel_w;
    constexpr int U = 3, XR = 2;  // K <= 1536
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int units_r = (a.I + 4 * RB - 1) / (4 * RB);
    const bool routed = bid < a.slots * units_r;
    if (!routed && !a.sWgu) return;
    const int sl = routed ? bid / units_r : 0;
    const int t = sl / max(1, a.topk), k = sl % max(1, a.topk);
    const int u = routed ? bid % units_r : bid - a.slots * units_r;
    const int M = routed ? 1 : a.T;
    XRegs<MT, XR> xr;
    xload<MT, XR>(xr, a.x + (routed ? (long)t * a.K : 0L), a.K, nullptr, M, a.K, a.norm_w);
    if (routed) {
        if (wave == 0) {
            int e;
            float v, wsum;
            topk_select(a.logits + (long)t * a.E, a.E, a.topk, a.softmax_scoring, k, e, v, wsum);
            if (a.topk > 1 && a.norm_topk) v = v / (wsum + 1e-20f);
            if (a.scaling != 1.0f) v = v * a.scaling;
            if (lane == 0) {
                sel_e = e;
                sel_w = v;
                if (u == 0) {
                    a.ids_out[sl] = e;
                    a.w_out[sl] = v;
                }
            }
        }
        __syncthreads();
    }
    const int rows_I = routed ? a.I : a.Is;
    const int e_sel = sel_e;
    const WT* Wg = routed ? reinterpret_cast<const WT*>(a.Wgu) + (long)e_sel * 2 * a.I * a.K
                          : reinterpret_cast<const WT*>(a.sWgu);
    const WT* Wu = Wg + (long)rows_I * a.K;
    const int i0 = (u * 4 + wave) * RB;
    const bool active = i0 < rows_I;
    const int chunks = a.K >> 3;
    uint4 qg[U][RB], qu[U][RB];
#pragma unroll
    for (int uu = 0; uu < U; ++uu) {
        const int c = uu * 64 + lane;
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int i = min(i0 + r, rows_I - 1);
            const int cc = min(c, chunks - 1);
            qg[uu][r] = ldg_nt16(Wg + (long)i * a.K + (cc << 3));
            qu[uu][r] = ldg_nt16(Wu + (long)i * a.K + (cc << 3));
        }
    }
    xstage<MT, XR>(xr, M, a.K, a.norm_w != nullptr, a.eps, smem);
    if (!active) return;
    const float* xs = smem + XS_RED;
    float ag[RB][MT], au[RB][MT];
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int m = 0; m < MT; ++m) { ag[r][m] = 0.f; au[r][m] = 0.f; }
#pragma unroll
    for (int uu = 0; uu < U; ++uu) {
        const int c = uu * 64 + lane;
        if (c >= chunks) continue;
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            float wg[8], wu[8];
            unpack8<WT>(qg[uu][r], wg);
            unpack8<WT>(qu[uu][r], wu);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                if (m < M) {
                    float xv[8];
                    ld_x8(xs + m * a.K + (c << 3), xv);
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        ag[r][m] = fmaf(xv[j], wg[j], ag[r][m]);
                        au[r][m] = fmaf(xv[j], wu[j], au[r][m]);
                    }
                }
            }
        }
    }
    const float scale = routed ? sel_w : 1.f;
    float* hout = routed ? a.h + (long)sl * a.I : a.hs;
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const float gs = wave_sum(ag[r][m]);
            const float us = wave_sum(au[r][m]);
            const int i = i0 + r;
            if (lane == 0 && m < M && i < rows_I) {
                float hv = (gs / (1.0f + expf(-gs))) * us;  // silu (candle: x / (1 + exp(-x)))
                if (routed) hv = hv * scale;
                hout[(long)m * rows_I + i] = hv;
            }
        }
}

template <typename WT, int MT>
__global__ __launch_bounds__(256) void moe_gateup_slot_kernel(MoeDec2Args a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    gateup_slot_body<WT, MT>(a, blockIdx.x, smem);
}
// the shared-expert blocks of the slot grid on their own (bid offset past the routed slots), so the
// routed launch carries single-token registers and LDS (B > 1: MT = T only where it is needed)
template <typename WT, int MT, int RB>
__global__ __launch_bounds__(256) void moe_gateup_shared_kernel(MoeDec2Args a, int bid0) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    gateup_slot_body<WT, MT, RB>(a, bid0 + blockIdx.x, smem);
}

// ------------------------------------------------------------------ MoE down + combine + residual
// A wave owns output row j of every token: v = sum_k h~[row(t,k)] . Wd_{e_k}[j]
// (h~ already carries w_k) + hs[t] . Wsd[j];  X[t][j] += v.  Per token the block first
// loads the activations it needs ([topk x I] routed rows + [Is] shared row) into registers,
// then issues every weight load, then stages the activations through LDS (STAGE: when
// they fit in 64 KB), so that no activation load queues behind the weight stream.
constexpr int DN_HREG = 8;  // float4 activation registers per thread (topk*I + Is <= 8192)

template <typename WT, bool STAGE>
__global__ __launch_bounds__(256) void moe_down2_kernel(MoeDec2Args a) {
    extern __shared__ __attribute__((aligned(16))) float hsm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = blockIdx.x * 4 + wave;
    const bool active = j < a.Hout;
    if (!STAGE && !active) return;
    const int K = a.topk;
    const int ch_r = K > 0 ? (a.I >> 3) : 0, ch_s = a.sWd ? (a.Is >> 3) : 0;
    const int jj0 = min(j, a.Hout - 1);
    const WT* Ws = reinterpret_cast<const WT*>(a.sWd) + (long)jj0 * a.Is;
    const int nr4 = K * (a.I >> 2), ns4 = ch_s ? (a.Is >> 2) : 0;  // float4 counts (routed, shared)
    for (int t = 0; t < a.T; ++t) {
        float4 hreg[DN_HREG];
        if (STAGE) {
#pragma unroll
            for (int r = 0; r < DN_HREG; ++r) {
                const int f = tid + r * 256;
                const float* src = nullptr;
                if (f < nr4) {
                    const int k = f / (a.I >> 2), off = f - k * (a.I >> 2);
                    const int row = a.apos ? a.apos[t * K + k] : t * K + k;
                    src = a.h + (long)row * a.I + off * 4;
                } else if (f < nr4 + ns4) {
                    src = a.hs + (long)t * a.Is + (f - nr4) * 4;
                }
                hreg[r] = src ? *reinterpret_cast<const float4*>(src) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        float acc = 0.f;
        for (int br = 0, bs = 0; br < ch_r || bs < ch_s; br += 128, bs += 256) {
            uint4 qr[8][2], qs[4];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (k < K) {
                    const int e = a.ids[t * K + k];
                    const WT* Wd = reinterpret_cast<const WT*>(a.Wd) + ((long)e * a.Hout + jj0) * a.I;
#pragma unroll
                    for (int uu = 0; uu < 2; ++uu) {
                        const int c = br + uu * 64 + lane;
                        qr[k][uu] = ldg_nt16(Wd + (min(c, ch_r - 1) << 3));
                    }
                }
            }
#pragma unroll
            for (int uu = 0; uu < 4; ++uu) {
                const int c = bs + uu * 64 + lane;
                qs[uu] = ch_s ? ldg_nt16(Ws + (min(c, ch_s - 1) << 3)) : make_uint4(0u, 0u, 0u, 0u);
            }
            if (STAGE && br == 0) {
                if (t > 0) __syncthreads();  // previous token's rows consumed
#pragma unroll
                for (int r = 0; r < DN_HREG; ++r) {
                    const int f = tid + r * 256;
                    if (f < nr4 + ns4) *reinterpret_cast<float4*>(hsm + f * 4) = hreg[r];
                }
                __syncthreads();
            }
            if (!active) continue;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (k < K) {
                    const float* hp = STAGE ? hsm + (long)k * a.I
                                            : a.h + (long)(a.apos ? a.apos[t * K + k] : t * K + k) * a.I;
#pragma unroll
                    for (int uu = 0; uu < 2; ++uu) {
                        const int c = br + uu * 64 + lane;
                        if (c < ch_r) {
                            float hv[8], w8[8];
                            ld_x8(hp + (c << 3), hv);
                            unpack8<WT>(qr[k][uu], w8);
#pragma unroll
                            for (int q = 0; q < 8; ++q) acc = fmaf(hv[q], w8[q], acc);
                        }
                    }
                }
            }
            const float* hs = STAGE ? hsm + (long)K * a.I : a.hs + (long)t * a.Is;
#pragma unroll
            for (int uu = 0; uu < 4; ++uu) {
                const int c = bs + uu * 64 + lane;
                if (c < ch_s) {
                    float hv[8], w8[8];
                    ld_x8(hs + (c << 3), hv);
                    unpack8<WT>(qs[uu], w8);
#pragma unroll
                    for (int q = 0; q < 8; ++q) acc = fmaf(hv[q], w8[q], acc);
                }
            }
        }
        if (active) {
            const float v = wave_sum(acc);
            if (lane == 0) {
                float* xp = a.out + (long)t * a.Hout + j;
                *xp = *xp + v;
            }
        }
    }
}

// Slot-mode down (T <= 8, topk = KT at compile time, I <= 1024, Is <= 2048): per token,
// activations -> registers, every routed + shared weight load, then LDS staging and FMAs;
// straight-line so each consumer waits only for the loads it needs.
template <typename WT, int KT>
__device__ __forceinline__ void down_slot_body(const MoeDec2Args& a, const int bid, float* hsm) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = bid * 4 + wave;
    const bool active = j < a.Hout;
    const int jj = min(j, a.Hout - 1);
    const int ch_r = a.I >> 3, ch_s = a.sWd ? (a.Is >> 3) : 0;
    const int nr4 = KT * (a.I >> 2), ns4 = a.sWd ? (a.Is >> 2) : 0, n4 = nr4 + ns4;
    const WT* Ws = a.sWd ? reinterpret_cast<const WT*>(a.sWd) + (long)jj * a.Is
                         : reinterpret_cast<const WT*>(a.Wd) + (long)jj * a.I;
    const int cs_max = a.sWd ? ch_s - 1 : ch_r - 1;
    for (int t = 0; t < a.T; ++t) {
        // slot rows t*KT .. t*KT+KT-1 of h are contiguous: [KT*I routed | Is shared] as one vector
        const float* hr = a.h + (long)t * KT * a.I;
        const float* hsh = a.sWd ? a.hs + (long)t * a.Is : hr;
        f32x4 hreg[DN_HREG];  // native vector type: a float4 struct array stays in scratch here
#pragma unroll
        for (int r = 0; r < DN_HREG; ++r) {
            const int f = min(tid + r * 256, n4 - 1);
            const float* src = f < nr4 ? hr + f * 4 : hsh + (f - nr4) * 4;
            hreg[r] = *reinterpret_cast<const f32x4*>(src);
        }
        uint4 qr[KT][2], qs[4];
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            const int e = a.ids[t * KT + k];
            const WT* Wd = reinterpret_cast<const WT*>(a.Wd) + ((long)e * a.Hout + jj) * a.I;
#pragma unroll
            for (int uu = 0; uu < 2; ++uu) qr[k][uu] = ldg_nt16(Wd + (min(uu * 64 + lane, ch_r - 1) << 3));
        }
#pragma unroll
        for (int uu = 0; uu < 4; ++uu) qs[uu] = ldg_nt16(Ws + (min(uu * 64 + lane, cs_max) << 3));
        __syncthreads();  // previous token's rows consumed (unconditional: keeps hreg in VGPRs)
#pragma unroll
        for (int r = 0; r < DN_HREG; ++r)  // LDS holds 256*DN_HREG float4: no bounds branch
            *reinterpret_cast<f32x4*>(hsm + (tid + r * 256) * 4) = hreg[r];
        __syncthreads();
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < KT; ++k) {
#pragma unroll
            for (int uu = 0; uu < 2; ++uu) {
                const int c = uu * 64 + lane;
                if (c < ch_r) {
                    float hv[8], w8[8];
                    ld_x8(hsm + k * a.I + (c << 3), hv);
                    unpack8<WT>(qr[k][uu], w8);
#pragma unroll
                    for (int q = 0; q < 8; ++q) acc = fmaf(hv[q], w8[q], acc);
                }
            }
        }
#pragma unroll
        for (int uu = 0; uu < 4; ++uu) {
            const int c = uu * 64 + lane;
            if (c < ch_s) {
                float hv[8], w8[8];
                ld_x8(hsm + nr4 * 4 + (c << 3), hv);
                unpack8<WT>(qs[uu], w8);
#pragma unroll
                for (int q = 0; q < 8; ++q) acc = fmaf(hv[q], w8[q], acc);
            }
        }
        const float v = wave_sum(acc);
        if (active && lane == 0) {
            float* xp = a.out + (long)t * a.Hout + j;
            *xp = *xp + v;
        }
    }
}

template <typename WT, int KT>
__global__ __launch_bounds__(256) void moe_down_slot_kernel(MoeDec2Args a) {
    extern __shared__ __attribute__((aligned(16))) float hsm[];
    down_slot_body<WT, KT>(a, blockIdx.x, hsm);
}

// ------------------------------------------------------------------ decode gate/up, T = 1 (mix)
// Rank form of the greedy top-k (block.rs:1254-1301: softmax, stable descending sort, ties ->
// lower expert id): lane e holds score s_e; rank_e = #{j : s_j > s_e or (s_j == s_e and j < e)};
// pick k is the lane whose rank is k.  Identical picks to topk_select, no serial argmax rounds.
// lds: 128 floats private to the calling wave (wave_rank64).  Returns (expert, weight) of pick `want`.
// coop: the four waves of a block all call this (same logits), each counting the keys of one quarter and
// summing the quarters over part (4 x 64 ints, one block barrier).  At one page every routed wave ranks
// the same 64 scores, 28 waves per CU at once: the whole-rank form is bound by the CU's LDS read rate
// (32 broadcast 16-byte reads per wave), the quarter form reads a quarter of that.
__device__ __forceinline__ void topk_rank_pick(float logit, int E, int K, int softmax_scoring, int norm_topk,
                                               float scaling, int want, float* lds, int* part, bool coop,
                                               int& e_out, float& w_out) {
    const int lane = threadIdx.x & 63;
    float sc;
    if (softmax_scoring) {
        const float v = lane < E ? logit : -INFINITY;
        const float mx = wave_max(v);
        const float ex = lane < E ? expf(v - mx) : 0.f;
        const float sum = wave_sum(ex);
        sc = lane < E ? ex / sum : -INFINITY;
    } else {
        sc = lane < E ? 1.0f / (1.0f + expf(-logit)) : -INFINITY;
    }
    int rank;
    if (coop) {
        const int wave = threadIdx.x >> 6;
        const unsigned long long key = ((unsigned long long)fkey(sc) << 32) | (unsigned)(63 - lane);
        unsigned long long* kl = reinterpret_cast<unsigned long long*>(lds);
        kl[lane] = key;
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        int r0 = 0, r1 = 0;
#pragma unroll
        for (int j2 = 0; j2 < 8; ++j2) {
            const ulonglong2 o = reinterpret_cast<const ulonglong2*>(kl)[8 * wave + j2];
            r0 += o.x > key ? 1 : 0;
            r1 += o.y > key ? 1 : 0;
        }
        part[wave * 64 + lane] = r0 + r1;
        __syncthreads();
        rank = part[lane] + part[64 + lane] + part[128 + lane] + part[192 + lane];
    } else {
        rank = wave_rank64<true>(sc, lds);
    }
    if (lane >= E) rank = 1 << 20;
    // sum of the top-k scores in pick order (topk_select adds them in rank order); the pick's lane is uniform,
    // so its score comes over with a lane read, not an LDS permute
    float wsum = 0.f;
    if (K > 1 && norm_topk) {
        for (int k = 0; k < K; ++k) {
            const unsigned long long bm = __ballot(rank == k);
            const int e = __builtin_ctzll(bm);
            wsum += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sc), e));
        }
    }
    const unsigned long long bm = __ballot(rank == want);
    const int e = __builtin_ctzll(bm);
    float v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sc), e));
    if (K > 1 && norm_topk) v = v / (wsum + 1e-20f);
    if (scaling != 1.0f) v = v * scaling;
    e_out = e;
    w_out = v;
}

template <typename WT>
__global__ __launch_bounds__(256) void moe_gateup_mix_kernel(MoeDec2Args a, const float* xn, int routed_first) {
    constexpr int RB = 1;  // one gate + up row pair per wave (66 VGPRs: the 1792-block grid is resident at once)
    WaveSpan span_(a.span);
    __shared__ __attribute__((aligned(16))) float rank_lds[4][128];
    __shared__ int part_s[4 * 64];
    constexpr int U = 3;  // K <= 1536
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x;
    const int wpr = (a.I + RB - 1) / RB;                 // routed waves per pick
    const int n_sh = a.sWgu ? (a.Is + RB - 1) / RB : 0;  // shared waves
    const int n_rt = a.topk * wpr;
    // wave roles: routed_first = 0: wave 0 of every block streams the shared expert, waves 1..3 a routed
    // expert; 1: the first ceil(n_rt / 4) blocks are all routed and the shared blocks come last, so the waves
    // with the longer chain (logits -> picks -> weights) are dispatched first and the ones without it last
    const int nbr = (n_rt + 3) >> 2;
    const bool shared = routed_first ? b >= nbr : wave == 0;
    const int widx = routed_first ? (shared ? 4 * (b - nbr) + wave : 4 * b + wave) : (shared ? b : 3 * b + wave - 1);
    if (shared ? widx >= n_sh : widx >= n_rt) return;   // whole wave: no block barrier below
    const int chunks = a.K >> 3;
    const int sl = shared ? 0 : widx / wpr;
    const int i0 = (shared ? widx : widx % wpr) * RB;
    int e = 0;
    float wk = 1.f;
    uint4 qg[U][RB], qu[U][RB];
    float xr[U][8];
    auto issue = [&](const WT* Wg, const WT* Wu, int rows) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int cc = min(u * 64 + lane, chunks - 1);
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int i = min(i0 + r, rows - 1);
                qg[u][r] = ldg_nt16(Wg + (long)i * a.K + (cc << 3));
                qu[u][r] = ldg_nt16(Wu + (long)i * a.K + (cc << 3));
            }
        }
    };
    auto load_x = [&]() {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int cc = min(u * 64 + lane, chunks - 1);
            ld_x8(xn + (cc << 3), xr[u]);
        }
    };
    if (shared) {
        // the shared expert needs nothing from this step: its weight stream goes out first
        const WT* Wg = reinterpret_cast<const WT*>(a.sWgu);
        issue(Wg, Wg + (long)a.Is * a.K, a.Is);
        load_x();
    } else {
        // the token row goes out behind the pick's weight rows: its L2 latency hides under theirs, and the pick
        // runs with no row registers live (the 1792-block grid's residency is set by this kernel's VGPRs)
        const float lg = a.logits[min(lane, a.E - 1)];
        // a whole routed block (routed_first: blocks < n_rt / 4 hold four routed waves, none returned) ranks
        // cooperatively; any other routed wave alone
        const bool coop = routed_first && b < (n_rt >> 2);
        topk_rank_pick(lg, a.E, a.topk, a.softmax_scoring, a.norm_topk, a.scaling, sl, rank_lds[wave], part_s, coop, e,
                       wk);
        const WT* Wg = reinterpret_cast<const WT*>(a.Wgu) + (long)e * 2 * a.I * a.K;
        issue(Wg, Wg + (long)a.I * a.K, a.I);
        load_x();
        if (i0 == 0 && lane == 0) { a.ids_out[sl] = e; a.w_out[sl] = wk; }
    }
    const int rows = shared ? a.Is : a.I;
    float ag[RB], au[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) { ag[r] = 0.f; au[r] = 0.f; }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int cc = u * 64 + lane;
        if (cc >= chunks) continue;
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            float wg[8], wu[8];
            unpack8<WT>(qg[u][r], wg);
            unpack8<WT>(qu[u][r], wu);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                ag[r] = fmaf(xr[u][j], wg[j], ag[r]);
                au[r] = fmaf(xr[u][j], wu[j], au[r]);
            }
        }
    }
    float* hout = shared ? a.hs : a.h + (long)sl * a.I;
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        const float gs = wave_sum(ag[r]);
        const float us = wave_sum(au[r]);
        const int i = i0 + r;
        if (lane == 0 && i < rows) {
            float hv = (gs / (1.0f + expf(-gs))) * us;  // silu (candle: x / (1 + exp(-x)))
            if (!shared) hv = hv * wk;
            hout[i] = hv;
        }
    }
}

// Decode down + combine + residual for one token (T = 1), split-K over the block's NW = 8 waves:
// the K axis [topk routed h rows (I each, slot order, w_k already folded) | shared h (Is)] is
// cut in 8 contiguous chunk ranges, wave w owns one for the block's RPB = 2 output rows, its h
// values come straight from L2 into registers (no block barrier before the FMAs); the 8 wave
// partials meet once in LDS and x[j] += ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)).
template <typename WT>
__global__ __launch_bounds__(512) void moe_down_mix_kernel(MoeDec2Args a) {
    constexpr int RPB = 2, NW = 8;
    WaveSpan span_(a.span);
    __shared__ float part[NW][RPB];
    constexpr int U = 16 / NW;  // chunks per lane: (topk * I + Is) / 8 / NW waves <= 64 U (= 2)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j0 = blockIdx.x * RPB;
    const int cpi = a.I >> 3, cps = a.sWd ? (a.Is >> 3) : 0;
    const int nr = a.topk * cpi, nch = nr + cps;
    const int per = (nch + NW - 1) / NW;
    const int c0 = wave * per, c1 = min(nch, c0 + per);
    // lanes past the wave's range load its last chunk again (dropped below), so a range inside one segment
    // (the model: 6 x 112 routed + 224 shared chunks over 8 waves of 112) reads one expert id at a uniform
    // address, issued as the wave's first load: the weight addresses wait for it alone, where the per-lane
    // id loads sat behind the h loads in the in-order vmcnt.  Same process, one page, 256 tokens: 108.90 vs
    // 109.08 ms, every one of four alternating rounds (profiles/r06_ab/down_mix_uniform_id_same_process.log)
    const int glim = c1 > c0 ? c1 - 1 : nch - 1;
    const int sf = __builtin_amdgcn_readfirstlane(c0 < nr ? c0 / cpi : -1);  // (the division runs on the VALU)
    const int sl = __builtin_amdgcn_readfirstlane(glim < nr ? glim / cpi : -1);
    const bool uni = sf == sl;
    const int e_w = (uni && sf >= 0) ? a.ids[sf] : 0;
    // the residual rows, loaded first (not after the LDS combine: one dependent round trip fewer)
    const float xres = a.out[min(j0 + (int)(threadIdx.x & (RPB - 1)), a.Hout - 1)];
    // 1. h of this wave's chunks (independent of the picks)
    f32x4 hv[U][2];
    int seg[U], off[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int g = min(c0 + u * 64 + lane, glim);
        const bool rt = g < nr;
        seg[u] = rt ? g / cpi : -1;
        off[u] = (rt ? g % cpi : g - nr) << 3;
        const float* src = rt ? a.h + (long)seg[u] * a.I + off[u] : a.hs + off[u];
        hv[u][0] = *reinterpret_cast<const f32x4*>(src);
        hv[u][1] = *reinterpret_cast<const f32x4*>(src + 4);
    }
    // 2. the picked experts' down rows (+ shared) for RPB output rows
    uint4 q[RPB][U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int e = uni ? e_w : (seg[u] >= 0 ? a.ids[seg[u]] : 0);  // shared chunks (all at topk 0) read no id
#pragma unroll
        for (int r = 0; r < RPB; ++r) {
            const int j = min(j0 + r, a.Hout - 1);
            const WT* W = seg[u] >= 0 ? reinterpret_cast<const WT*>(a.Wd) + ((long)e * a.Hout + j) * a.I + off[u]
                                      : reinterpret_cast<const WT*>(a.sWd) + (long)j * a.Is + off[u];
            q[r][u] = ldg_nt16(W);
        }
    }
    float acc[RPB];
#pragma unroll
    for (int r = 0; r < RPB; ++r) acc[r] = 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (c0 + u * 64 + lane < c1) {
            const float hx[8] = {hv[u][0][0], hv[u][0][1], hv[u][0][2], hv[u][0][3],
                                 hv[u][1][0], hv[u][1][1], hv[u][1][2], hv[u][1][3]};
#pragma unroll
            for (int r = 0; r < RPB; ++r) {
                float w8[8];
                unpack8<WT>(q[r][u], w8);
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[r] = fmaf(hx[k], w8[k], acc[r]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RPB; ++r) {
        const float v = wave_sum(acc[r]);
        if (lane == 0) part[wave][r] = v;
    }
    __syncthreads();
    if (threadIdx.x < RPB && j0 + threadIdx.x < a.Hout) {
        const int r = threadIdx.x;
        const float v = ((part[0][r] + part[1][r]) + (part[2][r] + part[3][r])) + ((part[4][r] + part[5][r]) + (part[6][r] + part[7][r]));
        a.out[j0 + r] = xres + v;
    }
}

bool moe_down_mix_ok(const MoeDec2Args& a) {
    const int nch = a.topk * (a.I >> 3) + (a.sWd ? (a.Is >> 3) : 0);
    return a.slot_mode && a.T == 1 && !a.apos && a.I % 8 == 0 && (!a.sWd || a.Is % 8 == 0) && (nch + 7) / 8 <= 128 &&
           a.ids;
}

void launch_moe_down_mix(const MoeDec2Args& a, hipStream_t s) {
    if (!moe_down_mix_ok(a)) throw std::runtime_error("EINVAL: moe_down_mix outside its range");
    // 8 waves of 2 chunks per lane (50 VGPRs, 8 waves per SIMD) beat 4 of 4 (84 VGPRs): shorter per-wave
    // load chains, 6.49 -> 6.01 us; 2 output rows per block
    const dim3 grid((a.Hout + 1) / 2);
    with_wt(a.wdtype, [&](auto wt) { DSOCR_LAUNCH((moe_down_mix_kernel<decltype(wt)>), grid, dim3(512), 0, s, a); });
}

bool moe_gateup_mix_ok(const MoeDec2Args& a) {
    return a.slot_mode && a.logits && a.T == 1 && a.E <= 64 && a.topk <= 8 && a.K % 8 == 0 && a.K <= 64 * 3 * 8 &&
           a.ids_out && a.w_out;
}

// DSOCR_GU_ORDER (A/B switch, read at every launch): 0 (default since round 6) = one shared wave per block; 1 =
// routed blocks first, shared blocks last.  Round 5 kept 1 from a same-process A/B under a graph-mode kernel trace
// (9.13 -> 8.77 us per launch, profiles/r05_ab_gu_order.txt); without the profiler, in separate processes on one
// box, 0 is the faster: 256-token decode 107.9 vs 109.8 ms (mean of three alternating pairs, never slower,
// profiles/r06_ab/gu_order_repeat.log).  The waves' arithmetic is unchanged.
static int gu_order() {
    const char* e = getenv("DSOCR_GU_ORDER");
    return e ? atoi(e) : 0;
}

void launch_moe_gateup_mix(const MoeDec2Args& a, const float* xn, hipStream_t s) {
    if (!moe_gateup_mix_ok(a) || !xn) throw std::runtime_error("EINVAL: moe_gateup_mix outside its range");
    // one gate + up row pair per wave: 9.46 -> 8.73 us against two (98 / 90 VGPRs), 3.47 -> 3.55 pages/s
    const int n_sh = a.sWgu ? a.Is : 0;
    const int n_rt = a.topk * a.I;
    const int rf = gu_order();
    dim3 grid(rf ? (n_rt + 3) / 4 + (n_sh + 3) / 4 : std::max(n_sh, (n_rt + 2) / 3));
    with_wt(a.wdtype, [&](auto wt) { DSOCR_LAUNCH((moe_gateup_mix_kernel<decltype(wt)>), grid, dim3(256), 0, s, a, xn, rf); });
}

// ------------------------------------------------------------------ which kernels a decode MoE layer runs
// One choice per stage, each enumerator named after the kernels that run.  moe_plan() makes the three choices
// once; launch_moe_decode switches on them and the name / kind queries spell the same enumerators, so a name
// cannot disagree with its launch.
namespace {
enum class Route {
    InGateupMix,   // topk_rank_pick in every routed wave of moe_gateup_mix (after the logits GEMV)
    InGateupSlot,  // topk_select in the self-routing gate/up blocks (moe_gateup_slot, or moe_gateup2's slot branch)
    MoeRoute,      // logits GEMV, then moe_route: route_token + group_assignments
    InGateupMm,    // topk_wave64 inside the matrix-core gate/up: no router launch
    DecRouteGrp,   // topk_wave64 in the one-launch router (also the packed path)
    DecRouter,     // topk_write in dec_router's last-block epilogue
};
enum class GateUp {
    Mix,         // moe_gateup_mix_kernel (T = 1)
    Shared,      // moe_gateup_shared_kernel alone: one token through a dense / shared-only MLP (layer 0)
    Slot,        // moe_gateup_slot_kernel, routed slots and shared blocks in one grid (T <= 2)
    SlotShared,  // moe_gateup_slot_kernel<1> over the routed slots, then moe_gateup_shared_kernel if shared (T = 3..8)
    Gateup2,     // moe_gateup2_kernel (sorted groups; also self-routing slots whose K is too long for the slot kernel)
    Grp,         // moe_gateup_grp_kernel
    Mm,          // moe_gateup_mm_kernel (decode_mm.hip); routes too under Route::InGateupMm
    Q,           // moe_gateup_q_kernel (decode_q.hip)
};
enum class Down {
    Mix,          // moe_down_mix_kernel (T = 1)
    Slot,         // moe_down_slot_kernel (top-k 6 or 3)
    Down2Staged,  // moe_down2_kernel<STAGE>: the token's h rows through LDS
    Down2,        // moe_down2_kernel, h straight from global memory
    Grp,          // moe_down_grp_kernel
    Mm,           // moe_down_mm_kernel (decode_mm.hip)
    Q,            // moe_down_q_kernel (decode_q.hip)
};

// The forms behind launch_moe_gateup2 / launch_moe_down2, read off the launch's own arguments (the two are entry
// points of their own as well: the dense layer-0 MLP, kbench).
GateUp gateup2_form(const MoeDec2Args& a) {
    if (a.T == 1 && a.slots == 0 && a.sWgu && a.Is > 0 && a.K % 8 == 0 && a.K <= 64 * 3 * 8) return GateUp::Shared;
    if (a.slot_mode && a.K <= 64 * 3 * 8 && a.T <= 8) return a.T > 2 ? GateUp::SlotShared : GateUp::Slot;
    return GateUp::Gateup2;
}
long down2_f4(const MoeDec2Args& a) { return (long)a.topk * (a.I / 4) + (a.sWd ? a.Is / 4 : 0); }  // float4 of h per token
Down down2_form(const MoeDec2Args& a) {
    const long f4 = down2_f4(a);
    if (a.slot_mode && !a.apos && (a.topk == 6 || a.topk == 3) && a.I <= 1024 && (!a.sWd || a.Is <= 2048) &&
        f4 <= 256L * DN_HREG)
        return Down::Slot;
    return f4 <= 256L * DN_HREG && f4 * 16 <= (long)STAGE_LDS_MAX ? Down::Down2Staged : Down::Down2;
}

void launch_gateup2_form(GateUp form, const MoeDec2Args& a, hipStream_t s) {
    constexpr int RB = 2;
    const int units_r = (a.I + 4 * RB - 1) / (4 * RB);
    const int units_s = a.sWgu ? (a.Is + 4 * RB - 1) / (4 * RB) : 0;
    const dim3 grid(a.slots * units_r + units_s);
    // the shared expert alone over mt >= T token rows (slots = 0: every block is a shared block): one gate + up row
    // pair per wave, 4 rows per block (RB = 1: twice the blocks of RB = 2, half as long, same per-row arithmetic)
    auto shared_alone = [&](int mt) {
        MoeDec2Args sh = a;
        sh.slots = 0;
        const size_t lds = stage_bytes(mt, a.K);
        const dim3 ns((a.Is + 3) / 4);
        with_wt(a.wdtype, [&](auto wt) {
            with_rows<1, 4, 8>(mt, [&](auto m) {
                DSOCR_LAUNCH((moe_gateup_shared_kernel<decltype(wt), decltype(m)::value, 1>), ns, dim3(256), lds, s, sh, 0);
            });
        });
    };
    switch (form) {
        case GateUp::Shared:
            shared_alone(1);
            return;
        case GateUp::SlotShared: {
            // routed slots (one token each) with MT = 1, then the shared expert over the T tokens, so the routed
            // launch carries single-token registers and LDS
            MoeDec2Args r = a;
            r.sWgu = nullptr;
            with_wt(a.wdtype, [&](auto wt) {
                DSOCR_LAUNCH((moe_gateup_slot_kernel<decltype(wt), 1>), dim3(a.slots * units_r), dim3(256), stage_bytes(1, a.K), s, r);
            });
            if (units_s) shared_alone(a.T <= 4 ? 4 : 8);
            return;
        }
        case GateUp::Slot: {
            const int mt = a.T == 1 ? 1 : (a.T <= 2 ? 2 : (a.T <= 4 ? 4 : 8));  // (T > 2 takes SlotShared)
            const size_t lds = stage_bytes(mt, a.K);
            with_wt(a.wdtype, [&](auto wt) {
                with_rows<1, 2, 4, 8>(mt, [&](auto m) {
                    DSOCR_LAUNCH((moe_gateup_slot_kernel<decltype(wt), decltype(m)::value>), grid, dim3(256), lds, s, a);
                });
            });
            return;
        }
        case GateUp::Gateup2: {
            const int mt = a.T == 1 ? 1 : (a.T <= 4 ? 4 : 8);
            const size_t lds = stage_bytes(mt, a.K);
            if (lds > STAGE_LDS_MAX) throw std::runtime_error("EINVAL: moe_gateup2 hidden size too large for LDS staging");
            with_wt(a.wdtype, [&](auto wt) {
                with_rows<1, 4, 8>(mt, [&](auto m) {
                    DSOCR_LAUNCH((moe_gateup2_kernel<decltype(wt), decltype(m)::value>), grid, dim3(256), lds, s, a);
                });
            });
            return;
        }
        default: throw std::runtime_error("EINTERNAL: moe_gateup2 dispatch");
    }
}

void launch_down2_form(Down form, const MoeDec2Args& a, hipStream_t s) {
    if (a.topk > 8) throw std::runtime_error("EINVAL: moe_down2 supports top_k <= 8");
    const dim3 grid((a.Hout + 3) / 4);
    switch (form) {
        case Down::Slot: {
            const size_t lds = (size_t)256 * DN_HREG * 16;
            with_wt(a.wdtype, [&](auto wt) {
                with_rows<6, 3>(a.topk, [&](auto kt) {
                    DSOCR_LAUNCH((moe_down_slot_kernel<decltype(wt), decltype(kt)::value>), grid, dim3(256), lds, s, a);
                });
            });
            return;
        }
        case Down::Down2Staged: {
            const size_t lds = (size_t)down2_f4(a) * 16;
            with_wt(a.wdtype, [&](auto wt) { DSOCR_LAUNCH((moe_down2_kernel<decltype(wt), true>), grid, dim3(256), lds, s, a); });
            return;
        }
        case Down::Down2:
            with_wt(a.wdtype, [&](auto wt) { DSOCR_LAUNCH((moe_down2_kernel<decltype(wt), false>), grid, dim3(256), 0, s, a); });
            return;
        default: throw std::runtime_error("EINTERNAL: moe_down2 dispatch");
    }
}
}  // namespace

void launch_moe_gateup2(const MoeDec2Args& a, hipStream_t s) { launch_gateup2_form(gateup2_form(a), a, s); }
void launch_moe_down2(const MoeDec2Args& a, hipStream_t s) { launch_down2_form(down2_form(a), a, s); }

// ------------------------------------------------------------------ grouped decode MoE (3..8 tokens)
// At 3..8 pages the slot kernels stream an expert once per (token, pick): 48 picks at 8 pages read
// ~2.8x the bytes of the distinct experts.  Here the router epilogue's records (MOE_GRP_*) give each
// distinct expert once with its tokens.
//
// Gate/up: blocks [0, units_s) are the shared expert over all T tokens, then (record s, unit u)
// s-major (records past n_active exit before any barrier).  Per block: the record (one scalar round
// trip), the activation rows of its tokens into registers, the RB gate + RB up rows per wave
// (16-byte nontemporal loads), then the rows are staged in LDS and every weight chunk is FMA'd
// against each token's row — the per-row arithmetic of the slot kernels (chunk u-major, then j).
template <typename WT, int RB>
__global__ __launch_bounds__(256) void moe_gateup_grp_kernel(MoeDec2Args a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int U = 3, XR = 2, MT = 8;  // K <= 1536, T <= 8
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int units_r = (a.I + 4 * RB - 1) / (4 * RB);
    const int units_s = a.sWgu ? (a.Is + 4 * RB - 1) / (4 * RB) : 0;
    int bid = blockIdx.x;
    const bool shared = bid < units_s;
    int s = 0, u = bid;
    if (!shared) {
        bid -= units_s;
        s = bid / units_r;
        u = bid % units_r;
    }
    const int* rec = a.grp + MOE_GRP_REC * (1 + s);
    int e = 0, cnt = a.T;
    int rows[MT];
    float wts[MT];
    if (!shared) {
        if (s >= a.grp[0]) return;  // block-uniform, before any barrier
        e = rec[0];
        cnt = rec[1];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            rows[m] = rec[2 + min(m, cnt - 1)];
            wts[m] = __int_as_float(rec[10 + min(m, cnt - 1)]);
        }
    } else {
#pragma unroll
        for (int m = 0; m < MT; ++m) { rows[m] = min(m, cnt - 1); wts[m] = 1.f; }
    }
    // 1. activation rows (token t = row / topk for routed picks) into registers
    float4 xr[MT][XR];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int t = shared ? rows[m] : rows[m] / a.topk;
        const float* xp = a.x + (long)t * a.K;
#pragma unroll
        for (int i = 0; i < XR; ++i) xr[m][i] = *reinterpret_cast<const float4*>(xp + min((tid + i * 256) * 4, a.K - 4));
    }
    // 2. the weight stream
    const int rows_I = shared ? a.Is : a.I;
    const WT* Wg = shared ? reinterpret_cast<const WT*>(a.sWgu) : reinterpret_cast<const WT*>(a.Wgu) + (long)e * 2 * a.I * a.K;
    const WT* Wu = Wg + (long)rows_I * a.K;
    const int i0 = (u * 4 + wave) * RB;
    const int chunks = a.K >> 3;
    uint4 qg[U][RB], qu[U][RB];
#pragma unroll
    for (int uu = 0; uu < U; ++uu) {
        const int cc = min(uu * 64 + lane, chunks - 1);
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int i = min(i0 + r, rows_I - 1);
            qg[uu][r] = ldg_nt16(Wg + (long)i * a.K + (cc << 3));
            qu[uu][r] = ldg_nt16(Wu + (long)i * a.K + (cc << 3));
        }
    }
    // 3. stage the rows (waits for the activation loads only)
    float* xs = smem;
#pragma unroll
    for (int m = 0; m < MT; ++m)
        if (m < cnt)
#pragma unroll
            for (int i = 0; i < XR; ++i) {
                const int k = (tid + i * 256) * 4;
                if (k < a.K) *reinterpret_cast<float4*>(xs + m * a.K + k) = xr[m][i];
            }
    __syncthreads();
    if (i0 >= rows_I) return;
    float ag[RB][MT], au[RB][MT];
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int m = 0; m < MT; ++m) { ag[r][m] = 0.f; au[r][m] = 0.f; }
#pragma unroll
    for (int uu = 0; uu < U; ++uu) {
        const int c = uu * 64 + lane;
        if (c >= chunks) continue;
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            float wg[8], wu[8];
            unpack8<WT>(qg[uu][r], wg);
            unpack8<WT>(qu[uu][r], wu);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                if (m < cnt) {
                    float xv[8];
                    ld_x8(xs + m * a.K + (c << 3), xv);
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        ag[r][m] = fmaf(xv[j], wg[j], ag[r][m]);
                        au[r][m] = fmaf(xv[j], wu[j], au[r][m]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (m < cnt) {
                const float gs = wave_sum(ag[r][m]);
                const float us = wave_sum(au[r][m]);
                const int i = i0 + r;
                if (lane == 0 && i < rows_I) {
                    float hv = (gs / (1.0f + expf(-gs))) * us;  // silu (candle: x / (1 + exp(-x)))
                    if (shared) a.hs[(long)m * a.Is + i] = hv;
                    else a.h[(long)rows[m] * a.I + i] = hv * wts[m];
                }
            }
        }
}

// Down + combine + residual: block owns RPB output rows j of every token.  The K axis is
// [I chunks of each active expert in record order | Is chunks of the shared expert], cut in 4
// contiguous ranges (one per wave); a lane FMAs each 8-weight chunk of row j against the h rows of
// the tokens that picked that expert (h~ already carries w_k), one accumulator per token; the
// 4 wave partials meet once in LDS: out[t][j] += (p0 + p1) + (p2 + p3).
template <typename WT, int RPB, int U>
__global__ __launch_bounds__(256) void moe_down_grp_kernel(MoeDec2Args a) {
    constexpr int MT = 8;
    __shared__ int exp_s[64];
    __shared__ int row_s[64][MT];  // record s: h row of token t, or -1
    __shared__ float part[4][RPB][MT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_act = a.grp[0];
    for (int i = tid; i < n_act * MT; i += 256) {
        const int s = i / MT, t = i % MT;
        const int* rec = a.grp + MOE_GRP_REC * (1 + s);
        const int cnt = rec[1];
        int row = -1;
        for (int m = 0; m < cnt; ++m) {
            const int rw = rec[2 + m];
            if (rw / a.topk == t) row = rw;
        }
        row_s[s][t] = row;
        if (t == 0) exp_s[s] = rec[0];
    }
    __syncthreads();
    const int j0 = blockIdx.x * RPB;
    const int cpi = a.I >> 3, cps = a.sWd ? (a.Is >> 3) : 0;
    const int nr = n_act * cpi, nch = nr + cps;
    const int per = (nch + 3) / 4;
    const int c0 = wave * per, c1 = min(nch, c0 + per);
    float acc[MT][RPB];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int r = 0; r < RPB; ++r) acc[t][r] = 0.f;
    for (int base = c0; base < c1; base += 64 * U) {
        uint4 q[U][RPB];
        int seg[U], off[U];
#pragma unroll
        for (int uu = 0; uu < U; ++uu) {
            const int g = min(base + uu * 64 + lane, c1 - 1);
            const bool rt = g < nr;
            seg[uu] = rt ? g / cpi : -1;
            off[uu] = (rt ? g % cpi : g - nr) << 3;
            const int e = rt ? exp_s[seg[uu]] : 0;
#pragma unroll
            for (int r = 0; r < RPB; ++r) {
                const int j = min(j0 + r, a.Hout - 1);
                const WT* W = rt ? reinterpret_cast<const WT*>(a.Wd) + ((long)e * a.Hout + j) * a.I + off[uu]
                                 : reinterpret_cast<const WT*>(a.sWd) + (long)j * a.Is + off[uu];
                q[uu][r] = ldg_nt16(W);
            }
        }
#pragma unroll
        for (int uu = 0; uu < U; ++uu) {
            if (base + uu * 64 + lane >= c1) continue;
            float w8[RPB][8];
#pragma unroll
            for (int r = 0; r < RPB; ++r) unpack8<WT>(q[uu][r], w8[r]);
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                if (t >= a.T) continue;
                const int row = seg[uu] >= 0 ? row_s[seg[uu]][t] : t;
                if (row < 0) continue;
                const float* hp = seg[uu] >= 0 ? a.h + (long)row * a.I + off[uu] : a.hs + (long)t * a.Is + off[uu];
                float hv[8];
                ld_x8(hp, hv);
#pragma unroll
                for (int r = 0; r < RPB; ++r)
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc[t][r] = fmaf(hv[k], w8[r][k], acc[t][r]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        if (t >= a.T) continue;
#pragma unroll
        for (int r = 0; r < RPB; ++r) {
            const float v = wave_sum(acc[t][r]);
            if (lane == 0) part[wave][r][t] = v;
        }
    }
    __syncthreads();
    if (tid < RPB * MT) {
        const int r = tid / MT, t = tid % MT;
        if (t < a.T && j0 + r < a.Hout) {
            const float v = (part[0][r][t] + part[1][r][t]) + (part[2][r][t] + part[3][r][t]);
            float* xp = a.out + (long)t * a.Hout + j0 + r;
            *xp = *xp + v;
        }
    }
}

bool moe_grp_ok(const MoeDec2Args& a) {
    return a.grp && a.T >= 1 && a.T <= 8 && a.topk <= 8 && a.T * a.topk <= 64 && a.E <= 256 && a.K % 8 == 0 &&
           a.K <= 64 * 3 * 8 && a.I % 8 == 0 && (!a.sWd || a.Is % 8 == 0) && !a.norm_w && (!a.sWgu) == (!a.sWd);
}

void launch_moe_gateup_grp(const MoeDec2Args& a, hipStream_t s) {
    if (!moe_grp_ok(a)) throw std::runtime_error("EINVAL: grouped decode gate/up outside its range");
    constexpr int RB = 2;
    const int units_r = (a.I + 4 * RB - 1) / (4 * RB);
    const int units_s = a.sWgu ? (a.Is + 4 * RB - 1) / (4 * RB) : 0;
    const int slots = std::min(a.E, a.T * a.topk);
    const size_t lds = sizeof(float) * 8 * (size_t)a.K;
    dim3 grid(units_s + slots * units_r);
    with_wt(a.wdtype, [&](auto wt) { DSOCR_LAUNCH((moe_gateup_grp_kernel<decltype(wt), RB>), grid, dim3(256), lds, s, a); });
}

void launch_moe_down_grp(const MoeDec2Args& a, hipStream_t s) {
    if (!moe_grp_ok(a)) throw std::runtime_error("EINVAL: grouped decode down outside its range");
    constexpr int RPB = 2, U = 8;
    dim3 grid((a.Hout + RPB - 1) / RPB);
    with_wt(a.wdtype, [&](auto wt) { DSOCR_LAUNCH((moe_down_grp_kernel<decltype(wt), RPB, U>), grid, dim3(256), 0, s, a); });
}

// ------------------------------------------------------------------ decode MoE layer dispatch

namespace {
struct MoePlan {
    Route route;
    GateUp gu;
    Down dn;
    MoeDec2Args m;
    DecGemvArgs router;
    MoeQArgs q;      // GateUp::Q / Down::Q: the packed launches' arguments (decode_q.hip)
    MoeDec2Args mr;  // Route::InGateupMm: the arguments of the gate/up launch that also routes
};

// DSOCR_ROUTE_FUSED=0 (A/B switch, read at every plan): at 3..8 tokens the dec_route_grp launch + a plain
// gate/up instead of the router inside the matrix-core gate/up launch (moe_gateup_mm_route_ok; 141.0 vs 143.9 ms
// per 128 8-page steps, profiles/r06_ab/decode8_switches.log).  Round 5's third form, the same routing as a
// one-block launch before a plain gate/up, measured slower than both (144.9) and was removed in round 6.
static bool route_fused_on() {
    const char* e = getenv("DSOCR_ROUTE_FUSED");
    return !(e && atoi(e) == 0);
}

// The only place that reads the layer's shapes: T = 1 mix, T <= 2 (or no grouped form) self-routing slots, 3..8
// grouped by expert, more than 8 sorted; packed experts (T <= 8) take the grouped packed kernels.
MoePlan moe_plan(const MoeDecodeArgs& a) {
    const int T = a.T, E = a.E, K = a.topk, TK = T * K;
    if (T <= 0 || TK > 512 || E > 256 || K > 8 || K > E)
        throw std::runtime_error("EINVAL: decode MoE supports batch*top_k <= 512, <= 256 experts, top_k <= min(8, E)");
    if (a.H % 8 || a.I % 8 || (a.Is && a.Is % 8)) throw std::runtime_error("EINVAL: MoE dims must be multiples of 8");
    MoePlan p;
    const bool fuse_norm = T <= 2;  // T > 2: the rows are normalised once (by the router launch, into xn)
    const float* mx = (fuse_norm || !a.norm_w) ? a.x : a.xn;
    const float* mnorm = fuse_norm ? a.norm_w : nullptr;
    MoeDec2Args& m = p.m;
    m.T = T; m.K = a.H; m.Hout = a.H; m.x = mx; m.norm_w = mnorm; m.eps = a.eps; m.out = a.out;
    m.topk = K; m.E = E; m.I = a.I; m.Wgu = a.Wgu; m.Wd = a.Wd; m.wdtype = a.wdtype; m.h = a.h; m.ids = a.ids;
    if (a.sWgu && a.sWd && a.Is > 0) { m.Is = a.Is; m.sWgu = a.sWgu; m.sWd = a.sWd; m.hs = a.hs; }
    m.Wgu_swz = a.Wgu_swz; m.sWgu_swz = a.sWgu_swz; m.Wd_swz = a.Wd_swz; m.sWd_swz = a.sWd_swz;
    m.dn_part = a.dn_part; m.dn_tick = a.dn_tick; m.span = a.span; m.stamps = a.stamps;
    DecGemvArgs& gr = p.router;
    gr.M = T; gr.N = E; gr.K = a.H; gr.x = mx; gr.ldx = a.H; gr.W = a.router; gr.ldw = a.H; gr.wdtype = a.router_wdt;
    gr.bias = a.router_bias; gr.y = a.logits; gr.ldy = E; gr.norm_w = mnorm; gr.eps = a.eps; gr.span = a.route_span;
    if (a.qWgu.q && T <= 8) {
        // packed experts: dec_route_grp (norm + router + top-k + expert records, rows -> a.xn), then the
        // grouped packed gate/up and down
        MoeQArgs& q = p.q;
        q.T = T; q.topk = K; q.E = E; q.H = a.H; q.I = a.I; q.slots = std::min(E, TK);
        q.x = a.norm_w ? a.xn : a.x; q.grp = a.grp; q.Wgu = a.qWgu; q.Wd = a.qWd; q.h = a.h; q.out = a.out;
        if (a.qsWgu.q && a.qsWd.q && a.Is > 0) { q.Is = a.Is; q.sWgu = a.qsWgu; q.sWd = a.qsWd; q.hs = a.hs; }
        q.span = a.span;
        if (dec_route_grp_ok(T, E, a.H, K) && a.route_cnt && a.grp && a.xn && moe_q_ok(q)) {
            p.route = Route::DecRouteGrp;
            p.gu = GateUp::Q;
            p.dn = Down::Q;
            return p;
        }
        if (!a.Wgu || !a.Wd) throw std::runtime_error("EINVAL: packed decode MoE outside its range (T <= 8, E <= 64, H <= 1536)");
    }
    bool grouped = false;
    if (T >= 3 && T <= 8 && dec_router_ok(T, E, a.H, K) && a.route_cnt && a.grp) {
        m.slot_mode = 1; m.slots = TK; m.grp = a.grp; m.aw = a.wts;
        grouped = moe_grp_ok(m);
    }
    if (grouped) {
        // dec_route_grp (norm + router + top-k + records, one launch), else dec_router's last-block epilogue
        // writes the records; gate/up and down on the matrix cores where their shapes allow
        p.route = dec_route_grp_ok(T, E, a.H, K) ? Route::DecRouteGrp : Route::DecRouter;
        p.gu = moe_gateup_mm_ok(m) ? GateUp::Mm : GateUp::Grp;
        p.dn = moe_down_mm_ok(m) ? Down::Mm : Down::Grp;
        if (p.route == Route::DecRouteGrp && p.gu == GateUp::Mm && a.norm_w && a.router_wdt == a.wdtype && route_fused_on()) {
            MoeDec2Args r = m;
            r.x = a.x; r.norm_w = a.norm_w; r.eps = a.eps;
            r.router = a.router; r.router_bias = a.router_bias; r.router_swz = a.router_swz;
            r.softmax_scoring = a.softmax_scoring; r.norm_topk = a.norm_topk; r.scaling = a.scaling;
            r.ids_out = a.ids; r.w_out = a.wts; r.logits = a.logits;  // (block 0 also writes the logits)
            if (moe_gateup_mm_route_ok(r)) {
                p.mr = r;
                p.route = Route::InGateupMm;  // the routing runs inside the gate/up launch (no router launch)
            }
        }
    } else if (T <= 8) {
        // every gate/up block routes itself from the router logits (rank / serial greedy top-k)
        m.grp = nullptr;
        m.slot_mode = 1; m.slots = TK;
        m.logits = a.logits; m.softmax_scoring = a.softmax_scoring; m.norm_topk = a.norm_topk;
        m.scaling = a.scaling; m.ids_out = a.ids; m.w_out = a.wts;
        const bool mix = fuse_norm && moe_gateup_mix_ok(m) && a.xn_router;
        p.route = mix ? Route::InGateupMix : Route::InGateupSlot;
        p.gu = mix ? GateUp::Mix : gateup2_form(m);
        if (mix) gr.xn_out = a.xn_router;  // the router hands its normalised row to gate/up
        p.dn = moe_down_mix_ok(m) ? Down::Mix : down2_form(m);  // one token: the split-K down
    } else {
        if (!(a.eoff && a.arow && a.apos && a.active && a.n_active && a.aw))
            throw std::runtime_error("EINVAL: decode MoE over 8 tokens needs the grouping workspaces");
        m.slots = std::min(E, TK);
        m.eoff = a.eoff; m.arow = a.arow; m.apos = a.apos; m.aw = a.aw; m.active = a.active; m.n_active = a.n_active;
        p.route = Route::MoeRoute;
        p.gu = gateup2_form(m);
        p.dn = down2_form(m);
    }
    return p;
}
}  // namespace

bool moe_decode_route_launch(const MoeDecodeArgs& a) { return moe_plan(a).route != Route::InGateupMm; }

const char* moe_decode_route_kind(const MoeDecodeArgs& a) {
    switch (moe_plan(a).route) {
        case Route::InGateupMix: return "moe_gateup_mix";
        case Route::InGateupSlot: return "moe_gateup_slot";
        case Route::MoeRoute: return "moe_route";
        case Route::InGateupMm: return "moe_gateup_mm";
        case Route::DecRouteGrp: return "dec_route_grp";
        case Route::DecRouter: return "dec_router";
    }
    return "none";
}

void moe_decode_kernel_names(const MoeDecodeArgs& a, const char** gateup, const char** down) {
    const MoePlan p = moe_plan(a);
    const char* gu = "none";
    const char* dn = "none";
    switch (p.gu) {
        case GateUp::Mix: gu = "moe_gateup_mix_kernel"; break;
        case GateUp::Shared: gu = "moe_gateup_shared_kernel"; break;
        case GateUp::Slot: gu = "moe_gateup_slot_kernel"; break;
        case GateUp::SlotShared: gu = p.m.sWgu ? "moe_gateup_slot_kernel+moe_gateup_shared_kernel" : "moe_gateup_slot_kernel"; break;
        case GateUp::Gateup2: gu = "moe_gateup2_kernel"; break;
        case GateUp::Grp: gu = "moe_gateup_grp_kernel"; break;
        case GateUp::Mm: gu = "moe_gateup_mm_kernel"; break;
        case GateUp::Q: gu = "moe_gateup_q_kernel"; break;
    }
    switch (p.dn) {
        case Down::Mix: dn = "moe_down_mix_kernel"; break;
        case Down::Slot: dn = "moe_down_slot_kernel"; break;
        case Down::Down2Staged:
        case Down::Down2: dn = "moe_down2_kernel"; break;
        case Down::Grp: dn = "moe_down_grp_kernel"; break;
        case Down::Mm: dn = "moe_down_mm_kernel"; break;
        case Down::Q: dn = "moe_down_q_kernel"; break;
    }
    if (gateup) *gateup = gu;
    if (down) *down = dn;
}

void launch_moe_decode(const MoeDecodeArgs& a, hipStream_t s, int parts) {
    const MoePlan p = moe_plan(a);
    const MoeDec2Args& m = p.m;
    if (parts & MOE_ROUTE) {
        DecRouteEpi re;
        re.topk = a.topk; re.softmax_scoring = a.softmax_scoring; re.norm_topk = a.norm_topk;
        re.scaling = a.scaling; re.ids = a.ids; re.w = a.wts; re.grp = a.grp; re.counter = a.route_cnt;
        // every form but the two one-launch ones normalises the rows of T > 2 tokens first (into a.xn)
        const bool one_launch = p.route == Route::InGateupMm || p.route == Route::DecRouteGrp;
        if (!one_launch && a.T > 2 && a.norm_w) launch_rmsnorm(a.x, a.H, a.xn, a.H, a.T, a.H, a.norm_w, a.eps, s);
        switch (p.route) {
            case Route::InGateupMm: break;  // (the gate/up launch routes)
            case Route::DecRouteGrp: {
                // norm + logits + top-k + records in one block (the grouped kernels read a.xn)
                DecGemvArgs g = p.router;
                g.x = a.x; g.norm_w = a.norm_w; g.xn_out = a.norm_w ? a.xn : nullptr;
                launch_dec_route_grp(g, re, s);
                break;
            }
            case Route::DecRouter: launch_dec_router(p.router, re, s); break;
            case Route::InGateupMix:
            case Route::InGateupSlot: launch_dec_gemv(p.router, s); break;
            case Route::MoeRoute: {
                launch_dec_gemv(p.router, s);
                MoeRouteArgs ra;
                ra.logits = a.logits; ra.T = a.T; ra.E = a.E; ra.topk = a.topk; ra.softmax_scoring = a.softmax_scoring;
                ra.norm_topk = a.norm_topk; ra.scaling = a.scaling; ra.ids = a.ids; ra.w = a.wts; ra.eoff = a.eoff;
                ra.arow = a.arow; ra.apos = a.apos; ra.aw = a.aw; ra.active = a.active; ra.n_active = a.n_active;
                launch_moe_route(ra, s);
                break;
            }
        }
    }
    if (parts & MOE_GATEUP) {
        switch (p.gu) {
            case GateUp::Q: launch_moe_gateup_q(p.q, s); break;
            case GateUp::Mix: launch_moe_gateup_mix(m, a.xn_router, s); break;
            case GateUp::Mm: launch_moe_gateup_mm(p.route == Route::InGateupMm ? p.mr : m, s); break;
            case GateUp::Grp: launch_moe_gateup_grp(m, s); break;
            case GateUp::Shared:
            case GateUp::Slot:
            case GateUp::SlotShared:
            case GateUp::Gateup2: launch_gateup2_form(p.gu, m, s); break;
        }
    }
    if (parts & MOE_DOWN) {
        switch (p.dn) {
            case Down::Q: launch_moe_down_q(p.q, s); break;
            case Down::Mm: launch_moe_down_mm(m, s); break;
            case Down::Grp: launch_moe_down_grp(m, s); break;
            case Down::Mix: launch_moe_down_mix(m, s); break;
            case Down::Slot:
            case Down::Down2Staged:
            case Down::Down2: launch_down2_form(p.dn, m, s); break;
        }
    }
}

}  // namespace dsocr
