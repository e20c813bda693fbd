// Decode MoE routers: dec_router, dec_route_grp and the one-block moe_route.
#include "decode_common.hpp"

namespace dsocr {

// ------------------------------------------------------------------ router + top-k
// MoE router logits (E x K GEMV, norm fused) whose LAST-arriving block routes every token:
// softmax (or sigmoid) + greedy top-k (block.rs:1254-1301) -> ids[t*topk+k], w[t*topk+k].
// Logits are stored write-through (sc1 atomics) so the hand-off needs only the arrival
// ticket and one agent acquire in the last block (cdna_hip_programming.md Guideline 16 R1).
__device__ __forceinline__ void topk_write(const float* lg, int E, int K, int softmax_scoring, int norm_topk,
                                           float scaling, int* ids, float* w, bool sc1 = false) {
    const int lane = threadIdx.x & 63;
    float sc[4];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = min(lane + 64 * j, E - 1);
        // sc1: logits handed over inside the launch (stored sc1 by other blocks)
        sc[j] = sc1 ? __hip_atomic_load(lg + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : lg[e];
        if (lane + 64 * j >= E) sc[j] = -INFINITY;
        mx = fmaxf(mx, sc[j]);
    }
    if (softmax_scoring) {
        mx = wave_max(mx);
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sc[j] = (lane + 64 * j) < E ? expf(sc[j] - mx) : 0.f;
            sum += sc[j];
        }
        sum = wave_sum(sum);
#pragma unroll
        for (int j = 0; j < 4; ++j) sc[j] = (lane + 64 * j) < E ? sc[j] / sum : -INFINITY;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) sc[j] = (lane + 64 * j) < E ? 1.0f / (1.0f + expf(-sc[j])) : -INFINITY;
    }
    float picked[8];
    int pid[8];
    float wsum = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        picked[k] = 0.f;
        pid[k] = 0;
        if (k < K) {
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
            picked[k] = bv;
            pid[k] = bi;
            wsum += bv;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k < K) {
                float v = picked[k];
                if (K > 1 && norm_topk) v = v / (wsum + 1e-20f);
                if (scaling != 1.0f) v = v * scaling;
                ids[k] = pid[k];
                w[k] = v;
            }
        }
    }
}

template <typename WT, int MT>
__global__ __launch_bounds__(256) void dec_router_kernel(DecGemvArgs a, DecRouteEpi r) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ int last_s;
    constexpr int U = 3, XR = 2;  // K <= 1536
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x * 4 + wave;
    const bool active = n < a.N;
    const WT* W = reinterpret_cast<const WT*>(a.W);
    const int chunks = a.K >> 3;
    XRegs<MT, XR> xr;
    xload<MT, XR>(xr, a.x, a.ldx, nullptr, a.M, a.K, a.norm_w);
    uint4 wq[U];
#pragma unroll
    for (int u = 0; u < U; ++u) wq[u] = ldg_nt16(W + (long)min(n, a.N - 1) * a.ldw + (min(u * 64 + lane, chunks - 1) << 3));
    xstage<MT, XR>(xr, a.M, a.K, a.norm_w != nullptr, a.eps, smem);
    const float* xs = smem + XS_RED;
    float acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c = u * 64 + lane;
        if (c < chunks) {
            float w8[8];
            unpack8<WT>(wq[u], w8);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                if (m < a.M) {
                    float xv[8];
                    ld_x8(xs + m * a.K + (c << 3), xv);
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[m] = fmaf(xv[j], w8[j], acc[m]);
                }
            }
        }
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const float v = wave_sum(acc[m]) + (a.bias ? a.bias[min(n, a.N - 1)] : 0.f);
        if (lane == 0 && active && m < a.M)
            __hip_atomic_store(a.y + (long)m * a.ldy + n, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const int old = __hip_atomic_fetch_add(r.counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = old == (int)gridDim.x - 1;
        if (last) __hip_atomic_store(r.counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_s = last;
    }
    __syncthreads();
    if (!last_s) return;
    // every logit was stored sc1 and is read back with sc1 loads: no acquire fence needed
    // (MI355X_MICROARCH.md, hand-offs with sc1 loads in place of the acquire, first row)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (!r.grp) {
        for (int t = wave; t < a.M; t += 4)
            topk_write(a.y + (long)t * a.ldy, a.N, r.topk, r.softmax_scoring, r.norm_topk, r.scaling,
                       r.ids + t * r.topk, r.w + t * r.topk, true);
        return;
    }
    // picks into LDS, then wave 0 groups them by expert (records in increasing expert order, the
    // tokens of a record in increasing order: the h rows t*topk + k are scanned in order)
    __shared__ int ids_s[64];
    __shared__ float w_s[64];
    for (int t = wave; t < a.M; t += 4)
        topk_write(a.y + (long)t * a.ldy, a.N, r.topk, r.softmax_scoring, r.norm_topk, r.scaling, ids_s + t * r.topk,
                   w_s + t * r.topk, true);
    __syncthreads();
    const int TK = a.M * r.topk;
    if (threadIdx.x < TK) {
        r.ids[threadIdx.x] = ids_s[threadIdx.x];
        r.w[threadIdx.x] = w_s[threadIdx.x];
    }
    if (wave == 0) {
        int base = 0;
        for (int e0 = 0; e0 < a.N; e0 += 64) {
            const int e = e0 + lane;
            int cnt = 0;
            for (int i = 0; i < TK; ++i) cnt += ids_s[i] == e ? 1 : 0;
            const unsigned long long act = __ballot(cnt > 0 && e < a.N);
            const int s = base + __popcll(act & ((1ull << lane) - 1ull));
            if (cnt > 0 && e < a.N) {
                int* rec = r.grp + MOE_GRP_REC * (1 + s);
                rec[0] = e;
                rec[1] = cnt;
                int n = 0;
                for (int i = 0; i < TK; ++i)
                    if (ids_s[i] == e) {
                        rec[2 + n] = i;
                        rec[10 + n] = __float_as_int(w_s[i]);
                        ++n;
                    }
            }
            base += __popcll(act);
        }
        if (lane == 0) r.grp[0] = base;
    }
}

bool dec_router_ok(int T, int E, int K, int topk) {
    return T <= 8 && E <= 256 && K <= 64 * 3 * 8 && topk <= 8 && T * topk <= 64;
}

// Decode router for T <= 8 tokens, E <= 64 experts: RMSNorm + router logits + greedy top-k +
// expert records in one launch.  Blocks of 8 waves and 8 expert rows.  Wave w normalises token row w
// in the GEMV chunk layout (lane: chunks lane, lane+64, lane+128; its squares summed u-major then j,
// one wave sum, x / den * w — dec_gemv_rows' NORM form) in registers and puts expert row w of the
// block into LDS; then wave w dots its token row with the block's 8 expert rows (dec_gemv's per-row
// arithmetic; the last block also hands the rows to the expert kernels: xn_out).  Logits are stored write-through (sc1); the last block to
// take its ticket reads them back with sc1 loads (MI355X_MICROARCH.md hand-offs, first row), routes
// token w on wave w (topk_wave64) and wave 0 groups the picks by expert (MOE_GRP_* records).
template <typename WT>
__global__ __launch_bounds__(512) void dec_route_grp_kernel(DecGemvArgs a, DecRouteEpi r) {
    WaveSpan span_(a.span);
    constexpr int U = 3, MT = 8;  // K <= 1536, T <= 8
    extern __shared__ __attribute__((aligned(16))) uint4 ws[];  // [8 experts][K / 8] 16-bit weight chunks
    __shared__ float lg_s[MT][64];
    __shared__ __attribute__((aligned(16))) float rank_s[MT][128];
    __shared__ int ids_s[64];
    __shared__ float w_s[64];
    __shared__ int last_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#define RG_STAMP(i)                                                      \
    if (r.stamps && tid == 0 && (blockIdx.x == 0 || (i) >= 5)) r.stamps[i] = __builtin_amdgcn_s_memrealtime();
    RG_STAMP(0);
    const int n0 = blockIdx.x * MT;
    const int chunks = a.K >> 3;
    const WT* W = reinterpret_cast<const WT*>(a.W);
    // wave w: expert row n0 + w into LDS (16-bit, as stored) and token row w normalised in registers; then
    // every wave dots its token row with the block's 8 expert rows.  The products and their order per
    // (token, expert) are dec_gemv's (lane chunks u-major, then j; one wave sum); the LDS traffic is the
    // 16-bit weights once per wave instead of the f32 token rows once per expert (half the bytes)
    uint4 wq[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
        wq[u] = ldg_nt16(W + (long)min(n0 + wave, a.N - 1) * a.ldw + (min(u * 64 + lane, chunks - 1) << 3));
    float xv[U][8];
    if (wave < a.M) {
        float nw[U][8];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int cc = min(u * 64 + lane, chunks - 1);
            ld_x8(a.x + (long)wave * a.ldx + (cc << 3), xv[u]);
            if (a.norm_w) ld_x8(a.norm_w + (cc << 3), nw[u]);
        }
        if (a.norm_w) {
            float q = 0.f;
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (u * 64 + lane < chunks)
#pragma unroll
                    for (int j = 0; j < 8; ++j) q += xv[u][j] * xv[u][j];
            const float den = sqrtf(wave_sum(q) / (float)a.K + a.eps);
            RG_STAMP(1);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < 8; ++j) xv[u][j] = (xv[u][j] / den) * nw[u][j];
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c = u * 64 + lane;
        if (c < chunks) ws[wave * chunks + c] = wq[u];
    }
    __syncthreads();
    RG_STAMP(2);
    RG_STAMP(3);
    float mine = 0.f;  // lane e keeps expert n0 + e's logit for token `wave`
    if (wave < a.M) {
        float acc[MT];
#pragma unroll
        for (int e = 0; e < MT; ++e) acc[e] = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = u * 64 + lane;
            if (c < chunks) {
#pragma unroll
                for (int e = 0; e < MT; ++e) {
                    float w8[8];
                    unpack8<WT>(ws[e * chunks + c], w8);
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[e] = fmaf(xv[u][j], w8[j], acc[e]);
                }
            }
        }
#pragma unroll
        for (int e = 0; e < MT; ++e) {
            const float v = wave_sum(acc[e]) + (a.bias ? a.bias[min(n0 + e, a.N - 1)] : 0.f);
            if (lane == e) mine = v;
        }
    }
    RG_STAMP(4);
    if (wave < a.M && lane < MT && n0 + lane < a.N)
        __hip_atomic_store(a.y + (long)wave * a.ldy + n0 + lane, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        const int old = __hip_atomic_fetch_add(r.counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = old == (int)gridDim.x - 1;
        if (last) __hip_atomic_store(r.counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_s = last;
    }
    __syncthreads();
    if (!last_s) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no instruction: keeps the sc1 loads below
    RG_STAMP(5);
    {
        const int m = tid >> 6, e = tid & 63;  // 512 threads: one logit each
        lg_s[m][e] = (m < a.M && e < a.N)
                         ? __hip_atomic_load(a.y + (long)m * a.ldy + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                         : -INFINITY;
    }
    __syncthreads();
    if (wave < a.M)
        topk_wave64(lg_s[wave][lane], a.N, r.topk, r.softmax_scoring, r.norm_topk, r.scaling, rank_s[wave],
                    ids_s + wave * r.topk, w_s + wave * r.topk);
    __syncthreads();
    RG_STAMP(6);
    const int TK = a.M * r.topk;
    if (tid < TK) {
        r.ids[tid] = ids_s[tid];
        r.w[tid] = w_s[tid];
    }
    // wave 0, lane e: the tokens that picked expert e (a token's picks are distinct, so at most one
    // per token), in increasing token order -> record s = number of picked experts below e
    if (wave == 0 && r.grp)  // scratch: wave 0's rank keys (read by now)
        group_picks_wave64<0>(ids_s, w_s, a.M, r.topk, a.N, r.grp, reinterpret_cast<int*>(&rank_s[0][0]));
    // the normalised rows for the expert kernels, from this (last) block's registers after its last barrier: a
    // global store before a barrier makes the barrier wait for its acknowledgement
    if (a.xn_out && wave < a.M)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = u * 64 + lane;
            if (c < chunks) {
                float* g = a.xn_out + (long)wave * a.K + (c << 3);
                *reinterpret_cast<float4*>(g) = make_float4(xv[u][0], xv[u][1], xv[u][2], xv[u][3]);
                *reinterpret_cast<float4*>(g + 4) = make_float4(xv[u][4], xv[u][5], xv[u][6], xv[u][7]);
            }
        }
    RG_STAMP(7);
#undef RG_STAMP
}

bool dec_route_grp_ok(int T, int E, int K, int topk) {
    return T >= 1 && T <= 8 && E >= 1 && E <= 64 && K % 8 == 0 && K <= 64 * 3 * 8 && topk >= 1 && topk <= 8 &&
           topk <= E && T * topk <= 64;
}

void launch_dec_route_grp(const DecGemvArgs& a, const DecRouteEpi& r, hipStream_t s) {
    if (!dec_route_grp_ok(a.M, a.N, a.K, r.topk) || !r.ids || !r.w || !r.counter || !a.y)
        throw std::runtime_error("EINVAL: decode router (grouped) outside its range");
    dim3 grid((a.N + 7) / 8);
    const size_t lds = sizeof(uint16_t) * 8 * (size_t)a.K;
    with_wt(a.wdtype, [&](auto wt) { DSOCR_LAUNCH((dec_route_grp_kernel<decltype(wt)>), grid, dim3(512), lds, s, a, r); });
}

void launch_dec_router(const DecGemvArgs& a, const DecRouteEpi& r, hipStream_t s) {
    if (!dec_router_ok(a.M, a.N, a.K, r.topk) || !r.counter) throw std::runtime_error("EINVAL: dec_router out of range");
    const int mt = a.M == 1 ? 1 : (a.M <= 2 ? 2 : (a.M <= 4 ? 4 : 8));
    const size_t lds = stage_bytes(mt, a.K);
    dim3 grid((a.N + 3) / 4);
    with_wt(a.wdtype, [&](auto wt) {
        with_rows<1, 2, 4, 8>(mt, [&](auto m) {
            DSOCR_LAUNCH((dec_router_kernel<decltype(wt), decltype(m)::value>), grid, dim3(256), lds, s, a, r);
        });
    });
}

// ------------------------------------------------------------------ MoE routing (one block)
// softmax (or sigmoid) + greedy top-k (stable, block.rs:1271-1301) per token, then
// grouping: eoff[E+1], arow/apos/aw by sorted position, and the compact list of active
// experts (block.rs:1303-1324 sorts on the host; here one block does it in LDS).
constexpr int RT_MAXT = 64;  // tokens per routing block

struct RouteLds {
    int ids[RT_MAXT * 8];
    float w[RT_MAXT * 8];
    int cnt[257];
    int cur[257];
};

// top-k of one token's E logits (lg in LDS or global) by one wave
__device__ __forceinline__ void route_token(const MoeRouteArgs& a, const float* lg, int t, RouteLds& L) {
    const int lane = threadIdx.x & 63, E = a.E, K = a.topk;
    float sc[4];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = lane + 64 * j;
        sc[j] = e < E ? lg[e] : -INFINITY;
        mx = fmaxf(mx, sc[j]);
    }
    if (a.softmax_scoring) {
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
    float picked[8];
    float wsum = 0.f;
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
        picked[k] = bv;
        wsum += bv;
        if (lane == 0) { L.ids[t * K + k] = bi; a.ids[t * K + k] = bi; }
    }
    if (lane == 0)
        for (int k = 0; k < K; ++k) {
            float v = picked[k];
            if (K > 1 && a.norm_topk) v = v / (wsum + 1e-20f);
            if (a.scaling != 1.0f) v = v * a.scaling;
            a.w[t * K + k] = v;
            L.w[t * K + k] = v;
        }
}

// block-wide grouping of L.ids (T*topk assignments) by expert; call after a barrier
__device__ __forceinline__ void group_assignments(const MoeRouteArgs& a, RouteLds& L) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nt = blockDim.x;
    const int E = a.E, n = a.T * a.topk;
    for (int i = tid; i < n; i += nt) atomicAdd(&L.cnt[L.ids[i]], 1);
    __syncthreads();
    if (wave == 0) {  // exclusive scan of the E counts + active-expert compaction, 4 experts per lane
        int c[4], local = 0, al = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = lane * 4 + j;
            c[j] = e < E ? L.cnt[e] : 0;
            local += c[j];
            al += c[j] > 0;
        }
        int incl = local, ai = al;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(incl, o, 64), z = __shfl_up(ai, o, 64);
            if (lane >= o) { incl += y; ai += z; }
        }
        int acc = incl - local, ap = ai - al;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = lane * 4 + j;
            if (e < E) {
                L.cnt[e] = acc;
                acc += c[j];
                if (c[j] > 0) a.active[ap++] = e;
            }
        }
        if (lane == 63) { L.cnt[E] = incl; *a.n_active = ai; }
    }
    __syncthreads();
    for (int e = tid; e <= E; e += nt) a.eoff[e] = L.cnt[e];
    for (int i = tid; i < n; i += nt) {
        const int e = L.ids[i];
        const int p = L.cnt[e] + atomicAdd(&L.cur[e], 1);
        a.arow[p] = i / a.topk;
        a.apos[i] = p;
        a.aw[p] = L.w[i];
    }
}

__global__ __launch_bounds__(256) void moe_route_kernel(MoeRouteArgs a) {
    __shared__ RouteLds L;
    const int wave = threadIdx.x >> 6;
    for (int e = threadIdx.x; e <= a.E; e += 256) { L.cnt[e] = 0; L.cur[e] = 0; }
    for (int t = wave; t < a.T; t += 4) route_token(a, a.logits + (long)t * a.E, t, L);
    __syncthreads();
    group_assignments(a, L);
}

void launch_moe_route(const MoeRouteArgs& a, hipStream_t s) {
    if (a.T > RT_MAXT || a.E > 256 || a.topk > 8) throw std::runtime_error("EINVAL: routing supports T <= 64, E <= 256, top_k <= 8");
    DSOCR_LAUNCH(moe_route_kernel, dim3(1), dim3(256), 0, s, a);
}

}  // namespace dsocr
