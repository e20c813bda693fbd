// Fused decode sampling: argmax with the n-gram ban, screened final selection, step bookkeeping.
#include "decode_common.hpp"

namespace dsocr {

// ------------------------------------------------------------------ sampling (fused)
// argmax over the vocabulary with the no-repeat-ngram ban evaluated inside each block
// (sampling.rs:141-158), then one block per page finalises: fallback, EOS / output /
// context bookkeeping, next-step embedding and the KV position advance.
constexpr int SP_BLOCK = 256;
constexpr int SP_PER_BLOCK = 2048;  // 8 logits per thread, all loaded before the first compare
size_t dec_sample_blocks(int V) { return (size_t)(V + SP_PER_BLOCK - 1) / SP_PER_BLOCK; }

__device__ __forceinline__ bool sp_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// (value, index) argmax over the block (first index on ties); result in sv[0] / si[0]
__device__ __forceinline__ void block_argmax(float bv, int bi, float* sv, int* si) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    wave_argmax(bv, bi);
    if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w)
            if (sp_better(sv[w], si[w], bv, bi)) { bv = sv[w]; bi = si[w]; }
        sv[0] = bv;
        si[0] = bi;
    }
    __syncthreads();
}

// ROWS (here and in the two final kernels): the page's ngram / eos come from its RowParams record a.rows[b]
// instead of the launch arguments (a few scalar-uniform loads per block), and a page whose record says do_sample
// leaves its selection slots to dec_stoch_select_kernel<true>: a block-uniform return before any barrier.
template <bool LDSCTX, bool ROWS>
__global__ __launch_bounds__(SP_BLOCK) void dec_argmax_partial_kernel(DecSampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) int ctx_s[];  // the page's context, staged once per block (LDSCTX)
    __shared__ float sv[SP_BLOCK];
    __shared__ int si[SP_BLOCK];
    __shared__ unsigned ban[SP_PER_BLOCK / 32];  // banned-token bitmap of this block's vocab range
    const int b = blockIdx.y;
    if (ROWS && a.rows[b].do_sample) return;
    const float* lg = a.logits + (long)b * a.ld;
    const int v0 = blockIdx.x * SP_PER_BLOCK, v1 = min(a.V, v0 + SP_PER_BLOCK);
    // this block's logits first (independent loads in flight during the n-gram scan)
    constexpr int PER = SP_PER_BLOCK / SP_BLOCK;
    float xv[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int v = v0 + threadIdx.x + j * SP_BLOCK;
        xv[j] = v < v1 ? lg[v] : -INFINITY;
    }
    for (int i = threadIdx.x; i < SP_PER_BLOCK / 32; i += SP_BLOCK) ban[i] = 0u;
    const int n = a.ctx_len[b], g = ROWS ? a.rows[b].ngram : a.ngram;
    const int* ctx = a.ctx + (long)b * a.ctx_cap;
    const bool use_ban = g > 1 && n >= g - 1;
    if (LDSCTX && use_ban)
        for (int i = threadIdx.x; i < n; i += SP_BLOCK) ctx_s[i] = ctx[i];
    __syncthreads();
    const int* cx = LDSCTX ? ctx_s : ctx;
    if (use_ban) {
        for (int i = threadIdx.x; i <= n - g; i += SP_BLOCK) {
            const int t = cx[i + g - 1];
            if (t < v0 || t >= v1) continue;
            bool match = true;
            for (int jj = 0; jj < g - 1; ++jj)
                if (cx[i + jj] != cx[n - g + 1 + jj]) { match = false; break; }
            if (match) atomicOr(&ban[(t - v0) >> 5], 1u << ((t - v0) & 31));
        }
    }
    __syncthreads();
    float bv = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int v = v0 + threadIdx.x + j * SP_BLOCK;
        const float x = xv[j];
        if (v >= v1 || !(x > -INFINITY) || !(x < INFINITY)) continue;
        if (ban[(v - v0) >> 5] & (1u << ((v - v0) & 31))) continue;
        if (sp_better(x, v, bv, bi)) { bv = x; bi = v; }
    }
    block_argmax(bv, bi, sv, si);
    if (threadIdx.x == 0) {
        a.red_val[(long)b * a.red_blocks + blockIdx.x] = sv[0];
        a.red_idx[(long)b * a.red_blocks + blockIdx.x] = si[0];
    }
}

// exact logit of row v: the dec_gemv_stream arithmetic (lane chunks u*64 + lane, 8 fmaf each in
// order, DPP wave sum) on the staged row xs (one wave)
template <typename WT>
__device__ __forceinline__ float exact_row_logit(const uint16_t* W, int v, int K, const float* xs) {
    const int lane = threadIdx.x & 63, chunks = K >> 3;
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int c = u * 64 + lane;
        const uint4 q = ldg_nt16(W + (long)v * K + (min(c, chunks - 1) << 3));
        if (c < chunks) {
            float w8[8], xv[8];
            unpack8<WT>(q, w8);
            ld_x8(xs + (c << 3), xv);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc = fmaf(xv[j], w8[j], acc);
        }
    }
    return wave_sum(acc);
}

// (value, index) argmax over the block's waves: each wave's result to its LDS slot (sv / si must
// not be in use), one barrier, every thread reduces the slots itself; result in (bv, bi)
__device__ __forceinline__ void waves_argmax(float& bv, int& bi, float* sv, int* si) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
    __syncthreads();
    bv = sv[0];
    bi = si[0];
    for (int w = 1; w < nw; ++w)
        if (sp_better(sv[w], si[w], bv, bi)) { bv = sv[w]; bi = si[w]; }
}

// Screened final selection (one block per page): T = the best lower bound over the unbanned rows
// (max of the lm_head blocks'); every kept row whose upper bound reaches T is rescored exactly
// and the first-index argmax taken — the exact path's token (sampling.rs:104-118).  If nothing
// survives (every unbanned logit non-finite) the reference's fallback runs: the argmax over every
// token, unbanned.  The kernel is a chain of dependent memory round trips, so everything that
// does not depend on the token is loaded up front: the step bookkeeping words, and the next
// step's n-gram ban as PREFIX matches (positions whose first g-2 tokens equal the known part of
// the next suffix) that only need the new token compared once it is known.
constexpr int SP_LIST = 1024;  // LDS survivor list (more: rescored straight from the block slots)
constexpr int SP_PM = 256;     // LDS prefix matches (more: the ban is rescanned after the update)

__device__ __forceinline__ void screened_rescore(const DecSampleArgs& a, const uint16_t* W, const float* xs,
                                                 const int* list, int n, float T, const int* bc, long sb,
                                                 float& bv, int& bi) {
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (n <= SP_LIST) {
        for (int c = wave; c < n; c += nw) {
            const int v = list[c];
            const float x = a.w_exact_wdt == WDT_F16 ? exact_row_logit<f16_t>(W, v, a.K, xs) : exact_row_logit<bf16_t>(W, v, a.K, xs);
            if ((x > -INFINITY) && (x < INFINITY) && sp_better(x, v, bv, bi)) { bv = x; bi = v; }
        }
        return;
    }
    for (int j = wave; j < a.nblk; j += nw) {
        const int c = bc[j];
        for (int i = 0; i < c; ++i) {
            if (!(a.cand_hi[sb + (long)i * a.nblk + j] >= T)) continue;
            const int v = a.cand[sb + (long)i * a.nblk + j];
            const float x = a.w_exact_wdt == WDT_F16 ? exact_row_logit<f16_t>(W, v, a.K, xs) : exact_row_logit<bf16_t>(W, v, a.K, xs);
            if ((x > -INFINITY) && (x < INFINITY) && sp_better(x, v, bv, bi)) { bv = x; bi = v; }
        }
    }
}

template <int NT, bool ROWS>
__global__ __launch_bounds__(NT) void dec_screen_final_kernel(DecSampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];  // [K] staged row | survivor list
    __shared__ float sv[NT / 64], sv2[NT / 64];
    __shared__ int si2[NT / 64];
    __shared__ int nlist, nban_s, pm_n;
    __shared__ int pm_c1[SP_PM], pm_c2[SP_PM];
    __shared__ int banv_s[SP_PM];
    float* xs = dyn;
    int* list = reinterpret_cast<int*>(dyn + a.K);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint16_t* W = reinterpret_cast<const uint16_t*>(a.w_exact);
    const int* bc = a.blk_cnt + (long)b * a.nblk;
    const float* bt = a.blk_t + (long)b * a.nblk;
    const long sb = (long)b * a.nblk * a.slot;
    const int* cx = a.ctx + (long)b * a.ctx_cap;
    const unsigned long long t0 = a.stats ? wall_clock64() : 0;
#define SP_STAMP(k) if (a.stats && tid == 0) a.stats[4 + (k)] += wall_clock64() - t0;
    // ---- token-independent loads
    const int n = a.ctx_len[b], g = ROWS ? a.rows[b].ngram : a.ngram;
    const int eos = ROWS ? a.rows[b].eos : a.eos;
    int done0 = 0, olen0 = 0, kvp0 = 0, kvl0 = 0;
    if (tid == 0) {
        if (a.out_ids) { done0 = a.done[b]; olen0 = a.out_len[b]; }
        if (a.kv_pos) { kvp0 = a.kv_pos[b]; kvl0 = a.kv_len[b]; }
        nlist = 0;
        pm_n = 0;
        nban_s = 0;
    }
    // per-block threshold and count (thread j < nblk), the first token of the two prefix-match
    // positions this thread checks, and the staged row: all in flight before the first barrier
    const bool ban = a.ban_out && g > 1 && n + 1 >= g - 1;
    const int last_i = n + 1 - g;  // next step's positions: 0 .. n+1-g
    const int jc = min(tid, a.nblk - 1);
    float T = bt[jc];
    const int c0 = bc[jc];
    // block jc's first E kept rows: they do not depend on T, so they load in this round trip too
    constexpr int E = 16;
    float h[E];
    int v[E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const long e = sb + (long)min(i, (int)a.slot - 1) * a.nblk + jc;
        h[i] = a.cand_hi[e];
        v[i] = a.cand[e];
    }
    if (tid >= a.nblk) T = -INFINITY;
    for (int j = tid + NT; j < a.nblk; j += NT) T = fmaxf(T, bt[j]);
    // (preloaded whatever g is; read only when the ban applies, g > 1, where the indices are below n: clamped to the
    // row for g < 2, where n + 1 - g and n + 2 - g reach past a full context)
    const int lc = min(max(last_i, 0), (int)a.ctx_cap - 1);
    const int pa = cx[min(tid, lc)], pb = cx[min(tid + NT, lc)], s0 = cx[min(max(n + 2 - g, 0), (int)a.ctx_cap - 1)];
    for (int k = tid * 4; k < a.K; k += NT * 4)
        *reinterpret_cast<float4*>(xs + k) = *reinterpret_cast<const float4*>(a.xn + (long)b * a.K + k);
    T = wave_max(T);
    if (lane == 0) sv[wave] = T;
    __syncthreads();
    T = sv[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) T = fmaxf(T, sv[w]);
    SP_STAMP(0)
    // ---- kept rows whose upper bound reaches T (a block's first E entries are already in registers)
    if (tid < a.nblk) {
        if (a.stats) atomicAdd(&nban_s, c0);  // (diagnostics: kept rows, reset below)
#pragma unroll
        for (int i = 0; i < E; ++i)
            if (i < c0 && h[i] >= T) {
                const int p = atomicAdd(&nlist, 1);
                if (p < SP_LIST) list[p] = v[i];
            }
        for (int i = E; i < c0; ++i) {
            const float hh = a.cand_hi[sb + (long)i * a.nblk + tid];
            const int vv = a.cand[sb + (long)i * a.nblk + tid];
            if (hh >= T) {
                const int p = atomicAdd(&nlist, 1);
                if (p < SP_LIST) list[p] = vv;
            }
        }
    }
    for (int j = tid + NT; j < a.nblk; j += NT) {  // more blocks than threads
        const int c = bc[j];
        for (int i = 0; i < c; ++i) {
            const float hh = a.cand_hi[sb + (long)i * a.nblk + j];
            const int vv = a.cand[sb + (long)i * a.nblk + j];
            if (hh >= T) {
                const int p = atomicAdd(&nlist, 1);
                if (p < SP_LIST) list[p] = vv;
            }
        }
    }
    SP_STAMP(6)
    // ---- next step's n-gram ban, prefix part: ctx'[i..i+g-3] == ctx[n+2-g..n-1] (first token
    // compared from the preloaded values; the rest only for the rare positions that pass)
    if (ban)
        for (int i = tid, r = 0; i <= last_i; i += NT, ++r) {
            const int first = r == 0 ? pa : (r == 1 ? pb : cx[i]);
            bool match = g < 3 || first == s0;
            for (int jj = 1; match && jj < g - 2; ++jj)
                if (cx[i + jj] != cx[n + 2 - g + jj]) match = false;
            if (match) {
                const int p = atomicAdd(&pm_n, 1);
                if (p < SP_PM) {
                    pm_c1[p] = cx[i + g - 2];                          // index <= n-1
                    pm_c2[p] = i + g - 1 < n ? cx[i + g - 1] : -1;     // -1: the new token
                }
            }
        }
    __syncthreads();
    SP_STAMP(1)
    const int nl = nlist;
    if (a.stats) {
        if (tid == 0) { a.stats[0] += 1; a.stats[1] += (unsigned long long)nban_s; a.stats[2] += (unsigned long long)nl; }
        __syncthreads();
        if (tid == 0) nban_s = 0;
    }
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    // at most one survivor per wave (the usual case: ~9 of 16 waves): each wave also loads its survivor's
    // embedding row now, so the next step's input row is in registers when the argmax is known (the gather
    // after the argmax was one more dependent round trip at the end of the step)
    constexpr int EU = 3;  // 16-byte chunks per lane of the embedding row (H <= 64 * 8 * EU)
    const bool emb_pre = a.table && nl <= NT / 64 && a.H % 8 == 0 && a.H <= 64 * 8 * EU;
    uint4 erow[EU];
    int ev = -1;
    if (emb_pre && wave < nl) {
        ev = list[wave];
        const uint16_t* tab = reinterpret_cast<const uint16_t*>(a.table) + (long)ev * a.H;
#pragma unroll
        for (int u = 0; u < EU; ++u) erow[u] = ldg_nt16(tab + (min(u * 64 + lane, a.H / 8 - 1) << 3));
    }
    screened_rescore(a, W, xs, list, nl, T, bc, sb, bv, bi);
    SP_STAMP(2)
    waves_argmax(bv, bi, sv2, si2);
    SP_STAMP(3)
    if (bi == 0x7fffffff) {
        // fallback (sampling.rs:34-96): argmax of every token ignoring the ban
        bv = -INFINITY;
        bi = 0x7fffffff;
        for (int v = wave; v < a.V; v += NT / 64) {
            const float x = a.w_exact_wdt == WDT_F16 ? exact_row_logit<f16_t>(W, v, a.K, xs) : exact_row_logit<bf16_t>(W, v, a.K, xs);
            if ((x > -INFINITY) && (x < INFINITY) && sp_better(x, v, bv, bi)) { bv = x; bi = v; }
        }
        __syncthreads();
        waves_argmax(bv, bi, sv2, si2);
    }
    const int t = bi == 0x7fffffff ? 0 : bi;
    // the next step's ban from the prefix matches into LDS first: the global stores below then need no barrier
    // after them (a barrier waits for the acknowledgement of every store before it)
    const bool ban_fast = a.ban_out && pm_n <= SP_PM;
    if (ban_fast) {
        for (int p = tid; p < pm_n; p += NT)
            if (pm_c1[p] == t) {
                const int q = atomicAdd(&nban_s, 1);
                banv_s[q] = pm_c2[p] < 0 ? t : pm_c2[p];  // q < pm_n <= SP_PM
            }
        __syncthreads();
    }
    if (tid == 0) {
        a.out_tok[b] = t;
        if (a.out_ids && !done0) {
            if (eos >= 0 && t == eos) {
                a.done[b] = 1;
            } else {
                if (olen0 < a.out_cap) { a.out_ids[(long)b * a.out_cap + olen0] = t; a.out_len[b] = olen0 + 1; }
                if (olen0 + 1 >= a.out_cap) a.done[b] = 1;
                if (n < a.ctx_cap) { a.ctx[(long)b * a.ctx_cap + n] = t; a.ctx_len[b] = n + 1; }
            }
        }
        if (a.kv_pos) {
            a.kv_pos[b] = kvp0 + 1;
            a.kv_len[b] = kvl0 + 1;
        }
    }
    if (a.table) {
        const bool hit = emb_pre && bi != 0x7fffffff && t == bi && __syncthreads_or(ev == t);
        if (hit) {  // the wave that holds the winner's row writes it
            if (ev == t) {
#pragma unroll
                for (int u = 0; u < EU; ++u) {
                    const int cc = u * 64 + lane;
                    if (cc < a.H / 8) {
                        float w8[8];
                        if (a.table_dt == WDT_BF16) unpack8<bf16_t>(erow[u], w8);
                        else unpack8<f16_t>(erow[u], w8);
                        float* d = a.x_next + (long)b * a.H + (cc << 3);
                        *reinterpret_cast<float4*>(d) = make_float4(w8[0], w8[1], w8[2], w8[3]);
                        *reinterpret_cast<float4*>(d + 4) = make_float4(w8[4], w8[5], w8[6], w8[7]);
                    }
                }
            }
        } else {
            const uint16_t* tab = reinterpret_cast<const uint16_t*>(a.table);
            for (int c = tid; c < a.H; c += NT) {
                const uint32_t bits = tab[(long)t * a.H + c];
                a.x_next[(long)b * a.H + c] = a.table_dt == WDT_BF16 ? bf16_bits_to_f32(bits) : f16_bits_to_f32(bits);
            }
        }
    }
    SP_STAMP(4)
    if (!a.ban_out) return;
    // (a page that did not take the token is done: its later selections are never read)
    int* out = a.ban_out + (long)b * a.ban_ld;
    if (ban_fast) {
        const int nb = nban_s;
        for (int q = tid; q < nb; q += NT)
            if (q + 1 < a.ban_ld) out[1 + q] = banv_s[q];
        if (tid == 0) out[0] = min(nb, (int)a.ban_ld - 1);
        SP_STAMP(5)
        return;
    } else {
        // too many prefix matches (tiny n-gram sizes): full scan of the updated context
        __syncthreads();
        const int n1 = n + 1;
        for (int i = tid; i <= n1 - g; i += NT) {
            bool match = true;
            for (int jj = 0; jj < g - 1; ++jj) {
                const int x0 = i + jj < n ? cx[i + jj] : t, x1 = n1 - g + 1 + jj < n ? cx[n1 - g + 1 + jj] : t;
                if (x0 != x1) { match = false; break; }
            }
            if (match) {
                const int q = atomicAdd(&nban_s, 1);
                if (q + 1 < a.ban_ld) out[1 + q] = i + g - 1 < n ? cx[i + g - 1] : t;
            }
        }
    }
    __syncthreads();
    if (tid == 0) out[0] = min(nban_s, (int)a.ban_ld - 1);
    SP_STAMP(5)
#undef SP_STAMP
}

template <int NT, bool ROWS>
__global__ __launch_bounds__(NT) void dec_sample_final_kernel(DecSampleArgs a) {
    __shared__ float sv[SP_BLOCK];
    __shared__ int si[SP_BLOCK];
    __shared__ int tok_s, nban_s;
    const int b = blockIdx.x;
    const int eos = ROWS ? a.rows[b].eos : a.eos;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int j = threadIdx.x; j < a.red_blocks; j += NT) {
        float v = a.red_val[(long)b * a.red_blocks + j];
        int i = a.red_idx[(long)b * a.red_blocks + j];
        if (i != 0x7fffffff && sp_better(v, i, bv, bi)) { bv = v; bi = i; }
    }
    block_argmax(bv, bi, sv, si);
    const bool found = si[0] != 0x7fffffff;
    __syncthreads();
    if (!found) {  // everything banned / non-finite: argmax of the penalised logits, else 0
        const float* lg = a.logits + (long)b * a.ld;
        bv = -INFINITY;
        bi = 0x7fffffff;
        for (int v = threadIdx.x; v < a.V; v += NT) {
            float x = lg[v];
            if (!(x > -INFINITY) || !(x < INFINITY)) continue;
            if (sp_better(x, v, bv, bi)) { bv = x; bi = v; }
        }
        sv[threadIdx.x] = bv;
        si[threadIdx.x] = bi;
        __syncthreads();
        for (int o = NT / 2; o > 0; o >>= 1) {
            if (threadIdx.x < o && sp_better(sv[threadIdx.x + o], si[threadIdx.x + o], sv[threadIdx.x], si[threadIdx.x])) {
                sv[threadIdx.x] = sv[threadIdx.x + o];
                si[threadIdx.x] = si[threadIdx.x + o];
            }
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) {
        const int t = si[0] == 0x7fffffff ? 0 : si[0];
        tok_s = t;
        nban_s = 0;
        a.out_tok[b] = t;
        if (a.out_ids && !a.done[b]) {
            if (eos >= 0 && t == eos) {
                a.done[b] = 1;
            } else {
                const int st = a.out_len[b];
                if (st < a.out_cap) { a.out_ids[(long)b * a.out_cap + st] = t; a.out_len[b] = st + 1; }
                if (st + 1 >= a.out_cap) a.done[b] = 1;
                const int n = a.ctx_len[b];
                if (n < a.ctx_cap) { a.ctx[(long)b * a.ctx_cap + n] = t; a.ctx_len[b] = n + 1; }
            }
        }
        if (a.kv_pos) {
            a.kv_pos[b] += 1;
            a.kv_len[b] += 1;
        }
    }
    __syncthreads();
    if (a.ban_out) {
        // the next step's banned tokens (sampling.rs:141-158 on the updated context)
        const int n = a.ctx_len[b], g = ROWS ? a.rows[b].ngram : a.ngram;
        const int* cx = a.ctx + (long)b * a.ctx_cap;
        int* out = a.ban_out + (long)b * a.ban_ld;
        if (g > 1 && n >= g - 1)
            for (int i = threadIdx.x; i <= n - g; i += NT) {
                bool match = true;
                for (int jj = 0; jj < g - 1; ++jj)
                    if (cx[i + jj] != cx[n - g + 1 + jj]) { match = false; break; }
                if (match) {
                    const int p = atomicAdd(&nban_s, 1);
                    if (p + 1 < a.ban_ld) out[1 + p] = cx[i + g - 1];
                }
            }
        __syncthreads();
        if (threadIdx.x == 0) out[0] = min(nban_s, (int)a.ban_ld - 1);
    }
    if (!a.table) return;
    const int t = tok_s;
    const uint16_t* tab = reinterpret_cast<const uint16_t*>(a.table);
    for (int c = threadIdx.x; c < a.H; c += NT) {
        const uint32_t bits = tab[(long)t * a.H + c];
        a.x_next[(long)b * a.H + c] = a.table_dt == WDT_BF16 ? bf16_bits_to_f32(bits) : f16_bits_to_f32(bits);
    }
}

void launch_dec_sample(const DecSampleArgs& a0, hipStream_t s) {
    DecSampleArgs a = a0;
    a.red_blocks = (int)dec_sample_blocks(a.V);
    // (with per-row parameters the caller picks the screened head only when no row samples)
    const bool screen = (a.rows || !a.do_sample) && a.blk_cnt && a.blk_t && a.cand && a.cand_hi && a.w_exact && a.xn && a.nblk > 0;
    if (a.ban_out && a.ban_ld < a.ctx_cap + 1) throw std::runtime_error("EINVAL: ban list shorter than the context");
    if (screen) {
        if (a.K % 8 || a.K > 1536) throw std::runtime_error("EINVAL: screened selection needs K % 8 == 0, K <= 1536");
        const size_t lds = sizeof(float) * a.K + sizeof(int) * SP_LIST;
        if (a.rows) DSOCR_LAUNCH((dec_screen_final_kernel<1024, true>), dim3(a.B), dim3(1024), lds, s, a);
        else DSOCR_LAUNCH((dec_screen_final_kernel<1024, false>), dim3(a.B), dim3(1024), lds, s, a);
        return;
    }
    if (a.rows) {
        // per-row exact head: both selectors every step (the mix of rows changes without the launches changing);
        // every row's selection slots are written by exactly one of them
        if (a.ctx_cap <= 16384) DSOCR_LAUNCH((dec_argmax_partial_kernel<true, true>), dim3(a.red_blocks, a.B), dim3(SP_BLOCK), sizeof(int) * a.ctx_cap, s, a);
        else DSOCR_LAUNCH((dec_argmax_partial_kernel<false, true>), dim3(a.red_blocks, a.B), dim3(SP_BLOCK), 0, s, a);
        launch_dec_stoch_select(a, s);
        DSOCR_LAUNCH((dec_sample_final_kernel<SP_BLOCK, true>), dim3(a.B), dim3(SP_BLOCK), 0, s, a);
        return;
    }
    if (a.do_sample) launch_dec_stoch_select(a, s);  // sampling.hip: the chosen id in selection slot 0
    else if (a.ctx_cap <= 16384) DSOCR_LAUNCH((dec_argmax_partial_kernel<true, false>), dim3(a.red_blocks, a.B), dim3(SP_BLOCK), sizeof(int) * a.ctx_cap, s, a);
    else DSOCR_LAUNCH((dec_argmax_partial_kernel<false, false>), dim3(a.red_blocks, a.B), dim3(SP_BLOCK), 0, s, a);
    DSOCR_LAUNCH((dec_sample_final_kernel<SP_BLOCK, false>), dim3(a.B), dim3(SP_BLOCK), 0, s, a);
}

}  // namespace dsocr
