// Hybrid-mask grouped-query attention of the DeepSeek-OCR-2 vision encoder (vision/qwen2.rs:519-571), f32 end to
// end like attention.hip.  A sequence is [P image rows | L - P query rows]; row i sees key j iff
//     j < P  or  (i >= P and j <= i):
// image rows see every image key and no query key, query rows see every image key and the queries up to
// themselves.  The reference adds f32::MIN to the masked scores, which an f32 softmax turns into exact zeros, so
// leaving those keys out is the same result.
//
// Structure:
//   * One workgroup owns 32 query rows of one KV head and ALL the query heads of that KV group (one wave per
//     head, 7 at the real shape): a K/V tile of 32 keys is staged in LDS once and read by every head, where
//     attention_fwd2 restages it per head.
//   * Row blocks never mix the two row kinds (image blocks tile [0, P), query blocks tile [P, L)), so a block
//     knows its last visible key: P for an image block, its own last row for a query block.  Tiles past it are
//     never visited, and keys past it inside the last tile are staged as zeros (nothing is read from them).
//   * The element mask runs only on the tiles that straddle P or the diagonal; every other tile is all visible.
//   * The math is attention_fwd2's (the shared tile of attn_tile.hpp): S^T = K.Q^T on v_mfma_f32_32x32x2_f32 with
//     the lane's own query in the accumulator column, P fed to the O^T = V^T.P^T MFMA straight from that accumulator (keys in its permuted
//     order), online softmax without cross-lane shuffles, tile t + 1 in registers while tile t is consumed.
//   * Synchronisation is the in-block LDS barrier only (one per tile); the sequences are short (288 / 512 rows),
//     so the keys are not split across workgroups.
#include <algorithm>
#include <cstdint>
#include <stdexcept>

#include "attn_tile.hpp"
#include "dev_common.hpp"
#include "kernels.hpp"

namespace dsocr {

constexpr int AP_Q = 32;   // query rows per workgroup (per wave: one head each)
constexpr int AP_KT = 32;  // keys per tile

// NW waves: wave w computes head (chunk * NW + w) of the KV group (idle when the group has fewer heads; it
// still stages its share of every tile)
template <int HD, int NW>
__global__ __launch_bounds__(64 * NW) void attention_prefix_kernel(AttnPrefixArgs a) {
    constexpr int NT = 64 * NW, KP = HD + 4, VP = AP_KT + 4;
    constexpr int F4T = AP_KT * HD / 4;         // float4 per operand per tile
    constexpr int FPT = (F4T + NT - 1) / NT;    // ... per thread
    __shared__ __attribute__((aligned(16))) float Ks[2][AP_KT][KP];
    __shared__ __attribute__((aligned(16))) float Vt[2][HD][VP];
    const int P = a.prefix, L = a.L;
    const int nbi = (P + AP_Q - 1) / AP_Q;
    // rows [r0, r1) of this block and one past its last visible key
    int r0, r1, kend;
    if ((int)blockIdx.x < nbi) {
        r0 = blockIdx.x * AP_Q;
        r1 = min(P, r0 + AP_Q);
        kend = P;
    } else {
        r0 = P + ((int)blockIdx.x - nbi) * AP_Q;
        r1 = min(L, r0 + AP_Q);
        kend = r1;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l32 = lane & 31;
    const int G = a.heads / a.kv_heads, chunks = (G + NW - 1) / NW;
    const int kvh = blockIdx.y / chunks, hg = (blockIdx.y % chunks) * NW + wave;
    const bool active = hg < G;
    const int h = kvh * G + (active ? hg : 0);
    const long row0 = (long)blockIdx.z * L;
    const float* Q = a.q + row0 * a.ldq + (long)h * HD;
    const float* K = a.k + row0 * a.ldk + (long)kvh * HD;
    const float* V = a.v + row0 * a.ldv + (long)kvh * HD;
    const int q_lane = r0 + l32;
    const bool q_valid = active && q_lane < r1;
    float qreg[HD / 2];
    attn_tile_load_q<HD>(Q + (long)min(q_lane, r1 - 1) * a.ldq, half, qreg);
    // staging: thread covers float4 f = tid + NT j of the tile (clamped to the last one: a duplicate writes the
    // same value): key f / (HD/4), cols (f % (HD/4)) * 4; keys at or past kend come out as zeros
    // (macros, not lambdas: a captured register array is demoted to scratch)
    float4 rk[FPT], rv[FPT];
#define AP_GLOAD(K0)                                                                           \
    _Pragma("unroll") for (int j = 0; j < FPT; ++j) {                                          \
        const int f = min(tid + NT * j, F4T - 1);                                              \
        const int key = (K0) + f / (HD / 4);                                                   \
        const int kc = min(key, kend - 1);                                                     \
        const int c4 = (f % (HD / 4)) * 4;                                                     \
        rk[j] = *reinterpret_cast<const float4*>(K + (long)kc * a.ldk + c4);                   \
        rv[j] = *reinterpret_cast<const float4*>(V + (long)kc * a.ldv + c4);                   \
        if (key >= kend) rk[j] = rv[j] = make_float4(0.f, 0.f, 0.f, 0.f);                      \
    }
#define AP_LSTORE(BUF)                                                                         \
    _Pragma("unroll") for (int j = 0; j < FPT; ++j) {                                          \
        const int f = min(tid + NT * j, F4T - 1);                                              \
        const int kr = f / (HD / 4), c4 = (f % (HD / 4)) * 4;                                  \
        *reinterpret_cast<float4*>(&Ks[BUF][kr][c4]) = rk[j];                                  \
        Vt[BUF][c4 + 0][kr] = rv[j].x;                                                         \
        Vt[BUF][c4 + 1][kr] = rv[j].y;                                                         \
        Vt[BUF][c4 + 2][kr] = rv[j].z;                                                         \
        Vt[BUF][c4 + 3][kr] = rv[j].w;                                                         \
    }
    f32x16 o[HD / 32];
#pragma unroll
    for (int t = 0; t < HD / 32; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    AP_GLOAD(0);
    AP_LSTORE(0);
    __syncthreads();
    int buf = 0;
    for (int k0 = 0; k0 < kend; k0 += AP_KT, buf ^= 1) {
        AP_GLOAD(k0 + AP_KT);  // unconditional (clamped keys)
        if (active) {
            // S^T = K . Q^T: lane (half, l32) feeds dims i + half*HD/2
            f32x16 sc;
            attn_tile_scores<HD>(&Ks[buf][l32][0], half, qreg, sc);
            // all of the tile visible to every row of the block: it lies inside the prefix, or the block is a
            // query block and the tile ends at or before its first row (block-uniform)
            const bool all_visible = k0 + AP_KT <= P || (r0 >= P && k0 + AP_KT - 1 <= r0);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = k0 + attn_tile_key(r, half);
                float v = sc[r] * a.scale;
                if (!all_visible && !(key < P || (q_lane >= P && key <= q_lane))) v = -INFINITY;
                sc[r] = v;
            }
            attn_tile_softmax<HD>(sc, m_run, l_run, o);
            // O^T += V^T . P^T, keys in the accumulator's permuted order
            attn_tile_pv_lds<HD>(&Vt[buf][0][0], half, l32, sc, o);
        }
        AP_LSTORE(buf ^ 1);
        __syncthreads();
    }
    // O^T accumulator: row = d (within t), column = this lane's query; registers 4g .. 4g+3 are 4 adjacent dims
    if (q_valid) {
        float* op = a.o + (row0 + q_lane) * a.ldo + (long)h * HD;
#pragma unroll
        for (int t = 0; t < HD / 32; ++t)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                *reinterpret_cast<float4*>(op + t * 32 + 8 * g4 + 4 * half) =
                    make_float4(o[t][4 * g4] / l_run, o[t][4 * g4 + 1] / l_run, o[t][4 * g4 + 2] / l_run, o[t][4 * g4 + 3] / l_run);
    }
#undef AP_GLOAD
#undef AP_LSTORE
}

bool attention_prefix_ok(const AttnPrefixArgs& a) {
    if (a.n_seq <= 0 || a.L <= 0 || a.heads <= 0 || a.kv_heads <= 0) return false;
    if (a.hd != 32 && a.hd != 64) return false;
    if (a.heads % a.kv_heads) return false;
    if (a.prefix < 0 || a.prefix > a.L) return false;
    if (a.n_seq > 65535) return false;
    if (!a.q || !a.k || !a.v || !a.o) return false;
    // 16-byte row loads / stores
    if (a.ldq % 4 || a.ldk % 4 || a.ldv % 4 || a.ldo % 4) return false;
    if (a.ldq < (long)a.heads * a.hd || a.ldo < (long)a.heads * a.hd || a.ldk < (long)a.kv_heads * a.hd ||
        a.ldv < (long)a.kv_heads * a.hd)
        return false;
    for (const void* p : {(const void*)a.q, (const void*)a.k, (const void*)a.v, (const void*)a.o})
        if (reinterpret_cast<uintptr_t>(p) & 15) return false;
    return true;
}

template <int HD>
static void launch_prefix_hd(const AttnPrefixArgs& a, dim3 grid, int nw, hipStream_t s) {
    switch (nw) {
        case 1: hipLaunchKernelGGL((attention_prefix_kernel<HD, 1>), grid, dim3(64), 0, s, a); break;
        case 2: hipLaunchKernelGGL((attention_prefix_kernel<HD, 2>), grid, dim3(128), 0, s, a); break;
        case 4: hipLaunchKernelGGL((attention_prefix_kernel<HD, 4>), grid, dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL((attention_prefix_kernel<HD, 8>), grid, dim3(512), 0, s, a); break;
    }
}

void launch_attention_prefix(const AttnPrefixArgs& a, hipStream_t s) {
    if (!attention_prefix_ok(a)) throw std::runtime_error("EINVAL: attention_prefix: shape outside the kernel's contract");
    const int G = a.heads / a.kv_heads;
    const int nw = G <= 1 ? 1 : G <= 2 ? 2 : G <= 4 ? 4 : 8;  // waves per workgroup: the heads of a KV group, 8 at most
    const int chunks = (G + nw - 1) / nw;
    const int nblk = (a.prefix + AP_Q - 1) / AP_Q + (a.L - a.prefix + AP_Q - 1) / AP_Q;
    const dim3 grid(nblk, a.kv_heads * chunks, a.n_seq);
    if (a.hd == 64) launch_prefix_hd<64>(a, grid, nw, s);
    else launch_prefix_hd<32>(a, grid, nw, s);
}

}  // namespace dsocr
