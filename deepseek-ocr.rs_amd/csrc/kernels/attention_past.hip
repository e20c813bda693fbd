// Prefill attention behind a cached past, f32 end to end like attention.hip: every sequence brings n_q new rows
// (already rotated, their K / V rows already appended) and attends them causally to the past + n_q rows its cache
// now holds.  Query row i sits at position past + i and sees keys [0, past + i].  Two kernels serve the one contract
// (attn_behind_past_ok), both on the shared tile of attn_tile.hpp: a wave stages a K tile in its own slice of LDS
// (row pitch hd + 4 floats: the 16-byte fragment reads of 32 rows fall on distinct banks), computes S^T = K.Q^T on
// v_mfma_f32_32x32x2_f32 with the lane's own query in the accumulator column, takes the softmax of its 32 keys and
// feeds P straight from that accumulator into O^T = V^T.P^T (keys in the accumulator's permuted order; V rows are
// read from the cache as they are: 32 lanes, 32 consecutive floats of one row).  Products are exact f32, as in
// attention_fwd2.
//
// attention_past: split over the keys.  The new rows are few (a prompt suffix behind a cached page is a handful of
// rows against ~700 keys), so the parallelism comes from the keys, not from the queries:
//   * attention_past_kernel: one workgroup per (128-key piece, head, sequence x 32-query tile), four waves, wave w
//     owning keys [32 w, 32 w + 32) of the piece.  It writes its unnormalised (m, l, O[hd]) per query to the
//     workspace.
//   * attention_past_merge_kernel, a second launch: thread (query, d) combines the query's records in key order
//     (m = max m_i, l = sum l_i e^(m_i - m), o = sum o_i e^(m_i - m), out = o / l).
// Nothing is handed over inside a launch: a wave reads only the caches and writes only its own records; the kernel
// boundary orders the records before the combine.
//
// attention_chunk: tiled over the queries, the shape a chunked prefill needs: many new rows behind a few hundred keys.
//   * One workgroup per (32-query tile, head, sequence), eight waves.  Wave w owns the 32-key tiles w, w + 8, ... of
//     the keys [0, past + last query of the tile] and visits them in ascending order with an online softmax of its
//     own, rescaling its running (m, l, O^T) per tile.  Nothing is shared between waves until then, so the key loop
//     has no workgroup barrier.
//   * When the tiles are done every wave leaves its (m, l, O) per query in its LDS slice (the K tile is dead by
//     then) and, after one barrier, thread (query, d) combines the eight records in wave order and writes o.
// One launch, no record buffer in memory, nothing handed from one workgroup to another.
//
// Sizes of attention_chunk.  32 queries per workgroup is the MFMA's accumulator width.  Eight waves: a 128-row chunk
// with 10 heads is only 40 workgroups, so the keys of a tile are spread over as many waves as the LDS holds at hd 128
// (8 x 32 x 132 x 4 B = 132 KB of the CU's 160 KB; one workgroup per CU, which 40 workgroups never exceed).  At 512
// threads a lane may hold 256 registers; hd 128 needs 64 (q) + 64 (O^T) + 16 (S^T) + addressing, no spill.
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "attn_tile.hpp"
#include "dev_common.hpp"
#include "kernels.hpp"

namespace dsocr {

constexpr int PA_Q = ATTN_TILE;   // queries per tile (one accumulator column per lane pair)
constexpr int PA_KT = ATTN_TILE;  // keys per tile
constexpr int PA_WAVES = 4;       // attention_past: waves per workgroup, a piece of 128 keys
constexpr int CA_WAVES = 8;       // attention_chunk: waves per workgroup, each with its own key tiles and running softmax

// a wave's K tile into its LDS slice: rows clamped to the last visible key (a clamped row's scores are masked by
// the caller)
template <int HD>
__device__ __forceinline__ void pa_stage_k(float* Ks, const float* K, long row_stride, int k0, int last_key, int lane) {
#pragma unroll
    for (int j = 0; j < HD / 8; ++j) {
        const int f = lane + 64 * j;
        const int row = f / (HD / 4), c4 = (f % (HD / 4)) * 4;
        const int key = min(k0 + row, last_key);
        *reinterpret_cast<float4*>(&Ks[row * (HD + 4) + c4]) = *reinterpret_cast<const float4*>(K + (long)key * row_stride + c4);
    }
}

// accumulator register r of lane (half, l32): key k0 + attn_tile_key(r, half), query l32; scaled, and masked past
// the query's own position
__device__ __forceinline__ void pa_scale_mask(f32x16& sc, float scale, int k0, int half, int last_key) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int key = k0 + attn_tile_key(r, half);
        sc[r] = key > last_key ? -INFINITY : sc[r] * scale;
    }
}

template <int HD>
__global__ __launch_bounds__(64 * PA_WAVES) void attention_past_kernel(AttnPastArgs a) {
    constexpr int KP = HD + 4;
    extern __shared__ __attribute__((aligned(16))) float pa_lds[];
    const int nqt = (a.max_q + PA_Q - 1) / PA_Q, nkt = (a.max_total + PA_KT - 1) / PA_KT;
    const int s = blockIdx.z / nqt, qt = blockIdx.z % nqt, h = blockIdx.y;
    const int past = a.past[s], nq = a.n_q[s];
    const int q0 = qt * PA_Q;
    if (q0 >= nq) return;
    const int kend = past + min(nq, q0 + PA_Q);  // keys [0, kend): what the tile's last query sees
    if ((int)blockIdx.x * PA_WAVES * PA_KT >= kend) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l32 = lane & 31;
    const int kvh = h / (a.heads / a.kv_heads);
    const int ktile = blockIdx.x * PA_WAVES + wave, k0 = ktile * PA_KT;
    const float* Q = a.q.ptr + a.q.seq_off[s] + (long)h * a.q.head_stride;
    const float* K = a.k.ptr + a.k.seq_off[s] + (long)kvh * a.k.head_stride;
    const float* V = a.v.ptr + a.v.seq_off[s] + (long)kvh * a.v.head_stride;
    float* Ks = pa_lds + wave * PA_KT * KP;
    pa_stage_k<HD>(Ks, K, a.k.row_stride, k0, kend - 1, lane);
    __syncthreads();
    if (k0 >= kend) return;  // (wave-uniform; no barrier follows)
    const int q_lane = q0 + l32;  // lanes l and l + 32 share a query and split the head dims
    const bool q_valid = q_lane < nq;
    float qreg[HD / 2];
    attn_tile_load_q<HD>(Q + (long)(q_valid ? q_lane : 0) * a.q.row_stride, half, qreg);
    f32x16 sc;
    attn_tile_scores<HD>(Ks + l32 * KP, half, qreg, sc);
    pa_scale_mask(sc, a.scale, k0, half, past + q_lane);
    // the wave's only tile: its (m, l) are the tile's, and O^T starts from zero
    const float m = attn_tile_max(sc);
    const float l = attn_tile_exp(sc, m);
    f32x16 o[HD / 32];
#pragma unroll
    for (int t = 0; t < HD / 32; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
    attn_tile_pv_rows<HD>(V, a.v.row_stride, k0, kend - 1, half, l32, sc, o);
    if (!q_valid) return;
    float* rec = a.part + (((((long)s * a.heads + h) * nqt + qt) * nkt + ktile) * PA_Q + l32) * (HD + 2);
    attn_rec_write<HD>(rec, 2, half, m, l, o);
}

// thread (query, d): the query's key tiles [0, ceil((past + q + 1) / 32)) were all written by the launch before
template <int HD>
__global__ __launch_bounds__(256) void attention_past_merge_kernel(AttnPastArgs a) {
    const int s = blockIdx.z, h = blockIdx.y;
    const int past = a.past[s], nq = a.n_q[s];
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int q = (int)(idx / HD), d = (int)(idx % HD);
    if (q >= nq) return;
    const int nqt = (a.max_q + PA_Q - 1) / PA_Q, nkt = (a.max_total + PA_KT - 1) / PA_KT;
    const int qt = q / PA_Q, ql = q % PA_Q;
    const int n = (past + q + PA_KT) / PA_KT;
    const float* rec0 = a.part + (((((long)s * a.heads + h) * nqt + qt) * nkt) * PA_Q + ql) * (HD + 2);
    a.o[a.o_seq_off[s] + (long)q * a.o_row_stride + (long)h * a.o_head_stride + d] =
        attn_rec_combine(rec0, (long)PA_Q * (HD + 2), n, 2, d);
}

template <int HD>
__global__ __launch_bounds__(64 * CA_WAVES) void attention_chunk_kernel(AttnPastArgs a) {
    constexpr int KP = HD + 4;
    extern __shared__ __attribute__((aligned(16))) float ca_lds[];
    const int s = blockIdx.z, qt = blockIdx.x, h = blockIdx.y;
    const int past = a.past[s], nq = a.n_q[s];
    const int q0 = qt * PA_Q;
    if (q0 >= nq) return;  // (the whole workgroup)
    const int kend = past + min(nq, q0 + PA_Q);  // keys [0, kend): what the tile's last query sees
    const int ntile = (kend + PA_KT - 1) / PA_KT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l32 = lane & 31;
    const int kvh = h / (a.heads / a.kv_heads);
    const float* Q = a.q.ptr + a.q.seq_off[s] + (long)h * a.q.head_stride;
    const float* K = a.k.ptr + a.k.seq_off[s] + (long)kvh * a.k.head_stride;
    const float* V = a.v.ptr + a.v.seq_off[s] + (long)kvh * a.v.head_stride;
    float* Ks = ca_lds + wave * PA_KT * KP;
    const int q_lane = q0 + l32;  // lanes l and l + 32 share a query and split the head dims
    const bool q_valid = q_lane < nq;
    float qreg[HD / 2];
    attn_tile_load_q<HD>(Q + (long)(q_valid ? q_lane : 0) * a.q.row_stride, half, qreg);
    float m_run = -INFINITY, l_run = 0.f;
    f32x16 o[HD / 32];
#pragma unroll
    for (int t = 0; t < HD / 32; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
    // Inside the loop a wave touches only its own LDS slice, and a wave's LDS instructions execute in issue order, so
    // the staged tile needs no workgroup barrier: a wavefront-scope fence keeps the compiler from moving the fragment
    // reads above the stores (or the next tile's stores above this tile's reads).  Waves run their own trip counts.
    for (int kt = wave; kt < ntile; kt += CA_WAVES) {
        const int k0 = kt * PA_KT;
        pa_stage_k<HD>(Ks, K, a.k.row_stride, k0, kend - 1, lane);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        {
            f32x16 sc;
            attn_tile_scores<HD>(Ks + l32 * KP, half, qreg, sc);
            pa_scale_mask(sc, a.scale, k0, half, past + q_lane);
            // (a query that sees no key of the tile and none before it in this wave: nothing changes)
            attn_tile_softmax<HD>(sc, m_run, l_run, o);
            attn_tile_pv_rows<HD>(V, a.v.row_stride, k0, kend - 1, half, l32, sc, o);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // this tile's fragment reads are issued before the next tile's stores
    }
    // the wave's record per query in its own slice: [0] m, [1] l, [4 + d] O (after its last tile's reads, as above)
    attn_rec_write<HD>(Ks + l32 * KP, 4, half, m_run, l_run, o);
    __syncthreads();
    // thread (query, d): the eight records in wave order (a wave that saw no key of the query left m = -inf)
    for (int idx = tid; idx < PA_Q * HD; idx += 64 * CA_WAVES) {
        const int q = idx / HD, d = idx % HD;
        if (q0 + q >= nq) continue;
        a.o[a.o_seq_off[s] + (long)(q0 + q) * a.o_row_stride + (long)h * a.o_head_stride + d] =
            attn_rec_combine(ca_lds + q * KP, PA_KT * KP, CA_WAVES, 4, d);
    }
}

size_t attention_past_part_floats(int n_seq, int heads, int max_q, int max_total, int hd) {
    const size_t nqt = (size_t)(max_q + PA_Q - 1) / PA_Q, nkt = (size_t)(max_total + PA_KT - 1) / PA_KT;
    return (size_t)n_seq * heads * nqt * nkt * PA_Q * (hd + 2);
}

// what both kernels ask of an AttnPastArgs
static bool attn_behind_past_ok(const AttnPastArgs& a) {
    if (a.hd != 32 && a.hd != 64 && a.hd != 128) return false;
    if (a.n_seq <= 0 || a.heads <= 0 || a.kv_heads <= 0 || a.heads % a.kv_heads) return false;
    if (a.max_q < 1 || a.max_total < a.max_q) return false;
    if (!a.q.ptr || !a.k.ptr || !a.v.ptr || !a.o || !a.past || !a.n_q) return false;
    if (!a.q.seq_off || !a.k.seq_off || !a.v.seq_off || !a.o_seq_off) return false;
    // 16-byte loads of q and k rows
    if (a.q.row_stride % 4 || a.q.head_stride % 4 || a.k.row_stride % 4 || a.k.head_stride % 4) return false;
    if (a.q.row_stride < a.hd || a.k.row_stride < a.hd || a.v.row_stride < a.hd) return false;
    if ((reinterpret_cast<uintptr_t>(a.q.ptr) | reinterpret_cast<uintptr_t>(a.k.ptr)) & 15) return false;
    return a.heads <= 65535;  // grid y
}

bool attention_past_ok(const AttnPastArgs& a) {
    if (!attn_behind_past_ok(a)) return false;
    const long nqt = (a.max_q + PA_Q - 1) / PA_Q;
    if ((long)a.n_seq * nqt > 65535) return false;  // grid z
    return a.part && a.part_floats >= attention_past_part_floats(a.n_seq, a.heads, a.max_q, a.max_total, a.hd);
}

bool attention_chunk_ok(const AttnPastArgs& a) { return attn_behind_past_ok(a) && a.n_seq <= 65535; }

// dynamic LDS above 64 KB (set at every launch: cheap, and right on every device)
static void pa_allow_lds(const void* kernel, size_t lds, const char* who) {
    if (lds <= 64 * 1024) return;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess)
        throw std::runtime_error(std::string("EDEVICE: ") + who + ": dynamic LDS limit: " + hipGetErrorString(e));
}

template <int HD>
static void launch_past_hd(const AttnPastArgs& a, hipStream_t s) {
    const size_t lds = (size_t)PA_WAVES * PA_KT * (HD + 4) * sizeof(float);  // hd 128: 66 KB
    pa_allow_lds(reinterpret_cast<const void*>(&attention_past_kernel<HD>), lds, "attention_past");
    const int nqt = (a.max_q + PA_Q - 1) / PA_Q;
    const dim3 g1((a.max_total + PA_WAVES * PA_KT - 1) / (PA_WAVES * PA_KT), a.heads, a.n_seq * nqt);
    const dim3 g2((unsigned)(((long)a.max_q * HD + 255) / 256), a.heads, a.n_seq);
    DSOCR_LAUNCH(attention_past_kernel<HD>, g1, dim3(64 * PA_WAVES), lds, s, a);
    DSOCR_LAUNCH(attention_past_merge_kernel<HD>, g2, dim3(256), 0, s, a);
}

template <int HD>
static void launch_chunk_hd(const AttnPastArgs& a, hipStream_t s) {
    const size_t lds = (size_t)CA_WAVES * PA_KT * (HD + 4) * sizeof(float);  // above 64 KB at hd 64 and 128
    pa_allow_lds(reinterpret_cast<const void*>(&attention_chunk_kernel<HD>), lds, "attention_chunk");
    const dim3 g((a.max_q + PA_Q - 1) / PA_Q, a.heads, a.n_seq);
    DSOCR_LAUNCH(attention_chunk_kernel<HD>, g, dim3(64 * CA_WAVES), lds, s, a);
}

void launch_attention_past(const AttnPastArgs& a, hipStream_t s) {
    if (!attention_past_ok(a)) throw std::runtime_error("EINVAL: attention_past: shape outside the kernel's contract");
    if (a.hd == 128) launch_past_hd<128>(a, s);
    else if (a.hd == 64) launch_past_hd<64>(a, s);
    else launch_past_hd<32>(a, s);
}

void launch_attention_chunk(const AttnPastArgs& a, hipStream_t s) {
    if (!attention_chunk_ok(a)) throw std::runtime_error("EINVAL: attention_chunk: shape outside the kernel's contract");
    if (a.hd == 128) launch_chunk_hd<128>(a, s);
    else if (a.hd == 64) launch_chunk_hd<64>(a, s);
    else launch_chunk_hd<32>(a, s);
}

}  // namespace dsocr
