// Prefill attention of a chunk behind a cached past, tiled over the queries: the contract of attention_past.hip
// (every sequence brings n_q new rows, already rotated, their K / V rows already appended; query row i sits at
// position past + i and sees keys [0, past + i]), in the shape a chunked prefill needs: many new rows behind a few
// hundred keys.
//
//   * One workgroup per (32-query tile, head, sequence), eight waves.  Wave w owns the 32-key tiles w, w + 8, ... of
//     the keys [0, past + last query of the tile] and visits them in ascending order with an online softmax of its
//     own: it stages the K tile in its slice of LDS (row pitch hd + 4 floats: the 16-byte fragment reads of 32 rows
//     fall on distinct banks), computes S^T = K.Q^T on v_mfma_f32_32x32x2_f32 with the lane's own query in the
//     accumulator column, rescales its running (m, l, O^T) and feeds P straight from that accumulator into
//     O^T += V^T.P^T (V rows read from the cache as they are).  Products are exact f32, as in attention_past.
//     Nothing is shared between waves until then, so the key loop has no workgroup barrier.
//   * When the tiles are done every wave leaves its (m, l, O) per query in its LDS slice (the K tile is dead by
//     then) and, after one barrier, thread (query, d) combines the eight records in wave order and writes o.
// One launch, no record buffer in memory, nothing handed from one workgroup to another.
//
// Sizes.  32 queries per workgroup is the MFMA's accumulator width.  Eight waves: a 128-row chunk with 10 heads is
// only 40 workgroups, so the keys of a tile are spread over as many waves as the LDS holds at hd 128
// (8 x 32 x 132 x 4 B = 132 KB of the CU's 160 KB; one workgroup per CU, which 40 workgroups never exceed).  At 512
// threads a lane may hold 256 registers; hd 128 needs 64 (q) + 64 (O^T) + 16 (S^T) + addressing, no spill.
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "dev_common.hpp"
#include "kernels.hpp"

namespace dsocr {

constexpr int CA_Q = 32;      // queries per workgroup (one accumulator column per lane pair)
constexpr int CA_KT = 32;     // keys per tile
constexpr int CA_WAVES = 8;   // waves per workgroup, each with its own key tiles and its own running softmax

template <int HD>
__global__ __launch_bounds__(64 * CA_WAVES) void attention_chunk_kernel(AttnPastArgs a) {
    constexpr int KP = HD + 4;
    extern __shared__ __attribute__((aligned(16))) float ca_lds[];
    const int s = blockIdx.z, qt = blockIdx.x, h = blockIdx.y;
    const int past = a.past[s], nq = a.n_q[s];
    const int q0 = qt * CA_Q;
    if (q0 >= nq) return;  // (the whole workgroup)
    const int kend = past + min(nq, q0 + CA_Q);  // keys [0, kend): what the tile's last query sees
    const int ntile = (kend + CA_KT - 1) / CA_KT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l32 = lane & 31;
    const int kvh = h / (a.heads / a.kv_heads);
    const float* Q = a.q.ptr + a.q.seq_off[s] + (long)h * a.q.head_stride;
    const float* K = a.k.ptr + a.k.seq_off[s] + (long)kvh * a.k.head_stride;
    const float* V = a.v.ptr + a.v.seq_off[s] + (long)kvh * a.v.head_stride;
    float* Ks = ca_lds + wave * CA_KT * KP;
    const int q_lane = q0 + l32;  // lanes l and l + 32 share a query and split the head dims
    const bool q_valid = q_lane < nq;
    const int last_key = past + q_lane;
    float qreg[HD / 2];
    {
        const float* qr = Q + (long)(q_valid ? q_lane : 0) * a.q.row_stride + half * (HD / 2);
#pragma unroll
        for (int i = 0; i < HD / 2; i += 4) {
            const float4 v4 = *reinterpret_cast<const float4*>(qr + i);
            qreg[i] = v4.x; qreg[i + 1] = v4.y; qreg[i + 2] = v4.z; qreg[i + 3] = v4.w;
        }
    }
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
        const int k0 = kt * CA_KT;
        {
            // this wave's K tile: rows clamped to the last visible key (a clamped row's scores are masked below)
#pragma unroll
            for (int j = 0; j < HD / 8; ++j) {
                const int f = lane + 64 * j;
                const int row = f / (HD / 4), c4 = (f % (HD / 4)) * 4;
                const int key = min(k0 + row, kend - 1);
                *reinterpret_cast<float4*>(&Ks[row * KP + c4]) = *reinterpret_cast<const float4*>(K + (long)key * a.k.row_stride + c4);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        {
            f32x16 sc;
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[r] = 0.f;
#pragma unroll
            for (int i = 0; i < HD / 2; i += 4) {
                const float4 k4 = *reinterpret_cast<const float4*>(&Ks[l32 * KP + half * (HD / 2) + i]);
                sc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.x, qreg[i], sc, 0, 0, 0);
                sc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.y, qreg[i + 1], sc, 0, 0, 0);
                sc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.z, qreg[i + 2], sc, 0, 0, 0);
                sc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.w, qreg[i + 3], sc, 0, 0, 0);
            }
            // accumulator register r of lane (half, l32): key k0 + kappa(r, half), query l32
            float mt = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * half;
                const float v = key > last_key ? -INFINITY : sc[r] * a.scale;
                sc[r] = v;
                mt = fmaxf(mt, v);
            }
            mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
            const float m_new = fmaxf(m_run, mt);
            // (m_new == -inf: this query sees no key of the tile and none before it in this wave: nothing changes)
            const float alpha = (m_run == -INFINITY) ? 0.f : __expf(m_run - m_new);
            float lt = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = (m_new == -INFINITY) ? 0.f : __expf(sc[r] - m_new);
                sc[r] = p;
                lt += p;
            }
            lt += __shfl_xor(lt, 32, 64);
            l_run = l_run * alpha + lt;
            m_run = m_new;
#pragma unroll
            for (int t = 0; t < HD / 32; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[t][r] *= alpha;
            // O^T += V^T . P^T over the tile's keys in the accumulator's order; masked keys carry p = 0 and read a
            // clamped (written) row
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int key = min(k0 + 8 * g4 + 4 * half + j, kend - 1);
                    const float* vr = V + (long)key * a.v.row_stride + l32;
#pragma unroll
                    for (int t = 0; t < HD / 32; ++t)
                        o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[t * 32], sc[4 * g4 + j], o[t], 0, 0, 0);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // this tile's fragment reads are issued before the next tile's stores
    }
    // the wave's record per query in its own slice: [0] m, [1] l, [4 + d] O (after its last tile's reads, as above)
    {
        float* rec = Ks + l32 * KP;
        if (half == 0) { rec[0] = m_run; rec[1] = l_run; }
#pragma unroll
        for (int t = 0; t < HD / 32; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) rec[4 + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * half] = o[t][r];
    }
    __syncthreads();
    // thread (query, d): the eight records in wave order (a wave that saw no key of the query left m = -inf)
    for (int idx = tid; idx < CA_Q * HD; idx += 64 * CA_WAVES) {
        const int q = idx / HD, d = idx % HD;
        if (q0 + q >= nq) continue;
        const float* rec0 = ca_lds + q * KP;
        float m = -INFINITY;
#pragma unroll
        for (int w = 0; w < CA_WAVES; ++w) m = fmaxf(m, rec0[w * CA_KT * KP]);
        float l = 0.f, acc = 0.f;
#pragma unroll
        for (int w = 0; w < CA_WAVES; ++w) {
            const float* r = rec0 + w * CA_KT * KP;
            const float wt = r[0] == -INFINITY ? 0.f : __expf(r[0] - m);
            l += r[1] * wt;
            acc += r[4 + d] * wt;
        }
        a.o[a.o_seq_off[s] + (long)(q0 + q) * a.o_row_stride + (long)h * a.o_head_stride + d] = acc / l;
    }
}

bool attention_chunk_ok(const AttnPastArgs& a) {
    if (a.hd != 32 && a.hd != 64 && a.hd != 128) return false;
    if (a.n_seq <= 0 || a.heads <= 0 || a.kv_heads <= 0 || a.heads % a.kv_heads) return false;
    if (a.max_q < 1 || a.max_total < a.max_q) return false;
    if (!a.q.ptr || !a.k.ptr || !a.v.ptr || !a.o || !a.past || !a.n_q) return false;
    if (!a.q.seq_off || !a.k.seq_off || !a.v.seq_off || !a.o_seq_off) return false;
    // 16-byte loads of q and k rows
    if (a.q.row_stride % 4 || a.q.head_stride % 4 || a.k.row_stride % 4 || a.k.head_stride % 4) return false;
    if (a.q.row_stride < a.hd || a.k.row_stride < a.hd || a.v.row_stride < a.hd) return false;
    if ((reinterpret_cast<uintptr_t>(a.q.ptr) | reinterpret_cast<uintptr_t>(a.k.ptr)) & 15) return false;
    if (a.heads > 65535 || a.n_seq > 65535) return false;
    return true;
}

template <int HD>
static void launch_chunk_hd(const AttnPastArgs& a, hipStream_t s) {
    const size_t lds = (size_t)CA_WAVES * CA_KT * (HD + 4) * sizeof(float);
    if (lds > 64 * 1024) {  // hd 64 and 128 (set at every launch: cheap, and right on every device)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&attention_chunk_kernel<HD>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess)
            throw std::runtime_error(std::string("EDEVICE: attention_chunk: dynamic LDS limit: ") + hipGetErrorString(e));
    }
    const dim3 g((a.max_q + CA_Q - 1) / CA_Q, a.heads, a.n_seq);
    DSOCR_LAUNCH(attention_chunk_kernel<HD>, g, dim3(64 * CA_WAVES), lds, s, a);
}

void launch_attention_chunk(const AttnPastArgs& a, hipStream_t s) {
    if (!attention_chunk_ok(a)) throw std::runtime_error("EINVAL: attention_chunk: shape outside the kernel's contract");
    if (a.hd == 128) launch_chunk_hd<128>(a, s);
    else if (a.hd == 64) launch_chunk_hd<64>(a, s);
    else launch_chunk_hd<32>(a, s);
}

}  // namespace dsocr
