// Decode attention over an f16 K/V cache (DSOCR_LOAD_KV_F16).
//
// Contract: the cache keeps f16(K_rot) and f16(V) in the f32 cache's layout and element strides
// ([page][kv_head][max_len][hd] row-major), rounded once at append: round to nearest even, clamped to
// +-65504 so a large value never becomes inf in the cache.  Everything else is f32: q, scores, softmax, the P.V
// accumulation, the partial records and the merge; a cached half widens exactly.  The step's own new key and value
// enter this step's attention unrounded (from LDS, as in dec_attn_body) and are stored rounded for later steps.
// Not served here (the engine refuses them under the flag): decode sessions, prefix entries and chunked admission
// (attention_past / attention_chunk, the slot-move and prefix-copy kernels read an f32 cache), the persistent
// layer launch (DSOCR_PERSIST) and the fused one-page q/k/v + attention launch; an FP8 cache is not part of this.
//
// grid (chunks of 128 keys, heads, B), 256 threads.  Wave w owns keys 32 w .. 32 w + 31 of the chunk; a key is
// HD / 8 lanes (LPK: 16 at hd 128), lane l holding dims 8 (l % LPK) .. + 7 of key 32 w + i KPI + l / LPK in
// instruction i (KPI = 64 / LPK keys per instruction, NI = 32 / KPI instructions: 8 / 4 / 2 at hd 128 / 64 / 32).
// Every K and every V instruction is one contiguous 1 KiB of the cache; the lane's dims are the same in all of
// them, so its eight q values live in registers.  All K and V loads (16-byte nontemporal) are issued before
// anything that depends on the position but the clamp.  No MFMA: every shipped config is MHA, so there is one
// query row per K/V head - 1 of 16 matrix columns; the kernel is a byte stream.
#include "decode_common.hpp"

namespace dsocr {

namespace {
constexpr int KV16_CH = 128;  // keys per block

// RTNE to f16 with the clamp (NaN passes through the compares)
__device__ __forceinline__ uint32_t f16_rne_clamp(float x) {
    x = x > 65504.f ? 65504.f : (x < -65504.f ? -65504.f : x);
    const _Float16 h = (_Float16)x;
    uint16_t b;
    __builtin_memcpy(&b, &h, 2);
    return b;
}

}  // namespace

template <int HD, bool PREROT>
__global__ __launch_bounds__(256) void dec_attn_kv16_kernel(DecAttnKv16Args a) {
    constexpr int CH = KV16_CH;
    constexpr int LPK = HD / 8, KPI = 64 / LPK, NI = 32 / KPI;
    constexpr int PR = HD + 4;
    static_assert(HD == 128 || HD == 64 || HD == 32, "unsupported head_dim");
    __shared__ __attribute__((aligned(16))) float qs[HD];
    __shared__ __attribute__((aligned(16))) float knew[HD];
    __shared__ __attribute__((aligned(16))) float vnew[HD];
    __shared__ float p_s[CH];
    __shared__ float red[8];
    __shared__ int last_s;
    __shared__ __attribute__((aligned(16))) float o_s[2048];  // P.V partials [256 / LPK][HD]; reused by the merge
    WaveSpan span_(a.span);
    const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int k0 = c * CH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int gq = a.heads / a.kv_heads, kvh = h / gq;
    const long cbase = (long)b * a.page_stride + (long)kvh * a.head_stride;
    uint16_t* Kc = a.kc16 + cbase;
    uint16_t* Vc = a.vc16 + cbase;
    const int sub = lane % LPK, kslot = lane / LPK;
    auto key_of = [&](int i) { return wave * 32 + i * KPI + kslot; };
    // the raw q / k / v elements of this thread's dim (and of its rotation partner): no position needed, so one
    // round trip together with it
    const float* row = a.qkv + (long)b * a.ld;
    const float* qrow = row + h * HD;
    const float* krow = row + a.heads * HD + kvh * HD;
    const float* vrow = row + (a.heads + a.kv_heads) * HD + kvh * HD;
    const int td = tid & (HD - 1);
    int ix = td, ir = td;
    float sg = 0.f;
    const bool rot = !PREROT && td < a.rope_dim;
    if (rot) {
        const int half = a.rope_dim / 2;
        auto map = [&](int i) { return !a.use_mla ? i : (i < half ? 2 * i : 2 * (i - half) + 1); };
        ix = map(td);
        ir = td < half ? map(td + half) : map(td - half);
        sg = td < half ? -1.f : 1.f;
    }
    const float qx = qrow[ix], kx = krow[ix], vx = vrow[td];
    const float qr = PREROT ? 0.f : qrow[ir], kr = PREROT ? 0.f : krow[ir];
    const int pos = a.kv_pos[b];
    const int len = pos + 1;
    if (k0 >= len) return;
    // 1. the chunk's K / V loads (keys clamped to the position: keys past it are masked at use)
    const int klim = min(k0 + CH, len) - 1;
    uint4 kreg[NI], vreg[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) kreg[i] = ldg_nt16(Kc + (long)min(k0 + key_of(i), klim) * HD + sub * 8);
#pragma unroll
    for (int i = 0; i < NI; ++i) vreg[i] = ldg_nt16(Vc + (long)min(k0 + key_of(i), klim) * HD + sub * 8);
    const bool own = pos >= k0 && pos < k0 + CH;
    const int nc = (len + CH - 1) / CH;
    // 2. rotated q (and the new k, v in the owning chunk): x*cos + sign*partner*sin
    if (tid < HD) {
        float cs = 1.f, sn = 0.f;
        if (rot) {
            cs = a.cos[(long)pos * a.rope_dim + td];
            sn = a.sin[(long)pos * a.rope_dim + td];
        }
        qs[tid] = PREROT ? qx : qx * cs + (sg * qr) * sn;
        if (own) {
            knew[tid] = PREROT ? kx : kx * cs + (sg * kr) * sn;
            vnew[tid] = vx;
        }
    }
    __syncthreads();
    // append: one writer per kv head, one dword per two dims, rounded (the attention below uses the f32 rows)
    if (own && h == kvh * gq && tid < HD) {
        const float* src = tid < HD / 2 ? knew : vnew;
        uint16_t* dst = (tid < HD / 2 ? Kc : Vc) + (long)pos * HD;
        const int d2 = tid % (HD / 2);
        const uint32_t w = f16_rne_clamp(src[2 * d2]) | (f16_rne_clamp(src[2 * d2 + 1]) << 16);
        reinterpret_cast<uint32_t*>(dst)[d2] = w;
    }
    const int kn = min(CH, len - k0);
    // 3. scores: eight fmaf per key and lane, then the transposing butterfly inside the key's LPK lanes (one
    //    DPP row at hd 128): after it lane l holds key i = (l % LPK) >> 1 summed over all of the key's lanes
    float q8[8], kn8[8];
    ld_x8(qs + sub * 8, q8);
    ld_x8(knew + sub * 8, kn8);
    float v[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        float kf[8];
        unpack8<f16_t>(kreg[i], kf);
        const bool mine = k0 + key_of(i) == pos;
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = fmaf(q8[j], mine ? kn8[j] : kf[j], acc);
        v[i] = acc;
    }
    if constexpr (NI >= 8) bfly<DPP_ROW_ROR8, 8, 8>(v, lane);
    if constexpr (NI >= 4) bfly<DPP_ROW_HALF_MIRROR, 4, 4>(v, lane);
    bfly<DPP_QUAD_XOR2, 2, 2>(v, lane);
    const float r = v[0] + dpp_f<DPP_QUAD_XOR1>(0.f, v[0]);
    {
        const int kk = key_of(sub >> 1);
        const float sc = kk < kn ? r * a.scale : -INFINITY;
        if ((sub & 1) == 0) p_s[kk] = sc;
        const float mw = wave_max(sc);
        if (lane == 0) red[wave] = mw;
    }
    __syncthreads();
    const float m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (wave < 2) {  // whole waves active for the DPP reduction
        const float p = tid < kn ? expf(p_s[tid] - m) : 0.f;
        p_s[tid] = p;
        const float l = wave_sum(p);
        if (lane == 0) red[4 + wave] = l;
    }
    __syncthreads();
    // 4. P.V over this lane's NI keys (same lane <-> (key, dims) map as K)
    float vn8[8];
    ld_x8(vnew + sub * 8, vn8);
    float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int key = key_of(i);
        float vf[8];
        unpack8<f16_t>(vreg[i], vf);
        const bool mine = k0 + key == pos, past = key >= kn;
        const float p = p_s[key];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float x = past ? 0.f : (mine ? vn8[j] : vf[j]);  // never 0 * (stale cache bits)
            o[j] = fmaf(p, x, o[j]);
        }
    }
    const float l_run = red[4] + red[5];
    *reinterpret_cast<float4*>(o_s + tid * 8) = make_float4(o[0], o[1], o[2], o[3]);
    *reinterpret_cast<float4*>(o_s + tid * 8 + 4) = make_float4(o[4], o[5], o[6], o[7]);
    __syncthreads();
    // partial record of chunk c: [m, l, -, -, o[HD]], stored WRITE-THROUGH (sc1) so the hand-off needs no
    // L2-writeback release fence (as dec_attn_body's ticket path)
    const int chunks = (a.max_len + CH - 1) / CH;
    float* part0 = a.part + ((long)b * a.heads + h) * chunks * PR;
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(part0, (short)0, chunks * PR * 4, 0x00020000);
    if (tid < HD) {
        float t = o_s[tid];
#pragma unroll 8
        for (int g = 1; g < 2048 / HD; ++g) t += o_s[g * HD + tid];
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(t), rsrc, (c * PR + 4 + tid) * 4, 0, 16);
    }
    if (tid == 0) {
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(m), rsrc, c * PR * 4, 0, 16);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(l_run), rsrc, (c * PR + 1) * 4, 0, 16);
    }
    // 5. arrival ticket (every storing wave drains, then one relaxed agent add); the last chunk block of (b, h)
    //    merges every partial.  Every partial byte was stored sc1 and every load of it below is an sc1 buffer
    //    load, so no acquire fence is needed.  No sentinel, no polling: no block waits on another.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        int* cnt = a.counters + (long)b * a.heads + h;
        const int old = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = old == nc - 1;
        if (last) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_s = last;
    }
    __syncthreads();
    if (!last_s) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no instruction: keeps the loads below the ticket
    auto ld1 = [&](int idx) { return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, idx * 4, 0, 16)); };
    float* ms = o_s;  // (every read of the P.V partials is behind the barriers above)
    float* ls = ms + 512;
    float* accp = ms + 1024;
    float* lp = ms + 1280;
    constexpr int KS = 256 / HD, NJ = 64 / KS;
    const int dim = tid % HD, grp = tid / HD;
    float l = 0.f, acc = 0.f;
    if (nc <= 64) {
        // ONE round trip: (m, l) of chunk `lane` (every wave holds all of them) and this thread's o partials
        // (clamped indices, weight 0 past nc by a select) are all in flight together
        float ov[NJ];
        const int tc = min(lane, nc - 1);
#pragma unroll
        for (int j = 0; j < NJ; ++j) ov[j] = ld1(min(grp + KS * j, nc - 1) * PR + 4 + dim);
        const float mt = ld1(tc * PR), lt0 = ld1(tc * PR + 1);
        const float mm = wave_max(lane < nc ? mt : -INFINITY);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int cc = grp + KS * j;
            const float mc = __shfl(mt, min(cc, 63)), lc = __shfl(lt0, min(cc, 63));
            if (cc < nc) {
                const float w = expf(mc - mm);
                l += lc * w;
                acc += ov[j] * w;
            }
        }
    } else {
        for (int cc = tid; cc < nc; cc += 256) {
            ms[cc] = ld1(cc * PR);
            ls[cc] = ld1(cc * PR + 1);
        }
        __syncthreads();
        float mm = -INFINITY;
        for (int cc = 0; cc < nc; ++cc) mm = fmaxf(mm, ms[cc]);
#pragma unroll 4
        for (int cc = grp; cc < nc; cc += KS) {
            const float w = expf(ms[cc] - mm);
            l += ls[cc] * w;
            acc += ld1(cc * PR + 4 + dim) * w;
        }
    }
    accp[grp * HD + dim] = acc;
    lp[grp * HD + dim] = l;
    __syncthreads();
    if (tid < HD) {
        float at = 0.f, lt = 0.f;
#pragma unroll
        for (int g = 0; g < KS; ++g) { at += accp[g * HD + tid]; lt += lp[g * HD + tid]; }
        a.o[(long)b * a.o_ld + (long)h * HD + tid] = at / lt;
    }
}

void launch_dec_attn_kv16(const DecAttnKv16Args& a, hipStream_t s) {
    if (!a.counters) throw std::runtime_error("EINTERNAL: dec_attn_kv16 needs a zeroed counter array");
    if (!a.kc16 || !a.vc16) throw std::runtime_error("EINTERNAL: dec_attn_kv16 needs the f16 cache pointers");
    if (a.max_len > 512 * KV16_CH) throw std::runtime_error("EINVAL: decode context too long for the attention combine");
    if (a.hd != 128 && a.hd != 64 && a.hd != 32) throw std::runtime_error("EINVAL: decode attention supports head_dim 32 / 64 / 128");
    if (a.kv_heads <= 0 || a.heads % a.kv_heads) throw std::runtime_error("EINVAL: heads must be a positive multiple of kv_heads");
    if (a.prerot && a.rope_dim != a.hd) throw std::runtime_error("EINVAL: pre-rotated rows need rope_dim == head_dim");
    dim3 g1((a.max_len + KV16_CH - 1) / KV16_CH, a.heads, a.B);
    const bool prerot = a.prerot != 0;
    with_rows<128, 64, 32>(a.hd, [&](auto hd) {
        constexpr int HD = decltype(hd)::value;
        if (prerot) DSOCR_LAUNCH((dec_attn_kv16_kernel<HD, true>), g1, dim3(256), 0, s, a);
        else DSOCR_LAUNCH((dec_attn_kv16_kernel<HD, false>), g1, dim3(256), 0, s, a);
    });
}

}  // namespace dsocr
