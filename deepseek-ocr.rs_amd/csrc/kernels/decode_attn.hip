// Decode q/k/v projection + RoPE, decode attention and the launch that fuses both.
#include "decode_common.hpp"

namespace dsocr {

// ------------------------------------------------------------------ q/k/v projection + RoPE
// dec_gemv for the fused q/k/v rows with the rotation (rotate_half RoPE, block.rs:1403-1471) in
// the epilogue: a wave owns the row pair (d, d + HD/2) of one head segment, so both halves of
// the rotation meet in one lane; q and k segments are rotated at the decode position, v rows pass
// through.  The per-row arithmetic is dec_gemv's (chunk u-major, then j), the rotation is the
// attention kernel's formula x*cos + sign*partner*sin.  One token (M = 1).
// (Every wave normalising the row itself, without LDS or a block barrier, measured +0.75 us per layer:
// the block-staged row is read from LDS, not re-read from L2 by each wave.)
// SC1: the rows are handed to attention blocks of the same launch (dec_qkv_attn): stored write-through
template <typename WT, bool SC1>
__device__ __forceinline__ void qkv_rope_body(const DecGemvArgs& a, const DecRopeEpi& r, int bid) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int U = 3, XR = 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = r.hd / 2;
    const int p = bid * 4 + wave;                        // pair index
    const int npairs = a.N / 2;
    const bool active = p < npairs;
    const int pp = min(p, npairs - 1);
    const int n0 = (pp / half) * r.hd + pp % half, n1 = n0 + half;
    const WT* W = reinterpret_cast<const WT*>(a.W);
    const int chunks = a.K >> 3;
    XRegs<1, XR> xr;
    xload<1, XR>(xr, a.x, a.ldx, nullptr, 1, a.K, a.norm_w);
    const int pos = r.kv_pos[0];
    uint4 w0[U], w1[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int cc = min(u * 64 + lane, chunks - 1);
        w0[u] = ldg_nt16(W + (long)n0 * a.ldw + (cc << 3));
        w1[u] = ldg_nt16(W + (long)n1 * a.ldw + (cc << 3));
    }
    const int d = n0 % r.hd;
    const bool rot = n0 < r.rot_rows;
    const float c0 = rot ? r.cos[(long)pos * r.hd + d] : 1.f, s0 = rot ? r.sin[(long)pos * r.hd + d] : 0.f;
    const float c1 = rot ? r.cos[(long)pos * r.hd + d + half] : 1.f, s1 = rot ? r.sin[(long)pos * r.hd + d + half] : 0.f;
    xstage<1, XR>(xr, 1, a.K, a.norm_w != nullptr, a.eps, smem);
    if (!active) return;
    const float* xs = smem + XS_RED;
    float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int cc = u * 64 + lane;
        if (cc < chunks) {
            float f0[8], f1[8], xv[8];
            unpack8<WT>(w0[u], f0);
            unpack8<WT>(w1[u], f1);
            ld_x8(xs + (cc << 3), xv);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                acc0 = fmaf(xv[j], f0[j], acc0);
                acc1 = fmaf(xv[j], f1[j], acc1);
            }
        }
    }
    float y0 = wave_sum(acc0), y1 = wave_sum(acc1);
    if (lane == 0) {
        y0 = y0 + (a.bias ? a.bias[n0] : 0.f);
        y1 = y1 + (a.bias ? a.bias[n1] : 0.f);
        if (rot) {
            const float o0 = y0 * c0 + (-1.f * y1) * s0;
            const float o1 = y1 * c1 + (1.f * y0) * s1;
            y0 = o0;
            y1 = o1;
        }
        if (SC1) {
            __hip_atomic_store(a.y + n0, y0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.y + n1, y1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            a.y[n0] = y0;
            a.y[n1] = y1;
        }
    }
}

template <typename WT>
__global__ __launch_bounds__(256) void dec_qkv_rope_kernel(DecGemvArgs a, DecRopeEpi r) {
    qkv_rope_body<WT, false>(a, r, blockIdx.x);
}

bool dec_qkv_rope_ok(const DecGemvArgs& a, const DecRopeEpi& r) {
    return a.M == 1 && r.hd % 2 == 0 && a.N % r.hd == 0 && a.K % 8 == 0 && a.K <= 64 * 3 * 8 && r.kv_pos && r.cos &&
           r.sin;
}

void launch_dec_qkv_rope(const DecGemvArgs& a, const DecRopeEpi& r, hipStream_t s) {
    if (!dec_qkv_rope_ok(a, r)) throw std::runtime_error("EINVAL: dec_qkv_rope outside its range");
    const size_t lds = stage_bytes(1, a.K);
    dim3 grid((a.N / 2 + 3) / 4);
    with_wt(a.wdtype, [&](auto wt) { DSOCR_LAUNCH((dec_qkv_rope_kernel<decltype(wt)>), grid, dim3(256), lds, s, a, r); });
}

// ------------------------------------------------------------------ decode attention
// grid (chunks of 64 keys, heads, B).  The token being decoded sits at pos = kv_pos[b]: q and the new
// k are rotated here (rotate_half RoPE, block.rs:1403-1471) unless the projection's epilogue already
// did (PREROT, one page: dec_qkv_rope); the block owning chunk pos/64 appends k, v to the f32 cache
// (block.rs:776-789) and uses them directly.  Each block issues its K and V cache loads first, then
// builds q; the chunk partials of a (page, head) are merged by chunk 0's block polling them (POLL, <= 24
// chunks of 128-dim heads) or by the last arriver of a ticket (flash-decoding combine).
// phase clock (DecAttn2Args::stamps): thread 0 of each block stores s_memrealtime into the block's own
// 8-word record (no atomics: 680 blocks on one word serialised the launch)
__device__ __forceinline__ void da_stamp(unsigned long long* st, int slot) {
    if (!st || threadIdx.x != 0) return;
    const long blk = blockIdx.x + (long)gridDim.x * (blockIdx.y + (long)gridDim.y * blockIdx.z);
    st[blk * 8 + slot] = __builtin_amdgcn_s_memrealtime();
}

constexpr int DA_CH = 64;       // keys per block
constexpr int DA2_CH_MIN = DA_CH;
constexpr uint32_t DA_SENT = 0x7FBADBADu;  // "record word not written yet" (a NaN payload no arithmetic produces)

// sum over aligned groups of N lanes (N = 4 or 8), result in every lane of the group
template <int N>
__device__ __forceinline__ float group_sum(float v) {
    v += dpp_f<DPP_QUAD_XOR1>(0.f, v);
    v += dpp_f<DPP_QUAD_XOR2>(0.f, v);
    if (N == 8) v += dpp_f<DPP_ROW_HALF_MIRROR>(0.f, v);
    return v;
}

// FUSED (dec_qkv_attn, one page, PREROT + POLL): q and the new k / v come from q/k/v blocks of the
// same launch, stored write-through into a row that enters the launch sentinel-filled; this block
// issues its K / V cache loads first, then polls its rows until no word holds the sentinel, and the
// merging block (chunk 0) refills them once every chunk of the head has read them (its record is
// written after that read) - or, with DecAttn2Args::no_refill, leaves them to the next launch's projection
// blocks, which clean the copy they do not use.  The cache stream overlaps the projection's weight stream.
template <int HD, bool PREROT, bool POLL, bool FUSED>
__device__ __forceinline__ void dec_attn_body(const DecAttn2Args& a, const int c, const int h, const int b) {
    constexpr int CH = DA_CH;
    constexpr int LPK = 256 / CH;                                // lanes per key when scoring
    constexpr int DPL = HD / LPK;                                // dims per lane when scoring
    constexpr int DG = HD / 4, KG = 256 / DG, KPG = CH / KG;     // PV: float4 dim groups x key groups
    static_assert(KPG >= 1 && DPL % 4 == 0, "unsupported head_dim");
    __shared__ float qs[HD];
    __shared__ float knew[HD];
    __shared__ float vnew[HD];
    __shared__ float p_s[CH];
    __shared__ float red[8];
    __shared__ int last_s;
    __shared__ float4 o_s[384];  // P.V partials; reused by the combine (m, l per chunk + per-group sums)
    const int k0 = c * CH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kvh = h / (a.heads / a.kv_heads);
    float* Kc = a.kc + (long)b * a.page_stride + (long)kvh * a.head_stride;
    float* Vc = a.vc + (long)b * a.page_stride + (long)kvh * a.head_stride;
    // 1. the chunk's K / V cache loads (keys clamped to the position: keys past it are masked at use)
    const int key = tid / LPK, sub = tid % LPK;
    const int dg = tid % DG, kg = tid / DG;
    float4 kreg[DPL / 4];
    float4 vreg[KPG];
    // TK (128-dim heads): K is loaded like V, instruction i of wave w reading keys w*16 + 2i and
    // w*16 + 2i + 1 whole (1 KiB contiguous per instruction: 8 L2 lines, where one key per 4 lanes touched
    // 64 lines per instruction); lane l holds dims 4 (l & 31) .. + 3 of key tk_key(i) = w*16 + 2i + (l >> 5),
    // and the q.k dot products are finished by a transposing butterfly over the 32 lanes of a key
    // (9 swizzle / DPP adds for 8 keys).
    constexpr bool TK = HD == 128;
    const int tk_half = lane >> 5, tk_d4 = (lane & 31) * 4;
    auto tk_key = [&](int i) { return wave * 16 + 2 * i + tk_half; };
    auto issue_k = [&](int kb, int klim) {
        if constexpr (TK) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                kreg[i] = ldg_nt_f4(Kc + (long)min(kb + tk_key(i), klim) * HD + tk_d4);
        } else {
            const float4* kp = reinterpret_cast<const float4*>(Kc + (long)min(kb + key, klim) * HD + sub * DPL);
#pragma unroll
            for (int i = 0; i < DPL / 4; ++i) kreg[i] = kp[i];
        }
    };
    auto issue_v = [&](int kb, int klim) {
#pragma unroll
        for (int j = 0; j < KPG; ++j) {
            const int kk = min(kb + (TK ? tk_key(j) : kg * KPG + j), klim);
            vreg[j] = ldg_nt_f4(Vc + (long)kk * HD + dg * 4);
        }
    };
    const float* row = a.qkv + (long)b * a.ld;
    float q_pre = 0.f, k_pre = 0.f, v_pre = 0.f;
    if (PREROT && !FUSED) {  // unconditional (every thread loads a valid element): one round trip with pos
        const int td = tid & (HD - 1);
        q_pre = row[h * HD + td];
        k_pre = row[a.heads * HD + kvh * HD + td];
        v_pre = row[(a.heads + a.kv_heads) * HD + kvh * HD + td];
    }
    const int pos = a.kv_pos[b];
    const int len = pos + 1;
    if (k0 >= len) return;
    if (FUSED && a.kv_delay > 0) {
        // the projection blocks' weight stream first: this block's K / V cache loads wait kv_delay ticks
        // (s_memrealtime, 10 ns) so the two streams do not share HBM while q is still being computed
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (__builtin_amdgcn_s_memrealtime() - t0 < (unsigned long long)a.kv_delay) __builtin_amdgcn_s_sleep(2);
    }
    issue_k(k0, min(k0 + CH, len) - 1);
    issue_v(k0, min(k0 + CH, len) - 1);
    const bool own = pos >= k0 && pos < k0 + CH;
    bool gave_up = false;
    if constexpr (FUSED) {
        // the head's q (and, owning the position, the new k / v) from this launch's projection blocks
        const int td = tid & (HD - 1);
        const auto rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(row), (short)0,
                                                          (a.heads + 2 * a.kv_heads) * HD * 4, 0x00020000);
        const int oq = (h * HD + td) * 4, ok = ((a.heads + kvh) * HD + td) * 4,
                  ov = ((a.heads + a.kv_heads + kvh) * HD + td) * 4;
        for (unsigned it = 0;; ++it) {
            asm volatile("" ::: "memory");
            bool pend = false;
            if (tid < HD) {  // waves 0..HD/64-1 poll (the others only join the vote): half the polling traffic
                q_pre = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rr, oq, 0, 16));
                k_pre = own ? __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rr, ok, 0, 16)) : 0.f;
                v_pre = own ? __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rr, ov, 0, 16)) : 0.f;
                pend = __float_as_uint(q_pre) == DA_SENT || __float_as_uint(k_pre) == DA_SENT ||
                       __float_as_uint(v_pre) == DA_SENT;
            }
            if (!__syncthreads_or(pend)) break;
            if (it > (1u << 20)) {
                if (tid == 0) __hip_atomic_store(a.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                gave_up = true;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        da_stamp(a.stamps, 2);
    }
    // a block that gave up (the error flag is set; the host raises after the step) leaves the K / V cache
    // untouched: sentinel q / k / v never enter the cache.  It still writes its record so the merge of its
    // head does not wait out a second bounded spin.
    const bool write_kv = own && !gave_up;
    const int nc = (len + CH - 1) / CH;
    // 2. RoPE inputs
    const float* krow = row + a.heads * HD + kvh * HD;
    const float* vrow = row + (a.heads + a.kv_heads) * HD + kvh * HD;
    float qx = 0.f, qr = 0.f, kx = 0.f, kr = 0.f, vx = 0.f, cs = 1.f, sn = 0.f, sg = 0.f;
    if (PREROT) {
        if (tid < HD) {
            qs[tid] = q_pre;
            if (own) {
                knew[tid] = k_pre;
                vnew[tid] = v_pre;
                if (write_kv && h == kvh * (a.heads / a.kv_heads)) {  // one writer per kv head
                    Kc[(long)pos * HD + tid] = k_pre;
                    Vc[(long)pos * HD + tid] = v_pre;
                }
            }
        }
    } else if (tid < HD) {
        int ix = tid, ir = tid;
        if (tid < a.rope_dim) {
            const int half = a.rope_dim / 2;
            auto map = [&](int i) { return !a.use_mla ? i : (i < half ? 2 * i : 2 * (i - half) + 1); };
            ix = map(tid);
            ir = tid < half ? map(tid + half) : map(tid - half);
            sg = tid < half ? -1.f : 1.f;
            cs = a.cos[(long)pos * a.rope_dim + tid];
            sn = a.sin[(long)pos * a.rope_dim + tid];
        }
        qx = row[h * HD + ix];
        qr = row[h * HD + ir];
        if (own) {
            kx = krow[ix];
            kr = krow[ir];
            vx = vrow[tid];
        }
    }
    // 3. rotated q (and the new k, v in the owning chunk): x*cos + sign*partner*sin
    if (!PREROT && tid < HD) {
        qs[tid] = qx * cs + (sg * qr) * sn;
        if (own) {
            const float kv = kx * cs + (sg * kr) * sn;
            knew[tid] = kv;
            vnew[tid] = vx;
            if (h == kvh * (a.heads / a.kv_heads)) {  // one writer per kv head
                Kc[(long)pos * HD + tid] = kv;
                Vc[(long)pos * HD + tid] = vx;
            }
        }
    }
    __syncthreads();
    const int kn = min(CH, len - k0);
    // 4. scores: LPK lanes per key, wave w owns keys w*CH/4 .. (w+1)*CH/4 - 1
    if constexpr (TK) {
        const float4 q4 = *reinterpret_cast<const float4*>(qs + tk_d4);
        const float4 kn4 = *reinterpret_cast<const float4*>(knew + tk_d4);
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float4 k4 = k0 + tk_key(i) == pos ? kn4 : kreg[i];
            v[i] = fmaf(q4.w, k4.w, fmaf(q4.z, k4.z, fmaf(q4.y, k4.y, q4.x * k4.x)));
        }
        // butterfly: after the xor-16 / 8 / 4 steps lane l holds key i = b2 + 2 b3 + 4 b4 (bits of l)
        // summed over its 8 lanes of that bit pattern; the quad sum finishes the 32 lanes
        const int b4 = (lane >> 4) & 1, b3 = (lane >> 3) & 1, b2 = (lane >> 2) & 1;
        float u[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float keep = b4 ? v[j + 4] : v[j], send = b4 ? v[j] : v[j + 4];
            u[j] = keep + __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(send), 0x1f | (16 << 10)));
        }
        float t[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float keep = b3 ? u[j + 2] : u[j], send = b3 ? u[j] : u[j + 2];
            t[j] = keep + __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(send), 0x1f | (8 << 10)));
        }
        float r;
        {
            const float keep = b2 ? t[1] : t[0], send = b2 ? t[0] : t[1];
            r = keep + __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(send), 0x1f | (4 << 10)));
        }
        r = group_sum<4>(r);
        const int kk = tk_key(b2 + 2 * b3 + 4 * b4);
        const float sc = kk < kn ? r * a.scale : -INFINITY;
        if ((lane & 3) == 0) p_s[kk] = sc;
        const float mw = wave_max(sc);
        if (lane == 0) red[wave] = mw;
    } else {
        float acc = 0.f;
        if (key < kn) {
            if (k0 + key == pos) {
#pragma unroll
                for (int i = 0; i < DPL; ++i) acc = fmaf(qs[sub * DPL + i], knew[sub * DPL + i], acc);
            } else {
#pragma unroll
                for (int i = 0; i < DPL / 4; ++i) {
                    acc = fmaf(qs[sub * DPL + 4 * i + 0], kreg[i].x, acc);
                    acc = fmaf(qs[sub * DPL + 4 * i + 1], kreg[i].y, acc);
                    acc = fmaf(qs[sub * DPL + 4 * i + 2], kreg[i].z, acc);
                    acc = fmaf(qs[sub * DPL + 4 * i + 3], kreg[i].w, acc);
                }
            }
        }
        acc = group_sum<LPK>(acc);
        const float sc = key < kn ? acc * a.scale : -INFINITY;
        if (sub == 0) p_s[key] = sc;
        const float mw = wave_max(sc);
        if (lane == 0) red[wave] = mw;
    }
    __syncthreads();
    const float m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (wave == 0) {  // whole wave active for the DPP reduction
        const float p = (tid < CH && tid < kn) ? expf(p_s[tid] - m) : 0.f;
        if (tid < CH) p_s[tid] = p;
        const float l = wave_sum(p);
        if (tid == 0) red[4] = l;
    }
    __syncthreads();
    if (!FUSED) da_stamp(a.stamps, 2);  // standalone: the chunk's scores and softmax done (K landed)
    // 5. P.V over this thread's KPG keys
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < KPG; ++j) {
        const int key2 = TK ? tk_key(j) : kg * KPG + j;
        if (key2 >= kn) vreg[j] = make_float4(0.f, 0.f, 0.f, 0.f);  // never 0 * (stale cache bits)
        else if (k0 + key2 == pos) vreg[j] = *reinterpret_cast<const float4*>(vnew + dg * 4);
    }
#pragma unroll
    for (int j = 0; j < KPG; ++j) {
        const float p = p_s[TK ? tk_key(j) : kg * KPG + j];
        o.x = fmaf(p, vreg[j].x, o.x);
        o.y = fmaf(p, vreg[j].y, o.y);
        o.z = fmaf(p, vreg[j].z, o.z);
        o.w = fmaf(p, vreg[j].w, o.w);
    }
    const float l_run = red[4];
    o_s[tid] = o;
    __syncthreads();
    // partial record of chunk c: [m, l, -, -, o[HD]] (16-byte aligned), stored WRITE-THROUGH (sc1)
    // so the hand-off needs no L2-writeback release fence (cdna_hip_programming.md Guideline 16 R1)
    constexpr int PR = HD + 4;
    const int chunks = (a.max_len + CH - 1) / CH;
    float* part0 = a.part + ((long)b * a.heads + h) * chunks * PR;
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(part0, (short)0, chunks * PR * 4, 0x00020000);
    if (tid < DG) {
        float4 t = o_s[tid];
        for (int g = 1; g < KG; ++g) {
            const float4 u = o_s[g * DG + tid];
            t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
        }
        u32x4 bits;
        __builtin_memcpy(&bits, &t, 16);
        __builtin_amdgcn_raw_buffer_store_b128(bits, rsrc, (c * PR + 4 + tid * 4) * 4, 0, 16);
    }
    if (tid == 0) {
        // (the two padding words are never read: they carry the sentinel, so a refilled record is all sentinel)
        const uint32_t ml[4] = {__float_as_uint(m), __float_as_uint(l_run), DA_SENT, DA_SENT};
        u32x4 bits;
        __builtin_memcpy(&bits, ml, 16);
        __builtin_amdgcn_raw_buffer_store_b128(bits, rsrc, c * PR * 4, 0, 16);
    }
    da_stamp(a.stamps, 3);
    // 6. POLL: no ticket.  Chunk 0's block merges: it polls the records of the other chunks until
    //    none of the words it needs still holds the sentinel (the record buffer enters every launch
    //    filled with it: dec_attn_part_init, then each merge refills what it read), so a writer
    //    neither waits for its stores' acknowledgement nor takes an atomic round trip.  A word is
    //    written once per launch and read with sc1 loads; a value is never the sentinel's NaN
    //    payload (arithmetic produces the canonical NaN).  Bounded spin: a give-up sets *err.
    //    Otherwise: arrival ticket (every storing wave drains, then one relaxed agent add); the last
    //    chunk block of (b, h) merges every partial.  Every partial byte was stored sc1 and
    //    every load of it below is an sc1 buffer load, so no acquire fence is needed
    //    (MI355X_MICROARCH.md, hand-offs with sc1 loads in place of the acquire, first row).
    if constexpr (POLL) {
        if (c != 0) return;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (POLL) {
        last_s = 1;
    } else if (tid == 0) {
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
    // chunk maxima / sums into LDS, then each of the 256/HD thread groups folds a strided
    // subset of the chunks for its dim (unconditional loads: a predicated load becomes an
    // exec-masked branch with a vmcnt(0) drain)
    float* ms = reinterpret_cast<float*>(o_s);
    float* ls = ms + 512;
    float* accp = ms + 1024;
    float* lp = ms + 1280;
    constexpr int KS = 256 / HD;
    const int dim = tid % HD, grp = tid / HD;
    float l = 0.f, acc = 0.f;
    bool refill = false;
    constexpr int NJ = 12;  // o partials per thread held in registers (nc <= KS * NJ)
    if (nc <= KS * NJ && nc <= 64) {
        // ONE round trip: (m, l) of chunk `lane` (every wave holds all of them) and this thread's o partials
        // (clamped indices, weight 0 past nc by a select) are all in flight together
        float ov[NJ];
        const int tc = min(lane, nc - 1);
        float mt, lt0;
        for (unsigned it = 0;; ++it) {
            asm volatile("" ::: "memory");  // the records change under us: re-load them every pass
#pragma unroll
            for (int j = 0; j < NJ; ++j) ov[j] = ld1(min(grp + KS * j, nc - 1) * PR + 4 + dim);
            mt = ld1(tc * PR);
            lt0 = ld1(tc * PR + 1);
            if (!POLL) break;
            bool pend = __float_as_uint(mt) == DA_SENT || __float_as_uint(lt0) == DA_SENT;
#pragma unroll
            for (int j = 0; j < NJ; ++j) pend = pend || __float_as_uint(ov[j]) == DA_SENT;
            if (!__syncthreads_or(pend)) break;
            if (it > (1u << 20)) {
                if (tid == 0) __hip_atomic_store(a.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        da_stamp(a.stamps, 4);
        refill = POLL;  // the words this thread read are refilled at the very end (after the last barrier)
        // chunk maxima / sums straight from the lanes that hold them: a wave max and lane reads, no LDS round
        // trips or barrier (kbench attn stamps: the LDS form took ~2.5 us from the last poll to the exit)
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
    // deferred refill (two hand-off copies alternating by layer): the words read here stay as they are, the
    // next launch's projection blocks clean this copy (dec_qkv_attn_kernel) - the merging block, the last of
    // the launch to finish, leaves with the context row stored
    if (FUSED && a.no_refill) {
        da_stamp(a.stamps, 5);
        return;
    }
    if constexpr (FUSED) {
        // every chunk of this head has read its q / k / v (its record, merged above, came after): refill
        if (tid < HD) {
            const uint32_t sent = DA_SENT;
            const auto rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(row), (short)0,
                                                              (a.heads + 2 * a.kv_heads) * HD * 4, 0x00020000);
            __builtin_amdgcn_raw_buffer_store_b32(sent, rr, (h * HD + tid) * 4, 0, 16);
            __builtin_amdgcn_raw_buffer_store_b32(sent, rr, ((a.heads + kvh) * HD + tid) * 4, 0, 16);
            __builtin_amdgcn_raw_buffer_store_b32(sent, rr, ((a.heads + a.kv_heads + kvh) * HD + tid) * 4, 0, 16);
        }
    }
    if (POLL && refill) {
        // refill the record words this thread read (each word by exactly one thread) for the next launch.
        // Here, after the block's last barrier: a __syncthreads waits for the write-through acknowledgements
        // of every store before it (kbench attn stamps: merge poll -> exit 2.5-3 us with the refill before
        // the combine's barriers)
        const uint32_t sent = DA_SENT;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (grp + KS * j < nc) __builtin_amdgcn_raw_buffer_store_b32(sent, rsrc, ((grp + KS * j) * PR + 4 + dim) * 4, 0, 16);
        if (tid < nc) {
            __builtin_amdgcn_raw_buffer_store_b32(sent, rsrc, (tid * PR) * 4, 0, 16);
            __builtin_amdgcn_raw_buffer_store_b32(sent, rsrc, (tid * PR + 1) * 4, 0, 16);
        }
    }
    da_stamp(a.stamps, 5);
}

template <int HD, bool PREROT, bool POLL>
__global__ __launch_bounds__(256) void dec_attn_kernel(DecAttn2Args a) {
    WaveSpan span_(a.span);
    da_stamp(a.stamps, 0);
    dec_attn_body<HD, PREROT, POLL, false>(a, blockIdx.x, blockIdx.y, blockIdx.z);
}

// One page (MHA, 128-dim heads, <= 24 chunks): the q/k/v projection (qkv_rope_body, blocks [0, nq)) and
// the decode attention (blocks nq + h * chunks + c) in ONE launch: the attention blocks stream their K / V
// cache chunk while the projection blocks stream the q/k/v weights, then take q / k / v by polling
// (FUSED above) - the kernel boundary between the two and the attention's load latency leave the chain.
template <typename WT>
__global__ __launch_bounds__(256) void dec_qkv_attn_kernel(DecGemvArgs g, DecRopeEpi r, DecAttn2Args a, int nq) {
    WaveSpan span_(a.span);
    da_stamp(a.stamps, 0);
    if ((int)blockIdx.x < nq) {
        qkv_rope_body<WT, true>(g, r, blockIdx.x);
        da_stamp(a.stamps, 1);
        // deferred refill: these blocks are done well before the merging blocks; they write the sentinel over
        // the OTHER hand-off copy (last read by the previous launch, next read by the following one), one word
        // per thread, in the store form of the in-launch refill
        if (a.clean_qkv || a.clean_part) {
            const uint32_t sent = DA_SENT;
            const int t = (int)blockIdx.x * 256 + (int)threadIdx.x, nt = nq * 256;
            if (a.clean_qkv) {
                const int words = (a.heads + 2 * a.kv_heads) * 128;
                const auto rq = __builtin_amdgcn_make_buffer_rsrc(a.clean_qkv, (short)0, words * 4, 0x00020000);
                for (int i = t; i < words; i += nt) __builtin_amdgcn_raw_buffer_store_b32(sent, rq, i * 4, 0, 16);
            }
            if (a.clean_part) {
                const int words = a.heads * ((a.max_len + DA_CH - 1) / DA_CH) * (128 + 4);
                const auto rp = __builtin_amdgcn_make_buffer_rsrc(a.clean_part, (short)0, words * 4, 0x00020000);
                for (int i = t; i < words; i += nt) __builtin_amdgcn_raw_buffer_store_b32(sent, rp, i * 4, 0, 16);
            }
        }
        return;
    }
    const int chunks = (a.max_len + DA_CH - 1) / DA_CH;
    const int i = (int)blockIdx.x - nq;
    dec_attn_body<128, true, true, true>(a, i % chunks, i / chunks, 0);
}

// ------------------------------------------------------------------ residency of the polled hand-offs
// A polling block waits on blocks of its own grid.  HIP promises no dispatch order (MI355X_MICROARCH.md,
// "Contract"), so such a launch is deadlock-free only if the blocks that can wait never hold every slot the
// device has for the kernel: then a block that never waits always finds a slot, runs to completion, and
// every producer eventually runs.  Rule: waiting < usable slots, with usable slots per CU =
// min(API answer, 8) less one where the API may over-admit (the guide's residency note: at 82-98 SGPRs
// the API reports one block per CU more than the hardware admits).  Blocks that can wait:
//   dec_qkv_attn: every attention block (each polls its head's q / k / v row) = chunks * heads;
//   dec_attn (POLL): the merging block of each (page, head) = B * heads.
bool poll_wait_fits(long waiting_blocks, int api_blocks_per_cu, int cus) {
    if (waiting_blocks <= 0) return true;
    int per_cu = std::min(api_blocks_per_cu, 8);
    if (per_cu >= 6) per_cu -= 1;
    return per_cu > 0 && cus > 0 && waiting_blocks < (long)per_cu * cus;
}

namespace {
int qkv_attn_blocks_per_cu(int wdtype, size_t lds) {
    return with_wt(wdtype, [&](auto wt) {
        static int v = -1;  // per weight type; the dynamic LDS is stage_bytes(1, K): one model per process
        if (v < 0) v = blocks_per_cu(dec_qkv_attn_kernel<decltype(wt)>, lds);
        return v;
    });
}
int attn_poll_blocks_per_cu(bool prerot) {
    static int pr = -1, npr = -1;
    int& v = prerot ? pr : npr;
    if (v < 0) v = prerot ? blocks_per_cu(dec_attn_kernel<128, true, true>, 0) : blocks_per_cu(dec_attn_kernel<128, false, true>, 0);
    return v;
}
}  // namespace

bool dec_qkv_attn_ok(const DecGemvArgs& g, const DecRopeEpi& r, const DecAttn2Args& a) {
    const int chunks = (a.max_len + DA_CH - 1) / DA_CH;
    if (!(dec_qkv_rope_ok(g, r) && a.B == 1 && a.hd == 128 && r.hd == 128 && a.heads == a.kv_heads && a.err &&
          chunks <= 24 && a.max_len <= 512 * DA_CH && g.y == a.qkv && g.N == (a.heads + 2 * a.kv_heads) * a.hd &&
          r.rot_rows == (a.heads + a.kv_heads) * a.hd))
        return false;
    // the copy a launch cleans is never the one its own blocks poll
    if ((a.clean_qkv && a.clean_qkv == a.qkv) || (a.clean_part && a.clean_part == a.part)) return false;
    return poll_wait_fits((long)chunks * a.heads, qkv_attn_blocks_per_cu(g.wdtype, stage_bytes(1, g.K)), device_cus());
}

bool dec_attn_polled(const DecAttn2Args& a) {
    const int chunks = (a.max_len + DA_CH - 1) / DA_CH;
    return a.err && a.hd == 128 && chunks <= 24 &&
           poll_wait_fits((long)a.B * a.heads, attn_poll_blocks_per_cu(a.prerot != 0), device_cus());
}

void launch_dec_qkv_attn(const DecGemvArgs& g, const DecRopeEpi& r, const DecAttn2Args& a, hipStream_t s) {
    if (!dec_qkv_attn_ok(g, r, a)) throw std::runtime_error("EINVAL: dec_qkv_attn outside its range");
    const int nq = (g.N / 2 + 3) / 4;
    const int chunks = (a.max_len + DA_CH - 1) / DA_CH;
    const size_t lds = stage_bytes(1, g.K);
    dim3 grid(nq + chunks * a.heads);
    with_wt(g.wdtype, [&](auto wt) { DSOCR_LAUNCH((dec_qkv_attn_kernel<decltype(wt)>), grid, dim3(256), lds, s, g, r, a, nq); });
}

void dec_qkv_sentinel_init(float* qkv, size_t floats, hipStream_t s) {
    if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(qkv), (int)DA_SENT, floats, s) != hipSuccess)
        throw std::runtime_error("EINTERNAL: hipMemsetD32Async (q/k/v hand-off row)");
}

void dec_attn_part_init(float* part, size_t bytes, hipStream_t s) {
    if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(part), (int)DA_SENT, bytes / 4, s) != hipSuccess)
        throw std::runtime_error("EINTERNAL: hipMemsetD32Async (attention records)");
}

size_t dec_attn_workspace(int B, int heads, int hd, int max_len) {
    return (size_t)B * heads * ((max_len + DA2_CH_MIN - 1) / DA2_CH_MIN) * (hd + 4) * sizeof(float);
}

void launch_dec_attn(const DecAttn2Args& a, hipStream_t s) {
    if (!a.counters) throw std::runtime_error("EINTERNAL: dec_attn needs a zeroed counter array");
    if (a.max_len > 512 * DA_CH) throw std::runtime_error("EINVAL: decode context too long for the attention combine");
    if (a.hd != 128 && a.hd != 64 && a.hd != 32) throw std::runtime_error("EINVAL: decode attention supports head_dim 32 / 64 / 128");
    const int chunks = (a.max_len + DA_CH - 1) / DA_CH;
    const bool prerot = a.prerot != 0;
    dim3 g1(chunks, a.heads, a.B);
    // polling merge (no ticket): 128-dim heads, <= 24 chunks (one load round trip in the merge), a
    // give-up flag, a sentinel-filled record buffer, the merging blocks within the residency rule;
    // otherwise the arrival ticket (no block waits)
    if (dec_attn_polled(a)) {
        if (prerot) DSOCR_LAUNCH((dec_attn_kernel<128, true, true>), g1, dim3(256), 0, s, a);
        else DSOCR_LAUNCH((dec_attn_kernel<128, false, true>), g1, dim3(256), 0, s, a);
        return;
    }
    with_rows<128, 64, 32>(a.hd, [&](auto hd) {
        constexpr int HD = decltype(hd)::value;
        if (prerot) DSOCR_LAUNCH((dec_attn_kernel<HD, true, false>), g1, dim3(256), 0, s, a);
        else DSOCR_LAUNCH((dec_attn_kernel<HD, false, false>), g1, dim3(256), 0, s, a);
    });
}

}  // namespace dsocr
