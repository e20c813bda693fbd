// What the matrix-core MoE units that stream reduced-byte codes share (decode_f8mm.hip, decode_f4mm.hip): the
// power-of-two epilogue scales, the end of the down launches (direct add, or the group-partials + ticket meeting) and
// the host-side sizing of their launches.
#pragma once
#include <algorithm>

#include "decode_common.hpp"
#include "mm_planes.hpp"

namespace dsocr {

// 2^e as an f32 (|e| <= 126)
__device__ __forceinline__ float pow2i(int e) { return __uint_as_float((uint32_t)(127 + e) << 23); }
// exponent i of four int8 packed in a dword
__device__ __forceinline__ float pow2b(uint32_t e4, int i) { return pow2i((int)(int8_t)(e4 >> (8 * i))); }

constexpr int MMC_DN_RT = 64;  // output rows per block of a down launch: 16 per wave

// The end of a down launch of 256 threads (every thread calls it): tot = the lane's C tile of this block's segments
// (token column lane & 15, rows j0 + 4 (lane >> 4) .. +3), gi = the block's group of G, tile = its 64-row tile.
// G == 1: the block holds the whole sum and adds it to out; the workspace is not touched.  Else: partial tile ->
// part[group][t][j], write-through (sc1); the block that completes the row tile's ticket sums the groups in group
// order (an empty group stored zeros) and leaves the ticket at zero for the next launch.  Nobody waits or polls.
__device__ __forceinline__ void mmc_down_finish(const f32x4& tot, int G, int gi, int tile, int j0, int T, int H, float* out,
                                                float* dn_part, int* dn_tick, int* last_s) {
    const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, g = lane >> 4;
    if (G == 1) {
        if (col < T) {
            float4* op = reinterpret_cast<float4*>(out + (long)col * H + j0 + 4 * g);
            float4 o = *op;
            o.x += tot[0]; o.y += tot[1]; o.z += tot[2]; o.w += tot[3];
            *op = o;
        }
        return;
    }
    const auto prs = __builtin_amdgcn_make_buffer_rsrc(dn_part, (short)0, 0x7fffffff, 0x00020000);
    if (col < T) {
        u32x4 bits;
        __builtin_memcpy(&bits, &tot, 16);
        __builtin_amdgcn_raw_buffer_store_b128(bits, prs, (int)((((long)gi * MM_MT + col) * H + j0 + 4 * g) * 4), 0, 16);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        int* tk = dn_tick + tile;
        const int old = __hip_atomic_fetch_add(tk, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = old == G - 1;
        if (last) __hip_atomic_store(tk, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *last_s = last;
    }
    __syncthreads();
    if (!*last_s) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no instruction: keeps the sc1 loads below
    const int t = tid >> 4, j = tile * MMC_DN_RT + 4 * (tid & 15);  // thread = (token, 4 rows) for tid < 128
    if (tid < 128 && t < T) {
        const int base = (int)(((long)t * H + j) * 4), gstride = MM_MT * H * 4;
        float4* op = reinterpret_cast<float4*>(out + (long)t * H + j);
        const float4 o = *op;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
        for (int q = 0; q < G; ++q) {
            const u32x4 pv = __builtin_amdgcn_raw_buffer_load_b128(prs, base + q * gstride, 0, 16);
            v[0] += __uint_as_float(pv[0]); v[1] += __uint_as_float(pv[1]);
            v[2] += __uint_as_float(pv[2]); v[3] += __uint_as_float(pv[3]);
        }
        *op = make_float4(o.x + v[0], o.y + v[1], o.z + v[2], o.w + v[3]);
    }
}

// blocks of `kernel` that are resident at once on the device (persistent grids)
inline int mmc_resident_blocks(const void* kernel, int threads, size_t lds) {
    int per_cu = 0, dev = 0, cus = 0;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds);
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return std::max(1, per_cu) * std::max(1, cus);
}

// bytes of the three staged planes of MM_MT token rows of K elements
inline size_t mmc_plane_bytes(int K) { return sizeof(uint16_t) * 3 * MM_MT * (size_t)mm_pitch(K); }

// groups of segments per 64-row tile of a down launch: enough blocks for three per CU, at most one group per routed
// slot (the workspace's size: moe_down_mm_part_floats), one when the launch has no workspace
template <typename Args>
inline int mmc_down_groups(const Args& a) {
    if (!a.dn_part || !a.dn_tick) return 1;
    const int tiles = a.H / MMC_DN_RT;
    return std::max(1, std::min((768 + tiles - 1) / tiles, a.slots));
}

}  // namespace dsocr
