// Decode sessions (Engine::session_*): one page's decode state moved between two slots of the running batch,
// and a new slot's scalar rows and context written from one staged host buffer.  Neither kernel synchronises
// across workgroups: every block reads the source slot's rows and writes the destination slot's (src != dst).
#include "dev_common.hpp"

namespace dsocr {

constexpr int SM_BLOCK = 256;
constexpr int SM_VEC = 4;  // 16-byte chunks per thread and cache (K, V): all loaded before the first store

// Grid (row chunks + 1, kv heads, layers).  Blocks x < gridDim.x - 1 copy K and V rows [0, kv_len) of one
// (layer, kv head): rows are hd floats back to back, so the range is one contiguous run of kv_len * hd / 4
// 16-byte chunks, read and written by consecutive lanes (nontemporal: ~150 MB at a full-size 1200-row page,
// read once and not read again before the next decode step streams it).  The last x block of (head 0, layer 0)
// moves the slot's small rows; thread 0 of it writes the scalars.
__global__ __launch_bounds__(SM_BLOCK) void session_slot_move_kernel(SlotMoveArgs a) {
    const int nchunk = (int)gridDim.x - 1;
    if ((int)blockIdx.x < nchunk) {
        const int rows = min(min(a.kv_len[a.src], a.rows_bound), a.cap_rows);
        const long n16 = (long)rows * a.hd / 4;
        const long base = (long)blockIdx.z * a.layer_stride + (long)blockIdx.y * a.head_stride;
        const long so = base + (long)a.src * a.page_stride, dof = base + (long)a.dst * a.page_stride;
        const long c0 = (long)blockIdx.x * SM_BLOCK * SM_VEC + threadIdx.x;
        f32x4 k[SM_VEC], v[SM_VEC];
#pragma unroll
        for (int u = 0; u < SM_VEC; ++u) {
            const long c = c0 + (long)u * SM_BLOCK;
            if (c < n16) {
                k[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.kc + so) + c);
                v[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.vc + so) + c);
            }
        }
#pragma unroll
        for (int u = 0; u < SM_VEC; ++u) {
            const long c = c0 + (long)u * SM_BLOCK;
            if (c < n16) {
                __builtin_nontemporal_store(k[u], reinterpret_cast<f32x4*>(a.kc + dof) + c);
                __builtin_nontemporal_store(v[u], reinterpret_cast<f32x4*>(a.vc + dof) + c);
            }
        }
        return;
    }
    if (blockIdx.y || blockIdx.z) return;
    const int t = threadIdx.x, s = a.src, d = a.dst;
    if (a.ctx)
        for (long i = t; i < a.ctx_cap; i += SM_BLOCK) a.ctx[(long)d * a.ctx_cap + i] = a.ctx[(long)s * a.ctx_cap + i];
    if (a.out)
        for (long i = t; i < a.out_cap; i += SM_BLOCK) a.out[(long)d * a.out_cap + i] = a.out[(long)s * a.out_cap + i];
    if (a.ban)
        for (long i = t; i < a.ban_ld; i += SM_BLOCK) a.ban[(long)d * a.ban_ld + i] = a.ban[(long)s * a.ban_ld + i];
    if (a.rng)
        for (int i = t; i < a.rng_words; i += SM_BLOCK) a.rng[(long)d * a.rng_words + i] = a.rng[(long)s * a.rng_words + i];
    if (a.x)
        for (int i = t; i < a.H; i += SM_BLOCK) a.x[(long)d * a.H + i] = a.x[(long)s * a.H + i];
    if (a.rowpar && t < ROWPAR_INTS)
        reinterpret_cast<int*>(a.rowpar + d)[t] = reinterpret_cast<const int*>(a.rowpar + s)[t];
    if (a.lp && a.out_len) {
        const long n = min((long)a.out_len[s], a.out_cap), so = (long)s * a.out_cap, dof = (long)d * a.out_cap;
        for (long i = t; i < n; i += SM_BLOCK) a.lp[dof + i] = a.lp[so + i];
        for (long i = t; i < n * a.lp_k; i += SM_BLOCK) {
            a.lp_top_id[dof * a.lp_k + i] = a.lp_top_id[so * a.lp_k + i];
            a.lp_top[dof * a.lp_k + i] = a.lp_top[so * a.lp_k + i];
        }
    }
    if (t == 0) {
        a.kv_len[d] = a.kv_len[s];
        if (a.kv_pos) a.kv_pos[d] = a.kv_pos[s];
        if (a.ctx_len) a.ctx_len[d] = a.ctx_len[s];
        if (a.out_len) a.out_len[d] = a.out_len[s];
        if (a.done) a.done[d] = a.done[s];
        if (a.tok) a.tok[d] = a.tok[s];
    }
}

void launch_session_slot_move(const SlotMoveArgs& a, hipStream_t s) {
    if (!a.kc || !a.vc || !a.kv_len) throw std::runtime_error("EINVAL: slot move needs the K / V caches and kv_len");
    if (a.src == a.dst || a.src < 0 || a.dst < 0 || a.src >= a.slots || a.dst >= a.slots)
        throw std::runtime_error("EINVAL: slot move needs two different slots inside the session");
    if (a.layers <= 0 || a.kv_heads <= 0 || a.hd <= 0 || a.hd % 4 || a.cap_rows <= 0)
        throw std::runtime_error("EINVAL: slot move needs head_dim % 4 == 0 and a positive shape");
    if (a.head_stride < (long)a.cap_rows * a.hd || a.page_stride < (long)a.kv_heads * a.head_stride ||
        a.layer_stride < (long)a.slots * a.page_stride || a.head_stride % 4 || a.page_stride % 4 || a.layer_stride % 4)
        throw std::runtime_error("EINVAL: slot move strides do not hold the cache shape (or break 16-byte alignment)");
    if ((reinterpret_cast<uintptr_t>(a.kc) | reinterpret_cast<uintptr_t>(a.vc)) & 15)
        throw std::runtime_error("EINVAL: slot move needs 16-byte aligned caches");
    if (a.lp && (!a.out_len || a.out_cap <= 0 || a.lp_k < 0 || (a.lp_k && (!a.lp_top_id || !a.lp_top))))
        throw std::runtime_error("EINVAL: slot move log-probability rows");
    const int rows = a.rows_bound > 0 ? (a.rows_bound < a.cap_rows ? a.rows_bound : a.cap_rows) : a.cap_rows;
    const long n16 = (long)rows * a.hd / 4;
    const int per = SM_BLOCK * SM_VEC;
    const int nchunk = (int)((n16 + per - 1) / per);
    SlotMoveArgs b = a;
    b.rows_bound = rows;
    DSOCR_LAUNCH(session_slot_move_kernel, dim3(nchunk + 1, a.kv_heads, a.layers), dim3(SM_BLOCK), 0, s, b);
}

// Grid (row chunks, kv heads, layers): rows [0, rows) of one (layer, kv head) are one contiguous run of
// rows * hd / 4 16-byte chunks on both sides (the slot's head starts at row 0, the entry's block is dense), copied
// as in session_slot_move_kernel.  TO_SLOT picks the direction; the entry holds every K block, then every V block.
template <bool TO_SLOT>
__global__ __launch_bounds__(SM_BLOCK) void session_prefix_copy_kernel(PrefixCopyArgs a) {
    const long n16 = (long)a.rows * a.hd / 4;
    const long so = (long)blockIdx.z * a.layer_stride + (long)a.slot * a.page_stride + (long)blockIdx.y * a.head_stride;
    const long eo = ((long)blockIdx.z * a.kv_heads + blockIdx.y) * a.rows * a.hd;
    const long ev = (long)a.layers * a.kv_heads * a.rows * a.hd;  // the entry's V blocks follow its K blocks
    const f32x4* ks = reinterpret_cast<const f32x4*>(TO_SLOT ? a.entry + eo : a.kc + so);
    const f32x4* vs = reinterpret_cast<const f32x4*>(TO_SLOT ? a.entry + ev + eo : a.vc + so);
    f32x4* kd = reinterpret_cast<f32x4*>(TO_SLOT ? a.kc + so : a.entry + eo);
    f32x4* vd = reinterpret_cast<f32x4*>(TO_SLOT ? a.vc + so : a.entry + ev + eo);
    const long c0 = (long)blockIdx.x * SM_BLOCK * SM_VEC + threadIdx.x;
    f32x4 k[SM_VEC], v[SM_VEC];
#pragma unroll
    for (int u = 0; u < SM_VEC; ++u) {
        const long c = c0 + (long)u * SM_BLOCK;
        if (c < n16) {
            k[u] = __builtin_nontemporal_load(ks + c);
            v[u] = __builtin_nontemporal_load(vs + c);
        }
    }
#pragma unroll
    for (int u = 0; u < SM_VEC; ++u) {
        const long c = c0 + (long)u * SM_BLOCK;
        if (c < n16) {
            __builtin_nontemporal_store(k[u], kd + c);
            __builtin_nontemporal_store(v[u], vd + c);
        }
    }
}

void launch_session_prefix_copy(const PrefixCopyArgs& a, hipStream_t s) {
    if (!a.kc || !a.vc || !a.entry) throw std::runtime_error("EINVAL: prefix copy needs the K / V caches and an entry");
    if (a.layers <= 0 || a.kv_heads <= 0 || a.hd <= 0 || a.hd % 4 || a.cap_rows <= 0 || a.slots <= 0)
        throw std::runtime_error("EINVAL: prefix copy needs head_dim % 4 == 0 and a positive shape");
    if (a.slot < 0 || a.slot >= a.slots) throw std::runtime_error("EINVAL: prefix copy slot outside the session");
    if (a.rows < 1 || a.rows > a.cap_rows) throw std::runtime_error("EINVAL: prefix copy rows must be 1..cap_rows");
    if (a.head_stride < (long)a.cap_rows * a.hd || a.page_stride < (long)a.kv_heads * a.head_stride ||
        a.layer_stride < (long)a.slots * a.page_stride || a.head_stride % 4 || a.page_stride % 4 || a.layer_stride % 4)
        throw std::runtime_error("EINVAL: prefix copy strides do not hold the cache shape (or break 16-byte alignment)");
    if ((reinterpret_cast<uintptr_t>(a.kc) | reinterpret_cast<uintptr_t>(a.vc) | reinterpret_cast<uintptr_t>(a.entry)) & 15)
        throw std::runtime_error("EINVAL: prefix copy needs 16-byte aligned caches and entry");
    if (a.kv_heads > 65535 || a.layers > 65535) throw std::runtime_error("EINVAL: prefix copy grid");
    const long n16 = (long)a.rows * a.hd / 4;
    const int per = SM_BLOCK * SM_VEC;
    const dim3 grid((unsigned)((n16 + per - 1) / per), a.kv_heads, a.layers);
    if (a.to_slot) DSOCR_LAUNCH(session_prefix_copy_kernel<true>, grid, dim3(SM_BLOCK), 0, s, a);
    else DSOCR_LAUNCH(session_prefix_copy_kernel<false>, grid, dim3(SM_BLOCK), 0, s, a);
}

// stage: [SS_HEAD header ints (RowParams at SS_ROWPAR) | rng words | ctx ids]; the slot's context row is written whole (zeros past ctx_len)
__global__ __launch_bounds__(SM_BLOCK) void session_slot_init_kernel(SlotInitArgs a) {
    const int* h = a.stage;
    const int d = a.slot;
    const long i = (long)blockIdx.x * SM_BLOCK + threadIdx.x;
    const int n = h[SS_CTX_LEN];
    if (i < a.ctx_cap) a.ctx[(long)d * a.ctx_cap + i] = i < n ? h[SS_HEAD + a.rng_words + i] : 0;
    if (a.lp) {
        const long base = (long)d * a.out_cap, step = (long)gridDim.x * SM_BLOCK;
        for (long j = i; j < a.out_cap; j += step) a.lp[base + j] = -INFINITY;
        for (long j = i; j < a.out_cap * a.lp_k; j += step) {
            a.lp_top_id[base * a.lp_k + j] = -1;
            a.lp_top[base * a.lp_k + j] = -INFINITY;
        }
    }
    if (blockIdx.x) return;
    if (a.rng && (int)threadIdx.x < a.rng_words) a.rng[(long)d * a.rng_words + threadIdx.x] = (uint32_t)h[SS_HEAD + threadIdx.x];
    if (a.rowpar && (int)threadIdx.x < ROWPAR_INTS) reinterpret_cast<int*>(a.rowpar + d)[threadIdx.x] = h[SS_ROWPAR + threadIdx.x];
    if (threadIdx.x == 0) {
        a.ctx_len[d] = n;
        a.kv_pos[d] = h[SS_KV_POS];
        a.kv_len[d] = h[SS_KV_LEN];
        a.done[d] = 0;
        a.out_len[d] = 0;
        a.tok[d] = 0;
        if (a.ban) a.ban[(long)d * a.ban_ld] = 0;
    }
}

void launch_session_slot_init(const SlotInitArgs& a, hipStream_t s) {
    if (!a.stage || !a.ctx || !a.ctx_len || !a.kv_pos || !a.kv_len || !a.done || !a.out_len || !a.tok || a.slot < 0 ||
        a.ctx_cap <= 0 || a.rng_words < 0 || a.rng_words > SM_BLOCK)
        throw std::runtime_error("EINVAL: slot init arguments");
    if (a.lp && (a.out_cap <= 0 || a.lp_k < 0 || (a.lp_k && (!a.lp_top_id || !a.lp_top))))
        throw std::runtime_error("EINVAL: slot init log-probability rows");
    const int blocks = (int)((a.ctx_cap + SM_BLOCK - 1) / SM_BLOCK);
    DSOCR_LAUNCH(session_slot_init_kernel, dim3(blocks), dim3(SM_BLOCK), 0, s, a);
}

}  // namespace dsocr
