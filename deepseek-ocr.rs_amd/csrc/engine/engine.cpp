// DeepSeek-OCR page engine (host orchestration of the gfx950 kernels).
// Reference call stacks followed here: SURVEY §3.2-3.4; per-stage citations inline.
#include "engine.hpp"

#include <algorithm>
#include <chrono>
#include <random>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <fstream>
#include <functional>
#include <sstream>

#include "../common/host_util.hpp"
#include "dsq.hpp"
#include "host_ops.hpp"

namespace dsocr {

// ============================================================================ weight source
namespace {

struct HostMat {
    std::vector<uint16_t> data;
    int dt = WDT_BF16;
};

struct Source {
    std::unique_ptr<SafeTensors> st;
    uint64_t seed = 0;
    bool synth = false;
    int mode = 1;  // dsocr_dtype: 0 f32, 1 f16, 2 bf16
    // .dsq snapshot (crates/dsq-runtime): its records replace the checkpoint's linears, decoded to
    // fp16 on the GPU (dequant); a snapshot linear's bias comes from its record only, as
    // SnapshotLinear::{Quantized, Float} carries it (dsq-runtime/src/lib.rs:336-366)
    const DsqFile* snap = nullptr;
    std::function<void(const DsqRecord&, uint16_t*)> dequant;

    const DsqRecord* snap_weight_of_bias(const std::string& n) const {
        if (!snap || n.size() < 5 || n.compare(n.size() - 5, 5, ".bias") != 0) return nullptr;
        return snap->find(n.substr(0, n.size() - 5) + ".weight");
    }
    bool has(const std::string& n) const {
        if (snap) {
            if (snap->find(n)) return true;
            if (const DsqRecord* r = snap_weight_of_bias(n)) return r->has_bias;
        }
        return synth ? synth_has(n) : st->has(n);
    }

    static bool is_language(const std::string& n) {
        return n.rfind("model.layers.", 0) == 0 || n.rfind("model.embed_tokens.", 0) == 0;
    }
    bool round16(const std::string& n) const { return mode == 1 && is_language(n); }

    // exact f32 values (with the f16 rounding rule applied)
    std::vector<float> f32(const std::string& n, size_t numel) const {
        if (const DsqRecord* r = snap_weight_of_bias(n)) {
            std::vector<float> b = snap->bias(*r);
            if (b.size() != numel)
                throw std::runtime_error("EINVAL: snapshot bias for `" + r->name + "` has " + std::to_string(b.size()) +
                                         " values, expected " + std::to_string(numel));
            return b;
        }
        std::vector<float> out(numel);
        if (synth) {
            std::vector<uint16_t> b(numel);
            synth_bf16(n, seed, numel, b.data());
            for (size_t i = 0; i < numel; ++i) out[i] = bf16_to_f32(b[i]);
        } else {
            const StTensor& t = st->get(n);
            if ((size_t)t.numel() != numel)
                throw std::runtime_error("EINVAL: shape mismatch for `" + n + "`: " + std::to_string(t.numel()) +
                                         " vs expected " + std::to_string(numel));
            if (t.dtype == "BF16") {
                const uint16_t* p = (const uint16_t*)t.data;
                for (size_t i = 0; i < numel; ++i) out[i] = bf16_to_f32(p[i]);
            } else if (t.dtype == "F16") {
                const uint16_t* p = (const uint16_t*)t.data;
                for (size_t i = 0; i < numel; ++i) out[i] = f16_to_f32(p[i]);
            } else if (t.dtype == "F32") {
                std::memcpy(out.data(), t.data, numel * 4);
            } else {
                throw std::runtime_error("EINVAL: unsupported dtype " + t.dtype + " for `" + n + "`");
            }
        }
        if (round16(n))
            for (auto& v : out) v = f16_to_f32(f32_to_f16_rne(v));
        return out;
    }

    // 16-bit storage: f16 for language tensors in f16 mode (bf16 -> f16 RNE, the
    // reference's VarBuilder F16 load), otherwise the checkpoint's own 16-bit type.
    // out_dim / in_dim (when known) are checked against a snapshot record (dsq-runtime/src/lib.rs:326-334)
    HostMat h16(const std::string& n, size_t numel, long out_dim = -1, long in_dim = -1) const {
        HostMat m;
        m.data.resize(numel);
        if (const DsqRecord* r = snap ? snap->find(n) : nullptr) {
            if ((size_t)r->out_dim * r->in_dim != numel || (out_dim >= 0 && (long)r->out_dim != out_dim) ||
                (in_dim >= 0 && (long)r->in_dim != in_dim))
                throw std::runtime_error("EINVAL: snapshot tensor `" + n + "` dims mismatch (" + std::to_string(r->out_dim) +
                                         "x" + std::to_string(r->in_dim) + " for " + std::to_string(numel) + " values)");
            dequant(*r, m.data.data());
            m.dt = WDT_F16;
            return m;
        }
        const bool to_f16 = round16(n);
        if (synth) {
            synth_bf16(n, seed, numel, m.data.data());
            if (to_f16) {
#pragma omp parallel for schedule(static)
                for (long i = 0; i < (long)numel; ++i) m.data[i] = f32_to_f16_rne(bf16_to_f32(m.data[i]));
                m.dt = WDT_F16;
            } else {
                m.dt = WDT_BF16;
            }
            return m;
        }
        const StTensor& t = st->get(n);
        if ((size_t)t.numel() != numel)
            throw std::runtime_error("EINVAL: shape mismatch for `" + n + "`: " + std::to_string(t.numel()) +
                                     " vs expected " + std::to_string(numel));
        const uint16_t* p = (const uint16_t*)t.data;
        if (t.dtype == "BF16") {
            if (to_f16) {
#pragma omp parallel for schedule(static)
                for (long i = 0; i < (long)numel; ++i) m.data[i] = f32_to_f16_rne(bf16_to_f32(p[i]));
                m.dt = WDT_F16;
            } else {
                std::memcpy(m.data.data(), p, numel * 2);
                m.dt = WDT_BF16;
            }
        } else if (t.dtype == "F16") {
            std::memcpy(m.data.data(), p, numel * 2);
            m.dt = WDT_F16;
        } else if (t.dtype == "F32" && to_f16) {
            const float* f = (const float*)t.data;
            for (size_t i = 0; i < numel; ++i) m.data[i] = f32_to_f16_rne(f[i]);
            m.dt = WDT_F16;
        } else {
            throw std::runtime_error("EINVAL: matrix `" + n + "` has dtype " + t.dtype +
                                     "; only BF16/F16 checkpoints are supported for large tensors");
        }
        return m;
    }
};

std::string read_file(const std::string& p) {
    std::ifstream f(p);
    if (!f) throw std::runtime_error("ENOENT: cannot read config " + p);
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

double ms_between(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, a, b);
    return ms;
}

}  // namespace

// One decode session (Engine::session_*, after generate below): the state that outlives a call.  The device rows
// live in the engine's decode rows (rows_), reserved once at session_open for `S` slots; the graphs hold their addresses.
struct Engine::Session {
    static constexpr int kBurstCap = 8;  // k_max: the most steps one session_step replays
    int S = 0, n = 0, max_context = 0;
    GenParams p;
    SessionFeatures feat;   // what the session was opened with: which rows every slot has (RowParams, s_lp*, s_bias, s_stop*)
    bool screened = false;  // fixed parameters: the screened head at every n (else the exact head at every n)
    int* stage = nullptr;   // ss_stage: an admission's staged slot rows
    struct Slot {
        // Controls::active() of the slot's page: which of its device flags / records are on (rows_.bias_on, stop_n,
        // pen, ngw, g_on), and the automaton's sizes, which a move copies
        unsigned ctl = 0;
        int g_states = 0;
        long g_edges = 0;
        size_t max_new = 0;
        int kv_pos = 0;    // the device kv_pos of the slot: prompt + steps replayed since its admission
        int reported = 0;  // tokens the polls have handed out
        RowParams rp;      // host copy of the slot's device record (per_request)
        int prompt = 0;    // prompt rows: K/V rows [0, prompt) never change after the admission
        std::vector<int> ids;       // the prompt's ids and mask (what a prefix entry kept from this slot carries)
        std::vector<uint8_t> mask;
    };
    // A page prefix: K/V rows [0, rows) of every layer and kv head ([layers][kv_heads][rows][hd] of K, then of V) in
    // a device allocation of its own (no captured graph reads it: not a frozen workspace), with the ids and mask of
    // those rows for checking a later prompt against them.  Freed with the session or by session_prefix_drop.
    struct PrefixEntry {
        DeviceBuffer kv;
        int rows = 0;
        std::vector<int> ids;
        std::vector<uint8_t> mask;
    };
    std::map<int, PrefixEntry> prefix;  // handle -> entry (at most Engine::kMaxPrefixEntries)
    int next_handle = 1;
    size_t prefix_admissions = 0, prefix_rows_reused = 0;
    std::vector<Slot> slot;
    // the controls some active slot carries: what a burst's head and step graph depend on
    unsigned carried() const {
        unsigned m = 0;
        for (int b = 0; b < n; ++b) m |= slot[b].ctl;
        return m;
    }
    std::shared_ptr<PendingAdmit> pending;  // a chunked admission in flight, staged in slot S - 1 (session_admit_begin)
    int next_ticket = 1;
    // the step for n active pages under the [exact, screened] head, [without, with] the stop match launch,
    // [without, with] the windowed-ban launch, captured on first use
    HipGraphExec graph[9][2][2][2];
    bool ban_stale = false;  // the last burst ran its selections at ngram 0 (a windowed burst, fixed parameters)
    size_t head_steps[2] = {0, 0};  // steps replayed under the [exact, screened] head
    PinnedBuffer<int> pin;  // poll: [done | output length] x S, then the decode error flag
    size_t steps = 0;
};

// ============================================================================ lifecycle
void* Engine::dev_alloc(size_t bytes) {
    void* p = nullptr;
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) throw std::runtime_error("ENOMEM: hipMalloc(" + std::to_string(bytes) + ") failed");
    allocations_.push_back(p);
    return p;
}

void* Engine::ws(const std::string& name0, size_t bytes) {
    const std::string name = ws_prefix_.empty() ? name0 : ws_prefix_ + name0;
    auto it = ws_.find(name);
    if (it != ws_.end() && it->second.second >= bytes) return it->second.first;
    if (capturing_) throw std::runtime_error("EINTERNAL: workspace growth during graph capture: " + name);
    if (ws_frozen_.count(name)) throw std::runtime_error("EINTERNAL: workspace growth inside a decode session: " + name);
    if (it != ws_.end()) {
        HIP_CHECK(hipDeviceSynchronize());  // both vision streams may still read it
        HIP_CHECK(hipFree(it->second.first));
    }
    void* p = nullptr;
    size_t cap = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&p, cap);
    if (e != hipSuccess) throw std::runtime_error("ENOMEM: workspace " + name + " (" + std::to_string(cap) + " bytes)");
    ws_[name] = {p, cap};
    return p;
}

Engine::Engine(const std::string& config_path, const std::string& weights_path, int device, int dtype, uint64_t seed,
               const std::string& snapshot_path, uint32_t load_flags)
    : device_(device), dtype_(dtype) {
    if (load_flags & ~1u) throw std::runtime_error("EINVAL: unknown load flags");
    if ((load_flags & 1u) && snapshot_path.empty())
        throw std::runtime_error("EINVAL: packed experts need a .dsq snapshot (snapshot_path)");
    int n = 0;
    HIP_CHECK(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) throw std::runtime_error("EDEVICE: no HIP device with ordinal " + std::to_string(device));
    HIP_CHECK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
        throw std::runtime_error(std::string("EDEVICE: device is ") + prop.gcnArchName + ", engine is built for gfx950");
    HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    cfg_ = resolve_config(Json::parse(read_file(config_path)));
    const LangConfig& L = cfg_.lang;
    if (L.has_lora) throw std::runtime_error("EINVAL: LoRA attention path not yet implemented");  // block.rs:452-454
    if (L.topk_method != "greedy") throw std::runtime_error("EINVAL: MoE topk_method `" + L.topk_method + "` not yet supported (greedy only)");
    if (L.scoring != "softmax" && L.scoring != "sigmoid") throw std::runtime_error("EINVAL: MoE scoring `" + L.scoring + "` not yet supported");
    if (L.hidden_act != "silu" && L.hidden_act != "swish") throw std::runtime_error("EINVAL: activation `" + L.hidden_act + "` not implemented on this engine");
    if (L.n_routed > 256) throw std::runtime_error("EINVAL: at most 256 routed experts supported");
    if (L.topk > 8) throw std::runtime_error("EINVAL: at most 8 experts per token supported");
    if (!snapshot_path.empty() && dtype != 1)
        throw std::runtime_error("EINVAL: .dsq snapshots load as fp16 (dequant-on-load): use dtype f16");
    if (!snapshot_path.empty() && cfg_.variant == VARIANT_OCR2)
        throw std::runtime_error("EINVAL: .dsq snapshots are not supported for DeepSeek-OCR-2 configs (load the checkpoint without snapshot_path)");
    load_weights(weights_path, seed, snapshot_path, (load_flags & 1u) != 0);
    ensure_rope(4096);
    ensure_small(64);
    HIP_CHECK(hipStreamSynchronize(stream_));
}

PagePixels::~PagePixels() {
    if (global_dev) (void)hipFree(global_dev);
    if (tiles_dev) (void)hipFree(tiles_dev);
}

void* Engine::pinned(const std::string& name, size_t bytes) {
    auto it = pinned_.find(name);
    if (it != pinned_.end() && it->second.second >= bytes) return it->second.first;
    if (it != pinned_.end()) {
        HIP_CHECK(hipStreamSynchronize(stream_));  // an in-flight copy may still read the old buffer
        (void)hipHostFree(it->second.first);
    }
    void* h = nullptr;
    const size_t cap = bytes + bytes / 8 + 256;
    if (hipHostMalloc(&h, cap) != hipSuccess) throw std::runtime_error("ENOMEM: pinned staging " + name);
    pinned_[name] = {h, cap};
    return h;
}

// Stage a page's preprocessed pixels in HBM once (outside any timed region): generate() then
// gathers them device-to-device.
void Engine::upload_page(PagePixels& pg) {
    if (pg.global_dev && pg.dev_ordinal == device_) return;
    if (pg.global_chw.empty()) throw std::runtime_error("EINVAL: page pixels live on another device");
    if (pg.global_dev) { (void)hipFree(pg.global_dev); pg.global_dev = nullptr; }
    if (pg.tiles_dev) { (void)hipFree(pg.tiles_dev); pg.tiles_dev = nullptr; }
    HIP_CHECK(hipMalloc(&pg.global_dev, pg.global_chw.size() * 4));
    HIP_CHECK(hipMemcpy(pg.global_dev, pg.global_chw.data(), pg.global_chw.size() * 4, hipMemcpyHostToDevice));
    if (!pg.tiles_chw.empty()) {
        HIP_CHECK(hipMalloc(&pg.tiles_dev, pg.tiles_chw.size() * 4));
        HIP_CHECK(hipMemcpy(pg.tiles_dev, pg.tiles_chw.data(), pg.tiles_chw.size() * 4, hipMemcpyHostToDevice));
    }
    pg.dev_ordinal = device_;
}

// a1-a3 on the GPU (preprocess.hip): the page's RGB8 bytes go up once; the tap tables and the
// geometry come from the host functions the host path uses; the f32 CHW tensors are produced in
// HBM (px.global_dev / px.tiles_dev), bit-identical to dsocr_prepare_page's arrays
void Engine::prepare_page_device(const uint8_t* rgb, int w, int h, PagePixels& px) {
    hipStream_t st = stream_;
    const int G = px.crop ? px.base : px.tile;  // model/mod.rs:1714
    if (px.variant == VARIANT_OCR2) check_ocr2_view_size(G, "global view");
    px.gsize = G;
    if (px.global_dev) { (void)hipFree(px.global_dev); px.global_dev = nullptr; }
    if (px.tiles_dev) { (void)hipFree(px.tiles_dev); px.tiles_dev = nullptr; }
    HIP_CHECK(hipMalloc(&px.global_dev, (size_t)3 * G * G * 4));
    const size_t nbytes = (size_t)w * h * 3;
    uint8_t* d_rgb = nbytes ? (uint8_t*)ws("pp_rgb", nbytes) : nullptr;
    if (nbytes) HIP_CHECK(hipMemcpyAsync(d_rgb, rgb, nbytes, hipMemcpyHostToDevice, st));
    auto upload_taps = [&](const ResampleCoeffs& rc, const char* name) -> std::pair<int*, int*> {
        std::vector<int> b(rc.bounds.size() * 2);
        for (size_t i = 0; i < rc.bounds.size(); ++i) { b[2 * i] = rc.bounds[i].first; b[2 * i + 1] = rc.bounds[i].second; }
        int* db = (int*)ws(std::string(name) + "_b", b.size() * 4);
        int* dc = (int*)ws(std::string(name) + "_c", rc.coeffs.size() * 4);
        HIP_CHECK(hipMemcpyAsync(db, b.data(), b.size() * 4, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(dc, rc.coeffs.data(), rc.coeffs.size() * 4, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));  // the host tables die with this lambda
        return {db, dc};
    };
    // ---- global view
    PpOut g;
    g.mode = 0; g.size = G; g.n_out = 1; g.out = px.global_dev;
    if (w > 0 && h > 0) {
        int nw, nh, xo, yo;
        global_view_geometry(w, h, G, &nw, &nh, &xo, &yo);
        const ResampleCoeffs cx = compute_resample_coeffs(w, nw), cy = compute_resample_coeffs(h, nh);
        auto tx = upload_taps(cx, "pp_gx");
        auto ty = upload_taps(cy, "pp_gy");
        uint8_t* hz = (uint8_t*)ws("pp_hz", (size_t)h * nw * 3);
        launch_pp_resize_h(d_rgb, w, h, tx.first, tx.second, cx.ksize, nw, hz, st);
        g.hz = hz; g.dw = nw; g.bounds = ty.first; g.coeffs = ty.second; g.ksize = cy.ksize;
        g.ox = xo; g.oy = yo; g.nw = nw; g.nh = nh;
    }
    launch_pp_resize_v_chw(g, st);
    // ---- tiles (vision/preprocess.rs:67-138, PreprocessParams::ocr1: 2..9 tiles)
    px.n_tiles = 0;
    px.crop_w = px.crop_h = 1;
    int gw = 1, gh = 1;
    if (px.crop && w > 0 && h > 0 && choose_tile_grid(w, h, px.tile, 2, tile_max_num(px.variant), &gw, &gh)) {
        if (px.variant == VARIANT_OCR2) check_ocr2_view_size(px.tile, "tile");
        const int T = px.tile, tw = T * gw, th = T * gh;
        px.crop_w = gw;
        px.crop_h = gh;
        px.n_tiles = gw * gh;
        HIP_CHECK(hipMalloc(&px.tiles_dev, (size_t)px.n_tiles * 3 * T * T * 4));
        const ResampleCoeffs cx = compute_resample_coeffs(w, tw), cy = compute_resample_coeffs(h, th);
        auto tx = upload_taps(cx, "pp_tx");
        auto ty = upload_taps(cy, "pp_ty");
        uint8_t* hz = (uint8_t*)ws("pp_thz", (size_t)h * tw * 3);
        launch_pp_resize_h(d_rgb, w, h, tx.first, tx.second, cx.ksize, tw, hz, st);
        PpOut t;
        t.mode = 1; t.size = T; t.n_out = px.n_tiles; t.grid_w = gw; t.out = px.tiles_dev;
        t.hz = hz; t.dw = tw; t.bounds = ty.first; t.coeffs = ty.second; t.ksize = cy.ksize;
        launch_pp_resize_v_chw(t, st);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(st));
    px.global_chw.clear();
    px.tiles_chw.clear();
    px.dev_ordinal = device_;
    px.n_image_tokens = image_placeholder_count(px.base, px.tile, px.crop, px.crop_w, px.crop_h, px.variant);
}

Engine::~Engine() {
    if (stream_) (void)hipStreamSynchronize(stream_);
    if (vstream_) (void)hipStreamSynchronize(vstream_);
    for (auto& e : vis_ev_)  // (span_ev_ and persist_ev_ own their events)
        if (e) (void)hipEventDestroy(e);
    for (auto& kv : pinned_) (void)hipHostFree(kv.second.first);
    for (auto& kv : winmaps_) { (void)hipFree(kv.second.first); (void)hipFree(kv.second.second); }
    for (auto& kv : ws_) (void)hipFree(kv.second.first);
    for (void* p : allocations_) (void)hipFree(p);
    if (stream_) (void)hipStreamDestroy(stream_);
    if (vstream_) (void)hipStreamDestroy(vstream_);
}

void Engine::ensure_small(int n) {
    if (n <= small_cap_) return;
    std::vector<float> ones(n, 1.f);
    std::vector<int> iota(n);
    for (int i = 0; i < n; ++i) iota[i] = i;
    ones_ = (float*)dev_alloc(n * sizeof(float));
    iota_ = (int*)dev_alloc(n * sizeof(int));
    HIP_CHECK(hipMemcpy(ones_, ones.data(), n * sizeof(float), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(iota_, iota.data(), n * sizeof(int), hipMemcpyHostToDevice));
    small_cap_ = n;
}

// RoPE tables exactly as rope.rs:172-207 (f32 inv_freq, angle = pos * inv_freq, [half | half]).
void Engine::ensure_rope(int len) {
    if (len <= rope_cap_) return;
    int cap = rope_cap_ > 0 ? rope_cap_ : 1;
    while (cap < len) cap *= 2;
    const int rd = cfg_.lang.rope_dim, half = rd / 2;
    std::vector<float> inv(half), c((size_t)cap * rd), s((size_t)cap * rd);
    for (int i = 0; i < half; ++i) inv[i] = 1.0f / powf(cfg_.lang.rope_theta, ((float)i * 2.0f) / (float)rd);
    for (int p = 0; p < cap; ++p)
        for (int i = 0; i < half; ++i) {
            float a = (float)p * inv[i];
            c[(size_t)p * rd + i] = c[(size_t)p * rd + half + i] = cosf(a);
            s[(size_t)p * rd + i] = s[(size_t)p * rd + half + i] = sinf(a);
        }
    rope_cos_ = (float*)dev_alloc(c.size() * 4);
    rope_sin_ = (float*)dev_alloc(s.size() * 4);
    HIP_CHECK(hipMemcpy(rope_cos_, c.data(), c.size() * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(rope_sin_, s.data(), s.size() * 4, hipMemcpyHostToDevice));
    rope_cap_ = cap;
}

// ============================================================================ loading
void Engine::packed_info(size_t* packed_layers, size_t* moe_layers, size_t* packed_bytes) const {
    size_t pl = 0, ml = 0, pb = 0;
    for (const DecLayer& d : layers_) {
        if (!d.moe) continue;
        ++ml;
        if (d.packed) { ++pl; pb += d.packed_bytes; }
    }
    if (packed_layers) *packed_layers = pl;
    if (moe_layers) *moe_layers = ml;
    if (packed_bytes) *packed_bytes = pb;
}

void Engine::load_weights(const std::string& path, uint64_t seed, const std::string& snapshot_path, bool packed_experts) {
    Source src;
    src.mode = dtype_;
    if (path.empty()) {
        src.synth = true;
        src.seed = seed;
    } else {
        src.st.reset(new SafeTensors(path));
    }
    std::unique_ptr<DsqFile> snap;
    if (!snapshot_path.empty()) {
        snap.reset(new DsqFile(snapshot_path));
        src.snap = snap.get();
        src.dequant = [&](const DsqRecord& r, uint16_t* host_out) {
            const size_t need = dsq_payload_bytes(r.q_dtype, r.out_dim, r.in_dim);
            if (r.q_len != need)
                throw std::runtime_error("EINVAL: snapshot tensor `" + r.name + "` payload is " + std::to_string(r.q_len) +
                                         " bytes, expected " + std::to_string(need));
            const size_t n = (size_t)r.out_dim * r.in_dim;
            void* d_src = ws("load_dsq_src", need);
            void* d_dst = ws("load_dsq_dst", n * 2);
            HIP_CHECK(hipMemcpyAsync(d_src, snap->payload(r), need, hipMemcpyHostToDevice, stream_));
            launch_dsq_dequant(r.q_dtype, d_src, r.out_dim, r.in_dim, d_dst, stream_);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipMemcpyAsync(host_out, d_dst, n * 2, hipMemcpyDeviceToHost, stream_));
            HIP_CHECK(hipStreamSynchronize(stream_));
        };
    }
    // packed experts: the records `names` (each rows_each x in_dim, one Q4_K / Q8_0 dtype for all, no bias) kept
    // as one packed table in that order; records_qtype: their common dtype, -1 when one is missing or of another kind
    auto records_qtype = [&](const std::vector<std::string>& names, long rows_each, long in_dim) -> int {
        if (!snap || names.empty()) return -1;
        int qt = -1;
        for (const std::string& n : names) {
            const DsqRecord* r = snap->find(n);
            if (!r || r->has_bias || (long)r->out_dim != rows_each || (long)r->in_dim != in_dim) return -1;
            if (qt < 0) qt = r->q_dtype;
            if (r->q_dtype != qt || !dsq_packed_ok(qt, in_dim)) return -1;
            if (r->q_len != dsq_payload_bytes(qt, rows_each, in_dim)) return -1;
        }
        return qt;
    };
    auto pack_records = [&](const std::vector<std::string>& names, long rows_each, long in_dim, QMat& out, size_t& bytes) {
        const int qt = records_qtype(names, rows_each, in_dim);
        if (qt < 0) throw std::logic_error("pack_records on records that were not checked");
        const long total = rows_each * (long)names.size();
        const size_t nbytes = dsq_packed_bytes(qt, total, in_dim);
        void* buf = dev_alloc(nbytes);
        out = dsq_packed_view(qt, buf, total, in_dim);
        long row0 = 0;
        for (const std::string& n : names) {
            const DsqRecord* r = snap->find(n);
            void* d_src = ws("load_dsq_src", r->q_len);
            HIP_CHECK(hipMemcpyAsync(d_src, snap->payload(*r), r->q_len, hipMemcpyHostToDevice, stream_));
            launch_dsq_repack(out, row0, d_src, rows_each, in_dim, stream_);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipStreamSynchronize(stream_));  // (the staging buffer is reused by the next record)
            row0 += rows_each;
        }
        bytes += nbytes;
    };
    auto up16 = [&](const HostMat& m) -> void* {
        void* p = dev_alloc(m.data.size() * 2);
        HIP_CHECK(hipMemcpy(p, m.data.data(), m.data.size() * 2, hipMemcpyHostToDevice));
        return p;
    };
    auto upf = [&](const std::vector<float>& v) -> float* {
        float* p = (float*)dev_alloc(v.size() * 4);
        HIP_CHECK(hipMemcpy(p, v.data(), v.size() * 4, hipMemcpyHostToDevice));
        return p;
    };
    auto vecf = [&](const std::string& n, size_t numel) -> float* { return upf(src.f32(n, numel)); };
    auto optvec = [&](const std::string& n, size_t numel) -> float* { return src.has(n) ? vecf(n, numel) : nullptr; };
    auto lin = [&](const std::string& pre, int N, int K, bool allow_bias) -> Lin {
        Lin l;
        HostMat m = src.h16(pre + ".weight", (size_t)N * K, N, K);
        l.W = up16(m);
        l.wdt = m.dt;
        l.N = N;
        l.K = K;
        if (allow_bias && src.has(pre + ".bias")) l.b = vecf(pre + ".bias", N);
        return l;
    };
    // concatenation of several [Ni][K] matrices (+ optional biases) into one [sum Ni][K]
    auto lin_cat = [&](const std::vector<std::string>& pres, const std::vector<int>& Ns, int K) -> Lin {
        Lin l;
        HostMat all;
        std::vector<float> bias;
        bool any_bias = false;
        int N = 0;
        for (size_t i = 0; i < pres.size(); ++i) {
            HostMat m = src.h16(pres[i] + ".weight", (size_t)Ns[i] * K, Ns[i], K);
            if (i == 0) all.dt = m.dt;
            else if (m.dt != all.dt) throw std::runtime_error("EINVAL: mixed dtypes in fused linear " + pres[i]);
            all.data.insert(all.data.end(), m.data.begin(), m.data.end());
            std::vector<float> b(Ns[i], 0.f);
            if (src.has(pres[i] + ".bias")) { b = src.f32(pres[i] + ".bias", Ns[i]); any_bias = true; }
            bias.insert(bias.end(), b.begin(), b.end());
            N += Ns[i];
        }
        l.W = up16(all);
        l.wdt = all.dt;
        l.N = N;
        l.K = K;
        if (any_bias) l.b = upf(bias);
        return l;
    };
    // conv [O][C][kh][kw] -> [O][kh][kw][C] (NHWC im2col order)
    auto conv = [&](const std::string& n, int O, int C, int kh, int kw) -> Lin {
        HostMat m = src.h16(n, (size_t)O * C * kh * kw);
        HostMat r;
        r.dt = m.dt;
        r.data.resize(m.data.size());
        for (int o = 0; o < O; ++o)
            for (int c = 0; c < C; ++c)
                for (int y = 0; y < kh; ++y)
                    for (int x = 0; x < kw; ++x)
                        r.data[(((size_t)o * kh + y) * kw + x) * C + c] = m.data[(((size_t)o * C + c) * kh + y) * kw + x];
        Lin l;
        l.W = up16(r);
        l.wdt = r.dt;
        l.N = O;
        l.K = C * kh * kw;
        return l;
    };

    // ---------------- SAM (vision/sam.rs:143-184)
    const SamConfig& S = cfg_.sam;
    const std::string sp = "model.sam_model.";
    sam_.patch = lin(sp + "patch_embed.proj", S.dim, 3 * S.patch * S.patch, true);
    const int tps = S.image_size / S.patch;
    if (src.has(sp + "pos_embed")) {
        sam_.has_pos = true;
        sam_.pos_grid = tps;
        std::vector<float> pos = src.f32(sp + "pos_embed", (size_t)tps * tps * S.dim);  // [1][g][g][C]
        sam_.pos_host.resize(pos.size());
        for (int y = 0; y < tps; ++y)
            for (int x = 0; x < tps; ++x)
                for (int c = 0; c < S.dim; ++c)
                    sam_.pos_host[((size_t)c * tps + y) * tps + x] = pos[((size_t)y * tps + x) * S.dim + c];
    }
    const int hd = S.dim / S.heads;
    for (int b = 0; b < S.depth; ++b) {
        SamBlock blk;
        const std::string bp = sp + "blocks." + std::to_string(b) + ".";
        blk.global = S.is_global(b);
        blk.n1 = {vecf(bp + "norm1.weight", S.dim), vecf(bp + "norm1.bias", S.dim)};
        blk.n2 = {vecf(bp + "norm2.weight", S.dim), vecf(bp + "norm2.bias", S.dim)};
        blk.qkv = lin(bp + "attn.qkv", 3 * S.dim, S.dim, true);
        blk.proj = lin(bp + "attn.proj", S.dim, S.dim, true);
        const int hid = (int)(S.dim * S.mlp_ratio);
        std::string f1 = src.has(bp + "mlp.fc1.weight") ? "mlp.fc1" : "mlp.lin1";
        std::string f2 = src.has(bp + "mlp.fc2.weight") ? "mlp.fc2" : "mlp.lin2";
        blk.fc1 = lin(bp + f1, hid, S.dim, true);
        blk.fc2 = lin(bp + f2, S.dim, hid, true);
        blk.use_rel = src.has(bp + "attn.rel_pos_h");
        if (blk.use_rel) {
            const int tokens = blk.global ? tps : S.window;
            blk.rel_len = 2 * tokens - 1;
            blk.relh = src.f32(bp + "attn.rel_pos_h", (size_t)blk.rel_len * hd);
            blk.relw = src.f32(bp + "attn.rel_pos_w", (size_t)blk.rel_len * hd);
        }
        sam_.blocks.push_back(std::move(blk));
    }
    sam_.neck0 = conv(sp + "neck.0.weight", S.neck, S.dim, 1, 1);
    sam_.neck1 = {vecf(sp + "neck.1.weight", S.neck), vecf(sp + "neck.1.bias", S.neck)};
    sam_.neck2 = conv(sp + "neck.2.weight", S.neck, S.neck, 3, 3);
    sam_.neck3 = {vecf(sp + "neck.3.weight", S.neck), vecf(sp + "neck.3.bias", S.neck)};
    sam_.net2 = conv(sp + "net_2.weight", S.out_ch[0], S.neck, 3, 3);
    sam_.net3 = conv(sp + "net_3.weight", S.out_ch[1], S.out_ch[0], 3, 3);

    if (cfg_.variant == VARIANT_OCR2) {
        // ---------------- Qwen2 encoder (vision/qwen2.rs:116-144, transformer/weights.rs:180-262): names under
        // model.qwen2_model. contain "model.layers." but are vision tensors (Source::is_language tests the prefix),
        // so they keep the checkpoint's values in every dtype mode (model/mod.rs:1039-1071)
        const Qwen2EncConfig& Q = cfg_.enc;
        const std::string qp = "model.qwen2_model.";
        const int D = Q.dim, hd = Q.head_dim, KV = Q.kv_heads * hd;
        // biases: q/k/v only (attention_bias), none on o_proj or the MLP
        auto lin_nobias = [&](const std::string& pre, int N, int K) { return lin(pre, N, K, false); };
        for (int l = 0; l < Q.layers; ++l) {
            EncLayer e;
            const std::string lp = qp + "model.model.layers." + std::to_string(l) + ".";
            e.in_norm = {vecf(lp + "input_layernorm.weight", D), nullptr};
            e.post_norm = {vecf(lp + "post_attention_layernorm.weight", D), nullptr};
            e.qkv = lin_cat({lp + "self_attn.q_proj", lp + "self_attn.k_proj", lp + "self_attn.v_proj"}, {Q.heads * hd, KV, KV}, D);
            e.o = lin_nobias(lp + "self_attn.o_proj", D, Q.heads * hd);
            HostMat g = src.h16(lp + "mlp.gate_proj.weight", (size_t)Q.inter * D, Q.inter, D);
            HostMat u = src.h16(lp + "mlp.up_proj.weight", (size_t)Q.inter * D, Q.inter, D);
            if (g.dt != u.dt) throw std::runtime_error("EINVAL: mixed dtypes in fused linear " + lp + "mlp");
            g.data.insert(g.data.end(), u.data.begin(), u.data.end());
            e.gu.W = up16(g);
            e.gu.wdt = g.dt;
            e.gu.N = 2 * Q.inter;
            e.gu.K = D;
            e.down = lin_nobias(lp + "mlp.down_proj", D, Q.inter);
            enc_.layers.push_back(e);
        }
        enc_.norm = vecf(qp + "model.model.norm.weight", D);
        enc_.query_768 = vecf(qp + "query_768.weight", (size_t)Q.query_768 * D);
        enc_.query_1024 = vecf(qp + "query_1024.weight", (size_t)Q.query_1024 * D);
        {   // build_rope_tables (qwen2.rs:573-604): inv_freq = 1 / theta^(i / half) (f32 powf), f32 angles, [half | half]
            const int Lmax = 2 * Q.query_1024, half = hd / 2;
            std::vector<float> inv(half), c((size_t)Lmax * hd), s((size_t)Lmax * hd);
            for (int i = 0; i < half; ++i) inv[i] = 1.0f / powf(Q.rope_theta, (float)i / (float)half);
            for (int p = 0; p < Lmax; ++p)
                for (int i = 0; i < half; ++i) {
                    const float a = (float)p * inv[i];
                    c[(size_t)p * hd + i] = c[(size_t)p * hd + half + i] = cosf(a);
                    s[(size_t)p * hd + i] = s[(size_t)p * hd + half + i] = sinf(a);
                }
            enc_.cos = upf(c);
            enc_.sin = upf(s);
        }
        if (S.out_ch[1] != D) throw std::runtime_error("EINVAL: SAM output channels must equal the qwen2-0-5b encoder width");
    } else {
    // ---------------- CLIP (vision/clip.rs:73-88)
    const ClipConfig& C = cfg_.clip;
    const std::string cp = "model.vision_model.";
    clip_.cls = vecf(cp + "embeddings.class_embedding", C.hidden);
    clip_.pos_host = src.f32(cp + "embeddings.position_embedding.weight", (size_t)(C.seq + 1) * C.hidden);
    clip_.pre = {vecf(cp + "pre_layrnorm.weight", C.hidden), vecf(cp + "pre_layrnorm.bias", C.hidden)};
    for (int l = 0; l < C.layers; ++l) {
        ClipLayer cl;
        const std::string lp = cp + "transformer.layers." + std::to_string(l) + ".";
        cl.ln1 = {vecf(lp + "layer_norm1.weight", C.hidden), vecf(lp + "layer_norm1.bias", C.hidden)};
        cl.ln2 = {vecf(lp + "layer_norm2.weight", C.hidden), vecf(lp + "layer_norm2.bias", C.hidden)};
        cl.qkv = lin(lp + "self_attn.qkv_proj", 3 * C.hidden, C.hidden, true);
        cl.out = lin(lp + "self_attn.out_proj", C.hidden, C.hidden, true);
        cl.fc1 = lin(lp + "mlp.fc1", C.ffn, C.hidden, true);
        cl.fc2 = lin(lp + "mlp.fc2", C.hidden, C.ffn, true);
        clip_.layers.push_back(cl);
    }
    if (C.hidden != S.out_ch[1]) throw std::runtime_error("EINVAL: CLIP width must equal SAM output channels");
    if (C.hidden + S.out_ch[1] != cfg_.proj_in) throw std::runtime_error("EINVAL: combined hidden dims do not match projector input");
    }

    // ---------------- projector (model/mod.rs:258-390; Ocr2: one biased linear, qwen2.rs:407-444)
    proj_ = lin("model.projector.layers", cfg_.proj_out, cfg_.proj_in, true);
    newline_ = cfg_.variant != VARIANT_OCR2 && src.has("model.image_newline")
                   ? vecf("model.image_newline", cfg_.proj_out)
                   : upf(std::vector<float>(cfg_.proj_out, 0.f));  // (Ocr2 has no newline rows)
    separator_ = vecf("model.view_seperator", cfg_.proj_out);

    // ---------------- language model (transformer/weights.rs:444-606)
    const LangConfig& L = cfg_.lang;
    {
        HostMat m = src.h16("model.embed_tokens.weight", (size_t)L.vocab * L.hidden);
        embed_ = up16(m);
        embed_dt_ = m.dt;
    }
    const int H = L.hidden, KVH = L.kv_heads * L.head_dim;
    for (int l = 0; l < L.layers; ++l) {
        DecLayer d;
        const std::string lp = "model.layers." + std::to_string(l) + ".";
        d.in_norm = {vecf(lp + "input_layernorm.weight", H), nullptr};
        d.post_norm = {vecf(lp + "post_attention_layernorm.weight", H), nullptr};
        d.qkv = lin_cat({lp + "self_attn.q_proj", lp + "self_attn.k_proj", lp + "self_attn.v_proj"},
                        {L.heads * L.head_dim, KVH, L.kv_heads * L.v_head_dim}, H);
        d.o = lin(lp + "self_attn.o_proj", H, L.heads * L.v_head_dim, true);
        d.moe = L.moe_layer(l);
        if (!d.moe) {
            d.gu = lin_cat({lp + "mlp.gate_proj", lp + "mlp.up_proj"}, {L.inter, L.inter}, H);
            d.down = lin(lp + "mlp.down_proj", H, L.inter, true);
            if (d.gu.b || d.down.b) throw std::runtime_error("EINVAL: biased dense MLP not supported");
        } else {
            const int E = L.n_routed, I = L.moe_inter;
            HostMat r = src.h16(lp + "mlp.gate.weight", (size_t)E * H);
            d.router.W = up16(r);
            d.router.wdt = r.dt;
            d.router.N = E;
            d.router.K = H;
            d.router.b = optvec(lp + "mlp.gate.e_score_correction_bias", E);
            HostMat gu, dn;
            gu.data.resize((size_t)E * 2 * I * H);
            dn.data.resize((size_t)E * H * I);
            for (int e = 0; e < E; ++e) {
                const std::string ep = lp + "mlp.experts." + std::to_string(e) + ".";
                HostMat g = src.h16(ep + "gate_proj.weight", (size_t)I * H, I, H);
                HostMat u = src.h16(ep + "up_proj.weight", (size_t)I * H, I, H);
                HostMat w = src.h16(ep + "down_proj.weight", (size_t)H * I, H, I);
                if (src.has(ep + "gate_proj.bias") || src.has(ep + "down_proj.bias"))
                    throw std::runtime_error("EINVAL: biased experts not supported");
                std::copy(g.data.begin(), g.data.end(), gu.data.begin() + (size_t)e * 2 * I * H);
                std::copy(u.data.begin(), u.data.end(), gu.data.begin() + (size_t)e * 2 * I * H + (size_t)I * H);
                std::copy(w.data.begin(), w.data.end(), dn.data.begin() + (size_t)e * H * I);
                gu.dt = dn.dt = g.dt;
            }
            d.e_gu = up16(gu);
            d.e_d = up16(dn);
            d.e_wdt = gu.dt;
            if (L.n_shared > 0) {
                const int Is = I * L.n_shared;
                d.has_shared = true;
                d.s_gu = lin_cat({lp + "mlp.shared_experts.gate_proj", lp + "mlp.shared_experts.up_proj"}, {Is, Is}, H);
                d.s_d = lin(lp + "mlp.shared_experts.down_proj", H, Is, true);
            }
            if (packed_experts && d.e_wdt == WDT_F16 && dec_route_grp_ok(8, E, H, L.topk)) {
                // every routed and shared record Q4_K / Q8_0 (one dtype per matrix role): keep the blocks; any
                // other layer runs the fp16 kernels
                std::vector<std::string> gu_n, dn_n;
                for (int e = 0; e < E; ++e) {
                    const std::string ep = lp + "mlp.experts." + std::to_string(e) + ".";
                    gu_n.push_back(ep + "gate_proj.weight");
                    gu_n.push_back(ep + "up_proj.weight");
                    dn_n.push_back(ep + "down_proj.weight");
                }
                const long Is = (long)I * L.n_shared;
                const std::vector<std::string> sgu_n = {lp + "mlp.shared_experts.gate_proj.weight",
                                                        lp + "mlp.shared_experts.up_proj.weight"};
                const std::vector<std::string> sdn_n = {lp + "mlp.shared_experts.down_proj.weight"};
                bool ok = records_qtype(gu_n, I, H) >= 0 && records_qtype(dn_n, H, I) >= 0;
                if (ok && d.has_shared)
                    ok = !d.s_gu.b && !d.s_d.b && records_qtype(sgu_n, Is, H) >= 0 && records_qtype(sdn_n, H, Is) >= 0;
                if (ok) {
                    pack_records(gu_n, I, H, d.q_gu, d.packed_bytes);
                    pack_records(dn_n, H, I, d.q_d, d.packed_bytes);
                    if (d.has_shared) {
                        pack_records(sgu_n, Is, H, d.q_sgu, d.packed_bytes);
                        pack_records(sdn_n, H, Is, d.q_sd, d.packed_bytes);
                    }
                    d.packed = true;
                }
            }
        }
        layers_.push_back(d);
    }
    HIP_CHECK(hipDeviceSynchronize());
    final_norm_ = vecf("model.norm.weight", H);  // f32 copy (model/mod.rs:1008-1014)
    lm_head_ = lin("lm_head", L.vocab, H, false);
    if ((lm_head_.wdt == WDT_BF16 || lm_head_.wdt == WDT_F16) && H % 16 == 0 && H <= 1536) {
        // int8 screening copy of the lm_head (per-row scale + rigorous error bound), lmhead.hip
        // (+ for 3..8 pages: s ||Q|| per row and the fragment-ordered copy the int8 matrix cores read; the
        // per-row arrays padded to whole 16-row tiles)
        const size_t vp = (size_t)(L.vocab + 15) / 16 * 16;
        lmq_ = dev_alloc((size_t)L.vocab * H);
        lmq_scale_ = (float*)dev_alloc(vp * 4);
        lmq_bound_ = (float*)dev_alloc(vp * 4);
        HIP_CHECK(hipMemset(lmq_scale_, 0, vp * 4));
        HIP_CHECK(hipMemset(lmq_bound_, 0, vp * 4));
        if (lmhead_q8mm_ok(8, L.vocab, H)) {
            lmq_qnorm_ = (float*)dev_alloc(vp * 4);
            HIP_CHECK(hipMemset(lmq_qnorm_, 0, vp * 4));
            lmq_frag_ = dev_alloc(lmhead_qfrag_bytes(L.vocab, H));
        }
        launch_lmhead_quantize(lm_head_.W, L.vocab, H, lmq_, lmq_scale_, lmq_bound_, nullptr, lmq_qnorm_, lmq_frag_,
                               lm_head_.wdt);
        HIP_CHECK(hipDeviceSynchronize());
    }
}

// ============================================================================ compute helpers
void Engine::linear(const float* x, int M, int ldx, const Lin& l, float* y, int ldy, int act, int accumulate,
                    const int* c_rows) {
    flops_acc_ += 2.0 * M * (double)l.N * l.K;
    if (M <= 16 && !c_rows) {
        DecGemvArgs a;
        a.M = M; a.N = l.N; a.K = l.K; a.x = x; a.ldx = ldx; a.W = l.W; a.ldw = l.K; a.wdtype = l.wdt;
        a.bias = l.b; a.y = y; a.ldy = ldy; a.act = act; a.accumulate = accumulate;
        launch_dec_gemv(a, stream_);
    } else if ((l.wdt == WDT_F16 || l.wdt == WDT_BF16) && l.K % 32 == 0 && ldx % 4 == 0 &&
               (reinterpret_cast<uintptr_t>(x) & 15) == 0) {
        // the exact-f32 linear on the bf16 matrix cores: the f32 rows split into 3 bf16 planes (and f16
        // weights into hi / lo bf16) inside the GEMM's fragment loads (gemm_bf16.hip, gemm_f32a)
        GemmBf16Args g;
        g.M = M; g.N = l.N; g.K = l.K; g.A = x; g.lda = ldx; g.W = l.W; g.ldw = l.K; g.w_f16 = l.wdt == WDT_F16;
        g.bias = l.b; g.C = y; g.ldc = ldy; g.c_rows = c_rows; g.act = act; g.accumulate = accumulate;
        g.splits = gemm_f32a_splits(M, l.N, l.K);
        if (g.splits > 1) g.part = wsf("g_splitk", (size_t)g.splits * M * l.N);
        launch_gemm_f32a(g, stream_);
    } else {
        GemmArgs g;
        g.M = M; g.N = l.N; g.K = l.K; g.A = x; g.lda = ldx; g.W = l.W; g.ldw = l.K; g.wdtype = l.wdt;
        g.bias = l.b; g.C = y; g.ldc = ldy; g.c_rows = c_rows; g.act = act; g.accumulate = accumulate;
        launch_gemm(g, stream_);
    }
}

float* Engine::sam_pos(int g) {
    auto it = sam_.pos_dev.find(g);
    if (it != sam_.pos_dev.end()) return it->second;
    const int C = cfg_.sam.dim, src = sam_.pos_grid;
    std::vector<float> r = bicubic_resize_aa(sam_.pos_host, C, src, src, g, g);  // sam.rs:982-998
    std::vector<float> nhwc((size_t)g * g * C);
    for (int c = 0; c < C; ++c)
        for (int p = 0; p < g * g; ++p) nhwc[(size_t)p * C + c] = r[(size_t)c * g * g + p];
    float* d = (float*)dev_alloc(nhwc.size() * 4);
    HIP_CHECK(hipMemcpy(d, nhwc.data(), nhwc.size() * 4, hipMemcpyHostToDevice));
    sam_.pos_dev[g] = d;
    return d;
}

std::pair<float*, float*> Engine::sam_rel(SamBlock& b, int g) {
    auto it = b.rel_dev.find(g);
    if (it != b.rel_dev.end()) return it->second;
    const int hd = cfg_.sam.dim / cfg_.sam.heads;
    std::vector<float> rh = rel_pos_resize(b.relh, b.rel_len, hd, g);
    std::vector<float> rw = rel_pos_resize(b.relw, b.rel_len, hd, g);
    float* dh = (float*)dev_alloc(rh.size() * 4);
    float* dw = (float*)dev_alloc(rw.size() * 4);
    HIP_CHECK(hipMemcpy(dh, rh.data(), rh.size() * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dw, rw.data(), rw.size() * 4, hipMemcpyHostToDevice));
    b.rel_dev[g] = {dh, dw};
    return {dh, dw};
}

float* Engine::clip_pos(int tokens) {
    auto it = clip_.pos_dev.find(tokens);
    if (it != clip_.pos_dev.end()) return it->second;
    const ClipConfig& C = cfg_.clip;
    std::vector<float> out;
    if (tokens == C.seq + 1) {
        out = clip_.pos_host;
    } else {  // clip.rs:486-544
        const int s = (int)std::lround(std::sqrt((double)C.seq)), t = (int)std::lround(std::sqrt((double)(tokens - 1)));
        if (t * t != tokens - 1) throw std::runtime_error("EINVAL: clip positional table tgt tokens not square");
        std::vector<float> grid((size_t)C.hidden * s * s);
        for (int p = 0; p < s * s; ++p)
            for (int c = 0; c < C.hidden; ++c) grid[(size_t)c * s * s + p] = clip_.pos_host[(size_t)(1 + p) * C.hidden + c];
        std::vector<float> r = bicubic_resize_aa(grid, C.hidden, s, s, t, t);
        out.resize((size_t)tokens * C.hidden);
        std::copy(clip_.pos_host.begin(), clip_.pos_host.begin() + C.hidden, out.begin());
        for (int p = 0; p < t * t; ++p)
            for (int c = 0; c < C.hidden; ++c) out[(size_t)(1 + p) * C.hidden + c] = r[(size_t)c * t * t + p];
    }
    float* d = (float*)dev_alloc(out.size() * 4);
    HIP_CHECK(hipMemcpy(d, out.data(), out.size() * 4, hipMemcpyHostToDevice));
    clip_.pos_dev[tokens] = d;
    return d;
}

// ============================================================================ vision
// DSOCR_VIS_STREAMS=0 (A/B switch, read once): every vision pass of a batch on the engine stream
static bool vis_streams_on() {
    static const bool v = !(getenv("DSOCR_VIS_STREAMS") && atoi(getenv("DSOCR_VIS_STREAMS")) == 0);
    return v;
}

// SamBackbone::forward (sam.rs:210-289) + ClipVisionModel::forward (clip.rs:98-102) +
// build_clip_sam_tokens + ImageProjector::project (model/mod.rs:604-650, 392-444).
float* Engine::vision_pass(const float* imgs, int n, int Spx, const std::string& out) {
    const SamConfig& S = cfg_.sam;
    const ClipConfig& CC = cfg_.clip;
    const int C = S.dim, heads = S.heads, hd = C / heads;
    if (Spx % S.patch) throw std::runtime_error("EINVAL: image dimensions must be divisible by patch size");
    const int g = Spx / S.patch;
    if (g % 2 || (g / 2) % 2) throw std::runtime_error("EINVAL: spatial dims cannot be evenly downsampled by stride 2");
    const long rows = (long)n * g * g;
    hipStream_t st = stream_;
    // a sliced admission runs one stage per call (vis_stage_: 1 SAM, 2 CLIP / the OCR2 encoder's layers, 3 projector);
    // every call asks for the same workspaces by name and size, so a stage finds what the one before it left
    const bool s1 = vis_stage_ == 0 || vis_stage_ == 1, s2 = vis_stage_ == 0 || vis_stage_ == 2;
    const bool s3 = vis_stage_ == 0 || vis_stage_ == 3;
    const int g2 = g / 2, g4 = g / 4, c0 = S.out_ch[0], c1 = S.out_ch[1];
    const int Sq = g4 * g4;
    float* sam_out = wsf("v_samout", (size_t)n * Sq * c1);
    if (s1) {
    // patch embed
    float* cols = wsf("v_cols", (size_t)rows * 3 * S.patch * S.patch);
    launch_patch_im2col(imgs, n, Spx, Spx, S.patch, cols, st);
    float* x = wsf("v_x", (size_t)rows * C);
    linear(cols, (int)rows, 3 * S.patch * S.patch, sam_.patch, x, C);
    if (sam_.has_pos) launch_add_broadcast(x, sam_pos(g), (long)g * g, C, n, st);

    // window partition maps (sam.rs:926-980)
    const int W = S.window;
    const int gp = g + (W - g % W) % W, nw = gp / W;
    const long wrows = (long)n * nw * nw * W * W;
    auto wm = winmaps_.find({n, g});
    if (wm == winmaps_.end()) {  // built once per (images, grid): tok -> window slot and back
        const WindowMaps maps = window_maps(n, g, W);
        const std::vector<int>& tok2win = maps.tok2win;
        const std::vector<int>& win2tok = maps.win2tok;
        int *a = nullptr, *b2 = nullptr;
        HIP_CHECK(hipMalloc(&a, tok2win.size() * 4));
        HIP_CHECK(hipMalloc(&b2, win2tok.size() * 4));
        HIP_CHECK(hipMemcpy(a, tok2win.data(), tok2win.size() * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(b2, win2tok.data(), win2tok.size() * 4, hipMemcpyHostToDevice));
        wm = winmaps_.emplace(std::make_pair(n, g), std::make_pair(a, b2)).first;
    }
    int* d_tok2win = wm->second.first;
    int* d_win2tok = wm->second.second;
    const long maxrows = std::max(rows, wrows);
    float* xn = wsf("v_xn", (size_t)maxrows * C);
    float* qkv = wsf("v_qkv", (size_t)maxrows * 3 * C);
    float* ctx = wsf("v_ctx", (size_t)maxrows * C);
    const int hid = (int)(C * S.mlp_ratio);
    float* hbuf = wsf("v_h", (size_t)rows * hid);

    for (int bi = 0; bi < S.depth; ++bi) {
        SamBlock& blk = sam_.blocks[bi];
        const bool win = !blk.global;
        const int L = win ? W * W : g * g;
        const int nseq = win ? n * nw * nw : n;
        const long arows = (long)nseq * L;
        if (win) {
            HIP_CHECK(hipMemsetAsync(xn, 0, (size_t)wrows * C * 4, st));
            launch_layernorm(x, C, xn, C, d_tok2win, (int)rows, C, blk.n1.w, blk.n1.b, 1e-6f, st);
        } else {
            launch_layernorm(x, C, xn, C, nullptr, (int)rows, C, blk.n1.w, blk.n1.b, 1e-6f, st);
        }
        linear(xn, (int)arows, C, blk.qkv, qkv, 3 * C);
        AttnArgs a;
        a.q = {qkv, 3L * C, hd, nullptr};
        a.k = {qkv + C, 3L * C, hd, nullptr};
        a.v = {qkv + 2 * C, 3L * C, hd, nullptr};
        a.o = ctx;
        a.o_row_stride = C;
        a.o_head_stride = hd;
        a.n_seq = nseq;
        a.L = L;
        a.heads = heads;
        a.kv_heads = heads;
        a.hd = hd;
        a.scale = (float)(1.0 / std::sqrt((double)hd));
        if (blk.use_rel) {
            const int gg = win ? W : g;
            auto rel = win ? std::make_pair<float*, float*>(nullptr, nullptr) : sam_rel(blk, g);
            if (win) rel = sam_rel(blk, W);
            float* rb = wsf("v_relbias", (size_t)nseq * heads * L * (2 * gg));
            launch_sam_relbias(qkv, 3L * C, nseq, gg, gg, heads, hd, rel.first, rel.second, rb, st);
            a.relbias = rb;
            a.rel_h = gg;
            a.rel_w = gg;
        }
        flops_acc_ += 4.0 * nseq * (double)L * L * hd * heads;
        launch_attention(a, st);
        // proj + residual (window_unpartition via row scatter)
        linear(ctx, (int)arows, C, blk.proj, x, C, 0, 1, win ? d_win2tok : nullptr);
        launch_layernorm(x, C, xn, C, nullptr, (int)rows, C, blk.n2.w, blk.n2.b, 1e-6f, st);
        linear(xn, (int)rows, C, blk.fc1, hbuf, hid, ACT_GELU_ERF);
        linear(hbuf, (int)rows, hid, blk.fc2, x, C, 0, 1);
    }
    // neck (sam.rs:503-520) in NHWC
    const int NC = S.neck;
    float* y = wsf("v_neck", (size_t)rows * NC);
    linear(x, (int)rows, C, sam_.neck0, y, NC);
    launch_layernorm(y, NC, y, NC, nullptr, (int)rows, NC, sam_.neck1.w, sam_.neck1.b, 1e-6f, st);
    float* ncols = wsf("v_ncols", (size_t)rows * 9 * NC);
    launch_conv_im2col_nhwc(y, n, g, g, NC, 3, 3, 1, 1, ncols, st);
    linear(ncols, (int)rows, 9 * NC, sam_.neck2, y, NC);
    launch_layernorm(y, NC, y, NC, nullptr, (int)rows, NC, sam_.neck3.w, sam_.neck3.b, 1e-6f, st);
    // downsample (sam.rs:550-575)
    launch_conv_im2col_nhwc(y, n, g, g, NC, 3, 3, 2, 1, ncols, st);
    float* z = wsf("v_net2", (size_t)n * g2 * g2 * c0);
    linear(ncols, n * g2 * g2, 9 * NC, sam_.net2, z, c0);
    float* ncols2 = wsf("v_ncols2", (size_t)n * g4 * g4 * 9 * c0);
    launch_conv_im2col_nhwc(z, n, g2, g2, c0, 3, 3, 2, 1, ncols2, st);
    linear(ncols2, n * Sq, 9 * c0, sam_.net3, sam_out, c1);
    }  // s1
    // Ocr2: the NHWC rows are already the reference's flatten(2,3).transpose(1,2) token rows (qwen2.rs:157-161)
    if (cfg_.variant == VARIANT_OCR2) return encoder_pass(sam_out, n, Sq, out);

    // CLIP (clip.rs:165-309) on SAM features
    const int T = Sq + 1, CH = CC.hidden, chd = CH / CC.heads;
    const long crow = (long)n * T;
    float* cx = wsf("c_x", (size_t)crow * CH);
    if (s2) {
    launch_clip_embed(sam_out, clip_.cls, clip_pos(T), n, Sq, CH, cx, st);
    launch_layernorm(cx, CH, cx, CH, nullptr, (int)crow, CH, clip_.pre.w, clip_.pre.b, 1e-5f, st);
    }
    float* cxn = wsf("c_xn", (size_t)crow * CH);
    float* cqkv = wsf("c_qkv", (size_t)crow * 3 * CH);
    float* cctx = wsf("c_ctx", (size_t)crow * CH);
    float* ch = wsf("c_h", (size_t)crow * CC.ffn);
    for (int l = 0; s2 && l < CC.layers; ++l) {
        ClipLayer& cl = clip_.layers[l];
        launch_layernorm(cx, CH, cxn, CH, nullptr, (int)crow, CH, cl.ln1.w, cl.ln1.b, 1e-5f, st);
        linear(cxn, (int)crow, CH, cl.qkv, cqkv, 3 * CH);
        AttnArgs a;
        a.q = {cqkv, 3L * CH, chd, nullptr};
        a.k = {cqkv + CH, 3L * CH, chd, nullptr};
        a.v = {cqkv + 2 * CH, 3L * CH, chd, nullptr};
        a.o = cctx;
        a.o_row_stride = CH;
        a.o_head_stride = chd;
        a.n_seq = n;
        a.L = T;
        a.heads = CC.heads;
        a.kv_heads = CC.heads;
        a.hd = chd;
        a.scale = (float)(1.0 / std::sqrt((double)chd));
        flops_acc_ += 4.0 * n * (double)T * T * chd * CC.heads;
        launch_attention(a, st);
        linear(cctx, (int)crow, CH, cl.out, cx, CH, 0, 1);
        launch_layernorm(cx, CH, cxn, CH, nullptr, (int)crow, CH, cl.ln2.w, cl.ln2.b, 1e-5f, st);
        linear(cxn, (int)crow, CH, cl.fc1, ch, CC.ffn, ACT_QUICK_GELU);
        linear(ch, (int)crow, CC.ffn, cl.fc2, cx, CH, 0, 1);
    }
    // concat + projector
    float* pre = wsf("p_pre", (size_t)n * Sq * (CH + c1));
    float* post = wsf(out, (size_t)n * Sq * cfg_.proj_out);
    if (s3) {
        launch_concat_clip_sam(cx, sam_out, n, Sq, CH, c1, pre, st);
        linear(pre, n * Sq, CH + c1, proj_, post, cfg_.proj_out);
    }
    return post;
}

// Qwen2DecoderAsEncoder::forward_tokens (qwen2.rs:166-220) + Qwen2Projector (407-444) on n views of P SAM tokens:
// [image tokens | queries] at positions 0 .. 2P-1, the decoder blocks (block.rs) under the hybrid mask, the final
// RMSNorm, and the projector on the query half only (RMSNorm and the linear are row-wise, so taking the query rows
// first gives the same values as the reference's narrow() after the norm)
float* Engine::encoder_pass(const float* sam_out, int n, int P, const std::string& out) {
    const Qwen2EncConfig& Q = cfg_.enc;
    const float* query = P == Q.query_768 ? enc_.query_768 : P == Q.query_1024 ? enc_.query_1024 : nullptr;
    if (!query)
        throw std::runtime_error("EINVAL: unsupported Qwen2 query length " + std::to_string(P) + " (expected " +
                                 std::to_string(Q.query_768) + " or " + std::to_string(Q.query_1024) + ")");
    hipStream_t st = stream_;
    const int D = Q.dim, hd = Q.head_dim, L = 2 * P, QW = Q.heads * hd, KW = Q.kv_heads * hd, W3 = QW + 2 * KW;
    const long rows = (long)n * L;
    float* x = wsf("q2_x", (size_t)rows * D);
    float* xn = wsf("q2_xn", (size_t)rows * D);
    float* qkv = wsf("q2_qkv", (size_t)rows * W3);
    float* ctx = wsf("q2_ctx", (size_t)rows * QW);
    float* gu = wsf("q2_gu", (size_t)rows * 2 * Q.inter);
    float* hbuf = wsf("q2_h", (size_t)rows * Q.inter);
    const bool s2 = vis_stage_ == 0 || vis_stage_ == 2, s3 = vis_stage_ == 0 || vis_stage_ == 3;
    if (s2) launch_ocr2_build_seq(sam_out, query, n, P, D, x, st);
    for (const EncLayer& e : enc_.layers) {
        if (!s2) break;
        launch_rmsnorm(x, D, xn, D, (int)rows, D, e.in_norm.w, Q.rms_eps, st);
        linear(xn, (int)rows, D, e.qkv, qkv, W3);
        launch_ocr2_rope(qkv, W3, rows, L, Q.heads + Q.kv_heads, hd, enc_.cos, enc_.sin, st);
        AttnPrefixArgs a;
        a.q = qkv; a.k = qkv + QW; a.v = qkv + QW + KW; a.o = ctx;
        a.ldq = a.ldk = a.ldv = W3; a.ldo = QW;
        a.n_seq = n; a.L = L; a.prefix = P; a.heads = Q.heads; a.kv_heads = Q.kv_heads; a.hd = hd;
        a.scale = (float)(1.0 / std::sqrt((double)hd));
        // visible (row, key) pairs per head and sequence: P^2 among the image rows, P^2 + P (P + 1) / 2 for the queries
        flops_acc_ += 4.0 * n * Q.heads * hd * (2.0 * P * P + 0.5 * P * (P + 1.0));
        launch_attention_prefix(a, st);
        linear(ctx, (int)rows, QW, e.o, x, D, 0, 1);
        launch_rmsnorm(x, D, xn, D, (int)rows, D, e.post_norm.w, Q.rms_eps, st);
        linear(xn, (int)rows, D, e.gu, gu, 2 * Q.inter);
        launch_silu_mul(gu, 2 * Q.inter, Q.inter, (int)rows, hbuf, Q.inter, st);
        linear(hbuf, (int)rows, Q.inter, e.down, x, D, 0, 1);
    }
    float* qx = wsf("q2_q", (size_t)n * P * D);
    float* post = wsf(out, (size_t)n * P * cfg_.proj_out);
    if (s3) {
        launch_ocr2_take_queries(x, n, P, D, qx, st);
        launch_rmsnorm(qx, D, qx, D, n * P, D, enc_.norm, Q.rms_eps, st);
        linear(qx, n * P, D, proj_, post, cfg_.proj_out);
    }
    return post;
}

void Engine::check_page_variant(const PagePixels& pg) const {
    if (pg.variant != cfg_.variant)
        throw std::runtime_error(std::string("EINVAL: page was prepared for ") +
                                 (pg.variant == VARIANT_OCR2 ? "DeepSeek-OCR-2" : "DeepSeek-OCR") + " but the engine runs " +
                                 (cfg_.variant == VARIANT_OCR2 ? "DeepSeek-OCR-2" : "DeepSeek-OCR") +
                                 " (image slot layout mismatch)");
}

// row kinds of launch_assemble_rows: token embedding, caller-supplied image row, vision row, the two markers
enum RowKind : int { ROW_TOKEN = 0, ROW_HOST = 1, ROW_VISION = 2, ROW_NEWLINE = 3, ROW_SEPARATOR = 4 };

// The <image> slots of a page in prompt order, as (kind, index into the page's [local | global] vision rows):
// format_local_tokens (model/mod.rs:677-709) walks the tile grid row by row with a newline after each, then
// format_global_tokens (656-675) the global view likewise, then the separator
static std::vector<std::pair<int, long>> image_row_order(const PagePixels& pg) {
    std::vector<std::pair<int, long>> seq;
    const int ls = pg.tile / 64, gs = pg.gsize / 64;
    const long n_local = pg.n_tiles > 0 ? (long)pg.n_tiles * ls * ls : 0;
    if (pg.variant == VARIANT_OCR2) {
        // Qwen2VisionEncoder::encode (qwen2.rs:337-372): the tiles' tokens tile-major, the global view's, the
        // separator; no newline rows and no 2-D re-tiling, so the order is the vision rows' own
        for (long i = 0; i < n_local + (long)gs * gs; ++i) seq.push_back({ROW_VISION, i});
        seq.push_back({ROW_SEPARATOR, 0});
        return seq;
    }
    for (int R = 0; n_local && R < pg.crop_h * ls; ++R) {
        for (int Cc = 0; Cc < pg.crop_w * ls; ++Cc) {
            const int crop = (R / ls) * pg.crop_w + (Cc / ls);
            seq.push_back({ROW_VISION, ((long)crop * ls + R % ls) * ls + Cc % ls});
        }
        seq.push_back({ROW_NEWLINE, 0});
    }
    for (int R = 0; R < gs; ++R) {
        for (int Cc = 0; Cc < gs; ++Cc) seq.push_back({ROW_VISION, n_local + (long)R * gs + Cc});
        seq.push_back({ROW_NEWLINE, 0});
    }
    seq.push_back({ROW_SEPARATOR, 0});
    return seq;
}

std::vector<std::vector<float>> Engine::image_embeddings(const std::vector<const PagePixels*>& pages) {
    std::vector<std::vector<float>> result;
    const int H = cfg_.proj_out;
    for (const PagePixels* p : pages) {
        check_page_variant(*p);
        // one page at a time keeps this helper simple; generate() batches pages.
        float* gimg = p->global_dev && p->dev_ordinal == device_ ? p->global_dev : upload("e_gimg", p->global_chw);
        float* gpost = vision_pass(gimg, 1, p->gsize, "e_gpost");
        const int gs = p->gsize / 64;
        std::vector<float> gh((size_t)gs * gs * H);
        HIP_CHECK(hipMemcpyAsync(gh.data(), gpost, gh.size() * 4, hipMemcpyDeviceToHost, stream_));
        std::vector<float> lh;
        int ls = 0;
        if (p->n_tiles > 0) {
            float* timg = p->tiles_dev && p->dev_ordinal == device_ ? p->tiles_dev : upload("e_timg", p->tiles_chw);
            float* lpost = vision_pass(timg, p->n_tiles, p->tile, "e_lpost");
            ls = p->tile / 64;
            lh.resize((size_t)p->n_tiles * ls * ls * H);
            HIP_CHECK(hipMemcpyAsync(lh.data(), lpost, lh.size() * 4, hipMemcpyDeviceToHost, stream_));
        }
        HIP_CHECK(hipStreamSynchronize(stream_));
        std::vector<float> nl(H), sp(H);
        HIP_CHECK(hipMemcpy(nl.data(), newline_, H * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(sp.data(), separator_, H * 4, hipMemcpyDeviceToHost));
        std::vector<float> rows;
        const size_t n_local = lh.size() / H;
        for (const auto& [kind, i] : image_row_order(*p)) {
            const float* r = kind == ROW_NEWLINE ? nl.data() : kind == ROW_SEPARATOR ? sp.data()
                             : (size_t)i < n_local ? &lh[i * H] : &gh[(i - n_local) * H];
            rows.insert(rows.end(), r, r + H);
        }
        result.push_back(std::move(rows));
    }
    return result;
}

// ============================================================================ decoder
void Engine::layer_forward_prefill(int l, int T, int B, const int* row_page, const int* row_pos, const long* q_off,
                                   const long* kv_off, const long* o_off, const int* seq_len, int max_len, int Lmax,
                                   const int* past, int max_total, bool chunk_attn) {
    const LangConfig& L = cfg_.lang;
    DecLayer& d = layers_[l];
    hipStream_t st = stream_;
    const int H = L.hidden, hd = L.head_dim, KVH = L.kv_heads * hd, QKVN = d.qkv.N;
    float* X = wsf("d_x", (size_t)T * H);
    float* XN = wsf("d_xn", (size_t)T * H);
    float* QKV = wsf("d_qkv", (size_t)T * QKVN);
    float* CTX = wsf("d_ctx", (size_t)T * H);
    // (a session prefills one page into its own slot of the session cache: kv_page0_)
    float* kc = kc_ + (long)l * layer_kv(B) + (long)kv_page0_ * page_stride_;
    float* vc = vc_ + (long)l * layer_kv(B) + (long)kv_page0_ * page_stride_;

    launch_rmsnorm(X, H, XN, H, T, H, d.in_norm.w, L.rms_eps, st);
    linear(XN, T, H, d.qkv, QKV, QKVN);
    RopeKvArgs r;
    r.qkv = QKV; r.ld = QKVN; r.rows = T; r.row_page = row_page; r.row_pos = row_pos;
    r.heads = L.heads; r.kv_heads = L.kv_heads; r.hd = hd; r.rope_dim = L.rope_dim; r.use_mla = L.use_mla;
    r.cos = rope_cos_; r.sin = rope_sin_; r.kc = kc; r.vc = vc; r.page_stride = page_stride_; r.head_stride = head_stride_;
    launch_rope_kv(r, st);
    if (past) {
        // behind a cached past (a page prefix entry): seq_len counts the new rows, row_pos starts at the past
        AttnPastArgs a;
        a.q = {QKV, QKVN, hd, q_off};
        a.k = {kc, hd, head_stride_, kv_off};
        a.v = {vc, hd, head_stride_, kv_off};
        a.o = CTX; a.o_row_stride = H; a.o_head_stride = hd; a.o_seq_off = o_off;
        a.n_seq = B; a.past = past; a.n_q = seq_len; a.max_q = max_len; a.max_total = max_total;
        a.heads = L.heads; a.kv_heads = L.kv_heads; a.hd = hd;
        a.scale = (float)(1.0 / std::sqrt((double)hd));
        flops_acc_ += 4.0 * (double)T * max_total * hd * L.heads;  // (upper bound: every new row against every key)
        if (chunk_attn) {  // a chunk of a sliced admission: query tiles, one launch, no record workspace
            launch_attention_chunk(a, st);
            ++chunk_attn_launches_;
        } else {
            a.part_floats = attention_past_part_floats(B, L.heads, max_len, max_total, hd);
            a.part = wsf("d_attn_past", a.part_floats);
            launch_attention_past(a, st);
        }
    } else {
        AttnArgs a;
        a.q = {QKV, QKVN, hd, q_off};
        a.k = {kc, hd, head_stride_, kv_off};
        a.v = {vc, hd, head_stride_, kv_off};
        a.o = CTX; a.o_row_stride = H; a.o_head_stride = hd; a.o_seq_off = o_off;
        a.n_seq = B; a.L = max_len; a.seq_len = seq_len;
        a.heads = L.heads; a.kv_heads = L.kv_heads; a.hd = hd;
        a.scale = (float)(1.0 / std::sqrt((double)hd));
        a.causal = 1;
        // the key-piece workspace grows as L^2 (n_seq * heads * sum over query blocks of their pieces * 128 * (hd + 2)
        // floats: 89 MB at 8 x 706 tokens, 2.8 GB at 8 x 4096); above 512 MB the prefill runs the one-block-per-
        // query-block kernel, which needs none
        constexpr size_t kPartCapFloats = (size_t)128 << 20;
        const size_t part_floats = attention_causal_part_floats(B, L.heads, max_len, hd);
        if (part_floats <= kPartCapFloats) {
            a.part_floats = part_floats;
            a.part = wsf("d_attn_part", a.part_floats);
        }
        for (int q = 0; q < B && q < (int)prefill_lens_.size(); ++q)
            flops_acc_ += 2.0 * (double)prefill_lens_[q] * (prefill_lens_[q] + 1) * hd * L.heads;
        launch_attention(a, st);
    }
    (void)Lmax;
    (void)KVH;
    linear(CTX, T, H, d.o, X, H, 0, 1);
    launch_rmsnorm(X, H, XN, H, T, H, d.post_norm.w, L.rms_eps, st);
    if (!d.moe) {
        const int I = L.inter;
        float* G = wsf("d_g", (size_t)T * 2 * I);
        float* HH = wsf("d_hh", (size_t)T * I);
        linear(XN, T, H, d.gu, G, 2 * I);
        launch_silu_mul(G, 2 * I, I, T, HH, I, st);
        linear(HH, T, I, d.down, X, H, 0, 1);
        return;
    }
    // MoE (run_moe, block.rs:1215-1395) with device-side routing
    const int E = L.n_routed, K = L.topk, I = L.moe_inter, TK = T * K;
    float* LOG = wsf("d_log", (size_t)T * E);
    int* IDS = wsi("d_ids", TK);
    float* WTS = wsf("d_wts", TK);
    int* EOFF = wsi("d_eoff", E + 1);
    int* AROW = wsi("d_arow", TK);
    int* APOS = wsi("d_apos", TK);
    linear(XN, T, H, d.router, LOG, E);
    launch_router_topk(LOG, T, E, K, L.scoring == "softmax", L.norm_topk, L.routed_scaling, IDS, WTS, st);
    launch_moe_group(IDS, T, K, E, EOFF, AROW, APOS, nullptr, st);
    float* G = wsf("d_eg", (size_t)TK * 2 * I);
    float* HH = wsf("d_ehh", (size_t)TK * I);
    float* Y = wsf("d_ey", (size_t)TK * H);
    GemmArgs g1;
    g1.M = TK; g1.N = 2 * I; g1.K = H; g1.A = XN; g1.lda = H; g1.a_rows = AROW; g1.W = d.e_gu; g1.ldw = H;
    g1.wdtype = d.e_wdt; g1.w_group_stride = (long)2 * I * H; g1.C = G; g1.ldc = 2 * I;
    g1.group_off = EOFF; g1.groups = E; g1.max_group_rows = T;
    launch_gemm(g1, st);
    flops_acc_ += 2.0 * TK * (2.0 * I) * H + 2.0 * TK * (double)H * I;  // routed gate/up + down (next launch)
    launch_silu_mul(G, 2 * I, I, TK, HH, I, st);
    GemmArgs g2;
    g2.M = TK; g2.N = H; g2.K = I; g2.A = HH; g2.lda = I; g2.W = d.e_d; g2.ldw = I; g2.wdtype = d.e_wdt;
    g2.w_group_stride = (long)H * I; g2.C = Y; g2.ldc = H; g2.group_off = EOFF; g2.groups = E; g2.max_group_rows = T;
    launch_gemm(g2, st);
    float* YS = nullptr;
    if (d.has_shared) {
        const int Is = d.s_d.K;
        float* GS = wsf("d_sg", (size_t)T * 2 * Is);
        float* HS = wsf("d_shh", (size_t)T * Is);
        YS = wsf("d_sy", (size_t)T * H);
        linear(XN, T, H, d.s_gu, GS, 2 * Is);
        launch_silu_mul(GS, 2 * Is, Is, T, HS, Is, st);
        linear(HS, T, Is, d.s_d, YS, H);
    }
    launch_moe_combine(Y, APOS, WTS, YS, T, K, H, X, 1, st);
}

// DSOCR_ROUTER_SWZ=0 (A/B switch, read at every MoE argument build, i.e. per capture): the routing inside gate/up
// reads the row-major router rows instead of their fragment-ordered copy
static bool router_swz_off() {
    const char* e = getenv("DSOCR_ROUTER_SWZ");
    return e && atoi(e) == 0;
}
// DSOCR_MM_SWZ=0 (A/B switch, per capture): 3..8 pages' q/k/v, o_proj and dense gate|up read row-major weights
static bool mm_swz_off() {
    const char* e = getenv("DSOCR_MM_SWZ");
    return e && atoi(e) == 0;
}

// Decode MoE arguments of layer l for B pages (shared by decode_step and profile_decode): the
// layer's weights and the named workspaces; launch_moe_decode (decode_moe.hip) picks the kernels.
MoeDecodeArgs Engine::moe_args(int l, int B, float* X) {
    const LangConfig& L = cfg_.lang;
    DecLayer& d = layers_[l];
    const int H = L.hidden, E = L.n_routed, K = L.topk, I = L.moe_inter, TK = B * K;
    MoeDecodeArgs a;
    a.T = B; a.H = H; a.E = E; a.topk = K; a.I = I;
    a.x = X; a.norm_w = d.post_norm.w; a.eps = L.rms_eps; a.out = X;
    a.router = d.router.W; a.router_wdt = d.router.wdt; a.router_bias = d.router.b;
    a.Wgu = d.e_gu; a.Wd = d.e_d; a.wdtype = d.e_wdt;
    if (d.has_shared) {
        if (d.s_gu.wdt != d.e_wdt) throw std::runtime_error("EINTERNAL: shared/routed expert dtype mismatch");
        a.Is = d.s_d.K; a.sWgu = d.s_gu.W; a.sWd = d.s_d.W; a.hs = wsf("s_shh", (size_t)B * a.Is);
    }
    a.softmax_scoring = L.scoring == "softmax"; a.norm_topk = L.norm_topk; a.scaling = L.routed_scaling;
    a.xn = wsf("s_xn", (size_t)B * H);
    a.xn_router = wsf("s_xn_router", (size_t)B * H);
    a.logits = wsf("s_log", (size_t)B * E);
    a.ids = wsi("s_ids", TK); a.wts = wsf("s_wts", TK);
    a.h = wsf("s_ehh", (size_t)TK * I);
    a.grp = wsi("s_grp", moe_grp_ints(E, B, K));
    a.route_cnt = rows_.route_cnt;
    if (B >= 3 && B <= 8) {  // matrix-core grouped kernels: down partials + tickets
        a.dn_part = wsf("s_dnpart", moe_down_mm_part_floats(E, B, K, I, a.Is, H));
        a.dn_tick = rows_.dn_tick;  // one ticket per 64-row tile
    }
    if (B <= 8 && d.packed) {  // the packed decode kernels (decode_q.hip)
        a.qWgu = d.q_gu; a.qWd = d.q_d; a.qsWgu = d.q_sgu; a.qsWd = d.q_sd;
    }
    if (B <= 8 && d.e_gu_swz && (!d.has_shared || d.s_gu_swz)) {  // fragment-ordered experts
        a.Wgu_swz = d.e_gu_swz; a.Wd_swz = d.e_d_swz; a.sWgu_swz = d.s_gu_swz; a.sWd_swz = d.s_d_swz;
        if (!router_swz_off()) a.router_swz = d.router_swz;
    }
    if (B > 8) {
        a.eoff = wsi("s_eoff", E + 1); a.arow = wsi("s_arow", TK); a.apos = wsi("s_apos", TK);
        a.aw = wsf("s_aw", TK); a.active = wsi("s_active", E); a.n_active = wsi("s_nact", 1);
    }
    return a;
}

// Decode attention arguments of layer l (shared by decode_step and profile_decode, which points q/k/v, the
// position and the output at scratch rows): RoPE + K/V append + flash-decoding on the named workspaces
// The hand-off buffers (the sentinel-filled q/k/v row and the flash-decoding records) exist in two copies,
// rows_.qkv[c] / rows_.part[c] (workspaces "s_qkv" / "s_part" and "s_qkv1" / "s_part1").  Every launch but the fused one-page one uses copy 0 and leaves
// it sentinel-filled itself.  With the deferred refill (att_refill_defer) layer l of the fused one-page path
// uses copy l & 1, leaves the words it read as they are and cleans the copy of layer l - 1; the last layer of
// the step refills its own.  Invariant: at every step boundary every word of both copies holds the sentinel.
DecAttn2Args Engine::attn_args(int l, int B, int Lmax, int copy) {
    const LangConfig& L = cfg_.lang;
    const int hd = L.head_dim, QKVN = layers_[l].qkv.N;
    const long layer_kv = this->layer_kv(B);
    DecAttn2Args da;
    da.qkv = rows_.qkv[copy]; da.ld = QKVN; da.kv_pos = rows_.kv_pos; da.B = B;
    da.heads = L.heads; da.kv_heads = L.kv_heads; da.hd = hd; da.rope_dim = L.rope_dim; da.use_mla = L.use_mla;
    da.max_len = Lmax; da.cos = rope_cos_; da.sin = rope_sin_;
    da.kc = kc_ + (long)l * layer_kv; da.vc = vc_ + (long)l * layer_kv;
    da.page_stride = page_stride_; da.head_stride = head_stride_;
    da.scale = (float)(1.0 / std::sqrt((double)hd));
    da.part = rows_.part[copy];
    da.o = wsf("s_ctx", (size_t)B * L.hidden); da.o_ld = L.hidden;
    da.counters = rows_.attn_cnt;
    da.err = rows_.err;
    return da;
}

// DSOCR_NO_GRAPH=1 (read per generate and per profile section): the decode step's kernels launched eagerly
// instead of replayed from a hipGraph (rocprofv3 kernel tracing of graph replays is unreliable on this stack;
// kernel durations are unchanged)
static bool graphs_on() {
    const char* e = getenv("DSOCR_NO_GRAPH");
    return !(e && atoi(e) != 0);
}

bool Engine::persist_ok(int B, int Lmax) {
    // opt-in (DSOCR_PERSIST=1, read per generate): measured slower than the per-layer launch chain on MI355X
    // (43.5 vs 33.5 us per layer), kept as the A/B of the persistent-layer design
    const char* e = getenv("DSOCR_PERSIST");
    if (!e || atoi(e) == 0) return false;
    const LangConfig& L = cfg_.lang;
    for (const DecLayer& d : layers_)
        if (d.packed) return false;  // the persistent launch streams the fp16 experts only
    if (B != 1 || L.use_mla || L.rope_dim != L.head_dim || L.v_head_dim != L.head_dim || L.n_shared <= 0 ||
        L.topk_method != "greedy" || L.hidden_act != "silu")
        return false;
    if (!dec_persist_shape_ok(L.hidden, L.heads, L.kv_heads, L.head_dim, L.n_routed, L.topk, L.moe_inter,
                              L.n_shared * L.moe_inter, L.inter, Lmax))
        return false;
    for (const DecLayer& d : layers_) {
        if (d.qkv.wdt != WDT_F16 || d.qkv.b || d.o.wdt != WDT_F16 || d.o.b) return false;
        if (d.moe) {
            if (!d.router.W || d.router.wdt != WDT_F16 || d.e_wdt != WDT_F16 || !d.has_shared || d.s_gu.wdt != WDT_F16 ||
                d.s_d.wdt != WDT_F16 || d.s_gu.b || d.s_d.b)
                return false;
        } else if (!d.gu.W || d.gu.wdt != WDT_F16 || d.down.wdt != WDT_F16) {
            return false;
        }
    }
    return dec_persist_resident() != 0;
}

// the persistent decode's weight table: every down projection transposed to [inter][H] (split-K rows), the
// per-layer pointer table on the device, the granule buffer (made once, outside any capture)
void Engine::ensure_persist() {
    if (persist_lw_ || capturing_) return;
    const LangConfig& L = cfg_.lang;
    const int H = L.hidden, E = L.n_routed, I = L.moe_inter;
    std::vector<PersistLayerW> tab(layers_.size());
    for (size_t l = 0; l < layers_.size(); ++l) {
        DecLayer& d = layers_[l];
        PersistLayerW& w = tab[l];
        w.qkv = (const uint16_t*)d.qkv.W;
        w.o = (const uint16_t*)d.o.W;
        w.in_w = d.in_norm.w;
        w.post_w = d.post_norm.w;
        w.moe = d.moe ? 1 : 0;
        if (d.moe) {
            if (!d.e_dT) {
                d.e_dT = dev_alloc((size_t)E * I * H * 2);
                for (int e = 0; e < E; ++e)
                    launch_transpose16((const uint16_t*)d.e_d + (size_t)e * H * I, (uint16_t*)d.e_dT + (size_t)e * I * H, H, I,
                                       stream_);
            }
            const int Is = d.s_d.K;
            if (!d.s_dT) {
                d.s_dT = dev_alloc((size_t)Is * H * 2);
                launch_transpose16(d.s_d.W, d.s_dT, H, Is, stream_);
            }
            w.router = (const uint16_t*)d.router.W;
            w.router_bias = d.router.b;
            w.e_gu = (const uint16_t*)d.e_gu;
            w.e_dT = (const uint16_t*)d.e_dT;
            w.s_gu = (const uint16_t*)d.s_gu.W;
            w.s_dT = (const uint16_t*)d.s_dT;
            w.inter = Is;
        } else {
            if (!d.s_dT) {
                d.s_dT = dev_alloc((size_t)L.inter * H * 2);
                launch_transpose16(d.down.W, d.s_dT, H, L.inter, stream_);
            }
            w.s_gu = (const uint16_t*)d.gu.W;
            w.s_dT = (const uint16_t*)d.s_dT;
            w.inter = L.inter;
        }
    }
    PersistLayerW* dtab = (PersistLayerW*)dev_alloc(tab.size() * sizeof(PersistLayerW));
    HIP_CHECK(hipMemcpyAsync(dtab, tab.data(), tab.size() * sizeof(PersistLayerW), hipMemcpyHostToDevice, stream_));
    persist_g_ = (unsigned long long*)dev_alloc(dec_persist_granules(L.layers) * 8);
    HIP_CHECK(hipStreamSynchronize(stream_));
    persist_lw_ = dtab;
}

// the dense MLP's matrix-core form at 3..8 pages (decode_mm.hip): q/k/v-sized K for gate|up, K % 64 for down
bool Engine::dense_mm_ok(const DecLayer& d, int B) const {
    const LangConfig& L = cfg_.lang;
    DecGemvArgs g1;
    g1.M = B; g1.N = 2 * L.inter; g1.K = L.hidden; g1.ldw = L.hidden;
    DecGemvArgs g2;
    g2.M = B; g2.N = L.hidden; g2.K = L.inter; g2.ldw = L.inter; g2.ldx = L.inter;
    return d.gu.W && d.down.W && dec_mm_ok(g1) && dec_mm_splitk_ok(g2);
}

void Engine::decode_step(int B, int Lmax) {
    // One token for each of B pages: 8 launches per layer (decode_common.hpp).  For B <= 2 the
    // RMSNorms are fused into the consuming GEMV / expert kernels (x normalised on the fly).
    const LangConfig& L = cfg_.lang;
    hipStream_t st = stream_;
    const int H = L.hidden, hd = L.head_dim;
    const bool fuse_norm = B <= 2;
    if (B > rows_.S || Lmax != rows_.Lcap) throw std::runtime_error("EINTERNAL: decode step outside the reserved decode rows");
    float* X = rows_.x;
    float* XN = wsf("s_xn", (size_t)B * H);
    int* kv_pos = rows_.kv_pos;
    float* CTX = wsf("s_ctx", (size_t)B * H);
    if (L.heads % L.kv_heads) throw std::runtime_error("EINVAL: num_attention_heads must be a multiple of num_key_value_heads");
    int* err = rows_.err;
    if (B == 1 && persist_active_ && !step_skip_ && !span_rec_) {
        // every layer of the step in one persistent launch (decode_persist.hip)
        DecPersistArgs pa;
        pa.layers = L.layers; pa.lw = persist_lw_; pa.x = X; pa.kv_pos = kv_pos;
        pa.cos = rope_cos_; pa.sin = rope_sin_; pa.kc = kc_; pa.vc = vc_;
        pa.layer_kv = (long)B * page_stride_; pa.head_stride = head_stride_;
        pa.scale = (float)(1.0 / std::sqrt((double)hd)); pa.eps = L.rms_eps;
        pa.softmax_scoring = L.scoring == "softmax"; pa.norm_topk = L.norm_topk; pa.scaling = L.routed_scaling;
        pa.g = persist_g_; pa.err = err;
        const bool stamp = persist_stamp_mode_ && !persist_ev_.empty() && persist_stamps_;
        if (stamp) { pa.stamps = persist_stamps_; pa.stamp_pos0 = persist_stamp_pos0_; pa.stamp_cap = persist_stamp_cap_; }
        // stamped: the launch's own dispatch begin / end (hipExtLaunchKernelGGL events: what rocprofv3's kernel trace
        // reports); the timed generate runs its steps eagerly (events on a dispatch packet cannot be captured)
        ScopedSet pe(prof_events(), stamp ? ProfEvents{persist_ev_[0], persist_ev_[1]} : ProfEvents());
        launch_dec_persist(pa, st);
        return;
    }
    // launch spans (set_spans): HIP events on the stream around the launch (dispatch-level duration,
    // what rocprofv3's kernel trace reports) + the in-kernel wave span folded right after it
    auto stamped = [&](int kind, int l, const std::function<void()>& launch, const int* ids, int n_ids) {
        if (!span_rec_ || chain_active_) {  // (chain spans: the launch carries its own slot region)
            launch();
            return;
        }
        const HipEvent* ev = &span_ev_[((size_t)kind * L.layers + l) * 2];
        const bool events = (span_mode_ & SPAN_EVENTS) != 0, waves = (span_mode_ & SPAN_WAVES) != 0;
        if (events) HIP_CHECK(hipEventRecord(ev[0], st));
        launch();
        if (events) HIP_CHECK(hipEventRecord(ev[1], st));
        // the fold (wave span + the launch's distinct experts): after every launch with wave spans only; an
        // events-only generate runs no extra kernel, so its step is the production chain plus the event
        // markers (bench.py prices its launches with the expert counts of a wave-span generate of the same batch)
        if (waves) launch_span_reduce(span_slots_, span_rec(kind, l), span_step_, span_cap_, ids, n_ids, st);
    };
    // the q/k/v projection, its RoPE epilogue (one page) and the attention of layer l on hand-off copy `copy`
    const bool one_page = B == 1 && !L.use_mla && L.rope_dim == hd;
    auto qkv_args = [&](int l, int copy, DecGemvArgs& g, DecRopeEpi& re, DecAttn2Args& da) {
        const DecLayer& d = layers_[l];
        const int QKVN = d.qkv.N;
        da = attn_args(l, B, Lmax, copy);
        da.kv_delay = att_kv_delay();
        da.span = chain_active_ ? chain_slots(l, SPAN_ATTN) : ((span_rec_ && (span_mode_ & SPAN_WAVES)) ? span_slots_ : nullptr);
        g = DecGemvArgs();
        g.M = B; g.N = QKVN; g.K = H; g.W = d.qkv.W; g.ldw = H; g.wdtype = d.qkv.wdt; g.bias = d.qkv.b;
        g.y = const_cast<float*>(da.qkv); g.ldy = QKVN; g.x = X; g.ldx = H; g.norm_w = d.in_norm.w; g.eps = L.rms_eps;
        re = DecRopeEpi();
        if (one_page) {
            re.kv_pos = kv_pos; re.cos = rope_cos_; re.sin = rope_sin_; re.hd = hd;
            re.rot_rows = (L.heads + L.kv_heads) * hd;
            da.prerot = 1;
        }
    };
    // deferred refill (att_refill_defer, attn_args): the layers that take the fused one-page launch, known
    // before the loop - a layer hands its refill on only to a fused launch right behind it in the same step,
    // and cleans the other copy only behind a launch that handed its refill on
    std::vector<char> defer_l(L.layers, 0);
    if (one_page && qkv_attn_fused() && att_refill_defer() && !(step_skip_ & SKIP_ATTN))
        for (int l = 0; l < L.layers; ++l) {
            DecGemvArgs g; DecRopeEpi re; DecAttn2Args da;
            qkv_args(l, l & 1, g, re, da);
            defer_l[l] = dec_qkv_attn_ok(g, re, da);
        }
    for (int l = 0; l < L.layers; ++l) {
        DecLayer& d = layers_[l];
        const int QKVN = d.qkv.N;
        // attention: [norm] qkv -> rope + append + flash-decoding -> o_proj + residual
        // q/k/v projection with the input RMSNorm fused; one page: RoPE in the projection's epilogue, so the
        // attention reads q / k already rotated (B <= 2: the row block-staged; 3..8: dec_gemv_lds / dec_mm)
        DecGemvArgs g; DecRopeEpi re; DecAttn2Args da;
        qkv_args(l, defer_l[l] ? l & 1 : 0, g, re, da);
        if (defer_l[l]) {
            da.no_refill = l + 1 < L.layers && defer_l[l + 1];
            if (l >= 1 && defer_l[l - 1]) {
                const DecAttn2Args prev = attn_args(l - 1, B, Lmax, (l - 1) & 1);
                da.clean_qkv = const_cast<float*>(prev.qkv); da.clean_part = prev.part;
            }
        }
        bool attn_done = false;
        if (one_page) {
            if (qkv_attn_fused() && dec_qkv_attn_ok(g, re, da)) {
                // one launch: the attention blocks stream their K / V chunk beside the projection
                // (s_qkv stays sentinel-filled between launches; SKIP_ATTN, the profile's variant without
                // attention, projects into a scratch row so the hand-off row keeps its sentinels)
                if (step_skip_ & SKIP_ATTN) {
                    g.y = wsf("p_qkv_skip", (size_t)QKVN);
                    launch_dec_qkv_rope(g, re, st);
                } else {
                    stamped(SPAN_ATTN, l, [&] { launch_dec_qkv_attn(g, re, da, st); }, nullptr, 0);
                }
                attn_done = true;
            } else {
                launch_dec_qkv_rope(g, re, st);
            }
        } else if (B <= 8) {
            if (B >= 3 && !mm_swz_off()) g.w_swz = d.qkv_swz;
            launch_dec_gemv(g, st);
        } else {
            launch_rmsnorm(X, H, XN, H, B, H, d.in_norm.w, L.rms_eps, st);
            g.x = XN; g.norm_w = nullptr;
            launch_dec_gemv(g, st);
        }
        if (!attn_done && !(step_skip_ & SKIP_ATTN)) stamped(SPAN_ATTN, l, [&] { launch_dec_attn(da, st); }, nullptr, 0);
        // o_proj + residual
        DecGemvArgs go;
        go.M = B; go.N = H; go.K = L.heads * hd; go.x = CTX; go.ldx = H; go.W = d.o.W; go.ldw = go.K;
        go.wdtype = d.o.wdt; go.bias = d.o.b; go.y = X; go.ldy = H; go.accumulate = 1; go.span = chain_slots(l, SPAN_OPROJ);
        if (B >= 3 && B <= 8 && !mm_swz_off()) go.w_swz = d.o_swz;
        launch_dec_gemv(go, st);
        // MLP / MoE
        if (!d.moe && B >= 3 && B <= 8 && dense_mm_ok(d, B)) {
            // dense MLP (layer 0) on the matrix cores: gate|up with the post-attention RMSNorm fused,
            // SwiGLU, down as a split-K launch accumulating into the residual
            const int I = L.inter;
            float* G = wsf("s_dg", (size_t)B * 2 * I);
            float* HH = wsf("s_dhh", (size_t)B * I);
            DecGemvArgs g1;
            g1.M = B; g1.N = 2 * I; g1.K = H; g1.x = X; g1.ldx = H; g1.norm_w = d.post_norm.w; g1.eps = L.rms_eps;
            g1.W = d.gu.W; g1.ldw = H; g1.wdtype = d.gu.wdt; g1.bias = d.gu.b; g1.y = G; g1.ldy = 2 * I;
            if (!mm_swz_off()) g1.w_swz = d.gu_swz;
            launch_dec_gemv(g1, st);
            launch_silu_mul(G, 2 * I, I, B, HH, I, st);
            DecGemvArgs g2;
            g2.M = B; g2.N = H; g2.K = I; g2.x = HH; g2.ldx = I; g2.W = d.down.W; g2.ldw = I; g2.wdtype = d.down.wdt;
            g2.bias = d.down.b; g2.y = X; g2.ldy = H; g2.accumulate = 1;
            launch_dec_mm_splitk(g2, wsf("s_dpart", dec_mm_splitk_part_floats(H, I)), rows_.d_tick, st);
            continue;
        }
        if (!d.moe) {
            const float* mx = X;
            const float* mnorm = d.post_norm.w;
            if (!fuse_norm) { launch_rmsnorm(X, H, XN, H, B, H, d.post_norm.w, L.rms_eps, st); mx = XN; mnorm = nullptr; }
            MoeDec2Args m;
            m.T = B; m.K = H; m.Hout = H; m.x = mx; m.norm_w = mnorm; m.eps = L.rms_eps; m.out = X;
            m.topk = 0; m.E = 0; m.slots = 0; m.I = 8; m.Is = L.inter;
            m.sWgu = d.gu.W; m.sWd = d.down.W; m.wdtype = d.gu.wdt;
            m.hs = wsf("s_hh", (size_t)B * L.inter);
            m.n_active = wsi("s_nact", 1);
            launch_moe_gateup2(m, st);
            // one page: the down projection split over the 8 waves of a block (moe_down_mix; all of K in flight
            // at once) — moe_down2 walks each 6848-long row in four dependent load rounds
            MoeDec2Args dn = m;
            dn.slot_mode = 1;
            dn.ids = wsi("s_dense_ids", 8);  // no routed segments at topk 0: moe_down_mix reads no id
            if (dn.topk != 0) throw std::logic_error("dense layer with routed experts");
            if (B == 1 && moe_down_mix_ok(dn)) launch_moe_down_mix(dn, st);
            else launch_moe_down2(m, st);
            continue;
        }
        if (!span_rec_) {
            const int parts = MOE_ROUTE | ((step_skip_ & SKIP_GATEUP) ? 0 : MOE_GATEUP) | ((step_skip_ & SKIP_DOWN) ? 0 : MOE_DOWN);
            launch_moe_decode(moe_args(l, B, X), st, parts);
            continue;
        }
        MoeDecodeArgs ma = moe_args(l, B, X);
        ma.route_span = chain_slots(l, SPAN_ROUTER);
        launch_moe_decode(ma, st, MOE_ROUTE);
        ma.span = chain_active_ ? chain_slots(l, SPAN_GATEUP) : ((span_mode_ & SPAN_WAVES) ? span_slots_ : nullptr);
        stamped(SPAN_GATEUP, l, [&] { launch_moe_decode(ma, st, MOE_GATEUP); }, ma.ids, B * ma.topk);
        if (chain_active_) ma.span = chain_slots(l, SPAN_DOWN);
        stamped(SPAN_DOWN, l, [&] { launch_moe_decode(ma, st, MOE_DOWN); }, ma.ids, B * ma.topk);
    }
}

// the screened head's launch arguments for B rows of s_x (workspaces allocated here: call before a graph
// capture): B <= 2 the single-token kernel per page, 3..8 one int8 stream on the matrix cores
LmHeadQ8Args Engine::head_q8_args(int B) {
    const LangConfig& L = cfg_.lang;
    const int H = L.hidden;
    LmHeadQ8Args q;
    q.x = rows_.x; q.ldx = H; q.norm_w = final_norm_; q.eps = L.rms_eps;
    q.q = lmq_; q.scale = lmq_scale_; q.bound = lmq_bound_; q.B = B; q.N = L.vocab; q.K = H;
    if (B >= 3) {
        q.qfrag = lmq_frag_; q.qnorm = lmq_qnorm_;
        lmhead_q8mm_grid(L.vocab, H, B, &q.nblk, &q.slot);
    } else {
        lmhead_q8_grid(L.vocab, H, B, &q.nblk, &q.slot);
    }
    q.blk_cnt = wsi("s_blkcnt", (size_t)B * q.nblk); q.blk_t = wsf("s_blkt", (size_t)B * q.nblk);
    q.cand = wsi("s_cand", (size_t)B * q.nblk * q.slot); q.cand_hi = wsf("s_candhi", (size_t)B * q.nblk * q.slot);
    q.xn_out = wsf("s_lmxn", (size_t)B * H);
    return q;
}

void Engine::reserve_head_ws(int B) {
    if (!lmq_ || B > 8 || (B >= 3 && !lmq_frag_)) return;
    (void)head_q8_args(B);
}

// 3..8 pages: fragment-ordered copies of the lm_head and of every MoE layer's experts for the
// matrix-core kernels (decode_mm.hip: every wave weight load one contiguous 1 KiB block; lm_head 6.0 vs
// 4.6 TB/s row-major on MI355X, tools/kbench lm8), made once, outside any capture (HBM: + vocab x hidden
// + the expert weights again, ~5.3 GB of the 288)
void Engine::ensure_mm_weights(int B) {
    if (B > 8 || capturing_) return;
    const LangConfig& L = cfg_.lang;
    if (B >= 3 && !lm_swz_) {
        DecGemvArgs g;
        g.M = B; g.N = L.vocab; g.K = L.hidden; g.ldw = L.hidden;
        if (dec_mm_ok(g)) {
            lm_swz_ = dev_alloc(mm_swizzle_elems(L.vocab, L.hidden) * 2);
            launch_mm_swizzle(lm_head_.W, L.vocab, L.hidden, lm_swz_, stream_);
        }
    }
    // the experts of every MoE layer (routed [E * 2I][H], [E * H][I]; shared [2Is][H], [H][Is]): the
    // grouped matrix-core kernels stream them (3..8 pages)
    const int H = L.hidden, E = L.n_routed, I = L.moe_inter;
    if (B < 3) return;
    // q/k/v, o_proj and the dense gate|up for dec_mm (each wave load one contiguous 1 KiB instead of 64 bytes of
    // 16 rows: tools/mb_bcast.hip)
    auto swz = [&](const Lin& w, void*& out) {
        DecGemvArgs g;
        g.M = B; g.N = w.N; g.K = w.K; g.ldw = w.K;
        if (out || !w.W || (w.wdt != WDT_F16 && w.wdt != WDT_BF16) || !dec_mm_ok(g)) return;
        out = dev_alloc(mm_swizzle_elems(w.N, w.K) * 2);
        launch_mm_swizzle(w.W, w.N, w.K, out, stream_);
    };
    for (DecLayer& d : layers_) {
        swz(d.qkv, d.qkv_swz);
        swz(d.o, d.o_swz);
        if (!d.moe) swz(d.gu, d.gu_swz);
    }
    for (DecLayer& d : layers_) {
        if (!d.moe || d.packed || d.e_gu_swz || d.e_wdt != WDT_F16 || H % 32 || I % 32) continue;
        d.e_gu_swz = dev_alloc(mm_swizzle_elems(E * 2 * I, H) * 2);
        launch_mm_swizzle(d.e_gu, E * 2 * I, H, d.e_gu_swz, stream_);
        d.e_d_swz = dev_alloc(mm_swizzle_elems(E * H, I) * 2);
        launch_mm_swizzle(d.e_d, E * H, I, d.e_d_swz, stream_);
        if (d.has_shared && d.s_gu.wdt == WDT_F16) {
            const int Is = d.s_d.K;
            d.s_gu_swz = dev_alloc(mm_swizzle_elems(2 * Is, H) * 2);
            launch_mm_swizzle(d.s_gu.W, 2 * Is, H, d.s_gu_swz, stream_);
            d.s_d_swz = dev_alloc(mm_swizzle_elems(H, Is) * 2);
            launch_mm_swizzle(d.s_d.W, H, Is, d.s_d_swz, stream_);
        }
        if (d.router.W && d.router.wdt == WDT_F16 && E % 16 == 0) {
            d.router_swz = dev_alloc(mm_swizzle_elems(E, H) * 2);
            launch_mm_swizzle(d.router.W, E, H, d.router_swz, stream_);
        }
    }
    HIP_CHECK(hipStreamSynchronize(stream_));
}

// one page: q/k/v projection + decode attention as one launch (dec_qkv_attn); DSOCR_QKV_ATTN=0 (A/B
// switch, read once) keeps the two launches
// the fused launch's K / V loads held back behind the projection's weight stream: 150 ticks (1.5 us) from the
// attention block's entry (tools/kbench qkvattn1 sweep 0..300: 12.99 -> 12.49 us at L 1217, 11.36 -> 10.88 at
// L 707; decode layers 417.9 -> 411.6 us per step).  DSOCR_ATT_KV_DELAY (ticks of 10 ns) overrides; 0 = off
int Engine::att_kv_delay() {
    const char* e = getenv("DSOCR_ATT_KV_DELAY");
    return e ? std::max(0, atoi(e)) : 150;
}

// the fused one-page launch's sentinel refill moved off the merging blocks' exit onto the next layer's
// projection blocks (two hand-off copies, attn_args); DSOCR_ATT_REFILL_DEFER=0 (A/B switch): one copy, every
// launch refills what it read.  Read once per decode step (so once per captured step graph): both forms leave
// every hand-off word sentinel-filled at the step boundary, so either may follow the other - which is what lets
// one process time both (tools/ab_trace.py)
bool Engine::att_refill_defer() {
    const char* e = getenv("DSOCR_ATT_REFILL_DEFER");
    return !(e && atoi(e) == 0);
}

bool Engine::qkv_attn_fused() {
    static const bool v = !(getenv("DSOCR_QKV_ATTN") && atoi(getenv("DSOCR_QKV_ATTN")) == 0);
    return v;
}

// screened selection applies (lmhead.hip): int8 copy present, B <= 8 (3..8: the matrix-core form), no
// repetition penalty
// (DSOCR_SCREEN=0 forces the exact lm_head; read per generate call)
bool Engine::screen_applies(int B, float rep_penalty) const {
    if (getenv("DSOCR_SCREEN") && atoi(getenv("DSOCR_SCREEN")) == 0) return false;
    const bool pen = rep_penalty > 0.f && fabsf(rep_penalty - 1.0f) > 1.1920929e-07f;
    return lmq_ && !pen && (B <= 2 || (B <= 8 && lmq_frag_ && lmhead_q8mm_ok(B, cfg_.lang.vocab, cfg_.lang.hidden)));
}

// final norm + lm_head + greedy selection + step bookkeeping for the B decode rows in s_x
// screened: the int8 lm_head + screened final kernel (sa.ban_out holds the ban list the last step left, whichever
// head wrote it); else the exact lm_head, the penalty and the selection kernels
void Engine::decode_head(int B, DecSampleArgs& sa, const SampleArgs& pen, bool screened, const DecLpArgs* lp, bool stops,
                         int window) {
    const LangConfig& L = cfg_.lang;
    hipStream_t st = stream_;
    const int H = L.hidden;
    float* SX = rows_.x;
    if (screened && lp) throw std::runtime_error("EINTERNAL: log-probabilities need the exact head");
    if (screened && rows_.bias && !sess_) throw std::runtime_error("EINTERNAL: a logit bias needs the exact head");
    if (screened && rows_.pen && !sess_) throw std::runtime_error("EINTERNAL: penalties need the exact head");
    if (screened && window >= 0) throw std::runtime_error("EINTERNAL: a windowed n-gram ban needs the exact head");
    if (screened && rows_.g_on && !sess_) throw std::runtime_error("EINTERNAL: a token automaton needs the exact head");
    if (screened) {
        // screened selection: int8 lm_head intervals + running threshold, exact rescoring of the
        // few kept rows — the exact path's token from half the lm_head bytes
        LmHeadQ8Args q = head_q8_args(B);
        q.ban = sa.ban_out; q.ban_ld = sa.ban_ld;
        launch_lmhead_q8(q, st);
        DecSampleArgs ss = sa;
        ss.blk_cnt = q.blk_cnt; ss.blk_t = q.blk_t; ss.cand = q.cand; ss.cand_hi = q.cand_hi; ss.nblk = q.nblk; ss.slot = q.slot;
        ss.w_exact = lm_head_.W; ss.w_exact_wdt = lm_head_.wdt; ss.xn = q.xn_out; ss.K = H;
        if (getenv("DSOCR_SCREEN_STATS")) ss.stats = reinterpret_cast<unsigned long long*>(wsi("s_scrstats", 32));
        launch_dec_sample(ss, st);
        if (stops) stop_match(sa, 0);  // (selection is untouched: the match only reads what the final kernel appended)
        return;
    }
    DecGemvArgs g;
    g.M = B; g.N = L.vocab; g.K = H; g.W = lm_head_.W; g.ldw = H; g.wdtype = lm_head_.wdt; g.bias = lm_head_.b;
    g.y = const_cast<float*>(sa.logits); g.ldy = L.vocab;
    if (B <= 2 || (lm_swz_ && B <= 8)) {  // final RMSNorm fused (B 3..8: dec_mm on the fragment-ordered copy)
        g.x = SX; g.ldx = H; g.norm_w = final_norm_; g.eps = L.rms_eps;
        if (B > 2) g.w_swz = lm_swz_;
    } else {
        float* SXN = wsf("s_xn", (size_t)B * H);
        launch_rmsnorm(SX, H, SXN, H, B, H, final_norm_, L.rms_eps, st);
        g.x = SXN; g.ldx = H;
    }
    launch_dec_gemv(g, st);
    if (trace_) launch_trace_logits(sa.logits, B, L.vocab, sa.ld, sa.out_len, sa.done, trace_, trace_steps_, st);
    TailPlan t;
    t.bias = rows_.bias != nullptr; t.guided = rows_.g_on != nullptr; t.penalties = rows_.pen != nullptr;
    t.stops = stops; t.window = window; t.lp = lp;
    selection_tail(sa, pen, 0, t);
}

// The exact selection on logits already formed (the decode step's lm_head, or a prefill's), in the one order every
// control is defined against
void Engine::selection_tail(const DecSampleArgs& sa, const SampleArgs& pen, int row0, const TailPlan& t) {
    hipStream_t st = stream_;
    if (t.bias) launch_dec_logit_bias(bias_args(sa, row0), st);  // l' = l + b: what everything below reads
    if (t.guided) launch_dec_guided_mask(guided_mask_args(sa, row0), st);  // -inf wherever the row's state has no edge
    if (t.lp) launch_dec_lp_partial(*t.lp, st);
    launch_rep_penalty(pen, st);
    if (t.penalties) launch_dec_out_penalty(penalty_args(sa, row0), st);  // frequency / presence, per row
    DecSampleArgs s0 = sa;
    if (t.window >= 0) {  // every row's ban in the window launch, the selection without one
        launch_dec_ngram_window(ngram_window_args(sa, row0, t.window), st);
        s0.ngram = 0;  // (per-request rows: a windowed row's RowParams carry ngram 0, the others keep their own ban)
    }
    launch_dec_sample(s0, st);  // the token, its embedding into the row's s_x, the ban list, the KV position
    if (t.guided) launch_dec_guided_advance(guided_advance_args(sa, row0), st);  // the appended token's edge
    if (t.stops) stop_match(sa, row0);
    if (t.lp) launch_dec_lp_final(*t.lp, st);
}

// ---- the decode rows (engine.hpp DecodeRows).  Every buffer below has its size in this one function; the names
// are the workspace names tools and a session's freeze-by-prefix know.
void Engine::reserve_decode_rows(const DecodeRowsSpec& spec) {
    const LangConfig& L = cfg_.lang;
    const int S = spec.rows, H = L.hidden, V = L.vocab;
    hipStream_t st = stream_;
    last_B_ = last_Lmax_ = 0;  // profile_decode replays a generate that finished on these rows
    rows_ = DecodeRows();
    DecodeRows& r = rows_;
    r.S = S; r.Lcap = spec.Lcap; r.ctx_cap = spec.ctx_cap; r.out_cap = spec.out_cap; r.ban_ld = r.ctx_cap + 1;
    // KV cache [layers][S][kvh][Lcap][hd] f32 (block.rs:776-789 keeps the cache in f32)
    head_stride_ = (long)r.Lcap * L.head_dim;
    page_stride_ = (long)L.kv_heads * head_stride_;
    const size_t kv_floats = (size_t)L.layers * S * page_stride_;
    kc_ = wsf("kv_k", kv_floats);
    vc_ = wsf("kv_v", kv_floats);
    if (spec.zero_fill) {
        HIP_CHECK(hipMemsetAsync(kc_, 0, kv_floats * 4, st));
        HIP_CHECK(hipMemsetAsync(vc_, 0, kv_floats * 4, st));
    }
    // n ints under `name`, zeroed on request (+ pad bytes: rows the caller fills with upload()-sized copies)
    auto ints = [&](const char* name, size_t n, bool zero, size_t pad = 0) {
        int* d = (int*)ws(name, n * sizeof(int) + pad);
        if (zero) HIP_CHECK(hipMemsetAsync(d, 0, sizeof(int) * n, st));
        return d;
    };
    // the step-wide words: the arrival tickets (every launch leaves them zero) and the fused kernels' give-up flag
    r.attn_cnt = ints("s_attn_cnt", (size_t)S * L.heads, true);
    r.route_cnt = ints("s_route_cnt", 16, true);
    r.dn_tick = ints("s_dntick", (size_t)H / 64 + 1, true);
    r.d_tick = ints("s_dtick", dec_mm_splitk_ticks(H), true);
    r.err = ints("s_err", 4, true);
    // the hand-off copies: the attention records of `rows` pages, or of whichever n <= rows needs the most
    for (int n = spec.handoff_max ? 1 : S; n <= S; ++n)
        r.part_floats = std::max(r.part_floats, dec_attn_workspace(n, L.heads, L.head_dim, r.Lcap) / 4 + 16);
    r.qkv_floats = (size_t)S * layers_[0].qkv.N;
    r.part[0] = wsf("s_part", r.part_floats); r.qkv[0] = wsf("s_qkv", r.qkv_floats);
    r.part[1] = wsf("s_part1", r.part_floats); r.qkv[1] = wsf("s_qkv1", r.qkv_floats);
    wsf("p_qkv_skip", r.qkv_floats);  // the profile's variant without attention projects here (allocated before capture)
    refill_handoffs();
    // the per-row state
    const bool z = spec.zero_fill;
    const size_t pad = z ? 0 : 16;
    r.x = wsf("s_x", (size_t)S * H);
    if (z) HIP_CHECK(hipMemsetAsync(r.x, 0, sizeof(float) * S * H, st));
    wsf("s_xn", (size_t)S * H);
    r.logits = wsf("s_logits", (size_t)S * V);
    r.ctx = ints("s_ctx_ids", (size_t)S * r.ctx_cap, z, pad);
    r.ctx_len = ints("s_ctx_len", S, z, pad);
    r.kv_pos = ints("s_kvpos", S, z);
    r.kv_len = ints("s_kvlen", S, z);
    r.done = ints("s_done", S, z, pad);
    r.out_len = ints("s_outlen", S, z, pad);
    r.out = ints("s_out", (size_t)S * r.out_cap, z);
    r.tok = ints("s_tok", S, z);
    const size_t red = dec_sample_blocks(V);
    r.red_val = wsf("s_redv", (size_t)S * red);
    r.red_idx = wsi("s_redi", (size_t)S * red);
    if (spec.sampler) {
        r.st_key = reinterpret_cast<uint32_t*>(wsi("s_stkey", (size_t)S * 2 * V));
        r.st_idx = wsi("s_stidx", (size_t)S * 2 * V);
        r.st_w = reinterpret_cast<double*>(wsf("s_stw", (size_t)S * 2 * V));
        r.rng = reinterpret_cast<uint32_t*>(ints("s_rng", (size_t)S * RNG_WORDS, z, pad));
    }
    if (spec.rowpar) r.rowpar = reinterpret_cast<RowParams*>(ws("s_rowpar", sizeof(RowParams) * S));
    // the n-gram ban list each selection kernel leaves for the screened head of the next step
    if (spec.ban) r.ban = ints("s_ban", (size_t)S * r.ban_ld, z);
    if (spec.lp_k >= 0) {
        const size_t R = (size_t)S, nch = dec_lp_chunks(V), cap = (size_t)r.out_cap, kk = (size_t)std::max(spec.lp_k, 1);
        r.lp_k = spec.lp_k;
        r.lp = wsf("s_lp", R * cap);
        r.lp_top = wsf("s_lptop", R * cap * kk);
        r.lp_top_id = wsi("s_lptopid", R * cap * kk);
        if (spec.lp_side) r.lp_side = wsf("s_lpctx", R * (size_t)r.ctx_cap);
        r.lp_rec = wsi("s_lprec", R * 2);
        r.lp_pmax = wsf("s_lppmax", R * nch); r.lp_psum = wsf("s_lppsum", R * nch);
        r.lp_ptv = wsf("s_lpptv", R * nch * kk); r.lp_pti = wsi("s_lppti", R * nch * kk);
        if (z) {  // (an admission resets its slot's entries)
            HIP_CHECK(hipMemsetAsync(r.lp_rec, 0, sizeof(int) * 2 * R, st));
            HIP_CHECK(hipMemsetAsync(r.lp, 0, sizeof(float) * R * cap, st));
            HIP_CHECK(hipMemsetAsync(r.lp_top_id, 0, sizeof(int) * R * cap * r.lp_k, st));
            HIP_CHECK(hipMemsetAsync(r.lp_top, 0, sizeof(float) * R * cap * r.lp_k, st));
            if (r.lp_side) HIP_CHECK(hipMemsetAsync(r.lp_side, 0, sizeof(float) * R * r.ctx_cap, st));
        }
    }
    if (spec.bias) {  // (the dense rows are written by launch_logit_bias_build before a flag is set)
        r.bias_ld = logit_bias_ld(V);
        r.bias = wsf("s_bias", (size_t)S * r.bias_ld);
        r.bias_on = ints("s_biason", S, true);
        r.bias_stage_cap = std::max<size_t>(spec.bias_stage, 1);
        r.bias_stage = wsi("s_biasstage", 2 * r.bias_stage_cap);
    }
    if (spec.stops) {  // (a table is written by launch_stop_table_build before its count is set)
        r.stop_tab = wsi("s_stoptab", (size_t)S * STOP_ROW_INTS);
        r.stop_n = ints("s_stopn", S, true);
        r.stop_seen = ints("s_stopseen", S, true);
        r.stop_hit = ints("s_stophit", (size_t)S * 2, true);
        r.stop_stage_rows = std::max(spec.stop_stage_rows, 1);
        r.stop_stage = wsi("s_stopstage", (size_t)r.stop_stage_rows * STOP_STAGE_INTS);
    }
    if (spec.penalties) {  // every record off until an admission / init_sampling writes it
        r.pen = reinterpret_cast<PenaltyRec*>(ws("s_pen", sizeof(PenaltyRec) * S));
        const std::vector<PenaltyRec> off((size_t)S);
        upload_to(r.pen, "s_penstage", off);
    }
    if (spec.ngram_window) {  // the same
        r.ngw = reinterpret_cast<NgramWindowRec*>(ws("s_ngw", sizeof(NgramWindowRec) * S));
        const std::vector<NgramWindowRec> off((size_t)S);
        upload_to(r.ngw, "s_ngwstage", off);
    }
    if (spec.guided) {  // (a row's tables are written by launch_guided_build, which sets its flag)
        const size_t R = (size_t)S;
        r.g_states = std::min(std::max(spec.guided_states, 1), GUIDED_MAX_STATES);
        r.g_edges = std::min(std::max<long>(spec.guided_edges, 1), GUIDED_MAX_EDGES);
        r.g_mask_ld = guided_mask_ld(V);
        r.g_mask = reinterpret_cast<uint32_t*>(wsi("s_gmask", R * r.g_states * r.g_mask_ld));
        r.g_rowptr = wsi("s_growptr", R * (r.g_states + 1));
        r.g_tok = wsi("s_gtok", R * r.g_edges);
        r.g_next = wsi("s_gnext", R * r.g_edges);
        r.g_state = ints("s_gstate", S, true);
        r.g_seen = ints("s_gseen", S, true);
        r.g_status = ints("s_gstatus", S, true);
        r.g_on = ints("s_gon", S, true);
        r.g_stage_cap = std::max<size_t>(spec.guided_stage, 1);
        r.g_stage = wsi("s_gstage", r.g_stage_cap);
    }
}

// The fused one-page launch takes q / k / v by polling its hand-off row, and the attention merge polls its records:
// both enter a launch sentinel-filled.  A step at another n leaves them in that n's layout, so a session refills them
// whenever n changes (admit, retire)
void Engine::refill_handoffs() {
    for (int c = 0; c < 2; ++c) {
        dec_attn_part_init(rows_.part[c], rows_.part_floats * 4, stream_);
        dec_qkv_sentinel_init(rows_.qkv[c], rows_.qkv_floats, stream_);
    }
}

// selection arguments for the B rows from slot0 on (generate and a session's step: slot0 = 0; an admission: its
// slot, B = 1).  per_request: the kernels read the rows' RowParams records, not the scalars
void Engine::sample_args(int B, int slot0, const GenParams& p, bool per_request, DecSampleArgs& sa, SampleArgs& pen) {
    const DecodeRows& r = rows_;
    const int V = cfg_.lang.vocab, H = cfg_.lang.hidden;
    const size_t o = (size_t)slot0, red = dec_sample_blocks(V);
    pen = SampleArgs();
    pen.logits = r.logits + o * V; pen.B = B; pen.V = V; pen.ld = V;
    pen.ctx = r.ctx + o * r.ctx_cap; pen.ctx_cap = r.ctx_cap; pen.ctx_len = r.ctx_len + o;
    pen.rep_penalty = p.rep_penalty;
    sa = DecSampleArgs();
    sa.logits = pen.logits; sa.B = B; sa.V = V; sa.ld = V;
    sa.ctx = r.ctx + o * r.ctx_cap; sa.ctx_cap = r.ctx_cap; sa.ctx_len = r.ctx_len + o; sa.ngram = p.ngram;
    sa.red_blocks = (int)red; sa.red_val = r.red_val + o * red; sa.red_idx = r.red_idx + o * red;
    sa.out_tok = r.tok + o; sa.out_ids = r.out + o * r.out_cap; sa.out_len = r.out_len + o;
    sa.out_cap = r.out_cap; sa.done = r.done + o;
    sa.eos = p.ignore_eos ? -1 : (int)p.eos;
    sa.table = embed_; sa.table_dt = embed_dt_; sa.H = H; sa.x_next = r.x + o * H;
    sa.kv_pos = r.kv_pos + o; sa.kv_len = r.kv_len + o;
    if (per_request) pen.rows = sa.rows = r.rowpar + o;
    if (p.do_sample || per_request) {
        // stochastic selection (sampling.hip) on the sampler's scratch and the rows' RNG states
        sa.do_sample = p.do_sample ? 1 : 0; sa.temperature = p.temperature; sa.top_p = p.top_p; sa.top_k = p.top_k;
        sa.st_ld = V;
        sa.st_key = r.st_key + o * 2 * V; sa.st_idx = r.st_idx + o * 2 * V; sa.st_w = r.st_w + o * V;
        sa.rng = r.rng + o * RNG_WORDS;
    }
    if (r.ban) { sa.ban_ld = r.ban_ld; sa.ban_out = r.ban + o * r.ban_ld; }
    if (r.pen) sa.pen = r.pen + o;  // min-p of the sampled rows
}

// the log-probability rows as the arguments of the pages [row0, row0 + sa.B) whose selection sa describes
DecLpArgs Engine::lp_args(const DecSampleArgs& sa, int row0) {
    const DecodeRows& r = rows_;
    const size_t o = (size_t)row0, nch = dec_lp_chunks(sa.V), cap = (size_t)r.out_cap, K = (size_t)r.lp_k;
    DecLpArgs a;
    a.logits = sa.logits; a.B = sa.B; a.V = sa.V; a.ld = sa.ld; a.K = r.lp_k;
    a.tok = sa.out_tok; a.out_len = sa.out_len; a.out_cap = sa.out_cap;
    a.ctx = sa.ctx; a.ctx_cap = sa.ctx_cap; a.ctx_len = sa.ctx_len;
    a.lp = r.lp + o * cap; a.top_lp = r.lp_top + o * cap * K; a.top_id = r.lp_top_id + o * cap * K;
    if (r.lp_side) a.side = r.lp_side + o * r.ctx_cap;
    a.rec = r.lp_rec + o * 2;
    a.part_max = r.lp_pmax + o * nch; a.part_sum = r.lp_psum + o * nch;
    a.part_tv = r.lp_ptv + o * nch * K; a.part_ti = r.lp_pti + o * nch * K;
    return a;
}

DecBiasArgs Engine::bias_args(const DecSampleArgs& sa, int row0) {
    const DecodeRows& r = rows_;
    DecBiasArgs a;
    a.logits = const_cast<float*>(sa.logits); a.B = sa.B; a.V = sa.V; a.ld = sa.ld;
    a.bias = r.bias + (size_t)row0 * r.bias_ld; a.bias_ld = r.bias_ld; a.on = r.bias_on + row0;
    return a;
}

DecPenaltyArgs Engine::penalty_args(const DecSampleArgs& sa, int row0) {
    DecPenaltyArgs a;
    a.logits = const_cast<float*>(sa.logits); a.B = sa.B; a.V = sa.V; a.ld = sa.ld;
    a.out_ids = sa.out_ids; a.out_cap = sa.out_cap; a.out_len = sa.out_len;
    a.rec = rows_.pen + row0;
    return a;
}

PenaltyRec Penalties::rec() const {
    PenaltyRec r;
    r.frequency = frequency; r.presence = presence;
    r.ln_min_p = min_p > 0.0 ? std::log(min_p) : -INFINITY;
    return r;
}

DecNgramWindowArgs Engine::ngram_window_args(const DecSampleArgs& sa, int row0, int plain) {
    DecNgramWindowArgs a;
    a.logits = const_cast<float*>(sa.logits); a.B = sa.B; a.V = sa.V; a.ld = sa.ld;
    a.ctx = sa.ctx; a.ctx_cap = sa.ctx_cap; a.ctx_len = sa.ctx_len;
    a.rec = rows_.ngw + row0;
    a.plain = plain;
    return a;
}

NgramWindowRec NgramWindow::rec() const {
    NgramWindowRec r;
    if (!active()) return r;
    r.g = g; r.w = w;
    for (int t : whitelist) {
        bool seen = false;
        for (int q = 0; q < r.n_white; ++q) seen = seen || r.white[q] == t;
        if (!seen && r.n_white < NGRAM_MAX_WHITELIST) r.white[r.n_white++] = t;
    }
    return r;
}

void validate_ngram_window(const NgramWindow& nw, int vocab) {
    if (nw.g >= 2 && nw.w < 1) throw std::runtime_error("EINVAL: n-gram window: window must be at least 1");
    std::vector<int> uniq;
    for (int t : nw.whitelist) {
        if (t < 0 || t >= vocab) throw std::runtime_error("EINVAL: n-gram window: whitelist id outside the vocabulary");
        if (std::find(uniq.begin(), uniq.end(), t) == uniq.end()) uniq.push_back(t);
    }
    if (uniq.size() > (size_t)NGRAM_MAX_WHITELIST)
        throw std::runtime_error("EINVAL: n-gram window: more than " + std::to_string(NGRAM_MAX_WHITELIST) + " whitelist ids");
}

// (one record per row in the staging buffer, as for the penalties)
void Engine::write_ngram_windows(const GenRequest* reqs, int row0, int n) {
    const DecodeRows& r = rows_;
    if (!r.ngw) throw std::runtime_error("EINTERNAL: no n-gram window records are reserved");
    NgramWindowRec* h = (NgramWindowRec*)pinned("s_ngwstage", sizeof(NgramWindowRec) * (size_t)r.S);
    for (int i = 0; i < n; ++i) h[row0 + i] = reqs[i].ctl.ngw.rec();
    HIP_CHECK(hipMemcpyAsync(r.ngw + row0, h + row0, sizeof(NgramWindowRec) * (size_t)n, hipMemcpyHostToDevice, stream_));
}

void validate_penalties(const Penalties& pn) {
    if (!std::isfinite(pn.frequency) || !std::isfinite(pn.presence))
        throw std::runtime_error("EINVAL: penalties: frequency_penalty and presence_penalty must be finite");
    if (std::isnan(pn.min_p) || pn.min_p < 0.0 || pn.min_p > 1.0)
        throw std::runtime_error("EINVAL: penalties: min_p must lie in [0, 1]");
}

// (the staging buffer holds one record per row: rows written between two synchronisations do not overlap)
void Engine::write_penalties(const GenRequest* reqs, int row0, int n) {
    const DecodeRows& r = rows_;
    if (!r.pen) throw std::runtime_error("EINTERNAL: no penalty records are reserved");
    PenaltyRec* h = (PenaltyRec*)pinned("s_penstage", sizeof(PenaltyRec) * (size_t)r.S);
    for (int i = 0; i < n; ++i) h[row0 + i] = reqs[i].ctl.pen.rec();
    HIP_CHECK(hipMemcpyAsync(r.pen + row0, h + row0, sizeof(PenaltyRec) * (size_t)n, hipMemcpyHostToDevice, stream_));
}

void validate_logit_bias(const LogitBias& lb, int vocab) {
    const size_t n = lb.ids.size();
    if (lb.values.size() != n) throw std::runtime_error("EINVAL: logit bias: ids and values differ in length");
    if (n > (size_t)vocab) throw std::runtime_error("EINVAL: logit bias: more entries than the vocabulary has ids");
    if (lb.allow_only && n == 0) throw std::runtime_error("EINVAL: logit bias: allow_only with an empty list permits no token");
    std::vector<uint8_t> seen((size_t)vocab, 0);
    for (size_t i = 0; i < n; ++i) {
        const int t = lb.ids[i];
        if (t < 0 || t >= vocab) throw std::runtime_error("EINVAL: logit bias: token id " + std::to_string(t) + " outside the vocabulary");
        if (seen[t]) throw std::runtime_error("EINVAL: logit bias: duplicate token id " + std::to_string(t));
        seen[t] = 1;
        const float v = lb.values[i];
        if (std::isnan(v) || v == INFINITY) throw std::runtime_error("EINVAL: logit bias: a value is NaN or +inf");
    }
}

// One row's list over PCIe ([ids | values], pinned staging under "s_biasstage"), then the fill + scatter on the
// stream.  The caller synchronises before the staging region is reused
void Engine::build_logit_bias(const LogitBias& lb, int row, size_t stage_off) {
    const DecodeRows& r = rows_;
    if (!r.bias) throw std::runtime_error("EINTERNAL: no logit bias rows are reserved");
    const size_t n = lb.ids.size(), cap = r.bias_stage_cap;
    if (stage_off + n > cap) throw std::runtime_error("EINTERNAL: logit bias staging buffer too small");
    LogitBiasBuildArgs a;
    a.row = r.bias + (size_t)row * r.bias_ld; a.V = cfg_.lang.vocab; a.ld = r.bias_ld;
    a.on = r.bias_on + row; a.on_value = lb.active() ? 1 : 0; a.allow_only = lb.allow_only ? 1 : 0;
    if (a.on_value && n) {
        int* h = (int*)pinned("s_biasstage", 2 * cap * sizeof(int));
        std::memcpy(h + stage_off, lb.ids.data(), n * sizeof(int));
        std::memcpy(h + cap + stage_off, lb.values.data(), n * sizeof(float));
        HIP_CHECK(hipMemcpyAsync(r.bias_stage + stage_off, h + stage_off, n * sizeof(int), hipMemcpyHostToDevice, stream_));
        HIP_CHECK(hipMemcpyAsync(r.bias_stage + cap + stage_off, h + cap + stage_off, n * sizeof(float), hipMemcpyHostToDevice, stream_));
        a.ids = r.bias_stage + stage_off;
        a.values = reinterpret_cast<const float*>(r.bias_stage + cap + stage_off);
        a.n = (int)n;
    }
    launch_logit_bias_build(a, stream_);
}

DecGuidedMaskArgs Engine::guided_mask_args(const DecSampleArgs& sa, int row0) {
    DecGuidedMaskArgs a;
    a.logits = const_cast<float*>(sa.logits); a.B = sa.B; a.V = sa.V; a.ld = sa.ld;
    a.done = sa.done;
    a.t = rows_.guided_tables().at(row0);
    return a;
}

DecGuidedAdvanceArgs Engine::guided_advance_args(const DecSampleArgs& sa, int row0) {
    DecGuidedAdvanceArgs a;
    a.B = sa.B; a.out = sa.out_ids; a.out_cap = sa.out_cap; a.out_len = sa.out_len; a.done = sa.done;
    a.t = rows_.guided_tables().at(row0);
    return a;
}

void validate_guided(const Guided& g, int vocab, long eos) {
    if (!g.active() && g.accepting.empty() && g.row_ptr.empty() && g.edge_tok.empty() && g.edge_next.empty()) return;
    const int n = g.n_states;
    if (n < 1 || n > GUIDED_MAX_STATES)
        throw std::runtime_error("EINVAL: token automaton: n_states must be 1.." + std::to_string(GUIDED_MAX_STATES));
    if (g.accepting.size() != (size_t)n || g.row_ptr.size() != (size_t)n + 1)
        throw std::runtime_error("EINVAL: token automaton: accepting has n_states entries and row_ptr n_states + 1");
    if (g.row_ptr[0] != 0) throw std::runtime_error("EINVAL: token automaton: row_ptr must start at 0");
    for (int s = 0; s < n; ++s)
        if (g.row_ptr[s + 1] < g.row_ptr[s]) throw std::runtime_error("EINVAL: token automaton: row_ptr must not decrease");
    const long E = g.row_ptr[n];
    if (E > GUIDED_MAX_EDGES)
        throw std::runtime_error("EINVAL: token automaton: more than " + std::to_string(GUIDED_MAX_EDGES) + " edges");
    if (g.edge_tok.size() != (size_t)E || g.edge_next.size() != (size_t)E)
        throw std::runtime_error("EINVAL: token automaton: row_ptr must end at the number of edges");
    for (int s = 0; s < n; ++s)
        for (int e = g.row_ptr[s]; e < g.row_ptr[s + 1]; ++e) {
            const int t = g.edge_tok[e];
            if (t < 0 || t >= vocab) throw std::runtime_error("EINVAL: token automaton: token id " + std::to_string(t) + " outside the vocabulary");
            if ((long)t == eos) throw std::runtime_error("EINVAL: token automaton: an edge on the EOS id (mark the state accepting instead)");
            if (e > g.row_ptr[s] && g.edge_tok[e - 1] >= t)
                throw std::runtime_error("EINVAL: token automaton: token ids must ascend strictly within a state");
            if (g.edge_next[e] < 0 || g.edge_next[e] >= n) throw std::runtime_error("EINVAL: token automaton: edge_next outside [0, n_states)");
        }
    if (g.start < 0 || g.start >= n) throw std::runtime_error("EINVAL: token automaton: start outside [0, n_states)");
    if (g.row_ptr[g.start] == g.row_ptr[g.start + 1]) throw std::runtime_error("EINVAL: token automaton: the start state is terminal");
}

// One row's automaton over PCIe ([accepting | row_ptr | edge_tok | edge_next], pinned staging under "s_gstage"),
// then the fill + scatter on the stream.  The caller synchronises before the staging region is reused
void Engine::build_guided(const Guided& g, int row, size_t stage_off, long eos) {
    const DecodeRows& r = rows_;
    if (!r.g_on) throw std::runtime_error("EINTERNAL: no token automaton rows are reserved");
    GuidedBuildArgs a;
    a.t = r.guided_tables().at(row);
    if (g.active()) {
        const size_t n = (size_t)g.n_states, E = (size_t)g.edges(), ints = guided_stage_ints(g.n_states, g.edges());
        if (stage_off + ints > r.g_stage_cap) throw std::runtime_error("EINTERNAL: token automaton staging buffer too small");
        if (g.n_states > r.g_states || g.edges() > r.g_edges) throw std::runtime_error("EINTERNAL: token automaton rows too small");
        int* h = (int*)pinned("s_gstage", r.g_stage_cap * sizeof(int)) + stage_off;
        for (size_t i = 0; i < n; ++i) h[i] = g.accepting[i] ? 1 : 0;
        std::memcpy(h + n, g.row_ptr.data(), (n + 1) * sizeof(int));
        if (E) {
            std::memcpy(h + 2 * n + 1, g.edge_tok.data(), E * sizeof(int));
            std::memcpy(h + 2 * n + 1 + E, g.edge_next.data(), E * sizeof(int));
        }
        HIP_CHECK(hipMemcpyAsync(r.g_stage + stage_off, h, ints * sizeof(int), hipMemcpyHostToDevice, stream_));
        a.stage = r.g_stage + stage_off;
        a.n_states = g.n_states; a.start = g.start; a.V = cfg_.lang.vocab; a.E = g.edges();
        a.eos = (eos >= 0 && eos < cfg_.lang.vocab) ? (int)eos : -1;
    }
    launch_guided_build(a, stream_);
}

DecStopArgs Engine::stop_args(const DecSampleArgs& sa, int row0) {
    const DecodeRows& r = rows_;
    DecStopArgs a;
    a.B = sa.B; a.out = sa.out_ids; a.out_cap = sa.out_cap; a.out_len = sa.out_len; a.done = sa.done;
    a.tab = r.stop_tab + (size_t)row0 * STOP_ROW_INTS; a.n_seq = r.stop_n + row0;
    a.seen = r.stop_seen + row0; a.hit = r.stop_hit + (size_t)row0 * 2;
    return a;
}

// (a launch recorded into a step graph is counted where the graph is replayed)
void Engine::stop_match(const DecSampleArgs& sa, int row0) {
    if (!rows_.stop_tab) throw std::runtime_error("EINTERNAL: no stop rows are reserved");
    launch_dec_stop_match(stop_args(sa, row0), stream_);
    if (!capturing_) ++stop_launches_;
}

void validate_stop_set(const StopSet& st, int vocab) {
    if (st.seqs.size() > (size_t)STOP_MAX_SEQS)
        throw std::runtime_error("EINVAL: stop set: more than " + std::to_string(STOP_MAX_SEQS) + " sequences");
    for (size_t i = 0; i < st.seqs.size(); ++i) {
        const std::vector<int>& q = st.seqs[i];
        if (q.empty() || q.size() > (size_t)STOP_MAX_LEN)
            throw std::runtime_error("EINVAL: stop set: a sequence has 1.." + std::to_string(STOP_MAX_LEN) + " token ids");
        for (int t : q)
            if (t < 0 || t >= vocab) throw std::runtime_error("EINVAL: stop set: token id " + std::to_string(t) + " outside the vocabulary");
        for (size_t j = 0; j < i; ++j)
            if (st.seqs[j] == q) throw std::runtime_error("EINVAL: stop set: sequences " + std::to_string(j) + " and " + std::to_string(i) + " are identical");
    }
}

// One row's list over PCIe ([n | lens | ids], pinned staging under "s_stopstage"), then the table build on the
// stream.  The caller synchronises before the staging region is reused
void Engine::build_stop_table(const StopSet& stp, int row, int stage_row) {
    const DecodeRows& r = rows_;
    if (!r.stop_tab) throw std::runtime_error("EINTERNAL: no stop rows are reserved");
    if (stage_row < 0 || stage_row >= r.stop_stage_rows) throw std::runtime_error("EINTERNAL: stop staging buffer too small");
    StopBuildArgs a;
    a.tab = r.stop_tab + (size_t)row * STOP_ROW_INTS; a.n_seq = r.stop_n + row; a.seen = r.stop_seen + row;
    a.hit = r.stop_hit + (size_t)row * 2;
    if (stp.active()) {
        int* h = (int*)pinned("s_stopstage", (size_t)r.stop_stage_rows * STOP_STAGE_INTS * sizeof(int)) + (size_t)stage_row * STOP_STAGE_INTS;
        std::memset(h, 0, STOP_STAGE_INTS * sizeof(int));
        h[0] = (int)stp.seqs.size();
        size_t off = 0;
        for (size_t i = 0; i < stp.seqs.size(); ++i) {
            h[1 + i] = (int)stp.seqs[i].size();
            std::memcpy(h + 1 + STOP_MAX_SEQS + off, stp.seqs[i].data(), stp.seqs[i].size() * sizeof(int));
            off += stp.seqs[i].size();
        }
        int* d = r.stop_stage + (size_t)stage_row * STOP_STAGE_INTS;
        HIP_CHECK(hipMemcpyAsync(d, h, STOP_STAGE_INTS * sizeof(int), hipMemcpyHostToDevice, stream_));
        a.stage = d;
    }
    launch_stop_table_build(a, stream_);
}

void Controls::validate(int vocab, long eos) const {
    if (bias.active()) validate_logit_bias(bias, vocab);  // (a record that is off passes the other four)
    validate_stop_set(stops, vocab);
    validate_penalties(pen);
    validate_ngram_window(ngw, vocab);
    validate_guided(guided, vocab, eos);
}

// Every write goes to a buffer that no launch of the selection tail before its own reads, so all of them can precede
// the tail.  A request without a control clears the row's flag / count or writes an off record.  The caller
// synchronises before the staging regions are reused
void Engine::write_controls(const GenRequest* reqs, int row0, int n, long eos) {
    const DecodeRows& r = rows_;
    size_t bias_off = 0, guided_off = 0;
    for (int i = 0; i < n; ++i) {
        const Controls& c = reqs[i].ctl;
        if (r.bias) {
            build_logit_bias(c.bias, row0 + i, bias_off);
            bias_off += c.bias.ids.size();
        }
        if (r.g_on) {
            build_guided(c.guided, row0 + i, guided_off, eos);
            if (c.guided.active()) guided_off += guided_stage_ints(c.guided.n_states, c.guided.edges());
        }
        if (r.stop_tab) build_stop_table(c.stops, row0 + i, i);
    }
    if (r.pen) write_penalties(reqs, row0, n);
    if (r.ngw) write_ngram_windows(reqs, row0, n);
}

// rand_core 0.6.4 SeedableRng::seed_from_u64 for ChaCha12Rng (rand 0.8.5 StdRng): the 32-byte key
// is filled by PCG32 (state advanced first, XSH-RR output, little-endian words); block counter 0,
// stream 0, empty result buffer (sampling.hip reads this layout)
std::vector<uint32_t> rng_state_from_u64(uint64_t state) {
    std::vector<uint32_t> st(RNG_WORDS, 0u);
    for (int i = 0; i < 8; ++i) {
        state = state * 6364136223846793005ull + 11634580027462260723ull;
        const uint32_t xorshifted = (uint32_t)(((state >> 18) ^ state) >> 27);
        const uint32_t rot = (uint32_t)(state >> 59);
        st[RNG_KEY + i] = (xorshifted >> rot) | (xorshifted << ((32 - rot) & 31));
    }
    st[RNG_IDX] = 64;
    return st;
}

// ============================================================================ generate
// One generate() call: what its phases hand to each other.  The events and the pinned buffer die with it.
struct Engine::GenState {
    GenState(const std::vector<GenRequest>& r, const GenParams& gp, TokenCb c, void* u)
        : reqs(r), p(gp), cb(c), user(u), B((int)r.size()) {}
    const std::vector<GenRequest>& reqs;
    const GenParams& p;
    TokenCb cb;
    void* user;
    const int B;
    HipEvent ev[6];  // stream marks: vision [0, 1], prefill [2, 3], decode loop [4, 5]
    std::vector<int> prompt_len;
    int max_p = 0;
    std::vector<const float*> gpost, lpost;              // per page: its global / local post rows (device)
    std::vector<float> host_rows;                        // caller-supplied image rows of every page (ROW_HOST)
    float* vis_rows = nullptr;                           // every page's [local | global] post rows, contiguous
    std::vector<std::vector<std::pair<int, long>>> img;  // per page: (kind, index) of every <image> slot
    std::vector<std::vector<int>> extra;                 // per page: the tokens a forward without cache appends
    std::vector<int> kvpos, kvlen;                       // first decode position / cache length of every page
    PinnedBuffer<int> pin;  // poll(): [done | output length | last token] x B
    int streamed = 0;       // tokens the stream callback has seen
    size_t steps = 0;
};

std::vector<std::vector<int64_t>> Engine::generate(const std::vector<GenRequest>& reqs, const GenParams& p, TokenCb cb,
                                                   void* user) {
    if (sess_) throw std::runtime_error("EINVAL: a decode session is open on this engine (close it before generate)");
    timings_ = Timings();
    timings_.pages = reqs.size();
    if (p.lp_k > LP_MAX_TOP) throw std::runtime_error("EINVAL: at most 20 alternatives per token (DSOCR_MAX_TOP_LOGPROBS)");
    if (p.lp_k >= 0 && !p.use_cache) throw std::runtime_error("EINVAL: log-probabilities need the K/V cache (use_cache = 1)");
    last_lp_ = LogprobRows();
    last_stop_hits_.clear();
    last_guided_.clear();
    // the controls: every check before any device work.  Each record, then what the call must offer the ones that are
    // on: the K/V cache, no logits trace, no persistent step.  (The blocks differ on purpose.  A bias is refused
    // under DSOCR_PERSIST only where the persistent step would really run: reset_decode_state.  No exported form
    // passes a trace together with a penalty record or a windowed ban, and none can with an automaton: the first two
    // checks guard the engine's own interface, the third does not exist.)
    unsigned on = 0;
    for (const GenRequest& rq : reqs) {
        rq.ctl.validate(cfg_.lang.vocab, p.ignore_eos ? -1 : p.eos);
        on |= rq.ctl.active();
    }
    const char* pe = getenv("DSOCR_PERSIST");
    const bool persist = pe && atoi(pe) != 0;  // (the switch itself, whether or not the step would fit this model and batch)
    const struct { unsigned bit; bool trace; const char *cache, *persist; } needs[] = {
        {Controls::BIAS, true, "EINVAL: a logit bias needs the K/V cache (use_cache = 1) and no logits trace", nullptr},
        {Controls::STOPS, true, "EINVAL: stop sequences need the K/V cache (use_cache = 1) and no logits trace",
         "EINVAL: stop sequences do not combine with the persistent decode step (DSOCR_PERSIST)"},
        {Controls::PEN, true, "EINVAL: penalties need the K/V cache (use_cache = 1) and no logits trace",
         "EINVAL: penalties do not combine with the persistent decode step (DSOCR_PERSIST)"},
        {Controls::NGW, true, "EINVAL: a windowed n-gram ban needs the K/V cache (use_cache = 1) and no logits trace",
         "EINVAL: a windowed n-gram ban does not combine with the persistent decode step (DSOCR_PERSIST)"},
        {Controls::GUIDED, false, "EINVAL: a token automaton needs the K/V cache (use_cache = 1)",
         "EINVAL: a token automaton does not combine with the persistent decode step (DSOCR_PERSIST)"},
    };
    for (const auto& c : needs) {
        if (!(on & c.bit)) continue;
        if (!p.use_cache || (c.trace && p.trace)) throw std::runtime_error(c.cache);
        if (c.persist && persist) throw std::runtime_error(c.persist);
    }
    if (reqs.empty() || p.max_new == 0) return std::vector<std::vector<int64_t>>(reqs.size());
    ensure_small(std::max((int)reqs.size(), 64));
    GenState g(reqs, p, cb, user);
    // what a running generate sets for decode_step / decode_head is back to idle on every exit, a throw included
    // (profile_decode runs unstamped; every later generate is stamped again while span_mode_ is set)
    ScopedSet idle_chain(chain_active_, false);
    ScopedSet idle_rec(span_rec_, nullptr);
    ScopedSet idle_step(span_step_, nullptr);
    ScopedSet idle_slots(span_slots_, nullptr);
    ScopedSet idle_trace(trace_, nullptr);
    hipStream_t st = stream_;
    HIP_CHECK(hipEventRecord(g.ev[0], st));
    flops_acc_ = 0;
    embed_pages(g);
    HIP_CHECK(hipEventRecord(g.ev[1], st));
    timings_.vision_flops = flops_acc_;
    plan_image_rows(g);
    reset_decode_state(g);
    HIP_CHECK(hipEventRecord(g.ev[2], st));
    flops_acc_ = 0;
    forward_rows(g, g.prompt_len);
    init_sampling(g);
    HIP_CHECK(hipEventRecord(g.ev[3], st));
    timings_.prefill_flops = flops_acc_;
    g.pin = PinnedBuffer<int>(3 * g.B + 1);
    if (cb && g.B == 1) {
        poll(g);
        if (g.pin[g.B] > 0) stream_tokens(g, g.pin[g.B]);
    }
    if (p.use_cache) decode_cached(g);
    else decode_uncached(g);
    return collect_outputs(g);
}

// ---------------- 1. vision (compute_image_embeddings, batched over pages): g.gpost / g.lpost
void Engine::embed_pages(GenState& g) {
    const std::vector<GenRequest>& reqs = g.reqs;
    const int B = g.B, H = cfg_.lang.hidden;
    hipStream_t st = stream_;
    g.prompt_len.resize(B);
    for (int b = 0; b < B; ++b) {
        g.prompt_len[b] = (int)reqs[b].ids.size();
        if (g.prompt_len[b] == 0) throw std::runtime_error("EINVAL: empty prompt");
        g.max_p = std::max(g.max_p, g.prompt_len[b]);
    }
    // group pages by global/tile size
    std::map<int, std::vector<int>> gsz, tsz;
    for (int b = 0; b < B; ++b)
        if (reqs[b].page) {
            check_page_variant(*reqs[b].page);
            gsz[reqs[b].page->gsize].push_back(b);
            if (reqs[b].page->n_tiles > 0) tsz[reqs[b].page->tile].push_back(b);
        }
    g.gpost.assign(B, nullptr);
    g.lpost.assign(B, nullptr);
    int pass_id = 0;
    // pixels of one size group as one contiguous device batch: device-to-device gathers of
    // HBM-resident pages (dsocr_page_to_device / dsocr_prepare_page_device), host uploads otherwise
    auto gather = [&](const std::vector<int>& pages, bool tiles, size_t n_floats) -> float* {
        float* d = wsf("g_img" + std::to_string(pass_id++), n_floats);
        if (vis_stage_ > 1) return d;  // (a later stage of a sliced admission: the SAM slice gathered the pixels)
        size_t off = 0;
        bool host_copy = false;
        for (int b : pages) {
            const PagePixels& pg = *reqs[b].page;
            const size_t nf = tiles ? (size_t)pg.n_tiles * 3 * pg.tile * pg.tile : (size_t)3 * pg.gsize * pg.gsize;
            const float* dev = tiles ? pg.tiles_dev : pg.global_dev;
            const std::vector<float>& host = tiles ? pg.tiles_chw : pg.global_chw;
            if (dev && pg.dev_ordinal == device_) {
                HIP_CHECK(hipMemcpyAsync(d + off, dev, nf * 4, hipMemcpyDeviceToDevice, st));
            } else if (host.size() == nf) {
                HIP_CHECK(hipMemcpyAsync(d + off, host.data(), nf * 4, hipMemcpyHostToDevice, st));
                host_copy = true;
            } else {
                throw std::runtime_error("EINVAL: page pixels live on another device");
            }
            off += nf;
        }
        if (off != n_floats) throw std::runtime_error("EINTERNAL: pixel batch size mismatch");
        if (host_copy) HIP_CHECK(hipStreamSynchronize(st));  // host sources may be pageable temporaries
        return d;
    };
    // every pixel batch gathered first, then the passes: odd passes on the second vision stream
    // (DSOCR_VIS_STREAMS=0: all on one stream), joined before the image rows are assembled
    std::vector<float*> g_img, t_img;
    std::vector<int> t_n;
    for (auto& kv : gsz) g_img.push_back(gather(kv.second, false, kv.second.size() * 3 * (size_t)kv.first * kv.first));
    for (auto& kv : tsz) {
        int n = 0;
        for (int b : kv.second) n += reqs[b].page->n_tiles;
        t_img.push_back(gather(kv.second, true, (size_t)n * 3 * kv.first * kv.first));
        t_n.push_back(n);
    }
    const bool two = vis_streams_on() && gsz.size() + tsz.size() >= 2;
    if (two && !vstream_) {
        HIP_CHECK(hipStreamCreateWithFlags(&vstream_, hipStreamNonBlocking));
        for (auto& e : vis_ev_) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));  // (freed in ~Engine)
    }
    if (two) {
        HIP_CHECK(hipEventRecord(vis_ev_[0], st));  // pixels gathered
        HIP_CHECK(hipStreamWaitEvent(vstream_, vis_ev_[0], 0));
    }
    int vis_k = 0;
    bool side = false;
    auto run_pass = [&](float* dimg, int n, int S) -> float* {
        const std::string name = "vis_out" + std::to_string(vis_k);
        if (!two || (vis_k++ & 1) == 0) return vision_pass(dimg, n, S, name);
        // this pass alone on the second stream, with that stream's own workspaces
        const hipStream_t first = stream_;
        ScopedSet on_side(stream_, vstream_), off_side(vstream_, first);
        ScopedSet prefix(ws_prefix_, "vs1_");
        side = true;
        return vision_pass(dimg, n, S, name);
    };
    size_t gi = 0, ti = 0;
    for (auto& kv : gsz) {
        const int S = kv.first, Sq = (S / 64) * (S / 64);
        float* post = run_pass(g_img[gi++], (int)kv.second.size(), S);
        for (size_t i = 0; i < kv.second.size(); ++i) g.gpost[kv.second[i]] = post + (size_t)i * Sq * H;
    }
    for (auto& kv : tsz) {
        const int S = kv.first, Sq = (S / 64) * (S / 64);
        float* post = run_pass(t_img[ti], t_n[ti], S);
        ++ti;
        size_t off = 0;
        for (int b : kv.second) {
            g.lpost[b] = post + off * Sq * H;
            off += reqs[b].page->n_tiles;
        }
    }
    if (side) {
        HIP_CHECK(hipEventRecord(vis_ev_[1], vstream_));
        HIP_CHECK(hipStreamWaitEvent(st, vis_ev_[1], 0));
    }
}

// ---------------- 2. image rows for the injection (model/mod.rs:1208-1239): g.host_rows (kind ROW_HOST),
// g.vis_rows (one contiguous device buffer of every page's vision rows, to keep the assemble kernel simple)
// and g.img; checks every prompt against its mask and the vocabulary
void Engine::plan_image_rows(GenState& g) {
    const std::vector<GenRequest>& reqs = g.reqs;
    const int B = g.B, H = cfg_.lang.hidden;
    hipStream_t st = stream_;
    std::vector<long> host_row_base(B, 0);
    for (int b = 0; b < B; ++b)
        if (!reqs[b].page && reqs[b].image_rows) {
            host_row_base[b] = (long)(g.host_rows.size() / H);
            g.host_rows.insert(g.host_rows.end(), reqs[b].image_rows, reqs[b].image_rows + reqs[b].n_image_rows * H);
        }
    long vis_rows_total = 0;
    std::vector<long> vis_base(B, 0), vis_local_rows(B, 0), vis_global_rows(B, 0);
    for (int b = 0; b < B; ++b)
        if (const PagePixels* pg = reqs[b].page) {
            vis_base[b] = vis_rows_total;
            vis_local_rows[b] = (long)pg->n_tiles * (pg->tile / 64) * (pg->tile / 64);
            vis_global_rows[b] = (long)(pg->gsize / 64) * (pg->gsize / 64);
            vis_rows_total += vis_local_rows[b] + vis_global_rows[b];
        }
    g.vis_rows = wsf("g_visrows", (size_t)std::max<long>(vis_rows_total, 1) * H);
    for (int b = 0; b < B; ++b)
        if (reqs[b].page) {
            if (vis_local_rows[b])
                HIP_CHECK(hipMemcpyAsync(g.vis_rows + vis_base[b] * H, g.lpost[b], vis_local_rows[b] * H * 4,
                                         hipMemcpyDeviceToDevice, st));
            HIP_CHECK(hipMemcpyAsync(g.vis_rows + (vis_base[b] + vis_local_rows[b]) * H, g.gpost[b],
                                     vis_global_rows[b] * H * 4, hipMemcpyDeviceToDevice, st));
        }
    // image-row sequence of every page (assemble_artifacts order, model/mod.rs:879-923)
    g.img.resize(B);
    for (int b = 0; b < B; ++b) {
        const GenRequest& rq = reqs[b];
        if (rq.page) {
            g.img[b] = image_row_order(*rq.page);
            for (auto& r : g.img[b])
                if (r.first == ROW_VISION) r.second += vis_base[b];
        } else if (rq.image_rows) {
            for (size_t i = 0; i < rq.n_image_rows; ++i) g.img[b].push_back({ROW_HOST, host_row_base[b] + (long)i});
        }
        size_t n_mask = 0;
        for (int i = 0; i < g.prompt_len[b]; ++i) n_mask += (!rq.mask.empty() && rq.mask[i]) ? 1 : 0;
        if (n_mask != g.img[b].size())
            throw std::runtime_error("EINVAL: prompt/image embedding mismatch: image embeddings provide " +
                                     std::to_string(g.img[b].size()) + " tokens but mask requires " + std::to_string(n_mask));
        for (int i = 0; i < g.prompt_len[b]; ++i)
            if ((rq.mask.empty() || !rq.mask[i]) && (rq.ids[i] < 0 || rq.ids[i] >= cfg_.lang.vocab))
                throw std::runtime_error("EINVAL: token id out of bounds for vocab size");
    }
}

// the decode rows of this call: a KV cache and context rows of prompt + max_new + 1 rows per page, nothing zero-filled
// (init_sampling uploads the rows after the prefill), the scratch and rows only that its selection needs
void Engine::reset_decode_state(GenState& g) {
    const GenParams& p = g.p;
    const int B = g.B;
    DecodeRowsSpec spec;
    spec.rows = B; spec.Lcap = g.max_p + (int)p.max_new + 1; spec.ctx_cap = spec.Lcap; spec.out_cap = (long)p.max_new;
    spec.sampler = p.do_sample;
    // what the requests' controls ask for, in one pass: the rows of each control some page carries, one staging
    // region per list / automaton / stop set, automaton tables sized for the call's largest
    bool exact = false;
    for (const GenRequest& rq : g.reqs) {
        const Controls& c = rq.ctl;
        exact = exact || c.needs_exact_head();
        if (c.bias.active()) { spec.bias = true; spec.bias_stage += c.bias.ids.size(); }
        if (c.stops.active()) { spec.stops = true; spec.stop_stage_rows = B; }
        spec.penalties = spec.penalties || c.pen.active();
        spec.ngram_window = spec.ngram_window || c.ngw.active();
        if (c.guided.active()) {
            if (!spec.guided) { spec.guided = true; spec.guided_states = 1; spec.guided_edges = 1; }
            spec.guided_states = std::max(spec.guided_states, c.guided.n_states);
            spec.guided_edges = std::max(spec.guided_edges, c.guided.edges());
            spec.guided_stage += guided_stage_ints(c.guided.n_states, c.guided.edges());
        }
    }
    // the screened head (exact lm_head instead while sampling, tracing, keeping log-probabilities, or with a control
    // that acts on the logits row; a stop set runs under whichever head runs without it)
    spec.ban = !p.do_sample && !p.trace && p.lp_k < 0 && !exact && screen_applies(B, p.rep_penalty);
    // (the side row: dec_lp_final takes an emitted token's raw logit from it wherever a penalty may have rewritten
    // logits[tok]: the repetition penalty at the context ids, the frequency / presence penalty at the generated ones,
    // which the context row holds as well)
    spec.lp_k = p.lp_k; spec.lp_side = rep_penalty_active(p.rep_penalty) || spec.penalties;
    ensure_rope(spec.Lcap + 1);
    reserve_decode_rows(spec);
    // one page: the persistent decode step (its granules: no tag of an earlier generate may match this one's)
    persist_active_ = p.use_cache && persist_ok(B, spec.Lcap);
    if (persist_active_ && spec.bias) {
        persist_active_ = false;
        throw std::runtime_error("EINVAL: a logit bias does not combine with the persistent decode step (DSOCR_PERSIST)");
    }
    if (persist_active_) {
        ensure_persist();
        HIP_CHECK(hipMemsetAsync(persist_g_, 0xff, dec_persist_granules(cfg_.lang.layers) * 8, stream_));
    }
    g.extra.resize(B);
}

// ---------------- 3. the forward over whole token sequences (DeepseekOcrModel::forward,
// model/mod.rs:1181-1251): embed + inject (1208-1239), every layer, final norm + lm_head on the
// last row of each page (the reference projects every position, transformer/model.rs:243-270;
// only the last row is ever read).  The prefill runs it once on the prompts; use_cache = false
// (generate_without_cache, model/mod.rs:2051-2283) re-runs it on prompt + generated (g.extra) every step.
void Engine::forward_rows(GenState& g, const std::vector<int>& lens, const std::vector<int>& past, int row0, bool head,
                          bool chunk_attn) {
    const LangConfig& L = cfg_.lang;
    const int B = g.B, H = L.hidden, QKVN = layers_[0].qkv.N;
    hipStream_t st = stream_;
    ScopedSet page0(kv_page0_, row0);
    float* SX = rows_.x + (size_t)row0 * H;
    const PrefillPlan plan = prefill_row_plan(lens, QKVN, H, page_stride_, past);
    const long Tn = plan.T;
    const int maxl = plan.max_len;
    prefill_lens_ = lens;
    std::vector<int> kind(Tn), index(Tn);
    long r0 = 0;
    for (int b = 0; b < B; ++b) {
        const GenRequest& rq = g.reqs[b];
        const int plen = g.prompt_len[b];
        // the image rows before the first row of this call (behind a prefix entry there are none from past[b] on:
        // session_admit_prefix checks it, and g.img is empty; a chunk of a sliced admission starts among them)
        size_t j = 0;
        if (!past.empty() && !rq.mask.empty() && !g.img[b].empty())
            for (int i = 0; i < past[b] && i < plen; ++i) j += rq.mask[i] ? 1 : 0;
        for (int i = past.empty() ? 0 : past[b], end = i + lens[b]; i < end; ++i) {
            const long r = r0 + i - (past.empty() ? 0 : past[b]);
            if (i < plen && !rq.mask.empty() && rq.mask[i]) {
                kind[r] = g.img[b][j].first;
                index[r] = (int)g.img[b][j].second;
                ++j;
            } else {
                kind[r] = ROW_TOKEN;
                index[r] = i < plen ? rq.ids[i] : g.extra[b][i - plen];
            }
        }
        r0 += lens[b];
    }
    float* X = wsf("d_x", (size_t)Tn * H);
    int* dk = upload("g_kind", kind);
    int* di = upload("g_index", index);
    float* hr = g.host_rows.empty() ? nullptr : upload("g_hostrows", g.host_rows);
    launch_assemble_rows(dk, di, (int)Tn, H, embed_, embed_dt_, hr, g.vis_rows, newline_, separator_, X, H, st);
    int* d_row_page = upload("g_rowpage", plan.row_page);
    int* d_row_pos = upload("g_rowpos", plan.row_pos);
    long* d_q_off = upload("g_qoff", plan.q_off);
    long* d_kv_off = upload("g_kvoff", plan.kv_off);
    long* d_o_off = upload("g_ooff", plan.o_off);
    int* d_plen = upload("g_plen", lens);
    // every past == 0 is the plain prefill: the same launches, workspaces and order as without the argument
    const bool behind = std::any_of(past.begin(), past.end(), [](int p) { return p > 0; });
    const int* d_past = behind ? upload("g_past", past) : nullptr;
    for (int l = 0; l < L.layers; ++l)
        layer_forward_prefill(l, (int)Tn, B, d_row_page, d_row_pos, d_q_off, d_kv_off, d_o_off, d_plen, maxl, rows_.Lcap,
                              d_past, plan.max_total, chunk_attn);
    if (!head) return;  // (a chunk before the prompt's last: nobody reads its last row's logits)
    std::vector<int> last_rows(B), lr_kind(B, ROW_HOST);
    r0 = 0;
    for (int b = 0; b < B; ++b) { r0 += lens[b]; last_rows[b] = (int)(r0 - 1); }
    int* lk = upload("g_lrkind", lr_kind);
    int* li = upload("g_lrindex", last_rows);
    launch_assemble_rows(lk, li, B, H, nullptr, 0, X, nullptr, nullptr, nullptr, SX, H, st);
    float* SXN = wsf("s_xn", (size_t)B * H);
    launch_rmsnorm(SX, H, SXN, H, B, H, final_norm_, L.rms_eps, st);
    linear(SXN, B, H, lm_head_, rows_.logits + (size_t)row0 * L.vocab, L.vocab);
}

// sampling state (context = prompt ids (+ generated), sampling.rs:34-96), then the prefill's own selection:
// the first token of every page
void Engine::init_sampling(GenState& g) {
    const LangConfig& L = cfg_.lang;
    const GenParams& p = g.p;
    const int B = g.B;
    const DecodeRows& r = rows_;
    hipStream_t st = stream_;
    const long ctx_cap = r.ctx_cap;
    std::vector<int> ctx((size_t)B * ctx_cap, 0), zeros(B, 0);
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < g.prompt_len[b]; ++i) ctx[(size_t)b * ctx_cap + i] = g.reqs[b].ids[i];
    g.kvpos = g.prompt_len;
    g.kvlen = g.prompt_len;
    for (int& v : g.kvlen) ++v;
    upload_to(r.ctx, "s_ctx_ids", ctx);
    upload_to(r.ctx_len, "s_ctx_len", g.prompt_len);
    HIP_CHECK(hipMemcpyAsync(r.kv_pos, g.kvpos.data(), B * 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(r.kv_len, g.kvlen.data(), B * 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    upload_to(r.done, "s_done", zeros);
    upload_to(r.out_len, "s_outlen", zeros);
    if (p.do_sample) {
        // StdRng::seed_from_u64(seed) per page — every page starts from init_rng(seed) like a single-page
        // generate call (model/mod.rs:1917) — or entropy
        uint64_t seed = p.seed;
        if (!p.seed_set) {
            std::random_device rd;
            seed = ((uint64_t)rd() << 32) ^ rd();
        }
        const std::vector<uint32_t> rng = rng_state_from_u64(seed);
        std::vector<uint32_t> all((size_t)B * RNG_WORDS);
        for (int b = 0; b < B; ++b) memcpy(&all[(size_t)b * RNG_WORDS], rng.data(), sizeof(uint32_t) * RNG_WORDS);
        upload_to(r.rng, "s_rng", all);
    }
    // penalty (applied in place to the logits when != 1) + fused greedy selection
    SampleArgs pen;
    DecSampleArgs sa;
    sample_args(B, 0, p, false, sa, pen);
    ensure_mm_weights(B);
    if (r.ban) {  // the screened head
        reserve_head_ws(B);
        if (getenv("DSOCR_SCREEN_STATS")) HIP_CHECK(hipMemsetAsync(wsi("s_scrstats", 32), 0, 128, st));
    }
    // parity trace: the raw logits of every step of every page ([B][max_new][V], index = tokens
    // emitted so far), copied before the repetition penalty like the reference's debug dump
    // (crates/infer-deepseek/src/debug.rs) — the exact lm_head runs (no screening) while tracing
    trace_ = p.trace ? wsf("s_trace", (size_t)B * p.max_new * L.vocab) : nullptr;
    trace_steps_ = (long)p.max_new;
    if (trace_) {
        HIP_CHECK(hipMemsetAsync(trace_, 0, sizeof(float) * B * p.max_new * L.vocab, st));
        launch_trace_logits(r.logits, B, L.vocab, L.vocab, r.out_len, r.done, trace_, trace_steps_, st);
    }
    // every page's controls, then the prefill's own selection: the first token of every page (with log-probabilities:
    // an entry for it too).  The fused selection kernel advances the KV position; after the prefill the first decode
    // position must be P, so it starts one behind (no launch of the tail before it reads kv_pos / kv_len)
    write_controls(g.reqs.data(), 0, B, p.ignore_eos ? -1 : p.eos);
    std::vector<int> pm1(B), lm1(B);
    for (int b = 0; b < B; ++b) { pm1[b] = g.kvpos[b] - 1; lm1[b] = g.kvlen[b] - 1; }
    HIP_CHECK(hipMemcpyAsync(r.kv_pos, pm1.data(), B * 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(r.kv_len, lm1.data(), B * 4, hipMemcpyHostToDevice, st));
    const DecLpArgs lp = p.lp_k >= 0 ? lp_args(sa, 0) : DecLpArgs();
    TailPlan t;
    t.bias = r.bias != nullptr; t.guided = r.g_on != nullptr; t.penalties = r.pen != nullptr; t.stops = r.stop_tab != nullptr;
    t.window = r.ngw ? p.ngram : -1;
    t.lp = p.lp_k >= 0 ? &lp : nullptr;
    selection_tail(sa, pen, 0, t);
    HIP_CHECK(hipStreamSynchronize(st));
}

// done flags, output lengths and the last tokens of every page into g.pin; true when every page is done
bool Engine::poll(GenState& g) {
    const int B = g.B;
    HIP_CHECK(hipMemcpyAsync(g.pin, rows_.done, B * 4, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipMemcpyAsync(g.pin + B, rows_.out_len, B * 4, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipMemcpyAsync(g.pin + 2 * B, rows_.tok, B * 4, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    bool all = true;
    for (int b = 0; b < B; ++b) all &= g.pin[b] != 0;
    return all;
}

// stream callback with the n tokens so far (B = 1; model/mod.rs:1980-1982 calls it after every token)
void Engine::stream_tokens(GenState& g, int n) {
    if (n <= g.streamed) return;  // no new token (EOS selected, or the page is done)
    g.streamed = n;
    std::vector<int> tmp(n);
    if (n) HIP_CHECK(hipMemcpy(tmp.data(), rows_.out, n * 4, hipMemcpyDeviceToHost));
    std::vector<int64_t> t64(tmp.begin(), tmp.end());
    g.cb(t64.size(), t64.data(), g.user);
}

// ---------------- 4'. generate_without_cache (model/mod.rs:2051-2283): every step re-runs the
// whole forward on prompt + generated tokens (image rows re-injected at the same slots), then
// the same selection / bookkeeping kernels as the cached loop
void Engine::decode_uncached(GenState& g) {
    const int B = g.B, V = cfg_.lang.vocab;
    hipStream_t st = stream_;
    HIP_CHECK(hipEventRecord(g.ev[4], st));
    std::vector<int> lens = g.prompt_len;
    SampleArgs pen;
    DecSampleArgs sa;
    sample_args(B, 0, g.p, false, sa, pen);
    for (size_t i = 1; i < g.p.max_new; ++i) {
        if (poll(g)) break;
        for (int b = 0; b < B; ++b)
            if (!g.pin[b]) { g.extra[b].push_back(g.pin[2 * B + b]); ++lens[b]; }
        forward_rows(g, lens);
        if (trace_) launch_trace_logits(rows_.logits, B, V, V, rows_.out_len, rows_.done, trace_, trace_steps_, st);
        launch_rep_penalty(pen, st);
        launch_dec_sample(sa, st);
        ++g.steps;
        if (g.cb && B == 1) {
            poll(g);
            stream_tokens(g, g.pin[B]);
        }
    }
    HIP_CHECK(hipEventRecord(g.ev[5], st));
    HIP_CHECK(hipStreamSynchronize(st));
}

// launch spans (set_spans): this generate's record buffers; span_rec_ marks it as stamped
void Engine::begin_spans(GenState& g) {
    const int layers = cfg_.lang.layers;
    hipStream_t st = stream_;
    spans_kinds_ = SPAN_KINDS;
    if (span_mode_ == SPAN_CHAIN) {
        span_cap_ = (int)std::max<size_t>(g.p.max_new, 1) + 1;  // the fold records at (tokens emitted) <= max_new
        const size_t nreg = (size_t)layers * SPAN_KINDS_CHAIN;
        span_chain_ = (unsigned long long*)ws("s_span_chain", nreg * SPAN_SLOTS * 16);
        span_chain_rec_ = (unsigned long long*)ws("s_span_chain_rec", (size_t)span_cap_ * nreg * 32);
        span_tmark_ = (unsigned long long*)ws("s_span_tmark", 16);
        span_rec_ = span_chain_rec_;
        span_step_ = rows_.out_len;
        chain_active_ = true;
        HIP_CHECK(hipMemsetAsync(span_chain_rec_, 0, (size_t)span_cap_ * nreg * 32, st));
    } else if (span_mode_) {
        span_cap_ = (int)std::max<size_t>(g.p.max_new, 1);
        const size_t rec_bytes = (size_t)SPAN_KINDS * layers * span_cap_ * 4 * 8;
        span_slots_ = (unsigned long long*)ws("s_span_slots", (size_t)SPAN_SLOTS * 16);
        span_rec_ = (unsigned long long*)ws("s_span_rec", rec_bytes);
        span_step_ = rows_.out_len;
        HIP_CHECK(hipMemsetAsync(span_slots_, 0, (size_t)SPAN_SLOTS * 16, st));
        HIP_CHECK(hipMemsetAsync(span_rec_, 0, rec_bytes, st));
        if (span_ev_.empty()) span_ev_.resize((size_t)SPAN_KINDS * layers * 2);
        span_ev_ns_.assign((size_t)SPAN_KINDS * layers * span_cap_, 0.0);
    }
}

// after a stamped step: the dispatch-level duration of every bracketed launch, at the step's index
void Engine::read_span_events(size_t step) {
    HIP_CHECK(hipEventSynchronize(span_ev_.back()));
    const size_t k = std::min(step, (size_t)span_cap_ - 1);
    for (size_t i = 0; i < (size_t)SPAN_KINDS * cfg_.lang.layers; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, span_ev_[2 * i], span_ev_[2 * i + 1]) == hipSuccess)
            span_ev_ns_[i * span_cap_ + k] = ms * 1e6;
        else
            (void)hipGetLastError();  // pair not recorded this step (e.g. the dense layer)
    }
}

// the stamped generate's records into spans_host_ (spans_steps_ is reported with the records it sizes)
void Engine::collect_spans() {
    const int layers = cfg_.lang.layers;
    if (chain_active_) {
        const size_t nreg = (size_t)layers * SPAN_KINDS_CHAIN;
        std::vector<unsigned long long> dev((size_t)span_cap_ * nreg * 4);
        HIP_CHECK(hipMemcpy(dev.data(), span_chain_rec_, dev.size() * 8, hipMemcpyDeviceToHost));
        spans_host_.assign((size_t)SPAN_KINDS_CHAIN * layers * span_cap_ * SPAN_FIELDS, 0);
        // fold at step s's end recorded at index (tokens emitted) = s + 1: shift back to s
        for (int s = 1; s < span_cap_; ++s)
            for (int l = 0; l < layers; ++l)
                for (int k = 0; k < SPAN_KINDS_CHAIN; ++k) {
                    const unsigned long long* r = &dev[((size_t)s * nreg + (size_t)l * SPAN_KINDS_CHAIN + k) * 4];
                    unsigned long long* o = &spans_host_[(((size_t)k * layers + l) * span_cap_ + s - 1) * SPAN_FIELDS];
                    o[0] = r[0]; o[1] = r[1]; o[3] = r[2];
                }
        spans_steps_ = span_cap_;
        spans_kinds_ = SPAN_KINDS_CHAIN;
    } else if (span_rec_) {
        const size_t nrec = (size_t)SPAN_KINDS * layers * span_cap_;
        std::vector<unsigned long long> dev(nrec * 4);
        HIP_CHECK(hipMemcpy(dev.data(), span_rec_, dev.size() * 8, hipMemcpyDeviceToHost));
        spans_host_.assign(nrec * SPAN_FIELDS, 0);
        for (size_t r = 0; r < nrec; ++r) {
            for (int f = 0; f < 4; ++f) spans_host_[r * SPAN_FIELDS + f] = dev[r * 4 + f];
            if (span_mode_ & SPAN_EVENTS) spans_host_[r * SPAN_FIELDS + 4] = (unsigned long long)llround(span_ev_ns_[r]);
        }
        spans_steps_ = span_cap_;
    }
}

// one decode step: the layers, the head and the selection (captured once, replayed per token)
void Engine::step_body(GenState& g) {
    SampleArgs pen;
    DecSampleArgs sa;
    sample_args(g.B, 0, g.p, false, sa, pen);
    const DecLpArgs lp = g.p.lp_k >= 0 ? lp_args(sa, 0) : DecLpArgs();
    decode_step(g.B, rows_.Lcap);
    decode_head(g.B, sa, pen, rows_.ban != nullptr, g.p.lp_k >= 0 ? &lp : nullptr, rows_.stop_tab != nullptr,
                rows_.ngw ? g.p.ngram : -1);
    // chain spans: the step's one fold, after the head (the step counter has advanced: record at count - 1)
    if (chain_active_)
        launch_span_chain_fold(span_chain_, cfg_.lang.layers * SPAN_KINDS_CHAIN, span_chain_rec_, span_step_, span_cap_,
                               span_tmark_, stream_);
}

// ---------------- 4. decode loop (decode.iterative) as a replayed hipGraph (eager launches: graphs_on())
void Engine::decode_cached(GenState& g) {
    const LangConfig& L = cfg_.lang;
    const GenParams& p = g.p;
    const int B = g.B, H = L.hidden;
    hipStream_t st = stream_;
    begin_spans(g);
    // make sure every decode workspace exists before capture: a dry step allocates them
    // (it writes the step-0 K/V slot, which the real step rewrites), then the state is restored
    decode_step(B, rows_.Lcap);
    if (persist_active_) {  // the dry step's granules carry step 1's tags: reset them
        HIP_CHECK(hipMemsetAsync(persist_g_, 0xff, dec_persist_granules(L.layers) * 8, st));
        persist_stamps_host_.clear();
        persist_ev_us_.clear();
        if (persist_stamp_mode_) {
            persist_stamp_pos0_ = g.kvpos[0];
            persist_stamp_cap_ = (int)p.max_new;
            const size_t n = (size_t)persist_stamp_cap_ * PK_G * L.layers * PK_STAMPS;
            persist_stamps_ = (unsigned long long*)ws("p_pk_stamps", n * 8);
            HIP_CHECK(hipMemsetAsync(persist_stamps_, 0, n * 8, st));
        }
    }
    if (chain_active_) {  // the dry step's stamps must not join step 1's: clear the regions and the marks
        HIP_CHECK(hipMemsetAsync(span_chain_, 0, (size_t)L.layers * SPAN_KINDS_CHAIN * SPAN_SLOTS * 16, st));
        HIP_CHECK(hipMemsetAsync(span_tmark_, 0, 16, st));
    }
    HIP_CHECK(hipMemcpyAsync(rows_.kv_pos, g.kvpos.data(), B * 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(rows_.kv_len, g.kvlen.data(), B * 4, hipMemcpyHostToDevice, st));
    launch_embed_tokens(embed_, embed_dt_, rows_.tok, B, H, rows_.x, H, st);
    HIP_CHECK(hipStreamSynchronize(st));

    const bool use_graph = graphs_on();
    const bool pk_timed = persist_active_ && persist_stamp_mode_ && !span_rec_;
    if (pk_timed && persist_ev_.empty()) persist_ev_.resize(2);
    HipGraphExec gexec;
    if (use_graph && !pk_timed) {
        StreamCapture cap(st, capturing_);
        step_body(g);
        gexec = cap.finish();
    }
    HIP_CHECK(hipEventRecord(g.ev[4], st));
    // stop sets: a stop ends a page under ignore_eos too, so the done flags are polled at the usual cadence, and once
    // before the first step (a stop may have fired on the prefill's selection)
    // (an automaton ends its page the same way: complete or violated)
    const bool stop_rows = rows_.stop_tab != nullptr;
    const bool stops = stop_rows || rows_.g_on != nullptr;
    const bool finished = stops && poll(g);
    for (size_t i = 1; i < p.max_new && !finished; ++i) {
        if (gexec) gexec.launch(st);
        else step_body(g);
        if (gexec && stop_rows) ++stop_launches_;
        if (span_rec_ && (span_mode_ & SPAN_EVENTS)) read_span_events(i);
        if (pk_timed) {  // the persistent launch's dispatch duration (events recorded around it in the step)
            HIP_CHECK(hipEventSynchronize(persist_ev_[1]));
            float ms = 0.f;
            HIP_CHECK(hipEventElapsedTime(&ms, persist_ev_[0], persist_ev_[1]));
            persist_ev_us_.push_back(ms * 1e3);
        }
        ++g.steps;
        const bool check = g.cb != nullptr || ((!p.ignore_eos || stops) && (i % 8 == 0 || i + 1 == p.max_new));
        if (check) {
            const bool all = poll(g);
            if (g.cb && B == 1) stream_tokens(g, g.pin[B]);
            if (all) break;
        }
    }
    HIP_CHECK(hipEventRecord(g.ev[5], st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (pk_timed) {
        persist_stamps_host_.resize((size_t)persist_stamp_cap_ * PK_G * L.layers * PK_STAMPS);
        HIP_CHECK(hipMemcpy(persist_stamps_host_.data(), persist_stamps_, persist_stamps_host_.size() * 8,
                            hipMemcpyDeviceToHost));
        persist_stamp_mode_ = 0;
    }
    collect_spans();
}

// the decode error flag, the generated ids of every page and the stage timings (and the parity trace)
std::vector<std::vector<int64_t>> Engine::collect_outputs(GenState& g) {
    const GenParams& p = g.p;
    const int B = g.B;
    int e = 0;
    HIP_CHECK(hipMemcpy(&e, rows_.err, sizeof(int), hipMemcpyDeviceToHost));
    if (e) throw std::runtime_error("EINTERNAL: decode hand-off timed out inside a fused kernel");
    if (rows_.ban && getenv("DSOCR_SCREEN_STATS")) {
        unsigned long long h[16] = {0};
        HIP_CHECK(hipMemcpy(h, wsi("s_scrstats", 32), sizeof(h), hipMemcpyDeviceToHost));
        const double st = h[0] ? (double)h[0] : 1.0;
        fprintf(stderr, "[screen] steps %llu kept/step %.1f survivors/step %.2f phase_us", h[0], h[1] / st, h[2] / st);
        for (int k = 0; k < 7; ++k) fprintf(stderr, " %.2f", h[4 + k] / st / 100.0);  // wall clock: 100 MHz
        fprintf(stderr, "\n");
    }
    std::vector<int> h_out((size_t)B * p.max_new), h_outlen(B);
    HIP_CHECK(hipMemcpy(h_out.data(), rows_.out, h_out.size() * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(h_outlen.data(), rows_.out_len, B * 4, hipMemcpyDeviceToHost));
    std::vector<std::vector<int64_t>> out(B);
    for (int b = 0; b < B; ++b) out[b].assign(h_out.begin() + (size_t)b * p.max_new, h_out.begin() + (size_t)b * p.max_new + h_outlen[b]);
    timings_.vision_compute_ms = ms_between(g.ev[0], g.ev[1]);
    timings_.prefill_ms = ms_between(g.ev[2], g.ev[3]);
    timings_.iterative_ms = ms_between(g.ev[4], g.ev[5]);
    timings_.generate_ms = timings_.prefill_ms + timings_.iterative_ms;
    timings_.steps = g.steps;
    if (trace_ && p.trace)
        HIP_CHECK(hipMemcpy(p.trace, trace_, sizeof(float) * B * p.max_new * cfg_.lang.vocab, hipMemcpyDeviceToHost));
    if (p.lp_k >= 0) {  // the entries, once: a few bytes per token
        LogprobRows& r = last_lp_;
        r.K = p.lp_k; r.cap = p.max_new; r.n = h_outlen;
        r.lp.resize((size_t)B * r.cap);
        HIP_CHECK(hipMemcpy(r.lp.data(), rows_.lp, r.lp.size() * 4, hipMemcpyDeviceToHost));
        r.top_id.resize((size_t)B * r.cap * r.K);
        r.top_lp.resize(r.top_id.size());
        if (!r.top_id.empty()) {
            HIP_CHECK(hipMemcpy(r.top_id.data(), rows_.lp_top_id, r.top_id.size() * 4, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(r.top_lp.data(), rows_.lp_top, r.top_lp.size() * 4, hipMemcpyDeviceToHost));
        }
    }
    if (rows_.stop_tab) {
        last_stop_hits_.resize((size_t)B * 2);
        HIP_CHECK(hipMemcpy(last_stop_hits_.data(), rows_.stop_hit, (size_t)B * 2 * 4, hipMemcpyDeviceToHost));
    }
    if (rows_.g_on) {
        std::vector<int> st((size_t)B), stat((size_t)B);
        HIP_CHECK(hipMemcpy(st.data(), rows_.g_state, (size_t)B * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(stat.data(), rows_.g_status, (size_t)B * 4, hipMemcpyDeviceToHost));
        last_guided_.resize((size_t)B * 2);
        for (int b = 0; b < B; ++b) {  // (a page without an automaton: its words were never written past the zero fill)
            const bool on = g.reqs[b].ctl.guided.active();
            last_guided_[2 * b] = on ? st[b] : 0;
            last_guided_[2 * b + 1] = on ? stat[b] : 0;
        }
    }
    last_B_ = B;
    last_Lmax_ = rows_.Lcap;
    return out;
}

// ============================================================================ decode sessions
// A session keeps the decode state of up to S pages alive across calls.  Its step is decode_step + decode_head,
// unchanged, captured once per active count n; admission runs generate's own phases (embed_pages,
// plan_image_rows, forward_rows, the first selection) on one page, pointed at slot n of the session's rows.
Engine::Session& Engine::open_session() {
    if (!sess_) throw std::runtime_error("EINVAL: no decode session is open on this engine");
    return *sess_;
}

// a request's selection parameters as the device record the per-row kernels read (kernels.hpp RowParams)
static RowParams resolve_row_params(const GenParams& p) {
    RowParams r;
    r.do_sample = (p.do_sample && p.temperature > 0.0) ? 1 : 0;
    r.temperature = p.temperature; r.top_p = p.top_p; r.top_k = p.top_k;
    r.rep_penalty = rep_penalty_active(p.rep_penalty) ? p.rep_penalty : 1.0f;
    r.ngram = p.ngram;
    r.eos = p.ignore_eos ? -1 : (int)p.eos;
    return r;
}

void Engine::session_open(int S, int max_context, const GenParams& p, const SessionFeatures& feat) {
    if (sess_) throw std::runtime_error("EINVAL: a decode session is already open on this engine");
    if (S < 1 || S > 8) throw std::runtime_error("EINVAL: a session has 1..8 slots");
    if (!p.use_cache || p.trace) throw std::runtime_error("EINVAL: a session decodes with the K/V cache and without a logits trace");
    if (p.max_new == 0 || max_context < 3 || (size_t)max_context < p.max_new + 2)
        throw std::runtime_error("EINVAL: max_context must hold a prompt row, max_new_tokens and one more row");
    if (span_mode_ || persist_stamp_mode_) throw std::runtime_error("EINVAL: launch spans and persist stamps are off inside a session");
    const LangConfig& L = cfg_.lang;
    if (L.heads % L.kv_heads) throw std::runtime_error("EINVAL: num_attention_heads must be a multiple of num_key_value_heads");
    if (L.head_dim % 4) throw std::runtime_error("EINVAL: a session needs head_dim % 4 == 0");
    const int H = L.hidden;
    hipStream_t st = stream_;
    auto sp = std::make_unique<Session>();
    Session& s = *sp;
    s.S = S; s.max_context = max_context; s.p = p; s.feat = feat;
    // Capacity invariant.  The selection kernels advance kv_pos of every row on every step, done or not, so a
    // finished page that waits for the end of its burst keeps appending K/V rows.  A page is admitted only with
    // prompt + max_new + 1 <= max_context and produces its last token at kv_pos <= prompt + max_new - 1; it is
    // retired at the next burst boundary, at most kBurstCap steps later.  Every slot therefore has
    // max_context + kBurstCap rows, and session_step refuses (on the host, before any launch) a burst that would
    // take a slot's kv_pos past them.  The context row has the same length; the output row stops on the device
    // at out_cap (dec_sample: out_len < out_cap, n < ctx_cap).
    DecodeRowsSpec spec;
    spec.rows = S; spec.Lcap = max_context + Session::kBurstCap; spec.ctx_cap = spec.Lcap; spec.out_cap = (long)p.max_new;
    s.screened = !p.do_sample && !feat.per_request && !feat.logprobs;
    for (int n = 1; n <= S; ++n) s.screened = s.screened && screen_applies(n, p.rep_penalty);
    // per-request parameters: what both heads need at every n, so nothing grows after the freeze (any slot may
    // sample: the sampler's scratch and RNG rows for all of them; the ban rows are always kept and both final
    // kernels write them every step: either head can take over from the other at a step boundary)
    spec.sampler = p.do_sample || feat.per_request;
    spec.ban = s.screened || feat.per_request;
    spec.rowpar = true;
    spec.handoff_max = true;  // the step runs at every n <= S
    spec.zero_fill = true;    // the dry steps below read kv_pos 0 and a zero input row
    if (feat.logit_bias) {    // every slot's row, and one admission's list at a time (at most vocab pairs)
        spec.bias = true;
        spec.bias_stage = (size_t)L.vocab;
    }
    spec.stops = feat.stops;  // every slot's table, and one admission's list at a time
    spec.penalties = feat.penalties;  // every slot's record
    spec.ngram_window = feat.ngram_window;  // the same
    if (feat.guided) {  // every slot's tables at the caps, and one admission's automaton at a time
        spec.guided = true;
        spec.guided_stage = guided_stage_ints(GUIDED_MAX_STATES, GUIDED_MAX_EDGES);
    }
    if (feat.logprobs) {  // (the raw logits at the context ids too where a penalty can apply)
        spec.lp_k = LP_MAX_TOP;
        spec.lp_side = feat.per_request || rep_penalty_active(p.rep_penalty) || feat.penalties;
    }
    s.slot.resize(S);
    s.pin = PinnedBuffer<int>(2 * S + 1);
    ensure_small(64);
    ensure_rope(spec.Lcap + 1);
    const long head_stride0 = head_stride_, page_stride0 = page_stride_;
    try {
        kv_pages_ = S;
        kv_page0_ = 0;
        persist_active_ = false;  // (DSOCR_PERSIST is a generate-only switch)
        reserve_decode_rows(spec);
        {
            const std::vector<RowParams> init((size_t)S, resolve_row_params(p));
            HIP_CHECK(hipMemcpy(rows_.rowpar, init.data(), sizeof(RowParams) * S, hipMemcpyHostToDevice));
        }
        s.stage = wsi("ss_stage", (size_t)SS_HEAD + RNG_WORDS + rows_.ctx_cap);
        ensure_mm_weights(S);
        if (rows_.ban) {
            for (int n = 1; n <= S; ++n) reserve_head_ws(n);
            if (getenv("DSOCR_SCREEN_STATS")) HIP_CHECK(hipMemsetAsync(wsi("s_scrstats", 32), 0, sizeof(int) * 32, st));
        }
        // every workspace the decode step asks for by name, at every n: a dry step per n allocates them (it
        // appends K/V row 0 of the empty slots, which an admission's prefill rewrites)
        for (int n = 1; n <= S; ++n) {
            decode_step(n, rows_.Lcap);
            refill_handoffs();
        }
        HIP_CHECK(hipMemsetAsync(rows_.x, 0, sizeof(float) * S * H, st));
        HIP_CHECK(hipStreamSynchronize(st));
        // from here on no admission may move one of them: the captured graphs hold their addresses
        for (const auto& kv : ws_)
            if (kv.first.rfind("s_", 0) == 0 || kv.first.rfind("kv_", 0) == 0 || kv.first.rfind("p_", 0) == 0 ||
                kv.first.rfind("ss_", 0) == 0)
                ws_frozen_.insert(kv.first);
    } catch (...) {
        kv_pages_ = 0;
        ws_frozen_.clear();
        head_stride_ = head_stride0;
        page_stride_ = page_stride0;
        throw;
    }
    sess_ = std::move(sp);
}

int Engine::session_admit(const GenRequest& rq, size_t max_new, bool seed_set, uint64_t seed) {
    GenParams p = open_session().p;
    p.max_new = max_new; p.seed_set = seed_set; p.seed = seed;
    return session_admit(rq, p);
}

void Engine::session_admit_checks(const Session& s, const GenRequest& rq, const GenParams& rp, bool behind_prefix) const {
    const size_t max_new = rp.max_new;
    const int V = cfg_.lang.vocab;
    if (!rp.use_cache || rp.trace) throw std::runtime_error("EINVAL: a session decodes with the K/V cache and without a logits trace");
    if (!s.feat.per_request) {
        const GenParams& q = s.p;
        if (rp.do_sample != q.do_sample || rp.temperature != q.temperature || rp.top_p != q.top_p || rp.top_k != q.top_k ||
            rp.rep_penalty != q.rep_penalty || rp.ngram != q.ngram || rp.eos != q.eos || rp.ignore_eos != q.ignore_eos)
            throw std::runtime_error("EINVAL: this session's parameters are fixed (only max_new_tokens and the seed vary "
                                     "per request): open it with DSOCR_SESSION_PER_REQUEST");
    }
    rq.ctl.validate(V, rp.ignore_eos ? -1 : rp.eos);
    const struct { unsigned bit; bool have; const char* refusal; } feats[] = {
        {Controls::BIAS, s.feat.logit_bias, "EINVAL: this session was opened without DSOCR_SESSION_LOGIT_BIAS"},
        {Controls::STOPS, s.feat.stops, "EINVAL: this session was opened without DSOCR_SESSION_STOP"},
        {Controls::PEN, s.feat.penalties, "EINVAL: this session was opened without DSOCR_SESSION_PENALTIES"},
        {Controls::NGW, s.feat.ngram_window, "EINVAL: this session was opened without DSOCR_SESSION_NGRAM_WINDOW"},
        {Controls::GUIDED, s.feat.guided, "EINVAL: this session was opened without DSOCR_SESSION_GUIDED"},
    };
    for (const auto& f : feats)
        if ((rq.ctl.active() & f.bit) && !f.have) throw std::runtime_error(f.refusal);
    if (s.pending) throw std::runtime_error("EINVAL: a chunked admission is pending (advance it to the end or cancel it)");
    if (s.n >= s.S) throw std::runtime_error("EINVAL: every session slot is in use (retire one first)");
    const size_t P = rq.ids.size();
    if (P == 0) throw std::runtime_error("EINVAL: empty prompt");
    if (max_new == 0 || (long)max_new > rows_.out_cap)
        throw std::runtime_error("EINVAL: max_new_tokens must be 1.." + std::to_string(rows_.out_cap) + " in this session");
    if (P + max_new + 1 > (size_t)s.max_context)
        throw std::runtime_error("EINVAL: the page needs " + std::to_string(P + max_new + 1) +
                                 " context rows (prompt + max_new_tokens + 1), the session has " + std::to_string(s.max_context));
    if (!rq.mask.empty() && rq.mask.size() != P) throw std::runtime_error("EINVAL: image mask length differs from the prompt's");
    size_t rows = 0, n_mask = 0;
    if (rq.page) {
        check_page_variant(*rq.page);
        rows = image_row_order(*rq.page).size();
    } else if (rq.image_rows) {
        rows = rq.n_image_rows;
    }
    for (size_t i = 0; i < P; ++i) n_mask += (!rq.mask.empty() && rq.mask[i]) ? 1 : 0;
    if (behind_prefix) {  // its image rows are the entry's: the request brings none (the mask is checked against the entry)
        if (rq.page || rq.image_rows) throw std::runtime_error("EINVAL: a prefix admission carries no page and no image rows");
    } else if (n_mask != rows) {
        throw std::runtime_error("EINVAL: prompt/image embedding mismatch: image embeddings provide " + std::to_string(rows) +
                                 " tokens but mask requires " + std::to_string(n_mask));
    }
    for (size_t i = 0; i < P; ++i)
        if ((rq.mask.empty() || !rq.mask[i]) && (rq.ids[i] < 0 || rq.ids[i] >= V))
            throw std::runtime_error("EINVAL: token id out of bounds for vocab size");
}

int Engine::session_admit(const GenRequest& rq, const GenParams& rp) {
    Session& s = open_session();
    const size_t max_new = rp.max_new;
    // every check first: nothing below may fail on the request itself once device state changes
    session_admit_checks(s, rq, rp, false);
    const RowParams row = resolve_row_params(rp);
    const int slot = s.n;
    const std::vector<GenRequest> reqs{rq};
    GenParams gp = s.feat.per_request ? rp : s.p;
    gp.max_new = max_new;
    GenState g(reqs, gp, nullptr, nullptr);
    embed_pages(g);
    plan_image_rows(g);
    // the prefill of this page alone, into slot `slot` of the session cache and of the x / logits rows
    g.extra.resize(1);
    forward_rows(g, g.prompt_len, {}, slot);
    return session_admit_tail(s, rq, rp, row);
}

// the slot's rows in one launch from one staged buffer (the selection kernel advances the KV position, so it starts
// one behind: init_sampling), then the first selection on the logits the prefill left in the slot's s_logits row
int Engine::session_admit_tail(Session& s, const GenRequest& rq, const GenParams& rp, const RowParams& row_in, int at,
                               bool finish) {
    // a windowed ban replaces the page's plain one: its RowParams carry ngram 0 from here on
    RowParams row = row_in;
    const Controls& c = rq.ctl;
    const bool windowed = c.ngw.active();
    if (windowed) row.ngram = 0;
    const size_t max_new = rp.max_new, P = rq.ids.size();
    const bool seed_set = rp.seed_set;
    uint64_t seed = rp.seed;
    const int slot = at < 0 ? s.n : at;
    hipStream_t st = stream_;
    const size_t stage_ints = (size_t)SS_HEAD + RNG_WORDS + P;
    int* h = (int*)pinned("ss_stage", stage_ints * 4);
    std::memset(h, 0, ((size_t)SS_HEAD + RNG_WORDS) * 4);
    h[SS_CTX_LEN] = (int)P; h[SS_KV_POS] = (int)P - 1; h[SS_KV_LEN] = (int)P;
    if (s.feat.per_request ? row.do_sample != 0 : s.p.do_sample) {
        if (!seed_set) {
            std::random_device rd;
            seed = ((uint64_t)rd() << 32) ^ rd();
        }
        const std::vector<uint32_t> rng = rng_state_from_u64(seed);
        std::memcpy(h + SS_HEAD, rng.data(), sizeof(uint32_t) * RNG_WORDS);
    }
    if (s.feat.per_request) std::memcpy(h + SS_ROWPAR, &row, sizeof(RowParams));
    std::memcpy(h + SS_HEAD + RNG_WORDS, rq.ids.data(), P * 4);
    HIP_CHECK(hipMemcpyAsync(s.stage, h, stage_ints * 4, hipMemcpyHostToDevice, st));
    SlotInitArgs ia;
    const DecodeRows& r = rows_;
    ia.stage = s.stage; ia.slot = slot; ia.ctx = r.ctx; ia.ctx_cap = r.ctx_cap; ia.ctx_len = r.ctx_len;
    ia.kv_pos = r.kv_pos; ia.kv_len = r.kv_len; ia.done = r.done; ia.out_len = r.out_len; ia.tok = r.tok;
    ia.rng = r.rng; ia.rng_words = RNG_WORDS; ia.ban = r.ban; ia.ban_ld = r.ban_ld;
    if (s.feat.per_request) ia.rowpar = r.rowpar;
    DecSampleArgs sa;
    SampleArgs pen;
    sample_args(1, slot, s.p, s.feat.per_request, sa, pen);
    DecLpArgs lp;
    if (s.feat.logprobs) {  // (slot init takes the rows' bases)
        ia.lp = r.lp; ia.lp_top_id = r.lp_top_id; ia.lp_top = r.lp_top; ia.lp_k = r.lp_k; ia.out_cap = r.out_cap;
        lp = lp_args(sa, slot);
    }
    launch_session_slot_init(ia, st);
    // the slot's controls (none: the flag or count alone is cleared, or an off record written), then the first
    // selection on the prefill's logits: the first token, its embedding into the slot's s_x row, the ban list, entry 0
    // of the slot's log-probabilities.  The mask, the advance, the window ban and the match run only for a request that
    // carries the control
    write_controls(&rq, slot, 1, rp.ignore_eos ? -1 : rp.eos);
    TailPlan t;
    t.bias = s.feat.logit_bias; t.guided = c.guided.active(); t.penalties = s.feat.penalties; t.stops = c.stops.active();
    t.window = windowed ? 0 : -1;
    t.lp = s.feat.logprobs ? &lp : nullptr;
    selection_tail(sa, pen, slot, t);
    if (finish) {  // (else the caller has a launch to add before the one refill and synchronisation)
        refill_handoffs();
        HIP_CHECK(hipStreamSynchronize(st));
    }
    Session::Slot& sl = s.slot[slot];
    sl.max_new = max_new; sl.kv_pos = (int)P; sl.reported = 0; sl.rp = row; sl.prompt = (int)P;
    sl.ctl = c.active();
    sl.g_states = c.guided.n_states;
    sl.g_edges = c.guided.edges();
    sl.ids = rq.ids;
    sl.mask = rq.mask.empty() ? std::vector<uint8_t>(P, 0) : rq.mask;
    if (at < 0) ++s.n;
    return slot;
}

// ---- page prefix cache.  The copy both ways is launch_session_prefix_copy between the slot's cache rows and the
// entry's dense block; an entry never aliases a slot, so it survives the slot's retirement, moves and reuse.
static PrefixCopyArgs prefix_copy_args(const LangConfig& L, float* kc, float* vc, int S, int Lcap, long page_stride,
                                       long head_stride, int slot, int rows, float* entry, int to_slot) {
    PrefixCopyArgs c;
    c.kc = kc; c.vc = vc; c.layers = L.layers; c.slots = S; c.kv_heads = L.kv_heads; c.cap_rows = Lcap; c.hd = L.head_dim;
    c.layer_stride = (long)S * page_stride; c.page_stride = page_stride; c.head_stride = head_stride;
    c.slot = slot; c.rows = rows; c.to_slot = to_slot; c.entry = entry;
    return c;
}

int Engine::session_prefix_keep(int slot, int rows) {
    Session& s = open_session();
    if (slot < 0 || slot >= s.n) throw std::runtime_error("EINVAL: slot " + std::to_string(slot) + " is not active");
    const Session::Slot& sl = s.slot[slot];
    if (rows < 1 || rows > sl.prompt)
        throw std::runtime_error("EINVAL: a prefix has 1.." + std::to_string(sl.prompt) + " rows of this slot's prompt");
    if ((int)s.prefix.size() >= kMaxPrefixEntries)
        throw std::runtime_error("EINVAL: the session holds " + std::to_string(kMaxPrefixEntries) + " prefix entries (drop one first)");
    const LangConfig& L = cfg_.lang;
    Session::PrefixEntry e;
    e.kv = DeviceBuffer(session_prefix_floats(L.layers, L.kv_heads, rows, L.head_dim) * sizeof(float));  // ENOMEM
    e.rows = rows;
    e.ids.assign(sl.ids.begin(), sl.ids.begin() + rows);
    e.mask.assign(sl.mask.begin(), sl.mask.begin() + rows);
    launch_session_prefix_copy(prefix_copy_args(L, kc_, vc_, s.S, rows_.Lcap, page_stride_, head_stride_, slot, rows,
                                                (float*)e.kv.get(), 0), stream_);
    HIP_CHECK(hipStreamSynchronize(stream_));
    const int handle = s.next_handle++;
    s.prefix.emplace(handle, std::move(e));
    return handle;
}

int Engine::session_admit_prefix(int handle, const GenRequest& rq, const GenParams& rp) {
    Session& s = open_session();
    const LangConfig& L = cfg_.lang;
    // every check first: a refused admission changes nothing on the device
    const auto it = s.prefix.find(handle);
    if (it == s.prefix.end()) throw std::runtime_error("EINVAL: unknown prefix handle " + std::to_string(handle));
    const Session::PrefixEntry& e = it->second;
    session_admit_checks(s, rq, rp, true);
    const int P = (int)rq.ids.size(), rows = e.rows;
    if (P < rows + 1)
        throw std::runtime_error("EINVAL: the prompt must be longer than the prefix's " + std::to_string(rows) +
                                 " rows (the last row's logits come from a new row)");
    for (int i = 0; i < P; ++i) {
        const uint8_t m = rq.mask.empty() ? 0 : (rq.mask[i] ? 1 : 0);
        if (i < rows) {
            if (rq.ids[i] != e.ids[i] || m != (e.mask[i] ? 1 : 0))
                throw std::runtime_error("EINVAL: the prompt differs from the prefix entry at position " + std::to_string(i));
        } else if (m) {
            throw std::runtime_error("EINVAL: image position " + std::to_string(i) + " lies behind the prefix (the request carries no image rows)");
        }
    }
    const RowParams row = resolve_row_params(rp);
    const int slot = s.n;
    hipStream_t st = stream_;
    launch_session_prefix_copy(prefix_copy_args(L, kc_, vc_, s.S, rows_.Lcap, page_stride_, head_stride_, slot, rows,
                                                (float*)e.kv.get(), 1), st);
    const std::vector<GenRequest> reqs{rq};
    GenParams gp = s.feat.per_request ? rp : s.p;
    gp.max_new = rp.max_new;
    GenState g(reqs, gp, nullptr, nullptr);
    g.prompt_len = {P};
    g.max_p = P;
    g.img.resize(1);
    g.extra.resize(1);
    forward_rows(g, {P - rows}, {rows}, slot);  // the suffix alone, behind the copied rows
    const int got = session_admit_tail(s, rq, rp, row);
    ++s.prefix_admissions;
    s.prefix_rows_reused += (size_t)rows;
    return got;
}

// ---- chunked admission: session_admit's phases as slices, one per call, so that bursts of the running slots fit
// between them.  The page is staged in slot S - 1: active slots stay dense in [0, n) with n <= S - 1 while an
// admission is pending (no other admission can raise n), so no step, retire or compaction touches the staging
// slot's cache rows, and its per-slot rows are written only by the last slice.  When the last chunk's tail has made
// the first selection there, the page moves to slot n (launch_session_slot_move) unless n == S - 1.  Everything a
// slice leaves behind for the next lives in the staging slot's cache rows and in g_visrows, which only admissions
// write; cancelling therefore only forgets the host state.
struct Engine::PendingAdmit {
    std::vector<GenRequest> reqs;    // the request (ids, mask; image rows re-pointed at `rows`), what `g` refers to
    std::vector<float> rows;         // caller-supplied image rows, copied at begin
    GenParams gp, rp;
    RowParams row;
    std::unique_ptr<GenState> g;
    int chunk = 0, done = 0, total = 0, slices = 0, ticket = 0;
    bool vision = false;             // vision slices are still to run
    bool split = false;              // ... one per stage (vstage = the next: 1 SAM, 2 CLIP / encoder, 3 projector)
    int vstage = 1;
    bool planned = false;            // plan_image_rows has run
};

int Engine::session_admit_begin(const GenRequest& rq, const GenParams& rp, int chunk_rows) {
    Session& s = open_session();
    // every check first; nothing is launched here
    session_admit_checks(s, rq, rp, false);  // (a pending admission and a full session among them)
    if (chunk_rows < 32) throw std::runtime_error("EINVAL: a prefill chunk has at least 32 rows");
    auto pa = std::make_shared<PendingAdmit>();
    pa->reqs.push_back(rq);
    if (!rq.page && rq.image_rows) {
        pa->rows.assign(rq.image_rows, rq.image_rows + rq.n_image_rows * (size_t)cfg_.lang.hidden);
        pa->reqs[0].image_rows = pa->rows.data();
    }
    pa->rp = rp;
    pa->row = resolve_row_params(rp);
    pa->gp = s.feat.per_request ? rp : s.p;
    pa->gp.max_new = rp.max_new;
    pa->g = std::make_unique<GenState>(pa->reqs, pa->gp, nullptr, nullptr);
    pa->g->extra.resize(1);
    pa->chunk = chunk_rows;
    pa->total = (int)rq.ids.size();
    pa->vision = rq.page != nullptr;
    // The stages can run one per call when every vision pass keeps its own workspaces between calls: one pass (no
    // tiles), or two on the two vision streams (the second under the vs1_ prefix).  With DSOCR_VIS_STREAMS=0 both
    // passes of a tiled page share the v_* / c_* workspaces, and vision stays one slice.
    pa->split = pa->vision && (rq.page->n_tiles == 0 || vis_streams_on());
    pa->ticket = s.next_ticket++;
    s.pending = std::move(pa);
    return s.pending->ticket;
}

bool Engine::session_admit_advance(int* slot_out) {
    Session& s = open_session();
    if (!s.pending) throw std::runtime_error("EINVAL: no chunked admission is pending");
    PendingAdmit& pa = *s.pending;
    GenState& g = *pa.g;
    const int stage = s.S - 1;
    hipStream_t st = stream_;
    try {
        if (pa.vision) {  // SAM, then CLIP / the OCR2 encoder, then projector + plan_image_rows (or all in one)
            {
                ScopedSet stage(vis_stage_, pa.split ? pa.vstage : 0);
                embed_pages(g);
            }
            if (!pa.split || pa.vstage == 3) {
                plan_image_rows(g);
                pa.planned = true;
                pa.vision = false;
            }
            ++pa.vstage;
            HIP_CHECK(hipStreamSynchronize(st));
            ++pa.slices;
            return false;
        }
        if (!pa.planned) {  // no page: host work only (the prompt length, the caller's image rows), and g_visrows
            embed_pages(g);
            plan_image_rows(g);
            pa.planned = true;
        }
        const int len = std::min(pa.chunk, pa.total - pa.done);
        const bool last = pa.done + len == pa.total;
        // the first chunk is the plain causal prefill of its rows; the others attend behind the rows already appended
        if (pa.done == 0) forward_rows(g, {len}, {}, stage, last, true);
        else forward_rows(g, {len}, {pa.done}, stage, last, true);
        pa.done += len;
        ++pa.slices;
        if (!last) {
            HIP_CHECK(hipStreamSynchronize(st));
            return false;
        }
        session_admit_tail(s, pa.reqs[0], pa.rp, pa.row, stage, false);
        const int slot = s.n;
        if (slot != stage) session_slot_move(s, stage, slot, std::min(pa.total + 1, rows_.Lcap));
        refill_handoffs();
        HIP_CHECK(hipStreamSynchronize(st));
        ++s.n;
        s.pending.reset();
        if (slot_out) *slot_out = slot;
        return true;
    } catch (...) {
        s.pending.reset();  // a failed slice ends the admission; the running slots are as they were
        throw;
    }
}

void Engine::session_admit_cancel() {
    Session& s = open_session();
    if (!s.pending) throw std::runtime_error("EINVAL: no chunked admission is pending");
    HIP_CHECK(hipStreamSynchronize(stream_));
    s.pending.reset();
}

void Engine::session_prefix_drop(int handle) {
    Session& s = open_session();
    const auto it = s.prefix.find(handle);
    if (it == s.prefix.end()) throw std::runtime_error("EINVAL: unknown prefix handle " + std::to_string(handle));
    HIP_CHECK(hipStreamSynchronize(stream_));  // (an admission that copied from it has finished: admissions synchronise)
    s.prefix.erase(it);
}

Engine::PrefixStats Engine::session_prefix_stats() const {
    if (!sess_) throw std::runtime_error("EINVAL: no decode session is open on this engine");
    PrefixStats out;
    out.entries = sess_->prefix.size();
    for (const auto& kv : sess_->prefix) out.bytes += kv.second.kv.bytes();
    out.admissions = sess_->prefix_admissions;
    out.rows_reused = sess_->prefix_rows_reused;
    return out;
}

void Engine::session_step_body(Session& s, bool screened, bool stops, bool windowed) {
    // fixed parameters: the one ngram is switched off for the launch and the window kernel bans for every row;
    // per request: only the rows with a record (their RowParams carry ngram 0)
    const int window = windowed ? (s.feat.per_request ? 0 : s.p.ngram) : -1;
    DecSampleArgs sa;
    SampleArgs pen;
    sample_args(s.n, 0, s.p, s.feat.per_request, sa, pen);
    decode_step(s.n, rows_.Lcap);
    if (s.feat.logprobs) {
        const DecLpArgs lp = lp_args(sa, 0);
        decode_head(s.n, sa, pen, screened, &lp, stops, window);
    } else {
        decode_head(s.n, sa, pen, screened, nullptr, stops, window);
    }
}

// the head of the next burst.  Fixed parameters: decided at session_open.  Per request: screened iff every active
// slot is greedy with penalty 1.0 and the screened head applies at this n; it changes only where the set of
// active slots does (admit, retire), and the ban rows both final kernels keep make the change a step boundary
bool Engine::session_head_screened(const Session& s, unsigned carried) const {
    if (s.feat.logprobs) return false;  // the screened head never forms the logits
    if (carried & Controls::EXACT_HEAD) return false;  // ... which a constraint, a penalty, a windowed ban or an automaton acts on
    if (!s.feat.per_request) return s.screened;
    for (int b = 0; b < s.n; ++b)
        if (s.slot[b].rp.do_sample || s.slot[b].rp.rep_penalty != 1.0f) return false;
    return screen_applies(s.n, 1.0f);
}

std::vector<Engine::SlotStatus> Engine::session_step(int k) {
    Session& s = open_session();
    if (k < 1) throw std::runtime_error("EINVAL: a burst has at least one step");
    if (s.n == 0) return {};
    k = std::min(k, (int)Session::kBurstCap);
    // the capacity invariant (session_open), asserted before any launch: after this burst no slot's kv_pos may
    // pass its cache rows.  A slot retired at the burst boundary after it finished never gets here
    for (int b = 0; b < s.n; ++b) {
        const int room = rows_.Lcap - s.slot[b].kv_pos;
        if (room < 1)
            throw std::runtime_error("EINVAL: slot " + std::to_string(b) + " has used its " + std::to_string(rows_.Lcap) +
                                     " cache rows: retire finished slots at every burst boundary");
        k = std::min(k, room);
    }
    hipStream_t st = stream_;
    const bool use_graph = graphs_on();
    // a windowed ban is part of the step iff an active slot carries one.  With fixed parameters such a step runs
    // every selection at ngram 0, so the ban lists it leaves for a screened head are empty: the burst after it
    // runs the exact head once more, which writes them again
    const unsigned carried = s.carried();
    const bool windowed = (carried & Controls::NGW) != 0;
    const bool screened = session_head_screened(s, carried) && !s.ban_stale;
    // the match launch is part of the step iff an active slot carries a stop set: resolved here, once per burst
    const bool stops = (carried & Controls::STOPS) != 0;
    HipGraphExec& graph = s.graph[s.n][screened ? 1 : 0][stops ? 1 : 0][windowed ? 1 : 0];
    if (use_graph && !graph) {
        StreamCapture cap(st, capturing_);
        session_step_body(s, screened, stops, windowed);
        graph = cap.finish();
    }
    for (int i = 0; i < k; ++i) {
        if (use_graph) graph.launch(st);
        else session_step_body(s, screened, stops, windowed);
    }
    s.ban_stale = windowed && !s.feat.per_request && rows_.ban != nullptr;
    if (use_graph && stops) stop_launches_ += (size_t)k;
    for (int b = 0; b < s.n; ++b) s.slot[b].kv_pos += k;
    s.steps += (size_t)k;
    s.head_steps[screened ? 1 : 0] += (size_t)k;
    return session_poll();
}

std::vector<Engine::SlotStatus> Engine::session_poll() {
    Session& s = open_session();
    hipStream_t st = stream_;
    const int S = s.S;
    HIP_CHECK(hipMemcpyAsync(s.pin, rows_.done, S * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(s.pin + S, rows_.out_len, S * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(s.pin + 2 * S, rows_.err, 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (s.pin[2 * S]) throw std::runtime_error("EINTERNAL: decode hand-off timed out inside a fused kernel");
    std::vector<SlotStatus> out(s.n);
    std::vector<int> tmp;
    for (int b = 0; b < s.n; ++b) {
        Session::Slot& sl = s.slot[b];
        const int len = std::min(s.pin[S + b], (int)sl.max_new);
        out[b].slot = b;
        out[b].out_len = len;
        out[b].done = (s.pin[b] != 0 || len >= (int)sl.max_new) ? 1 : 0;
        if (len > sl.reported) {
            tmp.resize(len - sl.reported);
            HIP_CHECK(hipMemcpy(tmp.data(), rows_.out + (size_t)b * rows_.out_cap + sl.reported, tmp.size() * 4, hipMemcpyDeviceToHost));
            out[b].fresh.assign(tmp.begin(), tmp.end());
            sl.reported = len;
        }
    }
    return out;
}

std::vector<int64_t> Engine::session_retire(int slot, int* moved_from) {
    Session& s = open_session();
    if (slot < 0 || slot >= s.n) throw std::runtime_error("EINVAL: slot " + std::to_string(slot) + " is not active");
    const LangConfig& L = cfg_.lang;
    const DecodeRows& r = rows_;
    hipStream_t st = stream_;
    HIP_CHECK(hipStreamSynchronize(st));
    int len = 0;
    HIP_CHECK(hipMemcpy(&len, r.out_len + slot, 4, hipMemcpyDeviceToHost));
    len = std::min(len, (int)s.slot[slot].max_new);
    std::vector<int> ids(len);
    if (len) HIP_CHECK(hipMemcpy(ids.data(), r.out + (size_t)slot * r.out_cap, (size_t)len * 4, hipMemcpyDeviceToHost));
    const int last = s.n - 1;
    if (moved_from) *moved_from = -1;
    if (slot != last) {  // active pages stay dense: the last one moves into the freed slot
        session_slot_move(s, last, slot, std::min(s.slot[last].kv_pos + 1, r.Lcap));
        if (moved_from) *moved_from = last;
    }
    --s.n;
    refill_handoffs();
    HIP_CHECK(hipStreamSynchronize(st));
    return std::vector<int64_t>(ids.begin(), ids.end());
}

// the page of slot `src` (cache rows [0, rows_bound) and every per-slot row) into slot `dst`, one launch
void Engine::session_slot_move(Session& s, int src, int dst, int rows_bound) {
    const LangConfig& L = cfg_.lang;
    const DecodeRows& r = rows_;
    SlotMoveArgs m;
    m.kc = kc_; m.vc = vc_; m.layers = L.layers; m.slots = s.S; m.kv_heads = L.kv_heads; m.cap_rows = r.Lcap;
    m.hd = L.head_dim; m.layer_stride = (long)s.S * page_stride_; m.page_stride = page_stride_;
    m.head_stride = head_stride_; m.src = src; m.dst = dst;
    m.rows_bound = rows_bound;
    m.kv_len = r.kv_len; m.kv_pos = r.kv_pos; m.ctx = r.ctx; m.ctx_cap = r.ctx_cap; m.ctx_len = r.ctx_len;
    m.out = r.out; m.out_cap = r.out_cap; m.out_len = r.out_len; m.done = r.done; m.tok = r.tok;
    m.rng = r.rng; m.rng_words = RNG_WORDS; m.ban = r.ban; m.ban_ld = r.ban_ld; m.x = r.x; m.H = L.hidden;
    if (s.feat.per_request) m.rowpar = r.rowpar;
    if (s.feat.logprobs) { m.lp = r.lp; m.lp_top_id = r.lp_top_id; m.lp_top = r.lp_top; m.lp_k = r.lp_k; }
    launch_session_slot_move(m, stream_);
    if (s.feat.logit_bias) {  // the constraint travels as a copy of its row (an unconstrained page: the flag alone)
        if (s.slot[src].ctl & Controls::BIAS)
            HIP_CHECK(hipMemcpyAsync(r.bias + (size_t)dst * r.bias_ld, r.bias + (size_t)src * r.bias_ld,
                                     sizeof(float) * r.bias_ld, hipMemcpyDeviceToDevice, stream_));
        HIP_CHECK(hipMemcpyAsync(r.bias_on + dst, r.bias_on + src, sizeof(int), hipMemcpyDeviceToDevice, stream_));
    }
    if (s.feat.penalties)  // the record travels with its page: 16 bytes
        HIP_CHECK(hipMemcpyAsync(r.pen + dst, r.pen + src, sizeof(PenaltyRec), hipMemcpyDeviceToDevice, stream_));
    if (s.feat.ngram_window)  // the same: 144 bytes
        HIP_CHECK(hipMemcpyAsync(r.ngw + dst, r.ngw + src, sizeof(NgramWindowRec), hipMemcpyDeviceToDevice, stream_));
    // the automaton travels with its page: the used part of its tables (a page without one: the flag and scalars alone)
    if (s.feat.guided)
        launch_guided_slot_move(r.guided_tables(), src, dst, (s.slot[src].ctl & Controls::GUIDED) ? s.slot[src].g_states : 0,
                                (s.slot[src].ctl & Controls::GUIDED) ? s.slot[src].g_edges : 0, stream_);
    // the stop set travels with its page: a launch of its own (a page without one: the count, seen and hit alone)
    if (s.feat.stops) launch_stop_slot_move(r.stop_tab, r.stop_n, r.stop_seen, r.stop_hit, src, dst, stream_);
    s.slot[dst] = s.slot[src];
}

void Engine::session_guided_state(int slot, int* state, int* status) {
    Session& s = open_session();
    if (!s.feat.guided) throw std::runtime_error("EINVAL: this session was opened without DSOCR_SESSION_GUIDED");
    if (slot < 0 || slot >= s.n) throw std::runtime_error("EINVAL: slot " + std::to_string(slot) + " is not active");
    int st = 0, stat = 0;
    if (s.slot[slot].ctl & Controls::GUIDED) {
        HIP_CHECK(hipStreamSynchronize(stream_));
        HIP_CHECK(hipMemcpy(&st, rows_.g_state + slot, 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(&stat, rows_.g_status + slot, 4, hipMemcpyDeviceToHost));
    }
    if (state) *state = st;
    if (status) *status = stat;
}

void Engine::session_stop_hit(int slot, int* seq, int* match_len) {
    Session& s = open_session();
    if (!s.feat.stops) throw std::runtime_error("EINVAL: this session was opened without DSOCR_SESSION_STOP");
    if (slot < 0 || slot >= s.n) throw std::runtime_error("EINVAL: slot " + std::to_string(slot) + " is not active");
    HIP_CHECK(hipStreamSynchronize(stream_));
    int hit[2] = {-1, 0}, len = 0;
    HIP_CHECK(hipMemcpy(hit, rows_.stop_hit + (size_t)slot * 2, 8, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(&len, rows_.out_len + slot, 4, hipMemcpyDeviceToHost));
    // a match ends the page, so out_len is where it fired: one behind the slot's own max_new_tokens (the session's
    // output rows are longer) is outside what the page returns
    if (hit[0] < 0 || len > (int)s.slot[slot].max_new) { hit[0] = -1; hit[1] = 0; }
    if (seq) *seq = hit[0];
    if (match_len) *match_len = hit[1];
}

void Engine::session_logprobs(int slot, size_t first, size_t count, int top_k, float* token_lp, int64_t* top_id,
                              float* top_lp) {
    Session& s = open_session();
    if (!s.feat.logprobs) throw std::runtime_error("EINVAL: this session was opened without DSOCR_SESSION_LOGPROBS");
    if (slot < 0 || slot >= s.n) throw std::runtime_error("EINVAL: slot " + std::to_string(slot) + " is not active");
    if (top_k < 0 || top_k > LP_MAX_TOP) throw std::runtime_error("EINVAL: top_k must be 0..20");
    if (count && (!token_lp || (top_k && (!top_id || !top_lp)))) throw std::runtime_error("EINVAL: NULL argument");
    HIP_CHECK(hipStreamSynchronize(stream_));
    int len = 0;
    HIP_CHECK(hipMemcpy(&len, rows_.out_len + slot, 4, hipMemcpyDeviceToHost));
    len = std::min(len, (int)s.slot[slot].max_new);
    if (first > (size_t)len || count > (size_t)len - first)
        throw std::runtime_error("EINVAL: entries [" + std::to_string(first) + ", " + std::to_string(first + count) +
                                 ") pass the slot's " + std::to_string(len) + " tokens");
    if (!count) return;
    const size_t e0 = (size_t)slot * rows_.out_cap + first;  // the slot's first entry asked for
    HIP_CHECK(hipMemcpy(token_lp, rows_.lp + e0, count * 4, hipMemcpyDeviceToHost));
    if (!top_k) return;
    std::vector<int> ids(count * LP_MAX_TOP);
    std::vector<float> lps(count * LP_MAX_TOP);
    HIP_CHECK(hipMemcpy(ids.data(), rows_.lp_top_id + e0 * LP_MAX_TOP, ids.size() * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(lps.data(), rows_.lp_top + e0 * LP_MAX_TOP, lps.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < count; ++i)
        for (int k = 0; k < top_k; ++k) {
            top_id[i * top_k + k] = ids[i * LP_MAX_TOP + k];
            top_lp[i * top_k + k] = lps[i * LP_MAX_TOP + k];
        }
}

void Engine::session_close() {
    open_session();
    (void)hipStreamSynchronize(stream_);
    sess_.reset();
    kv_pages_ = 0;
    kv_page0_ = 0;
    ws_frozen_.clear();
    // the cache strides are the session's now: profile_decode replays the last generate, so it asks for a new one
    last_B_ = 0;
    last_Lmax_ = 0;
}

bool Engine::session_info(SessionInfo* out) const {
    if (!sess_) return false;
    if (out) {
        out->slots = sess_->S; out->active = sess_->n; out->max_context = sess_->max_context;
        out->out_cap = (int)rows_.out_cap; out->kv_cap = rows_.Lcap; out->burst_cap = Session::kBurstCap;
        out->steps = sess_->steps;
        out->steps_screened = sess_->head_steps[1]; out->steps_exact = sess_->head_steps[0];
        out->feat = sess_->feat;
        out->chunk_attn_launches = chunk_attn_launches_;
        if (const PendingAdmit* pa = sess_->pending.get()) {
            out->pending = true;
            out->pending_stage = pa->vision ? (pa->split ? pa->vstage : 1) : 0;
            out->pending_rows_done = pa->done; out->pending_rows_total = pa->total; out->pending_slices = pa->slices;
        }
    }
    return true;
}

// ============================================================================ profile_decode
// `body` captured as one hipGraph on the engine stream, replayed once to warm, then n replays between two
// events: the mean us of a replay
double Engine::replay_us(int n, const std::function<void()>& body) {
    hipStream_t st = stream_;
    HipEvent e0, e1;
    StreamCapture cap(st, capturing_);
    body();
    const HipGraphExec ge = cap.finish();
    ge.launch(st);
    HIP_CHECK(hipEventRecord(e0, st));
    for (int i = 0; i < n; ++i) ge.launch(st);
    HIP_CHECK(hipEventRecord(e1, st));
    HIP_CHECK(hipEventSynchronize(e1));
    return 1000.0 * ms_between(e0, e1) / n;
}

// Two figures per kernel (eager launches go host-bound below ~3.5 us per kernel, MI355X_MICROARCH.md
// graph-replay-floor, so they cannot time the short decode kernels):
//  * avg_us: every launch carries its own start / stop events on its dispatch packet
//    (hipExtLaunchKernelGGL through DSOCR_LAUNCH: the begin / end timestamps rocprofv3's kernel
//    trace reports), eager, one launch at a time — the figure the committed rocprof summaries
//    corroborate;
//  * replay_us: n launches back to back in one hipGraph replay, span / n - the kernel inside a
//    dependent chain as the decode loop runs it (duration + the ~1.2 us kernel boundary, minus
//    whatever startup the chained dispatch hides).
void Engine::time_launches(KernelProfile& kp, int n, const std::function<void(int)>& body) {
    body(0);  // warm (code objects, TLB) and every workspace allocated before capture
    std::vector<HipEvent> ev(2 * n);
    for (int i = 0; i < n; ++i) {
        ScopedSet timing(prof_events(), ProfEvents{ev[2 * i], ev[2 * i + 1]});  // the body's first launch times itself
        body(i);
        if (prof_events().start) throw std::runtime_error("EINTERNAL: profiled body made no instrumented launch");
    }
    HIP_CHECK(hipEventSynchronize(ev[2 * n - 1]));
    double sum = 0;
    for (int i = 0; i < n; ++i) sum += ms_between(ev[2 * i], ev[2 * i + 1]);
    kp.avg_us = 1000.0 * sum / n;
    kp.launches = n;
    if (graphs_on())
        kp.replay_us = replay_us(1, [&] { for (int i = 0; i < n; ++i) body(i); }) / n;
}

Engine::DecodeProfile Engine::profile_decode(int iters) {
    if (sess_) throw std::runtime_error("EINVAL: a decode session is open on this engine (close it before profile_decode)");
    DecodeProfile prof;
    const LangConfig& L = cfg_.lang;
    const int B = last_B_, Lmax = last_Lmax_;
    if (B == 0 || Lmax == 0) throw std::runtime_error("EINVAL: run a generate() first");
    const int H = L.hidden, hd = L.head_dim, QKVN = layers_[0].qkv.N;
    hipStream_t st = stream_;
    std::vector<int> kvpos(B);
    HIP_CHECK(hipMemcpy(kvpos.data(), rows_.kv_pos, B * 4, hipMemcpyDeviceToHost));
    // the replays re-run the last decoded position (pos - 1): its K/V slot is rewritten with the same values
    std::vector<int> pm1(B);
    long keys = 0;
    for (int b = 0; b < B; ++b) { pm1[b] = std::max(0, kvpos[b] - 1); keys += pm1[b] + 1; }
    int* d_pos = wsi("p_kvpos", B);
    HIP_CHECK(hipMemcpy(d_pos, pm1.data(), B * 4, hipMemcpyHostToDevice));
    prof.tokens = B;
    prof.kv_len = pm1[0] + 1;
    // a scratch q/k/v row (zeros) for the attention replays: s_qkv holds the fused launch's sentinels
    float* qkv0 = wsf("p_qkv_attn", (size_t)B * QKVN);
    HIP_CHECK(hipMemsetAsync(qkv0, 0, (size_t)B * QKVN * 4, st));
    // the replays rewrite the K / V slot of pos - 1 in every layer (the attention replays from the scratch
    // row): keep those slots and put them back after the attention replays and at the end, so the
    // step-graph replays and any later use of the engine state see the cache the generate left
    const size_t slot_w = (size_t)hd * 4, n_slots = (size_t)L.layers * B * 2;
    float* kv_saved = wsf("p_kv_saved", n_slots * L.kv_heads * hd);
    auto kv_slots = [&](bool restore) {
        for (int l = 0; l < L.layers; ++l)
            for (int b = 0; b < B; ++b)
                for (int kv = 0; kv < 2; ++kv) {
                    float* base = (kv ? vc_ : kc_) + (long)l * B * page_stride_ + (long)b * page_stride_ + (long)pm1[b] * hd;
                    float* keep = kv_saved + (((size_t)l * B + b) * 2 + kv) * L.kv_heads * hd;
                    if (restore)
                        HIP_CHECK(hipMemcpy2DAsync(base, head_stride_ * 4, keep, slot_w, slot_w, L.kv_heads, hipMemcpyDeviceToDevice, st));
                    else
                        HIP_CHECK(hipMemcpy2DAsync(keep, slot_w, base, head_stride_ * 4, slot_w, L.kv_heads, hipMemcpyDeviceToDevice, st));
                }
    };
    kv_slots(false);
    std::vector<int> moe_layers;
    for (int l = 0; l < L.layers; ++l)
        if (layers_[l].moe) moe_layers.push_back(l);
    if (!moe_layers.empty()) {
        const int E = L.n_routed, K = L.topk, I = L.moe_inter, TK = B * K;
        std::vector<int> ids(TK);
        HIP_CHECK(hipMemcpy(ids.data(), wsi("s_ids", TK), TK * 4, hipMemcpyDeviceToHost));
        std::vector<char> seen(E, 0);
        for (int v : ids)
            if (v >= 0 && v < E && !seen[v]) { seen[v] = 1; ++prof.experts_touched; }
        const float* Xc = rows_.x;
        // replay on a scratch copy of the residual stream so the engine state is untouched
        float* Xs = wsf("p_x", (size_t)B * H);
        HIP_CHECK(hipMemcpyAsync(Xs, Xc, (size_t)B * H * 4, hipMemcpyDeviceToDevice, st));
        // the gate/up and down launches of decode_step's dispatch (launch_moe_decode), replayed
        // alone on the routing state the last step left (logits, normalised rows, expert groups)
        auto args = [&](int i) { return moe_args(moe_layers[i % moe_layers.size()], B, Xs); };
        const int n = iters * (int)moe_layers.size();
        moe_decode_kernel_names(args(0), &prof.gateup_kernel, &prof.down_kernel);
        // rotating over the layers (~55 MB each) defeats the 256 MB Infinity Cache
        time_launches(prof.moe_gateup, n, [&](int i) { launch_moe_decode(args(i), st, MOE_GATEUP); });
        time_launches(prof.moe_down, n, [&](int i) { launch_moe_decode(args(i), st, MOE_DOWN); });
        const DecLayer& d0 = layers_[moe_layers[0]];
        const double Is = d0.has_shared ? d0.s_d.K : 0;
        const double touched = (double)prof.experts_touched;
        prof.moe_gateup.bytes = (touched * 2.0 * I + 2.0 * Is) * H * 2.0   // fp16 gate+up rows
                                + (double)B * H * 4 + (double)(TK * I + B * Is) * 4;  // x in, h out
        prof.moe_gateup.flops = 2.0 * (TK * 2.0 * I + B * 2.0 * Is) * H;
        prof.moe_down.bytes = (touched * I + Is) * H * 2.0 + (double)(TK * I + B * Is) * 4 + 2.0 * B * H * 4;
        prof.moe_down.flops = 2.0 * (TK * (double)I + B * Is) * H;
        if (d0.packed && B <= 8) {
            // packed layers stream the blocks: 144 bytes per 256 weights (Q4_K), 34 per 32 (Q8_0)
            auto bpw = [](const QMat& m) { return m.qtype == DSQ_Q4K ? 144.0 / 256.0 : 34.0 / 32.0; };
            prof.moe_gateup.bytes = (touched * 2.0 * I * bpw(d0.q_gu) + 2.0 * Is * (Is ? bpw(d0.q_sgu) : 0.0)) * H
                                    + (double)B * H * 4 + (double)(TK * I + B * Is) * 4;
            prof.moe_down.bytes = (touched * I * bpw(d0.q_d) + Is * (Is ? bpw(d0.q_sd) : 0.0)) * H
                                  + (double)(TK * I + B * Is) * 4 + 2.0 * B * H * 4;
        }
    }
    float* CTX = wsf("p_ctx", (size_t)B * H);
    time_launches(prof.attention, iters * L.layers, [&](int i) {
        DecAttn2Args da = attn_args(i % L.layers, B, Lmax);
        da.qkv = qkv0; da.kv_pos = d_pos; da.o = CTX;  // (the replays rewrite the K / V slot of pos - 1 from qkv0)
        launch_dec_attn(da, st);
    });
    kv_slots(true);
    // K and V of every attended key (f32 cache) + q/k/v row + context out
    prof.attention.bytes = (double)keys * L.kv_heads * hd * 4.0 * 2.0 + (double)B * (QKVN + H) * 4.0;
    prof.attention.flops = 4.0 * keys * L.heads * hd;
    profile_gemvs(prof, iters, moe_layers);
    if (graphs_on()) profile_step_context(prof, iters, (int)moe_layers.size());
    kv_slots(true);
    HIP_CHECK(hipStreamSynchronize(st));
    return prof;
}

// lm_head (exact and screened) and the attention-side GEMVs and routing of every layer, on scratch outputs
void Engine::profile_gemvs(DecodeProfile& prof, int iters, const std::vector<int>& moe_layers) {
    const LangConfig& L = cfg_.lang;
    const int B = last_B_, H = L.hidden, hd = L.head_dim, QKVN = layers_[0].qkv.N;
    hipStream_t st = stream_;
    const float* SX = rows_.x;
    float* LG = wsf("p_logits", (size_t)B * L.vocab);
    float* SXN = wsf("p_xn", (size_t)B * H);
    ensure_mm_weights(B);
    const bool fused = B <= 2 || (lm_swz_ && B <= 8);
    if (!fused) launch_rmsnorm(SX, H, SXN, H, B, H, final_norm_, L.rms_eps, st);
    time_launches(prof.lm_head, iters, [&](int) {
        DecGemvArgs g;
        g.M = B; g.N = L.vocab; g.K = H; g.W = lm_head_.W; g.ldw = H; g.wdtype = lm_head_.wdt; g.bias = lm_head_.b;
        g.y = LG; g.ldy = L.vocab;
        if (fused) {
            g.x = SX; g.ldx = H; g.norm_w = final_norm_; g.eps = L.rms_eps;
            if (B > 2) g.w_swz = lm_swz_;
        } else { g.x = SXN; g.ldx = H; }
        launch_dec_gemv(g, st);
    });
    prof.lm_head.bytes = (double)L.vocab * H * 2.0 + (double)B * (L.vocab + H) * 4.0;
    prof.lm_head.flops = 2.0 * B * (double)L.vocab * H;
    if (screen_applies(B, 1.0f)) {
        // screened head: int8 lm_head + selection (no bookkeeping, no ban: side-effect free)
        const LmHeadQ8Args q = head_q8_args(B);
        DecSampleArgs ss;
        ss.B = B; ss.V = L.vocab; ss.ld = L.vocab; ss.ctx = wsi("p_sctx", 64); ss.ctx_cap = 64;
        ss.ctx_len = wsi("p_ctxlen", B); ss.ngram = 0; ss.out_tok = wsi("p_tok", B);
        ss.blk_cnt = q.blk_cnt; ss.blk_t = q.blk_t; ss.cand = q.cand; ss.cand_hi = q.cand_hi; ss.nblk = q.nblk;
        ss.slot = q.slot; ss.w_exact = lm_head_.W; ss.w_exact_wdt = lm_head_.wdt; ss.xn = q.xn_out; ss.K = H;
        HIP_CHECK(hipMemsetAsync(ss.ctx_len, 0, B * 4, st));
        time_launches(prof.lm_head_screened, iters, [&](int) {
            launch_lmhead_q8(q, st);
            launch_dec_sample(ss, st);
        });
        prof.lm_head_screened.bytes = (double)L.vocab * H + (double)L.vocab * 8.0 + (double)B * H * 4.0;
        prof.lm_head_screened.flops = 2.0 * B * (double)L.vocab * H;
    }
    float* Y = wsf("p_qkv", (size_t)B * QKVN);
    float* XO = wsf("p_xo", (size_t)B * H);
    const int n = iters * L.layers;
    const bool fuse_norm = B <= 2;
    time_launches(prof.qkv, n, [&](int i) {
        const DecLayer& d = layers_[i % L.layers];
        DecGemvArgs g;
        g.M = B; g.N = QKVN; g.K = H; g.W = d.qkv.W; g.ldw = H; g.wdtype = d.qkv.wdt; g.bias = d.qkv.b;
        g.y = Y; g.ldy = QKVN; g.x = SX; g.ldx = H;
        if (fuse_norm) { g.norm_w = d.in_norm.w; g.eps = L.rms_eps; }
        launch_dec_gemv(g, st);
    });
    prof.qkv.bytes = (double)QKVN * H * 2.0 + (double)B * (H + QKVN) * 4.0;
    prof.qkv.flops = 2.0 * B * (double)QKVN * H;
    time_launches(prof.o_proj, n, [&](int i) {
        const DecLayer& d = layers_[i % L.layers];
        DecGemvArgs go;
        go.M = B; go.N = H; go.K = L.heads * hd; go.x = SX; go.ldx = H; go.W = d.o.W; go.ldw = go.K;
        go.wdtype = d.o.wdt; go.bias = d.o.b; go.y = XO; go.ldy = H; go.accumulate = 0;
        launch_dec_gemv(go, st);
    });
    prof.o_proj.bytes = (double)H * L.heads * hd * 2.0 + (double)B * 2 * H * 4.0;
    prof.o_proj.flops = 2.0 * B * (double)H * L.heads * hd;
    if (!moe_layers.empty() && moe_decode_route_launch(moe_args(moe_layers[0], B, XO))) {
        // the routing launches of the dispatch ([RMSNorm +] router GEMV [+ routing / grouping]; none when the
        // gate/up launch routes itself)
        time_launches(prof.router, iters * (int)moe_layers.size(), [&](int i) {
            MoeDecodeArgs ma = moe_args(moe_layers[i % moe_layers.size()], B, XO);
            ma.x = SX;
            launch_moe_decode(ma, st, MOE_ROUTE);
        });
        prof.router.bytes = (double)L.n_routed * H * 2.0 + (double)B * (H + L.n_routed) * 4.0;
        prof.router.flops = 2.0 * B * (double)L.n_routed * H;
    }
}

// every decoder layer of one step as one hipGraph (what the decode loop replays, minus lm_head and
// selection), and the same graph without one kernel's launches: the difference per launch is that kernel's
// in-context cost (its dispatch and its place in the dependent chain included).  The residual stream is
// restored at the head of each replay and the KV slot written is the next free position (past every
// generated token)
void Engine::profile_step_context(DecodeProfile& prof, int iters, int n_moe) {
    const int B = last_B_, Lmax = last_Lmax_, H = cfg_.lang.hidden, n = std::max(8, iters * 4);
    hipStream_t st = stream_;
    float* X = rows_.x;
    float* X0 = wsf("p_x0", (size_t)B * H);
    HIP_CHECK(hipMemcpyAsync(X0, X, (size_t)B * H * 4, hipMemcpyDeviceToDevice, st));
    decode_step(B, Lmax);  // every workspace exists before capture
    auto step_us = [&](int skip) {
        ScopedSet skipping(step_skip_, skip);
        return replay_us(n, [&] {
            HIP_CHECK(hipMemcpyAsync(X, X0, (size_t)B * H * 4, hipMemcpyDeviceToDevice, st));
            decode_step(B, Lmax);
        });
    };
    double full = step_us(0);
    const double no_gu = n_moe ? step_us(SKIP_GATEUP) : full;
    const double no_dn = n_moe ? step_us(SKIP_DOWN) : full;
    const double no_at = step_us(SKIP_ATTN);
    full = 0.5 * (full + step_us(0));  // bracket the variants: replay-to-replay drift averages out
    prof.layers_step.avg_us = full;
    prof.layers_step.launches = n;
    if (n_moe) {
        prof.moe_gateup.ctx_us = (full - no_gu) / n_moe;
        prof.moe_down.ctx_us = (full - no_dn) / n_moe;
    }
    prof.attention.ctx_us = (full - no_at) / cfg_.lang.layers;
    HIP_CHECK(hipMemcpyAsync(X, X0, (size_t)B * H * 4, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace dsocr
