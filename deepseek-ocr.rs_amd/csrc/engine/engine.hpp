// Engine: device-resident DeepSeek-OCR (SAM + CLIP + projector + DeepSeek-V2 MoE
// decoder) orchestrating the gfx950 kernels.  One engine per GPU; pages are
// batched inside an engine and sharded across GPUs by the caller (one process per
// GPU, no collectives: SURVEY §8e).
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "../kernels/kernels.hpp"
#include "config.hpp"
#include "hip_raii.hpp"

namespace dsocr {

struct Lin {
    void* W = nullptr;
    int wdt = WDT_BF16;
    int N = 0, K = 0;
    float* b = nullptr;
};
struct Ln {
    float* w = nullptr;
    float* b = nullptr;
};

struct SamBlock {
    Ln n1, n2;
    Lin qkv, proj, fc1, fc2;
    bool global = false;
    int rel_len = 0;                       // rows of the stored rel tables (2*tokens-1)
    std::vector<float> relh, relw;         // host copies [rel_len][hd]
    std::map<int, std::pair<float*, float*>> rel_dev;  // grid -> resized device tables
    bool use_rel = false;
};
struct SamW {
    Lin patch;
    bool has_pos = false;
    int pos_grid = 0;
    std::vector<float> pos_host;           // [C][grid][grid]
    std::map<int, float*> pos_dev;         // grid -> [grid*grid][C]
    std::vector<SamBlock> blocks;
    Lin neck0, neck2, net2, net3;
    Ln neck1, neck3;
};
struct ClipLayer {
    Ln ln1, ln2;
    Lin qkv, out, fc1, fc2;
};
struct ClipW {
    float* cls = nullptr;
    std::vector<float> pos_host;           // [seq+1][C]
    std::map<int, float*> pos_dev;         // tokens -> [tokens][C]
    Ln pre;
    std::vector<ClipLayer> layers;
};
struct DecLayer {
    Ln in_norm, post_norm;
    Lin qkv, o;
    bool moe = false;
    Lin gu, down;                 // dense MLP (layer 0) [2I][H], [H][I]
    Lin router;                   // [E][H]
    float* router_bias = nullptr; // e_score_correction_bias
    void* e_gu = nullptr;         // [E][2Im][H]
    void* e_d = nullptr;          // [E][H][Im]
    int e_wdt = WDT_F16;
    bool has_shared = false;
    Lin s_gu, s_d;                // [2Is][H], [H][Is]
    // fragment-ordered copies for the 3..8-page matrix-core kernels (Engine::ensure_mm_weights)
    void* e_gu_swz = nullptr; void* e_d_swz = nullptr; void* s_gu_swz = nullptr; void* s_d_swz = nullptr;
    void* router_swz = nullptr;  // fragment-ordered router rows (3..8 pages: the routing inside gate/up)
    void* qkv_swz = nullptr; void* o_swz = nullptr; void* gu_swz = nullptr;  // ... q/k/v, o_proj, dense gate|up
    // the persistent one-page decode (decode_persist.hip): down projections transposed to [inter][H] rows
    void* e_dT = nullptr;         // routed [E][Im][H]
    void* s_dT = nullptr;         // shared [Is][H] (MoE) / dense [I][H]
    // packed experts (DSOCR_LOAD_PACKED_EXPERTS): the snapshot's Q4_K / Q8_0 blocks kept for the packed decode
    // kernels (decode_q.hip), beside the fp16 copies above; routed [E][2Im][H], [E][H][Im], shared [2Is][H], [H][Is]
    bool packed = false;
    QMat q_gu, q_d, q_sgu, q_sd;
    size_t packed_bytes = 0;
};

// DeepSeek-OCR-2: the Qwen2 decoder used as the vision encoder (vision/qwen2.rs)
struct EncLayer {
    Ln in_norm, post_norm;
    Lin qkv, o;    // q|k|v fused [(heads + 2 kv) hd][D] with biases; o_proj without
    Lin gu, down;  // gate|up fused [2I][D], [D][I]
};
struct Qwen2EncW {
    std::vector<EncLayer> layers;
    float* norm = nullptr;
    float* query_768 = nullptr;   // [144][D]
    float* query_1024 = nullptr;  // [256][D]
    float* cos = nullptr;         // [512][hd] (qwen2.rs:573-604)
    float* sin = nullptr;
};

struct PagePixels {
    int variant = 0;  // 0 = DeepSeek-OCR, 1 = DeepSeek-OCR-2: the tile budget and the <image> slot layout
    int base = 1024, tile = 640;
    bool crop = true;
    int crop_w = 1, crop_h = 1;
    std::vector<float> global_chw;  // [3][G][G]
    int gsize = 0;
    std::vector<float> tiles_chw;   // [n][3][T][T]
    int n_tiles = 0;
    size_t n_image_tokens = 0;
    // optional device-resident copies (dsocr_page_to_device): generate() then reads the pixels
    // from HBM (device-to-device gather) instead of uploading the host arrays
    float* global_dev = nullptr;
    float* tiles_dev = nullptr;
    int dev_ordinal = -1;
    ~PagePixels();
};

struct Timings {
    double vision_prepare_ms = 0, vision_compute_ms = 0, prefill_ms = 0, iterative_ms = 0, generate_ms = 0;
    size_t steps = 0, pages = 0;
    // algorithmic f32 FLOPs of the stage (linears 2 M N K, attention 4 L_q L_k d per head; causal
    // prefill counts the lower triangle): the MFMA roofline's numerator
    double vision_flops = 0, prefill_flops = 0;
};

// One request's constraint on the tokens it may emit: the logits row becomes l + b with
// b[ids[i]] = values[i] and, elsewhere, 0 or (allow_only) -inf.  Checked by validate_logit_bias before any device work.
struct LogitBias {
    std::vector<int> ids;
    std::vector<float> values;
    bool allow_only = false;
    bool active() const { return allow_only || !ids.empty(); }
};
// EINVAL: an id outside [0, vocab), a duplicate id, a NaN or +inf value, allow_only without ids, more ids than vocab
void validate_logit_bias(const LogitBias& lb, int vocab);

// One request's stop set: 1..STOP_MAX_SEQS sequences of 1..STOP_MAX_LEN token ids; the page is done
// from the step on whose output tail equals one of them.  Checked by validate_stop_set before any device work.
struct StopSet {
    std::vector<std::vector<int>> seqs;
    bool active() const { return !seqs.empty(); }
};
// EINVAL: more than 16 sequences, a length of 0 or above 32, an id outside [0, vocab), two identical sequences
void validate_stop_set(const StopSet& st, int vocab);

// One request's frequency / presence penalties and min-p.  Off: all three at their defaults.
struct Penalties {
    float frequency = 0.f, presence = 0.f;
    double min_p = 0.0;
    bool active() const { return frequency != 0.f || presence != 0.f || min_p > 0.0; }
    // the record the kernels read: ln_min_p = log(min_p) in f64, -inf when the filter is off
    PenaltyRec rec() const;
};
// EINVAL: a non-finite frequency or presence; min_p NaN, below 0 or above 1
void validate_penalties(const Penalties& pn);

// One request's windowed no-repeat n-gram ban: size g, window w, and ids that are never banned.
// Off: g < 2.  On: the record replaces the request's plain no_repeat_ngram_size ban.
struct NgramWindow {
    int g = 0, w = 0;
    std::vector<int> whitelist;
    bool active() const { return g >= 2; }
    // the record the kernel reads (the whitelist without repeats)
    NgramWindowRec rec() const;
};
// EINVAL: on with w < 1; more than NGRAM_MAX_WHITELIST ids; an id outside [0, vocab)
void validate_ngram_window(const NgramWindow& nw, int vocab);

// One request's token automaton: n_states states, a start state, a byte per state (accepting: the
// EOS id is kept there) and the edges in CSR form, ids strictly ascending within a state.  A state without an
// outgoing edge is terminal: reaching it completes the page.  Off: n_states == 0.
struct Guided {
    int n_states = 0, start = 0;
    std::vector<uint8_t> accepting;
    std::vector<int> row_ptr, edge_tok, edge_next;
    bool active() const { return n_states > 0; }
    long edges() const { return (long)edge_tok.size(); }
};
// EINVAL: n_states outside [1, GUIDED_MAX_STATES]; more than GUIDED_MAX_EDGES edges; row_ptr not non-decreasing from
// 0 to E; a token outside [0, vocab) or equal to eos; tokens not strictly ascending within a state; edge_next or
// start outside [0, n_states); a terminal start.  (A record that is off passes.)
void validate_guided(const Guided& g, int vocab, long eos);

// The per-request decode controls: what a request carries beyond its prompt and GenParams.  A new
// control is a member here, a step of Engine::write_controls and a launch of Engine::selection_tail.
struct Controls {
    LogitBias bias;
    StopSet stops;
    Penalties pen;
    NgramWindow ngw;
    Guided guided;
    // which of them are on, as one mask (a session's slots keep it; a batch's is the OR over its requests)
    enum : unsigned { BIAS = 1, STOPS = 2, PEN = 4, NGW = 8, GUIDED = 16, EXACT_HEAD = BIAS | PEN | NGW | GUIDED };
    unsigned active() const {
        return (bias.active() ? BIAS : 0u) | (stops.active() ? STOPS : 0u) | (pen.active() ? PEN : 0u) |
               (ngw.active() ? NGW : 0u) | (guided.active() ? GUIDED : 0u);
    }
    // the controls that act on the logits row: the screened head never forms it (a stop set runs under either head)
    bool needs_exact_head() const { return (active() & EXACT_HEAD) != 0; }
    // every validate_* above (a bias or stop set that is off is not looked at); eos < 0: no EOS rule
    void validate(int vocab, long eos) const;
};

struct GenRequest {
    Controls ctl;
    std::vector<int> ids;
    std::vector<uint8_t> mask;
    const PagePixels* page = nullptr;
    const float* image_rows = nullptr;
    size_t n_image_rows = 0;
};
struct GenParams {
    size_t max_new = 512;
    float rep_penalty = 1.f;
    int ngram = 20;
    long eos = -1;
    bool ignore_eos = false;
    // sampling (do_sample && temperature > 0, sampling.rs:67-86); rng = init_rng(seed) per call
    bool do_sample = false;
    double temperature = 0.0, top_p = -1.0;
    long top_k = 0;
    bool seed_set = false;
    uint64_t seed = 0;
    bool use_cache = true;  // false: generate_without_cache (model/mod.rs:2051-2283)
    float* trace = nullptr; // host [B][max_new][vocab]: raw logits of every step (parity hook)
    int lp_k = -1;          // >= 0: per-token log-probabilities with lp_k alternatives (0..LP_MAX_TOP); the exact head runs
};
// The device rows a decode batch runs on, one record per engine: a generate call or a session
// reserves and initialises them (Engine::reserve_decode_rows), and every decode launch, admission, poll and profile
// takes its pointers from here.  Row b of a per-row buffer starts b x its capacity behind the base.
struct DecodeRows {
    // capacities: rows, cache rows per page, ints per context / output / ban row, floats per hand-off copy
    int S = 0, Lcap = 0;
    long ctx_cap = 0, out_cap = 0, ban_ld = 0;
    size_t part_floats = 0, qkv_floats = 0;
    // per-row state (ban, rng, rowpar: nullptr when the spec did not ask for them)
    float *x = nullptr, *logits = nullptr;
    int *ctx = nullptr, *ctx_len = nullptr, *kv_pos = nullptr, *kv_len = nullptr, *done = nullptr, *out_len = nullptr,
        *out = nullptr, *tok = nullptr, *ban = nullptr;
    uint32_t* rng = nullptr;
    RowParams* rowpar = nullptr;
    // selection scratch (st_*: the sampler's; st_w is 2 V floats per row viewed as V doubles)
    float* red_val = nullptr;
    int *red_idx = nullptr, *st_idx = nullptr;
    uint32_t* st_key = nullptr;
    double* st_w = nullptr;
    // step-wide words: the fused kernels' give-up flag and the arrival tickets (zero between launches)
    int *err = nullptr, *attn_cnt = nullptr, *route_cnt = nullptr, *dn_tick = nullptr, *d_tick = nullptr;
    // the two hand-off copies (Engine::attn_args): sentinel-filled at every step boundary
    float *qkv[2] = {nullptr, nullptr}, *part[2] = {nullptr, nullptr};
    // log-probability rows (lp_k >= 0): entries [S][out_cap] (x lp_k alternatives), the side logits and the partials
    int lp_k = -1;
    float *lp = nullptr, *lp_top = nullptr, *lp_side = nullptr, *lp_pmax = nullptr, *lp_psum = nullptr, *lp_ptv = nullptr;
    int *lp_top_id = nullptr, *lp_rec = nullptr, *lp_pti = nullptr;
    // logit bias rows (spec.bias): the dense rows [S][bias_ld], the per-row flag, and the staging buffer an
    // admission's sparse list is uploaded to ([ids | values], bias_stage_cap pairs)
    float* bias = nullptr;
    long bias_ld = 0;
    int *bias_on = nullptr, *bias_stage = nullptr;
    size_t bias_stage_cap = 0;
    // stop sequences (spec.stops): the tables [S][STOP_ROW_INTS], the sequence counts, the output lengths already
    // examined and the hits [S][2], and the staging buffer the admissions' lists are uploaded to
    int *stop_tab = nullptr, *stop_n = nullptr, *stop_seen = nullptr, *stop_hit = nullptr, *stop_stage = nullptr;
    int stop_stage_rows = 0;
    // frequency / presence / min-p records (spec.penalties): one per row, every one starts off
    PenaltyRec* pen = nullptr;
    // windowed n-gram ban records (spec.ngram_window): one per row, every one starts off
    NgramWindowRec* ngw = nullptr;
    // guided decoding (spec.guided): every row's bitmask [g_states][g_mask_ld] and CSR (g_states + 1 row pointers,
    // g_edges edges), the state / seen / status / flag words, and the staging buffer automata are uploaded to
    uint32_t* g_mask = nullptr;
    long g_mask_ld = 0, g_edges = 0;
    int g_states = 0;
    int *g_rowptr = nullptr, *g_tok = nullptr, *g_next = nullptr, *g_state = nullptr, *g_seen = nullptr,
        *g_status = nullptr, *g_on = nullptr, *g_stage = nullptr;
    size_t g_stage_cap = 0;
    GuidedTables guided_tables() const {
        GuidedTables t;
        t.mask = g_mask; t.mask_ld = g_mask_ld; t.cap_states = g_states; t.cap_edges = g_edges;
        t.rowptr = g_rowptr; t.tok = g_tok; t.next = g_next;
        t.state = g_state; t.seen = g_seen; t.status = g_status; t.on = g_on;
        return t;
    }
};
// What a caller of Engine::reserve_decode_rows asks for
struct DecodeRowsSpec {
    int rows = 0, Lcap = 0;
    long ctx_cap = 0, out_cap = 0;
    bool sampler = false, ban = false, rowpar = false;  // sampler scratch + RNG rows / ban rows / RowParams rows
    bool handoff_max = false;  // hand-off records sized for every n in 1..rows (else for exactly `rows`)
    bool zero_fill = false;    // the cache and the per-row state start as zeros (else the caller uploads the rows)
    int lp_k = -1;             // >= 0: log-probability rows with lp_k alternatives
    bool lp_side = false;      // ... and the raw logits at the context ids
    bool bias = false;         // logit bias rows (every flag starts 0) ...
    size_t bias_stage = 0;     // ... and a list staging buffer of this many (id, value) pairs
    bool stops = false;        // stop-sequence rows (every count starts 0) ...
    int stop_stage_rows = 1;   // ... and staging for this many lists at a time
    bool penalties = false;    // PenaltyRec rows (every record starts off)
    bool ngram_window = false; // NgramWindowRec rows (every record starts off)
    bool guided = false;       // token-automaton rows (every flag starts 0) of guided_states states and guided_edges
    int guided_states = GUIDED_MAX_STATES;  // edges each ...
    long guided_edges = GUIDED_MAX_EDGES;
    size_t guided_stage = 0;   // ... and a staging buffer of this many ints
};
typedef void (*TokenCb)(size_t, const int64_t*, void*);
// rand_core seed_from_u64 for rand 0.8.5 StdRng, in the layout sampling.hip reads (RNG_WORDS words)
std::vector<uint32_t> rng_state_from_u64(uint64_t seed);

class Engine {
  public:
    Engine(const std::string& config_path, const std::string& weights_path, int device, int dtype, uint64_t seed,
           const std::string& snapshot_path = "", uint32_t load_flags = 0);
    ~Engine();
    // MoE layers that kept their packed blocks / all MoE layers / device bytes of the packed tables
    void packed_info(size_t* packed_layers, size_t* moe_layers, size_t* packed_bytes) const;

    const ModelConfig& cfg() const { return cfg_; }
    int variant() const { return cfg_.variant; }
    // vision embeddings of pages (host output rows per page concatenated)
    std::vector<std::vector<float>> image_embeddings(const std::vector<const PagePixels*>& pages);
    // batched generate; returns generated ids per page
    std::vector<std::vector<int64_t>> generate(const std::vector<GenRequest>& reqs, const GenParams& p, TokenCb cb,
                                               void* user);
    Timings last_timings() const { return timings_; }
    // the log-probability entries of the last generate with p.lp_k >= 0: per page n[b] entries (one per emitted id,
    // same index) of rows [b][cap]: lp, and [b][cap][K]: top_id / top_lp
    struct LogprobRows {
        int K = 0;
        size_t cap = 0;
        std::vector<int> n;
        std::vector<float> lp, top_lp;
        std::vector<int> top_id;
    };
    const LogprobRows& last_logprobs() const { return last_lp_; }
    // the stop hits of the last generate: {seq, match_len} per page ({-1, 0}: no stop fired; empty: no page had stops)
    const std::vector<int>& last_stop_hits() const { return last_stop_hits_; }
    // the last generate's [state, status] per request (empty when no request carried an automaton)
    const std::vector<int>& last_guided() const { return last_guided_; }
    // dec_stop_match launches of this engine so far (issued or replayed inside a step graph)
    size_t stop_launches() const { return stop_launches_; }
    // Replays the decode MoE grouped GEMV (routed experts, gate/up + down) of every MoE
    // layer on the last decode step's routing, timing each launch pair with HIP events.
    struct KernelProfile {
        double avg_us = 0, bytes = 0, flops = 0;
        int launches = 0;
        double replay_us = 0;
        double ctx_us = 0;  // in-context marginal cost per launch (step graph with / without it)
    };
    struct DecodeProfile {
        KernelProfile moe_gateup, moe_down, attention, lm_head, qkv, o_proj, router, layers_step, lm_head_screened;
        int experts_touched = 0, tokens = 0, kv_len = 0;
        const char* gateup_kernel = "";  // kernels the dispatch picked at this batch size
        const char* down_kernel = "";
    };
    DecodeProfile profile_decode(int iters);
    // In-context launch spans (diagnostics, off by default): while on, every decode step of a generate
    // records per layer the (first wave entry, last wave exit) of its MoE gate/up, MoE down and
    // attention launches, with the distinct experts the MoE launches streamed (WaveSpan +
    // span_reduce_kernel; one extra fold launch after each stamped launch, inside the replayed graph).
    // SPAN_CHAIN (alone): no fold or event between launches; the gate/up, down, attention, o_proj and router
    // launches of every layer stamp their own slot region and one fold runs at the end of each step, so the
    // step is the production chain plus the waves' slot stores: exit(k) - exit(k - 1) is a launch's
    // dispatch-level duration (its boundary included, as a back-to-back rocprofv3 kernel-trace record)
    enum SpanKind : int { SPAN_GATEUP = 0, SPAN_DOWN = 1, SPAN_ATTN = 2, SPAN_KINDS = 3, SPAN_OPROJ = 3, SPAN_ROUTER = 4,
                          SPAN_KINDS_CHAIN = 5 };
    static constexpr int SPAN_FIELDS = 5;
    enum SpanMode : int { SPAN_WAVES = 1, SPAN_EVENTS = 2, SPAN_CHAIN = 4 };  // bit mask; 0 = off
    void set_spans(int mode) { span_mode_ = (mode & SPAN_CHAIN) ? SPAN_CHAIN : mode & (SPAN_WAVES | SPAN_EVENTS); }
    int span_kinds() const { return spans_kinds_; }
    // [kind][layer][step][SPAN_FIELDS] u64 {entry, exit (100 MHz wall clock), distinct experts, waves,
    // dispatch duration in ns (HIP events recorded around the launch inside the replayed graph)} of the
    // last generate with spans on; step = tokens emitted before the step (1 .. steps - 1 are decode steps)
    const std::vector<unsigned long long>& spans() const { return spans_host_; }
    int span_steps() const { return spans_steps_; }  // the steps of spans_host_ (set with it)
    hipStream_t stream() const { return stream_; }
    // persistent decode diagnostics: mode 1 = the next generate times every persistent launch with HIP events
    // and records the phase clocks (PK_STAMPS per workgroup and layer) of its decode steps; read them after it
    void set_persist_stamps(int mode) { persist_stamp_mode_ = mode; }
    bool persist_used() const { return persist_active_; }
    const std::vector<unsigned long long>& persist_stamps() const { return persist_stamps_host_; }
    const std::vector<double>& persist_launch_us() const { return persist_ev_us_; }
    void upload_page(PagePixels& pg);
    void prepare_page_device(const uint8_t* rgb, int w, int h, PagePixels& px);

    // ---- decode sessions: a long-lived batch of up to `slots` pages; pages are admitted
    // (vision + prefill into their own slot) and retired between bursts of the unchanged decode step.  Active
    // pages occupy slots [0, active).  A session and generate / profile_decode exclude each other (EINVAL).
    // What a session is opened with, fixed until it closes (the DSOCR_SESSION_* bits):
    struct SessionFeatures {
        // p are the defaults and every admission brings its own selection parameters (a RowParams record per slot,
        // read by the per-row selection kernels); the head is chosen per burst: screened while every active slot is
        // greedy without a penalty, else the exact head with both selectors
        bool per_request = false;
        // every slot keeps out_cap x LP_MAX_TOP log-probability entries; the exact head runs at every n
        bool logprobs = false;
        // every slot keeps a dense bias row; an admission may carry a constraint (GenRequest::bias), and a burst runs
        // the exact head iff an active slot carries one
        bool logit_bias = false;
        // every slot keeps a stop table; an admission may carry a stop set (GenRequest::stops), and a burst's step
        // graph contains the match launch iff an active slot carries one
        bool stops = false;
        // every slot keeps a PenaltyRec; an admission may carry penalties (GenRequest::pen), and a burst runs the
        // exact head iff an active slot carries a record that is on
        bool penalties = false;
        // every slot keeps an NgramWindowRec; an admission may carry a windowed ban (GenRequest::ngw), and a burst
        // runs the exact head with the window launch iff an active slot carries a record that is on
        bool ngram_window = false;
        // every slot keeps the tables of a token automaton; an admission may carry one
        // (GenRequest::guided), and a burst runs the exact head iff an active slot carries one
        bool guided = false;
    };
    struct SessionInfo {
        int slots = 0, active = 0, max_context = 0, out_cap = 0, kv_cap = 0, burst_cap = 0;
        size_t steps = 0;  // decode steps replayed since the session opened
        size_t steps_screened = 0, steps_exact = 0;  // ... under the screened / the exact lm_head + selection
        SessionFeatures feat;
        // a chunked admission in flight (session_admit_begin): prompt rows prefilled so far / in all, slices run
        bool pending = false;
        int pending_rows_done = 0, pending_rows_total = 0, pending_slices = 0;
        int pending_stage = 0;           // the vision stage the next slice runs (1 SAM, 2 CLIP / encoder, 3 projector), 0: none
        size_t chunk_attn_launches = 0;  // launch_attention_chunk launches of this engine so far
    };
    struct SlotStatus {
        int slot = 0, done = 0, out_len = 0;
        std::vector<int64_t> fresh;  // the tokens since the last poll
    };
    // p: the session's sampling parameters (use_cache must be set, no trace); p.max_new = out_cap
    void session_open(int slots, int max_context, const GenParams& p, const SessionFeatures& feat);
    // {seq, match_len} of a live slot ({-1, 0}: no stop fired within its max_new_tokens)
    void session_stop_hit(int slot, int* seq, int* match_len);
    // the automaton state and status (0 running, 1 complete, 2 violated) of an active slot; both 0 without an automaton
    void session_guided_state(int slot, int* state, int* status);
    // entries [first, first + count) of a live slot, trimmed to top_k <= LP_MAX_TOP alternatives ([count][top_k])
    void session_logprobs(int slot, size_t first, size_t count, int top_k, float* token_lp, int64_t* top_id, float* top_lp);
    int session_admit(const GenRequest& rq, size_t max_new, bool seed_set, uint64_t seed);
    // the request's whole parameter set (max_new, seed and what select_token_id reads).  Without per_request:
    // EINVAL when it differs from the session's in more than max_new / seed
    int session_admit(const GenRequest& rq, const GenParams& p);
    std::vector<SlotStatus> session_step(int k);
    std::vector<SlotStatus> session_poll();
    // the page's ids; *moved_from = the slot whose page now lives in `slot` (the last active one), or -1
    std::vector<int64_t> session_retire(int slot, int* moved_from);
    void session_close();
    bool session_info(SessionInfo* out) const;  // false: no session is open
    // ---- page prefix cache: K/V rows [0, rows) of a live slot's prompt kept in an entry of their
    // own; a later request whose prompt starts with the same ids / mask is admitted behind a copy of them and
    // prefills only its remaining rows.  Entries are not workspaces: no captured graph reads them.
    static constexpr int kMaxPrefixEntries = 64;
    struct PrefixStats {
        size_t entries = 0, bytes = 0, admissions = 0, rows_reused = 0;
    };
    int session_prefix_keep(int slot, int rows);  // -> handle; ENOMEM when the allocation fails
    int session_admit_prefix(int handle, const GenRequest& rq, const GenParams& p);
    void session_prefix_drop(int handle);
    PrefixStats session_prefix_stats() const;
    // ---- chunked admission: session_admit in slices, so that session_step can run between them.
    // begin: every check of session_admit, no device work; the page is staged in the session's last slot.
    // advance: one slice (vision, then the prefill in chunks of chunk_rows prompt rows, the last one with the
    // admission's tail), synchronised; true with *slot set when the page is active.  cancel drops it.
    // rq.page must stay alive until the admission completes or is cancelled; rq.image_rows are copied at begin.
    int session_admit_begin(const GenRequest& rq, const GenParams& p, int chunk_rows);
    bool session_admit_advance(int* slot);
    void session_admit_cancel();

  private:
    // ---- loading
    void load_weights(const std::string& path, uint64_t seed, const std::string& snapshot_path, bool packed_experts);
    // ---- workspace
    void* ws(const std::string& name, size_t bytes);
    float* wsf(const std::string& name, size_t n) { return (float*)ws(name, n * sizeof(float)); }
    int* wsi(const std::string& name, size_t n) { return (int*)ws(name, n * sizeof(int)); }
    long* wsl(const std::string& name, size_t n) { return (long*)ws(name, n * sizeof(long)); }
    template <typename T>
    T* upload(const std::string& name, const std::vector<T>& v) {
        // host vectors are often temporaries: stage them in a per-name pinned buffer and copy
        // asynchronously (each name is uploaded at most once per generate(), which ends with a
        // stream synchronisation, so a staging buffer is never rewritten while in flight)
        T* p = (T*)ws(name, v.size() * sizeof(T) + 16);
        upload_to(p, name, v);
        return p;
    }
    // ... into rows reserved elsewhere (DecodeRows), staged under `name`
    template <typename T>
    void upload_to(T* dst, const std::string& name, const std::vector<T>& v) {
        const size_t bytes = v.size() * sizeof(T);
        if (v.empty()) return;
        void* h = pinned(name, bytes);
        std::memcpy(h, v.data(), bytes);
        HIP_CHECK(hipMemcpyAsync(dst, h, bytes, hipMemcpyHostToDevice, stream_));
    }
    void* pinned(const std::string& name, size_t bytes);
    // ---- compute pieces
    void linear(const float* x, int M, int ldx, const Lin& l, float* y, int ldy, int act = 0, int accumulate = 0,
                const int* c_rows = nullptr);
    float* sam_pos(int g);
    std::pair<float*, float*> sam_rel(SamBlock& b, int g);
    float* clip_pos(int tokens);
    // runs SAM+CLIP+projector on n images of size S; returns device rows [n*(S/64)^2][H] in buffer `out`
    float* vision_pass(const float* imgs, int n, int S, const std::string& out);
    // OCR2: Qwen2 encoder + projector on n views' SAM token rows [n][P][D]; device rows [n*P][H] in buffer `out`
    float* encoder_pass(const float* sam_out, int n, int P, const std::string& out);
    void check_page_variant(const PagePixels& pg) const;
    void decode_step(int B, int Lmax);
    // one page: every decoder layer of a step as one persistent launch (decode_persist.hip) when the model's
    // shape and dtypes fit it, all 256 workgroups are resident and DSOCR_PERSIST=1 (opt-in)
    bool persist_ok(int B, int Lmax);
    void ensure_persist();
    MoeDecodeArgs moe_args(int l, int B, float* X);
    DecAttn2Args attn_args(int l, int B, int Lmax, int copy = 0);
    // the decode rows: reserved under their workspace names and initialised (tickets and flag zeroed, hand-offs
    // sentinel-filled) by the one function that knows their sizes
    DecodeRows rows_;
    void reserve_decode_rows(const DecodeRowsSpec& spec);
    void refill_handoffs();
    // selection arguments of rows [slot0, slot0 + B): p's scalars, and per_request the rows' own RowParams records
    void sample_args(int B, int slot0, const GenParams& p, bool per_request, DecSampleArgs& sa, SampleArgs& pen);
    // the log-probability rows of the pages from row0 on that sa selects for
    DecLpArgs lp_args(const DecSampleArgs& sa, int row0);
    // the logit bias rows of the same pages (only where rows_.bias is set)
    DecBiasArgs bias_args(const DecSampleArgs& sa, int row0);
    // row `row`'s dense bias row and flag from the constraint (an inactive one clears the flag); `stage_off`: where
    // in the staging buffer its list goes (pairs)
    void build_logit_bias(const LogitBias& lb, int row, size_t stage_off);
    // the penalty records of the same pages (only where rows_.pen is set), and rows [row0, row0 + n)'s records
    // written from the requests' (pinned staging under "s_penstage"; the caller synchronises before the next write)
    DecPenaltyArgs penalty_args(const DecSampleArgs& sa, int row0);
    void write_penalties(const GenRequest* reqs, int row0, int n);
    // the windowed-ban records likewise (only where rows_.ngw is set; staging under "s_ngwstage").  plain: the
    // n-gram size the launch applies, with an unbounded window, to rows whose record is off (0: such rows are skipped)
    DecNgramWindowArgs ngram_window_args(const DecSampleArgs& sa, int row0, int plain);
    void write_ngram_windows(const GenRequest* reqs, int row0, int n);
    // the automaton rows of the same pages (only where rows_.g_on is set): one row's tables from a request's automaton
    // (staged at stage_off ints of "s_gstage"; the caller synchronises before the region is reused), the mask and the
    // advance launches
    void build_guided(const Guided& g, int row, size_t stage_off, long eos);
    DecGuidedMaskArgs guided_mask_args(const DecSampleArgs& sa, int row0);
    DecGuidedAdvanceArgs guided_advance_args(const DecSampleArgs& sa, int row0);
    // the stop rows of the same pages (only where rows_.stop_tab is set), and the match launch on them (counted)
    DecStopArgs stop_args(const DecSampleArgs& sa, int row0);
    void stop_match(const DecSampleArgs& sa, int row0);
    // row `row`'s table from the stop set (an inactive one clears the count), staged in list region `stage_row`
    void build_stop_table(const StopSet& st, int row, int stage_row);
    // stops: the match launch follows the final selection kernel
    void decode_head(int B, DecSampleArgs& sa, const SampleArgs& pen, bool screened, const DecLpArgs* lp = nullptr,
                     bool stops = false, int window = -1);  // window >= 0: the windowed-ban launch, with this plain size
    // Which launches of the exact selection tail run.  window >= 0: the window launch with this plain size, and the
    // selection on a copy of sa with ngram = 0
    struct TailPlan {
        bool bias = false, guided = false, penalties = false, stops = false;
        int window = -1;
        const DecLpArgs* lp = nullptr;
    };
    // The one place that issues the exact selection on logits already formed, for the pages from row0 on that sa
    // describes: bias add, automaton mask, log-prob partial, repetition penalty, output penalty, window ban,
    // selection, automaton advance, stop match, log-prob final
    void selection_tail(const DecSampleArgs& sa, const SampleArgs& pen, int row0, const TailPlan& t);
    // rows [row0, row0 + n)'s bias row, automaton tables, penalty record, window record and stop table from the
    // requests, each only where rows_ has that buffer; staging offsets are packed from 0 in request order
    void write_controls(const GenRequest* reqs, int row0, int n, long eos);
    void reserve_head_ws(int B);
    LmHeadQ8Args head_q8_args(int B);
    bool screen_applies(int B, float rep_penalty) const;
    // generate(): the state of one call (engine.cpp) and its phases, in call order
    struct GenState;
    void embed_pages(GenState& g);
    void plan_image_rows(GenState& g);
    void reset_decode_state(GenState& g);
    // past (optional, per sequence): rows [0, past[b]) are already in the cache and lens[b] counts the rows after them
    // row0: the decode row (and cache page) of the first sequence - a session's admission prefills into its slot
    // head: the final norm + lm_head on every sequence's last row (a chunk that is not the prompt's last needs none)
    // chunk_attn: rows behind a past attend through launch_attention_chunk (query tiles), not launch_attention_past
    void forward_rows(GenState& g, const std::vector<int>& lens, const std::vector<int>& past = {}, int row0 = 0,
                      bool head = true, bool chunk_attn = false);
    void init_sampling(GenState& g);
    bool poll(GenState& g);
    void stream_tokens(GenState& g, int n);
    void decode_uncached(GenState& g);
    void decode_cached(GenState& g);
    void step_body(GenState& g);
    void begin_spans(GenState& g);
    void read_span_events(size_t step);
    void collect_spans();
    std::vector<std::vector<int64_t>> collect_outputs(GenState& g);
    // decode sessions (engine.cpp, after generate)
    struct Session;
    std::unique_ptr<Session> sess_;
    Session& open_session();
    void session_step_body(Session& s, bool screened, bool stops, bool windowed);
    bool session_head_screened(const Session& s, unsigned carried) const;  // carried: Session::carried()
    // profile_decode: its two timers and the sections after the MoE and attention replays
    double replay_us(int n, const std::function<void()>& body);
    void time_launches(KernelProfile& kp, int n, const std::function<void(int)>& body);
    void profile_gemvs(DecodeProfile& prof, int iters, const std::vector<int>& moe_layers);
    void profile_step_context(DecodeProfile& prof, int iters, int n_moe);
    void layer_forward_prefill(int l, int T, int B, const int* row_page, const int* row_pos, const long* q_off,
                               const long* kv_off, const long* o_off, const int* seq_len, int max_len, int Lmax,
                               const int* past = nullptr, int max_total = 0, bool chunk_attn = false);
    // what both admissions check about the request's parameters, the free slot and the context it needs
    void session_admit_checks(const Session& s, const GenRequest& rq, const GenParams& rp, bool behind_prefix) const;
    // the tail both admissions share: the slot's rows from one staged buffer, then the first selection
    // (slot: where the page's rows are; -1 = the first free slot, s.n.  The caller makes it active)
    int session_admit_tail(Session& s, const GenRequest& rq, const GenParams& rp, const RowParams& row, int slot = -1,
                           bool finish = true);
    struct PendingAdmit;
    void session_slot_move(Session& s, int src, int dst, int rows_bound);

    ModelConfig cfg_;
    int device_ = 0;
    int dtype_ = 1;
    hipStream_t stream_ = nullptr;
    // the page batch's second vision pass (tiles beside the global views) runs on vstream_ with its own
    // workspaces (ws_prefix_): the two towers' small CLIP / norm kernels fill each other's idle CUs
    hipStream_t vstream_ = nullptr;
    hipEvent_t vis_ev_[2] = {nullptr, nullptr};
    std::string ws_prefix_;
    std::vector<void*> allocations_;
    std::map<std::string, std::pair<void*, size_t>> ws_;
    bool capturing_ = false;

    SamW sam_;
    ClipW clip_;
    Qwen2EncW enc_;
    Lin proj_;
    float* newline_ = nullptr;
    float* separator_ = nullptr;
    void* embed_ = nullptr;
    int embed_dt_ = WDT_F16;
    std::vector<DecLayer> layers_;
    float* final_norm_ = nullptr;
    Lin lm_head_;
    void* lm_swz_ = nullptr;         // lm_head in dec_mm fragment order (3..8 pages; made on first use)
    void ensure_mm_weights(int B);
    bool dense_mm_ok(const DecLayer& d, int B) const;
    void* lmq_ = nullptr;            // int8 [vocab][hidden] screening copy of lm_head
    float* lmq_scale_ = nullptr;     // per-row scale
    float* lmq_bound_ = nullptr;     // per-row error-bound factor (times ||x||)
    float* lmq_qnorm_ = nullptr;     // per-row s ||Q|| (3..8 pages: the token rows' int8 representation error)
    void* lmq_frag_ = nullptr;       // the int8 rows in the int8 matrix cores' fragment order (3..8 pages)
    float* rope_cos_ = nullptr;
    float* rope_sin_ = nullptr;
    int rope_cap_ = 0;
    float* ones_ = nullptr;
    int* iota_ = nullptr;
    int small_cap_ = 0;
    // kv cache
    float* kc_ = nullptr;
    float* vc_ = nullptr;
    long page_stride_ = 0, head_stride_ = 0;
    // a session's cache holds kv_pages_ pages per layer whatever the batch a launch runs (0: the launch's own
    // B, as generate sizes it); its prefill writes page kv_page0_
    int kv_pages_ = 0, kv_page0_ = 0;
    long layer_kv(int B) const { return (long)(kv_pages_ ? kv_pages_ : B) * page_stride_; }
    std::set<std::string> ws_frozen_;  // workspaces the session's captured graphs hold: growing one is EINTERNAL
    Timings timings_;
    int vis_stage_ = 0;  // vision_pass / encoder_pass: 0 every stage (the default), 1..3 that stage alone
    size_t chunk_attn_launches_ = 0;
    size_t stop_launches_ = 0;
    std::vector<int> last_stop_hits_;
    std::vector<int> last_guided_;
    double flops_acc_ = 0;  // FLOPs issued by linear() / attention since the last stage mark
    std::vector<int> prefill_lens_;  // rows per page of the prefill being issued
    int last_B_ = 0;
    std::map<std::string, std::pair<void*, size_t>> pinned_;
    std::map<std::pair<int, int>, std::pair<int*, int*>> winmaps_;  // (n, grid) -> tok2win, win2tok
    int last_Lmax_ = 0;
    float* trace_ = nullptr;  // device logits trace of the running generate (parity hook)
    LogprobRows last_lp_;
    int span_mode_ = 0;
    // profile_decode: launches decode_step leaves out (the with / without step-graph differences)
    enum StepSkip : int { SKIP_GATEUP = 1, SKIP_DOWN = 2, SKIP_ATTN = 4 };
    int step_skip_ = 0;
    static bool qkv_attn_fused();
    static bool att_refill_defer();
    static int att_kv_delay();
    unsigned long long* span_slots_ = nullptr;  // device [SPAN_SLOTS][2]
    unsigned long long* span_rec_ = nullptr;    // device [SPAN_KINDS][layers][span_cap_][4]
    const int* span_step_ = nullptr;            // device step counter (out_len of page 0)
    int span_cap_ = 0;
    std::vector<unsigned long long> spans_host_;
    int spans_steps_ = 0;
    std::vector<HipEvent> span_ev_;             // [SPAN_KINDS][layers][2]
    std::vector<double> span_ev_ns_;            // [SPAN_KINDS][layers][span_cap_]
    int spans_kinds_ = SPAN_KINDS;
    bool chain_active_ = false;                 // a SPAN_CHAIN generate is running
    unsigned long long* span_chain_ = nullptr;  // device [layers * SPAN_KINDS_CHAIN][SPAN_SLOTS][2]
    unsigned long long* span_chain_rec_ = nullptr;  // device [span_cap_][layers * SPAN_KINDS_CHAIN][4]
    unsigned long long* span_tmark_ = nullptr;  // device [2]
    unsigned long long* chain_slots(int layer, int kind) const {
        return chain_active_ ? span_chain_ + ((size_t)layer * SPAN_KINDS_CHAIN + kind) * SPAN_SLOTS * 2 : nullptr;
    }
    unsigned long long* span_rec(int kind, int layer) const {
        return span_rec_ + ((size_t)kind * cfg_.lang.layers + layer) * span_cap_ * 4;
    }
    long trace_steps_ = 0;
    bool persist_active_ = false;               // this generate's decode steps run dec_persist
    PersistLayerW* persist_lw_ = nullptr;       // device [layers]
    unsigned long long* persist_g_ = nullptr;   // granules [dec_persist_granules(layers)]
    unsigned long long* persist_stamps_ = nullptr;  // device phase clocks of the last stamped step (optional)
    int persist_stamp_mode_ = 0;                // 1: the next generate records stamps of its decode steps
    int persist_stamp_pos0_ = 0, persist_stamp_cap_ = 0;
    std::vector<unsigned long long> persist_stamps_host_;
    std::vector<HipEvent> persist_ev_;          // [steps][2] HIP events around each persistent launch (timing mode)
    std::vector<double> persist_ev_us_;

    void* dev_alloc(size_t bytes);
    void ensure_rope(int len);
    void ensure_small(int n);
};

}  // namespace dsocr
