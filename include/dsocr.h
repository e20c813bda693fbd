/*
 * dsocr.h — C ABI of the MI355X-native DeepSeek-OCR page engine (gfx950).
 *
 * Drop-in boundary for the reference's `OcrEngine` (TimmyOVO/deepseek-ocr.rs,
 * crates/core/src/inference.rs:189-209) and its loader `load_model`
 * (crates/infer-deepseek/src/model/mod.rs:90-115).  A Rust FFI crate (or the
 * Python mirror in deepseek-ocr.rs_amd/dsocr) binds these symbols; see
 * INTEGRATION.md.  Plain C types only: no torch, no C++ types.
 *
 * Ownership: the caller owns every host buffer it passes; the engine owns its
 * device memory.  An engine handle is Send-not-Sync like the reference engine
 * (server/src/state.rs:22 keeps one behind a Mutex): one thread at a time.
 * Errors: every call returns a dsocr_status; dsocr_last_error() gives the
 * thread-local message.  DSOCR_EINVAL maps to the reference server's HTTP 400
 * ("prompt formatting failed" / "prompt/image embedding mismatch",
 * server/src/generation.rs:108-118), everything else to 500.
 */
#ifndef DSOCR_H
#define DSOCR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    DSOCR_OK = 0,
    DSOCR_EINVAL = 1,    /* bad arguments / prompt-image mismatch (reference: anyhow context -> 400) */
    DSOCR_ENOENT = 2,    /* missing file or tensor */
    DSOCR_EDEVICE = 3,   /* HIP runtime failure / no gfx950 device */
    DSOCR_ENOMEM = 4,    /* device allocation failed */
    DSOCR_EINTERNAL = 5  /* anything else (-> 500) */
} dsocr_status;

/* Reference `Precision` (core/src/runtime.rs:15-19).  F16 = the reference's GPU default:
 * decoder weights rounded bf16->f16, f32 compute. */
typedef enum { DSOCR_F32 = 0, DSOCR_F16 = 1, DSOCR_BF16 = 2 } dsocr_dtype;

typedef struct dsocr_engine dsocr_engine;
typedef struct dsocr_page_pixels dsocr_page_pixels;

/* ModelLoadArgs (core/src/inference.rs:178-186). weights_path == NULL selects the
 * deterministic synthetic checkpoint (seeded, real tensor names/shapes). */
typedef struct {
    const char* config_path;
    const char* weights_path;
    const char* snapshot_path; /* optional .dsq snapshot (crates/dsq): its Q4_K / Q6_K / Q8_0 / float linears
                                  replace the checkpoint's, decoded to fp16 on the GPU at load (dtype must be
                                  DSOCR_F16); NULL = none */
    int device_ordinal;
    dsocr_dtype dtype;
    uint64_t synthetic_seed;
} dsocr_load_args;

/* VisionSettings (core/src/inference.rs:13-18). */
typedef struct {
    uint32_t base_size;
    uint32_t image_size;
    int crop_mode;
} dsocr_vision_settings;

/* DecodeParameters (core/src/inference.rs:21-79) + generation options (model/mod.rs:177-218). */
typedef struct {
    size_t max_new_tokens;
    int do_sample;               /* sampling iff do_sample && temperature > 0 (sampling.rs:67), else greedy */
    double temperature;
    double top_p;                /* active in [0, 1) (apply_top_p); otherwise unset */
    size_t top_k;                /* 0: unset */
    float repetition_penalty;    /* 1.0: off */
    size_t no_repeat_ngram_size; /* 0 or 1: off (reference default 20) */
    uint64_t seed;               /* StdRng::seed_from_u64(seed) when has_seed, else entropy */
    int use_cache;               /* 0: generate_without_cache (model/mod.rs:2051-2283): the whole forward re-runs
                                    on prompt + generated tokens every step (same ids, O(n^2) work) */
    int64_t eos_token_id;        /* < 0: none (reference: config eos_token_id) */
    int ignore_eos;              /* benchmark mode: always produce max_new_tokens */
    int has_seed;                /* DecodeParameters::seed is Some */
} dsocr_decode_params;

/* stream callback: invoked after each generated token (model/mod.rs:1980-1982). */
typedef void (*dsocr_stream_cb)(size_t n_generated, const int64_t* tokens, void* user);

/* One page of a batched generate call. */
typedef struct {
    const int64_t* input_ids;      /* [prompt_len], BOS first (build_prompt_tokens) */
    const uint8_t* image_mask;     /* [prompt_len], 1 on <image> slots; may be NULL if no image */
    size_t prompt_len;
    const dsocr_page_pixels* page; /* if non-NULL the vision tower runs on device for this page */
    const float* image_rows;       /* else: host image embeddings [n_image_rows][hidden] (or NULL) */
    size_t n_image_rows;
} dsocr_request;

typedef struct {
    int64_t* out_ids; /* caller buffer, capacity max_new_tokens */
    size_t cap;
    size_t n_out;
    dsocr_status status;
} dsocr_result;

/* Stage times of the last call, named after the reference Timer events
 * (model/mod.rs:1871,1924,1975,2464,2498). */
typedef struct {
    double vision_prepare_ms;     /* vision.prepare_inputs (host, this call's pages) */
    double vision_compute_ms;     /* vision.compute_embeddings */
    double decode_prefill_ms;     /* decode.prefill */
    double decode_iterative_ms;   /* decode.iterative */
    double decode_generate_ms;    /* decode.generate */
    size_t decode_steps;          /* decode forwards executed */
    size_t pages;
    double vision_flops;          /* algorithmic f32 FLOPs of vision.compute_embeddings (linears 2MNK, */
    double prefill_flops;         /* attention 4 Lq Lk d per head, causal: lower triangle) and of decode.prefill */
} dsocr_timings;

/* ---- engine lifecycle (load_model, model/mod.rs:90-115; DeepseekOcrModel::load 946-1105) */
dsocr_status dsocr_engine_load(const dsocr_load_args* args, dsocr_engine** out);
/* Load flags.  DSOCR_LOAD_PACKED_EXPERTS (needs snapshot_path, else DSOCR_EINVAL): every MoE layer whose routed
 * and shared gate / up / down records are all Q4_K or Q8_0 (one dtype per matrix role) keeps those blocks on
 * the device beside the fp16 copies, and decode steps of 1..8 tokens stream and decode the blocks in the
 * gate/up and down launches instead of the fp16 matrices (each weight is the fp16 value dequant-on-load
 * stores, so only the order of the f32 sums differs).  A layer with any other record kind, prefill, more
 * than 8 tokens, attention, the dense layer and the lm_head run the fp16 kernels as without the flag.
 * dsocr_engine_load(args, out) is dsocr_engine_load_flags(args, flags, out) with flags =
 * DSOCR_LOAD_PACKED_EXPERTS when args carries a snapshot and the environment has DSOCR_DSQ_PACKED set to a
 * non-zero value, else 0. */
#define DSOCR_LOAD_PACKED_EXPERTS 1u
dsocr_status dsocr_engine_load_flags(const dsocr_load_args* args, uint32_t flags, dsocr_engine** out);
/* MoE layers that kept packed blocks, MoE layers in all, device bytes of the packed tables (any may be NULL) */
dsocr_status dsocr_engine_packed_info(const dsocr_engine* e, size_t* packed_layers, size_t* moe_layers,
                                      size_t* packed_bytes);
void dsocr_engine_free(dsocr_engine* e);
const char* dsocr_last_error(void);
/* hidden size (image-row width), vocab, eos id, layers */
dsocr_status dsocr_engine_info(const dsocr_engine* e, size_t* hidden, size_t* vocab, int64_t* eos_token_id,
                               size_t* num_layers);

/* ---- host preprocessing a1-a3 (build_global_view 2308-2330, dynamic_preprocess_with_params
 *      preprocess.rs:67-138, image_to_tensor 2332-2347).  rgb: HWC uint8. */
dsocr_status dsocr_prepare_page(const uint8_t* rgb, uint32_t width, uint32_t height,
                                const dsocr_vision_settings* vs, dsocr_page_pixels** out);
/* a1-a3 on the GPU of `e` (vision/resample.rs + preprocess.rs + model/mod.rs:2295-2347, the same
 * results as dsocr_prepare_page bit for bit): only the RGB8 bytes cross PCIe, the f32 CHW tensors
 * are produced in HBM.  The page's pixels are device-resident only (dsocr_page_pixels_view returns
 * NULL arrays; dsocr_page_read_device copies them back). */
dsocr_status dsocr_prepare_page_device(dsocr_engine* e, const uint8_t* rgb, uint32_t w, uint32_t h,
                                       const dsocr_vision_settings* vs, dsocr_page_pixels** out);
/* ---- model variants behind one engine type (detect_ocr_variant, model/mod.rs:2691-2710): 0 = DeepSeek-OCR,
 *      1 = DeepSeek-OCR-2 (SAM -> Qwen2 decoder as encoder -> projector, vision/qwen2.rs).  A page decides its tile
 *      grid (at most 9 tiles for variant 0, 6 for variant 1, preprocess.rs:27-35) and its <image> slot count (flat
 *      grids without newline slots for variant 1, model/mod.rs:2630-2680) without an engine, so it carries the
 *      variant it was prepared for; a page handed to an engine of the other variant is DSOCR_EINVAL.  Variant 1
 *      views must be 768 or 1024 px (the encoder's two query tables); anything else is DSOCR_EINVAL. */
dsocr_status dsocr_engine_variant(const dsocr_engine* e, int* variant);
/* The same config resolution without an engine or a GPU (host only): the variant of a config.json, SAM's two
 * downsample channel counts after the variant's rule (sam.rs:64-90: the last one is the encoder width for variant 1)
 * and, for variant 1, the encoder's {width, layers, heads, kv_heads, intermediate_size} (zeros for variant 0).
 * Any output may be NULL.  A config the engine would refuse is DSOCR_EINVAL here too. */
dsocr_status dsocr_config_variant(const char* config_path, int* variant, uint32_t* sam_out_channels /* [2] */,
                                  uint32_t* encoder /* [5] */);
dsocr_status dsocr_prepare_page_variant(const uint8_t* rgb, uint32_t width, uint32_t height,
                                        const dsocr_vision_settings* vs, int variant, dsocr_page_pixels** out);
/* dsocr_prepare_page_device for the variant of `e` (dsocr_prepare_page_device itself always prepares variant 0) */
dsocr_status dsocr_prepare_page_device_variant(dsocr_engine* e, const uint8_t* rgb, uint32_t w, uint32_t h,
                                               const dsocr_vision_settings* vs, dsocr_page_pixels** out);
dsocr_status dsocr_page_read_device(const dsocr_page_pixels* p, float* global_out /* [3][G][G] */,
                                    float* tiles_out /* [n_tiles][3][T][T] or NULL */);
void dsocr_page_free(dsocr_page_pixels* p);
/* Stage the page's preprocessed pixels in the engine's device memory (HBM) once, e.g. ahead of
 * a timed or latency-critical generate; later calls gather them device-to-device.  The device
 * copy is owned by the page (freed by dsocr_page_free).  Reference counterpart: none (the
 * reference re-uploads every tensor per call, model/mod.rs:2332-2347). */
dsocr_status dsocr_page_to_device(dsocr_engine* e, dsocr_page_pixels* p);
/* crop grid (w,h), tile count, and the number of <image> slots build_image_placeholders emits */
dsocr_status dsocr_page_info(const dsocr_page_pixels* p, uint32_t* crop_w, uint32_t* crop_h, uint32_t* n_tiles,
                             size_t* n_image_tokens);
/* normalised CHW f32 views: global [3][S][S], tiles [n][3][T][T] (NULL if none) */
dsocr_status dsocr_page_pixels_view(const dsocr_page_pixels* p, const float** global_chw, uint32_t* global_size,
                                    const float** tiles_chw, uint32_t* tile_size);

/* ---- compute_image_embeddings (model/mod.rs:1276-1314): rows [n][hidden] per page,
 *      concatenated into `out` (capacity cap_rows); rows_per_page[i] receives each count. */
dsocr_status dsocr_image_embeddings(dsocr_engine* e, const dsocr_page_pixels* const* pages, size_t n_pages,
                                    float* out, size_t cap_rows, size_t* rows_per_page);

/* ---- generate (model/mod.rs:1870-2048), batch-1 semantics per page */
dsocr_status dsocr_generate(dsocr_engine* e, const dsocr_request* req, const dsocr_decode_params* params,
                            dsocr_stream_cb cb, void* user, int64_t* out_ids, size_t cap, size_t* n_out);
/* B pages at once (vision batched, prefill batched, decode batched); each result equals dsocr_generate. */
dsocr_status dsocr_generate_batch(dsocr_engine* e, size_t n, const dsocr_request* reqs,
                                  const dsocr_decode_params* params, dsocr_result* results);
dsocr_status dsocr_last_timings(const dsocr_engine* e, dsocr_timings* t);
/* Parity hook: dsocr_generate_batch plus the raw logits (before repetition penalty and n-gram ban) of
 * every step of every page, logits_out [n][max_new_tokens][vocab] host f32, step s = the logits the
 * s-th generated token was selected from (step 0 = the prefill's last row).  The reference's
 * counterparts: the cli-debug top-2 logits dump (crates/infer-deepseek/src/debug.rs:17-21,
 * model/mod.rs:1937-1949) and the teacher-forcing logits its baseline tests compare
 * (tests/baseline.rs:1108).  Selection runs on the exact lm_head while tracing (the screened head
 * never forms the full logits; its ids equal the exact head's).  logits_cap = capacity of logits_out in
 * floats; DSOCR_EINVAL (nothing written) when n * max_new_tokens * vocab exceeds it. */
dsocr_status dsocr_generate_trace(dsocr_engine* e, size_t n, const dsocr_request* reqs,
                                  const dsocr_decode_params* params, dsocr_result* results, float* logits_out,
                                  size_t logits_cap);

/* Per-token log-probabilities.  dsocr_generate_batch plus, for every id a page emits and at the same index, its
 * log-probability and the top_k (0 .. DSOCR_MAX_TOP_LOGPROBS) most likely alternatives, reduced on the device inside
 * the decode step: lp = l[tok] - m - log sum_v exp(l[v] - m) over the finite raw logits l of the exact lm_head (f32,
 * before repetition penalty, n-gram ban and temperature: the values dsocr_generate_trace exposes), m their maximum;
 * -inf when l[tok] is not finite or the row has no finite entry.  Alternatives: the largest raw logits, descending,
 * the lower id first on equal values, each with its own log-probability; (-1, -inf) past the last finite entry.
 * An EOS that is not emitted has no entry.  Selection runs on the exact lm_head (as while tracing); the ids equal
 * dsocr_generate_batch's.  lp[i] are caller buffers of page i: token_lp [cap], top_id / top_lp [cap][top_k] (may be
 * NULL when top_k == 0), cap >= max_new_tokens; n is set on return.  use_cache = 0 is DSOCR_EINVAL. */
#define DSOCR_MAX_TOP_LOGPROBS 20
typedef struct {
    float* token_lp;
    int64_t* top_id;
    float* top_lp;
    size_t cap;
    size_t n;
} dsocr_logprobs;
dsocr_status dsocr_generate_logprobs(dsocr_engine* e, size_t n, const dsocr_request* reqs,
                                     const dsocr_decode_params* params, dsocr_result* results, size_t top_k,
                                     dsocr_logprobs* lp);

/* ---- per-request logit bias and token allow / deny sets.  A constraint belongs to one request: n pairs
 * (ids[i], values[i]) and the flag allow_only.  The exact lm_head's f32 logits row l of that request becomes
 * l' = l + b with b[ids[i]] = values[i] and, for every id not listed, b = 0 (allow_only == 0) or -inf (allow_only
 * != 0).  An allow list is allow_only = 1 with values 0; a deny list is allow_only = 0 with values -inf.  l' replaces
 * l for everything downstream, in this order: the log-probability partials (log-probabilities and alternatives are
 * those of the constrained distribution), the repetition penalty, the n-gram ban, greedy or stochastic selection.
 * A -inf entry behaves exactly like an n-gram-banned token under select_token_id: argmax_first skips it, in the
 * fallbacks too, and the sampler gives it weight 0, so a denied id is never emitted while any id of the row has a
 * finite l'; if none has, the reference's last resort (id 0) stands.
 * Checked on the host before any device state changes, each DSOCR_EINVAL: an id outside [0, vocab), a duplicate id,
 * a NaN or +inf value, allow_only with n == 0, n > vocab.  n == 0 with allow_only == 0 (or a NULL pointer where one
 * is taken) is "no constraint".  A call or session burst in which any active page carries a constraint runs the
 * exact lm_head and selectors (as log-probabilities do); a page without one in such a batch produces bit for bit
 * the ids and log-probability entries it produces alone.  A constraint together with the logits trace, use_cache = 0
 * or the persistent step (DSOCR_PERSIST) is DSOCR_EINVAL.  With no constraint anywhere nothing changes.
 *   dsocr_logit_bias_check: the checks alone, against a vocabulary size; needs no engine and no device.
 *   dsocr_generate_logit_bias: dsocr_generate_batch with one constraint per request (bias [n], entries may be
 *   NULL; bias itself NULL: none).  lp != NULL: also dsocr_generate_logprobs' entries with top_k alternatives
 *   (lp NULL: top_k must be 0).
 *   dsocr_session_stage_logit_bias: stages one constraint (copied) for the NEXT admission call on this engine's
 *   session, whichever form it takes: dsocr_session_admit, _admit_params, _admit_prefix or _admit_begin (the
 *   constraint then belongs to the chunked admission: it is applied by the slice that makes the first selection,
 *   and dsocr_session_admit_cancel drops it with the admission).  That call consumes it whether it succeeds or not;
 *   staging again before it replaces it, and lb == NULL (or "no constraint") clears it.  DSOCR_EINVAL, nothing
 *   staged, when the list fails a check, no session is open, or the session was opened without
 *   DSOCR_SESSION_LOGIT_BIAS. */
typedef struct {
    const int64_t* ids;
    const float* values;
    size_t n;
    int allow_only;
} dsocr_logit_bias;
dsocr_status dsocr_logit_bias_check(const dsocr_logit_bias* lb, size_t vocab);
dsocr_status dsocr_generate_logit_bias(dsocr_engine* e, size_t n, const dsocr_request* reqs,
                                       const dsocr_decode_params* params, dsocr_result* results,
                                       const dsocr_logit_bias* const* bias, size_t top_k, dsocr_logprobs* lp);
dsocr_status dsocr_session_stage_logit_bias(dsocr_engine* e, const dsocr_logit_bias* lb);

/* ---- stop sequences matched inside the decode step, per request.  A stop set belongs to one request.  It holds n
 * sequences (1 <= n <= DSOCR_MAX_STOP_SEQS = 16), each of 1 .. DSOCR_MAX_STOP_LEN = 32 token ids in [0, vocab).
 *   When a match fires.  After a step appends token number L to a page's output, sequence s of length m <= L matches
 *   when out[L-m .. L) == s.  The prompt is never matched against.  Only the tail is looked at, because one token
 *   arrives per step.
 *   What a match does.  The page is done from that step on, exactly as for EOS.  No later step appends a token, a
 *   context id or a log-probability entry for it.
 *   What is recorded.  The page records (seq, match_len) with seq the lowest matching index.
 *   EOS in the same step.  A step in which EOS was selected emits nothing and therefore matches nothing.
 *   max_new_tokens in the same step.  A stop that completes on the step that also reaches max_new_tokens still
 *   records its hit.
 *   No trimming on the device.  out_len, the ids that dsocr_session_retire and dsocr_generate* return, and the
 *   log-probability entries all include the matched tokens.  Trimming is the caller's job.
 *   Selection is untouched.  Stops never change which token is selected.  A page's ids are a prefix of the ids it
 *   produces without stops, for any head, any batch and any neighbour.
 *   Heads.  Stops do not force the exact head; the screened head keeps running where it runs today.
 *   Refusals.  A stop set together with the logits trace, use_cache = 0 or with the persistent step (DSOCR_PERSIST=1
 *   in the environment, whether or not that step would fit the model) is DSOCR_EINVAL.
 *   Off by default.  With no stop set anywhere, nothing is launched and nothing changes.
 * The match is one launch (dec_stop_match, one wave per page) right after the step's final selection kernel, and after
 * the first selection a prefill or an admission makes; it writes the done word EOS writes.
 * dsocr_stop_set_check: the checks alone, against a vocabulary size; needs no engine and no device.  Each of these is
 * DSOCR_EINVAL, before any device state changes: n > 16, a length of 0 or above 32, an id outside [0, vocab), two
 * identical sequences.  n == 0 or a NULL pointer means "no stops".
 * dsocr_generate_stop: dsocr_generate_logit_bias with one stop set per request (stops [n], entries may be NULL;
 * stops itself NULL: none) and the hits [n] (may be NULL); bias and lp may be NULL (lp NULL: top_k must be 0).  The call
 * polls the done words every 8 steps (under ignore_eos too, and once before the first step), so decode_steps of
 * dsocr_last_timings is 0 when every page stopped on its first token and else the steps run when the poll saw every
 * page done: the first multiple of 8 at or behind the last page's end, at most max_new_tokens - 1.  It takes no
 * stream callback.
 * dsocr_generate_stop_stream: dsocr_generate, one page with its stream callback, with a stop set (NULL: none) and
 * the hit (may be NULL).  The callback sees the tokens as they are emitted, matched ones included: holding back a
 * tail that may still become a stop is the caller's job.  With a callback the done word is polled after every step,
 * so decode_steps is the number of steps up to the match.
 * dsocr_session_stage_stop: stages one stop set (copied) for the NEXT admission call on this engine's session,
 * whichever form it takes, exactly like dsocr_session_stage_logit_bias: that call consumes it whether it succeeds or
 * not, a chunked admission owns it until its last slice applies it (dsocr_session_admit_cancel drops it), staging
 * again replaces it, NULL or n == 0 clears it.  DSOCR_EINVAL, nothing staged, when the set fails a check, no session
 * is open, or the session was opened without DSOCR_SESSION_STOP.
 * dsocr_session_stop_hit: the hit of a live slot (it follows its page through the compaction of
 * dsocr_session_retire); seq = -1 while no stop has fired within the slot's own max_new_tokens.
 * dsocr_stop_launches: match launches of this engine so far, issued or replayed inside a step graph (0 for ever
 * while no request carries a stop set). */
#define DSOCR_MAX_STOP_SEQS 16
#define DSOCR_MAX_STOP_LEN 32
typedef struct {
    const int64_t* ids; /* the sequences back to back */
    const size_t* lens;
    size_t n;
} dsocr_stop_set;
typedef struct {
    int32_t seq; /* -1: no stop fired */
    int32_t match_len;
} dsocr_stop_hit;
dsocr_status dsocr_stop_set_check(const dsocr_stop_set* stops, size_t vocab);
dsocr_status dsocr_generate_stop(dsocr_engine* e, size_t n, const dsocr_request* reqs, const dsocr_decode_params* params,
                                 dsocr_result* results, const dsocr_stop_set* const* stops, dsocr_stop_hit* hits,
                                 const dsocr_logit_bias* const* bias, size_t top_k, dsocr_logprobs* lp);
dsocr_status dsocr_generate_stop_stream(dsocr_engine* e, const dsocr_request* req, const dsocr_decode_params* params,
                                        const dsocr_stop_set* stops, dsocr_stream_cb cb, void* user, int64_t* out_ids,
                                        size_t cap, size_t* n_out, dsocr_stop_hit* hit);
dsocr_status dsocr_session_stage_stop(dsocr_engine* e, const dsocr_stop_set* stops);
dsocr_status dsocr_session_stop_hit(dsocr_engine* e, int slot, dsocr_stop_hit* out);
dsocr_status dsocr_stop_launches(const dsocr_engine* e, size_t* n);

/* ---- frequency / presence penalties and min-p, per request (no reference counterpart: the
 * reference has the multiplicative repetition_penalty only).  With c[t] the number of times id t occurs in the page's
 * GENERATED tokens so far (the prefill's own selection included; prompt and image slots do not count), every step's
 * logits become l[t] - (frequency * c[t] + presence) where c[t] > 0, in f32 with each operation rounded, after the
 * logit bias, the log-probability partials and the repetition penalty, before the n-gram ban and the selection.
 * min_p acts on sampled rows only: a candidate stays iff logit / T - max(logit / T) >= log(min_p), the maximum taken
 * over the finite logits the n-gram ban leaves; top-k, top-p and the draw then run on the survivors.  Off:
 * frequency == 0, presence == 0 and min_p <= 0 (a NULL record too).  A call or burst in which a record is on runs
 * the exact lm_head and selectors.  DSOCR_EINVAL, before any device state changes: a non-finite frequency or
 * presence; min_p NaN, below 0 or above 1; a record that is on with the logits trace, use_cache = 0 or DSOCR_PERSIST.
 *   dsocr_penalties_check: the checks alone; needs no engine and no device.
 *   dsocr_generate_penalties: dsocr_generate_stop with one record per request (pen [n], entries may be NULL; pen
 *   itself NULL: none).
 *   dsocr_session_stage_penalties: stages one record (copied) for the NEXT admission call on this engine's session,
 *   whichever form it takes, exactly like dsocr_session_stage_stop.  DSOCR_EINVAL, nothing staged, when the record
 *   fails a check, no session is open, or it is on and the session was opened without DSOCR_SESSION_PENALTIES. */
typedef struct {
    float frequency;
    float presence;
    double min_p;
} dsocr_penalties;
dsocr_status dsocr_penalties_check(const dsocr_penalties* pen);
dsocr_status dsocr_generate_penalties(dsocr_engine* e, size_t n, const dsocr_request* reqs,
                                      const dsocr_decode_params* params, dsocr_result* results,
                                      const dsocr_penalties* const* pen, const dsocr_stop_set* const* stops,
                                      dsocr_stop_hit* hits, const dsocr_logit_bias* const* bias, size_t top_k,
                                      dsocr_logprobs* lp);
dsocr_status dsocr_session_stage_penalties(dsocr_engine* e, const dsocr_penalties* pen);

/* ---- windowed no-repeat n-gram ban with a token whitelist, per request (no reference counterpart:
 * the reference's no_repeat_ngram_size looks through the whole context).  A record {ngram_size g, window w,
 * whitelist[0..k)} is off when it is NULL or g < 2.  With ctx[0..n) the page's context row (prompt and generated
 * ids: what the plain ban reads) and n >= g: for every start i with max(0, n - w) <= i <= n - g and
 * ctx[i .. i+g-1) == ctx[n-g+1 .. n), the id t = ctx[i+g-1] is a candidate; a candidate outside [0, vocab) or in the
 * whitelist is skipped, every other one gets l[t] = -inf.  A ban that would leave the row without a finite logit is
 * dropped for that step (sampling.rs:61-63).  With w >= n and an empty whitelist this is the plain ban.  The window
 * counts context positions, prompt included: the upstream vLLM processor counts generated tokens only, so the two
 * differ while the window still reaches into the prompt.  The step order: lm_head, logit bias, log-probability
 * partials, repetition penalty, frequency / presence, this ban (in the plain ban's place), selection.  A record that
 * is on replaces the request's no_repeat_ngram_size: the plain ban is not applied on top of it.  A call or burst in
 * which a record is on runs the exact lm_head and selectors.  DSOCR_EINVAL, before any device state changes: w < 1
 * with g >= 2 (w < g is legal and never matches); more than DSOCR_MAX_NGRAM_WHITELIST distinct ids (repeats count
 * once); a whitelist id outside [0, vocab); a record that is on with the logits trace, use_cache = 0 or DSOCR_PERSIST.
 *   dsocr_ngram_window_check: the record's own checks against `vocab`; needs no engine and no device.
 *   dsocr_generate_ngram_window: dsocr_generate_penalties with one record per request (ngw [n], entries may be
 *   NULL; ngw itself NULL: none).
 *   dsocr_session_stage_ngram_window: stages one record (copied) for the NEXT admission call on this engine's
 *   session, whichever form it takes, exactly like dsocr_session_stage_penalties.  DSOCR_EINVAL, nothing staged, when
 *   the record fails a check, no session is open, or it is on and the session was opened without
 *   DSOCR_SESSION_NGRAM_WINDOW. */
#define DSOCR_MAX_NGRAM_WHITELIST 32
typedef struct {
    int32_t ngram_size;
    int32_t window;
    const int32_t* whitelist;
    size_t n_whitelist;
} dsocr_ngram_window;
dsocr_status dsocr_ngram_window_check(const dsocr_ngram_window* ngw, size_t vocab);
dsocr_status dsocr_generate_ngram_window(dsocr_engine* e, size_t n, const dsocr_request* reqs,
                                         const dsocr_decode_params* params, dsocr_result* results,
                                         const dsocr_ngram_window* const* ngw, const dsocr_penalties* const* pen,
                                         const dsocr_stop_set* const* stops, dsocr_stop_hit* hits,
                                         const dsocr_logit_bias* const* bias, size_t top_k, dsocr_logprobs* lp);
dsocr_status dsocr_session_stage_ngram_window(dsocr_engine* e, const dsocr_ngram_window* ngw);

/* ---- guided decoding: a per-request token automaton (no reference counterpart).  The request carries n_states
 * states, a start state, one byte per state (accepting: the request's EOS id may be selected there) and the edges in
 * CSR form: the edges of state s are row_ptr[s] .. row_ptr[s + 1] - 1, edge_tok strictly ascending within a state,
 * edge_next the state an edge leads to.  A state without an outgoing edge is terminal.  In every step (the prefill's
 * own selection included) a page in state s gets l[t] = -inf for every id t without an edge from s, except its EOS
 * id, which is kept iff accepting[s]; ids with an edge keep their logits bit for bit.  The step order: lm_head, logit
 * bias, this mask, log-probability partials (entries and alternatives are those of the constrained distribution),
 * repetition penalty, frequency / presence, n-gram ban, selection, the advance, the stop match.  The advance: when the
 * step appended a token, the state follows its edge; arriving at a terminal state ends the page (status 1, complete);
 * a token without an edge, which only the selection's last resort (id 0 when no finite logit remains) can produce,
 * ends it with state -1 and status 2 (violated).  A call or burst in which a page carries an automaton runs the exact
 * lm_head and selectors; a page without one in such a batch keeps its ids and log-probability entries bit for bit.
 * DSOCR_EINVAL, before any device state changes: n_states outside [1, DSOCR_MAX_GUIDED_STATES]; more than
 * DSOCR_MAX_GUIDED_EDGES edges; row_ptr not non-decreasing from 0; an edge token outside [0, vocab) or equal to the
 * request's EOS id; tokens not strictly ascending within a state; edge_next or start outside [0, n_states); a
 * terminal start; a NULL array; an automaton with use_cache = 0 or DSOCR_PERSIST.  (The logits trace cannot be asked
 * for together with an automaton: dsocr_generate_trace takes none.)  Under ignore_eos no id is the EOS id.
 *   dsocr_guided_check: the record's own checks against `vocab` and `eos` (negative: none); needs no engine and no
 *   device.
 *   dsocr_generate_guided: dsocr_generate_ngram_window with one automaton (guided [n], entries may be NULL; guided
 *   itself NULL: none) and one result (gres [n] or NULL) per request.
 *   dsocr_session_stage_guided: stages one automaton (copied) for the NEXT admission call on this engine's session,
 *   whichever form it takes, exactly like dsocr_session_stage_ngram_window; a chunked admission keeps it on the host
 *   until its last slice.  DSOCR_EINVAL, nothing staged, when the record fails a check that needs no EOS id, no
 *   session is open, or the session was opened without DSOCR_SESSION_GUIDED; the EOS rule is checked by the admission.
 *   dsocr_session_guided_state: the state and status of a live slot ({0, 0} for a page without an automaton); it
 *   follows its page through the compaction of dsocr_session_retire. */
#define DSOCR_MAX_GUIDED_STATES 1024
#define DSOCR_MAX_GUIDED_EDGES (1 << 20)
typedef struct {
    int32_t n_states, start;
    const uint8_t* accepting;    /* [n_states] */
    const int32_t *row_ptr, *edge_tok, *edge_next; /* [n_states + 1], [E], [E] with E = row_ptr[n_states] */
} dsocr_guided;
typedef struct {
    int32_t state;   /* the automaton state after the last appended token (-1: violated) */
    int32_t status;  /* 0 running, or cut by max_new_tokens / EOS / a stop; 1 complete; 2 violated */
} dsocr_guided_result;
dsocr_status dsocr_guided_check(const dsocr_guided* g, int vocab, long long eos);
dsocr_status dsocr_generate_guided(dsocr_engine* e, size_t n, const dsocr_request* reqs,
                                   const dsocr_decode_params* params, dsocr_result* results,
                                   const dsocr_guided* const* guided, dsocr_guided_result* gres,
                                   const dsocr_ngram_window* const* ngw, const dsocr_penalties* const* pen,
                                   const dsocr_stop_set* const* stops, dsocr_stop_hit* hits,
                                   const dsocr_logit_bias* const* bias, size_t top_k, dsocr_logprobs* lp);
dsocr_status dsocr_session_stage_guided(dsocr_engine* e, const dsocr_guided* g);
dsocr_status dsocr_session_guided_state(dsocr_engine* e, int slot, dsocr_guided_result* out);

/* ---- decode sessions: pages join and leave a running batch between decode steps (no reference counterpart: the
 * reference server decodes one request at a time behind its Mutex, server/src/state.rs:22).  A session is a
 * long-lived batch of `slots` (1..8) pages with max_context rows each (a page needs prompt_len + max_new_tokens
 * + 1).  Between bursts of decode steps a page is admitted (vision + prefill into its own slot; the other slots'
 * state is untouched) or retired.  Active pages always occupy slots [0, active): retiring slot i < active - 1
 * moves the last active page into slot i (one device launch), which dsocr_session_retire reports in *moved_from.
 * Every page's ids equal dsocr_generate of that page alone with that page's parameters and seed, whatever else
 * is in the batch.
 *   dsocr_session_open: params are fixed for the session (do_sample, temperature, top_k, top_p,
 *   repetition_penalty, no_repeat_ngram_size, eos_token_id, ignore_eos; use_cache must be non-zero);
 *   params->max_new_tokens is the session's output capacity, the upper bound of a request's own max_new_tokens.
 *   Per request only max_new_tokens and the seed vary.
 *   dsocr_session_open_ex with DSOCR_SESSION_PER_REQUEST: params are the defaults (dsocr_session_admit uses them)
 *   and params->max_new_tokens is still the output capacity; dsocr_session_admit_params gives a page its own
 *   do_sample / temperature / top_k / top_p / repetition_penalty / no_repeat_ngram_size / eos_token_id /
 *   ignore_eos beside max_new_tokens and the seed.  The parameters live in one device record per slot that the
 *   selection kernels read per row.  Each burst runs under one lm_head + selection head: the screened one while
 *   every active page is greedy without a repetition penalty (where a fixed greedy session would use it), else
 *   the exact one with both the greedy and the sampling selector; dsocr_session_head_steps counts both.
 *   Launch spans, the persistent step and the logits trace are off.
 *   dsocr_generate / _batch / _trace / dsocr_profile_decode on an engine with an open session are DSOCR_EINVAL,
 *   and so is opening a second session.
 *   A finished page keeps its slot until it is retired, and every step appends one K/V row to every active slot:
 *   retire finished pages after every step call.  dsocr_session_step replays at most 8 steps (fewer where a slot
 *   would run out of cache rows; DSOCR_EINVAL before any launch when a slot has none left). */
typedef struct {
    int32_t slot;     /* 0 .. active - 1 */
    int32_t done;     /* eos was selected, or out_len reached the request's max_new_tokens */
    int32_t out_len;  /* tokens generated so far (at most the request's max_new_tokens) */
    int32_t n_new;    /* tokens since the last poll: the next n_new entries of `tokens` */
} dsocr_slot_status;
typedef struct {
    size_t slots, active, max_context, out_cap;
    size_t kv_cap;     /* cache rows per slot: max_context + burst_cap */
    size_t burst_cap;  /* most steps one dsocr_session_step replays */
    size_t steps;      /* decode steps replayed since the session opened */
    size_t flags;      /* the DSOCR_SESSION_* flags the session was opened with (| DSOCR_SESSION_ADMIT_PENDING) */
} dsocr_session_desc;
dsocr_status dsocr_session_open(dsocr_engine* e, size_t slots, size_t max_context, const dsocr_decode_params* params);
/* flags = 0: dsocr_session_open.  Unknown flag bits are DSOCR_EINVAL. */
#define DSOCR_SESSION_PER_REQUEST 1u
/* DSOCR_SESSION_LOGPROBS (combines with DSOCR_SESSION_PER_REQUEST): every slot keeps out_cap log-probability entries
 * with DSOCR_MAX_TOP_LOGPROBS alternatives each (see dsocr_generate_logprobs), written by every step and by the
 * admission's first selection; the exact head runs at every active count. */
#define DSOCR_SESSION_LOGPROBS 2u
/* DSOCR_SESSION_LOGIT_BIAS (combines with both flags above): every slot keeps a dense f32 bias row (vocab floats,
 * reserved at open), the add launch is part of the exact step, and an admission may carry a constraint
 * (dsocr_session_stage_logit_bias).  A burst runs the exact head iff an active slot carries a constraint
 * (dsocr_session_head_steps shows it); the constraint follows its page through the compaction of
 * dsocr_session_retire (the row is copied) and ends with the page. */
#define DSOCR_SESSION_LOGIT_BIAS 4u
/* DSOCR_SESSION_STOP (combines with the three flags above): every slot keeps a stop table (16 x 33 int32, reserved
 * at open) with its count, examined length and hit, and an admission may carry a stop set
 * (dsocr_session_stage_stop).  The step graph of a burst contains the match launch iff an active slot carries a stop
 * set; the head is whichever runs without it.  A stop that fires in the middle of a burst leaves out_len at the match. */
#define DSOCR_SESSION_STOP 8u
/* DSOCR_SESSION_PENALTIES (combines with the four flags above): every slot keeps a 16-byte penalty record (reserved
 * at open, off until an admission brings one: dsocr_session_stage_penalties), and the penalty launch is part of the
 * exact step.  A burst runs the exact head iff an active slot carries a record that is on; the record follows its
 * page through the compaction of dsocr_session_retire and ends with the page. */
#define DSOCR_SESSION_PENALTIES 16u
/* DSOCR_SESSION_NGRAM_WINDOW (combines with the five flags above): every slot keeps a 144-byte windowed-ban record
 * (reserved at open, off until an admission brings one: dsocr_session_stage_ngram_window).  A burst runs the exact
 * head with the window launch iff an active slot carries a record that is on; the record follows its page through
 * the compaction of dsocr_session_retire and ends with the page. */
#define DSOCR_SESSION_NGRAM_WINDOW 32u
/* DSOCR_SESSION_GUIDED (combines with the six flags above): every slot keeps the tables of a token automaton at the
 * caps (a bitmask of 1024 x ceil(vocab / 32) words and 1025 + 2 x 2^20 int32 of edges: about 25 MB per slot at a
 * vocabulary of 129280, reserved at open), and an admission may carry one (dsocr_session_stage_guided).  A burst runs
 * the exact head, with the mask and advance launches, iff an active slot carries an automaton; the tables follow
 * their page through the compaction of dsocr_session_retire (the used part is copied) and end with the page. */
#define DSOCR_SESSION_GUIDED 64u
dsocr_status dsocr_session_open_ex(dsocr_engine* e, size_t slots, size_t max_context, const dsocr_decode_params* params,
                                   uint32_t flags);
/* Every check (free slot, context need, prompt/image mismatch, token ids, page variant) happens before any device
 * state changes; on an error the running slots are as they were.  *slot receives the page's slot (= active before). */
dsocr_status dsocr_session_admit(dsocr_engine* e, const dsocr_request* req, size_t max_new_tokens, int has_seed,
                                 uint64_t seed, int* slot);
/* dsocr_session_admit with the request's whole parameter set: params->max_new_tokens (1 .. the session's capacity),
 * has_seed / seed and everything select_token_id reads (use_cache must be non-zero).  On a session opened without
 * DSOCR_SESSION_PER_REQUEST it is DSOCR_EINVAL when params differ from the session's in more than max_new_tokens
 * and the seed.  Like dsocr_session_admit, every check runs before any device state changes. */
dsocr_status dsocr_session_admit_params(dsocr_engine* e, const dsocr_request* req, const dsocr_decode_params* params,
                                        int* slot);
/* decode steps replayed under the screened / the exact head since the session opened (either pointer may be NULL;
 * both session kinds).  DSOCR_EINVAL when no session is open. */
dsocr_status dsocr_session_head_steps(const dsocr_engine* e, size_t* screened, size_t* exact);
/* up to k decode steps for the active pages, then one poll.  status [cap_slots >= slots], tokens
 * [cap_tokens >= slots * out_cap]: the new tokens of slot 0, then slot 1, ... (DSOCR_EINVAL if either is short) */
dsocr_status dsocr_session_step(dsocr_engine* e, size_t k, dsocr_slot_status* status, size_t cap_slots, size_t* n_slots,
                                int64_t* tokens, size_t cap_tokens, size_t* n_tokens);
dsocr_status dsocr_session_poll(dsocr_engine* e, dsocr_slot_status* status, size_t cap_slots, size_t* n_slots,
                                int64_t* tokens, size_t cap_tokens, size_t* n_tokens);
/* the page's ids (truncated to its max_new_tokens) and its slot freed; *moved_from (optional): -1, or the slot
 * whose page now lives in `slot` */
dsocr_status dsocr_session_retire(dsocr_engine* e, int slot, int64_t* out_ids, size_t cap, size_t* n_out,
                                  int* moved_from);
/* entries [first, first + count) of a live slot: token_lp [count], top_id / top_lp [count][top_k], top_k <=
 * DSOCR_MAX_TOP_LOGPROBS.  DSOCR_EINVAL when the session was opened without DSOCR_SESSION_LOGPROBS or the range
 * passes the slot's out_len.  dsocr_session_retire does not return them: read them before it. */
dsocr_status dsocr_session_logprobs(dsocr_engine* e, int slot, size_t first, size_t count, size_t top_k, float* token_lp,
                                    int64_t* top_id, float* top_lp);
/* ---- page prefix cache: the K/V rows of a prompt's first `rows` positions (BOS and the page's image rows) kept
 * beside the session, so that a later prompt on the same page skips vision and the prefill of those rows.
 *   dsocr_session_prefix_keep: copies rows [0, rows) of a live slot (1 <= rows <= the slot's prompt length; prompt
 *   rows never change after the admission, so the slot may have decoded any number of steps) into a new entry that
 *   also keeps the prompt's first `rows` ids and mask bytes.  The entry lives in its own device allocation until
 *   dsocr_session_prefix_drop or dsocr_session_close; a session holds at most DSOCR_MAX_PREFIX_ENTRIES.
 *   DSOCR_ENOMEM when the allocation fails, DSOCR_EINVAL for a bad slot / rows or a full table.
 *   dsocr_session_admit_prefix: dsocr_session_admit_params for a request whose prompt starts with the entry's:
 *   req carries ids and mask of the WHOLE prompt and neither a page nor image rows.  Every check runs before any
 *   device state changes: the checks of dsocr_session_admit_params, prompt_len >= rows + 1 (the last row's logits
 *   come from a new row), ids and mask equal to the entry's over [0, rows), no mask byte set from `rows` on.  Then
 *   the entry is copied into the new slot and only rows [rows, prompt_len) are prefilled behind it.
 *   dsocr_session_prefix_stats: entries alive, device bytes they hold, prefix admissions and the rows those
 *   admissions did not prefill, since the session opened (any pointer may be NULL). */
#define DSOCR_MAX_PREFIX_ENTRIES 64
dsocr_status dsocr_session_prefix_keep(dsocr_engine* e, int slot, size_t rows, int* handle);
dsocr_status dsocr_session_admit_prefix(dsocr_engine* e, int handle, const dsocr_request* req,
                                        const dsocr_decode_params* params, int* slot);
dsocr_status dsocr_session_prefix_drop(dsocr_engine* e, int handle);
dsocr_status dsocr_session_prefix_stats(const dsocr_engine* e, size_t* entries, size_t* bytes, size_t* admissions,
                                        size_t* rows_reused);
/* ---- chunked admission: dsocr_session_admit_params in slices, so that dsocr_session_step can run between them and a
 * running stream never waits for a whole vision + prefill.  Off unless called: the calls above launch what they did.
 *   dsocr_session_admit_begin: every check of dsocr_session_admit_params, then DSOCR_EINVAL when chunk_rows < 32, an
 *   admission is already pending or no slot is free.  Launches nothing; *ticket numbers the admission.  req->page
 *   must stay alive until the admission completes or is cancelled (ids, mask and image rows are copied).
 *   dsocr_session_admit_advance: exactly one slice, synchronised.  Slices: the vision of the page in three (SAM;
 *   CLIP or the OCR2 encoder; projector and the image-row plan.  None without a page; one slice for a tiled page
 *   when DSOCR_VIS_STREAMS=0 makes both vision passes share their workspaces), then the prompt in chunks of chunk_rows rows, each a prefill of its rows behind the rows already
 *   appended (the first is the plain causal prefill; the others attend through the query-tiled kernel of
 *   dsocr_k_attention_chunk).  The last chunk also makes the first selection and sets *done = 1 and *slot (= active
 *   before); until then *done = 0 and *slot = -1.  A slice that fails ends the admission.
 *   dsocr_session_admit_cancel: forgets the pending admission; nothing a later step or admission reads was changed.
 *   While an admission is pending the page is staged in the last slot: dsocr_session_step, _poll, _retire (with its
 *   compaction), _logprobs and _prefix_keep stay legal, dsocr_session_admit* and _admit_prefix are DSOCR_EINVAL,
 *   dsocr_session_close drops it, dsocr_session_info reports DSOCR_SESSION_ADMIT_PENDING in flags and
 *   dsocr_session_admit_progress the prompt rows prefilled, the prompt's rows, the slices run and the vision stage
 *   the next slice runs (1..3, 0: none left); *chunk_attn_launches counts the engine's launch_attention_chunk
 *   launches so far, pending or not (any pointer may be NULL).  The session descriptor's layout is unchanged.  The ids of every page equal a plain admission's. */
#define DSOCR_SESSION_ADMIT_PENDING 0x100u
dsocr_status dsocr_session_admit_begin(dsocr_engine* e, const dsocr_request* req, const dsocr_decode_params* params,
                                       size_t chunk_rows, int* ticket);
dsocr_status dsocr_session_admit_advance(dsocr_engine* e, int* done, int* slot);
dsocr_status dsocr_session_admit_cancel(dsocr_engine* e);
dsocr_status dsocr_session_admit_progress(const dsocr_engine* e, int* pending, size_t* rows_done, size_t* rows_total,
                                          size_t* slices, int* vision_stage, size_t* chunk_attn_launches);
dsocr_status dsocr_session_close(dsocr_engine* e);
/* DSOCR_EINVAL when no session is open */
dsocr_status dsocr_session_info(const dsocr_engine* e, dsocr_session_desc* out);

/* Decode-kernel profile (bench roofline): replays the dominant decode kernels of the
 * last generate() call on its final routing / KV state, each timed with HIP events on
 * the engine stream.  avg_us = mean duration of one launch; bytes / flops = algorithmic
 * HBM traffic / work of one launch (fp16 weights touched + f32 activations / KV reads). */
typedef struct dsocr_kernel_profile {
    double avg_us;     /* one launch between its own pair of events (the begin-to-end rocprofv3 reports) */
    double bytes;
    double flops;
    int launches;
    double replay_us;  /* per launch in a back-to-back hipGraph replay (incl. the kernel boundary) */
    double ctx_us;     /* in context: (one decode step's layers replayed as a hipGraph - the same graph without this
                          launch in any layer) / its launches per step, i.e. what it costs inside the real step
                          chain, its own dispatch included (MoE gate/up, MoE down, attention; else 0) */
} dsocr_kernel_profile;
typedef struct dsocr_decode_profile {
    dsocr_kernel_profile moe_gateup;  /* decode MoE gate/up launch(es) of one layer (routed + shared): the kernel
                                         the dispatch picks at this batch size, named in moe_gateup_kernel */
    dsocr_kernel_profile moe_down;    /* routed + shared down + combine + residual (moe_down_kernel) */
    dsocr_kernel_profile attention;   /* dec_attn_kernel (RoPE / KV append / flash-decoding / combine): one layer */
    dsocr_kernel_profile lm_head;     /* exact lm_head over the 129280 x 1280 rows: dec_gemv_stream (1-2 pages) or
                                         the matrix-core dec_mm on the fragment-ordered copy (3-8 pages) */
    int experts_touched;              /* routed experts active in the replayed step (per layer, summed / layers) */
    int tokens;                       /* pages in the batch */
    int kv_len;                       /* keys attended by page 0 */
    dsocr_kernel_profile qkv;         /* RMSNorm + fused q/k/v projection, one layer (dec_qkv_rope with RoPE in the
                                         epilogue at 1 page, dec_gemv at 2, dec_mm at 3-8) */
    dsocr_kernel_profile o_proj;      /* o_proj + residual, one layer (dec_gemv at 1-2 pages, dec_mm at 3-8) */
    dsocr_kernel_profile router;      /* MoE router: dec_gemv logits at 1-2 pages (the mix kernels rank-select),
                                         dec_route_grp (RMSNorm + logits + top-k + expert records) at 3-8 */
    dsocr_kernel_profile layers_step; /* every decoder layer of one decode step, replayed as one hipGraph */
    dsocr_kernel_profile lm_head_screened; /* int8 screened lm_head + exact rescoring selection (B <= 8, no penalty;
                                              3..8: one int8 stream on the int8 matrix cores) */
    const char* moe_gateup_kernel;    /* static strings: kernel names of the two MoE entries above */
    const char* moe_down_kernel;
} dsocr_decode_profile;
dsocr_status dsocr_profile_decode(dsocr_engine* e, int iters, dsocr_decode_profile* out);

/* In-context launch spans (diagnostics for the roofline line; no reference counterpart).  mode is a bit
 * mask, 0 = off: 1 = wave spans (every wave of the MoE gate/up (kind 0), MoE down (1) and attention (2)
 * launches writes its entry / exit s_memrealtime (100 MHz) to a slot, a one-block fold launch after each
 * keeps the first entry / last exit), 2 = HIP events recorded on the stream around those launches inside
 * the replayed step graph (the dispatch-level duration rocprofv3's kernel trace reports; read back after
 * every step; no extra kernel runs, so the step is the production chain plus the event markers), 4 (alone)
 * = chain spans: the gate/up, down, attention, o_proj (kind 3) and router (kind 4) launches of every layer
 * stamp their waves into their own slot regions and ONE fold launch runs at the end of each step (no fold
 * or event between launches), so exit(launch) - exit(previous launch) is the launch's dispatch-level
 * duration with its boundary, as rocprofv3 records a back-to-back dispatch; kinds = 5 then.  Mode 1
 * also records the distinct experts each MoE launch streamed (mode 2 alone leaves that field 0).  The decode steps
 * of every following generate are recorded; dsocr_engine_spans copies the last such generate's records,
 * [kinds][layers][steps][5] uint64 {entry, exit, distinct experts, waves, event duration ns}, into out
 * (cap = capacity in uint64; DSOCR_EINVAL if short; out NULL: only the dimensions are returned);
 * step s = tokens emitted before the step, decode steps are 1 .. steps - 1, unused entries are 0. */
dsocr_status dsocr_engine_set_spans(dsocr_engine* e, int mode);
dsocr_status dsocr_engine_spans(const dsocr_engine* e, uint64_t* out, size_t cap, size_t* kinds, size_t* layers,
                                size_t* steps);

/* ---- one-page persistent decode (decode_persist.hip; no reference counterpart: the reference's decode step is
 * Candle's per-op launches, model/mod.rs:1977-2034).  At B = 1 every decoder layer of a step runs as ONE
 * persistent launch when DSOCR_PERSIST=1 and the model's shape and dtypes fit it (opt-in: measured slower than
 * the per-layer launch chain).
 * dsocr_engine_set_persist_stamps(e, 1): the next generate times each persistent launch with HIP events and
 * records its phase clocks; dsocr_engine_persist_info then returns whether the last generate used the persistent
 * launch (*used), the launch durations in us (durations[cap_d], *n_launches) and the phase clocks
 * [steps][256 workgroups][layers][9] uint64 (s_memrealtime, 100 MHz) of its decode steps (stamps[cap_s],
 * *n_stamps; step i = position prompt_len + i).  NULL arrays: sizes only. */
dsocr_status dsocr_engine_set_persist_stamps(dsocr_engine* e, int mode);
dsocr_status dsocr_engine_persist_info(const dsocr_engine* e, int* used, double* durations, size_t cap_d,
                                       size_t* n_launches, uint64_t* stamps, size_t cap_s, size_t* n_stamps);

/* ---- device helpers for tests / tooling (plain pointers; no torch) */
dsocr_status dsocr_device_count(int* n);
dsocr_status dsocr_dev_alloc(size_t bytes, void** ptr);
dsocr_status dsocr_dev_free(void* ptr);
dsocr_status dsocr_memcpy_h2d(void* dst, const void* src, size_t bytes);
dsocr_status dsocr_memcpy_d2h(void* dst, const void* src, size_t bytes);
dsocr_status dsocr_dev_sync(void);
/* host: deterministic synthetic bf16 weights (same recipe as oracle/synth.c) */
dsocr_status dsocr_synth_bf16(const char* name, uint64_t seed, uint64_t n, uint16_t* out);
/* host: Pillow-exact bicubic resize (vision/resample.rs:101-160), RGB8 HWC */
dsocr_status dsocr_resize_bicubic(const uint8_t* src, uint32_t sw, uint32_t sh, uint8_t* dst, uint32_t dw,
                                  uint32_t dh);
/* fast_image_resize Convolution(CatmullRom) on RGB8 HWC (host; the dots.ocr and PaddleOCR-VL preprocessing resize,
 * crates/infer-paddleocr/src/vision/preprocess.rs:223-243, infer-dots vision/preprocess.rs) */
dsocr_status dsocr_resize_catmull_rom(const uint8_t* src, uint32_t sw, uint32_t sh, uint8_t* dst, uint32_t dw,
                                      uint32_t dh);

/* ---- kernel-level entry points (device pointers, default stream) for parity tests */
/* C[M][N] = act(A[M][K] . W[N][K]^T + bias) (+ C if accumulate); wdtype 0 = bf16, 1 = f16 */
dsocr_status dsocr_k_gemm(int M, int N, int K, const float* A, const void* W, int wdtype, const float* bias, float* C,
                          int act, int accumulate);
/* Vision / prefill linear (sam.rs:656-701, clip.rs:418-447; block.rs linears) on the fused split kernel:
 * f32 A [M][K], 16-bit W [N][K] (wdtype 0 bf16: 3 bf16 planes of A; 1 f16: W split into hi / lo bf16 too,
 * 5 products), C = act(A W^T + bias) (+ C), exact f32 products; splits <= 0 picks the engine's split-K. */
dsocr_status dsocr_k_gemm_f32a(int M, int N, int K, const float* A, const void* W, int wdtype, const float* bias,
                               float* C, int act, int accumulate, int splits);
/* Routed-expert linear of the prefill (block.rs:1215-1395 applies expert e to the rows that picked it):
 * group g owns gathered rows group_off[g] .. group_off[g+1] (device array), row r reads A row
 * a_rows ? a_rows[r] : r and writes C row c_rows ? c_rows[r] : r (-1 drops it), weights W + g * w_group_stride
 * ([N][K] 16-bit), bias + g * bias_group_stride.  kernel 0: the engine's dispatch (launch_gemm); 1 / 2: the
 * grouped kernel with 32- / 128-row tiles whatever the rows per group. */
dsocr_status dsocr_k_gemm_grouped(int M, int N, int K, const float* A, int lda, const int* a_rows, const void* W,
                                  int wdtype, long long w_group_stride, const float* bias, long long bias_group_stride,
                                  float* C, int ldc, const int* c_rows, int act, int accumulate, const int* group_off,
                                  int groups, int max_group_rows, int kernel);
/* Decode linear (transformer/block.rs attention / MLP projections at seq_len 1): y[M][N] =
 * act(xn . W^T + bias) (+ y), xn = rmsnorm(x; norm_w, eps) when norm_w != NULL (block.rs:24-29), else x. */
dsocr_status dsocr_k_gemv(int M, int N, int K, const float* x, const float* norm_w, float eps, const void* W,
                          int wdtype, const float* bias, float* y, int act, int accumulate);
/* dsocr_k_gemv with every stride and form the engine passes: x [M][ldx], W [N][ldw] (16-bit), y [M][ldy].
 * swizzle != 0: W (row-major, ldw == K) is first copied to dec_mm's fragment order and the launch reads the copy,
 * as the engine does at 3..8 pages; DSOCR_EINVAL where the dispatch would not run dec_mm on it.  *kind (optional)
 * receives the kernel the dispatch picked, as dsocr_k_gemv_kind names it.  dsocr_k_gemv is this with
 * (ldx = K, ldw = K, ldy = N, swizzle = 0). */
dsocr_status dsocr_k_gemv_ex(int M, int N, int K, const float* x, int ldx, const float* norm_w, float eps,
                             const void* W, int ldw, int wdtype, const float* bias, float* y, int ldy, int act,
                             int accumulate, int swizzle, const char** kind);
/* Which kernel the decode-linear dispatch picks (pure host decision, no device call; static string):
 * "dec_gemv_rb1" / "dec_gemv_rb2" / "dec_gemv_rb4" (dec_gemv_kernel, 1 / 2 / 4 weight rows per wave),
 * "dec_gemv_stream" (1..2 tokens, N > 16384, K <= 1536), "dec_gemv_lds_r1" / "dec_gemv_lds_r2" (3..8 tokens,
 * K <= 1536), "dec_mm_wk8" / "dec_mm_wr8" (3..8 tokens, K = 1280 on the matrix cores; wr8 from N = 16384) and
 * "dec_mm_wk8_swz" / "dec_mm_wr8_swz" (the same on a fragment-ordered copy), "none" for an empty call.  The kind
 * is that of the first launch; *rows_per_launch (optional) is how many token rows one launch takes (at most 16,
 * fewer when K is long: the call is split into ceil(M / rows) launches). */
dsocr_status dsocr_k_gemv_kind(int M, int N, int K, int ldw, int wdtype, int has_norm, int has_xn_out, int swizzle,
                               const char** kind, int* rows_per_launch);
/* W [N][K] row-major 16-bit -> dec_mm's fragment order [ceil(N/16) tiles][K/32 steps][64 lanes][8]: lane l of
 * step t of tile T holds W[min(16 T + (l & 15), N - 1)][32 t + 8 (l >> 4) .. + 7].  out: 16 ceil(N/16) K
 * elements.  K % 32 == 0.  Device pointers. */
dsocr_status dsocr_k_mm_swizzle(int N, int K, const void* w, void* out);
/* h[r][i] = silu(g[r][i]) * g[r][I + i] (candle silu: x / (1 + exp(-x))), g [rows][ldg] = gate | up, h [rows][ldh]:
 * the launch between the two matrix-core linears of the dense MLP at 3..8 pages. */
dsocr_status dsocr_k_silu_mul(int rows, int I, const float* g, int ldg, float* h, int ldh);
/* Long-K decode linear for 1..8 rows on the matrix cores (the dense layer-0 down projection of the
 * 3..8-page decode, K = 6848): y[M][N] (+)= x . W^T + bias, split-K with an in-launch ordered sum. */
dsocr_status dsocr_k_gemv_splitk(int M, int N, int K, const float* x, const void* W, int wdtype, const float* bias,
                                 float* y, int accumulate);
dsocr_status dsocr_k_layernorm(int rows, int cols, const float* x, const float* w, const float* b, float eps,
                               float* y);
/* DSQ record payload (device bytes, crates/dsq/src/lib.rs:60-110 dtype codes 0/1/8/12/14/16) ->
 * fp16 [out_dim][in_dim] on the device; replaces dsq-runtime's qtensor_from_ggml + QMatMul for the
 * dequant-on-load path (crates/dsq-runtime/src/lib.rs:336-366). */
dsocr_status dsocr_k_dsq_dequant(int qtype, const void* src, size_t src_bytes, size_t out_dim, size_t in_dim,
                                 void* out_f16);
dsocr_status dsocr_k_rmsnorm(int rows, int cols, const float* x, const float* w, float eps, float* y);
/* softmax(scale * q.k^T [+ SAM decomposed rel-pos] [causal]) . v over n_seq uniform sequences of L
 * rows; q,k,v,o are [n_seq*L][heads*hd]; relh/relw (optional) are the resized [2g-1][hd] tables of
 * a gh x gw grid (gh*gw == L). */
dsocr_status dsocr_k_attention(int n_seq, int L, int heads, int hd, float scale, int causal, const float* q,
                               const float* k, const float* v, float* o, const float* relh, const float* relw, int gh,
                               int gw);
/* Grouped-query attention under the DeepSeek-OCR-2 encoder's hybrid mask (vision/qwen2.rs:519-571): n_seq
 * sequences of L rows, the first `prefix` image tokens, the rest queries; row i sees key j iff j < prefix or
 * (i >= prefix and j <= i).  q, o are [n_seq*L][heads*hd]; k, v are [n_seq*L][kv_heads*hd]; f32 device pointers.
 * hd 32 or 64, heads % kv_heads == 0, 0 <= prefix <= L; anything else is DSOCR_EINVAL. */
dsocr_status dsocr_k_attention_prefix(int n_seq, int L, int prefix, int heads, int kv_heads, int hd, float scale,
                                      const float* q, const float* k, const float* v, float* o);
/* Bidirectional attention over bf16 values with f32 math on the bf16 matrix cores (the dots.ocr ViT,
 * dots_vit.rs:433-498): qkv bf16 [n_seq*L][ld] holding q | k | v (heads*hd each) per row; o [n_seq*L][o_ld]
 * f32 (o_bf16 = 0) or bf16 (o_bf16 = 1, RNE). */
dsocr_status dsocr_k_attention_bf16(int n_seq, int L, int heads, int hd, float scale, const void* qkv, long ld,
                                    void* o, long o_ld, int o_bf16);
/* The dots.ocr tower's linear (quant.rs:124-160 on bf16 tensors): A bf16 [M][lda], W bf16 [N][ldw], bias f32 [N]
 * or NULL, K % 64 == 0.  out_bf16 = 1: C bf16 [M][ldc] with every reference op rounded on its own,
 * v = rnd(A W^T); bias: v = rnd(v + b); accumulate: v = rnd(C + v); out_bf16 = 0: C f32.  variant 0: the engine's
 * dispatch; 2: the 128 x 128 kernel with two LDS stages; 3: the 256 x 256 ping-pong kernel (bf16 out, ldc % 8 == 0).
 * group_m: M bands per raster group (-1 the default).  swiglu != 0: W rows and bias interleaved per 32
 * (fc1 32b..32b+31, then fc3 32b..32b+31), N = 2 I, C = h [M][ldc] of I columns.  rope_cos / rope_sin (f32
 * [M][128], or NULL): columns below rope_cols (a multiple of 256) are heads of 128 dims, rotated in the epilogue. */
dsocr_status dsocr_k_gemm_bf16(int M, int N, int K, const void* A, long lda, const void* W, long ldw, const float* bias,
                               void* C, long ldc, int out_bf16, int accumulate, int variant, int group_m, int swiglu,
                               const float* rope_cos, const float* rope_sin, int rope_cols);
/* One row op of the dots.ocr tower (dots_vit.rs) on bf16 tensors, f32 math, bf16 (RNE) out:
 *  RMSNORM     x [rows][cols] bf16 (aux = 0) or f32 (aux = 1), p0 = w, eps; y bf16 (may alias a bf16 x)
 *  LAYERNORM   x bf16 [rows][cols], p0 = w, p1 = b, eps
 *  SWIGLU      x = [fc1 | fc3] bf16 [rows][2 cols]; y = rnd(silu(g) * u) [rows][cols]
 *  GELU        y bf16 [rows][cols] in place (x unused)
 *  ROPE_QK     x = q|k|v bf16 [rows][3 aux cols] (aux heads of cols dims), p0 = cos, p1 = sin f32 [rows][cols];
 *              y gets the rotated q | k columns (its v columns are not written)
 *  TO_BF16     x f32 [rows][ld] (first cols columns) -> y bf16 [rows][aux], zeros from column cols on
 *  BF16_TO_F32 x bf16 -> y f32, rows * cols values */
enum {
    DSOCR_DOTS_RMSNORM = 0, DSOCR_DOTS_LAYERNORM = 1, DSOCR_DOTS_SWIGLU = 2, DSOCR_DOTS_GELU = 3,
    DSOCR_DOTS_ROPE_QK = 4, DSOCR_DOTS_TO_BF16 = 5, DSOCR_DOTS_BF16_TO_F32 = 6
};
dsocr_status dsocr_k_dots_op(int op, long rows, int cols, int aux, long ld, const void* x, const float* p0,
                             const float* p1, float eps, void* y);
/* ---- the vision tower's kernels (SAM / CLIP / projector, the OCR-2 encoder's row ops) in the forms the engine
 * launches them.  Every call forwards to the launch the engine makes. */
/* dsocr_k_gemm_f32a with everything the engine's linear passes: A [M][lda], C [.][ldc], c_rows (device, M ints or
 * NULL): row r of the product goes to C row c_rows[r], -1 drops it (the window un-partition); c_cap: rows C holds
 * (every c_rows entry is checked against it).  variant 0: the default kernel; 2: two LDS stages (bf16 weights).
 * splits 0: the engine's split-K count for (M, N, K); > 0: that many K slices (<= K / 32).  With more than one slice
 * the bias, activation, accumulate and row scatter run in the split-K reduce over a [splits][M][N] workspace.
 * *splits_used (optional) receives the count launched. */
dsocr_status dsocr_k_gemm_f32a_ex(int M, int N, int K, const float* A, long lda, const void* W, int wdtype,
                                  const float* bias, float* C, long ldc, const int* c_rows, int c_cap, int act,
                                  int accumulate, int variant, int splits, int* splits_used);
/* Row norms with row strides (floats, multiples of 4, >= cols; cols % 4 == 0); y may be x.  out_rows (device, rows
 * ints or NULL): row r is written to y row out_rows[r], -1 drops it (the window partition); y_rows: rows y holds. */
dsocr_status dsocr_k_layernorm_ex(int rows, int cols, const float* x, int ldx, const float* w, const float* b, float eps,
                                  float* y, int ldy, const int* out_rows, int y_rows);
dsocr_status dsocr_k_rmsnorm_ex(int rows, int cols, const float* x, int ldx, const float* w, float eps, float* y,
                                int ldy);
/* SAM's decomposed rel-pos terms (sam.rs:1124-1192): q [n_seq * gh * gw][q_ld] with head h at columns h * hd,
 * relh [2 gh - 1][hd], relw [2 gw - 1][hd]; out [n_seq][heads][gh * gw][gh + gw]: entry kh < gh is
 * q . relh[qh - kh + gh - 1], entry gh + kw is q . relw[qw - kw + gw - 1]. */
dsocr_status dsocr_k_sam_relbias(int n_seq, int gh, int gw, int heads, int hd, const float* q, long q_ld,
                                 const float* relh, const float* relw, float* out);
/* Bidirectional attention over n_seq uniform sequences of L rows of one fused buffer qkv [n_seq * L][ld] holding
 * q | k | v (heads * hd floats each; ld >= 3 heads hd, ld % 4 == 0); o [n_seq * L][o_ld], o_ld >= heads * hd; columns
 * past heads * hd of an o row are not written.  relh / relw (both or neither): SAM's rel-pos tables of a gh x gw
 * grid (gh * gw == L), the bias table built from the buffer's q columns as the engine does.  hd 32, 64 or 128. */
dsocr_status dsocr_k_attention_fused(int n_seq, int L, int heads, int hd, float scale, const float* qkv, long ld,
                                     float* o, long o_ld, const float* relh, const float* relw, int gh, int gw);
/* One data-movement kernel of the page path: op, its nd dims d[] and np device pointers p[] (the last one is the
 * destination), all f32 unless noted:
 *  PATCH_IM2COL      d: n, H, W, ps              p: img [n][3][H][W], cols [n (H/ps) (W/ps)][3 ps ps] (K order c, ky, kx)
 *  CONV_IM2COL_NHWC  d: n, H, W, C, kh, kw, stride, pad   p: x [n][H][W][C], cols [n oh ow][kh kw C] (K order ky, kx, c)
 *  ADD_BROADCAST     d: rows_per_rep, cols, reps p: t [rows_per_rep][cols], x [reps][rows_per_rep][cols] (x += t)
 *  CLIP_EMBED        d: n, S, C                  p: sam [n][S][C], cls [C], pos [S + 1][C], out [n][S + 1][C]
 *  CONCAT_CLIP_SAM   d: n, S, C1, C2             p: clip [n][S + 1][C1], sam [n][S][C2], out [n][S][C1 + C2]
 *  ASSEMBLE_ROWS     d: rows, H, table_dt, ld_dst   p: kind [rows] int, index [rows] int, table [.][H] 16-bit,
 *                    srcA [.][H], srcB [.][H], vecA [H], vecB [H], dst [rows][ld_dst]; kind 0: table row index
 *                    (widened), 1: srcA row, 2: srcB row, 3: vecA, 4: vecB
 *  EMBED_TOKENS      d: n, H, table_dt, ld       p: table [.][H] 16-bit, ids [n] int, out [n][ld]
 *  TRACE_LOGITS      d: B, V, ld, steps          p: logits [B][ld], out_len [B] int, done [B] int, trace [B][steps][V]:
 *                    page b's row goes to trace[b][out_len[b]] unless done[b] or out_len[b] >= steps
 *  OCR2_BUILD_SEQ    d: n, P, D                  p: feat [n][P][D], query [P][D], out [n][2 P][D]
 *  OCR2_ROPE         d: rows, L, n_heads, hd, ld p: cos [L][hd], sin [L][hd], x [rows][ld] (in place: the first
 *                    n_heads heads of every row, position = row % L)
 *  OCR2_TAKE_QUERIES d: n, P, D                  p: src [n][2 P][D], dst [n][P][D]
 * table_dt 0 = bf16, 1 = f16.  The row indices in kind / index / ids / out_len are the caller's to keep in range. */
enum {
    DSOCR_VIS_PATCH_IM2COL = 0, DSOCR_VIS_CONV_IM2COL_NHWC = 1, DSOCR_VIS_ADD_BROADCAST = 2, DSOCR_VIS_CLIP_EMBED = 3,
    DSOCR_VIS_CONCAT_CLIP_SAM = 4, DSOCR_VIS_ASSEMBLE_ROWS = 5, DSOCR_VIS_EMBED_TOKENS = 6, DSOCR_VIS_TRACE_LOGITS = 7,
    DSOCR_VIS_OCR2_BUILD_SEQ = 8, DSOCR_VIS_OCR2_ROPE = 9, DSOCR_VIS_OCR2_TAKE_QUERIES = 10
};
dsocr_status dsocr_k_vision_op(int op, const long long* d, int nd, const void* const* p, int np);
/* host: SAM's window partition as row maps (sam.rs:926-980) for n images of a g x g token grid and windows of
 * W x W, the grid padded to nw = ceil(g / W) windows a side: tok2win [n g g] is each token's window row,
 * win2tok [n nw nw W W] the inverse, -1 on the padding rows. */
dsocr_status dsocr_window_maps(int n, int g, int W, int* tok2win, int* win2tok);
/* Decode attention step (block.rs:608-789 at seq_len 1, rope block.rs:1403-1471): for page b the
 * token at position pos = kv_pos[b] has its q / k rotated (cos/sin tables [max_len][rope_dim]; prerot != 0:
 * the q / k rows of qkv are already rotated), k and v appended to the f32 cache [B][kv_heads][max_len][hd]
 * at pos, then o[b] = softmax(scale * q.K[:pos+1]^T) . V[:pos+1].  qkv: [B][(heads + 2 kv_heads) * hd];
 * o: [B][heads*hd]. */
dsocr_status dsocr_k_decode_attention(int B, int heads, int kv_heads, int hd, int rope_dim, int max_len, float scale,
                                      const float* qkv, const float* cos, const float* sin, float* kc, float* vc,
                                      const int* kv_pos, float* o, int prerot);
/* The decoder prefill between the q|k|v linear and the o linear, as the engine launches it on a ragged batch
 * (block.rs:608-789, rope block.rs:1403-1471): B sequences of lens[b] rows (host array) packed one after another,
 * T = sum lens rows in all.  qkv [T][(heads + 2 kv_heads) * hd]: the q columns are rotated in place at the row's
 * position in its sequence (cos / sin tables [>= max lens][rope_dim]; use_mla: the even/odd regroup first), the
 * rotated k and the v columns appended to the f32 caches kc / vc [B][kv_heads][cap][hd] at (b, head, position);
 * then o [T][heads * hd] = causal softmax(scale * q.K^T) . V per sequence, k / v read from the cache.
 * use_part != 0: the key-piece form (one block per 128-query block and 128-key piece, then the piece combine; the
 * workspace enters filled with NaN); 0: one block per query block.  hd 32 runs one kernel either way.
 * DSOCR_EINVAL: hd not 32 / 64 / 128, heads % kv_heads != 0, rope_dim odd or > hd, cap < max lens, a sequence
 * without rows, or (heads + kv_heads) * hd > 8192.  lens is a host pointer; the rest are device pointers. */
dsocr_status dsocr_k_prefill_attention(int B, int heads, int kv_heads, int hd, int rope_dim, int use_mla, int cap,
                                       float scale, const int* lens, float* qkv, const float* cos, const float* sin,
                                       float* kc, float* vc, float* o, int use_part);
/* The same stage for a prefill behind a cached past (a prompt suffix admitted through a page prefix entry): sequence
 * b brings lens[b] >= 1 new rows at positions past[b] .. past[b] + lens[b] - 1 (past[b] >= 0, past[b] + lens[b] <=
 * cap; host arrays).  The caches arrive holding rows [0, past[b]) of every sequence; the new rows are rotated at
 * their shifted positions and appended, then o [T][heads * hd] = softmax(scale * q.K^T) . V of every new row over
 * keys [0, its own position] (launch_attention_past: key pieces + a combine launch; its workspace enters filled
 * with NaN).  cos / sin [>= cap][rope_dim].  DSOCR_EINVAL as dsocr_k_prefill_attention, before any launch. */
dsocr_status dsocr_k_prefill_attention_past(int B, int heads, int kv_heads, int hd, int rope_dim, int use_mla, int cap,
                                            float scale, const int* past, const int* lens, float* qkv, const float* cos,
                                            const float* sin, float* kc, float* vc, float* o);
/* The same stage as a chunk of a sliced admission runs it (launch_attention_chunk: one workgroup per 32-query tile,
 * head and sequence, the keys streamed in tiles with an online softmax; one launch, no workspace).  The arguments of
 * dsocr_k_prefill_attention_past, plus the session cache's shape: kc / vc hold `pages` pages of [kv_heads][cap][hd]
 * and sequence b lives in page page0 + b (0 <= page0, page0 + B <= pages).  Rows past past[b] + lens[b] are never
 * read.  DSOCR_EINVAL, before any launch, for hd outside {32, 64, 128}, heads % kv_heads != 0, lens[b] < 1,
 * past[b] < 0 or past[b] + lens[b] > cap. */
dsocr_status dsocr_k_attention_chunk(int B, int heads, int kv_heads, int hd, int rope_dim, int use_mla, int cap,
                                     float scale, const int* past, const int* lens, float* qkv, const float* cos,
                                     const float* sin, float* kc, float* vc, float* o, int page0, int pages);
/* One page's decode attention sub-layer as the engine runs it (block.rs:446-804 at seq_len 1): RMSNorm +
 * q/k/v projection (Wqkv [3H][H], 16-bit) with RoPE in the epilogue, K/V append at kv_pos[s], softmax
 * attention over positions 0..kv_pos[s], for `steps` launches back to back (x [steps][H], kv_pos [steps],
 * o [steps][H]).  fused != 0: the one-launch form (dec_qkv_attn: attention blocks poll the q/k/v row, which
 * must enter the first launch filled with DSOCR_HANDOFF_SENTINEL words and is left so by every launch);
 * fused == 0 or the residency rule refusing it: projection and attention as two launches.  *used_fused
 * reports which ran.  128-dim MHA heads only.  Device pointers. */
#define DSOCR_HANDOFF_SENTINEL 0x7FBADBADu
dsocr_status dsocr_k_qkv_attention(int fused, int steps, int H, int heads, int hd, int max_len, float scale,
                                   float eps, const float* x, const float* norm_w, const void* Wqkv, int wdtype,
                                   const float* cos, const float* sin, float* kc, float* vc, const int* kv_pos,
                                   float* qkv_row, float* o, int* used_fused);
/* `layers` consecutive fused launches (dec_qkv_attn) as the layer sequence of one decode step, on two hand-off
 * copies the call allocates and fills with DSOCR_HANDOFF_SENTINEL.  defer != 0: the engine's deferred refill
 * (launch l on copy l & 1; every launch but the last leaves the words it read to the next launch, which cleans
 * that copy from its projection blocks; the last refills its own); defer == 0: every launch on copy 0, refilled
 * in-launch.  Per launch l: x [layers][H], Wqkv [layers][3H][H] (16-bit), kc / vc [layers][heads][max_len][hd],
 * kv_pos [layers], o [layers][H] (device pointers).  Returned to host memory: qkv_copies [2][3H] and
 * part_copies [2][heads * ceil(max_len / 64) * (hd + 4)], the final words of both copies, and *err_word, the
 * kernels' give-up flag.  128-dim MHA heads only; DSOCR_EINVAL when the fused launch is refused. */
dsocr_status dsocr_k_qkv_attention_layers(int defer, int layers, int H, int heads, int hd, int max_len, float scale,
                                          float eps, const float* x, const float* norm_w, const void* Wqkv, int wdtype,
                                          const float* cos, const float* sin, float* kc, float* vc, const int* kv_pos,
                                          float* o, uint32_t* qkv_copies, uint32_t* part_copies, int* err_word);
/* Residency rule of the polled in-launch hand-offs (pure host decision, no device call): 1 when
 * waiting_blocks (blocks that may spin on blocks of the same grid) < usable slots = (min(api, 8), one fewer
 * where the occupancy API may over-admit) x cus; else 0 (the engine then launches the non-polling form). */
int dsocr_k_poll_wait_fits(long waiting_blocks, int api_blocks_per_cu, int cus);
/* Decode MoE layer (the north-star kernel chain, block.rs:1215-1395): [RMSNorm] + router GEMV +
 * softmax top-k + grouping + grouped SwiGLU experts + shared experts + weighted combine,
 * out[T][H] += moe(xn), xn = rmsnorm(x; norm_w, eps) if norm_w != NULL else x.  Runs exactly the
 * engine's decode dispatch for T tokens (the same launches Engine::decode_step issues).
 * Wgu: [E][2I][H] (gate rows then up rows), Wd: [E][H][I], router [E][H], shared Wgu [2Is][H],
 * shared Wd [H][Is] (shared may be NULL), all 16-bit (wdtype). */
dsocr_status dsocr_k_moe(int T, int H, int E, int topk, int I, int Is, const float* x, const float* norm_w,
                         float eps, const void* router,
                         const void* Wgu, const void* Wd, const void* sWgu, const void* sWd, int wdtype,
                         int norm_topk, float scaling, float* out, int* topk_ids_out, float* topk_w_out);
/* dsocr_k_moe with the router's other options: softmax_scoring 0 = sigmoid scores, router_bias = the
 * e_score_correction_bias added to the logits (device [E], or NULL), logits_out = the router logits the
 * launches left in their workspace (host [T][E], or NULL).  dsocr_k_moe is this with (1, NULL, NULL).
 * DSOCR_EINVAL for E > 256, top_k > 8, top_k > E or a NULL x / router / Wgu / Wd / out. */
dsocr_status dsocr_k_moe_ex(int T, int H, int E, int topk, int I, int Is, const float* x, const float* norm_w,
                            float eps, const void* router,
                            const void* Wgu, const void* Wd, const void* sWgu, const void* sWd, int wdtype,
                            int norm_topk, float scaling, float* out, int* topk_ids_out, float* topk_w_out,
                            int softmax_scoring, const float* router_bias, float* logits_out);
/* Which routing implementation the decode dispatch picks for dsocr_k_moe_ex at this shape with f16 weights
 * (static string): "moe_gateup_mix" (one token, E <= 64), "moe_gateup_slot" (every gate/up block routes itself),
 * "dec_route_grp" (3..8 tokens, E <= 64: norm + router + top-k + records in one launch), "moe_gateup_mm" (the same
 * routing inside the matrix-core gate/up launch; DSOCR_ROUTE_FUSED=0 turns it off), "dec_router" (3..8 tokens,
 * E > 64: the router GEMV's last block routes), "moe_route" (more than 8 tokens). */
dsocr_status dsocr_k_moe_route_kind(int T, int H, int E, int topk, int I, int Is, int has_norm, const char** kind);
/* The prefill's routing (block.rs:1243-1324) from given logits [T][E]: scores, greedy top-k -> ids / w [T][topk],
 * then the grouping by expert: eoff [E + 1], arow [T topk] (sorted position -> token), apos [T topk]
 * (assignment t topk + k -> sorted position).  Device pointers.  E <= 256, top_k <= min(8, E). */
dsocr_status dsocr_k_moe_prefill_route(int T, int E, int topk, const float* logits, int softmax_scoring, int norm_topk,
                                       float scaling, int* ids, float* w, int* eoff, int* arow, int* apos);
/* The prefill's combine: out[t] (+)= sum_k w[t][k] * y[apos[t topk + k]] (+ shared[t]); y [T topk][H], shared
 * [T][H] or NULL, accumulate != 0 adds to out.  Device pointers. */
dsocr_status dsocr_k_moe_combine(int T, int topk, int H, const float* y, const int* apos, const float* w,
                                 const float* shared, float* out, int accumulate);
/* The same layer from packed DSQ blocks (T <= 8): payloads are raw record bytes in record layout on the
 * device, experts concatenated — Wgu_payload rows [E][2I] of in_dim H (per expert the gate record then the up
 * record), Wd_payload [E][H] of in_dim I, shared [2Is] of H and [H] of Is (NULL / Is = 0: no shared expert);
 * qtypes 8 (Q8_0) or 12 (Q4_K).  The call repacks them as the engine does at load and runs the engine's packed
 * dispatch (router f16 [E][H]).  DSOCR_EINVAL for another qtype or an in_dim that is not whole blocks. */
dsocr_status dsocr_k_moe_packed(int T, int H, int E, int topk, int I, int Is, const float* x, const float* norm_w,
                                float eps, const void* router_f16, int gu_qtype, const void* Wgu_payload, int d_qtype,
                                const void* Wd_payload, int sgu_qtype, const void* sWgu_payload, int sd_qtype,
                                const void* sWd_payload, int norm_topk, float scaling, float* out, int* topk_ids_out,
                                float* topk_w_out);
/* y[T][rows] = x[T][in_dim] . W^T (T <= 8, device pointers) with W a record-layout payload of qtype 8 / 12,
 * through the engine's repack and the unpack function the packed MoE kernels call.  Terms with x == 0 are
 * skipped and the sums start from -0, so a one-hot x row returns the decoded weights bit for bit. */
dsocr_status dsocr_k_dsq_rows_dot(int qtype, size_t rows, size_t in_dim, const void* payload, int T, const float* x,
                                  float* y);
/* Kernel names launch_moe_decode picks for a decode MoE of T tokens (static strings), e.g. the bench's
 * roofline label: "moe_gateup_mix_kernel" at T = 1, "moe_gateup_grp_kernel" at T = 3..8. */
dsocr_status dsocr_k_moe_kernels(int T, int H, int E, int topk, int I, int Is, int has_norm, const char** gateup,
                                 const char** down);
/* Screened greedy selection (the engine's decode head at B <= 2 without repetition penalty): the
 * int8 copy of W (bf16 [V][K], quantised as at engine load) gives every row an interval that holds
 * the exact logit, the surviving rows are rescored with the exact kernel's arithmetic; out_tok[b] =
 * the first-index argmax of rmsnorm(x_b; norm_w, eps) . W^T over the rows not in page b's ban list
 * (ban [B][ban_ld]: count then tokens, or NULL), as argmax_index (sampling.rs:104-118). */
dsocr_status dsocr_k_lmhead_screened(int B, int V, int K, const float* x, const float* norm_w, float eps,
                                     const void* W, const int* ban, int ban_ld, int* out_tok);
/* Greedy selection with repetition penalty + n-gram ban (sampling.rs:34-158) over B rows of V
 * logits; ctx [B][ctx_cap] int32 with ctx_len[B]. */
dsocr_status dsocr_k_sample_greedy(int B, int V, float* logits, const int* ctx, int ctx_cap, const int* ctx_len,
                                   int ngram, float rep_penalty, int* out_tok);
/* Stochastic selection (select_token_id's do_sample branch: top-k, top-p, WeightedIndex over rand's
 * StdRng seeded by seed_from_u64(seed)) on device logits [B][V] after the repetition penalty and the
 * n-gram ban; `draws` successive selections on the same logits with the RNG state carried over
 * (out_tok [draws][B]).  Device pointers, like dsocr_k_sample_greedy. */
dsocr_status dsocr_k_sample_stoch(int B, int V, float* logits, const int* ctx, int ctx_cap, const int* ctx_len,
                                  int ngram, float rep_penalty, double temperature, size_t top_k, double top_p,
                                  uint64_t seed, int draws, int* out_tok);
/* Selection with per-row parameters, as the exact head of a DSOCR_SESSION_PER_REQUEST session launches it: the
 * repetition penalty (once, each row its own), then `draws` times the greedy selector, the sampling selector and
 * the final kernel on the same logits, each row taking the selector its record names, sampled rows' RNG state
 * (seed_from_u64(seeds[b])) carried over (out_tok [draws][B]).  Row b equals dsocr_k_sample_greedy /
 * dsocr_k_sample_stoch of that row alone.  rows / seeds: host arrays [B]; the rest device pointers. */
typedef struct {
    int do_sample;               /* sampling iff do_sample && temperature > 0 */
    double temperature;
    double top_p;
    size_t top_k;
    float repetition_penalty;
    size_t no_repeat_ngram_size;
    int64_t eos_token_id;        /* < 0: none */
} dsocr_row_params;
dsocr_status dsocr_k_select_rows(int B, int V, float* logits, const int* ctx, int ctx_cap, const int* ctx_len,
                                 const dsocr_row_params* rows, const uint64_t* seeds, int draws, int* out_tok);
/* The screened head with its parts shown: the launches of Engine::decode_head's screened branch (the load-time
 * quantisation once, then per step the int8 lm_head and the screened final kernel) for `steps` consecutive steps
 * on one set of state rows, every intermediate copied back.  Step t reads x [t][B][ldx] and the ban list step
 * t - 1 left (step 0: `ban`, or empty lists); B <= 2 runs the single-token kernel, 3..8 the matrix-core form.
 * rows == NULL: ngram / eos apply to every row; else row b takes rows[b] (greedy records only) and the kernels'
 * per-row instantiations run.  table (optional): the embedding rows [V][H], table_dt 0 bf16 / 1 f16.  The state
 * starts at out_len = done = 0, kv_pos = kv_len = ctx_len.  Every pointer is a HOST pointer; every output may be
 * NULL.  Per step (leading dimension [steps]): out_tok [B], ban_out [B][ban_ld], ctx_out [B][ctx_cap],
 * ctx_len_out [B], out_ids [B][out_cap], out_len / done / kv_pos / kv_len [B], x_next [B][H].  Of step `probe`,
 * in the device layout (nblk, slot: dsocr_k_lmhead_screen_grid): blk_cnt / blk_t [B][nblk], cand / cand_hi
 * [B][slot][nblk], xn_out [B][K], and xn_gemv [B][K], the rows the exact kernel (dec_gemv) stages from the same
 * input.  Of the quantisation: q [V][K], scale / bound [V], and (K % 64 == 0) qnorm [V],
 * qfrag [ceil(V / 16)][K / 64][64][16].  steps == 0 quantises only.
 * DSOCR_EINVAL outside the kernels' contract: K % 16 != 0, K outside 16..1536, B outside 1..8, 3..8 rows at a K
 * the matrix-core form does not take (768, 1024, 1280, 1536; V >= 16), ban_ld < ctx_cap + 1, a sampling record. */
typedef struct {
    int B, V, K, wdtype, steps, probe;
    const void* W;               /* [V][K] 16-bit rows (wdtype 0 bf16, 1 f16) */
    const float* x;              /* [steps][B][ldx] */
    long long ldx;
    const float* norm_w;         /* [K] */
    float eps;
    const int* ctx;              /* [B][ctx_cap] */
    int ctx_cap;
    const int* ctx_len;          /* [B] */
    int ngram, eos;              /* rows == NULL; eos < 0: none */
    const dsocr_row_params* rows;
    const int* ban;              /* [B][ban_ld]: count, then tokens (NULL: empty) */
    int ban_ld, out_cap;
    const void* table;           /* [V][H] or NULL */
    int table_dt, H;
    int* out_tok; int* ban_out; int* ctx_out; int* ctx_len_out; int* out_ids; int* out_len; int* done;
    int* kv_pos; int* kv_len; float* x_next;
    int* blk_cnt; float* blk_t; int* cand; float* cand_hi; float* xn_out; float* xn_gemv;
    int8_t* q; float* scale; float* bound; float* qnorm; int8_t* qfrag;
} dsocr_screen_steps;
dsocr_status dsocr_k_lmhead_screen_steps(const dsocr_screen_steps* s);
/* The screened lm_head's grid for (B, V, K): blocks per row, entries per block slot, and whether the matrix-core
 * form runs (B >= 3).  DSOCR_EINVAL as above. */
dsocr_status dsocr_k_lmhead_screen_grid(int B, int V, int K, int* nblk, long long* slot, int* matrix_core);

/* One page's decode state from slot src to slot dst of a session (src != dst), one launch: K / V rows
 * [0, kv_len[src]) of every layer and kv head of the f32 caches kc / vc [layers][slots][kv_heads][cap][hd]
 * (16-byte vector copies, hd % 4 == 0), the rows ctx [slots][ctx_cap], out [slots][out_cap], ban [slots][ban_ld],
 * rng [slots][rng_words], x [slots][H] and the per-slot scalars kv_len, kv_pos, ctx_len, out_len, done, tok.
 * Rows from kv_len on, the source and every other slot are not written.  Any array but kc, vc, kv_len may be
 * NULL.  Device pointers. */
/* The two log-probability launches (dec_lp_partial, dec_lp_final) once on host rows: logits [B][ld], tok [B];
 * emit[b] = 0 leaves lp[b], top_id[b][0..K), top_lp[b][0..K) untouched.  _penalty: with a context row per page
 * ([B][ctx_cap], ctx_len [B]) and the repetition-penalty launch between the two, as the engine's step runs them:
 * the result equals the call without it on the same raw logits. */
dsocr_status dsocr_k_logprobs(int B, int V, int K, const float* logits, int ld, const int* tok, const uint8_t* emit,
                              float* lp, int64_t* top_id, float* top_lp);
/* The logit bias launches once on host rows: launch_logit_bias_build for every row with flags[b] != 0 (its list:
 * pairs [first[b], first[b] + count[b]) of ids / values, and allow_only[b]), then launch_dec_logit_bias on logits
 * [B][ld] (in / out), which sit `offset` floats behind a 16-byte aligned device address (an odd offset: the scalar
 * path).  dense [B][dense_ld] receives the dense rows (dense_ld = (V + 3) / 4 * 4; zeros for a row without flag).
 * Lists are not validated here (an id outside [0, V) is skipped). */
dsocr_status dsocr_k_logit_bias(int B, int V, int ld, int offset, float* logits, const int64_t* ids, const float* values,
                                const int* first, const int* count, const int* flags, const int* allow_only,
                                float* dense, int dense_ld);
/* The stop launches on host rows: launch_stop_table_build for every row with n_seq[b] != 0 (lens [B][16], ids [B][512]:
 * the row's sequences back to back), then `steps` rounds.  Round t does per row what a final selection kernel does
 * with tokens[t][b]: a done row keeps everything, emit[t][b] == 0 (EOS selected) sets done alone, else the token is
 * appended to out [B][out_cap] / out_len (done when out_cap is reached); then one launch_dec_stop_match over the B
 * rows.  out, out_len, done, seen and hit [B][2] are in / out (the cells of a row with n_seq == 0 reach the device as
 * given and come back as the device left them); *_steps, each optional, receive every round's values ([steps][B],
 * hit [steps][B][2]). */
dsocr_status dsocr_k_stop_match(int B, int steps, int out_cap, const int* n_seq, const int* lens, const int64_t* ids,
                                const int* tokens, const uint8_t* emit, int* out, int* out_len, int* done, int* seen,
                                int* hit, int* done_steps, int* seen_steps, int* hit_steps, int* out_len_steps);
/* launch_dec_out_penalty once on host rows: logits [B][ld] (in / out), out_ids [B][out_cap], out_len [B] and one
 * record per row (never NULL; min_p is not read by this kernel). */
dsocr_status dsocr_k_out_penalty(int B, int V, int ld, float* logits, const int* out_ids, int out_cap,
                                 const int* out_len, const dsocr_penalties* pen);
/* launch_guided_build + launch_dec_guided_mask once on host rows.  Every row with on[b] != 0 is built from the one
 * automaton `g` (checked like dsocr_guided_check) with the EOS id `eos`; then its state is set to state[b] and the
 * mask runs over logits (in / out): B rows of ld floats that start row_off floats behind a 16-byte aligned address.
 * mask_out [n_states][mask_ld] (mask_ld = ceil(V / 32) rounded up to a multiple of 4) receives the bitmask of the
 * first row that is on. */
dsocr_status dsocr_k_guided_mask(int B, int V, int ld, int row_off, float* logits, const dsocr_guided* g, long long eos,
                                 const int* on, const int* state, const int* done, uint32_t* mask_out);
/* launch_dec_guided_advance over a scripted run: rows with on[b] != 0 are built from `g`; in step i a row that is not
 * done and has emit[i][b] != 0 appends tokens[i][b] to its output, then the advance runs; steps_out [steps][B][4]
 * receives {state, seen, status, done} of every row after every step. */
dsocr_status dsocr_k_guided_advance(int B, int steps, const dsocr_guided* g, const int* on, const int* tokens,
                                    const uint8_t* emit, int* steps_out);
/* launch_dec_ngram_window once on host rows: logits [B][ld] (in / out), ctx [B][ctx_cap], ctx_len [B] and one record
 * pointer per row (an entry may be NULL: off).  plain >= 2: a row whose record is off is banned as {plain, unbounded
 * window, no whitelist}; else it is left alone. */
dsocr_status dsocr_k_ngram_window(int B, int V, int ld, float* logits, const int* ctx, int ctx_cap, const int* ctx_len,
                                  const dsocr_ngram_window* const* recs, int plain);
/* dsocr_k_sample_stoch with a per-row ln_min_p (host array [B]; -inf: no filter): the sampling selector and the
 * final kernel `draws` times on the same logits, the RNG state carried over (out_tok [draws][B]).  The other
 * pointers are device pointers, as there. */
dsocr_status dsocr_k_sample_stoch_min_p(int B, int V, float* logits, const int* ctx, int ctx_cap, const int* ctx_len,
                                        int ngram, float rep_penalty, double temperature, size_t top_k, double top_p,
                                        const double* ln_min_p, uint64_t seed, int draws, int* out_tok);
dsocr_status dsocr_k_logprobs_penalty(int B, int V, int K, const float* logits, int ld, const int* tok, const uint8_t* emit,
                                      const int* ctx, int ctx_cap, const int* ctx_len, float penalty, float* lp,
                                      int64_t* top_id, float* top_lp);
dsocr_status dsocr_k_session_slot_move(int layers, int slots, int kv_heads, int cap, int hd, float* kc, float* vc,
                                       int* kv_len, int* kv_pos, int* ctx, long long ctx_cap, int* ctx_len, int* out,
                                       long long out_cap, int* out_len, int* done, int* tok, uint32_t* rng,
                                       int rng_words, int* ban, long long ban_ld, float* x, int H, int src, int dst);
/* launch_session_prefix_copy once: K / V rows [0, rows) of every layer and kv head between slot `slot` of the f32
 * caches kc / vc [layers][slots][kv_heads][cap][hd] and a dense entry of 2 * layers * kv_heads * rows * hd floats
 * ([layers][kv_heads][rows][hd] of K, then of V); to_slot 0: slot -> entry, 1: entry -> slot.  Nothing else is
 * written.  DSOCR_EINVAL: rows outside 1..cap, slot outside the caches, hd % 4 != 0.  Device pointers. */
dsocr_status dsocr_k_session_prefix_copy(int layers, int slots, int kv_heads, int cap, int hd, float* kc, float* vc,
                                         int slot, int rows, float* entry, int to_slot);

/* ---- dots.ocr vision tower (BASELINE configs[3]; crates/infer-dots/src/vision/dots_vit.rs
 *      DotsVisionModel::load / forward, vision/preprocess.rs preprocess_image).  The tower runs in the
 *      reference's bf16 semantics (every op's output rounded to bf16; attention scores / softmax /
 *      probs.V in f32).  config_path: the dots config.json (its `vision_config`, plus an optional
 *      `preprocessor_config` object with the preprocessor_config.json fields); weights_path NULL
 *      selects the seeded synthetic checkpoint (tensor names `vision_tower.*`). */
typedef struct dsocr_dots dsocr_dots;
dsocr_status dsocr_dots_load(const char* config_path, const char* weights_path, uint64_t synthetic_seed, int device,
                             dsocr_dots** out);
void dsocr_dots_free(dsocr_dots* d);
dsocr_status dsocr_dots_info(const dsocr_dots* d, size_t* hidden, size_t* embed_dim, size_t* layers, size_t* patch_dim);
/* preprocess_image (host): RGB8 HWC -> patches [N][3*p*p] in merge-group order; grid_thw = (t, h, w) */
dsocr_status dsocr_dots_preprocess(const char* config_path, const uint8_t* rgb, uint32_t width, uint32_t height,
                                   float* patches, size_t cap_patches, size_t* n_patches, uint32_t* grid_thw);
/* preprocess + tower for one page: out [groups][hidden] f32 (bf16 values), groups = N / merge^2 */
dsocr_status dsocr_dots_embed(dsocr_dots* d, const uint8_t* rgb, uint32_t width, uint32_t height, float* out,
                              size_t cap_rows, size_t* n_rows, uint32_t* grid_thw);
/* tower on device-resident patches (device pointers; the bench's inputs-in-HBM form); the first
 * time_attention_layers layers' attention launches are timed alone (0: no per-layer sync) */
dsocr_status dsocr_dots_embed_device(dsocr_dots* d, const float* patches, uint32_t grid_t, uint32_t grid_h,
                                     uint32_t grid_w, float* out, int time_attention_layers);
typedef struct {
    double total_ms, patch_ms, blocks_ms, attention_ms, merger_ms;
    size_t tokens, groups;
} dsocr_dots_timings;
dsocr_status dsocr_dots_last_timings(const dsocr_dots* d, dsocr_dots_timings* t);

#ifdef __cplusplus
}
#endif
#endif /* DSOCR_H */
