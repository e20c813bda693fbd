// C ABI (include/dsocr.h).  Exceptions never cross this boundary: messages are
// prefixed with a status tag ("EINVAL: ...") and mapped to dsocr_status.
#include "../../../include/dsocr.h"

#include <fcntl.h>
#include <signal.h>
#include <unistd.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <utility>

#include "../common/host_util.hpp"
#include "dots.hpp"
#include "engine.hpp"
#include "host_ops.hpp"

struct dsocr_engine {
    std::unique_ptr<dsocr::Engine> impl;
    dsocr::Controls staged;  // the dsocr_session_stage_* calls fill it: consumed by the next admission call
};
struct dsocr_page_pixels {
    dsocr::PagePixels px;
};
struct dsocr_dots {
    std::unique_ptr<dsocr::DotsVision> impl;
};

namespace {
thread_local std::string g_last_error;

dsocr_status status_from(const std::string& msg) {
    g_last_error = msg;
    auto starts = [&](const char* p) { return msg.rfind(p, 0) == 0; };
    if (starts("EINVAL")) return DSOCR_EINVAL;
    if (starts("ENOENT")) return DSOCR_ENOENT;
    if (starts("EDEVICE")) return DSOCR_EDEVICE;
    if (starts("ENOMEM")) return DSOCR_ENOMEM;
    return DSOCR_EINTERNAL;
}

template <typename F>
dsocr_status guarded(F&& f) {
    try {
        f();
        g_last_error.clear();
        return DSOCR_OK;
    } catch (const std::exception& e) {
        return status_from(e.what());
    } catch (...) {
        return status_from("EINTERNAL: unknown error");
    }
}

// Diagnostics (DSOCR_SEGV_MAPS=1): on SIGSEGV write the fault address and /proc/self/maps to stderr
// (async-signal-safe: open/read/write only), then hand the signal back to the handler that was there
// before (a profiler's or the default), so unsymbolised PCs in its stack dump resolve to library + offset.
struct sigaction g_prev_segv;
// "0x" + 16 hex digits of v into out (no libc formatting: snprintf is not async-signal-safe)
size_t hex_u64(uint64_t v, char* out) {
    static const char dig[] = "0123456789abcdef";
    out[0] = '0';
    out[1] = 'x';
    for (int i = 0; i < 16; ++i) out[2 + i] = dig[(v >> (60 - 4 * i)) & 15];
    return 18;
}
void segv_maps_handler(int sig, siginfo_t* si, void* uc) {
    char buf[4096];
    static const char head[] = "\n[dsocr] SIGSEGV at ", tail[] = "; /proc/self/maps follows\n";
    size_t n = 0;
    memcpy(buf, head, sizeof(head) - 1);
    n += sizeof(head) - 1;
    n += hex_u64(si ? (uint64_t)(uintptr_t)si->si_addr : 0, buf + n);
    memcpy(buf + n, tail, sizeof(tail) - 1);
    n += sizeof(tail) - 1;
    (void)!write(2, buf, n);
    const int fd = open("/proc/self/maps", O_RDONLY);
    if (fd >= 0) {
        ssize_t r;
        while ((r = read(fd, buf, sizeof(buf))) > 0) (void)!write(2, buf, (size_t)r);
        close(fd);
    }
    (void)!write(2, "[dsocr] end of maps\n", 20);
    sigaction(SIGSEGV, &g_prev_segv, nullptr);  // the faulting instruction re-runs under the previous handler
    (void)sig;
    (void)uc;
}
void install_segv_maps_once() {
    static bool done = false;
    if (done || !getenv("DSOCR_SEGV_MAPS")) return;
    done = true;
    struct sigaction sa;
    memset(&sa, 0, sizeof(sa));
    sa.sa_sigaction = segv_maps_handler;
    sa.sa_flags = SA_SIGINFO;
    sigemptyset(&sa.sa_mask);
    sigaction(SIGSEGV, &sa, &g_prev_segv);
}

void check_hip(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string("EDEVICE: ") + what + ": " + hipGetErrorString(e));
}

dsocr::GenParams to_params(const dsocr_decode_params* p) {
    if (!p) throw std::runtime_error("EINVAL: decode params are NULL");
    dsocr::GenParams g;
    g.use_cache = p->use_cache != 0;  // false: generate_without_cache (model/mod.rs:2051-2283)
    g.max_new = p->max_new_tokens;
    g.rep_penalty = p->repetition_penalty;
    g.ngram = p->no_repeat_ngram_size > 1 ? (int)p->no_repeat_ngram_size : 0;
    g.eos = p->eos_token_id;
    g.ignore_eos = p->ignore_eos != 0;
    // select_token_id samples only when do_sample && temperature > 0 (sampling.rs:67); otherwise
    // it is the greedy path
    g.do_sample = p->do_sample != 0 && p->temperature > 0.0;
    g.temperature = p->temperature;
    g.top_p = p->top_p;
    g.top_k = (long)p->top_k;
    g.seed_set = p->has_seed != 0;
    g.seed = p->seed;
    return g;
}

dsocr::GenRequest to_request(const dsocr_request& r) {
    dsocr::GenRequest g;
    if (!r.input_ids || r.prompt_len == 0) throw std::runtime_error("EINVAL: empty prompt");
    g.ids.resize(r.prompt_len);
    for (size_t i = 0; i < r.prompt_len; ++i) {
        if (r.input_ids[i] < 0 || r.input_ids[i] > INT32_MAX) throw std::runtime_error("EINVAL: token id out of range");
        g.ids[i] = (int)r.input_ids[i];
    }
    if (r.image_mask) g.mask.assign(r.image_mask, r.image_mask + r.prompt_len);
    g.page = r.page ? &r.page->px : nullptr;
    g.image_rows = r.image_rows;
    g.n_image_rows = r.n_image_rows;
    return g;
}
// the constraint as the engine takes it, checked against `vocab` (NULL: none)
dsocr::LogitBias to_bias(const dsocr_logit_bias* lb, size_t vocab) {
    dsocr::LogitBias b;
    if (!lb) return b;
    if (lb->n && (!lb->ids || !lb->values)) throw std::runtime_error("EINVAL: logit bias: NULL ids / values");
    if (lb->n > vocab) throw std::runtime_error("EINVAL: logit bias: more entries than the vocabulary has ids");
    b.allow_only = lb->allow_only != 0;
    b.ids.resize(lb->n);
    b.values.assign(lb->values, lb->values + lb->n);
    for (size_t i = 0; i < lb->n; ++i) {
        if (lb->ids[i] < 0 || lb->ids[i] >= (int64_t)vocab)
            throw std::runtime_error("EINVAL: logit bias: token id " + std::to_string(lb->ids[i]) + " outside the vocabulary");
        b.ids[i] = (int)lb->ids[i];
    }
    dsocr::validate_logit_bias(b, (int)vocab);
    return b;
}

// the stop set as the engine takes it, checked against `vocab` (NULL or n == 0: none)
dsocr::StopSet to_stops(const dsocr_stop_set* ss, size_t vocab) {
    dsocr::StopSet st;
    if (!ss || ss->n == 0) return st;
    if (!ss->ids || !ss->lens) throw std::runtime_error("EINVAL: stop set: NULL ids / lens");
    if (ss->n > DSOCR_MAX_STOP_SEQS) throw std::runtime_error("EINVAL: stop set: more than DSOCR_MAX_STOP_SEQS sequences");
    size_t off = 0;
    for (size_t i = 0; i < ss->n; ++i) {
        const size_t m = ss->lens[i];
        if (m == 0 || m > DSOCR_MAX_STOP_LEN) throw std::runtime_error("EINVAL: stop set: a sequence has 1..DSOCR_MAX_STOP_LEN token ids");
        std::vector<int> q(m);
        for (size_t j = 0; j < m; ++j) {
            const int64_t t = ss->ids[off + j];
            if (t < 0 || t >= (int64_t)vocab)
                throw std::runtime_error("EINVAL: stop set: token id " + std::to_string(t) + " outside the vocabulary");
            q[j] = (int)t;
        }
        off += m;
        st.seqs.push_back(std::move(q));
    }
    dsocr::validate_stop_set(st, (int)vocab);
    return st;
}

// the penalty record as the engine takes it, checked (NULL: off)
dsocr::Penalties to_penalties(const dsocr_penalties* pn) {
    dsocr::Penalties p;
    if (!pn) return p;
    p.frequency = pn->frequency; p.presence = pn->presence; p.min_p = pn->min_p;
    dsocr::validate_penalties(p);
    return p;
}

// the windowed n-gram ban as the engine takes it, checked against `vocab` (NULL: off)
dsocr::NgramWindow to_ngram_window(const dsocr_ngram_window* nw, size_t vocab) {
    dsocr::NgramWindow w;
    if (!nw) return w;
    if (nw->n_whitelist && !nw->whitelist) throw std::runtime_error("EINVAL: n-gram window: NULL whitelist");
    if (nw->n_whitelist > (size_t)vocab) throw std::runtime_error("EINVAL: n-gram window: more whitelist ids than the vocabulary has");
    w.g = nw->ngram_size; w.w = nw->window;
    w.whitelist.assign(nw->whitelist, nw->whitelist + nw->n_whitelist);
    dsocr::validate_ngram_window(w, (int)vocab);
    return w;
}

// the token automaton as the engine takes it, checked against `vocab` and `eos` (negative: no EOS rule; NULL: off).
// Nothing is read past what the checks so far allow: E comes from a row_ptr already known to be sane
dsocr::Guided to_guided(const dsocr_guided* gd, int vocab, long long eos) {
    dsocr::Guided g;
    if (!gd) return g;
    if (gd->n_states < 1 || gd->n_states > DSOCR_MAX_GUIDED_STATES)
        throw std::runtime_error("EINVAL: token automaton: n_states must be 1.." + std::to_string(DSOCR_MAX_GUIDED_STATES));
    if (!gd->accepting || !gd->row_ptr) throw std::runtime_error("EINVAL: token automaton: NULL accepting or row_ptr");
    const size_t n = (size_t)gd->n_states;
    if (gd->row_ptr[0] != 0) throw std::runtime_error("EINVAL: token automaton: row_ptr must start at 0");
    for (size_t i = 0; i < n; ++i)
        if (gd->row_ptr[i + 1] < gd->row_ptr[i]) throw std::runtime_error("EINVAL: token automaton: row_ptr must not decrease");
    const long E = gd->row_ptr[n];
    if (E > (long)DSOCR_MAX_GUIDED_EDGES)
        throw std::runtime_error("EINVAL: token automaton: more than " + std::to_string(DSOCR_MAX_GUIDED_EDGES) + " edges");
    if (E && (!gd->edge_tok || !gd->edge_next)) throw std::runtime_error("EINVAL: token automaton: NULL edge arrays");
    g.n_states = gd->n_states; g.start = gd->start;
    g.accepting.assign(gd->accepting, gd->accepting + n);
    g.row_ptr.assign(gd->row_ptr, gd->row_ptr + n + 1);
    if (E) {
        g.edge_tok.assign(gd->edge_tok, gd->edge_tok + E);
        g.edge_next.assign(gd->edge_next, gd->edge_next + E);
    }
    dsocr::validate_guided(g, vocab, eos < 0 ? -1L : (long)std::min<long long>(eos, INT32_MAX));
    return g;
}

// a session admission's request: the staged controls move into it (consumed whatever the admission does)
dsocr::GenRequest to_admission(dsocr_engine* e, const dsocr_request& r) {
    dsocr::Controls c = std::exchange(e->staged, dsocr::Controls());
    dsocr::GenRequest g = to_request(r);
    g.ctl = std::move(c);
    return g;
}

// What every dsocr_session_stage_* call does with its control: the staged one is cleared, then `convert` (a to_*
// above: conversion and checks) gives the new one, which needs a session opened with `feature`
template <typename T, typename Convert>
void stage_control(dsocr_engine* e, T dsocr::Controls::*member, bool dsocr::Engine::SessionFeatures::*feature,
                   const char* flag, Convert convert) {
    if (!e) throw std::runtime_error("EINVAL: NULL argument");
    e->staged.*member = T();
    dsocr::Engine::SessionInfo si;
    if (!e->impl->session_info(&si)) throw std::runtime_error("EINVAL: no decode session is open on this engine");
    T v = convert((size_t)e->impl->cfg().lang.vocab);
    if (v.active() && !(si.feat.*feature)) throw std::runtime_error(std::string("EINVAL: this session was opened without ") + flag);
    e->staged.*member = std::move(v);
}

// the DSOCR_SESSION_* feature bits as the engine takes them, and back (DSOCR_SESSION_ADMIT_PENDING is state, not one of them)
const struct { uint32_t bit; bool dsocr::Engine::SessionFeatures::*member; } kSessionFeatures[] = {
    {DSOCR_SESSION_PER_REQUEST, &dsocr::Engine::SessionFeatures::per_request},
    {DSOCR_SESSION_LOGPROBS, &dsocr::Engine::SessionFeatures::logprobs},
    {DSOCR_SESSION_LOGIT_BIAS, &dsocr::Engine::SessionFeatures::logit_bias},
    {DSOCR_SESSION_STOP, &dsocr::Engine::SessionFeatures::stops},
    {DSOCR_SESSION_PENALTIES, &dsocr::Engine::SessionFeatures::penalties},
    {DSOCR_SESSION_NGRAM_WINDOW, &dsocr::Engine::SessionFeatures::ngram_window},
    {DSOCR_SESSION_GUIDED, &dsocr::Engine::SessionFeatures::guided},
};
dsocr::Engine::SessionFeatures to_features(uint32_t flags) {
    dsocr::Engine::SessionFeatures f;
    for (const auto& k : kSessionFeatures) {
        f.*k.member = (flags & k.bit) != 0;
        flags &= ~k.bit;
    }
    if (flags) throw std::runtime_error("EINVAL: unknown session flags");
    return f;
}
uint32_t feature_flags(const dsocr::Engine::SessionFeatures& f) {
    uint32_t flags = 0;
    for (const auto& k : kSessionFeatures) flags |= f.*k.member ? k.bit : 0u;
    return flags;
}

// ---- generate: the exported forms marshal through generate_page (one page, the stream callback) or generate_pages
// (a batch).  They differ in what an output longer than its buffer is: an error there, a truncation here.

// a page's ids into its batch result: what fits, and DSOCR_EINVAL when that is not all of them
void write_result(const std::vector<int64_t>& ids, dsocr_result& out) {
    out.status = DSOCR_OK;
    const size_t m = std::min(ids.size(), out.cap);
    if (out.out_ids) std::memcpy(out.out_ids, ids.data(), m * sizeof(int64_t));
    out.n_out = m;
    if (m < ids.size()) out.status = DSOCR_EINVAL;
}

// page i's entries of the last generate, which ran with lp_k = top_k
void write_logprobs(const dsocr::Engine::LogprobRows& rows, size_t i, size_t top_k, dsocr_logprobs& out) {
    const size_t ne = rows.n.empty() ? 0 : (size_t)rows.n[i];
    out.n = ne;
    for (size_t t = 0; t < ne; ++t) {
        out.token_lp[t] = rows.lp[i * rows.cap + t];
        for (size_t k = 0; k < top_k; ++k) {
            out.top_id[t * top_k + k] = rows.top_id[(i * rows.cap + t) * top_k + k];
            out.top_lp[t * top_k + k] = rows.top_lp[(i * rows.cap + t) * top_k + k];
        }
    }
}

// page i's pair of Engine::last_stop_hits ({-1, 0}: no stop fired, or no page had stops)
void write_stop_hit(const std::vector<int>& sh, size_t i, dsocr_stop_hit& out) {
    out.seq = sh.size() >= 2 * (i + 1) ? sh[2 * i] : -1;
    out.match_len = out.seq >= 0 ? sh[2 * i + 1] : 0;
}

// page i's pair of Engine::last_guided ({0, 0}: the page, or every page, had no automaton)
void write_guided(const std::vector<int>& gs, size_t i, dsocr_guided_result& out) {
    const bool have = gs.size() >= 2 * (i + 1);
    out.state = have ? gs[2 * i] : 0;
    out.status = have ? gs[2 * i + 1] : 0;
}

void generate_page(dsocr_engine* e, const dsocr_request* req, const dsocr_decode_params* params,
                   const dsocr_stop_set* stops, dsocr_stream_cb cb, void* user, int64_t* out_ids, size_t cap,
                   size_t* n_out, dsocr_stop_hit* hit) {
    if (!e || !req || !out_ids || !n_out) throw std::runtime_error("EINVAL: NULL argument");
    std::vector<dsocr::GenRequest> reqs{to_request(*req)};
    reqs[0].ctl.stops = to_stops(stops, (size_t)e->impl->cfg().lang.vocab);
    auto r = e->impl->generate(reqs, to_params(params), cb, user);
    if (r[0].size() > cap) throw std::runtime_error("EINVAL: output capacity too small");
    std::memcpy(out_ids, r[0].data(), r[0].size() * sizeof(int64_t));
    *n_out = r[0].size();
    if (hit) write_stop_hit(e->impl->last_stop_hits(), 0, *hit);
}

// What a batch form asks for beyond the ids.  A new per-request feature adds its fields here and its step to
// generate_pages; its exported form fills the record.
struct GenExtras {
    const dsocr_stop_set* const* stops = nullptr;   // one stop set per request (the list or an entry may be NULL) ...
    dsocr_stop_hit* hits = nullptr;                 // ... and where every request's hit goes
    const dsocr_logit_bias* const* bias = nullptr;  // one constraint per request (the list or an entry may be NULL)
    const dsocr_penalties* const* pen = nullptr;    // one penalty record per request (the same)
    const dsocr_ngram_window* const* ngw = nullptr; // one windowed n-gram ban per request (the same)
    const dsocr_guided* const* guided = nullptr;    // one token automaton per request (the same) ...
    dsocr_guided_result* gres = nullptr;            // ... and where every request's final state and status go
    bool lp_on = false;  // per-token log-probabilities with top_k alternatives into lp[n] (NULL only with n == 0)
    size_t top_k = 0;
    dsocr_logprobs* lp = nullptr;
    float* logits_out = nullptr;  // the raw logits of every step (logits_cap floats)
    size_t logits_cap = 0;
};

void generate_pages(dsocr_engine* e, size_t n, const dsocr_request* reqs, const dsocr_decode_params* params,
                    dsocr_result* results, const GenExtras& x) {
    if (!e || (!reqs && n) || (!results && n) || (x.lp_on && !x.lp && n) || (!params && (x.lp_on || x.logits_out)))
        throw std::runtime_error("EINVAL: NULL argument");
    if (x.top_k > DSOCR_MAX_TOP_LOGPROBS) throw std::runtime_error("EINVAL: top_k above DSOCR_MAX_TOP_LOGPROBS");
    if (!x.lp_on && x.top_k) throw std::runtime_error("EINVAL: top_k without log-probability buffers");
    if (x.lp_on) {
        if (!params->use_cache) throw std::runtime_error("EINVAL: log-probabilities need use_cache = 1");
        for (size_t i = 0; i < n; ++i) {
            if (!x.lp[i].token_lp || (x.top_k && (!x.lp[i].top_id || !x.lp[i].top_lp))) throw std::runtime_error("EINVAL: NULL log-probability buffer");
            if (x.lp[i].cap < (size_t)params->max_new_tokens) throw std::runtime_error("EINVAL: log-probability buffers hold fewer than max_new_tokens entries");
        }
    }
    const size_t vocab = (size_t)e->impl->cfg().lang.vocab;
    if (x.logits_out) {
        const size_t need = n * (size_t)params->max_new_tokens * vocab;
        if (need > x.logits_cap)
            throw std::runtime_error("EINVAL: logits_out holds " + std::to_string(x.logits_cap) + " floats, the trace needs " +
                                     std::to_string(need) + " (n * max_new_tokens * vocab)");
    }
    std::vector<dsocr::GenRequest> rq;
    for (size_t i = 0; i < n; ++i) {
        rq.push_back(to_request(reqs[i]));
        dsocr::Controls& c = rq.back().ctl;
        if (x.bias) c.bias = to_bias(x.bias[i], vocab);
        if (x.stops) c.stops = to_stops(x.stops[i], vocab);
        if (x.pen) c.pen = to_penalties(x.pen[i]);
        if (x.ngw) c.ngw = to_ngram_window(x.ngw[i], vocab);
        if (x.guided) c.guided = to_guided(x.guided[i], (int)vocab, !params || params->ignore_eos ? -1 : (long long)params->eos_token_id);
    }
    dsocr::GenParams g = to_params(params);
    g.trace = x.logits_out;
    if (x.lp_on) g.lp_k = (int)x.top_k;
    auto r = e->impl->generate(rq, g, nullptr, nullptr);
    for (size_t i = 0; i < n; ++i) {
        write_result(r[i], results[i]);
        if (x.hits) write_stop_hit(e->impl->last_stop_hits(), i, x.hits[i]);
        if (x.lp) write_logprobs(e->impl->last_logprobs(), i, x.top_k, x.lp[i]);
        if (x.gres) write_guided(e->impl->last_guided(), i, x.gres[i]);
    }
}
}  // namespace

static dsocr_status prepare_page_device_as(dsocr_engine* e, const uint8_t* rgb, uint32_t w, uint32_t h,
                                           const dsocr_vision_settings* vs, int variant, dsocr_page_pixels** out);

extern "C" {

const char* dsocr_last_error(void) { return g_last_error.c_str(); }

dsocr_status dsocr_engine_load(const dsocr_load_args* args, dsocr_engine** out) {
    const char* e = getenv("DSOCR_DSQ_PACKED");
    const bool packed = e && atoi(e) != 0 && args && args->snapshot_path;
    return dsocr_engine_load_flags(args, packed ? DSOCR_LOAD_PACKED_EXPERTS : 0u, out);
}

dsocr_status dsocr_engine_packed_info(const dsocr_engine* e, size_t* packed_layers, size_t* moe_layers,
                                      size_t* packed_bytes) {
    return guarded([&] {
        if (!e) throw std::runtime_error("EINVAL: NULL engine");
        e->impl->packed_info(packed_layers, moe_layers, packed_bytes);
    });
}

dsocr_status dsocr_engine_load_flags(const dsocr_load_args* args, uint32_t flags, dsocr_engine** out) {
    return guarded([&] {
        if (!args || !out) throw std::runtime_error("EINVAL: NULL argument");
        if (!args->config_path) throw std::runtime_error("EINVAL: config_path is required");
        if (args->dtype < DSOCR_F32 || args->dtype > DSOCR_BF16) throw std::runtime_error("EINVAL: bad dtype");
        install_segv_maps_once();
        auto* e = new dsocr_engine;
        try {
            e->impl.reset(new dsocr::Engine(args->config_path, args->weights_path ? args->weights_path : "",
                                            args->device_ordinal, (int)args->dtype, args->synthetic_seed,
                                            args->snapshot_path ? args->snapshot_path : "", flags));
        } catch (...) {
            delete e;
            throw;
        }
        *out = e;
    });
}

void dsocr_engine_free(dsocr_engine* e) { delete e; }

dsocr_status dsocr_engine_info(const dsocr_engine* e, size_t* hidden, size_t* vocab, int64_t* eos, size_t* layers) {
    return guarded([&] {
        if (!e) throw std::runtime_error("EINVAL: NULL engine");
        const auto& c = e->impl->cfg();
        if (hidden) *hidden = c.lang.hidden;
        if (vocab) *vocab = c.lang.vocab;
        if (eos) *eos = c.lang.eos;
        if (layers) *layers = c.lang.layers;
    });
}

dsocr_status dsocr_prepare_page(const uint8_t* rgb, uint32_t w, uint32_t h, const dsocr_vision_settings* vs,
                                dsocr_page_pixels** out) {
    return dsocr_prepare_page_variant(rgb, w, h, vs, 0, out);
}

dsocr_status dsocr_config_variant(const char* config_path, int* variant, uint32_t* sam_out_channels, uint32_t* encoder) {
    return guarded([&] {
        if (!config_path) throw std::runtime_error("EINVAL: config_path is required");
        std::ifstream f(config_path);
        if (!f) throw std::runtime_error(std::string("ENOENT: cannot read config ") + config_path);
        std::stringstream ss;
        ss << f.rdbuf();
        const dsocr::ModelConfig c = dsocr::resolve_config(dsocr::Json::parse(ss.str()));
        if (variant) *variant = c.variant;
        if (sam_out_channels) { sam_out_channels[0] = c.sam.out_ch[0]; sam_out_channels[1] = c.sam.out_ch[1]; }
        if (encoder) {
            const bool o2 = c.variant == dsocr::VARIANT_OCR2;
            const dsocr::Qwen2EncConfig& q = c.enc;
            const uint32_t v[5] = {(uint32_t)q.dim, (uint32_t)q.layers, (uint32_t)q.heads, (uint32_t)q.kv_heads, (uint32_t)q.inter};
            for (int i = 0; i < 5; ++i) encoder[i] = o2 ? v[i] : 0u;
        }
    });
}

dsocr_status dsocr_engine_variant(const dsocr_engine* e, int* variant) {
    return guarded([&] {
        if (!e || !variant) throw std::runtime_error("EINVAL: NULL argument");
        *variant = e->impl->variant();
    });
}

dsocr_status dsocr_prepare_page_variant(const uint8_t* rgb, uint32_t w, uint32_t h, const dsocr_vision_settings* vs,
                                        int variant, dsocr_page_pixels** out) {
    return guarded([&] {
        if (!rgb || !vs || !out) throw std::runtime_error("EINVAL: NULL argument");
        if (variant != 0 && variant != 1) throw std::runtime_error("EINVAL: variant must be 0 (DeepSeek-OCR) or 1 (DeepSeek-OCR-2)");
        std::unique_ptr<dsocr_page_pixels> p(new dsocr_page_pixels);  // released only on success
        dsocr::PagePixels& px = p->px;
        px.variant = variant;
        px.base = (int)vs->base_size;
        px.tile = (int)vs->image_size;
        px.crop = vs->crop_mode != 0;
        const int gsize = px.crop ? px.base : px.tile;  // model/mod.rs:1714
        if (variant == 1) dsocr::check_ocr2_view_size(gsize, "global view");
        std::vector<uint8_t> gview = dsocr::build_global_view(rgb, (int)w, (int)h, gsize);
        px.gsize = gsize;
        px.global_chw.resize((size_t)3 * gsize * gsize);
        dsocr::image_to_chw(gview.data(), gsize, gsize, px.global_chw.data());
        if (px.crop) {
            int gw = 1, gh = 1;
            auto tiles = dsocr::dynamic_preprocess(rgb, (int)w, (int)h, px.tile, 2, dsocr::tile_max_num(variant), &gw, &gh);
            if (variant == 1 && !tiles.empty()) dsocr::check_ocr2_view_size(px.tile, "tile");
            px.crop_w = gw;
            px.crop_h = gh;
            px.n_tiles = (int)tiles.size();
            px.tiles_chw.resize((size_t)px.n_tiles * 3 * px.tile * px.tile);
            for (int i = 0; i < px.n_tiles; ++i)
                dsocr::image_to_chw(tiles[i].data(), px.tile, px.tile, px.tiles_chw.data() + (size_t)i * 3 * px.tile * px.tile);
        }
        px.n_image_tokens = dsocr::image_placeholder_count(px.base, px.tile, px.crop, px.crop_w, px.crop_h, variant);
        *out = p.release();
    });
}

dsocr_status dsocr_prepare_page_device(dsocr_engine* e, const uint8_t* rgb, uint32_t w, uint32_t h,
                                       const dsocr_vision_settings* vs, dsocr_page_pixels** out) {
    return prepare_page_device_as(e, rgb, w, h, vs, 0, out);
}

dsocr_status dsocr_prepare_page_device_variant(dsocr_engine* e, const uint8_t* rgb, uint32_t w, uint32_t h,
                                               const dsocr_vision_settings* vs, dsocr_page_pixels** out) {
    return prepare_page_device_as(e, rgb, w, h, vs, e ? e->impl->variant() : 0, out);
}

static dsocr_status prepare_page_device_as(dsocr_engine* e, const uint8_t* rgb, uint32_t w, uint32_t h,
                                           const dsocr_vision_settings* vs, int variant, dsocr_page_pixels** out) {
    return guarded([&] {
        if (!e || !rgb || !vs || !out) throw std::runtime_error("EINVAL: NULL argument");
        auto* p = new dsocr_page_pixels;
        p->px.variant = variant;
        p->px.base = (int)vs->base_size;
        p->px.tile = (int)vs->image_size;
        p->px.crop = vs->crop_mode != 0;
        try {
            e->impl->prepare_page_device(rgb, (int)w, (int)h, p->px);
        } catch (...) {
            delete p;
            throw;
        }
        *out = p;
    });
}

dsocr_status dsocr_page_read_device(const dsocr_page_pixels* p, float* global_out, float* tiles_out) {
    return guarded([&] {
        if (!p) throw std::runtime_error("EINVAL: NULL page");
        if (!p->px.global_dev) throw std::runtime_error("EINVAL: page has no device pixels");
        const size_t G = (size_t)p->px.gsize, T = (size_t)p->px.tile;
        check_hip(hipSetDevice(p->px.dev_ordinal), "hipSetDevice");
        if (global_out) check_hip(hipMemcpy(global_out, p->px.global_dev, 3 * G * G * 4, hipMemcpyDeviceToHost), "d2h");
        if (tiles_out && p->px.tiles_dev)
            check_hip(hipMemcpy(tiles_out, p->px.tiles_dev, (size_t)p->px.n_tiles * 3 * T * T * 4, hipMemcpyDeviceToHost), "d2h");
    });
}

void dsocr_page_free(dsocr_page_pixels* p) { delete p; }

dsocr_status dsocr_page_to_device(dsocr_engine* e, dsocr_page_pixels* p) {
    return guarded([&] {
        if (!e || !p) throw std::runtime_error("EINVAL: NULL argument");
        e->impl->upload_page(p->px);
    });
}

dsocr_status dsocr_page_info(const dsocr_page_pixels* p, uint32_t* cw, uint32_t* ch, uint32_t* nt, size_t* ntok) {
    return guarded([&] {
        if (!p) throw std::runtime_error("EINVAL: NULL page");
        if (cw) *cw = p->px.crop_w;
        if (ch) *ch = p->px.crop_h;
        if (nt) *nt = p->px.n_tiles;
        if (ntok) *ntok = p->px.n_image_tokens;
    });
}

dsocr_status dsocr_page_pixels_view(const dsocr_page_pixels* p, const float** g, uint32_t* gs, const float** t,
                                    uint32_t* ts) {
    return guarded([&] {
        if (!p) throw std::runtime_error("EINVAL: NULL page");
        if (g) *g = p->px.global_chw.empty() ? nullptr : p->px.global_chw.data();
        if (gs) *gs = p->px.gsize;
        if (t) *t = p->px.tiles_chw.empty() ? nullptr : p->px.tiles_chw.data();
        if (ts) *ts = p->px.tile;
    });
}

dsocr_status dsocr_image_embeddings(dsocr_engine* e, const dsocr_page_pixels* const* pages, size_t n, float* out,
                                    size_t cap_rows, size_t* rows_per_page) {
    return guarded([&] {
        if (!e || (!pages && n)) throw std::runtime_error("EINVAL: NULL argument");
        std::vector<const dsocr::PagePixels*> ps;
        for (size_t i = 0; i < n; ++i) {
            if (!pages[i]) throw std::runtime_error("EINVAL: page " + std::to_string(i) + " is NULL");
            ps.push_back(&pages[i]->px);
        }
        auto rows = e->impl->image_embeddings(ps);
        const size_t H = e->impl->cfg().lang.hidden;
        size_t off = 0;
        for (size_t i = 0; i < n; ++i) {
            const size_t r = rows[i].size() / H;
            if (rows_per_page) rows_per_page[i] = r;
            if (off + r > cap_rows) throw std::runtime_error("EINVAL: output capacity too small");
            if (out) std::memcpy(out + off * H, rows[i].data(), rows[i].size() * 4);
            off += r;
        }
    });
}

dsocr_status dsocr_generate(dsocr_engine* e, const dsocr_request* req, const dsocr_decode_params* params,
                            dsocr_stream_cb cb, void* user, int64_t* out_ids, size_t cap, size_t* n_out) {
    return guarded([&] { generate_page(e, req, params, nullptr, cb, user, out_ids, cap, n_out, nullptr); });
}

dsocr_status dsocr_generate_stop_stream(dsocr_engine* e, const dsocr_request* req, const dsocr_decode_params* params,
                                        const dsocr_stop_set* stops, dsocr_stream_cb cb, void* user, int64_t* out_ids,
                                        size_t cap, size_t* n_out, dsocr_stop_hit* hit) {
    return guarded([&] { generate_page(e, req, params, stops, cb, user, out_ids, cap, n_out, hit); });
}

dsocr_status dsocr_generate_batch(dsocr_engine* e, size_t n, const dsocr_request* reqs,
                                  const dsocr_decode_params* params, dsocr_result* results) {
    // (NULL params: to_params' error, after the requests')
    return guarded([&] { generate_pages(e, n, reqs, params, results, GenExtras()); });
}

dsocr_status dsocr_generate_trace(dsocr_engine* e, size_t n, const dsocr_request* reqs,
                                  const dsocr_decode_params* params, dsocr_result* results, float* logits_out,
                                  size_t logits_cap) {
    return guarded([&] {
        if (!logits_out || !params) throw std::runtime_error("EINVAL: NULL argument");
        GenExtras x;
        x.logits_out = logits_out;
        x.logits_cap = logits_cap;
        generate_pages(e, n, reqs, params, results, x);
    });
}

dsocr_status dsocr_generate_logprobs(dsocr_engine* e, size_t n, const dsocr_request* reqs,
                                     const dsocr_decode_params* params, dsocr_result* results, size_t top_k,
                                     dsocr_logprobs* lp) {
    return guarded([&] {
        GenExtras x;
        x.lp_on = true;  // whatever lp is: a NULL lp with n > 0 is refused
        x.top_k = top_k;
        x.lp = lp;
        generate_pages(e, n, reqs, params, results, x);
    });
}

// (the narrower control forms are the widest one with NULL lists)
dsocr_status dsocr_generate_stop(dsocr_engine* e, size_t n, const dsocr_request* reqs, const dsocr_decode_params* params,
                                 dsocr_result* results, const dsocr_stop_set* const* stops, dsocr_stop_hit* hits,
                                 const dsocr_logit_bias* const* bias, size_t top_k, dsocr_logprobs* lp) {
    return dsocr_generate_guided(e, n, reqs, params, results, nullptr, nullptr, nullptr, nullptr, stops, hits, bias, top_k, lp);
}

dsocr_status dsocr_generate_penalties(dsocr_engine* e, size_t n, const dsocr_request* reqs,
                                      const dsocr_decode_params* params, dsocr_result* results,
                                      const dsocr_penalties* const* pen, const dsocr_stop_set* const* stops,
                                      dsocr_stop_hit* hits, const dsocr_logit_bias* const* bias, size_t top_k,
                                      dsocr_logprobs* lp) {
    return dsocr_generate_guided(e, n, reqs, params, results, nullptr, nullptr, nullptr, pen, stops, hits, bias, top_k, lp);
}

dsocr_status dsocr_generate_ngram_window(dsocr_engine* e, size_t n, const dsocr_request* reqs,
                                         const dsocr_decode_params* params, dsocr_result* results,
                                         const dsocr_ngram_window* const* ngw, const dsocr_penalties* const* pen,
                                         const dsocr_stop_set* const* stops, dsocr_stop_hit* hits,
                                         const dsocr_logit_bias* const* bias, size_t top_k, dsocr_logprobs* lp) {
    return dsocr_generate_guided(e, n, reqs, params, results, nullptr, nullptr, ngw, pen, stops, hits, bias, top_k, lp);
}

dsocr_status dsocr_ngram_window_check(const dsocr_ngram_window* ngw, size_t vocab) {
    return guarded([&] {
        if (vocab == 0 || vocab > (size_t)INT32_MAX) throw std::runtime_error("EINVAL: bad vocabulary size");
        (void)to_ngram_window(ngw, vocab);
    });
}

dsocr_status dsocr_session_stage_ngram_window(dsocr_engine* e, const dsocr_ngram_window* ngw) {
    return guarded([&] {
        stage_control(e, &dsocr::Controls::ngw, &dsocr::Engine::SessionFeatures::ngram_window, "DSOCR_SESSION_NGRAM_WINDOW",
                      [&](size_t vocab) { return to_ngram_window(ngw, vocab); });
    });
}

dsocr_status dsocr_generate_guided(dsocr_engine* e, size_t n, const dsocr_request* reqs,
                                   const dsocr_decode_params* params, dsocr_result* results,
                                   const dsocr_guided* const* guided, dsocr_guided_result* gres,
                                   const dsocr_ngram_window* const* ngw, const dsocr_penalties* const* pen,
                                   const dsocr_stop_set* const* stops, dsocr_stop_hit* hits,
                                   const dsocr_logit_bias* const* bias, size_t top_k, dsocr_logprobs* lp) {
    return guarded([&] {
        if (!params) throw std::runtime_error("EINVAL: NULL argument");
        GenExtras x;
        x.guided = guided;
        x.gres = gres;
        x.ngw = ngw;
        x.pen = pen;
        x.stops = stops;
        x.hits = hits;
        x.bias = bias;
        x.lp_on = lp != nullptr;  // (top_k without lp is refused)
        x.top_k = top_k;
        x.lp = lp;
        generate_pages(e, n, reqs, params, results, x);
    });
}

dsocr_status dsocr_guided_check(const dsocr_guided* g, int vocab, long long eos) {
    return guarded([&] {
        if (vocab <= 0) throw std::runtime_error("EINVAL: bad vocabulary size");
        (void)to_guided(g, vocab, eos);
    });
}

dsocr_status dsocr_session_stage_guided(dsocr_engine* e, const dsocr_guided* g) {
    return guarded([&] {
        stage_control(e, &dsocr::Controls::guided, &dsocr::Engine::SessionFeatures::guided, "DSOCR_SESSION_GUIDED",
                      [&](size_t vocab) { return to_guided(g, (int)vocab, -1); });  // (the EOS rule: the admission's own check)
    });
}

dsocr_status dsocr_session_guided_state(dsocr_engine* e, int slot, dsocr_guided_result* out) {
    return guarded([&] {
        if (!e || !out) throw std::runtime_error("EINVAL: NULL argument");
        int st = 0, stat = 0;
        e->impl->session_guided_state(slot, &st, &stat);
        out->state = st; out->status = stat;
    });
}

dsocr_status dsocr_penalties_check(const dsocr_penalties* pen) {
    return guarded([&] { (void)to_penalties(pen); });
}

dsocr_status dsocr_session_stage_penalties(dsocr_engine* e, const dsocr_penalties* pen) {
    return guarded([&] {
        stage_control(e, &dsocr::Controls::pen, &dsocr::Engine::SessionFeatures::penalties, "DSOCR_SESSION_PENALTIES",
                      [&](size_t) { return to_penalties(pen); });
    });
}

dsocr_status dsocr_generate_logit_bias(dsocr_engine* e, size_t n, const dsocr_request* reqs,
                                       const dsocr_decode_params* params, dsocr_result* results,
                                       const dsocr_logit_bias* const* bias, size_t top_k, dsocr_logprobs* lp) {
    return dsocr_generate_stop(e, n, reqs, params, results, nullptr, nullptr, bias, top_k, lp);
}

dsocr_status dsocr_logit_bias_check(const dsocr_logit_bias* lb, size_t vocab) {
    return guarded([&] {
        if (vocab == 0 || vocab > (size_t)INT32_MAX) throw std::runtime_error("EINVAL: vocab must be 1..2^31 - 1");
        (void)to_bias(lb, vocab);
    });
}

dsocr_status dsocr_stop_set_check(const dsocr_stop_set* ss, size_t vocab) {
    return guarded([&] {
        if (vocab == 0 || vocab > (size_t)INT32_MAX) throw std::runtime_error("EINVAL: vocab must be 1..2^31 - 1");
        (void)to_stops(ss, vocab);
    });
}

dsocr_status dsocr_session_stage_stop(dsocr_engine* e, const dsocr_stop_set* ss) {
    return guarded([&] {
        stage_control(e, &dsocr::Controls::stops, &dsocr::Engine::SessionFeatures::stops, "DSOCR_SESSION_STOP",
                      [&](size_t vocab) { return to_stops(ss, vocab); });
    });
}

dsocr_status dsocr_session_stop_hit(dsocr_engine* e, int slot, dsocr_stop_hit* out) {
    return guarded([&] {
        if (!e || !out) throw std::runtime_error("EINVAL: NULL argument");
        int seq = -1, len = 0;
        e->impl->session_stop_hit(slot, &seq, &len);
        out->seq = seq; out->match_len = len;
    });
}

dsocr_status dsocr_stop_launches(const dsocr_engine* e, size_t* n) {
    return guarded([&] {
        if (!e || !n) throw std::runtime_error("EINVAL: NULL argument");
        *n = e->impl->stop_launches();
    });
}

dsocr_status dsocr_session_stage_logit_bias(dsocr_engine* e, const dsocr_logit_bias* lb) {
    return guarded([&] {
        stage_control(e, &dsocr::Controls::bias, &dsocr::Engine::SessionFeatures::logit_bias, "DSOCR_SESSION_LOGIT_BIAS",
                      [&](size_t vocab) { return to_bias(lb, vocab); });
    });
}

// ---- decode sessions
dsocr_status dsocr_session_open(dsocr_engine* e, size_t slots, size_t max_context, const dsocr_decode_params* params) {
    return guarded([&] {
        if (!e) throw std::runtime_error("EINVAL: NULL argument");
        if (slots > 8 || max_context > (size_t)INT32_MAX / 2) throw std::runtime_error("EINVAL: a session has 1..8 slots");
        e->impl->session_open((int)slots, (int)max_context, to_params(params), dsocr::Engine::SessionFeatures());
    });
}

dsocr_status dsocr_session_open_ex(dsocr_engine* e, size_t slots, size_t max_context, const dsocr_decode_params* params,
                                   uint32_t flags) {
    return guarded([&] {
        if (!e) throw std::runtime_error("EINVAL: NULL argument");
        const dsocr::Engine::SessionFeatures feat = to_features(flags);
        if (slots > 8 || max_context > (size_t)INT32_MAX / 2) throw std::runtime_error("EINVAL: a session has 1..8 slots");
        e->impl->session_open((int)slots, (int)max_context, to_params(params), feat);
    });
}

dsocr_status dsocr_session_admit_params(dsocr_engine* e, const dsocr_request* req, const dsocr_decode_params* params,
                                        int* slot) {
    return guarded([&] {
        if (!e || !req) throw std::runtime_error("EINVAL: NULL argument");
        const int s = e->impl->session_admit(to_admission(e, *req), to_params(params));
        if (slot) *slot = s;
    });
}

dsocr_status dsocr_session_head_steps(const dsocr_engine* e, size_t* screened, size_t* exact) {
    return guarded([&] {
        if (!e) throw std::runtime_error("EINVAL: NULL argument");
        dsocr::Engine::SessionInfo si;
        if (!e->impl->session_info(&si)) throw std::runtime_error("EINVAL: no decode session is open on this engine");
        if (screened) *screened = si.steps_screened;
        if (exact) *exact = si.steps_exact;
    });
}

dsocr_status dsocr_session_admit(dsocr_engine* e, const dsocr_request* req, size_t max_new_tokens, int has_seed,
                                 uint64_t seed, int* slot) {
    return guarded([&] {
        if (!e || !req) throw std::runtime_error("EINVAL: NULL argument");
        const int s = e->impl->session_admit(to_admission(e, *req), max_new_tokens, has_seed != 0, seed);
        if (slot) *slot = s;
    });
}

namespace {
void session_report(dsocr_engine* e, bool step, size_t k, dsocr_slot_status* status, size_t cap_slots, size_t* n_slots,
                    int64_t* tokens, size_t cap_tokens, size_t* n_tokens) {
    if (!e || !status || !n_slots || !tokens || !n_tokens) throw std::runtime_error("EINVAL: NULL argument");
    dsocr::Engine::SessionInfo si;
    if (!e->impl->session_info(&si)) throw std::runtime_error("EINVAL: no decode session is open on this engine");
    // checked before the poll: a poll hands its tokens out once
    if (cap_slots < (size_t)si.slots || cap_tokens < (size_t)si.slots * si.out_cap)
        throw std::runtime_error("EINVAL: status needs `slots` entries and tokens slots * out_cap");
    if (step && (k == 0 || k > (size_t)INT32_MAX)) throw std::runtime_error("EINVAL: a burst has at least one step");
    const auto st = step ? e->impl->session_step((int)k) : e->impl->session_poll();
    size_t nt = 0;
    for (size_t i = 0; i < st.size(); ++i) {
        status[i].slot = st[i].slot;
        status[i].done = st[i].done;
        status[i].out_len = st[i].out_len;
        status[i].n_new = (int32_t)st[i].fresh.size();
        for (int64_t t : st[i].fresh) tokens[nt++] = t;
    }
    *n_slots = st.size();
    *n_tokens = nt;
}
}  // namespace

dsocr_status dsocr_session_step(dsocr_engine* e, size_t k, dsocr_slot_status* status, size_t cap_slots, size_t* n_slots,
                                int64_t* tokens, size_t cap_tokens, size_t* n_tokens) {
    return guarded([&] { session_report(e, true, k, status, cap_slots, n_slots, tokens, cap_tokens, n_tokens); });
}

dsocr_status dsocr_session_poll(dsocr_engine* e, dsocr_slot_status* status, size_t cap_slots, size_t* n_slots,
                                int64_t* tokens, size_t cap_tokens, size_t* n_tokens) {
    return guarded([&] { session_report(e, false, 0, status, cap_slots, n_slots, tokens, cap_tokens, n_tokens); });
}

dsocr_status dsocr_session_retire(dsocr_engine* e, int slot, int64_t* out_ids, size_t cap, size_t* n_out,
                                  int* moved_from) {
    return guarded([&] {
        if (!e || !out_ids || !n_out) throw std::runtime_error("EINVAL: NULL argument");
        dsocr::Engine::SessionInfo si;
        if (!e->impl->session_info(&si)) throw std::runtime_error("EINVAL: no decode session is open on this engine");
        if (cap < (size_t)si.out_cap) throw std::runtime_error("EINVAL: output capacity too small (the session's out_cap)");
        const auto ids = e->impl->session_retire(slot, moved_from);
        std::memcpy(out_ids, ids.data(), ids.size() * sizeof(int64_t));
        *n_out = ids.size();
    });
}

dsocr_status dsocr_session_close(dsocr_engine* e) {
    return guarded([&] {
        if (!e) throw std::runtime_error("EINVAL: NULL argument");
        e->impl->session_close();
    });
}

dsocr_status dsocr_session_info(const dsocr_engine* e, dsocr_session_desc* out) {
    return guarded([&] {
        if (!e || !out) throw std::runtime_error("EINVAL: NULL argument");
        dsocr::Engine::SessionInfo si;
        if (!e->impl->session_info(&si)) throw std::runtime_error("EINVAL: no decode session is open on this engine");
        out->slots = (size_t)si.slots; out->active = (size_t)si.active; out->max_context = (size_t)si.max_context;
        out->out_cap = (size_t)si.out_cap; out->kv_cap = (size_t)si.kv_cap; out->burst_cap = (size_t)si.burst_cap;
        out->steps = si.steps;
        out->flags = feature_flags(si.feat) | (si.pending ? DSOCR_SESSION_ADMIT_PENDING : 0u);
    });
}

dsocr_status dsocr_session_logprobs(dsocr_engine* e, int slot, size_t first, size_t count, size_t top_k, float* token_lp,
                                    int64_t* top_id, float* top_lp) {
    return guarded([&] {
        if (!e) throw std::runtime_error("EINVAL: NULL argument");
        if (top_k > DSOCR_MAX_TOP_LOGPROBS) throw std::runtime_error("EINVAL: top_k above DSOCR_MAX_TOP_LOGPROBS");
        e->impl->session_logprobs(slot, first, count, (int)top_k, token_lp, top_id, top_lp);
    });
}

// ---- page prefix cache
dsocr_status dsocr_session_prefix_keep(dsocr_engine* e, int slot, size_t rows, int* handle) {
    return guarded([&] {
        if (!e || !handle) throw std::runtime_error("EINVAL: NULL argument");
        if (rows > (size_t)INT32_MAX) throw std::runtime_error("EINVAL: a prefix has 1..prompt_len rows");
        *handle = e->impl->session_prefix_keep(slot, (int)rows);
    });
}

dsocr_status dsocr_session_admit_prefix(dsocr_engine* e, int handle, const dsocr_request* req,
                                        const dsocr_decode_params* params, int* slot) {
    return guarded([&] {
        if (!e || !req) throw std::runtime_error("EINVAL: NULL argument");
        const int s = e->impl->session_admit_prefix(handle, to_admission(e, *req), to_params(params));
        if (slot) *slot = s;
    });
}

// ---- chunked admission
dsocr_status dsocr_session_admit_begin(dsocr_engine* e, const dsocr_request* req, const dsocr_decode_params* params,
                                       size_t chunk_rows, int* ticket) {
    return guarded([&] {
        if (!e || !req) throw std::runtime_error("EINVAL: NULL argument");
        const int rows = (int)std::min(chunk_rows, (size_t)INT32_MAX);
        const int t = e->impl->session_admit_begin(to_admission(e, *req), to_params(params), rows);
        if (ticket) *ticket = t;
    });
}

dsocr_status dsocr_session_admit_advance(dsocr_engine* e, int* done, int* slot) {
    return guarded([&] {
        if (!e || !done) throw std::runtime_error("EINVAL: NULL argument");
        int s = -1;
        *done = e->impl->session_admit_advance(&s) ? 1 : 0;
        if (slot) *slot = s;
    });
}

dsocr_status dsocr_session_admit_cancel(dsocr_engine* e) {
    return guarded([&] {
        if (!e) throw std::runtime_error("EINVAL: NULL argument");
        e->impl->session_admit_cancel();
    });
}

dsocr_status dsocr_session_admit_progress(const dsocr_engine* e, int* pending, size_t* rows_done, size_t* rows_total,
                                          size_t* slices, int* vision_stage, size_t* chunk_attn_launches) {
    return guarded([&] {
        if (!e) throw std::runtime_error("EINVAL: NULL argument");
        dsocr::Engine::SessionInfo si;
        if (!e->impl->session_info(&si)) throw std::runtime_error("EINVAL: no decode session is open on this engine");
        if (pending) *pending = si.pending ? 1 : 0;
        if (rows_done) *rows_done = (size_t)si.pending_rows_done;
        if (rows_total) *rows_total = (size_t)si.pending_rows_total;
        if (slices) *slices = (size_t)si.pending_slices;
        if (vision_stage) *vision_stage = si.pending_stage;
        if (chunk_attn_launches) *chunk_attn_launches = si.chunk_attn_launches;
    });
}

dsocr_status dsocr_session_prefix_drop(dsocr_engine* e, int handle) {
    return guarded([&] {
        if (!e) throw std::runtime_error("EINVAL: NULL argument");
        e->impl->session_prefix_drop(handle);
    });
}

dsocr_status dsocr_session_prefix_stats(const dsocr_engine* e, size_t* entries, size_t* bytes, size_t* admissions,
                                        size_t* rows_reused) {
    return guarded([&] {
        if (!e) throw std::runtime_error("EINVAL: NULL argument");
        const dsocr::Engine::PrefixStats st = e->impl->session_prefix_stats();
        if (entries) *entries = st.entries;
        if (bytes) *bytes = st.bytes;
        if (admissions) *admissions = st.admissions;
        if (rows_reused) *rows_reused = st.rows_reused;
    });
}

dsocr_status dsocr_k_session_prefix_copy(int layers, int slots, int kv_heads, int cap, int hd, float* kc, float* vc,
                                         int slot, int rows, float* entry, int to_slot) {
    return guarded([&] {
        dsocr::PrefixCopyArgs c;
        c.kc = kc; c.vc = vc; c.layers = layers; c.slots = slots; c.kv_heads = kv_heads; c.cap_rows = cap; c.hd = hd;
        c.head_stride = (long)cap * hd; c.page_stride = (long)kv_heads * c.head_stride;
        c.layer_stride = (long)slots * c.page_stride;
        c.slot = slot; c.rows = rows; c.to_slot = to_slot ? 1 : 0; c.entry = entry;
        dsocr::launch_session_prefix_copy(c, nullptr);
        check_hip(hipGetLastError(), "session_prefix_copy launch");
        check_hip(hipDeviceSynchronize(), "session_prefix_copy");
    });
}

dsocr_status dsocr_k_session_slot_move(int layers, int slots, int kv_heads, int cap, int hd, float* kc, float* vc,
                                       int* kv_len, int* kv_pos, int* ctx, long long ctx_cap, int* ctx_len, int* out,
                                       long long out_cap, int* out_len, int* done, int* tok, uint32_t* rng,
                                       int rng_words, int* ban, long long ban_ld, float* x, int H, int src, int dst) {
    return guarded([&] {
        if (ctx_cap < 0 || out_cap < 0 || ban_ld < 0 || rng_words < 0 || H < 0)
            throw std::runtime_error("EINVAL: negative row length");
        dsocr::SlotMoveArgs m;
        m.kc = kc; m.vc = vc; m.layers = layers; m.slots = slots; m.kv_heads = kv_heads; m.cap_rows = cap; m.hd = hd;
        m.head_stride = (long)cap * hd; m.page_stride = (long)kv_heads * m.head_stride;
        m.layer_stride = (long)slots * m.page_stride;
        m.src = src; m.dst = dst; m.rows_bound = cap;
        m.kv_len = kv_len; m.kv_pos = kv_pos; m.ctx = ctx; m.ctx_cap = ctx_cap; m.ctx_len = ctx_len;
        m.out = out; m.out_cap = out_cap; m.out_len = out_len; m.done = done; m.tok = tok;
        m.rng = rng; m.rng_words = rng_words; m.ban = ban; m.ban_ld = ban_ld; m.x = x; m.H = H;
        dsocr::launch_session_slot_move(m, nullptr);
        check_hip(hipDeviceSynchronize(), "session_slot_move");
    });
}

dsocr_status dsocr_last_timings(const dsocr_engine* e, dsocr_timings* t) {
    return guarded([&] {
        if (!e || !t) throw std::runtime_error("EINVAL: NULL argument");
        dsocr::Timings x = e->impl->last_timings();
        t->vision_prepare_ms = x.vision_prepare_ms;
        t->vision_compute_ms = x.vision_compute_ms;
        t->decode_prefill_ms = x.prefill_ms;
        t->decode_iterative_ms = x.iterative_ms;
        t->decode_generate_ms = x.generate_ms;
        t->decode_steps = x.steps;
        t->pages = x.pages;
        t->vision_flops = x.vision_flops;
        t->prefill_flops = x.prefill_flops;
    });
}

dsocr_status dsocr_profile_decode(dsocr_engine* e, int iters, dsocr_decode_profile* out) {
    return guarded([&] {
        if (!e || iters <= 0 || !out) throw std::runtime_error("EINVAL: bad arguments");
        auto p = e->impl->profile_decode(iters);
        auto cp = [](const dsocr::Engine::KernelProfile& k) {
            dsocr_kernel_profile r;
            r.avg_us = k.avg_us; r.bytes = k.bytes; r.flops = k.flops; r.launches = k.launches; r.replay_us = k.replay_us;
            r.ctx_us = k.ctx_us;
            return r;
        };
        out->moe_gateup = cp(p.moe_gateup);
        out->moe_down = cp(p.moe_down);
        out->attention = cp(p.attention);
        out->lm_head = cp(p.lm_head);
        out->experts_touched = p.experts_touched;
        out->tokens = p.tokens;
        out->kv_len = p.kv_len;
        out->qkv = cp(p.qkv);
        out->o_proj = cp(p.o_proj);
        out->router = cp(p.router);
        out->layers_step = cp(p.layers_step);
        out->lm_head_screened = cp(p.lm_head_screened);
        out->moe_gateup_kernel = p.gateup_kernel;
        out->moe_down_kernel = p.down_kernel;
    });
}

// ---------------------------------------------------------------- device helpers
dsocr_status dsocr_engine_set_spans(dsocr_engine* e, int enable) {
    return guarded([&] {
        if (!e) throw std::runtime_error("EINVAL: NULL engine");
        e->impl->set_spans(enable);
    });
}

dsocr_status dsocr_engine_spans(const dsocr_engine* e, uint64_t* out, size_t cap, size_t* kinds, size_t* layers,
                                size_t* steps) {
    return guarded([&] {
        if (!e) throw std::runtime_error("EINVAL: NULL engine");
        const auto& v = e->impl->spans();
        const size_t nl = e->impl->cfg().lang.layers;
        const size_t ns = v.empty() ? 0 : (size_t)e->impl->span_steps();
        if (kinds) *kinds = (size_t)e->impl->span_kinds();
        if (layers) *layers = nl;
        if (steps) *steps = ns;
        if (!out) return;  // size query
        if (v.size() > cap)
            throw std::runtime_error("EINVAL: span buffer holds " + std::to_string(cap) + " values, " +
                                     std::to_string(v.size()) + " needed");
        if (!v.empty()) std::memcpy(out, v.data(), v.size() * 8);
    });
}
static_assert(dsocr::Engine::SPAN_FIELDS == 5, "dsocr.h documents 5 fields per span record");

dsocr_status dsocr_engine_set_persist_stamps(dsocr_engine* e, int mode) {
    return guarded([&] {
        if (!e) throw std::runtime_error("EINVAL: NULL engine");
        e->impl->set_persist_stamps(mode);
    });
}

dsocr_status dsocr_engine_persist_info(const dsocr_engine* e, int* used, double* durations, size_t cap_d,
                                       size_t* n_launches, uint64_t* stamps, size_t cap_s, size_t* n_stamps) {
    return guarded([&] {
        if (!e) throw std::runtime_error("EINVAL: NULL engine");
        const auto& d = e->impl->persist_launch_us();
        const auto& st = e->impl->persist_stamps();
        if (used) *used = e->impl->persist_used() ? 1 : 0;
        if (n_launches) *n_launches = d.size();
        if (n_stamps) *n_stamps = st.size();
        if (durations) {
            if (d.size() > cap_d) throw std::runtime_error("EINVAL: duration buffer too small");
            if (!d.empty()) std::memcpy(durations, d.data(), d.size() * sizeof(double));
        }
        if (stamps) {
            if (st.size() > cap_s) throw std::runtime_error("EINVAL: stamp buffer too small");
            if (!st.empty()) std::memcpy(stamps, st.data(), st.size() * 8);
        }
    });
}

dsocr_status dsocr_device_count(int* n) {
    return guarded([&] { check_hip(hipGetDeviceCount(n), "hipGetDeviceCount"); });
}
dsocr_status dsocr_dev_alloc(size_t bytes, void** ptr) {
    return guarded([&] {
        if (hipMalloc(ptr, bytes ? bytes : 16) != hipSuccess) throw std::runtime_error("ENOMEM: hipMalloc failed");
    });
}
dsocr_status dsocr_dev_free(void* ptr) {
    return guarded([&] { check_hip(hipFree(ptr), "hipFree"); });
}
dsocr_status dsocr_memcpy_h2d(void* dst, const void* src, size_t bytes) {
    return guarded([&] { check_hip(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice), "hipMemcpy H2D"); });
}
dsocr_status dsocr_memcpy_d2h(void* dst, const void* src, size_t bytes) {
    return guarded([&] { check_hip(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost), "hipMemcpy D2H"); });
}
dsocr_status dsocr_dev_sync(void) {
    return guarded([&] { check_hip(hipDeviceSynchronize(), "hipDeviceSynchronize"); });
}
dsocr_status dsocr_synth_bf16(const char* name, uint64_t seed, uint64_t n, uint16_t* out) {
    return guarded([&] {
        if (!name || (!out && n)) throw std::runtime_error("EINVAL: NULL argument");
        dsocr::synth_bf16(name, seed, n, out);
    });
}
dsocr_status dsocr_resize_bicubic(const uint8_t* src, uint32_t sw, uint32_t sh, uint8_t* dst, uint32_t dw, uint32_t dh) {
    return guarded([&] {
        if (!src || !dst) throw std::runtime_error("EINVAL: NULL argument");
        dsocr::resize_bicubic(src, (int)sw, (int)sh, dst, (int)dw, (int)dh);
    });
}

dsocr_status dsocr_resize_catmull_rom(const uint8_t* src, uint32_t sw, uint32_t sh, uint8_t* dst, uint32_t dw,
                                      uint32_t dh) {
    return guarded([&] {
        if (!src || !dst || !sw || !sh || !dw || !dh) throw std::runtime_error("EINVAL: NULL argument or empty image");
        dsocr::resize_catmull_rom_fir(src, (int)sw, (int)sh, dst, (int)dw, (int)dh);
    });
}

// ---------------------------------------------------------------- kernel-level entry points
dsocr_status dsocr_k_gemm(int M, int N, int K, const float* A, const void* W, int wdtype, const float* bias, float* C,
                          int act, int accumulate) {
    return guarded([&] {
        if (K % 8) throw std::runtime_error("EINVAL: K must be a multiple of 8");
        dsocr::GemmArgs g;
        g.M = M; g.N = N; g.K = K; g.A = A; g.lda = K; g.W = W; g.ldw = K; g.wdtype = wdtype; g.bias = bias;
        g.C = C; g.ldc = N; g.act = act; g.accumulate = accumulate;
        dsocr::launch_gemm(g, nullptr);
        check_hip(hipGetLastError(), "gemm launch");
        check_hip(hipDeviceSynchronize(), "gemm");
    });
}
dsocr_status dsocr_k_gemm_grouped(int M, int N, int K, const float* A, int lda, const int* a_rows, const void* W,
                                  int wdtype, long long w_group_stride, const float* bias, long long bias_group_stride,
                                  float* C, int ldc, const int* c_rows, int act, int accumulate, const int* group_off,
                                  int groups, int max_group_rows, int kernel) {
    return guarded([&] {
        if (!A || !W || !C || !group_off || groups < 1 || M < 0 || N < 1 || K < 1)
            throw std::runtime_error("EINVAL: grouped gemm arguments");
        dsocr::GemmArgs g;
        g.M = M; g.N = N; g.K = K; g.A = A; g.lda = lda; g.a_rows = a_rows; g.W = W; g.ldw = K; g.wdtype = wdtype;
        g.w_group_stride = (long)w_group_stride; g.bias = bias; g.bias_group_stride = (long)bias_group_stride;
        g.C = C; g.ldc = ldc; g.c_rows = c_rows; g.act = act; g.accumulate = accumulate;
        g.group_off = group_off; g.groups = groups; g.max_group_rows = max_group_rows;
        if (kernel == 1 || kernel == 2) dsocr::launch_gemm_f32a_grouped(g, nullptr, kernel == 2 ? 128 : 32);
        else dsocr::launch_gemm(g, nullptr);
        check_hip(hipGetLastError(), "grouped gemm launch");
        check_hip(hipDeviceSynchronize(), "grouped gemm");
    });
}
dsocr_status dsocr_k_gemm_f32a(int M, int N, int K, const float* A, const void* W, int wdtype, const float* bias,
                               float* C, int act, int accumulate, int splits) {
    return guarded([&] {
        if (wdtype != dsocr::WDT_BF16 && wdtype != dsocr::WDT_F16) throw std::runtime_error("EINVAL: weights must be bf16 or f16");
        dsocr::GemmBf16Args g;
        g.M = M; g.N = N; g.K = K; g.A = A; g.lda = K; g.W = W; g.ldw = K; g.bias = bias;
        g.w_f16 = wdtype == dsocr::WDT_F16;
        g.C = C; g.ldc = N; g.act = act; g.accumulate = accumulate;
        if (!dsocr::gemm_f32a_ok(g)) throw std::runtime_error("EINVAL: gemm_f32a needs K % 32 == 0 and 16-byte aligned rows");
        g.splits = splits > 0 ? splits : dsocr::gemm_f32a_splits(M, N, K);
        float* part = nullptr;
        if (g.splits > 1) {
            check_hip(hipMalloc(&part, sizeof(float) * (size_t)g.splits * M * N), "hipMalloc");
            g.part = part;
        }
        dsocr::launch_gemm_f32a(g, nullptr);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (part) (void)hipFree(part);
        check_hip(e, "gemm_f32a");
    });
}
dsocr_status dsocr_k_gemv(int M, int N, int K, const float* x, const float* norm_w, float eps, const void* W,
                          int wdtype, const float* bias, float* y, int act, int accumulate) {
    return dsocr_k_gemv_ex(M, N, K, x, K, norm_w, eps, W, K, wdtype, bias, y, N, act, accumulate, 0, nullptr);
}
static bool gemv_kind_is_mm(const char* kind) { return std::strncmp(kind, "dec_mm_", 7) == 0; }
dsocr_status dsocr_k_gemv_ex(int M, int N, int K, const float* x, int ldx, const float* norm_w, float eps,
                             const void* W, int ldw, int wdtype, const float* bias, float* y, int ldy, int act,
                             int accumulate, int swizzle, const char** kind) {
    return guarded([&] {
        if (K < 8 || K % 8) throw std::runtime_error("EINVAL: K must be a positive multiple of 8");
        if (M < 0 || N < 0 || ldx < K || ldw < K || ldy < N || ldx % 4 || ldw % 8)
            throw std::runtime_error("EINVAL: gemv strides (ldx >= K, ldx % 4 == 0, ldw >= K, ldw % 8 == 0, ldy >= N)");
        if (wdtype != dsocr::WDT_BF16 && wdtype != dsocr::WDT_F16) throw std::runtime_error("EINVAL: weights must be bf16 or f16");
        dsocr::DecGemvArgs a;
        a.M = M; a.N = N; a.K = K; a.x = x; a.ldx = ldx; a.W = W; a.ldw = ldw; a.wdtype = wdtype; a.bias = bias;
        a.y = y; a.ldy = ldy; a.act = act; a.accumulate = accumulate; a.norm_w = norm_w; a.eps = eps;
        void* swz = nullptr;
        if (swizzle) {
            // the fragment-ordered form runs only where the dispatch takes dec_mm: anything else is refused, so
            // a caller never believes it ran the swizzled kernel when it did not
            if (ldw != K) throw std::runtime_error("EINVAL: swizzle needs row-major W with ldw == K");
            if (!dsocr::dec_mm_ok(a) || !gemv_kind_is_mm(dsocr::dec_gemv_kernel_kind(a)))
                throw std::runtime_error("EINVAL: swizzle outside dec_mm's range (M 3..8, K 1280, N >= 16)");
            check_hip(hipMalloc(&swz, sizeof(uint16_t) * dsocr::mm_swizzle_elems(N, K)), "hipMalloc");
            a.w_swz = swz;
        }
        if (kind) *kind = dsocr::dec_gemv_kernel_kind(a);
        hipError_t e = hipSuccess;
        try {
            if (swz) dsocr::launch_mm_swizzle(W, N, K, swz, nullptr);
            dsocr::launch_dec_gemv(a, nullptr);
            e = hipGetLastError();
        } catch (...) {
            (void)hipDeviceSynchronize();
            if (swz) (void)hipFree(swz);
            throw;
        }
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (swz) (void)hipFree(swz);
        check_hip(e, "gemv");
    });
}
dsocr_status dsocr_k_gemv_kind(int M, int N, int K, int ldw, int wdtype, int has_norm, int has_xn_out, int swizzle,
                               const char** kind, int* rows_per_launch) {
    return guarded([&] {
        if (!kind) throw std::runtime_error("EINVAL: NULL argument");
        // only which pointers are set matters to the decision; none is dereferenced
        static float fd = 0.f;
        static uint16_t wd = 0;
        dsocr::DecGemvArgs a;
        a.M = M; a.N = N; a.K = K; a.x = &fd; a.ldx = K; a.W = &wd; a.ldw = ldw; a.wdtype = wdtype;
        a.y = &fd; a.ldy = N; a.norm_w = has_norm ? &fd : nullptr; a.xn_out = has_xn_out ? &fd : nullptr;
        a.w_swz = swizzle ? &wd : nullptr;
        *kind = dsocr::dec_gemv_kernel_kind(a, rows_per_launch);
    });
}
dsocr_status dsocr_k_mm_swizzle(int N, int K, const void* w, void* out) {
    return guarded([&] {
        if (N < 1 || K < 32 || K % 32 || !w || !out) throw std::runtime_error("EINVAL: mm_swizzle needs N >= 1, K % 32 == 0, w, out");
        dsocr::launch_mm_swizzle(w, N, K, out, nullptr);
        check_hip(hipGetLastError(), "mm_swizzle launch");
        check_hip(hipDeviceSynchronize(), "mm_swizzle");
    });
}
dsocr_status dsocr_k_silu_mul(int rows, int I, const float* g, int ldg, float* h, int ldh) {
    return guarded([&] {
        if (rows < 0 || I < 1 || ldg < 2 * I || ldh < I || !g || !h) throw std::runtime_error("EINVAL: silu_mul needs ldg >= 2 I, ldh >= I");
        dsocr::launch_silu_mul(g, ldg, I, rows, h, ldh, nullptr);
        check_hip(hipGetLastError(), "silu_mul launch");
        check_hip(hipDeviceSynchronize(), "silu_mul");
    });
}
dsocr_status dsocr_k_gemv_splitk(int M, int N, int K, const float* x, const void* W, int wdtype, const float* bias,
                                 float* y, int accumulate) {
    return guarded([&] {
        dsocr::DecGemvArgs a;
        a.M = M; a.N = N; a.K = K; a.x = x; a.ldx = K; a.W = W; a.ldw = K; a.wdtype = wdtype; a.bias = bias;
        a.y = y; a.ldy = N; a.accumulate = accumulate;
        if (!dsocr::dec_mm_splitk_ok(a)) throw std::runtime_error("EINVAL: gemv_splitk needs M <= 8, K % 64 == 0");
        float* part = nullptr;
        int* tick = nullptr;
        check_hip(hipMalloc(&part, sizeof(float) * dsocr::dec_mm_splitk_part_floats(N, K)), "hipMalloc");
        check_hip(hipMalloc(&tick, sizeof(int) * dsocr::dec_mm_splitk_ticks(N)), "hipMalloc");
        check_hip(hipMemset(tick, 0, sizeof(int) * dsocr::dec_mm_splitk_ticks(N)), "hipMemset");
        dsocr::launch_dec_mm_splitk(a, part, tick, nullptr);
        hipError_t e = hipDeviceSynchronize();
        (void)hipFree(part);
        (void)hipFree(tick);
        check_hip(e, "gemv_splitk");
    });
}
dsocr_status dsocr_k_layernorm(int rows, int cols, const float* x, const float* w, const float* b, float eps, float* y) {
    return guarded([&] {
        if (cols % 4) throw std::runtime_error("EINVAL: cols must be a multiple of 4");
        dsocr::launch_layernorm(x, cols, y, cols, nullptr, rows, cols, w, b, eps, nullptr);
        check_hip(hipDeviceSynchronize(), "layernorm");
    });
}
dsocr_status dsocr_k_dsq_dequant(int qtype, const void* src, size_t src_bytes, size_t out_dim, size_t in_dim,
                                 void* out_f16) {
    return guarded([&] {
        const size_t need = dsocr::dsq_payload_bytes(qtype, (long)out_dim, (long)in_dim);
        if (need == 0) throw std::runtime_error("EINVAL: unsupported snapshot tensor dtype code " + std::to_string(qtype));
        if (src_bytes != need)
            throw std::runtime_error("EINVAL: payload is " + std::to_string(src_bytes) + " bytes, expected " + std::to_string(need));
        dsocr::launch_dsq_dequant(qtype, src, (long)out_dim, (long)in_dim, out_f16, nullptr);
        check_hip(hipGetLastError(), "dsq_dequant launch");
        check_hip(hipDeviceSynchronize(), "dsq_dequant");
    });
}
dsocr_status dsocr_k_rmsnorm(int rows, int cols, const float* x, const float* w, float eps, float* y) {
    return guarded([&] {
        if (cols % 4) throw std::runtime_error("EINVAL: cols must be a multiple of 4");
        dsocr::launch_rmsnorm(x, cols, y, cols, rows, cols, w, eps, nullptr);
        check_hip(hipDeviceSynchronize(), "rmsnorm");
    });
}
dsocr_status dsocr_k_attention(int n_seq, int L, int heads, int hd, float scale, int causal, const float* q,
                               const float* k, const float* v, float* o, const float* relh, const float* relw, int gh,
                               int gw) {
    return guarded([&] {
        if (hd != 32 && hd != 64 && hd != 128) throw std::runtime_error("EINVAL: head_dim must be 32, 64 or 128");
        const long C = (long)heads * hd;
        dsocr::AttnArgs a;
        a.q = {q, C, hd, nullptr};
        a.k = {k, C, hd, nullptr};
        a.v = {v, C, hd, nullptr};
        a.o = o; a.o_row_stride = C; a.o_head_stride = hd; a.n_seq = n_seq; a.L = L; a.heads = heads;
        a.kv_heads = heads; a.hd = hd; a.scale = scale; a.causal = causal;
        float* rb = nullptr;
        float* part = nullptr;
        if (causal) {  // the engine's prefill form: key pieces + combine
            a.part_floats = dsocr::attention_causal_part_floats(n_seq, heads, L, hd);
            check_hip(hipMalloc(&part, sizeof(float) * a.part_floats), "hipMalloc attention pieces");
            a.part = part;
        }
        if (relh && relw) {
            if (gh * gw != L) throw std::runtime_error("EINVAL: rel-pos grid does not match L");
            check_hip(hipMalloc(&rb, sizeof(float) * (size_t)n_seq * heads * L * (gh + gw)), "hipMalloc relbias");
            dsocr::launch_sam_relbias(q, C, n_seq, gh, gw, heads, hd, relh, relw, rb, nullptr);
            a.relbias = rb; a.rel_h = gh; a.rel_w = gw;
        }
        dsocr::launch_attention(a, nullptr);
        hipError_t e = hipDeviceSynchronize();
        if (rb) (void)hipFree(rb);
        if (part) (void)hipFree(part);
        check_hip(e, "attention");
    });
}
dsocr_status dsocr_k_attention_prefix(int n_seq, int L, int prefix, int heads, int kv_heads, int hd, float scale,
                                      const float* q, const float* k, const float* v, float* o) {
    return guarded([&] {
        dsocr::AttnPrefixArgs a;
        a.q = q; a.k = k; a.v = v; a.o = o;
        a.ldq = a.ldo = (long)heads * hd;
        a.ldk = a.ldv = (long)kv_heads * hd;
        a.n_seq = n_seq; a.L = L; a.prefix = prefix; a.heads = heads; a.kv_heads = kv_heads; a.hd = hd; a.scale = scale;
        if (!dsocr::attention_prefix_ok(a))
            throw std::runtime_error("EINVAL: attention_prefix needs hd 32 or 64, heads % kv_heads == 0, 0 <= prefix <= L "
                                     "and 16-byte aligned device pointers");
        dsocr::launch_attention_prefix(a, nullptr);
        check_hip(hipGetLastError(), "attention_prefix launch");
        check_hip(hipDeviceSynchronize(), "attention_prefix");
    });
}
dsocr_status dsocr_k_attention_bf16(int n_seq, int L, int heads, int hd, float scale, const void* qkv, long ld,
                                    void* o, long o_ld, int o_bf16) {
    return guarded([&] {
        if (!qkv || !o || n_seq <= 0 || L <= 0 || heads <= 0) throw std::runtime_error("EINVAL: bad attention arguments");
        const long D = (long)heads * hd;
        if (ld < 3 * D || o_ld < D) throw std::runtime_error("EINVAL: row strides too small");
        dsocr::AttnBf16Args a;
        a.q = (const uint16_t*)qkv; a.k = (const uint16_t*)qkv + D; a.v = (const uint16_t*)qkv + 2 * D;
        a.q_rs = a.k_rs = a.v_rs = ld; a.q_hs = a.k_hs = a.v_hs = hd;
        a.o = o; a.o_rs = o_ld; a.o_hs = hd; a.o_bf16 = o_bf16;
        a.n_seq = n_seq; a.L = L; a.heads = heads; a.kv_heads = heads; a.hd = hd; a.scale = scale;
        const char* pv = getenv("DSOCR_DOTS_PV_PLANES");  // the tower's P.V plane count (3 unless set to 2)
        a.pv_planes = (pv && atoi(pv) == 2) ? 2 : 3;
        dsocr::launch_attention_bf16(a, nullptr);
        check_hip(hipGetLastError(), "attention_bf16 launch");
        check_hip(hipDeviceSynchronize(), "attention_bf16");
    });
}
dsocr_status dsocr_k_gemm_bf16(int M, int N, int K, const void* A, long lda, const void* W, long ldw, const float* bias,
                               void* C, long ldc, int out_bf16, int accumulate, int variant, int group_m, int swiglu,
                               const float* rope_cos, const float* rope_sin, int rope_cols) {
    return guarded([&] {
        if (!A || !W || !C || M < 0 || N < 1 || K < 1) throw std::runtime_error("EINVAL: bad gemm_bf16 arguments");
        if (lda < K || ldw < K || ldc < (swiglu ? N / 2 : N)) throw std::runtime_error("EINVAL: row strides too small");
        if (variant != 0 && variant != 2 && variant != 3) throw std::runtime_error("EINVAL: variant must be 0, 2 or 3");
        // variant 3 names the ping-pong kernel: refuse what the launcher would quietly hand to the 128 x 128 one
        if (variant == 3 && (!out_bf16 || ldc % 8 || (reinterpret_cast<uintptr_t>(C) & 15)))
            throw std::runtime_error("EINVAL: the ping-pong kernel needs bf16 out and 16-byte aligned C rows");
        dsocr::GemmBf16Args g;
        g.M = M; g.N = N; g.K = K; g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias;
        g.C = reinterpret_cast<float*>(C); g.ldc = ldc; g.out_bf16 = out_bf16; g.accumulate = accumulate;
        g.variant = variant; g.group_m = group_m; g.swiglu = swiglu;
        g.rope_cos = rope_cos; g.rope_sin = rope_sin; g.rope_cols = rope_cols;
        dsocr::launch_gemm_bf16(g, nullptr);
        check_hip(hipGetLastError(), "gemm_bf16 launch");
        check_hip(hipDeviceSynchronize(), "gemm_bf16");
    });
}
dsocr_status dsocr_k_dots_op(int op, long rows, int cols, int aux, long ld, const void* x, const float* p0,
                             const float* p1, float eps, void* y) {
    return guarded([&] {
        if (!y || rows < 0 || cols < 1) throw std::runtime_error("EINVAL: bad dots_op arguments");
        auto need = [](bool ok, const char* what) {
            if (!ok) throw std::runtime_error(std::string("EINVAL: dots_op needs ") + what);
        };
        switch (op) {
        case DSOCR_DOTS_RMSNORM:
            need(x && p0, "x and w");
            dsocr::launch_dots_rmsnorm(x, aux, rows, cols, p0, eps, y, nullptr);
            break;
        case DSOCR_DOTS_LAYERNORM:
            need(x && p0 && p1, "x, w and b");
            dsocr::launch_dots_layernorm(x, rows, cols, p0, p1, eps, y, nullptr);
            break;
        case DSOCR_DOTS_SWIGLU:
            need(x, "gu");
            dsocr::launch_dots_swiglu(x, rows, cols, y, nullptr);
            break;
        case DSOCR_DOTS_GELU:
            dsocr::launch_dots_gelu(y, rows * (long)cols, nullptr);
            break;
        case DSOCR_DOTS_ROPE_QK:
            need(x && p0 && p1 && aux > 0, "qkv, cos, sin and a head count");
            dsocr::launch_dots_rope_qk(x, rows, aux, cols, p0, p1, y, nullptr);
            break;
        case DSOCR_DOTS_TO_BF16:
            need(x && ld >= cols && aux >= cols, "x and row strides >= cols");
            dsocr::launch_dots_to_bf16(reinterpret_cast<const float*>(x), rows, cols, ld, y, aux, nullptr);
            break;
        case DSOCR_DOTS_BF16_TO_F32:
            need(x, "x");
            dsocr::launch_dots_bf16_to_f32(x, rows * (long)cols, reinterpret_cast<float*>(y), nullptr);
            break;
        default:
            throw std::runtime_error("EINVAL: unknown dots op " + std::to_string(op));
        }
        check_hip(hipGetLastError(), "dots_op launch");
        check_hip(hipDeviceSynchronize(), "dots_op");
    });
}
// ---------------------------------------------------------------- the vision tower's kernels in the engine's forms
// a device row map (c_rows / out_rows) read back and checked against the rows of the buffer it scatters into
static void check_row_map(const int* d_map, int n, int cap, const char* what) {
    std::vector<int> h((size_t)n);
    if (n) check_hip(hipMemcpy(h.data(), d_map, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost), "hipMemcpy row map");
    for (int v : h)
        if (v < -1 || v >= cap) throw std::runtime_error(std::string("EINVAL: ") + what + " entry outside [-1, rows of the target)");
}
dsocr_status dsocr_k_gemm_f32a_ex(int M, int N, int K, const float* A, long lda, const void* W, int wdtype,
                                  const float* bias, float* C, long ldc, const int* c_rows, int c_cap, int act,
                                  int accumulate, int variant, int splits, int* splits_used) {
    return guarded([&] {
        if (!A || !W || !C || M < 1 || N < 1 || K < 1) throw std::runtime_error("EINVAL: bad gemm_f32a arguments");
        if (wdtype != dsocr::WDT_BF16 && wdtype != dsocr::WDT_F16) throw std::runtime_error("EINVAL: weights must be bf16 or f16");
        if (lda < K || ldc < N) throw std::runtime_error("EINVAL: row strides too small");
        if (variant != 0 && variant != 2) throw std::runtime_error("EINVAL: variant must be 0 or 2");
        if (splits < 0 || splits > std::max(1, K / 32)) throw std::runtime_error("EINVAL: splits must be 0 .. K / 32");
        if (c_rows) check_row_map(c_rows, M, c_cap, "c_rows");
        dsocr::GemmBf16Args g;
        g.M = M; g.N = N; g.K = K; g.A = A; g.lda = lda; g.W = W; g.ldw = K; g.bias = bias;
        g.w_f16 = wdtype == dsocr::WDT_F16;
        g.C = C; g.ldc = ldc; g.c_rows = c_rows; g.act = act; g.accumulate = accumulate; g.variant = variant;
        if (!dsocr::gemm_f32a_ok(g)) throw std::runtime_error("EINVAL: gemm_f32a needs K % 32 == 0 and 16-byte aligned rows");
        // Engine::linear: the split count by the shape, the workspace [splits][M][N] only when there is a reduce
        g.splits = splits > 0 ? splits : dsocr::gemm_f32a_splits(M, N, K);
        float* part = nullptr;
        if (g.splits > 1) {
            check_hip(hipMalloc(&part, sizeof(float) * (size_t)g.splits * M * N), "hipMalloc");
            g.part = part;
        }
        if (splits_used) *splits_used = g.splits;
        dsocr::launch_gemm_f32a(g, nullptr);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (part) (void)hipFree(part);
        check_hip(e, "gemm_f32a_ex");
    });
}
dsocr_status dsocr_k_layernorm_ex(int rows, int cols, const float* x, int ldx, const float* w, const float* b, float eps,
                                  float* y, int ldy, const int* out_rows, int y_rows) {
    return guarded([&] {
        if (!x || !w || !b || !y || rows < 0 || cols < 1) throw std::runtime_error("EINVAL: bad layernorm arguments");
        if (cols % 4 || ldx % 4 || ldy % 4 || ldx < cols || ldy < cols)
            throw std::runtime_error("EINVAL: cols and the row strides must be multiples of 4, strides >= cols");
        if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(w) |
             reinterpret_cast<uintptr_t>(b)) & 15)
            throw std::runtime_error("EINVAL: layernorm needs 16-byte aligned pointers");
        if (out_rows) check_row_map(out_rows, rows, y_rows, "out_rows");
        dsocr::launch_layernorm(x, ldx, y, ldy, out_rows, rows, cols, w, b, eps, nullptr);
        check_hip(hipGetLastError(), "layernorm launch");
        check_hip(hipDeviceSynchronize(), "layernorm");
    });
}
dsocr_status dsocr_k_rmsnorm_ex(int rows, int cols, const float* x, int ldx, const float* w, float eps, float* y,
                                int ldy) {
    return guarded([&] {
        if (!x || !w || !y || rows < 0 || cols < 1) throw std::runtime_error("EINVAL: bad rmsnorm arguments");
        if (cols % 4 || ldx % 4 || ldy % 4 || ldx < cols || ldy < cols)
            throw std::runtime_error("EINVAL: cols and the row strides must be multiples of 4, strides >= cols");
        if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(w)) & 15)
            throw std::runtime_error("EINVAL: rmsnorm needs 16-byte aligned pointers");
        dsocr::launch_rmsnorm(x, ldx, y, ldy, rows, cols, w, eps, nullptr);
        check_hip(hipGetLastError(), "rmsnorm launch");
        check_hip(hipDeviceSynchronize(), "rmsnorm");
    });
}
static void check_relbias_args(int n_seq, int gh, int gw, int heads, int hd, const float* q, long q_ld) {
    if (!q || n_seq < 1 || gh < 1 || gw < 1 || heads < 1) throw std::runtime_error("EINVAL: bad rel-pos arguments");
    if (hd < 4 || hd % 4 || q_ld % 4 || q_ld < (long)heads * hd || (reinterpret_cast<uintptr_t>(q) & 15))
        throw std::runtime_error("EINVAL: rel-pos bias needs hd % 4 == 0 and 16-byte aligned q rows of >= heads * hd floats");
}
dsocr_status dsocr_k_sam_relbias(int n_seq, int gh, int gw, int heads, int hd, const float* q, long q_ld,
                                 const float* relh, const float* relw, float* out) {
    return guarded([&] {
        check_relbias_args(n_seq, gh, gw, heads, hd, q, q_ld);
        if (!relh || !relw || !out || ((reinterpret_cast<uintptr_t>(relh) | reinterpret_cast<uintptr_t>(relw)) & 15))
            throw std::runtime_error("EINVAL: rel-pos bias needs 16-byte aligned tables and an output");
        dsocr::launch_sam_relbias(q, q_ld, n_seq, gh, gw, heads, hd, relh, relw, out, nullptr);
        check_hip(hipGetLastError(), "sam_relbias launch");
        check_hip(hipDeviceSynchronize(), "sam_relbias");
    });
}
dsocr_status dsocr_k_attention_fused(int n_seq, int L, int heads, int hd, float scale, const float* qkv, long ld,
                                     float* o, long o_ld, const float* relh, const float* relw, int gh, int gw) {
    return guarded([&] {
        if (!qkv || !o || n_seq < 1 || L < 1 || heads < 1) throw std::runtime_error("EINVAL: bad attention arguments");
        if (hd != 32 && hd != 64 && hd != 128) throw std::runtime_error("EINVAL: head_dim must be 32, 64 or 128");
        const long C = (long)heads * hd;
        if (ld < 3 * C || o_ld < C || ld % 4 || (reinterpret_cast<uintptr_t>(qkv) & 15))
            throw std::runtime_error("EINVAL: attention needs ld >= 3 heads hd, o_ld >= heads hd and 16-byte aligned qkv rows");
        if ((relh == nullptr) != (relw == nullptr)) throw std::runtime_error("EINVAL: both rel-pos tables or neither");
        // Engine::vision_pass: q | k | v views of one buffer, the bias table from the fused buffer's q columns
        dsocr::AttnArgs a;
        a.q = {qkv, ld, hd, nullptr};
        a.k = {qkv + C, ld, hd, nullptr};
        a.v = {qkv + 2 * C, ld, hd, nullptr};
        a.o = o; a.o_row_stride = o_ld; a.o_head_stride = hd; a.n_seq = n_seq; a.L = L; a.heads = heads;
        a.kv_heads = heads; a.hd = hd; a.scale = scale;
        float* rb = nullptr;
        if (relh) {
            if ((long)gh * gw != L) throw std::runtime_error("EINVAL: rel-pos grid does not match L");
            check_relbias_args(n_seq, gh, gw, heads, hd, qkv, ld);
            if ((reinterpret_cast<uintptr_t>(relh) | reinterpret_cast<uintptr_t>(relw)) & 15)
                throw std::runtime_error("EINVAL: rel-pos bias needs 16-byte aligned tables");
            check_hip(hipMalloc(&rb, sizeof(float) * (size_t)n_seq * heads * L * (gh + gw)), "hipMalloc relbias");
            dsocr::launch_sam_relbias(qkv, ld, n_seq, gh, gw, heads, hd, relh, relw, rb, nullptr);
            a.relbias = rb; a.rel_h = gh; a.rel_w = gw;
        }
        dsocr::launch_attention(a, nullptr);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (rb) (void)hipFree(rb);
        check_hip(e, "attention_fused");
    });
}
dsocr_status dsocr_k_vision_op(int op, const long long* d, int nd, const void* const* p, int np) {
    return guarded([&] {
        auto shape = [&](int want_d, int want_p) {
            if (!d || !p || nd != want_d || np != want_p)
                throw std::runtime_error("EINVAL: vision op " + std::to_string(op) + " takes " + std::to_string(want_d) +
                                         " dims and " + std::to_string(want_p) + " pointers");
            for (int i = 0; i < np; ++i)
                if (!p[i]) throw std::runtime_error("EINVAL: vision op: NULL pointer " + std::to_string(i));
        };
        auto need = [](bool ok, const char* what) {
            if (!ok) throw std::runtime_error(std::string("EINVAL: vision op needs ") + what);
        };
        auto aligned = [&](std::initializer_list<int> idx) {
            for (int i : idx) need((reinterpret_cast<uintptr_t>(p[i]) & 15) == 0, "16-byte aligned pointers");
        };
        auto positive = [&](int n) {
            for (int i = 0; i < n; ++i) need(d[i] > 0 && d[i] <= 0x7fffffffLL, "positive 32-bit dims");
        };
        auto F = [&](int i) { return reinterpret_cast<const float*>(p[i]); };
        auto Fm = [&](int i) { return reinterpret_cast<float*>(const_cast<void*>(p[i])); };
        auto I = [&](int i) { return reinterpret_cast<const int*>(p[i]); };
        switch (op) {
        case DSOCR_VIS_PATCH_IM2COL:  // d: n, H, W, ps; p: img, cols
            shape(4, 2); positive(4);
            need(d[1] % d[3] == 0 && d[2] % d[3] == 0, "H and W divisible by the patch size");
            dsocr::launch_patch_im2col(F(0), (int)d[0], (int)d[1], (int)d[2], (int)d[3], Fm(1), nullptr);
            break;
        case DSOCR_VIS_CONV_IM2COL_NHWC:  // d: n, H, W, C, kh, kw, stride, pad; p: x, cols
            shape(8, 2); positive(7);
            need(d[7] >= 0 && d[7] < d[4] && d[7] < d[5] && d[3] % 4 == 0, "0 <= pad < kernel and C % 4 == 0");
            need(d[1] + 2 * d[7] >= d[4] && d[2] + 2 * d[7] >= d[5], "a kernel no larger than the padded image");
            aligned({0, 1});
            dsocr::launch_conv_im2col_nhwc(F(0), (int)d[0], (int)d[1], (int)d[2], (int)d[3], (int)d[4], (int)d[5], (int)d[6],
                                           (int)d[7], Fm(1), nullptr);
            break;
        case DSOCR_VIS_ADD_BROADCAST:  // d: rows_per_rep, cols, reps; p: t, x (in place)
            shape(3, 2); positive(3);
            dsocr::launch_add_broadcast(Fm(1), F(0), (long)d[0], (int)d[1], (int)d[2], nullptr);
            break;
        case DSOCR_VIS_CLIP_EMBED:  // d: n, S, C; p: sam, cls, pos, out
            shape(3, 4); positive(3);
            dsocr::launch_clip_embed(F(0), F(1), F(2), (int)d[0], (int)d[1], (int)d[2], Fm(3), nullptr);
            break;
        case DSOCR_VIS_CONCAT_CLIP_SAM:  // d: n, S, C1, C2; p: clip, sam, out
            shape(4, 3); positive(4);
            dsocr::launch_concat_clip_sam(F(0), F(1), (int)d[0], (int)d[1], (int)d[2], (int)d[3], Fm(2), nullptr);
            break;
        case DSOCR_VIS_ASSEMBLE_ROWS:  // d: rows, H, table_dt, ld_dst; p: kind, index, table, srcA, srcB, vecA, vecB, dst
            shape(4, 8); positive(2);
            need((d[2] == dsocr::WDT_BF16 || d[2] == dsocr::WDT_F16) && d[3] >= d[1], "a bf16 / f16 table and ld_dst >= H");
            dsocr::launch_assemble_rows(I(0), I(1), (int)d[0], (int)d[1], p[2], (int)d[2], F(3), F(4), F(5), F(6), Fm(7),
                                        (long)d[3], nullptr);
            break;
        case DSOCR_VIS_EMBED_TOKENS:  // d: n, H, table_dt, ld; p: table, ids, out
            shape(4, 3); positive(2);
            need((d[2] == dsocr::WDT_BF16 || d[2] == dsocr::WDT_F16) && d[3] >= d[1], "a bf16 / f16 table and ld >= H");
            dsocr::launch_embed_tokens(p[0], (int)d[2], I(1), (int)d[0], (int)d[1], Fm(2), (long)d[3], nullptr);
            break;
        case DSOCR_VIS_TRACE_LOGITS:  // d: B, V, ld, steps; p: logits, out_len, done, trace
            shape(4, 4); positive(4);
            need(d[2] >= d[1], "ld >= V");
            dsocr::launch_trace_logits(F(0), (int)d[0], (int)d[1], (long)d[2], I(1), I(2), Fm(3), (long)d[3], nullptr);
            break;
        case DSOCR_VIS_OCR2_BUILD_SEQ:  // d: n, P, D; p: feat, query, out
            shape(3, 3); positive(3);
            need(d[2] % 4 == 0, "D % 4 == 0");
            aligned({0, 1, 2});
            dsocr::launch_ocr2_build_seq(F(0), F(1), (int)d[0], (int)d[1], (int)d[2], Fm(2), nullptr);
            break;
        case DSOCR_VIS_OCR2_ROPE:  // d: rows, L, n_heads, hd, ld; p: cos, sin, x (in place)
            shape(5, 3); positive(5);
            need(d[3] % 2 == 0 && d[4] >= d[2] * d[3], "an even head dim and ld >= n_heads * hd");
            dsocr::launch_ocr2_rope(Fm(2), (long)d[4], (long)d[0], (int)d[1], (int)d[2], (int)d[3], F(0), F(1), nullptr);
            break;
        case DSOCR_VIS_OCR2_TAKE_QUERIES:  // d: n, P, D; p: src, dst
            shape(3, 2); positive(3);
            need(d[2] % 4 == 0, "D % 4 == 0");
            aligned({0, 1});
            dsocr::launch_ocr2_take_queries(F(0), (int)d[0], (int)d[1], (int)d[2], Fm(1), nullptr);
            break;
        default:
            throw std::runtime_error("EINVAL: unknown vision op " + std::to_string(op));
        }
        check_hip(hipGetLastError(), "vision_op launch");
        check_hip(hipDeviceSynchronize(), "vision_op");
    });
}
dsocr_status dsocr_window_maps(int n, int g, int W, int* tok2win, int* win2tok) {
    return guarded([&] {
        if (n < 1 || g < 1 || W < 1 || !tok2win || !win2tok) throw std::runtime_error("EINVAL: bad window map arguments");
        const long gp = g + (W - g % W) % W;
        if ((long)n * gp * gp > 0x7fffffffL) throw std::runtime_error("EINVAL: window rows exceed 32 bits");
        const dsocr::WindowMaps m = dsocr::window_maps(n, g, W);
        std::copy(m.tok2win.begin(), m.tok2win.end(), tok2win);
        std::copy(m.win2tok.begin(), m.win2tok.end(), win2tok);
    });
}
dsocr_status dsocr_k_decode_attention(int B, int heads, int kv_heads, int hd, int rope_dim, int max_len, float scale,
                                      const float* qkv, const float* cos, const float* sin, float* kc, float* vc,
                                      const int* kv_pos, float* o, int prerot) {
    return guarded([&] {
        if (hd != 32 && hd != 64 && hd != 128) throw std::runtime_error("EINVAL: head_dim must be 32, 64 or 128");
        if (prerot && rope_dim != hd) throw std::runtime_error("EINVAL: pre-rotated rows need rope_dim == head_dim");
        if (kv_heads <= 0 || heads % kv_heads || rope_dim > hd || rope_dim % 2)
            throw std::runtime_error("EINVAL: bad head / rope configuration");
        float* part = nullptr;
        int* cnt = nullptr;
        const size_t pb = dsocr::dec_attn_workspace(B, heads, hd, max_len);
        check_hip(hipMalloc(&part, pb), "hipMalloc");
        check_hip(hipMalloc(&cnt, sizeof(int) * (B * heads + 1)), "hipMalloc");
        check_hip(hipMemset(cnt, 0, sizeof(int) * (B * heads + 1)), "hipMemset");
        dsocr::dec_attn_part_init(part, pb, nullptr);
        dsocr::DecAttn2Args a;
        a.qkv = qkv; a.ld = (long)(heads + 2 * kv_heads) * hd; a.kv_pos = kv_pos; a.B = B; a.heads = heads;
        a.kv_heads = kv_heads; a.hd = hd; a.rope_dim = rope_dim; a.use_mla = 0; a.max_len = max_len;
        a.cos = cos; a.sin = sin; a.kc = kc; a.vc = vc; a.head_stride = (long)max_len * hd;
        a.page_stride = (long)kv_heads * max_len * hd; a.scale = scale; a.part = part; a.o = o;
        a.o_ld = (long)heads * hd; a.counters = cnt; a.err = cnt + B * heads;
        a.prerot = prerot != 0;
        dsocr::launch_dec_attn(a, nullptr);
        hipError_t e = hipDeviceSynchronize();
        int herr = 0;
        if (e == hipSuccess) e = hipMemcpy(&herr, a.err, sizeof(int), hipMemcpyDeviceToHost);
        (void)hipFree(part);
        (void)hipFree(cnt);
        check_hip(e, "decode attention");
        if (herr) throw std::runtime_error("EINTERNAL: decode attention merge timed out");
    });
}
// The one body of the three prefill-attention hooks below: the plan and the views of Engine::forward_rows /
// layer_forward_prefill on a cache of `cap` slots per head, into pages [page0, page0 + B) of a cache of `pages`.
// `past` is null for the plain causal prefill.  Args is AttnArgs or AttnPastArgs (the fields filled here carry the same
// names in both); run(a, rope, dev) sets what is its own (lengths, workspace), checks the kernel's contract, then
// rotates, appends and launches.
extern "C++" {  // (a template cannot have C linkage)
struct DevBufs {  // device buffers freed on return or throw
    std::vector<void*> bufs;
    ~DevBufs() { for (void* p : bufs) (void)hipFree(p); }
    void* alloc(size_t b) {
        void* p = nullptr;
        check_hip(hipMalloc(&p, b ? b : 16), "hipMalloc");
        bufs.push_back(p);
        return p;
    }
    void* upload(const void* src, size_t b) {
        void* p = alloc(b);
        check_hip(hipMemcpy(p, src, b, hipMemcpyHostToDevice), "h2d");
        return p;
    }
    // a workspace no launch has written: NaN wherever a combine reads past its own records
    float* workspace(size_t floats) {
        float* p = (float*)alloc(sizeof(float) * floats);
        check_hip(hipMemset(p, 0xFF, sizeof(float) * floats), "hipMemset");
        return p;
    }
};
struct PrefillCase {
    const dsocr::PrefillPlan& plan;
    const int* lens;  // device copies
    const int* past;  // (null without a past)
    DevBufs& dev;
};
template <class Args, class Run>
static void prefill_attention_case(int B, int heads, int kv_heads, int hd, int rope_dim, int use_mla, int cap, float scale,
                                   bool behind_past, const int* past, const int* lens, float* qkv, const float* cos,
                                   const float* sin, float* kc, float* vc, float* o, int page0, int pages, Run run) {
    if (heads <= 0 || kv_heads <= 0 || heads % kv_heads || rope_dim < 0 || rope_dim > hd || rope_dim % 2)
        throw std::runtime_error("EINVAL: bad head / rope configuration");
    if (B <= 0 || (behind_past && !past) || !lens || !qkv || !cos || !sin || !kc || !vc || !o)
        throw std::runtime_error("EINVAL: NULL argument");
    if (page0 < 0 || pages < 1 || (long)page0 + B > pages) throw std::runtime_error("EINVAL: pages [page0, page0 + B) must lie in the cache");
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 1)
            throw std::runtime_error(behind_past ? "EINVAL: every sequence needs at least one new row"
                                                 : "EINVAL: every sequence needs at least one row");
        if (behind_past && (past[b] < 0 || (long)past[b] + lens[b] > cap))
            throw std::runtime_error("EINVAL: past + new rows must fit in cap");
    }
    const long QKVN = (long)(heads + 2 * kv_heads) * hd, H = (long)heads * hd;
    const long head_stride = (long)cap * hd, page_stride = (long)kv_heads * head_stride;
    const std::vector<int> hl(lens, lens + B), hp(behind_past ? past : nullptr, behind_past ? past + B : nullptr);
    const dsocr::PrefillPlan plan = dsocr::prefill_row_plan(hl, QKVN, H, page_stride, hp);
    if (!behind_past && cap < plan.max_len) throw std::runtime_error("EINVAL: cap is below the longest sequence");
    float* kc0 = kc + (long)page0 * page_stride;
    float* vc0 = vc + (long)page0 * page_stride;
    DevBufs dev;
    dsocr::RopeKvArgs r;
    r.qkv = qkv; r.ld = QKVN; r.rows = (int)plan.T;
    r.row_page = (const int*)dev.upload(plan.row_page.data(), sizeof(int) * plan.row_page.size());
    r.row_pos = (const int*)dev.upload(plan.row_pos.data(), sizeof(int) * plan.row_pos.size());
    r.heads = heads; r.kv_heads = kv_heads; r.hd = hd; r.rope_dim = rope_dim; r.use_mla = use_mla ? 1 : 0;
    r.cos = cos; r.sin = sin; r.kc = kc0; r.vc = vc0; r.page_stride = page_stride; r.head_stride = head_stride;
    Args a;
    a.q = {qkv, QKVN, hd, (const long*)dev.upload(plan.q_off.data(), sizeof(long) * B)};
    const long* kv_off = (const long*)dev.upload(plan.kv_off.data(), sizeof(long) * B);
    a.k = {kc0, hd, head_stride, kv_off};
    a.v = {vc0, hd, head_stride, kv_off};
    a.o = o; a.o_row_stride = H; a.o_head_stride = hd;
    a.o_seq_off = (const long*)dev.upload(plan.o_off.data(), sizeof(long) * B);
    a.n_seq = B; a.heads = heads; a.kv_heads = kv_heads; a.hd = hd; a.scale = scale;
    const PrefillCase c{plan, (const int*)dev.upload(lens, sizeof(int) * B),
                        behind_past ? (const int*)dev.upload(past, sizeof(int) * B) : nullptr, dev};
    run(a, r, c);
}
// AttnPastArgs: the per-sequence lengths and the host-side bounds of the plan
static void set_past_lengths(dsocr::AttnPastArgs& a, const PrefillCase& c) {
    a.past = c.past; a.n_q = c.lens; a.max_q = c.plan.max_len; a.max_total = c.plan.max_total;
}
static void require_head_dim(int hd) {
    if (hd != 32 && hd != 64 && hd != 128) throw std::runtime_error("EINVAL: head_dim must be 32, 64 or 128");
}
}  // extern "C++"
dsocr_status dsocr_k_prefill_attention(int B, int heads, int kv_heads, int hd, int rope_dim, int use_mla, int cap,
                                       float scale, const int* lens, float* qkv, const float* cos, const float* sin,
                                       float* kc, float* vc, float* o, int use_part) {
    return guarded([&] {
        require_head_dim(hd);
        prefill_attention_case<dsocr::AttnArgs>(
            B, heads, kv_heads, hd, rope_dim, use_mla, cap, scale, false, nullptr, lens, qkv, cos, sin, kc, vc, o, 0,
            B > 0 ? B : 1, [&](dsocr::AttnArgs& a, const dsocr::RopeKvArgs& r, const PrefillCase& c) {
                a.L = c.plan.max_len; a.seq_len = c.lens; a.causal = 1;
                if (use_part) {
                    a.part_floats = dsocr::attention_causal_part_floats(B, heads, c.plan.max_len, hd);
                    a.part = c.dev.workspace(a.part_floats);
                }
                dsocr::launch_rope_kv(r, nullptr);
                dsocr::launch_attention(a, nullptr);
                check_hip(hipGetLastError(), "prefill attention launch");
                check_hip(hipDeviceSynchronize(), "prefill attention");
            });
    });
}
dsocr_status dsocr_k_prefill_attention_past(int B, int heads, int kv_heads, int hd, int rope_dim, int use_mla, int cap,
                                            float scale, const int* past, const int* lens, float* qkv, const float* cos,
                                            const float* sin, float* kc, float* vc, float* o) {
    return guarded([&] {
        require_head_dim(hd);
        prefill_attention_case<dsocr::AttnPastArgs>(
            B, heads, kv_heads, hd, rope_dim, use_mla, cap, scale, true, past, lens, qkv, cos, sin, kc, vc, o, 0,
            B > 0 ? B : 1, [&](dsocr::AttnPastArgs& a, const dsocr::RopeKvArgs& r, const PrefillCase& c) {
                set_past_lengths(a, c);
                a.part_floats = dsocr::attention_past_part_floats(B, heads, c.plan.max_len, c.plan.max_total, hd);
                a.part = c.dev.workspace(a.part_floats);
                // refused before anything is rotated or appended
                if (!dsocr::attention_past_ok(a)) throw std::runtime_error("EINVAL: attention_past: shape outside the kernel's contract");
                dsocr::launch_rope_kv(r, nullptr);
                dsocr::launch_attention_past(a, nullptr);
                check_hip(hipGetLastError(), "prefill attention (past) launch");
                check_hip(hipDeviceSynchronize(), "prefill attention (past)");
            });
    });
}
dsocr_status dsocr_k_attention_chunk(int B, int heads, int kv_heads, int hd, int rope_dim, int use_mla, int cap,
                                     float scale, const int* past, const int* lens, float* qkv, const float* cos,
                                     const float* sin, float* kc, float* vc, float* o, int page0, int pages) {
    return guarded([&] {
        prefill_attention_case<dsocr::AttnPastArgs>(
            B, heads, kv_heads, hd, rope_dim, use_mla, cap, scale, true, past, lens, qkv, cos, sin, kc, vc, o, page0,
            pages, [&](dsocr::AttnPastArgs& a, const dsocr::RopeKvArgs& r, const PrefillCase& c) {
                set_past_lengths(a, c);
                // refused before anything is rotated or appended
                if (!dsocr::attention_chunk_ok(a)) throw std::runtime_error("EINVAL: attention_chunk: shape outside the kernel's contract");
                dsocr::launch_rope_kv(r, nullptr);
                dsocr::launch_attention_chunk(a, nullptr);
                check_hip(hipGetLastError(), "attention_chunk launch");
                check_hip(hipDeviceSynchronize(), "attention_chunk");
            });
    });
}
dsocr_status dsocr_k_qkv_attention(int fused, int steps, int H, int heads, int hd, int max_len, float scale,
                                   float eps, const float* x, const float* norm_w, const void* Wqkv, int wdtype,
                                   const float* cos, const float* sin, float* kc, float* vc, const int* kv_pos,
                                   float* qkv_row, float* o, int* used_fused) {
    return guarded([&] {
        if (steps <= 0 || H <= 0 || heads <= 0 || hd != 128 || heads * hd != H)
            throw std::runtime_error("EINVAL: qkv_attention needs 128-dim MHA heads with heads * hd == H");
        if (wdtype != dsocr::WDT_F16 && wdtype != dsocr::WDT_BF16) throw std::runtime_error("EINVAL: 16-bit weights only");
        const int QKVN = 3 * H;
        {  // range check once, before anything is allocated (it does not depend on the step)
            dsocr::DecGemvArgs g;
            g.M = 1; g.N = QKVN; g.K = H; g.W = Wqkv; g.ldw = H; g.wdtype = wdtype; g.y = qkv_row; g.ldy = QKVN;
            g.x = x; g.ldx = H; g.norm_w = norm_w; g.eps = eps;
            dsocr::DecRopeEpi re;
            re.kv_pos = kv_pos; re.cos = cos; re.sin = sin; re.hd = hd; re.rot_rows = 2 * H;
            if (!dsocr::dec_qkv_rope_ok(g, re)) throw std::runtime_error("EINVAL: q/k/v projection outside dec_qkv_rope's range");
        }
        float* part = nullptr;
        int* cnt = nullptr;
        const size_t pb = dsocr::dec_attn_workspace(1, heads, hd, max_len);
        check_hip(hipMalloc(&part, pb), "hipMalloc");
        check_hip(hipMalloc(&cnt, sizeof(int) * (heads + 1)), "hipMalloc");
        check_hip(hipMemset(cnt, 0, sizeof(int) * (heads + 1)), "hipMemset");
        dsocr::dec_attn_part_init(part, pb, nullptr);
        bool took = false;
        for (int s = 0; s < steps; ++s) {
            dsocr::DecGemvArgs g;
            g.M = 1; g.N = QKVN; g.K = H; g.W = Wqkv; g.ldw = H; g.wdtype = wdtype; g.y = qkv_row; g.ldy = QKVN;
            g.x = x + (size_t)s * H; g.ldx = H; g.norm_w = norm_w; g.eps = eps;
            dsocr::DecRopeEpi re;
            re.kv_pos = kv_pos + s; re.cos = cos; re.sin = sin; re.hd = hd; re.rot_rows = 2 * H;
            dsocr::DecAttn2Args a;
            a.qkv = qkv_row; a.ld = QKVN; a.kv_pos = kv_pos + s; a.B = 1; a.heads = heads; a.kv_heads = heads;
            a.hd = hd; a.rope_dim = hd; a.use_mla = 0; a.max_len = max_len; a.cos = cos; a.sin = sin;
            a.kc = kc; a.vc = vc; a.head_stride = (long)max_len * hd; a.page_stride = (long)heads * max_len * hd;
            a.scale = scale; a.part = part; a.o = o + (size_t)s * H; a.o_ld = H; a.counters = cnt; a.err = cnt + heads;
            a.prerot = 1;
            if (fused && dsocr::dec_qkv_attn_ok(g, re, a)) {
                dsocr::launch_dec_qkv_attn(g, re, a, nullptr);
                took = true;
            } else {
                dsocr::launch_dec_qkv_rope(g, re, nullptr);
                dsocr::launch_dec_attn(a, nullptr);
            }
        }
        hipError_t e = hipDeviceSynchronize();
        int herr = 0;
        if (e == hipSuccess) e = hipMemcpy(&herr, cnt + heads, sizeof(int), hipMemcpyDeviceToHost);
        (void)hipFree(part);
        (void)hipFree(cnt);
        check_hip(e, "qkv_attention");
        if (herr) throw std::runtime_error("EINTERNAL: q/k/v hand-off or attention merge timed out");
        if (used_fused) *used_fused = took ? 1 : 0;
    });
}
dsocr_status dsocr_k_qkv_attention_layers(int defer, int layers, int H, int heads, int hd, int max_len, float scale,
                                          float eps, const float* x, const float* norm_w, const void* Wqkv, int wdtype,
                                          const float* cos, const float* sin, float* kc, float* vc, const int* kv_pos,
                                          float* o, uint32_t* qkv_copies, uint32_t* part_copies, int* err_word) {
    return guarded([&] {
        if (layers <= 0 || H <= 0 || heads <= 0 || hd != 128 || heads * hd != H || max_len <= 0)
            throw std::runtime_error("EINVAL: qkv_attention_layers needs 128-dim MHA heads with heads * hd == H");
        if (wdtype != dsocr::WDT_F16 && wdtype != dsocr::WDT_BF16) throw std::runtime_error("EINVAL: 16-bit weights only");
        if (!x || !norm_w || !Wqkv || !cos || !sin || !kc || !vc || !kv_pos || !o || !qkv_copies || !part_copies || !err_word)
            throw std::runtime_error("EINVAL: NULL argument");
        const int QKVN = 3 * H;
        const size_t pb = dsocr::dec_attn_workspace(1, heads, hd, max_len), pw = pb / 4;
        const size_t cache = (size_t)heads * max_len * hd;
        float* row[2] = {nullptr, nullptr};
        float* part[2] = {nullptr, nullptr};
        int* cnt = nullptr;
        auto release = [&] {
            for (int c = 0; c < 2; ++c) { (void)hipFree(row[c]); (void)hipFree(part[c]); }
            (void)hipFree(cnt);
        };
        try {
            for (int c = 0; c < 2; ++c) {
                check_hip(hipMalloc(&row[c], sizeof(float) * QKVN), "hipMalloc");
                check_hip(hipMalloc(&part[c], pb), "hipMalloc");
                dsocr::dec_qkv_sentinel_init(row[c], QKVN, nullptr);
                dsocr::dec_attn_part_init(part[c], pb, nullptr);
            }
            check_hip(hipMalloc(&cnt, sizeof(int) * (heads + 1)), "hipMalloc");
            check_hip(hipMemset(cnt, 0, sizeof(int) * (heads + 1)), "hipMemset");
            // the engine's plan (Engine::decode_step): deferred - layer l on copy l & 1, every layer but the last
            // leaves its refill to the next, layer l >= 1 cleans copy (l - 1) & 1; else copy 0, refilled in-launch
            for (int l = 0; l < layers; ++l) {
                const int c = defer ? l & 1 : 0;
                dsocr::DecGemvArgs g;
                g.M = 1; g.N = QKVN; g.K = H; g.W = (const uint16_t*)Wqkv + (size_t)l * QKVN * H; g.ldw = H; g.wdtype = wdtype;
                g.y = row[c]; g.ldy = QKVN; g.x = x + (size_t)l * H; g.ldx = H; g.norm_w = norm_w; g.eps = eps;
                dsocr::DecRopeEpi re;
                re.kv_pos = kv_pos + l; re.cos = cos; re.sin = sin; re.hd = hd; re.rot_rows = 2 * H;
                dsocr::DecAttn2Args a;
                a.qkv = row[c]; a.ld = QKVN; a.kv_pos = kv_pos + l; a.B = 1; a.heads = heads; a.kv_heads = heads;
                a.hd = hd; a.rope_dim = hd; a.use_mla = 0; a.max_len = max_len; a.cos = cos; a.sin = sin;
                a.kc = kc + (size_t)l * cache; a.vc = vc + (size_t)l * cache; a.head_stride = (long)max_len * hd;
                a.page_stride = (long)heads * max_len * hd; a.scale = scale; a.part = part[c];
                a.o = o + (size_t)l * H; a.o_ld = H; a.counters = cnt; a.err = cnt + heads; a.prerot = 1;
                if (defer) {
                    a.no_refill = l + 1 < layers;
                    if (l >= 1) { a.clean_qkv = row[c ^ 1]; a.clean_part = part[c ^ 1]; }
                }
                if (!dsocr::dec_qkv_attn_ok(g, re, a)) throw std::runtime_error("EINVAL: outside dec_qkv_attn's range");
                dsocr::launch_dec_qkv_attn(g, re, a, nullptr);
            }
            check_hip(hipDeviceSynchronize(), "qkv_attention_layers");
            check_hip(hipMemcpy(err_word, cnt + heads, sizeof(int), hipMemcpyDeviceToHost), "d2h");
            for (int c = 0; c < 2; ++c) {
                check_hip(hipMemcpy(qkv_copies + (size_t)c * QKVN, row[c], sizeof(float) * QKVN, hipMemcpyDeviceToHost), "d2h");
                check_hip(hipMemcpy(part_copies + (size_t)c * pw, part[c], pb, hipMemcpyDeviceToHost), "d2h");
            }
        } catch (...) {
            release();
            throw;
        }
        release();
    });
}
int dsocr_k_poll_wait_fits(long waiting_blocks, int api_blocks_per_cu, int cus) {
    return dsocr::poll_wait_fits(waiting_blocks, api_blocks_per_cu, cus) ? 1 : 0;
}
dsocr_status dsocr_k_moe(int T, int H, int E, int topk, int I, int Is, const float* x, const float* norm_w,
                         float eps, const void* router, const void* Wgu, const void* Wd, const void* sWgu,
                         const void* sWd, int wdtype, int norm_topk, float scaling, float* out, int* ids_out,
                         float* w_out) {
    return dsocr_k_moe_ex(T, H, E, topk, I, Is, x, norm_w, eps, router, Wgu, Wd, sWgu, sWd, wdtype, norm_topk, scaling,
                          out, ids_out, w_out, 1, nullptr, nullptr);
}
dsocr_status dsocr_k_moe_ex(int T, int H, int E, int topk, int I, int Is, const float* x, const float* norm_w,
                            float eps, const void* router, const void* Wgu, const void* Wd, const void* sWgu,
                            const void* sWd, int wdtype, int norm_topk, float scaling, float* out, int* ids_out,
                            float* w_out, int softmax_scoring, const float* router_bias, float* logits_out) {
    return guarded([&] {
        if (T <= 0 || H <= 0 || E <= 0 || topk <= 0 || I <= 0) throw std::runtime_error("EINVAL: bad MoE shape");
        if (E > 256 || topk > 8 || topk > E) throw std::runtime_error("EINVAL: decode MoE takes <= 256 experts, top_k <= min(8, E)");
        if (!x || !router || !Wgu || !Wd || !out) throw std::runtime_error("EINVAL: NULL argument");
        std::vector<void*> bufs;
        auto alloc = [&](size_t b) {
            void* p = nullptr;
            check_hip(hipMalloc(&p, b ? b : 16), "hipMalloc");
            bufs.push_back(p);
            return p;
        };
        try {
            const int TK = T * topk;
            // the engine's own dispatch (Engine::decode_step -> launch_moe_decode): mix kernels at one
            // token, slot kernels at two, the grouped (expert-deduplicated) kernels at 3..8, sorted groups above
            dsocr::MoeDecodeArgs a;
            a.T = T; a.H = H; a.E = E; a.topk = topk; a.I = I;
            a.x = x; a.norm_w = norm_w; a.eps = eps; a.out = out;
            a.router = router; a.router_wdt = wdtype; a.Wgu = Wgu; a.Wd = Wd; a.wdtype = wdtype;
            a.router_bias = router_bias;
            if (sWgu && sWd && Is > 0) {
                a.Is = Is; a.sWgu = sWgu; a.sWd = sWd; a.hs = (float*)alloc(sizeof(float) * (size_t)T * Is);
            }
            a.softmax_scoring = softmax_scoring ? 1 : 0; a.norm_topk = norm_topk; a.scaling = scaling;
            a.xn = (float*)alloc(sizeof(float) * (size_t)T * H);
            a.xn_router = (float*)alloc(sizeof(float) * (size_t)T * H);
            a.logits = (float*)alloc(sizeof(float) * (size_t)T * E);
            a.ids = (int*)alloc(sizeof(int) * TK);
            a.wts = (float*)alloc(sizeof(float) * TK);
            a.h = (float*)alloc(sizeof(float) * (size_t)TK * I);
            a.grp = (int*)alloc(sizeof(int) * dsocr::moe_grp_ints(E, T, topk));
            a.route_cnt = (int*)alloc(sizeof(int) * 16);
            check_hip(hipMemset(a.route_cnt, 0, sizeof(int) * 16), "hipMemset");
            if (wdtype == 1 && H % 32 == 0 && I % 32 == 0 && T <= 8) {
                // fragment-ordered expert copies, as Engine::ensure_mm_weights keeps them
                a.Wgu_swz = alloc(sizeof(uint16_t) * dsocr::mm_swizzle_elems(E * 2 * I, H));
                dsocr::launch_mm_swizzle(Wgu, E * 2 * I, H, const_cast<void*>(a.Wgu_swz), nullptr);
                a.Wd_swz = alloc(sizeof(uint16_t) * dsocr::mm_swizzle_elems(E * H, I));
                dsocr::launch_mm_swizzle(Wd, E * H, I, const_cast<void*>(a.Wd_swz), nullptr);
                if (a.Is > 0 && a.Is % 32 == 0) {
                    a.sWgu_swz = alloc(sizeof(uint16_t) * dsocr::mm_swizzle_elems(2 * a.Is, H));
                    dsocr::launch_mm_swizzle(sWgu, 2 * a.Is, H, const_cast<void*>(a.sWgu_swz), nullptr);
                    a.sWd_swz = alloc(sizeof(uint16_t) * dsocr::mm_swizzle_elems(H, a.Is));
                    dsocr::launch_mm_swizzle(sWd, H, a.Is, const_cast<void*>(a.sWd_swz), nullptr);
                }
            }
            if (T >= 3 && T <= 8) {
                a.dn_part = (float*)alloc(sizeof(float) * dsocr::moe_down_mm_part_floats(E, T, topk, I, a.Is, H));
                a.dn_tick = (int*)alloc(sizeof(int) * (H / 64 + 1));
                check_hip(hipMemset(a.dn_tick, 0, sizeof(int) * (H / 64 + 1)), "hipMemset");
            }
            if (T > 8) {
                a.eoff = (int*)alloc(sizeof(int) * (E + 1)); a.arow = (int*)alloc(sizeof(int) * TK);
                a.apos = (int*)alloc(sizeof(int) * TK); a.active = (int*)alloc(sizeof(int) * E);
                a.aw = (float*)alloc(sizeof(float) * TK); a.n_active = (int*)alloc(sizeof(int));
            }
            dsocr::launch_moe_decode(a, nullptr);
            check_hip(hipGetLastError(), "moe launch");
            check_hip(hipDeviceSynchronize(), "moe");
            if (ids_out) check_hip(hipMemcpy(ids_out, a.ids, sizeof(int) * TK, hipMemcpyDeviceToHost), "d2h");
            if (w_out) check_hip(hipMemcpy(w_out, a.wts, sizeof(float) * TK, hipMemcpyDeviceToHost), "d2h");
            if (logits_out)
                check_hip(hipMemcpy(logits_out, a.logits, sizeof(float) * (size_t)T * E, hipMemcpyDeviceToHost), "d2h");
        } catch (...) {
            for (void* p : bufs) (void)hipFree(p);
            throw;
        }
        for (void* p : bufs) (void)hipFree(p);
    });
}
dsocr_status dsocr_k_moe_prefill_route(int T, int E, int topk, const float* logits, int softmax_scoring, int norm_topk,
                                       float scaling, int* ids, float* w, int* eoff, int* arow, int* apos) {
    return guarded([&] {
        if (T <= 0 || E <= 0 || topk <= 0) throw std::runtime_error("EINVAL: bad routing shape");
        if (E > 256 || topk > 8 || topk > E) throw std::runtime_error("EINVAL: routing takes <= 256 experts, top_k <= min(8, E)");
        if (!logits || !ids || !w || !eoff || !arow || !apos) throw std::runtime_error("EINVAL: NULL argument");
        // the prefill's two launches (Engine::layer_forward_prefill)
        dsocr::launch_router_topk(logits, T, E, topk, softmax_scoring ? 1 : 0, norm_topk, scaling, ids, w, nullptr);
        dsocr::launch_moe_group(ids, T, topk, E, eoff, arow, apos, nullptr, nullptr);
        check_hip(hipGetLastError(), "prefill route launch");
        check_hip(hipDeviceSynchronize(), "prefill route");
    });
}
dsocr_status dsocr_k_moe_combine(int T, int topk, int H, const float* y, const int* apos, const float* w,
                                 const float* shared, float* out, int accumulate) {
    return guarded([&] {
        if (T <= 0 || H <= 0 || topk <= 0 || topk > 8) throw std::runtime_error("EINVAL: bad combine shape");
        if (!y || !apos || !w || !out) throw std::runtime_error("EINVAL: NULL argument");
        dsocr::launch_moe_combine(y, apos, w, shared, T, topk, H, out, accumulate ? 1 : 0, nullptr);
        check_hip(hipGetLastError(), "combine launch");
        check_hip(hipDeviceSynchronize(), "combine");
    });
}
dsocr_status dsocr_k_moe_packed(int T, int H, int E, int topk, int I, int Is, const float* x, const float* norm_w,
                                float eps, const void* router_f16, int gu_qtype, const void* Wgu_payload, int d_qtype,
                                const void* Wd_payload, int sgu_qtype, const void* sWgu_payload, int sd_qtype,
                                const void* sWd_payload, int norm_topk, float scaling, float* out, int* ids_out,
                                float* w_out) {
    return guarded([&] {
        if (T <= 0 || T > 8 || H <= 0 || E <= 0 || topk <= 0 || I <= 0 || Is < 0) throw std::runtime_error("EINVAL: bad MoE shape");
        if (!x || !router_f16 || !Wgu_payload || !Wd_payload || !out) throw std::runtime_error("EINVAL: NULL argument");
        const bool shared = sWgu_payload && sWd_payload && Is > 0;
        if (!dsocr::dsq_packed_ok(gu_qtype, H) || !dsocr::dsq_packed_ok(d_qtype, I) ||
            (shared && (!dsocr::dsq_packed_ok(sgu_qtype, H) || !dsocr::dsq_packed_ok(sd_qtype, Is))))
            throw std::runtime_error("EINVAL: packed experts take Q4_K (in_dim % 256 == 0) or Q8_0 (in_dim % 32 == 0) records");
        std::vector<void*> bufs;
        auto alloc = [&](size_t b) {
            void* p = nullptr;
            check_hip(hipMalloc(&p, b ? b : 16), "hipMalloc");
            bufs.push_back(p);
            return p;
        };
        try {
            const int TK = T * topk;
            auto pack = [&](int qt, const void* payload, long rows, long in_dim) {
                void* buf = alloc(dsocr::dsq_packed_bytes(qt, rows, in_dim));
                dsocr::QMat m = dsocr::dsq_packed_view(qt, buf, rows, in_dim);
                dsocr::launch_dsq_repack(m, 0, payload, rows, in_dim, nullptr);
                return m;
            };
            dsocr::MoeDecodeArgs a;
            a.T = T; a.H = H; a.E = E; a.topk = topk; a.I = I;
            a.x = x; a.norm_w = norm_w; a.eps = eps; a.out = out;
            a.router = router_f16; a.router_wdt = dsocr::WDT_F16; a.wdtype = dsocr::WDT_F16;
            a.qWgu = pack(gu_qtype, Wgu_payload, (long)E * 2 * I, H);
            a.qWd = pack(d_qtype, Wd_payload, (long)E * H, I);
            if (shared) {
                a.Is = Is;
                a.qsWgu = pack(sgu_qtype, sWgu_payload, 2L * Is, H);
                a.qsWd = pack(sd_qtype, sWd_payload, H, Is);
                a.hs = (float*)alloc(sizeof(float) * (size_t)T * Is);
            }
            a.softmax_scoring = 1; a.norm_topk = norm_topk; a.scaling = scaling;
            a.xn = (float*)alloc(sizeof(float) * (size_t)T * H);
            a.xn_router = (float*)alloc(sizeof(float) * (size_t)T * H);
            a.logits = (float*)alloc(sizeof(float) * (size_t)T * E);
            a.ids = (int*)alloc(sizeof(int) * TK);
            a.wts = (float*)alloc(sizeof(float) * TK);
            a.h = (float*)alloc(sizeof(float) * (size_t)TK * I);
            a.grp = (int*)alloc(sizeof(int) * dsocr::moe_grp_ints(E, T, topk));
            a.route_cnt = (int*)alloc(sizeof(int) * 16);
            check_hip(hipMemset(a.route_cnt, 0, sizeof(int) * 16), "hipMemset");
            const char* gu = nullptr;
            dsocr::moe_decode_kernel_names(a, &gu, nullptr);
            if (std::string(gu) != "moe_gateup_q_kernel") throw std::runtime_error("EINVAL: packed decode MoE outside its range");
            dsocr::launch_moe_decode(a, nullptr);
            check_hip(hipGetLastError(), "moe launch");
            check_hip(hipDeviceSynchronize(), "moe");
            if (ids_out) check_hip(hipMemcpy(ids_out, a.ids, sizeof(int) * TK, hipMemcpyDeviceToHost), "d2h");
            if (w_out) check_hip(hipMemcpy(w_out, a.wts, sizeof(float) * TK, hipMemcpyDeviceToHost), "d2h");
        } catch (...) {
            for (void* p : bufs) (void)hipFree(p);
            throw;
        }
        for (void* p : bufs) (void)hipFree(p);
    });
}
dsocr_status dsocr_k_dsq_rows_dot(int qtype, size_t rows, size_t in_dim, const void* payload, int T, const float* x,
                                  float* y) {
    return guarded([&] {
        if (!dsocr::dsq_packed_ok(qtype, (long)in_dim) || rows == 0)
            throw std::runtime_error("EINVAL: rows_dot takes Q4_K (in_dim % 256 == 0) or Q8_0 (in_dim % 32 == 0) rows");
        if (T < 1 || T > 8 || !payload || !x || !y) throw std::runtime_error("EINVAL: rows_dot takes 1..8 token rows");
        void* buf = nullptr;
        check_hip(hipMalloc(&buf, dsocr::dsq_packed_bytes(qtype, (long)rows, (long)in_dim)), "hipMalloc");
        try {
            const dsocr::QMat m = dsocr::dsq_packed_view(qtype, buf, (long)rows, (long)in_dim);
            dsocr::launch_dsq_repack(m, 0, payload, (long)rows, (long)in_dim, nullptr);
            dsocr::launch_dsq_rows_dot(m, (long)rows, (long)in_dim, T, x, y, nullptr);
            check_hip(hipGetLastError(), "rows_dot launch");
            check_hip(hipDeviceSynchronize(), "rows_dot");
        } catch (...) {
            (void)hipFree(buf);
            throw;
        }
        (void)hipFree(buf);
    });
}
dsocr_status dsocr_k_moe_kernels(int T, int H, int E, int topk, int I, int Is, int has_norm, const char** gateup,
                                 const char** down) {
    return guarded([&] {
        dsocr::MoeDecodeArgs a;
        a.T = T; a.H = H; a.E = E; a.topk = topk; a.I = I; a.Is = Is;
        int dummy = 0;
        float fd = 0.f;
        a.x = &fd; a.out = &fd; a.norm_w = has_norm ? &fd : nullptr;
        if (Is > 0) { a.sWgu = &dummy; a.sWd = &dummy; a.hs = &fd; }
        a.xn = a.xn_router = a.logits = a.wts = a.h = &fd;
        a.ids = a.grp = a.route_cnt = &dummy;
        if (T >= 3 && T <= 8) { a.dn_part = &fd; a.dn_tick = &dummy; }
        // the engine keeps fragment-ordered expert copies (Engine::ensure_mm_weights)
        a.Wgu_swz = a.Wd_swz = &dummy;
        if (Is > 0) a.sWgu_swz = a.sWd_swz = &dummy;
        if (T > 8) { a.eoff = a.arow = a.apos = a.active = a.n_active = &dummy; a.aw = &fd; }
        dsocr::moe_decode_kernel_names(a, gateup, down);
    });
}
dsocr_status dsocr_k_moe_route_kind(int T, int H, int E, int topk, int I, int Is, int has_norm, const char** kind) {
    return guarded([&] {
        if (!kind) throw std::runtime_error("EINVAL: NULL argument");
        // the arguments dsocr_k_moe_ex builds for f16 weights (which workspaces and fragment-ordered copies exist)
        dsocr::MoeDecodeArgs a;
        a.T = T; a.H = H; a.E = E; a.topk = topk; a.I = I;
        int dummy = 0;
        float fd = 0.f;
        a.x = &fd; a.out = &fd; a.norm_w = has_norm ? &fd : nullptr;
        a.router = a.Wgu = a.Wd = &dummy;
        if (Is > 0) { a.Is = Is; a.sWgu = &dummy; a.sWd = &dummy; a.hs = &fd; }
        a.xn = a.xn_router = a.logits = a.wts = a.h = &fd;
        a.ids = a.grp = a.route_cnt = &dummy;
        if (H % 32 == 0 && I % 32 == 0 && T <= 8) {
            a.Wgu_swz = a.Wd_swz = &dummy;
            if (Is > 0 && Is % 32 == 0) a.sWgu_swz = a.sWd_swz = &dummy;
        }
        if (T >= 3 && T <= 8) { a.dn_part = &fd; a.dn_tick = &dummy; }
        if (T > 8) { a.eoff = a.arow = a.apos = a.active = a.n_active = &dummy; a.aw = &fd; }
        *kind = dsocr::moe_decode_route_kind(a);
    });
}
dsocr_status dsocr_k_lmhead_screened(int B, int V, int K, const float* x, const float* norm_w, float eps,
                                     const void* W, const int* ban, int ban_ld, int* out_tok) {
    return guarded([&] {
        if (B <= 0 || V <= 0 || K % 16 || K > 1536 || !x || !norm_w || !W || !out_tok)
            throw std::runtime_error("EINVAL: screened lm_head needs B, V > 0, K % 16 == 0, K <= 1536, x / norm / W / out");
        if (ban && ban_ld < 2) throw std::runtime_error("EINVAL: ban list stride < 2");
        std::vector<void*> bufs;
        auto alloc = [&](size_t b) {
            void* p = nullptr;
            check_hip(hipMalloc(&p, b ? b : 16), "hipMalloc");
            bufs.push_back(p);
            return p;
        };
        try {
            // the engine's load-time quantisation and its per-step launches (Engine::decode_head)
            // (B = 3..8: the one-stream matrix-core form, as the engine runs it at 3..8 pages)
            const bool mm = B >= 3 && dsocr::lmhead_q8mm_ok(B, V, K);
            if (B > 2 && !mm) throw std::runtime_error("EINVAL: screened lm_head for 3..8 rows needs K in {768, 1024, 1280, 1536}");
            const size_t vp = (size_t)(V + 15) / 16 * 16;
            void* q = alloc((size_t)V * K);
            float* scale = (float*)alloc(sizeof(float) * vp);
            float* bound = (float*)alloc(sizeof(float) * vp);
            float* qnorm = mm ? (float*)alloc(sizeof(float) * vp) : nullptr;
            void* qfrag = mm ? alloc(dsocr::lmhead_qfrag_bytes(V, K)) : nullptr;
            check_hip(hipMemset(scale, 0, sizeof(float) * vp), "hipMemset");
            check_hip(hipMemset(bound, 0, sizeof(float) * vp), "hipMemset");
            if (qnorm) check_hip(hipMemset(qnorm, 0, sizeof(float) * vp), "hipMemset");
            dsocr::launch_lmhead_quantize(W, V, K, q, scale, bound, nullptr, qnorm, qfrag);
            dsocr::LmHeadQ8Args a;
            a.x = x; a.ldx = K; a.norm_w = norm_w; a.eps = eps; a.q = q; a.scale = scale; a.bound = bound;
            a.B = B; a.N = V; a.K = K; a.ban = ban; a.ban_ld = ban ? ban_ld : 0;
            a.qfrag = qfrag; a.qnorm = qnorm;
            if (mm) dsocr::lmhead_q8mm_grid(V, K, B, &a.nblk, &a.slot);
            else dsocr::lmhead_q8_grid(V, K, B, &a.nblk, &a.slot);
            a.blk_cnt = (int*)alloc(sizeof(int) * B * a.nblk);
            a.blk_t = (float*)alloc(sizeof(float) * B * a.nblk);
            a.cand = (int*)alloc(sizeof(int) * B * a.nblk * a.slot);
            a.cand_hi = (float*)alloc(sizeof(float) * B * a.nblk * a.slot);
            a.xn_out = (float*)alloc(sizeof(float) * B * K);
            dsocr::launch_lmhead_q8(a, nullptr);
            dsocr::DecSampleArgs ss;  // selection only: empty contexts, no bookkeeping
            ss.B = B; ss.V = V; ss.ld = V; ss.ctx = (int*)alloc(sizeof(int) * 64); ss.ctx_cap = 64;
            ss.ctx_len = (int*)alloc(sizeof(int) * B); ss.ngram = 0; ss.out_tok = out_tok;
            check_hip(hipMemset(ss.ctx_len, 0, sizeof(int) * B), "hipMemset");
            ss.blk_cnt = a.blk_cnt; ss.blk_t = a.blk_t; ss.cand = a.cand; ss.cand_hi = a.cand_hi; ss.nblk = a.nblk;
            ss.slot = a.slot; ss.w_exact = W; ss.xn = a.xn_out; ss.K = K;
            dsocr::launch_dec_sample(ss, nullptr);
            check_hip(hipGetLastError(), "screened lm_head launch");
            check_hip(hipDeviceSynchronize(), "screened lm_head");
        } catch (...) {
            for (void* p : bufs) (void)hipFree(p);
            throw;
        }
        for (void* p : bufs) (void)hipFree(p);
    });
}
// the screened head's contract for (B, V, K): EINVAL outside it; true: the matrix-core form runs
static bool screen_shape_mm(int B, int V, int K) {
    if (B < 1 || B > 8 || V < 1 || K < 16 || K % 16 || K > 1536)
        throw std::runtime_error("EINVAL: screened lm_head needs 1..8 rows, V > 0, K % 16 == 0, 16 <= K <= 1536");
    const bool mm = B >= 3;
    if (mm && !dsocr::lmhead_q8mm_ok(B, V, K))
        throw std::runtime_error("EINVAL: screened lm_head for 3..8 rows needs K in {768, 1024, 1280, 1536}, V >= 16");
    return mm;
}
dsocr_status dsocr_k_lmhead_screen_grid(int B, int V, int K, int* nblk, long long* slot, int* matrix_core) {
    return guarded([&] {
        if (!nblk || !slot || !matrix_core) throw std::runtime_error("EINVAL: NULL argument");
        const bool mm = screen_shape_mm(B, V, K);
        int nb = 0;
        long sl = 0;
        if (mm) dsocr::lmhead_q8mm_grid(V, K, B, &nb, &sl);
        else dsocr::lmhead_q8_grid(V, K, B, &nb, &sl);
        *nblk = nb; *slot = sl; *matrix_core = mm ? 1 : 0;
    });
}
dsocr_status dsocr_k_lmhead_screen_steps(const dsocr_screen_steps* sp) {
    return guarded([&] {
        if (!sp) throw std::runtime_error("EINVAL: NULL argument");
        const dsocr_screen_steps& s = *sp;
        const int B = s.B, V = s.V, K = s.K, steps = s.steps;
        const bool mm = screen_shape_mm(B, V, K);
        if (s.wdtype != dsocr::WDT_BF16 && s.wdtype != dsocr::WDT_F16) throw std::runtime_error("EINVAL: weights must be bf16 or f16");
        if (!s.W || steps < 0) throw std::runtime_error("EINVAL: W / steps");
        if (steps > 0) {
            if (!s.x || !s.norm_w || !s.ctx || !s.ctx_len || s.ldx < K || s.ldx % 4 || s.ctx_cap < 1 || s.out_cap < 1 ||
                s.ban_ld < s.ctx_cap + 1 || s.probe < 0 || s.probe >= steps)
                throw std::runtime_error("EINVAL: screened steps need x (ldx >= K, ldx % 4 == 0), norm_w, ctx, ctx_len, "
                                         "out_cap > 0, ban_ld >= ctx_cap + 1, 0 <= probe < steps");
            for (int b = 0; b < B; ++b)
                if (s.ctx_len[b] < 0 || s.ctx_len[b] > s.ctx_cap) throw std::runtime_error("EINVAL: context length");
            if (s.table && (s.H < 1 || (s.table_dt != dsocr::WDT_BF16 && s.table_dt != dsocr::WDT_F16)))
                throw std::runtime_error("EINVAL: embedding table needs H > 0 and a bf16 / f16 type");
            if (s.ban)
                for (int b = 0; b < B; ++b)
                    if (s.ban[(size_t)b * s.ban_ld] < 0 || s.ban[(size_t)b * s.ban_ld] > s.ban_ld - 1)
                        throw std::runtime_error("EINVAL: ban count");
        }
        std::vector<dsocr::RowParams> rp;
        if (s.rows && steps > 0) {
            rp.resize(B);
            for (int b = 0; b < B; ++b) {
                const dsocr_row_params& r = s.rows[b];
                if (r.do_sample != 0 && r.temperature > 0.0) throw std::runtime_error("EINVAL: the screened head takes greedy rows only");
                if (dsocr::rep_penalty_active(r.repetition_penalty)) throw std::runtime_error("EINVAL: the screened head takes no repetition penalty");
                rp[b].ngram = r.no_repeat_ngram_size > 1 ? (int)r.no_repeat_ngram_size : 0;
                rp[b].eos = r.eos_token_id < 0 ? -1 : (int)r.eos_token_id;
            }
        }
        std::vector<void*> bufs;
        auto alloc = [&](size_t b) {
            void* p = nullptr;
            check_hip(hipMalloc(&p, b ? b : 16), "hipMalloc");
            bufs.push_back(p);
            return p;
        };
        auto up = [&](const void* src, size_t b) {
            void* p = alloc(b);
            check_hip(hipMemcpy(p, src, b, hipMemcpyHostToDevice), "hipMemcpy H2D");
            return p;
        };
        auto zeroed = [&](size_t b) {
            void* p = alloc(b);
            check_hip(hipMemset(p, 0, b ? b : 16), "hipMemset");
            return p;
        };
        auto down = [&](void* dst, const void* src, size_t b) {
            if (dst && b) check_hip(hipMemcpy(dst, src, b, hipMemcpyDeviceToHost), "hipMemcpy D2H");
        };
        try {
            // ---- load time, as Engine::load: scale / bound / qnorm padded to whole 16-row tiles and zeroed
            const size_t vp = (size_t)(V + 15) / 16 * 16, I = sizeof(int), F = sizeof(float);
            const bool frag = K % 64 == 0 && (dsocr::lmhead_q8mm_ok(8, V, K) || s.qnorm || s.qfrag);
            void* W = up(s.W, (size_t)V * K * 2);
            void* q = alloc((size_t)V * K);
            float* scale = (float*)zeroed(F * vp);
            float* bound = (float*)zeroed(F * vp);
            float* qnorm = frag ? (float*)zeroed(F * vp) : nullptr;
            void* qfrag = frag ? alloc(dsocr::lmhead_qfrag_bytes(V, K)) : nullptr;
            dsocr::launch_lmhead_quantize(W, V, K, q, scale, bound, nullptr, qnorm, qfrag, s.wdtype);
            check_hip(hipGetLastError(), "lm_head quantisation launch");
            check_hip(hipDeviceSynchronize(), "lm_head quantisation");
            down(s.q, q, (size_t)V * K);
            down(s.scale, scale, F * V);
            down(s.bound, bound, F * V);
            if (frag) {
                down(s.qnorm, qnorm, F * V);
                down(s.qfrag, qfrag, dsocr::lmhead_qfrag_bytes(V, K));
            } else if (s.qnorm || s.qfrag) {
                throw std::runtime_error("EINVAL: the fragment-ordered copy needs K % 64 == 0");
            }
            if (steps > 0) {
                if (mm && !frag) throw std::runtime_error("EINTERNAL: matrix-core form without its copy");
                // ---- per step, as Engine::decode_head's screened branch
                const size_t cap = (size_t)s.ctx_cap, ocap = (size_t)s.out_cap, bld = (size_t)s.ban_ld;
                float* x = (float*)up(s.x, F * (size_t)steps * B * s.ldx);
                float* norm_w = (float*)up(s.norm_w, F * K);
                dsocr::LmHeadQ8Args a;
                a.norm_w = norm_w; a.ldx = s.ldx; a.eps = s.eps; a.q = q; a.scale = scale; a.bound = bound;
                a.B = B; a.N = V; a.K = K;
                if (mm) {
                    a.qfrag = qfrag; a.qnorm = qnorm;
                    dsocr::lmhead_q8mm_grid(V, K, B, &a.nblk, &a.slot);
                } else {
                    dsocr::lmhead_q8_grid(V, K, B, &a.nblk, &a.slot);
                }
                const size_t nb = (size_t)B * a.nblk, nc = nb * (size_t)a.slot;
                a.blk_cnt = (int*)zeroed(I * nb); a.blk_t = (float*)zeroed(F * nb);
                a.cand = (int*)zeroed(I * nc); a.cand_hi = (float*)zeroed(F * nc);
                a.xn_out = (float*)zeroed(F * B * K);
                dsocr::DecSampleArgs ss;
                ss.B = B; ss.V = V; ss.ld = V;
                ss.ctx = (int*)zeroed(I * B * cap); ss.ctx_cap = (long)cap;
                check_hip(hipMemcpy(ss.ctx, s.ctx, I * B * cap, hipMemcpyHostToDevice), "hipMemcpy H2D");
                ss.ctx_len = (int*)up(s.ctx_len, I * B);
                ss.ngram = s.ngram > 1 ? s.ngram : 0; ss.eos = s.eos < 0 ? -1 : s.eos;
                if (!rp.empty()) ss.rows = (const dsocr::RowParams*)up(rp.data(), sizeof(dsocr::RowParams) * B);
                ss.out_tok = (int*)zeroed(I * B);
                ss.out_ids = (int*)zeroed(I * B * ocap); ss.out_len = (int*)zeroed(I * B); ss.out_cap = (long)ocap;
                ss.done = (int*)zeroed(I * B);
                ss.kv_pos = (int*)up(s.ctx_len, I * B); ss.kv_len = (int*)up(s.ctx_len, I * B);
                ss.ban_out = (int*)zeroed(I * B * bld); ss.ban_ld = (long)bld;
                if (s.ban) check_hip(hipMemcpy(ss.ban_out, s.ban, I * B * bld, hipMemcpyHostToDevice), "hipMemcpy H2D");
                if (s.table) {
                    ss.table = up(s.table, (size_t)V * s.H * 2); ss.table_dt = s.table_dt; ss.H = s.H;
                    ss.x_next = (float*)zeroed(F * B * s.H);
                }
                ss.blk_cnt = a.blk_cnt; ss.blk_t = a.blk_t; ss.cand = a.cand; ss.cand_hi = a.cand_hi; ss.nblk = a.nblk;
                ss.slot = a.slot; ss.w_exact = W; ss.w_exact_wdt = s.wdtype; ss.xn = a.xn_out; ss.K = K;
                for (int t = 0; t < steps; ++t) {
                    a.x = x + (size_t)t * B * s.ldx;
                    a.ban = ss.ban_out; a.ban_ld = ss.ban_ld;
                    dsocr::launch_lmhead_q8(a, nullptr);
                    dsocr::launch_dec_sample(ss, nullptr);
                    check_hip(hipGetLastError(), "screened lm_head launch");
                    check_hip(hipDeviceSynchronize(), "screened lm_head");
                    const size_t tb = (size_t)t * B;
                    down(s.out_tok ? s.out_tok + tb : nullptr, ss.out_tok, I * B);
                    down(s.ban_out ? s.ban_out + tb * bld : nullptr, ss.ban_out, I * B * bld);
                    down(s.ctx_out ? s.ctx_out + tb * cap : nullptr, ss.ctx, I * B * cap);
                    down(s.ctx_len_out ? s.ctx_len_out + tb : nullptr, ss.ctx_len, I * B);
                    down(s.out_ids ? s.out_ids + tb * ocap : nullptr, ss.out_ids, I * B * ocap);
                    down(s.out_len ? s.out_len + tb : nullptr, ss.out_len, I * B);
                    down(s.done ? s.done + tb : nullptr, ss.done, I * B);
                    down(s.kv_pos ? s.kv_pos + tb : nullptr, ss.kv_pos, I * B);
                    down(s.kv_len ? s.kv_len + tb : nullptr, ss.kv_len, I * B);
                    if (s.table) down(s.x_next ? s.x_next + tb * s.H : nullptr, ss.x_next, F * B * s.H);
                    if (t == s.probe) {
                        down(s.blk_cnt, a.blk_cnt, I * nb);
                        down(s.blk_t, a.blk_t, F * nb);
                        down(s.cand, a.cand, I * nc);
                        down(s.cand_hi, a.cand_hi, F * nc);
                        down(s.xn_out, a.xn_out, F * B * K);
                        if (s.xn_gemv) {
                            // the rows the exact kernel stages from the same input (dec_gemv's own xn_out, on a few
                            // rows of W: the staging does not depend on N)
                            dsocr::DecGemvArgs g;
                            g.M = B; g.N = std::min(V, 4); g.K = K; g.x = a.x; g.ldx = (int)s.ldx; g.W = W; g.ldw = K;
                            g.wdtype = s.wdtype; g.norm_w = norm_w; g.eps = s.eps;
                            g.y = (float*)zeroed(F * B * 4); g.ldy = 4;
                            g.xn_out = (float*)zeroed(F * B * K);
                            dsocr::launch_dec_gemv(g, nullptr);
                            check_hip(hipGetLastError(), "dec_gemv launch");
                            check_hip(hipDeviceSynchronize(), "dec_gemv");
                            down(s.xn_gemv, g.xn_out, F * B * K);
                        }
                    }
                }
            }
        } catch (...) {
            (void)hipDeviceSynchronize();
            for (void* p : bufs) (void)hipFree(p);
            throw;
        }
        for (void* p : bufs) (void)hipFree(p);
    });
}
dsocr_status dsocr_k_sample_greedy(int B, int V, float* logits, const int* ctx, int ctx_cap, const int* ctx_len,
                                   int ngram, float rep_penalty, int* out_tok) {
    return guarded([&] {
        const int rb = (int)dsocr::dec_sample_blocks(V);
        int *ridx, *done;
        float* rval;
        check_hip(hipMalloc(&ridx, sizeof(int) * B * rb), "hipMalloc");
        check_hip(hipMalloc(&rval, sizeof(float) * B * rb), "hipMalloc");
        check_hip(hipMalloc(&done, sizeof(int) * B), "hipMalloc");
        check_hip(hipMemset(done, 0, sizeof(int) * B), "hipMemset");
        dsocr::SampleArgs p;
        p.logits = logits; p.B = B; p.V = V; p.ld = V; p.ctx = ctx; p.ctx_cap = ctx_cap; p.ctx_len = ctx_len;
        p.rep_penalty = rep_penalty;
        dsocr::launch_rep_penalty(p, nullptr);
        dsocr::DecSampleArgs a;  // selection only: no bookkeeping buffers
        a.logits = logits; a.B = B; a.V = V; a.ld = V; a.ctx = const_cast<int*>(ctx); a.ctx_cap = ctx_cap;
        a.ctx_len = const_cast<int*>(ctx_len); a.ngram = ngram; a.red_val = rval; a.red_idx = ridx;
        a.out_tok = out_tok; a.done = done;
        dsocr::launch_dec_sample(a, nullptr);
        hipError_t e = hipDeviceSynchronize();
        (void)hipFree(ridx); (void)hipFree(rval); (void)hipFree(done);
        check_hip(e, "sample");
    });
}

// the two log-probability launches once on host rows; ctx != NULL: the real penalty launch runs between them
static void k_logprobs(int B, int V, int K, const float* logits, int ld, const int* tok, const uint8_t* emit, float* lp,
                       int64_t* top_id, float* top_lp, const int* ctx, int ctx_cap, const int* ctx_len, float penalty) {
    if (B <= 0 || V <= 0 || K < 0 || K > DSOCR_MAX_TOP_LOGPROBS || ld < V || !logits || !tok || !emit || !lp ||
        (K && (!top_id || !top_lp)) || (ctx && (!ctx_len || ctx_cap <= 0)))
        throw std::runtime_error("EINVAL: bad log-probability arguments");
    for (int b = 0; b < B; ++b) {
        if (tok[b] < 0 || tok[b] >= V) throw std::runtime_error("EINVAL: token id out of bounds for vocab size");
        if (ctx && (ctx_len[b] < 0 || ctx_len[b] > ctx_cap)) throw std::runtime_error("EINVAL: context length");
    }
    std::vector<void*> bufs;
    auto dalloc = [&](size_t bytes) {
        void* p = nullptr;
        check_hip(hipMalloc(&p, bytes ? bytes : 16), "hipMalloc");
        bufs.push_back(p);
        return p;
    };
    auto up = [&](const void* src, size_t bytes) {
        void* p = dalloc(bytes);
        check_hip(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice), "hipMemcpy H2D");
        return p;
    };
    try {
        const size_t nch = dsocr::dec_lp_chunks(V), kk = (size_t)std::max(K, 1);
        std::vector<int> grown(B);
        for (int b = 0; b < B; ++b) grown[b] = emit[b] ? 1 : 0;
        std::vector<float> h_lp(lp, lp + B), h_tl((size_t)B * kk, 0.f);
        std::vector<int> h_ti((size_t)B * kk, 0);
        for (size_t i = 0; i < (size_t)B * K; ++i) { h_ti[i] = (int)top_id[i]; h_tl[i] = top_lp[i]; }
        dsocr::DecLpArgs a;
        float* d_logits = (float*)up(logits, sizeof(float) * (size_t)B * ld);
        a.logits = d_logits; a.B = B; a.V = V; a.ld = ld; a.K = K;
        a.tok = (const int*)up(tok, sizeof(int) * B);
        int* d_len = (int*)dalloc(sizeof(int) * B);
        check_hip(hipMemset(d_len, 0, sizeof(int) * B), "hipMemset");
        a.out_len = d_len; a.out_cap = 1;
        if (ctx) {
            a.ctx = (const int*)up(ctx, sizeof(int) * (size_t)B * ctx_cap);
            a.ctx_cap = ctx_cap;
            a.ctx_len = (const int*)up(ctx_len, sizeof(int) * B);
            a.side = (float*)dalloc(sizeof(float) * (size_t)B * ctx_cap);
        }
        a.rec = (int*)dalloc(sizeof(int) * 2 * B);
        a.part_max = (float*)dalloc(sizeof(float) * B * nch);
        a.part_sum = (float*)dalloc(sizeof(float) * B * nch);
        a.part_tv = (float*)dalloc(sizeof(float) * B * nch * kk);
        a.part_ti = (int*)dalloc(sizeof(int) * B * nch * kk);
        a.lp = (float*)up(h_lp.data(), sizeof(float) * B);
        a.top_id = (int*)up(h_ti.data(), sizeof(int) * B * kk);
        a.top_lp = (float*)up(h_tl.data(), sizeof(float) * B * kk);
        dsocr::launch_dec_lp_partial(a, nullptr);
        if (ctx) {
            dsocr::SampleArgs p;
            p.logits = d_logits; p.B = B; p.V = V; p.ld = ld; p.ctx = a.ctx; p.ctx_cap = ctx_cap; p.ctx_len = a.ctx_len;
            p.rep_penalty = penalty;
            dsocr::launch_rep_penalty(p, nullptr);
        }
        // the selection's part: the output length of every emitting row grows by one
        check_hip(hipMemcpy(d_len, grown.data(), sizeof(int) * B, hipMemcpyHostToDevice), "hipMemcpy H2D");
        dsocr::launch_dec_lp_final(a, nullptr);
        check_hip(hipDeviceSynchronize(), "logprobs");
        check_hip(hipMemcpy(h_lp.data(), a.lp, sizeof(float) * B, hipMemcpyDeviceToHost), "hipMemcpy D2H");
        check_hip(hipMemcpy(h_ti.data(), a.top_id, sizeof(int) * B * kk, hipMemcpyDeviceToHost), "hipMemcpy D2H");
        check_hip(hipMemcpy(h_tl.data(), a.top_lp, sizeof(float) * B * kk, hipMemcpyDeviceToHost), "hipMemcpy D2H");
        // every row back, emitting or not: the device rows started as the caller's values, so a row with emit = 0
        // shows whatever the final kernel did to it
        for (int b = 0; b < B; ++b) {
            lp[b] = h_lp[b];
            for (int k = 0; k < K; ++k) { top_id[(size_t)b * K + k] = h_ti[(size_t)b * K + k]; top_lp[(size_t)b * K + k] = h_tl[(size_t)b * K + k]; }
        }
    } catch (...) {
        for (void* p : bufs) (void)hipFree(p);
        throw;
    }
    for (void* p : bufs) (void)hipFree(p);
}

dsocr_status dsocr_k_logit_bias(int B, int V, int ld, int offset, float* logits, const int64_t* ids, const float* values,
                                const int* first, const int* count, const int* flags, const int* allow_only,
                                float* dense, int dense_ld) {
    return guarded([&] {
        if (B <= 0 || V <= 0 || ld < V || offset < 0 || !logits || !first || !count || !flags || !allow_only || !dense)
            throw std::runtime_error("EINVAL: bad logit bias hook arguments");
        if ((long)dense_ld != dsocr::logit_bias_ld(V)) throw std::runtime_error("EINVAL: dense_ld must be (V + 3) / 4 * 4");
        size_t total = 0;
        for (int b = 0; b < B; ++b) {
            if (first[b] < 0 || count[b] < 0 || count[b] > V) throw std::runtime_error("EINVAL: bad list range");
            total = std::max(total, (size_t)first[b] + (size_t)count[b]);
        }
        if (total && (!ids || !values)) throw std::runtime_error("EINVAL: NULL list");
        std::vector<int> h_ids(total);
        for (size_t i = 0; i < total; ++i) h_ids[i] = (int)std::min<int64_t>(std::max<int64_t>(ids[i], -1), INT32_MAX);
        const size_t nl = (size_t)B * ld, nd = (size_t)B * dense_ld;
        dsocr::DeviceBuffer d_logits((nl + (size_t)offset + 4) * 4), d_dense(nd * 4), d_on((size_t)B * 4),
            d_ids(std::max<size_t>(total, 1) * 4), d_vals(std::max<size_t>(total, 1) * 4);
        float* lg = (float*)d_logits.get() + offset;
        check_hip(hipMemcpy(lg, logits, nl * 4, hipMemcpyHostToDevice), "hipMemcpy H2D");
        check_hip(hipMemset(d_dense.get(), 0, nd * 4), "hipMemset");
        check_hip(hipMemset(d_on.get(), 0, (size_t)B * 4), "hipMemset");
        if (total) {
            check_hip(hipMemcpy(d_ids.get(), h_ids.data(), total * 4, hipMemcpyHostToDevice), "hipMemcpy H2D");
            check_hip(hipMemcpy(d_vals.get(), values, total * 4, hipMemcpyHostToDevice), "hipMemcpy H2D");
        }
        for (int b = 0; b < B; ++b) {
            dsocr::LogitBiasBuildArgs a;
            a.row = (float*)d_dense.get() + (size_t)b * dense_ld; a.V = V; a.ld = dense_ld;
            a.ids = (const int*)d_ids.get() + first[b]; a.values = (const float*)d_vals.get() + first[b]; a.n = count[b];
            a.allow_only = allow_only[b]; a.on = (int*)d_on.get() + b; a.on_value = flags[b] ? 1 : 0;
            dsocr::launch_logit_bias_build(a, nullptr);
        }
        dsocr::DecBiasArgs d;
        d.logits = lg; d.B = B; d.V = V; d.ld = ld; d.bias = (const float*)d_dense.get(); d.bias_ld = dense_ld;
        d.on = (const int*)d_on.get();
        dsocr::launch_dec_logit_bias(d, nullptr);
        check_hip(hipDeviceSynchronize(), "logit bias");
        check_hip(hipMemcpy(logits, lg, nl * 4, hipMemcpyDeviceToHost), "hipMemcpy D2H");
        check_hip(hipMemcpy(dense, d_dense.get(), nd * 4, hipMemcpyDeviceToHost), "hipMemcpy D2H");
    });
}

dsocr_status dsocr_k_stop_match(int B, int steps, int out_cap, const int* n_seq, const int* lens, const int64_t* ids,
                                const int* tokens, const uint8_t* emit, int* out, int* out_len, int* done, int* seen,
                                int* hit, int* done_steps, int* seen_steps, int* hit_steps, int* out_len_steps) {
    return guarded([&] {
        if (B <= 0 || steps < 0 || out_cap <= 0 || !n_seq || !lens || !ids || (steps && (!tokens || !emit)) || !out ||
            !out_len || !done || !seen || !hit)
            throw std::runtime_error("EINVAL: bad stop match hook arguments");
        const size_t nb = (size_t)B, cap = (size_t)out_cap;
        constexpr size_t MS = DSOCR_MAX_STOP_SEQS, ML = DSOCR_MAX_STOP_LEN;
        for (size_t b = 0; b < nb; ++b) {
            if (n_seq[b] < 0 || n_seq[b] > (int)MS) throw std::runtime_error("EINVAL: n_seq outside 0..DSOCR_MAX_STOP_SEQS");
            if (out_len[b] < 0 || out_len[b] > out_cap) throw std::runtime_error("EINVAL: out_len outside 0..out_cap");
            for (int s = 0; s < n_seq[b]; ++s)
                if (lens[b * MS + s] < 1 || lens[b * MS + s] > (int)ML)
                    throw std::runtime_error("EINVAL: a sequence length outside 1..DSOCR_MAX_STOP_LEN");
        }
        const size_t RI = dsocr::STOP_ROW_INTS, SI = dsocr::STOP_STAGE_INTS;
        dsocr::DeviceBuffer d_out(nb * cap * 4), d_len(nb * 4), d_done(nb * 4), d_tab(nb * RI * 4), d_n(nb * 4),
            d_seen(nb * 4), d_hit(nb * 8), d_stage(nb * SI * 4);
        check_hip(hipMemset(d_tab.get(), 0xff, nb * RI * 4), "hipMemset");
        check_hip(hipMemset(d_n.get(), 0, nb * 4), "hipMemset");
        std::vector<int> stage(nb * SI, 0);
        for (size_t b = 0; b < nb; ++b) {
            int* h = &stage[b * SI];
            h[0] = n_seq[b];
            size_t off = 0;
            for (int s = 0; s < n_seq[b]; ++s) {
                const int m = lens[b * MS + s];
                h[1 + s] = m;
                for (int j = 0; j < m; ++j)
                    h[1 + MS + off + j] = (int)std::min<int64_t>(std::max<int64_t>(ids[b * MS * ML + off + j], -1), INT32_MAX);
                off += (size_t)m;
            }
        }
        check_hip(hipMemcpy(d_stage.get(), stage.data(), stage.size() * 4, hipMemcpyHostToDevice), "hipMemcpy H2D");
        for (size_t b = 0; b < nb; ++b) {  // (a row without sequences: nothing is built, its cells keep the caller's values)
            if (!n_seq[b]) continue;
            dsocr::StopBuildArgs a;
            a.stage = (const int*)d_stage.get() + b * SI;
            a.tab = (int*)d_tab.get() + b * RI; a.n_seq = (int*)d_n.get() + b;
            a.seen = (int*)d_seen.get() + b; a.hit = (int*)d_hit.get() + 2 * b;
            dsocr::launch_stop_table_build(a, nullptr);
        }
        check_hip(hipDeviceSynchronize(), "stop table build");
        // the caller's initial cells over what the build reset
        check_hip(hipMemcpy(d_seen.get(), seen, nb * 4, hipMemcpyHostToDevice), "hipMemcpy H2D");
        check_hip(hipMemcpy(d_hit.get(), hit, nb * 8, hipMemcpyHostToDevice), "hipMemcpy H2D");
        dsocr::DecStopArgs m;
        m.B = B; m.out = (const int*)d_out.get(); m.out_cap = out_cap; m.out_len = (const int*)d_len.get();
        m.done = (int*)d_done.get(); m.tab = (const int*)d_tab.get(); m.n_seq = (const int*)d_n.get();
        m.seen = (int*)d_seen.get(); m.hit = (int*)d_hit.get();
        for (int t = 0; t < steps; ++t) {
            // what a final selection kernel does with its token: a done row keeps everything, EOS sets done alone
            for (size_t b = 0; b < nb; ++b) {
                if (done[b]) continue;
                if (!emit[(size_t)t * nb + b]) { done[b] = 1; continue; }
                const int st = out_len[b];
                if (st < out_cap) { out[b * cap + st] = tokens[(size_t)t * nb + b]; out_len[b] = st + 1; }
                if (st + 1 >= out_cap) done[b] = 1;
            }
            check_hip(hipMemcpy(d_out.get(), out, nb * cap * 4, hipMemcpyHostToDevice), "hipMemcpy H2D");
            check_hip(hipMemcpy(d_len.get(), out_len, nb * 4, hipMemcpyHostToDevice), "hipMemcpy H2D");
            check_hip(hipMemcpy(d_done.get(), done, nb * 4, hipMemcpyHostToDevice), "hipMemcpy H2D");
            dsocr::launch_dec_stop_match(m, nullptr);
            check_hip(hipDeviceSynchronize(), "stop match");
            check_hip(hipMemcpy(done, d_done.get(), nb * 4, hipMemcpyDeviceToHost), "hipMemcpy D2H");
            check_hip(hipMemcpy(seen, d_seen.get(), nb * 4, hipMemcpyDeviceToHost), "hipMemcpy D2H");
            check_hip(hipMemcpy(hit, d_hit.get(), nb * 8, hipMemcpyDeviceToHost), "hipMemcpy D2H");
            if (done_steps) std::memcpy(done_steps + (size_t)t * nb, done, nb * 4);
            if (seen_steps) std::memcpy(seen_steps + (size_t)t * nb, seen, nb * 4);
            if (hit_steps) std::memcpy(hit_steps + (size_t)t * nb * 2, hit, nb * 8);
            if (out_len_steps) std::memcpy(out_len_steps + (size_t)t * nb, out_len, nb * 4);
        }
    });
}

dsocr_status dsocr_k_logprobs(int B, int V, int K, const float* logits, int ld, const int* tok, const uint8_t* emit,
                              float* lp, int64_t* top_id, float* top_lp) {
    return guarded([&] { k_logprobs(B, V, K, logits, ld, tok, emit, lp, top_id, top_lp, nullptr, 0, nullptr, 1.f); });
}

dsocr_status dsocr_k_logprobs_penalty(int B, int V, int K, const float* logits, int ld, const int* tok, const uint8_t* emit,
                                      const int* ctx, int ctx_cap, const int* ctx_len, float penalty, float* lp,
                                      int64_t* top_id, float* top_lp) {
    return guarded([&] {
        if (!ctx) throw std::runtime_error("EINVAL: NULL context");
        k_logprobs(B, V, K, logits, ld, tok, emit, lp, top_id, top_lp, ctx, ctx_cap, ctx_len, penalty);
    });
}

// ln_min_p (host [B], optional): one PenaltyRec per row for the sampler (DecSampleArgs::pen)
static dsocr_status k_sample_stoch(int B, int V, float* logits, const int* ctx, int ctx_cap, const int* ctx_len,
                                   int ngram, float rep_penalty, double temperature, size_t top_k, double top_p,
                                   const double* ln_min_p, uint64_t seed, int draws, int* out_tok) {
    return guarded([&] {
        if (B <= 0 || V <= 0 || draws <= 0 || !(temperature > 0.0)) throw std::runtime_error("EINVAL: bad sampling arguments");
        const int rb = (int)dsocr::dec_sample_blocks(V);
        std::vector<void*> bufs;
        auto dalloc = [&](size_t bytes) {
            void* p = nullptr;
            check_hip(hipMalloc(&p, bytes), "hipMalloc");
            bufs.push_back(p);
            return p;
        };
        try {
            int* ridx = (int*)dalloc(sizeof(int) * B * rb);
            float* rval = (float*)dalloc(sizeof(float) * B * rb);
            int* done = (int*)dalloc(sizeof(int) * B);
            check_hip(hipMemset(done, 0, sizeof(int) * B), "hipMemset");
            dsocr::SampleArgs p;
            p.logits = logits; p.B = B; p.V = V; p.ld = V; p.ctx = ctx; p.ctx_cap = ctx_cap; p.ctx_len = ctx_len;
            p.rep_penalty = rep_penalty;
            dsocr::launch_rep_penalty(p, nullptr);
            dsocr::DecSampleArgs a;
            a.logits = logits; a.B = B; a.V = V; a.ld = V; a.ctx = const_cast<int*>(ctx); a.ctx_cap = ctx_cap;
            a.ctx_len = const_cast<int*>(ctx_len); a.ngram = ngram; a.red_val = rval; a.red_idx = ridx; a.done = done;
            a.do_sample = 1; a.temperature = temperature; a.top_k = (long)top_k; a.top_p = top_p; a.st_ld = V;
            a.st_key = (uint32_t*)dalloc(sizeof(uint32_t) * 2 * (size_t)B * V);
            a.st_idx = (int*)dalloc(sizeof(int) * 2 * (size_t)B * V);
            a.st_w = (double*)dalloc(sizeof(double) * (size_t)B * V);
            const std::vector<uint32_t> st = dsocr::rng_state_from_u64(seed);
            a.rng = (uint32_t*)dalloc(sizeof(uint32_t) * dsocr::RNG_WORDS * B);
            for (int b = 0; b < B; ++b)
                check_hip(hipMemcpy(a.rng + (size_t)b * dsocr::RNG_WORDS, st.data(), sizeof(uint32_t) * dsocr::RNG_WORDS,
                                    hipMemcpyHostToDevice), "hipMemcpy");
            if (ln_min_p) {
                std::vector<dsocr::PenaltyRec> recs(B);
                for (int b = 0; b < B; ++b) {
                    if (std::isnan(ln_min_p[b]) || ln_min_p[b] > 0.0) throw std::runtime_error("EINVAL: ln_min_p must be <= 0");
                    recs[b].ln_min_p = ln_min_p[b];
                }
                dsocr::PenaltyRec* d_pen = (dsocr::PenaltyRec*)dalloc(sizeof(dsocr::PenaltyRec) * B);
                check_hip(hipMemcpy(d_pen, recs.data(), sizeof(dsocr::PenaltyRec) * B, hipMemcpyHostToDevice), "hipMemcpy");
                a.pen = d_pen;
            }
            const bool stamps = getenv("DSOCR_SAMPLE_STAMPS") != nullptr;  // diagnostics: phase clocks to stderr
            if (stamps) {
                a.st_stamps = (unsigned long long*)dalloc(sizeof(unsigned long long) * 8);
                check_hip(hipMemset(a.st_stamps, 0, sizeof(unsigned long long) * 8), "hipMemset");
            }
            for (int d = 0; d < draws; ++d) {
                a.out_tok = out_tok + (size_t)d * B;
                dsocr::launch_dec_sample(a, nullptr);
            }
            check_hip(hipDeviceSynchronize(), "sample");
            if (stamps) {
                unsigned long long h[8];
                check_hip(hipMemcpy(h, a.st_stamps, sizeof(h), hipMemcpyDeviceToHost), "hipMemcpy");
                fprintf(stderr, "[sample stamps] phase clocks (shader cycles) from start:");
                for (int i = 1; i < 8; ++i) fprintf(stderr, " %lld", h[i] ? (long long)(h[i] - h[0]) : -1LL);
                fprintf(stderr, "\n");
            }
        } catch (...) {
            for (void* q : bufs) (void)hipFree(q);
            throw;
        }
        for (void* q : bufs) (void)hipFree(q);
    });
}

dsocr_status dsocr_k_sample_stoch(int B, int V, float* logits, const int* ctx, int ctx_cap, const int* ctx_len,
                                  int ngram, float rep_penalty, double temperature, size_t top_k, double top_p,
                                  uint64_t seed, int draws, int* out_tok) {
    return k_sample_stoch(B, V, logits, ctx, ctx_cap, ctx_len, ngram, rep_penalty, temperature, top_k, top_p, nullptr, seed,
                          draws, out_tok);
}

dsocr_status dsocr_k_sample_stoch_min_p(int B, int V, float* logits, const int* ctx, int ctx_cap, const int* ctx_len,
                                        int ngram, float rep_penalty, double temperature, size_t top_k, double top_p,
                                        const double* ln_min_p, uint64_t seed, int draws, int* out_tok) {
    if (!ln_min_p) return guarded([] { throw std::runtime_error("EINVAL: NULL ln_min_p"); });
    return k_sample_stoch(B, V, logits, ctx, ctx_cap, ctx_len, ngram, rep_penalty, temperature, top_k, top_p, ln_min_p, seed,
                          draws, out_tok);
}

dsocr_status dsocr_k_out_penalty(int B, int V, int ld, float* logits, const int* out_ids, int out_cap,
                                 const int* out_len, const dsocr_penalties* pen) {
    return guarded([&] {
        if (B <= 0 || V <= 0 || ld < V || out_cap <= 0 || !logits || !out_ids || !out_len || !pen)
            throw std::runtime_error("EINVAL: bad output penalty hook arguments");
        const size_t nb = (size_t)B, nl = nb * (size_t)ld, cap = (size_t)out_cap;
        std::vector<dsocr::PenaltyRec> recs(nb);
        for (size_t b = 0; b < nb; ++b) {
            if (out_len[b] < 0 || out_len[b] > out_cap) throw std::runtime_error("EINVAL: out_len outside 0..out_cap");
            recs[b].frequency = pen[b].frequency; recs[b].presence = pen[b].presence;
        }
        dsocr::DeviceBuffer d_logits(nl * 4), d_out(nb * cap * 4), d_len(nb * 4), d_rec(nb * sizeof(dsocr::PenaltyRec));
        check_hip(hipMemcpy(d_logits.get(), logits, nl * 4, hipMemcpyHostToDevice), "hipMemcpy H2D");
        check_hip(hipMemcpy(d_out.get(), out_ids, nb * cap * 4, hipMemcpyHostToDevice), "hipMemcpy H2D");
        check_hip(hipMemcpy(d_len.get(), out_len, nb * 4, hipMemcpyHostToDevice), "hipMemcpy H2D");
        check_hip(hipMemcpy(d_rec.get(), recs.data(), nb * sizeof(dsocr::PenaltyRec), hipMemcpyHostToDevice), "hipMemcpy H2D");
        dsocr::DecPenaltyArgs a;
        a.logits = (float*)d_logits.get(); a.B = B; a.V = V; a.ld = ld;
        a.out_ids = (const int*)d_out.get(); a.out_cap = out_cap; a.out_len = (const int*)d_len.get();
        a.rec = (const dsocr::PenaltyRec*)d_rec.get();
        dsocr::launch_dec_out_penalty(a, nullptr);
        check_hip(hipDeviceSynchronize(), "output penalty");
        check_hip(hipMemcpy(logits, d_logits.get(), nl * 4, hipMemcpyDeviceToHost), "hipMemcpy D2H");
    });
}

namespace {
// the hooks' device tables for B rows of one automaton, and its staged copy
struct GuidedHookRows {
    dsocr::DeviceBuffer mask, rowptr, tok, next, words, stage;
    dsocr::GuidedTables t;
    GuidedHookRows(int B, int V, const dsocr::Guided& g) {
        const size_t nb = (size_t)B, E = (size_t)std::max<long>(g.edges(), 1), n = (size_t)g.n_states;
        t.mask_ld = dsocr::guided_mask_ld(V); t.cap_states = g.n_states; t.cap_edges = (long)E;
        mask = dsocr::DeviceBuffer(nb * n * (size_t)t.mask_ld * 4);
        rowptr = dsocr::DeviceBuffer(nb * (n + 1) * 4);
        tok = dsocr::DeviceBuffer(nb * E * 4);
        next = dsocr::DeviceBuffer(nb * E * 4);
        words = dsocr::DeviceBuffer(nb * 4 * 4);
        check_hip(hipMemset(mask.get(), 0xff, nb * n * (size_t)t.mask_ld * 4), "hipMemset");  // (the build must clear it)
        check_hip(hipMemset(words.get(), 0, nb * 16), "hipMemset");
        t.mask = (uint32_t*)mask.get(); t.rowptr = (int*)rowptr.get(); t.tok = (int*)tok.get(); t.next = (int*)next.get();
        t.state = (int*)words.get(); t.seen = t.state + nb; t.status = t.seen + nb; t.on = t.status + nb;
        std::vector<int> h(dsocr::guided_stage_ints(g.n_states, g.edges()));
        for (size_t i = 0; i < n; ++i) h[i] = g.accepting[i] ? 1 : 0;
        std::memcpy(h.data() + n, g.row_ptr.data(), (n + 1) * 4);
        if (g.edges()) {
            std::memcpy(h.data() + 2 * n + 1, g.edge_tok.data(), (size_t)g.edges() * 4);
            std::memcpy(h.data() + 2 * n + 1 + g.edges(), g.edge_next.data(), (size_t)g.edges() * 4);
        }
        stage = dsocr::DeviceBuffer(h.size() * 4);
        check_hip(hipMemcpy(stage.get(), h.data(), h.size() * 4, hipMemcpyHostToDevice), "hipMemcpy H2D");
    }
    void build(int B, int V, const dsocr::Guided& g, long long eos, const int* on) {
        for (int b = 0; b < B; ++b) {
            dsocr::GuidedBuildArgs a;
            a.t = t.at(b);
            if (on[b]) {
                a.stage = (const int*)stage.get();
                a.n_states = g.n_states; a.start = g.start; a.V = V; a.E = g.edges();
                a.eos = (eos >= 0 && eos < V) ? (int)eos : -1;
            }
            dsocr::launch_guided_build(a, nullptr);
        }
        check_hip(hipDeviceSynchronize(), "guided build");
    }
};
}  // namespace

dsocr_status dsocr_k_guided_mask(int B, int V, int ld, int row_off, float* logits, const dsocr_guided* gd, long long eos,
                                 const int* on, const int* state, const int* done, uint32_t* mask_out) {
    return guarded([&] {
        if (B <= 0 || V <= 0 || ld < V || row_off < 0 || row_off > 3 || !logits || !gd || !on || !state || !done || !mask_out)
            throw std::runtime_error("EINVAL: bad guided mask hook arguments");
        const dsocr::Guided g = to_guided(gd, V, eos);
        const size_t nb = (size_t)B, nl = nb * (size_t)ld;
        for (size_t b = 0; b < nb; ++b)
            if (state[b] < -1 || state[b] >= g.n_states) throw std::runtime_error("EINVAL: state outside -1..n_states - 1");
        GuidedHookRows rows(B, V, g);
        rows.build(B, V, g, eos, on);
        dsocr::DeviceBuffer d_logits((nl + (size_t)row_off + 4) * 4), d_done(nb * 4);
        float* lg = (float*)d_logits.get() + row_off;
        check_hip(hipMemcpy(lg, logits, nl * 4, hipMemcpyHostToDevice), "hipMemcpy H2D");
        check_hip(hipMemcpy(d_done.get(), done, nb * 4, hipMemcpyHostToDevice), "hipMemcpy H2D");
        check_hip(hipMemcpy(rows.t.state, state, nb * 4, hipMemcpyHostToDevice), "hipMemcpy H2D");
        dsocr::DecGuidedMaskArgs a;
        a.logits = lg; a.B = B; a.V = V; a.ld = ld; a.done = (const int*)d_done.get(); a.t = rows.t;
        dsocr::launch_dec_guided_mask(a, nullptr);
        check_hip(hipDeviceSynchronize(), "guided mask");
        check_hip(hipMemcpy(logits, lg, nl * 4, hipMemcpyDeviceToHost), "hipMemcpy D2H");
        const size_t row_words = (size_t)g.n_states * (size_t)rows.t.mask_ld;
        std::memset(mask_out, 0, row_words * 4);
        for (size_t b = 0; b < nb; ++b)
            if (on[b]) {
                check_hip(hipMemcpy(mask_out, rows.t.mask + b * row_words, row_words * 4, hipMemcpyDeviceToHost), "hipMemcpy D2H");
                break;
            }
    });
}

dsocr_status dsocr_k_guided_advance(int B, int steps, const dsocr_guided* gd, const int* on, const int* tokens,
                                    const uint8_t* emit, int* steps_out) {
    return guarded([&] {
        if (B <= 0 || steps < 0 || !gd || !on || (steps && (!tokens || !emit || !steps_out)))
            throw std::runtime_error("EINVAL: bad guided advance hook arguments");
        const dsocr::Guided g = to_guided(gd, INT32_MAX, -1);
        const size_t nb = (size_t)B, cap = (size_t)std::max(steps, 1);
        GuidedHookRows rows(B, 32, g);  // (the bitmask is not read here: the smallest one)
        rows.build(B, 32, g, -1, on);
        std::vector<int> out(nb * cap, 0), out_len(nb, 0), done(nb, 0), w(nb * 4);
        dsocr::DeviceBuffer d_out(nb * cap * 4), d_len(nb * 4), d_done(nb * 4);
        dsocr::DecGuidedAdvanceArgs a;
        a.B = B; a.out = (const int*)d_out.get(); a.out_cap = (long)cap; a.out_len = (const int*)d_len.get();
        a.done = (int*)d_done.get(); a.t = rows.t;
        for (int i = 0; i < steps; ++i) {
            for (size_t b = 0; b < nb; ++b) {  // what a final selection kernel appends
                if (done[b] || !emit[(size_t)i * nb + b]) continue;
                out[b * cap + (size_t)out_len[b]] = tokens[(size_t)i * nb + b];
                ++out_len[b];
            }
            check_hip(hipMemcpy(d_out.get(), out.data(), nb * cap * 4, hipMemcpyHostToDevice), "hipMemcpy H2D");
            check_hip(hipMemcpy(d_len.get(), out_len.data(), nb * 4, hipMemcpyHostToDevice), "hipMemcpy H2D");
            check_hip(hipMemcpy(d_done.get(), done.data(), nb * 4, hipMemcpyHostToDevice), "hipMemcpy H2D");
            dsocr::launch_dec_guided_advance(a, nullptr);
            check_hip(hipDeviceSynchronize(), "guided advance");
            check_hip(hipMemcpy(done.data(), d_done.get(), nb * 4, hipMemcpyDeviceToHost), "hipMemcpy D2H");
            check_hip(hipMemcpy(w.data(), rows.words.get(), nb * 16, hipMemcpyDeviceToHost), "hipMemcpy D2H");
            for (size_t b = 0; b < nb; ++b) {
                int* o = steps_out + ((size_t)i * nb + b) * 4;
                o[0] = w[b]; o[1] = w[nb + b]; o[2] = w[2 * nb + b]; o[3] = done[b];
            }
        }
    });
}

dsocr_status dsocr_k_ngram_window(int B, int V, int ld, float* logits, const int* ctx, int ctx_cap, const int* ctx_len,
                                  const dsocr_ngram_window* const* recs, int plain) {
    return guarded([&] {
        if (B <= 0 || V <= 0 || ld < V || ctx_cap <= 0 || !logits || !ctx || !ctx_len || !recs)
            throw std::runtime_error("EINVAL: bad n-gram window hook arguments");
        const size_t nb = (size_t)B, nl = nb * (size_t)ld, cap = (size_t)ctx_cap;
        std::vector<dsocr::NgramWindowRec> rec(nb);
        for (size_t b = 0; b < nb; ++b) {
            if (ctx_len[b] < 0 || ctx_len[b] > ctx_cap) throw std::runtime_error("EINVAL: ctx_len outside 0..ctx_cap");
            rec[b] = to_ngram_window(recs[b], (size_t)V).rec();
        }
        dsocr::DeviceBuffer d_logits(nl * 4), d_ctx(nb * cap * 4), d_len(nb * 4), d_rec(nb * sizeof(dsocr::NgramWindowRec));
        check_hip(hipMemcpy(d_logits.get(), logits, nl * 4, hipMemcpyHostToDevice), "hipMemcpy H2D");
        check_hip(hipMemcpy(d_ctx.get(), ctx, nb * cap * 4, hipMemcpyHostToDevice), "hipMemcpy H2D");
        check_hip(hipMemcpy(d_len.get(), ctx_len, nb * 4, hipMemcpyHostToDevice), "hipMemcpy H2D");
        check_hip(hipMemcpy(d_rec.get(), rec.data(), nb * sizeof(dsocr::NgramWindowRec), hipMemcpyHostToDevice), "hipMemcpy H2D");
        dsocr::DecNgramWindowArgs a;
        a.logits = (float*)d_logits.get(); a.B = B; a.V = V; a.ld = ld;
        a.ctx = (const int*)d_ctx.get(); a.ctx_cap = ctx_cap; a.ctx_len = (const int*)d_len.get();
        a.rec = (const dsocr::NgramWindowRec*)d_rec.get();
        a.plain = plain;
        dsocr::launch_dec_ngram_window(a, nullptr);
        check_hip(hipDeviceSynchronize(), "n-gram window");
        check_hip(hipMemcpy(logits, d_logits.get(), nl * 4, hipMemcpyDeviceToHost), "hipMemcpy D2H");
    });
}

dsocr_status dsocr_k_select_rows(int B, int V, float* logits, const int* ctx, int ctx_cap, const int* ctx_len,
                                 const dsocr_row_params* rows, const uint64_t* seeds, int draws, int* out_tok) {
    return guarded([&] {
        if (B <= 0 || V <= 0 || draws <= 0 || ctx_cap <= 0 || !logits || !ctx || !ctx_len || !rows || !seeds || !out_tok)
            throw std::runtime_error("EINVAL: bad selection arguments");
        // the records as an admission resolves them (host arrays)
        std::vector<dsocr::RowParams> rp(B);
        for (int b = 0; b < B; ++b) {
            const dsocr_row_params& r = rows[b];
            rp[b].do_sample = (r.do_sample != 0 && r.temperature > 0.0) ? 1 : 0;
            rp[b].temperature = r.temperature; rp[b].top_p = r.top_p; rp[b].top_k = (long)r.top_k;
            rp[b].rep_penalty = dsocr::rep_penalty_active(r.repetition_penalty) ? r.repetition_penalty : 1.0f;
            rp[b].ngram = r.no_repeat_ngram_size > 1 ? (int)r.no_repeat_ngram_size : 0;
            rp[b].eos = r.eos_token_id < 0 ? -1 : (int)r.eos_token_id;
        }
        const int rb = (int)dsocr::dec_sample_blocks(V);
        std::vector<void*> bufs;
        auto dalloc = [&](size_t bytes) {
            void* p = nullptr;
            check_hip(hipMalloc(&p, bytes), "hipMalloc");
            bufs.push_back(p);
            return p;
        };
        try {
            dsocr::RowParams* d_rows = (dsocr::RowParams*)dalloc(sizeof(dsocr::RowParams) * B);
            check_hip(hipMemcpy(d_rows, rp.data(), sizeof(dsocr::RowParams) * B, hipMemcpyHostToDevice), "hipMemcpy");
            int* ridx = (int*)dalloc(sizeof(int) * B * rb);
            float* rval = (float*)dalloc(sizeof(float) * B * rb);
            int* done = (int*)dalloc(sizeof(int) * B);
            check_hip(hipMemset(done, 0, sizeof(int) * B), "hipMemset");
            dsocr::SampleArgs p;
            p.logits = logits; p.B = B; p.V = V; p.ld = V; p.ctx = ctx; p.ctx_cap = ctx_cap; p.ctx_len = ctx_len;
            p.rows = d_rows;
            dsocr::launch_rep_penalty(p, nullptr);
            dsocr::DecSampleArgs a;  // selection only: no output rows, so the context does not grow between draws
            a.logits = logits; a.B = B; a.V = V; a.ld = V; a.ctx = const_cast<int*>(ctx); a.ctx_cap = ctx_cap;
            a.ctx_len = const_cast<int*>(ctx_len); a.red_val = rval; a.red_idx = ridx; a.done = done;
            a.rows = d_rows;
            a.ban_ld = (long)ctx_cap + 1;
            a.ban_out = (int*)dalloc(sizeof(int) * (size_t)B * a.ban_ld);
            a.st_ld = V;
            a.st_key = (uint32_t*)dalloc(sizeof(uint32_t) * 2 * (size_t)B * V);
            a.st_idx = (int*)dalloc(sizeof(int) * 2 * (size_t)B * V);
            a.st_w = (double*)dalloc(sizeof(double) * (size_t)B * V);
            a.rng = (uint32_t*)dalloc(sizeof(uint32_t) * dsocr::RNG_WORDS * B);
            for (int b = 0; b < B; ++b) {
                const std::vector<uint32_t> st = dsocr::rng_state_from_u64(seeds[b]);
                check_hip(hipMemcpy(a.rng + (size_t)b * dsocr::RNG_WORDS, st.data(), sizeof(uint32_t) * dsocr::RNG_WORDS,
                                    hipMemcpyHostToDevice), "hipMemcpy");
            }
            for (int d = 0; d < draws; ++d) {
                a.out_tok = out_tok + (size_t)d * B;
                dsocr::launch_dec_sample(a, nullptr);
            }
            check_hip(hipDeviceSynchronize(), "select_rows");
        } catch (...) {
            for (void* q : bufs) (void)hipFree(q);
            throw;
        }
        for (void* q : bufs) (void)hipFree(q);
    });
}

// ---------------------------------------------------------------- dots.ocr vision tower
dsocr_status dsocr_dots_load(const char* config_path, const char* weights_path, uint64_t seed, int device,
                             dsocr_dots** out) {
    return guarded([&] {
        if (!config_path || !out) throw std::runtime_error("EINVAL: NULL argument");
        std::unique_ptr<dsocr_dots> d(new dsocr_dots);
        d->impl.reset(new dsocr::DotsVision(config_path, weights_path ? weights_path : "", seed, device));
        *out = d.release();
    });
}
void dsocr_dots_free(dsocr_dots* d) { delete d; }
dsocr_status dsocr_dots_info(const dsocr_dots* d, size_t* hidden, size_t* embed, size_t* layers, size_t* patch_dim) {
    return guarded([&] {
        if (!d) throw std::runtime_error("EINVAL: NULL handle");
        const dsocr::DotsConfig& c = d->impl->cfg();
        if (hidden) *hidden = c.hidden;
        if (embed) *embed = c.embed;
        if (layers) *layers = c.layers;
        if (patch_dim) *patch_dim = (size_t)c.channels * c.patch * c.patch;
    });
}
dsocr_status dsocr_dots_preprocess(const char* config_path, const uint8_t* rgb, uint32_t w, uint32_t h, float* patches,
                                   size_t cap, size_t* n_patches, uint32_t* grid) {
    return guarded([&] {
        if (!config_path || !rgb || !n_patches) throw std::runtime_error("EINVAL: NULL argument");
        std::ifstream f(config_path);
        if (!f) throw std::runtime_error(std::string("ENOENT: cannot read config ") + config_path);
        std::stringstream ss;
        ss << f.rdbuf();
        const dsocr::DotsConfig c = dsocr::parse_dots_config(dsocr::Json::parse(ss.str()));
        const dsocr::DotsPatches p = dsocr::dots_preprocess(c, rgb, (int)w, (int)h);
        const size_t n = (size_t)p.grid_t * p.grid_h * p.grid_w;
        *n_patches = n;
        if (grid) { grid[0] = p.grid_t; grid[1] = p.grid_h; grid[2] = p.grid_w; }
        if (patches) {
            if (n > cap) throw std::runtime_error("EINVAL: patch capacity too small");
            std::memcpy(patches, p.data.data(), p.data.size() * 4);
        }
    });
}
dsocr_status dsocr_dots_embed(dsocr_dots* d, const uint8_t* rgb, uint32_t w, uint32_t h, float* out, size_t cap_rows,
                              size_t* n_rows, uint32_t* grid) {
    return guarded([&] {
        if (!d || !rgb || !n_rows) throw std::runtime_error("EINVAL: NULL argument");
        const dsocr::DotsConfig& c = d->impl->cfg();
        const dsocr::DotsPatches p = dsocr::dots_preprocess(c, rgb, (int)w, (int)h);
        const size_t groups = (size_t)p.grid_t * p.grid_h * p.grid_w / (c.merge * c.merge);
        *n_rows = groups;
        if (grid) { grid[0] = p.grid_t; grid[1] = p.grid_h; grid[2] = p.grid_w; }
        if (groups > cap_rows) throw std::runtime_error("EINVAL: output capacity too small");
        std::vector<float> r = d->impl->embed(p);
        if (out) std::memcpy(out, r.data(), r.size() * 4);
    });
}
dsocr_status dsocr_dots_embed_device(dsocr_dots* d, const float* patches, uint32_t gt, uint32_t gh, uint32_t gw,
                                     float* out, int time_attention_layers) {
    return guarded([&] {
        if (!d || !patches || !out || !gt || !gh || !gw) throw std::runtime_error("EINVAL: bad arguments");
        d->impl->time_layers = std::max(0, time_attention_layers);
        d->impl->embed_device(patches, (int)gt, (int)gh, (int)gw, out);
        d->impl->time_layers = 0;
    });
}
dsocr_status dsocr_dots_last_timings(const dsocr_dots* d, dsocr_dots_timings* t) {
    return guarded([&] {
        if (!d || !t) throw std::runtime_error("EINVAL: NULL argument");
        const dsocr::DotsTimings x = d->impl->last_timings();
        t->total_ms = x.total_ms; t->patch_ms = x.patch_ms; t->blocks_ms = x.blocks_ms;
        t->attention_ms = x.attention_ms; t->merger_ms = x.merger_ms; t->tokens = x.tokens; t->groups = x.groups;
    });
}

}  // extern "C"
