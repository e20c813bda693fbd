"""Mixed-length pages through three decode paths on one GPU.

32 text pages of bench.py's kind (dsocr.synth.text_page_prompt), full-size synthetic weights, greedy, eos ignored.
Page i generates MAX_NEW[i] tokens: drawn once, numpy default_rng(4011).choice(LENGTHS, 32).
  (a) generate, one page after another (what the server does behind its lock)
  (b) generate_batch in arrival-order groups of 8 (a closed batch runs to its longest page; ids truncated after)
  (c) one 8-slot session fed in arrival order, bursts of 8 steps, finished pages retired at every burst boundary
  (d) the same session opened per request (DSOCR_SESSION_PER_REQUEST), every request default greedy: it must replay
      (c)'s launches (zero exact-head steps) and land inside (c)'s min-max spread
  (e) (d) with every fourth request sampled (T 0.7, top-p 0.9, seeded): the per-row exact head whenever one is active
  (f) (e)'s traffic through BatchScheduler over a fixed session: a sampled request waits for the session to drain
      and runs alone (what (e) replaces)
  (g) (c) opened with DSOCR_SESSION_LOGPROBS: the exact head plus the two log-probability launches every step, every
      page's entries (20 alternatives) read before its retire
  (h) (c) with DSOCR_SCREEN=0: the exact head without log-probabilities, so (h) - (g) is what the two launches and
      the reads cost and (c) - (h) what the head switch costs
  (p) the page prefix cache, on its own traffic: 16 full-size image pages, each asked two prompts in
      arrival order (32 requests of 64 tokens) through one 8-slot session, with the cache off (every request pays
      vision and the full prefill: the parent's code path) and on (the second prompt is admitted behind the kept
      prefix); the two alternate ROUNDS times; requests/s, steps and the wall time of a plain admission, a keep and
      a prefix admission
  (q) chunked admission, on (c)'s 32 text pages and on (p)'s image pages (one prompt each): plain
      admission (the parent's code path) against admit_begin / admit_advance with 128-row chunks, one slice per burst
      of 8 steps, alternating ROUNDS times; pages/s, the largest and 99th-percentile wall gap between two consecutive
      bursts while a slot runs, and the wall time per slice by kind
The arms alternate ROUNDS times; pages/s and decode steps are reported as median [min, max].  Also: the wall time
of one admission while other slots wait, and one session_slot_move of a 1200-row full-size page against its bytes.

    python tools/session_bench.py [--rounds 3] [--pages 32] [--arms a,b,c,d,e,f,g,h,p,q] [--out profiles/session_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "deepseek-ocr.rs_amd")]

LENGTHS = [64, 96, 128, 192, 256, 384, 512]
SLOTS = 8


def mmm(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run_single(eng, reqs, max_new, P):
    steps = 0
    for r, m in zip(reqs, max_new):
        out = eng.generate(r, None, None, None, P(max_new_tokens=m), ignore_eos=True)
        assert len(out) == m
        steps += eng.last_timings()["decode_steps"]
    return steps, {}


def run_batches(eng, reqs, max_new, P):
    steps = 0
    for g in range(0, len(reqs), SLOTS):
        group, ms = reqs[g:g + SLOTS], max_new[g:g + SLOTS]
        out = eng.generate_batch([(r, None, None, None) for r in group], P(max_new_tokens=max(ms)), ignore_eos=True)
        assert all(len(o) == max(ms) for o in out)
        steps += eng.last_timings()["decode_steps"]
    return steps, {}


def run_session(eng, reqs, max_new, P, logprobs=False):
    need = max(len(r) + m + 1 for r, m in zip(reqs, max_new))
    stalls, moves, done, nxt = [], [], 0, 0
    kw = {"logprobs": True} if logprobs else {}
    with eng.open_session(SLOTS, need, P(max_new_tokens=max(max_new)), ignore_eos=True, **kw) as s:
        active = 0
        while done < len(reqs):
            while active < SLOTS and nxt < len(reqs):
                t = time.perf_counter()
                s.admit(reqs[nxt], max_new_tokens=max_new[nxt])
                if active:
                    stalls.append((time.perf_counter() - t) * 1e3)
                active, nxt = active + 1, nxt + 1
            for st in sorted(s.step(8), key=lambda x: -x.slot):
                if st.done:
                    if logprobs:
                        lp, _, _ = s.logprobs(st.slot, 0, st.out_len, 20)
                        assert len(lp) == st.out_len and np.isfinite(lp).all()
                    t = time.perf_counter()
                    _, moved = s.retire(st.slot)
                    if moved >= 0:
                        moves.append((time.perf_counter() - t) * 1e3)
                    active, done = active - 1, done + 1
        steps, heads = s.info()["steps"], s.head_steps()
    return steps, {"admit_stall_ms": stalls, "retire_with_move_ms": moves, "head_steps": heads}


def run_session_exact(eng, reqs, max_new, P):
    """run_session under DSOCR_SCREEN=0 (read per call by the engine): the exact head, nothing else changed."""
    old = os.environ.get("DSOCR_SCREEN")
    os.environ["DSOCR_SCREEN"] = "0"
    try:
        return run_session(eng, reqs, max_new, P)
    finally:
        if old is None:
            del os.environ["DSOCR_SCREEN"]
        else:
            os.environ["DSOCR_SCREEN"] = old


SAMPLED = dict(do_sample=True, temperature=0.7, top_p=0.9)


def request_params(i, m, P, mixed):
    """Request i's own parameters: default greedy, or with `mixed` every fourth one sampled (seed 1000 + i)."""
    if mixed and i % 4 == 3:
        return P(max_new_tokens=m, seed=1000 + i, **SAMPLED)
    return P(max_new_tokens=m)


def run_session_params(eng, reqs, max_new, P, mixed):
    need = max(len(r) + m + 1 for r, m in zip(reqs, max_new))
    done, nxt = 0, 0
    with eng.open_session(SLOTS, need, P(max_new_tokens=max(max_new)), ignore_eos=True, per_request=True) as s:
        active = 0
        while done < len(reqs):
            while active < SLOTS and nxt < len(reqs):
                s.admit(reqs[nxt], params=request_params(nxt, max_new[nxt], P, mixed))
                active, nxt = active + 1, nxt + 1
            for st in sorted(s.step(8), key=lambda x: -x.slot):
                if st.done:
                    s.retire(st.slot)
                    active, done = active - 1, done + 1
        steps, heads = s.info()["steps"], s.head_steps()
    return steps, {"head_steps": heads}


class _SchedEngine:
    """The engine as BatchScheduler drives it, for prompts "KEY" that name one of the bench's token lists."""
    variant = 0

    def __init__(self, eng, reqs):
        self.eng, self.reqs, self.steps = eng, reqs, 0

    def open_session(self, slots, max_context, params):
        self._s = self.eng.open_session(slots, max_context, params, ignore_eos=True)
        close = self._s.close

        def closing():
            self.steps += self._s.info()["steps"]
            close()
        self._s.close = closing
        return self._s

    def decode(self, tokenizer, prompt, images, vision, params, stream=None):
        from dsocr import DecodeOutcome
        ids = self.eng.generate(self.reqs[int(prompt)], None, None, None, params, ignore_eos=True)
        self.steps += self.eng.last_timings()["decode_steps"]
        return DecodeOutcome("", len(self.reqs[int(prompt)]), len(ids), ids)


def run_scheduler_fixed(eng, reqs, max_new, P, mixed=True):
    from dsocr.scheduler import BatchScheduler
    need = max(len(r) + m + 1 for r, m in zip(reqs, max_new))
    se = _SchedEngine(eng, reqs)
    with BatchScheduler(se, None, SLOTS, need, P(max_new_tokens=max(max_new)),
                        prepare=lambda e, t, prompt, images, vision: (reqs[int(prompt)], [0] * len(reqs[int(prompt)]), [])) as sc:
        futs = [sc.submit(str(i), params=request_params(i, m, P, mixed)) for i, m in enumerate(max_new)]
        outs = [f.result() for f in futs]
        alone = sc.exclusive_runs
    assert all(o.response_tokens == m for o, m in zip(outs, max_new))
    return se.steps, {"exclusive_runs": alone}


PREFIX_PROMPTS = ["<image>\nConvert the document to markdown.", "<image>\nFree OCR."]
PREFIX_NEW = 64  # tokens per request of the prefix arms


def image_requests(eng, pages):
    """`pages` full-size image pages (bench.py's synthetic_page, pixels HBM-resident), each under PREFIX_PROMPTS:
    [(page, [(ids, mask)] per prompt, prefix rows)]."""
    from dsocr import Page, VisionSettings, build_prompt_tokens
    from dsocr.synth import SyntheticTokenizer, synthetic_page
    tok, vs, out = SyntheticTokenizer(eng.vocab), VisionSettings(1024, 640, True), []
    for i in range(pages):
        page = Page(synthetic_page(i), vs, eng)
        prompts = [build_prompt_tokens(tok, p, [page.n_image_tokens]) for p in PREFIX_PROMPTS]
        out.append((page, prompts, max(j for j, m in enumerate(prompts[0][1]) if m) + 1))
    return out


def run_prefix(eng, docs, P, cache):
    """Every page's prompts in arrival order (page 0 prompt 0, page 0 prompt 1, page 1 prompt 0, ...) through one
    8-slot session.  cache: the first prompt's admission is followed by keep_prefix, the later prompts go through
    admit_prefix, and the handle is dropped after the page's last prompt.  Wall times per call, in ms."""
    reqs = [(d, j) for d in range(len(docs)) for j in range(len(PREFIX_PROMPTS))]
    need = max(len(ids) for _, prompts, _ in docs for ids, _ in prompts) + PREFIX_NEW + 1
    t_plain, t_prefix, t_keep, handles = [], [], [], {}
    done, nxt, active = 0, 0, 0
    with eng.open_session(SLOTS, need, P(max_new_tokens=PREFIX_NEW), ignore_eos=True) as s:
        while done < len(reqs):
            while active < SLOTS and nxt < len(reqs):
                d, j = reqs[nxt]
                page, prompts, rows = docs[d]
                ids, mask = prompts[j]
                t = time.perf_counter()
                if cache and d in handles:
                    s.admit_prefix(handles[d], ids, mask, max_new_tokens=PREFIX_NEW)
                    t_prefix.append((time.perf_counter() - t) * 1e3)
                    if j == len(PREFIX_PROMPTS) - 1:
                        s.drop_prefix(handles.pop(d))
                else:
                    slot = s.admit(ids, mask, page, max_new_tokens=PREFIX_NEW)
                    t_plain.append((time.perf_counter() - t) * 1e3)
                    if cache:
                        t = time.perf_counter()
                        handles[d] = s.keep_prefix(slot, rows)
                        t_keep.append((time.perf_counter() - t) * 1e3)
                active, nxt = active + 1, nxt + 1
            for st in sorted(s.step(8), key=lambda x: -x.slot):
                if st.done:
                    s.retire(st.slot)
                    active, done = active - 1, done + 1
        steps, stats = s.info()["steps"], s.prefix_stats()
    return steps, {"admit_plain_ms": t_plain, "admit_prefix_ms": t_prefix, "keep_prefix_ms": t_keep,
                   "prefix_stats": stats}


def prefix_arms(eng, P, pages, rounds):
    """The page prefix cache: cache off (the parent's code path) and on, alternating."""
    docs = image_requests(eng, pages)
    for cache in (False, True):  # warm-up: workspaces and graphs
        run_prefix(eng, docs[:4], P, cache)
    res = {k: {"pages_s": [], "steps": [], "plain": [], "prefix": [], "keep": []} for k in ("cache_off", "cache_on")}
    for _ in range(rounds):
        for k, cache in (("cache_off", False), ("cache_on", True)):
            t = time.perf_counter()
            steps, extra = run_prefix(eng, docs, P, cache)
            r = res[k]
            r["pages_s"].append(len(docs) * len(PREFIX_PROMPTS) / (time.perf_counter() - t))
            r["steps"].append(int(steps))
            r["plain"] += extra["admit_plain_ms"]
            r["prefix"] += extra["admit_prefix_ms"]
            r["keep"] += extra["keep_prefix_ms"]
            r["stats"] = extra["prefix_stats"]
    out = {"pages": pages, "prompts_per_page": len(PREFIX_PROMPTS), "max_new": PREFIX_NEW, "rounds": rounds,
           "prefix_rows": docs[0][2], "prompt_len": [len(ids) for ids, _ in docs[0][1]]}
    for k, r in res.items():
        out[k] = {"requests_s": mmm(r["pages_s"]), "requests_s_rounds": r["pages_s"], "steps": mmm(r["steps"]),
                  "admit_plain_ms": mmm(r["plain"]), "prefix_stats": r["stats"]}
        if r["prefix"]:
            out[k]["admit_prefix_ms"] = mmm(r["prefix"])
            out[k]["keep_prefix_ms"] = mmm(r["keep"])
    out["on_over_off"] = out["cache_on"]["requests_s"]["median"] / out["cache_off"]["requests_s"]["median"]
    return out


def run_admission(eng, items, P, chunk):
    """items [(ids, mask, page, max_new)] in arrival order through one 8-slot session, a burst of 8 steps per turn.
    chunk = 0: every free slot is filled by a plain admission before the burst.  chunk > 0: one admission at a time
    in slices, one slice per turn.  Gaps: wall ms from the end of a burst to the start of the next while a slot ran."""
    need = max(len(it[0]) + it[3] + 1 for it in items)
    gaps, slices, admits = [], {"sam": [], "clip": [], "projector": [], "prefill": []}, []
    done, nxt, active, pending, last_end = 0, 0, 0, False, None
    with eng.open_session(SLOTS, need, P(max_new_tokens=max(it[3] for it in items)), ignore_eos=True) as s:
        while done < len(items):
            if chunk:
                if not pending and active < SLOTS and nxt < len(items):
                    ids, mask, page, m = items[nxt]
                    s.admit_begin(ids, mask, page, chunk_rows=chunk, max_new_tokens=m)
                    pending, nxt = True, nxt + 1
                if pending:
                    kind = ("prefill", "sam", "clip", "projector")[s.admit_progress()["vision_stage"]]
                    t = time.perf_counter()
                    fin, _ = s.admit_advance()
                    slices[kind].append((time.perf_counter() - t) * 1e3)
                    if fin:
                        pending, active = False, active + 1
            else:
                while active < SLOTS and nxt < len(items):
                    ids, mask, page, m = items[nxt]
                    t = time.perf_counter()
                    s.admit(ids, mask, page, max_new_tokens=m)
                    admits.append((time.perf_counter() - t) * 1e3)
                    active, nxt = active + 1, nxt + 1
            if not active:
                last_end = None
                continue
            t = time.perf_counter()
            if last_end is not None:
                gaps.append((t - last_end) * 1e3)
            status = s.step(8)
            last_end = time.perf_counter()
            for st in sorted(status, key=lambda x: -x.slot):
                if st.done:
                    s.retire(st.slot)
                    active, done = active - 1, done + 1
            if not active:
                last_end = None
            elif any(st.done for st in status):
                last_end = time.perf_counter()  # (a retire is not part of the gap an admission causes)
        steps = s.info()["steps"]
    return steps, {"gaps": gaps, "slices": slices, "admits": admits}


def chunk_arms(eng, P, text_items, image_items, rounds, chunk=128):
    out = {"chunk_rows": chunk, "rounds": rounds, "burst": 8}
    for name, items in (("text_pages", text_items), ("image_pages", image_items)):
        for c in (0, chunk):  # warm-up
            run_admission(eng, items[:SLOTS + 2], P, c)
        res = {k: {"pages_s": [], "gap_max": [], "gap_p99": [], "slices": {}, "admits": []} for k in ("plain", "chunked")}
        for _ in range(rounds):
            for k, c in (("plain", 0), ("chunked", chunk)):
                t = time.perf_counter()
                _, extra = run_admission(eng, items, P, c)
                r = res[k]
                r["pages_s"].append(len(items) / (time.perf_counter() - t))
                r["gap_max"].append(max(extra["gaps"]))
                r["gap_p99"].append(float(np.percentile(extra["gaps"], 99)))
                r["admits"] += extra["admits"]
                for kind, v in extra["slices"].items():
                    r["slices"].setdefault(kind, []).extend(v)
        out[name] = {"pages": len(items), "prompt_len": len(items[0][0])}
        for k, r in res.items():
            o = {"pages_s": mmm(r["pages_s"]), "gap_max_ms": mmm(r["gap_max"]), "gap_p99_ms": mmm(r["gap_p99"])}
            if r["admits"]:
                o["admit_ms"] = mmm(r["admits"])
            o["slice_ms"] = {kind: dict(mmm(v), n=len(v)) for kind, v in r["slices"].items() if v}
            out[name][k] = o
        out[name]["chunked_over_plain"] = out[name]["chunked"]["pages_s"]["median"] / out[name]["plain"]["pages_s"]["median"]
    return out


def slot_move_alone(cfg, rows=1200, reps=10):
    """dsocr_k_session_slot_move at the full-size cache shape, two slots: call wall time (launch + synchronise)."""
    from dsocr._lib import check, lib
    lang = cfg.get("language_config") or cfg
    layers, heads = int(lang["num_hidden_layers"]), int(lang["num_attention_heads"])
    kvh = int(lang.get("num_key_value_heads") or heads)
    hd = int(lang.get("head_dim") or int(lang["hidden_size"]) // heads)
    cap = rows + 8
    L = lib()
    n = layers * 2 * kvh * cap * hd * 4
    kc, vc, kl = C.c_void_p(), C.c_void_p(), C.c_void_p()
    for p, b in ((kc, n), (vc, n), (kl, 8)):
        check(L.dsocr_dev_alloc(b, C.byref(p)))
    lens = np.array([1, rows], np.int32)
    check(L.dsocr_memcpy_h2d(kl, lens.ctypes.data_as(C.c_void_p), 8))
    ms = []
    try:
        for i in range(reps + 2):
            t = time.perf_counter()
            check(L.dsocr_k_session_slot_move(layers, 2, kvh, cap, hd, kc, vc, kl, None, None, 0, None, None, 0, None,
                                              None, None, None, 0, None, 0, None, 0, 1, 0))
            if i >= 2:
                ms.append((time.perf_counter() - t) * 1e3)
            check(L.dsocr_memcpy_h2d(kl, lens.ctypes.data_as(C.c_void_p), 8))
    finally:
        for p in (kc, vc, kl):
            L.dsocr_dev_free(p)
    moved = 2 * layers * kvh * rows * hd * 4  # K and V, read once and written once each
    r = mmm(ms)
    r.update(rows=rows, bytes_copied=moved, gb_s_read_plus_write=2 * moved / (r["median"] * 1e-3) / 1e9)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--arms", default="a,b,c,d,e,f", help="which arms run (letters, comma separated)")
    ap.add_argument("--prefix-pages", type=int, default=16, help="image pages of arm p (two prompts each)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import dsocr
    from dsocr import DecodeParameters as P, ModelLoadArgs, load_model
    from dsocr.synth import text_page_prompt
    eng = load_model(ModelLoadArgs(config_path=dsocr.FULL_CONFIG, synthetic_seed=0, dtype="f16"))
    max_new = [int(v) for v in np.random.default_rng(4011).choice(LENGTHS, a.pages)]
    reqs = [text_page_prompt(i, vocab=eng.vocab) for i in range(a.pages)]
    paths = {"a_generate": run_single, "b_generate_batch": run_batches, "c_session": run_session,
             "d_session_per_request_greedy": lambda *x: run_session_params(*x, mixed=False),
             "e_session_per_request_mixed": lambda *x: run_session_params(*x, mixed=True),
             "f_scheduler_fixed_mixed": run_scheduler_fixed,
             "g_session_logprobs": lambda *x: run_session(*x, logprobs=True),
             "h_session_exact_head": run_session_exact}
    paths = {k: f for k, f in paths.items() if k[0] in a.arms.split(",")}
    for f in paths.values():  # warm-up: workspaces, fragment-ordered weights, graphs
        f(eng, reqs[:SLOTS], [16] * SLOTS, P)
    res = {k: {"pages_s": [], "steps": [], "extra": []} for k in paths}
    for _ in range(a.rounds):
        for k, f in paths.items():
            t = time.perf_counter()
            steps, extra = f(eng, reqs, max_new, P)
            res[k]["pages_s"].append(a.pages / (time.perf_counter() - t))
            res[k]["steps"].append(int(steps))
            res[k]["extra"].append(extra)
    out = {"pages": a.pages, "max_new": max_new, "prompt_len": len(reqs[0]), "rounds": a.rounds,
           "sampled_requests": {"every_fourth": [i for i in range(a.pages) if i % 4 == 3], "seed": "1000 + index",
                                "params": SAMPLED}}
    for k, v in res.items():
        out[k] = {"pages_s": mmm(v["pages_s"]), "pages_s_rounds": v["pages_s"], "steps": mmm(v["steps"])}
        for key in ("head_steps", "exclusive_runs"):
            if v["extra"] and key in v["extra"][0]:
                out[k][key] = v["extra"][-1][key]
    if "c_session" in res:
        stalls = [x for e in res["c_session"]["extra"] for x in e["admit_stall_ms"]]
        moves = [x for e in res["c_session"]["extra"] for x in e["retire_with_move_ms"]]
        out["c_session"]["admit_stall_ms"] = mmm(stalls) if stalls else None
        out["c_session"]["retire_with_move_ms"] = mmm(moves) if moves else None
    med = lambda k: out[k]["pages_s"]["median"]  # noqa: E731
    for name, (x, y) in {"c_over_a": ("c_session", "a_generate"), "c_over_b": ("c_session", "b_generate_batch"),
                         "d_over_c": ("d_session_per_request_greedy", "c_session"),
                         "e_over_f": ("e_session_per_request_mixed", "f_scheduler_fixed_mixed"),
                         "g_over_c": ("g_session_logprobs", "c_session"),
                         "g_over_h": ("g_session_logprobs", "h_session_exact_head")}.items():
        if x in out and y in out:
            out[name] = med(x) / med(y)
    if "d_over_c" in out:
        c = out["c_session"]["pages_s"]
        out["d_within_c_spread"] = bool(c["min"] <= med("d_session_per_request_greedy") <= c["max"])
    if "p" in a.arms.split(","):
        out["p_prefix_cache"] = prefix_arms(eng, P, a.prefix_pages, a.rounds)
    if "q" in a.arms.split(","):
        docs = image_requests(eng, a.prefix_pages)
        out["q_chunked_admission"] = chunk_arms(
            eng, P, [(r, None, None, m) for r, m in zip(reqs, max_new)],
            [(prompts[0][0], prompts[0][1], page, PREFIX_NEW) for page, prompts, _ in docs], a.rounds)
    eng.close()
    out["slot_move_1200_rows"] = slot_move_alone(json.load(open(dsocr.FULL_CONFIG)))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
