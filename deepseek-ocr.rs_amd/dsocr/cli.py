"""`deepseek-ocr-cli` for the MI355X engine: same flags, same stdout/stderr behaviour.

Mirrors crates/cli (args.rs:10-101, app.rs:40-330, prompt.rs:7-19, bench.rs:200-260) and the
shared flags of crates/config/src/args.rs:9-92.  What differs, and why:

* The reference resolves model files through its app-config TOML and downloads missing ones
  (`prepare_model_paths`); this CLI takes explicit paths (`--model-config`, `--weights`,
  `--tokenizer`, `--snapshot`) — there is no network and the config store is control plane.
  Without `--weights` the engine builds the deterministic synthetic checkpoint (same names
  and shapes), selected by `--synthetic-seed`.
* `--device` accepts `hip` / `hip:N` (also the reference spellings `cuda` / `cuda:N`, mapped
  to the HIP ordinal); `cpu` / `metal` are refused — the product path has no CPU engine.
* Sampling flags behave as the reference's: `--do-sample true --temperature T [--top-k K]
  [--top-p P] [--seed S]` samples on the GPU with the reference's RNG (sampling.hip); without a
  positive temperature selection is greedy (sampling.rs:67).

Usage: python -m dsocr.cli --prompt "<image>\\nConvert the document to markdown." --image page.png
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from typing import List, Optional

from . import FULL_CONFIG, OCR2_CONFIG
from ._lib import DsocrError
from .engine import DecodeParameters, ModelLoadArgs, VisionSettings, load_model, render_prompt
from .streaming import DeltaTracker, decode_ids


def _bool(v: str) -> bool:
    s = v.strip().lower()
    if s in ("1", "true", "yes", "on"):
        return True
    if s in ("0", "false", "no", "off"):
        return False
    raise argparse.ArgumentTypeError(f"invalid boolean {v!r}")


def add_model_args(p: argparse.ArgumentParser) -> None:
    """CommonModelArgs (config/src/args.rs:9-29)."""
    g = p.add_argument_group("Application")
    g.add_argument("--config", metavar="PATH", help="application config (accepted for compatibility; unused)")
    g.add_argument("--model", metavar="ID", default="deepseek-ocr",
                   help="model id: deepseek-ocr or deepseek-ocr-2 (MI355X engine), or paddleocr-vl (host CPU plumbing "
                        "path, configs[0])")
    g.add_argument("--model-config", metavar="PATH", help="model config.json (default: the bundled config of --model)")
    g.add_argument("--tokenizer", metavar="PATH", help="tokenizer.json (default: synthetic tokenizer)")
    g.add_argument("--weights", metavar="PATH", help="model .safetensors (default: synthetic weights)")
    g.add_argument("--snapshot", metavar="PATH", help="DSQ snapshot (.dsq) to dequantise on load")
    g.add_argument("--snapshot-packed", action="store_true", default=None,
                   help="decode the MoE experts from the snapshot's packed Q4_K / Q8_0 blocks (needs --snapshot; "
                        "default: the DSOCR_DSQ_PACKED environment switch decides)")
    g.add_argument("--synthetic-seed", type=int, default=0, help="seed of the synthetic checkpoint")


def add_inference_args(p: argparse.ArgumentParser) -> None:
    """CommonInferenceArgs (config/src/args.rs:31-92)."""
    g = p.add_argument_group("Inference")
    g.add_argument("--device", default="hip", help="hip | hip:N (cuda[:N] is accepted as an alias)")
    g.add_argument("--dtype", default="f16", choices=["f32", "f16", "bf16"])
    g.add_argument("--template", default="plain")
    g.add_argument("--base-size", type=int, default=None, help="default: the model's (1024)")
    g.add_argument("--image-size", type=int, default=None, help="default: the model's (640; deepseek-ocr-2: 768)")
    g.add_argument("--crop-mode", type=_bool, default=True, metavar="BOOL")
    g.add_argument("--max-new-tokens", type=int, default=512)
    g.add_argument("--no-cache", action="store_true")
    g.add_argument("--do-sample", type=_bool, default=False, metavar="BOOL")
    g.add_argument("--temperature", type=float, default=0.0)
    g.add_argument("--top-p", type=float, default=1.0)
    g.add_argument("--top-k", type=int, default=None)
    g.add_argument("--repetition-penalty", type=float, default=1.0)
    g.add_argument("--no-repeat-ngram-size", type=int, default=20)
    g.add_argument("--seed", type=int, default=None)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="deepseek-ocr-cli", description="DeepSeek-OCR CLI (MI355X engine)")
    add_model_args(p)
    add_inference_args(p)
    pr = p.add_mutually_exclusive_group()
    pr.add_argument("--prompt", help="prompt text; `<image>` marks image slots")
    pr.add_argument("--prompt-file", metavar="PATH", help="UTF-8 prompt file")
    p.add_argument("--image", dest="images", action="append", default=[], metavar="PATH",
                   help="image files for the <image> placeholders, in order")
    b = p.add_argument_group("Benchmark")
    b.add_argument("--bench", action="store_true", help="print per-stage timings")
    b.add_argument("--bench-output", metavar="PATH", help="write benchmark events to a JSON file")
    p.add_argument("-q", "--quiet", action="store_true", help="print only the final result")
    p.add_argument("--logprobs", type=int, default=None, metavar="K",
                   help="after the text, one JSON line per generated token: its id, its log-probability and the K "
                        "(0..20) most likely alternatives")
    p.add_argument("--ban-token", dest="ban_tokens", action="append", type=int, default=[], metavar="ID",
                   help="never emit this token id (repeatable)")
    p.add_argument("--allow-tokens-file", metavar="PATH",
                   help="emit only the token ids listed in this file, one id per line (blank lines and # comments skipped)")
    p.add_argument("--logit-bias", dest="logit_biases", action="append", default=[], metavar="ID=VALUE",
                   help="add VALUE to the logit of token ID before every selection (repeatable)")
    p.add_argument("--stop", dest="stops", action="append", default=[], metavar="STR",
                   help="end the generation in front of this string (repeatable, at most 16 stops in all)")
    p.add_argument("--stop-token-ids", metavar="ID,ID,...",
                   help="end the generation in front of any of these token ids")
    p.add_argument("--include-stop", action="store_true", help="keep the matched stop in the output")
    p.add_argument("--frequency-penalty", type=float, default=None, metavar="X",
                   help="lower a generated token's logit by X for every time it was generated so far")
    p.add_argument("--presence-penalty", type=float, default=None, metavar="X",
                   help="lower the logit of every token generated so far by X")
    p.add_argument("--min-p", type=float, default=None, metavar="X",
                   help="when sampling, keep only tokens at least X (0..1) times as likely as the most likely one")
    p.add_argument("--guided-choice", action="append", default=None, metavar="STR",
                   help="the output must be one of the given strings (repeat the option once per string): a token "
                        "automaton over their tokenisations constrains every step on the device")
    p.add_argument("--ngram-window-size", type=int, default=None, metavar="N",
                   help="ban the continuation of every N-gram that already occurs within the last --ngram-window "
                        "context tokens (replaces --no-repeat-ngram-size for the run); 0 = off")
    p.add_argument("--ngram-window", type=int, default=None, metavar="W",
                   help="the window of --ngram-window-size in tokens (default 100)")
    p.add_argument("--ngram-whitelist", metavar="ID,ID,...",
                   help="token ids --ngram-window-size never bans (at most 32)")
    p.add_argument("--slots", type=int, default=0, metavar="N",
                   help="treat every --image as its own one-page document (the prompt has one <image>) and decode them "
                        "together in a session of N slots (1..8); results print in input order.  0 = off")
    p.add_argument("--max-context", type=int, default=4096,
                   help="with --slots: context rows per slot (a page needs prompt + max_new_tokens + 1)")
    p.add_argument("--per-request-params", action="store_true",
                   help="with --slots: open the session per request, every page admitted with its own decode "
                        "parameters (device-side per-row selection); off by default")
    p.add_argument("--admit-chunk", type=int, default=0, metavar="ROWS",
                   help="with --slots: admit every page in slices (its vision, then ROWS >= 32 prompt rows at a time) "
                        "with a burst of the running pages between two slices; 0 = off (the default)")
    return p


# the engine's model ids -> (bundled config, base_size, image_size): the registry defaults of config.rs:96-110
ENGINE_MODELS = {"deepseek-ocr": (FULL_CONFIG, 1024, 640), "deepseek": (FULL_CONFIG, 1024, 640),
                 "deepseek-ocr-2": (OCR2_CONFIG, 1024, 768)}


def model_config(args) -> str:
    if args.model not in ENGINE_MODELS:
        raise DsocrError(1, f"model `{args.model}` is not served by the MI355X engine (deepseek-ocr, deepseek-ocr-2)")
    return args.model_config or ENGINE_MODELS[args.model][0]


def vision_settings(args) -> VisionSettings:
    """--base-size / --image-size, else the model's registry defaults."""
    _, base, image = ENGINE_MODELS.get(args.model, (None, 1024, 640))
    return VisionSettings(base if args.base_size is None else args.base_size,
                          image if args.image_size is None else args.image_size, args.crop_mode)


def parse_device(spec: str) -> int:
    s = spec.strip().lower()
    for pre in ("hip", "cuda"):
        if s == pre:
            return 0
        if s.startswith(pre + ":") and s[len(pre) + 1:].isdigit():
            return int(s[len(pre) + 1:])
    raise DsocrError(1, f"device {spec!r} is not supported by the MI355X engine (use hip or hip:N)")


def load_prompt(args) -> str:
    """prompt.rs:7-19."""
    if args.prompt_file:
        with open(args.prompt_file, encoding="utf-8") as f:
            return f.read()
    if args.prompt is not None:
        return args.prompt
    raise DsocrError(1, "prompt is required (use --prompt or --prompt-file)")


def decode_params(args) -> DecodeParameters:
    return DecodeParameters(max_new_tokens=args.max_new_tokens, do_sample=args.do_sample,
                            temperature=args.temperature, top_p=args.top_p, top_k=args.top_k,
                            repetition_penalty=args.repetition_penalty,
                            no_repeat_ngram_size=args.no_repeat_ngram_size, seed=args.seed,
                            use_cache=not args.no_cache)


def load_tokenizer(path: Optional[str], vocab_size: int):
    if path:
        from tokenizers import Tokenizer
        return Tokenizer.from_file(path)
    from .synth import SyntheticTokenizer
    return SyntheticTokenizer(vocab_size)


def open_image(path: str):
    from PIL import Image
    try:
        with Image.open(path) as im:
            return im.convert("RGB")
    except (OSError, ValueError) as e:
        raise DsocrError(3, f"failed to open image at {path}: {e}") from e


def stage_report(events: List[dict]) -> dict:
    """bench.rs:200-245: events + per-stage totals (count/total/avg/min/max ms)."""
    totals = {}
    for ev in events:
        t = totals.setdefault(ev["stage"], [])
        t.append(ev["duration_ms"])
    stage_totals = [{"stage": k, "count": len(v), "total_ms": sum(v), "total_ns": str(int(sum(v) * 1e6)),
                     "avg_ms": sum(v) / len(v), "min_ms": min(v), "max_ms": max(v)} for k, v in sorted(totals.items())]
    return {"events": events, "stage_totals": stage_totals}


def _event(stage: str, ms: float, **fields) -> dict:
    return {"stage": stage, "duration_ms": ms, "duration_ns": str(int(ms * 1e6)),
            "fields": [{"key": k, "value": v} for k, v in fields.items()]}


def token_constraint(args) -> dict:
    """--ban-token / --allow-tokens-file / --logit-bias as the keywords of ``engine.decode`` ({} when none is given).
    Syntax errors are reported here, before any load; ids are checked against the vocabulary by ``decode``."""
    kw = {}
    bias = {}
    for item in getattr(args, "logit_biases", None) or []:
        k, sep, v = item.partition("=")
        try:
            if not sep:
                raise ValueError
            t, f = int(k), float(v)
        except ValueError:
            raise DsocrError(1, f"--logit-bias takes ID=VALUE (an integer id, a number), not {item!r}") from None
        if t in bias:
            raise DsocrError(1, f"--logit-bias names token {t} twice")
        bias[t] = f
    if bias:
        kw["logit_bias"] = bias
    if getattr(args, "ban_tokens", None):
        kw["banned_token_ids"] = list(args.ban_tokens)
    path = getattr(args, "allow_tokens_file", None)
    if path:
        ids = []
        try:
            with open(path, encoding="utf-8") as f:
                for n, line in enumerate(f, 1):
                    text = line.split("#", 1)[0].strip()
                    if text:
                        try:
                            ids.append(int(text))
                        except ValueError:
                            raise DsocrError(1, f"{path}:{n}: {text!r} is not a token id") from None
        except OSError as e:
            raise DsocrError(2, f"cannot read --allow-tokens-file {path}: {e}") from None
        if not ids:
            raise DsocrError(1, f"--allow-tokens-file {path} lists no token id")
        kw["allowed_token_ids"] = ids
    if kw and getattr(args, "slots", 0):
        raise DsocrError(1, "--ban-token / --allow-tokens-file / --logit-bias apply to one document: not with --slots")
    kw.update(stop_arguments(args))
    kw.update(penalty_arguments(args))
    kw.update(ngram_window_arguments(args))
    guided_choices(args)
    return kw


def guided_choices(args) -> list:
    """--guided-choice as the list of strings ([] when the option is absent).  Checked here, before any load; the
    automaton needs the tokenizer and is built by ``guided_arguments``."""
    choices = getattr(args, "guided_choice", None) or []
    if any(c == "" for c in choices):
        raise DsocrError(1, "--guided-choice takes a non-empty string")
    if choices and getattr(args, "slots", 0):
        raise DsocrError(1, "--guided-choice applies to one document: not with --slots")
    return list(choices)


def guided_arguments(args, tokenizer) -> dict:
    """--guided-choice as the keyword of ``engine.decode`` ({} when the option is absent)."""
    from .guided import GuidedError, choice_automaton
    choices = guided_choices(args)
    if not choices:
        return {}
    try:
        return {"guided": choice_automaton(tokenizer, choices)}
    except GuidedError as e:
        raise DsocrError(1, f"--guided-choice: {e}") from None


def ngram_window_arguments(args) -> dict:
    """--ngram-window-size / --ngram-window / --ngram-whitelist as the keyword of ``engine.decode`` ({} when they ask
    for nothing).  Checked here, before any load."""
    from .ngram_window import NgramWindowError, make_ngram_window
    white = getattr(args, "ngram_whitelist", None)
    try:
        ids = None
        if white is not None:
            try:
                ids = [int(t) for t in white.split(",") if t.strip()]
            except ValueError:
                raise NgramWindowError("--ngram-whitelist takes token ids separated by commas") from None
        rec = make_ngram_window(getattr(args, "ngram_window_size", None), getattr(args, "ngram_window", None), ids)
    except NgramWindowError as e:
        raise DsocrError(1, f"--ngram-window-size / --ngram-window / --ngram-whitelist: {e}") from None
    if rec is None:
        return {}
    if getattr(args, "slots", 0):
        raise DsocrError(1, "--ngram-window-size applies to one document: not with --slots")
    return rec.kwargs()


def penalty_arguments(args) -> dict:
    """--frequency-penalty / --presence-penalty / --min-p as the keywords of ``engine.decode`` ({} when they ask for
    nothing).  Checked here, before any load."""
    from .penalties import PenaltyError, make_penalties
    try:
        pn = make_penalties(getattr(args, "frequency_penalty", None), getattr(args, "presence_penalty", None),
                            getattr(args, "min_p", None))
    except PenaltyError as e:
        raise DsocrError(1, f"--frequency-penalty / --presence-penalty / --min-p: {e}") from None
    if pn is None:
        return {}
    if getattr(args, "slots", 0):
        raise DsocrError(1, "--frequency-penalty / --presence-penalty / --min-p apply to one document: not with --slots")
    return {"frequency_penalty": pn.frequency, "presence_penalty": pn.presence, "min_p": pn.min_p}


def stop_arguments(args) -> dict:
    """--stop / --stop-token-ids / --include-stop as the keywords of ``engine.decode`` ({} when none is given).
    Syntax errors are reported here, before any load; the stops are encoded and checked by ``decode``."""
    kw = {}
    if getattr(args, "stops", None):
        if any(not s for s in args.stops):
            raise DsocrError(1, "--stop takes a non-empty string")
        kw["stop"] = list(args.stops)
    raw = getattr(args, "stop_token_ids", None)
    if raw:
        try:
            kw["stop_token_ids"] = [int(t) for t in raw.split(",") if t.strip()]
        except ValueError:
            raise DsocrError(1, f"--stop-token-ids takes integers separated by commas, not {raw!r}") from None
    if kw and getattr(args, "slots", 0):
        raise DsocrError(1, "--stop / --stop-token-ids apply to one document: not with --slots")
    if kw:
        kw["include_stop_in_output"] = bool(getattr(args, "include_stop", False))
    elif getattr(args, "include_stop", False):
        raise DsocrError(1, "--include-stop needs --stop or --stop-token-ids")
    return kw


def check_admit_chunk(args) -> None:
    """--admit-chunk is a setting of the decode session: refused without --slots and below 32 rows, before any load."""
    rows = int(getattr(args, "admit_chunk", 0) or 0)
    if rows and (not getattr(args, "slots", 0) or rows < 32):
        raise DsocrError(1, "--admit-chunk needs --slots and ROWS >= 32 (a chunked admission runs in a decode session)")


def run_inference(args, out=sys.stdout, err=sys.stderr) -> int:
    def info(msg):
        if not args.quiet:
            print(msg, file=err, flush=True)

    check_admit_chunk(args)
    constraint = token_constraint(args)
    prompt_raw = load_prompt(args)
    if args.model in PADDLE_IDS:
        return run_paddle(args, prompt_raw, out, err)
    device = parse_device(args.device)
    config = model_config(args)
    vocab = _vocab_of(config)
    events = []
    t0 = time.perf_counter()
    engine = load_model(ModelLoadArgs(config_path=config, weights_path=args.weights, snapshot_path=args.snapshot,
                                      snapshot_packed=getattr(args, "snapshot_packed", None),
                                      device=device, dtype=args.dtype, synthetic_seed=args.synthetic_seed))
    load_ms = (time.perf_counter() - t0) * 1e3
    events.append(_event("model.load", load_ms, model=args.model, kind="Deepseek", device=f"hip:{device}",
                         dtype=args.dtype))
    info(f"Model ready in {load_ms / 1e3:.2f}s (kind=Deepseek, flash-attn: true, weights="
         f"{args.weights or f'synthetic(seed={args.synthetic_seed})'})")
    try:
        tokenizer = load_tokenizer(args.tokenizer, vocab)
        constraint.update(guided_arguments(args, tokenizer))
        prompt = render_prompt(args.template, "", prompt_raw)
        slots = prompt.count("<image>")
        if getattr(args, "slots", 0):
            return run_documents(args, engine, tokenizer, prompt, out, info)
        if slots != len(args.images):
            raise DsocrError(1, f"prompt includes {slots} <image> tokens but {len(args.images)} image paths "
                                f"were provided")
        images = [open_image(p) for p in args.images]
        vision = vision_settings(args)
        params = decode_params(args)

        tracker = DeltaTracker()
        state = {"last": 0, "prefill_s": None}
        start = time.perf_counter()

        def on_token(count, ids):
            if count > 0 and state["prefill_s"] is None:
                state["prefill_s"] = time.perf_counter() - start
            if count <= state["last"]:
                state["last"] = count
                return
            delta = tracker.advance(decode_ids(tokenizer, ids[:count]), False)
            state["last"] = count
            if delta:
                out.write(delta)
                out.flush()

        info(f"Starting generation with requested budget {params.max_new_tokens} tokens")
        lp_k = getattr(args, "logprobs", None)
        if lp_k is not None and not 0 <= lp_k <= 20:
            raise DsocrError(1, "--logprobs takes 0..20")
        if lp_k is None and not constraint:
            outcome = engine.decode(tokenizer, prompt, images, vision, params, None if args.quiet else on_token)
        elif lp_k is None:  # a constrained decode does not stream: the text is written once, below
            outcome = engine.decode(tokenizer, prompt, images, vision, params, None, **constraint)
        else:  # the entries arrive with the ids: the text is written once, below
            outcome = engine.decode(tokenizer, prompt, images, vision, params, None, logprobs=lp_k, **constraint)
        elapsed = time.perf_counter() - start
        decoded = decode_ids(tokenizer, outcome.generated_tokens)
        if "include_stop_in_output" in constraint:  # stops: the text as the outcome cut it
            decoded = outcome.text
        if args.quiet:
            out.write(outcome.text + "\n")
        else:
            tail = tracker.advance(decoded, True)
            if tail:
                out.write(tail)
            out.write("\n")
            out.flush()
            info(f"Final output:\n{outcome.text}")
        if lp_k is not None:
            for tok, lp, top in zip(outcome.generated_tokens, outcome.token_logprobs, outcome.top_logprobs):
                out.write(json.dumps({"id": int(tok), "logprob": lp if lp > float("-inf") else -9999.0,
                                      "top_logprobs": [{"id": int(i), "logprob": v if v > float("-inf") else -9999.0}
                                                       for i, v in top if i >= 0]}) + "\n")
            out.flush()
        prefill_s = state["prefill_s"] if state["prefill_s"] is not None and state["prefill_s"] <= elapsed \
            else elapsed
        decode_s = max(elapsed - prefill_s, 0.0)
        info(f"Throughput: prefill={outcome.prompt_tokens} tok in {prefill_s:.2f}s "
             f"({outcome.prompt_tokens / prefill_s if prefill_s > 0 else 0.0:.2f} tok/s); "
             f"generation={outcome.response_tokens} tok in {decode_s:.2f}s "
             f"({outcome.response_tokens / decode_s if decode_s > 0 else 0.0:.2f} tok/s)")
        if args.bench or args.bench_output:
            t = engine.last_timings()
            events += [_event("vision.prepare_inputs", t["vision_prepare_ms"]),
                       _event("vision.compute_embeddings", t["vision_compute_ms"]),
                       _event("decode.prefill", t["decode_prefill_ms"], tokens=outcome.prompt_tokens),
                       _event("decode.iterative", t["decode_iterative_ms"], tokens=outcome.response_tokens),
                       _event("decode.generate", t["decode_generate_ms"])]
            report = stage_report(events)
            if args.bench_output:
                d = os.path.dirname(args.bench_output)
                if d:
                    os.makedirs(d, exist_ok=True)
                with open(args.bench_output, "w") as f:
                    json.dump(report, f, indent=2)
            if args.bench:
                for s in report["stage_totals"]:
                    print(f"[bench] {s['stage']:<28} count={s['count']:<3} total={s['total_ms']:.2f}ms "
                          f"avg={s['avg_ms']:.2f}ms", file=err)
    finally:
        engine.close()
    return 0


def run_documents(args, engine, tokenizer, prompt: str, out, info) -> int:
    """--slots N: every --image is a one-page document decoded with the same prompt; the pages share one decode
    session (scheduler.BatchScheduler) and the results are written in input order."""
    from .scheduler import BatchScheduler

    if prompt.count("<image>") != 1:
        raise DsocrError(1, "--slots decodes every --image as its own document: the prompt needs exactly one <image>")
    if not args.images:
        raise DsocrError(1, "--slots needs at least one --image")
    images = [open_image(p) for p in args.images]
    start = time.perf_counter()
    per_request = bool(getattr(args, "per_request_params", False))
    with BatchScheduler(engine, tokenizer, args.slots, args.max_context, decode_params(args),
                        vision_settings(args), per_request_params=per_request,
                        admit_chunk=int(getattr(args, "admit_chunk", 0) or 0)) as sched:
        futures = [sched.submit(prompt, [im], params=decode_params(args) if per_request else None) for im in images]
        outcomes = [f.result() for f in futures]
    elapsed = time.perf_counter() - start
    for path, o in zip(args.images, outcomes):
        if not args.quiet:
            out.write(f"==> {path} <==\n")
        out.write(o.text + "\n")
    out.flush()
    info(f"{len(outcomes)} pages, {sum(o.response_tokens for o in outcomes)} tokens in {elapsed:.2f}s "
         f"({len(outcomes) / elapsed if elapsed > 0 else 0.0:.2f} pages/s)")
    return 0


PADDLE_IDS = ("paddleocr-vl", "paddleocr", "paddle-ocr-vl")


def run_paddle(args, prompt_raw: str, out=sys.stdout, err=sys.stderr) -> int:
    """ModelKind::PaddleOcrVl on the host CPU (crates/infer-paddleocr model.rs:286-416; BASELINE configs[0]:
    Candle CPU backend plumbing): dsocr.paddle's numpy restatement with a seeded synthetic checkpoint."""
    from . import paddle

    def info(msg):
        if not args.quiet:
            print(msg, file=err, flush=True)

    if args.device.strip().lower() not in ("cpu", "hip", "cuda") and not args.device.lower().startswith(("hip:", "cuda:")):
        raise DsocrError(1, f"device {args.device!r} is not supported")
    if args.weights or args.snapshot:
        raise DsocrError(1, "the PaddleOCR-VL CPU path runs the seeded synthetic checkpoint only (no weights offline)")
    t0 = time.perf_counter()
    engine = paddle.PaddleOcrEngine(args.model_config or paddle.PADDLE_CONFIG, synthetic_seed=args.synthetic_seed)
    load_ms = (time.perf_counter() - t0) * 1e3
    info(f"Model ready in {load_ms / 1e3:.2f}s (kind=PaddleOcrVl, device=cpu, weights=synthetic(seed={args.synthetic_seed}))")
    if args.tokenizer:
        from tokenizers import Tokenizer
        tokenizer = Tokenizer.from_file(args.tokenizer)
    else:
        tokenizer = paddle.PaddleSyntheticTokenizer(engine.cfg)
    prompt = render_prompt(args.template, "", prompt_raw)
    slots = prompt.count("<image>")
    if slots != len(args.images):
        raise DsocrError(1, f"prompt includes {slots} <image> tokens but {len(args.images)} image paths were provided")
    images = [open_image(p) for p in args.images]
    vision = vision_settings(args)
    outcome = engine.decode(tokenizer, prompt, images, vision, decode_params(args))
    out.write(outcome.text + "\n")
    info(f"generated {outcome.response_tokens} tokens: {outcome.generated_tokens}")
    if args.bench or args.bench_output:
        t = engine.last_timings()
        events = [_event("model.load", load_ms, model=args.model, kind="PaddleOcrVl", device="cpu"),
                  _event("vision.compute_embeddings", t["vision_compute_ms"]),
                  _event("decode.prefill", t["decode_prefill_ms"], tokens=outcome.prompt_tokens),
                  _event("decode.iterative", t["decode_iterative_ms"], tokens=outcome.response_tokens)]
        report = stage_report(events)
        if args.bench_output:
            with open(args.bench_output, "w") as f:
                json.dump(report, f, indent=2)
        if args.bench:
            for s_ in report["stage_totals"]:
                print(f"[bench] {s_['stage']:<28} count={s_['count']:<3} total={s_['total_ms']:.2f}ms", file=err)
    engine.close()
    return 0


def _vocab_of(config_path: str) -> int:
    with open(config_path) as f:
        cfg = json.load(f)
    lang = cfg.get("language_config") or {}
    return int(lang.get("vocab_size") or cfg.get("vocab_size") or 129280)


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    try:
        return run_inference(args)
    except DsocrError as e:
        print(f"Error: {e}", file=sys.stderr)
        return 1


if __name__ == "__main__":
    sys.exit(main())
