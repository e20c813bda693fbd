"""Host-side mirror of the reference engine surface, bound to the C ABI.

Mirrors (TimmyOVO/deepseek-ocr.rs):
  * ``ModelLoadArgs`` / ``load_model``           core/src/inference.rs:178-186, model/mod.rs:90-115
  * ``VisionSettings`` / ``DecodeParameters``    core/src/inference.rs:13-79 (same defaults)
  * ``DecodeOutcome``                            core/src/inference.rs:161-167
  * ``OcrEngine.decode``                         model/mod.rs:2370-2455
  * ``build_prompt_tokens``                      model/mod.rs:2536-2603
  * ``render_prompt`` (plain template)           core/src/inference.rs:212-225, conversation/mod.rs:115-125
  * ``normalize_text``                           core/src/inference.rs:228-233
All compute runs in libdsocr.so on a gfx950 GPU; this module only marshals.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Any, Callable, Optional, Sequence

import numpy as np

from ._lib import (DTYPES, LOAD_PACKED_EXPERTS, MAX_TOP_LOGPROBS, DecodeParamsC, DsocrError, LoadArgs, LogitBiasC, LogprobsC,
                   GuidedC, GuidedResultC, NgramWindowC, PenaltiesC, SESSION_GUIDED, RequestC, ResultC, STREAM_CB, SESSION_LOGIT_BIAS, SESSION_LOGPROBS,
                   SESSION_NGRAM_WINDOW, SESSION_PENALTIES,
                   SESSION_PER_REQUEST, SESSION_STOP,
                   SessionDescC, SlotStatusC, StopHitC, StopSetC, TimingsC, VisionSettingsC, check, lib)
from .constraint import ConstraintError, LogitConstraint, merge_constraint
from .guided import STATUS_NAMES, GuidedError, TokenAutomaton
from .ngram_window import NgramWindow, NgramWindowError, make_ngram_window
from .penalties import Penalties, PenaltyError, make_penalties
from .stops import StopError, StopSet, apply_stops, merge_stops


def _stops(stop, stop_token_ids, tokenizer, vocab, stops: Optional[StopSet] = None) -> Optional[StopSet]:
    """The request's stop set: ``stops`` as merged elsewhere, or the two request arguments merged (dsocr.stops); a bad
    one is the engine's EINVAL."""
    if stops is not None:
        return stops
    try:
        return merge_stops(stop, stop_token_ids, tokenizer, vocab)
    except StopError as e:
        raise DsocrError(1, f"EINVAL: stop set: {e}") from None


def _stop_c(ss: Optional[StopSet], keep) -> Optional[StopSetC]:
    if ss is None:
        return None
    ids = np.ascontiguousarray([t for q in ss.seqs for t in q], np.int64)
    lens = (C.c_size_t * len(ss.seqs))(*[len(q) for q in ss.seqs])
    keep += [ids, lens]
    return StopSetC(ids.ctypes.data_as(C.POINTER(C.c_int64)), lens, len(ss.seqs))


def _constraint(logit_bias, allowed_token_ids, banned_token_ids, vocab) -> Optional[LogitConstraint]:
    """The three request arguments merged (dsocr.constraint); a bad one is the engine's EINVAL."""
    try:
        return merge_constraint(logit_bias, allowed_token_ids, banned_token_ids, vocab)
    except ConstraintError as e:
        raise DsocrError(1, f"EINVAL: logit bias: {e}") from None


def _bias_c(c: Optional[LogitConstraint], keep) -> Optional[LogitBiasC]:
    if c is None:
        return None
    ids = np.ascontiguousarray(c.ids, np.int64)
    vals = np.ascontiguousarray(c.values, np.float32)
    keep += [ids, vals]
    return LogitBiasC(ids.ctypes.data_as(C.POINTER(C.c_int64)), vals.ctypes.data_as(C.POINTER(C.c_float)), len(ids),
                      1 if c.allow_only else 0)


def _penalties(frequency_penalty, presence_penalty, min_p) -> Optional[Penalties]:
    """The three request arguments as one checked record (dsocr.penalties), None when they ask for nothing; a bad
    one is the engine's EINVAL."""
    try:
        return make_penalties(frequency_penalty, presence_penalty, min_p)
    except PenaltyError as e:
        raise DsocrError(1, f"EINVAL: penalties: {e}") from None


def _penalties_c(pn: Optional[Penalties]) -> Optional[PenaltiesC]:
    """(a record of three numbers: nothing for the caller to keep alive)"""
    if pn is None:
        return None
    return PenaltiesC(pn.frequency, pn.presence, pn.min_p)


def _ngram_window(ngram_window, vocab) -> Optional[NgramWindow]:
    """The ``ngram_window=`` argument (a ``dsocr.ngram_window.NgramWindow``, a mapping with ``ngram_size`` / ``window``
    / ``whitelist``, or None) as one checked record, None when it asks for nothing; a bad one is the engine's EINVAL."""
    try:
        if ngram_window is None or isinstance(ngram_window, NgramWindow):
            return make_ngram_window(ngram_window, vocab=vocab)
        if isinstance(ngram_window, dict):
            extra = set(ngram_window) - {"ngram_size", "window", "whitelist"}
            if extra:
                raise NgramWindowError(f"unknown field {sorted(extra)[0]!r}")
            return make_ngram_window(ngram_window.get("ngram_size"), ngram_window.get("window"),
                                     ngram_window.get("whitelist"), vocab=vocab)
        raise NgramWindowError("ngram_window must be a NgramWindow record or a mapping")
    except NgramWindowError as e:
        raise DsocrError(1, f"EINVAL: n-gram window: {e}") from None


def _ngram_window_c(nw: Optional[NgramWindow], keep) -> Optional[NgramWindowC]:
    """(``keep`` holds the whitelist array alive until the call returns)"""
    if nw is None:
        return None
    n = len(nw.whitelist)
    arr = (C.c_int32 * max(n, 1))(*nw.whitelist)
    keep.append(arr)
    return NgramWindowC(nw.ngram_size, nw.window, C.cast(arr, C.POINTER(C.c_int32)), n)


def _guided(guided, vocab) -> Optional[TokenAutomaton]:
    """The ``guided=`` argument (a ``dsocr.guided.TokenAutomaton`` or None), checked against the vocabulary; the EOS
    rule is the engine's own check.  A bad one is the engine's EINVAL."""
    if guided is None:
        return None
    if not isinstance(guided, TokenAutomaton):
        raise DsocrError(1, "EINVAL: token automaton: guided must be a dsocr.guided.TokenAutomaton")
    try:
        return guided.validate(vocab, None)
    except GuidedError as e:
        raise DsocrError(1, f"EINVAL: token automaton: {e}") from None


def _guided_c(ta: Optional[TokenAutomaton], keep) -> Optional[GuidedC]:
    """(``keep`` holds the four arrays alive until the call returns)"""
    if ta is None:
        return None
    def arr(values, dtype):  # (one element at least, so the pointer is never NULL; NumPy: no Python int per edge)
        a = np.ascontiguousarray(values, dtype) if len(values) else np.zeros(1, dtype)
        keep.append(a)
        return a

    acc = arr(np.asarray(ta.accepting, np.int64) != 0, np.uint8)
    rp, tk, nx = arr(ta.row_ptr, np.int32), arr(ta.edge_tok, np.int32), arr(ta.edge_next, np.int32)
    return GuidedC(ta.n_states, ta.start, acc.ctypes.data_as(C.POINTER(C.c_uint8)), rp.ctypes.data_as(C.POINTER(C.c_int32)),
                   tk.ctypes.data_as(C.POINTER(C.c_int32)), nx.ctypes.data_as(C.POINTER(C.c_int32)))


@dataclass
class VisionSettings:
    base_size: int = 1024
    image_size: int = 640
    crop_mode: bool = True


@dataclass
class DecodeParameters:
    """DecodeParameters::default (inference.rs:65-79)."""
    max_new_tokens: int = 512
    do_sample: bool = False
    temperature: float = 0.0
    top_p: Optional[float] = 1.0
    top_k: Optional[int] = None
    repetition_penalty: float = 1.0
    no_repeat_ngram_size: Optional[int] = 20
    seed: Optional[int] = None
    use_cache: bool = True


@dataclass
class DecodeOutcome:
    text: str
    prompt_tokens: int
    response_tokens: int
    generated_tokens: list = field(default_factory=list)
    # decode(..., logprobs=K): one log-probability per generated token, and per token its K most likely
    # alternatives as (id, logprob), most likely first
    token_logprobs: Optional[list] = None
    top_logprobs: Optional[list] = None
    # decode(..., stop=... / stop_token_ids=...): the matched stop string or token id; None when EOS or the length
    # limit ended the request (and for a request without stops)
    stop_reason: Any = None
    # decode(..., guided=...): "complete" (the automaton reached a terminal state), "violated", or None
    guided_status: Optional[str] = None


@dataclass
class ModelLoadArgs:
    kind: str = "deepseek"
    config_path: Optional[str] = None
    weights_path: Optional[str] = None   # None -> deterministic synthetic checkpoint
    snapshot_path: Optional[str] = None
    # MoE experts decoded from the snapshot's packed Q4_K / Q8_0 blocks at 1..8 decode tokens
    # (DSOCR_LOAD_PACKED_EXPERTS): None = dsocr_engine_load (the DSOCR_DSQ_PACKED environment switch decides),
    # True / False = dsocr_engine_load_flags
    snapshot_packed: Optional[bool] = None
    device: int = 0
    dtype: str = "f16"
    synthetic_seed: int = 0


def render_prompt(template: str, system_prompt: str, raw_prompt: str) -> str:
    """Only the `plain` template (the CLI default, config.rs:209-221): message trimmed, empty separators."""
    if template != "plain":
        raise ValueError(f"unknown conversation template {template}")
    return raw_prompt.strip()


def normalize_text(s: str) -> str:
    return s.replace("\r\n", "\n").replace("<｜end▁of▁sentence｜>", "").strip()


def _encode(tokenizer, text: str) -> list:
    enc = tokenizer.encode(text, add_special_tokens=False)
    return list(enc.ids) if hasattr(enc, "ids") else list(enc)


def build_prompt_tokens(tokenizer, prompt: str, image_token_counts: Sequence[int]):
    """model/mod.rs:2536-2603: [BOS=0] + encode(segment) + <image> x count per image; mask marks slots."""
    image_token_id = tokenizer.token_to_id("<image>")
    if image_token_id is None:
        raise DsocrError(1, "tokenizer missing <image> token")
    segments = prompt.split("<image>")
    if len(segments) - 1 != len(image_token_counts):
        raise DsocrError(1, f"prompt formatting failed: prompt/image embedding mismatch: {len(segments) - 1} slots vs "
                            f"{len(image_token_counts)} embeddings")
    ids, mask = [0], [0]
    for i, seg in enumerate(segments):
        t = _encode(tokenizer, seg)
        ids += t
        mask += [0] * len(t)
        if i < len(image_token_counts):
            ids += [int(image_token_id)] * int(image_token_counts[i])
            mask += [1] * int(image_token_counts[i])
    return ids, mask


class Page:
    """Preprocessed page pixels (a1-a3): global view + crop tiles.

    ``engine=None``: host C++ (dsocr_prepare_page_variant); with an engine: on that engine's GPU
    (dsocr_prepare_page_device_variant, bit-identical pixels, device-resident).  ``variant`` (0 = DeepSeek-OCR,
    1 = DeepSeek-OCR-2) sets the tile budget and the <image> slot layout; it defaults to the engine's when one is
    given and to 0 otherwise."""

    def __init__(self, rgb, vision: VisionSettings, engine=None, variant=None):
        if hasattr(rgb, "convert"):  # PIL image
            rgb = np.asarray(rgb.convert("RGB"))
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise DsocrError(1, "page must be HxWx3 uint8")
        vs = VisionSettingsC(vision.base_size, vision.image_size, 1 if vision.crop_mode else 0)
        h = C.c_void_p()
        if variant is None:
            variant = engine.variant if engine is not None else 0
        if engine is None:
            check(lib().dsocr_prepare_page_variant(rgb.ctypes.data_as(C.c_void_p), rgb.shape[1], rgb.shape[0],
                                                   C.byref(vs), int(variant), C.byref(h)))
        elif int(variant) == engine.variant:
            check(lib().dsocr_prepare_page_device_variant(engine._h, rgb.ctypes.data_as(C.c_void_p), rgb.shape[1],
                                                          rgb.shape[0], C.byref(vs), C.byref(h)))
        elif int(variant) == 0:
            check(lib().dsocr_prepare_page_device(engine._h, rgb.ctypes.data_as(C.c_void_p), rgb.shape[1],
                                                  rgb.shape[0], C.byref(vs), C.byref(h)))
        else:
            raise DsocrError(1, f"engine of variant {engine.variant} cannot prepare a page of variant {variant}")
        self.variant = int(variant)
        self.on_device = engine is not None
        self._h = h
        cw, ch, nt, ntok = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_size_t()
        check(lib().dsocr_page_info(h, C.byref(cw), C.byref(ch), C.byref(nt), C.byref(ntok)))
        self.crop_shape = (cw.value, ch.value)
        self.n_tiles = nt.value
        self.n_image_tokens = ntok.value

    def to_device(self, engine) -> "Page":
        """Stage the pixels in the engine's HBM (dsocr_page_to_device); returns self."""
        check(lib().dsocr_page_to_device(engine._h, self._h))
        return self

    def pixels(self):
        g, gs, t, ts = C.c_void_p(), C.c_uint32(), C.c_void_p(), C.c_uint32()
        check(lib().dsocr_page_pixels_view(self._h, C.byref(g), C.byref(gs), C.byref(t), C.byref(ts)))
        if self.on_device:
            glob = np.empty((3, gs.value, gs.value), np.float32)
            tiles = np.empty((self.n_tiles, 3, ts.value, ts.value), np.float32) if self.n_tiles else None
            check(lib().dsocr_page_read_device(self._h, glob.ctypes.data_as(C.c_void_p),
                                               tiles.ctypes.data_as(C.c_void_p) if tiles is not None else None))
            return glob, tiles
        glob = np.ctypeslib.as_array(C.cast(g, C.POINTER(C.c_float)), (3, gs.value, gs.value)).copy()
        tiles = None
        if self.n_tiles:
            tiles = np.ctypeslib.as_array(C.cast(t, C.POINTER(C.c_float)),
                                          (self.n_tiles, 3, ts.value, ts.value)).copy()
        return glob, tiles

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().dsocr_page_free(self._h)
                self._h = None
        except Exception:
            pass


def _params_c(p: DecodeParameters, eos: int, ignore_eos: bool) -> DecodeParamsC:
    return DecodeParamsC(max_new_tokens=p.max_new_tokens, do_sample=1 if p.do_sample else 0,
                         temperature=p.temperature, top_p=p.top_p if p.top_p is not None else -1.0,
                         top_k=p.top_k or 0, repetition_penalty=p.repetition_penalty,
                         no_repeat_ngram_size=p.no_repeat_ngram_size or 0, seed=p.seed or 0,
                         use_cache=1 if p.use_cache else 0, eos_token_id=eos, ignore_eos=1 if ignore_eos else 0,
                         has_seed=0 if p.seed is None else 1)


# ---------------------------------------------------------------------- what the generate* methods marshal with
# (a new per-request feature adds its record here: a `_x_c` like `_stop_c` / `_bias_c`, passed through `_ptr_array`)
def _check_top_k(top_k) -> None:
    if top_k is not None and not 0 <= int(top_k) <= MAX_TOP_LOGPROBS:
        raise DsocrError(1, f"top_k must be 0..{MAX_TOP_LOGPROBS}")


def _ptr_array(T, recs, keep):
    """``POINTER(T) * n`` over a list of optional records (None: a NULL entry)."""
    keep.append(recs)
    return (C.POINTER(T) * len(recs))(*[C.pointer(r) if r is not None else C.POINTER(T)() for r in recs])


def _stream_cb(stream: Optional[Callable]):
    """The C callback of ``stream(n, tokens)`` (None: a NULL one)."""
    return STREAM_CB(lambda k, toks, _u: stream(k, [toks[i] for i in range(k)])) if stream else STREAM_CB()


class _Batch:
    """The ``RequestC`` and ``ResultC`` arrays of a batch call over ``requests`` (each ``(ids, mask, page_or_None,
    image_rows_or_None)``), with room for ``cap`` ids per page; ``keep`` holds what the arrays point into."""

    def __init__(self, engine, requests, params):
        self.keep = []
        self.n, self.cap = len(requests), max(params.max_new_tokens, 1)
        self.reqs = (RequestC * self.n)(*[engine._request(*r, self.keep) for r in requests])
        self._outs = [np.empty(self.cap, np.int64) for _ in requests]
        self.res = (ResultC * self.n)(*[ResultC(o.ctypes.data_as(C.POINTER(C.c_int64)), len(o), 0, 0)
                                        for o in self._outs])

    def ids(self) -> list:
        """The ids per page, after the call."""
        return [self._outs[i][:self.res[i].n_out].tolist() for i in range(self.n)]


class _LogprobBuffers:
    """The log-probability buffers of ``n`` pages (``cap`` entries of ``k`` alternatives each) and their ``LogprobsC``
    array ``c``."""

    def __init__(self, n: int, cap: int, k: int):
        self.k = k
        self._tlp = [np.zeros(cap, np.float32) for _ in range(n)]
        self._tid = [np.zeros((cap, max(k, 1)), np.int64) for _ in range(n)]
        self._tl = [np.zeros((cap, max(k, 1)), np.float32) for _ in range(n)]
        self.c = (LogprobsC * n)(*[LogprobsC(self._tlp[i].ctypes.data_as(C.POINTER(C.c_float)),
                                             self._tid[i].ctypes.data_as(C.POINTER(C.c_int64)),
                                             self._tl[i].ctypes.data_as(C.POINTER(C.c_float)), cap, 0)
                                   for i in range(n)])

    def unpack(self) -> tuple:
        """After the call, per page: (token log-probabilities float32 [n_out], alternative ids int64 [n_out][k], their
        log-probabilities float32 [n_out][k])."""
        k, cnt = self.k, [int(r.n) for r in self.c]
        return ([a[:m].copy() for a, m in zip(self._tlp, cnt)],
                [a.reshape(-1)[:m * k].reshape(m, k).copy() for a, m in zip(self._tid, cnt)],
                [a.reshape(-1)[:m * k].reshape(m, k).copy() for a, m in zip(self._tl, cnt)])


class DeepseekOcrEngine:
    """OcrEngine implementation backed by the MI355X engine (one per GPU)."""

    def __init__(self, args: ModelLoadArgs):
        if args.kind != "deepseek":
            raise DsocrError(1, f"ModelKind::{args.kind} cannot be loaded by the Deepseek engine")
        if args.config_path is None:
            raise DsocrError(1, "config_path is required")
        la = LoadArgs(args.config_path.encode(), args.weights_path.encode() if args.weights_path else None,
                      args.snapshot_path.encode() if args.snapshot_path else None, args.device, DTYPES[args.dtype],
                      args.synthetic_seed)
        h = C.c_void_p()
        if args.snapshot_packed is None:
            check(lib().dsocr_engine_load(C.byref(la), C.byref(h)))
        else:
            check(lib().dsocr_engine_load_flags(C.byref(la), LOAD_PACKED_EXPERTS if args.snapshot_packed else 0,
                                                C.byref(h)))
        self._h = h
        self.args = args
        hid, voc, eos, nl = C.c_size_t(), C.c_size_t(), C.c_int64(), C.c_size_t()
        check(lib().dsocr_engine_info(h, C.byref(hid), C.byref(voc), C.byref(eos), C.byref(nl)))
        self.hidden, self.vocab, self.eos_token_id, self.num_layers = hid.value, voc.value, eos.value, nl.value
        var = C.c_int()
        check(lib().dsocr_engine_variant(h, C.byref(var)))
        self.variant = var.value  # 0 = DeepSeek-OCR, 1 = DeepSeek-OCR-2

    def packed_info(self) -> dict:
        """MoE layers decoding from packed snapshot blocks: {"packed_layers", "moe_layers", "packed_bytes"}."""
        pl, ml, pb = C.c_size_t(), C.c_size_t(), C.c_size_t()
        check(lib().dsocr_engine_packed_info(self._h, C.byref(pl), C.byref(ml), C.byref(pb)))
        return {"packed_layers": pl.value, "moe_layers": ml.value, "packed_bytes": pb.value}

    # OcrEngine accessors (inference.rs:189-198)
    def kind(self):
        return "deepseek"

    def device(self):
        return f"hip:{self.args.device}"

    def dtype(self):
        return self.args.dtype

    def weights_path(self):
        return self.args.weights_path

    def flash_attention_enabled(self):
        return True

    def close(self):
        if getattr(self, "_h", None):
            lib().dsocr_engine_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ lower seams
    def image_embeddings(self, pages: Sequence[Page]):
        n = len(pages)
        arr = (C.c_void_p * n)(*[p._h for p in pages])
        cap = sum(p.n_image_tokens for p in pages)
        out = np.empty((max(cap, 1), self.hidden), np.float32)
        rows = (C.c_size_t * n)()
        check(lib().dsocr_image_embeddings(self._h, arr, n, out.ctypes.data_as(C.c_void_p), cap, rows))
        res, off = [], 0
        for i in range(n):
            res.append(out[off:off + rows[i]].copy())
            off += rows[i]
        return res

    def _request(self, ids, mask, page, image_rows, keep):
        ids = np.ascontiguousarray(ids, np.int64)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        rows = None if image_rows is None else np.ascontiguousarray(image_rows, np.float32)
        keep += [ids, m, rows]
        return RequestC(ids.ctypes.data_as(C.POINTER(C.c_int64)),
                        None if m is None else m.ctypes.data_as(C.POINTER(C.c_uint8)), len(ids),
                        page._h if page is not None else None,
                        None if rows is None else rows.ctypes.data_as(C.POINTER(C.c_float)),
                        0 if rows is None else rows.shape[0])

    def generate(self, ids, mask=None, page: Optional[Page] = None, image_rows=None,
                 params: DecodeParameters = DecodeParameters(), stream: Optional[Callable] = None,
                 ignore_eos: bool = False):
        keep = []
        req = self._request(ids, mask, page, image_rows, keep)
        pc = _params_c(params, self.eos_token_id, ignore_eos)
        out = np.empty(max(params.max_new_tokens, 1), np.int64)
        n = C.c_size_t()
        cb = _stream_cb(stream)
        check(lib().dsocr_generate(self._h, C.byref(req), C.byref(pc), cb, None, out.ctypes.data_as(C.c_void_p),
                                   len(out), C.byref(n)))
        return out[:n.value].tolist()

    def generate_batch(self, requests, params: DecodeParameters = DecodeParameters(), ignore_eos: bool = False):
        """requests: list of (ids, mask, page_or_None, image_rows_or_None)."""
        b = _Batch(self, requests, params)
        pc = _params_c(params, self.eos_token_id, ignore_eos)
        check(lib().dsocr_generate_batch(self._h, b.n, b.reqs, C.byref(pc), b.res))
        return b.ids()

    def generate_trace(self, requests, params: DecodeParameters = DecodeParameters(), ignore_eos: bool = False):
        """generate_batch + the raw logits of every step (dsocr_generate_trace): returns
        (ids per page, logits [n][max_new][vocab] float32; rows past a page's last token are 0)."""
        b = _Batch(self, requests, params)
        logits = np.zeros((b.n, b.cap, self.vocab), np.float32)
        pc = _params_c(params, self.eos_token_id, ignore_eos)
        check(lib().dsocr_generate_trace(self._h, b.n, b.reqs, C.byref(pc), b.res,
                                         logits.ctypes.data_as(C.c_void_p), logits.size))
        return b.ids(), logits

    def generate_logprobs(self, requests, top_k: int = 0, params: DecodeParameters = DecodeParameters(),
                          ignore_eos: bool = False):
        """generate_batch + per-token log-probabilities (dsocr_generate_logprobs): returns (ids per page,
        token log-probabilities per page float32 [n_out], alternative ids per page int64 [n_out][top_k], their
        log-probabilities float32 [n_out][top_k])."""
        _check_top_k(int(top_k))
        b = _Batch(self, requests, params)
        lp = _LogprobBuffers(b.n, b.cap, int(top_k))
        pc = _params_c(params, self.eos_token_id, ignore_eos)
        check(lib().dsocr_generate_logprobs(self._h, b.n, b.reqs, C.byref(pc), b.res, lp.k, lp.c))
        return (b.ids(), *lp.unpack())

    _NA = object()  # _generate_controls: a list the C form does not take

    def _generate_controls(self, fn, mismatch, requests, params, ignore_eos, top_k, constraints, stop_sets=_NA,
                           penalties=_NA, ngram_windows=_NA, automata=_NA):
        """What the generate_* control methods share.  ``fn``: the C entry point; its arguments behind the results are
        the lists it takes, in the order [automata, guided results, ngram_windows, penalties, stop_sets, stop hits,
        constraints], then top_k and the log-probability buffers.  A list is one record (or None) per request, None
        for a NULL list; the first one ``fn`` takes is the method's own and is required.  Returns the ids per page,
        then the stop hits and the automaton results where ``fn`` has them, then the log-probability lists with
        ``top_k``; the ids alone when that is all."""
        na, vocab = self._NA, self.vocab
        taken = [x for x in (automata, ngram_windows, penalties, stop_sets, constraints) if x is not na]
        if len(taken[0]) != len(requests) or any(x is not None and len(x) != len(requests) for x in taken[1:]):
            raise DsocrError(1, mismatch)
        _check_top_k(top_k)
        b = _Batch(self, requests, params)
        hits = None if stop_sets is na else (StopHitC * b.n)()
        gres = None if automata is na else (GuidedResultC * b.n)()
        args = []
        for recs, T, conv, result in ((automata, GuidedC, lambda a, keep: _guided_c(_guided(a, vocab), keep), gres),
                                      (ngram_windows, NgramWindowC,
                                       lambda w, keep: _ngram_window_c(_ngram_window(w, vocab), keep), None),
                                      (penalties, PenaltiesC, lambda pn, keep: _penalties_c(pn), None),
                                      (stop_sets, StopSetC, _stop_c, hits),
                                      (constraints, LogitBiasC, _bias_c, None)):
            if recs is not na:
                args.append(None if recs is None else _ptr_array(T, [conv(r, b.keep) for r in recs], b.keep))
                args += [] if result is None else [result]
        lp = None if top_k is None else _LogprobBuffers(b.n, b.cap, int(top_k))
        pc = _params_c(params, self.eos_token_id, ignore_eos)
        check(fn(self._h, b.n, b.reqs, C.byref(pc), b.res, *args, lp.k if lp else 0, lp.c if lp else None))
        got = [b.ids()]
        if hits is not None:
            got.append([(int(h.seq), int(h.match_len)) for h in hits])
        if gres is not None:
            got.append([(int(g.state), int(g.status)) for g in gres])
        if lp:
            got += lp.unpack()
        return tuple(got) if len(got) > 1 else got[0]

    def generate_constrained(self, requests, constraints, params: DecodeParameters = DecodeParameters(),
                             ignore_eos: bool = False, top_k: Optional[int] = None):
        """generate_batch with one constraint per request (dsocr_generate_logit_bias): ``constraints[i]`` is a
        ``LogitConstraint`` (``dsocr.constraint.merge_constraint``) or None.  Returns the ids per page; with
        ``top_k`` (0..20) the tuple ``generate_logprobs`` returns, of the constrained distribution."""
        return self._generate_controls(lib().dsocr_generate_logit_bias, "one constraint (or None) per request", requests,
                                       params, ignore_eos, top_k, constraints)

    def generate_stops(self, requests, stop_sets, params: DecodeParameters = DecodeParameters(), ignore_eos: bool = False,
                       top_k: Optional[int] = None, constraints=None):
        """generate_batch with one stop set per request (dsocr_generate_stop): ``stop_sets[i]`` is a ``StopSet``
        (``dsocr.stops.merge_stops``) or None, ``constraints`` likewise (or None for none).  Returns ``(ids, hits)``:
        the ids per page, matched tokens included (the device never trims), and per page ``(seq, match_len)`` with
        ``seq = -1`` when no stop fired; with ``top_k`` (0..20) followed by the three lists ``generate_logprobs``
        returns."""
        return self._generate_controls(lib().dsocr_generate_stop, "one stop set (or None) per request", requests, params,
                                       ignore_eos, top_k, constraints, stop_sets)

    def generate_penalties(self, requests, penalties, params: DecodeParameters = DecodeParameters(),
                           ignore_eos: bool = False, top_k: Optional[int] = None, constraints=None, stop_sets=None):
        """generate_batch with one penalty record per request (dsocr_generate_penalties): ``penalties[i]`` is a
        ``dsocr.penalties.Penalties`` or None; ``constraints`` and ``stop_sets`` likewise (or None for none).  Returns
        what ``generate_stops`` returns: ``(ids, hits)``, with ``top_k`` followed by the three log-probability lists."""
        return self._generate_controls(lib().dsocr_generate_penalties, "one penalty record (or None) per request", requests,
                                       params, ignore_eos, top_k, constraints, stop_sets, penalties)

    def generate_ngram_window(self, requests, ngram_windows, params: DecodeParameters = DecodeParameters(),
                              ignore_eos: bool = False, top_k: Optional[int] = None, constraints=None, stop_sets=None,
                              penalties=None):
        """generate_batch with one windowed n-gram ban per request (dsocr_generate_ngram_window): ``ngram_windows[i]``
        is a ``dsocr.ngram_window.NgramWindow`` or None; ``penalties``, ``constraints`` and ``stop_sets`` likewise (or
        None for none).  Returns what ``generate_penalties`` returns."""
        return self._generate_controls(lib().dsocr_generate_ngram_window, "one n-gram window record (or None) per request",
                                       requests, params, ignore_eos, top_k, constraints, stop_sets, penalties, ngram_windows)

    def generate_guided(self, requests, automata, params: DecodeParameters = DecodeParameters(),
                        ignore_eos: bool = False, top_k: Optional[int] = None, constraints=None, stop_sets=None,
                        penalties=None, ngram_windows=None):
        """generate_batch with one token automaton per request (dsocr_generate_guided): ``automata[i]`` is a
        ``dsocr.guided.TokenAutomaton`` or None; the other lists as in ``generate_ngram_window`` (or None for none).
        Returns ``(ids, stop_hits, guided)`` with ``guided[i] = (state, status)`` (status 0 running or cut, 1 complete,
        2 violated), followed by the three log-probability lists when ``top_k`` is given."""
        return self._generate_controls(lib().dsocr_generate_guided, "one token automaton (or None) per request", requests,
                                       params, ignore_eos, top_k, constraints, stop_sets, penalties, ngram_windows, automata)

    def generate_stop_stream(self, request, stop_set, params: DecodeParameters = DecodeParameters(),
                             stream: Optional[Callable] = None, ignore_eos: bool = False):
        """``generate`` (one page, its stream callback) with a stop set (dsocr_generate_stop_stream): ``(ids, (seq,
        match_len))``.  ``stream(n, tokens)`` sees the tokens as they are emitted, matched ones included."""
        keep = []
        req = self._request(*request, keep)
        pc = _params_c(params, self.eos_token_id, ignore_eos)
        out = np.empty(max(params.max_new_tokens, 1), np.int64)
        n, hit = C.c_size_t(), StopHitC()
        rec = _stop_c(stop_set, keep)
        cb = _stream_cb(stream)
        check(lib().dsocr_generate_stop_stream(self._h, C.byref(req), C.byref(pc), C.byref(rec) if rec is not None else None,
                                               cb, None, out.ctypes.data_as(C.c_void_p), len(out), C.byref(n),
                                               C.byref(hit)))
        return out[:n.value].tolist(), (int(hit.seq), int(hit.match_len))

    def stop_launches(self) -> int:
        """dec_stop_match launches of this engine so far (dsocr_stop_launches)."""
        n = C.c_size_t()
        check(lib().dsocr_stop_launches(self._h, C.byref(n)))
        return int(n.value)

    def last_timings(self) -> dict:
        t = TimingsC()
        check(lib().dsocr_last_timings(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in TimingsC._fields_}

    SPAN_KINDS = ("moe_gateup", "moe_down", "attention", "o_proj", "router")  # the last two: chain spans only

    SPAN_WAVES, SPAN_EVENTS, SPAN_CHAIN = 1, 2, 4

    def set_spans(self, mode: int):
        """In-context launch spans for the following generates (dsocr_engine_set_spans): 0 off, bit 1 wave
        spans, bit 2 HIP events around the launches inside the replayed step graph, 4 (alone) chain spans
        (every layer's gate/up, down, attention, o_proj and router launches, one fold per step)."""
        check(lib().dsocr_engine_set_spans(self._h, int(mode)))

    def spans(self) -> dict:
        """Launch spans of the last generate run with spans on: {kind: array [layers][steps][5] uint64
        (entry, exit (100 MHz wall clock), distinct experts, waves, HIP-event dispatch duration ns)};
        only the decode steps (index 1 .. steps - 1) of the layers that have the launch are non-zero."""
        k, l, st = C.c_size_t(), C.c_size_t(), C.c_size_t()
        check(lib().dsocr_engine_spans(self._h, None, 0, C.byref(k), C.byref(l), C.byref(st)))
        if st.value == 0:
            return {}
        buf = np.zeros((k.value, l.value, st.value, 5), np.uint64)
        check(lib().dsocr_engine_spans(self._h, buf.ctypes.data_as(C.c_void_p), buf.size, None, None, None))
        return {name: buf[i] for i, name in enumerate(self.SPAN_KINDS[:k.value])}

    def set_persist_stamps(self, mode: int = 1):
        """The next generate times every persistent decode launch (HIP events) and records its phase clocks."""
        check(lib().dsocr_engine_set_persist_stamps(self._h, int(mode)))

    def persist_info(self, layers: int = 0) -> dict:
        """{used, launch_us [steps], stamps [steps][256][layers][9] uint64} of the last generate
        (dsocr_engine_persist_info)."""
        used, nd, ns = C.c_int(), C.c_size_t(), C.c_size_t()
        check(lib().dsocr_engine_persist_info(self._h, C.byref(used), None, 0, C.byref(nd), None, 0, C.byref(ns)))
        d = np.zeros(nd.value, np.float64)
        st = np.zeros(ns.value, np.uint64)
        check(lib().dsocr_engine_persist_info(self._h, None, d.ctypes.data_as(C.c_void_p), d.size, None,
                                              st.ctypes.data_as(C.c_void_p), st.size, None))
        out = {"used": bool(used.value), "launch_us": d}
        if layers and st.size:
            out["stamps"] = st.reshape(-1, 256, layers, 9)
        return out

    def profile_decode(self, iters: int = 3) -> dict:
        """HIP-event timings + algorithmic bytes of the dominant decode kernels (see dsocr.h)."""
        from ._lib import DecodeProfileC
        p = DecodeProfileC()
        check(lib().dsocr_profile_decode(self._h, iters, C.byref(p)))
        out = {}
        for k in ("moe_gateup", "moe_down", "attention", "lm_head", "qkv", "o_proj", "router", "layers_step",
                  "lm_head_screened"):
            kp = getattr(p, k)
            out[k] = {"avg_us": kp.avg_us, "bytes": kp.bytes, "flops": kp.flops, "launches": kp.launches,
                      "replay_us": kp.replay_us, "ctx_us": kp.ctx_us}
        out.update(experts_touched=p.experts_touched, tokens=p.tokens, kv_len=p.kv_len,
                   moe_gateup_kernel=(p.moe_gateup_kernel or b"").decode(),
                   moe_down_kernel=(p.moe_down_kernel or b"").decode())
        return out

    # ------------------------------------------------------------------ decode sessions
    def open_session(self, slots: int, max_context: int, params: DecodeParameters = DecodeParameters(),
                     ignore_eos: bool = False, per_request: bool = False, logprobs: bool = False,
                     logit_bias: bool = False, stops: bool = False, penalties: bool = False,
                     ngram_window: bool = False, guided: bool = False) -> "Session":
        """A long-lived batch of `slots` pages (dsocr_session_open): pages are admitted and retired between bursts
        of decode steps.  `params` are the session's; params.max_new_tokens bounds a request's own.
        ``per_request`` (dsocr_session_open_ex, DSOCR_SESSION_PER_REQUEST): `params` are only the defaults and
        ``Session.admit(..., params=...)`` gives every page its own.  ``logprobs`` (DSOCR_SESSION_LOGPROBS): every
        slot keeps per-token log-probabilities (``Session.logprobs``); the exact head runs.  ``logit_bias``
        (DSOCR_SESSION_LOGIT_BIAS): every admission may carry ``logit_bias`` / ``allowed_token_ids`` /
        ``banned_token_ids``; a burst with a constrained page runs the exact head.  ``stops`` (DSOCR_SESSION_STOP):
        every admission may carry ``stop`` / ``stop_token_ids``; the step of a burst with such a page contains the
        match launch.  ``penalties`` (DSOCR_SESSION_PENALTIES): every admission may carry ``frequency_penalty`` /
        ``presence_penalty`` / ``min_p``; a burst with such a page runs the exact head.  ``ngram_window``
        (DSOCR_SESSION_NGRAM_WINDOW): every admission may carry ``ngram_window``; a burst with such a page runs the
        exact head with the window launch.  ``guided`` (DSOCR_SESSION_GUIDED): every admission may carry ``guided``,
        a token automaton; a burst with such a page runs the exact head with the mask and advance launches."""
        return Session(self, slots, max_context, params, ignore_eos, per_request, logprobs, logit_bias, stops, penalties,
                       ngram_window, guided)

    # ------------------------------------------------------------------ OcrEngine::decode
    def decode(self, tokenizer, prompt: str, images: Sequence, vision: VisionSettings,
               params: DecodeParameters, stream: Optional[Callable] = None,
               logprobs: Optional[int] = None, logit_bias=None, allowed_token_ids=None,
               banned_token_ids=None, stop=None, stop_token_ids=None,
               include_stop_in_output: bool = False, frequency_penalty=None, presence_penalty=None,
               min_p=None, ngram_window=None, guided=None) -> DecodeOutcome:
        """``guided`` (a ``dsocr.guided.TokenAutomaton``): the page may only emit what the automaton allows, and ends
        when it reaches a terminal state; ``outcome.guided_status`` is then "complete" (``stream`` is not called).
        ``ngram_window`` (a ``dsocr.ngram_window.NgramWindow``): the windowed no-repeat n-gram ban with its
        whitelist, which replaces the plain ``no_repeat_ngram_size`` ban of ``params`` for this page (``stream`` is not
        called).
        ``frequency_penalty`` / ``presence_penalty`` lower the logit of every id the page has already generated
        (by ``frequency * count + presence``; prompt and image slots do not count) and ``min_p`` keeps, when sampling,
        only tokens at least ``min_p`` times as likely as the most likely one (``dsocr.penalties``; ``stream`` is not
        called).
        ``stop`` (a string or a list of strings) and ``stop_token_ids`` end the page on the step that completes one
        of them (merged by ``dsocr.stops.merge_stops``).  ``stream`` is called live, with every token as it is
        emitted, matched ones included (dsocr_generate_stop_stream: ``dsocr.stops.TokenHoldback`` tells a consumer
        what is safe to show); together with ``logprobs`` or a constraint it is not called (dsocr_generate_stop).  The matched tokens are trimmed from the ids, the text and the log-probability
        entries unless ``include_stop_in_output``; a stop string the token match cannot see (another tokenisation)
        cuts the text on the host.  ``outcome.stop_reason`` names the stop that fired.
        ``logprobs`` = K (0..20): the outcome carries every token's log-probability and its K most likely
        alternatives (``stream`` is then not called: the entries arrive with the ids).
        ``logit_bias`` ({id: value}), ``allowed_token_ids`` and ``banned_token_ids`` constrain the tokens the page
        may emit (merged by ``dsocr.constraint.merge_constraint``; ``stream`` is not called either)."""
        con = _constraint(logit_bias, allowed_token_ids, banned_token_ids, self.vocab)
        ss = _stops(stop, stop_token_ids, tokenizer, self.vocab)
        pen = _penalties(frequency_penalty, presence_penalty, min_p)
        ngw = _ngram_window(ngram_window, self.vocab)
        gd = _guided(guided, self.vocab)
        pages = [Page(im, vision, self) for im in images]
        ids, mask = build_prompt_tokens(tokenizer, prompt, [p.n_image_tokens for p in pages])
        token_lp = top = None
        if logprobs is not None or con is not None or ss is not None or pen is not None or ngw is not None or gd is not None:
            rows = np.concatenate(self.image_embeddings(pages), axis=0) if len(pages) > 1 else None
            req = (ids, mask, pages[0] if len(pages) == 1 else None, rows)
        if ss is not None or pen is not None or ngw is not None or gd is not None:
            guided_status = None
            if gd is not None:
                got = self.generate_guided([req], [gd], params, top_k=None if logprobs is None else int(logprobs),
                                           constraints=None if con is None else [con],
                                           stop_sets=None if ss is None else [ss],
                                           penalties=None if pen is None else [pen],
                                           ngram_windows=None if ngw is None else [ngw])
                guided_status = STATUS_NAMES.get(got[2][0][1])
                got = (got[0], got[1], *got[3:])
            elif ngw is not None:
                got = self.generate_ngram_window([req], [ngw], params, top_k=None if logprobs is None else int(logprobs),
                                                 constraints=None if con is None else [con],
                                                 stop_sets=None if ss is None else [ss],
                                                 penalties=None if pen is None else [pen])
            elif pen is not None:
                got = self.generate_penalties([req], [pen], params, top_k=None if logprobs is None else int(logprobs),
                                              constraints=None if con is None else [con],
                                              stop_sets=None if ss is None else [ss])
            elif stream is not None and logprobs is None and con is None:
                # live: the callback sees every token as it is emitted, matched ones included (the caller holds back)
                got = self.generate_stop_stream(req, ss, params, stream)
                got = ([got[0]], [got[1]])
            else:
                got = self.generate_stops([req], [ss], params, top_k=None if logprobs is None else int(logprobs),
                                          constraints=None if con is None else [con])
            gen, (hit_seq, match_len) = got[0][0], got[1][0]
            res = apply_stops(lambda t: _decode_tokens(tokenizer, t), gen, ss, hit_seq, match_len, include_stop_in_output)
            if logprobs is not None:
                token_lp = [float(x) for x in got[2][0]][:len(res.tokens)]
                top = [[(int(i), float(v)) for i, v in zip(got[3][0][t], got[4][0][t])] for t in range(len(token_lp))]
            return DecodeOutcome(normalize_text(res.text), len(ids), len(res.tokens), res.tokens, token_lp, top,
                                 res.stop_reason, guided_status)
        if con is not None and logprobs is None:
            gen = self.generate_constrained([req], [con], params)[0]
        elif logprobs is not None:
            if con is not None:
                g, lp, ti, tl = self.generate_constrained([req], [con], params, top_k=int(logprobs))
            else:
                g, lp, ti, tl = self.generate_logprobs([req], int(logprobs), params)
            gen = g[0]
            token_lp = [float(x) for x in lp[0]]
            top = [[(int(i), float(v)) for i, v in zip(ti[0][t], tl[0][t])] for t in range(len(token_lp))]
        elif len(pages) > 1:
            # several <image> slots: the pages' rows in image order (compute_image_embeddings over the
            # list, model/mod.rs:2387), injected at the mask positions in that order
            rows = np.concatenate(self.image_embeddings(pages), axis=0)
            gen = self.generate(ids, mask, None, rows, params, stream)
        else:
            gen = self.generate(ids, mask, pages[0] if pages else None, None, params, stream)
        text = ""
        if hasattr(tokenizer, "decode"):
            try:
                text = tokenizer.decode([int(t) for t in gen], skip_special_tokens=True)
            except TypeError:
                text = tokenizer.decode([int(t) for t in gen])
        return DecodeOutcome(normalize_text(text), len(ids), len(gen), gen, token_lp, top)


def _decode_tokens(tokenizer, toks) -> str:
    if not hasattr(tokenizer, "decode"):
        return ""
    try:
        return tokenizer.decode([int(t) for t in toks], skip_special_tokens=True)
    except TypeError:
        return tokenizer.decode([int(t) for t in toks])


@dataclass
class SlotStatus:
    slot: int
    done: bool
    out_len: int
    new_tokens: list


class Session:
    """One decode session of an engine (include/dsocr.h, "decode sessions").  Active pages occupy slots
    [0, active); ``retire`` returns (ids, moved_from): the last active page moves into the freed slot."""

    def __init__(self, engine: DeepseekOcrEngine, slots: int, max_context: int, params: DecodeParameters,
                 ignore_eos: bool = False, per_request: bool = False, logprobs: bool = False, logit_bias: bool = False,
                 stops: bool = False, penalties: bool = False, ngram_window: bool = False, guided: bool = False):
        self._e = None
        # the (StopSet, include) record of an admission follows its page: staged for the C call that admits it,
        # pending while a chunked admission runs, then its slot's
        self._staged_stops, self._pending_stops, self._slot_stops = None, None, {}
        self._pending_page = None  # the page of the pending chunked admission (the engine reads its pixels)
        pc = _params_c(params, engine.eos_token_id, ignore_eos)
        flags = ((SESSION_PER_REQUEST if per_request else 0) | (SESSION_LOGPROBS if logprobs else 0) |
                 (SESSION_LOGIT_BIAS if logit_bias else 0) | (SESSION_STOP if stops else 0) |
                 (SESSION_PENALTIES if penalties else 0) | (SESSION_NGRAM_WINDOW if ngram_window else 0) |
                 (SESSION_GUIDED if guided else 0))
        self.has_guided = bool(guided)
        self.has_ngram_window = bool(ngram_window)
        self.has_penalties = bool(penalties)
        self.has_stops = bool(stops)
        self.has_logprobs = bool(logprobs)
        self.has_logit_bias = bool(logit_bias)
        if flags:
            check(lib().dsocr_session_open_ex(engine._h, int(slots), int(max_context), C.byref(pc), flags))
        else:
            check(lib().dsocr_session_open(engine._h, int(slots), int(max_context), C.byref(pc)))
        self._e = engine
        self.params = params
        self.per_request = bool(per_request)
        self._eos, self._ignore_eos = engine.eos_token_id, bool(ignore_eos)
        d = self.info()
        self.slots, self.max_context, self.out_cap = d["slots"], d["max_context"], d["out_cap"]
        self.kv_cap, self.burst_cap = d["kv_cap"], d["burst_cap"]
        self._status = (SlotStatusC * self.slots)()
        self._tokens = np.empty(max(self.slots * self.out_cap, 1), np.int64)

    def info(self) -> dict:
        d = SessionDescC()
        check(lib().dsocr_session_info(self._e._h, C.byref(d)))
        return {k: int(getattr(d, k)) for k, _ in SessionDescC._fields_}

    def admit(self, ids, mask=None, page: Optional[Page] = None, image_rows=None,
              max_new_tokens: Optional[int] = None, seed: Optional[int] = None,
              params: Optional[DecodeParameters] = None, eos_token_id: Optional[int] = None,
              ignore_eos: Optional[bool] = None, logprobs: Optional[int] = None, logit_bias=None,
              allowed_token_ids=None, banned_token_ids=None, stop=None, stop_token_ids=None,
              include_stop_in_output: bool = False, tokenizer=None, stops: Optional[StopSet] = None,
              frequency_penalty=None, presence_penalty=None, min_p=None, ngram_window=None, guided=None) -> int:
        """Without ``params``: the session's parameters with this page's ``max_new_tokens`` / ``seed``
        (dsocr_session_admit).  With ``params``: the page's whole parameter set (dsocr_session_admit_params; its
        max_new_tokens and seed count, the two keyword arguments are then not read); ``eos_token_id`` /
        ``ignore_eos`` default to what the session was opened with.  ``logprobs`` (0..20) is a check only, it changes
        nothing on the device: a session opened with ``logprobs`` keeps 20 alternatives for every slot whatever is
        passed here, and ``Session.logprobs(..., top_k)`` decides how many are read.  Passing it states that the
        page's entries will be read, and is an error (EINVAL) on a session opened without ``logprobs``.
        ``logit_bias`` / ``allowed_token_ids`` / ``banned_token_ids``: the page's constraint (a session opened with
        ``logit_bias``; EINVAL otherwise), applied from its first token on.
        ``stop`` / ``stop_token_ids`` (or ``stops``, a ``StopSet`` merged elsewhere): the page's stop set (a session
        opened with ``stops``; EINVAL otherwise), matched from its first token on; a stop string needs ``tokenizer``.
        The session returns ids as the device wrote them, matched tokens included: ``stop_hit(slot)`` names the hit
        and ``retire_stopped`` trims by it unless ``include_stop_in_output``.
        ``frequency_penalty`` / ``presence_penalty`` / ``min_p``: the page's penalties (a session opened with
        ``penalties``; EINVAL otherwise), applied from its first token on; ``min_p`` acts on a sampled page only.
        ``ngram_window``: the page's windowed n-gram ban (a session opened with ``ngram_window``; EINVAL otherwise),
        which replaces its plain ``no_repeat_ngram_size`` ban."""
        req, _, _keep = self._admission((ids, mask, page, image_rows), None, logprobs,
                                        (logit_bias, allowed_token_ids, banned_token_ids),
                                        (stop, stop_token_ids, include_stop_in_output, tokenizer, stops),
                                        (frequency_penalty, presence_penalty, min_p), ngram_window, guided)
        slot = C.c_int(-1)
        if params is not None:
            pc = _params_c(params, self._eos if eos_token_id is None else int(eos_token_id),
                           self._ignore_eos if ignore_eos is None else bool(ignore_eos))
            self._admission_call(lib().dsocr_session_admit_params, C.byref(req), C.byref(pc), C.byref(slot))
        else:
            self._admission_call(lib().dsocr_session_admit, C.byref(req),
                                 self.out_cap if max_new_tokens is None else int(max_new_tokens),
                                 0 if seed is None else 1, seed or 0, C.byref(slot))
        return self._admitted_stops(slot.value)

    def _admission(self, request, request_params, logprobs, constraint, stops, penalties=(None, None, None),
                   ngram_window=None, guided=None):
        """What every admission form does before its C call, in this order: the ``logprobs`` check, the request
        (``request``: ids, mask, page, image rows), its parameter record (``request_params``: ``_request_params``'
        arguments, or None for none), the stop set merged and checked (``stops``: ``_check_stops``' arguments), then
        the constraint staged (``constraint``: ``_stage_constraint``'s arguments) and the stop set staged; the
        penalties (``penalties``: frequency_penalty, presence_penalty, min_p) are checked with the stop set, before
        anything is staged, and staged after it; the windowed n-gram ban (``ngram_window``) likewise, staged last.  Returns
        the request, the parameter record and the list that keeps their arrays alive; the checked stop record is
        ``_staged_stops``.  The token automaton (``guided``) is checked with the others and staged after them all."""
        self._check_logprobs(logprobs)
        keep = []
        req = self._e._request(*request, keep)
        pc = None if request_params is None else self._request_params(*request_params)
        checked = self._check_stops(*stops)
        pen = self._check_penalties(*penalties)
        ngw = self._check_ngram_window(ngram_window)
        gd = self._check_guided(guided)
        self._stage_constraint(*constraint)
        self._stage_stops(checked)
        self._stage_penalties(pen)
        self._stage_ngram_window(ngw)
        self._stage_guided(gd)
        return req, pc, keep

    def _check_guided(self, guided) -> Optional[TokenAutomaton]:
        """The token automaton of an admission, checked before anything is staged for it (None: none)."""
        gd = _guided(guided, self._e.vocab)
        if gd is not None and not self.has_guided:
            raise DsocrError(1, "EINVAL: this session was opened without guided")
        return gd

    def _stage_guided(self, gd: Optional[TokenAutomaton]) -> None:
        """Stages the checked automaton for the admission call that follows (dsocr_session_stage_guided), which
        consumes it.  Should the staging itself fail, what was staged before it is cleared."""
        if gd is None:
            return
        keep = []
        rec = _guided_c(gd, keep)
        try:
            check(lib().dsocr_session_stage_guided(self._e._h, C.byref(rec)))
        except DsocrError:
            lib().dsocr_session_stage_logit_bias(self._e._h, None)
            lib().dsocr_session_stage_stop(self._e._h, None)
            lib().dsocr_session_stage_penalties(self._e._h, None)
            lib().dsocr_session_stage_ngram_window(self._e._h, None)
            self._staged_stops = None
            raise

    def guided_state(self, slot: int):
        """``(state, status)`` of a live slot's automaton (dsocr_session_guided_state): status 0 running or cut, 1
        complete, 2 violated; ``(0, 0)`` for a page without one."""
        g = GuidedResultC()
        check(lib().dsocr_session_guided_state(self._e._h, int(slot), C.byref(g)))
        return int(g.state), int(g.status)

    def _check_ngram_window(self, ngram_window) -> Optional[NgramWindow]:
        """The windowed n-gram ban of an admission, checked before anything is staged for it (None: none)."""
        ngw = _ngram_window(ngram_window, self._e.vocab)
        if ngw is not None and not self.has_ngram_window:
            raise DsocrError(1, "EINVAL: this session was opened without ngram_window")
        return ngw

    def _stage_ngram_window(self, ngw: Optional[NgramWindow]) -> None:
        """Stages the checked record for the admission call that follows (dsocr_session_stage_ngram_window), which
        consumes it.  Should the staging itself fail, what was staged before it is cleared."""
        if ngw is None:
            return
        keep = []
        rec = _ngram_window_c(ngw, keep)
        try:
            check(lib().dsocr_session_stage_ngram_window(self._e._h, C.byref(rec)))
        except DsocrError:
            lib().dsocr_session_stage_logit_bias(self._e._h, None)
            lib().dsocr_session_stage_stop(self._e._h, None)
            lib().dsocr_session_stage_penalties(self._e._h, None)
            self._staged_stops = None
            raise

    def _check_penalties(self, frequency_penalty, presence_penalty, min_p) -> Optional[Penalties]:
        """The penalties of an admission, checked before anything is staged for it (None: none)."""
        pen = _penalties(frequency_penalty, presence_penalty, min_p)
        if pen is not None and not self.has_penalties:
            raise DsocrError(1, "EINVAL: this session was opened without penalties")
        return pen

    def _stage_penalties(self, pen: Optional[Penalties]) -> None:
        """Stages the checked record for the admission call that follows (dsocr_session_stage_penalties), which
        consumes it.  Should the staging itself fail, what was staged before it is cleared: nothing staged may
        outlive a failed admission."""
        if pen is None:
            return
        rec = _penalties_c(pen)
        try:
            check(lib().dsocr_session_stage_penalties(self._e._h, C.byref(rec)))
        except DsocrError:
            lib().dsocr_session_stage_logit_bias(self._e._h, None)
            lib().dsocr_session_stage_stop(self._e._h, None)
            self._staged_stops = None
            raise

    def _admission_call(self, fn, *args) -> None:
        """The C call of an admission.  It consumes what was staged whether it succeeds or not, so after a failure
        nothing is staged here either."""
        try:
            check(fn(self._e._h, *args))
        except Exception:
            self._staged_stops = None
            raise

    def _check_stops(self, stop, stop_token_ids, include, tokenizer, stops):
        """The stop set of an admission, merged and checked before anything is staged for it: ``(StopSet, include)``
        or None.  A bad set, or a session without ``stops``, raises here, while no constraint is staged yet."""
        self._staged_stops = None
        ss = _stops(stop, stop_token_ids, tokenizer, self._e.vocab, stops)
        if ss is None:
            return None
        if not self.has_stops:
            raise DsocrError(1, "EINVAL: this session was opened without stops")
        return ss, bool(include)

    def _stage_stops(self, checked) -> None:
        """Stages the checked stop set for the admission call that follows (dsocr_session_stage_stop), which
        consumes it.  Should the staging itself fail, the constraint staged just before is cleared with it: nothing
        staged may outlive a failed admission."""
        if checked is None:
            return
        keep = []
        rec = _stop_c(checked[0], keep)
        try:
            check(lib().dsocr_session_stage_stop(self._e._h, C.byref(rec)))
        except DsocrError:
            lib().dsocr_session_stage_logit_bias(self._e._h, None)
            raise
        self._staged_stops = checked

    def _admitted_stops(self, slot: int) -> int:
        """The staged (stop set, include) record follows its page: into its slot, or with a chunked admission."""
        rec, self._staged_stops = self._staged_stops, None
        self._slot_stops.pop(slot, None)
        if rec is not None:
            self._slot_stops[slot] = rec
        return slot

    def stop_hit(self, slot: int):
        """``(seq, match_len)`` of a live slot (dsocr_session_stop_hit); ``seq = -1``: no stop fired."""
        h = StopHitC()
        check(lib().dsocr_session_stop_hit(self._e._h, int(slot), C.byref(h)))
        return int(h.seq), int(h.match_len)

    def slot_stops(self, slot: int):
        """``(StopSet, include_stop_in_output)`` the page in ``slot`` was admitted with, or None."""
        return self._slot_stops.get(int(slot))

    def retire_stopped(self, slot: int, decode: Callable):
        """``retire`` for a page admitted with stops: ``(StopResult, moved_from)`` with the matched tokens trimmed
        unless the page asked for them (``dsocr.stops.apply_stops``; ``decode(ids) -> text``)."""
        rec = self.slot_stops(slot)
        hit = self.stop_hit(slot) if rec is not None and self.has_stops else (-1, 0)
        ids, moved = self.retire(slot)
        ss, include = rec if rec is not None else (None, False)
        return apply_stops(decode, ids, ss, hit[0], hit[1], include), moved

    def _stage_constraint(self, logit_bias, allowed_token_ids, banned_token_ids) -> None:
        """The constraint of the admission call that follows (dsocr_session_stage_logit_bias): merged and checked
        here, consumed by that call."""
        con = _constraint(logit_bias, allowed_token_ids, banned_token_ids, self._e.vocab)
        if con is None:
            return
        if not self.has_logit_bias:
            raise DsocrError(1, "EINVAL: this session was opened without logit_bias")
        keep = []
        rec = _bias_c(con, keep)
        check(lib().dsocr_session_stage_logit_bias(self._e._h, C.byref(rec)))

    def _check_logprobs(self, logprobs) -> None:
        """The `logprobs` keyword of every admission: a check only (see ``admit``)."""
        if logprobs is not None:
            if not self.has_logprobs:
                raise DsocrError(1, "this session was opened without logprobs")
            if not 0 <= int(logprobs) <= MAX_TOP_LOGPROBS:
                raise DsocrError(1, f"logprobs must be 0..{MAX_TOP_LOGPROBS}")

    def _request_params(self, params, max_new_tokens, seed, eos_token_id, ignore_eos):
        """A request's whole parameter record: `params`, or the session's with this max_new_tokens / seed."""
        if params is None:
            params = DecodeParameters(**{**self.params.__dict__,
                                         "max_new_tokens": self.out_cap if max_new_tokens is None else int(max_new_tokens),
                                         "seed": seed})
        return _params_c(params, self._eos if eos_token_id is None else int(eos_token_id),
                         self._ignore_eos if ignore_eos is None else bool(ignore_eos))

    # ------------------------------------------------------------------ chunked admission
    def admit_begin(self, ids, mask=None, page: Optional[Page] = None, image_rows=None, chunk_rows: int = 128,
                    max_new_tokens: Optional[int] = None, seed: Optional[int] = None,
                    params: Optional[DecodeParameters] = None, eos_token_id: Optional[int] = None,
                    ignore_eos: Optional[bool] = None, logprobs: Optional[int] = None, logit_bias=None,
                    allowed_token_ids=None, banned_token_ids=None, stop=None, stop_token_ids=None,
                    include_stop_in_output: bool = False, tokenizer=None, stops: Optional[StopSet] = None,
                    frequency_penalty=None, presence_penalty=None, min_p=None, ngram_window=None, guided=None) -> int:
        """``admit`` in slices (dsocr_session_admit_begin): every check runs here and nothing is launched; the work
        is done by ``admit_advance``, one slice per call (the page's vision, then the prompt in chunks of
        ``chunk_rows`` >= 32 rows), with ``step`` / ``retire`` legal in between.  Returns the admission's ticket.
        The keywords are ``admit``'s.  One admission may be pending; ``admit`` / ``admit_prefix`` are refused while
        it is."""
        req, pc, _keep = self._admission((ids, mask, page, image_rows),
                                         (params, max_new_tokens, seed, eos_token_id, ignore_eos), logprobs,
                                         (logit_bias, allowed_token_ids, banned_token_ids),
                                         (stop, stop_token_ids, include_stop_in_output, tokenizer, stops),
                                         (frequency_penalty, presence_penalty, min_p), ngram_window, guided)
        self._pending_stops = None
        ticket = C.c_int(-1)
        self._admission_call(lib().dsocr_session_admit_begin, C.byref(req), C.byref(pc), max(int(chunk_rows), 0),
                             C.byref(ticket))
        self._pending_stops, self._staged_stops = self._staged_stops, None  # (admit_advance hands it to the slot)
        self._pending_page = page  # the engine reads the page's pixels in the vision slice
        return ticket.value

    def admit_advance(self):
        """One slice of the pending admission, synchronised (dsocr_session_admit_advance): (done, slot), slot = -1
        until the last chunk has made the page active."""
        done, slot = C.c_int(0), C.c_int(-1)
        try:
            check(lib().dsocr_session_admit_advance(self._e._h, C.byref(done), C.byref(slot)))
        except DsocrError:
            if not self.admit_progress()["pending"]:
                self._pending_page = None
                self._pending_stops = None
            raise
        if done.value:
            self._pending_page = None
            self._staged_stops, self._pending_stops = self._pending_stops, None
            self._admitted_stops(slot.value)
        return bool(done.value), slot.value

    def admit_cancel(self) -> None:
        """Drops the pending admission (dsocr_session_admit_cancel); the running slots and later admissions see
        nothing of it."""
        check(lib().dsocr_session_admit_cancel(self._e._h))
        self._pending_page = None
        self._pending_stops = None

    def admit_progress(self) -> dict:
        """{"pending", "rows_done", "rows_total", "slices", "vision_stage"} of the pending admission (all zero without
        one; vision_stage: the stage the next slice runs, 1 SAM, 2 CLIP / encoder, 3 projector, 0 none left) and
        "chunk_attn_launches", the engine's launch_attention_chunk launches so far."""
        p, st, v = C.c_int(0), C.c_int(0), [C.c_size_t() for _ in range(4)]
        check(lib().dsocr_session_admit_progress(self._e._h, C.byref(p), C.byref(v[0]), C.byref(v[1]), C.byref(v[2]),
                                                 C.byref(st), C.byref(v[3])))
        return {"pending": bool(p.value), "rows_done": int(v[0].value), "rows_total": int(v[1].value),
                "slices": int(v[2].value), "vision_stage": int(st.value), "chunk_attn_launches": int(v[3].value)}

    # ------------------------------------------------------------------ page prefix cache
    def keep_prefix(self, slot: int, rows: int) -> int:
        """K/V rows [0, rows) of a live slot's prompt into a prefix entry (dsocr_session_prefix_keep); returns its
        handle.  1 <= rows <= the slot's prompt length; the slot may have decoded any number of steps."""
        h = C.c_int(-1)
        check(lib().dsocr_session_prefix_keep(self._e._h, int(slot), int(rows), C.byref(h)))
        return h.value

    def admit_prefix(self, handle: int, ids, mask=None, max_new_tokens: Optional[int] = None,
                     seed: Optional[int] = None, params: Optional[DecodeParameters] = None,
                     eos_token_id: Optional[int] = None, ignore_eos: Optional[bool] = None,
                     logprobs: Optional[int] = None, logit_bias=None, allowed_token_ids=None,
                     banned_token_ids=None, stop=None, stop_token_ids=None, include_stop_in_output: bool = False,
                     tokenizer=None, stops: Optional[StopSet] = None, frequency_penalty=None,
                     presence_penalty=None, min_p=None, ngram_window=None, guided=None) -> int:
        """``admit`` for a prompt that starts with the entry's rows (dsocr_session_admit_prefix): ``ids`` / ``mask``
        are the whole prompt's, no page and no image rows; vision and the prefill of the entry's rows are skipped.
        The keywords are ``admit``'s (without ``params``: the session's parameters with this ``max_new_tokens`` /
        ``seed``)."""
        req, pc, _keep = self._admission((ids, mask, None, None),
                                         (params, max_new_tokens, seed, eos_token_id, ignore_eos), logprobs,
                                         (logit_bias, allowed_token_ids, banned_token_ids),
                                         (stop, stop_token_ids, include_stop_in_output, tokenizer, stops),
                                         (frequency_penalty, presence_penalty, min_p), ngram_window, guided)
        slot = C.c_int(-1)
        self._admission_call(lib().dsocr_session_admit_prefix, int(handle), C.byref(req), C.byref(pc), C.byref(slot))
        return self._admitted_stops(slot.value)

    def drop_prefix(self, handle: int) -> None:
        check(lib().dsocr_session_prefix_drop(self._e._h, int(handle)))

    def prefix_stats(self) -> dict:
        """{"entries", "bytes", "admissions", "rows_reused"} of the session's prefix entries."""
        v = [C.c_size_t() for _ in range(4)]
        check(lib().dsocr_session_prefix_stats(self._e._h, *[C.byref(x) for x in v]))
        return dict(zip(("entries", "bytes", "admissions", "rows_reused"), (int(x.value) for x in v)))

    def head_steps(self) -> dict:
        """Decode steps replayed under each lm_head + selection head since the session opened."""
        a, b = C.c_size_t(), C.c_size_t()
        check(lib().dsocr_session_head_steps(self._e._h, C.byref(a), C.byref(b)))
        return {"screened": int(a.value), "exact": int(b.value)}

    def logprobs(self, slot: int, first: int, count: int, top_k: int = 0):
        """Entries [first, first + count) of a live slot (dsocr_session_logprobs): (token log-probabilities float32
        [count], alternative ids int64 [count][top_k], their log-probabilities float32 [count][top_k]).  Read them
        before ``retire``."""
        n, k = int(count), int(top_k)
        lp = np.zeros(max(n, 1), np.float32)
        ti = np.zeros(max(n * k, 1), np.int64)
        tl = np.zeros(max(n * k, 1), np.float32)
        check(lib().dsocr_session_logprobs(self._e._h, int(slot), int(first), n, k, lp.ctypes.data_as(C.c_void_p),
                                           ti.ctypes.data_as(C.c_void_p), tl.ctypes.data_as(C.c_void_p)))
        return lp[:n], ti[:n * k].reshape(n, k), tl[:n * k].reshape(n, k)

    def _report(self, ns, nt):
        out, off = [], 0
        for i in range(ns.value):
            s = self._status[i]
            out.append(SlotStatus(s.slot, bool(s.done), s.out_len, self._tokens[off:off + s.n_new].tolist()))
            off += s.n_new
        assert off == nt.value
        return out

    def step(self, k: int = 1) -> list:
        ns, nt = C.c_size_t(), C.c_size_t()
        check(lib().dsocr_session_step(self._e._h, int(k), self._status, self.slots, C.byref(ns),
                                       self._tokens.ctypes.data_as(C.c_void_p), self._tokens.size, C.byref(nt)))
        return self._report(ns, nt)

    def poll(self) -> list:
        ns, nt = C.c_size_t(), C.c_size_t()
        check(lib().dsocr_session_poll(self._e._h, self._status, self.slots, C.byref(ns),
                                       self._tokens.ctypes.data_as(C.c_void_p), self._tokens.size, C.byref(nt)))
        return self._report(ns, nt)

    def retire(self, slot: int):
        out = np.empty(max(self.out_cap, 1), np.int64)
        n, moved = C.c_size_t(), C.c_int(-1)
        check(lib().dsocr_session_retire(self._e._h, int(slot), out.ctypes.data_as(C.c_void_p), out.size, C.byref(n),
                                         C.byref(moved)))
        recs = self._slot_stops  # the (stop set, include) records follow the compaction
        recs.pop(int(slot), None)
        if moved.value >= 0 and moved.value in recs:
            recs[int(slot)] = recs.pop(moved.value)
        return out[:n.value].tolist(), moved.value

    def close(self):
        if self._e is not None and getattr(self._e, "_h", None):
            check(lib().dsocr_session_close(self._e._h))
        self._e = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def load_model(args: ModelLoadArgs) -> DeepseekOcrEngine:
    return DeepseekOcrEngine(args)
