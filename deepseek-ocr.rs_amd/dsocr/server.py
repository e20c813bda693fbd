"""OpenAI-compatible HTTP server over the MI355X engine (`deepseek-ocr-server`).

Mirrors crates/server: routes (routes.rs:20-232: GET /v1/health, GET/OPTIONS /v1/models,
POST /v1/responses, POST /v1/chat/completions), request/response shapes (models.rs:1-145),
message flattening and image loading (generation.rs:177-313), error classes (error.rs:10-50:
400 `invalid_request_error` / 500 `internal_error`, with engine messages containing
"prompt formatting failed" / "prompt/image embedding mismatch" mapped to 400,
generation.rs:108-118), the missing-image fallback (routes.rs:240-246) and the SSE event
sequence (stream.rs:140-374).  The engine sits behind one lock (Send-not-Sync, state.rs:22)
and decodes on a worker thread (spawn_blocking, generation.rs:38-49).

Not carried over: multi-model hot swapping from the app config (one DeepSeek-OCR engine per
process/GPU here) and fetching http(s) image URLs (no network on the target boxes: such
URLs are refused with 400, like any other unsupported URL scheme in the reference).
"""

import base64
import io
import json
import queue
import threading
import time
import uuid
from dataclasses import dataclass, field, replace
from typing import Any, List, Optional, Tuple

from ._lib import DsocrError
from .engine import DecodeParameters, VisionSettings
from .streaming import DeltaTracker, decode_ids

EMPTY_GENERATION_ERROR = ("generation failed: model returned empty output (response_tokens=0 and text is empty)")

MISSING_IMAGE_MARKDOWN = (
    "⚠️ **Image Required**\n\n- This OCR backend expects at least one `<image>` placeholder or attached image.\n"
    "- Please include `input_image` / `image_url`, or add `<image>` inside the prompt.\n\n---\n\n"
    "⚠️ **需要图像输入**\n\n- 当前 OCR 模型需要至少一个 `<image>` 占位符或实际图片。\n"
    "- 请在请求中附带 `input_image`/`image_url`，或在 prompt 中插入 `<image>`。")

_PATCH_FIELDS = ("max_new_tokens", "do_sample", "temperature", "top_p", "top_k", "repetition_penalty",
                 "no_repeat_ngram_size", "seed", "use_cache")


class ApiError(Exception):
    def __init__(self, status: int, message: str):
        super().__init__(message)
        self.status = status
        self.message = message

    @staticmethod
    def bad_request(msg):
        return ApiError(400, msg)

    @staticmethod
    def internal(msg):
        return ApiError(500, msg)

    def body(self) -> dict:
        return {"error": {"message": self.message,
                          "type": "invalid_request_error" if self.status == 400 else "internal_error"}}


# ---------------------------------------------------------------- message conversion (generation.rs:177-313)
def load_image(url: str):
    """generation.rs:261-296: data: URLs (base64) only; http(s) fetching is not available offline."""
    if url.startswith("data:"):
        meta, sep, payload = url[5:].partition(",")
        if not sep:
            raise ApiError.bad_request("invalid data URL")
        if not meta.endswith(";base64"):
            raise ApiError.bad_request("data URLs must specify base64 encoding")
        try:
            raw = base64.b64decode(payload, validate=True)
        except (ValueError, TypeError) as e:
            raise ApiError.bad_request(f"invalid base64 image payload: {e}")
        from PIL import Image
        try:
            with Image.open(io.BytesIO(raw)) as im:
                return im.convert("RGB")
        except (OSError, ValueError) as e:
            raise ApiError.bad_request(f"failed to decode inline image: {e}")
    if url.startswith("http://") or url.startswith("https://"):
        raise ApiError.bad_request(f"failed to fetch {url}: remote image URLs are not available on this host")
    raise ApiError.bad_request("only data: URIs or http(s) image URLs are supported")


def _image_url(part: dict) -> str:
    v = part.get("image_url")
    if isinstance(v, dict):
        v = v.get("url")
    if not isinstance(v, str):
        raise ApiError.bad_request("image part is missing image_url")
    return v


def flatten_content(content: Any) -> Tuple[str, list]:
    """generation.rs:238-259.  Parts are visited in REVERSE order, as the reference does."""
    if content is None:
        return "", []
    if isinstance(content, str):
        return content.strip(), []
    if not isinstance(content, list):
        raise ApiError.bad_request("message content must be a string or a list of parts")
    buf, images = "", []
    for part in reversed(content):
        kind = part.get("type") if isinstance(part, dict) else None
        if kind in ("image_url", "input_image"):
            buf += "<image>"
            images.append(load_image(_image_url(part)))
        elif kind in ("text", "input_text"):
            if buf:
                buf += "\n"
            buf += str(part.get("text", ""))
        else:
            raise ApiError.bad_request(f"unsupported message part type {kind!r}")
    return buf.strip(), images


def collect_prompt_sections(messages: List[dict]) -> Tuple[List[str], list]:
    """generation.rs:193-236: system messages before the LAST user message, then that user message."""
    user_idx = None
    for i in range(len(messages) - 1, -1, -1):
        if str(messages[i].get("role", "")).lower() == "user":
            user_idx = i
            break
    if user_idx is None:
        raise ApiError.bad_request("request must include at least one user message")
    sections, images = [], []
    for m in messages[:user_idx]:
        if str(m.get("role", "")).lower() != "system":
            continue
        text, imgs = flatten_content(m.get("content"))
        if text:
            sections.append(text)
        images += imgs
    text, imgs = flatten_content(messages[user_idx].get("content"))
    if text:
        sections.append(text)
    images += imgs
    if not sections and not images:
        raise ApiError.bad_request("user content must include text or images")
    return sections, images


def convert_messages(messages: List[dict]) -> Tuple[str, list]:
    """generation.rs:177-191 (DeepSeek: sections joined by a blank line, trimmed)."""
    sections, images = collect_prompt_sections(messages)
    return "\n\n".join(sections).strip(), images


def merge_decode(defaults: DecodeParameters, req: dict, max_tokens: Optional[int]) -> DecodeParameters:
    """DecodeParameters + DecodeParametersPatch (routes.rs:79-85): max tokens first, then the
    request's flattened patch fields."""
    p = replace(defaults, max_new_tokens=max_tokens if max_tokens is not None else defaults.max_new_tokens)
    patch = {k: req[k] for k in _PATCH_FIELDS if k in req and req[k] is not None}
    return replace(p, **patch)


# ---------------------------------------------------------------- log-probabilities (chat completions)
MAX_TOP_LOGPROBS = 20
NEG_INF_LOGPROB = -9999.0  # how -inf is written (the OpenAI convention): the JSON stays valid


def parse_logprobs(req: dict) -> Optional[int]:
    """`logprobs: true|false` and `top_logprobs: 0..20` of a chat completion body: None when log-probabilities are
    not asked for, else the number of alternatives per token.  400: top_logprobs without logprobs: true, or not an
    integer in 0..20."""
    want, top = req.get("logprobs"), req.get("top_logprobs")
    if want is not None and not isinstance(want, bool):
        raise ApiError.bad_request("`logprobs` must be a boolean")
    if top is not None:
        if isinstance(top, bool) or not isinstance(top, int) or not 0 <= top <= MAX_TOP_LOGPROBS:
            raise ApiError.bad_request(f"`top_logprobs` must be an integer in 0..{MAX_TOP_LOGPROBS}")
        if not want:
            raise ApiError.bad_request("`top_logprobs` requires `logprobs: true`")
    return (top or 0) if want else None


def _id_list(req: dict, name: str, vocab: Optional[int]) -> Optional[list]:
    ids = req.get(name)
    if ids is None:
        return None
    if not isinstance(ids, list):
        raise ApiError.bad_request(f"`{name}` must be a list of token ids")
    for t in ids:
        if isinstance(t, bool) or not isinstance(t, int) or t < 0 or (vocab is not None and t >= vocab):
            raise ApiError.bad_request(f"`{name}`: {t!r} is not a token id of this model")
    return ids


def parse_token_constraint(req: dict, vocab: Optional[int] = None) -> Optional[dict]:
    """OpenAI `logit_bias` ({"<token id>": number in [-100, 100]}) and the extension fields `allowed_token_ids` /
    `banned_token_ids` (lists of token ids) of a request body, as the keywords ``decode`` / ``submit`` take; None when
    the body constrains nothing.  400: a key that is not an integer token id, an id outside the vocabulary, a value
    that is not a number in [-100, 100], a field of the wrong type, an empty allow list."""
    from .constraint import ConstraintError, merge_constraint
    raw = req.get("logit_bias")
    bias = None
    if raw is not None:
        if not isinstance(raw, dict):
            raise ApiError.bad_request("`logit_bias` must map token ids to numbers")
        bias = {}
        for k, v in raw.items():
            try:
                t = int(k) if isinstance(k, str) and k.strip().lstrip("+-").isdigit() else None
            except ValueError:
                t = None
            if isinstance(k, int) and not isinstance(k, bool):
                t = k
            if t is None or t < 0 or (vocab is not None and t >= vocab):
                raise ApiError.bad_request(f"`logit_bias`: key {k!r} is not a token id of this model")
            if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or not -100 <= v <= 100:
                raise ApiError.bad_request(f"`logit_bias`: the value of {k!r} must be a number in [-100, 100]")
            if t in bias:
                raise ApiError.bad_request(f"`logit_bias`: token id {t} is listed twice")
            bias[t] = float(v)
    allowed = _id_list(req, "allowed_token_ids", vocab)
    banned = _id_list(req, "banned_token_ids", vocab)
    try:
        con = merge_constraint(bias, allowed, banned, vocab)
    except ConstraintError as e:
        raise ApiError.bad_request(f"token constraint: {e}")
    return None if con is None else con.kwargs()


MAX_STOP_STRINGS = 4  # the OpenAI limit on `stop`


def parse_stops(req: dict, tokenizer=None, vocab: Optional[int] = None) -> Optional[dict]:
    """OpenAI `stop` (a string, or a list of at most 4 strings) and the extension fields `stop_token_ids` (a list of
    token ids) and `include_stop_in_output` (a boolean) of a request body, as the keywords ``decode`` / ``submit``
    take; None when the body names no stop (`stop: null`, an empty list).  400: anything else in those fields, an
    empty string, a string that encodes to no or to more than 32 token ids, an id outside the vocabulary, more than
    16 sequences in all."""
    from .stops import StopError, merge_stops
    stop = req.get("stop")
    if stop is not None:
        if isinstance(stop, str):
            stop = [stop]
        if not isinstance(stop, list) or any(not isinstance(x, str) for x in stop):
            raise ApiError.bad_request("`stop` must be a string or a list of strings")
        if len(stop) > MAX_STOP_STRINGS:
            raise ApiError.bad_request(f"`stop` takes at most {MAX_STOP_STRINGS} strings")
    ids = _id_list(req, "stop_token_ids", vocab)
    include = req.get("include_stop_in_output")
    if include is not None and not isinstance(include, bool):
        raise ApiError.bad_request("`include_stop_in_output` must be a boolean")
    try:
        ss = merge_stops(stop, ids, tokenizer, vocab)
    except StopError as e:
        raise ApiError.bad_request(f"stop: {e}")
    if ss is None:
        return None
    return {"stop": stop, "stop_token_ids": ids, "include_stop_in_output": bool(include)}


PENALTY_BOUND = 2.0  # OpenAI's range of `frequency_penalty` / `presence_penalty`


def parse_penalties(req: dict) -> Optional[dict]:
    """OpenAI `frequency_penalty` / `presence_penalty` (numbers in [-2, 2]) and the extension field `min_p` (a number
    in [0, 1]) of a request body, as the keywords ``decode`` / ``submit`` take; None when the body asks for nothing
    (absent, null or zero fields).  400: anything else in those fields."""
    from .penalties import PenaltyError, make_penalties
    try:
        pn = make_penalties(req.get("frequency_penalty"), req.get("presence_penalty"), req.get("min_p"),
                            bound=PENALTY_BOUND)
    except PenaltyError as e:
        raise ApiError.bad_request(f"penalties: {e}")
    if pn is None:
        return None
    return {"frequency_penalty": pn.frequency, "presence_penalty": pn.presence, "min_p": pn.min_p}


def parse_ngram_window(req: dict, vocab: Optional[int] = None) -> Optional[dict]:
    """The windowed no-repeat n-gram ban of a request body: `ngram_size`, `window_size` (100 when only `ngram_size`
    is sent, as upstream) and `whitelist_token_ids`, at top level or inside `vllm_xargs` (where the model's published
    serving recipe puts them; a top-level field wins).  Returns the keyword ``decode`` / ``submit`` take, None when the
    body asks for nothing (absent or null fields, `ngram_size` 0).  400: anything else in those fields."""
    from .ngram_window import NgramWindowError, make_ngram_window
    xargs = req.get("vllm_xargs")
    if xargs is None:
        xargs = {}
    if not isinstance(xargs, dict):
        raise ApiError.bad_request("vllm_xargs must be an object")
    got = {}
    for name in ("ngram_size", "window_size", "whitelist_token_ids"):
        v = req.get(name)
        got[name] = xargs.get(name) if v is None else v
    try:
        rec = make_ngram_window(got["ngram_size"], got["window_size"], got["whitelist_token_ids"], vocab=vocab)
    except NgramWindowError as e:
        raise ApiError.bad_request(f"ngram window: {e}")
    return None if rec is None else rec.kwargs()


def parse_guided(req: dict, tokenizer, vocab: Optional[int] = None) -> Optional[dict]:
    """Guided decoding of a request body: `guided_choice` ([str, ...]), `structured_outputs` ({"choice": [...]}) or a
    raw `token_automaton` object (n_states, start, accepting, row_ptr, edge_tok, edge_next), at top level or inside
    `vllm_xargs` (a top-level field wins).  Returns the keyword ``decode`` / ``submit`` take, None when the body asks
    for nothing (absent or null fields).  400: more than one of them, or anything else in those fields.  A guided
    decode does not stream: a streaming request gets its tokens when the page has ended."""
    from .guided import GuidedError, automaton_from_mapping, choice_automaton
    xargs = req.get("vllm_xargs")
    if xargs is None:
        xargs = {}
    if not isinstance(xargs, dict):
        raise ApiError.bad_request("vllm_xargs must be an object")
    got = {}
    for name in ("guided_choice", "structured_outputs", "token_automaton"):
        v = req.get(name)
        v = xargs.get(name) if v is None else v
        if v is not None:
            got[name] = v
    if not got:
        return None
    if len(got) > 1:
        raise ApiError.bad_request("guided decoding: give one of guided_choice, structured_outputs and token_automaton")
    try:
        if "token_automaton" in got:
            aut = automaton_from_mapping(got["token_automaton"])
        else:
            choice = got.get("guided_choice")
            if "structured_outputs" in got:
                so = got["structured_outputs"]
                if not isinstance(so, dict) or set(so) != {"choice"}:
                    raise GuidedError("structured_outputs supports {\"choice\": [...]} only")
                choice = so["choice"]
            aut = choice_automaton(tokenizer, choice)
        aut.validate(vocab if vocab else 1 << 31)
    except GuidedError as e:
        raise ApiError.bad_request(f"guided decoding: {e}")
    return {"guided": aut}


def _held_back(on_token, stops: dict, tokenizer, vocab):
    """``on_token`` behind a ``dsocr.stops.TokenHoldback``: it is called once per token that no later hit can remove."""
    from .stops import TokenHoldback, merge_stops
    ss = merge_stops(stops["stop"], stops["stop_token_ids"], tokenizer, vocab)
    hb, shown = TokenHoldback(ss.seqs, stops["include_stop_in_output"]), [0]

    def cb(n, toks):
        toks = [int(t) for t in toks[:n]]
        for j in range(shown[0] + 1, hb.feed(toks) + 1):
            shown[0] = j
            on_token(j, toks[:j])
    return cb


def _lp_json(v: float) -> float:
    return float(v) if v == v and v > float("-inf") else NEG_INF_LOGPROB


def _token_json(tokenizer, tok: int, lp: float) -> dict:
    text = decode_ids(tokenizer, [int(tok)]) if tok >= 0 else ""  # every token decoded on its own
    return {"token": text, "logprob": _lp_json(lp), "bytes": list(text.encode("utf-8"))}


def logprob_content(tokenizer, tokens, token_lp, top_lp) -> list:
    """choices[0].logprobs.content: [{token, logprob, bytes, top_logprobs: [{token, logprob, bytes}]}]."""
    out = []
    for tok, lp, top in zip(tokens, token_lp, top_lp):
        e = _token_json(tokenizer, int(tok), lp)
        e["top_logprobs"] = [_token_json(tokenizer, int(i), v) for i, v in top if i >= 0]
        out.append(e)
    return out


# ---------------------------------------------------------------- state
@dataclass
class ServerState:
    engine: Any
    tokenizer: Any
    model_id: str = "deepseek-ocr"
    vision: VisionSettings = field(default_factory=VisionSettings)
    defaults: DecodeParameters = field(default_factory=DecodeParameters)
    lock: threading.Lock = field(default_factory=threading.Lock)
    # continuous batching (scheduler.BatchScheduler over `engine`, --slots N): concurrent requests share one decode
    # session instead of queueing behind the lock.  None (the default): one request at a time
    scheduler: Any = None

    def validate_model(self, requested: str):
        if requested != self.model_id:
            raise ApiError.bad_request(f"requested model `{requested}` is not available")


def _now() -> int:
    return int(time.time())


def generate_blocking(state: ServerState, prompt: str, images: list, params: DecodeParameters, on_token=None,
                      logprobs: Optional[int] = None, constraint: Optional[dict] = None, stops: Optional[dict] = None):
    """generation.rs:75-163.  ``stops``: the keywords of parse_stops (merged into ``constraint``'s: both are keywords
    of ``decode`` / ``submit``, and a decode with either does not stream).  ``constraint``: the keywords of parse_token_constraint and of parse_penalties.  With a scheduler the request joins the running decode session (its error reaches only
    its own future); without one it decodes alone behind the lock."""
    def classify(e):
        msg = str(e)
        if "prompt formatting failed" in msg or "prompt/image embedding mismatch" in msg:
            return ApiError.bad_request(msg)
        return ApiError.internal(f"generation failed: {msg}")

    live_stops = bool(stops) and not constraint and logprobs is None and on_token is not None
    if stops:
        constraint = dict(constraint or {}, **stops)
    if state.scheduler is not None:
        try:
            kw = {} if logprobs is None else {"logprobs": logprobs}
            kw.update(constraint or {})
            outcome = state.scheduler.submit(prompt, images, state.vision, params, on_token, **kw).result()
        except DsocrError as e:
            raise classify(e)
        except ApiError:
            raise
        except Exception as e:  # noqa: BLE001 - a scheduler failure is an internal error of this request
            raise ApiError.internal(f"generation failed: {e}")
    else:
        with state.lock:
            try:
                if logprobs is None and not constraint:
                    outcome = state.engine.decode(state.tokenizer, prompt, images, state.vision, params, on_token)
                elif live_stops:  # stops alone stream live, behind the hold-back of a tail that may become a stop
                    outcome = state.engine.decode(state.tokenizer, prompt, images, state.vision, params,
                                                  _held_back(on_token, stops, state.tokenizer,
                                                             getattr(state.engine, "vocab", None)), **constraint)
                elif logprobs is None:  # a constrained decode does not stream: the tokens arrive at the end
                    outcome = state.engine.decode(state.tokenizer, prompt, images, state.vision, params, None,
                                                  **constraint)
                    toks = [int(t) for t in outcome.generated_tokens]
                    for i in range(len(toks) if on_token is not None else 0):
                        on_token(i + 1, toks[:i + 1])
                else:  # the entries arrive with the ids: a streaming consumer gets every token with its entry
                    outcome = state.engine.decode(state.tokenizer, prompt, images, state.vision, params, None,
                                                  logprobs=logprobs, **(constraint or {}))
                    toks = [int(t) for t in outcome.generated_tokens]
                    for i in range(len(toks) if on_token is not None else 0):
                        on_token(i + 1, toks[:i + 1], (outcome.token_logprobs[i], outcome.top_logprobs[i]))
            except DsocrError as e:
                raise classify(e)
    if outcome.response_tokens == 0 and not outcome.text.strip():
        raise ApiError.internal(EMPTY_GENERATION_ERROR)
    return outcome


class StreamController:
    """stream.rs:120-374: initial event, per-token deltas through DeltaTracker, final event, [DONE]."""

    def __init__(self, tokenizer, kind: str, model: str):
        self.tokenizer, self.kind, self.model = tokenizer, kind, model
        self.created = _now()
        self.q: "queue.Queue[Optional[str]]" = queue.Queue()
        self.delta = DeltaTracker()
        self.last_count = 0
        self.role_sent = False
        self.finished = False
        self.pending_lp: list = []  # entries of the tokens since the last chunk (chat, logprobs: true)
        self.text_stop = None  # dsocr.stops.TextStop of a request with stop strings: nothing of a stop is ever sent
        self.stop_reason = None
        self.has_stops = False
        if kind == "chat":
            self.id = f"chatcmpl-{uuid.uuid4()}"
        else:
            self.id = f"resp-{uuid.uuid4()}"
            self.output_id = f"msg-{uuid.uuid4()}"

    def _send(self, obj):
        self.q.put(json.dumps(obj, ensure_ascii=False))

    def _head(self):
        return {"id": self.id, "object": "response", "created": self.created, "model": self.model}

    def send_initial(self):
        if self.kind == "chat":
            self._send({"id": self.id, "object": "chat.completion.chunk", "created": self.created,
                        "model": self.model,
                        "choices": [{"index": 0, "delta": {"role": "assistant"}, "finish_reason": None}]})
            self.role_sent = True
        else:
            self._send({"type": "response.created", "response": self._head()})

    def emit_delta(self, text: str, include_role: bool):
        if self.kind == "chat":
            delta = {"content": text}
            if include_role:
                delta["role"] = "assistant"
            choice = {"index": 0, "delta": delta, "finish_reason": None}
            if self.pending_lp:  # the entries of the tokens in this chunk
                choice["logprobs"], self.pending_lp = {"content": self.pending_lp}, []
            self._send({"id": self.id, "object": "chat.completion.chunk", "created": self.created,
                        "model": self.model, "choices": [choice]})
        else:
            self._send({"type": "response.output_text.delta", "response": self._head(),
                        "output_id": self.output_id, "output_index": 0, "delta": text})

    def process_tokens(self, count: int, ids, is_final: bool):
        if count == 0:
            return
        if count <= self.last_count:
            self.last_count = count
            return
        include_role = self.kind == "chat" and not self.role_sent
        full = decode_ids(self.tokenizer, ids[:count])
        if self.text_stop is not None:
            full, _ = self.text_stop.advance(full, is_final)
        emit = None
        if full:
            d = self.delta.advance(full, is_final)
            if include_role or d:
                emit = d
                if include_role:
                    self.role_sent = True
        self.last_count = count
        if emit is not None:
            self.emit_delta(emit, include_role)

    def callback(self):
        def on_token(count, ids, entry=None):
            if entry is not None and self.kind == "chat":
                self.pending_lp += logprob_content(self.tokenizer, [ids[count - 1]], [entry[0]], [entry[1]])
            self.process_tokens(count, ids, False)
        return on_token

    def flush_remaining(self, ids):
        if ids:
            self.process_tokens(len(ids), ids, True)

    def emit_rest(self, text: str):
        """A request with stops: what the outcome's text holds beyond the deltas sent (a cut inside a token's text)."""
        sent = self.delta.snapshot()
        if not text.startswith(sent):
            sent = sent.lstrip()
        rest = text[len(sent):] if text.startswith(sent) else ""
        if rest:
            self.delta.previous += rest
            self.emit_delta(rest, self.kind == "chat" and not self.role_sent)

    def finalize(self, normalized: str, prompt_tokens: int, completion_tokens: int):
        if self.finished:
            return
        self.finished = True
        if self.kind == "chat":
            choice = {"index": 0, "delta": {}, "finish_reason": "stop"}
            if self.has_stops:
                choice["stop_reason"] = self.stop_reason
            if self.pending_lp:  # tokens that produced no text of their own
                choice["logprobs"], self.pending_lp = {"content": self.pending_lp}, []
            self._send({"id": self.id, "object": "chat.completion.chunk", "created": self.created,
                        "model": self.model, "choices": [choice],
                        "usage": {"prompt_tokens": prompt_tokens, "completion_tokens": completion_tokens,
                                  "total_tokens": prompt_tokens + completion_tokens}})
        else:
            self._send({"type": "response.completed", "response": dict(self._head(), output=[
                {"id": self.output_id, "type": "message", "role": "assistant",
                 "content": [{"type": "output_text", "text": normalized}]}],
                usage={"input_tokens": prompt_tokens, "output_tokens": completion_tokens,
                       "total_tokens": prompt_tokens + completion_tokens},
                **({"stop_reason": self.stop_reason} if self.has_stops else {}))})
        self.q.put("[DONE]")
        self.q.put(None)

    def send_error(self, message: str):
        if self.finished:
            return
        self.finished = True
        self._send({"type": "response.error", "error": {"message": message}})
        self.q.put("[DONE]")
        self.q.put(None)

    def emit_fallback(self, text: str):
        self.emit_delta(text, True)
        self.finalize(text, 0, 0)

    def events(self):
        while True:
            item = self.q.get()
            if item is None:
                return
            yield f"data: {item}\n\n"


def _chat_response(model, text, pt, ct):
    return {"id": f"chatcmpl-{uuid.uuid4()}", "object": "chat.completion", "created": _now(), "model": model,
            "choices": [{"index": 0, "message": {"role": "assistant", "content": text}, "finish_reason": "stop"}],
            "usage": {"prompt_tokens": pt, "completion_tokens": ct, "total_tokens": pt + ct}}


def _responses_response(model, text, pt, ct):
    return {"id": f"resp-{uuid.uuid4()}", "object": "response", "created": _now(), "model": model,
            "output": [{"id": f"msg-{uuid.uuid4()}", "type": "message", "role": "assistant",
                        "content": [{"type": "output_text", "text": text}]}],
            "usage": {"prompt_tokens": pt, "completion_tokens": ct, "total_tokens": pt + ct}}


def handle_generation(state: ServerState, req: dict, kind: str):
    """Shared body of responses_endpoint / chat_completions_endpoint (routes.rs:55-222).
    Returns ("json", dict) or ("stream", StreamController)."""
    if not isinstance(req, dict):
        raise ApiError.bad_request("request body must be a JSON object")
    model = req.get("model")
    if not isinstance(model, str):
        raise ApiError.bad_request("missing field `model`")
    state.validate_model(model)
    messages = req.get("input" if kind == "responses" else "messages") or []
    prompt, images = convert_messages(messages)
    stream = bool(req.get("stream"))
    if "<image>" not in prompt:
        if stream:
            c = StreamController(state.tokenizer, kind, model)
            c.send_initial()
            c.emit_fallback(MISSING_IMAGE_MARKDOWN)
            return "stream", c
        mk = _chat_response if kind == "chat" else _responses_response
        return "json", mk(model, MISSING_IMAGE_MARKDOWN, 0, 0)
    max_tokens = req.get("max_output_tokens") if kind == "responses" else None
    if max_tokens is None:
        max_tokens = req.get("max_tokens")
    params = merge_decode(state.defaults, req, max_tokens)
    logprobs = parse_logprobs(req) if kind == "chat" else None  # (/v1/responses has no log-probabilities)
    constraint = parse_token_constraint(req, getattr(state.engine, "vocab", None))
    stops = parse_stops(req, state.tokenizer, getattr(state.engine, "vocab", None))
    penalties = parse_penalties(req)
    if penalties:  # keywords of decode / submit beside the constraint's; a penalised decode does not stream either
        constraint = dict(constraint or {}, **penalties)
    window = parse_ngram_window(req, getattr(state.engine, "vocab", None))
    if window:  # the same
        constraint = dict(constraint or {}, **window)
    guided = parse_guided(req, state.tokenizer, getattr(state.engine, "vocab", None))
    if guided:  # the same; the response names how the automaton ended
        constraint = dict(constraint or {}, **guided)
    if stream:
        c = StreamController(state.tokenizer, kind, model)
        if stops:
            from .stops import TextStop
            c.has_stops = True
            if stops["stop"]:
                c.text_stop = TextStop(stops["stop"], stops["include_stop_in_output"])

        def work():
            try:
                c.send_initial()
                out = generate_blocking(state, prompt, images, params, c.callback(), logprobs, constraint, stops)
                c.stop_reason = getattr(out, "stop_reason", None)
                c.flush_remaining(out.generated_tokens)
                if c.has_stops:
                    c.emit_rest(out.text)
                c.finalize(out.text, out.prompt_tokens, out.response_tokens)
            except ApiError as e:
                c.send_error(e.message)
            except Exception as e:  # noqa: BLE001 - reported to the client like generation.rs:60-70
                c.send_error(f"generation task failed: {e}")

        threading.Thread(target=work, daemon=True).start()
        return "stream", c
    out = generate_blocking(state, prompt, images, params, None, logprobs, constraint, stops)
    mk = _chat_response if kind == "chat" else _responses_response
    body = mk(model, out.text, out.prompt_tokens, out.response_tokens)
    if stops:  # the matched string or token id; null when EOS or the length limit ended the request
        if kind == "chat":
            body["choices"][0]["stop_reason"] = getattr(out, "stop_reason", None)
        else:
            body["stop_reason"] = getattr(out, "stop_reason", None)
    if guided:  # "complete" (the page ended in a terminal state: finish_reason "stop"), "violated" or null
        if kind == "chat":
            body["choices"][0]["guided_status"] = getattr(out, "guided_status", None)
        else:
            body["guided_status"] = getattr(out, "guided_status", None)
    if logprobs is not None:
        body["choices"][0]["logprobs"] = {"content": logprob_content(state.tokenizer, out.generated_tokens,
                                                                     out.token_logprobs or [], out.top_logprobs or [])}
    return "json", body


def create_app(state: ServerState):
    """The FastAPI application (app.rs:11-63: routes mounted under /v1, permissive CORS)."""
    from fastapi import FastAPI, Request
    from fastapi.middleware.cors import CORSMiddleware
    from fastapi.responses import JSONResponse, PlainTextResponse, Response, StreamingResponse
    from starlette.concurrency import run_in_threadpool

    app = FastAPI(title="DeepSeek-OCR API Server (MI355X)")
    app.add_middleware(CORSMiddleware, allow_origins=["*"], allow_methods=["*"], allow_headers=["*"])

    @app.exception_handler(ApiError)
    async def _api_error(_req, exc: ApiError):
        return JSONResponse(exc.body(), status_code=exc.status)

    @app.get("/v1/health")
    async def health():
        return PlainTextResponse("ok")

    @app.get("/v1/models")
    async def models():
        return {"object": "list", "data": [{"id": state.model_id, "object": "model", "created": _now(),
                                            "owned_by": "deepseek-ocr"}]}

    @app.options("/v1/models")
    async def options_models():
        return Response(status_code=200)

    async def _run(request: Request, kind: str):
        try:
            req = await request.json()
        except (ValueError, UnicodeDecodeError) as e:
            raise ApiError.bad_request(f"invalid JSON body: {e}")
        how, val = await run_in_threadpool(handle_generation, state, req, kind)
        if how == "stream":
            return StreamingResponse(val.events(), media_type="text/event-stream")
        return JSONResponse(val)

    @app.post("/v1/responses")
    async def responses(request: Request):
        return await _run(request, "responses")

    @app.post("/v1/chat/completions")
    async def chat(request: Request):
        return await _run(request, "chat")

    return app


def add_scheduler_args(p):
    p.add_argument("--slots", type=int, default=0,
                   help="decode-session slots (1..8): concurrent requests share one running batch; 0 = off")
    p.add_argument("--max-context", type=int, default=4096,
                   help="context rows per session slot (a request needs prompt + max_new_tokens + 1)")
    p.add_argument("--per-request-params", action="store_true",
                   help="with --slots: a request's own temperature / top_p / top_k / repetition_penalty / "
                        "no_repeat_ngram_size join the running batch (per-row selection on the device) instead of "
                        "waiting for it to drain; off by default")
    p.add_argument("--logprobs", action="store_true",
                   help="with --slots: open the decode session with per-token log-probabilities (the exact lm_head "
                        "runs for every request), so requests with `logprobs: true` join the running batch instead "
                        "of waiting for it to drain; off by default")
    p.add_argument("--logit-bias", action="store_true",
                   help="with --slots: open the decode session with a logit-bias row per slot, so requests with "
                        "`logit_bias` / `allowed_token_ids` / `banned_token_ids` join the running batch (a burst with "
                        "such a request runs the exact lm_head) instead of waiting for it to drain; off by default")
    p.add_argument("--stops", action="store_true",
                   help="with --slots: open the decode session with a stop table per slot, so requests with `stop` / "
                        "`stop_token_ids` join the running batch (the device ends such a page on the step that "
                        "completes a stop) instead of waiting for it to drain; off by default")
    p.add_argument("--penalties", action="store_true",
                   help="with --slots: open the decode session with a penalty record per slot, so requests with "
                        "`frequency_penalty` / `presence_penalty` / `min_p` join the running batch (a burst with such "
                        "a request runs the exact lm_head) instead of waiting for it to drain; off by default")
    p.add_argument("--ngram-window", action="store_true",
                   help="with --slots: open the decode session with a windowed n-gram ban record per slot, so requests "
                        "with `ngram_size` / `window_size` / `whitelist_token_ids` join the running batch (a burst with "
                        "such a request runs the exact lm_head) instead of waiting for it to drain; off by default")
    p.add_argument("--guided", action="store_true",
                   help="with --slots: open the decode session with the tables of a token automaton per slot (about "
                        "25 MB each at the full vocabulary), so requests with `guided_choice` / `structured_outputs` / "
                        "`token_automaton` join the running batch (a burst with such a request runs the exact "
                        "lm_head) instead of waiting for it to drain; off by default")
    p.add_argument("--prefix-cache", type=int, default=0,
                   help="with --slots: keep the K/V rows of up to N pages' image prefixes (LRU), so a later prompt on "
                        "the same image under the same vision settings skips vision and the prefill of those rows; "
                        "0 = off (the default)")
    p.add_argument("--admit-chunk", type=int, default=0, metavar="ROWS",
                   help="with --slots: admit a waiting request in slices (its vision, then ROWS >= 32 prompt rows at a "
                        "time) and run one burst of the running requests between two slices, so a stream waits for a "
                        "slice, not for a whole admission; 0 = off (the default)")


def make_scheduler(state: ServerState, slots: int, max_context: int, per_request_params: bool = False,
                   logprobs: bool = False, prefix_cache: int = 0, admit_chunk: int = 0, logit_bias: bool = False,
                   stops: bool = False, penalties: bool = False, ngram_window: bool = False, guided: bool = False):
    """The state's scheduler for --slots N (None for 0: requests take the lock path).  per_request_params: the
    DecodeParameters merge_decode builds from a request body are admitted into the session as that request's own.
    prefix_cache: --prefix-cache N (ValueError without --slots: the entries live in the decode session)."""
    if not 0 <= prefix_cache <= 64 or (prefix_cache and not slots):
        raise ValueError("--prefix-cache needs --slots (the prefix entries live in the decode session) and N in 0..64")
    if admit_chunk and (not slots or admit_chunk < 32):
        raise ValueError("--admit-chunk needs --slots (a chunked admission runs in the decode session) and ROWS >= 32")
    if logit_bias and not slots:
        raise ValueError("--logit-bias needs --slots (the bias rows live in the decode session)")
    if stops and not slots:
        raise ValueError("--stops needs --slots (the stop tables live in the decode session)")
    if penalties and not slots:
        raise ValueError("--penalties needs --slots (the penalty records live in the decode session)")
    if ngram_window and not slots:
        raise ValueError("--ngram-window needs --slots (the window records live in the decode session)")
    if guided and not slots:
        raise ValueError("--guided needs --slots (the automaton tables live in the decode session)")
    if not slots:
        return None
    from .scheduler import BatchScheduler
    return BatchScheduler(state.engine, state.tokenizer, slots, max_context, state.defaults, state.vision,
                          per_request_params=per_request_params, logprobs=logprobs, prefix_cache=prefix_cache,
                          admit_chunk=admit_chunk, **({"logit_bias": True} if logit_bias else {}),
                          **({"stops": True} if stops else {}), **({"penalties": True} if penalties else {}),
                          **({"ngram_window": True} if ngram_window else {}), **({"guided": True} if guided else {}))


def main(argv=None) -> int:
    """`deepseek-ocr-server` (server/src/args.rs + config defaults host 0.0.0.0, port 8000)."""
    import argparse

    from .cli import (_vocab_of, add_inference_args, add_model_args, decode_params, load_tokenizer, model_config,
                      parse_device, vision_settings)
    from .engine import ModelLoadArgs, load_model

    p = argparse.ArgumentParser(prog="deepseek-ocr-server", description="DeepSeek-OCR API Server (MI355X engine)")
    add_model_args(p)
    add_inference_args(p)
    p.add_argument("--host", default="0.0.0.0")
    p.add_argument("--port", type=int, default=8000)
    add_scheduler_args(p)
    args = p.parse_args(argv)
    if not 0 <= args.prefix_cache <= 64 or (args.prefix_cache and not args.slots):
        p.error("--prefix-cache needs --slots and N in 0..64 (a session holds at most 64 prefix entries)")
    if args.admit_chunk and (not args.slots or args.admit_chunk < 32):
        p.error("--admit-chunk needs --slots and ROWS >= 32 (a chunked admission runs in the decode session)")
    if args.logit_bias and not args.slots:
        p.error("--logit-bias needs --slots (the bias rows live in the decode session)")
    if args.stops and not args.slots:
        p.error("--stops needs --slots (the stop tables live in the decode session)")
    if args.penalties and not args.slots:
        p.error("--penalties needs --slots (the penalty records live in the decode session)")
    if args.ngram_window and not args.slots:
        p.error("--ngram-window needs --slots (the window records live in the decode session)")
    if args.guided and not args.slots:
        p.error("--guided needs --slots (the automaton tables live in the decode session)")
    config = model_config(args)  # --model deepseek-ocr | deepseek-ocr-2: the bundled config and vision defaults
    engine = load_model(ModelLoadArgs(config_path=config, weights_path=args.weights, snapshot_path=args.snapshot,
                                      snapshot_packed=getattr(args, "snapshot_packed", None),
                                      device=parse_device(args.device), dtype=args.dtype,
                                      synthetic_seed=args.synthetic_seed))
    state = ServerState(engine, load_tokenizer(args.tokenizer, _vocab_of(config)), args.model,
                        vision_settings(args), decode_params(args))
    state.scheduler = make_scheduler(state, args.slots, args.max_context, args.per_request_params, args.logprobs,
                                     args.prefix_cache, args.admit_chunk, args.logit_bias, args.stops,
                                     args.penalties, args.ngram_window, args.guided)
    import uvicorn
    uvicorn.run(create_app(state), host=args.host, port=args.port)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
