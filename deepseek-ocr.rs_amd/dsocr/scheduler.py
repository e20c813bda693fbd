"""Continuous batching over one engine: requests join and leave a decode session between bursts of steps.

``BatchScheduler`` owns the engine from one worker thread (the engine is Send-not-Sync).  ``submit`` does the host
work of a request on the caller's thread (page preprocessing on the host, prompt tokens) and returns a Future of
the ``DecodeOutcome``.  The worker loop is: admit waiting requests while slots are free, poll (an admission's prefill
yields the first token), step a burst, poll, hand every active request its new tokens, retire what finished.

A request whose parameters differ from the session's in more than ``max_new_tokens`` / ``seed``, or that needs more
context or output than the session has, waits until the session is empty and then runs alone through
``engine.decode``.  With ``per_request_params`` the session is opened per request (``open_session(...,
per_request=True)``) and every request is admitted with its own parameters: only one without ``use_cache``, or one
that needs more output or context than the session has, still runs alone.  Requests are served in arrival order: nothing behind such a request is admitted before it ran.

Log-probabilities: ``BatchScheduler(..., logprobs=True)`` opens the session with ``logprobs=True`` (the exact head
runs for everyone) and ``submit(..., logprobs=K)`` asks for a request's entries: they are fetched with its new tokens,
``on_token`` then receives ``(n, tokens, entry)`` with ``entry = (logprob, [(id, logprob)] * K)`` of the newest token,
and the outcome carries ``token_logprobs`` / ``top_logprobs``.  Without the scheduler's flag such a request runs alone
through ``engine.decode(..., logprobs=K)`` after the session drained, like any request that does not fit.

Token constraints: ``submit(..., logit_bias={id: value}, allowed_token_ids=[...], banned_token_ids=[...])`` are merged
into one constraint on the caller's thread (``dsocr.constraint.merge_constraint``; a bad one fails the future).
``BatchScheduler(..., logit_bias=True)`` opens the session with ``logit_bias=True`` and such a request shares it (a
burst with a constrained page runs the exact head); without the flag it runs alone through ``engine.decode(...)``
with the same three arguments after the session drained.  Prefix-cache keys do not see the constraint: a constrained
retry on a cached page is a prefix hit.

Stop sequences: ``submit(..., stop="...", stop_token_ids=[...], include_stop_in_output=False)`` are merged into one stop
set on the caller's thread (``dsocr.stops.merge_stops``; a bad one fails the future).  ``BatchScheduler(...,
stops=True)`` opens the session with ``stops=True`` and such a request shares it: the device ends the page on the step
that completes a sequence, the worker also searches the decoded text for the stop strings after every delivery (a stop
string can arise from another tokenisation) and retires the slot on a hit, ``on_token`` sees only tokens no later hit
can remove, and the outcome is trimmed unless ``include_stop_in_output``.  Without the flag the request runs alone
through ``engine.decode(...)`` with the same arguments after the session drained.

Penalties: ``submit(..., frequency_penalty=X, presence_penalty=X, min_p=X)`` are checked on the caller's thread
(``dsocr.penalties.make_penalties``; a bad one fails the future).  ``BatchScheduler(..., penalties=True)`` opens the
session with ``penalties=True`` and such a request shares it (a burst with a penalised page runs the exact head);
without the flag it runs alone through ``engine.decode(...)`` with the same arguments after the session drained.
Prefix-cache keys do not see the record.

Windowed n-gram ban: ``submit(..., ngram_window=NgramWindow(...))`` is checked on the caller's thread
(``dsocr.ngram_window.make_ngram_window``; a bad one fails the future).  ``BatchScheduler(..., ngram_window=True)``
opens the session with ``ngram_window=True`` and such a request shares it (a burst with such a page runs the exact
head); without the flag it runs alone through ``engine.decode(...)`` with the same argument after the session drained.
Prefix-cache keys do not see the record.

Guided decoding: ``submit(..., guided=TokenAutomaton(...))`` (``dsocr.guided``) is checked on the caller's thread (a
bad one fails the future).  ``BatchScheduler(..., guided=True)`` opens the session with ``guided=True`` and such a
request shares it: the automaton goes to the admission call, whichever form it takes, and the outcome carries
``guided_status`` (read from the slot before it is retired).  Without the flag the request runs alone through
``engine.decode``.  Prefix-cache keys do not see the automaton: a guided retry on a cached page is a prefix hit.

Page prefix cache: ``BatchScheduler(..., prefix_cache=N)`` (default 0: nothing changes) keeps the K/V rows of up to N
pages' prompt prefixes (BOS and the image rows) in the session.  After a one-image request is admitted its prefix is
kept (``Session.keep_prefix``, rows = index of the last image position + 1) under the key (SHA-256 of the image as
submitted, the vision settings, the prefix ids); a later request with the same key is admitted through
``Session.admit_prefix`` and skips vision and the prefill of those rows.  Eviction is LRU; an evicted handle is
dropped before the next keep.  Prompts with several images, exclusive requests and prompts with no text after the
image bypass the cache.  ``prefix_hits`` / ``prefix_misses`` count the lookups.

Chunked admission: ``BatchScheduler(..., admit_chunk=ROWS)`` (default 0: nothing changes; ROWS >= 32) admits a waiting
request in slices (``Session.admit_begin`` / ``admit_advance``: the page's vision, then the prompt ``ROWS`` rows at a
time) and alternates one slice with one burst of the running slots, so a running stream waits for a slice, not for a
whole admission.  Bursts stay 1 step while any request streams, else 8; with no slot running the slices run back to
back.  One admission is pending at a time and nothing behind it overtakes it.  Exclusive requests stay exclusive, a
prefix-cache hit is still admitted through ``admit_prefix`` in one call, and the prefix of a page admitted in slices
is kept when its last slice completes.  ``admit_slices`` counts the slices and ``events`` lists ``("slice", kind,
pages active after it)`` and ``("burst", active, steps)`` in the order they ran.

The engine object needs ``open_session(slots, max_context, params)`` (admit / step / poll / retire / close, see
``dsocr.engine.Session``), ``decode`` and, for prompts with several images, ``image_embeddings``; tests drive the
scheduler with a scripted fake.
"""
from __future__ import annotations

import threading
from collections import OrderedDict, deque
from concurrent.futures import Future
from dataclasses import dataclass, field, fields
from typing import Any, Callable, Optional, Sequence

from .constraint import merge_constraint
from .guided import STATUS_NAMES
from .ngram_window import make_ngram_window
from .penalties import make_penalties
from .stops import TextStop, TokenHoldback, merge_stops
from .engine import DecodeOutcome, DecodeParameters, Page, VisionSettings, build_prompt_tokens, normalize_text

BURST = 8  # steps between polls while nobody streams: the cadence Engine::decode_cached polls at


class CapacityError(RuntimeError):
    """A burst would take a slot past its cache rows (the host-side capacity invariant)."""


@dataclass
class _Request:
    prompt: str
    images: Sequence
    vision: VisionSettings
    params: DecodeParameters
    on_token: Optional[Callable]
    future: Future
    ids: list
    mask: list
    page: Any = None
    pages: list = field(default_factory=list)  # several images: their rows are embedded by the worker
    exclusive: bool = False
    tokens: list = field(default_factory=list)
    kv_pos: int = 0  # upper bound of the slot's device kv_pos: prompt + steps since admission
    done: bool = False
    logprobs: Optional[int] = None  # alternatives per token the request asked for
    token_lp: list = field(default_factory=list)
    top_lp: list = field(default_factory=list)
    prefix_key: Any = None  # prefix cache: (image digest, vision settings, prefix ids), or None to bypass it
    prefix_rows: int = 0
    constraint: Any = None  # the request's merged LogitConstraint, or None
    stops: Any = None       # the request's merged StopSet, or None
    penalties: Any = None   # the request's checked Penalties, or None
    ngram_window: Any = None  # the request's checked NgramWindow, or None
    guided: Any = None        # the request's checked TokenAutomaton, or None
    guided_status: Any = None  # "complete" / "violated" / None, read from the slot before it is retired
    stop_args: dict = field(default_factory=dict)  # ... as the keywords engine.decode takes
    include_stop: bool = False
    holdback: Any = None    # TokenHoldback of a streaming request with stops
    text_stop: Any = None   # TextStop of a request with stop strings
    shown: int = 0          # tokens on_token has seen


def _image_digest(im) -> str:
    """SHA-256 of an image as it was submitted: raw bytes as they are, an array or a PIL image by shape and pixels."""
    import hashlib
    h = hashlib.sha256()
    if isinstance(im, (bytes, bytearray, memoryview)):
        h.update(bytes(im))
        return h.hexdigest()
    import numpy as np
    if hasattr(im, "convert"):  # PIL image
        h.update(str(getattr(im, "mode", "")).encode())
    arr = np.ascontiguousarray(np.asarray(im))
    h.update(repr((arr.shape, arr.dtype.str)).encode())
    h.update(arr.tobytes())
    return h.hexdigest()


def _default_prepare(engine, tokenizer, prompt, images, vision):
    """Host work of one request: the pages (preprocessed on the host: the worker thread owns the GPU) and the
    prompt tokens.  Returns (ids, mask, pages)."""
    pages = [Page(im, vision, None, getattr(engine, "variant", 0)) for im in images]
    ids, mask = build_prompt_tokens(tokenizer, prompt, [p.n_image_tokens for p in pages])
    return ids, mask, pages


def _takes_entry(cb) -> bool:
    """True when ``cb(n, tokens, entry)`` is a valid call (or the signature cannot be read)."""
    import inspect
    try:
        inspect.signature(cb).bind(0, [], None)
    except TypeError:
        return False
    except ValueError:
        return True
    return True


def _penalty_kwargs(pn) -> dict:
    """A checked Penalties record as the keywords ``Session.admit`` and ``engine.decode`` take."""
    return dict(frequency_penalty=pn.frequency, presence_penalty=pn.presence, min_p=pn.min_p)


def _decode_text(tokenizer, ids) -> str:
    if not hasattr(tokenizer, "decode"):
        return ""
    try:
        return tokenizer.decode([int(t) for t in ids], skip_special_tokens=True)
    except TypeError:
        return tokenizer.decode([int(t) for t in ids])


class BatchScheduler:
    def __init__(self, engine, tokenizer, slots: int, max_context: int,
                 defaults: DecodeParameters = DecodeParameters(), vision: Optional[VisionSettings] = None,
                 prepare: Optional[Callable] = None, per_request_params: bool = False, logprobs: bool = False,
                 prefix_cache: int = 0, admit_chunk: int = 0, logit_bias: bool = False, stops: bool = False,
                 penalties: bool = False, ngram_window: bool = False, guided: bool = False):
        if not 1 <= int(slots) <= 8:
            raise ValueError("a session has 1..8 slots")
        if int(admit_chunk) != 0 and int(admit_chunk) < 32:
            raise ValueError("admit_chunk is 0 (off) or at least 32 prompt rows")
        self.admit_chunk = int(admit_chunk)
        self._pending = None           # the request whose admission is running in slices
        self.admit_slices = 0          # slices run (vision and prefill chunks)
        self.chunked_admissions = 0    # admissions completed in slices
        self.events: list = []         # ("slice", kind, active) / ("burst", active, steps), chunked mode only
        if not 0 <= int(prefix_cache) <= 64:
            raise ValueError("prefix_cache is 0..64 entries (a session holds at most 64)")
        self.prefix_cache = int(prefix_cache)
        self._prefix: OrderedDict = OrderedDict()  # key -> handle of the open session, least recently used first
        self.prefix_hits = 0
        self.prefix_misses = 0
        self.prefix_fallbacks = 0      # hits whose admit_prefix was refused and that were admitted plainly instead
        self.prefix_keep_failures = 0  # keeps (or the evictions before them) the session refused
        self.engine, self.tokenizer = engine, tokenizer
        self.slots, self.max_context = int(slots), int(max_context)
        self.defaults = defaults
        self.per_request_params = bool(per_request_params)
        self.logprobs = bool(logprobs)
        self.logit_bias = bool(logit_bias)
        self.stops = bool(stops)
        self.penalties = bool(penalties)
        self.ngram_window = bool(ngram_window)
        self.guided = bool(guided)
        self.vision = vision or VisionSettings()
        self._prepare = prepare or _default_prepare
        self._queue: deque = deque()
        self._active: list = []  # index = slot
        self._session = None
        self._cv = threading.Condition()
        self._stop = False
        self.max_active = 0      # most pages the session held at once
        self.exclusive_runs = 0  # requests that ran alone through engine.decode
        self.bursts: list = []   # (active pages, steps asked) of every burst, for tests and tools
        self._worker = threading.Thread(target=self._run, name="dsocr-scheduler", daemon=True)
        self._worker.start()

    # ------------------------------------------------------------------ caller's side
    def compatible(self, params: DecodeParameters, prompt_len: int) -> bool:
        """True when the request can share the session: only max_new_tokens / seed differ from the defaults (with
        per_request_params: whatever its selection parameters are)."""
        for f in fields(DecodeParameters):
            if self.per_request_params or f.name in ("max_new_tokens", "seed"):
                continue
            if getattr(params, f.name) != getattr(self.defaults, f.name):
                return False
        if not params.use_cache or params.max_new_tokens < 1:
            return False
        if params.max_new_tokens > self.defaults.max_new_tokens:
            return False
        return prompt_len + params.max_new_tokens + 1 <= self.max_context

    def submit(self, prompt: str, images: Sequence = (), vision: Optional[VisionSettings] = None,
               params: Optional[DecodeParameters] = None, on_token: Optional[Callable] = None,
               logprobs: Optional[int] = None, logit_bias=None, allowed_token_ids=None,
               banned_token_ids=None, stop=None, stop_token_ids=None,
               include_stop_in_output: bool = False, frequency_penalty=None, presence_penalty=None,
               min_p=None, ngram_window=None, guided=None) -> Future:
        """``guided``: the request's token automaton (see the module text).
        ``ngram_window``: the request's windowed n-gram ban (see the module text).
        ``frequency_penalty`` / ``presence_penalty`` / ``min_p``: the request's penalties (see the module text).
        ``stop`` / ``stop_token_ids`` / ``include_stop_in_output``: the request's stop set (see the module text).
        ``logit_bias`` / ``allowed_token_ids`` / ``banned_token_ids``: the request's token constraint (see the
        module text).  ``logprobs`` = K (0..20) asks for the request's per-token log-probabilities.  It changes the arity of
        ``on_token``: the callback is then called as ``on_token(n, tokens, entry)``, with ``entry = (logprob,
        [(id, logprob)] * K)`` of the newest token, instead of ``on_token(n, tokens)``.  A two-argument callback
        given together with ``logprobs`` is refused here (ValueError through the future) rather than failing on
        every token."""
        fut: Future = Future()
        if logprobs is not None and on_token is not None and not _takes_entry(on_token):
            fut.set_exception(ValueError("with logprobs, on_token is called as on_token(n, tokens, entry)"))
            return fut
        if logprobs is not None and not 0 <= int(logprobs) <= 20:
            fut.set_exception(ValueError("logprobs must be 0..20"))
            return fut
        try:
            constraint = merge_constraint(logit_bias, allowed_token_ids, banned_token_ids,
                                          getattr(self.engine, "vocab", None))
            stops = merge_stops(stop, stop_token_ids, self.tokenizer, getattr(self.engine, "vocab", None))
            penalties = make_penalties(frequency_penalty, presence_penalty, min_p)
            if ngram_window is not None and not hasattr(ngram_window, "ngram_size"):
                raise ValueError("ngram_window must be a dsocr.ngram_window.NgramWindow")
            window = make_ngram_window(ngram_window, vocab=getattr(self.engine, "vocab", None))
            if guided is not None:
                if not hasattr(guided, "validate"):
                    raise ValueError("guided must be a dsocr.guided.TokenAutomaton")
                guided.validate(getattr(self.engine, "vocab", None) or (1 << 31))
        except ValueError as e:
            fut.set_exception(e)
            return fut
        params = params or self.defaults
        vision = vision or self.vision
        try:
            ids, mask, pages = self._prepare(self.engine, self.tokenizer, prompt, list(images), vision)
        except Exception as e:  # noqa: BLE001 - the request's own error, reported through its future
            fut.set_exception(e)
            return fut
        rq = _Request(prompt, list(images), vision, params, on_token, fut, list(ids), list(mask))
        if len(pages) == 1:
            rq.page = pages[0]
        else:
            rq.pages = list(pages)
        rq.logprobs = None if logprobs is None else int(logprobs)
        rq.constraint = constraint
        rq.penalties = penalties
        rq.ngram_window = window
        rq.guided = guided
        if stops is not None:
            rq.stops, rq.include_stop = stops, bool(include_stop_in_output)
            rq.stop_args = dict(stop=stop, stop_token_ids=stop_token_ids, include_stop_in_output=rq.include_stop)
            if on_token is not None:
                rq.holdback = TokenHoldback(stops.seqs, rq.include_stop)
            if stops.strings:
                rq.text_stop = TextStop(stops.strings, rq.include_stop)
        rq.exclusive = (not self.compatible(params, len(rq.ids)) or (rq.logprobs is not None and not self.logprobs) or
                        (constraint is not None and not self.logit_bias) or (stops is not None and not self.stops) or
                        (penalties is not None and not self.penalties) or
                        (window is not None and not self.ngram_window) or
                        (guided is not None and not self.guided))
        if self.prefix_cache and len(rq.images) == 1 and not rq.exclusive and any(rq.mask):
            rows = max(i for i, m in enumerate(rq.mask) if m) + 1
            if rows < len(rq.ids):  # some text follows the image: the last row's logits come from a new row
                try:
                    rq.prefix_key = (_image_digest(rq.images[0]),
                                     (vision.base_size, vision.image_size, bool(vision.crop_mode)), tuple(rq.ids[:rows]))
                    rq.prefix_rows = rows
                except Exception:  # noqa: BLE001 - an image that cannot be hashed is served without the cache
                    rq.prefix_key = None
        with self._cv:
            if self._stop:
                fut.set_exception(RuntimeError("scheduler is closed"))
                return fut
            self._queue.append(rq)
            self._cv.notify_all()
        return fut

    def close(self):
        with self._cv:
            self._stop = True
            self._cv.notify_all()
        self._worker.join()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    # ------------------------------------------------------------------ worker
    def _run(self):
        try:
            while True:
                with self._cv:
                    while not self._stop and not self._queue and not self._active and self._pending is None:
                        self._cv.wait()
                    if self._stop:
                        break
                try:
                    self._turn()
                except Exception as e:  # noqa: BLE001 - a session-wide failure: every active request learns of it
                    self._fail_active(e)
        finally:
            self._fail_active(RuntimeError("scheduler is closed"))
            with self._cv:
                pending, self._queue = list(self._queue), deque()
            for rq in pending:
                rq.future.set_exception(RuntimeError("scheduler is closed"))

    def _fail_active(self, exc):
        active, self._active = self._active, []
        if self._pending is not None:
            active, self._pending = active + [self._pending], None
        for rq in active:
            if not rq.future.done():
                rq.future.set_exception(exc)
        self._close_session()

    def _close_session(self):
        s, self._session = self._session, None
        self._prefix.clear()  # the handles die with their session
        if s is not None:
            try:
                s.close()
            except Exception:  # noqa: BLE001 - closing after a failure must not hide it
                pass

    def _head(self):
        with self._cv:
            return self._queue[0] if self._queue else None

    def _pop(self):
        with self._cv:
            return self._queue.popleft()

    def _turn(self):
        admitted = False
        while True:
            rq = self._head()
            if rq is None:
                break
            if rq.exclusive:
                if self._active or self._pending is not None:
                    break  # it waits for the session to drain; nothing behind it overtakes it
                self._pop()
                self._run_exclusive(rq)
                continue
            if self._pending is not None or len(self._active) >= self.slots:
                break
            self._pop()
            if self.admit_chunk and not self._prefix_hit(rq):
                self._begin(rq)
                break
            admitted |= self._admit(rq)
        if self._pending is not None:  # one slice, then (below) one burst of the running slots
            admitted |= self._advance()
        if not self._active:
            return
        if admitted:  # the prefill's own selection: every new page has its first token
            self._deliver(self._session.poll())
            self._retire_done()
            if not self._active:
                return
        burst = 1 if any(rq.on_token is not None for rq in self._active) else min(BURST, self._session.burst_cap)
        # host-side capacity invariant: a finished page is retired at every burst boundary, so no slot's KV
        # position can pass the session's rows (max_context + burst cap); asserted before the burst is launched
        for slot, rq in enumerate(self._active):
            if rq.kv_pos + burst > self._session.kv_cap:
                raise CapacityError(f"slot {slot}: kv_pos {rq.kv_pos} + burst {burst} exceeds the session's "
                                    f"{self._session.kv_cap} cache rows")
        self.bursts.append((len(self._active), burst))
        if self.admit_chunk:
            self.events.append(("burst", len(self._active), burst))
        status = self._session.step(burst)
        for rq in self._active:
            rq.kv_pos += burst
        self._deliver(status)
        self._retire_done()

    def _prefix_hit(self, rq) -> bool:
        return rq.prefix_key is not None and rq.prefix_key in self._prefix

    def _open(self):
        if self._session is None:
            kw = {}
            if self.per_request_params:
                kw["per_request"] = True
            if self.logprobs:
                kw["logprobs"] = True
            if self.logit_bias:
                kw["logit_bias"] = True
            if self.stops:
                kw["stops"] = True
            if self.penalties:
                kw["penalties"] = True
            if self.ngram_window:
                kw["ngram_window"] = True
            if self.guided:
                kw["guided"] = True
            self._session = self.engine.open_session(self.slots, self.max_context, self.defaults, **kw)

    def _admit_args(self, rq):
        """(image rows of a prompt with several images, the keywords of admit / admit_prefix / admit_begin)"""
        rows = None
        if rq.pages:
            import numpy as np
            rows = np.concatenate(self.engine.image_embeddings(rq.pages), axis=0)
        kw = {} if rq.logprobs is None else {"logprobs": rq.logprobs}
        if rq.constraint is not None:
            kw.update(rq.constraint.kwargs())
        if rq.stops is not None:
            kw.update(stops=rq.stops, include_stop_in_output=rq.include_stop)
        if rq.penalties is not None:
            kw.update(_penalty_kwargs(rq.penalties))
        if rq.ngram_window is not None:
            kw.update(rq.ngram_window.kwargs())
        if rq.guided is not None:
            kw["guided"] = rq.guided
        if self.per_request_params:
            kw["params"] = rq.params
        else:
            kw.update(max_new_tokens=rq.params.max_new_tokens, seed=rq.params.seed)
        return rows, kw

    def _begin(self, rq):
        """The admission of `rq` in slices: every check now, no device work; `_advance` runs the slices."""
        try:
            self._open()
            rows, kw = self._admit_args(rq)
            self._session.admit_begin(rq.ids, rq.mask, rq.page, rows, chunk_rows=self.admit_chunk, **kw)
        except Exception as e:  # noqa: BLE001 - the request's own error: the running slots are untouched
            rq.future.set_exception(e)
            return
        self._pending = rq

    def _advance(self) -> bool:
        """One slice of the pending admission; True when it made the page active."""
        rq = self._pending
        progress = getattr(self._session, "admit_progress", None)
        kind = "vision" if progress is not None and progress()["vision_stage"] else "prefill"
        try:
            done, slot = self._session.admit_advance()
        except Exception as e:  # noqa: BLE001 - a failed slice ends that admission alone
            self._pending = None
            rq.future.set_exception(e)
            return False
        self.admit_slices += 1
        if done:
            self._pending = None
            self.chunked_admissions += 1
            self._admitted(rq, slot, None)
        self.events.append(("slice", kind, len(self._active)))
        return done

    def _admit(self, rq) -> bool:
        try:
            self._open()
            rows, kw = self._admit_args(rq)
            handle = self._prefix.get(rq.prefix_key) if rq.prefix_key is not None else None
            if handle is not None:  # the page's prefix is cached: no vision, only the rows behind it are prefilled
                self._prefix.move_to_end(rq.prefix_key)
                self.prefix_hits += 1
                try:
                    slot = self._session.admit_prefix(handle, rq.ids, rq.mask, **kw)
                except Exception:  # noqa: BLE001 - refused behind the entry: the plain admission decides (and reports)
                    self.prefix_fallbacks += 1
                    slot = self._session.admit(rq.ids, rq.mask, rq.page, rows, **kw)
            else:
                slot = self._session.admit(rq.ids, rq.mask, rq.page, rows, **kw)
        except Exception as e:  # noqa: BLE001 - the request's own error: the running slots are untouched
            rq.future.set_exception(e)
            return False
        self._admitted(rq, slot, handle)
        return True

    def _admitted(self, rq, slot, handle):
        if slot != len(self._active):
            raise RuntimeError(f"session admitted into slot {slot}, expected {len(self._active)}")
        if rq.prefix_key is not None and handle is None:
            self.prefix_misses += 1
            self._keep_prefix(rq, slot)
        rq.kv_pos = len(rq.ids)
        self._active.append(rq)
        self.max_active = max(self.max_active, len(self._active))

    def _keep_prefix(self, rq, slot):
        """The prefix of the page just admitted into `slot`, kept under its key; the least recently used handle is
        dropped first when the cache is full.  Best effort: a keep the session refuses (memory, its 64 entries)
        leaves the request as it is and the page uncached."""
        try:
            while len(self._prefix) >= self.prefix_cache:
                _, old = self._prefix.popitem(last=False)
                self._session.drop_prefix(old)
            self._prefix[rq.prefix_key] = self._session.keep_prefix(slot, rq.prefix_rows)
        except Exception:  # noqa: BLE001 - counted, so that a cache that keeps nothing shows
            self.prefix_keep_failures += 1

    def _deliver(self, status):
        for st in status:
            rq = self._active[st.slot]
            room = rq.params.max_new_tokens - len(rq.tokens)
            fresh = list(st.new_tokens)[:max(room, 0)]
            entries = []
            if rq.logprobs is not None and fresh:  # the new tokens' entries with them (read before any retire)
                lp, ti, tl = self._session.logprobs(st.slot, len(rq.tokens), len(fresh), rq.logprobs)
                entries = [(float(lp[i]), [(int(a), float(b)) for a, b in zip(ti[i], tl[i])]) for i in range(len(fresh))]
            for i, t in enumerate(fresh):
                rq.tokens.append(int(t))
                if entries:
                    rq.token_lp.append(entries[i][0])
                    rq.top_lp.append(entries[i][1])
                if rq.on_token is not None:
                    # with stops only what no later hit can remove (the rest follows, or arrives at the retirement)
                    self._show(rq, len(rq.tokens) if rq.holdback is None else rq.holdback.feed(rq.tokens))
            rq.done = bool(st.done) or len(rq.tokens) >= rq.params.max_new_tokens
            if rq.text_stop is not None and fresh and not rq.done:
                # the text-level backstop: a stop string the token match cannot see ends the request here
                if rq.text_stop.find(_decode_text(self.tokenizer, rq.tokens)) is not None:
                    rq.done = True

    def _show(self, rq, n):
        """``on_token`` for the tokens ``rq.shown .. n``, one call per token, each with its own entry (the entry of
        token j, not of the newest one: under a hold-back the two differ)."""
        for j in range(rq.shown + 1, n + 1):
            rq.shown = j
            try:
                if rq.logprobs is not None:
                    rq.on_token(j, list(rq.tokens[:j]), (rq.token_lp[j - 1], rq.top_lp[j - 1]))
                else:
                    rq.on_token(j, list(rq.tokens[:j]))
            except Exception:  # noqa: BLE001 - a consumer's failure is its own
                pass

    def _retire_done(self):
        # highest slot first: the page that moves into a freed slot is then never one that is itself finished
        for slot in range(len(self._active) - 1, -1, -1):
            rq = self._active[slot]
            if not rq.done:
                continue
            res = None
            if rq.guided is not None:  # how the automaton ended, while the slot is still live
                rq.guided_status = STATUS_NAMES.get(self._session.guided_state(slot)[1])
            if rq.stops is not None:
                res, moved = self._session.retire_stopped(slot, lambda t: _decode_text(self.tokenizer, t))
                ids = res.tokens
            else:
                ids, moved = self._session.retire(slot)
            last = len(self._active) - 1
            if moved >= 0:
                if moved != last:
                    raise RuntimeError(f"session moved slot {moved}, expected the last active slot {last}")
                self._active[slot] = self._active[last]
            self._active.pop()
            ids = [int(t) for t in ids][:rq.params.max_new_tokens]
            if res is not None and rq.on_token is not None:
                self._show(rq, len(ids))  # what the hold-back kept and no hit removed
            if res is not None:  # trimmed by the hit, the text cut at a stop string
                out = DecodeOutcome(normalize_text(res.text), len(rq.ids), len(ids), ids, stop_reason=res.stop_reason)
            else:
                out = DecodeOutcome(normalize_text(_decode_text(self.tokenizer, ids)), len(rq.ids), len(ids), ids)
            if rq.logprobs is not None:
                out.token_logprobs, out.top_logprobs = rq.token_lp[:len(ids)], rq.top_lp[:len(ids)]
            out.guided_status = rq.guided_status
            rq.future.set_result(out)

    def _run_exclusive(self, rq):
        self._close_session()  # a session and a generate exclude each other on one engine
        self.exclusive_runs += 1
        ckw = {} if rq.constraint is None else rq.constraint.kwargs()
        ckw.update(rq.stop_args)  # (a decode with stops does not stream either)
        if rq.penalties is not None:  # (nor does a penalised one)
            ckw.update(_penalty_kwargs(rq.penalties))
        if rq.ngram_window is not None:  # (nor one with a windowed ban)
            ckw.update(rq.ngram_window.kwargs())
        if rq.guided is not None:  # (nor a guided one)
            ckw["guided"] = rq.guided
        try:
            if rq.logprobs is None and not ckw:
                out = self.engine.decode(self.tokenizer, rq.prompt, rq.images, rq.vision, rq.params, rq.on_token)
            elif rq.logprobs is None:  # a constrained decode does not stream: the consumer gets the tokens afterwards
                out = self.engine.decode(self.tokenizer, rq.prompt, rq.images, rq.vision, rq.params, None, **ckw)
                if rq.on_token is not None:
                    toks = [int(t) for t in out.generated_tokens]
                    for i in range(len(toks)):
                        try:
                            rq.on_token(i + 1, toks[:i + 1])
                        except Exception:  # noqa: BLE001 - a consumer's failure is its own
                            pass
            else:  # the entries arrive with the ids: the consumer gets every token with its entry afterwards
                out = self.engine.decode(self.tokenizer, rq.prompt, rq.images, rq.vision, rq.params, None,
                                         logprobs=rq.logprobs, **ckw)
                if rq.on_token is not None:
                    toks = [int(t) for t in out.generated_tokens]
                    for i in range(len(toks)):
                        try:
                            rq.on_token(i + 1, toks[:i + 1], (out.token_logprobs[i], out.top_logprobs[i]))
                        except Exception:  # noqa: BLE001 - a consumer's failure is its own
                            pass
        except Exception as e:  # noqa: BLE001
            rq.future.set_exception(e)
            return
        rq.future.set_result(out)
