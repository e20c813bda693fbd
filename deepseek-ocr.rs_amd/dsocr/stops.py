"""Stop sequences, per request (include/dsocr.h, dsocr_stop_set).

The request-level arguments ``stop`` (a string or a list of strings) and ``stop_token_ids`` (a list of token ids) are
merged here, on the host, into the one stop set the engine takes: at most 16 sequences of 1..32 token ids.  The device
matches them inside the decode step and ends the page on the step that completes one; it never trims.  Trimming, the
hold-back of a stream's tail and the text-level backstop (a stop string can also arise from a tokenisation other than
its canonical one) are host work and live here too.  Pure Python: nothing here needs the library or a device.
"""
from __future__ import annotations

import operator
from dataclasses import dataclass, field
from typing import Iterable, Optional, Sequence, Union

EINVAL = 1
MAX_STOP_SEQS = 16  # DSOCR_MAX_STOP_SEQS
MAX_STOP_LEN = 32   # DSOCR_MAX_STOP_LEN


class StopError(ValueError):
    """A stop set the engine would refuse with DSOCR_EINVAL (status 1)."""
    status = EINVAL


@dataclass(frozen=True)
class StopSet:
    """``seqs[i]`` is a tuple of token ids; ``labels[i]`` is what ``stop_reason`` reports for it (the stop string, or
    the token id of a ``stop_token_ids`` entry); ``strings`` are the stop strings, for the text-level backstop."""
    seqs: tuple = field(default_factory=tuple)
    labels: tuple = field(default_factory=tuple)
    strings: tuple = field(default_factory=tuple)

    def kwargs(self) -> dict:
        """The argument that carries this set on (what ``Session.admit`` and its kin take)."""
        return {"stops": self}


def _token_id(t, vocab: Optional[int]) -> int:
    try:
        if isinstance(t, bool):
            raise TypeError
        i = operator.index(t)
    except TypeError:
        raise StopError(f"token id {t!r} is not an integer") from None
    if i < 0 or (vocab is not None and i >= vocab):
        raise StopError(f"token id {i} outside the vocabulary" + ("" if vocab is None else f" [0, {vocab})"))
    return i


def check_sequences(seqs: Sequence[Sequence[int]], vocab: Optional[int] = None) -> None:
    """dsocr_stop_set_check on the host: more than 16 sequences, a length of 0 or above 32, an id outside
    [0, vocab), two identical sequences."""
    if len(seqs) > MAX_STOP_SEQS:
        raise StopError(f"{len(seqs)} stop sequences (at most {MAX_STOP_SEQS})")
    seen = set()
    for s in seqs:
        if not 1 <= len(s) <= MAX_STOP_LEN:
            raise StopError(f"a stop sequence of {len(s)} token ids (1..{MAX_STOP_LEN})")
        t = tuple(_token_id(x, vocab) for x in s)
        if t in seen:
            raise StopError(f"stop sequence {list(t)} is listed twice")
        seen.add(t)


def merge_stops(stop: Union[None, str, Iterable[str]] = None, stop_token_ids: Optional[Iterable] = None, tokenizer=None,
                vocab: Optional[int] = None) -> Optional[StopSet]:
    """One stop set from the two arguments, or None when they say nothing.

    * a string of ``stop`` is encoded without special tokens into one id sequence (``tokenizer.encode(text,
      add_special_tokens=False).ids``); an empty string, or one that encodes to no id or to more than 32, is an error;
    * each entry of ``stop_token_ids`` is a sequence of length 1;
    * duplicates collapse (the first label stays); more than 16 sequences after that is an error.
    Ids are checked against ``vocab`` when it is given."""
    if isinstance(stop, str):
        stop = [stop]
    seqs, labels, strings = [], [], []
    index = {}

    def add(seq, label):
        if seq not in index:
            index[seq] = len(seqs)
            seqs.append(seq)
            labels.append(label)

    if stop is not None:
        try:
            items = list(stop)
        except TypeError:
            raise StopError("`stop` must be a string or a list of strings") from None
        for text in items:
            if not isinstance(text, str):
                raise StopError(f"stop {text!r} is not a string")
            if not text:
                raise StopError("an empty stop string")
            if tokenizer is None:
                raise StopError("a stop string needs a tokenizer")
            ids = tuple(int(t) for t in tokenizer.encode(text, add_special_tokens=False).ids)
            if not 1 <= len(ids) <= MAX_STOP_LEN:
                raise StopError(f"stop {text!r} encodes to {len(ids)} token ids (1..{MAX_STOP_LEN})")
            for t in ids:
                _token_id(t, vocab)
            add(ids, text)
            if text not in strings:
                strings.append(text)
    if stop_token_ids is not None:
        try:
            items = list(stop_token_ids)
        except TypeError:
            raise StopError("`stop_token_ids` must be a list of token ids") from None
        for t in items:
            i = _token_id(t, vocab)
            add((i,), i)
    if not seqs:
        return None
    if len(seqs) > MAX_STOP_SEQS:
        raise StopError(f"{len(seqs)} stop sequences (at most {MAX_STOP_SEQS})")
    return StopSet(tuple(seqs), tuple(labels), tuple(strings))


def first_stop(ids: Sequence[int], seqs: Sequence[Sequence[int]]):
    """Where the device stops on the stream ``ids``: ``(end_index, seq)`` with ``end_index`` = the number of tokens
    emitted when the first match completes and ``seq`` the lowest matching index there; None when nothing matches.
    The reference of the tests: the tail after every token against every sequence, in order."""
    ids = [int(t) for t in ids]
    for L in range(1, len(ids) + 1):
        for s, q in enumerate(seqs):
            m = len(q)
            if 1 <= m <= L and ids[L - m:L] == [int(t) for t in q]:
                return L, s
    return None


class TokenHoldback:
    """Withholds from a token stream the longest tail that is a proper prefix of some stop sequence, so that no id
    is handed out that a later hit removes.  ``feed(tokens)`` -> how many leading tokens are safe to show now;
    ``finish(tokens, match_len)`` -> how many to show in the end (the matched ones dropped, or everything)."""

    def __init__(self, seqs: Sequence[Sequence[int]], include_stop: bool = False):
        self.seqs = [tuple(int(t) for t in q) for q in seqs]
        self.include = bool(include_stop)
        self.released = 0

    def _held(self, tokens) -> int:
        n = len(tokens)
        best = 0
        for q in self.seqs:
            for k in range(min(len(q), n), best, -1):  # (a whole sequence at the tail is the hit itself: held too)
                if tuple(tokens[n - k:]) == q[:k]:
                    best = k
                    break
        return best

    def feed(self, tokens) -> int:
        tokens = [int(t) for t in tokens]
        if self.include:
            self.released = len(tokens)
        else:
            self.released = max(self.released, len(tokens) - self._held(tokens))
        return self.released

    def finish(self, tokens, match_len: int = 0) -> int:
        n = len(tokens)
        keep = n if self.include or match_len <= 0 else n - int(match_len)
        self.released = max(self.released, keep) if match_len <= 0 else keep
        return keep


class TextStop:
    """The text-level backstop: searches the accumulated text for the stop strings after every delta.

    ``advance(text, final)`` -> ``(safe, hit)``: ``safe`` is the text that may be shown now and ``hit`` the stop
    string found, or None.  Without a hit the longest tail of ``text`` that is a proper prefix of some stop string is
    held back (released when ``final``).  On a hit the text is cut in front of the stop (behind it with
    ``include_stop``), later calls return the same, and the caller retires the slot.  Of several stops the one that
    completes first wins (then the one listed first): what a character-by-character stream would see.  A cut never
    goes below what an earlier call handed out."""

    def __init__(self, strings: Sequence[str], include_stop: bool = False):
        self.strings = [s for s in strings if s]
        self.include = bool(include_stop)
        self.shown = 0
        self.hit: Optional[str] = None
        self.final_text: Optional[str] = None

    def find(self, text: str):
        best = None
        for i, s in enumerate(self.strings):
            at = text.find(s)
            if at >= 0:
                key = (at + len(s), i)
                if best is None or key < best[0]:
                    best = (key, at, s)
        return best

    def _held(self, text: str) -> int:
        n = len(text)
        best = 0
        for s in self.strings:
            for k in range(min(len(s) - 1, n), best, -1):
                if text.endswith(s[:k]):
                    best = k
                    break
        return best

    def advance(self, text: str, final: bool = False):
        if self.final_text is not None:
            return self.final_text, self.hit
        if not self.strings:
            self.shown = len(text)
            return text, None
        found = self.find(text)
        if found is not None:
            (end, _), at, s = found
            cut = max(end if self.include else at, self.shown)
            self.hit, self.final_text, self.shown = s, text[:cut], cut
            return self.final_text, s
        keep = len(text) if final else len(text) - self._held(text)
        self.shown = max(self.shown, min(keep, len(text)))
        return text[:self.shown], None


@dataclass
class StopResult:
    tokens: list
    text: str
    stop_reason: Union[None, str, int] = None
    entries: int = 0  # log-probability entries that stay (= len(tokens))


def apply_stops(decode, ids: Sequence[int], stops: Optional[StopSet], hit_seq: int = -1, match_len: int = 0,
                include_stop: bool = False) -> StopResult:
    """The host's part after a page ended: ``ids`` as the device returned them (matched tokens included), the
    device's hit, ``decode(ids) -> text``.  The matched ids are trimmed unless ``include_stop``; then the text-level
    backstop cuts the text at a stop string the token match could not see, and the ids are cut to the longest prefix
    whose text fits in front of it (with ``include_stop``: the shortest prefix whose text holds the stop)."""
    ids = [int(t) for t in ids]
    if stops is None:
        return StopResult(ids, decode(ids), None, len(ids))
    reason = None
    if hit_seq is not None and 0 <= hit_seq < len(stops.labels):
        reason = stops.labels[hit_seq]
        if not include_stop:
            ids = ids[:max(len(ids) - int(match_len), 0)]
    text = decode(ids)
    if stops.strings:
        ts = TextStop(stops.strings, include_stop)
        cut, found = ts.advance(text, True)
        if found is not None and (len(cut) < len(text) or reason is None):
            # the tokens whose text the cut keeps (decode lengths grow with the prefix)
            lo, hi = 0, len(ids)
            if include_stop:
                while lo < hi:  # shortest prefix whose text reaches the end of the stop
                    mid = (lo + hi) // 2
                    if len(decode(ids[:mid])) >= len(cut):
                        hi = mid
                    else:
                        lo = mid + 1
            else:
                while lo < hi:  # longest prefix whose text does not pass the cut
                    mid = (lo + hi + 1) // 2
                    if len(decode(ids[:mid])) <= len(cut):
                        lo = mid
                    else:
                        hi = mid - 1
            ids, text, reason = ids[:lo], cut, found
    return StopResult(ids, text, reason, len(ids))
