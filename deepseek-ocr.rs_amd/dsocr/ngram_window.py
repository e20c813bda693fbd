"""Windowed no-repeat n-gram ban with a token whitelist: pure host code.

With ``ctx[0..n)`` the page's context (prompt and generated ids) and a record ``{ngram_size g, window w, whitelist}``
that is on (``g >= 2``), every start ``i`` in ``[max(0, n - w), n - g]`` with ``ctx[i .. i+g-1) == ctx[n-g+1 .. n)``
makes ``t = ctx[i+g-1]`` a candidate; a candidate inside the vocabulary and outside the whitelist gets ``l[t] = -inf``,
unless that would leave the row without a finite logit.  With ``w >= n`` and no whitelist this is the reference's
``no_repeat_ngram_size`` ban.  The engine, the scheduler, the server and the CLI validate through
``make_ngram_window``; ``apply`` is the NumPy reference the tests compare the kernel with.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

MAX_WHITELIST = 32       # DSOCR_MAX_NGRAM_WHITELIST
DEFAULT_WINDOW = 100     # the upstream processor's window_size when only ngram_size is sent
UNBOUNDED = 2 ** 31 - 1  # a window no context outgrows


class NgramWindowError(ValueError):
    pass


@dataclass(frozen=True)
class NgramWindow:
    ngram_size: int
    window: int
    whitelist: Tuple[int, ...] = ()

    @property
    def off(self) -> bool:
        return self.ngram_size < 2

    def kwargs(self) -> dict:
        """The record as the ``ngram_window=`` keyword ``decode`` / ``admit`` / ``submit`` take."""
        return {"ngram_window": self}


def _integer(name: str, v) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise NgramWindowError(f"{name} must be an integer")
    return int(v)


def make_ngram_window(ngram_size=None, window=None, whitelist=None, vocab: Optional[int] = None) -> Optional[NgramWindow]:
    """The three request arguments as one checked record, or None when they ask for nothing (``ngram_size`` absent or
    below 2).  ``window`` defaults to ``DEFAULT_WINDOW``.  ``NgramWindowError``: a value that is no integer, a negative
    ``ngram_size``, ``window < 1``, more than ``MAX_WHITELIST`` distinct whitelist ids, an id below 0 or, with
    ``vocab``, outside it.  Repeated whitelist ids count once; the record keeps them in first-seen order."""
    if isinstance(ngram_size, NgramWindow):
        if window is not None or whitelist is not None:
            raise NgramWindowError("a NgramWindow record takes no further arguments")
        ngram_size, window, whitelist = ngram_size.ngram_size, ngram_size.window, ngram_size.whitelist
    if whitelist is None:
        whitelist = ()
    if isinstance(whitelist, (str, bytes)) or not isinstance(whitelist, (Sequence, np.ndarray)):
        raise NgramWindowError("whitelist_token_ids must be a list of token ids")
    ids = []
    for t in whitelist:
        t = _integer("a whitelist id", t)
        if t < 0 or (vocab is not None and t >= vocab) or t > UNBOUNDED:
            raise NgramWindowError(f"whitelist id {t} lies outside the vocabulary")
        if t not in ids:
            ids.append(t)
    if len(ids) > MAX_WHITELIST:
        raise NgramWindowError(f"at most {MAX_WHITELIST} whitelist ids")
    if ngram_size is None:
        if window is not None or ids:
            raise NgramWindowError("window_size / whitelist_token_ids need ngram_size")
        return None
    g = _integer("ngram_size", ngram_size)
    if g < 0 or g > UNBOUNDED:
        raise NgramWindowError("ngram_size must be 0 (off) or at least 2")
    w = DEFAULT_WINDOW if window is None else _integer("window_size", window)
    if g < 2:
        if g == 1:
            raise NgramWindowError("ngram_size must be 0 (off) or at least 2")
        return None
    if w < 1 or w > UNBOUNDED:
        raise NgramWindowError("window_size must be at least 1")
    return NgramWindow(g, w, tuple(ids))


def candidates(ctx, ngram_size: int, window: int) -> list:
    """The continuations of every n-gram that starts within the last ``window`` context positions and repeats the
    context's (g-1)-token suffix, in start order, repeats included."""
    c = [int(t) for t in np.asarray(ctx).reshape(-1)]
    n, g = len(c), int(ngram_size)
    if g < 2 or n < g:
        return []
    suffix = c[n - g + 1:]
    return [c[i + g - 1] for i in range(max(0, n - int(window)), n - g + 1) if c[i:i + g - 1] == suffix]


def apply(logits, ctx, rec: Optional[NgramWindow]) -> np.ndarray:
    """The banned copy of one f32 logits row under ``rec`` (None or off: an unchanged copy): every candidate inside
    ``[0, len(logits))`` and outside the whitelist becomes -inf, unless no finite logit would be left."""
    out = np.array(logits, np.float32, copy=True)
    if rec is None or rec.off:
        return out
    V = out.shape[0]
    ban = sorted({t for t in candidates(ctx, rec.ngram_size, rec.window) if 0 <= t < V and t not in rec.whitelist})
    if not ban:
        return out
    banned = out.copy()
    banned[ban] = -np.inf
    return banned if np.isfinite(banned).any() else out
