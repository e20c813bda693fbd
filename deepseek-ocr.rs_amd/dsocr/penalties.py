"""Frequency / presence penalties and min-p of one request: pure host code.

With ``c[t]`` the number of times id ``t`` occurs in the page's generated tokens so far, every step's logits become
``l[t] - (frequency * c[t] + presence)`` where ``c[t] > 0`` (f32, each operation rounded); ``min_p`` keeps, on sampled
rows, the candidates with ``logit / T - max(logit / T) >= log(min_p)``.  The engine, the scheduler, the server and the
CLI validate through ``make_penalties``; ``apply`` and ``min_p_keep`` are the NumPy references the tests compare the
kernels with.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np


class PenaltyError(ValueError):
    pass


@dataclass(frozen=True)
class Penalties:
    frequency: float = 0.0
    presence: float = 0.0
    min_p: float = 0.0

    @property
    def off(self) -> bool:
        return is_off(self.frequency, self.presence, self.min_p)

    @property
    def ln_min_p(self) -> float:
        return ln_min_p(self.min_p)


def is_off(frequency: float, presence: float, min_p: float) -> bool:
    """The record asks for nothing: ``frequency == 0 && presence == 0 && min_p <= 0``."""
    return frequency == 0 and presence == 0 and min_p <= 0


def ln_min_p(min_p: float) -> float:
    """``log(min_p)`` in f64 as the device record carries it; ``-inf`` means no filter."""
    return math.log(min_p) if min_p > 0 else -math.inf


def _number(name: str, v) -> float:
    if v is None:
        return 0.0
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise PenaltyError(f"{name} must be a number")
    return float(v)


def make_penalties(frequency_penalty=None, presence_penalty=None, min_p=None,
                   bound: Optional[float] = None) -> Optional[Penalties]:
    """The three request arguments as one checked record, or None when they ask for nothing.  A non-finite penalty,
    or ``min_p`` that is NaN or outside [0, 1], raises ``PenaltyError``; ``bound`` (the server: 2.0, OpenAI's range)
    additionally limits the magnitude of the two penalties.  The penalties are rounded to f32, as the engine holds
    them."""
    f = _number("frequency_penalty", frequency_penalty)
    p = _number("presence_penalty", presence_penalty)
    m = _number("min_p", min_p)
    for name, v in (("frequency_penalty", f), ("presence_penalty", p)):
        with np.errstate(over="ignore"):
            finite = math.isfinite(v) and math.isfinite(float(np.float32(v)))
        if not finite:
            raise PenaltyError(f"{name} must be finite")
        if bound is not None and abs(v) > bound:
            raise PenaltyError(f"{name} must lie in [-{bound:g}, {bound:g}]")
    if math.isnan(m) or m < 0 or m > 1:
        raise PenaltyError("min_p must lie in [0, 1]")
    f, p = float(np.float32(f)), float(np.float32(p))
    if is_off(f, p, m):
        return None
    return Penalties(f, p, m)


def apply(logits, out_ids, frequency: float, presence: float) -> np.ndarray:
    """The penalised copy of one f32 logits row: for every id ``t`` in [0, len(logits)) that occurs ``c > 0`` times in
    ``out_ids``, ``l[t] - (frequency * c + presence)`` with one f32 multiply, add and subtract, each rounded."""
    out = np.array(logits, np.float32, copy=True)
    if frequency == 0 and presence == 0:
        return out
    ids = np.asarray(out_ids, np.int64).reshape(-1)
    ids = ids[(ids >= 0) & (ids < out.shape[0])]
    if ids.size == 0:
        return out
    uniq, cnt = np.unique(ids, return_counts=True)
    fr, pr = np.float32(frequency), np.float32(presence)
    with np.errstate(invalid="ignore", over="ignore"):
        pen = (fr * cnt.astype(np.float32)).astype(np.float32) + pr
        out[uniq] = (out[uniq] - pen.astype(np.float32)).astype(np.float32)
    return out


def min_p_keep(q, ln_mp: float) -> np.ndarray:
    """The min-p condition on f64 candidate values ``q`` (finite, unbanned): ``q - max(q) >= ln_min_p``."""
    q = np.asarray(q, np.float64)
    if q.size == 0 or ln_mp == -math.inf:
        return np.ones(q.shape, bool)
    return (q - q.max()) >= ln_mp
