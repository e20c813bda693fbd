"""Per-request logit bias and token allow / deny sets (include/dsocr.h, dsocr_logit_bias).

The three request-level arguments ``logit_bias={id: value}``, ``allowed_token_ids=[...]`` and
``banned_token_ids=[...]`` are merged here, on the host, into the one constraint the engine takes: a list of
(id, value) pairs and the flag ``allow_only``.  Pure Python: nothing here needs the library or a device.
"""
from __future__ import annotations

import math
import operator
from dataclasses import dataclass, field
from typing import Iterable, Mapping, Optional

EINVAL = 1


class ConstraintError(ValueError):
    """A constraint the engine would refuse with DSOCR_EINVAL (status 1)."""
    status = EINVAL


@dataclass(frozen=True)
class LogitConstraint:
    """b[ids[i]] = values[i]; every other id gets 0, or -inf under ``allow_only``."""
    ids: tuple = field(default_factory=tuple)
    values: tuple = field(default_factory=tuple)
    allow_only: bool = False

    def kwargs(self) -> dict:
        """The arguments that merge back into this constraint (what ``decode`` / ``Session.admit`` take)."""
        kw = {"logit_bias": dict(zip(self.ids, self.values))}
        if self.allow_only:
            kw["allowed_token_ids"] = list(self.ids)
        return kw

    def dense(self, vocab: int):
        """The dense f32 row the device builds (numpy), for references and tests."""
        import numpy as np
        b = np.full(vocab, -np.inf if self.allow_only else 0.0, np.float32)
        if self.ids:
            b[list(self.ids)] = np.asarray(self.values, np.float32)
        return b


def _token_id(t, vocab: Optional[int]) -> int:
    try:
        if isinstance(t, bool):
            raise TypeError
        i = operator.index(t)
    except TypeError:
        raise ConstraintError(f"token id {t!r} is not an integer") from None
    if i < 0 or (vocab is not None and i >= vocab):
        raise ConstraintError(f"token id {i} outside the vocabulary" + ("" if vocab is None else f" [0, {vocab})"))
    return i


def merge_constraint(logit_bias: Optional[Mapping] = None, allowed_token_ids: Optional[Iterable] = None,
                     banned_token_ids: Optional[Iterable] = None, vocab: Optional[int] = None) -> Optional[LogitConstraint]:
    """One constraint from the three arguments, or None when they say nothing.

    * ``allowed_token_ids`` sets ``allow_only``: the listed ids get 0 (plus their ``logit_bias`` value, if any) and
      every other id -inf; a ``logit_bias`` entry on an id that is not allowed is dropped (the id stays at -inf).
      An empty list permits no token and is an error.
    * ``banned_token_ids`` get -inf, whatever ``logit_bias`` or ``allowed_token_ids`` say about them.
    * ``logit_bias`` values must be finite or -inf (NaN and +inf are errors).
    Ids are checked against ``vocab`` when it is given; repeated ids in a list count once.  The pairs come out in
    ascending id order, so equal arguments give equal constraints."""
    bias = {}
    for k, v in (logit_bias or {}).items():
        t = _token_id(k, vocab)
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ConstraintError(f"logit_bias[{t}] = {v!r} is not a number") from None
        if math.isnan(f) or f == math.inf:
            raise ConstraintError(f"logit_bias[{t}] is NaN or +inf")
        if t in bias:
            raise ConstraintError(f"duplicate token id {t} in logit_bias")
        bias[t] = f
    banned = {_token_id(t, vocab) for t in banned_token_ids} if banned_token_ids is not None else set()
    allow_only = allowed_token_ids is not None
    if allow_only:
        allowed = {_token_id(t, vocab) for t in allowed_token_ids}
        if not allowed:
            raise ConstraintError("allowed_token_ids is empty: no token may be emitted")
        entries = {t: bias.get(t, 0.0) for t in allowed}
    else:
        entries = dict(bias)
    for t in banned:
        if allow_only and t not in entries:
            continue  # (already -inf)
        entries[t] = -math.inf
    if not allow_only:
        entries = {t: v for t, v in entries.items() if v != 0.0}  # a zero bias says nothing
        if not entries:
            return None
    if vocab is not None and len(entries) > vocab:
        raise ConstraintError("more entries than the vocabulary has ids")
    ids = tuple(sorted(entries))
    return LogitConstraint(ids, tuple(entries[t] for t in ids), allow_only)
