"""Guided decoding: the token automaton a request may carry, and a compiler for ``guided_choice``.

Pure Python: nothing here needs the library.  The record is the C ABI's ``dsocr_guided``: states, a start state, a
byte per state (accepting: EOS may be selected there) and the edges in CSR form with ids ascending within a state.  A
state without an outgoing edge is terminal; reaching it completes the page.
"""
from __future__ import annotations

from bisect import bisect_left
from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

MAX_GUIDED_STATES = 1024       # DSOCR_MAX_GUIDED_STATES
MAX_GUIDED_EDGES = 1 << 20     # DSOCR_MAX_GUIDED_EDGES

STATUS_RUNNING, STATUS_COMPLETE, STATUS_VIOLATED = 0, 1, 2
STATUS_NAMES = {STATUS_RUNNING: None, STATUS_COMPLETE: "complete", STATUS_VIOLATED: "violated"}


class GuidedError(ValueError):
    """A bad automaton or choice list; ``status`` is the C ABI's DSOCR_EINVAL."""
    status = 1


@dataclass(frozen=True)
class TokenAutomaton:
    n_states: int
    start: int
    accepting: Tuple[int, ...]
    row_ptr: Tuple[int, ...]
    edge_tok: Tuple[int, ...]
    edge_next: Tuple[int, ...]

    def __post_init__(self):
        for name in ("accepting", "row_ptr", "edge_tok", "edge_next"):
            object.__setattr__(self, name, tuple(int(v) for v in getattr(self, name)))
        object.__setattr__(self, "n_states", int(self.n_states))
        object.__setattr__(self, "start", int(self.start))

    # ------------------------------------------------------------------ the C rules, in the C order
    def validate(self, vocab: int, eos: Optional[int] = None) -> "TokenAutomaton":
        n = self.n_states
        eos = -1 if eos is None or eos < 0 else int(eos)
        if n < 1 or n > MAX_GUIDED_STATES:
            raise GuidedError(f"n_states must be 1..{MAX_GUIDED_STATES}")
        if len(self.accepting) != n or len(self.row_ptr) != n + 1:
            raise GuidedError("accepting has n_states entries and row_ptr n_states + 1")
        if self.row_ptr[0] != 0:
            raise GuidedError("row_ptr must start at 0")
        if any(self.row_ptr[s + 1] < self.row_ptr[s] for s in range(n)):
            raise GuidedError("row_ptr must not decrease")
        e_n = self.row_ptr[n]
        if e_n > MAX_GUIDED_EDGES:
            raise GuidedError(f"more than {MAX_GUIDED_EDGES} edges")
        if len(self.edge_tok) != e_n or len(self.edge_next) != e_n:
            raise GuidedError("row_ptr must end at the number of edges")
        for s in range(n):
            for e in range(self.row_ptr[s], self.row_ptr[s + 1]):
                t = self.edge_tok[e]
                if t < 0 or t >= vocab:
                    raise GuidedError(f"token id {t} outside the vocabulary")
                if t == eos:
                    raise GuidedError("an edge on the EOS id (mark the state accepting instead)")
                if e > self.row_ptr[s] and self.edge_tok[e - 1] >= t:
                    raise GuidedError("token ids must ascend strictly within a state")
                if not 0 <= self.edge_next[e] < n:
                    raise GuidedError("edge_next outside [0, n_states)")
        if not 0 <= self.start < n:
            raise GuidedError("start outside [0, n_states)")
        if self.row_ptr[self.start] == self.row_ptr[self.start + 1]:
            raise GuidedError("the start state is terminal")
        return self

    # ------------------------------------------------------------------ what the kernels compute
    def edges(self, state: int) -> Tuple[Sequence[int], Sequence[int]]:
        a, b = self.row_ptr[state], self.row_ptr[state + 1]
        return self.edge_tok[a:b], self.edge_next[a:b]

    def terminal(self, state: int) -> bool:
        return self.row_ptr[state] == self.row_ptr[state + 1]

    def allowed(self, state: int, eos: Optional[int] = None) -> List[int]:
        """The ids the mask keeps in ``state``: its edges' and, in an accepting state, ``eos``."""
        if state < 0:
            return []
        ids = list(self.edges(state)[0])
        if eos is not None and eos >= 0 and self.accepting[state] and eos not in ids:
            ids.append(int(eos))
        return sorted(ids)

    def step(self, state: int, token: int) -> Tuple[int, int]:
        """(state, status) after ``token`` was appended in ``state``."""
        toks, nxt = self.edges(state)
        i = bisect_left(toks, token)
        if i == len(toks) or toks[i] != token:
            return -1, STATUS_VIOLATED
        ns = nxt[i]
        return ns, STATUS_COMPLETE if self.terminal(ns) else STATUS_RUNNING

    def walk(self, tokens: Iterable[int]) -> Tuple[int, int]:
        """(state, status) after a whole output; the walk stops where the device's does (complete or violated)."""
        state, status = self.start, STATUS_RUNNING
        for t in tokens:
            if status != STATUS_RUNNING:
                break
            state, status = self.step(state, int(t))
        return state, status

    def mask_row(self, state: int, vocab: int, eos: Optional[int] = None) -> np.ndarray:
        """The dense boolean row of ``state``: True where the mask keeps the logit."""
        row = np.zeros(vocab, dtype=bool)
        ids = [t for t in self.allowed(state, eos) if 0 <= t < vocab]
        row[ids] = True
        return row


def automaton_from_sequences(seqs: Iterable[Sequence[int]]) -> TokenAutomaton:
    """A trie over token-id sequences: shared prefixes merged, equal sequences once, a sequence's end accepting (a
    sequence that is a prefix of another leaves an accepting state with outgoing edges).  States are numbered
    breadth-first and edges ascend, so equal inputs give equal automata."""
    seqs = [tuple(int(t) for t in s) for s in seqs]
    if not seqs:
        raise GuidedError("no sequences")
    if any(len(s) == 0 for s in seqs):
        raise GuidedError("an empty sequence")
    children: List[dict] = [{}]
    accept: List[bool] = [False]
    for s in sorted(set(seqs)):
        node = 0
        for t in s:
            nxt = children[node].get(t)
            if nxt is None:
                nxt = len(children)
                children.append({})
                accept.append(False)
                children[node][t] = nxt
            node = nxt
        accept[node] = True
    # breadth-first renumbering, children in ascending id order
    order, number = [0], {0: 0}
    for node in order:
        for t in sorted(children[node]):
            c = children[node][t]
            number[c] = len(order)
            order.append(c)
    if len(order) > MAX_GUIDED_STATES:
        raise GuidedError(f"the choices need {len(order)} states, more than {MAX_GUIDED_STATES}")
    row_ptr, edge_tok, edge_next = [0], [], []
    for node in order:
        for t in sorted(children[node]):
            edge_tok.append(t)
            edge_next.append(number[children[node][t]])
        row_ptr.append(len(edge_tok))
    return TokenAutomaton(len(order), 0, tuple(int(accept[n]) for n in order), tuple(row_ptr), tuple(edge_tok),
                          tuple(edge_next))


def choice_automaton(tokenizer, strings: Sequence[str]) -> TokenAutomaton:
    """``guided_choice``: each string as ``tokenizer.encode(s, add_special_tokens=False)``, then the trie."""
    if isinstance(strings, (str, bytes)) or not isinstance(strings, (list, tuple)):
        raise GuidedError("guided_choice must be a list of strings")
    if not strings:
        raise GuidedError("guided_choice is empty")
    seqs = []
    for s in strings:
        if not isinstance(s, str) or s == "":
            raise GuidedError("guided_choice entries must be non-empty strings")
        enc = tokenizer.encode(s, add_special_tokens=False)
        ids = list(enc.ids) if hasattr(enc, "ids") else list(enc)
        if not ids:
            raise GuidedError(f"choice {s!r} encodes to no token")
        seqs.append(ids)
    return automaton_from_sequences(seqs)


def automaton_from_mapping(obj) -> TokenAutomaton:
    """The raw ``token_automaton`` object of a request: the six fields, all required."""
    fields = ("n_states", "start", "accepting", "row_ptr", "edge_tok", "edge_next")
    if not isinstance(obj, dict):
        raise GuidedError("token_automaton must be an object")
    extra = set(obj) - set(fields)
    if extra:
        raise GuidedError(f"unknown field {sorted(extra)[0]!r}")
    missing = [f for f in fields if f not in obj]
    if missing:
        raise GuidedError(f"missing field {missing[0]!r}")

    def _int(v, name):
        if isinstance(v, bool) or not isinstance(v, int):
            raise GuidedError(f"{name} must hold integers")
        return v

    def _ints(v, name):
        if not isinstance(v, (list, tuple)):
            raise GuidedError(f"{name} must be a list of integers")
        return tuple(_int(x, name) for x in v)

    return TokenAutomaton(_int(obj["n_states"], "n_states"), _int(obj["start"], "start"),
                          tuple(1 if x else 0 for x in _ints(obj["accepting"], "accepting")),
                          _ints(obj["row_ptr"], "row_ptr"), _ints(obj["edge_tok"], "edge_tok"),
                          _ints(obj["edge_next"], "edge_next"))
