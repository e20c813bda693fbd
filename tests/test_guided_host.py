"""Guided decoding, the host side: the trie compiler, the validation rules (Python and
``dsocr_guided_check`` must agree on every one), the server's request parsing and the exported symbols.  No GPU."""
import ctypes as C
import os

import pytest

from dsocr._lib import lib
from dsocr.engine import _guided_c
from dsocr.guided import (MAX_GUIDED_EDGES, MAX_GUIDED_STATES, GuidedError, TokenAutomaton, automaton_from_mapping,
                          automaton_from_sequences, choice_automaton)
from dsocr.synth import SyntheticTokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB, EOS = 512, 1


# ------------------------------------------------------------------ the trie
def test_trie_shared_prefixes_nested_and_duplicates():
    seqs = [[5, 6, 7], [5, 6], [5, 9], [8], [5, 6, 7]]  # a nested pair, a shared prefix, a duplicate
    a = automaton_from_sequences(seqs)
    # states: root, 5, 8, 5-6, 5-9, 5-6-7
    assert a.n_states == 6 and a.start == 0
    assert a.row_ptr == (0, 2, 4, 4, 5, 5, 5) and a.edge_tok == (5, 8, 6, 9, 7) and a.edge_next == (1, 2, 3, 4, 5)
    assert a.accepting == (0, 0, 1, 1, 1, 1)
    a.validate(VOCAB, EOS)
    assert automaton_from_sequences(reversed(seqs)) == a and automaton_from_sequences([tuple(s) for s in seqs]) == a
    # status 1 exactly at a leaf: [5, 6] is accepting with an outgoing edge (running, EOS allowed), [5, 6, 7] a leaf
    assert a.walk([5]) == (1, 0) and a.walk([5, 6]) == (3, 0) and a.walk([5, 6, 7]) == (5, 1)
    assert a.walk([8]) == (2, 1) and a.walk([5, 9]) == (4, 1)
    assert a.walk([5, 7]) == (-1, 2) and a.walk([5, 7, 6]) == (-1, 2)  # the walk stops where the device does
    assert a.walk([8, 5]) == (2, 1)
    assert a.allowed(3, EOS) == [EOS, 7] and a.allowed(1, EOS) == [6, 9] and a.allowed(5, EOS) == [EOS]
    row = a.mask_row(3, VOCAB, EOS)
    assert row.sum() == 2 and row[7] and row[EOS] and a.mask_row(0, VOCAB, EOS).nonzero()[0].tolist() == [5, 8]
    for bad in ([], [[]], [[1], []]):
        with pytest.raises(GuidedError):
            automaton_from_sequences(bad)


def test_choice_automaton_with_the_synthetic_tokenizer():
    tok = SyntheticTokenizer(VOCAB)
    strings = ["<7> <8> <9>", "<7> <8>", "<20>"]
    a = choice_automaton(tok, strings)
    seqs = [list(tok.encode(s, add_special_tokens=False).ids) if hasattr(tok.encode(s, add_special_tokens=False), "ids")
            else list(tok.encode(s, add_special_tokens=False)) for s in strings]
    assert a == automaton_from_sequences(seqs)
    assert a.walk(seqs[0])[1] == 1 and a.walk(seqs[2])[1] == 1 and a.walk(seqs[1])[1] == 0
    for bad in ([], [""], ["<7>", ""], "abc", [7], None):
        with pytest.raises(GuidedError):
            choice_automaton(tok, bad)


# ------------------------------------------------------------------ validation: Python and C agree rule by rule
def _ok():
    return dict(n_states=3, start=0, accepting=(0, 1, 1), row_ptr=(0, 2, 3, 3), edge_tok=(4, 9, 4), edge_next=(1, 2, 2))


def _c_check(a: TokenAutomaton, vocab=VOCAB, eos=EOS) -> int:
    keep = []
    rec = _guided_c(a, keep)
    return lib().dsocr_guided_check(C.byref(rec), vocab, eos)


RULES = {
    "n_states 0": dict(n_states=0, accepting=(), row_ptr=(0,), edge_tok=(), edge_next=()),
    "n_states above the cap": dict(n_states=MAX_GUIDED_STATES + 1, accepting=(0,) * (MAX_GUIDED_STATES + 1),
                                   row_ptr=(0, 1) + (1,) * MAX_GUIDED_STATES, edge_tok=(4,), edge_next=(1,)),
    "row_ptr does not start at 0": dict(row_ptr=(1, 2, 3, 3)),
    "row_ptr decreases": dict(row_ptr=(0, 2, 1, 3)),
    "token below 0": dict(edge_tok=(-1, 9, 4)),
    "token at vocab": dict(edge_tok=(4, VOCAB, 4)),
    "token equals EOS": dict(edge_tok=(EOS, 9, 4)),
    "tokens not ascending": dict(edge_tok=(9, 4, 4)),
    "tokens equal": dict(edge_tok=(4, 4, 4)),
    "edge_next below 0": dict(edge_next=(1, -1, 2)),
    "edge_next at n_states": dict(edge_next=(1, 3, 2)),
    "start below 0": dict(start=-1),
    "start at n_states": dict(start=3),
    "terminal start": dict(start=2),
}


def test_the_good_automaton_passes_both():
    a = TokenAutomaton(**_ok())
    assert a.validate(VOCAB, EOS) is a and _c_check(a) == 0
    assert lib().dsocr_guided_check(None, VOCAB, EOS) == 0  # NULL: no automaton
    # without an EOS id (negative) an edge on id 1 is an ordinary edge
    b = TokenAutomaton(**dict(_ok(), edge_tok=(EOS, 9, 4)))
    assert b.validate(VOCAB, None) is b and _c_check(b, eos=-1) == 0


@pytest.mark.parametrize("rule", sorted(RULES))
def test_every_refusal_rule(rule):
    a = TokenAutomaton(**dict(_ok(), **RULES[rule]))
    with pytest.raises(GuidedError) as ei:
        a.validate(VOCAB, EOS)
    assert ei.value.status == 1
    assert _c_check(a) == 1, rule
    assert "token automaton" in str(lib().dsocr_last_error())


def test_the_edge_cap():
    """E over the cap: one state that loops on 2^20 + 1 ids of a (large enough) vocabulary."""
    E = MAX_GUIDED_EDGES + 1
    a = TokenAutomaton(1, 0, (1,), (0, E), range(2, E + 2), (0,) * E)
    with pytest.raises(GuidedError):
        a.validate(E + 2, EOS)
    assert _c_check(a, vocab=E + 2) == 1
    ok = TokenAutomaton(1, 0, (1,), (0, E - 1), range(2, E + 1), (0,) * (E - 1))
    assert ok.validate(E + 2, EOS) is ok and _c_check(ok, vocab=E + 2) == 0


# ------------------------------------------------------------------ the server's parsing
class _StubEngine:
    vocab = VOCAB


def test_server_parsing():
    from dsocr.server import ApiError, parse_guided
    tok = SyntheticTokenizer(VOCAB)
    want = choice_automaton(tok, ["<7> <8>", "<9>"])
    assert parse_guided({}, tok, VOCAB) is None and parse_guided({"guided_choice": None}, tok, VOCAB) is None
    for body in ({"guided_choice": ["<7> <8>", "<9>"]}, {"structured_outputs": {"choice": ["<9>", "<7> <8>"]}},
                 {"vllm_xargs": {"guided_choice": ["<7> <8>", "<9>"]}},
                 {"vllm_xargs": {"structured_outputs": {"choice": ["<7> <8>", "<9>"]}}}):
        assert parse_guided(body, tok, VOCAB) == {"guided": want}
    raw = dict(n_states=2, start=0, accepting=[0, 1], row_ptr=[0, 1, 1], edge_tok=[7], edge_next=[1])
    assert parse_guided({"token_automaton": raw}, tok, VOCAB) == {"guided": TokenAutomaton(2, 0, (0, 1), (0, 1, 1), (7,), (1,))}
    assert parse_guided({"vllm_xargs": {"token_automaton": raw}}, tok, VOCAB)["guided"].n_states == 2
    # a top-level field wins over vllm_xargs
    assert parse_guided({"guided_choice": ["<9>"], "vllm_xargs": {"guided_choice": ["<7>"]}}, tok, VOCAB) == \
        {"guided": choice_automaton(tok, ["<9>"])}
    bad = [{"guided_choice": []}, {"guided_choice": "yes"}, {"guided_choice": [""]}, {"guided_choice": [3]},
           {"structured_outputs": {"json": {}}}, {"structured_outputs": ["a"]}, {"structured_outputs": {"choice": []}},
           {"vllm_xargs": 5}, {"guided_choice": ["<7>"], "token_automaton": raw},
           {"token_automaton": dict(raw, extra=1)}, {"token_automaton": {k: v for k, v in raw.items() if k != "start"}},
           {"token_automaton": dict(raw, edge_tok=[VOCAB])}, {"token_automaton": dict(raw, start=1)},
           {"token_automaton": dict(raw, row_ptr="0,1,1")}, {"token_automaton": [1]}]
    for body in bad:
        with pytest.raises(ApiError) as ei:
            parse_guided(body, tok, VOCAB)
        assert ei.value.status == 400, body


def test_server_answers_400_and_passes_the_automaton_on():
    """The endpoints with a stub engine: a bad value answers 400 before any decode; a good one reaches
    ``engine.decode`` as ``guided=`` and the response carries ``guided_status``."""
    from starlette.testclient import TestClient

    from dsocr import DecodeParameters, VisionSettings, server
    from dsocr.engine import DecodeOutcome
    tok = SyntheticTokenizer(VOCAB)
    calls = []

    class Stub(_StubEngine):
        def decode(self, tokenizer, prompt, images, vision, params, stream=None, **kw):
            calls.append(kw)
            return DecodeOutcome("<7> <8>", 4, 2, [7, 8], None, None, None, "complete")

    st = server.ServerState(Stub(), tok, "deepseek-ocr", VisionSettings(256, 128, True), DecodeParameters(max_new_tokens=8))
    c = TestClient(server.create_app(st))
    msg = [{"role": "user", "content": [{"type": "text", "text": "<image>\nWhich?"}]}]
    r = c.post("/v1/chat/completions", json={"model": "deepseek-ocr", "messages": msg, "guided_choice": []})
    assert r.status_code == 400 and not calls
    r = c.post("/v1/responses", json={"model": "deepseek-ocr", "input": msg, "structured_outputs": {"regex": "a"}})
    assert r.status_code == 400 and not calls
    r = c.post("/v1/chat/completions", json={"model": "deepseek-ocr", "messages": msg, "guided_choice": ["<7> <8>", "<9>"]})
    assert r.status_code == 200, r.text
    assert calls[-1]["guided"] == choice_automaton(tok, ["<7> <8>", "<9>"])
    ch = r.json()["choices"][0]
    assert ch["guided_status"] == "complete" and ch["finish_reason"] == "stop"
    r = c.post("/v1/responses", json={"model": "deepseek-ocr", "input": msg, "vllm_xargs": {"guided_choice": ["<9>"]}})
    assert r.status_code == 200 and r.json()["guided_status"] == "complete"
    r = c.post("/v1/chat/completions", json={"model": "deepseek-ocr", "messages": msg})
    assert "guided_status" not in r.json()["choices"][0] and "guided" not in calls[-1]


# ------------------------------------------------------------------ the library
def test_symbols_are_exported():
    names = ["dsocr_guided_check", "dsocr_generate_guided", "dsocr_session_stage_guided", "dsocr_session_guided_state",
             "dsocr_k_guided_mask", "dsocr_k_guided_advance"]
    L = lib()
    for n in names:
        assert hasattr(L, n), n
    header = open(os.path.join(ROOT, "include", "dsocr.h")).read()
    for n in names + ["DSOCR_SESSION_GUIDED 64u", "DSOCR_MAX_GUIDED_STATES 1024", "DSOCR_MAX_GUIDED_EDGES (1 << 20)"]:
        assert n in header, n


# ------------------------------------------------------------------ scheduler routing, the server switch, the CLI
def _scripted():
    """tests/test_logit_bias_host.py's scripted engine, its session extended by ``guided_state``."""
    from test_logit_bias_host import FakeEngine, FakeSession, _sched

    class Session(FakeSession):
        def guided_state(self, slot):
            self.eng.log.append(("guided_state", self.active[slot]["key"]))
            return (5, 1)

    class Engine(FakeEngine):
        def open_session(self, slots, max_context, params, **kw):
            return Session(self, slots, max_context, params, kw)

    return Engine(), _sched


def test_scheduler_shared_and_exclusive_paths():
    import numpy as np
    img = np.zeros((8, 8, 3), np.uint8)
    aut = automaton_from_sequences([[7, 8], [9]])
    eng, _sched = _scripted()
    with _sched(eng, guided=True) as s:          # the flag: a guided request shares the session
        plain = s.submit("11", [img]).result(timeout=20)
        out = s.submit("12", [img], guided=aut).result(timeout=20)
        assert s.exclusive_runs == 0
    assert eng.log[0] == ("open", {"guided": True})
    assert ("admit", 11, {}) in eng.log and ("admit", 12, {"guided": aut}) in eng.log
    assert out.guided_status == "complete" and plain.guided_status is None
    assert ("guided_state", 12) in eng.log and ("guided_state", 11) not in eng.log
    eng, _sched = _scripted()
    with _sched(eng) as s:                       # no flag: it drains the session and decodes alone, with the argument
        s.submit("11", [img]).result(timeout=20)
        s.submit("12", [img], guided=aut).result(timeout=20)
        assert s.exclusive_runs == 1
        for bad in (TokenAutomaton(**dict(_ok(), start=2)), TokenAutomaton(**dict(_ok(), edge_tok=(4, 512, 4))), [[7]]):
            with pytest.raises(ValueError):
                s.submit("13", [img], guided=bad).result(timeout=20)
    assert eng.log[0] == ("open", {}) and ("decode", 12, {"guided": aut}) in eng.log
    assert not any(e[1] == 13 for e in eng.log if e[0] in ("decode", "admit"))


def test_guided_retry_on_a_cached_page_is_a_prefix_hit():
    import numpy as np
    img = np.random.default_rng(3).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    aut = automaton_from_sequences([[7, 8], [9]])
    eng, _sched = _scripted()
    with _sched(eng, guided=True, prefix_cache=4) as s:
        s.submit("11", [img]).result(timeout=20)
        s.submit("12", [img.copy()], guided=aut).result(timeout=20)
        assert (s.prefix_hits, s.prefix_misses) == (1, 1)
    assert ("admit", 11, {}) in eng.log and ("admit_prefix", 12, {"guided": aut}) in eng.log


def test_server_switch_and_cli_option(capsys):
    import argparse

    from dsocr import DecodeParameters, DsocrError, VisionSettings, cli, server
    p = argparse.ArgumentParser()
    server.add_scheduler_args(p)
    assert p.parse_args([]).guided is False and p.parse_args(["--slots", "2", "--guided"]).guided is True
    eng, _ = _scripted()
    st = server.ServerState(eng, SyntheticTokenizer(VOCAB), "deepseek-ocr", VisionSettings(256, 128, True),
                            DecodeParameters(max_new_tokens=8))
    with pytest.raises(ValueError, match="--slots"):
        server.make_scheduler(st, 0, 128, guided=True)
    on = server.make_scheduler(st, 2, 128, guided=True)
    try:
        assert on.guided is True
    finally:
        on.close()
    with pytest.raises(SystemExit):
        server.main(["--guided"])
    assert "--guided needs --slots" in capsys.readouterr().err
    tok = SyntheticTokenizer(VOCAB)
    parse = lambda *argv: cli.build_parser().parse_args(["--prompt", "x", *argv])
    a = parse("--guided-choice", "<7> <8>", "--guided-choice", "<9>")
    assert cli.guided_choices(a) == ["<7> <8>", "<9>"] and cli.token_constraint(a) == {}
    assert cli.guided_arguments(a, tok) == {"guided": choice_automaton(tok, ["<7> <8>", "<9>"])}
    assert cli.guided_arguments(parse(), tok) == {} and cli.guided_choices(parse()) == []
    for argv in (["--guided-choice", ""], ["--guided-choice", "<7>", "--slots", "2"]):
        with pytest.raises(DsocrError) as ei:
            cli.token_constraint(parse(*argv))
        assert ei.value.status == 1
