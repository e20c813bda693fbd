"""Per-token log-probabilities above the engine, without a GPU: the C ABI exports, the scheduler, the server's chat
completions surface and the CLI, against a scripted engine of this file's own."""
import ctypes as C
import io
import json
import math
import os
import re
import threading

import pytest

from dsocr import DecodeOutcome, DecodeParameters, VisionSettings
from dsocr import cli, server
from dsocr.synth import SyntheticTokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dsocr_generate_logprobs", "dsocr_session_logprobs", "dsocr_k_logprobs", "dsocr_k_logprobs_penalty"]


def test_c_abi_exports_and_signatures():
    header = open(os.path.join(ROOT, "include", "dsocr.h")).read()
    declared = set(re.findall(r"\b(dsocr_[a-z0-9_]+)\s*\(", header))
    from dsocr._lib import EXPORTS, LIB_PATH, MAX_TOP_LOGPROBS, SESSION_LOGPROBS, SESSION_PER_REQUEST, LogprobsC, SessionDescC
    L = C.CDLL(LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared and s in EXPORTS and hasattr(L, s), s
    flat = " ".join(header.split())
    assert "#define DSOCR_MAX_TOP_LOGPROBS 20" in flat and MAX_TOP_LOGPROBS == 20
    assert "#define DSOCR_SESSION_LOGPROBS 2u" in flat and SESSION_LOGPROBS == 2 and SESSION_PER_REQUEST == 1
    assert ("dsocr_status dsocr_generate_logprobs(dsocr_engine* e, size_t n, const dsocr_request* reqs, "
            "const dsocr_decode_params* params, dsocr_result* results, size_t top_k, dsocr_logprobs* lp);") in flat
    assert ("dsocr_status dsocr_session_logprobs(dsocr_engine* e, int slot, size_t first, size_t count, size_t top_k, "
            "float* token_lp, int64_t* top_id, float* top_lp);") in flat
    assert ("dsocr_status dsocr_k_logprobs(int B, int V, int K, const float* logits, int ld, const int* tok, "
            "const uint8_t* emit, float* lp, int64_t* top_id, float* top_lp);") in flat
    assert [f for f, _ in LogprobsC._fields_] == ["token_lp", "top_id", "top_lp", "cap", "n"]
    assert SessionDescC._fields_[-1][0] == "flags"
    # host-side argument checks run before any device call
    assert L.dsocr_generate_logprobs(None, 0, None, None, None, 0, None) == 1
    assert L.dsocr_session_logprobs(None, 0, 0, 0, 0, None, None, None) == 1
    assert L.dsocr_k_logprobs(1, 8, 21, None, 8, None, None, None, None, None) == 1


def test_decode_outcome_keeps_its_positional_form():
    o = DecodeOutcome("t", 1, 2, [3, 4])
    assert o.token_logprobs is None and o.top_logprobs is None
    assert [f.name for f in DecodeParameters.__dataclass_fields__.values()][:2] == ["max_new_tokens", "do_sample"]
    assert "logprobs" not in DecodeParameters.__dataclass_fields__


# ------------------------------------------------------------------ a scripted engine
def _lp(tok):
    return -(tok % 7) / 4.0


def _top(tok, k):
    return [(tok + j, _lp(tok) - j) for j in range(k)]


class Status:
    def __init__(self, slot, done, out_len, new_tokens):
        self.slot, self.done, self.out_len, self.new_tokens = slot, done, out_len, new_tokens


class FakeSession:
    """Scripted streams: an admission yields the first token, every step k more.  Entry t of a slot is a function of
    its token, so a consumer can tell whether it got the entry of the token it was handed."""
    burst_cap = 8

    def __init__(self, eng, slots, max_context, params, logprobs):
        self.eng, self.slots, self.out_cap, self.has_logprobs = eng, slots, params.max_new_tokens, logprobs
        self.kv_cap = max_context + self.burst_cap
        self.active, self.closed = [], False
        eng.log.append(("open", slots, bool(logprobs)))

    def admit(self, ids, mask=None, page=None, image_rows=None, max_new_tokens=None, seed=None, logprobs=None):
        assert logprobs is None or self.has_logprobs
        key = ids[1]
        self.active.append(dict(key=key, stream=self.eng.scripts[key][:max_new_tokens], pos=1, reported=0))
        self.eng.log.append(("admit", key, logprobs))
        return len(self.active) - 1

    def poll(self):
        out = []
        for i, s in enumerate(self.active):
            pos = min(s["pos"], len(s["stream"]))
            fresh, s["reported"] = s["stream"][s["reported"]:pos], pos
            out.append(Status(i, s["pos"] >= len(s["stream"]), pos, list(fresh)))
        return out

    def step(self, k):
        self.eng.log.append(("step", len(self.active), k))
        for s in self.active:
            s["pos"] += k
        return self.poll()

    def logprobs(self, slot, first, count, top_k):
        s = self.active[slot]
        assert self.has_logprobs and first + count <= min(s["pos"], len(s["stream"]))
        toks = s["stream"][first:first + count]
        self.eng.log.append(("logprobs", s["key"], first, count, top_k))
        return ([_lp(t) for t in toks], [[a for a, _ in _top(t, top_k)] for t in toks],
                [[b for _, b in _top(t, top_k)] for t in toks])

    def retire(self, slot):
        s, last, moved = self.active[slot], len(self.active) - 1, -1
        if slot != last:
            self.active[slot], moved = self.active[last], last
        self.active.pop()
        self.eng.log.append(("retire", s["key"]))
        return list(s["stream"][:s["pos"]]), moved

    def close(self):
        self.closed = True
        self.eng.log.append(("close",))


class FakeEngine:
    variant = 0

    def __init__(self, scripts):
        self.scripts, self.log, self.session = scripts, [], None

    def open_session(self, slots, max_context, params, per_request=False, logprobs=False):
        assert self.session is None or self.session.closed
        self.session = FakeSession(self, slots, max_context, params, logprobs)
        return self.session

    def decode(self, tokenizer, prompt, images, vision, params, stream=None, logprobs=None):
        assert self.session is None or self.session.closed, "generate while a session is open"
        key = int(prompt.split(":")[1])
        self.log.append(("decode", key, logprobs))
        toks = self.scripts[key][:params.max_new_tokens]
        if stream:
            for k in range(1, len(toks) + 1):
                stream(k, toks[:k])
        out = DecodeOutcome(tokenizer.decode(toks, skip_special_tokens=True), 2, len(toks), list(toks))
        if logprobs is not None:
            out.token_logprobs, out.top_logprobs = [_lp(t) for t in toks], [_top(t, logprobs) for t in toks]
        return out


def _prepare(engine, tokenizer, prompt, images, vision):
    key = int(prompt.split(":")[1])
    return [0, key] + [5] * 10, [0] * 12, []


def _sched(eng, logprobs, slots=2):
    from dsocr.scheduler import BatchScheduler
    return BatchScheduler(eng, SyntheticTokenizer(512), slots, 128, DecodeParameters(max_new_tokens=64),
                          VisionSettings(256, 128, True), prepare=_prepare, logprobs=logprobs)


def test_scheduler_with_the_flag_streams_entries():
    eng = FakeEngine({1: [10 + i for i in range(6)], 2: [40 + i for i in range(11)]})
    seen = {1: [], 2: []}
    with _sched(eng, True) as s:
        f1 = s.submit("<image>doc:1", on_token=lambda n, t, e: seen[1].append((n, t[-1], e)), logprobs=3)
        f2 = s.submit("<image>doc:2", logprobs=0)
        f3 = s.submit("<image>doc:1")  # no log-probabilities asked: none fetched, the two-argument callback form
        o1, o2, o3 = f1.result(10), f2.result(10), f3.result(10)
    assert ("open", 2, True) in eng.log and not any(e[0] == "decode" for e in eng.log)
    assert ("admit", 1, 3) in eng.log and ("admit", 2, 0) in eng.log and ("admit", 1, None) in eng.log
    assert o1.generated_tokens == eng.scripts[1] and o2.generated_tokens == eng.scripts[2]
    assert o1.token_logprobs == [_lp(t) for t in o1.generated_tokens]
    assert o1.top_logprobs == [_top(t, 3) for t in o1.generated_tokens]
    assert o2.token_logprobs == [_lp(t) for t in o2.generated_tokens] and o2.top_logprobs == [[] for _ in o2.generated_tokens]
    assert o3.token_logprobs is None and o3.top_logprobs is None
    # every streamed token came with its own entry, one callback per token
    assert [(n, t) for n, t, _ in seen[1]] == list(enumerate(eng.scripts[1], 1))[:len(seen[1])] and len(seen[1]) == 6
    assert all(e == (_lp(t), _top(t, 3)) for _, t, e in seen[1])
    # the entries were read before the slot was retired
    lp1 = [i for i, e in enumerate(eng.log) if e[0] == "logprobs" and e[1] == 1]
    assert max(lp1) < eng.log.index(("retire", 1))
    assert sum(e[3] for e in eng.log if e[0] == "logprobs" and e[1] == 1) == 6


def test_scheduler_without_the_flag_runs_the_request_alone():
    eng = FakeEngine({1: [10 + i for i in range(20)], 2: [40 + i for i in range(5)], 3: [70 + i for i in range(4)]})
    got = []
    with _sched(eng, False) as s:
        f1 = s.submit("<image>doc:1")
        f2 = s.submit("<image>doc:2", logprobs=2, on_token=lambda n, t, e: got.append((t[-1], e)))
        f3 = s.submit("<image>doc:3")
        o1, o2, o3 = f1.result(10), f2.result(10), f3.result(10)
        assert s.exclusive_runs == 1
    assert ("open", 2, False) in eng.log
    kinds = [e for e in eng.log if e[0] in ("admit", "decode", "retire")]
    # arrival order: request 1 drains, request 2 runs alone, only then request 3 is admitted
    assert kinds.index(("retire", 1)) < kinds.index(("decode", 2, 2)) < kinds.index(("admit", 3, None))
    assert not any(e[0] == "logprobs" for e in eng.log)
    assert o2.token_logprobs == [_lp(t) for t in eng.scripts[2]] and o2.top_logprobs == [_top(t, 2) for t in eng.scripts[2]]
    assert got == [(t, (_lp(t), _top(t, 2))) for t in eng.scripts[2]]
    assert o1.token_logprobs is None and o3.generated_tokens == eng.scripts[3]


def test_scheduler_refuses_a_two_argument_callback_with_logprobs():
    eng = FakeEngine({1: [10, 11, 12]})
    with _sched(eng, True) as s:
        with pytest.raises(ValueError):
            s.submit("<image>doc:1", on_token=lambda n, t: None, logprobs=1).result(10)
        with pytest.raises(ValueError):
            s.submit("<image>doc:1", logprobs=21).result(10)
        assert s.submit("<image>doc:1", on_token=lambda n, t: None).result(10).generated_tokens == [10, 11, 12]
    assert not any(e[0] == "logprobs" for e in eng.log)


# ------------------------------------------------------------------ server
class LpEngine:
    """engine.decode with scripted entries: token 3 has a -inf log-probability and a padded (-1) alternative."""
    variant = 0

    def __init__(self):
        self.calls = []

    def decode(self, tokenizer, prompt, images, vision, params, stream=None, logprobs=None):
        self.calls.append(logprobs)
        toks = [11, 12, 13]
        if stream:
            for k in range(1, 4):
                stream(k, toks[:k])
        out = DecodeOutcome(tokenizer.decode(toks, skip_special_tokens=True), 4, 3, toks)
        if logprobs is not None:
            out.token_logprobs = [-0.25, -1.5, -math.inf]
            out.top_logprobs = [[(t, -0.25), (t + 1, -math.inf), (-1, -math.inf)][:logprobs] for t in toks]
        return out


PNG = ("data:image/png;base64,iVBORw0KGgoAAAANSUhEUgAAAAEAAAABCAYAAAAfFcSJAAAADUlEQVR42mP8z8BQDwAEhQGAhKmMIQAAAABJRU5E"
       "rkJggg==")


def _body(**kw):
    b = {"model": "deepseek-ocr", "messages": [{"role": "user", "content": [
        {"type": "text", "text": "<image>\nread"}, {"type": "image_url", "image_url": {"url": PNG}}]}]}
    b.update(kw)
    return b


def _state():
    tok = SyntheticTokenizer(512)
    return server.ServerState(LpEngine(), tok, "deepseek-ocr", VisionSettings(256, 128, True), DecodeParameters(max_new_tokens=8)), tok


def test_server_arguments_and_errors():
    assert server.parse_logprobs({}) is None and server.parse_logprobs({"logprobs": False}) is None
    assert server.parse_logprobs({"logprobs": True}) == 0
    assert server.parse_logprobs({"logprobs": True, "top_logprobs": 20}) == 20
    for bad in ({"top_logprobs": 2}, {"logprobs": False, "top_logprobs": 2}, {"logprobs": True, "top_logprobs": 21},
                {"logprobs": True, "top_logprobs": -1}, {"logprobs": True, "top_logprobs": 1.5}):
        with pytest.raises(server.ApiError) as ei:
            server.parse_logprobs(bad)
        assert ei.value.status == 400
    state, _ = _state()
    for bad in ({"top_logprobs": 3}, {"logprobs": True, "top_logprobs": 21}, {"logprobs": True, "top_logprobs": -1}):
        with pytest.raises(server.ApiError) as ei:
            server.handle_generation(state, _body(**bad), "chat")
        assert ei.value.status == 400
    assert state.engine.calls == []
    # /v1/responses is left alone: the fields are not read there
    how, _ = server.handle_generation(state, dict(_body(top_logprobs=99), input=_body()["messages"]), "responses")
    assert how == "json" and state.engine.calls == [None]


def test_server_response_shape():
    state, tok = _state()
    how, plain = server.handle_generation(state, _body(), "chat")
    assert "logprobs" not in plain["choices"][0] and state.engine.calls == [None]
    how, body = server.handle_generation(state, _body(logprobs=True, top_logprobs=3), "chat")
    assert how == "json" and state.engine.calls == [None, 3]
    text = json.dumps(body)  # valid JSON: no Infinity
    assert "Infinity" not in text and json.loads(text) == body
    content = body["choices"][0]["logprobs"]["content"]
    assert len(content) == 3
    for e, t, lp in zip(content, [11, 12, 13], [-0.25, -1.5, -9999.0]):
        word = tok.decode([t])  # each token decoded on its own
        assert e["token"] == word and e["bytes"] == list(word.encode("utf-8")) and e["logprob"] == lp
        assert [a["token"] for a in e["top_logprobs"]] == [tok.decode([t]), tok.decode([t + 1])]  # the -1 pad is dropped
        assert [a["logprob"] for a in e["top_logprobs"]] == [-0.25, -9999.0]
        assert all(a["bytes"] == list(a["token"].encode("utf-8")) for a in e["top_logprobs"])
    how, body = server.handle_generation(state, _body(logprobs=True), "chat")
    assert all(e["top_logprobs"] == [] for e in body["choices"][0]["logprobs"]["content"])


def test_server_sse_chunks_carry_their_tokens_entries():
    state, tok = _state()
    how, ctl = server.handle_generation(state, _body(logprobs=True, top_logprobs=1, stream=True), "chat")
    assert how == "stream"
    events = [json.loads(e[len("data: "):]) for e in ctl.events() if not e.startswith("data: [DONE]")]
    entries, texts = [], ""
    for ev in events:
        ch = ev["choices"][0]
        texts += ch["delta"].get("content", "")
        if "logprobs" in ch:
            entries += ch["logprobs"]["content"]
    assert [e["token"] for e in entries] == [tok.decode([t]) for t in (11, 12, 13)]
    assert [e["logprob"] for e in entries] == [-0.25, -1.5, -9999.0] and all(len(e["top_logprobs"]) == 1 for e in entries)
    assert texts.strip() == tok.decode([11, 12, 13]).strip()
    # without the fields the chunks are what they were
    how, ctl = server.handle_generation(state, _body(stream=True), "chat")
    assert all("logprobs" not in json.loads(e[6:])["choices"][0] for e in ctl.events() if "[DONE]" not in e)


def test_server_flag_opens_the_session_with_logprobs():
    import argparse
    p = argparse.ArgumentParser()
    server.add_scheduler_args(p)
    assert p.parse_args([]).logprobs is False and p.parse_args(["--slots", "2", "--logprobs"]).logprobs is True
    eng = FakeEngine({})
    state = server.ServerState(eng, SyntheticTokenizer(512), "deepseek-ocr")
    sch = server.make_scheduler(state, 2, 64, logprobs=True)
    try:
        assert sch.logprobs is True
    finally:
        sch.close()
    assert server.make_scheduler(state, 0, 64, logprobs=True) is None


# ------------------------------------------------------------------ CLI
def test_cli_prints_one_json_line_per_token(monkeypatch, tmp_path):
    args = cli.build_parser().parse_args(["--prompt", "<image>\nread", "--image", "x.png", "--logprobs", "3", "-q"])
    assert args.logprobs == 3 and cli.build_parser().parse_args(["--prompt", "x"]).logprobs is None
    eng = LpEngine()
    eng.close = lambda: None
    eng.last_timings = lambda: {}
    monkeypatch.setattr(cli, "load_model", lambda a: eng)
    monkeypatch.setattr(cli, "open_image", lambda p: object())
    out = io.StringIO()
    assert cli.run_inference(args, out, io.StringIO()) == 0
    lines = out.getvalue().strip().split("\n")
    recs = [json.loads(x) for x in lines[-3:]]
    assert eng.calls == [3] and [r["id"] for r in recs] == [11, 12, 13]
    assert [r["logprob"] for r in recs] == [-0.25, -1.5, -9999.0]
    assert recs[0]["top_logprobs"] == [{"id": 11, "logprob": -0.25}, {"id": 12, "logprob": -9999.0}]
    assert lines[0] == SyntheticTokenizer(512).decode([11, 12, 13], skip_special_tokens=True).strip()
