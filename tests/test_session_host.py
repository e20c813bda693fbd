"""Decode sessions, host side (no GPU): the C ABI exports, the scheduler's bookkeeping against a scripted engine,
and the server's two paths (scheduler / lock)."""
import base64
import ctypes as C
import io
import os
import re
import threading

import numpy as np
import pytest

from dsocr import DecodeOutcome, DecodeParameters, DsocrError, VisionSettings
from dsocr import cli, server
from dsocr.synth import SyntheticTokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dsocr_session_open", "dsocr_session_admit", "dsocr_session_step", "dsocr_session_poll",
               "dsocr_session_retire", "dsocr_session_close", "dsocr_session_info", "dsocr_k_session_slot_move"]


def test_c_abi_exports_the_session_symbols():
    header = open(os.path.join(ROOT, "include", "dsocr.h")).read()
    declared = set(re.findall(r"\b(dsocr_[a-z0-9_]+)\s*\(", header))
    from dsocr._lib import EXPORTS, LIB_PATH
    L = C.CDLL(LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared and s in EXPORTS, s
        assert hasattr(L, s), s


# ------------------------------------------------------------------ a scripted engine
class Status:
    def __init__(self, slot, done, out_len, new_tokens):
        self.slot, self.done, self.out_len, self.new_tokens = slot, done, out_len, new_tokens


class FakeSession:
    """Slots hold scripted token streams: an admission yields the first token, every step one more per slot.  A
    stream that ends before max_new ends like eos; `stuck` streams never yield again and never finish."""
    burst_cap = 8

    def __init__(self, eng, slots, max_context, params):
        self.eng, self.slots, self.max_context, self.out_cap = eng, slots, max_context, params.max_new_tokens
        self.kv_cap = max_context + self.burst_cap
        self.active = []
        self.closed = False
        eng.log.append(("open", slots, max_context))

    def admit(self, ids, mask=None, page=None, image_rows=None, max_new_tokens=None, seed=None):
        key = ids[1]
        if key in self.eng.admit_errors:
            raise self.eng.admit_errors[key]
        assert len(self.active) < self.slots
        self.active.append(dict(key=key, stream=self.eng.scripts[key], pos=1, reported=0, max_new=max_new_tokens,
                                seed=seed))
        self.eng.log.append(("admit", key, len(self.active) - 1))
        self.eng.peak = max(self.eng.peak, len(self.active))
        return len(self.active) - 1

    def _cap(self, s):
        return len(s["stream"]) if self.eng.overshoot else min(len(s["stream"]), s["max_new"])

    def poll(self):
        out = []
        for i, s in enumerate(self.active):
            stuck = s["key"] in self.eng.stuck
            pos = min(s["pos"], 1 if stuck else self._cap(s))
            fresh = s["stream"][s["reported"]:pos]
            s["reported"] = pos
            out.append(Status(i, (not stuck) and s["pos"] >= self._cap(s), pos, list(fresh)))
        return out

    def step(self, k):
        assert self.eng.gate.wait(10)
        self.eng.log.append(("step", len(self.active), k))
        for s in self.active:
            s["pos"] += k
        return self.poll()

    def retire(self, slot):
        s = self.active[slot]
        last = len(self.active) - 1
        moved = -1
        if slot != last:
            self.active[slot] = self.active[last]
            moved = last
        self.active.pop()
        self.eng.log.append(("retire", s["key"], slot))
        return list(s["stream"][:min(s["pos"], self._cap(s))]), moved

    def close(self):
        self.closed = True
        self.eng.log.append(("close",))


class FakeEngine:
    variant = 0

    def __init__(self, scripts):
        self.scripts = scripts
        self.log, self.peak = [], 0
        self.admit_errors, self.stuck = {}, set()
        self.overshoot = False  # True: the session hands out tokens past a request's max_new_tokens
        self.gate = threading.Event()
        self.session = None

    def open_session(self, slots, max_context, params):
        assert self.session is None or self.session.closed
        self.session = FakeSession(self, slots, max_context, params)
        return self.session

    def decode(self, tokenizer, prompt, images, vision, params, stream=None):
        assert self.session is None or self.session.closed, "generate while a session is open"
        key = int(prompt.split(":")[1])
        self.log.append(("decode", key))
        toks = self.scripts[key][:params.max_new_tokens]
        for k in range(1, len(toks) + 1):
            if stream:
                stream(k, toks[:k])
        return DecodeOutcome(tokenizer.decode(toks, skip_special_tokens=True), 2, len(toks), list(toks))


def _prepare(engine, tokenizer, prompt, images, vision):
    """prompt "<image>doc:KEY": ids [0, KEY] + padding to the scripted prompt length"""
    key = int(prompt.split(":")[1])
    return [0, key] + [5] * 10, [0] * 12, []


def _stream(key, n):
    return [100 * key + i for i in range(n)]


def _sched(eng, slots=2, max_context=128, defaults=DecodeParameters(max_new_tokens=64)):
    from dsocr.scheduler import BatchScheduler
    return BatchScheduler(eng, SyntheticTokenizer(512), slots, max_context, defaults, VisionSettings(256, 128, True),
                          prepare=_prepare)


def test_admission_order_slot_reuse_and_results():
    lens = {1: 5, 2: 20, 3: 9, 4: 7}
    eng = FakeEngine({k: _stream(k, n) for k, n in lens.items()})
    with _sched(eng) as s:
        futs = {k: s.submit(f"<image>doc:{k}") for k in lens}
        eng.gate.set()
        outs = {k: f.result(timeout=20) for k, f in futs.items()}
        assert s.max_active == 2
    for k, n in lens.items():
        assert outs[k].generated_tokens == _stream(k, n) and outs[k].response_tokens == n
        assert outs[k].prompt_tokens == 12
    admits = [e for e in eng.log if e[0] == "admit"]
    assert [e[1] for e in admits] == [1, 2, 3, 4]
    assert [e[2] for e in admits[:2]] == [0, 1] and eng.peak == 2
    # every admission after the first two took a slot that a retirement freed
    for i, e in enumerate(eng.log):
        if e[0] == "admit" and e[1] in (3, 4):
            assert any(p[0] == "retire" for p in eng.log[:i])
    assert all(b == 8 for _, b in s.bursts)  # nobody streams


def test_max_new_tokens_truncates_per_request():
    eng = FakeEngine({1: _stream(1, 40), 2: _stream(2, 40)})
    eng.overshoot = True
    eng.gate.set()
    with _sched(eng) as s:
        a = s.submit("<image>doc:1", params=DecodeParameters(max_new_tokens=6))
        b = s.submit("<image>doc:2", params=DecodeParameters(max_new_tokens=17, seed=3))
        assert a.result(timeout=20).generated_tokens == _stream(1, 6)
        assert b.result(timeout=20).generated_tokens == _stream(2, 17)


def test_on_token_counts_are_monotone_and_burst_is_one_while_streaming():
    eng = FakeEngine({1: _stream(1, 11), 2: _stream(2, 30)})
    seen = []
    with _sched(eng) as s:
        a = s.submit("<image>doc:1", on_token=lambda n, ids: seen.append((n, list(ids))))
        b = s.submit("<image>doc:2")
        eng.gate.set()
        ra, rb = a.result(timeout=20), b.result(timeout=20)
        bursts = list(s.bursts)
    assert [n for n, _ in seen] == list(range(1, 12))
    assert all(ids == _stream(1, n) for n, ids in seen) and seen[-1][1] == ra.generated_tokens
    assert rb.generated_tokens == _stream(2, 30)
    steps = [e for e in eng.log if e[0] == "step"]
    retired = eng.log.index(("retire", 1, 0))
    assert all(e[2] == 1 for e in eng.log[:retired] if e[0] == "step")      # a streaming request is active
    assert any(e[2] == 8 for e in eng.log[retired:] if e[0] == "step")      # it left: full bursts again
    assert len(steps) == len(bursts)


def test_foreign_parameters_run_alone_when_the_session_is_empty():
    eng = FakeEngine({1: _stream(1, 30), 2: _stream(2, 9), 3: _stream(3, 12), 4: _stream(4, 200)})
    with _sched(eng) as s:
        a = s.submit("<image>doc:1")
        x = s.submit("<image>doc:2", params=DecodeParameters(max_new_tokens=64, repetition_penalty=1.3))
        b = s.submit("<image>doc:3")
        big = s.submit("<image>doc:4", params=DecodeParameters(max_new_tokens=200))  # more than the session holds
        eng.gate.set()
        assert a.result(timeout=20).generated_tokens == _stream(1, 30)
        assert x.result(timeout=20).generated_tokens == _stream(2, 9)
        assert b.result(timeout=20).generated_tokens == _stream(3, 12)
        assert big.result(timeout=20).generated_tokens == _stream(4, 200)
    log = eng.log
    dx = log.index(("decode", 2))
    assert log.index(("retire", 1, 0)) < dx and log[dx - 1] == ("close",)   # the session drained and closed first
    assert log.index(("admit", 3, 0)) > dx                                   # nothing overtook it
    assert log.index(("decode", 4)) > log.index(("retire", 3, 0))


def test_admit_error_reaches_only_its_own_future():
    eng = FakeEngine({1: _stream(1, 20), 2: _stream(2, 5), 3: _stream(3, 8)})
    eng.admit_errors[2] = DsocrError(1, "prompt/image embedding mismatch: scripted")
    with _sched(eng) as s:
        a, bad, c = (s.submit(f"<image>doc:{k}") for k in (1, 2, 3))
        eng.gate.set()
        with pytest.raises(DsocrError, match="mismatch"):
            bad.result(timeout=20)
        assert a.result(timeout=20).generated_tokens == _stream(1, 20)
        assert c.result(timeout=20).generated_tokens == _stream(3, 8)


def test_capacity_assertion_fires_before_the_burst():
    from dsocr.scheduler import CapacityError
    eng = FakeEngine({1: _stream(1, 60), 2: _stream(2, 4)})
    eng.stuck.add(1)  # never finishes, never retires: its KV position runs towards the session's rows
    eng.gate.set()
    with _sched(eng, max_context=80) as s:
        a = s.submit("<image>doc:1")
        with pytest.raises(CapacityError):
            a.result(timeout=20)
        steps = [e[2] for e in eng.log if e[0] == "step"]
        # prompt 12 rows, 88 cache rows: nine full bursts fit (12 + 72 = 84), the tenth would reach 92
        assert sum(steps) == 72 and ("close",) in eng.log
        # the scheduler goes on serving
        assert s.submit("<image>doc:2").result(timeout=20).generated_tokens == _stream(2, 4)


# ------------------------------------------------------------------ the real Session over a scripted library
class FakeLib:
    """The library's session entry points as ``dsocr.engine.Session`` calls them: every staging and admission call is
    logged, and an admission raises while ``fail`` is set (after it has consumed what was staged, as the library
    does)."""

    def __init__(self):
        self.calls, self.fail, self.active = [], False, 0

    def dsocr_session_open_ex(self, h, slots, max_context, pc, flags):
        return 0

    def dsocr_session_info(self, h, desc):
        desc._obj.slots, desc._obj.max_context, desc._obj.out_cap = 4, 128, 16
        return 0

    def dsocr_session_stage_logit_bias(self, h, rec):
        self.calls.append("constraint")
        return 0

    def dsocr_session_stage_stop(self, h, rec):
        self.calls.append("stop")
        return 0

    def _admission(self, out):
        self.calls.append("admission")
        if self.fail:
            raise DsocrError(1, "scripted admission failure")
        out._obj.value = self.active
        self.active += 1
        return 0

    def dsocr_session_admit(self, h, req, max_new, has_seed, seed, slot):
        return self._admission(slot)

    def dsocr_session_admit_prefix(self, h, handle, req, pc, slot):
        return self._admission(slot)

    def dsocr_session_admit_begin(self, h, req, pc, chunk_rows, ticket):
        return self._admission(ticket)


@pytest.mark.parametrize("form", ["admit", "admit_begin", "admit_prefix"])
def test_a_failed_admission_leaves_nothing_staged(monkeypatch, form):
    """Every admission form stages the constraint, then the stop set, then makes its C call; when that call fails
    no stop record is left staged or pending, and the records of the pages admitted before are untouched."""
    from dsocr import engine as E
    from dsocr.stops import merge_stops
    fake = FakeLib()
    monkeypatch.setattr(E, "lib", lambda: fake)
    eng = E.DeepseekOcrEngine.__new__(E.DeepseekOcrEngine)
    eng._h, eng.eos_token_id, eng.vocab = None, 1, 512
    sess = E.Session(eng, 4, 128, DecodeParameters(max_new_tokens=16), logit_bias=True, stops=True)
    assert (sess._staged_stops, sess._pending_stops, sess._pending_page, sess._slot_stops) == (None, None, None, {})
    first = [merge_stops(None, [7], None, 512), merge_stops(None, [8, 9], None, 512)]
    assert [sess.admit([0, 5, 6], stops=ss, include_stop_in_output=bool(k)) for k, ss in enumerate(first)] == [0, 1]
    before = {k: sess.slot_stops(k) for k in range(4)}
    assert before == {0: (first[0], False), 1: (first[1], True), 2: None, 3: None}

    fake.fail, fake.calls = True, []
    args = ((3, [0, 5, 6]) if form == "admit_prefix" else ([0, 5, 6],))
    with pytest.raises(DsocrError, match="scripted"):
        getattr(sess, form)(*args, logit_bias={5: 1.0}, stop_token_ids=[11])
    assert fake.calls == ["constraint", "stop", "admission"]
    assert sess._staged_stops is None and sess._pending_stops is None
    assert {k: sess.slot_stops(k) for k in range(4)} == before

    fake.fail = False   # the next page carries no stops: none of the failed admission's reach its slot
    assert sess.admit([0, 5, 6]) == 2 and sess.slot_stops(2) is None
    assert {k: sess.slot_stops(k) for k in range(4)} == before


# ------------------------------------------------------------------ server and CLI
def _data_url(seed):
    from PIL import Image
    arr = np.random.default_rng(seed).integers(0, 256, (40, 60, 3), dtype=np.uint8)
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format="PNG")
    return "data:image/png;base64," + base64.b64encode(b.getvalue()).decode()


def _chat(c, key, **extra):
    return c.post("/v1/chat/completions", json=dict({"model": "deepseek-ocr", "messages": [
        {"role": "user", "content": [{"type": "text", "text": f"doc:{key}"},
                                     {"type": "image_url", "image_url": {"url": _data_url(key)}}]}]}, **extra))


def test_server_two_concurrent_requests_share_the_session():
    from starlette.testclient import TestClient
    eng = FakeEngine({1: _stream(1, 30), 2: _stream(2, 40), 3: _stream(3, 5)})
    eng.admit_errors[3] = DsocrError(1, "prompt/image embedding mismatch: scripted")
    st = server.ServerState(eng, SyntheticTokenizer(512), "deepseek-ocr", VisionSettings(256, 128, True),
                            DecodeParameters(max_new_tokens=64))
    st.scheduler = _sched(eng)
    submitted, submit = [], st.scheduler.submit
    st.scheduler.submit = lambda *a, **k: (submitted.append(1), submit(*a, **k))[1]
    try:
        c = TestClient(server.create_app(st))
        res = {}
        ts = [threading.Thread(target=lambda k=k: res.__setitem__(k, _chat(c, k))) for k in (1, 2, 3)]
        for t in ts:
            t.start()
        while len(submitted) < 3 and any(t.is_alive() for t in ts):  # the steps wait until every request is in
            threading.Event().wait(0.01)
        eng.gate.set()
        for t in ts:
            t.join(20)
        tok = SyntheticTokenizer(512)
        for k, n in ((1, 30), (2, 40)):
            assert res[k].status_code == 200, res[k].text
            assert res[k].json()["choices"][0]["message"]["content"] == tok.decode(_stream(k, n), skip_special_tokens=True)
            assert res[k].json()["usage"]["completion_tokens"] == n
        assert res[3].status_code == 400 and "mismatch" in res[3].json()["error"]["message"]
        assert eng.peak == 2 and not any(e[0] == "decode" for e in eng.log)
    finally:
        st.scheduler.close()


def test_server_slots_zero_takes_the_lock_path():
    from starlette.testclient import TestClient
    eng = FakeEngine({1: _stream(1, 6)})
    st = server.ServerState(eng, SyntheticTokenizer(512), "deepseek-ocr", VisionSettings(256, 128, True),
                            DecodeParameters(max_new_tokens=64))
    assert st.scheduler is None
    st.scheduler = server.make_scheduler(st, 0, 4096)
    assert st.scheduler is None
    r = _chat(TestClient(server.create_app(st)), 1)
    assert r.status_code == 200 and r.json()["usage"]["completion_tokens"] == 6
    assert eng.log == [("decode", 1)]
    import argparse
    p = argparse.ArgumentParser()
    server.add_scheduler_args(p)
    assert p.parse_args([]).slots == 0 and p.parse_args(["--slots", "4", "--max-context", "2048"]).max_context == 2048
    on = server.make_scheduler(st, 2, 128)
    try:
        assert on is not None and on.slots == 2 and on.max_context == 128
    finally:
        on.close()


def test_cli_has_the_session_flags():
    a = cli.build_parser().parse_args(["--prompt", "<image>", "--image", "a.png"])
    assert a.slots == 0
    a = cli.build_parser().parse_args(["--prompt", "<image>", "--image", "a.png", "--image", "b.png", "--slots", "2",
                                       "--max-context", "1024"])
    assert (a.slots, a.max_context, a.images) == (2, 1024, ["a.png", "b.png"])
