"""Logit bias and token allow / deny sets, host side (no GPU): the merge rules of the three Python arguments, every
EINVAL case through the C ABI's device-free check, the server's request parsing, the command line, and the scheduler's
choice between the shared and the exclusive path (and that a constrained retry on a cached page is a prefix hit)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from dsocr import DecodeParameters, DsocrError, VisionSettings
from dsocr import server
from dsocr.constraint import ConstraintError, LogitConstraint, merge_constraint
from dsocr.synth import SyntheticTokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dsocr_logit_bias_check", "dsocr_generate_logit_bias", "dsocr_session_stage_logit_bias",
               "dsocr_k_logit_bias"]
INF = math.inf


def test_c_abi_exports_the_logit_bias_symbols():
    header = open(os.path.join(ROOT, "include", "dsocr.h")).read()
    declared = set(re.findall(r"\b(dsocr_[a-z0-9_]+)\s*\(", header))
    from dsocr._lib import EXPORTS, LIB_PATH, SESSION_LOGIT_BIAS, LogitBiasC
    L = C.CDLL(LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared and s in EXPORTS and hasattr(L, s), s
    flat = " ".join(header.split())
    assert "#define DSOCR_SESSION_LOGIT_BIAS 4u" in flat and SESSION_LOGIT_BIAS == 4
    assert "typedef struct { const int64_t* ids; const float* values; size_t n; int allow_only; } dsocr_logit_bias;" in flat
    assert [f[0] for f in LogitBiasC._fields_] == ["ids", "values", "n", "allow_only"]
    from dsocr.engine import DeepseekOcrEngine, Session
    import inspect
    for fn in (DeepseekOcrEngine.decode, Session.admit, Session.admit_prefix, Session.admit_begin):
        assert {"logit_bias", "allowed_token_ids", "banned_token_ids"} <= set(inspect.signature(fn).parameters)


# ------------------------------------------------------------------ merge rules
def test_merge_rules():
    assert merge_constraint() is None and merge_constraint({}, None, []) is None
    assert merge_constraint({4: 0.0}) is None                      # a zero bias says nothing
    assert merge_constraint({5: 1.5, 2: -3}) == LogitConstraint((2, 5), (-3.0, 1.5), False)
    assert merge_constraint(banned_token_ids=[9, 3, 9]) == LogitConstraint((3, 9), (-INF, -INF), False)
    assert merge_constraint(allowed_token_ids=[7, 1, 7]) == LogitConstraint((1, 7), (0.0, 0.0), True)
    # a ban overrides a bias on the same id; an id both allowed and banned is banned
    assert merge_constraint({5: 9.0}, None, [5]) == LogitConstraint((5,), (-INF,), False)
    assert merge_constraint({1: 2.0, 8: 4.0}, [1, 2, 3], [2, 8]) == LogitConstraint((1, 2, 3), (2.0, -INF, 0.0), True)
    c = merge_constraint({1: 2.0}, [1, 3], [3], vocab=6)
    assert np.array_equal(c.dense(6), np.array([-INF, 2.0, -INF, -INF, -INF, -INF], np.float32))
    assert merge_constraint(**c.kwargs()) == c                     # the keywords round-trip
    assert np.array_equal(merge_constraint({2: -1.0}, banned_token_ids=[0]).dense(4),
                          np.array([-INF, 0, -1.0, 0], np.float32))
    for bad in (dict(logit_bias={-1: 0.0}), dict(logit_bias={6: 1.0}, vocab=6), dict(logit_bias={1: float("nan")}),
                dict(logit_bias={1: INF}), dict(allowed_token_ids=[]), dict(banned_token_ids=[6], vocab=6),
                dict(logit_bias={"x": 1.0}), dict(logit_bias={1.5: 1.0}), dict(logit_bias={1: "a"}),
                dict(allowed_token_ids=[True])):
        with pytest.raises(ConstraintError):
            merge_constraint(**bad)


# ------------------------------------------------------------------ every EINVAL case through the C ABI
def _check(ids, values, allow_only, vocab, n=None):
    from dsocr._lib import LogitBiasC, lib
    i = np.asarray(ids, np.int64)
    v = np.asarray(values, np.float32)
    rec = LogitBiasC(i.ctypes.data_as(C.POINTER(C.c_int64)), v.ctypes.data_as(C.POINTER(C.c_float)),
                     len(i) if n is None else n, allow_only)
    st = lib().dsocr_logit_bias_check(C.byref(rec), vocab)
    return st, (lib().dsocr_last_error() or b"").decode()


def test_c_abi_check():
    from dsocr._lib import lib
    assert _check([0, 9], [1.0, -INF], 0, 10)[0] == 0
    assert _check([3], [0.0], 1, 10)[0] == 0
    assert _check([], [], 0, 10)[0] == 0                            # "no constraint"
    assert lib().dsocr_logit_bias_check(None, 10) == 0
    assert _check(list(range(10)), [0.0] * 10, 1, 10)[0] == 0       # n == vocab
    cases = {"outside": ([10], [0.0], 0), "negative": ([-1], [0.0], 0), "duplicate": ([4, 4], [0.0, 1.0], 0),
             "nan": ([4], [float("nan")], 0), "+inf": ([4], [INF], 0), "allow_only, n == 0": ([], [], 1),
             "n > vocab": (list(range(10)) + [0], [0.0] * 11, 0)}
    for name, (ids, vals, allow) in cases.items():
        st, msg = _check(ids, vals, allow, 10)
        assert st == 1 and msg.startswith("EINVAL: logit bias"), (name, st, msg)
    assert _check([1], [0.0], 0, 0)[0] == 1                         # no vocabulary
    # the Python surface reports the same status without a device
    from dsocr.engine import _constraint
    with pytest.raises(DsocrError) as ei:
        _constraint({600: 1.0}, None, None, 512)
    assert ei.value.status == 1


# ------------------------------------------------------------------ server request parsing
def test_server_parsing():
    P = server.parse_token_constraint
    assert P({}, 512) is None and P({"logit_bias": {}}, 512) is None
    assert P({"logit_bias": {"17": -100, "3": 2.5}}, 512) == {"logit_bias": {3: 2.5, 17: -100.0}}   # string keys
    kw = P({"logit_bias": {"5": 1}, "allowed_token_ids": [5, 6], "banned_token_ids": [6]}, 512)
    assert merge_constraint(**kw) == LogitConstraint((5, 6), (1.0, -INF), True)
    assert P({"banned_token_ids": [4]}, 512) == {"logit_bias": {4: -INF}}
    bad = [{"logit_bias": {"17": 101}}, {"logit_bias": {"17": -100.5}}, {"logit_bias": {"x": 1}},
           {"logit_bias": {"1.5": 1}}, {"logit_bias": {"512": 1}}, {"logit_bias": {"-1": 1}}, {"logit_bias": {"3": "1"}},
           {"logit_bias": {"3": True}}, {"logit_bias": [1]}, {"logit_bias": {"3": None}},
           {"allowed_token_ids": []}, {"allowed_token_ids": [512]}, {"allowed_token_ids": "3"},
           {"banned_token_ids": [1.5]}, {"banned_token_ids": [-2]}, {"logit_bias": {"3": 1, "03": 2}}]
    for body in bad:
        with pytest.raises(server.ApiError) as ei:
            P(body, 512)
        assert ei.value.status == 400, body


# ------------------------------------------------------------------ a scripted engine for the scheduler
class Status:
    def __init__(self, slot, done, out_len, new_tokens):
        self.slot, self.done, self.out_len, self.new_tokens = slot, done, out_len, new_tokens


class FakeSession:
    burst_cap = 8

    def __init__(self, eng, slots, max_context, params, kw):
        self.eng, self.out_cap, self.kv_cap = eng, params.max_new_tokens, max_context + 8
        self.active, self.handles = [], {}
        eng.log.append(("open", dict(kw)))

    def _slot(self, kind, ids, kw):
        self.active.append(dict(key=ids[-1], pos=1, reported=0))
        self.eng.log.append((kind, ids[-1], {k: v for k, v in kw.items() if k not in ("max_new_tokens", "seed")}))
        return len(self.active) - 1

    def admit(self, ids, mask=None, page=None, image_rows=None, **kw):
        return self._slot("admit", ids, kw)

    def admit_prefix(self, handle, ids, mask=None, **kw):
        assert handle in self.handles
        return self._slot("admit_prefix", ids, kw)

    def keep_prefix(self, slot, rows):
        self.handles[len(self.handles) + 1] = rows
        return len(self.handles)

    def drop_prefix(self, handle):
        del self.handles[handle]

    def poll(self):
        out = []
        for i, s in enumerate(self.active):
            pos = min(s["pos"], 3)
            out.append(Status(i, s["pos"] >= 3, pos, [1000 * s["key"] + t for t in range(s["reported"], pos)]))
            s["reported"] = pos
        return out

    def step(self, k):
        for s in self.active:
            s["pos"] += k
        return self.poll()

    def retire(self, slot):
        s = self.active[slot]
        last, moved = len(self.active) - 1, -1
        if slot != last:
            self.active[slot], moved = self.active[last], last
        self.active.pop()
        return [1000 * s["key"] + t for t in range(3)], moved

    def close(self):
        self.eng.log.append(("close",))


class FakeEngine:
    variant, vocab = 0, 512

    def __init__(self):
        self.log = []

    def open_session(self, slots, max_context, params, **kw):
        return FakeSession(self, slots, max_context, params, kw)

    def decode(self, tokenizer, prompt, images, vision, params, stream=None, **kw):
        from dsocr.engine import DecodeOutcome
        self.log.append(("decode", int(prompt), dict(kw)))
        return DecodeOutcome("x", 7, 3, [1, 2, 3])


def _prepare(engine, tokenizer, prompt, images, vision):
    ids, mask = [0] + [9] * 4 * len(images) + [7, int(prompt)], [0] + [1] * 4 * len(images) + [0, 0]
    return ids, mask, [object() for _ in images]


def _sched(eng, **kw):
    from dsocr.scheduler import BatchScheduler
    return BatchScheduler(eng, SyntheticTokenizer(512), 2, 128, DecodeParameters(max_new_tokens=8),
                          VisionSettings(256, 128, True), prepare=_prepare, **kw)


def test_scheduler_shared_and_exclusive_paths():
    img = np.zeros((8, 8, 3), np.uint8)
    want = {"logit_bias": {3: -INF, 5: 2.0}}
    eng = FakeEngine()
    with _sched(eng, logit_bias=True) as s:   # the flag: a constrained request shares the session
        s.submit("11", [img]).result(timeout=20)
        s.submit("12", [img], logit_bias={5: 2.0}, banned_token_ids=[3]).result(timeout=20)
        assert s.exclusive_runs == 0
    assert eng.log[0] == ("open", {"logit_bias": True})
    assert ("admit", 11, {}) in eng.log and ("admit", 12, want) in eng.log
    eng = FakeEngine()
    with _sched(eng) as s:                    # no flag: it drains the session and decodes alone, with the arguments
        s.submit("11", [img]).result(timeout=20)
        out = s.submit("12", [img], allowed_token_ids=[4, 6], logit_bias={4: 1.0}).result(timeout=20)
        assert s.exclusive_runs == 1 and out.generated_tokens == [1, 2, 3]
        bad = s.submit("13", [img], logit_bias={512: 1.0})
        with pytest.raises(ValueError):
            bad.result(timeout=20)
    assert eng.log[0] == ("open", {}) and ("admit", 11, {}) in eng.log
    assert ("decode", 12, {"logit_bias": {4: 1.0, 6: 0.0}, "allowed_token_ids": [4, 6]}) in eng.log
    assert not any(e[0] == "decode" and e[1] == 13 for e in eng.log)


def test_constrained_retry_on_a_cached_page_is_a_prefix_hit():
    img = np.random.default_rng(3).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    eng = FakeEngine()
    with _sched(eng, logit_bias=True, prefix_cache=4) as s:
        s.submit("11", [img]).result(timeout=20)
        s.submit("12", [img.copy()], banned_token_ids=[3]).result(timeout=20)
        assert (s.prefix_hits, s.prefix_misses) == (1, 1)
    assert ("admit", 11, {}) in eng.log and ("admit_prefix", 12, {"logit_bias": {3: -INF}}) in eng.log


# ------------------------------------------------------------------ server option and command line
def test_server_flag_and_cli_options(tmp_path, capsys):
    import argparse
    p = argparse.ArgumentParser()
    server.add_scheduler_args(p)
    assert p.parse_args([]).logit_bias is False and p.parse_args(["--slots", "2", "--logit-bias"]).logit_bias is True
    st = server.ServerState(FakeEngine(), SyntheticTokenizer(512), "deepseek-ocr", VisionSettings(256, 128, True),
                            DecodeParameters(max_new_tokens=8))
    with pytest.raises(ValueError, match="--slots"):
        server.make_scheduler(st, 0, 128, logit_bias=True)
    on = server.make_scheduler(st, 2, 128, logit_bias=True)
    try:
        assert on.logit_bias is True
    finally:
        on.close()
    with pytest.raises(SystemExit):
        server.main(["--logit-bias"])
    assert "--logit-bias needs --slots" in capsys.readouterr().err
    from dsocr import cli
    f = tmp_path / "allow.txt"
    f.write_text("48\n49  # nine\n\n57\n")
    a = cli.build_parser().parse_args(["--prompt", "<image>", "--ban-token", "3", "--ban-token", "4", "--logit-bias",
                                       "7=-2.5", "--logit-bias", "9=30", "--allow-tokens-file", str(f)])
    assert cli.token_constraint(a) == {"logit_bias": {7: -2.5, 9: 30.0}, "banned_token_ids": [3, 4],
                                       "allowed_token_ids": [48, 49, 57]}
    assert cli.token_constraint(cli.build_parser().parse_args(["--prompt", "x"])) == {}
    for argv in (["--logit-bias", "7"], ["--logit-bias", "a=1"], ["--logit-bias", "7=x"],
                 ["--logit-bias", "7=1", "--logit-bias", "7=2"], ["--ban-token", "3", "--slots", "2"]):
        with pytest.raises(DsocrError) as ei:
            cli.token_constraint(cli.build_parser().parse_args(["--prompt", "x"] + argv))
        assert ei.value.status == 1
    g = tmp_path / "bad.txt"
    g.write_text("12\nx\n")
    with pytest.raises(DsocrError):
        cli.token_constraint(cli.build_parser().parse_args(["--prompt", "x", "--allow-tokens-file", str(g)]))
