"""Frequency / presence penalties and min-p, host side (no GPU): validation, the off test, ln_min_p and the NumPy
reference of ``dsocr.penalties``; the exported symbols and the device-free check entry point; the scheduler's choice
between the shared and the exclusive path (the scripted session of test_logit_bias_host.py); the server's request
parsing and its 400s; the command line."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

from dsocr import DecodeParameters, DsocrError, VisionSettings
from dsocr import server
from dsocr.penalties import Penalties, PenaltyError, apply, is_off, ln_min_p, make_penalties, min_p_keep
from dsocr.synth import SyntheticTokenizer
from test_logit_bias_host import FakeEngine, _sched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dsocr_penalties_check", "dsocr_generate_penalties", "dsocr_session_stage_penalties",
               "dsocr_k_out_penalty", "dsocr_k_sample_stoch_min_p"]
INF, NAN = math.inf, math.nan


def test_c_abi_exports_the_penalty_symbols():
    header = open(os.path.join(ROOT, "include", "dsocr.h")).read()
    declared = set(re.findall(r"\b(dsocr_[a-z0-9_]+)\s*\(", header))
    from dsocr._lib import EXPORTS, LIB_PATH, SESSION_PENALTIES, PenaltiesC
    L = C.CDLL(LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared and s in EXPORTS and hasattr(L, s), s
    flat = " ".join(header.split())
    assert "#define DSOCR_SESSION_PENALTIES 16u" in flat and SESSION_PENALTIES == 16
    assert "typedef struct { float frequency; float presence; double min_p; } dsocr_penalties;" in flat
    assert [f[0] for f in PenaltiesC._fields_] == ["frequency", "presence", "min_p"] and C.sizeof(PenaltiesC) == 16
    from dsocr.engine import DeepseekOcrEngine, Session
    for fn in (DeepseekOcrEngine.decode, Session.admit, Session.admit_prefix, Session.admit_begin):
        assert {"frequency_penalty", "presence_penalty", "min_p"} <= set(inspect.signature(fn).parameters)


# ------------------------------------------------------------------ dsocr.penalties
def test_validation_off_and_ln_min_p():
    assert make_penalties() is None and make_penalties(0, 0.0, 0) is None and make_penalties(None, -0.0, None) is None
    assert make_penalties(0.5) == Penalties(0.5, 0.0, 0.0) and make_penalties(None, -1, None) == Penalties(0.0, -1.0, 0.0)
    assert make_penalties(min_p=1) == Penalties(0.0, 0.0, 1.0)
    assert make_penalties(np.float32(0.1)).frequency == float(np.float32(0.1))       # held as f32
    assert make_penalties(0.1).frequency == float(np.float32(0.1))
    assert make_penalties(5.0).frequency == 5.0                                      # the engine sets no range ...
    for bad in (dict(frequency_penalty=2.5), dict(presence_penalty=-2.01)):          # ... the server's bound does
        with pytest.raises(PenaltyError):
            make_penalties(bound=2.0, **bad)
    assert make_penalties(2.0, -2.0, bound=2.0) == Penalties(2.0, -2.0, 0.0)
    for bad in (dict(frequency_penalty=NAN), dict(frequency_penalty=INF), dict(presence_penalty=-INF),
                dict(presence_penalty=1e39), dict(min_p=NAN), dict(min_p=-0.01), dict(min_p=1.0001), dict(min_p=INF),
                dict(frequency_penalty="1"), dict(presence_penalty=True), dict(min_p=[0.1])):
        with pytest.raises(PenaltyError):
            make_penalties(**bad)
    assert is_off(0, 0, 0) and is_off(0.0, -0.0, -1.0) and not is_off(0, 0, 1e-300) and not is_off(1e-30, 0, 0)
    assert Penalties().off and not Penalties(0.0, 0.0, 0.5).off
    assert ln_min_p(0) == -INF and ln_min_p(-1) == -INF and ln_min_p(1.0) == 0.0
    assert ln_min_p(0.1) == math.log(0.1) and Penalties(0, 0, 0.05).ln_min_p == math.log(0.05)


def test_numpy_reference():
    l = np.array([1.0, -2.0, -INF, 0.5, 3.0], np.float32)
    out = apply(l, [4, 1, 4, 9, -1, 2, 4], 0.7, 0.25)
    f, p = np.float32(0.7), np.float32(0.25)
    assert out[0] == l[0] and out[3] == l[3] and out[2] == -INF                      # untouched, -inf stays -inf
    assert out[4] == np.float32(l[4] - np.float32(np.float32(f * np.float32(3)) + p))
    assert out[1] == np.float32(l[1] - np.float32(f + p))
    assert out.dtype == np.float32 and apply(l, [], 0.7, 0.25).tobytes() == l.tobytes()
    assert apply(l, [4, 4], 0.0, 0.0).tobytes() == l.tobytes() and l[4] == 3.0       # a copy: the input is left alone
    assert apply(l, [0], 0.0, -1.5)[0] == np.float32(2.5)                            # a negative presence raises
    q = np.array([0.0, -1.0, -2.0, -2.5, 0.0])
    assert min_p_keep(q, math.log(0.1)).tolist() == [True, True, True, False, True]  # ln 0.1 = -2.30
    assert min_p_keep(q, 0.0).tolist() == [True, False, False, False, True]          # min_p = 1: the ties of the maximum
    assert min_p_keep(q, -INF).all() and min_p_keep([], -1.0).shape == (0,)


# ------------------------------------------------------------------ the check entry point, without an engine
def _check(f, p, m):
    from dsocr._lib import PenaltiesC, lib
    rec = PenaltiesC(f, p, m)
    st = lib().dsocr_penalties_check(C.byref(rec))
    return st, (lib().dsocr_last_error() or b"").decode()


def test_c_abi_check():
    from dsocr._lib import lib
    assert lib().dsocr_penalties_check(None) == 0                                    # "no record"
    for ok in ((0.0, 0.0, 0.0), (2.0, -2.0, 1.0), (-7.5, 100.0, 0.0), (0.0, 0.0, 1e-300), (0.0, 0.0, -0.0)):
        assert _check(*ok)[0] == 0, ok
    for bad in ((NAN, 0.0, 0.0), (INF, 0.0, 0.0), (0.0, -INF, 0.0), (0.0, NAN, 0.0), (0.0, 0.0, NAN), (0.0, 0.0, -1e-9),
                (0.0, 0.0, 1.0000001), (0.0, 0.0, INF)):
        st, msg = _check(*bad)
        assert st == 1 and msg.startswith("EINVAL: penalties"), (bad, st, msg)
    from dsocr.engine import _penalties, _penalties_c
    with pytest.raises(DsocrError) as ei:
        _penalties(None, None, 1.5)
    assert ei.value.status == 1
    assert _penalties(0, 0, 0) is None and _penalties_c(None) is None
    rec = _penalties_c(_penalties(0.5, -0.25, 0.1))
    assert (rec.frequency, rec.presence, rec.min_p) == (0.5, -0.25, 0.1)


# ------------------------------------------------------------------ scheduler routing
def test_scheduler_shared_and_exclusive_paths():
    img = np.zeros((8, 8, 3), np.uint8)
    want = {"frequency_penalty": 0.5, "presence_penalty": 0.0, "min_p": 0.25}
    eng = FakeEngine()
    with _sched(eng, penalties=True) as s:    # the flag: a penalised request shares the session
        s.submit("11", [img]).result(timeout=20)
        s.submit("12", [img], frequency_penalty=0.5, min_p=0.25).result(timeout=20)
        s.submit("13", [img], frequency_penalty=0.0, presence_penalty=0, min_p=0).result(timeout=20)  # off: no record
        assert s.exclusive_runs == 0
    assert eng.log[0] == ("open", {"penalties": True})
    assert ("admit", 11, {}) in eng.log and ("admit", 12, want) in eng.log and ("admit", 13, {}) in eng.log
    eng = FakeEngine()
    with _sched(eng) as s:                    # no flag: it drains the session and decodes alone, with the arguments
        s.submit("11", [img]).result(timeout=20)
        out = s.submit("12", [img], presence_penalty=-1.0).result(timeout=20)
        assert s.exclusive_runs == 1 and out.generated_tokens == [1, 2, 3]
        bad = s.submit("13", [img], min_p=1.5)
        with pytest.raises(ValueError):
            bad.result(timeout=20)
        s.submit("14", [img], min_p=0.0).result(timeout=20)   # an off record shares the session without the flag
        assert s.exclusive_runs == 1
    assert eng.log[0] == ("open", {}) and ("admit", 11, {}) in eng.log and ("admit", 14, {}) in eng.log
    assert ("decode", 12, {"frequency_penalty": 0.0, "presence_penalty": -1.0, "min_p": 0.0}) in eng.log
    assert not any(e[1] == 13 for e in eng.log if e[0] in ("decode", "admit"))


def test_penalised_retry_on_a_cached_page_is_a_prefix_hit():
    img = np.random.default_rng(3).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    eng = FakeEngine()
    with _sched(eng, penalties=True, prefix_cache=4) as s:
        s.submit("11", [img]).result(timeout=20)
        s.submit("12", [img.copy()], min_p=0.1).result(timeout=20)
        assert (s.prefix_hits, s.prefix_misses) == (1, 1)
    assert ("admit_prefix", 12, {"frequency_penalty": 0.0, "presence_penalty": 0.0, "min_p": 0.1}) in eng.log


# ------------------------------------------------------------------ server and command line
def test_server_parsing_and_400s():
    P = server.parse_penalties
    assert P({}) is None and P({"frequency_penalty": 0, "presence_penalty": None, "min_p": 0.0}) is None
    assert P({"frequency_penalty": 1.5}) == {"frequency_penalty": 1.5, "presence_penalty": 0.0, "min_p": 0.0}
    assert P({"presence_penalty": -2, "min_p": 1}) == {"frequency_penalty": 0.0, "presence_penalty": -2.0, "min_p": 1.0}
    for body in ({"frequency_penalty": 2.01}, {"presence_penalty": -2.5}, {"frequency_penalty": "1"},
                 {"presence_penalty": True}, {"min_p": -0.1}, {"min_p": 1.1}, {"min_p": "0.1"}, {"frequency_penalty": [1]},
                 {"frequency_penalty": float("nan")}, {"min_p": float("nan")}):
        with pytest.raises(server.ApiError) as ei:
            P(body)
        assert ei.value.status == 400, body
    # the request path: the fields reach decode as keywords, on both routes
    class Eng(FakeEngine):
        def decode(self, tokenizer, prompt, images, vision, params, stream=None, **kw):
            from dsocr.engine import DecodeOutcome
            if kw:
                self.log.append(("decode", prompt, dict(kw)))
            return DecodeOutcome("x", 7, 3, [1, 2, 3])

    eng = Eng()
    st = server.ServerState(eng, SyntheticTokenizer(512), "deepseek-ocr", VisionSettings(256, 128, True),
                            DecodeParameters(max_new_tokens=8))
    msg = [{"role": "user", "content": [{"type": "text", "text": "5"},
                                         {"type": "image_url", "image_url": {"url": _png_url()}}]}]
    for kind, key in (("chat", "messages"), ("responses", "input")):
        eng.log.clear()
        how, body = server.handle_generation(st, {"model": "deepseek-ocr", key: msg, "frequency_penalty": 0.5,
                                                  "min_p": 0.2}, kind)
        assert how == "json"
        assert [e[2] for e in eng.log if e[0] == "decode"] == [{"frequency_penalty": 0.5, "presence_penalty": 0.0, "min_p": 0.2}]
        with pytest.raises(server.ApiError) as ei:
            server.handle_generation(st, {"model": "deepseek-ocr", key: msg, "presence_penalty": 3}, kind)
        assert ei.value.status == 400
        eng.log.clear()
        server.handle_generation(st, {"model": "deepseek-ocr", key: msg, "frequency_penalty": 0}, kind)
        assert [e[2] for e in eng.log if e[0] == "decode"] == []   # nothing asked: the plain decode (no keywords logged)


def _png_url():
    import base64
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(buf, format="PNG")
    return "data:image/png;base64," + base64.b64encode(buf.getvalue()).decode()


def test_server_flag_and_cli_options(capsys):
    import argparse
    p = argparse.ArgumentParser()
    server.add_scheduler_args(p)
    assert p.parse_args([]).penalties is False and p.parse_args(["--slots", "2", "--penalties"]).penalties is True
    st = server.ServerState(FakeEngine(), SyntheticTokenizer(512), "deepseek-ocr", VisionSettings(256, 128, True),
                            DecodeParameters(max_new_tokens=8))
    with pytest.raises(ValueError, match="--slots"):
        server.make_scheduler(st, 0, 128, penalties=True)
    on = server.make_scheduler(st, 2, 128, penalties=True)
    try:
        assert on.penalties is True
    finally:
        on.close()
    with pytest.raises(SystemExit):
        server.main(["--penalties"])
    assert "--penalties needs --slots" in capsys.readouterr().err
    from dsocr import cli
    a = cli.build_parser().parse_args(["--prompt", "<image>", "--frequency-penalty", "0.5", "--presence-penalty", "-1",
                                       "--min-p", "0.05"])
    assert cli.penalty_arguments(a) == {"frequency_penalty": 0.5, "presence_penalty": -1.0, "min_p": 0.05}
    assert cli.token_constraint(a) == cli.penalty_arguments(a)
    assert cli.penalty_arguments(cli.build_parser().parse_args(["--prompt", "x"])) == {}
    assert cli.penalty_arguments(cli.build_parser().parse_args(["--prompt", "x", "--min-p", "0"])) == {}
    for argv in (["--min-p", "1.5"], ["--min-p", "-1"], ["--frequency-penalty", "nan"], ["--presence-penalty", "inf"],
                 ["--min-p", "0.1", "--slots", "2"]):
        with pytest.raises(DsocrError) as ei:
            cli.penalty_arguments(cli.build_parser().parse_args(["--prompt", "x"] + argv))
        assert ei.value.status == 1
