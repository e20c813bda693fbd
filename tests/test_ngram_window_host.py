"""The windowed no-repeat n-gram ban, host side (no GPU): validation and the NumPy reference of
``dsocr.ngram_window`` (against a direct restatement of the reference's ``banned_ngram_tokens`` for an unbounded
window); the exported symbols and the device-free check entry point; the scheduler's choice between the shared and
the exclusive path (the scripted session of test_logit_bias_host.py); the server's parsing of both request spellings
and its 400s; the command line."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from dsocr import DecodeParameters, DsocrError, VisionSettings
from dsocr import server
from dsocr.ngram_window import (DEFAULT_WINDOW, MAX_WHITELIST, UNBOUNDED, NgramWindow, NgramWindowError, apply,
                                candidates, make_ngram_window)
from dsocr.synth import SyntheticTokenizer
from test_logit_bias_host import FakeEngine, _sched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dsocr_ngram_window_check", "dsocr_generate_ngram_window", "dsocr_session_stage_ngram_window",
               "dsocr_k_ngram_window"]


def test_c_abi_exports_the_window_symbols():
    header = open(os.path.join(ROOT, "include", "dsocr.h")).read()
    declared = set(re.findall(r"\b(dsocr_[a-z0-9_]+)\s*\(", header))
    from dsocr._lib import EXPORTS, LIB_PATH, MAX_NGRAM_WHITELIST, SESSION_NGRAM_WINDOW, NgramWindowC
    L = C.CDLL(LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared and s in EXPORTS and hasattr(L, s), s
    flat = " ".join(header.split())
    assert "#define DSOCR_SESSION_NGRAM_WINDOW 32u" in flat and SESSION_NGRAM_WINDOW == 32
    assert "#define DSOCR_MAX_NGRAM_WHITELIST 32" in flat and MAX_NGRAM_WHITELIST == MAX_WHITELIST == 32
    assert ("typedef struct { int32_t ngram_size; int32_t window; const int32_t* whitelist; size_t n_whitelist; } "
            "dsocr_ngram_window;") in flat
    assert [f[0] for f in NgramWindowC._fields_] == ["ngram_size", "window", "whitelist", "n_whitelist"]
    assert C.sizeof(NgramWindowC) == 24
    from dsocr.engine import DeepseekOcrEngine, Session
    for fn in (DeepseekOcrEngine.decode, Session.admit, Session.admit_prefix, Session.admit_begin):
        assert "ngram_window" in inspect.signature(fn).parameters
    assert "ngram_window" in inspect.signature(DeepseekOcrEngine.open_session).parameters


# ------------------------------------------------------------------ dsocr.ngram_window
def test_validation():
    M = make_ngram_window
    assert M() is None and M(0) is None and M(0, 5, [1]) is None and M(None) is None
    assert M(30) == NgramWindow(30, DEFAULT_WINDOW, ()) and DEFAULT_WINDOW == 100
    assert M(30, 90, [7, 9, 7]) == NgramWindow(30, 90, (7, 9))           # repeats count once, first-seen order
    assert M(5, 2) == NgramWindow(5, 2, ())                              # w < g is legal (and never matches)
    assert M(np.int64(3), np.int32(8), np.array([1, 2])) == NgramWindow(3, 8, (1, 2))
    assert M(NgramWindow(3, 8, (1,))) == NgramWindow(3, 8, (1,)) and M(NgramWindow(0, 8)) is None
    assert M(2, 1, list(range(32)) + [0, 1]).whitelist == tuple(range(32))
    assert NgramWindow(1, 5).off and NgramWindow(0, 0).off and not NgramWindow(2, 1).off
    assert NgramWindow(2, 6, (3,)).kwargs() == {"ngram_window": NgramWindow(2, 6, (3,))}
    for bad in (dict(ngram_size=1), dict(ngram_size=-2), dict(ngram_size=2.0), dict(ngram_size="3"), dict(ngram_size=True),
                dict(ngram_size=3, window=0), dict(ngram_size=3, window=-1), dict(ngram_size=3, window=1.5),
                dict(ngram_size=3, whitelist=[-1]), dict(ngram_size=3, whitelist=[1.0]), dict(ngram_size=3, whitelist="12"),
                dict(ngram_size=3, whitelist=7), dict(ngram_size=3, whitelist=list(range(33))),
                dict(ngram_size=3, whitelist=[512], vocab=512), dict(window=5), dict(whitelist=[1]),
                dict(ngram_size=2 ** 31), dict(ngram_size=3, window=2 ** 31)):
        with pytest.raises(NgramWindowError):
            M(**bad)
    assert M(3, 5, [511], vocab=512).whitelist == (511,)


def _banned_ngram_tokens(sequence, ngram):
    """core/src/sampling.rs:141-158 restated: the continuations of every earlier occurrence of the last ngram - 1 ids."""
    banned = set()
    if ngram <= 1 or len(sequence) < ngram - 1:
        return banned
    history = {}
    for i in range(len(sequence) - ngram + 1):
        win = sequence[i:i + ngram]
        history.setdefault(tuple(win[:-1]), set()).add(win[-1])
    return set(history.get(tuple(sequence[len(sequence) - (ngram - 1):]), ()))


def test_numpy_reference_is_the_plain_ban_for_an_unbounded_window():
    r = np.random.default_rng(0)
    V = 40
    for trial in range(200):
        n = int(r.integers(0, 60))
        ctx = r.integers(0, int(r.integers(2, 5)), n).tolist()
        g = int(r.integers(2, 6))
        w = n + int(r.integers(0, 3)) if trial % 2 else UNBOUNDED
        assert set(candidates(ctx, g, w)) == _banned_ngram_tokens(ctx, g), (ctx, g, w)
        l = r.standard_normal(V).astype(np.float32)
        want = l.copy()
        for t in _banned_ngram_tokens(ctx, g):
            want[t] = -np.inf
        assert apply(l, ctx, NgramWindow(g, w)).tobytes() == want.tobytes()


def test_numpy_reference_window_whitelist_and_fallback():
    ctx = [1, 2, 7, 0, 1, 2, 8, 0, 0, 1, 2]
    assert candidates(ctx, 3, UNBOUNDED) == [7, 8] and candidates(ctx, 3, 7) == [8] and candidates(ctx, 3, 6) == []
    assert candidates(ctx, 3, 11) == [7, 8] and candidates(ctx, 3, 10) == [8]          # start 0 needs w >= n
    assert candidates([4, 4, 4], 3, 5) == [4] and candidates([4, 4], 3, 5) == [] and candidates(ctx, 1, 50) == []
    assert candidates(ctx, 12, 50) == []                                               # n < g
    l = np.arange(10, dtype=np.float32)
    out = apply(l, ctx, NgramWindow(3, 50, (7,)))
    assert out[8] == -np.inf and out[7] == 7 and np.isfinite(out).sum() == 9 and l[8] == 8   # a copy
    assert apply(l, ctx, None).tobytes() == l.tobytes() == apply(l, ctx, NgramWindow(0, 5)).tobytes()
    assert apply(l, [1, 50, 1, -3, 1], NgramWindow(2, 9)).tobytes() == l.tobytes()     # ids outside [0, V) are skipped
    only = np.full(10, -np.inf, np.float32)
    only[[7, 8]] = [1.0, 2.0]
    assert apply(only, ctx, NgramWindow(3, 50)).tobytes() == only.tobytes()            # nothing finite would be left
    only[3] = 0.5
    got = apply(only, ctx, NgramWindow(3, 50))
    assert got[7] == -np.inf and got[8] == -np.inf and got[3] == 0.5


# ------------------------------------------------------------------ the check entry point, without an engine
def _check(g, w, ids, vocab=512, n=None):
    from dsocr._lib import NgramWindowC, lib
    arr = (C.c_int32 * max(len(ids), 1))(*ids)
    rec = NgramWindowC(g, w, C.cast(arr, C.POINTER(C.c_int32)), len(ids) if n is None else n)
    st = lib().dsocr_ngram_window_check(C.byref(rec), vocab)
    return st, (lib().dsocr_last_error() or b"").decode()


def test_c_abi_check():
    from dsocr._lib import NgramWindowC, lib
    assert lib().dsocr_ngram_window_check(None, 512) == 0                              # "no record"
    for ok in ((30, 90, [3, 4]), (2, 1, []), (5, 2, []), (0, 0, []), (1, -5, [7]), (3, 2 ** 31 - 1, list(range(32))),
               (2, 5, list(range(32)) + [0, 31]), (2, 5, [511])):
        assert _check(*ok)[0] == 0, ok
    for bad in ((2, 0, []), (3, -1, []), (2, 5, [512]), (2, 5, [-1]), (2, 5, list(range(33))), (0, 0, [600])):
        st, msg = _check(*bad)
        assert st == 1 and msg.startswith("EINVAL: n-gram window"), (bad, st, msg)
    rec = NgramWindowC(2, 5, None, 3)                                                  # a count without a list
    assert lib().dsocr_ngram_window_check(C.byref(rec), 512) == 1
    assert _check(2, 5, [], vocab=0)[0] == 1
    from dsocr.engine import _ngram_window, _ngram_window_c
    with pytest.raises(DsocrError) as ei:
        _ngram_window(NgramWindow(2, 0), 512)
    assert ei.value.status == 1
    with pytest.raises(DsocrError):
        _ngram_window({"ngram_size": 2, "window_size": 5}, 512)                        # (the mapping's key is `window`)
    assert _ngram_window(None, 512) is None and _ngram_window(NgramWindow(0, 9), 512) is None
    assert _ngram_window({"ngram_size": 3, "window": 8, "whitelist": [1]}, 512) == NgramWindow(3, 8, (1,))
    keep = []
    c = _ngram_window_c(NgramWindow(30, 90, (3, 4)), keep)
    assert (c.ngram_size, c.window, c.n_whitelist, c.whitelist[0], c.whitelist[1]) == (30, 90, 2, 3, 4) and keep
    assert _ngram_window_c(None, keep) is None


# ------------------------------------------------------------------ scheduler routing
def test_scheduler_shared_and_exclusive_paths():
    img = np.zeros((8, 8, 3), np.uint8)
    rec = NgramWindow(30, 90, (3, 4))
    eng = FakeEngine()
    with _sched(eng, ngram_window=True) as s:    # the flag: a windowed request shares the session
        s.submit("11", [img]).result(timeout=20)
        s.submit("12", [img], ngram_window=rec).result(timeout=20)
        s.submit("13", [img], ngram_window=NgramWindow(0, 5)).result(timeout=20)       # off: no record
        assert s.exclusive_runs == 0
    assert eng.log[0] == ("open", {"ngram_window": True})
    assert ("admit", 11, {}) in eng.log and ("admit", 12, {"ngram_window": rec}) in eng.log and ("admit", 13, {}) in eng.log
    eng = FakeEngine()
    with _sched(eng) as s:                       # no flag: it drains the session and decodes alone, with the argument
        s.submit("11", [img]).result(timeout=20)
        out = s.submit("12", [img], ngram_window=rec).result(timeout=20)
        assert s.exclusive_runs == 1 and out.generated_tokens == [1, 2, 3]
        for bad in (NgramWindow(2, 0), NgramWindow(2, 5, (512,)), (2, 5)):
            with pytest.raises(ValueError):
                s.submit("13", [img], ngram_window=bad).result(timeout=20)
        s.submit("14", [img], ngram_window=None).result(timeout=20)
        assert s.exclusive_runs == 1
    assert eng.log[0] == ("open", {}) and ("admit", 11, {}) in eng.log and ("admit", 14, {}) in eng.log
    assert ("decode", 12, {"ngram_window": rec}) in eng.log
    assert not any(e[1] == 13 for e in eng.log if e[0] in ("decode", "admit"))


# ------------------------------------------------------------------ server and command line
def test_server_parsing_and_400s():
    P = server.parse_ngram_window
    assert P({}) is None and P({"ngram_size": None}) is None and P({"ngram_size": 0}) is None
    assert P({"vllm_xargs": {}}) is None and P({"vllm_xargs": None}) is None
    recipe = {"ngram_size": 30, "window_size": 90, "whitelist_token_ids": [128821, 128822]}
    want = {"ngram_window": NgramWindow(30, 90, (128821, 128822))}
    assert P(recipe) == want and P({"vllm_xargs": recipe}) == want                     # both spellings
    assert P(recipe, 129280) == want
    assert P({"ngram_size": 30}) == {"ngram_window": NgramWindow(30, 100, ())}         # upstream's default window
    assert P({"vllm_xargs": {"ngram_size": 30}}) == {"ngram_window": NgramWindow(30, 100, ())}
    # a top-level field wins over the one in vllm_xargs
    assert P({"ngram_size": 5, "vllm_xargs": recipe}) == {"ngram_window": NgramWindow(5, 90, (128821, 128822))}
    for body in ({"ngram_size": 1}, {"ngram_size": -1}, {"ngram_size": "30"}, {"ngram_size": 2.5}, {"ngram_size": True},
                 {"ngram_size": 3, "window_size": 0}, {"ngram_size": 3, "window_size": "9"},
                 {"ngram_size": 3, "whitelist_token_ids": [-1]}, {"ngram_size": 3, "whitelist_token_ids": "1,2"},
                 {"ngram_size": 3, "whitelist_token_ids": list(range(33))}, {"window_size": 90},
                 {"whitelist_token_ids": [1]}, {"vllm_xargs": [1]}, {"vllm_xargs": {"ngram_size": 1}},
                 {"vllm_xargs": {"ngram_size": 3, "window_size": -2}}):
        with pytest.raises(server.ApiError) as ei:
            P(body)
        assert ei.value.status == 400, body
    with pytest.raises(server.ApiError) as ei:
        P({"ngram_size": 3, "whitelist_token_ids": [512]}, 512)
    assert ei.value.status == 400

    # the request path: the record reaches decode as a keyword, on both routes and in both spellings
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
    small = {"ngram_size": 30, "window_size": 90, "whitelist_token_ids": [3, 4]}
    for kind, key in (("chat", "messages"), ("responses", "input")):
        for extra in (small, {"vllm_xargs": small}):
            eng.log.clear()
            how, body = server.handle_generation(st, {"model": "deepseek-ocr", key: msg, **extra}, kind)
            assert how == "json"
            assert [e[2] for e in eng.log if e[0] == "decode"] == [{"ngram_window": NgramWindow(30, 90, (3, 4))}]
        for bad in ({"ngram_size": 3, "window_size": 0}, {"vllm_xargs": {"ngram_size": 3, "whitelist_token_ids": [512]}}):
            with pytest.raises(server.ApiError) as ei:
                server.handle_generation(st, {"model": "deepseek-ocr", key: msg, **bad}, kind)
            assert ei.value.status == 400
        eng.log.clear()
        server.handle_generation(st, {"model": "deepseek-ocr", key: msg, "ngram_size": 0}, kind)
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
    assert p.parse_args([]).ngram_window is False and p.parse_args(["--slots", "2", "--ngram-window"]).ngram_window is True
    st = server.ServerState(FakeEngine(), SyntheticTokenizer(512), "deepseek-ocr", VisionSettings(256, 128, True),
                            DecodeParameters(max_new_tokens=8))
    with pytest.raises(ValueError, match="--slots"):
        server.make_scheduler(st, 0, 128, ngram_window=True)
    on = server.make_scheduler(st, 2, 128, ngram_window=True)
    try:
        assert on.ngram_window is True
    finally:
        on.close()
    with pytest.raises(SystemExit):
        server.main(["--ngram-window"])
    assert "--ngram-window needs --slots" in capsys.readouterr().err
    from dsocr import cli
    parse = lambda *argv: cli.build_parser().parse_args(["--prompt", "x", *argv])
    a = parse("--ngram-window-size", "30", "--ngram-window", "90", "--ngram-whitelist", "1,2")
    assert cli.ngram_window_arguments(a) == {"ngram_window": NgramWindow(30, 90, (1, 2))}
    assert cli.token_constraint(a) == cli.ngram_window_arguments(a)
    assert cli.ngram_window_arguments(parse("--ngram-window-size", "30")) == {"ngram_window": NgramWindow(30, 100, ())}
    assert cli.ngram_window_arguments(parse()) == {} and cli.ngram_window_arguments(parse("--ngram-window-size", "0")) == {}
    for argv in (["--ngram-window-size", "1"], ["--ngram-window-size", "3", "--ngram-window", "0"],
                 ["--ngram-window-size", "3", "--ngram-whitelist", "a,b"], ["--ngram-window-size", "3", "--ngram-whitelist", "-4"],
                 ["--ngram-window", "9"], ["--ngram-window-size", "3", "--slots", "2"]):
        with pytest.raises(DsocrError) as ei:
            cli.ngram_window_arguments(parse(*argv))
        assert ei.value.status == 1
