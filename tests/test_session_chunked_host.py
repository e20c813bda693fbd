"""Chunked admission, host side (no GPU): the C ABI exports, the scheduler's slice / burst bookkeeping against the
scripted engines of test_session_host.py and test_session_prefix_host.py, and the server and CLI flags."""
import argparse
import ctypes as C
import os
import re

import pytest

import test_session_host as H
import test_session_prefix_host as P
from dsocr import DecodeParameters, DsocrError, VisionSettings
from dsocr import cli, server
from dsocr.synth import SyntheticTokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dsocr_session_admit_begin", "dsocr_session_admit_advance", "dsocr_session_admit_cancel",
               "dsocr_session_admit_progress", "dsocr_k_attention_chunk"]
SLICES = 3  # slices of every scripted admission


def test_c_abi_exports_the_chunked_admission_symbols():
    header = open(os.path.join(ROOT, "include", "dsocr.h")).read()
    declared = set(re.findall(r"\b(dsocr_[a-z0-9_]+)\s*\(", header))
    from dsocr._lib import EXPORTS, LIB_PATH
    L = C.CDLL(LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared and s in EXPORTS, s
        assert hasattr(L, s), s
    assert "DSOCR_SESSION_ADMIT_PENDING" in header
    from dsocr.engine import Session
    for m in ("admit_begin", "admit_advance", "admit_cancel", "admit_progress"):
        assert callable(getattr(Session, m)), m


def _chunked(base):
    """`base` (a scripted session) with an admission in SLICES slices: the last one calls the plain `admit`."""
    class Chunked(base):
        pend = None

        def admit_begin(self, ids, mask=None, page=None, image_rows=None, chunk_rows=128, **kw):
            assert self.pend is None and chunk_rows >= 32 and len(self.active) < self.slots
            self.pend = [SLICES, (ids, mask, page, image_rows), kw]
            self.eng.log.append(("begin", chunk_rows))
            return 1

        def admit_advance(self):
            self.pend[0] -= 1
            self.eng.log.append(("advance",))
            if self.pend[0]:
                return False, -1
            (ids, mask, page, rows), kw = self.pend[1:]
            self.pend = None
            return True, base.admit(self, ids, mask, page, rows, **kw)

        def admit(self, *a, **kw):
            assert self.pend is None, "admit while an admission is pending"
            return base.admit(self, *a, **kw)
    return Chunked


class Engine(H.FakeEngine):
    def open_session(self, slots, max_context, params):
        assert self.session is None or self.session.closed
        self.session = _chunked(H.FakeSession)(self, slots, max_context, params)
        return self.session


def _sched(eng, admit_chunk, slots=2):
    from dsocr.scheduler import BatchScheduler
    return BatchScheduler(eng, SyntheticTokenizer(512), slots, 128, DecodeParameters(max_new_tokens=64),
                          VisionSettings(256, 128, True), prepare=H._prepare, admit_chunk=admit_chunk)


def _calls(eng):
    return [e for e in eng.log if e[0] in ("begin", "advance", "admit", "step")]


def test_slices_alternate_with_bursts():
    eng = Engine({1: H._stream(1, 40), 2: H._stream(2, 4)})
    with _sched(eng, 64) as s:   # the gate is closed: the first burst waits, so both requests are queued before it
        f1 = s.submit("<image>doc:1")
        f2 = s.submit("<image>doc:2")
        eng.gate.set()
        assert f1.result(timeout=20).generated_tokens == H._stream(1, 40)
        assert f2.result(timeout=20).generated_tokens == H._stream(2, 4)
        assert (s.admit_slices, s.chunked_admissions) == (2 * SLICES, 2)
        events = list(s.events)
    # nothing runs during the first admission: its slices back to back (its first burst then waits at the gate until
    # the second request is queued); the second one's slices alternate with bursts of 8
    assert _calls(eng)[:14] == [("begin", 64), ("advance",), ("advance",), ("advance",), ("admit", 1, 0), ("step", 1, 8),
                                ("begin", 64), ("advance",), ("step", 1, 8), ("advance",), ("step", 1, 8),
                                ("advance",), ("admit", 2, 1), ("step", 2, 8)]
    assert events[:10] == [("slice", "prefill", 0), ("slice", "prefill", 0), ("slice", "prefill", 1), ("burst", 1, 8),
                           ("slice", "prefill", 1), ("burst", 1, 8), ("slice", "prefill", 1), ("burst", 1, 8),
                           ("slice", "prefill", 2), ("burst", 2, 8)]


def test_burst_is_one_step_while_a_request_streams():
    eng = Engine({1: H._stream(1, 6), 2: H._stream(2, 3)})
    eng.gate.set()
    seen = []
    with _sched(eng, 32) as s:
        f1 = s.submit("<image>doc:1", on_token=lambda n, t: seen.append(n))
        assert s.submit("<image>doc:2").result(timeout=20).generated_tokens == H._stream(2, 3)
        assert f1.result(timeout=20).generated_tokens == H._stream(1, 6)
    assert seen == [1, 2, 3, 4, 5, 6]
    steps = [e for e in eng.log if e[0] == "step"]
    assert steps and {e[2] for e in steps} == {1}


def test_admit_chunk_zero_issues_todays_calls():
    eng = Engine({1: H._stream(1, 5), 2: H._stream(2, 5)})
    eng.gate.set()
    with _sched(eng, 0) as s:
        for k in (1, 2):
            assert s.submit(f"<image>doc:{k}").result(timeout=20).generated_tokens == H._stream(k, 5)
        assert s.events == [] and s.admit_slices == 0 and s.admit_chunk == 0
    assert not any(e[0] in ("begin", "advance") for e in eng.log)
    assert [e[:2] for e in eng.log if e[0] == "admit"] == [("admit", 1), ("admit", 2)]
    from dsocr.scheduler import BatchScheduler
    import inspect
    assert inspect.signature(BatchScheduler.__init__).parameters["admit_chunk"].default == 0
    with pytest.raises(ValueError):
        _sched(Engine({}), 31)


def test_exclusive_requests_stay_exclusive():
    eng = Engine({1: H._stream(1, 5), 2: H._stream(2, 5)})
    eng.gate.set()
    with _sched(eng, 32) as s:
        assert s.submit("<image>doc:1").result(timeout=20).generated_tokens == H._stream(1, 5)
        out = s.submit("<image>doc:2", params=DecodeParameters(max_new_tokens=64, repetition_penalty=1.3)).result(timeout=20)
        assert out.generated_tokens == H._stream(2, 5) and s.exclusive_runs == 1
    assert ("decode", 2) in eng.log and [e for e in eng.log if e[0] == "begin"] == [("begin", 32)]


def test_prefix_hits_bypass_chunking_and_the_prefix_is_kept_after_a_chunked_admission():
    class PrefixEngine(P.FakeEngine):
        def open_session(self, slots, max_context, params, **kw):
            return _chunked(P.FakeSession)(self, slots, max_context, params)

    from dsocr.scheduler import BatchScheduler
    eng = PrefixEngine()
    a = P._img(1)
    with BatchScheduler(eng, SyntheticTokenizer(512), 2, 128, DecodeParameters(max_new_tokens=8),
                        VisionSettings(256, 128, True), prepare=P._prepare_for(eng), prefix_cache=4, admit_chunk=32) as s:
        P._run(s, "11", [a])     # a miss: admitted in slices, its prefix kept when the last slice completes
        P._run(s, "12", [a])     # a hit: admit_prefix in one call
        assert (s.prefix_hits, s.prefix_misses, s.chunked_admissions) == (1, 1, 1)
    kinds = [e[0] for e in eng.log if e[0] in ("begin", "advance", "admit", "keep", "admit_prefix")]
    assert kinds == ["begin"] + ["advance"] * SLICES + ["admit", "keep", "admit_prefix"]


def test_server_and_cli_flags(capsys):
    p = argparse.ArgumentParser()
    server.add_scheduler_args(p)
    assert p.parse_args([]).admit_chunk == 0
    assert p.parse_args(["--slots", "4", "--admit-chunk", "128"]).admit_chunk == 128
    st = server.ServerState(P.FakeEngine(), SyntheticTokenizer(512), "deepseek-ocr", VisionSettings(256, 128, True),
                            DecodeParameters(max_new_tokens=8))
    with pytest.raises(ValueError, match="--slots"):
        server.make_scheduler(st, 0, 128, admit_chunk=128)
    with pytest.raises(ValueError, match=">= 32"):
        server.make_scheduler(st, 2, 128, admit_chunk=16)
    on = server.make_scheduler(st, 2, 128, admit_chunk=128)
    try:
        assert on.admit_chunk == 128
    finally:
        on.close()
    for argv in (["--admit-chunk", "128"], ["--slots", "2", "--admit-chunk", "16"]):
        with pytest.raises(SystemExit):
            server.main(argv)
        assert "--admit-chunk needs --slots and ROWS >= 32" in capsys.readouterr().err
    cp = cli.build_parser()
    assert cp.parse_args(["--prompt", "x"]).admit_chunk == 0
    args = cp.parse_args(["--prompt", "x", "--slots", "2", "--admit-chunk", "64"])
    assert args.admit_chunk == 64
    cli.check_admit_chunk(args)
    for argv in (["--prompt", "x", "--admit-chunk", "64"], ["--prompt", "x", "--slots", "2", "--admit-chunk", "8"]):
        with pytest.raises(DsocrError, match="--admit-chunk needs --slots"):
            cli.run_inference(cp.parse_args(argv))
