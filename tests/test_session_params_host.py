"""Per-request decode parameters, host side (no GPU): the C ABI exports, the scheduler against the scripted engine
of tests/test_session_host.py, the server's body -> DecodeParameters mapping and the CLI / server flags."""
import argparse
import ctypes as C
import os
import re

from dsocr import DecodeParameters, VisionSettings
from dsocr import cli, server
from dsocr.synth import SyntheticTokenizer

from test_session_host import FakeEngine, FakeSession, _prepare, _stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dsocr_session_open_ex", "dsocr_session_admit_params", "dsocr_session_head_steps", "dsocr_k_select_rows"]


def test_c_abi_exports_the_per_request_symbols():
    header = open(os.path.join(ROOT, "include", "dsocr.h")).read()
    declared = set(re.findall(r"\b(dsocr_[a-z0-9_]+)\s*\(", header))
    from dsocr._lib import EXPORTS, LIB_PATH, SESSION_PER_REQUEST
    L = C.CDLL(LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared and s in EXPORTS, s
        assert hasattr(L, s), s
    m = re.search(r"#define\s+DSOCR_SESSION_PER_REQUEST\s+(\d+)", header)
    assert m and int(m.group(1)) == SESSION_PER_REQUEST == 1


def test_row_params_struct_matches_the_header():
    """dsocr_row_params as ctypes lays it out: the field order and types of the header's declaration."""
    from dsocr._lib import RowParamsC
    header = open(os.path.join(ROOT, "include", "dsocr.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} dsocr_row_params;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [d.split()[-1] for d in body.split(";") if d.strip()]
    assert names == [n for n, _ in RowParamsC._fields_]


# ------------------------------------------------------------------ the scheduler against a scripted engine
class ParamSession(FakeSession):
    """FakeSession that also takes the per-request admission and records what it was given."""

    def admit(self, ids, mask=None, page=None, image_rows=None, max_new_tokens=None, seed=None, params=None):
        if params is not None:
            self.eng.log.append(("params", ids[1], params))
            max_new_tokens, seed = params.max_new_tokens, params.seed
        return super().admit(ids, mask, page, image_rows, max_new_tokens, seed)


class ParamEngine(FakeEngine):
    def open_session(self, slots, max_context, params, per_request=False):
        assert self.session is None or self.session.closed
        self.log.append(("per_request", per_request))
        self.session = ParamSession(self, slots, max_context, params)
        return self.session


def _sched(eng, per_request):
    from dsocr.scheduler import BatchScheduler
    return BatchScheduler(eng, SyntheticTokenizer(512), 2, 128, DecodeParameters(max_new_tokens=64),
                          VisionSettings(256, 128, True), prepare=_prepare, per_request_params=per_request)


FOREIGN = DecodeParameters(max_new_tokens=64, do_sample=True, temperature=0.7, top_p=0.9, repetition_penalty=1.3, seed=5)


def test_foreign_parameters_join_the_running_session():
    eng = ParamEngine({1: _stream(1, 30), 2: _stream(2, 9), 3: _stream(3, 12), 4: _stream(4, 200)})
    with _sched(eng, True) as s:
        assert s.compatible(FOREIGN, 12) and not s.compatible(DecodeParameters(max_new_tokens=65), 12)
        assert not s.compatible(DecodeParameters(max_new_tokens=8, use_cache=False), 12)
        assert not s.compatible(DecodeParameters(max_new_tokens=0), 12) and not s.compatible(FOREIGN, 128 - 64)
        a = s.submit("<image>doc:1")
        x = s.submit("<image>doc:2", params=FOREIGN)
        b = s.submit("<image>doc:3")
        big = s.submit("<image>doc:4", params=DecodeParameters(max_new_tokens=200))  # more than the session holds
        eng.gate.set()
        assert a.result(timeout=20).generated_tokens == _stream(1, 30)
        assert x.result(timeout=20).generated_tokens == _stream(2, 9)
        assert b.result(timeout=20).generated_tokens == _stream(3, 12)
        assert big.result(timeout=20).generated_tokens == _stream(4, 200)
        assert s.max_active == 2 and s.exclusive_runs == 1
    log = eng.log
    assert ("per_request", True) in log and ("per_request", False) not in log
    assert log.index(("admit", 2, 1)) < log.index(("retire", 1, 0))  # beside the running request, not after it
    assert ("decode", 2) not in log and ("decode", 4) in log
    given = {e[1]: e[2] for e in log if e[0] == "params"}
    assert given[2] == FOREIGN and given[1] == DecodeParameters(max_new_tokens=64)  # every admission brings its own


def test_foreign_parameters_still_run_alone_by_default():
    eng = ParamEngine({1: _stream(1, 30), 2: _stream(2, 9)})
    with _sched(eng, False) as s:
        assert not s.compatible(FOREIGN, 12)
        a = s.submit("<image>doc:1")
        x = s.submit("<image>doc:2", params=FOREIGN)
        eng.gate.set()
        assert a.result(timeout=20).generated_tokens == _stream(1, 30)
        assert x.result(timeout=20).generated_tokens == _stream(2, 9)
        assert s.exclusive_runs == 1
    log = eng.log
    assert ("per_request", True) not in log and not any(e[0] == "params" for e in log)
    assert log.index(("retire", 1, 0)) < log.index(("decode", 2))


# ------------------------------------------------------------------ server and CLI
def test_server_body_maps_to_the_requests_own_parameters():
    defaults = DecodeParameters(max_new_tokens=64)
    body = {"temperature": 0.7, "top_p": 0.9, "top_k": 40, "repetition_penalty": 1.2, "no_repeat_ngram_size": 4,
            "do_sample": True, "seed": 17, "unknown_field": 1, "use_cache": None}
    p = server.merge_decode(defaults, body, 32)
    assert p == DecodeParameters(max_new_tokens=32, do_sample=True, temperature=0.7, top_p=0.9, top_k=40,
                                 repetition_penalty=1.2, no_repeat_ngram_size=4, seed=17)
    assert server.merge_decode(defaults, {}, None) == defaults

    eng = ParamEngine({1: _stream(1, 6)})
    st = server.ServerState(eng, SyntheticTokenizer(512), "deepseek-ocr", VisionSettings(256, 128, True), defaults)
    ap = argparse.ArgumentParser()
    server.add_scheduler_args(ap)
    assert ap.parse_args([]).per_request_params is False
    args = ap.parse_args(["--slots", "2", "--max-context", "128", "--per-request-params"])
    assert args.per_request_params is True
    off = server.make_scheduler(st, 2, 128)
    on = server.make_scheduler(st, args.slots, args.max_context, args.per_request_params)
    try:
        assert off.per_request_params is False and not off.compatible(p, 12)
        assert on.per_request_params is True and on.compatible(p, 12)
    finally:
        off.close()
        on.close()


def test_cli_has_the_per_request_flag():
    a = cli.build_parser().parse_args(["--prompt", "<image>", "--image", "a.png"])
    assert a.per_request_params is False
    a = cli.build_parser().parse_args(["--prompt", "<image>", "--image", "a.png", "--slots", "2", "--per-request-params"])
    assert (a.slots, a.per_request_params) == (2, True)
