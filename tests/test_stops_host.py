"""Stop sequences, the host side: merging and checking, the NumPy/Python reference ``first_stop``,
the two hold-backs of a stream, the server's request parsing and ``stop_reason``.  No GPU."""
import ctypes as C
import io
import json
import base64

import numpy as np
import pytest

from dsocr import DecodeOutcome, DecodeParameters, VisionSettings, server
from dsocr._lib import MAX_STOP_LEN, MAX_STOP_SEQS, SESSION_STOP, StopHitC, StopSetC, lib
from dsocr.stops import StopError, StopSet, TextStop, TokenHoldback, apply_stops, first_stop, merge_stops
from dsocr.synth import SyntheticTokenizer

VOCAB = 512
TOK = SyntheticTokenizer(VOCAB)


def _check(seqs, vocab=VOCAB):
    """dsocr_stop_set_check on the sequences (no engine, no device)."""
    flat = np.asarray([t for q in seqs for t in q] or [0], np.int64)
    lens = (C.c_size_t * max(len(seqs), 1))(*[len(q) for q in seqs])
    rec = StopSetC(flat.ctypes.data_as(C.POINTER(C.c_int64)), lens, len(seqs))
    return lib().dsocr_stop_set_check(C.byref(rec), vocab)


def test_abi_constants_and_records():
    assert (MAX_STOP_SEQS, MAX_STOP_LEN, SESSION_STOP) == (16, 32, 8)
    assert C.sizeof(StopHitC) == 8 and C.sizeof(StopSetC) == 2 * C.sizeof(C.c_void_p) + C.sizeof(C.c_size_t)


@pytest.mark.parametrize("seqs,ok", [
    ([(5,)], True),
    ([tuple(range(20, 20 + 32))], True),                       # 32 ids
    ([tuple(range(20, 20 + 33))], False),                      # 33 ids
    ([(i + 20,) for i in range(16)], True),                    # 16 sequences
    ([(i + 20,) for i in range(17)], False),                   # 17 sequences
    ([()], False),                                             # a length of 0
    ([(VOCAB - 1,)], True), ([(VOCAB,)], False), ([(-1,)], False),
    ([(5, 6), (5, 6)], False),                                 # two identical sequences
    ([(5, 6), (5,), (6,)], True),
    ([], True),                                                # n == 0: "no stops"
])
def test_stop_set_check_and_merge_agree(seqs, ok):
    assert (_check(seqs) == 0) is ok
    from dsocr.stops import check_sequences
    if ok:
        check_sequences(seqs, VOCAB)
    else:
        with pytest.raises(StopError) as e:
            check_sequences(seqs, VOCAB)
        assert e.value.status == 1
    assert lib().dsocr_stop_set_check(None, VOCAB) == 0        # a NULL pointer: "no stops"


def test_merge_stops():
    assert merge_stops(None, None, TOK, VOCAB) is None and merge_stops([], [], TOK, VOCAB) is None
    one = merge_stops("end of table", None, TOK, VOCAB)
    assert one.seqs == (tuple(TOK.encode("end of table").ids),) and one.labels == ("end of table",)
    assert one.strings == ("end of table",) and len(one.seqs[0]) == 3
    both = merge_stops(["a b", "a b", "c"], [7, 7, 9], TOK, VOCAB)      # duplicates collapse
    assert [len(q) for q in both.seqs] == [2, 1, 1, 1] and both.labels == ("a b", "c", 7, 9)
    same = merge_stops(["c"], [TOK.encode("c").ids[0]], TOK, VOCAB)    # a string and the id it encodes to
    assert len(same.seqs) == 1 and same.labels == ("c",)
    assert len(merge_stops(None, range(20, 36), TOK, VOCAB).seqs) == 16
    assert len(merge_stops(" ".join(f"w{i}" for i in range(32)), None, TOK, VOCAB).seqs[0]) == 32
    for bad in (dict(stop=""), dict(stop=[3]), dict(stop=3), dict(stop="   "), dict(stop_token_ids=[VOCAB]),
                dict(stop_token_ids=[-1]), dict(stop_token_ids=[True]), dict(stop_token_ids=["5"]),
                dict(stop_token_ids=range(20, 37)), dict(stop=" ".join(f"w{i}" for i in range(33))),
                dict(stop_token_ids=5)):
        with pytest.raises(StopError) as e:
            merge_stops(bad.get("stop"), bad.get("stop_token_ids"), TOK, VOCAB)
        assert e.value.status == 1, bad


def test_first_stop_on_hand_written_streams():
    assert first_stop([], [(1,)]) is None
    assert first_stop([1, 2, 3], [(4,)]) is None
    assert first_stop([1, 2, 3], [(1,)]) == (1, 0)
    assert first_stop([1, 2, 3, 2, 3], [(9,), (2, 3), (3,)]) == (3, 1)      # two complete at token 3: the lower index
    assert first_stop([1, 2, 3, 2, 3], [(3, 2, 3)]) == (5, 0)
    assert first_stop([1, 2], [(0, 1, 2)]) is None                          # longer than the stream
    assert first_stop([316, 183] * 4, [(183, 316, 183)]) == (4, 0)
    assert first_stop(list(range(32)), [tuple(range(32))]) == (32, 0)


def _stream_tokens(tokens, seqs, include=False):
    """Feeds the stream token by token the way the device would cut it; what a consumer saw at each step."""
    fs = first_stop(tokens, seqs)
    end = len(tokens) if fs is None else fs[0]
    hb, seen = TokenHoldback(seqs, include), []
    for n in range(1, end + 1):
        seen.append(hb.feed(tokens[:n]))
    final = hb.finish(tokens[:end], 0 if fs is None else len(seqs[fs[1]]))
    return seen, final, end


def test_token_holdback():
    # a stop that is a prefix of another stop: (5, 6) fires before (5, 6, 7) can
    seen, final, end = _stream_tokens([1, 5, 2, 5, 6, 7], [(5, 6, 7), (5, 6)])
    assert end == 5 and final == 3 and seen == [1, 1, 3, 3, 3] and max(seen) <= final
    # no hit: everything is released at the end, a held prefix too
    seen, final, end = _stream_tokens([1, 5, 2, 5], [(5, 6)])
    assert seen == [1, 1, 3, 3] and final == 4 == end
    # include_stop_in_output: nothing is held
    seen, final, end = _stream_tokens([1, 5, 6, 9], [(5, 6)], include=True)
    assert seen == [1, 2, 3] and final == 3 == end
    # randomised: nothing shown is ever removed
    r = np.random.default_rng(0)
    for _ in range(200):
        toks = r.integers(0, 4, 24).tolist()
        seqs = list({tuple(r.integers(0, 4, r.integers(1, 5)).tolist()) for _ in range(3)})
        seen, final, end = _stream_tokens(toks, seqs)
        assert all(a <= b for a, b in zip(seen, seen[1:])) and max(seen) <= final <= end


def _stream_text(deltas, stops, include=False):
    ts, text, shown = TextStop(stops, include), "", []
    for d in deltas:
        text += d
        safe, hit = ts.advance(text, False)
        shown.append(safe)
        if hit is not None:
            return shown, safe, hit
    safe, hit = ts.advance(text, True)
    return shown, safe, hit


def test_text_stop():
    # a stop that is a prefix of another stop
    shown, final, hit = _stream_text(["x", "a", "b", "c"], ["abc", "ab"])
    assert (final, hit) == ("x", "ab") and shown == ["x", "x", "x"]
    # a stop split across two deltas
    shown, final, hit = _stream_text(["row 1 </ta", "ble> tail"], ["</table>"])
    assert (final, hit) == ("row 1 ", "</table>") and shown[0] == "row 1 "
    # a multi-byte character at the boundary: in front of the stop and inside it
    shown, final, hit = _stream_text(["caf", "é", "—", "fin"], ["—fin"])
    assert (final, hit) == ("café", "—fin") and shown == ["caf", "café", "café", "café"]
    # no hit: everything is released at the end
    shown, final, hit = _stream_text(["a <", "/tab"], ["</table>"])
    assert shown == ["a ", "a "] and (final, hit) == ("a </tab", None)
    # include_stop_in_output keeps the stop and nothing behind it
    shown, final, hit = _stream_text(["ab", "cSTOPde"], ["STOP"], include=True)
    assert (final, hit) == ("abcSTOP", "STOP")
    # every way of cutting a text into deltas shows only prefixes of the final text
    text, stops = "one two </table> three", ["</table>", "</tab", "three"]
    for cut in range(1, len(text)):
        for cut2 in range(cut, len(text)):
            shown, final, hit = _stream_text([text[:cut], text[cut:cut2], text[cut2:]], stops)
            assert (final, hit) == ("one two ", "</tab")
            assert all(final.startswith(s) for s in shown)


def test_apply_stops_trims_ids_text_and_names_the_reason():
    dec = lambda ids: TOK.decode(ids)
    ss = merge_stops(["<183>"], [400], TOK, VOCAB)
    # a token-level hit: trimmed by match_len, or kept
    r = apply_stops(dec, [316, 20, 400], ss, 1, 1)
    assert (r.tokens, r.text, r.stop_reason) == ([316, 20], "<316> <20>", 400)
    r = apply_stops(dec, [316, 20, 400], ss, 1, 1, include_stop=True)
    assert (r.tokens, r.stop_reason) == ([316, 20, 400], 400)
    # the text-level backstop: "<183>" is never the stop's own tokenisation in this stream
    r = apply_stops(dec, [316, 183, 316, 183], ss, -1, 0)
    assert (r.tokens, r.text, r.stop_reason) == ([316], "<316> ", "<183>")
    r = apply_stops(dec, [316, 183, 316, 183], ss, -1, 0, include_stop=True)
    assert (r.tokens, r.text, r.stop_reason) == ([316, 183], "<316> <183>", "<183>")
    # no hit; no stops
    r = apply_stops(dec, [316, 20], ss, -1, 0)
    assert (r.tokens, r.stop_reason) == ([316, 20], None)
    assert apply_stops(dec, [316, 183], None).tokens == [316, 183]


# ------------------------------------------------------------------ the server over a stand-in engine
class FakeEngine:
    """Decodes a fixed stream; with stops it does what the engine does (first_stop, then apply_stops)."""
    vocab = VOCAB

    def __init__(self, tokens=(316, 183, 20, 21, 316, 183)):
        self.tokens, self.calls = list(tokens), []

    def decode(self, tokenizer, prompt, images, vision, params, stream=None, stop=None, stop_token_ids=None,
               include_stop_in_output=False, **kw):
        self.calls.append(dict(stop=stop, stop_token_ids=stop_token_ids, include=include_stop_in_output))
        ss = merge_stops(stop, stop_token_ids, tokenizer, self.vocab)
        toks, hit = self.tokens, (-1, 0)
        if ss is not None:
            fs = first_stop(toks, ss.seqs)
            if fs is not None:
                toks, hit = toks[:fs[0]], (fs[1], len(ss.seqs[fs[1]]))
        for k in range(1, len(toks) + 1):
            if stream:
                stream(k, toks[:k])
        r = apply_stops(lambda t: tokenizer.decode(t), toks, ss, hit[0], hit[1], include_stop_in_output)
        return DecodeOutcome(r.text.strip(), 10, len(r.tokens), r.tokens, stop_reason=r.stop_reason)


def _data_url():
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(b, format="PNG")
    return "data:image/png;base64," + base64.b64encode(b.getvalue()).decode()


@pytest.fixture()
def client():
    from starlette.testclient import TestClient
    eng = FakeEngine()
    st = server.ServerState(eng, TOK, "deepseek-ocr", VisionSettings(256, 128, True), DecodeParameters(max_new_tokens=64))
    return TestClient(server.create_app(st)), eng


def _chat(**extra):
    msg = [{"role": "user", "content": [{"type": "text", "text": "OCR"},
                                        {"type": "image_url", "image_url": {"url": _data_url()}}]}]
    return dict(model="deepseek-ocr", messages=msg, **extra)


def test_parse_stops():
    assert server.parse_stops({}, TOK, VOCAB) is None
    assert server.parse_stops({"stop": None, "stop_token_ids": None}, TOK, VOCAB) is None
    assert server.parse_stops({"stop": []}, TOK, VOCAB) is None
    assert server.parse_stops({"stop": "x y"}, TOK, VOCAB) == {"stop": ["x y"], "stop_token_ids": None,
                                                                "include_stop_in_output": False}
    got = server.parse_stops({"stop": ["a", "b", "c", "d"], "stop_token_ids": [5], "include_stop_in_output": True}, TOK, VOCAB)
    assert got == {"stop": ["a", "b", "c", "d"], "stop_token_ids": [5], "include_stop_in_output": True}
    for bad in ({"stop": ["a", "b", "c", "d", "e"]}, {"stop": 5}, {"stop": [5]}, {"stop": {"a": 1}}, {"stop": ""},
                {"stop": [""]}, {"stop_token_ids": "5"}, {"stop_token_ids": [VOCAB]}, {"stop_token_ids": [1.5]},
                {"stop": "a", "include_stop_in_output": "yes"}, {"stop": True}):
        with pytest.raises(server.ApiError) as e:
            server.parse_stops(bad, TOK, VOCAB)
        assert e.value.status == 400, bad


@pytest.mark.parametrize("route,key", [("/v1/chat/completions", "messages"), ("/v1/responses", "input")])
def test_server_stop_fields(client, route, key):
    c, eng = client
    body = _chat()
    if key == "input":
        body["input"] = body.pop("messages")

    def text(j):
        return j["choices"][0]["message"]["content"] if key == "messages" else j["output"][0]["content"][0]["text"]

    def reason(j):
        return (j["choices"][0] if key == "messages" else j).get("stop_reason", "absent")

    plain = c.post(route, json=body).json()
    assert text(plain) == "<316> <183> <20> <21> <316> <183>" and reason(plain) == "absent"
    assert eng.calls[-1] == dict(stop=None, stop_token_ids=None, include=False)
    r = c.post(route, json=dict(body, stop="<20>")).json()                      # a string: the text-level backstop
    assert text(r) == "<316> <183>" and reason(r) == "<20>"
    if key == "messages":
        assert r["choices"][0]["finish_reason"] == "stop"
    r = c.post(route, json=dict(body, stop=["<21>", "zzz"], include_stop_in_output=True)).json()
    assert text(r) == "<316> <183> <20> <21>" and reason(r) == "<21>"
    r = c.post(route, json=dict(body, stop_token_ids=[20])).json()             # a token id: the device's match
    assert text(r) == "<316> <183>" and reason(r) == 20
    r = c.post(route, json=dict(body, stop=["never"], stop_token_ids=[99])).json()
    assert text(r) == text(plain) and reason(r) is None                        # carried stops, none fired: null
    assert reason(c.post(route, json=dict(body, stop=None)).json()) == "absent"
    for bad in (dict(stop=["a", "b", "c", "d", "e"]), dict(stop=7), dict(stop=[7]), dict(stop_token_ids=[VOCAB])):
        n = len(eng.calls)
        resp = c.post(route, json=dict(body, **bad))
        assert resp.status_code == 400 and len(eng.calls) == n, bad


def _sse(text):
    out = []
    for block in text.split("\n\n"):
        if block.startswith("data: "):
            d = block[6:]
            out.append(d if d == "[DONE]" else json.loads(d))
    return out


@pytest.mark.parametrize("extra,want,why", [
    (dict(stop="<20>"), "<316> <183>", "<20>"),
    (dict(stop="<20>", include_stop_in_output=True), "<316> <183> <20>", "<20>"),
    (dict(stop_token_ids=[21]), "<316> <183> <20>", 21),
    (dict(stop="never"), "<316> <183> <20> <21> <316> <183>", None)])
def test_server_stream_never_shows_a_stop(client, extra, want, why):
    c, _ = client
    ev = _sse(c.post("/v1/chat/completions", json=_chat(stream=True, **extra)).text)
    deltas = [e["choices"][0]["delta"].get("content", "") for e in ev[1:-2]]
    assert "".join(deltas).strip() == want
    assert ev[-2]["choices"][0]["finish_reason"] == "stop" and ev[-2]["choices"][0]["stop_reason"] == why
    if not extra.get("include_stop_in_output") and why == "<20>":
        assert all("2" not in d for d in deltas)   # not a character of the stop, in any delta
    plain = _sse(c.post("/v1/chat/completions", json=_chat(stream=True)).text)
    assert "stop_reason" not in plain[-2]["choices"][0]


def test_cli_stop_arguments():
    from dsocr import cli
    from dsocr._lib import DsocrError
    p = cli.build_parser()
    base = ["--model-config", "x.json", "--prompt", "<image>", "--image", "a.png"]
    assert cli.stop_arguments(p.parse_args(base)) == {}
    a = p.parse_args(base + ["--stop", "</table>", "--stop", "<|ref|>", "--stop-token-ids", "5, 7", "--include-stop"])
    assert cli.stop_arguments(a) == {"stop": ["</table>", "<|ref|>"], "stop_token_ids": [5, 7],
                                     "include_stop_in_output": True}
    for bad in (["--stop", ""], ["--stop-token-ids", "5,x"], ["--include-stop"], ["--stop", "a", "--slots", "2"]):
        with pytest.raises(DsocrError) as e:
            cli.stop_arguments(p.parse_args(base + bad))
        assert e.value.status == 1, bad


# ------------------------------------------------------------------ the scheduler over a scripted session
class NumTok:
    """Ids are their own words: ``encode("13 14")`` is ``[13, 14]`` and ``decode`` its inverse."""
    vocab_size = VOCAB

    def token_to_id(self, tok):
        return VOCAB - 1 if tok == "<image>" else None

    def encode(self, text, add_special_tokens=False):
        from dsocr.synth import _Enc
        return _Enc([int(w) for w in text.split()])

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(str(int(i)) for i in ids)


def _stop_session_engine(scripts):
    from test_logprobs_host import FakeEngine as LpEngine, FakeSession

    class StopSession(FakeSession):
        """The scripted session with the device's part of a stop set: the stream ends where first_stop says."""

        def __init__(self, *a):
            super().__init__(*a)
            self.recs = {}

        def admit(self, ids, mask=None, page=None, image_rows=None, stops=None, include_stop_in_output=False, **kw):
            slot = super().admit(ids, mask, page, image_rows, **kw)
            if stops is not None:
                s = self.active[slot]
                fs = first_stop(s["stream"], stops.seqs)
                s["stream"] = s["stream"] if fs is None else s["stream"][:fs[0]]
                s["stops"] = (stops, include_stop_in_output, fs)
            return slot

        def retire_stopped(self, slot, decode):
            stops, include, fs = self.active[slot]["stops"]
            ids, moved = self.retire(slot)
            hit = (-1, 0) if fs is None or len(ids) < fs[0] else (fs[1], len(stops.seqs[fs[1]]))
            return apply_stops(decode, ids, stops, hit[0], hit[1], include), moved

    class Engine(LpEngine):
        vocab = VOCAB

        def open_session(self, slots, max_context, params, per_request=False, logprobs=False, stops=False):
            assert stops
            self.session = StopSession(self, slots, max_context, params, logprobs)
            return self.session

    return Engine(scripts)


def test_scheduler_streams_every_token_with_its_own_entry_under_a_holdback():
    """A multi-token stop together with logprobs: ids held back as a possible stop are released later, in a jump,
    and each one still arrives in a call of its own with the entry of that token, not of the newest one."""
    from dsocr.scheduler import BatchScheduler
    from test_logprobs_host import _lp, _prepare, _top
    eng = _stop_session_engine({1: [10, 11, 12, 13, 14, 15, 16, 17, 18]})
    seen = []
    with BatchScheduler(eng, NumTok(), 2, 128, DecodeParameters(max_new_tokens=64), VisionSettings(256, 128, True),
                        prepare=_prepare, logprobs=True, stops=True) as s:
        out = s.submit("<image>doc:1", on_token=lambda n, t, e: seen.append((n, list(t), e)), logprobs=2,
                       stop=["13 14 99", "15 16"]).result(10)
    # 13 and 14 were held (a prefix of the first stop) until 15 showed that stop could not complete; 15 was held as
    # a prefix of the second stop, which then fired: trimmed, never shown
    assert out.generated_tokens == [10, 11, 12, 13, 14] and out.stop_reason == "15 16"
    assert out.token_logprobs == [_lp(t) for t in out.generated_tokens]
    assert [(n, t) for n, t, _ in seen] == [(j, [10, 11, 12, 13, 14][:j]) for j in range(1, 6)]
    assert all(e == (_lp(t[-1]), _top(t[-1], 2)) for _, t, e in seen)
    # without a hit the held tail is shown at the retirement, entries included
    eng = _stop_session_engine({1: [10, 11, 13, 14]})
    seen = []
    with BatchScheduler(eng, NumTok(), 2, 128, DecodeParameters(max_new_tokens=64), VisionSettings(256, 128, True),
                        prepare=_prepare, logprobs=True, stops=True) as s:
        out = s.submit("<image>doc:1", on_token=lambda n, t, e: seen.append((n, t[-1], e)), logprobs=1,
                       stop="13 14 99").result(10)
    assert out.generated_tokens == [10, 11, 13, 14] and out.stop_reason is None
    assert [(n, t) for n, t, _ in seen] == [(1, 10), (2, 11), (3, 13), (4, 14)]
    assert all(e == (_lp(t), _top(t, 1)) for _, t, e in seen)


def test_session_checks_stops_before_it_stages_a_constraint(monkeypatch):
    """A bad stop set must not leave the admission's logit bias staged for the next request: the stop set is merged
    and checked first, and nothing reaches the library when it fails."""
    from dsocr import engine as E
    from dsocr._lib import DsocrError

    calls = []

    class Lib:
        def dsocr_session_stage_logit_bias(self, h, rec):
            calls.append("bias")
            return 0

        def dsocr_session_stage_stop(self, h, rec):
            calls.append("stop")
            return 0

    monkeypatch.setattr(E, "lib", lambda: Lib())
    sess = E.Session.__new__(E.Session)
    sess._e = type("Eng", (), {"vocab": VOCAB, "_h": None})()
    sess.has_logit_bias, sess.has_stops = True, False

    def admit_prologue(**kw):   # the three lines every admission form starts with
        checked = sess._check_stops(kw.get("stop"), kw.get("stop_token_ids"), False, TOK, None)
        sess._stage_constraint({5: 1.0}, None, None)
        sess._stage_stops(checked)

    for bad in (dict(stop_token_ids=[5]), dict(stop_token_ids=[VOCAB]), dict(stop="")):   # no flag / bad id / empty
        with pytest.raises(DsocrError):
            admit_prologue(**bad)
        sess.has_stops = True
    assert calls == []
    admit_prologue(stop_token_ids=[5])
    assert calls == ["bias", "stop"]
