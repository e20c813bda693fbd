"""Stop sequences through the HTTP server and the CLI on the GPU (tiny config, the in-process server of
tests/test_cli_server.py): a string stop and a token-id stop, non-streaming and SSE, decoded alone (dsocr_generate_stop
behind the lock) and in the decode session (``--slots --stops``)."""
import base64
import io
import json
import os

import numpy as np
import pytest

from dsocr import DecodeParameters, ModelLoadArgs, VisionSettings, cli, load_model, server
from dsocr.synth import SyntheticTokenizer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, "deepseek-ocr.rs_amd", "dsocr", "configs", "tiny.json")
PROMPT = "<image>\nConvert the document to markdown."
TOK = SyntheticTokenizer(512)
MAX_NEW = 16


def _png(h=256, w=256, seed=5):
    from PIL import Image
    arr = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format="PNG")
    return b.getvalue()


def _sse(text):
    out = []
    for block in text.split("\n\n"):
        if block.startswith("data: "):
            d = block[6:]
            out.append(d if d == "[DONE]" else json.loads(d))
    return out


@pytest.fixture(scope="module")
def setup(gpu):
    from starlette.testclient import TestClient
    eng = load_model(ModelLoadArgs(config_path=TINY, synthetic_seed=7, dtype="f16"))
    png = _png()
    msg = [{"role": "user", "content": [{"type": "text", "text": "Convert the document to markdown."},
                                        {"type": "image_url", "image_url": {"url": "data:image/png;base64," +
                                                                            base64.b64encode(png).decode()}}]}]
    st = server.ServerState(eng, TOK, "deepseek-ocr", VisionSettings(256, 128, True), DecodeParameters(max_new_tokens=MAX_NEW))
    c = TestClient(server.create_app(st))
    plain = c.post("/v1/chat/completions", json={"model": "deepseek-ocr", "messages": msg}).json()
    text = plain["choices"][0]["message"]["content"]
    ids = [int(t[1:-1]) for t in text.split()]
    assert len(ids) == MAX_NEW and "stop_reason" not in plain["choices"][0]
    # the stop: the first id that is new at position >= 2 (its first occurrence is where the text is cut)
    k = next(i for i in range(2, MAX_NEW) if ids[i] not in ids[:i])
    yield dict(eng=eng, st=st, c=c, msg=msg, ids=ids, k=k, png=png)
    if st.scheduler is not None:
        st.scheduler.close()
    eng.close()


@pytest.mark.parametrize("slots", [0, 2], ids=["alone", "slots-stops"])
def test_server_stops(setup, slots):
    eng, st, c, msg, ids, k = (setup[x] for x in ("eng", "st", "c", "msg", "ids", "k"))
    stop, want, kept = f"<{ids[k]}>", TOK.decode(ids[:k]), TOK.decode(ids[:k + 1])
    if slots:
        st.scheduler = server.make_scheduler(st, slots, 1024, stops=True)
    try:
        base = {"model": "deepseek-ocr", "messages": msg}
        before = eng.stop_launches()
        # a string stop (here never its own tokenisation: the text-level backstop cuts in front of it)
        r = c.post("/v1/chat/completions", json=dict(base, stop=stop)).json()
        assert r["choices"][0]["message"]["content"] == want and want.endswith(f"<{ids[k - 1]}>")
        assert r["choices"][0]["stop_reason"] == stop and r["choices"][0]["finish_reason"] == "stop"
        assert r["usage"]["completion_tokens"] == k
        assert eng.stop_launches() > before         # the request carried a stop set onto the device
        r = c.post("/v1/responses", json={"model": "deepseek-ocr", "input": msg, "stop": [stop]}).json()
        assert r["output"][0]["content"][0]["text"] == want and r["stop_reason"] == stop
        # SSE: the deltas concatenated equal the non-streaming text, nothing of the stop in any of them
        ev = _sse(c.post("/v1/chat/completions", json=dict(base, stop=stop, stream=True)).text)
        deltas = [e["choices"][0]["delta"].get("content", "") for e in ev[1:-2]]
        assert "".join(deltas).strip() == want
        assert all(stop not in d for d in deltas) and stop not in "".join(deltas)
        assert ev[-2]["choices"][0]["stop_reason"] == stop
        # include_stop_in_output keeps the stop in the text
        r = c.post("/v1/chat/completions", json=dict(base, stop=stop, include_stop_in_output=True)).json()
        assert r["choices"][0]["message"]["content"] == kept
        ev = _sse(c.post("/v1/chat/completions", json=dict(base, stop=stop, include_stop_in_output=True, stream=True)).text)
        assert "".join(e["choices"][0]["delta"].get("content", "") for e in ev[1:-2]).strip() == kept
        # a token id: matched on the device, in the step that emits it
        r = c.post("/v1/chat/completions", json=dict(base, stop_token_ids=[ids[k]])).json()
        assert r["choices"][0]["message"]["content"] == want and r["choices"][0]["stop_reason"] == ids[k]
        ev = _sse(c.post("/v1/chat/completions", json=dict(base, stop_token_ids=[ids[k]], stream=True)).text)
        assert "".join(e["choices"][0]["delta"].get("content", "") for e in ev[1:-2]).strip() == want
        # a stop that never fires: the whole text, stop_reason null; no stops: no stop_reason
        r = c.post("/v1/chat/completions", json=dict(base, stop="never")).json()
        assert r["choices"][0]["message"]["content"] == TOK.decode(ids) and r["choices"][0]["stop_reason"] is None
        assert "stop_reason" not in c.post("/v1/chat/completions", json=base).json()["choices"][0]
        assert c.post("/v1/chat/completions", json=dict(base, stop=["a"] * 5)).status_code == 400
    finally:
        if st.scheduler is not None:
            st.scheduler.close()
            st.scheduler = None


def test_cli_stop(setup, tmp_path):
    ids, k = setup["ids"], setup["k"]
    p = tmp_path / "page.png"
    p.write_bytes(setup["png"])
    base = ["--model-config", TINY, "--synthetic-seed", "7", "--prompt", PROMPT, "--image", str(p), "--base-size", "256",
            "--image-size", "128", "--max-new-tokens", str(MAX_NEW), "-q"]
    for extra, want in ((["--stop", f"<{ids[k]}>"], TOK.decode(ids[:k])),
                        (["--stop-token-ids", str(ids[k])], TOK.decode(ids[:k])),
                        (["--stop", f"<{ids[k]}>", "--include-stop"], TOK.decode(ids[:k + 1]))):
        out = io.StringIO()
        assert cli.run_inference(cli.build_parser().parse_args(base + extra), out, io.StringIO()) == 0
        assert out.getvalue() == want + "\n"


class RoundTripTokenizer(SyntheticTokenizer):
    """The synthetic tokenizer with ``encode`` the inverse of ``decode`` on its own output: ``"<316>"`` is id 316, so
    a stop string taken from the text has a canonical encoding that does occur in the stream."""

    def encode(self, text, add_special_tokens=False):
        import re
        ids = []
        for piece in re.findall(r"<\d+>|\w+|[^\w\s]|\n", text):
            ids += [int(piece[1:-1])] if re.fullmatch(r"<\d+>", piece) else super().encode(piece).ids
        enc = super().encode("")
        enc.ids = ids
        return enc


@pytest.mark.parametrize("slots", [0, 2], ids=["alone", "slots-stops"])
def test_string_stop_matched_on_the_device(setup, slots):
    """merge_stops -> the device's hit -> ``stop_reason`` as the string: the two-id stop completes at token k + 1,
    the engine stops there (a streamed request decoding alone polls after every step: k decode steps, not 15), and
    the deltas arrive live, none of them with a token of the stop."""
    from starlette.testclient import TestClient
    eng, ids, k, msg = (setup[x] for x in ("eng", "ids", "k", "msg"))
    tok = RoundTripTokenizer(512)
    assert tok.encode(f"<{ids[k - 1]}> <{ids[k]}>").ids == [ids[k - 1], ids[k]]
    st = server.ServerState(eng, tok, "deepseek-ocr", VisionSettings(256, 128, True), DecodeParameters(max_new_tokens=MAX_NEW))
    if slots:
        st.scheduler = server.make_scheduler(st, slots, 1024, stops=True)
    try:
        c = TestClient(server.create_app(st))
        base = {"model": "deepseek-ocr", "messages": msg}
        assert c.post("/v1/chat/completions", json=base).json()["choices"][0]["message"]["content"] == TOK.decode(ids)
        stop, want = f"<{ids[k - 1]}> <{ids[k]}>", TOK.decode(ids[:k - 1])
        from dsocr.stops import first_stop
        assert first_stop(ids, [(ids[k - 1], ids[k])]) == (k + 1, 0)
        r = c.post("/v1/chat/completions", json=dict(base, stop=stop)).json()
        assert r["choices"][0]["message"]["content"] == want and r["choices"][0]["stop_reason"] == stop
        assert r["usage"]["completion_tokens"] == k - 1
        ev = _sse(c.post("/v1/chat/completions", json=dict(base, stop=stop, stream=True)).text)
        deltas = [e["choices"][0]["delta"].get("content", "") for e in ev[1:-2]]
        assert "".join(deltas).strip() == want and ev[-2]["choices"][0]["stop_reason"] == stop
        assert all(f"<{ids[k]}>" not in d for d in deltas)
        if not slots:
            assert eng.last_timings()["decode_steps"] == k   # stopped by the device at token k + 1
            # live: a delta per token shown (fewer only where a tail was held back for a step as a possible stop)
            assert min(2, k - 1) <= len([d for d in deltas if d]) <= k - 1
        r = c.post("/v1/chat/completions", json=dict(base, stop=stop, include_stop_in_output=True)).json()
        assert r["choices"][0]["message"]["content"] == TOK.decode(ids[:k + 1])
    finally:
        if st.scheduler is not None:
            st.scheduler.close()
            st.scheduler = None
