"""DeepSeek-OCR-2 on the GPU: the hybrid-mask GQA kernel against the f64 formula, the encoder at the reference's
width, and the tiny OCR2 engine (vision rows, greedy ids, logits, batching, variant mismatch, CLI) against
tests/ocr2_ref.py."""
import io
import json
import os

import numpy as np
import pytest

import ocr2_ref
from _dev import Dev as DevBuf
from dsocr import DecodeParameters, DsocrError, ModelLoadArgs, Page, VisionSettings, build_prompt_tokens, cli, load_model
from dsocr._lib import check, lib
from dsocr.synth import SyntheticTokenizer
from oracle.weights import Weights

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "deepseek-ocr.rs_amd", "dsocr", "configs")
OCR2_TINY = os.path.join(CFG, "ocr2-tiny.json")
OCR2_ENC = os.path.join(CFG, "ocr2-enc.json")
TINY = os.path.join(CFG, "tiny.json")
VS = VisionSettings(1024, 768, True)   # the registry defaults of deepseek-ocr-2 (config.rs:104-110)
SEED = 7
STEPS = 16
# (seed, h, w): a page that yields a 2x1 tile grid and one that yields no tiles.  At every compared step the CPU
# reference's top-2 logit gap exceeds 2e-2 for these seeds (checked on the CPU, asserted below).
PAGES = {"grid2x1": (16, 500, 930), "no_tiles": (4, 400, 600)}


# ---------------------------------------------------------------- kernel
def _prefix_ref(q, k, v, P, scale):
    """f64 attention of one head under the hybrid mask: row i sees key j iff j < P or (i >= P and j <= i)."""
    L = q.shape[0]
    s = (q.astype(np.float64) @ k.astype(np.float64).T) * scale
    i, j = np.arange(L)[:, None], np.arange(L)[None, :]
    s = np.where((j < P) | ((i >= P) & (j <= i)), s, -np.inf)
    s -= s.max(-1, keepdims=True)
    p = np.exp(s)
    return (p / p.sum(-1, keepdims=True)) @ v.astype(np.float64)


def _run_prefix(n_seq, P, L, heads, kv_heads, hd, q, k, v, scale):
    dq, dk, dv = DevBuf(q), DevBuf(k), DevBuf(v)
    do = DevBuf(nbytes=q.nbytes, dtype=np.float32, shape=q.shape)
    check(lib().dsocr_k_attention_prefix(n_seq, L, P, heads, kv_heads, hd, scale, dq.ptr, dk.ptr, dv.ptr, do.ptr))
    return do.get()


SHAPES = [(1, 144, 288, 14, 2, 64), (2, 256, 512, 14, 2, 64), (3, 5, 37, 4, 2, 32), (1, 31, 64, 4, 2, 64),
          (1, 32, 64, 4, 2, 64), (1, 33, 64, 4, 2, 64), (1, 0, 33, 2, 1, 64), (1, 40, 40, 7, 1, 64), (2, 33, 34, 4, 4, 64)]


@pytest.mark.parametrize("n_seq,P,L,heads,kv_heads,hd", SHAPES)
def test_attention_prefix_matches_f64(gpu, n_seq, P, L, heads, kv_heads, hd):
    rng = np.random.default_rng(P * 1000 + L)
    q = rng.standard_normal((n_seq * L, heads * hd)).astype(np.float32)
    k, v = (rng.standard_normal((n_seq * L, kv_heads * hd)).astype(np.float32) for _ in range(2))
    scale = float(1.0 / np.sqrt(hd))
    got = _run_prefix(n_seq, P, L, heads, kv_heads, hd, q, k, v, scale)
    worst = 0.0
    for s in range(n_seq):
        for h in range(heads):
            g = h // (heads // kv_heads)
            sl, hl, kl = slice(s * L, (s + 1) * L), slice(h * hd, (h + 1) * hd), slice(g * hd, (g + 1) * hd)
            ref = _prefix_ref(q[sl, hl], k[sl, kl], v[sl, kl], P, scale)
            worst = max(worst, float(np.max(np.abs(got[sl, hl] - ref))))
    print("attention_prefix max abs err", (n_seq, P, L, heads, kv_heads, hd), worst)
    assert worst < 2e-5, worst


def test_attention_prefix_masked_keys_contribute_nothing(gpu):
    """NaN in the K/V of keys a row cannot see must not reach that row: the image rows never read the query keys
    (skipped tiles, zero-staged tail of the straddling tile, masked elements)."""
    n_seq, P, L, heads, kv_heads, hd = 2, 40, 100, 4, 2, 64
    rng = np.random.default_rng(9)
    q = rng.standard_normal((n_seq * L, heads * hd)).astype(np.float32)
    k, v = (rng.standard_normal((n_seq * L, kv_heads * hd)).astype(np.float32) for _ in range(2))
    scale = float(1.0 / np.sqrt(hd))
    clean = _run_prefix(n_seq, P, L, heads, kv_heads, hd, q, k, v, scale)
    kp, vp = k.copy(), v.copy()
    for s in range(n_seq):
        kp[s * L + P:(s + 1) * L] = np.nan
        vp[s * L + P:(s + 1) * L] = np.nan
    got = _run_prefix(n_seq, P, L, heads, kv_heads, hd, q, kp, vp, scale)
    for s in range(n_seq):
        rows = slice(s * L, s * L + P)
        assert np.all(np.isfinite(got[rows]))
        assert np.array_equal(got[rows], clean[rows])
        for h in range(heads):
            g = h // (heads // kv_heads)
            hl, kl = slice(h * hd, (h + 1) * hd), slice(g * hd, (g + 1) * hd)
            ref = _prefix_ref(q[s * L:(s + 1) * L, hl], k[s * L:(s + 1) * L, kl], v[s * L:(s + 1) * L, kl], P, scale)
            assert np.max(np.abs(got[rows, hl] - ref[:P])) < 2e-5


@pytest.mark.parametrize("args", [(1, 64, 32, 4, 2, 48), (1, 64, 32, 4, 3, 64), (1, 64, 65, 4, 2, 64), (1, 64, -1, 4, 2, 64),
                                  (0, 64, 32, 4, 2, 64), (1, 64, 32, 4, 0, 64)])
def test_attention_prefix_rejects_shapes_outside_the_contract(gpu, args):
    n_seq, L, P, heads, kv_heads, hd = args
    buf = DevBuf(np.zeros((64, 256), np.float32))
    st = lib().dsocr_k_attention_prefix(n_seq, L, P, heads, kv_heads, hd, 0.125, buf.ptr, buf.ptr, buf.ptr, buf.ptr)
    assert st == 1  # DSOCR_EINVAL


# ---------------------------------------------------------------- encoder at the reference's width
def _img(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_encoder_full_width_non_crop_768(gpu):
    """ocr2-enc.json: encoder 896 wide, 14 / 2 heads, intermediate 4864 (2 layers) on one non-crop 768 px page."""
    eng = load_model(ModelLoadArgs(config_path=OCR2_ENC, synthetic_seed=SEED, dtype="f16"))
    try:
        assert eng.variant == 1 and eng.kind() == "deepseek"
        vs = VisionSettings(1024, 768, False)
        img = _img(11, 300, 420)
        page = Page(img, vs, variant=1)
        assert page.n_image_tokens == 145
        got = eng.image_embeddings([page])[0]
    finally:
        eng.close()
    orc = ocr2_ref.Ocr2Model(json.load(open(OCR2_ENC)), Weights(seed=SEED, dtype="f16"))
    ref, _ = orc.image_embeddings(img, 1024, 768, False)
    assert got.shape == ref.shape == (145, 128)
    err = float(np.max(np.abs(got - ref)))
    print("encoder full width: max abs err", err, "max|ref|", float(np.max(np.abs(ref))))
    assert err < 1e-3 * max(1.0, np.max(np.abs(ref)))
    assert np.array_equal(got[-1], orc.vision.separator())  # bit for bit


# ---------------------------------------------------------------- tiny engine
@pytest.fixture(scope="module")
def tiny2(gpu):
    eng = load_model(ModelLoadArgs(config_path=OCR2_TINY, synthetic_seed=SEED, dtype="f16"))
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def tiny2_ref():
    """The CPU reference of both pages, computed once: rows, prompt, greedy ids and logits."""
    orc = ocr2_ref.Ocr2Model(json.load(open(OCR2_TINY)), Weights(seed=SEED, dtype="f16"))
    tok = SyntheticTokenizer(512)
    out = {}
    for name, (seed, h, w) in PAGES.items():
        img = _img(seed, h, w)
        emb, crop = orc.image_embeddings(img, VS.base_size, VS.image_size, VS.crop_mode)
        ids, mask = build_prompt_tokens(tok, "<image>\nConvert the document to markdown.", [emb.shape[0]])
        gen, logits = orc.generate(ids, mask, emb, STEPS, eos_token_id=1, no_repeat_ngram_size=20, record_logits=True)
        out[name] = dict(img=img, emb=emb, crop=crop, ids=ids, mask=mask, gen=gen, logits=np.stack(logits))
    return out


@pytest.mark.parametrize("name", list(PAGES))
def test_tiny_ocr2_rows_ids_and_logits(tiny2, tiny2_ref, name):
    r = tiny2_ref[name]
    page = Page(r["img"], VS, variant=1)
    assert page.crop_shape == r["crop"] == ((2, 1) if name == "grid2x1" else (1, 1))
    assert page.n_image_tokens == r["emb"].shape[0] == ocr2_ref.placeholder_count(1024, 768, True, r["crop"])
    got = tiny2.image_embeddings([page])[0]
    assert got.shape == r["emb"].shape
    err = float(np.max(np.abs(got - r["emb"])))
    print(name, "rows max abs err", err)
    assert err < 1e-3 * max(1.0, np.max(np.abs(r["emb"])))
    assert np.array_equal(got[-1], r["emb"][-1])
    # the comparison is only meaningful away from near-ties of the reference
    assert len(r["gen"]) == STEPS
    top2 = np.sort(r["logits"], -1)[:, -2:]
    gap = float(np.min(top2[:, 1] - top2[:, 0]))
    print(name, "reference min top-2 logit gap", gap)
    assert gap > 2e-2, gap
    params = DecodeParameters(max_new_tokens=STEPS)
    ids, logits = tiny2.generate_trace([(r["ids"], r["mask"], page, None)], params)
    assert ids[0] == r["gen"]
    lerr = float(np.max(np.abs(logits[0, :STEPS] - r["logits"])))
    print(name, "logits max abs err", lerr)
    assert lerr < 2e-3, lerr
    # a device-prepared page (taking the variant from the engine) gives the same ids
    dpage = Page(r["img"], VS, tiny2)
    assert dpage.variant == 1 and dpage.n_image_tokens == page.n_image_tokens
    assert tiny2.generate(r["ids"], r["mask"], dpage, None, params) == r["gen"]


def test_tiny_ocr2_batch_equals_single(tiny2, tiny2_ref):
    params = DecodeParameters(max_new_tokens=STEPS)
    reqs = []
    for name in PAGES:
        r = tiny2_ref[name]
        reqs.append((r["ids"], r["mask"], Page(r["img"], VS, variant=1), None))
    singles = [tiny2.generate(*rq, params) for rq in reqs]
    assert tiny2.generate_batch(reqs, params) == singles
    assert singles == [tiny2_ref[name]["gen"] for name in PAGES]
    t = tiny2.last_timings()
    assert t["vision_flops"] > 0 and t["vision_compute_ms"] > 0


def test_wrong_variant_page_is_einval(tiny2, tiny2_ref):
    r = tiny2_ref["no_tiles"]
    p1 = Page(r["img"], VS, variant=0)   # an OCR1 page: newline slots, other count
    assert p1.n_image_tokens != r["emb"].shape[0]
    with pytest.raises(DsocrError) as e:
        tiny2.image_embeddings([p1])
    assert e.value.status == 1
    ids, mask = build_prompt_tokens(SyntheticTokenizer(512), "<image>\nx", [p1.n_image_tokens])
    with pytest.raises(DsocrError) as e:
        tiny2.generate(ids, mask, p1, None, DecodeParameters(max_new_tokens=2))
    assert e.value.status == 1
    # and the reverse: an OCR2 page on an OCR1 engine
    eng1 = load_model(ModelLoadArgs(config_path=TINY, synthetic_seed=SEED, dtype="f16"))
    try:
        assert eng1.variant == 0
        with pytest.raises(DsocrError) as e:
            eng1.image_embeddings([Page(r["img"], VS, variant=1)])
        assert e.value.status == 1
    finally:
        eng1.close()


def test_snapshot_with_ocr2_config_is_einval(gpu, tmp_path):
    snap = tmp_path / "none.dsq"
    snap.write_bytes(b"")
    with pytest.raises(DsocrError) as e:
        load_model(ModelLoadArgs(config_path=OCR2_TINY, synthetic_seed=SEED, dtype="f16", snapshot_path=str(snap)))
    assert e.value.status == 1 and "DeepSeek-OCR-2" in e.value.message


def test_cli_model_deepseek_ocr_2(gpu, tiny2_ref, tmp_path):
    """`--model deepseek-ocr-2` picks the OCR2 vision defaults (base 1024 / image 768 / crop on); with the tiny
    config it produces the ids of the direct call."""
    from PIL import Image
    r = tiny2_ref["grid2x1"]
    path = tmp_path / "page.png"
    Image.fromarray(r["img"]).save(path)
    args = cli.build_parser().parse_args(["--model", "deepseek-ocr-2", "--model-config", OCR2_TINY,
                                          "--synthetic-seed", str(SEED), "--prompt",
                                          "<image>\nConvert the document to markdown.", "--image", str(path),
                                          "--max-new-tokens", str(STEPS), "--quiet"])
    assert cli.vision_settings(args) == VS
    out, err = io.StringIO(), io.StringIO()
    assert cli.run_inference(args, out, err) == 0
    assert out.getvalue() == SyntheticTokenizer(512).decode(r["gen"]) + "\n"
