"""DeepSeek-OCR-2 host-side checks (no GPU): config resolution, tile grids and <image> slot counts through the C
ABI against tests/ocr2_ref.py, the new exports, and an independent pin of the reference helper's Qwen2 encoder
against transformers' DeepseekOcr2VisionModel."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import ocr2_ref
from dsocr._lib import EXPORTS, VisionSettingsC, lib
from oracle.weights import Weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "deepseek-ocr.rs_amd", "dsocr", "configs")
NEW_SYMBOLS = ["dsocr_config_variant", "dsocr_engine_variant", "dsocr_prepare_page_variant",
               "dsocr_prepare_page_device_variant", "dsocr_k_attention_prefix"]


def _resolve(path):
    var, sam, enc = C.c_int(-1), (C.c_uint32 * 2)(), (C.c_uint32 * 5)()
    st = lib().dsocr_config_variant(str(path).encode(), C.byref(var), sam, enc)
    return st, var.value, list(sam), list(enc)


def _write(tmp_path, name, cfg):
    p = tmp_path / name
    p.write_text(json.dumps(cfg))
    return p


# ---------------------------------------------------------------- config resolution
def test_bundled_ocr2_configs_resolve():
    """model/mod.rs:2691-2710, sam.rs:60-90, qwen2.rs:12-22: fails on the parent, where the symbol is missing and an
    OCR2 config is EINVAL (`clip-l-14-224 vision backbone missing from config`)."""
    assert _resolve(os.path.join(CFG, "deepseek-ocr-2.json")) == (0, 1, [512, 896], [896, 24, 14, 2, 4864])
    assert _resolve(os.path.join(CFG, "ocr2-tiny.json")) == (0, 1, [32, 128], [128, 2, 4, 2, 192])
    assert _resolve(os.path.join(CFG, "ocr2-enc.json")) == (0, 1, [32, 896], [896, 2, 14, 2, 4864])
    for name in ("deepseek-ocr-2.json", "ocr2-tiny.json", "ocr2-enc.json"):
        cfg = json.load(open(os.path.join(CFG, name)))
        assert ocr2_ref.detect_variant(cfg) == 1
        p = ocr2_ref.enc_params(cfg)
        assert _resolve(os.path.join(CFG, name))[3] == [p["dim"], p["layers"], p["heads"], p["kv_heads"], p["inter"]]


def test_both_detection_rules_and_the_sam_channel_rule(tmp_path):
    base = json.load(open(os.path.join(CFG, "tiny.json")))
    sam = base["vision_config"]["width"]["sam_vit_b"]          # downsample_channels [32, 64]
    # rule 1: model_name alone (any case), no qwen2 entry and no CLIP entry: the last SAM channel becomes 896
    c1 = dict(base, vision_config={"image_size": 256, "model_name": "DeepEncoderV2", "width": {"sam_vit_b": sam}},
              projector_config={"input_dim": 896, "n_embed": 128, "projector_type": "linear"})
    assert _resolve(_write(tmp_path, "c1.json", c1)) == (0, 1, [32, 896], [896, 24, 14, 2, 4864])
    assert ocr2_ref.detect_variant(c1) == 1
    # rule 2: a qwen2-0-5b entry alone; `width` and `dim` both name the encoder width, which SAM's last stage takes
    for key in ("width", "dim"):
        c2 = dict(base, vision_config={"image_size": 256, "width": {"sam_vit_b": sam, "qwen2-0-5b": {key: 128, "heads": 4}}},
                  projector_config={"input_dim": 128, "n_embed": 128, "projector_type": "linear"})
        assert _resolve(_write(tmp_path, "c2.json", c2)) == (0, 1, [32, 128], [128, 24, 4, 2, 4864])
        assert ocr2_ref.detect_variant(c2) == 1
        assert ocr2_ref.sam_out_channels(c2, sam["downsample_channels"]) == [32, 128]
    # a matching last channel is left alone
    sam2 = dict(sam, downsample_channels=[48, 896])
    c3 = dict(c1, vision_config={"model_name": "deepencoderv2", "width": {"sam_vit_b": sam2}})
    assert _resolve(_write(tmp_path, "c3.json", c3))[2] == [48, 896]
    # the projector must take the encoder width; the encoder's head dim must be one the kernel serves
    bad = dict(c1, projector_config={"input_dim": 2048, "n_embed": 128, "projector_type": "linear"})
    assert _resolve(_write(tmp_path, "bad.json", bad))[0] == 1
    bad2 = dict(base, vision_config={"width": {"sam_vit_b": sam, "qwen2-0-5b": {"dim": 96, "heads": 2}}},
                projector_config={"input_dim": 96, "n_embed": 128, "projector_type": "linear"})
    assert _resolve(_write(tmp_path, "bad2.json", bad2))[0] == 1


def test_ocr1_configs_resolve_unchanged(tmp_path):
    for name, ch in (("deepseek-ocr.json", [512, 1024]), ("tiny.json", [32, 64]), ("tiny256.json", None)):
        st, var, sam, enc = _resolve(os.path.join(CFG, name))
        cfg = json.load(open(os.path.join(CFG, name)))
        assert (st, var, enc) == (0, 0, [0] * 5) and ocr2_ref.detect_variant(cfg) == 0
        assert sam == (ch or cfg["vision_config"]["width"]["sam_vit_b"]["downsample_channels"])
    # an OCR1 config still needs its CLIP entry
    c = json.load(open(os.path.join(CFG, "tiny.json")))
    del c["vision_config"]["width"]["clip-l-14-224"]
    assert _resolve(_write(tmp_path, "noclip.json", c))[0] == 1
    assert b"clip-l-14-224" in lib().dsocr_last_error()


# ---------------------------------------------------------------- pages: tile grid and slot counts
def _page(w, h, base, image, crop, variant):
    """(status, crop grid, tiles, slots) of dsocr_prepare_page_variant on a gray page."""
    rgb = np.full((h, w, 3), 128, np.uint8)
    vs = VisionSettingsC(base, image, 1 if crop else 0)
    hnd = C.c_void_p()
    st = lib().dsocr_prepare_page_variant(rgb.ctypes.data_as(C.c_void_p), w, h, C.byref(vs), variant, C.byref(hnd))
    if st != 0:
        return st, None, None, None
    cw, ch, nt, ntok = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_size_t()
    assert lib().dsocr_page_info(hnd, C.byref(cw), C.byref(ch), C.byref(nt), C.byref(ntok)) == 0
    lib().dsocr_page_free(hnd)
    return 0, (cw.value, ch.value), nt.value, ntok.value


# pages (w, h) at the registry defaults (base 1024, tile 768, crop on): no tiles, 2x1, 3x2 and 1x6 grids
@pytest.mark.parametrize("wh,grid", [((100, 90), (1, 1)), ((1500, 800), (2, 1)), ((1500, 1000), (3, 2)),
                                     ((800, 4800), (1, 6))])
def test_ocr2_tile_grid_and_slots(wh, grid):
    st, crop, tiles, slots = _page(wh[0], wh[1], 1024, 768, True, 1)
    assert st == 0
    assert crop == grid == ocr2_ref.tile_grid(wh[0], wh[1], 768, 6)
    assert tiles == (0 if grid == (1, 1) else grid[0] * grid[1])
    assert slots == ocr2_ref.placeholder_count(1024, 768, True, grid)
    # flat layout (model/mod.rs:2630-2680): 144 per tile, 256 for the global view, one separator
    assert slots == 144 * tiles + 256 + 1


def test_max_num_six_caps_the_grid():
    """A 3:3 page takes 9 tiles under OCR1's max_num 9 and at most 6 under OCR2's (preprocess.rs:27-35)."""
    w = h = 2400
    st1, crop1, tiles1, slots1 = _page(w, h, 1024, 768, True, 0)
    st2, crop2, tiles2, slots2 = _page(w, h, 1024, 768, True, 1)
    assert (st1, st2) == (0, 0)
    assert crop1 == ocr2_ref.tile_grid(w, h, 768, 9) and tiles1 >= 7
    assert crop2 == ocr2_ref.tile_grid(w, h, 768, 6) and tiles2 <= 6 and tiles2 == crop2[0] * crop2[1]
    assert slots2 == ocr2_ref.placeholder_count(1024, 768, True, crop2)
    # the existing entry is variant 0, bit for bit the same page description
    rgb = np.full((h, w, 3), 128, np.uint8)
    vs = VisionSettingsC(1024, 768, 1)
    hnd = C.c_void_p()
    assert lib().dsocr_prepare_page(rgb.ctypes.data_as(C.c_void_p), w, h, C.byref(vs), C.byref(hnd)) == 0
    cw, ch, nt, ntok = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_size_t()
    assert lib().dsocr_page_info(hnd, C.byref(cw), C.byref(ch), C.byref(nt), C.byref(ntok)) == 0
    lib().dsocr_page_free(hnd)
    assert ((cw.value, ch.value), nt.value, ntok.value) == (crop1, tiles1, slots1)


@pytest.mark.parametrize("size,slots", [(768, 145), (1024, 257)])
def test_ocr2_non_crop_slots(size, slots):
    st, crop, tiles, n = _page(900, 700, 1024, size, False, 1)
    assert (st, crop, tiles, n) == (0, (1, 1), 0, slots)
    assert n == ocr2_ref.placeholder_count(1024, size, False, None)


def test_ocr2_other_global_sizes_are_einval():
    assert _page(300, 200, 1024, 640, False, 1)[0] == 1      # global view = image_size 640
    assert b"768 or 1024" in lib().dsocr_last_error()
    assert _page(300, 200, 512, 768, True, 1)[0] == 1        # global view = base_size 512
    assert _page(300, 200, 1024, 768, True, 2)[0] == 1       # unknown variant
    assert _page(300, 200, 1024, 640, False, 0)[0] == 0      # variant 0 is not restricted


# ---------------------------------------------------------------- C ABI exports
def test_c_abi_exports_the_ocr2_symbols():
    header = open(os.path.join(ROOT, "include", "dsocr.h")).read()
    declared = set(re.findall(r"\b(dsocr_[a-z0-9_]+)\s*\(", header))
    L = lib()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in EXPORTS, s
        assert hasattr(L, s), s


# ---------------------------------------------------------------- independent pin (transformers)
def test_ref_encoder_matches_transformers_vision_model():
    """tests/ocr2_ref.py's SAM -> Qwen2 encoder against transformers' DeepseekOcr2VisionModel on the same seeded f32
    weights: P = 144 (768 px), 2 layers, 4 / 2 heads.  Bound: the relative 2e-4 tests/test_oracle_crosscheck.py holds
    its SAM and text checks to."""
    torch = pytest.importorskip("torch")
    M = pytest.importorskip("transformers.models.deepseek_ocr2.modeling_deepseek_ocr2")
    Cfg = pytest.importorskip("transformers.models.deepseek_ocr2.configuration_deepseek_ocr2")
    cfg = json.load(open(os.path.join(CFG, "ocr2-tiny.json")))
    W = Weights(seed=21, dtype="f16")
    vis = ocr2_ref.Ocr2Vision(cfg, W)
    p, q = vis.sam.p, vis.enc.p
    sc = dict(hidden_size=p.embed_dim, output_channels=p.neck_channels, num_hidden_layers=p.depth,
              num_attention_heads=p.num_heads, image_size=p.image_size, patch_size=p.patch_size, hidden_act="gelu",
              layer_norm_eps=p.norm_eps, qkv_bias=True, mlp_ratio=p.mlp_ratio, window_size=p.window_size,
              global_attn_indexes=list(p.global_attn_indexes), downsample_channels=list(p.out_channels))
    ec = dict(hidden_size=q["dim"], intermediate_size=q["inter"], num_hidden_layers=q["layers"],
              num_attention_heads=q["heads"], num_key_value_heads=q["kv_heads"], hidden_act="silu",
              rms_norm_eps=q["eps"], max_position_embeddings=4096,
              rope_parameters={"rope_type": "default", "rope_theta": float(q["theta"])})
    vc = Cfg.DeepseekOcr2VisionConfig(sam_config=sc, encoder_config=ec)
    vc._attn_implementation = "eager"
    vc.sam_config._attn_implementation = "eager"
    vc.encoder_config._attn_implementation = "eager"
    model = M.DeepseekOcr2VisionModel(vc).eval()

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a, np.float32))

    sd = {}
    C_, tg = p.embed_dim, p.image_size // p.patch_size
    g = lambda n, s: t(W.get("model.sam_model." + n, s))
    nc = p.neck_channels
    c0, c1 = p.out_channels
    sd.update({"patch_embed.projection.weight": g("patch_embed.proj.weight", (C_, 3, p.patch_size, p.patch_size)),
               "patch_embed.projection.bias": g("patch_embed.proj.bias", (C_,)),
               "pos_embed": g("pos_embed", (1, tg, tg, C_)),
               "neck.conv1.weight": g("neck.0.weight", (nc, C_, 1, 1)),
               "neck.layer_norm1.weight": g("neck.1.weight", (nc,)), "neck.layer_norm1.bias": g("neck.1.bias", (nc,)),
               "neck.conv2.weight": g("neck.2.weight", (nc, nc, 3, 3)),
               "neck.layer_norm2.weight": g("neck.3.weight", (nc,)), "neck.layer_norm2.bias": g("neck.3.bias", (nc,)),
               "proj.conv1.weight": g("net_2.weight", (c0, nc, 3, 3)), "proj.conv2.weight": g("net_3.weight", (c1, c0, 3, 3))})
    hid = int(C_ * p.mlp_ratio)
    for b in range(p.depth):
        s, k = f"blocks.{b}.", f"layers.{b}."
        tok = tg if b in p.global_attn_indexes else p.window_size
        hd = C_ // p.num_heads
        sd.update({k + "layer_norm1.weight": g(s + "norm1.weight", (C_,)), k + "layer_norm1.bias": g(s + "norm1.bias", (C_,)),
                   k + "layer_norm2.weight": g(s + "norm2.weight", (C_,)), k + "layer_norm2.bias": g(s + "norm2.bias", (C_,)),
                   k + "attn.qkv.weight": g(s + "attn.qkv.weight", (3 * C_, C_)), k + "attn.qkv.bias": g(s + "attn.qkv.bias", (3 * C_,)),
                   k + "attn.proj.weight": g(s + "attn.proj.weight", (C_, C_)), k + "attn.proj.bias": g(s + "attn.proj.bias", (C_,)),
                   k + "attn.rel_pos_h": g(s + "attn.rel_pos_h", (2 * tok - 1, hd)),
                   k + "attn.rel_pos_w": g(s + "attn.rel_pos_w", (2 * tok - 1, hd)),
                   k + "mlp.lin1.weight": g(s + "mlp.fc1.weight", (hid, C_)), k + "mlp.lin1.bias": g(s + "mlp.fc1.bias", (hid,)),
                   k + "mlp.lin2.weight": g(s + "mlp.fc2.weight", (C_, hid)), k + "mlp.lin2.bias": g(s + "mlp.fc2.bias", (C_,))})
    full = {"sam_encoder." + k: v for k, v in sd.items()}
    D, hd, nh, nkv, I = q["dim"], q["hd"], q["heads"], q["kv_heads"], q["inter"]
    e = lambda n, s: t(W.get("model.qwen2_model." + n, s))
    full["query_768_resolution.weight"] = e("query_768.weight", (144, D))
    full["query_1024_resolution.weight"] = e("query_1024.weight", (256, D))
    full["vision_encoder.norm.weight"] = e("model.model.norm.weight", (D,))
    for li in range(q["layers"]):
        s, k = f"model.model.layers.{li}.", f"vision_encoder.layers.{li}."
        for n, rows in (("q_proj", nh * hd), ("k_proj", nkv * hd), ("v_proj", nkv * hd)):
            full[k + f"self_attn.{n}.weight"] = e(s + f"self_attn.{n}.weight", (rows, D))
            full[k + f"self_attn.{n}.bias"] = e(s + f"self_attn.{n}.bias", (rows,))
        full[k + "self_attn.o_proj.weight"] = e(s + "self_attn.o_proj.weight", (D, nh * hd))
        full[k + "input_layernorm.weight"] = e(s + "input_layernorm.weight", (D,))
        full[k + "post_attention_layernorm.weight"] = e(s + "post_attention_layernorm.weight", (D,))
        for n, shp in (("gate_proj", (I, D)), ("up_proj", (I, D)), ("down_proj", (D, I))):
            full[k + f"mlp.{n}.weight"] = e(s + f"mlp.{n}.weight", shp)
    missing, unexpected = model.load_state_dict(full, strict=False)
    assert not unexpected and all("rotary" in m for m in missing), (missing, unexpected)

    img = np.random.default_rng(5).uniform(-1, 1, (1, 3, 768, 768)).astype(np.float32)
    sam = vis.sam.forward(img)
    assert sam.shape == (1, 12, 12, D)
    ref = vis.enc.forward(sam.reshape(1, 144, D))
    with torch.no_grad():
        got = model(pixel_values=t(img)).last_hidden_state.numpy()
    assert got.shape == ref.shape == (1, 144, D)
    rel = float(np.max(np.abs(got - ref)) / max(1e-6, np.max(np.abs(ref))))
    print("ref encoder vs transformers: rel", rel)
    assert rel < 2e-4, rel
