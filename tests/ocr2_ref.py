"""CPU reference of the DeepSeek-OCR-2 vision path (TEST INFRASTRUCTURE), beside the read-only oracle/.

f32 numpy restatement of the reference's OCR2 additions; SAM, the decoder, weights and preprocessing come from
oracle/ unchanged:
  * detect_ocr_variant                      model/mod.rs:2691-2710
  * SAM out-channel rule                    vision/sam.rs:60-90
  * encoder constants                       vision/qwen2.rs:12-22, 53-103
  * Qwen2DecoderAsEncoder::forward          vision/qwen2.rs:146-220 (TransformerBlock = transformer/block.rs)
  * build_custom_attention_mask             vision/qwen2.rs:519-571
  * build_rope_tables                       vision/qwen2.rs:573-604
  * Qwen2Projector                          vision/qwen2.rs:407-444
  * Qwen2VisionEncoder::encode (assembly)   vision/qwen2.rs:337-372
  * build_image_placeholders (Ocr2)         model/mod.rs:2630-2680
  * PreprocessParams::ocr2 (max_num 6)      vision/preprocess.rs:27-35, model/mod.rs:1714-1726
"""
from __future__ import annotations

import math

import numpy as np

from oracle import preprocess
from oracle.config import resolved_language_config
from oracle.decoder import Decoder, apply_rope, rms_norm, silu, softmax
from oracle.model import OracleModel
from oracle.vision import Sam, linear

F32 = np.float32
QUERY_768, QUERY_1024 = 144, 256


def detect_variant(cfg: dict) -> int:
    """model/mod.rs:2691-2710: 1 (Ocr2) when vision_config.model_name is `deepencoderv2` (any case) or
    vision_config.width has a `qwen2-0-5b` entry, else 0."""
    vis = cfg.get("vision_config") or {}
    name = vis.get("model_name")
    if isinstance(name, str) and name.lower() == "deepencoderv2":
        return 1
    if (vis.get("width") or {}).get("qwen2-0-5b") is not None:
        return 1
    return 0


def enc_params(cfg: dict) -> dict:
    """qwen2.rs:12-22 constants; the qwen2-0-5b entry's width / dim is the reference's (sam.rs:64-73), the other
    overrides are the engine's documented testing extension."""
    q = ((cfg.get("vision_config") or {}).get("width") or {}).get("qwen2-0-5b") or {}
    p = dict(dim=896, layers=24, heads=14, kv_heads=2, inter=4864, eps=1e-6, theta=1e6)
    p["dim"] = q.get("width") or q.get("dim") or p["dim"]
    for src, dst in (("layers", "layers"), ("heads", "heads"), ("kv_heads", "kv_heads"), ("intermediate_size", "inter")):
        if q.get(src):
            p[dst] = q[src]
    p["hd"] = p["dim"] // p["heads"]
    return p


def sam_out_channels(cfg: dict, configured: list) -> list:
    """sam.rs:64-90: the last downsample channel is forced to the encoder width."""
    dim = enc_params(cfg)["dim"]
    out = list(configured)
    if not out or out[-1] != dim:
        out = [out[0] if out else 512, dim]
    return out


def visible_mask(P: int) -> np.ndarray:
    """qwen2.rs:519-571 as booleans over [image | query] rows: row i sees key j iff j < P or (i >= P and j <= i)."""
    L = 2 * P
    i = np.arange(L)[:, None]
    j = np.arange(L)[None, :]
    return (j < P) | ((i >= P) & (j <= i))


def rope_tables(length: int, rope_dim: int, theta: float):
    """qwen2.rs:573-604: inv_freq = 1 / theta^(i / half) in f32, f32 angles, [half | half]."""
    half = rope_dim // 2
    base = F32(theta)
    inv = np.array([F32(1.0) / (base ** (F32(i) / F32(half))) for i in range(half)], F32)
    ang = (np.arange(length, dtype=F32)[:, None] * inv[None, :]).astype(F32)
    cos, sin = np.cos(ang).astype(F32), np.sin(ang).astype(F32)
    return np.concatenate([cos, cos], 1), np.concatenate([sin, sin], 1)


class Qwen2Encoder:
    """Qwen2DecoderAsEncoder (qwen2.rs:106-244) on a weight source with .get(name, shape)."""

    def __init__(self, cfg: dict, W, prefix="model.qwen2_model."):
        self.p = enc_params(cfg)
        self.W = W
        self.pre = prefix

    def g(self, name, shape):
        return self.W.get(self.pre + name, shape)

    def query(self, P):
        D = self.p["dim"]
        if P == QUERY_768:
            return self.g("query_768.weight", (QUERY_768, D))
        if P == QUERY_1024:
            return self.g("query_1024.weight", (QUERY_1024, D))
        raise ValueError(f"unsupported Qwen2 query length {P} (expected {QUERY_768} or {QUERY_1024})")

    def forward(self, tokens: np.ndarray) -> np.ndarray:
        """tokens [B, P, D] (SAM features, row-major) -> query features [B, P, D]."""
        p = self.p
        B, P, D = tokens.shape
        assert D == p["dim"]
        nh, nkv, hd, I = p["heads"], p["kv_heads"], p["hd"], p["inter"]
        L = 2 * P
        x = np.concatenate([tokens, np.broadcast_to(self.query(P), (B, P, D))], 1).astype(F32)
        bias = np.where(visible_mask(P), F32(0.0), np.finfo(F32).min).astype(F32)   # f32::MIN added to the scores
        cos, sin = rope_tables(L, hd, p["theta"])
        scale = F32(math.sqrt(hd))
        for li in range(p["layers"]):
            lp = f"model.model.layers.{li}."
            h = rms_norm(x, self.g(lp + "input_layernorm.weight", (D,)), p["eps"]).reshape(B * L, D)
            q = linear(h, self.g(lp + "self_attn.q_proj.weight", (nh * hd, D)), self.g(lp + "self_attn.q_proj.bias", (nh * hd,)))
            k = linear(h, self.g(lp + "self_attn.k_proj.weight", (nkv * hd, D)), self.g(lp + "self_attn.k_proj.bias", (nkv * hd,)))
            v = linear(h, self.g(lp + "self_attn.v_proj.weight", (nkv * hd, D)), self.g(lp + "self_attn.v_proj.bias", (nkv * hd,)))
            q = q.reshape(B, L, nh, hd).transpose(0, 2, 1, 3)
            k = k.reshape(B, L, nkv, hd).transpose(0, 2, 1, 3)
            v = v.reshape(B, L, nkv, hd).transpose(0, 2, 1, 3)
            q = apply_rope(q, cos, sin, False)
            k = apply_rope(k, cos, sin, False)
            k = np.repeat(k, nh // nkv, axis=1)
            v = np.repeat(v, nh // nkv, axis=1)
            s = ((q @ k.transpose(0, 1, 3, 2)) / scale + bias[None, None]).astype(F32)
            o = (softmax(s) @ v).transpose(0, 2, 1, 3).reshape(B * L, nh * hd)
            x = x + linear(o, self.g(lp + "self_attn.o_proj.weight", (D, nh * hd))).reshape(B, L, D)   # no o_proj bias
            h = rms_norm(x, self.g(lp + "post_attention_layernorm.weight", (D,)), p["eps"]).reshape(B * L, D)
            gate = linear(h, self.g(lp + "mlp.gate_proj.weight", (I, D)))
            up = linear(h, self.g(lp + "mlp.up_proj.weight", (I, D)))
            x = x + linear((silu(gate) * up).astype(F32), self.g(lp + "mlp.down_proj.weight", (D, I))).reshape(B, L, D)
        x = rms_norm(x, self.g("model.model.norm.weight", (D,)), p["eps"])
        return np.ascontiguousarray(x[:, P:], F32)


class Ocr2Vision:
    """Qwen2VisionEncoder (qwen2.rs:265-405): SAM -> encoder -> projector, flat assembly."""

    def __init__(self, cfg: dict, W):
        self.cfg, self.W = cfg, W
        self.sam = Sam(cfg, W)
        self.sam.p.out_channels = sam_out_channels(cfg, self.sam.p.out_channels)
        self.enc = Qwen2Encoder(cfg, W)
        self.n_embed = (cfg.get("projector_config") or {}).get("n_embed") or resolved_language_config(cfg).hidden_size

    def separator(self):
        return self.W.get("model.view_seperator", (self.n_embed,))

    def encode_view(self, img):
        """img [B,3,S,S] -> [B, (S/64)^2, n_embed]."""
        sam = self.sam.forward(img)                          # NHWC [B, g, g, D]
        b, gh, gw, d = sam.shape
        feat = self.enc.forward(sam.reshape(b, gh * gw, d))  # == flatten(2,3).transpose(1,2) of the NCHW tensor
        w = self.W.get("model.projector.layers.weight", (self.n_embed, d))
        bias = self.W.get("model.projector.layers.bias", (self.n_embed,))
        return linear(feat.reshape(-1, d), w, bias).reshape(b, gh * gw, self.n_embed)

    def embeddings(self, glob, patches):
        """[tile tokens (tile-major, row-major inside a tile) | global tokens | view separator]."""
        segs = []
        if patches is not None and len(patches) > 0:
            segs.append(self.encode_view(patches).reshape(-1, self.n_embed))
        segs.append(self.encode_view(glob)[0])
        segs.append(self.separator()[None])
        return np.concatenate(segs, 0).astype(F32)


def tile_grid(width: int, height: int, tile: int, max_num: int = 6, min_num: int = 2):
    """preprocess.rs:67-138 grid choice only (no pixels): (w, h) of the crop grid, (1, 1) when the page needs no tiles."""
    if width <= tile and height <= tile:
        return (1, 1)
    aspect = width / height
    ratios = sorted({(i, j) for n in range(min_num, max_num + 1) for i in range(1, n + 1)
                     for j in range(1, n + 1) if min_num <= i * j <= max_num})
    best, best_diff = (1, 1), float("inf")
    area = float(width * height)
    for (wr, hr) in ratios:
        diff = abs(aspect - wr / hr)
        if diff < best_diff:
            best_diff, best = diff, (wr, hr)
        elif abs(diff - best_diff) < 2.220446049250313e-16 and area > 0.5 * (tile * tile * wr * hr):
            best = (wr, hr)
    return best


def placeholder_count(base_size: int, image_size: int, crop_mode: bool, crop_shape) -> int:
    """model/mod.rs:2630-2680 (Ocr2): flat grids, then one separator slot."""
    patch, down = 16, 4
    if crop_mode:
        ng = int(math.ceil((base_size // patch) / down))
        nl = int(math.ceil((image_size // patch) / down))
        wc, hc = crop_shape if crop_shape is not None else (1, 1)
        n = nl * nl * wc * hc if (wc > 1 or hc > 1) else 0
        return n + ng * ng + 1
    nq = int(math.ceil((image_size // patch) / down))
    return nq * nq + 1


def prepare_vision_input(img: np.ndarray, base: int = 1024, image_size: int = 768, crop_mode: bool = True):
    """model/mod.rs:1707-1758 with PreprocessParams::ocr2 (max_num 6)."""
    gsize = base if crop_mode else image_size
    glob = preprocess.image_to_tensor(preprocess.build_global_view(img, gsize))[None]
    if crop_mode:
        tiles, crop = preprocess.dynamic_preprocess(img, image_size, 2, 6)
        patches = np.stack([preprocess.image_to_tensor(t) for t in tiles]) if tiles else None
        return glob, patches, crop
    return glob, None, None


class Ocr2Model(OracleModel):
    """OracleModel with the OCR2 vision path; prefill_embeddings / generate are inherited unchanged."""

    def __init__(self, cfg: dict, weights):  # (OracleModel.__init__ builds the CLIP tower: not called)
        self.cfg = cfg
        self.W = weights
        self.vision = Ocr2Vision(cfg, weights)
        self.dec = Decoder(cfg, weights)
        self.lang = resolved_language_config(cfg)

    def image_embeddings(self, rgb: np.ndarray, base=1024, image_size=768, crop_mode=True):
        glob, patches, crop = prepare_vision_input(rgb, base, image_size, crop_mode)
        return self.vision.embeddings(glob, patches), crop
