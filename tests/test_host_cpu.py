"""CPU tests: oracle pinning (Pillow, reference constants), host preprocessing of
the product library (host-only entry points, no GPU), synthetic-weight recipe,
and the C-ABI export surface."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
from PIL import Image

from oracle import preprocess as opre
from oracle.config import clip_params, resolved_language_config, sam_params, should_use_moe
from oracle.decoder import banned_ngram_tokens, select_token_id
from oracle.weights import synth_bf16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = os.path.join(ROOT, "deepseek-ocr.rs_amd", "dsocr", "configs", "deepseek-ocr.json")
TINY = os.path.join(ROOT, "deepseek-ocr.rs_amd", "dsocr", "configs", "tiny.json")


def _lib():
    from dsocr._lib import lib
    return lib()


def _rand_img(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ----------------------------------------------------------------- oracle pinned by Pillow
# The reference resampler reproduces Pillow's 22-bit integer bicubic (resample.rs:9-11) except
# one detail: its round_half_towards_zero(center - support) (resample.rs:24-30, 55) yields
# xmin = 1 where Pillow's (int)(x + 0.5) truncation yields 0, for center - support in (-0.5, 0)
# -- i.e. only at strong upscales (scale < 0.5).  We follow the reference; these cases are
# pinned against Pillow only where the two agree, and product == oracle bit-exactly everywhere.
PILLOW_EXACT = [((37, 53), (20, 31)), ((300, 420), (128, 256)), ((64, 64), (64, 64)),
                ((1024, 1024), (1280, 1280)), ((1756, 2852), (1280, 1920)), ((2852, 1756), (1024, 631))]
REF_ONLY = [((100, 80), (640, 512)), ((17, 900), (40, 300))]


@pytest.mark.parametrize("src,dst", PILLOW_EXACT)
def test_oracle_resize_matches_pillow(src, dst):
    img = _rand_img(src[0], src[1], 3)
    ref = np.asarray(Image.fromarray(img).resize((dst[1], dst[0]), Image.BICUBIC))
    got = opre.resize_bicubic(img, dst[1], dst[0])
    assert np.array_equal(got, ref)


def test_reference_xmin_rounding_deviation_is_the_only_pillow_gap():
    """Strong upscale: the only difference to Pillow comes from the xmin rounding above."""
    row = np.random.default_rng(3).integers(0, 256, (1, 10, 3), dtype=np.uint8)
    b, _, _ = opre.compute_resample_coeffs(10, 40)
    assert b[6][0] == 1  # center 1.625 - support 2 = -0.375 -> reference rounds to 1 (Pillow: 0)
    got = opre.resize_bicubic(row, 40, 1)
    ref = np.asarray(Image.fromarray(row).resize((40, 1), Image.BICUBIC))
    diff = np.nonzero(np.any(got != ref, axis=-1)[0])[0]
    assert set(diff.tolist()) <= {6, 7}


@pytest.mark.parametrize("src,dst", PILLOW_EXACT + REF_ONLY)
def test_product_resize_bit_exact_vs_oracle(src, dst):
    img = _rand_img(src[0], src[1], 5)
    out = np.empty((dst[0], dst[1], 3), np.uint8)
    assert _lib().dsocr_resize_bicubic(img.ctypes.data_as(C.c_void_p), src[1], src[0],
                                       out.ctypes.data_as(C.c_void_p), dst[1], dst[0]) == 0
    assert np.array_equal(out, opre.resize_bicubic(img, dst[1], dst[0]))


@pytest.mark.parametrize("hw,expect", [((1024, 1024), (2, 2)), ((1756, 2852), (3, 2)), ((600, 500), (1, 1)),
                                       ((2000, 700), (1, 3)), ((700, 2600), (4, 1))])
def test_crop_grid(hw, expect):
    """dynamic_preprocess_with_params (preprocess.rs:67-138); 1024^2 -> (2,2) is SURVEY §0's 4 tiles."""
    img = _rand_img(hw[0], hw[1], 1)
    _, grid = opre.dynamic_preprocess(img, 640)
    assert grid == expect


def test_placeholder_counts():
    """1024^2 page, crop (2,2): 420 local + 273 global = 693 image tokens."""
    from oracle.model import image_placeholder_count
    assert image_placeholder_count(1024, 640, True, (2, 2)) == 693
    assert image_placeholder_count(1024, 640, True, (1, 1)) == 273
    assert image_placeholder_count(1024, 640, False, None) == 111


@pytest.mark.parametrize("hw,vs", [((1024, 1024), (1024, 640, True)), ((300, 420), (256, 128, True)),
                                   ((500, 333), (1024, 640, True)), ((900, 1300), (1024, 640, False))])
def test_product_prepare_page_matches_oracle(hw, vs):
    from dsocr import Page, VisionSettings
    img = _rand_img(hw[0], hw[1], 11)
    page = Page(img, VisionSettings(*vs))
    g, tiles = page.pixels()
    og, otiles, ocrop = opre.prepare_vision_input(img, vs[0], vs[1], vs[2])
    assert np.array_equal(g, og[0])
    if otiles is None:
        assert tiles is None
    else:
        assert page.crop_shape == ocrop
        assert np.array_equal(tiles, otiles)
    from oracle.model import image_placeholder_count
    assert page.n_image_tokens == image_placeholder_count(vs[0], vs[1], vs[2], ocrop)


# ----------------------------------------------------------------- reference constants
def test_reference_config_constants():
    """tests/config.rs:32-58, vision_sam.rs:25-36, vision_clip.rs:9-20, transformer_weights.rs:32-43."""
    cfg = json.load(open(FULL))
    lang = resolved_language_config(cfg)
    assert (lang.hidden_size, lang.num_hidden_layers, lang.num_attention_heads) == (1280, 12, 10)
    assert lang.torch_dtype == "bfloat16"
    sp = sam_params(cfg)
    assert (sp.image_size, sp.patch_size, sp.embed_dim, sp.depth, sp.num_heads) == (1024, 16, 768, 12, 12)
    assert sp.global_attn_indexes == [2, 5, 8, 11]
    cp = clip_params(cfg)
    assert (cp.hidden_size, cp.num_heads, cp.num_layers, cp.patch_size, cp.image_size) == (1024, 16, 24, 14, 224)
    assert cp.seq_length + 1 == 257
    assert not should_use_moe(lang, 0) and should_use_moe(lang, 1)


def test_window_partition_math():
    """vision_sam.rs:70-81: (64, 48, 14) -> padded 70 x 56, tiles 5 x 4."""
    h, w, win = 64, 48, 14
    ph, pw = (win - h % win) % win, (win - w % win) % win
    assert (h + ph, w + pw, (h + ph) // win, (w + pw) // win) == (70, 56, 5, 4)


def test_clip_pos_downsample_shape():
    """vision_clip.rs:22-33: 257 -> 101 tokens."""
    from oracle.vision import bicubic_resize_antialiased
    tab = np.zeros((1024, 16, 16), np.float32)
    assert bicubic_resize_antialiased(tab, 10, 10).shape == (1024, 10, 10)


def test_aa_bicubic_matches_torch():
    """sam.rs:1000-1123 restates aten::_upsample_bicubic2d_aa; pin the oracle against torch."""
    torch = pytest.importorskip("torch")
    from oracle.vision import bicubic_resize_antialiased
    x = np.random.default_rng(0).standard_normal((8, 64, 64)).astype(np.float32)
    ref = torch.nn.functional.interpolate(torch.from_numpy(x)[None], size=(40, 40), mode="bicubic",
                                          align_corners=False, antialias=True)[0].numpy()
    got = bicubic_resize_antialiased(x, 40, 40)
    assert np.max(np.abs(got - ref)) < 1e-5


def test_rel_pos_resize_matches_torch_linear():
    """get_rel_pos_vec's resize = F.interpolate(mode='linear'), sam.rs:1202-1231."""
    torch = pytest.importorskip("torch")
    from oracle.vision import get_rel_pos
    rel = np.random.default_rng(1).standard_normal((127, 64)).astype(np.float32)
    ref = torch.nn.functional.interpolate(torch.from_numpy(rel.T)[None], size=79, mode="linear")[0].numpy().T
    out = get_rel_pos(40, 40, rel)  # [q, k, hd] gathered from the resized table
    for qi, ki in [(0, 0), (5, 17), (39, 0), (0, 39), (20, 20)]:
        assert np.max(np.abs(out[qi, ki] - ref[qi - ki + 39])) < 1e-6


# ----------------------------------------------------------------- sampling semantics
def test_ngram_ban_and_argmax_ties():
    seq = [1, 2, 3, 1, 2]
    assert banned_ngram_tokens(seq, 3) == {3}
    assert banned_ngram_tokens([5, 6], 3) == set()
    lg = np.zeros(8, np.float32)
    lg[3] = lg[5] = 2.0
    assert select_token_id(lg, [0], 1.0, None) == 3            # first index on ties
    assert select_token_id(lg, [1, 2, 3, 1, 2], 1.0, 3) == 5   # 3 banned
    lg2 = np.full(4, -np.inf, np.float32)
    assert select_token_id(lg2, [0], 1.0, None) == 0


def test_repetition_penalty():
    lg = np.array([1.0, -1.0, 0.5, 3.0], np.float32)
    assert select_token_id(lg, [3], 4.0, None) == 0            # 3.0/4 < 1.0


# ----------------------------------------------------------------- synthetic recipe + C ABI
@pytest.mark.parametrize("name", ["model.layers.3.mlp.experts.7.up_proj.weight", "model.sam_model.blocks.0.norm1.weight",
                                  "lm_head.weight"])
def test_synth_recipe_product_equals_oracle(name):
    n = 4097
    ora = synth_bf16(name, 1234, n)
    prod = np.empty(n, np.uint16)
    assert _lib().dsocr_synth_bf16(name.encode(), 1234, n, prod.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(ora, prod)


def test_c_abi_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "dsocr.h")).read()
    declared = set(re.findall(r"\b(dsocr_[a-z0-9_]+)\s*\(", header)) - {"dsocr_stream_cb"}
    from dsocr._lib import EXPORTS
    assert declared == set(EXPORTS)
    L = _lib()
    for s in declared:
        assert hasattr(L, s), s


@pytest.mark.parametrize("waiting,api,cus,fits", [
    # dec_qkv_attn at its bound (24 chunks x 10 heads poll the q/k/v row): 4 blocks per CU (102 VGPRs) x 256 CUs
    (24 * 10, 4, 256, 1),
    # the same grid on a part that could hold one block per CU on 240 CUs: every slot could be a waiter
    (24 * 10, 1, 240, 0), (24 * 10, 1, 241, 1),
    # the 8-page polling merge: 8 pages x 10 heads merging blocks (the rest of the 1600-block grid never waits)
    (8 * 10, 4, 256, 1),
    # the API may over-admit one block per CU at 6..8: 7 reported -> 6 usable
    (6 * 256, 7, 256, 0), (6 * 256 - 1, 7, 256, 1), (8 * 256 - 1, 12, 256, 0), (7 * 256 - 1, 12, 256, 1),
    # no slot at all (occupancy query failed -> 0): never poll
    (1, 0, 256, 0), (0, 0, 256, 1)])
def test_poll_residency_rule(waiting, api, cus, fits):
    """Residency rule of the in-launch polled hand-offs (dec_qkv_attn, the dec_attn polling merge): the launch
    polls only if the blocks that may wait cannot fill every slot the device has for the kernel (HIP promises
    no dispatch order), else the engine takes the non-polling form.  Pure host decision through the C ABI."""
    assert _lib().dsocr_k_poll_wait_fits(waiting, api, cus) == fits


def test_engine_load_errors_without_gpu_are_loud():
    """The product path must fail loudly (never fall back to CPU) when no device/config is usable."""
    from dsocr import DsocrError, ModelLoadArgs, load_model
    with pytest.raises(DsocrError):
        load_model(ModelLoadArgs(config_path="/nonexistent/config.json"))


# Decode MoE dispatch over T = 1..9 tokens, I = 896, norm fused: (Is, (E, topk), H) -> "gate-up/down" per T, as the
# query answered BEFORE the plan was made the launch's own switch (recorded from that build), then corrected by
# _moe_names_fix for the two shapes where that answer named a kernel the launch did not run.
_MOE_GU = {"mix": "moe_gateup_mix_kernel", "slot": "moe_gateup_slot_kernel", "gu2": "moe_gateup2_kernel",
           "slot+sh": "moe_gateup_slot_kernel+moe_gateup_shared_kernel", "mm": "moe_gateup_mm_kernel"}
_MOE_DN = {"mix": "moe_down_mix_kernel", "slot": "moe_down_slot_kernel", "dn2": "moe_down2_kernel", "mm": "moe_down_mm_kernel"}
_MOE_NAMES_RECORDED = {
    (0, (64, 6), 1280): "mix/mix slot/slot mm/mm mm/mm mm/mm mm/mm mm/mm mm/mm gu2/dn2",
    (0, (64, 6), 2048): "slot/mix slot/slot slot/slot slot/slot slot/slot slot/slot slot/slot slot/slot gu2/dn2",
    (0, (128, 8), 1280): "slot/mix slot/slot mm/mm mm/mm mm/mm mm/mm mm/mm mm/mm gu2/dn2",
    (0, (128, 8), 2048): "slot/mix slot/slot slot/slot slot/slot slot/slot slot/slot slot/slot slot/slot gu2/dn2",
    (1792, (64, 6), 1280): "mix/mix slot/slot mm/mm mm/mm mm/mm mm/mm mm/mm mm/mm gu2/dn2",
    (1792, (64, 6), 2048): "slot/mix slot/slot slot+sh/slot slot+sh/slot slot+sh/slot slot+sh/slot slot+sh/slot slot+sh/slot gu2/dn2",
    (1792, (128, 8), 1280): "slot/slot slot/slot mm/mm mm/mm mm/mm mm/mm mm/mm mm/mm gu2/dn2",
    (1792, (128, 8), 2048): "slot/slot slot/slot slot+sh/slot slot+sh/slot slot+sh/slot slot+sh/slot slot+sh/slot slot+sh/slot gu2/dn2",
}
# (DSOCR_ROUTE_FUSED, (E, topk), H) -> routing implementation per T (the same with and without a shared expert); recorded
# from the same build, nothing corrected
_MOE_ROUTE_RECORDED = {
    **{(f, (64, 6), 1280): ["moe_gateup_mix", "moe_gateup_slot"] + [k] * 6 + ["moe_route"]
       for f, k in (("0", "dec_route_grp"), ("1", "moe_gateup_mm"))},
    **{(f, (128, 8), 1280): ["moe_gateup_slot"] * 2 + ["dec_router"] * 6 + ["moe_route"] for f in "01"},
    **{(f, ek, 2048): ["moe_gateup_slot"] * 8 + ["moe_route"] for f in "01" for ek in ((64, 6), (128, 8))},
}


def _moe_names_fix(gu, dn, H, topk):
    # 1. H > 1536 in slot mode (T <= 8 here): the name said moe_gateup_slot_kernel (+ shared), but the slot kernels
    #    stage K <= 1536 and launch_moe_gateup2 fell through to moe_gateup2_kernel (its self-routing slot branch)
    if H > 1536 and gu in ("slot", "slot+sh"):
        gu = "gu2"
    # 2. top-k 8 in slot mode: moe_down_slot_kernel exists for top-k 6 and 3 only, so wherever the split-K
    #    moe_down_mix_kernel did not take the token, launch_moe_down2 ran moe_down2_kernel under the name of the slot one
    if topk == 8 and dn == "slot":
        dn = "dn2"
    return gu, dn


_MOE_GRID = [(T, Is, ek, H) for T in range(1, 10) for Is in (0, 1792) for ek in ((64, 6), (128, 8)) for H in (1280, 2048)]


def test_moe_dispatch_kernel_names(monkeypatch):
    """Which kernels the dispatch picks (host-only query; the bench labels its roofline with it): the plan the launch
    switches on, over every token count of the decode forms, with and without a shared expert, 64 x top-6 and
    128 x top-8 experts, a hidden size the slot kernels stage and one they do not, both DSOCR_ROUTE_FUSED values."""
    import ctypes as C
    from dsocr._lib import check, lib
    for fused, (T, Is, (E, topk), H) in [(f, g) for f in "01" for g in _MOE_GRID]:
        monkeypatch.setenv("DSOCR_ROUTE_FUSED", fused)
        gu, dn = _MOE_NAMES_RECORDED[(Is, (E, topk), H)].split()[T - 1].split("/")
        gu, dn = _moe_names_fix(gu, dn, H, topk)
        g, d = C.c_char_p(), C.c_char_p()
        check(lib().dsocr_k_moe_kernels(T, H, E, topk, 896, Is, 1, C.byref(g), C.byref(d)))
        assert (g.value.decode(), d.value.decode()) == (_MOE_GU[gu], _MOE_DN[dn]), (fused, T, Is, E, topk, H)
    # the flagship's forms (1280 hidden, 64 x top-6 + 2 shared) as they were pinned before the grid
    want = {1: ("mix", "mix"), 2: ("slot", "slot"), 3: ("mm", "mm"), 8: ("mm", "mm"), 9: ("gu2", "dn2")}
    flag = _MOE_NAMES_RECORDED[(1792, (64, 6), 1280)].split()
    assert all(tuple(flag[T - 1].split("/")) == w for T, w in want.items())


def test_moe_dispatch_route_kinds(monkeypatch):
    """Which routing implementation the same plan picks (dsocr_k_moe_route_kind; test_moe_routing chooses its oracle
    by it), over the same grid."""
    import ctypes as C
    from dsocr._lib import check, lib
    for fused, (T, Is, (E, topk), H) in [(f, g) for f in "01" for g in _MOE_GRID]:
        monkeypatch.setenv("DSOCR_ROUTE_FUSED", fused)
        k = C.c_char_p()
        check(lib().dsocr_k_moe_route_kind(T, H, E, topk, 896, Is, 1, C.byref(k)))
        assert k.value.decode() == _MOE_ROUTE_RECORDED[(fused, (E, topk), H)][T - 1], (fused, T, Is, E, topk, H)


# (M, N, K, ldw, wdtype, norm, xn_out, swizzle) -> (kind, token rows per launch), worked out by hand from
# dec_gemv_rb / launch_dec_gemv / mm_dispatch: rows = min(16, (64 KiB - 512 B) / (4 K)); the staged-row template
# is 1, 2, 4, 8 or 16 by the first chunk's rows; 3..8 rows take dec_mm when K = 1280, N >= 16, ldw % 8 == 0 and no
# xn_out (WR 8 from N = 16384), else dec_gemv_lds when N <= 16384 and K <= 1536 (2 rows per wave from N = 2560);
# otherwise dec_gemv_kernel with 1 row per wave up to N = 16384, above it the stream kernel (1..2 rows, K <= 1536)
# or 4 (1..2 rows) / 2 rows per wave.  wdtype 0 bf16, 1 f16.
_GEMV_KINDS = [
    # the engine's linears at 3..8 pages, on the fragment-ordered copies (Engine::ensure_mm_weights)
    *[((B, 3840, 1280, 1280, 1, 1, 0, 1), ("dec_mm_wk8_swz", 12)) for B in (3, 4, 5, 8)],   # q/k/v, norm fused
    *[((B, 1280, 1280, 1280, 1, 0, 0, 1), ("dec_mm_wk8_swz", 12)) for B in (3, 8)],         # o_proj
    *[((B, 13696, 1280, 1280, 1, 1, 0, 1), ("dec_mm_wk8_swz", 12)) for B in (3, 8)],        # dense gate|up
    *[((B, 129280, 1280, 1280, 0, 1, 0, 1), ("dec_mm_wr8_swz", 12)) for B in (3, 8)],       # lm_head
    # the same without a copy (DSOCR_MM_SWZ=0, the screened-head tests)
    ((8, 3840, 1280, 1280, 1, 1, 0, 0), ("dec_mm_wk8", 12)), ((3, 129280, 1280, 1280, 0, 1, 0, 0), ("dec_mm_wr8", 12)),
    ((8, 16383, 1280, 1280, 1, 0, 0, 0), ("dec_mm_wk8", 12)), ((8, 16384, 1280, 1280, 1, 0, 0, 0), ("dec_mm_wr8", 12)),
    ((8, 16, 1280, 1288, 0, 0, 0, 0), ("dec_mm_wk8", 12)),
    # one or two pages at the lm_head: the stream kernel, whether or not a copy exists
    ((1, 129280, 1280, 1280, 0, 1, 0, 0), ("dec_gemv_stream", 12)), ((2, 129280, 1280, 1280, 0, 1, 0, 1), ("dec_gemv_stream", 12)),
    ((2, 16400, 256, 256, 0, 0, 0, 0), ("dec_gemv_stream", 16)),
    # outside dec_mm: K, N < 16, a handed-on xn, an unaligned weight pitch, more than 8 rows
    ((8, 896, 1792, 1792, 1, 0, 0, 0), ("dec_gemv_rb1", 9)), ((8, 8, 1280, 1280, 1, 0, 0, 0), ("dec_gemv_lds_r1", 12)),
    ((8, 3840, 1280, 1280, 1, 1, 1, 0), ("dec_gemv_rb1", 12)), ((8, 3840, 1280, 1284, 1, 1, 0, 0), ("dec_gemv_lds_r2", 12)),
    ((9, 3840, 1280, 1280, 1, 1, 0, 0), ("dec_gemv_rb1", 12)), ((13, 3840, 1280, 1280, 1, 1, 0, 1), ("dec_gemv_rb1", 12)),
    # dec_gemv_lds and its rows per wave
    ((4, 200, 512, 512, 0, 0, 0, 0), ("dec_gemv_lds_r1", 16)), ((8, 2600, 256, 256, 0, 1, 0, 0), ("dec_gemv_lds_r2", 16)),
    ((3, 2559, 256, 256, 1, 0, 0, 0), ("dec_gemv_lds_r1", 16)), ((3, 2560, 256, 256, 1, 0, 0, 0), ("dec_gemv_lds_r2", 16)),
    ((5, 16384, 1536, 1536, 1, 0, 0, 0), ("dec_gemv_lds_r2", 10)), ((5, 16384, 1544, 1544, 1, 0, 0, 0), ("dec_gemv_rb1", 10)),
    # dec_gemv_kernel's rows per wave
    ((1, 130, 64, 64, 1, 0, 0, 0), ("dec_gemv_rb1", 16)), ((2, 16384, 256, 256, 0, 0, 0, 0), ("dec_gemv_rb1", 16)),
    ((1, 16400, 1544, 1544, 1, 0, 0, 0), ("dec_gemv_rb4", 10)), ((2, 20000, 1792, 1792, 0, 1, 0, 0), ("dec_gemv_rb4", 9)),
    ((3, 16400, 256, 256, 0, 0, 0, 0), ("dec_gemv_rb2", 16)), ((16, 16400, 64, 64, 0, 0, 0, 0), ("dec_gemv_rb2", 16)),
    ((8, 16385, 1792, 1792, 1, 0, 0, 0), ("dec_gemv_rb2", 9)),
    # the row-chunk loop: the kind is the first chunk's
    ((3, 64, 6848, 6848, 1, 0, 0, 0), ("dec_gemv_rb1", 2)), ((8, 1280, 6848, 6848, 1, 0, 0, 0), ("dec_gemv_rb1", 2)),
    ((21, 513, 128, 128, 0, 1, 0, 0), ("dec_gemv_rb1", 16)), ((21, 16400, 128, 128, 0, 1, 0, 0), ("dec_gemv_rb2", 16)),
    # nothing to launch
    ((0, 1280, 1280, 1280, 1, 0, 0, 0), ("none", 12)), ((4, 0, 1280, 1280, 1, 0, 0, 0), ("none", 12)),
    ((1, 64, 16384, 16384, 1, 0, 0, 0), ("none", 0)),
]


def test_gemv_dispatch_kernel_kinds():
    """Which kernel launch_dec_gemv runs and how many token rows one launch takes (host-only query; the decision the
    launch itself switches on), pinned for the engine's decode linears and every branch of the dispatch."""
    import ctypes as C
    from dsocr._lib import check, lib
    for args, want in _GEMV_KINDS:
        k, r = C.c_char_p(), C.c_int(-1)
        check(lib().dsocr_k_gemv_kind(*args, C.byref(k), C.byref(r)))
        assert (k.value.decode(), r.value) == want, args
    kinds = {w[0] for _, w in _GEMV_KINDS}
    assert kinds >= {"dec_gemv_rb1", "dec_gemv_rb2", "dec_gemv_rb4", "dec_gemv_stream", "dec_gemv_lds_r1", "dec_gemv_lds_r2",
                     "dec_mm_wk8", "dec_mm_wr8", "dec_mm_wk8_swz", "dec_mm_wr8_swz"}
