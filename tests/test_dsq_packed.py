"""Decode MoE from packed Q4_K / Q8_0 snapshot blocks (DSOCR_LOAD_PACKED_EXPERTS, decode_q.hip).

Contract: every weight a packed kernel uses is the fp16 value dequant-on-load stores (oracle/dsq.py's f32
value rounded to fp16), widened to f32; products and sums are f32.  So the decode unpack is checked bit
for bit (one-hot rows through dsocr_k_dsq_rows_dot), the packed layer against the oracle's run_moe fed
the fp16-rounded dequantised weights (1e-4, the bar of test_moe_decode_layer at the same weight scale),
and a packed engine against the oracle reading the same snapshot (greedy ids) and against the same file
loaded dequant-on-load (logits within 2e-3, the bar of test_full_parity.py).
"""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import dsq
from test_dsq import SEED, TINY256, _random_blocks, make_tiny256_snapshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dsocr_engine_load_flags", "dsocr_engine_packed_info", "dsocr_k_moe_packed", "dsocr_k_dsq_rows_dot"]


# ------------------------------------------------------------------ CPU
def test_header_declares_and_library_exports_packed_symbols():
    header = open(os.path.join(ROOT, "include", "dsocr.h")).read()
    declared = set(re.findall(r"\b(dsocr_[a-z0-9_]+)\s*\(", header))
    from dsocr._lib import EXPORTS, LIB_PATH
    assert re.search(r"#define\s+DSOCR_LOAD_PACKED_EXPERTS\s+1u", header)
    L = C.CDLL(LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared and s in EXPORTS, s
        assert hasattr(L, s), s


def test_snapshot_packed_defaults_to_none():
    from dsocr import ModelLoadArgs
    assert ModelLoadArgs().snapshot_packed is None


# ------------------------------------------------------------------ MoE cases (oracle side on the CPU)
MOE_CASES = [(1, 256, 8, 3, 32, 1, True), (2, 512, 16, 6, 96, 2, True), (3, 256, 16, 6, 256, 1, False),
             (8, 256, 8, 3, 32, 1, False), (5, 256, 16, 6, 64, 2, True), (1, 1280, 64, 6, 896, 2, True),
             (8, 1280, 64, 6, 896, 2, True)]


def _qtype_for(in_dim):
    return dsq.Q4K if in_dim % 256 == 0 else dsq.Q8_0


def _payload(rng, rows, in_dim, production):
    """One record's payload: production shapes take random valid blocks of the synthetic snapshot's scale
    (dsocr.synth), the small ones quantise N(0, 0.05) values as make_tiny256_snapshot does."""
    qt = _qtype_for(in_dim)
    if production:
        from dsocr.synth import _q4k_blocks, _q8_0_blocks
        nb = rows * in_dim // dsq.BLOCK[qt]
        return qt, (_q4k_blocks(rng, nb) if qt == dsq.Q4K else _q8_0_blocks(rng, nb)).tobytes()
    return qt, dsq.quantize(qt, (rng.standard_normal((rows, in_dim)) * 0.05).astype(np.float32))


def _deq16(qt, payload, rows, cols):
    return dsq.dequant(qt, payload, rows, cols).astype(np.float16).astype(np.float32)


class _MoeCase:
    def __init__(self, T, H, E, topk, I, ns, norm):
        from oracle.decoder import Decoder, rms_norm, softmax
        self.shape = (T, H, E, topk, I, ns, norm)
        production = H == 1280
        rng = np.random.default_rng(700 + T + H + I)
        Is = I * ns
        self.x = rng.standard_normal((T, H)).astype(np.float32)
        self.router = (rng.standard_normal((E, H)) * 0.1).astype(np.float16)
        self.nw = (1.0 + 0.05 * rng.standard_normal(H)).astype(np.float32)
        self.out0 = rng.standard_normal((T, H)).astype(np.float32)
        rec = {}
        for e in range(E):
            rec[f"l.mlp.experts.{e}.gate_proj.weight"] = (I, H) + _payload(rng, I, H, production)
            rec[f"l.mlp.experts.{e}.up_proj.weight"] = (I, H) + _payload(rng, I, H, production)
            rec[f"l.mlp.experts.{e}.down_proj.weight"] = (H, I) + _payload(rng, H, I, production)
        rec["l.mlp.shared_experts.gate_proj.weight"] = (Is, H) + _payload(rng, Is, H, production)
        rec["l.mlp.shared_experts.up_proj.weight"] = (Is, H) + _payload(rng, Is, H, production)
        rec["l.mlp.shared_experts.down_proj.weight"] = (H, Is) + _payload(rng, H, Is, production)
        self.rec = rec
        router32 = self.router.astype(np.float32)
        cache = {}

        class _W:  # dequantises lazily: only the experts the oracle routes to
            def get(self, n, shape=None):
                n = n.replace("model.layers.1.", "l.")
                if n == "l.mlp.gate.weight":
                    return router32
                if n not in cache:
                    rows, cols, qt, payload = rec[n]
                    cache[n] = _deq16(qt, payload, rows, cols)
                return cache[n]

            def has(self, n):
                n = n.replace("model.layers.1.", "l.")
                return n == "l.mlp.gate.weight" or n in rec

        dec = Decoder.__new__(Decoder)
        dec.W = _W()
        dec.H = H

        class _L:
            n_routed_experts, num_experts_per_tok, moe_intermediate_size = E, topk, I
            topk_method, scoring_func, norm_topk_prob, routed_scaling_factor, n_shared_experts = \
                "greedy", "softmax", False, 1.0, ns
        dec.lang = _L()
        xin = rms_norm(self.x, self.nw, 1e-6) if norm else self.x
        self.ref = dec.moe(1, xin) + self.out0
        self.scores = softmax(xin @ router32.T)
        self.order = np.argsort(-self.scores, axis=-1, kind="stable")[:, :topk]


_moe_cache = {}


def _moe_case(case):
    if case not in _moe_cache:
        _moe_cache[case] = _MoeCase(*case)
    return _moe_cache[case]


@pytest.mark.parametrize("case", MOE_CASES)
def test_moe_oracle_side_is_usable(case):
    """The oracle output of every case is finite and its routing has no exact ties."""
    c = _moe_case(case)
    assert np.isfinite(c.ref).all()
    for t in range(case[0]):
        assert len(np.unique(c.scores[t])) == case[2], t


# ------------------------------------------------------------------ GPU: unpack, layer, errors
@pytest.mark.gpu
@pytest.mark.parametrize("qtype,rows,cols", [(dsq.Q4K, 37, 256), (dsq.Q4K, 5, 1280), (dsq.Q8_0, 37, 96),
                                             (dsq.Q8_0, 3, 896)])
def test_decode_unpack_bit_exact(gpu, qtype, rows, cols):
    from _dev import Dev
    from dsocr._lib import check, lib
    rng = np.random.default_rng(300 + qtype + cols)
    raw = _random_blocks(rng, qtype, rows * cols // dsq.BLOCK[qtype])
    ref = dsq.dequant(qtype, raw, rows, cols).astype(np.float16).astype(np.float32).view(np.uint32)
    src = Dev(np.frombuffer(raw, np.uint8))
    T = 8
    assert cols % T == 0
    for c0 in range(0, cols, T):
        x = np.zeros((T, cols), np.float32)
        x[np.arange(T), c0 + np.arange(T)] = 1.0
        dx, dy = Dev(x), Dev.zeros((T, rows), np.float32)
        check(lib().dsocr_k_dsq_rows_dot(qtype, rows, cols, src.ptr, T, dx.ptr, dy.ptr))
        got = dy.get().view(np.uint32)  # got[t][r] = W[r][c0 + t]
        assert np.array_equal(got.T, ref[:, c0:c0 + T]), (c0, np.argwhere(got.T != ref[:, c0:c0 + T])[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("case", MOE_CASES)
def test_moe_packed_matches_oracle(gpu, case):
    from _dev import Dev
    from dsocr._lib import check, lib
    T, H, E, topk, I, ns, norm = case
    Is = I * ns
    c = _moe_case(case)
    cat = lambda names: np.frombuffer(b"".join(c.rec[n][3] for n in names), np.uint8)
    gu = cat([f"l.mlp.experts.{e}.{p}_proj.weight" for e in range(E) for p in ("gate", "up")])
    dn = cat([f"l.mlp.experts.{e}.down_proj.weight" for e in range(E)])
    sgu = cat(["l.mlp.shared_experts.gate_proj.weight", "l.mlp.shared_experts.up_proj.weight"])
    sd = cat(["l.mlp.shared_experts.down_proj.weight"])
    dx, dr, dgu, ddn, dsgu, dsd = Dev(c.x), Dev(c.router.view(np.uint16)), Dev(gu), Dev(dn), Dev(sgu), Dev(sd)
    dnw, dout = Dev(c.nw), Dev(c.out0)
    ids = np.zeros(T * topk, np.int32)
    wts = np.zeros(T * topk, np.float32)
    check(lib().dsocr_k_moe_packed(T, H, E, topk, I, Is, dx.ptr, dnw.ptr if norm else None, 1e-6, dr.ptr,
                                   _qtype_for(H), dgu.ptr, _qtype_for(I), ddn.ptr, _qtype_for(H), dsgu.ptr,
                                   _qtype_for(Is), dsd.ptr, 0, 1.0, dout.ptr, ids.ctypes.data_as(C.c_void_p),
                                   wts.ctypes.data_as(C.c_void_p)))
    assert np.array_equal(ids.reshape(T, topk), c.order)
    err = float(np.max(np.abs(dout.get() - c.ref)))
    print(f"moe_packed {case}: max abs err {err:.3e}")
    assert err < 1e-4, err


@pytest.mark.gpu
def test_packed_hooks_reject_bad_arguments(gpu):
    from _dev import Dev
    from dsocr._lib import DsocrError, check, lib
    buf = Dev(np.zeros(1 << 16, np.uint8))
    x, y = Dev.zeros((8, 256), np.float32), Dev.zeros((8, 4), np.float32)
    with pytest.raises(DsocrError, match="EINVAL"):  # Q6_K
        check(lib().dsocr_k_dsq_rows_dot(dsq.Q6K, 4, 256, buf.ptr, 8, x.ptr, y.ptr))
    with pytest.raises(DsocrError, match="EINVAL"):  # Q4_K rows of 96
        check(lib().dsocr_k_dsq_rows_dot(dsq.Q4K, 4, 96, buf.ptr, 8, x.ptr, y.ptr))
    with pytest.raises(DsocrError, match="EINVAL"):  # Q8_0 rows of 40
        check(lib().dsocr_k_dsq_rows_dot(dsq.Q8_0, 4, 40, buf.ptr, 8, x.ptr, y.ptr))
    ids, wts = np.zeros(8, np.int32), np.zeros(8, np.float32)
    out = Dev.zeros((1, 256), np.float32)

    def moe(gu_qt, d_qt, I):
        return lib().dsocr_k_moe_packed(1, 256, 8, 3, I, 0, x.ptr, None, 1e-6, buf.ptr, gu_qt, buf.ptr, d_qt, buf.ptr,
                                        0, None, 0, None, 0, 1.0, out.ptr, ids.ctypes.data_as(C.c_void_p),
                                        wts.ctypes.data_as(C.c_void_p))
    with pytest.raises(DsocrError, match="EINVAL"):
        check(moe(dsq.Q6K, dsq.Q8_0, 32))
    with pytest.raises(DsocrError, match="EINVAL"):
        check(moe(dsq.Q4K, dsq.Q6K, 256))
    with pytest.raises(DsocrError, match="EINVAL"):  # down in_dim 48 is no whole Q8_0 block count
        check(moe(dsq.Q4K, dsq.Q8_0, 48))


# ------------------------------------------------------------------ GPU: engine
N_NEW = 24


def _write_snapshot(path, cfg, choose):
    """Quantised from the seeded synthetic weights as make_tiny256_snapshot does; choose(name, in_dim) -> qtype."""
    from oracle.weights import Weights
    base = Weights(seed=SEED, dtype="f32")
    tensors = []
    for name, out_dim, in_dim, bias in dsq.discover_linears(cfg):
        w = base.get(name, (out_dim, in_dim))
        qt = choose(name, in_dim)
        b = base.get(bias, (out_dim,)) if bias and base.has(bias) else None
        tensors.append((name, out_dim, in_dim, qt, dsq.quantize(qt, w), b))
    dsq.write_dsq(path, tensors, default_qdtype=dsq.Q4K)


def _all_q4k(name, in_dim):
    if name == "lm_head.weight" or name.startswith("model.projector"):
        return dsq.Q8_0
    return dsq.Q4K if in_dim % 256 == 0 else dsq.Q8_0


def _text_prompts(n):
    rng = np.random.default_rng(21)
    return [rng.integers(16, 500, int(rng.integers(5, 14))).astype(np.int64) for _ in range(n)]


def _check_engine(cfg_path, cfg, snap, batches, page_too):
    """Greedy ids of a packed engine vs the oracle reading the same file (an image page when page_too, and text
    batches of the given sizes), and generate_trace logits vs the same file loaded dequant-on-load."""
    from dsocr import DecodeParameters, ModelLoadArgs, Page, VisionSettings, build_prompt_tokens, load_model
    from dsocr.synth import SyntheticTokenizer
    from oracle.model import OracleModel
    from oracle.weights import Weights
    params = DecodeParameters(max_new_tokens=N_NEW)
    prompts = _text_prompts(max(batches))
    got, trace = {}, {}
    for packed in (True, False):
        eng = load_model(ModelLoadArgs(config_path=cfg_path, synthetic_seed=SEED, dtype="f16", snapshot_path=snap,
                                       snapshot_packed=packed))
        try:
            info = eng.packed_info()
            if packed:
                assert info["moe_layers"] > 0 and info["packed_layers"] == info["moe_layers"], info
                assert info["packed_bytes"] > 0
                if page_too:
                    img = np.random.default_rng(5).integers(0, 256, (300, 260, 3), dtype=np.uint8)
                    page = Page(img, VisionSettings(256, 128, True))
                    pids, pmask = build_prompt_tokens(SyntheticTokenizer(512), "<image>\nConvert the document to markdown.",
                                                      [page.n_image_tokens])
                    got["page"] = eng.generate(pids, pmask, page, None, params)
                for n in batches:
                    got[n] = eng.generate_batch([(p, None, None, None) for p in prompts[:n]], params, ignore_eos=True)
            else:
                assert info["packed_layers"] == 0
            for n in batches:
                trace[(packed, n)] = eng.generate_trace([(p, None, None, None) for p in prompts[:n]], params,
                                                        ignore_eos=True)
        finally:
            eng.close()
    oracle = OracleModel(cfg, Weights(seed=SEED, dtype="f16", snapshot=dsq.Snapshot(snap)))
    if page_too:
        emb, _ = oracle.image_embeddings(img, 256, 128, True)
        ref, _ = oracle.generate(pids, pmask, emb, N_NEW, eos_token_id=1, no_repeat_ngram_size=20)
        assert got["page"] == ref
    refs = [oracle.generate(p, np.zeros(len(p), np.uint8), None, N_NEW, eos_token_id=None, ignore_eos=True)[0]
            for p in prompts]
    for n in batches:
        for i in range(n):
            assert got[n][i] == refs[i], (n, i, got[n][i], refs[i])
        (ids_p, lg_p), (ids_u, lg_u) = trace[(True, n)], trace[(False, n)]
        assert ids_p == ids_u
        err = float(np.max(np.abs(np.asarray(lg_p) - np.asarray(lg_u))))
        print(f"packed vs dequant-on-load logits, {n} prompt(s): max abs diff {err:.3e}")
        assert err < 2e-3, (n, err)


@pytest.fixture(scope="module")
def q4k_snap(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("dsqp") / "tiny256_q4k.dsq")
    _write_snapshot(p, json.load(open(TINY256)), _all_q4k)
    return p


@pytest.mark.gpu
def test_packed_engine_q4k(gpu, q4k_snap):
    _check_engine(TINY256, json.load(open(TINY256)), q4k_snap, (3, 8), page_too=True)


@pytest.mark.gpu
def test_packed_engine_q8_0_down(gpu, tmp_path):
    """moe_intermediate_size 96: routed down in_dim 96 and shared down in_dim 192 are Q8_0."""
    cfg = json.load(open(TINY256))
    cfg["language_config"]["moe_intermediate_size"] = 96
    cfg_path = str(tmp_path / "tiny256_i96.json")
    json.dump(cfg, open(cfg_path, "w"))
    snap = str(tmp_path / "tiny256_i96.dsq")
    _write_snapshot(snap, cfg, _all_q4k)
    s = dsq.Snapshot(snap)
    assert s.records["model.layers.1.mlp.experts.0.down_proj.weight"]["q_dtype"] == dsq.Q8_0
    assert s.records["model.layers.1.mlp.shared_experts.down_proj.weight"]["q_dtype"] == dsq.Q8_0
    assert s.records["model.layers.1.mlp.experts.0.gate_proj.weight"]["q_dtype"] == dsq.Q4K
    _check_engine(cfg_path, cfg, snap, (1, 8), page_too=False)


@pytest.mark.gpu
def test_packed_fallback_and_switches(gpu, q4k_snap, tmp_path):
    from dsocr import DecodeParameters, DsocrError, ModelLoadArgs, load_model
    from oracle.model import OracleModel
    from oracle.weights import Weights
    cfg = json.load(open(TINY256))
    params = DecodeParameters(max_new_tokens=N_NEW)
    prompt = _text_prompts(1)[0]
    req = [(prompt, None, None, None)]
    # a Q6_K-mixed snapshot: no layer qualifies, the fp16 kernels run
    mixed = str(tmp_path / "mixed.dsq")
    make_tiny256_snapshot(mixed)
    eng = load_model(ModelLoadArgs(config_path=TINY256, synthetic_seed=SEED, dtype="f16", snapshot_path=mixed,
                                   snapshot_packed=True))
    try:
        assert eng.packed_info()["packed_layers"] == 0
        got = eng.generate_batch(req, params, ignore_eos=True)[0]
    finally:
        eng.close()
    oracle = OracleModel(cfg, Weights(seed=SEED, dtype="f16", snapshot=dsq.Snapshot(mixed)))
    assert got == oracle.generate(prompt, np.zeros(len(prompt), np.uint8), None, N_NEW, eos_token_id=None, ignore_eos=True)[0]
    # the flag without a snapshot
    with pytest.raises(DsocrError, match="EINVAL"):
        load_model(ModelLoadArgs(config_path=TINY256, synthetic_seed=SEED, dtype="f16", snapshot_packed=True))
    # the environment switch through dsocr_engine_load, in a fresh process
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from dsocr import ModelLoadArgs, load_model\n"
            "e = load_model(ModelLoadArgs(config_path=%r, synthetic_seed=%d, dtype='f16', snapshot_path=%r))\n"
            "print('PACKED_LAYERS', e.packed_info()['packed_layers']); e.close()\n"
            % (ROOT, os.path.join(ROOT, "deepseek-ocr.rs_amd"), TINY256, SEED, q4k_snap))
    for env_val, want in (("1", True), (None, False)):
        env = dict(os.environ)
        env.pop("DSOCR_DSQ_PACKED", None)
        if env_val:
            env["DSOCR_DSQ_PACKED"] = env_val
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        n = int(re.search(r"PACKED_LAYERS (\d+)", r.stdout).group(1))
        assert (n > 0) == want, (env_val, n)
    # profile_decode: packed kernel names, fewer MoE bytes than the fp16 engine on the same prompt
    prof = {}
    for packed in (True, False):
        eng = load_model(ModelLoadArgs(config_path=TINY256, synthetic_seed=SEED, dtype="f16", snapshot_path=q4k_snap,
                                       snapshot_packed=packed))
        try:
            eng.generate_batch(req, params, ignore_eos=True)
            prof[packed] = eng.profile_decode(2)
        finally:
            eng.close()
    assert prof[True]["moe_gateup_kernel"] == "moe_gateup_q_kernel" and prof[True]["moe_down_kernel"] == "moe_down_q_kernel"
    assert prof[False]["moe_gateup_kernel"] != "moe_gateup_q_kernel"
    for k in ("moe_gateup", "moe_down"):
        assert prof[True][k]["bytes"] < prof[False][k]["bytes"], (k, prof[True][k], prof[False][k])
    assert prof[True]["moe_gateup"]["bytes"] + prof[True]["moe_down"]["bytes"] < \
        prof[False]["moe_gateup"]["bytes"] + prof[False]["moe_down"]["bytes"]
