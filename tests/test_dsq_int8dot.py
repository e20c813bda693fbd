"""Integer-dot decode MoE from packed Q4_K / Q8_0 blocks (DSOCR_LOAD_PACKED_INT8_DOT, decode_qdot.hip).

Contract: activations quantised to Q8_K (for Q4_K rows) or Q8_0 (for Q8_0 rows) as the
ggml reference quantisers do, int32 block dots, f32 sums over blocks.  The quantiser is checked bit for bit
against a numpy f32 restatement, the row dots against an f64 sum over the same codes, the layer against the f64
layer computed from the codes the launches returned, the engine for its modes and finite, in-vocabulary output.
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
from test_dsq import SEED, TINY256, _random_blocks
from test_dsq_packed import MOE_CASES, N_NEW, ROOT, _all_q4k, _moe_case, _qtype_for, _text_prompts, _write_snapshot

pytestmark = pytest.mark.gpu
f32 = np.float32
# largest |y - ref| / sum |d_x q8 W| of test_rows_dot: measured 3.53e-8 (the f32 sum over <= 5 super-blocks, or
# <= 28 Q8_0 blocks, against the f64 reference); 10x for other sum orders
ROWS_DOT_REL = 3.53e-7


def q8_ref(kind, x):
    """The contract's quantisers in numpy f32: codes, d, bs (Q8_K only) and the products that were rounded."""
    T = x.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == dsq.Q4K:
            b = x.reshape(T, -1, 256)
            mx = np.take_along_axis(b, np.argmax(np.abs(b), axis=-1)[..., None], -1)[..., 0]  # first on ties
            iscale = np.where(mx != 0, f32(-128) / mx, f32(0)).astype(f32)
            p = iscale[..., None] * b
            q = np.minimum(127, np.rint(p)).astype(np.int8)
            d = np.where(mx != 0, f32(1) / iscale, f32(0)).astype(f32)
            bs = q.reshape(T, -1, 32).sum(-1, dtype=np.int32).astype(np.int16)
        else:
            b = x.reshape(T, -1, 32)
            d = np.abs(b).max(-1) / f32(127)
            inv = np.where(d != 0, f32(1) / d, f32(0)).astype(f32)
            p = b * inv[..., None]
            q = (np.sign(p) * np.floor(np.abs(p.astype(np.float64)) + 0.5)).astype(np.int8)  # roundf
            d, bs = d.astype(np.float16).astype(f32), None
    return q.reshape(x.shape), d, bs, p.reshape(x.shape)


def _dequant_codes(kind, q, d):
    blk = 256 if kind == dsq.Q4K else 32
    return (q.reshape(q.shape[0], -1, blk).astype(np.float64) * d.astype(np.float64)[..., None]).reshape(q.shape)


def _planted(kind, T, in_dim, plant):
    x = np.random.default_rng(40 + in_dim + T).standard_normal((T, in_dim)).astype(f32)
    top = 128.0 if kind == dsq.Q4K else 127.0  # makes iscale (Q8_K: -128 / -128) or 1 / d (Q8_0) exactly 1
    if plant == "zero":
        x[0, :32] = 0.0
        if kind == dsq.Q4K:
            x[0, :256] = 0.0
    elif plant == "negmax":
        x[0, 4] = -7.0
    elif plant == "tie":
        x[0, 3], x[0, 9] = 5.0, -5.0
    else:  # exact .5 products: half-even for Q8_K (2.5 -> 2, 3.5 -> 4, 127.5 -> 128 -> 127), half away for Q8_0
        x[0, :12] = [-top, 0.25, -0.25, 1.0, 2.0, 2.5, 3.5, -0.5, top - 0.5, -2.5, 0.5, 1.5]
    return x


@pytest.mark.parametrize("kind,T,in_dim", [(dsq.Q4K, 1, 256), (dsq.Q4K, 3, 1280), (dsq.Q8_0, 1, 32), (dsq.Q8_0, 3, 896)])
def test_quantiser_bit_exact(gpu, kind, T, in_dim):
    from _dev import Dev
    from dsocr._lib import check, lib
    for plant in ("zero", "negmax", "tie", "half"):
        x = _planted(kind, T, in_dim, plant)
        q, d, bs, _ = q8_ref(kind, x)
        dx, dq, dd = Dev(x), Dev.zeros(x.shape, np.int8), Dev.zeros(d.shape, f32)
        dbs = Dev.zeros((T, in_dim // 32), np.int16)
        check(lib().dsocr_k_q8_quantize(kind, T, in_dim, dx.ptr, dq.ptr, dd.ptr, dbs.ptr))
        assert np.array_equal(dq.get(), q), (plant, np.argwhere(dq.get() != q)[:5])
        assert np.array_equal(dd.get().view(np.uint32), d.view(np.uint32)), plant
        if bs is not None:
            assert np.array_equal(dbs.get(), bs), plant


ROWS = [(dsq.Q4K, 37, 256), (dsq.Q4K, 5, 1280), (dsq.Q8_0, 37, 96), (dsq.Q8_0, 3, 896)]


def _rows_dot(qtype, rows, cols, src, q, d, bs):
    from _dev import Dev
    from dsocr._lib import check, lib
    T = q.shape[0]
    dy = Dev.zeros((T, rows), f32)
    dq, dd, dbs = Dev(q), Dev(d), Dev(bs if bs is not None else np.zeros(1, np.int16))
    check(lib().dsocr_k_dsq_rows_dot_q8(qtype, rows, cols, src.ptr, T, dq.ptr, dd.ptr, dbs.ptr, dy.ptr))
    return dy.get()


@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("qtype,rows,cols", ROWS)
def test_rows_dot(gpu, qtype, rows, cols, T):
    from _dev import Dev
    rng = np.random.default_rng(300 + qtype + cols)
    raw = _random_blocks(rng, qtype, rows * cols // dsq.BLOCK[qtype])
    W = dsq.dequant(qtype, raw, rows, cols).astype(np.float64)
    q, d, bs, _ = q8_ref(qtype, rng.standard_normal((T, cols)).astype(f32))
    xq = _dequant_codes(qtype, q, d)
    got = _rows_dot(qtype, rows, cols, Dev(np.frombuffer(raw, np.uint8)), q, d, bs)
    rel = float(np.max(np.abs(got - xq @ W.T) / (np.abs(xq) @ np.abs(W).T)))
    print(f"rows_dot_q8 {(qtype, rows, cols, T)}: max err / sum |d_x q8 W| = {rel:.3e}")
    assert rel < ROWS_DOT_REL, rel


@pytest.mark.parametrize("qtype,rows,cols", ROWS)
def test_rows_dot_one_hot(gpu, qtype, rows, cols):
    """q8 = 1 at one column, d_x = 1: the row dot is d_w sc q - dmin_w m (Q4_K) or d_w q (Q8_0), within one f32
    ulp at the magnitude of the larger of the two products and the result (each product rounds once)."""
    from _dev import Dev
    rng = np.random.default_rng(300 + qtype + cols)
    raw = _random_blocks(rng, qtype, rows * cols // dsq.BLOCK[qtype])
    src = Dev(np.frombuffer(raw, np.uint8))
    blk = np.frombuffer(raw, np.uint8).reshape(rows, -1, dsq.BLOCK_BYTES[qtype])
    if qtype == dsq.Q4K:  # the two products, exact in f64
        dw, dmin = (blk[..., o:o + 2].copy().view("<f2")[..., 0].astype(np.float64) for o in (0, 2))
        sc, m = (np.stack([dsq._scale_min_k4(blk.reshape(-1, 144)[:, 4:16], j)[i] for j in range(8)], -1)
                 .reshape(rows, -1, 8).astype(np.float64) for i in (0, 1))
        qs = blk[..., 16:].reshape(rows, -1, 4, 32)
        nib = np.concatenate([qs & 0xF, qs >> 4], -1).reshape(rows, -1, 8, 32).astype(np.float64)
        a = (dw[..., None] * sc)[..., None] * nib
        b = np.broadcast_to((dmin[..., None] * m)[..., None], a.shape)
    else:
        dw = blk[..., 0:2].copy().view("<f2")[..., 0].astype(np.float64)
        a = dw[..., None] * blk[..., 2:].view(np.int8).astype(np.float64)
        b = np.zeros_like(a)
    a, b = a.reshape(rows, cols), b.reshape(rows, cols)
    ulp = np.spacing(np.maximum(np.maximum(np.abs(a), np.abs(b)), np.abs(a - b)).astype(f32)).astype(np.float64)
    nb = cols // dsq.BLOCK[qtype]
    worst = 0.0
    for c0 in range(0, cols, 8):
        q = np.zeros((8, cols), np.int8)
        q[np.arange(8), c0 + np.arange(8)] = 1
        bs = q.reshape(8, -1, 32).sum(-1).astype(np.int16) if qtype == dsq.Q4K else None
        got = _rows_dot(qtype, rows, cols, src, q, np.ones((8, nb), f32), bs).T.astype(np.float64)
        worst = max(worst, float(np.max(np.abs(got - (a - b)[:, c0:c0 + 8]) / ulp[:, c0:c0 + 8])))
    print(f"one-hot {(qtype, rows, cols)}: worst error {worst:.3f} ulp")
    assert worst <= 1.0, worst


def _codes_match(kind, got, x_ref, what):
    """got == the reference quantiser of x_ref, but for products within 1e-3 of a rounding boundary (+-1 there);
    the reference alone puts at most 1 % of the elements in that band."""
    q, _, _, p = q8_ref(kind, x_ref.astype(f32))
    frac = np.abs(p - np.floor(p))
    edge = np.abs(frac - 0.5) < 1e-3
    assert edge.mean() <= 0.01, (what, edge.mean())
    diff = np.abs(got.astype(np.int32) - q.astype(np.int32))
    assert diff[~edge].max(initial=0) == 0 and diff.max(initial=0) <= 1, (what, np.argwhere(diff > 0)[:5])


@pytest.mark.parametrize("case", [c for c in MOE_CASES if c[1] != 1280] + [(3, 1280, 64, 6, 896, 2, True)])
def test_moe_layer(gpu, case):
    from _dev import Dev
    from dsocr._lib import check, lib
    from oracle.decoder import rms_norm
    T, H, E, topk, I, ns, norm = case
    Is, TK = I * ns, T * topk
    c = _moe_case(case)
    cat = lambda names: np.frombuffer(b"".join(c.rec[n][3] for n in names), np.uint8)
    dgu = Dev(cat([f"l.mlp.experts.{e}.{p}_proj.weight" for e in range(E) for p in ("gate", "up")]))
    ddn = Dev(cat([f"l.mlp.experts.{e}.down_proj.weight" for e in range(E)]))
    dsgu = Dev(cat(["l.mlp.shared_experts.gate_proj.weight", "l.mlp.shared_experts.up_proj.weight"]))
    dsd = Dev(cat(["l.mlp.shared_experts.down_proj.weight"]))
    dx, dr, dnw, dout = Dev(c.x), Dev(c.router.view(np.uint16)), Dev(c.nw), Dev(c.out0)
    kx, kh, khs = _qtype_for(H), _qtype_for(I), _qtype_for(Is)
    nb = lambda k, n: n // dsq.BLOCK[k]
    ids, wts = np.zeros((T, topk), np.int32), np.zeros((T, topk), f32)
    xq, xd = np.zeros((T, H), np.int8), np.zeros((T, nb(kx, H)), f32)
    hq, hd = np.zeros((TK, I), np.int8), np.zeros((TK, nb(kh, I)), f32)
    sq, sd = np.zeros((T, Is), np.int8), np.zeros((T, nb(khs, Is)), f32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    check(lib().dsocr_k_moe_packed_q8(T, H, E, topk, I, Is, dx.ptr, dnw.ptr if norm else None, 1e-6, dr.ptr, kx, dgu.ptr,
                                      kh, ddn.ptr, kx, dsgu.ptr, khs, dsd.ptr, 0, 1.0, dout.ptr, vp(ids), vp(wts),
                                      vp(xq), vp(xd), vp(hq), vp(hd), vp(sq), vp(sd)))
    assert np.array_equal(ids, c.order)
    _codes_match(kx, xq, rms_norm(c.x, c.nw, 1e-6) if norm else c.x, "xn")
    # the f64 layer from the returned codes
    W = lambda n: dsq.dequant(c.rec[n][2], c.rec[n][3], c.rec[n][0], c.rec[n][1]).astype(np.float64)
    silu_mul = lambda g, u: g / (1.0 + np.exp(-g)) * u
    xn = _dequant_codes(kx, xq, xd)
    h = np.stack([silu_mul(W(f"l.mlp.experts.{e}.gate_proj.weight") @ xn[t], W(f"l.mlp.experts.{e}.up_proj.weight") @ xn[t])
                  * float(wts[t, k]) for t in range(T) for k, e in enumerate(ids[t])])
    hs = silu_mul(xn @ W("l.mlp.shared_experts.gate_proj.weight").T, xn @ W("l.mlp.shared_experts.up_proj.weight").T)
    _codes_match(kh, hq, h, "h")
    _codes_match(khs, sq, hs, "hs")
    hdq = _dequant_codes(kh, hq, hd)
    ref = c.out0.astype(np.float64) + _dequant_codes(khs, sq, sd) @ W("l.mlp.shared_experts.down_proj.weight").T
    for t in range(T):
        for k, e in enumerate(ids[t]):
            ref[t] += W(f"l.mlp.experts.{e}.down_proj.weight") @ hdq[t * topk + k]
    err = float(np.max(np.abs(dout.get() - ref)))
    print(f"moe_packed_q8 {case}: max abs err {err:.3e}; vs the fp16 oracle {float(np.max(np.abs(dout.get() - c.ref))):.3e}")
    assert err < 1e-4, err


CHILD = ("import sys; sys.path[:0] = [%r, %r]\n"
         "import numpy as np\n"
         "from dsocr import DecodeParameters, ModelLoadArgs, load_model\n"
         "e = load_model(ModelLoadArgs(config_path=%r, synthetic_seed=%d, dtype='f16', snapshot_path=%r))\n"
         "ids = e.generate_batch([(np.array(%r, np.int64), None, None, None)], DecodeParameters(max_new_tokens=%d), ignore_eos=True)\n"
         "print('MODE', e.packed_mode(), 'IDS', [int(t) for t in ids[0]]); e.close()\n")


def test_engine_modes(gpu, tmp_path):
    from dsocr import DecodeParameters, DsocrError, ModelLoadArgs, load_model
    snap = str(tmp_path / "tiny256_q4k.dsq")
    cfg = json.load(open(TINY256))
    _write_snapshot(snap, cfg, _all_q4k)
    vocab = cfg["language_config"]["vocab_size"]
    params = DecodeParameters(max_new_tokens=N_NEW)
    prompts = _text_prompts(3)
    ids, logits = {}, {}
    for packed, mode in (("int8", 2), (True, 1), (False, 0)):
        eng = load_model(ModelLoadArgs(config_path=TINY256, synthetic_seed=SEED, dtype="f16", snapshot_path=snap,
                                       snapshot_packed=packed))
        try:
            assert eng.packed_mode() == mode
            for n in (1, 3):
                ids[mode, n], logits[mode, n] = eng.generate_trace([(p, None, None, None) for p in prompts[:n]], params,
                                                                   ignore_eos=True)
            if mode == 2:
                assert eng.packed_info()["packed_layers"] == eng.packed_info()["moe_layers"] > 0
                eng.generate_batch([(prompts[0], None, None, None)], params, ignore_eos=True)
                prof = eng.profile_decode(2)
                assert (prof["moe_gateup_kernel"], prof["moe_down_kernel"]) == ("moe_gateup_qdot_kernel", "moe_down_qdot_kernel")
        finally:
            eng.close()
    for n in (1, 3):
        lg = np.asarray(logits[2, n])
        assert all(0 <= t < vocab for seq in ids[2, n] for t in seq) and np.isfinite(lg).all()
        print(f"int8-dot vs dequant-on-load logits, {n} page(s): max abs diff {float(np.max(np.abs(lg - np.asarray(logits[0, n])))):.3e}")
        assert ids[1, n] == ids[0, n]
    with pytest.raises(DsocrError, match="EINVAL"):  # the flag without a snapshot
        load_model(ModelLoadArgs(config_path=TINY256, synthetic_seed=SEED, dtype="f16", snapshot_packed="int8"))
    # the environment switches through dsocr_engine_load, each in a fresh process
    code = CHILD % (ROOT, os.path.join(ROOT, "deepseek-ocr.rs_amd"), TINY256, SEED, snap, [int(t) for t in prompts[0]], N_NEW)
    for var, mode in (("DSOCR_DSQ_INT8", 2), ("DSOCR_DSQ_PACKED", 1), (None, 0)):
        env = {k: v for k, v in os.environ.items() if k not in ("DSOCR_DSQ_INT8", "DSOCR_DSQ_PACKED")}
        if var:
            env[var] = "1"
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        got = re.search(r"MODE (\d) IDS (\[.*\])", r.stdout)
        assert int(got.group(1)) == mode, (var, r.stdout)
        if mode == 1:
            assert json.loads(got.group(2)) == [int(t) for t in ids[1, 1][0]], var
