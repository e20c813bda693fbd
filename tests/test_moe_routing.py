"""Every MoE routing implementation under every scoring variant and under exact ties.

The engine restates the reference's router (block.rs:1243-1301: logits (+ e_score_correction_bias) -> softmax or
sigmoid scores -> stable descending sort -> top-k -> optional renormalise (+1e-20) -> routed scaling) seven times:
the prefill's router_topk / moe_group / moe_combine kernels and six decode forms that launch_moe_decode picks by
token count and expert count (dsocr_k_moe_route_kind names the one a shape reaches).  Each is run here against a
plain numpy float64 reference:

  1. router logits within the suite's GEMV bound (test_gpu_kernels._bound) of the f64 logits, bias included;
  2. duplicated router rows give bit-identical logit columns;
  3. picked expert ids equal the reference's (ties keep the lower expert id);
  4. routing weights equal the reference routing applied in f64 to the returned logits, relative 1e-5
     (a few f32 ulp of expf, the sum and the divide);
  5. the layer output within 1e-4 * max(1, scaling) (the bar of test_moe_decode_layer at this weight scale; the
     routed term is linear in the scaling).

Margin rule (a condition on the inputs, asserted on the CPU by test_margin_rule_*): any two f32-rounded reference
scores of one token are an intended exact tie or differ by more than 1e-4 relative; no logit lies in (20, 30); every
logit outside the +40 saturation experts has |logit| <= 10.  The inputs are made to satisfy it by drawing: a token
row that breaks the rule is drawn again from the case's seeded stream until it holds, so every token of every case
is kept and checked.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from _dev import Dev, bf16_round, write_bf16_safetensors
from dsocr._lib import EINVAL, check, lib
from test_gpu_kernels import _bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, "deepseek-ocr.rs_amd", "dsocr", "configs", "tiny.json")
NEW_SYMBOLS = ["dsocr_k_moe_ex", "dsocr_k_moe_route_kind", "dsocr_k_moe_prefill_route", "dsocr_k_moe_combine"]
F64 = np.float64

# (name, softmax_scoring, norm_topk, scaling, bias)
VARIANTS = [("softmax", 1, 0, 1.0, False), ("softmax_norm_scale_bias", 1, 1, 2.5, True),
            ("sigmoid", 0, 0, 1.0, False), ("sigmoid_norm_scale_bias", 0, 1, 2.5, True)]
VARIANT = {v[0]: v for v in VARIANTS}
FUSED_OFF = {"DSOCR_ROUTE_FUSED": "0"}
# (routing kind, (T, H, E, topk, I, n_shared, fused norm), environment): the smallest shapes that reach each form
DECODE_SHAPES = [
    ("moe_gateup_mix", (1, 256, 16, 6, 64, 2, True), None),
    ("moe_gateup_mix", (1, 256, 64, 8, 32, 1, True), None),
    ("moe_gateup_mix", (1, 256, 5, 5, 32, 1, True), None),       # topk == E
    ("moe_gateup_slot", (2, 256, 16, 6, 64, 2, True), None),
    ("moe_gateup_slot", (1, 256, 96, 6, 32, 1, True), None),     # one token, more than 64 experts
    ("dec_route_grp", (3, 256, 16, 6, 64, 2, False), None),
    ("dec_route_grp", (8, 256, 64, 8, 32, 1, False), None),      # T * topk = 64
    ("dec_route_grp", (5, 640, 16, 6, 32, 1, True), FUSED_OFF),
    ("moe_gateup_mm", (5, 640, 16, 6, 32, 1, True), None),       # the router inside gate/up
    ("moe_gateup_mm", (8, 640, 64, 8, 32, 1, True), None),
    ("dec_router", (4, 256, 96, 6, 32, 1, False), None),
    ("dec_router", (8, 256, 256, 8, 32, 1, True), None),
    ("moe_route", (9, 128, 8, 3, 32, 1, False), None),
    ("moe_route", (17, 128, 96, 6, 32, 1, True), None),
    ("moe_route", (64, 128, 256, 8, 32, 1, True), None),         # T * topk = 512
]
ROUTE_KINDS = ["moe_gateup_mix", "moe_gateup_slot", "dec_route_grp", "moe_gateup_mm", "dec_router", "moe_route"]
TOPK1_SHAPE = ("dec_route_grp", (3, 256, 16, 1, 64, 2, False), None)
TIES = ["interior", "boundary_hi", "boundary_lo", "saturation"]


def _shape_id(kind, shape, env):
    return f"{kind}-{'x'.join(str(int(v)) for v in shape)}" + ("-fused0" if env else "")


def _decode_params():
    out = []
    for kind, shape, env in DECODE_SHAPES:
        for v in VARIANTS:
            out.append(pytest.param(kind, shape, env, v[0], None, id=f"{_shape_id(kind, shape, env)}-{v[0]}"))
    out.append(pytest.param(*TOPK1_SHAPE, "softmax_norm_scale_bias", None, id=_shape_id(*TOPK1_SHAPE) + "-topk1-norm"))
    out.append(pytest.param(*TOPK1_SHAPE, "sigmoid_norm_scale_bias", None,
                            id=_shape_id(*TOPK1_SHAPE) + "-topk1-norm-sigmoid"))
    return out


def _tie_params():
    out = []
    for kind, shape, env in DECODE_SHAPES:
        if shape[3] == shape[2]:
            continue  # topk == E: no unpicked expert to tie with
        for vname in ("softmax_norm_scale_bias", "sigmoid_norm_scale_bias"):
            for tie in TIES:
                if tie == "saturation" and VARIANT[vname][1]:
                    continue  # only the sigmoid saturates
                out.append(pytest.param(kind, shape, env, vname, tie, id=f"{_shape_id(kind, shape, env)}-{vname}-{tie}"))
    return out


# ------------------------------------------------------------------ the float64 reference
def ref_scores(logits, softmax):
    """f64 logits [T][E] -> the f32 scores the reference model ranks."""
    logits = np.asarray(logits, F64)
    if softmax:
        e = np.exp(logits - logits.max(-1, keepdims=True))
        s = e / e.sum(-1, keepdims=True)
    else:
        s = 1.0 / (1.0 + np.exp(-logits))
    return s.astype(np.float32)


def ref_route(logits, softmax, norm, scaling, topk, ids=None):
    """ids (stable descending sort: ties keep the lower expert id) and f64 routing weights."""
    s = ref_scores(logits, softmax)
    if ids is None:
        ids = np.argsort(-s, axis=-1, kind="stable")[:, :topk]
    w = np.take_along_axis(s, ids, -1).astype(F64)
    if topk > 1 and norm:
        w = w / (w.sum(-1, keepdims=True) + 1e-20)
    return ids.astype(np.int32), w * scaling


def rows_ok(logits, softmax, groups=(), sat=()):
    """The margin rule per token row -> bool [T].  groups: expert lists whose scores are intended to tie exactly."""
    logits = np.asarray(logits, F64)
    E = logits.shape[1]
    s = ref_scores(logits, softmax)
    ok = np.ones(len(logits), bool)
    keep = np.ones(E, bool)
    for g in groups:
        ok &= (s[:, g] == s[:, [g[0]]]).all(1)
        keep[list(g[1:])] = False
    v = np.sort(s[:, keep].astype(F64), axis=1)
    ok &= ((v[:, 1:] - v[:, :-1]) > 1e-4 * v[:, 1:]).all(1)
    plain = np.ones(E, bool)
    plain[list(sat)] = False
    ok &= (np.abs(logits[:, plain]) <= 10.0).all(1)
    ok &= ~((logits > 20.0) & (logits < 30.0)).any(1)
    return ok


def draw_rows(rng, n, width, accept, scale=1.0):
    """n rows of N(0, scale) f32 values; rows that `accept` refuses are drawn again from the same stream."""
    x = np.empty((n, width), np.float32)
    todo = np.arange(n)
    for _ in range(200000):
        x[todo] = (rng.standard_normal((len(todo), width)) * scale).astype(np.float32)
        todo = todo[~accept(x[todo])]
        if not len(todo):
            return x
    raise AssertionError("no rows within the margin rule")


def _silu(g):
    return g / (1.0 + np.exp(-g))


# ------------------------------------------------------------------ decode cases
@functools.lru_cache(maxsize=None)
def _experts(H, E, I, ns):
    """Expert / shared weights (f16, N(0, 0.05) as test_moe_decode_layer) and the norm weight, per layer size."""
    rng = np.random.default_rng([11, H, E, I, ns])
    Is = I * ns

    def f(*s):
        return (rng.standard_normal(s) * 0.05).astype(np.float16)

    return {"gate": f(E, I, H), "up": f(E, I, H), "down": f(E, H, I), "sg": f(Is, H), "su": f(Is, H), "sd": f(H, Is),
            "nw": (1.0 + 0.05 * rng.standard_normal(H)).astype(np.float32)}


class RouteCase:
    """One decode MoE layer: inputs that satisfy the margin rule and the f64 reference of its routing."""

    def __init__(self, kind, shape, env, vname, tie):
        self.kind, self.shape, self.env, self.vname, self.tie = kind, shape, env, vname, tie
        T, H, E, topk, I, ns, norm = shape
        _, self.softmax, self.norm_topk, self.scaling, has_bias = VARIANT[vname]
        self.id = f"{_shape_id(kind, shape, env)}-{vname}" + (f"-{tie}" if tie else "")
        rng = np.random.default_rng([T, H, E, topk, I, ns, int(norm), [v[0] for v in VARIANTS].index(vname),
                                     1 + TIES.index(tie) if tie else 0])
        self.W = _experts(H, E, I, ns)
        self.router = (rng.standard_normal((E, H)) * 0.1).astype(np.float16)
        self.bias = (rng.standard_normal(E) * 0.5).astype(np.float32) if has_bias else None
        self.out0 = rng.standard_normal((T, H)).astype(np.float32)
        self.groups, self.sat = [], []
        if tie == "saturation":
            # +40 on three experts: every token's sigmoid score for them is exactly 1.0f
            self.sat = sorted(int(e) for e in rng.choice(E, 3, replace=False))
            self.bias[self.sat] += np.float32(40.0)
            self.groups = [self.sat]
            self.x = draw_rows(rng, T, H, self._accept)
        elif tie:
            base_router, base_bias = self.router, self.bias
            for _ in range(10000):
                # token 0 under the untied router decides which rows are tied; the tied router must then keep it
                # (and every other token) inside the margin rule
                self.router, self.bias, self.groups = base_router, base_bias, []
                x0 = draw_rows(rng, 1, H, self._accept)
                order = ref_route(self.logits64(x0), self.softmax, 0, 1.0, E)[0][0]
                unpicked = np.sort(order[topk:])
                if tie == "interior":
                    src, cand = int(order[1]), unpicked
                else:
                    src = int(order[topk - 1])
                    cand = unpicked[unpicked > src] if tie == "boundary_hi" else unpicked[unpicked < src]
                if not len(cand):
                    continue
                dst = int(cand[len(cand) // 2])
                self.router = base_router.copy()
                self.router[dst] = base_router[src]
                if base_bias is not None:
                    self.bias = base_bias.copy()
                    self.bias[dst] = base_bias[src]
                self.groups = [sorted((src, dst))]
                if self._accept(x0)[0]:
                    break
            else:
                raise AssertionError("no token 0 for the tie")
            self.src, self.dst = src, dst
            self.x = np.concatenate([x0, draw_rows(rng, T - 1, H, self._accept)]) if T > 1 else x0
        else:
            self.x = draw_rows(rng, T, H, self._accept)
        self.logits = self.logits64(self.x)
        self.ids, self.w = ref_route(self.logits, self.softmax, self.norm_topk, self.scaling, topk)

    def xn64(self, x):
        x = np.asarray(x, F64)
        if not self.shape[6]:
            return x
        return x / np.sqrt((x * x).mean(-1, keepdims=True) + 1e-6) * self.W["nw"].astype(F64)

    def logits64(self, x):
        lg = self.xn64(x) @ self.router.astype(F64).T
        return lg + self.bias.astype(F64) if self.bias is not None else lg

    def _accept(self, x):
        return rows_ok(self.logits64(x), self.softmax, self.groups, self.sat)

    def logit_bound(self):
        """test_gpu_kernels._bound on the rows the router GEMV reads (the bias is added once, exactly rounded)."""
        return _bound(self.xn64(self.x), self.router.astype(F64))

    @functools.cached_property
    def ref_out(self):
        T, H, E, topk, I, ns, norm = self.shape
        W, xn = self.W, self.xn64(self.x)
        out = self.out0.astype(F64)
        for e in np.unique(self.ids):
            rows, slots = np.nonzero(self.ids == e)
            h = _silu(xn[rows] @ W["gate"][e].astype(F64).T) * (xn[rows] @ W["up"][e].astype(F64).T)
            out[rows] += self.w[rows, slots][:, None] * (h @ W["down"][e].astype(F64).T)
        hs = _silu(xn @ W["sg"].astype(F64).T) * (xn @ W["su"].astype(F64).T)
        return out + hs @ W["sd"].astype(F64).T

    def check_tie_structure(self, ids):
        """What the tie must do to token 0 (and the saturated experts to every token)."""
        topk = self.shape[3]
        if self.tie == "saturation":
            n = min(3, topk)
            assert np.array_equal(ids[:, :n], np.tile(self.sat[:n], (len(ids), 1))), "saturated experts not in id order"
        elif self.tie == "interior":
            lo, hi = self.groups[0]
            p = list(ids[0])
            assert lo in p and hi in p and p.index(hi) == p.index(lo) + 1, (self.id, p, lo, hi)
        elif self.tie:
            lo, hi = self.groups[0]
            p = list(ids[0])
            assert p[topk - 1] == lo and hi not in p, (self.id, p, lo, hi)


@functools.lru_cache(maxsize=None)
def route_case(kind, shape, env_key, vname, tie):
    return RouteCase(kind, shape, FUSED_OFF if env_key else None, vname, tie)


def _case(kind, shape, env, vname, tie):
    return route_case(kind, shape, bool(env), vname, tie)


# ------------------------------------------------------------------ prefill cases (logits given directly)
PREFILL_T, PREFILL_E, PREFILL_TOPK = [1, 5, 300], [8, 64, 96, 256], [1, 6, 8]
PREFILL_VARIANTS = [(n, s, nm, sc) for n, s, nm, sc, _ in VARIANTS]


def _both_ok(lg, groups=(), sat=()):
    """The margin rule under softmax and under sigmoid scoring (rows with +40 logits are for the sigmoid alone)."""
    if sat:
        return rows_ok(lg, 0, groups, sat)
    return rows_ok(lg, 1, groups) & rows_ok(lg, 0, groups)


@functools.lru_cache(maxsize=None)
def prefill_logits(T, E):
    """[T][E] f32 logits inside the margin rule under softmax and under sigmoid scoring."""
    rng = np.random.default_rng([23, T, E])
    return draw_rows(rng, T, E, _both_ok, scale=2.0)


@functools.lru_cache(maxsize=None)
def prefill_tie_rows(E, topk, softmax):
    """Tied logits written directly: (logits [rows][E], per-row (what, groups, sat))."""
    rng = np.random.default_rng([29, E, topk, softmax])
    rows, info = [], []
    for what in ["interior", "boundary_hi", "boundary_lo", "all_equal", "saturation"]:
        if what == "all_equal":
            rows.append(np.full(E, 0.375, np.float32))
            info.append((what, [list(range(E))], []))
            continue
        if (what == "interior" and topk < 2) or (what == "saturation" and softmax) or \
                (what != "saturation" and topk == E):
            continue  # (topk == E: no unpicked expert to tie with)
        for _ in range(10000):
            r = draw_rows(rng, 1, E, _both_ok, scale=2.0)[0]
            order = ref_route(r[None], softmax, 0, 1.0, E)[0][0]
            unpicked = np.sort(order[topk:])
            groups, sat = [], []
            if what == "saturation":
                if E - topk < 3:
                    sat = sorted(int(e) for e in rng.choice(E, 3, replace=False))
                else:
                    sat = sorted(int(e) for e in rng.choice(unpicked, 3, replace=False))
                r[sat] = np.float32([40.0, 43.0, 41.5])
                groups = [sat]
            else:
                src = int(order[1] if what == "interior" else order[topk - 1])
                cand = unpicked if what == "interior" else \
                    (unpicked[unpicked > src] if what == "boundary_hi" else unpicked[unpicked < src])
                if not len(cand):
                    continue
                dst = int(cand[len(cand) // 2])
                r[dst] = r[src]
                groups = [sorted((src, dst))]
            if _both_ok(r[None], groups, sat)[0]:
                break
        else:
            raise AssertionError("no tied row")
        rows.append(r)
        info.append((what, groups, sat))
    return np.stack(rows), info


# ------------------------------------------------------------------ CPU: the hooks exist, the cases obey the rule
def test_header_declares_and_library_exports_routing_symbols():
    import re
    header = open(os.path.join(ROOT, "include", "dsocr.h")).read()
    declared = set(re.findall(r"\b(dsocr_[a-z0-9_]+)\s*\(", header))
    from dsocr._lib import EXPORTS, LIB_PATH
    L = C.CDLL(LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared and s in EXPORTS, s
        assert hasattr(L, s), s


def _route_kind(shape):
    T, H, E, topk, I, ns, norm = shape
    k = C.c_char_p()
    check(lib().dsocr_k_moe_route_kind(T, H, E, topk, I, I * ns, int(norm), C.byref(k)))
    return k.value.decode()


def test_every_route_kind_is_reached(monkeypatch):
    """The dispatch decision is host code: every shape reaches the implementation its cases name, every kind
    the hook can return is named by a shape, and the hook honours DSOCR_ROUTE_FUSED as the plan does."""
    seen = set()
    for kind, shape, env in DECODE_SHAPES + [TOPK1_SHAPE]:
        with monkeypatch.context() as m:
            m.delenv("DSOCR_ROUTE_FUSED", raising=False)
            for k, v in (env or {}).items():
                m.setenv(k, v)
            assert _route_kind(shape) == kind, (shape, env)
        seen.add(kind)
    assert seen == set(ROUTE_KINDS)
    tied = {p.values[0] for p in _tie_params()}
    assert tied == set(ROUTE_KINDS)
    k = C.c_char_p()
    for bad in [(1, 256, 257, 6, 32, 32, 1), (1, 256, 16, 9, 32, 32, 1), (1, 256, 5, 6, 32, 32, 1)]:
        assert lib().dsocr_k_moe_route_kind(*bad, C.byref(k)) == EINVAL, bad


@pytest.mark.parametrize("kind,shape,env,vname,tie", _decode_params() + _tie_params())
def test_margin_rule_decode(kind, shape, env, vname, tie):
    """Every token of every decode case: scores apart by more than 1e-4 relative unless tied on purpose (then
    exactly equal), |logit| <= 10 outside the +40 experts, none in (20, 30); the tie does to token 0 what the
    case is named for."""
    c = _case(kind, shape, env, vname, tie)
    T, H, E, topk = shape[:4]
    assert c.x.shape == (T, H) and c.ids.shape == (T, topk)
    assert rows_ok(c.logits, c.softmax, c.groups, c.sat).all()
    s = ref_scores(c.logits, c.softmax)
    tied = {e for g in c.groups for e in g}
    for t in range(T):
        assert len(np.unique(s[t])) == E - len(tied) + len(c.groups), t
    if tie == "saturation":
        assert (s[:, c.sat] == np.float32(1.0)).all() and (c.logits[:, c.sat] > 30.0).all()
    elif tie:
        assert np.array_equal(c.router[c.src], c.router[c.dst])
        assert c.bias is None or c.bias[c.src] == c.bias[c.dst]
    c.check_tie_structure(c.ids)
    if topk == 1 and c.norm_topk:  # renormalisation must not apply to one pick
        assert np.all(c.w < c.scaling * 0.999)


@pytest.mark.parametrize("E", PREFILL_E)
def test_margin_rule_prefill(E):
    for T in PREFILL_T:
        lg = prefill_logits(T, E)
        assert lg.shape == (T, E) and rows_ok(lg, 1).all() and rows_ok(lg, 0).all()
    for topk in PREFILL_TOPK:
        for softmax in (1, 0):
            lg, info = prefill_tie_rows(E, topk, softmax)
            assert {i[0] for i in info} >= {"all_equal"} and len(lg) == len(info)
            for r, (what, groups, sat) in zip(lg, info):
                assert rows_ok(r[None], softmax, groups, sat)[0], (E, topk, softmax, what)


# ------------------------------------------------------------------ GPU: the decode implementations
@functools.lru_cache(maxsize=None)
def _dev_experts(H, E, I, ns):
    W = _experts(H, E, I, ns)
    u16 = lambda a: np.ascontiguousarray(a).view(np.uint16)
    return {"gu": Dev(u16(np.concatenate([W["gate"], W["up"]], axis=1))), "d": Dev(u16(W["down"])),
            "sgu": Dev(u16(np.concatenate([W["sg"], W["su"]]))), "sd": Dev(u16(W["sd"])), "nw": Dev(W["nw"])}


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _run_decode(c):
    T, H, E, topk, I, ns, norm = c.shape
    D = _dev_experts(H, E, I, ns)
    dx, dr, dout = Dev(c.x), Dev(np.ascontiguousarray(c.router).view(np.uint16)), Dev(c.out0)
    db = Dev(c.bias) if c.bias is not None else None
    ids, w, lg = np.zeros((T, topk), np.int32), np.zeros((T, topk), np.float32), np.zeros((T, E), np.float32)
    check(lib().dsocr_k_moe_ex(T, H, E, topk, I, I * ns, dx.ptr, D["nw"].ptr if norm else None, 1e-6, dr.ptr,
                               D["gu"].ptr, D["d"].ptr, D["sgu"].ptr, D["sd"].ptr, 1, c.norm_topk, c.scaling, dout.ptr,
                               _ptr(ids), _ptr(w), c.softmax, db.ptr if db else None, _ptr(lg)))
    return ids, w, lg, dout.get()


def _check_decode(c, monkeypatch):
    monkeypatch.delenv("DSOCR_ROUTE_FUSED", raising=False)
    for k, v in (c.env or {}).items():
        monkeypatch.setenv(k, v)
    assert _route_kind(c.shape) == c.kind
    ids, w, lg, out = _run_decode(c)
    topk = c.shape[3]
    lerr = np.abs(lg.astype(F64) - c.logits)
    assert np.all(lerr <= c.logit_bound()), (c.id, "logits", float(lerr.max()))
    for g in c.groups if c.tie != "saturation" else []:
        assert np.array_equal(lg[:, g[0]].view(np.uint32), lg[:, g[1]].view(np.uint32)), \
            (c.id, "duplicated router rows give different logit columns")
    assert np.array_equal(ids, c.ids), (c.id, "ids", ids.tolist(), c.ids.tolist())
    c.check_tie_structure(ids)
    wref = ref_route(lg, c.softmax, c.norm_topk, c.scaling, topk, ids=c.ids)[1]
    werr = float(np.max(np.abs(w - wref) / np.abs(wref)))
    oerr = float(np.max(np.abs(out - c.ref_out)))
    print(f"moe_routing {c.id}: max out err {oerr:.3e} max rel weight err {werr:.3e} max logit err {lerr.max():.3e}")
    assert werr <= 1e-5, (c.id, "weights", werr)
    assert oerr <= 1e-4 * max(1.0, c.scaling), (c.id, "output", oerr)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,shape,env,vname,tie", _decode_params())
def test_decode_routing_variants(gpu, monkeypatch, kind, shape, env, vname, tie):
    _check_decode(_case(kind, shape, env, vname, tie), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,shape,env,vname,tie", _tie_params())
def test_decode_routing_ties(gpu, monkeypatch, kind, shape, env, vname, tie):
    _check_decode(_case(kind, shape, env, vname, tie), monkeypatch)


@pytest.mark.gpu
def test_moe_hooks_reject_out_of_range(gpu):
    buf = Dev.zeros(4096, np.float32)
    p = buf.ptr

    def ex(E, topk, x=p, out=p):
        return lib().dsocr_k_moe_ex(1, 256, E, topk, 32, 0, x, None, 1e-6, p, p, p, None, None, 1, 0, 1.0, out, None,
                                    None, 1, None, None)

    def route(E, topk, logits=p, apos=p):
        return lib().dsocr_k_moe_prefill_route(1, E, topk, logits, 1, 0, 1.0, p, p, p, p, apos)

    for f in (ex, route):
        assert f(257, 6) == EINVAL and f(16, 9) == EINVAL and f(5, 6) == EINVAL and f(0, 1) == EINVAL
    assert ex(16, 6, x=None) == EINVAL and ex(16, 6, out=None) == EINVAL
    assert route(16, 6, logits=None) == EINVAL and route(16, 6, apos=None) == EINVAL
    comb = lib().dsocr_k_moe_combine
    assert comb(1, 9, 8, p, p, p, None, p, 0) == EINVAL and comb(1, 2, 8, None, p, p, None, p, 0) == EINVAL
    assert comb(1, 2, 8, p, p, p, None, None, 0) == EINVAL and comb(0, 2, 8, p, p, p, None, p, 0) == EINVAL


# ------------------------------------------------------------------ GPU: the prefill's routing, grouping, combine
def _run_prefill(lg, topk, softmax, norm, scaling):
    T, E = lg.shape
    dl = Dev(lg)
    ids, w = Dev.zeros((T, topk), np.int32), Dev.zeros((T, topk), np.float32)
    eoff, arow, apos = Dev.zeros(E + 1, np.int32), Dev.zeros(T * topk, np.int32), Dev.zeros(T * topk, np.int32)
    check(lib().dsocr_k_moe_prefill_route(T, E, topk, dl.ptr, softmax, norm, scaling, ids.ptr, w.ptr, eoff.ptr,
                                          arow.ptr, apos.ptr))
    return ids.get(), w.get(), eoff.get(), arow.get(), apos.get()


def _check_prefill(tag, lg, topk, softmax, norm, scaling):
    T, E = lg.shape
    ids, w, eoff, arow, apos = _run_prefill(lg, topk, softmax, norm, scaling)
    rids, rw = ref_route(lg, softmax, norm, scaling, topk)
    assert np.array_equal(ids, rids), (tag, "ids", np.argwhere(ids != rids)[:4].tolist())
    werr = float(np.max(np.abs(w - rw) / np.abs(rw)))
    print(f"moe_routing prefill {tag}: max rel weight err {werr:.3e}")
    assert werr <= 1e-5, (tag, "weights", werr)
    flat = rids.reshape(-1)
    assert np.array_equal(eoff, np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=E))])), (tag, "eoff")
    assert np.array_equal(np.sort(apos), np.arange(T * topk)), (tag, "apos is not a permutation")
    assert np.array_equal(arow[apos], np.arange(T * topk) // topk), (tag, "arow")
    by_pos = np.empty(T * topk, np.int64)
    by_pos[apos] = flat                      # the expert of the assignment at each sorted position
    assert np.array_equal(by_pos, np.repeat(np.arange(E), np.diff(eoff))), (tag, "positions outside their expert")
    return ids, w, apos


@pytest.mark.gpu
@pytest.mark.parametrize("variant", PREFILL_VARIANTS, ids=[v[0] for v in PREFILL_VARIANTS])
@pytest.mark.parametrize("topk", PREFILL_TOPK)
@pytest.mark.parametrize("E", PREFILL_E)
@pytest.mark.parametrize("T", PREFILL_T)
def test_prefill_route(gpu, T, E, topk, variant):
    """router_topk + moe_group as the prefill launches them; T * topk = 1800 and 2400 exceed the group kernel's
    1024-thread block."""
    name, softmax, norm, scaling = variant
    _check_prefill(f"T{T}-E{E}-k{topk}-{name}", prefill_logits(T, E), topk, softmax, norm, scaling)


@pytest.mark.gpu
@pytest.mark.parametrize("softmax", [1, 0], ids=["softmax", "sigmoid"])
@pytest.mark.parametrize("topk", PREFILL_TOPK)
@pytest.mark.parametrize("E", PREFILL_E)
def test_prefill_route_ties(gpu, E, topk, softmax):
    lg, info = prefill_tie_rows(E, topk, softmax)
    ids, _, _ = _check_prefill(f"ties-E{E}-k{topk}-{'softmax' if softmax else 'sigmoid'}", lg, topk, softmax, 1, 2.5)
    for r, (what, groups, sat) in enumerate(info):
        p = list(ids[r])
        if what == "all_equal":
            assert p == list(range(topk)), (what, p)
        elif what == "saturation":
            assert p[:min(3, topk)] == sat[:min(3, topk)], (what, p, sat)
        elif what == "interior":
            lo, hi = groups[0]
            assert lo in p and hi in p and p.index(hi) == p.index(lo) + 1, (what, p, lo, hi)
        else:
            lo, hi = groups[0]
            assert p[topk - 1] == lo and hi not in p, (what, p, lo, hi)


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [False, True], ids=["noshared", "shared"])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("T,E,topk,H", [(1, 8, 1, 8), (5, 96, 6, 300), (300, 256, 8, 72)])
def test_prefill_combine(gpu, T, E, topk, H, accumulate, shared):
    """moe_combine over the positions moe_group assigned: out (+)= sum_k w y[apos] (+ shared), against f64 within
    1e-6 * sum |w y| + 1e-6."""
    rng = np.random.default_rng([31, T, topk, H])
    ids, w, apos = _check_prefill(f"combine-T{T}-E{E}-k{topk}", prefill_logits(T, E), topk, 0, 1, 2.5)
    y = rng.standard_normal((T * topk, H)).astype(np.float32)
    sh = rng.standard_normal((T, H)).astype(np.float32)
    out0 = rng.standard_normal((T, H)).astype(np.float32)
    dy, dap, dw, dsh, dout = Dev(y), Dev(apos), Dev(w), Dev(sh), Dev(out0)
    check(lib().dsocr_k_moe_combine(T, topk, H, dy.ptr, dap.ptr, dw.ptr, dsh.ptr if shared else None, dout.ptr,
                                    accumulate))
    terms = w.astype(F64)[:, :, None] * y.astype(F64)[apos.reshape(T, topk)]
    ref = terms.sum(1) + (sh if shared else 0.0) + (out0 if accumulate else 0.0)
    err = np.abs(dout.get() - ref)
    assert np.all(err <= 1e-6 * np.abs(terms).sum(1) + 1e-6), float(err.max())


# ------------------------------------------------------------------ GPU: the options through the engine's config
LANG_OPTS = {"scoring_func": "sigmoid", "norm_topk_prob": True, "routed_scaling_factor": 2.5}
SEED = 7


def _variant_config(tmp_path):
    cfg = json.load(open(TINY))
    cfg["language_config"].update(LANG_OPTS)
    for k, v in LANG_OPTS.items():
        if k in cfg:
            cfg[k] = v
    path = tmp_path / "tiny_sigmoid.json"
    path.write_text(json.dumps(cfg))
    return cfg, str(path)


def _bias_checkpoint(cfg, path):
    """The synthetic tiny checkpoint as a bf16 safetensors file, plus an e_score_correction_bias per MoE layer."""
    from oracle.specs import tensor_names
    from oracle.weights import synth_bf16, synthetic_has
    tensors = {n: synth_bf16(n, SEED, int(np.prod(s))).reshape(s) for n, s in tensor_names(cfg).items()
               if synthetic_has(n)}
    L = cfg["language_config"]
    rng = np.random.default_rng(41)
    for l in range(L["first_k_dense_replace"], L["num_hidden_layers"]):
        b = rng.standard_normal(L["n_routed_experts"]) * 0.5
        b = np.where(np.abs(b) < 2.0 ** -10, 2.0 ** -10, b)  # bf16 values that an f16 load keeps exactly
        tensors[f"model.layers.{l}.mlp.gate.e_score_correction_bias"] = bf16_round(b.astype(np.float32))
    write_bf16_safetensors(path, tensors)


def _engine_vs_oracle(eng, orc):
    """One image page (24 tokens: prefill, then one-token decode), 4 text prompts (the grouped decode) and 9 text
    prompts (more than 8 tokens: moe_route) against the oracle's greedy ids."""
    from dsocr import DecodeParameters, Page, VisionSettings, build_prompt_tokens
    from dsocr.synth import SyntheticTokenizer
    img = np.random.default_rng(12).integers(0, 256, (300, 420, 3), dtype=np.uint8)
    page = Page(img, VisionSettings(256, 128, True))
    ids, mask = build_prompt_tokens(SyntheticTokenizer(512), "<image>\nConvert the document to markdown.",
                                    [page.n_image_tokens])
    got = [eng.generate(ids, mask, page, None, DecodeParameters(max_new_tokens=24))]
    emb, _ = orc.image_embeddings(img, 256, 128, True)
    ref = [orc.generate(ids, mask, emb, 24, eos_token_id=1, no_repeat_ngram_size=20)[0]]
    rng = np.random.default_rng(13)
    prompts = [[0] + [int(t) for t in rng.integers(2, 500, 12 + 3 * i)] for i in range(9)]
    p = DecodeParameters(max_new_tokens=12)
    for n in (4, 9):
        got += eng.generate_batch([(q, None, None, None) for q in prompts[:n]], p)
    refs = [orc.generate(q, [0] * len(q), None, 12, eos_token_id=1, no_repeat_ngram_size=20)[0] for q in prompts]
    ref += refs[:4] + refs
    assert got == ref, [i for i, (a, b) in enumerate(zip(got, ref)) if a != b]
    return got


@pytest.mark.gpu
def test_engine_sigmoid_norm_scaling_and_bias(gpu, tmp_path):
    """scoring_func sigmoid, norm_topk_prob, routed_scaling_factor 2.5 through the config plumbing, without and
    with mlp.gate.e_score_correction_bias in the checkpoint: prefill routing, one-token decode, the grouped decode
    at 4 prompts and moe_route at 9, ids equal to the oracle's; the bias changes the ids (it is not dropped)."""
    from dsocr import ModelLoadArgs, load_model
    from oracle.model import OracleModel
    from oracle.weights import Weights
    cfg, cfg_path = _variant_config(tmp_path)
    eng = load_model(ModelLoadArgs(config_path=cfg_path, synthetic_seed=SEED, dtype="f16"))
    try:
        plain = _engine_vs_oracle(eng, OracleModel(cfg, Weights(seed=SEED, dtype="f16")))
    finally:
        eng.close()
    ck = str(tmp_path / "bias.safetensors")
    _bias_checkpoint(cfg, ck)
    eng = load_model(ModelLoadArgs(config_path=cfg_path, weights_path=ck, dtype="f16"))
    try:
        biased = _engine_vs_oracle(eng, OracleModel(cfg, Weights(path=ck, dtype="f16")))
    finally:
        eng.close()
    assert biased != plain, "the correction bias changed no token: it was dropped"
