"""Cases, graphs and references for the neuron layers (csrc/neuron.hip: neuron_kernel) -- PReLU, Sigmoid, TanH, ELU, AbsVal,
Threshold, BNLL, Power, Exp and Log (tests/test_neuron_host.py, tests/test_gpu_neuron.py).  Everything here runs without a GPU.

A layer is written as a spec ``(type, fields)``: ``("Power", {"scale": -1})``, ``("PReLU", {"shared": True})``.  Per element
(the reference Caffe's CPU formulas, cited in the kernel's header):

``neuron64``   binary64 from the fp32 inputs and the fp32 parameters, unrounded -- the yardstick, and rounded once what conv
               mode "f64" computes.  Where Caffe's formula cancels (Sigmoid, ELU, BNLL) the function is evaluated in a form
               that does not (``expm1``, ``log1p``): the yardstick is the function's value, not a binary64 run of the formula.
``neuron32``   the exact ops in fp32, one rounding per arithmetic step in Caffe's order: PReLU (a product, an add), AbsVal,
               Threshold, Power with ``power: 1`` (a product if scale != 1, an add if shift != 0).
``derived``    Exp's ``inner`` / ``outer`` and Log's ``base_scale`` as csrc/net_graph.cpp forms them: binary64 from the fp32
               fields, rounded once (Caffe: fp32 from float library calls, an ulp apart at most).
``bound``      per element, for fp32 mode: the first-order propagation through Caffe's formula of half an ulp per fp32
               arithmetic step and ``LIB_ULPS`` ulps per library call -- the accuracy the device library is specified to
               (OpenCL's table: exp 3, log 3, tanh 5, pow 16), held as a cap with no margin.

A layer case is ``(C, H, W)``.  The layer under test reads the blob behind ``pre`` / ``sel`` of tests/general_conv_cases.py
(1x1 layers that hand an integer grid on unchanged in every conv mode; in fp32 and f64 mode any grid); above 240 channels
the 16-channel fan-out of tests/depthwise_cases.py.  ``NeuronOracleNet`` is ``norm_cases.NormOracleNet`` plus the ten layers
(``neuron32`` for the exact ops, fp32(``neuron64``) for the others).
"""
import json
import math
import os

import numpy as np

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from tests import depthwise_cases as D
from tests import fusion_cases as F
from tests import general_conv_cases as G
from tests import helpers as H
from tests import norm_cases as N

F32 = np.float32
F64 = np.float64
TYPES = ("PReLU", "Sigmoid", "TanH", "ELU", "AbsVal", "Threshold", "BNLL", "Power", "Exp", "Log")
KERNEL = "neuron"                      # the profiler's class and kernel name
LIB_ULPS = {"exp": 3.0, "log": 3.0, "tanh": 5.0, "pow": 16.0}

LAYER_CASES = [
    (4, 1, 1),                   # one quad
    (1, 3, 3),                   # scalar form, one channel
    (5, 7, 9),                   # scalar form, C % 4 == 1, rows ragged against the rows per block
    (6, 7, 9),                   # C % 4 == 2
    (16, 5, 5),                  # vector form
    (260, 5, 5),                 # the slope vector past one block's quads
    (64, 33, 67),                # several blocks, a ragged last block
]


def case_id(case):
    return "c%d_%dx%d" % tuple(case)


# ---- specs --------------------------------------------------------------------------------------------------------------------
_DEFAULTS = {
    "PReLU": {"shared": False}, "ELU": {"alpha": 1.0}, "Threshold": {"threshold": 0.0},
    "Power": {"power": 1.0, "scale": 1.0, "shift": 0.0}, "Exp": {"base": -1.0, "scale": 1.0, "shift": 0.0},
    "Log": {"base": -1.0, "scale": 1.0, "shift": 0.0},
}
_PARAM_FIELD = {"PReLU": "prelu_param", "ELU": "elu_param", "Threshold": "threshold_param", "Power": "power_param",
                "Exp": "exp_param", "Log": "log_param", "Sigmoid": "sigmoid_param", "TanH": "tanh_param"}


def fields(spec):
    """The spec's fields over the proto's defaults, every number as the fp32 value Caffe holds."""
    t, kw = spec
    out = dict(_DEFAULTS.get(t, {}))
    out.update(kw)
    return {k: (v if isinstance(v, bool) else float(F32(v))) for k, v in out.items() if k not in ("fill", "filler")}


def spec_id(spec):
    t, kw = spec
    return t + "".join("_%s%s" % (k, str(v).replace("-", "m").replace(".", "p")) for k, v in sorted(kw.items()))


def derived(spec):
    """Exp: (inner, outer); Log: base_scale -- binary64 from the fp32 fields, rounded once, as csrc/net_graph.cpp forms them."""
    t, f = spec[0], fields(spec)
    log_base = 1.0 if f["base"] == -1.0 else math.log(f["base"])
    if t == "Exp":
        outer = 1.0 if f["shift"] == 0 else (math.pow(f["base"], f["shift"]) if f["base"] != -1.0 else math.exp(f["shift"]))
        return F32(log_base * f["scale"]), F32(outer)
    assert t == "Log"
    return F32(1.0 / log_base)


def _slope(slope, C, shared):
    s = np.asarray(slope, F32).reshape(-1)
    assert s.size == (1 if shared else C), (s.size, C, shared)
    return (np.full(C, s[0], F32) if shared else s).reshape(1, C, 1, 1)


# ---- references ---------------------------------------------------------------------------------------------------------------
def neuron64(spec, x, slope=None):
    """The layer in binary64 from the fp32 values, unrounded: x (N, C, H, W)."""
    t, f = spec[0], fields(spec)
    x = np.asarray(x, F32).astype(F64)
    with np.errstate(all="ignore"):
        if t == "PReLU":
            return np.maximum(x, 0) + _slope(slope, x.shape[1], f["shared"]).astype(F64) * np.minimum(x, 0)
        if t == "Sigmoid":
            e = np.exp(-np.abs(x))
            return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        if t == "TanH":
            return np.tanh(x)
        if t == "ELU":
            return np.maximum(x, 0) + f["alpha"] * np.expm1(np.minimum(x, 0))
        if t == "AbsVal":
            return np.abs(x)
        if t == "Threshold":
            return (x > f["threshold"]).astype(F64)
        if t == "BNLL":
            return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))
        if t == "Power":
            if F32(f["power"]) * F32(f["scale"]) == 0:
                return np.full(x.shape, 1.0 if f["power"] == 0 else math.pow(f["shift"], f["power"]), F64)
            v = f["shift"] + f["scale"] * x
            return v if f["power"] == 1.0 else np.power(v, f["power"])
        if t == "Exp":
            inner, outer = derived(spec)
            return F64(outer) * np.exp(F64(inner) * x)
        assert t == "Log", t
        return F64(derived(spec)) * np.log(f["shift"] + f["scale"] * x)


EXACT_TYPES = ("PReLU", "AbsVal", "Threshold", "Power")


def is_exact(spec):
    return spec[0] in EXACT_TYPES and (spec[0] != "Power" or fields(spec)["power"] == 1.0)


def neuron32(spec, x, slope=None):
    """The exact ops in fp32, one rounding per arithmetic step, in Caffe's order."""
    assert is_exact(spec), spec
    t, f = spec[0], fields(spec)
    x = np.asarray(x, F32)
    zero = F32(0)
    if t == "PReLU":      # std::max(x, 0) + a * std::min(x, 0), the operands in std::max / std::min's order
        mx, mn = np.where(x < zero, zero, x), np.where(zero < x, zero, x)
        with np.errstate(invalid="ignore"):
            return (mx + (_slope(slope, x.shape[1], f["shared"]) * mn).astype(F32)).astype(F32)
    if t == "AbsVal":
        return np.abs(x)
    if t == "Threshold":
        return (x > F32(f["threshold"])).astype(F32)
    v = x
    if f["scale"] != 1.0:
        v = (v * F32(f["scale"])).astype(F32)
    if f["shift"] != 0.0:
        v = (v + F32(f["shift"])).astype(F32)
    return v.astype(F32)


def single_rounding(spec):
    """The fp32 formula rounds at most once: conv mode "f64" gives the same value."""
    f = fields(spec)
    return is_exact(spec) and (spec[0] != "Power" or f["scale"] == 1.0 or f["shift"] == 0.0)


def numpy32(spec, x):
    """Caffe's formula evaluated by numpy in fp32, step by step (the library ops; tests/test_neuron_host.py holds it to
    ``bound``: the inputs are ones the reference itself passes)."""
    t, f = spec[0], fields(spec)
    x = np.asarray(x, F32)
    one, half, zero = F32(1), F32(0.5), F32(0)
    with np.errstate(all="ignore"):
        if t == "Sigmoid":
            return half * np.tanh(half * x) + half
        if t == "TanH":
            return np.tanh(x)
        if t == "ELU":
            return np.maximum(x, zero) + F32(f["alpha"]) * (np.exp(np.minimum(x, zero)) - one)
        if t == "BNLL":
            l = np.log(one + np.exp(-np.abs(x)))
            return np.where(x > 0, x + l, l).astype(F32)
        if t == "Power":
            v = x if f["scale"] == 1.0 else x * F32(f["scale"])
            v = v if f["shift"] == 0.0 else v + F32(f["shift"])
            return np.power(v, F32(f["power"]))
        if t == "Exp":
            inner, outer = derived(spec)
            return outer * np.exp(inner * x)
        assert t == "Log", t
        return derived(spec) * np.log(F32(f["scale"]) * x + F32(f["shift"]))


def ulp32(v):
    """The fp32 spacing at |v| (2^-149 at 0), in binary64."""
    with np.errstate(all="ignore"):
        return np.spacing(np.abs(np.asarray(v, F64)).astype(F32)).astype(F64)


def bound(spec, x):
    """Per element: what an fp32 evaluation of Caffe's formula may differ from ``neuron64`` by -- half an ulp of each fp32
    arithmetic step's result and LIB_ULPS ulps of each library call's, propagated to first order (a step that Caffe skips,
    or whose result is exact -- a product with 0.5 -- adds nothing).  Absolute where the formula cancels (Sigmoid, ELU,
    BNLL: the terms do not scale with the result), relative -- multiples of the result's ulp -- elsewhere."""
    t, f = spec[0], fields(spec)
    x = np.asarray(x, F32).astype(F64)
    ref = neuron64(spec, x)
    Le, Ll, Lt, Lp = LIB_ULPS["exp"], LIB_ULPS["log"], LIB_ULPS["tanh"], LIB_ULPS["pow"]
    with np.errstate(all="ignore"):
        if t == "Sigmoid":     # 0.5 x exact; tanh; 0.5 T exact; + 0.5
            return 0.5 * Lt * ulp32(np.tanh(0.5 * x)) + 0.5 * ulp32(ref)
        if t == "TanH":
            return Lt * ulp32(ref)
        if t == "ELU":         # E = exp(min(x, 0)); d = E - 1; p = alpha d; max(x, 0) + p
            E = np.exp(np.minimum(x, 0))
            e_d = Le * ulp32(E) + 0.5 * ulp32(E - 1)
            return abs(f["alpha"]) * e_d + 0.5 * ulp32(f["alpha"] * (E - 1)) + np.where(x > 0, 0.5 * ulp32(ref), 0.0)
        if t == "BNLL":        # E = exp(-|x|); s = 1 + E; l = log(s); x > 0: x + l
            E = np.exp(-np.abs(x))
            s = 1 + E
            e_s = Le * ulp32(E) + 0.5 * ulp32(s)
            return e_s / s + Ll * ulp32(np.log(s)) + np.where(x > 0, 0.5 * ulp32(ref), 0.0)
        if t == "Exp":         # v = inner x; E = exp(v); outer E
            inner, outer = [F64(c) for c in derived(spec)]
            E = np.exp(inner * x)
            e_v = 0.5 * ulp32(inner * x) if inner != 1 else 0.0
            return abs(outer) * (E * e_v + Le * ulp32(E)) + (0.5 * ulp32(ref) if outer != 1 else 0.0)
        # Power / Log: v = scale x; w = v + shift
        v = f["scale"] * x
        w = v + f["shift"]
        e_w = np.zeros_like(x) + (0.5 * ulp32(v) if f["scale"] != 1.0 else 0.0) + (0.5 * ulp32(w) if f["shift"] != 0.0 else 0.0)
        rel_w = np.where(e_w > 0, e_w / np.where(w != 0, np.abs(w), 1.0), 0.0)      # (w = x exactly where no step ran: no error to carry)
        if t == "Log":
            bs = F64(derived(spec))
            return abs(bs) * (rel_w + Ll * ulp32(np.log(w))) + (0.5 * ulp32(ref) if bs != 1 else 0.0)
        assert t == "Power" and f["power"] != 1.0, spec
        return abs(f["power"]) * np.abs(ref) * rel_w + Lp * ulp32(ref)


def ulps(got, ref):
    """|got - ref| in fp32 ulps of ref, per element."""
    return np.abs(np.asarray(got, F64) - ref) / ulp32(ref)


# ---- layer text -------------------------------------------------------------------------------------------------------------
def _num(v):
    return v if isinstance(v, str) else repr(float(v))


def neuron_layer(name, spec, bottom, top=None, pnames=None, extra=""):
    """``top`` None: in place.  PReLU's ``fill``: the value of a constant filler; ``filler``: a filler message's text instead.
    ``extra``: text inside the layer's parameter message."""
    t, kw = spec
    body = ""
    if t == "PReLU":
        if "shared" in kw:
            body += " channel_shared: %s" % ("true" if kw["shared"] else "false")
        if "filler" in kw:
            body += " filler { %s }" % kw["filler"]
        elif "fill" in kw:
            body += ' filler { type: "constant" value: %s }' % _num(kw["fill"])
    else:
        body += "".join(" %s: %s" % (k, _num(v)) for k, v in kw.items())
    body += extra
    par = "".join(' param { name: "%s" }' % p for p in (pnames or []))
    msg = " %s {%s }" % (_PARAM_FIELD[t], body) if body else ""
    return 'layer { name: "%s" type: "%s" bottom: "%s" top: "%s"%s%s }\n' % (name, t, bottom, top or bottom, par, msg)


def layer_spec(L):
    """The spec of a layer message of the ten types (what ``neuron_layer`` wrote, read back)."""
    t = str(L.get("type"))
    pm = L.get(_PARAM_FIELD[t]) if t in _PARAM_FIELD else None
    kw = {}
    if pm is not None and t == "PReLU":
        kw["shared"] = str(pm.get("channel_shared", "false")) == "true"
        fl = pm.get("filler")
        if fl is not None:
            kw["filler"] = fl
    elif pm is not None:
        for k in _DEFAULTS.get(t, {}):
            if pm.get(k) is not None:
                kw[k] = float(str(pm.get(k)))
    return (t, kw)


def prelu_fill(spec):
    """What a fresh PReLU blob holds: a constant filler's value (0 when it names none), 0.25 without a filler or with one of
    another type."""
    kw = spec[1]
    if "fill" in kw:
        return float(kw["fill"])
    fl = kw.get("filler")
    if fl is None:
        return 0.25
    if isinstance(fl, str):
        fl = P.parse("f { %s }" % fl).get("f")
    return float(str(fl.get("value", 0.0))) if str(fl.get("type", "constant")) == "constant" else 0.25


def filler_params(msg):
    """{layer name: [slope blob]} of every PReLU layer of ``msg`` as its filler creates it: (C,), or no axes when shared."""
    ch = O.infer_channels(msg)
    out = {}
    for L in msg.getall("layer"):
        if str(L.get("type")) == "PReLU":
            spec = layer_spec(L)
            out[str(L.get("name"))] = [np.full(() if spec[1].get("shared") else (ch[str(L.get("bottom"))],), prelu_fill(spec), F32)]
    return out


def feeder_txt(C):
    return D.feeder_txt(C)


def ops_net_text(case, specs, in_place=False):
    """`pre` (/ `sel`) and one layer per spec, `n0`, `n1`, ...: out of place each reads the feeder's blob and writes its own
    top; in place each rewrites a copy of its own, made by a Power layer with the proto's defaults (`cp<i>`: an exact copy)."""
    C, h, w = case
    txt, bottom = D.feeder_txt(C)
    for i, spec in enumerate(specs):
        if in_place:
            txt += neuron_layer("cp%d" % i, ("Power", {}), bottom, "n%d" % i) + neuron_layer("op%d" % i, spec, "n%d" % i)
        else:
            txt += neuron_layer("op%d" % i, spec, bottom, "n%d" % i)
    return H.single_layer_net(txt, D.data_channels(C), h, w)


def concat_net_text(C, spec, h=7, w=9):
    """`pre` -> `s0`, `s1` (selections of C channels each) -> Concat `cin`; the layer `n0` on `s0` -> `a`, `n1` on `s1` -> `b`;
    Concat `cat` of `a` and `b`.  `n1` reads the view at channel C of `cin`'s 2 C and writes the view at channel C of `cat`'s
    (C = 12: the vector form on offset views; C = 6: the scalar form)."""
    return H.single_layer_net(G.conv_txt("pre", "data", 16, 1) + G.conv_txt("s0", "pre", C, 1) + G.conv_txt("s1", "pre", C, 1) +
                              F.concat_layer("cin", ["s0", "s1"]) + neuron_layer("n0", spec, "s0", "a") +
                              neuron_layer("n1", spec, "s1", "b") + F.concat_layer("cat", ["a", "b"]), 16, h, w)


# ---- the ops of the tests -----------------------------------------------------------------------------------------------------
EXACT_SPECS = [("PReLU", {}), ("PReLU", {"shared": True}), ("AbsVal", {}), ("Threshold", {}), ("Threshold", {"threshold": 1.5}),
               ("Power", {"scale": -1}), ("Power", {"scale": 3, "shift": -2})]
SIGNED_SPECS = [("Sigmoid", {}), ("TanH", {}), ("ELU", {}), ("ELU", {"alpha": 0.5}), ("BNLL", {}), ("Exp", {}),
                ("Exp", {"base": 2, "scale": 0.5, "shift": 1})]
POSITIVE_SPECS = [("Log", {"scale": 2, "shift": 3}), ("Power", {"power": 2}), ("Power", {"power": 0.5})]    # on non-negative inputs
LIBRARY_SPECS = SIGNED_SPECS + POSITIVE_SPECS
LIMIT = 20.0                       # Sigmoid, TanH and BNLL saturate there; exp(20) and 2^(0.5 * 20 + 1) are far from fp32's end
SPECIALS = [0.0, 2.0 ** -20, -2.0 ** -20, 1.0, -1.0, LIMIT, -LIMIT]


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def int_inputs(case, seed=0):
    """Integers in [-4, 4] with zeros among them, and PReLU slopes in {-2, .., 2}: a per-channel vector that holds a 0 and a -2
    (where it has the room), and the shared value -2."""
    C, h, w = case
    rng = np.random.default_rng(100 * C + 10 * h + w + seed)
    data = rng.integers(-4, 5, (1, D.data_channels(C), h, w)).astype(F32)
    data[0, 0, 0, 0] = 0
    sl = rng.integers(-2, 3, C).astype(F32)
    sl[0] = -2
    if C > 1:
        sl[C - 1] = 0
    return data, sl, np.array(-2, F32)


def random_inputs(case, seed=0):
    """Trained-like: normal activations whose deviation differs per channel by up to 30x, slopes around 0.25 with a fifth of
    them negative."""
    C, h, w = case
    rng = np.random.default_rng(7 * C + 3 * h + w + seed)
    cd = D.data_channels(C)
    data = (rng.normal(0, 1, (1, cd, h, w)) * np.exp(rng.uniform(-1.7, 1.7, (1, cd, 1, 1)))).astype(F32)
    sl = (rng.normal(0.25, 0.1, C) * np.where(rng.uniform(0, 1, C) < 0.2, -1.0, 1.0)).astype(F32)
    return data, sl


def library_inputs(case, seed=0):
    """The grid of the library ops: half of it uniform in [-LIMIT, LIMIT], half of it +-2^u with u uniform in [-20, log2 LIMIT],
    and SPECIALS (0, +-2^-20, +-1, +-LIMIT) planted at the front of every channel plane that has the room, rotated by the
    channel's index so that a one-pixel map holds them across its channels."""
    C, h, w = case
    rng = np.random.default_rng(31 * C + 5 * h + w + seed)
    cd = D.data_channels(C)
    lin = rng.uniform(-LIMIT, LIMIT, (1, cd, h, w))
    geo = np.exp2(rng.uniform(-20, math.log2(LIMIT), (1, cd, h, w))) * rng.choice([-1.0, 1.0], (1, cd, h, w))
    data = np.where(rng.uniform(0, 1, lin.shape) < 0.5, lin, geo).astype(F32).reshape(cd, h * w)
    k = min(h * w, len(SPECIALS))
    for c in range(cd):
        data[c, :k] = np.roll(np.asarray(SPECIALS, F32), -c)[:k]
    return data.reshape(1, cd, h, w)


def feeder_params(case):
    """Parameters of `pre` / `sel`, and the channels of `data` that the layers read (in their channel order)."""
    return D.feeder_params(case[0])


# ---- the oracle net -------------------------------------------------------------------------------------------------------------
def oracle_value(spec, x, slope=None):
    """What the oracle net holds: ``neuron32`` for the exact ops, fp32(``neuron64``) for the others."""
    return neuron32(spec, x, slope) if is_exact(spec) else neuron64(spec, x, slope).astype(F32)


class NeuronOracleNet(N.NormOracleNet):
    """``NormOracleNet`` plus the ten neuron layers (``oracle_value``; an in-place layer replaces its blob)."""

    def forward(self, **kwargs):
        if kwargs:
            assert set(kwargs.keys()) == set(self.inputs)
            for in_, blob in kwargs.items():
                self.blobs[in_].data[...] = blob
        every, snaps = self.layers, {}
        try:
            for L in every:
                t, name = str(L.get("type")), str(L.get("name"))
                if t not in TYPES:
                    self.layers = [L]
                    N.NormOracleNet.forward(self)
                    snaps.update(self.snapshots)
                    continue
                top = str(L.get("top"))
                out = oracle_value(layer_spec(L), self.blobs[str(L.get("bottom"))].data, self.params[name][0] if t == "PReLU" else None)
                self.blobs[top].data = np.ascontiguousarray(out, dtype=F32)
                snaps[(name, top)] = self.blobs[top].data
        finally:
            self.layers = every
        self.snapshots = snaps
        return {o: self.blobs[o].data for o in self.outputs}


def forwarded(onet, data, info):
    onet.blobs["data"].reshape(*data.shape)
    onet.blobs["im_info"].reshape(*info.shape)
    onet.forward(data=data, im_info=info)
    return onet


def graph_params(msg, seed=5, cls_bias=1.0):
    """``O.synth_params`` plus every PReLU layer's blob from its filler, and seeded blobs for BatchNorm (a mean around 0, a
    variance around 1, the factor 1) and Scale (gamma in +-[0.5, 1.5], beta ~ N(0, 0.5))."""
    params = O.synth_params(msg, seed=seed, cls_bias=cls_bias)
    params.update(filler_params(msg))
    rng = np.random.default_rng(seed + 3)
    ch = O.infer_channels(msg)
    for L in msg.getall("layer"):
        t, name, C = str(L.get("type")), str(L.get("name")), ch.get(str(L.get("bottom")))
        if t == "BatchNorm":
            params[name] = [rng.normal(0, 0.2, C).astype(F32), rng.uniform(0.5, 1.5, C).astype(F32), np.ones(1, F32)]
        elif t == "Scale":
            sp = L.get("scale_param")
            g = (rng.uniform(0.5, 1.5, C) * np.where(rng.uniform(0, 1, C) < 0.2, -1.0, 1.0)).astype(F32)
            params[name] = [g] + ([rng.normal(0, 0.5, C).astype(F32)] if sp is not None and str(sp.get("bias_term", "false")) == "true" else [])
    return params


# ---- graphs -----------------------------------------------------------------------------------------------------------------
NB_BLOBS = ["c1", "c2", "c2b"]


def neighbours_text(h, w, relu=True, fill=None):
    """Split-fp16 neighbours on the fused path: `c0` (3 -> 64, ReLU) and `c1` (64 -> 128; ``relu``: with its in-place ReLU);
    PReLU `pr` in place on `c1`; `c2` and `c2b`, 3x3 128-channel family convolutions of the rewritten `c1` -- without the PReLU
    `c1` would be a split-format blob, rewritten by it it stays plain fp32; `H.mini_detector`'s per-blob tail on the two."""
    txt = (G.conv_txt("c0", "data", 64, 3, 1, 1, 1, relu=True) + G.conv_txt("c1", "c0", 128, 3, 1, 1, 1, relu=relu) +
           neuron_layer("pr", ("PReLU", {} if fill is None else {"fill": fill}), "c1") + G.conv_txt("c2", "c1", 128, 3, 1, 1, 1, relu=True) +
           G.conv_txt("c2b", "c1", 128, 3, 1, 1, 1, relu=True))
    return H.mini_detector(txt, ["c2", "c2b"], 2, 3, h, w)


RANGE_BLOBS = ["c1", "n", "c2", "c2b"]


def range_text(h, w, scale=1.0e5):
    """`c1` -> Power `n` (``scale``) -> `c2`; `c2b` on `c1` itself."""
    txt = (G.conv_txt("c0", "data", 64, 3, 1, 1, 1, relu=True) + G.conv_txt("c1", "c0", 128, 3, 1, 1, 1, relu=True) +
           neuron_layer("n", ("Power", {"scale": scale}), "c1", "n") + G.conv_txt("c2", "n", 128, 3, 1, 1, 1, relu=True) +
           G.conv_txt("c2b", "c1", 128, 3, 1, 1, 1, relu=True))
    return H.mini_detector(txt, ["c2", "c2b"], 2, 3, h, w)


def head_text(h, w):
    """A Sigmoid top as the head blob of a ProposalLayer: `H.mini_detector`'s 1x1 predictors directly on `n`."""
    txt = (G.conv_txt("c0", "data", 64, 3, 1, 1, 1, relu=True) + G.conv_txt("c1", "c0", 128, 3, 1, 1, 1) +
           neuron_layer("n", ("Sigmoid", {}), "c1", "n"))
    return H.mini_detector(txt, "n", 2, 3, h, w)


# A MobileFaceNet-shaped mini detector: a stride-2 stem, depthwise / pointwise pairs, every convolution without a bias and
# followed by BatchNorm, Scale and PReLU in place, a squeeze-free two-class tail on the 128-channel map of stride 4.
MFN_SIZE = (48, 64)
MFN_GROUP_SIZES = [(48, 64), (41, 56), (33, 47)]
MFN_SEED, MFN_THRESH, MFN_MIN_SIZE = 21, 0.5, 2.0
MFN_PRELUS = ("stem", "dw1", "pw1", "dw2", "pw2", "dw3", "f4")
MFN_BLOBS = ("stem", "dw1", "pw1", "dw2", "pw2", "dw3", "f4")


def _mfn_unit(name, bottom, nout, k, stride=1, pad=0, group=None, top=None):
    top = top or name
    return (G.conv_txt(name, bottom, nout, k, stride, pad, 1, False, False, group=group, top=top) + N.bn_layer("bn_" + name, top) +
            N.scale_layer("scale_" + name, top) + neuron_layer("prelu_" + name, ("PReLU", {}), top))


def mfn_text(h, w):
    txt = (_mfn_unit("stem", "data", 64, 3, 2, 1) + _mfn_unit("dw1", "stem", 64, 3, 1, 1, group=64) + _mfn_unit("pw1", "dw1", 64, 1) +
           _mfn_unit("dw2", "pw1", 64, 3, 2, 1, group=64) + _mfn_unit("pw2", "dw2", 128, 1) +
           _mfn_unit("dw3", "pw2", 128, 3, 1, 1, group=128) + _mfn_unit("pw3", "dw3", 128, 1, top="f4"))
    return H.mini_detector(txt, "f4", 4, 3, h, w)


def mfn_unit(h, w, seed=4):
    return H.synth_image_blob(h, w, seed=seed + h), np.array([[h - 3, w - 3, 0.75]], F32)


_MFN = {}


def mfn_params():
    """Seeded parameters (computed once): ``graph_params``, the PReLU slopes around 0.25 with a fifth of them negative."""
    if "p" not in _MFN:
        msg = P.parse(mfn_text(*MFN_SIZE))
        p = graph_params(msg, seed=MFN_SEED, cls_bias=1.0)
        rng = np.random.default_rng(MFN_SEED)
        for name, blobs in p.items():
            if name.startswith("prelu_"):
                C = blobs[0].shape[0]
                blobs[0][...] = rng.normal(0.25, 0.1, C) * np.where(rng.uniform(0, 1, C) < 0.2, -1.0, 1.0)
        _MFN["p"] = p
    return _MFN["p"]


def mfn_oracle(h=MFN_SIZE[0], w=MFN_SIZE[1]):
    return NeuronOracleNet(P.parse(mfn_text(h, w)), params=mfn_params(), proposal_cfg=O.ProposalParams(
        pre_nms_topN=10000, score_thresh=MFN_THRESH, min_size=MFN_MIN_SIZE))


# ---- the field census (tests/golden/caffe_neuron_fields.json, names only) ------------------------------------------------------
HONOURED, REFUSED, INERT = "HONOURED", "REFUSED", "INERT"
VC, VHW = 16, (5, 7)                     # the value cases' and refusals' blob: 16 channels of 5 x 7


def field_net(layers_txt):
    return H.single_layer_net(G.conv_txt("pre", "data", VC, 1) + layers_txt, VC, *VHW)


def _vt(spec):
    return field_net(neuron_layer("n", spec, "pre", "n"))


class Value(object):
    """`text` holds the field at a non-default value, `twin` at its default: the two results differ, and each matches the
    reference.  ``slopes``: what is loaded into the PReLU blob of (text, twin), None: the fresh blob's filler value stays."""

    def __init__(self, message, field, spec, twin, slopes=(None, None)):
        self.message, self.field, self.spec, self.twin_spec, self.slopes = message, field, spec, twin, slopes
        self.text, self.twin = _vt(spec), _vt(twin)


VALUE_CASES = {
    "prelu_filler": Value("PReLUParameter", "filler", ("PReLU", {"fill": 0.5}), ("PReLU", {})),
    "prelu_channel_shared": Value("PReLUParameter", "channel_shared", ("PReLU", {"shared": True}), ("PReLU", {"shared": False}),
                                  slopes=(np.array(-2, F32), np.linspace(-1, 2, VC).astype(F32))),
    "elu_alpha": Value("ELUParameter", "alpha", ("ELU", {"alpha": 0.5}), ("ELU", {})),
    "threshold_threshold": Value("ThresholdParameter", "threshold", ("Threshold", {"threshold": 2.5}), ("Threshold", {})),
    "power_power": Value("PowerParameter", "power", ("Power", {"power": 2}), ("Power", {})),
    "power_scale": Value("PowerParameter", "scale", ("Power", {"scale": 3}), ("Power", {})),
    "power_shift": Value("PowerParameter", "shift", ("Power", {"shift": -2}), ("Power", {})),
    "exp_base": Value("ExpParameter", "base", ("Exp", {"base": 2}), ("Exp", {})),
    "exp_scale": Value("ExpParameter", "scale", ("Exp", {"scale": 0.5}), ("Exp", {})),
    "exp_shift": Value("ExpParameter", "shift", ("Exp", {"shift": 1}), ("Exp", {})),
    "log_base": Value("LogParameter", "base", ("Log", {"base": 2}), ("Log", {})),
    "log_scale": Value("LogParameter", "scale", ("Log", {"scale": 2}), ("Log", {})),
    "log_shift": Value("LogParameter", "shift", ("Log", {"shift": 3}), ("Log", {})),
}


def value_data(seed=0):
    """Integers in [1, 5] with both signs for the ops that take them; Log's and Power's cases read the magnitudes."""
    rng = np.random.default_rng(77 + seed)
    return (rng.integers(1, 6, (1, VC) + VHW) * rng.choice([-1, 1], (1, VC) + VHW)).astype(F32)


def value_input(spec):
    d = value_data()
    return np.abs(d) if spec[0] in ("Log",) or (spec[0] == "Power" and fields(spec)["power"] != 1.0) else d


class Refusal(object):
    """`layers` (behind `pre`, `b0`, `b1` and the 3-D `rs` of ``refusal_net``) is refused at caffe.Net() with a message matching
    `match`: the layer's type and name, and the field or the rule."""

    def __init__(self, layers, match):
        self.layers, self.match = layers, match


RESHAPE_3D = 'layer { name: "rs" type: "Reshape" bottom: "b0" top: "rs" reshape_param { shape { dim: 1 dim: -1 dim: 5 } } }\n'
BARE = 'layer { name: "%s" type: "%s" %s }\n'


def refusal_net(layers_txt):
    return H.single_layer_net(G.conv_txt("pre", "data", 16, 1) + G.conv_txt("b0", "pre", 8, 1) + G.conv_txt("b1", "pre", 8, 1) +
                              RESHAPE_3D + layers_txt, 16, 3, 5)


def _rf(name, spec):
    return neuron_layer(name, spec, "b0", "y")


REFUSALS = {
    "elu_alpha_nan": Refusal(_rf("e_nan", ("ELU", {"alpha": "nan"})), r"ELU 'e_nan'.*alpha"),
    "elu_alpha_huge": Refusal(_rf("e_huge", ("ELU", {"alpha": "1e39"})), r"ELU 'e_huge'.*alpha"),
    "threshold_inf": Refusal(_rf("t_inf", ("Threshold", {"threshold": "inf"})), r"Threshold 't_inf'.*threshold"),
    "power_power_nan": Refusal(_rf("p_pow", ("Power", {"power": "nan"})), r"Power 'p_pow'.*power"),
    "power_scale_inf": Refusal(_rf("p_scale", ("Power", {"scale": "-inf"})), r"Power 'p_scale'.*scale"),
    "power_shift_huge": Refusal(_rf("p_shift", ("Power", {"shift": "1e39"})), r"Power 'p_shift'.*shift"),
    "exp_base_zero": Refusal(_rf("x_zero", ("Exp", {"base": 0})), r"Exp 'x_zero'.*base"),
    "exp_base_negative": Refusal(_rf("x_neg", ("Exp", {"base": -2})), r"Exp 'x_neg'.*base"),
    "exp_base_one": Refusal(_rf("x_one", ("Exp", {"base": 1})), r"Exp 'x_one'.*base"),
    "exp_base_inf": Refusal(_rf("x_inf", ("Exp", {"base": "inf"})), r"Exp 'x_inf'.*base"),
    "exp_scale_nan": Refusal(_rf("x_scale", ("Exp", {"scale": "nan"})), r"Exp 'x_scale'.*scale"),
    "exp_shift_inf": Refusal(_rf("x_shift", ("Exp", {"shift": "inf"})), r"Exp 'x_shift'.*shift"),
    "log_base_zero": Refusal(_rf("l_zero", ("Log", {"base": 0})), r"Log 'l_zero'.*base"),
    "log_base_negative": Refusal(_rf("l_neg", ("Log", {"base": -0.5})), r"Log 'l_neg'.*base"),
    "log_base_one": Refusal(_rf("l_one", ("Log", {"base": 1})), r"Log 'l_one'.*base"),
    "log_scale_nan": Refusal(_rf("l_scale", ("Log", {"scale": "nan"})), r"Log 'l_scale'.*scale"),
    "log_shift_inf": Refusal(_rf("l_shift", ("Log", {"shift": "inf"})), r"Log 'l_shift'.*shift"),
    # values that are not of the field's type
    "type_alpha_word": Refusal(_rf("e_word", ("ELU", {"alpha": "abc"})), r"'e_word'.*alpha: 'abc' is not a number"),
    "type_power_tail": Refusal(_rf("p_tail", ("Power", {"power": "2x"})), r"'p_tail'.*power: '2x' is not a number"),
    "type_channel_shared": Refusal(BARE % ("pr_yes", "PReLU", 'bottom: "b0" top: "y" prelu_param { channel_shared: yes }'),
                                   r"'pr_yes'.*channel_shared: 'yes' is not a bool"),
    "type_filler_value": Refusal(_rf("pr_val", ("PReLU", {"filler": 'type: "constant" value: half'})), r"'pr_val'.*filler.value: 'half' is not a number"),
    # NeuronLayer's shape rules, by every type
    "sigmoid_two_tops": Refusal(BARE % ("s_tops", "Sigmoid", 'bottom: "b0" top: "t1" top: "t2"'), r"Sigmoid 's_tops'.*exactly one bottom and one top"),
    "tanh_two_bottoms": Refusal(BARE % ("t_bots", "TanH", 'bottom: "b0" bottom: "b1" top: "y"'), r"TanH 't_bots'.*exactly one bottom and one top"),
    "absval_net_input": Refusal(neuron_layer("a_in", ("AbsVal", {}), "data", "y"), r"AbsVal 'a_in'.*'data' is a net input"),
    "bnll_flat_input": Refusal(neuron_layer("b_flat", ("BNLL", {}), "im_info", "y"), r"BNLL 'b_flat'.*'im_info'"),
    "prelu_3d": Refusal(neuron_layer("pr_3d", ("PReLU", {}), "rs", "y"), r"PReLU 'pr_3d'.*'rs' is not 4-D"),
    "sigmoid_3d": Refusal(neuron_layer("s_3d", ("Sigmoid", {}), "rs", "y"), r"Sigmoid 's_3d'.*'rs' is not 4-D"),
    "prelu_member_after_concat": Refusal(F.concat_layer("cc", ["b0", "b1"]) + neuron_layer("pr_member", ("PReLU", {}), "b1"),
                                         r"PReLU 'pr_member'.*in place after Concat 'cc'"),
    "power_member_after_concat": Refusal(F.concat_layer("cc", ["b0", "b1"]) + neuron_layer("p_member", ("Power", {"scale": -1}), "b1"),
                                         r"Power 'p_member'.*in place after Concat 'cc'"),
}

_ENGINE = "picks Caffe's or cuDNN's implementation of the same function"
DISPOSITION = {(c.message, c.field): (HONOURED, name) for name, c in VALUE_CASES.items()}
DISPOSITION.update({("SigmoidParameter", "engine"): (INERT, _ENGINE), ("TanHParameter", "engine"): (INERT, _ENGINE)})
# accepted: the inert fields written out
ACCEPTED = {
    "sigmoid_engine": field_net(BARE % ("n", "Sigmoid", 'bottom: "pre" top: "n" sigmoid_param { engine: CAFFE }')),
    "tanh_engine": field_net(BARE % ("n", "TanH", 'bottom: "pre" top: "n" tanh_param { engine: CUDNN }')),
}


def census():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "caffe_neuron_fields.json")) as f:
        return json.load(f)
