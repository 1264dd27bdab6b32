"""Operand models of the convolution kernels in every conv mode (test infrastructure, numpy float64).

What a convolution layer computes in the modes "fp32", "f16x3", "f16x2", "f16" and "bf16", restated from the kernels
(smallhardface_amd/csrc/conv_f16x3*.h, conv.hip) as: which 16-bit OPERANDS are formed from the fp32 activations and
weights, which PRODUCTS of them are summed, and how the sums are scaled back.  The accumulation itself is not modelled:
on inputs for which every product and every partial sum is exactly representable in fp32 (tests/conv_mode_cases.py builds
such inputs, `exactness` checks them) the order of summation and the MFMA's internal rounding do not matter, the result
is ONE number, and a kernel must give it bit for bit.

Operands.  fp16(x) is round-to-nearest-even (np.float16), bf16(x) round-to-nearest-even on the bit pattern.
  * split activations / weights of the two-accumulator kernels (the 8-wave kernel, conv1_2 inside the fused first pair
    `_pc`, conv1_1 inside `_pc`): hi = fp16(x), lo = fp16((x - hi) * 2^11).
  * single-accumulator kernels (the dual-tile family with its slim and dilated forms, the 1x1 GEMM `_k1`, the three-heads
    kernel `_h3`): weights are lifted by one power of two s per layer (max |w| s in [8, 16), exponent clamped to +-14):
    hi = fp16(w s), lo = fp16(w s - hi), unscaled.  Activations: hi and the format's lo (x 2^11) as above -- formed by the
    kernel from fp32 input, or read as stored by the producer's split epilogue (IN_SPLIT) -- then hi 2^e and lo 2^(e - 11),
    each one fp16 multiplication, with the unit's activation exponent e (max |input| 2^e in [2^13, 2^14), 0 <= e <= 15).
  * bf16 mode: bf16(a) and bf16(w), no lift, no exponent, no low parts.
Products.  3: a_hi w_hi + a_hi w_lo + a_lo w_hi (a_lo w_lo is never formed); 2: a_lo w_hi is dropped; 1: a_hi w_hi only;
bf16: bf16(a) bf16(w).  The two-accumulator kernels sum a_hi w_hi in `main` and the lo products (which carry 2^11) in
`corr`: out = fma(corr, 2^-11, main).  The single-accumulator kernels sum all products in one accumulator:
out = acc * (2^-e / s).  Then + bias (one fp32 addition), ReLU, and where the graph has one the 2x2 / 2 max pool with
windows clipped at the ragged edge (a selection: no arithmetic).
Split activations on the fused path: an `out_split` / `pool_split` epilogue stores exactly these hi and lo (x 2^11) halves
of the value it would have stored as fp32; an IN_SPLIT consumer reads both halves at three products and the hi half only
at two or one -- fp16 of the producer's value, what it would have formed itself from fp32 input.
conv1_1.  Inside the fused first pair `_pc` it runs on the matrix cores and ALWAYS forms the three products of the split
image and the split weights (two accumulators; `NP` only selects conv1_2's products); under BF one bf16 product.  Not
fused -- conv_first_kernel in every mode, and the 8-wave kernel's FUSE1 halo staging -- it is fp32 fused multiply-adds.
The FUSE1 form exists for three products only: in "f16x2" and "f16" mode a first pair that `_pc` does not take (conv1_2
with Cout != 64) still runs conv1_2 at three products; in bf16 mode such a pair is not fused.
Layers outside the split kernels (ineligible shapes, every layer in fp32 mode) are fp32 fused multiply-adds or fp32
MFMAs: the exact sum where that is representable.

`layer_rule` restates which of these a layer of a graph runs on, per mode and path (net_forward.cpp conv_args,
conv_f16x3.hip plan_conv_f16x3); `net_model` chains the layers of a graph.  The `wrong` argument of `conv_model` builds
deliberately wrong variants (one product too few / too many, truncation instead of rounding, the odd element of a bf16
pair replaced by the even one, one tap shifted in the last column): tests use them to show that a comparison against the
model would notice.
"""
import numpy as np

try:
    from scipy import sparse as _sparse
except ImportError:      # (only a faster way to the same sums)
    _sparse = None

MODES = ("fp32", "f16x3", "f16x2", "f16", "bf16")
NPROD = {"f16x3": 3, "f16x2": 2, "f16": 1, "bf16": 1}
F64 = np.float64


# ------------------------------------------------------------------------------------------------------------
# conversions
# ------------------------------------------------------------------------------------------------------------
def f32(x):
    return np.asarray(x, F64).astype(np.float32).astype(F64)


def is_f32(x):
    x = np.asarray(x, F64)
    return bool(np.array_equal(x.astype(np.float32).astype(F64), x))


def f16(x, trunc=False):
    """fp32 -> fp16, round to nearest even (`trunc`: toward zero), as float64."""
    x32 = np.asarray(x, F64).astype(np.float32)
    with np.errstate(over="ignore"):
        h = x32.astype(np.float16)
    if trunc:
        big = np.abs(h.astype(F64)) > np.abs(x32.astype(F64))
        h = np.where(big, np.nextafter(h, np.float16(0)), h)
    return h.astype(F64)


def bf16(x, trunc=False):
    """fp32 -> bf16, round to nearest even on the bit pattern (`trunc`: the low 16 bits cut off), as float64."""
    u = np.ascontiguousarray(np.asarray(x, F64).astype(np.float32)).view(np.uint32).astype(np.uint64)
    if not trunc:
        u = u + np.uint64(0x7fff) + ((u >> np.uint64(16)) & np.uint64(1))
    u = (u & np.uint64(0xffff0000)).astype(np.uint32)
    return u.view(np.float32).astype(F64)


def _odd_from_even(x):
    """The channel-pair bug of a packed conversion: element 2j + 1 replaced by element 2j (axis 0 = channels)."""
    y = np.array(x, F64)
    n = y[1::2].shape[0]
    y[1::2] = y[0::2][:n]
    return y


def split_hi_lo(x, trunc=False):
    """(hi, lo x 2^11): hi = fp16(x), lo = fp16((x - hi) * 2^11) -- the split activation format and the 8-wave packs."""
    x = f32(x)
    hi = f16(x, trunc)
    return hi, f16((x - hi) * 2048.0, trunc)


def weight_lift_exponent(w):
    """pack_conv_weights_split16h: e with max |w| 2^e in [8, 16), clamped to [-14, 14]; 0 for an all-zero layer."""
    amax = float(np.abs(np.asarray(w, F64)).max()) if np.size(w) else 0.0
    e = int(np.floor(np.log2(8.0 / amax))) if amax > 0 else 0
    return max(-14, min(14, e))


def act_exponent(amax):
    """conv_act_exponent_of_bits: e >= 0 with amax 2^e in [2^13, 2^14), capped at 15; 0 for zero / unknown / not finite."""
    amax = float(np.float32(amax))
    if not (amax > 0) or not np.isfinite(amax):
        return 0
    return max(0, min(15, 13 - int(np.floor(np.log2(amax)))))


# ------------------------------------------------------------------------------------------------------------
# the sum over taps and channels, in float64 (exact on the grids)
# ------------------------------------------------------------------------------------------------------------
def corr(a, w, dil=1, shift_last_col=False):
    """'same' cross-correlation: a (C, H, W), w (O, C, k, k), pad = dil (k - 1) / 2 -> (O, H, W).
    `shift_last_col` (a wrong model): in the last output column the tap (k // 2, 0) reads one pixel to the right."""
    a, w = np.asarray(a, F64), np.asarray(w, F64)
    C, H, W = a.shape
    O, _, k, _ = w.shape
    pad = dil * (k - 1) // 2
    ap = np.zeros((C, H + 2 * pad + 1, W + 2 * pad + 1), F64)
    ap[:, pad:pad + H, pad:pad + W] = a
    taps = [(ky, kx) for ky in range(k) for kx in range(k) if w[:, :, ky, kx].any()]
    if not taps:
        return np.zeros((O, H, W), F64)
    cols = np.empty((len(taps), C, H, W), F64)
    for t, (ky, kx) in enumerate(taps):
        cols[t] = ap[:, ky * dil:ky * dil + H, kx * dil:kx * dil + W]
        if shift_last_col and ky == k // 2 and kx == 0:
            cols[t, :, :, W - 1] = ap[:, ky * dil:ky * dil + H, kx * dil + W]
    wm = np.stack([w[:, :, ky, kx] for ky, kx in taps], axis=1).reshape(O, len(taps) * C)
    cols = cols.reshape(len(taps) * C, H * W)
    # (the test layers have 64 non-zero weights per output channel: a sparse product when scipy is there -- the same exact
    # sums, a fraction of the work)
    if _sparse is not None and np.count_nonzero(wm) < 0.2 * wm.size:
        return np.asarray(_sparse.csr_matrix(wm) @ cols).reshape(O, H, W)
    return (wm @ cols).reshape(O, H, W)


def max_pool_2x2(x):
    """2x2 / 2 MAX pool, ceil mode: windows on a ragged edge are clipped (pooling_layer.cu:11-47)."""
    C, H, W = x.shape
    Hp, Wp = (H + 1) // 2, (W + 1) // 2
    xp = np.full((C, 2 * Hp, 2 * Wp), -np.inf, F64)
    xp[:, :H, :W] = x
    return xp.reshape(C, Hp, 2, Wp, 2).max(axis=(2, 4))


# ------------------------------------------------------------------------------------------------------------
# one convolution layer
# ------------------------------------------------------------------------------------------------------------
def product_groups(a, w, arith, nprod=3, bf=False, e_act=0, wrong=None):
    """[(scale, [(A, Wt), ...]), ...]: the accumulators of a layer -- each a sum of correlations of an activation operand
    with a weight operand -- and the power of two each is multiplied by in the epilogue.
    arith: "fp32" (exact kernels: the operands themselves), "w8" (two accumulators), "fam" (one accumulator)."""
    a, w = f32(a), f32(w)
    trunc = wrong == "trunc"
    if arith == "fp32":
        return [(1.0, [(a, w)])]
    if bf:
        ab = bf16(a, trunc)
        if wrong == "odd_lane":
            ab = _odd_from_even(ab)
        return [(1.0, [(ab, bf16(w, trunc))])]
    nprod = int(nprod) + (1 if wrong == "more" else -1 if wrong == "fewer" else 0)
    assert 0 <= nprod <= 4
    a_hi, a_lo = split_hi_lo(a, trunc)
    if arith == "w8":
        w_hi, w_lo = split_hi_lo(w, trunc)
        main = [(a_hi, w_hi)] if nprod >= 1 else []
        cor = ([(a_hi, w_lo)] if nprod >= 2 else []) + ([(a_lo, w_hi)] if nprod >= 3 else [])
        groups = [(1.0, main), (2.0 ** -11, cor)]
        if nprod >= 4:
            groups.append((2.0 ** -22, [(a_lo, w_lo)]))
        return groups
    assert arith == "fam", arith
    s = 2.0 ** weight_lift_exponent(w)
    ws = f32(w * s)
    w_hi = f16(ws, trunc)
    w_lo = f16(ws - w_hi, trunc)
    A_hi = f16(a_hi * 2.0 ** e_act)
    A_lo = f16(a_lo * 2.0 ** (e_act - 11))
    pairs = [(A_hi, w_hi)][:nprod] + ([(A_hi, w_lo)] if nprod >= 2 else []) + ([(A_lo, w_hi)] if nprod >= 3 else [])
    if nprod >= 4:
        pairs.append((A_lo, w_lo))
    return [(2.0 ** -e_act / s, pairs)]


def _quantum(x):
    """The largest power of two that divides every element of x (1.0 for all zeros)."""
    x = np.abs(np.asarray(x, F64))
    x = x[x > 0]
    if x.size == 0:
        return 1.0
    m, e = np.frexp(x)                       # x = m 2^e, m in [0.5, 1): an integer multiple of 2^(e - 53)
    mi = (m * 2.0 ** 53).astype(np.int64)
    low = mi & -mi
    return float(2.0 ** (np.log2(low.astype(F64)) + e - 53).min())


def exactness(groups, bias, dil=1):
    """Bits the widest accumulator needs: max over outputs of sum |A| |Wt| / (quantum of the products), per group, as
    log2.  Below 24 every partial sum in any order is an fp32 number.  Also checks that the epilogue's roundings (scale,
    sum of the accumulators, bias) are exact.  Returns the largest log2."""
    worst = 0.0
    total = None
    for scale, pairs in groups:
        if not pairs:
            continue
        live = [(A, Wt) for A, Wt in pairs if np.any(A) and np.any(Wt)]      # (an all-zero operand adds nothing)
        q = min([_quantum(A) * _quantum(Wt) for A, Wt in live] or [1.0])
        bound = sum(corr(np.abs(A), np.abs(Wt), dil) for A, Wt in pairs)
        worst = max(worst, float(np.log2(max(bound.max() / q, 1.0))))
        acc = sum(corr(A, Wt, dil) for A, Wt in pairs)
        assert is_f32(acc) and is_f32(acc * scale), "an accumulator is not an fp32 number"
        total = acc * scale if total is None else total + acc * scale
    assert is_f32(total), "the sum of the accumulators is not an fp32 number"
    if bias is not None:
        assert is_f32(total + np.asarray(bias, F64)[:, None, None]), "output + bias is not an fp32 number"
    return worst


def conv_model(a, w, bias, arith, nprod=3, bf=False, dil=1, relu=True, e_act=0, wrong=None):
    """The layer's output (O, H, W) as float32: the accumulators of `product_groups`, the epilogue's scale, the sum
    main + corr 2^-11 rounded once (an fma), + bias rounded once, ReLU."""
    groups = product_groups(a, w, arith, nprod, bf, e_act, wrong)
    total = None
    for scale, pairs in groups:
        if not pairs:
            continue
        acc = f32(sum(corr(A, Wt, dil, wrong == "edge") for A, Wt in pairs))
        total = acc * scale if total is None else total + acc * scale
    if total is None:
        total = np.zeros((np.shape(w)[0],) + np.shape(a)[1:], F64)
    v = f32(total)
    if bias is not None:
        v = f32(v + f32(bias)[:, None, None])
    if relu:
        v = np.maximum(v, 0.0)
    return (v + 0.0).astype(np.float32)          # (+ 0.0: the ReLU's -0 -> +0 on the bit patterns)


def conv_scalar(a, w, bias, arith, nprod, bf, dil, relu, e_act, co, y, x, groups=None):
    """One output element by a plain loop over taps and channels (the brute-force restatement of `conv_model`), and the
    list of its product terms per accumulator: (value as float32, [(scale, [terms]), ...])."""
    groups = product_groups(a, w, arith, nprod, bf, e_act) if groups is None else groups
    k = np.shape(w)[2]
    pad = dil * (k - 1) // 2
    C, H, W = np.shape(a)
    out, total = [], 0.0
    for scale, pairs in groups:
        terms = []
        for A, Wt in pairs:
            for c in range(C):
                for ky in range(k):
                    for kx in range(k):
                        iy, ix = y - pad + ky * dil, x - pad + kx * dil
                        if 0 <= iy < H and 0 <= ix < W and Wt[co, c, ky, kx] != 0 and A[c, iy, ix] != 0:
                            terms.append(float(A[c, iy, ix]) * float(Wt[co, c, ky, kx]))
        out.append((scale, terms))
        total += float(np.float32(sum(terms))) * scale
    v = float(np.float32(total))
    if bias is not None:
        v = float(np.float32(v + float(np.float32(bias[co]))))
    if relu:
        v = max(v, 0.0)
    return np.float32(v), out


# ------------------------------------------------------------------------------------------------------------
# graphs: which kernel class a layer runs on, and the chain
# ------------------------------------------------------------------------------------------------------------
def eligible(cin, cout, k, dil):
    """conv_f16x3_eligible (pad = dil for 3x3, 0 for 1x1 throughout the test graphs)."""
    return cin % 32 == 0 and cout % 64 == 0 and (k == 1 or (k == 3 and dil in (1, 2, 4)))


def family_shape(cin, cout, k, bf, aligned=True):
    """The layer goes to a single-accumulator kernel (family, `_k1`): conv_f16x3_family_shape + plan_conv_f16x3."""
    if not aligned or cin < 64:
        return False
    return (cout % 256 == 0 and not bf) if k == 1 else cout % 128 == 0


def layer_rule(L, graph, mode, fused, products=None):
    """How conv layer L of `graph` (a list of layer dicts, see tests/conv_mode_cases.py) runs in `mode` on the per-layer
    (`fused` False) or the fused path: dict(arith, nprod, bf, first) with
      first = None | "fp32" | "pc": the layer also computes its producer, the net's first convolution, in its halo
      staging -- in fp32 (8-wave FUSE1 form) or on the matrix cores (`_pc`).
    A first convolution that is absorbed gets arith "absorbed"."""
    products = products or {}
    by_top = {M["name"]: M for M in graph}
    readers = lambda name: [M for M in graph if M.get("bottom") == name]
    is_first = lambda M: M["op"] == "conv" and M["bottom"] == "data"
    split = mode != "fp32"
    bf = mode == "bf16"

    def absorbs(M):      # net_graph.cpp first_src + shf_net::absorbs_first
        F = by_top.get(M["bottom"])
        if not (fused and split and F is not None and is_first(F)):
            return False
        if not (F["relu"] and F["k"] == 3 and F["dil"] == 1 and F["nout"] == 64 and len(readers(F["name"])) == 1):
            return False
        if not eligible(64, M["nout"], M["k"], M["dil"]):
            return False
        return (not bf) or M["nout"] == 64

    if is_first(L):
        rd = readers(L["name"])
        if len(rd) == 1 and rd[0]["op"] == "conv" and absorbs(rd[0]):
            return dict(arith="absorbed", nprod=0, bf=False, first=None)
        return dict(arith="fp32", nprod=0, bf=False, first=None)       # conv_first_kernel: fp32 FMAs in every mode
    cin = L["cin"]
    if not split or not eligible(cin, L["nout"], L["k"], L["dil"]):
        return dict(arith="fp32", nprod=0, bf=False, first=None)
    nprod = 1 if bf else int(products.get(L["name"], NPROD[mode]))
    if absorbs(L):
        if L["nout"] == 64 and L.get("aligned", True):
            return dict(arith="w8", nprod=nprod, bf=bf, first="pc")
        # the 8-wave FUSE1 form is built for three products only (kernel table w8_fuse1): every fp16 mode runs it
        return dict(arith="w8", nprod=3, bf=False, first="fp32")
    arith = "fam" if family_shape(cin, L["nout"], L["k"], bf, L.get("aligned", True)) else "w8"
    return dict(arith=arith, nprod=nprod, bf=bf, first=None)


def first_conv_model(img, w, bias, how, bf=False, relu=True, wrong=None):
    """The net's first convolution (3 channels in).  how "fp32": conv_first_kernel and the 8-wave kernel's halo staging --
    fp32 fused multiply-adds; "pc": inside the fused first pair on the matrix cores -- ALWAYS three products of the
    split image and the split weights in the fp16 modes (whatever the pair's conv1_2 forms), one bf16 product in bf16."""
    if how == "fp32":
        return conv_model(img, w, bias, "fp32", relu=relu)
    return conv_model(img, w, bias, "w8", 3, bf, relu=relu, wrong=wrong)


def net_model(graph, params, data, mode, fused, products=None, wrong=None, wrong_layer=None, inputs=None):
    """{blob: (C, H, W) float32} of `graph` on image `data` (3, H, W).  `inputs`: blobs given from outside (the bits a
    layer's input held on the GPU) instead of being computed.  `wrong` applies to `wrong_layer` only."""
    blobs = {"data": np.asarray(data, np.float32)}
    amax = {}
    given = dict(inputs or {})
    for L in graph:
        name = L["name"]
        if name in given:
            blobs[name] = np.asarray(given[name], np.float32)
            amax[name] = float(np.abs(blobs[name]).max())
            continue
        if L["op"] == "pool":
            blobs[name] = max_pool_2x2(blobs[L["bottom"]].astype(F64)).astype(np.float32)
            amax[name] = amax.get(L["bottom"], 0.0)             # the un-pooled map's maximum serves as the bound
            continue
        if L["op"] != "conv":
            continue
        w, b = params[L.get("shared_as", name)]
        r = layer_rule(L, graph, mode, fused, products)
        wr = wrong if name == wrong_layer else None
        if r["arith"] == "absorbed":
            continue
        if r["first"]:
            F = [M for M in graph if M["name"] == L["bottom"]][0]
            x = first_conv_model(blobs[F["bottom"]], params[F["name"]][0], params[F["name"]][1], r["first"], r["bf"],
                                 wrong=wrong if F["name"] == wrong_layer else None)
            blobs[F["name"]] = x
            amax[F["name"]] = float(np.abs(x).max())
        x = blobs[L["bottom"]]
        e = act_exponent(amax.get(L["bottom"], 0.0)) if (r["arith"] == "fam" and not r["bf"]) else 0
        if "e_act" in L:
            e = L["e_act"]
        out = conv_model(x, w, b, r["arith"], r["nprod"], r["bf"], L["dil"], L["relu"], e, wr)
        blobs[name] = out
        amax[name] = float(np.abs(out).max())
    return blobs
