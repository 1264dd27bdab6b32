"""The neuron layers' references, bounds and field census, without a GPU (tests/neuron_cases.py; the GPU half is
tests/test_gpu_neuron.py)."""
import numpy as np
import pytest

from smallhardface_amd import prototxt as P
from tests import neuron_cases as L

F32, F64 = np.float32, np.float64


# ---- the exact ops: the fp32 restatement against binary64 ---------------------------------------------------------------------
@pytest.mark.parametrize("spec", L.EXACT_SPECS, ids=L.spec_id)
@pytest.mark.parametrize("case", L.LAYER_CASES, ids=L.case_id)
def test_neuron32_is_the_rounded_binary64_value_on_integer_grids(case, spec):
    """On integers every product and sum is exact: one rounding or three, the same value."""
    data, sl, shared = L.int_inputs(case)
    perm = L.feeder_params(case)[1]
    x = data[:, perm]
    slope = (shared if spec[1].get("shared") else sl) if spec[0] == "PReLU" else None
    got, want = L.neuron32(spec, x, slope), L.neuron64(spec, x, slope)
    assert got.dtype == F32 and got.shape == x.shape == want.shape
    np.testing.assert_array_equal(got, want.astype(F32))
    np.testing.assert_array_equal(got.astype(F64), want)           # ... which is exact itself
    assert np.abs(got).max() > 0 or case[1] * case[2] == 1


def test_prelu_keeps_the_operand_order_of_std_max_and_min():
    x = np.array([np.nan, -0.0, 0.0, -3.0, 3.0, np.inf, -np.inf], F32).reshape(1, 1, 1, 7)
    got = L.neuron32(("PReLU", {"shared": True}), x, np.array(-2, F32)).reshape(-1)
    assert np.isnan(got[0])                                         # std::max(NaN, 0) is NaN: both comparisons are false
    np.testing.assert_array_equal(got[1:], np.array([0, 0, 6, 3, np.inf, np.inf], F32))
    zero = L.neuron32(("PReLU", {"shared": True}), x, np.array(0, F32)).reshape(-1)
    assert np.isnan(zero[6])                                        # 0 * -inf: the product is formed, not selected away


def test_power_skips_the_steps_caffe_skips():
    x = np.array([-0.0, 2.0, -3.0], F32).reshape(1, 1, 1, 3)
    copy = L.neuron32(("Power", {}), x)
    assert np.signbit(copy.reshape(-1)[0]) and (copy == x).all()   # no product, no add: the -0 survives
    np.testing.assert_array_equal(L.neuron64(("Power", {"power": 0, "shift": 5}), x), np.ones(x.shape))
    np.testing.assert_array_equal(L.neuron64(("Power", {"scale": 0, "shift": 3, "power": 2}), x), np.full(x.shape, 9.0))
    assert L.is_exact(("Power", {"scale": 3, "shift": -2})) and not L.is_exact(("Power", {"power": 2}))
    assert L.single_rounding(("Power", {"scale": -1})) and not L.single_rounding(("Power", {"scale": 3, "shift": -2}))


def test_derived_constants_round_once():
    inner, outer = L.derived(("Exp", {"base": 2, "scale": 0.5, "shift": 1}))
    assert inner == F32(np.log(2.0) * 0.5) and outer == F32(2.0) and inner.dtype == outer.dtype == F32
    assert L.derived(("Exp", {})) == (F32(1), F32(1)) and L.derived(("Log", {})) == F32(1)
    assert L.derived(("Exp", {"shift": 1}))[1] == F32(np.e)
    assert L.derived(("Log", {"base": 10})) == F32(1.0 / np.log(F64(10)))


# ---- the library ops: the bound holds for the reference's own kind of evaluation -------------------------------------------------
@pytest.mark.parametrize("spec", L.LIBRARY_SPECS, ids=L.spec_id)
@pytest.mark.parametrize("case", L.LAYER_CASES, ids=L.case_id)
def test_bound_holds_for_an_fp32_evaluation_of_the_formula(case, spec):
    data = L.library_inputs(case)
    x = data[:, L.feeder_params(case)[1]]
    if spec in L.POSITIVE_SPECS:
        x = np.abs(x)
    ref, bnd = L.neuron64(spec, x), L.bound(spec, x)
    got = L.numpy32(spec, x)
    assert got.dtype == F32 and np.isfinite(ref).all() and np.isfinite(got).all() and (bnd > 0).all()
    err = np.abs(got.astype(F64) - ref)
    worst = int(np.argmax(err / bnd))
    print("%s %s: max err / bound %.3g, max %.3g ulps" % (L.case_id(case), L.spec_id(spec), float((err / bnd).max()), float(L.ulps(got, ref).max())))
    assert (err <= bnd).all(), (float(x.flat[worst]), float(err.flat[worst]), float(bnd.flat[worst]))


def test_library_grids_span_the_special_points():
    seen = set()
    for case in L.LAYER_CASES:
        x = L.library_inputs(case)[:, L.feeder_params(case)[1]]
        assert np.abs(x).max() <= L.LIMIT
        seen |= {float(v) for v in L.SPECIALS if (x == F32(v)).any()}
    assert seen == {float(v) for v in L.SPECIALS}
    big = L.library_inputs((64, 33, 67))
    assert all((big == F32(v)).any() for v in L.SPECIALS)
    # where they saturate: the reference is not the formula's binary64 run but the function
    x = np.array([-20.0, 20.0], F32).reshape(1, 1, 1, 2)
    s = L.neuron64(("Sigmoid", {}), x).reshape(-1)
    assert abs(s[0] / np.exp(-20.0) - 1) < 1e-8 and s[1] < 1 and abs(L.neuron64(("BNLL", {}), x).reshape(-1)[0] / np.exp(-20.0) - 1) < 1e-8


def test_bound_is_absolute_where_the_formula_cancels():
    x = np.array([-20.0], F32).reshape(1, 1, 1, 1)
    for spec in (("Sigmoid", {}), ("BNLL", {})):
        ref, bnd = L.neuron64(spec, x), L.bound(spec, x)
        assert bnd[0, 0, 0, 0] > 10 * L.ulp32(ref)[0, 0, 0, 0]          # not a multiple of the tiny result's ulp
    x = np.array([3.0], F32).reshape(1, 1, 1, 1)
    assert L.bound(("TanH", {}), x)[0, 0, 0, 0] == 5 * L.ulp32(np.tanh(3.0)) and L.bound(("Power", {"power": 2}), x)[0, 0, 0, 0] == 16 * L.ulp32(9.0)


# ---- text, specs and the oracle net ------------------------------------------------------------------------------------------------
def test_layer_text_round_trips_and_the_oracle_net_runs_it():
    specs = L.EXACT_SPECS + L.SIGNED_SPECS
    case = (5, 7, 9)
    for in_place in (False, True):
        msg = P.parse(L.ops_net_text(case, specs, in_place))
        mine = [m for m in msg.getall("layer") if str(m.get("name")).startswith("op")]
        assert [L.fields(L.layer_spec(m)) for m in mine] == [L.fields(s) for s in specs]
        data, sl, shared = L.int_inputs(case)
        params, perm = L.feeder_params(case)
        params.update(op0=[sl], op1=[shared])
        onet = L.forwarded(L.NeuronOracleNet(msg, params=params), data, np.array([[7, 9, 1]], F32))
        x = data[:, perm]
        for i, spec in enumerate(specs):
            slope = {0: sl, 1: shared}.get(i)
            np.testing.assert_array_equal(onet.blobs["n%d" % i].data, L.oracle_value(spec, x, slope))
    fills = L.filler_params(P.parse(L.field_net(L.neuron_layer("a", ("PReLU", {}), "pre", "a") + L.neuron_layer("b", ("PReLU", {"shared": True, "fill": 3}), "pre", "b") +
                                                L.neuron_layer("c", ("PReLU", {"filler": 'type: "gaussian" std: 2'}), "pre", "c") +
                                                L.neuron_layer("d", ("PReLU", {"filler": 'type: "constant"'}), "pre", "d"))))
    assert {k: (v[0].shape, float(v[0].reshape(-1)[0])) for k, v in fills.items()} == {
        "a": ((L.VC,), 0.25), "b": ((), 3.0), "c": ((L.VC,), 0.25), "d": ((L.VC,), 0.0)}


def test_the_mini_detector_parses_and_its_oracle_finds_faces():
    from oracle import oracle as O
    msg = P.parse(L.mfn_text(*L.MFN_SIZE))
    types = [str(m.get("type")) for m in msg.getall("layer")]
    assert types.count("PReLU") == len(L.MFN_PRELUS) == 7 and types.count("BatchNorm") == 7
    assert O.infer_channels(msg)["f4"] == 128


# ---- the field census ------------------------------------------------------------------------------------------------------------
def test_every_field_of_the_neuron_messages_has_exactly_one_disposition():
    census = L.census()
    assert sorted(census) == sorted(["PReLUParameter", "ELUParameter", "PowerParameter", "ExpParameter", "LogParameter", "ThresholdParameter",
                                     "SigmoidParameter", "TanHParameter"])
    keys = {(m, f) for m, fs in census.items() for f in fs}
    assert not sorted(keys - set(L.DISPOSITION)), "fields of the schema without a disposition"
    assert not sorted(set(L.DISPOSITION) - keys), "dispositions for fields the schema does not declare"
    for key, (kind, what) in L.DISPOSITION.items():
        if kind == L.HONOURED:
            case = L.VALUE_CASES[what]
            assert (case.message, case.field) == key and case.text != case.twin
            name = {"channel_shared": "channel_shared:", "filler": "filler {"}.get(case.field, case.field + ":")
            assert name in case.text, key
        elif kind == L.REFUSED:
            assert what in L.REFUSALS, key
        else:
            assert kind == L.INERT and len(what) > 10, key


@pytest.mark.parametrize("name", sorted(L.VALUE_CASES))
def test_value_case_reference_depends_on_its_field(name):
    case = L.VALUE_CASES[name]
    outs = []
    for spec, slope in zip((case.spec, case.twin_spec), case.slopes):
        x = L.value_input(case.spec)
        if spec[0] == "PReLU" and slope is None:
            slope = np.full(() if spec[1].get("shared") else (L.VC,), L.prelu_fill(spec), F32)
        outs.append(L.oracle_value(spec, x, slope))
        assert np.isfinite(outs[-1]).all()
    assert not np.array_equal(outs[0], outs[1])


def test_refusal_texts_parse_and_name_their_layer():
    import re
    for name, r in L.REFUSALS.items():
        msg = P.parse(L.refusal_net(r.layers))
        names = [str(m.get("name")) for m in msg.getall("layer")]
        quoted = re.findall(r"'(\w+)'", r.match)
        assert quoted and quoted[0] in names, name
