"""The graph reader's field census, the independent reading of the geometry and the value cases' references, without a GPU
(tests/graph_field_cases.py; the GPU half is tests/test_gpu_graph_fields.py)."""
import importlib

import numpy as np
import pytest

from oracle import graph_reader as R
from smallhardface_amd import prototxt as P
from smallhardface_amd import weights as W
from tests import buffer_history_cases as B
from tests import graph_field_cases as GF
from tests import helpers as H


# ---- A: the census ------------------------------------------------------------------------------------------------------------
def _census_keys():
    census = GF.census()
    keys = set()
    for t, (pf, message) in GF.TYPE_MESSAGE.items():
        for f in (census[message] if message else []):
            keys.add((t, f))
    keys |= {("Layer", f) for f in census["LayerParameter"]} | {("Net", f) for f in census["NetParameter"]}
    return census, keys


def test_every_field_of_the_schema_has_exactly_one_disposition():
    census, keys = _census_keys()
    assert set(census) == {m for _, m in GF.TYPE_MESSAGE.values() if m} | {"LayerParameter", "NetParameter"}
    missing = sorted(keys - set(GF.DISPOSITION))
    assert not missing, "fields of the schema without a disposition: %s" % missing
    stale = sorted(set(GF.DISPOSITION) - keys)
    assert not stale, "dispositions for fields the schema does not declare: %s" % stale
    # every accepted type's own parameter message is a field of LayerParameter
    for t, (pf, _) in GF.TYPE_MESSAGE.items():
        assert pf is None or pf in census["LayerParameter"], (t, pf)


def test_every_disposition_names_what_proves_it():
    for key, (kind, what) in GF.DISPOSITION.items():
        assert kind in (GF.HONOURED, GF.REFUSED, GF.INERT), key
        if kind == GF.INERT:
            assert isinstance(what, str) and len(what) > 10 and "\n" not in what, key
        elif kind == GF.REFUSED:
            assert what in GF.REFUSALS, key
        elif ":" in what:
            mod, attr = what.split(":")
            assert hasattr(importlib.import_module(mod), attr), key
        else:
            case = GF.VALUE_CASES[what]
            assert key[0] == case.scope and key[1] in case.fields, key
            assert ("%s:" % key[1]) in case.text, key
    # ... and no value case or refusal is an orphan of a renamed field
    fields = {f for _, f in GF.DISPOSITION}
    for name, case in GF.VALUE_CASES.items():
        assert set(case.fields) <= fields, name


# ---- B: the independent reader against the product's parser -------------------------------------------------------------------
def _family_texts():
    out = []
    for key in B.KEYS:
        h, w = B.CASES[key].sizes[0]
        out.append((key, h, w))
    return out + [("detector_dd", 64, 96), ("detector_plain", 64, 96)]


def family_setup(key, h, w):
    """(prototxt text, {layer: parameter arrays} as weights.py / the family's oracle net hold them)."""
    if key.startswith("detector_"):
        msg = H.detector_msg(key == "detector_dd")
        msg.set_nth("input_shape", 0, P.Msg([("dim", 1), ("dim", 3), ("dim", h), ("dim", w)]))
        return P.dumps(msg), W.synth_params(msg)
    text, onet, _, _ = B.CASES[key].setup(h, w)
    return text, onet.params


def _ints(msg, name, default):
    v = msg.getall(name) if msg is not None else []
    return int(v[0]) if v else default


@pytest.mark.parametrize("key,h,w", _family_texts(), ids=[k for k, _, _ in _family_texts()])
def test_reader_agrees_with_the_products_parser(key, h, w):
    text, params = family_setup(key, h, w)
    graph = R.read(text)
    msg = P.parse(text)
    layers = msg.getall("layer")
    assert [(L.name, L.type, L.bottoms, L.tops) for L in graph.layers] == [
        (str(m.get("name")), str(m.get("type")), [str(b) for b in m.getall("bottom")], [str(t) for t in m.getall("top")]) for m in layers]
    shapes = graph.blob_shapes()
    channels = W.infer_channels(msg, in_ch=shapes[graph.layers[0].bottoms[0] if graph.layers[0].bottoms else "data"][1])
    for L, m in zip(graph.layers, layers):
        if L.type in ("Convolution", "Deconvolution"):
            cp = m.get("convolution_param")
            assert L.hp["kernel"] == (_ints(cp, "kernel_size", 1),) * 2 and L.hp["pad"] == (_ints(cp, "pad", 0),) * 2, L.name
            assert L.hp["stride"] == (_ints(cp, "stride", 1),) * 2 and L.hp["dilation"] == (_ints(cp, "dilation", 1),) * 2, L.name
            assert L.hp["group"] == _ints(cp, "group", 1) and L.hp["num_output"] == int(cp.get("num_output")), L.name
            assert L.hp["bias_term"] == (str(cp.get("bias_term", "true")) != "false"), L.name
        elif L.type == "Concat":
            assert L.hp["axis"] == _ints(m.get("concat_param"), "axis", 1), L.name
        for t in L.tops:
            if shapes[t] is not None and len(shapes[t]) == 4 and L.type != "Reshape":
                assert shapes[t][1] == channels[t], (L.name, t)
    want = {name: [tuple(a.shape) for a in blobs] for name, blobs in params.items()}
    got = {name: [tuple(s) for s in shp] for name, shp in graph.param_shapes().items()}
    assert got == want


def test_reader_blob_shapes_equal_a_forwarded_oracle_net():
    """The whole shape of every blob, on the graphs whose oracle forwards in a moment: the reader's Reshape rules against the
    arrays the family's oracle net computes."""
    for key in ("pool_group", "slim", "dil2", "pool_mini", "chain"):
        h, w = B.CASES[key].sizes[0]
        text = B.CASES[key].setup(h, w)[0]
        onet = B.CASES[key].oracle(h, w)
        for name, shp in R.read(text).blob_shapes().items():
            if shp is not None and name != "im_info":
                assert tuple(onet.blobs[name].data.shape) == tuple(shp), (key, name)


def test_reader_resolves_what_the_product_refuses():
    """Caffe's rules beyond the product's: per-axis geometry, a Deconvolution's dilated extent, global pooling, negative axes."""
    g = R.read(GF.g("num_output: 8 kernel_h: 3 kernel_w: 5 pad_h: 1 pad_w: 2 stride: [1, 2] dilation: 2"))
    assert g.layer("g").hp["kernel"] == (3, 5) and g.layer("g").hp["pad"] == (1, 2) and g.layer("g").hp["stride"] == (1, 2)
    assert g.blob_shapes()["g"] == (1, 8, 7 + 2 - 5 + 1, (9 + 4 - 9) // 2 + 1) and g.param_shapes()["g"] == [(8, GF.C, 3, 5), (8,)]
    g = R.read(GF.up("num_output: 16 group: 16 kernel_size: 3 dilation: 2 stride: 2"))
    assert g.blob_shapes()["up"] == (1, 16, 2 * 6 + 5, 2 * 8 + 5) and g.param_shapes()["up"] == [(16, 1, 3, 3), (16,)]
    g = R.read(GF.net(GF.K.pool_txt("p", "pre", "AVE", global_pool=True)))
    assert g.blob_shapes()["p"] == (1, GF.C, 1, 1)
    g = R.read(GF.VALUE_CASES["concat_axis_negative"].text)
    assert g.blob_shapes()["cat"] == (1, 2 * GF.C, 7, 9)
    for bad in ("num_output: 8 kernel_size: 3 kernel_h: 3", "num_output: 8 kernel_size: [3, 3, 3]", "num_output: 8", "num_output: 8 kernel_size: 3 stride_h: 2"):
        with pytest.raises(R.GraphError):
            R.read(GF.g(bad))


@pytest.mark.parametrize("i", range(len(GF.ILL_TYPED)))
def test_ill_typed_scalars_raise_in_the_reader(i):
    with pytest.raises(R.GraphError):
        R.read(GF.ILL_TYPED[i])


def test_reader_shares_no_code_with_the_product():
    import ast
    import inspect
    tree = ast.parse(inspect.getsource(R))
    names = [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names]
    names += [n.module or "" for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
    assert not [n for n in names if n.split(".")[0] in ("smallhardface_amd", "oracle", "tests")], names


# ---- C: the value cases' references alone -------------------------------------------------------------------------------------
_REFS = {}


def value_reference(name, twin=False):
    """(blobs, largest dot product's magnitude, params, inputs) of a value case, computed once."""
    if (name, twin) not in _REFS:
        case = GF.VALUE_CASES[name]
        text = case.twin if twin else case.text
        params, inputs = GF.case_params(text), GF.case_inputs(text)
        _REFS[(name, twin)] = GF.reference(text, params, inputs["data"]) + (params, inputs)
    return _REFS[(name, twin)]


@pytest.mark.parametrize("name", sorted(GF.VALUE_CASES))
def test_value_case_is_exact_and_depends_on_its_field(name):
    blobs, worst, params, inputs = value_reference(name)
    assert worst < 2 ** 24
    for arr in list(blobs.values()) + [a for p in params.values() for a in p] + [inputs["data"]]:
        assert GF.on_grid(arr)
    out = R.read(GF.VALUE_CASES[name].text).layers[-1].tops[0]
    other = value_reference(name, twin=True)[0][out]
    assert other.shape != blobs[out].shape or not np.array_equal(other, blobs[out]), "the result does not depend on the field"
    assert np.abs(blobs[out]).max() > 0


@pytest.mark.parametrize("type_", sorted(GF.STANDALONE))
def test_standalone_reference_is_exact(type_):
    text, outs, unit = GF.STANDALONE[type_]
    params, inputs = GF.case_params(text), GF.case_inputs(text, unit=unit)
    blobs, worst = GF.reference(text, params, inputs["data"])
    assert worst < 2 ** 24 and all(GF.on_grid(blobs[o]) and np.abs(blobs[o]).max() > 0 for o in outs)
    assert type_ in [L.type for L in R.read(text).layers]


def test_standalone_covers_every_accepted_type():
    assert sorted(list(GF.STANDALONE) + list(GF.STANDALONE_REFUSED) + list(GF.STANDALONE_TAIL)) == GF.ACCEPTED_TYPES


# ---- D: the Python readers refuse and honour what the runtime does ------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n, r in GF.REFUSALS.items() if r.python))
def test_python_readers_refuse_in_the_runtimes_words(name):
    import re
    r = GF.REFUSALS[name]
    with pytest.raises(ValueError) as e:
        P.normalize_graph(P.parse(r.text))
    assert re.search(r.match, str(e.value)), str(e.value)
    with pytest.raises(ValueError):
        W.infer_channels(P.parse(r.text), in_ch=GF.C)


@pytest.mark.parametrize("name", sorted(GF.ACCEPTED))
def test_python_readers_accept_the_spellings_text_format_accepts(name):
    P.normalize_graph(P.parse(GF.ACCEPTED[name]))


@pytest.mark.parametrize("name", sorted(n for n, c in GF.VALUE_CASES.items() if c.scope in ("Convolution", "Deconvolution", "Concat")))
def test_python_readers_resolve_the_geometry_the_reader_resolves(name):
    """weights.py's parameter shapes on a value case's text equal the independent reader's: the *_h / *_w and repeated forms
    reach the oracle side as the square geometry they mean."""
    text = GF.VALUE_CASES[name].text
    msg = P.parse(text)
    got = {k: [tuple(a.shape) for a in v] for k, v in W.synth_params(msg).items()}
    want = {k: [tuple(s) for s in v] for k, v in R.read(text).param_shapes().items()}
    assert got == want
    norm = P.normalize_graph(msg)
    for L, m in zip(R.read(text).layers, norm.getall("layer")):
        if L.type in ("Convolution", "Deconvolution"):
            cp = m.get("convolution_param")
            assert (L.hp["kernel"], L.hp["pad"], L.hp["stride"], L.hp["dilation"]) == tuple(
                (_ints(cp, f, None),) * 2 for f in ("kernel_size", "pad", "stride", "dilation")), L.name


def test_integration_document_lists_the_refused_and_inert_fields():
    import os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "INTEGRATION.md")) as f:
        doc = f.read()
    table = doc.split("integration_table() -->\n")[1].split("\n<!-- /graph-field-table -->")[0]
    assert table == GF.integration_table()
