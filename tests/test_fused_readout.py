"""The read-out that tests/test_gpu_fused_forms.py relies on (helpers.mini_detector / read_fused_blob), checked on the
numpy oracle alone: one-hot predictors copy the probed blob into the predictors' tops bit for bit, so what the GPU tests
compare is the fused path's blob and nothing the read-out added."""
import numpy as np
import pytest

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from tests import helpers as H


def _conv(name, bottom, nout, k=3, pad=1, dil=1, relu=True, shared=False):
    s = ('layer { name: "%s" type: "Convolution" bottom: "%s" top: "%s" %sconvolution_param { num_output: %d '
         'kernel_size: %d pad: %d dilation: %d } }\n'
         % (name, bottom, name, 'param { name: "hw" } param { name: "hb" } ' if shared else "", nout, k, pad, dil))
    if relu:
        s += 'layer { name: "%s_relu" type: "ReLU" bottom: "%s" top: "%s" }\n' % (name, name, name)
    return s


POOL = 'layer { name: "p" type: "Pooling" bottom: "c1" top: "p" pooling_param { pool: MAX kernel_size: 2 stride: 2 } }\n'


def _oracle(txt, seed):
    msg = P.parse(txt)
    params = O.synth_params(msg, seed=seed)
    rng = np.random.default_rng(seed + 1)
    for name, blobs in params.items():
        if name.startswith("c") and not name.startswith("cls") and len(blobs) > 1:
            blobs[1][...] = rng.normal(0, 0.5, blobs[1].shape).astype(np.float32)
    return O.OracleNet(msg, params=params), rng


def test_read_out_of_a_pooled_blob_is_exact():
    h, w = 37, 53
    txt = H.mini_detector(_conv("c0", "data", 64) + _conv("c1", "c0", 128, relu=False) + POOL, "p", 2, 3, h, w)
    onet, rng = _oracle(txt, 3)
    assert H.readout_forwards(onet) == 4
    data = rng.normal(0, 1, (1, 3, h, w)).astype(np.float32)
    got = H.read_fused_blob(None, onet, data, np.array([[h, w, 1]], np.float32))
    want = onet.blobs["p"].data
    assert want.shape == (1, 128, 19, 27) and (want < 0).any()
    assert got.shape == want.shape[1:] and np.array_equal(got, want[0])
    assert onet.outputs == ["boxes", "cls_prob"]         # nothing else is a net output: what the fast forward requires


def test_read_out_per_blob_tail_is_exact():
    """The dilated template's tail over three blobs of one size (the three shared-weight heads' graph)."""
    h, w = 11, 14
    txt = H.mini_detector(_conv("c0", "data", 64) + _conv("h1", "c0", 128, 3, 1, 1, shared=True) +
                          _conv("h2", "c0", 128, 3, 2, 2, shared=True) + _conv("h4", "c0", 128, 3, 4, 4, shared=True),
                          ["h1", "h2", "h4"], 1, 3, h, w)
    onet, rng = _oracle(txt, 5)
    onet.params["h1"][1][...] = rng.normal(0, 0.5, 128).astype(np.float32)
    assert onet.params["h4"][1] is onet.params["h1"][1]
    assert H.readout_forwards(onet) == 32
    data = rng.normal(0, 1, (1, 3, h, w)).astype(np.float32)
    got = H.read_fused_blob(None, onet, data, np.array([[h, w, 1]], np.float32))
    assert len(got) == 3
    for g, name in zip(got, ("h1", "h2", "h4")):
        assert np.array_equal(g, onet.blobs[name].data[0]), name
    assert not np.array_equal(got[0], got[1])


def test_mini_detector_refuses_a_single_name_in_a_list():
    with pytest.raises(AssertionError):
        H.mini_detector(_conv("c0", "data", 128), ["c0"], 1)
