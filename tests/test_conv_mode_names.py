"""The drop-in Net's conv-mode names (no GPU): every name maps to the integer the C ABI takes and back, "f64" = 5 included."""
import pytest

from smallhardface_amd import caffe


class _FakeLib(object):
    """Records what the shim hands to shf_net_set_conv_mode / returns a chosen mode from shf_net_get_conv_mode."""

    def __init__(self):
        self.mode = 0

    def shf_net_set_conv_mode(self, h, mode):
        self.mode = mode
        return 0

    def shf_net_get_conv_mode(self, h):
        return self.mode


def _net():
    net = caffe.Net.__new__(caffe.Net)
    net._lib, net._h, net._dirty_layers = _FakeLib(), None, set()
    return net


def test_f64_is_mode_5_by_name_and_by_number():
    assert caffe.CONV_MODES["f64"] == 5 and caffe.CONV_MODES[5] == 5
    assert caffe.CONV_MODE_NAMES[5] == "f64"


def test_every_mode_name_round_trips_through_the_shim():
    net = _net()
    names = ["fp32", "f16x3", "f16x2", "f16", "bf16", "f64"]
    for number, name in enumerate(names):
        net.set_conv_mode(name)
        assert net._lib.mode == number
        assert net.conv_mode == name
        net.set_conv_mode(number)
        assert net._lib.mode == number and net.conv_mode == name
    assert sorted(k for k in caffe.CONV_MODES if isinstance(k, str)) == sorted(names)
    with pytest.raises(KeyError):
        net.set_conv_mode("f128")
