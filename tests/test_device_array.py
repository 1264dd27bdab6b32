"""caffe.DeviceArray (no GPU): a stand-in object with a ``__cuda_array_interface__`` dict whose pointer is never
dereferenced -- the class only carries a pointer, a shape, an owner and the ``flipped`` flag."""
import pytest

from smallhardface_amd import caffe


class _Fake(object):
    """What a torch tensor on the GPU shows to a consumer of the CUDA array interface."""

    def __init__(self, shape, typestr="<f4", strides=None, ptr=0x7f0000001000):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 2,
                                         "strides": strides}


def test_shape_pointer_owner():
    src = _Fake((1, 3, 5, 7))
    a = caffe.DeviceArray(src)
    assert a.shape == (1, 3, 5, 7) and a.ndim == 4
    assert a.ptr == 0x7f0000001000 and a.owner is src and a.flipped is False


def test_flipping_twice_returns_to_unflipped():
    a = caffe.DeviceArray(_Fake((1, 3, 5, 7)))
    f = a[..., ::-1]
    assert f.flipped is True and a.flipped is False          # a view: the source keeps its flag
    assert f.shape == a.shape and f.ptr == a.ptr and f.owner is a.owner
    ff = f[..., ::-1]
    assert ff.flipped is False and ff.ptr == a.ptr and ff.shape == a.shape


def test_cuda_array_interface_only_while_unflipped():
    a = caffe.DeviceArray(_Fake((2, 3, 4, 8)))
    cai = a.__cuda_array_interface__
    assert cai["shape"] == (2, 3, 4, 8) and cai["typestr"] == "<f4" and cai["data"] == (a.ptr, False)
    assert cai["strides"] is None
    f = a[..., ::-1]
    assert not hasattr(f, "__cuda_array_interface__")
    with pytest.raises(AttributeError):
        f.__cuda_array_interface__
    assert hasattr(f[..., ::-1], "__cuda_array_interface__")
    # an explicit flag at construction toggles the source's own
    assert caffe.DeviceArray(f, flipped=True).flipped is False
    assert caffe.DeviceArray(_Fake((1, 3, 4, 4)), flipped=True).flipped is True


@pytest.mark.parametrize("key", [0, slice(None), (0, 0), Ellipsis, (Ellipsis, slice(None, None, 1)),
                                 (Ellipsis, slice(None, None, -2)), (Ellipsis, slice(3, None, -1)),
                                 (slice(None), slice(None, None, -1)), (Ellipsis, 0), (Ellipsis, slice(None, None, -1), 0)],
                         ids=repr)
def test_any_other_index_is_a_type_error(key):
    a = caffe.DeviceArray(_Fake((1, 3, 5, 7)))
    with pytest.raises(TypeError):
        a[key]


def test_explicit_contiguous_strides_are_accepted():
    a = caffe.DeviceArray(_Fake((1, 3, 5, 7), strides=(420, 140, 28, 4)))
    assert a.shape == (1, 3, 5, 7)
    # an axis of length 1 may carry any stride
    assert caffe.DeviceArray(_Fake((1, 3, 5, 7), strides=(4, 140, 28, 4))).shape == (1, 3, 5, 7)


def test_fp16_is_a_value_error():
    with pytest.raises(ValueError):
        caffe.DeviceArray(_Fake((1, 3, 5, 7), typestr="<f2"))
    with pytest.raises(ValueError):
        caffe.DeviceArray(_Fake((1, 3, 5, 7), typestr="<f8"))


def test_strided_is_a_value_error():
    with pytest.raises(ValueError):
        caffe.DeviceArray(_Fake((1, 3, 5, 7), strides=(840, 280, 56, 8)))      # every second column
    with pytest.raises(ValueError):
        caffe.DeviceArray(_Fake((1, 3, 5, 7), strides=(420, 4, 84, 12)))       # an NHWC tensor permuted to NCHW


def test_three_axes_is_a_value_error():
    with pytest.raises(ValueError):
        caffe.DeviceArray(_Fake((3, 5, 7)))
    with pytest.raises(ValueError):
        caffe.DeviceArray(_Fake((1, 1, 3, 5, 7)))


def test_an_object_without_the_interface_is_a_type_error():
    with pytest.raises(TypeError):
        caffe.DeviceArray(object())
