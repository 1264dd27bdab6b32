"""The window's image exchange on the GPU: a ONE-rank `nccl` group (file store, no port), so pyramid.share_window_images
runs its RCCL branch -- the owner's one upload into its send slot, the device-tensor all-gather, results that are views
into the cached receive blocks -- and DevicePyramid.window_units reads those views in place."""
import numpy as np
import pytest

from smallhardface_amd.config import cfg
from tests import helpers as H

pytestmark = pytest.mark.gpu

SHAPES = [(37, 53), (64, 40)]      # odd sizes, non-square both ways: 0.5 takes cv::resize's 2x area path with its border
SCALES = [0.5, 1.3]                # loop (37 -> 18 rows, 53 -> 26 columns), 1.3 the bilinear one; every level is padded


def _levels(dp, units):
    """Every unit's (1, 3, H, W) level out of the pyramid's slot, after a size check of the unit against the slot."""
    slot = dp._slots[(dp._k - 1) % len(dp._slots)][0]
    out = []
    for ptr, Hh, Ww, lh, lw, s, flip in units:
        off = (ptr - slot.data_ptr()) // 4
        assert 0 <= off and off + 3 * Hh * Ww <= slot.numel() and lh <= Hh and lw <= Ww
        out.append(slot[off:off + 3 * Hh * Ww].cpu().numpy().reshape(1, 3, Hh, Ww))
    return out


@pytest.mark.timeout(300)
def test_shared_images_feed_the_device_pyramid_bit_exact(tmp_path):
    import torch
    import torch.distributed as dist
    from smallhardface_amd import pyramid
    from smallhardface_amd import test as T
    cfg.TEST.FLIP = True
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    ims = [np.random.default_rng(50 + k).integers(0, 256, hw + (3,)).astype(np.uint8) for k, hw in enumerate(SHAPES)]
    assert not dist.is_initialized()
    dist.init_process_group("nccl", init_method="file://" + str(tmp_path / "store"), rank=0, world_size=1, device_id=dev)
    try:
        c0 = dict(pyramid._IMAGE_COUNTS)
        # a window of a one-rank group is ONE image: two windows, the first one's result is kept while the second travels
        got = [pyramid.share_window_images({0: im}, 1, 0, 1, dev, force_collective=True)[0] for im in ims]
        assert pyramid._IMAGE_COUNTS["collectives"] - c0["collectives"] == 2
        assert pyramid._IMAGE_COUNTS["uploads"] - c0["uploads"] == 2
        for t, im in zip(got, ims):
            # what a launch will read: h * w * 3 bytes from this pointer, all of them inside the tensor's own allocation
            assert t.dtype == torch.uint8 and t.device == dev and t.is_contiguous() and tuple(t.shape) == im.shape
            assert t.storage_offset() + t.numel() <= t.untyped_storage().nbytes()
            np.testing.assert_array_equal(t.cpu().numpy(), im)
        assert got[0].untyped_storage().data_ptr() != got[1].untyped_storage().data_ptr()    # two of the three blocks
        gnet, _ = H.make_pair(H.detector_msg(True), cls_bias=1.0)
        dp_shared, dp_host = T.DevicePyramid(gnet), T.DevicePyramid(gnet)
        u_shared = dp_shared.window_units([None, None], scales=[SCALES, SCALES], im_devs=got)
        u_host = dp_host.window_units(ims, scales=[SCALES, SCALES])
        gnet.sync()
        assert len(u_shared) == len(u_host) == 2 * len(SCALES) * 2
        for a, b in zip(u_shared, u_host):
            assert tuple(a[1:]) == tuple(b[1:])
        for a, b in zip(_levels(dp_shared, u_shared), _levels(dp_host, u_host)):
            assert np.abs(b).max() > 0
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
        for t, im in zip(got, ims):                         # ... and nothing wrote the shared images meanwhile
            np.testing.assert_array_equal(t.cpu().numpy(), im)
        # a tensor that does not hold what the kernel would read is refused before any launch
        with pytest.raises(ValueError):
            dp_shared.window_units([None], scales=[SCALES], im_devs=[got[0].reshape(-1)])
        with pytest.raises(ValueError):
            dp_shared.window_units([ims[1]], scales=[SCALES], im_devs=[got[0]])
        with pytest.raises(ValueError):
            dp_shared.window_units([None], scales=[SCALES], im_devs=[got[0][:, ::2]])
    finally:
        dist.destroy_process_group()
