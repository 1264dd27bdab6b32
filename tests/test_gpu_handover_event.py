"""The hand-over event of the grouped pipeline outlives the head that recorded it.

After a pipelined grouped pass (FusedDetector, one lane set) every member lane waits, in its next pass, for the HEAD's
``ev_convs`` (``shf_net::logits_done``).  The root net is a member lane of every FusedDetector built over it, so it survives
the detector and its heads: the event it would wait for must survive with it.  ``Net.handover_event()`` (C ABI
``shf_debug_handover_event``) reports whether the lane waits for an event and whether it holds that event itself."""
import gc

import numpy as np
import pytest

from smallhardface_amd.config import cfg
from tests import helpers as H

pytestmark = pytest.mark.gpu


def test_a_lane_holds_the_event_it_waits_for_after_the_head_is_gone(monkeypatch):
    monkeypatch.delenv("SHF_PIPE_SHARED_CONV_STREAM", raising=False)      # (the default: pipelined heads)
    from smallhardface_amd import test as T
    cfg.MODEL.DIFFERENT_DILATION.ENABLE = True
    cfg.TEST.SCALES = [100, 300]
    gnet, _ = H.make_pair(H.detector_msg(True), cls_bias=1.0)
    gnet.set_conv_mode("f16x3")
    assert gnet.handover_event() == (False, False)                         # nothing has run
    im = np.random.default_rng(70).integers(0, 256, (110, 150, 3)).astype(np.uint8)
    units = list(T.pyramid_units(im))
    fd = T.FusedDetector(gnet, n_lanes=len(units), mode="group")
    fd.submit(units, 0.05)
    want = fd.collect()[0]
    assert len(want) > 0
    assert gnet.handover_event() == (True, True)                           # the head's event, shared with the lane
    del fd                                                                 # the heads go, the root net stays
    gc.collect()
    assert gnet.handover_event() == (True, True)
    # ... and the next detector over the same net, whose heads wait for that event on their own streams, gives the same rows
    fd = T.FusedDetector(gnet, n_lanes=len(units), mode="group", lane_sets=2)
    fd.submit(units, 0.05)
    np.testing.assert_array_equal(fd.collect()[0], want)
