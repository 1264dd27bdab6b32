"""The window's images on CPU: each decoded by its owner rank and shared in one all-gather per window
(pyramid.share_window_images, pyramid.WindowFeeder; gloo -- the same code runs over RCCL on the GPUs).

The ranks are spawned the way tests/test_pyramid_sharding.py spawns them, ONCE per world size: a rank runs every
scenario in a fixed order and sends back what it saw; the tests below each judge their part of that record."""
import os
import socket

import numpy as np
import pytest

from smallhardface_amd import pyramid

SHAPES = [(1, 1), (5, 9), (7, 4)]        # window image i is SHAPES[i]: a 1 x 1 x 3 image, two non-square ones
FEEDS = {1: [("owner", 3)], 2: [("owner", 4), ("owner", 9), ("all", 4)], 3: [("owner", 5)]}   # world -> (decode, n images)


def _image(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)


def _window(tag, n_valid):
    """The images of window `tag` (seeded: the checker regenerates them)."""
    return {i: _image(1000 * tag + i, *SHAPES[i]) for i in range(n_valid)}


def _feed_image(index):
    return _image(7000 + index, 2 + index % 3, 3 + index % 4)


def _all_need(rank, n_valid):
    """decode="all": the window images rank `rank`'s picks name in this test -- rank 0 both, rank 1 only image 1."""
    return [i for i in range(n_valid) if i >= rank]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _scenarios(rank, world):
    import torch
    dev = torch.device("cpu")
    force = world == 1
    counts = pyramid._IMAGE_COUNTS
    rec = {}

    def share(tag, n_valid, as_tensor=False):
        src = _window(tag, n_valid)
        mine = {i: (torch.from_numpy(src[i]) if as_tensor else src[i]) for i in pyramid.window_readers(rank, world, n_valid)}
        return pyramid.share_window_images(mine, n_valid, rank, world, dev, force_collective=force)

    # 1. a full window of uneven images, at the module's own starting capacity
    c0 = counts["collectives"]
    rec["cap0"] = pyramid._IMAGE_CAP["bytes"]
    rec["uneven"] = {i: t.numpy().copy() for i, t in share(1, world).items()}
    rec["uneven_collectives"] = counts["collectives"] - c0
    # 2. partly filled windows: every n_valid below world, down to an empty one
    rec["partial"] = {nv: {i: t.numpy().copy() for i, t in share(20 + nv, nv).items()} for nv in range(world)}
    # 4. lifetime: results are views into three receive blocks used in turn -- window k's stay intact through the calls for
    # windows k + 1 and k + 2 (no copy is taken here) and the call for k + 3 lands in window k's block
    kept, intact, ptrs = [], [], []
    for k in range(4):
        got = share(30 + k, world, as_tensor=True)
        kept.append(got)
        ptrs.append(got[0].data_ptr())
        intact.append([all(np.array_equal(kept[j][i].numpy(), _window(30 + j, world)[i]) for i in range(world))
                       for j in range(max(0, k - 2), k + 1)])
    rec["lifetime_intact"] = intact
    rec["lifetime_ptrs"] = ptrs
    rec["lifetime_k0_after_k3"] = all(np.array_equal(kept[0][i].numpy(), _window(33, world)[i]) for i in range(world))
    # 3. overflow: a capacity of 64 bytes, the 5 x 9 x 3 image (world >= 2) does not fit
    pyramid._IMAGE_CAP["bytes"] = 64
    rec["overflow"] = []
    for k in range(2):
        c0 = counts["collectives"]
        got = share(40 + k, world)
        rec["overflow"].append(({i: t.numpy().copy() for i, t in got.items()}, counts["collectives"] - c0,
                                pyramid._IMAGE_CAP["bytes"]))
    # 6. / 7. the feeder
    rec["feeds"] = []
    for decode, n in FEEDS[world]:
        log = []
        os.environ["SHF_SHARD_DECODE"] = decode            # read once, by the feeder's constructor
        fd = pyramid.WindowFeeder(None, n, rank, world, dev, force_collective=force,
                                  need=lambda n_valid: _all_need(rank, n_valid))

        def read(index, fd=fd, log=log):
            log.append((index, fd.window))
            return _feed_image(index)

        fd.read = read
        c0 = counts["collectives"]
        seen = []
        for base, n_valid, ims in fd:
            seen.append((base, n_valid, {i: t.numpy().copy() for i, t in ims.items()}))
        rec["feeds"].append({"decode": decode, "n": n, "log": log, "seen": seen, "stats": fd.stats(),
                             "module_collectives": counts["collectives"] - c0})
    os.environ.pop("SHF_SHARD_DECODE", None)
    return rec


def _worker(rank, world, port, q):
    import datetime
    import traceback
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    try:
        q.put((rank, _scenarios(rank, world), None))
    except Exception:                                       # (the parent fails with this text instead of waiting)
        q.put((rank, None, traceback.format_exc()))
        raise
    finally:
        dist.destroy_process_group()


_RUNS = {}


def _run(world):
    """{rank: record} of the `world`-rank run (a ONE-rank group runs the same collectives with the exchange forced)."""
    if world not in _RUNS:
        import torch.multiprocessing as mp
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
        for p in procs:
            p.start()
        res = {}
        try:
            for _ in procs:
                r, rec, err = q.get(timeout=240)
                assert err is None, "rank %d: %s" % (r, err)
                res[r] = rec
            for p in procs:
                p.join(timeout=30)
                assert p.exitcode == 0
        finally:
            for p in procs:
                if p.is_alive():
                    p.kill()
        _RUNS[world] = res
    return _RUNS[world]


def _same(got, want):
    assert got.dtype == np.uint8 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(got, want)


def test_window_readers_are_the_owners():
    for world in (1, 2, 3, 8):
        for n_valid in range(world + 1):
            seen = []
            for r in range(world):
                mine = pyramid.window_readers(r, world, n_valid)
                assert mine == [i for i in range(n_valid) if pyramid.image_owner(i, world) == r] and len(mine) <= 1
                seen += mine
            assert sorted(seen) == list(range(n_valid))     # every image of the window has exactly one reader


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 3, 1])
def test_share_window_images_uneven(world):
    """Images of different sizes in one window (1 x 1 x 3, 5 x 9 x 3, 7 x 4 x 3): every rank holds every image with the
    owner's bytes, after ONE collective, at the module's starting capacity of 8 MiB.  world 1: a one-rank group with the
    collective forced -- the same code path."""
    res = _run(world)
    for r in range(world):
        assert res[r]["cap0"] == 8 << 20
        assert sorted(res[r]["uneven"]) == list(range(world))
        for i in range(world):
            _same(res[r]["uneven"][i], _window(1, world)[i])
        assert res[r]["uneven_collectives"] == 1


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 3])
def test_share_window_images_partial_window(world):
    """n_valid < world: ranks that own nothing contribute nothing, results exist for exactly range(n_valid)."""
    res = _run(world)
    for r in range(world):
        assert sorted(res[r]["partial"]) == list(range(world))
        for nv, got in res[r]["partial"].items():
            assert sorted(got) == list(range(nv))
            for i in range(nv):
                _same(got[i], _window(20 + nv, nv)[i])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 3])
def test_share_window_images_overflow(world):
    """Capacity 64 bytes, one image of 135 (and at 3 ranks one of 84): every rank returns the right bytes and ends with
    the same larger capacity -- the next power of two that fits, 256 -- after exactly TWO collectives; the next window
    costs one."""
    res = _run(world)
    for r in range(world):
        (got0, n0, cap0), (got1, n1, cap1) = res[r]["overflow"]
        for k, got in ((0, got0), (1, got1)):
            assert sorted(got) == list(range(world))
            for i in range(world):
                _same(got[i], _window(40 + k, world)[i])
        assert (n0, n1) == (2, 1)
        assert cap0 == cap1 == 256
    # an image that fits a small capacity exactly does not raise it (one rank, the 1 x 1 x 3 image: 3 <= 64)
    (_, n0, cap0), (_, n1, cap1) = _run(1)[0]["overflow"]
    assert (n0, n1, cap0, cap1) == (1, 1, 64, 64)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 3])
def test_share_window_images_results_outlive_two_more_calls(world):
    """The three-block contract: the results are views (nothing is copied by the test), window k's are intact after the
    call for window k + 1 and after the call for k + 2; the call for k + 3 is handed window k's block again (the same
    address, now holding window k + 3).  Two blocks, or one, would fail the first half; more than three the second."""
    res = _run(world)
    for r in range(world):
        assert res[r]["lifetime_intact"] == [[True], [True, True], [True, True, True], [True, True, True]]
        p = res[r]["lifetime_ptrs"]
        assert len(set(p[:3])) == 3 and p[3] == p[0]
        assert res[r]["lifetime_k0_after_k3"]


def test_share_window_images_refuses_a_malformed_mine():
    """An image the rank does not own, or a missing one it owns: ValueError before any collective (no process group
    exists here, so reaching a collective would fail differently)."""
    im = _image(1, 4, 5)
    c0 = dict(pyramid._IMAGE_COUNTS)
    with pytest.raises(ValueError):
        pyramid.share_window_images({1: im}, 2, 0, 2, "cpu")                 # rank 0 owns image 0, not 1
    with pytest.raises(ValueError):
        pyramid.share_window_images({0: im, 1: im}, 2, 0, 2, "cpu")          # ... and not both
    with pytest.raises(ValueError):
        pyramid.share_window_images({}, 2, 0, 2, "cpu")                      # its own image is missing
    with pytest.raises(ValueError):
        pyramid.share_window_images({1: im}, 1, 1, 2, "cpu")                 # partly filled window: rank 1 owns nothing
    with pytest.raises(ValueError):
        pyramid.share_window_images({0: im}, 3, 0, 2, "cpu")                 # a window holds at most `world` images
    for bad in (im.astype(np.float32), im[:, :, :2], im[:, ::2], im.reshape(-1), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            pyramid.share_window_images({0: bad}, 1, 0, 1, "cpu", force_collective=True)
    assert pyramid._IMAGE_COUNTS == c0
    # one rank, nothing forced: no collective at all, the image itself comes back
    got = pyramid.share_window_images({0: im}, 1, 0, 1, "cpu")
    assert sorted(got) == [0] and np.array_equal(got[0].numpy(), im) and pyramid._IMAGE_COUNTS == c0
    assert pyramid.share_window_images({0: im}, 1, 0, 1, "cpu", async_op=True).wait()[0].shape == (4, 5, 3)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world,k", [(3, 0), (2, 0), (2, 1), (1, 0)])
def test_window_feeder_reads_each_image_once(world, k):
    """n = 5 images on 3 ranks, n = 4 on 2, n = 9 on 2 (five windows: the read-ahead bound and the block rotation have
    something to hold) and n = 3 on a forced one-rank group: rank r reads exactly range(r, n, world), each once -- n reads
    over all ranks, not n x world --, never more than two windows ahead of the window it is handing out; every rank is
    handed every image of every window with the owner's bytes; one image collective per window on every rank."""
    res = _run(world)
    decode, n = FEEDS[world][k]
    assert decode == "owner"
    n_windows = (n + world - 1) // world
    total = 0
    for r in range(world):
        f = res[r]["feeds"][k]
        assert (f["decode"], f["n"]) == (decode, n)
        assert sorted(i for i, _ in f["log"]) == list(range(r, n, world))
        total += len(f["log"])
        for index, window in f["log"]:
            assert 0 <= window and index // world <= window + 2, (index, window)
        assert [(b, nv) for b, nv, _ in f["seen"]] == [(w * world, min(world, n - w * world)) for w in range(n_windows)]
        for base, n_valid, ims in f["seen"]:
            assert sorted(ims) == list(range(n_valid))
            for i in range(n_valid):
                _same(ims[i], _feed_image(base + i))
        st = f["stats"]
        assert st["reads"] == len(f["log"]) and st["image_collectives"] == n_windows == f["module_collectives"]
        assert st["uploads"] == 0 and st["seconds"] >= 0.0        # (host tensors: nothing goes to a device)
    assert total == n


@pytest.mark.timeout(300)
def test_window_feeder_old_path_decodes_what_the_picks_need():
    """SHF_SHARD_DECODE=all: no image collective; a rank reads -- and is handed -- the images its picks need."""
    world, k = 2, 2
    res = _run(world)
    decode, n = FEEDS[world][k]
    assert decode == "all"
    for r in range(world):
        f = res[r]["feeds"][k]
        want = [w * world + i for w in range(2) for i in _all_need(r, world)]
        assert sorted(i for i, _ in f["log"]) == want
        assert f["stats"]["image_collectives"] == 0 and f["module_collectives"] == 0 and f["stats"]["reads"] == len(want)
        for base, n_valid, ims in f["seen"]:
            assert sorted(ims) == _all_need(r, n_valid)
            for i in ims:
                _same(ims[i], _feed_image(base + i))


def test_window_feeder_refuses_an_unknown_decode_mode():
    with pytest.raises(ValueError):
        pyramid.WindowFeeder(_feed_image, 3, 0, 1, "cpu", decode="some")


def test_window_feeder_reader_failure_names_the_path():
    def read(index):
        if index == 2:
            raise IOError("cannot read image /data/img%d.jpg" % index)
        return _feed_image(index)

    seen = []
    with pytest.raises(IOError, match="img2.jpg"):
        for base, n_valid, ims in pyramid.WindowFeeder(read, 3, 0, 1, "cpu", decode="owner"):
            seen.append(base)
    assert seen == [0]
