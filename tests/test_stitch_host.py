"""CPU: the host side of tiling -- adapt.tile_origins, frames.stitch_table (dvsr_frame_stitch_origins / _cover /
_table), frames.tile_view, engine.StreamPlan.max_image_bytes and the size check of adapt.super_resolve_frames,
adapt.tile_footprint / choose_tile, and the rejections of the tile arguments.  Nothing here touches a device.

Bars: origins are hand-written; the table is within 1 fp32 ulp of the numpy restatement (both compute in double and round once,
but the host compiler may contract the library's double arithmetic); weights of a position sum to 1 within 1e-6 (at most three
fp32 roundings of 2^-24 each)."""
import ctypes

import numpy as np
import pytest
import torch

import stitch_ref as ref
from dynavsr_amd import _lib as L
from dynavsr_amd import adapt, engine, frames

EDVR_M = (64, 5, 8, 5, 10, 4, 2, 0)
OPT = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}
AXES = [(36, 16, 8), (40, 20, 4), (32, 16, 4), (40, 16, 4), (16, 32, 8), (36, 16, 0), (48, 16, 8), (100, 36, 16)]


@pytest.fixture(scope="module")
def cpu_net():
    from dynavsr_amd.models.archs.EDVR_arch import EDVR
    return EDVR()


def test_origins_hand_written():
    assert adapt.tile_origins(36, 16, 8) == [0, 8, 16, 20]
    assert adapt.tile_origins(40, 20, 4) == [0, 16, 20]
    assert adapt.tile_origins(32, 16, 4) == [0, 12, 16]
    assert adapt.tile_origins(16, 16, 4) == [0] and adapt.tile_origins(16, 32, 8) == [0] and adapt.tile_origins(12, 16, 0) == [0]
    assert adapt.tile_origins(32, 16, 0) == [0, 16]
    for n, tile, overlap in AXES:
        got = adapt.tile_origins(n, tile, overlap)
        assert got == ref.origins(n, tile, overlap), (n, tile, overlap)
        assert all(o % 4 == 0 for o in got) and got[-1] == max(0, n - tile)
    # three tiles cover [20, 24) of (36, 16, 8) and nothing else
    assert L.lib().dvsr_frame_stitch_cover(36, 16, 8) == 3
    _, _, w = frames.stitch_table(36, 16, 8, 1)
    assert [r for r in range(36) if int((w[r] > 0).sum()) == 3] == [20, 21, 22, 23]
    assert L.lib().dvsr_frame_stitch_cover(40, 20, 4) == 2 and L.lib().dvsr_frame_stitch_cover(16, 32, 8) == 1


@pytest.mark.parametrize("bad", [(36, 18, 8), (36, 16, 6), (36, 16, 12), (34, 16, 8), (36, 16, -4), (0, 16, 8), (36, 0, 0)])
def test_bad_axes_are_refused(bad):
    with pytest.raises(ValueError):
        adapt.tile_origins(*bad)
    with pytest.raises(ValueError):
        frames.stitch_table(*bad, 4)
    assert L.lib().dvsr_frame_stitch_cover(*bad) == -1


def test_table_rejections():
    l = L.lib()
    first, w = torch.zeros(144, dtype=torch.int32), torch.zeros((144, 3))
    assert l.dvsr_frame_stitch_table(36, 16, 8, 4, 3, None, w.data_ptr()) == -1
    assert l.dvsr_frame_stitch_table(36, 16, 8, 4, 3, first.data_ptr(), None) == -1
    assert l.dvsr_frame_stitch_table(36, 16, 8, 4, 2, first.data_ptr(), w.data_ptr()) == -1     # the axis needs 3
    assert l.dvsr_frame_stitch_table(36, 16, 8, 4, 4, first.data_ptr(), w.data_ptr()) == -1
    assert l.dvsr_frame_stitch_table(36, 16, 8, 0, 3, first.data_ptr(), w.data_ptr()) == -1
    assert l.dvsr_frame_stitch_table(36, 16, 8, 17, 3, first.data_ptr(), w.data_ptr()) == -1
    assert not first.any() and not w.any()
    assert l.dvsr_frame_stitch_origins(36, 16, 8, (ctypes.c_int * 2)(), 2) == -1                # four origins, room for two
    assert l.dvsr_frame_stitch_table(36, 16, 8, 4, 3, first.data_ptr(), w.data_ptr()) == 0


def ulps(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("scale", [1, 2, 4])
@pytest.mark.parametrize("axis", AXES, ids=str)
def test_table_against_numpy(axis, scale):
    n, tile, overlap = axis
    o, first, w = frames.stitch_table(n, tile, overlap, scale)
    ro, rfirst, rw = ref.table(n, tile, overlap, scale)
    assert o.dtype == torch.int32 and first.dtype == torch.int32 and w.dtype == torch.float32
    assert np.array_equal(o.numpy(), ro) and np.array_equal(first.numpy(), rfirst)
    assert tuple(w.shape) == rw.shape == (scale * n, L.lib().dvsr_frame_stitch_cover(n, tile, overlap))
    assert int(ulps(w.numpy(), rw).max()) <= 1
    assert np.array_equal(w.numpy() == 0, rw == 0)                      # > 0 for every covering tile, 0 elsewhere
    assert float((w.double().sum(1) - 1).abs().max()) <= 1e-6
    tiles = len(ro)
    dense = ref.dense_of((o, first, w), tiles)
    L_, org = scale * min(tile, n), ro
    for r in range(scale * n):
        covering = [k for k in range(tiles) if org[k] <= r < org[k] + L_]
        assert [k for k in range(tiles) if dense[r, k] > 0] == covering, r
        if len(covering) == 1:
            assert dense[r, covering[0]].view(np.int32) == np.float32(1.0).view(np.int32), r     # exactly 1.0f
    # a pairwise overlap is a linear cross-fade: constant steps of 1 / (scale * overlap)
    if axis == (40, 20, 4):
        a, b = scale * 16, scale * 20
        np.testing.assert_allclose(np.diff(dense[a:b, 1].astype(np.float64)), 1.0 / (scale * 4), rtol=0, atol=2e-7)


@pytest.mark.parametrize("axis", [(40, 16, 4), (32, 16, 0), (56, 24, 8), (16, 16, 4)], ids=str)
def test_symmetric_layout_has_a_mirror_symmetric_table(axis):
    n, tile, overlap = axis
    org = adapt.tile_origins(n, tile, overlap)
    assert [n - tile - o for o in reversed(org)] == org or org == [0]    # the layout is symmetric ...
    for scale in (1, 4):
        table = frames.stitch_table(n, tile, overlap, scale)
        assert table[2].shape[1] <= 2                                  # (two terms: their sum does not depend on the order)
        dense = ref.dense_of(table, len(org))
        assert np.array_equal(dense.view(np.int32), dense[::-1, ::-1].view(np.int32))   # ... and so are the weights, bit for bit


# ---- the size check ---------------------------------------------------------------------------------
def test_max_image_bytes_and_the_size_check(cpu_net):
    small, large = engine.StreamPlan(EDVR_M, 720, 1280, 6), engine.StreamPlan(EDVR_M, 1080, 1920, 6)
    # the plan's answer, not a formula: for nf = 64 at scale 4 it is the up-sampling stage, 256 channels at 2h x 2w
    assert small.max_image_bytes == 4096 * 720 * 1280 < 2 ** 32
    assert large.max_image_bytes == 4096 * 1080 * 1920 >= 2 ** 32
    assert engine.StreamPlan(EDVR_M, 1024, 1024, 6).max_image_bytes == 2 ** 32
    assert engine.StreamPlan(EDVR_M, 16, 20, 6).max_image_bytes == engine.StreamPlan(EDVR_M, 16, 20, 72).max_image_bytes
    assert L.lib().dvsr_edvr_stream_max_image_bytes(None) == 0

    def run(h, w, **kw):
        next(adapt.super_resolve_frames(OPT, cpu_net, torch.zeros((1, 3, h, w)).expand(7, 3, h, w), **kw))
    # ValueError if and only if the plan of the size about to run says >= 2^32; otherwise the call goes on to the device check
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        run(720, 1280)
    with pytest.raises(ValueError, match="tile="):
        run(1080, 1920)
    with pytest.raises(ValueError, match="tile="):
        run(1024, 1024)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        run(1024, 1020)
    with pytest.raises(ValueError, match="tile="):
        run(1080, 1920, tile=(1080, 1920))                              # a tile >= the frame is the frame
    with pytest.raises(ValueError, match="tile="):
        run(1080, 1920, tile=(1080, 1024))                              # the tile itself is checked
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        run(1080, 1920, tile=(544, 976))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        run(1080, 1920, tile='auto', tile_budget=100e9)
    with pytest.raises(ValueError, match="choose_tile"):
        run(1080, 1920, tile='auto', tile_budget=1e6)


# ---- sizing -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip_test", [False, True])
@pytest.mark.parametrize("in_flight,scenes", [(1, 1), (2, 1), (2, 3)])
def test_tile_footprint_is_the_sum_of_the_plans_queries(cpu_net, in_flight, scenes, flip_test):
    h, w, th, tw, ov, s = 270, 478, 96, 128, 16, 4
    Hp, Wp = frames.padded_size(h, w, 4)
    n_t = len(adapt.tile_origins(Hp, th, ov)) * len(adapt.tile_origins(Wp, tw, ov))
    nv = 4 if flip_test else 1
    plan = engine.StreamPlan(cpu_net._cfg(), th, tw, n_t * nv * adapt.stream_slots(5, in_flight, scenes))
    want = plan.cache_bytes + in_flight * plan.workspace_bytes + in_flight * n_t * 3 * s * th * s * tw * 4 + \
        in_flight * 3 * s * Hp * s * Wp * 4
    if flip_test:
        want += in_flight * (2 * 3 * th * tw * 4 + 4 * 3 * s * th * s * tw * 4)
    assert adapt.tile_footprint(cpu_net, h, w, (th, tw), ov, in_flight, scenes, flip_test) == want
    # the whole frame: one tile of the padded size, no tile buffer
    plan = engine.StreamPlan(cpu_net._cfg(), Hp, Wp, nv * adapt.stream_slots(5, in_flight, scenes))
    want = plan.cache_bytes + in_flight * plan.workspace_bytes + in_flight * 3 * s * Hp * s * Wp * 4
    if flip_test:
        want += in_flight * (2 * 3 * Hp * Wp * 4 + 4 * 3 * s * Hp * s * Wp * 4)
    assert adapt.tile_footprint(cpu_net, h, w, None, ov, in_flight, scenes, flip_test) == want
    assert adapt.tile_footprint(cpu_net, h, w, (512, 512), ov, in_flight, scenes, flip_test) == want


def test_choose_tile(cpu_net):
    h, w = 1080, 1920
    prev = None
    for budget in (10e9, 16e9, 32e9, 64e9, 128e9, 256e9, 1e12):
        th, tw = adapt.choose_tile(cpu_net, h, w, budget)
        n_t = len(adapt.tile_origins(1080, th, 16)) * len(adapt.tile_origins(1920, tw, 16))
        assert th % 4 == 0 and tw % 4 == 0 and min(th, tw) >= 32
        assert adapt.tile_footprint(cpu_net, h, w, (th, tw)) <= budget
        assert engine.StreamPlan(cpu_net._cfg(), th, tw, 6).max_image_bytes < 2 ** 32     # never the whole 1080p frame
        assert prev is None or n_t <= prev, budget                    # monotone: more memory, no more tiles
        prev = n_t
    assert prev == 2                                                  # with all the memory in the world: 1080p in two tiles
    assert adapt.choose_tile(cpu_net, 180, 320, 1e12) == (180, 320)   # a frame that fits is one tile
    with pytest.raises(ValueError, match="choose_tile"):
        adapt.choose_tile(cpu_net, h, w, 1e6)
    with pytest.raises(ValueError):
        adapt.tile_footprint(torch.nn.Identity(), h, w, (64, 64))


# ---- arguments ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(tile=18), dict(tile=12), dict(tile=(16, 18)), dict(tile=(16, 20), tile_overlap=12),
                                dict(tile=32, tile_overlap=6), dict(tile=32, tile_overlap=-4), dict(tile=32, tile_budget=1e9),
                                dict(tile_budget=1e9), dict(tile='auto', tile_budget=0), dict(tile='best'), dict(tile=(16,)),
                                dict(tile=True), dict(tile=16.0), dict(tile=(16, 20), tile_overlap=8.0),
                                dict(tile=(16, 20), tile_overlap=8, multiple=8)], ids=str)
def test_argument_rejections(cpu_net, kw):
    """ValueError with a network on the CPU: the checks come before the device check and the first GPU call."""
    video = torch.zeros((7, 34, 38, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):
        next(adapt.super_resolve_frames(OPT, cpu_net, video, **kw))


def test_good_arguments_reach_the_device_check(cpu_net):
    video = torch.zeros((7, 34, 38, 3), dtype=torch.uint8)
    for kw in (dict(tile=(16, 20), tile_overlap=8), dict(tile=16, tile_overlap=0), dict(tile=(64, 64)), dict(tile=None)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            next(adapt.super_resolve_frames(OPT, cpu_net, video, **kw))


# ---- tile views -----------------------------------------------------------------------------------------
def test_tile_view_rgb():
    rs = np.random.RandomState(0)
    u8 = torch.from_numpy(rs.randint(0, 256, (34, 38, 3)).astype(np.uint8))
    v = frames.tile_view(u8, None, 20, 24, 16, 20)
    assert torch.equal(v, u8[20:34, 24:38]) and v.data_ptr() == u8[20:, 24:].data_ptr()
    f = torch.from_numpy(rs.uniform(0, 1, (3, 34, 38)).astype(np.float32))
    v = frames.tile_view(f, 'chw', 8, 12, 16, 20)
    assert torch.equal(v, f[:, 8:24, 12:32]) and v.data_ptr() == f[:, 8:, 12:].data_ptr()
    for bad in ((34, 0), (0, 38), (-4, 0)):
        with pytest.raises(ValueError):
            frames.tile_view(u8, None, bad[0], bad[1], 16, 20)


@pytest.mark.parametrize("layout", ['nv12', 'i420', 'i422', 'nv16', 'i422p10', 'p210', 'i444'])
def test_tile_view_yuv_packed_and_planar(layout):
    h, w = 34, 38
    rs = np.random.RandomState(1)
    words = frames.layout_depth(layout) > 8
    packed = torch.from_numpy(rs.randint(0, 256, (frames.packed_rows(layout, h), w)).astype(np.uint16 if words else np.uint8))
    planes = frames.yuv_planes(packed, layout)[0]
    loose = tuple(p.clone() for p in planes)
    c420, c444 = layout in frames.YUV_LAYOUTS + frames.YUV16_LAYOUTS, layout in frames.YUV444_LAYOUTS
    sy, sx = (2 if c420 else 1), (1 if c444 else 2)
    for y, x, th, tw in ((0, 0, 16, 20), (8, 12, 16, 20), (20, 20, 16, 20), (0, 0, 64, 64)):
        y1, x1 = min(y + th, h), min(x + tw, w)
        for src in (packed, loose):
            got = frames.tile_view(src, layout, y, x, th, tw)
            ps = frames.yuv_planes(src, layout)[0]
            assert isinstance(got, tuple) and len(got) == len(ps)
            assert torch.equal(got[0], ps[0][y:y1, x:x1])
            for g, p in zip(got[1:], ps[1:]):
                want = p[y // sy:-(-y1 // sy), x // sx:-(-x1 // sx)]
                assert torch.equal(g, want) and g.data_ptr() == want.data_ptr()        # a view: nothing copied
            # what comes back is a frame of the layout: ingest's checks accept it as it is
            assert frames.resolve_layout(got, layout) == (layout, y1 - y, x1 - x)
    if sx == 2:
        with pytest.raises(ValueError, match="chroma sample"):
            frames.tile_view(packed, layout, 0, 3, 16, 20)
    if sy == 2:
        with pytest.raises(ValueError, match="chroma sample"):
            frames.tile_view(packed, layout, 3, 0, 16, 20)
