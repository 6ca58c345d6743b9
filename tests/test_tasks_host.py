"""CPU: the host side of meta-training tasks made on the device (dynavsr_amd/data/tasks.py) -- SequenceIndex and draw_task
against what the reference's VSRBase counted and drew (tests/golden/task_reference.json, recorded by tools/gen_task_golden.py),
the px-from-H quirk, the argument checks of dvsr_task_degrade / dvsr_task_gather (which return before any launch, so device
pointers that nothing reads will do; the host table is real), the ValueErrors of make_batch / TaskSource ahead of their first
GPU call, and the tie-band condition of the recorded comparison in tests/test_gpu_tasks.py."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import task_ref as R
from dynavsr_amd.data import tasks as T

INVALID, UNSUPPORTED = -1, -2
A16 = 0x10000           # a 16-byte aligned address that nothing reads


@pytest.fixture(scope="module")
def lib():
    from dynavsr_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        from dynavsr_amd import build
        build.build()
    return _lib


@pytest.fixture(scope="module")
def reference():
    return R.load_reference()


def test_sequence_index_reproduces_the_recorded_tables(reference):
    meta, _ = reference
    assert len(meta["index"]) == 3
    for cfg in meta["index"]:
        ix = T.SequenceIndex(cfg["lengths"], cfg["n_frames"], cfg["interval_list"])
        assert ix.n_samples == len(ix) == cfg["n_samples"] == len(cfg["table"])
        assert ix.sampling_weights() == cfg["weights"]
        for idx, (key, str_idx, seq_idx, frames) in enumerate(cfg["table"]):
            assert ix.find_set(idx) == (key, str_idx, seq_idx), idx
            assert ix.find(idx) == (key, str_idx, frames), idx
        for bad in (-1, ix.n_samples):
            with pytest.raises(IndexError):
                ix.find(bad)
    strides = {s for cfg in meta["index"] for s in np.atleast_1d(cfg["interval_list"])}
    assert -1 in strides and any(f[3] == sorted(f[3], reverse=True) for f in meta["index"][1]["table"])   # a backward sample
    short = meta["index"][2]
    assert all(row[1] == 0 for row in short["table"] if row[0] == "short")       # too short for the widest stride


def test_draw_task_reproduces_the_recorded_draws(reference):
    meta, _ = reference
    d = meta["draws"]
    h, w = d["frame"]
    py_rng, np_rng = random.Random(d["seed"]), np.random.RandomState(d["seed"])
    assert len(d["draws"]) == 64
    for want in d["draws"]:
        got = T.draw_task(py_rng, np_rng, h, w, 2 * d["patch_size"])
        assert got.pop("crop") == 2 * d["patch_size"]
        assert got == want                                                   # floats included: the same arithmetic
    assert {(x["hflip"], x["vflip"]) for x in d["draws"]} == {(a, b) for a in (False, True) for b in (False, True)}


def test_px_is_drawn_from_the_height_unless_full_width():
    h, w, crop = 72, 96, 64

    def draws(**kw):
        py_rng, np_rng = random.Random(5), np.random.RandomState(5)
        return [T.draw_task(py_rng, np_rng, h, w, crop, **kw) for _ in range(200)]

    quirk, full = draws(), draws(full_width=True)
    assert max(d["px"] for d in quirk) == h - crop and min(d["px"] for d in quirk) == 0     # [0, H - crop]: 24 columns never cut
    assert max(d["px"] for d in full) == w - crop and max(d["py"] for d in full) == h - crop
    # the same generator state gives randrange(0, 9) under the quirk and randrange(0, 33) with the width
    a, b = random.Random(9), random.Random(9)
    assert T.draw_task(a, np.random.RandomState(0), h, w, crop)["px"] == [b.randrange(0, 9), b.randrange(0, 9)][1]
    a, b = random.Random(9), random.Random(9)
    assert T.draw_task(a, np.random.RandomState(0), h, w, crop, full_width=True)["px"] == [b.randrange(0, 9), b.randrange(0, 33)][1]
    with pytest.raises(ValueError, match="full_width"):
        T.draw_task(random.Random(0), np.random.RandomState(0), 96, 72, 64)
    with pytest.raises(ValueError, match="larger"):
        T.draw_task(random.Random(0), np.random.RandomState(0), 72, 96, 80)


def test_draw_order_without_augmentation_and_with_rot():
    """train=False draws no flips; rot is drawn only when asked for (the reference's `and` short-circuits)."""
    a, b = random.Random(3), random.Random(3)
    d = T.draw_task(a, np.random.RandomState(3), 72, 96, 64, augment=False)
    assert (d["hflip"], d["vflip"], d["rot"]) == (False, False, False)
    b.randrange(0, 9), b.randrange(0, 9)
    assert a.random() == b.random()                                          # two randrange and nothing else were consumed
    a, b = random.Random(3), random.Random(3)
    d = T.draw_task(a, np.random.RandomState(3), 72, 96, 64, rot=True)
    want = [b.randrange(0, 9), b.randrange(0, 9), b.random() < 0.5, b.random() < 0.5, b.random() < 0.5]
    assert [d["py"], d["px"], d["hflip"], d["vflip"], d["rot"]] == want
    assert T.draw_flags({"hflip": True, "vflip": False, "rot": True}) == 5


def _table(lib, n=2, src=A16 + 1, row=300, plane=0, kernel=0, flags=0):
    t = (lib.TaskFrame * n)()
    for i in range(n):
        t[i] = lib.TaskFrame(src, row, plane, kernel, flags)
    return t


def test_task_entries_bad_arguments_without_gpu(lib):
    l = lib.lib()
    U8, F32 = lib.FRAME_U8_HWC_RGB, lib.FRAME_F32_CHW

    def degrade(items="default", dev=A16, n=2, fmt=U8, ps=3, H=64, W=80, kernels=A16, nk=2, K=27, scale=4, dst=A16, **row):
        t = _table(lib, max(n, 1), **row) if items == "default" else items
        return l.dvsr_task_degrade(t, dev, n, fmt, ps, H, W, kernels, nk, K, scale, dst, 1, None)

    def gather(items="default", dev=A16, n=2, fmt=U8, ps=3, H=64, W=80, dst=A16, **row):
        t = _table(lib, max(n, 1), **row) if items == "default" else items
        return l.dvsr_task_gather(t, dev, n, fmt, ps, H, W, dst, None)

    f32 = dict(fmt=F32, src=A16, row=80, plane=64 * 80)
    both = [
        (dict(items=None), INVALID, b"null"),
        (dict(dev=None), INVALID, b"null"),
        (dict(dst=None), INVALID, b"null"),
        (dict(src=None), INVALID, b"null source"),
        (dict(n=0), INVALID, b"n=0"),
        (dict(n=21846), UNSUPPORTED, b"65535 planes"),
        (dict(fmt=3), INVALID, b"format"),
        (dict(fmt=-1), INVALID, b"format"),
        (dict(ps=2), INVALID, b"pixel stride"),
        (dict(ps=5), INVALID, b"pixel stride"),
        (dict(row=239), INVALID, b"row stride"),
        (dict(ps=4, row=319), INVALID, b"row stride"),
        (dict(f32, row=79), INVALID, b"row stride"),
        (dict(f32, plane=63 * 80 + 79), INVALID, b"plane stride"),
        (dict(f32, src=A16 + 2), INVALID, b"misaligned fp32 source"),
        (dict(flags=8), INVALID, b"flags"),
        (dict(flags=-1), INVALID, b"flags"),
        (dict(flags=4), INVALID, b"TRANSPOSE"),                              # 64 x 80, 16 x 20: not square
        (dict(dev=A16 + 4), INVALID, b"misaligned table"),
        (dict(dst=A16 + 2), INVALID, b"misaligned"),
        (dict(H=0), INVALID, b"H=0"),
    ]
    for f in (degrade, gather):
        for kw, code, word in both:
            assert f(**kw) == code, (f.__name__, kw)
            assert word in l.dvsr_last_error(), (f.__name__, kw, l.dvsr_last_error())
    only_degrade = [
        (dict(kernels=None), INVALID, b"null"),
        (dict(kernels=A16 + 1), INVALID, b"misaligned"),
        (dict(kernel=2), INVALID, b"kernel index"),
        (dict(kernel=-1), INVALID, b"kernel index"),
        (dict(nk=0), INVALID, b"n_kernels"),
        (dict(K=35), UNSUPPORTED, b"kernel edge"),
        (dict(K=0), UNSUPPORTED, b"kernel edge"),
        (dict(scale=5), UNSUPPORTED, b"scale"),
        (dict(scale=0), UNSUPPORTED, b"scale"),
        (dict(H=13, row=300), INVALID, b"reflection pad"),
        (dict(W=13), INVALID, b"reflection pad"),
        (dict(H=64, W=68, flags=4), INVALID, b"TRANSPOSE"),                  # a square-ish crop whose output 16 x 17 is not
    ]
    for kw, code, word in only_degrade:
        assert degrade(**kw) == code, kw
        assert word in l.dvsr_last_error(), (kw, l.dvsr_last_error())
    # the rows are all looked at: one bad row at the end
    t = _table(lib, 3)
    t[2].flags = 9
    assert gather(items=t, n=3) == INVALID and b"item 2" in l.dvsr_last_error()
    t = _table(lib, 3)
    t[2].kernel = 5
    assert degrade(items=t, n=3) == INVALID and b"item 2" in l.dvsr_last_error()
    assert ctypes.sizeof(lib.TaskFrame) == 32 and T.ITEM.itemsize == 32
    assert [T.ITEM.fields[k][1] for k in ("src", "row_stride", "plane_stride", "kernel", "flags")] == \
        [getattr(lib.TaskFrame, k).offset for k in ("src", "row_stride", "plane_stride", "kernel", "flags")]


class _Pool:
    """A FramePool's host face without a device: what make_batch and TaskSource look at before their first GPU call."""
    layout, format, pixel_stride, device = "hwc_rgb", 1, 3, torch.device("cpu")

    def __init__(self, lengths, h=72, w=96):
        self.lengths, self._hw = dict(lengths), (h, w)
        self.sequences = {k: None for k in lengths}

    def size(self, key):
        return self._hw


def _opt(patch_size=32, scale=4, interval=(1, 2, -1), batch_size=2, kernel_size=21, n_frames=5):
    return {"scale": scale, "datasets": {"train": {"N_frames": n_frames, "interval_list": list(interval), "patch_size": patch_size,
                                                    "kernel_size": kernel_size, "batch_size": batch_size}}}


def _draw(py=0, px=0, crop=64, **kw):
    d = {"py": py, "px": px, "sigma_x": 2.0, "sigma_y": 0.8, "theta": 0.4, "hflip": False, "vflip": False, "rot": False, "crop": crop}
    d.update(kw)
    return d


def test_value_errors_come_before_the_gpu():
    pool = _Pool({"000": 12, "001": 12})
    with pytest.raises(ValueError, match="larger than"):                     # a crop larger than a frame
        T.TaskSource(_opt(patch_size=40), pool)
    with pytest.raises(ValueError, match="a sample needs"):                  # a sequence shorter than a sample
        T.TaskSource(_opt(), _Pool({"000": 12, "001": 4}))
    with pytest.raises(ValueError, match="nothing to reflect"):              # K / 2 = 13 >= h = 4
        T.TaskSource(_opt(patch_size=8), pool)
    with pytest.raises(ValueError, match="full_width"):
        T.TaskSource(_opt(), _Pool({"000": 12}, h=96, w=72))
    with pytest.raises(ValueError, match="rank"):
        T.TaskSource(_opt(), pool, rank=2, world=2)
    with pytest.raises(ValueError, match="batch_size"):
        T.TaskSource(_opt(batch_size=1), pool, world=2)
    with pytest.raises(ValueError, match="scale"):
        T.TaskSource(_opt(scale=5), pool)
    src = T.TaskSource(_opt(), pool, seed=1)                                 # arguments that pass touch no device
    assert len(src) == src.index.n_samples // 2 and src.crop == 64
    picks, draws = src.draw([0, 1])
    assert len(picks) == len(draws) == 2 and all(len(f) == 5 for _, f in picks)
    good = [("000", [0, 1, 2, 3, 4]), ("001", [4, 3, 2, 1, 0])]
    for picks_, draws_, word in (
            (good, [_draw(), _draw(py=9)], "outside"),                       # 9 + 64 > 72
            (good, [_draw(), _draw(px=33)], "outside"),
            (good, [_draw(), _draw(crop=32)], "one crop size"),
            (good, [_draw()], "picks and"),
            ([("000", [0, 1, 2, 3, 12]), good[1]], [_draw(), _draw()], "frames"),
            ([("000", [0, 1, 2]), good[1]], [_draw(), _draw()], "frames"),
            ([("nope", [0, 1, 2, 3, 4]), good[1]], [_draw(), _draw()], "no sequence"),
            (good, [_draw(crop=16), _draw(crop=16)], "nothing to reflect"),
            (good, [_draw(crop=12), _draw(crop=12)], "reflection pad")):
        with pytest.raises(ValueError, match=word):
            T.make_batch(pool, picks_, draws_, 21, 4)
    with pytest.raises(ValueError, match="scale"):
        T.make_batch(pool, good, [_draw(), _draw()], 21, 5)
    with pytest.raises(ValueError, match="kernel_size"):
        T.make_batch(pool, good, [_draw(), _draw()], 0, 4)


def test_shifted_kernels_pad_to_the_largest_edge():
    """Every task's kernel is Degradation's own shifted kernel; edges that differ inside a batch are zero-padded alike."""
    from dynavsr_amd.data.random_kernel_generator import Degradation
    draws = [_draw(sigma_x=0.2 + 0.7 * i, sigma_y=4.9 - 0.6 * i, theta=-3.0 + 0.8 * i) for i in range(8)]
    for scale, ks in ((4, 21), (3, 21), (2, 21)):
        k = T.shifted_kernels(draws, ks, scale)
        assert k.dtype == np.float32 and k.shape[0] == 8 and k.shape[1] == k.shape[2]
        for i, d in enumerate(draws):
            g = Degradation(ks, scale, theta=d["theta"], sigma=[d["sigma_x"], d["sigma_y"]])
            own = g.kernel_shift(g.kernel).astype(np.float32)
            p = (k.shape[1] - own.shape[0]) // 2
            assert (k.shape[1] - own.shape[0]) % 2 == 0
            assert np.array_equal(k[i, p:k.shape[1] - p, p:k.shape[1] - p], own)
            assert np.count_nonzero(k[i]) == np.count_nonzero(own)           # zeros around it
    assert T.shifted_kernels(draws, 21, 4).shape[1] == 27 == T.nominal_edge(21, 4)
    assert T.nominal_edge(21, 2) == 25 and T.check_geometry(64, 27, 4) == (16, 4) and T.check_geometry(64, 25, 2) == (32, 16)


def test_recorded_tasks_are_what_the_gpu_test_expects(reference):
    """The shapes of the recorded tasks, the draws they carry, and that GT is the crop of the source bytes, flipped."""
    meta, z = reference
    assert [t["scale"] for t in meta["tasks"]] == [4, 4, 4, 4, 2]
    for t in meta["tasks"]:
        n, d, s = t["name"], t["draw"], t["scale"]
        h = 64 // s
        assert z[n + "_src"].shape == (5, 72, 96, 3) and z[n + "_gt"].shape == (5, 3, 64, 64)
        assert z[n + "_lr_unq"].shape == z[n + "_lqs"].shape == (5, 3, h, h) and z[n + "_slq"].shape == (5, 3, h // s, h // s)
        assert z[n + "_kernel"].shape == (21, 21)
        for i, f in enumerate(t["frames"]):
            assert np.array_equal(z[n + "_src"][i], R.frame_bytes(R.frame_name(t["key"], f)))
        crop = z[n + "_src"][:, d["py"]:d["py"] + 64, d["px"]:d["px"] + 64].transpose(0, 3, 1, 2)
        assert np.array_equal(R.flip_np(crop, R.flags_of(d)), z[n + "_gt"])
    for i, t in enumerate(meta["tasks"][:4]):
        assert t["draw"] == meta["draws"]["draws"][i] and t["idx"] == meta["draws"]["indices"][i]


def test_tie_band_leaves_out_little(reference):
    """The recorded comparison holds LQs to the recorded 8-bit level where the recorded unquantised LR is more than TIE_BAND away
    from a rounding tie; that must leave out no more than 2 % of the values of every task, or the test would check little."""
    meta, z = reference
    for t in meta["tasks"]:
        y = z[t["name"] + "_lr_unq"]
        left_out = 1.0 - float(R.outside_tie_band(y).mean())
        print("%s: left out %.3f %% of %d" % (t["name"], 100 * left_out, y.size))
        assert left_out <= 0.02
        assert float(y.min()) < 0.2 and float(y.max()) > 0.8                 # the data spans the levels
        # the recorded LQs is that LR, quantised and flipped
        q = np.round(np.clip(y * np.float32(255), 0, 255)) / np.float32(255)
        assert np.array_equal(R.flip_np(q, R.flags_of(t["draw"])), z[t["name"] + "_lqs"])
