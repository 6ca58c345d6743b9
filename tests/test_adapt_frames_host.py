"""CPU: the host side of adapt.adapt_frames -- the multiple a clip is padded to, the argument errors (every one a ValueError
before the first GPU call: CPU tensors, no networks), the region arithmetic, and the region losses' symbols."""
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT


def _opt(which="EDVR", scale=4):
    from dynavsr_amd.options import options as option
    opt = option.dict_to_nonedict(option.parse(os.path.join(
        ROOT, "dynavsr_amd", "options", "test", "EDVR", "EDVR_M_S4.yml"), is_train=False))
    opt["dist"] = False
    opt["scale"] = scale
    opt["network_G"]["which_model_G"] = which
    return opt


def test_adapt_multiple():
    from dynavsr_amd.adapt import adapt_multiple
    assert adapt_multiple(_opt("EDVR", 4)) == 16
    assert adapt_multiple(_opt("EDVR", 2)) == 8
    assert adapt_multiple(_opt("TOF", 4)) == 16
    assert adapt_multiple(_opt("DUF", 4)) == 4
    assert adapt_multiple(_opt("TOF", 3)) == 48 and adapt_multiple(_opt("DUF", 3)) == 3
    with pytest.raises(ValueError, match="which_model_G"):
        adapt_multiple(_opt("SRResNet", 4))


def _run(opt, frames, **kw):
    """Advances the generator once with no networks at all: whatever it raises, it raises before it touches one."""
    from dynavsr_amd.adapt import adapt_frames
    return next(adapt_frames(opt, None, None, None, None, None, frames, **kw))


def test_argument_errors_come_before_the_first_gpu_call():
    opt = _opt()
    u8 = torch.zeros((7, 30, 44, 3), dtype=torch.uint8)
    f32 = torch.zeros((7, 3, 32, 48))
    gt = torch.zeros((7, 120, 176, 3), dtype=torch.uint8)
    real = _opt()
    real["train"]["use_real"] = True
    with pytest.raises(ValueError, match="use_real"):
        _run(real, u8)
    with pytest.raises(ValueError, match="layout"):
        _run(opt, u8, layout="rgb24")
    with pytest.raises(ValueError, match="out="):
        _run(opt, u8, out="png")
    with pytest.raises(ValueError, match="planar"):
        _run(opt, f32, layout="hwc_rgb")
    with pytest.raises(ValueError, match="needs scores"):
        _run(opt, u8, gt=gt)
    with pytest.raises(ValueError, match="needs scores"):
        _run(opt, u8, gt=gt, scores=torch.zeros((7, 2), dtype=torch.float64))          # on the CPU
    with pytest.raises(ValueError, match="scores without gt"):
        _run(opt, u8, scores=torch.zeros((7, 2), dtype=torch.float64))
    with pytest.raises(ValueError, match="baseline=True"):
        _run(opt, u8, baseline=False, baseline_scores=torch.zeros((7, 2), dtype=torch.float64))
    with pytest.raises(ValueError, match="baseline_scores without gt"):
        _run(opt, u8, baseline_scores=torch.zeros((7, 2), dtype=torch.float64))
    assert opt["train"]["maml"]["adapt_iter"] == 1
    for bad in (torch.zeros((7, 2)), torch.zeros((6, 1)), torch.zeros((7,)), torch.zeros((7, 1), dtype=torch.float64), [0.0] * 7):
        with pytest.raises(ValueError, match="losses"):
            _run(opt, u8, losses=bad)
    with pytest.raises(ValueError, match="on the GPU"):
        _run(opt, u8, losses=torch.zeros((7, 1)))
    with pytest.raises(ValueError, match="packed nv12"):
        _run(opt, u8, out="nv12", out_size=(91, 133))
    with pytest.raises(ValueError, match="packed i422"):
        _run(opt, u8, out="i422", out_size=(90, 133))
    with pytest.raises(ValueError, match="multiple of 16"):
        _run(opt, u8, multiple=8)
    with pytest.raises(ValueError, match="pad_mode"):
        _run(opt, u8, pad_mode="zeros")
    with pytest.raises(ValueError, match="reflect pad"):
        _run(opt, torch.zeros((7, 6, 44, 3), dtype=torch.uint8))                         # 6 -> 16 rows cannot be reflected
    with pytest.raises(ValueError, match="no frames"):
        _run(opt, [])
    with pytest.raises(ValueError, match="out_size"):
        _run(opt, u8, out_size=(20, 176))                                                # 120 -> 20 is more than 4 : 1
    patch = _opt()
    patch["train"]["maml"].update({"use_patch": True, "num_patch": 2, "patch_size": 8})
    with pytest.raises(ValueError, match="patch"):
        _run(patch, torch.zeros((7, 8, 8, 3), dtype=torch.uint8), pad_mode="replicate")  # 2 x 2 whole SLR cells, a patch is 4 x 4


def test_region_arithmetic():
    """The SLR term counts the cells that hold at least one real pixel (ceil), the patches are drawn over the cells that hold
    real pixels alone (floor): h % s in {0, 1, s - 1}."""
    from dynavsr_amd.adapt import check_adapt_region, patch_region, slr_region
    s = 4
    for h, ceil_, floor_ in ((28, 7, 7), (29, 8, 7), (31, 8, 7), (32, 8, 8)):
        assert slr_region((h, 44), s) == (ceil_, 11)
        assert patch_region((h, 44), s) == (floor_, 11)
        assert slr_region((44, h), s) == (11, ceil_) and patch_region((44, h), s) == (11, floor_)
    assert slr_region((1, 1), 4) == (1, 1) and patch_region((3, 3), 4) == (0, 0)
    assert slr_region((30, 45), 2) == (15, 23) and patch_region((30, 45), 2) == (15, 22)
    opt = _opt()
    assert check_adapt_region(opt, (1, 5, 3, 32, 48), None) is None
    assert check_adapt_region(opt, (1, 5, 3, 32, 48), (32, 48)) is None                  # the whole clip: the calls of before
    assert check_adapt_region(opt, (1, 5, 3, 32, 48), (30, 44)) == (30, 44)
    for bad in ((0, 44), (33, 48), (32, 49), (30,), "30x44", (30.0, 44)):
        with pytest.raises(ValueError):
            check_adapt_region(opt, (1, 5, 3, 32, 48), bad)
    opt["train"]["maml"].update({"use_patch": True, "num_patch": 2, "patch_size": 8})    # the crop's edge is patch_size // 2 = 4
    assert check_adapt_region(opt, (1, 5, 3, 32, 48), (30, 44)) == (30, 44)
    assert check_adapt_region(opt, (1, 5, 3, 32, 48), (16, 19)) == (16, 19)
    with pytest.raises(ValueError, match="patch"):
        check_adapt_region(opt, (1, 5, 3, 32, 48), (15, 44))                             # floor(15 / 4) = 3 < 4
    with pytest.raises(ValueError, match="patch"):
        check_adapt_region(opt, (1, 5, 3, 16, 16), (8, 8))
    opt["train"]["maml"]["patch_size"] = 4                                               # an edge of 2: EDVR takes multiples of 4
    for region in ((8, 8), (30, 44)):
        with pytest.raises(ValueError, match="multiples of 4"):
            check_adapt_region(opt, (1, 5, 3, 32, 48), region)
    tof = _opt("TOF")
    tof["train"]["maml"].update({"use_patch": True, "num_patch": 2, "patch_size": 36})   # TOFlow: cut at the clip's own size
    assert check_adapt_region(tof, (1, 7, 3, 32, 48), (30, 44)) == (30, 44)
    with pytest.raises(ValueError, match="patch"):
        check_adapt_region(tof, (1, 7, 3, 32, 48), (17, 44))


REGION_SYMBOLS = ["dvsr_charbonnier_region_forward", "dvsr_charbonnier_region_backward",
                  "dvsr_l1_tail_region_forward", "dvsr_l1_tail_region_backward"]


def test_region_symbols_in_header_library_and_ctypes_table():
    from dynavsr_amd import _lib
    header = open(os.path.join(ROOT, "include", "dynavsr_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(re.findall(r" T (dvsr_[a-z0-9_]+)", nm))
    for name in REGION_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in exported, name
        assert name in _lib.lib()._signatures, name


def test_region_entry_points_check_their_arguments():
    """DVSR_REQUIRE in front of the launch: a region outside the plane, null pointers -- host code, no GPU."""
    from dynavsr_amd import _lib
    l = _lib.lib()
    assert l.dvsr_charbonnier_region_forward(None, None, None, 1, 3, 8, 8, 4, 4, 1e-6, None, 0, None) == -1
    assert b"null" in l.dvsr_last_error()
    for h, w in ((0, 4), (9, 4), (4, 0), (4, 9)):
        assert l.dvsr_charbonnier_region_backward(16, 16, 16, 16, 1, 3, 8, 8, h, w, 1e-6, None) == -1
        assert b"region" in l.dvsr_last_error()
        assert l.dvsr_l1_tail_region_backward(16, 16, 16, 10.0, 16, 1, 3, 8, 8, h, w, None) == -1
        assert b"region" in l.dvsr_last_error()
    assert l.dvsr_l1_tail_region_forward(16, 16, None, 10.0, 16, 0, 3, 8, 8, 4, 4, 16, 1 << 20, None) == -1
    assert l.dvsr_l1_tail_region_forward(16, 16, None, 10.0, 16, 2, 3, 8, 8, 4, 4, 16, 4096, None) != 0     # workspace of one group
