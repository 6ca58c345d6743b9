"""CPU: the Level-1 drop-in recipe of INTEGRATION.md, checked against what the reference drivers use.

With INTEGRATION's exact PYTHONPATH (dynavsr_amd first, then the repo, then codes/) a fresh interpreter
resolves what codes/test_dynavsr.py and codes/train_dynavsr.py use:
  * every project-local import (``data.*``, ``utils.*``, ``options.*``, ``models.*``) to a module file,
  * every ``util.X`` / ``option.X`` attribute the drivers touch, on THIS build's modules,
  * every method the drivers call on the model wrappers, on this build's wrapper classes.
Nothing of the reference is copied or shipped: the drivers were parsed once by oracle/gen_golden.py, which recorded
the names they use (tests/golden/dropin_drivers.json).  The host helpers of utils/util.py are also checked here
against the oracle's independent restatements (tests may import oracle/)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

# What the reference's two drivers use, recorded as names and line numbers by oracle/gen_golden.py (dropin): every
# project-local import with the provider the Level-1 recipe resolved it to ("codes": the reference's own file, relative to
# codes/; "repo": this build), every util.X / option.X, every attribute used on the model wrappers.
_RESOLVER = r"""
import ast, importlib.util, inspect, json, sys
uses = json.load(open(sys.argv[1]))["drivers"]
report = {"imports": {}, "missing_modules": [], "missing_attrs": [], "missing_methods": []}
import options.options as option
from utils import util
import models
from models.Video_base_model import VideoBaseModel
from models.LRestimator_model import LRimgestimator_Model
alias = {"util": util, "option": option}
def provides(cls, name):     # a method, or an attribute some method of the class (or a base) assigns on self
    if callable(getattr(cls, name, None)):
        return True
    for k in cls.__mro__[:-1]:
        for n in ast.walk(ast.parse(inspect.getsource(k))):
            if isinstance(n, ast.Attribute) and isinstance(n.ctx, ast.Store) and isinstance(n.value, ast.Name) \
                    and n.value.id == "self" and n.attr == name:
                return True
    return False
wrappers = {"model": VideoBaseModel, "modelcp": VideoBaseModel, "est_model": LRimgestimator_Model,
            "est_modelcp": LRimgestimator_Model, "est_model_fixed": LRimgestimator_Model}
for path, u in sorted(uses.items()):
    for m in sorted(u["imports"]):
        try:
            spec = importlib.util.find_spec(m)
        except Exception as e:
            spec = None
        if spec is None or not spec.origin:
            report["missing_modules"].append([path, m])
        else:
            report["imports"][m] = spec.origin
    for name, attr, line in u["attrs"]:
        if not hasattr(alias[name], attr):
            report["missing_attrs"].append([path, name + "." + attr, line])
    for name, attr, line in u["methods"]:
        if not provides(wrappers[name], attr):     # methods called and attributes read / written
            report["missing_methods"].append([path, name + "." + attr, line])
report["util_file"], report["option_file"], report["models_file"] = util.__file__, option.__file__, models.__file__
print(json.dumps(report))
"""


def test_level1_recipe_resolves_everything_the_drivers_use(tmp_path):
    rec_path = os.path.join(GOLDEN, "dropin_drivers.json")
    with open(rec_path) as f:
        uses = json.load(f)["drivers"]
    assert sorted(uses) == ["test_dynavsr.py", "train_dynavsr.py"]
    # a stand-in codes/ tree holding (empty) the reference files the recipe resolved the dataset imports to
    codes = tmp_path / "codes"
    theirs = {}
    for u in uses.values():
        for m, where in u["imports"].items():
            if where["provider"] == "codes":
                f = codes / where["file"]
                f.parent.mkdir(parents=True, exist_ok=True)
                f.write_text("")
                theirs[m] = str(f)
    assert {"data.data_sampler", "data.meta_learner"} <= set(theirs)
    env = dict(os.environ)
    # INTEGRATION.md, Level 1: PYTHONPATH=<repo>/dynavsr_amd:<repo>:<codes>
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "dynavsr_amd"), ROOT, str(codes)])
    env["PYTHONDONTWRITEBYTECODE"] = "1"
    r = subprocess.run([sys.executable, "-c", _RESOLVER, rec_path], env=env, cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert rep["missing_modules"] == [], rep["missing_modules"]
    assert rep["missing_attrs"] == [], rep["missing_attrs"]
    assert rep["missing_methods"] == [], rep["missing_methods"]
    # who provides what: models / options / utils.util are this build's, the dataset code is the codes/ tree's
    for k in ("util_file", "option_file", "models_file"):
        assert os.path.join(ROOT, "dynavsr_amd") in rep[k], rep[k]
    imp = rep["imports"]
    for m, f in theirs.items():
        assert imp[m] == f, (m, imp[m])
    for u in uses.values():
        for m, where in u["imports"].items():
            if where["provider"] == "repo":
                assert imp[m].startswith(os.path.join(ROOT, "dynavsr_amd")), (m, imp[m])
    assert imp["options.options"].startswith(ROOT) and imp["models"].startswith(ROOT) and imp["utils"].startswith(ROOT)


def test_packages_do_not_shadow_a_codes_tree(tmp_path):
    """Same mechanism without the reference: a stand-in codes/ tree with data/other.py and utils/other.py next to
    this build on the path -- both must stay importable, and `data.random_kernel_generator` of that tree wins
    (the DataLoader workers call it with CPU tensors; the device version is an explicit opt-in)."""
    codes = tmp_path / "codes"
    for pkg in ("data", "utils"):
        (codes / pkg).mkdir(parents=True)
        (codes / pkg / "__init__.py").write_text("")
        (codes / pkg / "other.py").write_text("WHO = 'codes'\n")
    (codes / "data" / "random_kernel_generator.py").write_text("WHO = 'codes'\n")
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "dynavsr_amd"), ROOT, str(codes)])
    code = ("import data.other, utils.other, data.random_kernel_generator as r\n"
            "from utils import util\n"
            "assert data.other.WHO == utils.other.WHO == r.WHO == 'codes'\n"
            "assert 'dynavsr_amd' in util.__file__ and hasattr(util, 'ProgressBar')\n"
            "import dynavsr_amd.data.random_kernel_generator as ours\n"
            "assert hasattr(ours, 'Degradation')\n")
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=str(tmp_path), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- utils/util.py host helpers -------------------------------------------------------------------
def test_util_ssim_psnr_match_the_oracle():
    from dynavsr_amd.utils import util
    from oracle import metrics as om
    rng = np.random.RandomState(3)
    a = rng.randint(0, 256, (37, 45, 3)).astype(np.uint8)
    b = np.clip(a.astype(np.int32) + rng.randint(-9, 10, a.shape), 0, 255).astype(np.uint8)
    assert abs(util.calculate_ssim(a, b) - om.calculate_ssim(a, b)) < 1e-12
    assert abs(util.calculate_ssim(a[:, :, 0], b[:, :, 0]) - om.calculate_ssim(a[:, :, 0], b[:, :, 0])) < 1e-12
    assert abs(util.calculate_ssim(a[:, :, :1], b[:, :, :1]) - util.calculate_ssim(a[:, :, 0], b[:, :, 0])) < 1e-15
    assert util.calculate_psnr(a, b) == om.calculate_psnr(a, b) and util.calculate_psnr(a, a) == float("inf")
    assert util.calculate_ssim(a, a) == pytest.approx(1.0, abs=1e-12)
    with pytest.raises(ValueError):
        util.calculate_ssim(a, b[:-1])
    with pytest.raises(ValueError):
        util.calculate_ssim(a[None], b[None])


def test_util_tensor2img_variants():
    from dynavsr_amd.utils import util
    from oracle import metrics as om
    t = torch.rand(3, 9, 11) * 1.4 - 0.2
    rgb, bgr = util.tensor2img(t, mode='rgb'), util.tensor2img(t)
    assert rgb.dtype == np.uint8 and rgb.shape == (9, 11, 3) and np.array_equal(rgb[:, :, ::-1], bgr)
    assert np.array_equal(rgb, om.tensor2img_rgb(t.numpy()))
    assert np.array_equal(util.tensor2rgbimg(t), rgb)
    assert util.tensor2img(t[0]).shape == (9, 11)
    assert util.tensor2img(t, out_type=np.float32, mode='rgb').max() <= 1.0
    # 4-D: make_grid tiling, nrow = floor(sqrt(B)), 2 px of zero padding around every tile
    g = util.tensor2img(torch.ones(5, 3, 4, 6), mode='rgb')
    assert g.shape == (3 * 6 + 2, 2 * 8 + 2, 3)
    assert g[:2].max() == 0 and g[2:6, 2:8].min() == 255 and g[2:6, 8:10].max() == 0 and g[14:18, 10:16].max() == 0
    assert util.tensor2img(torch.ones(1, 3, 4, 6)).shape == (4, 6, 3)       # squeeze() drops the batch of one
    with pytest.raises(TypeError):
        util.tensor2img(torch.ones(2, 2, 3, 4, 6))
    assert [v.shape for v in util.crop_border([rgb, bgr], 2)] == [(5, 7, 3)] * 2 and util.crop_border([rgb], 0)[0] is rgb


def test_util_files_logger_progress(tmp_path, capsys):
    import logging
    from dynavsr_amd.utils import util
    d = tmp_path / "exp"
    util.mkdirs([str(d), str(tmp_path / "a" / "b")])
    util.mkdir(str(d))
    (d / "x.txt").write_text("1")
    util.mkdir_and_rename(str(d))
    assert d.is_dir() and not list(d.iterdir())
    assert any(p.name.startswith("exp_archived_") and (p / "x.txt").exists() for p in tmp_path.iterdir())
    util.setup_logger("dropin_test", str(tmp_path), "val", level=logging.INFO, screen=False, tofile=True)
    logging.getLogger("dropin_test").info("hello")
    logs = [p for p in tmp_path.iterdir() if p.name.startswith("val_") and p.suffix == ".log"]
    assert len(logs) == 1 and "INFO: hello" in logs[0].read_text()
    util.set_random_seed(7)
    a = (np.random.rand(), torch.rand(1).item())
    util.set_random_seed(7)
    assert a == (np.random.rand(), torch.rand(1).item())
    bar = util.ProgressBar(3)
    for i in range(3):
        bar.update("step %d" % i)
    out = capsys.readouterr().out
    assert "3/3" in out and "step 2" in out and bar.completed == 3
    util.ProgressBar(0).update()
    assert "completed: 1" in capsys.readouterr().out
    # PNG writer: decodable by an independent inflate + un-filter
    import struct, zlib
    img = np.random.RandomState(0).randint(0, 256, (5, 7, 3)).astype(np.uint8)
    util.save_img(img, str(tmp_path / "f.png"))                               # BGR in, like cv2.imwrite
    raw = (tmp_path / "f.png").read_bytes()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n" and struct.unpack(">II", raw[16:24]) == (7, 5)
    n = struct.unpack(">I", raw[33:37])[0]
    rows = np.frombuffer(zlib.decompress(raw[41:41 + n]), np.uint8).reshape(5, 1 + 7 * 3)
    assert rows[:, 0].max() == 0 and np.array_equal(rows[:, 1:].reshape(5, 7, 3), img[:, :, ::-1])


def test_util_duf_downsample_and_flip_forward():
    from dynavsr_amd.utils import util
    x = torch.rand(1, 2, 3, 32, 40)
    y = util.DUF_downsample(x, scale=4)
    assert y.shape == (1, 2, 3, 8, 10)
    c = torch.full((1, 1, 3, 32, 32), 0.25)
    assert torch.allclose(util.DUF_downsample(c, scale=2), torch.full((1, 1, 3, 16, 16), 0.25), atol=1e-6)
    net = torch.nn.Conv2d(3, 3, 3, padding=1)
    inp = torch.rand(1, 3, 8, 8)
    ref = util.single_forward(net, inp)
    assert torch.equal(ref, net(inp).detach())
    sym = util.flipx4_forward(lambda t: (t * 2, None), inp)                   # tuple outputs: first element
    assert torch.allclose(sym, inp * 2, atol=1e-7)


def test_backbone_state_dicts_match_the_reference_modules():
    """networks.define_G's three video backbones expose exactly the reference modules' state-dict keys and shapes (in order),
    so reference checkpoints load with strict=True.  The reference's keys and shapes are recorded by oracle/gen_golden.py
    (dropin) in tests/golden/backbone_state_dicts.json; nothing else of the reference is used."""
    from dynavsr_amd.models.archs import DUF_arch, EDVR_arch, TOF_arch
    with open(os.path.join(GOLDEN, "backbone_state_dicts.json")) as f:
        rec = json.load(f)["networks"]
    nets = {"TOF": lambda: TOF_arch.TOFlow(adapt_official=True)}
    for n in ("DUF_16L", "DUF_28L", "DUF_52L"):
        for s in (2, 3, 4):
            nets[n + "x%d" % s] = (lambda n=n, s=s: getattr(DUF_arch, n)(scale=s, adapt_official=True))
    for s in (2, 4):
        cfg = dict(nf=64, nframes=5, groups=8, front_RBs=5, back_RBs=10, scale=s)
        nets["EDVR-Mx%d" % s] = (lambda cfg=cfg: EDVR_arch.EDVR(**cfg))
    assert len(nets) == 12 and sorted(nets) == sorted(rec)
    bad = []
    for name, make in nets.items():
        sd = make().state_dict()
        if [[k, list(v.shape)] for k, v in sd.items()] != rec[name]:
            bad.append(name)
    assert bad == [], bad


def test_async_png_writer(tmp_path):
    """Background PNG writer: same bytes as the synchronous path, the caller's buffer may be reused
    right after the call, errors surface at flush_png()."""
    from dynavsr_amd.utils import util
    rs = np.random.RandomState(1)
    imgs = [rs.randint(0, 256, (24, 40, 3)).astype(np.uint8) for _ in range(6)]
    for i, im in enumerate(imgs):
        util.write_png(str(tmp_path / ("s%d.png" % i)), im)
    util.async_png(True)
    try:
        buf = np.empty_like(imgs[0])
        for i, im in enumerate(imgs):
            buf[...] = im
            util.write_png(str(tmp_path / ("a%d.png" % i)), buf)      # the writer copies at the call
            buf[...] = 0
        util.save_img(imgs[0], str(tmp_path / "a_bgr.png"))
        util.flush_png()
        for i in range(6):
            assert (tmp_path / ("a%d.png" % i)).read_bytes() == (tmp_path / ("s%d.png" % i)).read_bytes()
        util.write_png(str(tmp_path / "no_such_dir" / "x.png"), imgs[0])
        with pytest.raises(OSError):
            util.flush_png()
        util.flush_png()                                               # the error is reported once
    finally:
        util.async_png(False)
    util.save_img(imgs[0], str(tmp_path / "s_bgr.png"))
    assert (tmp_path / "a_bgr.png").read_bytes() == (tmp_path / "s_bgr.png").read_bytes()
