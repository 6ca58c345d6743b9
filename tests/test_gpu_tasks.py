"""GPU: meta-training tasks made on the device -- dvsr_task_degrade and dvsr_task_gather against the per-item composition of
today's entries bit for bit, make_batch against the per-task loop, the five recorded tasks of the reference's own __getitem__
(tests/golden/task_reference*.npz, recorded by tools/gen_task_golden.py), and a TaskSource end to end."""
import ctypes
import os

import numpy as np
import pytest
import torch

import task_ref as R
from conftest import ROOT
from dynavsr_amd import _lib as L
from dynavsr_amd import frames
from dynavsr_amd.data import tasks as T
from dynavsr_amd.data.random_kernel_generator import Degradation

pytestmark = pytest.mark.gpu
DEV = "cuda"
U8_LAYOUT = {L.FRAME_U8_HWC_RGB: "hwc_rgb", L.FRAME_U8_HWC_BGR: "hwc_bgr"}
KERNEL_PARAMS = ((0.4, [2.0, 0.8]), (1.0, [1.0, 3.0]), (-2.1, [4.4, 0.3]))     # (theta, sigma) of up to three tasks


def byte_video(seed, t, h, w, c=3):
    r = np.random.RandomState(seed)
    v = np.stack([R.frame_bytes("v%d/%d" % (seed, i), h, w) for i in range(t)])
    if c == 4:
        v = np.concatenate([v, r.randint(0, 256, size=v.shape[:3] + (1,)).astype(np.uint8)], -1)
    return torch.from_numpy(v)


def table_of(views, fmt, kernel_of, flags_of):
    """(host table, device copy) of crops given as tensor views: uint8 [H,W,3|4] or float32 [3,H,W] with contiguous columns."""
    t = (L.TaskFrame * len(views))()
    for i, v in enumerate(views):
        if fmt == L.FRAME_F32_CHW:
            assert v.stride(2) == 1
            t[i] = L.TaskFrame(v.data_ptr(), v.stride(1), v.stride(0), kernel_of(i), flags_of(i))
        else:
            assert v.stride(2) == 1 and v.stride(1) in (3, 4)
            t[i] = L.TaskFrame(v.data_ptr(), v.stride(0), 0, kernel_of(i), flags_of(i))
    host = np.frombuffer(t, dtype=np.uint8)
    return t, torch.from_numpy(host.copy()).to(DEV)


def ingested(view, fmt):
    """The contiguous fp32 [3,H,W] crop that today's entries see."""
    if fmt == L.FRAME_F32_CHW:
        return frames.ingest(view, "chw", multiple=1).contiguous()
    return frames.ingest(view, U8_LAYOUT[fmt], multiple=1).contiguous()


def degradations(n, ks, scale):
    ds = [Degradation(ks, scale, theta=th, sigma=sg) for th, sg in KERNEL_PARAMS[:n]]
    kernels = torch.cat([d._shifted_on(DEV) for d in ds]).contiguous()
    return ds, kernels


def run_degrade(views, fmt, ps, H, W, ds, kernels, scale, kernel_of, flags_of, quantise):
    n, K = len(views), int(kernels.shape[-1])
    ho, wo = T.lr_size(H, K, scale), T.lr_size(W, K, scale)
    host, dev = table_of(views, fmt, kernel_of, flags_of)
    dst = torch.full((n, 3, ho, wo), float("nan"), device=DEV)
    L.check(L.lib().dvsr_task_degrade(host, dev.data_ptr(), n, fmt, ps, H, W, kernels.data_ptr(), kernels.shape[0], K, scale,
                                      dst.data_ptr(), quantise, L.stream()), "dvsr_task_degrade")
    torch.cuda.synchronize()
    assert not torch.isnan(dst).any()
    for i, v in enumerate(views):
        want = R.flip_t(ds[kernel_of(i)].apply(ingested(v, fmt)[None], quantise=bool(quantise))[0], flags_of(i))
        assert torch.equal(dst[i], want), (i, flags_of(i), float((dst[i] - want).abs().max()))


def case_views(case):
    """(views, fmt, pixel stride, H, W, tasks, flags_of) of the table cases: 1 = two byte sequences of different pitch, ragged
    tile; 2 = pixel stride 4, BGR, one byte off alignment, 3 x 3 tiles; 3 = fp32 planar, pitched rows, transposes; 5 = one item."""
    if case in (1, 5):
        a = byte_video(1, 5, 72, 96).to(DEV)                                           # pitch 288
        b = torch.zeros(5, 70, 112, 3, dtype=torch.uint8, device=DEV)
        b[:, :, :100] = byte_video(2, 5, 70, 100).to(DEV)
        b = b[:, :, :100]                                                              # pitch 336
        H, W = 64, 80
        crops = [(a, 3, 7), (b, 6, 20), (a, 8, 16)]
        views = [s[f, py:py + H, px:px + W] for s, py, px in crops for f in range(5)]
        if case == 5:
            return views[7:8], L.FRAME_U8_HWC_RGB, 3, H, W, 1, lambda i: 3
        return views, L.FRAME_U8_HWC_RGB, 3, H, W, 3, lambda i: i % 4                   # 0, 1, 2, 3 spread over the tasks
    if case == 2:
        H, W, fh, fw = 144, 272, 150, 280
        flat = torch.zeros(1 + 5 * fh * fw * 4, dtype=torch.uint8, device=DEV)
        flat[1:] = byte_video(3, 5, fh, fw, 4).to(DEV).reshape(-1)
        v = flat[1:].view(5, fh, fw, 4)
        assert v.data_ptr() % 2 == 1
        crops = [(2, 5), (6, 3)]
        return [v[f, py:py + H, px:px + W] for py, px in crops for f in range(5)], L.FRAME_U8_HWC_BGR, 4, H, W, 2, lambda i: (i * 3) % 4
    if case == 3:
        H = W = 64
        base = torch.rand(5, 3, 70, 72, generator=torch.Generator().manual_seed(4)).to(DEV)[:, :, :, :68]
        crops = [(1, 3), (6, 0)]
        return [base[f, :, py:py + H, px:px + W] for py, px in crops for f in range(5)], L.FRAME_F32_CHW, 1, H, W, 2, lambda i: 4 + i % 4
    raise ValueError(case)


# (case, kernel_size, scale): K = 27 takes the phase-plane kernel (4, 7), K = 25 at scale 2 the (2, 13) one, K = 19 the generic
DEGRADE_CASES = [(1, 21, 4), (2, 21, 4), (3, 21, 4), (1, 21, 2), (1, 13, 4), (5, 21, 4)]


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("case,ks,scale", DEGRADE_CASES)
def test_task_degrade_is_the_composition(case, ks, scale, generic, monkeypatch):
    """Item i, plane c = Degradation.apply on the contiguous crop of frames.ingest(view, multiple=1) with the item's kernel,
    flipped / transposed by its flags: torch.equal, quantiser on and off, and under DVSR_DEGRADE_GENERIC."""
    views, fmt, ps, H, W, tasks, flags_of = case_views(case)
    ds, kernels = degradations(tasks, ks, scale)
    assert int(kernels.shape[-1]) == {(21, 4): 27, (21, 2): 25, (13, 4): 19}[(ks, scale)]
    per_task = max(len(views) // tasks, 1)
    if generic:
        monkeypatch.setenv("DVSR_DEGRADE_GENERIC", "1")
    for quantise in (1, 0):
        run_degrade(views, fmt, ps, H, W, ds, kernels, scale, lambda i: i // per_task, flags_of, quantise)


def gather_sources(kind, H, W):
    """8 crops of H x W out of frames a little larger, as `kind` stores them."""
    if kind == "f32":
        base = torch.rand(8, 3, H + 5, W + 7, generator=torch.Generator().manual_seed(6)).to(DEV)
        return [base[f, :, 2:2 + H, 3:3 + W] for f in range(8)], L.FRAME_F32_CHW, 1
    c = 4 if kind == "rgb4" else 3
    v = byte_video(7, 8, H + 5, W + 7, c).to(DEV)
    return [v[f, 2:2 + H, 3:3 + W] for f in range(8)], (L.FRAME_U8_HWC_BGR if kind == "bgr" else L.FRAME_U8_HWC_RGB), c


@pytest.mark.parametrize("kind", ["rgb", "bgr", "rgb4", "f32"])
@pytest.mark.parametrize("H,W,n_flags", [(64, 64, 8), (37, 41, 4)])
def test_task_gather_is_ingest_flipped(kind, H, W, n_flags):
    """frames.ingest(view, multiple=1) flipped, bit for bit, for bytes (RGB, BGR, stride 4) and fp32: all eight flag values at
    64 x 64, the four without transpose at 37 x 41; every element of dst is written (it starts as NaN)."""
    views, fmt, ps = gather_sources(kind, H, W)
    host, dev = table_of(views, fmt, lambda i: 0, lambda i: i % n_flags)
    dst = torch.full((len(views), 3, H, W), float("nan"), device=DEV)
    L.check(L.lib().dvsr_task_gather(host, dev.data_ptr(), len(views), fmt, ps, H, W, dst.data_ptr(), L.stream()), "dvsr_task_gather")
    torch.cuda.synchronize()
    assert not torch.isnan(dst).any()
    for i, v in enumerate(views):
        assert torch.equal(dst[i], R.flip_t(ingested(v, fmt), i % n_flags)), (i, i % n_flags)


def small_pool():
    return T.FramePool({"000": R.sequence_bytes("000", 12), "001": R.sequence_bytes("001", 12)})


def loop_over_todays_entries(pool, picks, draws, kernels, scale):
    """The per-task loop that make_batch replaces: frames.degrade, Degradation.apply, frames.ingest, torch.flip."""
    gt, lqs, slq = [], [], []
    for (key, fr), d, k in zip(picks, draws, kernels):
        deg, fl = R.FixedKernel(k.numpy(), scale), R.flags_of(d)
        hr = [pool.view(key, f, d["py"], d["px"], d["crop"]) for f in fr]
        lr0 = torch.stack([frames.degrade(v, deg, pool.layout, quantise=True) for v in hr])
        gt.append(R.flip_t(torch.stack([frames.ingest(v, pool.layout, multiple=1).contiguous() for v in hr]), fl))
        lqs.append(R.flip_t(lr0, fl))
        slq.append(R.flip_t(deg.apply(lr0, quantise=False), fl))
    return {"GT": torch.stack(gt), "LQs": torch.stack(lqs), "SuperLQs": torch.stack(slq)}


@pytest.mark.parametrize("scale", [4, 2])
def test_make_batch_is_the_per_task_loop(scale):
    pool = small_pool()
    picks = [("000", [0, 2, 4, 6, 8]), ("001", [11, 10, 9, 8, 7]), ("000", [3, 4, 5, 6, 7])]
    draws = [dict(py=3, px=8, sigma_x=2.0, sigma_y=0.8, theta=0.4, hflip=True, vflip=False, rot=False, crop=64),
             dict(py=0, px=32, sigma_x=0.3, sigma_y=4.1, theta=-1.7, hflip=False, vflip=True, rot=True, crop=64),
             dict(py=8, px=0, sigma_x=4.9, sigma_y=3.3, theta=2.9, hflip=True, vflip=True, rot=False, crop=64)]
    out = T.make_batch(pool, picks, draws, 21, scale)
    h = 64 // scale
    assert tuple(out["GT"].shape) == (3, 5, 3, 64, 64) and tuple(out["LQs"].shape) == (3, 5, 3, h, h)
    assert tuple(out["SuperLQs"].shape) == (3, 5, 3, h // scale, h // scale) and out["draws"] == draws
    want = loop_over_todays_entries(pool, picks, draws, out["kernels"], scale)
    for k in ("GT", "LQs", "SuperLQs"):
        assert torch.equal(out[k], want[k]), k
    filled = {k: torch.full_like(v, float("nan")) for k, v in want.items()}
    again = T.make_batch(pool, picks, draws, 21, scale, out=filled)
    assert all(again[k] is filled[k] and torch.equal(filled[k], want[k]) for k in want)


def test_recorded_reference_tasks():
    """The five tasks that the reference's own __getitem__ returned: GT equal; LQs at the recorded 8-bit level wherever the
    recorded unquantised LR is outside the tie band; SuperLQs within 2e-6 of the CPU oracle applied to the device's own LQs, and
    within 2e-6 + (what the LQs differences at ties can do through |the shifted kernel|) of the recorded one, per pixel."""
    from oracle import degradation as od
    meta, z = R.load_reference()
    pool = T.FramePool({t["name"]: z[t["name"] + "_src"] for t in meta["tasks"]})
    for scale in (4, 2):
        group = [t for t in meta["tasks"] if t["scale"] == scale]
        draws = [dict(t["draw"], crop=64) for t in group]
        out = T.make_batch(pool, [(t["name"], list(range(5))) for t in group], draws, 21, scale)
        torch.cuda.synchronize()
        for b, t in enumerate(group):
            n, fl = t["name"], R.flags_of(t["draw"])
            assert torch.equal(out["GT"][b].cpu(), torch.from_numpy(z[n + "_gt"]).float() / 255.0), n
            lqs = out["LQs"][b].cpu().numpy()
            mask = R.flip_np(R.outside_tie_band(z[n + "_lr_unq"]), fl)
            lv_dev, lv_rec = np.rint(lqs.astype(np.float64) * 255), np.rint(z[n + "_lqs"].astype(np.float64) * 255)
            ties = int((lv_dev != lv_rec).sum())
            print("%s: %d of %d LQs values differ from the recorded level, all inside the tie band: %s" % (
                n, ties, lqs.size, bool((lv_dev == lv_rec)[mask].all())))
            assert (lv_dev == lv_rec)[mask].all(), n
            assert np.abs(lv_dev - lv_rec).max() <= 1
            slq = out["SuperLQs"][b].cpu().numpy().astype(np.float64)
            kernel = z[n + "_kernel"]
            lr0, lr0_rec = R.flip_np(lqs, fl), R.flip_np(z[n + "_lqs"], fl)          # the flips are their own inverses (no rot)
            oracle = R.flip_np(od.apply(lr0, kernel, scale), fl)
            err = float(np.abs(slq - oracle).max())
            bound = 2e-6 + R.flip_np(R.correlate_abs(np.abs(lr0.astype(np.float64) - lr0_rec), kernel, scale), fl)
            dev_rec = np.abs(slq - z[n + "_slq"])
            print("%s: SuperLQs max |device - oracle(device LQs)| %.3e; max |device - recorded| %.3e" % (n, err, float(dev_rec.max())))
            assert err <= 2e-6, n
            assert (dev_rec <= bound).all(), n


def _source_opt(batch_size=2):
    return {"scale": 4, "datasets": {"train": {"N_frames": 5, "interval_list": [1, 2, -1], "patch_size": 32, "kernel_size": 21,
                                               "batch_size": batch_size}}}


def test_task_source_end_to_end():
    """A TaskSource over two 12-frame 72 x 96 sequences, patch_size 32, B = 2, iterated twice: the same batches for the same
    seed, other crops for another seed, disjoint rank shards, and its first batch through one meta_train_step."""
    from dynavsr_amd import synth
    from dynavsr_amd.adapt import meta_train_step
    from dynavsr_amd.models import create_model
    from dynavsr_amd.options import options as option
    pool = small_pool()
    assert pool.nbytes == 2 * 12 * 72 * 96 * 3 and pool.lengths == {"000": 12, "001": 12}
    a, b, c = (T.TaskSource(_source_opt(), pool, seed=s) for s in (3, 3, 4))
    first = None
    for epoch in range(2):
        ba, bb, bc = list(a), list(b), list(c)
        assert len(ba) == len(a) == len(bb) == a.index.n_samples // 2 and len(ba) >= 4
        for x, y in zip(ba, bb):
            assert x["indices"] == y["indices"] and x["draws"] == y["draws"]
            assert all(torch.equal(x[k], y[k]) for k in ("GT", "LQs", "SuperLQs"))
            assert tuple(x["GT"].shape) == (2, 5, 3, 64, 64) and tuple(x["LQs"].shape) == (2, 5, 3, 16, 16)
            assert tuple(x["SuperLQs"].shape) == (2, 5, 3, 4, 4)
        assert [(d["py"], d["px"]) for x in ba for d in x["draws"]] != [(d["py"], d["px"]) for x in bc for d in x["draws"]]
        seen = [i for x in ba for i in x["indices"]]
        assert len(set(seen)) == len(seen)                                            # a permutation: no sample twice
        first = first or ba[0]
    assert [x["indices"] for x in ba] != [x["indices"] for x in list(T.TaskSource(_source_opt(), pool, seed=3))]   # a new epoch
    r0, r1 = (T.TaskSource(_source_opt(4), pool, seed=3, rank=r, world=2) for r in (0, 1))
    i0, i1 = ([i for x in s for i in x["indices"]] for s in (r0, r1))
    assert len(i0) == len(i1) > 0 and not set(i0) & set(i1) and r0.batch_size == 2
    still = T.TaskSource(_source_opt(), pool, seed=3, train=False)
    assert all(not (d["hflip"] or d["vflip"]) for x in still for d in x["draws"])

    opt = option.dict_to_nonedict(option.parse(os.path.join(ROOT, "dynavsr_amd", "options", "test", "EDVR", "EDVR_M_S4.yml"),
                                               is_train=False))
    opt["dist"] = False
    for k in ("pretrain_model_G", "pretrain_model_E"):
        opt["path"][k] = None
    opt["train"]["maml"]["adapt_iter"] = 1
    model, est = create_model(opt)
    modelcp, estcp = create_model(opt)
    model.netG.load_state_dict(synth.edvr_state_dict(0)); est.netE.load_state_dict(synth.mfdn_state_dict(0))
    params = [p for p in model.netG.parameters() if p.requires_grad] + [p for p in est.netE.parameters() if p.requires_grad]
    r = meta_train_step(opt, model, est, modelcp, estcp, first, torch.optim.SGD(params, lr=1e-4))
    losses = [float(r["loss_q"])] + [float(v) for v in r["loss_train"]] + [float(v) for v in r["loss_e"]]
    assert losses and all(np.isfinite(v) for v in losses), losses
