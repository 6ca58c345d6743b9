"""GPU: adapt.adapt_frames -- test-time adaptation of a decoded video at any frame size -- and the `region` / `baseline`
arguments of adapt_frame / adapt_video behind it.  EDVR-M x4 + MFDN with synthetic weights, T = 7 frames, nframes 5; every
result is pinned to an existing statement at the bar an existing test holds for it."""
import os
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, relerr
from dynavsr_amd import synth

pytestmark = pytest.mark.gpu
T = 7


def _opt(optimizer="Adam"):
    from dynavsr_amd.options import options as option
    opt = option.dict_to_nonedict(option.parse(os.path.join(
        ROOT, "dynavsr_amd", "options", "test", "EDVR", "EDVR_M_S4.yml"), is_train=False))
    opt["dist"] = False
    for k in ("pretrain_model_G", "pretrain_model_E"):
        opt["path"][k] = None
    opt["train"]["maml"]["optimizer"] = optimizer
    return opt


def _nets(opt):
    """(model, est, modelcp, estcp, est_fixed): the five wrappers of the test driver, synthetic weights."""
    from dynavsr_amd.models import create_model
    model, est = create_model(opt)
    modelcp, estcp = create_model(opt)
    _, est_fixed = create_model(opt)
    model.netG.load_state_dict(synth.edvr_state_dict(0)); est.netE.load_state_dict(synth.mfdn_state_dict(0))
    est_fixed.netE.load_state_dict(synth.mfdn_state_dict(1))
    return model, est, modelcp, estcp, est_fixed


def _u8_video(seed, h=30, w=44):
    """uint8 [T,h,w,3] RGB frames on the CPU, as a decoder delivers them."""
    return (synth.clip(seed, 1, T, h, w)[0] * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _padded_clips(frames, layout, windows):
    from dynavsr_amd import frames as fio
    ing = [fio.ingest(f, layout, 16, "reflect") for f in frames]
    return [torch.stack([ing[j] for j in win])[None] for win in windows]


def _baseline(model, clip):
    model.feed_data({"LQs": clip}, need_GT=False)
    model.test()
    return model.fake_H


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("frames_per_batch", [1, 2])
def test_multiple_of_16_frames_are_adapt_video_over_the_windows(overlap, frames_per_batch):
    """Float [3,32,48] frames need no padding: the pairs are adapt_video's over the hand-built clips of video_windows -- the
    baselines bit for bit (forward only), the adapted frames at the bar of test_adapt_video_overlap_equals_sequential_loop
    (1e-5; the batched step at its own bars: sr 1e-4, loss 2e-6), `losses` rows the result dicts' losses."""
    from dynavsr_amd.adapt import adapt_frames, adapt_video, video_windows
    opt = _opt()
    nets = _nets(opt)
    frames = synth.clip(100, 1, T, 32, 48)[0].cuda()
    windows, _ = video_windows(T, 5, "new_info")
    clips = [{"LQs": frames[win][None].contiguous()} for win in windows]
    want = [(b.clone(), r["sr"].clone(), torch.stack([l.reshape(()) for l in r["losses"]]).clone())
            for b, r in adapt_video(opt, *nets, clips, overlap=overlap, frames_per_batch=frames_per_batch)]
    losses = torch.full((T, 1), float("nan"), device="cuda")
    got = [(b.clone(), a.clone()) for b, a in adapt_frames(opt, *nets, frames, out="float", losses=losses, overlap=overlap,
                                                           frames_per_batch=frames_per_batch)]
    assert len(got) == len(want) == T
    bar = 1e-5 if frames_per_batch == 1 else 1e-4
    for i, ((b, a), (wb, wa, wl)) in enumerate(zip(got, want)):
        print(i, relerr(a, wa), float((losses[i] - wl).abs().max() / wl.abs().max()))
        assert tuple(a.shape) == (1, 3, 128, 192)
        assert torch.equal(b, wb)
        assert relerr(a, wa) < bar
        assert float((losses[i] - wl).abs().max()) <= 2e-6 * float(wl.abs().max())


def test_region_step_against_the_oracle():
    """One inner SGD step on a 30 x 44 clip reflect-padded to 32 x 48, adapt_frame(region=(30, 44)), against the functional
    oracle built as in test_inner_step_x2_sfdn_image_mode_vs_oracle with its two means over [:30, :44] and [:8, :11] -- at that
    test's bars (SLR 1e-5, loss 2e-5, adapted SR 2e-4).  And region=(32, 48), the whole clip, is region=None (two-run bar)."""
    from dynavsr_amd.adapt import adapt_frame
    from oracle import edvr as oedvr, mfdn as omfdn
    opt = _opt("SGD")
    model, est, modelcp, estcp, est_fixed = _nets(opt)
    PG, PE, PEF = synth.edvr_state_dict(0), synth.mfdn_state_dict(0), synth.mfdn_state_dict(1)
    lqs = F.pad(synth.clip(3, 1, 5, 30, 44)[0], (0, 4, 0, 2), mode="reflect")[None]          # [1,5,3,32,48]
    lr = opt["train"]["maml"]["lr_alpha"]
    r = adapt_frame(opt, model, est, modelcp, estcp, est_fixed, {"LQs": lqs.cuda()}, region=(30, 44))
    got = (r["slr"].clone(), float(r["losses"][0]), r["sr"].clone())
    OG = OrderedDict((k, v.clone().requires_grad_(True)) for k, v in PG.items())
    OE = OrderedDict((k, v.clone().requires_grad_(True)) for k, v in PE.items())
    slr = omfdn.mfdn_forward(OE, lqs)                                                      # [1,5,3,8,12]
    with torch.no_grad():
        slr_fixed = omfdn.mfdn_forward(PEF, lqs)
    loss = oedvr.charbonnier(oedvr.edvr_forward(OG, slr)[..., :30, :44], lqs[:, 2][..., :30, :44]) \
        + 10 * F.l1_loss(slr[..., :8, :11], slr_fixed[..., :8, :11])
    grads = torch.autograd.grad(loss, list(OG.values()) + list(OE.values()))
    with torch.no_grad():
        for p, g in zip(list(OG.values()) + list(OE.values()), grads):
            p -= lr * g
        sro = oedvr.edvr_forward(OG, lqs)
    want = float(loss.detach())
    print("slr %.3e loss %.3e sr %.3e" % (relerr(got[0], slr), abs(got[1] - want) / abs(want), relerr(got[2], sro)))
    assert tuple(got[2].shape) == (1, 3, 128, 192)                                         # the whole padded frame
    assert relerr(got[0], slr) < 1e-5
    assert abs(got[1] - want) < 2e-5 * abs(want)
    assert relerr(got[2], sro) < 2e-4
    whole = adapt_frame(opt, model, est, modelcp, estcp, est_fixed, {"LQs": lqs.cuda()})
    w_sr, w_loss = whole["sr"].clone(), float(whole["losses"][0])
    print("loss over the region %.8f, over the whole padded clip %.8f" % (got[1], w_loss))
    same = adapt_frame(opt, model, est, modelcp, estcp, est_fixed, {"LQs": lqs.cuda()}, region=(32, 48))
    assert abs(float(same["losses"][0]) - w_loss) <= 1e-5 * abs(w_loss)
    assert relerr(same["sr"], w_sr) < 1e-5


def test_any_size_decoder_formats():
    """uint8 HWC RGB frames of 30 x 44 from the CPU: the baselines are byte-equal to frames.emit of the model's forward on the
    ingested, padded clip (forward only: bit-identical); the adapted frames are the hand-built ingest -> adapt_frame(region) ->
    crop at the two-run bar; out=None gives uint8 [120,176,3].  The baselines check again for NV12 frames (packed [180,176] out)
    and for out_size=(90, 132)."""
    from dynavsr_amd import frames as fio
    from dynavsr_amd.adapt import adapt_frame, adapt_frames, video_windows
    opt = _opt()
    nets = _nets(opt)
    model = nets[0]
    video = _u8_video(5)
    windows, _ = video_windows(T, 5, "new_info")
    clips = _padded_clips(video, "hwc_rgb", windows)
    assert tuple(clips[0].shape) == (1, 5, 3, 32, 48)
    base = [_baseline(model, c).clone() for c in clips]
    want_u8 = [fio.emit(b, 120, 176, "hwc_rgb") for b in base]
    want_ad = [adapt_frame(opt, *nets, {"LQs": c}, region=(30, 44))["sr"][..., :120, :176].clone() for c in clips]
    got = [(b.clone(), a.clone()) for b, a in adapt_frames(opt, *nets, video, out="float")]
    assert len(got) == T
    for i, (b, a) in enumerate(got):
        print(i, relerr(a, want_ad[i]))
        assert tuple(b.shape) == tuple(a.shape) == (1, 3, 120, 176)
        assert torch.equal(b, base[i][..., :120, :176])
        assert relerr(a, want_ad[i]) < 1e-5
    got = [(b.clone(), a.clone()) for b, a in adapt_frames(opt, *nets, video)]
    for i, (b, a) in enumerate(got):
        assert b.dtype == a.dtype == torch.uint8 and tuple(b.shape) == tuple(a.shape) == (120, 176, 3) and a.is_cuda
        assert torch.equal(b, want_u8[i])
    small = [fio.emit(b, 120, 176, "hwc_rgb", size=(90, 132)) for b in base]
    for i, (b, a) in enumerate(adapt_frames(opt, *nets, video, out_size=(90, 132))):
        assert tuple(a.shape) == (90, 132, 3) and a.dtype == torch.uint8
        assert torch.equal(b, small[i])
    g = torch.Generator().manual_seed(9)
    nv12 = torch.randint(16, 236, (T, 45, 44), dtype=torch.uint8, generator=g)            # 30 x 44: 30 rows Y, 15 rows CbCr
    clips = _padded_clips(nv12, "nv12", windows)
    want = [fio.emit(_baseline(model, c), 120, 176, "nv12") for c in clips]
    for i, (b, a) in enumerate(adapt_frames(opt, *nets, nv12, layout="nv12")):
        assert tuple(b.shape) == tuple(a.shape) == (180, 176) and a.dtype == torch.uint8
        assert torch.equal(b, want[i])


@pytest.mark.parametrize("overlap", [False, True])
def test_batched_step_with_a_region_and_no_baseline_in_both_loops(overlap):
    """Padded frames with frames_per_batch=2: FrameBatch.adapt's region branch (the per-sample region losses) against the
    per-frame adapt_frame(region=(30, 44)) on the hand-built clips, at the bars of test_adapt_video_batched_at_the_north_star_size
    (baseline 5e-6: a two-clip forward may take other kernel kinds; loss 2e-6; adapted frame 1e-4).  baseline=False in the batched
    loop and in the per-frame loop (with and without overlap): None baselines, the adapted frames of the baseline=True run at the
    two-run bars, and the un-adapted network never runs at full size."""
    from dynavsr_amd.adapt import adapt_frame, adapt_frames, video_windows
    opt = _opt()
    nets = _nets(opt)
    model = nets[0]
    video = _u8_video(5)
    windows, _ = video_windows(T, 5, "new_info")
    clips = _padded_clips(video, "hwc_rgb", windows)
    want = []
    for c in clips:
        base = _baseline(model, c)[..., :120, :176].clone()
        r = adapt_frame(opt, *nets, {"LQs": c}, region=(30, 44))
        want.append((base, r["sr"][..., :120, :176].clone(), float(r["losses"][0])))
    losses = torch.full((T, 1), float("nan"), device="cuda")
    got = [(b.clone(), a.clone()) for b, a in adapt_frames(opt, *nets, video, out="float", losses=losses, overlap=overlap,
                                                           frames_per_batch=2)]
    assert len(got) == T
    for i, ((b, a), (wb, wa, wl)) in enumerate(zip(got, want)):
        print(i, relerr(b, wb), relerr(a, wa), abs(float(losses[i, 0]) - wl) / abs(wl))
        assert relerr(b, wb) < 5e-6
        assert abs(float(losses[i, 0]) - wl) <= 2e-6 * abs(wl)
        assert relerr(a, wa) < 1e-4
    full = []                                       # forwards of the un-adapted network on whole padded clips
    hook = model.netG.register_forward_pre_hook(
        lambda mod, args: full.append(1) if mod is model.netG and tuple(args[0].shape[-2:]) == (32, 48) else None)
    for k, bar in ((2, 1e-4), (1, 1e-5)):
        none = [(b, a.clone()) for b, a in adapt_frames(opt, *nets, video, out="float", overlap=overlap, frames_per_batch=k,
                                                        baseline=False)]
        assert len(none) == T and all(b is None for b, _ in none)
        for (_, a), (_, wa, _) in zip(none, want):
            assert relerr(a, wa) < bar
    hook.remove()
    assert full == []


def test_scenes_scores_and_no_baseline():
    """cuts=[3]: the two scenes come out as two separate calls give them (bars of the first test).  gt: the rows of
    `baseline_scores` / `scores` are frames.score of the yielded frames.  baseline=False: None baselines, the adapted frames of
    the baseline=True run (two-run bar), and the un-adapted network never runs at full size."""
    from dynavsr_amd import frames as fio
    from dynavsr_amd.adapt import adapt_frames, video_windows
    opt = _opt()
    nets = _nets(opt)
    model = nets[0]
    video = _u8_video(6)
    windows, scenes = video_windows(T, 5, "new_info", [3])
    assert scenes == 2 and all((max(win) < 3) == (c < 3) and (min(win) >= 3) == (c >= 3) for c, win in enumerate(windows))
    full = []                                       # forwards of the un-adapted network on a whole padded clip
    hook = model.netG.register_forward_pre_hook(
        lambda mod, args: full.append(1) if mod is model.netG and tuple(args[0].shape[-2:]) == (32, 48) else None)
    got = [(b.clone(), a.clone()) for b, a in adapt_frames(opt, *nets, video, out="float", cuts=[3])]
    assert len(full) == T
    parts = [(b.clone(), a.clone()) for b, a in adapt_frames(opt, *nets, video[:3], out="float", cuts=[])] + \
            [(b.clone(), a.clone()) for b, a in adapt_frames(opt, *nets, video[3:], out="float", cuts=[])]
    assert len(got) == len(parts) == T
    for (b, a), (wb, wa) in zip(got, parts):
        assert torch.equal(b, wb)
        assert relerr(a, wa) < 1e-5
    del full[:]
    none = [(b, a.clone()) for b, a in adapt_frames(opt, *nets, video, out="float", cuts=[3], baseline=False)]
    hook.remove()
    assert len(none) == T and all(b is None for b, _ in none)
    assert full == []
    for (_, a), (_, wa) in zip(none, got):
        assert relerr(a, wa) < 1e-5
    g = torch.Generator().manual_seed(11)
    gt = torch.randint(0, 256, (T, 120, 176, 3), dtype=torch.uint8, generator=g)
    scores = torch.full((T, 2), float("nan"), dtype=torch.float64, device="cuda")
    bscores = torch.full((T, 2), float("nan"), dtype=torch.float64, device="cuda")
    pairs = [(b.clone(), a.clone()) for b, a in adapt_frames(opt, *nets, video, cuts=[3], gt=gt, scores=scores,
                                                             baseline_scores=bscores)]
    for i, (b, a) in enumerate(pairs):
        assert torch.equal(bscores[i], fio.score(b, gt[i], "hwc_rgb", "hwc_rgb"))
        assert torch.equal(scores[i], fio.score(a, gt[i], "hwc_rgb", "hwc_rgb"))
    assert not torch.isnan(scores).any() and not torch.isnan(bscores).any()
    only = torch.full((T, 2), float("nan"), dtype=torch.float64, device="cuda")
    for _ in adapt_frames(opt, *nets, video, cuts=[3], gt=gt, scores=only, baseline=False):
        pass
    # the 8-bit images of frames 1e-5 apart: a value in [0, 1] moves by 1e-5 at most, so 2 * 255 * 1e-5 = 0.5 % of the pixels can
    # round to the neighbouring level, each changing its squared error by at most 2 * 255 + 1 -- 2.6 in the MSE, against an MSE
    # of ~1e4 to a random ground truth: 2.6e-4 of it
    assert float((only[:, 0] - scores[:, 0]).abs().max()) <= 1e-3 * float(scores[:, 0].min())


def test_use_patch_draws_inside_the_region(monkeypatch):
    """train.maml.use_patch: the patches are drawn over the SLR cells that hold real pixels alone, floor(h / s) x floor(w / s),
    so with origins p and a crop of ps cells s (p + ps) <= (h, w) and the pixel loss needs no mask.
    The crop's edge is ps = patch_size // 2 (the reference's `crop`) and EDVR takes multiples of 4, so patch_size 4 -- an edge
    of 2 -- cannot run on this backbone: with a region it is a ValueError that says so, region=(8, 8) included.  patch_size 8
    would give 4 x 4 patches, which fit the 7 x 11 cells of a 30 x 44 frame, but no test of the suite has run EDVR's training
    tape (forward with a graph + backward) at 4 x 4, where the L3 level is one pixel; a first run of it belongs in a test of
    that tape, not here.  The smallest patch whose training tape the suite covers is 8 x 8 (patch_size 16,
    test_use_patch_crop_and_inner_step).  It needs floor(h / 4) >= 8, so the frames are 38 x 44 (9 x 11 whole cells of the
    12 x 12 SLR clip), and the 30 x 44 frames (7 x 11 cells) are a ValueError, like region=(8, 8)."""
    from dynavsr_amd import adapt
    opt = _opt()
    opt["train"]["maml"].update({"use_patch": True, "num_patch": 2, "patch_size": 16})
    nets = _nets(opt)
    drawn = []
    real = adapt.draw_patch_positions

    def recording(min_h, min_w, ps, n):
        py, px = real(min_h, min_w, ps, n)
        drawn.append((min_h, min_w, ps, list(py), list(px)))
        return py, px
    monkeypatch.setattr(adapt, "draw_patch_positions", recording)
    h, w, s = 38, 44, 4
    losses = torch.full((T, 1), float("nan"), device="cuda")
    out = [a.clone() for _, a in adapt.adapt_frames(opt, *nets, _u8_video(7, h, w), losses=losses)]
    assert len(out) == T and all(tuple(a.shape) == (s * h, s * w, 3) for a in out)
    assert torch.isfinite(losses).all()
    assert len(drawn) == T
    for min_h, min_w, ps, py, px in drawn:
        assert (min_h, min_w, ps) == (h // s, w // s, 8) and len(py) == len(px) == 2
        assert all(s * (p + ps) <= h for p in py) and all(s * (p + ps) <= w for p in px)
    with pytest.raises(ValueError, match="patch"):
        next(adapt.adapt_frames(opt, *nets, _u8_video(7)))                                  # 30 x 44: 7 x 11 whole cells
    for patch_size in (4, 8, 16):                       # 4: an edge of 2, which EDVR does not take; 8, 16: 2 x 2 cells hold no patch
        opt["train"]["maml"]["patch_size"] = patch_size
        with pytest.raises(ValueError, match="patch"):
            adapt.adapt_frame(opt, *nets, {"LQs": synth.clip(8, 1, 5, 16, 16).cuda()}, region=(8, 8))
    assert len(drawn) == T
