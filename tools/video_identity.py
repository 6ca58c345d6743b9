#!/usr/bin/env python
"""A record of what the video path computes, line by line, to compare two checkouts of this repository.

    python tools/video_identity.py --tree PATH [--dump FILE] [--only SUBSTRING]      (GPU)
    python tools/video_identity.py --tree PATH --errors                              (no GPU)

--tree is the checkout whose dynavsr_amd is imported (default: this one), so the same script runs against an older commit's
checkout.  Only names that exist as adapt.* are used.  With a fixed seed and synth.edvr_state_dict(0) every case of the matrix
below runs twice -- the first run warms plans and buffers -- and prints, from the second run: the sha256 of every yielded
frame's bytes, the rows of `scores` as hex floats, the deltas of the stream plans' stats and the number of allocations
(torch.cuda.memory_stats()['allocation.all.allocated']).  Every launch on these paths is deterministic, so two checkouts that
compute the same thing print the same lines.  The adapted frames and losses of adapt_frames pass through backward kernels that
sum with atomics and are not reproducible bit for bit: they are written as fp32 to --dump (torch.save of {name: tensor}) and
compared by compare_dumps() / --compare.

    python tools/video_identity.py --compare NEW.pt PARENT1.pt PARENT2.pt PARENT3.pt

--errors: a list of bad calls of super_resolve_frames, adapt_frames, tile_footprint, choose_tile, tile_origins, score_summary
and evaluate_frames, each with arguments chosen so that exactly one check fires, the networks on the CPU so that a check
that moved behind a GPU call shows as another exception; prints the exception's type and text."""
import argparse
import hashlib
import itertools
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ap.add_argument("--errors", action="store_true")
ap.add_argument("--dump", default=None)
ap.add_argument("--only", default=None)
ap.add_argument("--compare", nargs="+", default=None)
args = ap.parse_args()
TREE = os.path.abspath(args.tree)
sys.path.insert(0, TREE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

T = 7
OPT = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}
DUF = {'scale': 1, 'network_G': {'which_model_G': 'DUF', 'nframes': 3}}
TILE, OVERLAP = (16, 20), 8                      # tests/test_gpu_stitch.py: 3 x 3 tiles of a 30 x 34 frame


class Mean(torch.nn.Module):                     # the two networks of tests/test_gpu_stitch.py
    nframes = 3

    def forward(self, x):
        return x.mean(1)


class Ramp(torch.nn.Module):
    """Not shift-equivariant: adds a ramp along x and y, so a tile's output depends on where the tile starts."""
    nframes = 3

    def forward(self, x):
        rx = torch.arange(x.shape[-1], dtype=torch.float32, device=x.device) * 0.03125
        ry = torch.arange(x.shape[-2], dtype=torch.float32, device=x.device)[:, None] * 0.0078125
        return x.mean(1) * 0.5 + rx + ry


def compare_dumps(paths):
    """paths[0] is the new tree's dump, the others the parent's: per entry, the whole video as one vector, the relative L2
    distance of every parent pair (largest: parent~parent) and of the new dump to every parent (largest: new~parent)."""
    dumps = [torch.load(p) for p in paths]

    def rel(a, b):
        a, b = a.double().flatten(), b.double().flatten()
        return float((a - b).norm() / b.norm())
    ok = True
    for name in sorted(dumps[0]):
        pp = max([rel(a[name], b[name]) for a, b in itertools.combinations(dumps[1:], 2)] or [float('nan')])
        npar = max(rel(dumps[0][name], d[name]) for d in dumps[1:])
        good = npar <= 2 * pp
        ok = ok and good
        print("%-44s parent~parent %.3e   new~parent %.3e   ratio %.2f   %s" % (name, pp, npar, npar / pp if pp else float('inf'),
                                                                              "ok" if good else "OUTSIDE 2x"))
    return ok


if args.compare:
    sys.exit(0 if compare_dumps(args.compare) else 1)

import dynavsr_amd  # noqa: E402
assert os.path.abspath(os.path.dirname(dynavsr_amd.__file__)) == os.path.join(TREE, "dynavsr_amd"), dynavsr_amd.__file__
from dynavsr_amd import adapt, engine, synth  # noqa: E402
from dynavsr_amd import frames as fio  # noqa: E402
from dynavsr_amd.models.archs.EDVR_arch import EDVR  # noqa: E402


def adapt_opt():
    from dynavsr_amd.options import options as option
    opt = option.dict_to_nonedict(option.parse(os.path.join(TREE, "dynavsr_amd", "options", "test", "EDVR", "EDVR_M_S4.yml"),
                                               is_train=False))
    opt["dist"] = False
    for k in ("pretrain_model_G", "pretrain_model_E"):
        opt["path"][k] = None
    return opt


def edvr():
    net = EDVR()
    net.load_state_dict(synth.edvr_state_dict(0), strict=True)
    return net


def u8_video(seed, t, h, w):
    return (synth.clip(seed, 1, t, h, w)[0] * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


# ---- --errors -------------------------------------------------------------------------------------------------------
def errors():
    net, mean = edvr(), Mean()
    f32 = torch.zeros((T, 3, 32, 48))
    u8 = torch.zeros((T, 13, 15, 3), dtype=torch.uint8)
    u8t = torch.zeros((T, 30, 34, 3), dtype=torch.uint8)
    gt = torch.zeros((T, 52, 60, 3), dtype=torch.uint8)
    cpu_scores = torch.zeros((T, 2), dtype=torch.float64)
    aopt = adapt_opt()
    real, noframes, patch = adapt_opt(), adapt_opt(), adapt_opt()
    real["train"]["use_real"] = True
    noframes["network_G"]["nframes"] = None
    patch["train"]["maml"].update({"use_patch": True, "num_patch": 2, "patch_size": 8})
    a44 = torch.zeros((T, 30, 44, 3), dtype=torch.uint8)
    agt = torch.zeros((T, 120, 176, 3), dtype=torch.uint8)

    def srf(net_, frames, opt=OPT, **kw):
        return lambda: next(adapt.super_resolve_frames(opt, net_, frames, **kw))

    def adf(frames, opt=aopt, **kw):
        return lambda: next(adapt.adapt_frames(opt, None, None, None, None, None, frames, **kw))
    calls = [
        # super_resolve_frames, in the order of its checks
        ("srf no frames", srf(net, [])),
        ("srf flip_test", srf(net, f32, flip_test=1)),
        ("srf pad_mode", srf(net, f32, pad_mode='zeros')),
        ("srf out_size pair", srf(net, f32, out_size=(40,))),
        ("srf tile_overlap", srf(net, u8t, tile=TILE, tile_overlap=6)),
        ("srf tile_budget without auto", srf(net, u8t, tile=TILE, tile_budget=1e9)),
        ("srf tile_budget sign", srf(net, u8t, tile='auto', tile_budget=-1)),
        ("srf tile name", srf(net, u8t, tile='big')),
        ("srf tile triple", srf(net, u8t, tile=(16, 20, 24))),
        ("srf tile side", srf(net, u8t, tile=(16, 18), tile_overlap=8)),
        ("srf tile under twice the overlap", srf(net, u8t, tile=(16, 20), tile_overlap=12)),
        ("srf tile auto, not EDVR", srf(mean, u8t, opt=DUF, tile='auto')),
        ("srf layout name", srf(net, u8, layout='rgb24')),
        ("srf layout against dtype", srf(net, f32, layout='hwc_rgb')),
        ("srf frames of two kinds", srf(net, [u8[0], u8[1], f32[0]])),
        ("srf out name", srf(net, u8, out='png')),
        ("srf matrix", srf(net, u8, matrix='bt2020')),
        ("srf yuv_range", srf(net, u8, yuv_range='tv')),
        ("srf out_size ratio", srf(net, u8, out_size=(8, 60))),
        ("srf packed nv12 odd", srf(net, u8, out='nv12', out_size=(41, 47))),
        ("srf packed i422 odd width", srf(net, u8, out='i422', out_size=(40, 47))),
        ("srf frames under 4 x 4", srf(net, torch.zeros((T, 3, 15, 3), dtype=torch.uint8))),
        ("srf multiple", srf(net, u8, multiple=0)),
        ("srf reflect pad", srf(net, torch.zeros((T, 6, 44, 3), dtype=torch.uint8), multiple=16)),
        ("srf scores without gt", srf(net, u8, scores=cpu_scores)),
        ("srf gt length", srf(net, u8, gt=gt[:5], scores=cpu_scores)),
        ("srf gt size", srf(net, u8, gt=torch.zeros((T, 50, 60, 3), dtype=torch.uint8), scores=cpu_scores)),
        ("srf score name", srf(net, u8, gt=gt, score='luma', scores=cpu_scores)),
        ("srf y of a yuv output, bt709", srf(net, u8, out='i444', gt=gt, score='y', matrix='bt709', scores=cpu_scores)),
        ("srf gt needs scores", srf(net, u8, gt=gt)),
        ("srf scores on the CPU", srf(net, u8, gt=gt, scores=cpu_scores)),
        ("srf float frames, scores on the CPU", srf(net, f32, gt=torch.zeros((T, 3, 128, 192)), scores=cpu_scores)),
        ("srf cuts name", srf(net, u8, cuts='scenes')),
        ("srf cuts not a sequence", srf(net, u8, cuts=4)),
        ("srf cuts not ints", srf(net, u8, cuts=[2.0])),
        ("srf cuts outside", srf(net, u8, cuts=[7])),
        ("srf cuts order", srf(net, u8, cuts=[4, 2])),
        ("srf cuts auto, padding", srf(net, u8, cuts='auto', padding='mirror')),
        ("srf tile auto, too few frames", srf(net, u8t[:2], tile='auto', tile_budget=1e9)),
        ("srf tile auto, nothing fits", srf(net, u8t, tile='auto', tile_budget=1)),
        ("srf tile against multiple", srf(net, u8t, tile=(16, 20), tile_overlap=8, multiple=8)),
        ("srf last tile's pad", srf(net, torch.zeros((T, 33, 34, 3), dtype=torch.uint8), multiple=16, tile=16, tile_overlap=0)),
        # behind the resolution: the two paths
        ("srf other network, too few frames", srf(mean, f32[:1], opt=DUF, padding='new_info')),
        ("srf other network, flip_test width", srf(mean, torch.zeros((T, 3, 32, 46)), opt=DUF, flip_test=True)),
        ("srf other network, padded flip_test width", srf(mean, u8, opt=DUF, flip_test=True)),
        ("srf EDVR, too few frames", srf(net, f32[:2])),
        ("srf EDVR, padding", srf(net, f32, padding='mirror')),
        ("srf EDVR, 4 GiB image", srf(net, torch.zeros((1, 3, 1080, 1920)), padding='replicate')),
        ("srf EDVR, 4 GiB image from bytes", srf(net, torch.zeros((1, 1080, 1920, 3), dtype=torch.uint8), padding='replicate')),
        ("srf EDVR on the CPU", srf(net, f32)),
        ("srf EDVR on the CPU, bytes", srf(net, u8)),
        ("srf EDVR on the CPU, tiles", srf(net, u8t, tile=TILE, tile_overlap=OVERLAP)),
        ("srf EDVR on the CPU, wrong planes", srf(net, torch.zeros((T, 1, 32, 48)))),
        # the tile geometry
        ("tile_origins tile", lambda: adapt.tile_origins(36, 10, 8)),
        ("tile_origins overlap", lambda: adapt.tile_origins(36, 16, 12)),
        ("tile_footprint network", lambda: adapt.tile_footprint(mean, 30, 34, TILE)),
        ("tile_footprint auto", lambda: adapt.tile_footprint(net, 30, 34, 'auto')),
        ("tile_footprint overlap", lambda: adapt.tile_footprint(net, 30, 34, TILE, overlap=-4)),
        ("tile_footprint tile", lambda: adapt.tile_footprint(net, 30, 34, (12, 20))),
        ("choose_tile overlap", lambda: adapt.choose_tile(net, 30, 34, 1e9, overlap=True)),
        ("choose_tile nothing fits", lambda: adapt.choose_tile(net, 30, 34, 1)),
        ("choose_tile network", lambda: adapt.choose_tile(mean, 30, 34, 1e9)),
        # the scores
        ("score_summary shape", lambda: adapt.score_summary(torch.zeros((T, 3)), 5)),
        ("score_summary nframes", lambda: adapt.score_summary(torch.zeros((T, 2)), 0)),
        ("score_summary cuts", lambda: adapt.score_summary(torch.zeros((T, 2)), 5, cuts=[9])),
        ("evaluate_frames gt length", lambda: adapt.evaluate_frames(OPT, net, u8, gt[:3], scores=cpu_scores)),
        ("evaluate_frames scores on the CPU", lambda: adapt.evaluate_frames(OPT, net, u8, gt, scores=cpu_scores)),
        ("evaluate_frames out name", lambda: adapt.evaluate_frames(OPT, net, u8, gt, scores=cpu_scores, out='png')),
        # adapt_frames
        ("adf use_real", adf(a44, opt=real)),
        ("adf no frames", adf([])),
        ("adf pad_mode", adf(a44, pad_mode='zeros')),
        ("adf multiple", adf(a44, multiple=8)),
        ("adf out_size pair", adf(a44, out_size=(90,))),
        ("adf layout name", adf(a44, layout='rgb24')),
        ("adf out name", adf(a44, out='png')),
        ("adf out_size ratio", adf(a44, out_size=(20, 176))),
        ("adf packed nv12 odd", adf(a44, out='nv12', out_size=(91, 133))),
        ("adf reflect pad", adf(torch.zeros((T, 6, 44, 3), dtype=torch.uint8))),
        ("adf scores without gt", adf(a44, scores=cpu_scores)),
        ("adf gt needs scores", adf(a44, gt=agt)),
        ("adf baseline_scores, no baseline", adf(a44, baseline=False, baseline_scores=cpu_scores)),
        ("adf baseline_scores without gt", adf(a44, baseline_scores=cpu_scores)),
        ("adf losses shape", adf(a44, losses=torch.zeros((T, 2)))),
        ("adf losses on the CPU", adf(a44, losses=torch.zeros((T, 1)))),
        ("adf nframes", adf(a44, opt=noframes)),
        ("adf patch", adf(torch.zeros((T, 8, 8, 3), dtype=torch.uint8), opt=patch, pad_mode='replicate')),
        ("adf cuts name", adf(a44, cuts='scenes')),
        ("adf cuts outside", adf(a44, cuts=[0])),
        ("adf cuts auto, padding", adf(a44, cuts='auto', padding='mirror')),
        ("adf too few frames", adf(a44[:2])),
    ]
    for name, call in calls:
        try:
            call()
            print("%-44s | no exception" % name)
        except Exception as e:                                    # noqa: BLE001 -- the type is what is recorded
            print("%-44s | %s: %s" % (name, type(e).__name__, " ".join(str(e).split())))
    print("%d calls" % len(calls))


# ---- the matrix -------------------------------------------------------------------------------------------------------
def digest(x):
    if not torch.is_tensor(x):
        return "(" + " ".join(digest(p) for p in x) + ")"
    x = x.detach().contiguous().cpu()
    raw = x.view(torch.uint8).numpy().tobytes() if x.numel() else b""
    return "%s%s:%s" % (str(x.dtype).replace("torch.", ""), list(x.shape), hashlib.sha256(raw).hexdigest()[:32])


def keep(x):
    return x.clone() if torch.is_tensor(x) else tuple(p.clone() for p in x)


def plan_stats():
    return {(p.h, p.w, p.slots): dict(p.stats) for p in engine._splans.values()}


def report(name, run):
    """run() -> (frames, scores or None, further lines); run twice, the second run recorded."""
    if args.only and args.only not in name:
        return None
    run()
    torch.cuda.synchronize()
    before, allocs = plan_stats(), torch.cuda.memory_stats()['allocation.all.allocated']
    frames, scores, more = run()
    allocs = torch.cuda.memory_stats()['allocation.all.allocated'] - allocs
    torch.cuda.synchronize()
    for i, f in enumerate(frames):
        print("%s | frame %d | %s" % (name, i, digest(f)))
    if scores is not None:
        for i, row in enumerate(scores.cpu().tolist()):
            print("%s | scores %d | %s %s" % (name, i, float(row[0]).hex(), float(row[1]).hex()))
    for line in more:
        print("%s | %s" % (name, line))
    for key, stats in sorted(plan_stats().items()):
        was = before.get(key, {})
        delta = {k: stats[k] - was.get(k, 0) for k in ('extracted', 'fused', 'packs')}
        if any(delta.values()):
            print("%s | plan %dx%d/%d | extracted +%d fused +%d packs +%d" % ((name,) + key + tuple(
                delta[k] for k in ('extracted', 'fused', 'packs'))))
    print("%s | allocations | %d" % (name, allocs))
    sys.stdout.flush()
    return frames


def matrix():
    torch.manual_seed(0)
    net = edvr().cuda()
    dev = torch.device('cuda')

    def srf(name, video, opt=OPT, net_=net, gt=None, **kw):
        def run():
            scores = torch.zeros((len(video), 2), dtype=torch.float64, device=dev) if gt is not None else None
            extra = {} if gt is None else {'gt': gt, 'scores': scores}
            return [keep(f) for f in adapt.super_resolve_frames(opt, net_, video, **extra, **kw)], scores, []
        return report(name, run)

    f32 = synth.clip(100, 1, T, 32, 48)[0].cuda()
    for in_flight, padding, out in itertools.product((1, 2), ('new_info', 'replicate'), (None, 'hwc_rgb')):
        srf("float 32x48 in_flight=%d %s out=%s" % (in_flight, padding, out), f32, in_flight=in_flight, padding=padding, out=out)
    u8 = u8_video(13, T, 13, 15)
    for layout, pad_mode, where in itertools.product(('hwc_rgb', 'hwc_bgr'), ('reflect', 'replicate'), ('cpu list', 'gpu tensor')):
        video = list(u8) if where == 'cpu list' else u8.cuda()
        srf("u8 13x15 %s %s %s" % (layout, pad_mode, where), video, layout=layout, pad_mode=pad_mode)
    src = synth.clip(18, 1, T, 18, 22)[0].cuda()
    for layout in ('nv12', 'i420', 'p010'):
        srf("yuv 18x22 %s" % layout, [fio.emit(f[None], 18, 22, layout) for f in src], layout=layout)
    srf("u8 13x15 out=i444p10", u8.cuda(), out='i444p10')
    srf("yuv 18x22 i422 out=nv16", [fio.emit(f[None], 18, 22, 'i422') for f in src], layout='i422', out='nv16')
    for out in ('float', 'hwc_bgr', 'nv12'):
        srf("u8 13x15 out_size=(40,46) out=%s" % out, u8.cuda(), out=out, out_size=(40, 46))
    u9 = torch.cat([u8_video(21, 4, 13, 15), 255 - u8_video(22, 5, 13, 15)]).cuda()       # two scenes, cut at 4
    srf("u8 13x15 T=9 cuts=[4]", u9, cuts=[4])
    srf("u8 13x15 T=9 cuts=auto", u9, cuts='auto')
    srf("u8 13x15 flip_test", u8.cuda(), flip_test=True)
    srf("float 32x48 flip_test", f32, flip_test=True)
    float2 = synth.clip(101, 1, T, 24, 40)[0].cuda()
    srf("float 24x40 out=float in_flight=3", float2, out='float', in_flight=3)
    ut = u8_video(30, T, 30, 34).cuda()
    tiles = dict(tile=TILE, tile_overlap=OVERLAP)
    srf("tiles 30x34", ut, **tiles)
    srf("tiles 30x34 flip_test", ut, flip_test=True, **tiles)
    ut9 = torch.cat([ut[:4], 255 - u8_video(31, 5, 30, 34).cuda()])
    srf("tiles 30x34 T=9 cuts=[4]", ut9, cuts=[4], **tiles)
    gt = u8_video(32, T, 120, 136).cuda()
    scored = srf("tiles 30x34 gt rgb", ut, gt=gt, score='rgb', **tiles)
    gt_nv12 = [fio.emit(f[None], 120, 136, 'nv12') for f in synth.clip(33, 1, T, 120, 136)[0].cuda()]
    srf("tiles 30x34 out=nv12 gt y", ut, out='nv12', gt=gt_nv12, gt_layout='nv12', score='y', **tiles)
    srf("u8 13x15 gt rgb crop_border=2", u8.cuda(), gt=u8_video(34, T, 52, 60).cuda(), crop_border=2)
    rs = np.random.RandomState(12)
    u5 = torch.from_numpy(rs.randint(0, 256, (5, 30, 34, 3)).astype(np.uint8)).cuda()
    f5 = synth.clip(35, 1, 5, 32, 36)[0].cuda()
    for other in (Mean(), Ramp()):
        who, kw = type(other).__name__, dict(opt=DUF, net_=other, padding='replicate')
        srf("%s plain float 32x36" % who, f5, **kw)
        srf("%s plain float 32x36 scored" % who, f5, gt=synth.clip(36, 1, 5, 32, 36)[0].cuda(), **kw)
        srf("%s padded multiple=4" % who, u5, multiple=4, **kw)
        srf("%s padded multiple=4 in_flight=1 out=float" % who, list(u5.cpu()), multiple=4, in_flight=1, out='float', **kw)
        srf("%s tiled" % who, u5, multiple=4, **tiles, **kw)
        srf("%s tiled from the CPU" % who, list(u5.cpu()), multiple=4, out='float', **tiles, **kw)
        srf("%s flip_test" % who, u5, multiple=4, flip_test=True, **kw)
        srf("%s tiled gt out_size" % who, u5, multiple=4, out_size=(40, 46), gt=u8_video(37, 5, 40, 46).cuda(), **tiles, **kw)

    def evaluated():
        summary, scores = adapt.evaluate_frames(OPT, net, ut9, torch.cat([gt, gt[:2]]), cuts='auto', **tiles)
        return [], scores, ["summary | " + repr(summary)]
    report("evaluate_frames tiles 30x34 T=9 cuts=auto", evaluated)

    def closed_early():
        gen = adapt.super_resolve_frames(OPT, net, f32, in_flight=2)
        first = [keep(next(gen)), keep(next(gen))]
        gen.close()
        with torch.no_grad():
            first.append(net(f32[:5][None]).clone())
        return first, None, []
    report("closed after two frames, then net(clip)", closed_early)

    def closed_early_clips():
        gen = adapt.super_resolve_video(OPT, net, (f32[i:i + 5][None] for i in range(3)), in_flight=2)
        first = [keep(next(gen))]
        gen.close()
        with torch.no_grad():
            first.append(net(f32[:5][None]).clone())
        return first, None, []
    report("super_resolve_video closed after one clip, then net(clip)", closed_early_clips)

    # adapt_frames on the decoder-format case of tests/test_gpu_adapt_frames.py
    from dynavsr_amd.models import create_model
    opt = adapt_opt()
    model, est = create_model(opt)
    modelcp, estcp = create_model(opt)
    _, est_fixed = create_model(opt)
    model.netG.load_state_dict(synth.edvr_state_dict(0)); est.netE.load_state_dict(synth.mfdn_state_dict(0))
    est_fixed.netE.load_state_dict(synth.mfdn_state_dict(1))
    nets = (model, est, modelcp, estcp, est_fixed)
    video, agt = u8_video(5, T, 30, 44), u8_video(6, T, 120, 176).cuda()
    dump = {}
    for K in (1, 2):
        name = "adapt_frames u8 30x44 frames_per_batch=%d" % K

        def adapted():
            losses = torch.zeros((T, 1), device=dev)
            scores, bscores = (torch.zeros((T, 2), dtype=torch.float64, device=dev) for _ in range(2))
            pairs = [(keep(b), keep(a)) for b, a in adapt.adapt_frames(
                opt, *nets, video, out='float', baseline=True, losses=losses, gt=agt, scores=scores, baseline_scores=bscores,
                frames_per_batch=K)]
            dump[name + " adapted"] = torch.stack([a for _, a in pairs]).cpu()
            dump[name + " losses"] = losses.cpu()
            return [b for b, _ in pairs], bscores, []
        report(name + " baseline", adapted)
    if args.dump and dump:
        torch.save(dump, args.dump)


if args.errors:
    errors()
else:
    assert torch.cuda.is_available(), "the matrix needs the GPU (--errors does not)"
    matrix()
    print("done")
