"""GPU: frames.score / dvsr_frame_score (csrc/frame_score.hip) against the numpy restatement of score_ref.py, and the gt=
arguments of adapt.super_resolve_frames end to end.

mse is compared EXACTLY (the kernel's 64-bit integer sum against numpy's: a pixel owned by two tiles or by none shows), SSIM at
the project's 8-bit bar of 1e-10 (float64 on both sides, the same separable form).  At depth 10 / 12 the bar is 1e-10 as well
unless the host-only difference between the separable and the 2-D-window form, computed on the CPU in the test for the very
inputs, exceeds 1e-11 -- then ten times that figure; it never depends on the kernel's output.  On the inputs of this file that
host-vs-host figure is at most 2.2e-15 (depth 10 and 12, every size below), so the bar is 1e-10 everywhere."""
import ctypes
import math

import numpy as np
import pytest
import torch

import score_ref as ref
from dynavsr_amd import adapt, frames, synth
from dynavsr_amd import _lib as L
from dynavsr_amd.utils import util

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
# (h, w, crop_border): one valid pixel | no valid region | exactly one tile | one pixel into a second tile on both axes | ragged |
# a crop | a crop that removes the valid region
SIZES = [(11, 11, 0), (10, 40, 0), (26, 42, 0), (27, 43, 0), (37, 53, 0), (59, 75, 3), (24, 40, 7)]
FORMATS = ['rgb-bgr', 'stride4', 'pitched', 'f32-u8', 'minmax', 'nv12-y', 'p010-i420p10', 'depth12']


def pair_u8(h, w, seed):
    r = np.random.RandomState(seed)
    a = r.randint(0, 256, (h, w, 3)).astype(np.uint8)
    b = np.clip(a.astype(np.int32) + r.randint(-25, 26, a.shape), 0, 255).astype(np.uint8)
    return a, b


def pitched(img, extra=5, offset=3):
    """(buffer, view, mask of the view's bytes): `img` [h,w,ps] (or [h,w]) inside a buffer of sentinel bytes, at an odd address
    and with `extra` bytes between rows."""
    x = img if img.ndim == 3 else img[:, :, None]
    h, w, ps = x.shape
    pitch = w * ps + extra
    buf = torch.full((offset + h * pitch + 16,), SENTINEL, dtype=torch.uint8, device='cuda')
    view = buf.as_strided((h, w, ps), (pitch, ps, 1), offset)
    view.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    mask = torch.zeros_like(buf, dtype=torch.bool)
    mask.as_strided((h, w, ps), (pitch, ps, 1), offset).fill_(True)
    return buf, (view if img.ndim == 3 else view[:, :, 0]), mask


def guard_ok(buf, mask):
    return bool((buf[~mask] == SENTINEL).all())


def gpu16(a):
    """A numpy uint16 array as a torch.uint16 GPU tensor (through int16, which every torch op knows)."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


def zeros16(shape):
    return torch.zeros(shape, dtype=torch.int16, device='cuda').view(torch.uint16)


def same(a, b):
    if a.dtype == torch.uint16:
        a, b = a.view(torch.int16), b.view(torch.int16)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def same_summary(x, y):
    """Two score summaries with the same scenes and the same figures (NaN in the same places)."""
    def eq(p, q):
        return p.keys() == q.keys() and all((p[k] == q[k]) or (math.isnan(p[k]) and math.isnan(q[k])) for k in p)
    return len(x['scenes']) == len(y['scenes']) and all(eq(p, q) for p, q in zip(x['scenes'], y['scenes'])) and eq(x['mean'], y['mean'])


def words(levels, depth, msb, r):
    """uint16 words holding `levels` at the top (P010 / P012) or the bottom (yuv420p10le / 12le), the other bits random."""
    junk = r.randint(0, 1 << (16 - depth), levels.shape)
    v = (levels << (16 - depth)) | junk if msb else levels | (junk << depth)
    return v.astype(np.uint16)


def build(fmt, h, w, seed):
    """-> (a, b, layout_a, layout_b, kw, numpy sample arrays of a and b per channel, depth, [(buffer, mask), ...])"""
    r = np.random.RandomState(seed)
    a, b = pair_u8(h, w, seed)
    guards, kw, depth = [], {}, 8
    chans = ('rgb', 'y')
    sa = {c: ref.samples(a, 'hwc_rgb', c) for c in chans}
    sb = {c: ref.samples(b, 'hwc_rgb', c) for c in chans}
    if fmt == 'rgb-bgr':
        ta, tb, la, lb = torch.from_numpy(a).cuda(), torch.from_numpy(np.ascontiguousarray(b[:, :, ::-1])).cuda(), 'hwc_rgb', 'hwc_bgr'
    elif fmt == 'stride4':
        a4 = np.concatenate([a, r.randint(0, 256, (h, w, 1)).astype(np.uint8)], axis=2)
        ta, tb, la, lb = torch.from_numpy(a4).cuda(), torch.from_numpy(b).cuda(), None, None
    elif fmt == 'pitched':
        bufa, ta, ma = pitched(a)
        bufb, tb, mb = pitched(np.ascontiguousarray(b[:, :, ::-1]), extra=5, offset=3)
        assert ta.data_ptr() % 2 == 1 and ta.stride(0) == 3 * w + 5
        assert frames.describe(ta, 'hwc_rgb')[0].data_ptr() == ta.data_ptr()       # passed by stride, not copied
        guards, la, lb = [(bufa, ma), (bufb, mb)], 'hwc_rgb', 'hwc_bgr'
    elif fmt in ('f32-u8', 'minmax'):
        lo, hi = (0.0, 1.0) if fmt == 'f32-u8' else (-1.0, 1.0)
        fa = (r.uniform(-0.1, 1.1, (3, h, w)) * (hi - lo) + lo).astype(np.float32)
        ties = ((np.arange(255, dtype=np.float64) + 0.5) / 255 * (hi - lo) + lo).astype(np.float32)
        fa.reshape(-1)[:min(255, fa.size)] = ties[:min(255, fa.size)]               # the ties of the quantiser too
        kw = dict(min_max=(lo, hi))
        sa = {c: ref.samples(fa, 'chw', c, (lo, hi)) for c in chans}
        b = np.clip(sa['rgb'] + r.randint(-25, 26, (h, w, 3)), 0, 255).astype(np.uint8)
        sb = {c: ref.samples(b, 'hwc_rgb', c) for c in chans}
        ta, tb, la, lb = torch.from_numpy(fa).cuda(), torch.from_numpy(b).cuda(), None, None
    elif fmt == 'nv12-y':
        chans = ('y',)
        ya, yb = a[:, :, 0], b[:, :, 0]
        buf, yv, m = pitched(ya, extra=3 if w % 2 == 0 else 2, offset=1)
        assert yv.stride(0) % 2 == 1 and yv.data_ptr() % 2 == 1
        uv = torch.zeros(((h + 1) // 2, (w + 1) // 2, 2), dtype=torch.uint8, device='cuda')
        u = torch.zeros(((h + 1) // 2, (w + 1) // 2), dtype=torch.uint8, device='cuda')
        ta, la = (yv, uv), 'nv12'
        tb, lb = (torch.from_numpy(np.ascontiguousarray(yb)).cuda(), u, u), 'i420'
        guards = [(buf, m)]
        sa, sb = {'y': ref.samples(ya, 'y', 'y')}, {'y': ref.samples(yb, 'y', 'y')}
    else:
        chans = ('y',)
        depth = 10 if fmt == 'p010-i420p10' else 12
        la_ = r.randint(0, 1 << depth, (h, w))
        lb_ = np.clip(la_ + r.randint(-(1 << (depth - 3)), 1 << (depth - 3), (h, w)), 0, (1 << depth) - 1)
        wa, wb = words(la_, depth, True, r), words(lb_, depth, False, r)
        cs = ((h + 1) // 2, (w + 1) // 2)
        uv, u = zeros16(cs + (2,)), zeros16(cs)
        ta, la = (gpu16(wa), uv), 'p010' if depth == 10 else 'p012'
        tb, lb = (gpu16(wb), u, u), 'i420p10' if depth == 10 else 'i420p12'
        sa, sb = {'y': ref.samples(wa, 'y_msb', 'y', depth=depth)}, {'y': ref.samples(wb, 'y_lsb', 'y', depth=depth)}
        assert np.array_equal(sa['y'][:, :, 0], la_) and np.array_equal(sb['y'][:, :, 0], lb_)
    return ta, tb, la, lb, kw, {c: (sa[c], sb[c]) for c in chans}, depth, guards


def check(got, sa, sb, k, depth, what):
    """got [mse, ssim] (CPU float64) against score_ref on the sample arrays."""
    sse, n, mse, ssim = ref.score(sa, sb, k, depth)
    bar = 1e-10
    if depth > 8 and not math.isnan(ssim):
        host = abs(ssim - ref.score(sa, sb, k, depth, separable=False)[3])       # separable vs 2-D window, both on the CPU
        print("%s: separable vs window form on the host %.3e" % (what, host))
        if host > 1e-11:
            bar = 10 * host
    m, s = float(got[0]), float(got[1])
    print("%s: sse %d over %d samples, ssim %.15f (reference %.15f, bar %.1e)" % (what, sse, n, s, ssim, bar))
    assert m == mse and round(m * n) == sse, (what, m, mse)
    if math.isnan(ssim):
        assert math.isnan(s), (what, s)
    else:
        assert abs(s - ssim) < bar, (what, s, ssim)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d-crop%d" % s)
def test_score_vs_numpy(size, fmt):
    h, w, k = size
    ta, tb, la, lb, kw, samples, depth, guards = build(fmt, h, w, 1000 * h + w)
    big = torch.full((12,), -7.0, dtype=torch.float64, device='cuda')
    for channel, (sa, sb) in samples.items():
        got = frames.score(ta, tb, la, lb, channel=channel, crop_border=k, **kw)
        assert got.dtype == torch.float64 and got.shape == (2,) and got.is_cuda
        again = frames.score(ta, tb, la, lb, channel=channel, crop_border=k, out=big[5:7], **kw)
        assert again.data_ptr() == big[5:7].data_ptr()
        assert torch.equal(got.view(torch.int64), again.view(torch.int64))          # bit-identical run to run
        assert bool((big[:5] == -7.0).all()) and bool((big[7:] == -7.0).all())      # nothing around out
        check(got.cpu(), sa, sb, k, depth, "%s %s %dx%d crop %d" % (fmt, channel, h, w, k))
        swapped = frames.score(tb, ta, lb, la, channel=channel, crop_border=k, **kw).cpu()
        assert float(swapped[0]) == float(got[0])                                   # the two sides take either format
    for buf, mask in guards:
        assert guard_ok(buf, mask)


def test_identical_and_extreme_pairs():
    a, _ = pair_u8(37, 53, 7)
    ta = torch.from_numpy(a).cuda()
    for channel in ('rgb', 'y'):
        m, s = frames.score(ta, ta.clone(), channel=channel).tolist()
        assert m == 0.0 and abs(s - 1.0) < 1e-12
        assert math.isinf(frames.psnr(m))
    zero, full = torch.zeros(27, 43, 3, dtype=torch.uint8, device='cuda'), torch.full((27, 43, 3), 255, dtype=torch.uint8, device='cuda')
    m, s = frames.score(zero, full).tolist()
    assert m == 65025.0 and abs(s - ref.ssim(np.zeros((27, 43, 3)), np.full((27, 43, 3), 255.0))) < 1e-10
    assert frames.score(zero, full, channel='y').tolist()[0] == float((235 - 16) ** 2)
    f0, f1 = torch.zeros(3, 27, 43, device='cuda'), torch.ones(3, 27, 43, device='cuda')
    assert frames.score(f0, full).tolist()[0] == 65025.0 and frames.score(f1 * 7, full).tolist()[0] == 0.0   # (clamped)
    top, uv = gpu16(np.full((12, 12), 1023 << 6, dtype=np.uint16)), zeros16((6, 6, 2))
    assert frames.score((top, uv), (zeros16((12, 12)), uv), 'p010', 'p010', channel='y').tolist()[0] == 1023.0 ** 2
    cpu = frames.score(torch.from_numpy(a), ta, channel='y').tolist()                # a CPU frame travels as bytes
    assert cpu[0] == 0.0


def test_ties_of_y8():
    """Every exact tie of the Y level and its neighbours, as bytes in both orders and as fp32: exactly score_ref's samples."""
    t = ref.tie_triples().astype(np.int32)
    px = [t]
    for c in range(3):
        for d in (-1, 1):
            n = t.copy()
            n[:, c] = np.clip(n[:, c] + d, 0, 255)
            px.append(n)
    px = np.concatenate(px).astype(np.uint8)                                       # 194 * 7 pixels
    h, w = 37, 37
    assert len(px) <= h * w
    a = np.zeros((h * w, 3), dtype=np.uint8)
    a[:len(px)] = px
    a = a.reshape(h, w, 3)
    b = np.roll(a.reshape(-1, 3), 97, axis=0).reshape(h, w, 3)
    sa, sb = ref.samples(a, 'hwc_rgb', 'y'), ref.samples(b, 'hwc_rgb', 'y')
    assert ref.is_tie(a[:, :, 0], a[:, :, 1], a[:, :, 2]).sum() >= 194
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    fa = torch.from_numpy(np.ascontiguousarray(np.transpose(a.astype(np.float32) / 255., (2, 0, 1)))).cuda()
    for x, lx in ((ta, 'hwc_rgb'), (ta.flip(-1).contiguous(), 'hwc_bgr'), (fa, 'chw')):
        check(frames.score(x, tb, lx, 'hwc_rgb', channel='y').cpu(), sa, sb, 0, 8, "ties " + lx)
        # against the levels themselves, as a Y plane: every sample of x is the integer rule's
        plane = (torch.from_numpy(sa[:, :, 0].astype(np.uint8)).cuda(), torch.zeros(19, 19, 2, dtype=torch.uint8, device='cuda'))
        assert frames.score(x, plane, lx, 'nv12', channel='y').tolist()[0] == 0.0, lx


def test_float_pair_is_frame_metrics():
    r = np.random.RandomState(3)
    a = (r.rand(3, 37, 53) * 1.2 - 0.1).astype(np.float32)
    b = np.clip(a + 0.05 * r.standard_normal(a.shape), -0.2, 1.3).astype(np.float32)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    got = frames.score(ta, tb, channel='rgb').cpu()
    want = util.frame_metrics(ta, tb, need_img=None).cpu()
    assert float(got[0]) == float(want[0])
    assert abs(float(got[1]) - float(want[1])) < 1e-10
    got = frames.score(ta * 2 - 1, tb * 2 - 1, min_max=(-1, 1)).cpu()
    want = util.frame_metrics(ta * 2 - 1, tb * 2 - 1, min_max=(-1, 1), need_img=None).cpu()
    assert float(got[0]) == float(want[0]) and abs(float(got[1]) - float(want[1])) < 1e-10


def test_c_abi_errors_leave_out_alone():
    """With real device memory on every pointer: a refused call launches nothing, so `out` keeps its sentinel."""
    lib = L.lib()
    h, w = 24, 40
    a = torch.zeros(h, w, 3, dtype=torch.uint8, device='cuda')
    b = torch.zeros(h, w, 4, dtype=torch.uint8, device='cuda')
    out = torch.full((4,), -7.0, dtype=torch.float64, device='cuda')
    need = lib.dvsr_frame_score_workspace_bytes(3, h, w)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    da, db = L.FrameDesc(L.FRAME_U8_HWC_RGB, h, w, 3 * w, 0, 3), L.FrameDesc(L.FRAME_U8_HWC_BGR, h, w, 4 * w, 0, 4)

    def call(da=da, db=db, args=L.ScoreArgs(L.SCORE_RGB, 0, 8, 0.0, 1.0), out_ptr=out.data_ptr() + 8, nbytes=need, a_ptr=a.data_ptr()):
        return lib.dvsr_frame_score(a_ptr, ctypes.byref(da), b.data_ptr(), ctypes.byref(db), ctypes.byref(args), out_ptr,
                                    ws.data_ptr(), nbytes, L.stream())
    bad = [dict(db=L.FrameDesc(L.FRAME_U8_HWC_BGR, h, w - 1, 4 * w, 0, 4)), dict(da=L.FrameDesc(9, h, w, 3 * w, 0, 3)),
           dict(args=L.ScoreArgs(3, 0, 8, 0.0, 1.0)), dict(args=L.ScoreArgs(L.SCORE_RGB, 0, 10, 0.0, 1.0)),
           dict(da=L.FrameDesc(L.FRAME_U8_Y, h, w, w, 0, 1)), dict(args=L.ScoreArgs(L.SCORE_RGB, 12, 8, 0.0, 1.0)),
           dict(da=L.FrameDesc(L.FRAME_U8_HWC_RGB, h, w, 3 * w - 1, 0, 3)), dict(out_ptr=out.data_ptr() + 4), dict(a_ptr=None),
           dict(da=L.FrameDesc(L.FRAME_U16_Y_MSB, h, w, 2 * w, 0, 2), db=L.FrameDesc(L.FRAME_U16_Y_10, h, w, 2 * w, 0, 2),
                args=L.ScoreArgs(L.SCORE_Y, 0, 10, 0.0, 1.0), a_ptr=a.data_ptr() + 1)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(nbytes=need - 1) == -3
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert call() == 0                                                            # ... and the good call writes out[1:3] alone
    torch.cuda.synchronize()
    assert out.tolist()[0] == -7.0 and out.tolist()[3] == -7.0 and out.tolist()[1] == 0.0 and abs(out.tolist()[2] - 1.0) < 1e-12


# ---- end to end ----------------------------------------------------------------------------------
T, H, W = 7, 13, 15
OPT = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}
_CASE = {}


def e2e():
    """Computed once and never modified: the network and the 8-bit video of tests/test_gpu_frame_io.py's 13 x 15 case, and
    ground-truth videos of the output's size in the formats the cases need."""
    if not _CASE:
        from dynavsr_amd.models.archs.EDVR_arch import EDVR
        net = EDVR()
        net.load_state_dict(synth.damp_residual_branch(synth.edvr_state_dict(0), 0.02), strict=True)
        u8 = (synth.clip(90 + H, 1, T, H, W)[0] * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()      # [T,h,w,3]
        r = np.random.RandomState(17)
        oh, ow = 4 * H, 4 * W
        gt8 = r.randint(0, 256, (T, oh, ow, 3)).astype(np.uint8)
        p010 = ((r.randint(0, 1024, (T, oh * 3 // 2, ow)) << 6) | r.randint(0, 64, (T, oh * 3 // 2, ow))).astype(np.uint16)
        _CASE.update(net=net.cuda(), u8=u8.cuda(), gt8=torch.from_numpy(gt8),
                     gtf=torch.from_numpy(np.ascontiguousarray(np.transpose(gt8.astype(np.float32) / 255., (0, 3, 1, 2)))).cuda(),
                     gtp010=gpu16(p010),
                     gt_small=torch.from_numpy(r.randint(0, 256, (T, 40, 50, 3)).astype(np.uint8)).cuda())
    return _CASE


E2E = {
    'uint8': (dict(), 'gt8', dict()),                                              # (a CPU ground truth: it travels as bytes)
    'float': (dict(out='float'), 'gtf', dict()),
    'nv12-y': (dict(out='nv12'), 'gt8', dict(score='y')),
    'p010': (dict(out='p010'), 'gtp010', dict(gt_layout='p010', score='y')),
    'out_size': (dict(out_size=(40, 50)), 'gt_small', dict(crop_border=2)),
    'cuts': (dict(cuts=[3]), 'gt8', dict(score='y', crop_border=4)),
    'flip_test': (dict(flip_test=True), 'gt8', dict()),
}


@pytest.mark.parametrize("name", list(E2E))
def test_video_scores_end_to_end(name):
    case = e2e()
    kw, gt_key, skw = E2E[name]
    net, video, gt = case['net'], case['u8'], case[gt_key]
    plain = [f.clone() for f in adapt.super_resolve_frames(OPT, net, video, in_flight=2, **kw)]
    rows = {}
    for in_flight in (1, 2):
        scores = torch.full((T, 2), -7.0, dtype=torch.float64, device='cuda')
        out = [f.clone() for f in adapt.super_resolve_frames(OPT, net, video, in_flight=in_flight, gt=gt, scores=scores, **kw, **skw)]
        assert len(out) == T
        for i in range(T):
            assert same(out[i], plain[i]), (name, i)                                # the frames are what they are
            x, lx = (out[i][0], 'chw') if kw.get('out') == 'float' else (out[i], kw.get('out'))
            want = frames.score(x, gt[i], lx, skw.get('gt_layout'), channel=skw.get('score', 'rgb'),
                                crop_border=skw.get('crop_border', 0))
            assert torch.equal(scores[i].view(torch.int64), want.view(torch.int64)), (name, in_flight, i, scores[i], want)
            assert math.isfinite(float(want[0])) and math.isfinite(float(want[1]))
        rows[in_flight] = scores.cpu()
    assert torch.equal(rows[1].view(torch.int64), rows[2].view(torch.int64))       # no dependence on in_flight
    if name in ('uint8', 'cuts', 'p010'):
        peak = 1023 if name == 'p010' else 255
        summary, scores = adapt.evaluate_frames(OPT, net, video, gt, **kw, **skw)
        assert torch.equal(scores.cpu().view(torch.int64), rows[2].view(torch.int64))
        assert same_summary(summary, adapt.score_summary(scores, 5, kw.get('cuts'), peak))
        want = ref.summary(rows[2].tolist(), 5, kw.get('cuts'), peak)
        assert len(summary['scenes']) == len(want['scenes']) == (2 if name == 'cuts' else 1)
        for k, v in want['mean'].items():
            assert (math.isnan(v) and math.isnan(summary['mean'][k])) or abs(summary['mean'][k] - v) <= 1e-12 * abs(v), k


def test_another_network_scores_too():
    """The one-line `Mean` network of tests/test_gpu_frame_io.py: the windows through super_resolve_video, frames.emit per
    result, one score launch behind it."""
    class Mean(torch.nn.Module):
        nframes = 3

        def forward(self, x):
            return x.mean(1)

    r = np.random.RandomState(11)
    u8 = torch.from_numpy(r.randint(0, 256, (5, 13, 15, 3)).astype(np.uint8))
    gt = torch.from_numpy(r.randint(0, 256, (5, 13, 15, 3)).astype(np.uint8)).cuda()
    opt = {'scale': 1, 'network_G': {'which_model_G': 'DUF', 'nframes': 3}}
    for kw in (dict(), dict(multiple=4), dict(out='float')):
        scores = torch.zeros((5, 2), dtype=torch.float64, device='cuda')
        out = [o.clone() for o in adapt.super_resolve_frames(opt, Mean(), u8, padding='replicate', gt=gt, scores=scores,
                                                             score='y', crop_border=1, **kw)]
        plain = [o.clone() for o in adapt.super_resolve_frames(opt, Mean(), u8, padding='replicate', **kw)]
        for i in range(5):
            assert torch.equal(out[i], plain[i])
            x = out[i][0] if kw.get('out') == 'float' else out[i]
            want = frames.score(x, gt[i], channel='y', crop_border=1)
            assert torch.equal(scores[i].view(torch.int64), want.view(torch.int64)), (kw, i)
    summary, got = adapt.evaluate_frames(opt, Mean(), u8, gt, padding='replicate', score='y', crop_border=1, out='float')
    assert torch.equal(got.view(torch.int64), scores.view(torch.int64)) and same_summary(summary, adapt.score_summary(got, 3))
