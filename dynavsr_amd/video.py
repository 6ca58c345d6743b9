"""A video through a network without adaptation: the front and back end that the adaptation loops (adapt.py) share.

    super_resolve_video    clips in, SR frames out, `in_flight` clips on the GPU at a time
    super_resolve_frames   a decoded video in, SR frames out: resolve the arguments (_frame_arguments), then the EDVR stream
                           path (_stream_frames: every frame's features extracted once) or, for any other network, windows
                           built here and run as clips (_clip_frames)
    the schedules          scene_bounds, video_windows, stream_slots, stream_schedule (pure Python)
    the tile geometry      tile_origins, tile_footprint, choose_tile
    the scores             score_summary, evaluate_frames
    a degraded video       degrade_frames, evaluate_degraded: a ground-truth video blurred, sub-sampled and quantised on the device,
                           super-resolved and scored against the frames it came from

This module imports nothing from adapt.py; adapt.py re-exports its public names."""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from . import engine
from . import frames as fio


def backbone_input(opt, clip):
    """What the drivers feed netG: the clip itself for EDVR / DUF; for TOFlow, which works at the output size, the
    clip brought there by F.interpolate(scale_factor=scale, mode='bicubic', align_corners=True)
    (test_dynavsr.py:188-193, 245-250) -- one native launch (tofops.upsample_bicubic_ac), differentiable."""
    if (opt['network_G'] or {}).get('which_model_G') == 'TOF' and clip.is_cuda:
        from . import tofops
        return tofops.upsample_bicubic_ac(clip, opt['scale'])
    if (opt['network_G'] or {}).get('which_model_G') == 'TOF':
        b, t, c, h, w = clip.shape
        up = F.interpolate(clip.reshape(b * t, c, h, w), scale_factor=opt['scale'], mode='bicubic', align_corners=True)
        return up.reshape(b, t, c, h * opt['scale'], w * opt['scale'])
    return clip


_EXTRA_STREAMS = {}


def _side_streams(lqs_device):
    """The side stream of the full-size forwards, created once per device: the caching allocator keeps one block pool per
    stream, and the 3 GB workspaces must come back from the pool, not from hipMalloc, on every call.  ONE stream carries
    both the next clip's baseline forward and the current clip's adapted forward: on two streams they run concurrently
    with each other as well whenever ROCm gives them separate hardware queues (GPU_MAX_HW_QUEUES >= 5), and three
    full-size tapes side by side take 32.5 ms per frame against 27.3 sequential and 23.3 with one stream (which is what
    two streams measured only while they happened to share a queue).  (The first of super_resolve_video's extra streams.)"""
    a = _clip_streams(lqs_device, 2)[1]
    return (a, a)


def _clip_streams(device, n):
    """The caller's current stream + n - 1 further HIP streams of the device.  The further ones are created once and shared
    with adapt_video's forward stream (_side_streams): one block pool of the caching allocator and one launch plan +
    workspace per stream must be found again on the next call -- and every extra stream a process has used takes part in
    ROCm's stream -> hardware-queue assignment, which the legs with a weight-gradient side stream are sensitive to (DESIGN
    3.1c; with two private streams here the per-frame pipeline that ran afterwards measured 61 instead of 71 frames/s)."""
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    have = _EXTRA_STREAMS.setdefault(key, [])
    while len(have) < n - 1:
        have.append(torch.cuda.Stream(device=key))
    return [torch.cuda.current_stream(key)] + have[:n - 1]


def _check_flip_test(flip_test, who):
    if not isinstance(flip_test, bool):
        raise ValueError("%s: flip_test=%r must be a bool" % (who, flip_test))


def _flip_test_forward(opt, net, lq):
    """flipx4_forward of the reference (utils/util.py:232-254) on one clip [B,N,3,H,W], on the current stream: the forward
    on the clip and on its three mirror images (frames.flip), then the un-flips and the mean in one launch (frames.flip_mean)."""
    if lq.dtype != torch.float32 or not lq.is_contiguous() or lq.data_ptr() % 16:
        lq = lq.float().clone(memory_format=torch.contiguous_format)
    ys = [net(backbone_input(opt, lq if v == 0 else fio.flip(lq, v))) for v in range(4)]
    return fio.flip_mean(*[y if y.is_contiguous() else y.contiguous() for y in ys])


def super_resolve_video(opt, net, clips, in_flight=2, flip_test=False):
    """The un-adapted forward of test_dynavsr.py:200-204 (`model.feed_data(val_data, need_GT=False); model.test()`) over a
    stream of clips, as a generator: yields the SR frame [B, 3, sH, sW] of every clip [B, N, 3, H, W], in order.

    `in_flight` clips are on the GPU at a time, one HIP stream each (round robin: the caller's stream and in_flight - 1
    further ones).  A single EDVR-M forward at 180x320 is 85 dependent launches of 1125-workgroup grids on 256 CUs -- 4.4
    rounds of workgroups each, the last one 40 % full, and 5-6 us of idle GPU between two launches -- and a second queue
    fills both: 161.9 -> 187.9 frames/s with two clips in flight, 189.2 with three (tools/fwd_concurrent.py; one forward
    over a batch of 8 clips: 180.4).  Every clip runs the launches it would run alone (its own plan and workspace, keyed
    by the stream) except the weight packing, which only the first clip on a stream does (the workspace and the packs in it
    are kept for the video; an in-place update of the weights between clips re-packs), so the outputs are bit-identical to
    `net(clip)`.  A yielded frame stays valid until the generator is
    advanced `in_flight` times; clips and results are ordered against the caller's current stream.

    flip_test=True: the reference's x4 self-ensemble (`flip_test` of test_Vid4_REDS4_with_GT.py, util.flipx4_forward) -- per
    clip four forwards, on the clip and on frames.flip of it in W, in H and in both, and one frames.flip_mean that un-flips
    and averages them in the reference's order, all on the clip's stream; the clip's and the output's width must be
    multiples of 4.  False takes exactly the calls above.  (The x8 ensemble with transposes is not provided.)"""
    _check_flip_test(flip_test, "super_resolve_video")
    main = None
    streams = None
    pending = []
    # one workspace per (plan, stream) for the whole video, and with it the packed weights: the network is the same for every
    # clip, so only the first forward on a stream packs (engine.FrozenWeights; keyed on the parameters' version counters)
    frozen = engine.FrozenWeights()
    was_training = net.training
    net.eval()
    try:
        for i, c in enumerate(clips):
            lq = c['LQs'] if isinstance(c, dict) else c
            if not lq.is_cuda:
                lq = lq.cuda()
            if streams is None:
                # (the caller's stream ON THE CLIPS' DEVICE -- not the current device's, which may be another one)
                main = torch.cuda.current_stream(lq.device)
                streams = _clip_streams(lq.device, max(1, int(in_flight)))
            yield from _hand_out(pending, main, len(streams) - 1)    # the oldest clip ran on the stream this one takes
            s = streams[i % len(streams)]
            if s != main:
                s.wait_stream(main)                  # the clip (and the weights) were produced on the caller's stream
            with torch.cuda.stream(s), torch.no_grad(), frozen:
                sr = _flip_test_forward(opt, net, lq) if flip_test else net(backbone_input(opt, lq))
                ev = torch.cuda.Event()
                ev.record(s)
            if s != main:
                lq.record_stream(s)
            pending.append((sr, ev))
        yield from _hand_out(pending, main)
    finally:
        # a generator closed early leaves forwards running on the side streams: whatever the caller does next on its stream
        # (an inner step updates the weights they read) must come behind them
        for _ in _hand_out(pending, main):
            pass
        net.train(was_training)


def _hand_out(pending, main, keep=0):
    """The in-order hand-out of the two video generators: yields the oldest results of `pending` [(result, event of the launch
    that wrote it), ...] until `keep` are left, each ordered against the caller's stream `main` first (the wait for its event,
    and record_stream, since the result was allocated on the stream it ran on).  keep = in_flight - 1 in front of a launch,
    0 to drain at the end; iterated without a consumer in a `finally`, it does the waits alone."""
    while len(pending) > keep:
        sr, ev = pending.pop(0)
        main.wait_event(ev)
        sr.record_stream(main)
        yield sr


def scene_bounds(T, cuts):
    """The scenes [(a, b), ...] of a video of T frames cut at `cuts`: a strictly increasing sequence of ints in (0, T), k
    meaning that frame k is the first frame of a new scene ([] = one scene).  Anything else is a ValueError."""
    import numbers
    T = int(T)
    if isinstance(cuts, (str, bytes)) or not hasattr(cuts, '__iter__'):
        raise ValueError("cuts=%r: a sequence of frame numbers (or None)" % (cuts,))
    ks = list(cuts)
    for k in ks:
        if isinstance(k, bool) or not isinstance(k, numbers.Integral):
            raise ValueError("cuts: %r is not an int" % (k,))
    ks = [int(k) for k in ks]
    for i, k in enumerate(ks):
        if not 0 < k < T:
            raise ValueError("cuts: %d is outside (0, %d) -- a cut names the first frame of a new scene" % (k, T))
        if i and k <= ks[i - 1]:
            raise ValueError("cuts: %s is not strictly increasing" % (ks,))
    edges = [0] + ks + [T]
    return list(zip(edges[:-1], edges[1:]))


def video_windows(T, nframes, padding='new_info', cuts=None):
    """(windows, scenes): the window (list of nframes frame numbers) of every centre 0 .. T - 1, and the number of scenes.

    cuts=None: one scene, data.util.index_generation(centre, T, nframes, padding); ValueError where a window leaves [0, T).
    Scene mode (any other `cuts`, see scene_bounds): the window of centre c in the scene [a, b) is
    a + index_generation(c - a, b - a, nframes, padding) -- what the reference's datasets give, which read one folder per
    scene -- and a scene too short for `padding` (some window would leave [a, b)) takes 'replicate', which never leaves it,
    for all of its windows.  Nothing is raised for a short scene."""
    from .data.util import index_generation
    T, nframes = int(T), int(nframes)
    if cuts is None:
        windows = [index_generation(c, T, nframes, padding) for c in range(T)]
        for c, win in enumerate(windows):
            if min(win) < 0 or max(win) >= T:
                raise ValueError("stream_schedule: %d frames are too few for windows of %d under padding %r (centre %d would "
                                 "read frames %s)" % (T, nframes, padding, c, win))
        return windows, 1
    scenes = scene_bounds(T, cuts)
    windows = []
    for a, b in scenes:
        wins = [index_generation(c, b - a, nframes, padding) for c in range(b - a)]
        if any(min(win) < 0 or max(win) >= b - a for win in wins):
            wins = [index_generation(c, b - a, nframes, 'replicate') for c in range(b - a)]
        windows += [[a + i for i in win] for win in wins]
    return windows, len(scenes)


def stream_slots(nframes, in_flight, scenes=1):
    """The capacity of the frame cache that stream_schedule assumes (see there)."""
    if scenes > 1 and in_flight > 1:
        return 2 * nframes + in_flight - 2
    return nframes + in_flight - 1


def stream_schedule(T, nframes, padding='new_info', in_flight=2, cuts=None):
    """The frame-cache schedule of super_resolve_frames, as pure Python: for every centre frame 0 .. T - 1 yields
    (centre, frames_to_extract, [(frame, slot), ...], window_slots).

    The window of a centre is data.util.index_generation(centre, T, nframes, padding).  A frame is extracted when a
    window first needs it; frames go in increasing order, each exactly once (a window that needs frame f finds 0 .. f
    extracted), frame f into slot f % slots of a cache of slots = nframes + in_flight - 1.  That capacity is enough for
    the four padding modes: a frame is overwritten nframes + in_flight - 1 frames later, when neither the current window,
    nor the in_flight - 1 before it that may still be running, nor any later one names it (tests/test_stream_schedule.py
    simulates it).  window_slots are the cache slots of the window's frames, in window order.
    T < nframes is accepted only where every window stays inside [0, T); otherwise ValueError, where the reference would
    index past the end of its frame list.

    cuts (None: all of the above, unchanged): scene mode, the windows of video_windows -- no window names a frame of
    another scene, and a short scene raises nothing.  The properties are the same; the capacity is not.  With more than
    one scene the windows that end a scene reach nframes frames back while the first window of the next one reaches
    nframes - 1 frames ahead, and the smallest cache that always works with slot = frame % slots is
        slots = nframes                        for in_flight == 1,
        slots = 2 * nframes + in_flight - 2    otherwise
    (stream_slots; found and held by simulation over nframes 3, 5, 7, in_flight 1 .. 4, the four modes, T <= 29 and cut
    sets of every single cut, a cut at every frame and random ones: tests/test_scene_schedule.py, which also shows that
    one slot fewer fails).  One scene (cuts=[]) keeps nframes + in_flight - 1."""
    T, nframes, in_flight = int(T), int(nframes), int(in_flight)
    if T < 1 or nframes < 1 or in_flight < 1:
        raise ValueError("stream_schedule: T=%d, nframes=%d, in_flight=%d must be positive" % (T, nframes, in_flight))
    windows, scenes = video_windows(T, nframes, padding, cuts)
    slots = stream_slots(nframes, in_flight, scenes)
    done = 0                       # frames 0 .. done - 1 are extracted
    for c, win in enumerate(windows):
        new = list(range(done, max(done, max(win) + 1)))
        done += len(new)
        yield c, new, [(f, f % slots) for f in new], [f % slots for f in win]


def _video_format(frames, layout, who="super_resolve_frames"):
    """(layout, h, w) of a video -- a [T,...] tensor or a list of frames of one kind and size.  No GPU call."""
    if len(frames) < 1:
        raise ValueError("%s: no frames" % who)
    first = fio.resolve_layout(frames[0], layout)
    if not torch.is_tensor(frames):
        def kind(f):        # a tensor's, or those of the planes of a YCbCr frame
            if torch.is_tensor(f):
                return f.dtype, tuple(f.shape)
            return [kind(p) for p in f] if isinstance(f, (tuple, list)) else type(f).__name__
        for i, f in enumerate(frames):
            if kind(f) != kind(frames[0]):
                raise ValueError("%s: frame %d is %s, frame 0 is %s" % (who, i, kind(f), kind(frames[0])))
            fio.resolve_layout(f, layout)
    return first


MAX_IMAGE_BYTES = 1 << 32     # the conv and DCN kernels address one image of a tensor with 32-bit offsets (csrc/common.h)


def tile_origins(n, tile, overlap):
    """The origins of the tiles of one axis of padded length n (a multiple of 4), in LR pixels: tile a multiple of 4, overlap a
    multiple of 4 with 0 <= overlap <= tile / 2.  tile >= n: [0], one tile of length n.  Otherwise step = tile - overlap and
    the origins are k * step for every k * step < n - tile, then n - tile: every tile has the same size, the last one is anchored
    at the edge, every origin is a multiple of 4 and a position is covered by at most 3 tiles (dvsr_frame_stitch_origins; host
    code)."""
    import ctypes
    from . import _lib as L
    n, tile, overlap = int(n), int(tile), int(overlap)
    count = L.lib().dvsr_frame_stitch_origins(n, tile, overlap, None, 0)
    if count < 1:
        raise ValueError("tile_origins: " + L.lib().dvsr_last_error().decode("utf-8", "replace"))
    arr = (ctypes.c_int * count)()
    L.lib().dvsr_frame_stitch_origins(n, tile, overlap, arr, count)
    return list(arr)


def _check_tile(tile, overlap, budget=None, who="super_resolve_frames"):
    """(tile, overlap) of the tile arguments: tile is None, 'auto' or (th, tw); ValueError for anything else.  No GPU call."""
    import numbers

    def integral(v):
        return isinstance(v, numbers.Integral) and not isinstance(v, bool)
    if not integral(overlap) or overlap < 0 or overlap % 4:
        raise ValueError("%s: tile_overlap=%r must be a multiple of 4, >= 0" % (who, overlap))
    if budget is not None and not (isinstance(tile, str) and tile == 'auto'):
        raise ValueError("%s: tile_budget is the budget of tile='auto', got tile=%r" % (who, tile))
    if budget is not None and (isinstance(budget, bool) or not isinstance(budget, numbers.Real) or not budget > 0):
        raise ValueError("%s: tile_budget=%r must be a positive number of bytes" % (who, budget))
    if tile is None:
        return None, int(overlap)
    if isinstance(tile, str):
        if tile != 'auto':
            raise ValueError("%s: tile=%r (None, 'auto', an int or (th, tw))" % (who, tile))
        return 'auto', int(overlap)
    if integral(tile):
        tile = (tile, tile)
    if not isinstance(tile, (tuple, list)) or len(tile) != 2 or not all(integral(v) for v in tile):
        raise ValueError("%s: tile=%r (None, 'auto', an int or (th, tw))" % (who, tile))
    for v in tile:
        if v % 4 or v < 16 or v < 2 * overlap:
            raise ValueError("%s: tile=%r with tile_overlap=%d: a tile side is a multiple of 4, at least 16 and at least twice the "
                             "overlap" % (who, tuple(tile), overlap))
    return (int(tile[0]), int(tile[1])), int(overlap)


def _tile_parts(net, h, w, tile, overlap, in_flight, scenes=1, flip_test=False, multiple=4):
    """tile_footprint's terms as a dict, 'plan' (a StreamPlan built for the query alone, never run), 'tile' and 'grid' beside
    them."""
    from .models.archs.EDVR_arch import EDVR
    if not isinstance(net, EDVR):
        raise ValueError("tile_footprint: the footprint comes from an EDVR stream plan's queries; got %s" % type(net).__name__)
    tile, overlap = _check_tile(tile, overlap, who="tile_footprint")
    if tile == 'auto':
        raise ValueError("tile_footprint: tile='auto' is choose_tile's answer, pass it")
    in_flight, scenes, mult = max(1, int(in_flight)), max(1, int(scenes)), int(multiple)
    mult *= 4 // math.gcd(mult, 4)
    Hp, Wp = fio.padded_size(h, w, mult)
    th, tw = (Hp, Wp) if tile is None else (min(tile[0], Hp), min(tile[1], Wp))
    ny, nx = len(tile_origins(Hp, th, overlap)), len(tile_origins(Wp, tw, overlap))
    n_tiles, nv, s = ny * nx, (4 if flip_test else 1), int(net.scale)
    plan = engine.StreamPlan(net._cfg(), th, tw, n_tiles * nv * stream_slots(int(net.nframes), in_flight, scenes))
    tile_out = 3 * s * th * s * tw * 4                       # one fuse tape's output
    return {'plan': plan, 'tile': (th, tw), 'grid': (ny, nx),
            'cache': plan.cache_bytes,
            'workspaces': in_flight * plan.workspace_bytes,
            'tile_buffers': in_flight * n_tiles * tile_out if n_tiles > 1 else 0,
            'staging': in_flight * 3 * s * Hp * s * Wp * 4,
            'flip': in_flight * (2 * 3 * th * tw * 4 + 4 * tile_out) if flip_test else 0}


_FOOTPRINT_TERMS = ('cache', 'workspaces', 'tile_buffers', 'staging', 'flip')


def tile_footprint(net, h, w, tile, overlap=16, in_flight=2, scenes=1, flip_test=False, multiple=4):
    """The bytes of every allocation that super_resolve_frames(net, h x w frames, tile=tile, tile_overlap=overlap, ...) makes for
    an EDVR network itself, from the stream plan's queries and without a GPU (the network may be on the CPU): the frame cache
    (n_tiles * nv * stream_slots slots of the tile's plan), one workspace per window in flight, and per window in flight the
    [n_tiles,3,s th,s tw] buffer of the fuse tapes' outputs (more than one tile), the stitched / fuse tape's [1,3,s Hp,s Wp]
    frame (the staging buffer, or the yielded tensor itself), and under flip_test the two [3,th,tw] mirror buffers and the
    four fuse outputs.  Not counted: the frames the caller holds, a frame's bytes on their way in, the yielded frames of
    `out` / `out_size` (a resampled frame and the encoder's bytes: a few times oh x ow), `scores`' workspace, and what the
    caching allocator rounds up.  tile=None: the whole frame as one tile.  `scenes`: 1, or any larger number for a video with
    cuts (stream_slots)."""
    parts = _tile_parts(net, h, w, tile, overlap, in_flight, scenes, flip_test, multiple)
    return sum(parts[k] for k in _FOOTPRINT_TERMS)


def choose_tile(net, h, w, budget, overlap=16, in_flight=2, scenes=1, flip_test=False, multiple=4):
    """(th, tw): the tile of the grid with the fewest tiles whose tile_footprint is at most `budget` bytes and whose plan passes
    the size check (StreamPlan.max_image_bytes < 2^32); among grids of one tile count the tile closest to square.  For a grid of
    ky x kx tiles the tile is the smallest that gives it: per axis the padded length itself (k = 1), or the smallest multiple of
    `multiple` (raised to a multiple of 4) >= (n + (k - 1) overlap) / k, at least 16 and 2 * overlap.  At most 16 tiles per axis
    are tried.  ValueError when no grid fits.  Host code."""
    _, overlap = _check_tile(None, overlap, who="choose_tile")
    mult = int(multiple) * (4 // math.gcd(int(multiple), 4))
    Hp, Wp = fio.padded_size(h, w, mult)

    def axis(n):
        found = {}
        for k in range(1, 17):
            t = n if k == 1 else max(-(-(n + (k - 1) * overlap) // (k * mult)) * mult, -(-16 // mult) * mult,
                                     -(-2 * overlap // mult) * mult)
            if t <= n and (k == 1 or t < n) and len(tile_origins(n, t, overlap)) == k:
                found.setdefault(k, t)
        return found
    ys, xs = axis(Hp), axis(Wp)
    grids = sorted(((ky * kx, abs(ys[ky] - xs[kx]), ys[ky], xs[kx]) for ky in ys for kx in xs))
    for _, _, th, tw in grids:
        parts = _tile_parts(net, h, w, (th, tw) if (th, tw) != (Hp, Wp) else None, overlap, in_flight, scenes, flip_test, mult)
        if parts['plan'].max_image_bytes < MAX_IMAGE_BYTES and sum(parts[k] for k in _FOOTPRINT_TERMS) <= budget:
            return th, tw
    raise ValueError("choose_tile: no grid of at most 16 x 16 tiles of a %d x %d frame fits %d bytes (overlap %d, in_flight %d)"
                     % (h, w, int(budget), overlap, max(1, int(in_flight))))


def _frame_format(who, frames, layout, out, multiple, pad_mode, matrix, yuv_range, out_size, sr_scale, default_multiple,
                  multiple_of, siting='left'):
    """The front end's checks of a video that is taken as a decoder delivers it, shared by super_resolve_frames and
    adapt_frames: (lay, h, w, out_fmt, Hp, Wp, out_size, mult) -- the frames' layout and size, the format of the yielded frames,
    the padded size, `out_size` (None where it is the SR frame's own size) and the multiple the frames are padded to
    (`multiple`, None: default_multiple; raised to a multiple of `multiple_of`).  ValueError for anything else; no GPU call."""
    lay, h, w = _video_format(frames, layout, who)
    if out not in (None, 'float', 'hwc_rgb', 'hwc_bgr') + fio.RGB_LAYOUTS and not fio.is_yuv(out):
        raise ValueError("%s: out=%r (None, 'float', 'hwc_rgb', 'hwc_bgr' or one of %s)" % (
            who, out, ', '.join(fio.RGB_LAYOUTS + fio.ALL_YUV_LAYOUTS)))
    fio.check_yuv_names(matrix, yuv_range, siting)
    out_fmt = out if out is not None else ('float' if lay == 'chw' else lay)
    if out_size == (sr_scale * h, sr_scale * w):
        out_size = None                           # the SR frame's own size: today's calls
    if out_size is not None:
        fio.check_resize(sr_scale * h, sr_scale * w, out_size, "%s: out_size" % who)
    if fio.is_yuv(out_fmt):
        oh, ow = out_size if out_size is not None else (sr_scale * h, sr_scale * w)
        if fio.packed_needs(out_fmt, oh, ow):
            raise ValueError("%s: a packed %s output of %d x %d needs %s%s" % (
                who, out_fmt, oh, ow, fio.packed_needs(out_fmt, oh, ow), " (out_size)" if out_size is not None else ""))
    if h < 4 or w < 4:
        raise ValueError("%s: frames of %d x %d (at least 4 x 4)" % (who, h, w))
    mult = int(multiple) if multiple is not None else int(default_multiple)
    if mult < 1:
        raise ValueError("%s: multiple=%r must be positive" % (who, multiple))
    if mult % multiple_of:
        mult *= multiple_of // math.gcd(mult, multiple_of)   # the EDVR plans and the tile grid take multiples of 4 only
    Hp, Wp = fio.padded_size(h, w, mult)
    fio.check_pad(h, w, Hp, -(-Wp // 4) * 4, pad_mode)
    return lay, h, w, out_fmt, Hp, Wp, out_size, mult


def _peak(out_fmt, gt_layout=None):
    """2^d - 1 of the samples that the scores of an `out_fmt` video against a `gt_layout` one compared: the depth of the output's
    layout, or, for a float or 8-bit output, that of an integer ground truth (frames.check_score), else 255."""
    for lay in (out_fmt, gt_layout):
        if fio.is_yuv(lay) or lay in fio.RGB_LAYOUTS:
            return 2 ** fio.layout_depth(lay) - 1
    return 255


_SCORES_LATER = object()      # `scores` of a check that runs ahead of the call that allocates them (evaluate_degraded)


def _check_scores(who, scores, T, name="scores"):
    if scores is _SCORES_LATER:
        return
    if not (torch.is_tensor(scores) and scores.dtype == torch.float64 and tuple(scores.shape) == (T, 2)
            and scores.is_cuda and scores.is_contiguous()):
        raise ValueError("%s: gt needs %s, a contiguous float64 [%d, 2] tensor on the GPU" % (who, name, T))


def _frame_scoring(who, T, gt, gt_layout, scores, score, crop_border, out_fmt, out_size, sr_scale, h, w, matrix, yuv_range):
    """The checks of the `gt` arguments of the two frame generators, and score_into(i, sr, into=scores): row i of `into` from
    the frame about to be yielded, on the current stream.  None without `gt`.  ValueError for anything else; no GPU call."""
    if gt is None:
        if scores is not None:
            raise ValueError("%s: scores without gt" % who)
        return None
    if len(gt) != T:
        raise ValueError("%s: gt has %d frames, the video %d" % (who, len(gt), T))
    glay, gh, gw = _video_format(gt, gt_layout, who)
    olay = 'chw' if out_fmt == 'float' else out_fmt
    oh, ow = out_size if out_size is not None else (sr_scale * h, sr_scale * w)
    fio.check_score((olay, oh, ow), (glay, gh, gw), score, crop_border, (0, 1), "%s: gt" % who)
    if fio.is_yuv(olay) and not fio.is_yuv(glay) and (matrix, yuv_range) != ('bt601', 'limited'):
        raise ValueError("%s: the Y plane of a %s output is the Y8 of an RGB gt for matrix='bt601', "
                         "yuv_range='limited' alone, not for %r, %r" % (who, olay, matrix, yuv_range))
    _check_scores(who, scores, T)

    def score_into(i, sr, into=scores):
        fio.score(sr[0] if olay == 'chw' else sr, gt[i], olay, glay, channel=score, crop_border=crop_border, out=into[i])
    return score_into


def _untouched(geometry, out_fmt, out_size):
    """Float output of an unpadded frame at its own size: the network's tensor is the yielded one (the fuse tape writes it, no
    staging buffer), nothing is cropped, resampled or converted."""
    h, w, Hp, Wp = geometry
    return out_fmt == 'float' and (Hp, Wp) == (h, w) and out_size is None


def _stream_buffer(buffers, k, make):
    """buffers[k], made by make() on first use: a buffer of stream k is allocated once per video, never per frame."""
    if k not in buffers:
        buffers[k] = make()
    return buffers[k]


def _finish_frame(who, sr, geometry, out_fmt, out_size, sr_scale, matrix, yuv_range, i=None, score_into=None, into=None,
                  resized=None, siting='left'):
    """The back end of the two frame generators for a network output sr [1,3,s Hp,s Wp] of a frame that was padded from
    h x w to Hp x Wp (geometry): frame i as it is yielded -- the s h x s w crop, resampled to `out_size` and converted to
    `out_fmt` -- and its score, on the current stream.  `resized`: the stream's frames.resize_buffer(out_size), which then
    holds the resampled frame in front of a conversion (None: emit(size=) allocates one per frame)."""
    h, w, Hp, Wp = geometry
    s = sr.shape[-2] // Hp
    if out_size is not None:
        if s != sr_scale:
            raise RuntimeError("%s: the network scales by %d, opt['scale'] says %d" % (who, s, sr_scale))
        if out_fmt == 'float':
            sr = fio.resize(sr, s * h, s * w, out_size)[None]
        elif resized is not None:
            fio.resize(sr, s * h, s * w, out_size, out=resized)
            sr = fio.emit(resized, out_size[0], out_size[1], out_fmt, matrix=matrix, yuv_range=yuv_range, siting=siting)
        else:
            sr = fio.emit(sr, s * h, s * w, out_fmt, matrix=matrix, yuv_range=yuv_range, size=out_size, siting=siting)
    elif out_fmt == 'float':
        sr = sr if _untouched(geometry, out_fmt, out_size) else fio.emit(sr, s * h, s * w, 'chw')[None]
    else:
        sr = fio.emit(sr, s * h, s * w, out_fmt, matrix=matrix, yuv_range=yuv_range, siting=siting)
    if score_into is not None:
        if into is None:
            score_into(i, sr)                      # (behind the conversion, on the caller's stream like it)
        else:
            score_into(i, sr, into)
    return sr


def super_resolve_frames(opt, net, frames, padding='new_info', in_flight=2, *, layout=None, out=None, pad_mode='reflect',
                         multiple=None, matrix='bt601', yuv_range='limited', cuts=None, cut_threshold=10.0, out_size=None,
                         flip_test=False, gt=None, gt_layout=None, score='rgb', crop_border=0, scores=None,
                         tile=None, tile_overlap=16, tile_budget=None, siting='left'):
    """Super-resolves a VIDEO: `frames` is a [T,3,H,W] tensor or a list of [3,H,W] frames (CPU or GPU); yields the SR frame
    [1,3,sH,sW] of every frame, in order -- what `net(frames[index_generation(i, T, nframes, padding)][None])` gives, the
    sliding-window test of the reference's video datasets (video_test_dataset_int.py:219, `padding: new_info` in the
    shipped YAMLs), without the caller cutting clips.

    EDVR: consecutive windows share all but one frame, and everything up to L3_fea depends on one frame alone, so every
    frame's L1 / L2 / L3 features are extracted ONCE into a cache of nframes + in_flight - 1 slots (engine.StreamPlan,
    stream_schedule) and each window runs one gather launch + the tape from PCD alignment on.  `in_flight` windows are on
    the GPU at a time, one HIP stream each (the caller's and _clip_streams' further ones); a window's extractions run on
    its own stream.  Two kinds of events order the cache: frame extracted -> the windows that gather it, and window done
    -> the extraction that overwrites one of its slots (the cache is read by the gather alone, at the start of a window;
    by stream_schedule's capacity the windows concerned finished long before).  Extraction at batch 1 may pick other kernel
    kinds than the batch of a whole clip, so results match the per-clip forward at the parity bar, not bit for bit; they
    do not depend on in_flight.
    Any other network (TOFlow, DUF): the windows are built here and run by super_resolve_video -- same interface, no cache.
    A yielded frame stays valid until the generator is advanced `in_flight` times; frames and results are ordered against
    the caller's current stream.

    What a decoder delivers is accepted as it is (frames.py, csrc/frame_io.hip): `frames` may also be uint8 [T,H,W,3|4] or
    a list of [H,W,3|4] in RGB or BGR order (`layout`: 'chw' | 'hwc_rgb' | 'hwc_bgr'; None = 'chw' for float frames,
    'hwc_rgb' for uint8), pitched and offset views passed by stride, CPU frames copied to the device as bytes; and any
    H, W >= 4: a frame is padded at the bottom and right from itself (`pad_mode` 'reflect' | 'replicate', the modes of
    torch.nn.functional.pad) to a multiple of `multiple` (None: 4 for EDVR, 1 for other networks; 16 for TOFlow), and the
    SR frame is cropped back to s*H x s*W.  `out`: None keeps [1,3,sH,sW] fp32 for float frames and gives uint8
    [sH,sW,3] on the device in the input's channel order for uint8 frames (util.tensor2img's image); 'float', 'hwc_rgb',
    'hwc_bgr' force one.  Float planar frames that need no padding, with `out` unset, take exactly the calls described
    above (the crop / conversion otherwise runs as one more launch on the window's stream, out of a per-stream staging
    buffer).
    What a VIDEO decoder delivers is YCbCr 4:2:0 (frames.py, csrc/frame_yuv.hip): with `layout` 'nv12' or 'i420' (never
    inferred) `frames` is a uint8 [T, H*3/2, W] tensor or a list of packed frames or of plane tuples, converted with `matrix`
    ('bt601' | 'bt709' | 'bt2020nc'), `yuv_range` ('limited' | 'full') and `siting` ('left' | 'center' | 'topleft': where the
    chroma samples sit, frames.py; one name for input and output) in the launch that fills the frame cache; `out` None then
    yields packed uint8 [sH*3/2, sW] frames of the input's layout on the device, written from the fp32 SR frame in one launch,
    and 'nv12' / 'i420' force such an output for RGB and float inputs too (sH and sW must be even).
    High-bit-depth video (HEVC Main10, AV1, VP9 profile 2): `layout` 'p010' / 'p012' (semi-planar, the level in the top bits of a
    16-bit word) or 'i420p10' / 'i420p12' (yuv420p10le / yuv420p12le), as uint16 or int16 tensors shaped like their 8-bit
    counterparts (csrc/frame_yuv.hip too); `out` None then yields packed torch.uint16 frames of the input's layout, quantised
    from the fp32 SR frame to 1024 / 4096 levels, and the four names force such an output for any input -- an 8-bit source can
    leave with 10 bits.
    Footage that is not 4:2:0 (frames.py): `layout` and `out` also take the 4:2:2 names 'i422' / 'nv16' / 'i422p10' /
    'i422p12' / 'p210' / 'p212' (packed [T, 2H, W] or planes; a packed output needs an even sW or `out_size` width alone) and the
    4:4:4 names 'i444' / 'i444p10' / 'i444p12' (packed [T, 3H, W]; any size), the 16-bit ones as the output of any input;
    everything said of the 4:2:0 layouts holds for them.
    RGB above 8 bits and planar integer RGB (frames.RGB_LAYOUTS, csrc/frame_rgb.hip): `layout` and `out` take
    'hwc_rgb16' / 'hwc_bgr16' (uint16 / int16 [T,H,W,3|4] words: 16-bit PNG / TIFF / DPX, rgb48le), 'chw_rgb8' / 'chw_gbr8' (uint8
    [T,3,H,W]: torchvision's decoded images, gbrp) and 'chw_rgb10' ... 'chw_gbr16' (uint16 / int16 [T,3,H,W]: gbrp10le / 12le / 16le,
    the level in the low bits), never inferred; `out` None yields the input's layout -- torch.uint16 (uint8 at depth 8) frames of
    2^d levels -- and the names force such an output for any input, so an 8-bit or YCbCr source can leave as 16-bit RGB.
    A video of several scenes: `cuts` (None: one scene, the calls of before) lists the first frame of every new scene, or is
    'auto' for frames.detect_cuts(frames, layout, threshold=cut_threshold); no window then crosses a cut (video_windows), so
    every scene comes out as if it had been passed alone, and the frame cache has stream_slots' capacity.
    A target output size: with `out_size` = (oh, ow) every yielded frame is oh x ow instead of sH x sW, for every network and
    every `out` ('float': [1,3,oh,ow]; a packed 4:2:0 output needs oh and ow even, sH and sW no longer).  The SR frame's
    sH x sW crop -- never the padding around it -- is resampled on the device (frames.resize: separable antialiased bicubic,
    torch's interpolate(mode='bicubic', antialias=True); per axis sH / oh <= 4 and oh / sH <= 2) by one more launch on the
    window's stream, in front of the conversion.  None, or (sH, sW) itself, takes exactly the calls described above.
    More GPU time for a better frame: `flip_test` = True is the reference's x4 self-ensemble (`flip_test` of
    test_Vid4_REDS4_with_GT.py, util.flipx4_forward; EDVR's published "with self-ensemble" numbers) -- the network runs on
    every window as it is, mirrored in W, in H and in both, and the un-flipped outputs are averaged, (((y0 + flipW(y1)) +
    flipH(y2)) + flipHW(y3)) / 4 in this order (frames.flip / frames.flip_mean, csrc/frame_flip.hip).  EDVR: the
    frame cache holds 4 x stream_slots slots, variant v (0 none, 1 W, 2 H, 3 both) of frame f in slot v * slots + f % slots;
    a frame is still extracted once per variant -- variant 0 by the call above, the others from frames.flip of the PADDED
    fp32 frame (the network sees flip(pad(x)): the padding stays at the bottom and right of the source) -- and a window runs
    four fuse tapes and one flip_mean that writes the tensor the single fuse tape writes otherwise, so crop, `out_size`,
    every `out` and `cuts` work as described.  Other networks: super_resolve_video(flip_test=True), which needs a (padded)
    width that is a multiple of 4.  False takes exactly the calls described above: no further plan, buffer or launch.  Not
    provided: the x8 ensemble with transposes (a transposed frame needs a second plan of W x H), and flip-test inside
    Video_base_model.test() or the adaptation loops.
    How good the frames are: `gt` is a video of T ground-truth frames of the OUTPUT's size (sH x sW, or `out_size`), a tensor or
    a list like `frames`, in any layout frames.score takes (`gt_layout`; None: by dtype), on the CPU or the GPU, and `scores` a
    float64 [T, 2] tensor on the GPU (required with `gt`).  Row i becomes [mse, ssim] of frames.score(yielded frame i, gt[i],
    channel=`score`, crop_border=`crop_border`) (csrc/frame_score.hip), launched on the window's stream behind the
    launch that produced the frame and ordered against the caller's stream exactly like the frame: what is scored is the frame
    the caller gets -- the bytes of a uint8 output, emit()'s 8-bit image of a 'float' one, the Y plane of a 4:2:0 output
    (`score` = 'y' alone; the 10- / 12-bit levels of a 16-bit one, against a GT of that depth).  A 4:2:0 output scored in 'y'
    against an RGB GT needs matrix='bt601', yuv_range='limited': the only pair for which the Y plane is the Y8 of the GT.
    score_summary turns `scores` into the reference's per-scene PSNR / SSIM means.  The yielded frames are what they are
    without `gt`; None takes exactly the calls described above.
    Frames too large for one plan: the kernels address one image of a tensor with 32-bit offsets, so an EDVR plan whose largest
    per-image tensor (engine.StreamPlan.max_image_bytes: 4096 h w bytes for nf = 64 at scale 4) reaches 2^32 -- 1080 x 1920 does
    -- is refused with a ValueError that names `tile`, and the workspace of a plan grows with its pixels.  `tile` = (th, tw), an
    int for both, or 'auto' (None: the whole frame, exactly the calls described above) cuts the padded frame into overlapping
    tiles of ONE size, th x tw LR pixels (multiples of 4 and of `multiple`, at least 16 and 2 * tile_overlap), tile_origins
    per axis with `tile_overlap` LR pixels (a multiple of 4; 16 is a policy default, not tuned on real footage) shared by
    neighbours; a tile >= the frame on both axes is the whole frame again.  The frame that goes into the crop / `out_size` /
    `out` / `gt` chain above is then frames.stitch (csrc/frame_stitch.hip) of, for every tile, what
    super_resolve_frames(..., out='float') gives for the video of that tile's view [y : min(y + th, h), x : min(x + tw, w)] of
    every frame (frames.tile_view; only a tile at the bottom or right edge is padded, from itself) -- a linear cross-fade over
    the overlaps.  It is NOT the whole-frame output: EDVR's receptive field is larger than any overlap.  EDVR: one plan of
    th x tw with n_tiles * nv * slots cache slots, tile t's variant v of frame f in slot (t * nv + v) * slots + f % slots; a CPU
    frame crosses the bus once and every tile view is extracted from it; a window runs the tiles' fuse tapes (and flip_mean per
    tile under flip_test) into a per-stream [n_tiles,3,s th,s tw] buffer and one stitch launch writes the tensor the single fuse
    tape writes otherwise, all on the window's stream.  Other networks: the tiles run as clips through super_resolve_video and
    are stitched on the caller's stream; with `tile` set `multiple` is raised to a multiple of 4.  'auto' is
    choose_tile(net, h, w, tile_budget, ...) (EDVR), `tile_budget` bytes or, None, 0.8 x the free device memory -- a policy value.
    Arguments are checked before the first GPU call (ValueError)."""
    a = _frame_arguments(opt, net, frames, padding, in_flight, layout, out, pad_mode, multiple, matrix, yuv_range, cuts,
                         cut_threshold, out_size, flip_test, gt, gt_layout, score, crop_border, scores, tile, tile_overlap,
                         tile_budget, siting)
    if a.is_edvr:
        yield from _stream_frames(net, frames, a)
    else:
        yield from _clip_frames(opt, net, frames, a)


def _frame_arguments(opt, net, frames, padding, in_flight, layout, out, pad_mode, multiple, matrix, yuv_range, cuts,
                     cut_threshold, out_size, flip_test, gt, gt_layout, score, crop_border, scores, tile, tile_overlap,
                     tile_budget, siting='left'):
    """The first stage of super_resolve_frames: its arguments checked and resolved into one record, which the two paths read.
    No GPU call, except for what cuts='auto' (frames.detect_cuts) and tile='auto' (the device's free memory) ask for, behind
    every check that can be made without them.  Fields beside the arguments themselves: T; is_edvr; lay, h, w, the frames'
    layout and size; Hp, Wp, the padded size (multiples of mult); out_fmt; out_size (None: the SR frame's own); sr_scale;
    n, the frames of a window; cuts (None, or the checked list); grid = (th, tw, the tiles' origins per axis) for more than one
    tile, else None; score_into (_frame_scoring); and `direct`: fp32 planar frames of the size the network takes in, its own
    tensor out -- nothing to convert, pad, crop or stitch, the calls of before the frame arguments."""
    from .models.archs.EDVR_arch import EDVR
    T = len(frames)
    if T < 1:
        raise ValueError("super_resolve_frames: no frames")
    _check_flip_test(flip_test, "super_resolve_frames")
    in_flight = max(1, int(in_flight))
    is_edvr = isinstance(net, EDVR)
    if pad_mode not in ('reflect', 'replicate'):
        raise ValueError("super_resolve_frames: pad_mode=%r ('reflect' or 'replicate')" % (pad_mode,))
    # float frames with none of the frame arguments given, at a size the network takes as it is: no per-frame check
    plain = layout is None and out is None and multiple is None and \
        torch.is_tensor(frames[0]) and frames[0].dtype not in (torch.uint8, torch.uint16, torch.int16)
    if is_edvr:
        plain = plain and torch.is_tensor(frames[0]) and frames[0].dim() == 3 and frames[0].is_floating_point() and \
            frames[0].shape[-2] % 4 == 0 and frames[0].shape[-1] % 4 == 0
    sr_scale = int(net.scale) if is_edvr else int(opt.get('scale') or 1)
    if out_size is not None:
        out_size = fio.check_size(out_size, "super_resolve_frames: out_size")
    tile, tile_overlap = _check_tile(tile, tile_overlap, tile_budget)
    if tile == 'auto' and not is_edvr:
        raise ValueError("super_resolve_frames: tile='auto' sizes an EDVR stream plan; pass (th, tw) for %s" % type(net).__name__)
    plain = plain and out_size is None and tile is None
    if plain:
        lay, h, w, out_fmt, mult = 'chw', int(frames[0].shape[-2]), int(frames[0].shape[-1]), 'float', None
        Hp, Wp = h, w
    else:
        lay, h, w, out_fmt, Hp, Wp, out_size, mult = _frame_format(
            "super_resolve_frames", frames, layout, out, multiple, pad_mode, matrix, yuv_range, out_size, sr_scale,
            4 if is_edvr else 1, 4 if is_edvr or tile is not None else 1, siting)
    score_into = _frame_scoring("super_resolve_frames", T, gt, gt_layout, scores, score, crop_border, out_fmt, out_size,
                                sr_scale, h, w, matrix, yuv_range)
    n = _window_length(opt, net)
    cuts = _resolve_cuts("super_resolve_frames", cuts, T, n, padding, frames, lay, cut_threshold)
    grid = None
    if tile is not None:
        if tile == 'auto':
            video_windows(T, n, padding, cuts)        # (the last check, in front of a query of the device's free memory)
            budget = tile_budget if tile_budget is not None else 0.8 * torch.cuda.mem_get_info(next(net.parameters()).device)[0]
            tile = choose_tile(net, h, w, budget, tile_overlap, in_flight, 1 if cuts is None else len(cuts) + 1, flip_test, mult)
        th, tw = min(tile[0], Hp), min(tile[1], Wp)
        if (th < Hp and th % mult) or (tw < Wp and tw % mult):
            raise ValueError("super_resolve_frames: tile=%r must be a multiple of multiple=%d" % (tuple(tile), mult))
        ys, xs = tile_origins(Hp, th, tile_overlap), tile_origins(Wp, tw, tile_overlap)
        if len(ys) * len(xs) > 1:
            grid = (th, tw, ys, xs)
            fio.check_pad(h - ys[-1], w - xs[-1], th, tw, pad_mode)     # the tile at the bottom right is padded from itself
    direct = plain or (grid is None and lay == 'chw' and _untouched((h, w, Hp, Wp), out_fmt, out_size))
    return SimpleNamespace(T=T, is_edvr=is_edvr, padding=padding, in_flight=in_flight, flip_test=flip_test, lay=lay, h=h, w=w,
                           Hp=Hp, Wp=Wp, mult=mult, pad_mode=pad_mode, matrix=matrix, yuv_range=yuv_range, siting=siting, out_fmt=out_fmt,
                           out_size=out_size, sr_scale=sr_scale, n=n, cuts=cuts, grid=grid, tile_overlap=tile_overlap,
                           score_into=score_into, direct=direct)


def _window_length(opt, net):
    """The frames of a window: the network's own count for EDVR, network_G.nframes of the options for any other network (the
    network's where they do not say)."""
    from .models.archs.EDVR_arch import EDVR
    if isinstance(net, EDVR) or not (opt.get('network_G') or {}).get('nframes'):
        return int(net.nframes)
    return int(opt['network_G']['nframes'])


def _resolve_cuts(who, cuts, T, n, padding, frames, lay, cut_threshold):
    """The `cuts` of the two frame generators as video_windows takes them: None, the checked sequence as a list, or for 'auto'
    frames.detect_cuts of the video -- a GPU call, so the padding mode is checked in front of it.  ValueError otherwise."""
    if isinstance(cuts, str):
        if cuts != 'auto':
            raise ValueError("%s: cuts=%r (None, 'auto' or a sequence of frame numbers)" % (who, cuts))
        video_windows(T, n, padding, [])                           # (the mode, before the first GPU call)
        return fio.detect_cuts(frames, lay, threshold=cut_threshold)
    if cuts is not None:
        return [a for a, _ in scene_bounds(T, cuts)][1:]
    return None


def _ingest_cache(make, capacity):
    """ingested(key) = make(key), the last `capacity` results kept: consecutive windows name a frame up to nframes times, and
    it is brought to the device / converted and padded once."""
    kept = {}

    def ingested(key):
        x = kept.get(key)
        if x is None:
            x = kept[key] = make(key)
            while len(kept) > capacity:
                kept.pop(next(iter(kept)))
        return x
    return ingested


def _clip_frames(opt, net, frames, a):
    """super_resolve_frames for a network without a frame cache (TOFlow, DUF): the windows are stacked into clips here -- of the
    frames as they are, of the ingested frames, or tile by tile -- and run by super_resolve_video; what follows a clip's
    output (stitch, crop, resize, conversion, score) runs on the caller's stream, which the outputs are ordered against."""
    windows, _ = video_windows(a.T, a.n, a.padding, a.cuts)        # (validates T, the mode and the cuts)
    if a.flip_test and a.Wp % 4:
        raise ValueError("super_resolve_frames: flip_test needs a width that is a multiple of 4, got %d (pass multiple=4)" % a.Wp)

    def run(clips):
        return super_resolve_video(opt, net, clips, a.in_flight, a.flip_test)

    def clips_of(frame, tiles=None):
        """One clip per window, the stack of frame(j) -- or, with `tiles`, one per window and tile, of frame((j, t))."""
        for win in windows:
            if tiles is None:
                yield torch.stack([frame(j) for j in win])[None]
            else:
                for t in range(tiles):
                    yield torch.stack([frame((j, t)) for j in win])[None]
    if a.direct:
        if a.score_into is None:
            yield from run(clips_of(lambda j: frames[j]))
            return
        for i, sr in enumerate(run(clips_of(lambda j: frames[j]))):
            a.score_into(i, sr)                        # (on the caller's stream, which the frame is ordered against)
            yield sr
        return

    def ingest(x):
        return fio.ingest(x, a.lay, a.mult, a.pad_mode, matrix=a.matrix, yuv_range=a.yuv_range, siting=a.siting)

    def finished(i, sr):
        return _finish_frame("super_resolve_frames", sr, (a.h, a.w, a.Hp, a.Wp), a.out_fmt, a.out_size, a.sr_scale, a.matrix,
                             a.yuv_range, i, a.score_into, siting=a.siting)
    if a.grid is None:
        ingested = _ingest_cache(lambda j: ingest(frames[j]), 2 * a.n)
        for i, sr in enumerate(run(clips_of(ingested))):
            yield finished(i, sr)
        return
    # every window as n_tiles clips, tile by tile; their outputs are copied into one buffer and stitched
    th, tw, ys, xs = a.grid
    origins = [(y, x) for y in ys for x in xs]
    first = frames[0] if torch.is_tensor(frames[0]) else frames[0][0]
    dev = first.device if first.is_cuda else torch.device('cuda', torch.cuda.current_device())
    on_device = _ingest_cache(lambda j: fio.to_device(frames[j], dev), 2 * a.n)       # (a CPU frame crosses the bus once)
    ingested = _ingest_cache(lambda jt: ingest(fio.tile_view(on_device(jt[0]), a.lay, origins[jt[1]][0], origins[jt[1]][1], th, tw)),
                             2 * a.n * len(origins))
    tiles_sr = run(clips_of(ingested, len(origins)))
    tables = None
    for i in range(a.T):
        buf = None
        for t in range(len(origins)):
            sr = next(tiles_sr)
            if buf is None:
                s = sr.shape[-2] // th
                if tuple(sr.shape) != (1, 3, s * th, s * tw) or s < 1:
                    raise RuntimeError("super_resolve_frames: a %d x %d tile came back as %s" % (th, tw, tuple(sr.shape)))
                buf = torch.empty((len(origins), 3, s * th, s * tw), dtype=torch.float32, device=sr.device)
                if tables is None:
                    tables = (fio.stitch_table(a.Hp, th, a.tile_overlap, s), fio.stitch_table(a.Wp, tw, a.tile_overlap, s))
            buf[t].copy_(sr[0])
        yield finished(i, fio.stitch(buf, len(ys), len(xs), tables[0], tables[1])[None])


class _CacheSlots:
    """The numbering of the EDVR frame cache and the events that order it.  Tile t's flip variant v of the frame in slot
    `slot` (= frame % slots) lives in cache slot (t * nv + v) * slots + slot; the n_tiles * nv copies of a slot are written by
    one frame's extraction and read by the same windows.  Two kinds of events: `extracted`, cache slot -> the event of its
    extraction, which the windows that gather it wait for; `readers`, cache slot -> the events of the windows reading it, which
    the extraction that overwrites it waits for."""

    def __init__(self, n_tiles, nv, slots):
        self.n_tiles, self.nv, self.slots = n_tiles, nv, slots
        self.extracted, self.readers = {}, {}

    def sid(self, t, v, slot):
        return (t * self.nv + v) * self.slots + slot

    def copies(self, slot):
        return [self.sid(t, v, slot) for t in range(self.n_tiles) for v in range(self.nv)]

    def wait_readers(self, stream, slot):
        for c in self.copies(slot):
            for ev in self.readers.pop(c, ()):
                stream.wait_event(ev)

    def mark_extracted(self, slot, ev):
        for c in self.copies(slot):
            self.extracted[c] = ev

    def wait_extracted(self, stream, wslots):
        for ev in set(self.extracted[c] for slot in set(wslots) for c in self.copies(slot)):
            stream.wait_event(ev)

    def mark_read(self, wslots, ev):
        for slot in set(wslots):
            for c in self.copies(slot):
                self.readers.setdefault(c, []).append(ev)


def _extract_frame(st, a, x, k, slot, s, main):
    """Frame x into cache slot `slot` of every tile and flip variant, on the current stream s (of index k): behind the windows
    that read what it overwrites, and with its event in `extracted`."""
    plan, ids, nv = st.plan, st.ids, st.ids.nv
    if a.direct:
        x = engine._prep(x if x.is_cuda else x.to(st.dev))
    else:
        x = fio.to_device(x, st.dev)                     # (8-bit frames travel as bytes)
    ids.wait_readers(s, slot)
    read = []                                            # the tensors the extraction launches read
    for t, (ty, tx) in enumerate(st.origins):
        xt = x if a.grid is None else fio.tile_view(x, a.lay, ty, tx, st.pth, st.ptw)
        if a.flip_test:                                  # the padded fp32 frame, then its mirror images one at a time
            flipped = _stream_buffer(st.flipped, k, lambda: [torch.empty((3, st.pth, st.ptw), dtype=torch.float32, device=st.dev)
                                                             for _ in range(2)])
            if a.direct:
                padded = xt if xt.data_ptr() % 16 == 0 else flipped[0].copy_(xt)
            else:
                padded = fio.ingest(xt, a.lay, a.mult, a.pad_mode, out=flipped[0], matrix=a.matrix, yuv_range=a.yuv_range,
                                    siting=a.siting)
        if a.direct:
            plan.extract(st.leaves, xt, ids.sid(t, 0, slot), st.cache)
        else:
            xt = plan.extract_frame(st.leaves, xt, ids.sid(t, 0, slot), st.cache, a.lay, a.pad_mode, a.matrix, a.yuv_range,
                                    a.siting)
        read += [xt] if torch.is_tensor(xt) else list(xt)
        for v in range(1, nv):
            plan.extract(st.leaves, fio.flip(padded, v, out=flipped[1]), ids.sid(t, v, slot), st.cache)
    ev = torch.cuda.Event()
    ev.record(s)
    ids.mark_extracted(slot, ev)
    if s != main:
        for t in read:
            t.record_stream(s)


def _fuse_tile(st, a, k, t, wslots, dst):
    """Tile t of the window in `wslots` -> dst [1,3,s pth,s ptw] on the current stream (of index k): the fuse tape, or, with
    flip_test, the four variants' fuse tapes and the launch that un-flips and averages them."""
    if not a.flip_test:
        st.plan.fuse(st.leaves, [st.ids.sid(t, 0, slot) for slot in wslots], st.cache, dst)
        return
    fused = _stream_buffer(st.fused, k, lambda: [torch.empty_like(dst) for _ in range(st.ids.nv)])
    for v in range(st.ids.nv):
        st.plan.fuse(st.leaves, [st.ids.sid(t, v, slot) for slot in wslots], st.cache, fused[v])
    fio.flip_mean(*fused, out=dst)


def _fuse(st, a, k, wslots, dst):
    """The window in `wslots` -> dst [1,3,s Hp,s Wp] on the current stream (of index k): _fuse_tile, or every tile's into the
    stream's tile buffer and the launch that stitches them."""
    if a.grid is None:
        _fuse_tile(st, a, k, 0, wslots, dst)
        return
    n_t = len(st.origins)
    tiled = _stream_buffer(st.tiled, k, lambda: torch.empty((n_t, 3, a.sr_scale * st.pth, a.sr_scale * st.ptw),
                                                            dtype=torch.float32, device=st.dev))
    for t in range(n_t):
        _fuse_tile(st, a, k, t, wslots, tiled[t:t + 1])
    fio._stitch_run(tiled, len(a.grid[2]), len(a.grid[3]), st.axes[0], st.axes[1], dst[0])


def _stream_frames(net, frames, a):
    """super_resolve_frames for EDVR: every frame's features extracted once into the frame cache (stream_schedule), a window =
    one gather + the tape from PCD alignment on, `in_flight` windows on the GPU at a time, one HIP stream each; a window's
    extractions, its fuse tapes and what follows them (flip_mean, stitch, crop, resize, conversion, score) run on its stream.
    Per-stream buffers: `staging`, the fuse tape's output when a crop / conversion follows it; `resized`, the resampled frame
    when a conversion follows it; flip_test: `flipped` [the padded frame, one mirror image of it] and `fused`, the four fuse
    tapes' outputs; tiles: `tiled`, the tiles' fuse outputs [n_t,3,s pth,s ptw]."""
    leaves = net.ordered_parameters()
    dev = leaves[0].device
    sched = list(stream_schedule(a.T, net.nframes, a.padding, a.in_flight, a.cuts))
    slots = stream_slots(net.nframes, a.in_flight, 1 if a.cuts is None else len(a.cuts) + 1)
    nv = 4 if a.flip_test else 1                      # variants of a frame in the cache
    # the tiles: one plan of the tile's size (the whole padded frame as the one tile without a grid)
    pth, ptw, origins = (a.Hp, a.Wp, [(0, 0)]) if a.grid is None else \
        (a.grid[0], a.grid[1], [(y, x) for y in a.grid[2] for x in a.grid[3]])
    plan = engine.get_stream_plan(net._cfg(), pth, ptw, len(origins) * nv * slots, dev)
    if plan.max_image_bytes >= MAX_IMAGE_BYTES:       # (a host query: before the device check and the first GPU call)
        raise ValueError("super_resolve_frames: a %d x %d %s needs a tensor of %d bytes per image, and the kernels address an image "
                         "with 32-bit offsets (< 2^32 bytes): pass tile= (a smaller tile, or 'auto') to run it in tiles"
                         % (pth, ptw, "frame" if a.grid is None else "tile", plan.max_image_bytes))
    if dev.type != 'cuda':
        raise RuntimeError("dynavsr_amd EDVR runs on the MI355X only (the network is on %s); there is no CPU fallback" % dev)
    if a.direct and tuple(frames[0].shape[-3:-2]) != (3,):
        raise RuntimeError("super_resolve_frames expects frames [3,H,W], got %s" % (tuple(frames[0].shape),))
    main = torch.cuda.current_stream(dev)
    streams = _clip_streams(dev, a.in_flight)
    with torch.cuda.device(dev):
        cache = plan.new_cache(dev)
    for s in streams[1:]:
        cache.record_stream(s)
    st = SimpleNamespace(plan=plan, cache=cache, leaves=leaves, dev=dev, ids=_CacheSlots(len(origins), nv, slots), pth=pth, ptw=ptw,
                         origins=origins, axes=None, staging={}, resized={}, flipped={}, fused={}, tiled={})
    if a.grid is not None:
        with torch.cuda.device(dev):               # the blend tables of the two axes, on the device once per video
            st.axes = [fio._stitch_axis(fio.stitch_table(nn, tt, a.tile_overlap, a.sr_scale), dev)
                       for nn, tt in ((a.Hp, pth), (a.Wp, ptw))]
    geometry, pending = (a.h, a.w, a.Hp, a.Wp), []

    def frame_tensor():
        return torch.empty((1, 3, a.sr_scale * a.Hp, a.sr_scale * a.Wp), dtype=torch.float32, device=dev)
    was_training = net.training
    net.eval()
    try:
        for step, (centre, _, new, wslots) in enumerate(sched):
            yield from _hand_out(pending, main, len(streams) - 1)
            k = step % len(streams)
            s = streams[k]
            if s != main:
                s.wait_stream(main)                  # the frames (and the weights) were produced on the caller's stream
            with torch.cuda.stream(s), torch.no_grad():
                for f, slot in new:
                    _extract_frame(st, a, frames[f], k, slot, s, main)
                st.ids.wait_extracted(s, wslots)
                untouched = _untouched(geometry, a.out_fmt, a.out_size)
                dst = frame_tensor() if untouched else _stream_buffer(st.staging, k, frame_tensor)
                _fuse(st, a, k, wslots, dst)
                buf = None
                if a.out_size is not None and a.out_fmt != 'float':
                    buf = _stream_buffer(st.resized, k, lambda: fio.resize_buffer(a.out_size, dev))
                # (the score: behind the launch that wrote sr; the event below covers the row too)
                sr = _finish_frame("super_resolve_frames", dst, geometry, a.out_fmt, a.out_size, a.sr_scale, a.matrix,
                                   a.yuv_range, centre, a.score_into, resized=buf, siting=a.siting)
                ev = torch.cuda.Event()
                ev.record(s)
            st.ids.mark_read(wslots, ev)
            pending.append((sr, ev))
        yield from _hand_out(pending, main)
    finally:
        # a generator closed early leaves windows running on the side streams: whatever the caller does next on its stream
        # (an update of the weights they read, the release of the cache) must come behind them
        for _ in _hand_out(pending, main):
            pass
        net.train(was_training)


def score_summary(scores, nframes, cuts=None, peak=255):
    """The reference's per-folder report (test_Vid4_REDS4_with_GT.py) from the [T, 2] rows [mse, ssim] that
    super_resolve_frames(gt=...) wrote: one device-to-host copy, then host arithmetic.

    A scene (scene_bounds(T, cuts); cuts=None: the whole video) plays the part of a folder.  With border_frame = nframes // 2,
    frame i of a scene of N frames is a centre frame when border_frame <= i < N - border_frame and a border frame otherwise.
    Per scene: 'psnr' / 'ssim' are the means of the per-frame values over all frames, '_center' / '_border' those over the two
    groups; a border mean over no frames is 0, like the reference, and a centre mean over no frames (a scene shorter than
    2 * border_frame, where the reference would divide by zero) is NaN.  The per-frame PSNR is frames.psnr(mse, peak): inf for
    identical frames.  Returns {'scenes': [{'first', 'frames', 'center_frames', 'border_frames', 'psnr', 'psnr_center',
    'psnr_border', 'ssim', 'ssim_center', 'ssim_border'}, ...], 'mean': the plain mean over scenes of the six values}."""
    rows = torch.as_tensor(scores).detach().to('cpu', torch.float64)
    if rows.dim() != 2 or rows.shape[1] != 2 or rows.shape[0] < 1:
        raise ValueError("score_summary: scores must be [T, 2], got %s" % (tuple(rows.shape),))
    nframes = int(nframes)
    if nframes < 1:
        raise ValueError("score_summary: nframes=%d must be positive" % nframes)
    rows = rows.tolist()
    border = nframes // 2

    def mean(v, empty):
        return sum(v) / len(v) if v else empty
    keys = ('psnr', 'psnr_center', 'psnr_border', 'ssim', 'ssim_center', 'ssim_border')
    scenes = []
    for a, b in scene_bounds(len(rows), [] if cuts is None else cuts):
        p = [fio.psnr(m, peak) for m, _ in rows[a:b]]
        s = [v for _, v in rows[a:b]]
        centre = [border <= i < (b - a) - border for i in range(b - a)]
        pc, pb = [v for v, c in zip(p, centre) if c], [v for v, c in zip(p, centre) if not c]
        sc, sb = [v for v, c in zip(s, centre) if c], [v for v, c in zip(s, centre) if not c]
        scenes.append({'first': a, 'frames': b - a, 'center_frames': len(pc), 'border_frames': len(pb),
                       'psnr': mean(p, 0.0), 'psnr_center': mean(pc, float('nan')), 'psnr_border': mean(pb, 0.0),
                       'ssim': mean(s, 0.0), 'ssim_center': mean(sc, float('nan')), 'ssim_border': mean(sb, 0.0)})
    return {'scenes': scenes, 'mean': {k: sum(sc[k] for sc in scenes) / len(scenes) for k in keys}}


def evaluate_frames(opt, net, frames, gt, **kw):
    """Drains super_resolve_frames(opt, net, frames, gt=gt, **kw) and returns (score_summary(scores, nframes, cuts, peak),
    scores): the evaluation scripts of the reference for one video.  `scores` (a float64 [T, 2] GPU tensor) is allocated on the
    network's device unless passed; cuts='auto' is resolved here, so that the summary has the scenes the windows had; `peak`
    (None: 255, or 2^d - 1 for a 10- / 12-bit output) goes to score_summary."""
    kw = dict(kw)
    peak = kw.pop('peak', None)
    T = len(frames)
    if isinstance(kw.get('cuts'), str) and kw['cuts'] == 'auto':
        kw['cuts'] = fio.detect_cuts(frames, kw.get('layout'), threshold=kw.get('cut_threshold', 10.0))
    if kw.get('scores') is None:
        p = next(iter(net.parameters()), None)
        dev = p.device if p is not None and p.is_cuda else torch.device('cuda', torch.cuda.current_device())
        kw['scores'] = torch.zeros((T, 2), dtype=torch.float64, device=dev)
    scores = kw['scores']
    for _ in super_resolve_frames(opt, net, frames, gt=gt, **kw):
        pass
    if peak is None:
        o = kw.get('out') if kw.get('out') is not None else kw.get('layout')
        peak = _peak(o, kw.get('gt_layout'))
    return score_summary(scores, _window_length(opt, net), kw.get('cuts'), peak), scores


def _degraded_geometry(who, hr, degradation, layout):
    """The host checks of degrade_frames: (lay, h, w, per_frame, K, scale, (Hc, Wc, h_lr, w_lr)).  ValueError for a video that
    _video_format refuses, a kernel set whose length is not the video's or whose shifted kernels differ in size, and everything
    frames.degraded_size refuses.  No GPU call."""
    lay, h, w = _video_format(hr, layout, who)
    if isinstance(degradation, fio.Imresize):                # BI: no kernel, the LR size is the crop's over the scale
        try:
            return lay, h, w, False, 0, degradation.scale, degradation.lr_size(h, w)
        except ValueError as e:
            raise ValueError("%s: %s" % (who, e))
    kernel = getattr(degradation, 'kernel', None)
    if kernel is None or getattr(kernel, 'ndim', 0) not in (2, 3):
        raise ValueError("%s: degradation must be a frames.Imresize or a data.random_kernel_generator.Degradation with a [K0,K0] "
                         "or [T,K0,K0] kernel" % who)
    per_frame = kernel.ndim == 3
    if per_frame and kernel.shape[0] != len(hr):
        raise ValueError("%s: %d per-frame kernels for a video of %d frames (frame j takes kernel j)" % (who, kernel.shape[0], len(hr)))
    edges = sorted(set(fio.degradation_edge(degradation, j, who)[0] for j in range(kernel.shape[0] if per_frame else 1)))
    if len(edges) != 1:
        raise ValueError("%s: the shifted per-frame kernels have edges %s; one LR size needs one edge" % (who, edges))
    K, scale = edges[0], int(degradation.scale)
    try:
        sizes = fio.degraded_size(h, w, K, scale)
    except ValueError as e:
        raise ValueError("%s: %s" % (who, e))
    return lay, h, w, per_frame, K, scale, sizes


def degrade_frames(hr, degradation, *, layout=None, quantise=True, matrix='bt601', yuv_range='limited', out=None, siting='left'):
    """A ground-truth video -> its LR video, fp32 [T,3,h_lr,w_lr] on the GPU: what super_resolve_frames / adapt_frames take.

    hr: a [T,...] tensor or a list of frames of one kind and size, in any `layout` frames.ingest takes (None: by dtype; the
    YCbCr layouts are never inferred), on the CPU or the GPU.  Frame j becomes frames.degrade(hr[j], degradation, layout,
    quantise=quantise): its top-left (h - h % scale) x (w - w % scale) crop blurred and sub-sampled with the degradation's
    shifted kernel and, with `quantise`, rounded to the 8-bit grid -- test_dynavsr.py's `degradation_mode: set` on a video that is
    never held as fp32 at HR size.  One launch per frame on the caller's stream; a CPU frame crosses the bus once, as bytes.
    `degradation` may also be a frames.Imresize(s) -- BI, MATLAB's imresize(hr, 1 / s) of the crop, Hc / s x Wc / s -- or a
    data.old_kernel_generator.Degradation, the YAMLs' `degradation_type: bicubic` (its kernel is applied as it is).  The
    reference's scripts build LR folders as a cascade of x2 applications with the 8-bit round trip between them: that is
    degrade_frames called on its own output.
    A [T,K0,K0] degradation.kernel needs T == len(hr), and frame j is degraded with kernel j.  That is NOT the reference's
    `preset` mode, which degrades a whole window of frames with the centre frame's kernel, so that one frame appears with up to
    nframes different blurs: here a frame is degraded once.
    out: the fp32 [T,3,h_lr,w_lr] GPU tensor to fill.  Arguments are checked before the first GPU call (ValueError)."""
    who = "degrade_frames"
    fio.check_yuv_names(matrix, yuv_range, siting)
    lay, h, w, per_frame, K, scale, (Hc, Wc, hl, wl) = _degraded_geometry(who, hr, degradation, layout)
    T = len(hr)
    if out is not None:
        if not (torch.is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == (T, 3, hl, wl)):
            raise ValueError("%s: out must be an fp32 [%d,3,%d,%d] tensor" % (who, T, hl, wl))
        if not out.is_cuda:
            raise RuntimeError("%s: out must be on the GPU (libdynavsr_hip); there is no CPU path" % who)
    first = hr[0] if torch.is_tensor(hr[0]) else hr[0][0]
    dev = out.device if out is not None else (first.device if first.is_cuda else torch.device('cuda', torch.cuda.current_device()))
    with torch.cuda.device(dev):
        lr = out if out is not None else torch.empty((T, 3, hl, wl), dtype=torch.float32, device=dev)
        for j in range(T):
            fio.degrade(hr[j], degradation, lay, kernel_index=j if per_frame else 0, quantise=quantise, out=lr[j], matrix=matrix,
                        yuv_range=yuv_range, siting=siting)
    return lr


def _degraded_evaluation(who, opt, hr, degradation, hr_layout, kw):
    """The checks that the two evaluate_degraded functions share, and the ground truth: (lay, (T, 3, h_lr, w_lr), gt) -- gt the
    top-left Hc x Wc view of every HR frame (frames.tile_view: plane views for YCbCr, nothing copied).  ValueError when the SR
    frames would not have the ground truth's size (an even shifted kernel: scale * h_lr != Hc), when the degradation's scale is
    not the network's, and for arguments that belong to the functions' own part.  No GPU call."""
    lay, h, w, _, K, scale, (Hc, Wc, hl, wl) = _degraded_geometry(who, hr, degradation, hr_layout)
    for name in ('gt', 'gt_layout', 'layout'):
        if name in kw:
            raise ValueError("%s: %s is the function's own (the LR video is fp32 planar, the ground truth the HR video)" % (who, name))
    if scale != int(opt['scale']):
        raise ValueError("%s: the degradation's scale %d is not opt['scale'] = %r" % (who, scale, opt['scale']))
    if scale * hl != Hc or scale * wl != Wc:
        raise ValueError("%s: an even shifted kernel (edge %d) gives LR frames of %d x %d, whose SR frames %d x %d are not the "
                         "%d x %d of the ground truth; use an odd kernel_size" % (who, K, hl, wl, scale * hl, scale * wl, Hc, Wc))
    gt = [fio.tile_view(f, lay, 0, 0, Hc, Wc) for f in hr]
    return lay, (len(hr), 3, hl, wl), gt


def _without_device_queries(kw):
    """`kw` of a frame generator for a check ahead of its call: cuts='auto' and tile='auto' ask the device, so the check takes one
    scene and no tile in their place (what the generators check in front of those queries)."""
    kw = dict(kw)
    if isinstance(kw.get('cuts'), str) and kw['cuts'] == 'auto':
        kw['cuts'] = []
    if isinstance(kw.get('tile'), str) and kw['tile'] == 'auto':
        kw.pop('tile')
        kw.pop('tile_budget', None)
    return kw


def evaluate_degraded(opt, net, hr, degradation, *, hr_layout=None, quantise=True, **kw):
    """"This ground-truth video, this blur: how good is the network?" in one call -- the un-adapted half of test_dynavsr.py with
    `degradation_mode: set`.  The LR video is degrade_frames(hr, degradation, layout=hr_layout, quantise=quantise, matrix=,
    yuv_range=), the ground truth the top-left Hc x Wc view of every HR frame (what the LR frames were made from; frames.tile_view,
    nothing copied), and the result is evaluate_frames(opt, net, lr, gt, gt_layout=hr_layout, **kw): (summary, scores).
    `kw` is evaluate_frames' (out, cuts -- 'auto' is resolved on the LR video --, score, crop_border, scores, peak, tile, ...;
    `matrix` / `yuv_range` name the conversion of a YCbCr `hr` and of a YCbCr `out` alike).
    ValueError before the first GPU call: degradation.scale != opt['scale']; scale * h_lr != Hc (an even shifted kernel: the SR
    frames would not have the ground truth's size); per-frame kernels of another count than the video; an HR frame not larger
    than the kernel's pad; `gt`, `gt_layout` or `layout` in kw; and what super_resolve_frames refuses for these arguments."""
    import inspect
    who = "evaluate_degraded"
    lay, shape, gt = _degraded_evaluation(who, opt, hr, degradation, hr_layout, kw)
    stand_in = torch.empty(shape, dtype=torch.float32, device='meta')       # the LR video's size and kind, for the checks alone
    check = {k: v for k, v in _without_device_queries(kw).items() if k != 'peak'}
    check['scores'] = check['scores'] if check.get('scores') is not None else _SCORES_LATER
    defaults = {k: p.default for k, p in inspect.signature(super_resolve_frames).parameters.items()
                if p.default is not inspect.Parameter.empty}
    unknown = sorted(set(check) - set(defaults))
    if unknown:
        raise TypeError("evaluate_degraded: super_resolve_frames takes no %s" % ', '.join(unknown))
    b = dict(defaults, gt=gt, gt_layout=lay, **check)
    a = _frame_arguments(opt, net, stand_in, *[b[k] for k in list(inspect.signature(_frame_arguments).parameters)[3:]])
    video_windows(a.T, a.n, a.padding, a.cuts)              # (the padding mode and the window length, which the paths check later)
    lr = degrade_frames(hr, degradation, layout=lay, quantise=quantise, matrix=kw.get('matrix', 'bt601'),
                        yuv_range=kw.get('yuv_range', 'limited'), siting=kw.get('siting', 'left'))
    return evaluate_frames(opt, net, lr, gt, gt_layout=lay, **kw)


def evaluate_bicubic(opt, net, frames, gt, *, layout=None, out=None, matrix='bt601', yuv_range='limited', cuts=None,
                     cut_threshold=10.0, gt_layout=None, score='rgb', crop_border=0, scores=None, peak=None, siting='left'):
    """The "Bicubic" row of an SR table for one video: frame i is frames.imresize(frames[i], opt['scale'], layout) -- MATLAB's
    imresize(lr, s) on the device -- in place of the network's output, then converted to `out` and scored against gt[i] exactly
    as evaluate_frames does it, so that the two summaries compare row for row: (score_summary(scores, nframes, cuts, peak),
    scores).  `net` only supplies the window length, for the border / centre split of the summary.  `frames` is what
    super_resolve_frames takes (any size: nothing is padded); `out`, `cuts` ('auto' included), `gt_layout`, `score`,
    `crop_border`, `scores` and `peak` are evaluate_frames'.  Arguments are checked before the first GPU call (ValueError)."""
    who = "evaluate_bicubic"
    T = len(frames)
    if T < 1:
        raise ValueError("%s: no frames" % who)
    try:
        s = fio.imresize_ratio(int(opt['scale']), who)[0]
    except (TypeError, KeyError):
        raise ValueError("%s: opt['scale'] must be 2, 3 or 4" % who)
    lay, h, w = _video_format(frames, layout, who)
    if out not in (None, 'float', 'hwc_rgb', 'hwc_bgr') + fio.RGB_LAYOUTS and not fio.is_yuv(out):
        raise ValueError("%s: out=%r (None, 'float', 'hwc_rgb', 'hwc_bgr' or one of %s)" % (
            who, out, ', '.join(fio.RGB_LAYOUTS + fio.ALL_YUV_LAYOUTS)))
    fio.check_yuv_names(matrix, yuv_range, siting)
    out_fmt = out if out is not None else ('float' if lay == 'chw' else lay)
    if fio.is_yuv(out_fmt) and fio.packed_needs(out_fmt, s * h, s * w):
        raise ValueError("%s: a packed %s output of %d x %d needs %s" % (who, out_fmt, s * h, s * w,
                                                                       fio.packed_needs(out_fmt, s * h, s * w)))
    score_into = _frame_scoring(who, T, gt, gt_layout, _SCORES_LATER if scores is None else scores, score, crop_border, out_fmt,
                                None, s, h, w, matrix, yuv_range)
    if score_into is None:
        raise ValueError("%s: gt is what the frames are scored against" % who)
    n = _window_length(opt, net)
    cuts = _resolve_cuts(who, cuts, T, n, 'replicate', frames, lay, cut_threshold)
    first = frames[0] if torch.is_tensor(frames[0]) else frames[0][0]
    dev = scores.device if scores is not None else (first.device if first.is_cuda else torch.device('cuda', torch.cuda.current_device()))
    with torch.cuda.device(dev):
        if scores is None:
            scores = torch.zeros((T, 2), dtype=torch.float64, device=dev)
        for i in range(T):
            sr = fio.imresize(frames[i], (s, 1), lay, matrix=matrix, yuv_range=yuv_range, siting=siting)[None]
            _finish_frame(who, sr, (s * h, s * w, s * h, s * w), out_fmt, None, 1, matrix, yuv_range, i, score_into, scores,
                          siting=siting)
    if peak is None:
        peak = _peak(out_fmt, gt_layout)
    return score_summary(scores, n, cuts, peak), scores
