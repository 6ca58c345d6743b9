"""Meta-training tasks made on the device from a pool of HR frames.

The reference makes one task per ``VSRBase.__getitem__`` (codes/data/meta_learner/vsrbase.py:135-198) in a DataLoader worker on
the CPU: it reads N frames, crops them at one position (``np_common_crop``, preprocessing.py:87-115), draws one blur kernel
(``set_kernel_params``, :39-49), applies ``Degradation.apply`` twice (HR -> LR, quantised to 8 bits, LR -> SLR; vsrbase.py:184-189)
and flips the three clips alike (``augment``, preprocessing.py:209-237).  Here the HR video lives on the device as the bytes it
was decoded to (``FramePool``), the host draws what the reference draws in the reference's order (``SequenceIndex``,
``draw_task``), and a whole batch of tasks is cut, blurred, sub-sampled, quantised, blurred again and flipped in FOUR launches
(``make_batch``: dvsr_task_degrade twice, dvsr_task_gather twice), bit-identical to the per-frame composition of
``frames.degrade`` / ``Degradation.apply`` / ``frames.ingest`` / ``torch.flip``.  ``TaskSource`` is the iterable that feeds
``adapt.meta_train_step``.

Everything here is a restatement of behaviour written for this project; the reference is cited by file and line.  Not provided:
file decoding (the caller's), Vimeo's septuplet layout, the wavelet-guided ``preprocessing.crop``, per-frame kernels inside a
task, a pool that does not fit the device."""
import ctypes
import math
import numbers
import functools
import random

import numpy as np
import torch

from dynavsr_amd import _lib as L
from dynavsr_amd.data.random_kernel_generator import Degradation

MAX_K, MAX_SCALE = 33, 4            # the limits of the degrade kernels (csrc/degrade.hip)
ITEM = np.dtype([("src", "<u8"), ("row_stride", "<i8"), ("plane_stride", "<i8"), ("kernel", "<i4"), ("flags", "<i4")])
assert ITEM.itemsize == ctypes.sizeof(L.TaskFrame) == 32
_FORMAT = {"chw": L.FRAME_F32_CHW, "hwc_rgb": L.FRAME_U8_HWC_RGB, "hwc_bgr": L.FRAME_U8_HWC_BGR}


class SequenceIndex:
    """The sample counting of ``VSRBase.__init__`` (vsrbase.py:66-87) and the lookup of ``find_set`` (:107-133) and
    ``__getitem__`` (:140-151), over sequence lengths instead of file lists.

    lengths: {name: number of frames} (insertion order is kept for ``sampling_weights``, as the reference's ``dict_hr``; ``find``
    walks the names sorted, as ``self.keys``).  interval_list: one stride or a list; a negative stride reads backwards.  A
    stride s makes samples of ``(n_frames - 1) |s| + 1`` frames; for every offset o below that length a sequence of T frames
    holds ``(T - o) // length`` of them (the reference's floor division, which is what this keeps)."""

    def __init__(self, lengths, n_frames, interval_list):
        self.lengths = {str(k): int(v) for k, v in dict(lengths).items()}
        self.keys = sorted(self.lengths)
        self.n_frames = int(n_frames)
        self.stride = [int(s) for s in (interval_list if isinstance(interval_list, (tuple, list)) else [interval_list])]
        if self.n_frames < 1 or not self.stride or any(s == 0 for s in self.stride):
            raise ValueError("SequenceIndex: n_frames=%r, interval_list=%r" % (n_frames, interval_list))
        self.sample_length = [(self.n_frames - 1) * abs(s) + 1 for s in self.stride]
        self.len_dict = {k: [[(t - o) // sl for o in range(sl)] for sl in self.sample_length] for k, t in self.lengths.items()}
        self.weighted_sample = [sum(sum(y) for y in x) for x in self.len_dict.values()]
        self.n_samples = sum(self.weighted_sample)

    def __len__(self):
        return self.n_samples

    def sampling_weights(self):
        """vsrbase.py:89-90: 1 / (samples of the sequence), in the order the sequences were given."""
        return [1 / x for x in self.weighted_sample]

    def find_set(self, idx):
        """(key, stride_index, seq_idx) of sample idx: find_set's walk, statement for statement."""
        if not 0 <= idx < self.n_samples:
            raise IndexError("sample %r outside [0, %d)" % (idx, self.n_samples))
        for k in self.keys:
            len_list = [sum(b) for b in self.len_dict[k]]
            set_length = sum(len_list)
            if idx >= set_length:
                idx -= set_length
                continue
            for str_idx, offset_list in enumerate(self.len_dict[k]):
                if idx >= len_list[str_idx]:
                    idx -= len_list[str_idx]
                    continue
                sl = self.sample_length[str_idx]
                for len_idx, length in enumerate(offset_list):
                    if idx < length:
                        seq_idx = len_idx + idx * sl + (0 if self.stride[str_idx] > 0 else sl - 1)
                        return k, str_idx, seq_idx
                    idx -= length
        raise IndexError("sample not found")                                # (negative counts of a very short sequence)

    def find(self, idx):
        """(key, stride_index, frame_indices) of sample idx: the slice of __getitem__ (vsrbase.py:143-151) on range(T)."""
        key, str_idx, seq_idx = self.find_set(int(idx))
        s, sl = self.stride[str_idx], self.sample_length[str_idx]
        seq_end = seq_idx + sl if s > 0 else seq_idx - sl
        frames = range(self.lengths[key])
        picked = frames[seq_idx:seq_end:s] if seq_end >= 0 else frames[seq_idx::s]
        return key, str_idx, list(picked)


def draw_task(py_rng, np_rng, h, w, crop, augment=True, rot=False, full_width=False):
    """The random draws of one ``__getitem__`` on h x w frames, in its statement order, from a ``random.Random`` and a
    ``numpy.random.RandomState`` that stand for the reference's global generators:

    1. ``py``, ``px`` from ``randrange`` (np_common_crop, preprocessing.py:106-107);
    2. ``sigma_x``, ``sigma_y``, ``theta`` from three ``random_sample()`` (set_kernel_params, :43-47): 0.2 + 4.8 u, -pi + 2 pi u;
    3. ``hflip``, ``vflip`` from ``random() < 0.5`` (augment, :215-216), only with ``augment`` (vsrbase.py:190: training);
    4. a ``rot`` draw only when ``rot`` is asked for -- the reference's ``and`` short-circuits (:217), and vsrbase.py:192 never asks.

    A QUIRK, kept by default: np_common_crop takes ``min_w`` from ``shape[0]`` (preprocessing.py:103-104), so ``px`` is drawn from
    [0, h - crop]; on 720 x 1280 frames the right 560 columns are never cut.  ``full_width=True`` draws ``px`` from the width.
    ValueError for a crop larger than the frame (or, under the quirk, a frame higher than wide, whose crops the reference
    silently truncates).  Returns a dict of the draws plus ``crop``."""
    h, w, crop = int(h), int(w), int(crop)
    if crop < 1 or crop > h or crop > w:
        raise ValueError("draw_task: a crop of %d is larger than a %d x %d frame" % (crop, h, w))
    if not full_width and h > w:
        raise ValueError("draw_task: px is drawn from the height (the reference's quirk), which on a %d x %d frame leaves the "
                         "frame; use full_width=True" % (h, w))
    py = py_rng.randrange(0, h - crop + 1)
    px = py_rng.randrange(0, (w if full_width else h) - crop + 1)
    sigma_x = 0.2 + np_rng.random_sample() * 4.8
    sigma_y = 0.2 + np_rng.random_sample() * 4.8
    theta = -math.pi + np_rng.random_sample() * 2 * math.pi
    hflip = vflip = False
    if augment:
        hflip = py_rng.random() < 0.5
        vflip = py_rng.random() < 0.5
        rot = bool(rot) and py_rng.random() < 0.5
    else:
        rot = False
    return {"py": py, "px": px, "sigma_x": sigma_x, "sigma_y": sigma_y, "theta": theta, "hflip": hflip, "vflip": vflip,
            "rot": rot, "crop": crop}


def draw_flags(draw):
    """The store flags of a draw: hflip mirrors W (x[..., ::-1]), vflip mirrors H, rot is the permute (preprocessing.py:220-233)."""
    return (L.FLIP_W if draw["hflip"] else 0) | (L.FLIP_H if draw["vflip"] else 0) | (L.TASK_TRANSPOSE if draw["rot"] else 0)


@functools.lru_cache(maxsize=None)
def nominal_edge(kernel_size, scale):
    """K of a symmetric kernel of that size after kernel_shift: what the size checks ahead of the first draw use."""
    return Degradation(int(kernel_size), int(scale)).shifted_edge()


def lr_size(n, K, scale):
    return (n + 2 * (K // 2) - K) // scale + 1


def check_geometry(crop, K, scale, who="make_batch"):
    """ValueError for what the two applications cannot do on a crop x crop patch; returns (h, hs), the LR and SLR edges."""
    if not (1 <= K <= MAX_K and 1 <= scale <= MAX_SCALE):
        raise ValueError("%s: kernel edge %d (1 .. %d) / scale %d (1 .. %d)" % (who, K, MAX_K, scale, MAX_SCALE))
    if K // 2 >= crop:
        raise ValueError("%s: the reflection pad %d is not smaller than the %d x %d crop" % (who, K // 2, crop, crop))
    h = lr_size(crop, K, scale)
    if K // 2 >= h:
        raise ValueError("%s: the reflection pad %d is not smaller than the %d x %d LR patch: the second application has nothing "
                         "to reflect" % (who, K // 2, h, h))
    return h, lr_size(h, K, scale)


class FramePool:
    """HR sequences on the device, kept as they came: {name: uint8 [T,H,W,3|4] ('hwc_rgb', the default, or 'hwc_bgr') or
    float32 [T,3,H,W] ('chw')}, torch tensors or numpy arrays.  Every sequence is brought to the device once (as bytes, for
    bytes) and made contiguous; all share a dtype and a pixel stride, their sizes may differ.  No file is read here."""

    def __init__(self, sequences, layout=None, device=None):
        if not sequences:
            raise ValueError("FramePool: no sequences")
        first = next(iter(dict(sequences).values()))
        first = torch.from_numpy(first) if isinstance(first, np.ndarray) else first
        if not torch.is_tensor(first):
            raise ValueError("FramePool: a sequence must be a tensor or an array, got %s" % type(first).__name__)
        u8 = first.dtype == torch.uint8
        if layout is None:
            layout = "hwc_rgb" if u8 else "chw"
        if layout not in _FORMAT or (layout == "chw") == u8 or not (u8 or first.dtype == torch.float32):
            raise ValueError("FramePool: layout %r of %s sequences (uint8: 'hwc_rgb' / 'hwc_bgr'; float32: 'chw')" % (layout, first.dtype))
        self.layout, self.format = layout, _FORMAT[layout]
        self.pixel_stride = int(first.shape[-1]) if u8 else 1
        checked = {}
        for name, seq in dict(sequences).items():
            seq = torch.from_numpy(seq) if isinstance(seq, np.ndarray) else seq
            ok = torch.is_tensor(seq) and seq.dtype == first.dtype and seq.dim() == 4 and seq.shape[0] >= 1
            ok = ok and (seq.shape[3] == self.pixel_stride and self.pixel_stride in (3, 4) if u8 else seq.shape[1] == 3)
            if not ok:
                raise ValueError("FramePool: sequence %r is %s; want %s" % (
                    name, tuple(seq.shape) if torch.is_tensor(seq) else type(seq).__name__,
                    "uint8 [T,H,W,%d]" % self.pixel_stride if u8 else "float32 [T,3,H,W]"))
            checked[str(name)] = seq
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.sequences = {k: v.to(self.device).contiguous() for k, v in checked.items()}
        self.lengths = {k: int(v.shape[0]) for k, v in self.sequences.items()}
        self.nbytes = sum(v.numel() * v.element_size() for v in self.sequences.values())

    def size(self, key):
        s = self.sequences[key].shape
        return (int(s[1]), int(s[2])) if self.layout != "chw" else (int(s[2]), int(s[3]))

    def crop_item(self, key, frame, py, px):
        """(src, row_stride, plane_stride) of the crop at (py, px) of one frame, as a dvsr_task_frame has them."""
        t = self.sequences[key]
        h, w = self.size(key)
        if self.layout == "chw":
            return t.data_ptr() + 4 * (frame * 3 * h * w + py * w + px), w, h * w
        ps = self.pixel_stride
        return t.data_ptr() + frame * h * w * ps + py * w * ps + px * ps, w * ps, 0

    def view(self, key, frame, py, px, crop):
        """The same crop as a tensor view (what frames.ingest / frames.degrade take)."""
        t = self.sequences[key][frame]
        return t[:, py:py + crop, px:px + crop] if self.layout == "chw" else t[py:py + crop, px:px + crop]


def table_bytes(n_items, n_tasks):
    """Bytes of one upload: three tables of n_items rows and n_tasks kernels of the largest edge."""
    return 3 * n_items * ITEM.itemsize + n_tasks * MAX_K * MAX_K * 4


class Staging:
    """One upload buffer: pinned host bytes, the device bytes they are copied to, and the event behind that copy."""

    def __init__(self, nbytes, device):
        self.host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        self.dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.event = None

    def wait(self):
        if self.event is not None:
            self.event.synchronize()

    def upload(self, nbytes):
        self.dev[:nbytes].copy_(self.host[:nbytes], non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()


def shifted_kernels(draws, kernel_size, scale):
    """[B,K,K] float32: one Degradation per task builds and shifts its kernel on the host (scipy, as Degradation.apply does).
    kernel_shift's zero padding hangs on ceil(max(shift)); where rounding noise makes it differ inside a batch (scale 3: a shift
    of 1.0), the smaller kernels are zero-padded on every side to the largest edge, which changes neither the taps that count nor
    the output size (both edges are odd or both even).  The bit contract of make_batch is against this padded kernel."""
    ks = []
    for d in draws:
        g = Degradation(int(kernel_size), int(scale), theta=d["theta"], sigma=[d["sigma_x"], d["sigma_y"]])
        ks.append(np.asarray(g.kernel_shift(g.kernel), dtype=np.float64))
    K = max(k.shape[0] for k in ks)
    return np.stack([np.pad(k, (K - k.shape[0]) // 2, "constant") for k in ks]).astype(np.float32)


def _check_out(out, name, shape, device):
    t = out.get(name) if out else None
    if t is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if not (torch.is_tensor(t) and t.dtype == torch.float32 and tuple(t.shape) == tuple(shape) and t.is_contiguous()):
        raise ValueError("make_batch: out[%r] must be a contiguous fp32 %s tensor" % (name, tuple(shape)))
    if not t.is_cuda:
        raise RuntimeError("make_batch: out[%r] must be on the GPU (libdynavsr_hip); there is no CPU path" % name)
    return t


def four_launches(pool, hp, dp, B, N, crop, K, scale, lr0, slq, gt, lqs):
    """The device part of make_batch on the current stream.  hp / dp: one upload in host and device memory -- the tables
    [HR flags 0 | HR flags | LR0 flags] of B N rows each, then the [B,K,K] kernels."""
    n, hl = B * N, int(lr0.shape[-1])
    tb = n * ITEM.itemsize
    kp, st, lib = dp + 3 * tb, L.stream(), L.lib()
    L.check(lib.dvsr_task_degrade(hp, dp, n, pool.format, pool.pixel_stride, crop, crop, kp, B, K, scale, lr0.data_ptr(), 1, st),
            "dvsr_task_degrade")
    L.check(lib.dvsr_task_degrade(hp + 2 * tb, dp + 2 * tb, n, L.FRAME_F32_CHW, 1, hl, hl, kp, B, K, scale, slq.data_ptr(), 0, st),
            "dvsr_task_degrade")
    L.check(lib.dvsr_task_gather(hp + tb, dp + tb, n, pool.format, pool.pixel_stride, crop, crop, gt.data_ptr(), st),
            "dvsr_task_gather")
    L.check(lib.dvsr_task_gather(hp + 2 * tb, dp + 2 * tb, n, L.FRAME_F32_CHW, 1, hl, hl, lqs.data_ptr(), st), "dvsr_task_gather")


def prepare_batch(pool, picks, draws, kernel_size, scale, staging=None):
    """The host part of make_batch: the checks (ValueError), the B shifted kernels and the three tables, written into
    `staging`'s pinned bytes (which the caller has waited for) or into an array of their own.  No GPU call; the rows of the LR0
    table get their addresses in launch_batch, which allocates that scratch."""
    B = len(picks)
    if B < 1 or len(draws) != B:
        raise ValueError("make_batch: %d picks and %d draws" % (B, len(draws)))
    N = len(picks[0][1])
    crop, scale = int(draws[0]["crop"]), int(scale)
    if isinstance(kernel_size, bool) or not isinstance(kernel_size, numbers.Integral) or kernel_size < 1:
        raise ValueError("make_batch: kernel_size=%r" % (kernel_size,))
    check_geometry(crop, nominal_edge(kernel_size, scale) if 1 <= scale <= MAX_SCALE else 0, scale)
    for (key, frames), d in zip(picks, draws):
        if key not in pool.sequences:
            raise ValueError("make_batch: no sequence %r in the pool" % (key,))
        if len(frames) != N or N < 1 or any(not 0 <= f < pool.lengths[key] for f in frames):
            raise ValueError("make_batch: frames %r of sequence %r (%d frames); every task has %d" % (list(frames), key, pool.lengths[key], N))
        h, w = pool.size(key)
        if int(d["crop"]) != crop or not (0 <= d["py"] and d["py"] + crop <= h and 0 <= d["px"] and d["px"] + crop <= w):
            raise ValueError("make_batch: a %d x %d crop at (%d, %d) is larger than or outside a %d x %d frame (one crop size "
                             "per batch: %d)" % (d["crop"], d["crop"], d["py"], d["px"], h, w, crop))
    kernels = shifted_kernels(draws, kernel_size, scale)
    K = int(kernels.shape[-1])
    hl, hs = check_geometry(crop, K, scale)
    n = B * N
    if 3 * n > 65535:
        raise ValueError("make_batch: %d tasks of %d frames are more than 65535 planes" % (B, N))
    tb = n * ITEM.itemsize
    total = 3 * tb + kernels.nbytes
    if staging is not None:
        if staging.host.numel() < total:
            raise ValueError("make_batch: staging of %d bytes, the batch needs %d" % (staging.host.numel(), total))
        host = staging.host.numpy()[:total]
    else:
        host = np.empty(total, dtype=np.uint8)
    t_hr0, t_hr, t_lr = (host[i * tb:(i + 1) * tb].view(ITEM) for i in range(3))
    i = 0
    for b, ((key, frames), d) in enumerate(zip(picks, draws)):
        flags = draw_flags(d)
        for f in frames:
            src, row, plane = pool.crop_item(key, int(f), int(d["py"]), int(d["px"]))
            t_hr0[i] = (src, row, plane, b, 0)
            t_hr[i] = (src, row, plane, b, flags)
            t_lr[i] = (0, hl, hl * hl, b, flags)
            i += 1
    host[3 * tb:].view(np.float32)[:] = kernels.reshape(-1)
    return {"B": B, "N": N, "crop": crop, "K": K, "scale": scale, "hl": hl, "hs": hs, "host": host, "lr_table": t_lr,
            "kernels": kernels, "draws": list(draws), "staging": staging}


def launch_batch(pool, prep, out=None):
    """The device part of make_batch on the current stream: the outputs and the scratch, one upload, four launches."""
    B, N, crop, hl, hs, host, staging = (prep[k] for k in ("B", "N", "crop", "hl", "hs", "host", "staging"))
    dev = pool.device
    with torch.cuda.device(dev):
        gt = _check_out(out, "GT", (B, N, 3, crop, crop), dev)
        lqs = _check_out(out, "LQs", (B, N, 3, hl, hl), dev)
        slq = _check_out(out, "SuperLQs", (B, N, 3, hs, hs), dev)
        lr0 = torch.empty((B * N, 3, hl, hl), dtype=torch.float32, device=dev)
        prep["lr_table"]["src"] = lr0.data_ptr() + 4 * 3 * hl * hl * np.arange(B * N, dtype=np.uint64)
        if staging is not None:
            staging.upload(host.size)
            devb = staging.dev
        else:
            devb = torch.from_numpy(host).to(dev)
        four_launches(pool, host.ctypes.data, devb.data_ptr(), B, N, crop, prep["K"], prep["scale"], lr0, slq, gt, lqs)
        if staging is None:
            devb.record_stream(torch.cuda.current_stream())
    return {"GT": gt, "LQs": lqs, "SuperLQs": slq, "kernels": torch.from_numpy(prep["kernels"]), "draws": prep["draws"]}


def make_batch(pool, picks, draws, kernel_size, scale, out=None, staging=None):
    """The deterministic part: B tasks in four launches on the current stream.

    picks: B pairs (sequence name, N frame indices); draws: B dicts of draw_task.  The crop is ``draws[b]['crop']`` square (the
    caller passes 2 * patch_size, vsrbase.py:165, at any scale) and the same for the batch.
      1. dvsr_task_degrade  HR -> LR0, flags 0, quantiser on (vsrbase.py:187-188), into a [B N,3,h,h] scratch
      2. dvsr_task_degrade  LR0 -> SuperLQs with the task's flags, quantiser off (:189)
      3. dvsr_task_gather   HR -> GT with flags          4. dvsr_task_gather   LR0 -> LQs with flags
    The flips are on the store side because the reference augments AFTER it degrades (:192).  The tables and the B shifted
    kernels go up in one copy (through `staging`, a Staging that the caller has waited for, or a pageable copy without).
    Returns {'GT': [B,N,3,crop,crop], 'LQs': [B,N,3,h,h], 'SuperLQs': [B,N,3,hs,hs], 'kernels': the [B,K,K] host tensor,
    'draws'} -- what adapt.meta_train_step reads.  Arguments are checked before the first GPU call (ValueError).
    prepare_batch and launch_batch are its host and device halves."""
    return launch_batch(pool, prepare_batch(pool, picks, draws, kernel_size, scale, staging), out)


class TaskSource:
    """Iterable over batches of tasks: ``for batch in TaskSource(opt, pool): meta_train_step(opt, ..., batch, optimizer)``.

    Reads the keys the reference reads: opt['scale'] and opt['datasets']['train'][N_frames | interval_list | patch_size |
    kernel_size | batch_size].  Each epoch (each ``iter()``) is a permutation of range(n_samples) from the source's own
    ``random.Random(seed)``, cut to a multiple of `world`, sharded [rank::world], in batches of batch_size // world with
    drop_last; the draws of a task come from generators seeded by (seed, rank).  ``train=False``: no augmentation.  The tables
    and kernels of a batch go up through two pinned buffers in turn, each guarded by an event: ``batch()`` waits for nothing but
    the copy of the buffer it used two batches ago.  ValueErrors (a crop larger than a frame, a sequence shorter than a sample, a
    pad that the LR patch cannot reflect) come before the first GPU call."""

    def __init__(self, opt, pool, seed=0, rank=0, world=1, train=True, full_width=False):
        ds = opt["datasets"]["train"]
        self.pool, self.scale = pool, int(opt["scale"])
        self.n_frames, self.kernel_size, self.patch_size = int(ds["N_frames"]), int(ds["kernel_size"]), int(ds["patch_size"])
        self.crop = 2 * self.patch_size                                      # vsrbase.py:165
        self.train, self.full_width = bool(train), bool(full_width)
        rank, world = int(rank), int(world)
        if world < 1 or not 0 <= rank < world:
            raise ValueError("TaskSource: rank %d of %d" % (rank, world))
        self.rank, self.world = rank, world
        self.batch_size = int(ds["batch_size"]) // world
        if self.batch_size < 1:
            raise ValueError("TaskSource: batch_size %r over %d ranks" % (ds["batch_size"], world))
        self.index = SequenceIndex(pool.lengths, self.n_frames, ds["interval_list"])
        short = [k for k, t in pool.lengths.items() if t < min(self.index.sample_length)]
        if short:
            raise ValueError("TaskSource: sequence %r has %d frames, a sample needs %d" % (short[0], pool.lengths[short[0]],
                                                                                             min(self.index.sample_length)))
        for k in pool.lengths:
            h, w = pool.size(k)
            if self.crop > h or self.crop > w:
                raise ValueError("TaskSource: a crop of %d (2 x patch_size) is larger than the %d x %d frames of %r" % (self.crop, h, w, k))
            if h > w and not self.full_width:
                raise ValueError("TaskSource: %r is %d x %d; frames higher than wide need full_width=True" % (k, h, w))
        if not 1 <= self.scale <= MAX_SCALE:
            raise ValueError("TaskSource: scale %d (1 .. %d)" % (self.scale, MAX_SCALE))
        check_geometry(self.crop, nominal_edge(self.kernel_size, self.scale), self.scale, "TaskSource")
        self._order = random.Random(seed)
        self._py = random.Random("dynavsr tasks %d/%d" % (int(seed), rank))
        self._np = np.random.RandomState([int(seed) % 2 ** 32, rank])
        self._staging, self._turn = None, 0

    def __len__(self):
        return (self.index.n_samples // self.world) // self.batch_size

    def __iter__(self):
        perm = list(range(self.index.n_samples))
        self._order.shuffle(perm)
        shard = perm[:len(perm) // self.world * self.world][self.rank::self.world]
        for i in range(0, len(shard) - self.batch_size + 1, self.batch_size):
            yield self.batch(shard[i:i + self.batch_size])

    def draw(self, indices):
        """(picks, draws) of the samples `indices`: the host part of batch()."""
        picks, draws = [], []
        for idx in indices:
            key, _, frames = self.index.find(idx)
            h, w = self.pool.size(key)
            picks.append((key, frames))
            draws.append(draw_task(self._py, self._np, h, w, self.crop, augment=self.train, full_width=self.full_width))
        return picks, draws

    def prepare(self, indices):
        """The host half of batch(): the draws, the kernels and the tables, in the pinned buffer whose turn it is -- after the
        copy that last read it, two batches ago, has run.  Nothing else is waited for."""
        picks, draws = self.draw(indices)
        if self._staging is None:
            nb = table_bytes(len(indices) * self.n_frames, len(indices))
            self._staging = [Staging(nb, self.pool.device) for _ in range(2)]
        s = self._staging[self._turn]
        self._turn ^= 1
        s.wait()
        prep = prepare_batch(self.pool, picks, draws, self.kernel_size, self.scale, staging=s)
        prep["indices"] = list(indices)
        return prep

    def launch(self, prep):
        out = launch_batch(self.pool, prep)
        out["indices"] = prep["indices"]
        return out

    def batch(self, indices):
        """One batch of the samples `indices`: prepare() then launch()."""
        return self.launch(self.prepare(indices))
