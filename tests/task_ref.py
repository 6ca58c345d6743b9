"""Helpers of tests/test_tasks_host.py and tests/test_gpu_tasks.py (and of tools/gen_task_golden.py, which invents its images
here): the recorded reference of tests/golden/task_reference{,_src}.npz and task_reference.json, the deterministic byte images, the tie band of the
quantised comparison, and the per-item composition that dvsr_task_degrade / dvsr_task_gather / make_batch must equal bit for bit."""
import json
import os
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_NPZ = os.path.join(HERE, "golden", "task_reference.npz")
GOLDEN_SRC_NPZ = os.path.join(HERE, "golden", "task_reference_src.npz")
GOLDEN_JSON = os.path.join(HERE, "golden", "task_reference.json")
TIE_BAND = 2e-3          # in 8-bit levels: tests/test_frame_degrade_host.py's, for the same reason
FRAME_H, FRAME_W = 72, 96
FLIP_W, FLIP_H, TRANSPOSE = 1, 2, 4


def frame_bytes(name, h=FRAME_H, w=FRAME_W):
    """The invented uint8 [h,w,3] RGB image that stands for the file `name`: smooth structure over the whole range plus noise, as
    footage has it (the bytes of tests/test_frame_degrade_host.py's hr_u8, seeded by the name)."""
    seed = zlib.crc32(name.encode()) % 1000
    r = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    img = np.stack([127.5 + 110.0 * np.sin(xx / (7.3 + c) + seed + c) * np.cos(yy / (5.1 + 2 * c) - c) for c in range(3)], -1)
    img = img + r.randint(-24, 25, size=img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def frame_name(key, index):
    return "%s/%08d.png" % (key, index)


def sequence_bytes(key, length, h=FRAME_H, w=FRAME_W):
    return np.stack([frame_bytes(frame_name(key, i), h, w) for i in range(length)])


def load_reference():
    """(meta, arrays): the JSON (index tables, draws, what each recorded task is) and the npz (its tensors)."""
    with open(GOLDEN_JSON) as f:
        meta = json.load(f)
    arrays = {}
    for path in (GOLDEN_NPZ, GOLDEN_SRC_NPZ):
        with np.load(path) as z:
            arrays.update({k: z[k] for k in z.files})
    return meta, arrays


def outside_tie_band(y):
    """Where 255 y of an unquantised LR value lies more than TIE_BAND from a half-integer: there a result within 2e-6 of y has
    y's 8-bit level."""
    v = 255.0 * np.asarray(y, dtype=np.float64)
    return np.abs(v - np.floor(v) - 0.5) > TIE_BAND


def flags_of(draw):
    return (FLIP_W if draw["hflip"] else 0) | (FLIP_H if draw["vflip"] else 0) | (TRANSPOSE if draw.get("rot") else 0)


def flip_np(x, flags):
    """The reference's augment on the last two axes of an array: hflip, vflip, then the permute."""
    if flags & FLIP_W:
        x = x[..., :, ::-1]
    if flags & FLIP_H:
        x = x[..., ::-1, :]
    if flags & TRANSPOSE:
        x = np.swapaxes(x, -1, -2)
    return np.ascontiguousarray(x)


def flip_t(x, flags):
    """The same on a torch tensor: torch.flip / .transpose(-1, -2)."""
    import torch
    dims = [d for d, bit in ((-1, FLIP_W), (-2, FLIP_H)) if flags & bit]
    if dims:
        x = torch.flip(x, dims)
    if flags & TRANSPOSE:
        x = x.transpose(-1, -2)
    return x.contiguous()


def correlate_abs(img, kernel, scale):
    """oracle.degradation.apply's correlation of a non-negative [N,C,H,W] image with |the shifted kernel| in float64: what a
    per-pixel difference of the input can do to the output, at most."""
    from oracle import degradation as od
    k = np.abs(od.kernel_shift(np.asarray(kernel, dtype=np.float64), scale).astype(np.float32).astype(np.float64))
    kk = k.shape[0]
    p = kk // 2
    x = np.pad(np.asarray(img, dtype=np.float64), ((0, 0), (0, 0), (p, p), (p, p)), mode="reflect")
    h, w = img.shape[-2:]
    ho, wo = (h + 2 * p - kk) // scale + 1, (w + 2 * p - kk) // scale + 1
    y = np.zeros(img.shape[:2] + (ho, wo))
    for dy in range(kk):
        for dx in range(kk):
            y += k[dy, dx] * x[:, :, dy:dy + (ho - 1) * scale + 1:scale, dx:dx + (wo - 1) * scale + 1:scale]
    return y


class FixedKernel:
    """A Degradation whose shifted kernel is given: what the composition applies when make_batch has zero-padded a kernel."""

    def __new__(cls, shifted, scale):
        from dynavsr_amd.data.random_kernel_generator import Degradation
        import torch
        d = Degradation(3, scale)
        shifted = np.ascontiguousarray(shifted, dtype=np.float32)
        d.kernel = shifted                                              # apply() looks at ndim alone
        d._shift_val_host = torch.from_numpy(shifted)[None]
        d._shifted_on = lambda device: d._shift_val_host.to(device)
        d.shifted_edge = lambda index=0: int(shifted.shape[0])
        return d
