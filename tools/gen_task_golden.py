"""Records what the reference's own meta-training dataset, VSRBase (codes/data/meta_learner/vsrbase.py), counts, draws and
returns into tests/golden/task_reference.npz, task_reference_src.npz and task_reference.json.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_task_golden.py /path/to/reference/codes

The reference checkout is needed only for this one-off recording: tests/test_tasks_host.py and tests/test_gpu_tasks.py read the
fixtures alone.  They hold inputs and outputs, data only.

The reference's `vsrbase`, `preprocessing` and `random_kernel_generator` are imported as they are.  Packages that their files
import at the top and this recording never calls (imageio, cv2, skimage, torchvision, ... where missing) get empty stand-ins,
and `np.int` (removed from numpy; random_kernel_generator.py:72) is `int` for this run.  A subclass of VSRBase invents the file
names (`_scan`) and `imageio.imread` returns tests/task_ref.py's deterministic byte image per name.  The reference's global
generators are seeded with `random.seed(s)`, `np.random.seed(s)`; the draws are read off by standing between `preprocessing` and
its `random` module, the kernel and the unquantised LR by standing around `Degradation.apply`.

task_reference.json
    index      three configurations {lengths, n_frames, interval_list, n_samples, weights, table}: one stride; [1, 2, -1]; a
               sequence too short for the widest stride.  table[idx] = [key, stride_index, seq_idx, [frame indices]]
    draws      {seed, lengths, frame, patch_size, indices, draws}: 64 consecutive __getitem__ calls of one seeded dataset
    tasks      what each recorded task t<i> is: seed, scale, idx, key, frames, draw
task_reference.npz, per task t<i> (4 at scale 4: HR 64 x 64 out of 72 x 96 frames, LR 16 x 16, SLR 4 x 4; 1 at scale 2)
    _src uint8 [N,72,96,3]     the N frames as read (in task_reference_src.npz: bytes of this kind do not compress, and
                               two files stay at half the size one would have)
    _gt  uint8 [N,3,64,64]     GT * 255 (exact), augmented
    _lr_unq float32 [N,3,h,h]  the first apply(), before quantisation and BEFORE augment
    _lqs, _slq float32         LQs, SuperLQs as returned
    _kernel float64 [21,21]    kernel_gen.kernel (unshifted)"""
import json
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import task_ref as R  # noqa: E402

STAND_INS = ("imageio", "tqdm", "cv2", "skimage", "skimage.io", "skimage.color", "skimage.transform", "torchvision",
             "torchvision.transforms")
INDEX_CONFIGS = (({"000": 12, "001": 9}, 5, 1), ({"000": 12, "001": 9, "002": 23}, 5, [1, 2, -1]), ({"000": 12, "short": 8}, 5, [1, 2]))
LENGTHS = {"000": 12, "001": 12}
SEED, N_DRAWS, N_TASKS = 20210, 64, 4


def stand_in(names):
    import importlib.util
    for name in names:
        top = name.split(".")[0]
        if top in sys.modules and not getattr(sys.modules[top], "_stand_in", False):
            continue
        if name == top and importlib.util.find_spec(top) is not None:
            continue
        mod = types.ModuleType(name)
        mod._stand_in = True
        sys.modules[name] = mod
        if "." in name:
            setattr(sys.modules[name.rsplit(".", 1)[0]], name.rsplit(".", 1)[1], mod)


class Tap:
    """Stands for the `random` module inside preprocessing: the same generator, every call noted."""

    def __init__(self):
        self.log = []

    def randrange(self, *a):
        v = random.randrange(*a)
        self.log.append(("randrange", v))
        return v

    def random(self):
        v = random.random()
        self.log.append(("random", v))
        return v


def options(scale, interval_list, n_frames=5, patch_size=32):
    return {"scale": scale, "datasets": {"train": {"img_type": "img", "interval_list": interval_list, "N_frames": n_frames,
                                                    "patch_size": patch_size, "kernel_size": 21}}}


def main():
    codes = sys.argv[1]
    stand_in(STAND_INS)
    if not hasattr(np, "int"):
        np.int = int
    sys.path.insert(0, codes)
    from data.meta_learner import preprocessing, vsrbase
    from data import random_kernel_generator as rkg

    class Invented(vsrbase.VSRBase):
        def __init__(self, opt, lengths, train=True):
            self._lengths = lengths
            super().__init__(opt, train=train)

        def _set_directory(self, data_root):
            self.apath = ""

        def _scan(self):
            return {k: [R.frame_name(k, i) for i in range(n)] for k, n in self._lengths.items()}

    vsrbase.imageio.imread = lambda name: R.frame_bytes(name)
    tap = Tap()
    preprocessing.random = tap
    seen = {}
    real_params, real_apply = preprocessing.set_kernel_params, rkg.Degradation.apply

    def params(*a, **k):
        seen["params"] = real_params(*a, **k)
        return seen["params"]

    def apply(self, img):
        y = real_apply(self, img)
        seen.setdefault("applied", []).append(y.clone())
        seen["kernel"] = np.array(self.kernel, dtype=np.float64)
        return y

    preprocessing.set_kernel_params, rkg.Degradation.apply = params, apply

    def frames_of(ds, idx):
        """the frame indices __getitem__ reads for idx (its own slice, vsrbase.py:140-151)"""
        key, str_idx, seq_idx = ds.find_set(idx)
        names = ds.dict_hr[key]
        end = seq_idx + ds.sample_length[str_idx] if ds.stride[str_idx] > 0 else seq_idx - ds.sample_length[str_idx]
        picked = names[seq_idx:end:ds.stride[str_idx]] if end >= 0 else names[seq_idx::ds.stride[str_idx]]
        return key, str_idx, seq_idx, [names.index(n) for n in picked]

    meta = {"index": []}
    for lengths, n_frames, interval in INDEX_CONFIGS:
        ds = Invented(options(4, interval, n_frames), lengths)
        table = []
        for idx in range(len(ds)):
            key, str_idx, seq_idx, fr = frames_of(ds, idx)
            table.append([key, str_idx, seq_idx, fr])
        meta["index"].append({"lengths": lengths, "n_frames": n_frames, "interval_list": interval, "n_samples": len(ds),
                              "weights": ds.sampling_weights(), "table": table})

    def get(ds, idx):
        tap.log.clear()
        seen.clear()
        item = ds[idx]
        kinds = [k for k, _ in tap.log]
        assert kinds == ["randrange", "randrange", "random", "random"], kinds
        p = seen["params"]
        draw = {"py": tap.log[0][1], "px": tap.log[1][1], "sigma_x": p["sigma"][0], "sigma_y": p["sigma"][1], "theta": p["theta"],
                "hflip": tap.log[2][1] < 0.5, "vflip": tap.log[3][1] < 0.5, "rot": False}
        return item, draw

    arrays, tasks = {}, []

    def record(ds, idx, seed, scale, item, draw):
        t = "t%d" % len(tasks)
        key, _, _, fr = frames_of(ds, idx)
        arrays[t + "_src"] = np.stack([R.frame_bytes(R.frame_name(key, f)) for f in fr])
        gt = item["GT"].numpy() * 255.0
        assert np.array_equal(gt, np.rint(gt)) or np.abs(gt - np.rint(gt)).max() < 1e-3
        arrays[t + "_gt"] = np.rint(gt).astype(np.uint8)
        assert np.array_equal(arrays[t + "_gt"].astype(np.float32) / np.float32(255), item["GT"].numpy())
        arrays[t + "_lr_unq"] = seen["applied"][0].numpy().astype(np.float32)
        arrays[t + "_lqs"] = item["LQs"].numpy().astype(np.float32)
        arrays[t + "_slq"] = item["SuperLQs"].numpy().astype(np.float32)
        arrays[t + "_kernel"] = seen["kernel"]
        tasks.append({"name": t, "seed": seed, "scale": scale, "idx": idx, "key": key, "frames": fr, "draw": draw})

    ds = Invented(options(4, [1, 2, -1]), LENGTHS)
    random.seed(SEED)
    np.random.seed(SEED)
    indices, draws = [(7 * i) % len(ds) for i in range(N_DRAWS)], []
    for i, idx in enumerate(indices):
        item, draw = get(ds, idx)
        draws.append(draw)
        if i < N_TASKS:
            record(ds, idx, SEED, 4, item, draw)
    meta["draws"] = {"seed": SEED, "lengths": LENGTHS, "frame": [R.FRAME_H, R.FRAME_W], "patch_size": 32, "n_frames": 5,
                     "interval_list": [1, 2, -1], "indices": indices, "draws": draws}
    ds2 = Invented(options(2, [1, 2, -1]), LENGTHS)
    random.seed(SEED + 1)
    np.random.seed(SEED + 1)
    item, draw = get(ds2, 11)
    record(ds2, 11, SEED + 1, 2, item, draw)
    meta["tasks"] = tasks

    golden = os.path.join(ROOT, "tests", "golden")
    for name, keep in (("task_reference.npz", lambda k: not k.endswith("_src")), ("task_reference_src.npz", lambda k: k.endswith("_src"))):
        dst = os.path.join(golden, name)
        np.savez_compressed(dst, **{k: v for k, v in arrays.items() if keep(k)})
        print(dst, os.path.getsize(dst), "bytes;", len(tasks), "tasks")
    for t in tasks:
        y = arrays[t["name"] + "_lr_unq"]
        print("  %s scale %d: LR %s, %.3f %% of its values inside the tie band" % (
            t["name"], t["scale"], y.shape, 100 * (1 - R.outside_tie_band(y).mean())))
    dst = os.path.join(golden, "task_reference.json")
    with open(dst, "w") as f:
        json.dump(meta, f, separators=(",", ":"))
    print(dst, os.path.getsize(dst), "bytes;", sum(c["n_samples"] for c in meta["index"]), "index rows,", len(draws), "draws")


if __name__ == "__main__":
    main()
