"""Records what the reference's own `imresize` / `calculate_weights_indices` (data/util.py) and
`old_kernel_generator.Degradation` return into tests/golden/imresize_reference.npz and old_kernel_reference.npz.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_imresize_golden.py /path/to/reference/codes

The reference checkout is needed only for this one-off recording: tests/test_imresize_host.py and tests/test_gpu_imresize.py
read the fixtures alone.  They hold inputs and outputs, data only.

imresize_reference.npz, per case `<name>` (37x50 at 1/4, 27x33 at 1/3, 24x40 at 1/2, 9x13 at x4, 12x10 at x2):
    <name>_in uint8 [3,H,W]                      a random byte image; the reference sees it / 255 in float32
    <name>_out float32 [3,oh,ow]                 imresize(in / 255, scale)
    <name>_scale int [2]                         num, den
    <name>_{h,w}_weights, _indices, _sym         calculate_weights_indices of the two axes: float32 weights, its indices into the
                                                 symmetric-padded copy, (sym_len_s, sym_len_e)
    <name>_{h,w}_dev float64                     the largest |reference weight, folded - the float64 restatement's| of the axis:
                                                 the fp32 rounding the reference's own evaluation carries (printed; the tests
                                                 hold the library's table to four times the largest of them)
old_kernel_reference.npz, per case `s<scale>_t<type>_<i>`: _kernel float32 [21,21], _params float64 [sigma_x, sigma_y, theta],
_dev float64: the largest |kernel - the same code run with float64 as torch's default dtype| (printed; the bar likewise).
The generator builds its kernels with `.cuda()`: torch.Tensor.cuda is patched to the identity inside this recorder only."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import imresize_ref as R  # noqa: E402

CASES = (("q_37x50", 37, 50, 1, 4), ("t_27x33", 27, 33, 1, 3), ("h_24x40", 24, 40, 1, 2), ("x4_9x13", 9, 13, 4, 1),
         ("x2_12x10", 12, 10, 2, 1))
OLD_CASES = [(s, t, sig, th) for s in (2, 4) for t in (0.0, 0.7)
             for sig, th in (((1.2, 2.4), 0.6), ((3.0, 0.8), 2.1), ((0.0, 0.0), 0.0))]


def load(codes, rel, name, stand_ins=()):
    spec = importlib.util.spec_from_file_location(name, os.path.join(codes, *rel))
    mod = importlib.util.module_from_spec(spec)
    for dep in stand_ins:       # imported at the top of that file, not used by what is recorded: an empty stand-in will do
        if importlib.util.find_spec(dep) is None:
            sys.modules[dep] = type(sys)(dep)
    spec.loader.exec_module(mod)
    return mod


def record_imresize(ref, seed):
    r = np.random.RandomState(seed)
    out, worst = {}, 0.0
    for name, h, w, num, den in CASES:
        img = r.randint(0, 256, (3, h, w)).astype(np.uint8)
        scale = num / den
        y = ref.imresize(torch.from_numpy(img.astype(np.float32) / np.float32(255.0)), scale)
        out[name + "_in"], out[name + "_out"] = img, y.numpy().astype(np.float32)
        out[name + "_scale"] = np.array([num, den])
        for axis, n_in in (("h", h), ("w", w)):
            n_out = int(np.ceil(n_in * scale))
            wt, idx, ss, se = ref.calculate_weights_indices(n_in, n_out, scale, 'cubic', 4, True)
            wt, idx = wt.numpy().astype(np.float32), idx.numpy().astype(np.int64)
            dev = float(np.abs(R.fold_reference(wt, idx, ss, n_in) - dense64(n_in, num, den)).max())
            out["%s_%s_weights" % (name, axis)], out["%s_%s_indices" % (name, axis)] = wt, idx
            out["%s_%s_sym" % (name, axis)], out["%s_%s_dev" % (name, axis)] = np.array([ss, se]), np.array(dev)
            worst = max(worst, dev)
        assert out[name + "_out"].shape == (3, R.n_out(h, num, den), R.n_out(w, num, den))
    return out, worst


def dense64(n_in, num, den):
    """The restatement's folded weights before their rounding to fp32, as a dense [n_out, n_in] matrix."""
    rows = R.axis_rows(n_in, num, den, True)
    m = np.zeros((len(rows), n_in))
    for i, (f, w) in enumerate(rows):
        m[i, f:f + len(w)] = w
    return m


def record_old(codes):
    real = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        old = load(codes, ("data", "old_kernel_generator.py"), "reference_old_kernel_generator")
        out = {}
        count = {}
        for s, t, sig, th in OLD_CASES:
            i = count[(s, t)] = count.get((s, t), -1) + 1
            d = old.Degradation(21, s, type=t, theta=th, sigma=list(sig))
            key = "s%d_t%.1f_%d" % (s, t, i)
            out[key + "_kernel"] = d.get_kernel().numpy().astype(np.float32)
            out[key + "_params"] = np.array([sig[0], sig[1], th])
            torch.set_default_dtype(torch.float64)      # the same code in double: what its fp32 evaluation deviates from
            try:
                d64 = old.Degradation(21, s, type=t, theta=th, sigma=list(sig)).get_kernel().numpy()
            finally:
                torch.set_default_dtype(torch.float32)
            assert d64.dtype == np.float64
            out[key + "_dev"] = np.array(float(np.abs(d64 - out[key + "_kernel"]).max()))
    finally:
        torch.Tensor.cuda = real
    return out


def main():
    codes = sys.argv[1]
    ref = load(codes, ("data", "util.py"), "reference_data_util", ("cv2",))
    golden = os.path.join(ROOT, "tests", "golden")
    out, worst = record_imresize(ref, 0)
    dst = os.path.join(golden, "imresize_reference.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes; largest deviation of the reference's folded fp32 weights from the float64 rule: %.3e" % worst)
    old = record_old(codes)
    dst = os.path.join(golden, "old_kernel_reference.npz")
    np.savez_compressed(dst, **old)
    print(dst, os.path.getsize(dst), "bytes;", len(old) // 3, "kernels; largest deviation of the reference's fp32 kernels from "
          "its own code run in float64: %.3e" % max(float(v) for k, v in old.items() if k.endswith("_dev")))


if __name__ == "__main__":
    main()
