"""Records what the reference's own `ycbcr2rgb`, `rgb2ycbcr(only_y=False)` and `bgr2ycbcr(only_y=False)` return into
tests/golden/ycbcr_reference.npz.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_ycbcr_golden.py /path/to/reference/codes

The reference checkout is needed only for this one-off recording: tests/test_yuv_host.py reads the fixture alone.  It holds
inputs and outputs, data only: a float64 image of 32 x 32 and a uint8 image of 64 x 64 pixels per function (keys `<function>_<f64|u8>_<in|out>`).
The YCbCr inputs are `rgb2ycbcr` of an RGB image with a margin to the gamut's faces, so that `ycbcr2rgb` stays in range (the
reference's uint8 path would wrap around).  The functions scale a float image IN PLACE, so each gets a copy.
For the uint8 images the functions are also run on the same pixels as float64: that gives the values they round.  A pixel
with a value within 1e-3 levels of a tie is drawn again (about 2 in 1000 values are, so a whole image without one does not
exist), and the recorder asserts that none is left -- the reference alone decides every byte of the fixture."""
import importlib.util
import os
import sys

import numpy as np

SIZE = 64          # the uint8 images
SIZE_F = 32        # the float64 images
TIE = 1e-3


def load_reference(codes):
    spec = importlib.util.spec_from_file_location("reference_data_util", os.path.join(codes, "data", "util.py"))
    ref = importlib.util.module_from_spec(spec)
    for dep in ("cv2",):        # imported at the top of that file, not used by the colour functions: an empty stand-in will do
        if importlib.util.find_spec(dep) is None:
            sys.modules[dep] = type(sys)(dep)
    spec.loader.exec_module(ref)
    return ref


def record(ref, seed):
    r = np.random.RandomState(seed)
    fns = {"rgb2ycbcr": lambda x: ref.rgb2ycbcr(x, only_y=False), "bgr2ycbcr": lambda x: ref.bgr2ycbcr(x, only_y=False),
           "ycbcr2rgb": ref.ycbcr2rgb}
    n = SIZE * SIZE
    draw_u8 = {"rgb2ycbcr": lambda k: r.randint(0, 256, (k, 3)).astype(np.uint8),
               "bgr2ycbcr": lambda k: r.randint(0, 256, (k, 3)).astype(np.uint8),
               "ycbcr2rgb": lambda k: ref.rgb2ycbcr(r.randint(8, 248, (k, 3)).astype(np.uint8), only_y=False)}
    draw_f = {"rgb2ycbcr": lambda k: r.uniform(0.0, 1.0, (k, 3)), "bgr2ycbcr": lambda k: r.uniform(0.0, 1.0, (k, 3)),
              "ycbcr2rgb": lambda k: ref.rgb2ycbcr(r.uniform(0.02, 0.98, (k, 3)), only_y=False)}
    out, worst, redrawn = {}, 0.5, 0
    for name, fn in fns.items():
        f_in = draw_f[name](SIZE_F * SIZE_F).reshape(SIZE_F, SIZE_F, 3)
        u_in = draw_u8[name](n)
        while True:
            levels = fn(u_in.astype(np.float64) / 255.0) * 255.0       # what the uint8 path rounds
            near = np.abs(levels - np.floor(levels) - 0.5).min(axis=1) < TIE
            if not near.any():
                break
            u_in[near] = draw_u8[name](int(near.sum()))               # a pixel near a tie is drawn again
            redrawn += int(near.sum())
        u_in = u_in.reshape(SIZE, SIZE, 3)
        out[name + "_f64_in"], out[name + "_f64_out"] = f_in, fn(f_in.copy())
        out[name + "_u8_in"], out[name + "_u8_out"] = u_in, fn(u_in.copy())
        levels = fn(u_in.astype(np.float64) / 255.0) * 255.0
        assert levels.min() >= 0.0 and levels.max() <= 255.0, (name, levels.min(), levels.max())
        assert np.array_equal(np.rint(levels).astype(np.uint8), out[name + "_u8_out"]), name
        worst = min(worst, float(np.abs(levels - np.floor(levels) - 0.5).min()))
    assert worst >= TIE, worst
    return out, worst, redrawn


def main():
    ref = load_reference(sys.argv[1])
    out, worst, redrawn = record(ref, 0)
    dst = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "ycbcr_reference.npz")
    np.savez_compressed(dst, **out)
    print(dst, "nearest tie %.3e levels, %d pixels drawn again" % (worst, redrawn), os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
