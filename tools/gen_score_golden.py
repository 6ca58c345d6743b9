"""Records what the reference's own `rgb2ycbcr` / `bgr2ycbcr` with only_y=True (data/util.py), `util.crop_border` and
`util.calculate_psnr` (utils/util.py) return into tests/golden/score_reference.npz.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_score_golden.py /path/to/reference/codes

The reference checkout is needed only for this one-off recording: tests/test_score_host.py reads the fixture alone.  It holds
inputs and outputs, data only (no image is larger than 64 x 64):
    y_<rgb|bgr>_u8_in / _out      a uint8 image [64,64,3] and the uint8 Y [64,64] the function returns for it
    y_<rgb|bgr>_f32_in / _out     the same kind of image as float32 in [0,1] ([48,48,3], bytes / 255: what the evaluation scripts
                                  pass after tensor2img(..) / 255.) and the float32 Y the function returns; each call gets a copy,
                                  because the functions scale a float image IN PLACE
    psnr_a, psnr_b                two uint8 images [40,56,3]; for every k of psnr_crops: crop_k<k>_a = util.crop_border([a], k)[0],
                                  psnr_rgb_k<k> = calculate_psnr of the cropped pair, psnr_y_k<k> = that of the cropped uint8 Y
                                  images (rgb2ycbcr, only_y=True), psnr_same = calculate_psnr(a, a) (inf)
A uint8 triple (R, G, B) whose Y level, evaluated in float64, lies within 1e-3 levels of a tie is drawn again (the 194 exact
ties of 65481 R + 128553 G + 24966 B among them), and the recorder asserts that none is left -- the reference alone decides
every value of the fixture.  cv2, torchvision and yaml are imported at the top of the reference's files and not used by the
recorded functions: empty stand-ins will do where they are not installed."""
import importlib.util
import os
import sys

import numpy as np

TIE = 1e-3
CROPS = (0, 3, 7)


def stand_in(name, **attrs):
    top = name.split('.')[0]
    if top in sys.modules:                       # the real module, or the stand-in of its parent package
        if hasattr(sys.modules[top], '__file__') and sys.modules[top].__file__:
            return
    elif importlib.util.find_spec(top) is not None:
        return
    mod = type(sys)(name)
    for k, v in attrs.items():
        setattr(mod, k, v)
    sys.modules[name] = mod


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference(codes):
    stand_in("cv2")
    stand_in("torchvision", utils=None)
    stand_in("torchvision.utils", make_grid=None)
    stand_in("yaml", Loader=None, Dumper=None)
    return load(os.path.join(codes, "data", "util.py"), "reference_data_util"), \
        load(os.path.join(codes, "utils", "util.py"), "reference_utils_util")


def draw_u8(r, shape, order):
    """A uint8 image [h,w,3] in channel order `order` without a pixel near a tie of its Y level."""
    h, w = shape
    px = r.randint(0, 256, (h * w, 3)).astype(np.uint8)
    coef = np.array([65.481, 128.553, 24.966] if order == 'rgb' else [24.966, 128.553, 65.481])
    redrawn = 0
    while True:
        levels = np.dot(px.astype(np.float64), coef) / 255.0 + 16.0
        near = np.abs(levels - np.floor(levels) - 0.5) < TIE
        if not near.any():
            return px.reshape(h, w, 3), redrawn
        px[near] = r.randint(0, 256, (int(near.sum()), 3)).astype(np.uint8)
        redrawn += int(near.sum())


def record(data_util, utils_util, seed):
    r = np.random.RandomState(seed)
    out, redrawn = {}, 0
    for order, fn in (('rgb', data_util.rgb2ycbcr), ('bgr', data_util.bgr2ycbcr)):
        u, n = draw_u8(r, (64, 64), order)
        redrawn += n
        out["y_%s_u8_in" % order], out["y_%s_u8_out" % order] = u, fn(u.copy(), only_y=True)
        u, n = draw_u8(r, (48, 48), order)
        redrawn += n
        f = u.astype(np.float32) / 255.
        out["y_%s_f32_in" % order], out["y_%s_f32_out" % order] = f, fn(f.copy(), only_y=True)
        assert out["y_%s_u8_out" % order].dtype == np.uint8 and out["y_%s_f32_out" % order].dtype == np.float32
    a, n1 = draw_u8(r, (40, 56), 'rgb')
    b = np.clip(a.astype(np.int32) + r.randint(-9, 10, a.shape), 0, 255).astype(np.uint8)
    while True:                                  # b's pixels near a tie take a's values
        levels = np.dot(b.astype(np.float64), [65.481, 128.553, 24.966]) / 255.0 + 16.0
        near = np.abs(levels - np.floor(levels) - 0.5) < TIE
        if not near.any():
            break
        b[near] = a[near]
    out["psnr_a"], out["psnr_b"], out["psnr_crops"] = a, b, np.array(CROPS)
    ya, yb = data_util.rgb2ycbcr(a.copy(), only_y=True), data_util.rgb2ycbcr(b.copy(), only_y=True)
    for k in CROPS:
        ca, cb = utils_util.crop_border([a, b], k)
        cya, cyb = utils_util.crop_border([ya, yb], k)
        out["crop_k%d_a" % k] = np.ascontiguousarray(ca)
        out["psnr_rgb_k%d" % k] = np.float64(utils_util.calculate_psnr(ca, cb))
        out["psnr_y_k%d" % k] = np.float64(utils_util.calculate_psnr(cya, cyb))
    out["psnr_same"] = np.float64(utils_util.calculate_psnr(a, a))
    return out, redrawn + n1


def main():
    data_util, utils_util = load_reference(sys.argv[1])
    out, redrawn = record(data_util, utils_util, 0)
    dst = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "score_reference.npz")
    np.savez_compressed(dst, **out)
    print(dst, "%d pixels drawn again" % redrawn, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
