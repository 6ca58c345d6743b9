"""The reference's older synthetic degradation (codes/data/old_kernel_generator.py), the `degradation_type: bicubic` of every
shipped EDVR and DUF test YAML: a separable base kernel (`type` < 0.5: the impulse, otherwise the bicubic down-sampling filter
of the scale) convolved with the anisotropic Gaussian, cropped to `kernel_size` and renormalised.

Host side (tiny, numpy like random_kernel_generator.py): the 21 x 21 base and Gaussian kernels and their combination.  Device
side: ``apply`` -- ReflectionPad2d(kernel_size // 2) and the depth-wise correlation at stride `scale` -- is one launch of
``dvsr_degrade_apply`` with the kernel AS IT IS: this generator applies no centre-of-mass shift.  ``apply(img, quantise=True)``
fuses the 8-bit round trip into the store.  There is no CPU path for ``apply``.

The class also has what the video path reads from a degradation (``kernel``, ``scale``, ``shifted_edge()``,
``_shifted_on(device)``), so frames.degrade, video.degrade_frames and the evaluate_degraded functions take it as they take a
random_kernel_generator.Degradation.  The reference's scripts build their LR folders as a cascade of x2 applications with an
8-bit round trip between them: that is video.degrade_frames called on its own output."""
import numpy as np
import torch
from scipy import signal

from dynavsr_amd import _lib as L

base_kernel_dict = {
    'impulse': {2: [1], 4: [1]},
    'bicubic': {2: [-0.01171875, -0.03515625, 0.11328125, 0.43359375, 0.43359375, 0.11328125, -0.03515625, -0.01171875],
                4: [-0.00170898, -0.01098633, -0.01831055, -0.01196289, 0.02270508, 0.09741211, 0.18188477, 0.2409668,
                    0.2409668, 0.18188477, 0.09741211, 0.02270508, -0.01196289, -0.01831055, -0.01098633, -0.00170898]},
}


class Degradation:
    def __init__(self, kernel_size, scale_factor, type=0.0, theta=0.0, sigma=[1.0, 1.0]):
        if scale_factor not in (2, 4):
            raise ValueError("old_kernel_generator.Degradation: scale_factor=%r has no base kernel (2 or 4)" % (scale_factor,))
        if not (1 <= int(kernel_size) <= 21 and int(kernel_size) % 2 == 1):
            raise ValueError("old_kernel_generator.Degradation: kernel_size=%r must be odd and at most 21" % (kernel_size,))
        self.kernel_size = int(kernel_size)
        self.scale = int(scale_factor)
        self.b_kernel_size = 21
        self.type = type
        self.build_base_kernel()
        self.G_kernel_size = 21
        self.theta = float(theta)
        self.sigma = [float(sigma[0]), float(sigma[1])]
        self.build_G_kernel()
        self.kernel = self.convolve_kernel()

    def set_parameters(self, sigma, theta):
        self.sigma = sigma
        self.theta = theta

    def build_base_kernel(self):
        c = self.b_kernel_size // 2
        k1 = np.asarray(base_kernel_dict['impulse' if self.type < 0.5 else 'bicubic'][self.scale], dtype=np.float64)
        n = k1.shape[0]
        left, right = (n - 1) // 2, (n + 2) // 2
        kernel = np.zeros((self.b_kernel_size, self.b_kernel_size))
        kernel[c - left:c + right, c - left:c + right] = k1[:, None] * k1[None]
        self.basis_kernel = kernel / kernel.sum()

    def build_G_kernel(self):
        n = self.G_kernel_size
        sx, sy = self.sigma[0], self.sigma[1]
        if sx == 0 and sy == 0:          # delta kernel: the base kernel alone
            k = np.zeros((n, n))
            k[n // 2, n // 2] = 1
        else:
            r = n // 2
            ax = np.linspace(-r, r, n)
            xx, yy = np.meshgrid(ax, ax)
            ct, st = np.cos(self.theta), np.sin(self.theta)
            ix, iy = 1.0 / (2.0 * sx ** 2), 1.0 / (2.0 * sy ** 2)
            a = ct ** 2 * ix + st ** 2 * iy
            b = st * ct * (iy - ix)
            c = st ** 2 * ix + ct ** 2 * iy
            k = np.exp(-(a * xx ** 2 + 2.0 * b * xx * yy + c * yy ** 2))
            k = k / k.sum()
        self.Gaussian_kernel = k

    def convolve_kernel(self):
        """conv2d(base, Gaussian, padding=10) -- a correlation; the Gaussian is invariant under the 180-degree turn -- cropped to
        kernel_size about the centre and renormalised."""
        full = signal.correlate2d(self.basis_kernel, self.Gaussian_kernel, mode='same')
        c, r = full.shape[0] // 2, self.kernel_size // 2
        k = full[c - r:c + r + 1, c - r:c + r + 1]
        return np.ascontiguousarray(k / k.sum())

    def set_kernel_directly(self, kernel):
        self.kernel = np.asarray(kernel.detach().cpu() if torch.is_tensor(kernel) else kernel, dtype=np.float64)

    def get_kernel(self):
        return self.kernel

    def get_features(self):
        return np.reshape(self.kernel, (self.kernel_size ** 2,))

    def shifted_edge(self, index=0):
        """K, the edge of the kernel apply() convolves with: the kernel's own (nothing is shifted or padded).  Host code."""
        return int(self.kernel.shape[-1])

    def _shifted_on(self, device):
        """The kernel as a [1,K,K] fp32 device tensor, kept until the kernel (compared by value) changes."""
        key = (self.kernel.tobytes(), self.kernel.shape, str(device))
        if getattr(self, "_dev_key", None) != key:
            self._dev_val = torch.from_numpy(np.ascontiguousarray(self.kernel)).float().reshape(1, *self.kernel.shape).to(device)
            self._dev_key = key
        return self._dev_val

    def apply(self, img, quantise=False):
        if not img.is_cuda:
            raise RuntimeError("Degradation.apply runs on the GPU (libdynavsr_hip); there is no CPU fallback")
        single = img.dim() == 3          # one image C H W
        x = img[None] if single else img
        assert x.dim() == 4
        kt = self._shifted_on(x.device)
        n, c, h, w = x.shape
        kk, s = kt.shape[-1], int(self.scale)
        pad = kk // 2
        ho, wo = (h + 2 * pad - kk) // s + 1, (w + 2 * pad - kk) // s + 1
        x = x.float().contiguous()
        out = torch.empty((n, c, ho, wo), dtype=torch.float32, device=x.device)
        L.check(L.lib().dvsr_degrade_apply(L.ptr(x), L.ptr(kt), L.ptr(out), n, c, h, w, kk, s, 1, 0, 1 if quantise else 0,
                                           L.stream()), "degrade_apply")
        return out[0] if single else out
