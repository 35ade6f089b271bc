"""The definition of the mean structural similarity that dip_ssim_dev implements (Wang, Bovik, Sheikh, Simoncelli 2004), restated
with torch on the CPU -- there is nothing else to compare against: the reference computes no SSIM.

    window      Gaussian 11 x 11, separable, g[k] = exp(-(k - 5)^2 / (2 * 1.5^2)) normalised to sum 1 in fp64
    constants   C1 = (0.01 * data_range)^2, C2 = (0.03 * data_range)^2
    moments     mu_x, mu_y, E[xx], E[yy], E[xy] by that filter over VALID positions only: (H - 10) x (W - 10) per channel
    covariances biased: s_xx = E[xx] - mu_x^2, ...
    map         S = ((2 mu_x mu_y + C1)(2 s_xy + C2)) / ((mu_x^2 + mu_y^2 + C1)(s_xx + s_yy + C2))
    ssim        the mean of S over all channels and valid positions

ssim_map(x, y, dtype) evaluates it in `dtype` with torch's conv2d (fp64: the truth; fp32: the yardstick of
test_kernels_gpu._check); model_fp32 is a numpy-float32 model of the kernel's order of operations (separable, fma chains,
optionally about a pivot)."""
import numpy as np
import torch
import torch.nn.functional as F

WIN, SIGMA, K1, K2 = 11, 1.5, 0.01, 0.03
HALO = WIN - 1


def taps64():
    """The 11 taps, normalised in fp64 (numpy float64)."""
    r = np.arange(WIN, dtype=np.float64) - (WIN // 2)
    g = np.exp(-(r * r) / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def taps32():
    """What the kernel holds: the fp64 taps rounded to fp32."""
    return taps64().astype(np.float32)


def constants(data_range=1.0):
    return (K1 * data_range) ** 2, (K2 * data_range) ** 2


def ssim_map(x, y, dtype=torch.float64, data_range=1.0, taps=None):
    """S as [1, C, H-10, W-10] in `dtype`; x, y are [1, C, H, W].  `taps`: None = the fp64 taps cast to `dtype`."""
    if x.shape != y.shape or x.dim() != 4 or x.shape[0] != 1:
        raise ValueError(f"ssim_ref: x and y are [1,C,H,W] of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.shape[2] < WIN or x.shape[3] < WIN:
        raise ValueError(f"ssim_ref: H and W must be >= {WIN}, got {tuple(x.shape[2:])}")
    g = torch.from_numpy(taps64() if taps is None else np.asarray(taps)).to(dtype)
    C = x.shape[1]
    w = (g[:, None] * g[None, :])[None, None].repeat(C, 1, 1, 1)
    f = lambda a: F.conv2d(a, w, groups=C)
    x, y = x.detach().cpu().to(dtype), y.detach().cpu().to(dtype)
    c1, c2 = constants(data_range)
    mx, my = f(x), f(y)
    sxx, syy, sxy = f(x * x) - mx * mx, f(y * y) - my * my, f(x * y) - mx * my
    return ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2))


def ssim(x, y, dtype=torch.float64, data_range=1.0):
    """The mean of the map, a python float."""
    return ssim_map(x, y, dtype, data_range).double().mean().item()


def _fma32(a, b, c):
    """fp32 fma of float32 arrays: the product of two floats is exact in fp64 (one more rounding of the sum at 2^-53)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def model_fp32(x, y, pivot=0.5, data_range=1.0):
    """The kernel's order of operations in numpy float32: x - pivot and y - pivot, their products rounded once, the horizontal
    then the vertical 11-tap fma chain in tap order for the five moments, mu = mu' + pivot, and the four factors of S from
    individually rounded operations.  pivot=None: no pivot.  Returns S as float32 [1, C, H-10, W-10]."""
    f32 = np.float32
    g = taps32()
    p = f32(0.0 if pivot is None else pivot)
    x, y = (x.detach().cpu().numpy().astype(f32) - p).astype(f32), (y.detach().cpu().numpy().astype(f32) - p).astype(f32)

    def filt(a):
        H, W = a.shape[-2:]
        h = np.zeros(a.shape[:-1] + (W - HALO,), f32)
        for k in range(WIN):
            h = _fma32(np.broadcast_to(g[k], h.shape), a[..., k:k + W - HALO], h)
        v = np.zeros(a.shape[:-2] + (H - HALO, W - HALO), f32)
        for k in range(WIN):
            v = _fma32(np.broadcast_to(g[k], v.shape), h[..., k:k + H - HALO, :], v)
        return v

    mx, my = filt(x), filt(y)
    sxx, syy, sxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
    mx, my = mx + p, my + p
    c1, c2 = (f32(c) for c in constants(data_range))
    return ((f32(2) * (mx * my) + c1) * (f32(2) * sxy + c2)) / (((mx * mx + my * my) + c1) * ((sxx + syy) + c2))


def inputs(C, H, W, kind, seed=0):
    """The input classes of the tests as (out, gt), [1, C, H, W] float32 in [0, 1]: 'noisy' a smooth image plus noise against
    itself plus more noise, 'flat' a constant output against a textured gt, 'constants' two different constants, 'equal'
    out == gt."""
    gen = torch.Generator().manual_seed(1000 * seed + 97 * C + 13 * H + W)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    gt = torch.stack([0.5 + 0.4 * torch.sin(6 * xx + 3 * yy + c) for c in range(C)])[None]
    gt = (gt + 0.05 * torch.randn(gt.shape, generator=gen)).clamp(0, 1).float()
    if kind == "noisy":
        return (gt + 0.1 * torch.randn(gt.shape, generator=gen)).clamp(0, 1).float(), gt
    if kind == "flat":
        return torch.full_like(gt, 0.7), gt
    if kind == "constants":
        return torch.full_like(gt, 0.7), torch.full_like(gt, 0.3)
    if kind == "equal":
        return gt.clone(), gt
    raise ValueError(kind)
