"""The SGLD step (dip_adam_sgld_step_dev, csrc/misc_kernels.hip) and the posterior monitor (dip_posterior_dev,
csrc/monitor_kernels.hip) restated: the key constant, the perturbation over a range table built on tests/noise_ref.py, the
numpy-float32 Welford update and the range table a parameter list must give (no test lives here).

    p[i] = fmaf(std, nrm(i), p1[i])    for i inside a range;    nrm(i) = normal i % 4 of Philox quad offset + i / 4 under key
    seed ^ KEY -- quads count from element 0 of the arena, whatever the table holds."""
import numpy as np

import noise_ref as R

KEY = 0x53474C4453474C44                   # "SGLDSGLD": the SGLD stream's key is seed ^ KEY (include/dip_hip.h)
MAX_RANGES = 512


def stream_seed(seed):
    """The reg-noise seed whose stream is the SGLD stream of `seed`."""
    return (int(seed) ^ KEY) & R.MASK64


def inside(n, ranges):
    """bool[n]: the elements that lie in one of the [begin, end) ranges (clipped to n)."""
    m = np.zeros(int(n), dtype=bool)
    for b, e in ranges:
        m[max(int(b), 0):min(int(e), int(n))] = True
    return m


def perturb(p1, ranges, std, seed, offset):
    """The float64 evaluation of the perturbation of the flat float32 array p1: p1 + float32(std) * normals inside the ranges,
    p1 elsewhere (the kernel rounds the fma once to float32; its normals are the reg-noise kernel's, pinned by
    tests/test_noise_gpu.py)."""
    p1 = np.asarray(p1, dtype=np.float32).reshape(-1)
    nrm = R.normals(p1.size, stream_seed(seed), offset)
    out = p1.astype(np.float64)
    m = inside(p1.size, ranges)
    out[m] += float(np.float32(std)) * nrm[m]
    return out


def welford(mean, m2, x, k):
    """One sample: d = x - mean; mean' = mean + d / k; m2' = m2 + d * (x - mean'), k = the sample's number (1 for the first)
    as a float32, every operation rounded to float32 on its own (numpy float32 arrays do exactly that)."""
    mean, m2, x = (np.asarray(a, dtype=np.float32) for a in (mean, m2, x))
    k = np.float32(k)
    d = x - mean
    mean2 = mean + d / k
    return mean2, m2 + d * (x - mean2)


def is_sample(i, burn_in, every):
    return i >= burn_in and (i - burn_in) % every == 0


def expected_ranges(params, noised=None):
    """The table of a parameter list laid out like the engine's arena (every slot rounded up to four floats, in list order):
    the extents of the 4-D parameters (or of `noised`, by identity), merged where one ends exactly where the next begins."""
    ids = None if noised is None else {id(p) for p in noised}
    out, off = [], 0
    for p in params:
        n = p.numel()
        take = p.dim() == 4 if ids is None else id(p) in ids
        if take:
            if out and out[-1][1] == off:
                out[-1] = (out[-1][0], off + n)
            else:
                out.append((off, off + n))
        off += (n + 3) // 4 * 4
    return out
