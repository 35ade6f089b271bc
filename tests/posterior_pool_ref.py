"""dip_posterior_pool (csrc/monitor_kernels.hip) and the record of dip_posterior_rec_dev restated in numpy, and the textbook
formula they are held to (no test lives here).

Pooling C chains of k samples each (Gelman & Rubin 1992; BDA3 section 11.4), per element, from the chains' Welford rows
mean_c and m2_c -- numpy float32 arrays round every operation on its own, as the kernel does:

    s = 0;  for c: s = s + mean_c          mu = s / (float)C
    w = 0;  for c: w = w + m2_c            W  = w / (float)(C * (k - 1))
    q = 0;  for c: d = mean_c - mu; q = q + d * d        Bk = q / (float)(C - 1)
    f = (float)(k - 1) / (float)k          V  = f * W + Bk
    R = sqrt(V / W);   !(W > 0): degenerate, R = NaN, left out of the summary"""
import numpy as np

F = np.float32


def pool(mean, m2, k, chains=None):
    """(mu, V, W, R, summary) of the rows `chains` (default: all, in order) of mean / m2 ([rows, n] float32): float32 arrays
    [n] and summary = float64 [mean of R over the non-degenerate elements, their max, the number of degenerate ones]."""
    mean, m2 = np.asarray(mean, dtype=F), np.asarray(m2, dtype=F)
    chains = list(range(mean.shape[0])) if chains is None else list(chains)
    C, n = len(chains), mean.shape[1]
    s, w, q = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
    for c in chains:
        s = s + mean[c]
        w = w + m2[c]
    mu = s / F(C)
    W = w / F(C * (k - 1))
    for c in chains:
        d = mean[c] - mu
        q = q + d * d
    Bk = q / F(C - 1)
    f = F(k - 1) / F(k)
    V = f * W + Bk
    good = W > 0
    R = np.full(n, np.nan, F)
    with np.errstate(all="ignore"):
        R[good] = np.sqrt(V[good] / W[good])
    assert all(a.dtype == F for a in (mu, V, W, R))
    r64 = R[good].astype(np.float64)
    summary = np.array([r64.sum() / good.sum() if good.any() else np.nan, r64.max() if good.any() else np.nan,
                        n - good.sum()], dtype=np.float64)
    return mu, V, W, R, summary


def chain_rows(x):
    """The rows of raw samples x [C, k, n] in float64: every chain's mean and sum of squared deviations, [C, n] each."""
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(axis=1)
    return mean, ((x - mean[:, None, :]) ** 2).sum(axis=1)


def textbook(x):
    """(mu, V, W, R) of raw samples x [C, k, n], in float64: W the mean of the chains' sample variances, B / k the sample
    variance of the chains' means, V = (k - 1) / k W + B / k, R = sqrt(V / W)."""
    x = np.asarray(x, dtype=np.float64)
    C, k, n = x.shape
    W = x.var(axis=1, ddof=1).mean(axis=0)
    Bk = x.mean(axis=1).var(axis=0, ddof=1)
    V = (k - 1) / k * W + Bk
    return x.mean(axis=(0, 1)), V, W, np.sqrt(V / W)


def synthetic(rng, C, k, n):
    """x[c, j, i] = base_i + off_c + e_ci + eps_cji: C chains of k samples around one image, the chains' means apart by a
    common offset N(0, 0.02) and a per-element one N(0, 0.01), the samples N(0, 0.03) around their chain's mean."""
    base = rng.uniform(0.05, 0.95, n)
    off = rng.normal(0.0, 0.02, C)
    e = rng.normal(0.0, 0.01, (C, n))
    x = np.empty((C, k, n), dtype=np.float64)
    for c in range(C):
        x[c] = base + off[c] + e[c] + rng.normal(0.0, 0.03, (k, n))
    return x


def record(iteration, mean, gt):
    """Row {iteration, mse_mean, psnr_mean} of dip_posterior_rec_dev from the stored float32 mean and the ground truth: the sum
    of squared errors in float64, every column rounded once to float32."""
    e = np.asarray(mean, dtype=F).astype(np.float64).reshape(-1) - np.asarray(gt, dtype=F).astype(np.float64).reshape(-1)
    mse = float((e * e).sum()) / e.size
    return np.array([F(iteration), F(mse), F(-10.0 * np.log10(mse))], dtype=F)
