"""The early-stopping contract of utils.fit_monitor.EarlyStopMonitor restated in numpy, fp64, two passes per window: the
reference of tests/test_early_stop_gpu.py and tests/test_early_stop_host.py (no test lives here).

Outputs x_0, x_1, ... of n floats, window W >= 2, patience P >= 1.  For t >= W - 1, while not stopped:
    mu_t = mean over the window x_{t-W+1..t};  var_t = sum |x - mu_t|^2 / (W n)
    var_t < var_min (strict): var_min = var_t, best_iter = t, wait = 0;   otherwise wait += 1 and wait >= P stops.
Rows: (var, var_min, best_iter, wait, stopped); warm-up rows (inf, inf, -1, 0, 0); rows after the stopping iteration repeat it."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)          # 2^-23


def window_variance(xs, t, window):
    """var_t: the fp64 two-pass variance over x_{t-window+1..t}, all elements."""
    w = np.asarray(xs[t - window + 1:t + 1], dtype=np.float64).reshape(window, -1)
    mu = w.mean(axis=0, dtype=np.float64)
    return float(((w - mu) ** 2).sum(dtype=np.float64) / w.size)


def wmv_reference(xs, window, patience):
    """(rows [T, 5] float64, stop_iter or None, margins): `margins` holds |var_t - var_min| / var_min of every comparison that
    was taken against a finite var_min (how far each decision is from a tie)."""
    T = len(xs)
    rows = np.zeros((T, 5), dtype=np.float64)
    var, var_min, best, wait, stopped, stop_iter = np.inf, np.inf, -1, 0, 0, None
    margins = []
    for t in range(T):
        if not stopped and t >= window - 1:
            var = window_variance(xs, t, window)
            if np.isfinite(var_min) and var_min > 0 and np.isfinite(var):
                margins.append(abs(var - var_min) / var_min)
            if var < var_min:
                var_min, best, wait = var, t, 0
            else:
                wait += 1
                if wait >= patience:
                    stopped, stop_iter = 1, t
        rows[t] = (var, var_min, best, wait, stopped)
    return rows, stop_iter, margins


def brute_force(xs, window, patience):
    """The same decisions from a plain loop over numpy's per-element variance of every window, averaged over the elements
    (no state carried but the decision's)."""
    vs = [np.inf if t < window - 1 else float(np.var(np.asarray(xs[t - window + 1:t + 1], dtype=np.float64), axis=0).mean())
          for t in range(len(xs))]
    best, wait = -1, 0
    for t, v in enumerate(vs):
        if t < window - 1:
            continue
        if best < 0 or v < vs[best]:
            best, wait = t, 0
        else:
            wait += 1
            if wait >= patience:
                return best, t
    return best, None


def sequence(shape, T=60, seed=0):
    """x_t = b + a_t N(0,1) in float32, b ~ U(0.2, 0.8) per element, a_t = 0.002 + 0.05 |t - 17| / 17: [T, n] float32.  The
    window variance falls until the window is centred on t = 17 and rises again."""
    n = int(np.prod(shape))
    rng = np.random.default_rng(seed)
    b = rng.uniform(0.2, 0.8, size=n)
    xs = np.empty((T, n), dtype=np.float32)
    for t in range(T):
        a = 0.002 + 0.05 * abs(t - 17) / 17.0
        xs[t] = (b + a * rng.standard_normal(n)).astype(np.float32)
    return xs
