"""The ring-free early-stopping contract (ES-EMV: utils.fit_monitor.EarlyStopMonitor(mode='emv'), dip_early_stop_emv_dev)
restated in numpy, fp64: the reference of tests/test_early_stop_emv_gpu.py, tests/test_group_early_stop_gpu.py and
tests/test_early_stop_emv_host.py (no test lives here).

Outputs x_0, x_1, ... of n floats, alpha in (0, 1), warmup >= 1, patience P >= 1:
    t = 0:                          mu = x_0, v = 0
    t >= 1, while not stopped:      d = x_t - mu;  mu += alpha d;  v = (1 - alpha) (v + alpha sum(d^2) / n)
    t >= warmup, while not stopped: var = v;  var < var_min (strict): var_min = var, best_iter = t, wait = 0;
                                    otherwise wait += 1 and wait >= P stops.
Rows: (var, var_min, best_iter, wait, stopped); rows before `warmup` are (inf, inf, -1, 0, 0); rows after the stopping iteration
repeat it."""
import numpy as np

import early_stop_ref as R

EPS32 = R.EPS32


def emv_reference(xs, alpha, warmup, patience, state=None):
    """(rows [T, 5] float64, stop_iter or None, margins), like early_stop_ref.wmv_reference: `margins` holds
    |var_t - var_min| / var_min of every comparison taken against a finite, positive var_min.  `state`: a dict that receives
    the final mu and v (frozen at the stopping iteration)."""
    T = len(xs)
    rows = np.zeros((T, 5), dtype=np.float64)
    var, var_min, best, wait, stopped, stop_iter = np.inf, np.inf, -1, 0, 0, None
    mu, v = None, 0.0
    margins = []
    for t in range(T):
        if not stopped:
            x = np.asarray(xs[t], dtype=np.float64).reshape(-1)
            if t == 0:
                mu, v = x.copy(), 0.0
            else:
                d = x - mu
                mu = mu + alpha * d
                v = (1.0 - alpha) * (v + alpha * float((d * d).sum(dtype=np.float64)) / x.size)
            if t >= warmup:
                var = v
                if np.isfinite(var_min) and var_min > 0 and np.isfinite(var):
                    margins.append(abs(var - var_min) / var_min)
                if var < var_min:
                    var_min, best, wait = var, t, 0
                else:
                    wait += 1
                    if wait >= patience:
                        stopped, stop_iter = 1, t
        rows[t] = (var, var_min, best, wait, stopped)
    if state is not None:
        state.update(mu=mu, v=v)
    return rows, stop_iter, margins


def group_sequence(shape, b):
    """S_b of the grouped tests: 60 outputs of early_stop_ref.sequence(shape, T=66, seed=b) from 3 b on, so that the amplitude's
    minimum -- and with it every instance's decisions -- falls on another iteration per instance."""
    return R.sequence(shape, T=66, seed=b)[3 * b:3 * b + 60]
