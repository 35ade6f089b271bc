"""Device-side bookkeeping for the notebooks' closures (no counterpart file in the reference: the reference does this work
inline, on the host, in every closure -- denoising.ipynb:214-248 (FitMonitor), super-resolution.ipynb:188-191 (SRFitMonitor),
restoration.ipynb:192-211 (RestorationFitMonitor): an `out.detach().cpu()` and a synchronisation per PSNR and iteration, and
a copy of all parameters to the CPU per checkpoint).  Four kinds of record; each is one streaming pass over the output, a
one-block finalize and -- where the closure has one -- a conditional copy of the flat parameter arena.  Nothing synchronises;
the host reads the record table when it wants to print.

    FitMonitor             dip_fit_monitor_dev: EMA of the output, three PSNRs, the 5 dB fall-back BETWEEN the show_every-th
                           iterations; columns loss, mse_noisy, mse_gt, mse_gt_sm, psrn_noisy, psrn_gt, psrn_gt_sm, fell_back
    SRFitMonitor           dip_sr_monitor_dev: psnr_LR / psnr_HR from the two outputs of utils.loss_head.SRHead; columns loss,
                           mse_LR, mse_HR, psnr_LR, psnr_HR (img_HR is optional)
    RestorationFitMonitor  dip_restore_monitor_dev: psrn_masked / psrn, the fall-back ON every show_every-th iteration; columns
                           loss, mse_masked, mse, psrn_masked, psrn, fell_back
    EarlyStopMonitor       no notebook decides WHEN to stop; this is the ground-truth-free criterion of Wang et al., "Early
                           Stopping for Deep Image Prior": stop after `patience` iterations without a new minimum of the moving
                           variance of the output, keep the minimum's output and parameters.  'wmv' (dip_early_stop_dev): over
                           a ring of the last `window` outputs, 4 * window * n bytes; 'emv' (dip_early_stop_emv_dev): the
                           exponential form, no ring.  Columns var, var_min, best_iter, wait, stopped
    PosteriorMonitor       no notebook has it either: the sample mean and variance of the outputs of an SGLD fit (Cheng et al.,
                           "A Bayesian Perspective on the Deep Image Prior"; dip_optim.FusedAdam(noise_std=)) after a burn-in,
                           dip_posterior_dev: mean, variance(), count.  img_gt=: dip_posterior_rec_dev, one record per SAMPLE;
                           columns iteration, mse_mean, psnr_mean (the PSNR of the posterior mean)
    SSIMMonitor            nor this: the mean structural similarity of the output against a ground truth (and of a smoothed
                           output, img_avg=), dip_ssim_dev; columns ssim, ssim_sm.  ssim(x, y) is the one-shot function

In the eager closure, after backward():

    monitor = FitMonitor(net, img_noisy_torch, img_torch, exp_weight=0.99, show_every=100)
    def closure():
        out = net(net_input_saved + noise.normal_() * reg_noise_std)
        total_loss = mse(out, img_noisy_torch)
        total_loss.backward()
        monitor.update(out, total_loss)          # no host sync (SRFitMonitor: mon.update(out_HR, head.out_LR, total_loss))
        return total_loss
    optimize('adam', p, closure, LR, num_iter)
    hist = monitor.history()                     # [iters, 8] numpy, ONE device->host copy
    out_avg = monitor.out_avg                    # the smoothed output (1 x C x H x W, on the GPU)

    mon = SRFitMonitor(img_LR_var, img_HR_var, capacity=num_iter)
    mon = RestorationFitMonitor(net, img_var, mask_var, show_every=50, capacity=num_iter)
    es = EarlyStopMonitor(img_noisy_torch, window=100, patience=1000, net=net, capacity=num_iter)     # es.update(out)
    es = EarlyStopMonitor(img_noisy_torch, patience=1000, net=net, capacity=num_iter, mode='emv', alpha=0.1)
    sm = SSIMMonitor(img_torch, img_avg=monitor.out_avg, capacity=num_iter)                           # sm.update(out)

Inside the autograd-free iteration (no Python between the iterations) the same entry points read the iteration index from device
memory (`monitor.counter`); `monitor.i` stays the host's count, and the two forms may alternate at any iteration boundary:

    it = NativeIteration(net, head, opt, net_input, reg_noise=reg, monitor=monitor, early_stop=es)
    it.run(show_every); print(monitor.last())    # the notebook's print loop
    issued, losses = it.run_until(num_iter, check_every=50)                         # one 4-byte read per 50 iterations
    es.best_iter, es.best_out; es.restore_best()                                    # the net carries the minimum's parameters

B fits through one launch list (dip_group.GroupedFits) take the Grouped* form of a kind: settings only, until the group adopts
it (once) and carves its buffers from the slab rows.  ONE call per entry point then serves all B inside the one hipGraph, and
every instance takes its own decisions:

    mon = GroupedFitMonitor(imgs_gt, exp_weight=0.99, show_every=100, capacity=num_iter)
    es = GroupedEarlyStopMonitor(mode='emv', alpha=0.1, patience=1000, capacity=num_iter)
    g = GroupedFits(nets, net_inputs, imgs_noisy, reg_noise_std=1/30, monitor=mon, early_stop=es)
    g.capture(); issued = g.run_until(num_iter - 3, check_every=50)                 # until ALL instances have stopped
    hist = mon.history()                         # [B, iters, 8] numpy, ONE device->host copy
    mon.last()[b]["psrn_gt_sm"]; mon.out_avg[b]; es.best_iter, es.stopped, es.best_out[b]; es.restore_best()

    mon = GroupedSRFitMonitor(imgs_HR, capacity=num_iter)                           # GroupedFits(..., downsamplers=downs)
    mon = GroupedRestorationFitMonitor(show_every=50, capacity=num_iter)            # GroupedFits(..., masks=masks)
    sm = GroupedSSIMMonitor(imgs_gt, capacity=num_iter)                             # GroupedFits(..., ssim=sm), any group kind
    pm = GroupedPosteriorMonitor(burn_in, every, imgs_gt=None)                      # GroupedFits(..., posterior=pm), any group kind
    pm.mean, pm.variance(), pm.count; pm.pooled(chains=None).rhat                   # B chains pooled: dip_posterior_pool

A kind's device buffers are declared ONCE, in its table below (FIT_BUFFERS ...): the solo monitor allocates them, the group
carves them from its slab and views them, and the plan's key and keep-alive list name them, all from that table.
"""
import ctypes as C
import weakref
from types import SimpleNamespace
from typing import Callable, NamedTuple, Optional

import numpy as np
import torch

import dip_native as N


_ptr = lambda t: None if t is None else t.data_ptr()
_F32, _F64, _I32 = torch.float32, torch.float64, torch.int32


# ---------------------------------------------------------------- the buffers of every kind, said once
class Buf(NamedTuple):
    """One device buffer of a monitor kind.  The functions take `z`, the sizes (monitor_sizes), or `m`, the monitor."""
    name: str                           # the solo monitor's attribute, the grouped monitor's [B, ...] view, the descriptor's field
    count: Callable                     # count(z): elements
    shape: Optional[Callable] = None    # shape(z) of one instance (None: flat); a group's view is [B, *shape(z)]
    dtype: torch.dtype = _F32
    init: str = "empty"                 # 'empty', 'zero', 'early_stop' (early_stop_state_fill) or 'given': the caller's image
    when: Callable = lambda m: True     # when(m): does monitor m have it?  ('given': asked of the grouped monitor only)
    lazy: bool = False                  # a solo monitor allocates it at first use, when its size is known (_ensure_*)
    key: Optional[str] = None           # a group's name for it behind 'mon_' / 'es_' (None: `name`)
    view: bool = True                   # a grouped monitor exposes it


def monitor_sizes(m, nblk, n, img, one, n_lr=None, n_arena=None):
    """The sizes the tables are evaluated on: n / n_lr elements of the net output / the LR image, n_arena of the parameter
    arena, `img` the shape of an output-sized buffer and `one` that of a scalar (a solo monitor: (1, C, H, W) and (1,); a
    group, in front of which B goes: (C, H, W) and ()), nblk = dip_fit_monitor_nblk."""
    return SimpleNamespace(n=n, n_lr=n_lr, n_arena=n_arena, capacity=m.capacity, window=getattr(m, "window", None),
                           img=tuple(img), one=one, nblk=nblk)


_records = lambda ncol: Buf("records", lambda z: z.capacity * ncol, lambda z: (z.capacity, ncol), init="zero")
_COUNTER = Buf("counter", lambda z: 1, lambda z: z.one, _I32, "zero")       # the row index the *_dev entry points read
_STATE = Buf("state", lambda z: 4, init="zero")                            # [psnr_last, restore, have_last, snapshot]
_SNAPSHOT = Buf("snapshot", lambda z: z.n_arena, when=lambda m: m.backtracking, lazy=True)
_image = lambda name, key, when: Buf(name, lambda z: z.n, lambda z: z.img, init="given", when=when, key=key, view=False)

FIT_BUFFERS = (_image("gt", "gt", lambda m: m.imgs_gt is not None),
               Buf("out_avg", lambda z: z.n, lambda z: z.img, init="zero", key="avg"),
               Buf("partial", lambda z: 4 * z.nblk(z.n), view=False),
               _records(8), _STATE, _COUNTER, _SNAPSHOT)
SR_BUFFERS = (_image("img_HR", "hr", lambda m: m.imgs_HR is not None),
              Buf("partial", lambda z: z.nblk(z.n) + z.nblk(z.n_lr), lazy=True, view=False),   # (n: known with the first output)
              _records(5), _COUNTER)
RESTORE_BUFFERS = (Buf("partial", lambda z: 2 * z.nblk(z.n), view=False), _records(6), _STATE, _COUNTER, _SNAPSHOT)
EARLY_STOP_BUFFERS = (Buf("ring", lambda z: z.window * z.n, lambda z: (z.window, z.n), when=lambda m: m.mode == "wmv"),
                      Buf("mean", lambda z: z.n, dtype=_F64),
                      Buf("partial", lambda z: z.nblk(z.n), dtype=_F64),
                      _records(5),
                      Buf("state", lambda z: 16, dtype=_I32, init="early_stop"),
                      _COUNTER,
                      Buf("best_out", lambda z: z.n, lambda z: z.img, init="zero"),
                      Buf("best_params", lambda z: z.n_arena, init="zero", when=lambda m: m.keep_params, lazy=True))
POSTERIOR_BUFFERS = (Buf("mean", lambda z: z.n, lambda z: z.img, init="zero"),
                     Buf("m2", lambda z: z.n, lambda z: z.img, init="zero"),
                     Buf("samples", lambda z: 1, lambda z: z.one, _I32, "zero"),          # the descriptor's `count`
                     _COUNTER)
# (with a ground truth -- img_gt= / imgs_gt= -- three more, behind the four: the PSNR of the posterior mean, one row per SAMPLE)
POSTERIOR_REC_BUFFERS = POSTERIOR_BUFFERS + (_image("gt", "gt", lambda m: True),
                                             Buf("partial", lambda z: z.nblk(z.n), dtype=_F64, view=False),
                                             _records(3))
_ssim_valid = lambda z: (*z.img[:-2], z.img[-2] - 10, z.img[-1] - 10)         # the valid positions of an 11 x 11 window
SSIM_BUFFERS = (_image("gt", "gt", lambda m: True),
                Buf("map", lambda z: int(np.prod(_ssim_valid(z))), _ssim_valid, when=lambda m: m.keep_map),
                Buf("partial", lambda z: 2 * N.lib().dip_ssim_nblk(*z.img[-3:]), view=False),     # (out and avg: a row each)
                _records(2), _COUNTER)


# ---------------------------------------------------------------- descriptors and launches
# One descriptor function per kind: `m` carries the settings, the mapping `t` the buffers by name -- the table's, and what the
# caller brings: out (/ out_LR), the images, loss.  A solo monitor passes its attributes, a group its slab rows.
def fit_monitor_descriptor(m, t):
    p = lambda k: _ptr(t.get(k))
    return N.DipFitMonitorDesc(p("out"), p("noisy"), p("gt"), p("out_avg"), t["noisy"].numel(), m.exp_weight, m.backtrack_db,
                               p("loss"), p("partial"), p("records"), m.capacity, m.show_every, 1 if m.backtracking else 0, 0,
                               p("counter"), p("state"))


def sr_monitor_descriptor(m, t):
    p = lambda k: _ptr(t.get(k))
    return N.DipSRMonitorDesc(p("out"), p("out_LR"), p("img_HR"), p("img_LR"), t["out"].numel(), t["img_LR"].numel(), p("loss"),
                              p("partial"), p("records"), m.capacity, 0, p("counter"))


def restore_monitor_descriptor(m, t):
    """`mask` is [mask_c][hw], out / img are planes of hw."""
    p = lambda k: _ptr(t.get(k))
    return N.DipRestoreMonitorDesc(p("out"), p("img"), p("mask"), t["img"].numel(), int(t["hw"]), int(t["mask_c"]), m.backtrack_db,
                                   p("loss"), p("partial"), p("records"), m.capacity, m.show_every, 1 if m.backtracking else 0, 0,
                                   p("counter"), p("state"))


def early_stop_descriptor(m, t):
    """DipEarlyStopDesc ('wmv') of monitor m (window, patience, capacity)."""
    p = lambda k: _ptr(t.get(k))
    return N.DipEarlyStopDesc(p("out"), p("ring"), p("mean"), p("partial"), p("records"), p("state"), p("counter"),
                              p("best_out"), t["out"].numel(), m.window, m.patience, m.capacity, p("loss"))


def early_stop_emv_descriptor(m, t):
    """DipEarlyStopEmvDesc of monitor m (alpha, warmup, patience, capacity): no ring, no loss."""
    p = lambda k: _ptr(t.get(k))
    return N.DipEarlyStopEmvDesc(p("out"), p("mean"), p("partial"), p("records"), p("state"), p("counter"), p("best_out"),
                                 t["out"].numel(), m.alpha, m.warmup, m.patience, m.capacity, 0)


def posterior_descriptor(m, t):
    """DipPosteriorDesc of monitor m (burn_in, every): mean, m2, the sample count and the iteration counter; with a ground truth
    DipPosteriorRecDesc: the same and gt, the fp64 partials and the record table of `capacity` sample rows."""
    p = lambda k: _ptr(t.get(k))
    head = (p("out"), p("mean"), p("m2"), p("samples"), p("counter"), t["out"].numel(), m.burn_in, m.every)
    if not m.with_gt:
        return N.DipPosteriorDesc(*head)
    return N.DipPosteriorRecDesc(*head, p("gt"), p("partial"), p("records"), m.capacity, 0)


SSIM_WIN, SSIM_K1, SSIM_K2 = 11, 0.01, 0.03


def ssim_descriptor(m, t):
    """DipSsimDesc of monitor m (chw, data_range, with_avg, capacity): out, the optional second source `avg`, gt, the optional
    map; c1 = (K1 data_range)^2, c2 = (K2 data_range)^2 and the pivot data_range / 2.  No `counter` in t: the functional form."""
    p = lambda k: _ptr(t.get(k))
    Cc, H, W = (int(s) for s in m.chw)
    return N.DipSsimDesc(p("out"), p("avg") if m.with_avg else None, p("gt"), p("map"), p("partial"), p("records"), p("counter"),
                         m.capacity, Cc, H, W, (SSIM_K1 * m.data_range) ** 2, (SSIM_K2 * m.data_range) ** 2,
                         0.5 * m.data_range, N.lib().dip_ssim_nblk(Cc, H, W))


_ENTRY = {N.DipFitMonitorDesc: "fit_monitor_dev", N.DipSRMonitorDesc: "sr_monitor_dev",
          N.DipRestoreMonitorDesc: "restore_monitor_dev", N.DipEarlyStopDesc: "early_stop_dev",
          N.DipEarlyStopEmvDesc: "early_stop_emv_dev", N.DipPosteriorDesc: "posterior_dev",
          N.DipPosteriorRecDesc: "posterior_rec_dev", N.DipSsimDesc: "ssim_dev"}


def monitor_launches(lib, desc, params_ptr=None, n_arena=0, arena_ptr=None):
    """The device-indexed entry point of `desc` and, with an arena of the kind (snapshot; best_params), the conditional copy
    between it and the parameter arena -- dip_arena_backtrack, or dip_early_stop_keep -- as (fn, args, name) triples."""
    name = _ENTRY[type(desc)]
    ops = [(getattr(lib, "dip_" + name), (C.byref(desc),), name)]
    if arena_ptr is not None:
        copy = "early_stop_keep" if name.startswith("early_stop") else "arena_backtrack"
        ops.append((getattr(lib, "dip_" + copy), (params_ptr, arena_ptr, n_arena, desc.state), copy))
    return ops


fit_monitor_launches = restore_monitor_launches = early_stop_launches = monitor_launches


def _mask4(mask, C_out, hw_shape, who):
    """`mask` as a contiguous fp32 [1, 1|C_out, H, W] tensor: the rule of utils.loss_head.MSEHead(mask=)."""
    m = mask.detach().float()
    while m.dim() < 4:
        m = m[None]
    if m.shape[0] != 1 or m.shape[1] not in (1, C_out) or tuple(m.shape[2:]) != tuple(hw_shape):
        raise ValueError(f"dip-amd: {who}: mask must be [1,1|{C_out},{hw_shape[0]},{hw_shape[1]}], got {tuple(m.shape)}")
    return m.contiguous()


def early_stop_state(dev):
    """The 64-byte state of dip_early_stop_dev before the first iteration, as int32[16]: var_min = var = +inf (double[1],
    double[2]), best_iter = -1 (int32[9]), everything else zero."""
    return early_stop_state_fill(torch.zeros(16, dtype=torch.int32, device=dev))


def early_stop_state_fill(st):
    """Writes that state into `st` (int32[16], 8-byte aligned; a row of a group's slab) and returns it."""
    st.zero_()
    st.view(torch.float64)[1:3] = float("inf")
    st[9] = -1
    return st


def _early_stop_settings(who, mode, window, alpha, warmup, patience, capacity):
    """(mode, window, alpha, warmup, patience, capacity) of an early-stopping monitor, or the ValueError that says what is
    wrong: needs no GPU.  `window` belongs to 'wmv' and is not looked at in 'emv'; warmup=None is ceil(2 / alpha) -- v starts
    at zero and ramps up for about 1 / alpha iterations, and a decision taken on the ramp is a false minimum."""
    if mode not in ("wmv", "emv"):
        raise ValueError(f"dip-amd: {who}: mode is 'wmv' (windowed moving variance) or 'emv' (exponential moving variance), "
                         f"got {mode!r}")
    if mode == "wmv" and int(window) < 2:
        raise ValueError(f"dip-amd: {who}: window must be >= 2, got {window}")
    if int(patience) < 1:
        raise ValueError(f"dip-amd: {who}: patience must be >= 1, got {patience}")
    if int(capacity) < 1 or int(capacity) > 2 ** 24:
        raise ValueError(f"dip-amd: {who}: capacity must be in [1, 2**24] (best_iter is a float32 column), got "
                         f"{capacity}")
    if not 0.0 < float(alpha) < 1.0:                                # (a NaN compares false)
        raise ValueError(f"dip-amd: {who}: alpha must be in (0, 1), got {alpha}")
    if warmup is None:
        warmup = int(np.ceil(2.0 / float(alpha)))
    if int(warmup) < 1 or int(warmup) > 2 ** 24:
        raise ValueError(f"dip-amd: {who}: warmup must be in [1, 2**24], got {warmup}")
    return mode, int(window), float(alpha), int(warmup), int(patience), int(capacity)


def _ssim_settings(who, img, data_range=1.0, capacity=1):
    """(chw, data_range, capacity) of an SSIM over images shaped like `img`, or the error that says what is wrong: needs no GPU."""
    if not isinstance(img, torch.Tensor):
        raise TypeError(f"dip-amd: {who}: the images are tensors shaped like the net output ([1,C,H,W]), got {type(img).__name__}")
    if img.dim() != 4 or img.shape[0] != 1 or img.shape[1] < 1:
        raise ValueError(f"dip-amd: {who}: the images must be [1,C,H,W], got {tuple(img.shape)}")
    if img.shape[2] < SSIM_WIN or img.shape[3] < SSIM_WIN:
        raise ValueError(f"dip-amd: {who}: H and W must be >= {SSIM_WIN} (the {SSIM_WIN} x {SSIM_WIN} window is applied at valid "
                         f"positions only), got {tuple(img.shape[2:])}")
    if not 0.0 < float(data_range) < float("inf"):                  # (a NaN compares false)
        raise ValueError(f"dip-amd: {who}: data_range must be positive and finite, got {data_range}")
    if int(capacity) < 1:
        raise ValueError(f"dip-amd: {who}: capacity must be > 0, got {capacity}")
    return tuple(int(s) for s in img.shape[1:]), float(data_range), int(capacity)


# ---------------------------------------------------------------- the kinds: what a solo and a grouped monitor share
class _FitKind:
    COLUMNS = ("loss", "mse_noisy", "mse_gt", "mse_gt_sm", "psrn_noisy", "psrn_gt", "psrn_gt_sm", "fell_back")
    BUFFERS, ARENA, _descriptor = FIT_BUFFERS, ("snapshot", torch.empty_like), fit_monitor_descriptor
    head_kind = None                                                # any head: the record needs the net output only


class _SRKind:
    COLUMNS = ("loss", "mse_LR", "mse_HR", "psnr_LR", "psnr_HR")
    BUFFERS, ARENA, _descriptor = SR_BUFFERS, None, sr_monitor_descriptor
    head_kind = "sr"                                                # the record needs the two outputs of an SRHead


class _RestoreKind:
    COLUMNS = ("loss", "mse_masked", "mse", "psrn_masked", "psrn", "fell_back")
    BUFFERS, ARENA, _descriptor = RESTORE_BUFFERS, ("snapshot", torch.empty_like), restore_monitor_descriptor
    head_kind = None


class _EarlyStopKind:
    COLUMNS = ("var", "var_min", "best_iter", "wait", "stopped")
    BUFFERS, ARENA = EARLY_STOP_BUFFERS, ("best_params", torch.zeros_like)
    head_kind = None

    def _descriptor(self, t):
        return (early_stop_emv_descriptor if self.mode == "emv" else early_stop_descriptor)(self, t)

    @property
    def memory_bytes(self):
        """Device memory the monitor holds, per instance times B ('wmv': the ring dominates, 4 * window * n; 'emv' has none)."""
        self._table()
        return sum(t.numel() * t.element_size() for t in self._buffers() if t is not None)


class _PosteriorKind:
    COLUMNS = ()                                                    # no record table: mean, m2 and the sample count
    REC_COLUMNS = ("iteration", "mse_mean", "psnr_mean")            # with a ground truth: one row per SAMPLE
    BUFFERS, ARENA, _descriptor = POSTERIOR_BUFFERS, None, posterior_descriptor
    head_kind = None
    with_gt = False
    MAX_SAMPLES = 2 ** 24
    MAX_ITER = 2 ** 31 - 1                                          # the int32 iteration index

    def _init_posterior(self, burn_in, every, with_gt, capacity):
        """(what needs no GPU: the settings) -> the capacity of _init_count: the record rows with a ground truth, else the
        iteration index's range.  A monitor with a ground truth takes the longer table and the columns as its own."""
        who = type(self).__name__
        if int(burn_in) < 0:
            raise ValueError(f"dip-amd: {who}: burn_in must be >= 0, got {burn_in}")
        if int(every) < 1:
            raise ValueError(f"dip-amd: {who}: every must be >= 1, got {every}")
        if with_gt and not 1 <= int(capacity) <= self.MAX_SAMPLES:
            raise ValueError(f"dip-amd: {who}: capacity (sample rows of the record table) must be in [1, 2**24], got {capacity}")
        self.burn_in, self.every, self.with_gt = int(burn_in), int(every), bool(with_gt)
        if self.with_gt:
            self.BUFFERS, self.COLUMNS = POSTERIOR_REC_BUFFERS, self.REC_COLUMNS
        return int(capacity) if self.with_gt else self.MAX_ITER

    def samples_after(self, i):
        """How many of the iterations [0, i) are samples."""
        return 0 if i <= self.burn_in else (i - self.burn_in - 1) // self.every + 1

    def _check_room(self, n):
        """Refuses n more iterations when they would pass the sample cap (or the int32 index), or the record table of a monitor
        with a ground truth: before anything is issued."""
        who, k = type(self).__name__, self.samples_after(self.i + int(n))
        if k > self.MAX_SAMPLES or self.i + int(n) > self.MAX_ITER:
            raise RuntimeError(f"dip-amd: {who}: {int(n)} more iteration(s) after {self.i} would pass the cap of "
                               f"2**24 samples (burn_in {self.burn_in}, every {self.every}); sample less often")
        if self.with_gt and k > self.capacity:
            raise RuntimeError(f"dip-amd: {who} capacity exceeded ({int(n)} more iteration(s) after {self.i} make {k} samples > "
                               f"capacity {self.capacity}); construct it with capacity >= the number of samples")

    def history(self):
        """The records of the samples so far as a [count, 3] float32 numpy array (a grouped monitor: [B, count, 3]): iteration,
        mse_mean, psnr_mean of the posterior mean against the ground truth; one device->host copy, synchronises once."""
        return self._table()[..., :self.samples_after(self.i), :].contiguous().cpu().numpy()

    def last(self):
        """The latest sample's record as a dict keyed by COLUMNS (a grouped monitor: a list of B dicts); synchronises."""
        k = self.samples_after(self.i)
        if k < 1:
            raise RuntimeError(f"dip-amd: {type(self).__name__}.last(): no sample has been taken yet")
        r = self._table()[..., k - 1, :].contiguous().cpu().numpy()
        rows = [dict(zip(self.COLUMNS, (float(x) for x in row))) for row in r.reshape(-1, len(self.COLUMNS))]
        return rows if r.ndim > 1 else rows[0]


class _SSIMKind:
    COLUMNS = ("ssim", "ssim_sm")
    BUFFERS, ARENA, _descriptor = SSIM_BUFFERS, None, ssim_descriptor
    head_kind = None                                                # either head: the record needs the net output only


class _Records:
    """What every monitor has: a record table of `capacity` rows of COLUMNS in device memory ([capacity, columns]; a grouped
    monitor: [B, capacity, columns]) and the host's count `i` of recorded iterations."""
    COLUMNS, BUFFERS = (), ()

    def _init_count(self, capacity):
        self.capacity = int(capacity)
        self.i = 0

    def _check_room(self, n):
        """Refuses n more iterations when they do not fit: before anything is issued -- eager, native or replayed."""
        if self.i + int(n) > self.capacity:
            raise RuntimeError(f"dip-amd: {type(self).__name__} capacity exceeded ({self.i} recorded + {int(n)} > capacity "
                               f"{self.capacity}); construct it with capacity >= num_iter")

    def _buf(self, name):
        return next(b for b in self.BUFFERS if b.name == name)

    def _buffers(self):
        """The table's buffers as this monitor holds them (None: absent, or not allocated yet)."""
        return [getattr(self, b.name) for b in self.BUFFERS]

    def _table(self, need=0):
        return self.records

    def history(self):
        """All records so far as a [iters, len(COLUMNS)] float32 numpy array (a grouped monitor: [B, iters, len(COLUMNS)]);
        one device->host copy, synchronises once."""
        return self._table()[..., :self.i, :].contiguous().cpu().numpy()

    def last(self):
        """The latest record as a dict keyed by COLUMNS (a grouped monitor: a list of B dicts); synchronises."""
        r = self._table(1)[..., self.i - 1, :].contiguous().cpu().numpy()
        rows = [dict(zip(self.COLUMNS, (float(x) for x in row))) for row in r.reshape(-1, len(self.COLUMNS))]
        return rows if r.ndim > 1 else rows[0]


# ---------------------------------------------------------------- one fit
class _DeviceRecords(_Records):
    """What the solo monitors share: the table's buffers as torch tensors, the eager update(), the device counter the *_dev
    entry points index the record table with, and what dip_optim.NativeIteration asks of a monitor (_plan, _plan_key,
    _plan_keep, _sync_counter, _advance).  A kind supplies _check_update / _issue (the eager form) and _check_plan."""
    INPUTS = ()            # the caller's tensors the descriptor points at, besides the table's
    SETTINGS = ()          # what else a descriptor is filled from, by value
    engine = None          # the net's engine when the monitor copies its flat parameter arena (_init_backtracking)

    def _init_device(self, dev, capacity, img, **sizes):
        """Allocates the table's buffers on `dev`, but for the caller's images and what is allocated at first use."""
        self.lib = N.lib()
        self.dev = dev
        self._init_count(capacity)
        self._z = z = monitor_sizes(self, self.lib.dip_fit_monitor_nblk, img=img, one=(1,), **sizes)
        for b in self.BUFFERS:
            if b.init == "given":
                continue
            t = None
            if not b.lazy and b.when(self):
                make = torch.zeros if b.init == "zero" else torch.empty
                t = early_stop_state(dev) if b.init == "early_stop" else \
                    make(b.shape(z) if b.shape else b.count(z), dtype=b.dtype, device=dev)
            setattr(self, b.name, t)
        # `counter` is the iteration index as the *_dev kernels read it (NativeIteration), _counter_host the value it will
        # hold once all issued work has run; a by-value update() leaves both alone, NativeIteration re-aligns them
        self._counter_host = 0

    def _init_backtracking(self, net, backtracking):
        """`engine` = the net's engine when the monitor back-tracks (it checkpoints the flat parameter arena), else None."""
        self.engine = None
        if backtracking:
            eng = getattr(net, "__dict__", {}).get("_dip_engine")
            if eng is None:
                raise RuntimeError("dip-amd: back-tracking needs a net built by models.skip.skip() (flat parameter arena)")
            if getattr(eng, "kind", "skip") != "skip":
                raise NotImplementedError(f"dip-amd: {type(self).__name__} back-tracking covers skip() nets only; construct it "
                                          "with backtracking=False for a ResNet")
            self.engine = eng

    def _ensure_arena(self):
        """The kind's copy of the parameter arena (ARENA: snapshot; best_params), as large as the engine's arena and on its
        device: allocated, or allocated anew, when it is not.  None without an engine."""
        if self.engine is None or self.ARENA is None:
            return None
        name, make = self.ARENA
        params, t = self.engine.params, getattr(self, name)
        if t is None or t.numel() != params.numel() or t.device != params.device:
            t = make(params)
            setattr(self, name, t)
        return t

    def _sync_counter(self):
        """Sets the device counter to `i` on the current stream when it would not hold it (update() calls since the last
        native iteration, or an `i` set by hand)."""
        if self._counter_host != self.i:
            self.counter.fill_(self.i)
            self._counter_host = self.i

    def _advance(self, n):
        """n iterations were issued through the device-indexed entry point."""
        self.i += n
        self._counter_host += n

    def _recorded(self, n):
        """n iterations were issued with the row passed by value."""
        self.i += n

    def _update(self, outs, loss=None):
        """The eager form, once per closure evaluation: checks, fp32 contiguous outputs, the kind's launches on the current
        stream of the monitor's device."""
        self._check_room(1)
        outs = [o.detach() for o in outs]
        self._check_update(*outs)
        outs = [o.contiguous().float() for o in outs]
        with torch.cuda.device(self.dev):        # raw HIP launches go to the current device's streams
            stream = torch.cuda.current_stream(self.dev).cuda_stream
            lptr = None
            if loss is not None:
                self._loss = loss.detach().reshape(1).float()          # keep alive until the launch has run
                lptr = self._loss.data_ptr()
            self._issue(outs, lptr, stream)
        self._keep = outs
        self._recorded(1)

    # ------------------------------------------------------------------ the device-indexed form (dip_optim.NativeIteration)
    def _dev_descriptor(self, out, out_LR=None):
        """The kind's descriptor over this monitor's buffers for the output buffer(s); `loss` is filled in per iteration."""
        return self._descriptor(dict(vars(self), out=out, out_LR=out_LR))

    def _launches(self, desc):
        """The kind's entry point over `desc` and, with an engine, the conditional copy of its parameter arena."""
        arena = self._ensure_arena()
        if arena is None:
            return monitor_launches(self.lib, desc)
        params = self.engine.params
        return monitor_launches(self.lib, desc, params.data_ptr(), params.numel(), arena.data_ptr())

    def _plan(self, eng, out, head):
        """(descriptor, launches) of an iteration under `head` that writes the net output to `out`."""
        self._check_plan(out, head)
        desc = self._dev_descriptor(out, getattr(head, "out_LR", None))
        return desc, self._launches(desc)

    def _plan_keep(self):
        """The objects behind _plan_key, among them every buffer the descriptor points to: alive as long as the plan."""
        return (self, self.engine, *(getattr(self, k) for k in self.INPUTS), *self._buffers())

    def _plan_key(self):
        """What a compiled command array (dip_optim.NativeIteration) was built from: buffers by identity, settings by value."""
        return (*(id(o) for o in self._plan_keep()), *(getattr(self, k) for k in self.SETTINGS))


class _BackTracking:
    """The parameter checkpoint of the denoising and restoration closures: `snapshot` is as large as the engine's arena."""
    backtracking = property(lambda self: self.engine is not None)

    def _ensure_snapshot(self):
        """The snapshot arena, as large as the engine's parameter arena and on its device (None without back-tracking)."""
        return self._ensure_arena()

    def _backtrack(self, stream):
        """Behind the eager entry point: the fall-back / checkpoint it decided on (state[1], state[3])."""
        snap = self._ensure_snapshot()
        if snap is not None:
            params = self.engine.params
            N.check(self.lib.dip_arena_backtrack(params.data_ptr(), snap.data_ptr(), params.numel(), self.state.data_ptr(),
                                                 stream), "arena_backtrack")


class FitMonitor(_FitKind, _BackTracking, _DeviceRecords):
    INPUTS, SETTINGS = ("noisy",), ("exp_weight", "show_every", "backtrack_db", "capacity", "n")

    def __init__(self, net, img_noisy, img_gt=None, exp_weight=0.99, show_every=100, backtrack_db=5.0,
                 backtracking=True, capacity=16384):
        if not img_noisy.is_cuda:
            raise RuntimeError("dip-amd: FitMonitor works on MI355X tensors only (no CPU fallback)")
        self.noisy = img_noisy.detach().contiguous().float()
        self.gt = None if img_gt is None else img_gt.detach().to(img_noisy.device).contiguous().float()
        if self.gt is not None and self.gt.shape != self.noisy.shape:
            raise ValueError("FitMonitor: img_gt and img_noisy differ in shape")
        self.n = self.noisy.numel()
        self.exp_weight, self.show_every, self.backtrack_db = float(exp_weight), int(show_every), float(backtrack_db)
        self._init_device(img_noisy.device, capacity, self.noisy.shape, n=self.n)
        self._init_backtracking(net, backtracking)

    def update(self, out, loss=None):
        """Call once per closure evaluation, after backward() (like the reference, the fall-back
        overwrites the parameters AFTER the gradients of this iteration were computed)."""
        self._update((out,), loss)

    def _check_update(self, o):
        if o.shape != self.noisy.shape or not o.is_cuda:
            raise ValueError("FitMonitor.update: output shape/device does not match the target image")

    def _issue(self, outs, lptr, stream):
        check = 1 if (self.engine is not None and self.i % self.show_every) else 0
        N.check(self.lib.dip_fit_monitor(outs[0].data_ptr(), self.noisy.data_ptr(), _ptr(self.gt), self.out_avg.data_ptr(),
                                         self.n, self.exp_weight, 1 if self.i == 0 else 0, lptr, self.partial.data_ptr(),
                                         self.records[self.i].data_ptr(), self.state.data_ptr(), check, self.backtrack_db,
                                         stream), "fit_monitor")
        self._backtrack(stream)

    def _check_plan(self, out, head):
        if tuple(self.noisy.shape) != tuple(out.shape):
            raise ValueError(f"dip-amd: the FitMonitor's image is {tuple(self.noisy.shape)}, the net output is {tuple(out.shape)}")


class SRFitMonitor(_SRKind, _DeviceRecords):
    """psnr_LR / psnr_HR of the super-resolution closure (super-resolution.ipynb:188-191) on the device: one record per
    iteration, {loss, mse_LR, mse_HR, psnr_LR, psnr_HR}, from the two outputs of utils.loss_head.SRHead -- out_HR against
    img_HR (optional: without it mse_HR = psnr_HR = 0) and out_LR against img_LR.  No EMA, no show_every, no back-tracking
    and no net: the reference closure has none of them.  update() is the eager form (dip_sr_monitor); NativeIteration(
    monitor=this) issues dip_sr_monitor_dev, which reads the row index from `counter`."""
    INPUTS, SETTINGS = ("img_LR",), ("capacity",)

    def __init__(self, img_LR, img_HR=None, capacity=16384):
        if not isinstance(img_LR, torch.Tensor) or not img_LR.is_cuda or (img_HR is not None and not img_HR.is_cuda):
            raise RuntimeError("dip-amd: SRFitMonitor works on MI355X tensors only (no CPU fallback)")
        if int(capacity) <= 0:
            raise ValueError("dip-amd: SRFitMonitor: capacity must be > 0")
        self.img_LR = img_LR.detach().contiguous().float()
        self.img_HR = None if img_HR is None else img_HR.detach().to(img_LR.device).contiguous().float()
        self.n_lr = self.img_LR.numel()
        self._init_device(img_LR.device, capacity, (), n=None, n_lr=self.n_lr)

    def _ensure_partial(self, n_hr):
        """The per-block sums (n_hr is the output's size: without img_HR it is only known when the first output arrives)."""
        self._z.n = n_hr
        n = self._buf("partial").count(self._z)
        if self.partial is None or self.partial.numel() != n:
            self.partial = torch.empty(n, dtype=torch.float32, device=self.dev)
        return self.partial

    def _check_outputs(self, hr_shape, lr_shape, who="SRFitMonitor.update"):
        if tuple(lr_shape) != tuple(self.img_LR.shape):
            raise ValueError(f"dip-amd: {who}: the SRFitMonitor's img_LR is {tuple(self.img_LR.shape)}, out_LR is "
                             f"{tuple(lr_shape)}")
        if self.img_HR is not None and tuple(hr_shape) != tuple(self.img_HR.shape):
            raise ValueError(f"dip-amd: {who}: the SRFitMonitor's img_HR is {tuple(self.img_HR.shape)}, out_HR is "
                             f"{tuple(hr_shape)}")

    def update(self, out_HR, out_LR, loss=None):
        """Call once per closure evaluation, after backward(): mon.update(out_HR, head.out_LR, total_loss)."""
        self._update((out_HR, out_LR), loss)

    def _check_update(self, hr, lr):
        if not hr.is_cuda or not lr.is_cuda or hr.device != self.dev or lr.device != self.dev:
            raise RuntimeError(f"dip-amd: SRFitMonitor.update: the outputs are on {hr.device} / {lr.device}, the monitor "
                               f"lives on {self.dev} (no CPU fallback)")
        self._check_outputs(hr.shape, lr.shape)

    def _issue(self, outs, lptr, stream):
        hr, lr = outs
        N.check(self.lib.dip_sr_monitor(hr.data_ptr(), lr.data_ptr(), _ptr(self.img_HR), self.img_LR.data_ptr(), hr.numel(),
                                        self.n_lr, lptr, self._ensure_partial(hr.numel()).data_ptr(),
                                        self.records[self.i].data_ptr(), stream), "sr_monitor")

    def _dev_descriptor(self, out_HR, out_LR):
        self._ensure_partial(out_HR.numel())
        return super()._dev_descriptor(out_HR, out_LR)

    def _check_plan(self, out, head):
        self._check_outputs(out.shape, head.out_LR.shape, who="NativeIteration")


class RestorationFitMonitor(_RestoreKind, _BackTracking, _DeviceRecords):
    """psrn_masked / psrn and the back-tracking of the restoration closure (restoration.ipynb:192-211) on the device: one record
    per iteration, {loss, mse_masked, mse, psrn_masked, psrn, fell_back}, from the net output against `img` -- masked:
    (out - img) * mask, the notebook's out * img_mask_np against img_masked -- and, when i % show_every == 0, the fall-back to
    the last checkpoint when psrn_masked dropped by more than backtrack_db, or else the checkpoint.  No EMA: the closure has
    none.  `mask` is [1, 1|C, H, W], as for utils.loss_head.MSEHead(mask=).  update() is the eager form (dip_restore_monitor +
    dip_arena_backtrack); NativeIteration(monitor=this) issues dip_restore_monitor_dev, which reads the row index from
    `counter`.  Back-tracking needs a skip() net (flat parameter arena); backtracking=False records only."""
    INPUTS, SETTINGS = ("img", "mask"), ("show_every", "backtrack_db", "mask_c", "capacity", "n", "hw")

    def __init__(self, net, img, mask, show_every=50, backtrack_db=5.0, backtracking=True, capacity=16384):
        # (what needs no GPU is refused first: the types and shapes, the settings, the net)
        if not isinstance(img, torch.Tensor) or not isinstance(mask, torch.Tensor):
            raise TypeError("dip-amd: RestorationFitMonitor: img and mask are tensors ([1,C,H,W] and [1,1|C,H,W])")
        if img.dim() != 4 or img.shape[0] != 1:
            raise ValueError(f"dip-amd: RestorationFitMonitor: img must be [1,C,H,W], got {tuple(img.shape)}")
        mask = _mask4(mask, img.shape[1], img.shape[2:], "RestorationFitMonitor")
        if int(show_every) <= 0 or int(capacity) <= 0:
            raise ValueError("dip-amd: RestorationFitMonitor: show_every and capacity must be > 0")
        self._init_backtracking(net, backtracking)
        if not img.is_cuda:
            raise RuntimeError("dip-amd: RestorationFitMonitor works on MI355X tensors only (no CPU fallback)")
        self.img = img.detach().contiguous().float()
        self.mask, self.mask_c = mask.to(img.device), int(mask.shape[1])
        self.n, self.hw = self.img.numel(), int(img.shape[2] * img.shape[3])
        self.show_every, self.backtrack_db = int(show_every), float(backtrack_db)
        self._init_device(img.device, capacity, self.img.shape, n=self.n)

    def update(self, out, loss=None):
        """Call once per closure evaluation, after backward() (like the reference, the fall-back overwrites the parameters
        AFTER the gradients of this iteration were computed)."""
        self._update((out,), loss)

    def _check_update(self, o):
        if o.shape != self.img.shape or not o.is_cuda or o.device != self.dev:
            raise ValueError("dip-amd: RestorationFitMonitor.update: output shape/device does not match the image")

    def _issue(self, outs, lptr, stream):
        check = 1 if (self.engine is not None and self.i % self.show_every == 0) else 0      # restoration.ipynb:198
        N.check(self.lib.dip_restore_monitor(outs[0].data_ptr(), self.img.data_ptr(), self.mask.data_ptr(), self.mask_c, self.n,
                                             self.hw, lptr, self.partial.data_ptr(), self.records[self.i].data_ptr(),
                                             self.state.data_ptr(), check, self.backtrack_db, stream), "restore_monitor")
        self._backtrack(stream)

    def _check_plan(self, out, head):
        if tuple(self.img.shape) != tuple(out.shape):
            raise ValueError(f"dip-amd: the RestorationFitMonitor's image is {tuple(self.img.shape)}, the net output is "
                             f"{tuple(out.shape)}")


class EarlyStopMonitor(_EarlyStopKind, _DeviceRecords):
    """When to stop, without a ground truth: the windowed moving variance of the net output (ES-WMV; Wang et al., "Early
    Stopping for Deep Image Prior") on the device.  The variance over the last `window` outputs falls while the fit converges on
    the image and rises again once it fits the noise; the fit counts as done after `patience` iterations without a new minimum,
    and the output at the minimum is kept in `best_out`.  One record per iteration, {var, var_min, best_iter, wait, stopped};
    the first window - 1 rows are {inf, inf, -1, 0, 0}, the rows after the stopping iteration repeat its row.  Once stopped,
    the window, var_min, best_iter, best_out and best_params are frozen.  A NaN output makes the variance NaN: no minimum is
    taken and `wait` advances (the fp64 running mean keeps the NaN, so the monitor then stops after `patience` iterations).

    `img_like` gives the shape [1,C,H,W] and the device of the output.  net= a skip() net: the flat parameter arena at the
    minimum is kept too (`best_params`; restore_best() copies it back); without it only best_out is kept.  update(out) is the
    eager form, NativeIteration(early_stop=this) issues the same entry point (dip_early_stop_dev reads the row index from
    `counter`, the ring head and the fill count from `state`), and the two may alternate.

    Memory: the ring holds `window` outputs, 4 * window * n bytes -- 315 MB for window = 100 at 3 x 512 x 512 -- plus 8 n bytes
    of fp64 mean and 4 n of best_out (`memory_bytes`).

    mode='emv' is the ring-free form of the same paper, the exponential moving variance (dip_early_stop_emv_dev): mu <- mu +
    alpha (x - mu), v <- (1 - alpha) (v + alpha |x - mu|^2 / n), decisions on v from iteration `warmup` on (None: ceil(2 /
    alpha); v ramps up from zero for about 1 / alpha iterations and a decision on the ramp is a false minimum).  The same
    record, the same state, best_out / best_params / restore_best() / run_until; `ring` is None and `window` is ignored: 8 n
    bytes of mean plus 4 n of best_out, 9.4 MB at 3 x 512 x 512."""
    SETTINGS = ("window", "patience", "capacity", "n", "mode", "alpha", "warmup")
    _recorded = _DeviceRecords._advance            # update() goes through the device-indexed entry point: the counter moves

    def __init__(self, img_like, window=100, patience=1000, net=None, capacity=16384, *, mode="wmv", alpha=0.1, warmup=None):
        # (what needs no GPU is refused first: the settings, the net)
        if not isinstance(img_like, torch.Tensor):
            raise TypeError("dip-amd: EarlyStopMonitor: img_like is a tensor shaped like the net output ([1,C,H,W])")
        self.mode, self.window, self.alpha, self.warmup, self.patience, capacity = _early_stop_settings(
            "EarlyStopMonitor", mode, window, alpha, warmup, patience, capacity)
        self._init_backtracking(net, net is not None)               # `engine`: the net's, or None without net=
        if not img_like.is_cuda:
            raise RuntimeError("dip-amd: EarlyStopMonitor works on MI355X tensors only (no CPU fallback)")
        self.shape, self.n = tuple(img_like.shape), img_like.numel()
        if self.n < 1:
            raise ValueError("dip-amd: EarlyStopMonitor: img_like is empty")
        self._init_device(img_like.device, capacity, self.shape, n=self.n)

    @property
    def best_iter(self):
        """The iteration of the minimum, -1 before the first decision (reads one value; synchronises)."""
        return int(self.state[9].item())

    @property
    def stopped(self):
        """1 once `patience` iterations passed without a new minimum (reads one value; synchronises)."""
        return int(self.state[10].item())

    def _ensure_best_params(self):
        """The arena kept at the minimum, zero until then, as large as the engine's parameter arena and on its device (None
        without net=)."""
        return self._ensure_arena()

    def restore_best(self):
        """Copies best_params back into the net's parameter arena: the net then produces best_out again."""
        if self.engine is None:
            raise RuntimeError("dip-amd: EarlyStopMonitor.restore_best needs net= (the monitor keeps best_out only)")
        if self.best_params is None or self.best_iter < 0:
            raise RuntimeError("dip-amd: EarlyStopMonitor.restore_best: no minimum has been recorded yet")
        params = self.engine.params
        if params.numel() != self.best_params.numel() or params.device != self.best_params.device:
            raise RuntimeError("dip-amd: EarlyStopMonitor.restore_best: the net's parameter arena changed since the minimum")
        with torch.no_grad():
            params.copy_(self.best_params)

    def _check_out(self, shape, who):
        if tuple(shape) != self.shape:
            raise ValueError(f"dip-amd: {who}: the EarlyStopMonitor was built for {self.shape}, the net output is {tuple(shape)}")

    def update(self, out):
        """Call once per closure evaluation, after backward() and before the optimiser's step: best_params are then the
        parameters that produced best_out."""
        self._update((out,))

    def _check_update(self, o):
        self._check_out(o.shape, "EarlyStopMonitor.update")
        if not o.is_cuda or o.device != self.dev:
            raise ValueError(f"dip-amd: EarlyStopMonitor.update: the output is on {o.device}, the monitor lives on {self.dev} "
                             "(no CPU fallback)")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("dip-amd: EarlyStopMonitor.update cannot be captured into a hipGraph (the row index is "
                               "host-synchronised state)")

    def _issue(self, outs, lptr, stream):
        self._sync_counter()
        for fn, args, name in self._launches(self._dev_descriptor(outs[0])):
            N.check(fn(*args, stream), name)

    def _check_plan(self, out, head):
        self._check_out(out.shape, "NativeIteration")


class PosteriorMonitor(_PosteriorKind, _DeviceRecords):
    """Sample mean and variance of the net outputs of an SGLD fit (dip_optim.FusedAdam(noise_std=...); Cheng et al., "A Bayesian
    Perspective on the Deep Image Prior") on the device: iteration i is a sample iff i >= burn_in and (i - burn_in) % every == 0,
    and a sample updates `mean` and `m2` ([1,C,H,W] fp32, zero before the first) by Welford's rule in individually rounded fp32
    operations (dip_posterior_dev; include/dip_hip.h states them).  `mean` is the posterior-mean estimate, variance() = m2 /
    (count - 1) the per-pixel uncertainty map.

    `img_like` gives the shape [1,C,H,W] and the device of the output.  update(out) is the eager form -- after backward() and
    before the optimiser's step, so the sample is the output of the parameters that are about to be stepped and perturbed --
    and NativeIteration(posterior=this) issues the same entry point in the same place; the two may alternate.  At most 2**24
    samples (the count is a float in the update): what would pass it is refused before anything is issued.  B chains through
    one launch list: GroupedPosteriorMonitor.

    img_gt= (optional, shaped like img_like) adds the curve the SGLD paper shows, the PSNR of the posterior mean against the
    ground truth: dip_posterior_rec_dev takes dip_posterior_dev's place -- mean and m2 are those of a monitor without it, bit
    for bit -- and on every SAMPLE iteration, and only then, writes row number `count` of a [capacity, 3] table {iteration,
    mse_mean, psnr_mean}.  history() is [count, 3] from one copy, last() a dict; what would pass `capacity` samples is refused
    before anything is issued.  Without img_gt there is no table: history() / last() raise."""
    SETTINGS = ("burn_in", "every", "n")
    _recorded = _DeviceRecords._advance            # update() goes through the device-indexed entry point: the counter moves

    def __init__(self, img_like, burn_in, every=1, img_gt=None, capacity=16384):
        # (what needs no GPU is refused first: the type, the settings)
        if not isinstance(img_like, torch.Tensor):
            raise TypeError("dip-amd: PosteriorMonitor: img_like is a tensor shaped like the net output ([1,C,H,W])")
        capacity = self._init_posterior(burn_in, every, img_gt is not None, capacity)
        if img_gt is not None and (not isinstance(img_gt, torch.Tensor) or tuple(img_gt.shape) != tuple(img_like.shape)):
            raise ValueError(f"dip-amd: PosteriorMonitor: img_gt must be a tensor shaped like img_like {tuple(img_like.shape)}, got "
                             f"{tuple(getattr(img_gt, 'shape', ()))}")
        if not img_like.is_cuda:
            raise RuntimeError("dip-amd: PosteriorMonitor works on MI355X tensors only (no CPU fallback)")
        self.shape, self.n = tuple(img_like.shape), img_like.numel()
        if self.n < 1:
            raise ValueError("dip-amd: PosteriorMonitor: img_like is empty")
        if self.with_gt:
            self.gt = img_gt.detach().to(img_like.device).contiguous().float()
            self.SETTINGS = PosteriorMonitor.SETTINGS + ("capacity",)
        self._init_device(img_like.device, capacity, self.shape, n=self.n)

    def _table(self, need=0):
        if not self.with_gt:
            raise RuntimeError("dip-amd: PosteriorMonitor keeps no record table (read mean, variance() and count)")
        return self.records

    @property
    def count(self):
        """Samples taken so far (reads one value; synchronises)."""
        return int(self.samples.item())

    def variance(self):
        """The sample variance of the outputs per element, m2 / (count - 1), [1,C,H,W]; synchronises."""
        k = self.count
        if k < 2:
            raise RuntimeError(f"dip-amd: PosteriorMonitor.variance needs at least two samples, {k} taken so far")
        return self.m2 / float(k - 1)

    def _check_out(self, shape, who):
        if tuple(shape) != self.shape:
            raise ValueError(f"dip-amd: {who}: the PosteriorMonitor was built for {self.shape}, the net output is {tuple(shape)}")

    def update(self, out):
        """Call once per closure evaluation, after backward() and before the optimiser's step."""
        self._update((out,))

    def _check_update(self, o):
        self._check_out(o.shape, "PosteriorMonitor.update")
        if not o.is_cuda or o.device != self.dev:
            raise ValueError(f"dip-amd: PosteriorMonitor.update: the output is on {o.device}, the monitor lives on {self.dev} "
                             "(no CPU fallback)")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("dip-amd: PosteriorMonitor.update cannot be captured into a hipGraph (the iteration index is "
                               "host-synchronised state)")

    def _issue(self, outs, lptr, stream):
        self._sync_counter()
        for fn, args, name in self._launches(self._dev_descriptor(outs[0])):
            N.check(fn(*args, stream), name)

    def _check_plan(self, out, head):
        self._check_out(out.shape, "NativeIteration")


class SSIMMonitor(_SSIMKind, _DeviceRecords):
    """The mean structural similarity (SSIM; Wang, Bovik, Sheikh, Simoncelli 2004) of the net output against a ground truth on
    the device, the number a restoration result is quoted with next to its PSNR: one record per iteration, {ssim, ssim_sm}.
    Gaussian 11 x 11 window (sigma 1.5), K1 = 0.01, K2 = 0.03, biased covariances, valid positions only -- (H-10) x (W-10) per
    channel -- and the mean over all channels and positions (dip_ssim_dev; include/dip_hip.h states the definition and the
    arithmetic).  It aims at skimage.metrics.structural_similarity(gaussian_weights=True, use_sample_covariance=False,
    data_range=data_range) and was not checked against that library.

    `img_gt` is [1,C,H,W] like the net output.  img_avg= a second source of that shape, read where it lies (fp32, contiguous, on
    the device): with img_avg=fit_monitor.out_avg -- call FitMonitor.update first -- `ssim_sm` is the SSIM of the denoising
    notebook's smoothed result; without it the column is 0.  keep_map=True keeps S of the last iteration in `map`
    ([1,C,H-10,W-10]).  update(out) is the eager form, after backward(); NativeIteration(ssim=this) issues the same entry point
    behind monitor=, and the two may alternate.  It does not touch the fit."""
    INPUTS, SETTINGS = ("avg",), ("chw", "data_range", "capacity")
    _recorded = _DeviceRecords._advance            # update() goes through the device-indexed entry point: the counter moves

    def __init__(self, img_gt, img_avg=None, data_range=1.0, keep_map=False, capacity=16384):
        # (what needs no GPU is refused first: the types, the shapes, the settings)
        self.chw, self.data_range, capacity = _ssim_settings("SSIMMonitor", img_gt, data_range, capacity)
        if img_avg is not None:
            if not isinstance(img_avg, torch.Tensor) or tuple(img_avg.shape) != tuple(img_gt.shape):
                raise ValueError(f"dip-amd: SSIMMonitor: img_avg must be shaped like img_gt {tuple(img_gt.shape)}, got "
                                 f"{tuple(getattr(img_avg, 'shape', ()))}")
            if img_avg.dtype != torch.float32 or not img_avg.is_contiguous():
                raise ValueError("dip-amd: SSIMMonitor: img_avg is read where it lies: it must be a contiguous fp32 tensor")
        self.keep_map = bool(keep_map)
        if not img_gt.is_cuda or (img_avg is not None and img_avg.device != img_gt.device):
            raise RuntimeError("dip-amd: SSIMMonitor works on MI355X tensors only (no CPU fallback)")
        self.gt = img_gt.detach().contiguous().float()
        self.avg = None if img_avg is None else img_avg.detach()
        self.shape, self.n = tuple(self.gt.shape), self.gt.numel()
        self._init_device(img_gt.device, capacity, self.shape, n=self.n)

    with_avg = property(lambda self: self.avg is not None)

    def _check_out(self, shape, who):
        if tuple(shape) != self.shape:
            raise ValueError(f"dip-amd: {who}: the SSIMMonitor's img_gt is {self.shape}, the net output is {tuple(shape)}")

    def update(self, out):
        """Call once per closure evaluation, after backward() and behind FitMonitor.update (out_avg is then this iteration's)."""
        self._update((out,))

    def _check_update(self, o):
        self._check_out(o.shape, "SSIMMonitor.update")
        if not o.is_cuda or o.device != self.dev:
            raise RuntimeError(f"dip-amd: SSIMMonitor.update: the output is on {o.device}, the monitor lives on {self.dev} "
                               "(no CPU fallback)")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("dip-amd: SSIMMonitor.update cannot be captured into a hipGraph (the row index is "
                               "host-synchronised state)")

    def _issue(self, outs, lptr, stream):
        self._sync_counter()
        for fn, args, name in self._launches(self._dev_descriptor(outs[0])):
            N.check(fn(*args, stream), name)

    def _check_plan(self, out, head):
        self._check_out(out.shape, "NativeIteration")


def ssim(x, y, data_range=1.0, full=False):
    """The SSIM of x against y ([1,C,H,W] on the device) as SSIMMonitor records it, through the same entry point: a 0-dim device
    tensor (no host synchronisation), and with full=True also the map [1,C,H-10,W-10]."""
    chw, data_range, _ = _ssim_settings("ssim", x, data_range)
    if not isinstance(y, torch.Tensor) or tuple(y.shape) != tuple(x.shape):
        raise ValueError(f"dip-amd: ssim: x and y must have one shape, got {tuple(x.shape)} and {tuple(getattr(y, 'shape', ()))}")
    if not x.is_cuda or y.device != x.device:
        raise RuntimeError("dip-amd: ssim works on MI355X tensors only (no CPU fallback)")
    x, y = x.detach().contiguous().float(), y.detach().contiguous().float()
    m = SimpleNamespace(chw=chw, data_range=data_range, with_avg=False, capacity=1)
    z = monitor_sizes(m, None, x.numel(), x.shape, (1,))
    new = lambda name: torch.empty(next(b for b in SSIM_BUFFERS if b.name == name).count(z), dtype=_F32, device=x.device)
    t = dict(out=x, gt=y, partial=new("partial"), records=new("records"), map=new("map") if full else None)
    with torch.cuda.device(x.device):
        for fn, args, name in monitor_launches(N.lib(), ssim_descriptor(m, t)):
            N.check(fn(*args, torch.cuda.current_stream(x.device).cuda_stream), name)
    value = t["records"][0]
    return (value, t["map"].view(_ssim_valid(z))) if full else value


# ---------------------------------------------------------------- B fits through one launch list
class _GroupedRecords(_Records):
    """What the grouped monitors share: settings only, until a dip_group.GroupedFits adopts the monitor (once), carves the
    table's buffers from its slab rows and exposes them here as [B, ...] views; `i` is the host's count of issued iterations."""

    def _init_group(self, capacity):
        self._init_count(capacity)
        self._group = None         # weak: the group holds the monitor, and a cycle would keep slab and hipGraph alive
        self._adopted = False
        for b in self.BUFFERS:
            if b.view:
                setattr(self, b.name, None)

    def _adopt(self, group, **views):
        """`group` takes this monitor: the [B, ...] views over its slab rows become attributes."""
        self._group, self._adopted = weakref.ref(group), True
        self.__dict__.update(views)

    def _check_images(self, imgs, shapes, name, what):
        """`imgs` (None, or one [1,C,H,W] image per instance) against the shapes the group works on."""
        if imgs is None:
            return
        who = type(self).__name__
        if len(imgs) != len(shapes):
            raise ValueError(f"dip-amd: {who} has {len(imgs)} {name} for {len(shapes)} instances")
        for b, (im, shape) in enumerate(zip(imgs, shapes)):
            if tuple(im.shape) != tuple(shape):
                raise ValueError(f"dip-amd: {who}: {name}[{b}] is {tuple(im.shape)}, {what} is {tuple(shape)}")

    @property
    def group(self):
        """The GroupedFits that adopted this monitor (None before adoption, or once that group is gone)."""
        return None if self._group is None else self._group()

    def _table(self, need=0):
        if self.records is None:
            raise RuntimeError(f"dip-amd: this {type(self).__name__} has not been given to a GroupedFits yet")
        if self.i < need:
            raise RuntimeError(f"dip-amd: {type(self).__name__}.last(): nothing has been recorded yet")
        return self.records


class GroupedFitMonitor(_FitKind, _GroupedRecords):
    """The bookkeeping of FitMonitor for the B fits of a dip_group.GroupedFits: settings only.  It owns no device memory; the
    group that adopts it (GroupedFits(..., monitor=this)) places the per-instance buffers in its slab rows and exposes them
    here as [B, ...] views: records [B, capacity, 8], state [B, 4] (writable), counter [B] int32, out_avg [B, C, H, W] and
    snapshot [B, n_arena] (None without back-tracking).  `i` is the host's count of issued iterations."""

    def __init__(self, imgs_gt=None, exp_weight=0.99, show_every=100, backtrack_db=5.0, backtracking=True, capacity=16384):
        self.imgs_gt = None if imgs_gt is None else list(imgs_gt)
        if self.imgs_gt is not None and any(t is None for t in self.imgs_gt):
            raise ValueError("dip-amd: GroupedFitMonitor: imgs_gt holds one image per instance or is None (all or none)")
        self.exp_weight, self.show_every, self.backtrack_db = float(exp_weight), int(show_every), float(backtrack_db)
        self.backtracking = bool(backtracking)
        self._init_group(capacity)
        if self.show_every <= 0 or self.capacity <= 0:
            raise ValueError("dip-amd: GroupedFitMonitor: show_every and capacity must be > 0")

    def _check_targets(self, targets):
        """imgs_gt against the group's targets: one [1,C,H,W] image per instance, shaped like the target."""
        self._check_images(self.imgs_gt, [t.shape for t in targets], "imgs_gt", "the target")


class GroupedRestorationFitMonitor(_RestoreKind, _GroupedRecords):
    """RestorationFitMonitor for the B fits of a dip_group.GroupedFits(masks=...): settings only.  The image and the mask are
    the slab's own target and mask rows (no second copy); the group that adopts it places partial sums, records, state, counter
    and -- with back-tracking -- the snapshot in its slab rows, behind everything a monitor-less masked group owns, and exposes
    records [B, capacity, 6], state [B, 4] (writable), counter [B] int32 and snapshot [B, n_arena] (None without back-tracking)
    here.  ONE dip_restore_monitor_dev and ONE dip_arena_backtrack call inside the group bracket serve all B, and every
    instance takes its own decision."""

    def __init__(self, show_every=50, backtrack_db=5.0, backtracking=True, capacity=16384):
        self.show_every, self.backtrack_db = int(show_every), float(backtrack_db)
        self.backtracking = bool(backtracking)
        self._init_group(capacity)
        if self.show_every <= 0 or self.capacity <= 0:
            raise ValueError("dip-amd: GroupedRestorationFitMonitor: show_every and capacity must be > 0")


class GroupedSRFitMonitor(_SRKind, _GroupedRecords):
    """SRFitMonitor for the B fits of a dip_group.GroupedFits(downsamplers=...): settings only.  The group that adopts it
    places the per-instance buffers -- the optional HR ground truth, the partial sums, the records, the counter -- in its slab
    rows, behind everything a monitor-less super-resolution group owns, and exposes records [B, capacity, 5] and counter [B]
    int32 here.  ONE dip_sr_monitor_dev call inside the group bracket serves all B."""

    def __init__(self, imgs_HR=None, capacity=16384):
        self.imgs_HR = None if imgs_HR is None else list(imgs_HR)
        if self.imgs_HR is not None and any(t is None for t in self.imgs_HR):
            raise ValueError("dip-amd: GroupedSRFitMonitor: imgs_HR holds one image per instance or is None (all or none)")
        self._init_group(capacity)
        if self.capacity <= 0:
            raise ValueError("dip-amd: GroupedSRFitMonitor: capacity must be > 0")

    def _check_count(self, B):
        """What can be said about imgs_HR before the net output's size is known (the shapes: _check_hr)."""
        if self.imgs_HR is not None and len(self.imgs_HR) != B:
            raise ValueError(f"dip-amd: GroupedSRFitMonitor has {len(self.imgs_HR)} imgs_HR for {B} instances")

    def _check_hr(self, B, hr_shape):
        """imgs_HR against the planned net output: one [1,C,H,W] image per instance."""
        self._check_images(self.imgs_HR, [hr_shape] * B, "imgs_HR", "the net output")


class GroupedEarlyStopMonitor(_EarlyStopKind, _GroupedRecords):
    """EarlyStopMonitor for the B fits of a dip_group.GroupedFits(..., early_stop=this): settings only.  A keyword of its own
    next to monitor=, independent of it, for all three group kinds (plain, masks=, downsamplers=): the record needs the net
    output only.  The group that adopts it places, behind everything else a row owns -- the monitor= buffers included -- the
    ring ('wmv' only), the fp64 mean, the partials, the records, the 64-byte state, the counter, best_out and, with
    keep_params, best_params, and exposes them here as [B, ...] views: records [B, capacity, 5], state [B, 16] int32, counter
    [B], best_out [B, C, H, W], best_params [B, n_arena] (None with keep_params=False), ring [B, window, n] (None in 'emv')
    and mean [B, n].  ONE dip_early_stop_dev ('emv': dip_early_stop_emv_dev) and ONE dip_early_stop_keep call inside the group
    bracket, behind the monitor= launches and in front of Adam, serve all B inside the ONE hipGraph of capture().

    Every instance takes its own decision.  A stopped instance's early-stop state is frozen; its fit goes on, because a row
    cannot leave the launch list: g.run_until() returns once ALL instances have stopped, restore_best() puts every minimum back.
    mode='emv' is what a group can afford in every row: 12 n bytes per instance instead of 4 * window * n."""

    def __init__(self, mode="wmv", window=100, alpha=0.1, warmup=None, patience=1000, keep_params=True, capacity=16384):
        self.mode, self.window, self.alpha, self.warmup, self.patience, capacity = _early_stop_settings(
            "GroupedEarlyStopMonitor", mode, window, alpha, warmup, patience, capacity)
        self.keep_params = bool(keep_params)
        self._init_group(capacity)

    @property
    def best_iter(self):
        """The iteration of every instance's minimum, -1 before its first decision: B ints (one copy; synchronises)."""
        self._table()
        return self.state[:, 9].tolist()

    @property
    def stopped(self):
        """Per instance, 1 once `patience` iterations passed without a new minimum: B ints (one copy; synchronises)."""
        self._table()
        return self.state[:, 10].tolist()

    def restore_best(self, b=None):
        """Copies best_params back over the parameter row of instance b (None: of every instance): nets[b] then produces
        best_out[b] again."""
        self._table()
        g = self.group
        if g is None:
            raise RuntimeError("dip-amd: GroupedEarlyStopMonitor.restore_best: the GroupedFits that adopted this monitor is gone")
        if self.best_params is None:
            raise RuntimeError("dip-amd: GroupedEarlyStopMonitor.restore_best needs keep_params=True (the monitor keeps best_out "
                               "only)")
        rows = range(g.B) if b is None else [int(b)]
        if any(not 0 <= r < g.B for r in rows):
            raise IndexError(f"dip-amd: GroupedEarlyStopMonitor.restore_best: instance {b} of {g.B}")
        best = self.best_iter
        none = [r for r in rows if best[r] < 0]
        if none:
            raise RuntimeError(f"dip-amd: GroupedEarlyStopMonitor.restore_best: no minimum has been recorded yet for instance(s) "
                               f"{none}")
        params = g._strided(g.eng.params, g.eng.n_arena)
        with torch.no_grad():
            for r in rows:
                params[r].copy_(self.best_params[r])


class PooledPosterior(NamedTuple):
    """What GroupedPosteriorMonitor.pooled() returns: device tensors, nothing synchronised."""
    mean: torch.Tensor                  # [1, C, H, W] the mean over the pooled chains' means
    var: torch.Tensor                   # [1, C, H, W] V = (k - 1) / k W + B / k, the pooled estimate of the posterior variance
    within: torch.Tensor                # [1, C, H, W] W, the mean within-chain variance
    rhat: Optional[torch.Tensor]        # [1, C, H, W] sqrt(V / W), NaN where W is not positive; None with rhat_map=False
    summary: torch.Tensor               # fp64 [3]: mean and max of rhat over the other elements, the number of degenerate ones


class GroupedPosteriorMonitor(_PosteriorKind, _GroupedRecords):
    """PosteriorMonitor for the B fits of a dip_group.GroupedFits(..., posterior=this): settings only, until adopted.  A keyword of
    its own next to monitor=, early_stop= and ssim=, for all three group kinds (plain, masks=, downsamplers=: the sample is the
    net output, in a super-resolution group the HR output).  One burn_in / every for all B: the chains run in lockstep.  The
    group that adopts it places mean, m2, samples and counter in its slab rows, behind everything else a row owns -- the lr /
    reg_std sweep rows included -- and exposes them here: mean and m2 [B, C, H, W], samples and counter [B] int32.  ONE
    dip_posterior_dev call inside the group bracket, behind the monitor= and early_stop= launches and in front of ssim= and Adam
    (the order of a solo NativeIteration), serves all B inside the ONE hipGraph of capture(); instance b's rows are those of its
    solo NativeIteration(posterior=PosteriorMonitor(...)) fit, bit for bit.  `count` is the host's: samples_after(i), no
    synchronisation.

    imgs_gt= (one [1,C,H,W] image per instance, shaped like the net output) adds the PSNR of every instance's posterior mean:
    ONE dip_posterior_rec_dev call instead, with the gt, fp64 partial and record rows in the slab; records [B, capacity, 3],
    history() [B, count, 3], one row per SAMPLE.

    pooled(): B instances over one image with different param_noise_seeds are B independent chains; their pooled mean, the
    Gelman-Rubin variance estimate and R-hat come from one pass over the rows (dip_posterior_pool), nothing through the host."""

    def __init__(self, burn_in, every=1, imgs_gt=None, capacity=16384):
        self.imgs_gt = None if imgs_gt is None else list(imgs_gt)
        if self.imgs_gt is not None:
            if not self.imgs_gt or any(not isinstance(t, torch.Tensor) for t in self.imgs_gt):
                raise ValueError("dip-amd: GroupedPosteriorMonitor: imgs_gt holds one ground truth per instance or is None (all or "
                                 "none)")
            if self.imgs_gt[0].dim() != 4 or self.imgs_gt[0].shape[0] != 1:
                raise ValueError(f"dip-amd: GroupedPosteriorMonitor: imgs_gt must be [1,C,H,W] images, got "
                                 f"{tuple(self.imgs_gt[0].shape)}")
            self._check_images(self.imgs_gt, [self.imgs_gt[0].shape] * len(self.imgs_gt), "imgs_gt", "imgs_gt[0]")
        self._init_group(self._init_posterior(burn_in, every, self.imgs_gt is not None, capacity))
        self._chains = {}

    def _check_count(self, B):
        """What can be said about imgs_gt before the net output's size is known (the shapes: _check_out)."""
        if self.imgs_gt is not None and len(self.imgs_gt) != B:
            raise ValueError(f"dip-amd: GroupedPosteriorMonitor has {len(self.imgs_gt)} imgs_gt for {B} instances")

    def _check_out(self, B, out_shape):
        """imgs_gt against the (planned) net output: one [1,C,H,W] image per instance."""
        self._check_images(self.imgs_gt, [out_shape] * B, "imgs_gt", "the net output")

    def _adopted_group(self, who):
        g = self.group
        if self.mean is None or g is None:
            raise RuntimeError(f"dip-amd: GroupedPosteriorMonitor.{who}: " + ("the GroupedFits that adopted this monitor is gone"
                               if self._adopted else "this monitor has not been given to a GroupedFits yet"))
        return g

    def _table(self, need=0):
        self._adopted_group("history")
        if not self.with_gt:
            raise RuntimeError("dip-amd: GroupedPosteriorMonitor keeps no record table without imgs_gt= (read mean, variance() and "
                               "count)")
        return self.records

    @property
    def count(self):
        """Samples taken by every instance once all issued work has run: samples_after(i), from the host's count of issued
        iterations (nothing is read, nothing synchronises)."""
        return self.samples_after(self.i)

    def variance(self):
        """The sample variance of every instance's outputs per element, m2 / (count - 1), [B, C, H, W]; no synchronisation."""
        self._adopted_group("variance")
        k = self.count
        if k < 2:
            raise RuntimeError(f"dip-amd: GroupedPosteriorMonitor.variance needs at least two samples, {k} taken so far")
        return self.m2 / float(k - 1)

    def pooled(self, chains=None, rhat_map=True):
        """The chains pooled (default: all B; any subset of at least 2, in any order, without duplicates -- the sums walk them in
        list order): a PooledPosterior of device tensors from ONE dip_posterior_pool launch on the current stream, outside the
        group bracket, with k = count.  Nothing synchronises.  Meaningful where the pooled instances fit one image."""
        g = self._adopted_group("pooled")
        k = self.count
        if k < 2:
            raise RuntimeError(f"dip-amd: GroupedPosteriorMonitor.pooled needs at least two samples per chain, {k} taken so far")
        chains = tuple(range(g.B)) if chains is None else tuple(chains)
        if any(isinstance(c, bool) or int(c) != c for c in chains):
            raise ValueError(f"dip-amd: GroupedPosteriorMonitor.pooled: chains are instance indices, got {list(chains)}")
        chains = tuple(int(c) for c in chains)
        if len(chains) < 2:
            raise ValueError(f"dip-amd: GroupedPosteriorMonitor.pooled: pooling needs at least 2 chains, got {list(chains)}")
        if len(set(chains)) != len(chains):
            raise ValueError(f"dip-amd: GroupedPosteriorMonitor.pooled: a chain is pooled once, got {list(chains)}")
        if any(not 0 <= c < g.B for c in chains):
            raise IndexError(f"dip-amd: GroupedPosteriorMonitor.pooled: chains {list(chains)} of a group of {g.B}")
        dev, shape, n = self.mean.device, (1, *self.mean.shape[1:]), self.mean[0].numel()
        lib = N.lib()
        with torch.cuda.device(dev):
            idx = self._chains.get(chains)
            if idx is None:
                idx = self._chains[chains] = torch.tensor(chains, dtype=_I32, device=dev)
            new = lambda: torch.empty(shape, dtype=_F32, device=dev)
            out = PooledPosterior(new(), new(), new(), new() if rhat_map else None, torch.empty(3, dtype=_F64, device=dev))
            partial = torch.empty(3 * lib.dip_fit_monitor_nblk(n), dtype=_F64, device=dev)
            N.check(lib.dip_posterior_pool(self.mean.data_ptr(), self.m2.data_ptr(), self.mean.stride(0) * 4, idx.data_ptr(),
                                           len(chains), k, n, out.mean.data_ptr(), out.var.data_ptr(), out.within.data_ptr(),
                                           _ptr(out.rhat), partial.data_ptr(), out.summary.data_ptr(),
                                           torch.cuda.current_stream(dev).cuda_stream), "posterior_pool")
        return out


class GroupedSSIMMonitor(_SSIMKind, _GroupedRecords):
    """SSIMMonitor for the B fits of a dip_group.GroupedFits(..., ssim=this): settings only, until adopted.  A keyword of its own
    next to monitor= and early_stop=, for all three group kinds (plain, masks=, downsamplers=: the record needs the net output
    only; in a super-resolution group imgs_gt are the HR images).  The group that adopts it places, behind the es_ rows, the
    ground truth, the partials, the records and the counter in its slab rows and exposes records [B, capacity, 2] and counter
    [B] here.  ONE dip_ssim_dev call inside the group bracket, behind the monitor= and early_stop= launches and in front of
    Adam, serves all B inside the ONE hipGraph of capture(); instance b's records are those of its solo fit, bit for bit.
    with_avg=True records `ssim_sm` of the group's smoothed output too: it needs monitor=GroupedFitMonitor(...), whose out_avg
    rows lie in the slab and are this iteration's when the call runs."""
    keep_map = False                               # (no per-instance map: read g.out and call ssim(..., full=True))

    def __init__(self, imgs_gt, with_avg=False, data_range=1.0, capacity=16384):
        self.imgs_gt = list(imgs_gt) if imgs_gt is not None else []
        if not self.imgs_gt or any(t is None for t in self.imgs_gt):
            raise ValueError("dip-amd: GroupedSSIMMonitor: imgs_gt holds one ground truth per instance")
        self.chw, self.data_range, capacity = _ssim_settings("GroupedSSIMMonitor", self.imgs_gt[0], data_range, capacity)
        self._check_images(self.imgs_gt, [self.imgs_gt[0].shape] * len(self.imgs_gt), "imgs_gt", "imgs_gt[0]")
        self.with_avg = bool(with_avg)
        self._init_group(capacity)

    def _check_out(self, B, out_shape):
        """imgs_gt against the planned net output: one [1,C,H,W] image per instance."""
        self._check_images(self.imgs_gt, [out_shape] * B, "imgs_gt", "the net output")
