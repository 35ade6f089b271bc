"""Device-side bookkeeping for the notebooks' closures (no counterpart file in the reference: the
reference does this work inline, on the host, in every closure -- denoising.ipynb:214-248 (FitMonitor),
super-resolution.ipynb:188-191 (SRFitMonitor), restoration.ipynb:192-211 (RestorationFitMonitor)).

    monitor = FitMonitor(net, img_noisy_torch, img_torch, exp_weight=0.99, show_every=100)
    def closure():
        out = net(net_input_saved + noise.normal_() * reg_noise_std)
        total_loss = mse(out, img_noisy_torch)
        total_loss.backward()
        monitor.update(out, total_loss)          # EMA + 3 PSNRs + back-tracking, no host sync
        return total_loss
    optimize('adam', p, closure, LR, num_iter)
    hist = monitor.history()                     # [iters, 8] numpy, ONE device->host copy
    out_avg = monitor.out_avg                    # the smoothed output (1 x C x H x W, on the GPU)

The same bookkeeping inside the autograd-free iteration (no Python between the iterations):

    it = NativeIteration(net, head, opt, net_input, reg_noise=reg, monitor=monitor)
    it.run(show_every); print(monitor.last())    # the notebook's print loop
    it.run(n); hist = monitor.history()

There the iteration index is read from device memory (`monitor.counter`, dip_fit_monitor_dev); `monitor.i` stays the host's
count, and the two forms may alternate on one monitor at any iteration boundary.

B fits through one launch list (dip_group.GroupedFits) carry a GroupedFitMonitor: settings only, until the group adopts it and
carves its state -- per instance: gt, out_avg, partial sums, records, state, counter, snapshot -- from the slab rows.  Then ONE
dip_fit_monitor_dev / dip_arena_backtrack call inside the group bracket serves all B, and every instance takes its own
snapshot / fall-back decision:

    mon = GroupedFitMonitor(imgs_gt, exp_weight=0.99, show_every=100, capacity=num_iter)
    g = GroupedFits(nets, net_inputs, imgs_noisy, reg_noise_std=1/30, monitor=mon)
    g.capture(); g.run(num_iter - 3)
    hist = mon.history()                         # [B, iters, 8] numpy, ONE device->host copy
    mon.last()[b]["psrn_gt_sm"]; mon.out_avg[b]

Record columns: loss, mse_noisy, mse_gt, mse_gt_sm, psrn_noisy, psrn_gt, psrn_gt_sm, fell_back.

The super-resolution closure (super-resolution.ipynb:169-191, sr_prior_effect.ipynb cell 6) keeps another record: after
backward() it computes psnr_LR = compare_psnr(LR_np, out_LR) and psnr_HR = compare_psnr(HR_np, out_HR) on the host -- two
device-to-host copies and two synchronisations per iteration -- and has no EMA and no back-tracking.  SRFitMonitor is that
record on the device (dip_sr_monitor: one streaming pass over both sizes, a one-block finalize; columns loss, mse_LR, mse_HR,
psnr_LR, psnr_HR; img_HR is optional):

    mon = SRFitMonitor(img_LR_var, img_HR_var, capacity=num_iter)
    def closure():
        total_loss, out_HR = head(net_input)                 # head = utils.loss_head.SRHead(net, img_LR_var, downsampler)
        total_loss.backward()
        mon.update(out_HR, head.out_LR, total_loss)          # no host sync
        return total_loss
    psnr_history = mon.history()[:, 3:5]                     # [iters, 5] numpy, ONE device->host copy

    it = NativeIteration(net, head, opt, net_input, reg_noise=reg, monitor=mon)     # the same record inside the one call:
    it.run(n); mon.last()["psnr_HR"]                                               # dip_sr_monitor_dev, indexed by mon.counter

    mon = GroupedSRFitMonitor(imgs_HR, capacity=num_iter)                           # B fits: settings only, adopted once
    g = GroupedFits(nets, net_inputs, imgs_LR, downsamplers=downs, monitor=mon)     # ONE dip_sr_monitor_dev call for all B,
    g.capture(); g.run(num_iter - 3); mon.history()                                 # part of the ONE hipGraph; [B, iters, 5]

The restoration / inpainting closure (restoration.ipynb:180-219) keeps a third record: psrn_masked = compare_psnr(img_masked,
out * img_mask_np) and psrn = compare_psnr(img_np, out) on the host in every iteration (:192-193), and ON every show_every-th
iteration (:198 `i % show_every == 0`; the denoising notebook checks between them) the fall-back to the last parameter
checkpoint when psrn_masked dropped by more than 5 dB (:202-208), or else a copy of every parameter to the CPU (:209-211).  It
has no EMA.  RestorationFitMonitor is that bookkeeping on the device (dip_restore_monitor: one streaming pass, a one-block
finalize, then dip_arena_backtrack; columns loss, mse_masked, mse, psrn_masked, psrn, fell_back):

    mon = RestorationFitMonitor(net, img_var, mask_var, show_every=50, capacity=num_iter)
    def closure():
        total_loss, out = head(net_input)                    # head = utils.loss_head.MSEHead(net, img_var, mask=mask_var)
        total_loss.backward()
        mon.update(out, total_loss)                          # no host sync, no parameter copy to the CPU
        return total_loss

    it = NativeIteration(net, head, opt, net_input, reg_noise=reg, monitor=mon)     # dip_restore_monitor_dev + dip_arena_backtrack,
    it.run(n); mon.last()["psrn_masked"]                                           # indexed by mon.counter

    mon = GroupedRestorationFitMonitor(show_every=50, capacity=num_iter)            # B fits: settings only, adopted once
    g = GroupedFits(nets, net_inputs, imgs, masks=masks, monitor=mon)               # ONE dip_restore_monitor_dev and ONE
    g.capture(); g.run(num_iter - 3); mon.history()                                 # dip_arena_backtrack call; [B, iters, 6]

None of the notebooks decides WHEN to stop: num_iter is picked by hand and a person looks at the plot.  EarlyStopMonitor is the
ground-truth-free criterion for an unattended fit -- the windowed moving variance of the output (ES-WMV, Wang et al., "Early
Stopping for Deep Image Prior"): stop after `patience` iterations without a new minimum of the variance over the last `window`
outputs, keep the output (and, with net=, the parameters) of the minimum.  On the host that is an `out.detach().cpu()` and a
synchronisation per iteration; here the window is a ring in device memory (dip_early_stop_dev: one streaming pass, a one-block
finalize, a conditional copy; columns var, var_min, best_iter, wait, stopped), and the host polls a 4-byte flag:

    es = EarlyStopMonitor(img_noisy_torch, window=100, patience=1000, net=net, capacity=num_iter)
    def closure():
        total_loss, out = head(net_input)
        total_loss.backward()
        es.update(out)                                       # no host sync; after backward(), before the optimiser's step
        return total_loss

    it = NativeIteration(net, head, opt, net_input, reg_noise=reg, early_stop=es)   # next to monitor=, independent of it
    issued, losses = it.run_until(num_iter, check_every=50)                         # one 4-byte read per 50 iterations
    es.best_iter, es.best_out; es.restore_best()                                    # the net carries the minimum's parameters

The ring is 4 * window * n bytes.  mode='emv' is the ring-free form of the same paper, the exponential moving variance
(dip_early_stop_emv_dev): only the fp64 mean is carried per element, 20 n bytes of traffic instead of 28 n, decisions from
iteration `warmup` on.  That is what a group can afford in every row: B fits through one launch list take a
GroupedEarlyStopMonitor (settings only, adopted once; either mode), and every instance takes its own decision:

    es = EarlyStopMonitor(img_noisy_torch, patience=1000, net=net, capacity=num_iter, mode='emv', alpha=0.1)    # no ring

    mon = GroupedEarlyStopMonitor(mode='emv', alpha=0.1, patience=1000, capacity=num_iter)
    g = GroupedFits(nets, net_inputs, imgs_noisy, reg_noise_std=1/30, early_stop=mon)   # next to monitor=, independent of it
    g.capture(); issued = g.run_until(num_iter - 3, check_every=50)                     # until ALL instances have stopped
    mon.best_iter, mon.stopped, mon.best_out[b]; mon.restore_best()                     # per instance; the minima's parameters
The reference's per-iteration cost this replaces: three `.detach().cpu().numpy()` of the output, a
`.item()`, and -- whenever `i % show_every` is non-zero -- a copy of all 2.2 M parameters to the CPU.
"""
import ctypes as C
import weakref

import numpy as np
import torch

import dip_native as N


_ptr = lambda t: None if t is None else t.data_ptr()


# ---------------------------------------------------------------- the device-indexed records, said once
# FitMonitor / SRFitMonitor (one fit, dip_optim.NativeIteration) and dip_group.GroupedFits (B fits through one launch list) fill
# the descriptors and list the launches HERE; `m` carries the settings, the buffers are wherever the caller keeps them.
def fit_monitor_descriptor(m, out, noisy, gt, out_avg, partial, records, counter, state, loss=None):
    """DipFitMonitorDesc of monitor m (a FitMonitor or a GroupedFitMonitor) over these buffers."""
    return N.DipFitMonitorDesc(_ptr(out), _ptr(noisy), _ptr(gt), _ptr(out_avg), noisy.numel(), m.exp_weight, m.backtrack_db,
                               _ptr(loss), _ptr(partial), _ptr(records), m.capacity, m.show_every, 1 if m.backtracking else 0,
                               0, _ptr(counter), _ptr(state))


def fit_monitor_launches(lib, desc, params_ptr, n_arena, snapshot_ptr):
    """dip_fit_monitor_dev and, with a snapshot arena, dip_arena_backtrack as (fn, args, name) triples."""
    mon = [(lib.dip_fit_monitor_dev, (C.byref(desc),), "fit_monitor_dev")]
    if snapshot_ptr is not None:
        mon.append((lib.dip_arena_backtrack, (params_ptr, snapshot_ptr, n_arena, desc.state), "arena_backtrack"))
    return mon


def sr_monitor_descriptor(m, out_HR, out_LR, img_HR, img_LR, partial, records, counter, loss=None):
    """DipSRMonitorDesc of monitor m (an SRFitMonitor or a GroupedSRFitMonitor) over these buffers."""
    return N.DipSRMonitorDesc(_ptr(out_HR), _ptr(out_LR), _ptr(img_HR), _ptr(img_LR), out_HR.numel(), img_LR.numel(), _ptr(loss),
                              _ptr(partial), _ptr(records), m.capacity, 0, _ptr(counter))


def sr_monitor_launches(lib, desc):
    return [(lib.dip_sr_monitor_dev, (C.byref(desc),), "sr_monitor_dev")]


def restore_monitor_descriptor(m, out, img, mask, mask_c, hw, partial, records, counter, state, loss=None):
    """DipRestoreMonitorDesc of monitor m (a RestorationFitMonitor or a GroupedRestorationFitMonitor) over these buffers:
    `mask` is [mask_c][hw], out / img are planes of hw."""
    return N.DipRestoreMonitorDesc(_ptr(out), _ptr(img), _ptr(mask), img.numel(), int(hw), int(mask_c), m.backtrack_db, _ptr(loss),
                                   _ptr(partial), _ptr(records), m.capacity, m.show_every, 1 if m.backtracking else 0, 0,
                                   _ptr(counter), _ptr(state))


def restore_monitor_launches(lib, desc, params_ptr, n_arena, snapshot_ptr):
    """dip_restore_monitor_dev and, with a snapshot arena, dip_arena_backtrack as (fn, args, name) triples."""
    mon = [(lib.dip_restore_monitor_dev, (C.byref(desc),), "restore_monitor_dev")]
    if snapshot_ptr is not None:
        mon.append((lib.dip_arena_backtrack, (params_ptr, snapshot_ptr, n_arena, desc.state), "arena_backtrack"))
    return mon


def _mask4(mask, C_out, hw_shape, who):
    """`mask` as a contiguous fp32 [1, 1|C_out, H, W] tensor: the rule of utils.loss_head.MSEHead(mask=)."""
    m = mask.detach().float()
    while m.dim() < 4:
        m = m[None]
    if m.shape[0] != 1 or m.shape[1] not in (1, C_out) or tuple(m.shape[2:]) != tuple(hw_shape):
        raise ValueError(f"dip-amd: {who}: mask must be [1,1|{C_out},{hw_shape[0]},{hw_shape[1]}], got {tuple(m.shape)}")
    return m.contiguous()


class _DeviceRecords:
    """What FitMonitor and SRFitMonitor share: a [capacity, len(COLUMNS)] record table in device memory, the host's count `i`
    of recorded iterations, and the device counter the *_dev kernels index the table with (NativeIteration(monitor=))."""
    COLUMNS = ()

    def _init_records(self, dev, capacity):
        self.lib = N.lib()
        self.dev = dev
        self.capacity = int(capacity)
        self.records = torch.zeros((self.capacity, len(self.COLUMNS)), dtype=torch.float32, device=dev)
        self.i = 0
        # the iteration index as the *_dev kernels read it (NativeIteration(monitor=)), and the value it will hold once
        # all issued work has run; update() passes `i` by value and leaves both alone, NativeIteration re-aligns them
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self._counter_host = 0

    def _init_backtracking(self, net, backtracking):
        """`engine` = the net's engine when the monitor back-tracks (it checkpoints the flat parameter arena), else None."""
        self.engine = None
        self.snapshot = None
        if backtracking:
            eng = getattr(net, "__dict__", {}).get("_dip_engine")
            if eng is None:
                raise RuntimeError("dip-amd: back-tracking needs a net built by models.skip.skip() (flat parameter arena)")
            if getattr(eng, "kind", "skip") != "skip":
                raise NotImplementedError(f"dip-amd: {type(self).__name__} back-tracking covers skip() nets only; construct it "
                                          "with backtracking=False for a ResNet")
            self.engine = eng

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

    def history(self):
        """All records so far as a [iters, len(COLUMNS)] float32 numpy array (synchronises once)."""
        return self.records[:self.i].cpu().numpy()

    def last(self):
        """The latest record as a dict (synchronises)."""
        r = self.records[self.i - 1].cpu().numpy()
        return dict(zip(self.COLUMNS, (float(x) for x in r)))


class FitMonitor(_DeviceRecords):
    COLUMNS = ("loss", "mse_noisy", "mse_gt", "mse_gt_sm", "psrn_noisy", "psrn_gt", "psrn_gt_sm", "fell_back")
    head_kind = None                                                # any head: the record needs the net output only
    backtracking = property(lambda self: self.engine is not None)

    def __init__(self, net, img_noisy, img_gt=None, exp_weight=0.99, show_every=100, backtrack_db=5.0,
                 backtracking=True, capacity=16384):
        if not img_noisy.is_cuda:
            raise RuntimeError("dip-amd: FitMonitor works on MI355X tensors only (no CPU fallback)")
        self._init_records(img_noisy.device, capacity)
        self.noisy = img_noisy.detach().contiguous().float()
        self.gt = None if img_gt is None else img_gt.detach().to(self.dev).contiguous().float()
        if self.gt is not None and self.gt.shape != self.noisy.shape:
            raise ValueError("FitMonitor: img_gt and img_noisy differ in shape")
        self.n = self.noisy.numel()
        self.exp_weight, self.show_every, self.backtrack_db = float(exp_weight), int(show_every), float(backtrack_db)
        self.state = torch.zeros(4, dtype=torch.float32, device=self.dev)
        self.partial = torch.empty(4 * self.lib.dip_fit_monitor_nblk(self.n), dtype=torch.float32, device=self.dev)
        self.out_avg = torch.zeros_like(self.noisy)
        self._init_backtracking(net, backtracking)

    def update(self, out, loss=None):
        """Call once per closure evaluation, after backward() (like the reference, the fall-back
        overwrites the parameters AFTER the gradients of this iteration were computed)."""
        if self.i >= self.capacity:
            raise RuntimeError("FitMonitor: capacity exceeded; construct it with capacity >= num_iter")
        o = out.detach()
        if o.shape != self.noisy.shape or not o.is_cuda:
            raise ValueError("FitMonitor.update: output shape/device does not match the target image")
        o = o.contiguous().float()
        with torch.cuda.device(self.dev):        # raw HIP launches go to the current device's streams
            stream = torch.cuda.current_stream(self.dev).cuda_stream
            lptr = None
            if loss is not None:
                self._loss = loss.detach().reshape(1).float()          # keep alive until the launch has run
                lptr = self._loss.data_ptr()
            check = 1 if (self.engine is not None and self.i % self.show_every) else 0
            N.check(self.lib.dip_fit_monitor(o.data_ptr(), self.noisy.data_ptr(),
                                             self.gt.data_ptr() if self.gt is not None else None,
                                             self.out_avg.data_ptr(), self.n, self.exp_weight, 1 if self.i == 0 else 0,
                                             lptr, self.partial.data_ptr(), self.records[self.i].data_ptr(),
                                             self.state.data_ptr(), check, self.backtrack_db, stream), "fit_monitor")
            snap = self._ensure_snapshot()
            if snap is not None:
                params = self.engine.params
                N.check(self.lib.dip_arena_backtrack(params.data_ptr(), snap.data_ptr(), params.numel(),
                                                     self.state.data_ptr(), stream), "arena_backtrack")
        self._keep = o
        self.i += 1

    # ------------------------------------------------------------------ the device-indexed form (dip_optim.NativeIteration)
    def _ensure_snapshot(self):
        """The snapshot arena, as large as the engine's parameter arena and on its device (None without back-tracking)."""
        if self.engine is None:
            return None
        params = self.engine.params
        if self.snapshot is None or self.snapshot.numel() != params.numel() or self.snapshot.device != params.device:
            self.snapshot = torch.empty_like(params)
        return self.snapshot

    def _dev_descriptor(self, out):
        """DipFitMonitorDesc over this monitor's buffers for the output buffer `out`; `loss` is filled in per iteration."""
        return fit_monitor_descriptor(self, out, self.noisy, self.gt, self.out_avg, self.partial, self.records, self.counter,
                                      self.state)

    def _plan(self, eng, out, head):
        """(descriptor, launches) of an iteration that writes the net output to `out` (dip_optim.NativeIteration)."""
        if tuple(self.noisy.shape) != tuple(out.shape):
            raise ValueError(f"dip-amd: the FitMonitor's image is {tuple(self.noisy.shape)}, the net output is {tuple(out.shape)}")
        desc = self._dev_descriptor(out)
        return desc, fit_monitor_launches(self.lib, desc, eng.params.data_ptr(), eng.params.numel(),
                                          _ptr(self._ensure_snapshot()))

    def _plan_key(self):
        """What a compiled command array (dip_optim.NativeIteration) was built from: buffers by identity, settings by value."""
        return (id(self), id(self.records), id(self.state), id(self.out_avg), id(self.partial), id(self.snapshot),
                id(self.counter), self.exp_weight, self.show_every, self.backtrack_db, id(self.noisy), id(self.gt),
                id(self.engine), self.capacity, self.n)

    def _plan_keep(self):
        """The objects behind _plan_key and every buffer the descriptor points to: alive as long as the plan."""
        return (self, self.records, self.state, self.out_avg, self.partial, self.snapshot, self.counter, self.noisy, self.gt,
                self.engine)


class SRFitMonitor(_DeviceRecords):
    """psnr_LR / psnr_HR of the super-resolution closure (super-resolution.ipynb:188-191) on the device: one record per
    iteration, {loss, mse_LR, mse_HR, psnr_LR, psnr_HR}, from the two outputs of utils.loss_head.SRHead -- out_HR against
    img_HR (optional: without it mse_HR = psnr_HR = 0) and out_LR against img_LR.  No EMA, no show_every, no back-tracking
    and no net: the reference closure has none of them.  update() is the eager form (dip_sr_monitor); NativeIteration(
    monitor=this) issues dip_sr_monitor_dev, which reads the row index from `counter`."""
    COLUMNS = ("loss", "mse_LR", "mse_HR", "psnr_LR", "psnr_HR")
    head_kind = "sr"                                                # the record needs the two outputs of an SRHead
    engine = None                                                   # no back-tracking: tied to no net

    def __init__(self, img_LR, img_HR=None, capacity=16384):
        if not isinstance(img_LR, torch.Tensor) or not img_LR.is_cuda or (img_HR is not None and not img_HR.is_cuda):
            raise RuntimeError("dip-amd: SRFitMonitor works on MI355X tensors only (no CPU fallback)")
        if int(capacity) <= 0:
            raise ValueError("dip-amd: SRFitMonitor: capacity must be > 0")
        self._init_records(img_LR.device, capacity)
        self.img_LR = img_LR.detach().contiguous().float()
        self.img_HR = None if img_HR is None else img_HR.detach().to(self.dev).contiguous().float()
        self.n_lr = self.img_LR.numel()
        self.partial = None

    def _ensure_partial(self, n_hr):
        """The per-block sums: dip_fit_monitor_nblk(n_hr) + dip_fit_monitor_nblk(n_lr) floats (n_hr is the output's size:
        without img_HR it is only known when the first output arrives)."""
        n = self.lib.dip_fit_monitor_nblk(n_hr) + self.lib.dip_fit_monitor_nblk(self.n_lr)
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
        if self.i >= self.capacity:
            raise RuntimeError(f"dip-amd: SRFitMonitor capacity exceeded ({self.i} recorded, capacity {self.capacity}); "
                               "construct it with capacity >= num_iter")
        hr, lr = out_HR.detach(), out_LR.detach()
        if not hr.is_cuda or not lr.is_cuda or hr.device != self.dev or lr.device != self.dev:
            raise RuntimeError(f"dip-amd: SRFitMonitor.update: the outputs are on {hr.device} / {lr.device}, the monitor "
                               f"lives on {self.dev} (no CPU fallback)")
        self._check_outputs(hr.shape, lr.shape)
        hr, lr = hr.contiguous().float(), lr.contiguous().float()
        with torch.cuda.device(self.dev):        # raw HIP launches go to the current device's streams
            stream = torch.cuda.current_stream(self.dev).cuda_stream
            lptr = None
            if loss is not None:
                self._loss = loss.detach().reshape(1).float()          # keep alive until the launch has run
                lptr = self._loss.data_ptr()
            N.check(self.lib.dip_sr_monitor(hr.data_ptr(), lr.data_ptr(),
                                            self.img_HR.data_ptr() if self.img_HR is not None else None,
                                            self.img_LR.data_ptr(), hr.numel(), self.n_lr, lptr,
                                            self._ensure_partial(hr.numel()).data_ptr(), self.records[self.i].data_ptr(),
                                            stream), "sr_monitor")
        self._keep = (hr, lr)
        self.i += 1

    def _dev_descriptor(self, out_HR, out_LR):
        """DipSRMonitorDesc over this monitor's buffers for the output buffers; `loss` is filled in per iteration."""
        return sr_monitor_descriptor(self, out_HR, out_LR, self.img_HR, self.img_LR, self._ensure_partial(out_HR.numel()),
                                     self.records, self.counter)

    def _plan(self, eng, out, head):
        """(descriptor, launches) of an iteration under `head` (an SRHead whose LR buffer exists) that writes out_HR to `out`."""
        self._check_outputs(out.shape, head.out_LR.shape, who="NativeIteration")
        desc = self._dev_descriptor(out, head.out_LR)
        return desc, sr_monitor_launches(self.lib, desc)

    def _plan_key(self):
        return (id(self), id(self.records), id(self.partial), id(self.counter), id(self.img_LR), id(self.img_HR), self.capacity)

    def _plan_keep(self):
        return (self, self.records, self.partial, self.counter, self.img_LR, self.img_HR)


class RestorationFitMonitor(_DeviceRecords):
    """psrn_masked / psrn and the back-tracking of the restoration closure (restoration.ipynb:192-211) on the device: one record
    per iteration, {loss, mse_masked, mse, psrn_masked, psrn, fell_back}, from the net output against `img` -- masked:
    (out - img) * mask, the notebook's out * img_mask_np against img_masked -- and, when i % show_every == 0, the fall-back to
    the last checkpoint when psrn_masked dropped by more than backtrack_db, or else the checkpoint.  No EMA: the closure has
    none.  `mask` is [1, 1|C, H, W], as for utils.loss_head.MSEHead(mask=).  update() is the eager form (dip_restore_monitor +
    dip_arena_backtrack); NativeIteration(monitor=this) issues dip_restore_monitor_dev, which reads the row index from
    `counter`.  Back-tracking needs a skip() net (flat parameter arena); backtracking=False records only."""
    COLUMNS = ("loss", "mse_masked", "mse", "psrn_masked", "psrn", "fell_back")
    head_kind = None                                                # any head: the record needs the net output only
    backtracking = property(lambda self: self.engine is not None)

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
        self._init_records(img.device, capacity)
        self.img = img.detach().contiguous().float()
        self.mask, self.mask_c = mask.to(self.dev), int(mask.shape[1])
        self.n, self.hw = self.img.numel(), int(img.shape[2] * img.shape[3])
        self.show_every, self.backtrack_db = int(show_every), float(backtrack_db)
        self.state = torch.zeros(4, dtype=torch.float32, device=self.dev)
        self.partial = torch.empty(2 * self.lib.dip_fit_monitor_nblk(self.n), dtype=torch.float32, device=self.dev)

    def update(self, out, loss=None):
        """Call once per closure evaluation, after backward() (like the reference, the fall-back overwrites the parameters
        AFTER the gradients of this iteration were computed)."""
        if self.i >= self.capacity:
            raise RuntimeError(f"dip-amd: RestorationFitMonitor capacity exceeded ({self.i} recorded, capacity {self.capacity}); "
                               "construct it with capacity >= num_iter")
        o = out.detach()
        if o.shape != self.img.shape or not o.is_cuda or o.device != self.dev:
            raise ValueError("dip-amd: RestorationFitMonitor.update: output shape/device does not match the image")
        o = o.contiguous().float()
        with torch.cuda.device(self.dev):        # raw HIP launches go to the current device's streams
            stream = torch.cuda.current_stream(self.dev).cuda_stream
            lptr = None
            if loss is not None:
                self._loss = loss.detach().reshape(1).float()          # keep alive until the launch has run
                lptr = self._loss.data_ptr()
            check = 1 if (self.engine is not None and self.i % self.show_every == 0) else 0      # restoration.ipynb:198
            N.check(self.lib.dip_restore_monitor(o.data_ptr(), self.img.data_ptr(), self.mask.data_ptr(), self.mask_c, self.n,
                                                 self.hw, lptr, self.partial.data_ptr(), self.records[self.i].data_ptr(),
                                                 self.state.data_ptr(), check, self.backtrack_db, stream), "restore_monitor")
            snap = self._ensure_snapshot()
            if snap is not None:
                params = self.engine.params
                N.check(self.lib.dip_arena_backtrack(params.data_ptr(), snap.data_ptr(), params.numel(),
                                                     self.state.data_ptr(), stream), "arena_backtrack")
        self._keep = o
        self.i += 1

    # ------------------------------------------------------------------ the device-indexed form (dip_optim.NativeIteration)
    _ensure_snapshot = FitMonitor._ensure_snapshot

    def _dev_descriptor(self, out):
        """DipRestoreMonitorDesc over this monitor's buffers for the output buffer `out`; `loss` is filled in per iteration."""
        return restore_monitor_descriptor(self, out, self.img, self.mask, self.mask_c, self.hw, self.partial, self.records,
                                          self.counter, self.state)

    def _plan(self, eng, out, head):
        """(descriptor, launches) of an iteration that writes the net output to `out` (dip_optim.NativeIteration)."""
        if tuple(self.img.shape) != tuple(out.shape):
            raise ValueError(f"dip-amd: the RestorationFitMonitor's image is {tuple(self.img.shape)}, the net output is "
                             f"{tuple(out.shape)}")
        desc = self._dev_descriptor(out)
        return desc, restore_monitor_launches(self.lib, desc, eng.params.data_ptr(), eng.params.numel(),
                                              _ptr(self._ensure_snapshot()))

    def _plan_key(self):
        """What a compiled command array (dip_optim.NativeIteration) was built from: buffers by identity, settings by value."""
        return (id(self), id(self.records), id(self.state), id(self.partial), id(self.snapshot), id(self.counter),
                self.show_every, self.backtrack_db, id(self.img), id(self.mask), self.mask_c, id(self.engine), self.capacity,
                self.n, self.hw)

    def _plan_keep(self):
        """The objects behind _plan_key and every buffer the descriptor points to: alive as long as the plan."""
        return (self, self.records, self.state, self.partial, self.snapshot, self.counter, self.img, self.mask, self.engine)


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


def early_stop_descriptor(m, out, ring, mean, partial, records, state, counter, best_out, loss=None):
    """DipEarlyStopDesc of monitor m (window, patience, capacity) over these buffers."""
    return N.DipEarlyStopDesc(_ptr(out), _ptr(ring), _ptr(mean), _ptr(partial), _ptr(records), _ptr(state), _ptr(counter),
                              _ptr(best_out), out.numel(), m.window, m.patience, m.capacity, _ptr(loss))


def early_stop_launches(lib, desc, params_ptr, n_arena, best_params_ptr):
    """The entry point of `desc` -- dip_early_stop_dev, or dip_early_stop_emv_dev for a DipEarlyStopEmvDesc -- and, with a
    best_params arena, dip_early_stop_keep as (fn, args, name) triples."""
    emv = isinstance(desc, N.DipEarlyStopEmvDesc)
    es = [(lib.dip_early_stop_emv_dev if emv else lib.dip_early_stop_dev, (C.byref(desc),),
           "early_stop_emv_dev" if emv else "early_stop_dev")]
    if best_params_ptr is not None:
        es.append((lib.dip_early_stop_keep, (params_ptr, best_params_ptr, n_arena, desc.state), "early_stop_keep"))
    return es


def early_stop_emv_descriptor(m, out, mean, partial, records, state, counter, best_out):
    """DipEarlyStopEmvDesc of monitor m (alpha, warmup, patience, capacity) over these buffers: no ring, no loss."""
    return N.DipEarlyStopEmvDesc(_ptr(out), _ptr(mean), _ptr(partial), _ptr(records), _ptr(state), _ptr(counter), _ptr(best_out),
                                 out.numel(), m.alpha, m.warmup, m.patience, m.capacity, 0)


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


class EarlyStopMonitor(_DeviceRecords):
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
    COLUMNS = ("var", "var_min", "best_iter", "wait", "stopped")
    head_kind = None                                                # any head: the record needs the net output only

    def __init__(self, img_like, window=100, patience=1000, net=None, capacity=16384, *, mode="wmv", alpha=0.1, warmup=None):
        # (what needs no GPU is refused first: the settings, the net)
        if not isinstance(img_like, torch.Tensor):
            raise TypeError("dip-amd: EarlyStopMonitor: img_like is a tensor shaped like the net output ([1,C,H,W])")
        self.mode, self.window, self.alpha, self.warmup, self.patience, capacity = _early_stop_settings(
            "EarlyStopMonitor", mode, window, alpha, warmup, patience, capacity)
        self._init_backtracking(net, net is not None)               # `engine`: the net's, or None without net=
        if not img_like.is_cuda:
            raise RuntimeError("dip-amd: EarlyStopMonitor works on MI355X tensors only (no CPU fallback)")
        self._init_records(img_like.device, capacity)
        self.shape, self.n = tuple(img_like.shape), img_like.numel()
        if self.n < 1:
            raise ValueError("dip-amd: EarlyStopMonitor: img_like is empty")
        self.ring = torch.empty((self.window, self.n), dtype=torch.float32, device=self.dev) if self.mode == "wmv" else None
        self.mean = torch.empty(self.n, dtype=torch.float64, device=self.dev)
        self.partial = torch.empty(self.lib.dip_fit_monitor_nblk(self.n), dtype=torch.float64, device=self.dev)
        self.state = early_stop_state(self.dev)
        self.best_out = torch.zeros(self.shape, dtype=torch.float32, device=self.dev)
        self.best_params = None

    @property
    def memory_bytes(self):
        """Device memory this monitor holds ('wmv': the ring dominates, 4 * window * n; 'emv' has none)."""
        ts = (self.ring, self.mean, self.partial, self.state, self.best_out, self.records, self.counter, self.best_params)
        return sum(t.numel() * t.element_size() for t in ts if t is not None)

    @property
    def best_iter(self):
        """The iteration of the minimum, -1 before the first decision (reads one value; synchronises)."""
        return int(self.state[9].item())

    @property
    def stopped(self):
        """1 once `patience` iterations passed without a new minimum (reads one value; synchronises)."""
        return int(self.state[10].item())

    def _ensure_best_params(self):
        """The arena kept at the minimum, as large as the engine's parameter arena and on its device (None without net=)."""
        if self.engine is None:
            return None
        params = self.engine.params
        if self.best_params is None or self.best_params.numel() != params.numel() or self.best_params.device != params.device:
            self.best_params = torch.zeros_like(params)
        return self.best_params

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
        if self.i >= self.capacity:
            raise RuntimeError(f"dip-amd: EarlyStopMonitor capacity exceeded ({self.i} recorded, capacity {self.capacity}); "
                               "construct it with capacity >= num_iter")
        o = out.detach()
        self._check_out(o.shape, "EarlyStopMonitor.update")
        if not o.is_cuda or o.device != self.dev:
            raise ValueError(f"dip-amd: EarlyStopMonitor.update: the output is on {o.device}, the monitor lives on {self.dev} "
                             "(no CPU fallback)")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("dip-amd: EarlyStopMonitor.update cannot be captured into a hipGraph (the row index is "
                               "host-synchronised state)")
        o = o.contiguous().float()
        with torch.cuda.device(self.dev):        # raw HIP launches go to the current device's streams
            stream = torch.cuda.current_stream(self.dev).cuda_stream
            self._sync_counter()
            for fn, args, name in self._launches(self._dev_descriptor(o)):
                N.check(fn(*args, stream), name)
        self._keep = o
        self._advance(1)

    # ------------------------------------------------------------------ the form inside dip_optim.NativeIteration(early_stop=)
    def _dev_descriptor(self, out):
        """DipEarlyStopDesc ('emv': DipEarlyStopEmvDesc) over this monitor's buffers for the output buffer `out`."""
        if self.mode == "emv":
            return early_stop_emv_descriptor(self, out, self.mean, self.partial, self.records, self.state, self.counter,
                                             self.best_out)
        return early_stop_descriptor(self, out, self.ring, self.mean, self.partial, self.records, self.state, self.counter,
                                     self.best_out)

    def _launches(self, desc):
        """The mode's entry point over `desc` and, with net=, dip_early_stop_keep over the parameter arena."""
        if self.engine is None:
            return early_stop_launches(self.lib, desc, None, 0, None)
        params = self.engine.params
        return early_stop_launches(self.lib, desc, params.data_ptr(), params.numel(), _ptr(self._ensure_best_params()))

    def _plan(self, eng, out, head):
        """(descriptor, launches) of an iteration that writes the net output to `out` (dip_optim.NativeIteration)."""
        self._check_out(out.shape, "NativeIteration")
        desc = self._dev_descriptor(out)
        return desc, self._launches(desc)

    def _plan_key(self):
        """What a compiled command array (dip_optim.NativeIteration) was built from: buffers by identity, settings by value."""
        return (id(self), id(self.records), id(self.state), id(self.ring), id(self.mean), id(self.partial), id(self.best_out),
                id(self.best_params), id(self.counter), self.window, self.patience, id(self.engine), self.capacity, self.n,
                self.mode, self.alpha, self.warmup)

    def _plan_keep(self):
        """The objects behind _plan_key and every buffer the descriptor points to: alive as long as the plan."""
        return (self, self.records, self.state, self.ring, self.mean, self.partial, self.best_out, self.best_params,
                self.counter, self.engine)


class _GroupedRecords:
    """What GroupedFitMonitor and GroupedSRFitMonitor share: settings only, until a dip_group.GroupedFits adopts the monitor
    (once) and exposes the per-instance buffers of its slab rows here as [B, ...] views; `i` is the host's count of issued
    iterations."""
    COLUMNS = ()

    def _init_group(self, capacity):
        self.capacity = int(capacity)
        self.i = 0
        self._group = None         # weak: the group holds the monitor, and a cycle would keep slab and hipGraph alive
        self._adopted = False
        self.records = self.counter = None

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

    def _check_room(self, n):
        """Refuses n more iterations when they do not fit: before anything is issued, eager or replayed."""
        if self.i + int(n) > self.capacity:
            raise RuntimeError(f"dip-amd: {type(self).__name__} capacity exceeded ({self.i} recorded + {int(n)} > capacity "
                               f"{self.capacity}); construct it with capacity >= num_iter")

    def history(self):
        """All records so far as a [B, i, len(COLUMNS)] float32 numpy array (one device->host copy; synchronises)."""
        if self.records is None:
            raise RuntimeError(f"dip-amd: this {type(self).__name__} has not been given to a GroupedFits yet")
        return self.records[:, :self.i].contiguous().cpu().numpy()

    def last(self):
        """The latest record of every instance: a list of B dicts keyed by COLUMNS (synchronises)."""
        if self.records is None or self.i < 1:
            raise RuntimeError(f"dip-amd: {type(self).__name__}.last(): nothing has been recorded yet")
        r = self.records[:, self.i - 1].contiguous().cpu().numpy()
        return [dict(zip(self.COLUMNS, (float(x) for x in row))) for row in r]


class GroupedFitMonitor(_GroupedRecords):
    """The bookkeeping of FitMonitor for the B fits of a dip_group.GroupedFits: settings only.  It owns no device memory; the
    group that adopts it (GroupedFits(..., monitor=this)) places the per-instance buffers in its slab rows and exposes them
    here as [B, ...] views: records [B, capacity, 8], state [B, 4] (writable), counter [B] int32, out_avg [B, C, H, W] and
    snapshot [B, n_arena] (None without back-tracking).  `i` is the host's count of issued iterations."""
    COLUMNS = FitMonitor.COLUMNS

    def __init__(self, imgs_gt=None, exp_weight=0.99, show_every=100, backtrack_db=5.0, backtracking=True, capacity=16384):
        self.imgs_gt = None if imgs_gt is None else list(imgs_gt)
        if self.imgs_gt is not None and any(t is None for t in self.imgs_gt):
            raise ValueError("dip-amd: GroupedFitMonitor: imgs_gt holds one image per instance or is None (all or none)")
        self.exp_weight, self.show_every, self.backtrack_db = float(exp_weight), int(show_every), float(backtrack_db)
        self.backtracking = bool(backtracking)
        self._init_group(capacity)
        if self.show_every <= 0 or self.capacity <= 0:
            raise ValueError("dip-amd: GroupedFitMonitor: show_every and capacity must be > 0")
        self.state = self.out_avg = self.snapshot = None

    def _check_targets(self, targets):
        """imgs_gt against the group's targets: one [1,C,H,W] image per instance, shaped like the target."""
        self._check_images(self.imgs_gt, [t.shape for t in targets], "imgs_gt", "the target")


class GroupedRestorationFitMonitor(_GroupedRecords):
    """RestorationFitMonitor for the B fits of a dip_group.GroupedFits(masks=...): settings only.  The image and the mask are
    the slab's own target and mask rows (no second copy); the group that adopts it places partial sums, records, state, counter
    and -- with back-tracking -- the snapshot in its slab rows, behind everything a monitor-less masked group owns, and exposes
    records [B, capacity, 6], state [B, 4] (writable), counter [B] int32 and snapshot [B, n_arena] (None without back-tracking)
    here.  ONE dip_restore_monitor_dev and ONE dip_arena_backtrack call inside the group bracket serve all B, and every
    instance takes its own decision."""
    COLUMNS = RestorationFitMonitor.COLUMNS

    def __init__(self, show_every=50, backtrack_db=5.0, backtracking=True, capacity=16384):
        self.show_every, self.backtrack_db = int(show_every), float(backtrack_db)
        self.backtracking = bool(backtracking)
        self._init_group(capacity)
        if self.show_every <= 0 or self.capacity <= 0:
            raise ValueError("dip-amd: GroupedRestorationFitMonitor: show_every and capacity must be > 0")
        self.state = self.snapshot = None


class GroupedSRFitMonitor(_GroupedRecords):
    """SRFitMonitor for the B fits of a dip_group.GroupedFits(downsamplers=...): settings only.  The group that adopts it
    places the per-instance buffers -- the optional HR ground truth, the partial sums, the records, the counter -- in its slab
    rows, behind everything a monitor-less super-resolution group owns, and exposes records [B, capacity, 5] and counter [B]
    int32 here.  ONE dip_sr_monitor_dev call inside the group bracket serves all B."""
    COLUMNS = SRFitMonitor.COLUMNS

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


class GroupedEarlyStopMonitor(_GroupedRecords):
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
    COLUMNS = EarlyStopMonitor.COLUMNS

    def __init__(self, mode="wmv", window=100, alpha=0.1, warmup=None, patience=1000, keep_params=True, capacity=16384):
        self.mode, self.window, self.alpha, self.warmup, self.patience, capacity = _early_stop_settings(
            "GroupedEarlyStopMonitor", mode, window, alpha, warmup, patience, capacity)
        self.keep_params = bool(keep_params)
        self._init_group(capacity)
        self.state = self.best_out = self.best_params = self.ring = self.mean = self.partial = None

    def _views(self):
        if self.state is None:
            raise RuntimeError("dip-amd: this GroupedEarlyStopMonitor has not been given to a GroupedFits yet")
        return (self.ring, self.mean, self.partial, self.records, self.state, self.counter, self.best_out, self.best_params)

    @property
    def memory_bytes(self):
        """Device memory the B instances hold for early stopping (as EarlyStopMonitor.memory_bytes, times B)."""
        return sum(t.numel() * t.element_size() for t in self._views() if t is not None)

    @property
    def best_iter(self):
        """The iteration of every instance's minimum, -1 before its first decision: B ints (one copy; synchronises)."""
        return self._views()[4][:, 9].tolist()

    @property
    def stopped(self):
        """Per instance, 1 once `patience` iterations passed without a new minimum: B ints (one copy; synchronises)."""
        return self._views()[4][:, 10].tolist()

    def restore_best(self, b=None):
        """Copies best_params back over the parameter row of instance b (None: of every instance): nets[b] then produces
        best_out[b] again."""
        self._views()
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
