"""Device-side bookkeeping for the notebooks' closures (no counterpart file in the reference: the
reference does this work inline, on the host, in every closure -- denoising.ipynb:214-248,
restoration.ipynb:192-211).

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
The reference's per-iteration cost this replaces: three `.detach().cpu().numpy()` of the output, a
`.item()`, and -- whenever `i % show_every` is non-zero -- a copy of all 2.2 M parameters to the CPU.
"""
import ctypes as C
import weakref

import numpy as np
import torch

import dip_native as N


class FitMonitor:
    COLUMNS = ("loss", "mse_noisy", "mse_gt", "mse_gt_sm", "psrn_noisy", "psrn_gt", "psrn_gt_sm", "fell_back")

    def __init__(self, net, img_noisy, img_gt=None, exp_weight=0.99, show_every=100, backtrack_db=5.0,
                 backtracking=True, capacity=16384):
        if not img_noisy.is_cuda:
            raise RuntimeError("dip-amd: FitMonitor works on MI355X tensors only (no CPU fallback)")
        self.lib = N.lib()
        self.dev = img_noisy.device
        self.noisy = img_noisy.detach().contiguous().float()
        self.gt = None if img_gt is None else img_gt.detach().to(self.dev).contiguous().float()
        if self.gt is not None and self.gt.shape != self.noisy.shape:
            raise ValueError("FitMonitor: img_gt and img_noisy differ in shape")
        self.n = self.noisy.numel()
        self.exp_weight, self.show_every, self.backtrack_db = float(exp_weight), int(show_every), float(backtrack_db)
        self.capacity = int(capacity)
        self.records = torch.zeros((self.capacity, 8), dtype=torch.float32, device=self.dev)
        self.state = torch.zeros(4, dtype=torch.float32, device=self.dev)
        self.partial = torch.empty(4 * self.lib.dip_fit_monitor_nblk(self.n), dtype=torch.float32, device=self.dev)
        self.out_avg = torch.zeros_like(self.noisy)
        self.i = 0
        # the iteration index as dip_fit_monitor_dev reads it (NativeIteration(monitor=)), and the value it will hold once
        # all issued work has run; update() passes `i` by value and leaves both alone, NativeIteration re-aligns them
        self.counter = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self._counter_host = 0
        self.engine = None
        self.snapshot = None
        if backtracking:
            eng = getattr(net, "__dict__", {}).get("_dip_engine")
            if eng is None:
                raise RuntimeError("dip-amd: back-tracking needs a net built by models.skip.skip() (flat parameter arena)")
            if getattr(eng, "kind", "skip") != "skip":
                raise NotImplementedError("dip-amd: FitMonitor back-tracking covers skip() nets only; construct it with "
                                          "backtracking=False for a ResNet")
            self.engine = eng

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
        ptr = lambda t: None if t is None else t.data_ptr()
        return N.DipFitMonitorDesc(ptr(out), ptr(self.noisy), ptr(self.gt), ptr(self.out_avg), self.n, self.exp_weight,
                                   self.backtrack_db, None, ptr(self.partial), ptr(self.records), self.capacity,
                                   self.show_every, 1 if self.engine is not None else 0, 0, ptr(self.counter), ptr(self.state))

    def _sync_counter(self):
        """Sets the device counter to `i` on the current stream when it would not hold it (update() calls since the last
        native iteration, or an `i` set by hand)."""
        if self._counter_host != self.i:
            self.counter.fill_(self.i)
            self._counter_host = self.i

    def _advance(self, n):
        """n iterations were issued through dip_fit_monitor_dev."""
        self.i += n
        self._counter_host += n

    def history(self):
        """All records so far as a [iters, 8] float32 numpy array (synchronises once)."""
        return self.records[:self.i].cpu().numpy()

    def last(self):
        """The latest record as a dict (synchronises)."""
        r = self.records[self.i - 1].cpu().numpy()
        return dict(zip(self.COLUMNS, (float(x) for x in r)))


class GroupedFitMonitor:
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
        self.backtracking, self.capacity = bool(backtracking), int(capacity)
        if self.show_every <= 0 or self.capacity <= 0:
            raise ValueError("dip-amd: GroupedFitMonitor: show_every and capacity must be > 0")
        self.i = 0
        self._group = None         # weak: the group holds the monitor, and a cycle would keep slab and hipGraph alive
        self._adopted = False
        self.records = self.state = self.counter = self.out_avg = self.snapshot = None

    def _check_targets(self, targets):
        """imgs_gt against the group's targets: one [1,C,H,W] image per instance, shaped like the target."""
        if self.imgs_gt is None:
            return
        if len(self.imgs_gt) != len(targets):
            raise ValueError(f"dip-amd: GroupedFitMonitor has {len(self.imgs_gt)} imgs_gt for {len(targets)} instances")
        for b, (gt, t) in enumerate(zip(self.imgs_gt, targets)):
            if tuple(gt.shape) != tuple(t.shape):
                raise ValueError(f"dip-amd: GroupedFitMonitor: imgs_gt[{b}] is {tuple(gt.shape)}, the target is {tuple(t.shape)}")

    @property
    def group(self):
        """The GroupedFits that adopted this monitor (None before adoption, or once that group is gone)."""
        return None if self._group is None else self._group()

    def _adopt(self, group, records, state, counter, out_avg, snapshot):
        self._group, self._adopted = weakref.ref(group), True
        self.records, self.state, self.counter, self.out_avg, self.snapshot = records, state, counter, out_avg, snapshot

    def _check_room(self, n):
        """Refuses n more iterations when they do not fit: before anything is issued, eager or replayed."""
        if self.i + int(n) > self.capacity:
            raise RuntimeError(f"dip-amd: GroupedFitMonitor capacity exceeded ({self.i} recorded + {int(n)} > capacity "
                               f"{self.capacity}); construct it with capacity >= num_iter")

    def history(self):
        """All records so far as a [B, i, 8] float32 numpy array (one device->host copy; synchronises)."""
        if self.records is None:
            raise RuntimeError("dip-amd: this GroupedFitMonitor has not been given to a GroupedFits yet")
        return self.records[:, :self.i].contiguous().cpu().numpy()

    def last(self):
        """The latest record of every instance: a list of B dicts keyed by COLUMNS (synchronises)."""
        if self.records is None or self.i < 1:
            raise RuntimeError("dip-amd: GroupedFitMonitor.last(): nothing has been recorded yet")
        r = self.records[:, self.i - 1].contiguous().cpu().numpy()
        return [dict(zip(self.COLUMNS, (float(x) for x in row))) for row in r]
