"""Grouped multi-instance execution: B independent fits of one architecture -- B copies of
the reference's skip-net (models/skip.py:45-100) with own weights, own BatchNorm statistics, own Adam state, own input,
target and reg-noise stream, each advancing through the body of the reference's optimize() loop
(utils/common_utils.py:226-230) with the notebooks' closure (denoising.ipynb:204-221, inpainting.ipynb:295-313) --
through ONE launch list: every kernel launch of an iteration serves all B instances (gridDim.z x B workgroups;
csrc/dip_group.h), instead of B launch lists on B streams.  What fills an MI355X when one image (the 384x256 snail net:
~25 us of math per iteration) cannot: the B-streams form is bound by the dispatch rate of the command processor
(profiles/r03_dispatch_rate.txt), the grouped form issues 1/B of the launches.

Memory: EVERY buffer of a fit -- parameter / gradient / Adam arenas, BatchNorm state, packed weights, activations, scratch,
descriptor tables, net input, noise state, target, mask, output, loss -- is carved from one slab per instance; the B slabs
are the rows of one [B][stride] allocation, laid out identically.  The launch list is compiled for instance 0 (the
SkipEngine of nets[0], with the slab as its allocator) and issued between dip_group_begin / dip_group_end; instance b sees
every pointer advanced by b * stride.  Plans, tile walks and summation orders are those of a solo fit, so every instance
is bit-identical to the same fit run on its own (tests/test_group_gpu.py).

    g = GroupedFits(nets, net_inputs, targets, masks=None, reg_noise_std=1/30, seeds=range(B), lr=0.01, exp_weight=0.99)
    g.capture()                     # 3 eager warm-up iterations, then ONE hipGraph of the grouped iteration
    g.run(num_iter - 3)
    g.losses                        # [B] device tensor: total_loss of the last iteration, per instance
    g.out, g.out_avg                # [B, C, H, W]: network outputs / their exponential moving averages
    nets[b].state_dict()            # the parameters of nets[b] are views of its slab: always current

Super-resolution (super-resolution.ipynb:169-186 of the reference; the batches of super-resolution_eval_script.py and the arms
of sr_prior_effect.ipynb): `downsamplers=[...]`, one fixed-taps models.downsampler.Downsampler per instance, switches the
tail of every instance to the one of utils.loss_head.SRHead -- the whole net, dip_head_fwd, dip_sr_loss_fwd, dip_sr_loss_bwd
-- with `targets` the LR images.  The taps are per-instance data of the slab like the targets, so the instances may use
different taps of one (k, factor, pad); there is no mask.

    g = GroupedFits(nets, net_inputs, imgs_LR, downsamplers=downs, reg_noise_std=0.03)
    g.out, g.out_LR                 # [B, C, H, W] HR outputs, [B, C, Ho, Wo] their down-sampled versions

`tv_weights=` adds the TV prior of the same closure (total_loss = mse(out_LR, img_LR) + tv_weight * tv_loss(out_HR);
super-resolution.ipynb:180-181, sr_prior_effect.ipynb:109): the tail of SRHead(tv_weight=) -- dip_head_fwd, dip_sr_tv_loss_fwd,
dip_sr_tv_loss_bwd -- with the weight ONE float of every instance's slab, so a TV-weight sweep over one image is one group:

    g = GroupedFits(nets, net_inputs, [img_LR] * B, downsamplers=downs, tv_weights=[1e-7, 1e-6, 1e-5], tv_beta=0.5)

One float serves all instances; None or all zeros is the group above; zero and positive weights do not mix.

The rest of the denoising closure (denoising.ipynb:214-248: the exponential average of the output, three PSNRs, the parameter
checkpoint and the 5 dB fall-back; restoration.ipynb:192-211 is GroupedRestorationFitMonitor, below), per fit and with no Python
between the iterations:
`monitor=utils.fit_monitor.GroupedFitMonitor(imgs_gt, ...)`.  The monitor's state -- gt, out_avg, partial sums, records, state,
counter, snapshot -- is per-instance data of the slab like the targets; dip_fit_monitor_dev and dip_arena_backtrack are issued
inside the group bracket after the backward pass and before Adam (where monitor.update(out, loss) stands in the eager closure),
three dispatches for all B, and every instance takes its own snapshot / fall-back decision.  Instance b is bit-identical to
the same fit on its own under utils.fit_monitor.FitMonitor (tests/test_group_monitor_gpu.py).  The monitor carries the EMA:
exp_weight= / ema_init= are not combined with it, and out_avg starts from the first output.

    mon = GroupedFitMonitor(imgs_gt, exp_weight=0.99, show_every=100, capacity=num_iter)
    g = GroupedFits(nets, net_inputs, imgs_noisy, reg_noise_std=1/30, monitor=mon)
    g.capture(); g.run(num_iter - 3)            # the monitor's launches are part of the ONE hipGraph
    mon.history()                               # [B, iters, 8]; mon.last(), mon.out_avg (= g.out_avg), mon.state, mon.snapshot

A super-resolution group takes `monitor=utils.fit_monitor.GroupedSRFitMonitor(imgs_HR=None, capacity=...)` instead: the
psnr_LR / psnr_HR record of super-resolution.ipynb:188-191 per fit (utils.fit_monitor.SRFitMonitor has the columns).  Its
buffers -- the optional HR ground truth, the partial sums, the records, the counter -- are per-instance data of the slab behind
everything a monitor-less super-resolution group owns; ONE descriptor and ONE dip_sr_monitor_dev call inside the group bracket,
after the backward pass and before Adam, serve all B (two dispatches), inside the ONE hipGraph of capture().  Instance b's
records are bit-identical to the solo NativeIteration + SRFitMonitor fit; the fit itself is untouched, and out_avg stays None
(this closure has no moving average: exp_weight= / ema_init= are refused with it).

    mon = GroupedSRFitMonitor(imgs_HR, capacity=num_iter)
    g = GroupedFits(nets, net_inputs, imgs_LR, downsamplers=downs, reg_noise_std=0.03, monitor=mon)
    g.capture(); g.run(num_iter - 3); mon.history()        # [B, iters, 5]: loss, mse_LR, mse_HR, psnr_LR, psnr_HR

A masked group (masks=[...]: the restoration / inpainting closure, restoration.ipynb:180-219) takes
`monitor=utils.fit_monitor.GroupedRestorationFitMonitor(show_every=50, backtrack_db=5.0, ...)`: psrn_masked and psrn per fit and
iteration (restoration.ipynb:192-193) and, ON every show_every-th iteration, the fall-back to the last checkpoint when psrn_masked
dropped by more than 5 dB or else the checkpoint (:198-211).  Its descriptor points at the slab's own target and mask rows (no
second copy of either); partial sums, records, state, counter and -- with back-tracking -- the snapshot are per-instance data of
the slab behind everything a monitor-less masked group owns.  ONE dip_restore_monitor_dev and ONE dip_arena_backtrack call inside
the group bracket, after the backward pass and before Adam, serve all B inside the ONE hipGraph of capture(); every instance
takes its own decision and is bit-identical to the solo NativeIteration + RestorationFitMonitor fit.  It needs masks=, is not
combined with downsamplers= or exp_weight= / ema_init= (this closure has no moving average: out_avg stays None).

    mon = GroupedRestorationFitMonitor(show_every=50, capacity=num_iter)
    g = GroupedFits(nets, net_inputs, imgs, masks=masks, monitor=mon)
    g.capture(); g.run(num_iter - 3); mon.history()        # [B, iters, 6]: loss, mse_masked, mse, psrn_masked, psrn, fell_back

When to stop, per fit and without a ground truth: `early_stop=utils.fit_monitor.GroupedEarlyStopMonitor(mode='wmv'|'emv', ...)`,
a keyword of its own next to monitor=, independent of it, for all three group kinds (the record needs the net output only).
Its buffers -- the ring ('wmv' only: window * n floats per instance; 'emv', the exponential moving variance, has none), the fp64
mean, the partials, the records, the 64-byte state, the counter, best_out and, with keep_params, best_params -- are per-instance
data of the slab behind everything else, the monitor= buffers included.  ONE dip_early_stop_dev ('emv': dip_early_stop_emv_dev)
and ONE dip_early_stop_keep call inside the group bracket, behind the monitor's launches and in front of Adam, serve all B
inside the ONE hipGraph of capture(); every instance takes its own decision and is bit-identical to the solo
NativeIteration(early_stop=EarlyStopMonitor(net=...)) fit (tests/test_group_early_stop_gpu.py).  A stopped instance's early-stop
state freezes; its fit goes on, because a row cannot leave the launch list.

    mon = GroupedEarlyStopMonitor(mode='emv', alpha=0.1, patience=1000, capacity=num_iter)
    g = GroupedFits(nets, net_inputs, imgs_noisy, reg_noise_std=1/30, early_stop=mon)
    g.capture(); issued = 3 + g.run_until(num_iter - 3, check_every=50)     # one copy of B words and one sync per 50 iterations
    mon.best_iter, mon.stopped                  # B ints each; mon.history() [B, iters, 5], mon.best_out [B, C, H, W]
    mon.restore_best()                          # nets[b] carries the parameters of its minimum again (b=: one instance)

The mean structural similarity of every instance's output against its ground truth: `ssim=utils.fit_monitor.GroupedSSIMMonitor(
imgs_gt, with_avg=False)`, a third keyword for all three group kinds (a super-resolution group: imgs_gt are the HR images).  Its
buffers -- the ground truth, the partials, the records, the counter -- are per-instance data of the slab behind the es_ rows; ONE
dip_ssim_dev call inside the group bracket, behind the monitor= and early_stop= launches and in front of Adam, serves all B inside
the ONE hipGraph of capture(), and instance b's records are those of the solo NativeIteration(ssim=SSIMMonitor(...)) fit, bit for
bit (tests/test_ssim_gpu.py).  with_avg=True also records the SSIM of the smoothed output: it reads the out_avg rows of
monitor=GroupedFitMonitor(...).

    sm = GroupedSSIMMonitor(imgs_gt, capacity=num_iter)
    g = GroupedFits(nets, net_inputs, imgs_noisy, reg_noise_std=1/30, ssim=sm)
    g.capture(); g.run(num_iter - 3); sm.history()         # [B, iters, 2]: ssim, ssim_sm

SGLD fits (dip_optim.FusedAdam(weight_decay=, noise_std=, noise_seed=) per instance): `weight_decay=`, `param_noise_std=` (one
float or B floats: a noise-level sweep in one launch list) and `param_noise_seeds=` (default: `seeds`).  With one of them set
ONE grouped dip_adam_sgld_step_dev takes dip_adam_step_dev's place inside the bracket and the hipGraph, and the DipSgldState
{offset, seed, std} and the range table of the 4-D parameters are two more rows of the slab, behind everything else; without
them launch list and slab are what they were.  g.set_param_noise_std(x_or_list) rewrites the levels in stream order.  Every
instance is bit-identical to its solo NativeIteration fit with the same seeds (tests/test_sgld_fit_gpu.py).

    g = GroupedFits(nets, net_inputs, imgs_noisy, reg_noise_std=1/30, weight_decay=5e-8, param_noise_std=[1e-4, 2e-4, 4e-4])

The posterior of such fits, per instance and pooled: `posterior=utils.fit_monitor.GroupedPosteriorMonitor(burn_in, every=1,
imgs_gt=None)`, a fourth keyword for all three group kinds (a super-resolution group samples the HR output).  Its rows -- mean,
m2, the sample count and the iteration counter; with imgs_gt also the ground truth, fp64 partials and a [capacity, 3] record
table of the posterior mean's PSNR, one row per sample -- are per-instance data of the slab behind everything else a row owns,
the sgld and the lr / reg_std rows included, and only when the keyword is set.  ONE dip_posterior_dev (imgs_gt:
dip_posterior_rec_dev) call inside the group bracket, behind the early_stop= launches and in front of ssim= and Adam -- the order
of a solo NativeIteration -- serves all B inside the ONE hipGraph of capture(), and instance b's rows are those of the solo
NativeIteration(posterior=PosteriorMonitor(...)) fit, bit for bit (tests/test_group_posterior_gpu.py).  B instances over one
image with different param_noise_seeds are B independent chains: pm.pooled(chains=None) is ONE dip_posterior_pool launch outside
the bracket over the rows -- the pooled mean, the within-chain variance W, the Gelman-Rubin estimate V and R-hat = sqrt(V / W)
per element, and {mean, max, degenerate count} of R-hat as three doubles -- with nothing going through the host.

    pm = GroupedPosteriorMonitor(burn_in=7000, every=50, imgs_gt=[img] * B)
    g = GroupedFits(nets, [z] * B, [img_noisy] * B, reg_noise_std=1/30, weight_decay=5e-8, param_noise_std=1e-4,
                    param_noise_seeds=[1, 2, 3], posterior=pm)
    g.capture(); g.run(num_iter - 3)
    pm.mean, pm.variance(), pm.count            # [B, C, H, W] each; the host's sample count, no synchronisation
    pm.history()                                # [B, count, 3]: iteration, mse_mean, psnr_mean
    p = pm.pooled(); p.mean, p.var, p.rhat, p.summary           # [1, C, H, W] each; fp64 [3]

Learning-rate and input-noise sweeps: `lr=[B floats]` and / or `reg_noise_std=[B floats]` (a float is the group above, launch
for launch and byte for byte of slab).  A list puts the values into the slab -- one fp64 row `lr`, one fp32 row `reg_std`, behind
everything else the group owns, so no other row moves -- and ONE grouped dip_adam_tick_dev / dip_noise_axpy_dev3 stands where
dip_adam_tick / dip_noise_axpy_dev2 stood, inside the bracket and the ONE hipGraph; every instance reads the scalar of its own
row.  g.set_lr(list) / g.set_reg_noise_std(list) rewrite the rows in stream order (a schedule: run(k); set_lr([lr] * B);
run(k)), without a re-capture.  A construction list that mixes zero and positive noise levels is refused (a solo fit at level 0
feeds `saved` itself; on the noise path a -0.0 of the input comes out as +0.0); all zeros is the float 0; the setter may take an
instance to 0 (saved + 0 * N).  Every instance is bit-identical to its solo NativeIteration fit with FusedAdam(lr=lr[b]) and
RegNoise(std[b], seeds[b]) (tests/test_sweep_fit_gpu.py).

    g = GroupedFits(nets, [z] * B, [img] * B, lr=[0.01, 0.001, 0.1], reg_noise_std=[1/30, 1/20, 0.03])

There is no CPU or per-instance fallback here: the library must be loaded, and an architecture / size mismatch raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C

import torch

import dip_native as N
from dip_native import round_up

_ALIGN = 256


class Slab:
    """Bump allocator over one row of the [B][stride] allocation.  First pass (no buffer bound): hands out ordinary torch
    tensors and only measures; second pass (bind()): the same sequence of requests returns views of row 0."""

    def __init__(self, device):
        self.device = device
        self.buf = None
        self.off = 0
        self.sizes = []

    def bind(self, row0: torch.Tensor):
        self.buf, self.measured, self.off, self.replay = row0, self.off, 0, 0

    def alloc(self, n, dtype=torch.float32, zero=False):
        nbytes = int(n) * torch.empty((), dtype=dtype).element_size()
        step = round_up(max(nbytes, 1), _ALIGN)
        if self.buf is None:
            self.sizes.append(step)
            self.off += step
            return (torch.zeros if zero else torch.empty)(int(n), dtype=dtype, device=self.device)
        if self.replay >= len(self.sizes) or self.sizes[self.replay] != step or self.off + step > self.buf.numel():
            raise RuntimeError("dip-amd Slab: the second build asked for different buffers than the measuring one")
        self.replay += 1
        t = self.buf[self.off:self.off + nbytes].view(dtype)
        self.off += step
        if zero:
            t.zero_()
        return t


class GroupedFits:
    ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8

    def __init__(self, nets, net_inputs, targets, masks=None, reg_noise_std=0.0, seeds=None, lr=0.01, exp_weight=None,
                 ema_init="first", device=None, _dry_cpu=False, downsamplers=None, monitor=None, tv_weights=None, tv_beta=0.5,
                 early_stop=None, weight_decay=0.0, param_noise_std=0.0, param_noise_seeds=None, ssim=None, posterior=None):
        """nets: B nets of models.skip.skip() with identical architecture; net_inputs / targets (/ masks): one tensor per
        instance, identical shapes ([1,C,H,W]; masks [1,1|Cout,H,W] or None).  reg_noise_std / seeds: the closure's input
        noise (utils.reg_noise.RegNoise; seeds default to 0..B-1).  lr / reg_noise_std: one float, or B floats = a sweep: the
        values become per-instance rows of the slab (`lr` fp64, `reg_std` fp32, behind everything else) read by ONE grouped
        dip_adam_tick_dev / dip_noise_axpy_dev3; set_lr / set_reg_noise_std rewrite them.
        exp_weight: None = no moving average of the output;
        ema_init 'first' = out_avg starts as the first output (denoising.ipynb:214-215), 'zeros' = starts at 0.
        downsamplers: None = the denoising / inpainting closure; B fixed-taps Downsamplers of one (k, factor, pad) = the
        super-resolution closure, targets = the LR images [1,C,Ho,Wo], no masks.
        monitor: None, or a utils.fit_monitor.GroupedFitMonitor: EMA, PSNR records and back-tracking per instance, inside
        the launch list (then exp_weight / ema_init stay at their defaults: the monitor carries the weight and starts from
        the first output, as FitMonitor does); with downsamplers= a utils.fit_monitor.GroupedSRFitMonitor: the psnr_LR /
        psnr_HR record per instance (no moving average: exp_weight / ema_init stay at their defaults, out_avg stays None); with
        masks= a utils.fit_monitor.GroupedRestorationFitMonitor: psrn_masked / psrn records and back-tracking per instance
        (restoration.ipynb:192-211; no moving average either).
        tv_weights (with downsamplers= only): None, one float for all instances or B floats -- total_loss = mse(out_LR, img_LR)
        + tv_weights[b] * tv_loss(out_HR, tv_beta), the tail of SRHead(tv_weight=); all zero = None; a mix of zero and positive
        weights is refused (an instance with weight 0 on the TV path would differ from its solo fit where s == 0).
        early_stop: None, or a utils.fit_monitor.GroupedEarlyStopMonitor: the ground-truth-free stopping criterion per instance
        ('wmv' or the ring-free 'emv'), inside the launch list behind monitor='s launches and in front of Adam; independent of
        monitor= and of the group kind (the record needs the net output only).  run_until() polls it.
        weight_decay / param_noise_std / param_noise_seeds: SGLD fits (dip_optim.FusedAdam(weight_decay=, noise_std=,
        noise_seed=) per instance): param_noise_std is one float or B floats -- a noise-level sweep in one launch list -- the
        seeds default to `seeds`.  With one of them set ONE grouped dip_adam_sgld_step_dev takes dip_adam_step_dev's place and
        two rows join the slab behind everything else: the DipSgldState and the range table of the 4-D parameters.
        ssim: None, or a utils.fit_monitor.GroupedSSIMMonitor: the mean structural similarity of every instance's output against
        its ground truth (with_avg: of the GroupedFitMonitor's smoothed output too), inside the launch list behind the
        early_stop= launches and in front of Adam; independent of the group kind.  Its rows join the slab behind the es_ rows.
        posterior: None, or a utils.fit_monitor.GroupedPosteriorMonitor: the sample mean and m2 of every instance's outputs after
        a burn-in (with imgs_gt: the PSNR of that mean too), inside the launch list behind the early_stop= launches and in front
        of ssim= and Adam; independent of the group kind.  Its rows join the slab behind everything else, the sgld and the lr /
        reg_std rows included; posterior.pooled() pools the B chains (dip_posterior_pool)."""
        B = len(nets)
        if B < 1 or len(net_inputs) != B or len(targets) != B or (masks is not None and len(masks) != B):
            raise ValueError("GroupedFits: one net, one input, one target (and one mask) per instance")
        self.monitor = self._check_monitor(monitor, downsamplers, exp_weight, ema_init, targets, masks)
        self.early_stop = self._check_monitor_slot(early_stop, "early_stop")
        self.ssim = self._check_ssim(ssim, B, self.monitor, exp_weight)
        self.posterior = self._check_posterior(posterior, B, targets, downsamplers)
        self.downsamplers = None if downsamplers is None else self._check_downsamplers(downsamplers, B, masks)
        self.tv_weights, self.tv_beta = self._check_tv(tv_weights, tv_beta, B, downsamplers)
        self.weight_decay, self.param_noise_std, self.param_noise_seeds = self._check_sgld(
            weight_decay, param_noise_std, param_noise_seeds, B, [int(s) for s in (seeds if seeds is not None else range(B))])
        # (explicit zeros are the defaults: the launch list and the slab of a group without SGLD)
        self.sgld = self.weight_decay != 0.0 or any(s != 0.0 for s in self.param_noise_std) or param_noise_seeds is not None
        # (a float: today's group; a list: the values are rows of the slab)
        lr, reg_noise_std = self._check_sweep(lr, "lr", B), self._check_sweep(reg_noise_std, "reg_noise_std", B)
        engs = [getattr(n, "__dict__", {}).get("_dip_engine") for n in nets]
        if any(e is None or isinstance(e, Exception) for e in engs):
            raise RuntimeError("dip-amd: GroupedFits needs nets built by models.skip.skip()")
        if any(e.kind != "skip" for e in engs):
            raise NotImplementedError("dip-amd: GroupedFits covers skip() nets only (the ResNet backbone has no grouped "
                                      "launch list)")
        if device is None:
            device = net_inputs[0].device
        device = torch.device(device)
        # (_dry_cpu: the slab construction alone, on host memory, for the layout unit test -- nothing can be launched)
        self._dry = bool(_dry_cpu)
        if device.type != "cuda" and not self._dry:
            raise RuntimeError("dip-amd: GroupedFits runs on an MI355X only (no CPU fallback in this backend)")
        self.B, self.nets, self.device = B, list(nets), device
        self.eng = eng = engs[0]
        self.lib = N.lib()
        self.lr, self.std = lr, reg_noise_std
        self._lr_rows, self._std_rows = isinstance(lr, list), isinstance(reg_noise_std, list)
        self._noisy = self._std_rows or self.std > 0
        self.exp_weight = None if exp_weight is None else float(exp_weight)
        if ema_init not in ("first", "zeros"):
            raise ValueError("GroupedFits: ema_init is 'first' or 'zeros'")
        self.ema_first = ema_init == "first"
        self.seeds = [int(s) for s in (seeds if seeds is not None else range(B))]
        self.iterations = 0
        self.graph = None
        # --- same architecture, same sizes
        sig0 = [(k, tuple(p.shape)) for k, p in nets[0].named_parameters()]
        for b, n in enumerate(nets):
            if [(k, tuple(p.shape)) for k, p in n.named_parameters()] != sig0:
                raise ValueError(f"GroupedFits: net {b} differs from net 0 in architecture")
            if not n.training:
                raise NotImplementedError("dip-amd: eval-mode BatchNorm is not implemented")
        z0, t0 = net_inputs[0], targets[0]
        if z0.dim() != 4 or z0.shape[0] != 1:
            raise ValueError("GroupedFits: net inputs are [1,C,H,W]")
        for b in range(B):
            if net_inputs[b].shape != z0.shape or targets[b].shape != t0.shape:
                raise ValueError(f"GroupedFits: instance {b} differs from instance 0 in input / target shape")
            if masks is not None and (masks[b] is None) != (masks[0] is None):
                raise ValueError("GroupedFits: either every instance has a mask or none has")
        oc = eng.out_conv
        if oc.ks != 1 or oc.Cout > 4:
            raise NotImplementedError("dip-amd: the fused loss head covers a 1x1 output conv with <= 4 channels")
        if t0.dim() != 4 or t0.shape[0] != 1 or t0.shape[1] != oc.Cout:
            raise ValueError(f"GroupedFits: targets must be [1,{oc.Cout},H,W], got {tuple(t0.shape)}")
        if self.downsamplers is not None and self.downsamplers[0].downsampler_.weight.shape[0] != oc.Cout:
            raise ValueError(f"GroupedFits: the Downsamplers have {self.downsamplers[0].downsampler_.weight.shape[0]} planes, "
                             f"the net output has {oc.Cout}")
        self.mask_c = 0
        m0 = None
        if masks is not None and masks[0] is not None:
            m0 = self._mask4(masks[0])
            if m0.shape[1] not in (1, oc.Cout) or m0.shape[2:] != t0.shape[2:]:
                raise ValueError(f"GroupedFits: masks must be [1,1|{oc.Cout},H,W]")
            self.mask_c = int(m0.shape[1])
        _, Cimg, H, W = z0.shape
        # --- the slab: a measuring build, the allocation, the real build into row 0
        with self._devctx():
            slab = Slab(device)
            try:
                self._build_row0(slab, Cimg, H, W, t0, m0)
                self.stride = slab.off                               # a multiple of 256 by construction
                del self._x, self._row0_extra
                self._raw = torch.zeros(B * self.stride + _ALIGN, dtype=torch.uint8, device=device)
                o = (-self._raw.data_ptr()) % _ALIGN                  # (the device allocator aligns to >= 256 anyway)
                self.mem = self._raw[o:o + B * self.stride]
                slab.bind(self.mem[:self.stride])
                self._build_row0(slab, Cimg, H, W, t0, m0)
                if slab.off != self.stride:
                    raise RuntimeError("dip-amd GroupedFits: the slab build is not reproducible")
            finally:
                eng.slab = None            # whatever happened: a later (re-)plan of nets[0] uses torch's allocator
                if not hasattr(self, "mem") or slab.buf is None or slab.off != getattr(self, "stride", -1):
                    eng.device = None      # ... and a half-built engine state is rebuilt by the next forward
            # --- rows 1..B-1: a copy of row 0 (descriptor tables, constants, zeroed state), then what is the instance's own
            rows = self.mem.view(B, self.stride)
            if B > 1:
                rows[1:].copy_(rows[:1].expand(B - 1, self.stride))
            ex, mon = self._row0_extra, self.monitor
            own = (("saved", lambda b: net_inputs[b]), ("target", lambda b: targets[b]), ("mask", lambda b: self._mask4(masks[b])),
                   ("taps", lambda b: self.downsamplers[b]._taps), ("mon_gt", lambda b: mon.imgs_gt[b]),
                   ("mon_hr", lambda b: mon.imgs_HR[b]), ("ssim_gt", lambda b: self.ssim.imgs_gt[b]),
                   ("post_gt", lambda b: self.posterior.imgs_gt[b]))
            with torch.no_grad():
                for b in range(B):
                    if b > 0:
                        self._adopt_net(b)
                    for k, src in own:                       # the instance's own data, where row 0 has such a buffer
                        if ex.get(k) is not None:
                            self._inst(ex[k], b).copy_(src(b).detach().to(device).float().reshape(-1))
                    if self.tv_weights is not None:
                        self._inst(ex["tv_weight"], b).fill_(self.tv_weights[b])
                    self._inst(ex["rng"], b).copy_(torch.tensor([0, self.seeds[b]], dtype=torch.int64))
                    if self.sgld:
                        self._inst(ex["sgld"], b).copy_(self._sgld_state(b))
                    if self._lr_rows:
                        self._inst(ex["lr"], b).fill_(self.lr[b])
                    if self._std_rows:
                        self._inst(ex["reg_std"], b).fill_(self.std[b])
            # --- what the caller reads: strided views over the instances
            hr = (oc.Cout, eng.Hout, eng.Wout)
            self.losses = self._strided(ex["loss"])
            self.out = self._strided(ex["out"], *hr)
            self.out_LR = self._strided(ex.get("y"), *t0.shape[1:])
            self.out_avg = torch.zeros((B,) + hr, dtype=torch.float32, device=device) if self.exp_weight is not None else None
            for m, prefix, _, _ in self._monitors():          # the [B, ...] views a grouped monitor exposes, from its table
                z = self._monitor_sizes(m)
                shape = lambda b: b.shape(z) if b.shape else (b.count(z),)
                m._adopt(self, **{b.name: self._strided(ex[prefix + (b.key or b.name)], *shape(b)) for b in m.BUFFERS if b.view})
            if getattr(mon, "out_avg", None) is not None:     # GroupedFitMonitor: the monitor carries the moving average
                self.out_avg = mon.out_avg
            self._nbt_all = self._strided(eng.nbt, eng.nbt.numel())
            if not self._dry:
                torch.cuda.synchronize(device)

    # ------------------------------------------------------------------ construction helpers
    def _devctx(self):
        return contextlib.nullcontext() if self._dry else torch.cuda.device(self.device)

    _SLOTS = (("monitor", "mon_", "_mdesc", "_mon"), ("early_stop", "es_", "_edesc", "_es"),
              ("posterior", "post_", "_pdesc", "_post"), ("ssim", "ssim_", "_sdesc", "_ssim"))

    def _monitors(self):
        """The monitors of this group in launch order -- monitor=, then early_stop=, then posterior=, then ssim= (the order of a
        solo NativeIteration), all in front of Adam -- as (monitor, the prefix of its slab rows' names, the attribute of its
        descriptor, the attribute of its launches).  (The slab order differs in one place: the post_ rows lie behind
        everything else, _build_row0.)"""
        return [(getattr(self, slot), *rest) for slot, *rest in self._SLOTS if getattr(self, slot) is not None]

    @staticmethod
    def _check_monitor_slot(m, slot):
        """What holds for monitor=, early_stop=, posterior= and ssim= alike: the types the slot takes, and that a monitor is
        adopted once."""
        import utils.fit_monitor as FM
        if m is None:
            return None
        if slot == "posterior" and not isinstance(m, FM.GroupedPosteriorMonitor):
            raise TypeError(f"dip-amd: GroupedFits(posterior=) takes a utils.fit_monitor.GroupedPosteriorMonitor or None, got "
                            f"{type(m).__name__} (a solo PosteriorMonitor owns its buffers: they are no rows of the slab)")
        if slot == "ssim":
            if not isinstance(m, FM.GroupedSSIMMonitor):
                raise TypeError(f"dip-amd: GroupedFits(ssim=) takes a utils.fit_monitor.GroupedSSIMMonitor or None, got "
                                f"{type(m).__name__} (a solo SSIMMonitor owns its buffers: they are no rows of the slab)")
        elif slot == "early_stop":
            if not isinstance(m, FM.GroupedEarlyStopMonitor):
                raise TypeError(f"dip-amd: GroupedFits(early_stop=) takes a utils.fit_monitor.GroupedEarlyStopMonitor or None, got "
                                f"{type(m).__name__} (a solo EarlyStopMonitor owns its buffers: they are no rows of the slab)")
        elif slot == "monitor" and not isinstance(m, (FM.GroupedFitMonitor, FM.GroupedSRFitMonitor,
                                                      FM.GroupedRestorationFitMonitor)):
            raise TypeError(f"dip-amd: GroupedFits(monitor=) takes a utils.fit_monitor.GroupedFitMonitor, a GroupedSRFitMonitor, a "
                            f"GroupedRestorationFitMonitor or None, got {type(m).__name__} (a solo FitMonitor cannot "
                            "checkpoint a slab row)")
        if m._adopted:
            raise RuntimeError(f"dip-amd: this {type(m).__name__} already belongs to a GroupedFits (a monitor is adopted once)")
        return m

    @classmethod
    def _check_ssim(cls, ssim, B, monitor, exp_weight):
        """What can be said about `ssim` before anything is planned or allocated (the images' shape: _carve_monitor)."""
        from utils.fit_monitor import GroupedFitMonitor
        if ssim is None:
            return None
        cls._check_monitor_slot(ssim, "ssim")
        if len(ssim.imgs_gt) != B:
            raise ValueError(f"dip-amd: GroupedSSIMMonitor has {len(ssim.imgs_gt)} imgs_gt for {B} instances")
        if ssim.with_avg and not isinstance(monitor, GroupedFitMonitor):
            if exp_weight is not None:
                raise NotImplementedError("dip-amd: GroupedSSIMMonitor(with_avg=True) with exp_weight= is not implemented (that "
                                          "out_avg is no row of the slab and is updated behind Adam); use "
                                          "monitor=GroupedFitMonitor(...), which carries the moving average")
            raise ValueError("dip-amd: GroupedSSIMMonitor(with_avg=True) records the SSIM of the group's smoothed output: it "
                             "needs monitor=GroupedFitMonitor(...), which keeps out_avg")
        return ssim

    @classmethod
    def _check_posterior(cls, posterior, B, targets, downsamplers):
        """What can be said about `posterior` before anything is planned or allocated (a super-resolution group's HR shape:
        _carve_monitor)."""
        if posterior is None:
            return None
        cls._check_monitor_slot(posterior, "posterior")
        posterior._check_count(B)
        if downsamplers is None:                        # (the net output is shaped like the target)
            posterior._check_out(B, tuple(targets[0].shape))
        return posterior

    @classmethod
    def _check_monitor(cls, monitor, downsamplers, exp_weight, ema_init, targets, masks=None):
        """What can be said about `monitor` before anything is planned or allocated: the slot's checks, then the group kind
        its record belongs to."""
        from utils.fit_monitor import GroupedRestorationFitMonitor, GroupedSRFitMonitor
        if monitor is None:
            return None
        cls._check_monitor_slot(monitor, "monitor")
        sr, restore = isinstance(monitor, GroupedSRFitMonitor), isinstance(monitor, GroupedRestorationFitMonitor)
        if restore and downsamplers is not None:
            raise NotImplementedError("dip-amd: GroupedFits(monitor=GroupedRestorationFitMonitor) with downsamplers= is not "
                                      "implemented (the restoration closure has a mask and no down-sampler; the super-resolution "
                                      "closure's record is utils.fit_monitor.GroupedSRFitMonitor)")
        if restore and (masks is None or any(m is None for m in masks)):
            raise ValueError("dip-amd: a GroupedRestorationFitMonitor records psrn_masked of a masked group: it needs "
                             "GroupedFits(masks=[...]), one mask per instance (the denoising closure's monitor is "
                             "GroupedFitMonitor)")
        if downsamplers is not None and not sr:
            raise NotImplementedError("dip-amd: GroupedFits(monitor=GroupedFitMonitor) with downsamplers= is not implemented (the "
                                      "super-resolution closure records psnr_LR / psnr_HR on two sizes: another record, "
                                      "utils.fit_monitor.GroupedSRFitMonitor)")
        if sr and downsamplers is None:
            raise ValueError("dip-amd: a GroupedSRFitMonitor records out_LR and out_HR of a super-resolution group: it needs "
                             "GroupedFits(downsamplers=...) (the denoising closure's monitor is GroupedFitMonitor)")
        if exp_weight is not None or ema_init != "first":
            raise ValueError("dip-amd: GroupedFits: exp_weight= / ema_init= are not combined with monitor= (" +
                             ("the super-resolution closure has no moving average of the output)" if sr else
                              "the restoration closure has no moving average of the output)" if restore else
                              "the monitor carries exp_weight and starts out_avg from the first output)"))
        if sr:
            monitor._check_count(len(targets))          # (the shapes: when the net output is planned, _carve_monitor)
        elif not restore:                               # (the restoration monitor brings no images: target and mask are the group's)
            monitor._check_targets(targets)
        return monitor

    @staticmethod
    def _check_tv(tv_weights, tv_beta, B, downsamplers):
        """(the B weights or None = no TV term, tv_beta): the rule of SRHead(tv_weight=, tv_beta=), per instance."""
        from utils.loss_head import sr_check_tv
        if tv_weights is None:
            return None, float(tv_beta)
        if downsamplers is None:
            raise ValueError("dip-amd: GroupedFits: tv_weights= belongs to the super-resolution closure: it needs downsamplers=")
        ws = list(tv_weights) if isinstance(tv_weights, (list, tuple)) or hasattr(tv_weights, "__len__") else [tv_weights] * B
        if len(ws) != B:
            raise ValueError(f"GroupedFits: tv_weights is None, one float or one per instance: got {len(ws)} for {B} nets")
        beta = float(tv_beta)
        ws = [sr_check_tv(w, tv_beta, who="GroupedFits")[0] for w in ws]
        if all(w == 0 for w in ws):
            return None, beta
        if any(w == 0 for w in ws):
            raise ValueError(f"dip-amd: GroupedFits: tv_weights mixes zero and positive weights ({ws}): one launch list serves "
                             "either the TV tail or the plain one; fit the instances without TV in a group of their own")
        return ws, beta

    @staticmethod
    def _check_sgld(weight_decay, param_noise_std, param_noise_seeds, B, seeds):
        """(weight_decay, the B noise levels, the B seeds) of an SGLD group, or the ValueError that says what is wrong."""
        if not float(weight_decay) >= 0.0:                          # (a NaN compares false)
            raise ValueError(f"dip-amd: GroupedFits: weight_decay must be >= 0, got {weight_decay}")
        stds = list(param_noise_std) if isinstance(param_noise_std, (list, tuple)) or hasattr(param_noise_std, "__len__") \
            else [param_noise_std] * B
        if len(stds) != B:
            raise ValueError(f"GroupedFits: param_noise_std is one float or one per instance: got {len(stds)} for {B} nets")
        if any(not float(s) >= 0.0 for s in stds):
            raise ValueError(f"dip-amd: GroupedFits: param_noise_std must be >= 0, got {stds}")
        sd = list(seeds) if param_noise_seeds is None else [int(s) for s in param_noise_seeds]
        if len(sd) != B:
            raise ValueError(f"GroupedFits: param_noise_seeds holds one seed per instance: got {len(sd)} for {B} nets")
        return float(weight_decay), [float(s) for s in stds], [s & 0xFFFFFFFFFFFFFFFF for s in sd]

    @staticmethod
    def _check_sweep(x, what, B, setter=False):
        """lr / reg_noise_std as one float, or as B floats = per-instance rows of the slab; the ValueError that says what is
        wrong otherwise.  A list of noise levels that are all zero is the float 0; a construction list that mixes zero and
        positive levels is refused (setter: the rows exist, an instance may go to 0)."""
        import math
        import numbers
        ok = lambda v: isinstance(v, numbers.Real) and not isinstance(v, bool) and math.isfinite(v) and v >= 0
        seq = isinstance(x, (list, tuple)) or (hasattr(x, "__len__") and getattr(x, "ndim", 1) > 0
                                                and not isinstance(x, (str, bytes)))
        if not seq and not setter:
            return float(x)                       # (one value for all: a launch argument, taken as it always was)
        xs = list(x) if seq else [x] * B
        if len(xs) != B:
            raise ValueError(f"dip-amd: GroupedFits: {what} is one float or one per instance: got {len(xs)} for {B} nets")
        if not all(ok(v) for v in xs):
            raise ValueError(f"dip-amd: GroupedFits: {what} must hold finite numbers >= 0, got {xs!r}")
        xs = [float(v) for v in xs]
        if what == "reg_noise_std" and not setter:
            if all(v == 0 for v in xs):
                return 0.0
            if any(v == 0 for v in xs):
                raise ValueError(f"dip-amd: GroupedFits: reg_noise_std mixes zero and positive levels ({xs}): a solo fit at level 0 "
                                 "feeds net_input_saved itself, an instance at 0 on the noise path would differ from it where the "
                                 "input holds -0.0; fit the instances without noise in a group of their own (set_reg_noise_std "
                                 "may take an instance to 0 at run time)")
        return xs

    def set_lr(self, lr):
        """Other learning rates (B floats; one float serves all) for the iterations that follow: FusedAdam.set_lr per instance.
        The fp64 rows are rewritten in stream order; the launch list and a captured hipGraph stay as they are."""
        if not self._lr_rows:
            raise ValueError("dip-amd: GroupedFits.set_lr on a group whose lr is a launch argument: construct the group with a "
                             "list (lr=[lr] * B anneals a common value)")
        lrs = self._check_sweep(lr, "lr", self.B, setter=True)
        for b, v in enumerate(lrs):
            self._inst(self._row0_extra["lr"], b).fill_(v)
        self.lr = lrs

    def set_reg_noise_std(self, std):
        """Other input-noise levels (B floats; one float serves all) for the iterations that follow: RegNoise.set_std per
        instance, in stream order, without a re-plan or a re-capture.  An instance may go to 0: it then gets saved + 0 * N."""
        if not self._std_rows:
            raise ValueError("dip-amd: GroupedFits.set_reg_noise_std on a group whose level is a launch argument: construct the "
                             "group with a list (reg_noise_std=[std] * B anneals a common value)")
        stds = self._check_sweep(std, "reg_noise_std", self.B, setter=True)
        for b, v in enumerate(stds):
            self._inst(self._row0_extra["reg_std"], b).fill_(v)
        self.std = stds

    def _sgld_state(self, b):
        """Instance b's DipSgldState {offset 0, seed, std} as int64[3] on the host."""
        s = N.DipSgldState(0, self.param_noise_seeds[b], self.param_noise_std[b], 0.0)
        return torch.frombuffer(bytearray(bytes(s)), dtype=torch.int64)

    def set_param_noise_std(self, std):
        """Other noise levels (one float or B floats) for the iterations that follow: FusedAdam.set_noise_std per instance.
        The device floats are rewritten in stream order; the launch list and a captured hipGraph stay as they are."""
        if not self.sgld:
            raise ValueError("dip-amd: GroupedFits.set_param_noise_std on a group without SGLD: construct it with "
                             "param_noise_std= / weight_decay=")
        _, stds, _ = self._check_sgld(self.weight_decay, std, self.param_noise_seeds, self.B, self.seeds)
        for b, s in enumerate(stds):
            self._inst(self._row0_extra["sgld"], b).view(torch.float32)[4:5].fill_(s)
        self.param_noise_std = stds

    def param_noise_offsets(self):
        """The Philox offset of every instance's SGLD stream, as the device holds it."""
        return [int(self._inst(self._row0_extra["sgld"], b)[0].item()) & 0xFFFFFFFFFFFFFFFF for b in range(self.B)]

    def set_tv_weights(self, tv_weights):
        """Other positive weights for the iterations that follow (SRHead.set_tv_weight per instance): the device scalars are
        rewritten in stream order; the launch list and a captured hipGraph stay as they are."""
        if self.tv_weights is None:
            raise ValueError("dip-amd: GroupedFits.set_tv_weights on a group without a TV term: construct a new group")
        ws, _ = self._check_tv(tv_weights, self.tv_beta, self.B, self.downsamplers)
        if ws is None:
            raise ValueError("dip-amd: GroupedFits.set_tv_weights: switching the TV term off changes the launch list; construct "
                             "a new group")
        for b, w in enumerate(ws):
            self._inst(self._row0_extra["tv_weight"], b).fill_(w)
        self.tv_weights = ws

    @staticmethod
    def _check_downsamplers(downsamplers, B, masks):
        """What can be said about `downsamplers` before anything is planned or allocated (the rule of SRHead, per instance)."""
        from models.downsampler import Downsampler
        from utils.loss_head import sr_check_fixed_taps, sr_support
        downs = list(downsamplers)
        if len(downs) != B:
            raise ValueError(f"GroupedFits: one Downsampler per instance: got {len(downs)} for {B} nets")
        if masks is not None:
            raise ValueError("GroupedFits: masks and downsamplers exclude each other (the super-resolution loss has no mask)")
        for b, d in enumerate(downs):
            if not isinstance(d, Downsampler):
                raise TypeError(f"dip-amd: GroupedFits needs models.downsampler.Downsampler objects, instance {b} is a "
                                f"{type(d).__name__}")
            sr_check_fixed_taps(d, who="GroupedFits")
            if sr_support(d) != sr_support(downs[0]):
                raise ValueError(f"GroupedFits: the Downsampler of instance {b} has (k, factor, pad) = {sr_support(d)}, "
                                 f"instance 0 has {sr_support(downs[0])}: one launch list serves one filter support")
            if d.downsampler_.weight.shape[0] != downs[0].downsampler_.weight.shape[0]:
                raise ValueError(f"GroupedFits: the Downsampler of instance {b} differs from instance 0 in planes")
        return downs

    def pointers_outside_row0(self):
        """Self-check of the memory model: every device pointer of the launch list (descriptor fields and pointer
        arguments) must lie inside instance 0's slab -- the library refuses a grouped launch otherwise (rc -1).  Returns
        the offenders as (op name, field) pairs; [] when the list is sound."""
        lo, hi = self.mem.data_ptr(), self.mem.data_ptr() + self.stride
        bad = []

        def visit(name, field, v):
            if isinstance(v, C.Structure):
                for f, _ in v._fields_:
                    visit(name, field + "." + f, getattr(v, f))
            elif isinstance(v, int) and v >= (1 << 32) and not (lo <= v < hi):
                bad.append((name, field))

        eng = self.eng
        for ops in (eng.fwd_ops, eng.bwd_ops):
            for fn, args, name in ops:
                for k, a in enumerate(args):
                    visit(name, f"arg{k}", a._obj if hasattr(a, "_obj") else a)

        def pointer_args(ops):          # of launches whose descriptor is visited on its own (the head's: y_out, gl, dy_out)
            for fn, args, name in ops:
                for k, a in enumerate(args):
                    if not hasattr(a, "_obj"):
                        visit(name, f"arg{k}", a)

        visit("sr_loss" if self.downsamplers is not None else "loss_head", "desc", self._head)
        pointer_args(self._head_fwd + self._head_bwd)
        for _, prefix, desc, ops in self._monitors():
            visit({"mon_": "fit_monitor", "es_": "early_stop"}.get(prefix, prefix[:-1]), "desc", getattr(self, desc))
            pointer_args(getattr(self, ops))
        for k, t in self._row0_extra.items():
            if t is not None:
                visit("extra", k, t.data_ptr())
        for k in ("params", "grads", "packed", "pack_recs", "x_nhwc", "dy_out", "bnbuf", "nbt"):
            visit("engine", k, getattr(eng, k).data_ptr())
        if eng.bf3:
            visit("engine", "packed3", eng.packed3.data_ptr())
            visit("engine", "pack_recs3", eng.pack_recs3.data_ptr())
        return bad

    @staticmethod
    def _mask4(m):
        m = m.detach().float()
        while m.dim() < 4:
            m = m[None]
        return m.contiguous()

    def _build_row0(self, slab, Cimg, H, W, t0, m0):
        """Everything instance 0 owns, in a fixed order, from `slab`: the engine's buffers, the closure's input, the loss head's
        buffers -- those of utils.loss_head.MSEHead, or of SRHead -- with its descriptor and launches, the closure's end and,
        behind everything else, the monitors' buffers."""
        from utils import loss_head as LH
        eng, lib, sr, tv = self.eng, self.lib, self.downsamplers is not None, self.tv_weights is not None
        eng.slab = slab
        eng._build_arenas(self.device)
        if Cimg != eng.sc[0].down_a.Cin:
            raise RuntimeError(f"dip-amd: input has {Cimg} channels, net expects {eng.sc[0].down_a.Cin}")
        eng._build_plan(H, W, Cimg)
        Cn, Hn, Wn = eng.n_out, eng.Hout, eng.Wout
        if sr:
            geom = k, f, pad, Ho, Wo = LH.sr_geometry(self.downsamplers[0], Hn, Wn, who="GroupedFits")
            if (Ho, Wo) != tuple(t0.shape[2:]):
                raise ValueError(f"GroupedFits: targets (the LR images) are {tuple(t0.shape[2:])}, the down-sampled net output is "
                                 f"{(Ho, Wo)} (net output {(Hn, Wn)}, k {k}, factor {f}, pad {pad})")
        elif (Hn, Wn) != tuple(t0.shape[2:]):
            raise ValueError(f"GroupedFits: targets are {tuple(t0.shape[2:])}, the net output is {(Hn, Wn)}")
        nin, nout = Cimg * H * W, Cn * Hn * Wn
        ex = {}
        ex["saved"] = slab.alloc(nin)                       # net_input_saved (denoising.ipynb:198)
        ex["noisy"] = slab.alloc(nin) if self._noisy else None
        ex["rng"] = slab.alloc(2, torch.int64, zero=True)   # {Philox offset, seed} (dip_noise_axpy_dev2)
        if sr:
            ex["taps"] = slab.alloc(k * k)                  # per-instance data: every pointer of a grouped launch is in the slab
            ex["target"] = slab.alloc(Cn * Ho * Wo)         # img_LR
            ex["mask"] = None
            ex["out"] = slab.alloc(nout)                    # out_HR, NCHW
            ex["y"] = slab.alloc(Cn * Ho * Wo)              # out_LR
            self.nblk = lib.dip_sr_loss_nblk(Cn, Ho, Wo)
            ex["partials"] = slab.alloc(self.nblk)
            if tv:                                          # two more per-instance rows: the weight and the TV partials
                self.tv_nblk = lib.dip_sr_tv_nblk(Cn, Hn, Wn)
                ex["tv_weight"] = slab.alloc(1)
                ex["tv_partials"] = slab.alloc(self.tv_nblk)
        else:
            ex["target"] = slab.alloc(nout)
            ex["mask"] = slab.alloc(self.mask_c * Hn * Wn) if m0 is not None else None
            ex["out"] = slab.alloc(nout)
            self.nblk = lib.dip_loss_head_nblk(Hn * Wn, eng.out_conv.Cin)
            ex["partials"] = slab.alloc(self.nblk)
        ex["loss"] = slab.alloc(1, zero=True)
        ex["gl"] = slab.alloc(1)                            # d(total_loss)/d(total_loss) = 1 (total_loss.backward())
        ex["gl"].fill_(1.0)
        ex["m"] = slab.alloc(eng.n_arena, zero=True)        # Adam moments over the parameter arena
        ex["v"] = slab.alloc(eng.n_arena, zero=True)
        ex["iter"] = slab.alloc(16, torch.uint8, zero=True)  # DipIterState: step count, step size, sqrt(bias correction 2)
        self._row0_extra = ex
        self._x = ex["noisy"] if self._noisy else ex["saved"]
        at = lambda k: None if ex[k] is None else ex[k].data_ptr()
        if sr:
            self._head = LH.sr_descriptor(eng, geom, at("out"), at("taps"), at("target"), at("y"), at("partials"), self.nblk,
                                          at("loss"))
            if tv:
                self._head = LH.sr_tv_descriptor(self._head, at("tv_weight"), at("tv_partials"), self.tv_nblk, self.tv_beta)
            fwd, bwd = LH.sr_fwd_launches, LH.sr_bwd_launches
        else:
            self._head, self._tr = LH.mse_descriptor(eng, at("target"), at("mask"), self.mask_c, at("out"), at("partials"),
                                                     self.nblk, at("loss"))
            fwd, bwd = LH.mse_fwd_launches, LH.mse_bwd_launches
        # (MSE tail: dip_loss_head_fwd runs the output conv itself; super-resolution: the forward list runs to its end and
        # dip_head_fwd writes out_HR as net(x) does)
        self._with_out_conv = sr
        self._head_fwd, self._head_bwd = fwd(eng, self._head), bwd(eng, self._head, at("gl"))
        for m, prefix, desc, ops in self._monitors():
            if prefix != "post_":                           # (the posterior's rows: behind everything else, below)
                d, launches = self._carve_monitor(slab, m, prefix)
                setattr(self, desc, d)
                setattr(self, ops, launches)
        if self.sgld:
            # behind everything else: the DipSgldState and the range table of the 4-D parameters (dip_optim.noise_ranges: what
            # a solo FusedAdam over the net's parameters noises), and the extent a solo FusedAdam group steps
            import dip_optim
            plist = eng.param_list
            self._sgld_ranges = dip_optim.noise_ranges(plist, eng.slots, [p for p in plist if p.dim() == 4])
            if len(self._sgld_ranges) > dip_optim.SGLD_MAX_RANGES:
                raise RuntimeError(f"dip-amd: GroupedFits: {len(self._sgld_ranges)} noised ranges; dip_adam_sgld_step_dev takes at "
                                   f"most {dip_optim.SGLD_MAX_RANGES}")
            self._sgld_n = eng.slots[-1] + plist[-1].numel()
            ex["sgld"] = slab.alloc(3, torch.int64, zero=True)
            ex["sgld_ranges"] = slab.alloc(max(2 * len(self._sgld_ranges), 1), torch.int64, zero=True)
            ex["sgld"].copy_(self._sgld_state(0))
            if self._sgld_ranges:
                ex["sgld_ranges"][:2 * len(self._sgld_ranges)].copy_(
                    torch.tensor(self._sgld_ranges, dtype=torch.int64).reshape(-1))
        # a sweep's scalars, only when the keyword is a list and behind everything else: no other row's offset moves
        if self._lr_rows:
            ex["lr"] = slab.alloc(1, torch.float64)             # dip_adam_tick_dev reads it
            ex["lr"].fill_(self.lr[0])
        if self._std_rows:
            ex["reg_std"] = slab.alloc(1)                       # dip_noise_axpy_dev3 reads it
            ex["reg_std"].fill_(self.std[0])
        # the posterior's rows, only when the keyword is set and behind everything else, the sweep rows included
        if self.posterior is not None:
            self._pdesc, self._post = self._carve_monitor(slab, self.posterior, "post_")

    def _monitor_sizes(self, m):
        from utils.fit_monitor import monitor_sizes
        eng, ex = self.eng, self._row0_extra
        return monitor_sizes(m, self.lib.dip_fit_monitor_nblk, ex["out"].numel(), (eng.n_out, eng.Hout, eng.Wout), (),
                             n_lr=None if ex.get("y") is None else ex["y"].numel(), n_arena=eng.n_arena)

    def _carve_monitor(self, slab, m, prefix):
        """The buffers of monitor m (of any of the four slots) behind everything instance 0 owns so far: what the solo monitor of
        its kind allocates for one fit -- its table, utils.fit_monitor -- as per-instance data of the slab under the names
        prefix + key (None where m has no such buffer); ONE descriptor over them (the outputs = the head's, noisy / img / img_LR
        = the target, mask = the group's, loss = the slab's loss scalar: nothing is rewritten per iteration) and the launches
        of an iteration.  Both passes initialise the buffers, so the row copy carries them to every instance."""
        from utils import fit_monitor as FM
        eng, ex = self.eng, self._row0_extra
        if self.downsamplers is not None and prefix == "mon_":
            m._check_hr(self.B, (1, eng.n_out, eng.Hout, eng.Wout))
        if prefix in ("ssim_", "post_"):
            m._check_out(self.B, (1, eng.n_out, eng.Hout, eng.Wout))
        z = self._monitor_sizes(m)
        t = dict(out=ex["out"], out_LR=ex.get("y"), noisy=ex["target"], img=ex["target"], img_LR=ex["target"], mask=ex["mask"],
                 mask_c=self.mask_c, hw=eng.Hout * eng.Wout, loss=ex["loss"], avg=ex.get("mon_avg"))
        for b in m.BUFFERS:
            buf = None
            if b.when(m):
                buf = slab.alloc(b.count(z), b.dtype, zero=b.init == "zero")
                if b.init == "early_stop":
                    FM.early_stop_state_fill(buf)
            t[b.name] = ex[prefix + (b.key or b.name)] = buf
        desc = m._descriptor(t)
        arena = t[m.ARENA[0]] if m.ARENA else None
        return desc, FM.monitor_launches(self.lib, desc, eng.params.data_ptr(), eng.n_arena,
                                         None if arena is None else arena.data_ptr())

    def _off(self, t0):
        o = t0.data_ptr() - self.mem.data_ptr()
        assert 0 <= o and o + t0.numel() * t0.element_size() <= self.stride, "tensor is not in row 0 of the slab"
        return o

    def _inst(self, t0, b):
        """The buffer of instance b that corresponds to t0 (a flat tensor in row 0)."""
        o = self._off(t0) + b * self.stride
        return self.mem[o:o + t0.numel() * t0.element_size()].view(t0.dtype)

    def _strided(self, t0, *shape):
        """[B, *shape] view over the instances of t0 (row 0; None: no such buffer), without a copy."""
        if t0 is None:
            return None
        es = t0.element_size()
        assert self.stride % es == 0
        flat = self.mem.view(t0.dtype)
        inner = [1] * len(shape)
        for d in range(len(shape) - 2, -1, -1):
            inner[d] = inner[d + 1] * shape[d + 1]
        # (as_strided's offset counts from the start of the STORAGE, not of `flat`)
        return torch.as_strided(flat, (self.B,) + tuple(shape), [self.stride // es] + inner,
                                flat.storage_offset() + self._off(t0) // es)

    def _adopt_net(self, b):
        """Parameters and BatchNorm buffers of nets[b] move into row b (same offsets as instance 0) and become views of it,
        like SkipEngine._build_arenas does for a solo net: state_dict() / load_state_dict() / .data.copy_() keep working."""
        eng = self.eng
        net = self.nets[b]
        prow = self._inst(eng.params, b)
        for p, o in zip(net.parameters(), eng.slots):
            n = p.numel()
            prow[o:o + n].copy_(p.detach().reshape(-1).to(device=self.device, dtype=torch.float32))
            p.data = prow[o:o + n].view(p.shape)
            p.grad = None
        bnrow, nbtrow = self._inst(eng.bnbuf, b), self._inst(eng.nbt, b)
        bn_mods = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
        by_name = dict(net.named_modules())
        names0 = {id(m): k for k, m in self.nets[0].named_modules()}
        for k, rec in enumerate(eng.bns):
            m = by_name[names0[id(rec.module)]]                 # the same BatchNorm in nets[b]
            if rec.rm_off >= 0:
                bnrow[rec.rm_off:rec.rm_off + rec.C].copy_(m.running_mean.to(self.device))
                bnrow[rec.rv_off:rec.rv_off + rec.C].copy_(m.running_var.to(self.device))
                nbtrow[k] = m.num_batches_tracked.to(self.device)
                m._buffers["running_mean"] = bnrow[rec.rm_off:rec.rm_off + rec.C]
                m._buffers["running_var"] = bnrow[rec.rv_off:rec.rv_off + rec.C]
                m._buffers["num_batches_tracked"] = nbtrow[k]
        assert len(bn_mods) == len(eng.bns)

    # ------------------------------------------------------------------ one iteration
    def _iteration(self):
        """optimizer.zero_grad(); closure(); optimizer.step() for all B instances: ONE launch list."""
        eng, lib, ex = self.eng, self.lib, self._row0_extra
        dev = self.device
        main = torch.cuda.current_stream(dev)
        st = main.cuda_stream
        N.check(lib.dip_group_begin(self.B, self.stride, self.mem.data_ptr(), self.stride), "group_begin")
        try:
            # closure: net_input = net_input_saved + noise.normal_() * reg_noise_std
            if self._std_rows:              # a sweep: every instance reads the level of its own row
                N.check(lib.dip_noise_axpy_dev3(ex["saved"].data_ptr(), ex["noisy"].data_ptr(), ex["saved"].numel(),
                                                ex["reg_std"].data_ptr(), ex["rng"].data_ptr(), st), "noise_axpy_dev3")
            elif self._noisy:
                N.check(lib.dip_noise_axpy_dev2(ex["saved"].data_ptr(), ex["noisy"].data_ptr(), ex["saved"].numel(), self.std,
                                                ex["rng"].data_ptr(), st), "noise_axpy_dev2")
            # out = net(net_input); total_loss = mse(out [* mask], target [* mask])
            # (super-resolution: out_LR = downsampler(out); total_loss = mse(out_LR, img_LR))
            eng._launch_forward(self._x.data_ptr(), main, with_out_conv=self._with_out_conv)
            for fn, args, name in self._head_fwd:
                N.check(fn(*args, st), name)
            # total_loss.backward()
            for fn, args, name in self._head_bwd:
                N.check(fn(*args, st), name)
            eng._launch_backward(main)
            # monitor.update(out, total_loss): EMA, PSNRs, record; a fall-back overwrites the parameters after this
            # iteration's gradients and before Adam (denoising.ipynb:238-248), per instance
            # (super-resolution: monitor.update(out_HR, out_LR, total_loss): the psnr_LR / psnr_HR record)
            # es.update(out): behind the monitor (a fall-back has been applied), in front of Adam -- best_params are the
            # parameters that produced best_out; every instance takes its own decision
            # pm.update(out): the sample is the output of the parameters that are about to be stepped and perturbed
            # ssim.update(out): behind the monitor (its out_avg is this iteration's)
            for _, _, _, ops in self._monitors():
                for fn, args, name in getattr(self, ops):
                    N.check(fn(*args, st), name)
            # optimizer.step(): torch.optim.Adam semantics (dip_optim.FusedAdam), step count on the device
            if self._lr_rows:
                N.check(lib.dip_adam_tick_dev(ex["iter"].data_ptr(), ex["lr"].data_ptr(), self.ADAM_BETAS[0], self.ADAM_BETAS[1],
                                              st), "adam_tick_dev")
            else:
                N.check(lib.dip_adam_tick(ex["iter"].data_ptr(), self.lr, self.ADAM_BETAS[0], self.ADAM_BETAS[1], st),
                        "adam_tick")
            if self.sgld:                   # FusedAdam(weight_decay=, noise_std=, noise_seed=) per instance, ONE launch
                N.check(lib.dip_adam_sgld_step_dev(eng.params.data_ptr(), eng.grads.data_ptr(), ex["m"].data_ptr(),
                                                   ex["v"].data_ptr(), self._sgld_n, self.ADAM_BETAS[0], self.ADAM_BETAS[1],
                                                   self.ADAM_EPS, self.weight_decay, ex["iter"].data_ptr(),
                                                   ex["sgld"].data_ptr(), ex["sgld_ranges"].data_ptr(),
                                                   len(self._sgld_ranges), st), "adam_sgld_step_dev")
            else:
                N.check(lib.dip_adam_step_dev(eng.params.data_ptr(), eng.grads.data_ptr(), ex["m"].data_ptr(),
                                              ex["v"].data_ptr(), eng.n_arena, self.ADAM_BETAS[0], self.ADAM_BETAS[1],
                                              self.ADAM_EPS, ex["iter"].data_ptr(), st), "adam_step_dev")
        finally:
            lib.dip_group_end()
        # ATen, batched over the instances: BatchNorm's num_batches_tracked and the closure's out_avg
        if len(eng.bns):
            self._nbt_all.add_(1)
        if self.out_avg is not None and self.monitor is None:
            if self.iterations == 0 and self.ema_first and not torch.cuda.is_current_stream_capturing():
                self.out_avg.copy_(self.out)
            else:
                self.out_avg.mul_(self.exp_weight).add_(self.out, alpha=1 - self.exp_weight)

    def _check_room(self, n):
        """The monitors refuse n more iterations that do not fit their records, before anything is issued."""
        for m, *_ in self._monitors():
            m._check_room(n)

    def _issued(self, n):
        self.iterations += n
        for m, *_ in self._monitors():
            m.i += n

    def step(self, n=1):
        """n eager iterations (launches on the current stream + the engine's auxiliary streams)."""
        self._check_room(n)
        if self._dry:
            raise RuntimeError("dip-amd: a dry (host-memory) GroupedFits cannot launch anything")
        with torch.cuda.device(self.device):
            for _ in range(int(n)):
                self._iteration()
                self._issued(1)

    def capture(self, warmup=3):
        """`warmup` eager iterations (at least one), then the grouped iteration as ONE hipGraph (replayed by run()).  With a
        monitor the warm-up iterations are recorded like any other: they count towards monitor.i and its capacity."""
        dev = self.device
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            self.capture_stream = torch.cuda.Stream(dev)
            self.capture_stream.wait_stream(cur)
            with torch.cuda.stream(self.capture_stream):
                self.step(max(int(warmup), 1))
            cur.wait_stream(self.capture_stream)
            torch.cuda.synchronize(dev)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=self.capture_stream):
                self._iteration()
        return self

    def run(self, n=1):
        if self.graph is None:
            return self.step(n)
        self._check_room(n)
        for _ in range(int(n)):
            self.graph.replay()
        self._issued(int(n))

    def run_until(self, max_iter, check_every=50):
        """Runs until every instance's early stopping says stop, or max_iter: issues run(check_every) batches, eager or
        replayed, and reads the B `stopped` words after each batch (one copy and one synchronisation per batch).  Returns the
        iterations issued.  A stopped instance keeps training until the last one stops -- a row cannot leave the launch list --
        but its best_out / best_params are frozen (early_stop.restore_best() puts the minima back)."""
        es = self.early_stop
        if es is None:
            raise RuntimeError("dip-amd: GroupedFits.run_until needs early_stop=GroupedEarlyStopMonitor(...)")
        max_iter, check_every = max(int(max_iter), 0), int(check_every)
        if check_every < 1:
            raise ValueError(f"dip-amd: run_until: check_every must be >= 1, got {check_every}")
        self._check_room(max_iter)                # (before anything is issued, as run(max_iter) would)
        issued = 0
        while issued < max_iter:
            n = min(check_every, max_iter - issued)
            self.run(n)
            issued += n
            if all(es.stopped):
                break
        return issued

    def step_counts(self):
        """Adam's step count of every instance, as the device holds it."""
        return [int(self._inst(self._row0_extra["iter"], b).view(torch.int64)[0].item()) for b in range(self.B)]
