"""Fused Adam over flat arenas (libdip_hip.so: dip_adam_step).

Replaces `torch.optim.Adam(parameters, lr=LR)` of the reference's optimize()
(utils/common_utils.py:225) with torch 2.x Adam semantics (betas (0.9, 0.999), eps 1e-8, no
weight decay; bias corrections computed in double on the host).  Parameters that are views of
one contiguous fp32 CUDA arena (a SkipNet's parameters) are stepped by ONE launch; any other
CUDA fp32 tensor (net_input for opt_over='net,input', Downsampler weights) gets its own launch
of the same kernel.

The step count lives in device memory (DipIterState, advanced by dip_adam_tick), so `step()` is a
static launch sequence: `GraphedIteration` captures {zero_grad(); closure(); step()} into one
hipGraph and replays it.  Several independent fits: `GraphedIteration.group(dip_group.GroupedFits(...))`
captures ONE launch list that serves all of them (every kernel launch covers all instances), and
`GraphedIteration.group([(optimizer, closure), ...])` -- arbitrary closures -- one graph per fit on its own stream.

`NativeIteration` is the eager form without autograd: head (utils.loss_head.MSEHead or SRHead), reg-noise (utils.reg_noise.RegNoise) and
optimiser known statically, the whole iteration -- noise, forward list, loss head, backward list, Adam -- is ONE call into
the library (dip_iter_run), bit-identical to {zero_grad(); closure(); step()} and interchangeable with it at any iteration.
With monitor=utils.fit_monitor.FitMonitor(...) the same call also does the closure's bookkeeping (EMA, PSNRs, back-tracking);
with an SRHead and monitor=utils.fit_monitor.SRFitMonitor(...) the super-resolution closure's (psnr_LR / psnr_HR).
"""
from __future__ import annotations

import os

import torch

import dip_native as N


class _Group:
    """A maximal run of parameters that is contiguous in device memory."""

    def __init__(self, params):
        self.params = params
        self.base = params[0].data_ptr()
        last = params[-1]
        self.numel = (last.data_ptr() - self.base) // 4 + last.numel()
        dev = params[0].device
        self.m = torch.zeros(self.numel, dtype=torch.float32, device=dev)
        self.v = torch.zeros(self.numel, dtype=torch.float32, device=dev)
        self.gbuf = None
        self.offsets = [(p.data_ptr() - self.base) // 4 for p in params]


def _split_contiguous(params, max_gap=4):
    groups, run = [], []
    for p in params:
        if run:
            prev = run[-1]
            gap = (p.data_ptr() - (prev.data_ptr() + 4 * prev.numel())) // 4
            same = p.device == prev.device and p.untyped_storage().data_ptr() == prev.untyped_storage().data_ptr()
            if not (same and 0 <= gap < max_gap and (p.data_ptr() - prev.data_ptr()) % 4 == 0):
                groups.append(run)
                run = []
        run.append(p)
    if run:
        groups.append(run)
    return groups


def noise_ranges(params, offsets, noised):
    """The range table of a contiguous group: the [begin, end) extents, in elements from the group's base, of the parameters
    that are in `noised` (by identity), merged where adjacent.  Sorted and disjoint; an alignment gap is never inside one."""
    ids = {id(p) for p in noised}
    out = []
    for p, o in zip(params, offsets):
        if id(p) not in ids:
            continue
        if out and out[-1][1] == o:
            out[-1][1] = o + p.numel()
        else:
            out.append([o, o + p.numel()])
    return [tuple(r) for r in out]


SGLD_MAX_RANGES = 512                          # (the LDS table of adam_sgld_kernel, csrc/misc_kernels.hip)


class FusedAdam:
    """torch.optim.Adam over flat arenas (module docstring), and with weight_decay / noise_std the SGLD sampler of Cheng et
    al., "A Bayesian Perspective on the Deep Image Prior" (CVPR 2019) in the same launch (dip_adam_sgld_step_dev):

        weight_decay   torch.optim.Adam's: g <- g + weight_decay * p in front of the moments (the Gaussian prior)
        noise_std      after the step, p <- p + noise_std * N(0, 1) on the noised parameters; set_noise_std(x) changes it
                       between steps without a re-plan (one 4-byte write on the current stream)
        noise_seed     the seed of the Philox stream (key noise_seed ^ 0x53474C4453474C44: a RegNoise of the same seed draws
                       other normals); contiguous group j of the list starts at offset j << 48
        noise_params   None: every parameter of the list with dim() == 4 -- the convolution weights, what the paper's code
                       perturbs.  Otherwise an iterable of parameters of the list (by identity).  With get_params('net,input',
                       ...) the net input is 4-D too: pass the explicit list then.

    With weight_decay == 0 and noise_std == 0 at construction the optimiser issues what it always issued (dip_adam_tick +
    dip_adam_step_dev); otherwise dip_adam_tick + dip_adam_sgld_step_dev, also after set_noise_std(0): the stream keeps
    advancing.  Everything that varies per step is in device memory, so GraphedIteration captures the step as it is.

    device_lr=True: lr, too, lives in device memory -- one fp64 scalar per device next to the DipIterState -- and the tick reads it
    there (dip_adam_tick_dev, the arithmetic of dip_adam_tick).  set_lr(x) rewrites it in stream order: a learning-rate schedule
    under a captured GraphedIteration, and no re-plan of a NativeIteration.  `lr` is the host mirror."""

    def __init__(self, parameters, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, noise_std=0.0, noise_seed=0,
                 noise_params=None, device_lr=False):
        self.params = [p for p in parameters]
        self.device_lr = bool(device_lr)
        if self.device_lr:
            lr = self._check_lr(lr, "FusedAdam")
        self.lr, self.betas, self.eps = lr, betas, eps
        self._lr_dev = {}                      # device -> the fp64 scalar dip_adam_tick_dev reads (device_lr only)
        if not float(weight_decay) >= 0.0:                          # (a NaN compares false)
            raise ValueError(f"dip-amd: FusedAdam: weight_decay must be >= 0, got {weight_decay}")
        if not float(noise_std) >= 0.0:
            raise ValueError(f"dip-amd: FusedAdam: noise_std must be >= 0, got {noise_std}")
        self.weight_decay, self.noise_std = float(weight_decay), float(noise_std)
        self.noise_seed = int(noise_seed) & 0xFFFFFFFFFFFFFFFF
        self.sgld = self.weight_decay != 0.0 or self.noise_std != 0.0      # which entry point step() issues: fixed here
        if noise_params is None:
            self.noise_params = [p for p in self.params if p.dim() == 4]
        else:
            self.noise_params = list(noise_params)
            mine = {id(p) for p in self.params}
            if any(id(p) not in mine for p in self.noise_params):
                raise ValueError("dip-amd: FusedAdam: noise_params holds a parameter that is not in the optimiser's list")
        self.step_count = 0
        self._groups = None
        self._sig = None
        self._iter_state = {}                  # device -> DipIterState bytes (uint8[16])

    @staticmethod
    def _check_lr(lr, who):
        import math
        import numbers
        if isinstance(lr, bool) or not isinstance(lr, numbers.Real) or not math.isfinite(lr) or lr < 0:
            raise ValueError(f"dip-amd: {who}: lr must be a finite number >= 0, got {lr!r}")
        return float(lr)

    def set_lr(self, lr):
        """The learning rate from the next step on: one 8-byte fill per device on the current stream, no synchronisation.
        Neither a NativeIteration plan nor a captured GraphedIteration holds the value."""
        if not self.device_lr:
            raise RuntimeError("dip-amd: FusedAdam.set_lr: this optimiser passes lr as a launch argument (a plan or a captured "
                               "graph would keep the old value); construct it with device_lr=True")
        self.lr = self._check_lr(lr, "FusedAdam.set_lr")
        for t in self._lr_dev.values():
            t.fill_(self.lr)

    def _lr_scalar(self, dev):
        """The fp64 lr scalar of device `dev` (device_lr only), created holding the host mirror."""
        t = self._lr_dev.get(dev)
        if t is None:
            t = self._lr_dev[dev] = torch.full((1,), float(self.lr), dtype=torch.float64, device=dev)
        return t

    def _tick_launch(self, lib, dev, st):
        """(fn, args without the stream, name) of the tick: what step() issues and NativeIteration's Adam phase starts with."""
        b1, b2 = float(self.betas[0]), float(self.betas[1])
        if self.device_lr:
            return lib.dip_adam_tick_dev, (st.data_ptr(), self._lr_scalar(dev).data_ptr(), b1, b2), "adam_tick_dev"
        return lib.dip_adam_tick, (st.data_ptr(), float(self.lr), b1, b2), "adam_tick"

    def set_noise_std(self, std):
        """The noise level from the next step on: written into every group's DipSgldState on the current stream.  No re-plan
        (NativeIteration keeps its command arrays), so it can be annealed between run() calls."""
        if not float(std) >= 0.0:
            raise ValueError(f"dip-amd: FusedAdam.set_noise_std: noise_std must be >= 0, got {std}")
        if not self.sgld:
            raise RuntimeError("dip-amd: FusedAdam.set_noise_std: this optimiser was constructed without weight_decay / noise_std "
                               "and issues the plain Adam entry point; construct it with noise_std > 0")
        self.noise_std = float(std)
        for g in self._groups or ():
            g.sgld.view(torch.float32)[4:5].fill_(self.noise_std)

    def _init_sgld(self, g, j, old):
        """Group j's DipSgldState {offset = j << 48, seed, std} and range table in device memory (`old`: the state of the group
        that started at the same parameter before the parameters moved -- the stream goes on where it was)."""
        dev = g.params[0].device
        g.ranges = noise_ranges(g.params, g.offsets, self.noise_params)
        if len(g.ranges) > SGLD_MAX_RANGES:
            raise RuntimeError(f"dip-amd: FusedAdam: {len(g.ranges)} noised ranges in one contiguous group; "
                               f"dip_adam_sgld_step_dev takes at most {SGLD_MAX_RANGES}")
        if old is not None:
            g.sgld = old.to(dev)
        else:
            s = N.DipSgldState((j << 48) & 0xFFFFFFFFFFFFFFFF, self.noise_seed, self.noise_std, 0.0)
            g.sgld = torch.frombuffer(bytearray(bytes(s)), dtype=torch.int64).to(dev)        # int64[3]: 8-byte aligned
        g.sgld.view(torch.float32)[4:5].fill_(self.noise_std)
        g.range_table = torch.tensor(g.ranges, dtype=torch.int64).reshape(-1, 2).to(dev) if g.ranges else None

    def device_noise_offset(self, j=0):
        """The Philox offset of contiguous group j as the device holds it (synchronises)."""
        return int(self._groups[j].sgld[0].item()) & 0xFFFFFFFFFFFFFFFF

    # torch.optim API subset used by optimize() and the notebooks
    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:                  # torch.optim.Optimizer.zero_grad: views cannot be detached in place
                    if p.grad.grad_fn is not None:
                        p.grad = p.grad.detach()
                    else:
                        p.grad.requires_grad_(False)
                    p.grad.zero_()

    def _signature(self):
        return tuple(p.data_ptr() for p in self.params)

    def _prepare(self):
        for p in self.params:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("dip-amd FusedAdam: parameters must be contiguous fp32 CUDA tensors "
                                   f"(got {p.dtype} on {p.device}); this backend has no CPU optimiser path")
        old, old_sgld = {}, {}
        if self._groups is not None:          # parameters moved (net re-typed): carry the moments over
            for g in self._groups:
                for p, o in zip(g.params, g.offsets):
                    old[id(p)] = (g.m[o:o + p.numel()].clone(), g.v[o:o + p.numel()].clone())
                if self.sgld:
                    old_sgld[id(g.params[0])] = g.sgld
        self._groups = [_Group(run) for run in _split_contiguous(self.params)]
        for j, g in enumerate(self._groups):
            for p, o in zip(g.params, g.offsets):
                if id(p) in old:
                    g.m[o:o + p.numel()].copy_(old[id(p)][0])
                    g.v[o:o + p.numel()].copy_(old[id(p)][1])
            if self.sgld:
                self._init_sgld(g, j, old_sgld.get(id(g.params[0])))
        self._sig = self._signature()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._sig != self._signature():
            self._prepare()
        lib = N.lib()
        self.step_count += 1
        active = []
        for g in self._groups:
            grads = [p.grad for p in g.params]
            if all(gr is None for gr in grads):
                continue
            # fast path: the gradients are views of one arena with the parameters' layout
            g0 = grads[0]
            flat_ptr = None
            if g0 is not None and g0.is_cuda and g0.dtype == torch.float32:
                base = g0.data_ptr() - 4 * g.offsets[0]
                if all(gr is not None and gr.dtype == torch.float32 and gr.is_contiguous()
                       and gr.data_ptr() == base + 4 * o for gr, o in zip(grads, g.offsets)):
                    flat_ptr = base
            if flat_ptr is None:
                if g.gbuf is None:
                    g.gbuf = torch.zeros(g.numel, dtype=torch.float32, device=g.params[0].device)
                for p, gr, o in zip(g.params, grads, g.offsets):
                    if gr is None:
                        # torch skips params without grad; a zero gradient would still decay the moments, so
                        # step such params separately is required -- not supported in a fused run
                        raise RuntimeError("dip-amd FusedAdam: a parameter of a fused group has no gradient")
                    g.gbuf[o:o + p.numel()].copy_(gr.reshape(-1))
                flat_ptr = g.gbuf.data_ptr()
            active.append((g, flat_ptr))
        ticked = set()
        for g, flat_ptr in active:
            dev = g.params[0].device
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                st = self._state(dev, self.step_count - 1)
                if dev not in ticked:          # t <- t + 1, step_size and sqrt(bc2) in double, on the device
                    fn, args, name = self._tick_launch(lib, dev, st)
                    N.check(fn(*args, stream), name)
                    ticked.add(dev)
                fn, args, name = self._step_launch(lib, g, flat_ptr, st)
                N.check(fn(*args, stream), name)
        return loss

    def _step_launch(self, lib, g, grad_ptr, st):
        """(fn, args without the stream, name) of group g's update: what step() issues and NativeIteration's Adam phase holds."""
        b1, b2, eps = float(self.betas[0]), float(self.betas[1]), float(self.eps)
        if not self.sgld:
            return (lib.dip_adam_step_dev, (g.base, grad_ptr, g.m.data_ptr(), g.v.data_ptr(), g.numel, b1, b2, eps,
                                            st.data_ptr()), "adam_step_dev")
        return (lib.dip_adam_sgld_step_dev, (g.base, grad_ptr, g.m.data_ptr(), g.v.data_ptr(), g.numel, b1, b2, eps,
                                             self.weight_decay, st.data_ptr(), g.sgld.data_ptr(),
                                             None if g.range_table is None else g.range_table.data_ptr(), len(g.ranges)),
                "adam_sgld_step_dev")

    def _plan_key(self):
        """What NativeIteration's Adam phase was built from; with the defaults, what it always was.  device_lr: the identity of
        the table of lr scalars stands where the value of lr stands (set_lr changes neither the table nor its tensors)."""
        key = (("lr_dev", id(self._lr_dev)) if self.device_lr else self.lr, self.betas, self.eps, id(self._groups))
        if self.sgld:
            key += (self.weight_decay, tuple((id(g.sgld), id(g.range_table), tuple(g.ranges)) for g in self._groups or ()))
        return key

    def _state(self, dev, step):
        """The DipIterState of device `dev`; created holding `step` (the count before the step about to be taken)."""
        st = self._iter_state.get(dev)
        if st is None:
            st = self._iter_state[dev] = torch.zeros(16, dtype=torch.uint8, device=dev)
            st.view(torch.int64)[0] = step
        return st

    def device_step_count(self):
        """Adam's step count as the device holds it (after graph replays the host count is stale)."""
        counts = [int(st.view(torch.int64)[0].item()) for st in self._iter_state.values()]
        return max(counts) if counts else self.step_count


_LIVE_GRAPHS = []


class GraphedIteration:
    """One optimisation iteration -- optimizer.zero_grad(); closure(); optimizer.step(), i.e. the body
    of the reference's optimize() loop (utils/common_utils.py:226-230) -- captured ONCE into a
    hipGraph and replayed: ~300 kernel launches, the event fork/joins of the two-stream schedule and
    the ATen ops of the closure become a single graph launch per iteration.

    The closure must be replay-safe: no host synchronisation (.item(), .cpu(), print of a tensor),
    every tensor it keeps across iterations updated IN PLACE, reg-noise from utils.reg_noise.RegNoise
    (or torch's graph-safe device generator).  `lr` is frozen at capture time unless `device_lr=True`
    (FusedAdam(..., device_lr=True): opt.set_lr(x) between run() calls; RegNoise(..., device_std=True) likewise).

        it = GraphedIteration(optimizer, closure)     # 3 eager warm-up iterations, then the capture
        it.run(num_iter - 3)
    """

    def __init__(self, optimizer, closure, warmup=3, device=None):
        self.fits = [(optimizer, closure)]
        self._capture(warmup, device)

    @classmethod
    def group(cls, fits, warmup=3, device=None, single_graph=False):
        """Grouped multi-instance execution: `fits` = a dip_group.GroupedFits (B fits of one architecture with the
        fused closure: ONE launch list, one hipGraph -- see that module), or [(optimizer, closure), ...] of INDEPENDENT nets
        with arbitrary closures (own weights, own BatchNorm statistics, own Adam state).  In the second form every fit is captured into its own
        hipGraph on its own HIP stream and one run() step replays all of them, so the kernels of
        different instances overlap on the chip -- what fills an MI355X when one image (e.g. the
        384x256 snail net: 25 us of math per iteration) cannot.
        single_graph=True captures all fits as concurrent branches of ONE graph instead (one graph
        launch per iteration; cross-stream capture of this size is fragile in the HIP runtime, so it is
        opt-in)."""
        import dip_group
        if isinstance(fits, dip_group.GroupedFits):
            # ONE launch list for all the fits (every kernel launch serves all instances, csrc/dip_group.h), captured as
            # ONE hipGraph: the form for many small fits -- 1/B of the launches of the per-fit graphs below
            return fits.capture(warmup)
        self = cls.__new__(cls)
        self.fits = list(fits)
        if single_graph or len(self.fits) == 1:
            self._capture(warmup, device)
            return self
        if device is None:
            device = self.fits[0][0].params[0].device
        self.device = device
        self.iterations = 0
        self.graph = None
        self.members = []
        with torch.cuda.device(device):
            for opt, clo in self.fits:
                m = cls.__new__(cls)
                m.fits = [(opt, clo)]
                m._capture(warmup, device)
                self.members.append(m)
        self.iterations = self.members[0].iterations
        return self

    def _one(self, optimizer, closure):
        optimizer.zero_grad()
        closure()
        optimizer.step()

    def _capture(self, warmup, device):
        if device is None:
            device = self.fits[0][0].params[0].device
        self.device = device
        self.iterations = 0
        with torch.cuda.device(device):
            cur = torch.cuda.current_stream(device)
            # The eager warm-up runs on the SAME streams the capture uses: autograd caches the stream of
            # every AccumulateGrad node, and a node created on another stream would pull a dependency on a
            # non-capturing stream into the capture.
            self.capture_stream = torch.cuda.Stream(device)
            self.branch_streams = [torch.cuda.Stream(device) for _ in self.fits[1:]]
            streams = [self.capture_stream] + self.branch_streams
            for s in streams:
                s.wait_stream(cur)
            import dip_engine
            dip_engine._graph_warmup[0] += 1          # an engine without a captured form (ResNetEngine) refuses HERE
            try:
                for _ in range(max(int(warmup), 1)):
                    for (opt, clo), s in zip(self.fits, streams):
                        with torch.cuda.stream(s):
                            self._one(opt, clo)
            finally:
                dip_engine._graph_warmup[0] -= 1
            for s in streams:
                cur.wait_stream(s)
            torch.cuda.synchronize(device)
            self.iterations += max(int(warmup), 1)
            self.graph = torch.cuda.CUDAGraph()
            # ROCm 7.2: per-launch event timing AFTER a captured graph of this iteration had been destroyed aborted
            # 10-25 % of bench.py's small-config runs with glibc heap-corruption errors (bench.py now takes those
            # timings before any graph exists: 0 / 30).  DIP_KEEP_GRAPHS=1 keeps every captured graph alive until the
            # interpreter exits instead -- not the default, because eager iterations run ~11 % slower while a
            # graph of the same net is alive (128 -> 113 it/s at 512x512).
            if os.environ.get("DIP_KEEP_GRAPHS", "0") == "1":
                _LIVE_GRAPHS.append((self.graph, self.capture_stream, self.branch_streams))
            with torch.cuda.graph(self.graph, stream=self.capture_stream):
                main = torch.cuda.current_stream(device)
                start = torch.cuda.Event()
                start.record(main)
                for (opt, clo), s in zip(self.fits[1:], self.branch_streams):
                    s.wait_event(start)                       # fork at the START: the branches run concurrently
                    with torch.cuda.stream(s):
                        self._one(opt, clo)
                self._one(*self.fits[0])
                for s in self.branch_streams:
                    main.wait_stream(s)                       # join

    def run(self, n=1):
        if self.graph is not None:
            for _ in range(int(n)):
                self.graph.replay()
        else:                                   # one graph per instance, each on its own stream
            cur = torch.cuda.current_stream(self.device)
            for m in self.members:
                m.capture_stream.wait_stream(cur)
            for _ in range(int(n)):
                for m in self.members:
                    with torch.cuda.stream(m.capture_stream):
                        m.graph.replay()
            for m in self.members:
                cur.wait_stream(m.capture_stream)
        self.iterations += int(n)


class NativeIteration:
    """One optimisation iteration of a skip() net under the fused loss head, without autograd: exactly

        opt.zero_grad()
        x = reg_noise() if reg_noise else net_input
        loss, out = head(x)
        loss.backward()
        opt.step()

    -- the body of the reference's optimize() loop (utils/common_utils.py:223-230) around the closure of
    inpainting.ipynb:300-315 / denoising.ipynb:204-221 -- issued by ONE call into the library (dip_iter_run): the reg-noise
    launch, the engine's forward command list, dip_loss_head_fwd, the BatchNorm batch counters, dip_loss_head_bwd, the engine's
    backward command list, dip_adam_tick + dip_adam_step_dev.  The two lists are the objects the eager path issues (same
    launches, same two-stream schedule, same events), so the results are bit-identical and the two forms may be mixed on the same
    net / head / optimiser at any iteration boundary.  No autograd node is built, nothing synchronises.

        head = MSEHead(net, target, mask=mask_or_None)
        opt = FusedAdam(get_params('net', net, net_input), lr=LR)
        it = NativeIteration(net, head, opt, net_input, reg_noise=RegNoise(net_input, std) or None)
        loss = it.step()          # 0-dim device tensor
        losses = it.run(n)        # device tensor [n]
        it.out                    # the last network output [1,C,H,W], detached (a buffer this object owns and overwrites)

    The command arrays are built once and rebuilt when the engine re-plans (input size, re-typed net), when the optimiser's
    parameters move or lr / betas / eps change, and when the head's target / mask or the noise settings are replaced.  Every
    slot of them is iteration-invariant; the ONE value that changes per iteration -- where the loss scalar goes -- is a field
    of the loss-head descriptor this object owns, which the library reads when it launches.

    monitor=FitMonitor(...) adds the rest of the denoising closure (denoising.ipynb:214-248: the exponential average of the
    output, the three PSNRs, the back-tracking checkpoint and fall-back; restoration.ipynb:192-211 is RestorationFitMonitor,
    below) to the same call: one
    more command array on the main stream between the backward list and Adam -- where `monitor.update(out, loss)` stands in the
    eager closure, after backward() and before opt.step() -- holding dip_fit_monitor_dev and, for a back-tracking monitor,
    dip_arena_backtrack.  dip_fit_monitor_dev reads the iteration index from `monitor.counter` in device memory (first =
    (i == 0), check = i % show_every != 0, record row i) and advances it, so its slots are iteration-invariant too; the loss
    address goes into its descriptor next to the head's.  Bit-identical to the eager closure with monitor.update(), and the
    two may alternate on one monitor: when `monitor.i` is not what the device counter will hold, the counter is set on the
    current stream before the iteration is issued.

        monitor = FitMonitor(net, img_noisy, img_gt, exp_weight=0.99, show_every=100, capacity=num_iter)
        it = NativeIteration(net, head, opt, net_input, reg_noise=reg, monitor=monitor)
        it.run(show_every); print(monitor.last())     # the notebook's print loop
        monitor.history(); monitor.out_avg

    head = SRHead(net, img_LR, downsampler) (super-resolution.ipynb:169-186) takes the MSEHead's place: the forward list then
    runs WITH the output conv and the head's launches are dip_head_fwd + dip_sr_loss_fwd and dip_sr_loss_bwd; `it.out` is
    out_HR, `head.out_LR` the down-sampled output.

    monitor=SRFitMonitor(img_LR, img_HR) with an SRHead is the bookkeeping of the super-resolution closure
    (super-resolution.ipynb:188-191: psnr_LR, psnr_HR, psnr_history.append) in the same slot: ONE launch entry,
    dip_sr_monitor_dev, whose descriptor points at `it.out` (out_HR), the head's out_LR buffer and the monitor's images, with
    the loss address handled like FitMonitor's.  It reads and advances `monitor.counter` the same way, so eager
    `monitor.update(out_HR, head.out_LR, loss)` calls and native iterations alternate on one monitor.  It does not touch the
    fit: parameters and losses are bit-identical to monitor=None.  An SRFitMonitor with an MSEHead, images that do not match
    the head's LR size / the net output, and a monitor on another device are refused before anything is issued.

        monitor = SRFitMonitor(img_LR, img_HR, capacity=num_iter)
        it = NativeIteration(net, SRHead(net, img_LR, downsampler), opt, net_input, reg_noise=reg, monitor=monitor)
        it.run(num_iter); psnr_history = monitor.history()[:, 3:5]

    monitor=RestorationFitMonitor(net, img, mask) is the bookkeeping of the restoration / inpainting closure
    (restoration.ipynb:192-211: psrn_masked and psrn in every iteration; ON every show_every-th iteration the fall-back to the
    last checkpoint when psrn_masked dropped by more than 5 dB, or else the checkpoint) in the same slot and the same shape
    as FitMonitor's: dip_restore_monitor_dev -- its descriptor points at `it.out` and the monitor's image and mask, reads the
    iteration index from `monitor.counter` (check = i % show_every == 0, record row i) and advances it -- and, for a
    back-tracking monitor, dip_arena_backtrack.  The head is usually MSEHead(net, img, mask=mask); the monitor keeps its own
    mask ([1,1|C,H,W]) and asks nothing of the head.  Bit-identical to the eager closure with monitor.update(out, loss); the
    two may alternate on one monitor.

        monitor = RestorationFitMonitor(net, img_var, mask_var, show_every=50, capacity=num_iter)
        it = NativeIteration(net, MSEHead(net, img_var, mask=mask_var), opt, net_input, reg_noise=reg, monitor=monitor)
        it.run(num_iter); monitor.history()           # [iters, 6]: loss, mse_masked, mse, psrn_masked, psrn, fell_back

    step() / run(n) past the monitor's capacity raise before anything is issued.  The monitor's buffers and settings are
    part of the plan's key (replace `monitor.out_avg`, or assign another monitor to `it.monitor`: the arrays are rebuilt).

    early_stop=EarlyStopMonitor(img_like, window, patience, net=net) is independent of monitor=: the ground-truth-free stopping
    criterion (the windowed moving variance of the output; utils.fit_monitor) as one more command array on the main stream,
    behind the monitor's array if there is one and in front of Adam -- where `es.update(out)` stands in the eager closure, so
    `es.best_params` are the parameters that produced `es.best_out`.  It holds dip_early_stop_dev (which reads the row index
    from `es.counter` and the ring head from `es.state`) and, with net=, dip_early_stop_keep over the parameter arena.  It
    does not touch the fit: losses and parameters are bit-identical to early_stop=None, and with early_stop=None the plan's key
    is what it was.  Eager `es.update(out)` calls and native iterations alternate on one monitor.

        es = EarlyStopMonitor(img_noisy, window=100, patience=1000, net=net, capacity=num_iter)
        it = NativeIteration(net, head, opt, net_input, reg_noise=reg, early_stop=es)
        issued, losses = it.run_until(num_iter, check_every=50)      # polls the 4-byte `stopped` word once per 50 iterations
        es.best_iter, es.best_out; es.restore_best()

    An SGLD optimiser -- FusedAdam(..., weight_decay=, noise_std=, noise_seed=) -- is accepted as it is: the Adam phase then holds
    dip_adam_sgld_step_dev instead of dip_adam_step_dev, on the DipSgldState the eager opt.step() uses, so the two forms still
    alternate bit-identically; opt.set_noise_std(x) between run() calls needs no re-plan.  The plan's key gains the new fields only
    for such an optimiser.

    posterior=PosteriorMonitor(img_like, burn_in, every) is a third keyword, independent of the other two: the sample mean and
    variance of the outputs (utils.fit_monitor) as one more command array, dip_posterior_dev, behind monitor= and early_stop= and
    in front of Adam -- where `pm.update(out)` stands in the eager closure, so a sample is the output of the parameters that are
    about to be stepped and perturbed.  It does not touch the fit; with posterior=None the plan's key is what it was.  With
    PosteriorMonitor(..., img_gt=) the array holds dip_posterior_rec_dev instead (phase name posterior_rec_dev): the same mean
    and m2, and one record {iteration, mse_mean, psnr_mean} of the posterior mean against the ground truth per SAMPLE.

        opt = FusedAdam(get_params('net', net, net_input), lr=LR, weight_decay=5e-8, noise_std=1e-4, noise_seed=0)
        pm = PosteriorMonitor(img_noisy, burn_in=7000, every=50)
        it = NativeIteration(net, head, opt, net_input, reg_noise=reg, posterior=pm)
        it.run(num_iter); pm.mean, pm.variance(), pm.count

    ssim=SSIMMonitor(img_gt, img_avg=None) is a fourth keyword: the mean structural similarity of the output against a ground
    truth (utils.fit_monitor; with an SRHead img_gt is img_HR) as one more command array, dip_ssim_dev, behind the other three
    and in front of Adam.  It stands behind monitor= so that with img_avg=monitor.out_avg the smoothed output it reads is this
    iteration's.  It does not touch the fit; with ssim=None the plan's key is what it was.

        sm = SSIMMonitor(img_gt, img_avg=monitor.out_avg, capacity=num_iter)
        it = NativeIteration(net, head, opt, net_input, reg_noise=reg, monitor=monitor, ssim=sm)
        it.run(num_iter); sm.history()                # [iters, 2]: ssim, ssim_sm"""

    def __init__(self, net, head, optimizer, net_input, reg_noise=None, monitor=None, early_stop=None, posterior=None,
                 ssim=None):
        import dip_group
        from utils.loss_head import MSEHead, SRHead
        from utils.reg_noise import RegNoise
        if isinstance(net, dip_group.GroupedFits) or isinstance(head, dip_group.GroupedFits):
            raise NotImplementedError("dip-amd: NativeIteration drives ONE fit; grouped fits run through "
                                      "GraphedIteration.group(GroupedFits(...))")
        eng = getattr(net, "__dict__", {}).get("_dip_engine")
        if eng is None or isinstance(eng, Exception):
            raise RuntimeError("dip-amd: NativeIteration needs a net built by models.skip.skip()")
        if eng.kind != "skip":
            raise NotImplementedError("dip-amd: NativeIteration covers skip() nets; the ResNet backbone has no fused loss head "
                                      "(run it through the eager closure)")
        self.net, self.engine = net, eng
        self._check_training()
        if not isinstance(optimizer, FusedAdam):
            raise TypeError(f"dip-amd: NativeIteration needs a dip_optim.FusedAdam, got {type(optimizer).__name__}")
        want = eng.param_list
        if len(optimizer.params) != len(want) or any(a is not b for a, b in zip(optimizer.params, want)):
            raise ValueError("dip-amd: NativeIteration steps exactly the net's parameters (get_params('net', ...)); "
                             "opt_over with 'input' or 'down' goes through the eager closure")
        # (the monitor's type is refused before the first check that needs a GPU)
        self.monitor, self.device = monitor, getattr(net_input, "device", None)
        self.early_stop, self.posterior, self.ssim = early_stop, posterior, ssim
        self._check_monitors()
        if not isinstance(net_input, torch.Tensor) or not net_input.is_cuda:
            raise RuntimeError("dip-amd: NativeIteration works on MI355X tensors only (net_input is on the CPU; no CPU "
                               "fallback)")
        if net_input.dim() != 4 or net_input.shape[0] != 1 or net_input.dtype != torch.float32 \
                or not net_input.is_contiguous():
            raise ValueError(f"dip-amd: net_input must be a contiguous fp32 [1,C,H,W] tensor, got {net_input.dtype} "
                             f"{tuple(net_input.shape)}")
        if net_input.requires_grad:
            raise ValueError("dip-amd: net_input requires grad (opt_over='net,input'): that goes through the eager closure")
        if not isinstance(head, (MSEHead, SRHead)):
            raise TypeError(f"dip-amd: NativeIteration needs a utils.loss_head.MSEHead or SRHead, got {type(head).__name__}")
        if head.net is not net:
            raise ValueError(f"dip-amd: the {type(head).__name__} was built for another net")
        head._check_state()
        if reg_noise is not None:
            if not isinstance(reg_noise, RegNoise):
                raise TypeError("dip-amd: reg_noise must be a utils.reg_noise.RegNoise or None, got "
                                f"{type(reg_noise).__name__}")
            if reg_noise.saved.shape != net_input.shape or reg_noise.saved.device != net_input.device:
                raise ValueError("dip-amd: the RegNoise was built for another net_input")
        self.head, self.opt = head, optimizer
        self._check_monitors()                    # (now with the head: an SRFitMonitor records the two outputs of an SRHead)
        self.net_input, self.reg = net_input.detach(), reg_noise
        self.out = None
        self.iterations = 0
        self._key = None
        self._plan = None
        self._one = torch.ones(1, dtype=torch.float32, device=self.device)      # d loss / d loss, as autograd seeds backward()
        self._check_capture()

    def _check_capture(self):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("dip-amd: NativeIteration.step() cannot be captured into a hipGraph (its loss slot changes per "
                               "iteration); capture the eager closure with GraphedIteration instead")

    def _check_training(self):
        if not self.net.training:
            raise NotImplementedError("dip-amd: eval-mode BatchNorm is not implemented (NativeIteration needs net.train())")

    def _monitors(self):
        """The monitors of this iteration in launch order -- monitor=, then early_stop=, then posterior=, then ssim=, all in
        front of Adam -- as (slot, monitor) pairs."""
        return [(slot, getattr(self, slot)) for slot in ("monitor", "early_stop", "posterior", "ssim")
                if getattr(self, slot) is not None]

    def _check_monitors(self):
        """What can be said about monitor= and early_stop= before the output size is known (the image shape: _build)."""
        import utils.fit_monitor as FM
        takes = {"monitor": ((FM.FitMonitor, FM.SRFitMonitor, FM.RestorationFitMonitor), "dip-amd: monitor must be a "
                             "utils.fit_monitor.FitMonitor, an SRFitMonitor, a RestorationFitMonitor or None", "back-tracks"),
                 "early_stop": (FM.EarlyStopMonitor, "dip-amd: early_stop must be a utils.fit_monitor.EarlyStopMonitor or None",
                                "keeps the parameters of"),
                 "posterior": (FM.PosteriorMonitor, "dip-amd: posterior must be a utils.fit_monitor.PosteriorMonitor or None",
                               "samples"),
                 "ssim": (FM.SSIMMonitor, "dip-amd: ssim must be a utils.fit_monitor.SSIMMonitor or None", "records")}
        head = getattr(self, "head", None)
        for slot, m in self._monitors():
            types, refusal, copies = takes[slot]
            if not isinstance(m, types):
                raise TypeError(f"{refusal}, got {type(m).__name__}")
            if head is not None and m.head_kind not in (None, head.kind):
                raise TypeError(f"dip-amd: an SRFitMonitor records out_LR and out_HR of a utils.loss_head.SRHead, the head is a "
                                f"{type(head).__name__} (use a FitMonitor)")
            if m.dev != self.device:
                raise RuntimeError(f"dip-amd: the {type(m).__name__} lives on {m.dev}, the iteration runs on {self.device}")
            if m.engine is not None and m.engine is not self.engine:
                raise ValueError(f"dip-amd: the {type(m).__name__} {copies} another net (it was built for a different skip() net)")

    # -------------------------------------------------------------------------------------------- the command arrays
    def _signature(self, sig):
        """Everything a slot of the command arrays was computed from.  Objects by identity: the arrays hold raw pointers, and
        the plan keeps every object of its key alive, so neither an id nor an address can be recycled unnoticed."""
        eng, head, opt, reg = self.engine, self.head, self.opt, self.reg
        # (an engine that has never planned has no op lists yet: None never equals a built key)
        return (id(eng._clists), eng.shape_key, id(getattr(eng, "fwd_ops", None)), id(getattr(eng, "bwd_ops", None)), sig,
                *opt._plan_key(),
                head._plan_key(),
                None if reg is None else reg._plan_key()) \
            + tuple((slot, m._plan_key()) for slot, m in self._monitors())       # (no monitors: the key as it was)

    def _build(self):
        eng, head, opt, reg = self.engine, self.head, self.opt, self.reg
        lib = N.lib()
        dev = self.device
        self._check_monitors()
        noisy = reg is not None and reg.noisy
        x = self.net_input if reg is None else (reg.out if noisy else reg.saved)
        _, Cimg, H, W = x.shape
        eng._prepare(dev, H, W, Cimg)
        if opt._sig != opt._signature():
            opt._prepare()
        fwd, bwd = eng.iteration_lists(with_out_conv=head.with_out_conv)
        out = self.out
        if out is None or tuple(out.shape) != (1, eng.n_out, eng.Hout, eng.Wout) or out.device != dev:
            out = torch.empty((1, eng.n_out, eng.Hout, eng.Wout), dtype=torch.float32, device=dev)
        loss0 = torch.zeros((), dtype=torch.float32, device=dev)
        desc = head._descriptor(eng, out, loss0)
        pre = []
        if noisy:
            pre.append(reg._launch(lib))           # dip_noise_axpy_dev, or dip_noise_axpy_dev1s on the device-side level
        pre += eng._forward_prologue(x.data_ptr())
        mid = head.fwd_launches(eng, desc)
        if len(eng.bns):
            mid.append((lib.dip_counter_add_n, (eng.nbt.data_ptr(), eng.nbt.numel(), 1), "num_batches_tracked"))
        mid += head.bwd_launches(eng, desc, self._one.data_ptr())
        st = opt._state(dev, opt.step_count)
        adam = [opt._tick_launch(lib, dev, st)]    # dip_adam_tick, or dip_adam_tick_dev on the device-side lr
        pbase, gbase = eng.params.data_ptr(), eng.grads.data_ptr()
        for g in opt._groups:
            if g.params[0].device != dev or g.base < pbase or g.base + 4 * g.numel > pbase + 4 * eng.params.numel():
                raise RuntimeError("dip-amd: a FusedAdam group lies outside the net's parameter arena")
            # the gradient arena mirrors the parameter arena: the group's gradients are flat at the same offset
            # (an SGLD optimiser: dip_adam_sgld_step_dev on the DipSgldState the eager opt.step() uses)
            adam.append(opt._step_launch(lib, g, gbase + (g.base - pbase), st))
        on_main = lambda ops: N.CmdList([("launch", fn, args, 0, name) for fn, args, name in ops])
        phases = [on_main(pre), fwd, on_main(mid), bwd, on_main(adam)]
        # monitor.update()'s place in stream order: after backward(), before opt.step() -- a fall-back overwrites the parameters
        # after this iteration's gradients were computed and before Adam applies them; es.update(out)'s place is behind it
        # (the fall-back has been applied: the arena it keeps holds the parameters that produced `out`).  Each monitor checks
        # its images against the outputs -- an SRHead's LR buffer exists now -- and says what it launches.
        descs = {}
        for slot, m in self._monitors():
            descs[slot], ops = m._plan(eng, out, head)
            phases.insert(len(phases) - 1, on_main(ops))
        mdesc = descs.get("monitor")
        if mdesc is not None:
            mdesc.loss = loss0.data_ptr()
        lists = N.IterList(phases)
        views = [eng.grads[o:o + p.numel()].view(p.shape) for p, o in zip(eng.param_list, eng.slots)]
        self.out = out
        # everything a slot points to stays alive with the plan, and so does every object whose id is part of the key
        self._plan = dict(lists=lists, desc=desc, mdesc=mdesc, edesc=descs.get("early_stop"), views=views, x=x, state=st,
                          loss0=loss0,
                          keep=(head._plan_keep(), eng._clists, eng.fwd_ops, eng.bwd_ops, opt._groups,
                                eng.params, eng.grads, eng.nbt, eng.dy_out,
                                None if reg is None else (reg.saved, reg.out, reg.offset, reg.std_dev),
                                opt._lr_dev.get(dev),
                                [m._plan_keep() for _, m in self._monitors()]))
        self._key = self._signature(opt._sig)

    # -------------------------------------------------------------------------------------------- run
    def _begin(self, n=1):
        self._check_training()
        self._check_capture()
        self._check_monitors()                    # (`it.monitor` may have been replaced)
        self.head._check_state()                  # (an SRHead's down-sampler may have become trainable)
        for _, m in self._monitors():
            m._check_room(n)
        # (the parameters' addresses are part of the key: they also say that the engine's arena still holds the parameters)
        if self._signature(self.opt._signature()) != self._key:
            self._build()
        for _, m in self._monitors():
            m._sync_counter()                     # eager update() calls in between: the device index follows monitor.i
        eng = self.engine
        ptrs = [torch.cuda.current_stream(self.device).cuda_stream]
        if eng.two_streams:
            ptrs += [s_.cuda_stream for s_ in eng._aux_streams()[1]]
        return ptrs

    def _issue(self, loss_ptr, ptrs):
        self._plan["desc"].loss = loss_ptr        # read by the head's forward launch (dip_loss_head_fwd / dip_sr_loss_fwd)
        if self._plan["mdesc"] is not None:
            self._plan["mdesc"].loss = loss_ptr   # column 0 of this iteration's record (dip_fit_monitor_dev / dip_sr_monitor_dev)
        self._plan["lists"].run(ptrs)

    def _finish(self, n):
        eng = self.engine
        for p, v in zip(eng.param_list, self._plan["views"]):      # what autograd leaves after zero_grad() + backward()
            if p.grad is not v:
                p.grad = v
        eng.fwd_id += n                           # (a pending autograd backward of an earlier eager forward is stale now)
        eng.last_out, eng.last_head = self.out, self.head
        self.opt.step_count += n
        self.iterations += n
        for _, m in self._monitors():
            m._advance(n)

    @torch.no_grad()
    def step(self):
        """One iteration; returns the loss as a 0-dim device tensor (no host synchronisation)."""
        with torch.cuda.device(self.device):
            ptrs = self._begin()
            loss = torch.empty((), dtype=torch.float32, device=self.device)
            self._issue(loss.data_ptr(), ptrs)
            self._finish(1)
        return loss

    @torch.no_grad()
    def run(self, n):
        """n iterations; returns their losses as a device tensor [n] (no host synchronisation inside)."""
        n = max(int(n), 0)
        with torch.cuda.device(self.device):
            losses = torch.empty(n, dtype=torch.float32, device=self.device)
            if n == 0:
                return losses
            ptrs = self._begin(n)
            base = losses.data_ptr()
            done = 0
            try:
                for i in range(n):
                    self._issue(base + 4 * i, ptrs)
                    done += 1
            finally:
                if done:
                    self._finish(done)
        return losses

    def run_until(self, max_iter, check_every=50):
        """Runs until the EarlyStopMonitor says stop, or max_iter: issues `check_every` iterations at a time and reads the
        device's 4-byte `stopped` word after each batch (one copy and one synchronisation per batch).  Returns
        (iterations_issued, losses [iterations_issued], a device tensor).  It stops at the first batch boundary at or after the
        stopping iteration: at most check_every - 1 iterations too many, which keep training the net but cannot touch the
        frozen best_out / best_params (es.restore_best() puts the minimum's parameters back)."""
        es = self.early_stop
        if es is None:
            raise RuntimeError("dip-amd: NativeIteration.run_until needs early_stop=EarlyStopMonitor(...)")
        max_iter, check_every = max(int(max_iter), 0), int(check_every)
        if check_every < 1:
            raise ValueError(f"dip-amd: run_until: check_every must be >= 1, got {check_every}")
        es._check_room(max_iter)                   # (before anything is issued, as run(max_iter) would)
        parts, issued = [], 0
        while issued < max_iter:
            n = min(check_every, max_iter - issued)
            parts.append(self.run(n))
            issued += n
            if es.stopped:
                break
        with torch.cuda.device(self.device):
            losses = torch.cat(parts) if parts else torch.empty(0, dtype=torch.float32, device=self.device)
        return issued, losses


class ArenaLBFGS:
    """torch.optim.LBFGS (no line search: `line_search_fn=None`, the reference's setting,
    utils/common_utils.py:218) restated on FLAT vectors: when all parameters are views of one
    contiguous arena (a SkipNet's parameters; the gaps between tensors hold zeros in both the
    parameter and the gradient arena) the parameter vector and the gradient are the arenas themselves
    -- no per-tensor gather/scatter of 112 tensors per evaluation -- and the two-loop recursion runs
    on 2.2 M-element device vectors.  Other parameter lists are gathered/scattered like torch does.
    Same update rule, same stopping tests (with tolerance -1 the quirk `gtd > -tolerance_change`
    stops the run when the directional derivative exceeds 1), same history handling."""

    def __init__(self, params, lr=1, max_iter=20, max_eval=None, tolerance_grad=1e-7, tolerance_change=1e-9,
                 history_size=100, _allow_cpu=False):
        self.params = list(params)
        self.lr, self.max_iter = lr, max_iter
        self.max_eval = max_eval if max_eval is not None else max_iter * 5 // 4
        self.tolerance_grad, self.tolerance_change, self.history_size = tolerance_grad, tolerance_change, history_size
        self.state = {"func_evals": 0, "n_iter": 0}
        for p in self.params:          # (_allow_cpu: the algorithm-vs-torch.optim.LBFGS unit test only)
            if (not p.is_cuda and not _allow_cpu) or p.dtype != torch.float32:
                raise RuntimeError("dip-amd ArenaLBFGS: parameters must be fp32 CUDA tensors (no CPU optimiser path)")
        self._flat = None
        self._sig = None

    def _bind(self):
        """(Re)derives the flat view: a SkipNet's parameters become views of one arena at its first
        forward (and again after .type()/.to()), so this is checked at every step()."""
        sig = tuple(p.data_ptr() for p in self.params)
        if sig == self._sig:
            return
        self._sig = sig
        self._flat = None
        if len(_split_contiguous(self.params)) == 1:
            p0, pl = self.params[0], self.params[-1]
            n = (pl.data_ptr() - p0.data_ptr()) // 4 + pl.numel()
            st = p0.untyped_storage()
            off = (p0.data_ptr() - st.data_ptr()) // 4
            self._flat = torch.empty(0, dtype=torch.float32, device=p0.device).set_(st, off, (n,), (1,))
            self._offsets = [(p.data_ptr() - p0.data_ptr()) // 4 for p in self.params]

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            p.grad = None if set_to_none else (p.grad.zero_() if p.grad is not None else None)

    def _gather_flat_grad(self):
        g0 = self.params[0].grad
        if self._flat is not None and g0 is not None:
            base = g0.data_ptr() - 4 * self._offsets[0]
            if all(p.grad is not None and p.grad.is_contiguous() and p.grad.data_ptr() == base + 4 * o
                   for p, o in zip(self.params, self._offsets)):
                st = g0.untyped_storage()
                off = (base - st.data_ptr()) // 4
                return torch.empty(0, dtype=torch.float32, device=g0.device).set_(st, off, (self._flat.numel(),),
                                                                                  (1,)).clone()
        views = [(p.grad.reshape(-1) if p.grad is not None else p.new_zeros(p.numel())) for p in self.params]
        if self._flat is not None:
            # same layout as the fast path (arena length, alignment gaps zero): history vectors of both paths mix
            g = torch.zeros(self._flat.numel(), dtype=torch.float32, device=self._flat.device)
            for v, o in zip(views, self._offsets):
                g[o:o + v.numel()].copy_(v)
            return g
        return torch.cat(views, 0)

    def _add_grad(self, t, d):
        if self._flat is not None and d.numel() == self._flat.numel():
            self._flat.add_(d, alpha=t)
            return
        off = 0
        for p in self.params:
            n = p.numel()
            p.data.add_(d[off:off + n].view_as(p), alpha=t)
            off += n

    @torch.no_grad()
    def step(self, closure):
        closure = torch.enable_grad()(closure)
        lr, max_iter, max_eval = self.lr, self.max_iter, self.max_eval
        tg, tc, hs = self.tolerance_grad, self.tolerance_change, self.history_size
        st = self.state
        orig_loss = closure()
        self._bind()
        loss = float(orig_loss)
        current_evals = 1
        st["func_evals"] += 1
        g = self._gather_flat_grad()
        if float(g.abs().max()) <= tg:
            return orig_loss
        d, t = st.get("d"), st.get("t")
        old_dirs, old_stps, ro = st.get("old_dirs"), st.get("old_stps"), st.get("ro")
        H_diag, prev_g, prev_loss = st.get("H_diag"), st.get("prev_flat_grad"), st.get("prev_loss")
        n_iter = 0
        while n_iter < max_iter:
            n_iter += 1
            st["n_iter"] += 1
            if st["n_iter"] == 1:
                d = g.neg()
                old_dirs, old_stps, ro = [], [], []
                H_diag = 1
            else:
                y = g.sub(prev_g)
                s = d.mul(t)
                ys = float(y.dot(s))
                if ys > 1e-10:
                    if len(old_dirs) == hs:
                        old_dirs.pop(0)
                        old_stps.pop(0)
                        ro.pop(0)
                    old_dirs.append(y)
                    old_stps.append(s)
                    ro.append(1.0 / ys)
                    H_diag = ys / float(y.dot(y))
                num_old = len(old_dirs)
                al = [None] * num_old
                q = g.neg()
                for i in range(num_old - 1, -1, -1):
                    al[i] = float(old_stps[i].dot(q)) * ro[i]
                    q.add_(old_dirs[i], alpha=-al[i])
                d = r = torch.mul(q, H_diag)
                for i in range(num_old):
                    be_i = float(old_dirs[i].dot(r)) * ro[i]
                    r.add_(old_stps[i], alpha=al[i] - be_i)
            prev_g = g.clone(memory_format=torch.contiguous_format)
            prev_loss = loss
            t = min(1.0, 1.0 / float(g.abs().sum())) * lr if st["n_iter"] == 1 else lr
            gtd = float(g.dot(d))
            if gtd > -tc:
                break
            ls_func_evals = 0
            self._add_grad(t, d)
            if n_iter != max_iter:
                loss = float(closure())
                g = self._gather_flat_grad()
                ls_func_evals = 1
            current_evals += ls_func_evals
            st["func_evals"] += ls_func_evals
            if n_iter == max_iter or current_evals >= max_eval:
                break
            if float(g.abs().max()) <= tg:
                break
            if float(d.mul(t).abs().max()) <= tc:
                break
            if abs(loss - prev_loss) < tc:
                break
        st.update(d=d, t=t, old_dirs=old_dirs, old_stps=old_stps, ro=ro, H_diag=H_diag, prev_flat_grad=prev_g,
                  prev_loss=prev_loss)
        return orig_loss
