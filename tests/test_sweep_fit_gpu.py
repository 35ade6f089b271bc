"""Learning-rate and input-noise sweeps and schedules on a real MI355X: dip_group.GroupedFits(lr=[...], reg_noise_std=[...])
with its setters, eager and as ONE hipGraph, against the solo NativeIteration fits of its instances; FusedAdam(device_lr=True) +
RegNoise(device_std=True) eager, under NativeIteration and under GraphedIteration against the plain forms with the values
changed at the same iteration boundary; and the launch lists and plan keys of the defaults.  The scalars are read from device
memory by kernels that run the bodies of the by-value kernels, so every comparison is torch.equal."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

import dip_native as N  # noqa: E402
from test_group_gpu import _problem  # noqa: E402
from test_group_monitor_gpu import _stream_pool_stands_where_it_stood  # noqa: E402,F401  (autouse: the engines of this module
#                                                                                          draw pooled streams too)
from test_native_iter_gpu import _assert_same_state, _eager_step, _fit  # noqa: E402
from test_native_iter_host import _small  # noqa: E402
from test_sgld_fit_gpu import _group_nets, _mse_fit  # noqa: E402
from test_sr_head_gpu import _make_net  # noqa: E402
from test_sr_tv_gpu import _tv_weight_for  # noqa: E402

B = 3
HW = (36, 52)                     # 9 x 13 at the deepest scale: Concat's centre crops (tests/test_group_gpu.py)
LRS = [0.01, 0.001, 0.1]          # the learning rates of the reference's notebooks
STDS = [1. / 30., 1. / 20., 0.03]  # ... and their reg_noise_std
SEEDS = [40, 41, 42]
NEW = ("adam_tick_dev", "noise_axpy_dev3", "noise_axpy_dev1s")


class _Solo:
    """One instance on its own: FusedAdam(lr) + RegNoise(std, seed) + the head under NativeIteration; `losses` is its history."""

    def __init__(self, net, z, head, lr, std, seed, **monitors):
        from dip_optim import FusedAdam, NativeIteration
        from utils.common_utils import get_params
        from utils.reg_noise import RegNoise
        self.net, self.head = net, head
        self.opt = FusedAdam(get_params("net", net, z), lr=lr)
        self.reg = RegNoise(z, std, seed=seed)
        self.es, self.sm, self.mon = monitors.get("early_stop"), monitors.get("ssim"), None
        self.it = NativeIteration(net, head, self.opt, z, reg_noise=self.reg, **monitors)
        self.losses, self.loss = [], None

    def run(self, n):
        self.losses += list(self.it.run(n).unbind(0))
        self.loss = self.losses[-1]

    def set(self, lr, std):
        """What g.set_lr / g.set_reg_noise_std do to this instance, the plain way: the next run() re-plans."""
        self.opt.lr, self.reg.std = lr, std


def _group_history(g, run, n, hist):
    for _ in range(n):
        run(1)
        hist.append(g.losses.clone())


def _assert_group_equals_solo(g, nets, solo, hist, what=""):
    torch.cuda.synchronize()
    ex = g._row0_extra
    assert g.step_counts() == [len(hist)] * B == [s.opt.device_step_count() for s in solo], what
    for b, s in enumerate(solo):
        w = (what, b)
        assert torch.equal(torch.stack(hist)[:, b], torch.stack(s.losses)), (w, torch.stack(hist)[:, b].tolist(),
                                                                             torch.stack(s.losses).tolist())
        assert torch.equal(g.out[b:b + 1], s.it.out), w
        if g.out_LR is not None:
            assert torch.equal(g.out_LR[b:b + 1], s.head.out_LR), w
        for (k, pa), pb in zip(nets[b].named_parameters(), s.net.parameters()):
            assert torch.equal(pa, pb), (w, k)
        for (k, ba), bb in zip(nets[b].named_buffers(), s.net.buffers()):
            assert torch.equal(ba, bb), (w, k)
        eng = s.net.__dict__["_dip_engine"]
        gm, gv = g._inst(ex["m"], b), g._inst(ex["v"], b)
        assert len(s.opt._groups) >= 1
        for gr in s.opt._groups:
            o = (gr.base - eng.params.data_ptr()) // 4
            assert torch.equal(gm[o:o + gr.numel], gr.m.reshape(-1)) and torch.equal(gv[o:o + gr.numel], gr.v.reshape(-1)), w


def _mse_group(dev, **kw):
    """(group, nets, the solo twins' constructor arguments) of the masked MSE group at 36 x 52."""
    from dip_group import GroupedFits
    from utils.loss_head import MSEHead
    zs, ts, ms = _problem("skip3", HW, B, 1, dev)
    nets = _group_nets(dev, B)
    refs = [copy.deepcopy(n) for n in nets]
    g = GroupedFits(nets, zs, ts, masks=ms, seeds=SEEDS, lr=LRS, reg_noise_std=STDS, **kw)
    assert g.pointers_outside_row0() == []
    heads = [MSEHead(refs[b], ts[b], mask=ms[b]) for b in range(B)]
    return g, nets, refs, zs, heads


# ------------------------------------------------------------------------------------------ grouped sweeps == solo fits
def test_grouped_mse_sweep_equals_its_solo_fits(dev):
    """lr and reg_noise_std lists, masked MSE: 3 eager iterations, capture(), 3 replays; the rows behind everything else."""
    g, nets, refs, zs, heads = _mse_group(dev)
    assert list(g._row0_extra)[-2:] == ["lr", "reg_std"] and g.lr == LRS and g.std == STDS
    solo = [_Solo(refs[b], zs[b], heads[b], LRS[b], STDS[b], SEEDS[b]) for b in range(B)]
    for s in solo:
        s.run(6)
    hist = []
    _group_history(g, g.step, 2, hist)
    g.capture(warmup=1)                               # the third eager iteration, then ONE hipGraph
    hist.append(g.losses.clone())
    assert g.graph is not None and g.iterations == 3
    _group_history(g, g.run, 3, hist)
    _assert_group_equals_solo(g, nets, solo, hist)
    assert N.lib().dip_group_size() == 1
    # the instances really are different fits
    assert len({round(g.losses[b].item(), 9) for b in range(B)}) == B


def test_grouped_sr_sweep_with_tv_weights_equals_its_solo_fits(dev):
    """The 64 x 96, factor-4 super-resolution fit with a TV term: lists for lr, reg_noise_std and tv_weights in one group."""
    from dip_group import GroupedFits
    from utils.loss_head import SRHead
    from models.downsampler import Downsampler
    gen = torch.Generator().manual_seed(21)
    nets = [_make_net("small", 3 + b, 3)[0].to(dev) for b in range(B)]
    downs = [Downsampler(n_planes=3, factor=4, kernel_type="lanczos2", phase=0.5, preserve_size=True).to(dev) for _ in range(B)]
    zs = [(torch.rand(1, 8, 64, 96, generator=gen) * 0.1).to(dev) for _ in range(B)]
    lrs = [torch.rand(1, 3, 16, 24, generator=gen).to(dev) for _ in range(B)]
    w0 = _tv_weight_for(nets[0], downs[0], zs[0], lrs[0])
    ws = [w0 * r for r in (0.25, 1.0, 4.0)]
    refs = [copy.deepcopy(n) for n in nets]
    solo = [_Solo(refs[b], zs[b], SRHead(refs[b], lrs[b], downs[b], tv_weight=ws[b]), LRS[b], STDS[b], SEEDS[b]) for b in range(B)]
    for s in solo:
        s.run(6)
    g = GroupedFits(nets, zs, lrs, downsamplers=downs, tv_weights=ws, seeds=SEEDS, lr=LRS, reg_noise_std=STDS)
    assert g.pointers_outside_row0() == [] and list(g._row0_extra)[-2:] == ["lr", "reg_std"]
    hist = []
    _group_history(g, g.step, 2, hist)
    g.capture(warmup=1)
    hist.append(g.losses.clone())
    _group_history(g, g.run, 3, hist)
    _assert_group_equals_solo(g, nets, solo, hist)


def test_setters_under_a_captured_graph(dev):
    """capture(), 2 replays, set_lr + set_reg_noise_std (one instance to level 0), 2 more replays of the SAME graph: the solo
    fits whose opt.lr / reg.std were changed at the same boundary."""
    g, nets, refs, zs, heads = _mse_group(dev)
    solo = [_Solo(refs[b], zs[b], heads[b], LRS[b], STDS[b], SEEDS[b]) for b in range(B)]
    lrs2, stds2 = [1e-3, 0.1, 1. / 3.], [0.05, 0.0, 1. / 30.]
    hist = []
    g.capture(warmup=1)
    hist.append(g.losses.clone())
    graph = g.graph
    _group_history(g, g.run, 2, hist)
    g.set_lr(lrs2)
    g.set_reg_noise_std(stds2)
    _group_history(g, g.run, 2, hist)
    assert g.graph is graph and g.lr == lrs2 and g.std == stds2 and g.iterations == 5
    for b, s in enumerate(solo):
        s.run(3)
        s.set(lrs2[b], stds2[b])
        s.run(2)
    _assert_group_equals_solo(g, nets, solo, hist)
    ex = g._row0_extra
    assert [g._inst(ex["lr"], b).item() for b in range(B)] == lrs2
    assert [g._inst(ex["reg_std"], b).item() for b in range(B)] == [torch.tensor(v).float().item() for v in stds2]
    # instance 1 at level 0 on the noise path: saved + 0 * N
    assert torch.equal(g._inst(ex["noisy"], 1), g._inst(ex["saved"], 1))
    assert not torch.equal(g._inst(ex["noisy"], 0), g._inst(ex["saved"], 0))
    # the stream of every instance advanced in all 5 iterations (a solo fit at level 0 draws nothing)
    quads = (ex["saved"].numel() + 3) // 4
    assert [g._inst(ex["rng"], b).tolist() for b in range(B)] == [[5 * quads, SEEDS[b]] for b in range(B)]


def test_a_schedule_changes_the_fit(dev):
    """The setter is not a no-op: the group that anneals lr ends elsewhere than the group that does not."""
    res = []
    for anneal in (False, True):
        g, nets, *_ = _mse_group(dev)
        g.step(2)
        if anneal:
            g.set_lr([x * 0.1 for x in LRS])
        g.step(2)
        torch.cuda.synchronize()
        res.append(g.losses.clone())
    assert not torch.equal(res[0], res[1])


# ------------------------------------------------------------------------------------------ solo device forms
def _dev_fit(dev, device=True):
    from dip_optim import FusedAdam
    from utils.common_utils import get_params
    from utils.reg_noise import RegNoise
    torch.manual_seed(11)
    f = _fit(dev, _small(), 8, HW, 5, masked=True, noisy=True)
    f.opt = FusedAdam(get_params("net", f.net, f.z), lr=0.01, device_lr=device)
    f.reg = RegNoise(f.z, 1. / 30., seed=7, device_std=device)
    return f


def _same_fit(a, b, out_b, what):
    """_assert_same_state without the host-side step count (a graph replay does not advance it) and the gradients' identity."""
    torch.cuda.synchronize()
    sa, sb = a.net.state_dict(), b.net.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (what, k)
    for ga, gb in zip(a.opt._groups, b.opt._groups):
        assert torch.equal(ga.m, gb.m) and torch.equal(ga.v, gb.v), what
    assert a.opt.device_step_count() == b.opt.device_step_count(), what
    assert torch.equal(a.reg.offset, b.reg.offset) and torch.equal(a.out, out_b), what


def test_solo_device_forms_equal_the_plain_fit(dev):
    from dip_optim import GraphedIteration, NativeIteration
    plain, eager, native, graphed = _dev_fit(dev, False), _dev_fit(dev), _dev_fit(dev), _dev_fit(dev)
    # plain: the values are launch arguments; changed at the boundary
    lp = [_eager_step(plain) for _ in range(2)]
    plain.opt.lr, plain.reg.std = 1e-3, 0.05
    lp += [_eager_step(plain) for _ in range(2)]
    # eager, on the device scalars
    le = [_eager_step(eager) for _ in range(2)]
    eager.opt.set_lr(1e-3)
    eager.reg.set_std(0.05)
    le += [_eager_step(eager) for _ in range(2)]
    assert torch.equal(torch.stack(lp), torch.stack(le))
    _assert_same_state(plain, eager, plain.out, eager.out, "eager device forms")
    assert eager.opt.lr == 1e-3 and eager.reg.std == 0.05
    assert eager.opt._lr_scalar(eager.z.device).item() == 1e-3 and eager.reg.std_dev.item() == torch.tensor(0.05).float().item()
    # NativeIteration: the plan survives the setters
    it = NativeIteration(native.net, native.head, native.opt, native.z, reg_noise=native.reg)
    ln = list(it.run(2).unbind(0))
    plan, key = it._plan, it._key
    native.opt.set_lr(1e-3)
    native.reg.set_std(0.05)
    ln += list(it.run(2).unbind(0))
    assert it._plan is plan and it._key == key and len(key) == 11
    names = [n for cl in it._plan["lists"].phases for n in cl.names]
    assert names[0] == "noise_axpy_dev1s" and it._plan["lists"].phases[-1].names == ["adam_tick_dev", "adam_step_dev"]
    assert torch.equal(torch.stack(lp), torch.stack(ln))
    _assert_same_state(plain, native, plain.out, it.out, "native device forms")
    # GraphedIteration: one eager warm-up iteration, one replay, the setters, two replays of the same graph
    def closure():
        loss, out = graphed.head(graphed.reg())
        loss.backward()
        graphed.out = out
        return loss

    gi = GraphedIteration(graphed.opt, closure, warmup=1)
    graph = gi.graph
    gi.run(1)
    graphed.opt.set_lr(1e-3)
    graphed.reg.set_std(0.05)
    gi.run(2)
    assert gi.graph is graph and gi.iterations == 4
    _same_fit(plain, graphed, graphed.out, "graphed device forms")
    # annealed to 0 and back without leaving the noise path: out = saved + 0 * N, and the stream goes on
    off = int(eager.reg.offset.item())
    eager.reg.set_std(0.0)
    x = eager.reg()
    assert x is eager.reg.out and torch.equal(eager.reg.out, eager.reg.saved)
    assert int(eager.reg.offset.item()) == off + (eager.reg.saved.numel() + 3) // 4
    eager.reg.set_std(0.05)
    assert not torch.equal(eager.reg(), eager.reg.saved)
    # an optimiser / RegNoise built without the keywords refuses the setters and names them
    with pytest.raises(RuntimeError, match="dip-amd:.*device_lr=True"):
        plain.opt.set_lr(0.1)
    with pytest.raises(RuntimeError, match="dip-amd:.*device_std=True"):
        plain.reg.set_std(0.1)
    for bad in (float("nan"), -1.0):
        with pytest.raises(ValueError, match="dip-amd:"):
            eager.opt.set_lr(bad)
        with pytest.raises(ValueError, match="dip-amd:"):
            eager.reg.set_std(bad)


# ------------------------------------------------------------------------------------------ defaults untouched
def test_defaults_issue_the_parent_launches(dev, monkeypatch):
    """Floats and default keywords: the grouped iteration and NativeIteration's phases name adam_tick and noise_axpy_dev[2];
    no device-scalar entry point appears; the plan key has the length it had."""
    from dip_group import GroupedFits
    from dip_optim import NativeIteration
    zs, ts, ms = _problem("skip3", HW, B, 1, dev)
    g = GroupedFits(_group_nets(dev, B), zs, ts, masks=ms, seeds=SEEDS, lr=0.01, reg_noise_std=1. / 30.)
    assert not any(k in g._row0_extra for k in ("lr", "reg_std")) and g.lr == 0.01 and g.std == 1. / 30.
    seen, real = [], N.check

    def check(rc, what=""):
        seen.append(what)
        return real(rc, what)

    monkeypatch.setattr(N, "check", check)
    g.step(1)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert seen.count("adam_tick") == 1 and seen.count("noise_axpy_dev2") == 1 and not any(n in seen for n in NEW)
    with pytest.raises(ValueError, match="construct the group with a list"):
        g.set_lr([0.1] * B)
    # the same group with lists: the two device-scalar launches in their places, everything else the same
    gl = GroupedFits(_group_nets(dev, B), zs, ts, masks=ms, seeds=SEEDS, lr=[0.01] * B, reg_noise_std=[1. / 30.] * B)
    listed = []
    monkeypatch.setattr(N, "check", lambda rc, what="": (listed.append(what), real(rc, what))[1])
    gl.step(1)
    monkeypatch.undo()
    torch.cuda.synchronize()
    swap = {"adam_tick_dev": "adam_tick", "noise_axpy_dev3": "noise_axpy_dev2"}
    assert [swap.get(n, n) for n in listed] == seen and listed.count("adam_tick_dev") == 1 == listed.count("noise_axpy_dev3")
    assert gl.stride == g.stride + 512 and torch.equal(gl.losses, g.losses)           # one common value: the same fits
    # NativeIteration with defaults
    f = _mse_fit(dev, sgld=False)
    it = NativeIteration(f.net, f.head, f.opt, f.z, reg_noise=f.reg)
    it.run(1)
    names = [n for cl in it._plan["lists"].phases for n in cl.names]
    assert names[0] == "noise_axpy_dev" and it._plan["lists"].phases[-1].names == ["adam_tick", "adam_step_dev"]
    assert not any(n in names for n in NEW)
    assert len(it._key) == 11 and it._key[5] == 0.01 and it._key[-1][0] == 1. / 30.   # the VALUES of lr and std, where they stood
    assert f.reg.std_dev is None and f.opt._lr_dev == {}
    s = _mse_fit(dev)                                                                 # an SGLD optimiser: 13, without monitors
    its = NativeIteration(s.net, s.head, s.opt, s.z, reg_noise=s.reg)
    its.run(1)
    assert len(its._key) == 13 and its._plan["lists"].phases[-1].names == ["adam_tick", "adam_sgld_step_dev"]


# ------------------------------------------------------------------------------------------ composition
def test_lists_compose_with_early_stop_and_ssim(dev):
    """One group with lists for both knobs, early_stop=GroupedEarlyStopMonitor(mode='emv') and ssim=: fits and records are the
    solo NativeIteration(early_stop=, ssim=) fits'."""
    from dip_group import GroupedFits
    from utils.fit_monitor import EarlyStopMonitor, GroupedEarlyStopMonitor, GroupedSSIMMonitor, SSIMMonitor
    from utils.loss_head import MSEHead
    emv, cap = dict(alpha=0.25, warmup=3, patience=4), 16
    zs, ts, _ = _problem("skip3", HW, B, 0, dev)
    gen = torch.Generator().manual_seed(5)
    gts = [torch.rand(1, 3, *HW, generator=gen).to(dev) for _ in range(B)]
    nets = _group_nets(dev, B)
    refs = [copy.deepcopy(n) for n in nets]
    solo = []
    for b in range(B):
        es = EarlyStopMonitor(torch.empty(1, 3, *HW, device=dev), net=refs[b], capacity=cap, mode="emv", **emv)
        solo.append(_Solo(refs[b], zs[b], MSEHead(refs[b], ts[b]), LRS[b], STDS[b], SEEDS[b], early_stop=es,
                          ssim=SSIMMonitor(gts[b], capacity=cap)))
    ges, gsm = GroupedEarlyStopMonitor(mode="emv", capacity=cap, **emv), GroupedSSIMMonitor(gts, capacity=cap)
    g = GroupedFits(nets, zs, ts, seeds=SEEDS, lr=LRS, reg_noise_std=STDS, early_stop=ges, ssim=gsm)
    assert g.pointers_outside_row0() == []
    keys = list(g._row0_extra)
    assert keys[-2:] == ["lr", "reg_std"] and keys.index("lr") > max(i for i, k in enumerate(keys) if k.startswith(("es_", "ssim_")))
    hist = []
    _group_history(g, g.step, 2, hist)
    g.capture(warmup=1)
    hist.append(g.losses.clone())
    _group_history(g, g.run, 7, hist)
    for s in solo:
        s.run(10)
    _assert_group_equals_solo(g, nets, solo, hist)
    assert ges.i == gsm.i == 10 and ges.counter.tolist() == [10] * B
    for b, s in enumerate(solo):
        assert torch.equal(ges.records[b].view(torch.int32), s.es.records.view(torch.int32)), b
        assert torch.equal(ges.state[b], s.es.state) and torch.equal(ges.mean[b], s.es.mean), b
        assert torch.equal(ges.best_out[b:b + 1], s.es.best_out) and torch.equal(ges.best_params[b], s.es.best_params), b
        assert torch.equal(gsm.records[b].view(torch.int32), s.sm.records.view(torch.int32)), b
    assert ges.best_iter == [s.es.best_iter for s in solo] and ges.stopped == [s.es.stopped for s in solo]
