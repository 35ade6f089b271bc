"""SSIM on a real MI355X: dip_ssim_dev (csrc/ssim_kernels.hip) against the fp64 evaluation of tests/ssim_ref.py at sizes chosen
against the 16 x 64 tile, held to the per-op criterion of test_kernels_gpu._check; exactness for out == gt, guard bands, equal
bits of two runs, the capacity guard, the grouped dispatch against solo calls; utils.fit_monitor.SSIMMonitor eager and under
NativeIteration(ssim=) with either head and next to a FitMonitor; GroupedFits(ssim=) against its solo fits, eager and as ONE
hipGraph, for the group kinds.  Every fit comparison is torch.equal."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dip_native as N  # noqa: E402
import ssim_ref as R  # noqa: E402
from test_group_gpu import _net, _problem  # noqa: E402
from test_group_monitor_gpu import _stream_pool_stands_where_it_stood, native_mask  # noqa: E402,F401  (autouse: the engines
#                                           of this module draw pooled streams; the pool is left where it stood)
from test_kernels_gpu import _check  # noqa: E402
from test_native_iter_gpu import _assert_same_state  # noqa: E402
from test_native_monitor_gpu import _assert_same_monitor, _monitor  # noqa: E402
from test_sgld_fit_gpu import _mse_fit, _native  # noqa: E402
from test_sr_head_gpu import GUARD, SENTINEL, _guard_ok, _guarded, _sr_fit  # noqa: E402

TH, TW = 16, 64                                   # the kernel's tile of valid outputs
SIZES = {"one-pixel": (11, 11), "row-over-a-column-tile-edge": (11, TW + 11), "column-over-a-row-tile-edge": (TH + 11, 11),
         "one-tile": (TH + 10, TW + 10), "tile-plus-one": (TH + 11, TW + 11), "ragged": (33, 129)}
KINDS = ("noisy", "flat", "constants")
_REF = {}


def _ref(Cn, H, W, kind):
    """(out, gt, fp64 map, torch-fp32 map) of one case, computed once and shared (nothing modifies it)."""
    key = (Cn, H, W, kind)
    if key not in _REF:
        out, gt = R.inputs(Cn, H, W, kind)
        _REF[key] = (out, gt, R.ssim_map(out, gt), R.ssim_map(out, gt, torch.float32))
    return _REF[key]


# ------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("Cn", [1, 3, 4])
@pytest.mark.parametrize("size", list(SIZES))
def test_kernel_against_the_fp64_definition(dev, size, Cn):
    from utils.fit_monitor import ssim
    H, W = SIZES[size]
    assert N.lib().dip_ssim_nblk(Cn, H, W) == Cn * -(-(H - 10) // TH) * -(-(W - 10) // TW)
    for kind in KINDS:
        out, gt, m64, m32 = _ref(Cn, H, W, kind)
        val, smap = ssim(out.to(dev), gt.to(dev), full=True)
        assert tuple(smap.shape) == (1, Cn, H - 10, W - 10) and val.dim() == 0
        e, e32 = (smap.cpu().double() - m64).abs().max().item(), (m32.double() - m64).abs().max().item()
        print(f"{size} C{Cn} {kind}: map err / torch-fp32 err {e / max(e32, 1e-30):.3f}")
        _check(f"ssim map {size} C{Cn} {kind}", smap, m64, m32)
        _check(f"ssim mean {size} C{Cn} {kind}", val.reshape(1), m64.mean().reshape(1), m32.mean().reshape(1))
    # out == gt: every factor pair is the same bits
    _, gt, _, _ = _ref(Cn, H, W, "noisy")
    val, smap = ssim(gt.to(dev), gt.to(dev).clone(), full=True)
    assert torch.equal(smap, torch.ones_like(smap)) and val.item() == 1.0


def _desc(t, Cn, H, W, capacity, data_range=1.0):
    from utils.fit_monitor import ssim_descriptor
    from types import SimpleNamespace
    m = SimpleNamespace(chw=(Cn, H, W), data_range=data_range, with_avg="avg" in t, capacity=capacity)
    return ssim_descriptor(m, t)


@pytest.mark.parametrize("Cn,H,W", [(3, 33, 129), (1, 11, 11)])
def test_guards_determinism_capacity_and_the_second_source(dev, Cn, H, W):
    from utils.fit_monitor import ssim
    L = N.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    out, gt, m64, _ = _ref(Cn, H, W, "noisy")
    avg = (0.5 * (out + gt)).to(dev)
    out, gt = out.to(dev), gt.to(dev)
    nblk, cap, nmap = L.dip_ssim_nblk(Cn, H, W), 3, Cn * (H - 10) * (W - 10)
    runs = []
    for _ in range(2):
        bufs = {k: _guarded(n, dev) for k, n in (("map", nmap), ("partial", 2 * nblk), ("records", 2 * cap))}
        counter = torch.ones(1, dtype=torch.int32, device=dev)                # row 1
        t = dict(out=out, gt=gt, avg=avg, counter=counter, **{k: v[1] for k, v in bufs.items()})
        N.check(L.dip_ssim_dev(C.byref(_desc(t, Cn, H, W, cap)), st), "ssim_dev")
        torch.cuda.synchronize()
        assert all(_guard_ok(b) for b, _ in bufs.values())
        rec = bufs["records"][1].view(cap, 2)
        assert counter.item() == 2 and bool((rec[0] == SENTINEL).all()) and bool((rec[2] == SENTINEL).all())
        assert bool((bufs["map"][1] != SENTINEL).all()) and bool((bufs["partial"][1] != SENTINEL).all())
        runs.append({k: v[1].clone() for k, v in bufs.items()})
    for k in runs[0]:                                                         # two runs: the same bits
        assert torch.equal(runs[0][k].view(torch.int32), runs[1][k].view(torch.int32)), k
    rec = runs[0]["records"].view(cap, 2)[1]
    assert abs(rec[0].item() - m64.mean().item()) < 2e-6
    assert rec[0].item() == ssim(out, gt).item() and rec[1].item() == ssim(avg, gt).item()      # the functional form
    assert torch.equal(runs[0]["map"].view(1, Cn, H - 10, W - 10), ssim(out, gt, full=True)[1])
    # without avg and map: ssim_sm is 0, one row of partials is written
    bufs = {k: _guarded(n, dev) for k, n in (("partial", 2 * nblk), ("records", 2 * cap))}
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    t = dict(out=out, gt=gt, counter=counter, **{k: v[1] for k, v in bufs.items()})
    N.check(L.dip_ssim_dev(C.byref(_desc(t, Cn, H, W, cap)), st), "ssim_dev")
    torch.cuda.synchronize()
    assert bufs["records"][1][:2].tolist() == [rec[0].item(), 0.0] and bool((bufs["partial"][1][nblk:] == SENTINEL).all())
    # a counter outside the capacity: nothing is written at all
    for it in (cap, -1):
        bufs = {k: _guarded(n, dev) for k, n in (("map", nmap), ("partial", 2 * nblk), ("records", 2 * cap))}
        counter = torch.full((1,), it, dtype=torch.int32, device=dev)
        t = dict(out=out, gt=gt, avg=avg, counter=counter, **{k: v[1] for k, v in bufs.items()})
        N.check(L.dip_ssim_dev(C.byref(_desc(t, Cn, H, W, cap)), st), "ssim_dev")
        torch.cuda.synchronize()
        assert counter.item() == it and all(bool((b == SENTINEL).all()) for b, _ in bufs.values()), it


def test_data_range(dev):
    from utils.fit_monitor import ssim
    out, gt, _, _ = _ref(3, 33, 129, "noisy")
    dr = 4.0                                                                  # a power of two: the scaled problem is the same bits
    a, b = ssim(out.to(dev), gt.to(dev), full=True), ssim((out * dr).to(dev), (gt * dr).to(dev), data_range=dr, full=True)
    assert torch.equal(a[1], b[1]) and a[0].item() == b[0].item()


@pytest.mark.parametrize("mask", [0x7fffffff, 0], ids=["one-dispatch", "host-loop"])
def test_grouped_kernels_equal_solo_calls(dev, native_mask, mask):
    """Three rows of a hand-built [B][stride] slab through ONE dip_ssim_dev call inside the group bracket against three solo
    calls: records, counters and partials, bit for bit; guard bands between the buffers stay untouched."""
    L, B, (Cn, H, W), cap = native_mask, 3, (3, 33, 129), 4
    st = torch.cuda.current_stream(dev).cuda_stream
    n, nblk = Cn * H * W, L.dip_ssim_nblk(Cn, H, W)
    off, o = {}, GUARD
    for k, sz in (("out", n), ("avg", n), ("gt", n), ("partial", 2 * nblk), ("records", 2 * cap), ("counter", 1)):
        off[k] = (o, sz)
        o = (o + sz + GUARD + 63) // 64 * 64
    stride = o
    slab = torch.full((B, stride), SENTINEL, dtype=torch.float32, device=dev)
    get = lambda b, k: slab[b, off[k][0]:off[k][0] + off[k][1]]
    solo = []
    for b in range(B):
        out, gt = R.inputs(Cn, H, W, "noisy", seed=b + 1)
        get(b, "out").copy_(out.reshape(-1))
        get(b, "gt").copy_(gt.reshape(-1))
        get(b, "avg").copy_((0.5 * (out + gt)).reshape(-1))
        get(b, "counter").view(torch.int32).fill_(b)                          # every instance at its own row
        t = {k: get(b, k).clone() for k in off}
        t["counter"] = t["counter"].view(torch.int32)
        N.check(L.dip_ssim_dev(C.byref(_desc(t, Cn, H, W, cap)), st), "ssim_dev")
        solo.append(t)
    L.dip_group_native(mask)
    t0 = {k: get(0, k) for k in off}
    t0["counter"] = t0["counter"].view(torch.int32)
    N.check(L.dip_group_begin(B, 4 * stride, slab.data_ptr(), 4 * stride), "group_begin")
    try:
        N.check(L.dip_ssim_dev(C.byref(_desc(t0, Cn, H, W, cap)), st), "ssim_dev")
    finally:
        L.dip_group_end()
    torch.cuda.synchronize()
    keep = torch.ones(stride, dtype=torch.bool, device=dev)
    for lo, sz in off.values():
        keep[lo:lo + sz] = False
    assert bool((slab[:, keep] == SENTINEL).all())
    for b in range(B):
        for k in ("partial", "records", "counter"):
            assert torch.equal(get(b, k).view(torch.int32), solo[b][k].view(torch.int32)), (b, k)
        assert get(b, "counter").view(torch.int32).item() == b + 1
        assert bool((get(b, "records").view(cap, 2)[b] != SENTINEL).all())
    assert len({get(b, "records").view(cap, 2)[b, 0].item() for b in range(B)}) == B


# ------------------------------------------------------------------------------------------ 2. one fit
def _sm(f, shape=None, avg=None, capacity=16, seed=21, **kw):
    from utils.fit_monitor import SSIMMonitor
    dev = f.z.device
    gt = torch.rand(shape or f.target.shape, generator=torch.Generator().manual_seed(seed)).to(dev)
    return SSIMMonitor(gt, img_avg=avg, capacity=capacity, **kw)


def _eager_ssim_step(f, sm, mon=None):
    """test_native_iter_gpu._eager_step with the monitors' updates between backward() and opt.step(), in NativeIteration's
    order: monitor, then ssim."""
    f.opt.zero_grad()
    loss, out = f.head(f.reg())
    loss.backward()
    if mon is not None:
        mon.update(out, loss)
    sm.update(out)
    f.opt.step()
    f.out = out
    return loss.detach()


def _same_sm(a, b, what=""):
    torch.cuda.synchronize()
    assert a.i == b.i, what
    assert torch.equal(a.records.view(torch.int32), b.records.view(torch.int32)), (what, a.history().tolist(), b.history().tolist())
    assert torch.equal(a.counter, b.counter) and a.counter.item() == a.i, what
    assert (a.map is None) == (b.map is None), what
    if a.map is not None:
        assert torch.equal(a.map, b.map), what


def test_native_iteration_equals_the_eager_update_and_leaves_the_fit_alone(dev, monkeypatch):
    from utils.fit_monitor import ssim
    a, b, c, d = (_mse_fit(dev, sgld=False) for _ in range(4))
    sa, sb, sc = (_sm(f, keep_map=True) for f in (a, b, c))
    la = [_eager_ssim_step(a, sa) for _ in range(7)]
    itb = _native(b, ssim=sb)
    lb = torch.cat([itb.step().reshape(1) for _ in range(2)] + [itb.run(5)])
    assert itb._plan["lists"].phases[-2].names == ["ssim_dev"]                # behind the backward list, in front of Adam
    assert torch.equal(torch.stack(la), lb)
    _same_sm(sa, sb)
    _assert_same_state(a, b, a.out, itb.out)
    h = sa.history()
    assert h.shape == (7, 2) and np.all(h[:, 0] > -1) and np.all(h[:, 0] < 1) and not h[:, 1].any() and len(set(h[:, 0])) == 7
    assert sa.last() == dict(ssim=float(h[-1, 0]), ssim_sm=0.0)
    # the record and the map are the one-shot function's for the same tensors
    val, smap = ssim(itb.out, sb.gt, full=True)
    assert val.item() == h[-1, 0] and torch.equal(smap, sb.map) and tuple(sb.map.shape) == (1, 3, 26, 42)
    # alternating eager and native on one monitor
    itc = _native(c, ssim=sc)
    lc = list(itc.run(3)) + [_eager_ssim_step(c, sc), _eager_ssim_step(c, sc)] + [itc.step(), itc.step()]
    assert torch.equal(torch.stack(la), torch.stack(lc))
    _same_sm(sa, sc, "alternating")
    _assert_same_state(a, c, a.out, itc.out, "alternating")
    # ssim=None: the same fit, and the key it had
    itd = _native(d)
    ld = itd.run(7)
    assert torch.equal(ld, lb)
    _assert_same_state(b, d, itb.out, itd.out, "ssim=None")
    assert len(itb._key) == len(itd._key) + 1 and itb._key[-1] == ("ssim", sb._plan_key())
    assert not any(isinstance(k, tuple) and k[:1] == ("ssim",) for k in itd._key)
    # refused before anything is issued: the capacity, another shape, a CPU output, capture of update()
    small = _sm(b, capacity=2)
    itb.ssim = small
    with pytest.raises(RuntimeError, match="dip-amd: SSIMMonitor capacity exceeded"):
        itb.run(3)
    itb.ssim = _sm(b, shape=(1, 3, 36, 53))
    with pytest.raises(ValueError, match="dip-amd: NativeIteration: the SSIMMonitor's img_gt is"):
        itb.step()
    with pytest.raises(ValueError, match="dip-amd: SSIMMonitor.update: the SSIMMonitor's img_gt is"):
        small.update(torch.zeros(1, 3, 36, 53, device=dev))
    with pytest.raises(RuntimeError, match="dip-amd: SSIMMonitor.update: the output is on cpu"):
        small.update(torch.zeros(1, 3, 36, 52))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="dip-amd: SSIMMonitor.update cannot be captured"):
        small.update(itb.out)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert small.i == 0 and small.counter.item() == 0 and b.opt.step_count == 7


def test_combines_with_a_fit_monitor_and_its_smoothed_output(dev):
    from utils.fit_monitor import ssim
    a, b = _mse_fit(dev, sgld=False), _mse_fit(dev, sgld=False)
    ma, mb = _monitor(a), _monitor(b)
    sa, sb = _sm(a, avg=ma.out_avg), _sm(b, avg=mb.out_avg)
    la = [_eager_ssim_step(a, sa, ma) for _ in range(6)]
    it = _native(b, monitor=mb, ssim=sb)
    lb = it.run(6)
    assert [ph.names[0] for ph in it._plan["lists"].phases[-3:]] == ["fit_monitor_dev", "ssim_dev", "adam_tick"]
    assert torch.equal(torch.stack(la), lb)
    _same_sm(sa, sb)
    _assert_same_monitor(ma, mb)
    _assert_same_state(a, b, a.out, it.out)
    last = sb.last()
    assert last["ssim_sm"] == ssim(mb.out_avg, sb.gt).item() and last["ssim"] == ssim(it.out, sb.gt).item()
    assert last["ssim_sm"] != last["ssim"] and last["ssim_sm"] != 0.0


def test_with_an_sr_head(dev):
    from utils.fit_monitor import ssim
    a, b, c = (_sr_fit(dev, noisy=True) for _ in range(3))                    # 64 x 96 outputs, 16 x 24 LR images
    sa, sb = _sm(a, shape=(1, 3, 64, 96)), _sm(b, shape=(1, 3, 64, 96))       # gt is img_HR
    la = [_eager_ssim_step(a, sa) for _ in range(4)]
    it = _native(b, ssim=sb)
    lb = it.run(4)
    assert torch.equal(torch.stack(la), lb)
    _same_sm(sa, sb)
    _assert_same_state(a, b, a.out, it.out)
    assert sb.last()["ssim"] == ssim(it.out, sb.gt).item()
    itc = _native(c)
    assert torch.equal(itc.run(4), lb)
    _assert_same_state(b, c, it.out, itc.out, "ssim=None")


# ------------------------------------------------------------------------------------------ 3. B fits through one launch list
B, HW, STD = 3, (32, 48), 1. / 30.


class _Solo:
    """The fit on its own: RegNoise + MSEHead (masked or not) or SRHead [+ FitMonitor] + FusedAdam + NativeIteration(ssim=
    SSIMMonitor)."""

    def __init__(self, net, z, img, mask, down, gt_mon, gt, seed, capacity):
        from dip_optim import FusedAdam, NativeIteration
        from utils.common_utils import get_params
        from utils.fit_monitor import FitMonitor, SSIMMonitor
        from utils.loss_head import MSEHead, SRHead
        from utils.reg_noise import RegNoise
        self.net, self.reg = net, RegNoise(z, STD, seed=seed)
        self.head = MSEHead(net, img, mask=mask) if down is None else SRHead(net, img, down)
        self.opt = FusedAdam(get_params("net", net, z), lr=0.01)
        self.mon = FitMonitor(net, img, gt_mon, show_every=5, capacity=capacity) if gt_mon is not None else None
        self.sm = SSIMMonitor(gt, img_avg=None if self.mon is None else self.mon.out_avg, capacity=capacity)
        self.it = NativeIteration(net, self.head, self.opt, z, reg_noise=self.reg, monitor=self.mon, ssim=self.sm)
        self.loss = None

    def run(self, n):
        self.loss = self.it.run(n)[-1]


def _build(dev, case, capacity=16, with_ssim=True):
    """(group, its SSIM monitor, its nets, the ground truths) of a case: 'plain', 'monitor', 'masked' or 'sr'."""
    from dip_group import GroupedFits
    from models.downsampler import Downsampler
    from utils.fit_monitor import GroupedFitMonitor, GroupedSSIMMonitor
    zs, ts, ms = _problem("skip3", HW, B, 1 if case == "masked" else 0, dev)
    gen = torch.Generator().manual_seed(5)
    gts = [torch.rand(1, 3, *HW, generator=gen).to(dev) for _ in range(B)]
    gts_mon = [torch.rand(1, 3, *HW, generator=gen).to(dev) for _ in range(B)] if case == "monitor" else None
    downs = None
    if case == "sr":
        downs = [Downsampler(n_planes=3, factor=2, kernel_type="lanczos2", phase=0.5, preserve_size=True).to(dev)
                 for _ in range(B)]
        ts = [t[:, :, :HW[0] // 2, :HW[1] // 2].contiguous() for t in ts]              # the LR images
    nets = [_net("skip3", 10 + b).to(dev) for b in range(B)]
    refs = [copy.deepcopy(x) for x in nets]           # (the solo twins: copies taken before the group adopts the nets)
    mon = GroupedFitMonitor(gts_mon, show_every=5, capacity=capacity) if case == "monitor" else None
    sm = GroupedSSIMMonitor(gts, with_avg=case == "monitor", capacity=capacity) if with_ssim else None
    g = GroupedFits(nets, zs, ts, masks=ms, downsamplers=downs, reg_noise_std=STD, seeds=[40 + b for b in range(B)], lr=0.01,
                    monitor=mon, ssim=sm)
    assert g.pointers_outside_row0() == []
    return g, sm, nets, (refs, zs, ts, ms, downs, gts_mon, gts)


def _assert_same_group(g, sm, nets, solo, what):
    torch.cuda.synchronize()
    assert g.iterations == sm.i and sm.counter.tolist() == [sm.i] * B, what
    hist = sm.history()
    assert hist.shape == (B, sm.i, 2), what
    for b, s in enumerate(solo):
        w = (what, b)
        assert s.sm.i == sm.i, w
        assert torch.equal(sm.records[b].view(torch.int32), s.sm.records.view(torch.int32)), (w, hist[b].tolist(), s.sm.history().tolist())
        assert g.losses[b].item() == s.loss.item() and torch.equal(g.out[b:b + 1], s.it.out), w
        assert sm.last()[b] == s.sm.last(), w
        for (k, pa), pb in zip(nets[b].named_parameters(), s.net.parameters()):
            assert torch.equal(pa, pb), (w, k)
        if s.mon is not None:
            assert torch.equal(g.monitor.records[b], s.mon.records) and torch.equal(g.monitor.out_avg[b:b + 1], s.mon.out_avg), w


@pytest.mark.parametrize("case", ["plain", "monitor", "masked", "sr"],
                         ids=["denoising", "denoising-monitor-avg", "masked", "super-resolution"])
def test_group_with_ssim_bitwise_equals_solo_fits(dev, case):
    g, sm, nets, (refs, zs, ts, ms, downs, gts_mon, gts) = _build(dev, case)
    assert [name for _, _, name in g._ssim] == ["ssim_dev"] and sm.group is g
    solo = [_Solo(refs[b], zs[b], ts[b], None if ms is None else ms[b], None if downs is None else downs[b],
                  None if gts_mon is None else gts_mon[b], gts[b], 40 + b, 16) for b in range(B)]

    def both(n, run):
        run(n)
        for s in solo:
            s.run(n)

    both(2, g.step)
    g.capture(warmup=1)                               # the third eager iteration, then ONE hipGraph with the ssim launch
    for s in solo:
        s.run(1)
    _assert_same_group(g, sm, nets, solo, "after 3 eager")
    both(5, g.run)
    _assert_same_group(g, sm, nets, solo, "after 8")
    h = sm.history()
    assert np.all(np.abs(h[:, :, 0]) < 1) and len({float(x) for x in h[:, -1, 0]}) == B
    assert bool(h[:, :, 1].any()) == (case == "monitor")
    # the same group without ssim=: the same losses, outputs and parameters
    g0, _, nets0, _ = _build(dev, case, with_ssim=False)
    assert g0.ssim is None and g0.stride < g.stride and not hasattr(g0, "_sdesc")
    g0.step(2)
    g0.capture(warmup=1)
    g0.run(5)
    torch.cuda.synchronize()
    assert torch.equal(g0.losses, g.losses) and torch.equal(g0.out, g.out)
    for b in range(B):
        for (k, pa), pb in zip(nets[b].named_parameters(), nets0[b].parameters()):
            assert torch.equal(pa, pb), (b, k)
    with pytest.raises(RuntimeError, match="dip-amd: Grouped(Fit|SSIM)Monitor capacity exceeded"):
        g.run(9)
