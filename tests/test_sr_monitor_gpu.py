"""The super-resolution monitor on a real MI355X (utils.fit_monitor.SRFitMonitor / GroupedSRFitMonitor; dip_sr_monitor,
dip_sr_monitor_dev): the psnr_LR / psnr_HR record of the closure of super-resolution.ipynb:169-191 of the reference

    psnr_LR = compare_psnr(imgs['LR_np'], torch_to_np(out_LR)); psnr_HR = compare_psnr(imgs['HR_np'], torch_to_np(out_HR))

1. the kernels against the oracle's psnr() (2e-4 dB, the figure of tests/test_monitor_gpu.py for the existing monitor);
2. NativeIteration(SRHead, monitor=SRFitMonitor) against the eager closure with update() -- bit for bit;
3. the monitor does not touch the fit -- bit for bit against monitor=None;
4. GroupedFits(downsamplers=, monitor=GroupedSRFitMonitor) against the solo fits, eager and as ONE hipGraph -- bit for bit;
5. every refusal is raised before anything is issued."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_group_gpu import ALL, _net, native_mask  # noqa: E402,F401
from test_group_monitor_gpu import _stream_pool_stands_where_it_stood  # noqa: E402,F401  (autouse: the engines and the
#                                      captured groups of this module draw pooled streams; the pool is left where it stood)
from test_group_sr_gpu import _down, _lr_size  # noqa: E402
from test_native_iter_gpu import _assert_same_state, _eager_step  # noqa: E402
from test_sr_head_gpu import _native, _sr_fit  # noqa: E402

TOL_DB = 2e-4
SIGMAS = (0.3, 0.05, 0.002)          # 12 .. 54 dB
HW, F, LR = (32, 48), 4, (8, 12)     # the fits: HR 32 x 48, lanczos2 factor 4, LR 8 x 12


def _oracle():
    import dip_oracle as O
    return O


# ------------------------------------------------------------------------------------------ 1. kernels against the oracle
# (HR shape, LR shape)
KERNEL_SHAPES = [
    ((3, 32, 48), (3, 8, 12)),          # 5 HR blocks, the last one partial (4608 = 4.5 x 1024), one partial LR block
    ((1, 20, 12), (1, 5, 3)),           # fewer elements than one block (240), and LR far fewer (15)
    ((3, 592, 592), (3, 148, 148)),     # 1 051 392 > 1024 x 1024 elements: the block count saturates, the walk takes another trip
]
KERNEL_IDS = ["hr32x48-lr8x12", "hr20x12-lr5x3", "hr592-lr148-wraps"]
_INPUTS = {}


def _inputs(k):
    """gt = rand, out = clip(gt + N(0, s)) for s in SIGMAS, at both sizes (drawn once per shape, never modified)."""
    if k not in _INPUTS:
        rng = np.random.RandomState(100 + k)
        hr_shape, lr_shape = KERNEL_SHAPES[k]
        gt_hr, gt_lr = rng.rand(*hr_shape).astype(np.float32), rng.rand(*lr_shape).astype(np.float32)
        outs = [(np.clip(gt_hr + rng.normal(scale=s, size=hr_shape), 0, 1).astype(np.float32),
                 np.clip(gt_lr + rng.normal(scale=s, size=lr_shape), 0, 1).astype(np.float32)) for s in SIGMAS]
        _INPUTS[k] = (gt_hr, gt_lr, outs)
    return _INPUTS[k]


def _t(a, dev):
    return torch.from_numpy(a)[None].to(dev)


@pytest.mark.parametrize("with_hr", [True, False], ids=["img_HR", "no-HR"])
@pytest.mark.parametrize("k", range(len(KERNEL_SHAPES)), ids=KERNEL_IDS)
def test_update_matches_the_oracle_psnr(dev, built, k, with_hr):
    from utils.fit_monitor import SRFitMonitor
    O = _oracle()
    gt_hr, gt_lr, outs = _inputs(k)
    n_hr, n_lr = gt_hr.size, gt_lr.size
    assert built.dip_fit_monitor_nblk(n_hr) == min((n_hr + 1023) // 1024, 1024)
    assert (k == 2) == (n_hr > 1024 * 1024)
    mons = [SRFitMonitor(_t(gt_lr, dev), _t(gt_hr, dev) if with_hr else None, capacity=4) for _ in range(2)]
    for mon in mons:                                            # the same inputs twice: bit-equal rows
        for i, (o_hr, o_lr) in enumerate(outs):
            loss = torch.tensor(0.5 + i, device=dev)
            mon.update(_t(o_hr, dev), _t(o_lr, dev), loss if i != 1 else None)
            assert mon.i == i + 1
    torch.cuda.synchronize()
    hist = mons[0].history()
    assert hist.shape == (3, 5) and hist.dtype == np.float32
    assert torch.equal(mons[0].records, mons[1].records)
    assert torch.count_nonzero(mons[0].records[3]).item() == 0 and mons[0].counter.item() == 0      # update() leaves both alone
    for i, (o_hr, o_lr) in enumerate(outs):                     # update i landed in row i
        loss, mse_lr, mse_hr, psnr_lr, psnr_hr = (float(x) for x in hist[i])
        want_lr, want_hr = O.psnr(gt_lr, o_lr), O.psnr(gt_hr, o_hr)
        print(f"{KERNEL_IDS[k]} s={SIGMAS[i]}: psnr_LR {psnr_lr:.6f} (oracle {want_lr:.6f}), psnr_HR {psnr_hr:.6f} "
              f"(oracle {want_hr:.6f})")
        assert loss == (0.5 + i if i != 1 else 0.0)             # passed through; None -> 0
        assert psnr_lr == pytest.approx(want_lr, abs=TOL_DB), (i, "psnr_LR")
        assert mse_lr == pytest.approx(np.mean((gt_lr.astype(np.float64) - o_lr) ** 2), rel=1e-5), (i, "mse_LR")
        if with_hr:
            assert psnr_hr == pytest.approx(want_hr, abs=TOL_DB), (i, "psnr_HR")
            assert mse_hr == pytest.approx(np.mean((gt_hr.astype(np.float64) - o_hr) ** 2), rel=1e-5), (i, "mse_HR")
            if k < 2:                                           # two small draws differ: swapped columns would show
                assert abs(want_hr - want_lr) > 10 * TOL_DB
        else:
            assert mse_hr == 0.0 and psnr_hr == 0.0
    last = mons[0].last()
    assert tuple(last) == SRFitMonitor.COLUMNS and last["psnr_LR"] == float(hist[2, 3])


def test_dev_kernels_equal_update_and_guard_the_capacity(dev, built):
    """dip_sr_monitor_dev at counter = i writes row i exactly as update() does and advances the counter; a counter outside
    [0, capacity) writes nothing."""
    import ctypes
    import dip_native as N
    from utils.fit_monitor import SRFitMonitor
    gt_hr, gt_lr, outs = _inputs(0)
    cap = 4
    ref = SRFitMonitor(_t(gt_lr, dev), _t(gt_hr, dev), capacity=cap)
    mon = SRFitMonitor(_t(gt_lr, dev), _t(gt_hr, dev), capacity=cap)
    o_hr, o_lr = _t(outs[1][0], dev), _t(outs[1][1], dev)
    loss = torch.tensor([0.625], device=dev)
    ref.i = 2
    ref.update(o_hr, o_lr, loss)
    d = mon._dev_descriptor(o_hr, o_lr)
    d.loss = loss.data_ptr()
    st = torch.cuda.current_stream(dev).cuda_stream
    mon.counter.fill_(2)
    N.check(built.dip_sr_monitor_dev(ctypes.byref(d), st), "sr_monitor_dev")
    torch.cuda.synchronize()
    assert mon.counter.item() == 3 and torch.equal(mon.records, ref.records) and mon.records[2, 0].item() == 0.625
    assert torch.count_nonzero(mon.records[[0, 1, 3]]).item() == 0
    for at in (cap, cap + 5, -1):
        table = torch.full((cap + 1, 5), 123.5, device=dev)          # a sentinel row past `capacity`
        d.records = table.data_ptr()
        mon.counter.fill_(at)
        N.check(built.dip_sr_monitor_dev(ctypes.byref(d), st), "sr_monitor_dev")
        torch.cuda.synchronize()
        assert mon.counter.item() == at and bool((table == 123.5).all()), at


# ------------------------------------------------------------------------------------------ 2. native against eager
def _fit(dev):
    return _sr_fit(dev, noisy=True, hw=HW, f=F)


def _monitor(f, hr=True, capacity=8, seed=11):
    from utils.fit_monitor import SRFitMonitor
    g = torch.Generator().manual_seed(seed)
    img_hr = torch.rand(1, 3, *HW, generator=g).to(f.target.device) if hr else None
    return SRFitMonitor(f.target, img_hr, capacity=capacity)


def _eager_mon_step(f, mon):
    """The closure of super-resolution.ipynb:169-191 with the two host PSNRs replaced by mon.update()."""
    f.opt.zero_grad()
    loss, out = f.head(f.reg())
    loss.backward()
    mon.update(out, f.head.out_LR, loss)
    f.opt.step()
    f.out = out
    return loss.detach()


def _assert_same_records(ma, mb, n, what=""):
    torch.cuda.synchronize()
    assert ma.i == mb.i == n, what
    ha, hb = ma.history(), mb.history()
    assert ha.shape == hb.shape == (n, 5), what
    assert torch.equal(ma.records, mb.records), (what, ha.tolist(), hb.tolist())          # untouched rows too
    assert (ha[:, [0, 1, 3]] != 0).all(), what


def test_native_iteration_is_bit_identical_to_the_eager_closure_with_update(dev):
    a, b = _fit(dev), _fit(dev)
    ma, mb = _monitor(a), _monitor(b)
    assert tuple(a.target.shape) == (1, 3, *LR)
    la = [_eager_mon_step(a, ma) for _ in range(6)]
    it = _native(b, mb)
    lb = list(it.run(6).unbind(0))
    assert torch.equal(torch.stack(la), torch.stack(lb))
    _assert_same_records(ma, mb, 6)
    _assert_same_state(a, b, a.out, it.out)
    assert torch.equal(ma.records[:6, 0], torch.stack(la))          # column 0 is that iteration's loss
    assert (mb.history()[:, [2, 4]] != 0).all()                     # img_HR given: the HR columns are filled
    assert mb.counter.item() == 6 == it.iterations and ma.counter.item() == 0
    names = [[n for n in cl.names] for cl in it._plan["lists"].phases]
    assert len(names) == 6 and names[4] == ["sr_monitor_dev"] and names[5][0] == "adam_tick"
    # the record is what the notebook computes on the host
    O = _oracle()
    r = mb.last()
    assert r["psnr_HR"] == pytest.approx(O.psnr(mb.img_HR.cpu().numpy(), it.out.cpu().numpy()), abs=TOL_DB)
    assert r["psnr_LR"] == pytest.approx(O.psnr(mb.img_LR.cpu().numpy(), b.head.out_LR.cpu().numpy()), abs=TOL_DB)


def test_eager_and_native_iterations_alternate_on_one_monitor(dev):
    a, b = _fit(dev), _fit(dev)
    ma, mb = _monitor(a, hr=False), _monitor(b, hr=False)
    la = [_eager_mon_step(a, ma) for _ in range(6)]
    it = _native(b, mb)
    lb = [_eager_mon_step(b, mb), _eager_mon_step(b, mb)]
    assert mb.i == 2 and mb.counter.item() == 0
    lb += list(it.run(3).unbind(0))
    assert mb.i == 5 and mb.counter.item() == 5
    lb.append(_eager_mon_step(b, mb))
    assert mb.i == 6 and mb.counter.item() == 5
    assert torch.equal(torch.stack(la), torch.stack(lb))
    _assert_same_records(ma, mb, 6)
    _assert_same_state(a, b, a.out, b.out)
    assert (mb.history()[:, [2, 4]] == 0).all()                     # no img_HR


# ------------------------------------------------------------------------------------------ 3. the fit is untouched
def test_the_monitor_does_not_touch_the_fit(dev):
    a, b = _fit(dev), _fit(dev)
    mb = _monitor(b)
    ita, itb = _native(a, None), _native(b, mb)
    la, lb = ita.run(2), itb.run(2)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                          # the plan is built: no host synchronisation in run()
    try:
        la, lb = torch.cat([la, ita.run(4)]), torch.cat([lb, itb.run(4)])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(la, lb) and la.shape == (6,)
    _assert_same_state(a, b, ita.out, itb.out)
    assert torch.equal(a.head.out_LR, b.head.out_LR)
    assert len(ita._plan["lists"].phases) == 5 and len(itb._plan["lists"].phases) == 6
    assert mb.i == 6 and torch.equal(mb.records[:6, 0], lb)


# ------------------------------------------------------------------------------------------ 4. grouped against solo
def _solo(dev, net, z, img_lr, img_hr, down, std, seed, capacity):
    from dip_optim import FusedAdam, NativeIteration
    from utils.common_utils import get_params
    from utils.fit_monitor import SRFitMonitor
    from utils.loss_head import SRHead
    from utils.reg_noise import RegNoise
    mon = SRFitMonitor(img_lr, img_hr, capacity=capacity)
    it = NativeIteration(net, SRHead(net, img_lr, down), FusedAdam(get_params("net", net, z), lr=0.01), z,
                         reg_noise=RegNoise(z, std, seed=seed), monitor=mon)
    return it, mon


def _assert_group_equals_solo(g, mon, nets, refs, solos, n, with_hr):
    torch.cuda.synchronize()
    assert mon.i == n == g.iterations and g.step_counts() == [n] * g.B and mon.counter.tolist() == [n] * g.B
    hist = mon.history()
    assert hist.shape == (g.B, n, 5)
    for b, (it, smon) in enumerate(solos):
        assert smon.i == n
        assert np.array_equal(hist[b], smon.history()), (b, hist[b].tolist(), smon.history().tolist())
        assert torch.equal(mon.records[b], smon.records), b                  # the untouched rows too
        for (k, pa), pb in zip(nets[b].named_parameters(), refs[b].parameters()):
            assert torch.equal(pa, pb), (b, k)
        assert torch.equal(g.out[b:b + 1], it.out) and torch.equal(g.out_LR[b:b + 1], it.head.out_LR), b
        assert (hist[b][:, [0, 1, 3]] != 0).all() and bool((hist[b][:, [2, 4]] != 0).all()) == with_hr, b
    assert len({hist[b, -1, 3] for b in range(g.B)}) == g.B                  # the instances really are different fits


@pytest.mark.parametrize("mask,with_hr", [(ALL, True), (0, True), (ALL, False)],
                         ids=["one-dispatch-imgs_HR", "host-loop-imgs_HR", "one-dispatch-no-HR"])
def test_grouped_records_bitwise_equal_solo(dev, native_mask, mask, with_hr):
    from dip_group import GroupedFits
    from utils.fit_monitor import GroupedSRFitMonitor
    B, std, cap = 3, 0.03, 8
    gen = torch.Generator().manual_seed(21)
    zs = [(torch.rand(1, 8, *HW, generator=gen) * 0.1).to(dev) for _ in range(B)]
    nets = [_net("skip3", 60 + b).to(dev) for b in range(B)]
    # Gaussian taps of one support (7 x 7, factor 2): instances 0 and 2 share theirs, instance 1 has its own
    downs = [_down(3, 2, "gauss", dev=dev, phase=0, kernel_width=7, sigma=s) for s in (0.5, 0.8, 0.5)]
    assert not torch.equal(downs[0]._taps, downs[1]._taps)
    lr_shape = _lr_size(nets[0], zs[0], downs[0])
    assert lr_shape == (1, 3, 16, 24)
    lrs = [torch.rand(lr_shape, generator=gen).to(dev) for _ in range(B)]
    hrs = [torch.rand(1, 3, *HW, generator=gen).to(dev) for _ in range(B)] if with_hr else None
    refs = [copy.deepcopy(x) for x in nets]
    solos = [_solo(dev, refs[b], zs[b], lrs[b], hrs[b] if with_hr else None, downs[b], std, 40 + b, cap) for b in range(B)]
    native_mask.dip_group_native(mask)
    mon = GroupedSRFitMonitor(hrs, capacity=cap)
    g = GroupedFits(nets, zs, lrs, downsamplers=downs, reg_noise_std=std, seeds=[40 + b for b in range(B)], lr=0.01, monitor=mon)
    assert g.pointers_outside_row0() == [] and g.out_avg is None and mon.group is g
    assert tuple(mon.records.shape) == (B, cap, 5) and tuple(mon.counter.shape) == (B,)
    # eager
    g.step(2)
    for it, _ in solos:
        it.run(2)
    _assert_group_equals_solo(g, mon, nets, refs, solos, 2, with_hr)
    # one more eager iteration (recorded like any other), then ONE hipGraph that holds the monitor's launch
    g.capture(warmup=1)
    g.run(4)
    for it, _ in solos:
        it.run(5)
    assert g.graph is not None
    _assert_group_equals_solo(g, mon, nets, refs, solos, 7, with_hr)
    assert native_mask.dip_group_size() == 1
    # the capacity: refused before anything is issued, eager or replayed
    before = mon.records.clone()
    with pytest.raises(RuntimeError, match="dip-amd:.*GroupedSRFitMonitor capacity"):
        g.run(2)
    torch.cuda.synchronize()
    assert mon.i == 7 and g.iterations == 7 and g.step_counts() == [7] * B and mon.counter.tolist() == [7] * B
    assert torch.equal(mon.records, before)


# ------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_before_anything_is_issued(dev):
    from dip_optim import NativeIteration
    from test_native_iter_gpu import _tiny
    from utils.fit_monitor import SRFitMonitor
    f = _fit(dev)
    img_hr = torch.rand(1, 3, *HW, device=dev)

    def untouched(mon, it=None):
        torch.cuda.synchronize()
        assert mon.i == 0 and mon.counter.item() == 0 and torch.count_nonzero(mon.records).item() == 0
        assert f.opt.step_count == 0 and (it is None or it.iterations == 0)

    # an SRFitMonitor records the two outputs of an SRHead
    m = _tiny(dev, "snail")
    with pytest.raises(TypeError, match="dip-amd:.*SRFitMonitor.*SRHead"):
        NativeIteration(m.net, m.head, m.opt, m.z, monitor=SRFitMonitor(f.target))
    with pytest.raises(TypeError, match="dip-amd:.*FitMonitor"):
        _native(f, object())
    # img_LR / img_HR against the head's LR size / the net output: when the plan is built, before anything is issued
    for mon, word in ((SRFitMonitor(f.target[:, :, :7].contiguous(), img_hr), "img_LR"),
                      (SRFitMonitor(f.target, img_hr[:, :, :, :40].contiguous()), "img_HR"),
                      (SRFitMonitor(f.target, f.target), "img_HR")):
        it = _native(f, mon)
        with pytest.raises(ValueError, match=f"dip-amd:.*SRFitMonitor.*{word}"):
            it.step()
        with pytest.raises(ValueError, match=f"dip-amd:.*SRFitMonitor.*{word}"):
            it.run(2)
        untouched(mon, it)
    # another device (the monitor says where it lives)
    mon = SRFitMonitor(f.target, img_hr)
    mon.dev = torch.device("cuda", 1)
    with pytest.raises(RuntimeError, match="dip-amd:.*SRFitMonitor lives on cuda:1"):
        _native(f, mon)
    untouched(mon)
    # the capacity
    mon = SRFitMonitor(f.target, img_hr, capacity=3)
    it = _native(f, mon)
    with pytest.raises(RuntimeError, match="dip-amd:.*SRFitMonitor capacity"):
        it.run(4)
    untouched(mon, it)
    assert f.opt.device_step_count() == 0
    # the eager form
    for args, exc in (((img_hr.cpu(), f.target), RuntimeError), ((img_hr, f.target.cpu()), RuntimeError),
                      ((img_hr[:, :, :30], f.target), ValueError), ((img_hr, f.target[:, :1]), ValueError)):
        with pytest.raises(exc, match="dip-amd:.*SRFitMonitor"):
            mon.update(*args)
    untouched(mon)
    with pytest.raises(RuntimeError, match="dip-amd:.*SRFitMonitor"):
        SRFitMonitor(f.target.cpu())
    with pytest.raises(RuntimeError, match="dip-amd:.*SRFitMonitor"):
        SRFitMonitor(f.target, img_hr.cpu())
    it.run(3)                                                        # ... and the same objects still fit
    with pytest.raises(RuntimeError, match="dip-amd:.*SRFitMonitor capacity"):
        mon.update(img_hr, f.target)
    with pytest.raises(RuntimeError, match="dip-amd:.*SRFitMonitor capacity"):
        it.step()
    torch.cuda.synchronize()
    assert mon.i == 3 == mon.counter.item() == f.opt.step_count == f.opt.device_step_count() == it.iterations
    # a FitMonitor with an SRHead keeps working (tests/test_sr_head_gpu.py), an eager plain step too
    _eager_step(f)
    assert f.opt.step_count == 4
