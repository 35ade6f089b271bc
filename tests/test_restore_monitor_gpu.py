"""The restoration monitor on a real MI355X (utils.fit_monitor.RestorationFitMonitor / GroupedRestorationFitMonitor;
dip_restore_monitor, dip_restore_monitor_dev): the bookkeeping of the closure of restoration.ipynb:180-219 of the reference

    psrn_masked = compare_psnr(img_masked, out * img_mask_np);  psrn = compare_psnr(img_np, out)                  (:192-193)
    if i % show_every == 0: fall back when psrn_masked - psrn_masked_last < -5, else checkpoint                   (:198-211)

1. the kernels against an fp64 restatement in torch, within the rounding of their own summation order;
2. the device-indexed kernels against the host-indexed ones -- bit for bit; the overflow guard;
3. the notebook's closure with its host bookkeeping (numpy PSNRs, cloned parameter lists) against the same closure with
   monitor.update(): the same decisions, bit-identical parameters;
4. NativeIteration(monitor=RestorationFitMonitor) against the eager closure with update() -- bit for bit;
5. GroupedFits(masks=, monitor=GroupedRestorationFitMonitor) against the solo fits, eager and as ONE hipGraph -- bit for bit.

The bound of 1. and 3.: a thread's fmaf chain has L = ceil(n / (256 nblk)) links, the LDS tree eight levels, and every element
two roundings before it is squared (out - img, the mask product); all terms are >= 0, so the relative error of a sum is at most
(L/2 + 4 + 2 + 1/2) 2^-23 < (L + 10) 2^-23.  A PSNR is -10 log10 of it: 10 / ln 10 times that, plus its own fp32 rounding."""
import copy
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_group_gpu import ALL, native_mask  # noqa: E402,F401
from test_group_monitor_gpu import _stream_pool_stands_where_it_stood  # noqa: E402,F401  (autouse: the engines and the
#                                      captured groups of this module draw pooled streams; the pool is left where it stood)
from test_native_iter_gpu import _assert_same_state  # noqa: E402

import dip_native as N  # noqa: E402

HW = (40, 24)
DBS = [5.0, -1e30, 1e30]


def _rel_bound(n, nblk):
    return (math.ceil(n / (256 * nblk)) + 10) * 2.0 ** -23


def _db_bound(n, nblk, psnr):
    return 10.0 / math.log(10.0) * _rel_bound(n, nblk) + float(np.spacing(np.float32(abs(psnr))))


def _truth(out, img, mask):
    """(mse_masked, mse, psnr_masked, psnr) in fp64 from the fp32 values: compare_psnr over the whole array, data range 1."""
    d = out.double() - img.double()
    mm, m = ((d * mask.double()) ** 2).mean().item(), (d ** 2).mean().item()
    ps = lambda x: math.inf if x == 0 else -10.0 * math.log10(x)          # noqa: E731
    return mm, m, ps(mm), ps(m)


def _assert_record(rec, truth, n, nblk, what):
    """Columns 1..4 of a record row against the fp64 truth, each figure printed before it is held to the bound."""
    rel = _rel_bound(n, nblk)
    for col, name in ((1, "mse_masked"), (2, "mse")):
        got, want = float(rec[col]), truth[col - 1]
        print(f"{what} {name}: {got:.9e} (fp64 {want:.9e}, rel err {abs(got - want) / want if want else 0.0:.2e}, bound {rel:.2e})")
        assert abs(got - want) <= rel * want, (what, name, got, want)
    for col, name in ((3, "psrn_masked"), (4, "psrn")):
        got, want = float(rec[col]), truth[col - 1]
        if math.isinf(want):
            assert got == want, (what, name, got)
            continue
        print(f"{what} {name}: {got:.7f} dB (fp64 {want:.7f}, err {abs(got - want):.2e}, bound {_db_bound(n, nblk, want):.2e})")
        assert abs(got - want) <= _db_bound(n, nblk, want), (what, name, got, want)


# ------------------------------------------------------------------------------------------ 1. kernels against fp64
KERNEL_SHAPES = [(1, 1, 1), (3, 5, 17), (3, 40, 24), (3, 592, 591)]


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=["1x1x1", "3x5x17", "3x40x24", "3x592x591-wraps"])
def test_kernel_against_fp64(dev, built, shape):
    L = built
    C, H, W = shape
    n, hw = C * H * W, H * W
    nblk = L.dip_fit_monitor_nblk(n)
    assert nblk == min((n + 1023) // 1024, 1024) and (shape == KERNEL_SHAPES[-1]) == (n > 1024 * 1024)
    g = torch.Generator().manual_seed(n % 1000 + 23)
    img = torch.rand(1, C, H, W, generator=g)
    out = (img + 0.05 * torch.randn(1, C, H, W, generator=g)).clamp_(0, 1)
    if n == 1:
        out = (img + 0.03125).clamp_(0, 1)          # (one element: keep it off the image, a zero error has no PSNR)
    img, out = img.to(dev), out.to(dev)
    loss = torch.tensor([0.625], device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    db, delta = 5.0, 0.01                            # the drops: 0.01 dB on either side of the threshold (>= 1e-3 dB)
    for mask_c in sorted({1, C}):
        for kind in ("bernoulli", "non-binary"):
            m = torch.rand(1, mask_c, H, W, generator=g)
            mask = ((m > 0.5).float() if kind == "bernoulli" else 0.25 + m).to(dev)
            truth = _truth(out, img, mask)
            p = truth[2]
            # (check, state before) -> (restore, snapshot) the fp64 truth alone decides
            cases = [(0, [7., 1., 1., 1.], (0., 0.)), (1, [1000., 1., 0., 0.], (0., 1.))]
            if math.isfinite(p):
                assert _db_bound(n, nblk, p) < delta / 10
                cases += [(1, [p + db + delta, 0., 1., 1.], (1., 0.)), (1, [p + db - delta, 1., 1., 0.], (0., 1.))]
            for k, (check, s0, (restore, snap)) in enumerate(cases):
                what = f"{shape} mask_c={mask_c} {kind} case {k}"
                rec = torch.full((6,), -3., device=dev)
                state = torch.tensor(s0, device=dev)
                part = torch.full((2 * nblk,), -7., device=dev)
                N.check(L.dip_restore_monitor(out.data_ptr(), img.data_ptr(), mask.data_ptr(), mask_c, n, hw,
                                              loss.data_ptr() if k != 1 else None, part.data_ptr(), rec.data_ptr(),
                                              state.data_ptr(), check, db, stream), "restore_monitor")
                torch.cuda.synchronize()
                rec, st = rec.cpu().numpy(), state.tolist()
                assert rec[0] == (0.625 if k != 1 else 0.0), what                 # the loss is copied through; NULL -> 0
                _assert_record(rec, truth, n, nblk, what)
                assert rec[5] == restore and st[1] == restore and st[3] == snap, (what, rec.tolist(), st)
                if snap:
                    assert st[0] == rec[3] and st[2] == 1., (what, st)           # psnr_masked_last <- psnr_masked, have_last <- 1
                else:
                    assert st[0] == state.new_tensor(s0)[0].item() and st[2] == s0[2], (what, st)
                assert (part != -7.).all(), what                                  # every block left its two sums
            if kind == "non-binary" and n > 1:
                assert abs(truth[0] - truth[1]) > 100 * _rel_bound(n, nblk) * truth[1]          # swapped columns would show


# ------------------------------------------------------------------------------------------ 2. device-indexed == host-indexed
def _series(dev, shape, mask_c, seed):
    """img, mask and five outputs: four at 26 dB, the fifth at 10 dB (a drop of more than 5 dB at the third check)."""
    C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(1, C, H, W, generator=g)
    mask = (torch.rand(1, mask_c, H, W, generator=g) > 0.5).float()
    outs = [(img + s * torch.randn(1, C, H, W, generator=g)).clamp_(0, 1).to(dev) for s in (0.05, 0.05, 0.05, 0.05, 0.3)]
    return img.to(dev), mask.to(dev), outs


@pytest.mark.parametrize("shape,mask_c", [((3, 40, 24), 1), ((3, 5, 17), 3), ((3, 592, 591), 1)],
                         ids=["3x40x24-plane", "3x5x17-full", "wraps-plane"])
def test_dev_kernels_equal_the_host_indexed_kernels(dev, built, shape, mask_c):
    L = built
    C, H, W = shape
    n, hw, cap, show, db = C * H * W, H * W, 8, 2, 5.0
    nblk = L.dip_fit_monitor_nblk(n)
    img, mask, outs = _series(dev, shape, mask_c, 77)
    stream = torch.cuda.current_stream(dev).cuda_stream
    recs_a, st_a, part_a = torch.zeros(cap, 6, device=dev), torch.zeros(4, device=dev), torch.full((2 * nblk,), -7., device=dev)
    recs_b, st_b, part_b = torch.zeros(cap, 6, device=dev), torch.zeros(4, device=dev), torch.full((2 * nblk,), -7., device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    losses = torch.arange(1, 6, device=dev) * 0.125
    d = N.DipRestoreMonitorDesc(None, img.data_ptr(), mask.data_ptr(), n, hw, mask_c, db, None, part_b.data_ptr(),
                                recs_b.data_ptr(), cap, show, 1, 0, counter.data_ptr(), st_b.data_ptr())
    for i, out in enumerate(outs):
        lp = losses[i:].data_ptr()
        N.check(L.dip_restore_monitor(out.data_ptr(), img.data_ptr(), mask.data_ptr(), mask_c, n, hw, lp, part_a.data_ptr(),
                                      recs_a[i].data_ptr(), st_a.data_ptr(), 1 if i % show == 0 else 0, db, stream),
                "restore_monitor")
        d.out, d.loss = out.data_ptr(), lp
        N.check(L.dip_restore_monitor_dev(ctypes.byref(d), stream), "restore_monitor_dev")
        torch.cuda.synchronize()
        assert torch.equal(recs_b, recs_a), (i, recs_b.tolist(), recs_a.tolist())          # untouched rows too
        assert torch.equal(st_b, st_a) and torch.equal(part_b, part_a), (i, st_b.tolist(), st_a.tolist())
        assert counter.item() == i + 1
    assert recs_a[:5, 5].tolist() == [0., 0., 0., 0., 1.]                     # checked at 0, 2, 4: snapshot, snapshot, fall back
    assert recs_a[:5, 0].tolist() == losses.tolist() and torch.count_nonzero(recs_a[5:]).item() == 0
    assert st_a.tolist() == [recs_a[2, 3].item(), 1., 1., 0.]
    # a monitor that does not back-track checks nothing, whatever the index
    d.backtracking = 0
    counter.fill_(4)
    N.check(L.dip_restore_monitor_dev(ctypes.byref(d), stream), "restore_monitor_dev")
    torch.cuda.synchronize()
    assert st_b.tolist() == [recs_a[2, 3].item(), 0., 1., 0.] and recs_b[4].tolist() == recs_a[4, :5].tolist() + [0.]


@pytest.mark.parametrize("at", [0, 5, -1], ids=["at_capacity", "past_capacity", "negative"])
def test_dev_kernels_overflow_guard_writes_nothing(dev, built, at):
    L = built
    cap, shape = 4, (3, 40, 24)
    n, hw = 3 * 40 * 24, 40 * 24
    img, mask, outs = _series(dev, shape, 1, 78)
    i = at if at < 0 else cap + at
    nblk = L.dip_fit_monitor_nblk(n)
    part = torch.full((2 * nblk,), -7., device=dev)
    recs = torch.full((cap + 6, 6), 123.5, device=dev)          # sentinel rows past `capacity`
    state = torch.tensor([31.5, 1., 1., 1.], device=dev)
    counter = torch.tensor([i], dtype=torch.int32, device=dev)
    loss = torch.tensor([0.625], device=dev)
    d = N.DipRestoreMonitorDesc(outs[0].data_ptr(), img.data_ptr(), mask.data_ptr(), n, hw, 1, -1e30, loss.data_ptr(),
                                part.data_ptr(), recs.data_ptr(), cap, 2, 1, 0, counter.data_ptr(), state.data_ptr())
    N.check(L.dip_restore_monitor_dev(ctypes.byref(d), torch.cuda.current_stream(dev).cuda_stream), "restore_monitor_dev")
    torch.cuda.synchronize()
    assert torch.equal(recs, torch.full((cap + 6, 6), 123.5, device=dev))
    assert torch.equal(part, torch.full((2 * nblk,), -7., device=dev))
    assert counter.item() == i
    assert state.tolist() == [31.5, 0., 1., 0.]          # restore and snapshot cleared: the back-track launch is a no-op


# ------------------------------------------------------------------------------------------ the fits of 3. - 5.
def _net(seed):
    from models.skip import skip
    torch.manual_seed(seed)
    return skip(8, 3, num_channels_down=[16, 32], num_channels_up=[16, 32], num_channels_skip=[4, 4],
                upsample_mode="bilinear", need_sigmoid=True, need_bias=True, pad="reflection")


def _data(dev, seed, mask_c):
    g = torch.Generator().manual_seed(seed)
    z = (torch.rand(1, 8, *HW, generator=g) * 0.1).to(dev)
    img = torch.rand(1, 3, *HW, generator=g).to(dev)
    mask = (torch.rand(1, mask_c, *HW, generator=g) > 0.5).float().to(dev)
    return z, img, mask


class _Fit:
    """The restoration fit on its own: RegNoise + MSEHead(mask=) + FusedAdam; `mon` = a RestorationFitMonitor or None."""

    def __init__(self, dev, net_seed=3, data_seed=4, mask_c=3, noisy=True, reg_seed=7, net=None, data=None, monitor=True, **mon_kw):
        from dip_optim import FusedAdam
        from utils.common_utils import get_params
        from utils.loss_head import MSEHead
        from utils.reg_noise import RegNoise
        self.net = (_net(net_seed) if net is None else net).to(dev)
        self.z, self.img, self.mask = data if data is not None else _data(dev, data_seed, mask_c)
        self.target = self.img
        self.head = MSEHead(self.net, self.img, mask=self.mask)
        self.reg = RegNoise(self.z, 0.03, seed=reg_seed) if noisy else None
        self.opt = FusedAdam(get_params('net', self.net, self.z), lr=0.01)
        self.mon_kw = dict(dict(show_every=3, capacity=16), **mon_kw)
        self.mon = self.monitor() if monitor else None
        self.out = None

    def monitor(self, **kw):
        from utils.fit_monitor import RestorationFitMonitor
        return RestorationFitMonitor(self.net, self.img, self.mask, **dict(self.mon_kw, **kw))

    def forward_backward(self):
        self.opt.zero_grad()
        loss, out = self.head(self.reg() if self.reg is not None else self.z)
        loss.backward()
        self.out = out
        return loss, out

    def eager(self, mon="own"):
        """opt.zero_grad(); loss, out = head(x); loss.backward(); monitor.update(out, loss); opt.step()"""
        mon = self.mon if mon == "own" else mon
        loss, out = self.forward_backward()
        if mon is not None:
            mon.update(out, loss)
        self.opt.step()
        return loss.detach()

    def native(self, mon="own"):
        from dip_optim import NativeIteration
        return NativeIteration(self.net, self.head, self.opt, self.z, reg_noise=self.reg, monitor=self.mon if mon == "own" else mon)


def _assert_same_monitor(ma, mb, what=""):
    torch.cuda.synchronize()
    assert ma.i == mb.i, what
    ha, hb = ma.history(), mb.history()
    assert ha.shape == hb.shape == (ma.i, 6), what
    assert torch.equal(ma.records, mb.records), (what, ha.tolist(), hb.tolist())          # all 6 columns, untouched rows too
    assert torch.equal(ma.state, mb.state), (what, ma.state.tolist(), mb.state.tolist())
    assert (ma.snapshot is None) == (mb.snapshot is None), what
    if ma.snapshot is not None:
        assert torch.equal(ma.snapshot, mb.snapshot), what


def _assert_same(a, b, la, lb, out_b, what=""):
    assert torch.equal(torch.stack(la), torch.stack(lb)), (what, torch.stack(la).tolist(), torch.stack(lb).tolist())
    _assert_same_monitor(a.mon, b.mon, what)
    assert torch.equal(a.mon.records[:a.mon.i, 0], torch.stack(la)), what          # column 0 is that iteration's loss
    _assert_same_state(a, b, a.out, out_b, what)


# ------------------------------------------------------------------------------------------ 3. the notebook's host bookkeeping
@pytest.mark.parametrize("db", DBS)
def test_update_equals_the_notebooks_host_bookkeeping(dev, built, db):
    """Arm A is restoration.ipynb:180-219 as the notebook spells it -- the PSNRs with numpy on `.cpu().numpy()` copies
    (10 log10(1 / mse), compare_psnr's formula at data range 1, in fp64), last_net a list of cloned tensors -- arm B the same
    closure with monitor.update().  (The first check checkpoints in both arms: the notebook's psrn_masked_last = 0 decides the
    same for images in [0, 1], see the header.)"""
    k, show = 8, 3
    a, b = _Fit(dev, mask_c=1, monitor=False), _Fit(dev, mask_c=1, show_every=show, backtrack_db=db)
    img_np, mask_np = a.img.cpu().numpy()[0].astype(np.float64), a.mask.cpu().numpy()[0].astype(np.float64)
    img_masked = img_np * mask_np
    psnr = lambda x, y: 10.0 * np.log10(1.0 / np.mean((x - y) ** 2))          # noqa: E731
    n = a.img.numel()
    nblk = built.dip_fit_monitor_nblk(n)
    last_net, last = None, 0.0
    rows, diffs = [], []
    for i in range(k):
        loss, out = a.forward_backward()
        out_np = out.detach().cpu().numpy()[0].astype(np.float64)
        psrn_masked, psrn = psnr(img_masked, out_np * mask_np), psnr(img_np, out_np)          # :192-193
        fell = 0.
        if i % show == 0:                                                                     # :198
            if last_net is not None:
                diffs.append(psrn_masked - last)
            if last_net is not None and psrn_masked - last < -db:                             # :202-208
                for new, p in zip(last_net, a.net.parameters()):
                    p.data.copy_(new)
                fell = 1.
            else:                                                                             # :209-211
                last_net = [p.detach().clone() for p in a.net.parameters()]
                last = psrn_masked
        a.opt.step()
        rows.append((loss.item(), psrn_masked, psrn, fell))
        b.eager()
    torch.cuda.synchronize()
    assert len(diffs) == 2                                                    # checked at 0, 3, 6
    if db == 5.0:
        print("checked differences (dB):", diffs)
        assert all(abs(x + 5.0) >= 1e-3 for x in diffs), diffs                # the fp64 truth alone decides
    hist = b.mon.history()
    fell_a = [r[3] for r in rows]
    assert hist[:, 5].tolist() == fell_a, (hist[:, 5].tolist(), fell_a)
    assert fell_a == {-1e30: [0., 0., 0., 1., 0., 0., 1., 0.], 1e30: [0.] * 8}.get(db, fell_a)
    for (k1, pa), pb in zip(a.net.named_parameters(), b.net.parameters()):
        assert torch.equal(pa, pb), k1
    for i, (loss, pm, p, _) in enumerate(rows):
        assert hist[i, 0] == np.float32(loss)
        for col, want in ((3, pm), (4, p)):
            print(f"db={db} i={i} col {col}: {hist[i, col]:.7f} dB (numpy {want:.7f}, bound {_db_bound(n, nblk, want):.2e})")
            assert abs(float(hist[i, col]) - want) <= _db_bound(n, nblk, want), (i, col)
        assert abs(float(hist[i, 1]) - 10.0 ** (-pm / 10.0)) <= 2 * _rel_bound(n, nblk) * float(hist[i, 1])


# ------------------------------------------------------------------------------------------ 4. NativeIteration(monitor=)
def _run_both(dev, mode, k=7, **kw):
    a, b = _Fit(dev, **kw), _Fit(dev, **kw)
    la = [a.eager() for _ in range(k)]
    it = b.native()
    lb = [it.step() for _ in range(k)] if mode == "step" else list(it.run(k).unbind(0))
    _assert_same(a, b, la, lb, it.out, (mode, kw))
    assert b.mon.i == k == it.iterations == b.opt.step_count and b.mon.counter.item() == k
    return a, b, it


@pytest.mark.parametrize("mode", ["step", "run"])
@pytest.mark.parametrize("db", DBS)
def test_native_is_bit_identical_to_the_eager_closure_with_update(dev, db, mode):
    a, b, it = _run_both(dev, mode, backtrack_db=db)
    names = [n for cl in it._plan["lists"].phases for n in cl.names]
    assert len(it._plan["lists"].phases) == 6 and names.count("restore_monitor_dev") == 1 and names.count("arena_backtrack") == 1
    assert names.index("restore_monitor_dev") + 1 == names.index("arena_backtrack") < names.index("adam_tick")
    fell = b.mon.history()[:, 5].tolist()
    if db == -1e30:              # checked at 0, 3, 6: the first check checkpoints, every other one falls back
        assert fell == [0., 0., 0., 1., 0., 0., 1.], fell
    elif db == 1e30:
        assert fell == [0.] * 7, fell
    hist = b.mon.history()
    assert (hist[:, 1:5] > 0).all() and (hist[:, 1] < hist[:, 2]).all()          # a 0/1 mask: the masked error is the smaller
    assert b.mon.snapshot is not None and b.mon.snapshot.numel() == b.net.__dict__["_dip_engine"].params.numel()


def test_native_without_backtracking(dev):
    a, b, it = _run_both(dev, "run", backtracking=False)
    assert a.mon.snapshot is None and b.mon.snapshot is None and b.mon.engine is None
    assert "arena_backtrack" not in [n for cl in it._plan["lists"].phases for n in cl.names]
    hist = b.mon.history()
    assert (hist[:, 5] == 0).all() and (hist[:, 3] != 0).all() and b.mon.state.tolist() == [0., 0., 0., 0.]


@pytest.mark.parametrize("mode", ["step", "run"])
def test_native_under_a_one_plane_mask_without_reg_noise(dev, mode):
    a, b, it = _run_both(dev, mode, mask_c=1, noisy=False, backtrack_db=-1e30)
    assert b.head.mask_c == b.mon.mask_c == 1 and b.mon.history()[:, 5].tolist() == [0., 0., 0., 1., 0., 0., 1.]


def test_eager_and_native_iterations_alternate_on_one_monitor(dev):
    """eager x 2 -> run(3) -> eager x 1 -> step() on ONE net / head / optimiser / monitor == 7 eager iterations on the twin."""
    a, b = _Fit(dev, backtrack_db=-1e30), _Fit(dev, backtrack_db=-1e30)
    la = [a.eager() for _ in range(7)]
    it = b.native()
    lb = [b.eager(), b.eager()]
    assert b.mon.i == 2 and b.mon.counter.item() == 0          # update() passes i by value and leaves the counter alone
    lb += list(it.run(3).unbind(0))
    assert b.mon.i == 5 and b.mon.counter.item() == 5
    lb.append(b.eager())
    assert b.mon.i == 6 and b.mon.counter.item() == 5
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                    # the resync and the iteration: no host synchronisation
    try:
        lb.append(it.step())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert b.mon.i == 7 and b.mon.counter.item() == 7
    _assert_same(a, b, la, lb, it.out)
    assert b.mon.history()[:, 5].tolist() == [0., 0., 0., 1., 0., 0., 1.]


def test_capacity_is_refused_before_anything_is_issued(dev):
    b = _Fit(dev, capacity=4)
    it = b.native()
    assert it.run(4).shape == (4,)
    torch.cuda.synchronize()

    def frozen():
        return ([p.detach().clone() for p in b.net.parameters()], b.mon.records.clone(), b.mon.state.clone(),
                b.mon.counter.clone(), b.reg.offset.clone())

    before = frozen()
    with pytest.raises(RuntimeError, match="dip-amd:.*RestorationFitMonitor capacity"):
        it.step()
    with pytest.raises(RuntimeError, match="dip-amd:.*RestorationFitMonitor capacity"):
        it.run(1)
    with pytest.raises(RuntimeError, match="dip-amd:.*RestorationFitMonitor capacity"):
        b.mon.update(it.out)
    torch.cuda.synchronize()
    after = frozen()
    for p, q in zip(before[0], after[0]):
        assert torch.equal(p, q)
    for x, y in zip(before[1:], after[1:]):
        assert torch.equal(x, y)
    assert b.mon.i == 4 and it.iterations == 4 and b.opt.step_count == 4 and b.opt.device_step_count() == 4
    # a fresh run that would only overflow at its end is refused as a whole
    c = _Fit(dev, capacity=4)
    itc = c.native()
    with pytest.raises(RuntimeError, match="capacity"):
        itc.run(5)
    torch.cuda.synchronize()
    assert c.mon.i == 0 and itc.iterations == 0 and c.opt.step_count == 0 and c.mon.counter.item() == 0
    assert torch.count_nonzero(c.mon.records).item() == 0


def test_replacing_the_records_or_the_monitor_rebuilds_the_plan(dev):
    a, b = _Fit(dev, backtrack_db=-1e30), _Fit(dev, backtrack_db=-1e30)
    it = b.native()
    la, lb = [a.eager(), a.eager()], [it.step(), it.step()]
    lists0 = it._plan["lists"]
    for f in (a, b):
        f.mon.records = f.mon.records.clone()                    # a new buffer with the old values
    la.append(a.eager()), lb.append(it.step())
    assert it._plan["lists"] is not lists0
    _assert_same(a, b, la, lb, it.out, "records replaced")
    # another monitor on the same iteration object: its own records from row 0, its own counter
    first = (a.mon, b.mon)
    a.mon, b.mon = a.monitor(show_every=2), b.monitor(show_every=2)
    it.monitor = b.mon
    lists1 = it._plan["lists"]
    la2 = [a.eager() for _ in range(3)]
    lb2 = list(it.run(3).unbind(0))
    assert it._plan["lists"] is not lists1
    _assert_same(a, b, la2, lb2, it.out, "monitor replaced")
    assert b.mon.history()[:, 5].tolist() == [0., 0., 1.] and first[1].i == 3 and first[1].counter.item() == 3
    _assert_same_monitor(*first, "the first monitor was left alone")
    # refusals of the iteration: another net's back-tracking monitor, an image of another size
    other = _Fit(dev, net_seed=9)
    it.monitor = other.mon
    with pytest.raises(ValueError, match="dip-amd:.*RestorationFitMonitor back-tracks another net"):
        it.step()
    from utils.fit_monitor import RestorationFitMonitor
    it.monitor = RestorationFitMonitor(b.net, b.img[:, :, :32].contiguous(), b.mask[:, :, :32].contiguous(), capacity=4)
    with pytest.raises(ValueError, match="dip-amd:.*RestorationFitMonitor's image"):
        it.step()
    assert it.monitor.i == 0 and it.iterations == 6


def test_monitor_none_is_the_parent_iteration(dev):
    """monitor=None: the same five command arrays as before, the same key, and the same results as the eager closure; and a
    monitored fit's losses and parameters are those of the unmonitored one as long as nothing falls back."""
    a, b, c = _Fit(dev, monitor=False), _Fit(dev, monitor=False), _Fit(dev, backtrack_db=1e30)
    it, itc = b.native(), c.native()
    la = [a.eager() for _ in range(3)]
    lb = [it.step() for _ in range(3)]
    lc = list(itc.run(3).unbind(0))
    assert torch.equal(torch.stack(la), torch.stack(lb)) and torch.equal(torch.stack(la), torch.stack(lc))
    assert len(it._plan["lists"].phases) == 5 and it._plan["mdesc"] is None
    assert len(itc._key) == len(it._key) + 1                     # the key as it was, plus the monitor's
    _assert_same_state(a, b, a.out, it.out)
    _assert_same_state(a, c, a.out, itc.out)


# ------------------------------------------------------------------------------------------ 5. grouped
class _Solo:
    """Instance b on its own: NativeIteration under a RestorationFitMonitor."""

    def __init__(self, dev, net, data, seed, **mon_kw):
        self.fit = _Fit(dev, net=net, data=data, reg_seed=seed, **mon_kw)
        self.it = self.fit.native()
        self.mon = self.fit.mon
        self.loss = None

    def step(self, n):
        self.loss = self.it.run(n)[-1]


@pytest.mark.parametrize("mask", [ALL, 0], ids=["one-dispatch", "host-loop"])
@pytest.mark.parametrize("mask_c", [1, 3])
def test_monitored_group_bitwise_equals_solo_fits(dev, native_mask, mask_c, mask):
    from dip_group import GroupedFits
    from utils.fit_monitor import GroupedRestorationFitMonitor
    B, kw = 3, dict(show_every=2, backtrack_db=5.0, capacity=16)
    data = [_data(dev, 60 + b, mask_c) for b in range(B)]
    nets = [_net(10 + b).to(dev) for b in range(B)]
    refs = [copy.deepcopy(n) for n in nets]
    solo = [_Solo(dev, refs[b], data[b], 40 + b, **kw) for b in range(B)]
    native_mask.dip_group_native(mask)
    gm = GroupedRestorationFitMonitor(**kw)
    g = GroupedFits(nets, [d[0] for d in data], [d[1] for d in data], masks=[d[2] for d in data], reg_noise_std=0.03,
                    seeds=[40 + b for b in range(B)], lr=0.01, monitor=gm)
    assert g.pointers_outside_row0() == [] and g.out_avg is None
    assert [name for _, _, name in g._mon] == ["restore_monitor_dev", "arena_backtrack"]          # ONE call each for all B

    def both(n, run):
        run(n)
        for s in solo:
            s.step(n)

    def poke(b, above=True):
        """above: instance b will fall back at its next check (its last PSNR stands far above anything it can reach -- and stays
        there: a fall-back keeps psnr_masked_last, as the notebook does); not above: it will checkpoint again."""
        torch.cuda.synchronize()
        row = torch.tensor([1e30 if above else -1e30, 0., 1., 0.], device=dev)
        gm.state[b].copy_(row)
        solo[b].mon.state.copy_(row)

    def same(what):
        torch.cuda.synchronize()
        assert g.step_counts() == [gm.i] * B and g.iterations == gm.i and gm.counter.tolist() == [gm.i] * B, what
        hist = gm.history()
        assert hist.shape == (B, gm.i, 6), what
        for b, s in enumerate(solo):
            assert s.mon.i == gm.i and s.fit.opt.device_step_count() == gm.i, (what, b)
            assert torch.equal(gm.records[b], s.mon.records), (what, b, hist[b].tolist(), s.mon.history().tolist())
            assert torch.equal(gm.state[b], s.mon.state), (what, b, gm.state[b].tolist(), s.mon.state.tolist())
            assert torch.equal(gm.snapshot[b], s.mon.snapshot), (what, b)
            assert g.losses[b].item() == s.loss.item() == hist[b, -1, 0], (what, b)
            assert torch.equal(g.out[b:b + 1], s.it.out), (what, b)
            for (k, pa), pb in zip(nets[b].named_parameters(), refs[b].parameters()):
                assert torch.equal(pa, pb), (what, b, k)
            for (k, ba), bb in zip(nets[b].named_buffers(), refs[b].buffers()):
                assert torch.equal(ba, bb), (what, b, k)
            assert gm.last()[b] == s.mon.last(), (what, b)

    both(2, g.step)                                  # iteration 0 is the first checked one: every instance snapshots
    same("after 2 (eager)")
    assert gm.state[:, 2].tolist() == [1.] * B and gm.records[:, 0, 5].tolist() == [0.] * B
    poke(1)
    both(1, g.step)                                  # iteration 2, eager: instance 1 falls back, the others snapshot
    same("after 3 (eager)")
    assert gm.records[:, 2, 5].tolist() == [0., 1., 0.] and gm.state[:, 3].tolist() == [1., 0., 1.]
    g.capture(warmup=1)                              # iteration 3 eager, then ONE hipGraph
    assert g.graph is not None
    for s in solo:
        s.step(1)
    poke(1, above=False), poke(0)
    both(2, g.run)                                   # 4 (checked: instance 0 falls back, 1 checkpoints again) and 5, replayed
    same("after 6 (2 replayed)")
    assert gm.records[:, 4, 5].tolist() == [1., 0., 0.]
    poke(0, above=False), poke(2)
    both(3, g.run)                                   # 6 and 8 are checked: instance 2 falls back at both, between two replays
    same("after 9 (5 replayed)")
    fell = gm.history()[:, :, 5]
    assert fell[:, 6].tolist() == fell[:, 8].tolist() == [0., 0., 1.] and fell.sum() == 4
    assert len({round(g.losses[b].item(), 9) for b in range(B)}) == B          # the instances really are different fits
    assert native_mask.dip_group_size() == 1
