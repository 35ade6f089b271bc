"""NativeIteration(monitor=) on the GPU: the closure of denoising.ipynb:204-248 -- loss, backward, the exponential average of
the output, three PSNRs, the back-tracking checkpoint / fall-back, Adam -- as ONE dip_iter_run call per iteration, against the
eager closure it restates

    opt.zero_grad(); loss, out = head(reg()); loss.backward(); monitor.update(out, loss); opt.step()

The eager path is the truth (tests/test_monitor_gpu.py holds FitMonitor.update to the oracle, the rest of the suite the
iteration).  Both arms run the same arithmetic in the same order, so every comparison is torch.equal: no tolerance anywhere."""
import ctypes

import pytest
import torch

from test_native_iter_gpu import _assert_same_state, _eager_step, _tiny

pytestmark = pytest.mark.gpu

SHOW_EVERY = 3


def _monitor(f, db=5.0, gt=True, backtracking=True, capacity=16, seed=11):
    """A FitMonitor for the fit `f`: the head's target is the noisy image, the clean image is drawn from `seed`."""
    from utils.fit_monitor import FitMonitor
    g = torch.Generator().manual_seed(seed)
    clean = torch.rand(f.target.shape, generator=g).to(f.target.device) if gt else None
    return FitMonitor(f.net, f.target, clean, exp_weight=0.9, show_every=SHOW_EVERY, backtrack_db=db,
                      backtracking=backtracking, capacity=capacity)


def _eager_mon_step(f, mon):
    """test_native_iter_gpu._eager_step with monitor.update(out, loss) between backward() and opt.step()."""
    f.opt.zero_grad()
    x = f.reg() if f.reg is not None else f.z
    loss, out = f.head(x)
    loss.backward()
    mon.update(out, loss)
    f.opt.step()
    f.out = out
    return loss.detach()


def _native(f, mon):
    from dip_optim import NativeIteration
    return NativeIteration(f.net, f.head, f.opt, f.z, reg_noise=f.reg, monitor=mon)


def _assert_same_monitor(ma, mb, what=""):
    torch.cuda.synchronize()
    assert ma.i == mb.i, what
    ha, hb = ma.history(), mb.history()
    assert ha.shape == hb.shape == (ma.i, 8), what
    assert torch.equal(ma.records, mb.records), (what, ha.tolist(), hb.tolist())          # all 8 columns, untouched rows too
    assert torch.equal(ma.out_avg, mb.out_avg), what
    assert torch.equal(ma.state, mb.state), (what, ma.state.tolist(), mb.state.tolist())
    assert (ma.snapshot is None) == (mb.snapshot is None), what
    if ma.snapshot is not None:
        assert torch.equal(ma.snapshot, mb.snapshot), what


def _assert_same(a, b, ma, mb, la, lb, out_b, what=""):
    assert torch.equal(torch.stack(la), torch.stack(lb)), (what, torch.stack(la).tolist(), torch.stack(lb).tolist())
    _assert_same_monitor(ma, mb, what)
    assert torch.equal(ma.records[:ma.i, 0], torch.stack(la)), what          # column 0 is that iteration's loss
    _assert_same_state(a, b, a.out, out_b, what)


# ------------------------------------------------------------------------------------------ 1. kernel against kernel
def _kernel_inputs(dev, n, gt):
    g = torch.Generator().manual_seed(n % 1000 + 17)
    out = torch.rand(n, generator=g).to(dev)
    noisy = torch.rand(n, generator=g).to(dev)
    clean = torch.rand(n, generator=g).to(dev) if gt else None
    avg0 = torch.rand(n, generator=g).to(dev)
    return out, noisy, clean, avg0


# state before the call: nothing recorded yet (first checkpoint) / a last PSNR far above (restore) / far below (snapshot)
STATES = {"fresh": [0., 0., 0., 0.], "restore": [1000., 0., 1., 1.], "snapshot": [-1000., 1., 1., 0.]}


@pytest.mark.parametrize("gt", [True, False])
@pytest.mark.parametrize("n", [1, 255, 3 * 40 * 24, 1024 * 1024 + 3])
def test_dev_kernels_equal_the_host_indexed_kernels(dev, built, n, gt):
    import dip_native as N
    L = built
    cap, w, db = 8, 0.9, 5.0
    out, noisy, clean, avg0 = _kernel_inputs(dev, n, gt)
    nblk = L.dip_fit_monitor_nblk(n)
    assert (nblk == 1024 and n > 1024 * 1024) or nblk == (n + 1023) // 1024          # the last size wraps the grid-stride loop
    loss = torch.tensor([0.625], device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    stream = torch.cuda.current_stream(dev).cuda_stream
    taken = set()
    for i in (0, 1, SHOW_EVERY, SHOW_EVERY + 1):
        for sname, s0 in STATES.items():
            for backtracking in ((1, 0) if (sname == "restore" and n == 255) else (1,)):
                # the host-indexed kernels
                avg_a, part_a = avg0.clone(), torch.full((4 * nblk,), -7., device=dev)
                rec_a, st_a = torch.zeros(8, device=dev), torch.tensor(s0, device=dev)
                check = 1 if (backtracking and i % SHOW_EVERY) else 0
                N.check(L.dip_fit_monitor(ptr(out), ptr(noisy), ptr(clean), ptr(avg_a), n, w, 1 if i == 0 else 0, ptr(loss),
                                          ptr(part_a), ptr(rec_a), ptr(st_a), check, db, stream), "fit_monitor")
                # the device-indexed kernels
                avg_b, part_b = avg0.clone(), torch.full((4 * nblk,), -7., device=dev)
                recs_b, st_b = torch.zeros(cap, 8, device=dev), torch.tensor(s0, device=dev)
                counter = torch.tensor([i], dtype=torch.int32, device=dev)
                d = N.DipFitMonitorDesc(ptr(out), ptr(noisy), ptr(clean), ptr(avg_b), n, w, db, ptr(loss), ptr(part_b),
                                        ptr(recs_b), cap, SHOW_EVERY, backtracking, 0, ptr(counter), ptr(st_b))
                N.check(L.dip_fit_monitor_dev(ctypes.byref(d), stream), "fit_monitor_dev")
                torch.cuda.synchronize()
                what = (n, gt, i, sname, backtracking)
                assert torch.equal(recs_b[i], rec_a), (what, recs_b[i].tolist(), rec_a.tolist())
                rest = torch.cat([recs_b[:i], recs_b[i + 1:]])
                assert torch.count_nonzero(rest).item() == 0, what                  # no other row was touched
                assert torch.equal(st_b, st_a), (what, st_b.tolist(), st_a.tolist())
                assert torch.equal(avg_b, avg_a) and torch.equal(part_b, part_a), what
                assert counter.item() == i + 1, what
                assert rec_a[0].item() == 0.625 and rec_a[4].item() != 0., what
                assert (rec_a[5].item() != 0.) == gt, what
                if i == 0:
                    assert torch.equal(avg_a, out), what
                taken.add((st_a[1].item(), st_a[3].item()))
    assert taken == {(0., 0.), (1., 0.), (0., 1.)}          # not checked, restore, snapshot: every branch ran


@pytest.mark.parametrize("at", [0, 5, -1], ids=["at_capacity", "past_capacity", "negative"])
def test_dev_kernels_overflow_guard_writes_nothing(dev, built, at):
    import dip_native as N
    L = built
    cap, n = 4, 3 * 40 * 24
    out, noisy, clean, avg0 = _kernel_inputs(dev, n, True)
    i = at if at < 0 else cap + at
    nblk = L.dip_fit_monitor_nblk(n)
    avg, part = avg0.clone(), torch.full((4 * nblk,), -7., device=dev)
    recs = torch.full((cap + 1, 8), 123.5, device=dev)          # a sentinel row past `capacity`
    state = torch.tensor([31.5, 1., 1., 1.], device=dev)
    counter = torch.tensor([i], dtype=torch.int32, device=dev)
    loss = torch.tensor([0.625], device=dev)
    d = N.DipFitMonitorDesc(out.data_ptr(), noisy.data_ptr(), clean.data_ptr(), avg.data_ptr(), n, 0.9, -1e30, loss.data_ptr(),
                            part.data_ptr(), recs.data_ptr(), cap, SHOW_EVERY, 1, 0, counter.data_ptr(), state.data_ptr())
    N.check(L.dip_fit_monitor_dev(ctypes.byref(d), torch.cuda.current_stream(dev).cuda_stream), "fit_monitor_dev")
    torch.cuda.synchronize()
    assert torch.equal(recs, torch.full((cap + 1, 8), 123.5, device=dev))
    assert torch.equal(avg, avg0)
    assert counter.item() == i
    assert state.tolist() == [31.5, 0., 1., 0.]          # restore and snapshot cleared: the back-track launch is a no-op


# ------------------------------------------------------------------------------------------ 2. the whole iteration
def _run_both(dev, case, db, mode, masked=False, noisy=True, k=7, **mon_kw):
    a, b = _tiny(dev, case, masked=masked, noisy=noisy), _tiny(dev, case, masked=masked, noisy=noisy)
    ma, mb = _monitor(a, db, **mon_kw), _monitor(b, db, **mon_kw)
    la = [_eager_mon_step(a, ma) for _ in range(k)]
    it = _native(b, mb)
    lb = [it.step() for _ in range(k)] if mode == "step" else list(it.run(k).unbind(0))
    _assert_same(a, b, ma, mb, la, lb, it.out, (case, db, mode))
    assert mb.i == k == it.iterations == b.opt.step_count and mb.counter.item() == k
    return a, b, ma, mb, it


@pytest.mark.parametrize("mode", ["step", "run"])
@pytest.mark.parametrize("db", [5.0, -1e30, 1e30])
def test_bit_identical_to_the_eager_closure_with_update(dev, db, mode):
    a, b, ma, mb, it = _run_both(dev, "default", db, mode)
    for m in (ma, mb):
        fell = m.history()[:, 7].tolist()
        if db == -1e30:
            # the decision does not depend on the data: i = 0, 3, 6 are not checked, i = 1 is the first checkpoint, every
            # other checked iteration falls back -- both branches of the back-tracking ran, in both arms
            assert fell == [0., 0., 1., 0., 1., 1., 0.], fell
        elif db == 1e30:
            assert fell == [0.] * 7, fell
        hist = m.history()
        assert (hist[:, 4:7] != 0).all() and (hist[:, 1:4] > 0).all()          # gt given: every PSNR / MSE column is filled
    assert mb.snapshot is not None and mb.snapshot.numel() == b.net.__dict__["_dip_engine"].params.numel()


@pytest.mark.parametrize("mode", ["step", "run"])
@pytest.mark.parametrize("case,masked", [("library", True), ("snail", False)])
def test_bit_identical_on_the_other_nets(dev, case, masked, mode):
    _run_both(dev, case, 5.0, mode, masked=masked)


# ------------------------------------------------------------------------------------------ 3. alternation
def test_eager_and_native_iterations_alternate_on_one_monitor(dev):
    """eager x 2 -> run(3) -> eager x 1 -> step() on ONE net / head / optimiser / monitor == 7 eager iterations on the twin: the
    device counter is re-aligned with monitor.i in front of run(3) (2 eager updates) and in front of step() (1 more)."""
    a, b = _tiny(dev, "default", noisy=True), _tiny(dev, "default", noisy=True)
    ma, mb = _monitor(a, -1e30), _monitor(b, -1e30)
    la = [_eager_mon_step(a, ma) for _ in range(7)]
    it = _native(b, mb)
    lb = [_eager_mon_step(b, mb), _eager_mon_step(b, mb)]
    assert mb.i == 2 and mb.counter.item() == 0          # update() passes i by value and leaves the counter alone
    lb += list(it.run(3).unbind(0))
    assert mb.i == 5 and mb.counter.item() == 5
    lb.append(_eager_mon_step(b, mb))
    assert mb.i == 6 and mb.counter.item() == 5
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")              # the resync and the iteration: no host synchronisation
    try:
        lb.append(it.step())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert mb.i == 7 and mb.counter.item() == 7
    _assert_same(a, b, ma, mb, la, lb, it.out)
    assert mb.history()[:, 7].tolist() == [0., 0., 1., 0., 1., 1., 0.]


def test_fresh_monitor_with_a_hand_set_index(dev):
    """A monitor whose `i` is not 0 when the iteration first sees it: the counter follows `i`."""
    a, b = _tiny(dev, "snail", noisy=True), _tiny(dev, "snail", noisy=True)
    ma, mb = _monitor(a), _monitor(b)
    ma.i = mb.i = 4
    la = [_eager_mon_step(a, ma) for _ in range(3)]
    it = _native(b, mb)
    lb = list(it.run(3).unbind(0))
    assert torch.equal(torch.stack(la), torch.stack(lb))
    _assert_same_monitor(ma, mb)
    assert mb.i == 7 and mb.counter.item() == 7 and torch.count_nonzero(mb.records[:4]).item() == 0
    _assert_same_state(a, b, a.out, it.out)


# ------------------------------------------------------------------------------------------ 4. variants
def test_without_ground_truth_and_without_backtracking(dev):
    a, b, ma, mb, it = _run_both(dev, "default", 5.0, "run", gt=False, backtracking=False)
    assert ma.snapshot is None and mb.snapshot is None
    assert "arena_backtrack" not in [n for cl in it._plan["lists"].phases for n in cl.names]
    hist = mb.history()
    assert (hist[:, [2, 3, 5, 6, 7]] == 0).all() and (hist[:, 4] != 0).all()
    assert mb.state.tolist() == [0., 0., 0., 0.]


def test_without_reg_noise_under_a_masked_head(dev):
    _run_both(dev, "default", 5.0, "step", masked=True, noisy=False)


def test_monitor_none_is_the_parent_iteration(dev):
    """monitor=None: the same five command arrays as before and the same results as the eager closure."""
    a, b = _tiny(dev, "snail", noisy=True), _tiny(dev, "snail", noisy=True)
    it = _native(b, None)
    la = [_eager_step(a) for _ in range(2)]
    lb = [it.step(), it.step()]
    assert torch.equal(torch.stack(la), torch.stack(lb))
    assert len(it._plan["lists"].phases) == 5 and it._plan["mdesc"] is None
    assert len(_native(b, _monitor(b))._signature(b.opt._signature())) == len(it._key) + 1          # the key as it was
    _assert_same_state(a, b, a.out, it.out)


# ------------------------------------------------------------------------------------------ 5. capacity
def test_capacity_is_refused_before_anything_is_issued(dev):
    b = _tiny(dev, "snail", noisy=True)
    mb = _monitor(b, capacity=4)
    it = _native(b, mb)
    assert it.run(4).shape == (4,)
    torch.cuda.synchronize()

    def frozen():
        return ([p.detach().clone() for p in b.net.parameters()], mb.records.clone(), mb.out_avg.clone(), mb.state.clone(),
                mb.counter.clone(), b.reg.offset.clone())

    before = frozen()
    with pytest.raises(RuntimeError, match="capacity"):
        it.step()
    with pytest.raises(RuntimeError, match="capacity"):
        it.run(1)
    torch.cuda.synchronize()
    after = frozen()
    for p, q in zip(before[0], after[0]):
        assert torch.equal(p, q)
    for x, y in zip(before[1:], after[1:]):
        assert torch.equal(x, y)
    assert mb.i == 4 and it.iterations == 4 and b.opt.step_count == 4 and b.opt.device_step_count() == 4
    # a fresh run that would only overflow at its end is refused as a whole
    c = _tiny(dev, "snail", noisy=True)
    mc = _monitor(c, capacity=4)
    itc = _native(c, mc)
    params = [p.detach().clone() for p in c.net.parameters()]
    with pytest.raises(RuntimeError, match="capacity"):
        itc.run(5)
    torch.cuda.synchronize()
    for p, q in zip(c.net.parameters(), params):
        assert torch.equal(p, q)
    assert mc.i == 0 and itc.iterations == 0 and c.opt.step_count == 0 and mc.counter.item() == 0
    assert torch.count_nonzero(mc.records).item() == 0


# ------------------------------------------------------------------------------------------ 6. refusals
def test_refusals(dev):
    from dip_optim import NativeIteration
    from utils.fit_monitor import FitMonitor
    b = _tiny(dev, "default")
    other = _tiny(dev, "default", seed=4)
    with pytest.raises(TypeError, match="dip-amd:.*FitMonitor"):
        NativeIteration(b.net, b.head, b.opt, b.z, monitor=object())
    with pytest.raises(ValueError, match="dip-amd:.*another net"):
        NativeIteration(b.net, b.head, b.opt, b.z, monitor=_monitor(other))
    # a monitor that does not back-track holds no engine: another net's is fine
    NativeIteration(b.net, b.head, b.opt, b.z, monitor=_monitor(other, backtracking=False))
    # the image shape is checked when the plan is built (the output size is known then), before anything is issued
    small = FitMonitor(b.net, b.target[:, :, :32, :48].contiguous(), None, show_every=SHOW_EVERY, capacity=4)
    it = NativeIteration(b.net, b.head, b.opt, b.z, monitor=small)
    with pytest.raises(ValueError, match="dip-amd:.*FitMonitor"):
        it.step()
    assert small.i == 0 and it.iterations == 0 and b.opt.step_count == 0
    it.monitor = object()
    with pytest.raises(TypeError, match="dip-amd:.*FitMonitor"):
        it.step()
    with pytest.raises(RuntimeError):                            # a monitor on the CPU cannot exist
        FitMonitor(b.net, b.target.cpu())


# ------------------------------------------------------------------------------------------ 7. rebuild
def test_replacing_the_monitors_buffers_or_the_monitor_rebuilds_the_plan(dev):
    a, b = _tiny(dev, "default", noisy=True), _tiny(dev, "default", noisy=True)
    ma, mb = _monitor(a, -1e30), _monitor(b, -1e30)
    it = _native(b, mb)
    la = [_eager_mon_step(a, ma) for _ in range(2)]
    lb = [it.step(), it.step()]
    lists0 = it._plan["lists"]
    for m in (ma, mb):
        m.out_avg = m.out_avg.clone()                            # a new buffer with the old values
    la.append(_eager_mon_step(a, ma)), lb.append(it.step())
    assert it._plan["lists"] is not lists0
    _assert_same(a, b, ma, mb, la, lb, it.out, "out_avg replaced")
    # another monitor on the same iteration object: its own records from row 0, its own counter
    ma2, mb2 = _monitor(a, -1e30, seed=12), _monitor(b, -1e30, seed=12)
    it.monitor = mb2
    lists1 = it._plan["lists"]
    la2 = [_eager_mon_step(a, ma2) for _ in range(3)]
    lb2 = list(it.run(3).unbind(0))
    assert it._plan["lists"] is not lists1
    _assert_same(a, b, ma2, mb2, la2, lb2, it.out, "monitor replaced")
    assert mb2.history()[:, 7].tolist() == [0., 0., 1.] and mb.i == 3 and mb.counter.item() == 3
    _assert_same_monitor(ma, mb, "the first monitor was left alone")
