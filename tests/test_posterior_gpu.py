"""utils.fit_monitor.PosteriorMonitor on a real MI355X: dip_posterior_dev (csrc/monitor_kernels.hip) against the numpy-float32
restatement of the Welford update (tests/sgld_ref.py), bitwise; NativeIteration(posterior=) against pm.update(out) in the eager
closure; that it does not touch the fit; its combination with monitor= and early_stop=; the sample cap."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sgld_ref as S  # noqa: E402
from test_group_monitor_gpu import _stream_pool_stands_where_it_stood  # noqa: E402,F401  (autouse: the engines of this module
#                                                                                          draw pooled streams too)
from test_native_iter_gpu import _assert_same_state  # noqa: E402
from test_native_monitor_gpu import _assert_same_monitor, _monitor  # noqa: E402
from test_sgld_fit_gpu import _mse_fit, _native  # noqa: E402

BURN_IN, EVERY, ITERS = 3, 2, 9                    # samples fall at iterations 3, 5 and 7


def _pm(dev, shape, burn_in=BURN_IN, every=EVERY):
    from utils.fit_monitor import PosteriorMonitor
    return PosteriorMonitor(torch.empty(shape, device=dev), burn_in, every)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 1, 1, 5), (1, 1, 13, 79), (1, 3, 36, 52)], ids=["n1", "n5", "n1027", "3x36x52"])
def test_kernel_equals_the_numpy_float32_restatement(dev, shape):
    pm = _pm(dev, shape)
    n = int(np.prod(shape))
    g = torch.Generator().manual_seed(n)
    mean, m2, k = np.zeros(n, np.float32), np.zeros(n, np.float32), 0
    with pytest.raises(RuntimeError, match="dip-amd:.*at least two samples"):
        pm.variance()
    for i in range(ITERS):
        x = torch.rand(shape, generator=g) + 0.1 * torch.randn(shape, generator=g)
        pm.update(x.to(dev))
        if S.is_sample(i, BURN_IN, EVERY):
            k += 1
            mean, m2 = S.welford(mean, m2, x.numpy().reshape(-1), k)
            if k == 1:                               # the first sample needs no special case
                assert np.array_equal(mean, x.numpy().reshape(-1)) and not m2.any()
        torch.cuda.synchronize()
        assert pm.count == k and pm.i == i + 1 and int(pm.counter.item()) == i + 1, i
        assert tuple(pm.mean.shape) == shape and tuple(pm.m2.shape) == shape
        assert np.array_equal(pm.mean.cpu().numpy().reshape(-1).view(np.int32), mean.view(np.int32)), i
        assert np.array_equal(pm.m2.cpu().numpy().reshape(-1).view(np.int32), m2.view(np.int32)), i
        if k == 0:
            assert not pm.mean.any() and not pm.m2.any(), i       # untouched before the burn-in ends
        if k < 2:
            with pytest.raises(RuntimeError, match="dip-amd:.*at least two samples"):
                pm.variance()
    assert pm.count == 3
    var = pm.variance()
    assert tuple(var.shape) == shape and np.array_equal(var.cpu().numpy().reshape(-1), m2 / np.float32(2))


def test_refusals_before_anything_is_issued(dev):
    pm = _pm(dev, (1, 3, 8, 8), 0, 1)
    with pytest.raises(ValueError, match="dip-amd: PosteriorMonitor.update: the PosteriorMonitor was built for"):
        pm.update(torch.zeros(1, 3, 8, 9, device=dev))
    with pytest.raises(ValueError, match="dip-amd: PosteriorMonitor.update: the output is on cpu"):
        pm.update(torch.zeros(1, 3, 8, 8))
    assert pm.i == 0 and pm.count == 0
    # the sample cap: burn_in 0, every 1 -- iteration 2**24 would be sample 2**24 + 1
    pm.i = 2 ** 24
    with pytest.raises(RuntimeError, match="dip-amd: PosteriorMonitor.*2\\*\\*24 samples"):
        pm.update(torch.zeros(1, 3, 8, 8, device=dev))
    pm.i = 2 ** 24 - 1
    pm._check_room(1)
    with pytest.raises(RuntimeError, match="dip-amd: PosteriorMonitor.*2\\*\\*24 samples"):
        pm._check_room(2)
    assert int(pm.counter.item()) == 0 and pm.count == 0
    # NativeIteration: another image shape, before anything is issued
    f = _mse_fit(dev)
    it = _native(f, posterior=_pm(dev, (1, 3, 8, 8)))
    with pytest.raises(ValueError, match="dip-amd: NativeIteration: the PosteriorMonitor was built for"):
        it.step()
    assert f.opt.step_count == 0


def _eager_pm_step(f, pm, mon=None, es=None):
    """test_native_iter_gpu._eager_step with the monitors' updates between backward() and opt.step(), in NativeIteration's
    order: monitor, early stopping, posterior."""
    f.opt.zero_grad()
    loss, out = f.head(f.reg())
    loss.backward()
    if mon is not None:
        mon.update(out, loss)
    if es is not None:
        es.update(out)
    pm.update(out)
    f.opt.step()
    f.out = out
    return loss.detach()


def _same_pm(pa, pb, what=""):
    torch.cuda.synchronize()
    assert pa.i == pb.i and pa.count == pb.count, what
    assert torch.equal(pa.mean, pb.mean) and torch.equal(pa.m2, pb.m2) and torch.equal(pa.counter, pb.counter), what


def test_native_iteration_equals_the_eager_update_and_leaves_the_fit_alone(dev):
    a, b, c, d = (_mse_fit(dev, wd=5e-8) for _ in range(4))
    shape = tuple(a.target.shape)
    pa, pb, pc = (_pm(dev, shape, 2, 2) for _ in range(3))
    la = [_eager_pm_step(a, pa) for _ in range(7)]
    itb = _native(b, posterior=pb)
    lb = itb.run(7)
    assert itb._plan["lists"].phases[-2].names == ["posterior_dev"]           # behind the backward list, in front of Adam
    assert torch.equal(torch.stack(la), lb)
    _same_pm(pa, pb)
    assert pa.count == 3 and pa.i == 7                              # iterations 2, 4, 6
    _assert_same_state(a, b, a.out, itb.out)
    # alternating eager and native on one monitor
    itc = _native(c, posterior=pc)
    lc = list(itc.run(3)) + [_eager_pm_step(c, pc), _eager_pm_step(c, pc)] + list(itc.run(2))
    assert torch.equal(torch.stack(la), torch.stack(lc))
    _same_pm(pa, pc, "alternating")
    _assert_same_state(a, c, a.out, itc.out, "alternating")
    # posterior=None: the same fit, and the key it had
    itd = _native(d)
    ld = itd.run(7)
    assert torch.equal(ld, lb)
    _assert_same_state(b, d, itb.out, itd.out, "posterior=None")
    assert len(itd._key) == 13 and len(itb._key) == 14 and itb._key[-1] == ("posterior", pb._plan_key())
    # the sample is the output of the parameters about to be stepped: the mean after one sample is that iteration's output
    e = _mse_fit(dev)
    pe = _pm(dev, shape, 0, 100)
    ite = _native(e, posterior=pe)
    ite.run(1)
    torch.cuda.synchronize()
    assert torch.equal(pe.mean, ite.out) and pe.count == 1


def test_combines_with_monitor_and_early_stop(dev):
    from utils.fit_monitor import EarlyStopMonitor
    a, b = _mse_fit(dev), _mse_fit(dev)
    shape = tuple(a.target.shape)
    pa, pb = _pm(dev, shape, 1, 2), _pm(dev, shape, 1, 2)
    ma, mb = _monitor(a), _monitor(b)
    ea, eb = (EarlyStopMonitor(f.target, window=3, patience=2, net=f.net, capacity=16) for f in (a, b))
    la = [_eager_pm_step(a, pa, ma, ea) for _ in range(6)]
    it = _native(b, monitor=mb, early_stop=eb, posterior=pb)
    lb = it.run(6)
    names = [ph.names[0] for ph in it._plan["lists"].phases[-4:]]
    assert names == ["fit_monitor_dev", "early_stop_dev", "posterior_dev", "adam_tick"]
    assert torch.equal(torch.stack(la), lb)
    _same_pm(pa, pb)
    _assert_same_monitor(ma, mb)
    assert torch.equal(ea.records, eb.records) and torch.equal(ea.state, eb.state) and torch.equal(ea.best_out, eb.best_out)
    _assert_same_state(a, b, a.out, it.out)
    assert pa.count == 3
