"""GPU suite of the early-stopping monitor (utils.fit_monitor.EarlyStopMonitor; dip_early_stop_dev / dip_early_stop_keep;
NativeIteration(early_stop=) and run_until): the windowed moving variance of the net output on the device against the numpy
fp64 two-pass restatement of the contract (tests/early_stop_ref.py).

1. the entry point on raw buffers against the reference: records, decisions, best_out, the ring, sentinel tails, determinism;
2. edge cases: a constant sequence, W = 2 / P = 1, a NaN output, the capacity;
3. the eager closure with es.update(out) is bit-identical to NativeIteration(early_stop=), and the two alternate;
4. early_stop= does not touch the fit, with and without monitor=FitMonitor;
5. run_until against decisions taken on the host from the eager outputs; restore_best();
6. the refusals that need a device."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_group_monitor_gpu import _stream_pool_stands_where_it_stood  # noqa: E402,F401  (autouse: the engines of this
#                                                      module draw pooled streams; the pool is left where it stood)
from test_native_iter_gpu import _assert_same_state  # noqa: E402

import dip_native as N  # noqa: E402
import early_stop_ref as R  # noqa: E402

W, P, T = 5, 9, 60
TAIL = 67                    # sentinel floats behind every buffer the kernels write
SENT = -77.25
SHAPES = [(3, 37, 29), (1, 8, 8), (3, 96, 128)]
_REF = {}


def _reference(shape):
    """The sequence of a shape and its fp64 reference, computed once and shared (read-only)."""
    if shape not in _REF:
        xs = R.sequence(shape, T=T, seed=0)
        xs.setflags(write=False)
        _REF[shape] = (xs,) + R.wmv_reference(xs, W, P)
    return _REF[shape]


class _Raw:
    """dip_early_stop_dev over buffers of the test's own, each with a sentinel tail behind it."""

    def __init__(self, dev, lib, n, window, patience, capacity):
        from utils.fit_monitor import early_stop_state
        self.lib, self.n, self.window = lib, n, window
        f32 = lambda k: torch.full((k + TAIL,), SENT, dtype=torch.float32, device=dev)  # noqa: E731
        self.out, self.ring, self.best = f32(n), f32(window * n), f32(n)
        self.mean = torch.full((n + TAIL,), SENT, dtype=torch.float64, device=dev)
        self.nblk = lib.dip_fit_monitor_nblk(n)
        self.partial = torch.full((self.nblk + TAIL,), SENT, dtype=torch.float64, device=dev)
        self.records = torch.full((capacity * 5 + TAIL,), SENT, dtype=torch.float32, device=dev)
        self.state = early_stop_state(dev)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.capacity = capacity
        self.desc = N.DipEarlyStopDesc(self.out.data_ptr(), self.ring.data_ptr(), self.mean.data_ptr(), self.partial.data_ptr(),
                                       self.records.data_ptr(), self.state.data_ptr(), self.counter.data_ptr(),
                                       self.best.data_ptr(), n, window, patience, capacity, None)

    def feed(self, xs_dev):
        stream = torch.cuda.current_stream().cuda_stream
        for x in xs_dev:
            self.out[:self.n].copy_(x)
            N.check(self.lib.dip_early_stop_dev(ctypes.byref(self.desc), stream), "early_stop_dev")
        torch.cuda.synchronize()

    def rows(self, k):
        return self.records[:5 * k].view(k, 5).cpu().numpy()

    def tails_untouched(self):
        n, w = self.n, self.window
        for name, buf, used in (("out", self.out, n), ("ring", self.ring, w * n), ("best_out", self.best, n),
                                ("mean", self.mean, n), ("partial", self.partial, self.nblk),
                                ("records", self.records, 5 * self.capacity)):
            assert torch.all(buf[used:] == SENT).item(), name


# ------------------------------------------------------------------------------------------ 1. the entry point against fp64
@pytest.mark.parametrize("shape", SHAPES, ids=["3x37x29-4blocks", "1x8x8-1block", "3x96x128-36blocks"])
def test_entry_point_against_numpy_fp64(dev, built, shape):
    n = int(np.prod(shape))
    nblk = built.dip_fit_monitor_nblk(n)
    assert nblk == {3219: 4, 64: 1, 36864: 36}[n]
    if shape == (3, 37, 29):
        assert nblk > 1 and n % 2 == 1
    xs, ref, stop, margins = _reference(shape)
    # the reference's own decisions: the ones the issue states, none of them near a tie
    assert (int(ref[-1, 2]), stop) == (19, 28)
    assert min(margins) >= 1e-3
    xd = torch.tensor(xs).to(dev)                                    # (a copy: the shared reference stays read-only)
    raw = _Raw(dev, built, n, W, P, T)
    raw.feed(xd)
    got = raw.rows(T)
    # warm-up rows
    for t in range(W - 1):
        assert got[t].tolist() == [math.inf, math.inf, -1.0, 0.0, 0.0], t
    worst = 0.0
    for t in range(W - 1, T):
        for c in (0, 1):
            err = abs(float(got[t, c]) - ref[t, c])
            worst = max(worst, err / ref[t, c])
            assert err <= 2 * R.EPS32 * ref[t, c], (t, c, float(got[t, c]), ref[t, c])
        assert got[t, 2:].tolist() == ref[t, 2:].tolist(), (t, got[t].tolist(), ref[t].tolist())
    print(f"[early_stop {shape}] worst relative error of var / var_min: {worst:.3e} (bound {2 * R.EPS32:.3e})")
    for t in range(29, T):                                            # rows after the stopping iteration repeat its row
        assert np.array_equal(got[t], got[28]), t
    assert got[28, 4] == 1.0 and got[27, 4] == 0.0
    assert raw.counter.item() == T
    # best_out is x_19, bit for bit; the ring holds x_24..x_28 in their slots and none of the later inputs
    assert torch.equal(raw.best[:n], xd[19])
    ring = raw.ring[:W * n].view(W, n)
    for t in range(24, 29):
        assert torch.equal(ring[t % W], xd[t]), t
    st = raw.state.cpu()
    assert st[6:12].tolist() == [29 % W, W, P, 19, 1, 0]              # head, fill, wait, best_iter, stopped, improved
    assert st.view(torch.float64)[1].item() == pytest.approx(ref[28, 1], rel=1e-12)
    raw.tails_untouched()
    # determinism: the same sequence again, bit-identical records
    again = _Raw(dev, built, n, W, P, T)
    again.feed(xd)
    assert torch.equal(again.records, raw.records) and torch.equal(again.state, raw.state)
    assert torch.equal(again.best, raw.best) and torch.equal(again.ring, raw.ring) and torch.equal(again.mean, raw.mean)


def test_keep_copies_on_the_flag_only_and_writes_no_tail(dev, built):
    """dip_early_stop_keep: any n, any 4-byte alignment (the quad path needs both buffers 16-byte aligned)."""
    from utils.fit_monitor import early_stop_state
    stream = torch.cuda.current_stream().cuda_stream
    for n, off_s, off_d in ((3219, 0, 0), (3219, 1, 0), (3219, 0, 3), (1, 0, 0), (1027, 2, 2), (4096, 0, 0)):
        src = torch.rand(n + 8, device=dev)
        dst = torch.full((n + 8 + TAIL,), SENT, device=dev)
        st = early_stop_state(dev)
        args = (src[off_s:].data_ptr(), dst[off_d:].data_ptr(), n, st.data_ptr(), stream)
        N.check(built.dip_early_stop_keep(*args), "early_stop_keep")
        assert torch.all(dst == SENT).item(), (n, off_s, off_d)          # improved = 0: nothing
        st[11] = 1
        N.check(built.dip_early_stop_keep(*args), "early_stop_keep")
        assert torch.equal(dst[off_d:off_d + n], src[off_s:off_s + n]), (n, off_s, off_d)
        assert torch.all(dst[:off_d] == SENT).item() and torch.all(dst[off_d + n:] == SENT).item(), (n, off_s, off_d)


# ------------------------------------------------------------------------------------------ 2. edge cases
SHAPE = (3, 37, 29)


def _monitor(dev, **kw):
    from utils.fit_monitor import EarlyStopMonitor
    return EarlyStopMonitor(torch.empty(1, *SHAPE, device=dev), **kw)


def test_constant_sequence(dev, built):
    es = _monitor(dev, window=W, patience=P, capacity=32)
    x = torch.full((1, *SHAPE), 0.3, device=dev)
    for _ in range(W + P + 3):
        es.update(x)
    h = es.history()
    assert h.shape == (W + P + 3, 5)
    assert h[W - 1].tolist() == [0.0, 0.0, W - 1, 0.0, 0.0]           # var == 0.0 exactly
    assert h[W - 1 + P].tolist() == [0.0, 0.0, W - 1, P, 1.0]         # 0 < 0 is false: wait runs to P
    assert h[W - 2 + P, 4] == 0.0 and np.array_equal(h[-1], h[W - 1 + P])
    assert (es.best_iter, es.stopped) == (W - 1, 1)
    assert es.last() == dict(var=0.0, var_min=0.0, best_iter=W - 1, wait=P, stopped=1.0)


def test_smallest_window_and_patience(dev, built):
    xs = R.sequence(SHAPE, T=24, seed=3)[10:]                         # 14 outputs around the amplitude's minimum (t = 17)
    ref, stop, margins = R.wmv_reference(xs, 2, 1)
    assert stop is not None and stop < 13 and min(margins) >= 1e-3
    es = _monitor(dev, window=2, patience=1, capacity=14)
    xd = torch.tensor(xs).to(dev).view(14, 1, *SHAPE)
    for x in xd:
        es.update(x)
    h = es.history()
    assert h[0].tolist() == [math.inf, math.inf, -1.0, 0.0, 0.0]
    for t in range(1, 14):
        assert abs(h[t, 0] - ref[t, 0]) <= 2 * R.EPS32 * ref[t, 0] and abs(h[t, 1] - ref[t, 1]) <= 2 * R.EPS32 * ref[t, 1], t
        assert h[t, 2:].tolist() == ref[t, 2:].tolist(), t
    assert es.stopped == 1 and es.best_iter == int(ref[-1, 2])
    assert torch.equal(es.best_out, xd[es.best_iter])


def test_nan_output_takes_no_minimum_and_advances_wait(dev, built):
    xs = R.sequence(SHAPE, T=16, seed=0)                              # the variance falls all the way: a minimum per iteration
    es = _monitor(dev, window=W, patience=P, capacity=16)
    xd = torch.from_numpy(xs).to(dev).view(16, 1, *SHAPE)
    for t in range(8):
        es.update(xd[t])
    before = es.last()
    best_out = es.best_out.clone()
    assert before["best_iter"] == 7 and before["wait"] == 0
    bad = xd[8].clone()
    bad.view(-1)[1234] = float("nan")
    es.update(bad)
    for t in range(9, 8 + W):                                         # the NaN is in the window: every formulation says NaN
        es.update(xd[t])
    h = es.history()
    for k, t in enumerate(range(8, 8 + W)):
        assert math.isnan(h[t, 0]), t
        assert h[t, 1] == np.float32(before["var_min"]) and h[t, 2] == 7 and h[t, 3] == k + 1 and h[t, 4] == 0, (t, h[t].tolist())
    assert torch.equal(es.best_out, best_out) and es.best_iter == 7


def test_capacity_is_refused_and_leaves_the_state_unchanged(dev, built):
    es = _monitor(dev, window=3, patience=20, capacity=8)
    xs = torch.from_numpy(R.sequence(SHAPE, T=9, seed=1)).to(dev).view(9, 1, *SHAPE)
    for t in range(8):
        es.update(xs[t])
    torch.cuda.synchronize()
    keep = [t.clone() for t in (es.records, es.state, es.counter, es.ring, es.mean, es.best_out)]
    with pytest.raises(RuntimeError, match="dip-amd: EarlyStopMonitor capacity exceeded"):
        es.update(xs[8])
    torch.cuda.synchronize()
    assert es.i == 8 and es.counter.item() == 8
    for a, b in zip(keep, (es.records, es.state, es.counter, es.ring, es.mean, es.best_out)):
        assert torch.equal(a, b)
    # the device-side guard: a counter at the capacity writes nothing but improved <- 0
    es.state[11] = 1
    keep[1][11] = 0
    d = es._dev_descriptor(xs[8].contiguous())
    N.check(built.dip_early_stop_dev(ctypes.byref(d), torch.cuda.current_stream().cuda_stream), "early_stop_dev")
    torch.cuda.synchronize()
    for a, b in zip(keep, (es.records, es.state, es.counter, es.ring, es.mean, es.best_out)):
        assert torch.equal(a, b)
    # shape / device mismatches
    with pytest.raises(ValueError, match="dip-amd: EarlyStopMonitor.update"):
        _monitor(dev).update(torch.zeros(1, 3, 37, 30, device=dev))
    with pytest.raises(ValueError, match="dip-amd: EarlyStopMonitor.update"):
        _monitor(dev).update(torch.zeros(1, *SHAPE))
    m = _monitor(dev, window=4, patience=2)
    assert m.memory_bytes >= 4 * 4 * 3219 + 8 * 3219 + 4 * 3219
    with pytest.raises(RuntimeError, match="dip-amd: EarlyStopMonitor.restore_best needs net="):
        m.restore_best()


# ------------------------------------------------------------------------------------------ the fits of 3. - 6.
HW = (32, 48)
ES_KW = dict(window=4, patience=6)


def _net(seed):
    from models.skip import skip
    torch.manual_seed(seed)
    return skip(4, 3, num_channels_down=[8, 8], num_channels_up=[8, 8], num_channels_skip=[4, 4],
                upsample_mode="bilinear", need_sigmoid=True, need_bias=True, pad="reflection")


class _Fit:
    """A tiny denoising fit: RegNoise(std = 1/30) + MSEHead + FusedAdam; `es` = an EarlyStopMonitor(net=net) or None."""

    def __init__(self, dev, early_stop=True, capacity=256, hw=HW, **es_kw):
        from dip_optim import FusedAdam
        from utils.common_utils import get_params
        from utils.fit_monitor import EarlyStopMonitor
        from utils.loss_head import MSEHead
        from utils.reg_noise import RegNoise
        g = torch.Generator().manual_seed(4)
        self.dev = dev
        self.net = _net(3).to(dev)
        self.z = (torch.rand(1, 4, *hw, generator=g) * 0.1).to(dev)
        self.img = torch.rand(1, 3, *hw, generator=g).to(dev)
        self.head = MSEHead(self.net, self.img)
        self.reg = RegNoise(self.z, 1 / 30, seed=7)
        self.opt = FusedAdam(get_params('net', self.net, self.z), lr=0.01)
        self.es = EarlyStopMonitor(self.img, net=self.net, capacity=capacity, **dict(ES_KW, **es_kw)) if early_stop else None
        self.out = None

    def eager(self, mon=None, keep=None):
        """opt.zero_grad(); loss, out = head(x); loss.backward(); [mon.update(out, loss);] [es.update(out);] opt.step()"""
        self.opt.zero_grad()
        loss, out = self.head(self.reg())
        loss.backward()
        self.out = out
        if mon is not None:
            mon.update(out, loss)
        if self.es is not None:
            self.es.update(out)
        if keep is not None:
            keep.append(out.detach().clone())
        self.opt.step()
        return loss.detach()

    def native(self, **kw):
        from dip_optim import NativeIteration
        return NativeIteration(self.net, self.head, self.opt, self.z, reg_noise=self.reg, early_stop=self.es, **kw)

    def params(self):
        return self.net.__dict__["_dip_engine"].params


def _assert_same_es(a, b, what=""):
    torch.cuda.synchronize()
    assert a.i == b.i, what
    assert torch.equal(a.records, b.records), (what, a.history().tolist(), b.history().tolist())
    for k in ("state", "counter", "ring", "mean", "best_out", "best_params"):
        assert torch.equal(getattr(a, k), getattr(b, k)), (what, k)


# ------------------------------------------------------------------------------------------ 3. eager closure == native
def test_native_is_bit_identical_to_the_eager_closure_with_update(dev):
    a, b, c = _Fit(dev), _Fit(dev), _Fit(dev)
    la = [a.eager() for _ in range(40)]
    it = b.native()
    lb = it.run(40)
    assert torch.equal(torch.stack(la), lb)
    _assert_same_es(a.es, b.es, "eager vs native")
    _assert_same_state(a, b, a.out, it.out, "eager vs native")
    h = a.es.history()
    assert h.shape == (40, 5) and np.all(np.isinf(h[:3, 0])) and np.all(np.isfinite(h[3:, 0])) and h[-1, 2] >= 3
    assert torch.count_nonzero(a.es.best_params).item() > 0
    # 13 eager, 14 native, 13 eager on one monitor
    lc = [c.eager() for _ in range(13)]
    itc = c.native()
    lc += list(itc.run(14))
    lc += [c.eager() for _ in range(13)]
    assert torch.equal(torch.stack(lc), lb)
    _assert_same_es(c.es, b.es, "alternating vs native")
    _assert_same_state(c, b, c.out, it.out, "alternating vs native")


# ------------------------------------------------------------------------------------------ 4. non-interference
@pytest.mark.parametrize("with_monitor", [False, True], ids=["monitor=None", "monitor=FitMonitor"])
def test_early_stop_does_not_touch_the_fit(dev, with_monitor):
    from utils.fit_monitor import FitMonitor
    a, b = _Fit(dev, early_stop=False), _Fit(dev)
    ma = FitMonitor(a.net, a.img, show_every=5, capacity=64) if with_monitor else None
    mb = FitMonitor(b.net, b.img, show_every=5, capacity=64) if with_monitor else None
    ita, itb = a.native(monitor=ma), b.native(monitor=mb)
    assert len(itb._signature(())) == len(ita._signature(())) + 1          # early_stop=None: the key as it was
    la, lb = ita.run(30), itb.run(30)
    assert torch.equal(la, lb)
    _assert_same_state(a, b, ita.out, itb.out, "early_stop= vs None")
    assert b.es.i == 30 and b.es.best_iter >= 3
    if with_monitor:
        assert ma.i == mb.i == 30 and torch.equal(ma.records, mb.records) and torch.equal(ma.state, mb.state)
        assert torch.equal(ma.out_avg, mb.out_avg) and torch.equal(ma.snapshot, mb.snapshot)
        assert ita._plan["lists"].n == 6 and itb._plan["lists"].n == 7
    else:
        assert ita._plan["lists"].n == 5 and itb._plan["lists"].n == 6


# ------------------------------------------------------------------------------------------ 5. run_until
def test_run_until_against_host_decisions(dev):
    a = _Fit(dev, early_stop=False)
    outs = []
    for _ in range(200):
        a.eager(keep=outs)
    torch.cuda.synchronize()
    xs = torch.stack(outs).reshape(200, -1).cpu().numpy()
    ref, stop, margins = R.wmv_reference(xs, ES_KW["window"], ES_KW["patience"])
    best = int(ref[-1, 2])
    b = _Fit(dev)
    it = b.native()
    issued, losses = it.run_until(200, check_every=7)
    print(f"[run_until] reference: best_iter {best}, stop {stop}, smallest decision margin {min(margins):.2e}; issued {issued}")
    assert losses.shape == (issued,) and it.iterations == issued == b.es.i
    if stop is not None:
        assert issued == min(200, 7 * math.ceil((stop + 1) / 7))
        assert b.es.stopped == 1
        h = b.es.history()
        assert h[stop, 4] == 1.0 and (stop == 0 or h[stop - 1, 4] == 0.0)
    else:
        assert issued == 200 and b.es.stopped == 0
    assert b.es.best_iter == best
    assert torch.equal(b.es.best_out, outs[best])
    # restore_best(): the net carries the parameters of iteration best_iter again
    twin = _Fit(dev, early_stop=False)
    for _ in range(best):
        twin.eager()
    b.es.restore_best()
    assert torch.equal(b.params(), twin.params())
    assert torch.equal(b.net(b.z).detach(), twin.net(twin.z).detach())
    fresh = _Fit(dev)
    with pytest.raises(RuntimeError, match="dip-amd: EarlyStopMonitor.restore_best: no minimum"):
        fresh.es.restore_best()


# ------------------------------------------------------------------------------------------ 6. guards on the device
def test_guards(dev):
    from dip_optim import NativeIteration
    from utils.fit_monitor import EarlyStopMonitor
    f, other = _Fit(dev, capacity=5), _Fit(dev)
    mk = lambda es: NativeIteration(f.net, f.head, f.opt, f.z, reg_noise=f.reg, early_stop=es)  # noqa: E731
    with pytest.raises(ValueError, match="dip-amd: the EarlyStopMonitor keeps the parameters of another net"):
        mk(other.es)
    with pytest.raises(ValueError, match="dip-amd: NativeIteration: the EarlyStopMonitor was built for"):
        mk(EarlyStopMonitor(torch.empty(1, 3, 32, 50, device=dev), **ES_KW)).step()
    plain = NativeIteration(f.net, f.head, f.opt, f.z, reg_noise=f.reg)
    with pytest.raises(RuntimeError, match="dip-amd: NativeIteration.run_until needs early_stop="):
        plain.run_until(10)
    # past the capacity: refused before anything is issued
    it = f.native()
    it.run(3)
    torch.cuda.synchronize()
    params, recs, step = f.params().clone(), f.es.records.clone(), f.opt.step_count
    for call in (lambda: it.run(3), lambda: it.run_until(3, check_every=1)):
        with pytest.raises(RuntimeError, match="dip-amd: EarlyStopMonitor capacity exceeded"):
            call()
    torch.cuda.synchronize()
    assert torch.equal(f.params(), params) and torch.equal(f.es.records, recs)
    assert (f.es.i, it.iterations, f.opt.step_count, f.es.counter.item()) == (3, 3, step, 3)
    it.run(2)
    assert f.es.i == 5


def test_monitor_on_another_device_is_refused(dev):
    from dip_optim import NativeIteration
    from utils.fit_monitor import EarlyStopMonitor
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    f = _Fit(dev, early_stop=False)
    with pytest.raises(RuntimeError, match="dip-amd: the EarlyStopMonitor lives on"):
        NativeIteration(f.net, f.head, f.opt, f.z, reg_noise=f.reg,
                        early_stop=EarlyStopMonitor(torch.empty(1, 3, *HW, device="cuda:1"), **ES_KW))
