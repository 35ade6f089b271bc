"""GPU suite of the ring-free early-stopping criterion (dip_early_stop_emv_dev; utils.fit_monitor.EarlyStopMonitor(mode='emv');
NativeIteration(early_stop=) and run_until): the exponential moving variance of the net output on the device against the numpy
fp64 restatement of the contract (tests/early_stop_emv_ref.py).

1. the entry point on raw buffers against the reference: records, decisions, best_out, the frozen mean and v, sentinel tails,
   determinism;
2. edge cases: a constant sequence, warmup = 1 / patience = 1, a NaN output, the capacity;
3. the public interface: the eager closure with es.update(out) is bit-identical to NativeIteration(early_stop=), the two
   alternate, the fit is untouched, run_until against decisions taken on the host from the eager outputs, restore_best()."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_group_monitor_gpu import _stream_pool_stands_where_it_stood  # noqa: E402,F401  (autouse: the engines of this
#                                                      module draw pooled streams; the pool is left where it stood)
from test_early_stop_gpu import _Fit  # noqa: E402
from test_native_iter_gpu import _assert_same_state  # noqa: E402

import dip_native as N  # noqa: E402
import early_stop_emv_ref as E  # noqa: E402
import early_stop_ref as R  # noqa: E402

ALPHA, WARM, P, T = 0.25, 8, 9, 60
BEST, STOP = 20, 29
TAIL = 67                    # sentinel elements behind every buffer the kernels write
SENT = -77.25
SHAPES = [(3, 37, 29), (1, 8, 8), (3, 96, 128)]
_REF = {}


def _reference(shape):
    """S_0 of a shape and its fp64 reference, computed once and shared (read-only)."""
    if shape not in _REF:
        xs = E.group_sequence(shape, 0)
        xs.setflags(write=False)
        st = {}
        _REF[shape] = (xs,) + E.emv_reference(xs, ALPHA, WARM, P, state=st) + (st,)
    return _REF[shape]


class _Raw:
    """dip_early_stop_emv_dev over buffers of the test's own, each with a sentinel tail behind it."""

    def __init__(self, dev, lib, n, alpha, warmup, patience, capacity):
        from utils.fit_monitor import early_stop_state
        self.lib, self.n = lib, n
        f32 = lambda k: torch.full((k + TAIL,), SENT, dtype=torch.float32, device=dev)  # noqa: E731
        self.out, self.best = f32(n), f32(n)
        self.mean = torch.full((n + TAIL,), SENT, dtype=torch.float64, device=dev)
        self.nblk = lib.dip_fit_monitor_nblk(n)
        self.partial = torch.full((self.nblk + TAIL,), SENT, dtype=torch.float64, device=dev)
        self.records = torch.full((capacity * 5 + TAIL,), SENT, dtype=torch.float32, device=dev)
        self.state = early_stop_state(dev)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.capacity = capacity
        self.desc = N.DipEarlyStopEmvDesc(self.out.data_ptr(), self.mean.data_ptr(), self.partial.data_ptr(),
                                          self.records.data_ptr(), self.state.data_ptr(), self.counter.data_ptr(),
                                          self.best.data_ptr(), n, alpha, warmup, patience, capacity, 0)

    def feed(self, xs_dev):
        stream = torch.cuda.current_stream().cuda_stream
        for x in xs_dev:
            self.out[:self.n].copy_(x)
            N.check(self.lib.dip_early_stop_emv_dev(ctypes.byref(self.desc), stream), "early_stop_emv_dev")
        torch.cuda.synchronize()

    def rows(self, k):
        return self.records[:5 * k].view(k, 5).cpu().numpy()

    def tails_untouched(self):
        for name, buf, used in (("out", self.out, self.n), ("best_out", self.best, self.n), ("mean", self.mean, self.n),
                                ("partial", self.partial, self.nblk), ("records", self.records, 5 * self.capacity)):
            assert torch.all(buf[used:] == SENT).item(), name


# ------------------------------------------------------------------------------------------ 1. the entry point against fp64
@pytest.mark.parametrize("shape", SHAPES, ids=["3x37x29-4blocks", "1x8x8-1block", "3x96x128-36blocks"])
def test_entry_point_against_numpy_fp64(dev, built, shape):
    n = int(np.prod(shape))
    nblk = built.dip_fit_monitor_nblk(n)
    assert nblk == {3219: 4, 64: 1, 36864: 36}[n]
    xs, ref, stop, margins, final = _reference(shape)
    # the reference's own decisions: the ones the issue states, none of them near a tie
    assert (int(ref[-1, 2]), stop) == (BEST, STOP)
    assert min(margins) >= 1e-2
    xd = torch.tensor(xs).to(dev)                                    # (a copy: the shared reference stays read-only)
    raw = _Raw(dev, built, n, ALPHA, WARM, P, T)
    raw.feed(xd[:STOP + 1])
    at_stop = (raw.mean.clone(), raw.state.clone(), raw.best.clone())
    raw.feed(xd[STOP + 1:])
    got = raw.rows(T)
    for t in range(WARM):                                            # rows before the warm-up
        assert got[t].tolist() == [math.inf, math.inf, -1.0, 0.0, 0.0], t
    worst = 0.0
    for t in range(WARM, T):
        for c in (0, 1):
            err = abs(float(got[t, c]) - ref[t, c])
            worst = max(worst, err / ref[t, c])
            assert err <= 2 * R.EPS32 * ref[t, c], (t, c, float(got[t, c]), ref[t, c])
        assert got[t, 2:].tolist() == ref[t, 2:].tolist(), (t, got[t].tolist(), ref[t].tolist())
    print(f"[early_stop_emv {shape}] worst relative error of var / var_min: {worst:.3e} (bound {2 * R.EPS32:.3e})")
    for t in range(STOP + 1, T):                                     # rows after the stopping iteration repeat its row
        assert np.array_equal(got[t], got[STOP]), t
    assert got[STOP, 4] == 1.0 and got[STOP - 1, 4] == 0.0
    assert raw.counter.item() == T
    # best_out is x_20, bit for bit; the mean and v are frozen at the stopping iteration and are the reference's
    assert torch.equal(raw.best[:n], xd[BEST])
    for a, b in zip(at_stop, (raw.mean, raw.state, raw.best)):
        assert torch.equal(a, b)
    st = raw.state.cpu()
    assert st[6:12].tolist() == [0, 1, P, BEST, 1, 0]                 # head (unused), fill, wait, best_iter, stopped, improved
    f64 = st.view(torch.float64)
    assert f64[0].item() == pytest.approx(final["v"], rel=1e-12)
    assert f64[1].item() == pytest.approx(ref[STOP, 1], rel=1e-12) and f64[2].item() == pytest.approx(ref[STOP, 0], rel=1e-12)
    assert np.allclose(raw.mean[:n].cpu().numpy(), final["mu"], rtol=1e-12, atol=0)
    raw.tails_untouched()
    # determinism: the same sequence again, bit-identical
    again = _Raw(dev, built, n, ALPHA, WARM, P, T)
    again.feed(xd)
    assert torch.equal(again.records, raw.records) and torch.equal(again.state, raw.state)
    assert torch.equal(again.best, raw.best) and torch.equal(again.mean, raw.mean)


# ------------------------------------------------------------------------------------------ 2. edge cases
SHAPE = (3, 37, 29)


def _monitor(dev, **kw):
    from utils.fit_monitor import EarlyStopMonitor
    return EarlyStopMonitor(torch.empty(1, *SHAPE, device=dev), mode="emv", **kw)


def test_constant_sequence(dev, built):
    w, p = 4, 6
    es = _monitor(dev, alpha=ALPHA, warmup=w, patience=p, capacity=32)
    assert es.ring is None and es.memory_bytes < 13 * 3219 + 4 * 5 * 32 + 4096       # 8 n mean + 4 n best_out + small
    x = torch.full((1, *SHAPE), 0.3, device=dev)
    for _ in range(w + p + 3):
        es.update(x)
    h = es.history()
    assert h.shape == (w + p + 3, 5)
    assert h[w - 1].tolist() == [math.inf, math.inf, -1.0, 0.0, 0.0]
    assert h[w].tolist() == [0.0, 0.0, w, 0.0, 0.0]                   # var == 0.0 exactly
    assert h[w + p].tolist() == [0.0, 0.0, w, p, 1.0]                 # 0 < 0 is false: wait runs to P
    assert h[w + p - 1, 4] == 0.0 and np.array_equal(h[-1], h[w + p])
    assert (es.best_iter, es.stopped) == (w, 1)
    assert es.last() == dict(var=0.0, var_min=0.0, best_iter=w, wait=p, stopped=1.0)


def test_smallest_warmup_and_patience(dev, built):
    xs = R.sequence(SHAPE, T=24, seed=3)[10:]                         # 14 outputs around the amplitude's minimum (t = 17)
    ref, stop, margins = E.emv_reference(xs, ALPHA, 1, 1)
    assert stop is not None and stop < 13 and min(margins) >= 1e-3
    es = _monitor(dev, alpha=ALPHA, warmup=1, patience=1, capacity=14)
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
    xs = R.sequence(SHAPE, T=20, seed=0)                              # the variance falls all the way: a minimum per iteration
    ref, _, _ = E.emv_reference(xs[:12], ALPHA, WARM, 4)
    assert ref[11, 2] == 11 and ref[11, 3] == 0                       # (precondition, on the reference alone)
    es = _monitor(dev, alpha=ALPHA, warmup=WARM, patience=4, capacity=20)
    xd = torch.from_numpy(xs).to(dev).view(20, 1, *SHAPE)
    for t in range(12):
        es.update(xd[t])
    before = es.last()
    best_out = es.best_out.clone()
    assert before["best_iter"] == 11 and before["wait"] == 0
    bad = xd[12].clone()
    bad.view(-1)[1234] = float("nan")
    es.update(bad)
    for t in range(13, 18):                                           # v keeps the NaN: the fit stops after `patience`
        es.update(xd[t])
    h = es.history()
    for k, t in enumerate(range(12, 16)):
        assert math.isnan(h[t, 0]), t
        assert h[t, 1] == np.float32(before["var_min"]) and h[t, 2] == 11 and h[t, 3] == k + 1, (t, h[t].tolist())
        assert h[t, 4] == (1.0 if k == 3 else 0.0), (t, h[t].tolist())
    assert np.array_equal(h[16][1:], h[15][1:]) and np.array_equal(h[17][1:], h[15][1:])
    assert torch.equal(es.best_out, best_out) and (es.best_iter, es.stopped) == (11, 1)


def test_capacity_is_refused_and_leaves_the_state_unchanged(dev, built):
    es = _monitor(dev, alpha=ALPHA, warmup=2, patience=20, capacity=8)
    xs = torch.from_numpy(R.sequence(SHAPE, T=9, seed=1)).to(dev).view(9, 1, *SHAPE)
    for t in range(8):
        es.update(xs[t])
    torch.cuda.synchronize()
    bufs = lambda: (es.records, es.state, es.counter, es.mean, es.best_out)  # noqa: E731
    keep = [t.clone() for t in bufs()]
    with pytest.raises(RuntimeError, match="dip-amd: EarlyStopMonitor capacity exceeded"):
        es.update(xs[8])
    torch.cuda.synchronize()
    assert es.i == 8 and es.counter.item() == 8
    for a, b in zip(keep, bufs()):
        assert torch.equal(a, b)
    # the device-side guard: a counter at the capacity writes nothing but improved <- 0
    es.state[11] = 1
    keep[1][11] = 0
    d = es._dev_descriptor(xs[8].contiguous())
    assert isinstance(d, N.DipEarlyStopEmvDesc)
    N.check(built.dip_early_stop_emv_dev(ctypes.byref(d), torch.cuda.current_stream().cuda_stream), "early_stop_emv_dev")
    torch.cuda.synchronize()
    for a, b in zip(keep, bufs()):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------ 3. the public interface
EMV_KW = dict(mode="emv", alpha=ALPHA, warmup=WARM, patience=6)


def _assert_same_es(a, b, what=""):
    torch.cuda.synchronize()
    assert a.i == b.i and a.ring is None and b.ring is None, what
    assert torch.equal(a.records, b.records), (what, a.history().tolist(), b.history().tolist())
    for k in ("state", "counter", "mean", "best_out", "best_params"):
        assert torch.equal(getattr(a, k), getattr(b, k)), (what, k)


def test_native_is_bit_identical_to_the_eager_closure_with_update(dev):
    a, b, c, plain = _Fit(dev, **EMV_KW), _Fit(dev, **EMV_KW), _Fit(dev, **EMV_KW), _Fit(dev, early_stop=False)
    assert a.es.mode == "emv" and a.es.ring is None
    la = [a.eager() for _ in range(40)]
    it = b.native()
    lb = it.run(40)
    assert [name for name in it._plan["lists"].phases[-2].names] == ["early_stop_emv_dev", "early_stop_keep"]
    assert torch.equal(torch.stack(la), lb)
    _assert_same_es(a.es, b.es, "eager vs native")
    _assert_same_state(a, b, a.out, it.out, "eager vs native")
    h = a.es.history()
    assert h.shape == (40, 5) and np.all(np.isinf(h[:WARM, 0])) and np.all(np.isfinite(h[WARM:, 0])) and h[-1, 2] >= WARM
    assert torch.count_nonzero(a.es.best_params).item() > 0
    # 13 eager, 14 native, 13 eager on one monitor
    lc = [c.eager() for _ in range(13)]
    itc = c.native()
    lc += list(itc.run(14))
    lc += [c.eager() for _ in range(13)]
    assert torch.equal(torch.stack(lc), lb)
    _assert_same_es(c.es, b.es, "alternating vs native")
    _assert_same_state(c, b, c.out, it.out, "alternating vs native")
    # the fit against early_stop=None
    itp = plain.native()
    assert torch.equal(itp.run(40), lb)
    _assert_same_state(plain, b, itp.out, it.out, "early_stop=None vs emv")


def test_run_until_against_host_decisions(dev):
    a = _Fit(dev, early_stop=False)
    outs, arenas = [], [None]                                         # arenas[t]: the parameters that produce output t (t >= 1)
    for _ in range(200):
        a.eager(keep=outs)
        arenas.append(a.params().clone())
    torch.cuda.synchronize()
    xs = torch.stack(outs).reshape(200, -1).cpu().numpy()
    ref, stop, margins = E.emv_reference(xs, ALPHA, WARM, 6)
    best = int(ref[-1, 2])
    assert best >= WARM and min(margins) >= 1e-6                      # (far from fp32 / fp64 rounding: the stop hangs on no tie)
    b = _Fit(dev, **EMV_KW)
    it = b.native()
    issued, losses = it.run_until(200, check_every=7)
    print(f"[run_until emv] reference: best_iter {best}, stop {stop}, smallest decision margin {min(margins):.2e}; issued {issued}")
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
    assert torch.equal(twin.params(), arenas[best])
    b.es.restore_best()
    assert torch.equal(b.params(), twin.params())
    assert torch.equal(b.net(b.z).detach(), twin.net(twin.z).detach())
    fresh = _Fit(dev, **EMV_KW)
    with pytest.raises(RuntimeError, match="dip-amd: EarlyStopMonitor.restore_best: no minimum"):
        fresh.es.restore_best()
