"""GroupedFits(early_stop=) on a real MI355X: the ground-truth-free stopping criterion for B fits through ONE launch list --
dip_early_stop_dev / dip_early_stop_emv_dev and dip_early_stop_keep inside dip_group_begin / dip_group_end, the early-stop state
in the slab rows, every instance taking its own decision.

The bar is bit-exactness: instance b of a group with early stopping is the same fit on its own under
NativeIteration(early_stop=EarlyStopMonitor(net=...)); both arms run the same kernels on the same data in the same order, so
every comparison is torch.equal.  The decisions a test expects come from the numpy references (tests/early_stop_ref.py,
tests/early_stop_emv_ref.py).

1. the grouped kernels on a hand-built [B][stride] buffer against three solo monitors, both modes, both forms of the family;
2. whole fits: plain denoising, denoising with monitor=GroupedFitMonitor, a super-resolution group; eager, captured, replayed;
3. run_until, per-instance views, restore_best(), the capacity."""
import copy
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_group_monitor_gpu import MASKS, _stream_pool_stands_where_it_stood, native_mask  # noqa: E402,F401  (autouse: the
#                                   engines of this module draw pooled streams; the pool is left where it stood)
from test_group_gpu import _net, _problem  # noqa: E402

import dip_native as N  # noqa: E402
import early_stop_emv_ref as E  # noqa: E402
import early_stop_ref as R  # noqa: E402

B, T = 3, 60
WMV = dict(mode="wmv", window=5, patience=9)
EMV = dict(mode="emv", alpha=0.25, warmup=8, patience=9)
# best_iter, stopping iteration of S_b (early_stop_emv_ref.group_sequence), asserted on the references in the host suite
DECISIONS = {"wmv": [(19, 28), (16, 25), (13, 22)], "emv": [(20, 29), (17, 26), (14, 23)]}
SENT = -12345.0
GUARD = 64                   # floats of sentinel between the buffers of a row (keeps every buffer 256-byte aligned)
N_ARENA = 4099               # the float4 path of dip_early_stop_keep and its scalar tail


# ------------------------------------------------------------------------------------------ 1. kernel against kernel
class _Layout:
    """One row of a hand-built [B][stride] slab of floats: every buffer 256-byte aligned, a sentinel guard band around each
    (fp64 buffers take two floats per element)."""

    def __init__(self, n, window, nblk, capacity):
        self.off, self.size = {}, {}
        o = GUARD
        for k, sz in (("out", n), ("ring", window * n), ("mean", 2 * n), ("partial", 2 * nblk), ("records", capacity * 5),
                      ("state", 16), ("counter", 1), ("best_out", n), ("params", N_ARENA), ("keep", N_ARENA)):
            if sz == 0:
                continue
            self.off[k], self.size[k] = o, sz
            o = (o + sz + GUARD + 63) // 64 * 64
        self.stride = o                                   # floats; a multiple of 64 = 256 bytes

    def get(self, row, k):
        return row[..., self.off[k]:self.off[k] + self.size[k]]

    def guards(self, rows):
        keep = torch.ones(self.stride, dtype=torch.bool, device=rows.device)
        for k in self.off:
            keep[self.off[k]:self.off[k] + self.size[k]] = False
        return rows[:, keep]


@MASKS
@pytest.mark.parametrize("shape", [(3, 37, 29), (1, 8, 8)], ids=["3x37x29", "1x8x8"])
@pytest.mark.parametrize("mode", ["wmv", "emv"])
def test_grouped_kernels_equal_solo_calls(dev, native_mask, mode, shape, mask):
    from utils.fit_monitor import EarlyStopMonitor, early_stop_state
    L = native_mask
    kw = dict(WMV if mode == "wmv" else EMV)
    n = int(np.prod(shape))
    window = kw["window"] if mode == "wmv" else 0
    lay = _Layout(n, window, L.dip_fit_monitor_nblk(n), T)
    xs = torch.tensor(np.stack([E.group_sequence(shape, b) for b in range(B)])).to(dev)              # [B, T, n]
    gen = torch.Generator().manual_seed(n + 7)
    ps = torch.rand(B, T, N_ARENA, generator=gen).to(dev)                                            # the "parameters" of iteration t
    stream = torch.cuda.current_stream(dev).cuda_stream
    # three solo monitors, each with its own keep buffer behind it
    solo = [EarlyStopMonitor(torch.empty(1, *shape, device=dev), capacity=T, **kw) for _ in range(B)]
    solo_keep = torch.full((B, N_ARENA), SENT, device=dev)
    # ONE slab: sentinels everywhere, then what the kernels expect to find
    rows = torch.full((B, lay.stride), SENT, device=dev)
    lay.get(rows, "records").zero_()
    lay.get(rows, "best_out").zero_()
    lay.get(rows, "state").view(torch.int32).copy_(early_stop_state(dev).expand(B, 16))
    lay.get(rows, "counter").view(torch.int32).zero_()
    p = lambda k: rows.data_ptr() + 4 * lay.off[k]                                                   # noqa: E731
    if mode == "emv":
        desc = N.DipEarlyStopEmvDesc(p("out"), p("mean"), p("partial"), p("records"), p("state"), p("counter"), p("best_out"), n,
                                     kw["alpha"], kw["warmup"], kw["patience"], T, 0)
        entry, name = L.dip_early_stop_emv_dev, "early_stop_emv_dev"
    else:
        desc = N.DipEarlyStopDesc(p("out"), p("ring"), p("mean"), p("partial"), p("records"), p("state"), p("counter"),
                                  p("best_out"), n, window, kw["patience"], T, None)
        entry, name = L.dip_early_stop_dev, "early_stop_dev"
    L.dip_group_native(mask)
    stops = [s for _, s in DECISIONS[mode]]
    frozen_keys = ("mean", "state", "best_out", "keep") + (("ring",) if mode == "wmv" else ())
    frozen = {}
    for t in range(T):
        for b in range(B):
            solo[b].update(xs[b, t].view(1, *shape))
            N.check(L.dip_early_stop_keep(ps[b, t].data_ptr(), solo_keep[b].data_ptr(), N_ARENA, solo[b].state.data_ptr(), stream),
                    "early_stop_keep")
        lay.get(rows, "out").copy_(xs[:, t])
        lay.get(rows, "params").copy_(ps[:, t])
        N.check(L.dip_group_begin(B, 4 * lay.stride, rows.data_ptr(), 4 * lay.stride), "group_begin")
        try:                                                          # ONE grouped call per iteration
            N.check(entry(ctypes.byref(desc), stream), name)
            N.check(L.dip_early_stop_keep(p("params"), p("keep"), N_ARENA, p("state"), stream), "early_stop_keep")
        finally:
            assert L.dip_group_end() == 0
        for b in range(B):
            if t == stops[b]:                                         # what an instance holds at its stop ...
                torch.cuda.synchronize()
                frozen[b] = {k: lay.get(rows[b], k).clone() for k in frozen_keys}
    torch.cuda.synchronize()
    assert L.dip_group_size() == 1
    assert torch.all(lay.guards(rows) == SENT), (mode, shape, mask)
    i32 = lambda t: t.contiguous().view(torch.int32)                  # noqa: E731  (bit for bit; a NaN would compare unequal)
    for b in range(B):
        what = (mode, shape, mask, b)
        s = solo[b]
        get = lambda k: lay.get(rows[b], k)                           # noqa: E731
        assert torch.equal(i32(get("records")), i32(s.records.view(-1))), (what, s.history().tolist())
        assert torch.equal(get("state").view(torch.int32), s.state), what
        assert get("counter").view(torch.int32).item() == s.counter.item() == T, what
        assert torch.equal(get("mean").view(torch.float64), s.mean), what
        if mode == "wmv":
            assert torch.equal(i32(get("ring")), i32(s.ring.view(-1))), what
        assert torch.equal(i32(get("best_out")), i32(s.best_out.view(-1))), what
        assert torch.equal(i32(get("keep")), i32(solo_keep[b])), what
        # the decisions: three different ones, the references'
        best, stop = DECISIONS[mode][b]
        assert (s.best_iter, s.stopped) == (best, 1), what
        rec = get("records").view(T, 5)
        assert rec[stop, 4].item() == 1.0 and rec[stop - 1, 4].item() == 0.0, what
        assert torch.equal(get("best_out"), xs[b, best]) and torch.equal(get("keep"), ps[b, best]), what
        # ... it still holds at the end, while the others went on
        for k in frozen_keys:
            assert torch.equal(i32(frozen[b][k]), i32(get(k))), (what, k)
        assert torch.equal(rec[stop:], rec[stop:stop + 1].expand(T - stop, 5)), what


# ------------------------------------------------------------------------------------------ 2. whole fits
HW = (32, 48)
FIT_WMV = dict(mode="wmv", window=4, patience=6)
FIT_EMV = dict(mode="emv", alpha=0.25, warmup=8, patience=6)
STD = 1. / 30.


class _Solo:
    """The fit on its own: RegNoise + MSEHead (or SRHead) [+ FitMonitor] + FusedAdam + NativeIteration(early_stop=
    EarlyStopMonitor(net=...)); early_stop=False: the same fit with early_stop=None."""

    def __init__(self, net, z, img, down, gt, seed, capacity, monitor, es_kw, early_stop=True):
        from dip_optim import FusedAdam, NativeIteration
        from utils.common_utils import get_params
        from utils.fit_monitor import EarlyStopMonitor, FitMonitor
        from utils.loss_head import MSEHead, SRHead
        from utils.reg_noise import RegNoise
        self.net, self.reg = net, RegNoise(z, STD, seed=seed)
        self.head = MSEHead(net, img) if down is None else SRHead(net, img, down)
        self.opt = FusedAdam(get_params("net", net, z), lr=0.01)
        self.mon = FitMonitor(net, img, gt, show_every=5, capacity=capacity) if monitor else None
        self.es = None
        if early_stop:
            like = torch.empty(1, 3, *HW, device=z.device)
            kw = {k: v for k, v in es_kw.items() if k != "mode"}
            self.es = EarlyStopMonitor(like, net=net, capacity=capacity, mode=es_kw["mode"], **kw)
        self.it = NativeIteration(net, self.head, self.opt, z, reg_noise=self.reg, monitor=self.mon, early_stop=self.es)
        self.loss = None

    def run(self, n):
        self.loss = self.it.run(n)[-1]

    def arena(self):
        return self.net.__dict__["_dip_engine"].params


def _build(dev, case, es_kw, capacity=64, early_stop=True):
    """(group, its early-stop monitor, its nets, the solo twins) of a case: 'plain', 'monitor' or 'sr'."""
    from dip_group import GroupedFits
    from models.downsampler import Downsampler
    from utils.fit_monitor import GroupedEarlyStopMonitor, GroupedFitMonitor
    zs, ts, _ = _problem("skip3", HW, B, 0, dev)
    gen = torch.Generator().manual_seed(5)
    gts = [torch.rand(1, 3, *HW, generator=gen).to(dev) for _ in range(B)] if case == "monitor" else None
    downs = None
    if case == "sr":
        downs = [Downsampler(n_planes=3, factor=2, kernel_type="lanczos2", phase=0.5, preserve_size=True).to(dev)
                 for _ in range(B)]
        ts = [t[:, :, :HW[0] // 2, :HW[1] // 2].contiguous() for t in ts]              # the LR images
    nets = [_net("skip3", 10 + b).to(dev) for b in range(B)]
    refs = [copy.deepcopy(x) for x in nets]
    solo = [_Solo(refs[b], zs[b], ts[b], None if downs is None else downs[b], None if gts is None else gts[b], 40 + b, capacity,
                  case == "monitor", es_kw, early_stop) for b in range(B)]
    mon = GroupedFitMonitor(gts, show_every=5, capacity=capacity) if case == "monitor" else None
    es = GroupedEarlyStopMonitor(capacity=capacity, **es_kw) if early_stop else None
    g = GroupedFits(nets, zs, ts, downsamplers=downs, reg_noise_std=STD, seeds=[40 + b for b in range(B)], lr=0.01, monitor=mon,
                    early_stop=es)
    assert g.pointers_outside_row0() == []
    return g, es, nets, solo


def _assert_same_params(nets, others, what):
    for b, (na, nb) in enumerate(zip(nets, others)):
        for (k, pa), pb in zip(na.named_parameters(), nb.parameters()):
            assert torch.equal(pa, pb), (what, b, k)
        for (k, ba), bb in zip(na.named_buffers(), nb.buffers()):
            assert torch.equal(ba, bb), (what, b, k)


def _assert_same(g, es, nets, solo, what=""):
    torch.cuda.synchronize()
    assert g.iterations == es.i and g.step_counts() == [es.i] * B and es.counter.tolist() == [es.i] * B, what
    hist = es.history()
    assert hist.shape == (B, es.i, 5), what
    for b, s in enumerate(solo):
        w = (what, b)
        assert s.es.i == es.i, w
        assert torch.equal(es.records[b].view(torch.int32), s.es.records.view(torch.int32)), (w, hist[b].tolist(), s.es.history().tolist())
        assert torch.equal(es.state[b], s.es.state) and es.counter[b].item() == s.es.counter.item(), w
        assert torch.equal(es.mean[b], s.es.mean), w
        assert (es.ring is None) == (s.es.ring is None), w
        if es.ring is not None:
            fill = int(s.es.state[7].item())                          # (slots the window has not reached yet hold no output)
            assert torch.equal(es.ring[b, :fill], s.es.ring[:fill]), w
        assert torch.equal(es.best_out[b:b + 1], s.es.best_out), w
        assert torch.equal(es.best_params[b], s.es.best_params), w
        assert g.losses[b].item() == s.loss.item(), w
        assert torch.equal(g.out[b:b + 1], s.it.out), w
        assert es.last()[b] == s.es.last(), w
    _assert_same_params(nets, [s.net for s in solo], what)
    assert es.best_iter == [s.es.best_iter for s in solo] and es.stopped == [s.es.stopped for s in solo], what


@pytest.mark.parametrize("case", ["plain", "monitor", "sr"], ids=["denoising", "denoising-monitor", "super-resolution"])
@pytest.mark.parametrize("es_kw", [FIT_WMV, FIT_EMV], ids=["wmv", "emv"])
def test_group_with_early_stop_bitwise_equals_solo_fits(dev, es_kw, case):
    g, es, nets, solo = _build(dev, case, es_kw)
    dev_name = "early_stop_emv_dev" if es_kw["mode"] == "emv" else "early_stop_dev"
    assert [name for _, _, name in g._es] == [dev_name, "early_stop_keep"]
    assert es.group is g

    def both(n, run):
        run(n)
        for s in solo:
            s.run(n)

    both(2, g.step)
    g.capture(warmup=1)                               # the third eager iteration, then ONE hipGraph with the early-stop launches
    for s in solo:
        s.run(1)
    _assert_same(g, es, nets, solo, "after 3 eager")
    both(17, g.run)
    _assert_same(g, es, nets, solo, "after 20")
    both(20, g.run)
    _assert_same(g, es, nets, solo, "after 40")
    h = es.history()
    first = es_kw["window"] - 1 if es_kw["mode"] == "wmv" else es_kw["warmup"]
    assert np.all(np.isinf(h[:, :first, 0])) and np.all(np.isfinite(h[:, first:, 0])) and np.all(h[:, -1, 2] >= first)
    assert torch.count_nonzero(es.best_params).item() > 0
    assert es.memory_bytes == sum(s.es.memory_bytes for s in solo)    # what B solo monitors hold, and no more
    if case == "monitor":                            # the monitor's record is the solo FitMonitor's, untouched by early_stop=
        for b, s in enumerate(solo):
            assert torch.equal(g.monitor.records[b], s.mon.records) and torch.equal(g.monitor.out_avg[b:b + 1], s.mon.out_avg)
    # the same group without early_stop=: the same losses and parameters
    g0, _, nets0, _ = _build(dev, case, es_kw, early_stop=False)
    assert g0.early_stop is None and g0.stride < g.stride
    g0.step(2)
    g0.capture(warmup=1)
    g0.run(37)
    torch.cuda.synchronize()
    assert torch.equal(g0.losses, g.losses) and torch.equal(g0.out, g.out)
    _assert_same_params(nets, nets0, "early_stop= vs None")
    # the instances really are different fits
    assert len({round(g.losses[b].item(), 9) for b in range(B)}) == B


# ------------------------------------------------------------------------------------------ 3. run_until
_HOST = {}


def _host_decisions(dev):
    """Per instance: the fp64 reference rows over 200 iterations of the solo fit's outputs, and the parameter arena in front
    of every iteration.  Computed once and shared (read-only)."""
    if not _HOST:
        _, _, _, solo = _build(dev, "plain", FIT_EMV, early_stop=False)
        rows, arenas = [], []
        for s in solo:
            outs, ar = [], [None]                     # ar[t]: the parameters that produce output t (t >= 1)
            for _ in range(200):
                s.it.step()
                outs.append(s.it.out.clone())
                ar.append(s.arena().clone())
            torch.cuda.synchronize()
            xs = torch.stack(outs).reshape(200, -1).cpu().numpy()
            r, stop, margins = E.emv_reference(xs, FIT_EMV["alpha"], FIT_EMV["warmup"], FIT_EMV["patience"])
            print(f"[group run_until] instance {len(rows)}: best_iter {int(r[-1, 2])}, stop {stop}, smallest decision margin "
                  f"{min(margins):.2e}")
            assert min(margins) >= 1e-6             # (far from fp32 / fp64 rounding: no expected decision hangs on a tie)
            rows.append((r, stop))
            arenas.append(ar)
        _HOST.update(rows=rows, arenas=arenas)
    return _HOST["rows"], _HOST["arenas"]


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
def test_run_until_per_instance_decisions_and_restore_best(dev, captured):
    rows, arenas = _host_decisions(dev)
    stops = [stop for _, stop in rows]
    g, es, nets, _ = _build(dev, "plain", FIT_EMV, capacity=256)
    done = 0
    if captured:
        g.capture()                                   # three eager iterations, recorded like any other
        done = 3
        assert es.i == 3
    issued = done + g.run_until(200 - done, check_every=7)
    if all(s is not None for s in stops):
        last = max(stops)
        assert issued == min(200, done + 7 * math.ceil((last + 1 - done) / 7)), (issued, stops)
    else:
        assert issued == 200, (issued, stops)
    assert g.iterations == es.i == issued and es.counter.tolist() == [issued] * B
    # per instance: what the reference says at the last issued iteration
    assert es.stopped == [int(r[issued - 1, 4]) for r, _ in rows]
    best = [int(r[issued - 1, 2]) for r, _ in rows]
    assert es.best_iter == best and min(best) >= FIT_EMV["warmup"]
    h = es.history()
    for b, stop in enumerate(stops):
        if stop is not None and stop < issued:
            assert h[b, stop, 4] == 1.0 and h[b, stop - 1, 4] == 0.0, b
    # restore_best(b=1) touches row 1 only; restore_best() every row: the parameters the solo fit held at best_iter
    params = g._strided(g.eng.params, g.eng.n_arena)
    before = params.clone()
    assert all(not torch.equal(before[b], arenas[b][best[b]]) for b in range(B))
    es.restore_best(b=1)
    assert torch.equal(params[1], arenas[1][best[1]]) and torch.equal(params[0], before[0]) and torch.equal(params[2], before[2])
    es.restore_best()
    for b in range(B):
        assert torch.equal(params[b], arenas[b][best[b]]), b
        assert torch.equal(es.best_params[b], arenas[b][best[b]]), b


def test_capacity_is_refused_before_anything_is_issued(dev):
    g, es, nets, _ = _build(dev, "plain", FIT_EMV, capacity=10)
    g.step(4)
    torch.cuda.synchronize()
    keep = (es.records.clone(), es.state.clone(), g._strided(g.eng.params, g.eng.n_arena).clone())
    for call in (lambda: g.run_until(7, check_every=2), lambda: g.step(7), lambda: g.run(7)):
        with pytest.raises(RuntimeError, match="dip-amd: GroupedEarlyStopMonitor capacity exceeded"):
            call()
    torch.cuda.synchronize()
    assert (es.i, g.iterations, es.counter.tolist()) == (4, 4, [4] * B)
    assert torch.equal(keep[0], es.records) and torch.equal(keep[1], es.state)
    assert torch.equal(keep[2], g._strided(g.eng.params, g.eng.n_arena))
    with pytest.raises(RuntimeError, match="dip-amd: GroupedEarlyStopMonitor.restore_best: no minimum.*\\[0, 1, 2\\]"):
        es.restore_best()                             # (4 iterations, warmup 8: no decision has been taken)
    assert g.run_until(6, check_every=4) == 6 and es.i == 10
    assert es.stopped == [0] * B and es.best_iter == [int(x) for x in es.history()[:, -1, 2]]
