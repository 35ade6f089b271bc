"""GroupedFits(monitor=) on a real MI355X: the rest of the denoising / restoration closure (denoising.ipynb:214-248,
restoration.ipynb:192-211: EMA of the output, three PSNRs, parameter checkpoint, 5 dB fall-back) for B fits through ONE launch
list -- dip_fit_monitor_dev and dip_arena_backtrack inside dip_group_begin / dip_group_end, the monitor's state in the slab rows.

The bar is bit-exactness: instance b of a monitored group is the same fit on its own under utils.fit_monitor.FitMonitor and the
eager closure.  Both arms run the same arithmetic in the same order (fixed pairing order of the partial sums, fp64 finalise), so
every comparison is torch.equal: no tolerance anywhere.  Every test runs in both forms of the DIP_FAM_LOSS family: one dispatch
for all instances, and the library-side loop of B solo dispatches."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from test_group_gpu import _net, _problem

pytestmark = pytest.mark.gpu

import dip_native as N  # noqa: E402

ALL = 0x7fffffff
MASKS = pytest.mark.parametrize("mask", [ALL, 0], ids=["one-dispatch", "host-loop"])


@pytest.fixture
def native_mask():
    lib = N.lib()
    prev = lib.dip_group_native(-1)
    yield lib
    lib.dip_group_native(prev)
    assert lib.dip_group_size() == 1


@pytest.fixture(scope="module", autouse=True)
def _stream_pool_stands_where_it_stood():
    """torch hands out its pooled HIP streams round-robin, and every engine of this module draws three of them (a captured
    group three more and a capture stream).  Which pooled streams a later fit gets decides which of them share a hardware
    queue, and the suite's timing tests are sensitive to that.  So this module leaves the pool where a run without it would:
    one full turn of the pool first (that alone moves nothing), and after the last test as many draws as bring it back."""
    if not torch.cuda.is_available():
        yield
        return
    ring = [torch.cuda.Stream().cuda_stream]
    while True:
        h = torch.cuda.Stream().cuda_stream
        if h == ring[0]:
            break
        ring.append(h)
        assert len(ring) <= 1024 and len(set(ring)) == len(ring), \
            f"torch's stream pool is no ring of distinct streams ({len(ring)} draws): this fixture no longer knows how to restore it"
    for _ in range(len(ring) - 1):                   # (the draw that closed the turn was the first of a second one)
        torch.cuda.Stream()
    yield
    for _ in range(len(ring)):
        if torch.cuda.Stream().cuda_stream == ring[-1]:          # the next draw is ring[0] again
            break
    else:
        raise AssertionError("torch's stream pool changed while this module ran: its position could not be restored")


# ------------------------------------------------------------------------------------------ 1. kernel against kernel
SENT = -12345.0
SHOW, CAP, W, DB = 3, 8, 0.9, 5.0
# (counter, state before the call): first iteration / unchecked (stale flags must be cleared) / far above -> restore /
# far below -> snapshot / at capacity -> the overflow guard
FIRST = (0, [0., 0., 0., 0.])
UNCHECKED = (SHOW, [12.5, 1., 1., 1.])
RESTORE = (SHOW + 1, [1000., 0., 1., 0.])
SNAPSHOT = (SHOW + 1, [-1000., 0., 1., 0.])
FULL = (CAP, [3., 1., 1., 1.])
CALLS = [(FIRST, RESTORE, FULL), (UNCHECKED, SNAPSHOT, RESTORE)]


class _Layout:
    """One row of a hand-built [B][stride] slab: every buffer 256-byte aligned, a sentinel guard band around each."""
    GUARD = 64            # floats

    def __init__(self, n, gt, n_arena, nblk):
        self.off, self.size = {}, {}
        o = self.GUARD
        for k, sz in (("out", n), ("noisy", n), ("gt", n if gt else 0), ("avg", n), ("partial", 4 * nblk),
                      ("records", CAP * 8), ("state", 4), ("counter", 1), ("loss", 1), ("params", n_arena),
                      ("snapshot", n_arena)):
            if sz == 0:
                continue
            self.off[k], self.size[k] = o, sz
            o = (o + sz + self.GUARD + 63) // 64 * 64
        self.stride = o                                   # floats; a multiple of 64 = 256 bytes

    def get(self, row, k):
        return row[self.off[k]:self.off[k] + self.size[k]]

    def guards(self, row):
        keep = torch.ones(self.stride, dtype=torch.bool, device=row.device)
        for k in self.off:
            keep[self.off[k]:self.off[k] + self.size[k]] = False
        return row[keep]

    def launch(self, L, row, gt, stream):
        p = lambda k: row.data_ptr() + 4 * self.off[k]                                  # noqa: E731
        d = N.DipFitMonitorDesc(p("out"), p("noisy"), p("gt") if gt else None, p("avg"), self.size["out"], W, DB, p("loss"),
                                p("partial"), p("records"), CAP, SHOW, 1, 0, p("counter"), p("state"))
        N.check(L.dip_fit_monitor_dev(ctypes.byref(d), stream), "fit_monitor_dev")
        N.check(L.dip_arena_backtrack(p("params"), p("snapshot"), self.size["params"], p("state"), stream), "arena_backtrack")


@MASKS
@pytest.mark.parametrize("n_arena", [5, 4099], ids=["arena5", "arena4099"])          # the scalar tail / the float4 path
@pytest.mark.parametrize("gt", [True, False], ids=["gt", "no-gt"])
@pytest.mark.parametrize("n", [1, 255, 2880, 1024 * 1024 + 3])                       # the last wraps the grid-stride loop
def test_grouped_monitor_kernels_equal_solo_calls(dev, native_mask, n, gt, n_arena, mask):
    L = native_mask
    B = 3
    nblk = L.dip_fit_monitor_nblk(n)
    assert (nblk == 1024 and n > 1024 * 1024) or nblk == (n + 1023) // 1024
    lay = _Layout(n, gt, n_arena, nblk)
    stream = torch.cuda.current_stream(dev).cuda_stream
    gen = torch.Generator().manual_seed(n % 1000 + 31 + n_arena)
    for call in CALLS:
        rows = torch.full((B, lay.stride), SENT)
        for b, (counter, state) in enumerate(call):
            for k in ("out", "noisy", "avg", "params", "snapshot") + (("gt",) if gt else ()):
                lay.get(rows[b], k).copy_(torch.rand(lay.size[k], generator=gen))
            lay.get(rows[b], "partial").fill_(-7.)
            lay.get(rows[b], "records").zero_()
            lay.get(rows[b], "state").copy_(torch.tensor(state))
            lay.get(rows[b], "counter").view(torch.int32).fill_(counter)
            lay.get(rows[b], "loss").fill_(0.125 * (b + 1))
            # precondition, fp64: the PSNRs are finite and far from the +-1000 thresholds: no branch hangs on a rounding
            o, a0 = lay.get(rows[b], "out").double().numpy(), lay.get(rows[b], "avg").double().numpy()
            a = o if counter == 0 else a0 * np.float64(np.float32(W)) + o * (1.0 - np.float64(np.float32(W)))
            refs = [lay.get(rows[b], "noisy").double().numpy()] + ([lay.get(rows[b], "gt").double().numpy()] * 2 if gt else [])
            for x, r in zip((o, o, a), refs):
                psnr = -10.0 * np.log10(np.mean((x - r) ** 2))
                assert np.isfinite(psnr), (n, b)
                assert abs(psnr - (1000. - DB)) > 100. and abs(psnr - (-1000. - DB)) > 100., (n, b, psnr)
        rows = rows.to(dev)
        before = rows.clone()
        # B solo calls on copies of the rows
        solo = [rows[b].clone() for b in range(B)]
        for r in solo:
            lay.launch(L, r, gt, stream)
        # ONE grouped call
        L.dip_group_native(mask)
        N.check(L.dip_group_begin(B, 4 * lay.stride, rows.data_ptr(), 4 * lay.stride), "group_begin")
        try:
            lay.launch(L, rows[0], gt, stream)
        finally:
            assert L.dip_group_end() == 0
        torch.cuda.synchronize()
        for b, (counter, state) in enumerate(call):
            what = (n, gt, n_arena, mask, b, counter, state)
            for k in lay.off:                                    # buffer by buffer, for a readable failure ...
                assert torch.equal(lay.get(rows[b], k).view(torch.int32), lay.get(solo[b], k).view(torch.int32)), (what, k)
            assert torch.equal(rows[b].view(torch.int32), solo[b].view(torch.int32)), what     # ... and the whole row, bit for bit
            assert torch.all(lay.guards(rows[b]) == SENT), what
            get = lambda k, src=rows: lay.get(src[b], k)           # noqa: E731
            st, rec = get("state").tolist(), get("records").view(CAP, 8)
            if (counter, state) == FULL:
                for k in ("records", "avg", "counter", "params", "snapshot", "partial"):
                    assert torch.equal(get(k), get(k, before)), (what, k)
                assert st == [3., 0., 1., 0.], what
                continue
            assert get("counter").view(torch.int32).item() == counter + 1, what
            assert rec[counter, 0].item() == 0.125 * (b + 1) and rec[counter, 4].item() != 0., what
            assert torch.count_nonzero(torch.cat([rec[:counter], rec[counter + 1:]])).item() == 0, what
            if (counter, state) == RESTORE:
                assert st[1:] == [1., 1., 0.] and st[0] == 1000. and rec[counter, 7].item() == 1., what
                assert torch.equal(get("params"), get("snapshot", before)), what
                assert torch.equal(get("snapshot"), get("snapshot", before)), what
            elif (counter, state) == SNAPSHOT:
                assert st[1:] == [0., 1., 1.] and st[0] == rec[counter, 4].item() and rec[counter, 7].item() == 0., what
                assert torch.equal(get("snapshot"), get("params", before)), what
                assert torch.equal(get("params"), get("params", before)), what
            else:                                                   # first / unchecked: no decision, nothing moves
                assert st[1] == 0. and st[3] == 0. and st[0] == state[0], what
                assert torch.equal(get("params"), get("params", before)), what
                assert torch.equal(get("snapshot"), get("snapshot", before)), what
            if counter == 0:
                assert torch.equal(get("avg"), get("out")), what


# ------------------------------------------------------------------------------------------ 2. whole fits
class _Solo:
    """The fit on its own: RegNoise + MSEHead + FitMonitor + FusedAdam, the eager closure."""

    def __init__(self, net, z, img, mask, gt, std, seed, **mon_kw):
        from utils.common_utils import get_params
        from utils.fit_monitor import FitMonitor
        from utils.loss_head import MSEHead
        from utils.reg_noise import RegNoise
        from dip_optim import FusedAdam
        self.net, self.reg, self.head = net, RegNoise(z, std, seed=seed), MSEHead(net, img, mask)
        self.mon = FitMonitor(net, img, gt, **mon_kw)
        self.opt = FusedAdam(get_params("net", net, z), lr=0.01)
        self.loss = None

    def step(self, n=1):
        for _ in range(n):
            self.opt.zero_grad()
            loss, out = self.head(self.reg())
            loss.backward()
            self.mon.update(out, loss)
            self.opt.step()
            self.loss = loss.detach().clone()


def _poke(B, odd_above):
    return torch.tensor([[1000. if (b % 2 == 1) == odd_above else -1000., 0., 1., 0.] for b in range(B)])


def _setup(dev, lib, mask, kind, hw, B, std, mask_c, gt, **mon_kw):
    from dip_group import GroupedFits
    from utils.fit_monitor import GroupedFitMonitor
    zs, ts, ms = _problem(kind, hw, B, mask_c, dev)
    gen = torch.Generator().manual_seed(5)
    gts = [torch.rand(1, 3, *hw, generator=gen).to(dev) for _ in range(B)] if gt else None
    nets = [_net(kind, 10 + b).to(dev) for b in range(B)]
    refs = [copy.deepcopy(n) for n in nets]
    solo = [_Solo(refs[b], zs[b], ts[b], None if ms is None else ms[b], None if gts is None else gts[b], std, 40 + b, **mon_kw)
            for b in range(B)]
    lib.dip_group_native(mask)
    gm = GroupedFitMonitor(gts, **mon_kw)
    g = GroupedFits(nets, zs, ts, masks=ms, reg_noise_std=std, seeds=[40 + b for b in range(B)], lr=0.01, monitor=gm)
    assert g.pointers_outside_row0() == [] and g.out_avg is gm.out_avg
    return g, gm, nets, refs, solo


def _assert_same(g, gm, nets, refs, solo, what=""):
    torch.cuda.synchronize()
    B = g.B
    assert g.step_counts() == [gm.i] * B and g.iterations == gm.i, what
    assert gm.counter.tolist() == [gm.i] * B, what
    hist = gm.history()
    assert hist.shape == (B, gm.i, 8), what
    for b in range(B):
        s = solo[b]
        assert s.mon.i == gm.i and s.opt.device_step_count() == gm.i, (what, b)
        assert torch.equal(gm.records[b], s.mon.records), (what, b, hist[b].tolist(), s.mon.history().tolist())
        assert np.array_equal(hist[b], s.mon.history()), (what, b)
        assert torch.equal(gm.out_avg[b:b + 1], s.mon.out_avg), (what, b)
        assert torch.equal(gm.state[b], s.mon.state), (what, b, gm.state[b].tolist(), s.mon.state.tolist())
        assert (gm.snapshot is None) == (s.mon.snapshot is None), (what, b)
        if gm.snapshot is not None:
            assert torch.equal(gm.snapshot[b], s.mon.snapshot), (what, b)
        assert g.losses[b].item() == s.loss.item() == hist[b, -1, 0], (what, b)
        for (k, pa), pb in zip(nets[b].named_parameters(), refs[b].parameters()):
            assert torch.equal(pa, pb), (what, b, k)
        for (k, ba), bb in zip(nets[b].named_buffers(), refs[b].buffers()):
            assert torch.equal(ba, bb), (what, b, k)
        assert gm.last()[b] == s.mon.last(), (what, b)


FITS = [
    # kind, (H, W), B, reg-noise std, mask channels, gt
    ("skip3", (32, 64), 3, 1. / 30., 0, True),
    ("library", (40, 56), 4, 0.0, 1, False),
]
FIT_IDS = ["skip3-32x64-gt", "library-40x56-masked"]


@MASKS
@pytest.mark.parametrize("case", FITS, ids=FIT_IDS)
def test_monitored_group_bitwise_equals_solo_fits(dev, native_mask, case, mask):
    from dip_optim import GraphedIteration
    kind, hw, B, std, mask_c, gt = case
    g, gm, nets, refs, solo = _setup(dev, native_mask, mask, kind, hw, B, std, mask_c, gt, exp_weight=0.9, show_every=2,
                                     backtrack_db=5.0, backtracking=True, capacity=16)
    assert [name for _, _, name in g._mon] == ["fit_monitor_dev", "arena_backtrack"]

    def both(n, run):
        run(n)
        for s in solo:
            s.step(n)

    def poke(odd_above):
        torch.cuda.synchronize()
        st = _poke(B, odd_above).to(dev)
        gm.state.copy_(st)
        for b, s in enumerate(solo):
            s.mon.state.copy_(st[b])

    both(2, g.step)                                  # iteration 1 is the first checked one: every instance snapshots
    _assert_same(g, gm, nets, refs, solo, "after 2")
    assert gm.state[:, 3].tolist() == [1.] * B and gm.state[:, 1].tolist() == [0.] * B
    poke(odd_above=True)                             # odd instances: last PSNR far above -> fall back; even: far below -> snapshot
    both(1, g.step)
    assert GraphedIteration.group(g, warmup=1) is g and g.graph is not None          # one more eager iteration, ONE hipGraph
    for s in solo:
        s.step(1)
    _assert_same(g, gm, nets, refs, solo, "after 4 (eager)")
    both(2, g.run)
    _assert_same(g, gm, nets, refs, solo, "after 6 (2 replayed)")
    poke(odd_above=False)                            # the pattern flipped, between two replays
    both(2, g.run)
    _assert_same(g, gm, nets, refs, solo, "after 8 (4 replayed)")
    # precondition, on the solo twins' records alone: the instances took DIFFERENT decisions in one dispatch
    fell = [s.mon.history()[:, 7].tolist() for s in solo]
    assert [f[3] for f in fell] == [float(b % 2) for b in range(B)], fell
    assert [f[7] for f in fell] == [float(1 - b % 2) for b in range(B)], fell
    assert all(f[0] == f[1] == f[2] == f[4] == f[6] == 0. for f in fell), fell
    # the instances really are different fits
    assert len({round(g.losses[b].item(), 9) for b in range(B)}) == B
    assert native_mask.dip_group_size() == 1


# ------------------------------------------------------------------------------------------ 3. no back-tracking
@MASKS
def test_monitor_without_backtracking(dev, native_mask, mask):
    kind, hw, B, std, mask_c, gt = FITS[0]
    g, gm, nets, refs, solo = _setup(dev, native_mask, mask, kind, hw, B, std, mask_c, gt, exp_weight=0.9, show_every=2,
                                     backtracking=False, capacity=16)
    assert [name for _, _, name in g._mon] == ["fit_monitor_dev"]          # no arena_backtrack launch
    assert gm.snapshot is None and g._row0_extra["mon_snapshot"] is None
    g.step(2)
    gm.state.copy_(_poke(B, True).to(dev))            # would make the odd instances fall back, if anything were checked
    for b, s in enumerate(solo):
        s.step(2)
        s.mon.state.copy_(gm.state[b])
    g.capture(warmup=1)
    g.run(3)
    for s in solo:
        s.step(4)
    _assert_same(g, gm, nets, refs, solo)
    assert gm.i == 6 and torch.count_nonzero(gm.records[:, :, 7]).item() == 0
    assert torch.count_nonzero(gm.records[:, :6, 4]).item() == 6 * B


# ------------------------------------------------------------------------------------------ 4. capacity
@MASKS
def test_capacity_is_refused_before_anything_is_issued(dev, native_mask, mask):
    kind, hw, B, std, mask_c, gt = FITS[0]
    g, gm, nets, refs, solo = _setup(dev, native_mask, mask, kind, hw, B, std, mask_c, gt, exp_weight=0.9, show_every=2,
                                     capacity=5)
    g.step(2)
    with pytest.raises(RuntimeError, match="capacity"):
        g.step(4)                                     # eager, nothing of the 4 is issued
    assert gm.i == 2
    g.capture(warmup=1)
    g.run(2)
    for s in solo:
        s.step(5)
    _assert_same(g, gm, nets, refs, solo, "full")
    assert gm.i == 5 and gm.history().shape == (B, 5, 8)
    keep = (gm.records.clone(), gm.state.clone(), gm.out_avg.clone(), [p.detach().clone() for n in nets for p in n.parameters()])
    with pytest.raises(RuntimeError, match="capacity"):
        g.run(1)                                      # replay form
    with pytest.raises(RuntimeError, match="capacity"):
        g.step(1)                                     # eager form
    _assert_same(g, gm, nets, refs, solo, "after the refused calls")
    assert torch.equal(keep[0], gm.records) and torch.equal(keep[1], gm.state) and torch.equal(keep[2], gm.out_avg)
    for a, p in zip(keep[3], [p for n in nets for p in n.parameters()]):
        assert torch.equal(a, p)
    assert gm.counter.tolist() == [5] * B and g.iterations == 5
