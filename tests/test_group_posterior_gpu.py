"""The grouped posterior on a real MI355X: dip_posterior_pool alone against its numpy-float32 restatement
(tests/posterior_pool_ref.py), bitwise; dip_group.GroupedFits(posterior=GroupedPosteriorMonitor(...)) against the solo
NativeIteration(posterior=PosteriorMonitor(...)) fits and against the same group without the keyword, eager and as ONE hipGraph,
for the three group kinds; all four monitor slots together; pooled() on a group's rows; and the records of the posterior mean's
PSNR (dip_posterior_rec_dev), solo eager, solo native and grouped.  Every comparison of device results is torch.equal."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import posterior_pool_ref as R  # noqa: E402
from test_group_gpu import _problem  # noqa: E402
from test_group_monitor_gpu import _stream_pool_stands_where_it_stood  # noqa: E402,F401  (autouse: the engines of this module
#                                                                                          draw pooled streams too)
from test_native_iter_host import _small  # noqa: E402
from test_posterior_gpu import _eager_pm_step  # noqa: E402
from test_sr_head_gpu import _sr_setup  # noqa: E402

B, HW, SR_HW = 3, (36, 52), (64, 96)
BURN_IN, EVERY, ITERS = 3, 2, 10                   # samples fall at iterations 3, 5, 7 and 9
SAMPLES = [3, 5, 7, 9]
WD, STDS, PSEEDS, SEEDS = 5e-8, [0.01, 0.02, 0.03], [11, 2 ** 64 - 1, 2 ** 32 + 7], [40, 41, 42]
SENTINEL, GUARD = 12345.0, 8


# ------------------------------------------------------------------------------------------ 1. the pool kernel alone
def _rows(rng, C_, n, k):
    """Welford rows of C_ chains of k samples around one image: float32 means apart by about 0.02, m2 = (k - 1) * variance."""
    base = rng.uniform(0.05, 0.95, n)
    mean = (base + rng.normal(0, 0.02, (C_, 1)) + rng.normal(0, 0.01, (C_, n))).astype(np.float32)
    m2 = ((k - 1) * 0.03 ** 2 * rng.chisquare(k - 1, (C_, n)) / (k - 1)).astype(np.float32)
    return mean, m2


def _pool_on_device(dev, mean, m2, k, chains=None, stride=None, off=0, rhat=True):
    """dip_posterior_pool through ctypes on rows laid out at `stride` floats (default: n rounded up to 4, so that aligned rows
    take 16-byte accesses), `off` floats behind a 256-byte boundary -- off = 1: every row and output 4 bytes off 16-byte
    alignment.  Sentinels stand in front of and behind every output.  Returns numpy (mu, V, W, R or None, summary)."""
    import dip_native as N
    L = N.lib()
    rows, n = mean.shape
    up4 = lambda x: (x + 3) // 4 * 4
    stride = up4(n) if stride is None else stride
    buf = torch.full((2, off + rows * stride + 4), SENTINEL, dtype=torch.float32)
    for r in range(rows):
        buf[0, off + r * stride: off + r * stride + n] = torch.from_numpy(mean[r])
        buf[1, off + r * stride: off + r * stride + n] = torch.from_numpy(m2[r])
    row_len = up4(buf.shape[1])                    # (the second plane starts on a 16-byte boundary too)
    dbuf = torch.full((2, row_len), SENTINEL, dtype=torch.float32, device=dev)
    dbuf[:, :buf.shape[1]] = buf.to(dev)
    chains = list(range(rows)) if chains is None else chains
    idx = torch.tensor(chains, dtype=torch.int32, device=dev)
    seg = up4(n) + 2 * GUARD
    outs = torch.full((4, seg + 4), SENTINEL, dtype=torch.float32, device=dev)
    summ = torch.full((5,), SENTINEL, dtype=torch.float64, device=dev)
    partial = torch.empty(3 * L.dip_fit_monitor_nblk(n), dtype=torch.float64, device=dev)
    at = lambda j: outs[j].data_ptr() + 4 * (GUARD + off)
    assert dbuf.data_ptr() % 16 == 0 and dbuf[1].data_ptr() % 16 == 0 and outs.data_ptr() % 16 == 0 and outs[1].data_ptr() % 16 == 0
    with torch.cuda.device(dev):
        N.check(L.dip_posterior_pool(dbuf[0].data_ptr() + 4 * off, dbuf[1].data_ptr() + 4 * off, 4 * stride, idx.data_ptr(),
                                     len(chains), k, n, at(0), at(1), at(2), at(3) if rhat else None, partial.data_ptr(),
                                     summ.data_ptr() + 8, torch.cuda.current_stream(dev).cuda_stream), "posterior_pool")
    torch.cuda.synchronize()
    o, s = outs.cpu().numpy(), summ.cpu().numpy()
    lo, hi = GUARD + off, GUARD + off + n
    for j in range(4):                             # nothing in front of or behind an output was touched (nor rhat without a map)
        assert (o[j, :lo] == SENTINEL).all() and (o[j, hi:] == SENTINEL).all(), j
    assert s[0] == SENTINEL and s[4] == SENTINEL and (rhat or (o[3] == SENTINEL).all())
    assert torch.equal(dbuf[:, :buf.shape[1]].cpu(), buf)                                   # the rows were only read
    return o[0, lo:hi], o[1, lo:hi], o[2, lo:hi], (o[3, lo:hi] if rhat else None), s[1:4]


def _assert_pooled(got, want, n, what=""):
    for name, g, w in zip(("mean", "var", "within", "rhat"), got[:4], want[:4]):
        if g is None:
            continue
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, name)
        ok = ~np.isnan(w)
        assert np.array_equal(g[ok].view(np.int32), w[ok].view(np.int32)), (what, name, int((g[ok] != w[ok]).sum()))
    gs, ws = got[4], want[4]
    assert gs[2] == ws[2], (what, gs, ws)
    if ws[2] == n:
        assert np.isnan(gs[:2]).all(), (what, gs)
    else:
        assert gs[1] == ws[1] and abs(gs[0] - ws[0]) <= (n - 1) * 2.0 ** -52 * abs(ws[0]), (what, gs, ws)


@pytest.mark.parametrize("C_,n,k,off", [(2, 1, 2, 0), (5, 257, 40, 0), (8, 4099, 300, 0), (3, 255, 7, 1), (2, 2 ** 20 + 4099, 2, 0),
                                        (2, 2 ** 20 + 4098, 3, 1)],
                         ids=["C2-n1", "C5-n257-degenerate", "C8-n4099", "C3-n255-misaligned", "C2-grid-stride-16B",
                              "C2-grid-stride-4B"])
def test_pool_kernel_equals_the_numpy_float32_restatement(dev, C_, n, k, off):
    mean, m2 = _rows(np.random.default_rng(n + k), C_, n, k)
    if n == 257:                                   # two planted degenerate elements
        m2[:, 5] = 0                               # no within-chain variance, different means: V > 0, W = 0
        m2[:, 9] = 0
        mean[:, 9] = 0.5                           # ... and equal means: V = W = 0
    want = R.pool(mean, m2, k)
    got = _pool_on_device(dev, mean, m2, k, off=off)
    _assert_pooled(got, want, n)
    if n == 257:
        assert np.isnan(got[3][[5, 9]]).all() and np.isnan(got[3]).sum() == 2 and got[4][2] == 2
        assert got[1][5] > 0 and got[2][5] == 0 and got[1][9] == 0
        # without a map: the same summary, rhat untouched; every element degenerate: NaN, NaN, n
        _assert_pooled(_pool_on_device(dev, mean, m2, k, rhat=False), want, n, "no map")
        zero = np.zeros_like(m2)
        _assert_pooled(_pool_on_device(dev, mean, zero, k), R.pool(mean, zero, k), n, "all degenerate")


def test_pool_kernel_walks_the_chains_in_list_order(dev):
    """Rows embedded in a 4-row buffer at a stride of 3 n + 7 floats, pooled as [2, 0, 1] and as [0, 1, 2]: each is its
    restatement in list order, and the two differ somewhere (a float32 sum of three terms depends on the order)."""
    C_, n, k = 4, 1021, 7
    mean, m2 = _rows(np.random.default_rng(1), C_, n, k)
    res = {}
    for chains in ([2, 0, 1], [0, 1, 2], [3, 1]):
        res[tuple(chains)] = got = _pool_on_device(dev, mean, m2, k, chains=chains, stride=3 * n + 7)
        _assert_pooled(got, R.pool(mean, m2, k, chains), n, chains)
    a, b = res[(2, 0, 1)], res[(0, 1, 2)]
    assert any(not np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a[:4], b[:4]))


# ------------------------------------------------------------------------------------------ 2. B fits through one launch list
class _Solo:
    """The fit on its own: RegNoise + MSEHead (masked or not) or SRHead + the SGLD FusedAdam + NativeIteration(posterior=
    PosteriorMonitor)."""

    def __init__(self, b, net, z, img, mask, down, gt=None, capacity=16, posterior=True):
        from dip_optim import FusedAdam, NativeIteration
        from utils.common_utils import get_params
        from utils.fit_monitor import PosteriorMonitor
        from utils.loss_head import MSEHead, SRHead
        from utils.reg_noise import RegNoise
        self.net, self.z, self.reg = net, z, RegNoise(z, 1. / 30., seed=SEEDS[b])
        self.head = MSEHead(net, img, mask=mask) if down is None else SRHead(net, img, down)
        self.opt = FusedAdam(get_params("net", net, z), lr=0.01, weight_decay=WD, noise_std=STDS[b], noise_seed=PSEEDS[b])
        hw = HW if down is None else SR_HW
        like = torch.empty(1, 3, *hw, device=z.device)
        self.pm = PosteriorMonitor(like, BURN_IN, EVERY, img_gt=gt, capacity=capacity) if posterior else None
        self.it = NativeIteration(net, self.head, self.opt, z, reg_noise=self.reg, posterior=self.pm)
        self.loss, self.out = None, None

    def run(self, n):
        self.loss = self.it.run(n)[-1]


def _fits(dev, case, gt=False):
    """(B nets, what a group or the solo twins need besides) of a case: 'plain', 'masked' or 'sr'."""
    downs = None
    if case == "sr":                               # the super-resolution fit of tests/test_sr_head_gpu.py: 64 x 96, factor 4
        sets = [_sr_setup(dev, SR_HW, 4, 3, seed=3 + b) for b in range(B)]
        nets, downs, zs, ts = ([s[j] for s in sets] for j in range(4))
        ms = None
    else:                                          # the net and size of tests/test_sgld_fit_gpu.py: _small(), 36 x 52, noisy
        zs, ts, ms = _problem("skip3", HW, B, 1 if case == "masked" else 0, dev)
        nets = []
        for b in range(B):
            torch.manual_seed(30 + b)
            nets.append(_small().to(dev))
    refs = [copy.deepcopy(x) for x in nets]        # (the solo twins: copies taken before a group adopts the nets)
    gen = torch.Generator().manual_seed(5)
    gts = [torch.rand(1, 3, *(SR_HW if case == "sr" else HW), generator=gen).to(dev) for _ in range(B)] if gt else None
    return nets, SimpleNamespace(refs=refs, zs=zs, ts=ts, ms=ms, downs=downs, gts=gts)


def _build(dev, case, posterior=True, gt=False, capacity=16, **kw):
    """(group, its posterior monitor, its nets, what the solo twins need) of a case."""
    from dip_group import GroupedFits
    from utils.fit_monitor import GroupedPosteriorMonitor
    nets, p = _fits(dev, case, gt)
    zs, ts, ms, downs, gts = p.zs, p.ts, p.ms, p.downs, p.gts
    pm = GroupedPosteriorMonitor(BURN_IN, EVERY, imgs_gt=gts, capacity=capacity) if posterior else None
    g = GroupedFits(nets, zs, ts, masks=ms, downsamplers=downs, reg_noise_std=1. / 30., seeds=SEEDS, lr=0.01, weight_decay=WD,
                    param_noise_std=STDS, param_noise_seeds=PSEEDS, posterior=pm, **kw)
    assert g.pointers_outside_row0() == []
    return g, pm, nets, p


def _solo(p, b, **kw):
    kw.setdefault("gt", None if p.gts is None else p.gts[b])
    return _Solo(b, p.refs[b], p.zs[b], p.ts[b], None if p.ms is None else p.ms[b], None if p.downs is None else p.downs[b], **kw)


def _solos(p, **kw):
    return [_solo(p, b, **kw) for b in range(B)]


def _run_graphed(g, n=ITERS):
    """2 eager iterations, the third as capture()'s warm-up, the rest as replays of the ONE hipGraph."""
    g.step(2)
    g.capture(warmup=1)
    g.run(n - 3)
    torch.cuda.synchronize()


def _assert_same_fit(g, nets, g0, nets0, what):
    assert torch.equal(g.losses, g0.losses) and torch.equal(g.out, g0.out), what
    for b in range(B):
        for (k, pa), pb in zip(nets[b].named_parameters(), nets0[b].parameters()):
            assert torch.equal(pa, pb), (what, b, k)


def _assert_group_equals_solos(g, pm, nets, solo, what):
    torch.cuda.synchronize()
    assert g.iterations == pm.i == ITERS and pm.count == len(SAMPLES), what
    assert pm.counter.tolist() == [ITERS] * B and pm.samples.tolist() == [len(SAMPLES)] * B, what
    for b, s in enumerate(solo):
        w = (what, b)
        assert s.pm.i == pm.i and s.pm.count == pm.count, w
        assert torch.equal(pm.mean[b:b + 1], s.pm.mean) and torch.equal(pm.m2[b:b + 1], s.pm.m2), w
        assert torch.equal(pm.samples[b:b + 1], s.pm.samples) and torch.equal(pm.counter[b:b + 1], s.pm.counter), w
        assert g.losses[b].item() == s.loss.item() and torch.equal(g.out[b:b + 1], s.it.out), w
        for (k, pa), pb in zip(nets[b].named_parameters(), s.net.parameters()):
            assert torch.equal(pa, pb), (w, k)
    assert torch.equal(pm.variance(), pm.m2 / 3.0) and bool((pm.m2 > 0).any()) and len({float(x) for x in pm.mean[:, 0, 0, 0]}) == B


@pytest.mark.parametrize("case", ["plain", "masked", "sr"], ids=["denoising", "masked", "super-resolution"])
def test_group_with_posterior_bitwise_equals_solo_fits(dev, case):
    g, pm, nets, p = _build(dev, case)
    assert [name for _, _, name in g._post] == ["posterior_dev"] and pm.group is g
    assert list(g._row0_extra)[-4:] == ["post_mean", "post_m2", "post_samples", "post_counter"]
    assert tuple(pm.mean.shape) == (B, 3, *(SR_HW if case == "sr" else HW)) and pm.count == 0
    solo = _solos(p)
    for s in solo:
        s.run(ITERS)
    _run_graphed(g)                                # (the posterior launch is inside the graph: the replays advance the rows)
    _assert_group_equals_solos(g, pm, nets, solo, case)
    # the same group without posterior=: the same losses, outputs and parameters
    g0, _, nets0, _ = _build(dev, case, posterior=False)
    assert g0.posterior is None and g0.stride < g.stride and not hasattr(g0, "_pdesc")
    assert list(g0._row0_extra) == list(g._row0_extra)[:-4]
    _run_graphed(g0)
    _assert_same_fit(g, nets, g0, nets0, case)


# ------------------------------------------------------------------------------------------ 3. capture
def test_captured_group_equals_the_eager_group(dev):
    ge, pe, nets_e, _ = _build(dev, "plain")
    gc, pc, nets_c, _ = _build(dev, "plain")
    ge.step(ITERS)
    assert ge.graph is None
    gc.capture(warmup=3)
    torch.cuda.synchronize()
    assert pc.counter.tolist() == [3] * B and pc.samples.tolist() == [0] * B          # (capturing issues nothing)
    gc.run(ITERS - 3)
    torch.cuda.synchronize()
    assert gc.graph is not None and pc.counter.tolist() == [ITERS] * B and pc.samples.tolist() == [len(SAMPLES)] * B
    for name in ("mean", "m2", "samples", "counter"):
        assert torch.equal(getattr(pe, name), getattr(pc, name)), name
    assert pe.i == pc.i == ITERS and pe.count == pc.count == len(SAMPLES)
    _assert_same_fit(ge, nets_e, gc, nets_c, "capture")


# ------------------------------------------------------------------------------------------ 4. all four slots
def test_all_four_slots_in_the_solo_order(dev):
    from utils.fit_monitor import GroupedEarlyStopMonitor, GroupedFitMonitor, GroupedSSIMMonitor
    gen = torch.Generator().manual_seed(6)
    gts = [torch.rand(1, 3, *HW, generator=gen).to(dev) for _ in range(B)]
    others = lambda: dict(monitor=GroupedFitMonitor(gts, show_every=4, capacity=16),
                          early_stop=GroupedEarlyStopMonitor(mode="emv", alpha=0.25, patience=3, capacity=16),
                          ssim=GroupedSSIMMonitor(gts, with_avg=True, capacity=16))
    g, pm, nets, _ = _build(dev, "plain", **others())
    g0, _, nets0, _ = _build(dev, "plain", posterior=False, **others())
    names = [name for _, _, _, ops in g._monitors() for _, _, name in getattr(g, ops)]
    assert names == ["fit_monitor_dev", "arena_backtrack", "early_stop_emv_dev", "early_stop_keep", "posterior_dev", "ssim_dev"]
    assert [x for x in names if x != "posterior_dev"] == [name for _, _, _, ops in g0._monitors() for _, _, name in getattr(g0, ops)]
    # the post_ rows behind every other monitor's rows, and no other row moved
    keys = list(g._row0_extra)
    assert keys[-4:] == ["post_mean", "post_m2", "post_samples", "post_counter"] and keys[:-4] == list(g0._row0_extra)
    rel = lambda grp: {k: grp._off(t) for k, t in grp._row0_extra.items() if t is not None}
    assert {k: v for k, v in rel(g).items() if not k.startswith("post_")} == rel(g0)
    _run_graphed(g)
    _run_graphed(g0)
    _assert_same_fit(g, nets, g0, nets0, "four slots")
    for slot in ("monitor", "early_stop", "ssim"):
        a, b = getattr(g, slot), getattr(g0, slot)
        assert a.i == b.i == ITERS and torch.equal(a.records, b.records) and torch.equal(a.counter, b.counter), slot
    assert torch.equal(g.monitor.out_avg, g0.monitor.out_avg) and torch.equal(g.early_stop.state, g0.early_stop.state)
    assert pm.samples.tolist() == [len(SAMPLES)] * B and pm.counter.tolist() == [ITERS] * B


# ------------------------------------------------------------------------------------------ 5. pooled()
def test_pooled_on_a_groups_rows(dev):
    g, pm, nets, _ = _build(dev, "plain")
    with pytest.raises(RuntimeError, match="dip-amd: GroupedPosteriorMonitor.pooled needs at least two samples per chain, 0"):
        pm.pooled()
    g.step(6)                                      # iterations 3 and 5: two samples per chain
    assert pm.count == 2
    g.step(ITERS - 6)
    for chains, msg, err in (([1], "at least 2 chains", ValueError), ([0, 2, 0], "a chain is pooled once", ValueError),
                             ([0, B], "of a group of 3", IndexError), ([-1, 0], "of a group of 3", IndexError),
                             ([0.5, 1], "instance indices", ValueError)):
        with pytest.raises(err, match="dip-amd: GroupedPosteriorMonitor.pooled: .*" + msg):
            pm.pooled(chains=chains)
    k = pm.count
    assert k == len(SAMPLES)
    res = {None: pm.pooled(), (2, 0): pm.pooled(chains=[2, 0]), "nomap": pm.pooled(rhat_map=False)}
    torch.cuda.synchronize()
    n = pm.mean[0].numel()
    mean, m2 = pm.mean.reshape(B, n).cpu().numpy(), pm.m2.reshape(B, n).cpu().numpy()
    for key, chains in ((None, None), ((2, 0), [2, 0]), ("nomap", None)):
        p = res[key]
        for t in (p.mean, p.var, p.within) + (() if p.rhat is None else (p.rhat,)):
            assert tuple(t.shape) == (1, 3, *HW) and t.dtype == torch.float32 and t.device == pm.mean.device
        assert p.summary.dtype == torch.float64 and tuple(p.summary.shape) == (3,) and (p.rhat is None) == (key == "nomap")
        got = tuple(None if t is None else t.cpu().numpy().reshape(-1) for t in (p.mean, p.var, p.within, p.rhat)) \
            + (p.summary.cpu().numpy(),)
        _assert_pooled(got, R.pool(mean, m2, k, chains), n, key)
    assert not torch.equal(res[None].mean, res[(2, 0)].mean) and float(res[None].summary[2]) == 0
    # pooled() read the rows and wrote none of them; the fit goes on
    assert np.array_equal(pm.mean.reshape(B, n).cpu().numpy(), mean) and np.array_equal(pm.m2.reshape(B, n).cpu().numpy(), m2)
    g.step(1)


# ------------------------------------------------------------------------------------------ 6., 7. the records
def _ulp_close(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(float(a) - float(b)) <= float(np.spacing(np.abs(b)))


def test_records_of_the_posterior_mean(dev):
    cap = len(SAMPLES)
    g, pm, nets, p = _build(dev, "masked", gt=True, capacity=cap)
    assert [name for _, _, name in g._post] == ["posterior_rec_dev"] and tuple(pm.records.shape) == (B, cap, 3)
    assert list(g._row0_extra)[-7:] == ["post_mean", "post_m2", "post_samples", "post_counter", "post_gt", "post_partial",
                                         "post_records"]
    solo = _solos(p, capacity=cap)
    # solo 0 one iteration at a time: the mean every record was formed from is read back
    means = {}
    for i in range(ITERS):
        solo[0].run(1)
        if i in SAMPLES:
            means[i] = solo[0].pm.mean.cpu().numpy()
    assert solo[0].it._plan["lists"].phases[-2].names == ["posterior_rec_dev"]
    for s in solo[1:]:
        s.run(ITERS)
    _run_graphed(g)
    torch.cuda.synchronize()
    hist = pm.history()
    assert hist.shape == (B, cap, 3) and pm.count == cap and pm.samples.tolist() == [cap] * B
    for b, s in enumerate(solo):
        assert torch.equal(pm.records[b].view(torch.int32), s.pm.records.view(torch.int32)), (b, hist[b].tolist(), s.pm.history().tolist())
        assert torch.equal(pm.mean[b:b + 1], s.pm.mean) and torch.equal(pm.m2[b:b + 1], s.pm.m2), b
        assert s.pm.history().shape == (cap, 3) and pm.last()[b] == s.pm.last() and tuple(s.pm.last()) == s.pm.COLUMNS, b
        assert hist[b, :, 0].tolist() == [float(i) for i in SAMPLES], b                    # the iteration column is exact
    gt0 = p.gts[0].cpu().numpy()
    for r, i in enumerate(SAMPLES):                # mse_mean, psnr_mean: within one fp32 ulp of the fp64 values, rounded
        want = R.record(i, means[i], gt0)
        print(f"sample {r} (iteration {i}): device {hist[0, r].tolist()}, numpy {want.tolist()}")
        assert hist[0, r, 0] == want[0] and _ulp_close(hist[0, r, 1], want[1]) and _ulp_close(hist[0, r, 2], want[2]), (r, i)
        assert 0 < hist[0, r, 1] < 1 and hist[0, r, 2] > 0
    # mean / m2 with img_gt= are those without; the alternating eager / native forms on one monitor are the native one
    plain = _solo(_fits(dev, "masked")[1], 0)
    plain.run(ITERS)
    alt = _solo(_fits(dev, "masked")[1], 0, gt=p.gts[0], capacity=cap)
    alt.run(4)                                     # iterations 0..3 native (sample 3), 4..6 eager (sample 5), 7..9 native (7, 9)
    for _ in range(3):
        _eager_pm_step(alt, alt.pm)
    alt.run(3)
    torch.cuda.synchronize()
    assert not hasattr(plain.pm, "records") and not plain.pm.with_gt and plain.pm.COLUMNS == ()
    with pytest.raises(RuntimeError, match="dip-amd: PosteriorMonitor keeps no record table"):
        plain.pm.history()
    for other, what in ((plain, "without img_gt"), (alt, "alternating")):
        assert torch.equal(other.pm.mean, solo[0].pm.mean) and torch.equal(other.pm.m2, solo[0].pm.m2), what
        assert torch.equal(other.pm.samples, solo[0].pm.samples) and torch.equal(other.pm.counter, solo[0].pm.counter), what
    assert torch.equal(alt.pm.records.view(torch.int32), solo[0].pm.records.view(torch.int32))
    # no rows for non-sample iterations: a monitor with room to spare keeps the rows behind `count` zero
    big = _solo(_fits(dev, "masked")[1], 0, gt=p.gts[0], capacity=ITERS)
    big.run(ITERS)
    torch.cuda.synchronize()
    assert torch.equal(big.pm.records[:cap], solo[0].pm.records) and not big.pm.records[cap:].any() and big.pm.count == cap
    # past `capacity` samples: refused before anything is issued -- native, grouped (replayed and eager), and the eager update
    for call in (lambda: solo[0].it.run(2), lambda: g.run(2), lambda: g.step(2)):
        with pytest.raises(RuntimeError, match="dip-amd: (Grouped)?PosteriorMonitor capacity exceeded"):
            call()
    alt.run(1)                                     # (iteration 10 is no sample; iteration 11 would be the fifth)
    with pytest.raises(RuntimeError, match="dip-amd: PosteriorMonitor capacity exceeded"):
        alt.pm.update(alt.it.out)
    torch.cuda.synchronize()
    assert g.iterations == pm.i == solo[0].pm.i == ITERS and pm.counter.tolist() == [ITERS] * B
    assert int(solo[0].pm.counter.item()) == ITERS and int(alt.pm.counter.item()) == ITERS + 1 and alt.pm.i == ITERS + 1
    assert solo[0].pm.count == alt.pm.count == cap and pm.samples.tolist() == [cap] * B
    # 7. the fit with posterior= and imgs_gt= is the fit without
    g0, _, nets0, _ = _build(dev, "masked", posterior=False)
    _run_graphed(g0)
    _assert_same_fit(g, nets, g0, nets0, "imgs_gt")
