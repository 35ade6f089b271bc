"""Counted-wait kernels under contention (conv_thin4_mfma_kernel at every NJ, conv_small forward): the per-op oracle tests run
each kernel alone on an idle GPU, where every asm load lands long before its `s_waitcnt vmcnt(N)`; a wrong count, or a
register hipcc touches while its load is in flight, only shows when loads are slow.  Each test checks one uncontended launch
against the fp64 oracle with the per-op criterion, then issues K launches on one stream, each into its own buffer, while a
chip-wide device-to-device copy runs on a second stream, and asserts every contended output is bit-identical to the
uncontended one (the kernels are deterministic); conv_small's BatchNorm partial rows are checked against the fp64 output's
channel statistics as well.  The premise is checked, not assumed: events bracket the aggressor and every
tested launch, and at least half of the launches must lie inside the aggressor's window, or the test fails."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dip_native as N  # noqa: E402
from dip_native import round_up  # noqa: E402
import hipops as H  # noqa: E402
import test_kernels_gpu as TK  # noqa: E402
from test_kernels_gpu import REFLECT, ZERO  # noqa: E402

MIN_OVERLAP = 0.5


@functools.lru_cache(maxsize=None)
def _streams(dev):
    """One pair for the module, made back to back: the runtime hands hardware queues out round-robin, and a fresh pair per
    test can land on one queue, where the two streams serialise (the overlap check then fails)."""
    return torch.cuda.Stream(dev), torch.cuda.Stream(dev)


def _contended(dev, launch, outs):
    """launch(i, stream) writes outs[i]; runs launch(0) alone, then launch(1..K-1) beside a device-to-device copy on another
    stream.  Returns the fraction of the contended launches that started and ended inside the copy's window."""
    s_test, s_agg = _streams(dev)
    src = torch.empty(256 << 20, dtype=torch.float32, device=dev).fill_(1.0)     # 1 GiB
    dst = torch.empty_like(src)
    torch.cuda.synchronize()
    launch(0, s_test.cuda_stream)
    torch.cuda.synchronize()
    ev = lambda: torch.cuda.Event(enable_timing=True)                              # noqa: E731
    t0, a0, a1 = ev(), ev(), ev()
    t0.record(s_test)
    s_agg.wait_event(t0)
    with torch.cuda.stream(s_agg):
        for k in range(48):                                                        # ~0.45 ms each: ~20 ms of traffic
            (dst if k % 2 == 0 else src).copy_(src if k % 2 == 0 else dst)
            if k == 0:
                a0.record(s_agg)                                                   # the tested launches start after the
                s_test.wait_event(a0)                                              # first copy, with 47 more queued
    a1.record(s_agg)
    marks = []
    for i in range(1, len(outs)):
        b, e = ev(), ev()
        b.record(s_test)
        launch(i, s_test.cuda_stream)
        e.record(s_test)
        marks.append((b, e))
    torch.cuda.synchronize()
    lo, hi = t0.elapsed_time(a0), t0.elapsed_time(a1)
    inside = sum(1 for b, e in marks if t0.elapsed_time(b) >= lo and t0.elapsed_time(e) <= hi)
    return inside / len(marks), hi - lo


def _assert_identical(name, outs, frac, window):
    bad = [i for i in range(1, len(outs)) if not torch.equal(outs[i].nan_to_num(), outs[0].nan_to_num())
           or not torch.equal(outs[i].isnan(), outs[0].isnan())]
    assert not bad, f"{name}: {len(bad)} of {len(outs) - 1} contended launches differ from the uncontended one (e.g. {bad[:5]})"
    print(f"{name}: {len(outs) - 1} contended launches bit-identical, {100 * frac:.0f} % inside the aggressor's "
          f"{window:.1f} ms window")
    assert frac >= MIN_OVERLAP, f"{name}: only {100 * frac:.0f} % of the launches overlapped the aggressor ({window:.1f} ms)"


THIN4_CASES = [
    # ncols, dy channels (NJ = 1, 2, 4, 8), H, W, accumulate
    (1, 16, 45, 61, False),
    (2, 32, 33, 47, True),
    (3, 64, 130, 70, False),
    (4, 100, 21, 33, True),
    (4, 128, 45, 61, False),
    (4, 128, 3, 100, True),
    # the shapes above are walked in one row of output per wave (nhr = 3): the row loop's back edge and the entry into it
    # from the peeled first iteration never run.  These take walks of 5, 3 and 2 rows (t4m_th):
    (4, 128, 256, 256, False),
    (1, 16, 256, 256, True),
    (2, 32, 192, 160, False),
    (3, 64, 128, 128, True),
]


@pytest.mark.parametrize("case", THIN4_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_thin4_contended(dev, case):
    ncols, Cd, Hh, Ww, acc = case
    lib = N.lib()
    g_ = torch.Generator().manual_seed(ncols * 1000 + Cd + 7)
    Cl = 8
    w = torch.randn(Cd, Cl, 3, 3, generator=g_) / (Cd * 9) ** 0.5
    dy = torch.randn(1, Cd, Hh, Ww, generator=g_)
    base = torch.randn(1, Cl, Hh, Ww, generator=g_)
    res = {}
    for dt in (torch.float64, torch.float32):
        xx = torch.zeros(1, Cl, Hh, Ww, dtype=dt, requires_grad=True)
        y = torch.nn.functional.conv2d(xx, w.to(dt), None, 1, 1)
        (y * dy.to(dt)).sum().backward()
        res[dt] = (xx.grad + (base.to(dt) if acc else 0))[:, :ncols]
    packed, _, do = H.pack(w.to(dev))
    dyb = H.to_nhwc(dy.to(dev))
    Cg = round_up(Cl, 4)
    init = H.to_nhwc(base.to(dev)) if acc else torch.full((Hh * Ww * Cg,), float("nan"), device=dev)
    K = 300
    outs = [init.clone() for _ in range(K + 1)]
    descs = [N.DipConvDesc(dyb.data_ptr(), Hh, Ww, round_up(Cd, 4), round_up(Cd, 4), N.DipTransform(None, None, 1.0),
                           packed.data_ptr() + 4 * do, None, o.data_ptr(), Hh, Ww, Cg, Cl, 0, 3, 1, N.PAD_ZERO, 1, 1,
                           1 if acc else 0, None, 1, None) for o in outs]

    def launch(i, st):
        N.check(lib.dip_conv_thin4(C.byref(descs[i]), ncols, st), "conv_thin4")

    frac, window = _contended(dev, launch, outs)
    got = H.from_nhwc(outs[0], Cl, Hh, Ww)
    TK._check("conv_thin4", got[:, :ncols], res[torch.float64], res[torch.float32])
    _assert_identical(f"conv_thin4 NJ={(Cd + 15) // 16 if Cd <= 64 else 8}", outs, frac, window)


SMALL_CASES = [
    (128, 128, 3, 1, REFLECT, 32, 32, True),
    (132, 128, 3, 1, REFLECT, 32, 32, True),     # the 4-channel K tail
    (128, 4, 1, 1, REFLECT, 19, 27, False),
    (36, 64, 3, 1, ZERO, 21, 13, True),
]


@pytest.mark.parametrize("case", SMALL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_small_forward_contended(dev, case):
    lib = N.lib()
    Cin, Cout, ks, stride, pad, Hh, Ww, has_tr = case
    x, w, b, ta, tb = TK._mk(case)
    slope = 0.2
    ref = {dt: TK._ref_conv(TK._apply_tr(x, ta, tb, slope, dt) if has_tr else x.to(dt), w, b, stride, pad, dt)
           for dt in (torch.float64, torch.float32)}
    P = (ks - 1) // 2
    Ho, Wo = (Hh + 2 * P - ks) // stride + 1, (Ww + 2 * P - ks) // stride + 1
    xb = H.to_nhwc(x.to(dev))
    packed, fo, _ = H.pack(w.to(dev))
    Cy, CoutP = round_up(Cout, 4), round_up(Cout, 32)
    trd, keep = H.transform(ta.to(dev), tb.to(dev), slope) if has_tr else H.transform(None, None, 1.0)
    bb = b.to(dev).contiguous().float()
    K = 200
    outs = [torch.full((Ho * Wo * Cy,), float("nan"), dtype=torch.float32, device=dev) for _ in range(K + 1)]
    descs = []
    for o in outs:
        d = N.DipConvDesc(xb.data_ptr(), Hh, Ww, round_up(Cin, 4), round_up(Cin, 4), trd, packed.data_ptr() + 4 * fo,
                          bb.data_ptr(), o.data_ptr(), Ho, Wo, Cy, Cout, 0, ks, stride, pad if P > 0 else N.PAD_ZERO, P, 1, 0,
                          None, 1, None)
        descs.append(d)
    rows = lib.dip_conv_small_rows(C.byref(descs[0]))
    assert rows > 0, "shape not served by dip_conv_small"
    stats = [torch.full((rows * 3 * CoutP,), float("nan"), dtype=torch.float32, device=dev) for _ in outs]
    for d, s in zip(descs, stats):
        d.stats = s.data_ptr()

    def launch(i, st):
        N.check(lib.dip_conv_small(C.byref(descs[i]), st), "conv_small")

    frac, window = _contended(dev, launch, outs)
    TK._check("conv_small", H.from_nhwc(outs[0], Cout, Ho, Wo), ref[torch.float64], ref[torch.float32])
    # the uncontended partial rows -> per-channel count / mean / biased variance of the fp64 output (as test_small_gpu.py)
    st = stats[0].view(rows, 3, CoutP).cpu().double().numpy()
    n, m, M2 = st[:, 0, :Cout], st[:, 1, :Cout], st[:, 2, :Cout]
    N_ = n.sum(0)
    mean = (n * m).sum(0) / N_
    var = (M2.sum(0) + (n * (m - mean) ** 2).sum(0)) / N_
    r = ref[torch.float64][0].reshape(Cout, -1)
    assert np.allclose(N_, r.shape[1])
    assert np.allclose(mean, r.mean(1).numpy(), rtol=1e-5, atol=1e-5 * float(r.std()))
    assert np.allclose(var, r.var(1, unbiased=False).numpy(), rtol=2e-5)
    _assert_identical("conv_small", outs, frac, window)
    _assert_identical("conv_small stats", stats, frac, window)
