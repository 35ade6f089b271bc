"""Per-kernel parity of the closure side on a real MI355X: the fused loss head (csrc/loss_kernels.hip, all five forward
bodies), MaxPool2d / AvgPool2d(2, 2) with odd borders and ties (csrc/upcat_kernels.hip) and the Downsampler's fixed-taps
and dense kernels (csrc/misc_kernels.hip), each against a plain torch-CPU evaluation of the same op in float64, with the
float32 torch result as the yardstick (test_kernels_gpu._check).  Shapes are the smallest that reach the code in question:
strips shorter than a block, a second trip through the pixel loop, odd sizes, images barely larger than the filter."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import dip_native as N  # noqa: E402
from dip_native import round_up  # noqa: E402
import hipops as H  # noqa: E402
from test_kernels_gpu import _apply_tr, _check  # noqa: E402


# ----------------------------------------------------------------------------- loss head
def head_body(Cin, Cout):
    """The forward body dip_loss_head_fwd launches, by its own rule: the coalesced kernel needs Cin / 4 = nc4 a power of two
    in 4..32 and a lane per output channel inside a pixel's lane group (Cout <= nc4); everything else is lane-per-pixel."""
    nc4 = (Cin + 3) // 4
    if nc4 > 32 or (nc4 & (nc4 - 1)) != 0 or nc4 < 4 or Cout > nc4:
        return "general"
    return f"coal{nc4}"


HW_SHORT, HW_RAGGED, HW_CONTROL, HW_TWO_TRIPS = 77, 256 * 3 + 37, 64 * 96, 513 * 513
LRELU, NO_TR, SLOPE1 = 0.2, None, 1.0
SWISH, ELU, RELU = -1.0, -2.0, -3.0


def _head_cases():
    """(Cin, Cout, HW, mask, sigmoid, transform, wide channel stride, gscale, bias).  Per Cin: every HW class x every
    mask kind, the other axes rotating through them; then the activation codes, the 513 x 513 size and a non-binary mask."""
    cases = []
    for ci, Cin in enumerate((4, 8, 16, 32, 64, 128, 12, 20, 132)):
        for hi, HW in enumerate((HW_SHORT, HW_RAGGED, HW_CONTROL)):
            for mi, mask in enumerate(("nomask", "mask1", "maskC")):
                k = hi * 3 + mi
                Cout = (1, 2, 3, 4)[(k + 3 * (ci // 5)) % 4] if Cin in (16, 128) else (3, 1)[k % 2]
                cases.append((Cin, Cout, HW, mask, (k + ci) % 2 == 0, (NO_TR, LRELU, SLOPE1)[(k + ci) % 3],
                              (k // 2 + ci) % 2 == 1, (None, 3.0)[(k + ci // 2) % 2], k % 5 != 4))
    for Cin in (16, 128, 20):
        for j, act in enumerate((SWISH, ELU, RELU)):
            cases.append((Cin, (3, 1, 2)[j] if Cin != 20 else (3, 1, 3)[j], HW_RAGGED, ("mask1", "nomask", "maskC")[j],
                          j != 1, act, j == 2, (3.0, None, 3.0)[j], True))
    for Cin in (16, 32, 12):
        cases.append((Cin, 3, HW_TWO_TRIPS, "nomask", True, LRELU, False, None, True))
        cases.append((Cin, 1, HW_TWO_TRIPS, "maskC", False, NO_TR, False, 3.0, True))
    cases.append((16, 4, HW_RAGGED, "randmask", True, LRELU, False, 3.0, True))
    cases.append((128, 3, HW_SHORT, "randmask", False, LRELU, True, None, True))
    assert len(set(cases)) == len(cases) < 150
    return cases


HEAD_CASES = _head_cases()
# the table above must keep reaching: every body at every HW class, mask kind and sigmoid setting; Cout = 4 on 4 lanes
for _b in ("general", "coal4", "coal8", "coal16", "coal32"):
    _mine = [c for c in HEAD_CASES if head_body(c[0], c[1]) == _b]
    assert {c[2] for c in _mine} >= {HW_SHORT, HW_RAGGED, HW_CONTROL}, _b
    assert {c[3] for c in _mine} >= {"nomask", "mask1", "maskC"} and {c[4] for c in _mine} == {True, False}, _b
    assert {c[5] for c in _mine} >= {NO_TR, LRELU, SLOPE1} and {c[6] for c in _mine} == {True, False}, _b
    assert {c[7] for c in _mine} == {None, 3.0}, _b
assert {head_body(c[0], c[1]) for c in HEAD_CASES if c[2] == HW_TWO_TRIPS} == {"general", "coal4", "coal8"}
assert (16, 4) in {(c[0], c[1]) for c in HEAD_CASES} and head_body(16, 4) == "coal4"
assert {c[1] for c in HEAD_CASES if c[0] == 16} == {c[1] for c in HEAD_CASES if c[0] == 128} == {1, 2, 3, 4}


def _head_id(c):
    Cin, Cout, HW, mask, sig, act, wide, gs, bias = c
    actn = {None: "notr", LRELU: "lrelu", SLOPE1: "slope1", SWISH: "swish", ELU: "elu", RELU: "relu"}[act]
    return "-".join([head_body(Cin, Cout), f"{Cin}to{Cout}", f"hw{HW}", mask, "sig" if sig else "lin", actn,
                     "wide" if wide else "tight", "gs3" if gs else "gsnull", "bias" if bias else "nobias"])


def _head_inputs(c, seed=0):
    Cin, Cout, HW, mask, sig, act, wide, gs, bias = c
    g = torch.Generator().manual_seed(seed + 1000 * Cin + HW % 1000 + Cout)
    u = torch.randn(1, Cin, 1, HW, generator=g)
    w = torch.randn(Cout, Cin, generator=g) / Cin ** 0.5
    b = torch.randn(Cout, generator=g) * 0.5 if bias else None
    t = torch.rand(Cout, HW, generator=g)
    a = bb = None
    if act is not None:
        a = torch.rand(Cin, generator=g) + 0.5
        bb = torch.randn(Cin, generator=g) * 0.3
    m = None
    if mask != "nomask":
        mc = 1 if mask == "mask1" else Cout
        r = torch.rand(mc, HW, generator=g)
        m = r if mask == "randmask" else (r > 0.3).float()             # binary as in the inpainting notebook, or not
    return u, w, b, t, m, (a, bb, act if act is not None else 1.0)


def _head_ref(u, w, b, t, m, tr, sig, gs, dt):
    """float64 / float32 evaluation: (loss, out [Cout,HW], d(gscale * loss) / d(pre-sigmoid conv output) [HW,Cout])."""
    a, bb, slope = tr
    ua = _apply_tr(u, a, bb, slope, dt)
    z = F.conv2d(ua, w.to(dt)[:, :, None, None], b.to(dt) if b is not None else None)[0, :, 0, :]
    z = z.detach().requires_grad_(True)
    y = torch.sigmoid(z) if sig else z
    if m is not None:
        loss = F.mse_loss(y * m.to(dt), t.to(dt) * m.to(dt))
    else:
        loss = F.mse_loss(y, t.to(dt))
    ((gs if gs is not None else 1.0) * loss).backward()
    return loss.detach(), y.detach(), z.grad.t().contiguous()


def _dev(tr, dev):
    return tuple(v.to(dev) if torch.is_tensor(v) else v for v in tr)


def _run_head(c, dev, u, w, b, t, m, tr):
    Cin, Cout, HW, mask, sig, act, wide, gs, bias = c
    Cu = round_up(Cin, 4) + (8 if wide else 0)
    return H.loss_head(u.to(dev), w.to(dev), b.to(dev) if b is not None else None, t.to(dev),
                       m.to(dev) if m is not None else None, sig, _dev(tr, dev), Cu=Cu, gscale=gs)


@pytest.mark.parametrize("case", HEAD_CASES, ids=_head_id)
def test_loss_head_forward_backward(dev, case):
    """dip_loss_head_fwd / _bwd through the descriptor: out, loss and dy of every forward body against float64."""
    Cin, Cout, HW, mask, sig, act, wide, gs, bias = case
    u, w, b, t, m, tr = _head_inputs(case)
    l64, y64, g64 = _head_ref(u, w, b, t, m, tr, sig, gs, torch.float64)
    l32, y32, g32 = _head_ref(u, w, b, t, m, tr, sig, gs, torch.float32)
    loss, out, dy = _run_head(case, dev, u, w, b, t, m, tr)
    e_loss = abs(loss.item() - l64.item())
    print(f"{_head_id(case)}: loss {loss.item():.9g} (fp64 {l64.item():.9g}, rel err {e_loss / abs(l64.item()):.2e}; "
          f"torch fp32 {abs(l32.item() - l64.item()) / abs(l64.item()):.2e})")
    _check("loss_head.out", out, y64, y32)
    _check("loss_head.dy", dy[:, :Cout], g64, g32, floor=5e-6)
    assert torch.all(dy[:, Cout:] == 0), "pad channels of dy must be written as zeros"
    assert e_loss <= 2e-6 * abs(l64.item()), (loss.item(), l64.item())
    # deterministic: fixed-order trees and a fixed-order sum of the per-block partials
    loss2, out2, dy2 = _run_head(case, dev, u, w, b, t, m, tr)
    assert loss2.item() == loss.item() and torch.equal(out2, out) and torch.equal(dy2, dy)


NO_COAL_CASES = [(16, 3, HW_RAGGED, "mask1", True, LRELU, False, None, True),
                 (32, 3, HW_RAGGED, "maskC", True, LRELU, True, None, True),
                 (64, 4, HW_RAGGED, "nomask", False, LRELU, False, None, True),
                 (128, 3, HW_RAGGED, "mask1", True, LRELU, False, None, True)]
assert [head_body(c[0], c[1]) for c in NO_COAL_CASES] == ["coal4", "coal8", "coal16", "coal32"]


@pytest.fixture(scope="module")
def no_coal_outputs(dev, tmp_path_factory):
    """`out` and `loss` of NO_COAL_CASES from ONE fresh child process with DIP_LOSS_HEAD_NO_COAL=1 (the library reads the
    switch once per process): the lane-per-pixel kernel on descriptors the coalesced kernels take by default."""
    tmp = tmp_path_factory.mktemp("no_coal")
    torch.save([_head_inputs(c) for c in NO_COAL_CASES], tmp / "in.pt")
    code = ("import sys, torch; sys.path[:0] = [%r, %r]; import test_closure_kernels_gpu as T\n"
            "dev = torch.device('cuda:0'); res = []\n"
            "for c, inp in zip(T.NO_COAL_CASES, torch.load(%r)):\n"
            "    loss, out, dy = T._run_head(c, dev, *inp)\n"
            "    res.append((loss.cpu(), out.cpu()))\n"
            "torch.save(res, %r)\n") % (os.path.dirname(__file__), os.path.dirname(N.__file__), str(tmp / "in.pt"),
                                         str(tmp / "out.pt"))
    env = dict(os.environ, DIP_LOSS_HEAD_NO_COAL="1")
    subprocess.run([sys.executable, "-c", code], check=True, env=env, timeout=300)
    return torch.load(tmp / "out.pt")


@pytest.mark.parametrize("i", range(len(NO_COAL_CASES)), ids=[_head_id(c) for c in NO_COAL_CASES])
def test_loss_head_general_kernel_on_coalesced_shapes(dev, no_coal_outputs, i):
    """DIP_LOSS_HEAD_NO_COAL=1: the lane-per-pixel kernel meets the per-op criterion where the coalesced one runs by default."""
    case = NO_COAL_CASES[i]
    assert "DIP_LOSS_HEAD_NO_COAL" not in os.environ
    u, w, b, t, m, tr = _head_inputs(case)
    l64, y64, _ = _head_ref(u, w, b, t, m, tr, case[4], None, torch.float64)
    _, y32, _ = _head_ref(u, w, b, t, m, tr, case[4], None, torch.float32)
    loss_g, out_g = no_coal_outputs[i]
    loss, out, _ = _run_head(case, dev, u, w, b, t, m, tr)
    _check("loss_head.out(default)", out, y64, y32)
    _check("loss_head.out(no_coal)", out_g, y64, y32)
    for l in (loss, loss_g):
        assert abs(l.item() - l64.item()) <= 2e-6 * abs(l64.item())


@pytest.mark.parametrize("what", ["Cout0", "Cout5", "nblk", "Cu", "mask_c"])
def test_loss_head_refuses(dev, what):
    """Descriptors dip_loss_head_fwd must refuse before it launches anything: non-zero return, a message, nothing written."""
    lib = N.lib()
    case = (16, 3, HW_RAGGED, "mask1", True, LRELU, False, None, True)
    u, w, b, t, m, tr = _head_inputs(case)
    d, bufs = H.loss_head_desc(u.to(dev), w.to(dev), b.to(dev), t.to(dev), m.to(dev), True, _dev(tr, dev))
    assert d.nblk == lib.dip_loss_head_nblk(HW_RAGGED, 16) == 4
    if what == "Cout0":
        d.Cout = 0
    elif what == "Cout5":
        d.Cout = 5
    elif what == "nblk":
        d.nblk = d.nblk + 1
    elif what == "Cu":
        d.Cu = 18
    else:
        d.mask_c = 2
    rc = lib.dip_loss_head_fwd(C.byref(d), H.stream(dev))
    torch.cuda.synchronize()
    assert rc != 0
    assert b"loss_head" in lib.dip_last_error()
    assert torch.isnan(bufs["out"][:-8]).all() and torch.isnan(bufs["loss"][0]) and torch.isnan(bufs["partials"][:-8]).all()
    # the untouched descriptor is fine
    d2, _ = H.loss_head_desc(u.to(dev), w.to(dev), b.to(dev), t.to(dev), m.to(dev), True, _dev(tr, dev))
    assert lib.dip_loss_head_fwd(C.byref(d2), H.stream(dev)) == 0
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- MaxPool2d(2, 2) / AvgPool2d(2, 2)
POOL_SHAPES = [(16, 8, 12), (30, 10, 6), (128, 16, 32), (4, 9, 13), (20, 7, 8), (8, 6, 11), (132, 5, 5), (1, 3, 2)]
_pool_id = lambda s: "x".join(map(str, s))  # noqa: E731


def _pool_input(shape, family):
    Cc, Hh, Ww = shape
    g = torch.Generator().manual_seed(100 * Cc + 10 * Hh + Ww)
    if family == "randn":
        return torch.randn(1, Cc, Hh, Ww, generator=g)
    if family == "ties":            # three levels: ties in most windows, in every pair of positions
        return torch.randint(0, 3, (1, Cc, Hh, Ww), generator=g).float()
    return torch.full((1, Cc, Hh, Ww), 1.5)


def _border_is_zero(dx, Hh, Ww):
    ok = True
    if Hh & 1:
        ok = ok and bool(torch.all(dx[:, :, Hh - 1, :] == 0))
    if Ww & 1:
        ok = ok and bool(torch.all(dx[:, :, :, Ww - 1] == 0))
    return ok


def _check_pool_stats(mr, pooled64):
    """(mean, rstd) rows of dip_bn_finalize against the pooled tensor's batch statistics (tolerances of
    test_avgpool2_forward_stats_backward)."""
    Cc = pooled64.shape[1]
    r = pooled64[0].reshape(Cc, -1)
    s = mr.cpu().double()
    assert torch.allclose(s[0], r.mean(1), rtol=1e-5, atol=1e-6)
    assert torch.allclose(s[1], 1 / torch.sqrt(r.var(1, unbiased=False) + 1e-5), rtol=1e-5)


@pytest.mark.parametrize("family", ["randn", "ties", "const"])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=_pool_id)
def test_maxpool2_forward_stats_backward(dev, shape, family):
    """conv(..., downsample_mode='max'): the maximum and its routing are exact -- dy goes to the FIRST maximal element of
    the window in scan order (ATen's `val > maxval`), a floored odd border row / column / corner gets zeros."""
    Cc, Hh, Ww = shape
    x = _pool_input(shape, family)
    xr = x.clone().requires_grad_(True)
    ref = F.max_pool2d(xr, 2, 2)
    g = torch.randn(ref.shape, generator=torch.Generator().manual_seed(3)) + 3.0       # (never 0: a misrouted dy shows)
    (ref * g).sum().backward()
    y, mr = H.pool2(x.to(dev), "max", True)
    assert torch.equal(y.cpu(), ref.detach())
    _check_pool_stats(mr, ref.detach().double())
    y2, none = H.pool2(x.to(dev), "max", False)
    assert none is None and torch.equal(y2, y)
    dx = H.pool2_bwd(g.to(dev), x.to(dev), "max").cpu()
    assert torch.equal(dx, xr.grad)
    assert _border_is_zero(dx, Hh, Ww)


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=_pool_id)
def test_avgpool2_odd_borders(dev, shape):
    """test_avgpool2_forward_stats_backward at odd sizes: the floored border of dx is zero, the statistics count the pooled
    pixels only."""
    Cc, Hh, Ww = shape
    x = _pool_input(shape, "randn")
    ref = F.avg_pool2d(x.double(), 2, 2)
    y, mr = H.pool2(x.to(dev), "avg", True)
    assert torch.allclose(y.cpu().double(), ref, rtol=1e-6, atol=1e-6)
    _check_pool_stats(mr, ref)
    g = torch.randn(ref.shape, generator=torch.Generator().manual_seed(4)) + 3.0
    xr = x.double().requires_grad_(True)
    (F.avg_pool2d(xr, 2, 2) * g.double()).sum().backward()
    dx = H.pool2_bwd(g.to(dev), x.to(dev), "avg").cpu()
    assert torch.allclose(dx.double(), xr.grad, rtol=1e-6, atol=1e-7)
    assert _border_is_zero(dx, Hh, Ww)


# ----------------------------------------------------------------------------- Downsampler
def _down_configs():
    """(kernel_type, phase, factor, preserve_size, planes, kwargs)"""
    cfg = []
    for phase in (0.5, 0):
        for f in (2, 4, 8):
            for pres in (True, False):
                cfg.append(("lanczos2", phase, f, pres, 3 if (len(cfg) % 2 == 0 or (f == 4 and phase == 0.5)) else 1, {}))
    cfg.append(("lanczos2", 0.5, 4, True, 1, {}))
    for phase in (0.5, 0):
        for f in (2, 4):
            cfg.append(("lanczos3", phase, f, (f == 2) == (phase == 0.5), 1 if f == 2 else 3, {}))
    cfg.append(("gauss12", 0, 4, True, 3, {}))
    cfg.append(("gauss1sq2", 0, 4, False, 1, {}))
    cfg.append(("box", 0.5, 4, True, 3, dict(kernel_width=4)))
    cfg.append(("box", 0.5, 4, False, 1, dict(kernel_width=4)))
    return cfg


DOWN_CONFIGS = _down_configs()
DENSE_CONFIGS = [c for c in DOWN_CONFIGS if (c[0] == "lanczos2" and c[2] in (2, 4)) or c[0] == "box"
                 or (c[0], c[2]) in (("lanczos3", 2), ("gauss12", 4))]
SIZE_CLASSES = ["exact", "ragged", "one_pixel", "one_row"]
_down_id = lambda c: f"{c[0]}-ph{c[1]}-f{c[2]}-{'same' if c[3] else 'valid'}-{c[4]}pl"  # noqa: E731


def _down_module(cfg, dev):
    from models.downsampler import Downsampler
    kt, phase, f, pres, planes, kw = cfg
    return Downsampler(n_planes=planes, factor=f, kernel_type=kt, phase=phase, preserve_size=pres, **kw).to(dev)


def _down_size(k, f, pad, cls):
    """H, W by what (H + 2 pad - k) is: a multiple of f; no multiple (source rows / columns that reach no output pixel);
    0 and 1 (1 x 1 output: every source pixel is a frame pixel of the clamp logic); 1 and a multiple (1 x n output)."""
    base = k - 2 * pad                                   # smallest legal size (1 with preserve_size and an odd filter)
    nH, nW = (3, 5) if f <= 4 else (2, 3)
    if cls == "exact":
        return base + f * nH, base + f * nW
    if cls == "ragged":
        return base + f * nH + 1, base + f * nW + f - 1
    if cls == "one_pixel":
        return base, base + 1
    return base + 1, base + f * nW


def _down_ref(x, wgt, bias, gy, f, pad, dt):
    xx, ww, bb = (v.detach().to(dt).clone().requires_grad_(True) for v in (x, wgt, bias))       # (fresh leaves: to() may alias)
    y = F.conv2d(F.pad(xx, (pad,) * 4, mode="replicate"), ww, bb, stride=f)
    (y * gy.to(dt)).sum().backward()
    return y.detach(), xx.grad, ww.grad, bb.grad


def _down_data(cfg, cls, d):
    k, f, pad, planes = d.kernel.shape[0], cfg[2], d._pad, cfg[4]
    Hh, Ww = _down_size(k, f, pad, cls)
    assert max(Hh, Ww) <= 80
    g = torch.Generator().manual_seed(Hh * 100 + Ww + k)
    x = torch.rand(1, planes, Hh, Ww, generator=g)
    Ho, Wo = (Hh + 2 * pad - k) // f + 1, (Ww + 2 * pad - k) // f + 1
    if cls == "one_pixel":
        assert (Ho, Wo) == (1, 1)
    if cls == "one_row":
        assert Ho == 1 and Wo > 1
    gy = torch.randn(1, planes, Ho, Wo, generator=g)
    return x, gy, g


@pytest.mark.parametrize("cls", SIZE_CLASSES)
@pytest.mark.parametrize("cfg", DOWN_CONFIGS, ids=_down_id)
def test_downsampler_fixed_taps(dev, cfg, cls):
    """dip_lanczos_down_fwd / _bwd against ReplicationPad2d + the dense strided Conv2d with the module's own taps on the
    channel diagonal, and the dense kernels on the same weight."""
    d = _down_module(cfg, dev)
    k, f, pad = d.kernel.shape[0], cfg[2], d._pad
    x, gy, _ = _down_data(cfg, cls, d)
    wgt, bias = d.downsampler_.weight.detach().cpu(), d.downsampler_.bias.detach().cpu()
    assert wgt.shape[-1] == k and float(bias.abs().max()) == 0
    r64 = _down_ref(x, wgt, bias, gy, f, pad, torch.float64)
    r32 = _down_ref(x, wgt, bias, gy, f, pad, torch.float32)
    xd = x.to(dev).requires_grad_(True)
    y = d(xd)
    assert not d._nondiag and y.shape == r64[0].shape
    (y * gy.to(dev)).sum().backward()
    torch.cuda.synchronize()
    _check("lanczos_down.y", y, r64[0], r32[0])
    _check("lanczos_down.gx", xd.grad, r64[1], r32[1])
    # the dense evaluation of the same taps agrees with the depth-wise kernels to rounding
    d._nondiag = True
    xe = x.to(dev).requires_grad_(True)
    ye = d(xe)
    (ye * gy.to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert torch.allclose(ye, y, rtol=1e-5, atol=2e-6)
    assert torch.allclose(xe.grad, xd.grad, rtol=1e-5, atol=2e-6)


@pytest.mark.parametrize("cls", SIZE_CLASSES)
@pytest.mark.parametrize("cfg", DENSE_CONFIGS, ids=_down_id)
def test_downsampler_dense(dev, cfg, cls):
    """opt_over='down': dip_down_dense_fwd / _bwd_data / _bwd_weight with a random dense weight and bias."""
    from utils.common_utils import get_params
    d = _down_module(cfg, dev)
    k, f, pad, planes = d.kernel.shape[0], cfg[2], d._pad, cfg[4]
    x, gy, g = _down_data(cfg, cls, d)
    wgt = torch.randn(planes, planes, k, k, generator=g) / k
    bias = torch.randn(planes, generator=g)
    sd = d.state_dict()
    sd["downsampler_.weight"], sd["downsampler_.bias"] = wgt.to(dev), bias.to(dev)
    d.load_state_dict(sd)
    assert d._nondiag                                                   # not the fixed taps any more -> dense path
    params = get_params("down", None, x, d)
    assert len(params) == 2 and all(p.requires_grad for p in params)
    r64 = _down_ref(x, wgt, bias, gy, f, pad, torch.float64)
    r32 = _down_ref(x, wgt, bias, gy, f, pad, torch.float32)
    xd = x.to(dev).requires_grad_(True)
    y = d(xd)
    (y * gy.to(dev)).sum().backward()
    torch.cuda.synchronize()
    _check("down_dense.y", y, r64[0], r32[0])
    _check("down_dense.gx", xd.grad, r64[1], r32[1])
    for got, ref, name in ((d.downsampler_.weight.grad, r64[2], "dw"), (d.downsampler_.bias.grad, r64[3], "db")):
        assert got.shape == ref.shape
        err = (got.cpu().double() - ref).abs()
        print(f"down_dense.{name}: max|err| {err.max().item():.3e}, max|ref| {ref.abs().max().item():.3e}")
        assert torch.allclose(got.cpu().double(), ref, rtol=2e-5, atol=2e-6 * float(ref.abs().max())), name
