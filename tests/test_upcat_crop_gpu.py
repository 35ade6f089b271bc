"""dip_upcat_fwd at odd and cropped geometry on a real MI355X: nn.Upsample(scale_factor=2) + Concat's centre crop
(models/common.py:19-39 of the reference: both branches are cut to the smaller size with offset (size - target) // 2) against
the same ops in torch-CPU fp64 / fp32, with the per-op criterion of test_kernels_gpu.py.  Two paths of the kernel file that
the even-size cases of test_upcat_forward_backward never run: the 2x2-block kernel at an odd size (the last up-sampled row and
column are never produced) and the one-pixel-per-thread crop kernel behind the Hs / Ws / os_* / Hd / Wd / od_* fields, which
are filled here the way dip_engine._plan_scale computes them (`upcat_geom`; tests/test_oddsize_host.py holds that function
against dry-planned engines)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import dip_native as N  # noqa: E402
from dip_native import round_up  # noqa: E402
import hipops as H  # noqa: E402
from test_kernels_gpu import _apply_tr, _check  # noqa: E402

UPCAT_CASES = [
    # ns, nd, skip H x W, deep H x W, mode, non-zero offsets the planner's rule must give (None: the default geometry)
    # default geometry at an odd size: the deep branch is ceil(S / 2), its last up-sampled row / column is dropped
    (4, 128, 25, 39, 13, 20, "bilinear", None),
    (4, 16, 25, 38, 13, 19, "nearest", None),              # H odd / W even
    (128, 128, 9, 13, 5, 7, "nearest", None),
    # general crop
    (4, 16, 30, 33, 14, 16, "bilinear", dict(os_y=1)),     # 28 x 32: the SKIP branch is cut (pooling net at 30 x 33)
    (4, 16, 30, 47, 16, 24, "bilinear", dict(od_y=1)),     # 30 x 47: the up-sampled branch is cut, rows 1..30 of 32
    (4, 16, 29, 46, 15, 24, "nearest", dict(od_x=1)),      # 29 x 46: columns 1..46 of 48 (and the last row of 30 dropped)
    (4, 16, 30, 45, 14, 24, "bilinear", dict(os_y=1, od_x=1)),     # 28 x 45: one branch cut in each axis
]


def upcat_geom(Hs, Ws, Hd, Wd):
    """Output size and the DipUpcatDesc geometry fields of a Concat of a skip branch Hs x Ws with the x2 up-sampled Hd x Wd
    branch, as dip_engine._plan_scale computes them; geom is None for the default geometry (2x2-block kernel)."""
    Hu, Wu = 2 * Hd, 2 * Wd
    Ho, Wo = min(Hs, Hu), min(Ws, Wu)
    geom = dict(Hs=Hs, Ws=Ws, os_y=(Hs - Ho) // 2, os_x=(Ws - Wo) // 2, Hd=Hd, Wd=Wd, od_y=(Hu - Ho) // 2, od_x=(Wu - Wo) // 2)
    default = (Ho, Wo) == (Hs, Ws) and Hd == (Ho + 1) // 2 and Wd == (Wo + 1) // 2 and geom["od_y"] == 0 and geom["od_x"] == 0
    return Ho, Wo, (None if default else geom)


def upcat_inputs(case, seed=5):
    ns, nd, Hs, Ws, Hd, Wd, mode, _ = case
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(1, ns, Hs, Ws, generator=g)
    d = torch.randn(1, nd, Hd, Wd, generator=g)
    # the deep branch's last two rows and columns stand out: a bilinear source clamped at the CROPPED size instead of the deep
    # size reads row Hd - 2 where row Hd - 1 belongs and is off by ~ 6
    d[:, :, -1, :] += 3.0
    d[:, :, -2, :] -= 3.0
    d[:, :, :, -1] += 3.0
    d[:, :, :, -2] -= 3.0
    a_s, b_s = torch.rand(ns, generator=g) + 0.5, torch.randn(ns, generator=g) * 0.3
    a_d, b_d = torch.rand(nd, generator=g) + 0.5, torch.randn(nd, generator=g) * 0.3
    return s, d, (a_s, b_s), (a_d, b_d)


def upcat_ref(case, dt, slope=0.2, inputs=None, clamp_at_crop=False):
    """transform per branch -> F.interpolate(x2) -> centre crop of both to the smaller size -> cat.  clamp_at_crop: the WRONG
    kernel of the host test (the up-sampled image computed from the deep rows / columns the cropped output 'should' need)."""
    ns, nd, Hs, Ws, Hd, Wd, mode, _ = case
    s, d, (a_s, b_s), (a_d, b_d) = inputs or upcat_inputs(case)
    us = _apply_tr(s, a_s, b_s, slope, dt)
    ud = _apply_tr(d, a_d, b_d, slope, dt)
    Ho, Wo = min(Hs, 2 * Hd), min(Ws, 2 * Wd)
    if clamp_at_crop:
        ud = ud[:, :, :(Ho + 1) // 2, :(Wo + 1) // 2]
        up = F.interpolate(ud, scale_factor=2, mode=mode)
        up = F.pad(up, (0, 2 * Wd - up.shape[3], 0, 2 * Hd - up.shape[2]), mode="replicate")
    else:
        up = F.interpolate(ud, scale_factor=2, mode=mode)
    oy, ox = (Hs - Ho) // 2, (Ws - Wo) // 2
    py, px = (2 * Hd - Ho) // 2, (2 * Wd - Wo) // 2
    return torch.cat([us[:, :, oy:oy + Ho, ox:ox + Wo], up[:, :, py:py + Ho, px:px + Wo]], 1)


def _run(dev, case, inputs, fin=None, slope=0.2):
    """dip_upcat_fwd (fin=None) or dip_upcat_fwd_fin (fin = dict(gamma, beta)) -> (cat flat, stats [nblk,3,Cs], state | None)."""
    lib = N.lib()
    ns, nd, Hs, Ws, Hd, Wd, mode, want = case
    s, d, (a_s, b_s), (a_d, b_d) = inputs
    Ho, Wo, geom = upcat_geom(Hs, Ws, Hd, Wd)
    st = H.stream(dev)
    sb, db = H.to_nhwc(s.to(dev)), H.to_nhwc(d.to(dev))
    ts, k1 = H.transform(a_s.to(dev), b_s.to(dev), slope)
    td, k2 = H.transform(a_d.to(dev), b_d.to(dev), slope)
    Ccat, Cs_cat = ns + nd, round_up(ns + nd, 4)
    cat = torch.full((Ho * Wo * Cs_cat,), float("nan"), device=dev)
    nblk = lib.dip_upcat_nblk(Ho, Wo, Ccat)
    stats = torch.full((nblk * 3 * Cs_cat,), float("nan"), device=dev)
    desc = N.DipUpcatDesc(sb.data_ptr(), round_up(ns, 4), ns, ts, db.data_ptr(), round_up(nd, 4), nd, td, Ho, Wo,
                          N.UP_BILINEAR if mode == "bilinear" else N.UP_NEAREST, cat.data_ptr(), Cs_cat, stats.data_ptr(), nblk,
                          **(geom or {}))
    state = None
    if fin is None:
        N.check(lib.dip_upcat_fwd(C.byref(desc), st), "upcat_fwd")
    else:
        assert lib.dip_fin_rows_ok(nblk, Ccat) == 1
        state = torch.full((4 * Cs_cat,), float("nan"), device=dev)
        rm, rv = torch.zeros(Ccat, device=dev), torch.ones(Ccat, device=dev)
        tickets = torch.zeros(8, dtype=torch.int32, device=dev)
        gam, bet = fin["gamma"].to(dev), fin["beta"].to(dev)
        if fin["fused"]:
            f = N.DipBnFin(gam.data_ptr(), bet.data_ptr(), 1e-5, 0.1, state.data_ptr(), Cs_cat, Ccat, rm.data_ptr(),
                           rv.data_ptr(), tickets.data_ptr())
            N.check(lib.dip_upcat_fwd_fin(C.byref(desc), C.byref(f), st), "upcat_fwd_fin")
        else:
            N.check(lib.dip_upcat_fwd(C.byref(desc), st), "upcat_fwd")
            N.check(lib.dip_bn_finalize(stats.data_ptr(), nblk, Cs_cat, Ccat, gam.data_ptr(), bet.data_ptr(), 1e-5, 0.1,
                                        state.data_ptr(), Cs_cat, rm.data_ptr(), rv.data_ptr(), st), "bn_finalize")
        torch.cuda.synchronize()
        assert int(tickets.abs().sum()) == 0
        state = (state.view(4, Cs_cat)[:, :Ccat].clone(), rm, rv)
    torch.cuda.synchronize()
    return cat, stats.view(nblk, 3, Cs_cat), state


def _check_geom(case):
    ns, nd, Hs, Ws, Hd, Wd, mode, want = case
    Ho, Wo, geom = upcat_geom(Hs, Ws, Hd, Wd)
    if want is None:
        assert geom is None and (Ho, Wo) == (Hs, Ws) and (Hs % 2 == 1 or Ws % 2 == 1)
    else:
        offs = {k: v for k, v in geom.items() if k[:2] in ("os", "od") and v}
        assert offs == want, (offs, want)
    return Ho, Wo, geom


@pytest.mark.parametrize("case", UPCAT_CASES, ids=lambda c: "x".join(map(str, c[:7])))
def test_upcat_forward_odd_and_cropped(dev, case):
    ns, nd, Hs, Ws, Hd, Wd, mode, want = case
    Ho, Wo, geom = _check_geom(case)
    inputs = upcat_inputs(case)
    c64, c32 = upcat_ref(case, torch.float64, inputs=inputs), upcat_ref(case, torch.float32, inputs=inputs)
    assert c64.shape == (1, ns + nd, Ho, Wo)
    cat, stats, _ = _run(dev, case, inputs)
    Ccat, Cs_cat = ns + nd, round_up(ns + nd, 4)
    _check("upcat_fwd", H.from_nhwc(cat, Ccat, Ho, Wo), c64, c32)
    assert not bool(cat.isnan().any())                      # (ns, nd are multiples of 4: no pad channels in the concat)
    stn = stats.cpu().double().numpy()
    n, m, M2 = stn[:, 0, :Ccat], stn[:, 1, :Ccat], stn[:, 2, :Ccat]
    Nt = n.sum(0)
    mean = (n * m).sum(0) / Nt
    var = (M2.sum(0) + (n * (m - mean) ** 2).sum(0)) / Nt
    r = c64[0].reshape(Ccat, -1)
    assert np.allclose(Nt, Ho * Wo)
    assert np.allclose(mean, r.mean(1).numpy(), rtol=1e-5, atol=1e-6)
    assert np.allclose(var, r.var(1, unbiased=False).numpy(), rtol=2e-5)


@pytest.mark.parametrize("case", [UPCAT_CASES[0], UPCAT_CASES[6]], ids=lambda c: "x".join(map(str, c[:7])))
def test_upcat_ticketed_form_equals_three_launches(dev, case):
    """dip_upcat_fwd_fin (the last block to arrive finalises the concat BatchNorm) on one default-geometry and one cropped
    case: the tensor bit for bit, the state as tests/test_small_gpu.py holds it (another pairing of the rows in fp64)."""
    ns, nd = case[:2]
    _check_geom(case)
    inputs = upcat_inputs(case)
    g = torch.Generator().manual_seed(3)
    fin = dict(gamma=torch.rand(ns + nd, generator=g) + 0.5, beta=torch.randn(ns + nd, generator=g))
    cat0, _, st0 = _run(dev, case, inputs, dict(fin, fused=False))
    cat1, _, st1 = _run(dev, case, inputs, dict(fin, fused=True))
    assert torch.equal(cat0, cat1) and not bool(cat0.isnan().any())
    for a, b in zip(st0, st1):
        assert torch.allclose(a, b, rtol=1e-6, atol=1e-7)
