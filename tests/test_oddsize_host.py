"""CPU-side proofs about the odd-size GPU cases (tests/test_oddsize_gpu.py, tests/test_upcat_crop_gpu.py: the tables are
imported, not copied): every case reaches the edge it is meant to reach, the kernel it is meant for takes it, and its fp64
reference moves by far more than the per-op tolerance when the last padded row or column is dropped -- so a kernel that
mis-indexes that row can not pass.  Nothing here needs a GPU.

Which check applies to which case:

  padding      edge-reach identity   sensitivity (drop the last row / column the windows read)
  REFLECT      yes                   yes: forward output and weight gradient
  REPLICATE    P - 1 rows (even k)   yes, on the last row that IS read (see test_oddsize_gpu.reaches_edge)
  ZERO         yes                   no: the dropped row is zero already; the identity is what these cases pin
"""
import pytest
import torch
import torch.nn.functional as F

import test_oddsize_gpu as OS
import test_upcat_crop_gpu as UC
import test_kernels_gpu as TK
from test_kernels_gpu import REFLECT, ZERO, REPLICATE

ALL = [(f, c) for f, cases in OS.FAMILIES.items() for c in cases]
FAR = 1000.0           # "far more than the tolerance": three orders of magnitude


def _ids(fc):
    return fc[0] + "-" + OS._id(fc[1])


@pytest.mark.parametrize("fc", ALL, ids=_ids)
def test_case_reaches_the_edge_and_its_kernel(built, fc, monkeypatch):
    family, case = fc
    Cin, Cout, ks, stride, pad, Hh, Ww = case[:7]
    assert stride == 2 and (Hh % 2 == 1 or Ww % 2 == 1)
    assert OS.reaches_edge(case), OS.pad_rows_read(case)
    if ks % 2 == 1:        # the identity of the odd dimensions, spelled out
        P, (Ho, Wo) = (ks - 1) // 2, OS.out_dims(case)
        assert Hh % 2 == 0 or (Ho - 1) * 2 + ks - 1 - P == Hh - 1 + P
        assert Ww % 2 == 0 or (Wo - 1) * 2 + ks - 1 - P == Ww - 1 + P
    if family == "thin_s2":
        monkeypatch.setenv("DIP_THIN_ALL", "1")
    OS.expect_routing(family, case, OS.routing(family, case, built))


def test_tables_vary_what_they_should():
    for family, cases in OS.FAMILIES.items():
        dims = [OS.out_dims(c) for c in cases]
        assert any(Ho % 8 for Ho, _ in dims) and any(Wo % 16 for _, Wo in dims), family      # ragged 8 x 16 tiles, each dimension
    igemm = [c for f in OS.IGEMM_FAMILIES for c in OS.FAMILIES[f]]
    for cases in (igemm, OS.SMALL_S2_CASES, OS.THIN_S2_CASES):
        par = {(c[5] % 2, c[6] % 2) for c in cases}
        assert {(1, 0), (1, 1)} <= par or {(0, 1), (1, 1)} <= par, par
    assert {(1, 0), (0, 1), (1, 1)} <= {(c[5] % 2, c[6] % 2) for c in igemm}                # an H / W swap can not hide
    assert {REFLECT, ZERO} <= {c[4] for c in igemm} and {REFLECT, ZERO} <= {c[4] for c in OS.SMALL_S2_CASES}
    assert {True, False} <= {c[7] for c in igemm} and {True, False} <= {c[7] for c in OS.SMALL_S2_CASES}
    assert all(c in igemm for c in OS.SLOPE)


def _padded_eval(case, xp, w, b, dy, dt):
    ww = w.to(dt).detach().clone().requires_grad_(True)
    y = F.conv2d(xp.to(dt), ww, b.to(dt), stride=2)
    (y * dy.to(dt)).sum().backward()
    return y.detach(), ww.grad


@pytest.mark.parametrize("fc", [fc for fc in ALL if fc[1][4] != ZERO], ids=_ids)
def test_reference_sees_a_dropped_pad_row_or_column(fc):
    """The fp64 forward output and weight gradient with the last padded row (column) that a window reads zeroed instead of
    mirrored / replicated, against the tolerance TK._check would apply to the intact reference."""
    family, case = fc
    Cin, Cout, ks, stride, pad, Hh, Ww, use_tr = case
    P = (ks - 1) // 2
    slope = OS.SLOPE.get(case, 0.2)
    x, w, b, a, bb = TK._mk(case)
    mode = "reflect" if pad == REFLECT else "replicate"
    xp = {dt: F.pad(TK._apply_tr(x, a, bb, slope, dt), (P,) * 4, mode=mode) for dt in (torch.float64, torch.float32)}
    Ho, Wo = OS.out_dims(case)
    dy = torch.randn(1, Cout, Ho, Wo, generator=torch.Generator().manual_seed(9))
    y64, dw64 = _padded_eval(case, xp[torch.float64], w, b, dy, torch.float64)
    y32, dw32 = _padded_eval(case, xp[torch.float32], w, b, dy, torch.float32)
    assert torch.equal(y64, TK._ref_conv(TK._apply_tr(x, a, bb, slope, torch.float64), w, b, 2, pad, torch.float64))

    def tol(r64, r32, floor):
        return max(TK.PER_OP_RATIO * (r32.double() - r64).abs().max().item(), floor * r64.abs().max().item())

    ty, tw = tol(y64, y32, 2e-6), tol(dw64, dw32, 4e-6)
    rb, rr = OS.pad_rows_read(case)
    checked = 0
    for axis, S, nread in ((2, Hh, rb), (3, Ww, rr)):
        if S % 2 == 0:
            continue                       # even dimension: what the even-size tests of the suite already reach
        last = P + S - 1 + nread           # padded coordinate of the last row / column any window reads
        assert nread >= 1 and (last == S + 2 * P - 1 or ks % 2 == 0)
        xd = xp[torch.float64].clone()
        xd.select(axis, last).zero_()
        yd, dwd = _padded_eval(case, xd, w, b, dy, torch.float64)
        ey, ew = (yd - y64).abs().max().item(), (dwd - dw64).abs().max().item()
        assert ey >= FAR * ty and ew >= FAR * tw, (axis, ey / ty, ew / tw)
        checked += 1
    assert checked >= 1


# ----------------------------------------------------------------------------- upsample + concat geometry
def _planned(net, Hh, Ww, Cin=8):
    eng = net.__dict__["_dip_engine"]
    eng._build_arenas(torch.device("cpu"))
    eng._build_plan(Hh, Ww, Cin)
    return eng


def test_upcat_geometry_is_the_planners(built):
    """upcat_geom (what the GPU cases fill DipUpcatDesc with) == dip_engine._plan_scale on dry-planned engines, at every scale
    with a skip branch; the first two crop cases are the geometry of real nets."""
    from models.skip import skip
    pooled = lambda: skip(8, 3, [16, 16], [16, 16], [4, 4], downsample_mode="avg", pad="reflection")
    noskip = lambda: skip(8, 3, [16, 16], [16, 16], [4, 0], pad="reflection")
    plain = lambda: skip(8, 3, [16, 16, 16], [16, 16, 16], [4, 4, 4], pad="reflection")
    seen = {}
    for make, sizes in ((pooled, [(30, 33), (31, 45), (29, 46)]), (noskip, [(30, 47), (29, 46), (33, 35)]),
                        (plain, [(25, 39), (25, 38), (37, 50)])):
        for Hh, Ww in sizes:
            eng = _planned(make(), Hh, Ww)
            for s in eng.sc:
                st = s.st
                if not s.ns:
                    continue
                deep = st["deep"]
                assert UC.upcat_geom(st["H"], st["W"], deep.H, deep.W) == (st["Ho"], st["Wo"], st["geom"])
                seen[(st["H"], st["W"], deep.H, deep.W)] = st["geom"]
    for case in UC.UPCAT_CASES:
        UC._check_geom(case)
    assert seen[UC.UPCAT_CASES[0][2:6]] is None                         # 25 x 39 over 13 x 20: the default geometry, odd
    assert seen[UC.UPCAT_CASES[3][2:6]]["os_y"] == 1                    # the pooling net at 30 x 33
    assert seen[UC.UPCAT_CASES[4][2:6]]["od_y"] == 1                    # the net without a skip at scale 1, at 30 x 47


@pytest.mark.parametrize("case", [c for c in UC.UPCAT_CASES if c[6] == "bilinear" and c[7] and any(k[:2] == "od" for k in c[7])],
                         ids=lambda c: "x".join(map(str, c[:7])))
def test_upcat_reference_sees_a_clamp_at_the_cropped_size(case):
    """A bilinear source index clamped at the cropped size instead of the deep size: far outside the tolerance."""
    inputs = UC.upcat_inputs(case)
    c64, c32 = UC.upcat_ref(case, torch.float64, inputs=inputs), UC.upcat_ref(case, torch.float32, inputs=inputs)
    bad = UC.upcat_ref(case, torch.float64, inputs=inputs, clamp_at_crop=True)
    tol = max(TK.PER_OP_RATIO * (c32.double() - c64).abs().max().item(), 2e-6 * c64.abs().max().item())
    assert (bad - c64).abs().max().item() >= FAR * tol
