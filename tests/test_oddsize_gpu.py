"""Parity of the stride-2 kernels at ODD image sizes on a real MI355X.  A strided conv gives ceil(S / 2); for a k x k, pad
(k - 1) / 2, stride-2 conv the last window reaches the bottom / right padding only when S is odd, so at the even sizes of the
other kernel tests the last mirror (or zero) row and column are never read (3x3) or only P - 1 of the P are (5x5, 7x7).  Every
family of stride-2 kernels runs here at H odd / W even, H even / W odd and both odd, with reflection and zero padding, with
and without the producer transform in the loader: forward with the BatchNorm partials, weight / bias gradient and data
gradient against torch-CPU fp64 evaluations of the reference ops (nn.ReflectionPad2d + nn.Conv2d, models/common.py:114-124
of the reference; autograd), through the drivers and with the per-op criterion of test_kernels_gpu.py / test_small_gpu.py.

Before a launch each test asserts ON THE HOST which kernel takes the descriptor (`routing` below) and that the case reaches
the edge (`reaches_edge`); tests/test_oddsize_host.py proves on the CPU that each case's fp64 reference moves by far more
than the tolerance when the last padded row or column is dropped."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import dip_native as N  # noqa: E402
from dip_native import round_up  # noqa: E402
import test_kernels_gpu as TK  # noqa: E402
import test_small_gpu as TS  # noqa: E402
from test_kernels_gpu import REFLECT, ZERO, REPLICATE  # noqa: E402

# Cin, Cout, ks, stride, pad, H, W, transform -- the layout of TK.CONV_CASES
DMA_S2_CASES = [
    # LDS-DMA strided forward (dip_conv_variant == 5): source row 2 * (...) + parity; one pass and the planned split-K
    (128, 128, 3, 2, REFLECT, 33, 50, True),     # H odd: 17 x 25 output, ragged 8 x 16 tiles in both dimensions
    (128, 128, 3, 2, ZERO, 34, 51, True),        # W odd, zero padding (identity only: the dropped column is zero anyway)
    (32, 128, 3, 2, REFLECT, 37, 51, False),     # both odd, one 32-channel unit, no transform
    (256, 128, 3, 2, REFLECT, 21, 19, True),     # both odd, 8 units, W < H
    (36, 64, 3, 2, ZERO, 17, 33, True),          # 32 + 4-channel tail, 64 columns, zero padding
]
REG3_S2_CASES = [
    # register-staged launch_bn<3, 2, 16> (variant 0): what the LDS-DMA kernel refuses
    (320, 64, 3, 2, REFLECT, 19, 23, True),      # > 288 transformed channels
    (64, 128, 3, 2, REFLECT, 21, 35, True),      # Swish (activation code -1) is applied at staging: SLOPE below
]
REG57_S2_CASES = [
    # register-staged launch_bn<5, 2, 8> / <7, 2, 8>: all P = 2 / 3 padded rows and columns are read only at odd sizes
    (16, 32, 5, 2, REFLECT, 33, 35, True),
    (1, 16, 5, 2, ZERO, 35, 32, False),          # H odd / W even; one input plane
    (128, 128, 5, 2, REFLECT, 15, 23, True),
    (16, 32, 7, 2, REFLECT, 33, 37, True),
    (2, 16, 7, 2, ZERO, 25, 33, False),
]
LANCZOS_CASES = [
    # the Downsampler's dense k x k stride-2 conv behind replication padding, launch_bn<8, 2, 8> / <12, 2, 8>.  EVEN filters:
    # H + 2 P - k is odd at an odd H, the last padded row can not be a window's last row at ANY odd size (it is at the even
    # sizes of TK.CONV_CASES); what odd sizes add here is the floor in Hout and the P - 1 replicated rows: see reaches_edge
    (16, 16, 8, 2, REPLICATE, 33, 35, False),
    (12, 12, 12, 2, REPLICATE, 25, 41, False),
]
THIN_S2_CASES = [
    # conv_thin_kernel<., 2> and wgrad_thin at stride 2 (under DIP_THIN_ALL, as tests/test_thin_gpu.py): >= 4625 output pixels.
    # conv_thin serves no stride-2 data gradient: forward and weight gradient only
    (16, 32, 5, 2, REFLECT, 139, 137, True),     # 70 x 69
    (16, 48, 3, 2, ZERO, 141, 135, True),        # 71 x 68: 3 column blocks, zero padding
    (32, 64, 5, 2, REFLECT, 137, 140, True),     # 69 x 70: H odd / W even, 2 chunks of 16 channels
]
SMALL_S2_CASES = [
    # dip_conv_small: forward, data gradient (parity classes) and data gradient with the fused BatchNorm backward
    (128, 128, 3, 2, REFLECT, 19, 27, True),
    (32, 64, 5, 2, REFLECT, 25, 37, True),
    (4, 16, 5, 2, REFLECT, 33, 47, False),
    (128, 64, 3, 2, ZERO, 19, 22, True),         # H odd / W even
    (16, 8, 7, 2, REFLECT, 17, 21, True),
]
# producer activation of a case: LeakyReLU(0.2) unless named here (DipTransform.slope codes: -1 Swish)
SLOPE = {(64, 128, 3, 2, REFLECT, 21, 35, True): -1.0}

WGRAD_TAP_CFGS = [
    # Cin, Cout, ks, stride, H, W, tap_groups, chan_block, nsplit: the generic dip_conv_wgrad kernel (reflection padding,
    # transform on: TK.test_conv_wgrad_tap_groups_and_channel_blocks), 9 / 3 taps per workgroup, 5x5 by tap and by filter row
    (128, 128, 3, 2, 33, 35, 9, 0, 4),
    (128, 128, 3, 2, 33, 35, 3, 0, 4),
    (32, 128, 3, 2, 35, 61, 3, 0, 2),
    (128, 128, 5, 2, 15, 23, 25, 0, 2),
    (64, 128, 5, 2, 29, 45, 5, 0, 4),
]
THIN_CIN_CASES = [
    # <= 4 input channels: thin_cin_wgrad_kernel (weight gradient only: the forward is that of REG57 / the first conv)
    (1, 128, 5, 2, ZERO, 41, 37, False),
    (3, 8, 3, 2, REFLECT, 33, 49, False),
]

FAMILIES = {"dma_s2": DMA_S2_CASES, "reg3_s2": REG3_S2_CASES, "reg57_s2": REG57_S2_CASES, "lanczos": LANCZOS_CASES,
            "thin_s2": THIN_S2_CASES, "small_s2": SMALL_S2_CASES, "thin_cin": THIN_CIN_CASES,
            "wgrad_taps": [(c[0], c[1], c[2], c[3], REFLECT, c[4], c[5], True) for c in WGRAD_TAP_CFGS]}
_FAKE = 1 << 20            # a non-null pointer for descriptors that are only shown to the host-side predicates


def _id(c):
    return "x".join(map(str, c))


def out_dims(case):
    Cin, Cout, ks, stride, pad, Hh, Ww = case[:7]
    P = (ks - 1) // 2
    return (Hh + 2 * P - ks) // stride + 1, (Ww + 2 * P - ks) // stride + 1


def pad_rows_read(case):
    """(bottom, right): how many of the P padded rows / columns the LAST window of the conv reads."""
    Cin, Cout, ks, stride, pad, Hh, Ww = case[:7]
    P = (ks - 1) // 2
    Ho, Wo = out_dims(case)
    return (Ho - 1) * stride + ks - 1 - P - (Hh - 1), (Wo - 1) * stride + ks - 1 - P - (Ww - 1)


def reaches_edge(case):
    """(Ho - 1) * 2 + ks - 1 - P == H - 1 + P in every ODD dimension (and likewise for W): the last window reads all P padded
    rows.  In an even dimension an odd filter reads P - 1 of them (what the even-size tests cover).  An even filter (the
    Lanczos convs) reads P - 1 in an odd dimension and all P in an even one: nothing can be added to the identity there."""
    Cin, Cout, ks, stride, pad, Hh, Ww = case[:7]
    P = (ks - 1) // 2
    rb, rr = pad_rows_read(case)
    want = lambda S: P if (S % 2 == 1) == (ks % 2 == 1) else P - 1
    return (Hh % 2 == 1 or Ww % 2 == 1) and rb == want(Hh) and rr == want(Ww)


def fwd_desc(case, ksplit=1, stats=True):
    """The descriptor hipops.conv_fwd / conv_small_fwd build for `case` (pointers fake: host-side predicates only)."""
    Cin, Cout, ks, stride, pad, Hh, Ww, use_tr = case
    P = (ks - 1) // 2
    Ho, Wo = out_dims(case)
    tr = N.DipTransform(_FAKE, _FAKE, SLOPE.get(case, 0.2)) if use_tr else N.DipTransform(None, None, 1.0)
    return N.DipConvDesc(_FAKE, Hh, Ww, round_up(Cin, 4), round_up(Cin, 4), tr, _FAKE, _FAKE, _FAKE, Ho, Wo, round_up(Cout, 4),
                         Cout, 0, ks, stride, pad if P > 0 else N.PAD_ZERO, P, 1, 0, _FAKE if stats else None, ksplit,
                         _FAKE if ksplit > 1 else None)


def dgrad_desc(case, ksplit=1):
    """The descriptor hipops.conv_dgrad / conv_small_dgrad build for the data gradient of `case`."""
    Cin, Cout, ks, stride, pad, Hh, Ww = case[:7]
    P = (ks - 1) // 2
    Ho, Wo = out_dims(case)
    reflect = pad in (REFLECT, REPLICATE) and P > 0
    p = P if reflect else 0
    return N.DipConvDesc(_FAKE, Ho, Wo, round_up(Cout, 4), round_up(Cout, 4), N.DipTransform(None, None, 1.0), _FAKE, None,
                         _FAKE, Hh + 2 * p, Ww + 2 * p, round_up(Cin, 4), Cin, 0, ks, 1, N.PAD_ZERO,
                         (ks - 1) if reflect else (ks - 1 - P), stride, 0, None, ksplit, _FAKE if ksplit > 1 else None)


def wgrad_desc(case, nsplit=1, tap_groups=0, chan_block=0):
    Cin, Cout, ks, stride, pad, Hh, Ww, use_tr = case
    P = (ks - 1) // 2
    Ho, Wo = out_dims(case)
    tr = N.DipTransform(_FAKE, _FAKE, SLOPE.get(case, 0.2)) if use_tr else N.DipTransform(None, None, 1.0)
    return N.DipWgradDesc(_FAKE, Hh, Ww, round_up(Cin, 4), Cin, tr, _FAKE, Ho, Wo, round_up(Cout, 4), Cout, ks, stride,
                          pad if P > 0 else N.PAD_ZERO, P, _FAKE, _FAKE, nsplit, tap_groups, chan_block)


def planned_ksplit(case):
    Ho, Wo = out_dims(case)
    return N.conv_plan(Ho, Wo, round_up(case[0], 4), case[1], case[2], case[3])[0]


def routing(family, case, lib=None):
    """Host-side proof of which kernel runs `case`: dict(fwd=[variant one pass, variant planned split-K], dgrad=variant,
    small_rows=..., thin=..., wgrad_thin=..., wgrad_bf3=...), from the library's own predicates."""
    lib = lib or N.lib()
    Cin, Cout, ks, stride = case[:4]
    Ho, Wo = out_dims(case)
    d1, dk = fwd_desc(case), fwd_desc(case, planned_ksplit(case))
    dg = dgrad_desc(case)
    return dict(fwd=[lib.dip_conv_variant(C.byref(d1)), lib.dip_conv_variant(C.byref(dk))],
                dgrad=lib.dip_conv_variant(C.byref(dg)),
                small_rows=lib.dip_conv_small_rows(C.byref(fwd_desc(case, stats=False))),
                small_rows_dgrad=lib.dip_conv_small_rows(C.byref(dg)),
                thin=lib.dip_conv_thin_eligible(C.byref(d1)),
                wgrad_thin=lib.dip_wgrad_thin_shape_ok(Ho, Wo, Cin, Cout, ks, stride),
                wgrad_bf3=lib.dip_wgrad_bf3_eligible(C.byref(wgrad_desc(case))))


# what `routing` must say per family.  fwd: dip_conv_variant (0 register-staged, 5 LDS-DMA strided forward, 8 conv_thin);
# dgrad: 4 = phase mode (3x3, whole 128-column blocks of the gradient), otherwise the dilated evaluation: the other 3x3 shapes
# on the LDS-DMA kernel (1), the larger filters on the register-staged kernel (0)
def expect_routing(family, case, r):
    Cin, Cout, ks = case[:3]
    assert r["wgrad_bf3"] == 0, r                                  # (stride 2: never the bf16-pipe weight gradient)
    dgrad = (4 if round_up(Cin, 32) % 128 == 0 else 1) if ks == 3 else 0
    if family == "dma_s2":
        assert r["fwd"] == [5, 5] and r["thin"] == 0 and r["dgrad"] == dgrad, r
    elif family in ("reg3_s2", "reg57_s2", "lanczos"):
        assert r["fwd"] == [0, 0] and r["thin"] == 0 and r["dgrad"] == dgrad, r
    elif family == "thin_s2":
        assert r["fwd"][0] == 8 and r["thin"] == 1 and r["wgrad_thin"] == 1, r
    elif family == "small_s2":
        assert r["small_rows"] > 0 and r["small_rows_dgrad"] > 0, r
    elif family == "thin_cin":
        assert Cin <= 4 and ks in (3, 5, 7) and r["wgrad_thin"] == 0, r
    elif family == "wgrad_taps":
        assert Cin > 4 and r["wgrad_thin"] == 0, r
    else:
        raise KeyError(family)


def _pre(family, case):
    assert reaches_edge(case), (case, pad_rows_read(case))
    expect_routing(family, case, routing(family, case))


IGEMM_FAMILIES = ["dma_s2", "reg3_s2", "reg57_s2", "lanczos"]
IGEMM = [pytest.param(f, c, id=f + "-" + _id(c)) for f in IGEMM_FAMILIES for c in FAMILIES[f]]


@pytest.mark.parametrize("split", [False, True], ids=["onepass", "splitk"])
@pytest.mark.parametrize("family,case", IGEMM)
def test_odd_conv_forward_and_stats(dev, family, case, split):
    """dip_conv_igemm forward + BatchNorm partials, one pass and the planned split-K (both on the same kernel: asserted)."""
    _pre(family, case)
    assert planned_ksplit(case) > 1                      # (every shape here is small enough to be planned split-K)
    TK.test_conv_forward_and_stats(dev, case, split, slope=SLOPE.get(case, 0.2))


# 7 slabs and the planned launch; the <= 4 input channel kernel always runs its planned slabs (hipops.conv_wgrad): one arm
WGRAD = [pytest.param(f, c, ns, id="-".join((f, _id(c), ns or "nsplit7")))
         for f in IGEMM_FAMILIES + ["small_s2", "thin_cin"] for c in FAMILIES[f] for ns in (None, "plan") if ns or c[0] > 4]


@pytest.mark.parametrize("family,case,nsplit", WGRAD)
def test_odd_conv_wgrad(dev, family, case, nsplit):
    """dW, db of the same layers through dip_conv_wgrad (generic kernel; thin_cin_wgrad_kernel for <= 4 input channels)."""
    _pre(family, case)
    if case[0] <= 4:
        assert N.wgrad_plan2(*out_dims(case), *case[:4])[1] == 1           # streaming kernel: no tap groups
    TK.test_conv_wgrad(dev, case, nsplit, slope=SLOPE.get(case, 0.2))


@pytest.mark.parametrize("split", [False, True], ids=["onepass", "splitk"])
@pytest.mark.parametrize("family,case", IGEMM)
def test_odd_conv_dgrad(dev, family, case, split):
    """Stride-2 data gradient on dip_conv_igemm: phase mode for whole 128-column blocks of a 3x3, the dilated form on the
    register-staged kernel for 5x5 / 7x7 / 8x8 / 12x12 and the other 3x3 shapes."""
    _pre(family, case)
    TK.test_conv_dgrad(dev, case, split)


# ----------------------------------------------------------------------------- conv_thin / wgrad_thin at stride 2
@pytest.fixture
def thin_all(monkeypatch):
    """As tests/test_thin_gpu.py: the kernel, not the planner's bounds, is under test (DIP_THIN_ALL is read at every call)."""
    monkeypatch.setenv("DIP_THIN_ALL", "1")


@pytest.mark.parametrize("case", THIN_S2_CASES, ids=_id)
def test_odd_conv_thin_forward_and_stats(dev, thin_all, case):
    _pre("thin_s2", case)
    Ho, Wo = out_dims(case)
    assert Ho * Wo >= 4625
    assert N.conv_plan(Ho, Wo, round_up(case[0], 4), case[1], case[2], 2) == (1, N.lib().dip_conv_ntiles(Ho, Wo), 0)
    TK.test_conv_forward_and_stats(dev, case, True)


@pytest.mark.parametrize("nsplit", [None, "plan"], ids=["nsplit7", "planned"])
@pytest.mark.parametrize("case", THIN_S2_CASES, ids=_id)
def test_odd_wgrad_thin(dev, thin_all, case, nsplit):
    _pre("thin_s2", case)
    Ho, Wo = out_dims(case)
    n, g, cb = N.wgrad_plan2(Ho, Wo, *case[:4])
    assert n == N.lib().dip_wgrad_thin_nsplit(Ho, Wo, *case[:4]) and g == 1
    TK.test_conv_wgrad(dev, case, nsplit)


# ----------------------------------------------------------------------------- dip_conv_small
@pytest.mark.parametrize("case", SMALL_S2_CASES, ids=_id)
def test_odd_conv_small_forward_and_stats(dev, case):
    _pre("small_s2", case)
    TS.test_conv_small_forward_and_stats(dev, case)


@pytest.mark.parametrize("case", SMALL_S2_CASES, ids=_id)
def test_odd_conv_small_dgrad(dev, case):
    _pre("small_s2", case)
    TS.test_conv_small_dgrad(dev, case[:7])


@pytest.mark.parametrize("case", SMALL_S2_CASES, ids=_id)
def test_odd_conv_small_dgrad_with_fused_batchnorm_backward(dev, case):
    _pre("small_s2", case)
    TS.test_conv_small_dgrad_with_fused_batchnorm_backward(dev, case[:7])


# ----------------------------------------------------------------------------- generic weight gradient, forced tap groups
@pytest.mark.parametrize("cfg", WGRAD_TAP_CFGS, ids=_id)
def test_odd_conv_wgrad_tap_groups(dev, cfg):
    Cin, Cout, ks, stride, Hh, Ww, tg, cb, nsplit = cfg
    case = (Cin, Cout, ks, stride, REFLECT, Hh, Ww, True)
    _pre("wgrad_taps", case)
    assert tg in ((3, 9) if ks == 3 else (5, 25))
    TK.test_conv_wgrad_tap_groups_and_channel_blocks(dev, cfg)
