"""Routing of descriptors that carry an activation CODE in DipTransform.slope / bnb_slope (-1 Swish, -2 ELU, -3 ReLU;
csrc/dip_common.h: dip_act, dip_act_grad).  The LDS-DMA kernels (dip_conv_variant 1 / 3 / 4 / 5) and the weights-resident 1x1
kernel (6) stage their input through dip_act_leaky, which for a code would silently compute max(t, code * t): a coded
forward descriptor must reach a kernel that evaluates dip_act -- the register-staged kernel (0), its N = 160 form (2), the
bf16-pipe kernel (7) or conv_thin (8).  dip_conv_variant and the eligibility predicates are host code: no GPU here."""
import ctypes as C

import pytest

import dip_native as N
from dip_native import round_up
from test_kernels_gpu import CONV_CASES, REFLECT

CODES = [-1.0, -2.0, -3.0]
CODE_IDS = ["swish", "elu", "relu"]
D = 1 << 20         # a non-NULL pointer: the predicates look at the fields, never at memory

# forward shapes with a producer transform: CONV_CASES' plus two that the bf16-pipe kernel takes when wp3 is set
# (the 128^2 layers of the default net: 128 tiles, 64-column form; the smallest layer of that form, 20 channels)
TR_CASES = [c for c in CONV_CASES if c[7]] + [(128, 128, 3, 1, REFLECT, 128, 128, True), (20, 128, 3, 1, REFLECT, 64, 192, True)]
# dip_conv_variant of TR_CASES with LeakyReLU (slope 0.2), without / with wp3, as the library answered before this file existed
LEAKY_VARIANTS = {
    (132, 128, 3, 1, 24, 40): (1, 1), (128, 128, 3, 2, 32, 32): (5, 5), (128, 128, 3, 1, 16, 16): (1, 1),
    (128, 128, 1, 1, 24, 24): (1, 1), (128, 3, 1, 1, 16, 48): (1, 1), (16, 32, 5, 2, 32, 32): (0, 0),
    (32, 64, 5, 1, 16, 24): (0, 0), (8, 16, 3, 1, 16, 16): (1, 1), (256, 128, 3, 1, 16, 16): (1, 1),
    (48, 128, 3, 1, 8, 16): (1, 1), (72, 64, 3, 1, 8, 16): (1, 1), (36, 64, 3, 2, 16, 32): (5, 5),
    (20, 16, 7, 1, 16, 16): (0, 0), (16, 32, 7, 2, 32, 32): (0, 0), (4, 32, 3, 1, 19, 27): (1, 1),
    (3, 200, 3, 1, 16, 16): (1, 1), (128, 128, 1, 1, 256, 256): (6, 6),
    (128, 128, 3, 1, 128, 128): (1, 7), (20, 128, 3, 1, 64, 192): (1, 7),
}


def _key(case):
    return case[:4] + case[5:7]


def fwd_desc(case, slope, ksplit=1, wp3=False, stats=True):
    """The descriptor hipops.conv_fwd builds for `case`, with dummy pointers."""
    Cin, Cout, ks, stride, pad, Hh, Ww, use_tr = case
    P = (ks - 1) // 2
    Ho, Wo = (Hh + 2 * P - ks) // stride + 1, (Ww + 2 * P - ks) // stride + 1
    tr = N.DipTransform(D, D, slope) if use_tr else N.DipTransform(None, None, 1.0)
    d = N.DipConvDesc(D, Hh, Ww, round_up(Cin, 4), round_up(Cin, 4), tr, D, D, D, Ho, Wo, round_up(Cout, 4), Cout, 0, ks, stride,
                      pad if P > 0 else N.PAD_ZERO, P, 1, 0, D if stats else None, ksplit, D if ksplit > 1 else None)
    if wp3:
        d.wp3 = D
    return d


def dgrad_desc(Cin, Cout, ks, Hh, Ww, reflect):
    """The stride-1 data-gradient descriptor of test_bn_backward_statistics_fused_into_the_data_gradient, dummy pointers."""
    P = (ks - 1) // 2
    pad = P if reflect and P else 0
    off = (ks - 1) if pad else (ks - 1 - P)
    Cs = round_up(Cin, 4)
    return N.DipConvDesc(D, Hh, Ww, round_up(Cout, 4), round_up(Cout, 4), N.DipTransform(None, None, 1.0), D, None, D,
                         Hh + 2 * pad, Ww + 2 * pad, Cs, Cin, 0, ks, 1, N.PAD_ZERO, off, 1, 0, None, 1, None)


@pytest.fixture(scope="module")
def lib(built):
    for name in ("dip_conv_dma_eligible", "dip_conv_phase_eligible", "dip_conv1x1_res_eligible"):
        fn = getattr(built, name)
        fn.restype, fn.argtypes = C.c_int, [C.POINTER(N.DipConvDesc)]
    return built


@pytest.mark.parametrize("wp3", [False, True], ids=["fp32", "wp3"])
@pytest.mark.parametrize("code", CODES, ids=CODE_IDS)
@pytest.mark.parametrize("case", TR_CASES, ids=lambda c: "x".join(map(str, c)))
def test_coded_forward_descriptors_reach_a_dip_act_kernel(lib, case, code, wp3):
    for stats in (True, False):
        d = fwd_desc(case, code, wp3=wp3, stats=stats)
        v = lib.dip_conv_variant(C.byref(d))
        assert v in (0, 2, 7, 8), (v, stats)
        assert lib.dip_conv_dma_eligible(C.byref(d)) == 0
        assert lib.dip_conv_phase_eligible(C.byref(d)) == 0
        assert lib.dip_conv1x1_res_eligible(C.byref(d)) == 0


@pytest.mark.parametrize("case", TR_CASES, ids=lambda c: "x".join(map(str, c)))
def test_leaky_forward_descriptors_keep_their_variants(lib, case):
    got = tuple(lib.dip_conv_variant(C.byref(fwd_desc(case, 0.2, wp3=wp3))) for wp3 in (False, True))
    assert got == LEAKY_VARIANTS[_key(case)]


@pytest.mark.parametrize("code", CODES, ids=CODE_IDS)
@pytest.mark.parametrize("Cin,Cout,ks,Hh,Ww,reflect,variant", [
    (128, 128, 3, 24, 40, True, 1), (132, 128, 3, 16, 32, True, 3), (128, 128, 1, 16, 48, True, 1),
    (128, 128, 1, 256, 256, True, 6), (64, 96, 3, 19, 23, False, 1), (128, 8, 1, 16, 16, True, 1),
    (32, 32, 5, 12, 20, True, 0)])
def test_bnb_slope_code_does_not_reroute_the_data_gradient(lib, Cin, Cout, ks, Hh, Ww, reflect, variant, code):
    """bnb_slope is read by the epilogue alone (dip_act_grad, every code): a data-gradient descriptor with a coded
    bnb_slope keeps its kernel and stays fusable."""
    d = dgrad_desc(Cin, Cout, ks, Hh, Ww, reflect)
    assert lib.dip_conv_variant(C.byref(d)) == variant and lib.dip_conv_bnb_fusable(C.byref(d)) == 1
    d.bnb_y, d.bnb_state, d.bnb_partials, d.bnb_partials_thin = D, D, D, D
    d.bnb_Cy = d.bnb_Cs = round_up(Cin, 4)
    d.bnb_pad, d.bnb_slope = ((ks - 1) // 2 if reflect else 0), code
    assert lib.dip_conv_variant(C.byref(d)) == variant and lib.dip_conv_bnb_fusable(C.byref(d)) == 1
