"""Kernel parity for the activation CODES of DipTransform.slope / bnb_slope (-1 Swish, -2 ELU(alpha = 1), -3 ReLU:
models/common.py:62-92 of the reference; csrc/dip_common.h: dip_act, dip_act_grad) on a real MI355X.  The kernel tests of
test_kernels_gpu.py / test_thin_gpu.py / test_small_gpu.py / test_bnone_gpu.py / test_bf3_gpu.py run with slope 0.2 (or 1.0);
a descriptor with a code is routed to other kernels (tests/test_act_routing_host.py) and to other template instantiations
(TR == 2), and every BatchNorm-backward kernel then evaluates another derivative.  The bodies of those tests are reused as
they are (keyword `slope`): same inputs, same fp64 / torch-fp32 references with the activation swapped (t * sigmoid(t),
F.elu, torch.relu), same criterion (error against fp64 <= 2 x the error of torch's fp32 evaluation, same floors), and every
bit-equality assertion between two kernel forms carried over.

ReLU's derivative jumps at 0: wherever a reference differentiates the activation, the inputs are moved off the kink first
(test_kernels_gpu._bn_off_the_kink / _tr_off_the_kink: min |z| >= 1e-3 in fp64, asserted on the CPU; nothing is masked out).
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import dip_native as N  # noqa: E402
from dip_native import round_up  # noqa: E402
import test_act_routing_host as TR  # noqa: E402
import test_bf3_gpu as TB  # noqa: E402
import test_bnone_gpu as T1  # noqa: E402
import test_kernels_gpu as TK  # noqa: E402
import test_small_gpu as TS  # noqa: E402
import test_thin_gpu as TT  # noqa: E402
from test_kernels_gpu import CONV_CASES, REFLECT, ZERO  # noqa: E402

CODES = [-1.0, -2.0, -3.0]
CODE_IDS = ["swish", "elu", "relu"]
codes = pytest.mark.parametrize("code", CODES, ids=CODE_IDS)
_id = lambda c: "x".join(map(str, c))

RES_256 = (128, 128, 1, 1, REFLECT, 256, 256, True)      # with LeakyReLU: the weights-resident kernel; with a code: variant 0


def _variant(case, code, split=False):
    Cin, Cout, ks, stride = case[:4]
    d = TR.fwd_desc(case, code)
    if split:
        d.ksplit = N.conv_plan(d.Hout, d.Wout, round_up(Cin, 4), Cout, ks, stride)[0]
        d.ws = TR.D if d.ksplit > 1 else None
    return N.lib().dip_conv_variant(C.byref(d)), d.ksplit


# ----------------------------------------------------------------------------- forward transform (dip_act)
IGEMM_CASES = [(c, k) for c in CONV_CASES if c[7] and c[5] * c[6] <= 1600 for k in CODES] + [(RES_256, -1.0)]


@pytest.mark.parametrize("case,code", IGEMM_CASES, ids=lambda v: _id(v) if isinstance(v, tuple) else CODE_IDS[CODES.index(v)])
def test_conv_igemm_forward(dev, case, code):
    """conv_igemm_kernel (register-staged, dip_conv_variant == 0), one pass, incl. the zero-padded cases (a padded tap
    contributes 0, not act(b)) and the shapes that take the LDS-DMA / weights-resident kernels with LeakyReLU."""
    assert _variant(case, code)[0] == 0
    TK.test_conv_forward_and_stats(dev, case, False, slope=code)


@codes
@pytest.mark.parametrize("case", [(128, 128, 3, 1, REFLECT, 16, 16, True), (128, 128, 3, 2, REFLECT, 32, 32, True),
                                  (16, 32, 5, 2, REFLECT, 32, 32, True)], ids=_id)
def test_conv_igemm_forward_splitk(dev, case, code):
    v, ksplit = _variant(case, code, split=True)
    assert v == 0 and ksplit > 1
    TK.test_conv_forward_and_stats(dev, case, True, slope=code)


@codes
def test_conv_igemm_forward_extreme_preactivations(dev, code):
    """a[0] = 60: the pre-activations of channel 0 span about +-200, where expf(-t) overflows (Swish: t / (1 + inf) = -0,
    ELU: expm1f(-200) = -1).  Finite, and the same criterion.  The outputs reach |y| ~ 28 here and the tolerance is the floor,
    2e-6 x that; measured err / tol 0.74 (Swish), 0.997 (ELU), 0.41 (ReLU): the 1152 sequential fp32 accumulation steps of
    the matrix pipe at that magnitude (channel 0 leads the K order), not the activation (one ulp of t = 200 times nine weights
    of ~0.03 is 100 x smaller; the same inputs with LeakyReLU(0.2) / no activation measure 0.77 / 0.79)."""
    case = (128, 128, 3, 1, REFLECT, 16, 16, True)
    assert _variant(case, code)[0] == 0
    TK.test_conv_forward_and_stats(dev, case, False, slope=code, a0=60.0)


@codes
@pytest.mark.parametrize("case", [(32, 32, 5, 1, REFLECT, 72, 88, True), (8, 8, 3, 1, ZERO, 75, 70, True),
                                  (16, 48, 3, 2, ZERO, 140, 150, True)], ids=_id)
def test_conv_thin_forward(dev, case, code, monkeypatch):
    """conv_thin_kernel (dip_conv_variant == 8), on every shape as in test_thin_gpu.py (DIP_THIN_ALL is read at every call)."""
    monkeypatch.setenv("DIP_THIN_ALL", "1")
    assert case in TT.THIN_CASES
    assert _variant(case, code, split=True) == (8, 1)
    TK.test_conv_forward_and_stats(dev, case, True, slope=code)


@codes
@pytest.mark.parametrize("case", [(36, 64, 3, 1, ZERO, 21, 13, True), (32, 64, 5, 2, REFLECT, 24, 36, True),
                                  (128, 128, 1, 1, REFLECT, 32, 32, True)], ids=_id)
def test_conv_small_forward(dev, case, code):
    """conv_small's TR == 2 instantiations: zero padding, stride 2 (5x5), 1x1."""
    assert case in TS.SMALL_CASES
    TS.test_conv_small_forward_and_stats(dev, case, slope=code)


@codes
@pytest.mark.parametrize("case", [(128, 128, 3, 1, REFLECT, 16, 16, True), (132, 128, 3, 1, REFLECT, 24, 40, True),
                                  (128, 128, 3, 2, REFLECT, 32, 32, True), (32, 64, 5, 1, REFLECT, 16, 24, True),
                                  (8, 16, 3, 1, ZERO, 16, 16, True), (128, 3, 1, 1, REFLECT, 16, 48, True),
                                  (4, 32, 3, 1, REFLECT, 19, 27, True)], ids=_id)
def test_conv_wgrad(dev, case, code):
    """conv_wgrad_kernel (sliding-window and direct staging, the packed 4-channel tail), thin1x1_wgrad_kernel (Cout <= 8),
    thin_cin_wgrad_kernel (Cin <= 4), at the planned launch shape."""
    assert case in CONV_CASES
    TK.test_conv_wgrad(dev, case, "plan", slope=code)


@codes
@pytest.mark.parametrize("case", [(64, 32, 3, 1, REFLECT, 70, 90, True), (8, 8, 3, 1, ZERO, 75, 70, True)], ids=_id)
def test_wgrad_thin(dev, case, code):
    Cin, Cout, ks, stride, pad, Hh, Ww, _ = case
    assert case in TT.WGRAD_CASES
    assert N.lib().dip_wgrad_thin_shape_ok(Hh, Ww, Cin, Cout, ks, stride) == 1
    TK.test_conv_wgrad(dev, case, "plan", slope=code)


@codes
@pytest.mark.parametrize("case", [(36, 128, REFLECT, 64, 256, True), (36, 128, ZERO, 64, 256, True)], ids=_id)
def test_wgrad_tail(dev, case, code):
    """wgrad_tail_kernel<., 2>: the 4-channel tail behind one 32-channel chunk of a layer at the bf16-pipe floor (512 tiles
    of 2 x 16 pixels), streamed by dip_wgrad_tail_stream; the chunk itself is wgrad_bf3_kernel's TR == 2 form (9 products)."""
    Cin, Cout, pad, Hh, Ww, _ = case
    lib = N.lib()
    n, g, cb = N.wgrad_plan2(Hh, Ww, Cin, Cout, 3, 1)
    d = N.DipWgradDesc(TR.D, Hh, Ww, round_up(Cin, 4), Cin, N.DipTransform(TR.D, TR.D, code), TR.D, Hh, Ww, round_up(Cout, 4),
                       Cout, 3, 1, pad, 1, TR.D, TR.D, n, g, cb)
    assert lib.dip_wgrad_bf3_eligible(C.byref(d)) == 1 and lib.dip_wgrad_tail_stream_ok(C.byref(d)) == 1
    TB.test_wgrad_bf3(dev, case, 9, slope=code)


UPCAT_CASES = [(4, 128, 16, 32, "bilinear"), (0, 32, 8, 8, "nearest"), (128, 128, 8, 16, "nearest"), (4, 16, 12, 20, "bilinear"),
               (0, 8, 4, 6, "bilinear")]


@codes
@pytest.mark.parametrize("ns,nd,Hh,Ww,mode", UPCAT_CASES)
def test_upcat_forward_and_upsample_backward(dev, ns, nd, Hh, Ww, mode, code):
    """upcat_fwd_kernel (dip_act on both branches) and upsample_bwd_stats (dip_act_grad)."""
    TK.test_upcat_forward_backward(dev, ns, nd, Hh, Ww, mode, slope=code)


# ----------------------------------------------------------------------------- backward (dip_act_grad)
@codes
@pytest.mark.parametrize("Cc,Hh,Ww,P", [(128, 16, 32, 1), (4, 19, 23, 0), (132, 12, 20, 1), (16, 8, 8, 2)])
def test_bn_backward_chain(dev, Cc, Hh, Ww, P, code):
    """bn_bwd_stats, bn_bwd_apply, bn_bwd_apply_src (the two forms bit for bit)."""
    TK.test_bn_forward_backward_chain(dev, Cc, Hh, Ww, P, code)


@codes
def test_bn_backward_chain_extreme_preactivations(dev, code):
    """gamma[0] = 60: pre-activations of channel 0 out to about +-150, where expf(-t) overflows (Swish: sg = 1 / (1 + inf) = 0 and
    act' = 0 * (1 - 200) = -0; ELU: expf(-200) = 0).  Finite, and the same criterion."""
    TK.test_bn_forward_backward_chain(dev, 16, 8, 8, 2, code, gamma0=60.0)


@codes
@pytest.mark.parametrize("Cc,Co,Hh,Ww", [(128, 3, 40, 72), (16, 1, 33, 47)])
def test_bn_backward_from_the_thin_output_conv(dev, Cc, Co, Hh, Ww, code):
    """DipGradSrc.tw."""
    TK.test_bn_backward_from_the_thin_output_conv(dev, Cc, Co, Hh, Ww, code)


BNB_CASES = [(128, 128, 3, 24, 40, "reflect"), (132, 128, 3, 16, 32, "reflect"), (128, 128, 1, 16, 48, "reflect"),
             (64, 96, 3, 19, 23, "zero"), (128, 8, 1, 16, 16, "reflect"), (32, 32, 5, 12, 20, "reflect")]
BNB_256 = (128, 128, 1, 256, 256, "reflect")


@pytest.mark.parametrize("case,code", [(c, k) for c in BNB_CASES for k in CODES] + [(BNB_256, -2.0)],
                         ids=lambda v: _id(v) if isinstance(v, tuple) else CODE_IDS[CODES.index(v)])
def test_bn_backward_statistics_fused_into_the_data_gradient(dev, case, code):
    """The bnb epilogues of the LDS-DMA kernel (variant 1), conv_thin4 + LDS-DMA (3), the weights-resident kernel (6), the
    register-staged kernel (0) and the K = 8 data gradient: bnb_slope does not change the routing of a data gradient."""
    TK.test_bn_backward_statistics_fused_into_the_data_gradient(dev, *case[:5], code, case[5])


@codes
@pytest.mark.parametrize("case", [(128, 128, 3, 1, REFLECT, 32, 32), (36, 64, 3, 1, ZERO, 21, 13), (128, 128, 3, 2, REFLECT, 19, 27)],
                         ids=_id)
def test_conv_small_dgrad_with_fused_batchnorm_backward(dev, case, code):
    assert case in TS.DGRAD_CASES
    TS.test_conv_small_dgrad_with_fused_batchnorm_backward(dev, case, slope=code)


@codes
@pytest.mark.parametrize("Cc,Hh,Ww,P", [(128, 7, 11, 2), (128, 128, 128, 1)])
def test_bn_bwd_one(dev, Cc, Hh, Ww, P, code):
    T1.test_bn_bwd_one_matches_autograd(dev, Cc, Hh, Ww, P, code)


@codes
@pytest.mark.parametrize("ns,nd,Hh,Ww,mode,od", [(4, 16, 25, 39, "bilinear", (0, 0)), (4, 128, 128, 128, "bilinear", (0, 0))])
def test_upsample_bwd_one(dev, ns, nd, Hh, Ww, mode, od, code):
    T1.test_upsample_bwd_one_matches_autograd(dev, ns, nd, Hh, Ww, mode, od, slope=code)
