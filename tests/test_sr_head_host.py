"""CPU suite of the fused super-resolution tail (utils.loss_head.SRHead over dip_sr_loss_fwd / dip_sr_loss_bwd): the C ABI grew
by new symbols only, the library validates a descriptor before it launches anything, and the out-of-scope cases raise at
construction, the type refusals before anything needs a GPU."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT


def _small(nout=3):
    from models.skip import skip
    return skip(8, nout, num_channels_down=[16, 16], num_channels_up=[16, 16], num_channels_skip=[4, 4], upsample_mode="bilinear",
                need_sigmoid=True, need_bias=True, pad="reflection")


def _down(planes=3, **kw):
    from models.downsampler import Downsampler
    return Downsampler(n_planes=planes, factor=4, kernel_type='lanczos2', phase=0.5, preserve_size=True, **kw)


def test_header_binding_and_command_list_know_the_entry_points(built):
    import dip_native as N
    hdr = open(os.path.join(ROOT, "include", "dip_hip.h")).read()
    assert re.search(r"^int dip_sr_loss_nblk\(int C, int Ho, int Wo\);", hdr, flags=re.M)
    assert re.search(r"^int dip_sr_loss_fwd\(const DipSRLossDesc\* d, void\* stream\);", hdr, flags=re.M)
    assert re.search(r"^int dip_sr_loss_bwd\(const DipSRLossDesc\* d, const float\* gscale, float\* dy, int Cy, void\* stream\);",
                     hdr, flags=re.M)
    for name in ("dip_sr_loss_nblk", "dip_sr_loss_fwd", "dip_sr_loss_bwd"):
        assert name in N.EXPORTS and hasattr(built, name)
    for name, nargs in (("dip_sr_loss_fwd", 2), ("dip_sr_loss_bwd", 5)):
        fid = built.dip_list_fn_id(name.encode())
        assert fid >= 0, name
        assert built.dip_list_fn_nargs(fid) == nargs == len(N._SIGS[name][1]), name
    assert built.dip_list_fn_id(b"dip_sr_loss_nblk") == -1
    assert built.dip_abi_version() == N.ABI_VERSION           # new symbols and a new struct, no existing struct changed


def test_descriptor_layout_follows_the_header():
    import dip_native as N
    hdr = open(os.path.join(ROOT, "include", "dip_hip.h")).read()
    body = re.search(r"typedef struct DipSRLossDesc \{(.*?)\} DipSRLossDesc;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        is_ptr = "*" in decl
        for nm in decl.replace("*", " ").split(",") if not is_ptr else [decl.replace("*", " ")]:
            fields.append((nm.split()[-1], is_ptr))
    got = [(n, t is ctypes.c_void_p) for n, t in N.DipSRLossDesc._fields_]
    assert got == fields
    assert [n for n, _ in fields] == ["out", "taps", "target", "y", "partials", "nblk", "loss", "C", "H", "W", "k", "f", "pad",
                                      "Ho", "Wo", "sigmoid"]
    # LP64: 5 pointers, nblk + padding, loss, 9 ints + tail padding
    assert ctypes.sizeof(N.DipSRLossDesc) == 96
    assert N.DipSRLossDesc.loss.offset == 48 and N.DipSRLossDesc.C.offset == 56 and N.DipSRLossDesc.sigmoid.offset == 88


def _desc(N, L, **over):
    """A well-formed descriptor (fake addresses: nothing is launched by a refused call) with fields overridden."""
    g = dict(out=0x1000, taps=0x2000, target=0x3000, y=0x4000, partials=0x5000, loss=0x6000,
             C=3, H=64, W=48, k=16, f=4, pad=6, Ho=16, Wo=12, sigmoid=1)
    g.update(over)
    nblk = over.get("nblk", L.dip_sr_loss_nblk(g["C"], g["Ho"], g["Wo"]))
    return N.DipSRLossDesc(g["out"], g["taps"], g["target"], g["y"], g["partials"], nblk, g["loss"], g["C"], g["H"], g["W"],
                           g["k"], g["f"], g["pad"], g["Ho"], g["Wo"], g["sigmoid"])


def test_nblk():
    import dip_native as N
    L = N.lib()
    assert L.dip_sr_loss_nblk(3, 16, 12) == 3 and L.dip_sr_loss_nblk(3, 17, 33) == 3 * 2 * 3
    assert L.dip_sr_loss_nblk(1, 128, 128) == 64
    assert L.dip_sr_loss_nblk(0, 4, 4) == 0 and L.dip_sr_loss_nblk(1, 0, 4) == 0


REFUSALS = [dict(out=None), dict(taps=None), dict(target=None), dict(y=None), dict(partials=None), dict(loss=None),
            dict(C=0), dict(k=0), dict(f=0), dict(Ho=15), dict(Wo=13), dict(Ho=17), dict(H=65, Ho=17), dict(nblk=2),
            dict(nblk=4), dict(H=2, W=2, k=16, pad=6, Ho=1, Wo=1)]


@pytest.mark.parametrize("over", REFUSALS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_library_refuses_before_any_launch(built, over):
    """-1 with dip_last_error set, from both entry points; nothing reaches HIP (this machine may have no GPU at all)."""
    import dip_native as N
    L = built
    d = _desc(N, L, **over)
    for call in (lambda: L.dip_sr_loss_fwd(ctypes.byref(d), None), lambda: L.dip_sr_loss_bwd(ctypes.byref(d), None, 0x7000, 4, None)):
        assert call() == -1
        assert L.dip_last_error().startswith(b"sr_loss")


def test_library_refuses_null_descriptor_and_bad_channel_stride(built):
    import dip_native as N
    L = built
    assert L.dip_sr_loss_fwd(None, None) == -1 and b"NULL descriptor" in L.dip_last_error()
    assert L.dip_sr_loss_bwd(None, None, 0x7000, 4, None) == -1 and b"NULL descriptor" in L.dip_last_error()
    d = _desc(N, L)
    for Cy in (2, 3, 5, 6):                      # Cy < C, Cy % 4 != 0
        assert L.dip_sr_loss_bwd(ctypes.byref(d), None, 0x7000, Cy, None) == -1
        assert b"Cy" in L.dip_last_error()
    assert L.dip_sr_loss_bwd(ctypes.byref(d), None, None, 4, None) == -1


def test_srhead_refusals_type_checks_before_the_device_check():
    from models.resnet import ResNet
    from utils.loss_head import SRHead
    net = _small()
    lr = torch.rand(1, 3, 8, 8)
    # not a net of this backend; a ResNet
    with pytest.raises(RuntimeError, match="dip-amd:.*skip\\(\\)"):
        SRHead(torch.nn.Conv2d(8, 3, 1), lr, _down())
    with pytest.raises(NotImplementedError, match="dip-amd:.*ResNet"):
        SRHead(ResNet(8, 3, 2, 8, act_fun='LeakyReLU'), lr, _down())
    # the down-sampler of a skip() net, a trainable one, a trained (non-diagonal) one
    with pytest.raises(NotImplementedError, match="dip-amd:.*opt_over='down'.*spelled closure"):
        SRHead(net, lr, _down(_dense=True))
    d = _down()
    d.downsampler_.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="dip-amd:.*opt_over='down'.*spelled closure"):
        SRHead(net, lr, d)
    d = _down()
    d.downsampler_.bias.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="dip-amd:.*opt_over='down'.*spelled closure"):
        SRHead(net, lr, d)
    d = _down()
    d._nondiag = True
    with pytest.raises(NotImplementedError, match="dip-amd:.*opt_over='down'.*spelled closure"):
        SRHead(net, lr, d)
    with pytest.raises(TypeError, match="dip-amd:.*Downsampler"):
        SRHead(net, lr, torch.nn.AvgPool2d(4))
    # plane counts: down-sampler vs net, img_LR vs net
    with pytest.raises(ValueError, match="planes"):
        SRHead(net, lr, _down(planes=1))
    with pytest.raises(ValueError, match=r"\[1,3,Ho,Wo\]"):
        SRHead(net, torch.rand(1, 1, 8, 8), _down())
    with pytest.raises(ValueError, match=r"\[1,3,Ho,Wo\]"):
        SRHead(net, torch.rand(3, 8, 8), _down())
    # ... and only then the device
    with pytest.raises(RuntimeError, match="dip-amd:.*MI355X.*no CPU fallback"):
        SRHead(net, lr, _down())
    assert net.__dict__["_dip_engine"].device is None          # nothing above touched the net


def test_both_heads_describe_their_launches_the_same_way():
    from utils.loss_head import MSEHead, SRHead
    for cls in (MSEHead, SRHead):
        for name in ("_descriptor", "fwd_launches", "bwd_launches", "_plan_key", "_plan_keep", "_check_state"):
            assert callable(getattr(cls, name)), (cls.__name__, name)
    assert MSEHead.with_out_conv is False and SRHead.with_out_conv is True


def test_native_iteration_refusals_keep_their_text_and_order():
    """tests/test_native_iter_host.py with the new head type importable: the same precedence, and the head's type is still the
    last thing looked at (a CPU net_input is refused first)."""
    from dip_optim import FusedAdam, NativeIteration
    from utils.common_utils import get_params
    from utils.loss_head import SRHead  # noqa: F401
    z = torch.rand(1, 8, 32, 32) * 0.1
    net = _small()
    opt = FusedAdam(get_params('net', net, z), lr=0.01)
    with pytest.raises(RuntimeError, match="dip-amd:.*skip\\(\\)"):
        NativeIteration(torch.nn.Conv2d(8, 3, 1), None, opt, z)
    with pytest.raises(TypeError, match="dip-amd:.*FusedAdam"):
        NativeIteration(net, None, torch.optim.Adam(net.parameters(), lr=0.01), z)
    with pytest.raises(ValueError, match="dip-amd:.*get_params\\('net'"):
        NativeIteration(net, None, FusedAdam(list(net.parameters())[:-1], lr=0.01), z)
    with pytest.raises(TypeError, match="dip-amd:.*FitMonitor"):
        NativeIteration(net, None, opt, z, monitor=object())
    net.eval()
    with pytest.raises(NotImplementedError, match="dip-amd:.*eval"):
        NativeIteration(net, None, opt, z)
    net.train()
    with pytest.raises(RuntimeError, match="dip-amd:.*CPU"):
        NativeIteration(net, object(), opt, z)
    import inspect
    assert "with_out_conv" in inspect.signature(net.__dict__["_dip_engine"].iteration_lists).parameters
