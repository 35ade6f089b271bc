"""CPU suite of dip_optim.NativeIteration (the autograd-free iteration, one dip_iter_run call): the out-of-scope cases raise at
construction, the library knows the new entry points and the header declares them, and dip_iter_run's host-side contract."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT


def _small():
    from models.skip import skip
    return skip(8, 3, num_channels_down=[16, 16], num_channels_up=[16, 16], num_channels_skip=[4, 4], upsample_mode="bilinear",
                need_sigmoid=True, need_bias=True, pad="reflection")


def test_exists_and_documents_the_sequence():
    import dip_optim
    assert hasattr(dip_optim, "NativeIteration")
    doc = dip_optim.NativeIteration.__doc__
    for line in ("opt.zero_grad()", "loss.backward()", "opt.step()", "dip_iter_run"):
        assert line in doc


def test_out_of_scope_cases_raise_at_construction():
    from dip_optim import ArenaLBFGS, FusedAdam, NativeIteration
    from models.resnet import ResNet
    from utils.common_utils import get_params
    z = torch.rand(1, 8, 32, 32) * 0.1
    net = _small()
    opt = FusedAdam(get_params('net', net, z), lr=0.01)
    # a ResNet: no fused loss head on that backbone
    res = ResNet(8, 3, 2, 8, act_fun='LeakyReLU')
    with pytest.raises(NotImplementedError, match="dip-amd:.*ResNet"):
        NativeIteration(res, None, FusedAdam(get_params('net', res, z), lr=0.01), z)
    # not a net of this backend at all
    with pytest.raises(RuntimeError, match="dip-amd:.*skip\\(\\)"):
        NativeIteration(torch.nn.Conv2d(8, 3, 1), None, opt, z)
    # an optimiser that is not FusedAdam
    with pytest.raises(TypeError, match="dip-amd:.*FusedAdam"):
        NativeIteration(net, None, torch.optim.Adam(net.parameters(), lr=0.01), z)
    with pytest.raises(TypeError, match="dip-amd:.*FusedAdam"):
        NativeIteration(net, None, ArenaLBFGS(list(net.parameters()), _allow_cpu=True), z)
    # parameters that include the input, or a Downsampler's
    zin = z.clone()
    with pytest.raises(ValueError, match="dip-amd:.*get_params\\('net'"):
        NativeIteration(net, None, FusedAdam(get_params('net,input', net, zin), lr=0.01), zin)
    from models.downsampler import Downsampler
    down = Downsampler(n_planes=3, factor=2, kernel_type='lanczos2', phase=0.5, preserve_size=True)
    with pytest.raises(ValueError, match="dip-amd:.*get_params\\('net'"):
        NativeIteration(net, None, FusedAdam(get_params('down', net, z, downsampler=down), lr=0.01), z)
    with pytest.raises(ValueError, match="dip-amd:.*get_params\\('net'"):
        NativeIteration(net, None, FusedAdam(list(net.parameters())[:-1], lr=0.01), z)
    # net.eval()
    net.eval()
    with pytest.raises(NotImplementedError, match="dip-amd:.*eval"):
        NativeIteration(net, None, opt, z)
    net.train()
    # a CPU tensor
    with pytest.raises(RuntimeError, match="dip-amd:.*CPU"):
        NativeIteration(net, None, opt, z)
    # nothing above touched the net or the optimiser
    assert opt.step_count == 0 and opt._groups is None
    assert net.__dict__["_dip_engine"].device is None


def test_grouped_fits_are_refused():
    from dip_group import GroupedFits
    from dip_optim import FusedAdam, NativeIteration
    nets = [_small(), _small()]
    zs = [torch.rand(1, 8, 32, 32) * 0.1 for _ in nets]
    ts = [torch.rand(1, 3, 32, 32) for _ in nets]
    g = GroupedFits(nets, zs, ts, device="cpu", _dry_cpu=True)
    with pytest.raises(NotImplementedError, match="dip-amd:.*[Gg]rouped"):
        NativeIteration(g, None, None, zs[0])
    with pytest.raises(NotImplementedError, match="dip-amd:.*[Gg]rouped"):
        NativeIteration(nets[0], g, FusedAdam(list(nets[0].parameters()), lr=0.01), zs[0])


def test_library_and_header_know_the_new_entry_points(built):
    import dip_native as N
    hdr = open(os.path.join(ROOT, "include", "dip_hip.h")).read()
    assert re.search(r"^int dip_iter_run\(const DipPhase\* phases, int nphases,", hdr, flags=re.M)
    assert re.search(r"^int dip_counter_add_n\(uint64_t\* counters, int n, uint64_t inc, void\* stream\);", hdr, flags=re.M)
    # the comment in front of dip_iter_run names the reference lines it replaces
    head = hdr[:hdr.index("int dip_iter_run(")]
    comment = head[head.rindex("/*", 0, head.rindex("typedef struct DipPhase")):]
    assert "utils/common_utils.py:223-230" in comment and "inpainting.ipynb:300-315" in comment
    assert "dip_iter_run" in N.EXPORTS and "dip_counter_add_n" in N.EXPORTS
    assert hasattr(built, "dip_iter_run")
    assert built.dip_abi_version() == N.ABI_VERSION           # new entry points, no existing struct changed
    assert ctypes.sizeof(N.DipPhase) == 24 and ctypes.sizeof(N.DipCmd) == 32
    # the launches of an iteration are command-list entry points; dip_iter_run itself issues lists, it is not one
    for name, nargs in (("dip_counter_add_n", 4), ("dip_loss_head_fwd", 2), ("dip_loss_head_bwd", 5), ("dip_adam_tick", 5),
                        ("dip_adam_step_dev", 10), ("dip_noise_axpy_dev", 7), ("dip_pack_weights", 6), ("dip_nchw_to_nhwc", 6)):
        fid = built.dip_list_fn_id(name.encode())
        assert fid >= 0, name
        assert built.dip_list_fn_nargs(fid) == nargs == len(N._SIGS[name][1]), name
    assert built.dip_list_fn_id(b"dip_iter_run") == -1


def test_iter_run_host_contract(built):
    """dip_iter_run walks its phases in order, stops at the first failing command and says which phase / command it was."""
    import dip_native as N
    L = built
    streams = (ctypes.c_void_p * 1)()
    failed = (ctypes.c_int * 2)(7, 7)
    # no phases: nothing to do
    assert L.dip_iter_run(None, 0, streams, 1, failed) == -1          # (a NULL phase table is refused even when empty)
    empty = (N.DipPhase * 2)(N.DipPhase(None, None, 0, 0), N.DipPhase(None, None, 0, 0))
    assert L.dip_iter_run(empty, 2, streams, 1, failed) == 0 and list(failed) == [-1, -1]
    assert L.dip_iter_run(empty, 2, streams, 0, failed) == -1
    # phase 1 holds a RECORD whose event index is out of range: refused without touching HIP
    bad = (N.DipCmd * 1)(N.DipCmd(N.CMD_RECORD, -1, 0, 3, None, 0, 0))
    ev = (ctypes.c_void_p * 1)()
    phases = (N.DipPhase * 2)(N.DipPhase(None, None, 0, 0),
                              N.DipPhase(ctypes.cast(bad, ctypes.POINTER(N.DipCmd)), ctypes.cast(ev, ctypes.POINTER(ctypes.c_void_p)), 1, 1))
    assert L.dip_iter_run(phases, 2, streams, 1, failed) == -1 and list(failed) == [1, 0]
    assert L.dip_iter_run(phases, 2, streams, 1, None) == -1
    # a phase that claims commands / events without a table
    broken = (N.DipPhase * 1)(N.DipPhase(None, None, 2, 0))
    assert L.dip_iter_run(broken, 1, streams, 1, failed) == -1 and list(failed) == [0, -1]
    assert b"malformed phase" in L.dip_last_error()
    broken = (N.DipPhase * 1)(N.DipPhase(ctypes.cast(bad, ctypes.POINTER(N.DipCmd)), None, 1, 4))
    assert L.dip_iter_run(broken, 1, streams, 1, failed) == -1 and list(failed) == [0, -1]
    # dip_counter_add_n validates before it launches
    assert L.dip_counter_add_n(None, 4, 1, None) == -1 and L.dip_counter_add_n(1 << 20, 0, 1, None) == -1
    if not torch.cuda.is_available():
        # the wrapper names the failing launch: without a GPU the first launch of the second phase fails inside the library
        src = N.DipGradSrc(None, 0, 0, 4, 0)
        args = (ctypes.byref(src), None, 4, 4, 4, 4, None, 4, 0.2, None, 4, None, 1)
        it = N.IterList([N.CmdList([]), N.CmdList([("launch", L.dip_bn_bwd_stats, args, 0, "bnb_stats:probe")])])
        with pytest.raises(RuntimeError, match="phase 1: bnb_stats:probe"):
            it.run([None])
        assert list(it._failed) == [1, 0]
