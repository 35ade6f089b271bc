"""CPU suite of the super-resolution monitor (utils.fit_monitor.SRFitMonitor / GroupedSRFitMonitor, dip_sr_monitor,
dip_sr_monitor_dev, DipSRMonitorDesc): the psnr_LR / psnr_HR record of the closure of super-resolution.ipynb:169-191 of the
reference.  The entry points are declared, exported, command-list functions and validate on the host before they launch; the
memory model of a monitored super-resolution group on host memory (the dry mode: nothing can be launched) -- the monitor's
buffers are per-instance data of the slab rows, behind everything a monitor-less group owns; every refusal that needs no GPU."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

ALIGN = 256
B, HW, LR = 3, (32, 48), (8, 12)


def _small(seed):
    from models.skip import skip
    torch.manual_seed(seed)
    return skip(8, 3, num_channels_down=[16, 32, 32], num_channels_up=[16, 32, 32], num_channels_skip=[4, 0, 4],
                upsample_mode="bilinear", need_sigmoid=True, need_bias=True, pad="reflection")


def _down():
    from models.downsampler import Downsampler
    return Downsampler(n_planes=3, factor=4, kernel_type="lanczos2", phase=0.5, preserve_size=True)


def _problem(seed=3):
    g = torch.Generator().manual_seed(seed)
    zs = [torch.rand(1, 8, *HW, generator=g) * 0.1 for _ in range(B)]
    lrs = [torch.rand(1, 3, *LR, generator=g) for _ in range(B)]
    hrs = [torch.rand(1, 3, *HW, generator=g) for _ in range(B)]
    return zs, lrs, hrs


def _dry(monitor=None, sr=True, **kw):
    from dip_group import GroupedFits
    zs, lrs, hrs = _problem()
    return GroupedFits([_small(k) for k in range(B)], zs, lrs if sr else hrs, downsamplers=[_down() for _ in range(B)] if sr else None,
                       reg_noise_std=0.03, seeds=[5, 6, 7], device="cpu", _dry_cpu=True, monitor=monitor, **kw)


def _up(nbytes):
    return (max(nbytes, 1) + ALIGN - 1) // ALIGN * ALIGN


# ------------------------------------------------------------------------------------------ 1. the C ABI
def test_symbols_header_and_descriptor(built):
    import dip_native as N
    hdr = open(os.path.join(ROOT, "include", "dip_hip.h")).read()
    assert re.search(r"^int dip_sr_monitor_dev\(const DipSRMonitorDesc\* d, void\* stream\);", hdr, flags=re.M)
    assert re.search(r"^int dip_sr_monitor\(const float\* out_HR, const float\* out_LR,", hdr, flags=re.M)
    head = hdr[:hdr.index("typedef struct DipSRMonitorDesc")]
    comment = head[head.rindex("/*"):]
    assert "super-resolution.ipynb:169-191" in comment
    size = int(re.search(r"sizeof\(DipSRMonitorDesc\) == (\d+)", comment).group(1))
    assert ctypes.sizeof(N.DipSRMonitorDesc) == size
    # every field of the header's struct, in order, is a field of the binding's
    body = hdr[hdr.index("typedef struct DipSRMonitorDesc {"):hdr.index("} DipSRMonitorDesc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            names += [re.split(r"[\s\*]+", first.strip())[-1]] + [r.strip().lstrip("*") for r in rest]
    assert names == [f[0] for f in N.DipSRMonitorDesc._fields_]
    for name in ("dip_sr_monitor", "dip_sr_monitor_dev"):
        assert name in N.EXPORTS and hasattr(built, name)
    assert built.dip_abi_version() == N.ABI_VERSION == 9          # new entry points, a new struct, no existing one changed
    assert ctypes.sizeof(N.DipFitMonitorDesc) == 104 and ctypes.sizeof(N.DipSRLossDesc) == 96


def test_command_list_knows_the_launches(built):
    import dip_native as N
    for name, nargs in (("dip_sr_monitor", 10), ("dip_sr_monitor_dev", 2)):
        fid = built.dip_list_fn_id(name.encode())
        assert fid >= 0, name
        assert built.dip_list_fn_nargs(fid) == nargs == len(N._SIGS[name][1]), name


def test_validates_on_the_host_before_any_launch(built):
    import dip_native as N
    L = built
    fake = 1 << 20

    def desc(**kw):
        d = N.DipSRMonitorDesc(fake, fake, None, fake, 64, 16, None, fake, fake, 4, 0, fake)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    assert L.dip_sr_monitor_dev(None, None) == -1
    assert b"sr_monitor_dev" in L.dip_last_error()
    for bad in (dict(n_hr=0), dict(n_lr=0), dict(n_lr=-3), dict(capacity=0), dict(out_HR=None), dict(out_LR=None),
                dict(img_LR=None), dict(partial=None), dict(records=None), dict(counter=None)):
        d = desc(**bad)
        assert L.dip_sr_monitor_dev(ctypes.byref(d), None) == -1, bad
        assert b"sr_monitor_dev" in L.dip_last_error(), bad
    assert L.dip_sr_monitor(fake, fake, None, fake, 0, 16, None, fake, fake, None) == -1
    assert L.dip_sr_monitor(fake, fake, None, None, 64, 16, None, fake, fake, None) == -1
    assert L.dip_sr_monitor(fake, fake, None, fake, 64, 16, None, fake, None, None) == -1
    assert b"sr_monitor" in L.dip_last_error()
    # through a command list: the failing command is named
    d = desc(capacity=0)
    cl = N.CmdList([("launch", L.dip_sr_monitor_dev, (ctypes.byref(d),), 0, "sr_monitor_dev")])
    with pytest.raises(RuntimeError, match="sr_monitor_dev"):
        cl.run([None])
    assert cl._failed.value == 0


def test_column_tuples():
    from utils.fit_monitor import FitMonitor, GroupedFitMonitor, GroupedSRFitMonitor, SRFitMonitor
    assert SRFitMonitor.COLUMNS == GroupedSRFitMonitor.COLUMNS == ("loss", "mse_LR", "mse_HR", "psnr_LR", "psnr_HR")
    assert FitMonitor.COLUMNS == GroupedFitMonitor.COLUMNS and len(FitMonitor.COLUMNS) == 8
    # one base under the solo monitors, one under the grouped ones: the counter handling and the read-outs are said once
    assert SRFitMonitor._sync_counter is FitMonitor._sync_counter and SRFitMonitor._advance is FitMonitor._advance
    assert GroupedSRFitMonitor.history is GroupedFitMonitor.history and GroupedSRFitMonitor.last is GroupedFitMonitor.last
    with pytest.raises(RuntimeError, match="dip-amd:.*SRFitMonitor.*MI355X"):
        SRFitMonitor(torch.rand(1, 3, *LR))
    with pytest.raises(ValueError, match="dip-amd:.*imgs_HR"):
        GroupedSRFitMonitor([torch.rand(1, 3, *HW), None])
    with pytest.raises(ValueError, match="dip-amd:.*capacity"):
        GroupedSRFitMonitor(capacity=0)


# ------------------------------------------------------------------------------------------ 2. the slab of a monitored group
@pytest.mark.parametrize("hr", [True, False], ids=["imgs_HR", "no-HR"])
def test_monitor_buffers_are_rows_of_the_slab(built, hr):
    from utils.fit_monitor import GroupedSRFitMonitor
    _, lrs, hrs = _problem()
    cap = 24
    mon = GroupedSRFitMonitor(hrs if hr else None, capacity=cap)
    assert mon.records is None and mon.counter is None and mon.i == 0 and mon.group is None
    with pytest.raises(RuntimeError, match="dip-amd:.*GroupedSRFitMonitor"):
        mon.history()
    plain = _dry()
    g = _dry(mon)
    assert g.pointers_outside_row0() == []
    assert g.monitor is mon and mon.group is g and g.out_avg is None
    # the slab grows by exactly the aligned sum of the monitor's buffers, and nothing in front of them moves
    n_hr, n_lr = 3 * HW[0] * HW[1], 3 * LR[0] * LR[1]
    nblk = built.dip_fit_monitor_nblk(n_hr) + built.dip_fit_monitor_nblk(n_lr)
    sizes = ([4 * n_hr] if hr else []) + [4 * nblk, 4 * 5 * cap, 4]
    assert g.stride - plain.stride == sum(_up(s) for s in sizes)
    assert g.mem.numel() == B * g.stride and g.stride % ALIGN == 0
    for k, t in plain._row0_extra.items():
        assert (t is None) == (g._row0_extra[k] is None), k
        if t is not None:
            assert g._off(g._row0_extra[k]) == plain._off(t), k
    mon_keys = [k for k, t in g._row0_extra.items() if k.startswith("mon_") and t is not None]
    assert mon_keys == (["mon_hr"] if hr else []) + ["mon_partial", "mon_records", "mon_counter"]
    assert min(g._off(g._row0_extra[k]) for k in mon_keys) == plain.stride
    # the views
    s4 = g.stride // 4
    assert mon.records.shape == (B, cap, 5) and mon.records.stride() == (s4, 5, 1) and mon.records.dtype == torch.float32
    assert mon.counter.shape == (B,) and mon.counter.dtype == torch.int32 and mon.counter.stride() == (s4,)
    assert g.out_LR.shape == (B, 3, *LR) and g.out.shape == (B, 3, *HW)
    lo = g.mem.data_ptr()
    for b in range(B):
        for v in (mon.records[b], mon.counter[b]):
            assert lo + b * g.stride <= v.data_ptr() < lo + (b + 1) * g.stride
        assert torch.count_nonzero(mon.records[b]).item() == 0 and mon.counter[b].item() == 0
        if hr:
            assert torch.equal(g._inst(g._row0_extra["mon_hr"], b).view(hrs[b].shape), hrs[b])
        else:
            assert g._row0_extra["mon_hr"] is None
        assert torch.equal(g._inst(g._row0_extra["target"], b).view(lrs[b].shape), lrs[b])
    # the launches of the monitor phase, and ONE descriptor for all instances: the head's two outputs, the LR target, the loss
    assert [name for _, _, name in g._mon] == ["sr_monitor_dev"]
    assert g._mon[0][0] is g.lib.dip_sr_monitor_dev
    d, ex = g._mdesc, g._row0_extra
    assert (d.out_HR, d.out_LR, d.img_LR, d.loss) == tuple(ex[k].data_ptr() for k in ("out", "y", "target", "loss"))
    assert (d.partial, d.records, d.counter) == tuple(ex[k].data_ptr() for k in ("mon_partial", "mon_records", "mon_counter"))
    assert d.img_HR == (ex["mon_hr"].data_ptr() if hr else None)
    assert (d.n_hr, d.n_lr, d.capacity) == (n_hr, n_lr, cap)
    assert (d.out_HR, d.out_LR, d.img_LR, d.loss) == (g._head.out, g._head.y, g._head.target, g._head.loss)
    # history / last over the views
    mon.records[1, 1] = torch.tensor([.5, .25, .125, 6., 9.])
    mon.i = 2
    h = mon.history()
    assert h.shape == (B, 2, 5) and h.dtype.name == "float32" and h[1, 1].tolist() == [.5, .25, .125, 6., 9.]
    last = mon.last()
    assert len(last) == B and all(tuple(r) == GroupedSRFitMonitor.COLUMNS for r in last)
    assert last[1] == dict(loss=.5, mse_LR=.25, mse_HR=.125, psnr_LR=6., psnr_HR=9.) and last[0]["psnr_LR"] == 0.


def test_monitorless_sr_group_is_unchanged(built):
    g = _dry()
    assert g.monitor is None and not any(k.startswith("mon_") for k in g._row0_extra) and not hasattr(g, "_mdesc")
    assert g.pointers_outside_row0() == []


# ------------------------------------------------------------------------------------------ 3. refusals that need no GPU
def test_group_refusals_need_no_gpu(built):
    from dip_group import GroupedFits
    from utils.fit_monitor import GroupedFitMonitor, GroupedSRFitMonitor, SRFitMonitor
    zs, lrs, hrs = _problem()
    nets = [_small(k) for k in range(B)]
    downs = [_down() for _ in range(B)]
    kw = dict(device="cpu", _dry_cpu=True)
    sr = lambda mon, **k: GroupedFits(nets, zs, lrs, downsamplers=downs, monitor=mon, **kw, **k)
    # unchanged: the denoising monitor on a super-resolution group, and something that is no grouped monitor
    with pytest.raises(NotImplementedError, match="dip-amd:.*downsamplers"):
        sr(GroupedFitMonitor())
    with pytest.raises(TypeError, match="dip-amd:.*GroupedFitMonitor"):
        sr(object())
    with pytest.raises(TypeError, match="dip-amd:.*GroupedFitMonitor"):
        sr(SRFitMonitor)
    # new: the super-resolution monitor without a super-resolution group
    with pytest.raises(ValueError, match="dip-amd:.*GroupedSRFitMonitor.*downsamplers"):
        GroupedFits(nets, zs, hrs, monitor=GroupedSRFitMonitor(), **kw)
    # imgs_HR: one per instance, shaped like the net output
    with pytest.raises(ValueError, match="dip-amd:.*imgs_HR"):
        sr(GroupedSRFitMonitor(hrs[:2]))
    with pytest.raises(ValueError, match="dip-amd:.*imgs_HR"):
        sr(GroupedSRFitMonitor([hrs[0], hrs[1][:, :, :-1], hrs[2]]))
    with pytest.raises(ValueError, match="dip-amd:.*imgs_HR"):
        sr(GroupedSRFitMonitor(lrs))                               # the LR size is not the net output's
    # this closure has no moving average
    with pytest.raises(ValueError, match="dip-amd:.*exp_weight"):
        sr(GroupedSRFitMonitor(), exp_weight=0.99)
    with pytest.raises(ValueError, match="dip-amd:.*ema_init"):
        sr(GroupedSRFitMonitor(), ema_init="zeros")
    for n in nets:                                                 # a refused construction leaves no allocator behind
        assert n.__dict__["_dip_engine"].slab is None
    # a refused construction does not adopt; an adopted monitor is adopted once
    mon = GroupedSRFitMonitor(hrs, capacity=5)
    with pytest.raises(ValueError):
        sr(mon, exp_weight=0.5)
    assert mon.group is None and mon.records is None
    g = sr(mon)
    with pytest.raises(RuntimeError, match="dip-amd:.*adopted once"):
        GroupedFits([_small(9 + k) for k in range(B)], zs, lrs, downsamplers=downs, monitor=mon, **kw)
    # capacity: refused before anything is issued (here: before the dry group's own refusal to launch)
    with pytest.raises(RuntimeError, match="dip-amd:.*GroupedSRFitMonitor capacity"):
        g.step(6)
    with pytest.raises(RuntimeError, match="capacity"):
        g.run(6)
    mon.i = 5
    with pytest.raises(RuntimeError, match="capacity"):
        g.step(1)
    mon.i = 0
    with pytest.raises(RuntimeError, match="dry"):
        g.step(5)
    assert mon.i == 0 and g.iterations == 0


def test_native_iteration_type_checks_are_reached_on_the_cpu():
    from dip_optim import FusedAdam, NativeIteration
    from utils.common_utils import get_params
    from utils.fit_monitor import GroupedSRFitMonitor
    z = torch.rand(1, 8, 32, 32) * 0.1
    net = _small(0)
    opt = FusedAdam(get_params('net', net, z), lr=0.01)
    with pytest.raises(TypeError, match="dip-amd:.*FitMonitor"):
        NativeIteration(net, None, opt, z, monitor=object())
    with pytest.raises(TypeError, match="dip-amd:.*SRFitMonitor"):
        NativeIteration(net, None, opt, z, monitor=GroupedSRFitMonitor())          # the grouped settings object is no solo monitor
    with pytest.raises(RuntimeError, match="dip-amd:.*CPU"):
        NativeIteration(net, None, opt, z, monitor=None)
    assert opt.step_count == 0 and opt._groups is None


def test_docs_describe_the_monitor():
    import dip_group
    import dip_optim
    from utils import fit_monitor
    for doc in (dip_optim.NativeIteration.__doc__, fit_monitor.__doc__, dip_group.__doc__):
        assert "SRFitMonitor" in doc and "dip_sr_monitor_dev" in doc
    assert "GroupedSRFitMonitor" in fit_monitor.__doc__ and "GroupedSRFitMonitor" in dip_group.__doc__
    for name in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "SRFitMonitor" in open(os.path.join(ROOT, name)).read(), name
