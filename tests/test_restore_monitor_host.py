"""CPU suite of the restoration monitor (utils.fit_monitor.RestorationFitMonitor / GroupedRestorationFitMonitor,
dip_restore_monitor, dip_restore_monitor_dev, DipRestoreMonitorDesc): the psrn_masked / psrn record and the back-tracking of the
closure of restoration.ipynb:180-219 of the reference.  The entry points are declared, exported, command-list functions and
validate on the host before they launch; every refusal of the solo monitor, of NativeIteration(monitor=) and of
GroupedFits(masks=, monitor=) that needs no GPU; the memory model of a monitored masked group on host memory (the dry mode:
nothing can be launched) -- the monitor's buffers are per-instance data of the slab rows, behind everything a monitor-less
masked group owns, and its descriptor points at the group's own target and mask rows."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

ALIGN = 256
B, HW = 3, (40, 24)


def _small(seed):
    from models.skip import skip
    torch.manual_seed(seed)
    return skip(8, 3, num_channels_down=[16, 32], num_channels_up=[16, 32], num_channels_skip=[4, 4],
                upsample_mode="bilinear", need_sigmoid=True, need_bias=True, pad="reflection")


def _problem(mask_c=1, seed=3):
    g = torch.Generator().manual_seed(seed)
    zs = [torch.rand(1, 8, *HW, generator=g) * 0.1 for _ in range(B)]
    imgs = [torch.rand(1, 3, *HW, generator=g) for _ in range(B)]
    masks = [(torch.rand(1, mask_c, *HW, generator=g) > 0.5).float() for _ in range(B)]
    return zs, imgs, masks


def _dry(monitor=None, mask_c=1, **kw):
    from dip_group import GroupedFits
    zs, imgs, masks = _problem(mask_c)
    return GroupedFits([_small(k) for k in range(B)], zs, imgs, masks=masks, reg_noise_std=0.03, seeds=[5, 6, 7], device="cpu",
                       _dry_cpu=True, monitor=monitor, **kw)


def _up(nbytes):
    return (max(nbytes, 1) + ALIGN - 1) // ALIGN * ALIGN


# ------------------------------------------------------------------------------------------ 1. the C ABI
def test_symbols_header_and_descriptor(built):
    import dip_native as N
    hdr = open(os.path.join(ROOT, "include", "dip_hip.h")).read()
    assert re.search(r"^int dip_restore_monitor_dev\(const DipRestoreMonitorDesc\* d, void\* stream\);", hdr, flags=re.M)
    assert re.search(r"^int dip_restore_monitor\(const float\* out, const float\* img, const float\* mask, int mask_c, "
                     r"int64_t n, int64_t hw,", hdr, flags=re.M)
    head = hdr[:hdr.index("typedef struct DipRestoreMonitorDesc")]
    comment = head[head.rindex("/*"):]
    for line in ("restoration.ipynb:192", "restoration.ipynb:193", "restoration.ipynb:198", "restoration.ipynb:202-208",
                 "restoration.ipynb:209-211"):
        assert line in comment, line
    assert "decide identically" in comment                      # the notebook's psrn_masked_last = 0 against have_last
    size = int(re.search(r"sizeof\(DipRestoreMonitorDesc\) == (\d+)", comment).group(1))
    assert ctypes.sizeof(N.DipRestoreMonitorDesc) == size == 104
    # every field of the header's struct, in order, is a field of the binding's
    body = hdr[hdr.index("typedef struct DipRestoreMonitorDesc {"):hdr.index("} DipRestoreMonitorDesc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            names += [re.split(r"[\s\*]+", first.strip())[-1]] + [r.strip().lstrip("*") for r in rest]
    assert names == [f[0] for f in N.DipRestoreMonitorDesc._fields_]
    # `state` has the layout dip_arena_backtrack reads: the same offsets of counter / state as in DipFitMonitorDesc
    assert N.DipRestoreMonitorDesc.state.offset == N.DipFitMonitorDesc.state.offset == 96
    for name in ("dip_restore_monitor", "dip_restore_monitor_dev"):
        assert name in N.EXPORTS and hasattr(built, name)
    assert built.dip_abi_version() == N.ABI_VERSION == 9          # new entry points, a new struct, no existing one changed
    assert ctypes.sizeof(N.DipFitMonitorDesc) == 104 and ctypes.sizeof(N.DipSRMonitorDesc) == 88
    # the three places that said FitMonitor covers restoration.ipynb:192-211 point at the new entry points
    import dip_optim
    from utils import fit_monitor
    fm = hdr[hdr.index("/* dip_fit_monitor with the iteration index in DEVICE memory"):hdr.index("typedef struct DipFitMonitorDesc")]
    assert "restoration.ipynb:192-211 is dip_restore_monitor" in fm
    assert "restoration.ipynb:192-211 (RestorationFitMonitor)" in fit_monitor.__doc__
    assert "restoration.ipynb:192-211 is RestorationFitMonitor" in dip_optim.NativeIteration.__doc__


def test_command_list_knows_the_launches(built):
    import dip_native as N
    for name, nargs in (("dip_restore_monitor", 13), ("dip_restore_monitor_dev", 2)):
        fid = built.dip_list_fn_id(name.encode())
        assert fid >= 0, name
        assert built.dip_list_fn_nargs(fid) == nargs == len(N._SIGS[name][1]), name


def test_validates_on_the_host_before_any_launch(built):
    import dip_native as N
    L = built
    fake = 1 << 20

    def desc(**kw):
        d = N.DipRestoreMonitorDesc(fake, fake, fake, 3 * 64, 64, 1, 5.0, None, fake, fake, 4, 2, 1, 0, fake, fake)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    assert L.dip_restore_monitor_dev(None, None) == -1
    assert b"restore_monitor_dev" in L.dip_last_error()
    for bad in (dict(n=0), dict(n=-192), dict(hw=0), dict(hw=-64), dict(capacity=0), dict(show_every=0), dict(show_every=-1),
                dict(mask_c=0), dict(mask_c=2), dict(mask_c=4), dict(n=3 * 64 + 1), dict(hw=100),
                dict(out=None), dict(img=None), dict(mask=None), dict(partial=None), dict(records=None), dict(counter=None),
                dict(state=None)):
        d = desc(**bad)
        assert L.dip_restore_monitor_dev(ctypes.byref(d), None) == -1, bad
        assert b"restore_monitor_dev" in L.dip_last_error(), bad
    call = lambda **kw: L.dip_restore_monitor(*[{**dict(out=fake, img=fake, mask=fake, mask_c=3, n=192, hw=64, loss=None,   # noqa: E731
                                                        partial=fake, record=fake, state=fake, check=1, db=5.0, stream=None),
                                                 **kw}[k] for k in ("out", "img", "mask", "mask_c", "n", "hw", "loss", "partial",
                                                                    "record", "state", "check", "db", "stream")])
    for bad in (dict(out=None), dict(img=None), dict(mask=None), dict(partial=None), dict(record=None), dict(state=None),
                dict(n=0), dict(hw=0), dict(mask_c=2), dict(n=193), dict(hw=-64)):
        assert call(**bad) == -1, bad
        assert b"restore_monitor" in L.dip_last_error(), bad
    # through a command list: the failing command is named
    d = desc(capacity=0)
    cl = N.CmdList([("launch", L.dip_restore_monitor_dev, (ctypes.byref(d),), 0, "restore_monitor_dev")])
    with pytest.raises(RuntimeError, match="restore_monitor_dev"):
        cl.run([None])
    assert cl._failed.value == 0


# ------------------------------------------------------------------------------------------ 2. the solo monitor
def test_columns_and_solo_refusals():
    from models.resnet import ResNet
    from utils import fit_monitor as FM
    from utils.fit_monitor import FitMonitor, GroupedFitMonitor, GroupedRestorationFitMonitor, RestorationFitMonitor
    cols = ("loss", "mse_masked", "mse", "psrn_masked", "psrn", "fell_back")
    assert RestorationFitMonitor.COLUMNS == GroupedRestorationFitMonitor.COLUMNS == cols
    assert RestorationFitMonitor.head_kind is None
    # one base under the solo monitors, one under the grouped ones; the builders stand once, at module level
    assert RestorationFitMonitor._sync_counter is FitMonitor._sync_counter and RestorationFitMonitor._advance is FitMonitor._advance
    assert RestorationFitMonitor._ensure_snapshot is FitMonitor._ensure_snapshot
    assert GroupedRestorationFitMonitor.history is GroupedFitMonitor.history
    assert callable(FM.restore_monitor_descriptor) and callable(FM.restore_monitor_launches)
    for name in ("update", "_dev_descriptor", "_plan", "_plan_key", "_plan_keep", "_ensure_snapshot"):
        assert callable(getattr(RestorationFitMonitor, name)), name
    net = _small(0)
    img, mask = torch.rand(1, 3, *HW), torch.ones(1, 1, *HW)
    with pytest.raises(RuntimeError, match="dip-amd:.*RestorationFitMonitor.*MI355X"):
        RestorationFitMonitor(net, img, mask)
    with pytest.raises(RuntimeError, match="dip-amd:.*RestorationFitMonitor.*MI355X"):
        RestorationFitMonitor(net, img, torch.ones(1, 3, *HW), backtracking=False)
    # the mask: [1, 1|C, H, W], as MSEHead checks its own (lower ranks are padded in front)
    for bad in (torch.ones(1, 2, *HW), torch.ones(1, 1, HW[0], HW[1] + 1), torch.ones(2, 1, *HW), torch.ones(1, 1, 1, 1, *HW)):
        with pytest.raises(ValueError, match=r"dip-amd:.*RestorationFitMonitor.*mask must be \[1,1\|3,40,24\]"):
            RestorationFitMonitor(net, img, bad)
    with pytest.raises(RuntimeError, match="MI355X"):          # a [H, W] mask is a [1,1,H,W] mask: only the device is refused
        RestorationFitMonitor(net, img, torch.ones(*HW))
    with pytest.raises(ValueError, match=r"dip-amd:.*RestorationFitMonitor.*img must be \[1,C,H,W\]"):
        RestorationFitMonitor(net, img[0], mask)
    with pytest.raises(TypeError, match="dip-amd:.*RestorationFitMonitor"):
        RestorationFitMonitor(net, img, None)
    for kw in (dict(show_every=0), dict(capacity=0)):
        with pytest.raises(ValueError, match="dip-amd:.*RestorationFitMonitor.*show_every and capacity"):
            RestorationFitMonitor(net, img, mask, **kw)
    # back-tracking needs a skip() net and refuses a ResNet, as FitMonitor does
    with pytest.raises(RuntimeError, match="dip-amd: back-tracking needs a net built by models.skip.skip"):
        RestorationFitMonitor(torch.nn.Sequential(), img, mask)
    with pytest.raises(NotImplementedError, match="dip-amd: RestorationFitMonitor back-tracking covers skip"):
        RestorationFitMonitor(ResNet(1, 3, 1, 8), img, mask)
    with pytest.raises(RuntimeError, match="MI355X"):          # without back-tracking the net is not looked at
        RestorationFitMonitor(ResNet(1, 3, 1, 8), img, mask, backtracking=False)
    # the grouped settings object
    for kw in (dict(show_every=0), dict(capacity=0)):
        with pytest.raises(ValueError, match="dip-amd:.*GroupedRestorationFitMonitor.*show_every and capacity"):
            GroupedRestorationFitMonitor(**kw)
    mon = GroupedRestorationFitMonitor()
    assert (mon.show_every, mon.backtrack_db, mon.backtracking, mon.capacity) == (50, 5.0, True, 16384)
    assert mon.records is mon.state is mon.counter is mon.snapshot is None and mon.i == 0 and mon.group is None
    with pytest.raises(RuntimeError, match="dip-amd:.*GroupedRestorationFitMonitor"):
        mon.history()


# ------------------------------------------------------------------------------------------ 3. NativeIteration(monitor=)
def test_native_iteration_type_checks_are_reached_on_the_cpu():
    from dip_optim import FusedAdam, NativeIteration
    from utils.common_utils import get_params
    from utils.fit_monitor import GroupedRestorationFitMonitor
    z = torch.rand(1, 8, 32, 32) * 0.1
    net = _small(0)
    opt = FusedAdam(get_params('net', net, z), lr=0.01)
    for bad in (object(), GroupedRestorationFitMonitor()):          # the grouped settings object is no solo monitor
        with pytest.raises(TypeError, match="dip-amd:.*RestorationFitMonitor") as e:
            NativeIteration(net, None, opt, z, monitor=bad)
        # ... and the text still says what the earlier tests pin
        for pat in ("dip-amd:.*FitMonitor", "dip-amd:.*SRFitMonitor"):
            assert re.search(pat, str(e.value)), pat
    with pytest.raises(RuntimeError, match="dip-amd:.*CPU"):
        NativeIteration(net, None, opt, z, monitor=None)
    assert opt.step_count == 0 and opt._groups is None


# ------------------------------------------------------------------------------------------ 4. the slab of a monitored group
@pytest.mark.parametrize("backtracking", [True, False], ids=["backtracking", "records-only"])
@pytest.mark.parametrize("mask_c", [1, 3])
def test_monitor_buffers_are_rows_of_the_slab(built, mask_c, backtracking):
    from utils.fit_monitor import GroupedRestorationFitMonitor
    _, imgs, masks = _problem(mask_c)
    cap = 24
    mon = GroupedRestorationFitMonitor(show_every=2, backtrack_db=4.0, backtracking=backtracking, capacity=cap)
    plain = _dry(mask_c=mask_c)
    g = _dry(mon, mask_c=mask_c)
    assert g.pointers_outside_row0() == []
    assert g.monitor is mon and mon.group is g and g.out_avg is None
    # the slab grows by exactly the aligned sum of the monitor's buffers, and nothing in front of them moves
    n = 3 * HW[0] * HW[1]
    n_arena = g.eng.n_arena
    sizes = [4 * 2 * built.dip_fit_monitor_nblk(n), 4 * 6 * cap, 16, 4] + ([4 * n_arena] if backtracking else [])
    assert g.stride - plain.stride == sum(_up(s) for s in sizes)
    assert g.mem.numel() == B * g.stride and g.stride % ALIGN == 0
    assert list(plain._row0_extra) == [k for k in g._row0_extra if not k.startswith("mon_")]
    for k, t in plain._row0_extra.items():
        assert (t is None) == (g._row0_extra[k] is None), k
        if t is not None:
            assert g._off(g._row0_extra[k]) == plain._off(t) and g._row0_extra[k].numel() == t.numel(), k
    for k in ("params", "grads", "packed", "x_nhwc", "dy_out", "bnbuf", "nbt"):
        assert getattr(g.eng, k).data_ptr() - g.mem.data_ptr() == getattr(plain.eng, k).data_ptr() - plain.mem.data_ptr(), k
    mon_keys = [k for k, t in g._row0_extra.items() if k.startswith("mon_") and t is not None]
    assert mon_keys == ["mon_partial", "mon_records", "mon_state", "mon_counter"] + (["mon_snapshot"] if backtracking else [])
    assert "mon_avg" not in g._row0_extra and "mon_gt" not in g._row0_extra          # no EMA, no second copy of an image
    assert min(g._off(g._row0_extra[k]) for k in mon_keys) == plain.stride
    # the views
    s4 = g.stride // 4
    assert mon.records.shape == (B, cap, 6) and mon.records.stride() == (s4, 6, 1) and mon.records.dtype == torch.float32
    assert mon.state.shape == (B, 4) and mon.state.stride() == (s4, 1)
    assert mon.counter.shape == (B,) and mon.counter.dtype == torch.int32 and mon.counter.stride() == (s4,)
    if backtracking:
        assert mon.snapshot.shape == (B, n_arena) and mon.snapshot.stride() == (s4, 1)
    else:
        assert mon.snapshot is None
    lo = g.mem.data_ptr()
    for b in range(B):
        for v in (mon.records[b], mon.state[b], mon.counter[b]) + ((mon.snapshot[b],) if backtracking else ()):
            assert lo + b * g.stride <= v.data_ptr() < lo + (b + 1) * g.stride
        assert torch.count_nonzero(mon.records[b]).item() == 0 and mon.counter[b].item() == 0
        assert mon.state[b].tolist() == [0., 0., 0., 0.]
        assert torch.equal(g._inst(g._row0_extra["target"], b).view(imgs[b].shape), imgs[b])
        assert torch.equal(g._inst(g._row0_extra["mask"], b).view(masks[b].shape), masks[b])
    # the launches of the monitor phase, and ONE descriptor for all instances: the head's output, target, mask and loss
    assert [name for _, _, name in g._mon] == ["restore_monitor_dev"] + (["arena_backtrack"] if backtracking else [])
    assert g._mon[0][0] is g.lib.dip_restore_monitor_dev
    d, ex = g._mdesc, g._row0_extra
    assert isinstance(d, __import__("dip_native").DipRestoreMonitorDesc)
    assert (d.out, d.img, d.mask, d.loss) == tuple(ex[k].data_ptr() for k in ("out", "target", "mask", "loss"))
    assert (d.out, d.img, d.mask, d.loss, d.mask_c) == (g._head.out, g._head.target, g._head.mask, g._head.loss, g._head.mask_c)
    assert (d.partial, d.records, d.counter, d.state) == tuple(ex[k].data_ptr() for k in ("mon_partial", "mon_records",
                                                                                          "mon_counter", "mon_state"))
    assert (d.n, d.hw, d.mask_c, d.capacity, d.show_every, d.backtracking) == (n, HW[0] * HW[1], mask_c, cap, 2, int(backtracking))
    assert d.backtrack_db == 4.0
    if backtracking:
        fn, args, _ = g._mon[1]
        assert fn is g.lib.dip_arena_backtrack
        assert args == (g.eng.params.data_ptr(), ex["mon_snapshot"].data_ptr(), n_arena, d.state)
    # history / last over the views
    mon.records[1, 1] = torch.tensor([.5, .25, .125, 6., 9., 1.])
    mon.i = 2
    h = mon.history()
    assert h.shape == (B, 2, 6) and h.dtype.name == "float32" and h[1, 1].tolist() == [.5, .25, .125, 6., 9., 1.]
    last = mon.last()
    assert len(last) == B and all(tuple(r) == GroupedRestorationFitMonitor.COLUMNS for r in last)
    assert last[1] == dict(loss=.5, mse_masked=.25, mse=.125, psrn_masked=6., psrn=9., fell_back=1.)


def test_monitorless_masked_group_is_unchanged(built):
    g = _dry()
    assert g.monitor is None and not any(k.startswith("mon_") for k in g._row0_extra) and not hasattr(g, "_mdesc")
    assert g.pointers_outside_row0() == []


# ------------------------------------------------------------------------------------------ 5. refusals that need no GPU
def test_group_refusals_need_no_gpu(built):
    from dip_group import GroupedFits
    from models.downsampler import Downsampler
    from utils.fit_monitor import (GroupedFitMonitor, GroupedRestorationFitMonitor, GroupedSRFitMonitor,
                                   RestorationFitMonitor)
    zs, imgs, masks = _problem()
    nets = [_small(k) for k in range(B)]
    kw = dict(device="cpu", _dry_cpu=True)
    G = GroupedRestorationFitMonitor
    # without masks=
    with pytest.raises(ValueError, match="dip-amd:.*GroupedRestorationFitMonitor.*masks"):
        GroupedFits(nets, zs, imgs, monitor=G(), **kw)
    with pytest.raises(ValueError, match="dip-amd:.*GroupedRestorationFitMonitor.*masks"):
        GroupedFits(nets, zs, imgs, masks=[None] * B, monitor=G(), **kw)
    # with downsamplers=
    downs = [Downsampler(n_planes=3, factor=4, kernel_type="lanczos2", phase=0.5, preserve_size=True) for _ in range(B)]
    lrs = [torch.rand(1, 3, HW[0] // 4, HW[1] // 4) for _ in range(B)]
    with pytest.raises(NotImplementedError, match="dip-amd:.*GroupedRestorationFitMonitor.*downsamplers"):
        GroupedFits(nets, zs, lrs, downsamplers=downs, monitor=G(), **kw)
    # this closure has no moving average: the existing refusal
    with pytest.raises(ValueError, match="dip-amd:.*exp_weight"):
        GroupedFits(nets, zs, imgs, masks=masks, monitor=G(), exp_weight=0.99, **kw)
    with pytest.raises(ValueError, match="dip-amd:.*ema_init"):
        GroupedFits(nets, zs, imgs, masks=masks, monitor=G(), ema_init="zeros", **kw)
    # unchanged: what the earlier tests pin
    with pytest.raises(TypeError, match="dip-amd:.*GroupedFitMonitor"):
        GroupedFits(nets, zs, imgs, masks=masks, monitor=object(), **kw)
    with pytest.raises(TypeError, match="dip-amd:.*GroupedFitMonitor"):
        GroupedFits(nets, zs, imgs, masks=masks, monitor=RestorationFitMonitor, **kw)          # a solo monitor class
    with pytest.raises(NotImplementedError, match="dip-amd:.*downsamplers"):
        GroupedFits(nets, zs, lrs, downsamplers=downs, monitor=GroupedFitMonitor(), **kw)
    with pytest.raises(ValueError, match="dip-amd:.*GroupedSRFitMonitor.*downsamplers"):
        GroupedFits(nets, zs, imgs, masks=masks, monitor=GroupedSRFitMonitor(), **kw)
    for n in nets:                                                 # a refused construction leaves no allocator behind
        assert n.__dict__["_dip_engine"].slab is None
    # a refused construction does not adopt; an adopted monitor is adopted once
    mon = G(show_every=2, capacity=5)
    with pytest.raises(ValueError):
        GroupedFits(nets, zs, imgs, masks=masks, monitor=mon, exp_weight=0.5, **kw)
    assert mon.group is None and mon.records is None
    g = GroupedFits(nets, zs, imgs, masks=masks, monitor=mon, **kw)
    with pytest.raises(RuntimeError, match="dip-amd:.*adopted once"):
        GroupedFits([_small(9 + k) for k in range(B)], zs, imgs, masks=masks, monitor=mon, **kw)
    # capacity: refused before anything is issued (here: before the dry group's own refusal to launch)
    with pytest.raises(RuntimeError, match="dip-amd:.*GroupedRestorationFitMonitor capacity"):
        g.step(6)
    with pytest.raises(RuntimeError, match="capacity"):
        g.run(6)
    with pytest.raises(RuntimeError, match="dry"):
        g.step(5)
    assert mon.i == 0 and g.iterations == 0


def test_docs_describe_the_monitor():
    import dip_group
    import dip_optim
    from utils import fit_monitor
    for doc in (dip_optim.NativeIteration.__doc__, fit_monitor.__doc__, dip_group.__doc__):
        assert "RestorationFitMonitor" in doc and "dip_restore_monitor_dev" in doc and "restoration.ipynb:192-211" in doc
    assert "GroupedRestorationFitMonitor" in fit_monitor.__doc__ and "GroupedRestorationFitMonitor" in dip_group.__doc__
    for name in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "RestorationFitMonitor" in open(os.path.join(ROOT, name)).read(), name
