"""CPU suite of GroupedFits(monitor=): the memory model of a monitored group on host memory (the dry mode: nothing can be
launched) -- the monitor's buffers are per-instance data of the slab rows, behind everything a monitor-less group owns --
the views a utils.fit_monitor.GroupedFitMonitor exposes after adoption, and every refusal that needs no GPU."""
import pytest
import torch

ALIGN = 256


def _small(seed):
    from models.skip import skip
    torch.manual_seed(seed)
    return skip(8, 3, num_channels_down=[16, 32, 32], num_channels_up=[16, 32, 32], num_channels_skip=[4, 0, 4],
                upsample_mode="bilinear", need_sigmoid=True, need_bias=True, pad="reflection")


B, HW = 3, (36, 52)


def _problem(seed=3):
    g = torch.Generator().manual_seed(seed)
    zs = [torch.rand(1, 8, *HW, generator=g) * 0.1 for _ in range(B)]
    ts = [torch.rand(1, 3, *HW, generator=g) for _ in range(B)]
    gts = [torch.rand(1, 3, *HW, generator=g) for _ in range(B)]
    return zs, ts, gts


def _dry(monitor=None, **kw):
    from dip_group import GroupedFits
    zs, ts, _ = _problem()
    return GroupedFits([_small(k) for k in range(B)], zs, ts, reg_noise_std=1 / 30., seeds=[5, 6, 7], device="cpu",
                       _dry_cpu=True, monitor=monitor, **kw)


def _up(nbytes):
    return (max(nbytes, 1) + ALIGN - 1) // ALIGN * ALIGN


@pytest.mark.parametrize("gt", [True, False], ids=["gt", "no-gt"])
@pytest.mark.parametrize("backtracking", [True, False], ids=["backtracking", "records-only"])
def test_monitor_buffers_are_rows_of_the_slab(built, gt, backtracking):
    from utils.fit_monitor import FitMonitor, GroupedFitMonitor
    _, ts, gts = _problem()
    cap = 24
    mon = GroupedFitMonitor(gts if gt else None, exp_weight=0.9, show_every=4, backtracking=backtracking, capacity=cap)
    assert mon.records is None and mon.state is None and mon.counter is None and mon.out_avg is None and mon.snapshot is None
    assert mon.i == 0 and GroupedFitMonitor.COLUMNS == FitMonitor.COLUMNS
    plain = _dry()
    g = _dry(mon)
    assert g.pointers_outside_row0() == []
    assert g.monitor is mon and mon.group is g
    # the slab grows by exactly the aligned sum of the monitor's buffers, and nothing in front of them moves
    n = 3 * HW[0] * HW[1]
    n_arena = g.eng.n_arena
    sizes = ([4 * n] if gt else []) + [4 * n, 4 * 4 * built.dip_fit_monitor_nblk(n), 4 * 8 * cap, 16, 4] + \
        ([4 * n_arena] if backtracking else [])
    assert g.stride - plain.stride == sum(_up(s) for s in sizes)
    assert g.mem.numel() == B * g.stride and g.stride % ALIGN == 0
    for k, t in plain._row0_extra.items():
        if t is not None:
            assert g._off(g._row0_extra[k]) == plain._off(t), k
    assert min(g._off(t) for k, t in g._row0_extra.items() if k.startswith("mon_") and t is not None) == plain.stride
    # the views
    s4 = g.stride // 4
    assert mon.records.shape == (B, cap, 8) and mon.records.stride() == (s4, 8, 1)
    assert mon.state.shape == (B, 4) and mon.state.stride() == (s4, 1)
    assert mon.counter.shape == (B,) and mon.counter.dtype == torch.int32 and mon.counter.stride() == (s4,)
    assert mon.out_avg.shape == (B, 3, *HW) and g.out_avg is mon.out_avg
    if backtracking:
        assert mon.snapshot.shape == (B, n_arena) and mon.snapshot.stride() == (s4, 1)
    else:
        assert mon.snapshot is None and g._row0_extra["mon_snapshot"] is None
    assert [name for _, _, name in g._mon] == ["fit_monitor_dev"] + (["arena_backtrack"] if backtracking else [])
    lo = g.mem.data_ptr()
    for b in range(B):
        for v in (mon.records[b], mon.state[b], mon.counter[b], mon.out_avg[b]) + ((mon.snapshot[b],) if backtracking else ()):
            assert lo + b * g.stride <= v.data_ptr() < lo + (b + 1) * g.stride
        assert torch.count_nonzero(mon.records[b]).item() == 0 and mon.state[b].tolist() == [0.] * 4
        assert mon.counter[b].item() == 0
        if gt:
            assert torch.equal(g._inst(g._row0_extra["mon_gt"], b).view(gts[b].shape), gts[b])
        else:
            assert g._row0_extra["mon_gt"] is None
        assert torch.equal(g._inst(g._row0_extra["target"], b).view(ts[b].shape), ts[b])
    # state is writable through the view, per instance
    mon.state[1] = torch.tensor([1000., 0., 1., 0.])
    assert g._inst(g._row0_extra["mon_state"], 1).tolist() == [1000., 0., 1., 0.]
    assert g._inst(g._row0_extra["mon_state"], 0).tolist() == [0.] * 4
    # the descriptor: one for all instances, loss fixed
    d, ex = g._mdesc, g._row0_extra
    assert (d.out, d.noisy, d.loss) == (ex["out"].data_ptr(), ex["target"].data_ptr(), ex["loss"].data_ptr())
    assert (d.n, d.capacity, d.show_every, d.backtracking) == (n, cap, 4, int(backtracking))
    assert d.exp_weight == pytest.approx(0.9) and (d.gt is not None) == gt
    # history / last over the views
    mon.i = 2
    assert mon.history().shape == (B, 2, 8)
    last = mon.last()
    assert len(last) == B and all(tuple(r) == FitMonitor.COLUMNS for r in last)


def test_monitor_refusals_need_no_gpu(built):
    from dip_group import GroupedFits
    from models.downsampler import Downsampler
    from utils.fit_monitor import FitMonitor, GroupedFitMonitor
    zs, ts, gts = _problem()
    nets = [_small(k) for k in range(B)]
    kw = dict(device="cpu", _dry_cpu=True)
    # not a GroupedFitMonitor
    with pytest.raises(TypeError, match="dip-amd:.*GroupedFitMonitor"):
        GroupedFits(nets, zs, ts, monitor=object(), **kw)
    with pytest.raises(TypeError, match="dip-amd:.*GroupedFitMonitor"):
        GroupedFits(nets, zs, ts, monitor=FitMonitor, **kw)
    # super-resolution groups have another record
    downs = [Downsampler(n_planes=3, factor=4, kernel_type='lanczos2', phase=0.5, preserve_size=True) for _ in range(B)]
    with pytest.raises(NotImplementedError, match="dip-amd:.*downsamplers"):
        GroupedFits(nets, zs, [t[:, :, :9, :13] for t in ts], downsamplers=downs, monitor=GroupedFitMonitor(), **kw)
    # the monitor carries the EMA settings
    with pytest.raises(ValueError, match="dip-amd:.*exp_weight"):
        GroupedFits(nets, zs, ts, exp_weight=0.99, monitor=GroupedFitMonitor(), **kw)
    with pytest.raises(ValueError, match="dip-amd:.*ema_init"):
        GroupedFits(nets, zs, ts, ema_init="zeros", monitor=GroupedFitMonitor(), **kw)
    # imgs_gt: all or none, one per instance, shaped like the targets
    with pytest.raises(ValueError, match="dip-amd:.*imgs_gt"):
        GroupedFitMonitor([gts[0], None, gts[2]])
    with pytest.raises(ValueError, match="dip-amd:.*imgs_gt"):
        GroupedFits(nets, zs, ts, monitor=GroupedFitMonitor(gts[:2]), **kw)
    with pytest.raises(ValueError, match="dip-amd:.*imgs_gt"):
        GroupedFits(nets, zs, ts, monitor=GroupedFitMonitor([gts[0], gts[1][:, :, :-1], gts[2]]), **kw)
    # a refused construction does not adopt; an adopted monitor is adopted once
    mon = GroupedFitMonitor(gts, capacity=5)
    with pytest.raises(ValueError):
        GroupedFits(nets, zs, ts, exp_weight=0.5, monitor=mon, **kw)
    assert mon.group is None and mon.records is None
    g = GroupedFits(nets, zs, ts, monitor=mon, **kw)
    with pytest.raises(RuntimeError, match="dip-amd:.*adopted once"):
        GroupedFits([_small(9 + k) for k in range(B)], zs, ts, monitor=mon, **kw)
    # capacity: refused before anything is issued (here: before the dry group's own refusal to launch)
    with pytest.raises(RuntimeError, match="capacity"):
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


def test_monitorless_group_is_unchanged(built):
    """monitor=None: the same allocation sequence as before the parameter existed -- no monitor key, no descriptor."""
    g = _dry(exp_weight=0.99)
    assert g.monitor is None and not any(k.startswith("mon_") for k in g._row0_extra)
    assert not hasattr(g, "_mdesc") and g.out_avg.shape == (B, 3, *HW)
    assert g.pointers_outside_row0() == []
