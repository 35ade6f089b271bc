"""dip_group.GroupedFits(downsamplers=) without a GPU: the slab of a super-resolution group (B copies of the closure of
super-resolution.ipynb:169-186 of the reference: out_LR = downsampler(net(x)); mse(out_LR, img_LR)) built on host memory
(_dry_cpu: nothing can be launched), and every error the constructor raises before anything is allocated."""
import pytest
import torch


def _small(seed):
    from models.skip import skip
    torch.manual_seed(seed)
    return skip(8, 3, num_channels_down=[16, 32, 32], num_channels_up=[16, 32, 32], num_channels_skip=[4, 0, 4],
                upsample_mode="bilinear", need_sigmoid=True, need_bias=True, pad="reflection")


def _down(f=4, kernel="lanczos2", planes=3, **kw):
    from models.downsampler import Downsampler
    kw.setdefault("phase", 0.5)
    return Downsampler(n_planes=planes, factor=f, kernel_type=kernel, preserve_size=True, **kw)


HW = (64, 96)
LR = (16, 24)


def _problem(B, lr=LR):
    g = torch.Generator().manual_seed(3)
    zs = [torch.rand(1, 8, *HW, generator=g) * 0.1 for _ in range(B)]
    ts = [torch.rand(1, 3, *lr, generator=g) for _ in range(B)]
    return zs, ts


def _build(B=3, **kw):
    from dip_group import GroupedFits
    zs, ts = _problem(B)
    downs = [_down() for _ in range(B)]
    with torch.no_grad():
        for b, d in enumerate(downs):                # per-instance taps: same support, different values
            d._taps.mul_(1.0 + 0.25 * b)
    nets = [_small(b) for b in range(B)]
    g = GroupedFits(nets, zs, ts, downsamplers=downs, reg_noise_std=0.03, seeds=[5, 6, 7][:B], exp_weight=0.99, device="cpu",
                    _dry_cpu=True, **kw)
    return g, nets, zs, ts, downs


def test_slab_of_a_super_resolution_group(built):
    B = 3
    g, nets, zs, ts, downs = _build(B)
    assert g.stride % 256 == 0 and g.mem.data_ptr() % 256 == 0 and g.mem.numel() == B * g.stride
    assert g.pointers_outside_row0() == []
    ex = g._row0_extra
    # the order of the row's own buffers behind the engine's
    order = [k for k in ("saved", "noisy", "rng", "taps", "target", "out", "y", "partials", "loss", "gl", "m", "v", "iter")]
    offs = [g._off(ex[k]) for k in order]
    assert offs == sorted(offs) and [k for k in ex if ex[k] is not None] == order
    assert ex["mask"] is None
    assert ex["taps"].numel() == 16 * 16 and ex["target"].numel() == 3 * LR[0] * LR[1] == ex["y"].numel()
    assert ex["out"].numel() == 3 * HW[0] * HW[1]
    assert ex["partials"].numel() == g.lib.dip_sr_loss_nblk(3, *LR) == g._head.nblk
    for b in range(B):
        lo = g.mem.data_ptr() + b * g.stride
        for k in ("taps", "target", "y"):
            t = g._inst(ex[k], b)
            assert lo <= t.data_ptr() and t.data_ptr() + 4 * t.numel() <= lo + g.stride, (b, k)
        assert torch.equal(g._inst(ex["taps"], b).view(16, 16), downs[b]._taps)
        assert torch.equal(g._inst(ex["target"], b).view(ts[b].shape), ts[b])
        assert torch.equal(g._inst(ex["saved"], b).view(zs[b].shape), zs[b])
        assert g._inst(ex["rng"], b).tolist() == [0, 5 + b] and g._inst(ex["gl"], b).item() == 1.0
    assert not torch.equal(g._inst(ex["taps"], 0), g._inst(ex["taps"], 1))
    # the descriptor: instance 0's buffers, the geometry of the down-sampler behind the planned output
    d = g._head
    assert (d.out, d.taps, d.target, d.y, d.partials, d.loss) == tuple(ex[k].data_ptr() for k in
                                                                      ("out", "taps", "target", "y", "partials", "loss"))
    assert (d.C, d.H, d.W, d.k, d.f, d.pad, d.Ho, d.Wo, d.sigmoid) == (3, 64, 96, 16, 4, 6, 16, 24, 1)
    # read-outs
    assert g.out.shape == (B, 3, *HW) and g.out.stride() == (g.stride // 4, HW[0] * HW[1], HW[1], 1)
    assert g.out_LR.shape == (B, 3, *LR) and g.out_LR.stride() == (g.stride // 4, LR[0] * LR[1], LR[1], 1)
    assert g.out_LR[2].data_ptr() == g._inst(ex["y"], 2).data_ptr()
    assert g.losses.shape == (B,) and g.out_avg.shape == g.out.shape
    # the launches of the head come from the place SRHead's come from
    assert [n for _, _, n in g._head_fwd + g._head_bwd] == ["head_fwd", "sr_loss_fwd", "sr_loss_bwd"]
    with pytest.raises(RuntimeError, match="dry"):
        g.step()


def test_second_slab_build_reproduces_the_first(built):
    g1 = _build(3)[0]
    g2 = _build(3)[0]
    assert g1.stride == g2.stride
    for k, t in g1._row0_extra.items():
        u = g2._row0_extra[k]
        assert (t is None) == (u is None)
        if t is not None:
            assert g1._off(t) == g2._off(u) and t.numel() == u.numel() and t.dtype == u.dtype, k
    assert torch.equal(g1.mem, g2.mem)              # same nets, same data: the same bytes in every row


def test_no_downsamplers_is_the_layout_of_before(built):
    from dip_group import GroupedFits
    zs, _ = _problem(2)
    ts = [torch.rand(1, 3, *HW) for _ in range(2)]
    g = GroupedFits([_small(0), _small(1)], zs, ts, device="cpu", _dry_cpu=True)
    assert g.downsamplers is None and g.out_LR is None
    assert [k for k, t in g._row0_extra.items() if t is not None] == ["saved", "rng", "target", "out", "partials", "loss", "gl",
                                                                       "m", "v", "iter"]
    assert [n for _, _, n in g._head_fwd + g._head_bwd] == ["loss_head_fwd", "loss_head_bwd"]
    assert g.pointers_outside_row0() == []


def test_validation_errors(built):
    from dip_group import GroupedFits
    from utils.common_utils import get_params
    B = 2
    zs, ts = _problem(B)
    nets = [_small(0), _small(1)]
    mk = lambda downs, targets=ts, **kw: GroupedFits(nets, zs, targets, downsamplers=downs, device="cpu", _dry_cpu=True, **kw)
    with pytest.raises(ValueError, match="one Downsampler per instance"):
        mk([_down()])
    with pytest.raises(TypeError, match="dip-amd:.*Downsampler"):
        mk([_down(), torch.nn.AvgPool2d(4)])
    trainable = _down()
    get_params('down', nets[0], zs[0], downsampler=trainable)
    assert trainable.downsampler_.weight.requires_grad
    with pytest.raises(NotImplementedError, match="dip-amd: GroupedFits covers the fixed-taps Downsampler.*opt_over='down'"):
        mk([_down(), trainable])
    with pytest.raises(NotImplementedError, match="dip-amd:.*fixed-taps"):
        mk([_down(_dense=True), _down()])
    with pytest.raises(ValueError, match=r"\(k, factor, pad\)"):
        mk([_down(4), _down(2)])                                   # k 16 / 8
    with pytest.raises(ValueError, match=r"\(k, factor, pad\)"):
        mk([_down(4), _down(4, "lanczos3")])                       # same factor, k 16 / 24
    with pytest.raises(ValueError, match="planes"):
        mk([_down(planes=1), _down(planes=1)])
    with pytest.raises(ValueError, match="planes"):
        mk([_down(), _down(planes=1)])
    with pytest.raises(ValueError, match="masks and downsamplers"):
        mk([_down(), _down()], masks=[torch.ones(1, 1, *LR)] * 2)
    with pytest.raises(ValueError, match=r"\(15, 24\).*\(16, 24\)"):
        mk([_down(), _down()], targets=[torch.rand(1, 3, 15, 24) for _ in range(B)])
    for n in nets:                                                 # a failed construction leaves no allocator behind
        eng = n.__dict__["_dip_engine"]
        assert eng.slab is None
    g = mk([_down(), _down()])                                     # ... and the same nets still build
    assert g.pointers_outside_row0() == []
