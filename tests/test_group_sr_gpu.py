"""Grouped super-resolution fits on a real MI355X (dip_group.GroupedFits(downsamplers=), the grouped forms of dip_head_fwd,
dip_sr_loss_fwd and dip_sr_loss_bwd): B copies of the closure of super-resolution.ipynb:169-186 of the reference
(out_LR = downsampler(net(x)); mse(out_LR, img_LR)) through ONE launch list.  The bar is the one of tests/test_group_gpu.py:
every instance reaches, bit for bit, what the same fit reaches on its own -- no tolerance anywhere -- in both forms a kernel
family can take (one dispatch for all instances, and the library-side loop of solo dispatches)."""
import copy
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import dip_native as N  # noqa: E402
from test_group_gpu import ALL, _net, native_mask  # noqa: E402,F401

GUARD = 64                     # floats of sentinel between the buffers of a row (keeps every buffer 256-byte aligned)
SENTINEL = -12345.5
MASKS = pytest.mark.parametrize("mask", [ALL, 0], ids=["one-dispatch", "host-loop"])


def _down(planes, f, kernel="lanczos2", dev=None, **kw):
    from models.downsampler import Downsampler
    kw.setdefault("phase", 0.5)
    d = Downsampler(n_planes=planes, factor=f, kernel_type=kernel, preserve_size=True, **kw)
    return d if dev is None else d.to(dev)


# ------------------------------------------------------------------------------------------ 1. the kernels in a group
# (factor, planes, HR size, what the case reaches); lanczos2 with phase 1/2: k = 4 f
KERNEL_CASES = [
    (4, 3, (40, 56)),          # k 16, LR 10 x 14: the compile-time <16, 4> kernels, one ragged tile per plane
    (2, 3, (80, 78)),          # k 8, LR 40 x 39: the generic kernels, 3 x 3 tiles per plane ("blocks")
    (8, 1, (64, 64)),          # k 32, LR 8 x 8: the window exceeds the LDS budget at 16 rows -> the forward walks bands (rp 4)
    (4, 84, (16, 20)),         # k 16, 84 planes: the backward's staged footprint exceeds the LDS budget -> the unstaged kernel
]
KERNEL_IDS = ["k16f4-lr10x14", "k8f2-lr40x39", "k32f8-hr64", "k16f4-84planes-unstaged"]


def _row_layout(sizes):
    """name -> (offset, n) in floats of one row: a guard, then every buffer rounded up to 64 floats and followed by a guard."""
    off, lay = GUARD, {}
    for name, n in sizes:
        lay[name] = (off, n)
        off += (n + 63) // 64 * 64 + GUARD
    return lay, off


def _issue(L, lay, base, geo, sig, with_gs, st):
    """dip_head_fwd, dip_sr_loss_fwd, dip_sr_loss_bwd on the row that starts at `base` (a device address)."""
    Cn, Hh, Ww, k, f, pad, Ho, Wo, Cs, nblk = geo
    p = lambda name: base + 4 * lay[name][0]
    desc = N.DipSRLossDesc(p("out"), p("taps"), p("target"), p("y"), p("partials"), nblk, p("loss"), Cn, Hh, Ww, k, f, pad,
                           Ho, Wo, sig)
    N.check(L.dip_head_fwd(p("src"), p("out"), Cn, Hh * Ww, Cs, sig, st), "head_fwd")
    N.check(L.dip_sr_loss_fwd(C.byref(desc), st), "sr_loss_fwd")
    N.check(L.dip_sr_loss_bwd(C.byref(desc), p("gscale") if with_gs else None, p("dy"), Cs, st), "sr_loss_bwd")


@MASKS
@pytest.mark.parametrize("case", KERNEL_CASES, ids=KERNEL_IDS)
def test_kernels_in_a_group_equal_the_solo_launches(dev, native_mask, case, mask):
    L = native_mask
    B = 3
    f, Cn, (Hh, Ww) = case
    d = _down(Cn, f)
    k, pad = int(d.kernel.shape[0]), int(d._pad)
    assert k == 4 * f
    Ho, Wo = (Hh + 2 * pad - k) // f + 1, (Ww + 2 * pad - k) // f + 1
    Cs = N.round_up(Cn, 4)
    nblk = L.dip_sr_loss_nblk(Cn, Ho, Wo)
    geo = (Cn, Hh, Ww, k, f, pad, Ho, Wo, Cs, nblk)
    lay, nrow = _row_layout([("src", Hh * Ww * Cs), ("out", Cn * Hh * Ww), ("taps", k * k), ("target", Cn * Ho * Wo),
                             ("y", Cn * Ho * Wo), ("partials", nblk), ("loss", 1), ("dy", Hh * Ww * Cs), ("gscale", 1)])
    assert nrow % 64 == 0                                       # stride: a multiple of 256 bytes
    gen = torch.Generator().manual_seed(Hh * 100 + Ww + k)
    init = torch.full((B, nrow), SENTINEL, dtype=torch.float32)
    for b in range(B):                                          # different data in every row, the taps and gscale included
        put = lambda name, t: init[b, lay[name][0]:lay[name][0] + lay[name][1]].copy_(t.reshape(-1))
        put("src", torch.randn(Hh * Ww * Cs, generator=gen))
        put("taps", d._taps * (1.0 + 0.125 * b))
        put("target", torch.rand(Cn * Ho * Wo, generator=gen))
        put("gscale", torch.tensor([1.75 + 0.25 * b]))
    init = init.to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    L.dip_group_native(mask)
    written = ("out", "y", "partials", "loss", "dy")
    for sig in (1, 0):
        for with_gs in (False, True):
            solo, grp = init.clone(), init.clone()
            for b in range(B):
                _issue(L, lay, solo.data_ptr() + 4 * b * nrow, geo, sig, with_gs, st)
            assert L.dip_group_begin(B, 4 * nrow, grp.data_ptr(), 4 * nrow) == 0
            try:
                _issue(L, lay, grp.data_ptr(), geo, sig, with_gs, st)
            finally:
                assert L.dip_group_end() == 0
            torch.cuda.synchronize()
            assert L.dip_group_size() == 1
            what = (sig, with_gs)
            for name in written:
                o, n = lay[name]
                assert bool((solo[:, o:o + n] != SENTINEL).all()), (what, name)          # the solo launches wrote every row
                assert torch.equal(grp[:, o:o + n], solo[:, o:o + n]), (what, name)
            # everything else -- the guards, the inputs, the slack behind every buffer -- is what it was
            keep = torch.ones(nrow, dtype=torch.bool, device=dev)
            for name in written:
                keep[lay[name][0]:lay[name][0] + lay[name][1]] = False
            assert torch.equal(grp[:, keep], init[:, keep]) and torch.equal(solo[:, keep], init[:, keep]), what
            # the rows really are different problems
            o, n = lay["loss"]
            assert len({grp[b, o].item() for b in range(B)}) == B, what
            if Cs > Cn:
                o, n = lay["dy"]
                assert bool((grp[:, o:o + n].view(B, Hh * Ww, Cs)[:, :, Cn:] == 0).all()), what


# ------------------------------------------------------------------------------------------ 2. fits
def _solo_sr_fit(net, z, img_lr, down, std, seed, ema, dev):
    """The fit on its own: utils.reg_noise.RegNoise + utils.loss_head.SRHead + dip_optim.FusedAdam, eager launches."""
    from utils.common_utils import get_params
    from utils.loss_head import SRHead
    from utils.reg_noise import RegNoise
    from dip_optim import FusedAdam
    reg = RegNoise(z, std, seed=seed)
    head = SRHead(net, img_lr, down)
    st = {"avg": None, "out": None, "loss": torch.zeros((), device=dev), "n": 0, "head": head}

    def closure():
        loss, out = head(reg())
        if ema:
            if st["n"] == 0:
                st["avg"] = out.clone()
            else:
                st["avg"].mul_(0.99).add_(out, alpha=1 - 0.99)
        st["n"] += 1
        st["out"] = out
        loss.backward()
        st["loss"].copy_(loss.detach())
        return loss

    opt = FusedAdam(get_params("net", net, z), lr=0.01)
    return opt, closure, st


def _lr_size(net, z, down):
    """The LR size behind the PLANNED output of the net (on a copy: a forward moves the BatchNorm statistics)."""
    with torch.no_grad():
        return tuple(down(copy.deepcopy(net)(z)).shape)


def _run_solo(opt, clo, n):
    for _ in range(n):
        opt.zero_grad()
        clo()
        opt.step()


def _assert_instance(g, b, net, ref, opt, st, n, ema):
    assert opt.device_step_count() == n
    assert g.losses[b].item() == st["loss"].item(), (b, g.losses[b].item(), st["loss"].item())
    for (k, pa), pb in zip(net.named_parameters(), ref.parameters()):
        assert torch.equal(pa, pb), (b, k)
    for (k, ba), bb in zip(net.named_buffers(), ref.buffers()):
        assert torch.equal(ba, bb), (b, k)                      # BatchNorm running statistics, num_batches_tracked
    assert torch.equal(g.out[b:b + 1], st["out"]), b
    assert torch.equal(g.out_LR[b:b + 1], st["head"].out_LR), b
    if ema:
        assert torch.equal(g.out_avg[b:b + 1], st["avg"]), b


FIT_CASES = [
    # kind, HR size, factor, B, reg-noise std, EMA, iterations eager + replayed
    ("skip3", (64, 96), 4, 3, 0.03, True, (3, 4)),
    ("skip3", (36, 52), 2, 2, 0.0, False, (2, 3)),             # 9 x 13 at the deepest scale: Concat's centre crops
    ("wide", (128, 128), 4, 2, 0.0, False, (2, 2)),            # 128-channel layers: implicit GEMM, LDS-DMA, split-K
]
FIT_IDS = ["skip3-64x96-x4", "skip3-36x52-x2", "wide-128-x4"]


@MASKS
@pytest.mark.parametrize("case", FIT_CASES, ids=FIT_IDS)
def test_grouped_sr_fits_bitwise_equal_solo(dev, native_mask, case, mask):
    from dip_group import GroupedFits
    from dip_optim import GraphedIteration
    kind, hw, f, B, std, ema, (n_eager, n_graph) = case
    n = n_eager + n_graph
    cin = {"skip3": 8, "wide": 32}[kind]
    gen = torch.Generator().manual_seed(99)
    zs = [(torch.rand(1, cin, *hw, generator=gen) * 0.1).to(dev) for _ in range(B)]
    nets = [_net(kind, 10 + b).to(dev) for b in range(B)]
    downs = [_down(3, f, dev=dev) for _ in range(B)]
    lr_shape = _lr_size(nets[0], zs[0], downs[0])
    ts = [torch.rand(lr_shape, generator=gen).to(dev) for _ in range(B)]
    refs = [copy.deepcopy(x) for x in nets]
    solo = []
    for b, ref in enumerate(refs):
        opt, clo, st = _solo_sr_fit(ref, zs[b], ts[b], downs[b], std, 40 + b, ema, dev)
        _run_solo(opt, clo, n)
        solo.append((opt, st))
    torch.cuda.synchronize()
    native_mask.dip_group_native(mask)
    g = GroupedFits(nets, zs, ts, downsamplers=downs, reg_noise_std=std, seeds=[40 + b for b in range(B)], lr=0.01,
                    exp_weight=0.99 if ema else None, ema_init="first")
    assert g.pointers_outside_row0() == []
    assert tuple(g.out.shape) == (B, 3, g.eng.Hout, g.eng.Wout) and tuple(g.out_LR.shape) == (B,) + lr_shape[1:]
    g.step(n_eager - 1)
    it = GraphedIteration.group(g, warmup=1)                   # one more eager iteration, then ONE hipGraph
    assert it is g and g.graph is not None
    it.run(n_graph)
    torch.cuda.synchronize()
    assert g.iterations == n and g.step_counts() == [n] * B
    assert native_mask.dip_group_size() == 1
    for b in range(B):
        _assert_instance(g, b, nets[b], refs[b], *solo[b], n, ema)
    losses = [g.losses[b].item() for b in range(B)]
    assert len(set(losses)) == B, losses                       # the instances really are different fits


# ------------------------------------------------------------------------------------------ 3. per-instance taps
def test_instances_may_use_different_taps(dev, native_mask):
    """Two instances with the same net, input, target and noise seed; Gaussian down-samplers of one width and different
    sigma: each equals its own solo fit, and the two differ."""
    from dip_group import GroupedFits
    B, hw, n = 2, (32, 48), 3
    gen = torch.Generator().manual_seed(5)
    z = (torch.rand(1, 8, *hw, generator=gen) * 0.1).to(dev)
    nets = [_net("skip3", 31).to(dev) for _ in range(B)]
    downs = [_down(3, 2, "gauss", dev=dev, phase=0, kernel_width=7, sigma=s) for s in (0.5, 0.8)]
    assert not torch.equal(downs[0]._taps, downs[1]._taps) and downs[0]._taps.shape == downs[1]._taps.shape == (7, 7)
    lr_shape = _lr_size(nets[0], z, downs[0])
    assert lr_shape == (1, 3, 16, 24)
    t = torch.rand(lr_shape, generator=gen).to(dev)
    refs = [copy.deepcopy(x) for x in nets]
    solo = []
    for b, ref in enumerate(refs):
        opt, clo, st = _solo_sr_fit(ref, z, t, downs[b], 0.03, 7, False, dev)
        _run_solo(opt, clo, n)
        solo.append((opt, st))
    native_mask.dip_group_native(ALL)
    g = GroupedFits(nets, [z, z], [t, t], downsamplers=downs, reg_noise_std=0.03, seeds=[7, 7], lr=0.01)
    g.step(n)
    torch.cuda.synchronize()
    for b in range(B):
        _assert_instance(g, b, nets[b], refs[b], *solo[b], n, False)
    assert g.losses[0].item() != g.losses[1].item()
    assert not torch.equal(g.out_LR[0], g.out_LR[1]) and not torch.equal(g.out[0], g.out[1])


# ------------------------------------------------------------------------------------------ 4. errors on the device
def test_errors_on_the_device(dev, native_mask):
    from dip_group import GroupedFits
    from utils.common_utils import get_params
    B, hw = 2, (32, 48)
    gen = torch.Generator().manual_seed(6)
    zs = [(torch.rand(1, 8, *hw, generator=gen) * 0.1).to(dev) for _ in range(B)]
    ts = [torch.rand(1, 3, 8, 12, generator=gen).to(dev) for _ in range(B)]
    nets = [_net("skip3", 50 + b).to(dev) for b in range(B)]
    good = lambda: [_down(3, 4, dev=dev) for _ in range(B)]
    with pytest.raises(ValueError, match=r"\(k, factor, pad\)"):
        GroupedFits(nets, zs, ts, downsamplers=[_down(3, 4, dev=dev), _down(3, 2, dev=dev)])
    with pytest.raises(ValueError, match="masks and downsamplers"):
        GroupedFits(nets, zs, ts, masks=[torch.ones(1, 1, 8, 12, device=dev)] * B, downsamplers=good())
    trained = good()
    get_params('down', nets[1], zs[1], downsampler=trained[1])
    with pytest.raises(NotImplementedError, match="dip-amd:.*opt_over='down'"):
        GroupedFits(nets, zs, ts, downsamplers=trained)
    with pytest.raises(ValueError, match=r"\(8, 11\).*\(8, 12\)"):
        GroupedFits(nets, zs, [x[..., :11].contiguous() for x in ts], downsamplers=good())
    # nothing above left a half-built engine behind: the same nets fit
    g = GroupedFits(nets, zs, ts, downsamplers=good())
    g.step(2)
    torch.cuda.synchronize()
    assert g.step_counts() == [2, 2] and bool(torch.isfinite(g.losses).all())
    assert native_mask.dip_group_size() == 1
