"""The fused super-resolution tail on a real MI355X: dip_sr_loss_fwd / dip_sr_loss_bwd against the chain of kernels they
replace (bit for bit) and against an fp64 evaluation; utils.loss_head.SRHead against the notebook's spelling
(super-resolution.ipynb:169-186: out_HR = net(x); out_LR = downsampler(out_HR); mse(out_LR, img_LR)); NativeIteration(SRHead)
against the eager SRHead closure (bit for bit)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import dip_native as N  # noqa: E402
from test_closure_gpu import _same_grads, _small_net, _spec_small  # noqa: E402
from test_closure_kernels_gpu import DOWN_CONFIGS, SIZE_CLASSES, _down_id, _down_module, _down_size  # noqa: E402
from test_kernels_gpu import _check  # noqa: E402
from test_native_iter_gpu import _assert_same_state, _eager_step  # noqa: E402
from test_native_monitor_gpu import _assert_same as _assert_same_with_monitor, _eager_mon_step  # noqa: E402

GUARD = 64                     # floats of sentinel on either side of every written buffer (keeps the 16-byte alignment)
SENTINEL = -12345.5
CLASSES = SIZE_CLASSES + ["blocks"]


def _size(k, f, pad, cls):
    """test_closure_kernels_gpu._down_size, plus "blocks": a 40 x 39 output -- 3 x 3 tiles of 16 x 16 per channel (at least
    three blocks even with one plane), ragged in both directions, and source rows / columns that reach no output pixel."""
    if cls != "blocks":
        return _down_size(k, f, pad, cls)
    base = k - 2 * pad
    return base + f * 39 + 1, base + f * 38 + f - 1


def _guarded(n, dev):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _guard_ok(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


_CASES = {}


def _case(dev, cfg, cls):
    """Inputs of one kernel case and what the two new launches return for sigmoid in (0, 1) x gscale in (None, 1.75), computed
    once and shared by the tests below (nothing modifies it)."""
    key = (cfg[:5], tuple(sorted(cfg[5].items())), cls)
    if key in _CASES:
        return _CASES[key]
    L = N.lib()
    d = _down_module(cfg, dev)
    k, f, pad, Cn = d.kernel.shape[0], cfg[2], d._pad, cfg[4]
    Hh, Ww = _size(k, f, pad, cls)
    Ho, Wo = (Hh + 2 * pad - k) // f + 1, (Ww + 2 * pad - k) // f + 1
    if cls == "blocks":
        assert (Ho, Wo) == (40, 39) and L.dip_sr_loss_nblk(Cn, Ho, Wo) == 9 * Cn
    g = torch.Generator().manual_seed(Hh * 100 + Ww + k)
    z = torch.randn(1, Cn, Hh, Ww, generator=g)                      # what the sigmoid is applied to
    t = torch.rand(1, Cn, Ho, Wo, generator=g)
    taps = d._taps
    assert taps.is_cuda and tuple(taps.shape) == (k, k)
    c = SimpleNamespace(d=d, k=k, f=f, pad=pad, C=Cn, H=Hh, W=Ww, Ho=Ho, Wo=Wo, z=z, t=t, taps=taps, runs={})
    st = torch.cuda.current_stream(dev).cuda_stream
    nblk = L.dip_sr_loss_nblk(Cn, Ho, Wo)
    Cy = 4
    for sig in (0, 1):
        out = (torch.sigmoid(z) if sig else z).to(dev).contiguous()
        td = t.to(dev)
        ybuf, y = _guarded(Cn * Ho * Wo, dev)
        pbuf, partials = _guarded(nblk, dev)
        loss = torch.full((1,), SENTINEL, dtype=torch.float32, device=dev)
        desc = N.DipSRLossDesc(out.data_ptr(), taps.data_ptr(), td.data_ptr(), y.data_ptr(), partials.data_ptr(), nblk,
                               loss.data_ptr(), Cn, Hh, Ww, k, f, pad, Ho, Wo, sig)
        N.check(L.dip_sr_loss_fwd(C.byref(desc), st), "sr_loss_fwd")
        for gs in (None, 1.75):
            gst = None if gs is None else torch.tensor([gs], dtype=torch.float32, device=dev)
            dbuf, dy = _guarded(Hh * Ww * Cy, dev)
            N.check(L.dip_sr_loss_bwd(C.byref(desc), None if gst is None else gst.data_ptr(), dy.data_ptr(), Cy, st),
                    "sr_loss_bwd")
            torch.cuda.synchronize()
            c.runs[(sig, gs)] = SimpleNamespace(out=out, td=td, y=y.view(1, Cn, Ho, Wo), ybuf=ybuf, pbuf=pbuf, partials=partials,
                                                loss=loss, dy=dy.view(Hh * Ww, Cy), dbuf=dbuf)
    _CASES[key] = c
    return c


# ------------------------------------------------------------------------------------------ 1. kernel against the chain
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("cfg", DOWN_CONFIGS, ids=_down_id)
def test_kernels_equal_the_chain_they_replace(dev, cfg, cls):
    """y == dip_lanczos_down_fwd(out); dy == dip_head_bwd(dip_lanczos_down_bwd((y - t) * kk * gs), out): torch.equal.  Pad
    channels of dy are zero and nothing is written outside y, dy and partials."""
    L = N.lib()
    c = _case(dev, cfg, cls)
    st = torch.cuda.current_stream(dev).cuda_stream
    kk = np.float32(2.0) / (np.float32(c.C) * np.float32(c.Ho * c.Wo))
    assert kk.dtype == np.float32
    for (sig, gs), r in c.runs.items():
        y_ref = torch.empty_like(r.y)
        N.check(L.dip_lanczos_down_fwd(r.out.data_ptr(), c.taps.data_ptr(), y_ref.data_ptr(), c.C, c.H, c.W, c.k, c.f, c.pad, st),
                "lanczos_down_fwd")
        assert torch.equal(r.y, y_ref), (sig, gs)
        v = (y_ref - r.td) * float(kk)
        v = (v * gs if gs is not None else v * 1.0).contiguous()
        gx = torch.empty((1, c.C, c.H, c.W), dtype=torch.float32, device=dev)
        N.check(L.dip_lanczos_down_bwd(v.data_ptr(), c.taps.data_ptr(), gx.data_ptr(), c.C, c.H, c.W, c.k, c.f, c.pad, st),
                "lanczos_down_bwd")
        dy_ref = torch.full((c.H * c.W, 4), SENTINEL, dtype=torch.float32, device=dev)
        N.check(L.dip_head_bwd(gx.data_ptr(), r.out.data_ptr(), dy_ref.data_ptr(), c.C, c.H * c.W, 4, sig, st), "head_bwd")
        torch.cuda.synchronize()
        assert torch.equal(r.dy, dy_ref), (sig, gs, (r.dy - dy_ref).abs().max().item())
        assert bool((r.dy[:, c.C:] == 0).all())
        assert _guard_ok(r.ybuf) and _guard_ok(r.dbuf) and _guard_ok(r.pbuf), (sig, gs)
        assert bool(torch.isfinite(r.partials).all()) and float(r.loss) != SENTINEL


# ------------------------------------------------------------------------------------------ 2. kernel against fp64
def _ref(c, sig, gs, dt):
    z = c.z.to(dt).clone().requires_grad_(True)
    out = torch.sigmoid(z) if sig else z
    w = c.d.downsampler_.weight.detach().cpu().to(dt)
    y = F.conv2d(F.pad(out, (c.pad,) * 4, mode="replicate"), w, None, stride=c.f)
    loss = F.mse_loss(y, c.t.to(dt))
    (loss * (1.0 if gs is None else gs)).backward()
    return loss.detach().reshape(1), z.grad.detach()


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("cfg", DOWN_CONFIGS, ids=_down_id)
def test_kernels_against_fp64(dev, cfg, cls):
    """*loss and dy against ReplicationPad2d + the dense strided Conv2d with the taps on the channel diagonal + mse_loss in
    float64 on the CPU, through autograd and the sigmoid; criterion: tests/test_kernels_gpu._check."""
    c = _case(dev, cfg, cls)
    for (sig, gs), r in c.runs.items():
        l64, g64 = _ref(c, sig, gs, torch.float64)
        l32, g32 = _ref(c, sig, gs, torch.float32)
        _check(f"sr_loss.loss[{sig},{gs}]", r.loss, l64, l32)
        dy = r.dy[:, :c.C].t().reshape(1, c.C, c.H, c.W)
        _check(f"sr_loss.dy[{sig},{gs}]", dy, g64, g32)


# ------------------------------------------------------------------------------------------ 3. head against the spelling
def _make_net(kind, seed, nout):
    """"small": test_closure_gpu._small_net (strided convs: the output has the input's size, also at sizes not divisible by 8);
    "pool": tests/test_net_gpu.py's tiny_poolcrop (downsample_mode='avg': the pooling floors, so at such a size the output is
    SMALLER than the input and the head's geometry follows Hout / Wout, not the input)."""
    if kind == "small":
        return _small_net(seed, nout), _spec_small(nout)
    from models.skip import skip
    from test_net_gpu import NETS
    from test_oracle import _spec
    cfg = NETS["tiny_poolcrop"]
    assert cfg["args"][1] == nout
    torch.manual_seed(seed)
    return skip(*cfg["args"], **cfg["kw"]), _spec(cfg)


def _sr_setup(dev, hw, f, nout, seed=3, kernel="lanczos2", phase=0.5, kind="small"):
    from models.downsampler import Downsampler
    net, spec = _make_net(kind, seed, nout)
    net = net.to(dev)
    net.spec = spec
    down = Downsampler(n_planes=nout, factor=f, kernel_type=kernel, phase=phase, preserve_size=True).to(dev)
    g = torch.Generator().manual_seed(seed + 1)
    z = (torch.rand(1, 8, *hw, generator=g) * 0.1).to(dev)
    with torch.no_grad():
        shape = down(net(z)).shape
    lr = torch.rand(shape, generator=g).to(dev)
    return net, down, z, lr


@pytest.mark.parametrize("hw,f,nout,kind", [((64, 96), 4, 3, "small"), ((40, 56), 2, 1, "small"), ((52, 70), 2, 3, "small"),
                                            ((50, 70), 2, 3, "pool")],
                         ids=["64x96-f4", "40x56-f2-1pl", "52x70-f2", "50x70-f2-pool-shrinks"])
def test_head_matches_the_notebook_spelling(dev, hw, f, nout, kind):
    from utils.loss_head import SRHead
    net, down, z, lr = _sr_setup(dev, hw, f, nout, kind=kind)
    out = net(z)          # (52 x 70, not divisible by 8: Concat's centre crops, but strided convs return the input's size)
    if kind == "pool":    # the pooling floors 50 x 70 -> 25 x 35 -> 12 x 17 -> 6 x 8: the output is smaller than the input
        assert out.shape[2] < hw[0] and out.shape[3] < hw[1], tuple(out.shape)
    else:
        assert tuple(out.shape[2:]) == hw
    out_lr = down(out)
    loss = F.mse_loss(out_lr, lr)
    loss.backward()
    ref = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    for p in net.parameters():
        p.grad = None
    head = SRHead(net, lr, down)
    hloss, hout = head(z)
    assert hloss.dim() == 0 and hloss.requires_grad and not hout.requires_grad
    hloss.backward()
    torch.cuda.synchronize()
    got = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    assert torch.equal(hout, out.detach())
    assert tuple(head.out_LR.shape) == tuple(lr.shape) and torch.equal(head.out_LR, out_lr.detach())
    rel = abs(hloss.item() - loss.item()) / abs(loss.item())
    print(f"SRHead loss {hloss.item():.8e}, spelled {loss.item():.8e}, rel {rel:.2e}")
    assert rel <= 1e-5
    _same_grads(got, ref, net.spec)


# ------------------------------------------------------------------------------------------ 4. native against eager
def _sr_fit(dev, seed=3, noisy=False, hw=(64, 96), f=4, nout=3, lr_rate=0.01, kind="small"):
    from dip_optim import FusedAdam
    from utils.common_utils import get_params
    from utils.loss_head import SRHead
    from utils.reg_noise import RegNoise
    net, down, z, lr = _sr_setup(dev, hw, f, nout, seed, kind=kind)
    head = SRHead(net, lr, down)
    reg = RegNoise(z, 0.03, seed=7) if noisy else None
    opt = FusedAdam(get_params('net', net, z), lr=lr_rate)
    return SimpleNamespace(net=net, z=z, target=lr, down=down, head=head, reg=reg, opt=opt, out=None)


def _native(f, monitor=None):
    from dip_optim import NativeIteration
    return NativeIteration(f.net, f.head, f.opt, f.z, reg_noise=f.reg, monitor=monitor)


def _same(a, b, la, lb, out_b, what=""):
    assert torch.equal(torch.stack(la), torch.stack(list(lb))), (what, torch.stack(la).tolist(), torch.stack(list(lb)).tolist())
    _assert_same_state(a, b, a.out, out_b, what)              # parameters, buffers, Adam moments and step, gradients, out
    assert torch.equal(a.head.out_LR, b.head.out_LR), what


@pytest.mark.parametrize("use_run", [False, True], ids=["step", "run"])
@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("noisy", [False, True], ids=["plain", "regnoise"])
def test_native_iteration_is_bit_identical_to_the_eager_closure(dev, noisy, k, use_run):
    a, b = _sr_fit(dev, noisy=noisy), _sr_fit(dev, noisy=noisy)
    it = _native(b)
    la = [_eager_step(a) for _ in range(k)]
    lb = it.run(k) if use_run else [it.step() for _ in range(k)]
    _same(a, b, la, lb, it.out)
    assert it.iterations == k and tuple(it.out.shape) == tuple(a.out.shape)
    names = [n for cl in it._plan["lists"].phases for n in cl.names]
    i0 = names.index("head_fwd")
    assert names[i0:i0 + 4] == ["head_fwd", "sr_loss_fwd", "num_batches_tracked", "sr_loss_bwd"]
    assert "loss_head_fwd" not in names


def test_native_iteration_on_a_net_whose_output_is_smaller_than_its_input(dev):
    kw = dict(noisy=True, hw=(50, 70), f=2, kind="pool")
    a, b = _sr_fit(dev, **kw), _sr_fit(dev, **kw)
    it = _native(b)
    la = [_eager_step(a) for _ in range(3)]
    lb = [it.step()] + list(it.run(2))
    _same(a, b, la, lb, it.out)
    assert it.out.shape[2] < 50 and it.out.shape[3] < 70
    assert tuple(b.head.out_LR.shape[2:]) == (it.out.shape[2] // 2, it.out.shape[3] // 2)


def test_native_and_eager_alternate_on_one_fit(dev):
    a, b = _sr_fit(dev, noisy=True), _sr_fit(dev, noisy=True)
    it = _native(b)
    la = [_eager_step(a) for _ in range(6)]
    lb = [it.step(), it.step(), _eager_step(b), _eager_step(b)] + list(it.run(2))
    _same(a, b, la, lb, it.out)


def test_native_iteration_with_a_monitor(dev):
    from utils.fit_monitor import FitMonitor
    a, b = _sr_fit(dev, noisy=True), _sr_fit(dev, noisy=True)
    g = torch.Generator().manual_seed(5)
    hr_like = torch.rand(1, 3, 64, 96, generator=g).to(dev)
    gt = torch.rand(1, 3, 64, 96, generator=g).to(dev)
    ma, mb = (FitMonitor(f.net, hr_like, gt, exp_weight=0.9, show_every=3, capacity=16) for f in (a, b))
    it = _native(b, mb)
    la = [_eager_mon_step(a, ma) for _ in range(7)]
    lb = [it.step() for _ in range(3)] + list(it.run(4))
    _assert_same_with_monitor(a, b, ma, mb, la, lb, it.out)
    assert torch.equal(a.head.out_LR, b.head.out_LR)


def test_replanning_target_taps_and_input_size(dev):
    a, b = _sr_fit(dev), _sr_fit(dev)
    it = _native(b)
    la, lb = [_eager_step(a)], [it.step()]
    lists0 = it._plan["lists"]
    lb.append(it.step())
    la.append(_eager_step(a))
    assert it._plan["lists"] is lists0
    # another target
    t2 = torch.rand(a.target.shape, generator=torch.Generator().manual_seed(9)).to(dev)
    a.head.target, b.head.target = t2.clone(), t2.clone()
    la.append(_eager_step(a))
    lb.append(it.step())
    lists1 = it._plan["lists"]
    assert lists1 is not lists0
    _same(a, b, la, lb, it.out, "target")
    # the down-sampler's state reloaded: new taps (here: scaled), picked up by both forms
    for f in (a, b):
        sd = {k_: v.clone() for k_, v in f.down.state_dict().items()}
        sd["downsampler_.weight"] = sd["downsampler_.weight"] * 0.5
        f.down.load_state_dict(sd)
        assert not f.down._nondiag
    la.append(_eager_step(a))
    lb.append(it.step())
    assert it._plan["lists"] is not lists1
    _same(a, b, la, lb, it.out, "taps")
    with torch.no_grad():
        assert torch.equal(b.head.out_LR, b.down(it.out))
    # another input size: the engine re-plans; img_LR of the old size is refused, one of the new size accepted
    g = torch.Generator().manual_seed(2)
    z2 = (torch.rand(1, 8, 48, 64, generator=g) * 0.1).to(dev)
    lr2 = torch.rand(1, 3, 12, 16, generator=g).to(dev)
    from dip_optim import NativeIteration
    for f in (a, b):
        f.z = z2
    it2 = NativeIteration(b.net, b.head, b.opt, z2)
    with pytest.raises(ValueError, match="SRHead: img_LR is"):
        it2.step()
    a.head.target, b.head.target = lr2.clone(), lr2.clone()
    la = [_eager_step(a), _eager_step(a)]
    lb = [it2.step(), it2.step()]
    _same(a, b, la, lb, it2.out, "size")
    assert tuple(it2.out.shape) == (1, 3, 48, 64) and tuple(b.head.out_LR.shape) == (1, 3, 12, 16)


# ------------------------------------------------------------------------------------------ 5. refusals on the device
def test_refusals_on_the_device(dev):
    from dip_optim import NativeIteration
    from utils.loss_head import SRHead
    f = _sr_fit(dev)
    from dip_optim import FusedAdam
    from utils.common_utils import get_params
    other = _small_net(5, 3).to(dev)
    with pytest.raises(ValueError, match="dip-amd:.*SRHead was built for another net"):
        NativeIteration(other, f.head, FusedAdam(get_params('net', other, f.z), lr=0.01), f.z)
    with pytest.raises(TypeError, match="dip-amd:.*MSEHead or SRHead, got"):
        NativeIteration(f.net, object(), f.opt, f.z)
    # a wrong LR size
    bad = SRHead(f.net, torch.rand(1, 3, 15, 24, device=dev), f.down)
    with pytest.raises(ValueError, match="SRHead: img_LR is"):
        bad(f.z)
    with pytest.raises(ValueError, match="SRHead: img_LR is"):
        NativeIteration(f.net, bad, f.opt, f.z).step()
    # net.eval()
    f.net.eval()
    with pytest.raises(NotImplementedError, match="dip-amd:.*eval"):
        f.head(f.z)
    with pytest.raises(NotImplementedError, match="dip-amd:.*eval"):
        NativeIteration(f.net, f.head, f.opt, f.z)
    f.net.train()
    it = NativeIteration(f.net, f.head, f.opt, f.z)
    it.step()
    # a down-sampler that became trainable: refused by the next call of either form, and at construction
    f.down.downsampler_.weight.requires_grad_(True)
    for call in (lambda: f.head(f.z), it.step, lambda: SRHead(f.net, f.target, f.down),
                 lambda: NativeIteration(f.net, f.head, f.opt, f.z)):
        with pytest.raises(NotImplementedError, match="dip-amd:.*opt_over='down'"):
            call()
    f.down.downsampler_.weight.requires_grad_(False)
    it.step()
    torch.cuda.synchronize()
    assert it.iterations == 2
