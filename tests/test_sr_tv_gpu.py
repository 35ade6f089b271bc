"""The TV term of the fused super-resolution tail on a real MI355X (total_loss = mse(out_LR, img_LR) + tv_weight *
tv_loss(out_HR); super-resolution.ipynb:180-181, sr_prior_effect.ipynb:109 of the reference): dip_sr_tv_loss_fwd / _bwd against
an fp64 evaluation of the spelled closure, the NaN pattern of the reference at s == 0, utils.loss_head.SRHead(tv_weight=) against
the notebook's spelling, NativeIteration against the eager closure (bit for bit), set_tv_weight without a re-plan, and
GroupedFits(tv_weights=) against the solo fits (bit for bit)."""
import copy
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import dip_native as N  # noqa: E402
from test_closure_gpu import _same_grads  # noqa: E402
from test_closure_kernels_gpu import DOWN_CONFIGS, _down_id, _down_module  # noqa: E402
from test_group_gpu import ALL, _net, native_mask  # noqa: E402,F401
from test_group_sr_gpu import _down, _lr_size  # noqa: E402
from test_kernels_gpu import _check  # noqa: E402
from test_native_iter_gpu import _assert_same_state, _eager_step  # noqa: E402
from test_sr_head_gpu import CLASSES, GUARD, SENTINEL, _guard_ok, _guarded, _size, _sr_setup  # noqa: E402,F401
from test_sr_monitor_gpu import _assert_group_equals_solo, _assert_same_records, _eager_mon_step  # noqa: E402

BETAS = (0.5, 1.0, 2.0, 0.75)


def _tv_loss(x, beta):
    from utils.sr_utils import tv_loss
    return tv_loss(x, beta)


# ------------------------------------------------------------------------------------------ 1. kernels against fp64
def _ref(c, sig, gs, dt, w_mse=1.0, w_tv=None, target=None):
    """w_mse * mse(down(out), t) + w_tv * tv_loss(out, beta) through autograd on the CPU, out = sigmoid(z) or z:
    ReplicationPad2d + the dense strided Conv2d with the taps on the channel diagonal, as test_sr_head_gpu._ref."""
    z = c.z.to(dt).clone().requires_grad_(True)
    out = torch.sigmoid(z) if sig else z
    loss = torch.zeros((), dtype=dt)
    if w_mse:
        wgt = c.d.downsampler_.weight.detach().cpu().to(dt)
        y = F.conv2d(F.pad(out, (c.pad,) * 4, mode="replicate"), wgt, None, stride=c.f)
        loss = loss + w_mse * F.mse_loss(y, (c.t if target is None else target).to(dt))
    w_tv = c.w[sig] if w_tv is None else w_tv
    if w_tv:
        loss = loss + w_tv * _tv_loss(out, c.beta)
    (loss * (1.0 if gs is None else gs)).backward()
    return loss.detach().reshape(1), z.grad.detach()


def _tv_desc(L, c, out, td, y, partials, tvp, tvw, loss, sig):
    sr = N.DipSRLossDesc(out.data_ptr(), c.taps.data_ptr(), td.data_ptr(), y.data_ptr(), partials.data_ptr(), c.nblk,
                         loss.data_ptr(), c.C, c.H, c.W, c.k, c.f, c.pad, c.Ho, c.Wo, sig)
    return N.DipSRTVDesc(sr, tvw.data_ptr(), tvp.data_ptr(), c.tv_nblk, c.beta)


_CASES = {}


def _case(dev, cfg, hw, beta=0.5):
    """Inputs of one kernel case and what the two launches return for sigmoid in (0, 1) x gscale in (None, 1.75), computed once
    and shared by the tests below (nothing modifies it).  hw: a size class of test_sr_head_gpu or an HR size (H, W).
    tv_weight per sigmoid setting, from the fp64 reference: max|TV gradient| == max|MSE gradient|."""
    key = (cfg[:5], tuple(sorted(cfg[5].items())), hw, beta)
    if key in _CASES:
        return _CASES[key]
    L = N.lib()
    d = _down_module(cfg, dev)
    k, f, pad, Cn = d.kernel.shape[0], cfg[2], d._pad, cfg[4]
    Hh, Ww = _size(k, f, pad, hw) if isinstance(hw, str) else hw
    Ho, Wo = (Hh + 2 * pad - k) // f + 1, (Ww + 2 * pad - k) // f + 1
    g = torch.Generator().manual_seed(Hh * 100 + Ww + k)
    z = torch.randn(1, Cn, Hh, Ww, generator=g)                      # what the sigmoid is applied to
    t = torch.rand(1, Cn, Ho, Wo, generator=g)
    Cy = 4 if Cn <= 4 else N.round_up(Cn, 4)
    c = SimpleNamespace(d=d, k=k, f=f, pad=pad, C=Cn, H=Hh, W=Ww, Ho=Ho, Wo=Wo, z=z, t=t, taps=d._taps, beta=beta, Cy=Cy,
                        nblk=L.dip_sr_loss_nblk(Cn, Ho, Wo), tv_nblk=L.dip_sr_tv_nblk(Cn, Hh, Ww), runs={}, w={}, share={})
    assert c.tv_nblk == Cn * ((Hh + 15) // 16) * ((Ww + 63) // 64)
    st = torch.cuda.current_stream(dev).cuda_stream
    for sig in (0, 1):
        _, g_mse = _ref(c, sig, None, torch.float64, 1.0, 0.0)
        _, g_tv = _ref(c, sig, None, torch.float64, 0.0, 1.0)
        m_mse, m_tv = g_mse.abs().max().item(), g_tv.abs().max().item()
        assert np.isfinite(m_tv) and m_mse > 0
        if m_tv == 0:
            assert Hh == 1 or Ww == 1                                # no term at all: the TV sum is 0, nothing is read
            c.w[sig], c.share[sig] = 1.0, 0.0
        else:
            c.w[sig] = float(np.float32(m_mse / m_tv))               # (as the device scalar holds it)
            c.share[sig] = c.w[sig] * m_tv / m_mse
        out = (torch.sigmoid(z) if sig else z).to(dev).contiguous()
        td = t.to(dev)
        tvw = torch.tensor([c.w[sig]], dtype=torch.float32, device=dev)
        ybuf, y = _guarded(Cn * Ho * Wo, dev)
        pbuf, partials = _guarded(c.nblk, dev)
        tbuf, tvp = _guarded(c.tv_nblk, dev)
        loss = torch.full((1,), SENTINEL, dtype=torch.float32, device=dev)
        desc = _tv_desc(L, c, out, td, y, partials, tvp, tvw, loss, sig)
        N.check(L.dip_sr_tv_loss_fwd(C.byref(desc), st), "sr_tv_loss_fwd")
        for gs in (None, 1.75):
            gst = None if gs is None else torch.tensor([gs], dtype=torch.float32, device=dev)
            dbuf, dy = _guarded(Hh * Ww * Cy, dev)
            N.check(L.dip_sr_tv_loss_bwd(C.byref(desc), None if gst is None else gst.data_ptr(), dy.data_ptr(), Cy, st),
                    "sr_tv_loss_bwd")
            torch.cuda.synchronize()
            c.runs[(sig, gs)] = SimpleNamespace(out=out, td=td, y=y.view(1, Cn, Ho, Wo), ybuf=ybuf, pbuf=pbuf, tbuf=tbuf, tvp=tvp,
                                                partials=partials, loss=loss, dy=dy.view(Hh * Ww, Cy), dbuf=dbuf, desc=desc,
                                                tvw=tvw, gst=gst)
    _CASES[key] = c
    return c


def _check_case(dev, c, what):
    L = N.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    for (sig, gs), r in c.runs.items():
        tag = f"{what}[{c.H}x{c.W},beta {c.beta},{sig},{gs}]"
        # the TV share of the gradient this case checks (0 only where the image has no term)
        assert c.share[sig] == 0.0 or abs(c.share[sig] - 1.0) <= 1e-6, (tag, c.share)
        l64, g64 = _ref(c, sig, gs, torch.float64)
        l32, g32 = _ref(c, sig, gs, torch.float32)
        dy = r.dy[:, :c.C].t().reshape(1, c.C, c.H, c.W)
        e_l = abs(r.loss.item() - l64.item())
        e_g = (dy.detach().cpu().double() - g64).abs().max().item()
        print(f"{tag}: loss err {e_l:.3e} (torch-fp32 {abs(l32.item() - l64.item()):.3e}), dy err {e_g:.3e} "
              f"(torch-fp32 {(g32.double() - g64).abs().max().item():.3e}), tv_weight {c.w[sig]:.3e}")
        _check(f"sr_tv_loss.loss{tag}", r.loss, l64, l32)
        _check(f"sr_tv_loss.dy{tag}", dy, g64, g32)
        # y is the down-sampler's own output, bit for bit; pad channels; guards
        y_ref = torch.empty_like(r.y)
        N.check(L.dip_lanczos_down_fwd(r.out.data_ptr(), c.taps.data_ptr(), y_ref.data_ptr(), c.C, c.H, c.W, c.k, c.f, c.pad, st),
                "lanczos_down_fwd")
        torch.cuda.synchronize()
        assert torch.equal(r.y, y_ref), tag
        assert bool((r.dy[:, c.C:] == 0).all()), tag
        assert _guard_ok(r.ybuf) and _guard_ok(r.dbuf) and _guard_ok(r.pbuf) and _guard_ok(r.tbuf), tag
        assert bool(torch.isfinite(r.partials).all()) and bool(torch.isfinite(r.tvp).all()) and float(r.loss) != SENTINEL
    # two runs are the same bits
    for (sig, gs), r in c.runs.items():
        loss0, dy0, y0 = r.loss.clone(), r.dy.clone(), r.y.clone()
        N.check(L.dip_sr_tv_loss_fwd(C.byref(r.desc), st), "sr_tv_loss_fwd")
        N.check(L.dip_sr_tv_loss_bwd(C.byref(r.desc), None if r.gst is None else r.gst.data_ptr(), r.dy.data_ptr(), c.Cy, st),
                "sr_tv_loss_bwd")
        torch.cuda.synchronize()
        assert torch.equal(r.loss, loss0) and torch.equal(r.dy, dy0) and torch.equal(r.y, y0), (what, sig, gs)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("cfg", DOWN_CONFIGS, ids=_down_id)
def test_kernels_against_fp64(dev, cfg, cls):
    """*loss and dy against mse_loss(ReplicationPad2d + strided Conv2d) + tv_weight * utils.sr_utils.tv_loss in float64 on the
    CPU, through autograd and the sigmoid; criterion: tests/test_kernels_gpu._check.  The size classes of test_sr_head_gpu."""
    _check_case(dev, _case(dev, cfg, cls), cls)


# HR sizes: both multiples of 16 (one / two tiles of the forward pass wide); both 1 modulo 16 (the one-pixel remainder tiles of the
# backward receive left and above contributions only; 65 = one column behind a forward tile); H != W everywhere
HR_SIZES = [(32, 64), (48, 80), (33, 65), (17, 81)]
_L2 = [c for c in DOWN_CONFIGS if c[0] == "lanczos2" and c[1] == 0.5 and c[3] and c[2] in (2, 4)]
# 16 planes: the largest staged form at k 16 / f 4 (47.2 KB); 17: a and b push it past the 48 KB budget (the plain tail still
# stages); 84: the plain tail does not stage either
_PLANES = [("lanczos2", 0.5, 4, True, p, {}) for p in (16, 17, 84)]


@pytest.mark.parametrize("hw", HR_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("cfg", _L2, ids=_down_id)
def test_kernels_against_fp64_tile_sizes(dev, cfg, hw):
    _check_case(dev, _case(dev, cfg, hw), "tiles")


@pytest.mark.parametrize("cfg", _PLANES, ids=_down_id)
def test_kernels_against_fp64_staged_and_unstaged(dev, cfg):
    _check_case(dev, _case(dev, cfg, (17, 33)), "planes")


@pytest.mark.parametrize("beta", BETAS)
def test_kernels_against_fp64_betas(dev, beta):
    """The three exact forms (sqrt, identity, square) and powf, staged (3 planes) and unstaged (17 planes)."""
    _check_case(dev, _case(dev, _L2[0], (33, 65), beta), "beta")
    _check_case(dev, _case(dev, _PLANES[1], (17, 33), beta), "beta-unstaged")


# ------------------------------------------------------------------------------------------ 2. TV alone
@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("cfg,hw", [(_L2[0], (33, 65)), (_L2[1], (48, 80)), (_PLANES[1], (17, 33))], ids=["a", "b", "unstaged"])
def test_tv_alone(dev, cfg, hw, beta):
    """target = y of a first forward: the MSE residual is exactly zero, *loss and dy are the TV term and its gradient."""
    L = N.lib()
    c = _case(dev, cfg, hw, beta)
    st = torch.cuda.current_stream(dev).cuda_stream
    for (sig, gs), r in c.runs.items():
        td = r.y.clone()
        ybuf, y = _guarded(c.C * c.Ho * c.Wo, dev)
        pbuf, partials = _guarded(c.nblk, dev)
        tbuf, tvp = _guarded(c.tv_nblk, dev)
        dbuf, dy = _guarded(c.H * c.W * c.Cy, dev)
        loss = torch.full((1,), SENTINEL, dtype=torch.float32, device=dev)
        desc = _tv_desc(L, c, r.out, td, y, partials, tvp, r.tvw, loss, sig)
        N.check(L.dip_sr_tv_loss_fwd(C.byref(desc), st), "sr_tv_loss_fwd")
        N.check(L.dip_sr_tv_loss_bwd(C.byref(desc), None if r.gst is None else r.gst.data_ptr(), dy.data_ptr(), c.Cy, st),
                "sr_tv_loss_bwd")
        torch.cuda.synchronize()
        assert torch.equal(y, td.reshape(-1)) and bool((partials == 0).all())
        l64, g64 = _ref(c, sig, gs, torch.float64, 0.0)
        l32, g32 = _ref(c, sig, gs, torch.float32, 0.0)
        assert l64.item() > 0 and g64.abs().max().item() > 0
        _check(f"tv_alone.loss[{sig},{gs}]", loss, l64, l32)
        _check(f"tv_alone.dy[{sig},{gs}]", dy.view(c.H * c.W, c.Cy)[:, :c.C].t().reshape(1, c.C, c.H, c.W), g64, g32)
        assert _guard_ok(ybuf) and _guard_ok(dbuf) and _guard_ok(pbuf) and _guard_ok(tbuf)


# ------------------------------------------------------------------------------------------ 3. s == 0
@pytest.mark.parametrize("beta", [0.5, 1.0, 2.0])
def test_constant_patch_gives_the_nans_of_the_reference(dev, beta):
    """No epsilon, as in the reference: a constant 4 x 4 patch has nine terms with s == 0; for beta 0.5 the NaN pattern of dy is
    the one autograd leaves over the spelled tv_loss on the same device; beta 1 and 2 stay finite.  *loss is finite in all."""
    L = N.lib()
    cfg = _L2[0]
    d = _down_module(cfg, dev)
    k, f, pad, Cn = d.kernel.shape[0], cfg[2], d._pad, cfg[4]
    Hh, Ww = 20, 36
    Ho, Wo = (Hh + 2 * pad - k) // f + 1, (Ww + 2 * pad - k) // f + 1
    g = torch.Generator().manual_seed(4)
    out = torch.rand(1, Cn, Hh, Ww, generator=g)
    out[:, :, 3:7, 14:18] = 0.25                                     # (across the backward's tile border at x = 16)
    out = out.to(dev)
    td = torch.rand(1, Cn, Ho, Wo, generator=g).to(dev)
    w = 0.125
    c = SimpleNamespace(taps=d._taps, nblk=L.dip_sr_loss_nblk(Cn, Ho, Wo), tv_nblk=L.dip_sr_tv_nblk(Cn, Hh, Ww), C=Cn, H=Hh, W=Ww,
                        k=k, f=f, pad=pad, Ho=Ho, Wo=Wo, beta=beta)
    st = torch.cuda.current_stream(dev).cuda_stream
    tvw = torch.tensor([w], dtype=torch.float32, device=dev)
    y = torch.empty(Cn * Ho * Wo, device=dev)
    partials, tvp = torch.empty(c.nblk, device=dev), torch.empty(c.tv_nblk, device=dev)
    loss = torch.full((1,), SENTINEL, dtype=torch.float32, device=dev)
    dy = torch.full((Hh * Ww, 4), SENTINEL, dtype=torch.float32, device=dev)
    desc = _tv_desc(L, c, out, td, y, partials, tvp, tvw, loss, 0)
    N.check(L.dip_sr_tv_loss_fwd(C.byref(desc), st), "sr_tv_loss_fwd")
    N.check(L.dip_sr_tv_loss_bwd(C.byref(desc), None, dy.data_ptr(), 4, st), "sr_tv_loss_bwd")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all()) and loss.item() != SENTINEL
    got = dy[:, :Cn].t().reshape(1, Cn, Hh, Ww)
    x = out.clone().requires_grad_(True)
    (w * _tv_loss(x, beta)).backward()
    want = torch.isnan(x.grad)
    assert torch.equal(torch.isnan(got), want), (beta, int(torch.isnan(got).sum()), int(want.sum()))
    if beta < 1:
        assert int(want.sum()) >= 9 * Cn
        assert bool(torch.isfinite(got[~want]).all())
    else:
        assert not bool(want.any()) and bool(torch.isfinite(got).all())
    assert bool((dy[:, Cn:] == 0).all())


# ------------------------------------------------------------------------------------------ 4. head against the spelling
def _grads(net):
    g = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    for p in net.parameters():
        p.grad = None
    return g


def _spelled(net, down, z, lr, w, beta, tv64):
    """The notebook's closure; tv64: the TV term as tv_loss(out_HR.double()).float() (the yardstick's second evaluation)."""
    out = net(z)
    out_lr = down(out)
    mse = F.mse_loss(out_lr, lr)
    tv = _tv_loss(out.double(), beta).float() if tv64 else _tv_loss(out, beta)
    loss = mse + (w if w is not None else 0.0) * tv
    return out, out_lr, mse, tv, loss


@pytest.mark.parametrize("hw,f,nout,kind", [((64, 96), 4, 3, "small"), ((40, 56), 2, 1, "small"), ((52, 70), 2, 3, "small"),
                                            ((50, 70), 2, 3, "pool")],
                         ids=["64x96-f4", "40x56-f2-1pl", "52x70-f2", "50x70-f2-pool-shrinks"])
def test_head_matches_the_notebook_spelling(dev, hw, f, nout, kind):
    """SRHead(tv_weight=w) against loss = mse(down(net(z)), lr) + w * tv_loss(net(z)) through autograd, w such that the two terms
    are equal; gradients by test_closure_gpu._same_grads as it is (2e-5 relative per tensor + 1e-7 x the largest gradient norm).
    That criterion was set for two HIP evaluations of one gradient; here dy differs from autograd's in rounding, so the test
    also prints, per case, the worst relative L2 distance of a tensor beside the yardstick -- the spelled closure evaluated
    twice, as written and with the TV term as tv_loss(out.double()).float().  Measured on an MI355X (worst tensor; fused against
    spelled / spelled against spelled-with-TV-in-double): 64x96-f4 5.0e-3 / 2.5e-3, 40x56-f2-1pl 4.6e-3 / 5.8e-3, 52x70-f2
    4.8e-3 / 1.9e-3, 50x70-f2-pool 3.3e-3 / 2.2e-3 -- always a deep-scale BatchNorm weight (1.1.7...0.2.weight) whose gradient
    is a sum of O(gmax) terms and sits under _same_grads' floor: _same_grads holds in all four cases without the yardstick;
    loss: relative <= 8.1e-8."""
    from utils.loss_head import SRHead
    import parity as PT
    net, down, z, lr = _sr_setup(dev, hw, f, nout, kind=kind)
    beta = 0.5
    out, out_lr, mse, tv, _ = _spelled(net, down, z, lr, None, beta, False)
    w = float(mse.detach() / tv.detach())
    (mse + w * tv).backward()
    loss = (mse + w * tv).detach()
    share = w * tv.item() / mse.item()
    assert 0.25 <= share <= 4.0, share
    ref = _grads(net)
    # the yardstick: the same closure with the TV term evaluated in double
    _, _, _, _, loss2 = _spelled(net, down, z, lr, w, beta, True)
    loss2.backward()
    ref2 = _grads(net)
    head = SRHead(net, lr, down, tv_weight=w, tv_beta=beta)
    hloss, hout = head(z)
    assert hloss.dim() == 0 and hloss.requires_grad and not hout.requires_grad
    hloss.backward()
    torch.cuda.synchronize()
    got = _grads(net)
    assert torch.equal(hout, out.detach())
    assert tuple(head.out_LR.shape) == tuple(lr.shape) and torch.equal(head.out_LR, out_lr.detach())
    rel = abs(hloss.item() - loss.item()) / abs(loss.item())
    print(f"SRHead(tv) loss {hloss.item():.8e}, spelled {loss.item():.8e}, rel {rel:.2e}, TV / MSE {share:.3f}")
    assert rel <= 1e-5
    zero = PT.zero_grad_keys(net.spec)
    worst = (0.0, 0.0, None)
    for k in ref:
        if k not in zero:
            n = ref[k].double().norm().item()
            e, y = (got[k].double() - ref[k].double()).norm().item(), (ref2[k].double() - ref[k].double()).norm().item()
            if e / n > worst[0]:
                worst = (e / n, y / n, k)
    print(f"worst tensor {worst[2]}: fused-vs-spelled {worst[0]:.3e}, spelled-vs-spelled(tv in double) {worst[1]:.3e} (relative L2)")
    _same_grads(got, ref, net.spec)


# ------------------------------------------------------------------------------------------ 5. native against eager
def _tv_weight_for(net, down, z, lr, beta=0.5, ratio=1.0):
    """The weight at which the TV term is `ratio` x the MSE term at the start of the fit (on a copy: a forward moves the
    BatchNorm statistics)."""
    with torch.no_grad():
        out = copy.deepcopy(net)(z)
        return ratio * float(F.mse_loss(down(out), lr) / _tv_loss(out, beta))


def _tv_fit(dev, seed=3, noisy=False, hw=(64, 96), f=4, nout=3, ratio=1.0, beta=0.5):
    from dip_optim import FusedAdam
    from utils.common_utils import get_params
    from utils.loss_head import SRHead
    from utils.reg_noise import RegNoise
    net, down, z, lr = _sr_setup(dev, hw, f, nout, seed)
    w = _tv_weight_for(net, down, z, lr, beta, ratio)
    head = SRHead(net, lr, down, tv_weight=w, tv_beta=beta)
    reg = RegNoise(z, 0.03, seed=7) if noisy else None
    opt = FusedAdam(get_params('net', net, z), lr=0.01)
    return SimpleNamespace(net=net, z=z, target=lr, down=down, head=head, reg=reg, opt=opt, out=None, w=w)


def _native(f, monitor=None):
    from dip_optim import NativeIteration
    return NativeIteration(f.net, f.head, f.opt, f.z, reg_noise=f.reg, monitor=monitor)


def _same(a, b, la, lb, out_b, what=""):
    assert torch.equal(torch.stack(la), torch.stack(list(lb))), (what, torch.stack(la).tolist(), torch.stack(list(lb)).tolist())
    _assert_same_state(a, b, a.out, out_b, what)
    assert torch.equal(a.head.out_LR, b.head.out_LR), what


@pytest.mark.parametrize("use_run", [False, True], ids=["step", "run"])
@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("noisy", [False, True], ids=["plain", "regnoise"])
def test_native_iteration_is_bit_identical_to_the_eager_closure(dev, noisy, k, use_run):
    a, b = _tv_fit(dev, noisy=noisy), _tv_fit(dev, noisy=noisy)
    assert a.w == b.w > 0
    it = _native(b)
    la = [_eager_step(a) for _ in range(k)]
    lb = it.run(k) if use_run else [it.step() for _ in range(k)]
    _same(a, b, la, lb, it.out)
    names = [n for cl in it._plan["lists"].phases for n in cl.names]
    i0 = names.index("head_fwd")
    assert names[i0:i0 + 4] == ["head_fwd", "sr_tv_loss_fwd", "num_batches_tracked", "sr_tv_loss_bwd"]
    assert "sr_loss_fwd" not in names and "sr_loss_bwd" not in names
    # the TV term is in the loss: the same fit without it reports another one
    c = _tv_fit(dev, noisy=noisy)
    c.head.set_tv_weight(c.w * 2)
    assert _eager_step(c).item() > la[0].item()


def test_native_and_eager_alternate_on_one_fit(dev):
    a, b = _tv_fit(dev, noisy=True), _tv_fit(dev, noisy=True)
    it = _native(b)
    la = [_eager_step(a) for _ in range(6)]
    lb = [it.step(), it.step(), _eager_step(b), _eager_step(b)] + list(it.run(2))
    _same(a, b, la, lb, it.out)


def test_native_iteration_with_a_monitor(dev):
    """The records of an SRFitMonitor: `loss` is the total loss, mse_LR the MSE alone."""
    from utils.fit_monitor import SRFitMonitor
    a, b = _tv_fit(dev, noisy=True), _tv_fit(dev, noisy=True)
    g = torch.Generator().manual_seed(11)
    img_hr = torch.rand(1, 3, 64, 96, generator=g).to(dev)
    ma, mb = SRFitMonitor(a.target, img_hr, capacity=8), SRFitMonitor(b.target, img_hr, capacity=8)
    it = _native(b, mb)
    la = [_eager_mon_step(a, ma) for _ in range(6)]
    lb = [it.step() for _ in range(2)] + list(it.run(4).unbind(0))
    assert torch.equal(torch.stack(la), torch.stack(lb))
    _assert_same_records(ma, mb, 6)
    _assert_same_state(a, b, a.out, it.out)
    h = mb.history()
    assert np.array_equal(h[:, 0], torch.stack(lb).cpu().numpy())
    mse_last = F.mse_loss(b.head.out_LR, b.target).item()
    tv_last = b.w * _tv_loss(it.out, 0.5).item()
    assert h[-1, 1] == pytest.approx(mse_last, rel=1e-5) and tv_last > 0.01 * mse_last
    assert h[-1, 0] - h[-1, 1] == pytest.approx(tv_last, rel=1e-3)                  # loss = MSE + the TV term
    assert (h[:, 0] > h[:, 1]).all()


# ------------------------------------------------------------------------------------------ 6. set_tv_weight
def test_set_tv_weight_keeps_the_plan(dev):
    from dip_optim import NativeIteration
    from utils.loss_head import SRHead
    a, b = _tv_fit(dev, noisy=True), _tv_fit(dev, noisy=True)
    ita, itb = _native(a), _native(b)
    la, lb = list(ita.run(2).unbind(0)), list(itb.run(2).unbind(0))
    lists = ita._plan["lists"]
    key = a.head._plan_key()
    w2 = a.w * 3.0
    a.head.set_tv_weight(w2)
    assert a.head._plan_key() == key and a.head.tv_weight == w2
    la += list(ita.run(2).unbind(0))
    assert ita._plan["lists"] is lists
    # the twin: a head constructed with the new weight, from the same state
    b.head = SRHead(b.net, b.target, b.down, tv_weight=w2)
    itb2 = NativeIteration(b.net, b.head, b.opt, b.z, reg_noise=b.reg)
    lb += list(itb2.run(2).unbind(0))
    la.append(_eager_step(a))                         # ... and the eager form reads the same scalar
    lb.append(_eager_step(b))
    _same(a, b, la, lb, b.out)
    assert la[2].item() != la[1].item()
    for bad in (0.0, 0):
        with pytest.raises(ValueError, match="dip-amd:.*set_tv_weight.*new SRHead"):
            a.head.set_tv_weight(bad)
    plain = SRHead(a.net, a.target, a.down)
    with pytest.raises(ValueError, match="dip-amd:.*set_tv_weight.*new SRHead"):
        plain.set_tv_weight(w2)
    assert a.head.tv_weight == w2 and ita._plan["lists"] is lists


# ------------------------------------------------------------------------------------------ 7. grouped
def _solo_tv(net, z, img_lr, img_hr, down, w, std, seed, capacity):
    from dip_optim import FusedAdam, NativeIteration
    from utils.common_utils import get_params
    from utils.fit_monitor import SRFitMonitor
    from utils.loss_head import SRHead
    from utils.reg_noise import RegNoise
    mon = SRFitMonitor(img_lr, img_hr, capacity=capacity)
    it = NativeIteration(net, SRHead(net, img_lr, down, tv_weight=w), FusedAdam(get_params("net", net, z), lr=0.01), z,
                         reg_noise=RegNoise(z, std, seed=seed), monitor=mon)
    return it, mon


def _assert_adam_and_loss(g, solos, refs):
    ex = g._row0_extra
    for b, (it, smon) in enumerate(solos):
        eng = refs[b].__dict__["_dip_engine"]
        gm, gv = g._inst(ex["m"], b), g._inst(ex["v"], b)
        assert len(it.opt._groups) >= 1
        for gr in it.opt._groups:
            o = (gr.base - eng.params.data_ptr()) // 4
            assert torch.equal(gm[o:o + gr.numel], gr.m.reshape(-1)) and torch.equal(gv[o:o + gr.numel], gr.v.reshape(-1)), b
        assert g.losses[b].item() == smon.history()[-1, 0], b


@pytest.mark.parametrize("mask", [ALL, 0], ids=["one-dispatch", "host-loop"])
def test_grouped_tv_fits_bitwise_equal_solo(dev, native_mask, mask):
    """B = 3 fits of one image with three TV weights (a weight sweep) and two tap sets, eager and as ONE hipGraph: parameters,
    Adam state, losses, out, out_LR and the monitor's records of every instance equal its solo NativeIteration fit."""
    from dip_group import GroupedFits
    from utils.fit_monitor import GroupedSRFitMonitor
    B, std, cap, hw = 3, 0.03, 8, (64, 96)
    gen = torch.Generator().manual_seed(21)
    zs = [(torch.rand(1, 8, *hw, generator=gen) * 0.1).to(dev) for _ in range(B)]
    nets = [_net("skip3", 60 + b).to(dev) for b in range(B)]
    downs = [_down(3, 2, "gauss", dev=dev, phase=0, kernel_width=7, sigma=s) for s in (0.5, 0.8, 0.5)]
    assert not torch.equal(downs[0]._taps, downs[1]._taps)
    lr_shape = _lr_size(nets[0], zs[0], downs[0])
    lr = torch.rand(lr_shape, generator=gen).to(dev)
    lrs = [lr.clone() for _ in range(B)]
    hrs = [torch.rand(1, 3, *hw, generator=gen).to(dev) for _ in range(B)]
    w0 = _tv_weight_for(nets[0], downs[0], zs[0], lr)
    ws = [w0 * r for r in (0.25, 1.0, 4.0)]
    refs = [copy.deepcopy(x) for x in nets]
    solos = [_solo_tv(refs[b], zs[b], lrs[b], hrs[b], downs[b], ws[b], std, 40 + b, cap) for b in range(B)]
    native_mask.dip_group_native(mask)
    with pytest.raises(ValueError, match="dip-amd:.*mixes zero and positive"):
        GroupedFits(nets, zs, lrs, downsamplers=downs, tv_weights=[ws[0], 0.0, ws[2]])
    mon = GroupedSRFitMonitor(hrs, capacity=cap)
    g = GroupedFits(nets, zs, lrs, downsamplers=downs, reg_noise_std=std, seeds=[40 + b for b in range(B)], lr=0.01, monitor=mon,
                    tv_weights=ws)
    assert g.pointers_outside_row0() == []
    assert [n for _, _, n in g._head_fwd + g._head_bwd] == ["head_fwd", "sr_tv_loss_fwd", "sr_tv_loss_bwd"]
    g.step(2)
    for it, _ in solos:
        it.run(2)
    _assert_group_equals_solo(g, mon, nets, refs, solos, 2, True)
    _assert_adam_and_loss(g, solos, refs)
    g.capture(warmup=1)
    g.run(4)
    for it, _ in solos:
        it.run(5)
    assert g.graph is not None
    _assert_group_equals_solo(g, mon, nets, refs, solos, 7, True)
    _assert_adam_and_loss(g, solos, refs)
    assert native_mask.dip_group_size() == 1
    # the records: loss = MSE + the instance's own TV term
    h = mon.history()
    assert (h[:, :, 0] > h[:, :, 1]).all()
