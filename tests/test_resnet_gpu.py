"""GPU suite of the ResNet backbone (models/resnet.py, dip_engine.ResNetEngine, csrc/res_kernels.hip): the two join
kernels against numpy, every fixture of tools/make_resnet_golden.py through the whole-net criterion of tests/parity.py
(constants unchanged), the fused-Adam trajectory, the inpainting notebook's ResNet arm, the out-of-scope guards, and
the full-size net once."""
import copy
import ctypes as CT
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import parity as PT
import resnet_oracle as RO

pytestmark = pytest.mark.gpu

FIXTURES = ("a", "b", "nores")
ACTS = {"LeakyReLU": "LeakyReLU", "ReLU": torch.nn.ReLU}
EPS = float(np.finfo(np.float32).eps)


def _load(name):
    g = np.load(os.path.join(GOLDEN, f"resnet_tiny_{name}.npz"))
    meta = json.loads(str(g["meta"]))
    return g, meta, ACTS[meta["act_fun"]]


def _net_from(g, meta, act):
    from models.resnet import ResNet
    net = ResNet(*meta["args"], act_fun=act, **meta["kw"])
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/")}
    assert list(net.state_dict().keys()) == list(sd.keys())
    net.load_state_dict(sd)
    return net, sd


# ---------------------------------------------------------------------------------------------- 6. the join kernels
ACT_CODES = [0.2, 1.0, -1.0, -2.0, -3.0, 0.05]      # LeakyReLU(0.2), none, Swish, ELU, ReLU, LeakyReLU(0.05)


def _np_act(t, code):
    if code > 0:
        return np.maximum(t, t.dtype.type(code) * t)
    if code == -1.0:
        return t / (1 + np.exp(-t))
    if code == -3.0:
        return np.maximum(t, 0)
    return np.where(t > 0, t, np.expm1(t))


def _np_act_grad(t, code):
    one = np.ones_like(t)
    if code > 0:
        return np.where(t > 0, one, one * t.dtype.type(code))
    if code == -1.0:
        sg = 1 / (1 + np.exp(-t))
        return sg * (1 + t * (1 - sg))
    if code == -3.0:
        return np.where(t > 0, one, 0 * one)
    return np.where(t > 0, one, np.exp(t))


def _nhwc(dev, rng, H, W, C, Cs):
    a = rng.standard_normal((H, W, Cs)).astype(np.float32)
    return a, torch.from_numpy(a).to(dev).contiguous()


@pytest.mark.parametrize("H,W,C,pad_s", [(7, 13, 4, 0), (33, 19, 8, 4), (37, 50, 32, 0), (21, 45, 36, 8), (130, 67, 32, 4)])
def test_res_join_fwd_against_numpy(dev, built, H, W, C, pad_s):
    """out = act_a(a_a x_a + b_a) + act_b(a_b x_b + b_b).  Element-wise, no accumulation: the only differences from an fp32
    numpy evaluation of the same expression are the fused multiply-add (one rounding of a*x+b instead of two: up to
    eps/2 * |a x|) and the exponential of Swish / ELU (a few ulp of the activation, which is 1.1-Lipschitz).  Bound per
    element: 8 eps * (|a_a x_a| + |b_a| + |a_b x_b| + |b_b|) against the fp64 evaluation -- 4 roundings of <= eps/2 each
    would be 2 eps; the factor 4 on top leaves room for expf."""
    import dip_native as N
    rng = np.random.default_rng(H * 1000 + W)
    for code_a in ACT_CODES:
        for ident_a, ident_b in ((False, False), (True, False), (False, True)):
            Csa, Csb, Cso = C + pad_s, C + (pad_s // 2) // 4 * 4, C + pad_s
            xa, txa = _nhwc(dev, rng, H, W, C, Csa)
            xb, txb = _nhwc(dev, rng, H, W, C, Csb)
            coef = rng.uniform(0.5, 1.5, (4, C)).astype(np.float32) * np.array([[1], [0.3], [-1], [0.3]], np.float32)
            tcoef = torch.from_numpy(coef).to(dev).contiguous()
            out = torch.full((H, W, Cso), float("nan"), device=dev)
            p = lambda r: tcoef.data_ptr() + 4 * C * r
            ta = N.DipTransform(None, None, 1.0) if ident_a else N.DipTransform(p(0), p(1), code_a)
            tb = N.DipTransform(None, None, 1.0) if ident_b else N.DipTransform(p(2), p(3), 1.0)
            N.check(built.dip_res_join_fwd(txa.data_ptr(), Csa, CT.byref(ta), txb.data_ptr(), Csb, CT.byref(tb), out.data_ptr(),
                                           Cso, H * W, C, None), "res_join_fwd")
            torch.cuda.synchronize()
            got = out.cpu().numpy()

            def ref(dt):
                A, B = xa[:, :, :C].astype(dt), xb[:, :, :C].astype(dt)
                c = coef.astype(dt)
                sa = A if ident_a else _np_act(c[0] * A + c[1], code_a)
                sb = B if ident_b else c[2] * B + c[3]
                return sa + sb
            mag = (np.abs(xa[:, :, :C]) if ident_a else np.abs(coef[0] * xa[:, :, :C]) + np.abs(coef[1])) + \
                  (np.abs(xb[:, :, :C]) if ident_b else np.abs(coef[2] * xb[:, :, :C]) + np.abs(coef[3]))
            err = np.abs(got[:, :, :C].astype(np.float64) - ref(np.float64))
            assert (err <= 8 * EPS * mag.astype(np.float64)).all(), (code_a, ident_a, ident_b, float((err / mag).max()))
            e32 = np.abs(got[:, :, :C] - ref(np.float32)).max()
            assert np.isnan(got[:, :, C:]).all()            # pad channels of the output are not touched
    print(f"res_join_fwd {H}x{W}x{C}: last max |got - fp32 numpy| {e32:.2e}")


@pytest.mark.parametrize("H,W,C,pad_s,gpad", [(7, 13, 4, 0, 0), (33, 19, 8, 4, 1), (37, 50, 32, 0, 1), (21, 45, 36, 8, 0),
                                              (130, 67, 32, 4, 1)])
def test_res_join_bwd_against_numpy(dev, built, H, W, C, pad_s, gpad):
    """gout = (g + src) [* act'(a y + b)], src read through a DipGradSrc (gpad = 1: a padded buffer folded by reflection, as
    the data gradient of a reflection-padded 3x3 conv leaves it).  Roundings: the fold's <= 3 extra additions, the sum with
    g, one product, the activation derivative: bound 8 eps * (sum of the |terms|) * |act'| against fp64 where act' is exact
    (the piecewise-linear activations), 8 eps * (sum of the |terms|) * (|act'| + 1 + |a y| + |b|) for Swish / ELU, whose
    derivative carries an ABSOLUTE error of a few eps * (1 + |t|) (see the comment at the bound).  act' of (Leaky)ReLU jumps at 0: elements whose fp64
    pre-activation sits within 8 eps * (|a y| + |b|) of the kink (where fused and unfused evaluation may pick different
    branches, both correct) are left out; they must be fewer than 1e-4 of the tensor."""
    import dip_native as N
    rng = np.random.default_rng(H * 1000 + W + 7)
    Cs = C + pad_s
    for code in ACT_CODES:
        for with_g, with_y, ident in ((True, False, False), (True, True, False), (False, True, False), (True, True, True)):
            g, tg = _nhwc(dev, rng, H, W, C, Cs)
            y, ty_ = _nhwc(dev, rng, H, W, C, Cs)
            Hg, Wg = H + 2 * gpad, W + 2 * gpad
            s, ts = _nhwc(dev, rng, Hg, Wg, C, Cs)
            coef = rng.uniform(0.5, 1.5, (2, C)).astype(np.float32) * np.array([[1], [0.3]], np.float32)
            tcoef = torch.from_numpy(coef).to(dev).contiguous()
            out = torch.full((H, W, Cs), float("nan"), device=dev)
            src = N.DipGradSrc(ts.data_ptr(), gpad, 1 if gpad else 0, Cs, 0)
            tr = N.DipTransform(None, None, code) if ident else N.DipTransform(tcoef.data_ptr(), tcoef.data_ptr() + 4 * C, code)
            N.check(built.dip_res_join_bwd(tg.data_ptr() if with_g else None, Cs, CT.byref(src), ty_.data_ptr() if with_y else None,
                                           Cs, CT.byref(tr) if with_y else None, out.data_ptr(), Cs, H, W, C, None), "res_join_bwd")
            torch.cuda.synchronize()
            got = out.cpu().numpy()[:, :, :C].astype(np.float64)
            # fp64 reference: fold the padded source (adjoint of nn.ReflectionPad2d(gpad)), add g, multiply
            S = s[:, :, :C].astype(np.float64)
            mag = np.abs(S)
            if gpad:
                ts64 = torch.from_numpy(S).permute(2, 0, 1)[None].clone().requires_grad_(False)
                x0 = torch.zeros(1, C, H, W, dtype=torch.float64, requires_grad=True)
                torch.nn.functional.pad(x0, (gpad,) * 4, mode="reflect").backward(ts64)
                S = x0.grad[0].permute(1, 2, 0).numpy()
                x1 = torch.zeros(1, C, H, W, dtype=torch.float64, requires_grad=True)
                torch.nn.functional.pad(x1, (gpad,) * 4, mode="reflect").backward(torch.from_numpy(mag).permute(2, 0, 1)[None])
                mag = x1.grad[0].permute(1, 2, 0).numpy()
            ref = S.copy()
            if with_g:
                ref += g[:, :, :C].astype(np.float64)
                mag = mag + np.abs(g[:, :, :C])
            keep = np.ones_like(ref, dtype=bool)
            if with_y:
                Y = y[:, :, :C].astype(np.float64)
                c = coef.astype(np.float64)
                t = Y if ident else c[0] * Y + c[1]
                tm = np.abs(Y) if ident else np.abs(c[0] * Y) + np.abs(c[1])
                d = _np_act_grad(t, code)
                # Swish / ELU: act' is a difference of O(1) terms (zero at t = -1.28 for Swish), so its error is absolute --
                # a few eps * (1 + |t|) from its own arithmetic and expf, plus |act''| <= 1 times the eps * (|a y| + |b|) that
                # the pre-activation itself carries; the piecewise-linear derivatives are exact
                smooth = code in (-1.0, -2.0)
                ref, mag = ref * d, mag * (np.abs(d) + ((1.0 + tm) if smooth else 0.0))
                if code in (0.2, 0.05, -3.0):
                    keep = np.abs(t) > 8 * EPS * tm
            assert (~keep).sum() <= 1e-4 * keep.size + 1
            err = np.abs(got - ref)
            assert (err[keep] <= 8 * EPS * mag[keep] + 1e-30).all(), (code, with_g, with_y, ident, float(err[keep].max()))


# ---------------------------------------------------------------------------------------------- 7 / 8. fixtures
def _loss_fn(t, m):
    return lambda o, dt: torch.nn.functional.mse_loss(o * m.to(dt), t.to(dt) * m.to(dt))


def _parity(net, spec, sd, zc, lf, out, loss, grads, g32=None, gx=None):
    """Whole-net criterion of tests/parity.py (constants unchanged) with the truth of tests/resnet_oracle.py."""
    hm = RO.hip_masks(net, spec)
    need_x = gx is not None
    zrec = {}
    out64, loss64, g64n = RO.grads(spec, sd, zc, lf, torch.float64, z_requires_grad=need_x, zrec=zrec)
    out32, loss32, g32o = RO.grads(spec, sd, zc, lf, torch.float32, z_requires_grad=need_x)
    _, _, g64 = RO.grads(spec, sd, zc, lf, torch.float64, masks=hm, z_requires_grad=need_x)
    if g32 is None:
        g32 = g32o
    named = dict(grads)
    if need_x:
        named["__input__"] = gx
        g32 = dict(g32, __input__=g32o["__input__"])
    rep = PT.grad_report(named, g64, g32, g64n, spec.zero_grad_keys())
    mrep = PT.mask_report(hm, zrec)
    psnr = PT.psnr(out.detach().cpu().numpy(), out32.numpy())
    rel = abs(float(loss) - loss32) / abs(loss32)
    print(f"out PSNR {psnr:.1f} dB, loss rel {rel:.2e}, {PT.fmt(rep)}; {PT.fmt_masks(mrep)}")
    assert psnr >= 100.0, psnr
    assert rel <= 1e-5, rel
    PT.check(rep, mrep)
    return rep


@pytest.mark.parametrize("name", FIXTURES)
def test_resnet_golden_reference_vectors(dev, name):
    from utils.common_utils import get_params, optimize
    g, meta, act = _load(name)
    net, sd = _net_from(g, meta, act)
    net = net.to(dev)
    spec = RO.ResNetSpec(*meta["args"], act_fun=act, **meta["kw"])
    zc, tc, mc = (torch.from_numpy(g[k]) for k in ("z", "target", "mask"))
    z, target, mask = zc.to(dev), tc.to(dev), mc.to(dev)
    mse = torch.nn.MSELoss()
    out = net(z)
    loss = mse(out * mask, target * mask)
    loss.backward()
    torch.cuda.synchronize()
    eng = net.__dict__["_dip_engine"]
    assert eng._arena_ok()
    names = [n for _, _, n in eng.fwd_ops + eng.bwd_ops]
    nj = meta["args"][2] if meta["kw"].get("need_residual", True) else 0
    assert sum(n.startswith("res_join_fwd:") for n in names) == nj == sum(n.startswith("res_join_bwd:") for n in names)
    assert not any(n.startswith("dgrad+:") for n in names)
    psnr = PT.psnr(out.detach().cpu().numpy(), g["out"])
    rel = abs(loss.item() - float(g["loss"])) / float(g["loss"])
    print(f"{name}: vs fixture: out PSNR {psnr:.1f} dB, loss rel {rel:.2e}")
    assert psnr >= 100.0 and rel <= 1e-5, (psnr, rel)
    grads = {k: p.grad for k, p in net.named_parameters()}
    learn = {k: v for k, v in sd.items() if k in spec.param_names()}
    # the reference's own fp32 gradients (the fixture) set the noise scale
    _parity(net, spec, learn, zc, _loss_fn(tc, mc), out, loss.item(), grads, g32={k: torch.from_numpy(g["grad/" + k]) for k in grads})
    for k, v in net.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1
    bn_keys = [k for k in sd if k.endswith(("running_mean", "running_var", "num_batches_tracked"))]

    # parameters after 1 and 3 fused-Adam iterations (rule and numbers of tests/test_net_gpu.py:154-179)
    for nsteps in (1, 3):
        net.load_state_dict(sd)
        for p in net.parameters():
            p.grad = None

        def closure():
            o = net(z)
            l = mse(o * mask, target * mask)
            l.backward()
            return l

        optimize("adam", get_params("net", net, z), closure, 0.01, nsteps)
        torch.cuda.synchronize()
        assert eng._arena_ok()
        nbad = ntot = 0
        for k, p in net.named_parameters():
            ref = torch.from_numpy(g[f"adam{nsteps}/" + k]).double()
            gr = torch.from_numpy(g["grad/" + k]).double()
            big = gr.abs() > 1e-3 * gr.abs().max().clamp_min(1e-30)
            if k.endswith(".bias") and gr.abs().max() < 1e-6:
                continue
            d = (p.detach().cpu().double() - ref).abs()
            nbad += int((d[big] > 2e-4).sum())
            ntot += int(big.sum())
        print(f"{name}: adam{nsteps}: {nbad} of {ntot} compared entries beyond 2e-4")
        assert nbad <= 1e-3 * ntot, (nsteps, nbad, ntot)
    assert bn_keys


# ---------------------------------------------------------------------------------------------- 11. options
def test_resnet_input_gradient_second_backward_deepcopy_replan(dev):
    from utils.common_utils import get_params
    g, meta, act = _load("a")
    net, sd = _net_from(g, meta, act)
    net = net.to(dev)
    spec = RO.ResNetSpec(*meta["args"], act_fun=act, **meta["kw"])
    learn = {k: v for k, v in sd.items() if k in spec.param_names()}
    zc, tc, mc = (torch.from_numpy(g[k]) for k in ("z", "target", "mask"))
    z, target, mask = zc.to(dev).clone(), tc.to(dev), mc.to(dev)
    mse = torch.nn.MSELoss()
    params = get_params("net,input", net, z)            # opt_over='net,input': one more data gradient at the bottom
    assert params[-1] is z and z.requires_grad
    out = net(z)
    loss = mse(out * mask, target * mask)
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in net.named_parameters()}
    _parity(net, spec, learn, zc, _loss_fn(tc, mc), out, loss.item(), grads, gx=z.grad)
    eng = net.__dict__["_dip_engine"]
    base = eng.grads.data_ptr()
    assert all(p.grad.data_ptr() == base + 4 * o for p, o in zip(eng.param_list, eng.slots))     # .grad views alias the arena
    # a second backward() without zero_grad() accumulates (tests/test_closure_gpu.py:297 for skip nets)
    gz1 = z.grad.clone()
    out = net(z)
    mse(out * mask, target * mask).backward()
    torch.cuda.synchronize()
    for k, p in net.named_parameters():
        assert torch.allclose(p.grad, 2 * grads[k], rtol=1e-5, atol=1e-9), k
    assert torch.allclose(z.grad, 2 * gz1, rtol=1e-5, atol=1e-12)
    # deepcopy -> an engine of its own, same numbers, independent parameters
    for p in net.parameters():
        p.grad = None
    net2 = copy.deepcopy(net)
    eng2 = net2.__dict__["_dip_engine"]
    assert eng2 is not eng and eng2.kind == "resnet"
    o1, o2 = net(z.detach()), net2(z.detach())
    torch.cuda.synchronize()
    assert torch.equal(o1, o2) and eng2._arena_ok() and eng._arena_ok()
    assert eng2.params.data_ptr() != eng.params.data_ptr()
    with torch.no_grad():
        next(net2.parameters()).add_(1.0)
    assert not torch.equal(next(net2.parameters()), next(net.parameters()))
    # a second input size -> a new plan, and back
    key = eng.shape_key
    z2 = torch.rand(1, 1, 29, 37, device=dev) * 0.1
    o = net(z2)
    assert o.shape == (1, 3, 29, 37) and eng.shape_key == (29, 37, 1) != key
    sdn = {k: v.detach().cpu() for k, v in net.state_dict().items() if k in learn}
    ref, _, _ = RO.grads(spec, sdn, z2.cpu(), lambda o_, dt: o_.sum(), torch.float32)
    assert PT.psnr(o.detach().cpu().numpy(), ref.numpy()) >= 100.0


def test_resnet_need_residual_false_has_no_join(dev):
    g, meta, act = _load("nores")
    net, _ = _net_from(g, meta, act)
    net = net.to(dev)
    net(torch.from_numpy(g["z"]).to(dev))
    eng = net.__dict__["_dip_engine"]
    names = [n for _, _, n in eng.fwd_ops + eng.bwd_ops]
    assert not any(n.startswith("res_join") for n in names) and "act_bwd:first" in names


# ---------------------------------------------------------------------------------------------- 12. guards
def test_resnet_out_of_scope_paths_raise(dev):
    from models.resnet import ResNet
    from utils.common_utils import get_noise, get_params, optimize
    from utils.fit_monitor import FitMonitor
    from utils.loss_head import MSEHead
    from dip_group import GroupedFits
    import dip_engine
    nets = [ResNet(1, 3, 1, 8).to(dev) for _ in range(2)]
    zs = [get_noise(1, "noise", (32, 32)).to(dev) for _ in range(2)]
    ts = [torch.rand(1, 3, 32, 32, device=dev) for _ in range(2)]
    with pytest.raises(NotImplementedError, match="GroupedFits covers skip"):
        GroupedFits(nets, zs, ts)
    with pytest.raises(NotImplementedError, match="back-tracking covers skip"):
        FitMonitor(nets[0], ts[0], backtracking=True)
    FitMonitor(nets[0], ts[0], backtracking=False)              # the monitor itself does not need the engine
    with pytest.raises(NotImplementedError, match="1x1 output conv"):
        MSEHead(nets[0], ts[0])
    net, z, t = nets[0], zs[0], ts[0]
    mse = torch.nn.MSELoss()

    def closure():
        l = mse(net(z), t)
        l.backward()
        return l

    with pytest.raises(NotImplementedError, match="hipGraph capture"):
        optimize("adam", get_params("net", net, z), closure, 0.01, 8, graph=True)
    assert dip_engine._graph_warmup[0] == 0
    assert not torch.cuda.is_current_stream_capturing()
    optimize("adam", get_params("net", net, z), closure, 0.01, 2)          # ... and the eager path is untouched by the refusal
    with pytest.raises(NotImplementedError, match="eval-mode"):
        net.eval()


# ---------------------------------------------------------------------------------------------- 9. the notebook arm
def test_inpainting_notebook_resnet_arm(dev):
    """inpainting.ipynb, NET_TYPE = 'ResNet' of the 'library' figure, restated cell by cell on a synthetic 96 x 128 image:
    the import cell, `net = ResNet(input_depth, img_np.shape[0], 8, 32, need_sigmoid=True, act_fun='LeakyReLU')`,
    LR = 0.001, param_noise = False, input_depth = 1, masked MSE, optimize('adam').  40 iterations: the loss is finite
    and falls: mean of the last 5 below a third of the mean of the first 3.

    The factor: the same 40 iterations on the CPU through tests/resnet_oracle.py (fp32, torch.optim.Adam, seed 0, the
    same image / mask / input construction) gave
        0.0685 0.0521 0.0457 0.0429 0.0409 0.0395 0.0382 0.0364 0.0346 0.0326 0.0333 0.0296 0.0286 0.0252 0.0222 0.0214
        0.0183 0.0160 0.0153 0.0139 0.0115 0.0121 0.0100 0.0079 0.0082 0.0068 0.0068 0.0059 0.0058 0.0053 0.0050 0.0050
        0.0047 0.0042 0.0041 0.0040 0.0036 0.0037 0.0034 0.0033
    i.e. a factor 15.5 between the two means; 3 leaves a five-fold margin for trajectories of different summation orders
    separating over 40 Adam steps."""
    # --- import cell (the names the notebook imports from models)
    from models.resnet import ResNet
    from models.unet import UNet  # noqa: F401
    from models.skip import skip  # noqa: F401
    from utils.inpainting_utils import get_noise, get_params, optimize
    torch.manual_seed(0)
    H, W = 96, 128
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    img = torch.stack([0.5 + 0.4 * torch.sin(6.0 * xx + 3.0 * yy), 0.5 + 0.4 * torch.cos(5.0 * yy), 0.3 + 0.5 * xx * yy])[None]
    img_mask = torch.ones(1, 1, H, W)
    img_mask[:, :, 30:50, 40:90] = 0
    img_mask[:, :, 70:80, 10:30] = 0
    img_var, mask_var = img.to(dev), img_mask.to(dev)
    # --- set-up cell
    input_depth, LR, num_iter, param_noise = 1, 0.001, 40, False
    net = ResNet(input_depth, img.shape[1], 8, 32, need_sigmoid=True, act_fun='LeakyReLU')
    net = net.to(dev)
    net_input = get_noise(input_depth, 'noise', (H, W)).to(dev)
    mse = torch.nn.MSELoss().to(dev)
    losses = []

    def closure():
        out = net(net_input)
        total_loss = mse(out * mask_var, img_var * mask_var)
        total_loss.backward()
        losses.append(total_loss.detach())
        return total_loss

    p = get_params('net', net, net_input)
    optimize('adam', p, closure, LR, num_iter)
    torch.cuda.synchronize()
    ls = [float(l) for l in losses]
    print("loss curve:", " ".join(f"{v:.4f}" for v in ls))
    assert len(ls) == num_iter and all(np.isfinite(ls))
    assert np.mean(ls[-5:]) < np.mean(ls[:3]) / 3.0, (ls[:3], ls[-5:])
    eng = net.__dict__["_dip_engine"]
    assert eng._arena_ok() and eng.shape_key == (H, W, 1)
    assert eng.fwd_id == num_iter and len(eng._clists) <= 3           # planned once: one command list per direction


# ---------------------------------------------------------------------------------------------- 10. full size, once
def test_resnet_fullsize_iteration1_parity(dev):
    """The notebook's net, ResNet(1, 3, 8, 32), at 448 x 704: iteration-1 parity against tests/resnet_oracle.py (fp64 truth
    and fp32 yard-stick on the host).  Here the chain convs run on conv_thin / wgrad_thin, not on the low-resolution
    kernels the tiny fixtures take."""
    from models.resnet import ResNet
    from utils.common_utils import get_noise
    torch.manual_seed(0)
    net = ResNet(1, 3, 8, 32, need_sigmoid=True, act_fun='LeakyReLU')
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0.0, 0.3)
    spec = RO.ResNetSpec(1, 3, 8, 32)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items() if k in spec.param_names()}
    H, W = 448, 704
    zc = get_noise(1, 'noise', (H, W))
    tc = torch.rand(1, 3, H, W)
    mc = (torch.rand(1, 1, H, W) > 0.3).float()
    net = net.to(dev)
    z, target, mask = zc.to(dev), tc.to(dev), mc.to(dev)
    out = net(z)
    loss = torch.nn.functional.mse_loss(out * mask, target * mask)
    loss.backward()
    torch.cuda.synchronize()
    eng = net.__dict__["_dip_engine"]
    nthin = sum(1 for fn, args, n in eng.fwd_ops + eng.bwd_ops if fn is eng.lib.dip_conv_igemm and eng.lib.dip_conv_thin_eligible(args[0]))
    assert nthin >= 34, nthin           # 17 chain convs forward + their data gradients
    grads = {k: p.grad for k, p in net.named_parameters()}
    _parity(net, spec, sd, zc, _loss_fn(tc, mc), out, loss.item(), grads)
