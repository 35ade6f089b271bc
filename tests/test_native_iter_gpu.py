"""dip_optim.NativeIteration on the GPU: the autograd-free iteration (ONE dip_iter_run call: reg-noise, forward list, fused loss
head, backward list, Adam) against the eager closure it restates

    opt.zero_grad(); x = reg() if reg else net_input; loss, out = head(x); loss.backward(); opt.step()

The eager path is the truth (the rest of the suite holds it to the oracle); both issue the same launches in the same order on
the same streams, so every comparison here is torch.equal -- no tolerance anywhere."""
import statistics
import time
from types import SimpleNamespace

import pytest
import torch

from test_net_gpu import NETS

pytestmark = pytest.mark.gpu

# the `default`, `library` and `snail` constructions of tests/test_net_gpu.py and an input size for each
CASES = {"default": ("tiny_default", (64, 64)), "library": ("tiny_library", (64, 96)), "snail": ("tiny_snail", (48, 64))}
LIBRARY_CH = [16, 32, 64, 128, 128, 128]          # inpainting.ipynb:222-232 of the reference


def _fit(dev, net, cin, size, seed, masked, noisy, lr=0.01):
    from dip_optim import FusedAdam
    from utils.common_utils import get_params
    from utils.loss_head import MSEHead
    from utils.reg_noise import RegNoise
    net = net.to(dev)
    g = torch.Generator().manual_seed(seed + 1)
    z = (torch.rand(1, cin, *size, generator=g) * 0.1).to(dev)
    target = torch.rand(1, 3, *size, generator=g).to(dev)
    mask = (torch.rand(1, 1, *size, generator=g) > 0.3).float().to(dev) if masked else None
    head = MSEHead(net, target, mask=mask)
    reg = RegNoise(z, 1. / 30., seed=7) if noisy else None
    opt = FusedAdam(get_params('net', net, z), lr=lr)
    return SimpleNamespace(net=net, z=z, target=target, mask=mask, head=head, reg=reg, opt=opt, out=None)


def _tiny(dev, case, seed=3, masked=False, noisy=False, size=None):
    from models.skip import skip
    name, sz = CASES[case]
    cfg = NETS[name]
    torch.manual_seed(seed)
    return _fit(dev, skip(*cfg["args"], **cfg["kw"]), cfg["args"][0], size or sz, seed, masked, noisy)


def _eager_step(f):
    """One iteration of the eager closure (autograd drives the engine)."""
    f.opt.zero_grad()
    x = f.reg() if f.reg is not None else f.z
    loss, out = f.head(x)
    loss.backward()
    f.opt.step()
    f.out = out
    return loss.detach()


def _native(f):
    from dip_optim import NativeIteration
    return NativeIteration(f.net, f.head, f.opt, f.z, reg_noise=f.reg)


def _assert_same_state(a, b, out_a, out_b, what=""):
    """Everything an iteration leaves behind, bit for bit: parameters, BatchNorm buffers, Adam's moments and step count, the
    last output and the last gradients."""
    torch.cuda.synchronize()
    sa, sb = a.net.state_dict(), b.net.state_dict()
    assert list(sa) == list(sb)
    for k in sa:                                    # parameters + running_mean / running_var / num_batches_tracked
        assert torch.equal(sa[k], sb[k]), (what, k)
    assert any(k.endswith("num_batches_tracked") for k in sa)
    for (k, p), (_, q) in zip(a.net.named_parameters(), b.net.named_parameters()):
        assert p.requires_grad and q.requires_grad
        assert p.grad is not None and q.grad is not None, (what, k)
        assert torch.equal(p.grad, q.grad), (what, k)
    assert len(a.opt._groups) == len(b.opt._groups)
    for ga, gb in zip(a.opt._groups, b.opt._groups):
        assert torch.equal(ga.m, gb.m) and torch.equal(ga.v, gb.v), what
    assert a.opt.device_step_count() == b.opt.device_step_count() == a.opt.step_count == b.opt.step_count, what
    if a.reg is not None:
        assert torch.equal(a.reg.offset, b.reg.offset), what
    assert torch.equal(out_a, out_b), what


def _check_k(a, b, k):
    """k eager iterations on fit a, k NativeIteration.step() on its twin b."""
    it = _native(b)
    la = [_eager_step(a) for _ in range(k)]
    lb = [it.step() for _ in range(k)]
    for x in lb:
        assert x.dim() == 0 and not x.requires_grad and x.grad_fn is None
    assert torch.equal(torch.stack(la), torch.stack(lb)), (torch.stack(la).tolist(), torch.stack(lb).tolist())
    assert tuple(it.out.shape) == tuple(a.out.shape) and not it.out.requires_grad
    _assert_same_state(a, b, a.out, it.out)
    # p.grad is the engine's gradient-arena view, as the eager path leaves it
    eng = b.net.__dict__["_dip_engine"]
    for p, o in zip(eng.param_list, eng.slots):
        assert p.grad.data_ptr() == eng.grads.data_ptr() + 4 * o
    assert it.iterations == k
    return it


def test_two_eager_fits_from_one_seed_are_bit_identical(dev):
    """The premise of every test below: the eager path is deterministic on this card."""
    a, b = _tiny(dev, "default", masked=True, noisy=True), _tiny(dev, "default", masked=True, noisy=True)
    la = [_eager_step(a) for _ in range(3)]
    lb = [_eager_step(b) for _ in range(3)]
    assert torch.equal(torch.stack(la), torch.stack(lb))
    _assert_same_state(a, b, a.out, b.out)


@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("masked,noisy", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("case", list(CASES))
def test_bit_identical_to_the_eager_closure(dev, case, masked, noisy, k):
    a, b = _tiny(dev, case, masked=masked, noisy=noisy), _tiny(dev, case, masked=masked, noisy=noisy)
    _check_k(a, b, k)


def test_bit_identical_default_net_512(dev):
    """The headline construction (denoising.ipynb:160-165: 2 217 831 parameters) at 512 x 512, reg-noise on, k = 2."""
    from models import get_net

    def make():
        torch.manual_seed(0)
        net = get_net(32, 'skip', 'reflection', skip_n33d=128, skip_n33u=128, skip_n11=4, num_scales=5, upsample_mode='bilinear')
        return _fit(dev, net, 32, (512, 512), 0, masked=False, noisy=True)

    _check_k(make(), make(), 2)


def test_interchangeable_with_the_eager_closure(dev):
    """2 native steps, 2 eager closure steps, 2 native steps on ONE net == 6 eager steps."""
    a, b = _tiny(dev, "default", masked=True, noisy=True), _tiny(dev, "default", masked=True, noisy=True)
    la = [_eager_step(a) for _ in range(6)]
    it = _native(b)
    lb = [it.step(), it.step(), _eager_step(b), _eager_step(b)]
    out_mid = b.out
    lb += [it.step(), it.step()]
    assert torch.equal(torch.stack(la), torch.stack(lb))
    assert out_mid.data_ptr() != it.out.data_ptr()
    _assert_same_state(a, b, a.out, it.out)


def test_run_returns_the_losses_without_a_host_sync(dev):
    a, b = _tiny(dev, "snail", noisy=True), _tiny(dev, "snail", noisy=True)
    it = _native(b)
    la = [_eager_step(a) for _ in range(5)]
    first = it.step()                                # warm-up: plans, arenas and command arrays are built here
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses = it.run(4)
        one_more = it.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    la.append(_eager_step(a))
    assert losses.shape == (4,) and not losses.requires_grad and losses.grad_fn is None
    assert torch.equal(torch.stack(la), torch.cat([first[None], losses, one_more[None]]))
    _assert_same_state(a, b, a.out, it.out)
    assert it.run(0).shape == (0,)


def test_no_autograd(dev):
    a, b = _tiny(dev, "library", masked=True), _tiny(dev, "library", masked=True)
    it = _native(b)
    with torch.no_grad():
        l0 = it.step()
    with torch.enable_grad():
        l1 = it.step()
    for x in (l0, l1, it.out):
        assert not x.requires_grad and x.grad_fn is None
    for p in b.net.parameters():
        assert p.requires_grad and p.is_leaf and p.grad is not None and not p.grad.requires_grad
    la = [_eager_step(a) for _ in range(2)]
    assert torch.equal(torch.stack(la), torch.stack([l0, l1]))
    _assert_same_state(a, b, a.out, it.out)


def test_replanning_target_mask_lr(dev):
    """Replacing the head's target or mask, or changing the optimiser's lr, must not replay stale slots."""
    a, b = _tiny(dev, "default", masked=True, noisy=True), _tiny(dev, "default", masked=True, noisy=True)
    it = _native(b)
    la, lb = [_eager_step(a)], [it.step()]
    g = torch.Generator().manual_seed(99)
    new_target = torch.rand(a.target.shape, generator=g).to(dev)
    new_mask = (torch.rand(a.mask.shape, generator=g) > 0.5).float().to(dev)
    for f in (a, b):
        f.head.target = new_target.clone()
    la.append(_eager_step(a)), lb.append(it.step())
    _assert_same_state(a, b, a.out, it.out, "target")
    for f in (a, b):
        f.head.mask = new_mask.clone()
    la.append(_eager_step(a)), lb.append(it.step())
    _assert_same_state(a, b, a.out, it.out, "mask")
    for f in (a, b):
        f.head.mask, f.head.mask_c = None, 0
    la.append(_eager_step(a)), lb.append(it.step())
    _assert_same_state(a, b, a.out, it.out, "no mask")
    for f in (a, b):
        f.opt.lr = 0.003
    la.append(_eager_step(a)), lb.append(it.step())
    _assert_same_state(a, b, a.out, it.out, "lr")
    for f in (a, b):
        f.head.target.mul_(0.5)                      # in place: same slots, new values
    la.append(_eager_step(a)), lb.append(it.step())
    _assert_same_state(a, b, a.out, it.out, "in place")
    assert torch.equal(torch.stack(la), torch.stack(lb))
    assert len(set(x.item() for x in la)) == len(la)          # (every change did change the loss)


def test_replanning_input_size(dev):
    """Another input size on the same net rebuilds the engine's plan and with it the command arrays -- in both directions."""
    from dip_optim import NativeIteration
    from utils.loss_head import MSEHead
    a, b = _tiny(dev, "default", noisy=False), _tiny(dev, "default", noisy=False)
    it = _native(b)
    la, lb = [_eager_step(a)], [it.step()]
    lists0 = it._plan["lists"]
    g = torch.Generator().manual_seed(5)
    z2 = (torch.rand(1, 8, 32, 48, generator=g) * 0.1).to(dev)
    t2 = torch.rand(1, 3, 32, 48, generator=g).to(dev)
    a2 = SimpleNamespace(net=a.net, z=z2, head=MSEHead(a.net, t2), reg=None, opt=a.opt, out=None)
    it2 = NativeIteration(b.net, MSEHead(b.net, t2), b.opt, z2)
    la.append(_eager_step(a2)), lb.append(it2.step())
    assert tuple(it2.out.shape) == (1, 3, 32, 48)
    _assert_same_state(a, b, a2.out, it2.out, "32x48")
    la.append(_eager_step(a)), lb.append(it.step())          # back to 64 x 64: the first object notices the new plan
    assert it._plan["lists"] is not lists0
    _assert_same_state(a, b, a.out, it.out, "64x64 again")
    assert torch.equal(torch.stack(la), torch.stack(lb))


def test_command_list_cache_is_keyed_on_the_list_it_compiled(dev):
    """The engine's compiled lists are found again by the identity of the op list they were compiled from -- the forward list
    without the output conv by that of fwd_ops, not of the slice -- another list under the same key is compiled afresh in
    place of the old one, and an iteration compiles nothing."""
    b = _tiny(dev, "default", size=(32, 48))         # (the size of tests/golden/net_tiny_default.npz)
    it = _native(b)
    it.step()
    eng = b.net.__dict__["_dip_engine"]
    fwd, bwd = eng._launch_forward(None, None, False, compile_only=True), eng._launch_backward(None, compile_only=True)
    assert fwd is not None and bwd is not None and fwd is not bwd
    assert eng._launch_forward(None, None, False, compile_only=True) is fwd
    assert eng._launch_backward(None, compile_only=True) is bwd
    lists = it._plan["lists"]
    for _ in range(20):
        it.step()
    assert eng._launch_forward(None, None, False, compile_only=True) is fwd          # no recompile per iteration
    assert eng._launch_backward(None, compile_only=True) is bwd
    assert it._plan["lists"] is lists and it.iterations == 21
    n = len(eng._clists)
    eng.bwd_ops = list(eng.bwd_ops)                  # same length, same contents, another object
    bwd2 = eng._launch_backward(None, compile_only=True)
    assert bwd2 is not bwd and len(eng._clists) == n
    assert eng._launch_backward(None, compile_only=True) is bwd2
    assert eng._launch_forward(None, None, False, compile_only=True) is fwd
    torch.cuda.synchronize()


def test_refuses_capture_and_eval(dev, monkeypatch):
    b = _tiny(dev, "snail")
    it = _native(b)
    it.step()
    torch.cuda.synchronize()
    before = [p.detach().clone() for p in b.net.parameters()]
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="dip-amd:.*hipGraph"):
        it.step()
    with pytest.raises(RuntimeError, match="dip-amd:.*hipGraph"):
        _native(b)
    monkeypatch.undo()
    b.net.eval()
    with pytest.raises(NotImplementedError, match="dip-amd:.*eval"):
        it.step()
    with pytest.raises(NotImplementedError, match="dip-amd:.*eval"):
        _native(b)
    b.net.train()
    torch.cuda.synchronize()
    for p, q in zip(b.net.parameters(), before):             # a refused step launched nothing
        assert torch.equal(p, q)
    assert it.iterations == 1 and b.opt.step_count == 1
    it.step()


def test_guards_on_the_device(dev):
    """The out-of-scope cases that need device tensors to come about (the rest: tests/test_native_iter_host.py)."""
    from dip_optim import FusedAdam, NativeIteration
    from utils.common_utils import get_params
    from utils.loss_head import MSEHead
    b = _tiny(dev, "default")
    other = _tiny(dev, "default", seed=4)
    with pytest.raises(ValueError, match="dip-amd:.*another net"):
        NativeIteration(b.net, other.head, b.opt, b.z)
    with pytest.raises(TypeError, match="dip-amd:.*MSEHead"):
        NativeIteration(b.net, lambda x: x, b.opt, b.z)
    with pytest.raises(TypeError, match="dip-amd:.*FusedAdam"):
        NativeIteration(b.net, b.head, torch.optim.Adam(b.net.parameters(), lr=0.01), b.z)
    with pytest.raises(TypeError, match="dip-amd:.*RegNoise"):
        NativeIteration(b.net, b.head, b.opt, b.z, reg_noise=lambda: b.z)
    zin = b.z.clone()
    opt_in = FusedAdam(get_params('net,input', b.net, zin), lr=0.01)
    with pytest.raises(ValueError, match="dip-amd:.*get_params"):
        NativeIteration(b.net, MSEHead(b.net, b.target), opt_in, zin)
    with pytest.raises(RuntimeError, match="dip-amd:.*CPU"):
        NativeIteration(b.net, b.head, b.opt, b.z.cpu())


def test_host_issue_time_is_below_the_eager_closure_library_448x704(dev):
    """The 'library' inpainting net (inpainting.ipynb:222-232) at 448 x 704, masked MSE, no reg-noise: median host-issue time
    per iteration (first call until the last step returns, before the closing synchronize) of 5 interleaved blocks x 50
    iterations; NativeIteration's median must be below the eager closure's, measured here on the same card."""
    from models.skip import skip

    def make():
        torch.manual_seed(0)
        net = skip(1, 3, num_channels_down=LIBRARY_CH, num_channels_up=LIBRARY_CH, num_channels_skip=[0] * 6, filter_size_up=3,
                   filter_size_down=5, filter_skip_size=1, upsample_mode='nearest', need1x1_up=False, need_sigmoid=True,
                   need_bias=True, pad='reflection', act_fun='LeakyReLU')
        return _fit(dev, net, 1, (448, 704), 0, masked=True, noisy=False)

    a, b = make(), make()
    it = _native(b)
    for _ in range(5):                               # warm-up of both forms
        _eager_step(a)
        it.step()
    torch.cuda.synchronize()
    blocks, n = 5, 50
    host = {"eager": [], "native": []}
    wall = {"eager": [], "native": []}
    for _ in range(blocks):
        for name, one in (("eager", lambda: _eager_step(a)), ("native", it.step)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                one()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host[name].append((t1 - t0) / n * 1e3)
            wall[name].append((t2 - t0) / n * 1e3)
    med = {k: statistics.median(v) for k, v in host.items()}
    print("host-issue ms/iteration: eager", [round(x, 3) for x in host["eager"]], "native", [round(x, 3) for x in host["native"]])
    print("wall ms/iteration:       eager", [round(x, 3) for x in wall["eager"]], "native", [round(x, 3) for x in wall["native"]])
    print(f"medians: eager {med['eager']:.3f} ms, native {med['native']:.3f} ms, ratio {med['eager'] / med['native']:.2f}")
    _assert_same_state(a, b, a.out, it.out)          # 255 iterations each, still bit-identical
    assert med["native"] < med["eager"], med
