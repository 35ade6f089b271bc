"""SGLD fits on a real MI355X: dip_optim.FusedAdam(weight_decay=, noise_std=, noise_seed=) eager, under NativeIteration, under
GraphedIteration and as rows of a dip_group.GroupedFits.  The eager SGLD step is held to the specification -- plain
FusedAdam.step() followed by dip_noise_axpy over the arena per tests/sgld_ref.py -- and every other form to the eager one; all
comparisons are torch.equal."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

import hipops as H  # noqa: E402
import sgld_ref as S  # noqa: E402
from test_group_gpu import _problem  # noqa: E402
from test_group_monitor_gpu import _stream_pool_stands_where_it_stood  # noqa: E402,F401  (autouse: the engines of this module
#                                                                                          draw pooled streams too)
from test_native_iter_gpu import _assert_same_state, _eager_step, _fit  # noqa: E402
from test_native_iter_host import _small  # noqa: E402
from test_sr_head_gpu import _sr_fit  # noqa: E402

HW = (36, 52)                     # 9 x 13 at the deepest scale: Concat's centre crops (tests/test_group_gpu.py)
STD, WD = 0.01, 5e-8


def _sgld_opt(f, std=STD, wd=0.0, seed=3, **kw):
    from dip_optim import FusedAdam
    from utils.common_utils import get_params
    return FusedAdam(get_params('net', f.net, f.z), lr=0.01, weight_decay=wd, noise_std=std, noise_seed=seed, **kw)


def _mse_fit(dev, std=STD, wd=0.0, seed=3, sgld=True, reg_seed=None, hw=HW):
    torch.manual_seed(11)
    f = _fit(dev, _small(), 8, hw, 5, masked=True, noisy=True)
    if reg_seed is not None:
        from utils.reg_noise import RegNoise
        f.reg = RegNoise(f.z, 1. / 30., seed=reg_seed)
    if sgld:
        f.opt = _sgld_opt(f, std, wd, seed)
    return f


def _make(dev, head, **kw):
    if head == "mse":
        return _mse_fit(dev, **kw)
    f = _sr_fit(dev, noisy=True)                                    # 64 x 96, factor 4 (tests/test_sr_head_gpu.py)
    f.opt = _sgld_opt(f, kw.get("std", STD), kw.get("wd", 0.0), kw.get("seed", 3))
    return f


def _native(f, **kw):
    from dip_optim import NativeIteration
    return NativeIteration(f.net, f.head, f.opt, f.z, reg_noise=f.reg, **kw)


def _same_sgld(a, b, what=""):
    assert len(a.opt._groups) == len(b.opt._groups) == 1
    assert torch.equal(a.opt._groups[0].sgld, b.opt._groups[0].sgld), what
    assert a.opt._groups[0].ranges == b.opt._groups[0].ranges


def _reference_steps(f, stds, seed):
    """The specification on a plain-Adam fit: FusedAdam.step(), then the arena perturbed by dip_noise_axpy under the SGLD key
    inside the 4-D parameters' ranges, with stds[t] at offset t * ceil(n / 4)."""
    eng = f.net.__dict__["_dip_engine"]
    for t, std in enumerate(stds):
        _eager_step(f)
        g = f.opt._groups[0]
        assert len(f.opt._groups) == 1 and g.base == eng.params.data_ptr()
        n = g.numel
        ranges = S.expected_ranges(eng.param_list)
        arena = eng.params[:n]
        noisy, _ = H.noise_axpy(arena, std, S.stream_seed(seed), t * ((n + 3) // 4), "host")
        inside = torch.from_numpy(S.inside(n, ranges)).to(arena.device)
        with torch.no_grad():
            arena.copy_(torch.where(inside, noisy, arena))
    return n, ranges


def _params_equal(a, b, what=""):
    torch.cuda.synchronize()
    for (k, p), (_, q) in zip(a.net.named_parameters(), b.net.named_parameters()):
        assert torch.equal(p, q), (what, k)


# ------------------------------------------------------------------------------------------ eager == the specification
def test_eager_sgld_is_adam_plus_the_pinned_noise(dev):
    seed = 2 ** 32 + 7
    a, ref = _mse_fit(dev, seed=seed), _mse_fit(dev, sgld=False)
    for _ in range(4):
        _eager_step(a)
    n, ranges = _reference_steps(ref, [STD] * 4, seed)
    _params_equal(a, ref)
    g = a.opt._groups[0]
    assert g.ranges == ranges and g.numel == n and len(ranges) >= 2
    assert a.opt.device_noise_offset() == 4 * ((n + 3) // 4)
    # the noise is there (which parameters it lands on: test_explicit_subset_and_weight_decay, after one step)
    plain = _mse_fit(dev, sgld=False)
    for _ in range(4):
        _eager_step(plain)
    torch.cuda.synchronize()
    for (k, p), (_, q) in zip(a.net.named_parameters(), plain.net.named_parameters()):
        if p.dim() == 4:
            assert not torch.equal(p, q), k


def test_explicit_subset_and_weight_decay(dev):
    """noise_params = two weights: only they are perturbed in step 0; weight_decay alone moves every parameter and draws no noise."""
    a, plain = _mse_fit(dev, sgld=False), _mse_fit(dev, sgld=False)
    convs = [p for p in a.net.parameters() if p.dim() == 4]
    sub = [convs[1], convs[-1]]
    a.opt = _sgld_opt(a, noise_params=sub)
    _eager_step(a)
    _eager_step(plain)
    torch.cuda.synchronize()
    for p, q in zip(a.net.parameters(), plain.net.parameters()):
        assert torch.equal(p, q) != any(p is s for s in sub)
    assert len(a.opt._groups[0].ranges) == 2
    w = _mse_fit(dev, std=0.0, wd=1e-2)
    _eager_step(w)
    torch.cuda.synchronize()
    assert w.opt.sgld and not all(torch.equal(p, q) for p, q in zip(w.net.parameters(), plain.net.parameters()))


def test_streams_are_separated(dev):
    """RegNoise(seed=0) and noise_seed=0 together: the normals added to the first weights in step 0 are not the normals added
    to the input (without the key XOR they would be, element for element), they are the SGLD key's."""
    a, plain = _mse_fit(dev, seed=0, reg_seed=0), _mse_fit(dev, sgld=False, reg_seed=0)
    _eager_step(a)
    _eager_step(plain)
    torch.cuda.synchronize()
    b0, e0 = a.opt._groups[0].ranges[0]
    k = min(256, e0 - b0)
    eng_a, eng_p = a.net.__dict__["_dip_engine"], plain.net.__dict__["_dip_engine"]
    z_p = ((eng_a.params[b0:b0 + k] - eng_p.params[b0:b0 + k]) / STD).cpu().double()
    z_in = ((a.reg.out.reshape(-1)[b0:b0 + k] - a.z.reshape(-1)[b0:b0 + k]) / (1. / 30.)).cpu().double()
    want_in = H.noise_axpy(torch.zeros(b0 + k, device=dev), 1.0, 0, 0, "host")[0][b0:].cpu().double()
    want_p = H.noise_axpy(torch.zeros(b0 + k, device=dev), 1.0, S.stream_seed(0), 0, "host")[0][b0:].cpu().double()
    assert (z_in - want_in).abs().max() < 1e-3 and (z_p - want_p).abs().max() < 1e-3       # (each is the stream it should be)
    assert (z_p - z_in).abs().max() > 0.5 and (z_p - z_in).abs().mean() > 0.3              # ... and they are not each other


# ------------------------------------------------------------------------------------------ eager == native
@pytest.mark.parametrize("head", ["mse", "sr"])
def test_native_iteration_is_bit_identical_to_the_eager_closure(dev, head):
    kw = dict(wd=WD, seed=2 ** 64 - 1)
    a, b, c = _make(dev, head, **kw), _make(dev, head, **kw), _make(dev, head, **kw)
    la = [_eager_step(a) for _ in range(6)]
    it = _native(b)
    lb = it.run(6)
    assert "adam_sgld_step_dev" in it._plan["lists"].phases[-1].names and "adam_step_dev" not in it._plan["lists"].phases[-1].names
    assert torch.equal(torch.stack(la), lb)
    _assert_same_state(a, b, a.out, it.out, head)
    _same_sgld(a, b, head)
    n = a.opt._groups[0].numel
    assert b.opt.device_noise_offset() == 6 * ((n + 3) // 4)
    # alternating every 2 iterations on one net / head / optimiser
    itc = _native(c)
    lc = list(itc.run(2)) + [_eager_step(c), _eager_step(c)] + list(itc.run(2))
    assert torch.equal(torch.stack(la), torch.stack(lc))
    _assert_same_state(a, c, a.out, itc.out, head + " alternating")
    _same_sgld(a, c, head + " alternating")


def test_default_optimiser_keeps_its_plan(dev):
    """With the new keywords at their defaults the Adam phase holds dip_adam_step_dev and the key has the fields it had."""
    f = _mse_fit(dev, sgld=False)
    it = _native(f)
    it.run(1)
    assert it._plan["lists"].phases[-1].names == ["adam_tick", "adam_step_dev"]
    assert not hasattr(f.opt._groups[0], "sgld")
    assert len(it._key) == 11                                     # engine (4), parameters, lr, betas, eps, groups, head, reg
    s = _mse_fit(dev)
    its = _native(s)
    its.run(1)
    assert len(its._key) == 13 and its._key[9] == 0.0 and its._plan["lists"].phases[-1].names == ["adam_tick", "adam_sgld_step_dev"]


def test_noise_level_through_the_setter(dev):
    seed, stds = 9, [STD, STD, 0.05, 0.05, 0.0, 0.0]
    a, ref = _mse_fit(dev, seed=seed), _mse_fit(dev, sgld=False)
    it = _native(a)
    it.run(2)
    plan = it._plan
    a.opt.set_noise_std(0.05)
    it.run(2)
    a.opt.set_noise_std(0.0)                                       # the SGLD entry point stays and the stream keeps advancing
    it.run(2)
    assert it._plan is plan
    n, _ = _reference_steps(ref, stds, seed)
    _params_equal(a, ref)
    assert a.opt.device_noise_offset() == 6 * ((n + 3) // 4) and a.opt.noise_std == 0.0


# ------------------------------------------------------------------------------------------ hipGraph capture
def test_graphed_iteration_of_an_eager_sgld_closure(dev):
    from dip_optim import GraphedIteration
    a, b = _mse_fit(dev, wd=WD), _mse_fit(dev, wd=WD)
    for _ in range(6):
        _eager_step(a)

    def closure():
        loss, out = b.head(b.reg())
        loss.backward()
        b.out = out
        return loss

    it = GraphedIteration(b.opt, closure, warmup=2)
    torch.cuda.synchronize()
    n = b.opt._groups[0].numel
    assert b.opt.device_noise_offset() == 2 * ((n + 3) // 4)
    it.run(4)
    torch.cuda.synchronize()
    assert b.opt.device_noise_offset() == 6 * ((n + 3) // 4) and b.opt.device_step_count() == 6
    _params_equal(a, b)
    _same_sgld(a, b)


# ------------------------------------------------------------------------------------------ grouped == solo
def _group_nets(dev, B):
    nets = []
    for b in range(B):
        torch.manual_seed(30 + b)
        nets.append(_small().to(dev))
    return nets


def test_grouped_fits_equal_their_solo_fits(dev):
    """B = 3, a noise-level sweep with seeds of its own, 2 eager iterations + 1 warm-up + 3 replays of the ONE hipGraph: every
    instance is its solo NativeIteration fit."""
    from dip_group import GroupedFits
    from dip_optim import FusedAdam, GraphedIteration, NativeIteration
    from utils.common_utils import get_params
    from utils.loss_head import MSEHead
    from utils.reg_noise import RegNoise
    B, iters = 3, 6
    stds, pseeds, seeds = [0.01, 0.0, 0.03], [11, 2 ** 64 - 1, 2 ** 32 + 7], [40, 41, 42]
    zs, ts, _ = _problem("skip3", HW, B, 0, dev)
    nets = _group_nets(dev, B)
    refs = [copy.deepcopy(n) for n in nets]
    solo = []
    for b, ref in enumerate(refs):
        opt = FusedAdam(get_params("net", ref, zs[b]), lr=0.01, weight_decay=WD, noise_std=stds[b], noise_seed=pseeds[b])
        it = NativeIteration(ref, MSEHead(ref, ts[b]), opt, zs[b], reg_noise=RegNoise(zs[b], 1. / 30., seed=seeds[b]))
        solo.append((opt, it.run(iters)))
    torch.cuda.synchronize()
    g = GroupedFits(nets, zs, ts, reg_noise_std=1. / 30., seeds=seeds, lr=0.01, weight_decay=WD, param_noise_std=stds,
                    param_noise_seeds=pseeds)
    assert g.pointers_outside_row0() == [] and list(g._row0_extra)[-2:] == ["sgld", "sgld_ranges"]
    g.step(2)
    it = GraphedIteration.group(g, warmup=1)
    it.run(3)
    torch.cuda.synchronize()
    assert g.step_counts() == [iters] * B
    n = solo[0][0]._groups[0].numel
    assert g._sgld_n == n and g._sgld_ranges == solo[0][0]._groups[0].ranges
    assert g.param_noise_offsets() == [iters * ((n + 3) // 4)] * B == [opt.device_noise_offset() for opt, _ in solo]
    for b in range(B):
        assert g.losses[b].item() == solo[b][1][-1].item(), b
        for (k, pa), pb in zip(nets[b].named_parameters(), refs[b].parameters()):
            assert torch.equal(pa, pb), (b, k)
        for (k, ba), bb in zip(nets[b].named_buffers(), refs[b].buffers()):
            assert torch.equal(ba, bb), (b, k)


def test_grouped_setter_and_explicit_zeros(dev):
    """set_param_noise_std between runs equals the solo setter; a group built with explicit zeros is the group built without
    the keywords (the parent's launch list), bit for bit."""
    from dip_group import GroupedFits
    from dip_optim import FusedAdam, NativeIteration
    from utils.common_utils import get_params
    from utils.loss_head import MSEHead
    from utils.reg_noise import RegNoise
    B = 3
    zs, ts, _ = _problem("skip3", HW, B, 0, dev)
    res = []
    for kw in ({}, dict(weight_decay=0.0, param_noise_std=[0.0] * B)):
        nets = _group_nets(dev, B)
        g = GroupedFits(nets, zs, ts, reg_noise_std=1. / 30., seeds=[1, 2, 3], **kw)
        assert not g.sgld and "sgld" not in g._row0_extra
        g.step(3)
        torch.cuda.synchronize()
        res.append((g.losses.clone(), [p.detach().clone() for n in nets for p in n.parameters()], g.stride))
    assert torch.equal(res[0][0], res[1][0]) and res[0][2] == res[1][2]
    assert all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1]))
    # the setter
    nets = _group_nets(dev, B)
    refs = [copy.deepcopy(n) for n in nets]
    g = GroupedFits(nets, zs, ts, reg_noise_std=1. / 30., seeds=[1, 2, 3], param_noise_std=0.01)
    g.step(2)
    g.set_param_noise_std([0.0, 0.02, 0.05])
    g.step(2)
    for b, ref in enumerate(refs):
        opt = FusedAdam(get_params("net", ref, zs[b]), lr=0.01, noise_std=0.01, noise_seed=[1, 2, 3][b])
        it = NativeIteration(ref, MSEHead(ref, ts[b]), opt, zs[b], reg_noise=RegNoise(zs[b], 1. / 30., seed=[1, 2, 3][b]))
        it.run(2)
        opt.set_noise_std([0.0, 0.02, 0.05][b])
        it.run(2)
    torch.cuda.synchronize()
    for b in range(B):
        for (k, pa), pb in zip(nets[b].named_parameters(), refs[b].parameters()):
            assert torch.equal(pa, pb), (b, k)
