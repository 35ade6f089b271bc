"""CPU suite of the ResNet backbone: the import cell of the reference's inpainting / restoration notebooks, the module tree
against the reference's state_dict (fixtures of tools/make_resnet_golden.py), the CPU truth tests/resnet_oracle.py against the
fixtures, loud failure off the MI355X path, and the launch list planned on host memory."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import resnet_oracle as RO

FIXTURES = ("a", "b", "nores")
ACTS = {"LeakyReLU": "LeakyReLU", "ReLU": torch.nn.ReLU}


def _load(name):
    g = np.load(os.path.join(GOLDEN, f"resnet_tiny_{name}.npz"))
    meta = json.loads(str(g["meta"]))
    return g, meta, ACTS[meta["act_fun"]]


def test_notebook_import_cell_and_factories():
    """`from models.resnet import ResNet` / `from models.unet import UNet` head inpainting.ipynb and restoration.ipynb."""
    from models.resnet import ResNet, ResidualSequential, get_block  # noqa: F401
    from models.unet import UNet
    from models import get_net
    with pytest.raises(NotImplementedError, match="no gfx950 path"):
        UNet()
    with pytest.raises(NotImplementedError, match="UNet"):
        UNet(num_input_channels=1, num_output_channels=3, feature_scale=8, more_layers=1, concat_x=False, upsample_mode='deconv',
             pad='zero', norm_layer=torch.nn.InstanceNorm2d, need_sigmoid=True, need_bias=True)
    with pytest.raises(NotImplementedError):            # get_net stays as it is: the reference's own 'ResNet' line is broken
        get_net(3, 'ResNet', 'reflection', 'bilinear')
    assert len(get_block(8, torch.nn.BatchNorm2d, 'LeakyReLU')) == 5


@pytest.mark.parametrize("name", FIXTURES)
def test_state_dict_matches_reference_bitwise(name):
    from models.resnet import ResNet
    g, meta, act = _load(name)
    torch.manual_seed(meta["seed"])
    net = ResNet(*meta["args"], act_fun=act, **meta["kw"])
    sd = net.state_dict()
    keys = [k[4:] for k in g.files if k.startswith("sd0/")]
    assert list(sd.keys()) == keys
    for k in keys:
        assert tuple(sd[k].shape) == g["sd0/" + k].shape, k
        assert np.array_equal(sd[k].numpy(), g["sd0/" + k]), k          # same construction order -> same RNG stream
    assert sum(p.numel() for p in net.parameters()) == meta["n_params"]
    spec = RO.ResNetSpec(*meta["args"], act_fun=act, **meta["kw"])
    assert spec.param_names() == [k for k, _ in net.named_parameters()]
    # need_sigmoid=False still ends in Sigmoid: the tree the reference really builds
    tail = list(ResNet(*meta["args"], need_sigmoid=False).model._modules.values())[-1]
    assert isinstance(tail, torch.nn.Sigmoid)


def test_notebook_resnet_parameter_count():
    from models.resnet import ResNet
    _, meta, _ = _load("a")
    n = sum(p.numel() for p in ResNet(1, 3, 8, 32, need_sigmoid=True, act_fun='LeakyReLU').parameters())
    assert n == meta["n_params_resnet_1_3_8_32"] == 158979


@pytest.mark.parametrize("name", FIXTURES)
def test_cpu_oracle_reproduces_fixture_bitwise(name):
    """tests/resnet_oracle.py in fp32 against the reference's recorded output, loss and gradients: BITWISE -- its op
    sequence is torch's own (F.pad / F.conv2d / F.batch_norm / activation / + / sigmoid, in the module tree's order), so
    the same ATen kernels run on the same values in the same order (same thread cap: conftest's 16)."""
    g, meta, act = _load(name)
    spec = RO.ResNetSpec(*meta["args"], act_fun=act, **meta["kw"])
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/")}
    z, t, m = (torch.from_numpy(g[k]) for k in ("z", "target", "mask"))
    lf = lambda o, dt: torch.nn.functional.mse_loss(o * m.to(dt), t.to(dt) * m.to(dt))
    out, loss, grads = RO.grads(spec, sd, z, lf, torch.float32)
    assert np.array_equal(out.numpy(), g["out"])
    assert loss == float(g["loss"])
    for k, v in grads.items():
        assert np.array_equal(v.numpy(), g["grad/" + k]), k
    # the eager definition kept in the parameter-holder modules says the same (ResidualSequential.forward)
    from models.resnet import ResNet
    net = ResNet(*meta["args"], act_fun=act, **meta["kw"])
    net.load_state_dict(sd)
    assert np.array_equal(net.model(z).detach().numpy(), g["out"])
    # imposed branch pattern == own pattern -> same fp64 gradients; pre-activations are recorded
    zrec = {}
    _, _, g64 = RO.grads(spec, sd, z, lf, torch.float64, zrec=zrec)
    _, _, g64m = RO.grads(spec, sd, z, lf, torch.float64, masks={k: v > 0 for k, v in zrec.items()})
    assert set(zrec) == {"model.0"} | {spec.block(k)[1] for k in range(spec.num_blocks)}
    for k in g64:
        assert torch.allclose(g64[k], g64m[k], rtol=1e-12, atol=1e-18), k


def test_no_cpu_fallback_and_unsupported_options():
    from models.resnet import ResNet
    net = ResNet(1, 3, 2, 8)
    with pytest.raises(RuntimeError, match="MI355X"):
        net(torch.zeros(1, 1, 16, 16))
    for kw in (dict(act_fun=torch.nn.Tanh), dict(act_fun='Tanh'), dict(norm_layer=torch.nn.InstanceNorm2d),
               dict(pad='replication')):
        bad = ResNet(1, 3, 1, 8, **kw) if kw.get("act_fun") != 'Tanh' else None
        if bad is None:          # an unknown activation STRING fails in act(), at construction, as in the reference
            with pytest.raises(AssertionError):
                ResNet(1, 3, 1, 8, **kw)
            continue
        with pytest.raises(NotImplementedError):
            bad(torch.zeros(1, 1, 16, 16))
    with pytest.raises(NotImplementedError, match="multiples of 4"):
        ResNet(1, 3, 1, 6)(torch.zeros(1, 1, 16, 16))
    with pytest.raises(NotImplementedError, match="eval-mode"):
        net.eval()
    assert net.training


def test_resnet_launch_list_planned_on_host_memory(built):
    """The planner runs on host memory (nothing can be launched): one res_join_fwd and one res_join_bwd per block, no
    accumulating data gradient, every weight gradient on the list."""
    from models.resnet import ResNet
    import dip_engine
    net = ResNet(1, 3, 2, 8)
    eng = net.__dict__["_dip_engine"]
    assert isinstance(eng, dip_engine.ResNetEngine) and eng.kind == "resnet"
    assert len(eng.convs) == 7 and len(eng.bns) == 5
    eng._build_arenas(torch.device("cpu"))
    assert eng._arena_ok()
    for H, W in ((32, 48), (448, 704)):
        eng._build_plan(H, W, 1)
        fwd, bwd = [n for _, _, n in eng.fwd_ops], [n for _, _, n in eng.bwd_ops]
        assert [n for n in fwd if n.startswith("res_join")] == ["res_join_fwd:b0", "res_join_fwd:b1"]
        assert [n for n in bwd if n.startswith("res_join")] == ["res_join_bwd:b1", "res_join_bwd:b0"]
        assert not any(n.startswith("dgrad+:") for n in fwd + bwd)
        assert sum(n.startswith("wgrad:") for n in bwd) == 7
        assert [n for _, _, n in eng.bwd_input_ops][0] == "dgrad:first"
        assert bwd.index("res_join_bwd:b0") < bwd.index("wgrad:first")
    # at full resolution the chain convs are conv_thin launches (plain stores), forward and data gradient
    thin = [n for fn, a, n in eng.fwd_ops + eng.bwd_ops if fn is built.dip_conv_igemm and built.dip_conv_thin_eligible(a[0])]
    assert {"conv_fwd:b0.conv1", "conv_fwd:b1.conv2", "conv_fwd:tail", "dgrad:b0.conv1", "dgrad:b1.conv2", "dgrad:tail"} <= set(thin)
    # need_residual=False: no join, the activation derivative at the bottom is a launch of its own
    e2 = ResNet(1, 3, 2, 8, need_residual=False).__dict__["_dip_engine"]
    e2._build_arenas(torch.device("cpu"))
    e2._build_plan(32, 48, 1)
    names = [n for _, _, n in e2.fwd_ops + e2.bwd_ops]
    assert not any(n.startswith("res_join") for n in names) and "act_bwd:first" in names
    # the two new entry points are command-list entry points
    assert built.dip_list_fn_id(b"dip_res_join_fwd") >= 0 and built.dip_list_fn_id(b"dip_res_join_bwd") >= 0

