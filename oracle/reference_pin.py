"""The bitwise pin of the oracle against the REAL reference, as stored digests (tests/golden/reference_pin.json).

verify_against_reference.py compares the two live, which needs a reference checkout next to the tests.  This module
runs the same comparison in two halves: `reference_digests()` (needs the checkout: oracle/_refload.py) records, for the
ten net configurations of verify_against_reference.CONFIGS plus the Downsampler and get_noise, the SHA-256 of every
float32 tensor the reference computes -- output, loss, every gradient, every parameter after one Adam step -- on
deterministic inputs; `oracle_digests()` computes the same digests from oracle/dip_oracle.py alone.  Equal digests =
bitwise-equal tensors.

  python oracle/reference_pin.py        (with the reference checkout: DIP_REFERENCE, default in _refload.py)
"""
import hashlib
import json
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dip_oracle as O  # noqa: E402
from verify_against_reference import CONFIGS, spec_from  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(HERE), "tests", "golden", "reference_pin.json")


def digest(t) -> str:
    a = t.detach().contiguous().cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()[:32]


def pin_inputs(name, cfg):
    """Weights (independent of either skip(): one seeded generator per parameter name), input and target."""
    spec = spec_from(cfg)
    weights = {}
    for k, shape in O.param_shapes(spec).items():
        g = torch.Generator().manual_seed(zlib.crc32(f"{name}/{k}".encode()))
        fan = max(1, int(np.prod(shape[1:]))) if len(shape) > 1 else 4
        weights[k] = (torch.rand(shape, generator=g) * 2 - 1) / fan ** 0.5
    H, W = cfg["hw"]
    torch.manual_seed(zlib.crc32(name.encode()))
    x = O.get_noise(cfg["args"][0], "noise", (H, W)) if cfg["args"][0] != 2 else O.get_noise(2, "meshgrid", (H, W)).float()
    return spec, weights, x


def _target(name, shape):
    return torch.rand(shape, generator=torch.Generator().manual_seed(zlib.crc32(("target/" + name).encode())))


def _net_digests(name, out, loss, named_grads, step, named_params):
    d = {"out": digest(out), "loss": float(loss).hex(), "grad": {k: digest(g) for k, g in named_grads}}
    step()
    d["adam1"] = {k: digest(p) for k, p in named_params()}
    return d


def oracle_digests():
    res = {"nets": {}}
    for name, cfg in CONFIGS.items():
        spec, weights, x = pin_inputs(name, cfg)
        onet = O.OracleNet(spec, {k: v.clone() for k, v in weights.items()})
        out = onet(x)
        loss = torch.nn.functional.mse_loss(out, _target(name, out.shape))
        loss.backward()
        opt = torch.optim.Adam(onet.params, lr=0.01)
        res["nets"][name] = _net_digests(name, out, loss.item(), [(k, p.grad) for k, p in zip(onet.names, onet.params)],
                                         opt.step, lambda: zip(onet.names, onet.params))
    res["downsampler"] = {}
    for factor, kt in ((4, "lanczos2"), (2, "lanczos2"), (4, "lanczos3")):
        sup = {"lanczos2": 2, "lanczos3": 3}[kt]
        x = torch.rand((1, 3, 64, 96), generator=torch.Generator().manual_seed(factor * 10 + sup))
        res["downsampler"][f"{kt}_f{factor}"] = {"kernel": digest(O.lanczos_kernel(factor, 0.5, 2 * sup * factor + 1, sup)),
                                                  "y": digest(O.downsampler_forward(x, factor, kt, 0.5, True))}
    torch.manual_seed(3)
    res["get_noise"] = {"noise": digest(O.get_noise(32, "noise", (16, 24))), "meshgrid": digest(O.get_noise(2, "meshgrid", (8, 12)))}
    return res


def reference_digests():
    import _refload
    assert _refload.available(), "reference checkout not found"
    rm = _refload.load_ref_models()
    cu = _refload.load_ref_common_utils()
    res = {"nets": {}}
    for name, cfg in CONFIGS.items():
        spec, weights, x = pin_inputs(name, cfg)
        net = rm.skip(*cfg["args"], **cfg["kw"])
        missing, unexpected = net.load_state_dict(weights, strict=False)
        assert not unexpected and all(k.endswith(("running_mean", "running_var", "num_batches_tracked")) for k in missing)
        out = net(x)
        loss = torch.nn.functional.mse_loss(out, _target(name, out.shape))
        loss.backward()
        opt = torch.optim.Adam(net.parameters(), lr=0.01)
        names = list(O.param_shapes(spec))
        by = dict(net.named_parameters())
        res["nets"][name] = _net_digests(name, out, loss.item(), [(k, by[k].grad) for k in names], opt.step,
                                         lambda: [(k, by[k]) for k in names])
    res["downsampler"] = {}
    for factor, kt in ((4, "lanczos2"), (2, "lanczos2"), (4, "lanczos3")):
        sup = {"lanczos2": 2, "lanczos3": 3}[kt]
        x = torch.rand((1, 3, 64, 96), generator=torch.Generator().manual_seed(factor * 10 + sup))
        d = rm.downsampler.Downsampler(n_planes=3, factor=factor, kernel_type=kt, phase=0.5, preserve_size=True)
        res["downsampler"][f"{kt}_f{factor}"] = {"kernel": digest(d.kernel), "y": digest(d(x))}
    torch.manual_seed(3)
    res["get_noise"] = {"noise": digest(cu.get_noise(32, "noise", (16, 24))), "meshgrid": digest(cu.get_noise(2, "meshgrid", (8, 12)))}
    return res


if __name__ == "__main__":
    torch.set_num_threads(1)
    ref = reference_digests()
    assert oracle_digests() == ref, "the oracle is not bitwise equal to the reference on these inputs"
    ref["source"] = ("the real reference on torch CPU fp32 (1 thread), oracle/reference_pin.py; torch " + torch.__version__)
    with open(GOLDEN, "w") as f:
        json.dump(ref, f, indent=1, sort_keys=True)
    print(f"wrote {GOLDEN}: {len(ref['nets'])} nets, oracle bitwise equal")
