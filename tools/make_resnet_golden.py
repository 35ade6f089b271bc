"""Writes tests/golden/resnet_tiny_*.npz from the REAL reference (build container only; the reference checkout is imported
read-only through oracle/_refload.py, as oracle/make_golden.py does for the skip nets; nothing of it is copied).

Layout (that of net_tiny_*.npz):  sd/<key> state_dict the vectors were made with, z, target, mask, out, loss, grad/<key>,
adam1/<key>, adam3/<key> (parameters after 1 and 3 optimize('adam') iterations, lr 0.01), out_after3; plus
  sd0/<key>   the state_dict right after `torch.manual_seed(seed)` construction (sd/ differs from it in the BatchNorm affine
              parameters only, which are drawn non-degenerate afterwards, as for the skip-net fixtures),
  meta        JSON: constructor arguments, seed, size, and the parameter count of the notebook's ResNet(1, 3, 8, 32).

It then checks the fixture as a yard-stick (tests/parity.py): the reference's own fp32 gradients against the fp64 truth of
tests/resnet_oracle.py, and the fp32-vs-fp64 LeakyReLU branch mismatches against MASK_FRAC.

    python tools/make_resnet_golden.py
"""
import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import _refload  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")

ACTS = {"LeakyReLU": "LeakyReLU", "ReLU": torch.nn.ReLU}
CASES = {
    "a": dict(args=(1, 3, 2, 8), kw=dict(pad="reflection"), act="LeakyReLU", hw=(32, 48), seed=31),
    "b": dict(args=(4, 3, 3, 16), kw=dict(pad="zero"), act="ReLU", hw=(40, 40), seed=32),
    "nores": dict(args=(1, 3, 2, 8), kw=dict(need_residual=False, pad="reflection"), act="LeakyReLU", hw=(32, 48), seed=33),
}


def gen(name, cfg, n_notebook):
    rm = _refload.load_ref_models()
    cu = _refload.load_ref_common_utils()
    ResNet = __import__("ref_models.resnet", fromlist=["ResNet"]).ResNet
    torch.manual_seed(cfg["seed"])
    net = ResNet(*cfg["args"], act_fun=ACTS[cfg["act"]], **cfg["kw"])
    rec = {}
    for k, v in net.state_dict().items():
        rec["sd0/" + k] = v.detach().numpy().copy()
    with torch.no_grad():                       # non-degenerate BatchNorm affine parameters (oracle/make_golden.py:133-141)
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0.0, 0.3)
    H, W = cfg["hw"]
    cin, cout = cfg["args"][:2]
    z = cu.get_noise(cin, "noise", (H, W)).float()          # uniform x 0.1: BatchNorm sees the notebook's scale
    target = torch.rand(1, cout, H, W)
    mask = (torch.rand(1, 1, H, W) > 0.3).float()
    rec.update({"z": z.numpy(), "target": target.numpy(), "mask": mask.numpy()})
    for k, v in net.state_dict().items():
        rec["sd/" + k] = v.detach().numpy().copy()
    out = net(z)
    loss = torch.nn.functional.mse_loss(out * mask, target * mask)
    loss.backward()
    rec["out"] = out.detach().numpy().copy()
    rec["loss"] = np.array(loss.item(), dtype=np.float64)
    for k, p in net.named_parameters():
        rec["grad/" + k] = p.grad.numpy().copy()
    for p in net.parameters():
        p.grad = None
    mse = torch.nn.MSELoss()
    for nsteps in (1, 3):
        net2 = copy.deepcopy(net)

        def closure2():
            o = net2(z)
            l = mse(o * mask, target * mask)
            l.backward()
            return l

        cu.optimize("adam", cu.get_params("net", net2, z), closure2, 0.01, nsteps)
        for k, p in net2.named_parameters():
            rec[f"adam{nsteps}/" + k] = p.detach().numpy().copy()
        if nsteps == 3:
            rec["out_after3"] = net2(z).detach().numpy().copy()
    meta = dict(args=list(cfg["args"]), kw=cfg["kw"], act_fun=cfg["act"], hw=list(cfg["hw"]), seed=cfg["seed"],
                n_params=sum(p.numel() for p in net.parameters()), n_params_resnet_1_3_8_32=n_notebook)
    rec["meta"] = np.array(json.dumps(meta))
    path = os.path.join(OUT, f"resnet_tiny_{name}.npz")
    np.savez_compressed(path, **rec)
    print(f"resnet_tiny_{name}.npz: {sum(v.size for v in rec.values())} values, {os.path.getsize(path)} bytes")
    check(name, cfg, rec)


def check(name, cfg, rec):
    """The fixture as a yard-stick: the reference's fp32 gradients meet tests/parity.py against the fp64 truth, and the
    fp32 / fp64 branch patterns differ on fewer than MASK_FRAC of the activated elements."""
    import parity as PT
    import resnet_oracle as RO
    spec = RO.ResNetSpec(*cfg["args"], act_fun=ACTS[cfg["act"]], **cfg["kw"])
    sd = {k[3:]: torch.from_numpy(v) for k, v in rec.items() if k.startswith("sd/")}
    z, t, m = (torch.from_numpy(rec[k]) for k in ("z", "target", "mask"))
    lf = lambda o, dt: torch.nn.functional.mse_loss(o * m.to(dt), t.to(dt) * m.to(dt))
    z32, z64 = {}, {}
    o32, l32, g32 = RO.grads(spec, sd, z, lf, torch.float32, zrec=z32)
    _, l64, g64n = RO.grads(spec, sd, z, lf, torch.float64, zrec=z64)
    bit = all(torch.equal(g32[k], torch.from_numpy(rec["grad/" + k])) for k in g32) and \
        torch.equal(o32, torch.from_numpy(rec["out"]))
    masks32 = {k: v > 0 for k, v in z32.items()}
    _, _, g64 = RO.grads(spec, sd, z, lf, torch.float64, masks=masks32)
    ref = {k: torch.from_numpy(rec["grad/" + k]) for k in g32}
    rep = PT.grad_report(ref, g64, ref, g64n, spec.zero_grad_keys())
    mrep = PT.mask_report(masks32, z64)
    PT.check(rep, mrep)
    gn = {k: float(v.norm()) for k, v in g64n.items()}
    zk = next(iter(spec.zero_grad_keys()))
    print(f"  {name}: fp32 restatement bitwise == reference: {bit}; loss fp32 {l32:.9g} fp64 {l64:.9g}; {PT.fmt(rep)}; "
          f"{PT.fmt_masks(mrep)}; |g| zero tensor {gn[zk]:.1e}, others {min(v for k, v in gn.items() if k != zk):.1e} .. "
          f"{max(gn.values()):.1e}")


if __name__ == "__main__":
    assert _refload.available(), "the reference checkout is needed (DIP_REFERENCE)"
    _refload.load_ref_models()
    RN = __import__("ref_models.resnet", fromlist=["ResNet"]).ResNet
    n_notebook = sum(p.numel() for p in RN(1, 3, 8, 32, need_sigmoid=True, act_fun="LeakyReLU").parameters())
    for name, cfg in CASES.items():
        gen(name, cfg, n_notebook)
