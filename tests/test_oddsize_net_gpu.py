"""128-channel nets at ODD sizes against the CPU oracle on a real MI355X: one forward / backward through
test_fullsize_gpu._iter1 (oracle in fp32, fp64 and fp64 on the HIP branch pattern; the thresholds of tests/parity.py).  The
odd-size nets of test_net_gpu.py (tiny_ragged*, tiny_poolcrop, tiny_noskipcrop) have 16..32 channels at ~37 x 50 and stay on
dip_conv_small and the thin paths; here the LDS-DMA strided forward, the phase-mode data gradient, wgrad_bf3, conv_bf3,
conv_thin4 and the ring data gradient run together on a size where every scale but one is odd in both dimensions:

  * the default skip net (denoising.ipynb:160-165 of the reference) at 161 x 241: 161x241 -> 81x121 -> 41x61 -> 21x31 ->
    11x16 -> 6x8; every Concat drops the last up-sampled row and / or column;
  * the kate net (inpainting.ipynb:203-209: skip = 128, nearest) at 97 x 131: 128-channel skip concats at odd sizes.

The launch lists are inspected BEFORE the run (`net_routing`, on a dry plan of the same net) so that a change of the routing
can not leave the test hollow, and on the engine that ran."""
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import dip_native as N  # noqa: E402
import dip_oracle as O  # noqa: E402
from test_fullsize_gpu import _iter1  # noqa: E402


def _default():
    from models import get_net
    return get_net(32, "skip", "reflection", skip_n33d=128, skip_n33u=128, skip_n11=4, num_scales=5, upsample_mode="bilinear"), \
        O.default_spec()


def _kate():
    from models.skip import skip
    net = skip(32, 3, num_channels_down=[128] * 5, num_channels_up=[128] * 5, num_channels_skip=[128] * 5,
               filter_size_up=3, filter_size_down=3, upsample_mode="nearest", filter_skip_size=1,
               need_sigmoid=True, need_bias=True, pad="reflection", act_fun="LeakyReLU")
    return net, O.SkipSpec(32, 3, [128] * 5, [128] * 5, [128] * 5, pad="reflection", upsample_mode="nearest")


NETS = {
    # name: (constructor, H, W, seed, what net_routing must find at least once)
    "default_161x241": (_default, 161, 241, 0, ("v5_odd", "phase", "wgrad_bf3", "v7", "upcat_odd")),
    # (49 x 66 and below: the strided convs of this size are dip_conv_small's, the stride-1 top scale is the bf16 pipe's)
    "kate_97x131": (_kate, 97, 131, 2, ("v7", "upcat_odd", "skip128_odd")),
}


def net_routing(eng):
    """Counts over the engine's launch lists: variant-5 strided forwards on an odd input, phase-mode data gradients, bf16-pipe
    weight gradients, variant-7 convs, concats at an odd size (and those with a 128-channel skip branch)."""
    lib = eng.lib
    r = dict(v5_odd=0, phase=0, wgrad_bf3=0, v7=0, upcat_odd=0, skip128_odd=0)
    for fn, args, name in list(eng.fwd_ops) + list(eng.bwd_ops):
        d = getattr(args[0], "_obj", None) if args else None
        if fn is lib.dip_conv_igemm and isinstance(d, N.DipConvDesc):
            v = lib.dip_conv_variant(args[0])
            r["v5_odd"] += int(v == 5 and (d.Hin % 2 == 1 or d.Win % 2 == 1))
            r["phase"] += int(v == 4 and d.dil == 2)
            r["v7"] += int(v == 7)
        elif fn is lib.dip_conv_wgrad and isinstance(d, N.DipWgradDesc):
            r["wgrad_bf3"] += int(lib.dip_wgrad_bf3_eligible(args[0]))
        elif fn in (lib.dip_upcat_fwd, lib.dip_upcat_fwd_fin) and isinstance(d, N.DipUpcatDesc):
            odd = d.H % 2 == 1 or d.W % 2 == 1
            r["upcat_odd"] += int(odd)
            r["skip128_odd"] += int(odd and d.ns == 128)
    return r


def dry_plan(make, Hh, Ww):
    """Both planner passes of a fresh instance of the net on CPU memory (nothing is launched)."""
    net, _ = make()
    eng = net.__dict__["_dip_engine"]
    eng._build_arenas(torch.device("cpu"))
    eng._build_plan(Hh, Ww, 32)
    return eng


@pytest.mark.parametrize("name", list(NETS))
def test_odd_size_net_iter1_vs_oracle(dev, name):
    make, Hh, Ww, seed, need = NETS[name]
    from utils.common_utils import get_noise
    planned = net_routing(dry_plan(make, Hh, Ww))
    assert all(planned[k] >= 1 for k in need), (name, planned)
    torch.manual_seed(seed)
    net, spec = make()
    z = get_noise(32, "noise", (Hh, Ww))
    np.random.seed(seed)
    target = torch.from_numpy(np.random.rand(1, 3, Hh, Ww).astype(np.float32))
    tg = target.to(dev)
    t0 = time.time()
    net, out = _iter1(dev, net, spec, z, lambda o, dt: F.mse_loss(o, target.to(dt)), lambda o: F.mse_loss(o, tg),
                      f"{name} (odd size)")
    print(f"{name}: whole test body {time.time() - t0:.1f} s")
    assert tuple(out.shape) == (1, 3, Hh, Ww)
    ran = net_routing(net.__dict__["_dip_engine"])
    assert ran == planned, (ran, planned)
