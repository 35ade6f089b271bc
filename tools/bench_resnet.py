"""The inpainting notebook's ResNet arm as a benchmark: ResNet(1, 3, 8, 32, need_sigmoid=True, act_fun='LeakyReLU') at
448 x 704, masked MSE, Adam (LR 0.001), no parameter noise -- the native engine against torch-ROCm eager on the same card
in the same call.

    python tools/bench_resnet.py [--steps K] [--warmup W] [--pairs P] [--size H W] [--native-only]

The yard-stick is the identical module tree run by stock torch.nn modules on the device (`net.model(x)`: the parameter
holders of models/resnet.py ARE stock modules, and ResidualSequential.forward is the eager `out + x`), stepped by
torch.optim.Adam.  The two are timed interleaved, A B A B ..., each leg = W warm-up iterations, then K timed iterations
between two synchronisations (the shape of bench.py's timed region); medians over the legs.  One JSON line.
Per-kernel-family times come from a separate run under a kernel-trace profiler with --native-only.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--size", type=int, nargs=2, default=(448, 704))
    ap.add_argument("--native-only", action="store_true")
    args = ap.parse_args()
    import torch          # before the library: libdip_hip.so must bind to the HIP runtime torch has loaded
    ge.build()
    from models.resnet import ResNet
    from utils.common_utils import get_noise, get_params
    from dip_optim import FusedAdam
    assert torch.cuda.is_available(), "bench_resnet.py needs an MI355X"
    dev = torch.device("cuda:0")
    H, W = args.size
    torch.manual_seed(0)
    img = torch.nn.functional.avg_pool2d(torch.rand(1, 3, H + 4, W + 4), 5, stride=1).to(dev)
    mask = (torch.rand(1, 1, H, W) > 0.3).float().to(dev)
    z = get_noise(1, 'noise', (H, W)).to(dev)
    mse = torch.nn.MSELoss()

    def make(native):
        torch.manual_seed(1)
        net = ResNet(1, 3, 8, 32, need_sigmoid=True, act_fun='LeakyReLU').to(dev)
        fwd = net if native else net.model              # eager: the stock nn.Module tree itself
        opt = FusedAdam(get_params('net', net, z), lr=0.001) if native else torch.optim.Adam(net.parameters(), lr=0.001)
        last = {}

        def step():
            opt.zero_grad()
            loss = mse(fwd(z) * mask, img * mask)
            loss.backward()
            opt.step()
            last["loss"] = loss.detach()
        return net, step, last

    def leg(step):
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps

    net_n, step_n, last_n = make(True)
    legs = {"native": [], "eager": []}
    if args.native_only:
        legs["native"] = [leg(step_n) for _ in range(args.pairs)]
    else:
        net_e, step_e, last_e = make(False)
        for _ in range(args.pairs):                      # A B A B ...
            legs["native"].append(leg(step_n))
            legs["eager"].append(leg(step_e))
    eng = net_n.__dict__["_dip_engine"]
    res = {"bench": "resnet_1_3_8_32", "size": [H, W], "steps": args.steps, "warmup": args.warmup, "pairs": args.pairs,
           "device": torch.cuda.get_device_name(0), "build": eng.lib.dip_build_id().decode(),
           # the two launch lists; around them per iteration: weight repack(s), input layout, head forward / backward, Adam
           "list_launches_per_iter": len(eng.fwd_ops) + len(eng.bwd_ops),
           "native_ms": [round(1e3 * t, 4) for t in legs["native"]],
           "native_ms_median": round(1e3 * statistics.median(legs["native"]), 4),
           "native_it_s": round(1.0 / statistics.median(legs["native"]), 2),
           "native_loss": float(last_n["loss"])}
    if legs["eager"]:
        me, mn = statistics.median(legs["eager"]), statistics.median(legs["native"])
        spread = max(max(v) / min(v) - 1.0 for v in legs.values())
        res.update({"eager_ms": [round(1e3 * t, 4) for t in legs["eager"]], "eager_ms_median": round(1e3 * me, 4),
                    "eager_it_s": round(1.0 / me, 2), "eager_loss": float(last_e["loss"]),
                    "native_over_eager_it_s": round(me / mn, 4), "pair_spread": round(spread, 4)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
