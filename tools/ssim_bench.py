"""What NativeIteration(ssim=SSIMMonitor(...)) costs per iteration, in one process on one card.

    python tools/ssim_bench.py [--size 512] [--blocks 5] [--iters 60] [--out profiles/ssim_bench.json]
    rocprofv3 --kernel-trace --stats -d <dir> -o ssim -- python tools/ssim_bench.py --trace 100       # kernel times, a run of
                                                                                                      # its own, no counters

bench.py's `default` net at size x size, reg-noise 1/30, Adam at LR 0.01, two fits from one seed: NativeIteration(ssim=None) and
ssim=SSIMMonitor(img_gt).  After the warm-up the legs alternate in blocks, A B A B ...: a block's wall time runs from its first
call until the closing synchronize() returns; medians, minima and maxima over the blocks.  The two fits must hold bit-identical
parameters at the end (the monitor does not touch the fit).  --trace N issues N iterations of the monitored leg and nothing else,
for a profiler that lists the kernels; --avg adds a FitMonitor and records ssim_sm of its out_avg too (two sources per launch)."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def _fit(dev, size, with_ssim, with_avg, capacity):
    import torch
    import bench
    from dip_optim import FusedAdam, NativeIteration
    from utils.common_utils import get_params
    from utils.fit_monitor import FitMonitor, SSIMMonitor
    from utils.loss_head import MSEHead
    from utils.reg_noise import RegNoise
    torch.manual_seed(0)
    net, depth = bench.build_net("default")
    z, img = bench.make_problem(0, (size, size), depth)
    f = SimpleNamespace(net=net.to(dev), z=z.to(dev), img=img.to(dev))
    gt = (f.img * 0.9 + 0.05).contiguous()                  # any image of the output's shape: the cost does not depend on it
    f.reg = RegNoise(f.z, 1 / 30, seed=1234)
    f.opt = FusedAdam(get_params('net', f.net, f.z), lr=0.01)
    f.head = MSEHead(f.net, f.img)
    f.mon = FitMonitor(f.net, f.img, gt, backtracking=False, capacity=capacity) if with_avg else None
    f.sm = SSIMMonitor(gt, img_avg=None if f.mon is None else f.mon.out_avg, capacity=capacity) if with_ssim else None
    f.it = NativeIteration(f.net, f.head, f.opt, f.z, reg_noise=f.reg, monitor=f.mon, ssim=f.sm)
    f.run = f.it.run
    return f


def _stats(v, nd=4):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd),
            "blocks": [round(x, nd) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--avg", action="store_true", help="a FitMonitor next to it, and ssim_sm of its out_avg")
    ap.add_argument("--trace", type=int, default=0, help="issue this many monitored iterations and nothing else")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_bench.json"))
    args = ap.parse_args()
    import torch          # before the library: libdip_hip.so must bind to the HIP runtime torch has loaded
    ge.build()
    import dip_native
    assert torch.cuda.is_available(), "ssim_bench.py needs an MI355X"
    dev = torch.device("cuda:0")
    if args.trace:
        f = _fit(dev, args.size, True, args.avg, args.trace)
        f.run(args.trace)
        torch.cuda.synchronize()
        print(json.dumps({"traced_iterations": args.trace, "last_record": f.sm.last()}))
        return
    capacity = args.warmup + args.blocks * args.iters
    legs = {"plain": _fit(dev, args.size, False, args.avg, capacity), "ssim": _fit(dev, args.size, True, args.avg, capacity)}
    for f in legs.values():
        f.run(args.warmup)
    torch.cuda.synchronize()
    wall = {k: [] for k in legs}
    for _ in range(args.blocks):
        for name, f in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f.run(args.iters)
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) / args.iters * 1e3)
    same = all(torch.equal(p, q) for p, q in zip(legs["plain"].net.parameters(), legs["ssim"].net.parameters()))
    med = {k: statistics.median(v) for k, v in wall.items()}
    rec = {"tool": "tools/ssim_bench.py", "net": "default", "HW": [args.size, args.size], "with_avg": args.avg,
           "blocks": args.blocks, "iters_per_block": args.iters, "warmup": args.warmup,
           "wall_ms_per_iteration": {k: _stats(v) for k, v in wall.items()},
           "added_us_per_iteration_median": round((med["ssim"] - med["plain"]) * 1e3, 2),
           "added_us_per_iteration_by_block": [round((y - x) * 1e3, 2) for x, y in zip(wall["plain"], wall["ssim"])],
           "last_record": legs["ssim"].sm.last(), "bit_identical_parameters": bool(same),
           "device": torch.cuda.get_device_name(0), "build_id": dip_native.lib().dip_build_id().decode()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))
    if not same:
        raise SystemExit("the monitored fit diverged from the plain one")


if __name__ == "__main__":
    main()
