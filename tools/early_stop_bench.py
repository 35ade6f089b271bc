"""What the device-side early-stopping criterion costs per iteration: NativeIteration(early_stop=EarlyStopMonitor(...)) against
the same fit with early_stop=None, in one process on one card.

    python tools/early_stop_bench.py [--size 512] [--window 100] [--blocks 7] [--iters 50] [--out profiles/early_stop_bench.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/early_stop_bench.py --trace 100        # kernel times, a run of its own

bench.py's `default` net at size x size, reg-noise 1/30, Adam at LR 0.01, two fits from one seed.  After the warm-up the two
legs alternate in blocks, A B A B ...: a block's wall time runs from its first call until the closing synchronize() returns;
medians, minima and maxima over the blocks.  The early_stop=None leg of the same call is the yard-stick.  The two fits must
hold bit-identical parameters at the end (the monitor does not touch the fit).  --trace N issues N monitored iterations and
nothing else, for a profiler that lists the kernels."""
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

ORDER = ("plain", "early_stop")


def _stats(v, nd=4):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd),
            "blocks": [round(x, nd) for x in v]}


def _fit(dev, size, monitored, window, patience, capacity):
    import torch
    import bench
    from dip_optim import FusedAdam, NativeIteration
    from utils.common_utils import get_params
    from utils.fit_monitor import EarlyStopMonitor
    from utils.loss_head import MSEHead
    from utils.reg_noise import RegNoise
    torch.manual_seed(0)
    net, depth = bench.build_net("default")
    z, img = bench.make_problem(0, (size, size), depth)
    f = SimpleNamespace(net=net.to(dev), z=z.to(dev), img=img.to(dev))
    f.reg = RegNoise(f.z, 1 / 30, seed=1234)
    f.opt = FusedAdam(get_params('net', f.net, f.z), lr=0.01)
    f.head = MSEHead(f.net, f.img)
    f.es = EarlyStopMonitor(f.img, window=window, patience=patience, net=f.net, capacity=capacity) if monitored else None
    f.it = NativeIteration(f.net, f.head, f.opt, f.z, reg_noise=f.reg, early_stop=f.es)
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--window", type=int, default=100)
    ap.add_argument("--patience", type=int, default=1000)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--trace", type=int, default=0, help="issue this many monitored iterations and nothing else")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "early_stop_bench.json"))
    args = ap.parse_args()
    if not args.trace and (args.blocks * args.iters < 300 or args.warmup < 3):
        ap.error("at least 300 iterations per leg after at least 3 warm-up iterations")
    import torch          # before the library: libdip_hip.so must bind to the HIP runtime torch has loaded
    ge.build()
    import dip_native
    assert torch.cuda.is_available(), "early_stop_bench.py needs an MI355X"
    dev = torch.device("cuda:0")
    if args.trace:
        f = _fit(dev, args.size, True, args.window, args.patience, args.trace)
        f.it.run(args.trace)
        torch.cuda.synchronize()
        print(json.dumps({"traced_iterations": args.trace, "last_record": f.es.last()}))
        return
    capacity = args.warmup + args.blocks * args.iters
    fits = {"plain": _fit(dev, args.size, False, args.window, args.patience, capacity),
            "early_stop": _fit(dev, args.size, True, args.window, args.patience, capacity)}
    for name in ORDER:
        fits[name].it.run(args.warmup)
    torch.cuda.synchronize()
    wall = {k: [] for k in ORDER}
    for _ in range(args.blocks):
        for name in ORDER:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fits[name].it.run(args.iters)
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) / args.iters * 1e3)
    a, b = fits["plain"], fits["early_stop"]
    same = all(torch.equal(p, q) for p, q in zip(a.net.parameters(), b.net.parameters()))
    n = b.img.numel()
    med = {k: statistics.median(wall[k]) for k in ORDER}
    rec = {"tool": "tools/early_stop_bench.py", "HW": [args.size, args.size], "n": n, "window": args.window,
           "patience": args.patience, "blocks": args.blocks, "iters_per_block": args.iters, "warmup": args.warmup,
           "order": list(ORDER), "wall_ms_per_iteration": {k: _stats(wall[k]) for k in ORDER},
           "added_us_per_iteration_median": round((med["early_stop"] - med["plain"]) * 1e3, 2),
           "added_us_per_iteration_by_block": [round((y - x) * 1e3, 2) for x, y in zip(wall["plain"], wall["early_stop"])],
           "bytes_moved_per_iteration": 28 * n, "monitor_memory_bytes": b.es.memory_bytes,
           "bit_identical_parameters": bool(same), "last_record": b.es.last(),
           "device": torch.cuda.get_device_name(0),
           "build_id": dip_native.lib().dip_build_id().decode()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))
    if not same:
        raise SystemExit("the monitored fit diverged from the plain one")


if __name__ == "__main__":
    main()
