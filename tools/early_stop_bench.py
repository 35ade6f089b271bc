"""What the device-side early-stopping criteria cost per iteration, solo and grouped, in one process on one card.

    python tools/early_stop_bench.py [--size 512] [--window 100] [--alpha 0.1] [--B 8] [--blocks 7] [--iters 50]
                                     [--out profiles/early_stop_group_bench.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/early_stop_bench.py --trace 100 --trace-leg emv   # kernel times,
                                                                                                         # a run of its own

Solo legs: bench.py's `default` net at size x size, reg-noise 1/30, Adam at LR 0.01, three fits from one seed --
NativeIteration(early_stop=None), early_stop=EarlyStopMonitor(mode='wmv') and mode='emv'.  Group legs: bench.py's `snail` net
(256 x 384) x B as one dip_group.GroupedFits, captured into its ONE hipGraph, with early_stop=None,
GroupedEarlyStopMonitor(mode='wmv') and mode='emv'.  After the warm-up the legs of a family alternate in blocks, A B C A B C ...:
a block's wall time runs from its first call until the closing synchronize() returns; medians, minima and maxima over the
blocks.  The early_stop=None leg of the same call is the yard-stick.  The fits of a family must hold bit-identical parameters at
the end (the monitor does not touch the fit).  --order builds the legs in another order: the fit that is built third has
measured about 0.23 ms slower per solo iteration whatever it monitors (the cause was not measured -- the
pooled streams it draws are a supposition), so a criterion is judged from the second position.  --trace N issues N monitored
iterations of one leg and nothing else, for a profiler that lists the kernels.  (profiles/early_stop_bench.json is the record of the windowed form alone, from before the
other legs existed.)"""
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

ORDER = ("plain", "early_stop", "early_stop_emv")
MODE = {"plain": None, "early_stop": "wmv", "early_stop_emv": "emv"}
TRACE_LEGS = ("wmv", "emv", "group_wmv", "group_emv")


def _stats(v, nd=4):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd),
            "blocks": [round(x, nd) for x in v]}


def _fit(dev, size, mode, args, capacity):
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
    f.es = None if mode is None else EarlyStopMonitor(f.img, window=args.window, patience=args.patience, net=f.net,
                                                      capacity=capacity, mode=mode, alpha=args.alpha)
    f.it = NativeIteration(f.net, f.head, f.opt, f.z, reg_noise=f.reg, early_stop=f.es)
    f.run = f.it.run
    f.nets = [f.net]
    return f


def _group(dev, B, mode, args, capacity, warmup):
    """bench.py's `snail` net x B as ONE captured GroupedFits; `warmup` eager iterations are part of the capture."""
    import torch
    import bench
    from dip_group import GroupedFits
    from utils.fit_monitor import GroupedEarlyStopMonitor
    hw = bench.CONFIGS["snail"]["size"]
    nets, zs, ts = [], [], []
    for b in range(B):
        torch.manual_seed(b)
        net, depth = bench.build_net("snail")
        z, noisy = bench.make_problem(b, hw, depth)
        nets.append(net.to(dev)), zs.append(z.to(dev)), ts.append(noisy.to(dev))
    es = None if mode is None else GroupedEarlyStopMonitor(mode=mode, window=args.window, alpha=args.alpha,
                                                           patience=args.patience, capacity=capacity)
    g = GroupedFits(nets, zs, ts, reg_noise_std=1. / 30., seeds=[1234 + b for b in range(B)], lr=0.01, early_stop=es)
    g.capture(warmup=warmup)
    return SimpleNamespace(g=g, es=es, run=g.run, nets=nets, n=ts[0].numel())


def _alternate(legs, blocks, iters):
    """ms per iteration of every block, the legs taking turns."""
    import torch
    wall = {k: [] for k in legs}
    for _ in range(blocks):
        for name, f in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f.run(iters)
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) / iters * 1e3)
    return wall


def _report(legs, wall):
    import torch
    plain = legs["plain"]
    same = all(torch.equal(p, q) for f in legs.values() for a, b in zip(plain.nets, f.nets)
               for p, q in zip(a.parameters(), b.parameters()))
    med = {k: statistics.median(wall[k]) for k in legs}
    return {"order": list(legs), "wall_ms_per_iteration": {k: _stats(wall[k]) for k in legs},
            "added_us_per_iteration_median": {k: round((med[k] - med["plain"]) * 1e3, 2) for k in legs if k != "plain"},
            "added_us_per_iteration_by_block": {k: [round((y - x) * 1e3, 2) for x, y in zip(wall["plain"], wall[k])]
                                                for k in legs if k != "plain"},
            "monitor_memory_bytes": {k: f.es.memory_bytes for k, f in legs.items() if f.es is not None},
            "bit_identical_parameters": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--window", type=int, default=100)
    ap.add_argument("--alpha", type=float, default=0.1)
    ap.add_argument("--patience", type=int, default=1000)
    ap.add_argument("--B", type=int, default=8, help="instances of the group legs (0: solo legs only)")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--trace", type=int, default=0, help="issue this many monitored iterations of --trace-leg and nothing else")
    ap.add_argument("--trace-leg", default="wmv", choices=TRACE_LEGS)
    ap.add_argument("--order", nargs="+", default=list(ORDER), choices=ORDER,
                    help="the legs in the order in which they are built and take their turns (always with 'plain')")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "early_stop_group_bench.json"))
    args = ap.parse_args()
    if not args.trace and (args.blocks * args.iters < 300 or args.warmup < 3):
        ap.error("at least 300 iterations per leg after at least 3 warm-up iterations")
    if "plain" not in args.order or len(set(args.order)) != len(args.order):
        ap.error("--order names every leg once and includes 'plain', the yard-stick")
    import torch          # before the library: libdip_hip.so must bind to the HIP runtime torch has loaded
    ge.build()
    import dip_native
    assert torch.cuda.is_available(), "early_stop_bench.py needs an MI355X"
    dev = torch.device("cuda:0")
    if args.trace:
        mode = args.trace_leg.split("_")[-1]
        if args.trace_leg.startswith("group"):
            f = _group(dev, max(args.B, 1), mode, args, args.trace + 3, 3)
        else:
            f = _fit(dev, args.size, mode, args, args.trace)
        f.run(args.trace)
        torch.cuda.synchronize()
        print(json.dumps({"traced_leg": args.trace_leg, "traced_iterations": args.trace, "last_record": f.es.last()}))
        return
    capacity = args.warmup + args.blocks * args.iters
    solo = {name: _fit(dev, args.size, MODE[name], args, capacity) for name in args.order}
    for f in solo.values():
        f.run(args.warmup)
    torch.cuda.synchronize()
    n = solo["plain"].img.numel()
    rec = {"tool": "tools/early_stop_bench.py", "window": args.window, "alpha": args.alpha,
           "patience": args.patience, "blocks": args.blocks,
           "iters_per_block": args.iters, "warmup": args.warmup,
           "solo": dict(_report(solo, _alternate(solo, args.blocks, args.iters)), net="default", HW=[args.size, args.size], n=n,
                        bytes_moved_per_iteration={k: (28 if MODE[k] == "wmv" else 20) * n for k in solo if MODE[k]},
                        last_record={k: f.es.last() for k, f in solo.items() if f.es is not None})}
    ok = rec["solo"]["bit_identical_parameters"]
    del solo
    if args.B > 0:
        grp = {name: _group(dev, args.B, MODE[name], args, capacity, args.warmup) for name in args.order}
        torch.cuda.synchronize()
        n = grp["plain"].n
        rec["group"] = dict(_report(grp, _alternate(grp, args.blocks, args.iters)), net="snail", B=args.B, n_per_instance=n,
                            form="ONE hipGraph per group iteration (GroupedFits.capture)",
                            bytes_moved_per_iteration={k: (28 if MODE[k] == "wmv" else 20) * n * args.B for k in grp if MODE[k]},
                            last_record={k: f.es.last()[0] for k, f in grp.items() if f.es is not None})
        ok = ok and rec["group"]["bit_identical_parameters"]
    rec.update(device=torch.cuda.get_device_name(0), build_id=dip_native.lib().dip_build_id().decode())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))
    if not ok:
        raise SystemExit("a monitored fit diverged from the plain one")


if __name__ == "__main__":
    main()
