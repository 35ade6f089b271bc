"""What the monitor costs inside a group, and what it saves over doing the bookkeeping from Python: B = 8 fits of the denoising
notebook's small net (bench.py's `snail` net at 256 x 384, reg-noise 1/30; denoising.ipynb:143-150, :204-248), aggregate
iterations per second, four legs in ONE process:

  plain       -- dip_group.GroupedFits, eager, no monitor and no EMA: the fit step alone;
  monitored   -- GroupedFits(monitor=GroupedFitMonitor(imgs_gt, ...)), eager: EMA, 3 PSNRs, records, back-tracking in the
                 launch list (3 dispatches per iteration for all B);
  graphed     -- the same as ONE hipGraph (GroupedFits.capture());
  python      -- what could be done before monitor= existed: the plain group, eager, plus B solo
                 FitMonitor(backtracking=False).update(g.out[b:b+1], g.losses[b]) per iteration from Python (2 B dispatches;
                 no back-tracking: a solo monitor cannot checkpoint a slab row).

    python tools/bench_group_monitor.py [--B 8] [--blocks 5] [--iters 50] [--warmup 10] [--legs plain monitored graphed python]
                                        [--out profiles/group_monitor_bench.json]

`--warmup` iterations of every leg, then `--blocks` rounds; in a round every leg runs one block of `--iters` iterations; a
block's wall time runs from its first call until the closing synchronize() returns.  Medians [min .. max] over the blocks;
it/s = B * iters / wall.  At the end the tool checks that `monitored` and `graphed` hold identical records and parameters.
For the dispatch counts run one leg alone under `rocprofv3 --kernel-trace --stats` (no counters), with DIP_GROUP_NATIVE unset
and with DIP_GROUP_NATIVE=0: iterations = warmup + blocks * iters."""
import argparse
import json
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

LEGS = ("plain", "monitored", "graphed", "python")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--legs", nargs="+", default=list(LEGS), choices=LEGS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_monitor_bench.json"))
    args = ap.parse_args()
    if args.blocks < 1 or args.iters < 1 or args.warmup < 3:
        ap.error("at least one block of at least one iteration after at least 3 warm-up iterations")
    import torch          # before the library: libdip_hip.so must bind to the HIP runtime torch has loaded
    ge.build()
    import bench
    import dip_native
    from dip_group import GroupedFits
    from utils.fit_monitor import FitMonitor, GroupedFitMonitor
    assert torch.cuda.is_available(), "bench_group_monitor.py needs an MI355X"
    dev = torch.device("cuda:0")
    B, legs = args.B, list(args.legs)
    hw = bench.CONFIGS["snail"]["size"]
    n_done = args.warmup + args.blocks * args.iters
    seeds = [1234 + b for b in range(B)]

    def problem(b):
        torch.manual_seed(b)
        net, depth = bench.build_net("snail")
        z, noisy = bench.make_problem(b, hw, depth)
        gt = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(noisy, (1, 1, 1, 1), mode="replicate"), 3, stride=1)
        return net.to(dev), z.to(dev), noisy.to(dev), gt.to(dev)

    sets = {leg: [problem(b) for b in range(B)] for leg in legs}
    groups, mons, run = {}, {}, {}
    for leg in legs:
        nets, zs, ts, gts = (list(x) for x in zip(*sets[leg]))
        if leg in ("monitored", "graphed"):
            mons[leg] = GroupedFitMonitor(gts, exp_weight=0.99, show_every=100, backtrack_db=5.0, capacity=n_done)
        groups[leg] = g = GroupedFits(nets, zs, ts, reg_noise_std=1. / 30., seeds=seeds, lr=0.01, monitor=mons.get(leg))
        if leg == "graphed":
            g.capture(warmup=args.warmup)
            run[leg] = g.run
        elif leg == "python":
            solo = [FitMonitor(None, ts[b], gts[b], exp_weight=0.99, show_every=100, backtracking=False, capacity=n_done)
                    for b in range(B)]
            mons[leg] = solo

            def run_python(n, g=g, solo=solo):
                for _ in range(n):
                    g.step(1)
                    for b, m in enumerate(solo):
                        m.update(g.out[b:b + 1], g.losses[b])

            run_python(args.warmup)
            run[leg] = run_python
        else:
            g.step(args.warmup)
            run[leg] = g.step
    torch.cuda.synchronize()
    wall = {leg: [] for leg in legs}
    for _ in range(args.blocks):
        for leg in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run[leg](args.iters)
            torch.cuda.synchronize()
            wall[leg].append(time.perf_counter() - t0)
    counts_ok = all(g.step_counts() == [n_done] * B for g in groups.values())
    same = None
    if "monitored" in legs and "graphed" in legs:
        a, c = mons["monitored"], mons["graphed"]
        same = a.i == c.i == n_done and torch.equal(a.records, c.records) and torch.equal(a.state, c.state) \
            and torch.equal(a.out_avg, c.out_avg) and torch.equal(a.snapshot, c.snapshot) \
            and all(torch.equal(p, q) for b in range(B)
                    for p, q in zip(sets["monitored"][b][0].parameters(), sets["graphed"][b][0].parameters()))
    ips = {leg: [B * args.iters / t for t in wall[leg]] for leg in legs}
    st = lambda v: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1),      # noqa: E731
                    "blocks": [round(x, 1) for x in v]}
    rec = {"tool": "tools/bench_group_monitor.py", "net": "snail", "size": list(hw), "B": B, "reg_noise_std": 1. / 30.,
           "legs": legs, "blocks": args.blocks, "iters_per_block_and_fit": args.iters, "warmup": args.warmup,
           "aggregate_it_per_s": {leg: st(ips[leg]) for leg in legs},
           "block_wall_s": {leg: [round(t, 4) for t in wall[leg]] for leg in legs},
           "iterations_per_fit": n_done, "step_counts_agree": bool(counts_ok),
           "monitored_and_graphed_bit_identical": same, "fell_back_rows": None if "monitored" not in legs else
           int(torch.count_nonzero(mons["monitored"].records[:, :, 7]).item()),
           "group_native_mask": dip_native.lib().dip_group_native(-1),
           "device": torch.cuda.get_device_name(0), "host": socket.gethostname(),
           "build_id": dip_native.lib().dip_build_id().decode()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    for leg in legs:
        s = rec["aggregate_it_per_s"][leg]
        print(f"{leg:10s} {s['median']:8.1f} it/s [{s['min']:.1f} .. {s['max']:.1f}]")
    if same is False or not counts_ok:
        raise SystemExit("the monitored legs diverged")


if __name__ == "__main__":
    main()
