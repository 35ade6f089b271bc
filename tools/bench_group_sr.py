"""What grouping buys for super-resolution fits: B fits of the super-resolution notebook's net (bench.py's `sr` net: skip,
128 channels x 5 scales, input_depth 32; reg-noise 0.03, Lanczos2 down-sampler of factor 4; super-resolution.ipynb:141-186)
at HR 128 x 128 and 256 x 256, in aggregate iterations per second, three legs:

  solo     -- the B fits one after another, each as dip_optim.NativeIteration + utils.loss_head.SRHead (one dip_iter_run call
              per iteration): the best a batch of SR fits could do before GroupedFits(downsamplers=);
  grouped  -- dip_group.GroupedFits(downsamplers=), eager: one launch list for the B fits;
  graphed  -- the same as ONE hipGraph (GroupedFits.capture()).

    python tools/bench_group_sr.py [--sizes 128 256] [--B 8] [--blocks 5] [--iters 50] [--out profiles/group_sr_bench.json]

One process per size (under `timeout`, chained with `&&`), on one card.  Three sets of B nets from the same seeds; after
`--warmup` iterations of every leg, blocks of `--iters` iterations per fit alternate solo / grouped / graphed (`--blocks` of
each); a block's wall time runs from its first call until the closing synchronize() returns.  Medians, minima and maxima over
the blocks; it/s = B * iters / wall.  All three legs have done the same number of iterations at the end, and the tool checks
that every fit has the same parameters, bit for bit, in all three."""
import argparse
import json
import os
import shlex
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

LEGS = ("solo", "grouped", "graphed")


def child(size, B, blocks, iters, warmup, out_path):
    import torch          # before the library: libdip_hip.so must bind to the HIP runtime torch has loaded
    ge.build()
    import bench
    import dip_native
    from dip_group import GroupedFits
    from dip_optim import FusedAdam, NativeIteration
    from models.downsampler import Downsampler
    from utils.common_utils import get_params
    from utils.loss_head import SRHead
    from utils.reg_noise import RegNoise
    assert torch.cuda.is_available(), "bench_group_sr.py needs an MI355X"
    dev = torch.device("cuda:0")
    hw = (size, size)

    def problem(b):
        torch.manual_seed(b)
        net, depth = bench.build_net("sr")
        z, target = bench.make_problem(b, hw, depth)
        lr = torch.nn.functional.avg_pool2d(target, 4)                  # a (size / 4)^2 LR image, as bench.py's `sr`
        down = Downsampler(n_planes=3, factor=4, kernel_type='lanczos2', phase=0.5, preserve_size=True)
        return net.to(dev), z.to(dev), lr.to(dev), down.to(dev)

    sets = {leg: [problem(b) for b in range(B)] for leg in LEGS}
    seeds = [1234 + b for b in range(B)]
    solo = []
    for b, (net, z, lr, down) in enumerate(sets["solo"]):
        solo.append(NativeIteration(net, SRHead(net, lr, down), FusedAdam(get_params('net', net, z), lr=0.01), z,
                                    reg_noise=RegNoise(z, 0.03, seed=seeds[b])))
    groups = {}
    for leg in ("grouped", "graphed"):
        nets, zs, lrs, downs = (list(x) for x in zip(*sets[leg]))
        groups[leg] = GroupedFits(nets, zs, lrs, downsamplers=downs, reg_noise_std=0.03, seeds=seeds, lr=0.01)
    for it in solo:
        it.run(warmup)
    groups["grouped"].step(warmup)
    groups["graphed"].capture(warmup=warmup)

    def run_solo(n):
        for it in solo:
            it.run(n)

    run = {"solo": run_solo, "grouped": groups["grouped"].step, "graphed": groups["graphed"].run}
    assert groups["graphed"].graph is not None and groups["grouped"].graph is None
    torch.cuda.synchronize()
    wall = {leg: [] for leg in LEGS}
    for _ in range(blocks):
        for leg in LEGS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run[leg](iters)
            torch.cuda.synchronize()
            wall[leg].append(time.perf_counter() - t0)
    n_done = warmup + blocks * iters
    counts_ok = all(g.step_counts() == [n_done] * B for g in groups.values()) and all(it.iterations == n_done for it in solo)
    same = all(torch.equal(p, q) and torch.equal(p, r)
               for b in range(B)
               for p, q, r in zip(*(sets[leg][b][0].parameters() for leg in LEGS)))
    ips = {leg: [B * iters / t for t in wall[leg]] for leg in LEGS}
    st = lambda v: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1),      # noqa: E731
                    "blocks": [round(x, 1) for x in v]}
    rec = {"HR": list(hw), "LR": [size // 4, size // 4], "B": B, "factor": 4, "kernel": "lanczos2", "reg_noise_std": 0.03,
           "blocks": blocks, "iters_per_block_and_fit": iters, "warmup": warmup,
           "aggregate_it_per_s": {leg: st(ips[leg]) for leg in LEGS},
           "block_wall_s": {leg: [round(t, 4) for t in wall[leg]] for leg in LEGS},
           "iterations_per_fit": n_done, "step_counts_agree": bool(counts_ok), "bit_identical_across_legs": bool(same),
           "device": torch.cuda.get_device_name(0), "host": socket.gethostname(),
           "build_id": dip_native.lib().dip_build_id().decode()}
    med = lambda leg: rec["aggregate_it_per_s"][leg]["median"]          # noqa: E731
    rec["ratio_grouped_over_solo"] = round(med("grouped") / med("solo"), 3)
    rec["ratio_graphed_over_solo"] = round(med("graphed") / med("solo"), 3)
    with open(out_path, "w") as f:
        json.dump(rec, f)
    print(json.dumps(rec))
    if not (same and counts_ok):
        raise SystemExit("the legs diverged")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_sr_bench.json"))
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.blocks < 5 or args.iters < 50 or args.warmup < 3:
        ap.error("at least 5 blocks of at least 50 iterations after at least 3 warm-up iterations")
    if any(s % 32 or s < 64 for s in args.sizes):
        ap.error("sizes are multiples of 32 from 64 (five scales, factor 4)")
    if args.child is not None:
        child(args.child, args.B, args.blocks, args.iters, args.warmup, args.out)
        return
    parts = {s: f"{args.out}.{s}.part" for s in args.sizes}
    steps = [" ".join(["timeout", "-k", "10", str(args.timeout), shlex.quote(sys.executable), shlex.quote(os.path.abspath(__file__)),
                       "--child", str(s), "--B", str(args.B), "--blocks", str(args.blocks), "--iters", str(args.iters),
                       "--warmup", str(args.warmup), "--out", shlex.quote(p)]) for s, p in parts.items()]
    rc = subprocess.run(["bash", "-c", " && ".join(steps)]).returncode          # a failing step ends the chain
    done = {}
    for s, p in parts.items():
        if os.path.exists(p):
            with open(p) as f:
                done[str(s)] = json.load(f)
            os.remove(p)
    if done:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/bench_group_sr.py", "results": done}, f, indent=1)
            f.write("\n")
    if rc:
        raise SystemExit(f"a size failed (exit status {rc}); results so far: {sorted(done)}")


if __name__ == "__main__":
    main()
