"""What the device-side super-resolution record costs, and what it replaces: utils.fit_monitor.SRFitMonitor /
GroupedSRFitMonitor (dip_sr_monitor_dev) against the closure of super-resolution.ipynb:169-191, which computes psnr_LR and
psnr_HR on the host in every iteration (two device-to-host copies, two synchronisations).

    python tools/bench_sr_monitor.py [--blocks 5] [--iters 50] [--B 8] [--group-size 256] [--out profiles/sr_monitor_bench.json]

`solo`: bench.py's `sr` configuration (the default net at 512 x 512, Lanczos2 down-sampler of factor 4, reg-noise 0.03), four
nets from one seed, blocks A B C D A B C D ...:
  native        -- NativeIteration(SRHead), no record;
  native_mon    -- NativeIteration(SRHead, monitor=SRFitMonitor(img_LR, img_HR)): the record inside the one call;
  eager_host    -- the eager SRHead closure followed by the notebook's two host PSNRs (out_LR and out_HR copied to the host);
  spelled_host  -- the notebook's spelling (net, downsampler, mse as separate ops) followed by the same two host PSNRs.
`group`: B fits of the same net at --group-size (the sizes of tools/bench_group_sr.py), four groups from the same seeds:
  grouped / grouped_mon -- GroupedFits(downsamplers=) eager, without / with monitor=GroupedSRFitMonitor(imgs_HR);
  graphed / graphed_mon -- the same as ONE hipGraph.
A block's wall time runs from its first call until the closing synchronize() returns; medians, minima and maxima over the
blocks.  The monitored and the unmonitored fits must hold bit-identical parameters at the end.  Each part runs in a child
process of its own under `timeout`, chained with `&&`.

For the kernel time of the new launches run one monitored leg alone under `rocprofv3 --kernel-trace --stats` (no counters):
    rocprofv3 --kernel-trace --stats -d DIR -o sr_monitor -- python tools/bench_sr_monitor.py --child profile-solo
    rocprofv3 --kernel-trace --stats -d DIR -o sr_monitor -- python tools/bench_sr_monitor.py --child profile-group
(60 iterations of native_mon / grouped_mon and nothing else)."""
import argparse
import json
import os
import shlex
import socket
import statistics
import subprocess
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def _stats(v, nd=4):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd),
            "blocks": [round(x, nd) for x in v]}


def _problem(seed, hw, dev):
    """Net, input, LR image, HR image and down-sampler of one fit (bench.py's `sr` net; the LR image as bench.py makes it)."""
    import torch
    import bench
    from models.downsampler import Downsampler
    torch.manual_seed(seed)
    net, depth = bench.build_net("sr")
    z, hr = bench.make_problem(seed, hw, depth)
    lr = torch.nn.functional.avg_pool2d(hr, 4)
    down = Downsampler(n_planes=3, factor=4, kernel_type='lanczos2', phase=0.5, preserve_size=True)
    return SimpleNamespace(net=net.to(dev), z=z.to(dev), lr=lr.to(dev), hr=hr.to(dev), down=down.to(dev))


def _host_psnr(img_np, out):
    """compare_psnr(img_np, torch_to_np(out)) of the notebook: the output goes to the host."""
    import numpy as np
    mse = np.mean((img_np.astype(np.float64) - out.detach().cpu().numpy()[0].astype(np.float64)) ** 2)
    return 10.0 * np.log10(1.0 / mse)


def _solo_forms(dev, capacity, which):
    import torch
    import bench
    from dip_optim import FusedAdam, NativeIteration
    from utils.common_utils import get_params
    from utils.fit_monitor import SRFitMonitor
    from utils.loss_head import SRHead
    from utils.reg_noise import RegNoise
    size = bench.CONFIGS["sr"]["size"]
    forms, fits = {}, {}
    mse = torch.nn.MSELoss()
    for name in which:
        f = fits[name] = _problem(0, size, dev)
        f.reg = RegNoise(f.z, 0.03, seed=1234)
        f.opt = FusedAdam(get_params('net', f.net, f.z), lr=0.01)
        f.history = []
        if name in ("native", "native_mon"):
            f.mon = SRFitMonitor(f.lr, f.hr, capacity=capacity) if name == "native_mon" else None
            f.it = NativeIteration(f.net, SRHead(f.net, f.lr, f.down), f.opt, f.z, reg_noise=f.reg, monitor=f.mon)
            forms[name] = f.it.step
            continue
        f.lr_np, f.hr_np = f.lr.cpu().numpy()[0], f.hr.cpu().numpy()[0]
        if name == "eager_host":
            f.head = SRHead(f.net, f.lr, f.down)

            def one(f=f):
                f.opt.zero_grad()
                loss, out = f.head(f.reg())
                loss.backward()
                f.history.append([_host_psnr(f.lr_np, f.head.out_LR), _host_psnr(f.hr_np, out)])
                f.opt.step()
        else:
            def one(f=f):
                f.opt.zero_grad()
                out = f.net(f.reg())
                out_lr = f.down(out)
                loss = mse(out_lr, f.lr)
                loss.backward()
                f.history.append([_host_psnr(f.lr_np, out_lr), _host_psnr(f.hr_np, out)])
                f.opt.step()
        forms[name] = one
    return forms, fits, size


def child_solo(blocks, iters, warmup, out_path):
    import torch          # before the library: libdip_hip.so must bind to the HIP runtime torch has loaded
    ge.build()
    import dip_native
    assert torch.cuda.is_available(), "bench_sr_monitor.py needs an MI355X"
    dev = torch.device("cuda:0")
    order = ("native", "native_mon", "eager_host", "spelled_host")
    forms, fits, size = _solo_forms(dev, warmup + blocks * iters, order)
    for _ in range(warmup):
        for name in order:
            forms[name]()
    torch.cuda.synchronize()
    wall = {k: [] for k in order}
    for _ in range(blocks):
        for name in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                forms[name]()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) / iters * 1e3)
    a, b, c = fits["native"], fits["native_mon"], fits["eager_host"]
    same = all(torch.equal(p, q) and torch.equal(p, r) for p, q, r in zip(a.net.parameters(), b.net.parameters(), c.net.parameters()))
    hist = b.mon.history()
    host = c.history
    dev_vs_host = max(max(abs(float(hist[i, 3]) - host[i][0]), abs(float(hist[i, 4]) - host[i][1])) for i in range(len(host)))
    rec = {"part": "solo", "config": "sr", "HR": list(size), "LR": [size[0] // 4, size[1] // 4], "factor": 4, "kernel": "lanczos2",
           "reg_noise_std": 0.03, "blocks": blocks, "iters_per_block": iters, "warmup": warmup, "order": list(order),
           "launches_per_iteration": {k: sum(1 for cl in fits[k].it._plan["lists"].phases for n in cl.names if n not in ("record", "wait"))
                                      for k in ("native", "native_mon")},
           "wall_ms_per_iteration": {k: _stats(wall[k]) for k in order},
           "iterations_recorded": int(b.mon.i), "bit_identical_parameters_native_native_mon_eager_host": bool(same),
           "max_abs_dB_device_record_vs_host_psnr": dev_vs_host, "last_record": b.mon.last(),
           "device": torch.cuda.get_device_name(0), "host": socket.gethostname(),
           "build_id": dip_native.lib().dip_build_id().decode()}
    med = lambda k: rec["wall_ms_per_iteration"][k]["median"]          # noqa: E731
    rec["monitor_cost_ms"] = round(med("native_mon") - med("native"), 4)
    rec["host_psnr_cost_ms_eager"] = round(med("eager_host") - med("native"), 4)
    with open(out_path, "w") as f:
        json.dump(rec, f)
    print(json.dumps(rec))
    if not same:
        raise SystemExit("the monitored and the unmonitored fit diverged")


def _groups(dev, size, B, capacity, which):
    from dip_group import GroupedFits
    from utils.fit_monitor import GroupedSRFitMonitor
    out = {}
    seeds = [1234 + b for b in range(B)]
    for leg in which:
        ps = [_problem(b, (size, size), dev) for b in range(B)]
        mon = GroupedSRFitMonitor([p.hr for p in ps], capacity=capacity) if leg.endswith("_mon") else None
        g = GroupedFits([p.net for p in ps], [p.z for p in ps], [p.lr for p in ps], downsamplers=[p.down for p in ps],
                        reg_noise_std=0.03, seeds=seeds, lr=0.01, monitor=mon)
        out[leg] = SimpleNamespace(g=g, mon=mon, nets=[p.net for p in ps])
    return out


def child_group(size, B, blocks, iters, warmup, out_path):
    import torch
    ge.build()
    import dip_native
    assert torch.cuda.is_available(), "bench_sr_monitor.py needs an MI355X"
    dev = torch.device("cuda:0")
    legs = ("grouped", "grouped_mon", "graphed", "graphed_mon")
    gs = _groups(dev, size, B, warmup + blocks * iters, legs)
    run = {}
    for leg in legs:
        if leg.startswith("graphed"):
            gs[leg].g.capture(warmup=warmup)
            run[leg] = gs[leg].g.run
        else:
            gs[leg].g.step(warmup)
            run[leg] = gs[leg].g.step
    torch.cuda.synchronize()
    wall = {leg: [] for leg in legs}
    for _ in range(blocks):
        for leg in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run[leg](iters)
            torch.cuda.synchronize()
            wall[leg].append((time.perf_counter() - t0) / iters * 1e3)
    same = all(torch.equal(p, q) and torch.equal(p, r) and torch.equal(p, s)
               for b in range(B) for p, q, r, s in zip(*(gs[leg].nets[b].parameters() for leg in legs)))
    same_rec = torch.equal(gs["grouped_mon"].mon.records, gs["graphed_mon"].mon.records)
    rec = {"part": "group", "HR": [size, size], "LR": [size // 4, size // 4], "B": B, "factor": 4, "kernel": "lanczos2",
           "reg_noise_std": 0.03, "blocks": blocks, "iters_per_block": iters, "warmup": warmup, "order": list(legs),
           "wall_ms_per_grouped_iteration": {leg: _stats(wall[leg]) for leg in legs},
           "aggregate_it_per_s": {leg: round(B * 1e3 / statistics.median(wall[leg]), 1) for leg in legs},
           "iterations_recorded": int(gs["grouped_mon"].mon.i), "bit_identical_parameters_across_legs": bool(same),
           "bit_identical_records_eager_graph": bool(same_rec), "last_records": gs["graphed_mon"].mon.last(),
           "device": torch.cuda.get_device_name(0), "host": socket.gethostname(),
           "build_id": dip_native.lib().dip_build_id().decode()}
    med = lambda k: rec["wall_ms_per_grouped_iteration"][k]["median"]          # noqa: E731
    rec["monitor_cost_ms"] = {"eager": round(med("grouped_mon") - med("grouped"), 4),
                              "graph": round(med("graphed_mon") - med("graphed"), 4)}
    with open(out_path, "w") as f:
        json.dump(rec, f)
    print(json.dumps(rec))
    if not (same and same_rec):
        raise SystemExit("the legs diverged")


def child_profile(what, size, B, n=60):
    """n iterations of ONE monitored leg and nothing else: the process to put behind `rocprofv3 --kernel-trace --stats --`."""
    import torch
    ge.build()
    dev = torch.device("cuda:0")
    if what == "solo":
        forms, fits, _ = _solo_forms(dev, n, ("native_mon",))
        fits["native_mon"].it.run(n)
    else:
        gs = _groups(dev, size, B, n, ("grouped_mon",))
        gs["grouped_mon"].g.step(n)
    torch.cuda.synchronize()
    print(f"profile-{what}: {n} iterations")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["solo", "group"], choices=["solo", "group"])
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--group-size", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per part")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sr_monitor_bench.json"))
    ap.add_argument("--child", default=None, choices=["solo", "group", "profile-solo", "profile-group"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child in ("profile-solo", "profile-group"):
        child_profile(args.child.split("-")[1], args.group_size, args.B)
        return
    if args.blocks < 5 or args.iters < 50 or args.warmup < 3:
        ap.error("at least 5 blocks of at least 50 iterations after at least 3 warm-up iterations")
    if args.group_size % 32 or args.group_size < 64:
        ap.error("--group-size is a multiple of 32 from 64 (five scales, factor 4)")
    if args.child == "solo":
        child_solo(args.blocks, args.iters, args.warmup, args.out)
        return
    if args.child == "group":
        child_group(args.group_size, args.B, args.blocks, args.iters, args.warmup, args.out)
        return
    parts = {p: f"{args.out}.{p}.part" for p in args.parts}
    steps = [" ".join(["timeout", "-k", "10", str(args.timeout), shlex.quote(sys.executable), shlex.quote(os.path.abspath(__file__)),
                       "--child", p, "--B", str(args.B), "--group-size", str(args.group_size), "--blocks", str(args.blocks),
                       "--iters", str(args.iters), "--warmup", str(args.warmup), "--out", shlex.quote(path)])
             for p, path in parts.items()]
    rc = subprocess.run(["bash", "-c", " && ".join(steps)]).returncode          # a failing step ends the chain
    done = {}
    for p, path in parts.items():
        if os.path.exists(path):
            with open(path) as f:
                done[p] = json.load(f)
            os.remove(path)
    if done:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/bench_sr_monitor.py", "results": done}, f, indent=1)
            f.write("\n")
    if rc:
        raise SystemExit(f"a part failed (exit status {rc}); results so far: {sorted(done)}")


if __name__ == "__main__":
    main()
