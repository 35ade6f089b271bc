"""dip_optim.NativeIteration (the whole iteration as ONE dip_iter_run call, no autograd) against the eager MSEHead closure

    opt.zero_grad(); x = reg(); loss, out = head(x); loss.backward(); opt.step()

for bench.py's `default` (512 x 512, reg-noise 1/30) and `library` (448 x 704, masked MSE) configurations.

    python tools/bench_native_iter.py [--configs default library] [--blocks 5] [--iters 50] [--out profiles/NAME.json]
    python tools/bench_native_iter.py --monitor          # the denoising closure: + FitMonitor (EMA, 3 PSNRs, back-tracking)
    python tools/bench_native_iter.py --configs sr --out profiles/sr_head_bench.json

`sr` is bench.py's `sr` configuration (the default net at 512 x 512, Lanczos2 down-sampler of factor 4, reg-noise 0.03;
super-resolution.ipynb:169-186) in THREE forms, three nets from one seed, blocks A B C A B C ...: the notebook's spelling
(out = net(x); mse(downsampler(out), img_LR)), the eager utils.loss_head.SRHead closure, and NativeIteration(SRHead); the last
two must still be bit-identical at the end.

With --monitor both forms carry a utils.fit_monitor.FitMonitor with ground truth and back-tracking on (denoising.ipynb:204-248):
the eager closure calls monitor.update(out, loss) between backward() and opt.step(), the other form is
NativeIteration(monitor=); `default` only unless --configs says otherwise, result in profiles/native_iter_monitor_bench.json.

Per configuration two nets are built from one seed; blocks of `--iters` iterations alternate between the two forms (A B A B
..., `--blocks` of each) in ONE process on one card.  Per block and iteration:
  * wall       -- first call until the closing synchronize() returns;
  * host_issue -- first call until the last step() returns, BEFORE the closing synchronize() (when the GPU is the limit and
                  the launch queue fills, this tends towards the wall time: read it next to `wall`).
Medians, minima and maxima over the blocks, and a final check that the two nets are still bit-identical.
Every configuration runs in a child process of its own under `timeout`, the children chained with `&&`; one JSON file.
"""
import argparse
import json
import os
import shlex
import statistics
import subprocess
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def _stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
            "blocks": [round(x, 4) for x in v]}


def child(config, blocks, iters, warmup, out_path, monitor=False):
    import torch          # before the library: libdip_hip.so must bind to the HIP runtime torch has loaded
    ge.build()
    import bench
    import dip_native
    from dip_optim import FusedAdam, NativeIteration
    from utils.common_utils import get_params
    from utils.fit_monitor import FitMonitor
    from utils.loss_head import MSEHead
    from utils.reg_noise import RegNoise
    assert torch.cuda.is_available(), "bench_native_iter.py needs an MI355X"
    dev = torch.device("cuda:0")
    size = bench.CONFIGS[config]["size"]
    reg_std = {"default": 1. / 30., "library": 0.0}[config]

    def make():
        torch.manual_seed(0)
        net, depth = bench.build_net(config)
        net = net.to(dev)
        z, target = bench.make_problem(0, size, depth)
        z, target = z.to(dev), target.to(dev)
        mask = None
        if config == "library":
            g = torch.Generator().manual_seed(1000)
            mask = (torch.rand(1, 1, *size, generator=g) > 0.3).float().expand(1, 3, *size).contiguous().to(dev)
        head = MSEHead(net, target, mask)
        reg = RegNoise(z, reg_std, seed=1234) if reg_std > 0 else None
        opt = FusedAdam(get_params('net', net, z), lr=0.01)
        mon = None
        if monitor:           # the notebook's settings (denoising.ipynb:136-137); room for every iteration of this run
            g = torch.Generator().manual_seed(2000)
            gt = torch.rand(target.shape, generator=g).to(dev)
            mon = FitMonitor(net, target, gt, exp_weight=0.99, show_every=100, backtrack_db=5.0,
                             capacity=warmup + blocks * iters)
        return net, z, head, reg, opt, mon

    net_a, z_a, head_a, reg_a, opt_a, mon_a = make()
    net_b, z_b, head_b, reg_b, opt_b, mon_b = make()
    last = {}

    def eager():
        opt_a.zero_grad()
        loss, out = head_a(reg_a() if reg_a is not None else z_a)
        loss.backward()
        if mon_a is not None:
            mon_a.update(out, loss)
        opt_a.step()
        last["out"] = out

    it = NativeIteration(net_b, head_b, opt_b, z_b, reg_noise=reg_b, monitor=mon_b)
    for _ in range(warmup):
        eager()
        it.step()
    torch.cuda.synchronize()
    res = {k: {"wall": [], "host": []} for k in ("eager", "native")}
    for _ in range(blocks):
        for name, one in (("eager", eager), ("native", it.step)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                one()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            res[name]["host"].append((t1 - t0) / iters * 1e3)
            res[name]["wall"].append((t2 - t0) / iters * 1e3)
    same = all(torch.equal(p, q) for p, q in zip(net_a.parameters(), net_b.parameters())) and torch.equal(last["out"], it.out)
    if monitor:
        same = same and mon_a.i == mon_b.i and torch.equal(mon_a.records, mon_b.records) \
            and torch.equal(mon_a.out_avg, mon_b.out_avg) and torch.equal(mon_a.state, mon_b.state)
    eng = net_b.__dict__["_dip_engine"]
    rec = {
        "config": config, "size": list(size), "blocks": blocks, "iters_per_block": iters, "warmup": warmup,
        "launches_per_iteration": sum(1 for cl in it._plan["lists"].phases for n in cl.names if n not in ("record", "wait")),
        "two_streams": bool(eng.two_streams),
        "eager_ms": {"wall": _stats(res["eager"]["wall"]), "host_issue": _stats(res["eager"]["host"])},
        "native_ms": {"wall": _stats(res["native"]["wall"]), "host_issue": _stats(res["native"]["host"])},
        "bit_identical_after_run": bool(same),
        **({"monitor": {"gt": True, "backtracking": True, "show_every": mon_b.show_every, "exp_weight": mon_b.exp_weight,
                        "iterations_recorded": mon_b.i, "fell_back": int(mon_b.history()[:, 7].sum()),
                        "last": mon_b.last()}} if monitor else {}),
        "device": torch.cuda.get_device_name(0), "build_id": dip_native.lib().dip_build_id().decode(),
    }
    e, n = rec["eager_ms"], rec["native_ms"]
    rec["host_issue_ratio_eager_over_native"] = round(e["host_issue"]["median"] / n["host_issue"]["median"], 3)
    rec["wall_ratio_eager_over_native"] = round(e["wall"]["median"] / n["wall"]["median"], 3)
    rec["it_per_s"] = {"eager": round(1e3 / e["wall"]["median"], 1), "native": round(1e3 / n["wall"]["median"], 1)}
    with open(out_path, "w") as f:
        json.dump(rec, f)
    print(json.dumps(rec))
    if not same:
        raise SystemExit("the two forms diverged")


def child_sr(blocks, iters, warmup, out_path, order=("spelled", "eager", "native")):
    import torch          # before the library: libdip_hip.so must bind to the HIP runtime torch has loaded
    ge.build()
    import bench
    import dip_native
    from dip_optim import FusedAdam, NativeIteration
    from models.downsampler import Downsampler
    from utils.common_utils import get_params
    from utils.loss_head import SRHead
    from utils.reg_noise import RegNoise
    assert torch.cuda.is_available(), "bench_native_iter.py needs an MI355X"
    dev = torch.device("cuda:0")
    size = bench.CONFIGS["sr"]["size"]

    def make():
        torch.manual_seed(0)
        net, depth = bench.build_net("sr")
        net = net.to(dev)
        z, target = bench.make_problem(0, size, depth)
        z, lr = z.to(dev), torch.nn.functional.avg_pool2d(target.to(dev), 4)          # a 128 x 128 LR image, as bench.py
        down = Downsampler(n_planes=3, factor=4, kernel_type='lanczos2', phase=0.5, preserve_size=True).to(dev)
        return SimpleNamespace(net=net, z=z, lr=lr, down=down, reg=RegNoise(z, 0.03, seed=1234),
                               opt=FusedAdam(get_params('net', net, z), lr=0.01))

    fits = {name: make() for name in order}          # (built, and later timed, in the order given)
    a, b, c = fits["spelled"], fits["eager"], fits["native"]
    mse = torch.nn.MSELoss()
    head_b, head_c = SRHead(b.net, b.lr, b.down), SRHead(c.net, c.lr, c.down)
    last = {}

    def spelled():
        a.opt.zero_grad()
        out = a.net(a.reg())
        loss = mse(a.down(out), a.lr)
        loss.backward()
        a.opt.step()

    def eager():
        b.opt.zero_grad()
        loss, out = head_b(b.reg())
        loss.backward()
        b.opt.step()
        last["out"] = out

    it = NativeIteration(c.net, head_c, c.opt, c.z, reg_noise=c.reg)
    forms = tuple((name, {"spelled": spelled, "eager": eager, "native": it.step}[name]) for name in order)
    for _ in range(warmup):
        for _, one in forms:
            one()
    torch.cuda.synchronize()
    res = {k: {"wall": [], "host": []} for k, _ in forms}
    for _ in range(blocks):
        for name, one in forms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                one()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            res[name]["host"].append((t1 - t0) / iters * 1e3)
            res[name]["wall"].append((t2 - t0) / iters * 1e3)
    same = all(torch.equal(p, q) for p, q in zip(b.net.parameters(), c.net.parameters())) and torch.equal(last["out"], it.out) \
        and torch.equal(head_b.out_LR, head_c.out_LR)
    # the spelled closure rounds the loss differently: how far its parameters have drifted from the fused forms' (information)
    drift = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(a.net.parameters(), b.net.parameters()))
    eng = c.net.__dict__["_dip_engine"]
    rec = {
        "config": "sr", "order": list(order), "size": list(size), "factor": 4, "kernel": "lanczos2", "reg_noise_std": 0.03,
        "blocks": blocks, "iters_per_block": iters, "warmup": warmup,
        "launches_per_iteration": sum(1 for cl in it._plan["lists"].phases for n in cl.names if n not in ("record", "wait")),
        "two_streams": bool(eng.two_streams),
        **{f"{k}_ms": {"wall": _stats(res[k]["wall"]), "host_issue": _stats(res[k]["host"])} for k, _ in forms},
        "bit_identical_after_run": bool(same), "spelled_max_param_drift": drift,
        "device": torch.cuda.get_device_name(0), "build_id": dip_native.lib().dip_build_id().decode(),
    }
    med = lambda k, w: rec[f"{k}_ms"][w]["median"]          # noqa: E731
    rec["it_per_s"] = {k: round(1e3 / med(k, "wall"), 1) for k, _ in forms}
    rec["wall_ratio_spelled_over_eager"] = round(med("spelled", "wall") / med("eager", "wall"), 3)
    rec["wall_ratio_spelled_over_native"] = round(med("spelled", "wall") / med("native", "wall"), 3)
    rec["host_issue_ratio_spelled_over_native"] = round(med("spelled", "host_issue") / med("native", "host_issue"), 3)
    with open(out_path, "w") as f:
        json.dump(rec, f)
    print(json.dumps(rec))
    if not same:
        raise SystemExit("the eager SRHead closure and NativeIteration(SRHead) diverged")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=None, choices=["default", "library", "sr"])
    ap.add_argument("--monitor", action="store_true", help="both forms with a FitMonitor (ground truth, back-tracking)")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--out", default=None)
    ap.add_argument("--sr-order", nargs=3, default=["spelled", "eager", "native"], choices=["spelled", "eager", "native"],
                    help="`sr`: the order in which the three forms are built and timed within a round of blocks")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.configs is None:
        args.configs = ["default"] if args.monitor else ["default", "library"]
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "native_iter_monitor_bench.json" if args.monitor else "native_iter_bench.json")
    if args.blocks < 5 or args.iters < 50:
        ap.error("at least 5 blocks of at least 50 iterations")
    if sorted(args.sr_order) != ["eager", "native", "spelled"]:
        ap.error("--sr-order takes each of spelled, eager, native once")
    if args.monitor and "sr" in args.configs:
        ap.error("--monitor covers the MSEHead configurations")
    if args.child == "sr":
        child_sr(args.blocks, args.iters, args.warmup, args.out, tuple(args.sr_order))
        return
    if args.child is not None:
        child(args.child, args.blocks, args.iters, args.warmup, args.out, args.monitor)
        return
    parts = {c: f"{args.out}.{c}.part" for c in args.configs}
    steps = [" ".join(["timeout", "-k", "10", str(args.timeout), shlex.quote(sys.executable), shlex.quote(os.path.abspath(__file__)),
                       "--child", c, "--blocks", str(args.blocks), "--iters", str(args.iters), "--warmup", str(args.warmup),
                       "--out", shlex.quote(p)] + (["--sr-order", *args.sr_order] if c == "sr" else [])
                      + (["--monitor"] if args.monitor else [])) for c, p in parts.items()]
    rc = subprocess.run(["bash", "-c", " && ".join(steps)]).returncode          # a failing step ends the chain
    done = {}
    for c, p in parts.items():
        if os.path.exists(p):
            with open(p) as f:
                done[c] = json.load(f)
            os.remove(p)
    if done:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/bench_native_iter.py" + (" --monitor" if args.monitor else ""), "results": done}, f, indent=1)
            f.write("\n")
    if rc:
        raise SystemExit(f"a configuration failed (exit status {rc}); results so far: {sorted(done)}")


if __name__ == "__main__":
    main()
