"""What the device-side restoration bookkeeping costs, and what it replaces: utils.fit_monitor.RestorationFitMonitor
(dip_restore_monitor / dip_restore_monitor_dev + dip_arena_backtrack) against the closure of restoration.ipynb:180-219, which
computes psrn_masked and psrn on the host in every iteration (two device-to-host copies, two synchronisations) and copies every
parameter to the CPU on every show_every-th iteration.

    python tools/bench_restore_monitor.py [--blocks 5] [--iters 50] [--show-every 50] [--out profiles/restore_monitor_bench.json]

Two sizes: `tiny` (a two-scale 16/32-channel skip net at 64 x 64) and `512` (bench.py's `default` net at 512 x 512), each with a
Bernoulli(0.5) mask, reg-noise 0.03 and Adam at LR 0.001 (the notebook's barbara arm).  Three fits from one seed per size, blocks
A B C A B C ...:
  host_notebook -- the eager MSEHead(mask=) closure followed by the notebook's bookkeeping on the host: the two PSNRs from
                   `.cpu().numpy()` copies of the output, `last_net = [x.cpu() for x in net.parameters()]` on every
                   show_every-th iteration, the fall-back test;
  eager_update  -- the same closure with monitor.update(out, total_loss);
  native_mon    -- NativeIteration(monitor=RestorationFitMonitor(...)): the bookkeeping inside the one call.
A block's wall time runs from its first call until the closing synchronize() returns; medians, minima and maxima over the
blocks.  host_notebook on the same card in the same call is the yard-stick: no speed-up is assumed.  The three fits must hold
bit-identical parameters at the end and must have taken the same fall-back decisions.  Each size runs in a child process of its
own under `timeout`, chained with `&&`."""
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

SIZES = {"tiny": (64, 64), "512": (512, 512)}
ORDER = ("host_notebook", "eager_update", "native_mon")


def _stats(v, nd=4):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd),
            "blocks": [round(x, nd) for x in v]}


def _problem(which, dev):
    """Net, input, image and mask of one fit (the same from every call: one seed)."""
    import torch
    import bench
    from models.skip import skip
    hw = SIZES[which]
    torch.manual_seed(0)
    if which == "tiny":
        net, depth = skip(8, 3, num_channels_down=[16, 32], num_channels_up=[16, 32], num_channels_skip=[4, 4],
                          upsample_mode="bilinear", need_sigmoid=True, need_bias=True, pad="reflection"), 8
    else:
        net, depth = bench.build_net("default")
    z, img = bench.make_problem(0, hw, depth)
    mask = (torch.rand(1, 1, *hw, generator=torch.Generator().manual_seed(1)) > 0.5).float()          # get_bernoulli_mask(img, 0.5)
    return SimpleNamespace(net=net.to(dev), z=z.to(dev), img=img.to(dev), mask=mask.to(dev))


def _forms(which, dev, capacity, show_every, lr):
    import numpy as np
    from dip_optim import FusedAdam, NativeIteration
    from utils.common_utils import get_params
    from utils.fit_monitor import RestorationFitMonitor
    from utils.loss_head import MSEHead
    from utils.reg_noise import RegNoise
    forms, fits = {}, {}
    psnr = lambda a, b: 10.0 * np.log10(1.0 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))          # noqa: E731
    for name in ORDER:
        f = fits[name] = _problem(which, dev)
        f.reg = RegNoise(f.z, 0.03, seed=1234)
        f.opt = FusedAdam(get_params('net', f.net, f.z), lr=lr)
        f.head = MSEHead(f.net, f.img, mask=f.mask)
        f.fell = []
        if name == "host_notebook":
            f.img_np, f.mask_np = f.img.cpu().numpy()[0], f.mask.cpu().numpy()[0]
            f.img_masked = f.img_np * f.mask_np
            f.i, f.last_net, f.last = 0, None, 0.0

            def one(f=f):
                f.opt.zero_grad()
                loss, out = f.head(f.reg())
                loss.backward()
                psrn_masked = psnr(f.img_masked, out.detach().cpu().numpy()[0] * f.mask_np)
                psrn = psnr(f.img_np, out.detach().cpu().numpy()[0])          # noqa: F841  (the notebook prints it)
                fell = 0.0
                if f.i % show_every == 0:
                    if f.last_net is not None and psrn_masked - f.last < -5:
                        for new_param, net_param in zip(f.last_net, f.net.parameters()):
                            net_param.data.copy_(new_param.to(net_param.device))
                        fell = 1.0
                    else:
                        f.last_net = [x.detach().cpu() for x in f.net.parameters()]
                        f.last = psrn_masked
                f.fell.append(fell)
                f.i += 1
                f.opt.step()
        else:
            f.mon = RestorationFitMonitor(f.net, f.img, f.mask, show_every=show_every, capacity=capacity)
            if name == "eager_update":
                def one(f=f):
                    f.opt.zero_grad()
                    loss, out = f.head(f.reg())
                    loss.backward()
                    f.mon.update(out, loss)
                    f.opt.step()
            else:
                f.it = NativeIteration(f.net, f.head, f.opt, f.z, reg_noise=f.reg, monitor=f.mon)
                one = f.it.step
        forms[name] = one
    return forms, fits


def child(which, blocks, iters, warmup, show_every, lr, out_path):
    import torch          # before the library: libdip_hip.so must bind to the HIP runtime torch has loaded
    ge.build()
    import dip_native
    assert torch.cuda.is_available(), "bench_restore_monitor.py needs an MI355X"
    dev = torch.device("cuda:0")
    forms, fits = _forms(which, dev, warmup + blocks * iters, show_every, lr)
    for _ in range(warmup):
        for name in ORDER:
            forms[name]()
    torch.cuda.synchronize()
    wall = {k: [] for k in ORDER}
    for _ in range(blocks):
        for name in ORDER:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                forms[name]()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) / iters * 1e3)
    a, b, c = (fits[k] for k in ORDER)
    same = all(torch.equal(p, q) and torch.equal(p, r) for p, q, r in zip(a.net.parameters(), b.net.parameters(), c.net.parameters()))
    same_rec = torch.equal(b.mon.records, c.mon.records)
    same_fell = a.fell == b.mon.history()[:, 5].tolist()
    rec = {"size": which, "HW": list(SIZES[which]), "parameters": sum(p.numel() for p in a.net.parameters()),
           "mask": "bernoulli 0.5, one plane", "reg_noise_std": 0.03, "lr": lr, "show_every": show_every, "blocks": blocks,
           "iters_per_block": iters, "warmup": warmup, "order": list(ORDER),
           "wall_ms_per_iteration": {k: _stats(wall[k]) for k in ORDER},
           "iterations_recorded": int(c.mon.i), "fall_backs": int(sum(a.fell)),
           "bit_identical_parameters": bool(same), "bit_identical_records_eager_native": bool(same_rec),
           "same_fall_back_decisions_as_host": bool(same_fell), "last_record": c.mon.last(),
           "device": torch.cuda.get_device_name(0), "host": socket.gethostname(),
           "build_id": dip_native.lib().dip_build_id().decode()}
    with open(out_path, "w") as f:
        json.dump(rec, f)
    print(json.dumps(rec))
    if not (same and same_rec and same_fell):
        raise SystemExit("the three fits diverged")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--show-every", type=int, default=50)
    ap.add_argument("--lr", type=float, default=0.001)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "restore_monitor_bench.json"))
    ap.add_argument("--child", default=None, choices=list(SIZES), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.blocks < 5 or args.iters < 50 or args.warmup < 3 or args.show_every < 1:
        ap.error("at least 5 blocks of at least 50 iterations after at least 3 warm-up iterations")
    if args.child is not None:
        child(args.child, args.blocks, args.iters, args.warmup, args.show_every, args.lr, args.out)
        return
    parts = {s: f"{args.out}.{s}.part" for s in args.sizes}
    steps = [" ".join(["timeout", "-k", "10", str(args.timeout), shlex.quote(sys.executable), shlex.quote(os.path.abspath(__file__)),
                       "--child", s, "--blocks", str(args.blocks), "--iters", str(args.iters), "--warmup", str(args.warmup),
                       "--show-every", str(args.show_every), "--lr", str(args.lr), "--out", shlex.quote(path)])
             for s, path in parts.items()]
    rc = subprocess.run(["bash", "-c", " && ".join(steps)]).returncode          # a failing step ends the chain
    done = {}
    for s, path in parts.items():
        if os.path.exists(path):
            with open(path) as f:
                done[s] = json.load(f)
            os.remove(path)
    if done:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/bench_restore_monitor.py", "results": done}, f, indent=1)
            f.write("\n")
    if rc:
        raise SystemExit(f"a size failed (exit status {rc}); results so far: {sorted(done)}")


if __name__ == "__main__":
    main()
