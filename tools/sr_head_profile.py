"""Kernel time of the fused super-resolution tail (dip_sr_loss_fwd / dip_sr_loss_bwd) beside the launches it replaces, from ONE
rocprofv3 kernel trace of bench.py's `sr` problem (default net, 512 x 512, Lanczos2 x4, reg-noise 0.03):

    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python tools/sr_head_profile.py --run 20
    python tools/sr_head_profile.py --summary DIR 20 > profiles/sr_head_kernels.txt

--run N: N iterations of the notebook's spelling (out = net(x); mse(downsampler(out), img_LR)) and then N of the SRHead closure,
on two nets from one seed (the first 3 iterations of each are warm-up and left out of the summary).
--summary: the launches between the output conv and the first backward conv of either form, classified by kernel name."""
import glob
import os
import re
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP = 3


def run(n):
    import torch          # before the library: libdip_hip.so must bind to the HIP runtime torch has loaded
    import __graft_entry__ as ge
    ge.build()
    import bench
    from dip_optim import FusedAdam
    from models.downsampler import Downsampler
    from utils.common_utils import get_params
    from utils.loss_head import SRHead
    from utils.reg_noise import RegNoise
    dev = torch.device("cuda:0")
    size = bench.CONFIGS["sr"]["size"]
    mse = torch.nn.MSELoss()
    for form in ("spelled", "srhead"):
        torch.manual_seed(0)
        net, depth = bench.build_net("sr")
        net = net.to(dev)
        z, target = bench.make_problem(0, size, depth)
        z, lr = z.to(dev), torch.nn.functional.avg_pool2d(target.to(dev), 4)
        down = Downsampler(n_planes=3, factor=4, kernel_type='lanczos2', phase=0.5, preserve_size=True).to(dev)
        reg, opt = RegNoise(z, 0.03, seed=1234), FusedAdam(get_params('net', net, z), lr=0.01)
        head = SRHead(net, lr, down) if form == "srhead" else None
        for _ in range(WARMUP + n):
            opt.zero_grad()
            if head is None:
                loss = mse(down(net(reg())), lr)
            else:
                loss, _ = head(reg())
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        print(f"[sr_head_profile] {form}: {WARMUP + n} iterations, last loss {loss.item():.6e}")


# the launches between the output conv and the first backward conv, by kernel name: (pattern, side)
NEW = ("sr_loss_fwd_kernel", "loss_reduce_kernel", "sr_loss_bwd_kernel")
REPLACED = ("lanczos_fwd_kernel", "mse_kernel_cuda", "at::native::reduce_kernel", "elementwise_kernel_manual_unroll",
            "lanczos_bwd_kernel", "head_bwd_kernel")          # (manual_unroll: ATen's mse_loss_backward, the one TensorIterator
#                                                               kernel with three operands in this trace)
BOTH = ("head_fwd_kernel",)


def summary(d, n):
    db = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)[0]
    cur = sqlite3.connect(db).cursor()
    launches = {}
    for name, start, end in cur.execute("select name, start, end from kernels order by start"):
        launches.setdefault(re.sub(r"\(anonymous namespace\)::", "", name), []).append((end - start) / 1e3)
    per = WARMUP + n                   # iterations of ONE form in the trace
    tot = {"new": 0.0, "replaced": 0.0}
    print(f"# source: {os.path.basename(db)}; {per} iterations of each form (notebook spelling, SRHead closure) in one trace;")
    print(f"# the first {WARMUP} iterations of a form are warm-up: their launches are left out of the figures below")
    print(f"{'kernel':86s} {'calls':>6s} {'/iter':>6s} {'avg_us':>8s} {'min_us':>8s} {'max_us':>8s}  side")
    avg = {}
    for name in sorted(launches):
        side = next((sd for pats, sd in ((NEW, "new"), (REPLACED, "replaced"), (BOTH, "both")) if any(p in name for p in pats)),
                    None)
        if side is None:
            continue
        v = launches[name]
        forms = 2 if side == "both" else 1
        if len(v) % (per * forms):
            raise SystemExit(f"{name}: {len(v)} launches are no multiple of {per * forms} iterations")
        m = len(v) // (per * forms)    # launches per iteration
        if forms == 2:                 # spelled form first, then the SRHead form: drop each form's warm-up
            v = v[WARMUP * m:per * m] + v[(per + WARMUP) * m:]
        else:
            v = v[WARMUP * m:]
        a = sum(v) / len(v)
        avg[name] = a
        if side in tot:
            tot[side] += a * m
        print(f"{name[:86]:86s} {len(v):6d} {m:6d} {a:8.2f} {min(v):8.2f} {max(v):8.2f}  {side}")
    print(f"# kernel time per iteration: new launches {tot['new']:.2f} us, replaced launches {tot['replaced']:.2f} us")
    lf = [a for k, a in avg.items() if "lanczos_fwd_kernel" in k]
    sf = [a for k, a in avg.items() if "sr_loss_fwd_kernel" in k]
    if lf and sf:
        print(f"# forward alone: sr_loss_fwd_kernel {sf[0]:.2f} us (+ loss_reduce_kernel) vs lanczos_fwd_kernel {lf[0]:.2f} us")


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--run":
        run(int(sys.argv[2]))
    elif len(sys.argv) >= 4 and sys.argv[1] == "--summary":
        summary(sys.argv[2], int(sys.argv[3]))
    else:
        raise SystemExit(__doc__)
