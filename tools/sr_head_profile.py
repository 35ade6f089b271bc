"""Kernel time of the fused super-resolution tail (dip_sr_loss_fwd / dip_sr_loss_bwd) beside the launches it replaces, from ONE
rocprofv3 kernel trace of bench.py's `sr` problem (default net, 512 x 512, Lanczos2 x4, reg-noise 0.03):

    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python tools/sr_head_profile.py --run 20
    python tools/sr_head_profile.py --summary DIR 20 > profiles/sr_head_kernels.txt

--run N: N iterations of the notebook's spelling (out = net(x); mse(downsampler(out), img_LR)) and then N of the SRHead closure,
on two nets from one seed (the first 3 iterations of each are warm-up and left out of the summary).
--summary: the launches between the output conv and the first backward conv of either form, classified by kernel name.

--tv (after --run N / --summary DIR N): the closure with the TV prior (super-resolution.ipynb:180-181, sr_prior_effect.ipynb:109),
total_loss = mse(out_LR, img_LR) + tv_weight * tv_loss(out_HR), spelled and as SRHead(tv_weight=):

    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python tools/sr_head_profile.py --run 12 --tv
    python tools/sr_head_profile.py --summary DIR 12 --tv > profiles/sr_tv_kernels.txt

(12, not 20: the TV term has no epsilon, and on this smooth synthetic problem a fit of either spelling can meet a pixel with
s == 0 and go NaN from about the 20th iteration on -- DESIGN.md section 7.)

The ATen chain of the spelled TV term has no names of its own (slices are views; sub, pow, add, sum, mul and their backward are
TensorIterator kernels), so the --tv summary goes by position: an ATen kernel launched between the first head_fwd_kernel and the
last head_bwd_kernel launch (the spelled iterations; autograd reaches the net's node after both branches of the loss) and never
after the first sr_loss_fwd_kernel launch (the head's iterations) is one of the launches the head replaces."""
import glob
import os
import re
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP = 3


TV_WEIGHT = 1e-7          # sr_prior_effect.ipynb


def run(n, tv=False):
    import torch          # before the library: libdip_hip.so must bind to the HIP runtime torch has loaded
    import __graft_entry__ as ge
    ge.build()
    import bench
    from dip_optim import FusedAdam
    from models.downsampler import Downsampler
    from utils.common_utils import get_params
    from utils.loss_head import SRHead
    from utils.reg_noise import RegNoise
    from utils.sr_utils import tv_loss
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
        head = None
        if form == "srhead":
            head = SRHead(net, lr, down, tv_weight=TV_WEIGHT) if tv else SRHead(net, lr, down)
        for _ in range(WARMUP + n):
            opt.zero_grad()
            if head is None and tv:
                out = net(reg())
                loss = mse(down(out), lr) + TV_WEIGHT * tv_loss(out)
            elif head is None:
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


NEW_TV = ("sr_loss_fwd_kernel", "sr_tv_fwd_kernel", "sr_tv_reduce_kernel", "sr_loss_bwd_kernel")
REPLACED_HIP = ("lanczos_fwd_kernel", "lanczos_bwd_kernel", "head_bwd_kernel")


def summary_tv(d, n):
    db = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)[0]
    cur = sqlite3.connect(db).cursor()
    launches = {}
    for name, start, end in cur.execute("select name, start, end from kernels order by start"):
        launches.setdefault(re.sub(r"\(anonymous namespace\)::", "", name), []).append((start, (end - start) / 1e3))
    t0 = min(v[0][0] for k, v in launches.items() if any(p in k for p in NEW_TV))  # the head form's first tail
    ta = min(v[0][0] for k, v in launches.items() if "head_fwd_kernel" in k)       # the spelled form's first tail ...
    tb = max(v[-1][0] for k, v in launches.items() if "head_bwd_kernel" in k)      # ... and the end of its last one
    per = WARMUP + n
    tot = {"new": 0.0, "replaced": 0.0}
    print(f"# source: {os.path.basename(db)}; {per} iterations of each form (notebook spelling with the TV term, SRHead(tv_weight=)")
    print(f"# closure) in one trace; the first {WARMUP} iterations of a form are warm-up and left out; an ATen kernel launched")
    print("# inside the spelled iterations and never inside the head's is one the head replaces")
    print(f"{'kernel':86s} {'calls':>6s} {'/iter':>6s} {'avg_us':>8s} {'min_us':>8s} {'max_us':>8s}  side")
    for name in sorted(launches):
        pre = [us for st, us in launches[name] if ta <= st <= tb]
        post = [us for st, us in launches[name] if st >= t0]
        if any(p in name for p in NEW_TV):
            side, v = "new", post
        elif any(p in name for p in REPLACED_HIP) or ("at::" in name and not post):
            side, v = "replaced", pre
        else:
            continue
        if not v:                      # (a set-up launch outside the iterations)
            continue
        if len(v) % per:
            raise SystemExit(f"{name}: {len(v)} launches are no multiple of {per} iterations")
        m = len(v) // per
        v = v[WARMUP * m:]
        a = sum(v) / len(v)
        tot[side] += a * m
        print(f"{name[:86]:86s} {len(v):6d} {m:6d} {a:8.2f} {min(v):8.2f} {max(v):8.2f}  {side}")
    print(f"# kernel time per iteration: new launches {tot['new']:.2f} us, replaced launches {tot['replaced']:.2f} us")


if __name__ == "__main__":
    tv = "--tv" in sys.argv
    if tv:
        sys.argv.remove("--tv")
    if len(sys.argv) >= 3 and sys.argv[1] == "--run":
        run(int(sys.argv[2]), tv)
    elif len(sys.argv) >= 4 and sys.argv[1] == "--summary":
        (summary_tv if tv else summary)(sys.argv[2], int(sys.argv[3]))
    else:
        raise SystemExit(__doc__)
