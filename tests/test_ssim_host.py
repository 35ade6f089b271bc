"""SSIM without a GPU: the definition as tests/ssim_ref.py restates it (there is nothing else to compare against), the fp32
model of the kernel's order of operations with and without the pivot, and the host side of utils.fit_monitor.SSIMMonitor /
ssim / GroupedSSIMMonitor, NativeIteration(ssim=) and GroupedFits(ssim=): every refusal that needs no GPU, the buffer table, and
the slab layout of a dry (host-memory) group."""
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT

import ssim_ref as R

SIZES = [(3, 11, 11), (1, 11, 75), (3, 27, 75), (3, 33, 129), (1, 12, 140), (3, 64, 64)]


# ------------------------------------------------------------------------------------------ 1. the definition
@pytest.mark.parametrize("chw", [(3, 11, 11), (1, 12, 75), (4, 33, 40)])
def test_reference_identity_symmetry_and_constants(chw):
    out, gt = R.inputs(*chw, "noisy")
    assert torch.equal(R.ssim_map(gt, gt), torch.ones(1, chw[0], chw[1] - 10, chw[2] - 10, dtype=torch.float64))
    assert R.ssim(gt, gt) == 1.0
    assert torch.equal(R.ssim_map(out, gt), R.ssim_map(gt, out))
    assert tuple(R.ssim_map(out, gt).shape) == (1, chw[0], chw[1] - 10, chw[2] - 10)
    assert R.ssim(out, gt) < 1.0
    c1, _ = R.constants()
    for a, b in ((0.7, 0.3), (0.0, 1.0), (0.25, 0.25)):
        got = R.ssim_map(torch.full((1, *chw), a), torch.full((1, *chw), b))
        a, b = float(np.float32(a)), float(np.float32(b))
        assert (got - (2 * a * b + c1) / (a * a + b * b + c1)).abs().max().item() < 1e-10
    dr = 255.0
    assert abs(R.ssim(out.double() * dr, gt.double() * dr, data_range=dr) - R.ssim(out, gt)) < 1e-12
    with pytest.raises(ValueError):
        R.ssim_map(torch.zeros(1, 1, 10, 11), torch.zeros(1, 1, 10, 11))


def test_reference_taps_and_the_kernels_taps():
    g = R.taps64()
    assert len(g) == 11 and abs(g.sum() - 1.0) < 1e-15 and np.array_equal(g, g[::-1]) and g.argmax() == 5
    assert abs(g[4] / g[5] - np.exp(-1 / 4.5)) < 1e-15
    src = open(os.path.join(ROOT, "deep-image-prior_amd", "csrc", "ssim_kernels.hip")).read()
    body = re.search(r"constexpr float g\[SSIM_WIN\] = \{([^}]*)\}", src).group(1)
    kernel = np.array([np.float32(t.strip().rstrip("f")) for t in body.split(",")], dtype=np.float32)
    assert np.array_equal(kernel, R.taps32())                       # the fp64 taps rounded to fp32, bit for bit


# ------------------------------------------------------------------------------------------ 2. the fp32 model and the pivot
def test_fp32_model_with_and_without_the_pivot():
    """The kernel's order of operations in numpy float32 against torch's own fp32 conv2d evaluation, both against fp64: the
    figures behind the pivot rule, printed; the model with the pivot meets the per-op criterion the GPU test applies to the
    kernel (error <= 2 x torch-fp32's, or the 2e-6 * scale floor)."""
    worst = {"pivot": [0.0, 0.0], "none": [0.0, 0.0], "torch32": [0.0, 0.0]}
    for chw in SIZES:
        for kind in ("noisy", "flat", "constants"):
            out, gt = R.inputs(*chw, kind)
            m64, m32 = R.ssim_map(out, gt), R.ssim_map(out, gt, torch.float32).double()
            err = {"torch32": m32, "pivot": torch.from_numpy(R.model_fp32(out, gt, 0.5)).double(),
                   "none": torch.from_numpy(R.model_fp32(out, gt, None)).double()}
            e = {k: ((v - m64).abs().max().item(), abs(v.mean().item() - m64.mean().item())) for k, v in err.items()}
            print(f"{kind:9s} {chw}: " + "  ".join(f"{k} map {a:.1e} mean {b:.1e}" for k, (a, b) in e.items()))
            scale = m64.abs().max().item()
            assert e["pivot"][0] <= max(2 * e["torch32"][0], 2e-6 * scale), (kind, chw, e)
            assert e["pivot"][1] <= max(2 * e["torch32"][1], 2e-6 * scale), (kind, chw, e)
            if kind != "constants":
                for k in worst:
                    worst[k] = [max(worst[k][0], e[k][0]), max(worst[k][1], e[k][1])]
    print("worst but for two constants: " + "  ".join(f"{k} map {a:.1e} mean {b:.1e}" for k, (a, b) in worst.items()))
    assert worst["pivot"][0] < worst["none"][0] and worst["pivot"][1] < worst["none"][1]
    out, gt = R.inputs(3, 27, 75, "equal")
    assert np.array_equal(R.model_fp32(out, gt), np.ones((1, 3, 17, 65), np.float32))


# ------------------------------------------------------------------------------------------ 3. the C ABI and the buffer table
def test_symbols_header_descriptor_and_nblk(built):
    import dip_native as N
    hdr = open(os.path.join(ROOT, "include", "dip_hip.h")).read()
    assert re.search(r"^int dip_ssim_nblk\(int C, int H, int W\);", hdr, flags=re.M)
    assert re.search(r"^int dip_ssim_dev\(const DipSsimDesc\* d, void\* stream\);", hdr, flags=re.M)
    fields = re.search(r"typedef struct DipSsimDesc \{(.*?)\} DipSsimDesc;", hdr, flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip(" *") for decl in fields.split(";") if decl.strip() for n in decl.strip().split(" ", 1)[1].split(",")]
    names = [n.split("*")[-1].strip() for n in names]
    assert names == [f for f, _ in N.DipSsimDesc._fields_] and "sizeof(DipSsimDesc) == 88" in hdr
    assert N.ABI_VERSION == 9 and built.dip_list_fn_id(b"dip_ssim_dev") >= 0
    th, tw = 16, 64
    for C, H, W in [(1, 11, 11), (3, th + 10, tw + 10), (3, th + 11, tw + 11), (4, 33, 129), (3, 512, 512)]:
        assert built.dip_ssim_nblk(C, H, W) == C * -(-(H - 10) // th) * -(-(W - 10) // tw)
    assert built.dip_ssim_nblk(1, 10, 64) == built.dip_ssim_nblk(1, 64, 10) == built.dip_ssim_nblk(0, 64, 64) == -1
    # refused before any launch (no GPU is touched): -1 and a message
    bad = [N.DipSsimDesc(), N.DipSsimDesc(out=1 << 40, gt=1 << 40, partial=1 << 40, records=1 << 40, C=1, H=10, W=11, nblk=1),
           N.DipSsimDesc(out=1 << 40, gt=1 << 40, partial=1 << 40, records=1 << 40, C=0, H=11, W=11, nblk=1),
           N.DipSsimDesc(out=1 << 40, gt=1 << 40, partial=1 << 40, records=1 << 40, C=1, H=11, W=11, nblk=2),
           N.DipSsimDesc(out=1 << 40, gt=1 << 40, partial=1 << 40, records=1 << 40, counter=1 << 40, C=1, H=11, W=11, nblk=1)]
    for d in bad:
        assert built.dip_ssim_dev(d, None) == -1 and b"ssim_dev" in built.dip_last_error()
    assert built.dip_ssim_dev(None, None) == -1


def test_buffer_table_sizes(built):
    from utils.fit_monitor import SSIM_BUFFERS, monitor_sizes, ssim_descriptor
    assert [b.name for b in SSIM_BUFFERS] == ["gt", "map", "partial", "records", "counter"]
    for img in ((1, 3, 33, 129), (3, 33, 129)):                       # a solo monitor's and a group's
        z = monitor_sizes(SimpleNamespace(capacity=7), built.dip_fit_monitor_nblk, 3 * 33 * 129, img, ())
        n = {b.name: b.count(z) for b in SSIM_BUFFERS}
        assert n == dict(gt=3 * 33 * 129, map=3 * 23 * 119, partial=2 * built.dip_ssim_nblk(3, 33, 129), records=14, counter=1)
        assert SSIM_BUFFERS[1].shape(z) == (*img[:-2], 23, 119) and SSIM_BUFFERS[3].shape(z) == (7, 2)
    m = SimpleNamespace(chw=(3, 33, 129), data_range=2.0, with_avg=False, capacity=7)
    d = ssim_descriptor(m, {})
    assert (d.C, d.H, d.W, d.nblk, d.capacity) == (3, 33, 129, built.dip_ssim_nblk(3, 33, 129), 7)
    assert d.pivot == 1.0 and d.c1 == np.float32(0.02 ** 2) and d.c2 == np.float32(0.06 ** 2) and not d.avg and not d.counter


# ------------------------------------------------------------------------------------------ 4. refusals that need no GPU
def test_refusals_before_a_gpu_is_needed(built):
    from utils.fit_monitor import GroupedSSIMMonitor, SSIMMonitor, ssim
    img = torch.rand(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="dip-amd: SSIMMonitor works on MI355X tensors only"):
        SSIMMonitor(img)
    with pytest.raises(RuntimeError, match="dip-amd: ssim works on MI355X tensors only"):
        ssim(img, img)
    for make in (SSIMMonitor, lambda t, **kw: ssim(t, t, **kw), lambda t, **kw: GroupedSSIMMonitor([t, t], **kw)):
        with pytest.raises(ValueError, match="H and W must be >= 11"):
            make(torch.rand(1, 3, 10, 16))
        with pytest.raises(ValueError, match="H and W must be >= 11"):
            make(torch.rand(1, 3, 16, 10))
        with pytest.raises(ValueError, match=r"must be \[1,C,H,W\]"):
            make(torch.rand(3, 16, 16))
        with pytest.raises(ValueError, match="data_range must be positive"):
            make(img, data_range=0.0)
    with pytest.raises(TypeError, match="dip-amd: SSIMMonitor"):
        SSIMMonitor([1, 3, 16, 16])
    with pytest.raises(ValueError, match="capacity must be > 0"):
        SSIMMonitor(img, capacity=0)
    with pytest.raises(ValueError, match="img_avg must be shaped like img_gt"):
        SSIMMonitor(img, img_avg=torch.rand(1, 3, 16, 17))
    with pytest.raises(ValueError, match="contiguous fp32"):
        SSIMMonitor(img, img_avg=torch.rand(1, 3, 16, 16).double())
    with pytest.raises(ValueError, match="x and y must have one shape"):
        ssim(img, torch.rand(1, 3, 16, 17))
    with pytest.raises(ValueError, match="one ground truth per instance"):
        GroupedSSIMMonitor([])
    with pytest.raises(ValueError, match=r"imgs_gt\[1\] is"):
        GroupedSSIMMonitor([img, torch.rand(1, 3, 16, 17)])
    mon = GroupedSSIMMonitor([img, img], capacity=5)
    assert mon.records is None and mon.counter is None and mon.map is None and mon.i == 0 and mon.group is None
    with pytest.raises(RuntimeError, match="has not been given to a GroupedFits yet"):
        mon.history()


def _small(seed=0):
    from models.skip import skip
    torch.manual_seed(seed)
    return skip(8, 3, num_channels_down=[16, 16], num_channels_up=[16, 16], num_channels_skip=[4, 4], upsample_mode="bilinear",
                need_sigmoid=True, need_bias=True, pad="reflection")


def test_native_iteration_slot_type_errors(built):
    from dip_optim import FusedAdam, NativeIteration
    from utils.fit_monitor import GroupedSSIMMonitor
    net = _small()
    z = torch.rand(1, 8, 32, 32) * 0.1
    opt = FusedAdam(list(net.parameters()), lr=0.01)
    for wrong in (SimpleNamespace(), GroupedSSIMMonitor([torch.rand(1, 3, 32, 32)])):
        with pytest.raises(TypeError, match="dip-amd: ssim must be a utils.fit_monitor.SSIMMonitor or None"):
            NativeIteration(net, None, opt, z, ssim=wrong)


# ------------------------------------------------------------------------------------------ 5. the dry group
B, HW = 2, (64, 96)


def _dry(**kw):
    from dip_group import GroupedFits
    from test_group_sr_host import _small as small
    gen = torch.Generator().manual_seed(3)
    rand = lambda c, hw=HW: [torch.rand(1, c, *hw, generator=gen) for _ in range(B)]
    zs = [z * 0.1 for z in rand(8)]
    return GroupedFits([small(b) for b in range(B)], zs, rand(3), seeds=[5, 6], device="cpu", _dry_cpu=True, **kw), rand


def test_dry_group_plans_the_ssim_rows_behind_everything_else(built):
    from test_group_tail_layout_host import GOLDEN, _fingerprint
    from utils.fit_monitor import GroupedEarlyStopMonitor, GroupedFitMonitor, GroupedSSIMMonitor
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    g0, _ = _dry()
    plain = json.loads(json.dumps(_fingerprint(g0)))
    assert plain == golden["a_mse"] and not hasattr(g0, "_sdesc")      # without the keyword: the recorded layout
    gen = torch.Generator().manual_seed(11)
    gts = [torch.rand(1, 3, *HW, generator=gen) for _ in range(B)]
    mon = GroupedSSIMMonitor(gts, capacity=24)
    g, _ = _dry(ssim=mon)
    assert g.pointers_outside_row0() == []
    got = json.loads(json.dumps(_fingerprint(g)))
    n0 = len(plain["extra"])
    assert got["extra"][:n0] == plain["extra"]                          # everything else is where it was
    nblk = built.dip_ssim_nblk(3, *HW)
    names = [(k, n) for k, _, n, _ in got["extra"][n0:]]
    assert names == [("ssim_gt", 3 * HW[0] * HW[1]), ("ssim_map", None), ("ssim_partial", 2 * nblk), ("ssim_records", 48),
                     ("ssim_counter", 1)]
    offs = [o for _, o, _, _ in got["extra"][n0:] if o is not None]
    assert offs == sorted(offs) and offs[0] >= plain["tail_bytes"] and got["tail_bytes"] > plain["tail_bytes"]
    for k in ("head_fwd", "head_bwd", "head", "with_out_conv"):
        assert got[k] == plain[k]
    assert [name for _, _, name in g._ssim] == ["ssim_dev"]
    d = g._sdesc
    ex = g._row0_extra
    at = lambda k: ex[k].data_ptr()
    assert (d.out, d.gt, d.partial, d.records, d.counter) == (at("out"), at("ssim_gt"), at("ssim_partial"), at("ssim_records"),
                                                              at("ssim_counter"))
    assert not d.avg and not d.map and (d.C, d.H, d.W, d.nblk, d.capacity) == (3, *HW, nblk, 24)
    # adoption: the views, the instances' own ground truths, and a monitor is adopted once
    assert tuple(mon.records.shape) == (B, 24, 2) and tuple(mon.counter.shape) == (B,) and mon.group is g
    for b in range(B):
        assert torch.equal(g._inst(ex["ssim_gt"], b).view(1, 3, *HW), gts[b])
    with pytest.raises(RuntimeError, match="already belongs to a GroupedFits"):
        _dry(ssim=mon)
    # behind the monitor= and the early_stop= rows; with_avg reads the monitor's out_avg row
    fm = GroupedFitMonitor(None, backtracking=False, capacity=24)
    es = GroupedEarlyStopMonitor(mode="emv", keep_params=False, capacity=24)
    g2, _ = _dry(monitor=fm, early_stop=es, ssim=GroupedSSIMMonitor(gts, with_avg=True, capacity=24))
    keys = [k for k, t in g2._row0_extra.items() if t is not None]
    first = lambda p: min(i for i, k in enumerate(keys) if k.startswith(p))
    last = lambda p: max(i for i, k in enumerate(keys) if k.startswith(p))
    assert last("mon_") < first("es_") <= last("es_") < first("ssim_") and last("ssim_") == len(keys) - 1
    assert g2._sdesc.avg == g2._row0_extra["mon_avg"].data_ptr() and g2.pointers_outside_row0() == []


def test_group_refusals(built):
    from utils.fit_monitor import GroupedSSIMMonitor, SSIMMonitor
    gen = torch.Generator().manual_seed(11)
    gts = [torch.rand(1, 3, *HW, generator=gen) for _ in range(B)]
    with pytest.raises(TypeError, match=r"GroupedFits\(ssim=\) takes a utils.fit_monitor.GroupedSSIMMonitor"):
        _dry(ssim=SimpleNamespace())
    with pytest.raises(ValueError, match="has 3 imgs_gt for 2 instances"):
        _dry(ssim=GroupedSSIMMonitor(gts + gts[:1]))
    with pytest.raises(ValueError, match=r"imgs_gt\[0\] is .* the net output is"):
        _dry(ssim=GroupedSSIMMonitor([t[..., :48] for t in gts]))
    with pytest.raises(ValueError, match="needs monitor=GroupedFitMonitor"):
        _dry(ssim=GroupedSSIMMonitor(gts, with_avg=True))
    with pytest.raises(NotImplementedError, match="with exp_weight= is not implemented"):
        _dry(ssim=GroupedSSIMMonitor(gts, with_avg=True), exp_weight=0.99)
    mon = GroupedSSIMMonitor(gts, capacity=2)
    g, _ = _dry(ssim=mon)
    with pytest.raises(RuntimeError, match="GroupedSSIMMonitor capacity exceeded"):
        g.step(3)
