"""Per-instance learning rate and input-noise level without a GPU: the three entry points that read the scalar from device
memory (dip_adam_tick_dev, dip_noise_axpy_dev3, dip_noise_axpy_dev1s) in the header, the library, the command-list table and
the binding; what they refuse; every refusal of FusedAdam(device_lr=), RegNoise(device_std=) and GroupedFits(lr=[...],
reg_noise_std=[...]) that is raised before a GPU is needed; and the slab of a group built with lists -- the rows of the same
group built with floats, as tests/golden/group_tail_layout.json recorded them at the parent commit, plus one fp64 and one fp32
row behind them."""
import ctypes as C
import json
import os
import re

import pytest
import torch

from conftest import ROOT

NEW = ("dip_adam_tick_dev", "dip_noise_axpy_dev3", "dip_noise_axpy_dev1s")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "group_tail_layout.json")


# ------------------------------------------------------------------------------------------ 1. the C ABI
def test_entry_points_are_declared_exported_registered_and_bound(built):
    import dip_native as N
    hdr = open(os.path.join(ROOT, "include", "dip_hip.h")).read()
    declared = set(re.findall(r"^\s*int\s+(dip_[a-z0-9_]+)\s*\(", hdr, flags=re.M))
    raw = C.CDLL(N.LIB_PATH)
    for name in NEW:
        assert name in declared and name in N.EXPORTS and hasattr(raw, name), name
        fid = built.dip_list_fn_id(name.encode())
        assert fid >= 0 and built.dip_list_fn_nargs(fid) == len(N._SIGS[name][1]), name
    assert "#define DIP_ABI_VERSION 9\n" in hdr and built.dip_abi_version() == N.ABI_VERSION == 9
    # the prototypes: pointers where the scalars were
    sig = lambda name: re.search(r"int\s+%s\s*\(([^)]*)\)" % name, hdr).group(1)
    assert "const double* lr_dev" in sig("dip_adam_tick_dev") and "double lr" not in sig("dip_adam_tick_dev")
    for name in NEW[1:]:
        assert "const float* sigma_dev" in sig(name) and "float sigma" not in sig(name), name
    assert "uint64_t seed" in sig("dip_noise_axpy_dev1s") and "uint64_t seed" not in sig("dip_noise_axpy_dev3")


def test_null_pointers_and_empty_extents_are_refused(built):
    """Every refusal returns -1 with a message that names the entry point, before anything is launched (so a box without a GPU
    sees the refusal, not hipErrorNoDevice)."""
    L = built
    buf = (C.c_char * 256)()
    p = C.addressof(buf)

    def refused(rc, who):
        assert rc == -1 and who.encode() in L.dip_last_error(), (who, rc, L.dip_last_error())

    refused(L.dip_adam_tick_dev(None, p, 0.9, 0.999, None), "adam_tick_dev")
    refused(L.dip_adam_tick_dev(p, None, 0.9, 0.999, None), "adam_tick_dev")
    for z, out, n, sig, st in ((None, p, 4, p, p), (p, None, 4, p, p), (p, p, 4, None, p), (p, p, 4, p, None), (p, p, 0, p, p),
                               (p, p, -3, p, p)):
        refused(L.dip_noise_axpy_dev3(z, out, n, sig, st, None), "noise_axpy_dev3")
        refused(L.dip_noise_axpy_dev1s(z, out, n, sig, 7, st, None), "noise_axpy_dev1s")


# ------------------------------------------------------------------------------------------ 2. solo fits
BAD = (float("nan"), float("inf"), -0.01, "0.1", None, True)


def test_fused_adam_device_lr_refusals():
    from dip_optim import FusedAdam
    p = [torch.zeros(4)]
    for bad in BAD:
        with pytest.raises(ValueError, match="dip-amd:.*lr"):
            FusedAdam(p, lr=bad, device_lr=True)
    opt = FusedAdam(p, lr=0.01, device_lr=True)
    key = opt._plan_key()
    for bad in BAD:
        with pytest.raises(ValueError, match="dip-amd:.*set_lr"):
            opt.set_lr(bad)
    assert opt.lr == 0.01
    opt.set_lr(1e-3)                                  # (no scalar exists yet: the mirror alone; the scalar is created from it)
    opt.set_lr(0)
    assert opt.lr == 0.0 and isinstance(opt.lr, float)
    # the key: the same length, the scalar's identity where the value stood, and the setter does not move it
    plain = FusedAdam(p, lr=0.01)
    assert len(key) == len(plain._plan_key()) == 4 and plain._plan_key()[0] == 0.01
    assert opt._plan_key() == key and key[0] != 0.01 and key[1:3] == plain._plan_key()[1:3]
    with pytest.raises(RuntimeError, match="dip-amd:.*device_lr=True"):
        plain.set_lr(0.1)
    assert plain.lr == 0.01


def test_reg_noise_device_std_refusals():
    from utils.reg_noise import RegNoise, check_level
    z = torch.zeros(1, 2, 4, 4)
    for bad in BAD:
        with pytest.raises(ValueError, match="dip-amd:.*reg_noise_std"):
            RegNoise(z, bad, device_std=True)                         # (before the "MI355X tensors only" refusal)
        with pytest.raises(ValueError, match="dip-amd:.*set_std"):
            check_level(bad, "RegNoise.set_std")
    with pytest.raises(RuntimeError, match="MI355X"):
        RegNoise(z, 0.05, device_std=True)
    assert check_level(0, "x") == 0.0 and check_level(1 / 20., "x") == 0.05
    # without the keyword set_std() is refused and names it (an object that never reached a device: the refusal needs none)
    reg = RegNoise.__new__(RegNoise)
    reg.device_std, reg.std = False, 0.05
    with pytest.raises(RuntimeError, match="dip-amd:.*device_std=True"):
        reg.set_std(0.03)
    assert reg.std == 0.05


# ------------------------------------------------------------------------------------------ 3. grouped fits
B = 2


def _dry(**kw):
    from dip_group import GroupedFits
    from test_group_sr_host import _small
    gen = torch.Generator().manual_seed(3)
    zs = [torch.rand(1, 8, 36, 52, generator=gen) * 0.1 for _ in range(B)]
    ts = [torch.rand(1, 3, 36, 52, generator=gen) for _ in range(B)]
    return GroupedFits([_small(b) for b in range(B)], zs, ts, device="cpu", _dry_cpu=True, **kw)


def test_group_lists_are_validated_before_anything_needs_a_gpu(built):
    for what in ("lr", "reg_noise_std"):
        for bad in ([0.01], [0.01] * 3, [0.01, float("nan")], [float("inf"), 0.01], [0.01, -0.01], [0.01, "x"], [None, 0.01],
                    [True, 0.01]):
            with pytest.raises(ValueError, match="dip-amd:.*%s" % what):
                _dry(**{what: bad})
    with pytest.raises(ValueError, match="dip-amd:.*mixes zero and positive"):
        _dry(reg_noise_std=[0.0, 0.05])
    # all zeros is the float 0; a zero lr is a value like any other
    g = _dry(reg_noise_std=[0.0, 0.0], lr=[0.0, 0.1])
    assert g.std == 0.0 and "reg_std" not in g._row0_extra and g._row0_extra["noisy"] is None and g.lr == [0.0, 0.1]
    # a group built with floats has no rows to rewrite
    f = _dry(lr=0.01, reg_noise_std=1 / 30.)
    assert f.lr == 0.01 and f.std == 1 / 30. and "lr" not in f._row0_extra and "reg_std" not in f._row0_extra
    with pytest.raises(ValueError, match="dip-amd:.*set_lr.*construct the group with a list"):
        f.set_lr([0.1, 0.1])
    with pytest.raises(ValueError, match="dip-amd:.*set_reg_noise_std.*construct the group with a list"):
        f.set_reg_noise_std([0.1, 0.1])
    # the setters: the same validation; they rewrite the rows (host memory here) and the mirrors
    s = _dry(lr=[0.01, 0.1], reg_noise_std=[1 / 30., 1 / 20.])
    ex = s._row0_extra
    assert [s._inst(ex["lr"], b).item() for b in range(B)] == [0.01, 0.1] and ex["lr"].dtype == torch.float64
    assert [s._inst(ex["reg_std"], b).item() for b in range(B)] == [torch.tensor(v).float().item() for v in (1 / 30., 1 / 20.)]
    for bad in ([0.01], [0.01, float("nan")], [0.01, -1.0], float("inf"), "x"):
        with pytest.raises(ValueError, match="dip-amd:.*lr"):
            s.set_lr(bad)
        with pytest.raises(ValueError, match="dip-amd:.*reg_noise_std"):
            s.set_reg_noise_std(bad)
    assert s.lr == [0.01, 0.1] and s.std == [1 / 30., 1 / 20.]
    s.set_lr([1e-3] * B)
    s.set_reg_noise_std([0.0, 0.03])                                  # (at run time an instance may go to 0)
    assert s.lr == [1e-3] * B and s.std == [0.0, 0.03]
    assert [s._inst(ex["lr"], b).item() for b in range(B)] == [1e-3] * B
    assert [s._inst(ex["reg_std"], b).item() for b in range(B)] == [0.0, torch.tensor(0.03).float().item()]
    s.set_lr(0.05)                                                    # (one float serves all)
    assert s.lr == [0.05] * B and [s._inst(ex["lr"], b).item() for b in range(B)] == [0.05] * B


@pytest.mark.parametrize("case,lists", [("a_mse", ("lr",)), ("b_mse_mask_noise_ema", ("lr", "reg_std")),
                                        ("b_mse_mask_noise_ema", ("reg_std",)), ("f_sr_tv", ("lr", "reg_std")),
                                        ("m_mse_mask_restore_early_stop_emv", ("lr", "reg_std"))])
def test_slab_of_a_group_with_lists_is_the_float_groups_plus_two_rows(built, monkeypatch, case, lists):
    """The recorded layout of the parent commit (tests/golden/group_tail_layout.json) is the yardstick: the group built with
    floats has it; the group built with lists has every row of it at the same offset, the new rows behind them -- 256 bytes
    each, `lr` first -- and the head's and the monitors' launches and descriptors unchanged."""
    import dip_group
    import test_group_tail_layout_host as T
    with open(GOLDEN) as fh:
        want = json.load(fh)[case]
    got = json.loads(json.dumps(T._fingerprint(T._group(case))))
    assert got["tail_bytes"] == want["tail_bytes"] and got["extra"] == want["extra"]
    real = dip_group.GroupedFits
    noise = {"a_mse": 0.0, "f_sr_tv": 0.03}.get(case, 1 / 30.)

    def with_lists(*a, **kw):
        if "lr" in lists:
            kw["lr"] = [0.01, 0.1]
        if "reg_std" in lists:
            kw["reg_noise_std"] = [noise, noise * 1.5]
        return real(*a, **kw)

    monkeypatch.setattr(dip_group, "GroupedFits", with_lists)
    g = T._group(case)
    monkeypatch.undo()
    assert g.pointers_outside_row0() == []
    got = json.loads(json.dumps(T._fingerprint(g)))
    rows = [["lr", 1, "torch.float64"], ["reg_std", 1, "torch.float32"]]
    extra = [[name, want["tail_bytes"] + 256 * k, n, dt] for k, (name, n, dt) in enumerate(r for r in rows if r[0] in lists)]
    assert got["extra"] == want["extra"] + extra
    assert got["tail_bytes"] == want["tail_bytes"] + 256 * len(lists)
    for k in want:
        if k not in ("extra", "tail_bytes"):
            assert got[k] == want[k], (case, k)
    ex = g._row0_extra
    if "lr" in lists:
        assert [g._inst(ex["lr"], b).item() for b in range(T.B)] == [0.01, 0.1]
    if "reg_std" in lists:
        assert [g._inst(ex["reg_std"], b).item() for b in range(T.B)] == \
            [torch.tensor(v).float().item() for v in (noise, noise * 1.5)]


def test_grouped_iteration_issues_the_device_scalar_launches(built):
    """The host side of a grouped iteration with lists, without a GPU, the way tests/test_host.py walks the float group: every
    launch goes through the real C ABI (marshalling, the slab range check of the two new pointers) and fails at hipLaunchKernel
    with "no ROCm-capable device" (rc 100); anything else fails the walk.  With lists the two device-scalar entry points stand
    where dip_adam_tick and dip_noise_axpy_dev2 stood; with floats the names are the parent's."""
    import subprocess
    import sys
    code = r"""
import sys, contextlib, torch
assert torch.cuda.device_count() == 0, "a GPU is visible: the walk launches with host pointers and must not reach one"
sys.path.insert(0, %r)
import dip_native as N
from models.skip import skip
import dip_group as G
seen = []
real = N.check
def check(rc, what=""):
    seen.append((what, rc))
    if rc not in (0, 100):
        real(rc, what)
N.check = check
class FakeStream:
    cuda_stream = None
torch.cuda.current_stream = lambda d=None: FakeStream()
torch.cuda.device = lambda d: contextlib.nullcontext()
torch.cuda.is_current_stream_capturing = lambda: False
def net(seed):
    torch.manual_seed(seed)
    return skip(8, 3, num_channels_down=[16, 32, 32], num_channels_up=[16, 32, 32], num_channels_skip=[4, 4, 4],
                upsample_mode="bilinear", need_sigmoid=True, need_bias=True, pad="reflection")
B = 3
def walk(**kw):
    del seen[:]
    g = G.GroupedFits([net(k) for k in range(B)], [torch.rand(1, 8, 32, 64) * 0.1 for _ in range(B)],
                      [torch.rand(1, 3, 32, 64) for _ in range(B)], device="cpu", _dry_cpu=True, **kw)
    g._dry = False
    g.step(2)
    assert N.lib().dip_group_size() == 1 and g.iterations == 2
    return [w for w, rc in seen if rc == 100]
lists = walk(lr=[0.01, 0.001, 0.1], reg_noise_std=[1 / 30., 1 / 20., 0.03])
floats = walk(lr=0.01, reg_noise_std=1 / 30.)
for must in ("noise_axpy_dev3", "adam_tick_dev", "adam_step_dev"):
    assert lists.count(must) == 2, (must, lists.count(must))
assert "adam_tick" not in lists and "noise_axpy_dev2" not in lists
for must in ("noise_axpy_dev2", "adam_tick", "adam_step_dev"):
    assert floats.count(must) == 2, (must, floats.count(must))
assert not any(n in floats for n in ("noise_axpy_dev3", "noise_axpy_dev1s", "adam_tick_dev"))
swap = {"noise_axpy_dev3": "noise_axpy_dev2", "adam_tick_dev": "adam_tick"}
assert [swap.get(n, n) for n in lists] == floats
print("WALK_OK", len(lists))
""" % os.path.join(ROOT, "deep-image-prior_amd")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, DIP_TWO_STREAMS="0", DIP_NO_CLIST="1", HIP_VISIBLE_DEVICES="-1",
                                CUDA_VISIBLE_DEVICES="-1"))
    assert "WALK_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
