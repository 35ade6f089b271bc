"""CPU suite of the early-stopping monitor (utils.fit_monitor.EarlyStopMonitor, dip_early_stop_dev, dip_early_stop_keep,
DipEarlyStopDesc, NativeIteration(early_stop=) / run_until): the entry points are declared, exported, command-list functions
and validate on the host before they launch; the refusals that need no GPU; the numpy restatement of the contract
(tests/early_stop_ref.py) against a brute-force loop."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import early_stop_ref as R


def _small(seed=0):
    from models.skip import skip
    torch.manual_seed(seed)
    return skip(4, 3, num_channels_down=[8, 8], num_channels_up=[8, 8], num_channels_skip=[4, 4],
                upsample_mode="bilinear", need_sigmoid=True, need_bias=True, pad="reflection")


# ------------------------------------------------------------------------------------------ 1. the C ABI
def test_symbols_header_and_descriptor(built):
    import dip_native as N
    from utils import fit_monitor as FM
    hdr = open(os.path.join(ROOT, "include", "dip_hip.h")).read()
    assert re.search(r"^int dip_early_stop_dev\(const DipEarlyStopDesc\* d, void\* stream\);", hdr, flags=re.M)
    assert re.search(r"^int dip_early_stop_keep\(const float\* src, float\* dst, int64_t n, const void\* state, void\* stream\);",
                     hdr, flags=re.M)
    head = hdr[:hdr.index("typedef struct DipEarlyStopDesc")]
    comment = head[head.rindex("/*"):]
    assert "out.detach().cpu()" in comment                          # what the entry point replaces
    size = int(re.search(r"sizeof\(DipEarlyStopDesc\) == (\d+)", comment).group(1))
    assert ctypes.sizeof(N.DipEarlyStopDesc) == size == 96
    fields = ["out", "ring", "mean", "partial", "records", "state", "counter", "best_out", "n", "window", "patience",
              "capacity", "loss"]
    assert [f[0] for f in N.DipEarlyStopDesc._fields_] == fields
    offsets = [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 76, 80, 88]
    assert [getattr(N.DipEarlyStopDesc, f).offset for f in fields] == offsets
    # every field of the header's struct, in order, is a field of the binding's
    body = hdr[hdr.index("typedef struct DipEarlyStopDesc {"):hdr.index("} DipEarlyStopDesc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            names += [re.split(r"[\s\*]+", first.strip())[-1]] + [r.strip().lstrip("*") for r in rest]
    assert names == fields
    for name in ("dip_early_stop_dev", "dip_early_stop_keep"):
        assert name in N.EXPORTS and hasattr(built, name)
    assert built.dip_abi_version() == N.ABI_VERSION == 9            # new entry points, a new struct, no existing one changed
    assert ctypes.sizeof(N.DipFitMonitorDesc) == 104 and ctypes.sizeof(N.DipSRMonitorDesc) == 88
    assert ctypes.sizeof(N.DipRestoreMonitorDesc) == 104
    for name in ("EarlyStopMonitor", "early_stop_state", "early_stop_descriptor", "early_stop_launches"):
        assert callable(getattr(FM, name)), name
    from dip_optim import NativeIteration
    assert callable(NativeIteration.run_until)


def test_command_list_knows_the_launches(built):
    import dip_native as N
    for name, nargs in (("dip_early_stop_dev", 2), ("dip_early_stop_keep", 5)):
        fid = built.dip_list_fn_id(name.encode())
        assert fid >= 0, name
        assert built.dip_list_fn_nargs(fid) == nargs == len(N._SIGS[name][1]), name


def test_validates_on_the_host_before_any_launch(built):
    import dip_native as N
    L = built
    fake = 1 << 20

    def desc(**kw):
        d = N.DipEarlyStopDesc(fake, fake, fake, fake, fake, fake, fake, fake, 192, 5, 9, 16, None)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    assert L.dip_early_stop_dev(None, None) == -1
    assert b"early_stop_dev: NULL descriptor" in L.dip_last_error()
    for f in ("out", "ring", "mean", "partial", "records", "state", "counter", "best_out"):
        d = desc(**{f: None})
        assert L.dip_early_stop_dev(ctypes.byref(d), None) == -1, f
        assert b"early_stop_dev: a required pointer is NULL" in L.dip_last_error(), f
    for bad in (dict(n=0), dict(n=-192), dict(window=0), dict(window=-3), dict(patience=0), dict(patience=-1), dict(capacity=0),
                dict(capacity=-4)):
        d = desc(**bad)
        assert L.dip_early_stop_dev(ctypes.byref(d), None) == -1, bad
        assert b"early_stop_dev: n, window, patience and capacity must be > 0" in L.dip_last_error(), bad
    d = desc(window=1)
    assert L.dip_early_stop_dev(ctypes.byref(d), None) == -1
    assert b"early_stop_dev: window must be >= 2" in L.dip_last_error()
    for bad in (dict(src=None), dict(dst=None), dict(state=None), dict(n=0), dict(n=-1)):
        a = {**dict(src=fake, dst=fake, n=192, state=fake), **bad}
        assert L.dip_early_stop_keep(a["src"], a["dst"], a["n"], a["state"], None) == -1, bad
        assert b"early_stop_keep" in L.dip_last_error(), bad
    # through a command list: the failing command is named
    d = desc(window=1)
    cl = N.CmdList([("launch", L.dip_early_stop_dev, (ctypes.byref(d),), 0, "early_stop_dev")])
    with pytest.raises(RuntimeError, match="early_stop_dev.*window must be >= 2"):
        cl.run([None])
    assert cl._failed.value == 0


# ------------------------------------------------------------------------------------------ 2. the monitor
def test_columns_and_constructor_refusals():
    from models.resnet import ResNet
    from utils.fit_monitor import EarlyStopMonitor, FitMonitor
    assert EarlyStopMonitor.COLUMNS == ("var", "var_min", "best_iter", "wait", "stopped")
    assert EarlyStopMonitor.head_kind is None
    assert EarlyStopMonitor._sync_counter is FitMonitor._sync_counter and EarlyStopMonitor._advance is FitMonitor._advance
    assert EarlyStopMonitor.history is FitMonitor.history and EarlyStopMonitor.last is FitMonitor.last
    for name in ("update", "restore_best", "_plan", "_plan_key", "_plan_keep"):
        assert callable(getattr(EarlyStopMonitor, name)), name
    assert isinstance(EarlyStopMonitor.memory_bytes, property)
    assert "315 MB" in EarlyStopMonitor.__doc__
    img = torch.rand(1, 3, 37, 29)
    with pytest.raises(RuntimeError, match="dip-amd: EarlyStopMonitor.*MI355X"):
        EarlyStopMonitor(img)
    with pytest.raises(RuntimeError, match="dip-amd: EarlyStopMonitor.*MI355X"):
        EarlyStopMonitor(img, window=2, patience=1, net=_small(), capacity=2 ** 24)
    for kw, what in ((dict(window=1), "window"), (dict(window=0), "window"), (dict(patience=0), "patience"),
                     (dict(capacity=0), "capacity"), (dict(capacity=2 ** 24 + 1), "capacity")):
        with pytest.raises(ValueError, match=f"dip-amd: EarlyStopMonitor: {what}"):
            EarlyStopMonitor(img, **kw)
    with pytest.raises(TypeError, match="dip-amd: EarlyStopMonitor"):
        EarlyStopMonitor(None)
    # net=: a skip() net; anything else is refused as the back-tracking monitors refuse it
    with pytest.raises(RuntimeError, match="dip-amd: back-tracking needs a net built by models.skip.skip"):
        EarlyStopMonitor(img, net=torch.nn.Sequential())
    with pytest.raises(NotImplementedError, match="dip-amd: EarlyStopMonitor back-tracking covers skip"):
        EarlyStopMonitor(img, net=ResNet(1, 3, 1, 8))


# ------------------------------------------------------------------------------------------ 3. NativeIteration(early_stop=)
def test_native_iteration_type_check_is_reached_on_the_cpu():
    from dip_optim import FusedAdam, NativeIteration
    from utils.common_utils import get_params
    from utils.fit_monitor import GroupedFitMonitor
    z = torch.rand(1, 4, 32, 48) * 0.1
    net = _small()
    opt = FusedAdam(get_params('net', net, z), lr=0.01)
    for bad in (object(), GroupedFitMonitor(), 3):
        with pytest.raises(TypeError, match="dip-amd: early_stop must be a utils.fit_monitor.EarlyStopMonitor or None"):
            NativeIteration(net, None, opt, z, early_stop=bad)
    # monitor='s own check and its message stand in front of it, unchanged
    with pytest.raises(TypeError, match="dip-amd: monitor must be"):
        NativeIteration(net, None, opt, z, monitor=object(), early_stop=object())
    with pytest.raises(RuntimeError, match="dip-amd:.*CPU"):
        NativeIteration(net, None, opt, z, early_stop=None)
    assert opt.step_count == 0 and opt._groups is None


def test_docs_describe_the_monitor():
    import dip_optim
    from utils import fit_monitor
    for doc in (dip_optim.NativeIteration.__doc__, fit_monitor.__doc__):
        assert "EarlyStopMonitor" in doc and "run_until" in doc
    assert "dip_early_stop_dev" in fit_monitor.__doc__ and "out.detach().cpu()" in fit_monitor.__doc__
    for name in ("README.md", "DESIGN.md"):
        assert "EarlyStopMonitor" in open(os.path.join(ROOT, name)).read(), name
    assert "GroupedFits(early_stop=" in open(os.path.join(ROOT, "README.md")).read()          # said to be out of scope


# ------------------------------------------------------------------------------------------ 4. the reference helper
@pytest.mark.parametrize("shape", [(3, 37, 29), (1, 8, 8), (3, 96, 128)], ids=["3x37x29", "1x8x8", "3x96x128"])
def test_reference_on_the_issue_sequences(shape):
    xs = R.sequence(shape, T=60, seed=0)
    rows, stop, margins = R.wmv_reference(xs, 5, 9)
    assert (rows[-1, 2], stop) == (19, 28)
    assert min(margins) >= 1e-3                                     # no decision hangs on rounding
    assert R.brute_force(xs, 5, 9) == (19, 28)
    assert np.all(np.isinf(rows[:4, :2])) and np.all(rows[:4, 2] == -1) and np.all(rows[:4, 3:] == 0)
    assert np.array_equal(rows[29:], np.repeat(rows[28:29], 31, axis=0)) and rows[28, 4] == 1 and rows[27, 4] == 0


def test_reference_agrees_with_a_brute_force_loop():
    rng = np.random.default_rng(5)
    for W, P, T in ((2, 1, 12), (3, 4, 40), (7, 5, 60), (4, 100, 30)):
        xs = (0.5 + rng.standard_normal((T, 17)) * np.abs(np.linspace(-1, 2, T))[:, None]).astype(np.float32)
        rows, stop, _ = R.wmv_reference(xs, W, P)
        best, bstop = R.brute_force(xs, W, P)
        assert (int(rows[-1, 2]), stop) == (best, bstop), (W, P)
        for t in range(W - 1, T if stop is None else stop + 1):
            v = np.var(xs[t - W + 1:t + 1].astype(np.float64), axis=0).mean()          # per-element mean over the window
            assert abs(rows[t, 0] - v) <= 1e-12 * v, (W, P, t)
    # a constant sequence: variance exactly 0 at t = W - 1, which stays the minimum; stops at W - 1 + P
    rows, stop, _ = R.wmv_reference(np.full((20, 9), 0.3, dtype=np.float32), 4, 6)
    assert rows[3, 0] == 0.0 and rows[-1, 2] == 3 and stop == 9
