"""CPU suite of the ring-free early-stopping criterion and of grouped early stopping (dip_early_stop_emv_dev,
DipEarlyStopEmvDesc; utils.fit_monitor.EarlyStopMonitor(mode='emv'), GroupedEarlyStopMonitor; dip_group.GroupedFits(
early_stop=)): the entry point is declared, exported, a command-list function and validates on the host before it launches;
the refusals that need no GPU; the memory model of a group with early stopping on host memory (the dry mode); the numpy
restatement of the contract (tests/early_stop_emv_ref.py) on the sequences the GPU tests use."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import early_stop_emv_ref as E
import early_stop_ref as R
from test_group_monitor_host import ALIGN, B, HW, _dry, _problem, _small, _up


# ------------------------------------------------------------------------------------------ 1. the C ABI
def test_symbols_header_and_descriptor(built):
    import dip_native as N
    from utils import fit_monitor as FM
    hdr = open(os.path.join(ROOT, "include", "dip_hip.h")).read()
    assert re.search(r"^int dip_early_stop_emv_dev\(const DipEarlyStopEmvDesc\* d, void\* stream\);", hdr, flags=re.M)
    head = hdr[:hdr.index("typedef struct DipEarlyStopEmvDesc")]
    comment = head[head.rindex("/*"):]
    size = int(re.search(r"sizeof\(DipEarlyStopEmvDesc\) == (\d+)", comment).group(1))
    assert ctypes.sizeof(N.DipEarlyStopEmvDesc) == size == 88
    fields = ["out", "mean", "partial", "records", "state", "counter", "best_out", "n", "alpha", "warmup", "patience", "capacity",
              "reserved"]
    assert [f[0] for f in N.DipEarlyStopEmvDesc._fields_] == fields
    offsets = [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 76, 80, 84]
    assert [getattr(N.DipEarlyStopEmvDesc, f).offset for f in fields] == offsets
    # every field of the header's struct, in order, is a field of the binding's
    body = hdr[hdr.index("typedef struct DipEarlyStopEmvDesc {"):hdr.index("} DipEarlyStopEmvDesc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            names += [re.split(r"[\s\*]+", first.strip())[-1]] + [r.strip().lstrip("*") for r in rest]
    assert names == fields
    assert "dip_early_stop_emv_dev" in N.EXPORTS and hasattr(built, "dip_early_stop_emv_dev")
    assert built.dip_abi_version() == N.ABI_VERSION == 9            # a new entry point, a new struct, no existing one changed
    assert ctypes.sizeof(N.DipEarlyStopDesc) == 96
    for name in ("GroupedEarlyStopMonitor", "early_stop_emv_descriptor", "early_stop_state_fill"):
        assert callable(getattr(FM, name)), name
    from dip_group import GroupedFits
    assert callable(GroupedFits.run_until)


def test_command_list_knows_the_launch(built):
    import dip_native as N
    fid = built.dip_list_fn_id(b"dip_early_stop_emv_dev")
    assert fid >= 0
    assert built.dip_list_fn_nargs(fid) == 2 == len(N._SIGS["dip_early_stop_emv_dev"][1])


def test_validates_on_the_host_before_any_launch(built):
    import dip_native as N
    L = built
    fake = 1 << 20

    def desc(**kw):
        d = N.DipEarlyStopEmvDesc(fake, fake, fake, fake, fake, fake, fake, 192, 0.25, 8, 9, 16, 0)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    assert L.dip_early_stop_emv_dev(None, None) == -1
    assert b"early_stop_emv_dev: NULL descriptor" in L.dip_last_error()
    for f in ("out", "mean", "partial", "records", "state", "counter", "best_out"):
        d = desc(**{f: None})
        assert L.dip_early_stop_emv_dev(ctypes.byref(d), None) == -1, f
        assert b"early_stop_emv_dev: a required pointer is NULL" in L.dip_last_error(), f
    for bad in (dict(n=0), dict(n=-192), dict(patience=0), dict(patience=-1), dict(capacity=0), dict(capacity=-4),
                dict(warmup=0), dict(warmup=-2)):
        d = desc(**bad)
        assert L.dip_early_stop_emv_dev(ctypes.byref(d), None) == -1, bad
        assert b"early_stop_emv_dev: n, patience, capacity and warmup must be > 0" in L.dip_last_error(), bad
    for alpha in (0.0, 1.0, -0.25, 1.5, math.nan, math.inf):
        d = desc(alpha=alpha)
        assert L.dip_early_stop_emv_dev(ctypes.byref(d), None) == -1, alpha
        assert b"early_stop_emv_dev: alpha must be in (0, 1)" in L.dip_last_error(), alpha
    d = desc(n=2 ** 33 + 1)
    assert L.dip_early_stop_emv_dev(ctypes.byref(d), None) == -1
    assert b"early_stop_emv_dev: n must be <= 2^33" in L.dip_last_error()
    # through a command list: the failing command is named
    d = desc(alpha=1.0)
    cl = N.CmdList([("launch", L.dip_early_stop_emv_dev, (ctypes.byref(d),), 0, "early_stop_emv_dev")])
    with pytest.raises(RuntimeError, match=r"early_stop_emv_dev.*alpha must be in \(0, 1\)"):
        cl.run([None])
    assert cl._failed.value == 0


# ------------------------------------------------------------------------------------------ 2. the monitors
def test_constructor_refusals_of_both_monitors():
    import inspect
    from utils.fit_monitor import EarlyStopMonitor, GroupedEarlyStopMonitor, _GroupedRecords
    img = torch.rand(1, 3, 37, 29)
    sig = inspect.signature(EarlyStopMonitor.__init__)
    assert list(sig.parameters)[1:] == ["img_like", "window", "patience", "net", "capacity", "mode", "alpha", "warmup"]
    for k, default in (("mode", "wmv"), ("alpha", 0.1), ("warmup", None)):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default == default
    # bad settings: a ValueError in front of the device check (a CPU image would be a RuntimeError)
    bads = ((dict(mode="ema"), "mode"), (dict(mode=None), "mode"), (dict(mode="emv", alpha=0.0), "alpha"),
            (dict(mode="emv", alpha=1.0), "alpha"), (dict(mode="emv", alpha=float("nan")), "alpha"),
            (dict(mode="emv", warmup=0), "warmup"), (dict(mode="emv", warmup=-3), "warmup"),
            (dict(mode="emv", patience=0), "patience"), (dict(mode="emv", capacity=0), "capacity"), (dict(window=1), "window"))
    for kw, what in bads:
        with pytest.raises(ValueError, match=f"dip-amd: EarlyStopMonitor: {what}"):
            EarlyStopMonitor(img, **kw)
        with pytest.raises(ValueError, match=f"dip-amd: GroupedEarlyStopMonitor: {what}"):
            GroupedEarlyStopMonitor(**kw)
    # 'emv' ignores the window; good settings reach the device check
    with pytest.raises(RuntimeError, match="dip-amd: EarlyStopMonitor.*MI355X"):
        EarlyStopMonitor(img, window=0, mode="emv")
    with pytest.raises(TypeError):
        EarlyStopMonitor(img, 100, 1000, None, 16, "emv")             # the new arguments are keyword-only
    # the grouped monitor: settings only, no device
    m = GroupedEarlyStopMonitor()
    assert isinstance(m, _GroupedRecords) and GroupedEarlyStopMonitor.COLUMNS == EarlyStopMonitor.COLUMNS
    assert (m.mode, m.window, m.alpha, m.warmup, m.patience, m.keep_params, m.capacity) == ("wmv", 100, 0.1, 20, 1000, True, 16384)
    assert GroupedEarlyStopMonitor(mode="emv", alpha=0.25).warmup == 8 and GroupedEarlyStopMonitor(alpha=0.3).warmup == 7
    assert GroupedEarlyStopMonitor(mode="emv", window=0).mode == "emv"
    assert m.records is None and m.state is None and m.group is None and m.i == 0
    for call in (lambda: m.stopped, lambda: m.best_iter, lambda: m.memory_bytes, m.restore_best, m.history):
        with pytest.raises(RuntimeError, match="dip-amd:.*GroupedEarlyStopMonitor.*not been given to a GroupedFits"):
            call()


def test_group_refusals_need_no_gpu(built):
    from dip_group import GroupedFits
    from dip_optim import FusedAdam, NativeIteration
    from utils.common_utils import get_params
    from utils.fit_monitor import EarlyStopMonitor, GroupedEarlyStopMonitor, GroupedFitMonitor
    zs, ts, _ = _problem()
    nets = [_small(k) for k in range(B)]
    kw = dict(device="cpu", _dry_cpu=True)
    for bad in (object(), 3, GroupedFitMonitor(), GroupedEarlyStopMonitor):
        with pytest.raises(TypeError, match="dip-amd: GroupedFits\\(early_stop=\\) takes a utils.fit_monitor.GroupedEarlyStopMonitor"):
            GroupedFits(nets, zs, ts, early_stop=bad, **kw)
    # a solo EarlyStopMonitor (built without its device check) is named
    solo = EarlyStopMonitor.__new__(EarlyStopMonitor)
    with pytest.raises(TypeError, match="dip-amd: GroupedFits\\(early_stop=\\).*got EarlyStopMonitor.*solo EarlyStopMonitor"):
        GroupedFits(nets, zs, ts, early_stop=solo, **kw)
    # ... and a grouped one handed to NativeIteration meets the existing text
    z = torch.rand(1, 8, 32, 48) * 0.1
    opt = FusedAdam(get_params('net', nets[0], z), lr=0.01)
    with pytest.raises(TypeError, match="dip-amd: early_stop must be a utils.fit_monitor.EarlyStopMonitor or None"):
        NativeIteration(nets[0], None, opt, z, early_stop=GroupedEarlyStopMonitor())
    # a refused construction does not adopt; an adopted monitor is adopted once
    es = GroupedEarlyStopMonitor(mode="emv", capacity=5)
    with pytest.raises(ValueError):
        GroupedFits(nets, zs, ts, exp_weight=0.5, monitor=GroupedFitMonitor(), early_stop=es, **kw)
    assert es.group is None and es.records is None
    g = GroupedFits(nets, zs, ts, early_stop=es, **kw)
    with pytest.raises(RuntimeError, match="dip-amd:.*GroupedEarlyStopMonitor already belongs.*adopted once"):
        GroupedFits([_small(9 + k) for k in range(B)], zs, ts, early_stop=es, **kw)
    # capacity: refused before anything is issued (here: before the dry group's own refusal to launch)
    for call in (lambda: g.step(6), lambda: g.run(6), lambda: g.run_until(6, check_every=2)):
        with pytest.raises(RuntimeError, match="dip-amd: GroupedEarlyStopMonitor capacity exceeded"):
            call()
    with pytest.raises(RuntimeError, match="dry"):
        g.run_until(5, check_every=2)
    assert es.i == 0 and g.iterations == 0
    with pytest.raises(ValueError, match="dip-amd: run_until: check_every"):
        g.run_until(5, check_every=0)
    with pytest.raises(RuntimeError, match="dip-amd: GroupedFits.run_until needs early_stop="):
        _dry().run_until(5)
    # restore_best: no minimum yet; keep_params=False keeps best_out only
    with pytest.raises(RuntimeError, match="dip-amd: GroupedEarlyStopMonitor.restore_best: no minimum"):
        es.restore_best()
    with pytest.raises(RuntimeError, match="dip-amd: GroupedEarlyStopMonitor.restore_best: no minimum.*\\[1\\]"):
        es.restore_best(b=1)
    nk = GroupedEarlyStopMonitor(mode="emv", keep_params=False, capacity=5)
    g2 = _dry(early_stop=nk)
    with pytest.raises(RuntimeError, match="dip-amd: GroupedEarlyStopMonitor.restore_best needs keep_params=True"):
        nk.restore_best()
    assert g2.early_stop is nk and nk.best_params is None


# ------------------------------------------------------------------------------------------ 3. the slab of a dry group
@pytest.mark.parametrize("with_monitor", [False, True], ids=["early_stop-only", "behind-monitor"])
@pytest.mark.parametrize("keep", [True, False], ids=["keep_params", "best_out-only"])
@pytest.mark.parametrize("mode", ["wmv", "emv"])
def test_early_stop_buffers_are_rows_of_the_slab(built, mode, keep, with_monitor):
    from utils.fit_monitor import GroupedEarlyStopMonitor, GroupedFitMonitor, early_stop_state
    cap, window = 24, 5
    mon = (lambda: GroupedFitMonitor(None, show_every=4, capacity=cap)) if with_monitor else (lambda: None)
    es = GroupedEarlyStopMonitor(mode=mode, window=window, alpha=0.25, patience=9, keep_params=keep, capacity=cap)
    plain = _dry(mon())
    g = _dry(mon(), early_stop=es)
    assert g.pointers_outside_row0() == []
    assert g.early_stop is es and es.group is g
    # early_stop=None: the stride of a group without the keyword
    assert _dry(mon(), early_stop=None).stride == plain.stride
    # the slab grows by exactly the aligned sum of the early-stop buffers, in the documented order, behind everything else
    n = 3 * HW[0] * HW[1]
    n_arena = g.eng.n_arena
    order = (["es_ring"] if mode == "wmv" else []) + ["es_mean", "es_partial", "es_records", "es_state", "es_counter",
                                                        "es_best_out"] + (["es_best_params"] if keep else [])
    sizes = dict(es_ring=4 * window * n, es_mean=8 * n, es_partial=8 * built.dip_fit_monitor_nblk(n), es_records=4 * 5 * cap,
                 es_state=64, es_counter=4, es_best_out=4 * n, es_best_params=4 * n_arena)
    ex = g._row0_extra
    assert [k for k, t in ex.items() if k.startswith("es_") and t is not None] == order
    off = plain.stride
    for k in order:
        assert g._off(ex[k]) == off and ex[k].numel() * ex[k].element_size() == sizes[k], k
        off += _up(sizes[k])
    assert g.stride == off and g.stride % ALIGN == 0 and g.mem.numel() == B * g.stride
    if mode == "emv":
        assert ex["es_ring"] is None and es.ring is None
    for k, t in plain._row0_extra.items():                          # nothing in front of them moves
        if t is not None:
            assert g._off(ex[k]) == plain._off(t), k
    # the views
    s4 = g.stride // 4
    assert es.records.shape == (B, cap, 5) and es.records.stride() == (s4, 5, 1)
    assert es.state.shape == (B, 16) and es.state.dtype == torch.int32 and es.state.stride() == (s4, 1)
    assert es.counter.shape == (B,) and es.counter.dtype == torch.int32
    assert es.best_out.shape == (B, 3, *HW) and es.mean.shape == (B, n) and es.mean.dtype == torch.float64
    assert (es.ring.shape == (B, window, n)) if mode == "wmv" else es.ring is None
    assert (es.best_params.shape == (B, n_arena)) if keep else es.best_params is None
    per = sum(sizes[k] for k in order)
    assert es.memory_bytes == B * per
    if mode == "emv":
        assert per - sizes["es_mean"] - sizes["es_best_out"] - (sizes["es_best_params"] if keep else 0) < 4096   # 12 n + small
    lo = g.mem.data_ptr()
    for b in range(B):
        for v in (es.records[b], es.state[b], es.counter[b], es.best_out[b], es.mean[b]):
            assert lo + b * g.stride <= v.data_ptr() < lo + (b + 1) * g.stride
        assert torch.equal(es.state[b], early_stop_state("cpu"))    # the row copy carried the initial state
        assert torch.count_nonzero(es.records[b]).item() == 0 and es.counter[b].item() == 0
        assert torch.count_nonzero(es.best_out[b]).item() == 0
    assert es.best_iter == [-1] * B and es.stopped == [0] * B
    # ONE descriptor for all instances, and the launches behind the monitor's
    d = g._edesc
    assert (d.out, d.mean, d.records, d.state, d.counter, d.best_out) == tuple(
        ex[k].data_ptr() for k in ("out", "es_mean", "es_records", "es_state", "es_counter", "es_best_out"))
    assert (d.n, d.patience, d.capacity) == (n, 9, cap)
    if mode == "emv":
        assert (d.alpha, d.warmup) == (0.25, 8)
    else:
        assert (d.ring, d.window) == (ex["es_ring"].data_ptr(), window)
    dev_name = "early_stop_emv_dev" if mode == "emv" else "early_stop_dev"
    assert [name for _, _, name in g._es] == [dev_name] + (["early_stop_keep"] if keep else [])
    es.i = 2
    assert es.history().shape == (B, 2, 5) and [tuple(r) for r in es.last()] == [es.COLUMNS] * B


def test_group_without_early_stop_is_unchanged(built):
    g = _dry()
    assert g.early_stop is None and not any(k.startswith("es_") for k in g._row0_extra)
    assert not hasattr(g, "_edesc") and not hasattr(g, "_es")


def test_docs_describe_grouped_early_stopping():
    import dip_group
    from utils import fit_monitor
    for doc in (dip_group.__doc__, fit_monitor.__doc__):
        assert "GroupedEarlyStopMonitor" in doc and "run_until" in doc and "emv" in doc
    assert "dip_early_stop_emv_dev" in fit_monitor.__doc__
    for name in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "GroupedEarlyStopMonitor" in text and "dip_early_stop_emv_dev" in text, name


# ------------------------------------------------------------------------------------------ 4. the reference helper
EMV = dict(alpha=0.25, warmup=8, patience=9)
DECISIONS = {0: (20, 29), 1: (17, 26), 2: (14, 23)}                 # best_iter, stop of S_b under EMV ...
WMV_DECISIONS = {0: (19, 28), 1: (16, 25), 2: (13, 22)}             # ... and under the windowed form (window 5, patience 9)


@pytest.mark.parametrize("shape", [(3, 37, 29), (1, 8, 8)], ids=["3x37x29", "1x8x8"])
def test_reference_on_the_issue_sequences(shape):
    for b in range(3):
        xs = E.group_sequence(shape, b)
        assert xs.shape == (60, int(np.prod(shape))) and np.array_equal(xs, R.sequence(shape, T=66, seed=b)[3 * b:3 * b + 60])
        rows, stop, margins = E.emv_reference(xs, **EMV)
        best, stop_at = DECISIONS[b]
        assert (int(rows[-1, 2]), stop) == (best, stop_at), b
        assert min(margins) >= 1e-2                                 # no decision hangs on rounding
        assert np.all(np.isinf(rows[:8, :2])) and np.all(rows[:8, 2] == -1) and np.all(rows[:8, 3:] == 0)
        assert np.array_equal(rows[stop_at:], np.repeat(rows[stop_at:stop_at + 1], 60 - stop_at, axis=0))
        assert rows[stop_at, 4] == 1 and rows[stop_at - 1, 4] == 0
        wrows, wstop, wmargins = R.wmv_reference(xs, 5, 9)
        assert (int(wrows[-1, 2]), wstop) == WMV_DECISIONS[b], b
        assert min(wmargins) >= 1e-2
    # without a warm-up the second iteration is a false minimum: v ramps up from zero.  The reason for warmup = ceil(2 / alpha)
    rows, stop, _ = E.emv_reference(E.group_sequence(shape, 0), alpha=0.1, warmup=1, patience=9)
    assert (int(rows[-1, 2]), stop) == (1, 10)


def test_reference_against_a_closed_form():
    """mu_t and v_t of the recurrence, unrolled: mu_t = (1 - a)^t x_0 + a sum_k (1 - a)^(t - k) x_k."""
    rng = np.random.default_rng(11)
    xs = rng.standard_normal((12, 7)).astype(np.float32)
    a = 0.3
    st = {}
    rows, stop, _ = E.emv_reference(xs, a, 1, 100, state=st)
    assert stop is None
    x = xs.astype(np.float64)
    mu = [(1 - a) ** t * x[0] + a * sum((1 - a) ** (t - k) * x[k] for k in range(1, t + 1)) for t in range(12)]
    v = 0.0
    for t in range(1, 12):
        v = (1 - a) * (v + a * np.mean((x[t] - mu[t - 1]) ** 2))
        assert abs(rows[t, 0] - v) <= 1e-12 * v, t
    assert np.allclose(st["mu"], mu[-1], rtol=1e-12, atol=0) and abs(st["v"] - v) <= 1e-12 * v
    # a constant sequence: v == 0 exactly; the first decision (t = warmup) stays the minimum; stops at warmup + patience
    rows, stop, _ = E.emv_reference(np.full((20, 9), 0.3, dtype=np.float32), 0.25, 4, 6)
    assert rows[4, 0] == 0.0 and rows[-1, 2] == 4 and stop == 10
