"""The tail of a dip_group.GroupedFits row -- everything behind the engine's own buffers: net input, noise state, the loss
head's buffers, Adam's state, the monitor's and the early stopping's buffers -- as a fingerprint, for the combinations of MSE /
masked / super-resolution tail, TV term, monitor= and early_stop=: the slab layout, the head's, the monitor's and the early
stopping's launches and descriptors, and the per-instance constants.  The expected values (tests/golden/group_tail_layout.json)
were recorded by running this file as a script at the commit BEFORE the description in question was unified (the tail's; then,
with the restoration and early-stopping cases added, the monitors' buffer tables); pointers are written relative to the row's own buffers, so the engine's layout may change
without disturbing them.  Host memory only (_dry_cpu: nothing can be launched)."""
import ctypes as C
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "group_tail_layout.json")
B, HW, LR = 2, (64, 96), (16, 24)
CASES = ("a_mse", "b_mse_mask_noise_ema", "c_mse_mask_noise_monitor_backtracking", "d_mse_monitor_records_only",
         "e_sr", "f_sr_tv", "g_sr_monitor_hr", "h_sr_tv_monitor",
         "i_mse_mask_restore_backtracking", "j_mse_mask_restore_records_only", "k_mse_early_stop_wmv",
         "l_mse_early_stop_emv_no_params", "m_mse_mask_restore_early_stop_emv", "n_sr_monitor_hr_early_stop_wmv")


def _group(case):
    from dip_group import GroupedFits
    from test_group_sr_host import _down, _small
    from utils.fit_monitor import (GroupedEarlyStopMonitor, GroupedFitMonitor, GroupedRestorationFitMonitor,
                                   GroupedSRFitMonitor)
    gen = torch.Generator().manual_seed(3)
    rand = lambda c, hw: [torch.rand(1, c, *hw, generator=gen) for _ in range(B)]
    zs = [z * 0.1 for z in rand(8, HW)]
    nets = [_small(b) for b in range(B)]
    kw = dict(seeds=[5, 6], device="cpu", _dry_cpu=True)
    if case[0] in "abcdijklm":
        ts = rand(3, HW)
        if case[0] in "bcijm":
            kw.update(masks=[(m > 0.5).float() for m in rand(1, HW)], reg_noise_std=1 / 30.)
        if case[0] == "b":
            kw.update(exp_weight=0.99)
        if case[0] == "c":
            kw.update(monitor=GroupedFitMonitor(rand(3, HW), exp_weight=0.9, show_every=4, backtracking=True, capacity=24))
        if case[0] == "d":
            kw.update(monitor=GroupedFitMonitor(None, exp_weight=0.9, show_every=4, backtracking=False, capacity=24))
        if case[0] in "ijm":
            kw.update(monitor=GroupedRestorationFitMonitor(show_every=4, backtracking=case[0] != "j", capacity=24))
        if case[0] == "k":
            kw.update(early_stop=GroupedEarlyStopMonitor(mode="wmv", window=4, patience=3, capacity=24))
        if case[0] == "l":
            kw.update(early_stop=GroupedEarlyStopMonitor(mode="emv", alpha=0.25, patience=3, keep_params=False, capacity=24))
        if case[0] == "m":
            kw.update(early_stop=GroupedEarlyStopMonitor(mode="emv", capacity=24))
        return GroupedFits(nets, zs, ts, **kw)
    downs = [_down() for _ in range(B)]
    with torch.no_grad():
        for b, d in enumerate(downs):
            d._taps.mul_(1.0 + 0.25 * b)
    if case[0] in "fh":
        kw.update(tv_weights=[1e-6, 3e-6])
    if case[0] in "gn":
        kw.update(monitor=GroupedSRFitMonitor(rand(3, HW), capacity=24))
    if case[0] == "n":
        kw.update(early_stop=GroupedEarlyStopMonitor("wmv", window=4, capacity=24))
    if case[0] == "h":
        kw.update(monitor=GroupedSRFitMonitor(None, capacity=24))
    return GroupedFits(nets, zs, rand(3, LR), downsamplers=downs, reg_noise_std=0.03, **kw)


def _fingerprint(g):
    ex = g._row0_extra
    base = g._off(ex["saved"])
    where = {t.data_ptr(): "ex:" + k for k, t in ex.items() if t is not None}
    lo = g.mem.data_ptr()

    def pointer(v):
        if not v:
            return None
        return where.get(v) or ("engine" if lo <= v < lo + g.stride else "outside")

    def struct(s):
        out = {}
        for f, ty in s._fields_:
            v = getattr(s, f)
            out[f] = struct(v) if isinstance(v, C.Structure) else pointer(v) if ty is C.c_void_p else v
        return out

    descs = {id(g._head): "&head"}
    if g.monitor is not None:
        descs[id(g._mdesc)] = "&mdesc"
    if g.early_stop is not None:
        descs[id(g._edesc)] = "&edesc"

    def launches(ops):
        return [[name, [descs[id(a._obj)] if hasattr(a, "_obj") else pointer(a) if isinstance(a, int) and a >= 1 << 32 else a
                        for a in args]] for _, args, name in ops]

    return {
        "tail_bytes": g.stride - base,
        "extra": [[k, None if t is None else g._off(t) - base, None if t is None else t.numel(),
                   None if t is None else str(t.dtype)] for k, t in ex.items()],
        "head_fwd": launches(g._head_fwd), "head_bwd": launches(g._head_bwd),
        "mon": launches(g._mon) if g.monitor is not None else None,
        "es": launches(g._es) if g.early_stop is not None else None,
        "with_out_conv": g._with_out_conv,
        "head": [type(g._head).__name__, struct(g._head)],
        "mdesc": [type(g._mdesc).__name__, struct(g._mdesc)] if g.monitor is not None else None,
        "edesc": [type(g._edesc).__name__, struct(g._edesc)] if g.early_stop is not None else None,
        "values": {k: [g._inst(ex[k], b).tolist() for b in range(B)]
                   for k in ("tv_weight", "gl", "rng", "mon_state", "mon_counter", "es_state", "es_counter") if ex.get(k) is not None},
    }


@pytest.mark.parametrize("case", CASES)
def test_tail_layout_and_launches_are_the_recorded_ones(built, case):
    with open(GOLDEN) as fh:
        want = json.load(fh)[case]
    g = _group(case)
    assert g.pointers_outside_row0() == []
    assert hasattr(g, "_mdesc") == (g.monitor is not None)
    assert hasattr(g, "_edesc") == (g.early_stop is not None)
    got = json.loads(json.dumps(_fingerprint(g)))
    for k in want:
        assert got[k] == want[k], (case, k)
    assert got == want


if __name__ == "__main__":
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    import __graft_entry__ as ge
    ge.build()
    with open(GOLDEN, "w") as fh:
        json.dump({case: _fingerprint(_group(case)) for case in CASES}, fh, indent=1, sort_keys=False)
        fh.write("\n")
