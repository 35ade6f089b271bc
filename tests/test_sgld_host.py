"""CPU suite of the SGLD step and the posterior monitor (dip_adam_sgld_step[_dev], dip_posterior_dev; dip_optim.FusedAdam(
weight_decay=, noise_std=, noise_seed=, noise_params=), dip_group.GroupedFits(weight_decay=, param_noise_std=,
param_noise_seeds=), utils.fit_monitor.PosteriorMonitor): the ABI, the range tables, what is refused at construction, the slab
rows of an SGLD group and which entry point an optimiser dispatches to.  Nothing is launched."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_native_iter_host import _small

import sgld_ref as S


def _arena_offsets(params):
    off, out = 0, []
    for p in params:
        out.append(off)
        off += (p.numel() + 3) // 4 * 4
    return out


# ------------------------------------------------------------------------------------------ ABI
def test_header_binding_and_library_know_the_entry_points(built):
    import dip_native as N
    hdr = open(os.path.join(ROOT, "include", "dip_hip.h")).read()
    assert re.search(r"^int dip_adam_sgld_step_dev\(float\* p, const float\* g, float\* m, float\* v, int64_t n,", hdr, flags=re.M)
    assert re.search(r"^int dip_adam_sgld_step\(float\* p, const float\* g, float\* m, float\* v, int64_t n, double lr,", hdr,
                     flags=re.M)
    assert re.search(r"^int dip_posterior_dev\(const DipPosteriorDesc\* d, void\* stream\);", hdr, flags=re.M)
    assert "typedef struct DipSgldState {" in hdr and "0x53474C4453474C44" in hdr
    for name in ("dip_adam_sgld_step", "dip_adam_sgld_step_dev", "dip_posterior_dev"):
        assert name in N.EXPORTS and hasattr(built, name)
        fid = built.dip_list_fn_id(name.encode())
        assert fid >= 0 and built.dip_list_fn_nargs(fid) == len(N._SIGS[name][1]), name
    assert len(N._SIGS["dip_adam_sgld_step_dev"][1]) == 14 and len(N._SIGS["dip_adam_sgld_step"][1]) == 17
    assert ctypes.sizeof(N.DipSgldState) == 24 and ctypes.sizeof(N.DipPosteriorDesc) == 56
    assert [f for f, _ in N.DipSgldState._fields_] == ["offset", "seed", "std", "pad_"]
    assert built.dip_abi_version() == N.ABI_VERSION == 9           # additions do not bump it
    assert S.KEY == int.from_bytes(b"SGLDSGLD", "big")


def test_entry_points_refuse_before_they_launch(built):
    """What needs no GPU: n <= 0 is a no-op, NULL pointers and a bad table are -1 with the error set."""
    L = built
    P = 1 << 20                                                      # (never dereferenced: refused, or n == 0)
    assert L.dip_adam_sgld_step_dev(None, None, None, None, 0, 0.9, 0.999, 1e-8, 0.0, None, None, None, 0, None) == 0
    assert L.dip_adam_sgld_step(None, None, None, None, -3, 0.01, 0.9, 0.999, 1e-8, 0.0, 1, 0.0, 0, 0, None, 0, None) == 0
    for args in ((None, P, P, P), (P, None, P, P), (P, P, None, P), (P, P, P, None)):
        assert L.dip_adam_sgld_step_dev(*args, 8, 0.9, 0.999, 1e-8, 0.0, P, P, P, 1, None) == -1
        assert b"adam_sgld_step_dev" in L.dip_last_error() and b"NULL" in L.dip_last_error()
        assert L.dip_adam_sgld_step(*args, 8, 0.01, 0.9, 0.999, 1e-8, 0.0, 1, 0.1, 0, 0, P, 1, None) == -1
    assert L.dip_adam_sgld_step_dev(P, P, P, P, 8, 0.9, 0.999, 1e-8, 0.0, None, P, P, 1, None) == -1
    assert b"iteration state" in L.dip_last_error()
    assert L.dip_adam_sgld_step_dev(P, P, P, P, 8, 0.9, 0.999, 1e-8, 0.0, P, P, None, 1, None) == -1
    assert b"range table is NULL" in L.dip_last_error()
    assert L.dip_adam_sgld_step_dev(P, P, P, P, 8, 0.9, 0.999, 1e-8, 0.0, P, P, P, S.MAX_RANGES + 1, None) == -1
    assert b"512" in L.dip_last_error()
    assert L.dip_adam_sgld_step(P, P, P, P, 8, 0.01, 0.9, 0.999, 1e-8, 0.0, 1, 0.1, 0, 0, P, -1, None) == -1
    assert L.dip_posterior_dev(None, None) == -1
    import dip_native as N
    d = N.DipPosteriorDesc(P, P, P, P, P, 8, 0, 1)
    for field in ("out", "mean", "m2", "count", "counter"):
        bad = N.DipPosteriorDesc(P, P, P, P, P, 8, 0, 1)
        setattr(bad, field, None)
        assert L.dip_posterior_dev(ctypes.byref(bad), None) == -1 and b"NULL" in L.dip_last_error(), field
    for n, burn, every in ((0, 0, 1), (8, -1, 1), (8, 0, 0)):
        d.n, d.burn_in, d.every = n, burn, every
        assert L.dip_posterior_dev(ctypes.byref(d), None) == -1


# ------------------------------------------------------------------------------------------ range tables
def test_range_table_of_a_small_net():
    from dip_optim import noise_ranges
    net = _small()
    params = list(net.parameters())
    offs = _arena_offsets(params)
    total = offs[-1] + params[-1].numel()
    got = noise_ranges(params, offs, [p for p in params if p.dim() == 4])
    assert got == S.expected_ranges(params) and len(got) >= 2
    # sorted, disjoint, inside the group; exactly the 4-D parameters' elements; no alignment gap inside a range
    assert all(0 <= b < e <= total for b, e in got)
    assert all(got[k][1] <= got[k + 1][0] for k in range(len(got) - 1))
    m = S.inside(total, got)
    want = np.zeros(total, dtype=bool)
    for p, o in zip(params, offs):
        if p.dim() == 4:
            want[o:o + p.numel()] = True
    assert np.array_equal(m, want) and m.sum() == sum(p.numel() for p in params if p.dim() == 4)
    # the explicit subset: two parameters that are not neighbours, and a weight with its own bias
    convs = [p for p in params if p.dim() == 4]
    sub = [convs[0], convs[-1]]
    assert noise_ranges(params, offs, sub) == S.expected_ranges(params, sub) and len(noise_ranges(params, offs, sub)) == 2
    assert noise_ranges(params, offs, []) == []


def test_adjacent_extents_merge_and_gaps_do_not():
    from dip_optim import noise_ranges
    a, b, c, d = (torch.zeros(*s) for s in ((2, 2, 1, 1), (4, 1, 1, 1), (3, 1, 1, 1), (5,)))     # 4, 4, 3 (gap of 1), 5 elements
    params = [a, b, c, d]
    offs = _arena_offsets(params)
    assert offs == [0, 4, 8, 12]
    assert noise_ranges(params, offs, [a, b, c]) == [(0, 11)] == S.expected_ranges(params)
    assert noise_ranges(params, offs, [a, b, c, d]) == [(0, 11), (12, 17)]                       # the gap at 11 is not noised
    assert noise_ranges(params, offs, [a, c]) == [(0, 4), (8, 11)]


# ------------------------------------------------------------------------------------------ constructor validation
def test_fused_adam_validates_its_sgld_keywords():
    from dip_optim import FusedAdam
    net = _small()
    params = list(net.parameters())
    for kw in (dict(noise_std=-1e-3), dict(weight_decay=-1e-8), dict(noise_std=float("nan")), dict(weight_decay=float("nan"))):
        with pytest.raises(ValueError, match="dip-amd: FusedAdam"):
            FusedAdam(params, lr=0.01, **kw)
    with pytest.raises(ValueError, match="dip-amd:.*not in the optimiser's list"):
        FusedAdam(params, lr=0.01, noise_std=0.01, noise_params=[torch.nn.Parameter(torch.zeros(2, 2, 1, 1))])
    opt = FusedAdam(params, lr=0.01, noise_std=0.01)
    assert opt.sgld and [id(p) for p in opt.noise_params] == [id(p) for p in params if p.dim() == 4]
    with pytest.raises(ValueError, match="dip-amd:.*noise_std must be >= 0"):
        opt.set_noise_std(-1.0)
    opt.set_noise_std(0.0)
    assert opt.sgld and opt.noise_std == 0.0                        # the SGLD entry point stays
    plain = FusedAdam(params, lr=0.01)
    assert not plain.sgld and not FusedAdam(params, lr=0.01, weight_decay=0.0, noise_std=0.0, noise_seed=9).sgld
    with pytest.raises(RuntimeError, match="dip-amd:.*set_noise_std"):
        plain.set_noise_std(0.1)
    assert FusedAdam(params, lr=0.01, weight_decay=5e-8).sgld
    assert "get_params('net,input'" in FusedAdam.__doc__


def test_defaults_dispatch_to_the_plain_adam_entry_point(built):
    """Which entry point an optimiser's step is, on the launch's name and argument count (what NativeIteration's Adam phase
    holds and step() issues): dip_adam_step_dev with the defaults, dip_adam_sgld_step_dev otherwise."""
    import dip_native as N
    from dip_optim import FusedAdam, _Group
    net = _small()
    params = list(net.parameters())
    flat = torch.zeros(16)
    g = _Group([flat[0:8].view(2, 4, 1, 1), flat[8:12]])            # (views of one host tensor: nothing is launched)
    st = torch.zeros(16, dtype=torch.uint8)
    plain = FusedAdam(params, lr=0.01)
    fn, args, name = plain._step_launch(built, g, 0, st)
    assert name == "adam_step_dev" and fn.__name__ == "dip_adam_step_dev" and len(args) + 1 == len(N._SIGS[fn.__name__][1])
    assert plain._plan_key() == (0.01, (0.9, 0.999), 1e-8, id(None))            # the key's Adam part as it always was
    sg = FusedAdam(params, lr=0.01, weight_decay=5e-8, noise_std=0.01, noise_seed=3)
    g.sgld, g.ranges, g.range_table = torch.zeros(3, dtype=torch.int64), [(0, 4)], torch.zeros(1, 2, dtype=torch.int64)
    fn, args, name = sg._step_launch(built, g, 0, st)
    assert name == "adam_sgld_step_dev" and fn.__name__ == "dip_adam_sgld_step_dev"
    assert len(args) + 1 == len(N._SIGS[fn.__name__][1])
    assert args[8] == 5e-8 and args[10] == g.sgld.data_ptr() and args[11] == g.range_table.data_ptr() and args[12] == 1
    sg._groups = [g]
    assert sg._plan_key()[:4] == (0.01, (0.9, 0.999), 1e-8, id(sg._groups)) and len(sg._plan_key()) == 6


def test_posterior_monitor_and_native_iteration_validate():
    from dip_optim import FusedAdam, NativeIteration
    from utils.fit_monitor import POSTERIOR_BUFFERS, PosteriorMonitor
    img = torch.zeros(1, 3, 8, 8)
    with pytest.raises(ValueError, match="dip-amd: PosteriorMonitor: every must be >= 1"):
        PosteriorMonitor(img, 0, every=0)
    with pytest.raises(ValueError, match="dip-amd: PosteriorMonitor: burn_in must be >= 0"):
        PosteriorMonitor(img, -1)
    with pytest.raises(TypeError, match="dip-amd: PosteriorMonitor"):
        PosteriorMonitor([1, 3, 8, 8], 0)
    with pytest.raises(RuntimeError, match="dip-amd: PosteriorMonitor works on MI355X tensors only"):
        PosteriorMonitor(img, 0)
    assert [b.name for b in POSTERIOR_BUFFERS] == ["mean", "m2", "samples", "counter"]
    # a wrong type in posterior= is refused before anything that needs a GPU
    net = _small()
    z = torch.rand(1, 8, 32, 32) * 0.1
    opt = FusedAdam(list(net.parameters()), lr=0.01)
    with pytest.raises(TypeError, match="dip-amd: posterior must be a utils.fit_monitor.PosteriorMonitor"):
        NativeIteration(net, None, opt, z, posterior=SimpleNamespace())
    # the sample count of an iteration range, and the cap
    pm = SimpleNamespace(burn_in=3, every=2)
    count = lambda i: PosteriorMonitor.samples_after(pm, i)
    assert [count(i) for i in range(10)] == [0, 0, 0, 0, 1, 1, 2, 2, 3, 3]
    assert [count(i) for i in range(10)] == [sum(S.is_sample(j, 3, 2) for j in range(i)) for i in range(10)]
    assert PosteriorMonitor.MAX_SAMPLES == 2 ** 24


# ------------------------------------------------------------------------------------------ the grouped slab
def _dry_group(**kw):
    from dip_group import GroupedFits
    gen = torch.Generator().manual_seed(3)
    nets = [_small() for _ in range(3)]
    zs = [torch.rand(1, 8, 36, 52, generator=gen) * 0.1 for _ in nets]
    ts = [torch.rand(1, 3, 36, 52, generator=gen) for _ in nets]
    return GroupedFits(nets, zs, ts, seeds=[5, 6, 7], reg_noise_std=1 / 30., device="cpu", _dry_cpu=True, **kw), nets


def test_grouped_fits_validate_their_sgld_keywords():
    for kw, msg in ((dict(param_noise_std=[0.1, 0.2]), "one float or one per instance"),
                    (dict(param_noise_std=0.1, param_noise_seeds=[1, 2]), "one seed per instance"),
                    (dict(param_noise_std=[0.1, -0.2, 0.3]), "param_noise_std must be >= 0"),
                    (dict(weight_decay=-1.0), "weight_decay must be >= 0")):
        with pytest.raises(ValueError, match=msg):
            _dry_group(**kw)


def test_grouped_slab_rows(built):
    """Keywords unset (or explicit zeros): _row0_extra holds exactly the keys it held; with param_noise_std set, the two new
    rows behind everything else, every pointer inside row 0."""
    plain, _ = _dry_group()
    keys = list(plain._row0_extra)
    assert keys == ["saved", "noisy", "rng", "target", "mask", "out", "partials", "loss", "gl", "m", "v", "iter"]
    zeros, _ = _dry_group(weight_decay=0.0, param_noise_std=[0.0, 0.0, 0.0])
    assert list(zeros._row0_extra) == keys and zeros.stride == plain.stride and not zeros.sgld and not plain.sgld
    g, nets = _dry_group(weight_decay=5e-8, param_noise_std=[0.01, 0.02, 0.03], param_noise_seeds=[11, 2 ** 64 - 1, 13])
    ex = g._row0_extra
    assert list(ex) == keys + ["sgld", "sgld_ranges"] and g.sgld
    assert g.pointers_outside_row0() == []
    for k in keys:                                                  # nothing in front of the new rows moved
        if plain._row0_extra[k] is not None:
            assert g._off(ex[k]) - g._off(ex["saved"]) == plain._off(plain._row0_extra[k]) - plain._off(plain._row0_extra["saved"])
    assert g._off(ex["sgld"]) > max(g._off(ex[k]) for k in keys if ex[k] is not None)
    assert g._off(ex["sgld_ranges"]) > g._off(ex["sgld"]) and g.stride > plain.stride
    assert ex["sgld"].dtype == torch.int64 and ex["sgld"].numel() == 3 and ex["sgld"].data_ptr() % 8 == 0
    want = S.expected_ranges(g.eng.param_list)
    assert g._sgld_ranges == want and ex["sgld_ranges"].tolist() == [x for r in want for x in r]
    assert g._sgld_n == g.eng.slots[-1] + g.eng.param_list[-1].numel() <= g.eng.n_arena
    import dip_native as N
    for b, (std, seed) in enumerate(zip([0.01, 0.02, 0.03], [11, 2 ** 64 - 1, 13])):
        raw = bytes(g._inst(ex["sgld"], b).numpy().tobytes())
        s = N.DipSgldState.from_buffer_copy(raw)
        assert (s.offset, s.seed) == (0, seed) and s.std == np.float32(std), b
        assert g._inst(ex["sgld_ranges"], b).tolist() == ex["sgld_ranges"].tolist()
    # seeds default to `seeds`; the setter rewrites the float only
    d, _ = _dry_group(param_noise_std=0.05)
    assert d.param_noise_seeds == [5, 6, 7] and d.param_noise_std == [0.05] * 3
    d.set_param_noise_std([0.0, 0.5, 0.25])
    got = [N.DipSgldState.from_buffer_copy(bytes(d._inst(d._row0_extra["sgld"], b).numpy().tobytes())) for b in range(3)]
    assert [(s.offset, s.seed, s.std) for s in got] == [(0, 5, 0.0), (0, 6, 0.5), (0, 7, 0.25)]
    with pytest.raises(ValueError, match="dip-amd:.*without SGLD"):
        plain.set_param_noise_std(0.1)
