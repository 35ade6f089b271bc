"""CPU suite of the TV term of the fused super-resolution tail (total_loss = mse(out_LR, img_LR) + tv_weight * tv_loss(out_HR);
super-resolution.ipynb:180-181, sr_prior_effect.ipynb:109 of the reference): DipSRTVDesc and its three entry points beside the
pinned DipSRLossDesc ABI, what the library refuses before a launch, the constructor refusals of SRHead(tv_weight=) and
GroupedFits(tv_weights=), and the slab / launch names of a TV group built on host memory."""
import ctypes
import math
import os
import re

import pytest
import torch

from conftest import ROOT
from test_group_sr_host import LR, HW, _build, _down as _gdown, _problem, _small as _gsmall
from test_sr_head_host import _desc, _down, _small


def test_header_binding_and_command_list_know_the_entry_points(built):
    import dip_native as N
    hdr = open(os.path.join(ROOT, "include", "dip_hip.h")).read()
    assert re.search(r"^int dip_sr_tv_nblk\(int C, int H, int W\);", hdr, flags=re.M)
    assert re.search(r"^int dip_sr_tv_loss_fwd\(const DipSRTVDesc\* d, void\* stream\);", hdr, flags=re.M)
    assert re.search(r"^int dip_sr_tv_loss_bwd\(const DipSRTVDesc\* d, const float\* gscale, float\* dy, int Cy, void\* stream\);",
                     hdr, flags=re.M)
    assert re.search(r"typedef struct DipSRTVDesc \{.*?\} DipSRTVDesc;", hdr, flags=re.S)
    for name in ("dip_sr_tv_nblk", "dip_sr_tv_loss_fwd", "dip_sr_tv_loss_bwd"):
        assert name in N.EXPORTS and hasattr(built, name)
    for name, nargs in (("dip_sr_tv_loss_fwd", 2), ("dip_sr_tv_loss_bwd", 5)):
        fid = built.dip_list_fn_id(name.encode())
        assert fid >= 0, name
        assert built.dip_list_fn_nargs(fid) == nargs == len(N._SIGS[name][1]), name
    assert built.dip_list_fn_id(b"dip_sr_tv_nblk") == -1
    # what is pinned stays: new symbols and a new struct only
    assert built.dip_abi_version() == N.ABI_VERSION == 9
    assert ctypes.sizeof(N.DipSRLossDesc) == 96
    for name in ("dip_sr_loss_fwd", "dip_sr_loss_bwd"):
        assert built.dip_list_fn_id(name.encode()) >= 0


def test_descriptor_layout_follows_the_header():
    import dip_native as N
    hdr = open(os.path.join(ROOT, "include", "dip_hip.h")).read()
    body = re.search(r"typedef struct DipSRTVDesc \{(.*?)\} DipSRTVDesc;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls == ["DipSRLossDesc sr", "const float* tv_weight", "float* tv_partials", "int tv_nblk", "float beta"]
    want = {"DipSRLossDesc": N.DipSRLossDesc, "int": ctypes.c_int32, "float": ctypes.c_float}
    fields = [(d.replace("*", " ").split()[-1], ctypes.c_void_p if "*" in d else want[d.split()[0]]) for d in decls]
    assert list(N.DipSRTVDesc._fields_) == fields
    size = int(re.search(r"sizeof\(DipSRTVDesc\) == (\d+)", hdr).group(1))
    assert ctypes.sizeof(N.DipSRTVDesc) == size == 120
    T = N.DipSRTVDesc
    assert (T.sr.offset, T.tv_weight.offset, T.tv_partials.offset, T.tv_nblk.offset, T.beta.offset) == (0, 96, 104, 112, 116)
    # the embedded descriptor is the pinned one; `loss` / `out` of the TV descriptor are its fields (NativeIteration rewrites
    # desc.loss every iteration)
    d = T(_desc(N, N.lib()), 0x8000, 0x9000, 1, 0.5)
    d.loss = 0x1230
    assert d.sr.loss == 0x1230 == d.loss and d.out == d.sr.out == 0x1000


def test_tv_nblk():
    import dip_native as N
    L = N.lib()
    assert L.dip_sr_tv_nblk(3, 512, 512) == 3 * 32 * 8
    assert L.dip_sr_tv_nblk(1, 1, 1) == 1 and L.dip_sr_tv_nblk(2, 17, 65) == 2 * 2 * 2 and L.dip_sr_tv_nblk(1, 16, 64) == 1
    assert L.dip_sr_tv_nblk(0, 4, 4) == 0 and L.dip_sr_tv_nblk(1, 0, 4) == 0 and L.dip_sr_tv_nblk(1, 4, 0) == 0


def _tv_desc(N, L, tv=None, **over):
    sr = _desc(N, L, **over)
    g = dict(tv_weight=0x8000, tv_partials=0x9000, tv_nblk=L.dip_sr_tv_nblk(sr.C, sr.H, sr.W), beta=0.5)
    g.update(tv or {})
    return N.DipSRTVDesc(sr, g["tv_weight"], g["tv_partials"], g["tv_nblk"], g["beta"])


def _refused(L, d):
    for call in (lambda: L.dip_sr_tv_loss_fwd(ctypes.byref(d), None),
                 lambda: L.dip_sr_tv_loss_bwd(ctypes.byref(d), None, 0x7000, 4, None)):
        assert call() == -1
        yield L.dip_last_error()


SR_REFUSALS = [dict(out=None), dict(taps=None), dict(target=None), dict(y=None), dict(partials=None), dict(loss=None),
               dict(C=0), dict(k=0), dict(f=0), dict(Ho=15), dict(Wo=13), dict(nblk=2),
               dict(H=2, W=2, k=16, pad=6, Ho=1, Wo=1)]
TV_REFUSALS = [dict(tv_weight=None), dict(tv_partials=None), dict(tv_nblk=0), dict(tv_nblk=7), dict(beta=0.0), dict(beta=-0.5),
               dict(beta=math.inf), dict(beta=math.nan)]
_ids = lambda o: ",".join(f"{k}={v}" for k, v in o.items())  # noqa: E731


@pytest.mark.parametrize("over", SR_REFUSALS, ids=_ids)
def test_library_refuses_what_the_plain_tail_refuses(built, over):
    """-1 with dip_last_error set, from both entry points, before anything reaches HIP (this machine may have no GPU)."""
    import dip_native as N
    for err in _refused(built, _tv_desc(N, built, **over)):
        assert err.startswith(b"sr_loss")


@pytest.mark.parametrize("tv", TV_REFUSALS, ids=_ids)
def test_library_refuses_a_bad_tv_part(built, tv):
    import dip_native as N
    for err in _refused(built, _tv_desc(N, built, tv=tv)):
        assert err.startswith(b"sr_tv_loss")


def test_library_refuses_null_descriptor_and_bad_channel_stride(built):
    import dip_native as N
    L = built
    assert L.dip_sr_tv_loss_fwd(None, None) == -1 and b"NULL descriptor" in L.dip_last_error()
    assert L.dip_sr_tv_loss_bwd(None, None, 0x7000, 4, None) == -1 and b"NULL descriptor" in L.dip_last_error()
    d = _tv_desc(N, L)
    for Cy in (2, 3, 5, 6):
        assert L.dip_sr_tv_loss_bwd(ctypes.byref(d), None, 0x7000, Cy, None) == -1
        assert b"Cy" in L.dip_last_error()
    assert L.dip_sr_tv_loss_bwd(ctypes.byref(d), None, None, 4, None) == -1


# ------------------------------------------------------------------------------------------ SRHead(tv_weight=, tv_beta=)
@pytest.mark.parametrize("kw", [dict(tv_weight=-1e-7), dict(tv_weight=math.inf), dict(tv_weight=math.nan),
                                dict(tv_weight=1e-6, tv_beta=0.0), dict(tv_weight=1e-6, tv_beta=-1.0),
                                dict(tv_weight=0.0, tv_beta=0.0), dict(tv_weight=1e-6, tv_beta=math.nan)], ids=_ids)
def test_srhead_refuses_a_bad_weight_or_beta_at_construction(kw):
    from utils.loss_head import SRHead
    net = _small()
    with pytest.raises(ValueError, match="dip-amd:.*SRHead: tv_(weight|beta) must be finite"):
        SRHead(net, torch.rand(1, 3, 8, 8), _down(), **kw)
    assert net.__dict__["_dip_engine"].device is None


def test_srhead_without_tv_is_the_object_it_was():
    """tv_weight == 0 (the default): the descriptor, the launches and the plan key of the plain tail."""
    import inspect
    from utils.loss_head import SRHead
    sig = inspect.signature(SRHead.__init__)
    assert list(sig.parameters)[1:] == ["net", "img_LR", "downsampler", "tv_weight", "tv_beta"]
    assert sig.parameters["tv_weight"].default == 0.0 and sig.parameters["tv_beta"].default == 0.5
    h = SRHead.__new__(SRHead)                      # (the constructor needs device tensors: the launch choice alone)
    h._tv = False
    import dip_native as N
    from types import SimpleNamespace
    lib = SimpleNamespace(dip_head_fwd="hf", dip_sr_loss_fwd="f", dip_sr_loss_bwd="b", dip_sr_tv_loss_fwd="tf",
                          dip_sr_tv_loss_bwd="tb")
    eng = SimpleNamespace(lib=lib, n_out=3, Hout=8, Wout=8, need_sigmoid=True, y_out=torch.zeros(1), dy_out=torch.zeros(1))
    sr = _desc(N, N.lib())
    assert [n for _, _, n in h.fwd_launches(eng, sr) + h.bwd_launches(eng, sr, 0)] == ["head_fwd", "sr_loss_fwd", "sr_loss_bwd"]
    h._tv = True
    tv = N.DipSRTVDesc(sr, 0x8000, 0x9000, 1, 0.5)
    ops = h.fwd_launches(eng, tv) + h.bwd_launches(eng, tv, 0)
    assert [n for _, _, n in ops] == ["head_fwd", "sr_tv_loss_fwd", "sr_tv_loss_bwd"]
    assert [fn for fn, _, _ in ops] == ["hf", "tf", "tb"] and ops[0][1][1] == sr.out


def test_set_tv_weight_does_not_cross_zero():
    from utils.loss_head import SRHead
    h = SRHead.__new__(SRHead)
    h.tv_weight, h.tv_beta, h._tv, h._tvw = 1e-6, 0.5, True, None
    key = (h.tv_beta, id(h._tvw))
    h.set_tv_weight(3e-6)
    assert h.tv_weight == 3e-6 and key == (h.tv_beta, id(h._tvw))
    with pytest.raises(ValueError, match="dip-amd:.*set_tv_weight.*new SRHead"):
        h.set_tv_weight(0.0)
    for bad in (-1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="tv_weight must be finite"):
            h.set_tv_weight(bad)
    assert h.tv_weight == 3e-6
    h.tv_weight, h._tv = 0.0, False
    with pytest.raises(ValueError, match="dip-amd:.*set_tv_weight.*new SRHead"):
        h.set_tv_weight(1e-6)
    h.set_tv_weight(0.0)


# ------------------------------------------------------------------------------------------ GroupedFits(tv_weights=)
def _group_args(B=3):
    zs, ts = _problem(B)
    return [_gsmall(b) for b in range(B)], zs, ts, [_gdown() for _ in range(B)]


def test_group_refusals_before_anything_is_planned():
    from dip_group import GroupedFits
    nets, zs, ts, downs = _group_args()
    kw = dict(device="cpu", _dry_cpu=True)
    with pytest.raises(ValueError, match="dip-amd:.*mixes zero and positive"):
        GroupedFits(nets, zs, ts, downsamplers=downs, tv_weights=[1e-6, 0.0, 1e-5], **kw)
    with pytest.raises(ValueError, match="dip-amd:.*tv_weights=.*needs downsamplers="):
        GroupedFits(nets, zs, [torch.rand(1, 3, *HW) for _ in nets], tv_weights=1e-6, **kw)
    with pytest.raises(ValueError, match="one per instance: got 2 for 3"):
        GroupedFits(nets, zs, ts, downsamplers=downs, tv_weights=[1e-6, 1e-5], **kw)
    with pytest.raises(ValueError, match="dip-amd:.*GroupedFits: tv_weight must be finite"):
        GroupedFits(nets, zs, ts, downsamplers=downs, tv_weights=[1e-6, -1e-6, 1e-5], **kw)
    with pytest.raises(ValueError, match="dip-amd:.*GroupedFits: tv_weight must be finite"):
        GroupedFits(nets, zs, ts, downsamplers=downs, tv_weights=math.nan, **kw)
    with pytest.raises(ValueError, match="dip-amd:.*GroupedFits: tv_beta must be finite"):
        GroupedFits(nets, zs, ts, downsamplers=downs, tv_weights=1e-6, tv_beta=0.0, **kw)
    for n in nets:
        assert n.__dict__["_dip_engine"].device is None


def test_a_tv_group_plans_the_tv_launches_and_owns_two_more_rows(built):
    B = 3
    ws = [1e-7, 1e-6, 1e-5]
    g, nets, zs, ts, downs = _build(B, tv_weights=ws, tv_beta=0.75)
    assert [n for _, _, n in g._head_fwd + g._head_bwd] == ["head_fwd", "sr_tv_loss_fwd", "sr_tv_loss_bwd"]
    assert g.pointers_outside_row0() == []
    ex = g._row0_extra
    order = ["saved", "noisy", "rng", "taps", "target", "out", "y", "partials", "tv_weight", "tv_partials", "loss", "gl", "m",
             "v", "iter"]
    offs = [g._off(ex[k]) for k in order]
    assert offs == sorted(offs) and [k for k in ex if ex[k] is not None] == order
    assert ex["tv_weight"].numel() == 1
    assert ex["tv_partials"].numel() == g.lib.dip_sr_tv_nblk(3, *HW) == g._head.tv_nblk
    for b in range(B):
        assert g._inst(ex["tv_weight"], b).item() == torch.tensor(ws[b], dtype=torch.float32).item()
        lo = g.mem.data_ptr() + b * g.stride
        for k in ("tv_weight", "tv_partials"):
            t = g._inst(ex[k], b)
            assert lo <= t.data_ptr() and t.data_ptr() + 4 * t.numel() <= lo + g.stride, (b, k)
    d = g._head
    assert (d.tv_weight, d.tv_partials, d.beta) == (ex["tv_weight"].data_ptr(), ex["tv_partials"].data_ptr(), 0.75)
    s = d.sr
    assert (s.out, s.taps, s.target, s.y, s.partials, s.loss) == tuple(ex[k].data_ptr() for k in
                                                                      ("out", "taps", "target", "y", "partials", "loss"))
    assert (s.C, s.H, s.W, s.k, s.f, s.pad, s.Ho, s.Wo, s.sigmoid) == (3, 64, 96, 16, 4, 6, 16, 24, 1)
    assert s.nblk == g.lib.dip_sr_loss_nblk(3, *LR)
    # one float for all instances
    g1, *_ = _build(2, tv_weights=2e-6)
    assert g1.tv_weights == [2e-6, 2e-6] and g1.tv_beta == 0.5
    assert [g1._inst(g1._row0_extra["tv_weight"], b).item() for b in range(2)] == [torch.tensor(2e-6).item()] * 2
    # other positive weights: the scalars alone
    g1.set_tv_weights([1e-6, 3e-6])
    assert [g1._inst(g1._row0_extra["tv_weight"], b).item() for b in range(2)] == [torch.tensor(w).item() for w in (1e-6, 3e-6)]
    with pytest.raises(ValueError, match="mixes zero and positive"):
        g1.set_tv_weights([0.0, 3e-6])
    with pytest.raises(ValueError, match="construct a new group"):
        g1.set_tv_weights(0.0)


@pytest.mark.parametrize("tvw", [None, 0.0, [0.0, 0.0, 0.0]], ids=["none", "zero", "zeros"])
def test_a_group_without_tv_plans_exactly_what_it_planned(built, tvw):
    g0, *_ = _build(3)
    g, *_ = _build(3, tv_weights=tvw)
    assert g.tv_weights is None
    assert [n for _, _, n in g._head_fwd + g._head_bwd] == ["head_fwd", "sr_loss_fwd", "sr_loss_bwd"]
    import dip_native as N
    assert isinstance(g._head, N.DipSRLossDesc)
    order = ["saved", "noisy", "rng", "taps", "target", "out", "y", "partials", "loss", "gl", "m", "v", "iter"]
    assert [k for k in g._row0_extra if g._row0_extra[k] is not None] == order
    assert g.stride == g0.stride and [g._off(g._row0_extra[k]) for k in order] == [g0._off(g0._row0_extra[k]) for k in order]
    with pytest.raises(ValueError, match="without a TV term"):
        g.set_tv_weights(1e-6)
