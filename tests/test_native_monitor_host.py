"""CPU suite of NativeIteration(monitor=): the device-indexed monitor entry point (dip_fit_monitor_dev, DipFitMonitorDesc) is
declared, exported, a command-list function and validates on the host before it launches; the new keyword's type check is
reached on CPU tensors and monitor=None raises what it raised before."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT


def _small():
    from models.skip import skip
    return skip(8, 3, num_channels_down=[16, 16], num_channels_up=[16, 16], num_channels_skip=[4, 4], upsample_mode="bilinear",
                need_sigmoid=True, need_bias=True, pad="reflection")


def test_header_declares_the_entry_point_and_the_descriptor(built):
    import dip_native as N
    hdr = open(os.path.join(ROOT, "include", "dip_hip.h")).read()
    assert re.search(r"^int dip_fit_monitor_dev\(const DipFitMonitorDesc\* d, void\* stream\);", hdr, flags=re.M)
    assert re.search(r"^typedef struct DipFitMonitorDesc \{", hdr, flags=re.M)
    # the comment in front of the struct names the reference lines the entry replaces, and states the struct's size
    head = hdr[:hdr.index("typedef struct DipFitMonitorDesc")]
    comment = head[head.rindex("/*"):]
    assert "denoising.ipynb:214-248" in comment
    size = int(re.search(r"sizeof\(DipFitMonitorDesc\) == (\d+)", comment).group(1))
    assert ctypes.sizeof(N.DipFitMonitorDesc) == size == 104
    # every field of the header's struct, in order, is a field of the binding's
    body = hdr[hdr.index("typedef struct DipFitMonitorDesc {"):hdr.index("} DipFitMonitorDesc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            names += [re.split(r"[\s\*]+", first.strip())[-1]] + [r.strip().lstrip("*") for r in rest]
    assert names == [f[0] for f in N.DipFitMonitorDesc._fields_]
    assert "dip_fit_monitor_dev" in N.EXPORTS and hasattr(built, "dip_fit_monitor_dev")
    assert built.dip_abi_version() == N.ABI_VERSION == 9          # new entry point, new struct, no existing struct changed
    # the existing entry is still declared as it was
    assert "int dip_fit_monitor(const float* out, const float* noisy, const float* gt, float* out_avg, int64_t n," in hdr


def test_command_list_knows_the_monitor_launches(built):
    import dip_native as N
    for name, nargs in (("dip_fit_monitor_dev", 2), ("dip_arena_backtrack", 5)):
        fid = built.dip_list_fn_id(name.encode())
        assert fid >= 0, name
        assert built.dip_list_fn_nargs(fid) == nargs == len(N._SIGS[name][1]), name


def _desc(N, **kw):
    """A descriptor whose pointers are non-NULL but never dereferenced: validation refuses before any launch."""
    fake = 1 << 20
    d = N.DipFitMonitorDesc(fake, fake, None, fake, 64, 0.99, 5.0, None, fake, fake, 4, 3, 1, 0, fake, fake)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_validates_on_the_host_before_any_launch(built):
    import dip_native as N
    L = built
    assert L.dip_fit_monitor_dev(None, None) == -1
    assert b"fit_monitor_dev" in L.dip_last_error()
    for bad in (dict(n=0), dict(n=-5), dict(capacity=0), dict(show_every=0), dict(show_every=-1), dict(out=None), dict(noisy=None),
                dict(out_avg=None), dict(partial=None), dict(records=None), dict(counter=None), dict(state=None)):
        d = _desc(N, **bad)
        assert L.dip_fit_monitor_dev(ctypes.byref(d), None) == -1, bad
        assert b"fit_monitor_dev" in L.dip_last_error(), bad
    # ... and through a command list: the failing command is named, nothing after it is issued
    d = _desc(N, capacity=0)
    cl = N.CmdList([("launch", L.dip_fit_monitor_dev, (ctypes.byref(d),), 0, "fit_monitor_dev"),
                    ("launch", L.dip_arena_backtrack, (1 << 20, 1 << 21, 16, 1 << 22), 0, "arena_backtrack")])
    with pytest.raises(RuntimeError, match="fit_monitor_dev"):
        cl.run([None])
    assert cl._failed.value == 0


def test_monitor_keyword_type_check_is_reached_on_the_cpu():
    from dip_optim import FusedAdam, NativeIteration
    from utils.common_utils import get_params
    z = torch.rand(1, 8, 32, 32) * 0.1
    net = _small()
    opt = FusedAdam(get_params('net', net, z), lr=0.01)
    with pytest.raises(TypeError, match="dip-amd:.*FitMonitor"):
        NativeIteration(net, None, opt, z, monitor=object())
    with pytest.raises(TypeError, match="dip-amd:.*FitMonitor"):
        NativeIteration(net, None, opt, z, monitor=lambda out, loss: None)
    # monitor=None: today's error, and the checks in front of the new one keep their precedence
    with pytest.raises(RuntimeError, match="dip-amd:.*CPU"):
        NativeIteration(net, None, opt, z, monitor=None)
    with pytest.raises(RuntimeError, match="dip-amd:.*CPU"):
        NativeIteration(net, None, opt, z)
    with pytest.raises(TypeError, match="dip-amd:.*FusedAdam"):
        NativeIteration(net, None, torch.optim.Adam(net.parameters(), lr=0.01), z, monitor=object())
    assert opt.step_count == 0 and opt._groups is None
    assert net.__dict__["_dip_engine"].device is None


def test_docstrings_describe_the_monitor():
    import dip_optim
    from utils import fit_monitor
    doc = dip_optim.NativeIteration.__doc__
    for word in ("monitor=", "FitMonitor", "dip_fit_monitor_dev", "capacity"):
        assert word in doc, word
    assert "NativeIteration" in fit_monitor.__doc__ and "dip_fit_monitor_dev" in fit_monitor.__doc__
