"""The launch lists of dip_engine's planner as a fingerprint: the allocations in order, every op of the forward / backward /
input-gradient lists (entry point, op name, its arguments with every descriptor expanded field by field and every pointer
written as [allocation role, byte offset]) and the stream schedule's inputs (_fwd_side, _bulk2, _backward_deps).
The recorded file is kept small: the sizes of the shared scratch pool stand in it as they are; every op is ONE 8-hex-digit
digest over (entry point, op name, arguments), a list the concatenation of its ops' digests; the whole ordered
(role, byte size) list and the schedule's inputs are one digest each.  On a mismatch the message carries what was planned.
The expected values (tests/golden/engine_launch_lists.json) were recorded by running this file as a script at the commit
BEFORE the planner's scratch pool / descriptor builders were introduced; the planner may be rewritten freely as long as
what it emits stays the same, bit for bit.  Host memory only: _build_arenas(cpu) + _build_plan run the whole emitting pass,
nothing is launched."""
import bisect
import ctypes as C
import functools
import hashlib
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_launch_lists.json")
LISTS = ("fwd_ops", "bwd_ops", "bwd_input_ops")
DIGITS = 8          # hex digits of an op's digest
DEFAULT_KW = dict(skip_n33d=128, skip_n33u=128, skip_n11=4, num_scales=5)
# engine switches, set as attributes between construction and _build_plan (the library reads some of the environment
# variables of the same names once per process, so the environment is not used)
SWITCHES = {
    "ticket": dict(ticket_fin=True, bnb_one=False),
    "fusebnb": dict(fuse_bnb=True),
    "fuse1x1": dict(fuse_bnb_1x1=True, thin_src=False),
    "noone": dict(bnb_one=False),
    "onestream": dict(two_streams=False, defer_scale=-1, tail_inline=False, bulk2_max_pixels=0),
}
BASE = ([("default", (256, 256)), ("default", (100, 76)), ("default_zero", (128, 128))]
        + [(n, (64, 48)) for n in ("tiny_default", "tiny_library", "tiny_snail", "tiny_avg", "tiny_max", "tiny_skip3",
                                   "tiny_lanczos2", "tiny_feat7", "tiny_zero")]
        + [("tiny_poolcrop", (37, 45)), ("tiny_noskipcrop", (37, 45)), ("resnet_res", (32, 40)), ("resnet_plain", (32, 40))])
SWITCHED = [("default", (256, 256)), ("tiny_default", (64, 48)), ("tiny_poolcrop", (37, 45)), ("resnet_res", (32, 40))]
CASES = {f"{n}@{h}x{w}": (n, (h, w), None) for n, (h, w) in BASE}
CASES.update({f"{n}@{h}x{w}+{s}": (n, (h, w), s) for s in SWITCHES for n, (h, w) in SWITCHED})
# every entry point the planner can put on a launch list
ENTRY_POINTS = frozenset("""dip_bn_finalize dip_conv_small dip_conv_igemm dip_avgpool2_fwd dip_maxpool2_fwd dip_upcat_fwd
    dip_upcat_fwd_fin dip_conv_wgrad dip_wgrad_reduce dip_conv_thin4 dip_conv_igemm_dma_cols dip_conv_dgrad_ring dip_bn_bwd_one
    dip_bn_bwd_stats dip_bn_bwd_stats_fin dip_bn_bwd_finalize dip_bn_bwd_finalize2 dip_bn_bwd_apply_src
    dip_upsample_bwd_one dip_upsample_bwd_stats dip_upsample_bwd_stats_crop
    dip_upsample_bwd_stats_crop_fin dip_bn_bwd_apply dip_fold_to_nhwc dip_avgpool2_bwd dip_maxpool2_bwd
    dip_res_join_fwd dip_res_join_bwd""".split())


def _net(name):
    if name.startswith("default"):
        from models import get_net
        if name == "default":
            return get_net(32, 'skip', 'reflection', upsample_mode='bilinear', **DEFAULT_KW)
        return get_net(32, 'skip', 'zero', upsample_mode='nearest', **DEFAULT_KW)
    if name.startswith("resnet"):
        from models.resnet import ResNet
        if name == "resnet_res":
            return ResNet(8, 3, 2, 16, need_residual=True, pad='reflection')
        return ResNet(8, 3, 2, 16, need_residual=False, pad='zero')
    from models.skip import skip
    from test_net_gpu import NETS
    return skip(*NETS[name]["args"], **NETS[name]["kw"])


def _planned(case):
    name, (H, W), switch = CASES[case]
    torch.manual_seed(0)
    eng = _net(name).__dict__["_dip_engine"]
    for k, v in (SWITCHES[switch] if switch else {}).items():
        assert hasattr(eng, k), k
        setattr(eng, k, v)
    eng._build_arenas(torch.device("cpu"))
    eng._build_plan(H, W, eng._net_cin())
    return eng


def _fingerprint(eng, expand=None):
    """expand = (list name, op index): the expanded arguments of that op instead of the fingerprint."""
    roles = [(r, getattr(eng, r)) for r in ("params", "grads", "bnbuf", "packed", "packed3") if getattr(eng, r, None) is not None]
    for k, bn in enumerate(eng.bns):
        roles += [(f"bn{k}.state", bn.state), (f"bn{k}.coef", bn.coef)]
    roles += [(f"alloc{k}", t) for k, t in enumerate(eng._alloc)]
    spans = sorted((t.data_ptr(), t.numel() * t.element_size(), r) for r, t in roles)
    starts = [s[0] for s in spans]

    def pointer(v):
        if not v:
            return None
        k = bisect.bisect_right(starts, v) - 1
        assert k >= 0 and v < spans[k][0] + spans[k][1], f"pointer {v:#x} resolves to no allocation"
        return [spans[k][2], v - spans[k][0]]

    def struct(s):
        out = {}
        for f, ty in s._fields_:
            v = getattr(s, f)
            out[f] = struct(v) if isinstance(v, C.Structure) else pointer(v) if ty is C.c_void_p else v
        return out

    def arguments(fn, args):
        assert len(args) == len(fn.argtypes) - 1, fn.__name__          # (the trailing stream is added at launch)
        return [[type(a._obj).__name__, struct(a._obj)] if hasattr(a, "_obj") else pointer(a) if ty is C.c_void_p
                or a is None else a for a, ty in zip(args, fn.argtypes)]

    if expand is not None:
        fn, args, _ = getattr(eng, expand[0])[expand[1]]
        return arguments(fn, args)

    def digest(what, n):
        return hashlib.sha256(json.dumps(what).encode()).hexdigest()[:n]

    alloc = [[r, t.numel() * t.element_size()] for r, t in roles]
    sched = [sorted(eng._fwd_side), sorted(eng._bulk2), eng._backward_deps(eng.bwd_ops)]
    ops = {l: [(fn.__name__, name, digest([fn.__name__, name, arguments(fn, args)], DIGITS)) for fn, args, name in getattr(eng, l)]
           for l in LISTS}
    # (the shared scratch pool is what the emitting pass allocates first: 11 float32 buffers, then the int32 tickets)
    compact = {"pool": [t.numel() * t.element_size() for t in eng._alloc[:12]], "alloc": [len(alloc), digest(alloc, 16)],
               "ops": {l: "".join(d for _, _, d in ops[l]) for l in LISTS}, "sched": digest(sched, 16)}
    return compact, {"alloc": alloc, "sched": sched, "ops": ops}


@functools.lru_cache(maxsize=None)
def _recorded(case):
    """(compact fingerprint, the recorded one, entry points reached, what differs first or None): one plan per case and session."""
    with open(GOLDEN) as fh:
        want = json.load(fh)[case]
    eng = _planned(case)
    got, detail = _fingerprint(eng)
    got = json.loads(json.dumps(got))
    reached = {fn for ops in detail["ops"].values() for fn, _, _ in ops}
    first = None
    for l in LISTS:
        w = want["ops"][l]
        for k, (fn, name, d) in enumerate(detail["ops"][l]):
            if d != w[DIGITS * k:DIGITS * (k + 1)]:
                first = (f"{case}: {l}[{k}] = {fn} {name!r} has digest {d}, recorded {w[DIGITS * k:DIGITS * (k + 1)]!r}; "
                         f"its arguments: {_fingerprint(eng, (l, k))}")
                break
        if first is None and len(w) != DIGITS * len(detail["ops"][l]):
            first = f"{case}: {l} has {len(detail['ops'][l])} ops, recorded {len(w) // DIGITS}"
        if first is not None:
            return got, want, reached, first
    for k in ("pool", "alloc", "sched"):
        if got[k] != want[k]:
            return got, want, reached, f"{case}: {k} is {got[k]}, recorded {want[k]}; planned: {detail['sched' if k == 'sched' else 'alloc']}"
    return got, want, reached, None


@pytest.mark.parametrize("case", list(CASES))
def test_launch_lists_are_the_recorded_ones(built, case):
    got, want, _, first = _recorded(case)
    assert first is None, first
    assert got == want


def test_the_cases_reach_every_entry_point_of_the_planner(built):
    reached = set().union(*(_recorded(case)[2] for case in CASES))
    assert reached == ENTRY_POINTS, reached ^ ENTRY_POINTS


if __name__ == "__main__":
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    import __graft_entry__ as ge
    ge.build()
    with open(GOLDEN, "w") as fh:
        fh.write("{\n" + ",\n".join(json.dumps(case) + ": " + json.dumps(_fingerprint(_planned(case))[0], separators=(",", ":"))
                                    for case in CASES) + "\n}\n")
