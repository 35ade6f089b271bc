"""adam_sgld_kernel on a real MI355X (csrc/misc_kernels.hip, through dip_adam_sgld_step and dip_adam_sgld_step_dev): the fused
launch against the two pinned kernels it fuses -- dip_adam_step (tests/test_kernels_gpu.py holds it to torch.optim.Adam) and
dip_noise_axpy (tests/test_noise_gpu.py holds its stream to tests/noise_ref.py) -- composed per the specification, bitwise;
weight decay against torch.optim.Adam(weight_decay=) on the CPU; one grouped launch over rows with different streams; what
is refused."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dip_native as N  # noqa: E402
import hipops as H  # noqa: E402
import sgld_ref as S  # noqa: E402
from test_noise_gpu import native_mask  # noqa: E402,F401

SIZES = [1, 3, 4, 5, 1023, 1024, 1027, 3075]      # tests/test_noise_gpu.py's: one element, every n % 4, one block, three blocks
STREAMS = [(2 ** 32 + 7, 2 ** 32 - 100), (2 ** 64 - 1, 0)]        # (seed, offset): the 32-bit boundary falls inside a launch
LR, B1, B2, EPS = 0.01, 0.9, 0.999, 1e-8
GUARD = 8


def _tables(n):
    """The range tables of a size: none; all of [0, n); boundaries off the quad grid, clipped to n; two adjacent ranges; a
    range that ends at n.  Sorted, disjoint, non-empty ranges."""
    clip = lambda rs: [(b, min(e, n)) for b, e in rs if b < min(e, n)]
    half = max(1, n // 2)
    return {"none": [],
            "all": [(0, n)],
            "off-grid": clip([(1, 2), (3, 9), (max(n - 5, 9), n)]),
            "adjacent": clip([(1, half), (half, n - 1)]) if n >= 4 else clip([(0, half), (half, n)]),
            "ends-at-n": [(n - min(n, 3), n)]}


def _table_dev(ranges, dev):
    t = torch.tensor([x for r in ranges for x in r] or [0], dtype=torch.int64, device=dev)
    return t, (t.data_ptr() if ranges else None)


class _Buf:
    """A float buffer of n elements `shift` floats past a 16-byte boundary, sentinels on both sides."""

    def __init__(self, src, dev, shift=0):
        self.n, self.lo = src.numel(), 4 + shift
        self.raw = torch.full((self.lo + self.n + GUARD,), H.SENTINEL, dtype=torch.float32, device=dev)
        assert self.raw.data_ptr() % 16 == 0
        self.raw[self.lo:self.lo + self.n] = src.to(dev)

    ptr = property(lambda self: self.raw.data_ptr() + 4 * self.lo)
    val = property(lambda self: self.raw[self.lo:self.lo + self.n])

    def guards_ok(self):
        return bool((self.raw[:self.lo] == H.SENTINEL).all()) and bool((self.raw[self.lo + self.n:] == H.SENTINEL).all())


def _inputs(n, steps, seed=5):
    g = torch.Generator().manual_seed(seed + n)
    p, m = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1
    v = torch.rand(n, generator=g) * 0.01                          # v >= 0
    grads = [torch.randn(n, generator=g) * (10.0 ** torch.randint(-4, 1, (n,), generator=g).float()) for _ in range(steps)]
    return p, m, v, grads


def _iter_state(dev, step=0):
    st = torch.zeros(16, dtype=torch.uint8, device=dev)
    st.view(torch.int64)[0] = step
    return st


def _sgld_state(dev, offset, seed, std):
    """[guard, DipSgldState (3 words), guard] as int64."""
    raw = bytes(N.DipSgldState(H.as_u64(offset), H.as_u64(seed), std, 0.0))
    words = np.frombuffer(raw, dtype=np.int64).tolist()
    return torch.tensor([-7] + words + [-7], dtype=torch.int64, device=dev)


def _read_state(t):
    w = t.cpu().numpy()
    assert w[0] == -7 and w[-1] == -7, "wrote around the DipSgldState"
    s = N.DipSgldState.from_buffer_copy(w[1:4].tobytes())
    return s.offset, s.seed, s.std


def _composed(dev, n, p, m, v, grads, ranges, std, seed, offset, wd=0.0):
    """The specification from the two pinned kernels: dip_adam_step on a copy, then dip_noise_axpy(z = that result, sigma =
    std, seed ^ KEY, offset + t * ceil(n / 4)) inside the ranges.  Returns the (p, m, v) after every step."""
    assert wd == 0.0
    L = N.lib()
    pb, mb, vb = _Buf(p, dev), _Buf(m, dev), _Buf(v, dev)
    inside = torch.from_numpy(S.inside(n, ranges)).to(dev)
    out = []
    for t, g in enumerate(grads):
        gd = g.to(dev)
        N.check(L.dip_adam_step(pb.ptr, gd.data_ptr(), mb.ptr, vb.ptr, n, LR, B1, B2, EPS, t + 1, H.stream(dev)), "adam_step")
        torch.cuda.synchronize()
        noisy, _ = H.noise_axpy(pb.val.clone(), std, S.stream_seed(seed), offset + t * ((n + 3) // 4), "host")
        pb.val.copy_(torch.where(inside, noisy, pb.val))
        out.append((pb.val.clone(), mb.val.clone(), vb.val.clone()))
    return out


def _fused(dev, n, p, m, v, grads, ranges, std, seed, offset, wd=0.0, entry="host", shift=0):
    """The fused launch, `entry` = "host" (dip_adam_sgld_step: scalars by value) or "dev" (dip_adam_sgld_step_dev: DipIterState
    + DipSgldState in device memory).  Returns the (p, m, v) after every step and, for "dev", the DipSgldState afterwards."""
    L = N.lib()
    pb, mb, vb = _Buf(p, dev, shift), _Buf(m, dev), _Buf(v, dev)
    table, tptr = _table_dev(ranges, dev)
    st, ns = _iter_state(dev), _sgld_state(dev, offset, seed, std)
    out = []
    for t, g in enumerate(grads):
        gb = _Buf(g, dev)
        gkeep = gb.raw.clone()
        if entry == "host":
            rc = L.dip_adam_sgld_step(pb.ptr, gb.ptr, mb.ptr, vb.ptr, n, LR, B1, B2, EPS, wd, t + 1, std, H.as_u64(seed),
                                      H.as_u64(offset + t * ((n + 3) // 4)), tptr, len(ranges), H.stream(dev))
        else:
            N.check(L.dip_adam_tick(st.data_ptr(), LR, B1, B2, H.stream(dev)), "adam_tick")
            rc = L.dip_adam_sgld_step_dev(pb.ptr, gb.ptr, mb.ptr, vb.ptr, n, B1, B2, EPS, wd, st.data_ptr(), ns.data_ptr() + 8,
                                          tptr, len(ranges), H.stream(dev))
        N.check(rc, "adam_sgld_step" + ("" if entry == "host" else "_dev"))
        torch.cuda.synchronize()
        assert pb.guards_ok() and mb.guards_ok() and vb.guards_ok(), f"adam_sgld_step({entry}): wrote outside p, m or v"
        assert torch.equal(gb.raw, gkeep), "the gradient was written"
        out.append((pb.val.clone(), mb.val.clone(), vb.val.clone()))
    return out, (_read_state(ns) if entry == "dev" else None)


def _assert_steps_equal(got, want, what):
    for t, (a, b) in enumerate(zip(got, want)):
        for name, x, y in zip("pmv", a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (what, "step", t, name,
                                                                           int((x.view(torch.int32) != y.view(torch.int32)).sum()))


# ------------------------------------------------------------------------------------------ fused == composed, bitwise
@pytest.mark.parametrize("n", SIZES)
def test_fused_equals_the_two_pinned_kernels_composed(dev, n):
    """3 steps, every table, both streams, both entry points: p inside the ranges is dip_noise_axpy of dip_adam_step's
    result, outside it is dip_adam_step's; m and v are dip_adam_step's; the DipSgldState's offset ends 3 * ceil(n / 4) further
    and seed and std are what they were."""
    std = 1.0 / 30.0
    p, m, v, grads = _inputs(n, 3)
    quads = (n + 3) // 4
    for name, ranges in _tables(n).items():
        for seed, offset in STREAMS:
            want = _composed(dev, n, p, m, v, grads, ranges, std, seed, offset)
            host, _ = _fused(dev, n, p, m, v, grads, ranges, std, seed, offset, entry="host")
            _assert_steps_equal(host, want, (name, seed, "host"))
            devd, state = _fused(dev, n, p, m, v, grads, ranges, std, seed, offset, entry="dev")
            _assert_steps_equal(devd, want, (name, seed, "dev"))
            assert state == (offset + 3 * quads, seed, np.float32(std)), (name, state)
            if ranges:                              # the noise is there: p differs from plain Adam exactly inside the ranges
                plain = _composed(dev, n, p, m, v, grads[:1], [], std, seed, offset)[0][0]
                changed = (host[0][0] != plain).cpu().numpy()
                assert not changed[~S.inside(n, ranges)].any() and changed[S.inside(n, ranges)].mean() > 0.5, name


@pytest.mark.parametrize("n", [5, 1024, 1027])
def test_scalar_path_equals_vector_path(dev, n):
    """p one float past a 16-byte boundary: the element-by-element path gives the aligned call's values."""
    std, (seed, offset) = 0.05, STREAMS[0]
    p, m, v, grads = _inputs(n, 2)
    ranges = _tables(n)["off-grid"]
    want, _ = _fused(dev, n, p, m, v, grads, ranges, std, seed, offset, entry="host")
    for entry in ("host", "dev"):
        got, _ = _fused(dev, n, p, m, v, grads, ranges, std, seed, offset, entry=entry, shift=1)
        _assert_steps_equal(got, want, entry)


def test_float64_restatement_agrees(dev):
    """One step against tests/sgld_ref.perturb on dip_adam_step's result: the fma's one rounding (half an ulp of p) plus the
    std-fold of the normals' tolerance of tests/test_noise_gpu.py."""
    import noise_ref as R
    from test_noise_gpu import _tolerance
    n, std, (seed, offset) = 1027, 0.05, STREAMS[0]
    p, m, v, grads = _inputs(n, 1)
    ranges = _tables(n)["off-grid"]
    p1 = _composed(dev, n, p, m, v, grads, [], std, seed, offset)[0][0].cpu().numpy()
    got = _fused(dev, n, p, m, v, grads, ranges, std, seed, offset)[0][0][0].cpu().double().numpy()
    want = S.perturb(p1, ranges, std, seed, offset)
    ks = S.stream_seed(seed)
    _, _, tol = _tolerance(R.normals(n, ks, offset), R.normals32(n, ks, offset))
    err = np.abs(got - want)
    bound = std * tol + 0.5 * np.spacing(np.abs(got).astype(np.float32)).astype(np.float64)
    print(f"sgld vs float64 restatement: worst err / bound {float((err / bound).max()):.3f}")
    assert np.all(err <= bound)
    assert np.array_equal(got[~S.inside(n, ranges)], p1.astype(np.float64)[~S.inside(n, ranges)])


# ------------------------------------------------------------------------------------------ pure noise
@pytest.mark.parametrize("n", [5, 1027])
def test_pure_noise_is_noise_axpy(dev, n):
    """g = m = v = 0 and no weight decay: Adam leaves p alone, the output is dip_noise_axpy of p under the SGLD key, bitwise."""
    std, (seed, offset) = 1.0 / 30.0, STREAMS[1]
    p = _inputs(n, 0)[0]
    zero = torch.zeros(n)
    got, _ = _fused(dev, n, p, zero, zero, [zero], [(0, n)], std, seed, offset)
    want, _ = H.noise_axpy(p.to(dev), std, S.stream_seed(seed), offset, "host")
    assert torch.equal(got[0][0].view(torch.int32), want.view(torch.int32))
    assert not torch.equal(want, H.noise_axpy(p.to(dev), std, seed, offset, "host")[0])     # the key XOR is there
    assert not got[0][1].any() and not got[0][2].any()


# ------------------------------------------------------------------------------------------ weight decay
def test_zero_weight_decay_is_adam_step_bitwise(dev):
    n = 100003
    p, m, v, grads = _inputs(n, 2)
    grads = [torch.where(torch.arange(n) % 7 == 0, torch.tensor(-0.0), g) for g in grads]        # -0.0 gradients stay -0.0
    want = _composed(dev, n, p, m, v, grads, [], 0.0, 0, 0)
    for entry in ("host", "dev"):
        got, _ = _fused(dev, n, p, m, v, grads, [], 0.0, 0, 0, wd=0.0, entry=entry)
        _assert_steps_equal(got, want, entry)


@pytest.mark.parametrize("wd", [5e-8, 1e-2])
def test_weight_decay_matches_torch(dev, wd):
    """The new entry point, no noise, against torch.optim.Adam(weight_decay=wd, foreach=False) on the CPU, per step from the
    oracle's state: the criterion of tests/test_kernels_gpu.py::test_adam_matches_torch with g' = g + wd p (ATen's one-rounding
    grad.add(param, alpha=wd)) as the gradient operand -- moments within 1 ulp of the larger operand (bitwise on an AVX-512
    host), parameters within 2 ulp-units."""
    lib = N.lib()
    g = torch.Generator().manual_seed(11)
    n = 100003
    p0 = torch.randn(n, generator=g)
    pt = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([pt], lr=LR, weight_decay=wd, foreach=False)
    p = p0.to(dev)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    eps32 = torch.finfo(torch.float32).eps
    worst, bitwise = 0.0, True
    for step in range(1, 9):
        gr = torch.randn(n, generator=g) * (10.0 ** torch.randint(-6, 1, (n,), generator=g).float())
        p_old = pt.detach().clone()
        pt.grad = gr.clone()
        st0 = opt.state[pt]
        m_old = st0["exp_avg"].clone() if "exp_avg" in st0 else torch.zeros(n)
        v_old = st0["exp_avg_sq"].clone() if "exp_avg_sq" in st0 else torch.zeros(n)
        opt.step()
        st = opt.state[pt]
        p.copy_(p_old.to(dev))
        m.copy_(m_old.to(dev))
        v.copy_(v_old.to(dev))
        gd = gr.to(dev)
        N.check(lib.dip_adam_sgld_step(p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), n, LR, B1, B2, EPS, wd, step,
                                       0.0, 0, 0, None, 0, H.stream(dev)), "adam_sgld_step")
        torch.cuda.synchronize()
        g1 = torch.add(gr, p_old, alpha=wd)                         # the decayed gradient, as ATen forms it
        assert ((m.cpu() - st["exp_avg"]).abs() <= eps32 * torch.maximum(m_old.abs(), g1.abs())).all(), step
        assert ((v.cpu() - st["exp_avg_sq"]).abs() <= eps32 * torch.maximum(v_old, g1 * g1)).all(), step
        bitwise = bitwise and torch.equal(m.cpu(), st["exp_avg"]) and torch.equal(v.cpu(), st["exp_avg_sq"])
        p_new = pt.detach()
        d = (p.cpu() - p_new).abs()
        scale = torch.maximum(torch.maximum(p_old.abs(), p_new.abs()), (p_new - p_old).abs())
        r = (d / (eps32 * scale)).max().item()
        worst = max(worst, r)
        assert r <= 2.0, (step, r)
    print(f"adam, weight_decay {wd}: worst parameter deviation {worst:.2f} ulp-units; moments bitwise equal: {bitwise}")


# ------------------------------------------------------------------------------------------ a grouped launch
@pytest.mark.parametrize("mask", [64, 0], ids=["one-dispatch", "host-loop"])
def test_grouped_launch_equals_the_solo_launches(dev, native_mask, mask):
    """B = 3 rows of guard | p | g | m | v | DipIterState | DipSgldState | table | guard with different seeds, offsets and stds,
    ONE dip_adam_sgld_step_dev on row 0's pointers inside dip_group_begin / dip_group_end: every row's p, m, v are its solo
    call's, every offset advanced by ceil(n / 4), every other byte of the slab unchanged."""
    L = native_mask
    n, B, G = 1027, 3, 8
    wd = 5e-8
    rows = [(2 ** 32 - 50, 7, 0.01), (0, 2 ** 32 + 7, 0.02), (5 * 2 ** 32 + 3, 2 ** 64 - 1, 0.03)]        # (offset, seed, std)
    ranges = _tables(n)["off-grid"]
    n4 = N.round_up(n + G, 4)
    p_off = G
    g_off, m_off, v_off = p_off + n4, p_off + 2 * n4, p_off + 3 * n4
    it_off = v_off + n4                                             # 16 bytes
    ns_off = it_off + 4                                             # 24 bytes
    tb_off = ns_off + 6                                             # 16 bytes per range
    row = tb_off + 4 * len(ranges) + G
    stride = N.round_up(row, 64)
    assert all(o % 4 == 0 for o in (p_off, g_off, m_off, v_off, it_off)) and ns_off % 2 == 0 and tb_off % 2 == 0
    data = [_inputs(n, 1, seed=20 + b) for b in range(B)]
    solo = []
    for b, (offset, seed, std) in enumerate(rows):
        p, m, v, grads = data[b]
        solo.append(_fused(dev, n, p, m, v, grads, ranges, std, seed, offset, wd=wd, entry="dev")[0][0])
    assert len({tuple(s[0][:8].tolist()) for s in solo}) == B
    slab = torch.full((B, stride), H.SENTINEL, dtype=torch.float32, device=dev)
    assert slab.data_ptr() % 256 == 0
    words = slab.view(torch.int64)
    for b, (offset, seed, std) in enumerate(rows):
        p, m, v, grads = data[b]
        for off, src in ((p_off, p), (g_off, grads[0]), (m_off, m), (v_off, v)):
            slab[b, off:off + n] = src.to(dev)
        words[b, it_off // 2:it_off // 2 + 2] = 0
        words[b, ns_off // 2:ns_off // 2 + 3] = _sgld_state(dev, offset, seed, std)[1:4]
        words[b, tb_off // 2:tb_off // 2 + 2 * len(ranges)] = torch.tensor([x for r in ranges for x in r], device=dev)
    base = slab.data_ptr()
    at = lambda off: base + 4 * off
    L.dip_group_native(mask)
    N.check(L.dip_group_begin(B, 4 * stride, base, 4 * row), "group_begin")
    try:
        rc = L.dip_adam_tick(at(it_off), LR, B1, B2, H.stream(dev))
        before = None
        if rc == 0:
            torch.cuda.synchronize()
            before = slab.clone()
            rc = L.dip_adam_sgld_step_dev(at(p_off), at(g_off), at(m_off), at(v_off), n, B1, B2, EPS, wd, at(it_off), at(ns_off),
                                          at(tb_off), len(ranges), H.stream(dev))
    finally:
        assert L.dip_group_end() == 0
    N.check(rc, "adam_sgld_step_dev (grouped)")
    torch.cuda.synchronize()
    after = slab.view(torch.int64)
    for b, (offset, seed, std) in enumerate(rows):
        for off, want, name in zip((p_off, m_off, v_off), solo[b], "pmv"):
            assert torch.equal(slab[b, off:off + n].view(torch.int32), want.view(torch.int32)), (b, name)
        s = N.DipSgldState.from_buffer_copy(after[b, ns_off // 2:ns_off // 2 + 3].cpu().numpy().tobytes())
        assert (s.offset, s.seed, s.std) == (offset + 257, seed, np.float32(std)), b
    keep = torch.ones_like(slab, dtype=torch.bool)
    for off in (p_off, m_off, v_off):
        keep[:, off:off + n] = False
    keep[:, ns_off:ns_off + 2] = False                              # the offset word
    assert torch.equal(slab.view(torch.int32)[keep], before.view(torch.int32)[keep])


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing(dev):
    L = N.lib()
    n = 64
    bufs = [_Buf(torch.ones(n), dev) for _ in range(4)]
    keep = [b.raw.clone() for b in bufs]
    st, ns = _iter_state(dev), _sgld_state(dev, 5, 7, 0.1)
    table, tptr = _table_dev([(0, n)], dev)
    ptrs = [b.ptr for b in bufs]
    for k in range(4):
        a = list(ptrs)
        a[k] = None
        assert L.dip_adam_sgld_step_dev(*a, n, B1, B2, EPS, 0.0, st.data_ptr(), ns.data_ptr() + 8, tptr, 1, H.stream(dev)) == -1
        assert b"NULL" in L.dip_last_error()
        assert L.dip_adam_sgld_step(*a, n, LR, B1, B2, EPS, 0.0, 1, 0.1, 7, 5, tptr, 1, H.stream(dev)) == -1
    assert L.dip_adam_sgld_step_dev(*ptrs, n, B1, B2, EPS, 0.0, None, ns.data_ptr() + 8, tptr, 1, H.stream(dev)) == -1
    assert L.dip_adam_sgld_step_dev(*ptrs, n, B1, B2, EPS, 0.0, st.data_ptr(), ns.data_ptr() + 8, None, 1, H.stream(dev)) == -1
    assert b"range table is NULL" in L.dip_last_error()
    long_table = torch.zeros(2 * (S.MAX_RANGES + 1), dtype=torch.int64, device=dev)
    assert L.dip_adam_sgld_step_dev(*ptrs, n, B1, B2, EPS, 0.0, st.data_ptr(), ns.data_ptr() + 8, long_table.data_ptr(),
                                    S.MAX_RANGES + 1, H.stream(dev)) == -1
    assert b"512" in L.dip_last_error()
    assert L.dip_adam_sgld_step_dev(*ptrs, 0, B1, B2, EPS, 0.0, st.data_ptr(), ns.data_ptr() + 8, tptr, 1, H.stream(dev)) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(b.raw, k) for b, k in zip(bufs, keep))
    assert _read_state(ns) == (5, 7, np.float32(0.1)) and int(st.view(torch.int64)[0]) == 0
    # noise == NULL: weight decay only, and the full table of 512 ranges is taken
    full = torch.arange(2 * S.MAX_RANGES, dtype=torch.int64, device=dev)          # [0,1) [2,3) ... (beyond n: ignored)
    N.check(L.dip_adam_tick(st.data_ptr(), LR, B1, B2, H.stream(dev)), "adam_tick")
    N.check(L.dip_adam_sgld_step_dev(*ptrs, n, B1, B2, EPS, 0.0, st.data_ptr(), None, tptr, 1, H.stream(dev)), "no noise")
    torch.cuda.synchronize()
    plain = bufs[0].val.clone()
    assert _read_state(ns) == (5, 7, np.float32(0.1))
    N.check(L.dip_adam_sgld_step_dev(*ptrs, n, B1, B2, EPS, 0.0, st.data_ptr(), ns.data_ptr() + 8, full.data_ptr(),
                                     S.MAX_RANGES, H.stream(dev)), "512 ranges")
    torch.cuda.synchronize()
    assert _read_state(ns)[0] == 5 + n // 4 and all(b.guards_ok() for b in bufs)
    assert len(plain.unique()) == 1
    changed = (bufs[0].val != bufs[0].val[1]).cpu().numpy()          # odd elements are outside every range: all alike
    assert not changed[1::2].any() and changed[0::2].all()
