"""The reg-noise kernel on a real MI355X (noise_axpy_kernel, csrc/misc_kernels.hip, through dip_noise_axpy, dip_noise_axpy_dev
and dip_noise_axpy_dev2) against the numpy restatement of its stream (tests/noise_ref.py; DESIGN.md "The reg-noise stream"):
(a) element-by-element parity with the float64 evaluation, (b) the structure of the stream -- shifts, the scalar path, ragged
sizes, the device counter, continuity, the device seed -- bitwise, (c) one grouped launch over rows with different streams,
(d) utils.reg_noise.RegNoise.  The statistics of the stream are those of the reference (tests/test_noise_host.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dip_native as N  # noqa: E402
import hipops as H  # noqa: E402
import noise_ref as R  # noqa: E402

SIZES = [1, 3, 4, 5, 1023, 1024, 1027, 3075]      # one element, every n % 4, one 256-quad block, three blocks + a ragged quad
SEEDS = [7, 2 ** 32 + 7, 2 ** 64 - 1]
OFFSETS = [0, 2 ** 32 - 100, 5 * 2 ** 32 + 3]     # the middle one: the 32-bit boundary falls inside the launch (quad 100)
SEED_IDS = ["seed7", "seed2^32+7", "seed2^64-1"]
OFFSET_IDS = ["off0", "off2^32-100", "off5*2^32+3"]
# The kernel evaluates Box-Muller with the hardware's log2 / sin / cos (v_log_f32, v_sin_f32, v_cos_f32) and two more fp32
# multiplications on the angle, where numpy's float32 evaluation (noise_ref.normals32, error e32) has three correctly rounded
# library calls: about four extra error terms of the size e32 is made of, the angle's multiplied by the radius (<= 5.9);
# doubled: 8 x e32, plus the project's floor of 2e-6 max|ref| (tests/test_kernels_gpu.py: _check).
NOISE_RATIO = 8.0
FLOOR = 2e-6


def _zeros(n, dev):
    return torch.zeros(n, dtype=torch.float32, device=dev)


def _host(n, seed, offset, dev, sigma=0.5, **kw):
    return H.noise_axpy(_zeros(n, dev), sigma, seed, offset, "host", **kw)[0]


def _tolerance(ref64, ref32):
    e32 = float(np.abs(ref32.astype(np.float64) - ref64).max())
    scale = float(np.abs(ref64).max())
    return e32, scale, max(NOISE_RATIO * e32, FLOOR * scale)


# ------------------------------------------------------------------------------------------ (a) parity
@pytest.mark.parametrize("offset", OFFSETS, ids=OFFSET_IDS)
@pytest.mark.parametrize("seed", SEEDS, ids=SEED_IDS)
def test_parity_with_the_reference(dev, seed, offset):
    """(out - z) / sigma with z = 0, sigma = 0.5 (out is the kernel's normal halved, exactly) against normals() at every
    size; the tolerance is measured on the same draws (the sizes share their leading elements: 3075 distinct draws)."""
    nmax = max(SIZES)
    ref64, ref32 = R.normals(nmax, seed, offset), R.normals32(nmax, seed, offset)
    e32, scale, tol = _tolerance(ref64, ref32)
    worst = 0.0
    for n in SIZES:
        out = _host(n, seed, offset, dev)
        got = out.cpu().double().numpy() / 0.5
        assert got.shape == (n,) and np.all(np.isfinite(got)), n
        err = float(np.abs(got - ref64[:n]).max())
        worst = max(worst, err)
        assert err <= tol, f"n {n}: max|err| {err:.3e} > tol {tol:.3e} (numpy-fp32 err {e32:.3e}, scale {scale:.3e})"
    print(f"noise seed {seed} offset {offset}: err/e32 {worst / e32:.3f} err/tol {worst / tol:.3f} (err {worst:.3e}, "
          f"numpy-fp32 err {e32:.3e}, scale {scale:.3e})")


def test_axpy_is_one_fma(dev):
    """z ~ U(0, 0.1), sigma = 1/30: out == fmaf(sigma, nrm, z) to 1 ulp of out, nrm being the kernel's own normal (z = 0 run)."""
    n, seed, offset = 1024, 7, 2 ** 32 - 100
    nrm = _host(n, seed, offset, dev, sigma=1.0)                      # fmaf(1, nrm, 0) == nrm
    assert torch.equal(nrm * 0.5, _host(n, seed, offset, dev, sigma=0.5))
    g = torch.Generator().manual_seed(3)
    z = (torch.rand(n, generator=g) * 0.1).to(dev)
    sigma = np.float32(1.0 / 30.0)
    out, _ = H.noise_axpy(z, float(sigma), seed, offset, "host")
    want = float(sigma) * nrm.cpu().double().numpy() + z.cpu().double().numpy()       # product exact, one fp64 rounding
    got = out.cpu().numpy()
    ulp = np.spacing(np.abs(got)).astype(np.float64)
    d = np.abs(got.astype(np.float64) - want) / ulp
    print(f"axpy: worst deviation {d.max():.3f} ulp of out")
    assert np.all(d <= 1.0)


# ------------------------------------------------------------------------------------------ (b) structure, bitwise
@pytest.mark.parametrize("k", [1, 37])
def test_offset_shifts_the_stream_by_quads(dev, k):
    n, seed = 3075, 2 ** 32 + 7
    for base in (0, 2 ** 32 - 20):
        a, b = _host(n, seed, base, dev), _host(n, seed, base + k, dev)
        assert torch.equal(b[:n - 4 * k], a[4 * k:]), base
        assert not torch.equal(b[:n - 4 * k], a[:n - 4 * k])


@pytest.mark.parametrize("n", [5, 1024, 1027])
def test_scalar_path_equals_vector_path(dev, n):
    """z and out one float past a 16-byte boundary, in all four combinations: the same values as the aligned call."""
    seed, offset = 2 ** 64 - 1, 2 ** 32 - 100
    g = torch.Generator().manual_seed(n)
    z = (torch.rand(n, generator=g) * 0.1).to(dev)
    want, _ = H.noise_axpy(z, 1.0 / 30.0, seed, offset, "host")
    for zs, os_ in ((0, 1), (1, 0), (1, 1)):
        got, _ = H.noise_axpy(z, 1.0 / 30.0, seed, offset, "host", z_shift=zs, out_shift=os_)
        assert torch.equal(got, want), (zs, os_)
    for variant in ("dev", "dev2"):
        got, _ = H.noise_axpy(z, 1.0 / 30.0, seed, offset, variant, z_shift=1, out_shift=1)
        assert torch.equal(got, want), variant


@pytest.mark.parametrize("n", [1, 3, 5, 1023, 1027, 3075])
def test_ragged_sizes_are_prefixes(dev, n):
    """The first n elements equal those of the next multiple of four (the sentinels behind out[n - 1] are checked by the
    wrapper at every call)."""
    seed, offset = 7, 5 * 2 ** 32 + 3
    full = _host((n + 3) // 4 * 4, seed, offset, dev)
    assert torch.equal(_host(n, seed, offset, dev), full[:n])
    assert torch.equal(_host(n, seed, offset, dev, out_shift=1), full[:n])


@pytest.mark.parametrize("offset", OFFSETS, ids=OFFSET_IDS)
@pytest.mark.parametrize("n", SIZES)
def test_device_counter_equals_host_offset(dev, n, offset):
    seed = 2 ** 32 + 7
    want = _host(n, seed, offset, dev)
    got, counter = H.noise_axpy(_zeros(n, dev), 0.5, seed, offset, "dev")
    assert torch.equal(got, want)
    assert counter == offset + (n + 3) // 4
    # the seed argument counts, both halves
    for other in (seed - 2 ** 32, seed + 1):
        assert not torch.equal(H.noise_axpy(_zeros(n, dev), 0.5, other, offset, "dev")[0], want)


@pytest.mark.parametrize("offset", [0, 2 ** 32 - 300], ids=["off0", "off2^32-300"])
def test_calls_continue_the_stream(dev, offset):
    seed = 2 ** 64 - 1
    # a ragged call consumes ceil(n / 4) counters: the next call starts at the next quad, no Philox block is used twice
    n1, n2 = 1027, 1024
    state = H.noise_state(dev, offset)
    a, c1 = H.noise_axpy(_zeros(n1, dev), 0.5, seed, None, "dev", state=state)
    b, c2 = H.noise_axpy(_zeros(n2, dev), 0.5, seed, None, "dev", state=state)
    assert (c1, c2) == (offset + 257, offset + 257 + 256)
    assert torch.equal(a, _host(n1, seed, offset, dev))
    assert torch.equal(b, _host(n2, seed, offset + 257, dev))
    assert not torch.equal(b, _host(n2, seed, offset + 256, dev))
    # n1 % 4 == 0: two calls are one call of n1 + n2, for both device variants
    n1 = 1024
    whole = _host(n1 + n2, seed, offset, dev)
    for variant in ("dev", "dev2"):
        state = H.noise_state(dev, offset, seed if variant == "dev2" else None)
        a, _ = H.noise_axpy(_zeros(n1, dev), 0.5, seed, None, variant, state=state)
        b, _ = H.noise_axpy(_zeros(n2, dev), 0.5, seed, None, variant, state=state)
        assert torch.equal(torch.cat([a, b]), whole), variant
        assert H.as_u64(state[1].item()) == offset + 512


@pytest.mark.parametrize("offset", OFFSETS, ids=OFFSET_IDS)
@pytest.mark.parametrize("seed", SEEDS, ids=SEED_IDS)
def test_device_seed_equals_host_seed(dev, seed, offset):
    for n in (5, 1027):
        want = _host(n, seed, offset, dev)
        got, (counter, seed_word) = H.noise_axpy(_zeros(n, dev), 0.5, seed, offset, "dev2")
        assert torch.equal(got, want), n
        assert counter == offset + (n + 3) // 4 and seed_word == seed, n       # the counter word advances, the seed word stays
        # state[1] is the seed: another value there is another stream, and the offset is not read as the seed
        other, _ = H.noise_axpy(_zeros(n, dev), 0.5, seed ^ (1 << 33), offset, "dev2")
        assert not torch.equal(other, want), n
        if seed != offset:
            assert not torch.equal(got, _host(n, offset, offset, dev)), n


# ------------------------------------------------------------------------------------------ (c) a grouped launch
@pytest.fixture
def native_mask():
    lib = N.lib()
    prev = lib.dip_group_native(-1)
    yield lib
    lib.dip_group_native(prev)
    assert lib.dip_group_size() == 1


@pytest.mark.parametrize("mask", [64, 0], ids=["one-dispatch", "host-loop"])
def test_grouped_launch_gives_every_row_its_own_stream(dev, native_mask, mask):
    """B = 3 rows of guard | z | guard | out | guard | {offset, seed} | guard with different offsets and seeds, ONE
    dip_noise_axpy_dev2 call on row 0's pointers inside dip_group_begin / dip_group_end: every row's out is its solo dev2 call's,
    every counter advanced by ceil(n / 4), every seed word and every other word of the slab unchanged."""
    L = native_mask
    n, B, G = 1027, 3, 8
    sigma = 1.0 / 30.0
    states = [(2 ** 32 - 50, 7), (0, 2 ** 32 + 7), (5 * 2 ** 32 + 3, 2 ** 64 - 1)]          # (offset, seed) per row
    z_off = G
    out_off = N.round_up(z_off + n + G, 4)
    st_off = N.round_up(out_off + n + G, 4)                     # two uint64 = four floats, 16-byte aligned
    row = st_off + 4 + G
    stride = N.round_up(row, 64)                                # floats: a multiple of 256 bytes
    assert (4 * stride) % 256 == 0 and stride > row
    g = torch.Generator().manual_seed(11)
    zs = [(torch.rand(n, generator=g) * 0.1).to(dev) for _ in range(B)]
    solo = [H.noise_axpy(zs[b], sigma, states[b][1], states[b][0], "dev2")[0] for b in range(B)]
    assert len({tuple(s[:8].tolist()) for s in solo}) == B      # the rows really are different streams

    slab = torch.full((B, stride), H.SENTINEL, dtype=torch.float32, device=dev)
    assert slab.data_ptr() % 256 == 0
    words = slab.view(torch.int64)                              # [B, stride / 2]
    for b in range(B):
        slab[b, z_off:z_off + n] = zs[b]
        slab[b, out_off:out_off + n] = float("nan")
        words[b, st_off // 2] = H.as_i64(states[b][0])
        words[b, st_off // 2 + 1] = H.as_i64(states[b][1])
    before = slab.clone()
    base = slab.data_ptr()
    L.dip_group_native(mask)
    N.check(L.dip_group_begin(B, 4 * stride, base, 4 * row), "group_begin")
    try:
        rc = L.dip_noise_axpy_dev2(base + 4 * z_off, base + 4 * out_off, n, sigma, base + 4 * st_off, H.stream(dev))
    finally:
        assert L.dip_group_end() == 0
    N.check(rc, "noise_axpy_dev2 (grouped)")
    torch.cuda.synchronize()
    after_words = slab.view(torch.int64)
    for b in range(B):
        assert torch.equal(slab[b, out_off:out_off + n], solo[b]), b
        assert H.as_u64(after_words[b, st_off // 2].item()) == states[b][0] + 257, b
        assert H.as_u64(after_words[b, st_off // 2 + 1].item()) == states[b][1], b
    # everything but out and the counter word: the guards, z, the seed words, the slack between the rows
    keep = torch.ones_like(slab, dtype=torch.bool)
    keep[:, out_off:out_off + n] = False
    keep[:, st_off:st_off + 2] = False
    assert torch.equal(slab.view(torch.int32)[keep], before.view(torch.int32)[keep])


# ------------------------------------------------------------------------------------------ (d) RegNoise
def test_reg_noise_follows_the_stream(dev):
    from utils.reg_noise import RegNoise
    seed, std = 2 ** 32 + 7, 0.03
    g = torch.Generator().manual_seed(5)
    z = (torch.rand(1, 3, 5, 7, generator=g) * 0.1).to(dev)              # 105 elements: numel % 4 == 1, 27 quads a call
    reg = RegNoise(z, std, seed=seed)
    z64 = z.cpu().double().numpy().reshape(-1)
    for k in range(3):
        out = reg()
        torch.cuda.synchronize()
        assert out.shape == z.shape
        ref64, ref32 = R.normals(105, seed, 27 * k), R.normals32(105, seed, 27 * k)
        e32, scale, tol = _tolerance(ref64, ref32)
        # + one rounding of the fma's result (|out| < 0.5: half an ulp is at most 2^-26)
        err = float(np.abs(out.cpu().double().numpy().reshape(-1) - (z64 + float(np.float32(std)) * ref64)).max())
        print(f"RegNoise call {k}: err {err:.3e}, tol {std * tol + 2.0 ** -26:.3e}")
        assert err <= std * tol + 2.0 ** -26, k
        assert reg.offset.item() == 27 * (k + 1)
    assert reg.offset.item() == 81
