"""CPU suite of the reg-noise stream (noise_axpy_kernel: Philox4x32-10 + Box-Muller; DESIGN.md "The reg-noise stream"): the
numpy restatement (tests/noise_ref.py) against the published Random123 known-answer vectors, the rounding facts of the
word -> u mapping, the statistics of the stream the restatement defines (tests/test_noise_gpu.py ties the kernel to it element
by element, so these are the kernel's statistics too), and the host-side argument checks of the three entry points."""
import functools
import math

import numpy as np
import pytest
import torch

import noise_ref as R

# ------------------------------------------------------------------------------------------ 1. Philox4x32-10
KAT = [  # counter words | key words -> output words (Random123 kat_vectors, philox4x32 10 rounds)
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    for ctr, key, want in KAT:
        assert tuple(int(w) for w in R.philox4x32_10(ctr, key)) == want, (ctr, key)
    # vectorised over quads: the three at once, and a key broadcast over counters
    got = R.philox4x32_10(np.array([k[0] for k in KAT]), np.array([k[1] for k in KAT]))
    assert got.dtype == np.uint32 and got.tolist() == [list(k[2]) for k in KAT]
    two = R.philox4x32_10(np.array([KAT[0][0], KAT[0][0]]), np.array(KAT[0][1]))
    assert two.tolist() == [list(KAT[0][2])] * 2
    # nine rounds are another generator (the vectors can tell)
    assert tuple(int(w) for w in R.philox4x32_10(KAT[0][0], KAT[0][1], rounds=9)) != KAT[0][2]


def test_counter_and_key_layout():
    """words(): counter {lo(q + offset), hi(q + offset), 0, 0}, key {lo(seed), hi(seed)}, 64-bit sums."""
    seed, off = (0x299f31d0 << 32) | 0xa4093822, (0x85a308d3 << 32) | 0x243f6a88
    w = R.words(9, seed, off - 1)                      # 3 quads: counters off - 1, off, off + 1
    assert w.shape == (3, 4)
    assert w[1].tolist() == R.philox4x32_10((0x243f6a88, 0x85a308d3, 0, 0), (0xa4093822, 0x299f31d0)).tolist()
    # the carry out of the low word reaches the high word; the sum wraps modulo 2^64
    w = R.words(8, 7, 2 ** 32 - 1)
    assert w[0].tolist() == R.philox4x32_10((0xffffffff, 0, 0, 0), (7, 0)).tolist()
    assert w[1].tolist() == R.philox4x32_10((0, 1, 0, 0), (7, 0)).tolist()
    w = R.words(8, 2 ** 64 - 1, 2 ** 64 - 1)
    assert w[0].tolist() == R.philox4x32_10((0xffffffff, 0xffffffff, 0, 0), (0xffffffff, 0xffffffff)).tolist()
    assert w[1].tolist() == R.philox4x32_10((0, 0, 0, 0), (0xffffffff, 0xffffffff)).tolist()
    # high words matter: neither the seed's nor the offset's may be dropped
    assert not np.array_equal(R.words(4, 7, 0), R.words(4, 2 ** 32 + 7, 0))
    assert not np.array_equal(R.words(4, 7, 3), R.words(4, 7, 2 ** 32 + 3))
    for n, nq in ((1, 1), (3, 1), (4, 1), (5, 2), (1027, 257)):
        assert R.words(n, 1, 0).shape == (nq, 4) and R.normals(n, 1, 0).shape == (n,) and R.normals32(n, 1, 0).shape == (n,)
    assert R.normals(5, 1, 0).dtype == np.float64 and R.normals32(5, 1, 0).dtype == np.float32
    # ragged n: the first n elements of the next multiple of four; the next call starts one quad later
    assert np.array_equal(R.normals(1027, 7, 0), R.normals(1028, 7, 0)[:1027])
    assert np.array_equal(R.normals(1028, 7, 0)[4:], R.normals(1024, 7, 1))


# ------------------------------------------------------------------------------------------ 2. the word -> u mapping
def test_rounding_facts_of_u():
    u = R.uniform(np.array([0xffffffff, 0xffffff00, 0, 0xff, 0x100], dtype=np.uint32))
    assert u.dtype == np.float32
    assert u[0] == 1.0 and u[1] == 1.0                               # 2^24 - 1 + 0.5 ties to even: 2^24
    assert u[2] == np.float32(2.0 ** -25) and u[3] == u[2]            # the low 8 bits do not count
    assert u[4] == np.float32(1.5 * 2.0 ** -24)
    # u == 1: radius 0, the pair is (0, +-0) whatever the angle
    z = R._box_muller(R.uniform(np.array([[0xffffffff, 0x12345678, 0xffffffff, 0xffffffff]], dtype=np.uint32)), np.float64)
    assert np.all(z == 0.0)
    z = R._box_muller(R.uniform(np.array([[0xffffffff, 0x12345678, 0xffffffff, 0]], dtype=np.uint32)), np.float32)
    assert np.all(z == 0.0)
    # u == 2^-25: the largest radius, sqrt(50 ln 2)
    z = R._box_muller(R.uniform(np.array([[0, 0, 0, 0x40000000]], dtype=np.uint32)), np.float64)
    rmax = math.sqrt(50.0 * math.log(2.0))
    assert abs(rmax - 5.887) < 1e-3
    assert abs(math.hypot(z[0], z[1]) - rmax) < 1e-12 and abs(math.hypot(z[2], z[3]) - rmax) < 1e-12
    assert np.abs(z).max() <= rmax + 1e-12 and abs(z[0] - rmax) < 1e-6


def test_u_is_in_0_1_for_every_word():
    """All 2^24 values of w >> 8: u in [2^-25, 1], non-decreasing, on the grid (k + 0.5) 2^-24 below 2^23 and on the
    ties-to-even grid (even k stays k, odd k becomes k + 1) from 2^23 up."""
    k = np.arange(1 << 24, dtype=np.uint32)
    u = R.uniform(k << np.uint32(8))
    assert u.min() == np.float32(2.0 ** -25) and u.max() == 1.0
    assert not np.any(u <= 0) and not np.any(u > 1) and np.all(np.diff(u) >= 0)
    half = 1 << 23
    assert np.array_equal(u[:half].astype(np.float64) * 2.0 ** 24, k[:half] + 0.5)
    assert np.array_equal(u[half:].astype(np.float64) * 2.0 ** 24, (k[half:] + (k[half:] & 1)).astype(np.float64))


# ------------------------------------------------------------------------------------------ 3. the stream is a normal stream
NS = 1 << 20
# 5 sigma of each estimator under independence at n = 2^20, Kolmogorov-Smirnov at alpha = 1e-6:
#   KS    sqrt(ln(2 / 1e-6) / 2) / sqrt(n) = 2.630e-3         mean  5 / sqrt(n)          = 4.88e-3
#   std   5 / sqrt(2 n)                    = 3.45e-3          E x^4 5 sqrt(96 / n)       = 4.78e-2   (Var x^4 = 105 - 9)
#   correlations 5 / sqrt(n) = 4.88e-3
KS_MAX, MEAN_MAX, STD_MAX, KURT_MAX, CORR_MAX = 2.63e-3, 4.9e-3, 3.5e-3, 4.8e-2, 4.9e-3
DRAWS = [(7, 0), (40, 0), (41, 0), (1234, 0), (2 ** 32 + 7, 0), (7, 2 ** 32 - NS // 8)]
DRAW_IDS = ["seed7", "seed40", "seed41", "seed1234", "seed2^32+7", "seed7-across-2^32"]


@functools.lru_cache(maxsize=None)
def _draw(seed, offset):
    x = R.normals(NS, seed, offset)
    x.setflags(write=False)
    return x


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


def _ks(x):
    xs = np.sort(x)
    cdf = 0.5 * (1.0 + torch.erf(torch.from_numpy(xs / math.sqrt(2.0))).numpy())
    n = xs.size
    return float(max((np.arange(1, n + 1) / n - cdf).max(), (cdf - np.arange(0, n) / n).max()))


def test_thresholds_are_the_derived_ones():
    """The bounds above are the formulas' values at n = 2^20, rounded to two or three digits: nothing was tuned."""
    for bound, derived in ((KS_MAX, math.sqrt(math.log(2.0 / 1e-6) / 2.0) / math.sqrt(NS)), (MEAN_MAX, 5.0 / math.sqrt(NS)),
                           (CORR_MAX, 5.0 / math.sqrt(NS)), (STD_MAX, 5.0 / math.sqrt(2.0 * NS)),
                           (KURT_MAX, 5.0 * math.sqrt(96.0 / NS))):
        assert abs(bound / derived - 1.0) < 0.02, (bound, derived)


@pytest.mark.parametrize("seed,offset", DRAWS, ids=DRAW_IDS)
def test_reference_stream_is_normal(seed, offset):
    x = _draw(seed, offset)
    assert x.shape == (NS,) and np.all(np.isfinite(x))
    ks, mean, std, m4 = _ks(x), float(x.mean()), float(x.std()), float((x ** 4).mean())
    lags = [_corr(x[:-k], x[k:]) for k in (1, 2, 3, 4)]              # lags 1..3 stay inside a quad
    print(f"seed {seed} offset {offset}: KS {ks:.3e} mean {mean:.3e} std-1 {std - 1:.3e} Ex4-3 {m4 - 3:.3e} "
          f"lags {' '.join(f'{c:.2e}' for c in lags)}")
    assert ks < KS_MAX
    assert abs(mean) < MEAN_MAX
    assert abs(std - 1.0) < STD_MAX
    assert abs(m4 - 3.0) < KURT_MAX
    for k, c in zip((1, 2, 3, 4), lags):
        assert abs(c) < CORR_MAX, (k, c)
    assert np.abs(x).max() <= math.sqrt(50.0 * math.log(2.0)) + 1e-12


def test_streams_are_uncorrelated():
    a = _draw(7, 0)
    pairs = {"seed 7 vs seed 8": R.normals(NS, 8, 0), "seed 7 vs seed 2^32 + 7": _draw(2 ** 32 + 7, 0),
             "a call vs the next call": R.normals(NS, 7, NS // 4)}
    for name, b in pairs.items():
        c = _corr(a, b)
        print(f"{name}: correlation {c:.2e}")
        assert abs(c) < CORR_MAX, name
    # the draw across 2^32 continues the stream: its second half is the draw at offset 2^32
    assert np.array_equal(_draw(7, 2 ** 32 - NS // 8)[NS // 2:], R.normals(NS // 2, 7, 2 ** 32))
    assert not np.array_equal(_draw(7, 2 ** 32 - NS // 8)[NS // 2:], R.normals(NS // 2, 7, 0))


def test_float32_evaluation_stays_close():
    """normals32 is the same stream evaluated in float32: its distance from the float64 evaluation (the yardstick of the
    kernel's tolerance in tests/test_noise_gpu.py) is a few float32 roundings at |x| <= 5.9."""
    e32 = float(np.abs(R.normals32(NS, 7, 0).astype(np.float64) - _draw(7, 0)).max())
    print(f"e32 {e32:.3e} over 2^20 draws, max |x| {np.abs(_draw(7, 0)).max():.2f}")
    assert 0 < e32 < 1e-5


# ------------------------------------------------------------------------------------------ 4. argument validation
def test_entry_points_validate_on_the_host_before_any_launch(built):
    L = built
    fake = 1 << 20
    calls = {
        "noise_axpy": lambda z, out, n: L.dip_noise_axpy(z, out, n, 0.5, 7, 0, None),
        "noise_axpy_dev": lambda z, out, n: L.dip_noise_axpy_dev(z, out, n, 0.5, 7, fake, None),
        "noise_axpy_dev2": lambda z, out, n: L.dip_noise_axpy_dev2(z, out, n, 0.5, fake, None),
    }
    for name, call in calls.items():
        for z, out in ((None, fake), (fake, None), (None, None)):
            assert call(z, out, 16) == -1, (name, z, out)
            assert name.encode() + b": z or out is NULL" in L.dip_last_error(), (name, z, out)
        for n in (0, -1, -(1 << 40)):
            assert call(None, None, n) == 0, (name, n)
            assert call(fake, fake, n) == 0, (name, n)
    # the counter / state pointer is still refused first
    assert L.dip_noise_axpy_dev(fake, fake, 16, 0.5, 7, None, None) == -1
    assert b"noise_axpy_dev: offset pointer is NULL" in L.dip_last_error()
    assert L.dip_noise_axpy_dev2(fake, fake, 16, 0.5, None, None) == -1
    assert b"noise_axpy_dev2: state pointer is NULL" in L.dip_last_error()
    assert L.dip_noise_axpy_dev(fake, fake, 0, 0.5, 7, None, None) == 0
    assert L.dip_noise_axpy_dev2(fake, fake, 0, 0.5, None, None) == 0
