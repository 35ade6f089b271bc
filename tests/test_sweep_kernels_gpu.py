"""The entry points that read a hyper-parameter from device memory, on a real MI355X, against the entry points that take it by
value: dip_adam_tick_dev against dip_adam_tick, dip_noise_axpy_dev3 against dip_noise_axpy_dev2, dip_noise_axpy_dev1s against
dip_noise_axpy_dev -- solo, and inside dip_group_begin / dip_group_end with another scalar in every row, in both forms a kernel
family can take.  They run the same kernel bodies on the same values, so every comparison is byte equality."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import dip_native as N  # noqa: E402
from test_group_gpu import ALL, native_mask  # noqa: E402,F401

LRS = (0.01, 1e-3, 0.1, 1. / 3., 0.0)
SIZES = (1, 3, 4, 5, 1023, 1025, 36 * 52 * 8)             # the quad tail, one block and two, the net input of the group tests
GUARD = 64
ROW = 256                                                  # bytes per instance in the grouped tick test
MASKS = pytest.mark.parametrize("mask", [ALL, 0], ids=["one-dispatch", "host-loop"])
B1, B2 = 0.9, 0.999


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ------------------------------------------------------------------------------------------ dip_adam_tick_dev
def test_tick_reads_lr_from_the_device(dev):
    """Steps 1..6 from a zeroed DipIterState: the 16 state bytes after every step are dip_adam_tick's."""
    L, st = N.lib(), _stream(dev)
    for lr in LRS:
        a = torch.zeros(16, dtype=torch.uint8, device=dev)
        b = torch.zeros(16, dtype=torch.uint8, device=dev)
        lr_dev = torch.full((1,), lr, dtype=torch.float64, device=dev)
        got, want = [], []
        for _ in range(6):
            N.check(L.dip_adam_tick(a.data_ptr(), lr, B1, B2, st), "adam_tick")
            N.check(L.dip_adam_tick_dev(b.data_ptr(), lr_dev.data_ptr(), B1, B2, st), "adam_tick_dev")
            want.append(a.clone())
            got.append(b.clone())
        assert torch.equal(torch.stack(got), torch.stack(want)), lr
        assert got[-1].view(torch.int64)[0].item() == 6
        assert (got[0].view(torch.float32)[2].item() == 0.0) == (lr == 0.0)           # step_size = lr / bc1
        assert lr_dev.item() == lr                                                    # (read only)
    # a rewritten scalar is read by the next launch, in stream order
    lr_dev.fill_(0.01)
    a.zero_()
    b.zero_()
    N.check(L.dip_adam_tick(a.data_ptr(), 0.01, B1, B2, st), "adam_tick")
    N.check(L.dip_adam_tick_dev(b.data_ptr(), lr_dev.data_ptr(), B1, B2, st), "adam_tick_dev")
    lr_dev.fill_(0.1)
    N.check(L.dip_adam_tick(a.data_ptr(), 0.1, B1, B2, st), "adam_tick")
    N.check(L.dip_adam_tick_dev(b.data_ptr(), lr_dev.data_ptr(), B1, B2, st), "adam_tick_dev")
    assert torch.equal(a, b)


@MASKS
def test_tick_in_a_group_reads_every_rows_own_lr(dev, native_mask, mask):
    """B = 3 rows {DipIterState at 0, lr at 64, the rest sentinel}: ONE grouped dip_adam_tick_dev per step against three solo
    dip_adam_tick calls with the rows' lrs."""
    L, st, B = native_mask, _stream(dev), 3
    lrs = [0.01, 1e-3, 0.1]
    rows = torch.full((B, ROW), 0xA5, dtype=torch.uint8, device=dev)
    rows[:, :16] = 0
    for b, lr in enumerate(lrs):
        rows[b, 64:72].view(torch.float64).fill_(lr)
    init = rows.clone()
    solo = torch.zeros(B, 16, dtype=torch.uint8, device=dev)
    L.dip_group_native(mask)
    assert rows.data_ptr() % 256 == 0
    for step in range(6):
        for b, lr in enumerate(lrs):
            N.check(L.dip_adam_tick(solo[b].data_ptr(), lr, B1, B2, st), "adam_tick")
        assert L.dip_group_begin(B, ROW, rows.data_ptr(), ROW) == 0
        try:
            N.check(L.dip_adam_tick_dev(rows.data_ptr(), rows.data_ptr() + 64, B1, B2, st), "adam_tick_dev")
        finally:
            assert L.dip_group_end() == 0
        assert torch.equal(rows[:, :16], solo), step
    assert torch.equal(rows[:, 16:], init[:, 16:])                                    # the lrs and the sentinels stand
    assert len({rows[b, 8:12].view(torch.float32).item() for b in range(B)}) == B     # three step sizes
    # a pointer outside row 0 is refused by the group's range check, like any other
    other = torch.zeros(1, dtype=torch.float64, device=dev)
    assert L.dip_group_begin(B, ROW, rows.data_ptr(), ROW) == 0
    try:
        assert L.dip_adam_tick_dev(rows.data_ptr(), other.data_ptr(), B1, B2, st) != 0
    finally:
        assert L.dip_group_end() == 0
    assert torch.equal(rows[:, :16], solo)


# ------------------------------------------------------------------------------------------ dip_noise_axpy_dev3 / _dev1s
def _buffers(n, dev, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n + GUARD, generator=g).to(dev)
    out = torch.full((n + GUARD,), float("nan"), device=dev)
    return z, out


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("sigma", [1. / 30., 0.0], ids=["sigma-1/30", "sigma-0"])
@pytest.mark.parametrize("n", SIZES)
def test_dev3_equals_dev2(dev, n, sigma):
    """Two consecutive calls each: outputs, {offset, seed} and the NaN-filled elements behind n."""
    L, st = N.lib(), _stream(dev)
    z, out2 = _buffers(n, dev, n)
    _, out3 = _buffers(n, dev, n)
    s2 = torch.tensor([5, 2 ** 32 + 7], dtype=torch.int64, device=dev)
    s3 = s2.clone()
    sig = torch.full((1,), sigma, dtype=torch.float32, device=dev)
    quads = (n + 3) // 4
    prev = None
    for call in range(2):
        N.check(L.dip_noise_axpy_dev2(z.data_ptr(), out2.data_ptr(), n, sigma, s2.data_ptr(), st), "noise_axpy_dev2")
        N.check(L.dip_noise_axpy_dev3(z.data_ptr(), out3.data_ptr(), n, sig.data_ptr(), s3.data_ptr(), st), "noise_axpy_dev3")
        assert _same_bits(out3[:n], out2[:n]) and not bool(torch.isnan(out3[:n]).any()), (n, call)
        assert bool(torch.isnan(out3[n:]).all()) and bool(torch.isnan(out2[n:]).all()), (n, call)
        assert torch.equal(s3, s2) and s3.tolist() == [5 + (call + 1) * quads, 2 ** 32 + 7], (n, call)
        if sigma > 0 and n >= 4:
            assert prev is None or not torch.equal(prev, out3[:n])                   # the second call draws other normals
            prev = out3[:n].clone()
        if sigma == 0:
            assert torch.equal(out3[:n], z[:n])                                       # z + 0 * N (equal up to the sign of zero)
    assert sig.item() == torch.tensor(sigma).float().item()


@pytest.mark.parametrize("n", SIZES)
def test_dev1s_equals_dev(dev, n):
    L, st = N.lib(), _stream(dev)
    z, out1 = _buffers(n, dev, n + 1)
    _, outs = _buffers(n, dev, n + 1)
    seed = 2 ** 64 - 3
    o1 = torch.tensor([11], dtype=torch.int64, device=dev)
    os_ = o1.clone()
    sig = torch.full((1,), 0.05, dtype=torch.float32, device=dev)
    quads = (n + 3) // 4
    for call in range(2):
        N.check(L.dip_noise_axpy_dev(z.data_ptr(), out1.data_ptr(), n, 0.05, seed, o1.data_ptr(), st), "noise_axpy_dev")
        N.check(L.dip_noise_axpy_dev1s(z.data_ptr(), outs.data_ptr(), n, sig.data_ptr(), seed, os_.data_ptr(), st),
                "noise_axpy_dev1s")
        assert _same_bits(outs[:n], out1[:n]) and not bool(torch.isnan(outs[:n]).any()), (n, call)
        assert bool(torch.isnan(outs[n:]).all()), (n, call)
        assert torch.equal(os_, o1) and os_.item() == 11 + (call + 1) * quads, (n, call)


@MASKS
@pytest.mark.parametrize("n", [5, 1025])
def test_dev3_in_a_group_reads_every_rows_own_sigma(dev, native_mask, mask, n):
    """B = 3 rows {z, out, sigma, {offset, seed}} with another level (one of them 0) and another seed per row: ONE grouped
    dip_noise_axpy_dev3 against three solo dip_noise_axpy_dev2 calls."""
    L, st, B = native_mask, _stream(dev), 3
    sigmas, seeds = [1. / 30., 0.0, 1. / 20.], [40, 41, 2 ** 40 + 1]
    nz = (n + GUARD + 63) // 64 * 64
    o_z, o_out, o_sig, o_st = 0, nz, 2 * nz, 2 * nz + 64                 # in floats; every buffer 256-byte aligned
    nrow = 2 * nz + 128
    g = torch.Generator().manual_seed(n)
    rows = torch.full((B, nrow), float("nan"), device=dev)
    rows[:, o_z:o_z + n] = torch.randn(B, n, generator=g).to(dev)
    for b in range(B):
        rows[b, o_sig] = sigmas[b]
        rows[b, o_st:o_st + 4].view(torch.int64).copy_(torch.tensor([3 * b, seeds[b]], dtype=torch.int64))
    solo = rows.clone()
    L.dip_group_native(mask)
    p = lambda t, b, o: t.data_ptr() + 4 * (b * nrow + o)
    for call in range(2):
        for b in range(B):
            N.check(L.dip_noise_axpy_dev2(p(solo, b, o_z), p(solo, b, o_out), n, sigmas[b], p(solo, b, o_st), st), "noise_axpy_dev2")
        assert L.dip_group_begin(B, 4 * nrow, rows.data_ptr(), 4 * nrow) == 0
        try:
            N.check(L.dip_noise_axpy_dev3(p(rows, 0, o_z), p(rows, 0, o_out), n, p(rows, 0, o_sig), p(rows, 0, o_st), st),
                    "noise_axpy_dev3")
        finally:
            assert L.dip_group_end() == 0
        assert _same_bits(rows, solo), call                                # outputs, states, and every NaN where it was
        assert not bool(torch.isnan(rows[:, o_out:o_out + n]).any()) and bool(torch.isnan(rows[:, o_out + n:o_sig]).all())
    assert torch.equal(rows[1, o_out:o_out + n], rows[1, o_z:o_z + n])     # the row at level 0: z + 0 * N
    assert not torch.equal(rows[0, o_out:o_out + n], rows[0, o_z:o_z + n])
