"""CPU suite of the grouped posterior (utils.fit_monitor.GroupedPosteriorMonitor, dip_group.GroupedFits(posterior=),
dip_posterior_pool, dip_posterior_rec_dev): the ABI of the two entry points, what is refused at construction, where the post_
rows lie in a slab row, and the yardstick of the pooled arithmetic -- the numpy-float32 restatement (tests/posterior_pool_ref.py)
against the textbook fp64 formula on raw samples.  Nothing is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import posterior_pool_ref as R
from test_sgld_host import _dry_group

P = 1 << 20                                  # a pointer that is never dereferenced: the call is refused first


# ------------------------------------------------------------------------------------------ ABI
def test_header_binding_and_library_know_the_entry_points(built):
    import dip_native as N
    hdr = open(os.path.join(ROOT, "include", "dip_hip.h")).read()
    assert re.search(r"^int dip_posterior_rec_dev\(const DipPosteriorRecDesc\* d, void\* stream\);", hdr, flags=re.M)
    assert re.search(r"^int dip_posterior_pool\(const float\* mean0, const float\* m20, long long stride, const int\* chains, "
                     r"int nchains, int k, int64_t n,$", hdr, flags=re.M)
    assert "typedef struct DipPosteriorRecDesc {" in hdr and "sizeof(DipPosteriorRecDesc) == 88" in hdr
    for name, nargs in (("dip_posterior_rec_dev", 2), ("dip_posterior_pool", 14)):
        assert name in N.EXPORTS and hasattr(built, name) and len(N._SIGS[name][1]) == nargs
        fid = built.dip_list_fn_id(name.encode())
        assert fid >= 0 and built.dip_list_fn_nargs(fid) == nargs, name
    assert ctypes.sizeof(N.DipPosteriorRecDesc) == 88 and ctypes.sizeof(N.DipPosteriorDesc) == 56
    names = [f for f, _ in N.DipPosteriorRecDesc._fields_]
    assert names[:8] == [f for f, _ in N.DipPosteriorDesc._fields_] and names[8:] == ["gt", "partial", "records", "capacity",
                                                                                      "reserved"]
    assert built.dip_abi_version() == N.ABI_VERSION == 9            # additions do not bump it


def test_posterior_rec_dev_refuses_before_it_launches(built):
    import dip_native as N
    L = built
    assert L.dip_posterior_rec_dev(None, None) == -1 and b"posterior_rec_dev" in L.dip_last_error()
    good = lambda: N.DipPosteriorRecDesc(P, P, P, P, P, 8, 0, 1, P, P, P, 4, 0)
    for field in ("out", "mean", "m2", "count", "counter", "gt", "partial", "records"):
        bad = good()
        setattr(bad, field, None)
        assert L.dip_posterior_rec_dev(ctypes.byref(bad), None) == -1 and b"NULL" in L.dip_last_error(), field
    for field, v in (("n", 0), ("n", -5), ("burn_in", -1), ("every", 0), ("capacity", 0)):
        bad = good()
        setattr(bad, field, v)
        assert L.dip_posterior_rec_dev(ctypes.byref(bad), None) == -1 and b"posterior_rec_dev" in L.dip_last_error(), field


def test_posterior_pool_refuses_before_it_launches(built):
    L = built
    ok = dict(mean0=P, m20=P, stride=4096, chains=P, nchains=3, k=5, n=64, mean=P, var=P, within=P, rhat=P, partial=P,
              summary=P, stream=None)
    call = lambda **kw: L.dip_posterior_pool(*dict(ok, **kw).values())
    for name in ("mean0", "m20", "chains", "mean", "var", "within", "partial", "summary"):
        assert call(**{name: None}) == -1 and b"posterior_pool" in L.dip_last_error() and b"NULL" in L.dip_last_error(), name
    for kw, msg in ((dict(n=0), b"n must be"), (dict(n=-1), b"n must be"), (dict(k=1), b"k (samples per chain)"),
                    (dict(k=0), b"k (samples per chain)"), (dict(nchains=1), b"at least 2 chains"),
                    (dict(nchains=0), b"at least 2 chains"), (dict(stride=4098), b"4-byte aligned"),
                    (dict(mean0=P + 2), b"4-byte aligned")):
        assert call(**kw) == -1 and msg in L.dip_last_error(), kw
    # one launch outside the bracket: refused while a group is open
    assert L.dip_group_begin(2, 1 << 16, P, 1 << 16) == 0
    try:
        assert call() == -1 and b"bracket is open" in L.dip_last_error()
    finally:
        L.dip_group_end()
    assert L.dip_group_size() == 1


# ------------------------------------------------------------------------------------------ construction
def test_monitors_validate_their_settings():
    from utils.fit_monitor import (POSTERIOR_BUFFERS, POSTERIOR_REC_BUFFERS, GroupedPosteriorMonitor, PosteriorMonitor,
                                   _GroupedRecords, _PosteriorKind)
    img = torch.zeros(1, 3, 8, 8)
    for kw, msg in ((dict(burn_in=-1), "burn_in must be >= 0"), (dict(burn_in=0, every=0), "every must be >= 1"),
                    (dict(burn_in=0, imgs_gt=[img], capacity=0), "capacity"), (dict(burn_in=0, imgs_gt=[]), "one ground truth"),
                    (dict(burn_in=0, imgs_gt=[img, None]), "one ground truth"),
                    (dict(burn_in=0, imgs_gt=[img, torch.zeros(1, 3, 8, 9)]), r"imgs_gt\[1\] is \(1, 3, 8, 9\)"),
                    (dict(burn_in=0, imgs_gt=[torch.zeros(3, 8, 8)]), r"must be \[1,C,H,W\]")):
        with pytest.raises(ValueError, match="dip-amd: GroupedPosteriorMonitor.*" + msg):
            GroupedPosteriorMonitor(**kw)
    m = GroupedPosteriorMonitor(3, 2)
    assert isinstance(m, (_PosteriorKind, _GroupedRecords)) and (m.burn_in, m.every, m.i, m.count) == (3, 2, 0, 0)
    assert m.mean is None and m.m2 is None and m.samples is None and m.counter is None and m.group is None
    assert m.BUFFERS is POSTERIOR_BUFFERS and m.COLUMNS == () and not m.with_gt
    for call in (m.variance, m.pooled, m.history):
        with pytest.raises(RuntimeError, match="dip-amd: GroupedPosteriorMonitor.*has not been given to a GroupedFits"):
            call()
    r = GroupedPosteriorMonitor(3, 2, imgs_gt=[img, img], capacity=7)
    assert r.BUFFERS is POSTERIOR_REC_BUFFERS and r.COLUMNS == ("iteration", "mse_mean", "psnr_mean") and r.capacity == 7
    assert [b.name for b in POSTERIOR_REC_BUFFERS] == ["mean", "m2", "samples", "counter", "gt", "partial", "records"]
    # the host's sample count, and what does not fit: the cap of 2**24 samples, the record rows
    m.i = 10
    assert m.count == 4 == len([i for i in range(10) if i >= 3 and (i - 3) % 2 == 0])
    f = GroupedPosteriorMonitor(0, 1)
    f.i = 2 ** 24 - 1
    f._check_room(1)
    with pytest.raises(RuntimeError, match=r"dip-amd: GroupedPosteriorMonitor.*2\*\*24 samples"):
        f._check_room(2)
    r.i = 3
    r._check_room(13)                                               # samples at 3, 5, ..., 15: seven
    with pytest.raises(RuntimeError, match="dip-amd: GroupedPosteriorMonitor capacity exceeded"):
        r._check_room(15)
    # the solo monitor's new keywords, before anything that needs a GPU
    with pytest.raises(ValueError, match="dip-amd: PosteriorMonitor: img_gt must be a tensor shaped like img_like"):
        PosteriorMonitor(img, 0, img_gt=torch.zeros(1, 3, 8, 9))
    with pytest.raises(ValueError, match="dip-amd: PosteriorMonitor: capacity"):
        PosteriorMonitor(img, 0, img_gt=img, capacity=0)
    with pytest.raises(RuntimeError, match="dip-amd: PosteriorMonitor works on MI355X tensors only"):
        PosteriorMonitor(img, 0, img_gt=img)


def test_grouped_fits_validate_posterior():
    from utils.fit_monitor import GroupedPosteriorMonitor, GroupedSSIMMonitor
    gen = torch.Generator().manual_seed(1)
    gts = [torch.rand(1, 3, 36, 52, generator=gen) for _ in range(3)]
    solo_like = type("PosteriorMonitor", (), {})()                  # (a solo monitor needs a GPU to exist; its type is what counts)
    for bad in (solo_like, GroupedSSIMMonitor(gts), 3):
        with pytest.raises(TypeError, match="dip-amd: GroupedFits\\(posterior=\\) takes a utils.fit_monitor.GroupedPosteriorMonitor"):
            _dry_group(posterior=bad)
    with pytest.raises(ValueError, match="dip-amd: GroupedPosteriorMonitor has 2 imgs_gt for 3 instances"):
        _dry_group(posterior=GroupedPosteriorMonitor(0, imgs_gt=gts[:2]))
    with pytest.raises(ValueError, match=r"dip-amd: GroupedPosteriorMonitor: imgs_gt\[0\] is \(1, 3, 36, 50\), the net output is"):
        _dry_group(posterior=GroupedPosteriorMonitor(0, imgs_gt=[t[..., :50] for t in gts]))
    m = GroupedPosteriorMonitor(3, 2)
    g, _ = _dry_group(posterior=m)
    assert m.group is g and g.posterior is m
    with pytest.raises(RuntimeError, match="dip-amd: this GroupedPosteriorMonitor already belongs to a GroupedFits"):
        _dry_group(posterior=m)
    # the solo type's own refusal names the class
    from utils.fit_monitor import PosteriorMonitor
    with pytest.raises(TypeError, match="got PosteriorMonitor \\(a solo PosteriorMonitor owns its buffers"):
        _dry_group(posterior=PosteriorMonitor.__new__(PosteriorMonitor))


# ------------------------------------------------------------------------------------------ the slab
POST = ["post_mean", "post_m2", "post_samples", "post_counter"]


def _offsets(g):
    ex = g._row0_extra
    return {k: (None if t is None else g._off(t) - g._off(ex["saved"])) for k, t in ex.items()}


def _check_rows_behind(g, plain, n, names):
    """The post_ rows of g behind every other row, every other row where it lies in `plain`, views and pointers sound."""
    ex, off, off0 = g._row0_extra, _offsets(g), _offsets(plain)
    assert list(ex)[-len(names):] == names and list(ex)[:-len(names)] == list(plain._row0_extra)
    assert {k: v for k, v in off.items() if k not in names} == off0
    ends = [off[k] + ex[k].numel() * ex[k].element_size() for k in off0 if off0[k] is not None]
    assert off["post_mean"] >= max(ends) and [off[k] for k in names] == sorted(off[k] for k in names)
    assert g.stride > plain.stride and g.pointers_outside_row0() == []
    assert ex["post_mean"].numel() == ex["post_m2"].numel() == n
    assert ex["post_samples"].dtype == ex["post_counter"].dtype == torch.int32
    m, B = g.posterior, g.B
    assert tuple(m.mean.shape) == tuple(m.m2.shape) == (B, *g.out.shape[1:]) and tuple(m.samples.shape) == tuple(m.counter.shape) == (B,)
    assert m.samples.dtype == m.counter.dtype == torch.int32
    for b in range(B):                                              # zero-initialised in every row, views over the rows
        for k in POST:
            assert not g._inst(ex[k], b).any(), (b, k)
        assert m.mean[b].data_ptr() == g._inst(ex["post_mean"], b).data_ptr()
        assert m.counter[b].data_ptr() == g._inst(ex["post_counter"], b).data_ptr()
    d = g._pdesc
    assert (d.out, d.mean, d.m2, d.count, d.counter) == tuple(ex[k].data_ptr() for k in ["out"] + POST)
    assert (d.n, d.burn_in, d.every) == (n, 3, 2)


@pytest.mark.parametrize("case", ["a_mse", "f_sr_tv", "m_mse_mask_restore_early_stop_emv"])
def test_post_rows_lie_behind_the_recorded_tails(built, monkeypatch, case):
    import json
    import dip_group
    import dip_native as N
    import test_group_tail_layout_host as T
    from utils.fit_monitor import GroupedPosteriorMonitor
    plain = T._group(case)
    with open(T.GOLDEN) as fh:                                      # without the keyword: the recorded layout and launch lists
        assert json.loads(json.dumps(T._fingerprint(plain))) == json.load(fh)[case]
    assert plain.posterior is None and not hasattr(plain, "_pdesc") and not hasattr(plain, "_post")
    assert [s[0] for s in dip_group.GroupedFits._SLOTS] == ["monitor", "early_stop", "posterior", "ssim"]

    class WithPosterior(dip_group.GroupedFits):
        def __init__(self, *a, **kw):
            super().__init__(*a, posterior=GroupedPosteriorMonitor(3, 2), **kw)

    monkeypatch.setattr(dip_group, "GroupedFits", WithPosterior)
    g = T._group(case)
    monkeypatch.undo()
    n = 3 * T.HW[0] * T.HW[1]                                       # (the sample is the HR output in a super-resolution group)
    _check_rows_behind(g, plain, n, POST)
    assert isinstance(g._pdesc, N.DipPosteriorDesc) and [name for _, _, name in g._post] == ["posterior_dev"]
    fp, fp0 = T._fingerprint(g), T._fingerprint(plain)
    for k in ("head_fwd", "head_bwd", "mon", "es", "head", "mdesc", "edesc", "values", "with_out_conv"):
        assert fp[k] == fp0[k], (case, k)
    order = [prefix for _, prefix, _, _ in g._monitors()]
    assert order == [p for p in ("mon_", "es_", "post_", "ssim_") if p in order] and "post_" in order


def test_post_rows_lie_behind_the_sweep_and_sgld_rows(built):
    from utils.fit_monitor import GroupedPosteriorMonitor
    import dip_native as N
    kw = dict(lr=[0.01, 0.02, 0.03], reg_noise_std=[1 / 30., 1 / 20., 0.03], weight_decay=5e-8, param_noise_std=0.01)
    plain, _ = _dry_group(**{k: v for k, v in kw.items() if k != "reg_noise_std"})
    g, _ = _dry_group(posterior=GroupedPosteriorMonitor(3, 2), **{k: v for k, v in kw.items() if k != "reg_noise_std"})
    assert list(plain._row0_extra)[-3:] == ["sgld", "sgld_ranges", "lr"]
    _check_rows_behind(g, plain, 3 * 36 * 52, POST)
    # with ground truths: three more rows behind the four, the images in their own instances' rows
    gen = torch.Generator().manual_seed(2)
    gts = [torch.rand(1, 3, 36, 52, generator=gen) for _ in range(3)]
    r, _ = _dry_group(posterior=GroupedPosteriorMonitor(3, 2, imgs_gt=gts, capacity=5), lr=kw["lr"])
    plain_lr, _ = _dry_group(lr=kw["lr"])
    names = POST + ["post_gt", "post_partial", "post_records"]
    _check_rows_behind(r, plain_lr, 3 * 36 * 52, names)
    ex, d, m = r._row0_extra, r._pdesc, r.posterior
    assert isinstance(d, N.DipPosteriorRecDesc) and [name for _, _, name in r._post] == ["posterior_rec_dev"]
    assert (d.gt, d.partial, d.records, d.capacity) == (ex["post_gt"].data_ptr(), ex["post_partial"].data_ptr(),
                                                        ex["post_records"].data_ptr(), 5)
    assert ex["post_partial"].dtype == torch.float64 and ex["post_partial"].numel() == built.dip_fit_monitor_nblk(3 * 36 * 52)
    assert ex["post_partial"].data_ptr() % 8 == 0 and tuple(m.records.shape) == (3, 5, 3) and not m.records.any()
    for b in range(3):
        assert torch.equal(r._inst(ex["post_gt"], b).view(1, 3, 36, 52), gts[b])
    assert m.history().shape == (3, 0, 3)
    with pytest.raises(RuntimeError, match="dip-amd: GroupedPosteriorMonitor.last\\(\\): no sample"):
        m.last()
    with pytest.raises(RuntimeError, match="dip-amd: GroupedPosteriorMonitor keeps no record table without imgs_gt="):
        g.posterior.history()
    # the group refuses what a monitor refuses, before anything is issued (a dry group cannot launch: room is checked first)
    m.i = r.iterations = 3
    with pytest.raises(RuntimeError, match="dip-amd: GroupedPosteriorMonitor capacity exceeded"):
        r.run(11)
    with pytest.raises(RuntimeError, match="dip-amd: GroupedPosteriorMonitor capacity exceeded"):
        r.step(11)


# ------------------------------------------------------------------------------------------ the yardstick of the pooled arithmetic
@pytest.mark.parametrize("C,k,n", [(2, 2, 1000), (3, 7, 5000), (5, 40, 20000), (8, 300, 20000), (16, 3, 20000)])
def test_float32_restatement_against_the_textbook_formula(C, k, n):
    """The cap: relative error of var at most 1e-5.  The restatement reaches 3.2e-6 against the raw-sample fp64 formula (rounding
    the inputs to fp32 dominates) and 2.5e-7 against fp64 from the same fp32 inputs; the cap is about three times the former."""
    x = R.synthetic(np.random.default_rng(5), C, k, n)
    mean64, m264 = R.chain_rows(x)
    mean32, m232 = mean64.astype(np.float32), m264.astype(np.float32)
    mu, V, W, Rh, summary = R.pool(mean32, m232, k)
    mu_t, V_t, W_t, R_t = R.textbook(x)
    rel = lambda a, b: float(np.max(np.abs(a.astype(np.float64) - b) / np.abs(b)))
    # (fp64 from the same fp32 inputs: the operations' own error)
    m, s = mean32.astype(np.float64), m232.astype(np.float64)
    W_s = s.sum(axis=0) / (C * (k - 1))
    V_s = (k - 1) / k * W_s + m.var(axis=0, ddof=1)
    print(f"C {C} k {k} n {n}: var rel err {rel(V, V_t):.2e} (same inputs {rel(V, V_s):.2e}), within {rel(W, W_t):.2e}, "
          f"mean {rel(mu, mu_t):.2e}, rhat {rel(Rh, R_t):.2e}")
    assert rel(V, V_t) <= 1e-5
    assert rel(W, W_t) <= 1e-5 and rel(mu, mu_t) <= 1e-6 and rel(Rh, R_t) <= 1e-5
    assert summary[2] == 0 and abs(summary[0] - R_t.mean()) <= 1e-5 * R_t.mean() and summary[1] == Rh.max()


def test_restatement_order_and_degenerate_elements():
    rng = np.random.default_rng(7)
    mean = rng.uniform(0.1, 0.9, (4, 257)).astype(np.float32)
    m2 = rng.uniform(0.01, 0.1, (4, 257)).astype(np.float32)
    m2[:, 5] = 0                                                    # no within-chain variance, different means: R = NaN
    m2[:, 9] = 0
    mean[:, 9] = 0.5                                                # ... and equal means: 0 / 0
    a, b = R.pool(mean, m2, 7, [2, 0, 1]), R.pool(mean, m2, 7, [0, 1, 2])
    assert any(not np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a[:4], b[:4]))      # the order shows
    assert np.isnan(a[3][[5, 9]]).all() and np.isnan(a[3]).sum() == 2 and a[4][2] == 2
    assert a[1][5] > 0 and a[1][9] == 0 and a[2][5] == 0
    good = ~np.isnan(a[3])
    assert a[4][1] == a[3][good].max() and abs(a[4][0] - a[3][good].astype(np.float64).mean()) < 1e-12
    none = R.pool(mean, np.zeros_like(m2), 7)
    assert np.isnan(none[4][:2]).all() and none[4][2] == 257
