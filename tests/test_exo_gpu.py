"""GPU tests (``-m gpu``) of ``sup3r_amd.exo``: ``s3_exo_nearest`` and
``s3_exo_group_mean`` through the C ABI into sentinel-filled buffers with red
zones, then ``ExoRasterizer``, ``ExoDataHandler`` and ``ArrayStrategy(
exo_handler_kwargs=...)`` end to end.

Nearest ids are compared with scipy's ``KDTree.query`` on inputs for which
the test first asserts, in float64 on the host, that no source has its
second-nearest ``d2`` within a relative 2^-50 of its nearest and that no
``d2`` lies within a relative 2^-50 of ``r r`` (``exo_ref.nearest_margins``
checks a relative 1e-9 of ``r``, which is stronger).  Sources are random
float32 points, over the targets' box and beyond it on every side; a float32
point over an axis-aligned float32 grid lies EXACTLY between two rows or
columns about once in 10^5 draws, so ``exo_ref.untie`` moves such a point by
one float32 step before the conditions are asserted — no case is dropped.
Planted ties and points at exactly ``r`` are compared with the brute-force
restatement instead.

Group means: bit-equal to ``exo_ref.exact_group_mean`` where every summation
order is exact (values ``k / 64``, ``|k| <= 2^15``); for general values
``|out - exact| <= 2^-24 |exact| + n 2^-52 A + q`` with ``A = sum |x| / n`` and
``q = 2^(E - 62)``, ``E = floor(log2(max |x|))``, the documented bound of the
fixed-point accumulation; against the pandas route ``2^-23 A + 2^-24 |mean|``
more."""
import ctypes as C
import logging
import os
import sys
import warnings

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import exo_ref  # noqa: E402
from test_exo_cpu import (TIMES, lr_grid, source_raster,  # noqa: E402
                          two_step_topo)

pytestmark = pytest.mark.gpu

CFG = os.path.join(os.path.dirname(__file__), '..', 'sup3r_amd', 'configs')
EINVAL = -1
PAD = 64                       # sentinel words in front of and behind a buffer
SENTINEL = 0x5A5AC3C3
NANS = np.array([0x7FC00000, 0x7FC00001, 0x7F800001, 0xFFC12345],
                dtype=np.uint32)             # quiet, payload, signalling, negative


def padded(words, device):
    import torch
    return torch.full((PAD + int(words) + PAD,), SENTINEL, dtype=torch.int32,
                      device=device)


def zones_intact(buf, words):
    host = buf.cpu().numpy().view(np.uint32)
    return bool((host[:PAD] == SENTINEL).all()
                and (host[PAD + int(words):] == SENTINEL).all())


def payload(buf, words):
    return buf.cpu().numpy().view(np.uint32)[PAD:PAD + int(words)].copy()


def inner(buf):
    return C.c_void_p(buf.data_ptr() + 4 * PAD)


def device():
    from sup3r_amd import _lib
    from sup3r_amd.engine import Device
    return Device.get(), _lib.lib()


def upload(arr):
    import torch
    dev, _ = device()
    return torch.from_numpy(np.ascontiguousarray(arr)).to(dev.torch_device)


# ------------------------------------------------------------------ nearest
def run_nearest(src, tgt, r, want_dist=True, work_words=None):
    """``s3_exo_nearest`` -> (rc, nn int32 (n,), dist float64 (n,) or None);
    asserts that nothing around nn, dist and the workspace was written"""
    dev, L = device()
    src = np.ascontiguousarray(src, np.float32)
    tgt = np.ascontiguousarray(tgt, np.float32)
    n, m = len(src), len(tgt)
    n_bytes = int(L.s3_exo_nearest_work_bytes(m))
    assert n_bytes > 0 and n_bytes % 8 == 0
    words = n_bytes // 4 if work_words is None else work_words
    work = padded(words, dev.torch_device)
    nn = padded(n, dev.torch_device)
    dist = padded(2 * n, dev.torch_device)
    assert (work.data_ptr() + 4 * PAD) % 8 == 0
    assert (dist.data_ptr() + 4 * PAD) % 8 == 0
    s, t = upload(src), upload(tgt)
    rc = L.s3_exo_nearest(dev.ctx, C.c_void_p(s.data_ptr()), n,
                          C.c_void_p(t.data_ptr()), m, float(r), inner(work),
                          4 * words, inner(nn),
                          inner(dist) if want_dist else None)
    dev.sync()
    assert zones_intact(work, words) and zones_intact(nn, n)
    assert zones_intact(dist, 2 * n)
    d = payload(dist, 2 * n).view(np.float64)
    if not want_dist:
        assert (payload(dist, 2 * n) == SENTINEL).all()
    return rc, payload(nn, n).view(np.int32), d if want_dist else None


def make_grid(h, w, form='plain', spacing=0.37):
    """(h w, 2) float32 targets and their spacing: 'plain' axis-aligned,
    'rotated' by 0.6 rad, 'sheared' (the columns lean by 0.7 of a step per
    row)"""
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    y, x = spacing * i.astype(np.float64), spacing * j.astype(np.float64)
    if form == 'rotated':
        c, s = np.cos(0.6), np.sin(0.6)
        y, x = c * y + s * x, -s * y + c * x
    elif form == 'sheared':
        x = x + 0.7 * y
    tgt = np.stack([40.013 - y, -105.021 + x], axis=-1).reshape(-1, 2)
    return tgt.astype(np.float32), spacing


def random_sources(n, tgt, margin, seed):
    """float32 points over the targets' box widened by ``margin`` on every
    side, no one exactly between its two nearest targets; from 8 points on,
    the first four lie beyond the box, one on each side"""
    rng = np.random.default_rng(seed)
    lo, hi = tgt.min(axis=0) - margin, tgt.max(axis=0) + margin
    src = rng.uniform(lo, hi, size=(n, 2))
    if n >= 8:               # one beyond the box on each side, whatever the draw
        mid, out = (lo + hi) / 2, 0.6 * margin
        src[:4] = [[lo[0] + out / 3, mid[1]], [hi[0] - out / 3, mid[1]],
                   [mid[0], lo[1] + out / 3], [mid[0], hi[1] - out / 3]]
    return exo_ref.untie(src.astype(np.float32), tgt)


def check_against_scipy(src, tgt, r):
    gap, clear = exo_ref.nearest_margins(src, tgt, r)
    assert gap > 2.0 ** -50 and clear, (gap, clear)
    dists, nn = exo_ref.query_tree(tgt.astype(np.float64),
                                   src.astype(np.float64), r)
    rc, got, d = run_nearest(src, tgt, r)
    assert rc == 0
    assert np.array_equal(got, nn)
    miss = nn == len(tgt)
    assert np.array_equal(np.isinf(d), miss) and (d[miss] > 0).all()
    assert (np.abs(d[~miss] - dists[~miss]) <= np.spacing(dists[~miss])).all()
    rc, again, none = run_nearest(src, tgt, r, want_dist=False)
    assert rc == 0 and none is None and np.array_equal(again, got)
    return nn


def n_over_the_grid_cap():
    """one source more than a full grid of the query kernel covers in one
    step: 8 workgroups of 256 per CU"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus * 8 * 256 + 1


@pytest.mark.parametrize('shape', [(2, 2), (3, 5), (37, 41)])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 'cap+1'])
def test_nearest_is_scipys_query(shape, n):
    tgt, spacing = make_grid(*shape)
    n = n_over_the_grid_cap() if n == 'cap+1' else n
    src = random_sources(n, tgt, 1.5 * spacing, seed=n % 1000 + shape[1])
    nn = check_against_scipy(src, tgt, spacing)
    if n >= 63:           # hits and misses; sources beyond the box on every side
        assert (nn < len(tgt)).any() and (nn == len(tgt)).any()
        assert (src < tgt.min(axis=0)).any(axis=0).all()
        assert (src > tgt.max(axis=0)).any(axis=0).all()


@pytest.mark.parametrize('form', ['rotated', 'sheared'])
def test_nearest_on_curvilinear_grids_reaches_diagonal_cells(form):
    tgt, spacing = make_grid(9, 11, form)
    src = random_sources(3000, tgt, 1.2 * spacing, seed=7)
    r = spacing
    nn = check_against_scipy(src, tgt, r)
    hit = nn < len(tgt)
    # cells of side r over the box, as the kernel lays them: some nearest
    # target lies one cell off in BOTH directions
    lo = tgt.min(axis=0).astype(np.float64)
    cs = np.floor((src[hit].astype(np.float64) - lo) / r)
    ct = np.floor((tgt[nn[hit]].astype(np.float64) - lo) / r)
    assert ((cs != ct).all(axis=1)).any()


def test_nearest_with_many_targets_per_cell_and_with_the_cell_cap():
    tgt, spacing = make_grid(37, 41)
    src = random_sources(4097, tgt, 5 * spacing, seed=11)
    check_against_scipy(src, tgt, 4 * spacing)
    # r = spacing / 1000: box / r is 4 * 10^4 cells a side, far above the cap;
    # the side grows, nearly everything misses; a few sources sit next to a
    # target
    r = spacing / 1000
    rng = np.random.default_rng(12)
    near = tgt[rng.integers(0, len(tgt), 40)] + rng.uniform(
        -0.4 * r, 0.4 * r, (40, 2)).astype(np.float32)
    src2 = exo_ref.untie(np.concatenate([src[:2000], near.astype(np.float32)]),
                         tgt)
    nn = check_against_scipy(src2, tgt, r)
    assert 10 <= (nn < len(tgt)).sum() <= 60
    # every source missed
    far = exo_ref.untie(src[:500] + np.float32(50), tgt)
    nn = check_against_scipy(far, tgt, spacing)
    assert (nn == len(tgt)).all()


def test_planted_ties_and_points_at_exactly_r():
    i, j = np.meshgrid(np.arange(3), np.arange(5), indexing='ij')
    tgt = np.stack([i, j], axis=-1).reshape(-1, 2).astype(np.float32)
    centres = np.stack(np.meshgrid(np.arange(2) + 0.5, np.arange(4) + 0.5,
                                   indexing='ij'), -1).reshape(-1, 2)
    edges = np.concatenate([
        np.stack(np.meshgrid(np.arange(3), np.arange(4) + 0.5,
                             indexing='ij'), -1).reshape(-1, 2),
        np.stack(np.meshgrid(np.arange(2) + 0.5, np.arange(5),
                             indexing='ij'), -1).reshape(-1, 2)])
    outside = np.array([[-0.5, 2.0], [2.5, 4.5], [1.0, -0.5], [1.0, 4.5]])
    src = np.concatenate([centres, edges, outside, tgt]).astype(np.float32)
    for r in (0.75, 1.0, 0.5, float(np.sqrt(0.5))):
        want, want_d = exo_ref.brute_nearest(src, tgt, r)
        rc, got, d = run_nearest(src, tgt, r)
        assert rc == 0 and np.array_equal(got, want), r
        assert np.array_equal(d, want_d), r
    # r = 0.5: an edge midpoint has d2 == r r in float64 and misses; a centre
    # of four targets under r = 0.75 goes to the smallest id of the four
    want, _ = exo_ref.brute_nearest(src, tgt, 0.5)
    assert (want[len(centres):len(centres) + len(edges)] == len(tgt)).all()
    want, _ = exo_ref.brute_nearest(src, tgt, 0.75)
    assert want[0] == 0 and want[1] == 1 and want[4] == 5


# --------------------------------------------------------------- group mean
def run_group_mean(nn, vals, m, t_out, cols, scale=1.0, work_words=None,
                   prefill=None):
    """``s3_exo_group_mean`` -> (rc, out uint32 (m, t_out), NaN count);
    asserts the red zones of out, the workspace and the count word"""
    dev, L = device()
    nn = np.ascontiguousarray(nn, np.int32)
    vals = np.ascontiguousarray(vals, np.float32)
    n, t_used = vals.shape
    n_bytes = int(L.s3_exo_group_mean_work_bytes(m, t_used))
    assert n_bytes > 0 and n_bytes % 8 == 0
    words = n_bytes // 4 if work_words is None else work_words
    work = padded(words, dev.torch_device)
    out = padded(m * t_out, dev.torch_device)
    count = padded(2, dev.torch_device)
    assert (count.data_ptr() + 4 * PAD) % 8 == 0
    col = np.ascontiguousarray(cols, np.int32)
    ids, x = upload(nn), upload(vals)
    rc = L.s3_exo_group_mean(
        dev.ctx, C.c_void_p(ids.data_ptr()), C.c_void_p(x.data_ptr()), n, m,
        t_used, t_out,
        col.ctypes.data_as(C.POINTER(C.c_int32)), float(scale), inner(work),
        4 * words, inner(out), inner(count))
    dev.sync()
    assert zones_intact(work, words) and zones_intact(out, m * t_out)
    assert zones_intact(count, 2)
    return (rc, payload(out, m * t_out).reshape(m, t_out),
            int(payload(count, 2).view(np.uint64)[0]))


def exact_lists(t, seed, shuffle):
    """8 targets with lists of 1, 2, 64, 65, 0, 3 (all NaN), 10 (NaNs of
    several payloads among them) and 5 values ``k / 64``; misses sprinkled"""
    rng = np.random.default_rng(seed)
    lengths = [1, 2, 64, 65, 0, 3, 10, 5]
    nn = np.concatenate([np.full(n, i) for i, n in enumerate(lengths)]
                        + [np.full(7, 8)])
    k = rng.integers(-2 ** 15, 2 ** 15 + 1, size=(len(nn), t))
    vals = (k / 64).astype(np.float32)
    bits = vals.view(np.uint32)
    bits[nn == 5] = NANS[rng.integers(0, 4, size=(3, t))]
    six = np.flatnonzero(nn == 6)
    bits[six[:4]] = NANS[:, None]
    if shuffle:
        order = rng.permutation(len(nn))
        nn, vals = nn[order], vals[order]
    return nn, vals


@pytest.mark.parametrize('t', [1, 3])
@pytest.mark.parametrize('scale', [1.0, 0.5])
@pytest.mark.parametrize('shuffle', [False, True])
def test_group_mean_is_exact_where_the_sums_are(t, scale, shuffle):
    nn, vals = exact_lists(t, seed=3 * t + shuffle, shuffle=shuffle)
    t_out = 2 * t - 1                   # t = 3: columns 1 and 3 stay untouched
    cols = [0] if t == 1 else [4, 0, 2]
    want, n, _ = exo_ref.exact_group_mean(nn, vals, 8, t_out, cols, scale)
    rc, got, n_nan = run_group_mean(nn, vals, 8, t_out, cols, scale)
    assert rc == 0
    assert np.array_equal(got[:, cols], want[:, cols].view(np.uint32))
    assert np.isnan(want[4, cols]).all() and np.isnan(want[5, cols]).all()
    assert not np.isnan(want[[0, 1, 2, 3, 6, 7]][:, cols]).any()
    assert n[6, 0] == 6
    untouched = [c for c in range(t_out) if c not in cols]
    assert (got[:, untouched] == SENTINEL).all()
    assert n_nan == 2 * t
    rc, again, n_again = run_group_mean(nn, vals, 8, t_out, cols, scale)
    assert rc == 0 and np.array_equal(again, got) and n_again == n_nan


def test_group_mean_of_one_long_list():
    rng = np.random.default_rng(21)
    nn = np.concatenate([np.full(100000, 2), np.full(9, 0), np.full(5, 4)])
    vals = (rng.integers(-2 ** 15, 2 ** 15 + 1, size=(len(nn), 1)) / 64
            ).astype(np.float32)
    order = rng.permutation(len(nn))
    for idx in (np.arange(len(nn)), order):
        want, n, _ = exo_ref.exact_group_mean(nn[idx], vals[idx], 4, 1, [0])
        rc, got, n_nan = run_group_mean(nn[idx], vals[idx], 4, 1, [0])
        assert rc == 0 and n[2, 0] == 100000
        assert np.array_equal(got, want.view(np.uint32))
        assert n_nan == 2                       # targets 1 and 3


@pytest.mark.parametrize('kind', ['normal', 'topography'])
def test_group_mean_of_general_values_within_the_bound(kind):
    rng = np.random.default_rng(31)
    m, n_src, t = 12 * 13, 20000, 2
    nn = rng.integers(0, m + 20, size=n_src).clip(max=m)    # ~11 % misses
    nn[rng.integers(0, n_src, 3000)] = 5                     # one long list
    vals = (rng.standard_normal((n_src, t)) if kind == 'normal'
            else rng.uniform(0, 4000, (n_src, t))).astype(np.float32)
    vals[rng.integers(0, n_src, 200), 0] = np.nan
    exact, n, mean_abs = exo_ref.exact_group_mean(nn, vals, m, t, [0, 1])
    rc, got, _ = run_group_mean(nn, vals, m, t, [0, 1])
    assert rc == 0
    got = got.view(np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(exact))
    top = float(np.nanmax(np.abs(vals)))
    q = 2.0 ** (np.floor(np.log2(top)) - 62)
    assert q <= 2.0 ** -60 * top
    ok = ~np.isnan(exact)
    e64 = exact.astype(np.float64)
    lim = 2.0 ** -24 * np.abs(e64) + n * 2.0 ** -52 * mean_abs + q
    err = np.abs(got.astype(np.float64) - e64)
    print(f'{kind}: worst error / bound against the exact mean '
          f'{(err[ok] / lim[ok]).max():.3f}')
    assert (err[ok] <= lim[ok]).all()
    # the pandas route of the reference, column by column
    for k in range(t):
        ref = exo_ref.get_data_2d('x', vals[:, k:k + 1], nn, (m, 1, 1))
        ref = ref.reshape(-1).astype(np.float64)
        okk = ok[:, k]
        assert np.array_equal(np.isnan(ref), ~okk)
        lim_p = lim[:, k] + 2.0 ** -23 * mean_abs[:, k] + 2.0 ** -24 * np.abs(
            ref)
        err_p = np.abs(got[:, k].astype(np.float64) - ref)
        print(f'{kind}[{k}]: worst error / bound against pandas '
              f'{(err_p[okk] / lim_p[okk]).max():.3f}')
        assert (err_p[okk] <= lim_p[okk]).all()


def test_group_mean_in_slabs():
    """more columns than one slab of the workspace holds"""
    from sup3r_amd import _lib
    rng = np.random.default_rng(41)
    t = _lib.EXO_MAX_SLAB + 5
    nn = rng.integers(0, 7, size=300)                        # 6: a miss
    vals = (rng.integers(-2 ** 15, 2 ** 15 + 1, size=(300, t)) / 64).astype(
        np.float32)
    cols = list(rng.permutation(t + 2)[:t])
    want, _, _ = exo_ref.exact_group_mean(nn, vals, 6, t + 2, cols)
    rc, got, n_nan = run_group_mean(nn, vals, 6, t + 2, cols)
    assert rc == 0 and n_nan == 0
    assert np.array_equal(got[:, cols], want[:, cols].view(np.uint32))
    rest = [c for c in range(t + 2) if c not in cols]
    assert (got[:, rest] == SENTINEL).all()


def test_what_the_entry_points_refuse():
    from sup3r_amd import _lib
    dev, L = device()
    tgt, spacing = make_grid(3, 5)
    src = random_sources(10, tgt, spacing, seed=1)
    for r in (0.0, -1.0, float('inf'), float('nan')):
        rc, nn, d = run_nearest(src, tgt, r)
        assert rc == EINVAL and 'r must be' in _lib.last_error(dev.ctx)
        assert (nn.view(np.uint32) == SENTINEL).all()
    full = int(L.s3_exo_nearest_work_bytes(len(tgt))) // 4
    rc, nn, _ = run_nearest(src, tgt, spacing, work_words=full - 2)
    assert rc == EINVAL and 'work is smaller' in _lib.last_error(dev.ctx)
    assert (nn.view(np.uint32) == SENTINEL).all()
    s, t = upload(src), upload(tgt)
    buf = padded(full, dev.torch_device)

    def nearest(n, m):
        return L.s3_exo_nearest(dev.ctx, C.c_void_p(s.data_ptr()), n,
                                C.c_void_p(t.data_ptr()), m, spacing,
                                inner(buf), 4 * full, inner(buf), None)
    assert nearest(0, 15) == EINVAL and nearest(10, 0) == EINVAL
    assert nearest(-1, 15) == EINVAL and nearest(2 ** 31, 15) == EINVAL
    assert L.s3_exo_nearest_work_bytes(0) < 0
    assert L.s3_exo_group_mean_work_bytes(0, 1) < 0
    ids = np.zeros(10, np.int32)
    vals = np.ones((10, 2), np.float32)
    for cols in ([0, 3], [-1, 0]):
        rc, out, _ = run_group_mean(ids, vals, 4, 3, cols)
        assert rc == EINVAL and 'column map' in _lib.last_error(dev.ctx)
        assert (out == SENTINEL).all()
    rc, out, _ = run_group_mean(ids, vals, 4, 1, [0, 0])     # t_used > t_out
    assert rc == EINVAL and (out == SENTINEL).all()
    full = int(L.s3_exo_group_mean_work_bytes(4, 2)) // 4
    rc, out, _ = run_group_mean(ids, vals, 4, 2, [0, 1], work_words=full - 2)
    assert rc == EINVAL and 'work is smaller' in _lib.last_error(dev.ctx)
    assert (out == SENTINEL).all()
    dev.sync()
    assert (buf.cpu().numpy().view(np.uint32) == SENTINEL).all()


# --------------------------------------------------------------- end to end
def pair_bound(exact, n, mean_abs, top):
    """|device - numpy backend|: each against the exact mean"""
    q = 2.0 ** (np.floor(np.log2(top)) - 62)
    return 2.0 ** -23 * np.abs(exact) + n * 2.0 ** -51 * mean_abs + q


def test_rasterizer_2d_fills_holes_as_nn_fill_array():
    from sup3r_amd import exo
    lr = lr_grid()
    ll, vals = source_raster(
        lr, factor=5, jitter=0.01,
        holes=lambda p: (p[..., 0] > 39.2) & (p[..., 1] < -104))
    tgt = exo_ref.get_lat_lon(lr.astype(np.float32), (12, 14))
    ll = exo_ref.untie(ll.reshape(-1, 2), tgt.reshape(-1, 2)).reshape(ll.shape)
    kw = dict(source_files=exo.ExoSource(ll, topography=vals), s_enhance=2)
    raw = exo.ExoRasterizer('topography', exo.ExoInput(lr, TIMES),
                            fill_nans=False, **kw)
    assert raw.backend.name == 'device'
    unfilled = raw.data
    assert unfilled.values.is_cuda and unfilled.shape == (12, 14, 1)
    field = unfilled.numpy()
    holes = int(np.isnan(field).sum())
    assert 0 < holes < field.size
    # against the reference's route
    dists, nn = exo_ref.query_tree(raw.hr_lat_lon, ll.reshape(-1, 2),
                                   raw.get_distance_upper_bound())
    assert np.array_equal(raw.nn, nn)
    miss = nn == 12 * 14
    assert np.array_equal(np.isinf(raw.dists), miss)
    assert (np.abs(raw.dists[~miss] - dists[~miss])
            <= np.spacing(dists[~miss])).all()
    want = exo_ref.get_data_2d('topography', vals.reshape(-1, 1), nn,
                               raw.hr_shape)
    assert np.array_equal(np.isnan(field[..., 0]), np.isnan(want))
    exact, n, mean_abs = exo_ref.exact_group_mean(
        nn, vals.reshape(-1, 1), 12 * 14, 1, [0])
    ok = ~np.isnan(exact[:, 0])
    lim = (2.0 ** -24 * np.abs(exact[ok, 0]) + n[ok, 0] * 2.0 ** -52
           * mean_abs[ok, 0] + 2.0 ** -23 * mean_abs[ok, 0]
           + 2.0 ** -24 * np.abs(want.reshape(-1)[ok])
           + 2.0 ** (np.floor(np.log2(np.nanmax(np.abs(vals)))) - 62))
    assert (np.abs(field.reshape(-1)[ok].astype(np.float64)
                   - want.reshape(-1)[ok]) <= lim).all()
    filled = exo.ExoRasterizer('topography', exo.ExoInput(lr, TIMES), **kw)
    with pytest.warns(UserWarning, match=f'^{holes} target pixels did not '
                      'have unique high-resolution topography source data'):
        got = filled.data.numpy()
    assert np.array_equal(got.view(np.uint32),
                          exo_ref.nn_fill_array(field).view(np.uint32))


def test_rasterizer_3d_with_partial_time_overlap_and_obs(caplog):
    from sup3r_amd import exo
    lr = lr_grid(4, 5)
    src_times = pd.date_range('2020-01-01 02:00', periods=5, freq='h')
    ll, vals = source_raster(lr, factor=3, t=5, seed=3, jitter=0.01)
    vals[::7, ::5, 1] = np.nan
    ll = exo_ref.untie(ll.reshape(-1, 2), lr.reshape(-1, 2)).reshape(ll.shape)
    kw = dict(fill_nans=False, source_files=exo.ExoSource(
        ll, time_index=src_times, u_10m=vals))
    dev_r = exo.ExoRasterizer('u_10m', exo.ExoInput(lr, TIMES), **kw)
    host_r = exo.ExoRasterizer('u_10m', exo.ExoInput(lr, TIMES),
                               device=False, **kw)
    got, want = dev_r.data, host_r.data
    assert got.values.is_cuda and got.shape == want.shape == (4, 5, 4)
    assert got.as_array().shape == (4, 5, 4, 1)
    g, w = got.numpy(), want.numpy()
    assert np.isnan(g[..., :2]).all() and not np.isnan(g[..., 2:]).any()
    assert np.array_equal(np.isnan(g), np.isnan(w))
    assert np.array_equal(dev_r.nn, host_r.nn)
    exact, n, mean_abs = exo_ref.exact_group_mean(
        dev_r.nn, vals.reshape(-1, 5)[:, :2], 20, 4, [2, 3])
    lim = pair_bound(exact[:, 2:].astype(np.float64), n, mean_abs,
                     np.nanmax(np.abs(vals)))
    assert (np.abs(g.reshape(20, 4)[:, 2:].astype(np.float64)
                   - w.reshape(20, 4)[:, 2:]) <= lim).all()
    assert np.array_equal(g.reshape(20, 4)[:, 2:].view(np.uint32),
                          exact[:, 2:].view(np.uint32))
    # observations: NaN kept, nothing filled, the coverage message
    rng = np.random.default_rng(5)
    obs_ll = np.stack([rng.uniform(38.9, 40.1, 9),
                       rng.uniform(-105.1, -103.5, 9)], axis=1)
    obs = rng.standard_normal((9, 4)).astype(np.float32)
    okw = dict(s_enhance=2, source_files=exo.ExoSource(
        obs_ll, time_index=TIMES, u_10m=obs))
    o = exo.ExoRasterizer('u_10m_obs', exo.ExoInput(lr, TIMES), **okw)
    h = exo.ExoRasterizer('u_10m_obs', exo.ExoInput(lr, TIMES), device=False,
                          **okw)
    with warnings.catch_warnings(), caplog.at_level(logging.INFO,
                                                     'sup3r_amd.exo'):
        warnings.simplefilter('error')
        field = o.data.numpy()
    assert o.fill_nans is False
    hits = int((h.nn != 80).sum())
    assert 0 < hits <= 9
    cover = (~np.isnan(field)).sum() / field.size
    assert (f'Found {hits} of 9 observations within' in caplog.text
            and f'Observations cover {cover:.4e} of the high-res domain.'
            in caplog.text)
    assert np.isnan(field).any() and not np.isnan(field).all()
    assert np.array_equal(field, h.data.numpy(), equal_nan=True)


def test_handler_on_a_two_step_chain_equals_the_host_backend():
    from sup3r_amd import exo
    model = two_step_topo()
    lr = lr_grid()
    ll, vals = source_raster(lr, factor=24, jitter=0.003)
    src = exo.ExoSource(ll, topography=vals)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        hd = exo.ExoDataHandler('topography', exo.ExoInput(lr, TIMES),
                                model=model, source_files=src)
        hh = exo.ExoDataHandler('topography', exo.ExoInput(lr, TIMES),
                                model=model, source_files=src, device=False)
    assert hd.steps == hh.steps == [
        {'model': 0, 'combine_type': 'input', 's_enhance': 1, 't_enhance': 1},
        {'model': 0, 'combine_type': 'layer', 's_enhance': 2, 't_enhance': 1},
        {'model': 1, 'combine_type': 'input', 's_enhance': 2, 't_enhance': 1},
        {'model': 1, 'combine_type': 'layer', 's_enhance': 6, 't_enhance': 1}]
    sd, sh = (h.data['topography']['steps'] for h in (hd, hh))
    assert [s.shape for s in sd] == [(6, 7, 1), (12, 14, 1), (12, 14, 1),
                                     (36, 42, 1)]
    assert sd[1]['data'] is sd[2]['data']
    # one upload of the source for all steps
    assert sum(1 for k in hd._shared if k[1][0] in ('data', 'lat_lon')) == 2
    top = float(np.abs(vals).max())
    for a, b in zip(sd, sh):
        assert a['data'].is_cuda and a['data'].dtype.is_floating_point
        x, y = a['data'].cpu().numpy(), b['data']
        assert x.dtype == np.float32 and not np.isnan(x).any()
        # each against the exact mean: n 2^-51 A + q <= 2^-38 top for the
        # fewer than 2^12 sources a low-res pixel collects (24 * 24, and the
        # bound reaches a little past the pixel)
        lim = 2.0 ** -23 * np.abs(y) + 2.0 ** -38 * top
        assert (np.abs(x.astype(np.float64) - y) <= lim).all()


def test_forward_pass_over_rasterised_fields_equals_passed_fields():
    from sup3r_amd import ForwardPass, Sup3rGan, exo
    from sup3r_amd.forward_pass import register_model
    from sup3r_amd.strategy import ArrayStrategy
    feats = ['u_10m', 'v_10m', 'u_100m', 'v_100m', 'u_200m', 'v_200m']
    Sup3rGan.seed(13)
    means = {f: np.float32(0.2 * (i + 1)) for i, f in enumerate(feats)}
    stds = {f: np.float32(1.5 + 0.2 * i) for i, f in enumerate(feats)}
    means['topography'] = np.float32(2000.0)
    stds['topography'] = np.float32(1000.0)
    m = Sup3rGan(os.path.join(CFG, 'sup3r/sup3rcc/gen_wind_5x_1x_6f.json'),
                 os.path.join(CFG, 'test_disc_s_same.json'), means=means,
                 stdevs=stds, precision='bf16')
    m.set_model_params(lr_features=feats + ['topography'],
                       hr_out_features=feats, hr_exo_features=['topography'],
                       s_enhance=5, t_enhance=1)
    m.init_weights((1, 10, 9, 7), (1, 50, 45, 7))
    key = {'model_dir': 'fwp-exo-rasterised'}
    register_model('Sup3rGan', key, m)
    rng = np.random.default_rng(23)
    lr = lr_grid(16, 14)
    times = pd.date_range('2020-01-01', periods=3, freq='h')
    domain = (rng.standard_normal((16, 14, 3, 6)) * 2 + 0.4).astype(np.float32)
    ll, vals = source_raster(lr, factor=15, jitter=0.002)
    src = exo.ExoSource(ll, topography=vals)
    common = dict(spatial_pad=1, temporal_pad=0, max_nodes=1, model=m,
                  input_lat_lon=lr, input_time_index=times)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fields = exo.ExoDataHandler('topography', exo.ExoInput(lr, times),
                                    model=m, source_files=src).data
        a = ArrayStrategy(domain, key, (8, 7, 3), exo_handler_kwargs={
            'topography': {'source_files': src}}, **common)
    steps = fields['topography']['steps']
    assert [(s['combine_type'], s.shape) for s in steps] == [
        ('input', (16, 14, 1)), ('layer', (80, 70, 1))]
    assert all(s['data'].is_cuda for s in steps)
    for s in steps:
        s['data'] = s['data'].cpu().numpy()
    b = ArrayStrategy(domain, key, (8, 7, 3), exo_data=fields, **common)

    def run(st):
        done, kept = ForwardPass.run(st, 0, return_data=True)
        assert done == st.n_chunks == 4
        return dict(kept)
    got, want = run(a), run(b)
    assert sorted(got) == sorted(want) and len(got) == 4
    for k in want:
        assert np.isfinite(got[k]).all()
        assert np.array_equal(got[k], want[k])
