"""GPU tests (``-m gpu``) of the dual rasterizer: ``s3_regrid_knn`` and
``s3_regrid_apply`` through the C ABI into sentinel-filled buffers with red
zones, then ``DualRasterizer`` on ``DeviceBackend`` against the
``NumpyBackend`` route and as a container of ``DeviceDualBatchHandler``.

k-NN ids are compared with the brute-force float64 haversine of
tests/regrid_ref.py on inputs for which the test first asserts that no target
has two of its first ``k + 1`` distances within a relative 1e-9
(``gap_report``); planted exact ties (doubled source points: the same bits on
any libm) are checked for the smallest id.  Distances: within a relative 1e-14
of numpy's.  Weights: bit-equal to rex's formula applied to the device's own
distances, and within a relative 2^-22 of the reference's.  Weighted sums:
bit-equal to the float64 rank-order sum computed in numpy from the device's
indices and weights (NaN where that is NaN)."""
import ctypes as C
import warnings

import numpy as np
import pytest

from tests import dual_rasterizer_cases as cases
from tests import regrid_ref as R

pytestmark = pytest.mark.gpu

EINVAL = -1
PAD = 64                       # sentinel words in front of and behind a buffer
SENTINEL = 0x5A5AC3C3


def device():
    from sup3r_amd import _lib
    from sup3r_amd.engine import Device
    return Device.get(), _lib.lib()


def padded(words):
    import torch
    dev, _ = device()
    return torch.full((PAD + int(words) + PAD,), SENTINEL, dtype=torch.int32,
                      device=dev.torch_device)


def zones_intact(buf, words):
    host = buf.cpu().numpy().view(np.uint32)
    return bool((host[:PAD] == SENTINEL).all()
                and (host[PAD + int(words):] == SENTINEL).all())


def payload(buf, words):
    return buf.cpu().numpy().view(np.uint32)[PAD:PAD + int(words)].copy()


def inner(buf):
    return C.c_void_p(buf.data_ptr() + 4 * PAD)


def upload(arr):
    import torch
    dev, _ = device()
    return torch.from_numpy(np.ascontiguousarray(arr)).to(dev.torch_device)


def ptr(t):
    return C.c_void_p(t.data_ptr())


# --------------------------------------------------------------------- k-NN
def run_knn(src, tgt, k, want_dist=True, work_words=None, n_src=None,
            n_tgt=None):
    """``s3_regrid_knn`` -> (rc, idx (m, k), dist (m, k) or None, w (m, k));
    asserts that nothing around the outputs and the workspace was written"""
    dev, L = device()
    src = np.ascontiguousarray(src, np.float32).reshape(-1, 2)
    tgt = np.ascontiguousarray(tgt, np.float32).reshape(-1, 2)
    n, m = len(src), len(tgt)
    kk = max(1, min(int(k), 8))
    n_bytes = int(L.s3_regrid_knn_work_bytes(n))
    assert n_bytes > 0 and n_bytes % 8 == 0
    words = n_bytes // 4 if work_words is None else work_words
    work, idx = padded(words), padded(m * kk)
    dist, w = padded(2 * m * kk), padded(m * kk)
    assert (work.data_ptr() + 4 * PAD) % 8 == 0
    s, t = upload(src), upload(tgt)
    rc = L.s3_regrid_knn(
        dev.ctx, ptr(s), n if n_src is None else n_src, ptr(t),
        m if n_tgt is None else n_tgt, int(k), inner(work), 4 * words,
        inner(idx), inner(dist) if want_dist else None, inner(w))
    dev.sync()
    for buf, size in ((work, words), (idx, m * kk), (dist, 2 * m * kk),
                      (w, m * kk)):
        assert zones_intact(buf, size)
    if rc != 0:
        for buf, size in ((idx, m * kk), (dist, 2 * m * kk), (w, m * kk)):
            assert (payload(buf, size) == SENTINEL).all()
        return rc, None, None, None
    if not want_dist:
        assert (payload(dist, 2 * m * kk) == SENTINEL).all()
    return (rc, payload(idx, m * kk).view(np.int32).reshape(m, kk),
            payload(dist, 2 * m * kk).view(np.float64).reshape(m, kk)
            if want_dist else None,
            payload(w, m * kk).view(np.float32).reshape(m, kk))


def jittered(n1, n2, lat, lon, step, seed, jitter=0.3):
    """(n1 n2, 2) float32: a grid from (lat, lon) southward and eastward,
    every point moved by up to ``jitter`` of a step"""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(n1), np.arange(n2), indexing='ij')
    pts = np.stack([lat - step * i, lon + step * j], -1).reshape(-1, 2)
    pts = pts + rng.uniform(-jitter, jitter, pts.shape) * step
    return pts.astype(np.float32)


def check_knn(src, tgt, k, min_gap=1e-9):
    """the device against brute force on a gap-checked input"""
    assert R.gap_report(src, tgt, k).min() > min_gap
    want_d, want_i = R.brute_knn(src, tgt, k)
    rc, idx, dist, w = run_knn(src, tgt, k)
    assert rc == 0
    np.testing.assert_array_equal(idx, want_i)
    np.testing.assert_allclose(dist, want_d, rtol=1e-14, atol=0)
    np.testing.assert_array_equal(w.view(np.uint32),
                                  R.weights(dist).view(np.uint32))
    np.testing.assert_allclose(w, R.weights(want_d), rtol=2.0 ** -22, atol=0)
    # without the distances: the same ids and weights
    rc, idx2, none, w2 = run_knn(src, tgt, k, want_dist=False)
    assert rc == 0 and none is None
    np.testing.assert_array_equal(idx2, idx)
    np.testing.assert_array_equal(w2.view(np.uint32), w.view(np.uint32))
    return idx, dist, w


KNN_CASES = {
    'small': lambda: (jittered(12, 15, 41.0, -107.0, 0.25, 1),
                      jittered(5, 6, 40.2, -106.1, 0.31, 2)),
    'n_src_is_k': lambda: (jittered(2, 2, 40.0, -105.0, 0.25, 3),
                           jittered(3, 3, 40.1, -105.1, 0.2, 4)),
    'one_target': lambda: (jittered(12, 15, 41.0, -107.0, 0.25, 5),
                           np.array([[39.77, -105.31]], np.float32)),
    'rings': lambda: (jittered(70, 90, 45.0, -112.0, 0.11, 6),
                      jittered(33, 41, 44.2, -110.9, 0.17, 7)),
    # the targets' grid reaches two steps beyond the sources' box on every side
    'outside': lambda: (jittered(12, 15, 41.0, -107.0, 0.25, 8),
                        jittered(11, 12, 41.6, -107.6, 0.42, 9)),
}


@pytest.mark.parametrize('name', list(KNN_CASES))
def test_knn_against_brute_force(name):
    src, tgt = KNN_CASES[name]()
    if name == 'outside':
        box_lo, box_hi = src.min(axis=0), src.max(axis=0)
        assert (tgt[:, 0] > box_hi[0]).any() and (tgt[:, 0] < box_lo[0]).any()
        assert (tgt[:, 1] > box_hi[1]).any() and (tgt[:, 1] < box_lo[1]).any()
    check_knn(src, tgt, 4)


def test_knn_on_the_rasterizer_grids_against_the_balltree():
    src, tgt = cases.paired_grids()
    idx, dist, _ = check_knn(src, tgt, 4)
    tree_d, tree_i = R.balltree_knn(src, tgt, 4)
    np.testing.assert_array_equal(idx, tree_i)
    np.testing.assert_allclose(dist, tree_d, rtol=1e-14, atol=0)


@pytest.mark.parametrize('k', [1, 8])
def test_knn_k(k):
    src, tgt = KNN_CASES['small']()
    check_knn(src, tgt, k)


def test_knn_target_on_a_source():
    src, tgt = KNN_CASES['small']()
    tgt = np.concatenate([tgt, src[77:78]])
    rc, idx, dist, w = run_knn(src, tgt, 4)
    assert rc == 0
    assert idx[-1, 0] == 77 and dist[-1, 0] == 0.0
    assert w[-1, 0] == 1.0 and (w[-1, 1:] < 1e-8).all()
    np.testing.assert_array_equal(w.view(np.uint32),
                                  R.weights(dist).view(np.uint32))
    want_d, want_i = R.brute_knn(src, tgt, 4)
    np.testing.assert_array_equal(idx, want_i)


def test_knn_planted_ties_go_to_the_smaller_id():
    def knn(src, tgt, k):
        rc, idx, dist, _ = run_knn(src, tgt, k)
        assert rc == 0
        return idx, dist
    cases.ties_procedure(knn)


def test_knn_latitude_bands_date_line():
    east = jittered(9, 12, 12.0, 176.0, 0.33, 11)          # 176 .. 179.96
    west = jittered(9, 12, 12.0, -179.9, 0.33, 12)         # -180 .. -176
    src = np.concatenate([east, west])
    src[:, 1] = np.clip(src[:, 1], -180.0, 180.0)
    assert src[:, 1].max() - src[:, 1].min() > 180.0
    rng = np.random.default_rng(13)
    lat = rng.uniform(9.5, 12.0, 40)
    tgt = np.stack([lat, np.where(np.arange(40) % 2, 179.9, -179.9)],
                   -1).astype(np.float32)
    idx, _, _ = check_knn(src, tgt, 4)
    # neighbours come from both sides of the line
    sides = (idx < len(east))
    assert (sides.any(axis=1) & (~sides).any(axis=1)).any()


def test_knn_latitude_bands_polar_cap():
    rng = np.random.default_rng(14)
    src = np.stack([rng.uniform(85.2, 89.9, 700),
                    rng.uniform(-180.0, 180.0, 700)], -1).astype(np.float32)
    tgt = np.stack([rng.uniform(84.0, 89.95, 60),
                    rng.uniform(-180.0, 180.0, 60)], -1).astype(np.float32)
    check_knn(src, tgt, 4)


def test_knn_einval():
    from sup3r_amd import _lib
    dev, L = device()
    src, tgt = KNN_CASES['small']()
    full = int(L.s3_regrid_knn_work_bytes(len(src))) // 4

    def bad(text, **kw):
        args = dict(src=src, tgt=tgt, k=4)
        args.update(kw)
        rc = run_knn(**args)[0]
        msg = _lib.last_error(dev.ctx)
        assert rc == EINVAL and msg.startswith('s3_regrid_knn') \
            and text in msg, (kw.keys(), rc, msg)
    bad('fewer sources than k', src=src[:3])
    bad('fewer sources than k', src=src[:7], k=8)
    bad('k outside', k=0)
    bad('k outside', k=9)
    for where in ('src', 'tgt'):
        for value in (np.nan, np.inf, -np.inf):
            for col in (0, 1):
                pts = {'src': src.copy(), 'tgt': tgt.copy()}
                pts[where][len(pts[where]) // 2, col] = value
                bad('not finite', **pts)
    bad('start at 1', n_src=0)
    bad('start at 1', n_tgt=0)
    bad('2^31', n_src=2 ** 31)
    bad('2^31', n_tgt=2 ** 31)
    bad('work is smaller', work_words=full - 2)
    assert L.s3_regrid_knn_work_bytes(0) < 0
    assert L.s3_regrid_knn_work_bytes(2 ** 31) < 0
    s, t = upload(src), upload(tgt)
    work, out = padded(full), padded(2 * len(tgt) * 4)
    for args in ((None, ptr(t), inner(work), inner(out), inner(out)),
                 (ptr(s), None, inner(work), inner(out), inner(out)),
                 (ptr(s), ptr(t), None, inner(out), inner(out)),
                 (ptr(s), ptr(t), inner(work), None, inner(out)),
                 (ptr(s), ptr(t), inner(work), inner(out), None)):
        rc = L.s3_regrid_knn(dev.ctx, args[0], len(src), args[1], len(tgt), 4,
                             args[2], 4 * full, args[3], None, args[4])
        assert rc == EINVAL
    rc = L.s3_regrid_knn(dev.ctx, ptr(s), len(src), ptr(t), len(tgt), 4,
                         C.c_void_p(work.data_ptr() + 4 * PAD + 4),
                         4 * full, inner(out), None, inner(out))
    assert rc == EINVAL and '8-byte aligned' in _lib.last_error(dev.ctx)
    dev.sync()
    assert (payload(out, 2 * len(tgt) * 4) == SENTINEL).all()


# -------------------------------------------------------------------- apply
@pytest.fixture(scope='module')
def tables():
    """indices and weights of the device for 180 sources and 30 targets, for
    k = 4 (and the host copies)"""
    src, tgt = KNN_CASES['small']()
    rc, idx, _, w = run_knn(src, tgt, 4)
    assert rc == 0
    return idx, w, upload(idx), upload(w)


def run_apply(planes, idx_d, w_d, n_tgt, k, t_out, n_src=None):
    """``s3_regrid_apply`` -> (rc, outputs as uint32 (n_tgt, t_out), counts);
    asserts the red zones of every output and of the counts"""
    import torch
    dev, L = device()
    n_var = len(planes)
    n_src = planes[0].shape[0] if n_src is None else n_src
    t_src = planes[0].shape[1]
    size = n_tgt * max(t_out, 1)
    srcs = [padded(p.size) for p in planes]
    for buf, p in zip(srcs, planes):
        buf[PAD:PAD + p.size] = torch.from_numpy(
            np.ascontiguousarray(p).view(np.int32).reshape(-1)).to(buf.device)
    outs = [padded(size) for _ in planes]
    counts = padded(2 * n_var)
    assert (counts.data_ptr() + 4 * PAD) % 8 == 0
    vp = C.c_void_p * n_var
    rc = L.s3_regrid_apply(
        dev.ctx, n_var, vp(*[b.data_ptr() + 4 * PAD for b in srcs]),
        vp(*[b.data_ptr() + 4 * PAD for b in outs]), n_src, n_tgt, t_src,
        t_out, k, ptr(idx_d), ptr(w_d), inner(counts))
    dev.sync()
    assert zones_intact(counts, 2 * n_var)
    for buf, p in zip(srcs, planes):
        assert zones_intact(buf, p.size)
        np.testing.assert_array_equal(payload(buf, p.size),
                                      p.view(np.uint32).reshape(-1))
    for buf in outs:
        assert zones_intact(buf, size)
    if rc != 0:
        for buf in outs:
            assert (payload(buf, size) == SENTINEL).all()
        return rc, None, None
    return (rc, [payload(b, size).reshape(n_tgt, t_out) for b in outs],
            payload(counts, 2 * n_var).view(np.int64))


def check_apply(planes, tables, t_out):
    idx, w, idx_d, w_d = tables
    rc, outs, counts = run_apply(planes, idx_d, w_d, len(idx), 4, t_out)
    assert rc == 0
    for plane, out, count in zip(planes, outs, counts):
        want = R.rank_order_sum(w, idx, plane, t_out)
        nan = np.isnan(want)
        got = out.view(np.float32)
        np.testing.assert_array_equal(np.isnan(got), nan)
        np.testing.assert_array_equal(out[~nan], want.view(np.uint32)[~nan])
        assert count == nan.sum()
    return outs, counts


def plane_of(n, t, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, t)) * 30 + 5).astype(np.float32)


@pytest.mark.parametrize('t', [1, 3, 4, 5, 63, 64, 65, 257])
def test_apply_row_lengths(tables, t):
    check_apply([plane_of(180, t, t), plane_of(180, t, 100 + t)], tables, t)


@pytest.mark.parametrize('t_src, t_out', [(9, 1), (66, 63), (300, 257),
                                          (1100, 1027)])
def test_apply_time_crop(tables, t_src, t_out):
    check_apply([plane_of(180, t_src, t_src)], tables, t_out)


@pytest.mark.parametrize('n_var', [1, 2, 9])
def test_apply_variables(tables, n_var):
    planes = [plane_of(180, 21, 40 + v) for v in range(n_var)]
    planes[-1][int(tables[0][3, 1]), 5] = np.nan
    outs, counts = check_apply(planes, tables, 21)
    assert counts[-1] >= 1 and (counts[:-1] == 0).all()


def test_apply_special_values(tables):
    idx = tables[0]
    a, b = plane_of(180, 37, 1), plane_of(180, 37, 2)
    rng = np.random.default_rng(3)
    for plane, values in ((a, [np.nan, np.inf, -0.0]),
                          (b, [-np.inf, np.nan, np.inf])):
        for value in values:
            rows = rng.choice(np.unique(idx), 6, replace=False)
            plane[rows, rng.integers(0, 37, 6)] = value
    a[int(idx[0, 0]), 0] = np.inf                       # inf - inf in one sum
    a[int(idx[0, 1]), 0] = -np.inf
    zeros = -np.zeros((180, 37), np.float32)
    first, counts = check_apply([a, b, zeros], tables, 37)
    assert counts[0] > 0 and counts[1] > 0 and counts[2] == 0
    assert np.isnan(first[0].view(np.float32)[0, 0])
    assert (first[2] == 0x80000000).all()               # -0.0 survives the sum
    again, counts2 = check_apply([a, b, zeros], tables, 37)
    for x, y in zip(first, again):
        np.testing.assert_array_equal(x, y)             # NaN bits included
    np.testing.assert_array_equal(counts, counts2)


def test_apply_k_1_and_8():
    src, tgt = KNN_CASES['small']()
    for k in (1, 8):
        rc, idx, _, w = run_knn(src, tgt, k)
        assert rc == 0
        plane = plane_of(180, 13, k)
        rc, outs, counts = run_apply([plane], upload(idx), upload(w),
                                     len(tgt), k, 13)
        assert rc == 0 and counts[0] == 0
        np.testing.assert_array_equal(
            outs[0], R.rank_order_sum(w, idx, plane).view(np.uint32))


def test_apply_plane_past_2_31_elements():
    import torch
    dev, L = device()
    rows, t = 33000, 65600
    assert rows * t > 2 ** 31
    plane = torch.empty((rows, t), dtype=torch.float32,
                        device=dev.torch_device)
    idx = np.array([[32999, 0, 32760, 17], [32737, 32999, 5, 32760],
                    [17, 5, 0, 32737]], np.int32)
    assert (idx.astype(np.int64).max(axis=1) * t > 2 ** 31).all()
    w = np.array([[.4, .3, .2, .1], [.7, .1, .1, .1], [.25, .25, .25, .25]],
                 np.float32)
    rng = np.random.default_rng(9)
    host = {}
    for r in np.unique(idx):
        host[int(r)] = (rng.standard_normal(t) * 10).astype(np.float32)
        plane[int(r)] = torch.from_numpy(host[int(r)]).to(plane.device)
    out = padded(3 * t)
    counts = padded(2)
    vp = C.c_void_p * 1
    idx_d, w_d = upload(idx), upload(w)         # (referenced until the sync)
    rc = L.s3_regrid_apply(dev.ctx, 1, vp(plane.data_ptr()),
                           vp(out.data_ptr() + 4 * PAD), rows, 3, t, t, 4,
                           ptr(idx_d), ptr(w_d), inner(counts))
    dev.sync()
    assert rc == 0 and zones_intact(out, 3 * t)
    assert payload(counts, 2).view(np.int64)[0] == 0
    got = payload(out, 3 * t).reshape(3, t)
    for j in range(3):
        acc = w[j, 0].astype(np.float64) * host[int(idx[j, 0])].astype(
            np.float64)
        for q in range(1, 4):
            acc = acc + w[j, q].astype(np.float64) * host[
                int(idx[j, q])].astype(np.float64)
        np.testing.assert_array_equal(got[j],
                                      acc.astype(np.float32).view(np.uint32))


def test_apply_einval(tables):
    from sup3r_amd import _lib
    dev, L = device()
    idx, w, idx_d, w_d = tables
    plane = plane_of(180, 8, 1)

    def bad(text, planes=(plane,), k=4, t_out=8, **kw):
        rc = run_apply(list(planes), idx_d, w_d, len(idx), k, t_out, **kw)[0]
        msg = _lib.last_error(dev.ctx)
        assert rc == EINVAL and msg.startswith('s3_regrid_apply') \
            and text in msg, (rc, msg)
    bad('T_out', t_out=9)
    bad('T_out', t_out=0)
    bad('k outside', k=0)
    bad('k outside', k=9)
    bad('n_src and n_tgt', n_src=0)
    vp = C.c_void_p * 1
    out, counts = padded(len(idx) * 8), padded(2)
    src = upload(plane)
    ok = dict(n_var=1, src=vp(src.data_ptr()), out=vp(out.data_ptr() + 4 * PAD),
              idx=ptr(idx_d), w=ptr(w_d), counts=inner(counts))
    for key, value in (('n_var', 0), ('n_var', -1), ('src', None),
                       ('out', None), ('idx', None), ('w', None),
                       ('counts', None), ('src', vp(None)),
                       ('out', vp(None))):
        a = dict(ok)
        a[key] = value
        rc = L.s3_regrid_apply(dev.ctx, a['n_var'], a['src'], a['out'], 180,
                               len(idx), 8, 8, 4, a['idx'], a['w'],
                               a['counts'])
        assert rc == EINVAL, key
        assert _lib.last_error(dev.ctx).startswith('s3_regrid_apply')
    dev.sync()
    assert (payload(out, len(idx) * 8) == SENTINEL).all()


# ------------------------------------------------------ the class on the device
@pytest.fixture(scope='module')
def backends():
    from sup3r_amd.derive import DeviceBackend, NumpyBackend
    return DeviceBackend(), NumpyBackend()


def same_cubes(r_dev, r_np, dev_be):
    """the k-NN indices agree, hence the cubes do, bit for bit"""
    for name in ('low_res', 'high_res'):
        got = cases.host(dev_be, getattr(r_dev, name))
        want = np.asarray(getattr(r_np, name))
        assert got.shape == want.shape
        np.testing.assert_array_equal(got.view(np.uint32),
                                      want.view(np.uint32))


def regridders_agree(r_dev, lr, dev_be, np_be):
    from sup3r_amd import Regridder
    src, tgt = lr.lat_lon.reshape(-1, 2), r_dev.lr_lat_lon.reshape(-1, 2)
    a = Regridder(src, tgt, backend=dev_be)
    b = Regridder(src, tgt, backend=np_be)
    np.testing.assert_array_equal(a.indices, b.indices)
    np.testing.assert_allclose(a.distances, b.distances, rtol=1e-14, atol=0)


def test_class_shapes(backends):
    dev_be, np_be = backends
    r_dev = cases.shapes_procedure(dev_be)
    r_np = cases.shapes_procedure(np_be)
    regridders_agree(r_dev, cases.pair()[0], dev_be, np_be)
    same_cubes(r_dev, r_np, dev_be)
    assert r_dev.low_res.is_cuda and r_dev.low_res is r_dev.low_res


def test_class_nan_fill(backends):
    dev_be, np_be = backends
    r_dev, texts = cases.nan_fill_procedure(dev_be)
    r_np, texts_np = cases.nan_fill_procedure(np_be)
    assert [t for t in texts if 'NaN values' in t] == \
        [t for t in texts_np if 'NaN values' in t]
    lr = cases.pair(t_hr=5, lr_lat_lon=R.hr_grid())[0]
    from sup3r_amd import Regridder
    src = lr.lat_lon.reshape(-1, 2)
    np.testing.assert_array_equal(
        Regridder(src, src, backend=dev_be).indices,
        Regridder(src, src, backend=np_be).indices)
    same_cubes(r_dev, r_np, dev_be)


def test_class_uneven_hr_shape(backends):
    dev_be, np_be = backends
    r_dev = cases.uneven_procedure(dev_be)
    r_np = cases.uneven_procedure(np_be)
    regridders_agree(r_dev, cases.pair(hr_shape=(21, 23))[0], dev_be, np_be)
    same_cubes(r_dev, r_np, dev_be)


def test_class_regrid_lr_false_counts_for_itself(backends):
    from sup3r_amd import DualRasterizer
    dev_be, _ = backends
    lr, hr = cases.pair(lr_lat_lon=R.hr_grid(10, 10))
    before = {f: np.array(lr[f]) for f in cases.FEATURES}
    r = DualRasterizer((lr, hr), s_enhance=2, regrid_lr=False, backend=dev_be)
    for i, f in enumerate(cases.FEATURES):
        np.testing.assert_array_equal(
            cases.host(dev_be, r.low_res)[..., i].view(np.uint32),
            before[f].view(np.uint32))
    lr, hr = cases.pair(lr_lat_lon=R.hr_grid(10, 10))
    lr[cases.FEATURES[0]][1, 1, 1] = np.nan
    with pytest.warns(UserWarning, match='u_100m data has 0.167% NaN'):
        r = DualRasterizer((lr, hr), s_enhance=2, regrid_lr=False,
                           backend=dev_be)
    assert not np.isnan(cases.host(dev_be, r.low_res)).any()
    lr, hr = cases.pair(lr_lat_lon=R.hr_grid(10, 10))
    lr[cases.FEATURES[1]][:, :2] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with pytest.raises(ValueError, match='v_100m data has 20.000% NaN'):
            DualRasterizer((lr, hr), s_enhance=2, regrid_lr=False,
                           backend=dev_be)


def test_class_feeds_the_dual_batch_handler(backends):
    from sup3r_amd import (DeviceDualBatchHandler, DeviceDualSampler,
                           DualRasterizer)
    dev_be, _ = backends
    lr, hr = cases.pair(t_hr=12, t_enhance=2)
    r = DualRasterizer((lr, hr), s_enhance=2, t_enhance=2, backend=dev_be)
    low = cases.host(dev_be, r.low_res).copy()
    high = cases.host(dev_be, r.high_res).copy()
    by_hand = DeviceDualSampler(low, high, r.lr_features, r.hr_features,
                                sample_shape=(8, 8, 4), batch_size=3,
                                s_enhance=2, t_enhance=2, seed=4)
    bh = DeviceDualBatchHandler.from_containers(
        [r], sample_shape=(8, 8, 4), batch_size=3, n_batches=2, s_enhance=2,
        t_enhance=2, seed=4)
    by_hand.normalize(bh.means, bh.stds)
    # the rasterizer's device cubes are the sampler's memory: not copied
    assert bh.containers[0].low_res.data_ptr() == r.low_res.data_ptr()
    a_low, a_high = next(bh.containers[0])
    b_low, b_high = next(by_hand)
    assert tuple(a_low.shape) == (3, 4, 4, 2, 2)
    assert tuple(a_high.shape) == (3, 8, 8, 4, 2)
    np.testing.assert_array_equal(a_low.cpu().numpy(), b_low.cpu().numpy())
    np.testing.assert_array_equal(a_high.cpu().numpy(), b_high.cpu().numpy())
    batch = next(iter(bh))
    bh.stop()
    assert tuple(batch.low_res.shape) == (3, 4, 4, 2, 2)
    assert tuple(batch.high_res.shape) == (3, 8, 8, 4, 2)
    assert batch.low_res.is_cuda and set(bh.means) == set(cases.FEATURES)
