"""Inputs and procedures that tests/test_dual_rasterizer_cpu.py runs on
``NumpyBackend`` and tests/test_dual_rasterizer_gpu.py on ``DeviceBackend``:
the reference's ``test_dual_rasterizer_shapes`` and ``test_dual_nan_fill``
(tests/rasterizers/test_dual.py) on arrays, and the uneven hi-res shape."""
import warnings

import numpy as np
import pandas as pd

from sup3r_amd import DualRasterizer
from sup3r_amd.derive import DeriveData
from tests import regrid_ref as R

FEATURES = ['u_100m', 'v_100m']


def fields(shape, seed, features=FEATURES):
    rng = np.random.default_rng(seed)
    return {f: (rng.standard_normal(shape) * 4 + 3 * i).astype(np.float32)
            for i, f in enumerate(features)}


def pair(hr_shape=(20, 20), t_hr=6, t_lr=None, t_enhance=1, seed=0,
         lr_lat_lon=None):
    """(low-res, hi-res) ``DeriveData`` on host arrays, not bound: the
    curvilinear hi-res grid near (39.01, -105.15) and the 0.25-degree grid
    around it"""
    hr_ll = R.hr_grid(*hr_shape)
    lr_ll = R.lr_grid() if lr_lat_lon is None else lr_lat_lon
    t_lr = t_hr // t_enhance if t_lr is None else t_lr
    hr_ti = pd.date_range('2020-01-01', periods=t_hr, freq='h')
    lr_ti = pd.date_range('2020-01-01', periods=t_lr, freq=f'{t_enhance}h')
    hr = DeriveData(fields((*hr_shape, t_hr), seed), hr_ll, hr_ti)
    lr = DeriveData(fields((*lr_ll.shape[:2], t_lr), seed + 1), lr_ll, lr_ti)
    return lr, hr


def host(backend, x):
    return np.asarray(backend.to_numpy(x))


def shapes_procedure(backend):
    """``test_dual_rasterizer_shapes``; returns the rasterizer"""
    lr, hr = pair()
    r = DualRasterizer({'low_res': lr, 'high_res': hr}, s_enhance=2,
                       t_enhance=1, backend=backend)
    assert r.lr_data.shape == (r.hr_data.shape[0] // 2,
                               r.hr_data.shape[1] // 2, *r.hr_data.shape[2:])
    assert tuple(r.low_res.shape) == (10, 10, 6, 2)
    assert tuple(r.high_res.shape) == (20, 20, 6, 2)
    assert r.lr_features == FEATURES and r.hr_features == FEATURES
    np.testing.assert_array_equal(r.lr_data.lat_lon, r.lr_lat_lon)
    assert len(r.lr_data.time_index) == 6
    return r


def nan_fill_procedure(backend):
    """``test_dual_nan_fill``: both members on the hi-res grid, a 5 x 5 x 1
    block of NaN in the first low-res feature, ``s_enhance = 1``; returns the
    rasterizer and the warnings"""
    hr_ll = R.hr_grid()
    lr, hr = pair(t_hr=5, lr_lat_lon=hr_ll)
    assert not any(np.isnan(lr[f]).any() for f in FEATURES)
    lr[FEATURES[0]][5:10, 5:10, 2] = np.nan
    assert np.isnan(lr[FEATURES[0]]).any()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        r = DualRasterizer({'low_res': lr, 'high_res': hr}, s_enhance=1,
                           t_enhance=1, backend=backend)
    assert not np.isnan(host(backend, r.low_res)).any()
    for f in FEATURES:
        assert not np.isnan(host(backend, r.lr_data[f])).any()
    texts = [str(w.message) for w in caught]
    named = [t for t in texts if t.endswith('% NaN values!')]
    assert len(named) == 1 and named[0].startswith(f'{FEATURES[0]} data has ')
    return r, texts


def uneven_procedure(backend):
    """hi-res 21 x 23 with ``s_enhance = 2`` -> 20 x 22, with the warning"""
    lr, hr = pair(hr_shape=(21, 23))
    want = {f: np.array(hr[f][:20, :22]) for f in FEATURES}
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        r = DualRasterizer((lr, hr), s_enhance=2, backend=backend)
    texts = [str(w.message) for w in caught]
    assert ('hr_data.shape: (21, 23, 6) is not divisible by s_enhance: 2. '
            'Using shape: (20, 22, 6) instead.') in texts
    assert r.hr_data.shape == (20, 22, 6) and r.lr_data.shape == (10, 11, 6)
    assert r.hr_data.lat_lon.shape == (20, 22, 2)
    for f in FEATURES:
        np.testing.assert_array_equal(
            host(backend, r.hr_data[f]).view(np.uint32),
            want[f].view(np.uint32))
    assert tuple(r.high_res.shape) == (20, 22, 6, 2)
    return r


def paired_grids():
    """sources and targets of the shapes procedure, flat"""
    from sup3r_amd.dual_rasterizer import spatial_coarsening
    return (R.lr_grid().reshape(-1, 2),
            spatial_coarsening(R.hr_grid(), 2).reshape(-1, 2))


def ties_procedure(knn):
    """exact ties planted by doubling source points (the same bits on any
    libm): inside the first four, and across the 4th / 5th place; the smaller
    id wins.  ``knn(src, tgt, k) -> (idx, dist)`` on the host."""
    src, tgt = paired_grids()
    n0 = len(src)
    _, base = R.brute_knn(src, tgt, 4)
    a = int(base[0, 1])                       # 2nd of target 0
    j = next(j for j in range(1, len(tgt)) if a not in base[j])
    b = int(base[j, 3])                       # 4th of target j
    assert b not in base[0] and a != b
    src = np.concatenate([src, src[[a, b]]])
    idx, dist = knn(src, tgt, 4)
    assert list(idx[0]) == [base[0, 0], a, n0, base[0, 2]]
    assert dist[0, 1] == dist[0, 2]
    assert list(idx[j]) == list(base[j]) and n0 + 1 not in idx[j]
    idx5, dist5 = knn(src, tgt, 5)
    assert list(idx5[j, 3:]) == [b, n0 + 1] and dist5[j, 3] == dist5[j, 4]
    np.testing.assert_array_equal(idx5[:, :4], idx)
