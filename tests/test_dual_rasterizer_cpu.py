"""CPU tests of ``sup3r_amd.dual_rasterizer`` on ``NumpyBackend``: the
reference's rasterizer procedures on arrays, its assertions and messages, the
backend's k-NN and weighted sum against the BallTree restatement
(tests/regrid_ref.py), and a rasterizer as a container of
``DeviceDualBatchHandler.from_containers`` over numpy stand-ins for the
device cubes."""
import os
import re
import warnings

import numpy as np
import pandas as pd
import pytest

import sup3r_amd
from sup3r_amd import (DeviceDualBatchHandler, DeviceDualSampler,
                       DualRasterizer, Regridder)
from sup3r_amd.derive import NumpyBackend
from tests import dual_rasterizer_cases as cases
from tests import regrid_ref as R
from tests import stats_ref

BE = NumpyBackend()
FEATURES = cases.FEATURES


def test_exports():
    for name in ('DeviceRegridder', 'Regridder', 'DeviceDualRasterizer',
                 'DualRasterizer'):
        assert name in sup3r_amd.__all__, name
    assert sup3r_amd.DualRasterizer is sup3r_amd.DeviceDualRasterizer
    assert sup3r_amd.Regridder is sup3r_amd.DeviceRegridder


def test_header_declares_the_regridder():
    from sup3r_amd import _lib
    here = os.path.dirname(os.path.abspath(__file__))
    header = open(os.path.join(here, '..', 'include', 'sup3r_hip.h')).read()
    for name in ('s3_regrid_knn_work_bytes', 's3_regrid_knn',
                 's3_regrid_apply'):
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert name in _lib.EXPORTS
    assert re.search(r'#define\s+S3_REGRID_MAX_K\s+' + str(_lib.REGRID_MAX_K),
                     header)


# ----------------------------------------------- the reference's procedures
def test_dual_rasterizer_shapes():
    cases.shapes_procedure(BE)


def test_dual_nan_fill():
    r, _ = cases.nan_fill_procedure(BE)
    # the fill is scipy's nearest value over the whole (L1, L2, T) block
    lr, hr = cases.pair(t_hr=5, lr_lat_lon=R.hr_grid())
    lr[FEATURES[0]][5:10, 5:10, 2] = np.nan
    raw = DualRasterizer((lr, hr), run_qa=False, backend=BE)
    holes = np.isnan(raw.lr_data[FEATURES[0]])
    assert 25 <= holes.sum() < 200 and not np.isnan(
        raw.lr_data[FEATURES[1]]).any()
    from scipy import ndimage as nd
    near = nd.distance_transform_edt(holes, return_distances=False,
                                     return_indices=True)
    want = raw.lr_data[FEATURES[0]][tuple(near)]
    np.testing.assert_array_equal(r.lr_data[FEATURES[0]], want)
    np.testing.assert_array_equal(r.lr_data[FEATURES[1]],
                                  raw.lr_data[FEATURES[1]])


def test_hr_shape_not_divisible_by_s_enhance():
    cases.uneven_procedure(BE)


def test_ten_percent_of_nan_is_a_value_error():
    lr, hr = cases.pair(t_hr=5, lr_lat_lon=R.hr_grid())
    lr[FEATURES[1]][:, :9, :] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with pytest.raises(ValueError,
                           match=r'v_100m data has \d+\.\d{3}% NaN values!'):
            DualRasterizer((lr, hr), backend=BE)
        # without the QA nothing is checked or filled
        r = DualRasterizer((lr, hr), run_qa=False, backend=BE)
    assert np.isnan(r.lr_data[FEATURES[1]]).any()


def test_assertion_messages():
    lr, hr = cases.pair()
    with pytest.raises(AssertionError, match='requires a data tuple or '
                       'dictionary with two members, low and high resolution '
                       "in that order.*Received <class 'list'>"):
        DualRasterizer([lr, hr], backend=BE)
    with pytest.raises(AssertionError, match='requires a data tuple'):
        DualRasterizer((lr, np.zeros((4, 4, 6))), backend=BE)
    with pytest.raises(AssertionError, match=re.escape(
            'Time steps of high-res data (3600.0 seconds) and low-res data '
            '(3600.0 seconds) are inconsistent with t_enhance = 2.')):
        DualRasterizer((lr, hr), t_enhance=2, backend=BE)
    small, _ = cases.pair(lr_lat_lon=R.lr_grid()[:4, :4])
    with pytest.raises(AssertionError, match=re.escape(
            'The required low-res shape (20, 20, 6) is inconsistent with the '
            'shape of the raw data (4, 4, 6)')):
        DualRasterizer((small, hr), s_enhance=1, backend=BE)
    short, _ = cases.pair(t_lr=4)
    with pytest.raises(AssertionError, match='required low-res shape'):
        DualRasterizer((short, hr), s_enhance=2, backend=BE)


def test_t_enhance_with_the_time_crop():
    # 7 hi-res hours, t_enhance 2 -> 3 low-res steps of the 5 at hand, 6 hours
    lr, hr = cases.pair(t_hr=7, t_lr=5, t_enhance=2)
    src = {f: np.array(lr[f]) for f in FEATURES}
    with pytest.warns(UserWarning, match=r'Using shape: \(20, 20, 6\)'):
        r = DualRasterizer((lr, hr), s_enhance=2, t_enhance=2, backend=BE)
    assert r.lr_required_shape == (10, 10, 3)
    assert r.hr_required_shape == (20, 20, 6)
    assert r.lr_data.shape == (10, 10, 3) and r.hr_data.shape == (20, 20, 6)
    assert list(r.lr_data.time_index) == list(lr.time_index[:3])
    assert list(r.hr_data.time_index) == list(hr.time_index[:6])
    reg = Regridder(lr.lat_lon.reshape(-1, 2), r.lr_lat_lon.reshape(-1, 2),
                    backend=BE)
    for f in FEATURES:
        want = R.rank_order_sum(reg.weights, reg.indices, src[f], t_out=3)
        np.testing.assert_array_equal(
            r.lr_data[f].reshape(100, 3).view(np.uint32), want.view(np.uint32))


def test_regrid_lr_false_leaves_the_low_res_bits_alone():
    lr, hr = cases.pair(lr_lat_lon=R.hr_grid(10, 10))
    before = {f: np.array(lr[f]) for f in FEATURES}
    r = DualRasterizer((lr, hr), s_enhance=2, regrid_lr=False, backend=BE)
    for i, f in enumerate(FEATURES):
        np.testing.assert_array_equal(r.lr_data[f].view(np.uint32),
                                      before[f].view(np.uint32))
        np.testing.assert_array_equal(r.low_res[..., i].view(np.uint32),
                                      before[f].view(np.uint32))
    # ... and the QA counts for itself
    lr[FEATURES[0]][1, 1, 1] = np.nan
    with pytest.warns(UserWarning, match='u_100m data has 0.167% NaN'):
        r = DualRasterizer((lr, hr), s_enhance=2, regrid_lr=False, backend=BE)
    assert not np.isnan(r.low_res).any()


def test_ignored_arguments_are_one_debug_line(caplog):
    lr, hr = cases.pair()
    with caplog.at_level('DEBUG', logger='sup3r_amd.dual_rasterizer'):
        DualRasterizer((lr, hr), s_enhance=2, regrid_workers=8,
                       lr_cache_kwargs={'cache_pattern': 'x'}, backend=BE)
    text = [rec.getMessage() for rec in caplog.records]
    assert sum('max_workers=8 ignored' in t for t in text) == 1
    assert sum('lr_cache_kwargs' in t and 'ignored' in t for t in text) == 1


# ------------------------------------------ NumpyBackend against regrid_ref
paired_grids = cases.paired_grids


def test_numpy_backend_against_the_balltree():
    src, tgt = paired_grids()
    assert R.gap_report(src, tgt, 4).min() > 1e-9
    dist, ind = R.balltree_knn(src, tgt, 4)
    reg = Regridder(src, pd.DataFrame({'latitude': tgt[:, 0],
                                       'longitude': tgt[:, 1]}), backend=BE)
    np.testing.assert_array_equal(reg.indices, ind)
    np.testing.assert_allclose(reg.distances, dist, rtol=1e-14, atol=0)
    want_w = R.weights(dist)
    np.testing.assert_array_equal(
        reg.weights.view(np.uint32), R.weights(reg.distances).view(np.uint32))
    np.testing.assert_allclose(reg.weights, want_w, rtol=2.0 ** -22, atol=0)
    np.testing.assert_allclose(reg.weights.sum(axis=1), 1.0, rtol=3e-7)
    rng = np.random.default_rng(5)
    data = (rng.standard_normal((*R.lr_grid().shape[:2], 7)) * 50).astype(
        np.float32)
    got = reg(data)
    assert got.shape == (100, 7) and got.dtype == np.float32
    want = R.regrid(want_w, ind, data)
    rows = data.reshape(-1, 7)
    bound = 2.0 ** -21 * np.einsum(
        'jk,jkt->jt', np.abs(want_w).astype(np.float64),
        np.abs(rows[ind]).astype(np.float64))
    assert (np.abs(got.astype(np.float64) - want) <= bound).all()
    np.testing.assert_array_equal(reg(data.reshape(-1, 7)), got)


def test_numpy_backend_rules():
    src, tgt = paired_grids()
    # a target on a source: distance 0, floor 1e-12, weight 1 on it
    tgt = np.concatenate([tgt, src[17:18]])
    h = BE.regrid_knn(src, tgt, 4)
    assert h['idx'][-1, 0] == 17 and h['dist'][-1, 0] == 0.0
    assert h['w'][-1, 0] == 1.0 and (h['w'][-1, 1:] < 1e-8).all()

    def knn(s, t, k):
        out = BE.regrid_knn(s, t, k)
        return out['idx'], out['dist']
    cases.ties_procedure(knn)
    n = len(src)
    with pytest.raises(ValueError, match='not finite'):
        BE.regrid_knn(np.array([[np.nan, 0.]] * 4, np.float32), tgt, 4)
    with pytest.raises(ValueError, match='k = 5'):
        BE.regrid_knn(src[:4], tgt, 5)
    # NaN propagates and is counted per plane; -0.0 survives the sum
    planes = [np.zeros((n, 3), np.float32), -np.zeros((n, 3), np.float32)]
    planes[0][int(h['idx'][0, 2]), 1] = np.nan
    outs, counts = BE.regrid_apply(h, planes, 2)
    assert outs[0].shape == (len(tgt), 2)
    assert counts[0] == np.isnan(outs[0]).sum() >= 1 and counts[1] == 0
    assert np.isnan(outs[0][0, 1]) and np.signbit(outs[1]).all()


# ----------------------------------------------------------------- end to end
class NumpyDualSampler(DeviceDualSampler):
    """``DeviceDualSampler`` over host cubes: gathers, moments and the
    normalisation in numpy (tests/stats_ref.py)"""

    def __init__(self, low_res, high_res, lr_features, hr_features,
                 sample_shape=None, batch_size=16, s_enhance=1, t_enhance=1,
                 feature_sets=None, seed=None):
        cubes = {'low_res': stats_ref.NumpyCube(low_res, lr_features),
                 'high_res': stats_ref.NumpyCube(high_res, hr_features)}
        s1, s2, t = sample_shape
        boxes = {'low_res': (s1 // s_enhance, s2 // s_enhance,
                             t // t_enhance), 'high_res': (s1, s2, t)}

        def gather(name):
            def run(origins, channels):
                b1, b2, bt = boxes[name]
                return np.stack([
                    cubes[name].data[i:i + b1, j:j + b2, k:k + bt]
                    [..., channels] for i, j, k in origins])
            return run
        super().__init__(
            low_res, high_res, lr_features, hr_features, sample_shape,
            batch_size=batch_size, s_enhance=s_enhance, t_enhance=t_enhance,
            feature_sets=feature_sets, seed=seed,
            gather={k: gather(k) for k in cubes})
        self.cubes = cubes

    def channel_moments(self, names):
        names = list(names)
        hr_names = [f.lower() for f in self.cubes['high_res'].features]
        hr = [f for f in names if f.lower() in hr_names]
        lr = [f for f in names if f.lower() not in hr_names]
        out = self.cubes['high_res'].moments(hr) if hr else {}
        if lr:
            out.update(self.cubes['low_res'].moments(lr))
        return {f: out[f] for f in names}

    def normalize(self, means, stds):
        for cube in self.cubes.values():
            cube.normalize(means, stds)


class NumpyDualHandler(DeviceDualBatchHandler):
    SAMPLER = NumpyDualSampler


def test_rasterizer_is_a_container_of_the_dual_batch_handler():
    lr, hr = cases.pair(t_hr=12, t_enhance=2)
    r = DualRasterizer((lr, hr), s_enhance=2, t_enhance=2, backend=BE)
    low, high = np.array(r.low_res), np.array(r.high_res)
    assert low.shape == (10, 10, 6, 2) and high.shape == (20, 20, 12, 2)
    kw = dict(sample_shape=(8, 8, 4), batch_size=3, n_batches=2, s_enhance=2,
              t_enhance=2, seed=4)
    bh = NumpyDualHandler.from_containers([r], **kw)
    batches = list(bh)
    bh.stop()
    assert len(batches) == 2
    for b in batches:
        assert np.asarray(b.low_res).shape == (3, 4, 4, 2, 2)
        assert np.asarray(b.high_res).shape == (3, 8, 8, 4, 2)
    assert set(bh.means) == set(FEATURES)
    # the rasterizer's cubes are the caller's: from_containers left them alone
    np.testing.assert_array_equal(np.array(r.low_res), low)
    # the same cubes fed to the sampler by hand, normalised with the
    # handler's stats: equal samples from the same seed
    by_hand = NumpyDualSampler(*r, sample_shape=(8, 8, 4), batch_size=3,
                               s_enhance=2, t_enhance=2, seed=4)
    by_hand.normalize(bh.means, bh.stds)
    again = NumpyDualHandler.from_containers([r], **kw)
    for _ in range(3):
        a_low, a_high = next(again.containers[0])
        b_low, b_high = next(by_hand)
        np.testing.assert_array_equal(a_low, b_low)
        np.testing.assert_array_equal(a_high, b_high)
    again.stop()
    assert again.means == bh.means and again.stds == bh.stds
