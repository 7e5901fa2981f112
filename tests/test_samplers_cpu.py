"""Index logic of the device-resident samplers and of the data-centric / dual
batch queues (sup3r_amd/samplers.py, batch_queue_dc.py, batch_queue_dual.py)
without a GPU: a numpy gather stands in for ``s3_sample_gather`` and an
identity transform for the device one.  The few lines of index arithmetic that
are checked are restated here; every comparison is exact."""
import warnings

import numpy as np
import pytest

from sup3r_amd import (DeviceBatchHandlerDC, DeviceBatchQueue,
                       DeviceDualBatchHandler, DeviceDualBatchQueue,
                       DeviceDualSampler, DeviceSampler, DeviceSamplerDC,
                       DeviceValBatchQueueDC)
from sup3r_amd.samplers import start_probabilities

FEATS = ['u_10m', 'v_10m', 'U_100m', 'pressure_0m', 'topography']


def np_gather(cube, box, log=None):
    """``(origins, channels) -> batch`` by numpy slicing"""
    s1, s2, t = box

    def gather(origins, channels):
        if log is not None:
            log.append((np.array(origins), list(channels)))
        return np.stack([cube[i:i + s1, j:j + s2, k:k + t][..., channels]
                         for i, j, k in origins])
    return gather


def cube_of(shape, seed=0):
    return np.random.default_rng(seed).standard_normal(shape).astype(
        np.float32)


def sampler(shape=(9, 11, 40, 2), box=(4, 5, 3), batch_size=4, seed=3,
            feats=('a', 'b'), cls=DeviceSampler, **kw):
    cube = cube_of(shape)
    box3 = tuple(box) + (1,) * (3 - len(box))
    return cube, cls(cube, list(feats), box, batch_size=batch_size, seed=seed,
                     gather=np_gather(cube, box3), **kw)


def identity_transform(samples, **_):
    return samples, samples


def chunk_of(start, n_starts, n_bins):
    """the bin of a start: its chunk of np.array_split(arange(n_starts))"""
    chunks = np.array_split(np.arange(n_starts), n_bins)
    return next(b for b, c in enumerate(chunks) if start in c)


# ------------------------------------------------------------- feature sets
def test_feature_sets_wildcards_and_hr_indices():
    cube = cube_of((6, 6, 8, 5))
    s = DeviceSampler(cube, FEATS, (3, 3, 2), batch_size=2,
                      feature_sets={'lr_only_features': ['pres*'],
                                    'hr_exo_features': ['topography']},
                      gather=np_gather(cube, (3, 3, 2)))
    assert s.features == FEATS and s.lr_features == FEATS
    assert s.lr_only_features == ['pressure_0m']
    assert s.hr_exo_features == ['topography']
    assert s.hr_out_features == ['u_10m', 'v_10m', 'u_100m']
    assert list(s.hr_features_ind) == [0, 1, 2, 4]
    assert s.hr_features == ['u_10m', 'v_10m', 'u_100m', 'topography']
    assert s.shape == (6, 6, 8, 5) and s.size == cube.size
    assert s.compute() is s and s.hr_sample_shape == (3, 3, 2)
    plain = DeviceSampler(cube, FEATS, (3, 3), batch_size=2,
                          gather=np_gather(cube, (3, 3, 1)))
    assert plain.sample_shape == (3, 3, 1)       # 2-tuple: trailing 1
    assert list(plain.hr_features_ind) == [0, 1, 2, 3, 4]
    sub = DeviceSampler(cube, FEATS, (3, 3, 2), batch_size=2,
                        feature_sets={'features': ['topography', 'u_10m']},
                        gather=np_gather(cube, (3, 3, 2)))
    np.testing.assert_array_equal(
        next(sub)[0], cube[sub.last_origins[0][0]:, sub.last_origins[0][1]:,
                           sub.last_origins[0][2]:][:3, :3, :2][..., [4, 0]])


def test_feature_sets_errors():
    cube = cube_of((6, 6, 8, 5))
    g = np_gather(cube, (3, 3, 2))
    s = DeviceSampler(cube, FEATS, (3, 3, 2), batch_size=2, gather=g,
                      feature_sets={'hr_exo_features': ['u_10m']})
    with pytest.raises(AssertionError):          # exo not at the end
        s.hr_exo_features
    s = DeviceSampler(cube, FEATS, (3, 3, 2), batch_size=2, gather=g,
                      feature_sets={'lr_only_features': ['*']})
    with pytest.raises(RuntimeError):            # nothing left to output
        s.hr_out_features
    with pytest.raises(KeyError):
        DeviceSampler(cube, FEATS, (3, 3, 2), gather=g, batch_size=2,
                      feature_sets={'features': ['nope']})
    with pytest.raises(AssertionError):          # one name per channel
        DeviceSampler(cube, FEATS[:4], (3, 3, 2), gather=g, batch_size=2)


def test_preflight():
    cube = cube_of((6, 7, 10, 2))
    g = np_gather(cube, (3, 3, 2))
    with pytest.raises(AssertionError):          # box larger than the raster
        DeviceSampler(cube, ['a', 'b'], (7, 3, 2), batch_size=2, gather=g)
    with pytest.raises(AssertionError):
        DeviceSampler(cube, ['a', 'b'], (3, 8, 2), batch_size=2, gather=g)
    with pytest.raises(AssertionError):          # t > T
        DeviceSampler(cube, ['a', 'b'], (3, 3, 11), batch_size=1, gather=g)
    with warnings.catch_warnings():
        warnings.simplefilter('error')           # 5 * 2 = T: still fast
        s = DeviceSampler(cube, ['a', 'b'], (3, 3, 2), batch_size=5, gather=g)
    assert s._fast_batch_possible()
    with pytest.warns(UserWarning, match='larger than the number of time'):
        s = DeviceSampler(cube, ['a', 'b'], (3, 3, 2), batch_size=6, gather=g,
                          seed=1)
    assert not s._fast_batch_possible()
    next(s)
    assert len({tuple(o) for o in s.last_origins}) > 1   # independent boxes


# ------------------------------------------------------------------- replay
@pytest.mark.parametrize('seed', [0, 17])
def test_fast_batches_replay_the_documented_draws(seed):
    (S1, S2, T, _), (s1, s2, t), B = (9, 11, 40, 2), (4, 5, 3), 4
    cube, s = sampler(seed=seed)
    rng = np.random.default_rng(seed)
    for _ in range(50):
        batch = next(s)
        i0 = rng.integers(0, S1 - s1 + 1)
        j0 = rng.integers(0, S2 - s2 + 1)
        k0 = rng.integers(0, T - B * t + 1)
        want = np.array([(i0, j0, k0 + m * t) for m in range(B)])
        np.testing.assert_array_equal(s.last_origins, want)
        lo, hi = s.last_origins.min(0), s.last_origins.max(0)
        assert (lo >= 0).all() and (hi + (s1, s2, t) <= (S1, S2, T)).all()
        # the reference's reshape of one (s1, s2, B t) box
        box = cube[i0:i0 + s1, j0:j0 + s2, k0:k0 + B * t]
        np.testing.assert_array_equal(
            batch, box.reshape(s1, s2, B, t, 2).transpose(2, 0, 1, 3, 4))


def test_slow_batches_replay_the_documented_draws():
    (S1, S2, T, _), (s1, s2, t), B = (9, 11, 10, 2), (4, 5, 3), 4
    with pytest.warns(UserWarning):
        cube, s = sampler(shape=(S1, S2, T, 2), seed=5)
    rng = np.random.default_rng(5)
    for _ in range(50):
        next(s)
        want = [(rng.integers(0, S1 - s1 + 1), rng.integers(0, S2 - s2 + 1),
                 rng.integers(0, T - t + 1)) for _ in range(B)]
        np.testing.assert_array_equal(s.last_origins, np.array(want))
        assert (s.last_origins + (s1, s2, t) <= (S1, S2, T)).all()


def test_get_sample_index_is_slices_and_features():
    _, s = sampler()
    rows, cols, steps, feats = s.get_sample_index()
    assert (rows.stop - rows.start, cols.stop - cols.start,
            steps.stop - steps.start) == (4, 5, 3 * 4)
    assert feats == ['a', 'b']
    one = s.get_sample_index(n_obs=1)[2]
    assert one.stop - one.start == 3


# ------------------------------------------------------------ data centric
def test_start_probabilities_is_the_array_split_construction():
    w = [0.2, 0.5, 0.3]
    want = np.array([w[0]] * 3 + [w[1]] * 2 + [w[2]] * 2)
    np.testing.assert_array_equal(start_probabilities(7, w),
                                  want / want.sum())
    # 12 box starts: a (3, 3) box on a (5, 6) grid has 3 x 4 of them
    w5 = [1.0, 0.0, 2.0, 0.5, 0.5]
    sizes = [len(c) for c in np.array_split(np.arange(12), 5)]
    assert sizes == [3, 3, 2, 2, 2]
    want = np.concatenate([[x] * k for x, k in zip(w5, sizes)])
    np.testing.assert_array_equal(start_probabilities(12, w5),
                                  want / want.sum())
    np.testing.assert_array_equal(DeviceSamplerDC.start_probabilities(7, w),
                                  start_probabilities(7, w))


@pytest.mark.parametrize('space_bin,time_bin', [(0, 0), (2, 1), (4, 3)])
def test_one_hot_weights_confine_every_draw(space_bin, time_bin):
    cube = cube_of((5, 6, 30, 1))
    s = DeviceSamplerDC(cube, ['a'], (3, 3, 2), batch_size=2, seed=9,
                        gather=np_gather(cube, (3, 3, 2)),
                        spatial_weights=np.eye(5)[space_bin],
                        temporal_weights=np.eye(4)[time_bin])
    n_time_starts = 30 - 2 * 2 + 1
    for _ in range(200):
        rows, cols, steps, _ = s.get_sample_index()
        flat = rows.start * 4 + cols.start           # row-major, 4 columns
        assert chunk_of(flat, 12, 5) == space_bin
        assert chunk_of(steps.start, n_time_starts, 4) == time_bin
        assert rows.stop <= 5 and cols.stop <= 6 and steps.stop <= 30


def test_weighted_draws_replay():
    cube = cube_of((5, 6, 30, 1))
    ws, wt = [0.1, 0.9], [0.5, 0.25, 0.25]
    s = DeviceSamplerDC(cube, ['a'], (3, 3, 2), batch_size=2, seed=4,
                        gather=np_gather(cube, (3, 3, 2)),
                        spatial_weights=ws, temporal_weights=wt)
    rng = np.random.default_rng(4)
    for _ in range(20):
        next(s)
        start = rng.choice(np.arange(12), p=start_probabilities(12, ws))
        k0 = rng.choice(np.arange(27), p=start_probabilities(27, wt))
        np.testing.assert_array_equal(
            s.last_origins, [(start // 4, start % 4, k0 + 2 * m)
                             for m in range(2)])


def test_weights_without_a_start_are_a_value_error():
    with pytest.raises(ValueError, match='7 starts'):
        start_probabilities(7, [0.0, 0.0, 0.0])
    with pytest.raises(ValueError, match='2 starts'):
        start_probabilities(2, [0.0, 0.0, 1.0])      # third chunk is empty
    cube = cube_of((5, 6, 30, 1))
    s = DeviceSamplerDC(cube, ['a'], (3, 3, 2), batch_size=2,
                        gather=np_gather(cube, (3, 3, 2)),
                        spatial_weights=[0, 0])
    with pytest.raises(ValueError, match=r'\[0\.0, 0\.0\]'):
        next(s)


def dc_samplers(n, seed0=0, shape=(6, 8, 20, 2), box=(4, 4, 4), batch_size=6):
    """slow-batch DC samplers (6 * 4 steps > 20): every origin is a draw"""
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for q in range(n):
            cube = cube_of(shape, seed=seed0 + q)
            out.append(DeviceSamplerDC(
                cube, ['a', 'b'], box, batch_size=batch_size, seed=seed0 + q,
                gather=np_gather(cube, box)))
    return out


def test_val_queue_dc_visits_every_cell_once_in_filing_order():
    (smp,) = dc_samplers(1)
    q = DeviceValBatchQueueDC([smp], n_space_bins=2, n_time_bins=4,
                              batch_size=6, n_batches=99, s_enhance=2,
                              t_enhance=2, transform=identity_transform)
    assert len(q) == 8
    n_box, n_time = (6 - 4 + 1) * (8 - 4 + 1), 20 - 4 + 1
    for _ in range(2):                           # a second pass starts over
        cells = []
        for i, batch in enumerate(q):
            assert batch.high_res.shape == (6, 4, 4, 4, 2)
            org = smp.last_origins
            sp = {chunk_of(o[0] * 5 + o[1], n_box, 2) for o in org}
            tm = {chunk_of(o[2], n_time, 4) for o in org}
            assert sp == {i // 4} and tm == {i % 4}
            cells.append((i // 4, i % 4))
        assert sorted(cells) == [(a, b) for a in range(2) for b in range(4)]
    assert not q.queue_thread.is_alive()


def test_batch_handler_dc():
    train, val = dc_samplers(2), dc_samplers(1, seed0=7)
    kw = dict(batch_size=6, n_batches=3, s_enhance=2, t_enhance=2,
              transform=identity_transform, seed=0)
    with pytest.raises(AssertionError, match='requires validation data'):
        DeviceBatchHandlerDC(train, None, n_space_bins=2, n_time_bins=2, **kw)
    with pytest.raises(AssertionError, match='requires validation data'):
        DeviceBatchHandlerDC(train, [], n_space_bins=2, n_time_bins=2, **kw)
    with pytest.raises(AssertionError, match='too large'):   # 15 box starts
        DeviceBatchHandlerDC(train, val, n_space_bins=16, n_time_bins=2, **kw)
    with pytest.raises(AssertionError, match='too large'):   # 17 time starts
        DeviceBatchHandlerDC(train, val, n_space_bins=2, n_time_bins=18, **kw)
    bh = DeviceBatchHandlerDC(train, val, n_space_bins=3, n_time_bins=2, **kw)
    assert isinstance(bh.val_data, DeviceValBatchQueueDC)
    assert len(bh.val_data) == 6 and len(bh) == 3
    np.testing.assert_array_equal(bh.spatial_weights, np.ones(3) / 3)
    np.testing.assert_array_equal(bh.temporal_weights, np.ones(2) / 2)
    bh.start()
    assert bh.running and bh.queue_len == 0
    assert not bh.queue_thread.is_alive()        # device-resident samplers
    assert not bh.val_data.queue_thread.is_alive()
    new_s, new_t = np.float32([0, 0, 1]), np.float32([1, 0])
    bh.update_weights(new_s, new_t)
    for _ in bh:
        drawn = train[bh.container_index]
        assert drawn.spatial_weights is new_s
        assert drawn.temporal_weights is new_t
        for o in drawn.last_origins:
            assert chunk_of(o[0] * 5 + o[1], 15, 3) == 2
            assert chunk_of(o[2], 17, 2) == 0
    bh.stop()
    assert not bh.running


def test_device_tensors_pass_through_as_arrays():
    from sup3r_amd.batch_queue import _as_arrays

    class OnDevice:
        is_cuda = True
    a, b = OnDevice(), OnDevice()
    assert _as_arrays(a) is a
    assert _as_arrays((a, b)) == (a, b)
    assert isinstance(_as_arrays([[1.0, 2.0]]), np.ndarray)
    got = _as_arrays((a, [1.0]))
    assert got[0] is a and isinstance(got[1], np.ndarray)


def test_queue_over_resident_samplers_starts_no_thread():
    cube, s = sampler()
    q = DeviceBatchQueue([s], batch_size=4, n_batches=3, s_enhance=1,
                         t_enhance=1, transform=identity_transform, seed=0)
    assert q.device_resident
    rng = np.random.default_rng(3)
    n = 0
    for b in q:
        assert q.running and not q.queue_thread.is_alive() \
            and q.queue_len == 0
        i0, j0 = rng.integers(0, 9 - 4 + 1), rng.integers(0, 11 - 5 + 1)
        k0 = rng.integers(0, 40 - 12 + 1)
        np.testing.assert_array_equal(
            b.high_res[2], cube[i0:i0 + 4, j0:j0 + 5, k0 + 6:k0 + 9])
        n += 1
    q.stop()
    assert n == 3 and not q.running


# --------------------------------------------------------------------- dual
def dual(lr_shape=(6, 7, 20), s=2, te=3, box=(4, 6, 6), batch_size=3, obs=True,
         seed=2, hr_shape=None, feature_sets=None):
    lr = cube_of(lr_shape + (3,), seed=1)
    hr_shape = hr_shape or (lr_shape[0] * s, lr_shape[1] * s, lr_shape[2] * te)
    hr = cube_of(hr_shape + (3,), seed=2)
    ob = hr.copy()
    ob[np.random.default_rng(3).random(ob.shape) < 0.7] = np.nan
    lr_box = (box[0] // s, box[1] // s, box[2] // te)
    logs = {k: [] for k in ('low_res', 'high_res', 'obs')}
    gather = {'low_res': np_gather(lr, lr_box, logs['low_res']),
              'high_res': np_gather(hr, box, logs['high_res']),
              'obs': np_gather(ob, box, logs['obs'])}
    smp = DeviceDualSampler(
        lr, hr, ['u', 'v', 'cape'], ['u', 'v', 'topo'], box,
        batch_size=batch_size, s_enhance=s, t_enhance=te,
        feature_sets=feature_sets or {'lr_only_features': ['cape'],
                                      'hr_exo_features': ['topo']},
        obs=ob if obs else None, seed=seed, gather=gather)
    return smp, (lr, hr, ob), logs


def test_dual_sampler_features_and_members():
    smp, _, _ = dual()
    assert smp.dset_names == ['low_res', 'high_res', 'obs']
    assert smp.features == ['u', 'v', 'cape', 'topo']
    assert smp.lr_features == ['u', 'v', 'cape']
    assert smp.hr_features == ['u', 'v', 'topo']
    assert smp.hr_out_features == ['u', 'v']
    assert smp.lr_sample_shape == (2, 3, 2) and smp.sample_shape == (4, 6, 6)
    assert dual(obs=False)[0].dset_names == ['low_res', 'high_res']
    with pytest.raises(AssertionError, match='not compatible'):
        dual(hr_shape=(12, 14, 59))
    with pytest.raises(AssertionError, match='not compatible'):
        dual(hr_shape=(12, 15, 60))


def test_dual_sampler_origins_and_payload():
    smp, (lr, hr, ob), logs = dual()
    rng = np.random.default_rng(2)
    for _ in range(20):
        low, high, obs = next(smp)
        i0, j0 = rng.integers(0, 6 - 2 + 1), rng.integers(0, 7 - 3 + 1)
        k0 = rng.integers(0, 20 - 3 * 2 + 1)
        np.testing.assert_array_equal(
            smp.last_lr_origins, [(i0, j0, k0 + 2 * m) for m in range(3)])
        np.testing.assert_array_equal(smp.last_origins,
                                      smp.last_lr_origins * (2, 2, 3))
        assert logs['low_res'][-1][1] == [0, 1, 2]
        assert logs['high_res'][-1][1] == [0, 1, 2]
        assert logs['obs'][-1][1] == [0, 1]
        m = 1
        i, j, k = smp.last_origins[m]
        np.testing.assert_array_equal(high[m], hr[i:i + 4, j:j + 6, k:k + 6])
        np.testing.assert_array_equal(
            obs[m].view(np.uint32),
            ob[i:i + 4, j:j + 6, k:k + 6, :2].view(np.uint32))
        i, j, k = smp.last_lr_origins[m]
        np.testing.assert_array_equal(low[m], lr[i:i + 2, j:j + 3, k:k + 2])
    lr_ix, hr_ix, obs_ix = smp.get_sample_index(n_obs=1)
    for a, b, f in zip(lr_ix[:3], hr_ix[:3], (2, 2, 3)):
        assert (b.start, b.stop) == (a.start * f, a.stop * f)
    assert obs_ix[:3] == hr_ix[:3] and obs_ix[3] == ['u', 'v']


def test_dual_queue():
    smp, _, _ = dual()
    with pytest.raises(AssertionError, match='s_enhance'):
        DeviceDualBatchQueue([smp], batch_size=3, s_enhance=1, t_enhance=3)
    with pytest.raises(AssertionError, match='t_enhance'):
        DeviceDualBatchQueue([smp], batch_size=3, s_enhance=2, t_enhance=2)
    q = DeviceDualBatchQueue([smp], batch_size=3, n_batches=2, s_enhance=2,
                             t_enhance=3, seed=0)
    assert q.BATCH_MEMBERS == ('low_res', 'high_res', 'obs')
    assert q.queue_shape == [(3, 2, 3, 2, 3), (3, 4, 6, 6, 3),
                             (3, 4, 6, 6, 2)]
    assert q.shapes == ((3, 2, 3, 2, 3), (3, 4, 6, 6, 3))
    batches = list(q)                            # no smoothing: no device
    assert len(batches) == 2 and not q.queue_thread.is_alive()
    for b in batches:
        assert b.dset_names == ['low_res', 'high_res', 'obs']
        assert b.low_res.shape == (3, 2, 3, 2, 3)
        assert b.high_res.shape == (3, 4, 6, 6, 3)
        assert b.obs.shape == (3, 4, 6, 6, 2) and np.isnan(b.obs).any()
    smooth = DeviceDualBatchQueue(
        [smp], batch_size=3, n_batches=2, s_enhance=2, t_enhance=3,
        transform_kwargs={'smoothing': 0.8, 'smoothing_ignore': []})
    with pytest.raises(NotImplementedError, match='over time'):
        next(iter(smooth))
    bh = DeviceDualBatchHandler([smp], [dual(seed=8)[0]], batch_size=3,
                                n_batches=2, s_enhance=2, t_enhance=3)
    assert isinstance(bh.val_data, DeviceDualBatchQueue)
    assert bh.val_data.BATCH_MEMBERS == ('low_res', 'high_res', 'obs')
    assert set(bh.means) == {'u', 'v', 'cape', 'topo'}


def test_header_declares_the_gather():
    import os
    import re
    from sup3r_amd import _lib
    root = os.path.join(os.path.dirname(__file__), '..')
    with open(os.path.join(root, 'include', 'sup3r_hip.h')) as f:
        header = f.read()
    assert re.search(r'\bint\s+s3_sample_gather\s*\(', header)
    assert 's3_sample_gather' in _lib.EXPORTS
    for name, value in (('ORIGINS', _lib.SAMPLE_MAX_ORIGINS),
                        ('CHANNELS', _lib.SAMPLE_MAX_CHANNELS)):
        assert re.search(rf'#define S3_SAMPLE_MAX_{name} {value}\b', header)
