"""CPU tests of ``DeviceStatsCollection`` and ``from_containers``: the numpy
containers of tests/stats_ref.py stand in for the device samplers, so what is
checked here is the control flow and the float32 arithmetic across containers
— the kernels are in tests/test_stats_gpu.py."""
import json
import warnings

import numpy as np
import pytest

import sup3r_amd
from sup3r_amd import stats as S
from sup3r_amd.batch_queue import (DeviceBatchHandler, _container_kwargs,
                                   _signature_names)
from sup3r_amd.batch_queue_conditional import DeviceBatchHandlerMom1SF
from sup3r_amd.batch_queue_dc import DeviceBatchHandlerDC
from sup3r_amd.batch_queue_dual import (DeviceBatchHandlerCC,
                                        DeviceDualBatchHandler)
from sup3r_amd.samplers import (DeviceDualSampler, DeviceSampler,
                                DeviceSamplerDC)
from sup3r_amd.samplers_cc import DeviceDualSamplerCC
from tests import stats_ref as R

FEATS = ['u_100m', 'v_100m', 'pressure']


def cube(shape, seed, loc=(0., 5., 1e5), scale=(3., 1., 50.)):
    rng = np.random.default_rng(seed)
    c = shape[-1]
    return (rng.standard_normal(shape) * np.array(scale[:c])
            + np.array(loc[:c])).astype(np.float32)


@pytest.fixture()
def cubes():
    return [cube((4, 5, 6, 3), 0), cube((3, 3, 10, 3), 1, loc=(1., 4., 9e4))]


def samplers(cubes, feats=FEATS):
    return [R.NumpySampler(c, feats) for c in cubes]


def test_weights_are_float32_shares_of_the_data(cubes):
    col = S.DeviceStatsCollection(samplers(cubes))
    w = col.container_weights
    assert w.dtype == np.float32
    np.testing.assert_array_equal(
        w, (np.array([360, 270]) / 630).astype(np.float32))
    np.testing.assert_array_equal(w, R.container_weights([360, 270]))


def test_means_and_stds_follow_the_reference_arithmetic(cubes):
    col = S.DeviceStatsCollection(samplers(cubes))
    means, stds = R.collection_stats(cubes)
    assert list(col.means) == FEATS and list(col.stds) == FEATS
    for q, f in enumerate(FEATS):
        assert type(col.means[f]) is np.float32
        assert type(col.stds[f]) is np.float32
        assert col.means[f] == means[q] and col.stds[f] == stds[q]
    # the formula is the reference's: it ignores the spread of the means
    pooled = np.concatenate([c.reshape(-1, 3) for c in cubes])
    assert col.stds['pressure'] < 0.1 * pooled[:, 2].std()


def test_one_read_of_each_cube_feeds_means_and_stds(cubes):
    ss = samplers(cubes)
    S.DeviceStatsCollection(ss)
    assert [s._cube.reads for s in ss] == [1, 1]


def test_containers_are_normalized_in_place(cubes):
    ss = samplers(cubes)
    col = S.DeviceStatsCollection(ss)
    m = [col.means[f] for f in FEATS]
    s = [col.stds[f] for f in FEATS]
    for sampler, c in zip(ss, cubes):
        np.testing.assert_array_equal(sampler.data, R.normalize(c, m, s))


def test_features_are_the_union_in_first_seen_order():
    a = R.NumpySampler(cube((2, 2, 4, 2), 0), ['b', 'a'])
    b = R.NumpySampler(cube((2, 2, 4, 2), 1), ['a', 'b'])
    col = S.DeviceStatsCollection([a, b])
    assert col.features == ['b', 'a']


def test_partial_dicts_only_the_missing_features_are_computed(cubes):
    ss = samplers(cubes)
    given = {'u_100m': 7.0}
    with pytest.warns(UserWarning, match='Not all features'):
        col = S.DeviceStatsCollection(ss, means=given,
                                      stds={'pressure': 2.0})
    means, stds = R.collection_stats(cubes)
    assert col.means is given and col.means['u_100m'] == 7.0
    assert col.means['v_100m'] == means[1] and col.means['pressure'] == means[2]
    assert col.stds['pressure'] == 2.0
    assert col.stds['u_100m'] == stds[0] and col.stds['v_100m'] == stds[1]
    want = R.normalize(cubes[0], [7.0, means[1], means[2]],
                       [stds[0], stds[1], 2.0])
    np.testing.assert_array_equal(ss[0].data, want)


def test_complete_dicts_read_no_cube(cubes):
    ss = samplers(cubes)
    full = {f: 1.0 for f in FEATS}
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        col = S.DeviceStatsCollection(ss, means=dict(full), stds=dict(full))
    assert [s._cube.reads for s in ss] == [0, 0]
    assert col.means == full


def test_json_round_trip_and_rewrite_on_added_features(cubes, tmp_path):
    mp, sp = str(tmp_path / 'means.json'), str(tmp_path / 'stds.json')
    col = S.DeviceStatsCollection(samplers(cubes), means=mp, stds=sp)
    on_file = json.load(open(mp))
    assert on_file == {f: float(col.means[f]) for f in FEATS}
    assert all(type(v) is float for v in on_file.values())
    assert json.load(open(sp)) == {f: float(col.stds[f]) for f in FEATS}
    # second run: everything comes from the files, nothing is read or written
    ss = samplers(cubes)
    stamp = open(mp).read()
    col2 = S.DeviceStatsCollection(ss, means=mp, stds=sp)
    assert [s._cube.reads for s in ss] == [0, 0]
    assert col2.means == on_file and open(mp).read() == stamp
    # a file from a run with fewer features: warned about, completed, rewritten
    json.dump({'u_100m': 0.5}, open(mp, 'w'))
    with pytest.warns(UserWarning, match='Not all features'):
        col3 = S.DeviceStatsCollection(samplers(cubes), means=mp, stds=sp)
    again = json.load(open(mp))
    assert again['u_100m'] == 0.5 and set(again) == set(FEATS)
    assert again['pressure'] == float(col3.means['pressure'])


def test_other_types_are_an_assertion(cubes):
    with pytest.raises(AssertionError, match='Received incompatible type'):
        S.DeviceStatsCollection(samplers(cubes), means=[1.0, 2.0, 3.0])


def test_all_nan_feature_is_nan_with_a_warning(cubes):
    cubes[0][..., 1] = np.nan
    cubes[1][..., 1] = np.nan
    with pytest.warns(UserWarning, match='holds no value'):
        col = S.DeviceStatsCollection(samplers(cubes))
    assert np.isnan(col.means['v_100m']) and np.isnan(col.stds['v_100m'])
    assert np.isfinite(col.means['u_100m'])


# ------------------------------------------------------------- dual samplers
def dual_sampler(with_obs=True, seed=0):
    """a DeviceDualSampler with stand-in gathers whose cubes are replaced by
    numpy cubes: the split and the member loop run as on the device"""
    lr = cube((3, 3, 4, 2), seed, loc=(0., 300.), scale=(2., 10.))
    hr = cube((6, 6, 8, 2), seed + 1, loc=(1., 50.), scale=(4., 5.))
    obs = hr.copy()
    obs[::2, :, :, 0] = np.nan
    gather = {k: (lambda org, ch: None) for k in ('low_res', 'high_res', 'obs')}
    s = DeviceDualSampler(lr, hr, ['u', 'temperature'], ['u', 'topography'],
                          sample_shape=(4, 4, 2), batch_size=2, s_enhance=2,
                          t_enhance=2, obs=obs if with_obs else None,
                          gather=gather,
                          feature_sets={'hr_exo_features': ['topography']})
    s._lr = R.NumpyCube(lr, ['u', 'temperature'])
    s._hr = s._cube = R.NumpyCube(hr, ['u', 'topography'])
    if with_obs:
        s._obs = R.NumpyCube(obs, ['u', 'topography'])
    return s, lr, hr, obs


def test_dual_split_high_res_first_then_low_res():
    s, lr, hr, _ = dual_sampler()
    assert s.features == ['u', 'temperature', 'topography']
    got = s.channel_moments(['u', 'temperature', 'topography'])
    n_hr, m_hr, s_hr = R.nan_moments(hr)
    n_lr, m_lr, s_lr = R.nan_moments(lr)
    assert got['u'] == (n_hr[0], m_hr[0], s_hr[0])              # not low_res'
    assert got['topography'] == (n_hr[1], m_hr[1], s_hr[1])
    assert got['temperature'] == (n_lr[1], m_lr[1], s_lr[1])
    assert s._obs.reads == 0


def test_dual_normalize_covers_every_member_obs_included():
    s, lr, hr, obs = dual_sampler()
    col = S.DeviceStatsCollection([s])
    m, sd = col.means, col.stds
    want_lr = R.normalize(lr, [m['u'], m['temperature']],
                          [sd['u'], sd['temperature']])
    want_hr = R.normalize(hr, [m['u'], m['topography']],
                          [sd['u'], sd['topography']])
    want_obs = R.normalize(obs, [m['u'], m['topography']],
                           [sd['u'], sd['topography']])
    np.testing.assert_array_equal(s._lr.data, want_lr)
    np.testing.assert_array_equal(s._hr.data, want_hr)
    np.testing.assert_array_equal(s._obs.data, want_obs)
    assert np.isnan(s._obs.data[::2, :, :, 0]).all()


def test_features_in_only_one_dict_are_left_alone():
    s, lr, hr, _ = dual_sampler(with_obs=False)
    s.normalize({'u': 1.0, 'temperature': 2.0}, {'u': 2.0, 'topography': 4.0})
    np.testing.assert_array_equal(s._lr.data[..., 1], lr[..., 1])
    np.testing.assert_array_equal(s._hr.data[..., 1], hr[..., 1])
    np.testing.assert_array_equal(s._lr.data[..., 0],
                                  (lr[..., 0] - np.float32(1)) / np.float32(2))
    np.testing.assert_array_equal(s._hr.data[..., 0],
                                  (hr[..., 0] - np.float32(1)) / np.float32(2))


def test_stand_in_cubes_refuse_statistics():
    s = DeviceSampler(np.zeros((4, 4, 4, 1), np.float32), ['a'],
                      sample_shape=(2, 2, 1), batch_size=2,
                      gather=lambda org, ch: None)
    with pytest.raises(RuntimeError, match='needs the cube on the device'):
        s.channel_moments(['a'])
    with pytest.raises(RuntimeError, match='needs the cube on the device'):
        s.normalize({'a': 0.0}, {'a': 1.0})
    s.normalize({'b': 0.0}, {'b': 1.0})           # nothing to do: no pass


# ------------------------------------------------------------ from_containers
class NumpyHandler(DeviceBatchHandler):
    SAMPLER = R.NumpySampler


def identity_transform(samples, **kwargs):
    return samples, samples


def test_from_containers_normalizes_val_with_the_training_stats(cubes):
    val = cube((3, 4, 5, 3), 9, loc=(2., 2., 8e4))
    train = [{'data': c, 'features': FEATS} for c in cubes]

    class Obj:
        data, features = val, FEATS
    bh = NumpyHandler.from_containers(
        train, [Obj()], sample_shape=(2, 2, 1), batch_size=2, n_batches=3,
        transform=identity_transform, seed=4)
    means, stds = R.collection_stats(cubes)
    assert [bh.means[f] for f in FEATS] == list(means)
    assert [bh.stds[f] for f in FEATS] == list(stds)
    for sampler, c in zip(bh.containers, cubes):
        np.testing.assert_array_equal(sampler.data,
                                      R.normalize(c, means, stds))
    assert len(bh.val_data.containers) == 1
    np.testing.assert_array_equal(bh.val_data.containers[0].data,
                                  R.normalize(val, means, stds))
    assert bh.n_batches == 3 and bh.val_data.n_batches == 3
    # kwargs went where their names are taken: seed to the sampler AND the
    # queues, transform to the queues only
    assert bh.containers[0].seed == 4
    assert bh._transform is identity_transform
    assert bh.val_data._transform is identity_transform
    batch = next(iter(bh))
    assert batch.high_res.shape == (2, 2, 2, 3)


def test_from_containers_takes_given_stats_and_no_val(cubes):
    full = {f: 2.0 for f in FEATS}
    bh = NumpyHandler.from_containers(
        [{'data': cubes[0], 'features': FEATS}], sample_shape=(2, 2, 1),
        batch_size=2, means=dict(full), stds=dict(full),
        transform=identity_transform)
    assert bh.val_data == [] and bh.means == full
    np.testing.assert_array_equal(
        bh.containers[0].data, R.normalize(cubes[0], [2.] * 3, [2.] * 3))


def test_bad_kwargs_message(cubes):
    with pytest.raises(AssertionError) as err:
        NumpyHandler.from_containers(
            [{'data': cubes[0], 'features': FEATS}], sample_shape=(2, 2, 1),
            batch_size=2, n_space_bins=2, bogus=1)
    msg = str(err.value)
    assert msg.startswith('NumpyHandler received bad kwargs = ')
    assert "'bogus'" in msg and "'n_space_bins'" in msg


def test_kwargs_routing_by_signature():
    dc = _signature_names(DeviceBatchHandlerDC)
    assert {'n_space_bins', 'n_time_bins', 'seed', 'transform'} <= dc
    assert {'spatial_weights', 'temporal_weights', 'seed', 'device',
            'gather'} <= _signature_names(DeviceSamplerDC)
    assert 'n_space_bins' not in _signature_names(DeviceSamplerDC)
    assert {'s_enhance', 't_enhance'} <= _signature_names(DeviceDualSampler)
    mom = _signature_names(DeviceBatchHandlerMom1SF)
    assert {'time_enhance_mode', 's_padding', 'lower_models'} <= mom
    # data keywords, samplers and stats are not kwargs
    for names in (dc, mom, _signature_names(DeviceDualSampler)):
        assert not names & {'self', 'samplers', 'train_samplers', 'means',
                            'data', 'features', 'low_res', 'obs'}


def test_sampler_classes_and_container_keywords():
    assert DeviceBatchHandler.SAMPLER is DeviceSampler
    assert DeviceBatchHandlerDC.SAMPLER is DeviceSamplerDC
    assert DeviceDualBatchHandler.SAMPLER is DeviceDualSampler
    assert DeviceBatchHandlerCC.SAMPLER is DeviceDualSamplerCC
    assert DeviceBatchHandlerMom1SF.SAMPLER is DeviceSampler
    dual = {'low_res': 1, 'high_res': 2, 'lr_features': 3, 'hr_features': 4}
    assert _container_kwargs(dual, DeviceDualSampler) == dual
    assert _container_kwargs({**dual, 'obs': 5, 'other': 6},
                             DeviceDualSampler) == {**dual, 'obs': 5}
    cc = {'daily': 1, 'hourly': 2, 'lr_features': 3, 'hr_features': 4}
    assert _container_kwargs(cc, DeviceDualSamplerCC) == cc

    class Deriver:                       # the DeviceDeriver surface
        data, features = 'not the cube', ['a']

        def as_array(self):
            return 'cube'
    assert _container_kwargs(Deriver(), DeviceSampler) == {
        'data': 'cube', 'features': ['a']}
    with pytest.raises(KeyError):
        _container_kwargs({'data': 1}, DeviceSampler)


def test_new_names_are_exported():
    for name in S.__all__:
        assert name in sup3r_amd.__all__ and hasattr(sup3r_amd, name)
    assert sup3r_amd.StatsCollection is S.DeviceStatsCollection
    for name in ('channel_moments', 'normalize_channels'):
        assert name in sup3r_amd.__all__ and hasattr(sup3r_amd, name)
    assert hasattr(sup3r_amd.DeviceBatchHandler, 'from_containers')


def test_abi_names_and_limits():
    import os
    import re
    from sup3r_amd import _lib
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include',
                               'sup3r_hip.h')).read()
    for name in ('s3_channel_moments', 's3_normalize_channels'):
        assert re.search(r'\bint\s+' + name + r'\s*\(', header)
        assert name in _lib.EXPORTS
    assert re.search(r'#define\s+S3_STATS_MAX_CHANNELS\s+%d\b'
                     % _lib.STATS_MAX_CHANNELS, header)
    assert _lib.STATS_MAX_CHANNELS >= _lib.SAMPLE_MAX_CHANNELS


def test_sum_of_squares_misses_one_ulp_in_the_offset_case():
    """the offset case of the GPU tests discriminates: float64 sum(x^2)
    misses the float32 ulp that the two-pass float64 reference defines"""
    rng = np.random.default_rng(11)
    n = 65 * 4097
    x = np.stack([1e5 + 0.1 * rng.standard_normal(n),
                  -3e4 + 1e-2 * rng.standard_normal(n)],
                 axis=1).astype(np.float32)
    _, _, std = R.nan_moments(x)
    _, bad = R.sumsq_moments(x)
    assert max(R.ulp_distance(bad[q], std[q]) for q in range(2)) > 1
