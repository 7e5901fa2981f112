"""CPU tests of ``sup3r_amd.derive`` with ``NumpyBackend``: the host control
flow of ``DeviceDeriver`` (registry lookup, alias recursion, "derive the
missing inputs first", the fall-through to level interpolation, the launch
plan, roll / coarsen / NaN mask) and the selection rule of
``s3_level_interp`` as ``_select_levels`` states it, against the ``numpy.ma``
restatement of the reference in ``tests/derive_ref.py`` (unverified against
dask, see there).  The procedures of the reference's
tests/derivers/test_height_interp.py, test_single_level.py and
test_derive_features.py are followed on arrays."""
import json
import os
import warnings

import numpy as np
import pandas as pd
import pytest
from scipy.interpolate import interp1d

from sup3r_amd import derive as D
from tests import derive_ref as R

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden',
                      'deriver_registries.json')


def _deriver(arrays, ll, ti, features, **kw):
    data = D.DeriveData(arrays, ll, ti, **{k: kw.pop(k) for k in
                                           ('level', 'height', 'attrs')
                                           if k in kw})
    return D.DeviceDeriver(data, features, backend=D.NumpyBackend(), **kw)


def _fake(shape=(10, 10, 20), n_lev=3, seed=1, names=('u',)):
    """the shapes of make_fake_nc_file in the reference's tests"""
    arrays, ll, ti = R.era5_like(seed, shape, n_lev)
    arrays = {k: v for k, v in arrays.items()
              if k in ('zg', 'topography') + tuple(names)}
    return arrays, ll, ti


# ------------------------------------------------------------ names, registry
def test_parse_feature():
    f = D.parse_feature('u_100m')
    assert (f.basename, f.height, f.pressure) == ('u', 100, None)
    f = D.parse_feature('temperature_max_500pa')
    assert (f.basename, f.height, f.pressure) == ('temperature_max', None, 500)
    assert f.map_wildcard('ta_(.*)') == 'ta_500pa'
    assert D.parse_feature('v_40m').map_wildcard('va_(.*)') == 'va_40m'
    assert D.parse_feature('topography').map_wildcard('x_(.*)') == 'x'
    assert D.parse_feature('u_10m').map_wildcard('uas') == 'uas'
    assert D.get_feature_basename('relativehumidity_2m') == 'relativehumidity'


def test_registries_match_the_reference_names():
    with open(GOLDEN) as f:
        golden = json.load(f)
    for name, want in golden.items():
        reg = getattr(D, name)
        assert list(reg) == list(want), name
        for key, val in want.items():
            got = reg[key]
            got = '=' + got if isinstance(got, str) else got.__name__
            assert got == val, (name, key)
    import sup3r_amd
    for name in D.__all__:
        assert name in sup3r_amd.__all__ and hasattr(sup3r_amd, name)


def test_inputs_of_the_classes():
    assert D.UWind.inputs == ('windspeed_(.*)', 'winddirection_(.*)')
    assert D.Windspeed.inputs == D.Winddirection.inputs == ('u_(.*)', 'v_(.*)')
    assert D.CloudMask.inputs == ('ghi', 'clearky_ghi')
    assert D.USolar.inputs == D.VSolar.inputs == ('wind_speed',
                                                  'wind_direction')
    assert D.TasMin.inputs == ('tasmin',) and D.TasMax.inputs == ('tasmax',)
    assert D.UWindPowerLaw.inputs == ('uas',)
    assert D.VWindPowerLaw.inputs == ('vas',)
    assert D.Sza.inputs == () and D.Latitude.inputs == ()


# --------------------------------------------------------- the selection rule
@pytest.mark.parametrize('L', [1, 2, 3, 5, 8])
def test_selection_rule_against_numpy_ma(L):
    """duplicates, NaN levels (also at index 0, also whole columns), targets
    below, above and equal to levels: linear results bit for bit"""
    rng = np.random.default_rng(L)
    P = 1500
    lev = rng.integers(0, 12, (P, L)).astype(np.float32) * 10
    lev[rng.random((P, L)) < 0.15] = np.nan
    lev[:20] = np.nan
    var = rng.normal(size=(P, L)).astype(np.float32)
    var[rng.random((P, L)) < 0.05] = np.nan
    be = D.NumpyBackend()
    for target in (-5.0, 0.0, 30.0, 35.0, 115.0):
        ref = R.interp_to_level(lev, var, np.float32(target))
        got = be.level_interp(('column', lev.reshape(P, 1, 1, L), None),
                              [var.reshape(P, 1, 1, L)], [], [],
                              [target])[0][0].reshape(P)
        assert got.dtype == np.float32 and ref.dtype == np.float32
        # (bit for bit where a number comes out; NaN where NaN does: the
        # sign and payload of a NaN are not numpy's to promise)
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got), nan), target
        assert np.array_equal(got[~nan].view(np.int32),
                              ref[~nan].view(np.int32)), target


# ------------------------------------------- test_height_interp.py, on arrays
@pytest.mark.parametrize('height', [20, 2, 1000, 0])
def test_plevel_height_interp(height):
    arrays, ll, ti = _fake()
    with pytest.warns(match='Received some upper case features'):
        dv = _deriver(arrays, ll, ti, [f'U_{height}m'],
                      interp_kwargs={'method': 'linear'})
    out = R.interp_to_level(R.height_array(arrays), arrays['u'],
                            np.float32(height))
    assert dv[f'u_{height}m'].dtype == np.float32
    assert np.array_equal(out, dv[f'u_{height}m'])


def test_plevel_height_interp_and_derivation():
    arrays, ll, ti = _fake(names=('u', 'v'))
    ws = _deriver(dict(arrays), ll, ti, ['windspeed_20m'])['windspeed_20m']
    uv = _deriver(dict(arrays), ll, ti, ['u_20m', 'v_20m'])
    assert np.allclose(ws, np.hypot(uv['u_20m'], uv['v_20m']), atol=1e-4)


def test_plevel_height_interp_with_filtered_load_features():
    arrays, ll, ti = R.era5_like(2, (10, 10, 20), 3)
    arrays.pop('v')
    no_sfc = {k: v for k, v in arrays.items() if k != 'u_10m'}
    filt = _deriver(dict(no_sfc), ll, ti, ['u_20m'])
    no_filt = _deriver(dict(arrays), ll, ti, ['u_20m'])
    assert np.array_equal(
        filt['u_20m'], R.interp_to_level(R.height_array(arrays), arrays['u'],
                                         np.float32(20)))
    assert not np.array_equal(filt['u_20m'], no_filt['u_20m'])


def test_only_interp_method():
    hgt = np.zeros((10, 10, 5, 3), np.float32)
    ws = np.zeros((10, 10, 5, 3), np.float32)
    hgt[..., 0], hgt[..., 1], hgt[..., 2] = 10, 40, 100
    ws[..., 0], ws[..., 1], ws[..., 2] = 5, 8, 12
    be = D.NumpyBackend()
    for level in (50, 60):
        out = be.level_interp(('column', hgt, None), [ws], [], [],
                              [level])[0][0]
        func = interp1d(hgt[0, 0, 0], ws[0, 0, 0], fill_value='extrapolate')
        assert np.allclose(out, func(level))
        assert np.allclose(R.interp_to_level(hgt, ws, level), func(level))


def test_single_levels_height_interp():
    rng = np.random.default_rng(3)
    shape = (10, 10, 20)
    arrays = {'u_10m': rng.normal(size=shape).astype(np.float32),
              'u_100m': rng.normal(size=shape).astype(np.float32)}
    ti = pd.date_range('2020-01-01', periods=20, freq='h')
    dv = _deriver(dict(arrays), R.grid(10, 10), ti, ['u_30m'],
                  interp_kwargs={'method': 'linear'})
    hgt = np.zeros((*shape, 2), np.float32)
    hgt[..., 0], hgt[..., 1] = 10, 100
    u = np.stack([arrays['u_10m'], arrays['u_100m']], axis=-1)
    out = R.interp_to_level(hgt, u, np.float32(30))
    assert dv['u_30m'].dtype == np.float32
    assert np.array_equal(out, dv['u_30m'])


def _with_single_levels(arrays, names):
    hgt = R.height_array(arrays)
    levs = [np.full((*hgt.shape[:-1], 1), D.parse_feature(n).height,
                    np.float32) for n in names]
    u = np.concatenate([arrays['u']] + [arrays[n][..., None] for n in names],
                       axis=-1)
    return np.concatenate([hgt] + levs, axis=-1), u


def test_plevel_height_interp_with_single_lev_data():
    arrays, ll, ti = R.era5_like(4, (10, 10, 20), 3)
    arrays.pop('v')
    dv = _deriver(dict(arrays), ll, ti, ['u_100m'])
    hgt, u = _with_single_levels(arrays, ['u_10m'])
    out = R.interp_to_level(hgt, u, np.float32(100))
    assert dv['u_100m'].dtype == np.float32
    assert np.array_equal(out, dv['u_100m'])


def test_log_interp():
    arrays, ll, ti = R.era5_like(5, (10, 10, 20), 3)
    arrays.pop('v')
    arrays['u_100m'] = np.random.default_rng(6).normal(
        size=(10, 10, 20)).astype(np.float32)
    dv = _deriver(dict(arrays), ll, ti, ['u_40m'],
                  interp_kwargs={'method': 'log'})
    hgt, u = _with_single_levels(arrays, ['u_10m', 'u_100m'])
    out = R.interp_to_level(hgt, u, np.float32(40), method='log')
    assert dv['u_40m'].dtype == np.float32
    assert np.array_equal(np.asarray(out), np.asarray(dv['u_40m']))


# --------------------------------------------- test_single_level.py, on arrays
def _wswd(shape=(10, 10, 12), seed=7, flip=False):
    rng = np.random.default_rng(seed)
    arrays = {'windspeed_100m': rng.uniform(0, 20, shape).astype(np.float32),
              'winddirection_100m': rng.uniform(0, 360, shape).astype(
                  np.float32)}
    ti = pd.date_range('2020-01-01', periods=shape[2], freq='h')
    return arrays, R.grid(shape[0], shape[1], flip), ti


def test_unneeded_uv_transform():
    rng = np.random.default_rng(8)
    arrays = {'u_100m': rng.normal(size=(10, 10, 12)).astype(np.float32),
              'v_100m': rng.normal(size=(10, 10, 12)).astype(np.float32)}
    ti = pd.date_range('2020-01-01', periods=12, freq='h')
    with pytest.warns(match='Received some upper case features'):
        dv = _deriver(dict(arrays), R.grid(10, 10), ti, ['U_100m', 'V_100m'])
    assert dv.launch_plan == []
    assert np.array_equal(arrays['u_100m'], dv['U_100m'])
    assert np.array_equal(arrays['v_100m'], dv['V_100m'])


@pytest.mark.parametrize('flip', [False, True])
def test_uv_transform(flip):
    arrays, ll, ti = _wswd(flip=flip)
    with pytest.warns(match='Received some upper case features'):
        dv = _deriver(dict(arrays), ll, ti, ['U_100m', 'V_100m'])
    u, v = R.transform_rotate_wind(arrays['windspeed_100m'],
                                   arrays['winddirection_100m'], ll)
    assert np.array_equal(u.astype(np.float32), dv['U_100m'])
    assert np.array_equal(v.astype(np.float32), dv['V_100m'])
    # ... and back
    back = _deriver({'u_100m': dv['u_100m'], 'v_100m': dv['v_100m']}, ll, ti,
                    ['windspeed_100m', 'winddirection_100m'])
    assert np.allclose(back['windspeed_100m'], arrays['windspeed_100m'],
                       atol=1e-4)


@pytest.mark.parametrize('shape', [(20, 20), (11, 10)])
def test_hr_coarsening(shape):
    arrays, ll, ti = _wswd((*shape, 6))
    feats = ['windspeed_100m', 'winddirection_100m']
    dv = _deriver(dict(arrays), ll, ti, feats, hr_spatial_coarsen=2)
    assert dv.as_array().shape == (shape[0] // 2, shape[1] // 2, 6, 2)
    assert dv.shape == (shape[0] // 2, shape[1] // 2, 6, 2)
    assert dv.lat_lon.shape == (shape[0] // 2, shape[1] // 2, 2)
    assert ll.shape == (shape[0], shape[1], 2)
    assert dv.as_array().dtype == np.dtype(np.float32)
    s1 = shape[0] - shape[0] % 2
    want = arrays['windspeed_100m'][:s1].reshape(
        s1 // 2, 2, shape[1] // 2, 2, 6).mean(axis=(1, 3))
    assert np.allclose(dv['windspeed_100m'], want, rtol=1e-6)
    assert np.allclose(dv.lat_lon[0, 0], ll[:2, :2].mean(axis=(0, 1)))


# ------------------------------------------- test_derive_features.py, on arrays
@pytest.mark.parametrize('feature', [
    'windspeed_100m', 'winddirection_100m', 'latitude_feature',
    'longitude_feature', 'soy_encoding', 'sod_encoding'])
def test_derive_feature(feature):
    rng = np.random.default_rng(9)
    shape = (20, 20, 5)
    arrays = {'u_100m': rng.normal(size=shape).astype(np.float32),
              'v_100m': rng.normal(size=shape).astype(np.float32)}
    ll = R.grid(20, 20)
    ti = pd.date_range('2013-06-30 22:30', periods=5, freq='37min')
    dv = _deriver(arrays, ll, ti, [feature])
    assert dv.as_array().shape == (20, 20, 5, 1)
    got = dv[feature]
    if feature == 'latitude_feature':
        want = np.repeat(ll[..., 0][..., None], 5, axis=-1)
    elif feature == 'longitude_feature':
        want = np.repeat(ll[..., 1][..., None], 5, axis=-1)
    elif feature.endswith('encoding'):
        want = np.broadcast_to(R.time_encoding(ti, feature[:3]), shape)
    else:
        ws, wd = R.invert_uv(arrays['u_100m'], arrays['v_100m'], ll)
        want = (ws if feature.startswith('windspeed') else wd).astype(
            np.float32)
    assert np.array_equal(got, want)


# ------------------------------------------------------------- control flow
def _gcm(seed=10, shape=(6, 5, 8)):
    rng = np.random.default_rng(seed)
    arrays = {'uas': rng.normal(0, 5, shape), 'vas': rng.normal(0, 5, shape),
              'tas': rng.uniform(250, 310, shape),
              'rsds': rng.uniform(-5, 400, shape),
              'clearsky_ghi': rng.uniform(0, 350, shape),
              'hurs': rng.uniform(0, 100, shape)}
    arrays = {k: v.astype(np.float32) for k, v in arrays.items()}
    ti = pd.date_range('2050-01-01', periods=shape[2], freq='D')
    return arrays, R.grid(shape[0], shape[1]), ti


def test_alias_recursion():
    rng = np.random.default_rng(11)
    shape = (4, 5, 6)
    ua = rng.normal(size=shape).astype(np.float32)
    ti = pd.date_range('2050-01-01', periods=6, freq='D')
    dv = _deriver({'ua_100m': ua, 'hurs': ua + 1}, R.grid(4, 5), ti,
                  ['u_100m', 'relativehumidity_2m'],
                  FeatureRegistry=D.RegistryNCforCC)
    assert np.array_equal(dv['u_100m'], ua)
    assert np.array_equal(dv['relativehumidity_2m'], ua + 1)
    assert dv.map_new_name('pressure_500pa', 'level_(.*)') == 'level_500pa'
    assert dv.map_new_name('u_40m', 'ua_(.*)') == 'ua_40m'
    assert dv.map_new_name('windspeed', 'wind_speed') == 'wind_speed'
    # pressure_500pa -> level_500pa -> the level coordinate, interpolated
    level = np.array([1000, 850, 500, 250], np.float32)
    dv = _deriver({'ua_100m': ua}, R.grid(4, 5), ti, ['pressure_500pa'],
                  FeatureRegistry=D.RegistryNCforCC, level=level)
    assert np.array_equal(dv['pressure_500pa'],
                          np.full(shape, 500, np.float32))


def test_gcm_registry_with_power_law():
    arrays, ll, ti = _gcm()
    feats = ['u_100m', 'v_100m', 'temperature_2m', 'clearsky_ratio',
             'relativehumidity_2m']
    dv = _deriver(dict(arrays), ll, ti, feats,
                  FeatureRegistry=D.RegistryNCforCCwithPowerLaw)
    assert np.array_equal(dv['u_100m'], R.power_law(arrays['uas'], 100))
    assert np.array_equal(dv['v_100m'], R.power_law(arrays['vas'], 100))
    assert np.array_equal(dv['temperature_2m'], R.to_celsius(arrays['tas']))
    assert dv.data.attrs['tas']['units'] == 'C'
    assert np.array_equal(dv['clearsky_ratio'], R.clearsky_ratio_cc(
        arrays['rsds'], arrays['clearsky_ghi']), equal_nan=True)
    assert np.array_equal(dv['relativehumidity_2m'], arrays['hurs'])
    # Celsius input is left alone
    dv = _deriver({'tas': arrays['tas']}, ll, ti, ['temperature_2m'],
                  FeatureRegistry=D.RegistryNCforCC,
                  attrs={'tas': {'units': 'C'}})
    assert np.array_equal(dv['temperature_2m'], arrays['tas'])


def test_nsrdb_registry():
    rng = np.random.default_rng(12)
    shape = (5, 4, 24)
    cs = np.clip(400 * np.sin(np.linspace(-1, 4, 24)), 0, None)
    cs = np.round(np.broadcast_to(cs, shape) * rng.uniform(
        0.9, 1, shape)).astype(np.float32)
    arrays = {'ghi': (cs * rng.uniform(0, 1, shape)).astype(np.float32),
              'clearsky_ghi': cs,
              'wind_speed': rng.uniform(0, 10, shape).astype(np.float32),
              'wind_direction': rng.uniform(0, 360, shape).astype(np.float32),
              'air_temperature': rng.normal(size=shape).astype(np.float32)}
    ll = R.grid(5, 4)
    ti = pd.date_range('2018-01-01', periods=24, freq='h')
    dv = _deriver(dict(arrays), ll, ti, ['clearsky_ratio', 'U', 'V',
                                          'windspeed', 'air_temperature'],
                  FeatureRegistry=D.RegistryH5SolarCC)
    want = R.clearsky_ratio(arrays['ghi'], cs)
    assert np.isnan(want).any() and not np.isnan(want).all()
    assert np.array_equal(dv['clearsky_ratio'], want, equal_nan=True)
    u, v = R.transform_rotate_wind(arrays['wind_speed'],
                                   arrays['wind_direction'], ll)
    assert np.array_equal(dv['u'], u.astype(np.float32))
    assert np.array_equal(dv['v'], v.astype(np.float32))
    assert np.array_equal(dv['windspeed'], arrays['wind_speed'])
    got = D.CloudMask.compute(D.DeriveData(arrays, ll, ti,
                                           backend=D.NumpyBackend()))
    assert np.array_equal(got, R.cloud_mask(arrays['ghi'], cs), equal_nan=True)


def test_inputs_that_name_the_feature_fall_through_to_interpolation():
    """RegistryBase: u_20m <- windspeed_20m <- u_20m: no compute method can
    run, the multi-level ``u`` is interpolated instead"""
    arrays, ll, ti = _fake()
    dv = _deriver(arrays, ll, ti, ['u_20m'])
    assert not dv.no_overlap('windspeed_20m')
    assert dv.check_registry('u_20m') is None
    assert [g.variables for g in dv.launch_plan] == [['u']]


def test_underivable_feature():
    arrays, ll, ti = _fake()
    with pytest.raises(RuntimeError, match='Could not find "dewpoint_2m"'):
        _deriver(arrays, ll, ti, ['dewpoint_2m'])
    with pytest.raises(RuntimeError, match='Could not find'):
        _deriver(arrays, ll, ti, ['cloud_mask'])     # 'clearky_ghi'


def test_sza_raises():
    arrays, ll, ti = _fake()
    with pytest.raises(NotImplementedError, match='rex'):
        _deriver(arrays, ll, ti, ['sza'])


def test_user_registry():
    class Double(D.DerivedFeature):
        inputs = ('u_(.*)',)

        @classmethod
        def compute(cls, data, height):
            return 2 * np.asarray(data[f'u_{height}m'])

    arrays, ll, ti = _fake()
    dv = _deriver(arrays, ll, ti, ['gust_20m'],
                  FeatureRegistry={**D.RegistryBase, 'gust_(.*)': Double})
    want = R.interp_to_level(R.height_array(arrays), arrays['u'],
                             np.float32(20))
    assert np.array_equal(dv['gust_20m'], 2 * want)
    assert dv.features == ['gust_20m']


# ------------------------------------------------------------------ the plan
def test_launch_plan_groups():
    arrays, ll, ti = R.era5_like(13)
    arrays.pop('u_10m')
    feats = [f'{v}_{h}m' for h in (40, 80, 120) for v in 'uv']
    dv = _deriver(dict(arrays), ll, ti, feats)
    assert len(dv.launch_plan) == 1
    g = dv.launch_plan[0]
    assert g.variables == ['u', 'v'] and g.targets == [40, 80, 120]
    assert g.source == 'zg - topography' and g.companions == ()
    hgt = R.height_array(arrays)
    for f in feats:
        want = R.interp_to_level(hgt, arrays[f[0]],
                                 np.float32(D.parse_feature(f).height))
        assert np.array_equal(dv[f], want), f
    # only u has a single-level companion: two level structures
    arrays, ll, ti = R.era5_like(13)
    dv = _deriver(dict(arrays), ll, ti, feats)
    assert [(g.variables, g.companions) for g in dv.launch_plan] == [
        (['u'], (10.0,)), (['v'], ())]
    hgt_u, u = _with_single_levels(arrays, ['u_10m'])
    assert np.array_equal(dv['u_40m'],
                          R.interp_to_level(hgt_u, u, np.float32(40)))
    assert np.array_equal(dv['v_40m'],
                          R.interp_to_level(hgt, arrays['v'], np.float32(40)))


def test_pairs_share_one_computation():
    arrays, ll, ti = _wswd()
    calls = []

    class Counting(D.NumpyBackend):
        def uv_from_wswd(self, *a):
            calls.append(1)
            return super().uv_from_wswd(*a)

    data = D.DeriveData(arrays, ll, ti)
    D.DeviceDeriver(data, ['u_100m', 'v_100m'], backend=Counting())
    assert len(calls) == 1


def test_pressure_and_height_coordinates():
    rng = np.random.default_rng(14)
    shape, level = (4, 3, 5), np.array([1000, 850, 700, 500], np.float32)
    u = rng.normal(size=(*shape, 4)).astype(np.float32)
    ti = pd.date_range('2020-01-01', periods=5, freq='h')
    dv = _deriver({'u': u}, R.grid(4, 3), ti, ['u_800pa'], level=level)
    want = R.interp_to_level(np.broadcast_to(level, u.shape), u,
                             np.float32(800))
    assert np.array_equal(dv['u_800pa'], want)
    assert dv.launch_plan[0].source == 'level'
    height = np.array([10, 50, 120, 300], np.float32)
    dv = _deriver({'u': u}, R.grid(4, 3), ti, ['u_80m'], height=height)
    want = R.interp_to_level(np.broadcast_to(height, u.shape), u,
                             np.float32(80))
    assert np.array_equal(dv['u_80m'], want)
    with pytest.raises(AssertionError, match='"zg" and "topography"'):
        _deriver({'u': u}, R.grid(4, 3), ti, ['u_80m'])


def test_level_check_and_nan_warnings():
    arrays, ll, ti = _fake()
    with pytest.warns(match='were greater than the minimum requested level'):
        _deriver(dict(arrays), ll, ti, ['u_1m'],
                 interp_kwargs={'run_level_check': True})
    with pytest.warns(match='were lower than the maximum requested level'):
        _deriver(dict(arrays), ll, ti, ['u_5000m'],
                 interp_kwargs={'run_level_check': True})
    bad = dict(arrays)
    bad['zg'] = arrays['zg'].copy()
    bad['zg'][0, 0, 0, 1] = np.nan
    with pytest.warns(match='NaN values found in the interpolation level'):
        _deriver(bad, ll, ti, ['u_20m'])
    bad = dict(arrays)
    bad['u'] = arrays['u'].copy()
    bad['u'][:] = np.nan
    with pytest.warns(match='NaN values found in the interpolation variable'):
        with pytest.raises(AssertionError, match='interpolated output'):
            _deriver(bad, ll, ti, ['u_20m'])


# ------------------------------------------------------- after the derivation
@pytest.mark.parametrize('roll', [0, 1, 5, -1, 9])
def test_time_roll(roll):
    arrays, ll, ti = _wswd((4, 5, 6))
    feats = ['windspeed_100m', 'u_100m']
    dv = _deriver(dict(arrays), ll, ti, feats, time_roll=roll,
                  time_shift=-30)
    plain = _deriver(dict(arrays), ll, ti, feats)
    assert np.array_equal(dv.as_array(),
                          np.roll(plain.as_array(), roll, axis=2))
    assert np.array_equal(dv['u_100m'], np.roll(plain['u_100m'], roll, axis=2))
    assert dv.time_index.equals(ti.shift(-30, freq='min'))
    assert np.array_equal(plain.as_array(['u_100m', 'windspeed_100m']),
                          plain.as_array()[..., ::-1])


def test_nan_mask():
    arrays, ll, ti = _wswd((4, 5, 6))
    arrays['windspeed_100m'][0, 0, 0] = np.nan
    arrays['winddirection_100m'][3, 4, 5] = np.nan
    feats = ['windspeed_100m', 'winddirection_100m']
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dv = _deriver(dict(arrays), ll, ti, feats,
                      nan_method_kwargs={'method': 'mask'})
    assert dv.as_array().shape == (4, 5, 4, 2)
    assert dv.time_index.equals(ti[1:5])
    assert np.array_equal(dv['windspeed_100m'],
                          arrays['windspeed_100m'][:, :, 1:5])
    with pytest.raises(NotImplementedError, match='interpolate_na'):
        _deriver(dict(arrays), ll, ti, feats,
                 nan_method_kwargs={'method': 'linear', 'dim': 'time'})
    clean, _, _ = _wswd((4, 5, 6))
    dv = _deriver(clean, ll, ti, feats,
                  nan_method_kwargs={'method': 'linear', 'dim': 'time'})
    assert dv.as_array().shape == (4, 5, 6, 2)


def test_remaining_compute_methods():
    """PressureWRF, SurfaceRH and TempNCforCC through a registry"""
    rng = np.random.default_rng(15)
    shape = (4, 5, 6)
    arrays = {'p_100m': rng.normal(0, 300, shape),
              'pb_100m': rng.uniform(9e4, 1e5, shape),
              'd2m': rng.uniform(-20, 15, shape),
              'temperature_2m': rng.uniform(-10, 30, shape),
              'ta_100m': rng.uniform(250, 300, shape)}
    arrays = {k: v.astype(np.float32) for k, v in arrays.items()}
    ti = pd.date_range('2020-01-01', periods=6, freq='h')
    dv = _deriver(dict(arrays), R.grid(4, 5), ti,
                  ['pressure_100m', 'relativehumidity_2m'],
                  FeatureRegistry={**D.RegistryBase,
                                   'pressure_(.*)': D.PressureWRF})
    assert np.array_equal(dv['pressure_100m'],
                          arrays['p_100m'] + arrays['pb_100m'])
    want = R.surface_rh(arrays['d2m'], arrays['temperature_2m'])
    assert want.dtype == np.float32
    assert np.array_equal(dv['relativehumidity_2m'], want)
    dv = _deriver({'ta_100m': arrays['ta_100m']}, R.grid(4, 5), ti,
                  ['temperature_100m'], FeatureRegistry=D.RegistryNCforCC)
    assert np.array_equal(dv['temperature_100m'],
                          R.to_celsius(arrays['ta_100m']))
    assert dv.data.attrs['temperature_100m']['units'] == 'C'


def test_all_features_and_the_cube():
    """``features='all'`` keeps multi-level arrays and a 2-D topography:
    they are reachable by name, and the default cube says why it cannot hold
    them"""
    arrays, ll, ti = _fake()
    dv = _deriver(arrays, ll, ti, 'all')
    assert dv.features == ['zg', 'topography', 'u']
    assert dv['u'].shape == (10, 10, 20, 3)
    with pytest.raises(ValueError, match='not .s1, s2, t. features'):
        dv.as_array()
    with pytest.raises(ValueError, match='not .s1, s2, t. features'):
        _deriver(arrays, ll, ti, 'all', time_roll=1)


def test_pair_halves_do_not_outlive_their_use():
    arrays, ll, ti = _wswd()
    data = D.DeriveData(arrays, ll, ti, backend=D.NumpyBackend())
    u = D.UWind.compute(data, 100)
    assert len(data._pairs) == 1                  # v waits for its caller
    v = D.VWind.compute(data, 100)
    assert data._pairs == {}
    u2, v2 = R.transform_rotate_wind(arrays['windspeed_100m'],
                                     arrays['winddirection_100m'], ll)
    assert np.array_equal(u, u2.astype(np.float32))
    assert np.array_equal(v, v2.astype(np.float32))
    D.UWind.compute(data, 100)
    data.clear_pairs()
    assert data._pairs == {}
    dv = D.DeviceDeriver(data, ['u_100m'], backend=data.backend)
    assert dv.data._pairs == {} and data._pairs == {}
