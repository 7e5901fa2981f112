"""CPU tests of ``sup3r_amd.exo``: the host control flow and the
``NumpyBackend`` against the reference's route restated in ``tests/exo_ref.py``
(scipy's KD-tree and ``griddata``, the pandas group-by)."""
import os
import sys
import warnings

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import exo_ref  # noqa: E402

from sup3r_amd import exo  # noqa: E402
from sup3r_amd.strategy import ArrayStrategy  # noqa: E402
from sup3r_amd.utilities import ExoData  # noqa: E402


# ------------------------------------------------------------------ fixtures
def lr_grid(s1=6, s2=7, lat0=40.013, lon0=-105.021, step=0.37):
    """(s1, s2, 2) regular grid, latitudes descending as the rasterizers';
    no dyadic spacing: a float32 source then hardly ever lies exactly
    between two targets"""
    lats = lat0 - step * np.arange(s1)
    lons = lon0 + step * np.arange(s2)
    return np.dstack(np.meshgrid(lats, lons, indexing='ij')).astype(np.float32)


def source_raster(lr, factor=6, pad=0.6, seed=0, t=None, holes=None,
                  jitter=0.0):
    """a raster ``factor`` times finer than ``lr`` over its extent plus
    ``pad`` degrees: (lat_lon (h, w, 2), values (h, w[, t])); ``jitter``
    degrees of noise on the coordinates keep a source from lying at the same
    distance from two targets"""
    rng = np.random.default_rng(seed)
    h, w = lr.shape[0] * factor, lr.shape[1] * factor
    lats = np.linspace(lr[..., 0].max() + pad, lr[..., 0].min() - pad, h)
    lons = np.linspace(lr[..., 1].min() - pad, lr[..., 1].max() + pad, w)
    ll = np.dstack(np.meshgrid(lats, lons, indexing='ij'))
    ll = (ll + jitter * rng.uniform(-1, 1, ll.shape)).astype(np.float32)
    shape = (h, w) if t is None else (h, w, t)
    vals = (2000 + 1000 * rng.standard_normal(shape)).astype(np.float32)
    if holes is not None:
        vals[holes(ll)] = np.nan
    return ll, vals


class FakeModel:
    def __init__(self, lr_features, hr_exo_features, hr_out_features,
                 s_enhance=1, t_enhance=1, obs_features=None):
        self.lr_features = lr_features
        self.hr_exo_features = hr_exo_features
        self.hr_out_features = hr_out_features
        self.s_enhance, self.t_enhance = s_enhance, t_enhance
        self.s_enhancements, self.t_enhancements = [s_enhance], [t_enhance]
        if obs_features is not None:
            self.obs_features = obs_features


class SurfaceSpatialMetModel(FakeModel):
    """(the handler dispatches on the class name)"""


class FakeMultiStep:
    def __init__(self, models):
        self.models = models
        self.s_enhancements = [m.s_enhance for m in models]
        self.t_enhancements = [m.t_enhance for m in models]
        self.s_enhance = int(np.prod(self.s_enhancements))
        self.t_enhance = int(np.prod(self.t_enhancements))


def two_step_topo():
    return FakeMultiStep([
        FakeModel(['u_10m', 'v_10m', 'topography'], ['topography'],
                  ['u_10m', 'v_10m'], s_enhance=2),
        FakeModel(['u_10m', 'v_10m', 'topography'], ['topography'],
                  ['u_10m', 'v_10m'], s_enhance=3)])


TIMES = pd.date_range('2020-01-01', periods=4, freq='h')


def handler(feature, model=None, steps=None, lr=None, src=None, **kw):
    lr = lr_grid() if lr is None else lr
    if src is None:
        ll, vals = source_raster(lr)
        src = exo.ExoSource(ll, **{feature.replace('_obs', ''): vals})
    return exo.ExoDataHandler(feature, exo.ExoInput(lr, TIMES), model=model,
                              steps=steps, source_files=src, device=False,
                              **kw)


# ------------------------------------------------- get_lat_lon and get_times
@pytest.mark.parametrize('lon0', [-105.0, 178.5])
def test_get_lat_lon_is_the_reference_and_leaves_its_input(lon0):
    lr = lr_grid(5, 6, lon0=lon0).astype(np.float64)
    if lon0 > 0:
        lr[..., 1] = (lr[..., 1] + 180) % 360 - 180    # crosses 180
        assert not exo.is_increasing_lons(lr)
    keep = lr.copy()
    got = exo.get_lat_lon(lr, (15, 12))
    assert np.array_equal(lr, keep)
    want = exo_ref.get_lat_lon(keep.copy(), (15, 12))
    assert got.shape == (15, 12, 2) and np.array_equal(got, want)
    assert np.array_equal(exo.pad_lat_lon(keep), exo_ref.pad_lat_lon(keep))
    assert (np.abs(got[..., 1]) <= 180).all()


@pytest.mark.parametrize('start,periods', [('2020-02-27', 4),    # has 29 Feb
                                           ('2021-02-27', 4),
                                           ('2019-02-27', 3)])
def test_get_times_is_the_reference(start, periods):
    lr = pd.date_range(start, periods=periods, freq='D')
    n = 24 * periods
    if not any((lr.month == 2) & (lr.day == 29)):
        full = pd.date_range(lr[0], lr[-1] + pd.Timedelta('1D'), freq='h')[:-1]
        n = int((~((full.month == 2) & (full.day == 29))).sum())
    if n % periods:
        with pytest.raises(AssertionError):
            exo.get_times(lr, 24 * periods)
        return
    got = exo.get_times(lr, n)
    assert got.equals(exo_ref.get_times(lr, n))
    one = pd.DatetimeIndex(['2020-06-01'])
    assert exo.get_times(one, 24).equals(exo_ref.get_times(one, 24))


# ------------------------------------------------ steps and their enhancement
def test_steps_of_a_single_model():
    m = FakeModel(['u_10m', 'Topography'], ['topography'], ['u_10m'],
                  s_enhance=3, t_enhance=4)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')               # upper case feature
        steps = exo.ExoDataHandler.get_exo_steps('topography', [m])
    assert steps == [{'model': 0, 'combine_type': 'input'},
                     {'model': 0, 'combine_type': 'layer'}]
    lr = lr_grid()
    ll, vals = source_raster(lr, factor=12)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        h = handler('topography', model=m, lr=lr,
                    src=exo.ExoSource(ll, topography=vals))
    assert (h.s_enhancements, h.t_enhancements) == ([1, 3], [1, 4])
    shapes = [s.shape for s in h.data['topography']['steps']]
    assert shapes == [(6, 7, 1), (18, 21, 1)]
    assert [s['combine_type'] for s in h.data['topography']['steps']] == \
        ['input', 'layer']


def test_steps_of_a_two_step_spatial_chain():
    model = two_step_topo()
    lr = lr_grid()
    ll, vals = source_raster(lr, factor=24)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')               # holes filled
        h = handler('topography', model=model, lr=lr,
                    src=exo.ExoSource(ll, topography=vals))
    assert h.steps == [
        {'model': 0, 'combine_type': 'input', 's_enhance': 1, 't_enhance': 1},
        {'model': 0, 'combine_type': 'layer', 's_enhance': 2, 't_enhance': 1},
        {'model': 1, 'combine_type': 'input', 's_enhance': 2, 't_enhance': 1},
        {'model': 1, 'combine_type': 'layer', 's_enhance': 6, 't_enhance': 1}]
    steps = h.data['topography']['steps']
    assert [s.shape for s in steps] == [(6, 7, 1), (12, 14, 1), (12, 14, 1),
                                        (36, 42, 1)]
    # steps with the same factors share one raster
    assert steps[1]['data'] is steps[2]['data']
    assert len(h._step_data) == 3
    ExoData(h.data)                                   # what the models take
    # the steps= form: without factors they come from the model ...
    given = [{'model': 0, 'combine_type': 'input'},
             {'model': 1, 'combine_type': 'layer'}]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        h2 = handler('topography', model=model, steps=given, lr=lr,
                     src=exo.ExoSource(ll, topography=vals))
    assert (h2.s_enhancements, h2.t_enhancements) == ([1, 6], [1, 1])
    # ... and steps that carry them are left alone
    own = [{'model': 0, 'combine_type': 'layer', 's_enhance': 3,
            't_enhance': 1}]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        h3 = handler('topography', model=model, steps=own, lr=lr,
                     src=exo.ExoSource(ll, topography=vals))
    assert h3.s_enhancements == [3]
    assert h3.data['topography']['steps'][0].shape == (18, 21, 1)


def test_steps_of_a_surface_model_and_of_obs_features():
    sfc = SurfaceSpatialMetModel(['temperature_2m'], [], ['temperature_2m'],
                                 s_enhance=2)
    assert exo.ExoDataHandler.get_exo_steps('topography', [sfc]) == [
        {'model': 0, 'combine_type': 'input'},
        {'model': 0, 'combine_type': 'output'}]
    h = handler('topography', model=sfc, fill_nans=False)
    assert (h.s_enhancements, h.t_enhancements) == ([1, 2], [1, 1])
    obs = FakeModel(['u_10m'], [], ['u_10m'], s_enhance=2, t_enhance=1,
                    obs_features=['u_10m_obs'])
    assert exo.ExoDataHandler.get_exo_steps('u_10m_obs', [obs]) == [
        {'model': 0, 'combine_type': 'layer'}]
    assert exo.ExoDataHandler.get_exo_steps('u_10m', [obs]) == [
        {'model': 0, 'combine_type': 'input'},
        {'model': 0, 'combine_type': 'output'}]
    lr = lr_grid()
    ll, vals = source_raster(lr, factor=2, t=4)
    h = handler('u_10m_obs', model=obs, lr=lr,
                src=exo.ExoSource(ll, time_index=TIMES, u_10m=vals))
    assert h.s_enhancements == [2]
    assert h.data['u_10m_obs']['steps'][0].shape == (12, 14, 4, 1)


def _model_kinds():
    single = FakeModel(['u_10m', 'topography'], ['topography'], ['u_10m'],
                       s_enhance=3, t_enhance=4)
    sfc = SurfaceSpatialMetModel(['temperature_2m'], [], ['temperature_2m'],
                                 s_enhance=2)
    obs = FakeModel(['u_10m'], [], ['u_10m'], s_enhance=2,
                    obs_features=['topography'])
    return {'single': (single, [(1, 1), (3, 4)]),
            'chain': (two_step_topo(), [(1, 1), (2, 1), (2, 1), (6, 1)]),
            'surface': (sfc, [(1, 1), (2, 1)]),
            'obs': (obs, [(2, 1)])}


@pytest.mark.parametrize('kind', ['single', 'chain', 'surface', 'obs'])
def test_steps_form_with_and_without_factors(kind):
    """``steps=`` without factors gets the model's products, with factors it
    is left alone; both give the fields ``model=`` alone gives"""
    model, factors = _model_kinds()[kind]
    lr = lr_grid()
    ll, vals = source_raster(lr, factor=24)
    src = exo.ExoSource(ll, topography=vals)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        auto = handler('topography', model=model, lr=lr, src=src)
        assert list(zip(auto.s_enhancements, auto.t_enhancements)) == factors
        bare = [{'model': s['model'], 'combine_type': s['combine_type']}
                for s in auto.steps]
        assert all('s_enhance' not in s for s in bare)
        h1 = handler('topography', model=model, steps=bare, lr=lr, src=src)
        assert h1.steps == auto.steps
        fixed = [dict(s, s_enhance=2, t_enhance=1) for s in bare]
        h2 = handler('topography', model=model, steps=fixed, lr=lr, src=src)
        assert h2.s_enhancements == [2] * len(bare)
        # with the factors in every step no model is needed
        h3 = handler('topography', steps=[dict(s) for s in fixed], lr=lr,
                     src=src)
    for a, b in zip(auto.data['topography']['steps'],
                    h1.data['topography']['steps']):
        assert a.shape == b.shape == (6 * a['s_enhance'], 7 * a['s_enhance'],
                                      1)
        assert np.array_equal(a['data'], b['data'])
    for a, b in zip(h2.data['topography']['steps'],
                    h3.data['topography']['steps']):
        assert a.shape == (12, 14, 1) and np.array_equal(a['data'], b['data'])


def test_the_three_assertions():
    model = two_step_topo()
    with pytest.raises(AssertionError, match='exceeds number of model steps'):
        handler('topography', model=model,
                steps=[{'model': 2, 'combine_type': 'input'}])
    with pytest.raises(AssertionError, match='without valid combine_type'):
        handler('topography', model=model,
                steps=[{'model': 0, 'combine_type': 'middle'}])
    h = object.__new__(exo.ExoDataHandler)
    h.models, h.steps = None, [{'model': 0, 'combine_type': 'input'}]
    en_check = all('s_enhance' in v for v in h.steps) or h.models is not None
    assert not en_check                # the condition the first assert guards
    import inspect
    assert 'needs s_enhance and t_enhance' in inspect.getsource(
        exo.ExoDataHandler.__init__)


# ------------------------------------------------------------------ dispatch
def test_dispatch_and_sza():
    lr = exo.ExoInput(lr_grid(), TIMES)
    ll, vals = source_raster(lr.lat_lon)
    src = exo.ExoSource(ll, topography=vals, u_10m=vals[..., None])
    kw = dict(source_files=src, device=False)
    assert type(exo.ExoRasterizer('topography', lr, **kw)) is \
        exo.BaseExoRasterizer
    assert type(exo.ExoRasterizer('u_10m_obs', lr, **kw)) is exo.ObsRasterizer
    sza = exo.ExoRasterizer('SZA', lr, **kw)
    assert type(sza) is exo.SzaRasterizer
    with pytest.raises(NotImplementedError, match='SolarPosition'):
        sza.data
    # plain mappings in the place of the containers
    r = exo.ExoRasterizer(
        'topography', {'lat_lon': lr.lat_lon, 'time_index': TIMES},
        source_files={'lat_lon': ll, 'topography': vals}, device=False,
        cache_dir='/somewhere', s_enhance=2)
    corner = '_'.join(str(float(v)) for v in lr.lat_lon[-1, 0])
    assert r.cache_file == os.path.join(
        '/somewhere', f'exo_topography_{corner}_6x7_2x_1x.nc')
    assert r.lr_shape == (6, 7, 4) and r.hr_shape == (12, 14, 4)
    assert r.source_lat_lon.dtype == np.float32
    assert exo.ExoRasterizer('topography', lr, **kw).cache_file is None


# -------------------------------------- NumpyBackend against KD-tree + pandas
def bound(exact_abs, mean_abs, n):
    """the group-mean bound against the pandas route (float32 Kahan sum)"""
    return (2.0 ** -24 * exact_abs + n * 2.0 ** -52 * mean_abs
            + 2.0 ** -23 * mean_abs + 2.0 ** -24 * exact_abs)


def test_numpy_backend_2d_against_the_reference_route():
    lr = lr_grid()
    ll, vals = source_raster(
        lr, factor=5, jitter=0.01,
        holes=lambda p: (p[..., 0] > 39.2) & (p[..., 1] < -104))
    want_ll = exo_ref.get_lat_lon(lr.astype(np.float32), (12, 14))
    ll = exo_ref.untie(ll.reshape(-1, 2), want_ll.reshape(-1, 2)).reshape(
        ll.shape)
    r = exo.ExoRasterizer('topography', exo.ExoInput(lr, TIMES),
                          source_files=exo.ExoSource(ll, topography=vals),
                          s_enhance=2, device=False, fill_nans=False)
    hr_ll = r.hr_lat_lon
    assert hr_ll.dtype == np.float32
    assert np.array_equal(hr_ll, want_ll.astype(np.float32))
    dub = exo_ref.get_distance_upper_bound(hr_ll)
    assert r.get_distance_upper_bound() == dub
    src = ll.reshape(-1, 2)
    gap, clear = exo_ref.nearest_margins(src, hr_ll.reshape(-1, 2), dub)
    assert gap > 2.0 ** -50 and clear
    dists, nn = exo_ref.query_tree(hr_ll, src, dub)
    assert np.array_equal(r.nn, nn)
    assert np.array_equal(r.dists, dists)
    want = exo_ref.get_data_2d('topography', vals.reshape(-1, 1), nn,
                               r.hr_shape)
    got = r.data
    assert got.shape == (12, 14, 1) and got.values.dtype == np.float32
    assert np.array_equal(np.isnan(got.values[..., 0]), np.isnan(want))
    assert np.isnan(want).any()
    exact, n, mean_abs = exo_ref.exact_group_mean(
        nn, vals.reshape(-1, 1), 12 * 14, 1, [0])
    ok = ~np.isnan(want.reshape(-1))
    err = np.abs(got.values.reshape(-1)[ok].astype(np.float64)
                 - want.reshape(-1)[ok])
    lim = bound(np.abs(exact[ok, 0]), mean_abs[ok, 0], n[ok, 0])
    assert (err <= lim).all()
    # filled: the reference's warning with its count, nn_fill_array's result
    r2 = exo.ExoRasterizer('topography', exo.ExoInput(lr, TIMES),
                           source_files=exo.ExoSource(ll, topography=vals),
                           s_enhance=2, device=False, scale_factor=0.5)
    with pytest.warns(UserWarning, match=f'^{int(np.isnan(want).sum())} '
                      'target pixels did not have unique high-resolution '
                      'topography source data'):
        filled = r2.data.values
    assert np.array_equal(filled, exo_ref.nn_fill_array(
        (got.values.astype(np.float64) * 0.5).astype(np.float32)))


def test_numpy_backend_3d_and_obs_against_the_reference_route():
    lr = lr_grid(4, 5)
    src_times = pd.date_range('2020-01-01 02:00', periods=5, freq='h')
    ll, vals = source_raster(lr, factor=3, t=5, seed=3, jitter=0.01)
    vals[::7, ::5, 1] = np.nan
    ll = exo_ref.untie(ll.reshape(-1, 2), lr.reshape(-1, 2)).reshape(ll.shape)
    r = exo.ExoRasterizer(
        'u_10m', exo.ExoInput(lr, TIMES), device=False, fill_nans=False,
        source_files=exo.ExoSource(ll, time_index=src_times, u_10m=vals))
    dub = r.get_distance_upper_bound()
    dists, nn = exo_ref.query_tree(r.hr_lat_lon, ll.reshape(-1, 2), dub)
    want = exo_ref.get_data_3d('u_10m', vals.reshape(-1, 5), src_times, nn,
                               dists, r.hr_shape, r.hr_time_index)
    got = r.data
    assert got.shape == (4, 5, 4) and got.as_array().shape == (4, 5, 4, 1)
    assert got.time_index.equals(TIMES)
    # hours 0 and 1 have no source step; 2 and 3 are source steps 0 and 1
    assert np.isnan(got.values[..., :2]).all()
    assert not np.isnan(got.values[..., 2:]).any()
    assert np.array_equal(np.isnan(got.values), np.isnan(want))
    assert np.allclose(got.values[..., 2:], want[..., 2:], rtol=3e-7)
    # observations: far fewer points than targets, NaN kept, no fill
    rng = np.random.default_rng(5)
    obs_ll = np.stack([rng.uniform(38.4, 40.1, 9),
                       rng.uniform(-105.1, -102.9, 9)], axis=1)
    obs = rng.standard_normal((9, 4)).astype(np.float32)
    o = exo.ExoRasterizer(
        'u_10m_obs', exo.ExoInput(lr, TIMES), device=False, s_enhance=2,
        source_files=exo.ExoSource(obs_ll, time_index=TIMES, u_10m=obs))
    with warnings.catch_warnings():
        warnings.simplefilter('error')                # no fill warning
        field = o.data.values
    assert o.fill_nans is False
    assert np.isnan(field).any() and not np.isnan(field).all()
    dists, nn = exo_ref.query_tree(o.hr_lat_lon, obs_ll.astype(np.float32),
                                   o.distance_upper_bound)
    want = exo_ref.get_data_3d('u_10m', obs, TIMES, nn, dists, o.hr_shape,
                               o.hr_time_index)
    assert np.array_equal(np.isnan(field), np.isnan(want))
    assert np.allclose(field[~np.isnan(want)], want[~np.isnan(want)],
                       rtol=3e-7)
    # nothing within the bound: the reference's warning
    far = exo.ExoRasterizer(
        'u_10m_obs', exo.ExoInput(lr, TIMES), device=False,
        source_files=exo.ExoSource(obs_ll + 30, time_index=TIMES, u_10m=obs))
    with pytest.warns(UserWarning, match='No observations found within the '
                      'distance upper bound'):
        assert np.isnan(far.data.values).all()


def test_numpy_backend_ties_follow_the_device_rule():
    tgt = np.array([[0, 0], [0, 1], [1, 0], [1, 1]], np.float32)
    src = np.array([[0.5, 0.5], [0, 0.5], [3, 3], [1, 0.25]], np.float32)
    be = exo.NumpyBackend()
    nn, d = be.nearest(src, tgt, 0.75)
    want_nn, want_d = exo_ref.brute_nearest(src, tgt, 0.75)
    assert list(nn) == list(want_nn) == [0, 0, 4, 2]
    assert np.array_equal(d, want_d)
    # a point at exactly r is a miss
    nn, _ = be.nearest(np.array([[0, 0.5]], np.float32), tgt, 0.5)
    assert list(nn) == [4]


# ----------------------------------------------------------------- strategy
def test_array_strategy_rasterises_what_exo_data_would_carry():
    model = two_step_topo()
    lr = lr_grid(6, 8)
    ll, vals = source_raster(lr, factor=24)
    src = exo.ExoSource(ll, topography=vals)
    domain = np.random.default_rng(0).standard_normal(
        (6, 8, 4, 3)).astype(np.float32)
    common = dict(model_kwargs={}, fwp_chunk_shape=(4, 4, 4), spatial_pad=1,
                  temporal_pad=0, model=model, input_lat_lon=lr,
                  input_time_index=TIMES)
    kwargs = {'topography': {'source_files': src, 'device': False}}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        a = ArrayStrategy(domain, exo_handler_kwargs=kwargs, **common)
        fields = handler('topography', model=model, lr=lr, src=src).data
    b = ArrayStrategy(domain, exo_data=fields, **common)
    assert a.n_chunks == b.n_chunks == 4
    for i in range(a.n_chunks):
        ca, cb = a.init_chunk(i), b.init_chunk(i)
        sa, sb = (c.exo_data['topography']['steps'] for c in (ca, cb))
        assert len(sa) == len(sb) == 4
        for x, y in zip(sa, sb):
            assert {k: v for k, v in x.items() if k != 'data'} == \
                {k: v for k, v in y.items() if k != 'data'}
            assert isinstance(x['data'], np.ndarray)
            assert np.array_equal(x['data'], y['data'])
    with pytest.raises(ValueError, match='exo_data or exo_handler_kwargs'):
        ArrayStrategy(domain, exo_data=fields, exo_handler_kwargs=kwargs,
                      **common)
    # with neither, nothing changes
    assert ArrayStrategy(domain, **common).init_chunk(0).exo_data is None


def test_package_exports_and_header():
    import re
    import sup3r_amd
    from sup3r_amd import _lib
    for name in exo.__all__:
        assert name in sup3r_amd.__all__ and hasattr(sup3r_amd, name)
    root = os.path.join(os.path.dirname(__file__), '..')
    with open(os.path.join(root, 'include', 'sup3r_hip.h')) as f:
        header = f.read()
    for name in ('s3_exo_nearest', 's3_exo_group_mean'):
        assert re.search(rf'\bint\s+{name}\s*\(', header)
        assert name in _lib.EXPORTS and f'{name}_work_bytes' in _lib.EXPORTS
    assert re.search(rf'#define S3_EXO_MAX_SLAB {_lib.EXO_MAX_SLAB}\b', header)
