"""CPU tests of the non-neural downscalers: the numpy
restatement ``tests/interp_ref.py`` (what the GPU tests compare against)
pinned against Pillow and scipy, the reference's linear-model test
procedures run on it, and the host logic of ``LinearInterp``,
``SurfaceSpatialMetModel`` and ``MultiStepSurfaceMetGan`` — nothing here
needs a GPU."""
import json
import os
import re

import numpy as np
import pytest

from tests import interp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRHP = ['temperature_2m', 'temperature_10m', 'temperature_100m',
        'relativehumidity_2m', 'relativehumidity_10m',
        'relativehumidity_100m', 'pressure_0m', 'pressure_100m',
        'pressure_200m']


@pytest.mark.parametrize('method', R.METHODS)
def test_restated_resize_is_pillows(method):
    """bit-identical to Pillow 12 in mode 'F' (float32 and float64 arrays
    in), odd and 2 x 2 shapes, s in {1, 2, 3, 5, 10, 15}; the dense form
    within an ulp of max|field|"""
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(0)
    for s in (1, 2, 3, 5, 10, 15):
        for shape in ((7, 5), (2, 2), (4, 9)):
            for dtype in (np.float32, np.float64):
                a = (rng.standard_normal(shape) * 30 + 10).astype(dtype)
                want = np.array(Image.fromarray(a).resize(
                    (shape[1] * s, shape[0] * s),
                    resample=getattr(Image.Resampling, method)))
                got = R.resize(a, s, method)
                assert got.dtype == np.float32 and got.shape == want.shape
                if method == 'HAMMING':
                    np.testing.assert_array_max_ulp(got, want, maxulp=1)
                else:
                    np.testing.assert_array_equal(got, want)
                dense = R.resize(a, s, method, dense=True)
                assert np.abs(dense - want).max() <= \
                    np.spacing(np.abs(want).max())


def _grid_interp(low, s, t, t_centered):
    """scipy's RegularGridInterpolator with linear extrapolation on
    cell-centred coordinates (time at the cell start unless centred)"""
    interp = pytest.importorskip('scipy.interpolate')
    axes, new = [], []
    for n, e, centred in ((low.shape[0], s, True), (low.shape[1], s, True),
                          (low.shape[2], t, t_centered)):
        off = 0.5 if centred else 0.0
        axes.append((np.arange(n) + off) / n)
        new.append((np.arange(n * e) + off) / (n * e))
    f = interp.RegularGridInterpolator(tuple(axes), low, bounds_error=False,
                                       fill_value=None)
    pts = np.stack(np.meshgrid(*new, indexing='ij'), axis=-1)
    return f(pts)


@pytest.mark.parametrize('shape,s,t,tc', [
    ((4, 5, 6), 2, 3, False), ((3, 7, 4), 3, 2, True),
    ((5, 4, 3), 1, 4, False), ((6, 5, 24), 5, 1, True),
    ((2, 2, 2), 3, 24, False)])
def test_restated_st_interp_is_scipys(shape, s, t, tc):
    low = np.random.default_rng(1).standard_normal(shape) * 7
    want = _grid_interp(low, s, t, tc)
    got = R.st_interp(low, s, t, tc)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


def _reference_linear_procedures(generate):
    """the reference's test_linear_spatial / test_linear_temporal
    arrangements (tests/forward_pass/test_linear_model.py): a field that
    varies along one axis, checked against interp1d with extrapolation"""
    interp1d = pytest.importorskip('scipy.interpolate').interp1d
    rng = np.random.default_rng(5)
    vals = rng.uniform(0, 100, 3)
    lr = np.broadcast_to(vals[None, None, :, None, None],
                         (1, 2, 3, 6, 1)).copy()
    hr = generate(lr, 2, 1, False)
    assert hr.shape == (1, 4, 6, 6, 1)
    truth = interp1d(np.arange(3), vals, fill_value='extrapolate')(
        np.linspace(-1 / 4, 2 + 1 / 4, 6))
    assert np.allclose(truth, hr[0, 0, :, 0, 0])
    lr = np.broadcast_to(vals[None, None, None, :, None],
                         (1, 2, 2, 3, 1)).copy()
    hr = generate(lr, 1, 3, True)
    assert hr.shape == (1, 2, 2, 9, 1)
    truth = interp1d(np.arange(3), vals, fill_value='extrapolate')(
        np.linspace(-1 / 3, 2 + 1 / 3, 9))
    assert np.allclose(hr[0, 0, 0, :, 0], truth)


def test_reference_linear_procedures_on_the_restatement():
    _reference_linear_procedures(R.linear_generate)


def test_public_names():
    import sup3r_amd
    from sup3r_amd import (LinearInterp, MultiStepSurfaceMetGan,
                           SurfaceSpatialMetModel)
    for name in ('LinearInterp', 'SurfaceSpatialMetModel',
                 'MultiStepSurfaceMetGan'):
        assert name in sup3r_amd.__all__
    assert issubclass(MultiStepSurfaceMetGan, sup3r_amd.MultiStepGan)
    assert issubclass(SurfaceSpatialMetModel, LinearInterp)


def test_product_does_not_import_sklearn_or_the_restatement():
    pkg = os.path.join(ROOT, 'sup3r_amd')
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r'^\s*(from|import)\s+(sklearn|tests)\b',
                                     src, flags=re.M), f


def test_linear_meta_save_load(tmp_path):
    from sup3r_amd import LinearInterp
    res = {'spatial': '30km', 'temporal': '60min'}
    m = LinearInterp(['u_10m', 'v_10m'], 3, 4, t_centered=True,
                     input_resolution=res)
    assert m.meta == {'input_resolution': res,
                      'lr_features': ['u_10m', 'v_10m'], 's_enhance': 3,
                      't_enhance': 4, 't_centered': True,
                      'hr_out_features': ['u_10m', 'v_10m'],
                      'class': 'LinearInterp'}
    assert (m.input_dims, m.is_5d, m.is_4d) == (5, True, False)
    assert m.s_enhancements == [3] and m.t_enhancements == [4]
    assert m.hr_exo_features == [] and m.means is None and m.stdevs is None
    m.save(str(tmp_path))
    with open(tmp_path / 'model_params.json') as f:
        assert json.load(f) == {'meta': m.meta}
    m2 = LinearInterp.load(str(tmp_path))
    assert m2.meta == m.meta and m2.input_resolution == res
    with pytest.raises(AssertionError):
        LinearInterp.load(str(tmp_path / 'nowhere'))
    # an axis of length 1 is refused before anything reaches a device
    with pytest.raises(AssertionError):
        m.generate(np.zeros((1, 4, 1, 3, 2), np.float32))


def test_surface_meta_roundtrip_drops_what_the_reference_drops(tmp_path):
    """``load`` keeps only the meta keys that are ``__init__`` arguments:
    the lapse rate, regression weights and pressure constants of a saved
    model come back as the class defaults (reference quirk, kept)"""
    from sup3r_amd import SurfaceSpatialMetModel as S
    res = {'spatial': '3km', 'temporal': '1440min'}
    m = S(TRHP, 15, noise_adders=0.1, temp_lapse=0.007, w_delta_temp=-3.5,
          w_delta_topo=-0.02, pres_div=40000.0, pres_exp=5.0,
          interp_method='BICUBIC', input_resolution=res, fix_bias=False)
    assert set(m.meta) == {
        'temp_lapse_rate', 's_enhance', 't_enhance', 'noise_adders',
        'input_resolution', 'weight_for_delta_temp', 'weight_for_delta_topo',
        'pressure_divisor', 'pressure_exponent', 'lr_features',
        'hr_out_features', 'interp_method', 'fix_bias', 'class'}
    assert m.meta['noise_adders'] == [0.1] * 9
    assert (m.meta['temp_lapse_rate'], m.meta['pressure_exponent']) == \
        (0.007, 5.0)
    m.save(str(tmp_path))
    m2 = S.load(str(tmp_path))
    for key in ('lr_features', 's_enhance', 'noise_adders',
                'input_resolution', 'interp_method', 'fix_bias', 'class',
                't_enhance'):
        assert m2.meta[key] == m.meta[key], key
    assert m2.meta['temp_lapse_rate'] == S.TEMP_LAPSE
    assert m2.meta['weight_for_delta_temp'] == S.W_DELTA_TEMP
    assert m2.meta['weight_for_delta_topo'] == S.W_DELTA_TOPO
    assert m2.meta['pressure_divisor'] == S.PRES_DIV
    assert m2.meta['pressure_exponent'] == S.PRES_EXP
    assert len(m2) == 1 and m2.input_dims == 4 and m2.is_4d
    assert m2.s_enhance == 15 and m2.t_enhance == 1
    assert m2.hr_exo_features == [] and m2.means is None
    assert m2.model_params == {'meta': m2.meta}


def test_feature_partition_and_rh_pairing():
    from sup3r_amd import SurfaceSpatialMetModel as S
    feats = ['temperature_12m', 'relativehumidity_2m', 'temperature_2m',
             'pressure_0m', 'u_10m', 'temperature_min_2m',
             'relativehumidity_min_2m', 'relativehumidity_max_2m',
             'temperature_max_2m', 'relativehumidity_12m']
    m = S(feats, 2)
    assert m.feature_inds_temp == [0, 2, 5, 8]
    assert m.feature_inds_pres == [3]
    assert m.feature_inds_rh == [1, 6, 7, 9]
    assert m.feature_inds_other == [4]
    # endswith: '_2m' pairs with the 'temperature_12m' listed first
    assert m._get_temp_rh_ind(1) == 0
    assert m._get_temp_rh_ind(6) == 5 and m._get_temp_rh_ind(7) == 8
    assert m._get_temp_rh_ind(9) == 0
    for i in m.feature_inds_rh:
        assert m._get_temp_rh_ind(i) == R.temp_rh_ind(feats, i)
    kinds, pair = m._channel_plan()
    assert list(kinds) == [1, 3, 1, 2, 0, 1, 3, 3, 1, 3]
    assert list(pair) == [-1, 0, -1, -1, -1, -1, 5, 8, -1, 0]
    with pytest.raises(KeyError):
        S(['relativehumidity_100m', 'temperature_10m'], 2)._get_temp_rh_ind(0)
    with pytest.raises(KeyError):
        S(['temperature_2m', 'relativehumidity_min_2m'], 2)._get_temp_rh_ind(1)
    with pytest.raises(KeyError):
        S(['temperature_2m', 'relativehumidity_100m'], 2)._channel_plan()


def test_get_s_enhance():
    from sup3r_amd import SurfaceSpatialMetModel as S
    assert S._get_s_enhance(np.zeros((4, 5)), np.zeros((12, 15))) == 3
    for lr, hr in (((4, 5), (10, 15)), ((4, 5), (8, 15)),
                   ((4, 5, 1), (8, 10)), ((4, 5), (8, 10, 1))):
        with pytest.raises(AssertionError):
            S._get_s_enhance(np.zeros(lr), np.zeros(hr))


def test_interp_method_names_are_pillows():
    from sup3r_amd import SurfaceSpatialMetModel as S
    from sup3r_amd.surface import Resampling
    Image = pytest.importorskip('PIL.Image')
    for name in R.METHODS:
        S(['a'], 2, interp_method=name)
        assert getattr(Resampling, name) == int(getattr(Image.Resampling,
                                                        name))
    with pytest.raises(AttributeError):
        S(['a'], 2, interp_method='CUBIC')


def test_product_coefficients_are_the_restatements():
    from sup3r_amd.surface import Resampling, pillow_coeffs
    for method in R.METHODS:
        for n, s in ((75, 15), (7, 3), (2, 2), (5, 1)):
            lo, cnt, w = pillow_coeffs(n, n * s, getattr(Resampling, method))
            lo2, cnt2, w2 = R.coeffs(n, n * s, method)
            assert np.array_equal(lo, lo2) and np.array_equal(cnt, cnt2)
            assert np.array_equal(w, w2)
            assert w.shape[1] <= 8


def test_lstsq_regression():
    from sup3r_amd.surface import LstsqRegression
    rng = np.random.default_rng(2)
    x = rng.standard_normal((500, 2))
    y = x @ np.array([-3.9, -0.017]) + rng.standard_normal(500) * 1e-3
    r = LstsqRegression().fit(x, y)
    np.testing.assert_allclose(r.coef_, [-3.9, -0.017], atol=1e-3)
    assert r.intercept_ == 0.0
    np.testing.assert_allclose(r.predict(x), x @ r.coef_)


def _topo(s, h=6, w=5):
    rng = np.random.default_rng(4)
    topo_hr = rng.uniform(0, 800, (h * s, w * s)).astype(np.float32)
    return R.coarsen(topo_hr, s).astype(np.float32), topo_hr


def test_host_side_errors_before_any_device_work():
    """the checks ``generate`` makes on the host raise without a GPU: the
    topography shapes, the negative adjusted low-res pressure (+ the units
    warning), and MultiStepSurfaceMetGan's two topography steps"""
    from sup3r_amd import MultiStepSurfaceMetGan, SurfaceSpatialMetModel
    m = SurfaceSpatialMetModel(['temperature_2m', 'pressure_0m'], 2)
    topo_lr, topo_hr = _topo(2)
    x = np.ones((2, 6, 5, 2), np.float32)
    x[..., 1] = -1e6
    exo = {'topography': {'steps': [{'data': topo_lr}, {'data': topo_hr}]}}
    with pytest.warns(UserWarning, match='not be in Pa'):
        with pytest.raises(ValueError, match='negative'):
            m.generate(x, exogenous_data=exo)
    bad = {'topography': {'steps': [{'data': topo_lr},
                                    {'data': topo_hr[:-1]}]}}
    with pytest.raises(AssertionError):
        m.generate(x, exogenous_data=bad)
    with pytest.raises(AssertionError):       # s_enhance 3 vs topo ratio 2
        SurfaceSpatialMetModel(['temperature_2m'], 3).generate(
            x[..., :1], exogenous_data=exo)
    ms = MultiStepSurfaceMetGan([m])
    with pytest.raises(AssertionError):
        ms.generate(x)
    one = {'topography': {'steps': [{'model': 0, 'combine_type': 'input',
                                     'data': topo_lr}]}}
    with pytest.raises(AssertionError):
        ms.generate(x, exogenous_data=one)


def test_models_are_picked_by_class_name(tmp_path):
    """``get_model`` and ``MultiStepGan.load`` find the new classes from
    the name / ``meta.class``; the chunk executor sends them through
    ``model.generate`` (no ``_gen``: no device batch path)"""
    from sup3r_amd import (LinearInterp, MultiStepGan, MultiStepSurfaceMetGan,
                           SurfaceSpatialMetModel)
    from sup3r_amd.forward_pass import ForwardPass, get_model
    LinearInterp(['temperature_2m'], 2, 3).save(str(tmp_path / 'lin'))
    SurfaceSpatialMetModel(['temperature_2m'], 5).save(str(tmp_path / 'sur'))
    ms = MultiStepGan.load([str(tmp_path / 'sur'), str(tmp_path / 'lin')])
    assert [type(m) for m in ms.models] == [SurfaceSpatialMetModel,
                                            LinearInterp]
    assert ms.s_enhancements == [5, 2] and ms.t_enhancements == [1, 3]
    assert ms.means == (None, None) and ms.input_dims == 4
    sur = get_model('SurfaceSpatialMetModel', str(tmp_path / 'sur'))
    assert type(sur) is SurfaceSpatialMetModel and sur.s_enhance == 5
    lin = get_model('LinearInterp', {'model_dir': str(tmp_path / 'lin')})
    assert type(lin) is LinearInterp and lin.t_enhance == 3
    msg = get_model('MultiStepSurfaceMetGan', {
        'surface_model_kwargs': {'model_dir': str(tmp_path / 'sur')},
        'temporal_model_kwargs': {'model_dirs': [str(tmp_path / 'lin')]}})
    assert type(msg) is MultiStepSurfaceMetGan and len(msg) == 2
    assert [type(m) for m in msg.models] == [SurfaceSpatialMetModel,
                                             LinearInterp]

    class Chunk:
        exo_data = None
    for model in (sur, lin, msg):
        assert ForwardPass._device_path(model, Chunk()) is False
