"""GPU tests (``-m gpu``) of the non-neural downscalers on the MI355X
(SURVEY.md §2 row 7): ``s3_resize2d`` / ``s3_st_interp`` /
``s3_surface_downscale`` against the numpy restatement tests/interp_ref.py
(itself pinned to Pillow and scipy by tests/test_interp_cpu.py), noise,
errors, the multi-step arrangement of the reference's
``test_multi_step_surface`` and the chunk executor."""
import json
import os

import numpy as np
import pytest

from tests import interp_ref as R
from tests.test_interp_cpu import TRHP, _reference_linear_procedures

pytestmark = pytest.mark.gpu

CFG = os.path.join(os.path.dirname(__file__), '..', 'sup3r_amd', 'configs')
# the assumed 9-feature trhp layout + a _max_ pair
FEATS = TRHP + ['temperature_max_2m', 'relativehumidity_max_2m']


def _ulps(ref, n):
    return n * float(np.spacing(np.float32(np.abs(ref).max())))


def _surface_inputs(n, h, w, s, feats=FEATS, seed=0):
    """degrees C, % and Pa; float32-exact topography (the device's input)"""
    rng = np.random.default_rng(seed)
    cols = []
    for f in feats:
        if f.startswith('temperature'):
            cols.append(15 + 6 * rng.standard_normal((n, h, w)))
        elif f.startswith('relativehumidity'):
            cols.append(np.clip(60 + 15 * rng.standard_normal((n, h, w)),
                                1, 100))
        elif f.startswith('pressure'):
            cols.append(95000 + 800 * rng.standard_normal((n, h, w)))
        else:
            cols.append(rng.standard_normal((n, h, w)))
    low = np.stack(cols, axis=-1).astype(np.float32)
    topo_hr = rng.uniform(0, 1500, (h * s, w * s)).astype(np.float32)
    topo_lr = R.coarsen(topo_hr.astype(np.float64), s).astype(np.float32)
    return low, topo_lr.astype(np.float64), topo_hr.astype(np.float64)


def _exo(topo_lr, topo_hr):
    return {'topography': {'steps': [{'data': topo_lr}, {'data': topo_hr}]}}


@pytest.mark.parametrize('method', R.METHODS)
def test_resize2d_vs_restatement(method):
    from sup3r_amd.surface import resize2d
    rng = np.random.default_rng(1)
    for shape, s in (((3, 75, 75, 9), 15), ((2, 7, 5, 3), 3),
                     ((1, 2, 2, 2), 2), ((2, 5, 3, 1), 1), ((1, 9, 4, 2), 5)):
        x = (rng.standard_normal(shape) * 10 + 5).astype(np.float32)
        y = resize2d(x, s, method).cpu().numpy()
        ref = np.moveaxis(R.resize(np.moveaxis(x, -1, 1), s, method,
                                   dense=shape[1] > 50), 1, -1)
        assert y.shape == ref.shape
        err = float(np.abs(y - ref).max())
        assert err <= _ulps(ref, 4), (method, shape, s, err)


@pytest.mark.parametrize('shape,s,t,tc', [
    ((2, 5, 4, 6, 3), 3, 4, False),      # float4 stores
    ((1, 4, 6, 5, 2), 2, 3, True),       # scalar stores
    ((2, 3, 5, 4, 1), 1, 2, False),      # s = 1
    ((1, 6, 3, 5, 2), 2, 1, True),       # t = 1
    ((1, 61, 3, 2, 1), 2, 2, False)])    # the reference fails on 61
def test_linear_interp_vs_restatement(shape, s, t, tc):
    from sup3r_amd import LinearInterp
    x = (np.random.default_rng(2).standard_normal(shape) * 20).astype(
        np.float32)
    model = LinearInterp([f'f{i}' for i in range(shape[-1])], s, t,
                         t_centered=tc)
    y = model.generate(x)
    ref = R.linear_generate(x, s, t, tc)
    assert y.shape == ref.shape and y.dtype == np.float32
    assert float(np.abs(y - ref).max()) <= 1e-6 * float(np.abs(x).max())
    np.testing.assert_array_equal(model.generate(x), y)


def test_reference_linear_procedures_on_the_device():
    from sup3r_amd import LinearInterp

    def generate(lr, s, t, tc):
        return LinearInterp(['feature'], s, t, t_centered=tc).generate(lr)
    _reference_linear_procedures(generate)


@pytest.mark.parametrize('method', R.METHODS)
def test_surface_vs_restatement(method):
    from sup3r_amd import SurfaceSpatialMetModel
    low, topo_lr, topo_hr = _surface_inputs(4, 20, 20, 15)
    for fix_bias in (True, False):
        model = SurfaceSpatialMetModel(FEATS, 15, interp_method=method,
                                       fix_bias=fix_bias)
        y = model.generate(low, exogenous_data=_exo(topo_lr, topo_hr))
        ref = R.surface_generate(low, topo_lr, topo_hr, FEATS, 15, method,
                                 fix_bias)
        assert y.shape == ref.shape == (4, 300, 300, len(FEATS))
        for i, f in enumerate(FEATS):
            err = float(np.abs(y[..., i] - ref[..., i]).max())
            scale = float(np.abs(ref[..., i]).max())
            assert err <= 2e-6 * scale, (method, fix_bias, f, err / scale)
        if fix_bias and method == 'LANCZOS':
            # two identical calls: bit-identical
            y2 = model.generate(low, exogenous_data=_exo(topo_lr, topo_hr))
            np.testing.assert_array_equal(y, y2)


def test_surface_noise():
    from sup3r_amd import SurfaceSpatialMetModel as S
    low, topo_lr, topo_hr = _surface_inputs(3, 12, 10, 5, TRHP, seed=3)
    exo = _exo(topo_lr, topo_hr)
    stdev = [0.07, None, 0.5, 0.1] + [None] * 5
    base = S(TRHP, 5).generate(low, exogenous_data=exo)
    noisy = S(TRHP, 5, noise_adders=stdev)
    S.seed(11)
    y1 = noisy.generate(low, exogenous_data=exo)
    y2 = noisy.generate(low, exogenous_data=exo)
    S.seed(11)
    np.testing.assert_array_equal(noisy.generate(low, exogenous_data=exo), y1)
    assert not np.array_equal(y1, y2)
    for i, sd in enumerate(stdev):
        d = (y1[..., i].astype(np.float64) - base[..., i])
        if sd is None:
            np.testing.assert_array_equal(y1[..., i], base[..., i])
            continue
        tol = _ulps(base[..., i], 1)
        assert d.min() >= -tol and d.max() < sd + tol, (i, d.min(), d.max())
        sigma = sd / np.sqrt(12 * d.size)
        assert abs(d.mean() - sd / 2) <= 5 * sigma + tol, (i, d.mean())
    # a scalar applies to every feature
    ys = S(TRHP, 5, noise_adders=0.2).generate(low, exogenous_data=exo)
    assert all((ys[..., i] != base[..., i]).any() for i in range(len(TRHP)))


def test_surface_pressure_error_from_the_device():
    """positive adjusted low-res pressure (host check passes) whose high-res
    field turns negative: ValueError from the device min-reduction"""
    from sup3r_amd import SurfaceSpatialMetModel as S
    low, topo_lr, topo_hr = _surface_inputs(2, 8, 8, 5, ['pressure_0m'])
    low[:] = 1.0
    with pytest.warns(UserWarning, match='not be in Pa'):
        with pytest.raises(ValueError, match='negative'):
            S(['pressure_0m'], 5).generate(
                low, exogenous_data=_exo(topo_lr, topo_hr))


def test_surface_train():
    """the regression recovers the weights that generated the humidity"""
    from sup3r_amd import SurfaceSpatialMetModel as S
    rng = np.random.default_rng(6)
    s, lat, lon, nd = 5, 40, 30, 6
    topo = rng.uniform(0, 2000, (lat, lon))
    temp = 15 + 3 * rng.standard_normal((lat, lon, nd))
    rh = 50 - 4.0 * temp - 0.02 * topo[..., None]
    w_t, w_z, regr, x, y = S(['temperature_2m', 'relativehumidity_2m'],
                             s).train(temp, rh, topo, {'spatial': '3km'})
    assert x.shape == (lat * lon * nd, 2) and y.shape == (lat * lon * nd,)
    np.testing.assert_allclose([w_t, w_z], [-4.0, -0.02], rtol=1e-3)
    assert np.abs(regr.predict(x) - y).mean() < 1e-2


def _gan(feats, t_enhance):
    """the reference test_multi_step_surface generator config, fp32"""
    from sup3r_amd import Sup3rGan
    gen = [{'class': 'FlexiblePadding',
            'paddings': [[0, 0], [3, 3], [3, 3], [3, 3], [0, 0]],
            'mode': 'REFLECT'},
           {'class': 'Conv3D', 'filters': 64, 'kernel_size': 3, 'strides': 1},
           {'class': 'Cropping3D', 'cropping': 2},
           {'alpha': 0.2, 'class': 'LeakyReLU'},
           {'class': 'SpatioTemporalExpansion', 'temporal_mult': t_enhance,
            'temporal_method': 'nearest'},
           {'class': 'FlexiblePadding',
            'paddings': [[0, 0], [3, 3], [3, 3], [3, 3], [0, 0]],
            'mode': 'REFLECT'},
           {'class': 'Conv3D', 'filters': 3, 'kernel_size': 3, 'strides': 1},
           {'class': 'Cropping3D', 'cropping': 2}]
    Sup3rGan.seed(0)
    m = Sup3rGan(gen, os.path.join(CFG, 'test_disc_st_same.json'),
                 precision='f32')
    m.set_norm_stats(dict(zip(feats, (0.3, 0.9, 0.1))),
                     dict(zip(feats, (0.02, 0.07, 0.03))))
    m.set_model_params(lr_features=feats, hr_out_features=feats,
                       input_resolution={'spatial': '30km',
                                         'temporal': '60min'},
                       s_enhance=1, t_enhance=t_enhance)
    m.init_weights((1, 12, 10, 4, 3), (1, 12, 10, 4 * t_enhance, 3))
    return m


def test_multi_step_surface(tmp_path):
    from sup3r_amd import MultiStepSurfaceMetGan
    feats = ['temperature_2m', 'relativehumidity_2m', 'pressure_0m']
    s, t = 2, 2
    gan = _gan(feats, t)
    gan.save(str(tmp_path / 'model'))
    os.makedirs(tmp_path / 'surface')
    with open(tmp_path / 'surface' / 'model_params.json', 'w') as f:
        json.dump({'meta': {'lr_features': feats, 'hr_out_features': feats,
                            's_enhance': s}}, f)
    ms = MultiStepSurfaceMetGan.load(
        surface_model_kwargs={'model_dir': str(tmp_path / 'surface')},
        temporal_model_kwargs={'model_dirs': str(tmp_path / 'model')})
    for m in ms.models:
        assert isinstance(m.s_enhance, int) and isinstance(m.t_enhance, int)
    with pytest.raises(AssertionError):
        ms.generate(np.ones((2, 10, 10, 3)))
    low, topo_lr, topo_hr = _surface_inputs(5, 4, 4, s, feats, seed=8)
    exo = {'topography': {'steps': [
        {'model': 0, 'combine_type': 'input', 'data': topo_lr},
        {'model': 0, 'combine_type': 'output', 'data': topo_hr}]}}
    hi = ms.generate(low, exogenous_data=exo)
    assert hi.shape == (1, 8, 8, 2 * 5, 3)
    sur = R.surface_generate(low, topo_lr, topo_hr, feats, s)
    ref = ms.models[1].generate(np.moveaxis(sur, 0, 2)[None])
    assert float(np.abs(hi - ref).max()) <= 1e-4 * float(np.abs(ref).max())


def test_forward_pass_with_topography_steps(tmp_path):
    """``ForwardPass.run`` over an ``ArrayStrategy`` and ``run_chunk`` with
    ``model_class`` 'SurfaceSpatialMetModel', topography as an 'input' step
    (s_enhance 1) and an 'output' step (s_enhance s): equal to
    ``model.generate`` chunk by chunk and close to the restatement"""
    from sup3r_amd import ForwardPass, SurfaceSpatialMetModel
    from sup3r_amd.strategy import ArrayStrategy
    feats = ['temperature_2m', 'relativehumidity_2m', 'pressure_0m']
    s = 3
    low, topo_lr, topo_hr = _surface_inputs(7, 12, 10, s, feats, seed=9)
    domain = np.transpose(low, (1, 2, 0, 3))            # (s1, s2, t, f)
    model = SurfaceSpatialMetModel(feats, s)
    model.save(str(tmp_path))
    kwargs = {'model_dir': str(tmp_path)}
    exo = {'topography': {'steps': [
        {'model': 0, 'combine_type': 'input', 'data': topo_lr[..., None],
         's_enhance': 1, 't_enhance': 1},
        {'model': 0, 'combine_type': 'output', 'data': topo_hr[..., None],
         's_enhance': s, 't_enhance': 1}]}}
    st = ArrayStrategy(domain, kwargs, (6, 5, 4), spatial_pad=1,
                       temporal_pad=1, model_class='SurfaceSpatialMetModel',
                       exo_data=exo, max_nodes=1)
    n, kept = ForwardPass.run(st, 0, return_data=True)
    assert n == st.fwp_slicer.n_chunks == len(kept) >= 4
    fwp = ForwardPass(st, 0)
    for idx, data in kept:
        c = fwp.get_input_chunk(idx)
        x = np.transpose(c.input_data, (2, 0, 1, 3))
        tl = c.exo_data['topography']['steps'][0]['data'][:, :, 0, 0]
        th = c.exo_data['topography']['steps'][1]['data'][:, :, 0, 0]
        y = model.generate(x, exogenous_data=_exo(tl, th))
        want = np.transpose(y, (1, 2, 0, 3))[tuple(c.hr_crop_slice)]
        np.testing.assert_array_equal(data, want)
        if idx == kept[0][0]:
            ref = R.surface_generate(x, tl, th, feats, s)
            ref = np.transpose(ref, (1, 2, 0, 3))[tuple(c.hr_crop_slice)]
            for i in range(len(feats)):
                assert np.abs(data[..., i] - ref[..., i]).max() <= \
                    2e-6 * np.abs(ref[..., i]).max()
            failed, out = ForwardPass.run_chunk(
                c, str(tmp_path), 'SurfaceSpatialMetModel', False)
            assert not failed
            np.testing.assert_array_equal(out, data)
