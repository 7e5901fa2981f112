"""CPU tests of ``sup3r_amd.qa`` with ``QaNumpyBackend``: the fixed
re-coarsening order against the reference's numpy calls (bit for bit on
time-first input), the procedure of the reference's tests/output/test_qa.py on
arrays, and the restated select / bin index of the kernels against
``np.percentile`` / ``np.histogram``."""
import os

import numpy as np
import pandas as pd
import pytest

from sup3r_amd import derive as D
from sup3r_amd import qa as Q
from sup3r_amd.forward_pass import NpzOutputHandler
from tests import qa_ref as R

BE = Q.QaNumpyBackend()
S, TE = 3, 4
FEATS = ['u_100m', 'v_100m']


# ------------------------------------------------------- the order of the sums
@pytest.mark.parametrize('s,te', [(2, 4), (3, 4), (5, 12), (3, 24), (4, 8)])
@pytest.mark.parametrize('method', R.METHODS)
def test_fixed_order_is_the_numpy_path_on_time_first_input(s, te, method):
    rng = np.random.default_rng(s * 100 + te)
    tf = (rng.standard_normal((2 * te, 3 * s, 4 * s)) * 30 + 280).astype(
        np.float32)
    if method in ('total', 'average'):
        tf[rng.random(tf.shape) < 0.05] = np.nan
    elif method in ('max', 'min'):
        tf[te + 1, s, 2 * s + 1] = np.nan
    want = R.numpy_path(tf, s, te, method)
    got = R.fixed_order(np.transpose(tf, (1, 2, 0)), s, te, method)
    assert want.dtype == np.float32
    assert R.same_bits(got, want)
    # the backend states the same order, for either layout
    cube = np.ascontiguousarray(np.transpose(tf, (1, 2, 0)))[..., None]
    for hr, layout in ((tf, 'tfirst'), (cube, 'cube')):
        syn = BE.recoarsen(hr, layout, [0], [method], s, te)[0][0]
        assert R.same_bits(syn, want)
    # a contiguous (H1, H2, HT) array: numpy's order differs, within the
    # counted bound (no NaN here: nansum / max agree on where they are)
    clean = np.nan_to_num(np.transpose(tf, (1, 2, 0)), nan=1.0)
    a = R.coarsen_contiguous(clean, s, te, method)
    b = R.fixed_order(clean, s, te, method)
    scale = te if method == 'total' else 1
    bound = (s * s + te) * 2.0 ** -24 * np.abs(clean).max() * scale
    assert np.abs(a.astype(np.float64) - b).max() <= bound


def test_unknown_method_and_factors():
    x = np.zeros((6, 6, 8, 1), np.float32)
    with pytest.raises(KeyError, match='Did not recognize temporal_coarsening'):
        BE.recoarsen(x, 'cube', [0], ['median'], 3, 4)
    with pytest.raises(ValueError, match='s_enhance must evenly divide'):
        BE.recoarsen(x, 'cube', [0], ['total'], 4, 4)
    with pytest.raises(ValueError, match='t_enhance must evenly divide'):
        BE.recoarsen(x, 'cube', [0], ['total'], 3, 3)


# ----------------------------------------------------- test_qa on arrays
def _source(seed=0, shape=(8, 8, 8), names=('u_100m', 'v_100m', 'pressure_0m')):
    rng = np.random.default_rng(seed)
    arrays = {n: rng.standard_normal(shape).astype(np.float32) * 5
              for n in names}
    lat = np.linspace(40, 39, shape[0])[:, None] * np.ones((1, shape[1]))
    lon = np.ones((shape[0], 1)) * np.linspace(-105, -104, shape[1])[None]
    ti = pd.date_range('2020-01-01', periods=shape[2], freq='h')
    return D.DeriveData(arrays, np.stack([lat, lon], -1), ti)


def _hi_res(src, feats=FEATS, seed=1):
    """a 3x / 4x 'forward pass' of the source: repeat + noise, time-first"""
    rng = np.random.default_rng(seed)
    out = {}
    for f in feats:
        lr = np.asarray(src[f])
        hr = lr.repeat(S, 0).repeat(S, 1).repeat(TE, 2)
        hr = hr + rng.standard_normal(hr.shape).astype(np.float32)
        out[f] = np.ascontiguousarray(np.transpose(hr, (2, 0, 1)))
    return out


def _outputs(tmp_path, kind, hr):
    """the three forms of ``out_file_path``"""
    if kind == 'nc':
        return dict(hr)
    if kind == 'h5':
        return {k: v.reshape(v.shape[0], -1) for k, v in hr.items()}
    cube = np.stack([np.transpose(hr[f], (1, 2, 0)) for f in hr], -1)
    fp = str(tmp_path / 'out_0.npz')
    NpzOutputHandler._write_output(cube, list(hr), None, None, fp)
    return fp


@pytest.mark.parametrize('kind', ['nc', 'h5', 'npz'])
def test_qa(tmp_path, kind):
    src = _source()
    hr = _hi_res(src)
    qa_fp = str(tmp_path / 'qa.npz')
    with Q.Sup3rQa(src, _outputs(tmp_path, kind, hr), S, TE, 'subsample',
                   qa_fp=qa_fp, save_sources=True, backend=BE) as qa:
        assert qa.features == FEATS                       # features=None
        assert qa.output_names == FEATS and qa.source_features == FEATS
        assert qa.output_type == kind
        data = qa.get_dset_out(qa.features[0])
        assert data.shape == (24, 24, 32)
        data = qa.coarsen_data(0, qa.features[0], data)
        assert isinstance(qa.time_index, pd.DatetimeIndex)
        assert qa.meta.shape == (64, 2)
        assert data.shape == tuple(qa.input_handler.data.shape)
        errors = qa.run()
        assert os.path.exists(qa_fp) and not os.path.exists(qa_fp + '.tmp.npz')
        with np.load(qa_fp) as qa_out:
            assert np.array_equal(qa_out['meta'], qa.meta)
            assert np.array_equal(qa_out['time_index'],
                                  np.asarray(qa.time_index).astype('int64'))
            for idf, dset in enumerate(qa.features):
                qa_true = qa_out[dset + '_true']
                assert qa_true.shape == (8, 64) and qa_true.dtype == np.float32
                source = np.asarray(qa.input_handler.data[dset]).transpose(
                    2, 0, 1).flatten()
                fwp = np.transpose(hr[dset], axes=(1, 2, 0))
                fwp = qa.coarsen_data(idf, dset, fwp)
                assert R.same_bits(fwp, R.numpy_path(hr[dset], S, TE,
                                                     'subsample'))
                fwp = np.transpose(fwp, axes=(2, 0, 1)).flatten()
                assert np.array_equal(qa_true.flatten(), source)
                assert np.array_equal(qa_out[dset + '_synthetic'].flatten(),
                                      fwp)
                assert np.array_equal(qa_out[dset + '_error'].flatten(),
                                      fwp - source)
                assert np.array_equal(
                    errors[dset].transpose(2, 0, 1).flatten(), fwp - source)
                st = qa.error_stats[dset]
                e = (fwp - source).astype(np.float64)
                assert st['count'] == e.size
                np.testing.assert_allclose(
                    [st['bias'], st['mae'], st['rmse'], st['max_abs']],
                    [e.mean(), np.abs(e).mean(), np.sqrt((e * e).mean()),
                     np.abs(e).max()], rtol=1e-12)
    assert qa.output_handler is None                      # closed


def test_qa_methods_per_feature_names_and_export(tmp_path):
    src = _source()
    hr = _hi_res(src)
    out = {'U_out': hr['u_100m'], 'V_out': hr['v_100m'],
           'time_index': np.arange(32), 'meta': np.zeros((576, 2))}
    qa_fp = str(tmp_path / 'qa.npz')
    qa = Q.Sup3rQa(src, out, S, TE, ['average', 'max'],
                   features=['U_out', 'V_out'], source_features=FEATS,
                   output_names=['u', 'v'], qa_fp=qa_fp, save_sources=False,
                   backend=BE)
    assert Q.Sup3rQa(src, out, S, TE, 'total', source_features=FEATS,
                     backend=BE).features == ['U_out', 'V_out']
    errors = qa.run()
    for name, f, method in (('U_out', 'u_100m', 'average'),
                            ('V_out', 'v_100m', 'max')):
        want = R.numpy_path(hr[f], S, TE, method) - np.asarray(src[f])
        assert R.same_bits(errors[name], want)
    with np.load(qa_fp) as z:
        assert sorted(z.files) == ['meta', 'time_index', 'u_error', 'v_error']
    qa.export(qa_fp, errors['U_out'], 'extra', 'copy')
    with np.load(qa_fp) as z:
        assert np.array_equal(z['extra_copy'], z['u_error'])
        assert len(z.files) == 5


def test_qa_shape_mismatch_and_unknown_output(tmp_path):
    src = _source()
    hr = _hi_res(src)
    qa = Q.Sup3rQa(src, hr, S, 2, 'subsample', backend=BE)
    with pytest.raises(RuntimeError) as e:
        qa.run()
    assert str(e.value) == (
        'Sup3rQa failed while trying to inspect the "u_100m" feature. '
        'The source low-res data had shape (8, 8, 8) while the '
        're-coarsened synthetic data had shape (8, 8, 16).')
    with pytest.raises(TypeError, match='Did not recognize output file type'):
        Q.Sup3rQa(src, str(tmp_path / 'out.h5'), S, TE, 'subsample',
                  backend=BE)
    with pytest.raises(KeyError, match='Did not recognize temporal_coarsening'):
        Q.Sup3rQa(src, hr, S, TE, 'median', backend=BE).run()
    with pytest.raises(TypeError, match='npz'):
        Q.Sup3rQa(src, hr, S, TE, 'subsample', qa_fp='qa.h5', backend=BE)


def _scale_bc(data, lat_lon, feature_name, scalar, adder,
              lr_padded_slice=None):
    """a transform with the call of ``local_linear_bc``"""
    assert lat_lon.shape == (8, 8, 2) and lr_padded_slice is None
    return data * np.float32(scalar) + np.float32(adder)


def test_qa_bias_correction_of_one_feature():
    src, plain = _source(), _source()
    hr = _hi_res(src)
    kwargs = {'U_100m': {'feature_name': 'u_100m', 'scalar': 2.0,
                         'adder': 1.0}}
    qa = Q.Sup3rQa(src, hr, S, TE, 'subsample', bias_correct_method=_scale_bc,
                   bias_correct_kwargs=kwargs, backend=BE)
    errors = qa.run()
    u = np.asarray(plain['u_100m']) * np.float32(2) + np.float32(1)
    assert R.same_bits(errors['u_100m'],
                       R.numpy_path(hr['u_100m'], S, TE, 'subsample') - u)
    assert R.same_bits(errors['v_100m'],
                       R.numpy_path(hr['v_100m'], S, TE, 'subsample')
                       - np.asarray(plain['v_100m']))
    # a feature of the kwargs that is not there needs a derive method
    with pytest.raises(AssertionError, match='need to be derived prior to '
                       'bias correction, but the input_handler has no derive'):
        Q.Sup3rQa(_source(), hr, S, TE, 'subsample',
                  bias_correct_method=_scale_bc,
                  bias_correct_kwargs={'windspeed_100m': {}}, backend=BE)


def test_qa_feature_that_has_to_be_derived():
    src = _source()
    ws = np.hypot(np.asarray(src['u_100m']), np.asarray(src['v_100m']))
    rng = np.random.default_rng(5)
    hr = ws.repeat(S, 0).repeat(S, 1).repeat(TE, 2)
    hr = (hr + rng.standard_normal(hr.shape)).astype(np.float32)
    out = {'windspeed_100m': np.ascontiguousarray(hr.transpose(2, 0, 1))}
    qa = Q.Sup3rQa(src, out, S, TE, 'average', backend=BE)
    assert isinstance(qa.input_handler, D.DeviceDeriver)
    errors = qa.run()
    want = R.numpy_path(out['windspeed_100m'], S, TE, 'average')
    got_ws = np.asarray(qa.input_handler['windspeed_100m'])
    np.testing.assert_allclose(got_ws, ws, rtol=1e-6)
    assert R.same_bits(errors['windspeed_100m'], want - got_ws)
    # ... and through a deriver handed in, bias-corrected after deriving
    deriver = D.DeviceDeriver(_source(), ['u_100m', 'v_100m'],
                              backend=D.NumpyBackend())
    qa = Q.Sup3rQa(deriver, out, S, TE, 'average',
                   bias_correct_method=_scale_bc, bias_correct_kwargs={
                       'windspeed_100m': {'feature_name': 'w', 'scalar': 0.5,
                                          'adder': 0.0}}, backend=BE)
    got = np.asarray(qa.input_handler['windspeed_100m'])
    np.testing.assert_allclose(got, ws * 0.5, rtol=1e-6)


# ------------------------------------------- the reference's utilities tests
def test_continuous_dist():
    a = np.linspace(-6, 6, 10)
    counts, centers = Q.continuous_dist(a, bins=20, range=[-10, 10],
                                        backend=BE)
    assert not all(np.isnan(counts))
    assert centers[0] < -9.0
    assert centers[-1] > 9.0
    c2, x2 = R.continuous_dist(a, bins=20, range=[-10, 10])
    assert np.array_equal(counts, c2) and np.array_equal(centers, x2)
    c3, _ = Q.continuous_dist(a, backend=BE)              # bins=None
    assert np.array_equal(c3, R.continuous_dist(a)[0])


@pytest.mark.parametrize('name', ['direct_dist', 'gradient_dist',
                                  'time_derivative_dist'])
def test_dist_smoke(name):
    a = np.random.default_rng(0).random((10, 10))
    got = getattr(Q, name)(a, backend=BE)
    want = getattr(R, name)(a)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    b = np.random.default_rng(1).random((6, 7, 9)).astype(np.float32) * 360
    got = getattr(Q, name)(b, bins=12, scale=3, period=360, interpolate=True,
                           backend=BE)
    want = getattr(R, name)(b, bins=12, scale=3, period=360, interpolate=True)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


@pytest.mark.parametrize('name', ['tke_frequency_spectrum',
                                  'tke_wavenumber_spectrum'])
def test_uv_spectrum_smoke(name):
    rng = np.random.default_rng(2)
    u, v = rng.random((10, 10)), rng.random((10, 10))
    (x, E), (x2, E2) = getattr(Q, name)(u, v, backend=BE), getattr(R, name)(u, v)
    assert np.array_equal(x, x2) and E.shape == E2.shape
    np.testing.assert_allclose(E, E2, rtol=1e-12)


@pytest.mark.parametrize('name', ['frequency_spectrum', 'wavenumber_spectrum'])
def test_spectrum_smoke(name):
    ke = np.random.default_rng(3).random((10, 10))
    (x, E), (x2, E2) = getattr(Q, name)(ke, backend=BE), getattr(R, name)(ke)
    assert np.array_equal(x, x2)
    np.testing.assert_allclose(E, E2, rtol=1e-12)
    if name == 'wavenumber_spectrum':
        x, E = Q.wavenumber_spectrum(ke, x_range=[0.1, 2.0], axis=1,
                                     backend=BE)
        x2, E2 = R.wavenumber_spectrum(ke, x_range=[0.1, 2.0], axis=1)
        assert np.array_equal(x, x2)
        np.testing.assert_allclose(E, E2, rtol=1e-12)
    else:
        var = np.random.default_rng(4).random((7, 12, 9))
        x, E = Q.frequency_spectrum(var, backend=BE)
        np.testing.assert_allclose(E, R.frequency_spectrum(var)[1], rtol=1e-12)


# ------------------------------------- the kernels' select and bin index
def _same_scalar(a, b):
    return np.asarray(a).dtype == np.asarray(b).dtype and \
        np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 255, 256, 257, 4099])
def test_select_is_np_percentile(n):
    rng = np.random.default_rng(n)
    cases = [np.abs(rng.standard_normal(n)).astype(np.float32),
             np.full(n, 1.5, np.float32),
             # values that differ in the lowest mantissa bit only
             (np.float32(1) + rng.integers(0, 2, n).astype(np.float32)
              * np.float32(2.0 ** -23)).astype(np.float32),
             np.abs(np.array([0.0, -0.0] * n, np.float32)[:n]),
             (rng.integers(0, 50, n).astype(np.uint32)).view(np.float32)]
    for x in cases:
        for q in (0, 50, 99.9, 100):
            assert _same_scalar(BE.percentile(x, q), np.percentile(x, q)), q


@pytest.mark.parametrize('bins', [1, 40, 4096])
@pytest.mark.parametrize('rng_', [None, (-1.0, 1.5), (0, 2)])
def test_bin_index_is_np_histogram(bins, rng_):
    rng = np.random.default_rng(bins)
    x = rng.standard_normal(5000).astype(np.float32)
    lo, hi = (x.min(), x.max()) if rng_ is None else rng_
    edges = np.histogram(x, bins=bins, range=rng_)[1].astype(np.float32)
    planted = np.concatenate([edges, np.nextafter(edges, np.float32(-9)),
                              np.nextafter(edges, np.float32(9))])
    x = np.concatenate([x, planted[(planted >= lo) | (rng_ is not None)]])
    x = x if rng_ is not None else x[(x >= lo) & (x <= hi)]
    got, e = BE.histogram(x, bins, rng_)
    want, e2 = np.histogram(x, bins=bins, range=rng_)
    assert e.dtype == e2.dtype and np.array_equal(e, e2)
    assert np.array_equal(got, want)
    one = np.full(7, 3.25, np.float32)                    # min = max
    assert np.array_equal(BE.histogram(one, bins, None)[0],
                          np.histogram(one, bins=bins)[0])
