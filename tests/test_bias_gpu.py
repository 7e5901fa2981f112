"""GPU tests (``-m gpu``) of the device bias correction: ``s3_bias_correct``
(through ``DeviceBiasCorrection.correct``, a thin ctypes wrapper) against the
numpy restatement ``tests/bias_ref.py``, the executor's fused normalisation,
``ArrayStrategy(bias_correct_method=...)`` end to end and the non-finite
error.

Tolerance rule for everything that is not bit-identical: the restatement is
evaluated in float64 (``R64``) and with every input and intermediate in
float32 (``R32``) on the test's own inputs; the device result must lie within
``2 * max|R32 - R64|`` of ``R64`` (a different association or a fused
multiply-add can double a rounding error but not more), and the bound never
goes below one float32 ulp of the result.  Each case prints the two figures
(``profiles/bias/NOTES.md`` records them)."""
import json
import os

import numpy as np
import pandas as pd
import pytest

from tests import bias_ref as R

pytestmark = pytest.mark.gpu

CFG = os.path.join(os.path.dirname(__file__), '..', 'sup3r_amd', 'configs')

T = 10
#: four chunks of one padded shape (6, 6, T) cut from a (12, 10) domain:
#: interior; the pad-(1, 0) / (0, 1) pair (space and time); a ragged corner
#: whose 3 x 2 window is reflected more than once
CHUNKS = [
    ((slice(2, 8), slice(1, 7)), ((0, 0), (0, 0), (0, 0))),
    ((slice(0, 5), slice(0, 6)), ((1, 0), (0, 0), (2, 0))),
    ((slice(7, 12), slice(4, 10)), ((0, 1), (0, 0), (0, 2))),
    ((slice(9, 12), slice(7, 10)), ((1, 2), (2, 1), (1, 1))),
]


def _times(start, freq, chunks=CHUNKS):
    """per chunk the time index of its un-padded window"""
    return [pd.date_range(start, periods=T - p[2][0] - p[2][1], freq=freq)
            for _, p in chunks]


def _windows(rng, tis, lo=-3.0, hi=3.0, chunks=CHUNKS):
    return [rng.uniform(lo, hi, (sl[0].stop - sl[0].start,
                                 sl[1].stop - sl[1].start,
                                 len(ti))).astype(np.float32)
            for (sl, _), ti in zip(chunks, tis)]


def _device(method, kw, windows, tis, chunks=CHUNKS):
    from sup3r_amd import bias as B
    bc = B.DeviceBiasCorrection(method, {'f': dict(kw)}, ['f'])
    x = np.stack([np.pad(w, p, mode='reflect')
                  for w, (_, p) in zip(windows, chunks)])[..., None]
    wins = [B.ChunkWindow(sl, p, ti) for (sl, p), ti in zip(chunks, tis)]
    y, counts = bc.correct(bc.dev.to_device(x), wins)
    return y.cpu().numpy()[..., 0], int(counts.cpu().numpy()[0])


def _ref(method, kw, windows, tis, dtype, chunks=CHUNKS):
    out = []
    for w, (sl, p), ti in zip(windows, chunks, tis):
        kws = {k: v for k, v in kw.items() if k != 'threshold'}
        if method != 'global_linear_bc':
            kws.update(feature_name='f', lr_padded_slice=sl)
        if method not in ('global_linear_bc', 'local_linear_bc'):
            kws['date_range_kwargs'] = ti
        out.append(R.pad_after(R.FUNCTIONS[method], w, p, dtype=dtype,
                               **kws))
    return np.stack(out)


def _within_rule(name, dev, r32, r64):
    """the tolerance rule of this file's docstring; prints the figures"""
    assert r32.dtype == np.float32 and r64.dtype == np.float64
    ref_err = float(np.abs(r32.astype(np.float64) - r64).max())
    ulp = np.spacing(np.abs(r64).astype(np.float32)).astype(np.float64)
    bound = np.maximum(2 * ref_err, ulp)
    err = np.abs(dev.astype(np.float64) - r64)
    scale = max(float(np.abs(r64).max()), 1e-30)
    print(f'[bias tolerance] {name}: max|R32-R64| = {ref_err:.3e} '
          f'({ref_err / scale:.2e} rel), device max err = '
          f'{float(err.max()):.3e} ({float(err.max()) / scale:.2e} rel), '
          f'device == R32 bitwise: {bool(np.array_equal(dev, r32))}')
    assert np.isfinite(r64).all() and np.isfinite(dev).all()
    worst = float((err - bound).max())
    assert worst <= 0, (name, worst, ref_err)


def _linear_fp(rng, months=12):
    fp = R.seeded_linear_tables(rng, (12, 10), feature='f', months=months)
    return fp


# ------------------------------------------------------------ linear kinds
@pytest.mark.parametrize('case', [
    'const_2d', 'const_3d', 'const_out_range', 'month', 'month_every_clamp',
    'global', 'const_smoothing', 'month_smoothing', 'avg_smoothing'])
def test_linear_kinds_are_bit_identical_to_the_float32_restatement(case):
    rng = np.random.default_rng(100)
    tis = _times('2015-01-30 00:00', '12h')         # January into February
    assert len({m for ti in tis for m in ti.month}) == 2
    windows = _windows(rng, tis)
    method, kw = 'local_linear_bc', {}
    if case == 'const_2d':
        kw = dict(bias_fp=_linear_fp(rng, months=0))
    elif case == 'const_3d':
        kw = dict(bias_fp=_linear_fp(rng))
    elif case == 'const_out_range':
        kw = dict(bias_fp=_linear_fp(rng), out_range=(1.5, -1.0))
    elif case == 'const_smoothing':
        kw = dict(bias_fp=_linear_fp(rng), smoothing=1.5)
    elif case == 'global':
        method, kw = 'global_linear_bc', dict(scalar=1.3, adder=-0.7,
                                              out_range=(-2, 2))
    else:
        method = 'monthly_local_linear_bc'
        kw = dict(bias_fp=_linear_fp(rng), temporal_avg=False)
        if case == 'month_every_clamp':
            kw.update(scalar_range=(0.9, 1.2), adder_range=(1.0, -1.0),
                      out_range=(-2.5, 2.5))
        elif case == 'month_smoothing':
            kw.update(smoothing=1.0)
        elif case == 'avg_smoothing':
            kw.update(temporal_avg=True, smoothing=1.0, out_range=(-3, 3))
    dev, bad = _device(method, kw, windows, tis)
    ref = _ref(method, kw, windows, tis, np.float32)
    assert ref.dtype == np.float32 and bad == 0
    np.testing.assert_array_equal(dev, ref)
    raw = np.stack([np.pad(w, p, mode='reflect')
                    for w, (_, p) in zip(windows, CHUNKS)])
    assert np.abs(dev - raw).max() > 0.1            # something was corrected


def test_linear_nan_factor_propagates_like_numpy():
    rng = np.random.default_rng(101)
    tis = _times('2015-03-01', '6h')
    windows = _windows(rng, tis)
    fp = _linear_fp(rng)
    fp['f_scalar'][3, 3, :] = np.nan
    kw = dict(bias_fp=fp, temporal_avg=False, scalar_range=(0.9, 1.2),
              out_range=(-2, 2))
    with pytest.warns(UserWarning, match='had NaNs'):
        dev, bad = _device('monthly_local_linear_bc', kw, windows, tis)
    with pytest.warns(UserWarning, match='had NaNs'):
        ref = _ref('monthly_local_linear_bc', kw, windows, tis, np.float32)
    np.testing.assert_array_equal(dev, ref)          # NaN == NaN here
    assert bad == int(np.isnan(ref).sum()) > 0


def test_monthly_temporal_avg_within_the_tolerance_rule():
    rng = np.random.default_rng(102)
    tis = _times('2015-01-30 00:00', '12h')
    windows = _windows(rng, tis)
    kw = dict(bias_fp=_linear_fp(rng), temporal_avg=True,
              scalar_range=(0.8, 1.3), out_range=(-3.5, 3.5))
    dev, bad = _device('monthly_local_linear_bc', kw, windows, tis)
    assert bad == 0
    _within_rule('monthly temporal_avg',
                 dev, _ref('monthly_local_linear_bc', kw, windows, tis,
                           np.float32),
                 _ref('monthly_local_linear_bc', kw, windows, tis,
                      np.float64))


# ----------------------------------------------------------- QDM / PresRat
def _qdm_inputs(seed, presrat=False, n_q=101):
    rng = np.random.default_rng(seed)
    fp = R.seeded_qdm_tables(rng, (12, 10), n_windows=4, n_q=n_q,
                             feature='f', base_dset='obs', presrat=presrat)
    # doy 87 .. 96: the windows' boundary (doy 91.25) lies inside every chunk
    tis = _times('2015-03-28', '1D')
    idx = R.closest_time_idx(tis[0], fp['time_window_center'])
    assert set(idx) == {0, 1}
    # inside the future distribution's range and beyond both of its ends
    windows = _windows(rng, tis, lo=1.0, hi=70.0)
    return fp, tis, windows


QDM_CASES = {
    'relative': dict(),
    'absolute': dict(relative=False),
    'relative_no_trend': dict(no_trend=True),
    'absolute_no_trend': dict(relative=False, no_trend=True),
    'relative_delta_range': dict(delta_range=(0.9, 1.05)),
    'absolute_delta_range': dict(relative=False, delta_range=(2.0, -1.0)),
    'relative_denom_min': dict(delta_denom_min=8.0),
    'relative_denom_zero_and_min': dict(delta_denom_zero=3.0,
                                        delta_denom_min=2.0),
    'relative_out_range': dict(out_range=(5.0, 30.0)),
    'absolute_out_range': dict(relative=False, out_range=(30.0, 5.0)),
}


@pytest.mark.parametrize('case', sorted(QDM_CASES))
def test_qdm_within_the_tolerance_rule(case):
    fp, tis, windows = _qdm_inputs(200)
    if case == 'relative_denom_zero_and_min':
        # sites whose historical distribution is all zero
        fp['bias_f_params'][::3, ::2] = 0
    kw = dict(QDM_CASES[case], bias_fp=fp, base_dset='obs')
    dev, bad = _device('local_qdm_bc', kw, windows, tis)
    assert bad == 0
    r32 = _ref('local_qdm_bc', kw, windows, tis, np.float32)
    r64 = _ref('local_qdm_bc', kw, windows, tis, np.float64)
    _within_rule(f'qdm {case}', dev, r32, r64)
    raw = np.stack([np.pad(w, p, mode='reflect')
                    for w, (_, p) in zip(windows, CHUNKS)])
    beyond = (raw < fp['bias_fut_f_params'][..., 0].min()).sum() + \
        (raw > fp['bias_fut_f_params'][..., -1].max()).sum()
    assert beyond > 0                      # data beyond both table ends
    if 'out_range' in case:
        assert (dev == 5.0).any() and (dev == 30.0).any()


def test_qdm_repeated_knots_and_data_on_the_repeated_value():
    fp, tis, windows = _qdm_inputs(201, n_q=21)
    for key in ('bias_fut_f_params', 'bias_f_params', 'base_obs_params'):
        tab = fp[key]
        tab[..., 4:9] = tab[..., 4:5]                # five equal knots
        tab[..., 0:2] = tab[..., 0:1]                # ... and at the low end
    for w, (sl, _) in zip(windows, CHUNKS):
        # every window's first steps sit exactly on repeated knots / the ends
        rows = fp['bias_fut_f_params'][sl]
        w[:, :, 0] = rows[:, :, 0, 4]
        w[:, :, 1] = rows[:, :, 0, 0]
        w[:, :, 2] = rows[:, :, 0, -1]
    for relative in (True, False):
        kw = dict(bias_fp=fp, base_dset='obs', relative=relative)
        dev, bad = _device('local_qdm_bc', kw, windows, tis)
        assert bad == 0
        _within_rule(f'qdm repeated knots relative={relative}', dev,
                     _ref('local_qdm_bc', kw, windows, tis, np.float32),
                     _ref('local_qdm_bc', kw, windows, tis, np.float64))


@pytest.mark.parametrize('case', ['relative', 'absolute', 'k_range',
                                  'no_trend', 'out_range'])
def test_presrat_within_the_tolerance_rule(case):
    fp, tis, windows = _qdm_inputs(202, presrat=True)
    kw = dict(bias_fp=fp, base_dset='obs')
    kw.update({'relative': {}, 'absolute': dict(relative=False),
               'k_range': dict(k_range=(0.95, 1.1)),
               'no_trend': dict(no_trend=True),
               'out_range': dict(out_range=(0.0, 25.0))}[case])
    dev, bad = _device('local_presrat_bc', kw, windows, tis)
    assert bad == 0
    _within_rule(f'presrat {case}', dev,
                 _ref('local_presrat_bc', kw, windows, tis, np.float32),
                 _ref('local_presrat_bc', kw, windows, tis, np.float64))
    if case != 'no_trend':
        # the zero rate: values below tau_fut became 0, the rest were scaled
        assert (dev == 0).any() and (dev > 0).any()
    else:
        assert (dev > 0).all()


def test_reference_properties_hold_on_the_device():
    """tests/bias/test_qdm_bias_correction.py:266-452 of the reference, on the
    device result"""
    fp, tis, windows = _qdm_inputs(203)
    # (np.allclose's default rtol = 1e-5 is relative to the RESULT, a float32
    # evaluation's error to the table values: lift the distributions so that
    # data - 10 stays away from zero — [26, ~85] instead of [1, ~60])
    for key in ('bias_fut_f_params', 'bias_f_params', 'base_obs_params'):
        fp[key] = fp[key] + np.float32(25)
    fut, hist = fp['bias_fut_f_params'], fp['bias_f_params']
    # keep the data inside the future distribution: outside it the mapping
    # clamps, and only a shift of all three distributions is a shift there
    for w, (sl, _) in zip(windows, CHUNKS):
        lo = fut[sl][..., 0].max(-1)[..., None]
        hi = fut[sl][..., -1].min(-1)[..., None]
        w[...] = lo + (hi - lo) * (w - 1.0) / 69.0
    raw = np.stack([np.pad(w, p, mode='reflect')
                    for w, (_, p) in zip(windows, CHUNKS)])

    def run(**kw):
        names = dict(base_obs_params=kw.pop('base', fp['base_obs_params']),
                     bias_f_params=kw.pop('bias', hist),
                     bias_fut_f_params=kw.pop('bias_fut', fut))
        dev, bad = _device('local_qdm_bc', dict(
            kw, bias_fp=dict(fp, **names), base_dset='obs'), windows, tis)
        assert bad == 0
        return dev
    for relative in (True, False):
        assert np.allclose(run(no_trend=True, relative=relative),
                           run(bias_fut=hist, relative=relative))
        assert np.allclose(run(base=fut, bias=fut, relative=relative), raw)
    ten = np.float32(10)
    assert np.allclose(run(base=fut - ten, bias=fut, relative=False),
                       raw - 10)
    assert np.allclose(run(base=fut, bias=fut - ten, relative=False),
                       raw + 10)
    assert np.allclose(run(base=fut - ten, bias=fut - ten, relative=False),
                       raw)


# ------------------------------- pass-through channels, normalisation, ABI
@pytest.mark.parametrize('stats', ['none', 'fp32', 'fp64'])
def test_channels_without_a_descriptor_pass_through_normalised(stats):
    """four channels, one corrected; 300 time steps = two LDS segments of the
    kernel; the normalisation is s3_chunk_time_first's (numpy's) arithmetic"""
    from sup3r_amd import bias as B
    rng = np.random.default_rng(300)
    fp = R.seeded_linear_tables(rng, (5, 4), feature='c')
    ti = pd.date_range('2015-01-01', periods=300, freq='1D')
    x = rng.uniform(-3, 3, (2, 5, 4, 300, 4)).astype(np.float32)
    bc = B.DeviceBiasCorrection(
        'monthly_local_linear_bc',
        {'c': dict(bias_fp=fp, temporal_avg=False)}, ['a', 'b', 'c', 'd'])
    wins = [B.ChunkWindow((slice(0, 5), slice(0, 4)), None, ti)] * 2
    mean = std = None
    if stats != 'none':
        dt = np.float32 if stats == 'fp32' else np.float64
        mean = np.array([0.1, -0.2, 0.3, 0.05], dtype=dt)
        std = np.array([1.5, 0.7, 2.25, 1.1], dtype=dt)
    xd = bc.dev.to_device(x)
    out = bc.dev.empty(x.shape)
    y, counts = bc.correct(xd, wins, out=out, mean=mean, std=std,
                           stats_fp32=stats == 'fp32')
    want = x.copy()
    for k in range(2):
        want[k, ..., 2] = R.monthly_local_linear_bc(
            x[k, ..., 2], 'c', fp, ti, temporal_avg=False, dtype=np.float32)
    if stats != 'none':
        want = ((want - mean) / std).astype(np.float32)
    np.testing.assert_array_equal(y.cpu().numpy(), want)
    np.testing.assert_array_equal(xd.cpu().numpy(), x)     # x untouched
    assert not counts.cpu().numpy().any()


def test_inconsistent_extents_are_refused():
    from sup3r_amd import bias as B
    rng = np.random.default_rng(301)
    fp = R.seeded_linear_tables(rng, (5, 4), feature='f', months=0)
    bc = B.DeviceBiasCorrection('local_linear_bc', {'f': dict(bias_fp=fp)},
                                ['f'])
    x = bc.dev.to_device(rng.standard_normal((1, 4, 4, 3, 1)))
    # a window that leaves the factor tables
    with pytest.raises(RuntimeError, match='leaves the factor tables'):
        bc.correct(x, [B.ChunkWindow((slice(3, 7), slice(0, 4)))])
    # a month index is needed but no time index was given
    fp3 = R.seeded_linear_tables(rng, (5, 4), feature='f')
    bc = B.DeviceBiasCorrection(
        'monthly_local_linear_bc',
        {'f': dict(bias_fp=fp3, temporal_avg=False)}, ['f'])
    with pytest.raises(ValueError, match='low-res time index'):
        bc.correct(x, [B.ChunkWindow((slice(0, 4), slice(0, 4)))])
    with pytest.raises(ValueError, match='expected 1 channels'):
        bc.correct(bc.dev.empty((1, 4, 4, 3, 2)),
                   [B.ChunkWindow((slice(0, 4), slice(0, 4)))])


def test_public_functions_host_and_device_round_trip():
    import torch

    import sup3r_amd as S
    rng = np.random.default_rng(302)
    lat = np.linspace(45, 40, 9)[:, None] + np.zeros((1, 8))
    lon = np.linspace(-110, -104, 8)[None] + np.zeros((9, 1))
    fp = R.seeded_linear_tables(rng, (9, 8), feature='u_10m')
    src = dict(fp, latitude=lat, longitude=lon)
    dom = np.stack([lat[2:8, 1:7], lon[2:8, 1:7]], -1)       # 6 x 6 domain
    cut = {k: v[2:8, 1:7] for k, v in fp.items()}
    ti = pd.date_range('2015-01-30', periods=7, freq='12h')
    data = rng.uniform(-3, 3, (4, 5, 7)).astype(np.float32)
    sl = (slice(1, 5), slice(0, 5))
    got = S.monthly_local_linear_bc(data, dom, 'u_10m', src, ti,
                                    lr_padded_slice=sl, temporal_avg=False,
                                    out_range=(-2, 2))
    assert isinstance(got, np.ndarray) and got.dtype == np.float32
    np.testing.assert_array_equal(got, R.monthly_local_linear_bc(
        data, 'u_10m', cut, ti, lr_padded_slice=sl, temporal_avg=False,
        out_range=(-2, 2)))
    # date_range_kwargs as the reference passes them
    kws = dict(start='2015-01-30 00:00:00', end='2015-02-02 00:00:00',
               freq='12h')
    np.testing.assert_array_equal(got, S.monthly_local_linear_bc(
        data, dom, 'u_10m', src, kws, lr_padded_slice=sl, temporal_avg=False,
        out_range=(-2, 2)))
    from sup3r_amd.engine import Device
    dev = Device.get()
    t = dev.to_device(data)
    got_t = S.local_linear_bc(t, dom, 'u_10m', src, lr_padded_slice=sl)
    assert isinstance(got_t, torch.Tensor) and got_t.is_cuda
    np.testing.assert_array_equal(t.cpu().numpy(), data)    # input untouched
    np.testing.assert_array_equal(got_t.cpu().numpy(), R.local_linear_bc(
        data, 'u_10m', cut, lr_padded_slice=sl))
    np.testing.assert_array_equal(
        S.global_linear_bc(data, 1.25, 0.5, out_range=(0, 2)),
        R.global_linear_bc(data, 1.25, 0.5, out_range=(0, 2)))
    with pytest.raises(RuntimeError, match='threshold'):
        S.local_linear_bc(data, dom + 0.3, 'u_10m', src, lr_padded_slice=sl)
    # QDM / PresRat through the functions, full domain, no slice
    q = R.seeded_qdm_tables(rng, (4, 5), 4, 31, feature='rsds',
                            base_dset='ghi', presrat=True)
    days = pd.date_range('2015-03-28', periods=7, freq='1D')
    pos = rng.uniform(2, 50, (4, 5, 7)).astype(np.float32)
    for name, kw in (('local_qdm_bc', dict(relative=False)),
                     ('local_presrat_bc', dict(k_range=(0.9, 1.1)))):
        got = getattr(S, name)(pos, None, 'ghi', 'rsds', q, days, **kw)
        _within_rule(f'function {name}', got,
                     R.FUNCTIONS[name](pos, 'ghi', 'rsds', q, days,
                                       dtype=np.float32, **kw),
                     R.FUNCTIONS[name](pos, 'ghi', 'rsds', q, days,
                                       dtype=np.float64, **kw))
    zero = dict(q, bias_rsds_params=np.zeros_like(q['bias_rsds_params']))
    with pytest.raises(RuntimeError, match='NaN / inf'):
        S.local_qdm_bc(pos, None, 'ghi', 'rsds', zero, days)


# ------------------------------------------------------------ the executor
FEATS = ['u_10m', 'v_10m']


def _model_5d(mean=0.2, std=1.25):
    """(``mean`` / ``std`` of about the data's: normalised input of order 1)"""
    from sup3r_amd import Sup3rGan
    Sup3rGan.seed(5)
    means = {f: np.float32(mean * (i + 1)) for i, f in enumerate(FEATS)}
    stds = {f: np.float32(std * (1 + 0.4 * i)) for i, f in enumerate(FEATS)}
    m = Sup3rGan(os.path.join(CFG, 'test_gen_st_2x_4x_2f.json'),
                 os.path.join(CFG, 'test_disc_st_same.json'), means=means,
                 stdevs=stds)
    m.set_model_params(lr_features=FEATS, hr_out_features=FEATS, s_enhance=2,
                       t_enhance=4)
    m.init_weights((1, 8, 8, 6, 2), (1, 16, 16, 24, 2))
    return m


def _model_4d(stat_dtype=np.float32):
    from sup3r_amd import Sup3rGan
    Sup3rGan.seed(9)
    means = {f: stat_dtype(0.3 * (i + 1)) for i, f in enumerate(FEATS)}
    stds = {f: stat_dtype(1.5 + 0.25 * i) for i, f in enumerate(FEATS)}
    m = Sup3rGan(os.path.join(CFG, 'test_gen_s_2x_2f.json'),
                 os.path.join(CFG, 'test_disc_s_same.json'), means=means,
                 stdevs=stds, precision='f32')
    m.set_model_params(lr_features=FEATS, hr_out_features=FEATS, s_enhance=2,
                       t_enhance=1)
    m.init_weights((1, 16, 16, 2), (1, 32, 32, 2))
    return m


def _identity(shape, feats):
    """scalar = 1, adder = 0 for every month: corrects nothing"""
    fp = {}
    for f in feats:
        fp[f'{f}_scalar'] = np.ones(shape + (12,), np.float32)
        fp[f'{f}_adder'] = np.zeros(shape + (12,), np.float32)
    return fp


def _run(strategy, batch=3):
    from sup3r_amd import ForwardPass
    done, kept = ForwardPass.run(strategy, 0, batch=batch, return_data=True)
    assert done == strategy.n_chunks
    return dict(kept)


def _on_device(strategy):
    """the group was corrected by s3_bias_correct inside the executor (the
    strategy's shared record holds the resident tables), not on the host
    route"""
    return any(k[0] == 'device' for k in strategy._bias_shared)


@pytest.mark.parametrize('kind', ['5d', '4d', '4d_fp64_stats'])
def test_identity_correction_is_bit_identical_to_no_correction(kind):
    """fused normalisation: with scalar = 1, adder = 0 and non-trivial means /
    stdevs the executor's output equals the same strategy without bias
    correction, bit for bit"""
    from sup3r_amd.forward_pass import register_model
    from sup3r_amd.strategy import ArrayStrategy
    rng = np.random.default_rng(400)
    if kind == '5d':
        m = _model_5d()
        domain = (rng.standard_normal((14, 11, 13, 2)) * 2 + 0.5).astype(
            np.float32)
        args = ((6, 5, 6),)
        pads = dict(spatial_pad=2, temporal_pad=2)
    else:
        m = _model_4d(np.float32 if kind == '4d' else np.float64)
        domain = (rng.standard_normal((44, 37, 9, 2)) * 2 + 0.4).astype(
            np.float32)
        args = ((22, 19, 5),)
        pads = dict(spatial_pad=2, temporal_pad=1)
    key = {'model_dir': f'bias-identity-{kind}'}
    register_model('Sup3rGan', key, m)
    ti = pd.date_range('2015-01-30', periods=domain.shape[2], freq='6h')
    fp = _identity(domain.shape[:2], FEATS)
    bck = {f: dict(bias_fp=fp, temporal_avg=False) for f in FEATS}
    plain = ArrayStrategy(domain, key, *args, model=m, **pads)
    for method, kws in (('monthly_local_linear_bc', bck),
                        ('local_linear_bc',
                         {f: dict(bias_fp=fp) for f in FEATS})):
        corrected = ArrayStrategy(
            domain, key, *args, model=m, bias_correct_method=method,
            bias_correct_kwargs=kws, input_time_index=ti, **pads)
        want, got = _run(plain), _run(corrected)
        assert _on_device(corrected)
        assert sorted(got) == sorted(want)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k])
        plain = ArrayStrategy(domain, key, *args, model=m, **pads)


def test_identity_correction_through_a_multi_step_chain_with_topography():
    """MultiStepGan([spatial 2x, spatial 5x + topography]) as in
    tests/test_forward_pass_gpu.py: only the first step's input is
    corrected"""
    from sup3r_amd import MultiStepGan, Sup3rGan
    from sup3r_amd.forward_pass import register_model
    from sup3r_amd.strategy import ArrayStrategy
    Sup3rGan.seed(19)
    f6 = ['u_10m', 'v_10m', 'u_100m', 'v_100m', 'u_200m', 'v_200m']
    st = {f: (0.1 * (i + 1), 1.0 + 0.25 * i) for i, f in enumerate(f6)}
    st['topography'] = (300.0, 150.0)
    means = {k: np.float32(v[0]) for k, v in st.items()}
    stds = {k: np.float32(v[1]) for k, v in st.items()}
    spec1 = json.load(open(os.path.join(CFG, 'sup3r/spatial/gen_2x_2f.json')))
    for layer in (spec1['hidden_layers'] if isinstance(spec1, dict)
                  else spec1):
        if layer.get('filters') == 2:
            layer['filters'] = 6
    m1 = Sup3rGan(spec1, os.path.join(CFG, 'test_disc_s_same.json'),
                  means=means, stdevs=stds, precision='bf16')
    m1.set_model_params(lr_features=f6, hr_out_features=f6, s_enhance=2,
                        t_enhance=1)
    m1.init_weights((1, 18, 17, 6), (1, 36, 34, 6))
    m2 = Sup3rGan(os.path.join(CFG, 'sup3r/sup3rcc/gen_wind_5x_1x_6f.json'),
                  os.path.join(CFG, 'test_disc_s_same.json'), means=means,
                  stdevs=stds, precision='bf16')
    m2.set_model_params(lr_features=f6 + ['topography'], hr_out_features=f6,
                        hr_exo_features=['topography'], s_enhance=5,
                        t_enhance=1)
    m2.init_weights((1, 36, 34, 7), (1, 180, 170, 7))
    ms = MultiStepGan([m1, m2])
    key = {'model_dirs': ['bias-s1', 'bias-s2']}
    register_model('MultiStepGan', key, ms)
    rng = np.random.default_rng(29)
    domain = (rng.standard_normal((32, 30, 5, 6)) * 2 + 0.4).astype(np.float32)
    topo_hr = (300 + 150 * rng.standard_normal((320, 300, 1))).astype(
        np.float32)
    topo_mid = topo_hr.reshape(64, 5, 60, 5, 1).mean(axis=(1, 3)).astype(
        np.float32)
    exo = {'topography': {'steps': [
        {'model': 1, 'combine_type': 'input', 'data': topo_mid,
         's_enhance': 2, 't_enhance': 1},
        {'model': 1, 'combine_type': 'layer', 'data': topo_hr,
         's_enhance': 10, 't_enhance': 1}]}}
    ti = pd.date_range('2015-01-31 12:00', periods=5, freq='6h')
    fp = _identity((32, 30), f6)

    def strategy(**kw):
        return ArrayStrategy(domain, key, (16, 15, 4), spatial_pad=1,
                             temporal_pad=1, exo_data=exo,
                             model_class='MultiStepGan', max_nodes=1,
                             model=ms, **kw)
    corrected = strategy(
        bias_correct_method='monthly_local_linear_bc',
        bias_correct_kwargs={f: dict(bias_fp=fp, temporal_avg=True)
                             for f in f6[:4]},
        input_time_index=ti)
    want, got = _run(strategy()), _run(corrected)
    assert _on_device(corrected) and len(want) == 8
    for k in want:
        np.testing.assert_array_equal(got[k], want[k])


def _reference_route(strategy_plain, model, method, kwargs, ti, batch=3):
    """``iter_chunks`` over chunks corrected one by one with tests/bias_ref.py
    in float32, then edge-padded like ``get_input_chunk``"""
    from sup3r_amd import ForwardPass
    fwp = ForwardPass(strategy_plain, 0)

    def chunks():
        for i in range(strategy_plain.n_chunks):
            c = strategy_plain.init_chunk(i)
            c.input_data = R.correct_chunk(c, method, kwargs,
                                           model.lr_features, ti)
            c.input_data, c.exo_data = fwp.pad_source_data(
                c.input_data, c.pad_width, c.exo_data)
            yield c
    return {c.index: np.array(d) for c, failed, d in
            ForwardPass.iter_chunks(chunks(), model, batch=batch)
            if not failed}


def test_strategy_end_to_end_monthly_and_qdm():
    """``ArrayStrategy`` + ``ForwardPass.run(return_data=True)`` equals
    ``iter_chunks`` over chunks corrected by the restatement.  The fp32
    generator's tolerance is the one tests/test_forward_pass_gpu.py uses for
    two fp32 routes that differ in rounding (``assert_allclose(rtol=0,
    atol=1e-4)`` in test_spatial_model_chunks_on_the_device_equal_the_
    generate_path); where the correction is bit-identical (per-step months)
    so is the output."""
    from sup3r_amd.forward_pass import register_model
    from sup3r_amd.strategy import ArrayStrategy
    m = _model_5d()
    key = {'model_dir': 'bias-e2e'}
    register_model('Sup3rGan', key, m)
    rng = np.random.default_rng(500)
    domain = (rng.standard_normal((14, 11, 13, 2)) * 2 + 0.5).astype(
        np.float32)
    args = dict(fwp_chunk_shape=(6, 5, 6), spatial_pad=2, temporal_pad=2,
                model=m)
    # 6-hourly from Jan 30 18:00: the month changes inside the padded windows
    ti = pd.date_range('2015-01-30 18:00', periods=13, freq='6h')
    lin = {}
    for f in FEATS:
        lin.update(R.seeded_linear_tables(rng, (14, 11), feature=f))
    for temporal_avg in (True, False):
        bck = {f: dict(bias_fp=lin, temporal_avg=temporal_avg,
                       out_range=(-4.0, 5.0)) for f in FEATS}
        st = ArrayStrategy(domain, key, **args,
                           bias_correct_method='monthly_local_linear_bc',
                           bias_correct_kwargs=bck, input_time_index=ti)
        months = [set(st.init_chunk(i).bias_correct.time_index.month)
                  for i in range(st.n_chunks)]
        assert any(len(s) == 2 for s in months)
        got = _run(st)
        assert _on_device(st)
        want = _reference_route(ArrayStrategy(domain, key, **args), m,
                                'monthly_local_linear_bc', bck, ti)
        plain = _run(ArrayStrategy(domain, key, **args))
        assert sorted(got) == sorted(want) == sorted(plain)
        for k in want:
            if temporal_avg:
                np.testing.assert_allclose(got[k], want[k], rtol=0, atol=1e-4)
            else:
                np.testing.assert_array_equal(got[k], want[k])
            assert np.abs(got[k] - plain[k]).max() > 1e-2
    # QDM on the first feature: daily steps across a time-window boundary
    m = _model_5d(mean=13.0, std=12.0)
    key = {'model_dir': 'bias-e2e-qdm'}
    register_model('Sup3rGan', key, m)
    args['model'] = m
    domain = rng.uniform(2.0, 50.0, (14, 11, 13, 2)).astype(np.float32)
    days = pd.date_range('2015-03-26', periods=13, freq='1D')
    q = R.seeded_qdm_tables(rng, (14, 11), 4, 101, feature='u_10m',
                            base_dset='u_obs')
    bck = {'u_10m': dict(bias_fp=q, base_dset='u_obs', relative=True,
                         out_range=(0.0, 80.0))}
    st = ArrayStrategy(domain, key, **args, bias_correct_method='local_qdm_bc',
                       bias_correct_kwargs=bck, input_time_index=days)
    got = _run(st)
    assert _on_device(st)
    want = _reference_route(ArrayStrategy(domain, key, **args), m,
                            'local_qdm_bc', bck, days)
    worst = 0.0
    for k in want:
        np.testing.assert_allclose(got[k], want[k], rtol=0, atol=1e-4)
        worst = max(worst, float(np.abs(got[k] - want[k]).max()))
    print(f'[bias e2e] local_qdm_bc executor vs restatement route: '
          f'max abs diff {worst:.3e}')


def test_host_route_for_a_model_that_normalises_for_itself():
    """an overridden ``norm_input``: the chunk is corrected with the public
    functions (window, then reflect padding) and goes on as before"""
    from sup3r_amd import Sup3rGan
    from sup3r_amd.forward_pass import register_model
    from sup3r_amd.strategy import ArrayStrategy

    class OwnNorm(Sup3rGan):
        def norm_input(self, low_res):
            return super().norm_input(low_res)
    m = _model_5d()
    m.__class__ = OwnNorm
    key = {'model_dir': 'bias-own-norm'}
    register_model('Sup3rGan', key, m)
    rng = np.random.default_rng(600)
    domain = rng.uniform(-3, 3, (14, 11, 13, 2)).astype(np.float32)
    ti = pd.date_range('2015-01-30 18:00', periods=13, freq='6h')
    lin = R.seeded_linear_tables(rng, (14, 11), feature='v_10m')
    bck = {'v_10m': dict(bias_fp=lin, temporal_avg=False)}
    args = dict(fwp_chunk_shape=(6, 5, 6), spatial_pad=2, temporal_pad=2,
                model=m)
    st = ArrayStrategy(domain, key, **args,
                       bias_correct_method='monthly_local_linear_bc',
                       bias_correct_kwargs=bck, input_time_index=ti)
    got = _run(st)
    assert not _on_device(st)
    want = _reference_route(ArrayStrategy(domain, key, **args), m,
                            'monthly_local_linear_bc', bck, ti)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k])


def test_relative_qdm_with_a_zero_denominator_raises_from_run():
    from sup3r_amd import ForwardPass
    from sup3r_amd.forward_pass import register_model
    from sup3r_amd.strategy import ArrayStrategy
    m = _model_5d(mean=13.0, std=12.0)
    key = {'model_dir': 'bias-nonfinite'}
    register_model('Sup3rGan', key, m)
    rng = np.random.default_rng(700)
    domain = rng.uniform(2.0, 50.0, (14, 11, 13, 2)).astype(np.float32)
    days = pd.date_range('2015-03-26', periods=13, freq='1D')
    q = R.seeded_qdm_tables(rng, (14, 11), 4, 21, feature='u_10m',
                            base_dset='u_obs')
    q['bias_u_10m_params'][...] = 0
    bck = {'u_10m': dict(bias_fp=q, base_dset='u_obs', relative=True)}
    args = dict(fwp_chunk_shape=(6, 5, 6), spatial_pad=2, temporal_pad=2,
                model=m, bias_correct_method='local_qdm_bc',
                input_time_index=days)
    with pytest.raises(RuntimeError, match='QDM bias correction resulted in '
                                           'NaN / inf values'):
        ForwardPass.run(ArrayStrategy(domain, key, bias_correct_kwargs=bck,
                                      **args), 0, return_data=True)
    # ... and delta_denom_zero makes the same run finite
    bck = {'u_10m': dict(bck['u_10m'], delta_denom_zero=5.0)}
    st = ArrayStrategy(domain, key, bias_correct_kwargs=bck, **args)
    assert ForwardPass.run(st, 0) == st.n_chunks


# ------------------------------------------- more than one launch per batch
def _many(n=33):
    """``n`` chunks of one padded shape, each with its own start time, so that
    chunk k's month / window / weight rows differ from chunk 0's"""
    chunks = (CHUNKS * (n // len(CHUNKS) + 1))[:n]
    return chunks


@pytest.mark.parametrize('case', ['month_smoothing', 'avg', 'qdm'])
def test_batches_of_more_than_32_chunks_are_split_into_launches(case):
    """33 chunks = two ``s3_bias_correct`` calls: the second one starts at
    chunk 32 of x, out, the month / window / weight arrays and the per-chunk
    tables"""
    from sup3r_amd import _lib
    chunks = _many(33)
    assert len(chunks) > _lib.BC_MAX_CHUNKS
    rng = np.random.default_rng(800)
    if case == 'qdm':
        fp = R.seeded_qdm_tables(rng, (12, 10), n_windows=4, n_q=31,
                                 feature='f', base_dset='obs')
        starts = pd.date_range('2015-03-20', periods=len(chunks), freq='2D')
        tis = [pd.date_range(s, periods=T - p[2][0] - p[2][1], freq='1D')
               for s, (_, p) in zip(starts, chunks)]
        windows = _windows(rng, tis, lo=1.0, hi=70.0, chunks=chunks)
        method, kw = 'local_qdm_bc', dict(bias_fp=fp, base_dset='obs')
    else:
        starts = pd.date_range('2015-01-25', periods=len(chunks), freq='3D')
        tis = [pd.date_range(s, periods=T - p[2][0] - p[2][1], freq='12h')
               for s, (_, p) in zip(starts, chunks)]
        windows = _windows(rng, tis, chunks=chunks)
        method = 'monthly_local_linear_bc'
        kw = dict(bias_fp=_linear_fp(rng), temporal_avg=case == 'avg')
        if case == 'month_smoothing':
            kw['smoothing'] = 1.0
    assert len({tuple(ti.month) for ti in tis}) > 3
    dev, bad = _device(method, kw, windows, tis, chunks=chunks)
    assert bad == 0 and dev.shape[0] == 33
    r32 = _ref(method, kw, windows, tis, np.float32, chunks=chunks)
    if case == 'month_smoothing':
        np.testing.assert_array_equal(dev, r32)
    else:
        _within_rule(f'33 chunks {case}', dev, r32,
                     _ref(method, kw, windows, tis, np.float64,
                          chunks=chunks))
    # the last chunk is not the first one's result
    assert np.abs(dev[32] - dev[0]).max() > 0


def test_presrat_raises_on_nan_only_qdm_on_inf_too():
    """bias_transforms.py:816 tests ``isfinite``, :1128 only ``isnan``: an
    infinite result (x / 0 with x > 0) raises from local_qdm_bc and passes
    local_presrat_bc, as in the restatement"""
    import sup3r_amd as S
    rng = np.random.default_rng(801)
    q = R.seeded_qdm_tables(rng, (4, 5), 4, 21, feature='rsds',
                            base_dset='ghi', presrat=True)
    q['bias_rsds_params'] = np.zeros_like(q['bias_rsds_params'])
    q['zero_rate_threshold'] = 0.0          # no floor: the denominator is 0
    q['rsds_tau_fut'] = np.zeros_like(q['rsds_tau_fut'])
    days = pd.date_range('2015-03-28', periods=7, freq='1D')
    pos = rng.uniform(2, 50, (4, 5, 7)).astype(np.float32)
    with pytest.raises(RuntimeError, match='NaN / inf'):
        S.local_qdm_bc(pos, None, 'ghi', 'rsds', q, days)
    want = R.local_presrat_bc(pos, 'ghi', 'rsds', q, days, dtype=np.float32)
    assert np.isinf(want).all()
    got = S.local_presrat_bc(pos, None, 'ghi', 'rsds', q, days)
    np.testing.assert_array_equal(got, want)


def test_identity_correction_with_an_input_exo_channel_5d():
    """a 5-D model whose last low-res feature is an 'input'-type exo field:
    the raw input is combined on the host, the kernel corrects the first
    channels and normalises all of them"""
    from sup3r_amd import Sup3rGan
    from sup3r_amd.configs.author_configs import pcc
    from sup3r_amd.forward_pass import register_model
    from sup3r_amd.strategy import ArrayStrategy
    feats = FEATS + ['topography']
    Sup3rGan.seed(31)
    means = {f: np.float32(0.2 * (i + 1)) for i, f in enumerate(feats)}
    stds = {f: np.float32(1.25 + 0.5 * i) for i, f in enumerate(feats)}
    m = Sup3rGan(pcc(3, 16) + pcc(3, 2, act=False),
                 os.path.join(CFG, 'test_disc_st_same.json'), means=means,
                 stdevs=stds)
    m.set_model_params(lr_features=feats, hr_out_features=FEATS, s_enhance=1,
                       t_enhance=1)
    m.init_weights((1, 8, 8, 6, 3), (1, 8, 8, 6, 2))
    assert m.is_5d
    key = {'model_dir': 'bias-exo-5d'}
    register_model('Sup3rGan', key, m)
    rng = np.random.default_rng(900)
    domain = (rng.standard_normal((14, 11, 13, 2)) * 2 + 0.5).astype(
        np.float32)
    topo = (0.6 + rng.standard_normal((14, 11, 1))).astype(np.float32)
    exo = {'topography': {'steps': [
        {'model': 0, 'combine_type': 'input', 'data': topo, 's_enhance': 1,
         't_enhance': 1}]}}
    ti = pd.date_range('2015-01-30 18:00', periods=13, freq='6h')
    lin = {}
    for f in FEATS:
        lin.update(R.seeded_linear_tables(rng, (14, 11), feature=f))
    args = dict(fwp_chunk_shape=(6, 5, 6), spatial_pad=2, temporal_pad=2,
                model=m, exo_data=exo)
    plain = _run(ArrayStrategy(domain, key, **args))
    ident = ArrayStrategy(
        domain, key, **args, bias_correct_method='monthly_local_linear_bc',
        bias_correct_kwargs={f: dict(bias_fp=_identity((14, 11), FEATS),
                                     temporal_avg=False) for f in FEATS},
        input_time_index=ti)
    got = _run(ident)
    assert _on_device(ident)
    for k in plain:
        np.testing.assert_array_equal(got[k], plain[k])
    # ... and a real correction equals the restatement's route bit for bit
    bck = {f: dict(bias_fp=lin, temporal_avg=False) for f in FEATS}
    st = ArrayStrategy(domain, key, **args,
                       bias_correct_method='monthly_local_linear_bc',
                       bias_correct_kwargs=bck, input_time_index=ti)
    got = _run(st)
    assert _on_device(st)
    want = _reference_route(ArrayStrategy(domain, key, **args), m,
                            'monthly_local_linear_bc', bck, ti)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k])
        assert np.abs(got[k] - plain[k]).max() > 1e-3
