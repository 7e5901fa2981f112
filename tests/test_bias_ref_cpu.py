"""Properties of the numpy restatement ``tests/bias_ref.py`` (what the GPU
tests compare ``s3_bias_correct`` against): the assertions the reference makes
of its own QDM correction, ``interp`` against ``numpy.interp``, and the linear
family against closed forms.  These tests exercise the restatement only, not
``sup3r_amd``."""
import numpy as np
import pandas as pd
import pytest

from tests import bias_ref as R


def _ti(start, periods, freq='6h'):
    return pd.date_range(start, periods=periods, freq=freq)


# ------------------------------------------ properties of the restatement
# (the reference's own assertions, tests/bias/test_qdm_bias_correction.py:
# 266-452, on seeded tables)
@pytest.fixture(scope='module')
def qdm_case():
    rng = np.random.default_rng(11)
    fp = R.seeded_qdm_tables(rng, (6, 5), n_windows=4, n_q=51)
    fp = {k: (np.asarray(v, np.float64) if k.endswith('_params') else v)
          for k, v in fp.items()}
    ti = _ti('2015-03-20', 40, '1D')          # spans two of the four windows
    lo = fp['bias_fut_rsds_params'][..., 0].min()
    hi = fp['bias_fut_rsds_params'][..., -1].max()
    data = rng.uniform(lo, hi, (6, 5, len(ti)))
    return fp, ti, data


def _qdm(fp, ti, data, **kw):
    return R.local_qdm_bc(data, 'ghi', 'rsds', fp, ti, dtype=np.float64, **kw)


def test_interp_equals_numpy_interp_in_float64():
    rng = np.random.default_rng(0)
    xp = np.sort(rng.uniform(0, 10, (7, 21)), axis=1)
    xp[:, 5:9] = xp[:, 5:6]                      # repeated knots
    fp = np.sort(rng.uniform(-3, 3, (7, 21)), axis=1)
    x = rng.uniform(-1, 11, (7, 50))
    x[:, 0], x[:, 1], x[:, 2] = xp[:, 5], xp[:, 0], xp[:, -1]
    got = R.interp(x, xp, fp)
    for s in range(7):
        np.testing.assert_array_equal(got[s], np.interp(x[s], xp[s], fp[s]))


def test_qdm_no_trend_equals_full_correction_with_bias_fut_as_bias(qdm_case):
    fp, ti, data = qdm_case
    fp2 = dict(fp, bias_fut_rsds_params=fp['bias_rsds_params'])
    for relative in (True, False):
        assert np.allclose(_qdm(fp, ti, data, no_trend=True,
                                relative=relative),
                           _qdm(fp2, ti, data, relative=relative))


@pytest.mark.parametrize('relative', [True, False])
def test_qdm_identical_distributions_leave_the_data_unchanged(qdm_case,
                                                              relative):
    fp, ti, data = qdm_case
    same = fp['bias_fut_rsds_params']
    fp2 = dict(fp, base_ghi_params=same, bias_rsds_params=same)
    assert np.allclose(_qdm(fp2, ti, data, relative=relative), data)


def test_qdm_shifted_distributions(qdm_case):
    fp, ti, data = qdm_case
    fut = fp['bias_fut_rsds_params']
    # base = fut - 10, bias = fut: shifts by -10
    fp2 = dict(fp, base_ghi_params=fut - 10, bias_rsds_params=fut)
    assert np.allclose(_qdm(fp2, ti, data, relative=False), data - 10)
    # base = fut, bias = fut - 10: shifts by +10
    fp3 = dict(fp, base_ghi_params=fut, bias_rsds_params=fut - 10)
    assert np.allclose(_qdm(fp3, ti, data, relative=False), data + 10)
    # both - 10: unchanged
    fp4 = dict(fp, base_ghi_params=fut - 10, bias_rsds_params=fut - 10)
    assert np.allclose(_qdm(fp4, ti, data, relative=False), data)


def test_presrat_zero_rate_and_k_factor():
    rng = np.random.default_rng(3)
    fp = R.seeded_qdm_tables(rng, (4, 3), n_windows=3, n_q=21, presrat=True)
    ti = _ti('2016-01-01', 12, '1D')
    data = rng.uniform(1, 40, (4, 3, 12)).astype(np.float64)
    q = R.local_qdm_bc(data, 'ghi', 'rsds', fp, ti, dtype=np.float64,
                       delta_denom_min=fp['zero_rate_threshold'])
    p = R.local_presrat_bc(data, 'ghi', 'rsds', fp, ti, dtype=np.float64)
    tau = fp['rsds_tau_fut'].astype(np.float64)
    k = fp['rsds_k_factor'].astype(np.float64)[:, :, :1]   # window 0 only
    np.testing.assert_allclose(p, np.where(q < tau, 0, q * k))
    assert (p == 0).any() and (p > 0).any()
    np.testing.assert_array_equal(
        R.local_presrat_bc(data, 'ghi', 'rsds', fp, ti, dtype=np.float64,
                           no_trend=True),
        R.local_qdm_bc(data, 'ghi', 'rsds', fp, ti, dtype=np.float64,
                       no_trend=True,
                       delta_denom_min=fp['zero_rate_threshold']))


def test_relative_qdm_with_a_zero_denominator_raises():
    rng = np.random.default_rng(4)
    fp = R.seeded_qdm_tables(rng, (3, 3), n_windows=2, n_q=11)
    fp['bias_rsds_params'] = np.zeros_like(fp['bias_rsds_params'])
    ti = _ti('2016-01-01', 5, '1D')
    data = rng.uniform(5, 20, (3, 3, 5))
    with pytest.raises(RuntimeError, match='NaN / inf'):
        R.local_qdm_bc(data, 'ghi', 'rsds', fp, ti, dtype=np.float64)
    out = R.local_qdm_bc(data, 'ghi', 'rsds', fp, ti, dtype=np.float64,
                         delta_denom_zero=2.0)
    assert np.isfinite(out).all()


# ------------------------------------------ linear restatement, closed forms
def test_monthly_temporal_avg_over_two_months():
    rng = np.random.default_rng(5)
    fp = {k: v.astype(np.float64) for k, v in
          R.seeded_linear_tables(rng, (5, 4)).items()}
    ti = _ti('2015-01-29', 20)                  # 12 steps in Jan, 8 in Feb
    assert list(np.bincount(ti.month)[1:3]) == [12, 8]
    data = rng.standard_normal((5, 4, 20))
    s, a = fp['u_10m_scalar'], fp['u_10m_adder']
    want = data * ((12 * s[..., 0] + 8 * s[..., 1]) / 20)[..., None] + \
        ((12 * a[..., 0] + 8 * a[..., 1]) / 20)[..., None]
    got = R.monthly_local_linear_bc(data, 'u_10m', fp, ti, temporal_avg=True,
                                    dtype=np.float64)
    np.testing.assert_allclose(got, want, rtol=1e-13)
    per_step = R.monthly_local_linear_bc(data, 'u_10m', fp, ti,
                                         temporal_avg=False, dtype=np.float64)
    m = ti.month.values - 1
    np.testing.assert_array_equal(per_step, data * s[..., m] + a[..., m])
    with pytest.warns(UserWarning, match='>2 months'):
        R.monthly_local_linear_bc(
            rng.standard_normal((5, 4, 300)), 'u_10m', fp,
            _ti('2015-01-29', 300), dtype=np.float64)


def test_linear_ranges_and_3d_factors_through_local_linear_bc():
    rng = np.random.default_rng(6)
    fp = {k: v.astype(np.float64) for k, v in
          R.seeded_linear_tables(rng, (5, 4)).items()}
    ti = _ti('2015-06-01', 8)
    data = rng.standard_normal((5, 4, 8)) * 3
    s = np.clip(fp['u_10m_scalar'][..., 5], 0.9, 1.1)[..., None]
    a = np.clip(fp['u_10m_adder'][..., 5], -0.5, 0.5)[..., None]
    got = R.monthly_local_linear_bc(
        data, 'u_10m', fp, ti, temporal_avg=False, scalar_range=(0.9, 1.1),
        adder_range=(0.5, -0.5), out_range=(-2, 2), dtype=np.float64)
    np.testing.assert_array_equal(got, np.clip(data * s + a, -2, 2))
    assert (got == 2).any() and (got == -2).any()
    # 3-D factors through local_linear_bc: the mean over the 12 months
    got = R.local_linear_bc(data[1:4, 0:3], 'u_10m', fp, dtype=np.float64,
                            lr_padded_slice=(slice(1, 4), slice(0, 3)))
    want = data[1:4, 0:3] * fp['u_10m_scalar'].mean(-1)[1:4, 0:3, None] + \
        fp['u_10m_adder'].mean(-1)[1:4, 0:3, None]
    np.testing.assert_allclose(got, want, rtol=1e-14)
    np.testing.assert_array_equal(
        R.global_linear_bc(data, 1.5, -0.25, out_range=(0, 1),
                           dtype=np.float64),
        np.clip(data * 1.5 - 0.25, 0, 1))
