"""CPU tests of ``sup3r_amd.bias_calc.SkillAssessment``: the class's plumbing
and the host half of the KS test, with ``tests/skill_ref.py``'s numpy
``Backend`` where the device's kernels would be called.  What ``s3_bc_skill``
computes is tested in ``test_skill_gpu.py``.

The numpy backend evaluates a pixel's annual statistics with the very calls of
the reference on the same 1-D float32 series, so those tables must be equal
bit for bit — the KS statistic and p-value included, which pass through the
integer counts and ``ks_from_counts`` on the way.  The monthly tables come
from ``bias_calc_ref.Backend.moments``, which reduces a 2-D array along an
axis: numpy adds in another order there than over a 1-D slice, hence the
tolerance that ``test_bias_calc_cpu.py`` uses for the same tables."""
import warnings

import numpy as np
import pandas as pd
import pytest
from scipy import stats

from tests import bias_calc_ref as R
from tests import skill_ref as S

KEYS_12 = ['pr_scalar', 'pr_adder', 'bias_pr_mean_monthly',
           'bias_pr_std_monthly', 'base_pr_obs_mean_monthly',
           'base_pr_obs_std_monthly']
KEYS_1 = ['pr_ks_stat', 'pr_ks_p', 'pr_bias', 'bias_pr_mean', 'bias_pr_std',
          'bias_pr_skew', 'bias_pr_kurtosis', 'bias_pr_zero_rate',
          'base_pr_obs_mean', 'base_pr_obs_std', 'base_pr_obs_skew',
          'base_pr_obs_kurtosis', 'base_pr_obs_zero_rate',
          'base_pr_obs_percentile_1', 'bias_pr_percentile_1',
          'base_pr_obs_percentile_5', 'bias_pr_percentile_5',
          'base_pr_obs_percentile_25', 'bias_pr_percentile_25',
          'base_pr_obs_percentile_50', 'bias_pr_percentile_50',
          'base_pr_obs_percentile_75', 'bias_pr_percentile_75',
          'base_pr_obs_percentile_95', 'bias_pr_percentile_95',
          'base_pr_obs_percentile_99', 'bias_pr_percentile_99']


def _kwargs(inp, **extra):
    kw = dict(inp)
    kw.pop('bias_fut_data')
    kw.pop('bias_fut_time_index')
    kw.update(extra)
    return kw


def _make(inp, **extra):
    import sup3r_amd
    return sup3r_amd.SkillAssessment(backend=S.Backend(),
                                     **_kwargs(inp, **extra))


@pytest.fixture(scope='module')
def inputs():
    return {layout: R.seeded_inputs(layout, years=('2020',))
            for layout in ('sites', 'raster')}


def test_init_out_has_the_reference_keys_shapes_and_dtypes(inputs):
    import sup3r_amd
    from sup3r_amd import bias_calc
    assert 'SkillAssessment' in bias_calc.__all__
    assert 'SkillAssessment' in sup3r_amd.__all__
    assert issubclass(sup3r_amd.SkillAssessment,
                      sup3r_amd.MonthlyLinearCorrection)
    assert sup3r_amd.SkillAssessment.PERCENTILES == (1, 5, 25, 50, 75, 95, 99)
    calc = _make(inputs['sites'])
    assert list(calc.out) == KEYS_12 + KEYS_1
    assert len(KEYS_12) == 6 and len(KEYS_1) == 13 + 14
    for k, v in calc.out.items():
        assert v.shape == (3, 4, 12 if k in KEYS_12 else 1), k
        assert v.dtype == np.float32 and np.isnan(v).all(), k
    assert list(S.init_out((3, 4), 'pr', 'pr_obs')) == KEYS_12 + KEYS_1


@pytest.mark.parametrize('mzr', [False, True])
@pytest.mark.parametrize('layout, decimals', [('sites', None), ('raster', 1)])
def test_run_is_the_per_pixel_reference_loop(inputs, layout, decimals, mzr,
                                             tmp_path):
    extra = dict(decimals=decimals, match_zero_rate=mzr)
    calc = _make(inputs[layout], **extra)
    fp = str(tmp_path / 'skill.npz')
    out = calc.run(fp_out=fp, max_workers=2)
    assert calc.bad_bias_gids == [3, 7, 11]            # no site in that column
    raw = S.run(_kwargs(inputs[layout], **extra), np.float32,
                fill_extend=False)
    for k in KEYS_1:
        assert np.isnan(raw[k][:, 3]).all() and \
            not np.isnan(raw[k][:, :3]).any(), k
    want = R.fill_and_smooth(raw)
    assert list(out) == list(want) == KEYS_12 + KEYS_1
    for k, v in out.items():
        assert v.dtype == np.float32 and v.shape == want[k].shape, k
        assert np.array_equal(np.isnan(v), np.isnan(want[k])), k
        if k in KEYS_1:
            assert np.array_equal(v, want[k]), k
        else:
            ok = ~np.isnan(v)
            assert np.allclose(v[ok], want[k][ok], rtol=2e-5, atol=1e-6), k
    # as in the reference, the monthly scalar and adder are never written
    assert np.isnan(out['pr_scalar']).all() and np.isnan(out['pr_adder']).all()
    assert not np.isnan(out['bias_pr_mean_monthly']).any()
    assert ((out['pr_ks_p'] >= 0) & (out['pr_ks_p'] <= 1)).all()
    # the file, re-read
    with np.load(fp) as f:
        assert sorted(f.files) == sorted(KEYS_12 + KEYS_1
                                         + ['latitude', 'longitude'])
        for k in KEYS_12 + KEYS_1:
            assert np.array_equal(f[k], out[k], equal_nan=True), k
        assert np.array_equal(f['latitude'],
                              inputs[layout]['bias_lat_lon'][..., 0])


def test_smoothing_keywords_reach_fill_and_smooth(inputs):
    calc = _make(inputs['sites'])
    out = calc.run(smooth_extend=1, smooth_interior=0.5)
    want = S.run(_kwargs(inputs['sites']), np.float32, smooth_extend=1,
                 smooth_interior=0.5)
    for k in KEYS_1:
        assert np.array_equal(out[k], want[k], equal_nan=True), k


# ------------------------------------------------------------- the p-value
@pytest.mark.parametrize('n1, n2', [(1, 1), (1, 7), (12, 12), (30, 45),
                                    (366, 731), (1000, 999)])
def test_exact_route_is_scipys(n1, n2):
    from sup3r_amd import bias_calc as B
    rng = np.random.default_rng(n1 + n2)
    for ties in (False, True):
        x = rng.normal(0, 1, n1)
        y = rng.normal(0.2, 1.3, n2)
        if ties:
            x, y = np.round(x), np.round(y)
        want = stats.ks_2samp(x, y)
        counts = np.array([S.ks_counts(x, y)])
        stat, pval = B.ks_from_counts(n1, n2, counts)
        assert S.ks_numerator(x, y) == round(want.statistic * n1 * n2)
        assert stat[0] == want.statistic and pval[0] == want.pvalue


def test_the_kernels_walk_over_base_run_ends_finds_the_extrema():
    """the formulation of ``s3_bc_skill`` (``skill_ref.ks_counts_walk``)
    against the brute force and scipy on 1000 random pairs of lengths 1 ..
    39, half of them integer-valued with heavy ties"""
    from sup3r_amd import bias_calc as B
    rng = np.random.default_rng(0)
    for it in range(1000):
        n1, n2 = (int(v) for v in rng.integers(1, 40, 2))
        if it % 2:
            x = rng.integers(-3, 4, n1).astype(np.float32)
            y = rng.integers(-3, 4, n2).astype(np.float32)
        else:
            x = rng.normal(0, 1, n1).astype(np.float32)
            y = rng.normal(0.3, 1, n2).astype(np.float32)
        c = S.ks_counts_walk(x, y)
        h = max(c[0] * n2 - c[1] * n1, c[3] * n1 - c[2] * n2, 0)
        assert h == S.ks_numerator(x, y), (it, c)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            want = stats.ks_2samp(x, y)
            stat, pval = B.ks_from_counts(n1, n2, np.array([c]))
        assert h == round(want.statistic * n1 * n2), it
        assert np.float32(stat[0]) == np.float32(want.statistic), it
        assert pval[0] == pytest.approx(want.pvalue, rel=1e-12, abs=0), it


def test_asymptotic_route_beyond_scipys_auto_limit():
    from sup3r_amd import bias_calc as B
    assert B.KS_MAX_AUTO_N == 10000
    rng = np.random.default_rng(5)
    n1, n2 = 10001, 400
    rows, want = [], []
    for shift in (0.0, 0.1):
        x = rng.normal(0, 1, n1)
        y = rng.normal(shift, 1, n2)
        rows.append(S.ks_counts(x, y))
        want.append(stats.ks_2samp(x, y))
    stat, pval = B.ks_from_counts(n1, n2, np.array(rows))
    for i, w in enumerate(want):
        assert stat[i] == w.statistic
        assert pval[i] == pytest.approx(w.pvalue, rel=1e-12)


def test_a_failed_exact_attempt_falls_back_with_scipys_warning(monkeypatch):
    from scipy.stats import _stats_py
    from sup3r_amd import bias_calc as B
    monkeypatch.setattr(_stats_py, '_attempt_exact_2kssamp',
                        lambda n1, n2, g, d, alt: (False, d, np.nan))
    rng = np.random.default_rng(6)
    x, y = rng.normal(0, 1, 50), rng.normal(0.5, 1, 70)
    with pytest.warns(RuntimeWarning, match='Exact calculation unsuccessful'):
        stat, pval = B.ks_from_counts(50, 70, np.array([S.ks_counts(x, y)]))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        want = stats.ks_2samp(x, y, method='asymp')
    assert stat[0] == pytest.approx(want.statistic, rel=1e-15)
    assert pval[0] == pytest.approx(want.pvalue, rel=1e-12)


def test_memoised_p_values_are_the_unmemoised_ones():
    from sup3r_amd import bias_calc as B
    rng = np.random.default_rng(7)
    n1, n2 = 40, 60
    rows = [S.ks_counts(np.round(rng.normal(0, 1, n1), 1),
                        np.round(rng.normal(0, 1, n2), 1)) for _ in range(60)]
    rows += rows[:5] + [(B._lib.BCC_SK_NO_KS,) * 4]
    memo = {}
    stat, pval = B.ks_from_counts(n1, n2, np.array(rows), memo)
    assert 1 < len(memo) < 60                         # numerators are shared
    assert np.isnan(stat[-1]) and np.isnan(pval[-1])
    for i, row in enumerate(rows[:-1]):
        s1, p1 = B.ks_from_counts(n1, n2, np.array([row]))
        assert stat[i] == s1[0] and pval[i] == p1[0], i


# ------------------------------------------------------------------ limits
def test_a_series_past_the_sort_limit_is_refused(inputs):
    inp = dict(inputs['sites'])
    n = 32769
    inp['bias_time_index'] = pd.date_range('1900-01-01', periods=n, freq='D')
    inp['bias_data'] = np.zeros((3, 4, n), np.float32)
    calc = _make(inp)
    with pytest.raises(ValueError, match='BCC_MAX_SORT'):
        calc.run()
    # the base series: hourly data without a daily reduction
    inp = dict(inputs['sites'])
    ti = pd.date_range('2000-01-01', periods=n, freq='h')
    inp['base_data'] = (np.zeros((n, 40), np.float32), ti)
    calc = _make(inp)
    with pytest.raises(ValueError, match='BCC_MAX_SORT'):
        calc.run(daily_reduction=None)
