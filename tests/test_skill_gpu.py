"""GPU tests (``-m gpu``) of ``s3_bc_skill`` through
``sup3r_amd.bias_calc.DeviceBackend.skill`` and of ``SkillAssessment`` on the
device, against ``tests/skill_ref.py`` (the reference's own numpy / scipy
calls).

Tolerances (none is taken from the code under test):
  * exact — the KS counts.  The device's integer numerator ``h`` equals the
    brute-force integer of ``skill_ref.ks_numerator`` and ``round(statistic D
    T)`` of ``scipy.stats.ks_2samp``; ``ks_stat`` as float32 equals scipy's;
    ``ks_p`` agrees to ``rtol = 1e-12`` (the same routine on the same
    arguments).  The KS numerator is discrete and the reference subtracts
    numpy's pairwise float32 mean, which may differ from the device's (an fp64
    sum rounded once) by an ulp: on continuous data the device's means are
    forced into the reference; on a dyadic grid (multiples of 2^-6, ``|x| <
    64``, ``n <= 4096``: every float32 partial sum is exact) nothing is
    forced, after the test has asserted that numpy's float32 mean is the
    float64 mean rounded;
  * percentiles: within one float32 ulp of the larger of the two neighbouring
    order statistics of ``np.percentile`` (the rule of ``_quantile_rows`` in
    ``test_bias_calc_gpu.py``, restated in ``_percentile_row``);
  * ``mean``, ``std``, ``skew``, ``kurtosis``, ``zero_rate``, ``bias``: the
    rule of DESIGN.md §8b — ``R32`` the reference on the float32 series,
    ``R64`` the same calls on float64 copies, the device within ``max(2 max|R32
    - R64|, ulp32(R64))`` of ``R64`` and in the class (NaN / inf) of ``R32``.
Each case prints its figures (``profiles/skill/NOTES.md`` records them)."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
from scipy import stats

from tests import bias_calc_ref as R
from tests import skill_ref as S

pytestmark = pytest.mark.gpu

PAIRS = [(1, 1), (1, 3), (2, 63), (3, 2), (63, 64), (64, 65), (65, 255),
         (255, 256), (256, 257), (257, 1023), (1023, 1025), (1025, 8192),
         (8192, 8193), (8193, 1), (64, 64), (32768, 32768)]
DYADIC = [p for p in PAIRS if max(p) <= 4096]
STATS = S.STAT_NAMES


@functools.lru_cache(None)
def _be():
    from sup3r_amd.bias_calc import DeviceBackend
    return DeviceBackend()


def _skill(base, bias, demean):
    be = _be()
    return be.skill(be.upload(base), be.upload(bias), demean)


def _n_pix(d, t):
    return 2 if max(d, t) > 8193 else 3


def _series(kind, d, t, n_pix=None):
    rng = np.random.default_rng([d, t, len(kind)])
    n_pix = n_pix or _n_pix(d, t)
    if kind == 'continuous':
        base = rng.gamma(0.7, 2.0, (n_pix, d))
        bias = rng.gamma(0.8, 1.7, (n_pix, t)) + 0.1
    elif kind == 'dyadic':
        base = np.round(rng.normal(0, 12, (n_pix, d)) * 64).clip(
            -4095, 4095) / 64
        bias = np.round(rng.normal(1, 10, (n_pix, t)) * 64).clip(
            -4095, 4095) / 64
    else:                                                 # 'integer'
        base = rng.integers(-3, 4, (n_pix, d))
        bias = rng.integers(-2, 5, (n_pix, t))
    return base.astype(np.float32), bias.astype(np.float32)


@functools.lru_cache(None)
def _case(kind, d, t, demean=True):
    """inputs and the device's answer, computed once per case and shared"""
    base, bias = _series(kind, d, t)
    res = _skill(base, bias, demean)
    for a in (base, bias, *res.values()):
        a.setflags(write=False)
    return base, bias, res


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(
        np.float32)).astype(np.float64)


def _numerator(row, d, t):
    c1p, c2p, c1m, c2m = (int(v) for v in row)
    assert 0 <= c1p <= d and 0 <= c1m <= d and 0 <= c2p <= t and 0 <= c2m <= t
    return max(c1p * t - c2p * d, c2m * d - c1m * t, 0)


def _check_ks(name, res, p, x1, x2, want):
    """pixel ``p``: the device's counts against the brute force on the
    compared values ``x1``, ``x2`` and against scipy's result ``want``"""
    from sup3r_amd import bias_calc as B
    d, t = len(x1), len(x2)
    h = _numerator(res['ks'][p], d, t)
    assert h == S.ks_numerator(x1, x2), name
    assert h == round(float(want.statistic) * d * t), name
    stat, pval = B.ks_from_counts(d, t, res['ks'][p:p + 1])
    assert np.float32(stat[0]) == np.float32(want.statistic), name
    assert pval[0] == pytest.approx(want.pvalue, rel=1e-12, abs=0), name
    return h


def _means(res, p):
    return res['stats'][p, 0, S.SK_MEAN], res['stats'][p, 1, S.SK_MEAN]


def _demeaned_ks(name, res, p, base, bias):
    """the reference's KS test with the device's two means forced"""
    m0, m1 = _means(res, p)
    with R.quiet():
        out = S.run_skill_eval(bias.copy(), base.copy(), 'f', 'd',
                               forced_means=(m0, m1))
    want = types.SimpleNamespace(statistic=out['f_ks_stat'],
                                 pvalue=out['f_ks_p'])
    return _check_ks(name, res, p, base - m0, bias - m1, want)


def _percentile_row(name, dev, series):
    """``dev`` (7,) against np.percentile of the float32 ``series`` (n,)"""
    want = np.percentile(series, S.PERCENTILES).astype(np.float32)
    if np.isnan(series).any():
        assert np.isnan(dev).all() and np.isnan(want).all(), name
        return 0.0
    s = np.sort(series)
    pos = (len(s) - 1) * (np.array(S.PERCENTILES) / 100)
    lo = np.floor(pos).astype(int)
    hi = np.minimum(lo + 1, len(s) - 1)
    bound = np.spacing(np.maximum(np.abs(s[lo]), np.abs(s[hi])))
    err = np.abs(dev.astype(np.float64) - want.astype(np.float64))
    assert (err <= bound).all(), (name, float((err - bound).max()))
    return float((err / np.maximum(bound, 1e-45)).max())


def _reference_stats(series, dtype):
    """the five statistics of one series with the reference's calls"""
    x = series.astype(dtype)
    with R.quiet():
        return [np.nanmean(x), np.nanstd(x), stats.skew(x), stats.kurtosis(x),
                np.nanmean(x == 0)]


def _rule(name, dev, r32, r64):
    """the tolerance rule of DESIGN.md §8b; prints the figures and returns
    the worst error / bound"""
    dev = np.asarray(dev, np.float64)
    r32 = np.asarray(r32, np.float64)
    r64 = np.asarray(r64, np.float64)
    assert np.array_equal(np.isnan(dev), np.isnan(r32)), name
    inf = np.isinf(r32)
    assert np.array_equal(dev[inf], r32[inf]), name
    ok = np.isfinite(r32) & np.isfinite(r64)
    if not ok.any():
        print(f'[skill tolerance] {name}: nothing finite')
        return 0.0
    ref_err = float(np.abs(r32 - r64)[ok].max())
    bound = np.maximum(2 * ref_err, _ulp(r64))
    err = np.abs(dev - r64)
    ratio = float((err / bound)[ok].max())
    print(f'[skill tolerance] {name}: max|R32-R64| = {ref_err:.3e}, device '
          f'max err = {float(err[ok].max()):.3e}, worst err / bound = '
          f'{ratio:.3f}, device == R32 bitwise: '
          f'{bool(np.array_equal(dev[ok], r32[ok]))}')
    assert ratio <= 1, (name, ratio, ref_err)
    return ratio


def _check_moments(name, res, base, bias):
    """all pixels of a case through the rule, statistic by statistic"""
    rows = {dt: np.array([[_reference_stats(x[p], dt) for x in (base, bias)]
                          for p in range(len(base))], np.float64)
            for dt in (np.float32, np.float64)}
    for j, stat in enumerate(STATS):
        _rule(f'{name} {stat}', res['stats'][:, :, j],
              rows[np.float32][:, :, j], rows[np.float64][:, :, j])
    dev = res['stats'][:, 1, S.SK_BIAS]
    assert np.array_equal(dev, res['stats'][:, 0, S.SK_BIAS], equal_nan=True)
    r32 = (rows[np.float32][:, 1, 0].astype(np.float32)
           - rows[np.float32][:, 0, 0].astype(np.float32))
    _rule(f'{name} bias', dev, r32,
          rows[np.float64][:, 1, 0] - rows[np.float64][:, 0, 0])
    assert np.array_equal(res['status'][:, 0], np.isnan(base).sum(axis=1))
    assert np.array_equal(res['status'][:, 2], np.isnan(bias).sum(axis=1))
    assert np.array_equal(res['status'][:, 1],
                          (~np.isfinite(base)).sum(axis=1))
    assert np.array_equal(res['status'][:, 3],
                          (~np.isfinite(bias)).sum(axis=1))


def _check_all(name, res, base, bias, demean):
    """every output of a launch against the reference"""
    for p in range(len(base)):
        for s, x in enumerate((base, bias)):
            _percentile_row(f'{name} p={p} s={s}',
                            res['stats'][p, s, S.SK_PCT0:S.SK_BIAS], x[p])
        if np.isnan(base[p]).any() or np.isnan(bias[p]).any():
            assert (res['ks'][p] == S.SK_NO_KS).all(), name
            with R.quiet():
                assert np.isnan(stats.ks_2samp(base[p], bias[p]).statistic)
        elif demean:
            _demeaned_ks(f'{name} p={p}', res, p, base[p], bias[p])
        else:
            _check_ks(f'{name} p={p}', res, p, base[p], bias[p],
                      stats.ks_2samp(base[p], bias[p]))
    _check_moments(name, res, base, bias)


# ------------------------------------------------------------ the KS counts
@pytest.mark.parametrize('d, t', PAIRS)
def test_ks_counts_on_continuous_data_with_the_means_forced(d, t):
    base, bias, res = _case('continuous', d, t)
    hs = [_demeaned_ks(f'D={d} T={t} p={p}', res, p, base[p], bias[p])
          for p in range(len(base))]
    print(f'[skill ks] continuous D={d} T={t}: h = {hs} of {d * t}')


@pytest.mark.parametrize('d, t', DYADIC)
def test_ks_counts_on_a_dyadic_grid_without_forcing(d, t):
    from sup3r_amd import bias_calc as B
    base, bias, res = _case('dyadic', d, t)
    for p in range(len(base)):
        for s, x in enumerate((base[p], bias[p])):
            m32 = np.nanmean(x)
            assert m32.dtype == np.float32
            assert m32 == np.float32(np.mean(x.astype(np.float64)))
            assert res['stats'][p, s, S.SK_MEAN] == m32
        want = S.run_skill_eval(bias[p].copy(), base[p].copy(), 'f', 'd')
        d32 = base[p] - np.nanmean(base[p]), bias[p] - np.nanmean(bias[p])
        h = _numerator(res['ks'][p], d, t)
        assert h == S.ks_numerator(*d32)
        assert h == round(float(want['f_ks_stat']) * d * t)
        stat, pval = B.ks_from_counts(d, t, res['ks'][p:p + 1])
        assert np.float32(stat[0]) == np.float32(want['f_ks_stat'])
        assert pval[0] == pytest.approx(want['f_ks_p'], rel=1e-12, abs=0)


@pytest.mark.parametrize('demean', [True, False])
@pytest.mark.parametrize('d, t', [(3, 2), (65, 255), (256, 257), (1025, 8192),
                                  (8193, 1), (64, 64)])
def test_ks_counts_on_integer_data_with_heavy_ties(d, t, demean):
    """seven distinct values per series: ties within each series and, without
    the demeaning, across them"""
    base, bias, res = _case('integer', d, t, demean)
    for p in range(len(base)):
        if demean:
            _demeaned_ks(f'integer D={d} T={t}', res, p, base[p], bias[p])
        else:
            _check_ks(f'integer raw D={d} T={t}', res, p, base[p], bias[p],
                      stats.ks_2samp(base[p], bias[p]))


# -------------------------------------------- percentiles and the moments
@pytest.mark.parametrize('d, t', PAIRS)
def test_percentiles_at_every_length(d, t):
    base, bias, res = _case('continuous', d, t)
    worst = max(_percentile_row(f'D={d} T={t} p={p} s={s}',
                                res['stats'][p, s, S.SK_PCT0:S.SK_BIAS], x[p])
                for p in range(len(base)) for s, x in enumerate((base, bias)))
    print(f'[skill tolerance] percentiles D={d} T={t}: worst err / bound = '
          f'{worst:.3f}')


@pytest.mark.parametrize('d, t', PAIRS)
def test_moments_at_every_length(d, t):
    base, bias, res = _case('continuous', d, t)
    _check_moments(f'D={d} T={t}', res, base, bias)


def test_moments_over_many_pixels():
    """70 pixels: the reference's own float32 error is sampled well"""
    base, bias = _series('continuous', 1023, 257, n_pix=70)
    _check_moments('P=70', _skill(base, bias, True), base, bias)


# -------------------------------------------------------------- edge cases
def _edge(case):
    rng = np.random.default_rng(11)
    base = rng.gamma(0.7, 2.0, (2, 65)).astype(np.float32)
    bias = rng.gamma(0.8, 1.7, (2, 257)).astype(np.float32)
    if case == 'bias_below':
        bias = -bias - 1
    elif case == 'bias_above':
        bias = bias + base.max() + 1
    elif case == 'identical':
        bias = base.copy()
    elif case == 'constant':
        base[0] = np.float32(0.1)
        bias[1] = np.float32(-7.3)
    elif case == 'nan_in_base':
        base[1, 17] = np.nan
    elif case == 'nan_in_bias':
        bias[0, 256] = np.nan
    elif case == 'signed_zeros':
        base[:, ::2] = 0.0
        base[:, 1::4] = -0.0
        bias[:, ::3] = -0.0
        bias[:, 1::3] = 0.0
    return base, bias


@pytest.mark.parametrize('demean', [True, False])
@pytest.mark.parametrize('case', ['bias_below', 'bias_above', 'identical',
                                  'constant', 'nan_in_base', 'nan_in_bias',
                                  'signed_zeros'])
def test_edge_cases(case, demean):
    from sup3r_amd import bias_calc as B
    base, bias = _edge(case)
    res = _skill(base, bias, demean)
    _check_all(f'{case} demean={demean}', res, base, bias, demean)
    d, t = base.shape[1], bias.shape[1]
    st = res['stats']
    if case in ('bias_below', 'bias_above') and not demean:
        assert [_numerator(r, d, t) for r in res['ks']] == [d * t] * 2
    if case == 'identical':
        assert [_numerator(r, d, t) for r in res['ks']] == [0, 0]
        stat, pval = B.ks_from_counts(d, t, res['ks'])
        assert (stat == 0).all() and (pval == 1).all()
    if case == 'constant':
        for p, s in ((0, 0), (1, 1)):
            assert np.isnan(st[p, s, [S.SK_SKEW, S.SK_KURTOSIS]]).all()
            assert len(set(st[p, s, S.SK_PCT0:S.SK_BIAS])) == 1 and st[p, s, 1] == 0
        assert not np.isnan(st[1, 0]).any() and not np.isnan(st[0, 1]).any()
    if case in ('nan_in_base', 'nan_in_bias'):
        p, s = (1, 0) if case == 'nan_in_base' else (0, 1)
        assert np.isnan(st[p, s, S.SK_SKEW:S.SK_ZERO_RATE]).all()
        assert np.isnan(st[p, s, S.SK_PCT0:S.SK_BIAS]).all()
        assert not np.isnan(st[p, s, [S.SK_MEAN, S.SK_STD,
                                      S.SK_ZERO_RATE]]).any()
        assert not np.isnan(st[p, 1 - s]).any()
        assert not np.isnan(st[1 - p]).any()
        assert (res['ks'][p] == S.SK_NO_KS).all()
        assert (res['ks'][1 - p] != S.SK_NO_KS).any()
    if case == 'signed_zeros':
        assert st[0, 0, S.SK_ZERO_RATE] == np.float32(
            np.mean(base[0] == 0)) > 0.7


def test_match_zero_rate_then_skill():
    """``match_zero_rate=True``: no demeaning, the bias series as
    ``s3_bc_match_zero_rate`` left it"""
    from sup3r_amd import bias_calc as B
    rng = np.random.default_rng(12)
    base = rng.gamma(0.5, 2.0, (3, 255)).astype(np.float32)
    base[:, ::3] = 0
    bias = np.round(rng.gamma(0.5, 2.0, (3, 1025)), 2).astype(np.float32)
    be = _be()
    d_base, d_bias = be.upload(base), be.upload(bias)
    d_bias, _, bad = be.match_zero_rate(d_base, d_bias)
    assert bad == 0
    res = be.skill(d_base, d_bias, False)
    matched = be.to_host(d_bias)
    for p in range(3):
        want = S.run_skill_eval(bias[p].copy(), base[p].copy(), 'f', 'd',
                                match_zero_rate=True)
        ref_bias, _ = R.match_zero_rate(bias[p].copy(), base[p])
        assert np.array_equal(matched[p], ref_bias)
        _check_ks(f'mzr p={p}', res, p, base[p], ref_bias,
                  stats.ks_2samp(base[p], ref_bias))
        stat, pval = B.ks_from_counts(255, 1025, res['ks'][p:p + 1])
        assert np.float32(stat[0]) == np.float32(want['f_ks_stat'])
        assert pval[0] == pytest.approx(want['f_ks_p'], rel=1e-12, abs=0)
        assert res['stats'][p, 1, S.SK_ZERO_RATE] == np.float32(
            want['bias_f_zero_rate'])
    _check_all('mzr', res, base, matched, False)


# ------------------------------------------------------------- determinism
def test_two_launches_and_two_grid_sizes_give_the_same_bits():
    base, bias = _series('continuous', 1023, 8193, n_pix=70)
    a = _skill(base, bias, True)
    b = _skill(base, bias, True)
    one = _skill(base[:1], bias[:1], True)
    for k in ('stats', 'ks', 'status'):
        assert a[k].tobytes() == b[k].tobytes(), k
        assert a[k][0].tobytes() == one[k][0].tobytes(), k


# ------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_with_a_message():
    import torch
    from sup3r_amd import _lib
    be = _be()
    L, ctx = _lib.lib(), be.dev.ctx
    dev = be.dev.torch_device
    x = torch.zeros(64, device=dev)
    work = torch.zeros(64, dtype=torch.int32, device=dev)
    stat = torch.full((2 * _lib.BCC_SK_STATS,), 7.0, device=dev)
    ks = torch.full((4,), 7, dtype=torch.int32, device=dev)
    status = torch.full((4,), 7, dtype=torch.int32, device=dev)
    ptr = [C.c_void_p(t.data_ptr()) for t in (x, x, work, stat, ks, status)]

    def call(d, t, p, null=None):
        a = list(ptr)
        if null is not None:
            a[null] = None
        return L.s3_bc_skill(ctx, a[0], d, a[1], t, p, 1, *a[2:])

    for null in range(6):
        assert call(8, 8, 1, null) == -1
        assert 'are needed' in _lib.last_error(ctx)
    for d, t, p in ((0, 8, 1), (8, 0, 1), (8, 8, 0)):
        assert call(d, t, p) == -1 and 'empty extent' in _lib.last_error(ctx)
    for d, t in ((8, 32769), (32769, 8)):
        assert call(d, t, 1) == -1
        assert 'S3_BCC_MAX_SORT' in _lib.last_error(ctx)
    # extents only: nothing is launched, no pointer is followed
    for d, t in ((32768, 1), (1, 32768)):
        assert call(d, t, 65536) == -1 and '2^31' in _lib.last_error(ctx)
    with pytest.raises(ValueError, match='S3_BCC_MAX_SORT'):
        be.skill(be.upload(np.zeros((1, 4), np.float32)),
                 be.upload(np.zeros((1, 32769), np.float32)), True)
    be.dev.sync()
    for t in (stat, ks, status):
        assert (t.cpu().numpy() == 7).all()


# -------------------------------------------------------------- end to end
class _DeviceBase(S.Backend):
    """the numpy backend on the device's base series: the KS numerator and
    the percentiles are then functions of the same float32 values"""

    def __init__(self, base, means):
        self.base, self.means = base, means

    def base_series(self, *args, **kwargs):
        return self.base.copy()

    def skill(self, base_series, bias_series, demean):
        res = super().skill(base_series, bias_series, demean)
        if demean:
            for p, (m0, m1) in enumerate(self.means):
                if not (np.isnan(m0) or np.isnan(m1)):
                    res['ks'][p] = S.ks_counts(base_series[p] - m0,
                                               bias_series[p] - m1)
        return res


@pytest.mark.parametrize('layout, mzr', [('sites', False), ('raster', True)])
def test_skill_assessment_end_to_end(layout, mzr):
    import sup3r_amd
    inp = R.seeded_inputs(layout, years=('2020', '2021'))
    inp.pop('bias_fut_data')
    inp.pop('bias_fut_time_index')
    inp['match_zero_rate'] = mzr
    calc = sup3r_amd.SkillAssessment(**inp)
    out = calc.run(fill_extend=False)
    be = calc.backend
    base = be.to_host(calc._base_series('avg')[0])
    flat = {k: v.reshape(12, -1) for k, v in out.items()}
    means = np.stack([flat['base_pr_obs_mean'][:, 0],
                      flat['bias_pr_mean'][:, 0]], axis=1)
    ref = sup3r_amd.SkillAssessment(backend=_DeviceBase(base, means), **inp)
    want = {k: v.reshape(12, -1)
            for k, v in ref.run(fill_extend=False).items()}
    assert list(out) == list(want) and calc.bad_bias_gids == [3, 7, 11]
    good = np.array([g not in (3, 7, 11) for g in range(12)])
    for k in out:
        assert np.array_equal(np.isnan(flat[k]), np.isnan(want[k])), k
        assert np.isnan(flat[k][~good]).all(), k
    assert np.array_equal(flat['pr_ks_stat'][good], want['pr_ks_stat'][good])
    assert np.array_equal(flat['pr_ks_p'][good], want['pr_ks_p'][good])
    # the series as the statistics saw them
    bias = np.asarray(inp['bias_data'], np.float32).reshape(12, -1).copy()
    if mzr:
        for p in np.where(good)[0]:
            bias[p], _ = R.match_zero_rate(bias[p], base[p])
    for p in np.where(good)[0]:
        for name, x in (('base_pr_obs', base), ('bias_pr', bias)):
            dev = np.array([flat[f'{name}_percentile_{q}'][p, 0]
                            for q in S.PERCENTILES])
            _percentile_row(f'{name} p={p}', dev, x[p])
    r64 = {name: np.array([_reference_stats(x[p], np.float64)
                           for p in np.where(good)[0]])
           for name, x in (('base_pr_obs', base), ('bias_pr', bias))}
    for name in r64:
        for j, stat in enumerate(STATS):
            k = f'{name}_{stat}'
            _rule(f'{layout} {k}', flat[k][good, 0], want[k][good, 0],
                  r64[name][:, j])
    _rule(f'{layout} pr_bias', flat['pr_bias'][good, 0],
          want['pr_bias'][good, 0],
          r64['bias_pr'][:, 0] - r64['base_pr_obs'][:, 0])
    # the monthly tables, from the same series
    month = {'base_pr_obs': calc._base_series('avg')[1].month,
             'bias_pr': calc.bias_ti.month}
    for name, x in (('base_pr_obs', base), ('bias_pr', bias)):
        x64 = x[good].astype(np.float64)
        for stat, fn in (('mean', np.nanmean), ('std', np.nanstd)):
            k = f'{name}_{stat}_monthly'
            m64 = np.stack([fn(x64[:, month[name] == m], axis=1)
                            for m in range(1, 13)], axis=1)
            _rule(f'{layout} {k}', flat[k][good], want[k][good], m64)
    assert np.isnan(flat['pr_scalar']).all()
