"""GPU tests (``-m gpu``) of the bias calculators: the five ``s3_bc_*``
kernels one by one through ``sup3r_amd.bias_calc.DeviceBackend`` (thin ctypes
wrappers), the six classes against the per-pixel loop of
``tests/bias_calc_ref.py``, and the computed tables fed to the corrections of
``sup3r_amd.bias``.

Tolerances (none is taken from the code under test):
  * exact — selections and integer counts: ``max`` / ``min`` / no reduction
    of a one-site pixel, the order statistics ``q = 0``, ``q = 1`` and ``tau``,
    ``obs_zero_rate``, ``z_fg``, which values ``match_zero_rate`` zeroes;
  * quantile rows on a given float32 series: within one float32 ulp of the
    larger of the two neighbouring order statistics of ``np.quantile(series,
    q).astype(float32)`` (numpy takes ``b - a`` in the array's dtype and
    switches formula at ``t >= 0.5``; a plain fp64 ``a + (b - a) frac`` rounded
    once differs from it by at most that);
  * sums and means (site mean, ``avg`` / ``sum``, moments, ``k_factor``, the
    clearsky ratio) and PresRat's corrected series: the rule of DESIGN.md §8b —
    the reference in float64 (``R64``) and in float32 (``R32``) on the test's
    own inputs, the device within ``2 * max|R32 - R64|`` of ``R64``, never held
    to less than one float32 ulp of the result;
  * class-level quantile tables and ``tau_fut``: order statistics are
    1-Lipschitz in the sup norm, so the measured ``max|series_dev -
    series_R64|`` of the stage before plus the one ulp above;
  * ``scalar`` / ``adder`` are float32 expressions of the four moments on the
    host, so their bound is the moments' bounds carried through ``s_o / s_b``
    and ``m_o - m_b scalar`` to first order, plus one float32 ulp for each of
    the expression's own roundings (written out in ``_linear_bounds``).
Where ``R32`` is NaN or inf the device must give the same class of value.
Each case prints its figures (``profiles/bias_calc/NOTES.md`` records them)."""
import ctypes as C
import functools

import numpy as np
import pandas as pd
import pytest

from tests import bias_calc_ref as R

pytestmark = pytest.mark.gpu

SORT_LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 32768]
QDM_KW = dict(n_quantiles=21, n_time_steps=8, window_size=100)
KINDS = R.LINEAR + ('QuantileDeltaMappingCorrection', 'PresRat')
THRESHOLD = 0.05


@functools.lru_cache(None)
def _be():
    from sup3r_amd.bias_calc import DeviceBackend
    return DeviceBackend()


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(
        np.float32)).astype(np.float64)


def _same_class(dev, r32):
    """NaN where R32 is NaN, the same infinity where it is infinite"""
    dev, r32 = np.asarray(dev), np.asarray(r32)
    assert np.array_equal(np.isnan(dev), np.isnan(r32))
    inf = np.isinf(r32)
    assert np.array_equal(dev[inf], r32[inf].astype(dev.dtype))
    return np.isfinite(r32)


def _rule(name, dev, r32, r64, extra=0.0):
    """the tolerance rule of DESIGN.md §8b (+ ``extra``, an error measured at
    the stage before); prints the figures"""
    dev = np.asarray(dev, np.float64)
    r32 = np.asarray(r32, np.float64)
    r64 = np.asarray(r64, np.float64)
    ok = _same_class(dev, r32) & np.isfinite(r64)
    if not ok.any():
        print(f'[bias_calc tolerance] {name}: nothing finite')
        return
    ref_err = float(np.abs(r32 - r64)[ok].max())
    bound = np.maximum(2 * ref_err, _ulp(r64)) + extra
    err = np.abs(dev - r64)
    print(f'[bias_calc tolerance] {name}: max|R32-R64| = {ref_err:.3e}, '
          f'device max err = {float(err[ok].max()):.3e}, extra = '
          f'{float(np.max(extra)):.3e}, device == R32 bitwise: '
          f'{bool(np.array_equal(dev[ok], r32[ok]))}')
    worst = float((err - bound)[ok].max())
    assert worst <= 0, (name, worst, ref_err)


def _quantile_rows(name, dev, series, q_count):
    """rows of one (pixel, window): ``dev`` (Q,) against np.quantile of the
    float32 ``series`` (n,)"""
    q = np.linspace(0, 1, q_count)
    want = np.quantile(series, q).astype(np.float32)
    if np.isnan(series).any():
        assert np.isnan(dev).all() and np.isnan(want).all(), name
        return 0.0
    s = np.sort(series)
    pos = (len(s) - 1) * q
    lo = np.floor(pos).astype(int)
    hi = np.minimum(lo + 1, len(s) - 1)
    bound = np.spacing(np.maximum(np.abs(s[lo]), np.abs(s[hi])))
    err = np.abs(dev.astype(np.float64) - want.astype(np.float64))
    assert (err <= bound).all(), (name, float((err - bound).max()))
    assert dev[0] == s[0], name                       # q = 0: the minimum
    if q_count > 1:
        assert dev[-1] == s[-1], name                 # q = 1: the maximum
    return float((err / np.maximum(bound, 1e-45)).max())


def _whole_window(n):
    return np.array([0, n], np.int32), np.arange(n, dtype=np.int32)


# ------------------------------------------------------------ sort lengths
@pytest.mark.parametrize('n', SORT_LENGTHS)
def test_window_quantiles_at_every_sort_length(n):
    """one window of n members scattered over a longer series, three pixels"""
    rng = np.random.default_rng(n)
    n_t = n + 5
    series = rng.normal(0, 3, (3, n_t)).astype(np.float32)
    member = np.sort(rng.permutation(n_t)[:n]).astype(np.int32)
    ptr = np.array([0, 0, n], np.int32)               # an empty window first
    be = _be()
    out = be.to_host(be.window_quantiles(be.upload(series), ptr, member, 7))
    assert out.shape == (3, 2, 7) and np.isnan(out[:, 0]).all()
    worst = max(_quantile_rows(f'n={n} p={p}', out[p, 1], series[p, member],
                               7) for p in range(3))
    print(f'[bias_calc tolerance] quantiles n={n}: worst err / bound = '
          f'{worst:.3f}')


@pytest.mark.parametrize('n', SORT_LENGTHS)
def test_match_zero_rate_at_every_sort_length(n):
    rng = np.random.default_rng(100 + n)
    bias = np.round(rng.gamma(0.5, 2.0, (3, n)), 1).astype(np.float32)
    base = rng.gamma(0.5, 2.0, (3, 40)).astype(np.float32)
    base[:, ::3] = 0
    base[1] = 1                                       # no zero at all
    base[2, 5] = np.nan
    be = _be()
    got, mv, bad = be.match_zero_rate(be.upload(base), be.upload(bias))
    got = be.to_host(got)
    assert bad == 0
    for p in range(3):
        want, mv_ref = R.match_zero_rate(bias[p].copy(), base[p])
        assert np.array_equal(got[p], want), (n, p)
        assert abs(mv[p] - mv_ref) <= 4 * np.spacing(abs(mv_ref)), (n, p)


def test_one_past_the_sort_limit_is_refused_with_the_outputs_untouched():
    import torch
    from sup3r_amd import _lib
    be = _be()
    n = _lib.BCC_MAX_SORT + 1
    series = be.upload(np.zeros((1, n), np.float32))
    ptr, member = _whole_window(n)
    with pytest.raises(ValueError, match='S3_BCC_MAX_SORT'):
        be.window_quantiles(series, ptr, member, 5)
    # the raw calls, with sentinels around the outputs
    L, ctx = _lib.lib(), be.dev.ctx
    out = torch.full((3, 5), 7.0, device=be.dev.torch_device)
    d_ptr, d_mem = be._ints(ptr), be._ints(member)
    rc = L.s3_bc_window_quantiles(
        ctx, be._p(series), 1, n, 1, ptr.ctypes.data_as(C.c_void_p),
        member.ctypes.data_as(C.c_void_p), be._p(d_ptr), be._p(d_mem), 5,
        C.c_void_p(out[1].data_ptr()))
    assert rc == -1 and 'S3_BCC_MAX_SORT' in _lib.last_error(ctx)
    base = be.upload(np.zeros((1, 4), np.float32))
    bad = torch.full((3,), 7, dtype=torch.int32, device=be.dev.torch_device)
    mv = torch.full((3,), 7.0, dtype=torch.float64,
                    device=be.dev.torch_device)
    rc = L.s3_bc_match_zero_rate(
        ctx, be._p(base), 4, be._p(series), 1, n,
        C.c_void_p(mv[1:].data_ptr()), C.c_void_p(bad[1:].data_ptr()))
    assert rc == -1 and 'S3_BCC_MAX_SORT' in _lib.last_error(ctx)
    be.dev.sync()
    assert (out.cpu().numpy() == 7).all() and (bad.cpu().numpy() == 7).all()
    assert (mv.cpu().numpy() == 7).all()
    assert (series.cpu().numpy() == 0).all()


def test_bad_indices_and_counts_are_refused():
    be = _be()
    series = be.upload(np.zeros((2, 10), np.float32))
    ptr, member = _whole_window(10)
    with pytest.raises(ValueError, match='at least one quantile'):
        be.window_quantiles(series, ptr, member, 0)
    for bad_member in (member + 1, member - 1):
        with pytest.raises(ValueError, match='out of range'):
            be.window_quantiles(series, ptr, bad_member, 3)
    with pytest.raises(ValueError, match='out of range'):
        be.window_quantiles(series, np.array([0, 5, 3], np.int32), member, 3)
    for group in ([0] * 9 + [1], [0] * 9 + [-2]):
        with pytest.raises(ValueError, match='group id'):
            be.moments(series, group, 1)
    with pytest.raises(ValueError, match='groups'):
        be.moments(series, [0] * 10, 13)
    base = np.zeros((4, 3), np.float32)
    days = (np.array([0, 2, 4], np.int32), np.arange(4, dtype=np.int32), 0)
    sites = np.array([0, 1, 3], np.int32)
    with pytest.raises(ValueError, match='site list'):
        be.base_series([(base, None)], sites, [0, 1, 3], [days], 2, 0)
    with pytest.raises(ValueError, match='day list'):
        be.base_series([(base, None)], sites, [0, 1, 2],
                       [(days[0], days[1] + 1, 0)], 2, 0)
    with pytest.raises(ValueError, match='leave the output'):
        be.base_series([(base, None)], sites, [0, 1, 2],
                       [(days[0], days[1], 1)], 2, 0)


# -------------------------------------------------------------- data cases
@pytest.mark.parametrize('case', ['all_equal', 'ties', 'zeros', 'one_nan'])
def test_window_quantiles_data_cases(case):
    rng = np.random.default_rng(3)
    n = 301
    series = rng.normal(0, 2, (2, n)).astype(np.float32)
    if case == 'all_equal':
        series[:] = np.float32(0.1)
    elif case == 'ties':
        series = np.round(series, 1)
    elif case == 'zeros':
        series[:, ::2] = 0.0
        series[:, 1::2] = -0.0
    else:
        series[1, 17] = np.nan
    be = _be()
    ptr, member = _whole_window(n)
    out = be.to_host(be.window_quantiles(be.upload(series), ptr, member, 50))
    for p in range(2):
        _quantile_rows(f'{case} p={p}', out[p, 0], series[p], 50)
    if case == 'zeros':
        # -0 sorts in front of +0: the key fixes what a float compare leaves open
        assert np.signbit(out[:, 0, :24]).all()
        assert not np.signbit(out[:, 0, 25:]).any()
    if case == 'one_nan':
        assert np.isnan(out[1]).all() and not np.isnan(out[0]).any()


@pytest.mark.parametrize('n_q', [1, 2, 50, 101])
def test_more_quantiles_than_members(n_q):
    rng = np.random.default_rng(n_q)
    series = rng.normal(0, 2, (5, 9)).astype(np.float32)
    member = np.array([7, 1, 4, 2, 8], np.int32)
    be = _be()
    out = be.to_host(be.window_quantiles(
        be.upload(series), np.array([0, 5], np.int32), member, n_q))
    assert out.shape == (5, 1, n_q)
    for p in range(5):
        _quantile_rows(f'Q={n_q} p={p}', out[p, 0], series[p, member], n_q)
    if n_q == 1:
        assert np.array_equal(out[:, 0, 0], series[:, member].min(axis=1))


# -------------------------------------------------- pixel and site counts
def _ragged_days(rng, shuffle=True):
    """days of 1, 23, 24 and 25 steps, then a leap day's 24: any order"""
    parts = []
    for day, k in (('2020-02-26', 1), ('2020-02-27', 23), ('2020-02-28', 24),
                   ('2020-02-29', 25), ('2020-12-31', 24)):
        parts.append(pd.Timestamp(day) + pd.to_timedelta(
            np.arange(k) * (86400 // k), unit='s'))
    ti = pd.DatetimeIndex(np.hstack(parts))
    return ti[rng.permutation(len(ti))] if shuffle else ti


def _site_lists(rng, n_pix, n_sites):
    counts = [(0, 1, 3, 70)[p % 4] for p in range(n_pix)]
    lists = [np.sort(rng.permutation(n_sites)[:c]) for c in counts]
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    idx = np.concatenate(lists).astype(np.int32)
    return ptr, idx, lists


@pytest.mark.parametrize('red', ['avg', 'max', 'min', 'sum', None])
@pytest.mark.parametrize('n_pix', [1, 5, 67])
def test_base_series(n_pix, red):
    """sites per pixel 0, 1, 3, 70; NaN sites, a step whose sites are all NaN,
    a day whose steps are all NaN; two launches write one series"""
    from sup3r_amd import bias_calc as B
    rng = np.random.default_rng(n_pix)
    n_sites = 80
    ti_a = _ragged_days(rng)
    ti_b = pd.date_range('2021-01-01', periods=30, freq='8h')
    ptr, idx, lists = _site_lists(rng, n_pix, n_sites)
    arrs = []
    for ti in (ti_a, ti_b):
        a = rng.normal(1, 2, (len(ti), n_sites)).astype(np.float32)
        a[rng.random(a.shape) < 0.05] = np.nan
        a[3] = np.nan                                  # every site of a step
        arrs.append(a)
    arrs[1][ti_b.normalize() == pd.Timestamp('2021-01-03')] = np.nan
    plans, base_ti = B.day_plan(list(zip(arrs, (ti_a, ti_b))),
                                reduce=red is not None)
    code = B.REDUCTIONS[red or 'none']
    be = _be()
    out = be.to_host(be.base_series(
        [(a, None) for a in arrs], ptr, idx, plans, len(base_ti), code,
        flags=1))
    assert out.shape == (n_pix, len(base_ti))
    for p, gid in enumerate(lists):
        if not len(gid):
            assert np.isnan(out[p]).all()
            continue
        with R.quiet():
            r32, t32 = R.get_base_data(
                [(a, ti, None) for a, ti in zip(arrs, (ti_a, ti_b))], 'x',
                gid, daily_reduction=red)
            r64, _ = R.get_base_data(
                [(a.astype(np.float64), ti, None)
                 for a, ti in zip(arrs, (ti_a, ti_b))], 'x', gid,
                daily_reduction=red)
        assert list(t32) == list(base_ti)
        if red in ('max', 'min', None) and len(gid) == 1:
            assert np.array_equal(out[p], r32, equal_nan=True), p
        elif p < 8:
            _rule(f'base_series {red} P={n_pix} p={p} sites={len(gid)}',
                  out[p], r32, r64)
        else:
            _rule_quiet(out[p], r32, r64)


def _rule_quiet(dev, r32, r64):
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        _rule('', dev, r32, r64)


@pytest.mark.parametrize('mode', ['clearsky_ratio', 'decimals', 'raster'])
def test_base_series_modes(mode):
    from sup3r_amd import bias_calc as B
    rng = np.random.default_rng(11)
    ti = _ragged_days(rng, shuffle=False)
    n_sites = 12
    ptr = np.array([0, 1, 4, 12], np.int32)
    idx = np.arange(12, dtype=np.int32)
    ghi = np.maximum(0, rng.normal(300, 200, (len(ti), n_sites))).astype(
        np.float32)
    cs = (ghi * rng.uniform(1, 1.5, ghi.shape)).astype(np.float32)
    day3 = ti.normalize() == pd.Timestamp('2020-02-28')
    cs[day3] = 0                                       # a night-only day
    flags, dec, dset = 1, 0, 'x'
    if mode == 'clearsky_ratio':
        flags, dset = 1 | 2, 'clearsky_ratio'
    elif mode == 'decimals':
        flags, dec = 1 | 4, 2
        ghi = (ghi / 100).astype(np.float32)
    else:
        flags = 0
        ghi[5, 7] = np.nan                             # a plain mean keeps it
    plans, base_ti = B.day_plan([(ghi, ti)], reduce=True)
    be = _be()
    out = be.to_host(be.base_series(
        [(ghi, cs if mode == 'clearsky_ratio' else None)], ptr, idx, plans,
        len(base_ti), 0, flags=flags, decimals=dec))
    for p in range(3):
        gid = idx[ptr[p]:ptr[p + 1]]
        kw = dict(raster=mode == 'raster', daily_reduction='avg',
                  decimals=2 if mode == 'decimals' else None)
        has_cs = mode == 'clearsky_ratio'
        with R.quiet():
            r32, _ = R.get_base_data(
                [(ghi, ti, cs if has_cs else None)], dset, gid, **kw)
            r64, _ = R.get_base_data(
                [(ghi.astype(np.float64), ti,
                  cs.astype(np.float64) if has_cs else None)], dset, gid,
                **kw)
        _rule(f'base_series {mode} p={p}', out[p], r32, r64)
        if mode == 'clearsky_ratio':
            assert out[p, 2] == 0                      # base.py:747
        if mode == 'raster':
            assert not np.isnan(out[p]).any()          # the day skips the step


# ----------------------------------------------------------------- moments
@pytest.mark.parametrize('n_groups', [1, 12])
@pytest.mark.parametrize('n_pix', [1, 5, 67])
def test_moments(n_pix, n_groups):
    """months absent from the series (May .. July, December), steps of no
    group, NaNs, a month without a valid value, day 366"""
    rng = np.random.default_rng(n_pix + n_groups)
    ti = pd.date_range('2020-08-01', '2021-04-30', freq='D')
    ti = ti[ti.month != 12].append(pd.DatetimeIndex(['2020-12-31']))
    assert ti[-1].day_of_year == 366
    series = rng.normal(3, 2, (n_pix, len(ti))).astype(np.float32)
    series[rng.random(series.shape) < 0.05] = np.nan
    series[:, ti.month == 2] = np.nan                  # nothing valid
    group = np.asarray(ti.month - 1, np.int32) if n_groups == 12 else \
        np.zeros(len(ti), np.int32)
    group[5:9] = -1
    be = _be()
    cnt, mean, std = be.moments(be.upload(series), group, n_groups)
    assert cnt.shape == mean.shape == std.shape == (n_pix, n_groups)
    r = {}
    with R.quiet():
        for dt in (np.float32, np.float64):
            m = np.full((n_pix, n_groups), np.nan, dt)
            s = np.full((n_pix, n_groups), np.nan, dt)
            for p in range(n_pix):
                for g in range(n_groups):
                    sel = series[p, group == g].astype(dt)
                    if len(sel):
                        m[p, g], s[p, g] = np.nanmean(sel), np.nanstd(sel)
            r[dt] = (m, s)
    want_cnt = np.stack([[(~np.isnan(series[p, group == g])).sum()
                          for g in range(n_groups)] for p in range(n_pix)])
    assert np.array_equal(cnt, want_cnt)
    if n_groups == 12:
        assert (cnt[:, [1, 4, 5, 6]] == 0).all() and (cnt[:, 11] <= 1).all()
        assert np.isnan(mean[:, [1, 4, 5, 6]]).all()
    _rule(f'moments mean P={n_pix} NT={n_groups}', mean, r[np.float32][0],
          r[np.float64][0])
    _rule(f'moments std P={n_pix} NT={n_groups}', std, r[np.float32][1],
          r[np.float64][1])


def test_match_zero_rate_refuses_nothing_but_counts_non_finite_values():
    be = _be()
    bias = np.arange(12, dtype=np.float32).reshape(2, 6)
    bias[1, 2] = np.inf
    base = np.zeros((2, 4), np.float32)
    got, mv, bad = be.match_zero_rate(be.upload(base), be.upload(bias))
    assert bad == 1 and np.isnan(mv[1])
    got = be.to_host(got)
    assert np.array_equal(got[1], bias[1])             # left as it is
    assert (got[0] == [0, 0, 0, 0, 0, 5]).all()        # all below the maximum


# ----------------------------------------------------------------- presrat
@functools.lru_cache(None)
def _presrat_case():
    """five pixels with tables computed by the reference in float32"""
    rng = np.random.default_rng(21)
    n_pix, n_w, n_q = 5, 6, 11
    base_ti = pd.date_range('2019-01-01', periods=700, freq='D')
    bias_ti = pd.date_range('2019-01-01', periods=730, freq='D')
    fut_ti = pd.date_range('2051-01-01', periods=731, freq='D')

    def mk(m, n):
        return np.maximum(0, rng.normal(m, 1, (n_pix, n))).astype(np.float32)
    base, bias, fut = mk(0.3, 700), mk(0.6, 730), mk(0.8, 731)
    base[1, 10:20] = np.nan                             # not counted
    bias[2] = np.round(bias[2], 1)                      # ties around tau
    return n_w, n_q, (base_ti, bias_ti, fut_ti), (base, bias, fut)


@pytest.mark.parametrize('relative', [True, False])
def test_presrat_kernel(relative):
    from sup3r_amd import bias_calc as B
    n_w, n_q, tis, (base, bias, fut) = _presrat_case()
    n_pix = len(base)
    centers, size = B.window_center(n_w), 100
    lists = [B.window_members(ti.day_of_year, centers, size) for ti in tis]
    last = B.last_window(fut.shape[1], *lists[2])
    assert (last < 0).sum() == 0
    with R.quiet():
        r32 = [R.run_single_presrat(
            bias[p], fut[p], base[p], *tis, 'pr', 'obs', n_q, n_w, size,
            relative, THRESHOLD) for p in range(n_pix)]
    # the kernel maps with the float32 tables of R32: its own R64 is the
    # mapping of those tables in float64
    keys = ('base_obs_params', 'bias_pr_params', 'bias_fut_pr_params')
    tables = [np.stack([r32[p][k] for p in range(n_pix)]) for k in keys]
    tables[0][1, 2] = np.nan                            # a window without rows
    be = _be()
    res = be.presrat(be.upload(base), be.upload(bias), be.upload(fut),
                     [be.upload(t.reshape(n_pix, -1)).reshape(t.shape)
                      for t in tables], relative, THRESHOLD, last, lists)
    assert not res['status'].any()
    c32 = np.full(fut.shape, np.nan, np.float32)
    c64 = np.full(fut.shape, np.nan, np.float64)
    with R.quiet():
        for p in range(n_pix):
            for w in range(n_w):
                m = lists[2][1][lists[2][0][w]:lists[2][0][w + 1]]
                for c, dt in ((c32, np.float32), (c64, np.float64)):
                    c[p, m] = R.qdm_row(
                        fut[p, m].astype(dt), *(t[p, w] for t in tables),
                        relative, THRESHOLD)
    _rule(f'presrat corrected relative={relative}', res['corrected'], c32,
          c64)
    assert np.isnan(res['corrected'][1]).any()
    corr_err = np.nanmax(np.abs(res['corrected'] - c64), axis=1)
    for p in range(n_pix):
        rate = R.zero_precipitation_rate(base[p], THRESHOLD)
        assert res['zero_rate'][p] == np.float32(rate)
        nth = min(round(rate * bias[p].size), bias[p].size - 1)
        tau = np.sort(bias[p])[nth]
        assert res['tau'][p] == tau
        z_fg = (fut[p] < tau).astype('i').sum() / fut[p].size
        assert res['z_fg'][p] == np.float32(z_fg)
        idx = round(z_fg * fut[p].size)
        # an order statistic of the corrected series: 1-Lipschitz
        want = np.sort(c64[p])[idx]
        bound = corr_err[p] + _ulp(want)
        assert abs(res['tau_fut'][p] - want) <= bound, p
        assert res['tau_fut'][p] == np.sort(res['corrected'][p])[idx]
    k32, k64 = [], []
    with R.quiet():
        for c, dt, k in ((c32, np.float32, k32), (c64, np.float64, k64)):
            for p in range(n_pix):
                k.append(R.calc_k_factor(
                    base[p].astype(dt), bias[p].astype(dt),
                    fut[p].astype(dt), c[p], *tis, centers, size, n_w,
                    THRESHOLD, store=dt))
    _rule(f'presrat k_factor relative={relative}', res['k_factor'],
          np.stack(k32), np.stack(k64))
    assert np.isnan(res['k_factor'][1]).any()           # plain means keep NaN
    assert np.isfinite(res['k_factor'][0]).all()


def test_presrat_counts_non_finite_series_and_the_index_error():
    from sup3r_amd import bias_calc as B
    n_w, n_q, tis, (base, bias, fut) = _presrat_case()
    centers, size = B.window_center(n_w), 100
    lists = [B.window_members(ti.day_of_year, centers, size) for ti in tis]
    last = B.last_window(fut.shape[1], *lists[2])
    be = _be()
    tables = [be.upload(np.ones((5, n_w * n_q), np.float32)).reshape(
        5, n_w, n_q) for _ in range(3)]
    bias, fut = bias.copy(), fut.copy()
    bias[0, 3] = np.nan
    fut[1, 4] = np.inf
    fut[1, 5] = np.nan
    fut[2] = -1                                         # everything below tau
    base = base.copy()
    base[2] = 1                                         # rate 0: tau = min(bias)
    res = be.presrat(be.upload(base), be.upload(bias), be.upload(fut), tables,
                     True, THRESHOLD, last, lists)
    assert list(res['status']) == [1, 2, 1]
    assert np.isnan(res['tau_fut'][2])


# ------------------------------------------------------------- class level
@functools.lru_cache(None)
def _inputs(layout):
    return R.seeded_inputs(layout)


def _kwargs(kind, layout, **extra):
    kw = dict(_inputs(layout))
    if kind in R.LINEAR:
        kw.pop('bias_fut_data')
        kw.pop('bias_fut_time_index')
    else:
        kw.update(QDM_KW)
    kw.update(extra)
    return kw


_REF = {}


def _reference(kind, layout, run_kw=(), **extra):
    """(R32, R64, extras32, extras64) of one case, computed once"""
    key = (kind, layout, run_kw, tuple(sorted(extra.items())))
    if key not in _REF:
        kw = _kwargs(kind, layout, **extra)
        e32, e64 = {}, {}
        _REF[key] = (
            R.run(kind, kw, np.float32, extras=e32, fill_extend=False,
                  **dict(run_kw)),
            R.run(kind, kw, np.float64, extras=e64, fill_extend=False,
                  **dict(run_kw)), e32, e64)
    return _REF[key]


def _linear_bounds(r32, r64, scalar_only):
    """The bounds of ``scalar`` and ``adder``: float32 expressions of moments
    that each lie within ``b_x = max(2 |R32 - R64|, ulp)`` of R64.
      scalar = s_o / s_b:  |d scalar| <= (b_so + |scalar| b_sb) / s_b
                           + ulp(scalar)            [the division's rounding]
      scalar = m_o / m_b likewise (ScalarCorrection)
      adder = m_o - m_b scalar:  |d adder| <= b_mo + |scalar| b_mb
                           + |m_b| |d scalar| + ulp(m_b scalar) + ulp(adder)"""
    def b(key):
        ok = np.isfinite(r64[key]) & np.isfinite(r32[key])
        err = np.abs(r32[key].astype(np.float64) - r64[key])[ok]
        return np.maximum(2 * (err.max() if err.size else 0.0),
                          _ulp(r64[key]))
    with np.errstate(all='ignore'):
        sc = np.abs(r64['pr_scalar'])
        num, den = ('base_pr_obs_mean', 'bias_pr_mean') if scalar_only else \
            ('base_pr_obs_std', 'bias_pr_std')
        d_scalar = (b(num) + sc * b(den)) / np.abs(r64[den]) + _ulp(sc)
        m_b = np.abs(r64['bias_pr_mean'])
        d_adder = (b('base_pr_obs_mean') + sc * b('bias_pr_mean')
                   + m_b * d_scalar + _ulp(m_b * sc)
                   + _ulp(r64['pr_adder']))
    return d_scalar, d_adder


def _check_linear(name, out, r32, r64, scalar_only):
    for key in ('bias_pr_mean', 'base_pr_obs_mean', 'bias_pr_std',
                'base_pr_obs_std'):
        _rule(f'{name} {key}', out[key], r32[key], r64[key])
    d_scalar, d_adder = _linear_bounds(r32, r64, scalar_only)
    for key, bound in (('pr_scalar', d_scalar), ('pr_adder', d_adder)):
        ok = _same_class(out[key], r32[key])
        err = np.abs(out[key].astype(np.float64) - r64[key])
        print(f'[bias_calc tolerance] {name} {key}: device max err = '
              f'{float(err[ok].max()):.3e}, smallest bound = '
              f'{float(bound[ok].min()):.3e}, max|R32-R64| = '
              f'{float(np.abs(r32[key] - r64[key])[ok].max()):.3e}')
        assert (err <= bound)[ok].all(), (name, key,
                                          float((err - bound)[ok].max()))


def _series_error(dev_series, per_pixel):
    """max |device series - R64 series| over the pixels that have one"""
    host = _be().to_host(dev_series).astype(np.float64)
    err = 0.0
    for gid, want in per_pixel.items():
        d = np.abs(host[gid] - want)
        assert np.array_equal(np.isnan(host[gid]), np.isnan(want))
        if np.isfinite(d).any():
            err = max(err, float(np.nanmax(d)))
    return err


def _check_tables(name, calc, out, r32, r64, e64, daily_reduction='avg'):
    base_dev, _ = calc._base_series(daily_reduction)
    base_err = _series_error(base_dev, e64['base'])
    for key, extra in (('base_pr_obs_params', base_err),
                       ('bias_pr_params', 0.0), ('bias_fut_pr_params', 0.0)):
        ok = _same_class(out[key], r32[key])
        err = np.abs(out[key].astype(np.float64) - r64[key])
        bound = extra + _ulp(r64[key])
        print(f'[bias_calc tolerance] {name} {key}: series err = '
              f'{extra:.3e}, device max err = {float(err[ok].max()):.3e}, '
              f'max|R32-R64| = '
              f'{float(np.abs(r32[key] - r64[key])[ok].max()):.3e}')
        assert (err <= bound)[ok].all(), (name, key,
                                          float((err - bound)[ok].max()))
    return base_err


@pytest.mark.parametrize('layout', ['sites', 'raster'])
@pytest.mark.parametrize('kind', KINDS)
def test_classes_against_the_per_pixel_loop(kind, layout):
    import sup3r_amd
    run_kw = (('zero_rate_threshold', THRESHOLD),) if kind == 'PresRat' \
        else ()
    calc = getattr(sup3r_amd, kind)(**_kwargs(kind, layout))
    out = calc.run(fill_extend=False, **dict(run_kw))
    r32, r64, _, e64 = _reference(kind, layout, run_kw)
    assert list(out) == list(r32)
    name = f'{kind} {layout}'
    for key, v in out.items():
        assert v.dtype == np.float32 and v.shape == r32[key].shape, key
        assert np.isnan(v[:, 3]).all(), key             # the bad pixels
    if kind in R.LINEAR:
        _check_linear(name, out, r32, r64, 'Scalar' in kind)
        return
    _check_tables(name, calc, out, r32, r64, e64)
    if kind == 'PresRat':
        assert np.array_equal(out['pr_obs_zero_rate'],
                              r32['pr_obs_zero_rate'], equal_nan=True)
        corr = calc.corrected_fut_data.reshape(12, -1).astype(np.float64)
        corr_err = max(float(np.nanmax(np.abs(corr[g] - c)))
                       for g, c in e64['corrected'].items())
        want = r64['pr_tau_fut']
        ok = _same_class(out['pr_tau_fut'], r32['pr_tau_fut'])
        err = np.abs(out['pr_tau_fut'] - want)
        print(f'[bias_calc tolerance] {name} tau_fut: corrected err = '
              f'{corr_err:.3e}, device max err = {float(err[ok].max()):.3e}')
        assert (err <= corr_err + _ulp(want))[ok].all()
        _rule(f'{name} k_factor', out['pr_k_factor'], r32['pr_k_factor'],
              r64['pr_k_factor'])


@pytest.mark.parametrize('red', ['avg', 'max', 'min', 'sum', None])
def test_daily_reductions_through_a_class(red):
    import sup3r_amd
    run_kw = (('daily_reduction', red),)
    years = dict(base_data=_inputs('sites')['base_data'][:1]) if red is None \
        else {}
    calc = sup3r_amd.MonthlyLinearCorrection(
        **_kwargs('MonthlyLinearCorrection', 'sites', **years))
    out = calc.run(fill_extend=False, daily_reduction=red)
    key = ('MonthlyLinearCorrection', 'sites', red)
    if key not in _REF:
        kw = _kwargs('MonthlyLinearCorrection', 'sites', **years)
        _REF[key] = tuple(R.run('MonthlyLinearCorrection', kw, dt,
                                fill_extend=False, **dict(run_kw))
                          for dt in (np.float32, np.float64))
    r32, r64 = _REF[key]
    _check_linear(f'MonthlyLinearCorrection daily_reduction={red}', out, r32,
                  r64, False)


@pytest.mark.parametrize('option', ['clearsky_ratio', 'match_zero_rate',
                                    'decimals'])
def test_options_through_a_class(option):
    import sup3r_amd
    inp = _inputs('sites')
    extra = {}
    if option == 'clearsky_ratio':
        rng = np.random.default_rng(9)
        extra = dict(base_dset='clearsky_ratio', base_cs_ghi=[
            (np.nan_to_num(a) * rng.uniform(1, 2, a.shape)).astype(np.float32)
            for a, _ in inp['base_data']])
    elif option == 'match_zero_rate':
        extra = dict(match_zero_rate=True)
    else:
        extra = dict(decimals=2)
    kw = _kwargs('LinearCorrection', 'sites', **extra)
    out = sup3r_amd.LinearCorrection(**kw).run(fill_extend=False)
    r32, r64 = (R.run('LinearCorrection', kw, dt, fill_extend=False)
                for dt in (np.float32, np.float64))
    if option == 'clearsky_ratio':
        r32 = {k.replace('clearsky_ratio', 'pr_obs'): v
               for k, v in r32.items()}
        r64 = {k.replace('clearsky_ratio', 'pr_obs'): v
               for k, v in r64.items()}
        out = {k.replace('clearsky_ratio', 'pr_obs'): v
               for k, v in out.items()}
    _check_linear(f'LinearCorrection {option}', out, r32, r64, False)


# -------------------------------------------------------------- end to end
def _identity_inputs():
    """base = bias = bias_fut: the base "sites" are the grid's own points,
    daily, so that the site mean and the daily mean copy the series"""
    inp = _inputs('raster')
    rng = np.random.default_rng(4)
    ti = pd.date_range('2019-01-01', '2021-12-31', freq='D')
    data = (5 + rng.gamma(2.0, 1.0, (3, 4, len(ti)))).astype(np.float32)
    return dict(base_data=(data.copy(), ti), bias_data=data,
                bias_fut_data=data.copy(), base_dset='obs',
                bias_feature='f', base_lat_lon=inp['bias_lat_lon'],
                bias_lat_lon=inp['bias_lat_lon'], bias_time_index=ti,
                bias_fut_time_index=ti), data, ti


@pytest.mark.parametrize('relative', [True, False])
def test_identity_tables_return_the_input(relative, tmp_path):
    """the reference's test_bc_identity(_absolute): three identical
    distributions change nothing (np.allclose, as there)"""
    import sup3r_amd
    inp, data, ti = _identity_inputs()
    fp = str(tmp_path / 'identity.npz')
    calc = sup3r_amd.QuantileDeltaMappingCorrection(
        n_quantiles=51, n_time_steps=12, window_size=60, **inp)
    out = calc.run(fp_out=fp)
    assert np.array_equal(out['base_obs_params'], out['bias_f_params'])
    assert np.array_equal(out['base_obs_params'], out['bias_fut_f_params'])
    assert not np.isnan(out['base_obs_params']).any()
    corrected = sup3r_amd.local_qdm_bc(
        data, inp['bias_lat_lon'], 'obs', 'f', fp, ti, relative=relative)
    assert corrected.shape == data.shape
    assert np.allclose(corrected, data)


def test_monthly_factors_give_the_bias_series_the_moments_of_the_base(
        tmp_path):
    """after monthly_local_linear_bc with the computed factors the corrected
    bias series has the base's monthly mean and std: within the moments'
    tolerance scaled by |scalar| (the correction multiplies every error of
    the series by it), plus the float32 roundings of ``x scalar + adder``
    (two ulps of the largest term) that a mean cannot average away"""
    import sup3r_amd
    kw = _kwargs('MonthlyLinearCorrection', 'sites')
    fp = str(tmp_path / 'monthly.npz')
    out = sup3r_amd.MonthlyLinearCorrection(**kw).run(fp_out=fp)
    ti = kw['bias_time_index']
    corrected = sup3r_amd.monthly_local_linear_bc(
        kw['bias_data'], kw['bias_lat_lon'], 'pr', fp, ti,
        temporal_avg=False)
    r32, r64, _, _ = _reference('MonthlyLinearCorrection', 'sites')
    good = ~np.isnan(r64['pr_scalar'][..., 0])
    worst = 0.0
    for m in range(12):
        sel = np.asarray(ti.month == m + 1)
        got_mean = corrected[..., sel].astype(np.float64).mean(axis=-1)
        got_std = corrected[..., sel].astype(np.float64).std(axis=-1)
        sc = np.abs(out['pr_scalar'][..., m]).astype(np.float64)
        big = np.abs(kw['bias_data'][..., sel]).max(axis=-1) * sc + np.abs(
            out['pr_adder'][..., m])
        for got, key in ((got_mean, 'base_pr_obs_mean'),
                         (got_std, 'base_pr_obs_std')):
            want = r64[key][..., m]
            ref_err = np.abs(r32[key].astype(np.float64) - r64[key])[
                np.isfinite(r64[key])].max()
            bias_key = key.replace('base_pr_obs', 'bias_pr')
            bias_err = np.abs(r32[bias_key].astype(np.float64)
                              - r64[bias_key])[np.isfinite(
                                  r64[bias_key])].max()
            tol = (np.maximum(2 * ref_err, _ulp(want))
                   + np.maximum(1.0, sc) * np.maximum(
                       2 * bias_err, _ulp(r64[bias_key][..., m]))
                   + 2 * _ulp(big))
            err = np.abs(got - want)
            assert (err <= tol)[good].all(), (m, key, float(
                (err - tol)[good].max()))
            worst = max(worst, float((err / tol)[good].max()))
    print(f'[bias_calc tolerance] monthly end to end: worst err / bound = '
          f'{worst:.3f}')


def test_presrat_tables_zero_exactly_the_values_below_tau_fut(tmp_path):
    import sup3r_amd
    kw = _kwargs('PresRat', 'sites')
    fp = str(tmp_path / 'presrat.npz')
    calc = sup3r_amd.PresRat(**kw)
    out = calc.run(fp_out=fp, zero_rate_threshold=THRESHOLD)
    ti = kw['bias_fut_time_index']
    data = kw['bias_fut_data']
    lat_lon = kw['bias_lat_lon']
    args = (data, lat_lon, 'pr_obs', 'pr', fp, ti)
    qdm = sup3r_amd.local_qdm_bc(*args, delta_denom_min=THRESHOLD)
    got = sup3r_amd.local_presrat_bc(*args)
    assert got.shape == data.shape and np.isfinite(got).all()
    tau = out['pr_tau_fut']                             # (3, 4, 1), filled
    assert np.array_equal(got == 0, (qdm < tau) | (qdm == 0))
    assert (got == 0).any() and (got != 0).any()
    k = out['pr_k_factor']
    from sup3r_amd import bias as B
    window = B.window_index(ti, calc.time_window_center)
    keep = qdm >= tau
    want = qdm * k[:, :, window]
    assert np.allclose(got[keep], want[keep], rtol=1e-6, atol=0)
