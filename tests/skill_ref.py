"""The reference's ``SkillAssessment`` (sup3r/bias/bias_calc.py:379-544)
followed line by line per pixel with its own numpy / scipy calls, on top of
``tests/bias_calc_ref.py`` (``get_base_data``, ``match_zero_rate``,
``get_linear_correction``, ``fill_and_smooth``).

``run(inp, dtype)`` evaluates the whole calculator in ``dtype`` (float32:
``R32``, the reference as it runs; float64: ``R64``, every input cast first) as
a Python loop over the pixels.

``run_skill_eval(forced_means=(base_mean, bias_mean))`` replaces the two means
in the KS subtraction only: the device's float32 mean (an fp64 sum rounded once) may
differ from numpy's pairwise float32 mean by an ulp, and the KS numerator is
discrete.

``ks_numerator`` is the integer KS statistic by brute force: both empirical
CDFs at every point of the union.  ``Backend`` adds ``skill`` to
``bias_calc_ref.Backend`` so that the class can be tested without a device."""
import numpy as np
import pandas as pd
from scipy import stats

from tests import bias_calc_ref as R

PERCENTILES = (1, 5, 25, 50, 75, 95, 99)
STAT_NAMES = ('mean', 'std', 'skew', 'kurtosis', 'zero_rate')


# ------------------------------------------------------------- bias_calc.py
def run_skill_eval(bias_data, base_data, bias_feature, base_dset,
                   match_zero_rate=False, forced_means=None):
    """bias_calc.py:431-481"""
    if match_zero_rate:
        bias_data, _ = R.match_zero_rate(bias_data, base_data)

    out = {}
    bias_mean = np.nanmean(bias_data)
    base_mean = np.nanmean(base_data)
    out[f'{bias_feature}_bias'] = bias_mean - base_mean

    out[f'bias_{bias_feature}_mean'] = bias_mean
    out[f'bias_{bias_feature}_std'] = np.nanstd(bias_data)
    out[f'bias_{bias_feature}_skew'] = stats.skew(bias_data)
    out[f'bias_{bias_feature}_kurtosis'] = stats.kurtosis(bias_data)
    out[f'bias_{bias_feature}_zero_rate'] = np.nanmean(bias_data == 0)

    out[f'base_{base_dset}_mean'] = base_mean
    out[f'base_{base_dset}_std'] = np.nanstd(base_data)
    out[f'base_{base_dset}_skew'] = stats.skew(base_data)
    out[f'base_{base_dset}_kurtosis'] = stats.kurtosis(base_data)
    out[f'base_{base_dset}_zero_rate'] = np.nanmean(base_data == 0)

    if match_zero_rate:
        ks_out = stats.ks_2samp(base_data, bias_data)
    else:
        if forced_means is not None:
            base_mean, bias_mean = (np.asarray(m, base_data.dtype)[()]
                                    for m in forced_means)
        ks_out = stats.ks_2samp(base_data - base_mean, bias_data - bias_mean)

    out[f'{bias_feature}_ks_stat'] = ks_out.statistic
    out[f'{bias_feature}_ks_p'] = ks_out.pvalue

    for p in PERCENTILES:
        base_k = f'base_{base_dset}_percentile_{p}'
        bias_k = f'bias_{bias_feature}_percentile_{p}'
        out[base_k] = np.percentile(base_data, p)
        out[bias_k] = np.percentile(bias_data, p)

    return out


def run_single_skill(bias_data, base_data, base_ti, bias_ti, bias_feature,
                     base_dset, match_zero_rate=False, store=np.float32):
    """bias_calc.py:483-544, behind ``get_base_data``.  As there, the monthly
    ``_scalar`` / ``_adder`` are computed and dropped."""
    arr = np.full(12, np.nan, dtype=store)
    out = {f'bias_{bias_feature}_mean_monthly': arr.copy(),
           f'bias_{bias_feature}_std_monthly': arr.copy(),
           f'base_{base_dset}_mean_monthly': arr.copy(),
           f'base_{base_dset}_std_monthly': arr.copy()}

    out.update(run_skill_eval(bias_data, base_data, bias_feature, base_dset,
                              match_zero_rate=match_zero_rate))

    for month in range(1, 13):
        bias_mask = bias_ti.month == month
        base_mask = base_ti.month == month

        if any(bias_mask) and any(base_mask):
            mout = R.get_linear_correction(bias_data[bias_mask],
                                           base_data[base_mask],
                                           bias_feature, base_dset)
            for k, v in mout.items():
                if not k.endswith(('_scalar', '_adder')):
                    k += '_monthly'
                    out[k][month - 1] = v

    return out


def init_out(shape, bias_feature, base_dset, store=np.float32):
    """bias_calc.py:385-428"""
    monthly_keys = [f'{bias_feature}_scalar', f'{bias_feature}_adder',
                    f'bias_{bias_feature}_mean_monthly',
                    f'bias_{bias_feature}_std_monthly',
                    f'base_{base_dset}_mean_monthly',
                    f'base_{base_dset}_std_monthly']
    annual_keys = [f'{bias_feature}_ks_stat', f'{bias_feature}_ks_p',
                   f'{bias_feature}_bias', f'bias_{bias_feature}_mean',
                   f'bias_{bias_feature}_std', f'bias_{bias_feature}_skew',
                   f'bias_{bias_feature}_kurtosis',
                   f'bias_{bias_feature}_zero_rate',
                   f'base_{base_dset}_mean', f'base_{base_dset}_std',
                   f'base_{base_dset}_skew', f'base_{base_dset}_kurtosis',
                   f'base_{base_dset}_zero_rate']
    out = {k: np.full((*shape, 12), np.nan, store) for k in monthly_keys}
    arr = np.full((*shape, 1), np.nan, store)
    for k in annual_keys:
        out[k] = arr.copy()
    for p in PERCENTILES:
        out[f'base_{base_dset}_percentile_{p}'] = arr.copy()
        out[f'bias_{bias_feature}_percentile_{p}'] = arr.copy()
    return out


def run(inp, dtype, daily_reduction='avg', fill_extend=True, smooth_extend=0,
        smooth_interior=0):
    """``SkillAssessment.run`` over the inputs ``inp`` (the keywords of the
    class as a dict) in ``dtype``, the tables stored in ``dtype`` too.
    As in ``bias_calc_ref.run`` a pixel is bad when no site maps to it."""
    bias_lat_lon = np.asarray(inp['bias_lat_lon'])
    base_lat_lon = np.asarray(inp['base_lat_lon'])
    raster = base_lat_lon.ndim == 3
    feat, dset = inp['bias_feature'], inp['base_dset']
    decimals = inp.get('decimals')
    mzr = inp.get('match_zero_rate', False)
    base_data = inp['base_data']
    if isinstance(base_data, tuple):
        base_data = [base_data]
    entries = [(R.site_major(a, base_lat_lon).astype(dtype, copy=False),
                pd.DatetimeIndex(ti), None) for a, ti in base_data]
    bias = np.asarray(inp['bias_data']).astype(dtype)
    bias_ti = pd.DatetimeIndex(inp['bias_time_index'])
    shape = bias.shape[:2]
    _, nn_ind = R.nn_query(bias_lat_lon, base_lat_lon,
                           inp.get('distance_upper_bound'))
    out = init_out(shape, feat, dset, store=dtype)
    for gid in range(shape[0] * shape[1]):
        base_gid = np.where(nn_ind == gid)[0]
        if len(base_gid) == 0:
            continue
        loc = np.unravel_index(gid, shape)
        bias_data = bias[loc]
        if decimals is not None:
            bias_data = np.around(bias_data, decimals=decimals)
        bias_data = np.array(bias_data)
        with R.quiet():
            base, base_ti = R.get_base_data(entries, dset, base_gid, raster,
                                            daily_reduction, decimals)
            single = run_single_skill(bias_data, base, base_ti, bias_ti,
                                      feat, dset, mzr, store=dtype)
        for key, arr in single.items():
            out[key][loc] = arr
    return R.fill_and_smooth(out, fill_extend, smooth_extend, smooth_interior)


# ------------------------------------------------------ the KS test, exactly
def ks_counts(x1, x2):
    """``(c1, c2)`` at the largest and at the smallest ``c1 n2 - c2 n1`` over
    every point of the union (the smallest ``c1`` among ties), with ``c =
    #(series <= point)`` counted by comparing every value with every point
    (no sort; beyond 2^28 comparisons: ``searchsorted`` on sorted copies), and
    ``(0, 0)`` where the difference never falls below 0."""
    x1, x2 = np.asarray(x1), np.asarray(x2)
    n1, n2 = len(x1), len(x2)
    pts = np.concatenate([x1, x2])
    c1 = np.empty(len(pts), np.int64)
    c2 = np.empty(len(pts), np.int64)
    if len(pts) * max(n1, n2) > 1 << 28:
        c1[:] = np.searchsorted(np.sort(x1), pts, side='right')
        c2[:] = np.searchsorted(np.sort(x2), pts, side='right')
        pts = pts[:0]
    step = max(1, (1 << 24) // max(n1, n2))
    for i in range(0, len(pts), step):
        chunk = pts[i:i + step, None]
        c1[i:i + step] = (x1[None, :] <= chunk).sum(axis=1)
        c2[i:i + step] = (x2[None, :] <= chunk).sum(axis=1)
    c1 = np.concatenate([[0], c1])
    c2 = np.concatenate([[0], c2])
    num = c1 * n2 - c2 * n1
    order = np.lexsort((c1, -num))
    hi = order[0]
    lo = np.lexsort((c1, num))[0]
    return int(c1[hi]), int(c2[hi]), int(c1[lo]), int(c2[lo])


def ks_counts_walk(x1, x2):
    """the four counts as ``s3_bc_skill`` finds them, restated in Python: only
    the ends of the runs of equal base values are visited, and only the
    sorted bias values are searched"""
    a, b = np.sort(x1), np.sort(x2)
    n1, n2 = len(a), len(b)
    hi, lo = [], [(-int(np.searchsorted(b, a[0], side='left')) * n1, 0)]
    for i in range(n1):
        last = i == n1 - 1
        if not last and a[i + 1] == a[i]:
            continue
        c1 = i + 1
        up = c1 * n2 - int(np.searchsorted(b, a[i], side='right')) * n1
        down = c1 * n2 - (n2 if last else int(
            np.searchsorted(b, a[i + 1], side='left'))) * n1
        hi.append((up, c1))
        lo.append((min(up, down), c1))
    n_hi = max(v for v, _ in hi)
    n_lo = min(v for v, _ in lo)
    c1p = min(c for v, c in hi if v == n_hi)
    c1m = min(c for v, c in lo if v == n_lo)
    return c1p, (c1p * n2 - n_hi) // n1, c1m, (c1m * n2 - n_lo) // n1


def ks_numerator(x1, x2):
    """the integer ``h`` with ``statistic = h / (n1 n2)``, two-sided"""
    c1p, c2p, c1m, c2m = ks_counts(x1, x2)
    n1, n2 = len(x1), len(x2)
    return max(c1p * n2 - c2p * n1, c2m * n1 - c1m * n2, 0)


# -------------------------------------------- the kernel's call, in numpy
(SK_MEAN, SK_STD, SK_SKEW, SK_KURTOSIS, SK_ZERO_RATE, SK_PCT0) = range(6)
SK_BIAS, SK_STATS, SK_NO_KS = 12, 13, -1


class Backend(R.Backend):
    """``bias_calc_ref.Backend`` plus ``skill``, computed in float32 with the
    calls of ``run_skill_eval``"""

    def skill(self, base_series, bias_series, demean):
        n_pix = len(base_series)
        res = {'stats': np.full((n_pix, 2, SK_STATS), np.nan, np.float32),
               'ks': np.full((n_pix, 4), SK_NO_KS, np.int32),
               'status': np.zeros((n_pix, 4), np.int32)}
        with R.quiet():
            for p in range(n_pix):
                rows = (np.asarray(base_series[p], np.float32),
                        np.asarray(bias_series[p], np.float32))
                for s, x in enumerate(rows):
                    st = res['stats'][p, s]
                    st[SK_MEAN] = np.nanmean(x)
                    st[SK_STD] = np.nanstd(x)
                    st[SK_SKEW] = stats.skew(x)
                    st[SK_KURTOSIS] = stats.kurtosis(x)
                    st[SK_ZERO_RATE] = np.nanmean(x == 0)
                    st[SK_PCT0:SK_BIAS] = [np.percentile(x, q)
                                           for q in PERCENTILES]
                    res['status'][p, 2 * s] = np.isnan(x).sum()
                    res['status'][p, 2 * s + 1] = (~np.isfinite(x)).sum()
                res['stats'][p, :, SK_BIAS] = (np.nanmean(rows[1])
                                               - np.nanmean(rows[0]))
                if demean:
                    rows = tuple(x - np.nanmean(x) for x in rows)
                if not any(np.isnan(x).any() for x in rows):
                    res['ks'][p] = ks_counts(*rows)
        return res
