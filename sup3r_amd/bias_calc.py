"""Computing bias-correction factors on the device.

The reference's calculators (sup3r/bias/bias_calc.py, qdm.py, presrat.py) under
their own names —

    LinearCorrection              bias_calc.py:21
    ScalarCorrection              :256
    MonthlyLinearCorrection       :311
    MonthlyScalarCorrection       :373
    SkillAssessment               :379
    QuantileDeltaMappingCorrection  qdm.py:35
    PresRat                       presrat.py:42

— with arrays in the place of files and handlers, as ``ArrayStrategy`` stands
in for ``ForwardPassStrategy``: ``bias_data`` ``(S1, S2, Tb)`` with
``bias_time_index`` and ``bias_lat_lon`` ``(S1, S2, 2)``; ``base_data`` one
``(array, time_index)`` pair or a list of them (one per "file", concatenated in
order), each array ``(T, n_sites)`` with ``base_lat_lon`` ``(n_sites, 2)`` (the
rex route: ``np.nanmean`` over the sites of a pixel, base.py:683-686) or
``(R1, R2, T)`` with ``base_lat_lon`` ``(R1, R2, 2)`` (the DataHandler route: a
plain mean, base.py:631); ``base_cs_ghi`` of the same layout for ``base_dset ==
'clearsky_ratio'``.  The keywords that are not about files keep the
reference's names and defaults.

The reference gives every low-res pixel to a process pool (abstract.py:79-97);
here the pixels are workgroups of six kernels (include/sup3r_hip.h):

    s3_bc_base_series       site mean + daily reduction -> (P, D)
    s3_bc_match_zero_rate   base.py:557-599
    s3_bc_moments           count, nanmean, nanstd per month
    s3_bc_window_quantiles  np.quantile per day-of-year window
    s3_bc_presrat           corrected future series, zero rate, tau_fut, k_factor
    s3_bc_skill             moments, zero rate, percentiles and the exact
                            two-sample KS counts of SkillAssessment

The host plans once per object (numpy / scipy): the KDTree mapping of base
sites to pixels and its default bound (base.py:175-182, 228-242), the day of
every base step, months, and the member lists of the day-of-year windows
(qdm.py:273-305, 583-623, restated verbatim — strict inequalities included:
with the default ``window_size = 365 / n_time_steps`` day 365 and 366 belong to
no window).  ``scalar`` / ``adder`` are formed on the host from the device's
float32 means and stds with the reference's float32 expressions, and
``fill_and_smooth`` (mixins.py:19-102) runs on the host over the finished
tables with the reference's own scipy calls: they are small and one-off.
``SkillAssessment``'s KS statistic and p-value are formed on the host from the
device's integer counts with scipy's own routines (``ks_from_counts``), once
per distinct numerator.

``run(fp_out=...)`` writes an ``.npz`` that ``BiasParams.load`` and the five
transforms of ``sup3r_amd.bias`` read back unchanged.

Deviations from the reference, on purpose:
  * pixels without a base site are the bad pixels; the reference's
    ``base_gid.any()`` also drops a pixel whose only site is site 0;
  * a day that spans two entries of ``base_data`` is a ``ValueError`` (the
    reference merges it);
  * ``match_zero_rate`` with non-finite bias values is a ``ValueError`` (the
    reference's ``sorted()`` on NaN is undefined); as in the reference, QDM and
    PresRat ignore ``match_zero_rate``;
  * an ``n_time_steps`` for which ``_window_center`` returns another number of
    centres is a ``ValueError`` (the reference indexes past its template);
  * only ``dist='empirical'`` with ``sampling='linear'``: anything else is a
    ``KeyError``;
  * a sorted series (a window, the bias series of ``match_zero_rate`` and
    PresRat, both series of ``SkillAssessment``) holds at most
    ``BCC_MAX_SORT`` = 32768 values: it is sorted in LDS.  Longer is a
    ``ValueError``;
  * ``SkillAssessment`` computes skew and kurtosis in float64 (scipy works in
    the float32 of its input), takes ``{feat}_bias`` between the float64
    means and rounds once (the reference subtracts two float32 means), and
    places its percentiles at the float64 ``(n - 1) p / 100`` (numpy >= 2
    evaluates that position in float32 for float32 data and a scalar ``p``);
    its KS test is two-sided only.

Not here: ``bias_calc_vortex.py``, the CLIs, reading h5 /
NetCDF, and deriving u / v from windspeed and direction (the caller passes the
derived series).
"""
import copy
import ctypes as C
import logging

import numpy as np

from . import _lib

logger = logging.getLogger(__name__)

__all__ = ['LinearCorrection', 'ScalarCorrection', 'MonthlyLinearCorrection',
           'MonthlyScalarCorrection', 'SkillAssessment',
           'QuantileDeltaMappingCorrection', 'PresRat']

REDUCTIONS = {'avg': _lib.BCC_AVG, 'average': _lib.BCC_AVG,
              'mean': _lib.BCC_AVG, 'max': _lib.BCC_MAX,
              'maximum': _lib.BCC_MAX, 'min': _lib.BCC_MIN,
              'minimum': _lib.BCC_MIN, 'sum': _lib.BCC_SUM,
              'total': _lib.BCC_SUM, 'none': _lib.BCC_NONE}
SORT_LIMIT = ('a sorted series may hold at most BCC_MAX_SORT = '
              f'{_lib.BCC_MAX_SORT} values (it is sorted in LDS)')


# ------------------------------------------------------------- host planning
def _time_index(ti):
    import pandas as pd
    return ti if isinstance(ti, pd.DatetimeIndex) else pd.DatetimeIndex(ti)


def default_distance_upper_bound(bias_lat_lon):
    """base.py:228-242 on the flattened ``(S1 * S2, 2)`` coordinates"""
    flat = np.asarray(bias_lat_lon).reshape(-1, 2)
    diff = np.diff(flat, axis=0)
    return np.max(np.median(diff, axis=0))


def site_mapping(bias_lat_lon, base_lat_lon, distance_upper_bound=None):
    """base.py:175-182: every base site to its nearest pixel within the bound,
    as the CSR list of sites per pixel.  Returns ``(site_ptr (P + 1), site_idx,
    nn_ind, bound)``; ``nn_ind == P`` marks a site beyond the bound."""
    from scipy.spatial import KDTree
    flat = np.asarray(bias_lat_lon).reshape(-1, 2)
    if distance_upper_bound is None:
        distance_upper_bound = default_distance_upper_bound(bias_lat_lon)
    _, nn_ind = KDTree(flat).query(np.asarray(base_lat_lon).reshape(-1, 2),
                                   distance_upper_bound=distance_upper_bound)
    n_pix = len(flat)
    order = np.argsort(nn_ind, kind='stable')
    order = order[nn_ind[order] < n_pix]
    counts = np.bincount(nn_ind[nn_ind < n_pix], minlength=n_pix)
    site_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return site_ptr, order.astype(np.int32), nn_ind, distance_upper_bound


def window_center(ntimes):
    """qdm.py:273-305"""
    assert ntimes > 0, 'Requires a positive number of intervals'
    dt = 365 / ntimes
    return np.arange(dt / 2, 366, dt)


def window_mask(doy, d0, window_size):
    """qdm.py:583-623"""
    d_start = d0 - window_size / 2
    d_end = d0 + window_size / 2
    if d_start < 0:
        idx = (doy > 365 + d_start) | (doy < d_end)
    elif d_end > 365:
        idx = (doy > d_start) | (doy < d_end - 365)
    else:
        idx = (doy > d_start) & (doy < d_end)
    return idx


def window_members(doy, centers, window_size):
    """the steps of every window as a CSR list ``(win_ptr (W + 1), member)``:
    ``member[win_ptr[w]:win_ptr[w + 1]] == np.where(window_mask(doy,
    centers[w], window_size))[0]``"""
    doy = np.asarray(doy)
    members = [np.where(window_mask(doy, d0, window_size))[0]
               for d0 in centers]
    ptr = np.concatenate([[0], np.cumsum([len(m) for m in members])])
    member = np.concatenate(members) if members else np.zeros(0)
    return ptr.astype(np.int32), member.astype(np.int32)


def last_window(n_steps, win_ptr, member):
    """per step the last window that holds it (-1: none): presrat.py:298-333
    writes the windows in order, a later one over an earlier one"""
    out = np.full(n_steps, -1, np.int32)
    for w in range(len(win_ptr) - 1):
        out[member[win_ptr[w]:win_ptr[w + 1]]] = w
    return out


def day_plan(entries, reduce):
    """base.py:730 per entry of ``base_data``: ``(plans, base_ti)`` with
    ``plans[i] = (day_ptr, step_idx, day_offset)`` — the steps of each of the
    entry's days (CSR, in the order of the sorted dates) and the rank of its
    first day among all days — and ``base_ti`` the time index of the reduced
    series.  Without a reduction every step is its own "day"."""
    import pandas as pd
    tis = [_time_index(ti) for _, ti in entries]
    if not reduce:
        plans, off = [], 0
        for ti in tis:
            n = len(ti)
            plans.append((np.arange(n + 1, dtype=np.int32),
                          np.arange(n, dtype=np.int32), off))
            off += n
        return plans, pd.DatetimeIndex(np.hstack([ti.values for ti in tis]))
    days = [ti.normalize().values for ti in tis]
    all_days = np.unique(np.concatenate(days))
    plans = []
    seen = np.zeros(len(all_days), bool)
    for d in days:
        rank = np.searchsorted(all_days, d)
        own = np.unique(rank)
        if seen[own].any():
            raise ValueError('a day spans two entries of base_data: every '
                             'day must lie in one of them')
        seen[own] = True
        if own[-1] - own[0] + 1 != len(own):
            raise ValueError('the days of the entries of base_data '
                             'interleave')
        order = np.argsort(rank, kind='stable').astype(np.int32)
        counts = np.bincount(rank - own[0], minlength=len(own))
        ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        plans.append((ptr, order, int(own[0])))
    return plans, pd.DatetimeIndex(all_days)


def fill_and_smooth(out, fill_extend=True, smooth_extend=0,
                    smooth_interior=0):
    """mixins.py:19-102 with ``nn_fill_array`` (utilities.py:55-75), on the
    host with the reference's own scipy calls"""
    from scipy import ndimage as nd

    def nn_fill_array(array):
        nan_mask = np.isnan(array)
        indices = nd.distance_transform_edt(
            nan_mask, return_distances=False, return_indices=True)
        return array[tuple(indices)]

    for key, arr in out.items():
        nan_mask = np.isnan(arr[..., 0])
        for idt in range(arr.shape[-1]):
            arr_smooth = arr[..., idt]
            needs_fill = (np.isnan(arr_smooth).any()
                          and fill_extend) or smooth_interior > 0
            if needs_fill:
                arr_smooth = nn_fill_array(arr_smooth)
            arr_smooth_int = arr_smooth_ext = arr_smooth
            if smooth_extend > 0:
                arr_smooth_ext = nd.gaussian_filter(
                    arr_smooth_ext, smooth_extend, mode='nearest')
            if smooth_interior > 0:
                arr_smooth_int = nd.gaussian_filter(
                    arr_smooth_int, smooth_interior, mode='nearest')
            out[key][nan_mask, idt] = arr_smooth_ext[nan_mask]
            out[key][~nan_mask, idt] = arr_smooth_int[~nan_mask]
    return out


# ----------------------------------------- the KS test from integer counts
KS_MAX_AUTO_N = 10000      # scipy's ks_2samp(method='auto'): exact up to here


def ks_pvalue(n1, n2, h, d):
    """``ks_2samp(method='auto', alternative='two-sided')`` from where it has
    its statistic: ``h`` the integer numerator of ``d = h / (n1 n2)`` and
    ``d`` the float64 statistic.  Returns ``(statistic, pvalue)`` — the exact
    route re-derives the statistic from ``h`` as scipy does."""
    import math
    import warnings
    from scipy import stats
    if max(n1, n2) <= KS_MAX_AUTO_N:
        try:
            from scipy.stats._stats_py import _attempt_exact_2kssamp
        except ImportError:                               # a private routine
            _attempt_exact_2kssamp = None
        success = False
        if _attempt_exact_2kssamp is not None:
            success, d, prob = _attempt_exact_2kssamp(
                n1, n2, math.gcd(n1, n2), h / (n1 * n2), 'two-sided')
        if success:
            return np.float64(d), np.clip(prob, 0, 1)
        warnings.warn('ks_2samp: Exact calculation unsuccessful. Switching '
                      'to method=asymp.', RuntimeWarning, stacklevel=2)
    m, n = sorted([float(n1), float(n2)], reverse=True)
    prob = stats.distributions.kstwo.sf(d, np.round(m * n / (m + n)))
    return np.float64(d), np.clip(prob, 0, 1)


def ks_from_counts(n1, n2, counts, memo=None):
    """statistic and p-value of every pixel from the kernel's counts ``(P, 4)``:
    ``(c1, c2)`` at the largest and at the smallest ``c1 n2 - c2 n1``.  The
    side is chosen on the integers; the statistic is scipy's float64 ``c1 / n1
    - c2 / n2``.  ``memo`` (a dict) shares the p-value among the pixels with
    one numerator and statistic.  Rows of ``BCC_SK_NO_KS`` give NaN."""
    counts = np.asarray(counts, np.int64)
    memo = {} if memo is None else memo
    stat = np.full(len(counts), np.nan)
    pval = np.full(len(counts), np.nan)
    for i, (c1p, c2p, c1m, c2m) in enumerate(counts.tolist()):
        if c1p == _lib.BCC_SK_NO_KS:
            continue
        up, down = c1p * n2 - c2p * n1, c2m * n1 - c1m * n2
        if down > up:
            h, d = down, np.clip(-(c1m / n1 - c2m / n2), 0, 1)
        else:
            h, d = max(up, 0), c1p / n1 - c2p / n2
        key = (n1, n2, h, float(d))
        if key not in memo:
            memo[key] = ks_pvalue(n1, n2, h, d)
        stat[i], pval[i] = memo[key]
    return stat, pval


# ------------------------------------------------------------ device backend
def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


class DeviceBackend:
    """The six kernels behind numpy-in / tensor-out methods.  Series stay on
    the device between the calls; index lists go up as int32."""

    def __init__(self, dev=None):
        from .engine import Device
        self.dev = dev or Device.get()

    # -- plumbing
    def _call(self, name, *args):
        ctx = self.dev.ctx
        rc = getattr(_lib.lib(), name)(ctx, *args)
        if rc == -1:                                      # S3_EINVAL
            raise ValueError(f'{name}: {_lib.last_error(ctx)}')
        _lib.check(rc, ctx, name)

    def _ints(self, a):
        import torch
        return torch.from_numpy(_i32(a)).to(self.dev.torch_device)

    def _new(self, shape, dtype=None, fill=None):
        import torch
        dtype = dtype or torch.float32
        if fill is None:
            return torch.empty(shape, dtype=dtype,
                               device=self.dev.torch_device)
        return torch.full(shape, fill, dtype=dtype,
                          device=self.dev.torch_device)

    def upload(self, a):
        """fp32 ``(P, T)`` host series -> device"""
        return self.dev.to_device(np.ascontiguousarray(a, np.float32))

    def to_host(self, t):
        return t.cpu().numpy()

    @staticmethod
    def _p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    # -- kernels
    def base_series(self, entries, site_ptr, site_idx, plans, n_days_total,
                    reduction, flags=0, decimals=0):
        """``entries``: ``(base (T, n_sites), cs_ghi | None)`` per launch;
        ``plans``: ``(day_ptr, step_idx, day_offset)`` per launch ->
        ``(P, n_days_total)``"""
        site_ptr, site_idx = _i32(site_ptr), _i32(site_idx)
        n_pix = len(site_ptr) - 1
        d_ptr, d_idx = self._ints(site_ptr), self._ints(
            site_idx if len(site_idx) else [0])
        if not len(site_idx):
            site_idx = np.zeros(1, np.int32)
        out = self._new((n_pix, int(n_days_total)), fill=float('nan'))
        keep = []
        for (base, cs), (day_ptr, step_idx, off) in zip(entries, plans):
            base = np.ascontiguousarray(base, np.float32)
            n_t, n_sites = base.shape
            x = self.dev.to_device(base)
            c = None if cs is None else self.dev.to_device(
                np.ascontiguousarray(cs, np.float32))
            day_ptr, step_idx = _i32(day_ptr), _i32(step_idx)
            g_ptr, g_idx = self._ints(day_ptr), self._ints(step_idx)
            keep.append((x, c, g_ptr, g_idx))
            self._call('s3_bc_base_series', self._p(x), self._p(c), n_t,
                       n_sites, n_pix, _hp(site_ptr), _hp(site_idx),
                       self._p(d_ptr), self._p(d_idx), len(day_ptr) - 1,
                       _hp(day_ptr), _hp(step_idx), self._p(g_ptr),
                       self._p(g_idx), int(reduction), int(flags),
                       int(decimals), int(n_days_total), int(off),
                       self._p(out))
        self.dev.sync()
        return out

    def moments(self, series, group, n_groups):
        """``(count int32, mean, std)`` host arrays ``(P, n_groups)``"""
        import torch
        group = _i32(group)
        n_pix, n_t = (int(v) for v in series.shape)
        g = self._ints(group)
        cnt = self._new((n_pix, n_groups), torch.int32, 0)
        mean = self._new((n_pix, n_groups), fill=float('nan'))
        std = self._new((n_pix, n_groups), fill=float('nan'))
        self._call('s3_bc_moments', self._p(series), n_pix, n_t, _hp(group),
                   self._p(g), int(n_groups), self._p(cnt), self._p(mean),
                   self._p(std))
        return self.to_host(cnt), self.to_host(mean), self.to_host(std)

    def window_quantiles(self, series, win_ptr, member, n_q):
        """device ``(P, W, n_q)``"""
        win_ptr, member = _i32(win_ptr), _i32(member)
        if not len(member):
            member = np.zeros(1, np.int32)
        n_pix, n_t = (int(v) for v in series.shape)
        n_w = len(win_ptr) - 1
        out = self._new((n_pix, n_w, int(n_q)), fill=float('nan'))
        d_ptr, d_mem = self._ints(win_ptr), self._ints(member)
        self._call('s3_bc_window_quantiles', self._p(series), n_pix, n_t,
                   n_w, _hp(win_ptr), _hp(member), self._p(d_ptr),
                   self._p(d_mem), int(n_q), self._p(out))
        self.dev.sync()
        return out

    def match_zero_rate(self, base_series, bias_series):
        """in place on ``bias_series``; returns ``(bias_series, min_value
        (P) float64 on the host, number of non-finite bias values)``"""
        import torch
        n_pix, n_t = (int(v) for v in bias_series.shape)
        mv = self._new((n_pix,), torch.float64, float('nan'))
        bad = self._new((1,), torch.int32, 0)
        self._call('s3_bc_match_zero_rate', self._p(base_series),
                   int(base_series.shape[1]), self._p(bias_series), n_pix,
                   n_t, self._p(mv), self._p(bad))
        return bias_series, self.to_host(mv), int(self.to_host(bad)[0])

    def skill(self, base_series, bias_series, demean):
        """host ``dict(stats (P, 2, BCC_SK_STATS) float32 — base, bias —, ks
        (P, 4) int32, status (P, 4) int32)``"""
        import torch
        n_pix, n_d = (int(v) for v in base_series.shape)
        n_t = int(bias_series.shape[1])
        if int(bias_series.shape[0]) != n_pix:
            raise ValueError('base and bias series of different pixel counts')
        work = self._new((n_pix, max(n_d, 1)), torch.int32)
        stats = self._new((n_pix, 2, _lib.BCC_SK_STATS), fill=float('nan'))
        ks = self._new((n_pix, _lib.BCC_SK_KS_WORDS), torch.int32,
                       _lib.BCC_SK_NO_KS)
        status = self._new((n_pix, _lib.BCC_SK_STATUS_WORDS), torch.int32, 0)
        self._call('s3_bc_skill', self._p(base_series), n_d,
                   self._p(bias_series), n_t, n_pix, int(bool(demean)),
                   self._p(work), self._p(stats), self._p(ks),
                   self._p(status))
        return {'stats': self.to_host(stats), 'ks': self.to_host(ks),
                'status': self.to_host(status)}

    def mask_windows(self, tables, bad_windows):
        """NaN rows for the windows in ``bad_windows`` (host bool ``(W,)``)"""
        import torch
        if np.any(bad_windows):
            idx = torch.from_numpy(np.where(bad_windows)[0]).to(
                self.dev.torch_device)
            for t in tables:
                t[:, idx, :] = float('nan')

    def presrat(self, base, bias, fut, tables, relative, threshold,
                last_win, lists):
        """``tables``: device base / bias / fut params ``(P, W, Q)``;
        ``lists``: ``(win_ptr, member)`` of base, bias, fut.  Returns host
        ``dict(corrected, zero_rate, tau, z_fg, tau_fut, k_factor, status)``"""
        import torch
        n_pix, n_w, n_q = (int(v) for v in tables[0].shape)
        last_win = _i32(last_win)
        d_last = self._ints(last_win)
        host = [(_i32(p), _i32(m if len(m) else [0])) for p, m in lists]
        devl = [(self._ints(p), self._ints(m)) for p, m in host]
        vp3 = C.c_void_p * 3
        hp = vp3(*[p.ctypes.data for p, _ in host])
        hm = vp3(*[m.ctypes.data for _, m in host])
        dp = vp3(*[p.data_ptr() for p, _ in devl])
        dm = vp3(*[m.data_ptr() for _, m in devl])
        res = {'corrected': self._new(tuple(fut.shape), fill=float('nan'))}
        for k in ('zero_rate', 'tau', 'z_fg', 'tau_fut'):
            res[k] = self._new((n_pix,), fill=float('nan'))
        res['k_factor'] = self._new((n_pix, n_w), fill=float('nan'))
        res['status'] = self._new((3,), torch.int32, 0)
        self._call('s3_bc_presrat', self._p(base), int(base.shape[1]),
                   self._p(bias), int(bias.shape[1]), self._p(fut),
                   int(fut.shape[1]), n_pix, n_w, n_q, self._p(tables[0]),
                   self._p(tables[1]), self._p(tables[2]), int(bool(relative)),
                   float(threshold), _hp(last_win), self._p(d_last), hp, hm,
                   dp, dm, *[self._p(res[k]) for k in (
                       'corrected', 'zero_rate', 'tau', 'z_fg', 'tau_fut',
                       'k_factor', 'status')])
        return {k: self.to_host(v) for k, v in res.items()}


# ------------------------------------------------------------------- classes
class _DataRetrievalBase:
    """``DataRetrievalBase`` (base.py:31-190) over arrays: the planning that
    every calculator shares."""

    def __init__(self, base_data, bias_data, base_dset, bias_feature, *,
                 base_lat_lon, bias_lat_lon, bias_time_index,
                 base_cs_ghi=None, distance_upper_bound=None, decimals=None,
                 match_zero_rate=False, backend=None):
        self.base_dset = base_dset
        self.bias_feature = bias_feature
        self.decimals = decimals
        self.match_zero_rate = match_zero_rate
        self.backend = backend
        self.bad_bias_gids = []
        self.bias_data = np.asarray(bias_data)
        self.bias_lat_lon = np.asarray(bias_lat_lon)
        self.bias_ti = _time_index(bias_time_index)
        if self.bias_data.ndim != 3 or self.bias_lat_lon.shape != (
                *self.bias_data.shape[:2], 2):
            raise ValueError(
                'bias_data (S1, S2, Tb) with bias_lat_lon (S1, S2, 2) '
                f'expected, got {self.bias_data.shape} and '
                f'{self.bias_lat_lon.shape}')
        if len(self.bias_ti) != self.bias_data.shape[-1]:
            raise ValueError(
                f'{len(self.bias_ti)} bias time steps for bias_data '
                f'{self.bias_data.shape}')
        self.raster_shape = self.bias_data.shape[:2]
        self.n_pix = int(np.prod(self.raster_shape))
        self.bias_gid_raster = np.arange(self.n_pix).reshape(
            self.raster_shape)

        if isinstance(base_data, tuple) and len(base_data) == 2 and \
                hasattr(base_data[0], 'shape'):
            base_data = [base_data]
        self.base_lat_lon = np.asarray(base_lat_lon)
        self.base_is_raster = self.base_lat_lon.ndim == 3
        cs = base_cs_ghi
        if cs is not None and hasattr(cs, 'shape'):
            cs = [cs]
        if cs is not None and len(cs) != len(base_data):
            raise ValueError('one base_cs_ghi array per entry of base_data')
        self.base_entries = []
        for i, (arr, ti) in enumerate(base_data):
            arr = self._site_major(arr)
            if len(ti) != arr.shape[0]:
                raise ValueError(f'{len(ti)} base time steps for a base '
                                 f'array of {arr.shape[0]} steps')
            c = None if cs is None else self._site_major(cs[i])
            if c is not None and c.shape != arr.shape:
                raise ValueError('base_cs_ghi must have the shape of its '
                                 'base array')
            self.base_entries.append((arr, ti, c))
        (self.site_ptr, self.site_idx, self.nn_ind,
         self.distance_upper_bound) = site_mapping(
            self.bias_lat_lon, self.base_lat_lon, distance_upper_bound)
        self.bad_bias_gids = list(np.where(np.diff(self.site_ptr) == 0)[0])
        self.out = None
        self._init_out()

    def _site_major(self, arr):
        """``(T, n_sites)`` as it is, ``(R1, R2, T)`` -> ``(T, R1 * R2)``"""
        arr = np.asarray(arr)
        n_sites = int(np.prod(self.base_lat_lon.shape[:-1]))
        if self.base_is_raster:
            if arr.ndim != 3 or arr.shape[:2] != self.base_lat_lon.shape[:2]:
                raise ValueError(
                    f'base array {arr.shape} for base_lat_lon '
                    f'{self.base_lat_lon.shape}')
            return np.ascontiguousarray(arr.reshape(n_sites, -1).T)
        if arr.ndim != 2 or arr.shape[1] != n_sites:
            raise ValueError(f'base array {arr.shape} for base_lat_lon '
                             f'{self.base_lat_lon.shape}')
        return arr

    @property
    def _backend(self):
        if self.backend is None:
            self.backend = DeviceBackend()
        return self.backend

    # -- the two series of every calculator
    def _base_series(self, daily_reduction):
        """(device series ``(P, D)``, its time index)"""
        name = 'none' if daily_reduction is None else str(
            daily_reduction).lower()
        if name not in REDUCTIONS:
            raise ValueError(f'daily_reduction "{daily_reduction}": one of '
                             f'{sorted(REDUCTIONS)} or None')
        red = REDUCTIONS[name]
        plans, base_ti = day_plan(
            [(a, ti) for a, ti, _ in self.base_entries],
            reduce=red != _lib.BCC_NONE)
        flags = 0 if self.base_is_raster else _lib.BCC_NANSKIP
        cs_ratio = red == _lib.BCC_AVG and self.base_dset == 'clearsky_ratio'
        if cs_ratio:
            if any(c is None for _, _, c in self.base_entries):
                raise ValueError('base_dset "clearsky_ratio" needs '
                                 'base_cs_ghi')
            flags |= _lib.BCC_CS_RATIO
        if self.decimals is not None:
            flags |= _lib.BCC_ROUND
        series = self._backend.base_series(
            [(a, c if cs_ratio else None) for a, _, c in self.base_entries],
            self.site_ptr, self.site_idx, plans, len(base_ti), red, flags,
            self.decimals or 0)
        if cs_ratio:
            host = self._backend.to_host(series)
            good = np.diff(self.site_ptr) > 0
            msg = ('Could not calculate daily average "clearsky_ratio" with '
                   'input ghi and cs ghi inputs')
            assert not np.isnan(host[good]).any(), msg
        return series, base_ti

    def _bias_series(self, data):
        """``get_bias_data`` (base.py:408-450) of every pixel: ``(P, T)``"""
        flat = np.asarray(data, np.float32).reshape(self.n_pix, -1)
        if self.decimals is not None:
            flat = np.around(flat, decimals=self.decimals)
        return self._backend.upload(flat)

    def _check_sort(self, n):
        if n > _lib.BCC_MAX_SORT:
            raise ValueError(f'{n} values: {SORT_LIMIT}')

    def _good(self, table):
        """NaN for the bad pixels, reshaped to the raster"""
        table = np.array(table, np.float32)
        table[np.diff(self.site_ptr) == 0] = np.nan
        return table.reshape(*self.raster_shape, *table.shape[1:])

    def _write(self, fp_out, out, attrs=None):
        if fp_out is None:
            return
        if not str(fp_out).endswith('.npz'):
            raise ValueError(f'fp_out "{fp_out}" must end in .npz (h5py is '
                             'not used here)')
        np.savez(fp_out, latitude=self.bias_lat_lon[..., 0],
                 longitude=self.bias_lat_lon[..., 1], **out,
                 **{k: np.asarray(v) for k, v in (attrs or {}).items()})
        logger.info('Wrote bias correction factors to file: %s', fp_out)


class LinearCorrection(_DataRetrievalBase):
    """bias_calc.py:21-253: ``*scalar + adder`` from the means and stds of the
    whole series (``NT = 1``)."""

    NT = 1

    def _init_out(self):
        keys = [f'{self.bias_feature}_scalar', f'{self.bias_feature}_adder',
                f'bias_{self.bias_feature}_mean',
                f'bias_{self.bias_feature}_std',
                f'base_{self.base_dset}_mean', f'base_{self.base_dset}_std']
        self.out = {k: np.full((*self.raster_shape, self.NT), np.nan,
                               np.float32) for k in keys}

    @staticmethod
    def get_linear_correction(bias_mean, bias_std, base_mean, base_std,
                              bias_feature, base_dset):
        """bias_calc.py:76-90 on float32 arrays of means and stds"""
        with np.errstate(divide='ignore', invalid='ignore'):
            bias_std = np.where(bias_std == 0, base_std, bias_std)
            scalar = base_std / bias_std
            adder = base_mean - bias_mean * scalar
        return {f'bias_{bias_feature}_mean': bias_mean,
                f'bias_{bias_feature}_std': bias_std,
                f'base_{base_dset}_mean': base_mean,
                f'base_{base_dset}_std': base_std,
                f'{bias_feature}_scalar': scalar,
                f'{bias_feature}_adder': adder}

    def _groups(self, bias_ti, base_ti):
        """group id per step of the two series, and the groups both have"""
        if self.NT == 1:
            return (np.zeros(len(bias_ti), np.int32),
                    np.zeros(len(base_ti), np.int32), np.ones(1, bool))
        g_bias = np.asarray(bias_ti.month, np.int32) - 1
        g_base = np.asarray(base_ti.month, np.int32) - 1
        both = np.isin(np.arange(12), g_bias) & np.isin(np.arange(12), g_base)
        return g_bias, g_base, both

    def run(self, fp_out=None, max_workers=None, daily_reduction='avg',
            fill_extend=True, smooth_extend=0, smooth_interior=0):
        """bias_calc.py:191-253; ``max_workers`` is accepted and ignored"""
        be = self._backend
        self._init_out()
        base, base_ti = self._base_series(daily_reduction)
        bias = self._bias_series(self.bias_data)
        if self.match_zero_rate:
            self._check_sort(len(self.bias_ti))
            bias, _, bad = be.match_zero_rate(base, bias)
            if bad:
                raise ValueError(f'match_zero_rate: {bad} non-finite values '
                                 'in bias_data')
        g_bias, g_base, both = self._groups(self.bias_ti, base_ti)
        _, bias_mean, bias_std = be.moments(bias, g_bias, self.NT)
        _, base_mean, base_std = be.moments(base, g_base, self.NT)
        res = self.get_linear_correction(
            bias_mean, bias_std, base_mean, base_std, self.bias_feature,
            self.base_dset)
        for k, v in res.items():
            v = np.array(v, np.float32)
            v[:, ~both] = np.nan             # bias_calc.py:358: both or none
            self.out[k] = self._good(v)
        self.out = fill_and_smooth(self.out, fill_extend, smooth_extend,
                                   smooth_interior)
        self._write(fp_out, self.out)
        return copy.deepcopy(self.out)


class ScalarCorrection(LinearCorrection):
    """bias_calc.py:256-308: ``scalar = mean(base) / mean(bias)``, adder 0; the
    two std tables of ``_init_out`` are never written and stay NaN"""

    @staticmethod
    def get_linear_correction(bias_mean, bias_std, base_mean, base_std,
                              bias_feature, base_dset):
        with np.errstate(divide='ignore', invalid='ignore'):
            scalar = base_mean / bias_mean
        return {f'bias_{bias_feature}_mean': bias_mean,
                f'base_{base_dset}_mean': base_mean,
                f'{bias_feature}_scalar': scalar,
                f'{bias_feature}_adder': np.zeros(scalar.shape, np.float32)}


class MonthlyLinearCorrection(LinearCorrection):
    """bias_calc.py:311-370: one scalar and adder per month"""

    NT = 12


class MonthlyScalarCorrection(MonthlyLinearCorrection, ScalarCorrection):
    """bias_calc.py:373-376"""

    NT = 12


class SkillAssessment(MonthlyLinearCorrection):
    """bias_calc.py:379-544: the historical skill of one dataset against
    another — monthly means and stds, and over the whole series the moments,
    zero rate, seven percentiles and the two-sample KS test of the
    mean-removed distributions (of the series as they are under
    ``match_zero_rate``).  As in the reference the ``_scalar`` / ``_adder``
    tables are created and never written (bias_calc.py:539-542)."""

    PERCENTILES = (1, 5, 25, 50, 75, 95, 99)

    def _init_out(self):
        feat, dset = self.bias_feature, self.base_dset
        monthly_keys = [f'{feat}_scalar', f'{feat}_adder',
                        f'bias_{feat}_mean_monthly',
                        f'bias_{feat}_std_monthly',
                        f'base_{dset}_mean_monthly',
                        f'base_{dset}_std_monthly']
        annual_keys = [f'{feat}_ks_stat', f'{feat}_ks_p', f'{feat}_bias',
                       f'bias_{feat}_mean', f'bias_{feat}_std',
                       f'bias_{feat}_skew', f'bias_{feat}_kurtosis',
                       f'bias_{feat}_zero_rate', f'base_{dset}_mean',
                       f'base_{dset}_std', f'base_{dset}_skew',
                       f'base_{dset}_kurtosis', f'base_{dset}_zero_rate']
        self.out = {k: np.full((*self.raster_shape, self.NT), np.nan,
                               np.float32) for k in monthly_keys}
        for k in annual_keys:
            self.out[k] = np.full((*self.raster_shape, 1), np.nan, np.float32)
        for p in self.PERCENTILES:
            for k in (f'base_{dset}_percentile_{p}',
                      f'bias_{feat}_percentile_{p}'):
                self.out[k] = np.full((*self.raster_shape, 1), np.nan,
                                      np.float32)

    def run(self, fp_out=None, max_workers=None, daily_reduction='avg',
            fill_extend=True, smooth_extend=0, smooth_interior=0):
        """bias_calc.py:191-253 over ``_run_single`` (:483-544);
        ``max_workers`` is accepted and ignored.  ``ks_seconds`` holds the
        host time spent on the p-values."""
        import time
        be = self._backend
        feat, dset = self.bias_feature, self.base_dset
        self._init_out()
        self._check_sort(len(self.bias_ti))
        base, base_ti = self._base_series(daily_reduction)
        self._check_sort(len(base_ti))
        bias = self._bias_series(self.bias_data)
        if self.match_zero_rate:
            bias, _, bad = be.match_zero_rate(base, bias)
            if bad:
                raise ValueError(f'match_zero_rate: {bad} non-finite values '
                                 'in bias_data')
        g_bias, g_base, both = self._groups(self.bias_ti, base_ti)
        _, bias_mean, bias_std = be.moments(bias, g_bias, self.NT)
        _, base_mean, base_std = be.moments(base, g_base, self.NT)
        res = self.get_linear_correction(bias_mean, bias_std, base_mean,
                                         base_std, feat, dset)
        for k, v in res.items():
            if k.endswith(('_scalar', '_adder')):
                continue
            v = np.array(v, np.float32)
            v[:, ~both] = np.nan             # bias_calc.py:532: both or none
            self.out[k + '_monthly'] = self._good(v)
        res = be.skill(base, bias, demean=not self.match_zero_rate)
        good = np.diff(self.site_ptr) > 0
        tic = time.perf_counter()
        stat = np.full(self.n_pix, np.nan)
        pval = np.full(self.n_pix, np.nan)
        stat[good], pval[good] = ks_from_counts(
            len(base_ti), len(self.bias_ti), res['ks'][good])
        self.ks_seconds = time.perf_counter() - tic
        st = res['stats']
        tables = {f'{feat}_ks_stat': stat, f'{feat}_ks_p': pval,
                  f'{feat}_bias': st[:, 1, _lib.BCC_SK_BIAS]}
        for s, name in ((0, f'base_{dset}'), (1, f'bias_{feat}')):
            for j, k in ((_lib.BCC_SK_MEAN, 'mean'), (_lib.BCC_SK_STD, 'std'),
                         (_lib.BCC_SK_SKEW, 'skew'),
                         (_lib.BCC_SK_KURTOSIS, 'kurtosis'),
                         (_lib.BCC_SK_ZERO_RATE, 'zero_rate')):
                tables[f'{name}_{k}'] = st[:, s, j]
            for j, p in enumerate(self.PERCENTILES):
                tables[f'{name}_percentile_{p}'] = st[:, s,
                                                      _lib.BCC_SK_PCT0 + j]
        for k, v in tables.items():
            self.out[k] = self._good(np.asarray(v)[:, None])
        self.out = fill_and_smooth(self.out, fill_extend, smooth_extend,
                                   smooth_interior)
        self._write(fp_out, self.out)
        return copy.deepcopy(self.out)


class QuantileDeltaMappingCorrection(_DataRetrievalBase):
    """qdm.py:35-623: the quantiles of the three series per day-of-year
    window."""

    def __init__(self, base_data, bias_data, bias_fut_data, base_dset,
                 bias_feature, *, base_lat_lon, bias_lat_lon,
                 bias_time_index, bias_fut_time_index, base_cs_ghi=None,
                 distance_upper_bound=None, decimals=None,
                 match_zero_rate=False, n_quantiles=101, dist='empirical',
                 relative=True, sampling='linear', log_base=10,
                 n_time_steps=24, window_size=120, backend=None):
        if dist != 'empirical':
            raise KeyError(f'dist "{dist}": only "empirical" is computed '
                           'here')
        if sampling != 'linear':
            msg = ('sampling option must be linear here (log and invlog '
                   f'are defined inside rex), but received: {sampling}')
            raise KeyError(msg)
        self.n_quantiles = int(n_quantiles)
        self.dist = dist
        self.relative = relative
        self.sampling = sampling
        self.log_base = log_base
        self.n_time_steps = int(n_time_steps)
        self.window_size = window_size
        self.time_window_center = window_center(self.n_time_steps)
        if len(self.time_window_center) != self.n_time_steps:
            raise ValueError(
                f'n_time_steps = {n_time_steps} gives '
                f'{len(self.time_window_center)} window centres (the '
                'reference indexes past its template there)')
        if self.n_quantiles < 1:
            raise ValueError('n_quantiles must be at least 1')
        super().__init__(
            base_data, bias_data, base_dset, bias_feature,
            base_lat_lon=base_lat_lon, bias_lat_lon=bias_lat_lon,
            bias_time_index=bias_time_index, base_cs_ghi=base_cs_ghi,
            distance_upper_bound=distance_upper_bound, decimals=decimals,
            match_zero_rate=match_zero_rate, backend=backend)
        self.bias_fut_data = np.asarray(bias_fut_data)
        self.bias_fut_ti = _time_index(bias_fut_time_index)
        if self.bias_fut_data.shape[:2] != self.raster_shape or \
                self.bias_fut_data.shape[-1] != len(self.bias_fut_ti):
            raise ValueError(
                f'bias_fut_data {self.bias_fut_data.shape} for a '
                f'{self.raster_shape} grid and {len(self.bias_fut_ti)} '
                'future time steps')

    def _init_out(self):
        keys = [f'bias_{self.bias_feature}_params',
                f'bias_fut_{self.bias_feature}_params',
                f'base_{self.base_dset}_params']
        shape = (*self.raster_shape, self.n_time_steps, self.n_quantiles)
        self.out = {k: np.full(shape, np.nan, np.float32) for k in keys}

    def _quantile_tables(self, daily_reduction):
        """qdm.py:334-373 for every pixel: the three device series, their
        window lists and the three device tables ``(P, W, Q)`` with the rows of
        a window that is empty in one series NaN in all (qdm.py:357)"""
        be = self._backend
        base, base_ti = self._base_series(daily_reduction)
        bias = self._bias_series(self.bias_data)
        fut = self._bias_series(self.bias_fut_data)
        size = self.window_size or 365 / self.n_time_steps
        lists = [window_members(ti.day_of_year, self.time_window_center, size)
                 for ti in (base_ti, self.bias_ti, self.bias_fut_ti)]
        for ptr, _ in lists:
            self._check_sort(int(np.diff(ptr).max()))
        tables = [be.window_quantiles(s, ptr, mem, self.n_quantiles)
                  for s, (ptr, mem) in zip((base, bias, fut), lists)]
        empty = np.zeros(self.n_time_steps, bool)
        for ptr, _ in lists:
            empty |= np.diff(ptr) == 0
        be.mask_windows(tables, empty)
        return (base, bias, fut), lists, tables

    def _attrs(self):
        return {'dist': self.dist, 'sampling': self.sampling,
                'log_base': self.log_base,
                'time_window_center': self.time_window_center}

    def _store_tables(self, tables):
        be = self._backend
        for key, t in zip((f'base_{self.base_dset}_params',
                           f'bias_{self.bias_feature}_params',
                           f'bias_fut_{self.bias_feature}_params'), tables):
            self.out[key] = self._good(be.to_host(t))

    def run(self, fp_out=None, max_workers=None, daily_reduction='avg',
            fill_extend=True, smooth_extend=0, smooth_interior=0):
        """qdm.py:530-580; ``max_workers`` is accepted and ignored"""
        self._init_out()
        _, _, tables = self._quantile_tables(daily_reduction)
        self._store_tables(tables)
        self.out = fill_and_smooth(self.out, fill_extend, smooth_extend,
                                   smooth_interior)
        self._write(fp_out, self.out, self._attrs())
        return copy.deepcopy(self.out)


class PresRat(QuantileDeltaMappingCorrection):
    """presrat.py:42-494: QDM's tables plus the zero rate of the observations,
    ``tau_fut`` and the ``k_factor`` of every window."""

    def _init_out(self):
        super()._init_out()
        shape = (*self.raster_shape, 1)
        self.out[f'{self.base_dset}_zero_rate'] = np.full(
            shape, np.nan, np.float32)
        self.out[f'{self.bias_feature}_tau_fut'] = np.full(
            shape, np.nan, np.float32)
        shape = (*self.raster_shape, self.n_time_steps)
        self.out[f'{self.bias_feature}_k_factor'] = np.full(
            shape, np.nan, np.float32)

    def run(self, fp_out=None, max_workers=None, daily_reduction='avg',
            fill_extend=True, smooth_extend=0, smooth_interior=0,
            zero_rate_threshold=1.157e-7):
        """presrat.py:362-441; ``max_workers`` is accepted and ignored"""
        be = self._backend
        self._init_out()
        if self.n_quantiles < 2:
            raise ValueError('PresRat maps through its tables: n_quantiles '
                             'must be at least 2')
        self._check_sort(len(self.bias_ti))
        self._check_sort(len(self.bias_fut_ti))
        series, lists, tables = self._quantile_tables(daily_reduction)
        last = last_window(len(self.bias_fut_ti), *lists[2])
        res = be.presrat(*series, tables, self.relative, zero_rate_threshold,
                         last, lists)
        good = np.diff(self.site_ptr) > 0
        status = res['status']
        # presrat.py:146, 155
        assert not (status[_lib.BCC_PR_BIAS_NONFINITE]
                    or status[_lib.BCC_PR_FUT_NONFINITE]), \
            'Unexpected invalid values'
        if np.isnan(res['tau_fut'][good]).any() and \
                status[_lib.BCC_PR_INDEX]:
            raise IndexError('round(z_fg * size) lies past the corrected '
                             'series (every future value below tau)')
        self.corrected_fut_data = self._good(res['corrected'])
        self._store_tables(tables)
        self.out[f'{self.base_dset}_zero_rate'] = self._good(
            res['zero_rate'][:, None])
        self.out[f'{self.bias_feature}_tau_fut'] = self._good(
            res['tau_fut'][:, None])
        self.out[f'{self.bias_feature}_k_factor'] = self._good(
            res['k_factor'])
        self.out = fill_and_smooth(self.out, fill_extend, smooth_extend,
                                   smooth_interior)
        attrs = self._attrs()
        attrs['zero_rate_threshold'] = zero_rate_threshold
        self._write(fp_out, self.out, attrs)
        return copy.deepcopy(self.out)
