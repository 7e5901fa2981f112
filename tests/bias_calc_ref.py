"""The reference's bias calculators, followed line by line per pixel with the
same numpy / pandas / scipy calls (sup3r/bias/base.py, bias_calc.py, qdm.py,
presrat.py, mixins.py): ``get_base_data`` / ``_reduce_base_data`` /
``_match_zero_rate`` / ``get_linear_correction`` / ``get_qdm_params`` /
``calc_tau_fut`` / ``calc_k_factor`` / ``_run_single`` / ``fill_and_smooth``.
Arrays stand in for the files: ``base_entries`` is a list of ``(array (T,
n_sites), time_index, cs_ghi | None)``.

``run(kind, inputs, dtype)`` evaluates a whole calculator in ``dtype``: float32
(``R32``, the reference as it runs on float32 data) or float64 (``R64``, every
input cast first).  It is a Python loop over the pixels, deliberately.

``Backend`` answers the calls of ``sup3r_amd.bias_calc.DeviceBackend`` with
these functions, so that the classes can be tested without a device.

Not available here: ``rex``.  ``sample_q_linear(n)`` is ``np.linspace(0, 1,
n)`` and the quantile delta mapping is ``tests/bias_ref.py``'s restatement."""
import contextlib
import warnings

import numpy as np
import pandas as pd
from scipy import ndimage as nd
from scipy.spatial import KDTree

from tests import bias_ref


@contextlib.contextmanager
def quiet():
    """numpy's warnings about empty slices, NaN and division off"""
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        yield


LINEAR = ('LinearCorrection', 'ScalarCorrection', 'MonthlyLinearCorrection',
          'MonthlyScalarCorrection')


# ------------------------------------------------------------------ base.py
def distance_upper_bound(bias_lat_lon):
    """base.py:228-242"""
    diff = np.diff(bias_lat_lon.reshape(-1, 2), axis=0)
    return np.max(np.median(diff, axis=0))


def nn_query(bias_lat_lon, base_lat_lon, bound=None):
    """base.py:175-182"""
    if bound is None:
        bound = distance_upper_bound(bias_lat_lon)
    tree = KDTree(bias_lat_lon.reshape(-1, 2))
    return tree.query(base_lat_lon.reshape(-1, 2),
                      distance_upper_bound=bound)


def reduce_base_data(base_ti, base_data, base_cs_ghi, base_dset,
                     daily_reduction):
    """base.py:694-780"""
    if daily_reduction is None:
        return base_data, base_ti
    daily_ti = pd.DatetimeIndex(sorted(set(base_ti.date)))
    df = pd.DataFrame({'date': base_ti.date, 'base_data': base_data,
                       'base_cs_ghi': base_cs_ghi})
    cs_ratio = (daily_reduction.lower() in ('avg', 'average', 'mean')
                and base_dset == 'clearsky_ratio')
    if cs_ratio:
        daily_ghi = df.groupby('date').sum()['base_data'].values
        daily_cs_ghi = df.groupby('date').sum()['base_cs_ghi'].values
        daily_ghi[daily_cs_ghi == 0] = 0
        daily_cs_ghi[daily_cs_ghi == 0] = 1
        base_data = daily_ghi / daily_cs_ghi
        assert not np.isnan(base_data).any()
    elif daily_reduction.lower() in ('avg', 'average', 'mean'):
        base_data = df.groupby('date').mean()['base_data'].values
    elif daily_reduction.lower() in ('max', 'maximum'):
        base_data = df.groupby('date').max()['base_data'].values
    elif daily_reduction.lower() in ('min', 'minimum'):
        base_data = df.groupby('date').min()['base_data'].values
    elif daily_reduction.lower() in ('sum', 'total'):
        base_data = df.groupby('date').sum()['base_data'].values
    assert base_data.shape == daily_ti.shape
    return base_data, daily_ti


def get_base_data(base_entries, base_dset, base_gid, raster=False,
                  daily_reduction='avg', decimals=None):
    """base.py:453-554 with _read_base_rex_data (:634-691, ``raster=False``:
    np.nanmean over the sites) or _read_base_sup3r_data (:602-631, a plain
    mean, the cs_ghi all NaN)"""
    out_data, out_ti, all_cs_ghi = [], [], []
    for arr, ti, cs in base_entries:
        base_data = arr[:, base_gid]
        if raster:
            base_data = base_data.T.mean(axis=0)
            base_cs_ghi = None if cs is None else cs[:, base_gid].T.mean(
                axis=0)
        else:
            base_data = np.nanmean(base_data, axis=1)
            base_cs_ghi = None if cs is None else np.nanmean(
                cs[:, base_gid], axis=1)
        if base_cs_ghi is None:
            base_cs_ghi = np.ones(len(base_data), dtype=np.float32) * np.nan
        out_data.append(base_data)
        out_ti.append(ti)
        all_cs_ghi.append(base_cs_ghi)
    out_data = np.hstack(out_data)
    out_ti = pd.DatetimeIndex(np.hstack(out_ti))
    all_cs_ghi = np.hstack(all_cs_ghi)
    if daily_reduction is not None:
        out_data, out_ti = reduce_base_data(out_ti, out_data, all_cs_ghi,
                                            base_dset, daily_reduction)
    if decimals is not None:
        out_data = np.around(out_data, decimals=decimals)
    return np.asarray(out_data), out_ti


def match_zero_rate(bias_data, base_data):
    """base.py:557-599; returns the threshold as well"""
    q_zero_base_in = np.nanmean(base_data == 0)
    q_bias = np.linspace(0, 1, len(bias_data))
    min_value_bias = np.interp(q_zero_base_in, q_bias, sorted(bias_data))
    bias_data[bias_data < min_value_bias] = 0
    return bias_data, min_value_bias


# ------------------------------------------------------------- bias_calc.py
def get_linear_correction(bias_data, base_data, bias_feature, base_dset):
    """bias_calc.py:51-92"""
    bias_std = np.nanstd(bias_data)
    if bias_std == 0:
        bias_std = np.nanstd(base_data)
    scalar = np.nanstd(base_data) / bias_std
    adder = np.nanmean(base_data) - np.nanmean(bias_data) * scalar
    return {f'bias_{bias_feature}_mean': np.nanmean(bias_data),
            f'bias_{bias_feature}_std': bias_std,
            f'base_{base_dset}_mean': np.nanmean(base_data),
            f'base_{base_dset}_std': np.nanstd(base_data),
            f'{bias_feature}_scalar': scalar,
            f'{bias_feature}_adder': adder}


def get_scalar_correction(bias_data, base_data, bias_feature, base_dset):
    """bias_calc.py:266-308"""
    base_mean = np.nanmean(base_data)
    bias_mean = np.nanmean(bias_data)
    scalar = base_mean / bias_mean
    adder = np.zeros(scalar.shape)
    return {f'bias_{bias_feature}_mean': bias_mean,
            f'base_{base_dset}_mean': base_mean,
            f'{bias_feature}_scalar': scalar,
            f'{bias_feature}_adder': adder}


def run_single_linear(kind, bias_data, base_data, base_ti, bias_ti,
                      bias_feature, base_dset, mzr=False, store=np.float32):
    """bias_calc.py:95-129 (NT = 1) / :320-370 (NT = 12), behind
    ``get_base_data``"""
    fn = get_scalar_correction if 'Scalar' in kind else get_linear_correction
    if mzr:
        bias_data, _ = match_zero_rate(bias_data, base_data)
    if not kind.startswith('Monthly'):
        return fn(bias_data, base_data, bias_feature, base_dset)
    base_arr = np.full(12, np.nan, dtype=store)
    out = {}
    for month in range(1, 13):
        bias_mask = bias_ti.month == month
        base_mask = base_ti.month == month
        if any(bias_mask) and any(base_mask):
            mout = fn(bias_data[bias_mask], base_data[base_mask],
                      bias_feature, base_dset)
            for k, v in mout.items():
                if k not in out:
                    out[k] = base_arr.copy()
                out[k][month - 1] = v
    return out


# ------------------------------------------------------------------- qdm.py
def window_center(ntimes):
    """qdm.py:302-305"""
    dt = 365 / ntimes
    return np.arange(dt / 2, 366, dt)


def window_mask(doy, d0, window_size):
    """qdm.py:613-623"""
    d_start = d0 - window_size / 2
    d_end = d0 + window_size / 2
    if d_start < 0:
        idx = (doy > 365 + d_start) | (doy < d_end)
    elif d_end > 365:
        idx = (doy > d_start) | (doy < d_end - 365)
    else:
        idx = (doy > d_start) & (doy < d_end)
    return idx


def get_qdm_params(bias_data, bias_fut_data, base_data, bias_feature,
                   base_dset, n_samples):
    """qdm.py:433-455, sampling == 'linear'"""
    quantiles = np.linspace(0, 1, n_samples)
    return {f'bias_{bias_feature}_params': np.quantile(bias_data, quantiles),
            f'bias_fut_{bias_feature}_params': np.quantile(bias_fut_data,
                                                           quantiles),
            f'base_{base_dset}_params': np.quantile(base_data, quantiles)}


def run_single_qdm(bias_data, bias_fut_data, base_data, base_ti, bias_ti,
                   bias_fut_ti, bias_feature, base_dset, n_samples,
                   n_time_steps, window_size, store=np.float32):
    """qdm.py:334-373"""
    window_size = window_size or 365 / n_time_steps
    centers = window_center(n_time_steps)
    template = np.full((n_time_steps, n_samples), np.nan, store)
    out = {}
    for nt, idt in enumerate(centers):
        base_idx = window_mask(base_ti.day_of_year, idt, window_size)
        bias_idx = window_mask(bias_ti.day_of_year, idt, window_size)
        bias_fut_idx = window_mask(bias_fut_ti.day_of_year, idt, window_size)
        if any(base_idx) and any(bias_idx) and any(bias_fut_idx):
            tmp = get_qdm_params(bias_data[bias_idx],
                                 bias_fut_data[bias_fut_idx],
                                 base_data[base_idx], bias_feature, base_dset,
                                 n_samples)
            for k, v in tmp.items():
                if k not in out:
                    out[k] = template.copy()
                out[k][(nt), :] = v
    return out


# --------------------------------------------------------------- presrat.py
def zero_precipitation_rate(arr, threshold=0.0):
    """mixins.py:159-161"""
    idx = np.isfinite(arr)
    return np.mean((arr[idx] <= threshold).astype('i'))


def calc_tau_fut(base_data, bias_data, bias_fut_data, corrected_fut_data,
                 zero_rate_threshold=1.157e-7):
    """presrat.py:138-163; returns tau and z_fg as well"""
    obs_zero_rate = zero_precipitation_rate(base_data, zero_rate_threshold)
    assert np.isfinite(bias_data).all(), 'Unexpected invalid values'
    n_threshold = round(obs_zero_rate * bias_data.size)
    n_threshold = min(n_threshold, bias_data.size - 1)
    tau = np.sort(bias_data)[n_threshold]
    assert np.isfinite(bias_fut_data).all(), 'Unexpected invalid values'
    z_fg = (bias_fut_data < tau).astype('i').sum() / bias_fut_data.size
    tau_fut = np.sort(corrected_fut_data)[
        round(z_fg * corrected_fut_data.size)]
    return tau_fut, obs_zero_rate, tau, z_fg


def calc_k_factor(base_data, bias_data, bias_fut_data, corrected_fut_data,
                  base_ti, bias_ti, bias_fut_ti, centers, window_size,
                  n_time_steps, zero_rate_threshold, store=np.float32):
    """presrat.py:228-249"""
    k = np.full(n_time_steps, np.nan, store)
    for nt, t in enumerate(centers):
        base_idt = window_mask(base_ti.day_of_year, t, window_size)
        bias_idt = window_mask(bias_ti.day_of_year, t, window_size)
        bias_fut_idt = window_mask(bias_fut_ti.day_of_year, t, window_size)
        with quiet():
            oh = base_data[base_idt].mean()
            mh = bias_data[bias_idt].mean()
            mf = bias_fut_data[bias_fut_idt].mean()
            mf_unbiased = corrected_fut_data[bias_fut_idt].mean()
        oh = np.maximum(oh, zero_rate_threshold)
        mh = np.maximum(mh, zero_rate_threshold)
        mf = np.maximum(mf, zero_rate_threshold)
        mf_unbiased = np.maximum(mf_unbiased, zero_rate_threshold)
        x = mf / mh
        x_hat = mf_unbiased / oh
        k[nt] = x / x_hat
    return k


def qdm_row(subset, oh, mh, mf, relative, denom_min):
    """``QuantileDeltaMapping(oh, mh, mf, dist='empirical', relative=...,
    sampling='linear', delta_denom_min=...)(subset)`` through the
    restatement of tests/bias_ref.py, in the dtype of ``subset``"""
    dt = subset.dtype
    return bias_ref.quantile_delta_mapping(
        subset[:, None], oh[None].astype(dt), mh[None].astype(dt),
        mf[None].astype(dt), relative=relative,
        delta_denom_min=denom_min)[:, 0]


def run_single_presrat(bias_data, bias_fut_data, base_data, base_ti, bias_ti,
                       bias_fut_ti, bias_feature, base_dset, n_samples,
                       n_time_steps, window_size, relative,
                       zero_rate_threshold, store=np.float32):
    """presrat.py:282-360; the extra key 'corrected' is the corrected series,
    'tau' and 'z_fg' the two intermediate figures"""
    window_size = window_size or 365 / n_time_steps
    centers = window_center(n_time_steps)
    template = np.full((n_time_steps, n_samples), np.nan, store)
    out = {k: template.copy() for k in (
        f'base_{base_dset}_params', f'bias_{bias_feature}_params',
        f'bias_fut_{bias_feature}_params')}
    corrected_fut_data = np.full_like(bias_fut_data, np.nan)
    for nt, t in enumerate(centers):
        base_idx = window_mask(base_ti.day_of_year, t, window_size)
        bias_idx = window_mask(bias_ti.day_of_year, t, window_size)
        bias_fut_idx = window_mask(bias_fut_ti.day_of_year, t, window_size)
        if any(base_idx) and any(bias_idx) and any(bias_fut_idx):
            tmp = get_qdm_params(bias_data[bias_idx],
                                 bias_fut_data[bias_fut_idx],
                                 base_data[base_idx], bias_feature, base_dset,
                                 n_samples)
            for k, v in tmp.items():
                out[k][(nt), :] = v
        subset = bias_fut_data[bias_fut_idx]
        corrected_fut_data[bias_fut_idx] = qdm_row(
            subset, np.asarray(out[f'base_{base_dset}_params'][nt]),
            np.asarray(out[f'bias_{bias_feature}_params'][nt]),
            np.asarray(out[f'bias_fut_{bias_feature}_params'][nt]),
            relative, zero_rate_threshold)
    tau_fut, obs_zero_rate, tau, z_fg = calc_tau_fut(
        base_data, bias_data, bias_fut_data, corrected_fut_data,
        zero_rate_threshold)
    k = calc_k_factor(base_data, bias_data, bias_fut_data,
                      corrected_fut_data, base_ti, bias_ti, bias_fut_ti,
                      centers, window_size, n_time_steps, zero_rate_threshold,
                      store)
    out[f'{bias_feature}_k_factor'] = k
    out[f'{base_dset}_zero_rate'] = obs_zero_rate
    out[f'{bias_feature}_tau_fut'] = tau_fut
    out['corrected'] = corrected_fut_data
    out['tau'] = tau
    out['z_fg'] = z_fg
    return out


# ---------------------------------------------------------------- mixins.py
def nn_fill_array(array):
    """utilities.py:55-75"""
    nan_mask = np.isnan(array)
    indices = nd.distance_transform_edt(nan_mask, return_distances=False,
                                        return_indices=True)
    return array[tuple(indices)]


def fill_and_smooth(out, fill_extend=True, smooth_extend=0,
                    smooth_interior=0):
    """mixins.py:69-102"""
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
                arr_smooth_ext = nd.gaussian_filter(arr_smooth_ext,
                                                    smooth_extend,
                                                    mode='nearest')
            if smooth_interior > 0:
                arr_smooth_int = nd.gaussian_filter(arr_smooth_int,
                                                    smooth_interior,
                                                    mode='nearest')
            out[key][nan_mask, idt] = arr_smooth_ext[nan_mask]
            out[key][~nan_mask, idt] = arr_smooth_int[~nan_mask]
    return out


# -------------------------------------------------------- a whole calculator
def init_out(kind, shape, bias_feature, base_dset, n_time_steps=None,
             n_quantiles=None, store=np.float32):
    """bias_calc.py:33-48, qdm.py:250-270, presrat.py:80-94"""
    if kind in LINEAR:
        nt = 12 if kind.startswith('Monthly') else 1
        keys = [f'{bias_feature}_scalar', f'{bias_feature}_adder',
                f'bias_{bias_feature}_mean', f'bias_{bias_feature}_std',
                f'base_{base_dset}_mean', f'base_{base_dset}_std']
        return {k: np.full((*shape, nt), np.nan, store) for k in keys}
    out = {k: np.full((*shape, n_time_steps, n_quantiles), np.nan, store)
           for k in (f'bias_{bias_feature}_params',
                     f'bias_fut_{bias_feature}_params',
                     f'base_{base_dset}_params')}
    if kind == 'PresRat':
        out[f'{base_dset}_zero_rate'] = np.full((*shape, 1), np.nan,
                                                store)
        out[f'{bias_feature}_tau_fut'] = np.full((*shape, 1), np.nan,
                                                 store)
        out[f'{bias_feature}_k_factor'] = np.full((*shape, n_time_steps),
                                                  np.nan, store)
    return out


def site_major(arr, lat_lon):
    """(R1, R2, T) -> (T, R1 * R2) for a raster ``lat_lon`` (R1, R2, 2)"""
    arr = np.asarray(arr)
    if lat_lon.ndim == 3:
        return np.ascontiguousarray(arr.reshape(-1, arr.shape[-1]).T)
    return arr


def run(kind, inp, dtype, daily_reduction='avg', fill_extend=True,
        smooth_extend=0, smooth_interior=0, zero_rate_threshold=1.157e-7,
        extras=None, only=None):
    """``_run`` (abstract.py:70-113) of calculator ``kind`` over the inputs
    ``inp`` (the keywords of the class as a dict) in ``dtype``; the tables
    are stored in ``dtype`` too, so that ``R64`` is not rounded to the
    reference's float32 tables.  ``extras``
    (a dict) receives per-pixel intermediates: 'base' (the reduced base
    series), 'bias' (after decimals / match_zero_rate), PresRat's 'corrected',
    'tau', 'z_fg'.  ``only``: the pixels to visit (default: all).

    One deviation: a pixel is bad when NO site maps to it (the reference's
    ``base_gid.any()`` also drops a pixel whose only site is site 0)."""
    bias_lat_lon = np.asarray(inp['bias_lat_lon'])
    base_lat_lon = np.asarray(inp['base_lat_lon'])
    raster = base_lat_lon.ndim == 3
    feat, dset = inp['bias_feature'], inp['base_dset']
    decimals = inp.get('decimals')
    base_data = inp['base_data']
    if isinstance(base_data, tuple):
        base_data = [base_data]
    cs = inp.get('base_cs_ghi')
    if cs is not None and hasattr(cs, 'shape'):
        cs = [cs]
    entries = [(site_major(a, base_lat_lon).astype(dtype, copy=False),
                pd.DatetimeIndex(ti),
                None if cs is None else site_major(
                    cs[i], base_lat_lon).astype(dtype, copy=False))
               for i, (a, ti) in enumerate(base_data)]
    bias = np.asarray(inp['bias_data']).astype(dtype)
    bias_ti = pd.DatetimeIndex(inp['bias_time_index'])
    shape = bias.shape[:2]
    qdm = kind not in LINEAR
    if qdm:
        fut = np.asarray(inp['bias_fut_data']).astype(dtype)
        fut_ti = pd.DatetimeIndex(inp['bias_fut_time_index'])
        n_q = inp.get('n_quantiles', 101)
        n_t = inp.get('n_time_steps', 24)
        w_size = inp.get('window_size', 120)
    _, nn_ind = nn_query(bias_lat_lon, base_lat_lon,
                         inp.get('distance_upper_bound'))
    out = init_out(kind, shape, feat, dset, n_t if qdm else None,
                   n_q if qdm else None, store=dtype)
    for gid in (range(shape[0] * shape[1]) if only is None else only):
        base_gid = np.where(nn_ind == gid)[0]
        if len(base_gid) == 0:
            continue
        loc = np.unravel_index(gid, shape)
        bias_data = bias[loc]
        if decimals is not None:
            bias_data = np.around(bias_data, decimals=decimals)
        bias_data = np.array(bias_data)
        with quiet():
            base, base_ti = get_base_data(entries, dset, base_gid, raster,
                                          daily_reduction, decimals)
        if qdm:
            fut_data = fut[loc]
            if decimals is not None:
                fut_data = np.around(fut_data, decimals=decimals)
        with quiet():
            if not qdm:
                single = run_single_linear(
                    kind, bias_data, base, base_ti, bias_ti, feat, dset,
                    mzr=inp.get('match_zero_rate', False), store=dtype)
            elif kind == 'PresRat':
                single = run_single_presrat(
                    bias_data, fut_data, base, base_ti, bias_ti, fut_ti,
                    feat, dset, n_q, n_t, w_size, inp.get('relative', True),
                    zero_rate_threshold, store=dtype)
            else:
                single = run_single_qdm(
                    bias_data, fut_data, base, base_ti, bias_ti, fut_ti,
                    feat, dset, n_q, n_t, w_size, store=dtype)
        if extras is not None:
            extras.setdefault('base', {})[gid] = base
            extras.setdefault('bias', {})[gid] = bias_data
            for k in ('corrected', 'tau', 'z_fg'):
                if k in single:
                    extras.setdefault(k, {})[gid] = single[k]
        for key, arr in single.items():
            if key in out:
                out[key][loc] = arr
    return fill_and_smooth(out, fill_extend, smooth_extend, smooth_interior)


# ------------------------------------------------------------ seeded inputs
def seeded_inputs(layout='sites', seed=0, years=('2019', '2020', '2021'),
                  fut_start='2050-01-01', base_freq='h', split=True):
    """The keywords of a calculator on a (3, 4) bias grid (1 degree) under a
    (7, 9) base raster (``layout='raster'``) or 40 scattered sites
    (``'sites'``), neither of which reaches the last column of the grid (three
    bad pixels, two of them corners): daily bias data over ``years`` (2020 is
    a leap year: day 366), base data at ``base_freq`` as one entry per year
    (``split``) or one entry.  The values look like precipitation: a third
    of the days is dry in the whole base domain, the bias series drizzles.
    The scattered sites hold NaNs, one pixel's sites all at once for a few
    steps."""
    rng = np.random.default_rng(seed)
    lat, lon = np.meshgrid(40.0 - np.arange(3), -105.0 + np.arange(4),
                           indexing='ij')
    bias_lat_lon = np.stack([lat, lon], axis=-1)
    bias_ti = pd.date_range(f'{years[0]}-01-01', f'{years[-1]}-12-31',
                            freq='D')
    fut_ti = pd.date_range(fut_start, periods=len(bias_ti), freq='D')
    season = 1 + 0.5 * np.sin(2 * np.pi * bias_ti.dayofyear.values / 365.25)
    bias = np.maximum(0, rng.normal(0.6, 1.0, (3, 4, len(bias_ti)))) * season
    fut = np.maximum(0, rng.normal(0.8, 1.2, (3, 4, len(fut_ti)))) * season
    if layout == 'raster':
        blat, blon = np.meshgrid(np.linspace(40.3, 37.8, 7),
                                 np.linspace(-105.3, -102.6, 9),
                                 indexing='ij')
        base_lat_lon = np.stack([blat, blon], axis=-1)
        n_sites = 63
    else:
        base_lat_lon = np.stack([rng.uniform(37.7, 40.3, 40),
                                 rng.uniform(-105.3, -102.6, 40)], axis=-1)
        n_sites = 40
    entries = []
    for y in (years if split else [None]):
        ti = pd.date_range(
            f'{y or years[0]}-01-01', f'{y or years[-1]}-12-31 23:59',
            freq=base_freq)
        days = (ti.normalize() - ti[0].normalize()).days.values
        wet = rng.random(days.max() + 1) > 1 / 3
        arr = np.maximum(0, rng.normal(0.2, 1.0, (len(ti), n_sites)))
        arr *= wet[days][:, None] * (1 + 0.3 * np.cos(
            2 * np.pi * ti.dayofyear.values / 365.25))[:, None]
        arr = arr.astype(np.float32)
        if layout == 'sites':
            arr[rng.random(arr.shape) < 0.01] = np.nan
            _, nn = nn_query(bias_lat_lon, base_lat_lon)
            arr[5:8, nn == 5] = np.nan
        else:
            arr = np.ascontiguousarray(arr.T).reshape(7, 9, -1)
        entries.append((arr, ti))
    return dict(base_data=entries if split else entries[0],
                bias_data=bias.astype(np.float32), base_dset='pr_obs',
                bias_feature='pr', base_lat_lon=base_lat_lon,
                bias_lat_lon=bias_lat_lon, bias_time_index=bias_ti,
                bias_fut_data=fut.astype(np.float32),
                bias_fut_time_index=fut_ti)


# -------------------------------------------- the kernels' calls, in numpy
class Backend:
    """What ``sup3r_amd.bias_calc.DeviceBackend`` offers, computed with the
    functions above in float32: series are numpy arrays ``(P, T)``."""

    def upload(self, a):
        return np.array(a, np.float32)

    def to_host(self, t):
        return np.asarray(t)

    def base_series(self, entries, site_ptr, site_idx, plans, n_days_total,
                    reduction, flags=0, decimals=0):
        n_pix = len(site_ptr) - 1
        out = np.full((n_pix, n_days_total), np.nan, np.float32)
        name = ['avg', 'max', 'min', 'sum', None][reduction]
        for (base, cs), (day_ptr, step_idx, off) in zip(entries, plans):
            n_days = len(day_ptr) - 1
            day = np.empty(len(step_idx), np.int64)
            for d in range(n_days):
                day[step_idx[day_ptr[d]:day_ptr[d + 1]]] = d
            ti = pd.DatetimeIndex(pd.Timestamp('2000-01-01')
                                  + pd.to_timedelta(day, unit='D'))
            for p in range(n_pix):
                gid = site_idx[site_ptr[p]:site_ptr[p + 1]]
                if not len(gid):
                    continue
                with quiet():
                    data, _ = get_base_data(
                        [(np.asarray(base, np.float32), ti, cs)],
                        'clearsky_ratio' if flags & 2 else 'x', gid,
                        raster=not flags & 1, daily_reduction=name,
                        decimals=decimals if flags & 4 else None)
                out[p, off:off + n_days] = data
        return out

    def moments(self, series, group, n_groups):
        n_pix = series.shape[0]
        cnt = np.zeros((n_pix, n_groups), np.int32)
        mean = np.full((n_pix, n_groups), np.nan, np.float32)
        std = np.full((n_pix, n_groups), np.nan, np.float32)
        with quiet():
            for g in range(n_groups):
                sel = series[:, np.asarray(group) == g]
                cnt[:, g] = (~np.isnan(sel)).sum(axis=1)
                if sel.shape[1]:
                    mean[:, g] = np.nanmean(sel, axis=1)
                    std[:, g] = np.nanstd(sel, axis=1)
        return cnt, mean, std

    def window_quantiles(self, series, win_ptr, member, n_q):
        n_pix, n_w = series.shape[0], len(win_ptr) - 1
        out = np.full((n_pix, n_w, n_q), np.nan, np.float32)
        q = np.linspace(0, 1, n_q)
        for w in range(n_w):
            m = member[win_ptr[w]:win_ptr[w + 1]]
            if len(m):
                out[:, w] = np.quantile(series[:, m], q, axis=1).T
        return out

    def match_zero_rate(self, base_series, bias_series):
        mv = np.full(len(bias_series), np.nan)
        bad = int((~np.isfinite(bias_series)).sum())
        if not bad:
            for p in range(len(bias_series)):
                bias_series[p], mv[p] = match_zero_rate(bias_series[p],
                                                        base_series[p])
        return bias_series, mv, bad

    def mask_windows(self, tables, bad_windows):
        for t in tables:
            t[:, np.asarray(bad_windows)] = np.nan

    def presrat(self, base, bias, fut, tables, relative, threshold,
                last_win, lists):
        n_pix, n_w, _ = tables[0].shape
        res = {'corrected': np.full(fut.shape, np.nan, np.float32),
               'zero_rate': np.full(n_pix, np.nan, np.float32),
               'tau': np.full(n_pix, np.nan, np.float32),
               'z_fg': np.full(n_pix, np.nan, np.float32),
               'tau_fut': np.full(n_pix, np.nan, np.float32),
               'k_factor': np.full((n_pix, n_w), np.nan, np.float32),
               'status': np.zeros(3, np.int32)}
        res['status'][0] = (~np.isfinite(bias)).sum()
        res['status'][1] = (~np.isfinite(fut)).sum()
        if res['status'][:2].any():
            return res
        members = [[m[p[w]:p[w + 1]] for w in range(n_w)] for p, m in lists]
        with quiet():
            for p in range(n_pix):
                c = res['corrected'][p]
                for w in range(n_w):
                    m = members[2][w]
                    c[m] = qdm_row(fut[p][m], tables[0][p, w],
                                   tables[1][p, w], tables[2][p, w], relative,
                                   threshold)
                rate = zero_precipitation_rate(base[p], threshold)
                res['zero_rate'][p] = rate
                tau = np.float32(np.nan)
                if not np.isnan(rate):
                    nth = min(round(rate * bias[p].size), bias[p].size - 1)
                    tau = np.sort(bias[p])[nth]
                z_fg = (fut[p] < tau).astype('i').sum() / fut[p].size
                res['tau'][p], res['z_fg'][p] = tau, z_fg
                idx = round(z_fg * c.size)
                if idx >= c.size:
                    res['status'][2] += 1
                else:
                    res['tau_fut'][p] = np.sort(c)[idx]
                for w in range(n_w):
                    means = [base[p][members[0][w]].mean(),
                             bias[p][members[1][w]].mean(),
                             fut[p][members[2][w]].mean(),
                             c[members[2][w]].mean()]
                    oh, mh, mf, mfu = (np.maximum(v, threshold)
                                       for v in means)
                    res['k_factor'][p, w] = (mf / mh) / (mfu / oh)
        return res
