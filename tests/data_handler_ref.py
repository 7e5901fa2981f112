"""numpy restatement of the reference's data-handler procedures, for the tests
of sup3r_amd/data_handlers.py.  Line numbers are those of the reference:

    rasterizers/base.py:143-231       target / shape -> row and column slices
    rasterizers/extended.py:128-154   flattened data -> raster
    data_handlers/base.py:325-380     DailyDataHandler._deriver_hook
    data_handlers/nc_cc.py:144-240    get_time_slice, get_clearsky_ghi,
                                      scale_clearsky_ghi

xarray's ``coarsen().mean() / .max() / .min() / .sum()`` and ``.max(dim=)``
are taken to skip NaN (``skipna=None`` on float data) and are restated with
numpy's ``nan*`` functions in float64.
"""
import warnings

import numpy as np
import pandas as pd


# ------------------------------------------------------------- rasterizer
def closest_row_col(lat_lon, target, threshold=None):
    """base.py:193-226"""
    dist = np.hypot(lat_lon[..., 0] - target[0], lat_lon[..., 1] - target[1])
    row, col = np.unravel_index(np.argmin(dist, axis=None), dist.shape)
    if threshold is not None and dist.min() > threshold:
        raise RuntimeError('exceeds the given threshold')
    return int(row), int(col)


def raster_slices(full_lat_lon, target=None, shape=None, threshold=None):
    """base.py:143-191: ``(lat_slice, lon_slice, lat_clipped, lon_clipped)``"""
    if target is None:
        target = full_lat_lon[-1, 0, :]
    if shape is None:
        shape = full_lat_lon.shape[:-1]
    row, col = closest_row_col(full_lat_lon, target, threshold)
    lat = slice(row - shape[0] + 1, row + 1)
    lon = slice(col, col + shape[1])
    new_lat = slice(max(lat.start, 0), min(lat.stop, full_lat_lon.shape[0]))
    new_lon = slice(max(lon.start, 0), min(lon.stop, full_lat_lon.shape[1]))
    return new_lat, new_lon, new_lat != lat, new_lon != lon


def parse_time_slice(value):
    """preprocessing/utilities.py:280-289"""
    return (value if isinstance(value, slice) else slice(*value)
            if isinstance(value, (tuple, list)) else slice(None))


def rasterize_grid(a, lat_slice, lon_slice, time_slice):
    """base.py:131-141: ``isel`` of a gridded array"""
    a = np.asarray(a)
    if a.ndim == 2:
        return a[lat_slice, lon_slice]
    return a[lat_slice, lon_slice, parse_time_slice(time_slice)]


def rasterize_flat(a, raster_index, time_slice):
    """extended.py:139-151"""
    a = np.asarray(a)
    flat = np.asarray(raster_index).flatten()
    if a.ndim == 1:
        return a[flat].reshape(raster_index.shape)
    dat = a[:, flat][parse_time_slice(time_slice)]          # (t, sites)
    return np.moveaxis(dat, 0, -1).reshape(*raster_index.shape, -1)


# ------------------------------------------------------------ daily handler
def windows(plane, w):
    """``(..., D, w)`` float64 windows of ``(..., D w)``"""
    plane = np.asarray(plane, np.float64)
    return plane.reshape(*plane.shape[:-1], -1, w)


def reduce64(plane, w, op):
    """float64 ``coarsen(time=w).<op>()`` and the windows' sums of |x| (NaN
    as 0), for the tolerance"""
    win = windows(plane, w)
    fn = {'mean': np.nanmean, 'max': np.nanmax, 'min': np.nanmin,
          'sum': np.nansum}[op]
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        finite = np.where(np.isfinite(win), np.abs(win), 0.0)
        return fn(win, axis=-1), finite.sum(axis=-1)


def daily_hook(planes, features, day_steps):
    """base.py:344-370: ``{name: (s1, s2, D) float32}`` of every feature, and
    of ``total_clearsky_ghi`` / ``total_ghi`` with ``clearsky_ratio``"""
    daily = {f: reduce64(planes[f], day_steps, 'mean')[0] for f in features}
    feats = [f for f in features if 'clearsky_ratio' not in f]
    if 'clearsky_ratio' in features:
        feats = [*feats, 'total_clearsky_ghi', 'total_ghi']
    for fname in feats:
        if '_max_' in fname:
            daily[fname] = reduce64(planes[fname], day_steps, 'max')[0]
        if '_min_' in fname:
            daily[fname] = reduce64(planes[fname], day_steps, 'min')[0]
        if 'total_' in fname:
            daily[fname] = reduce64(planes[fname.split('total_')[-1]],
                                    day_steps, 'sum')[0]
    daily = {k: v.astype(np.float32) for k, v in daily.items()}
    if 'clearsky_ratio' in features:
        with np.errstate(all='ignore'):
            daily['clearsky_ratio'] = (daily['total_ghi']
                                       / daily['total_clearsky_ghi'])
    return daily


def ulp32(x):
    """the spacing of float32 at ``|x|`` (inf / NaN: inf)"""
    x = np.abs(np.asarray(x, np.float64)).astype(np.float32)
    with np.errstate(all='ignore'):
        return np.where(np.isfinite(x), np.spacing(x), np.inf).astype(
            np.float64)


def sum_tolerance(ref64, sum_abs):
    """``ulp32(ref) + 2^-45 sum|x|``: both routes add at most ``w`` float64
    roundings of ``2^-53 sum|x|`` each (``w <= 256``), and one more float32
    rounding can separate them by an ulp"""
    return ulp32(ref64) + 2.0 ** -45 * np.asarray(sum_abs, np.float64)


def assert_close_sum(got, ref64, sum_abs, what=''):
    """``got`` float32 against the float64 reference: NaN and inf where the
    reference has them, else within :func:`sum_tolerance`"""
    got = np.asarray(got, np.float64)
    ref64 = np.asarray(ref64, np.float64)
    special = ~np.isfinite(ref64)
    np.testing.assert_array_equal(got[special], ref64[special], err_msg=what)
    err = np.abs(got[~special] - ref64[~special])
    tol = sum_tolerance(ref64, sum_abs)[~special]
    worst = float((err / tol).max()) if err.size else 0.0
    print(f'{what}: worst error / tolerance = {worst:.3f}')
    assert (err <= tol).all(), (what, worst)


# ---------------------------------------------------------------- NC for CC
def get_time_slice(target_ti, ti_nsrdb):
    """nc_cc.py:144-158"""
    t_start = np.where((target_ti[0].month == ti_nsrdb.month)
                       & (target_ti[0].day == ti_nsrdb.day))[0][0]
    t_end = 1 + np.where((target_ti[-1].month == ti_nsrdb.month)
                         & (target_ti[-1].day == ti_nsrdb.day))[0][-1]
    return slice(int(t_start), int(t_end))


def steps_per_day(ti_nsrdb):
    """nc_cc.py:203-205"""
    from scipy.stats import mode
    time_freq = (ti_nsrdb[1:] - ti_nsrdb[:-1]).seconds / 3600
    time_freq = float(mode(time_freq, keepdims=False).mode)
    return int(24 // time_freq)


def get_clearsky_ghi(target_lat_lon, target_ti, nsrdb_lat_lon, ti_nsrdb, cs,
                     agg=1):
    """nc_cc.py:160-229: ``(cs_ghi (s1, s2, D) float64, sum|x| (s1, s2, D),
    site index (n_pix, agg))``; ``cs`` is ``(T, n_sites)``"""
    from scipy.spatial import KDTree
    t_slice = get_time_slice(target_ti, ti_nsrdb)
    cc_meta = target_lat_lon.reshape((-1, 2))
    _, i = KDTree(nsrdb_lat_lon).query(cc_meta, k=agg)
    i = np.expand_dims(i, axis=1) if len(i.shape) == 1 else i
    data = np.asarray(cs, np.float64)[t_slice][:, i.flatten()]
    m = steps_per_day(ti_nsrdb)
    if data.shape[0] % m:
        raise ValueError("boundary='exact'")
    finite = np.where(np.isfinite(data), np.abs(data), 0.0)
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        # spatial coarsening from NSRDB to GCM, then to the daily average
        site = np.nanmean(data.reshape(len(data), -1, agg), axis=-1)
        day = np.nanmean(site.reshape(-1, m, site.shape[-1]), axis=1)
    sum_abs = finite.reshape(-1, m, len(i), agg).sum(axis=(1, 3))
    stamps = pd.DatetimeIndex(
        np.asarray(ti_nsrdb[t_slice].values, 'datetime64[ns]').astype(
            np.int64).reshape(-1, m).mean(axis=1).astype('datetime64[ns]'))
    frame = pd.DataFrame(day, index=stamps.strftime('%m.%d'))
    sums = pd.DataFrame(sum_abs, index=stamps.strftime('%m.%d'))
    label = target_ti.strftime('%m.%d')
    if frame.index.has_duplicates:
        raise ValueError('cannot reindex: duplicate labels')
    shape = (*target_lat_lon.shape[:2], len(target_ti))
    return (frame.reindex(label).to_numpy().T.reshape(shape),
            sums.reindex(label).fillna(0.0).to_numpy().T.reshape(shape), i)


def scale_clearsky_ghi(rsds, cs_ghi):
    """nc_cc.py:231-240 in float32: ``(scaled, scale)``"""
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        scale = (np.nanmax(rsds, axis=-1) / np.nanmax(cs_ghi, axis=-1)).astype(
            np.float32)
        return (cs_ghi * scale[..., None]).astype(np.float32), scale


# ------------------------------------------------------------------ inputs
def grid_lat_lon(s1, s2, lat0=40.0, lon0=-105.0, d=0.25):
    """a regular grid, latitude falling with the row (the reference's
    orientation: ``lat_lon[-1, 0]`` is the lower left corner)"""
    lat = lat0 + d * np.arange(s1)[::-1]
    lon = lon0 + d * np.arange(s2)
    return np.stack(np.meshgrid(lat, lon, indexing='ij'), axis=-1).astype(
        np.float32)


def solar_planes(s1, s2, days, seed=0):
    """hourly ``ghi``, ``clearsky_ghi`` (0 at night) and ``temperature_2m``"""
    rng = np.random.default_rng(seed)
    hour = np.arange(24 * days) % 24
    sun = np.clip(np.sin((hour - 6) / 12 * np.pi), 0, None).astype(np.float32)
    cs = (900 * sun * rng.uniform(0.9, 1.0, (s1, s2, 1))).astype(np.float32)
    ghi = (cs * rng.uniform(0.2, 1.0, cs.shape)).astype(np.float32)
    temp = rng.normal(280, 8, cs.shape).astype(np.float32)
    return {'ghi': ghi, 'clearsky_ghi': cs, 'temperature_2m': temp}
