"""Restatements for the tests of ``sup3r_amd.exo``.  Nothing here imports
``sup3r_amd``.

* the reference's own route, followed line by line with scipy's ``KDTree`` /
  ``griddata`` and the pandas group-by: ``get_distance_upper_bound``,
  ``query_tree``, ``_get_data_2d``, ``_get_data_3d`` (sup3r/preprocessing/
  rasterizers/exo.py:275-458), ``nn_fill_array`` (sup3r/utilities/
  utilities.py:55-75), ``get_lat_lon`` / ``get_times`` (sup3r/writers/
  base.py:348-551);
* a brute-force float64 nearest search under the device's rules: ``d2 = dlat
  dlat + dlon dlon`` on the widened inputs, a hit only if ``d2 < r r``, the
  smallest target id among equal ``d2``;
* an exact group mean: ``float32(float64(fsum) / n * scale)``."""
import math

import numpy as np
import pandas as pd
from scipy import ndimage as nd
from scipy.interpolate import griddata
from scipy.spatial import KDTree


# ------------------------------------------------------- the reference's route
def get_distance_upper_bound(hr_lat_lon):
    diff = np.diff(hr_lat_lon, axis=0)
    diff = np.abs(np.median(diff, axis=0)).max()
    return np.asarray(diff)


def query_tree(hr_lat_lon, source_lat_lon, distance_upper_bound):
    """-> (dists, nn) as ``KDTree.query`` returns them"""
    tree = KDTree(hr_lat_lon.reshape((-1, 2)))
    return tree.query(source_lat_lon,
                      distance_upper_bound=distance_upper_bound)


def get_data_2d(feature, source_data, nn, hr_shape):
    assert len(source_data.shape) == 2 and source_data.shape[1] == 1
    df = pd.DataFrame({feature: source_data.flatten(), 'gid_target': nn})
    n_target = np.prod(hr_shape[:-1])
    out = np.full((n_target, 1), np.nan, dtype=np.float32)
    df = df[df['gid_target'] != n_target]
    df = df.sort_values('gid_target')
    df = df.groupby('gid_target').mean()
    inds = df.index.values[df.index.values != n_target]
    out[inds, 0] = df[feature].values
    return out.reshape(hr_shape[:-1])


def get_data_3d(feature, source_data, source_time_index, nn, dists, hr_shape,
                hr_time_index):
    target_tmask = hr_time_index.isin(source_time_index)
    source_tmask = source_time_index.isin(hr_time_index)
    data = source_data[:, source_tmask]
    rows = pd.MultiIndex.from_product(
        [nn, range(data.shape[-1])], names=['gid_target', 'time'])
    dists = np.repeat(dists[:, None], data.shape[-1], axis=1)
    n_target = np.prod(hr_shape[:-1])
    df = pd.DataFrame(
        {feature: data.flatten(), 'distance': dists.flatten()}, index=rows)
    df = df[df.index.get_level_values(0) != n_target].sort_values(
        'gid_target')
    df = df.groupby(['gid_target', 'time']).apply(lambda x: x[feature].mean())
    out = np.full((n_target, len(hr_time_index)), np.nan, dtype=np.float32)
    inds = np.array(df.index.get_level_values(0).unique())[:, None]
    out[inds, target_tmask] = df.values.reshape((-1, data.shape[-1]))
    out = out.reshape((*hr_shape[:-1], -1))
    return out


def nn_fill_array(array):
    nan_mask = np.isnan(array)
    indices = nd.distance_transform_edt(
        nan_mask, return_distances=False, return_indices=True)
    return array[tuple(indices)]


def pad_lat_lon(lat_lon):
    padded_grid = np.zeros((2 + lat_lon.shape[0], 2 + lat_lon.shape[1], 2))
    padded_grid[1:-1, 1:-1, :] = lat_lon
    left_diffs = padded_grid[:, 2, 1] - padded_grid[:, 1, 1]
    right_diffs = padded_grid[:, -2, 1] - padded_grid[:, -3, 1]
    top_diffs = padded_grid[1, :, 0] - padded_grid[2, :, 0]
    bottom_diffs = padded_grid[-3, :, 0] - padded_grid[-2, :, 0]
    padded_grid[:, 0, 1] = padded_grid[:, 1, 1] - left_diffs
    padded_grid[:, 0, 0] = padded_grid[:, 1, 0]
    padded_grid[:, -1, 1] = padded_grid[:, -2, 1] + right_diffs
    padded_grid[:, -1, 0] = padded_grid[:, -2, 0]
    padded_grid[0, :, 0] = padded_grid[1, :, 0] + top_diffs
    padded_grid[0, :, 1] = padded_grid[1, :, 1]
    padded_grid[-1, :, 0] = padded_grid[-2, :, 0] - bottom_diffs
    padded_grid[-1, :, 1] = padded_grid[-2, :, 1]
    padded_grid[0, 0, 0] = padded_grid[0, 1, 0]
    padded_grid[0, 0, 1] = padded_grid[1, 0, 1]
    padded_grid[0, -1, 0] = padded_grid[0, -2, 0]
    padded_grid[0, -1, 1] = padded_grid[1, -1, 1]
    padded_grid[-1, 0, 0] = padded_grid[-1, 1, 0]
    padded_grid[-1, 0, 1] = padded_grid[-2, 0, 1]
    padded_grid[-1, -1, 0] = padded_grid[-1, -2, 0]
    padded_grid[-1, -1, 1] = padded_grid[-2, -1, 1]
    return padded_grid


def is_increasing_lons(lat_lon):
    for i in range(lat_lon.shape[0]):
        if lat_lon[i, :, 1][-1] < lat_lon[i, :, 1][0]:
            return False
    return True


def get_lat_lon(low_res_lat_lon, shape):
    """as the reference: modifies ``low_res_lat_lon`` in place"""
    assert low_res_lat_lon.shape[0] > 1 and low_res_lat_lon.shape[1] > 1
    low_res_lat_lon[..., 1] = (low_res_lat_lon[..., 1] + 180) % 360 - 180
    if not is_increasing_lons(low_res_lat_lon):
        low_res_lat_lon[..., 1] = (low_res_lat_lon[..., 1] + 360) % 360
    padded_grid = pad_lat_lon(low_res_lat_lon)
    lats = padded_grid[..., 0].flatten()
    lons = padded_grid[..., 1].flatten()
    lr_y, lr_x = low_res_lat_lon.shape[:-1]
    hr_y, hr_x = shape
    y = np.arange(0, 10, 10 / lr_y) + 5 / lr_y
    x = np.arange(0, 10, 10 / lr_x) + 5 / lr_x
    y = np.concatenate([[y[0] - 10 / lr_y], y, [y[-1] + 10 / lr_y]])
    x = np.concatenate([[x[0] - 10 / lr_x], x, [x[-1] + 10 / lr_x]])
    new_y = np.arange(0, 10, 10 / hr_y) + 5 / hr_y
    new_x = np.arange(0, 10, 10 / hr_x) + 5 / hr_x
    X, Y = np.meshgrid(x, y, copy=False)
    old = np.array([Y.flatten(), X.flatten()], dtype=np.float32).T
    X, Y = np.meshgrid(new_x, new_y, copy=False)
    new = np.array([Y.flatten(), X.flatten()], dtype=np.float32).T
    lons = griddata(old, lons, new)
    lats = griddata(old, lats, new)
    lons = (lons + 180) % 360 - 180
    lat_lon = np.dstack((lats.reshape(shape), lons.reshape(shape)))
    return lat_lon


def get_time_index_freqs(time_index):
    unique_freqs = (list(set(np.diff(time_index))) if len(time_index) > 1
                    else [np.timedelta64(1, 'D')])
    unique_freqs /= np.timedelta64(1, 's')
    nominal_freq = pd.tseries.offsets.DateOffset(seconds=min(unique_freqs))
    return nominal_freq, unique_freqs


def get_times(low_res_times, shape):
    t_enhance = int(shape / len(low_res_times))
    offset, _ = get_time_index_freqs(low_res_times)
    freq = pd.tseries.offsets.DateOffset(
        seconds=int(offset.seconds / t_enhance))
    times = pd.date_range(low_res_times[0], low_res_times[-1] + offset,
                          freq=freq)[:-1]
    has_leap = any((low_res_times.month == 2) & (low_res_times.day == 29))
    if not has_leap:
        leap_mask = (times.month == 2) & (times.day == 29)
        times = times[~leap_mask]
    assert len(times) == shape
    return times


# --------------------------------------------------- the device's rules, exact
def brute_nearest(src, tgt, r, block=4096):
    """``(nn int64, dists float64)``: ``n_target`` / ``inf`` for a miss"""
    src = np.asarray(src, np.float32).astype(np.float64)
    tgt = np.asarray(tgt, np.float32).astype(np.float64)
    m = len(tgt)
    r2 = float(r) * float(r)
    nn = np.full(len(src), m, dtype=np.int64)
    dists = np.full(len(src), np.inf)
    for lo in range(0, len(src), block):
        s = src[lo:lo + block]
        dla = s[:, None, 0] - tgt[None, :, 0]
        dlo = s[:, None, 1] - tgt[None, :, 1]
        d2 = dla * dla + dlo * dlo
        with np.errstate(invalid='ignore'):
            d2 = np.where(d2 < r2, d2, np.inf)
        best = d2.min(axis=1)
        first = np.argmax(d2 == best[:, None], axis=1)   # the smallest id
        hit = np.isfinite(best)
        nn[lo:lo + block] = np.where(hit, first, m)
        dists[lo:lo + block] = np.where(hit, np.sqrt(best), np.inf)
    return nn, dists


def _two_nearest_d2(src, tgt):
    """float64 ``d2`` of every source to its two nearest targets (the tree
    finds them; the arithmetic is the device's); (n, 2), inf where there is
    one target only"""
    src = np.asarray(src, np.float32).astype(np.float64)
    tgt = np.asarray(tgt, np.float32).astype(np.float64)
    k = min(2, len(tgt))
    _, idx = KDTree(tgt).query(src, k=k)
    idx = idx.reshape(len(src), k)
    d = src[:, None, :] - tgt[idx]
    d2 = np.sort(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1], axis=1)
    if k == 1:
        d2 = np.concatenate([d2, np.full_like(d2, np.inf)], axis=1)
    return d2


def nearest_margins(src, tgt, r):
    """what a comparison with scipy presupposes, in float64: ``gap``, the
    smallest relative difference between a source's nearest and
    second-nearest ``d2``, and ``clear``: no target lies within a relative
    1e-9 of the distance ``r`` from a source (so no ``d2`` within a relative
    2^-50 of ``r r``, by eight orders of magnitude)"""
    d2 = _two_nearest_d2(src, tgt)
    with np.errstate(invalid='ignore', divide='ignore'):
        rel = np.where(d2[:, 1] > 0, (d2[:, 1] - d2[:, 0]) / d2[:, 1], 0.0)
    tree = KDTree(np.asarray(tgt, np.float32).astype(np.float64))
    s64 = np.asarray(src, np.float32).astype(np.float64)
    inner = tree.query_ball_point(s64, float(r) * (1 - 1e-9),
                                  return_length=True)
    outer = tree.query_ball_point(s64, float(r) * (1 + 1e-9),
                                  return_length=True)
    return float(rel.min()), bool((inner == outer).all())


def untie(src, tgt):
    """``src`` with the latitude of every source that lies at exactly the
    same distance from its two nearest targets moved by one float32 step (a
    float32 point over an axis-aligned float32 grid sits exactly on the line
    between two rows or columns about once in 10^5 draws)"""
    src = np.array(src, np.float32)
    for _ in range(4):
        d2 = _two_nearest_d2(src, tgt)
        tied = d2[:, 0] == d2[:, 1]
        if not tied.any():
            break
        src[tied, 0] = np.nextafter(src[tied, 0], np.float32(np.inf))
        src[tied, 1] = np.nextafter(src[tied, 1], np.float32(np.inf))
    return src


def exact_group_mean(nn, values, n_target, t_out, cols, scale=1.0):
    """``(n_target, t_out)`` float32, NaN where nothing was written: per
    target and column ``float32(float64(fsum) / n * scale)`` over the non-NaN
    values mapped to it.  Also returns ``n`` and ``sum |x| / n`` per cell
    (``(n_target, len(cols))``), for the error bounds."""
    nn = np.asarray(nn, np.int64)
    values = np.asarray(values, np.float32)
    out = np.full((n_target, t_out), np.nan, dtype=np.float32)
    count = np.zeros((n_target, len(cols)), dtype=np.int64)
    mean_abs = np.zeros((n_target, len(cols)))
    order = np.argsort(nn, kind='stable')
    snn = nn[order]
    starts = np.searchsorted(snn, np.arange(n_target))
    stops = np.searchsorted(snn, np.arange(n_target), side='right')
    for k, col in enumerate(cols):
        with np.errstate(invalid='ignore'):           # signalling NaNs
            x = values[order, k].astype(np.float64)
        for m in range(n_target):
            grp = x[starts[m]:stops[m]]
            grp = grp[~np.isnan(grp)]
            if len(grp):
                out[m, col] = np.float32(
                    np.float64(math.fsum(grp)) / len(grp) * scale)
                count[m, k] = len(grp)
                mean_abs[m, k] = math.fsum(np.abs(grp)) / len(grp)
    return out, count, mean_abs
