"""Rasterising exogenous fields on the device: ``ExoRasterizer`` and
``ExoDataHandler``.

The generators are conditioned on exogenous fields — topography at every
model step's resolution, aggregated onto the enhanced grid.  The reference
makes them with ``ExoDataHandler`` -> ``ExoRasterizer`` (sup3r/preprocessing/
data_handlers/exo.py:276-498, sup3r/preprocessing/rasterizers/exo.py): a
KD-tree on the enhanced lat/lon grid, the nearest target of every high-res
source pixel under a distance bound, a pandas group mean per target, holes
filled by nearest neighbour.  The classes here keep the reference's names,
constructor keywords, control flow, warnings and errors, and work over arrays
in the place of files:

* in the place of ``file_paths`` + ``input_handler_*``: an :class:`ExoInput`
  (or any object or mapping with ``lat_lon`` ``(s1, s2, 2)`` and
  ``time_index``);
* in the place of ``source_files`` + ``source_handler_kwargs``: an
  :class:`ExoSource` (or a mapping with ``lat_lon`` ``(..., 2)``, the
  feature's values under its name, shaped ``(...)`` or ``(..., T_src)``, and
  optionally ``time_index``);
* ``cache_dir``, ``chunks`` and ``max_workers`` are accepted and ignored with
  a logged note; ``cache_file`` still returns the reference's file name when
  ``cache_dir`` is given (the directory is not created), so callers can do
  their own caching.

The arithmetic sits behind a backend.  ``DeviceBackend`` calls
``s3_exo_nearest`` and ``s3_exo_group_mean`` (include/sup3r_hip.h,
csrc/kernels_exo.hip) and fills holes with ``s3_nn_fill``; ``NumpyBackend``
restates the same rules in numpy for testing the host control flow without a
GPU — it is no fallback: nothing selects it but the caller (``device=False``)
or the absence of a GPU.

Deviations from the reference, on purpose:
  * the target grid is float32, as the source coordinates are (the reference
    keeps ``griddata``'s float64 for ``s_enhance > 1``);
  * on an exact tie of the squared distance the smallest target id wins (the
    KD-tree's choice follows its traversal);
  * ``scale_factor`` multiplies the float64 mean before the one rounding to
    float32 (the reference rounds the mean, then multiplies in float32);
  * ``get_lat_lon`` does not modify the caller's array;
  * ``ExoDataHandler`` rasterises steps that share ``(s_enhance, t_enhance)``
    once, and all its steps share one upload of the source.

Not here: reading files, caching to disk, ``SzaRasterizer``'s solar position,
time aggregation of the source (the reference matches steps exactly, too) and
a longitude wrap in the distance (the reference has none).
"""
import ctypes as C
import logging
import os
from dataclasses import dataclass
from typing import ClassVar, Optional
from warnings import warn

import numpy as np

from . import _lib
from .derive import lowered

logger = logging.getLogger(__name__)

# (the two backends are reached as sup3r_amd.exo.DeviceBackend / NumpyBackend)
__all__ = ['ExoInput', 'ExoSource', 'ExoRaster', 'BaseExoRasterizer',
           'ObsRasterizer', 'SzaRasterizer', 'ExoRasterizer',
           'SingleExoDataStep', 'ExoDataHandler', 'get_lat_lon', 'get_times',
           'pad_lat_lon', 'is_increasing_lons']


# ------------------------------------------------- the enhanced coordinates
def pad_lat_lon(lat_lon):
    """OutputHandler.pad_lat_lon (writers/base.py:348-406): one row and
    column more on every side, at the edge's own spacing"""
    grid = np.zeros((2 + lat_lon.shape[0], 2 + lat_lon.shape[1], 2))
    grid[1:-1, 1:-1, :] = lat_lon
    left_diffs = grid[:, 2, 1] - grid[:, 1, 1]
    right_diffs = grid[:, -2, 1] - grid[:, -3, 1]
    top_diffs = grid[1, :, 0] - grid[2, :, 0]
    bottom_diffs = grid[-3, :, 0] - grid[-2, :, 0]
    grid[:, 0, 1] = grid[:, 1, 1] - left_diffs
    grid[:, 0, 0] = grid[:, 1, 0]
    grid[:, -1, 1] = grid[:, -2, 1] + right_diffs
    grid[:, -1, 0] = grid[:, -2, 0]
    grid[0, :, 0] = grid[1, :, 0] + top_diffs
    grid[0, :, 1] = grid[1, :, 1]
    grid[-1, :, 0] = grid[-2, :, 0] - bottom_diffs
    grid[-1, :, 1] = grid[-2, :, 1]
    grid[0, 0, 0], grid[0, 0, 1] = grid[0, 1, 0], grid[1, 0, 1]
    grid[0, -1, 0], grid[0, -1, 1] = grid[0, -2, 0], grid[1, -1, 1]
    grid[-1, 0, 0], grid[-1, 0, 1] = grid[-1, 1, 0], grid[-2, 0, 1]
    grid[-1, -1, 0], grid[-1, -1, 1] = grid[-1, -2, 0], grid[-2, -1, 1]
    return grid


def is_increasing_lons(lat_lon):
    """writers/base.py:408-432: no row whose last longitude is below its
    first (a grid through the 180 -> -180 boundary has one)"""
    for i in range(lat_lon.shape[0]):
        if lat_lon[i, :, 1][-1] < lat_lon[i, :, 1][0]:
            return False
    return True


def get_lat_lon(low_res_lat_lon, shape):
    """OutputHandler.get_lat_lon (writers/base.py:434-508): the ``(s1, s2, 2)``
    low-res grid remeshed to ``shape`` with scipy's ``griddata`` over a padded
    grid; a grid through the 180 degree boundary is shifted to 0 - 360 for
    the interpolation.  Unlike the reference this does not modify the
    caller's array: it works on a copy."""
    from scipy.interpolate import griddata
    low_res_lat_lon = np.array(low_res_lat_lon)
    assert low_res_lat_lon.shape[0] > 1 and low_res_lat_lon.shape[1] > 1, (
        'low res lat/lon must have at least 2 rows and 2 columns')
    logger.debug('Getting high resolution lat / lon grid')
    low_res_lat_lon[..., 1] = (low_res_lat_lon[..., 1] + 180) % 360 - 180
    if not is_increasing_lons(low_res_lat_lon):
        logger.debug('Ensuring increasing longitudes.')
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
    return np.dstack((lats.reshape(shape), lons.reshape(shape)))


def get_time_index_freqs(time_index):
    """preprocessing/utilities.py:141-170: the nominal frequency (the
    smallest step; one day for a single step) and all steps in seconds"""
    import pandas as pd
    unique_freqs = (list(set(np.diff(time_index))) if len(time_index) > 1
                    else [np.timedelta64(1, 'D')])
    unique_freqs /= np.timedelta64(1, 's')
    nominal_freq = pd.tseries.offsets.DateOffset(seconds=min(unique_freqs))
    return nominal_freq, unique_freqs


def get_times(low_res_times, shape):
    """OutputHandler.get_times (writers/base.py:510-551): ``shape`` steps at
    the low-res frequency over ``t_enhance``; 29 February only where the
    low-res index has it"""
    import pandas as pd
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
    assert len(times) == shape, (
        f'High res times length {len(times)} does not match expected '
        f'shape {shape}')
    return times


# ------------------------------------------------------------ the containers
class ExoInput:
    """In the place of the input handler: the low-res ``lat_lon`` ``(s1, s2,
    2)`` and ``time_index``.  ``target`` and ``grid_shape`` are what the
    cache file name carries."""

    def __init__(self, lat_lon, time_index):
        import pandas as pd
        self.lat_lon = np.asarray(lat_lon)
        self.time_index = (time_index if isinstance(time_index,
                                                    pd.DatetimeIndex)
                           else pd.DatetimeIndex(time_index))

    @classmethod
    def wrap(cls, obj):
        if isinstance(obj, cls):
            return obj
        if isinstance(obj, dict):
            return cls(obj['lat_lon'], obj['time_index'])
        return cls(obj.lat_lon, obj.time_index)

    @property
    def target(self):
        """the lower left corner, as the rasterizers report it"""
        return tuple(float(v) for v in self.lat_lon[-1, 0])

    @property
    def grid_shape(self):
        return tuple(int(v) for v in self.lat_lon.shape[:2])


class ExoSource:
    """In the place of the source files: ``lat_lon`` ``(..., 2)``, the values
    of each feature under its (lower case) name, shaped ``(...)`` or ``(...,
    T_src)``, and an optional ``time_index`` (needed for time-dependent
    features)."""

    def __init__(self, lat_lon, time_index=None, **features):
        import pandas as pd
        self.lat_lon = np.asarray(lat_lon)
        self.time_index = (None if time_index is None
                           else time_index if isinstance(time_index,
                                                         pd.DatetimeIndex)
                           else pd.DatetimeIndex(time_index))
        self.features = {k.lower(): v for k, v in features.items()}

    @classmethod
    def wrap(cls, obj):
        if isinstance(obj, cls):
            return obj
        if isinstance(obj, dict):
            rest = {k: v for k, v in obj.items()
                    if k not in ('lat_lon', 'time_index')}
            return cls(obj['lat_lon'], obj.get('time_index'), **rest)
        raise TypeError('the source must be an ExoSource or a mapping with '
                        '"lat_lon" and the feature\'s values')

    def __contains__(self, name):
        return name.lower() in self.features

    def __getitem__(self, name):
        return self.features[name.lower()]

    def has_time(self, name):
        """the values carry a time axis behind the axes of ``lat_lon``"""
        return np.ndim(self[name]) == self.lat_lon.ndim


class ExoRaster:
    """What ``ExoRasterizer.data`` returns: ``values``, the ``(lats, lons, T
    or 1)`` float32 field — a device tensor or numpy —, with ``coords`` beside
    it."""

    def __init__(self, feature, values, coords):
        self.feature, self.values, self.coords = feature, values, coords

    @property
    def shape(self):
        return tuple(int(v) for v in self.values.shape)

    @property
    def lat_lon(self):
        return np.dstack((self.coords['latitude'], self.coords['longitude']))

    @property
    def time_index(self):
        return self.coords.get('time')

    def as_array(self):
        """with the feature axis: ``(lats, lons, 1)`` for a field without a
        time axis, else ``(lats, lons, T, 1)``"""
        return self.values if 'time' not in self.coords \
            else self.values[..., None]

    def numpy(self):
        v = self.values
        return v.detach().cpu().numpy() if hasattr(v, 'detach') \
            else np.asarray(v)


# ----------------------------------------------------------------- backends
class NumpyBackend:
    """The device's rules restated in numpy: float64 squared distances on
    the widened float32 inputs, ``d2 < r * r`` strictly, the smallest target
    id among equal ``d2``; the mean of the non-NaN values in float64, times
    the scale, rounded once.  The candidates of a source are the ``K``
    nearest the KD-tree returns (a tie among more than ``K`` targets would
    escape it)."""

    name = 'numpy'
    K = 9

    def asarray(self, x):
        return np.ascontiguousarray(np.asarray(x, dtype=np.float32))

    def to_numpy(self, x):
        return np.asarray(x)

    def nearest(self, src, tgt, r):
        """``src`` (N, 2), ``tgt`` (M, 2) float32 -> handle of (nn, dists)"""
        from scipy.spatial import KDTree
        src64, tgt64 = src.astype(np.float64), tgt.astype(np.float64)
        m = len(tgt64)
        k = min(self.K, m)
        ok_t = np.isfinite(tgt64).all(axis=1)
        ok_s = np.isfinite(src64).all(axis=1)
        safe_t = np.where(ok_t[:, None], tgt64, 1e300)
        _, cand = KDTree(safe_t).query(np.where(ok_s[:, None], src64, 0.0),
                                       k=k)
        cand = cand.reshape(len(src64), k)
        d = src64[:, None, :] - tgt64[cand]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
        with np.errstate(invalid='ignore'):
            hit = d2 < float(r) * float(r)
        hit &= ok_s[:, None] & ok_t[cand]
        key_d2 = np.where(hit, d2, np.inf)
        best_d2 = key_d2.min(axis=1)
        tied = hit & (key_d2 == best_d2[:, None])
        nn = np.where(tied, cand, m).min(axis=1)
        dists = np.where(nn < m, np.sqrt(best_d2), np.inf)
        return nn.astype(np.int32), dists

    def nn_host(self, handle):
        return handle[0].astype(np.int64), handle[1]

    def hits(self, handle, m):
        return int((handle[0] != m).sum())

    def take_columns(self, values, cols):
        return np.ascontiguousarray(values[:, cols])

    def group_mean(self, handle, values, m, t_out, cols, scale):
        """-> ((m, t_out) float32, NaN where nothing was written, number of
        NaN cells)"""
        nn = handle[0].astype(np.int64)
        out = np.full((m, t_out), np.nan, dtype=np.float32)
        for k, col in enumerate(cols):
            x = values[:, k].astype(np.float64)
            ok = (nn >= 0) & (nn < m) & ~np.isnan(x)
            total = np.bincount(nn[ok], weights=x[ok], minlength=m)
            n = np.bincount(nn[ok], minlength=m)
            with np.errstate(all='ignore'):
                out[:, col] = np.where(n > 0, total / n * float(scale),
                                       np.nan).astype(np.float32)
        return out, lambda: int(np.isnan(out).sum())

    def nn_fill(self, field):
        from scipy import ndimage as nd
        indices = nd.distance_transform_edt(
            np.isnan(field), return_distances=False, return_indices=True)
        return field[tuple(indices)]


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class DeviceBackend:
    """The same through the C ABI, on device tensors.  A missing kernel is an
    error: nothing is routed to numpy or torch arithmetic (a field with an
    axis above ``S3_NN_FILL_MAX_AXIS`` is the one exception: its holes are
    filled by the host's scipy call, with a logged note)."""

    name = 'device'

    def __init__(self, dev=None):
        from .engine import Device
        self.dev = dev or Device.get()
        self._work = None

    def _call(self, name, *args):
        ctx = self.dev.ctx
        rc = getattr(_lib.lib(), name)(ctx, *args)
        if rc == -1:                                      # S3_EINVAL
            raise ValueError(f'{name}: {_lib.last_error(ctx)}')
        _lib.check(rc, ctx, name)

    def _workspace(self, n_bytes):
        import torch
        if self._work is None or self._work.numel() * 8 < n_bytes:
            self._work = torch.empty((int(n_bytes) + 7) // 8,
                                     dtype=torch.int64,
                                     device=self.dev.torch_device)
        return self._work

    def asarray(self, x):
        return self.dev.to_device(x)

    def to_numpy(self, x):
        return x.detach().cpu().numpy()

    def nearest(self, src, tgt, r):
        """the ids stay on the device; the float64 distances are computed
        (by a second query) only when somebody reads them"""
        import torch
        n, m = int(src.shape[0]), int(tgt.shape[0])
        nn = torch.empty(n, dtype=torch.int32, device=self.dev.torch_device)
        n_bytes = int(_lib.lib().s3_exo_nearest_work_bytes(m))
        if n_bytes < 0:
            raise ValueError('s3_exo_nearest: 1 .. 2^31 - 1 targets')
        work = self._workspace(n_bytes)
        self._call('s3_exo_nearest', _vp(src), n, _vp(tgt), m, float(r),
                   _vp(work), work.numel() * 8, _vp(nn), None)
        return {'nn': nn, 'src': src, 'tgt': tgt, 'r': float(r)}

    def nn_host(self, handle):
        import torch
        src, tgt = handle['src'], handle['tgt']
        n, m = int(src.shape[0]), int(tgt.shape[0])
        dist = torch.empty(n, dtype=torch.float64,
                           device=self.dev.torch_device)
        work = self._workspace(int(_lib.lib().s3_exo_nearest_work_bytes(m)))
        self._call('s3_exo_nearest', _vp(src), n, _vp(tgt), m, handle['r'],
                   _vp(work), work.numel() * 8, _vp(handle['nn']), _vp(dist))
        return (handle['nn'].cpu().numpy().astype(np.int64),
                dist.cpu().numpy())

    def hits(self, handle, m):
        return int((handle['nn'] != m).sum().item())

    def take_columns(self, values, cols):
        import torch
        if len(cols) == values.shape[1] and list(cols) == list(
                range(values.shape[1])):
            return values
        idx = torch.from_numpy(np.asarray(cols, np.int64)).to(values.device)
        return torch.index_select(values, 1, idx).contiguous()

    def group_mean(self, handle, values, m, t_out, cols, scale):
        import torch
        n, t_used = (int(v) for v in values.shape)
        td = self.dev.torch_device
        if t_used == t_out:
            out = torch.empty((m, t_out), dtype=torch.float32, device=td)
        else:
            out = torch.full((m, t_out), float('nan'), dtype=torch.float32,
                             device=td)
        count = torch.empty(1, dtype=torch.int64, device=td)
        n_bytes = int(_lib.lib().s3_exo_group_mean_work_bytes(m, t_used))
        work = self._workspace(n_bytes)
        col = np.ascontiguousarray(cols, dtype=np.int32)
        self._call('s3_exo_group_mean', _vp(handle['nn']), _vp(values), n, m,
                   t_used, t_out, col.ctypes.data_as(C.POINTER(C.c_int32)),
                   float(scale), _vp(work), work.numel() * 8, _vp(out),
                   _vp(count))
        untouched = m * (t_out - t_used)
        return out, lambda: int(count.item()) + untouched

    def nn_fill(self, field):
        """``(H, W, T)`` in place through ``s3_nn_fill`` as its block ``(n,
        s1, s2, t, C) = (H, W, T, 1, 1)``: scipy's distance and tie order"""
        import torch
        h, w, t = (int(v) for v in field.shape)
        if max(h, w, t) > _lib.NN_FILL_MAX_AXIS:
            logger.info('exo raster %s has an axis above %d: filling its '
                        'holes on the host', (h, w, t),
                        _lib.NN_FILL_MAX_AXIS)
            filled = NumpyBackend().nn_fill(self.to_numpy(field))
            return self.asarray(filled)
        work = self._workspace(8 * h * w * t)
        count = torch.empty(1, dtype=torch.int32,
                            device=self.dev.torch_device)
        self._call('s3_nn_fill', _vp(field), h, w, t, 1, 1, 0, _vp(work),
                   _vp(count))
        return field


def default_backend(device=None):
    """the device backend where a GPU is present (``device`` None or True),
    else the numpy one"""
    if device is None:
        import torch
        device = torch.cuda.is_available()
    if device is False:
        return NumpyBackend()
    return DeviceBackend(None if device is True else device)


# ------------------------------------------------------------- rasterizers
@dataclass
class BaseExoRasterizer:
    """rasterizers/exo.py:34-458 over arrays.

    ``file_paths``: an :class:`ExoInput` (object or mapping with ``lat_lon``
    and ``time_index``); ``source_files``: an :class:`ExoSource` (or mapping).
    ``device``: True / a ``Device`` for the device backend, False for numpy,
    None for the device where a GPU is present; ``backend`` overrides it.
    ``shared``: a dict that several rasterizers of one source use to share
    its upload (``ExoDataHandler`` passes one)."""

    feature: Optional[str] = None
    file_paths: Optional[object] = None
    source_files: Optional[object] = None
    source_handler_kwargs: Optional[dict] = None
    s_enhance: int = 1
    t_enhance: int = 1
    input_handler_name: Optional[str] = None
    input_handler_kwargs: Optional[dict] = None
    cache_dir: Optional[str] = None
    chunks: Optional[object] = 'auto'
    distance_upper_bound: Optional[float] = None
    fill_nans: bool = True
    scale_factor: float = 1.0
    max_workers: int = 1
    device: Optional[object] = None
    backend: Optional[object] = None
    shared: Optional[dict] = None

    STATIC_FEATURES: ClassVar = ('topography', 'srl')

    def __post_init__(self):
        self._source_data = None
        self._source_handler = None
        self._hr_lat_lon = None
        self._source_lat_lon = None
        self._hr_time_index = None
        self._nn = None
        self._dists = None
        self._handle = None
        self.input_handler_kwargs = self.input_handler_kwargs or {}
        self.source_handler_kwargs = self.source_handler_kwargs or {}
        self.input_handler = ExoInput.wrap(self.file_paths)
        if self.backend is None:
            self.backend = default_backend(self.device)
        if self.shared is None:
            self.shared = {}
        if self.cache_dir is not None or self.max_workers != 1 or \
                self.chunks != 'auto':
            logger.info('cache_dir, chunks and max_workers are accepted and '
                        'ignored: nothing is cached or chunked here')

    # -- the source
    @property
    def source_name(self):
        """the name the source holds the feature under"""
        return self.feature.lower()

    @property
    def source_handler(self):
        assert self.source_files is not None, (
            'source_files must be provided to BaseExoRasterizer')
        if self._source_handler is None:
            self._source_handler = ExoSource.wrap(self.source_files)
        return self._source_handler

    def _host_source_data(self):
        src = self.source_handler
        data = np.asarray(src[self.source_name], dtype=np.float32)
        if not src.has_time(self.source_name):
            data = data[..., None]
        elif self.feature in self.STATIC_FEATURES:
            data = data[..., :1]
        return data.reshape((-1, data.shape[-1]))

    def _uploaded(self, key, make):
        key = (self.backend.name, key)
        if key not in self.shared:
            self.shared[key] = self.backend.asarray(make())
        return self.shared[key]

    @property
    def source_data(self):
        """``(n, T_src)`` float32 with the backend: uploaded once per source
        (``shared``)"""
        if self._source_data is None:
            self._source_data = self._uploaded(
                ('data', self.source_name, self.feature in
                 self.STATIC_FEATURES), self._host_source_data)
        return self._source_data

    @property
    def source_lat_lon(self):
        """``(n, 2)`` float32 lat, lon of the source, on the host"""
        if self._source_lat_lon is None:
            self._source_lat_lon = np.asarray(
                self.source_handler.lat_lon).reshape((-1, 2)).astype(
                    np.float32)
        return self._source_lat_lon

    # -- the target
    @property
    def cache_file(self):
        """the reference's cache file name under ``cache_dir`` (None without
        one); nothing is written there"""
        fn = f'exo_{self.feature}_'
        fn += f'{"_".join(map(str, self.input_handler.target))}_'
        fn += f'{"x".join(map(str, self.input_handler.grid_shape))}_'
        if self.source_data.shape[-1] > 1:
            start = str(self.hr_time_index[0])
            start = start.replace(':', '').replace('-', '').replace(' ', '')
            end = str(self.hr_time_index[-1])
            end = end.replace(':', '').replace('-', '').replace(' ', '')
            fn += f'{start}_{end}_'
        fn += f'{self.s_enhance}x_{self.t_enhance}x.nc'
        if self.cache_dir is None:
            return None
        return os.path.join(self.cache_dir, fn)

    @property
    def coords(self):
        coords = {'latitude': self.hr_lat_lon[..., 0],
                  'longitude': self.hr_lat_lon[..., 1]}
        if self.source_data.shape[1] > 1:
            coords['time'] = self.hr_time_index
        return coords

    @property
    def lr_shape(self):
        return (*self.input_handler.lat_lon.shape[:2],
                len(self.input_handler.time_index))

    @property
    def hr_shape(self):
        return (self.s_enhance * self.input_handler.lat_lon.shape[0],
                self.s_enhance * self.input_handler.lat_lon.shape[1],
                self.t_enhance * len(self.input_handler.time_index))

    @property
    def hr_lat_lon(self):
        """``(s1 s_enhance, s2 s_enhance, 2)`` float32"""
        if self._hr_lat_lon is None:
            ll = (get_lat_lon(self.input_handler.lat_lon, self.hr_shape[:-1])
                  if self.s_enhance > 1 else self.input_handler.lat_lon)
            self._hr_lat_lon = np.ascontiguousarray(ll, dtype=np.float32)
        return self._hr_lat_lon

    @property
    def hr_time_index(self):
        if self._hr_time_index is None:
            self._hr_time_index = (
                get_times(self.input_handler.time_index, self.hr_shape[-1])
                if self.t_enhance > 1 else self.input_handler.time_index)
        return self._hr_time_index

    def get_distance_upper_bound(self):
        """the bound of the mapping; by default the largest median spacing of
        the rows of ``hr_lat_lon`` (host numpy)"""
        if self.distance_upper_bound is None:
            assert self.hr_lat_lon.shape[0] > 1, (
                'hr_lat_lon must have at least 2 lat points to calculate '
                'distance upper bound. Either expand the grid or provide a '
                'distance_upper_bound explicitly.')
            diff = np.diff(self.hr_lat_lon, axis=0)
            diff = np.abs(np.median(diff, axis=0)).max()
            self.distance_upper_bound = np.asarray(diff)
            logger.info('Set distance upper bound to {:.4f}'.format(
                self.distance_upper_bound))
        return self.distance_upper_bound

    # -- the nearest-neighbour work
    def _nearest(self):
        """the backend's handle of the query (the ids stay where they are)"""
        if self._handle is None:
            key = ('nearest', self.s_enhance, id(self.source_handler),
                   float(self.get_distance_upper_bound()))
            skey = (self.backend.name, key)
            if skey not in self.shared:
                src = self._uploaded(('lat_lon',),
                                     lambda: self.source_lat_lon)
                tgt = self.backend.asarray(self.hr_lat_lon.reshape((-1, 2)))
                self.shared[skey] = self.backend.nearest(
                    src, tgt, float(self.get_distance_upper_bound()))
            self._handle = self.shared[skey]
        return self._handle

    def _download_nn(self):
        if self._nn is None:
            self._nn, self._dists = self.backend.nn_host(self._nearest())

    @property
    def nn(self):
        """host array as scipy returns it: ``n_target`` for a miss"""
        self._download_nn()
        return self._nn

    @property
    def dists(self):
        """host array as scipy returns it: ``inf`` for a miss"""
        self._download_nn()
        return self._dists

    # -- the field
    @property
    def data(self):
        """:class:`ExoRaster` of the ``(lats, lons, T or 1)`` float32 field"""
        return self.get_data()

    def get_data(self):
        assert len(self.source_data.shape) == 2
        if self.source_data.shape[1] == 1:
            hr_data, n_nan = self._get_data_2d()
        else:
            hr_data, n_nan = self._get_data_3d()
        # (scale_factor is applied with the mean)
        if self.fill_nans:
            count = n_nan()
            if count:
                msg = (f'{count} target pixels did not have unique '
                       f'high-resolution {self.feature} source data to map '
                       'from. If there are a lot of target pixels missing '
                       'source data this probably means the source data is '
                       'not high enough resolution. Filling raster with NN.')
                logger.warning(msg)
                warn(msg)
                hr_data = self.backend.nn_fill(hr_data)
        logger.info('Finished mapping raster for "%s"', self.feature)
        return ExoRaster(self.feature, hr_data, self.coords)

    def _group_mean(self, values, t_out, cols):
        n_target = int(np.prod(self.hr_shape[:-1]))
        out, n_nan = self.backend.group_mean(
            self._nearest(), values, n_target, t_out, cols,
            self.scale_factor)
        return out.reshape((*self.hr_shape[:-1], t_out)), n_nan

    def _get_data_2d(self):
        """time-independent data: ``(lats, lons, 1)`` and the NaN count"""
        assert (len(self.source_data.shape) == 2
                and self.source_data.shape[1] == 1)
        return self._group_mean(self.source_data, 1, [0])

    def _get_data_3d(self):
        """``(lats, lons, time)``: the source steps whose time is in
        ``hr_time_index`` go to the matching target steps, the other target
        steps stay NaN (no time aggregation, as in the reference)"""
        src_ti = self.source_handler.time_index
        assert src_ti is not None, (
            f'the source of "{self.feature}" has a time axis and needs a '
            'time_index')
        target_tmask = np.asarray(self.hr_time_index.isin(src_ti))
        source_tmask = np.asarray(src_ti.isin(self.hr_time_index))
        cols = np.flatnonzero(target_tmask)
        used = np.flatnonzero(source_tmask)
        if len(cols) != len(used):
            raise ValueError(
                f'{len(used)} source steps match {len(cols)} target steps: '
                'the time indices must not repeat a step')
        t_out = len(self.hr_time_index)
        if len(used) == 0:
            n_target = int(np.prod(self.hr_shape[:-1]))
            out = self.backend.asarray(np.full(
                (*self.hr_shape[:-1], t_out), np.nan, dtype=np.float32))
            return out, lambda: n_target * t_out
        data = self.backend.take_columns(self.source_data, used)
        return self._group_mean(data, t_out, cols)


class ObsRasterizer(BaseExoRasterizer):
    """rasterizers/exo.py:461-528: sparse observations — NaN stays where no
    observation lies within the bound.  The feature carries an ``_obs``
    suffix, the source holds it without."""

    @property
    def source_name(self):
        return self.feature.lower().replace('_obs', '')

    def _host_source_data(self):
        src = np.asarray(self.source_handler[self.source_name],
                         dtype=np.float32)
        return src.reshape((-1, src.shape[-1]))

    def _get_data_3d(self):
        hr_data, n_nan = super()._get_data_3d()
        size = int(np.prod(hr_data.shape))
        cover_frac = (size - n_nan()) / size
        if cover_frac == 0:
            msg = ('No observations found within the distance upper bound of '
                   f'{self.distance_upper_bound} degrees. ')
            warn(msg)
            logger.warning(msg)
        elif logger.isEnabledFor(logging.INFO):
            n_target = int(np.prod(self.hr_shape[:-1]))
            n_src = len(self.source_lat_lon)
            msg = (f'Found {self.backend.hits(self._nearest(), n_target)} of '
                   f'{n_src} observations within '
                   f'{float(self.distance_upper_bound):4f} degrees of '
                   'high-resolution grid points. Observations cover '
                   f'{cover_frac:.4e} of the high-res domain.')
            logger.info(msg)
        self.fill_nans = False  # override parent attribute to not fill nans
        return hr_data, n_nan


class SzaRasterizer(BaseExoRasterizer):
    """rasterizers/exo.py:531-547: needs rex's ``SolarPosition``"""

    @property
    def source_data(self):
        raise NotImplementedError(
            'sza needs SolarPosition of the rex package '
            '(rex.utilities.solar_position), which this package does not '
            'carry: pass the zenith angle as exo_data')

    def get_data(self):
        return self.source_data


class ExoRasterizer(BaseExoRasterizer):
    """Type agnostic ``ExoRasterizer`` (rasterizers/exo.py:550-573): returns
    the class the feature name selects."""

    def __new__(cls, feature, file_paths, source_files=None, **kwargs):
        if feature.lower() == 'sza':
            ExoClass = SzaRasterizer
        elif feature.lower().endswith('_obs'):
            ExoClass = ObsRasterizer
        else:
            ExoClass = BaseExoRasterizer
        kwargs = {'file_paths': file_paths, 'source_files': source_files,
                  'feature': feature, **kwargs}
        return ExoClass(**kwargs)


# ---------------------------------------------------------------- the handler
class SingleExoDataStep(dict):
    """data_handlers/exo.py:20-50: one step of one feature"""

    def __init__(self, feature, combine_type, model, data):
        step = {'model': model, 'combine_type': combine_type, 'data': data}
        for k, v in step.items():
            self.__setitem__(k, v)
        self.feature = feature

    @property
    def shape(self):
        return tuple(self['data'].shape)


class ExoDataHandler:
    """data_handlers/exo.py:276-498: the fields of one exogenous feature for
    every model step that uses it.  ``.data`` is what ``ExoData(...)`` and
    ``ArrayStrategy(exo_data=...)`` take."""

    def __init__(self, feature, file_paths, model=None, steps=None,
                 **exo_rasterizer_kwargs):
        self.feature = feature
        self.file_paths = file_paths
        self.model = model
        self.steps = steps
        self.exo_rasterizer_kwargs = exo_rasterizer_kwargs
        self.models = getattr(self.model, 'models', [self.model])
        self._shared = exo_rasterizer_kwargs.pop('shared', None) or {}
        self._step_data = {}
        if 'backend' not in self.exo_rasterizer_kwargs:
            self.exo_rasterizer_kwargs['backend'] = default_backend(
                self.exo_rasterizer_kwargs.pop('device', None))
        if self.exo_rasterizer_kwargs.get('source_files') is not None:
            self.exo_rasterizer_kwargs['source_files'] = ExoSource.wrap(
                self.exo_rasterizer_kwargs['source_files'])

        if self.steps is None:
            self.steps = self.get_exo_steps(self.feature, self.models)
        else:
            en_check = all('s_enhance' in v for v in self.steps)
            en_check = en_check and all('t_enhance' in v for v in self.steps)
            en_check = en_check or self.models is not None
            msg = (f'{self.__class__.__name__} needs s_enhance and t_enhance '
                   'provided in each step in steps list or models')
            assert en_check, msg
        self.s_enhancements, self.t_enhancements = self._get_all_enhancement()
        self.data = self.get_all_step_data()

    @classmethod
    def get_exo_steps(cls, feature, models):
        """the steps that use the feature: 'input' where it is a low-res
        feature (or the model is a ``SurfaceSpatialMetModel``), 'layer' where
        it is a high-res exo or an obs feature, 'output' where it is an
        output feature (or the surface model)"""
        steps = []
        for i, model in enumerate(models):
            is_sfc_model = model.__class__.__name__ == 'SurfaceSpatialMetModel'
            obs_features = getattr(model, 'obs_features', [])
            if feature.lower() in _lowered(model.lr_features) or is_sfc_model:
                steps.append({'model': i, 'combine_type': 'input'})
            if feature.lower() in _lowered(model.hr_exo_features):
                steps.append({'model': i, 'combine_type': 'layer'})
            if feature.lower() in _lowered(obs_features):
                steps.append({'model': i, 'combine_type': 'layer'})
            if (feature.lower() in _lowered(model.hr_out_features)
                    or is_sfc_model):
                steps.append({'model': i, 'combine_type': 'output'})
        return steps

    def get_exo_rasterizer(self, s_enhance, t_enhance):
        return ExoRasterizer(s_enhance=s_enhance, t_enhance=t_enhance,
                             feature=self.feature, file_paths=self.file_paths,
                             shared=self._shared,
                             **self.exo_rasterizer_kwargs)

    def get_single_step_data(self, s_enhance, t_enhance):
        """the raster at the given factors; steps that share them share it"""
        key = (int(s_enhance), int(t_enhance))
        if key not in self._step_data:
            self._step_data[key] = self.get_exo_rasterizer(
                s_enhance, t_enhance).data
        return self._step_data[key]

    @property
    def cache_files(self):
        return [self.get_exo_rasterizer(s_en, t_en).cache_file
                for s_en, t_en in zip(self.s_enhancements,
                                      self.t_enhancements)]

    def get_all_step_data(self):
        data = {self.feature: {'steps': []}}
        for i, (s_enhance, t_enhance) in enumerate(
                zip(self.s_enhancements, self.t_enhancements)):
            step_data = self.get_single_step_data(s_enhance=s_enhance,
                                                  t_enhance=t_enhance)
            step = SingleExoDataStep(
                self.feature, self.steps[i]['combine_type'],
                self.steps[i]['model'], data=step_data.as_array())
            step['s_enhance'] = s_enhance
            step['t_enhance'] = t_enhance
            data[self.feature]['steps'].append(step)
        shapes = [None if step is None else step.shape
                  for step in data[self.feature]['steps']]
        logger.info('Got exogenous_data of length {} with shapes: {}'.format(
            len(data[self.feature]['steps']), shapes))
        return data

    def _get_single_step_enhance(self, step):
        """the step with ``s_enhance`` / ``t_enhance``: its own where it
        carries both; else, for an 'input' step, the product of the
        enhancements before the model, for 'layer' and 'output' including
        it"""
        if all(key in step for key in ['s_enhance', 't_enhance']):
            return step
        mstep = step['model']
        combine_type = step.get('combine_type', None)
        msg = (f'Model index from exo_kwargs ({mstep} exceeds number '
               f'of model steps ({len(self.models)})')
        assert len(self.models) > mstep, msg
        msg = ('Received exo_kwargs entry without valid combine_type '
               '(input/layer/output)')
        assert combine_type.lower() in ('input', 'output', 'layer'), msg
        if combine_type.lower() == 'input':
            if mstep == 0:
                s_enhance = 1
                t_enhance = 1
            else:
                s_enhance = int(np.prod(self.model.s_enhancements[:mstep]))
                t_enhance = int(np.prod(self.model.t_enhancements[:mstep]))
        else:
            s_enhance = int(np.prod(self.model.s_enhancements[: mstep + 1]))
            t_enhance = int(np.prod(self.model.t_enhancements[: mstep + 1]))
        step.update({'s_enhance': s_enhance, 't_enhance': t_enhance})
        return step

    def _get_all_enhancement(self):
        for i, step in enumerate(self.steps):
            self.steps[i] = self._get_single_step_enhance(step)
        s_enhancements = [step['s_enhance'] for step in self.steps]
        t_enhancements = [step['t_enhance'] for step in self.steps]
        return s_enhancements, t_enhancements


def _lowered(features):
    """preprocessing/utilities.py:555-575 (warns about upper case names)"""
    return lowered(list(features))
