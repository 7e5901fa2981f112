"""Data handlers on the device: ``sup3r.preprocessing.data_handlers`` and the
rasterizers under them.

The reference puts its data handlers (data_handlers/base.py, nc_cc.py over
rasterizers/base.py, extended.py) between the deriver and the samplers: they
cut the training region and period out of the source, derive the features,
and — the CC handlers — build the daily cube the CC samplers pair with the
hourly one.  The classes here keep the reference's constructors and control
flow and work over arrays in the place of files:

``DeviceRasterizer`` (``Rasterizer``, ``BaseRasterizer``)
    ``target`` / ``shape`` / ``time_slice`` / ``threshold`` over a
    :class:`~sup3r_amd.derive.DeriveData` (gridded planes ``(s1, s2, t)``,
    multi-level ``(s1, s2, t, L)``, 2-D ``topography``), or ``raster_index`` /
    ``raster_file`` over a :class:`FlatData`, the flattened time-first layout
    of WTK / NSRDB H5 data: ``(T, n_sites)`` arrays plus 1-D ``(n_sites,)``
    ones.  The result is a ``DeriveData`` on the raster, bound to the backend.
``DeviceDataHandler`` (``DataHandler``)
    rasterise, ``_rasterizer_hook()``, derive (``DeviceDeriver``, which it
    subclasses), ``_deriver_hook()``.
``DailyDataHandler``, ``DataHandlerH5SolarCC``, ``DataHandlerH5WindCC``
    the daily cube: 24-hour means, maxima of ``*_max_*``, minima of
    ``*_min_*``, sums for ``total_*``, ``clearsky_ratio = total_ghi /
    total_clearsky_ghi``.  ``handler.daily`` / ``handler.hourly`` are the
    ``(S1, S2, T, C)`` cubes of ``requested_features``, stacked once and kept;
    with ``lr_features`` / ``hr_features`` beside them a handler is a
    container of ``DeviceBatchHandlerCC.from_containers`` (which normalises
    the two cubes in place) and unpacks into ``DeviceDualSamplerCC``.
``DataHandlerNCforCC``, ``DataHandlerNCforCCwithPowerLaw``
    ``clearsky_ghi`` from an NSRDB source (the k nearest sites, their mean,
    the daily mean, the ``'%m.%d'`` re-index) and its scaling to the
    per-pixel maximum of ``rsds``.

The arithmetic is four methods of the backends of ``derive.py``
(``raster_gather``, ``daily_reduce``, ``site_day_mean``,
``scale_to_time_max``): on ``DeviceBackend`` four entry points of
csrc/kernels_data_handler.hip, on ``NumpyBackend`` numpy, for testing the host
control flow without a GPU (``backend=NumpyBackend()``; nothing selects it but
the caller).

NaN semantics.  ``xr.Dataset.coarsen(...).mean() / .max() / .min() / .sum()``
and ``.max(dim='time')`` on float data skip NaN (``skipna=None`` picks the
``nan*`` functions for dtype kind ``f``): an all-NaN window gives a NaN mean,
maximum and minimum, a sum of 0 and a ratio of 0 / 0 = NaN.  This reading is
UNVERIFIED against xarray, which was not at hand when this was written;
``samplers_cc.coarsen_daily`` rests on the same reading.  Means and sums are
accumulated in float64 and rounded to float32 once, which xarray does not
promise either way.

Choices where the reference gave none, and deviations:
  * ``cache_kwargs``, ``chunks``, ``res_kwargs`` and ``BaseLoader`` are
    accepted and ignored, with one debug line;
  * as in the reference the deriver's constructor runs whenever ``features``
    is not empty — ``features='all'`` derives nothing, yet ``time_roll`` and
    the like apply — and not at all for ``features=[]`` (coordinates only);
  * a ``time_slice`` with a negative step is a ``ValueError``;
  * the daily ``time_index`` is the mean stamp of each window, which is what
    ``coarsen`` makes of a coordinate (11:30 for hourly data from 00:00);
  * ``handler.totals`` keeps ``total_ghi`` / ``total_clearsky_ghi`` (the
    reference drops them with ``daily_data[requested_features]``);
  * ``nsrdb_source_fp`` is a ``FlatData`` holding ``clearsky_ghi``, or the
    path of an ``.npz`` file of one (``FlatData.save`` / ``FlatData.load``);
  * ``nsrdb_smoothing`` is stored and unused, as in the reference.

Out of scope: reading h5 / NetCDF, ``Cacher`` / ``cache_kwargs``, dask
chunking; rex's ``get_raster_index`` (``target`` + ``shape`` on flat data
raises ``NotImplementedError``); ``Sza`` and ``interpolate_na``, which stay
``NotImplementedError``; the k-NN query of ``DataHandlerNCforCC`` on the device (``scipy.spatial.KDTree`` on the host, as the reference
calls it: the targets are a coarse GCM grid); fusing ``coarsen_daily`` into
the reduction.
"""
import logging
import os
from warnings import warn

import numpy as np

from .derive import (DeriveData, DeviceBackend, DeviceDeriver,
                     RegistryH5SolarCC, RegistryH5WindCC, RegistryNCforCC,
                     RegistryNCforCCwithPowerLaw, lowered)

logger = logging.getLogger(__name__)

__all__ = ['FlatData', 'DeviceRasterizer', 'Rasterizer', 'BaseRasterizer',
           'DeviceDataHandler', 'DataHandler', 'DailyDataHandler',
           'DataHandlerH5SolarCC', 'DataHandlerH5WindCC',
           'DataHandlerNCforCC', 'DataHandlerNCforCCwithPowerLaw']


# ---------------------------------------------------------------- utilities
def _parse_time_slice(value):
    """preprocessing/utilities.py:280-289"""
    return (value if isinstance(value, slice)
            else slice(*value) if isinstance(value, (tuple, list))
            else slice(None))


def parse_to_list(features=None):
    """preprocessing/utilities.py:497-510 without a dataset: a flat list,
    lower case; ``'all'`` stays ``['all']``, None is ``[]``"""
    if features is None:
        return []
    if isinstance(features, (set, tuple)):
        features = list(features)
    if not isinstance(features, list):
        features = [features]
    return lowered(np.array(features).flatten().tolist())


def _time_index(ti):
    import pandas as pd
    return ti if isinstance(ti, pd.DatetimeIndex) else pd.DatetimeIndex(ti)


def time_step_seconds(time_index):
    """``Sup3rX.time_step`` (accessor.py:502-505): the most common step in
    seconds, the smallest of them on a tie (scipy's ``mode``)"""
    sec = np.asarray((time_index[1:] - time_index[:-1]).total_seconds())
    values, counts = np.unique(sec, return_counts=True)
    return float(values[np.argmax(counts)])


def _on(backend, x):
    """``x`` on the backend: uploaded unless it lives there already"""
    if backend.name == 'device' and hasattr(x, 'data_ptr'):
        return x
    return backend.asarray(x)


def _dataset(backend, arrays, lat_lon, time_index, **kwargs):
    """a ``DeriveData`` of arrays that are on the backend already"""
    out = DeriveData({}, lat_lon, time_index, **kwargs)
    out.backend = backend
    out._arrays = dict(arrays)
    return out


class FlatData:
    """Flattened time-first data in the place of a WTK / NSRDB H5 file:
    ``arrays`` maps a name to ``(T, n_sites)`` float32, or ``(n_sites,)``
    for a feature without a time axis; ``meta_lat_lon`` is ``(n_sites, 2)``."""

    flattened = True

    def __init__(self, arrays, meta_lat_lon, time_index, attrs=None):
        self._arrays = {k.lower(): v for k, v in dict(arrays).items()}
        self.lat_lon = np.asarray(meta_lat_lon)
        self.time_index = _time_index(time_index)
        self.attrs = {k.lower(): dict(v) for k, v in (attrs or {}).items()}
        self.level = self.height = None
        assert self.lat_lon.ndim == 2 and self.lat_lon.shape[1] == 2, (
            f'meta_lat_lon is (n_sites, 2), not {self.lat_lon.shape}')
        for name, a in self._arrays.items():
            ok = (tuple(a.shape) in ((len(self.time_index), len(self.lat_lon)),
                                     (len(self.lat_lon),)))
            assert ok, (f'{name} is {tuple(a.shape)}: neither (T, n_sites) '
                        'nor (n_sites,)')

    @property
    def features(self):
        return list(self._arrays)

    data_vars = features

    def __contains__(self, name):
        return name.lower() in self._arrays

    def __getitem__(self, name):
        return self._arrays[name.lower()]

    def __setitem__(self, name, value):
        self._arrays[name.lower()] = value

    @property
    def time_step(self):
        return time_step_seconds(self.time_index)

    def save(self, path):
        """an ``.npz`` file :meth:`load` reads"""
        arrays = {k: (v.detach().cpu().numpy() if hasattr(v, 'detach')
                      else np.asarray(v)) for k, v in self._arrays.items()}
        np.savez(path, meta_lat_lon=self.lat_lon,
                 time_index=self.time_index.values, **arrays)

    @classmethod
    def load(cls, path):
        with np.load(path) as f:
            arrays = {k: f[k] for k in f.files
                      if k not in ('meta_lat_lon', 'time_index')}
            return cls(arrays, f['meta_lat_lon'], f['time_index'])


# --------------------------------------------------------------- rasterizer
class DeviceRasterizer:
    """``Rasterizer`` (rasterizers/extended.py:19-206 over ``BaseRasterizer``,
    base.py:17-231) with a ``DeriveData`` or a ``FlatData`` in the place of
    ``file_paths``."""

    def __init__(self, source, features='all', target=None, shape=None,
                 time_slice=slice(None), threshold=None, raster_file=None,
                 raster_index=None, feature_aliases=None, device=None,
                 backend=None):
        logger.info('Rasterizing features: %s', features)
        self.backend = backend or DeviceBackend(device)
        self.loader = self.source = source
        self.flattened = bool(getattr(source, 'flattened', False))
        self.raster_file = raster_file
        self._given_index = raster_index
        self.feature_aliases = {k.lower(): v.lower() for k, v in
                                (feature_aliases or {}).items()}
        self.threshold = threshold
        self.time_slice = time_slice
        self.grid_shape = shape
        self.target = target
        self.full_lat_lon = np.asarray(source.lat_lon)
        self.raster_index = self.get_raster_index()
        self.time_index = source.time_index[self.time_slice]
        self._lat_lon = None
        self.data = self.rasterize_data(features)
        if self.raster_file is not None and not os.path.exists(
                self.raster_file):
            self.save_raster_index()

    # -- the reference's properties (base.py:83-129)
    @property
    def time_slice(self):
        return self._time_slice

    @time_slice.setter
    def time_slice(self, value):
        self._time_slice = _parse_time_slice(value)

    @property
    def target(self):
        """the coordinate the raster's lower left corner landed on"""
        return np.asarray(self.lat_lon[-1, 0])

    @target.setter
    def target(self, value):
        self._target = np.asarray(value) if value is not None else None

    @property
    def grid_shape(self):
        return self.lat_lon.shape[:-1]

    @grid_shape.setter
    def grid_shape(self, value):
        self._grid_shape = value

    @property
    def lat_lon(self):
        if self._lat_lon is None:
            self._lat_lon = self.get_lat_lon()
        return self._lat_lon

    @property
    def features(self):
        return self.data.features

    def __contains__(self, name):
        return name in self.data

    def __getitem__(self, name):
        return self.data[name]

    # -- the raster index (base.py:143-226, extended.py:156-191)
    def check_target_and_shape(self, full_lat_lon):
        if self._target is None:
            self._target = full_lat_lon[-1, 0, :]
        if self._grid_shape is None:
            self._grid_shape = full_lat_lon.shape[:-1]

    def get_raster_index(self):
        logger.info('Getting raster index for target / shape: %s / %s',
                    np.asarray(self._target), np.asarray(self._grid_shape))
        if self.flattened:
            return self._get_flat_data_raster_index()
        self.check_target_and_shape(self.full_lat_lon)
        row, col = self.get_closest_row_col(self.full_lat_lon, self._target)
        lat_slice = slice(row - self._grid_shape[0] + 1, row + 1)
        lon_slice = slice(col, col + self._grid_shape[1])
        return self._check_raster_index(lat_slice, lon_slice)

    def _check_raster_index(self, lat_slice, lon_slice):
        lat_start, lat_end = lat_slice.start, lat_slice.stop
        lon_start, lon_end = lon_slice.start, lon_slice.stop
        lat_start = max(lat_start, 0)
        lat_end = min(lat_end, self.full_lat_lon.shape[0])
        lon_start = max(lon_start, 0)
        lon_end = min(lon_end, self.full_lat_lon.shape[1])
        new_lat_slice = slice(lat_start, lat_end)
        new_lon_slice = slice(lon_start, lon_end)
        msg = (f'Computed lat_slice = {lat_slice} exceeds available region. '
               f'Using {new_lat_slice}.')
        if lat_slice != new_lat_slice:
            logger.warning(msg)
            warn(msg)
        msg = (f'Computed lon_slice = {lon_slice} exceeds available region. '
               f'Using {new_lon_slice}.')
        if lon_slice != new_lon_slice:
            logger.warning(msg)
            warn(msg)
        return new_lat_slice, new_lon_slice

    def get_closest_row_col(self, lat_lon, target):
        dist = np.hypot(lat_lon[..., 0] - target[0],
                        lat_lon[..., 1] - target[1])
        row, col = np.unravel_index(np.argmin(dist, axis=None), dist.shape)
        msg = ('The distance between the closest coordinate: '
               f'{np.asarray(lat_lon[row, col])} and the requested '
               f'target: {np.asarray(target)} is {np.asarray(dist.min())}. ')
        if self.threshold is not None and dist.min() > self.threshold:
            add_msg = f'This exceeds the given threshold: {self.threshold}'
            logger.error(f'{msg} {add_msg}')
            raise RuntimeError(f'{msg} {add_msg}')
        logger.info(msg)
        return int(row), int(col)

    def _get_flat_data_raster_index(self):
        if self._given_index is not None:
            raster_index = np.asarray(self._given_index).astype(np.int32)
        elif self.raster_file is None or not os.path.exists(self.raster_file):
            msg = ('Either shape + target or a raster_file must be provided '
                   'for flattened data rasterization.')
            assert (self._target is not None
                    and self._grid_shape is not None), msg
            raise NotImplementedError(
                'target + shape on flattened data needs get_raster_index of '
                'the rex package (rex.resource_extraction), which is not '
                'reproducible here: pass raster_index= or a raster_file')
        else:
            raster_index = np.loadtxt(self.raster_file).astype(np.int32)
            logger.info(f'Loaded raster_index from {self.raster_file}')
        if raster_index.ndim != 2:
            raise ValueError('raster_index is a 2-D array of site numbers, '
                             f'not {raster_index.shape}')
        n_sites = len(self.full_lat_lon)
        if raster_index.min() < 0 or raster_index.max() >= n_sites:
            raise IndexError(f'raster_index outside the {n_sites} sites')
        return raster_index

    def save_raster_index(self):
        folder = os.path.dirname(self.raster_file)
        if folder:
            os.makedirs(folder, exist_ok=True)
        index = (self.raster_index if self.flattened else np.array(
            [[s.start, s.stop] for s in self.raster_index]))
        np.savetxt(self.raster_file, index)
        logger.info(f'Saved raster_index to {self.raster_file}')

    def get_lat_lon(self):
        if self.flattened:
            return self.full_lat_lon[self.raster_index]
        return self.full_lat_lon[self.raster_index[0], self.raster_index[1]]

    # -- the data (base.py:131-141, extended.py:122-154)
    def _steps(self):
        """the slice as ``(t0, step, n_k)``"""
        r = range(*self.time_slice.indices(len(self.source.time_index)))
        if r.step < 1:
            raise ValueError(f'time_slice {self.time_slice}: a negative step '
                             'is not rasterised')
        if len(r) == 0:
            raise ValueError(f'time_slice {self.time_slice} selects nothing '
                             f'of {len(self.source.time_index)} steps')
        return r.start, r.step, len(r)

    def rasterize_data(self, features='all'):
        logger.info('Rasterizing data for target / shape: %s / %s',
                    np.asarray(self._target), np.asarray(self._grid_shape))
        be, src = self.backend, self.source
        named = {self.feature_aliases.get(f, f): f for f in src.features}
        if isinstance(features, str) and features != 'all':
            features = [features]
        wanted = (list(named) if features == 'all'
                  else lowered(list(features)))
        missing = [f for f in wanted if f not in named]
        if missing:
            raise KeyError(f'{missing} not in the source: {list(named)}')
        arrays = [_on(be, src[named[f]]) for f in wanted]
        t0, step, n_k = self._steps()
        if self.flattened:
            planes = be.raster_gather(arrays, t0=t0, step=step, n_k=n_k,
                                      site=self.raster_index)
        else:
            planes = be.raster_gather(arrays, rows=self.raster_index[0],
                                      cols=self.raster_index[1], t0=t0,
                                      step=step, n_k=n_k)
        attrs = {f: src.attrs[named[f]] for f in wanted
                 if named[f] in src.attrs}
        return _dataset(be, zip(wanted, planes), self.lat_lon,
                        self.time_index, level=src.level, height=src.height,
                        attrs=attrs)


Rasterizer = BaseRasterizer = DeviceRasterizer


# ------------------------------------------------------------- data handlers
class DeviceDataHandler(DeviceDeriver):
    """``DataHandler`` (data_handlers/base.py:46-290) over a source in the
    place of ``file_paths``; ``kwargs`` (``raster_file``, ``raster_index``)
    go to the rasterizer."""

    def __init__(self, source, features='all', load_features='all',
                 res_kwargs=None, chunks='auto', target=None, shape=None,
                 time_slice=slice(None), threshold=None, time_roll=0,
                 time_shift=None, hr_spatial_coarsen=1,
                 nan_method_kwargs=None, feature_aliases=None,
                 BaseLoader=None, FeatureRegistry=None, interp_kwargs=None,
                 cache_kwargs=None, device=None, backend=None, **kwargs):
        ignored = {k: v for k, v in (('res_kwargs', res_kwargs),
                                     ('BaseLoader', BaseLoader),
                                     ('cache_kwargs', cache_kwargs))
                   if v is not None}
        if chunks != 'auto':
            ignored['chunks'] = chunks
        if ignored:
            logger.debug('%s: arrays are resident, %s ignored',
                         type(self).__name__, sorted(ignored))
        features = parse_to_list(features)
        just_coords = not features
        raster_feats = [] if just_coords else load_features
        self.backend = backend or DeviceBackend(device)
        self.rasterizer = DeviceRasterizer(
            source, features=raster_feats, target=target, shape=shape,
            time_slice=time_slice, threshold=threshold,
            feature_aliases=feature_aliases, backend=self.backend, **kwargs)
        self.loader = self.rasterizer.loader
        self.time_slice = self.rasterizer.time_slice
        self.data = self.rasterizer.data
        self._rasterizer_hook()
        self.data = self.rasterizer.data
        if features:
            super().__init__(
                data=self.data,
                features='all' if features == ['all'] else features,
                time_roll=time_roll, time_shift=time_shift,
                hr_spatial_coarsen=hr_spatial_coarsen,
                nan_method_kwargs=nan_method_kwargs,
                FeatureRegistry=FeatureRegistry, interp_kwargs=interp_kwargs,
                backend=self.backend)
        else:
            if FeatureRegistry is not None:
                self.FEATURE_REGISTRY = FeatureRegistry
            self.interp_kwargs = interp_kwargs
            self.launch_plan, self._planned_for = [], {}
            self._dry = self._cube = None
        self._deriver_hook()

    def _rasterizer_hook(self):
        """after the rasterizer is made, before anything is derived"""

    def _deriver_hook(self):
        """after the derivations"""

    @property
    def time_step(self):
        """seconds"""
        return time_step_seconds(self.time_index)


DataHandler = DeviceDataHandler


class DailyHourlyData:
    """The ``Sup3rDataset(daily=, hourly=)`` of a ``DailyDataHandler``: two
    ``DeriveData`` on one raster.  What it is asked beyond the two members
    is answered by the last one, ``hourly``, as a ``Sup3rDataset`` does."""

    def __init__(self, daily, hourly):
        self.daily, self.hourly = daily, hourly

    def __iter__(self):
        return iter((self.daily, self.hourly))

    def __len__(self):
        return 2

    def __contains__(self, name):
        return name in self.hourly

    def __getitem__(self, name):
        return self.hourly[name]

    def __getattr__(self, name):
        if name in ('daily', 'hourly'):
            raise AttributeError(name)
        return getattr(self.hourly, name)


def daily_op(name):
    """the reduction ``DailyDataHandler._deriver_hook`` (base.py:344-365)
    gives a feature by its name, and the feature it reduces: the mean unless
    ``_max_`` / ``_min_`` / ``total_`` is in the name, the later of them
    winning, as the three ``if`` there overwrite each other"""
    op, source = 'mean', name
    if '_max_' in name:
        op = 'max'
    if '_min_' in name:
        op = 'min'
    if 'total_' in name:
        op, source = 'sum', name.split('total_')[-1]
    return op, source


class DailyDataHandler(DeviceDataHandler):
    """``DailyDataHandler`` (data_handlers/base.py:293-380)"""

    def __init__(self, source, features, **kwargs):
        features = parse_to_list(features)
        self.requested_features = features.copy()
        if 'clearsky_ratio' in features:
            needed = [f for f in self.FEATURE_REGISTRY['clearsky_ratio'].inputs
                      if f not in features]
            features.extend(needed)
        super().__init__(source, features=features, **kwargs)

    def _deriver_hook(self):
        msg = ('Data needs to be hourly with at least 24 hours, but data '
               'shape is {}.'.format(self.shape))
        day_steps = int(24 * 3600 / self.time_step)
        assert len(self.time_index) % day_steps == 0, msg
        assert len(self.time_index) > day_steps, msg
        n_data_days = int(len(self.time_index) / day_steps)
        logger.info('Calculating daily average datasets for %s training '
                    'data days.', n_data_days)
        with_ratio = 'clearsky_ratio' in self.features
        names = [f for f in self.features if 'clearsky_ratio' not in f]
        if with_ratio:
            names += ['total_clearsky_ghi', 'total_ghi']
        # every feature has its mean first (clearsky_ratio's is replaced below)
        names += [f for f in self.features
                  if 'clearsky_ratio' in f and f != 'clearsky_ratio']
        sources, outputs = [], []

        def slot(name):
            if name not in sources:
                sources.append(name)
            return sources.index(name)
        for name in names:
            op, source = daily_op(name)
            outputs.append((slot(source), None, op))
        if with_ratio:
            names.append('clearsky_ratio')
            outputs.append((slot('ghi'), slot('clearsky_ghi'), 'ratio'))
        be = self.backend
        planes = be.daily_reduce([self.data[s] for s in sources], day_steps,
                                 outputs)
        reduced = dict(zip(names, planes))
        logger.info('Finished calculating daily average datasets for %s '
                    'training data days.', n_data_days)
        self.totals = {k: reduced[k] for k in ('total_ghi',
                                               'total_clearsky_ghi')
                       if with_ratio}
        ti = self.time_index
        firsts, lasts = ti[::day_steps], ti[day_steps - 1::day_steps]
        self.daily_time_index = firsts + (lasts - firsts) / 2
        feats = self.requested_features
        hourly = self.data.subset(feats)
        daily = _dataset(be, ((f, reduced[f]) for f in feats), self.lat_lon,
                         self.daily_time_index,
                         attrs={f: self.data.attrs[f] for f in feats
                                if f in self.data.attrs})
        hourly.name, daily.name = 'hourly', 'daily'
        self.hourly = be.stack([hourly[f] for f in feats], 0)
        self.daily = be.stack([daily[f] for f in feats], 0)
        self.lr_features = self.hr_features = list(feats)
        self._cube = None
        self.data = DailyHourlyData(daily=daily, hourly=hourly)


class DataHandlerH5SolarCC(DailyDataHandler):
    """base.py:383-388"""

    FEATURE_REGISTRY = RegistryH5SolarCC


class DataHandlerH5WindCC(DailyDataHandler):
    """base.py:391-396"""

    FEATURE_REGISTRY = RegistryH5WindCC


class DataHandlerNCforCC(DeviceDataHandler):
    """``DataHandlerNCforCC`` (data_handlers/nc_cc.py:24-240): a rasterizer
    hook adds ``clearsky_ghi`` from an NSRDB source when ``clearsky_ghi`` or
    ``clearsky_ratio`` is asked for and the source has none."""

    FEATURE_REGISTRY = RegistryNCforCC

    def __init__(self, source, features='all', nsrdb_source_fp=None,
                 nsrdb_agg=1, nsrdb_smoothing=0, scale_clearsky_ghi=True,
                 **kwargs):
        self._nsrdb_source_fp = nsrdb_source_fp
        self._nsrdb_agg = nsrdb_agg
        self._nsrdb_smoothing = nsrdb_smoothing
        self._features = features
        self._scale_clearsky_ghi = scale_clearsky_ghi
        self._cs_ghi_scale = 1
        super().__init__(source, features=features, **kwargs)

    def _rasterizer_hook(self):
        cs_feats = ['clearsky_ratio', 'clearsky_ghi']
        need_cs_ghi = any(f in self._features and f not in self.rasterizer
                          for f in cs_feats)
        if need_cs_ghi:
            self.rasterizer.data['clearsky_ghi'] = self.get_clearsky_ghi()
        if need_cs_ghi and self._scale_clearsky_ghi:
            self.scale_clearsky_ghi()

    def _nsrdb_exists(self):
        fp = self._nsrdb_source_fp
        return isinstance(fp, FlatData) or (
            isinstance(fp, (str, os.PathLike)) and os.path.exists(fp))

    def run_input_checks(self):
        msg = ('Need nsrdb_source_fp input arg as a valid filepath to '
               'retrieve clearsky_ghi (maybe for clearsky_ratio) but '
               'received: {}'.format(self._nsrdb_source_fp))
        assert self._nsrdb_source_fp is not None and self._nsrdb_exists(), msg
        time_step = time_step_seconds(self.loader.time_index)
        msg = ('Can only handle source CC data in hourly frequency but '
               'received daily frequency of {}hrs (should be 24) '
               'with raw time index: {}'.format(time_step / 3600,
                                                self.rasterizer.time_index))
        assert time_step / 3600 == 24.0, msg
        msg = ('Can only handle source CC data with time_slice.step == 1 '
               'but received: {}'.format(self.rasterizer.time_slice.step))
        assert (self.rasterizer.time_slice.step is None) | (
            self.rasterizer.time_slice.step == 1), msg

    def run_wrap_checks(self, cs_ghi):
        logger.info('Reshaped clearsky_ghi data to final shape %s to '
                    'correspond with CC daily average data over source '
                    'time_slice %s with (lat, lon) grid shape of %s',
                    tuple(cs_ghi.shape), self.rasterizer.time_slice,
                    self.rasterizer.grid_shape)
        msg = ('nsrdb clearsky GHI time dimension {} '
               'does not match the GCM time dimension {}'.format(
                   cs_ghi.shape[2], len(self.rasterizer.time_index)))
        assert cs_ghi.shape[2] == len(self.rasterizer.time_index), msg

    def get_time_slice(self, ti_nsrdb):
        ti = self.rasterizer.time_index
        t_start = np.where((ti[0].month == ti_nsrdb.month)
                           & (ti[0].day == ti_nsrdb.day))[0][0]
        t_end = 1 + np.where((ti[-1].month == ti_nsrdb.month)
                             & (ti[-1].day == ti_nsrdb.day))[0][-1]
        return slice(int(t_start), int(t_end))

    def get_clearsky_ghi(self):
        """``(lat, lon, time)`` daily means of the NSRDB ``clearsky_ghi`` at
        the raster's pixels and days (nc_cc.py:160-229)"""
        from scipy.spatial import KDTree
        self.run_input_checks()
        res = self._nsrdb_source_fp
        if not isinstance(res, FlatData):
            res = FlatData.load(res)
        ti_nsrdb = res.time_index
        t_slice = self.get_time_slice(ti_nsrdb)
        cc_meta = self.rasterizer.lat_lon.reshape((-1, 2))
        tree = KDTree(res.lat_lon)
        _, i = tree.query(cc_meta, k=self._nsrdb_agg)
        i = np.expand_dims(i, axis=1) if len(i.shape) == 1 else i
        logger.info('Extracting clearsky_ghi data with time slice %s and %s '
                    'locations with agg factor %s.', t_slice, i.shape[0],
                    i.shape[1])
        # temporal coarsening from NSRDB to daily average
        hours = np.asarray((ti_nsrdb[1:] - ti_nsrdb[:-1]).seconds) / 3600
        values, counts = np.unique(hours, return_counts=True)
        time_freq = float(values[np.argmax(counts)])
        m = int(24 // time_freq)
        n_steps = t_slice.stop - t_slice.start
        if n_steps % m:
            raise ValueError(
                f'Could not coarsen a dimension of size {n_steps} with '
                f"window {m} and boundary='exact'. Try a different "
                "'boundary' option.")
        # the '%m.%d' label of each source day is that of its mean stamp
        sliced = ti_nsrdb[t_slice]
        firsts, lasts = sliced[::m], sliced[m - 1::m]
        labels = list((firsts + (lasts - firsts) / 2).strftime('%m.%d'))
        if len(set(labels)) != len(labels):
            raise ValueError(
                "cannot reindex or align along dimension 'time' because the "
                '(pandas) index has duplicate values')
        where = {label: d for d, label in enumerate(labels)}
        target = self.rasterizer.time_index.strftime('%m.%d')
        day_map = np.array([where.get(label, -1) for label in target],
                           np.int32)
        be = self.backend
        src, t_lo = res['clearsky_ghi'], t_slice.start
        if not (be.name == 'device' and hasattr(src, 'data_ptr')):
            src, t_lo = be.asarray(np.asarray(src)[t_slice]), 0
        cs_ghi = be.site_day_mean(src, i, t_lo, m, day_map)
        cs_ghi = cs_ghi.reshape(*self.rasterizer.grid_shape, len(day_map))
        self.run_wrap_checks(cs_ghi)
        return cs_ghi

    def scale_clearsky_ghi(self):
        """nc_cc.py:231-240"""
        data = self.rasterizer.data
        scaled, self._cs_ghi_scale = self.backend.scale_to_time_max(
            data['rsds'], data['clearsky_ghi'])
        data['clearsky_ghi'] = scaled


class DataHandlerNCforCCwithPowerLaw(DataHandlerNCforCC):
    """nc_cc.py:243-246"""

    FEATURE_REGISTRY = RegistryNCforCCwithPowerLaw
