"""Bias correction of low-res input on the device.

The reference corrects every forward-pass chunk on the host before the
generator sees it (``ForwardPassStrategy.prep_chunk_data``,
sup3r/pipeline/strategy.py:502-517 -> ``bias_correct_features`` ->
sup3r/bias/bias_transforms.py).  This module has the five transforms of that
file with the reference's argument names and defaults —

    global_linear_bc            bias_transforms.py:224
    local_linear_bc             :251
    monthly_local_linear_bc     :351
    local_qdm_bc                :622
    local_presrat_bc            :958

— and ``DeviceBiasCorrection``, which keeps each feature's factor tables on
the device for the whole low-res domain and corrects a batch of padded chunks
with one ``s3_bias_correct`` launch (include/sup3r_hip.h), optionally writing
the result normalised so that the executor needs no second pass.

All arithmetic runs in the HIP kernel: there is no CPU fallback, a host array
makes a round trip through the device.  What the host does is planning: the
month / time-window index of every time step, the month weights of
``temporal_avg=True``, the grid window of the factor tables, and — with
``smoothing > 0`` — the reference's own ``scipy.ndimage.gaussian_filter`` call
on the chunk's small factor window.

Parameter source (``bias_fp``): ``h5py`` / ``rex`` are not needed; ``bias_fp``
is a mapping, the path of an ``.npz`` or a ``BiasParams`` carrying the
reference's dataset names (``{feature}_scalar``, ``{feature}_adder``,
``base_{base_dset}_params``, ``bias_{feature}_params``,
``bias_fut_{feature}_params``, ``{feature}_tau_fut``, ``{feature}_k_factor``,
optional ``latitude`` / ``longitude``) and attributes (``time_window_center``,
``dist``, ``sampling``, ``log_base``, ``zero_rate_threshold``).

The factors themselves are computed by ``sup3r_amd.bias_calc``, whose ``.npz``
output is read here unchanged.

Not here: parametric ``dist`` and the log samplings (defined inside ``rex``),
and the resident-domain executor (``ForwardPass.run_batched`` /
``upload_domain``).
The empirical quantile mapping itself lives in ``rex``
(``rex.utilities.bc_utils.QuantileDeltaMapping``), which is not available
where this project is built: it is restated from ``numpy.interp`` and Cannon
et al. 2015, eqs. 3-6, as the reference's docstrings describe it.
"""
import ctypes as C
import logging
import os
from warnings import warn

import numpy as np

from . import _lib

logger = logging.getLogger(__name__)

ATTRS = ('time_window_center', 'dist', 'sampling', 'log_base',
         'zero_rate_threshold')
METHODS = ('global_linear_bc', 'local_linear_bc', 'monthly_local_linear_bc',
           'local_qdm_bc', 'local_presrat_bc')
#: methods that read the chunk's time index
TIME_METHODS = ('monthly_local_linear_bc', 'local_qdm_bc', 'local_presrat_bc')

QDM_NONFINITE = (
    'QDM bias correction resulted in NaN / inf values! If this is a '
    'relative QDM, you may try setting ``delta_denom_min`` or '
    '``delta_denom_zero``')
PRESRAT_NONFINITE = (
    'Presrat bias correction resulted in NaN values! If this is a '
    'relative QDM, you may try setting ``delta_denom_min`` or '
    '``delta_denom_zero``')


# ---------------------------------------------------------------- parameters
class BiasParams:
    """The datasets and attributes of a bias-correction file, in memory.

    ``datasets``: name -> array (names are matched in lower case, as the
    reference's loader does); ``attrs``: the file's global attributes."""

    def __init__(self, datasets, attrs=None, source=None):
        self.datasets = {str(k).lower(): v for k, v in datasets.items()}
        self.attrs = dict(attrs or {})
        self.source = source or '<memory>'

    @classmethod
    def load(cls, bias_fp):
        """a ``BiasParams``, a mapping or the path of an ``.npz`` -> a
        ``BiasParams``; the attribute names (``ATTRS``) are taken out of a
        mapping / archive's keys"""
        if isinstance(bias_fp, cls):
            return bias_fp
        source = None
        if isinstance(bias_fp, (str, os.PathLike)):
            source = os.fspath(bias_fp)
            if not source.endswith('.npz'):
                raise ValueError(
                    f'bias_fp "{source}": only .npz archives, mappings and '
                    'BiasParams are read here (h5py / rex are not used)')
            with np.load(source, allow_pickle=False) as z:
                bias_fp = {k: z[k] for k in z.files}
        if not hasattr(bias_fp, 'items'):
            raise TypeError('bias_fp must be a mapping, an .npz path or a '
                            f'BiasParams, not {type(bias_fp).__name__}')
        data, attrs = {}, {}
        for k, v in bias_fp.items():
            if k in ATTRS:
                v = np.asarray(v)
                attrs[k] = v.item() if v.ndim == 0 else v
            elif k in ('attrs', 'cfg', 'global_attrs') and hasattr(v, 'items'):
                attrs.update(v)
            else:
                data[k] = v
        return cls(data, attrs, source)

    def get(self, var_names):
        """``_get_factors`` (bias_transforms.py:71-76): the named datasets, an
        ``AssertionError`` naming the missing ones"""
        missing = [d for d in var_names.values()
                   if d.lower() not in self.datasets]
        msg = f'Missing {" and ".join(missing)} in resource: {self.source}.'
        assert missing == [], msg
        return {k: np.asarray(self.datasets[v.lower()])
                for k, v in var_names.items()}


def grid_window(params, lat_lon, threshold=0.1):
    """Where the domain ``lat_lon`` (rows, cols, 2) lies in the tables' grid:
    ``(row0, col0)`` of its upper-left cell — the window of
    ``lat_lon.shape[:2]`` whose lower-left corner is the grid point nearest
    to ``lat_lon[-1, 0]``, as the reference's rasteriser places it
    (``_get_factors``, bias_transforms.py:27-77); ``RuntimeError`` if that
    point is farther than ``threshold``.  ``None`` when there is nothing to
    match (no ``lat_lon`` or no ``latitude`` / ``longitude`` datasets): the
    tables then must already have the domain's shape."""
    if lat_lon is None or 'latitude' not in params.datasets or \
            'longitude' not in params.datasets:
        return None
    lat_lon = np.asarray(lat_lon)
    lat = np.asarray(params.datasets['latitude'], dtype=np.float64)
    lon = np.asarray(params.datasets['longitude'], dtype=np.float64)
    target = lat_lon[-1, 0, :].astype(np.float64)
    dist = np.hypot(lat - target[0], lon - target[1])
    row, col = np.unravel_index(np.argmin(dist), dist.shape)
    if dist[row, col] > threshold:
        raise RuntimeError(
            f'The nearest bias-correction grid point to {tuple(target)} is '
            f'{dist[row, col]:.4f} away (threshold {threshold}): '
            f'{params.source} does not cover the domain')
    rows, cols = lat_lon.shape[:2]
    row0 = int(row) - rows + 1
    if row0 < 0 or int(col) + cols > lat.shape[1]:
        raise RuntimeError(
            f'A {rows} x {cols} window with its lower-left corner at grid '
            f'point ({row}, {col}) leaves the {lat.shape} grid of '
            f'{params.source}')
    return row0, int(col)


def _domain_tables(params, var_names, lat_lon, threshold):
    """the named tables cut to the domain (grid window or shape check)"""
    out = params.get(var_names)
    win = grid_window(params, lat_lon, threshold)
    if win is not None:
        rows, cols = np.asarray(lat_lon).shape[:2]
        sl = (slice(win[0], win[0] + rows), slice(win[1], win[1] + cols))
        out = {k: v[sl] for k, v in out.items()}
    elif lat_lon is not None:
        want = tuple(np.asarray(lat_lon).shape[:2])
        for k, v in out.items():
            if tuple(v.shape[:2]) != want:
                raise ValueError(
                    f'"{var_names[k]}" has grid {tuple(v.shape[:2])}, the '
                    f'domain {want}, and {params.source} has no latitude / '
                    'longitude to match them by')
    return out


# ------------------------------------------------------------ host planning
def make_time_index(date_range_kwargs):
    """``make_time_index_from_kws`` (sup3r/preprocessing/utilities.py:222-244);
    a ``DatetimeIndex`` is passed through"""
    import pandas as pd
    if isinstance(date_range_kwargs, pd.DatetimeIndex):
        return date_range_kwargs
    if not hasattr(date_range_kwargs, 'items'):
        return pd.DatetimeIndex(date_range_kwargs)
    kws = dict(date_range_kwargs)
    drop_leap = kws.pop('drop_leap', False)
    time_index = pd.date_range(**kws)
    if drop_leap:
        leap = (time_index.month == 2) & (time_index.day == 29)
        time_index = time_index[~leap]
    return time_index


def mirror_index(n_padded, lo, extent):
    """for every index of an axis reflect-padded by ``lo`` in front, the
    index into the un-padded ``extent`` it repeats — the index map of
    ``np.pad(mode='reflect')`` (any pad width) and the rule the kernel
    applies to the factor tables"""
    u = np.arange(n_padded) - lo
    if extent <= 1:
        return np.zeros(n_padded, dtype=np.int64)
    p = 2 * (extent - 1)
    m = np.mod(u, p)
    return np.where(m < extent, m, p - m).astype(np.int64)


def month_index(time_index, pad=(0, 0)):
    """month (0 .. 11) of every step of the window's time index, mirrored
    along time by the chunk's reflect padding"""
    months = np.asarray(time_index.month) - 1
    return months[mirror_index(len(months) + pad[0] + pad[1], pad[0],
                               len(months))].astype(np.int32)


def month_weights(time_index):
    """share of each month in the window's time index: ``sum_m w_m table[...,
    m]`` is the mean over the gathered months of ``temporal_avg=True``
    (bias_transforms.py:438-448).  Also returns the number of distinct
    months (the reference warns above two, :449-455)."""
    months = np.asarray(time_index.month) - 1
    counts = np.bincount(months, minlength=12).astype(np.float64)
    return counts / counts.sum(), int((counts > 0).sum())


def window_index(time_index, time_window_center, pad=(0, 0)):
    """``argmin |doy - time_window_center|`` per time step, first minimum on
    ties (bias_transforms.py:788-791), mirrored along time"""
    doy = np.asarray(time_index.day_of_year, dtype=np.float64)
    centers = np.asarray(time_window_center, dtype=np.float64).reshape(-1)
    idx = np.abs(doy[:, None] - centers[None, :]).argmin(axis=1)
    return idx[mirror_index(len(idx) + pad[0] + pad[1], pad[0],
                            len(idx))].astype(np.int32)


def _range(r):
    return None if r is None else (float(np.min(r)), float(np.max(r)))


def _nan_warning(feature, source):
    msg = ('Bias correction scalar/adder values had NaNs for '
           f'"{feature}" from: {source}')
    logger.warning(msg)
    warn(msg)


def _smooth(table, smoothing):
    """bias_transforms.py:334-341 / :465-472 on a (e1, e2, k) window"""
    from scipy.ndimage import gaussian_filter
    out = np.array(table, dtype=np.float32)
    for idt in range(out.shape[-1]):
        out[..., idt] = gaussian_filter(out[..., idt], smoothing,
                                        mode='nearest')
    return out


class _Feature:
    """One feature's correction: the descriptor fields and the host copy of
    its tables (domain-sized); ``DeviceBiasCorrection`` uploads them."""

    def __init__(self, method, feature, kwargs, lat_lon=None):
        if method not in METHODS:
            raise KeyError(f'unknown bias correction method "{method}"; '
                           f'have {METHODS}')
        kw = dict(kwargs)
        kw.pop('lr_padded_slice', None)
        kw.pop('date_range_kwargs', None)
        kw.pop('max_workers', None)
        self.method, self.feature = method, feature
        self.kind, self.flags, self.n_t, self.n_q = _lib.BC_LINEAR, 0, 1, 0
        self.tables = {}
        self.limits = {}
        self.smoothing = 0
        self.centers = None
        self.source = '<arguments>'
        self.month_mode = None          # 'month' / 'weights' for monthly
        out_range = _range(kw.pop('out_range', None))
        if out_range is not None:
            self.flags |= _lib.BC_OUT_RANGE
            self.limits['out'] = out_range
        if method == 'global_linear_bc':
            self.flags |= _lib.BC_GLOBAL
            self.tables = {
                'scalar': np.full((1, 1, 1), kw.pop('scalar'), np.float32),
                'adder': np.full((1, 1, 1), kw.pop('adder'), np.float32)}
        else:
            kw.setdefault('feature_name', feature)
            params = BiasParams.load(kw.pop('bias_fp'))
            self.source = params.source
            threshold = kw.pop('threshold', 0.1)
            name = kw.pop('feature_name')
            if method in ('local_linear_bc', 'monthly_local_linear_bc'):
                self._linear(method, name, params, kw, lat_lon, threshold)
            else:
                self._qdm(method, name, params, kw, lat_lon, threshold)
        if kw:
            raise TypeError(f'{method}() got unexpected keyword arguments '
                            f'{sorted(kw)}')

    def _linear(self, method, name, params, kw, lat_lon, threshold):
        t = _domain_tables(params, {'scalar': f'{name}_scalar',
                                    'adder': f'{name}_adder'},
                           lat_lon, threshold)
        scalar, adder = t['scalar'], t['adder']
        self.smoothing = kw.pop('smoothing', 0)
        if method == 'local_linear_bc':
            # (:311-313: seasonal factors are averaged over the months)
            if scalar.ndim == 3 and adder.ndim == 3:
                scalar, adder = scalar.mean(axis=-1), adder.mean(axis=-1)
        else:
            assert scalar.ndim == 3, 'Monthly bias correct needs 3D scalars'
            assert adder.ndim == 3, 'Monthly bias correct needs 3D adders'
            if scalar.shape[-1] != 12 or adder.shape[-1] != 12:
                raise ValueError(
                    'Monthly bias correct needs 12 months on the last axis, '
                    f'got {scalar.shape} / {adder.shape}')
            self.month_mode = 'weights' if kw.pop('temporal_avg', True) \
                else 'month'
            self.flags |= _lib.BC_WEIGHTS if self.month_mode == 'weights' \
                else _lib.BC_MONTH
            for key, flag in (('scalar', _lib.BC_SCALAR_RANGE),
                              ('adder', _lib.BC_ADDER_RANGE)):
                r = _range(kw.pop(f'{key}_range', None))
                if r is not None:
                    self.flags |= flag
                    self.limits[key] = r
        if scalar.ndim == 2:
            scalar, adder = scalar[..., None], adder[..., None]
        self.n_t = int(scalar.shape[-1])
        self.tables = {'scalar': np.ascontiguousarray(scalar, np.float32),
                       'adder': np.ascontiguousarray(adder, np.float32)}

    def _qdm(self, method, name, params, kw, lat_lon, threshold):
        base_dset = kw.pop('base_dset')
        names = {'oh': f'base_{base_dset}_params',
                 'mh': f'bias_{name}_params',
                 'mf': f'bias_fut_{name}_params'}
        presrat = method == 'local_presrat_bc'
        if presrat:
            names.update(tau=f'{name}_tau_fut', kfac=f'{name}_k_factor')
        t = _domain_tables(params, names, lat_lon, threshold)
        cfg = params.attrs
        dist = cfg.get('dist', 'empirical')
        if dist != 'empirical':
            raise KeyError(
                f'dist="{dist}": only the empirical distribution is '
                'implemented (parametric dist lives in rex)')
        sampling = cfg.get('sampling', 'linear')
        if sampling != 'linear':
            raise KeyError(
                f'sampling="{sampling}": only linear sampling is implemented '
                '(the log samplings are defined inside rex)')
        if 'time_window_center' not in cfg:
            raise KeyError(f'{params.source} lacks the attribute '
                           '"time_window_center"')
        self.centers = np.asarray(cfg['time_window_center'],
                                  dtype=np.float64).reshape(-1)
        self.kind = _lib.BC_QDM
        for k in ('oh', 'mh', 'mf'):
            if t[k].ndim != 4 or t[k].shape[2] != len(self.centers):
                raise ValueError(
                    f'"{names[k]}" must be (rows, cols, '
                    f'{len(self.centers)} time windows, quantiles), got '
                    f'{t[k].shape}')
        self.n_t, self.n_q = (int(v) for v in t['oh'].shape[2:])
        if kw.pop('relative', True):
            self.flags |= _lib.BC_RELATIVE
        no_trend = kw.pop('no_trend', False)
        if no_trend:
            self.flags |= _lib.BC_NO_TREND
        denom_min = kw.pop('delta_denom_min', None)
        if presrat:
            # (:1072-1073)
            denom_min = denom_min or cfg['zero_rate_threshold']
        if denom_min is not None:
            self.flags |= _lib.BC_DENOM_MIN
            self.limits['denom_min'] = float(denom_min)
        denom_zero = kw.pop('delta_denom_zero', None)
        if denom_zero is not None:
            self.flags |= _lib.BC_DENOM_ZERO
            self.limits['denom_zero'] = float(denom_zero)
        delta = _range(kw.pop('delta_range', None))
        if delta is not None:
            self.flags |= _lib.BC_DELTA_RANGE
            self.limits['delta'] = delta
        tabs = {k: np.ascontiguousarray(t[k], np.float32)
                for k in ('oh', 'mh', 'mf')}
        if presrat:
            self.flags |= _lib.BC_PRESRAT
            kfac = np.asarray(t['kfac'])
            k_range = kw.pop('k_range', None)
            if k_range is not None:
                # (:1075-1077)
                kfac = np.maximum(kfac, np.min(k_range))
                kfac = np.minimum(kfac, np.max(k_range))
            tau = np.asarray(t['tau'])
            tabs['tau'] = np.ascontiguousarray(
                tau.reshape(tau.shape[:2]), np.float32)
            tabs['kfac'] = np.ascontiguousarray(kfac, np.float32)
        self.tables = tabs

    @property
    def needs_time(self):
        return self.method in TIME_METHODS

    @property
    def nonfinite_message(self):
        if self.method == 'local_qdm_bc':
            return QDM_NONFINITE
        if self.method == 'local_presrat_bc':
            return PRESRAT_NONFINITE
        return None


class ChunkWindow:
    """What a chunk tells the correction: ``lr_pad_slice`` (its in-domain
    window of the low-res domain, space and time), ``pad_width`` (the reflect
    padding added around it at the domain's edges) and ``time_index`` (the
    window's time steps, un-mirrored)."""

    def __init__(self, lr_pad_slice, pad_width=None, time_index=None):
        self.lr_pad_slice = tuple(lr_pad_slice)
        self.pad_width = tuple(tuple(int(v) for v in p) for p in (
            pad_width or ((0, 0), (0, 0), (0, 0))))
        self.time_index = time_index


class BiasCorrectRecord(ChunkWindow):
    """the ``bias_correct`` record ``ArrayStrategy.init_chunk`` attaches to a
    chunk: the method, the per-feature kwargs, the chunk's window and the
    window's low-res time index.  ``shared`` is one dict per strategy in which
    the executor keeps the ``DeviceBiasCorrection`` (tables uploaded once)."""

    def __init__(self, method, kwargs, lr_pad_slice, time_index=None,
                 lat_lon=None, shared=None, domain_shape=None):
        super().__init__(lr_pad_slice, None, time_index)
        self.method, self.kwargs = method, kwargs
        self.lat_lon = lat_lon
        self.domain_shape = domain_shape
        self.shared = shared if shared is not None else {}


class BiasPlan:
    """The host half of a correction: each feature's tables (cut to the
    domain) and descriptor fields, and the per-batch planning — chunk
    geometry, month / window indices, month weights, the reference's
    warnings.  Needs no device.

    ``method``: one of ``METHODS``; ``kwargs``: feature -> keyword arguments
    of that method (the reference's ``bias_correct_kwargs``); ``lr_features``:
    the channel order of the tensors to correct — channels whose feature has
    no entry pass through; ``lat_lon`` (rows, cols, 2): the low-res domain the
    tables are matched to when they carry coordinates."""

    def __init__(self, method, kwargs, lr_features, lat_lon=None,
                 domain_shape=None):
        self.method = method
        self.lr_features = list(lr_features)
        lower = [f.lower() for f in self.lr_features]
        absent = [f for f in kwargs if f.lower() not in lower]
        if absent:
            raise ValueError(
                f'bias_correct_kwargs names {absent}, the model\'s low-res '
                f'features are {self.lr_features}')
        if len(self.lr_features) > _lib.BC_MAX_CHANNELS:
            raise RuntimeError(
                f's3_bias_correct carries at most {_lib.BC_MAX_CHANNELS} '
                f'channels, the input has {len(self.lr_features)}')
        by_name = {f.lower(): (f, kw) for f, kw in kwargs.items()}
        self.features = []
        for name in lower:
            if name not in by_name:
                self.features.append(None)
                continue
            f, kw = by_name[name]
            if method == 'monthly_local_linear_bc' and \
                    'temporal_avg' not in kw:
                # (bias/utilities.py:272-284)
                msg = ('The kwarg "temporal_avg" was not provided in the bias '
                       'correction kwargs but is present in the bias '
                       f'correction function "{method}". If this is not set '
                       'appropriately, especially for monthly bias '
                       'correction, it could result in QA results that look '
                       'worse than they actually are.')
                logger.warning(msg)
                warn(msg)
            self.features.append(_Feature(method, f, kw, lat_lon))
        shapes = {tuple(f.tables['scalar' if f.kind == _lib.BC_LINEAR
                                 else 'oh'].shape[:2])
                  for f in self.features
                  if f is not None and not f.flags & _lib.BC_GLOBAL}
        if len(shapes) > 1:
            raise ValueError(f'the features\' tables cover different grids: '
                             f'{sorted(shapes)}')
        self.grid = shapes.pop() if shapes else (0, 0)
        if domain_shape is not None and any(self.grid) and \
                tuple(self.grid) != tuple(int(v) for v in domain_shape[:2]):
            # (without coordinates the tables must already have the domain's
            # shape; with them ``_domain_tables`` has cut the tables to it)
            raise ValueError(
                f'the factor tables cover a {tuple(self.grid)} grid, the '
                f'low-res domain is {tuple(domain_shape[:2])}')
        self._nan_seen = set()

    @property
    def needs_time(self):
        return any(f is not None and f.needs_time for f in self.features)

    # -- host planning ---------------------------------------------------
    def geometry(self, windows, shape):
        """(n, 6) int32: o1, o2, lo1, lo2, e1, e2 per chunk of padded
        ``shape``"""
        geo = np.zeros((len(windows), 6), dtype=np.int32)
        for k, w in enumerate(windows):
            for a in range(2):
                sl = w.lr_pad_slice[a]
                start = 0 if sl is None or sl.start is None else sl.start
                lo, hi = w.pad_width[a]
                e = shape[a] - lo - hi
                if sl is not None and sl.stop is not None and \
                        sl.stop - start != e:
                    raise ValueError(
                        f'chunk axis {a}: {shape[a]} cells with padding '
                        f'{(lo, hi)} do not match lr_pad_slice {sl}')
                geo[k, a], geo[k, 2 + a], geo[k, 4 + a] = start, lo, e
        return geo

    def time_plan(self, windows, n_t):
        """per chunk: month index (n, t), month weights (n, 12), window index
        (n, t) — whichever the features need, else None"""
        want_m = any(f is not None and f.month_mode for f in self.features)
        qdm = [f for f in self.features
               if f is not None and f.kind == _lib.BC_QDM]
        if not (want_m or qdm):
            return None, None, None
        month = weights = window = None
        if want_m:
            month = np.zeros((len(windows), n_t), np.int32)
            weights = np.zeros((len(windows), 12), np.float64)
        if qdm:
            window = np.zeros((len(windows), n_t), np.int32)
            for f in qdm[1:]:
                if not np.array_equal(f.centers, qdm[0].centers):
                    raise ValueError('the features\' QDM tables have '
                                     'different time_window_center')
        for k, w in enumerate(windows):
            if w.time_index is None:
                raise ValueError(
                    f'{self.method} needs the chunk\'s low-res time index')
            pad = w.pad_width[2]
            if len(w.time_index) + pad[0] + pad[1] != n_t:
                msg = ('Time should align with data 3rd dimension but got '
                       f'{n_t} steps (padding {pad}) and time_index length '
                       f'{len(w.time_index)}: {w.time_index}')
                raise AssertionError(msg)
            if want_m:
                month[k] = month_index(w.time_index, pad)
                weights[k], distinct = month_weights(w.time_index)
                if distinct > 2 and any(
                        f is not None and f.month_mode == 'weights'
                        for f in self.features):
                    msg = ('Bias correction method "monthly_local_linear_bc" '
                           'was used with temporal averaging over a time '
                           'index with >2 months.')
                    warn(msg)
                    logger.warning(msg)
            if qdm:
                window[k] = window_index(w.time_index, qdm[0].centers, pad)
        return month, weights, window

    def _chunk_tables(self, f, windows, geo, shape, months):
        """smoothing > 0: the reference filters the chunk's own factor window
        (after the month gather / mean); the filtered windows, reflect-padded
        like the chunks, become per-chunk tables"""
        outs = {'scalar': [], 'adder': []}
        for k, w in enumerate(windows):
            o1, o2, lo1, lo2, e1, e2 = (int(v) for v in geo[k])
            sl = (slice(o1, o1 + e1), slice(o2, o2 + e2))
            for key in outs:
                tab = f.tables[key][sl]
                if f.month_mode == 'weights':
                    im = np.asarray(w.time_index.month) - 1
                    tab = tab[..., im].mean(axis=-1)[..., None]
                tab = _smooth(tab, f.smoothing)
                pw = ((lo1, shape[0] - lo1 - e1), (lo2, shape[1] - lo2 - e2),
                      (0, 0))
                outs[key].append(np.pad(tab, pw, mode='reflect'))
        return {k: np.stack(v, axis=0) for k, v in outs.items()}

    def _warn_nan(self, geo):
        for f in self.features:
            if f is None or f.kind != _lib.BC_LINEAR:
                continue
            for o1, o2, _, _, e1, e2 in (tuple(int(v) for v in g)
                                         for g in geo):
                key = (f.feature, o1, o2, e1, e2)
                if key in self._nan_seen:
                    continue
                self._nan_seen.add(key)
                sl = (slice(None), slice(None)) if f.flags & _lib.BC_GLOBAL \
                    else (slice(o1, o1 + e1), slice(o2, o2 + e2))
                if np.isnan(f.tables['scalar'][sl]).any() or \
                        np.isnan(f.tables['adder'][sl]).any():
                    _nan_warning(f.feature, f.source)



class DeviceBiasCorrection(BiasPlan):
    """The correction of a set of low-res features, resident on one device:
    a ``BiasPlan`` whose tables are uploaded once.

    ``correct(x, windows, ...)`` corrects a batch ``(n, s1, s2, t, c)`` of
    equal-shaped padded chunks, described by one ``ChunkWindow`` each, with
    one ``s3_bias_correct`` launch."""

    def __init__(self, method, kwargs, lr_features, dev=None, lat_lon=None,
                 domain_shape=None):
        from .engine import Device
        super().__init__(method, kwargs, lr_features, lat_lon=lat_lon,
                         domain_shape=domain_shape)
        self.dev = dev or Device.get()
        self.dtables = [None if f is None else {
            k: self.dev.to_device(v) for k, v in f.tables.items()}
            for f in self.features]

    def correct(self, x, windows, out=None, mean=None, std=None,
                stats_fp32=True, counts=None, upload=None, keep=None):
        """Correct ``x`` (device fp32 ``(n, s1, s2, t, c)``) into ``out``
        (default: in place) and return ``(out, counts)``: ``prepare`` + the
        launches."""
        keep = keep if keep is not None else []     # alive across the launch
        calls, out, counts = self.prepare(
            x, windows, out=out, mean=mean, std=std, stats_fp32=stats_fp32,
            counts=counts, upload=upload, keep=keep)
        L = _lib.lib()
        for args in calls:
            _lib.check(L.s3_bias_correct(self.dev.ctx, *args), self.dev.ctx,
                       's3_bias_correct')
        return out, counts

    def prepare(self, x, windows, out=None, mean=None, std=None,
                stats_fp32=True, counts=None, upload=None, keep=None):
        """Everything in front of the launch: the host planning, the small
        index upload, the descriptors.  Returns ``(calls, out, counts)``,
        ``calls`` = the argument tuples (behind the context) of one
        ``s3_bias_correct`` call per ``BC_MAX_CHUNKS`` chunks.  The device
        temporaries the calls point to live in ``keep``: pass a list and hold
        it until the calls have been made.

        ``x``: device fp32 ``(n, s1, s2, t, c)``; ``out``: default in place.

        ``mean`` / ``std`` (c values): write ``(result - mean) / std`` (fp32
        arithmetic with ``stats_fp32``, fp64 rounded once otherwise).
        ``counts``: device int32 ``(c,)`` the non-finite results per channel
        are added to (allocated and zeroed when None); ``check(counts)``
        raises for them.  ``upload(array)``: how a host array (the uint8 index
        buffer, fp32 per-chunk tables) reaches the device with its dtype kept
        (default: a plain copy); ``keep``: a list that keeps temporaries
        alive until the batch is finished."""
        import torch
        dev = self.dev
        if upload is None:
            def upload(a):
                return torch.from_numpy(np.ascontiguousarray(a)).to(
                    dev.torch_device)
        n, s1, s2, n_t, c = (int(v) for v in x.shape)
        if c != len(self.features) or len(windows) != n:
            raise ValueError(
                f'{tuple(x.shape)}: expected {len(self.features)} channels '
                f'and {len(windows)} chunks')
        out = x if out is None else out
        keep = keep if keep is not None else []
        if counts is None:
            counts = torch.zeros(c, dtype=torch.int32,
                                 device=dev.torch_device)
        geo = self.geometry(windows, (s1, s2))
        self._warn_nan(geo)
        month, weights, window = self.time_plan(windows, n_t)
        # one small upload: weights (fp64) first, then the int32 indices
        parts, offs, pos = [], {}, 0
        for name, arr in (('weights', weights), ('month', month),
                          ('window', window)):
            if arr is not None:
                raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
                offs[name] = pos
                parts.append(raw)
                pos += raw.size
        ptr = {'weights': None, 'month': None, 'window': None}
        if parts:
            tens = upload(np.concatenate(parts))           # raw bytes
            keep.append(tens)
            ptr.update({k: C.c_void_p(tens.data_ptr() + v)
                        for k, v in offs.items()})
        chans = (_lib.BiasChannel * c)()
        per_chunk = []
        for i, f in enumerate(self.features):
            d = chans[i]
            if f is None:
                d.kind = _lib.BC_NONE
                continue
            d.kind, d.flags, d.n_t, d.n_q = f.kind, f.flags, f.n_t, f.n_q
            tabs = self.dtables[i]
            if f.smoothing > 0:
                host = self._chunk_tables(f, windows, geo, (s1, s2), month)
                tabs = {k: upload(np.ascontiguousarray(v, np.float32))
                        for k, v in host.items()}
                per_chunk.append(tabs)
                d.flags |= _lib.BC_PER_CHUNK
                d.n_t = int(host['scalar'].shape[-1])
                if f.month_mode == 'weights':
                    # (the mean is already in the table)
                    d.flags &= ~_lib.BC_WEIGHTS
            for k, t in tabs.items():
                setattr(d, k, t.data_ptr())
            lim = f.limits
            d.scalar_lo, d.scalar_hi = lim.get('scalar', (0, 0))
            d.adder_lo, d.adder_hi = lim.get('adder', (0, 0))
            d.out_lo, d.out_hi = lim.get('out', (0, 0))
            d.delta_lo, d.delta_hi = lim.get('delta', (0, 0))
            d.denom_min = lim.get('denom_min', 0)
            d.denom_zero = lim.get('denom_zero', 0)
        keep.extend(per_chunk)
        pd = C.POINTER(C.c_double)
        mu = sd = None
        if mean is not None and std is not None:
            mu = np.ascontiguousarray(mean, dtype=np.float64)
            sd = np.ascontiguousarray(std, dtype=np.float64)
            if len(mu) != c or len(sd) != c:
                raise RuntimeError(
                    f'{len(mu)} normalisation statistics for {c} input '
                    'features')
        per = s1 * s2 * n_t * c
        calls = []
        for k0 in range(0, n, _lib.BC_MAX_CHUNKS):
            nk = min(_lib.BC_MAX_CHUNKS, n - k0)
            g = np.ascontiguousarray(geo[k0:k0 + nk])
            sub = (_lib.BiasChannel * c)()
            for i in range(c):
                sub[i] = chans[i]
                if sub[i].flags & _lib.BC_PER_CHUNK:
                    row = s1 * s2 * sub[i].n_t * 4
                    sub[i].scalar += k0 * row
                    sub[i].adder += k0 * row

            def off(p, stride):
                return None if p is None else C.c_void_p(
                    p.value + k0 * stride)
            calls.append((
                C.c_void_p(x.data_ptr() + 4 * per * k0), nk, s1, s2,
                n_t, c, sub, int(self.grid[0]), int(self.grid[1]),
                g.ctypes.data_as(C.POINTER(C.c_int32)),
                off(ptr['month'], 4 * n_t), off(ptr['window'], 4 * n_t),
                off(ptr['weights'], 8 * 12),
                mu.ctypes.data_as(pd) if mu is not None else None,
                sd.ctypes.data_as(pd) if sd is not None else None,
                int(bool(stats_fp32)),
                C.c_void_p(out.data_ptr() + 4 * per * k0),
                C.c_void_p(counts.data_ptr())))
        return calls, out, counts

    def check(self, counts):
        """raise the reference's ``RuntimeError`` (bias_transforms.py:816-823,
        :1128-1135) if a QDM / PresRat channel produced non-finite values"""
        host = counts.cpu().numpy()
        for f, bad in zip(self.features, host):
            if f is not None and bad and f.nonfinite_message:
                logger.error(f.nonfinite_message)
                raise RuntimeError(f.nonfinite_message)


# ------------------------------------------------- the reference's functions
def _apply(method, data, kwargs, lat_lon, lr_padded_slice, time_index):
    """one feature, one un-padded window ``(s1, s2, t)`` through the kernel;
    the result is the same kind as ``data``"""
    import torch

    from .engine import Device
    dev = Device.get()
    is_tensor = isinstance(data, torch.Tensor)
    msg = ('data was expected to be a 3D array but got shape '
           f'{tuple(data.shape)}')
    assert data.ndim == 3, msg
    bc = DeviceBiasCorrection(method, {'feature': kwargs}, ['feature'],
                              dev=dev, lat_lon=lat_lon)
    bc.features[0].feature = kwargs.get('feature_name', 'feature')
    x = dev.to_device(data).reshape(1, *data.shape, 1)
    if is_tensor and x.data_ptr() == data.data_ptr():
        x = x.clone()
    sl = lr_padded_slice if lr_padded_slice is not None else \
        (slice(None), slice(None))
    f = bc.features[0]
    if lr_padded_slice is None and not f.flags & _lib.BC_GLOBAL and \
            tuple(bc.grid) != tuple(data.shape[:2]):
        raise ValueError(f'data covers {tuple(data.shape[:2])} cells, the '
                         f'factors {tuple(bc.grid)}')
    win = ChunkWindow((sl[0], sl[1]), None, time_index)
    if time_index is not None and f.needs_time:
        msg = ('Time should align with data 3rd dimension but got data '
               f'{tuple(data.shape)} and time_index length '
               f'{len(time_index)}: {time_index}')
        assert data.shape[-1] == len(time_index), msg
    y, counts = bc.correct(x, [win])
    bc.check(counts)
    y = y.reshape(tuple(data.shape))
    return y if is_tensor else y.cpu().numpy()


def global_linear_bc(data, scalar, adder, out_range=None):
    """bias_transforms.py:224-248: ``data * scalar + adder`` with one scalar
    and one adder for the whole array, then the optional ``out_range``."""
    return _apply('global_linear_bc', data,
                  dict(scalar=scalar, adder=adder, out_range=out_range),
                  None, None, None)


def local_linear_bc(data, lat_lon, feature_name, bias_fp,
                    lr_padded_slice=None, out_range=None, smoothing=0,
                    threshold=0.1):
    """bias_transforms.py:251-348: site-by-site ``data * scalar + adder``
    with factors constant in time (3-D factors: their mean over the months)."""
    return _apply('local_linear_bc', data,
                  dict(feature_name=feature_name, bias_fp=bias_fp,
                       out_range=out_range, smoothing=smoothing,
                       threshold=threshold),
                  lat_lon, lr_padded_slice, None)


def monthly_local_linear_bc(data, lat_lon, feature_name, bias_fp,
                            date_range_kwargs, lr_padded_slice=None,
                            temporal_avg=True, out_range=None, smoothing=0,
                            scalar_range=None, adder_range=None,
                            threshold=0.1):
    """bias_transforms.py:351-487: site-by-site monthly factors, per time
    step (``temporal_avg=False``) or averaged over the time index."""
    return _apply('monthly_local_linear_bc', data,
                  dict(feature_name=feature_name, bias_fp=bias_fp,
                       temporal_avg=temporal_avg, out_range=out_range,
                       smoothing=smoothing, scalar_range=scalar_range,
                       adder_range=adder_range, threshold=threshold),
                  lat_lon, lr_padded_slice,
                  make_time_index(date_range_kwargs))


def local_qdm_bc(data, lat_lon, base_dset, feature_name, bias_fp,
                 date_range_kwargs, lr_padded_slice=None, threshold=0.1,
                 relative=True, no_trend=False, delta_denom_min=None,
                 delta_denom_zero=None, delta_range=None, out_range=None,
                 max_workers=1):
    """bias_transforms.py:622-824: empirical quantile delta mapping with the
    distributions of the nearest time window (``max_workers`` is accepted and
    ignored: there is no process pool here)."""
    return _apply('local_qdm_bc', data,
                  dict(base_dset=base_dset, feature_name=feature_name,
                       bias_fp=bias_fp, threshold=threshold,
                       relative=relative, no_trend=no_trend,
                       delta_denom_min=delta_denom_min,
                       delta_denom_zero=delta_denom_zero,
                       delta_range=delta_range, out_range=out_range),
                  lat_lon, lr_padded_slice,
                  make_time_index(date_range_kwargs))


def local_presrat_bc(data, lat_lon, base_dset, feature_name, bias_fp,
                     date_range_kwargs, lr_padded_slice=None, threshold=0.1,
                     relative=True, no_trend=False, delta_denom_min=None,
                     delta_denom_zero=None, delta_range=None, k_range=None,
                     out_range=None, max_workers=1):
    """bias_transforms.py:958-1137: QDM, then the zero rate (values below
    ``tau_fut`` become 0) and the ``k_factor`` of PresRat."""
    return _apply('local_presrat_bc', data,
                  dict(base_dset=base_dset, feature_name=feature_name,
                       bias_fp=bias_fp, threshold=threshold,
                       relative=relative, no_trend=no_trend,
                       delta_denom_min=delta_denom_min,
                       delta_denom_zero=delta_denom_zero,
                       delta_range=delta_range, k_range=k_range,
                       out_range=out_range),
                  lat_lon, lr_padded_slice,
                  make_time_index(date_range_kwargs))


def correct_chunk_host(chunk, lr_features):
    """A padded chunk carrying a ``bias_correct`` record, corrected the way
    the reference orders it — the un-padded window through the functions
    above, then the reflect padding again — for the executor's routes that
    normalise on the host.  Returns the corrected ``input_data``."""
    rec = chunk.bias_correct
    fn = globals()[rec.method]
    data = np.asarray(chunk.input_data)
    pw = tuple(tuple(p) for p in chunk.pad_width)
    core = tuple(slice(lo, n - hi) for (lo, hi), n in zip(pw, data.shape))
    out = np.array(data[core], dtype=np.float32)
    lower = [f.lower() for f in lr_features]
    for feature, kw in rec.kwargs.items():
        if feature.lower() not in lower:
            raise ValueError(
                f'bias_correct_kwargs names "{feature}", the model\'s '
                f'low-res features are {list(lr_features)}')
        i = lower.index(feature.lower())
        kw = dict(kw)
        kw.setdefault('feature_name', feature)
        kw['lr_padded_slice'] = rec.lr_pad_slice
        if rec.method in TIME_METHODS:
            kw['date_range_kwargs'] = rec.time_index
        if rec.method == 'global_linear_bc':
            kw.pop('feature_name')
            kw.pop('lr_padded_slice')
            out[..., i] = fn(out[..., i], **kw)
        else:
            out[..., i] = fn(out[..., i], rec.lat_lon, **kw)
    return np.pad(out, (*pw, (0, 0)), mode='reflect')
