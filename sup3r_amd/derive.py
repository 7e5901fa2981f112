"""Deriving input features on the device: ``sup3r.preprocessing.derivers``.

The reference's ``Deriver`` (derivers/base.py) turns the loaded variables into
the features a model is trained on or fed.  ``DeviceDeriver`` (also exported as
``Deriver``) keeps its constructor, its registry lookup and its control flow
(``derive``, ``check_registry``, ``_get_inputs``, ``no_overlap``,
``map_new_name``, ``has_interp_variables``, ``get_single_level_data``,
``get_multi_level_data``, ``do_level_interpolation``: base.py:83-410) and works
over arrays in the place of files: ``DeriveData`` stands in for the ``Sup3rX``
dataset.  Features stay planar, one ``(s1, s2, t)`` device tensor each, until
``as_array`` stacks them into the ``(s1, s2, t, C)`` cube the samplers and
``ArrayStrategy`` take.

The arithmetic sits behind a backend object.  ``DeviceBackend`` calls five
entry points (include/sup3r_hip.h, csrc/kernels_derive.hip):

    s3_level_interp      Interpolator.interp_to_level (utilities/
                         interpolation.py:13-173) for all variables and target
                         levels of one level structure, in one pass
    s3_derive_pointwise  the compute() methods of derivers/methods.py
    s3_time_flags        per step: any clearsky_ghi <= 1 / any NaN
    s3_stack_features    planes -> channels-last cube, ``time_roll`` fused
    s3_level_stats       the counts and extrema of ``run_level_check``

(and four more for the data handlers, data_handlers.py over
csrc/kernels_data_handler.hip: ``raster_gather``, ``daily_reduce``,
``site_day_mean``, ``scale_to_time_max``; and two for the dual rasterizer,
dual_rasterizer.py over csrc/kernels_regrid.hip: ``regrid_knn``,
``regrid_apply``).
``NumpyBackend`` is the same arithmetic restated in numpy, for testing the
host control flow on a machine without a GPU; it is no fallback: nothing
selects it but the caller.

Beyond the reference the constructor plans before it launches: a dry pass of
the control flow collects every feature that falls to level interpolation and
groups them by level structure (the multi-level variable's level source and
``L``, and the levels of the single-level companions ``u_10m``, ``u_100m``,
...); one launch then serves all variables and all requested heights of a
group.  ``UWind`` / ``VWind`` (``Windspeed`` / ``Winddirection``, ``USolar`` /
``VSolar``) compute both members of the pair in one launch and hand the other
to its sibling.

Deviations from the reference, on purpose:
  * the companions of a group are the single-level features loaded when the
    deriver was made: a height derived in this pass (``u_40m``) is not fed
    back as a level of a later one (``u_100m``), as the reference's
    one-feature-at-a-time order does;
  * ``CloudMask`` applies the night mask to the time axis, as
    ``ClearSkyRatio`` does (methods.py:160 indexes the first axis with a
    ``(t,)`` mask); its ``inputs`` keep the reference's spelling
    ``clearky_ghi``, so the registry cannot reach it there or here;
  * ``hr_spatial_coarsen`` is a plain block mean (``s3_coarsen``); xarray's
    ``coarsen().mean()`` skips NaNs;
  * ``run_level_check`` checks a group's level array once, for all its
    targets, from a 64-byte read-back of ``s3_level_stats`` (the
    single-level constants are folded in on the host);
  * ``Sza`` needs rex's ``SolarPosition``: the key stays in the registries,
    ``compute`` raises ``NotImplementedError``;
  * ``nan_method_kwargs`` other than ``{'method': 'mask'}`` on data that holds
    NaNs raises ``NotImplementedError`` (xarray's ``interpolate_na``).

Not here: reading or rasterising files, caching, the dask chunking arguments,
``ExoRasterizer``, and fusing the derivation into the sampler's gather.
"""
import copy
import ctypes as C
import logging
import re
import warnings
from inspect import signature
from warnings import warn

import numpy as np

from . import _lib
from .output_transform import grid_theta

logger = logging.getLogger(__name__)

# (the two backends are reached as sup3r_amd.derive.DeviceBackend /
# NumpyBackend: bias_calc has a DeviceBackend of its own)
__all__ = ['DeriveData', 'DeviceDeriver', 'Deriver', 'parse_feature',
           'get_feature_basename', 'DerivedFeature', 'SurfaceRH',
           'ClearSkyRatio', 'ClearSkyRatioCC', 'CloudMask', 'PressureWRF',
           'Windspeed', 'Winddirection', 'UWind', 'VWind', 'USolar', 'VSolar', 'UWindPowerLaw', 'VWindPowerLaw',
           'TempNCforCC', 'Tas', 'TasMin', 'TasMax', 'Sza', 'Latitude',
           'Longitude', 'SecondOfDayEncoding', 'SecondOfYearEncoding',
           'RegistryBase', 'RegistryH5WindCC', 'RegistryH5SolarCC',
           'RegistryNCforCC', 'RegistryNCforCCwithPowerLaw']


# ------------------------------------------------------------ feature names
def get_feature_basename(feature):
    """Feature name without its height / pressure suffix
    (utilities/utilities.py:78-92)."""
    height = re.findall(r'_\d+m', feature)
    press = re.findall(r'_\d+pa', feature)
    if height:
        return feature.replace(height[0], '')
    if press:
        return feature.replace(press[0], '')
    if '_(.*)' in feature:
        return feature.split('_(.*)')[0]
    return feature


class FeatureStruct:
    """``basename``, ``height`` and ``pressure`` of a feature name
    (derivers/utilities.py:92-117)"""

    def __init__(self, feature):
        height = re.findall(r'_\d+m', feature)
        press = re.findall(r'_\d+pa', feature)
        self.basename = get_feature_basename(feature)
        self.height = int(round(float(height[0][1:-1]))) if height else None
        self.pressure = int(round(float(press[0][1:-2]))) if press else None

    def map_wildcard(self, pattern):
        """the pattern with its wildcard replaced by the height, else the
        pressure, else dropped"""
        if '(.*)' not in pattern:
            return pattern
        head = pattern.split('_(.*)')[0]
        if self.height is not None:
            return f'{head}_{self.height}m'
        if self.pressure is not None:
            return f'{head}_{self.pressure}pa'
        return head


def parse_feature(feature):
    """derivers/utilities.py:88-119"""
    return FeatureStruct(feature)


def lowered(features):
    """preprocessing/utilities.py:563-575"""
    feats = (features.lower() if isinstance(features, str)
             else [f.lower() if isinstance(f, str) else f for f in features])
    was = [features] if isinstance(features, str) else list(features)
    now = [feats] if isinstance(feats, str) else list(feats)
    if was != now:
        msg = (f'Received some upper case features: {was}. '
               f'Using {now} instead.')
        logger.warning(msg)
        warn(msg)
    return feats


# ----------------------------------------------------------------- backends
_SEC_PER_DAY, _SEC_PER_YEAR = 86400, 31536000


def _select_levels(lev, target):
    """get_level_masks (interpolation.py:17-70) as indices: ``lev`` (P, L)
    float32, NaN levels are never candidates, ties take the lowest index, an
    empty candidate set gives index 0.  Returns ``(i1, i2)`` (P,)."""
    valid = ~np.isnan(lev)
    with np.errstate(invalid='ignore'):
        d = np.abs(lev - target)
        below = valid & (lev < target)
        above = valid & (lev >= target)

    def argmin(mask):
        idx = np.argmin(np.where(mask, d, np.inf), axis=-1)
        missed = mask.any(-1) & ~np.take_along_axis(
            mask, idx[:, None], -1)[:, 0]        # every candidate at inf
        return np.where(missed, np.argmax(mask, axis=-1), idx)

    i1 = np.where(below.any(-1), argmin(below), argmin(valid))
    others = valid.copy()
    np.put_along_axis(others, i1[:, None], False, -1)
    i2 = np.where(above.any(-1), argmin(above), argmin(others))
    return i1, i2


class NumpyBackend:
    """The backend's operations in numpy float32, the reference's expressions
    restated.  For tests of the host control flow."""

    name = 'numpy'

    def asarray(self, x):
        if hasattr(x, 'detach'):
            x = x.detach().cpu().numpy()
        return np.ascontiguousarray(np.asarray(x, dtype=np.float32))

    def to_numpy(self, x):
        return np.asarray(x)

    def level_interp(self, lev, var_ml, var_sl, sl_levels, targets,
                     method='linear'):
        """``lev``: ``('column', zg (P.., L), topo | None)``, ``('vector',
        (L,))`` or None; ``var_ml``: n_var arrays (s1, s2, t, L) (or empty);
        ``var_sl``: n_var lists of n_sl planes; returns n_var lists of
        n_out planes"""
        shape = (var_ml[0].shape[:3] if len(var_ml) else var_sl[0][0].shape)
        P = int(np.prod(shape))
        cols = []
        if lev is not None and lev[0] == 'column':
            zg = lev[1].reshape(P, -1)
            if lev[2] is not None:
                topo = lev[2]
                topo = (np.broadcast_to(topo[..., None], shape)
                        if topo.ndim == 2 else topo)
                zg = zg - topo.reshape(P, 1)
            cols.append(zg)
        elif lev is not None:
            vec = np.asarray(lev[1], np.float32)
            cols.append(np.broadcast_to(vec, (P, len(vec))))
        if len(sl_levels):
            sl = np.asarray(sl_levels, np.float32)
            cols.append(np.broadcast_to(sl, (P, len(sl))))
        levs = np.concatenate(cols, axis=-1).astype(np.float32)
        out = [[None] * len(targets) for _ in range(len(var_sl) or
                                                    len(var_ml))]
        n_var = len(out)
        full = []
        for v in range(n_var):
            parts = []
            if len(var_ml):
                parts.append(var_ml[v].reshape(P, -1))
            parts += [p.reshape(P, 1) for p in (var_sl[v] if var_sl else [])]
            full.append(np.concatenate(parts, axis=-1))
        for k, tg in enumerate(targets):
            tg = np.float32(tg)
            i1, i2 = _select_levels(levs, tg)
            l1 = np.take_along_axis(levs, i1[:, None], -1)[:, 0]
            l2 = np.take_along_axis(levs, i2[:, None], -1)[:, 0]
            for v in range(n_var):
                v1 = np.take_along_axis(full[v], i1[:, None], -1)[:, 0]
                v2 = np.take_along_axis(full[v], i2[:, None], -1)[:, 0]
                with np.errstate(all='ignore'):
                    if method == 'log':
                        r = self._log(l1, l2, v1, v2, tg)
                    else:
                        diff = l2 - l1
                        alpha = np.where(np.abs(diff) < np.float32(1e-3),
                                         np.float32(0), (tg - l1) / diff)
                        r = v1 * (1 - alpha) + v2 * alpha
                out[v][k] = r.astype(np.float32).reshape(shape)
        return out

    @staticmethod
    def _log(l1, l2, v1, v2, level):
        """_log_interp (interpolation.py:95-112)"""
        mask = l1 < l2
        h0, h1 = np.where(mask, l1, l2), np.where(mask, l2, l1)
        w0, w1 = np.where(mask, v1, v2), np.where(mask, v2, v1)
        coeff = np.where(h1 == h0, np.float32(0),
                         (w1 - w0) / np.log(h1 - h0 + 1))
        coeff = np.where(level < h0, -coeff, coeff)
        return coeff * np.log(np.abs(level - h0) + 1) + w0

    def uv_from_wswd(self, ws, wd, lat_lon):
        """transform_rotate_wind (derivers/utilities.py:146-201); the row
        flip is inside ``grid_theta``"""
        theta = grid_theta(lat_lon)
        wd = np.radians(wd)
        ct, st = np.cos(theta)[:, :, None], np.sin(theta)[:, :, None]
        u = ct * ws * np.sin(wd)
        u += st * ws * np.cos(wd)
        v = -st * ws * np.sin(wd)
        v += ct * ws * np.cos(wd)
        return u.astype(np.float32), v.astype(np.float32)

    def wswd_from_uv(self, u, v, lat_lon):
        """invert_uv (:204-258)"""
        theta = grid_theta(lat_lon)
        ct, st = np.cos(theta)[:, :, None], np.sin(theta)[:, :, None]
        u_rot = ct * u
        u_rot -= st * v
        v_rot = st * u
        v_rot += ct * v
        ws = np.hypot(u_rot, v_rot)
        wd = (np.degrees(np.arctan2(u_rot, v_rot)) + 360) % 360
        return ws.astype(np.float32), wd.astype(np.float32)

    def surface_rh(self, d2m, t2m):
        wvp = 6.1078 * np.exp(17.1 * d2m / (235 + d2m))
        sat = 6.1078 * np.exp(17.1 * t2m / (235 + t2m))
        return (100 * wvp / sat).astype(np.float32)

    def time_flags(self, x, mode, threshold=0.0):
        """(t,) int32 flags of a plane (s1, s2, t) or a cube (s1, s2, t, C)"""
        with np.errstate(invalid='ignore'):
            hit = np.isnan(x) if mode == 'nan' else x <= np.float32(threshold)
        axes = (0, 1) if x.ndim == 3 else (0, 1, 3)
        return hit.any(axis=axes).astype(np.int32)

    def flags_to_numpy(self, flags):
        return np.asarray(flags)

    def ratio_masked(self, a, b, flags):
        with np.errstate(all='ignore'):
            r = (a / b).astype(np.float32)
        r[..., np.asarray(flags, bool)] = np.nan
        return r

    def cloud_mask(self, a, b, flags):
        r = (a < b).astype(np.float32)
        r[..., np.asarray(flags, bool)] = np.nan
        return r

    def ratio_clip01(self, a, b):
        with np.errstate(all='ignore'):
            r = np.minimum(a / b, 1)
            return np.maximum(r, 0).astype(np.float32)

    def add(self, a, b):
        return a + b

    def scale(self, a, factor):
        return a * np.float32(factor)

    def offset(self, a, delta):
        return a + np.float32(delta)

    def broadcast_pixel(self, plane2d, t):
        p = np.asarray(plane2d, np.float32)
        return np.ascontiguousarray(np.repeat(p[..., None], t, axis=-1))

    def broadcast_time(self, vec, s1, s2):
        v = np.asarray(vec, np.float32)
        return np.ascontiguousarray(np.broadcast_to(v, (s1, s2, len(v))))

    def level_stats(self, zg, topo, lo, hi):
        """the figures of ``_check_lev_array`` of ``zg - topo``: see
        ``level_check``; of ``zg`` itself when ``topo`` is None"""
        if topo is not None:
            topo = topo[..., None] if topo.ndim == 2 else topo
            zg = zg - topo[..., None]
        lev = zg.reshape(-1, zg.shape[-1])
        nan = np.isnan(lev)
        clean = ~nan.any(-1)
        with np.errstate(all='ignore'), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            out = {'size': lev.size, 'columns': len(lev), 'nan': int(nan.sum()),
                   'all_nan': int(nan.all(-1).sum()),
                   'bad_min': int((clean & (np.float32(lo)
                                            < np.nanmin(lev, -1))).sum()),
                   'bad_max': int((clean & (np.float32(hi)
                                            > np.nanmax(lev, -1))).sum()),
                   'first': (float(np.nanmin(lev[:, 0])),
                             float(np.nanmax(lev[:, 0]))),
                   'last': (float(np.nanmin(lev[:, -1])),
                            float(np.nanmax(lev[:, -1])))}
        return out

    def stack(self, planes, roll=0):
        cube = np.stack(planes, axis=-1).astype(np.float32)
        return np.roll(cube, roll, axis=2) if roll else cube

    def coarsen(self, cube, s):
        s1, s2, t, c = cube.shape
        cube = cube[:s1 - s1 % s, :s2 - s2 % s]
        r = cube.reshape(s1 // s, s, s2 // s, s, t, c)
        return (r.sum(axis=(1, 3), dtype=np.float32)
                * np.float32(1.0 / (s * s))).astype(np.float32)

    def take_steps(self, cube, keep):
        return np.ascontiguousarray(cube[:, :, np.asarray(keep)])

    def channel(self, cube, i):
        return np.ascontiguousarray(cube[..., i])


    # -- the data handlers' operations (data_handlers.py)
    DAILY_OPS = ('mean', 'max', 'min', 'sum', 'ratio')

    def raster_gather(self, arrays, rows=None, cols=None, t0=0, step=1,
                      n_k=1, site=None):
        """``site`` None: ``a[rows, cols, t0 : : step][.., :n_k]`` of gridded
        ``(s1, s2, t [, L])`` arrays (a 2-D array has no time axis); else the
        raster ``site`` (n_i, n_j) of flat ``(t, sites)`` / ``(sites,)``
        arrays as ``(n_i, n_j, n_k)`` / ``(n_i, n_j)``.  Bits are copied."""
        steps = slice(t0, t0 + (n_k - 1) * step + 1, step)
        out = []
        for a in arrays:
            a = np.asarray(a)
            if site is None:
                a = a[rows, cols] if a.ndim == 2 else a[rows, cols, steps]
            elif a.ndim == 1:
                a = a[site]
            else:
                a = np.moveaxis(a[steps][:, site], 0, -1)
            out.append(np.ascontiguousarray(a))
        return out

    def daily_reduce(self, sources, w, outputs):
        """``sources``: planes (s1, s2, D w); ``outputs``: (source, second
        source | None, op in DAILY_OPS) each; returns planes (s1, s2, D).
        xarray's ``coarsen(time=w).mean() / .max() / .min() / .sum()`` with
        NaN skipped, in float64, rounded to float32 once; ``ratio`` is the
        float32 quotient of the two float32 sums."""
        wins = [np.asarray(a, np.float64).reshape(*a.shape[:2], -1, w)
                for a in sources]
        fn = {'mean': np.nanmean, 'max': np.nanmax, 'min': np.nanmin,
              'sum': np.nansum}
        out = []
        with np.errstate(all='ignore'), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for i, j, op in outputs:
                if op == 'ratio':
                    a = np.nansum(wins[i], axis=-1).astype(np.float32)
                    b = np.nansum(wins[j], axis=-1).astype(np.float32)
                    out.append(a / b)
                else:
                    out.append(fn[op](wins[i], axis=-1).astype(np.float32))
        return out

    def site_day_mean(self, src, idx, t_lo, m, day_map):
        """``src`` (t, sites), ``idx`` (n_pix, k), ``day_map`` (D,): ``out[p,
        d]`` = NaN where ``day_map[d] < 0``, else the NaN-skipping mean over
        the ``m`` steps of source day ``day_map[d]`` (counted from ``t_lo``)
        of the NaN-skipping mean over the ``k`` sites; float64, one rounding"""
        src = np.asarray(src, np.float64)
        idx, day_map = np.asarray(idx), np.asarray(day_map)
        n_days = (len(src) - t_lo) // m
        with np.errstate(all='ignore'), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            sites = np.nanmean(src[t_lo:t_lo + n_days * m][:, idx], axis=-1)
            days = np.nanmean(sites.reshape(n_days, m, -1), axis=1)   # (d, p)
        ok = (day_map >= 0) & (day_map < n_days)
        out = np.full((idx.shape[0], len(day_map)), np.nan, np.float32)
        out[:, ok] = days[day_map[ok]].T.astype(np.float32)
        return out

    def scale_to_time_max(self, a, b):
        """``scale = nanmax_t a / nanmax_t b`` per pixel (float32), ``b *
        scale``: returns ``(b scaled, scale)``"""
        with np.errstate(all='ignore'), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            scale = (np.nanmax(a, axis=-1) / np.nanmax(b, axis=-1)).astype(
                np.float32)
            return (b * scale[..., None]).astype(np.float32), scale

    # -- the regridder's operations (dual_rasterizer.py)
    def regrid_knn(self, src_lat_lon, tgt_lat_lon, k):
        """the ``k`` nearest of the sources ``(n_src, 2)`` (lat, lon, degrees)
        for every target ``(n_tgt, 2)``, by the device's rules
        (``s3_regrid_knn``): float32 inputs widened to float64, the haversine
        distance in radians by brute force, candidates in ``(distance, id)``
        order, rex's float32 inverse-distance weights.  Returns the handle
        ``regrid_apply`` takes: ``idx`` int32, ``dist`` float64 and ``w``
        float32, all ``(n_tgt, k)``."""
        src = np.deg2rad(np.asarray(src_lat_lon, np.float32).reshape(-1, 2)
                         .astype(np.float64))
        tgt = np.deg2rad(np.asarray(tgt_lat_lon, np.float32).reshape(-1, 2)
                         .astype(np.float64))
        n, m, k = len(src), len(tgt), int(k)
        if not 1 <= k <= _lib.REGRID_MAX_K or n < k or m < 1:
            raise ValueError(f'regrid_knn: k = {k} with {n} sources and {m} '
                             f'targets (1 <= k <= {_lib.REGRID_MAX_K}, '
                             'k <= n_src, 1 <= n_tgt)')
        if not (np.isfinite(src).all() and np.isfinite(tgt).all()):
            raise ValueError('regrid_knn: a coordinate that is not finite')
        cos_s = np.cos(src[:, 0])
        idx = np.empty((m, k), np.int32)
        dist = np.empty((m, k), np.float64)
        step = max(1, (1 << 21) // n)
        for at in range(0, m, step):
            t = tgt[at:at + step]
            s0 = np.sin(0.5 * (t[:, None, 0] - src[None, :, 0]))
            s1 = np.sin(0.5 * (t[:, None, 1] - src[None, :, 1]))
            h = s0 * s0 + np.cos(t[:, None, 0]) * cos_s[None] * s1 * s1
            d = 2.0 * np.arcsin(np.sqrt(np.minimum(h, 1.0)))
            # stable: equal distances stay in id order
            first = np.argsort(d, axis=1, kind='stable')[:, :k]
            idx[at:at + step] = first
            dist[at:at + step] = np.take_along_axis(d, first, axis=1)
        return {'idx': idx, 'dist': dist, 'w': self.regrid_weights(dist),
                'n_src': n, 'n_tgt': m, 'k': k}

    @staticmethod
    def regrid_weights(dist):
        """rex's weights: float32 distances floored at 1e-12, their
        reciprocals, divided by their sum taken left to right"""
        d = np.asarray(dist).astype(np.float32)
        d[d < np.float32(1e-12)] = np.float32(1e-12)
        w = np.float32(1.0) / d
        total = w[:, 0].copy()
        for q in range(1, w.shape[1]):
            total = total + w[:, q]
        return (w / total[:, None]).astype(np.float32)

    def regrid_apply(self, handle, planes, t_out):
        """``out[j, t] = float32(sum_k float64(w[j, k]) float64(plane[idx[j,
        k], t]))`` for ``t < t_out``, the sum in rank order from the first
        product (``s3_regrid_apply``); planes ``(s1, s2, T)`` or ``(n_src,
        T)``.  Returns ``(planes (n_tgt, t_out), NaN count of each)``."""
        idx, w = handle['idx'].astype(np.int64), handle['w'].astype(np.float64)
        outs, counts = [], []
        with np.errstate(all='ignore'):
            for a in planes:
                a = np.asarray(a, np.float32)
                rows = a.reshape(handle['n_src'], a.shape[-1])
                if not 1 <= t_out <= rows.shape[1]:
                    raise ValueError('regrid_apply: 1 <= t_out <= T is needed')
                rows = rows[:, :t_out]
                acc = w[:, 0, None] * rows[idx[:, 0]].astype(np.float64)
                for q in range(1, handle['k']):
                    acc = acc + w[:, q, None] * rows[idx[:, q]].astype(
                        np.float64)
                outs.append(acc.astype(np.float32))
                counts.append(int(np.isnan(outs[-1]).sum()))
        return outs, np.asarray(counts, np.int64)

    def to_index(self, x):
        return np.ascontiguousarray(x, dtype=np.int32)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class DeviceBackend:
    """The same operations on device tensors through the C ABI.  A missing
    kernel is an error: nothing is routed to numpy or torch arithmetic."""

    name = 'device'

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

    def asarray(self, x):
        return self.dev.to_device(x)

    def to_numpy(self, x):
        return x.detach().cpu().numpy()

    def _pointers(self, tensors):
        return (C.c_void_p * max(len(tensors), 1))(
            *[t.data_ptr() for t in tensors])

    # -- kernels
    def level_interp(self, lev, var_ml, var_sl, sl_levels, targets,
                     method='linear', out=None):
        """as ``NumpyBackend.level_interp``; ``out``: n_var lists of n_out
        planes to write into (default: new ones)"""
        n_var = len(var_sl) or len(var_ml)
        shape = tuple(var_ml[0].shape[:3] if len(var_ml)
                      else var_sl[0][0].shape)
        P, t = int(np.prod(shape)), int(shape[2])
        l_ml = int(var_ml[0].shape[3]) if len(var_ml) else 0
        source, lev_ml, topo, per_step, vec = _lib.LI_LEV_VECTOR, None, None, 0, None
        if lev is not None and lev[0] == 'column':
            source, lev_ml, topo = _lib.LI_LEV_COLUMN, lev[1], lev[2]
            per_step = int(topo is not None and topo.dim() == 3)
        elif lev is not None:
            vec = np.ascontiguousarray(lev[1], dtype=np.float32)
        sl = np.ascontiguousarray(sl_levels, dtype=np.float32)
        tg = np.ascontiguousarray(targets, dtype=np.float32)
        flat_sl = [p for planes in (var_sl or []) for p in planes]
        if out is None:
            out = [[self.dev.empty(shape) for _ in tg] for _ in range(n_var)]
        flat_out = [p for planes in out for p in planes]
        self._call(
            's3_level_interp', P, t, l_ml, len(sl), source, _ptr(lev_ml),
            _fp(vec) if vec is not None else None, _ptr(topo), per_step,
            _fp(sl) if len(sl) else None, n_var,
            self._pointers(list(var_ml)) if l_ml else None,
            self._pointers(flat_sl) if len(sl) else None, len(tg), _fp(tg),
            _lib.LI_LOG if method == 'log' else _lib.LI_LINEAR,
            self._pointers(flat_out))
        return out

    def pointwise(self, op, shape, in0, in1=None, theta=None, flags=None,
                  p0=0.0, n_out=1):
        s1, s2, t = (int(v) for v in shape)
        out = [self.dev.empty(shape) for _ in range(n_out)]
        cs, sn = theta if theta is not None else (None, None)
        self._call('s3_derive_pointwise', op, s1 * s2, t, _ptr(in0),
                   _ptr(in1), _ptr(cs), _ptr(sn), _ptr(flags), float(p0),
                   _ptr(out[0]), _ptr(out[1]) if n_out > 1 else None)
        return out[0] if n_out == 1 else tuple(out)

    def _theta(self, lat_lon):
        theta = grid_theta(lat_lon)
        return (self.asarray(np.cos(theta).astype(np.float32)),
                self.asarray(np.sin(theta).astype(np.float32)))

    def uv_from_wswd(self, ws, wd, lat_lon):
        return self.pointwise(_lib.DP_UV_FROM_WSWD, ws.shape, ws, wd,
                              theta=self._theta(lat_lon), n_out=2)

    def wswd_from_uv(self, u, v, lat_lon):
        return self.pointwise(_lib.DP_WSWD_FROM_UV, u.shape, u, v,
                              theta=self._theta(lat_lon), n_out=2)

    def surface_rh(self, d2m, t2m):
        return self.pointwise(_lib.DP_SURFACE_RH, d2m.shape, d2m, t2m)

    def time_flags(self, x, mode, threshold=0.0):
        import torch
        s1, s2, t = (int(v) for v in x.shape[:3])
        c = int(x.shape[3]) if x.dim() == 4 else 1
        flags = torch.empty(t, dtype=torch.int32, device=x.device)
        self._call('s3_time_flags',
                   _lib.TF_NAN if mode == 'nan' else _lib.TF_LE, _ptr(x),
                   s1 * s2, t, c, float(threshold), _ptr(flags))
        return flags

    def flags_to_numpy(self, flags):
        return flags.cpu().numpy()

    def ratio_masked(self, a, b, flags):
        return self.pointwise(_lib.DP_RATIO_MASKED, a.shape, a, b, flags=flags)

    def cloud_mask(self, a, b, flags):
        return self.pointwise(_lib.DP_CLOUD_MASK, a.shape, a, b, flags=flags)

    def ratio_clip01(self, a, b):
        return self.pointwise(_lib.DP_RATIO_CLIP01, a.shape, a, b)

    def add(self, a, b):
        return self.pointwise(_lib.DP_ADD, a.shape, a, b)

    def scale(self, a, factor):
        return self.pointwise(_lib.DP_SCALE, a.shape, a, p0=np.float32(factor))

    def offset(self, a, delta):
        return self.pointwise(_lib.DP_OFFSET, a.shape, a, p0=np.float32(delta))

    def broadcast_pixel(self, plane2d, t):
        p = self.asarray(np.asarray(plane2d, np.float32))
        return self.pointwise(_lib.DP_BCAST_PIXEL, (*p.shape, int(t)), p)

    def broadcast_time(self, vec, s1, s2):
        v = self.asarray(np.asarray(vec, np.float32))
        return self.pointwise(_lib.DP_BCAST_TIME, (s1, s2, len(vec)), v)

    def level_stats(self, zg, topo, lo, hi):
        import torch
        s1, s2, t, n_lev = (int(v) for v in zg.shape)
        st = torch.empty(_lib.LS_WORDS, dtype=torch.int64, device=zg.device)
        self._call('s3_level_stats', _ptr(zg), s1 * s2 * t, t, n_lev,
                   _ptr(topo), int(topo is not None and topo.dim() == 3),
                   float(lo), float(hi), _ptr(st))
        w = [int(v) for v in st.cpu().numpy()]

        def value(key):
            """the float behind an order key (include/sup3r_hip.h)"""
            bits = key & 0x7FFFFFFF if key & 0x80000000 else ~key & 0xFFFFFFFF
            return float(np.array([bits], np.uint32).view(np.float32)[0])

        def pair(mx, mn):
            return ((value(0xFFFFFFFF - w[mn]), value(w[mx])) if w[mx]
                    else (float('nan'), float('nan')))
        return {'size': s1 * s2 * t * n_lev, 'columns': s1 * s2 * t,
                'nan': w[_lib.LS_NAN], 'all_nan': w[_lib.LS_ALL_NAN],
                'bad_min': w[_lib.LS_BAD_MIN], 'bad_max': w[_lib.LS_BAD_MAX],
                'first': pair(_lib.LS_FIRST_MAX, _lib.LS_FIRST_MIN),
                'last': pair(_lib.LS_LAST_MAX, _lib.LS_LAST_MIN)}

    def stack(self, planes, roll=0):
        s1, s2, t = (int(v) for v in planes[0].shape)
        out = self.dev.empty((s1, s2, t, len(planes)))
        self._call('s3_stack_features', self._pointers(list(planes)),
                   len(planes), s1 * s2, t, int(roll), _ptr(out))
        return out

    def coarsen(self, cube, s):
        s1, s2, t, c = (int(v) for v in cube.shape)
        cube = cube[:s1 - s1 % s, :s2 - s2 % s].contiguous()
        out = self.dev.empty((s1 // s, s2 // s, t, c))
        self._call('s3_coarsen', _ptr(cube), 1, s1 - s1 % s, s2 - s2 % s, t,
                   c, int(s), 1, 0, _ptr(out))
        return out

    def take_steps(self, cube, keep):
        import torch
        idx = torch.from_numpy(np.asarray(keep, np.int64)).to(cube.device)
        return torch.index_select(cube, 2, idx).contiguous()

    def channel(self, cube, i):
        return cube[..., i].contiguous()


    # -- the data handlers' kernels (csrc/kernels_data_handler.hip)
    DAILY_OPS = NumpyBackend.DAILY_OPS

    def to_index(self, x):
        """an int32 table on the device"""
        import torch
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(
            self.dev.torch_device)

    def _gather(self, layout, arrays, out_shape, n_k, n_lev, src, r0, c0, t0,
                step, site):
        n_i, n_j = out_shape[:2]
        outs = []
        for at in range(0, len(arrays), _lib.STACK_MAX_PLANES):
            part = list(arrays[at:at + _lib.STACK_MAX_PLANES])
            new = [self.dev.empty(out_shape) for _ in part]
            self._call('s3_raster_gather', layout, len(part),
                       self._pointers(part), self._pointers(new), n_i, n_j,
                       n_k, n_lev, *src, r0, c0, t0, step, _ptr(site))
            outs += new
        return outs

    def raster_gather(self, arrays, rows=None, cols=None, t0=0, step=1,
                      n_k=1, site=None):
        """as ``NumpyBackend.raster_gather``: arrays of one geometry share a
        launch (``s3_raster_gather``)"""
        arrays = [a.contiguous() for a in arrays]
        out = [None] * len(arrays)
        groups = {}
        for i, a in enumerate(arrays):
            groups.setdefault(tuple(a.shape), []).append(i)
        if site is not None:
            site_np = np.asarray(site)
            n_i, n_j = site_np.shape
            table = self.to_index(site_np.reshape(-1))
        for shape, members in groups.items():
            part = [arrays[i] for i in members]
            if site is None:
                r = range(*rows.indices(shape[0]))
                c = range(*cols.indices(shape[1]))
                assert r.step == 1 and c.step == 1 and len(r) and len(c)
                flat2d = len(shape) == 2
                n_lev = shape[3] if len(shape) == 4 else 1
                o_shape = (len(r), len(c)) if flat2d else (
                    (len(r), len(c), n_k) + ((n_lev,) if len(shape) == 4
                                             else ()))
                new = self._gather(
                    _lib.RG_GRID, part, o_shape, 1 if flat2d else n_k, n_lev,
                    (shape[0], shape[1], 1 if flat2d else shape[2]),
                    r.start, c.start, 0 if flat2d else t0,
                    1 if flat2d else step, None)
            else:
                if site_np.size and (site_np.min() < 0
                                     or site_np.max() >= shape[-1]):
                    raise IndexError(
                        f'raster_index outside the {shape[-1]} sites')
                if len(shape) == 1:
                    new = self._gather(_lib.RG_FLAT_1D, part, (n_i, n_j), 1,
                                       1, (1, shape[0], 1), 0, 0, 0, 1, table)
                else:
                    new = self._gather(_lib.RG_FLAT, part, (n_i, n_j, n_k),
                                       n_k, 1, (1, shape[1], shape[0]), 0, 0,
                                       t0, step, table)
            for i, plane in zip(members, new):
                out[i] = plane
        return out

    def daily_reduce(self, sources, w, outputs):
        """as ``NumpyBackend.daily_reduce`` (``s3_daily_reduce``): one launch
        while the tables hold the sources and outputs, else one per run of
        outputs that fits"""
        s1, s2, t = (int(v) for v in sources[0].shape)
        assert t % w == 0, (t, w)
        days = t // w
        sources = [a.contiguous() for a in sources]
        out = [self.dev.empty((s1, s2, days)) for _ in outputs]
        ops = {name: i for i, name in enumerate(self.DAILY_OPS)}
        launch, used = [], []

        def flush():
            if not launch:
                return
            slot = {s: i for i, s in enumerate(used)}
            n = len(launch)
            i32 = C.c_int32 * n
            self._call(
                's3_daily_reduce', len(used),
                self._pointers([sources[s] for s in used]), s1 * s2, days,
                int(w), n, i32(*[slot[outputs[o][0]] for o in launch]),
                i32(*[slot.get(outputs[o][1], 0) for o in launch]),
                i32(*[ops[outputs[o][2]] for o in launch]),
                self._pointers([out[o] for o in launch]))
            launch.clear()
            used.clear()
        for o, (i, j, op) in enumerate(outputs):
            wanted = list(dict.fromkeys((i, j) if op == 'ratio' else (i,)))
            need = [s for s in wanted if s not in used]
            if (len(used) + len(need) > _lib.DAILY_MAX_SRC
                    or len(launch) + 1 > _lib.DAILY_MAX_OUT):
                flush()
                need = wanted
            used += need
            launch.append(o)
        flush()
        return out

    def site_day_mean(self, src, idx, t_lo, m, day_map):
        """as ``NumpyBackend.site_day_mean`` (``s3_site_day_mean``)"""
        src = src.contiguous()
        idx = np.asarray(idx)
        n_pix, k = idx.shape
        out = self.dev.empty((n_pix, len(day_map)))
        # (both tables stay referenced until the launch is enqueued: a freed
        # block would be handed to the next allocation)
        idx_d, map_d = self.to_index(idx), self.to_index(day_map)
        self._call('s3_site_day_mean', _ptr(src), int(src.shape[0]),
                   int(src.shape[1]), _ptr(idx_d), n_pix, k, int(t_lo),
                   int(m), _ptr(map_d), len(day_map), _ptr(out))
        return out

    def scale_to_time_max(self, a, b):
        """as ``NumpyBackend.scale_to_time_max``; ``b`` is scaled IN PLACE
        when it is contiguous (``s3_scale_to_time_max``)"""
        a, b = a.contiguous(), b.contiguous()
        s1, s2, t = (int(v) for v in b.shape)
        scale = self.dev.empty((s1, s2))
        self._call('s3_scale_to_time_max', _ptr(a), _ptr(b), s1 * s2, t,
                   _ptr(scale))
        return b, scale

    # -- the regridder's kernels (csrc/kernels_regrid.hip)
    def regrid_knn(self, src_lat_lon, tgt_lat_lon, k):
        """as ``NumpyBackend.regrid_knn`` (``s3_regrid_knn``); the handle's
        tables stay on the device"""
        import torch
        td = self.dev.torch_device
        src = self.asarray(np.ascontiguousarray(
            np.asarray(src_lat_lon, np.float32).reshape(-1, 2)))
        tgt = self.asarray(np.ascontiguousarray(
            np.asarray(tgt_lat_lon, np.float32).reshape(-1, 2)))
        n, m, k = int(src.shape[0]), int(tgt.shape[0]), int(k)
        n_bytes = int(_lib.lib().s3_regrid_knn_work_bytes(n))
        if n_bytes < 0:
            raise ValueError('s3_regrid_knn: 1 .. 2^31 - 1 sources')
        work = torch.empty((n_bytes + 7) // 8, dtype=torch.int64, device=td)
        idx = torch.empty((m, max(k, 1)), dtype=torch.int32, device=td)
        dist = torch.empty((m, max(k, 1)), dtype=torch.float64, device=td)
        w = torch.empty((m, max(k, 1)), dtype=torch.float32, device=td)
        self._call('s3_regrid_knn', _ptr(src), n, _ptr(tgt), m, k, _ptr(work),
                   work.numel() * 8, _ptr(idx), _ptr(dist), _ptr(w))
        return {'idx': idx, 'dist': dist, 'w': w, 'n_src': n, 'n_tgt': m,
                'k': k}

    def regrid_apply(self, handle, planes, t_out):
        """as ``NumpyBackend.regrid_apply``: all planes in one call
        (``s3_regrid_apply``); the NaN counts stay on the device (int64)"""
        import torch
        planes = [a.contiguous() for a in planes]
        n, m = handle['n_src'], handle['n_tgt']
        t_src = int(planes[0].shape[-1])
        for a in planes:
            assert a.numel() == n * t_src, (tuple(a.shape), n, t_src)
        outs = [self.dev.empty((m, max(int(t_out), 1))) for _ in planes]
        counts = torch.empty(len(planes), dtype=torch.int64,
                             device=self.dev.torch_device)
        self._call('s3_regrid_apply', len(planes), self._pointers(planes),
                   self._pointers(outs), n, m, t_src, int(t_out), handle['k'],
                   _ptr(handle['idx']), _ptr(handle['w']), _ptr(counts))
        return outs, counts

# --------------------------------------------------------------- the dataset
class DeriveData:
    """Arrays in the place of the ``Sup3rX`` dataset: ``arrays`` maps a name
    to ``(s1, s2, t)``, or ``(s1, s2, t, L)`` for a multi-level variable
    (``topography`` may be ``(s1, s2)``); ``level`` / ``height`` are the
    ``(L,)`` pressure / height coordinates.  Names are lower case.  The
    arrays go to the backend once, when a deriver binds it, and stay planar."""

    COORDS = ('level', 'height')

    def __init__(self, arrays, lat_lon, time_index, level=None, height=None,
                 attrs=None, backend=None):
        import pandas as pd
        self._arrays = {k.lower(): v for k, v in dict(arrays).items()}
        self.lat_lon = np.asarray(lat_lon)
        self.time_index = (time_index if isinstance(time_index,
                                                    pd.DatetimeIndex)
                           else pd.DatetimeIndex(time_index))
        self.level = None if level is None else np.asarray(level, np.float32)
        self.height = (None if height is None
                       else np.asarray(height, np.float32))
        self.attrs = {k.lower(): dict(v) for k, v in (attrs or {}).items()}
        self.backend = None
        self._pairs = {}              # see _pair
        if backend is not None:
            self.bind(backend)

    def bind(self, backend):
        """hand every array to the backend (an upload for the device one)"""
        if self.backend is not backend:
            self.backend = backend
            self._arrays = {k: backend.asarray(v)
                            for k, v in self._arrays.items()}
        return self

    @property
    def shape(self):
        """(s1, s2, t)"""
        return (*self.lat_lon.shape[:2], len(self.time_index))

    @property
    def features(self):
        return list(self._arrays)

    data_vars = features

    def __contains__(self, name):
        name = name.lower()
        return name in self._arrays or (
            name in self.COORDS and getattr(self, name) is not None)

    def __getitem__(self, name):
        name = name.lower()
        if name in self._arrays:
            return self._arrays[name]
        if name in self.COORDS and getattr(self, name) is not None:
            vec = getattr(self, name)
            return self._as(np.broadcast_to(vec, (*self.shape, len(vec))))
        raise KeyError(name)

    def _as(self, value):
        return self.backend.asarray(value) if self.backend else value

    def __setitem__(self, name, value):
        self._arrays[name.lower()] = self._as(value)

    def clear_pairs(self):
        """drop the halves of (u, v) / (speed, direction) pairs that were
        computed and not asked for"""
        self._pairs.clear()

    def subset(self, features):
        """the dataset restricted to ``features`` (``data[features]``)"""
        out = copy.copy(self)
        out._arrays = {f: self._arrays[f] for f in features}
        return out


# ----------------------------------------------------- derived-feature classes
class DerivedFeature:
    """methods.py:20-48: ``inputs`` name what ``compute`` needs"""

    inputs = ()

    @classmethod
    def compute(cls, data, **kwargs):
        raise NotImplementedError


def _pair(data, key, inputs, make, member):
    """One launch for both members of a pair: the first caller computes and
    takes its half, the sibling takes the other from ``data._pairs`` (keyed
    by the inputs' identity; the entry holds the inputs, so the ids stay
    theirs).  An entry goes when both halves are taken; a half nobody asks
    for stays until ``data.clear_pairs()``, which the deriver calls when it
    is done."""
    ident = (key, *[id(data[i]) for i in inputs])
    if ident not in data._pairs:
        data._pairs[ident] = (make(), [data[i] for i in inputs], set())
    outputs, _, taken = data._pairs[ident]
    taken.add(member)
    if len(taken) == 2:
        del data._pairs[ident]
    return outputs[member]


class SurfaceRH(DerivedFeature):
    """methods.py:51-72, 0 - 100"""

    inputs = ('d2m', 'temperature_2m')

    @classmethod
    def compute(cls, data):
        return data.backend.surface_rh(data['d2m'], data['temperature_2m'])


class ClearSkyRatio(DerivedFeature):
    """methods.py:75-102: NaN at every step with a night pixel"""

    inputs = ('ghi', 'clearsky_ghi')

    @classmethod
    def compute(cls, data):
        be = data.backend
        night = be.time_flags(data['clearsky_ghi'], 'le', 1.0)
        return be.ratio_masked(data['ghi'], data['clearsky_ghi'], night)


class ClearSkyRatioCC(DerivedFeature):
    """methods.py:105-130"""

    inputs = ('rsds', 'clearsky_ghi')

    @classmethod
    def compute(cls, data):
        return data.backend.ratio_clip01(data['rsds'], data['clearsky_ghi'])


class CloudMask(DerivedFeature):
    """methods.py:133-164 (``inputs`` as spelled there)"""

    inputs = ('ghi', 'clearky_ghi')

    @classmethod
    def compute(cls, data):
        be = data.backend
        night = be.time_flags(data['clearsky_ghi'], 'le', 1.0)
        return be.cloud_mask(data['ghi'], data['clearsky_ghi'], night)


class PressureWRF(DerivedFeature):
    """methods.py:167-177"""

    inputs = ('p_(.*)', 'pb_(.*)')

    @classmethod
    def compute(cls, data, height):
        return data.backend.add(data[f'p_{height}m'], data[f'pb_{height}m'])


class Windspeed(DerivedFeature):
    """methods.py:180-194"""

    inputs = ('u_(.*)', 'v_(.*)')

    @classmethod
    def _member(cls, data, height, member):
        names = (f'u_{height}m', f'v_{height}m')
        return _pair(data, 'wswd', names, lambda: data.backend.wswd_from_uv(
            data[names[0]], data[names[1]], data.lat_lon), member)

    @classmethod
    def compute(cls, data, height):
        return cls._member(data, height, 0)


class Winddirection(Windspeed):
    """methods.py:197-210"""

    @classmethod
    def compute(cls, data, height):
        return cls._member(data, height, 1)


class UWindPowerLaw(DerivedFeature):
    """methods.py:213-245"""

    ALPHA = 0.2
    NEAR_SFC_HEIGHT = 10
    inputs = ('uas',)

    @classmethod
    def compute(cls, data, height):
        factor = (float(height) / cls.NEAR_SFC_HEIGHT) ** cls.ALPHA
        return data.backend.scale(data[cls.inputs[0]], factor)


class VWindPowerLaw(UWindPowerLaw):
    """methods.py:248-265"""

    inputs = ('vas',)


class UWind(DerivedFeature):
    """methods.py:268-283"""

    inputs = ('windspeed_(.*)', 'winddirection_(.*)')

    @classmethod
    def _member(cls, data, names, member):
        return _pair(data, 'uv', names, lambda: data.backend.uv_from_wswd(
            data[names[0]], data[names[1]], data.lat_lon), member)

    @classmethod
    def compute(cls, data, height):
        return cls._member(data, (f'windspeed_{height}m',
                                  f'winddirection_{height}m'), 0)


class VWind(UWind):
    """methods.py:286-302"""

    @classmethod
    def compute(cls, data, height):
        return cls._member(data, (f'windspeed_{height}m',
                                  f'winddirection_{height}m'), 1)


class USolar(UWind):
    """methods.py:305-320"""

    inputs = ('wind_speed', 'wind_direction')

    @classmethod
    def compute(cls, data):
        return cls._member(data, cls.inputs, 0)


class VSolar(USolar):
    """methods.py:323-338"""

    @classmethod
    def compute(cls, data):
        return cls._member(data, cls.inputs, 1)


def _to_celsius(data, name):
    """methods.py:349-354: in place in the reference — the source feature
    turns to Celsius with it"""
    out = data[name]
    attrs = data.attrs.setdefault(name, {})
    if attrs.get('units', 'K') == 'K':
        out = data.backend.offset(out, -273.15)
        attrs['units'] = 'C'
        data[name] = out
    return out


class TempNCforCC(DerivedFeature):
    """methods.py:341-354"""

    inputs = ('ta_(.*)',)

    @classmethod
    def compute(cls, data, height):
        return _to_celsius(data, f'ta_{height}m')


class Tas(DerivedFeature):
    """methods.py:357-370"""

    inputs = ('tas',)

    @classmethod
    def compute(cls, data):
        return _to_celsius(data, cls.inputs[0])


class TasMin(Tas):
    inputs = ('tasmin',)


class TasMax(Tas):
    inputs = ('tasmax',)


class Sza(DerivedFeature):
    """methods.py:389-399"""

    @classmethod
    def compute(cls, data):
        raise NotImplementedError(
            'sza needs SolarPosition of the rex package '
            '(rex.utilities.solar_position), which this package does not '
            'carry: pass the zenith angle as a loaded feature')


class Latitude(DerivedFeature):
    """methods.py:402-411"""

    @classmethod
    def compute(cls, data):
        return data.backend.broadcast_pixel(data.lat_lon[..., 0],
                                            len(data.time_index))


class Longitude(DerivedFeature):
    """methods.py:414-423"""

    @classmethod
    def compute(cls, data):
        return data.backend.broadcast_pixel(data.lat_lon[..., 1],
                                            len(data.time_index))


class SpatioTemporalEncoding(DerivedFeature):
    """methods.py:426-469: the (t,) vector on the host with the reference's
    numpy expression, cast to float32, then broadcast"""

    @classmethod
    def _compute(cls, data, k, d, i=0):
        k = 2 * np.pi * (i + 1) * np.asarray(k) / d
        k = np.sin(k) if i % 2 == 0 else np.cos(k)
        s1, s2, _ = data.shape
        return data.backend.broadcast_time(k.astype(np.float32), s1, s2)


class SecondOfDayEncoding(SpatioTemporalEncoding):
    """methods.py:472-484"""

    @classmethod
    def compute(cls, data, i=1):
        ti = data.time_index
        sod = (np.asarray(ti.hour, np.int64) * 3600
               + np.asarray(ti.minute, np.int64) * 60
               + np.asarray(ti.second, np.int64))
        return cls._compute(data, sod, d=_SEC_PER_DAY, i=i)


class SecondOfYearEncoding(SpatioTemporalEncoding):
    """methods.py:487-501"""

    @classmethod
    def compute(cls, data, i=1):
        ti = data.time_index
        soy = ((np.asarray(ti.dayofyear, np.int64) - 1) * 86400
               + np.asarray(ti.hour, np.int64) * 3600
               + np.asarray(ti.minute, np.int64) * 60
               + np.asarray(ti.second, np.int64))
        return cls._compute(data, soy, d=_SEC_PER_YEAR, i=i)


RegistryBase = {
    'u_(.*)': UWind,
    'v_(.*)': VWind,
    'relativehumidity_2m': SurfaceRH,
    'windspeed_(.*)': Windspeed,
    'winddirection_(.*)': Winddirection,
    'cloud_mask': CloudMask,
    'clearsky_ratio': ClearSkyRatio,
    'sza': Sza,
    'latitude_feature': Latitude,
    'longitude_feature': Longitude,
    'soy_encoding': SecondOfYearEncoding,
    'sod_encoding': SecondOfDayEncoding,
}

RegistryH5WindCC = {
    **RegistryBase,
    'temperature_max_(.*)m': 'temperature_(.*)m',
    'temperature_min_(.*)m': 'temperature_(.*)m',
    'relativehumidity_max_(.*)m': 'relativehumidity_(.*)m',
    'relativehumidity_min_(.*)m': 'relativehumidity_(.*)m',
}

RegistryH5SolarCC = {
    **RegistryH5WindCC,
    'windspeed': 'wind_speed',
    'winddirection': 'wind_direction',
    'U': USolar,
    'V': VSolar,
}

RegistryNCforCC = copy.deepcopy(RegistryBase)
RegistryNCforCC.update({
    'u_(.*)': 'ua_(.*)',
    'v_(.*)': 'va_(.*)',
    'relativehumidity_2m': 'hurs',
    'relativehumidity_min_2m': 'hursmin',
    'relativehumidity_max_2m': 'hursmax',
    'clearsky_ratio': ClearSkyRatioCC,
    'temperature_(.*)': TempNCforCC,
    'temperature_2m': Tas,
    'temperature_max_2m': TasMax,
    'temperature_min_2m': TasMin,
    'pressure_(.*)': 'level_(.*)',
})

RegistryNCforCCwithPowerLaw = {
    **RegistryNCforCC,
    'u_(.*)': UWindPowerLaw,
    'v_(.*)': VWindPowerLaw,
}


# ------------------------------------------------------------------ the plan
class InterpGroup:
    """Features that one ``s3_level_interp`` launch serves: the variables of
    one level structure and every requested target level."""

    def __init__(self, key):
        self.key = key                # (source, L, companion levels, is height)
        self.variables = []           # basenames, in request order
        self.targets = []             # levels, in request order
        self.requests = {}            # feature -> (variable, target)
        self.sl_names = {}            # variable -> its single-level planes
        self.results = None           # feature -> plane, once launched

    @property
    def source(self):
        return self.key[0]

    @property
    def companions(self):
        return self.key[2]

    def add(self, feature, variable, target, sl_names):
        if variable not in self.variables:
            self.variables.append(variable)
            self.sl_names[variable] = list(sl_names)
        if target not in self.targets:
            self.targets.append(target)
        self.requests[feature] = (variable, target)

    def __repr__(self):
        return (f'InterpGroup({self.source}, variables={self.variables}, '
                f'targets={self.targets}, companions={self.companions})')


def level_check(stats, sl_levels, levels):
    """The error and the three warnings of Interpolator._check_lev_array
    (interpolation.py:176-237) from a backend's ``level_stats`` of the
    multi-level part (``size``, ``columns``, ``nan``, ``all_nan``, ``bad_min``
    / ``bad_max``: columns without a NaN whose lowest / highest level is
    above ``min(levels)`` / below ``max(levels)``, ``first`` / ``last``: (min,
    max) over the first / last level) and the constants ``sl_levels`` that
    do_level_interpolation appends to every column."""
    sl = [float(v) for v in sl_levels]
    size = stats['size'] + stats['columns'] * len(sl)
    if stats['all_nan'] == stats['columns'] and not sl:
        msg = 'All pressure level height data is NaN!'
        logger.error(msg)
        raise RuntimeError(msg)
    if stats['nan']:
        msg = ('Approximately {:.2f}% of the vertical level '
               'array is NaN. Data will be interpolated or extrapolated '
               'past these NaN values.'.format(100 * stats['nan'] / size))
        logger.warning(msg)
        warn(msg)
    # (a column's lowest level is the lower of its own and the constants')
    bad_min = stats['bad_min'] if not sl or min(levels) < min(sl) else 0
    bad_max = stats['bad_max'] if not sl or max(levels) > max(sl) else 0
    first = stats['first']
    last = (sl[-1], sl[-1]) if sl else stats['last']
    if bad_min:
        msg = ('Approximately {:.2f}% of the lowest vertical levels '
               '(maximum value of {:.3f}, minimum value of {:.3f}) '
               'were greater than the minimum requested level: {}'.format(
                   100 * bad_min / stats['columns'], first[1], first[0],
                   min(levels)))
        logger.warning(msg)
        warn(msg)
    if bad_max:
        msg = ('Approximately {:.2f}% of the highest vertical levels '
               '(minimum value of {:.3f}, maximum value of {:.3f}) '
               'were lower than the maximum requested level: {}'.format(
                   100 * bad_max / stats['columns'], last[0], last[1],
                   max(levels)))
        logger.warning(msg)
        warn(msg)


def vector_level_stats(vec, columns, lo, hi):
    """``level_stats`` of one ``(L,)`` coordinate shared by every column"""
    vec = np.asarray(vec, np.float32)
    nan = np.isnan(vec)
    clean = not nan.any()
    edge = lambda v: (float(v), float(v))            # noqa: E731
    return {'size': columns * len(vec), 'columns': columns,
            'nan': columns * int(nan.sum()),
            'all_nan': columns * int(nan.all()),
            'bad_min': columns * int(clean and lo < vec.min()),
            'bad_max': columns * int(clean and hi > vec.max()),
            'first': edge(vec[0]), 'last': edge(vec[-1])}


# --------------------------------------------------------------- the deriver
class DeviceDeriver:
    """``Deriver`` (derivers/base.py:413-501) over a ``DeriveData``."""

    FEATURE_REGISTRY = RegistryBase

    def __init__(self, data, features, time_roll=0, time_shift=None,
                 hr_spatial_coarsen=1, nan_method_kwargs=None,
                 FeatureRegistry=None, interp_kwargs=None, device=None,
                 backend=None):
        if FeatureRegistry is not None:
            self.FEATURE_REGISTRY = FeatureRegistry
        self.backend = backend or DeviceBackend(device)
        self.data = data.bind(self.backend)
        self.interp_kwargs = interp_kwargs
        self.launch_plan = []
        self._planned_for = {}        # feature -> InterpGroup
        self._dry = None              # names "derived" by the dry pass
        self._cube = None

        if isinstance(features, str) and features != 'all':
            features = [features]
        if features != 'all':
            features = lowered(list(features))
        new_features = ([] if features == 'all' else
                        [f for f in features if f not in self.data])
        # plan: the control flow once without a launch, to learn which
        # features fall to level interpolation, and with which levels
        self._dry = set()
        for f in new_features:
            if f not in self._dry:
                self.derive(f)
                self._dry.add(f)
        self._dry = None
        for f in new_features:
            if f not in self.data:        # (derived on the way, as an input)
                self.data[f] = self.derive(f)
            logger.info('Finished deriving %s.', f)
        self.data.clear_pairs()
        for g in self.launch_plan:
            g.results = {}                # the planes live on in self.data
        self.data = self.data.subset(
            self.data.features if features == 'all' else features)
        self._finish(time_roll, time_shift, hr_spatial_coarsen,
                     nan_method_kwargs)

    # -- membership: what the dry pass has "derived" counts as present
    def _has(self, feature):
        return feature in self.data or (
            self._dry is not None and feature.lower() in self._dry)

    def _known_features(self):
        feats = list(self.data.features)
        return feats + sorted(self._dry or ())

    def _derive_input(self, feature):
        """``self.data[f] = self.derive(f)`` (base.py:134)"""
        out = self.derive(feature)
        if self._dry is not None:
            self._dry.add(feature.lower())
        else:
            self.data[feature] = out

    # -- the registry lookup: what base.py:83-206 does, restated
    def _check_registry(self, feature):
        """the registry's entry for the name: an exact key first, else the
        first key that matches it as a regular expression; None without one"""
        name, registry = feature.lower(), self.FEATURE_REGISTRY
        if name in registry:
            return registry[name]
        return next((entry for key, entry in registry.items()
                     if re.match(key.lower(), name)), None)

    def _get_inputs(self, feature, method=None):
        """the inputs of the feature's method, wildcards filled with the
        feature's own height or pressure"""
        method = method or self._check_registry(feature)
        parsed = parse_feature(feature)
        return [parsed.map_wildcard(name)
                for name in getattr(method, 'inputs', ())]

    def get_inputs(self, feature):
        """the feature's inputs, followed by the inputs of each of those"""
        first = self._get_inputs(feature)
        return first + [name for inp in first
                        for name in self._get_inputs(inp)]

    def no_overlap(self, feature):
        """no input, one or two steps down, is the feature itself"""
        return feature not in self.get_inputs(feature)

    def check_registry(self, feature):
        """An alias (str) for ``derive`` to follow; or the computed feature,
        after deriving the inputs that are missing — if each of them can be
        had without coming back to where it started, or by interpolation; or
        None: no method, or inputs that cannot be had."""
        method = self._check_registry(feature)
        if isinstance(method, str):
            return method
        if not hasattr(method, 'inputs'):
            return None
        logger.debug('Found compute method (%s) for %s.', method, feature)
        inputs = self._get_inputs(feature, method)
        missing = [name for name in inputs if not self._has(name)]
        can_derive = all(self.no_overlap(name)
                         or self.has_interp_variables(name)
                         for name in missing)
        if missing and can_derive:
            logger.debug('Missing required features %s. Trying to derive '
                         'these first.', missing)
            for name in missing:
                self._derive_input(name)
        if all(self._has(name) for name in missing):
            logger.debug('All required features %s found. Proceeding.', inputs)
            if self._dry is not None:
                return True
            out = self._run_compute(feature, method)
            self.data.attrs[feature.lower()] = self.collect_input_attrs(
                feature, inputs)
            return out
        logger.debug('Some of the method inputs reference %s itself. We will '
                     'try height interpolation instead.', feature)
        return None

    def _run_compute(self, feature, method):
        """``method.compute(data, ...)`` with those of ``height``,
        ``pressure`` and ``basename`` that its signature names"""
        parsed = parse_feature(feature)
        wanted = signature(method.compute).parameters
        kwargs = {name: getattr(parsed, name) for name in wanted
                  if hasattr(parsed, name)}
        return self.data._as(method.compute(self.data, **kwargs))

    def map_new_name(self, feature, pattern):
        """the alias with its wildcard replaced by the feature's level"""
        parsed = parse_feature(feature)
        if '*' not in pattern:
            new_feature = pattern
        else:
            suffix = (f'_{parsed.height}m' if parsed.height is not None
                      else f'_{parsed.pressure}pa'
                      if parsed.pressure is not None else None)
            if suffix is None:
                msg = ('Found matching pattern "%s" for feature "%s" but '
                       'could not construct a valid new feature name')
                logger.error(msg, pattern, feature)
                raise RuntimeError(msg % (pattern, feature))
            new_feature = parse_feature(pattern).basename + suffix
        logger.debug('Found alternative name "%s" for "%s". Continuing '
                     'derivation for %s.', feature, new_feature, new_feature)
        return new_feature

    def has_interp_variables(self, feature):
        """two or more features of the basename at a height, or the
        multi-level variable itself"""
        base = parse_feature(feature).basename
        at_heights = sum(
            1 for name in self._known_features()
            if parse_feature(name).basename == base
            and parse_feature(name).height is not None)
        return at_heights > 1 or base in self.data

    def derive(self, feature):
        """base.py:208-251"""
        if not self._has(feature):
            compute_check = self.check_registry(feature)
            if compute_check is not None and isinstance(compute_check, str):
                new_feature = self.map_new_name(feature, compute_check)
                return self.derive(new_feature)
            if compute_check is not None:
                return compute_check
            if self.has_interp_variables(feature):
                logger.debug('Attempting level interpolation for "%s"',
                             feature)
                return self.do_level_interpolation(
                    feature, interp_kwargs=self.interp_kwargs)
            msg = ('Could not find "%s" in contained data or in the '
                   'available compute methods.')
            logger.error(msg, feature)
            raise RuntimeError(msg % feature)
        if self._dry is not None:
            return True
        if self._any_nan(self.data[feature]):
            msg = (f'Feature "{feature}" contains NaN values. Either use '
                   '`nan_method_kwargs` to handle NaN values or clean the '
                   'data.')
            logger.warning(msg)
            warn(msg)
        return self.data[feature]

    def _any_nan(self, x):
        if x.ndim not in (3, 4):
            return bool(np.isnan(self.backend.to_numpy(x)).any())
        flags = self.backend.time_flags(x, 'nan')
        return bool(self.backend.flags_to_numpy(flags).any())

    # -- level interpolation (base.py:253-410)
    def get_single_level_data(self, feature):
        """names and levels of the loaded single-level features of the
        basename (base.py:253-281), in the dataset's order"""
        fstruct = parse_feature(feature)
        pattern = fstruct.basename + '_(.*)'
        names, levs = [], []
        for f in list(self.data.data_vars):
            if re.match(pattern.lower(), f):
                pstruct = parse_feature(f)
                lev = (pstruct.height if pstruct.height is not None
                       else pstruct.pressure)
                names.append(f)
                levs.append(np.float32(lev))
        return names, levs

    def get_multi_level_data(self, feature):
        """the basename's multi-level array and its level source
        (base.py:283-325): ``('column', zg, topography)``, ``('vector',
        height | level)``, or ``(None, None)``"""
        fstruct = parse_feature(feature)
        if fstruct.basename not in self.data:
            return None, None
        var_array = self.data[fstruct.basename]
        if fstruct.height is not None:
            msg = (f'To interpolate {fstruct.basename} to {feature} the '
                   'loaded data needs to include "zg" and "topography" or '
                   'have a "height" dimension.')
            can_calc_height = ('zg' in self.data.features
                               and 'topography' in self.data.features)
            have_height = self.data.height is not None
            assert can_calc_height or have_height, msg
            if can_calc_height:
                return var_array, ('column', self.data['zg'],
                                   self.data['topography'])
            return var_array, ('vector', self.data.height)
        msg = (f'To interpolate {fstruct.basename} to {feature} the loaded '
               'data needs to include "level" (a.k.a pressure at multiple '
               'levels).')
        assert self.data.level is not None, msg
        return var_array, ('vector', self.data.level)

    def _group_key(self, feature):
        ml_var, lev = self.get_multi_level_data(feature)
        _, sl_levs = self.get_single_level_data(feature)
        if ml_var is None and not sl_levs:
            msg = 'Neither single level nor multi level data was found for %s'
            logger.error(msg, feature)
            raise RuntimeError(msg % feature)
        fstruct = parse_feature(feature)
        source = None if lev is None else (
            'zg - topography' if lev[0] == 'column'
            else 'height' if fstruct.height is not None else 'level')
        n_lev = 0 if ml_var is None else int(ml_var.shape[-1])
        return (source, n_lev, tuple(float(v) for v in sl_levs),
                fstruct.height is not None)

    def _plan_interp(self, feature):
        key = self._group_key(feature)
        fstruct = parse_feature(feature)
        level = (fstruct.height if fstruct.height is not None
                 else fstruct.pressure)
        group = next((g for g in self.launch_plan
                      if g.key == key and g.results is None
                      and len(set(g.variables) | {fstruct.basename})
                      <= _lib.LI_MAX_VARS
                      and len(set(g.targets) | {level})
                      <= _lib.LI_MAX_TARGETS), None)
        if group is None:
            group = InterpGroup(key)
            self.launch_plan.append(group)
        group.add(feature.lower(), fstruct.basename, level,
                  self.get_single_level_data(feature)[0])
        self._planned_for[feature.lower()] = group
        return group

    def _launch_group(self, group, interp_kwargs):
        interp_kwargs = interp_kwargs or {}
        method = interp_kwargs.get('method', 'linear')
        var_ml, var_sl, lev, sl_levs = [], [], None, list(group.companions)
        for variable in group.variables:
            probe = next(f for f, (v, _) in group.requests.items()
                         if v == variable)
            ml, lev_v = self.get_multi_level_data(probe)
            if ml is not None:
                var_ml.append(ml)
                lev = lev_v
            var_sl.append([self.data[n] for n in group.sl_names[variable]])
            if any(self._any_nan(arr) for arr in var_sl[-1] + (
                    [ml] if ml is not None else [])):
                msg = ('NaN values found in the interpolation variable '
                       f'array for {probe}.')
                logger.warning(msg)
                warn(msg)
        if lev is not None and lev[0] == 'column':
            if interp_kwargs.get('run_level_check', False):
                tg = [np.float32(v) for v in group.targets]
                level_check(self.backend.level_stats(
                    lev[1], lev[2], min(tg), max(tg)), sl_levs, tg)
            if self._any_nan(lev[1]) or self._any_nan(lev[2]):
                msg = ('NaN values found in the interpolation level array '
                       f'for {sorted(group.requests)}.')
                logger.warning(msg)
                warn(msg)
        elif lev is not None and interp_kwargs.get('run_level_check', False):
            tg = [np.float32(v) for v in group.targets]
            level_check(vector_level_stats(
                lev[1], int(np.prod(self.data.shape)), min(tg), max(tg)),
                sl_levs, tg)
        planes = self.backend.level_interp(
            lev, var_ml, var_sl if sl_levs else [], sl_levs,
            [np.float32(v) for v in group.targets], method)
        group.results = {}
        for feature, (variable, target) in group.requests.items():
            out = planes[group.variables.index(variable)][
                group.targets.index(target)]
            assert not self._any_nan(out), (
                f'NaN values found in the interpolated output for {feature}. '
                'Make sure there are no NaN values in the level or variable '
                'data.')
            group.results[feature] = out

    def collect_input_attrs(self, feature, inputs=None):
        """The attributes of the inputs (default: the loaded features of the
        basename) merged key by key: one value where all agree, else the
        list of them; plus ``inputs`` (what base.py:327-350 collects)."""
        if inputs is None:
            base = parse_feature(feature).basename
            inputs = [name for name in self.data.features
                      if parse_feature(name).basename == base]
        merged = {}
        for name in inputs:
            for key, value in (self.data.attrs.get(name.lower()) or {}).items():
                many = isinstance(value, (list, np.ndarray))
                merged.setdefault(key, []).extend(value if many else [value])
        attrs = {key: values[0] if len({str(v) for v in values}) == 1
                 else values for key, values in merged.items()}
        attrs.setdefault('inputs', inputs)
        return attrs

    def do_level_interpolation(self, feature, interp_kwargs=None):
        """Interpolate over height or pressure (base.py:352-410).  In the
        dry pass the request joins its group; afterwards the group's one
        launch serves every feature in it."""
        if self._dry is not None:
            self._plan_interp(feature)
            return True
        group = self._planned_for.get(feature.lower())
        if group is None or feature.lower() not in (group.results
                                                    or group.requests):
            group = self._plan_interp(feature)
        attrs = self.collect_input_attrs(feature)
        if group.results is None:
            self._launch_group(group, interp_kwargs)
        self.data.attrs[feature.lower()] = attrs
        return group.results[feature.lower()]

    # -- after derivation (base.py:466-501)
    def _finish(self, time_roll, time_shift, hr_spatial_coarsen,
                nan_method_kwargs):
        be = self.backend
        feats = self.features
        flat = [f for f in feats if self.data[f].ndim != 3]
        touched = (time_roll != 0 or hr_spatial_coarsen > 1
                   or nan_method_kwargs is not None)
        if touched and flat:
            raise ValueError(f'{flat} are not (s1, s2, t) features: they '
                             'cannot be rolled, coarsened or masked')
        if touched and feats:
            if time_roll != 0:
                logger.debug('Applying time_roll=%s to data array', time_roll)
            cube = be.stack([self.data[f] for f in feats], int(time_roll))
        if time_shift is not None:
            logger.debug('Applying time_shift=%s to time index', time_shift)
            self.data.time_index = self.data.time_index.shift(
                time_shift, freq='min')
        if not (touched and feats):
            return
        if hr_spatial_coarsen > 1:
            logger.debug('Applying hr_spatial_coarsen=%s to data.',
                         hr_spatial_coarsen)
            s = int(hr_spatial_coarsen)
            cube = be.coarsen(cube, s)
            ll = self.data.lat_lon
            s1, s2 = ll.shape[0] - ll.shape[0] % s, ll.shape[1] - ll.shape[1] % s
            self.data.lat_lon = ll[:s1, :s2].reshape(
                s1 // s, s, s2 // s, s, 2).mean(axis=(1, 3))
        if nan_method_kwargs is not None:
            flags = be.flags_to_numpy(be.time_flags(cube, 'nan'))
            if nan_method_kwargs['method'] == 'mask':
                if nan_method_kwargs.get('dim', 'time') != 'time':
                    raise NotImplementedError(
                        "nan_method_kwargs: only dim='time' is masked")
                keep = np.where(flags == 0)[0]
                cube = be.take_steps(cube, keep)
                self.data.time_index = self.data.time_index[keep]
            elif flags.any():
                raise NotImplementedError(
                    'nan_method_kwargs other than {"method": "mask"} needs '
                    "xarray's interpolate_na, which is out of scope here")
        self._cube = cube
        self.data._arrays = {f: be.channel(cube, i)
                             for i, f in enumerate(feats)}

    # -- results
    @property
    def features(self):
        return list(self.data.features)

    @property
    def lat_lon(self):
        return self.data.lat_lon

    @property
    def time_index(self):
        return self.data.time_index

    @property
    def shape(self):
        return (*self.data.shape, len(self.features))

    def __contains__(self, name):
        return name in self.data

    def __getitem__(self, name):
        return self.data[name]

    def as_array(self, features=None):
        """``(s1, s2, t, C)`` float32 in the order of ``features`` (default:
        all, in the deriver's order)"""
        if features is None and self._cube is not None:
            return self._cube
        feats = self.features if features is None else lowered(list(features))
        flat = [f for f in feats if self.data[f].ndim != 3]
        if flat:
            raise ValueError(f'{flat} are not (s1, s2, t) features: they '
                             'cannot be stacked into the cube; name the '
                             'features to stack')
        return self.backend.stack([self.data[f] for f in feats], 0)


Deriver = DeviceDeriver
