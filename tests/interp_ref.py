"""numpy-only restatement of the reference's non-neural downscalers, for the
tests of ``LinearInterp`` / ``SurfaceSpatialMetModel`` (the product never
imports it):

* Pillow's resize in mode 'F' (libImaging/Resample.c): ``precompute_coeffs``
  per axis in float64, the horizontal pass accumulated in float64 tap by tap
  and rounded to float32, then the vertical pass; NEAREST is Pillow's affine
  transform (source ``floor((o + 0.5) in / out)``), an unchanged size a copy.
  ``dense=True``: the same passes as float64 products with a dense per-axis
  weight matrix (fast at large sizes; the sum order is BLAS's, so a value may
  move by an ulp);
* ``st_interp`` (sup3r/models/utilities.py:161-212) in index space;
* ``SurfaceSpatialMetModel.generate`` (sup3r/models/surface.py:578-713)
  without noise, following the reference's dtype flow (float64 topography
  terms, float32 images, float32 block means)."""
import math
from fnmatch import fnmatch

import numpy as np

METHODS = ('NEAREST', 'BOX', 'BILINEAR', 'HAMMING', 'BICUBIC', 'LANCZOS')
SUPPORT = {'BOX': 0.5, 'BILINEAR': 1.0, 'HAMMING': 1.0, 'BICUBIC': 2.0,
           'LANCZOS': 3.0}
TEMP_LAPSE, PRES_DIV, PRES_EXP = 6.5 / 1000, 44307.69231, 5.25328
W_DELTA_TEMP, W_DELTA_TOPO = -3.99242830, -0.01736911


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _filter(method):
    f054, f046 = float(np.float32(0.54)), float(np.float32(0.46))

    def box(x):
        return 1.0 if -0.5 < x <= 0.5 else 0.0

    def bilinear(x):
        return max(0.0, 1.0 - abs(x))

    def hamming(x):
        x = abs(x)
        if x == 0.0:
            return 1.0
        if x >= 1.0:
            return 0.0
        x = x * math.pi
        return math.sin(x) / x * (f054 + f046 * math.cos(x))

    def bicubic(x):
        a, x = -0.5, abs(x)
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0

    def lanczos(x):
        return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0
    return {'BOX': box, 'BILINEAR': bilinear, 'HAMMING': hamming,
            'BICUBIC': bicubic, 'LANCZOS': lanczos}[method]


def coeffs(in_size, out_size, method):
    """(lo, cnt, w[out, K]) of one axis"""
    scale = in_size / out_size
    if in_size == out_size or method == 'NEAREST':
        lo = np.floor((np.arange(out_size) + 0.5) * scale).astype(np.int64)
        return lo, np.ones(out_size, np.int64), np.ones((out_size, 1))
    filt = _filter(method)
    fscale = max(scale, 1.0)
    support = SUPPORT[method] * fscale
    K = int(math.ceil(support)) * 2 + 1
    lo, cnt = np.zeros(out_size, np.int64), np.zeros(out_size, np.int64)
    w = np.zeros((out_size, K))
    for o in range(out_size):
        center = (o + 0.5) * scale
        first = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - first
        taps = [filt((k + first - center + 0.5) / fscale) for k in range(n)]
        total = 0.0
        for v in taps:
            total += v
        lo[o], cnt[o] = first, n
        w[o, :n] = [v / total for v in taps] if total != 0.0 else taps
    return lo, cnt, w


def _pass(a, size_out, method, axis, dense):
    a = np.moveaxis(a, axis, -1)
    n_in = a.shape[-1]
    lo, cnt, w = coeffs(n_in, size_out, method)
    if dense:
        m = np.zeros((size_out, n_in))
        for k in range(w.shape[1]):
            ok = k < cnt
            m[np.arange(size_out)[ok], (lo + k)[ok]] = w[ok, k]
        out = a.astype(np.float64) @ m.T
    else:
        out = np.zeros(a.shape[:-1] + (size_out,))
        for k in range(w.shape[1]):
            idx = np.minimum(lo + k, n_in - 1)
            out += a[..., idx].astype(np.float64) * np.where(k < cnt, w[:, k],
                                                             0.0)
    return np.moveaxis(out.astype(np.float32), -1, axis)


def resize(a, s, method='LANCZOS', dense=False):
    """``Image.fromarray(a).resize((w s, h s), method)`` of every trailing
    (h, w) image of ``a``, float32"""
    a = np.asarray(a, dtype=np.float32)
    if s == 1:
        return a.copy()
    h, w = a.shape[-2:]
    tmp = _pass(a, w * s, method, -1, dense)
    return _pass(tmp, h * s, method, -2, dense)


def interp_axis(n, e, centered):
    j = np.arange(n * e, dtype=np.float64)
    p = (j + 0.5) / e - 0.5 if centered else j / e
    i0 = np.clip(np.floor(p), 0, n - 2).astype(np.int64)
    return i0, p - i0


def st_interp(low, s, t, t_centered=False):
    """(s1, s2, t) -> (s1 s, s2 s, t t) float64: linear along each axis,
    the edge intervals extrapolated"""
    a = np.asarray(low, np.float64)
    assert a.ndim == 3 and not any(v <= 1 for v in a.shape)
    for axis, (e, centered) in enumerate(((s, True), (s, True),
                                          (t, t_centered))):
        i0, f = interp_axis(a.shape[axis], e, centered)
        shape = [1, 1, 1]
        shape[axis] = -1
        lo, hi = np.take(a, i0, axis), np.take(a, i0 + 1, axis)
        a = lo + f.reshape(shape) * (hi - lo)
    return a


def linear_generate(low_res, s, t, t_centered=False):
    """LinearInterp.generate: (n, s1, s2, t, f) -> float32"""
    n, s1, s2, tt, c = low_res.shape
    out = np.zeros((n, s1 * s, s2 * s, tt * t, c), np.float32)
    for i in range(n):
        for f in range(c):
            out[i, ..., f] = st_interp(low_res[i, ..., f], s, t, t_centered)
    return out


def coarsen(a, s):
    """s x s block means of the trailing (h, w) images"""
    *lead, h, w = a.shape
    return a.reshape(*lead, h // s, s, w // s, s).sum(axis=(-3, -1)) / s ** 2


def temp_rh_ind(features, idf_rh):
    """the reference's humidity -> temperature pairing (surface.py:212-248)"""
    name = features[idf_rh]
    suffix = name.split('_')[-1]
    for i, t in enumerate(features):
        if not fnmatch(t, 'temperature_*') or not t.endswith(suffix):
            continue
        plain = '_min_' not in name and '_max_' not in name
        if plain or ('_min_' in name and '_min_' in t) or \
                ('_max_' in name and '_max_' in t):
            return i
    raise KeyError(name)


def surface_generate(low_res, topo_lr, topo_hr, features, s,
                     method='LANCZOS', fix_bias=True, dense=True):
    """SurfaceSpatialMetModel.generate without noise: (n, h, w, f) ->
    (n, h s, w s, f) float32"""
    def R(a):
        return resize(a, s, method, dense)

    def fix(lr, hr):
        return hr - R(coarsen(hr, s) - lr) if fix_bias else hr

    def g(z):
        return 101325 * (1 - (1 - z / PRES_DIV) ** PRES_EXP)
    low_res = np.asarray(low_res)
    n, h, w, c = low_res.shape
    hi = np.zeros((n, h * s, w * s, c), np.float32)
    kind = ['T' if fnmatch(f, 'temperature_*') else
            'P' if fnmatch(f, 'pressure_*') else
            'RH' if fnmatch(f, 'relativehumidity_*') else 'O'
            for f in features]
    for i in [i for i, k in enumerate(kind) if k == 'T']:
        x = low_res[..., i]
        hr = R(x.copy() + topo_lr * TEMP_LAPSE)
        hr -= topo_hr * TEMP_LAPSE
        hi[..., i] = fix(x, hr)
    for i in [i for i, k in enumerate(kind) if k == 'P']:
        x = low_res[..., i]
        adj = x.copy() + g(topo_lr)
        if np.min(adj) < 0:
            raise ValueError('negative adjusted low-res pressure')
        hr = R(adj)
        hr -= g(topo_hr)
        hr = fix(x, hr)
        if np.min(hr) < 0:
            raise ValueError('negative high-res pressure')
        hi[..., i] = hr
    for i in [i for i, k in enumerate(kind) if k == 'RH']:
        it = temp_rh_ind(features, i)
        x = low_res[..., i]
        d_temp = hi[..., it] - R(low_res[..., it])
        d_topo = topo_hr - R(topo_lr)
        hr = R(x) + W_DELTA_TEMP * d_temp + W_DELTA_TOPO * d_topo
        hi[..., i] = fix(x, hr)
    for i in [i for i, k in enumerate(kind) if k == 'O']:
        x = low_res[..., i]
        hi[..., i] = fix(x, R(x))
    return hi
