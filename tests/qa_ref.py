"""Restatement of the reference's QA arithmetic for the tests of
``sup3r_amd.qa``: ``spatial_coarsening`` / ``temporal_coarsening``
(sup3r/utilities/utilities.py:345-523) and the eight functions of
sup3r/qa/utilities.py with the same numpy / scipy calls, and ``fixed_order``,
the separately rounded float32 operations that ``s3_qa_recoarsen`` and the
NumpyBackend follow.

``numpy_path`` is the reference's own route for one feature: time-first data
-> ``get_dset_out``'s transpose -> ``spatial_coarsening(obs_axis=False)`` ->
``temporal_coarsening``.  On that (non-contiguous) view numpy adds in the
order ``fixed_order`` states; on a contiguous (H1, H2, HT) array it does not,
and the two agree only within ``(s^2 + t_enhance) 2^-24 max|x|``."""
import numpy as np
from scipy.interpolate import interp1d

METHODS = ('subsample', 'average', 'total', 'max', 'min')


# ------------------------------------------------ the reference's numpy calls
def spatial_coarsening(data, s_enhance=2):
    """obs_axis=False, 2-D / 3-D / 4-D"""
    if s_enhance is None or s_enhance <= 1:
        return data
    if data.shape[0] % s_enhance or data.shape[1] % s_enhance:
        raise ValueError('s_enhance must evenly divide grid size. '
                         f'Received s_enhance: {s_enhance} with data shape: '
                         f'{data.shape}')
    shape = (data.shape[0] // s_enhance, s_enhance,
             data.shape[1] // s_enhance, s_enhance, *data.shape[2:])
    return np.reshape(data, shape).sum(axis=(1, 3)) / s_enhance**2


def temporal_coarsening(data, t_enhance=4, method='subsample'):
    """5-D (obs, s1, s2, t, f)"""
    if t_enhance is None or data.ndim != 5:
        return data
    split = (*data.shape[:3], -1, t_enhance, data.shape[4])
    if method == 'subsample':
        return data[:, :, :, ::t_enhance, :]
    if method == 'average':
        out = np.nansum(np.reshape(data, split), axis=4)
        out /= t_enhance
        return out
    if method == 'total':
        return np.nansum(np.reshape(data, split), axis=4)
    if method == 'max':
        return np.max(np.reshape(data, split), axis=4)
    if method == 'min':
        return np.min(np.reshape(data, split), axis=4)
    raise KeyError(f'Did not recognize temporal_coarsening method "{method}", '
                   'can only accept one of: [subsample, average, total, max, '
                   'min]')


def numpy_path(time_first, s, te, method):
    """(HT, H1, H2) -> (S1, S2, T) as Sup3rQa.get_dset_out + coarsen_data"""
    data = np.asarray(np.transpose(time_first, axes=(1, 2, 0)))
    data = spatial_coarsening(data, s_enhance=s)
    data = np.expand_dims(np.expand_dims(data, axis=0), axis=4)
    data = temporal_coarsening(data, t_enhance=te, method=method)
    return data.squeeze(axis=(0, 4))


def coarsen_contiguous(x, s, te, method):
    """the same calls on a contiguous (H1, H2, HT) array"""
    data = spatial_coarsening(np.ascontiguousarray(x), s_enhance=s)
    data = data[None, ..., None]
    return temporal_coarsening(data, t_enhance=te,
                               method=method).squeeze(axis=(0, 4))


# -------------------------------------------------------------- the fixed order
def fixed_order(x, s, te, method):
    """``x`` (H1, H2, HT) float32, any strides -> (S1, S2, T) float32: per step
    the row sums over j in order, their sum over i in order, a division by
    float32(s^2); then the t_enhance steps in order"""
    with np.errstate(invalid='ignore'):           # inf - inf is a NaN here too
        return _fixed_order(np.asarray(x, np.float32), s, te, method)


def _fixed_order(x, s, te, method):
    h1, h2, ht = x.shape
    assert h1 % s == 0 and h2 % s == 0 and ht % te == 0
    f32 = np.float32
    mean = np.empty((h1 // s, h2 // s, ht), f32)
    for i in range(s):
        row = x[i::s, 0::s, :].astype(f32)
        for j in range(1, s):
            row = (row + x[i::s, j::s, :]).astype(f32)
        mean = row if i == 0 else (mean + row).astype(f32)
    mean = (mean / f32(s * s)).astype(f32)
    steps = [mean[:, :, k::te] for k in range(te)]
    out = steps[0]
    if method == 'subsample':
        return np.ascontiguousarray(out)
    if method in ('max', 'min'):
        for nxt in steps[1:]:
            nan = np.isnan(out) | np.isnan(nxt)
            pick = np.where(nxt > out, nxt, out) if method == 'max' else \
                np.where(nxt < out, nxt, out)
            out = np.where(nan, f32(np.nan), pick).astype(f32)
        return np.ascontiguousarray(out)
    assert method in ('total', 'average'), method
    out = np.where(np.isnan(out), f32(0), out)
    for nxt in steps[1:]:
        out = (out + np.where(np.isnan(nxt), f32(0), nxt)).astype(f32)
    if method == 'average':
        out = (out / f32(te)).astype(f32)
    return np.ascontiguousarray(out)


def same_bits(a, b):
    """equal bits where neither is NaN, NaN in the same places (a NaN's sign
    and payload are not compared)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = np.isnan(a)
    if not np.array_equal(nan, np.isnan(b)):
        return False
    ia, ib = a.view(np.uint32 if a.dtype == np.float32 else np.uint64), \
        b.view(np.uint32 if b.dtype == np.float32 else np.uint64)
    return bool(np.array_equal(ia[~nan], ib[~nan]))


def summary(err):
    """count, sum e, sum |e|, sum e^2, max |e| of the finite errors, float64"""
    e = np.asarray(err)[np.isfinite(err)].astype(np.float64)
    return np.array([e.size, e.sum(), np.abs(e).sum(), (e * e).sum(),
                     np.abs(e).max() if e.size else 0.0])


# ------------------------------------------------------ sup3r/qa/utilities.py
def _fold(E, rng, first):
    x = np.arange(len(E)) if rng is None else \
        np.linspace(rng[0], rng[1], len(E))
    E = x**2 * E
    n = len(x) // 2
    return x[:n], E[first:n + first] + E[-n:][::-1]


def frequency_spectrum(var, f_range=None):
    var_f = np.fft.fftn(var.reshape((-1, var.shape[-1])))
    return _fold(np.mean(np.abs(var_f)**2, axis=0), f_range, 0)


def tke_frequency_spectrum(u, v, f_range=None):
    v_f = np.fft.fftn(v.reshape((-1, v.shape[-1])))
    u_f = np.fft.fftn(u.reshape((-1, u.shape[-1])))
    return _fold(np.mean(np.abs(v_f)**2 + np.abs(u_f)**2, axis=0), f_range, 0)


def wavenumber_spectrum(var, x_range=None, axis=0):
    return _fold(np.mean(np.abs(np.fft.fftn(var))**2, axis=axis), x_range, 1)


def tke_wavenumber_spectrum(u, v, x_range=None, axis=0):
    u_k, v_k = np.fft.fftn(u), np.fft.fftn(v)
    return _fold(np.mean(np.abs(v_k)**2 + np.abs(u_k)**2, axis=axis),
                 x_range, 1)


def continuous_dist(diffs, bins=None, range=None, interpolate=False):
    if bins is None:
        dx = np.abs(np.diff(diffs))
        dx = np.mean(dx[dx > 0])
        bins = int((np.max(diffs) - np.min(diffs)) / dx)
    counts, edges = np.histogram(diffs, bins=bins, range=range)
    centers = edges[:-1] + (np.diff(edges) / 2)
    if interpolate:
        keep = np.where(counts > 0)
        if len(centers[keep]) > 1:
            counts = interp1d(centers[keep], counts[keep], bounds_error=False,
                              fill_value=0)(centers)
    return counts.astype(float) / counts.sum(), centers


def _dist(diffs, bins, range, diff_max, percentile, interpolate):
    diff_max = diff_max or np.percentile(np.abs(diffs), percentile)
    diffs = diffs[(np.abs(diffs) < diff_max)]
    norm = np.sqrt(np.mean(diffs**2))
    counts, centers = continuous_dist(diffs, bins=bins, range=range,
                                      interpolate=interpolate)
    return centers, counts, norm


def transformed(kind, var, scale=1, period=None, t_steps=1):
    """the value the three ``*_dist`` functions count, as they compute it"""
    if kind == 'direct':
        if period is not None:
            diffs = (var + period) % period
            diffs /= scale
            return diffs
        return var / scale
    if kind == 'gradient':
        diffs = np.diff(var, axis=1).flatten()
    else:
        diffs = (var[..., t_steps:] - var[..., :-t_steps]).flatten()
    if period is not None:
        diffs = (diffs + period / 2) % period - period / 2
    diffs /= scale
    return diffs


def direct_dist(var, bins=40, range=None, diff_max=None, scale=1,
                percentile=99.9, interpolate=False, period=None):
    return _dist(transformed('direct', var, scale, period), bins, range,
                 diff_max, percentile, interpolate)


def gradient_dist(var, bins=40, range=None, diff_max=None, scale=1,
                  percentile=99.9, interpolate=False, period=None):
    return _dist(transformed('gradient', var, scale, period), bins, range,
                 diff_max, percentile, interpolate)


def time_derivative_dist(var, bins=40, range=None, diff_max=None, t_steps=1,
                         scale=1, percentile=99.9, interpolate=False,
                         period=None):
    assert t_steps < var.shape[-1]
    return _dist(transformed('time', var, scale, period, t_steps), bins, range,
                 diff_max, percentile, interpolate)
