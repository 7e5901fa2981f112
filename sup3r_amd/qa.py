"""QA of a forward pass: ``Sup3rQa`` (sup3r/qa/qa.py:36-514) over arrays in
the place of files, and the distributions and spectra of
sup3r/qa/utilities.py, on the device.

The arithmetic sits behind a backend as in ``derive.py``.  ``DeviceBackend``
runs the kernels of ``csrc/kernels_qa.hip`` through the C ABI; a missing kernel
is an error.  ``NumpyBackend`` states the same operations in numpy so that the
host logic can be tested without a GPU; it is never a fallback.

Arrays in the place of files
    ``source_file_paths``  a ``DeriveData``, or a ``DeviceDeriver`` / anything
                           with ``.data``, ``.features``, ``.time_index``,
                           ``.lat_lon`` and optionally ``.derive``
    ``out_file_path``      an ``.npz`` of ``NpzOutputHandler._write_output``
                           (``data`` of ``(H1, H2, HT, F)`` plus ``features``);
                           a mapping of name to array, time-first ``(HT, H1,
                           H2)`` (the NetCDF order) or flat ``(HT, H1 * H2)``
                           (the h5 order); or an ``(H1, H2, HT, F)`` array /
                           device tensor whose channels ``features`` names
    ``qa_fp``              an ``.npz``: ``<name>_error``, ``<name>_synthetic``,
                           ``<name>_true`` in ``(time, sites)`` order, ``meta``
                           and ``time_index``, written through a temporary file
``bias_correct_method`` names a transform of ``sup3r_amd.bias`` (a callable of
the same signature is taken too).  ``input_handler_name`` and
``input_handler_kwargs`` are kept for the signature: the source is handed in,
not opened.  ``get_node_cmd`` and the CLI are not here.
``error_stats`` is an addition: per feature the count of finite errors, their
bias, MAE, RMSE and largest magnitude, from the same pass as the error.
Step (4) of ``bias_correct_input_handler`` derives ``source_features`` (the
names ``run`` reads from the source; the reference passes ``features``, which
are the same names unless ``source_features`` is given).

Re-coarsening order.  The reference's result depends on numpy's summation
order, which follows the memory layout.  Both backends fix the order of the
reference's own path (time-first data through ``get_dset_out``): per step the
row sums over j, their sum over i, a division by ``float32(s^2)``, then the
``t_enhance`` steps in order.  Data is float32.

Limits and deviations of the distributions on the device
  * ``norm`` is the float32 rounding of ``sqrt(sum d^2 / n)`` from an fp64 sum;
    numpy's own value is a pairwise float32 sum.
  * NaN in the field is a ``ValueError`` naming the count; the reference
    returns NaN from the percentile and then fails inside ``np.histogram``.
  * ``continuous_dist(bins=None)`` raises ``NotImplementedError``: it needs
    the ordered neighbour differences of the compacted array.
  * more than 2^31 - 1 values, or more than 4096 bins, is a ``ValueError``.
  * ``range`` is taken as two Python floats; the field as float32.
Of the spectra: the kept axis is transformed by ``s3_dft_axis`` (a direct DFT
in float32, at most the device's LDS / 264 long: 620 on the MI355X; a longer
axis is a ``ValueError`` naming the limit), the power is summed in fp64 and
returned as float64.
"""
import ctypes as C
import logging
import os
from inspect import signature
from warnings import warn

import numpy as np
from scipy.interpolate import interp1d

from . import _lib
from .derive import DeriveData, DeviceDeriver, lowered

logger = logging.getLogger(__name__)

__all__ = ['Sup3rQa', 'direct_dist', 'gradient_dist', 'time_derivative_dist',
           'continuous_dist', 'frequency_spectrum', 'wavenumber_spectrum',
           'tke_frequency_spectrum', 'tke_wavenumber_spectrum',
           'QaNumpyBackend', 'QaDeviceBackend']


# ----------------------------------------------------------------- host parts
def percentile_plan(n, percentile):
    """the two 0-based ranks and the weight ``np.percentile(method='linear')``
    interpolates with over ``n`` float32 values, in numpy's own operations
    (``percentile`` / the ``linear`` virtual index / ``_get_indexes`` /
    ``_get_gamma``: all float32 when ``percentile`` is a Python number)"""
    q = np.asanyarray(np.true_divide(percentile, np.float32(100)))
    if not (0 <= q <= 1):
        raise ValueError('Percentiles must be in the range [0, 100]')
    vi = np.asanyarray((n - 1) * q)
    prev = np.asanyarray(np.floor(vi))
    nxt = np.asanyarray(prev + 1)
    if vi >= n - 1:
        prev, nxt = np.asanyarray(-1.0), np.asanyarray(-1.0)
    if vi < 0:
        prev, nxt = np.asanyarray(0.0), np.asanyarray(0.0)
    prev, nxt = prev.astype(np.intp), nxt.astype(np.intp)
    gamma = np.asanyarray(np.asanyarray(vi - prev), dtype=vi.dtype)
    return int(prev) % n, int(nxt) % n, gamma


def percentile_lerp(a, b, gamma):
    """numpy's ``_lerp`` of two float32 order statistics"""
    a, b = np.float32(a), np.float32(b)
    diff = np.subtract(b, a)
    out = np.asanyarray(np.add(a, diff * gamma))
    np.subtract(b, diff * (1 - gamma), out=out, where=gamma >= 0.5,
                casting='unsafe', dtype=type(out.dtype))
    return out[()]


def hist_plan(kept_min, kept_max, n_kept, bins, range):
    """what ``np.histogram`` derives before it looks at the values: the edge
    table, the outer edges as its comparisons see them, ``last - first`` as it
    holds it and whether the scaled index is taken in float64"""
    if not isinstance(bins, (int, np.integer)):
        raise TypeError('the device histogram takes a number of uniform bins')
    if range is not None:
        range = (float(range[0]), float(range[1]))
        first, last = range
        if first > last:
            raise ValueError('max must be larger than min in range parameter.')
        if not (np.isfinite(first) and np.isfinite(last)):
            raise ValueError(f'supplied range of [{first}, {last}] is not '
                             'finite')
        probe = np.zeros(0, np.float32)
    elif n_kept == 0:
        first, last = 0, 1
        probe = np.zeros(0, np.float32)
    else:
        first, last = np.float32(kept_min), np.float32(kept_max)
        probe = np.array([first, last], np.float32)
    if first == last:
        first, last = first - 0.5, last + 0.5
    edges = np.histogram(probe, bins=bins, range=range)[1]
    denom = np.subtract(last, first, dtype=np.result_type(last, first))
    wide = (np.zeros(1, np.float32) / denom).dtype == np.float64
    return (np.ascontiguousarray(edges, np.float32), np.float32(first),
            np.float32(last), float(denom), bool(wide))


def _finish_dist(counts, edges, interpolate):
    """utilities.py:378-387 behind ``np.histogram``"""
    centers = edges[:-1] + (np.diff(edges) / 2)
    if interpolate:
        indices = np.where(counts > 0)
        y = counts[indices]
        x = centers[indices]
        if len(x) > 1:
            interp = interp1d(x, y, bounds_error=False, fill_value=0)
            counts = interp(centers)
    counts = counts.astype(float) / counts.sum()
    return counts, centers


def _fold_spectrum(E, rng, wavenumber):
    """the reference's lines behind the mean of ``|fftn|^2``"""
    if rng is None:
        f = np.arange(len(E))
    else:
        f = np.linspace(rng[0], rng[1], len(E))
    n_steps = len(f) // 2
    E = f**2 * E
    E_a = E[1:n_steps + 1] if wavenumber else E[:n_steps]
    E_b = E[-n_steps:][::-1]
    return f[:n_steps], E_a + E_b


class _Xform:
    """how element e of the transformed value d reads the field (see
    include/sup3r_hip.h): ``kind`` direct / gradient / time"""

    def __init__(self, kind, shape, scale=1, period=None, t_steps=1):
        shape = tuple(int(v) for v in shape)
        self.kind, self.shape = kind, shape
        self.scale, self.period, self.t_steps = scale, period, int(t_steps)
        n_in = int(np.prod(shape))
        if kind == 'direct':
            self.diff, self.n = 0, n_in
            self.inner_out = self.inner_in = self.delta = 0
        elif kind == 'gradient':
            inner = int(np.prod(shape[2:]))
            self.diff, self.delta = 1, inner
            self.inner_in, self.inner_out = shape[1] * inner, (shape[1] - 1) * inner
            self.n = shape[0] * self.inner_out
        else:
            self.diff, self.delta = 1, self.t_steps
            self.inner_in, self.inner_out = shape[-1], shape[-1] - self.t_steps
            self.n = (n_in // shape[-1]) * self.inner_out
        self.has_period = int(period is not None)
        p = 0.0 if period is None else period
        self.period32 = float(np.float32(p))
        self.half32 = float(np.float32(p / 2))
        self.scale32 = float(np.float32(scale))

    def args(self):
        return (self.diff, self.n, self.inner_out, self.inner_in, self.delta,
                self.has_period, self.period32, self.half32, self.scale32)

    def numpy(self, var):
        """the reference's lines (utilities.py:214-218, 270-273, 333-336)"""
        if self.kind == 'direct':
            if self.period is not None:
                diffs = (var + self.period) % self.period
                diffs /= self.scale
            else:
                diffs = var / self.scale
            return diffs
        if self.kind == 'gradient':
            diffs = np.diff(var, axis=1).flatten()
        else:
            diffs = (var[..., self.t_steps:]
                     - var[..., :-self.t_steps]).flatten()
        if self.period is not None:
            diffs = (diffs + self.period / 2) % self.period - self.period / 2
        diffs /= self.scale
        return diffs


# ------------------------------------------------------------------- backends
class QaNumpyBackend:
    """The operations of the QA on numpy arrays: the re-coarsening in the
    fixed order, the reference's own lines for the distributions and spectra,
    and the select / bin index of the kernels restated for the CPU tests."""

    name = 'numpy'

    def asarray(self, x):
        return np.ascontiguousarray(np.asarray(x), dtype=np.float32)

    def to_numpy(self, x):
        return np.asarray(x)

    # -- re-coarsening
    @staticmethod
    def _fixed_order(x, s, te, method):
        """``x`` (H1, H2, HT) float32 in any memory order -> (S1, S2, T)"""
        h1, h2, ht = x.shape
        r = x.reshape(h1 // s, s, h2 // s, s, ht)
        tot = None
        for i in range(s):
            rs = r[:, i, :, 0]
            for j in range(1, s):
                rs = rs + r[:, i, :, j]
            tot = rs if tot is None else tot + rs
        sp = (tot / np.float32(s * s)).astype(np.float32)
        sp = sp.reshape(h1 // s, h2 // s, ht // te, te)
        if method == 'subsample':
            return np.ascontiguousarray(sp[..., 0])
        if method in ('max', 'min'):
            fn = np.maximum if method == 'max' else np.minimum
            out = sp[..., 0]
            for k in range(1, te):
                out = fn(out, sp[..., k])
            return np.ascontiguousarray(out)
        z = np.where(np.isnan(sp), np.float32(0), sp)
        out = z[..., 0]
        for k in range(1, te):
            out = out + z[..., k]
        if method == 'average':
            out = out / np.float32(te)
        return np.ascontiguousarray(out, dtype=np.float32)

    def recoarsen(self, hr, layout, channels, methods, s, te, true=None,
                  want_syn=True, want_err=True):
        """``hr`` cube (H1, H2, HT, C) with ``channels``, or time-first (HT,
        H1, H2): per feature ``(synthetic, error, summary)``"""
        out = []
        for f, method in enumerate(methods):
            x = (hr[..., channels[f]] if layout == 'cube'
                 else np.transpose(hr, (1, 2, 0)))
            _check_factors(x.shape, s, te, method)
            syn = self._fixed_order(x.astype(np.float32, copy=False), s, te,
                                    method)
            err = summary = None
            if true is not None and true[f] is not None:
                err = syn - true[f]
                e = err[np.isfinite(err)].astype(np.float64)
                summary = np.array([e.size, e.sum(), np.abs(e).sum(),
                                    (e * e).sum(),
                                    np.abs(e).max() if e.size else 0.0])
            out.append((syn if want_syn else None,
                        err if want_err else None, summary))
        return out

    def planar(self, hr, layout, channel):
        """``get_dset_out``: the (H1, H2, HT) copy of one feature"""
        if layout == 'cube':
            return np.ascontiguousarray(hr[..., channel])
        return np.asarray(np.transpose(hr, axes=(1, 2, 0)))

    # -- the kernels' select and bin index, restated
    @staticmethod
    def select(absd, rank):
        """order statistic ``rank`` of non-negative float32 values by the
        radix select of ``s3_qa_select``: four passes over 8 bits of the bit
        pattern, most significant first"""
        keys = np.ascontiguousarray(absd, np.float32).view(np.uint32).ravel()
        prefix, rank = 0, int(rank)
        for shift in (24, 16, 8, 0):
            hi = 0 if shift == 24 else (0xFFFFFFFF << (shift + 8)) & 0xFFFFFFFF
            live = keys[(keys & np.uint32(hi)) == np.uint32(prefix)]
            hist = np.bincount((live >> np.uint32(shift)) & np.uint32(255),
                               minlength=256)
            cum = np.cumsum(hist)
            b = int(np.searchsorted(cum, rank, side='right'))
            rank -= int(cum[b - 1]) if b else 0
            prefix |= b << shift
        return np.array([prefix], np.uint32).view(np.float32)[0]

    def percentile(self, absd, percentile):
        absd = np.asarray(absd, np.float32).ravel()
        r0, r1, gamma = percentile_plan(absd.size, percentile)
        return percentile_lerp(self.select(absd, r0), self.select(absd, r1),
                               gamma)

    @staticmethod
    def bin_index(d, edges, first, last, denom, wide):
        """the bin of every value of ``d`` inside ``[first, last]`` as
        ``s3_qa_hist`` computes it (``_histogram``'s uniform-bin lines)"""
        d = np.asarray(d, np.float32)
        d = d[(d >= first) & (d <= last)]
        nb = len(edges) - 1
        num = d - first
        if wide:
            f_idx = (num.astype(np.float64) / np.float64(denom)) * nb
        else:
            f_idx = (num / np.float32(denom)) * np.float32(nb)
        idx = f_idx.astype(np.intp)
        idx[idx == nb] -= 1
        idx[d < edges[idx]] -= 1
        idx[(d >= edges[idx + 1]) & (idx != nb - 1)] += 1
        return idx

    def histogram(self, d, bins, range):
        d = np.asarray(d, np.float32).ravel()
        edges, first, last, denom, wide = hist_plan(
            d.min() if d.size else 0, d.max() if d.size else 0, d.size, bins,
            range)
        idx = self.bin_index(d, edges, first, last, denom, wide)
        return np.bincount(idx, minlength=len(edges) - 1), edges

    # -- distributions and spectra: the reference's lines
    def dist(self, var, xf, bins, range, diff_max, percentile, interpolate):
        diffs = xf.numpy(np.asarray(var))
        diff_max = diff_max or np.percentile(np.abs(diffs), percentile)
        diffs = diffs[(np.abs(diffs) < diff_max)]
        norm = np.sqrt(np.mean(diffs**2))
        counts, centers = self.continuous(diffs, bins, range, interpolate)
        return centers, counts, norm

    def continuous(self, diffs, bins, range, interpolate):
        diffs = np.asarray(diffs)
        if bins is None:
            dx = np.abs(np.diff(diffs))
            dx = dx[dx > 0]
            dx = np.mean(dx)
            bins = int((np.max(diffs) - np.min(diffs)) / dx)
            logger.debug(f'Using n_bins={bins} to compute distribution')
        counts, edges = np.histogram(diffs, bins=bins, range=range)
        return _finish_dist(counts, edges, interpolate)

    def power(self, fields, keep_axis):
        """mean over the other axis of ``sum |fftn(field)|^2`` of 2-D fields"""
        E = sum(np.abs(np.fft.fftn(np.asarray(f)))**2 for f in fields)
        return np.mean(E, axis=1 - keep_axis)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class QaDeviceBackend:
    """The same on device tensors through the C ABI (``s3_qa_*``,
    ``s3_dft_axis``).  Nothing is routed to numpy or torch arithmetic."""

    name = 'device'

    def __init__(self, dev=None):
        from .engine import Device
        self.dev = dev or Device.get()

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
        return (C.c_void_p * len(tensors))(
            *[None if t is None else t.data_ptr() for t in tensors])

    # -- re-coarsening
    def recoarsen(self, hr, layout, channels, methods, s, te, true=None,
                  want_syn=True, want_err=True):
        import torch
        hr = self.asarray(hr)
        if layout == 'cube':
            h1, h2, ht, c = (int(v) for v in hr.shape)
        else:
            (ht, h1, h2), c = (int(v) for v in hr.shape), 1
        F = len(methods)
        codes = []
        for m in methods:
            _check_factors((h1, h2, ht), s, te, m)
            codes.append(_lib.TC_METHODS[m])
        shape = (h1 // s, h2 // s, ht // te)
        have_true = true is not None
        true = [self.asarray(t) for t in true] if have_true else None
        syn = [self.dev.empty(shape) for _ in methods] if want_syn else None
        err = ([self.dev.empty(shape) for _ in methods]
               if want_err and have_true else None)
        summary = (torch.empty((F, _lib.QA_SUMMARY_WORDS), dtype=torch.float64,
                               device=hr.device) if have_true else None)
        self.launch_recoarsen(hr, layout, channels, codes, s, te, true, syn,
                              err, summary)
        words = summary.cpu().numpy() if have_true else None
        return [(syn[f] if syn else None, err[f] if err else None,
                 words[f] if have_true else None) for f in range(F)]

    def launch_recoarsen(self, hr, layout, channels, codes, s, te, true, syn,
                         err, summary):
        """the launch alone: device tensors in, nothing allocated, nothing
        read back"""
        if layout == 'cube':
            h1, h2, ht, c = (int(v) for v in hr.shape)
        else:
            (ht, h1, h2), c = (int(v) for v in hr.shape), 1
        F = len(codes)
        ints = C.c_int32 * F
        self._call(
            's3_qa_recoarsen', _ptr(hr),
            _lib.QA_CUBE if layout == 'cube' else _lib.QA_TIME_FIRST, h1, h2,
            ht, c, ints(*[int(v) for v in channels]) if layout == 'cube'
            else None, ints(*codes), F, int(s), int(te),
            self._pointers(true) if true else None,
            self._pointers(syn) if syn else None,
            self._pointers(err) if err else None, _ptr(summary))

    def planar(self, hr, layout, channel):
        hr = self.asarray(hr)
        if layout == 'cube':
            return hr[..., channel].contiguous()
        return hr.permute(1, 2, 0).contiguous()

    # -- distributions
    def _select(self, v, xf, r0, r1):
        import torch
        out = torch.empty(4, dtype=torch.int32, device=v.device)
        self._call('s3_qa_select', _ptr(v), *xf.args(), r0, r1, _ptr(out))
        w = out.cpu().numpy().view(np.uint32)                # 16 bytes
        vals = w[:2].copy().view(np.float32)
        return vals[0], vals[1], int(w[2])

    def _hist(self, v, xf, flags, diff_max, plan=None):
        import torch
        stats = torch.empty(5, dtype=torch.float64, device=v.device)
        counts = edges_d = None
        first = last = np.float32(0)
        denom, wide, nb = 0.0, False, 0
        if plan is not None:
            edges, first, last, denom, wide = plan
            nb = len(edges) - 1
            if nb > _lib.QA_MAX_BINS:
                raise ValueError(f'{nb} bins: the device histogram takes at '
                                 f'most {_lib.QA_MAX_BINS}')
            edges_d = self.asarray(edges)
            counts = torch.empty(nb, dtype=torch.int32, device=v.device)
        self._call('s3_qa_hist', _ptr(v), *xf.args(), flags, float(diff_max),
                   float(first), float(last), float(denom), int(wide), nb,
                   _ptr(edges_d), _ptr(counts), _ptr(stats))
        st = stats.cpu().numpy()
        if st[4]:
            raise ValueError(f'{int(st[4])} NaN values in the field')
        cnt = (None if counts is None else
               counts.cpu().numpy().view(np.uint32).astype(np.intp))
        return st, cnt

    def _counts(self, v, xf, base, diff_max, bins, range):
        """count, sum d^2 and ``np.histogram`` of the kept values: one launch
        with ``range``, two without (the edges follow their min and max)"""
        S, H = _lib.QA_HIST_STATS, _lib.QA_HIST_COUNTS
        if range is not None:
            plan = hist_plan(0, 0, 1, bins, range)
            st, counts = self._hist(v, xf, base | S | H, diff_max, plan)
        else:
            st, _ = self._hist(v, xf, base | S, diff_max)
            plan = hist_plan(st[2], st[3], int(st[0]), bins, None)
            _, counts = self._hist(v, xf, base | H, diff_max, plan)
        return st, counts, plan[0]

    def percentile(self, v, xf, percentile):
        """``np.percentile(np.abs(d), percentile)`` of the transformed value"""
        r0, r1, gamma = percentile_plan(xf.n, percentile)
        a, b, nan = self._select(self.asarray(v), xf, r0, r1)
        if nan:
            raise ValueError(f'{nan} NaN values in the field')
        return percentile_lerp(a, b, gamma)

    def dist(self, var, xf, bins, range, diff_max, percentile, interpolate):
        v = self.asarray(var)
        if xf.n < 1:
            raise ValueError('the field leaves no value to count')
        if xf.n > 2 ** 31 - 1:
            raise ValueError(f'{xf.n} values: the device distributions take '
                             'at most 2^31 - 1')
        if not diff_max:
            diff_max = self.percentile(v, xf, percentile)
        st, counts, edges = self._counts(v, xf, 0, np.float32(diff_max), bins,
                                         range)
        with np.errstate(invalid='ignore', divide='ignore'):
            norm = np.float32(np.sqrt(st[1] / st[0]))
        counts, centers = _finish_dist(counts, edges, interpolate)
        return centers, counts, norm

    def continuous(self, diffs, bins, range, interpolate):
        if bins is None:
            raise NotImplementedError(
                'continuous_dist(bins=None) on the device: it needs the '
                'ordered neighbour differences of the compacted array')
        v = self.asarray(diffs)
        xf = _Xform('direct', tuple(v.shape))
        _, counts, edges = self._counts(v, xf, _lib.QA_HIST_KEEP_ALL, 0.0,
                                        bins, range)
        return _finish_dist(counts, edges, interpolate)

    # -- spectra
    def power(self, fields, keep_axis):
        import torch
        fields = [self.asarray(f) for f in fields]
        a, b = (int(v) for v in fields[0].shape)
        outer, L, inner = (a, b, 1) if keep_axis == 1 else (1, a, b)
        parts = []
        for f in fields:
            re, im = self.dev.empty((a, b)), self.dev.empty((a, b))
            try:
                self._call('s3_dft_axis', _ptr(f), None, _ptr(re), _ptr(im),
                           outer, L, inner, -1)
            except ValueError as e:
                raise ValueError(f'the kept axis of {L} is too long for the '
                                 f'device transform: {e}') from None
            parts += [re, im]
        parts += [None] * (4 - len(parts))
        out = torch.empty(L, dtype=torch.float64, device=fields[0].device)
        self._call('s3_qa_power_sum', *[_ptr(p) for p in parts], outer, L,
                   inner, _ptr(out))
        return out.cpu().numpy()


def _check_factors(shape, s, te, method):
    """the errors of spatial_coarsening / temporal_coarsening"""
    if method not in _lib.TC_METHODS:
        msg = (f'Did not recognize temporal_coarsening method "{method}", '
               'can only accept one of: [subsample, average, total, max, min]')
        logger.error(msg)
        raise KeyError(msg)
    if shape[0] % s != 0 or shape[1] % s != 0:
        msg = ('s_enhance must evenly divide grid size. '
               f'Received s_enhance: {s} with data shape: {tuple(shape)}')
        logger.error(msg)
        raise ValueError(msg)
    if shape[2] % te != 0:
        raise ValueError(f't_enhance must evenly divide the time axis. '
                         f'Received t_enhance: {te} with data shape: '
                         f'{tuple(shape)}')


def _backend(backend):
    return backend if backend is not None else QaDeviceBackend()


def _is_2d_ok(var, what):
    if var.ndim not in (2, 3):
        raise ValueError(f'{what} takes an (s1, s2, t) or 2-D field, got '
                         f'shape {tuple(var.shape)}')


# ------------------------------------------------- utilities.py's functions
def direct_dist(var, bins=40, range=None, diff_max=None, scale=1,
                percentile=99.9, interpolate=False, period=None, *,
                backend=None):
    """utilities.py:170-224: ``(centers, counts, norm)`` of ``var / scale``"""
    xf = _Xform('direct', var.shape, scale, period)
    return _backend(backend).dist(var, xf, bins, range, diff_max, percentile,
                                  interpolate)


def gradient_dist(var, bins=40, range=None, diff_max=None, scale=1,
                  percentile=99.9, interpolate=False, period=None, *,
                  backend=None):
    """utilities.py:227-279: the same of ``np.diff(var, axis=1)``"""
    _is_2d_ok(var, 'gradient_dist')
    xf = _Xform('gradient', var.shape, scale, period)
    return _backend(backend).dist(var, xf, bins, range, diff_max, percentile,
                                  interpolate)


def time_derivative_dist(var, bins=40, range=None, diff_max=None, t_steps=1,
                         scale=1, percentile=99.9, interpolate=False,
                         period=None, *, backend=None):
    """utilities.py:282-342: the same of ``var[..., k:] - var[..., :-k]``"""
    msg = (f'Received t_steps={t_steps} for time derivative calculation but '
           f'data only has {var.shape[-1]} time steps')
    assert t_steps < var.shape[-1], msg
    xf = _Xform('time', var.shape, scale, period, t_steps)
    return _backend(backend).dist(var, xf, bins, range, diff_max, percentile,
                                  interpolate)


def continuous_dist(diffs, bins=None, range=None, interpolate=False, *,
                    backend=None):
    """utilities.py:345-387: ``(counts, centers)`` of ``np.histogram``"""
    return _backend(backend).continuous(diffs, bins, range, interpolate)


def _rows(var):
    return var.reshape((-1, var.shape[-1]))


def frequency_spectrum(var, f_range=None, *, backend=None):
    """utilities.py:50-84"""
    E = _backend(backend).power([_rows(var)], 1)
    return _fold_spectrum(E, f_range, False)


def tke_frequency_spectrum(u, v, f_range=None, *, backend=None):
    """utilities.py:10-47"""
    E = _backend(backend).power([_rows(v), _rows(u)], 1)
    return _fold_spectrum(E, f_range, False)


def _wavenumber(fields, x_range, axis, backend):
    if any(f.ndim != 2 for f in fields) or axis not in (0, 1):
        raise ValueError('the wavenumber spectra take (lat, lon) fields and '
                         'axis 0 or 1')
    E = _backend(backend).power(fields, 1 - axis)
    return _fold_spectrum(E, x_range, True)


def wavenumber_spectrum(var, x_range=None, axis=0, *, backend=None):
    """utilities.py:131-167"""
    return _wavenumber([var], x_range, axis, backend)


def tke_wavenumber_spectrum(u, v, x_range=None, axis=0, *, backend=None):
    """utilities.py:87-128"""
    return _wavenumber([v, u], x_range, axis, backend)


# --------------------------------------------------------------------- Sup3rQa
class _Source:
    """a ``DeriveData`` as an input handler without ``derive``"""

    def __init__(self, data, backend):
        self.data = data.bind(backend)
        self.backend = backend

    features = property(lambda self: self.data.features)
    time_index = property(lambda self: self.data.time_index)
    lat_lon = property(lambda self: self.data.lat_lon)
    shape = property(lambda self: self.data.shape)

    def __contains__(self, name):
        return name in self.data

    def __getitem__(self, name):
        return self.data[name]


def _all_in(features, handler):
    return all(f in handler for f in features)


class Sup3rQa:
    """Class for doing QA on sup3r forward pass outputs (qa.py:36-514).

    Note
    ----
    This only works if the sup3r forward pass output can be reshaped into a 2D
    raster dataset (e.g. no sparsifying of the meta data).
    """

    IGNORE = ('meta', 'time_index', 'gids')

    def __init__(self, source_file_paths, out_file_path, s_enhance, t_enhance,
                 temporal_coarsening_method, features=None,
                 source_features=None, output_names=None,
                 input_handler_name=None, input_handler_kwargs=None,
                 qa_fp=None, bias_correct_method=None,
                 bias_correct_kwargs=None, save_sources=True, *,
                 backend=None):
        logger.info('Initializing Sup3rQa and retrieving source data...')
        self.backend = _backend(backend)
        self.s_enhance = s_enhance
        self.t_enhance = t_enhance
        self._t_meth = temporal_coarsening_method
        self._out_fp = out_file_path
        self._features = (
            features if isinstance(features, (list, tuple)) else [features])
        self._source_features = (
            source_features if isinstance(source_features, (list, tuple))
            else [source_features])
        self._out_names = (
            output_names if isinstance(output_names, (list, tuple))
            else [output_names])
        self.qa_fp = qa_fp
        if qa_fp is not None and not str(qa_fp).endswith('.npz'):
            raise TypeError(f'qa_fp must end in .npz: {qa_fp}')
        self.save_sources = save_sources
        self.error_stats = {}
        self.output_handler = self._open_output(out_file_path)

        self.bias_correct_method = bias_correct_method
        self.bias_correct_kwargs = (
            {} if bias_correct_kwargs is None
            else {k.lower(): v for k, v in bias_correct_kwargs.items()})
        self.input_handler_name = input_handler_name
        self.input_handler_kwargs = input_handler_kwargs or {}

        handler = source_file_paths
        if isinstance(handler, DeriveData):
            handler = _Source(handler, self.backend)
        self.input_handler = self.bias_correct_input_handler(handler)
        ll = np.asarray(self.input_handler.lat_lon)
        self.meta = ll.reshape(-1, ll.shape[-1])
        self.time_index = self.input_handler.time_index

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc_value, traceback):
        self.close()
        if exc_type is not None:
            raise

    def close(self):
        """Drop the opened output"""
        self.output_handler = None

    # -- the output in the place of the file
    def _open_output(self, out):
        """-> dict(kind='cube', data, names) or dict(kind='nc' | 'h5', sets)"""
        if isinstance(out, (str, os.PathLike)):
            if not str(out).endswith('.npz'):
                msg = 'Did not recognize output file type: {}'.format(out)
                logger.error(msg)
                raise TypeError(msg)
            with np.load(out) as z:
                return {'kind': 'cube', 'data': z['data'],
                        'names': [str(f) for f in z['features']]}
        if hasattr(out, 'keys'):
            sets = {k: out[k] for k in out.keys()}
            dims = {np.ndim(v) for k, v in sets.items()
                    if k.lower() not in self.IGNORE}
            if dims not in ({3}, {2}):
                raise TypeError('the datasets of a mapping are all time-first '
                                '(HT, H1, H2) or all flat (HT, H1 * H2)')
            return {'kind': 'nc' if dims == {3} else 'h5', 'sets': sets}
        if getattr(out, 'ndim', 0) == 4:
            names = self._features
            if names == [None] or len(names) != out.shape[-1]:
                raise ValueError('an (H1, H2, HT, F) output needs `features` '
                                 'to name its F channels')
            return {'kind': 'cube', 'data': out, 'names': list(names)}
        msg = 'Did not recognize output file type: {}'.format(type(out))
        logger.error(msg)
        raise TypeError(msg)

    @property
    def features(self):
        """Feature names of the output, excluding meta and time index"""
        if self._features is None or self._features == [None]:
            oh = self.output_handler
            features = oh['names'] if oh['kind'] == 'cube' else list(oh['sets'])
            features = [f for f in features if f.lower() not in self.IGNORE]
        elif isinstance(self._features, (list, tuple)):
            features = self._features
        return features

    @property
    def output_names(self):
        """Output dataset names corresponding to the features list"""
        if self._out_names is None or self._out_names == [None]:
            return self.features
        return self._out_names

    @property
    def source_features(self):
        """Source dataset names corresponding to the input source data"""
        if self._source_features is None or self._source_features == [None]:
            return self.features
        return self._source_features

    @property
    def output_type(self):
        """'nc' (time-first datasets), 'h5' (flat datasets) or 'npz' (the
        ``(H1, H2, HT, F)`` cube)"""
        kind = self.output_handler['kind']
        return 'npz' if kind == 'cube' else kind

    # -- the source
    def _bias_correct_feature(self, feature, handler):
        """bias/utilities.py:221-293 with the transforms of sup3r_amd.bias"""
        from . import bias
        data = handler[feature]
        method = self.bias_correct_method
        if method is None:
            return data
        if not callable(method):
            method = getattr(bias, method)
        logger.info(f'Running bias correction with: {method}.')
        feature_kwargs = self.bias_correct_kwargs[feature]
        params = signature(method).parameters
        if 'date_range_kwargs' in params:
            # (make_time_index takes the index itself in the place of kwargs)
            feature_kwargs['date_range_kwargs'] = handler.time_index
        if 'lr_padded_slice' in params and \
                'lr_padded_slice' not in feature_kwargs:
            feature_kwargs['lr_padded_slice'] = None
        if 'temporal_avg' in params and 'temporal_avg' not in feature_kwargs:
            msg = ('The kwarg "temporal_avg" was not provided in the bias '
                   'correction kwargs but is present in the bias '
                   'correction function "{}". If this is not set '
                   'appropriately, especially for monthly bias '
                   'correction, it could result in QA results that look '
                   'worse than they actually are.'.format(method))
            logger.warning(msg)
            warn(msg)
        return method(data, handler.lat_lon, **feature_kwargs)

    def bias_correct_input_handler(self, input_handler):
        """Apply bias correction to all source features which have bias
        correction data and return a deriver to use for derivations of
        features to match output features.

        (1) Check if we need to derive any features included in the
        bias_correct_kwargs.
        (2) Derive these features using the input_handler.derive method, and
        update the stored data.
        (3) Apply bias correction to all the features in the
        bias_correct_kwargs
        (4) Derive the features required for validation from the bias corrected
        data and update the stored data
        (5) Return the updated input_handler, now a deriver.
        """
        need_derive = list(
            set(lowered(self.bias_correct_kwargs))
            - set(input_handler.features))
        msg = (
            f'Features {need_derive} need to be derived prior to bias '
            'correction, but the input_handler has no derive method. '
            'Request an appropriate input_handler with '
            'input_handler_name=DataHandlerName.')
        assert len(need_derive) == 0 or hasattr(input_handler, 'derive'), msg
        for f in need_derive:
            input_handler.data[f] = input_handler.derive(f)
        bc_feats = list(
            set(input_handler.features).intersection(
                set(lowered(self.bias_correct_kwargs.keys()))))
        for f in bc_feats:
            input_handler.data[f] = self._bias_correct_feature(
                f, input_handler)
        want = lowered(list(self.source_features))
        if _all_in(want, input_handler):
            return input_handler
        return DeviceDeriver(
            input_handler.data, features=want,
            FeatureRegistry=getattr(input_handler, 'FEATURE_REGISTRY', None),
            backend=_derive_backend(self.backend))

    # -- the high-resolution output
    def _hr(self, name):
        """-> (array, layout, channel) of output feature ``name``"""
        oh = self.output_handler
        if oh['kind'] == 'cube':
            low = [n.lower() for n in oh['names']]
            if name.lower() not in low:
                raise KeyError(name)
            if not oh.get('bound'):
                oh['data'], oh['bound'] = self.backend.asarray(oh['data']), True
            return oh['data'], 'cube', low.index(name.lower())
        data = oh['sets'][name]
        if oh['kind'] == 'h5':
            shape = (len(self.input_handler.time_index) * self.t_enhance,
                     int(self.input_handler.shape[0] * self.s_enhance),
                     int(self.input_handler.shape[1] * self.s_enhance))
            data = data.reshape(shape)
        return data, 'tfirst', 0

    def get_dset_out(self, name):
        """A copy of the high-resolution output ``name`` of shape
        (spatial_1, spatial_2, temporal)"""
        logger.debug('Getting sup3r output dataset "{}"'.format(name))
        data, layout, ch = self._hr(name)
        return self.backend.planar(self.backend.asarray(data), layout, ch)

    def _method(self, idf):
        return self._t_meth if isinstance(self._t_meth, str) \
            else self._t_meth[idf]

    def coarsen_data(self, idf, feature, data):
        """Re-coarsen a high-resolution synthetic output dataset of shape
        (spatial_1, spatial_2, temporal); the result has that layout too"""
        t_meth = self._method(idf)
        logger.info(
            f'Coarsening feature "{feature}" with {self.s_enhance}x '
            f'spatial averaging and "{t_meth}" {self.t_enhance}x '
            'temporal averaging')
        data = self.backend.asarray(data)
        cube = data.reshape(*data.shape, 1)
        return self.backend.recoarsen(cube, 'cube', [0], [t_meth],
                                      self.s_enhance, self.t_enhance,
                                      want_err=False)[0][0]

    # -- the QA file
    def _dset(self, data):
        """(space1, space2, time) -> the (time, sites) order of the h5 file"""
        shape = (len(self.input_handler.time_index), len(self.meta))
        data = np.asarray(self.backend.to_numpy(data))
        return np.transpose(data, axes=(2, 0, 1)).reshape(shape)

    def _write(self, qa_fp, sets):
        old = {}
        if os.path.exists(qa_fp):
            with np.load(qa_fp) as z:
                old = {k: z[k] for k in z.files}
        else:
            logger.info('Initializing qa output file: "{}"'.format(qa_fp))
            old = {'meta': self.meta, 'time_index': np.asarray(
                self.input_handler.time_index).astype('int64')}
        old.update(sets)
        tmp = str(qa_fp) + '.tmp.npz'
        np.savez(tmp, **old)
        os.replace(tmp, qa_fp)

    def export(self, qa_fp, data, dset_name, dset_suffix=''):
        """Add ``data`` (space1, space2, time) to the QA file as
        ``dset_name[_dset_suffix]`` in float32 (time, sites) order"""
        if dset_suffix:
            dset_name = dset_name + '_' + dset_suffix
        logger.info('Adding dataset "{}" to output file.'.format(dset_name))
        self._write(qa_fp, {dset_name: self._dset(data).astype(np.float32)})

    def run(self):
        """Go through all datasets and get the error for the re-coarsened
        synthetic minus the true low-res source data.

        Returns
        -------
        errors : dict
            feature -> (space1, space2, time) array of the re-coarsened
            synthetic data minus the source true low-res data
        """
        errors, sets = {}, {}
        feats = list(self.features)
        ziter = list(zip(feats, self.source_features, self.output_names))
        jobs = []                            # (idf, hr, layout, channel, true)
        for idf, (feature, source_feature, _) in enumerate(ziter):
            logger.info(
                'Running QA on dataset {} of {} for feature "{}" '
                'with source feature name "{}"'.format(
                    idf + 1, len(feats), feature, source_feature))
            hr, layout, ch = self._hr(feature)
            data_true = self.input_handler[source_feature]
            hs = tuple(hr.shape[:3]) if layout == 'cube' else (
                hr.shape[1], hr.shape[2], hr.shape[0])
            _check_factors(hs, self.s_enhance, self.t_enhance,
                           self._method(idf))
            syn_shape = (hs[0] // self.s_enhance, hs[1] // self.s_enhance,
                         hs[2] // self.t_enhance)
            if syn_shape != tuple(data_true.shape):
                msg = (
                    'Sup3rQa failed while trying to inspect the "{}" feature. '
                    'The source low-res data had shape {} while the '
                    're-coarsened synthetic data had shape {}.'.format(
                        feature, tuple(data_true.shape), syn_shape))
                logger.error(msg)
                raise RuntimeError(msg)
            jobs.append((idf, hr, layout, ch, data_true))
        # one launch per QA_MAX_FEATURES features of the cube, one per
        # time-first field
        groups, cube_jobs = [], [j for j in jobs if j[2] == 'cube']
        for i in range(0, len(cube_jobs), _lib.QA_MAX_FEATURES):
            groups.append(cube_jobs[i:i + _lib.QA_MAX_FEATURES])
        groups += [[j] for j in jobs if j[2] != 'cube']
        want_syn = self.qa_fp is not None and self.save_sources
        results = {}
        for group in groups:
            out = self.backend.recoarsen(
                group[0][1], group[0][2], [j[3] for j in group],
                [self._method(j[0]) for j in group], self.s_enhance,
                self.t_enhance, true=[j[4] for j in group], want_syn=want_syn)
            for j, res in zip(group, out):
                results[j[0]] = (res, j[4])
        for idf, (feature, _, dset_out) in enumerate(ziter):
            (syn, err, words), data_true = results[idf]
            errors[feature] = err
            n = float(words[0])
            with np.errstate(invalid='ignore', divide='ignore'):
                self.error_stats[feature] = {
                    'count': int(n), 'bias': float(words[1] / n),
                    'mae': float(words[2] / n),
                    'rmse': float(np.sqrt(words[3] / n)),
                    'max_abs': float(words[4])}
            if self.qa_fp is not None:
                sets[dset_out + '_error'] = self._dset(err)
                if self.save_sources:
                    sets[dset_out + '_synthetic'] = self._dset(syn)
                    sets[dset_out + '_true'] = self._dset(data_true)
        if self.qa_fp is not None:
            self._write(self.qa_fp, {k: v.astype(np.float32)
                                     for k, v in sets.items()})
        logger.info('Finished Sup3rQa run method.')
        return errors


def _derive_backend(backend):
    """the ``derive.py`` backend that goes with a QA backend"""
    from . import derive
    if backend.name == 'numpy':
        return derive.NumpyBackend()
    return derive.DeviceBackend(backend.dev)
