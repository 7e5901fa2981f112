"""numpy restatement of the reference's bias-correction transforms, for the
tests of ``sup3r_amd.bias`` (the product never imports it).

* Linear family — ``global_linear_bc``, ``local_linear_bc``,
  ``monthly_local_linear_bc`` follow sup3r/bias/bias_transforms.py:224-487
  line by line (the factor file is a mapping here: ``{feature}_scalar`` /
  ``{feature}_adder`` already cut to the domain).
* ``local_qdm_bc`` / ``local_presrat_bc`` / ``_apply_qdm`` follow :490-824 and
  :958-1137 line by line, with one deliberate difference: ``k_factor`` and
  ``tau_fut`` are cut by ``lr_padded_slice`` like the three distributions (the
  reference leaves them domain-sized, which only broadcasts when no slice is
  given).
* The quantile mapping itself (``rex.utilities.bc_utils.
  QuantileDeltaMapping``) is NOT in the reference tree and ``rex`` is not
  available here: ``quantile_delta_mapping`` below is restated from
  ``numpy.interp`` both ways and Cannon et al. 2015, eqs. 3-6, which the
  reference's docstrings cite — **unverified against rex**.  With ``delta_
  denom_zero`` and ``delta_denom_min`` both given, zeros are replaced first
  and the floor applied second: a decision of this restatement, kept in
  ``relative_denominator`` alone.
* ``pad_after`` is the order of the reference's forward pass: correct the
  un-padded window, then reflect-pad it (forward_pass.py:66-72,122-186).

Every function takes ``dtype``: float64 is the reference's arithmetic on
float64 input (``R64``), float32 evaluates every input and intermediate in
float32 (``R32``) — ``interp`` is written out for that, since ``numpy.interp``
always computes in float64; in float64 it equals ``numpy.interp``."""
from warnings import warn

import numpy as np
from scipy.ndimage import gaussian_filter


def make_time_index(date_range_kwargs):
    """make_time_index_from_kws (sup3r/preprocessing/utilities.py:222-244)"""
    import pandas as pd
    if isinstance(date_range_kwargs, pd.DatetimeIndex):
        return date_range_kwargs
    kws = dict(date_range_kwargs)
    drop_leap = kws.pop('drop_leap', False)
    time_index = pd.date_range(**kws)
    if drop_leap:
        leap_mask = (time_index.month == 2) & (time_index.day == 29)
        time_index = time_index[~leap_mask]
    return time_index


def _out_range(out, out_range):
    if out_range is not None:
        out = np.maximum(out, out.dtype.type(np.min(out_range)))
        out = np.minimum(out, out.dtype.type(np.max(out_range)))
    return out


def global_linear_bc(data, scalar, adder, out_range=None, dtype=np.float32):
    """bias_transforms.py:224-248"""
    dt = np.dtype(dtype).type
    out = np.asarray(data, dtype) * dt(scalar) + dt(adder)
    return _out_range(out, out_range)


def local_linear_bc(data, feature_name, bias_fp, lr_padded_slice=None,
                    out_range=None, smoothing=0, dtype=np.float32):
    """bias_transforms.py:251-348"""
    data = np.asarray(data, dtype)
    scalar = np.asarray(bias_fp[f'{feature_name}_scalar'], dtype)
    adder = np.asarray(bias_fp[f'{feature_name}_adder'], dtype)
    if len(scalar.shape) == 3 and len(adder.shape) == 3:
        scalar = scalar.mean(axis=-1)
        adder = adder.mean(axis=-1)
    if lr_padded_slice is not None:
        spatial_slice = (lr_padded_slice[0], lr_padded_slice[1])
        scalar = scalar[spatial_slice]
        adder = adder[spatial_slice]
    if np.isnan(scalar).any() or np.isnan(adder).any():
        warn('Bias correction scalar/adder values had NaNs for '
             f'"{feature_name}" from: <memory>')
    scalar = np.repeat(np.expand_dims(scalar, axis=-1), data.shape[-1],
                       axis=-1)
    adder = np.repeat(np.expand_dims(adder, axis=-1), data.shape[-1], axis=-1)
    if smoothing > 0:
        for idt in range(scalar.shape[-1]):
            scalar[..., idt] = gaussian_filter(scalar[..., idt], smoothing,
                                               mode='nearest')
            adder[..., idt] = gaussian_filter(adder[..., idt], smoothing,
                                              mode='nearest')
    out = data * scalar + adder
    return _out_range(out, out_range)


def monthly_local_linear_bc(data, feature_name, bias_fp, date_range_kwargs,
                            lr_padded_slice=None, temporal_avg=True,
                            out_range=None, smoothing=0, scalar_range=None,
                            adder_range=None, dtype=np.float32):
    """bias_transforms.py:351-487"""
    dt = np.dtype(dtype).type
    data = np.asarray(data, dtype)
    time_index = make_time_index(date_range_kwargs)
    scalar = np.asarray(bias_fp[f'{feature_name}_scalar'], dtype)
    adder = np.asarray(bias_fp[f'{feature_name}_adder'], dtype)
    assert len(scalar.shape) == 3, 'Monthly bias correct needs 3D scalars'
    assert len(adder.shape) == 3, 'Monthly bias correct needs 3D adders'
    if lr_padded_slice is not None:
        spatial_slice = (lr_padded_slice[0], lr_padded_slice[1])
        scalar = scalar[spatial_slice]
        adder = adder[spatial_slice]
    imonths = time_index.month.values - 1
    scalar = scalar[..., imonths]
    adder = adder[..., imonths]
    if temporal_avg:
        scalar = scalar.mean(axis=-1)
        adder = adder.mean(axis=-1)
        scalar = np.repeat(np.expand_dims(scalar, axis=-1), data.shape[-1],
                           axis=-1)
        adder = np.repeat(np.expand_dims(adder, axis=-1), data.shape[-1],
                          axis=-1)
        if len(time_index.month.unique()) > 2:
            warn('Bias correction method "monthly_local_linear_bc" was used '
                 'with temporal averaging over a time index with >2 months.')
    if np.isnan(scalar).any() or np.isnan(adder).any():
        warn('Bias correction scalar/adder values had NaNs for '
             f'"{feature_name}" from: <memory>')
    if smoothing > 0:
        for idt in range(scalar.shape[-1]):
            scalar[..., idt] = gaussian_filter(scalar[..., idt], smoothing,
                                               mode='nearest')
            adder[..., idt] = gaussian_filter(adder[..., idt], smoothing,
                                              mode='nearest')
    if scalar_range is not None:
        scalar = np.minimum(scalar, dt(np.max(scalar_range)))
        scalar = np.maximum(scalar, dt(np.min(scalar_range)))
    if adder_range is not None:
        adder = np.minimum(adder, dt(np.max(adder_range)))
        adder = np.maximum(adder, dt(np.min(adder_range)))
    out = data * scalar + adder
    return _out_range(out, out_range)


# ------------------------------------------------------------------ QDM
def interp(x, xp, fp):
    """``numpy.interp(x[s], xp[s], fp[s])`` for every site ``s`` in the dtype
    of its arguments: ``x`` (sites, n), ``xp`` / ``fp`` (sites, Q).  Clamped
    at both ends; the segment is the last ``j`` with ``xp[j] <= x`` (what
    numpy's binary search finds, repeated knots included); ``slope * (x -
    xp[j]) + fp[j]`` as in numpy's ``arr_interp``."""
    Q = xp.shape[-1]
    j = np.zeros(x.shape, dtype=np.int64)
    for k in range(1, Q):                 # j = #(xp <= x) - 1, clipped
        j += (xp[:, k:k + 1] <= x)
    j = np.minimum(j, Q - 2)
    x0 = np.take_along_axis(xp, j, axis=1)
    x1 = np.take_along_axis(xp, j + 1, axis=1)
    f0 = np.take_along_axis(fp, j, axis=1)
    f1 = np.take_along_axis(fp, j + 1, axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        slope = (f1 - f0) / (x1 - x0)
        out = slope * (x - x0) + f0
    out = np.where(x < xp[:, :1], fp[:, :1], out)
    out = np.where(x >= xp[:, -1:], fp[:, -1:], out)
    return np.where(np.isnan(x), x, out).astype(x.dtype)


def relative_denominator(x_mh, delta_denom_min, delta_denom_zero):
    """the denominator of the relative delta (Cannon et al. 2015, eq. 4):
    zeros replaced by ``delta_denom_zero`` FIRST, then floored by
    ``delta_denom_min`` (this restatement's choice of precedence)"""
    dt = x_mh.dtype.type
    if delta_denom_zero is not None:
        x_mh = np.where(x_mh == 0, dt(delta_denom_zero), x_mh)
    if delta_denom_min is not None:
        x_mh = np.maximum(x_mh, dt(delta_denom_min))
    return x_mh


def quantile_delta_mapping(arr, params_oh, params_mh, params_mf=None,
                           relative=True, delta_denom_min=None,
                           delta_denom_zero=None, delta_range=None):
    """empirical QDM with linear sampling, **unverified against rex**:
    ``arr`` (time, space), params (space, Q) quantile values at the levels
    ``q_k = k / (Q - 1)``.  ``q = F_mf(x)``; ``x_oh = F_oh^-1(q)``; ``x_mh =
    F_mh^-1(q)``; relative: ``x_oh * (x / x_mh)``, absolute: ``x_oh + (x -
    x_mh)``; ``params_mf=None`` (no trend): ``mf := mh``."""
    dtype = arr.dtype
    dt = dtype.type
    if params_mf is None:
        params_mf = params_mh
    Q = params_oh.shape[-1]
    levels = (np.arange(Q, dtype=dtype) / dt(Q - 1))[None, :]
    levels = np.broadcast_to(levels, params_oh.shape)
    x = arr.T                                         # (space, time)
    q = interp(x, params_mf, levels)
    x_oh = interp(q, levels, params_oh)
    x_mh = interp(q, levels, params_mh)
    with np.errstate(divide='ignore', invalid='ignore'):
        if relative:
            x_mh = relative_denominator(x_mh, delta_denom_min,
                                        delta_denom_zero)
            delta = x / x_mh
        else:
            delta = x - x_mh
        if delta_range is not None:
            delta = np.maximum(delta, dt(np.min(delta_range)))
            delta = np.minimum(delta, dt(np.max(delta_range)))
        out = x_oh * delta if relative else x_oh + delta
    return out.T.astype(dtype)


def _apply_qdm(subset, base_params, bias_params, bias_fut_params,
               relative=True, no_trend=False, delta_denom_min=None,
               delta_denom_zero=None, delta_range=None):
    """bias_transforms.py:490-619"""
    bias_fut_params = None if no_trend else np.reshape(
        bias_fut_params, (-1, bias_fut_params.shape[-1]))
    tmp = np.reshape(subset, (-1, subset.shape[-1])).T
    tmp = quantile_delta_mapping(
        tmp, np.reshape(base_params, (-1, base_params.shape[-1])),
        np.reshape(bias_params, (-1, bias_params.shape[-1])),
        bias_fut_params, relative=relative, delta_denom_min=delta_denom_min,
        delta_denom_zero=delta_denom_zero, delta_range=delta_range)
    return np.reshape(tmp.T, subset.shape)


def closest_time_idx(time_index, time_window_center):
    """bias_transforms.py:788-791"""
    return np.array([np.argmin(abs(d - np.asarray(time_window_center)))
                     for d in time_index.day_of_year])


def _qdm_core(data, base_dset, feature_name, bias_fp, date_range_kwargs,
              lr_padded_slice, relative, no_trend, delta_denom_min,
              delta_denom_zero, delta_range, dtype, presrat, k_range=None):
    msg = f'data was expected to be a 3D array but got shape {data.shape}'
    assert data.ndim == 3, msg
    data = np.asarray(data, dtype)
    time_index = make_time_index(date_range_kwargs)
    assert data.shape[-1] == time_index.size
    dist = bias_fp.get('dist', 'empirical')
    sampling = bias_fp.get('sampling', 'linear')
    assert dist == 'empirical' and sampling == 'linear', (dist, sampling)
    base_params = np.asarray(bias_fp[f'base_{base_dset}_params'], dtype)
    bias_params = np.asarray(bias_fp[f'bias_{feature_name}_params'], dtype)
    bias_fut_params = np.asarray(
        bias_fp[f'bias_fut_{feature_name}_params'], dtype)
    if presrat:
        bias_tau_fut = np.asarray(bias_fp[f'{feature_name}_tau_fut'], dtype)
        bias_tau_fut = bias_tau_fut.reshape(bias_tau_fut.shape[:2] + (1,))
        k_factor = np.asarray(bias_fp[f'{feature_name}_k_factor'], dtype)
        delta_denom_min = delta_denom_min or bias_fp['zero_rate_threshold']
        if k_range is not None:
            k_factor = np.maximum(k_factor, np.dtype(dtype).type(
                np.min(k_range)))
            k_factor = np.minimum(k_factor, np.dtype(dtype).type(
                np.max(k_range)))
    if lr_padded_slice is not None:
        spatial_slice = (lr_padded_slice[0], lr_padded_slice[1])
        base_params = base_params[spatial_slice]
        bias_params = bias_params[spatial_slice]
        bias_fut_params = bias_fut_params[spatial_slice]
        if presrat:
            bias_tau_fut = bias_tau_fut[spatial_slice]
            k_factor = k_factor[spatial_slice]
    data_unbiased = np.full_like(data, np.nan)
    closest = closest_time_idx(time_index, bias_fp['time_window_center'])
    for nt in set(closest):
        subset_idx = closest == nt
        subset = _apply_qdm(
            data[:, :, subset_idx], base_params[:, :, nt],
            bias_params[:, :, nt], bias_fut_params[:, :, nt],
            relative=relative, no_trend=no_trend,
            delta_denom_min=delta_denom_min,
            delta_denom_zero=delta_denom_zero, delta_range=delta_range)
        if presrat and not no_trend:
            subset = np.where(subset < bias_tau_fut, np.dtype(dtype).type(0),
                              subset * k_factor[:, :, nt:nt + 1])
        data_unbiased[:, :, subset_idx] = subset
    return data_unbiased


def local_qdm_bc(data, base_dset, feature_name, bias_fp, date_range_kwargs,
                 lr_padded_slice=None, relative=True, no_trend=False,
                 delta_denom_min=None, delta_denom_zero=None,
                 delta_range=None, out_range=None, dtype=np.float32):
    """bias_transforms.py:622-824"""
    out = _qdm_core(data, base_dset, feature_name, bias_fp,
                    date_range_kwargs, lr_padded_slice, relative, no_trend,
                    delta_denom_min, delta_denom_zero, delta_range, dtype,
                    presrat=False)
    out = _out_range(out, out_range)
    if not np.isfinite(out).all():
        raise RuntimeError(
            'QDM bias correction resulted in NaN / inf values! If this is a '
            'relative QDM, you may try setting ``delta_denom_min`` or '
            '``delta_denom_zero``')
    return out


def local_presrat_bc(data, base_dset, feature_name, bias_fp,
                     date_range_kwargs, lr_padded_slice=None, relative=True,
                     no_trend=False, delta_denom_min=None,
                     delta_denom_zero=None, delta_range=None, k_range=None,
                     out_range=None, dtype=np.float32):
    """bias_transforms.py:958-1137"""
    out = _qdm_core(data, base_dset, feature_name, bias_fp,
                    date_range_kwargs, lr_padded_slice, relative, no_trend,
                    delta_denom_min, delta_denom_zero, delta_range, dtype,
                    presrat=True, k_range=k_range)
    out = _out_range(out, out_range)
    if np.isnan(out).any():
        raise RuntimeError(
            'Presrat bias correction resulted in NaN values! If this is a '
            'relative QDM, you may try setting ``delta_denom_min`` or '
            '``delta_denom_zero``')
    return out


FUNCTIONS = {'global_linear_bc': global_linear_bc,
             'local_linear_bc': local_linear_bc,
             'monthly_local_linear_bc': monthly_local_linear_bc,
             'local_qdm_bc': local_qdm_bc,
             'local_presrat_bc': local_presrat_bc}


def pad_after(fn, data, pad_width, **kwargs):
    """the forward pass's order: ``fn`` on the un-padded window ``data``
    (s1, s2, t), then ``np.pad(mode='reflect')`` by ``pad_width``
    (forward_pass.py:66-72,122-186)"""
    return np.pad(fn(data, **kwargs), tuple(pad_width), mode='reflect')


def correct_chunk(chunk, method, kwargs, lr_features, time_index,
                  dtype=np.float32):
    """an ``ArrayStrategy.init_chunk`` chunk (un-padded ``input_data``)
    corrected feature by feature like ``bias_correct_features``
    (sup3r/bias/utilities.py:296-332); returns the corrected array"""
    out = np.array(chunk.input_data, dtype=dtype)
    for feature, kw in kwargs.items():
        i = list(lr_features).index(feature)
        kw = {k: v for k, v in kw.items() if k != 'threshold'}
        kw.setdefault('feature_name', feature)
        if method != 'global_linear_bc':
            kw['lr_padded_slice'] = chunk.lr_pad_slice
        if method in ('monthly_local_linear_bc', 'local_qdm_bc',
                      'local_presrat_bc'):
            kw['date_range_kwargs'] = time_index[chunk.lr_pad_slice[2]]
        if method == 'global_linear_bc':
            kw.pop('feature_name')
        out[..., i] = FUNCTIONS[method](out[..., i], dtype=dtype, **kw)
    return out


# ------------------------------------------------------------ seeded inputs
def seeded_qdm_tables(rng, shape, n_windows=4, n_q=101, feature='rsds',
                      base_dset='ghi', presrat=False):
    """gamma-distributed samples per site and time window -> ``n_q`` evenly
    spaced quantiles each (values in about [1, 60]): a factor mapping with
    the reference's dataset names and attributes"""
    s1, s2 = shape
    levels = np.linspace(0, 1, n_q)

    def dist(scale, shift):
        smp = rng.gamma(3.0, scale, size=(s1, s2, n_windows, 400)) + shift
        return np.quantile(smp, levels, axis=-1).transpose(1, 2, 3, 0).astype(
            np.float32)
    fp = {f'base_{base_dset}_params': dist(3.0, 1.0),
          f'bias_{feature}_params': dist(3.6, 1.5),
          f'bias_fut_{feature}_params': dist(4.0, 2.0),
          'time_window_center': (np.arange(n_windows) + 0.5) * (
              365.0 / n_windows),
          'dist': 'empirical', 'sampling': 'linear', 'log_base': 10}
    if presrat:
        fp[f'{feature}_tau_fut'] = rng.uniform(
            2.0, 6.0, (s1, s2, 1)).astype(np.float32)
        fp[f'{feature}_k_factor'] = rng.uniform(
            0.8, 1.25, (s1, s2, n_windows)).astype(np.float32)
        fp['zero_rate_threshold'] = 1.182033e-5
    return fp


def seeded_linear_tables(rng, shape, feature='u_10m', months=12):
    s1, s2 = shape
    dims = (s1, s2) if not months else (s1, s2, months)
    return {f'{feature}_scalar': rng.uniform(0.7, 1.4, dims).astype(
                np.float32),
            f'{feature}_adder': rng.uniform(-2.0, 2.0, dims).astype(
                np.float32)}
