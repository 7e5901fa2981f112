"""Numpy restatements of the two kernels behind ``SolarMultiStepGan``'s device
route (s3_branch_join, s3_time_pad_reflect) in fp32 with one rounding per
operation, and of ``SolarMultiStepGan.temporal_pad``
(sup3r/models/multi_step.py:785-852)."""
import numpy as np


def reflect_index(j, t):
    """source index of position ``j`` (any integer, array or scalar) of an
    axis of length ``t`` continued by repeated reflection about its two ends,
    numpy's ``mode='reflect'``: the triangle wave of period 2 (t - 1); a
    length-1 axis repeats its one value"""
    j = np.asarray(j, dtype=np.int64)
    if t == 1:
        return np.zeros_like(j)
    p = 2 * (t - 1)
    m = ((j % p) + p) % p
    return np.where(m < t, m, p - m)


def _unnorm(v, scale, shift):
    if scale is None or shift is None:
        return v
    m = v * np.asarray(scale, np.float32)
    assert m.dtype == np.float32
    return m + np.asarray(shift, np.float32)


def branch_join(ya, map_a, scale_a, shift_a, yb, map_b, scale_b, shift_b,
                mean=None, std=None):
    """ya = (t, h, w, ca), yb = (t, h, w, cb) float32 -> (1, h, w, t, na + nb):
    either source un-normalised per SOURCE channel, the mapped channels
    concatenated, time moved last, normalised per DESTINATION channel"""
    parts = []
    for y, cmap, sc, sh in ((ya, map_a, scale_a, shift_a),
                            (yb, map_b, scale_b, shift_b)):
        if len(cmap):
            assert y.dtype == np.float32
            parts.append(_unnorm(y, sc, sh)[..., list(cmap)])
    x = np.concatenate(parts, axis=3)
    x = np.ascontiguousarray(np.transpose(x, (1, 2, 0, 3))[None])
    if mean is not None and std is not None:
        d = x - np.asarray(mean, np.float32)
        x = d / np.asarray(std, np.float32)
    assert x.dtype == np.float32
    return x


def time_pad_reflect(y, pad, scale=None, shift=None):
    """y = (outer, t, c) float32 -> (outer, t + 2 pad, c), reflect-padded by
    index, then un-normalised"""
    t = y.shape[1]
    idx = reflect_index(np.arange(-pad, t + pad), t)
    out = _unnorm(np.ascontiguousarray(y[:, idx]), scale, shift)
    assert out.dtype == np.float32
    return out


def temporal_pad(n_lr_t, hi_res, t_enhance, mode='reflect'):
    """``SolarMultiStepGan.temporal_pad`` on a (1, s1, s2, t, c) array"""
    t_pad = int((n_lr_t * t_enhance - hi_res.shape[-2]) / 2)
    return np.pad(hi_res, ((0, 0), (0, 0), (0, 0), (t_pad, t_pad), (0, 0)),
                  mode=mode)
