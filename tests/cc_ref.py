"""numpy restatement of ``DualSamplerCC.__next__`` (sup3r/preprocessing/
samplers/cc.py:185-203) for the tests of ``sup3r_amd.samplers_cc``: the middle
days, the night mask of a 24-hour window, the first hour of the daylight
window with and without the device's clamp, and the nearest-neighbour fill by
brute force under the rule scipy's ``distance_transform_edt(return_indices=
True)`` follows — among the sources at the minimal squared distance, the one
with the smallest column-major index.  Nothing here imports ``sup3r_amd``."""
import numpy as np


# ------------------------------------------------------------------ the fill
def nn_fill_indices(holes):
    """``(ndim, *shape)`` indices of the source of every element of the bool
    array ``holes`` (True: to be filled): the element itself where it is no
    hole, else the non-hole minimising ``(squared distance, column-major
    index)``; all -1 where there is no source.  Brute force, every hole against
    every source."""
    holes = np.asarray(holes, dtype=bool)
    shape, nd = holes.shape, holes.ndim
    out = np.indices(shape).astype(np.int64)
    src = np.argwhere(~holes).astype(np.int64)             # (n_src, nd)
    dst = np.argwhere(holes).astype(np.int64)
    if len(dst) == 0:
        return out
    if len(src) == 0:
        out[(slice(None),) + tuple(dst.T)] = -1
        return out
    weight = np.cumprod((1,) + shape[:-1]).astype(np.int64)   # column-major
    fidx = src @ weight
    total = int(np.prod(shape))
    for lo in range(0, len(dst), 256):
        d = dst[lo:lo + 256]
        d2 = ((d[:, None, :] - src[None, :, :]) ** 2).sum(axis=2)
        best = np.argmin(d2 * total + fidx[None, :], axis=1)
        out[(slice(None),) + tuple(d.T)] = src[best].T
    return out


def nn_fill(block, channel):
    """copy of the ``(n, s1, s2, t, C)`` float32 ``block`` with the NaNs of
    ``channel`` filled; values move as bit patterns; returns (filled, number
    of NaNs found)"""
    bits = np.ascontiguousarray(block).view(np.uint32).copy()
    plane = bits[..., channel]
    holes = (plane & 0x7FFFFFFF) > 0x7F800000
    idx = nn_fill_indices(holes)
    if (idx >= 0).all():
        bits[..., channel] = plane[tuple(idx)]
    return bits.view(np.float32), int(holes.sum())


def tied_fills(holes):
    """number of holes that have more than one source at the minimal distance"""
    holes = np.asarray(holes, dtype=bool)
    src = np.argwhere(~holes).astype(np.int64)
    dst = np.argwhere(holes).astype(np.int64)
    if len(src) == 0 or len(dst) == 0:
        return 0
    tied = 0
    for lo in range(0, len(dst), 256):
        d2 = ((dst[lo:lo + 256, None, :] - src[None, :, :]) ** 2).sum(axis=2)
        tied += int(((d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    return tied


# -------------------------------------------------------- the daylight window
def middle_days(t_raw, t):
    """``(start, length)`` of the hours ``get_middle_days`` keeps of ``t_raw``
    raw hours for a sample of ``t`` steps: everything when one day was drawn,
    else ``max(t, 24)`` hours around the middle"""
    if int(t_raw / 24) > 1:
        mid = int(np.ceil(t_raw / 2))
        return mid - max(t // 2, 12), max(t, 24)
    return 0, t_raw


def night_mask(window):
    """``(n, s1, s2, 24)`` clearsky ratio -> bool[24], True where any is NaN"""
    return np.isnan(window).any(axis=(0, 1, 2))


def mask_word(night):
    return int(sum(1 << k for k, dark in enumerate(night) if dark))


def window_start(night, t):
    """``(raw, clamped)`` first hour of the ``t`` < 24 hours kept of a 24-hour
    window with the bool night mask ``night``.  ``raw``: the first daylight
    hour minus ``ceil((t - daylight hours) / 2)``, as in the reference;
    ``clamped``: ``raw`` brought into ``[0, 24 - t]``.  All night: both are the
    centred window's ``(24 - t) // 2``."""
    night = np.asarray(night, dtype=bool)
    assert night.shape == (24,) and 0 < t < 24
    if night.all():
        return (24 - t) // 2, (24 - t) // 2
    day = np.flatnonzero(~night)
    raw = int(day[0]) - int(np.ceil((t - len(day)) / 2))
    return raw, min(max(raw, 0), 24 - t)


# ------------------------------------------------------------------ __next__
def cc_next(daily, hourly, lr_origins, hr_origins, lr_box, hr_shape,
            t_enhance, lr_channels, hr_channels, i_cs):
    """the batch ``DualSamplerCC`` builds from the ``(S1, S2, T, C)`` cubes at
    the drawn origins (``hr_origins``: of the raw ``24 * lr_t``-hour boxes).
    ``i_cs``: position of clearsky_ratio among ``hr_channels``, or None.
    Returns ``(low_res, high_res, info)``; ``info`` has the mask word, both
    starts and the NaNs found (None where that stage does not run)."""
    l1, l2, lt = lr_box
    s1, s2, t = hr_shape
    low = np.stack([daily[i:i + l1, j:j + l2, k:k + lt][..., lr_channels]
                    for i, j, k in lr_origins])
    t_raw = lt * (1 if t_enhance == 1 else 24)
    raw = np.stack([hourly[i:i + s1, j:j + s2, k:k + t_raw][..., hr_channels]
                    for i, j, k in hr_origins])
    info = dict(mask=None, start_raw=None, start=None, filled=None)
    if i_cs is None or t_enhance == 1:
        return low, raw, info
    if t_enhance != 24:
        m0, mlen = middle_days(t_raw, t)
        raw = raw[:, :, :, m0:m0 + mlen]
        if t < raw.shape[3]:
            night = night_mask(raw[..., i_cs])
            r, c = window_start(night, t)
            info.update(mask=mask_word(night), start_raw=r, start=c)
            raw = raw[:, :, :, c:c + t]
    high, info['filled'] = nn_fill(raw, i_cs)
    return low, high, info
