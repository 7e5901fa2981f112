"""``DualSamplerCC`` over cubes resident on the device.

The reference's sampler for climate-change data (sup3r/preprocessing/samplers/
cc.py) pairs a DAILY low-res cube with an HOURLY high-res one: whatever
``t_enhance`` is, a low-res step is a day and the hi-res slice drawn with it is
its 24 hours.  After cutting the batch it works on the clearsky-ratio channel,
which is NaN every night:

* ``1 < t_enhance < 24``: the ``24 * lr_t`` raw hours of a sample are cut down
  to the middle ``max(t, 24)`` (``get_middle_days``) and, if ``t < 24``, to the
  ``t`` hours centred on the daylight of that 24-hour window
  (``nsrdb_reduce_daily_data``: an hour is night if the channel is NaN anywhere
  in the batch at that hour);
* the NaNs that are left are filled from the nearest non-NaN element of the
  ``(n, s1, s2, t)`` block (``nn_fill_array``, scipy's Euclidean distance
  transform with indices).

:class:`DeviceDualSamplerCC` does both without leaving the device
(include/sup3r_hip.h, ``kernels_cc.hip``): ``s3_cc_night_mask`` reads the
windows out of the resident cube through the box origins and leaves a 24-bit
word on the device, ``s3_cc_window_gather`` computes the first hour from that
word in every workgroup and copies only the hours that are kept, ``s3_nn_fill``
fills in place, bit-identically to scipy (ties go to the source with the
smallest column-major index).  Nothing is downloaded: what happened is in
``sampler.cc_status``, a device tensor of four int32 words (night mask, the
start as the reference computes it, the start used, NaNs found) that is read
only when someone asks.

Two deliberate deviations of the daylight window, both visible in
``cc_status``:

1. the reference's start ``first daylight hour - ceil((t - daylight hours) /
   2)`` can be negative or lie past ``24 - t`` (daylight in hours 0-7 with
   ``t = 12``: ``slice(-2, 10)`` of 24 steps is empty).  The device clamps it
   into ``[0, 24 - t]``: the batch always has ``t`` steps;
2. if all 24 hours are night the reference warns and returns the unreduced
   24 hours, a data-dependent shape.  The device takes the centred window,
   ``start = (24 - t) // 2`` (and the fill then finds the nearest daylight of
   the other samples, or leaves NaN if there is none).

``s_enhance > 1`` coarsens ``daily`` once, on the host, by block means in
float32 (NaN-skipping); xarray is not a dependency of this package, so that
this equals ``coarsen().mean()`` bit for bit is unverified.

With ``gather=`` stand-ins (samplers.py) the hi-res stand-in is asked for the
raw ``24 * lr_t``-hour boxes and the reduction runs through the numpy helpers
below with the device's clamp; ``gather['nn_fill']``, a callable ``(high_res,
channel) -> high_res``, stands in for the fill (none: no fill).
"""
import ctypes as C

import numpy as np

from .samplers import DeviceDualSampler

CSR = 'clearsky_ratio'


def nsrdb_reduce_daily_data(data, shape, csr_ind=0, clamp=False):
    """numpy ``nsrdb_reduce_daily_data`` (samplers/utilities.py:258-297):
    ``(n, s1, s2, 24, C)`` -> the ``shape`` hours centred on the daylight.
    ``clamp``: the device's two deviations instead of the reference's empty
    slices / unreduced return."""
    steps = data.shape[3]
    if shape >= steps:
        return data
    night = np.isnan(data[..., csr_ind]).any(axis=(0, 1, 2))
    if night.all():
        if not clamp:
            return data
        start = (steps - shape) // 2
    else:
        day = np.flatnonzero(~night)
        start = int(day[0]) - int(np.ceil((shape - len(day)) / 2))
        if clamp:
            start = min(max(start, 0), steps - shape)
    return data[:, :, :, slice(start, start + shape)]


def coarsen_daily(daily, s_enhance):
    """block means over ``s_enhance x s_enhance`` pixels of ``(S1, S2, T, C)``"""
    if hasattr(daily, 'cpu'):
        daily = daily.cpu().numpy()
    daily = np.asarray(daily, dtype=np.float32)
    s = int(s_enhance)
    S1, S2, T, Cc = daily.shape
    assert S1 % s == 0 and S2 % s == 0, (
        f'the daily raster {(S1, S2)} is no multiple of s_enhance = {s}')
    blocks = daily.reshape(S1 // s, s, S2 // s, s, T, Cc)
    return np.nanmean(blocks, axis=(1, 3), dtype=np.float32)


class DeviceDualSamplerCC(DeviceDualSampler):
    """``DualSamplerCC``: ``daily`` ``(L1 s, L2 s, TL, C_lr)`` and ``hourly``
    ``(L1 s, L2 s, 24 TL, C_hr)`` on the same raster (``daily`` is coarsened
    by ``s_enhance`` here).  ``sample_shape`` is the hi-res one, ``(s1, s2,
    t)`` with ``t = lr_t * t_enhance``.  ``next(sampler)`` is ``(low_res,
    high_res)``; with ``clearsky_ratio`` among the output features and
    ``t_enhance != 1`` the hi-res member is reduced to daylight and filled as
    described in the module docstring, else it is the raw ``24 * lr_t``-hour
    box.  ``last_origins`` are the origins of those raw boxes."""

    def __init__(self, daily, hourly, lr_features, hr_features,
                 sample_shape=None, batch_size=16, s_enhance=1, t_enhance=24,
                 feature_sets=None, seed=None, device=None, gather=None):
        if int(t_enhance) == 1:
            # a spatial-only model: the daily data is its own truth
            hourly, hr_features = daily, lr_features
        if int(s_enhance) > 1:
            daily = coarsen_daily(daily, s_enhance)
        self._fill_stand_in = (gather or {}).get('nn_fill')
        super().__init__(daily, hourly, lr_features, hr_features,
                         sample_shape=sample_shape, batch_size=batch_size,
                         s_enhance=s_enhance, t_enhance=t_enhance,
                         feature_sets=feature_sets, seed=seed, device=device,
                         gather=gather)
        self.cc_status = None
        self._work = None
        if self._hr.tensor is not None:
            import torch
            from . import _lib
            self.cc_status = torch.zeros(
                _lib.CC_STATUS_WORDS, dtype=torch.int32,
                device=self._hr.dev.torch_device)

    # ------------------------------------------------------------- geometry
    @property
    def _hours_per_step(self):
        """hi-res steps drawn per low-res step"""
        return 1 if self.t_enhance == 1 else 24

    def check_for_consistent_shapes(self):
        enhanced = (self._lr.shape[0] * self.s_enhance,
                    self._lr.shape[1] * self.s_enhance,
                    self._lr.shape[2] * self._hours_per_step)
        assert self._hr.shape[:3] == enhanced, (
            f'hr_data.shape {self._hr.shape[:3]} and enhanced lr_data.shape '
            f'{enhanced} are not compatible with the given enhancement '
            f'factors t_enhance = {self.t_enhance}, s_enhance = '
            f'{self.s_enhance}')

    def get_sample_index(self, n_obs=None):
        """the parent's low-res index; the hi-res time slice is ``24 x`` the
        low-res one whatever ``t_enhance`` is (``1 x`` for ``t_enhance = 1``)"""
        lr, hr = super().get_sample_index(n_obs=n_obs)
        f = self._hours_per_step
        return lr, (*hr[:2], slice(f * lr[2].start, f * lr[2].stop), hr[-1])

    def _fast_batch_possible(self):
        """``24 * lr_t * batch_size`` raw hours must fit the time axis of
        ``self.data`` — in the reference a ``Sup3rDataset`` whose shape is that
        of its LAST member, the hi-res (hourly) one"""
        return (self._hours_per_step * self.lr_sample_shape[2]
                * self.batch_size <= self._hr.shape[2])

    # --------------------------------------------------------- host helpers
    @staticmethod
    def get_middle_days(high_res, sample_shape):
        """the middle ``max(t, 24)`` hours of ``(n, s1, s2, t_raw, C)`` if
        more than one day was drawn, else everything"""
        steps = high_res.shape[3]
        if int(steps / 24) > 1:
            mid = int(np.ceil(steps / 2))
            start = mid - max(sample_shape[-1] // 2, 12)
            high_res = high_res[:, :, :, slice(
                start, start + max(sample_shape[-1], 24))]
        return high_res

    def reduce_high_res_sub_daily(self, high_res, csr_ind=0, clamp=False):
        """hourly ``(n, s1, s2, t_raw, C)`` -> ``t`` steps: middle days, then
        daylight hours; only for ``1 < t_enhance < 24``"""
        if self.t_enhance not in (24, 1):
            high_res = self.get_middle_days(high_res, self.hr_sample_shape)
            high_res = nsrdb_reduce_daily_data(
                high_res, self.hr_sample_shape[-1], csr_ind=csr_ind,
                clamp=clamp)
        return high_res

    def _middle(self, t_raw):
        """(first hour, hours) that ``get_middle_days`` keeps of ``t_raw``"""
        t = self.hr_sample_shape[2]
        if self.t_enhance in (24, 1) or int(t_raw / 24) <= 1:
            return 0, t_raw
        return int(np.ceil(t_raw / 2)) - max(t // 2, 12), max(t, 24)

    @property
    def csr_index(self):
        """position of clearsky_ratio in the hi-res sample if the daylight
        reduction and the fill apply, else None"""
        out = self.hr_out_features
        if CSR in out and self.t_enhance != 1:
            return out.index(CSR)
        return None

    # ----------------------------------------------------------------- next
    def __next__(self):
        indices = self._batch_indices()
        n = self.batch_size
        t_raw = self._hours_per_step * self.lr_sample_shape[2]
        lr_org = self._origins([ix[0] for ix in indices],
                               self.lr_sample_shape[2], n)
        hr_org = self._origins([ix[1] for ix in indices], t_raw, n)
        self.last_lr_origins, self.last_origins = lr_org, hr_org
        low = self._lr.gather(lr_org, self.lr_sample_shape,
                              self._lr.channels(self.lr_features))
        s1, s2, t = self.hr_sample_shape
        channels = self._hr.channels(self.hr_features)
        i_cs = self.csr_index
        if i_cs is None:
            return low, self._hr.gather(hr_org, (s1, s2, t_raw), channels)
        if self._hr.tensor is None:                  # stand-in gathers
            high = self._hr.gather(hr_org, (s1, s2, t_raw), channels)
            high = self.reduce_high_res_sub_daily(high, csr_ind=i_cs,
                                                  clamp=True)
            if self._fill_stand_in is not None:
                high = self._fill_stand_in(high, i_cs)
            return low, high
        start, hours = self._middle(t_raw)
        org = hr_org + np.array([0, 0, start], dtype=np.int32)
        if t >= hours:
            high = self._hr.gather(org, (s1, s2, hours), channels)
        else:
            high = self._daylight_gather(org, (s1, s2, t), channels,
                                         channels[i_cs])
        self._nn_fill(high, i_cs)
        return low, high

    def _daylight_gather(self, origins, box, channels, csr_channel):
        """night mask of the 24-hour windows at ``origins``, then the ``t``
        hours of them that start where the mask says"""
        from . import _lib
        cube, dev = self._hr.tensor, self._hr.dev
        if len(channels) > self._hr.max_channels:
            raise ValueError(f'a sample carries at most '
                             f'{self._hr.max_channels} features, '
                             f'{len(channels)} were asked for')
        org = np.ascontiguousarray(origins, dtype=np.int32).reshape(-1, 3)
        ch = np.ascontiguousarray(channels, dtype=np.int32)
        S1, S2, T, Cc = self._hr.shape
        s1, s2, t = box
        ip = C.POINTER(C.c_int32)
        status = C.c_void_p(self.cc_status.data_ptr())
        L = _lib.lib()
        rc = L.s3_cc_night_mask(
            dev.ctx, C.c_void_p(cube.data_ptr()), S1, S2, T, Cc,
            org.ctypes.data_as(ip), len(org), s1, s2, int(csr_channel), status)
        _lib.check(rc, dev.ctx, 's3_cc_night_mask')
        out = dev.empty((len(org), s1, s2, t, len(ch)))
        rc = L.s3_cc_window_gather(
            dev.ctx, C.c_void_p(cube.data_ptr()), S1, S2, T, Cc,
            org.ctypes.data_as(ip), len(org), s1, s2, t,
            ch.ctypes.data_as(ip), len(ch), status,
            C.c_void_p(out.data_ptr()))
        _lib.check(rc, dev.ctx, 's3_cc_window_gather')
        return out

    def _nn_fill(self, high, channel):
        """``s3_nn_fill`` on ``channel`` of the batch, in place; the key
        workspace is kept from batch to batch"""
        from . import _lib
        dev = self._hr.dev
        n, s1, s2, t, c = (int(v) for v in high.shape)
        keys = n * s1 * s2 * t
        if self._work is None or self._work.numel() < 2 * keys:
            self._work = dev.empty((2 * keys,))            # 8 bytes per key
        rc = _lib.lib().s3_nn_fill(
            dev.ctx, C.c_void_p(high.data_ptr()), n, s1, s2, t, c,
            int(channel), C.c_void_p(self._work.data_ptr()),
            C.c_void_p(self.cc_status.data_ptr() + 4 * _lib.CC_FILLED))
        _lib.check(rc, dev.ctx, 's3_nn_fill')


# the reference's name
DualSamplerCC = DeviceDualSamplerCC

__all__ = ['DeviceDualSamplerCC', 'DualSamplerCC']
