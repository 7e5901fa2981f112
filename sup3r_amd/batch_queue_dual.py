"""Batch queue and handler for paired low-res / high-res data.

``DualBatchQueue`` (sup3r/preprocessing/batch_queues/dual.py) restated over
samplers that hand out tuples ``(low_res, high_res[, obs])``
(:class:`~sup3r_amd.samplers.DeviceDualSampler`, or anything duck-typed like
it with ``dset_names``, ``s_enhance`` and ``t_enhance``): the low-res member is
data of its own, so nothing is coarsened; the batch members are named after
the sampler's, ``obs`` (NaN where nothing was observed) included for
``Sup3rGanWithObs``.

Smoothing: 4-D batches are smoothed with ``s3_gaussian_smooth`` like those of
the single-source queue.  5-D batches with ``smoothing`` set raise
``NotImplementedError``: the reference filters every ``(s1, s2, t)`` volume
there — over time as well (dual.py:78-82) — and the device kernel filters the
two spatial axes only.  The features skipped by ``smoothing_ignore`` are
matched against ``lr_features`` (the names of the low-res channels); the
reference indexes ``features`` with the low-res channel number, which is the
same name whenever the low-res features lead the feature list.
"""
import ctypes as C

import numpy as np

from .batch_queue import DeviceBatchHandler, DeviceBatchQueue
from .samplers import DeviceDualSampler
from .samplers_cc import DeviceDualSamplerCC


class DeviceDualBatchQueue(DeviceBatchQueue):
    """``DualBatchQueue``: batches of ``samplers[0].dset_names`` members."""

    def __init__(self, samplers, **kwargs):
        self.BATCH_MEMBERS = tuple(samplers[0].dset_names)
        super().__init__(samplers, **kwargs)
        self.check_enhancement_factors()

    @property
    def queue_shape(self):
        """shapes of what a sampler hands out: low_res, high_res and — with
        observations — the hi-res box with the output features"""
        obs_shape = self.hr_shape[:-1] + (len(self.hr_out_features),)
        shapes = [(self.batch_size,) + self.lr_shape,
                  (self.batch_size,) + self.hr_shape,
                  (self.batch_size,) + obs_shape]
        return shapes[:len(self.BATCH_MEMBERS)]

    def check_enhancement_factors(self):
        """every sampler must pair its cubes with the queue's factors"""
        s_factors = [c.s_enhance for c in self.containers]
        assert all(self.s_enhance == s for s in s_factors), (
            f'Received s_enhance = {self.s_enhance} but not all DualSamplers '
            f'in the collection have the same value: {s_factors}.')
        t_factors = [c.t_enhance for c in self.containers]
        assert all(self.t_enhance == t for t in t_factors), (
            f'Received t_enhance = {self.t_enhance} but not all DualSamplers '
            f'in the collection have the same value: {t_factors}.')

    def transform(self, samples, smoothing=None, smoothing_ignore=None):
        """no coarsening: ``low_res`` is smoothed if asked for, the other
        members pass through"""
        if self._transform is not None:
            return self._transform(samples, smoothing=smoothing,
                                   smoothing_ignore=smoothing_ignore)
        low_res = samples[0]
        if smoothing is None:
            return (low_res, *samples[1:])
        if len(low_res.shape) != 4:
            raise NotImplementedError(
                'smoothing of 5-D dual batches: the reference filters every '
                '(s1, s2, t) volume, over time as well (batch_queues/dual.py:'
                '78-82); s3_gaussian_smooth filters the two spatial axes only')
        from . import _lib
        from .batch_transform import gaussian_taps
        from .engine import Device
        dev = Device.get()
        x = dev.to_device(low_res)
        n, s1, s2, c = (int(v) for v in x.shape)
        skip = smoothing_ignore or ()
        mask = sum(1 << j for j in range(c) if self.lr_features[j] not in skip)
        taps, radius = gaussian_taps(smoothing)
        w = np.ascontiguousarray(taps, dtype=np.float32)
        tmp, out = dev.empty(tuple(x.shape)), dev.empty(tuple(x.shape))
        rc = _lib.lib().s3_gaussian_smooth(
            dev.ctx, C.c_void_p(x.data_ptr()), n, s1, s2, 1, c,
            w.ctypes.data_as(C.POINTER(C.c_float)), radius, mask,
            C.c_void_p(tmp.data_ptr()), C.c_void_p(out.data_ptr()))
        _lib.check(rc, dev.ctx, 's3_gaussian_smooth')
        return (out, *samples[1:])


class DeviceDualBatchHandler(DeviceBatchHandler, DeviceDualBatchQueue):
    """``DualBatchHandler``: a training and a validation
    :class:`DeviceDualBatchQueue` + means / stds."""

    VAL_QUEUE = DeviceDualBatchQueue
    SAMPLER = DeviceDualSampler


class DeviceBatchHandlerCC(DeviceDualBatchHandler):
    """``BatchHandlerCC`` (batch_handlers/factory.py:319-321:
    ``BatchHandlerFactory(DualBatchQueue, DualSamplerCC)``): the dual queues
    over :class:`~sup3r_amd.samplers_cc.DeviceDualSamplerCC` samplers, which
    hand out daily low-res / hourly high-res batches with the clearsky ratio
    reduced to daylight and filled — what ``SolarCC`` trains on."""

    SAMPLER = DeviceDualSamplerCC


# the reference's names
DualBatchQueue, DualBatchHandler = DeviceDualBatchQueue, DeviceDualBatchHandler
BatchHandlerCC = DeviceBatchHandlerCC

__all__ = ['DeviceDualBatchQueue', 'DeviceDualBatchHandler', 'DualBatchQueue',
           'DualBatchHandler', 'DeviceBatchHandlerCC', 'BatchHandlerCC']
