"""Data-centric batch queues and handler: what ``Sup3rGanDC`` trains from.

``Sup3rGanDC`` (data_centric.py) scores one validation batch per (space bin,
time bin) after every epoch and hands the normalised scores back as sampling
weights.  The reference's ``BatchQueueDC`` / ``ValBatchQueueDC``
(sup3r/preprocessing/batch_queues/dc.py) and ``BatchHandlerDC``
(batch_handlers/dc.py) restated over samplers with ``update_weights``
(:class:`~sup3r_amd.samplers.DeviceSamplerDC`, or anything duck-typed like it).

Deviation from the reference, on purpose: batch ``i`` of a validation pass is
drawn from space bin ``i // n_time_bins`` and time bin ``i % n_time_bins``.
The reference draws it from ``i % n_space_bins`` and ``i % n_time_bins``
(batch_queues/dc.py:105-127); when the two bin counts share a factor that rule
visits some cells twice and others never (2 x 4: four of the eight cells), and
it disagrees with the cell ``(i // n_time_bins, i % n_time_bins)`` under which
``Sup3rGanDC.calc_val_loss_gen`` files the loss of batch ``i`` — in the
reference (models/dc.py:59-60) and here.
"""
import numpy as np

from .batch_queue import DeviceBatchHandler, DeviceBatchQueue, _as_arrays
from .samplers import DeviceSamplerDC


class DeviceBatchQueueDC(DeviceBatchQueue):
    """``BatchQueueDC``: every draw first pushes the queue's current bin
    weights into the sampler it draws from.  The weights start uniform;
    ``update_weights`` replaces them (``Sup3rGanDC.calc_val_loss``)."""

    def __init__(self, samplers, n_space_bins=1, n_time_bins=1, **kwargs):
        self.n_space_bins, self.n_time_bins = int(n_space_bins), \
            int(n_time_bins)
        self._spatial_weights = np.ones(self.n_space_bins) / self.n_space_bins
        self._temporal_weights = np.ones(self.n_time_bins) / self.n_time_bins
        super().__init__(samplers, **kwargs)

    @property
    def spatial_weights(self):
        return self._spatial_weights

    @property
    def temporal_weights(self):
        return self._temporal_weights

    def update_weights(self, spatial_weights, temporal_weights):
        self._spatial_weights = spatial_weights
        self._temporal_weights = temporal_weights

    def _bin_weights(self):
        """(spatial, temporal) weights of the draw about to be made"""
        return self.spatial_weights, self.temporal_weights

    def sample_batch(self):
        sampler = self.get_random_container()
        sampler.update_weights(*self._bin_weights())
        return _as_arrays(next(sampler))


class DeviceValBatchQueueDC(DeviceBatchQueueDC):
    """``ValBatchQueueDC``: one batch per (space bin, time bin) cell, drawn
    with one-hot weights — draw ``i`` (counted over the life of the queue,
    modulo the number of cells) from space bin ``i // n_time_bins`` and time
    bin ``i % n_time_bins``, so a pass of ``n_space_bins * n_time_bins``
    batches visits every cell once, in the order ``Sup3rGanDC`` files the
    losses (see the module docstring: the reference takes both indices modulo
    their bin count).  Draws are counted, not hand-outs, so batches that a
    feeder thread of host samplers drew ahead keep their place; that needs
    ``max_workers`` 1."""

    def __init__(self, samplers, n_space_bins=1, n_time_bins=1, **kwargs):
        self._draws = 0
        super().__init__(samplers, n_space_bins=n_space_bins,
                         n_time_bins=n_time_bins, **kwargs)
        self.n_batches = self.n_space_bins * self.n_time_bins

    def _bin_weights(self):
        with self._rng_lock:
            cell = self._draws % (self.n_space_bins * self.n_time_bins)
            self._draws += 1
        self._spatial_weights = np.eye(
            1, self.n_space_bins, cell // self.n_time_bins,
            dtype=np.float32)[0]
        self._temporal_weights = np.eye(
            1, self.n_time_bins, cell % self.n_time_bins, dtype=np.float32)[0]
        return self._spatial_weights, self._temporal_weights


class DeviceBatchHandlerDC(DeviceBatchHandler, DeviceBatchQueueDC):
    """``BatchHandlerDC``: a :class:`DeviceBatchQueueDC` to train from, a
    :class:`DeviceValBatchQueueDC` as ``val_data``, means / stds.  Takes
    ``n_space_bins`` / ``n_time_bins`` next to the handler's arguments.
    Validation samplers are required — the weights come from them — and there
    must be at least as many box starts / time starts as bins."""

    VAL_QUEUE = DeviceValBatchQueueDC
    SAMPLER = DeviceSamplerDC

    def __init__(self, train_samplers, val_samplers, **kwargs):
        assert val_samplers is not None and val_samplers != [], (
            f'{type(self).__name__} requires validation data. If you do not '
            'plan to sample training data based on performance across '
            'validation data use another type of batch handler.')
        super().__init__(train_samplers, val_samplers, **kwargs)
        shape, box = self.containers[0].shape, self.sample_shape
        msg = (f'The requested sample_shape {box} is too large for the '
               f'requested number of bins (space = {self.n_space_bins}, time ='
               f' {self.n_time_bins}) and the shape of the sample data '
               f'{tuple(shape[:3])}.')
        assert self.n_space_bins <= (shape[0] - box[0] + 1) * \
            (shape[1] - box[1] + 1), msg
        assert self.n_time_bins <= shape[2] - box[2] + 1, msg


# the reference's names
BatchQueueDC, ValBatchQueueDC = DeviceBatchQueueDC, DeviceValBatchQueueDC
BatchHandlerDC = DeviceBatchHandlerDC

__all__ = ['DeviceBatchQueueDC', 'DeviceValBatchQueueDC',
           'DeviceBatchHandlerDC', 'BatchQueueDC', 'ValBatchQueueDC',
           'BatchHandlerDC']
