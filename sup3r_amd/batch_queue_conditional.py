"""Batch queues and handlers for ``Sup3rCondMom`` on the device.

``Sup3rCondMom`` trains on batches that carry ``.output`` (the moment to
learn) and ``.mask`` next to ``.low_res`` / ``.high_res``.  The reference
builds both on the host (``ConditionalBatchQueue`` and its six ``QueueMom*``
subclasses, sup3r/preprocessing/batch_queues/conditional.py, with
``scipy.ndimage.zoom`` / ``scipy.interpolate.interp1d`` on hi-res-sized
arrays, batch_queues/utilities.py:12-54, :106-173); the 2nd-moment queues also
bring the first-moment model's output back to the host.  Here the same
constructor arguments and the same six rules run as one streaming kernel over
the hi-res batch (``s3_condmom_target``, include/sup3r_hip.h): nothing leaves
the device between the sampler and ``Sup3rCondMom._train_step``.

===============  =========================  ============================
queue            output                     kernel flags
===============  =========================  ============================
``Mom1``         HR (the same tensor)       — (no kernel call)
``Mom1SF``       HR - LR^                   subfilter
``Mom2``         (HR - <HR|LR>)^2           first moment, square
``Mom2Sep``      HR^2                       square
``Mom2SF``       (HR - LR^ - <SF|LR>)^2     subfilter, first moment, square
``Mom2SepSF``    (HR - LR^)^2               subfilter, square
===============  =========================  ============================

LR^ is the low-res batch enhanced back to the hi-res grid (a repeat in space;
in time a repeat, ``time_enhance_mode='constant'``, or linear interpolation
between / extrapolation past the low-res time steps, ``'linear'``); <.|LR> is
``lower_models[1]``'s output with the truth's exogenous channels behind it.

Deviation from the reference: ``time_enhance_mode='linear'`` with a single
low-res time step is a ``ValueError`` here; scipy's ``interp1d`` returns NaN
for it without a word.
"""
import ctypes as C

from .batch_queue import DeviceBatchHandler, DeviceBatchQueue, DsetTuple

TIME_ENHANCE_MODES = ('constant', 'linear')


def mask_box(shape, s_padding=0, t_padding=0, end_t_padding=False,
             t_enhance=1):
    """``(s_pad, t_lo, t_hi)`` of ``ConditionalBatchQueue.make_mask``
    (conditional.py:111-125) for a hi-res batch of ``shape``: the mask is 1 on
    ``[s_pad, s - s_pad)`` of both spatial axes and on ``[t_lo, t_hi)`` of the
    time axis (4-D batches: the whole of it)."""
    s_pad, t_pad = int(s_padding or 0), int(t_padding or 0)
    if len(shape) == 4:
        return s_pad, 0, 1
    t_max = None if t_pad == 0 else -t_pad
    if end_t_padding and t_enhance > 1:
        t_max = 1 - t_enhance - (0 if t_max is None else t_pad)
    t_lo, t_hi, _ = slice(t_pad, t_max).indices(int(shape[3]))
    return s_pad, t_lo, max(t_hi, t_lo)


class DeviceCondMomTarget:
    """``target(hr, lr, mom1, ...) -> (output, mask)`` device tensors: the
    python side of ``s3_condmom_target``."""

    def __init__(self, s_enhance, t_enhance, hr_features_ind, device=None):
        from .engine import Device
        self.s_enhance, self.t_enhance = int(s_enhance), int(t_enhance)
        self.hr_features_ind = [int(i) for i in hr_features_ind]
        self.dev = device or Device.get()

    def __call__(self, hr, lr=None, mom1=None, subfilter=False, square=False,
                 mode='constant', box=None, output=True):
        """``subfilter``: subtract the enhanced ``lr``; ``mom1`` (not None):
        subtract it; ``square``: square the result.  ``box`` (not None): also
        return the mask of that ``(s_pad, t_lo, t_hi)``.  ``output=False``:
        only the mask."""
        from . import _lib
        L, dev = _lib.lib(), self.dev
        hr = dev.to_device(hr)
        is_5d = hr.dim() == 5
        n, s1, s2 = (int(v) for v in hr.shape[:3])
        t = int(hr.shape[3]) if is_5d else 1
        c_hr = int(hr.shape[-1])
        te = self.t_enhance if is_5d else 1
        flags, c_lr, c_m, cmap = 0, 0, 0, None
        if output and subfilter:
            lr = dev.to_device(lr)
            c_lr = int(lr.shape[-1])
            flags |= _lib.CM_SUBFILTER
            if mode == 'linear':
                flags |= _lib.CM_LINEAR
            cmap = (C.c_int32 * c_hr)(*self.hr_features_ind[:c_hr])
        if output and mom1 is not None:
            mom1 = dev.to_device(mom1)
            c_m = int(mom1.shape[-1])
            flags |= _lib.CM_MOM1
        if output and square:
            flags |= _lib.CM_SQUARE
        out = dev.empty(tuple(hr.shape)) if output else None
        mask = dev.empty(tuple(hr.shape)) if box is not None else None
        s_pad, t_lo, t_hi = box if box is not None else (0, 0, t)

        def ptr(x):
            return None if x is None else C.c_void_p(x.data_ptr())
        rc = L.s3_condmom_target(
            dev.ctx, ptr(hr), ptr(lr) if flags & _lib.CM_SUBFILTER else None,
            ptr(mom1) if flags & _lib.CM_MOM1 else None, n, s1, s2, t, c_hr,
            c_lr, c_m, cmap, self.s_enhance, te, flags, int(s_pad), int(t_lo),
            int(t_hi), ptr(out), ptr(mask))
        _lib.check(rc, dev.ctx, 's3_condmom_target')
        return out, mask


class DeviceConditionalBatchQueue(DeviceBatchQueue):
    """``ConditionalBatchQueue`` (conditional.py:22-166): batches of
    (low_res, high_res, output, mask), all four on the device.

    ``target``: the callable that computes output and mask (signature of
    :class:`DeviceCondMomTarget.__call__`); injectable like ``transform`` so
    that the queue logic runs without a device.

    The mask depends on the batch shape and the padding arguments only: it is
    built with the first batch of a shape and that tensor is handed out with
    every later batch.  Its consumers only read it (the masked loss kernel;
    a recorded training step copies it into its own input buffer), so the
    batches may share it."""

    BATCH_MEMBERS = ('low_res', 'high_res', 'output', 'mask')
    SUBFILTER = False      # output starts from HR - enhanced LR
    FIRST_MOMENT = False   # ... minus lower_models[1]'s output
    SQUARE = False         # ... squared

    def __init__(self, samplers, time_enhance_mode='constant',
                 lower_models=None, s_padding=0, t_padding=0,
                 end_t_padding=False, target=None, **kwargs):
        if time_enhance_mode not in TIME_ENHANCE_MODES:
            raise ValueError(f'time_enhance_mode "{time_enhance_mode}" is not '
                             f'one of {list(TIME_ENHANCE_MODES)}')
        self.time_enhance_mode = time_enhance_mode
        self.lower_models = lower_models
        self.s_padding = s_padding
        self.t_padding = t_padding
        self.end_t_padding = end_t_padding
        self._target = target
        self._masks = {}
        super().__init__(samplers, **kwargs)
        if self.SUBFILTER:
            self._check_time_steps(self.sample_shape[2], self.t_enhance)
        if self.FIRST_MOMENT:
            self.first_moment_model       # fail now, not in the first batch

    @property
    def first_moment_model(self):
        """``lower_models[1]``: the model of <HR|LR> (or <SF|LR>)"""
        if not self.lower_models or 1 not in self.lower_models:
            raise KeyError(f'{type(self).__name__} needs the first-moment '
                           'model as lower_models[1]')
        return self.lower_models[1]

    def _check_time_steps(self, t_hr, t_enhance):
        if self.time_enhance_mode == 'linear' and t_enhance > 1 \
                and t_hr // t_enhance < 2:
            raise ValueError(
                'time_enhance_mode "linear" needs at least two low-res time '
                f'steps, {t_hr} hi-res steps at t_enhance {t_enhance} give '
                f'{t_hr // t_enhance}')

    @property
    def target(self):
        if self._target is None:
            self._target = DeviceCondMomTarget(self.s_enhance, self.t_enhance,
                                               self.hr_features_ind)
        return self._target

    def _box(self, shape):
        return mask_box(shape, self.s_padding, self.t_padding,
                        self.end_t_padding, self.t_enhance)

    def make_mask(self, high_res):
        """1 where the loss counts: inside the spatial / temporal padding
        (conditional.py:79-127).  One tensor per batch shape."""
        shape = tuple(high_res.shape)
        if shape not in self._masks:
            self._masks[shape] = self.target(
                high_res, box=self._box(shape), output=False)[1]
        return self._masks[shape]

    def _first_moment(self, lr, hr):
        model = self.first_moment_model
        return model._tf_generate(lr, model.get_hr_exo_input(hr))

    def _make(self, samples, box=None):
        lr, hr = samples
        if not (self.SUBFILTER or self.FIRST_MOMENT or self.SQUARE):
            return hr, (None if box is None else
                        self.target(hr, box=box, output=False)[1])
        if self.SUBFILTER:
            if len(hr.shape) != 5 and self.t_enhance > 1:
                raise ValueError('Data must be 5D to do temporal enhancing, '
                                 f'but received: {tuple(lr.shape)}')
            if len(hr.shape) == 5:
                self._check_time_steps(int(hr.shape[3]), self.t_enhance)
        mom1 = self._first_moment(lr, hr) if self.FIRST_MOMENT else None
        return self.target(hr, lr=lr if self.SUBFILTER else None, mom1=mom1,
                           subfilter=self.SUBFILTER, square=self.SQUARE,
                           mode=self.time_enhance_mode, box=box)

    def make_output(self, samples):
        """the training target of ``samples = (low_res, high_res)``: the
        moment this queue's model learns (see the module docstring)"""
        return self._make(samples)[0]

    def post_proc(self, samples):
        lr, hr = self.transform(samples, **self.transform_kwargs)
        shape = tuple(hr.shape)
        if shape in self._masks:
            output = self.make_output((lr, hr))
        else:         # first batch of this shape: the same pass writes both
            output, self._masks[shape] = self._make((lr, hr),
                                                    box=self._box(shape))
        return DsetTuple(low_res=lr, high_res=hr, output=output,
                         mask=self._masks[shape])


class DeviceQueueMom1(DeviceConditionalBatchQueue):
    """first moment: the output is the hi-res batch itself"""


class DeviceQueueMom1SF(DeviceConditionalBatchQueue):
    """first moment of the subfilter field SF = HR - LR^"""
    SUBFILTER = True


class DeviceQueueMom2(DeviceConditionalBatchQueue):
    """second moment: (HR - <HR|LR>)^2"""
    FIRST_MOMENT = SQUARE = True


class DeviceQueueMom2Sep(DeviceQueueMom1):
    """second moment learned apart from the first: HR^2"""
    SQUARE = True


class DeviceQueueMom2SF(DeviceConditionalBatchQueue):
    """second moment of the subfilter field: (SF - <SF|LR>)^2"""
    SUBFILTER = FIRST_MOMENT = SQUARE = True


class DeviceQueueMom2SepSF(DeviceQueueMom1SF):
    """second moment of the subfilter field apart from the first: SF^2"""
    SQUARE = True


def _handler(queue_cls, suffix):
    """a training queue + a validation queue of ``queue_cls`` + means / stds
    (``BatchHandlerFactory``, batch_handlers/factory.py:33-310)"""
    name = 'DeviceBatchHandler' + suffix
    doc = (f'``BatchHandler{suffix}``: :class:`DeviceBatchHandler` whose two '
           f'queues are :class:`{queue_cls.__name__}`; takes the conditional '
           'arguments (``time_enhance_mode``, ``lower_models``, ``s_padding``,'
           ' ``t_padding``, ``end_t_padding``) next to the handler\'s.')
    return type(name, (DeviceBatchHandler, queue_cls),
                {'VAL_QUEUE': queue_cls, '__doc__': doc,
                 '__module__': __name__})


DeviceBatchHandlerMom1 = _handler(DeviceQueueMom1, 'Mom1')
DeviceBatchHandlerMom1SF = _handler(DeviceQueueMom1SF, 'Mom1SF')
DeviceBatchHandlerMom2 = _handler(DeviceQueueMom2, 'Mom2')
DeviceBatchHandlerMom2Sep = _handler(DeviceQueueMom2Sep, 'Mom2Sep')
DeviceBatchHandlerMom2SF = _handler(DeviceQueueMom2SF, 'Mom2SF')
DeviceBatchHandlerMom2SepSF = _handler(DeviceQueueMom2SepSF, 'Mom2SepSF')

# the reference's names
ConditionalBatchQueue = DeviceConditionalBatchQueue
QueueMom1, QueueMom1SF = DeviceQueueMom1, DeviceQueueMom1SF
QueueMom2, QueueMom2Sep = DeviceQueueMom2, DeviceQueueMom2Sep
QueueMom2SF, QueueMom2SepSF = DeviceQueueMom2SF, DeviceQueueMom2SepSF
BatchHandlerMom1 = DeviceBatchHandlerMom1
BatchHandlerMom1SF = DeviceBatchHandlerMom1SF
BatchHandlerMom2 = DeviceBatchHandlerMom2
BatchHandlerMom2Sep = DeviceBatchHandlerMom2Sep
BatchHandlerMom2SF = DeviceBatchHandlerMom2SF
BatchHandlerMom2SepSF = DeviceBatchHandlerMom2SepSF

__all__ = [
    'DeviceCondMomTarget', 'DeviceConditionalBatchQueue', 'mask_box',
    'DeviceQueueMom1', 'DeviceQueueMom1SF', 'DeviceQueueMom2',
    'DeviceQueueMom2Sep', 'DeviceQueueMom2SF', 'DeviceQueueMom2SepSF',
    'DeviceBatchHandlerMom1', 'DeviceBatchHandlerMom1SF',
    'DeviceBatchHandlerMom2', 'DeviceBatchHandlerMom2Sep',
    'DeviceBatchHandlerMom2SF', 'DeviceBatchHandlerMom2SepSF',
    'ConditionalBatchQueue', 'QueueMom1', 'QueueMom1SF', 'QueueMom2',
    'QueueMom2Sep', 'QueueMom2SF', 'QueueMom2SepSF', 'BatchHandlerMom1',
    'BatchHandlerMom1SF', 'BatchHandlerMom2', 'BatchHandlerMom2Sep',
    'BatchHandlerMom2SF', 'BatchHandlerMom2SepSF',
]
