"""The cases of tests/test_disc_exact_gpu.py (TEST INFRASTRUCTURE): short conv
stacks with the discriminator's channel counts (sup3r_amd/configs/disc_st.json),
their integer data, the float64 reference (tests/support_ref.py) and the proof
that the comparison may be ``assert_array_equal``.

No device is touched here: tests/test_disc_exact_ref_cpu.py builds every case in
the CPU suite, so that no case reaches a GPU with an unmet condition.

Exactness conditions, asserted by ``build`` on the reference of every case:
  * x integers in [-3, 3], d_out integers in [-4, 4] (narrower where a case says
    so), biases integers in [-2, 2], filters one +-1 per output channel;
  * activations None / ReLU / LeakyReLU 0.25 or 0.5 (dyadic slopes);
  * every tensor a bf16 plan may store — each conv's input, each activation,
    each dPre — survives the round trip through bf16;
  * every bias / weight-gradient sum stays below 2^24 units of its granularity
    (``_reference``), so fp32 sums are exact in any order.
A split-bf16 (BF16X3) plan of the same case has a zero low part everywhere: the
same reference holds bit for bit.
"""
import functools
import zlib

import numpy as np

from tests import support_ref as R
from tests.test_train_support_gpu import _bf16_exact, _clean, _data, _reference, _weights

NOMINAL_CU = 256      # CU count the CPU suite builds the CU-dependent shapes for

# the "fills the chip" floors of the specialised kernels, lowered so that small
# shapes reach them
MIN1 = {'HALO_S2_MIN_TILES': 1, 'HALO32_MIN_TILES': 1, 'DGRAD_S2_MIN_TILES': 1, 'FEWCH_HALO_MIN_TILES': 1}
COUNTERS = ('persist_dgrad', 'gconv_splitk', 'dgrad_c2_slide', 'halo_s2_k64', 'fewch_halo', 'fewch_halo_signs',
            'dgrad_s2_o16', 'dgrad_s2_mb')


def conv(filters, strides=1, padding='valid', act=None, w='inj'):
    """Conv3D k = 3 (+ activation: 'relu', or a LeakyReLU slope)"""
    out = [{'class': 'Conv3D', 'filters': filters, 'kernel_size': 3, 'strides': strides, 'padding': padding, '_w': w}]
    if act == 'relu':
        out.append({'class': 'ReLU'})
    elif act is not None:
        assert act in (0.25, 0.5), 'dyadic slopes only'
        out.append({'class': 'LeakyReLU', 'alpha': act})
    return out


def front(padding='valid', acts=(0.25, 'relu', None), c=(32, 32, 64)):
    """2 -> 32, 32 -> 32 stride 2, 32 -> 64 (disc_st.json's first three convs).
    The first filter is any one-hot (its data gradient lands in fp32), the
    stride-2 one a permutation where it can be (its data gradient is ONE value
    per cell: what the plan stores as bf16 stays a short sum), else injective."""
    return (conv(c[0], 1, padding, acts[0], 'one_hot') +
            conv(c[1], 2, padding, acts[1], 'perm' if c[0] == c[1] else 'inj') +
            (conv(c[2], 1, padding, acts[2], 'inj') if len(c) > 2 else []))


def back(padding='valid', acts=('relu', 'relu', 'relu', None)):
    """2 -> 32, 32 -> 64, 64 -> 64 stride 2, 64 -> 128"""
    return (conv(32, 1, padding, acts[0], 'one_hot') + conv(64, 1, padding, acts[1], 'inj') +
            conv(64, 2, padding, acts[2], 'perm') + conv(128, 1, padding, acts[3], 'inj'))


def back_short(padding='valid', acts=('relu', 'relu', None)):
    """2 -> 64, 64 -> 64 stride 2, 64 -> 128: the 64-channel stride-2 conv right
    behind a few-channel conv (a cheap reference at many tiles)"""
    return (conv(64, 1, padding, acts[0], 'one_hot') + conv(64, 2, padding, acts[1], 'perm') +
            (conv(128, 1, padding, acts[2], 'inj') if len(acts) > 2 else []))


def _k(fwd=None, dgrad=None, wgrad=None):
    return {k: v for k, v in (('fwd', fwd), ('dgrad', dgrad), ('wgrad', wgrad)) if v is not None}


def _tiles(o, tile):
    return int(np.prod([-(-a // b) for a, b in zip(o, tile)]))


def _n_for_tiles(per_sample, cu):
    """smallest batch with more tiles than CUs (workgroups of a persistent
    kernel) and a tile count that is no multiple of 8 (unequal XCD shares)"""
    n = cu // per_sample + 1
    while (n * per_sample) % 8 == 0:
        n += 1
    return n


# --------------------------------------------------------------------- cases
# name -> dict(spec, shape (or CU count -> shape), d_lim, options, precision,
#              kernels {conv index: {fwd / dgrad / wgrad}}, counters {name: count},
#              io {conv index: {in16 / out16}}, ref (the case whose data and reference it shares))
CASES = {}


def _case(name, spec, shape, kernels, counters=None, options=None, d_lim=4, precision='bf16', io=None, ref=None,
          note=''):
    assert name not in CASES
    CASES[name] = dict(name=name, spec=spec, shape=shape, kernels=kernels, counters=counters or {},
                       options=dict(MIN1, **(options or {})), d_lim=d_lim, precision=precision, io=io or {},
                       ref=ref or name, note=note)


# the kernels of the front stack at shapes that reach all of them
_FRONT = {0: _k('gconv_fewch', 'c2', 'c2'), 1: _k('halo_s2', 's2', 'bf16_gen'), 2: _k('halo32', 'mfma_valid', 'bf16_gen')}
# the first conv writes bf16 + sign bytes on the LDS-halo walk; the stride-2 data
# gradient stores dPre of the first conv as bf16 only, masked from those bytes
_FRONT_CNT = {'fewch_halo': 1, 'fewch_halo_signs': 1, 'dgrad_s2_o16': 1, 'dgrad_s2_mb': 1, 'halo_s2_k64': 0,
              'dgrad_c2_slide': 0, 'persist_dgrad': 0}
_FRONT_IO = {0: {'in16': 0, 'out16': 1}, 1: {'in16': 1, 'out16': 1}, 2: {'in16': 1, 'out16': 0}}

# conv 2 outputs 5 x 9 x 17: one past the 2 x 4 x 16 tile of halo_s2 (and the 4 x 8 x 16
# one of dgrad_s2 over u = ceil(11 / 2), ceil(19 / 2), ceil(35 / 2) = 6, 10, 18: ragged) in
# every axis; conv 3 outputs 3 x 7 x 15: one below halo32's 4 x 8 x 16; conv 1 outputs
# 11 x 19 x 35: one below 3 x 3 x ... fewch-halo tiles of 4 x 8 x 32 + 3; conv 1's data
# gradient has 4 * 4 * 3 * 3 = 144 tiles (>= 64), 40 404 input positions (>= 4 096)
RAGGED = (4, 13, 21, 37, 2)
_case('front_ragged', front(), RAGGED, _FRONT, _FRONT_CNT, io=_FRONT_IO,
      note='two-fragment halo tile (NF = 2) as the 32 -> 64 data gradient: d_out is fp32, no bf16 dPre')
# conv 3 with an activation: its mask pass leaves the bf16 copy of dPre the persistent <2, true> form reads
# (T = 15 >= 8 time steps of dPre)
_case('front_ragged_persist', front(acts=(0.25, 'relu', 'relu')), RAGGED, _FRONT, dict(_FRONT_CNT, persist_dgrad=1),
      options={'PERSIST_DGRAD_MIN_TILES': 1}, io=_FRONT_IO)
# conv 2 outputs exactly one tile grid: 4 x 8 x 16 = 2 x 2 x 1 tiles of halo_s2, conv 3 outputs 2 x 6 x 14
_case('front_fit', front(acts=(0.5, 0.25, None)), (4, 11, 19, 35, 2), _FRONT, _FRONT_CNT, io=_FRONT_IO)
# one below the tile grid in every axis: conv 2 outputs 3 x 7 x 15 (N = 5: an odd batch)
_case('front_below', front(acts=(0.25, 0.5, None)), (5, 9, 17, 33, 2),
      {0: _k('gconv_fewch', 'c2', 'c2'), 1: _k('halo_s2', 's2', 'bf16_gen')}, _FRONT_CNT)
# one tile per sample, four tiles in all (fewer than the 8 XCDs: most workgroup slots of the
# XCD-interleaved walk are empty); 512 output positions, the floor of bf16_gen, which the
# bf16 input of halo_s2 hangs on.  48 tiles for dgrad_c2 (< 64): conv 1's data gradient is
# the gather kernel's, so nothing stores bf16 only
_case('front_few_tiles', front(acts=(0.25, None), c=(32, 32)), (4, 7, 11, 35, 2),
      {0: _k('gconv_fewch', 'gconv', 'c2'), 1: _k('halo_s2', 's2', 'bf16_gen')},
      {'fewch_halo': 1, 'dgrad_s2_o16': 0, 'dgrad_s2_mb': 0, 'halo_s2_k64': 0})


# more halo_s2 tiles (18 per sample) than CUs: every workgroup walks > 1 tile (prefetch of
# the next halo), the XCD shares are unequal
def _front_many(cu):
    return (_n_for_tiles(18, cu), 13, 21, 37, 2)


_case('front_many_tiles', front(acts=(0.25, 'relu'), c=(32, 32)), _front_many,
      {0: _k('gconv_fewch', 'c2', 'c2'), 1: _k('halo_s2', 's2', 'bf16_gen')}, _FRONT_CNT)

# ... the negative legs at the ragged shape: one specialised kernel switched off each, the
# gather kernels (gconv_mfma_kernel forward / adjoint, the gather walk of the few-channel
# conv) take the layer and op_info / the counters tell the plans apart
for _opt, _kern, _cnt in [
        ('NO_HALO_S2', {1: _k('gconv', 's2', 'bf16_gen')}, {}),
        ('NO_HALO32', {2: _k('gconv', 'mfma_valid', 'bf16_gen')}, {}),
        ('NO_FEWCH_HALO', {}, {'fewch_halo': 0, 'fewch_halo_signs': 0, 'dgrad_s2_mb': 0}),
        ('NO_SIGN_BYTES', {}, {'fewch_halo_signs': 0, 'dgrad_s2_mb': 0}),
        # (without its bf16-only consumers / producer nothing is stored as bf16 only)
        ('NO_DGRAD_S2', {1: _k('halo_s2', 'gconv', 'bf16_gen')}, {'dgrad_s2_o16': 0, 'dgrad_s2_mb': 0, 'fewch_halo_signs': 0}),
        ('NO_DGRAD_C2', {0: _k('gconv_fewch', 'gconv', 'c2')}, {'dgrad_s2_o16': 0, 'dgrad_s2_mb': 0})]:
    _case('front_ragged-' + _opt, front(), RAGGED, {**_FRONT, **_kern}, dict(_FRONT_CNT, **_cnt), options={_opt: 1},
          ref='front_ragged')

# the sliding-window form of the first conv's data gradient (bf16-only dPre, C_in = 2) at
# and below its floor: 4 * ceil(13 / 40) * ceil(21 / 16) * ceil(37 / 14) = 24 units
_SLIDE_UNITS = 4 * 1 * 2 * 3
_case('front_ragged-slide_at', front(), RAGGED, _FRONT, dict(_FRONT_CNT, dgrad_c2_slide=1),
      options={'DGRAD_C2_SLIDE_MIN_UNITS': _SLIDE_UNITS}, ref='front_ragged')
_case('front_ragged-slide_below', front(), RAGGED, _FRONT, _FRONT_CNT,
      options={'DGRAD_C2_SLIDE_MIN_UNITS': _SLIDE_UNITS + 1}, ref='front_ragged')


# C_in = 4 into the few-channel kernels (dgrad_c2 takes 1 ... 4 channels; wgrad_c2 only 2)
_case('front_cin4', front(), (4, 13, 21, 37, 4), {0: _k('gconv_fewch', 'c2'), 1: _k('halo_s2', 's2', 'bf16_gen')},
      {'fewch_halo': 1, 'dgrad_s2_o16': 0, 'dgrad_c2_slide': 0})

# dgrad_s2 with C_in = 16 (<2>, half-empty filter rows) and 64 (<4>): only C_in = 32 stores
# bf16.  wgrad_c2 with C_out = 16 and 64 on the first conv.  (C_in = 16 is below the gather
# kernel's 32 channels: that forward is the direct family's, fp32)
_case('s2_cin16', front(c=(16, 32, 64)), RAGGED, {0: _k('gconv_fewch', None, 'c2'), 1: _k(None, 's2')},
      {'dgrad_s2_o16': 0, 'dgrad_s2_mb': 0})
# (the gather forward of 64 -> 32: 54 K steps, 3 060 positions = 24 workgroups: split-K)
_case('s2_cin64', front(c=(64, 32, 64)), RAGGED, {0: _k('gconv_fewch', None, 'c2'), 1: _k('gconv', 's2', 'bf16_gen')},
      {'dgrad_s2_o16': 0, 'dgrad_s2_mb': 0, 'halo_s2_k64': 0, 'gconv_splitk': '>0'})

# halo32 with C_out = 32 (<2>) at lo = 0 and lo = 1 ('same'); the front stack has C_out = 64
# (<4>) at lo = 0, the 'same' stacks below at lo = 1.  Outputs 11 x 19 x 35 -> 9 x 17 x 33
# -> 9 x 17 x 33: one past the 4 x 8 x 16 tile
_case('halo32_c32', conv(32, 1, 'valid', 0.25, 'one_hot') + conv(32, 1, 'valid', 'relu', 'perm') +
      conv(32, 1, 'same', None, 'perm'), (2, 13, 21, 37, 2),
      {0: _k('gconv_fewch', None, 'c2'), 1: _k('halo32', 'gconv', 'bf16_gen'), 2: _k('halo32', 'gconv', 'bf16_gen')})

# ------------------------------------------------------------------ back stack
# conv 3 (64 -> 64 stride 2) outputs 5 x 9 x 17: one past the 2 x 2 x 16 tile of the k64 form
# in t, odd in s0 / s1; conv 4 outputs 3 x 7 x 15 (630 positions >= 512 for bf16_gen).
# Up to 1 024 positions a training plan hands a 64 -> C_out conv of the halo-tile family to
# the one-launch few-position kernels (plan.cpp, small_trunk); the 64 -> 128 conv is a subject
# of these cases, so that family is switched off (NO_FEWPOS) and the layer runs on the
# kernels it has at production sizes
_NO_FP = {'NO_FEWPOS': 1}
_BACK = {0: _k('gconv_fewch', None, 'c2'), 1: _k('halo32', 'mfma_valid', 'bf16_gen'), 2: _k('halo_s2', 'gconv', 'bf16_gen'),
         3: _k('mfma_tile', 'mfma_chunked', 'bf16_gen')}
_case('back_ragged', back(), (2, 15, 23, 39, 2), _BACK, {'halo_s2_k64': 1, 'fewch_halo': 1}, options=_NO_FP, d_lim=2)
_BACK_SHORT = {0: _k('gconv_fewch', 'gconv', 'c2'), 1: _k('halo_s2', 'gconv', 'bf16_gen'),
               2: _k('mfma_tile', 'mfma_chunked', 'bf16_gen')}
_case('back_short', back_short(), (2, 13, 21, 37, 2), _BACK_SHORT, {'halo_s2_k64': 1, 'fewch_halo': 1}, options=_NO_FP,
      d_lim=2)
# (the gather forward of 64 -> 64: 54 K steps over 1 530 positions = 12 workgroups: split-K)
_case('back_short-NO_HALO_S2_K64', back_short(), (2, 13, 21, 37, 2), {**_BACK_SHORT, **{1: _k('gconv', 'gconv', 'bf16_gen')}},
      {'halo_s2_k64': 0, 'gconv_splitk': '>0'}, options=dict(_NO_FP, NO_HALO_S2_K64=1), d_lim=2, ref='back_short')
# conv 2 outputs 2 x 2 x 16, one k64 tile per sample, 8 tiles / 512 positions in all; conv 3 then
# has no output left, so the stack ends at the stride-2 conv
_case('back_few_tiles', back_short(acts=('relu', None)), (8, 7, 7, 35, 2),
      {0: _k('gconv_fewch', None, 'c2'), 1: _k('halo_s2', 'gconv', 'bf16_gen')}, {'halo_s2_k64': 1}, d_lim=2)


# more k64 tiles (3 * 5 * 2 = 30 per sample) than CUs
def _back_many(cu):
    return (_n_for_tiles(30, cu), 13, 21, 37, 2)


_case('back_many_tiles', back_short(acts=('relu', None)), _back_many,
      {0: _k('gconv_fewch', None, 'c2'), 1: _k('halo_s2', 'gconv', 'bf16_gen')}, {'halo_s2_k64': 1}, d_lim=2)

# 64 -> 128 past the few-position sizes (6 930 outputs) and 128 -> 128 stride 2 behind it: the
# gather kernel forward and adjoint with four 32-channel K chunks per tap, bf16_gen with two
# C_in tiles of 64.  Outputs 4 x 5 x 17 (680 positions >= 512)
_case('deep', conv(64, 1, 'valid', 'relu', 'one_hot') + conv(128, 1, 'valid', 'relu', 'inj') +
      conv(128, 2, 'valid', None, 'perm'), (2, 13, 15, 39, 2),
      {0: _k('gconv_fewch', None, 'c2'), 1: _k('mfma_tile', 'mfma_chunked', 'bf16_gen'), 2: _k('gconv', 'gconv', 'bf16_gen')},
      {'halo_s2_k64': 0}, d_lim=2)

# ------------------------------------------------------------------- 'same'
# even extents: lo = 0 and one zero cell past the end, the stride-2 LDS kernels keep the
# layer; 'same' stride 1 with 32 input channels is halo32 at lo = 1, and the data gradient of
# 32 -> 64 'same' (a 64 -> 32 conv over the padded frame: conv_dgrad_mfma_supported) the
# halo-tile kernel's frame form with its fold
_FRONT_SAME = {0: _k('gconv_fewch', 'c2', 'c2'), 1: _k('halo_s2', 's2', 'bf16_gen'), 2: _k('halo32', 'mfma_frame', 'bf16_gen')}
_case('front_same_even', front('same'), (2, 24, 20, 44, 2), _FRONT_SAME, _FRONT_CNT)
# odd extents: lo = 1, the layer must fall to the gather kernels, forward and adjoint
_case('front_same_odd', front('same'), (3, 23, 21, 43, 2),
      {**_FRONT_SAME, **{1: _k('gconv', 'gconv', 'bf16_gen')}}, {'dgrad_s2_o16': 0, 'dgrad_s2_mb': 0, 'fewch_halo': 1})
# (64 -> 128 'same' is a trunk geometry: its weight gradient is the trunk kernel's, its data
# gradient the chunked frame form)
_BACK_SAME = {0: _k('gconv_fewch', None, 'c2'), 1: _k('halo32', 'mfma_frame', 'bf16_gen'), 2: _k('halo_s2', 'gconv', 'bf16_gen'),
              3: _k('mfma_tile', 'mfma_chunked', 'bf16_trunk')}
_case('back_same_even', back('same'), (1, 24, 20, 44, 2), _BACK_SAME, {'halo_s2_k64': 1}, d_lim=2)
_case('back_same_odd', back('same'), (1, 23, 21, 43, 2), {**_BACK_SAME, **{2: _k('gconv', 'gconv', 'bf16_gen')}},
      {'halo_s2_k64': 0}, d_lim=2)

# --------------------------------------------------------- split bf16 (BF16X3)
# the LDS-halo forwards are bf16-only: the gather kernels' x3 forms run forward, the x3
# forms of dgrad_c2 / dgrad_s2 / the halo tile and of both weight gradients backward
_X3 = {0: _k('gconv_fewch', 'c2', 'c2'), 1: _k('gconv', 's2', 'bf16_gen'), 2: _k('gconv', 'mfma_valid', 'bf16_gen')}
_X3_CNT = {'fewch_halo': 1, 'fewch_halo_signs': 0, 'dgrad_s2_o16': 0, 'dgrad_s2_mb': 0, 'halo_s2_k64': 0, 'persist_dgrad': 0}
_case('front_ragged-x3', front(), RAGGED, _X3, _X3_CNT, precision='bf16x3', ref='front_ragged')
_case('front_fit-x3', front(acts=(0.5, 0.25, None)), (4, 11, 19, 35, 2), _X3, _X3_CNT, precision='bf16x3', ref='front_fit')
_case('front_same_even-x3', front('same'), (2, 24, 20, 44, 2), {**_X3, **{2: _k('gconv', 'mfma_frame', 'bf16_gen')}}, _X3_CNT,
      precision='bf16x3', ref='front_same_even')
_case('back_short-x3', back_short(), (2, 13, 21, 37, 2),
      {0: _k('gconv_fewch', 'gconv', 'c2'), 1: _k('gconv', 'gconv', 'bf16_gen'), 2: _k('mfma_tile', 'mfma_chunked', 'bf16_gen')},
      {'halo_s2_k64': 0}, d_lim=2, precision='bf16x3', ref='back_short')


# ------------------------------------------------------------------ building
def shape_of(case, cu=NOMINAL_CU):
    return tuple(case['shape'](cu)) if callable(case['shape']) else tuple(case['shape'])


def out_shape(spec, shape):
    """output shape of a stack of k = 3 convs"""
    sp = list(shape[1:4])
    c = shape[-1]
    for s in spec:
        if s['class'] != 'Conv3D':
            continue
        st = s['strides']
        sp = [-(-n // st) if s['padding'] == 'same' else R.conv_out(n, 3, st) for n in sp]
        c = s['filters']
    assert min(sp) >= 1, sp
    return (shape[0],) + tuple(sp) + (c,)


def _is_int(a, lim):
    return bool(np.all(a == np.round(a)) and np.abs(a).max() <= lim)


@functools.lru_cache(maxsize=None)
def _build(ref_name, shape):
    """data + reference of the case ``ref_name`` at ``shape``, conditions asserted"""
    case = CASES[ref_name]
    spec = case['spec']
    rng = np.random.default_rng(zlib.crc32(ref_name.encode()))
    w = _weights(spec, shape[-1], rng, 3)
    x = _data(shape, rng)
    net = R.RefNet(_clean(spec), 3)
    d_out = _data(out_shape(spec, shape), rng, -case['d_lim'], case['d_lim'])
    ref = _reference(spec, 3, w, x, d_out, net=net)
    # ---- the conditions, on the reference
    assert _is_int(x, 3) and _is_int(d_out, 4), f'{ref_name}: data'
    for i, a in enumerate(w):
        if a.ndim == 1:
            assert _is_int(a, 2), f'{ref_name}: bias #{i}'
        else:
            flat = a.reshape(-1, a.shape[-1])
            assert (np.abs(flat).sum(axis=0) == 1).all() and set(np.unique(flat)) <= {-1.0, 0.0, 1.0}, \
                f'{ref_name}: filter #{i} is not one +-1 per output channel'
    convs = [rec for rec in net._tape if rec[0] == 'conv']
    acts = [rec for rec in net._tape if rec[0] == 'act']
    for i, rec in enumerate(convs):
        assert _bf16_exact(rec[4]), f'{ref_name}: the input of conv {i} does not survive bf16'
    for i, rec in enumerate(acts):
        assert rec[2] in (0.0, 0.25, 0.5), f'{ref_name}: slope {rec[2]}'
        assert _bf16_exact(rec[1]), f'{ref_name}: activation {i} does not survive bf16'
    for i, d in enumerate(net.dpre):
        assert _bf16_exact(d), f'{ref_name}: dPre of conv {i} does not survive bf16 (max |dPre| {np.abs(d).max()})'
    # (the output, dx and the gradients are fp32 tensors of the plan)
    # shared among the legs of a case: the reference stays as it is
    for a in ref[:2] + tuple(ref[2]):
        a.setflags(write=False)
    return dict(w=w, x=x, d_out=d_out, ref=ref)


def build(name, cu=NOMINAL_CU):
    """-> (case, shape, data + reference shared with the case it is a leg of)"""
    case = CASES[name]
    base = CASES[case['ref']]
    assert _clean(base['spec']) == _clean(case['spec']) and base['d_lim'] == case['d_lim']
    shape = shape_of(case, cu)
    assert shape == shape_of(base, cu)
    return case, shape, _build(case['ref'], shape)
