"""The cases of tests/test_tail_exact_gpu.py (TEST INFRASTRUCTURE): the
generator's expansion conv + depth-to-space + hi-res tail conv (Conv3D 8 ->
C_out <= 4 behind a REFLECT pad), their integer data, the float64 reference
(tests/support_ref.py) and the proof that the comparison may be
``assert_array_equal``.

No device is touched here: tests/test_tail_exact_ref_cpu.py builds every case in
the CPU suite, so that no case reaches a GPU with an unmet condition.

Data (``_build``):
  * x integers in [-3, 3], biases integers in [-2, 2], the filters in front of
    the tail conv one +-1 per output channel (``inj``), LeakyReLU 0.25: the cells
    the tail conv reads are multiples of 0.25 with |x| <= 5;
  * the tail filter is DENSE: every one of its 27 x 8 x C_out entries is +-1, so
    every (tap, input channel) slot moves every output;
  * d_out is sparse on a lattice (``lattice_d_out``): per sample and output
    channel its non-zero entries (+-1, +-2) sit on nested index sets whose
    members are at least 3 apart, so two of them never meet in one cell of
    the data-gradient frame — a cell receives at most one term per output
    channel and dPre of the expansion conv stays within 8 bits.
Conditions, asserted by ``_build`` on the reference with the tensor named:
  * each conv's input, each activation and each dPre survive bf16;
  * every bias / weight-gradient sum stays below 2^24 units (``_reference``,
    for two accumulated backward passes);
  * every entry of the tail conv's weight gradient is non-zero, and every (tap,
    input channel) slot of its data-gradient frame is non-zero at some lattice
    point;
  * the lattice reaches every residue (mod 3 per axis) that the shape has at
    interior positions and on each of the six reflect borders.
A split-bf16 (BF16X3) plan of the same case has a zero low part everywhere: the
same reference holds bit for bit.
"""
import functools
import itertools
import zlib

import numpy as np

from tests import support_ref as R
from tests.test_train_support_gpu import _bf16_exact, _clean, _conv, _data, _leaky, _pad, _reference, _weights

NOMINAL_CU = 256      # CU count the CPU suite builds the CU-dependent shapes for
TAIL_FLOOR = 65536    # positions from which the tail weight gradient (hence bf16 cells) is chosen

FWD_COUNTERS = ('tail_tile', 'tail_band', 'tail_slide', 'tail_sweep', 'tail_x3')
WGRAD_COUNTERS = ('wgrad_tail_tile', 'wgrad_tail_tile_in16', 'wgrad_tail_sweep')
COUNTERS = FWD_COUNTERS + WGRAD_COUNTERS


# --------------------------------------------------------------------- stacks
def stack(b, cout, pad0=(1, 1, 1)):
    """pad, Conv3D 64 -> b^2 8 (inj), depth-to-space b, LeakyReLU 0.25, pad REFLECT, Conv3D 8 -> cout (dense)"""
    return [_pad(3, list(pad0)), _conv(3, b * b * 8, 3, _w='inj'),
            {'class': 'SpatioTemporalExpansion', 'spatial_mult': b}, _leaky(), _pad(3, [1, 1, 1]),
            _conv(3, cout, 3, _w='dense')]


def stack4(cout):
    """pad, Conv3D 4 -> 8 (inj), LeakyReLU 0.25, pad REFLECT, Conv3D 8 -> cout (dense): no depth-to-space"""
    return [_pad(3, [1, 1, 1]), _conv(3, 8, 3, _w='inj'), _leaky(), _pad(3, [1, 1, 1]), _conv(3, cout, 3, _w='dense')]


def _n_min(hi, floor=TAIL_FLOOR):
    """smallest batch with >= floor hi-res positions"""
    return -(-floor // int(np.prod(hi)))


def _tiles(o, tile):
    return int(np.prod([-(-a // b) for a, b in zip(o, tile)]))


def _n_for_units(per_sample, cu):
    """smallest batch with more units than ``cu`` and a unit count that is no multiple of 8"""
    n = cu // per_sample + 1
    while (n * per_sample) % 8 == 0:
        n += 1
    return n


# -------------------------------------- the launchers' rules, restated (kernels_conv_tail_*.hip,
# kernels_conv_wgrad_fewch.hip): which forced plane shapes they accept
_SW_S1 = (4, 5, 6, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64, 80, 96)
_SW_S2 = (16, 24, 32, 40, 48, 56, 64, 72, 80, 96, 112, 128, 144, 160, 192, 256, 288)
_SEGS = (4, 6, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64, 80, 96, 128)
_WS_S1 = (4, 5, 6, 8, 10, 12, 16, 20, 24, 32, 40, 48)
_WS_S2 = (32, 64, 96, 128, 160, 192)


def forced(s1, s2, seg):
    return s1 * 1000000 + s2 * 1000 + seg


def _unforce(v):
    return v // 1000000, v // 1000 % 1000, v % 1000


def sweep_nset(v):
    """NSET of conv_tail_sweep_kernel for the forced shape ``v`` (0: the launcher refuses it)"""
    s1, s2, seg = _unforce(v)
    if s1 not in _SW_S1 or s2 not in _SW_S2 or seg not in _SEGS:
        return 0
    groups = s1 * (s2 // 8)
    npieces = ((s1 + 2) * (s2 + 2) + 2 + 63) // 64
    if groups > 8 * 16 * 3 or npieces > 7 * 8 or 3 * npieces * 1024 > 160 * 1024:
        return 0
    return -(-groups // 128)


def wsweep_ok(v):
    """does conv_wgrad_tail_sweep_kernel take the forced shape ``v``?"""
    s1, s2, seg = _unforce(v)
    if s1 not in _WS_S1 or s2 not in _WS_S2 or seg not in _SEGS or s1 * s2 > 2 * 512 * 3:
        return False
    npieces = ((s1 + 2) * (s2 + 2) + 2 + 63) // 64
    slot = npieces * 1024 + ((s1 * s2 // 2 + 63) // 64) * 1024
    return npieces <= 7 * 8 and 3 * slot + 4 * (s1 * s2 * 4) + 64 <= 160 * 1024


def tail_counters(cout, hi, options, precision, in16, wgrad, training=True, backwards=1):
    """the launch counters of the tail conv: launch_conv_tail_mfma / _sweep / _x3 and
    launch_conv_wgrad_tail restated.  ``in16`` / ``wgrad``: what the plan reports.

    The restatement is NARROWER than the code, enough for the shapes of this file: it takes
    conv_tail_sweep_supported() for granted where the banded form may slide (true while D[1] * D[2] * 8
    fits 32 bits) and takes it that an unforced wsweep_shape() finds a shape (4 x 32 planes always fit).
    A new case that lands on the slide or tile kernel against this rule has met one of these two, not a
    kernel regression: extend the rule."""
    opt = options or {}
    want = dict.fromkeys(COUNTERS, 0)
    v = opt.get('TAIL_SWEEP_SHAPE', 0)
    if precision == 'bf16x3':
        if cout == 2 and hi[2] >= 16 and not opt.get('NO_TAIL_X3'):
            want['tail_x3'] = 1
    elif in16 and hi[2] >= 16:
        band = cout == 2 and not opt.get('NO_TAIL_BAND')
        slide = band and hi[0] >= 4 and not opt.get('NO_TAIL_SLIDE')
        if slide and not opt.get('NO_TAIL_SWEEP'):
            assert not v or sweep_nset(v), 'the forward launcher would refuse the forced shape'
            want['tail_sweep'] = 1
        elif slide:
            want['tail_slide'] = 1
        else:
            want['tail_band' if band else 'tail_tile'] = 1
    if training and wgrad == 'tail':
        sweep = (in16 and cout == 2 and not opt.get('NO_WGRAD_TAIL_SWEEP') and hi[2] % 2 == 0 and hi[0] >= 4 and
                 hi[2] >= 32 and (not v or wsweep_ok(v)))
        want['wgrad_tail_sweep' if sweep else ('wgrad_tail_tile_in16' if in16 else 'wgrad_tail_tile')] = backwards
    return want


# ---------------------------------------------------------------------- cases
CASES = {}

# the data gradient of the tail conv where the few-channel frame kernel (C_out 2 or 4, select_conv in
# plan.cpp) does not take it: 8 -> 3 has no MFMA adjoint, the direct family runs
DGRAD_NOT_FEWCH = 'direct'


def expansion_info(b, out16):
    """what a bf16 / split-bf16 training plan gives the 64 -> b^2 8 'same' expansion conv: the halo-tile
    kernel forward, the trunk weight gradient, and as data gradient the halo tile over the padded frame up
    to 64 output channels (b = 2), else 64-channel passes of it (conv_dgrad_chunked_supported).  Its input
    is the plan's input: fp32"""
    return dict(fwd='mfma_tile', dgrad='mfma_chunked' if b * b * 8 > 64 else 'mfma_frame', wgrad='bf16_trunk', in16=0,
                out16=out16)


def _case(name, b, cout, hi, n=None, options=None, precision='bf16', training=True, backwards=1, ref=None, note='',
          spec=None, cin=64, exp=None, tail=None):
    """``hi``: hi-res extents (O0, O1, t); ``n``: batch (None: the smallest with TAIL_FLOOR positions;
    callable: CU count -> batch).  ``exp`` / ``tail``: corrections to the expected op_info of the two convs"""
    assert name not in CASES
    assert hi[0] % b == 0 and hi[1] % b == 0, (name, hi, b)
    CASES[name] = dict(name=name, b=b, cout=cout, hi=tuple(hi), n=n, options=dict(options or {}), precision=precision,
                       training=training, backwards=backwards, ref=ref or name, note=note,
                       spec=spec or stack(b, cout), cin=cin, exp=exp or {}, tail=tail or {})


def batch_of(case, cu=NOMINAL_CU):
    n = case['n']
    return _n_min(case['hi']) if n is None else (int(n(cu)) if callable(n) else int(n))


def shape_of(case, cu=NOMINAL_CU):
    """the plan's input shape"""
    hi, b = case['hi'], case['b']
    first = case['spec'][0]['paddings']
    lo = [hi[0] // b, hi[1] // b, hi[2]]
    # (a first pad narrower than the filter's reach: the conv is 'valid' along that axis)
    lo = [v + 2 - sum(first[1 + a]) for a, v in enumerate(lo)]
    return (batch_of(case, cu),) + tuple(lo) + (case['cin'],)


def positions(case, cu=NOMINAL_CU):
    return batch_of(case, cu) * int(np.prod(case['hi']))


def expected(case, cu=NOMINAL_CU):
    """-> ({conv index: op_info fields}, {counter: launches}) the case asserts"""
    cout, hi, opt, prec = case['cout'], case['hi'], case['options'], case['precision']
    pos = positions(case, cu)
    if prec == 'bf16x3':
        x3 = cout == 2 and hi[2] >= 16 and not opt.get('NO_TAIL_X3')
        tail = dict(fwd='tail_mfma' if x3 else ('small' if cout == 2 else 'direct'), in16=0, out16=0)
        if case['training']:
            tail['wgrad'] = 'c2'
    elif case['training']:
        in16 = int(pos >= TAIL_FLOOR and hi[2] >= 16)
        tail = dict(fwd='tail_mfma' if in16 else ('small' if cout == 2 else 'direct'), in16=in16, out16=0,
                    wgrad='tail' if pos >= TAIL_FLOOR else 'c2')
    else:
        # an inference plan hands the tail conv bf16 cells at any batch
        tail = dict(fwd='tail_mfma', in16=1, out16=0)
    if case['training']:
        tail['dgrad'] = 'fewch_frame' if cout in (2, 4) and not opt.get('NO_DGRAD_FEWCH') else DGRAD_NOT_FEWCH
    tail.update(case['tail'])
    exp = expansion_info(case['b'], tail['in16'])
    if not case['training']:
        exp = {k: v for k, v in exp.items() if k not in ('dgrad', 'wgrad')}
    exp.update(case['exp'])
    counters = tail_counters(cout, hi, opt, prec, tail['in16'], tail.get('wgrad'), case['training'], case['backwards'])
    return {0: exp, 1: tail}, counters


# ---- the forward tile kernel, 4 x 8 x 64 (conv_tail_mfma_kernel<false> / <true>) and the weight-gradient
# tile kernel, 4 x 8 x 32 (conv_wgrad_tail_kernel<true>): one past / exactly on / one below a multiple of
# the tile in every axis.  Hi-res s0 / s1 extents are multiples of b: 9 = 2 * 4 + 1 = 8 + 1 and
# 15 = 4 * 4 - 1 = 2 * 8 - 1 need b = 3, 4 and 8 b = 2; lo-res extents are >= 2 (reflect pad 1), so
# s0 = 3 or 5 cannot be had
NOSLIDE = {'NO_TAIL_SLIDE': 1}
for _tag, _b, _hi in (('ragged', 3, (9, 9, 65)), ('exact', 2, (4, 8, 64)), ('below', 3, (15, 15, 63))):
    # C_out = 2: the banded form, <false> at two channels, and the split-bf16 kernel (4 x 8 x 32)
    _case(f'tile_{_tag}_c2', _b, 2, _hi, options=NOSLIDE)
    _case(f'tile_{_tag}_c2-noband', _b, 2, _hi, options=dict(NOSLIDE, NO_TAIL_BAND=1), ref=f'tile_{_tag}_c2')
    _case(f'tile_{_tag}_c2-x3', _b, 2, _hi, precision='bf16x3', ref=f'tile_{_tag}_c2')
    # C_out = 3, 4: <false>, no option
    _case(f'tile_{_tag}_c3', _b, 3, _hi)
    _case(f'tile_{_tag}_c4', _b, 4, _hi)
_case('tile_ragged_c2-x3-NO_TAIL_X3', 3, 2, (9, 9, 65), options={'NO_TAIL_X3': 1}, precision='bf16x3', ref='tile_ragged_c2')
_case('tile_ragged_c2-NO_DGRAD_FEWCH', 3, 2, (9, 9, 65), options=dict(NOSLIDE, NO_DGRAD_FEWCH=1), ref='tile_ragged_c2')
_case('tile_exact_c4-NO_DGRAD_FEWCH', 2, 4, (4, 8, 64), options={'NO_DGRAD_FEWCH': 1}, ref='tile_exact_c4')
# the second backward pass accumulates: the reduce of conv_wgrad_tail_kernel<true>
_case('tile_ragged_c3-acc', 3, 3, (9, 9, 65), backwards=2, ref='tile_ragged_c3')

# the floor of 16 time steps (conv_tail_mfma_supported) and of 65 536 positions (conv_wgrad_tail_supported):
# 8 x 16 x 16 x 32 samples = 65 536 exactly; 31 samples = 63 488: wgrad_c2, fp32 cells, the direct family forward
_case('floor_t16', 2, 2, (8, 16, 16), options=NOSLIDE)
_case('floor_t15', 2, 2, (8, 16, 15), options=NOSLIDE, note='t = 15: off tail_mfma, fp32 cells')
_case('floor_pos_below', 2, 2, (8, 16, 16), n=31, options=NOSLIDE, note='63 488 positions: wgrad c2')


# many tiles: 10 x 18 x 16 is 3 x 3 x 1 = 9 forward tiles (and 9 weight-gradient tiles) per sample
def _many(cu):
    return max(_n_for_units(9, cu), _n_min((10, 18, 16)))


def _many2(cu):
    return max(_n_for_units(9, 2 * cu), _n_min((10, 18, 16)))


_case('many_tiles_c2', 2, 2, (10, 18, 16), n=_many, options=NOSLIDE)
_case('many_tiles_c2-noband', 2, 2, (10, 18, 16), n=_many, options=dict(NOSLIDE, NO_TAIL_BAND=1), ref='many_tiles_c2')
# ... and more weight-gradient tiles than its 2 x CU workgroups
_case('many_tiles_c3', 2, 3, (10, 18, 16), n=_many2)

# ---- the slide kernel (NO_TAIL_SWEEP): column 16 x 64 along s0.  33 = 2 * 16 + 1 (b = 3), 16 (b = 2), 15 (b = 3)
NOSWEEP = {'NO_TAIL_SWEEP': 1}
_case('slide_ragged', 3, 2, (6, 33, 65), options=NOSWEEP)
_case('slide_exact', 2, 2, (4, 16, 64), options=NOSWEEP, note='O[0] = 4: the floor of the slide kernel')
_case('slide_below', 3, 2, (6, 15, 63), options=NOSWEEP)
# O[0] = 3 < 4: the banded tile kernel.  Lo-res extents are >= 2 (reflect pad 1) and hi-res ones multiples
# of b, so O[0] = 3 needs an expansion conv that is 'valid' along s0 (no first pad there).  A training plan
# runs that conv on the direct family, which writes fp32: the tail conv gets fp32 cells and falls to the
# direct family itself, its weight gradient to conv_wgrad_tail_kernel<false>.  The inference plan of the
# same stack (infer_o0_3 below) has bf16 cells.
_O3 = dict(spec=stack(3, 2, pad0=(0, 1, 1)), exp=dict(fwd='direct', dgrad='gconv', wgrad='bf16_gen', out16=0))
_case('slide_o0_3', 3, 2, (3, 15, 64), options=NOSWEEP, tail=dict(in16=0, fwd='small'), **_O3)
# the launcher picks 8 rows per segment (one round of workgroups: the cost is rows + 5): 12 = 8 + 4
_case('slide_seg_ragged', 2, 2, (12, 16, 64), options=NOSWEEP)


# 4 x 34 x 16: 1 x 3 x 1 = 3 columns per sample; more columns than CUs
def _slide_many(cu):
    return max(_n_for_units(3, cu), _n_min((4, 34, 16)))


_case('slide_many_units', 2, 2, (4, 34, 16), n=_slide_many, options=NOSWEEP)

# ---- the sweep kernels (forward: default for C_out = 2; weight gradient: even t >= 32), TAIL_SWEEP_SHAPE
# = S1, S2, rows per unit.  nset = ceil(S1 * S2 / 8 / 128)
_F1, _F2, _F3, _FW = forced(4, 16, 4), forced(16, 96, 4), forced(40, 72, 4), forced(4, 32, 4)
# what the cost model picks, forward and weight gradient (the data of slide_exact)
_case('sweep_default', 2, 2, (4, 16, 64), ref='slide_exact')
_case('sweep_default-acc', 2, 2, (4, 16, 64), backwards=2, ref='slide_exact')
_case('sweep_default-NO_WGRAD_TAIL_SWEEP', 2, 2, (4, 16, 64), options={'NO_WGRAD_TAIL_SWEEP': 1}, ref='slide_exact')
_case('sweep_default-NO_DGRAD_FEWCH', 2, 2, (4, 16, 64), options={'NO_DGRAD_FEWCH': 1}, ref='slide_exact')
_case('sweep_default_ragged', 3, 2, (6, 33, 65), ref='slide_ragged')
# nset = 1: 4 x 16 planes.  9 = 2 * 4 + 1, 17 = 16 + 1, rows 4 + 2 | 8, 16, rows = O[0] | 15 = 4 * 4 - 1, 31 = 2 * 16 - 1
_case('sweep_n1_ragged', 3, 2, (6, 9, 17), options={'TAIL_SWEEP_SHAPE': _F1})
_case('sweep_n1_exact', 2, 2, (4, 8, 16), options={'TAIL_SWEEP_SHAPE': _F1})
_case('sweep_n1_below', 3, 2, (6, 15, 31), options={'TAIL_SWEEP_SHAPE': _F1})
# nset = 2: 16 x 96 planes (also a shape of the weight-gradient sweep: even t)
_case('sweep_n2_ragged', 3, 2, (6, 33, 97), options={'TAIL_SWEEP_SHAPE': _F2})
_case('sweep_n2_exact', 2, 2, (4, 16, 96), options={'TAIL_SWEEP_SHAPE': _F2})
# S2 = 96 > O[2] = 90, within the + 7 the unforced search allows
_case('sweep_n2_s2_past_t', 2, 2, (4, 16, 90), options={'TAIL_SWEEP_SHAPE': _F2})
# nset = 3: 40 x 72 planes (72 is no plane width of the weight-gradient sweep: its tile kernel runs)
_case('sweep_n3_ragged', 3, 2, (6, 42, 73), options={'TAIL_SWEEP_SHAPE': _F3})
_case('sweep_n3_exact', 2, 2, (4, 40, 72), options={'TAIL_SWEEP_SHAPE': _F3})
_case('sweep_n3_below', 3, 2, (6, 39, 71), options={'TAIL_SWEEP_SHAPE': _F3})
# more units than CUs: 9 x 1 planes of 4 x 16 per sample (the data of slide_many_units)
_case('sweep_many_units', 2, 2, (4, 34, 16), n=_slide_many, options={'TAIL_SWEEP_SHAPE': _F1}, ref='slide_many_units')
# the weight-gradient sweep on 4 x 32 planes: exact (the data of slide_exact) and ragged (33 = 8 * 4 + 1, 34 = 32 + 2, rows 4 + 2)
_case('wsweep_4x32_exact', 2, 2, (4, 16, 64), options={'TAIL_SWEEP_SHAPE': _FW}, ref='slide_exact')
_case('wsweep_4x32_ragged', 3, 2, (6, 33, 34), options={'TAIL_SWEEP_SHAPE': _FW})

# ---- b = 5: C_out = 200 = 3 x 64 + 8 in the expansion conv, the depth-to-space store of its 8-channel last tile
_case('b5_c200', 5, 2, (10, 15, 64))

# ---- fp32 cells into the tail weight gradient: conv_wgrad_tail_kernel<false>.  Behind a 4 -> 8 conv the
# plan keeps bf16 cells (the few-channel gather conv writes bf16 towards a conv input: cin4_c2); NO_DISC_BF16
# switches that off
_X4 = dict(fwd='gconv_fewch', dgrad='direct', wgrad='f32_gen', in16=0)
for _c in (2, 3):
    _case(f'fp32_cells_c{_c}', 1, _c, (9, 9, 65), spec=stack4(_c), cin=4, options={'NO_DISC_BF16': 1},
          tail=dict(in16=0, fwd='small' if _c == 2 else 'direct'), exp=dict(_X4, out16=0))
_case('fp32_cells_c2-acc', 1, 2, (9, 9, 65), spec=stack4(2), cin=4, options={'NO_DISC_BF16': 1}, backwards=2,
      tail=dict(in16=0, fwd='small'), exp=dict(_X4, out16=0), ref='fp32_cells_c2')
_case('cin4_c2', 1, 2, (9, 9, 65), spec=stack4(2), cin=4, exp=dict(_X4, out16=1), ref='fp32_cells_c2')

# ---- inference plans, forward only, one per forward variant, against the y of the training case
_case('infer_tile_c3', 3, 3, (9, 9, 65), training=False, ref='tile_ragged_c3')
_case('infer_band', 3, 2, (9, 9, 65), training=False, options=NOSLIDE, ref='tile_ragged_c2')
_case('infer_noband', 3, 2, (9, 9, 65), training=False, options=dict(NOSLIDE, NO_TAIL_BAND=1), ref='tile_ragged_c2')
_case('infer_slide', 3, 2, (6, 33, 65), training=False, options=NOSWEEP, ref='slide_ragged')
_case('infer_sweep', 3, 2, (6, 33, 65), training=False, ref='slide_ragged')
_case('infer_x3', 3, 2, (9, 9, 65), training=False, precision='bf16x3', ref='tile_ragged_c2')
# O[0] = 3: below the slide kernel's (and the sweep's) four rows, the banded tile kernel
_case('infer_o0_3', 3, 2, (3, 15, 64), training=False, options=NOSWEEP, ref='slide_o0_3',
      spec=_O3['spec'], exp=dict(fwd='direct', out16=1))
# fewer tiles than the 8 XCDs: a training plan has bf16 cells from 65 536 positions (32 tiles) on, an
# inference plan at any size: 4 samples of one 4 x 8 x 64 tile
_case('infer_few_tiles_c3', 2, 3, (4, 8, 64), n=4, training=False)
_case('infer_few_tiles_band', 2, 2, (4, 8, 64), n=4, training=False, options=NOSLIDE)


# ------------------------------------------------------------------ the data
def _axis_set(d, mode, rng):
    """indices of an axis of extent ``d``, at least 3 apart: from 0 on (mode 0), down from d - 1 (mode 1),
    from 1 or 2 on (mode 2), with gaps of 3 ... 5 so that every residue mod 3 occurs along the axis"""
    gaps = rng.integers(3, 6, size=d // 3 + 2)
    pos = np.cumsum(np.concatenate(([0 if mode != 2 else int(rng.integers(1, 3))], gaps)))
    pos = pos[pos < d]
    return (d - 1 - pos)[::-1] if mode == 1 else pos


def lattice_d_out(shape, rng):
    """(N, O0, O1, O2, C): per sample and channel, +-1 / +-2 on nested ``_axis_set``s — time steps t of one
    set, per t its own set of rows i, per (t, i) its own set of columns j — zero elsewhere.  Two non-zero
    entries of one (sample, channel) differ by >= 3 along t, or else along s0, or else along s1.  (The
    time sets take their three modes in turn, so that both t borders are reached at any batch >= 2.)"""
    d = np.zeros(shape, np.float32)
    for n in range(shape[0]):
        for c in range(shape[4]):
            for t in _axis_set(shape[3], (n * shape[4] + c) % 3, rng):
                for i in _axis_set(shape[1], int(rng.integers(3)), rng):
                    js = _axis_set(shape[2], int(rng.integers(3)), rng)
                    d[n, i, js, t, c] = rng.choice([-2.0, -1.0, 1.0, 2.0], size=len(js))
    return d


def lattice_gaps(d):
    """missing residues of the lattice: (interior, {(axis, side): on that border})"""
    o = d.shape[1:4]
    idx = np.argwhere(np.abs(d).sum(axis=(0, 4)) > 0)
    inner = np.all((idx > 0) & (idx < np.array(o) - 1), axis=1)
    have = {tuple(r) for r in idx[inner] % 3}
    need = set(itertools.product(*[sorted({i % 3 for i in range(1, n - 1)}) for n in o]))
    faces = {}
    for a in range(3):
        rest = [q for q in range(3) if q != a]
        need_f = set(itertools.product(*[sorted({i % 3 for i in range(o[q])}) for q in rest]))
        for side, at in (('lo', 0), ('hi', o[a] - 1)):
            on = idx[idx[:, a] == at]
            faces[(a, side)] = need_f - {tuple(r) for r in on[:, rest] % 3}
    return need - have, faces


def _lattice(shape, rng, name, cells):
    """a lattice that reaches every residue on every border and leaves no entry of the tail conv's
    weight gradient at zero (a sum of ~1 000 signed terms is zero once in ~1 000): one that does not
    is drawn again — the data changes, no assertion does"""
    for attempt in range(64):
        d = lattice_d_out(shape, rng)
        inner, faces = lattice_gaps(d)
        if inner or any(faces.values()):
            continue
        if np.all(R.conv_adj_w(cells, d.astype(np.float64), (3, 3, 3)) != 0):
            return d, attempt
    raise AssertionError(f'{name}: no lattice with every residue on every border and no zero in dw: {inner} {faces}')


@functools.lru_cache(maxsize=None)
def _build(ref_name, shape):
    """data + reference of the case ``ref_name`` at the input shape ``shape``, conditions asserted"""
    case = CASES[ref_name]
    spec, cout = case['spec'], case['cout']
    rng = np.random.default_rng(zlib.crc32(ref_name.encode()))
    w = _weights(spec, shape[-1], rng, 3)
    x = _data(shape, rng)
    net = R.RefNet(_clean(spec), 3)
    net.set_weights(w)
    y = net.forward(x)
    if not case['training']:
        # a forward-only base (no training plan reaches its shape): no d_out, no gradients
        cells = net._tape[-1][4]
        assert _bf16_exact(net._tape[1][4]) and _bf16_exact(cells), f'{ref_name}: a conv input does not survive bf16'
        assert np.all(cells * 4 == np.round(cells * 4)) and np.abs(cells).max() <= 5, f'{ref_name}: the tail conv\'s cells'
        assert set(np.unique(w[-2])) == {-1.0, 1.0}, f'{ref_name}: the tail filter is not dense'
        y.setflags(write=False)
        return dict(w=w, x=x, d_out=None, ref=(y, None, None), redrawn=0)
    d_out, redrawn = _lattice((shape[0],) + case['hi'] + (cout,), rng, ref_name, net._tape[-1][4])
    ref = _reference(spec, 3, w, x, d_out, backwards=2, net=net)
    # ---- the conditions, on the reference
    assert np.all(x == np.round(x)) and np.abs(x).max() <= 3, f'{ref_name}: x'
    assert np.all(d_out == np.round(d_out)) and np.abs(d_out).max() <= 2, f'{ref_name}: d_out'
    assert set(np.unique(w[-2])) == {-1.0, 1.0} and w[-2].shape == (3, 3, 3, 8, cout), f'{ref_name}: the tail filter is not dense'
    for i, a in enumerate(w[:-2]):
        if a.ndim == 1:
            assert np.all(a == np.round(a)) and np.abs(a).max() <= 2, f'{ref_name}: bias #{i}'
        else:
            flat = a.reshape(-1, a.shape[-1])
            assert (np.abs(flat).sum(axis=0) == 1).all(), f'{ref_name}: filter #{i} is not one +-1 per output channel'
    convs = [rec for rec in net._tape if rec[0] == 'conv']
    acts = [rec for rec in net._tape if rec[0] == 'act']
    for i, rec in enumerate(convs):
        assert _bf16_exact(rec[4]), f'{ref_name}: the input of conv {i} does not survive bf16'
    for i, rec in enumerate(acts):
        assert rec[2] == 0.25 and _bf16_exact(rec[1]), f'{ref_name}: activation {i} does not survive bf16'
    cells = convs[-1][4]
    assert np.all(cells * 4 == np.round(cells * 4)) and np.abs(cells).max() <= 5, f'{ref_name}: the tail conv\'s cells'
    for i, dp in enumerate(net.dpre):
        assert _bf16_exact(dp), f'{ref_name}: dPre of conv {i} does not survive bf16 (max |dPre| {np.abs(dp).max()})'
    # ---- every slot is visible: the weight gradient of the tail filter, and per (tap, input channel)
    # the data-gradient frame at the cells that tap reaches from a lattice point
    dw = ref[2][-2]
    assert dw.shape == w[-2].shape and np.all(dw != 0), f'{ref_name}: {int((dw == 0).sum())} zero entries in dw of the tail conv'
    frame = R.conv_adj_x(net.dpre[-1], np.asarray(w[-2], np.float64), cells.shape)
    lit = np.abs(d_out).sum(axis=4) > 0
    o = case['hi']
    for a, b, c in itertools.product(range(3), repeat=3):
        seen = np.abs(frame[:, a:a + o[0], b:b + o[1], c:c + o[2]][lit]).max(axis=0)
        assert np.all(seen > 0), f'{ref_name}: dx of the tail conv never shows tap {(a, b, c)}, channels {np.flatnonzero(seen == 0)}'
    # shared among the legs of a case: the reference stays as it is
    for a in ref[:2] + tuple(ref[2]):
        a.setflags(write=False)
    return dict(w=w, x=x, d_out=d_out, ref=ref, redrawn=redrawn)


def build(name, cu=NOMINAL_CU):
    """-> (case, input shape, data + reference shared with the case it is a leg of)"""
    case = CASES[name]
    base = CASES[case['ref']]
    assert _clean(base['spec']) == _clean(case['spec']) and base['hi'] == case['hi']
    shape = shape_of(case, cu)
    assert shape == shape_of(base, cu), (name, shape, shape_of(base, cu))
    return case, shape, _build(case['ref'], shape)
