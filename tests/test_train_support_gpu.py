"""The training step's support kernels (sup3r_amd/csrc/kernels_fold.hip,
kernels_pointwise.hip, kernels_reduce.hip, kernels_optim.hip, kernels_loss_content.hip) at the
edges of their variants, each against the float64 restatement of the same
operation (tests/support_ref.py, pinned on the CPU by
tests/test_support_ref_cpu.py).

Plan-level cases make every value a small integer times a power of two
(inputs in [-3, 3], d_out in [-4, 4], one-hot +-1 filters, LeakyReLU slope
0.25): every sum stays below 2^24 in units of its granularity, the result does
not depend on the summation order and the comparison is ``assert_array_equal``.
Each case asserts the launch counter (``_lib.STATS``) of the variant it is
named for and that the siblings' counters stayed put; grid-cap shapes come
from the device's CU count.

Few positions (P <= 8192) would send a conv to the one-launch fewpos kernels,
which leave the bias gradient and apply the activation adjoint themselves and
never reach ``launch_bias_grad`` / ``launch_conv_epilogue_bwd``: the small
cases A / B switch that family off (option NO_FEWPOS_MFMA) — their subject is
the support pass, not the conv.  See profiles/support/NOTES.md."""
import ctypes as C
import zlib

import numpy as np
import pytest

from tests import support_ref as R

pytestmark = pytest.mark.gpu

BIAS = ('bias_stage1', 'bias_stage1_v4', 'bias_cols', 'bias_cols_split')
PARTIAL = ('bias_partial', 'bias_partial_ride', 'bias_partial_flush')
EPI = ('epi_generic', 'epi_c4', 'epi_d2s4')
EPI_SUMS = ('epi_c4_bsum', 'epi_d2s4_bsum')
FOLD = ('fold_gather', 'fold_pad4', 'fold_pad4_fr16', 'fold16x8')
FOLD_MODE = ('fold_plain', 'fold_masked', 'fold_add')
AXPY = ('axpy', 'axpy4')
SUPPORT = BIAS + PARTIAL + EPI + EPI_SUMS + FOLD + FOLD_MODE + AXPY
SMALL = {'NO_FEWPOS_MFMA': 1}


def _cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _pos2d(target):
    """(a, b) with a * b >= target and as little above it as a near-square
    grid allows: 'just above' a block cap, ragged against every tile"""
    a = int(np.ceil(np.sqrt(target)))
    a += 1 - a % 2                       # odd
    return a, int(-(-target // a))


def _conv(nd, filters, k=1, **kw):
    return dict({'class': f'Conv{nd}D', 'filters': filters, 'kernel_size': k}, **kw)


def _pad(nd, lo, hi=None, mode='REFLECT'):
    hi = lo if hi is None else hi
    return {'class': 'FlexiblePadding', 'mode': mode,
            'paddings': [[0, 0]] + [[int(a), int(b)] for a, b in zip(lo[:nd], hi[:nd])] + [[0, 0]]}


def _leaky():
    return {'class': 'LeakyReLU', 'alpha': 0.25}


def _weights(spec, cin, rng, nd, kind='one_hot', bias=True):
    """keras-order weights: one +-1 per output channel (``one_hot``: any (tap,
    input channel); ``perm``: C_in == C_out, every input channel fed by exactly
    one (tap, output channel); ``inj``: no (tap, input channel) feeds two
    output channels), +-1 in EVERY entry (``dense``) or the identity (1 x 1
    convs), integer biases"""
    out = []
    for s in spec:
        if s['class'] not in ('Conv2D', 'Conv3D'):
            if s['class'] in ('SpatialExpansion', 'SpatioTemporalExpansion'):
                cin //= int(s.get('spatial_mult', 1)) ** 2
            if s['class'] == 'Sup3rConcat':
                cin += 1
            continue
        k = s['kernel_size']
        k = (k,) * nd if isinstance(k, int) else tuple(k)
        cout, taps = s['filters'], int(np.prod(k))
        flat = np.zeros((taps, cin, cout), np.float32)
        mode = s.get('_w', kind)
        if mode == 'identity':
            assert taps == 1 and cin == cout
            flat[0] = np.eye(cin)
        elif mode == 'inj':
            slot = rng.choice(taps * cin, size=cout, replace=False)
            flat[slot // cin, slot % cin, np.arange(cout)] = rng.choice([-1.0, 1.0], size=cout)
        elif mode == 'dense':
            flat[:] = rng.choice([-1.0, 1.0], size=flat.shape)
        else:
            src = rng.permutation(cin) if mode == 'perm' else rng.integers(cin, size=cout)
            flat[rng.integers(taps, size=cout), src, np.arange(cout)] = rng.choice([-1.0, 1.0], size=cout)
        out.append(flat.reshape(k + (cin, cout)))
        if s.get('use_bias', True):
            out.append(rng.integers(-2, 3, size=cout).astype(np.float32) if bias and mode != 'identity'
                       else np.zeros(cout, np.float32))
        cin = cout
    return out


def _clean(spec):
    return [{k: v for k, v in s.items() if not k.startswith('_')} for s in spec]


def _run(spec, shape, weights, x, d_out, precision='f32', options=None, exo=None, backwards=1, counters=None,
         need_dx=True):
    """forward + backward(need_dx) of a fresh plan -> (y, dx, grads, counter
    deltas, op infos).  ``backwards`` > 1: the later passes accumulate.
    ``counters``: the launch counters to report (default: the support passes')."""
    from sup3r_amd.engine import Network
    net = Network(_clean(spec), precision=precision)
    net.set_weights(weights)
    ph = net.plan(shape, training=True, options=options)
    dev = net.dev
    before = {k: dev.stat(k) for k in (SUPPORT + ('persist_dgrad',) if counters is None else counters)}
    exod = {k: dev.to_device(v) for k, v in (exo or {}).items()}
    y = ph.forward(dev.to_device(x), exod)
    dyd = dev.to_device(d_out)
    for k in range(backwards):
        dx = ph.backward(dyd, need_dx=need_dx, accumulate_wgrad=k > 0)
    dev.sync()
    y = y.cpu().numpy()
    dx = dx.cpu().numpy().reshape(x.shape) if need_dx else None   # (dx comes in the plan's 5-D view)
    grads = [g.copy() for g in net.grads]
    used = {k: dev.stat(k) - v for k, v in before.items()}
    info = [ph.op_info(i) for i in range(len(ph.plan.ops)) if ph.plan.ops[i]['kind'] == 1]    # (OP_CONV)
    del ph
    net.clear_plans()
    return y, dx, grads, used, info


def _gran(a):
    """largest power of two every value of ``a`` is a multiple of (down to 2^-16)"""
    for k in range(0, 17):
        if np.all(np.round(a * 2.0 ** k) == a * 2.0 ** k):
            return 2.0 ** -k
    raise AssertionError('values are not multiples of 2^-16')


def _reference(spec, nd, weights, x, d_out, exo=None, backwards=1, net=None):
    """float64 reference + the proof that fp32 sums of these terms are exact
    in any order: per conv, sum |dPre| per channel (the bias gradient) and
    max |x| times it (a bound on every weight-gradient sum), counted in units
    of the operands' granularity, stay below 2^24"""
    ref = net or R.RefNet(_clean(spec), nd)     # (net: the caller looks at its tape afterwards)
    ref.set_weights(weights)
    y = ref.forward(x, exo)
    dx = ref.backward(d_out)
    convs = [rec for rec in ref._tape if rec[0] == 'conv']
    for rec, dpre in zip(convs, ref.dpre):
        xp = rec[4]
        col = np.abs(dpre).reshape(-1, dpre.shape[-1]).sum(axis=0).max() * backwards
        assert col / _gran(dpre) < 2 ** 24, 'bias-gradient sum could round'
        assert np.abs(xp).max() * col / (_gran(dpre) * _gran(xp)) < 2 ** 24, 'weight-gradient sum could round'
    return y, dx, ref.grads


def _data(shape, rng, lo=-3, hi=3):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def _assert_used(used, expect, groups):
    """the named counters went up (``name`` or ``(name, count)``), every other
    counter of the listed sibling groups did not"""
    print('counters:', {k: v for k, v in used.items() if v})
    want = dict((e, None) if isinstance(e, str) else e for e in expect)
    for k, n in want.items():
        assert used[k] > 0 if n is None else used[k] == n, (k, n, used)
    for grp in groups:
        for k in grp:
            if k not in want:
                assert used[k] == 0, (k, used)


def _assert_exact(got, ref, what, scale=1.0):
    y, dx, grads = got
    y_ref, dx_ref, g_ref = ref
    np.testing.assert_array_equal(y, y_ref, err_msg=f'{what}: forward')
    np.testing.assert_array_equal(dx, dx_ref, err_msg=f'{what}: dx')
    assert len(grads) == len(g_ref)
    for i, (a, b) in enumerate(zip(grads, g_ref)):
        np.testing.assert_array_equal(a, scale * b, err_msg=f'{what}: gradient #{i}')


def _bias_kernel(c, n_pos):
    """the kernel launch_bias_grad picks (kernels_reduce.hip) for a 16-B aligned dPre"""
    if c > 256:
        return 'bias_cols_split' if n_pos >= 256 else 'bias_cols'
    return 'bias_stage1_v4' if c % 4 == 0 else 'bias_stage1'


# ===================================================================== A
# bias gradient: one 1 x 1 'valid' conv, no activation, C_in = 2, fp32
# (a spatial shape that depends on a grid cap is a function of the CU count,
# called inside the test: collecting the file touches no device)
def _s3(cu):
    return 4 * cu * (256 // 3)       # positions one sweep of the capped grid covers, c = 3


def _s4(cu):
    return 4 * cu * 256              # ... on the float4 kernel, c = 4


def _bias_cases():
    return [
        # id, c, spatial shape (or CU count -> shape), kernel
        ('c3_315', 3, (15, 21), 'bias_stage1'),
        ('c5_idle_lane', 5, (15, 21), 'bias_stage1'),
        ('c3_3d', 3, (5, 9, 7), 'bias_stage1'),
        ('c3_above_cap', 3, lambda cu: _pos2d(_s3(cu) + 7), 'bias_stage1'),
        ('c3_4deep_and_rest', 3, lambda cu: _pos2d(5 * _s3(cu) + 13), 'bias_stage1'),
        ('c255', 255, (15, 21), 'bias_stage1'),
        ('c256', 256, (15, 21), 'bias_stage1_v4'),
        ('c257', 257, (15, 21), 'bias_cols_split'),
        ('c4', 4, (15, 21), 'bias_stage1_v4'),
        ('c8', 8, (15, 21), 'bias_stage1_v4'),
        ('c12_idle_lanes', 12, (15, 21), 'bias_stage1_v4'),
        ('c64', 64, (15, 21), 'bias_stage1_v4'),
        ('c200_idle_lanes', 200, (15, 21), 'bias_stage1_v4'),
        ('c4_above_cap', 4, lambda cu: _pos2d(_s4(cu) + 7), 'bias_stage1_v4'),
        ('c4_2deep_and_rest', 4, lambda cu: _pos2d(3 * _s4(cu) + 11), 'bias_stage1_v4'),
        ('c257_p255', 257, (15, 17), 'bias_cols'),
        ('c257_p256', 257, (16, 16), 'bias_cols_split'),
        ('c257_p257', 257, (257, 1), 'bias_cols_split'),
        # (cols_split at two channel blocks cuts the rows into ceil(4 CU / 2) slices)
        ('c260_empty_slices', 260, lambda cu: _pos2d(-(-4 * cu // 2) * 32 + 100), 'bias_cols_split'),
    ]


def _shape_of(sp):
    return tuple(sp(_cu())) if callable(sp) else tuple(sp)


BIAS_CASES = _bias_cases()


def _bias_case(c, sp, rng):
    nd = len(sp)
    spec = [_conv(nd, c)]
    shape = (1,) + tuple(sp) + (2,)
    w = _weights(spec, 2, rng, nd)
    x = _data(shape, rng)
    d_out = _data(shape[:-1] + (c,), rng, -4, 4)
    return spec, nd, shape, w, x, d_out


@pytest.mark.parametrize('name,c,sp,kernel', BIAS_CASES, ids=[b[0] for b in BIAS_CASES])
def test_bias_gradient(name, c, sp, kernel):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    sp = _shape_of(sp)
    spec, nd, shape, w, x, d_out = _bias_case(c, sp, rng)
    assert kernel == _bias_kernel(c, int(np.prod(sp)))
    got = _run(spec, shape, w, x, d_out, options=SMALL)
    _assert_used(got[3], [(kernel, 1)], [BIAS, PARTIAL, EPI])
    _assert_exact(got[:3], _reference(spec, nd, w, x, d_out), name)


@pytest.mark.parametrize('c,sp,kernel', [(5, (15, 21), 'bias_stage1'), (12, (15, 21), 'bias_stage1_v4'),
                                         (257, (15, 17), 'bias_cols'), (257, (15, 21), 'bias_cols_split')])
def test_bias_gradient_accumulates(c, sp, kernel):
    """a second backward pass with accumulate_wgrad: db (and dw) double"""
    rng = np.random.default_rng(c)
    spec, nd, shape, w, x, d_out = _bias_case(c, sp, rng)
    got = _run(spec, shape, w, x, d_out, options=SMALL, backwards=2)
    _assert_used(got[3], [(kernel, 2)], [BIAS, PARTIAL])
    _assert_exact(got[:3], _reference(spec, nd, w, x, d_out, backwards=2), kernel, scale=2.0)


# ===================================================================== B
# mask pass and riding channel sums: one conv + activation, fp32
def _rides(cout):
    return cout % 4 == 0 and 256 % (cout // 4) == 0 and cout // 4 <= 64


def _mask_cases():
    out = [('generic_30_elements', 2, (3, 5), 1, 0.25, 'epi_generic')]
    for cout in (4, 12, 16, 64, 256, 260):
        out.append((f'c{cout}', cout, (15, 21), 1, 0.25 if cout != 64 else 0.0, 'epi_c4'))
    out.append(('c16_bsum_row_cap', 16, lambda cu: _pos2d(cu * 1024 + 333), 1, 0.25, 'epi_c4'))
    # depth-to-space after the conv: (b, C')
    out += [('d2s_b2_c4', 16, (5, 7), 2, 0.25, 'epi_d2s4'),
            ('d2s_b3_c4_3d', 36, (5, 7, 3), 3, 0.25, 'epi_d2s4'),
            ('d2s_b5_c8', 200, (5, 7), 5, 0.0, 'epi_d2s4'),
            ('d2s_b5_c8_3d_many_blocks', 200, (9, 11, 5), 5, 0.25, 'epi_d2s4'),
            ('d2s_b2_c2', 8, (5, 7), 2, 0.25, 'epi_generic'),
            ('d2s_b2_c1', 4, (5, 7), 2, 0.25, 'epi_generic'),
            ('d2s_b2_c4_no_act', 16, (5, 7), 2, None, 'epi_d2s4')]
    return out


MASK_CASES = _mask_cases()


@pytest.mark.parametrize('fuse', ['default', 'NO_BIAS_FUSE'])
@pytest.mark.parametrize('name,cout,sp,b,slope,kernel', MASK_CASES, ids=[m[0] for m in MASK_CASES])
def test_mask_pass_and_riding_sums(name, cout, sp, b, slope, kernel, fuse):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    sp = _shape_of(sp)
    nd = len(sp)
    spec = [_conv(nd, cout)]
    if b > 1:
        spec.append({'class': 'SpatialExpansion', 'spatial_mult': b} if nd == 2 else
                    {'class': 'SpatioTemporalExpansion', 'spatial_mult': b})
    if slope is not None:
        spec.append(_leaky() if slope else {'class': 'ReLU'})
    shape = (1,) + tuple(sp) + (2,)
    w = _weights(spec, 2, rng, nd)
    x = _data(shape, rng)
    osp = tuple(v * b for v in sp[:2]) + tuple(sp[2:])
    d_out = _data((1,) + osp + (cout // (b * b),), rng, -4, 4)
    opts = dict(SMALL)
    if fuse != 'default':
        opts[fuse] = 1
    got = _run(spec, shape, w, x, d_out, options=opts)
    n_pos = int(np.prod(sp))
    # sums ride the 4-channel pass for C_out / 4 | 256, <= 64; the depth-to-space
    # walk only takes them along with a bf16 y (never in an fp32 plan)
    rides = fuse == 'default' and kernel == 'epi_c4' and _rides(cout)
    expect = [(kernel, 1)]
    expect += [('epi_c4_bsum', 1), ('bias_partial', 1)] if rides else [(_bias_kernel(cout, n_pos), 1)]
    _assert_used(got[3], expect, [BIAS, PARTIAL, EPI, EPI_SUMS])
    _assert_exact(got[:3], _reference(spec, nd, w, x, d_out), name)


# ... and in a bf16 plan.  The depth-to-space walk takes channel sums along
# (conv_epilogue_bwd_d2s4_kernel<true, true> with blocks of (256 / c4) * c4
# lanes, c4 = C_out / 4) only next to a bf16 y and the bf16 copy of dPre, and a
# conv's output is stored as bf16 only if C' % 8 == 0 (conv_mfma_bf16_out_ok)
# and its consumer stages bf16 cells: the 64 -> b^2 * 8 expansion conv ahead of
# the reflect 8 -> 2 output conv, >= 16 time steps and >= 65 536 hi-res
# positions (conv_tail_mfma_supported, conv_wgrad_tail_supported) — the C2
# shape class; from 2 048 lo-res positions on the expansion conv's weight
# gradient is the bf16 trunk kernel, whose reduction the bias job rides.  So
# the issue's (b = 3, C' = 4) has no bf16 y in any plan (its fp32 case is
# above); the block of 252 lanes is reached with (b = 3, C' = 8): c4 = 18.
# (b = 5, C' = 8): c4 = 50, 250 lanes.
#
# Exact all the same.  Injective one-hot filters: y of the expansion conv is an
# integer in [-5, 5], a multiple of 0.25 after the activation (bf16-exact);
# every cell of a data-gradient frame is ONE value; with d_out in [-2, 2] the
# gradient of the hi-res tensor is a fold of <= 8 cells of <= 4 (integers <=
# 32) and dPre of the expansion conv that times 1 or 0.25: at most 7 bits, so
# its bf16 copy is exact and so is everything summed from it in fp32.
D2S16_CASES = [
    # id, b, (N, s1, s2, t) or CU count -> that
    ('b3_c8_block252', 3, (2, 15, 16, 16)),      # 69 120 hi-res positions
    ('b5_c8_block250', 5, (2, 9, 10, 16)),       # 72 000
    # rows of riding sums are capped at 16 CU blocks: 250 lanes * 4 channels each, C_out = 200
    ('b5_c8_block250_row_cap', 5, lambda cu: (2,) + _pos2d(16 * cu * 250 * 4 // (200 * 32) + 3) + (16,)),
]


@pytest.mark.parametrize('fuse', ['default', 'NO_BIAS_FUSE'])
@pytest.mark.parametrize('name,b,sp', D2S16_CASES, ids=[d[0] for d in D2S16_CASES])
def test_depth_to_space_mask_pass_with_riding_sums_bf16(name, b, sp, fuse):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    sp = _shape_of(sp)
    cout = b * b * 8
    spec = [_pad(3, [1, 1, 1]), _conv(3, cout, 3, _w='inj'), {'class': 'SpatioTemporalExpansion', 'spatial_mult': b},
            _leaky(), _pad(3, [1, 1, 1]), _conv(3, 2, 3, _w='inj')]
    shape = sp + (64,)
    w = _weights(spec, 64, rng, 3)
    x = _data(shape, rng)
    d_out = _data((sp[0], sp[1] * b, sp[2] * b, sp[3], 2), rng, -2, 2)
    got = _run(spec, shape, w, x, d_out, precision='bf16', options={fuse: 1} if fuse != 'default' else None)
    used, info = got[3], got[4]
    print('counters:', {k: v for k, v in used.items() if v}, [(i['dgrad'], i['wgrad'], i['out16']) for i in info])
    assert info[0]['out16'] == 1, info[0]
    n_rows = -(-int(np.prod(sp)) * (cout // 4) // ((256 // (cout // 4)) * (cout // 4)))
    assert (n_rows > 16 * _cu()) == name.endswith('row_cap'), n_rows
    # the expansion conv: the depth-to-space walk, with its sums in the default
    # plan; the 2-channel output conv has no activation: no mask pass of its own
    _assert_used(used, [('epi_d2s4', 1)] + ([('epi_d2s4_bsum', 1)] if fuse == 'default' else []), [EPI, EPI_SUMS])
    n_partial = used['bias_partial'] + used['bias_partial_ride']
    assert n_partial == (1 if fuse == 'default' else 0) and used['bias_partial_flush'] == 0, used
    # without the riding sums the bias gradient of C_out = 72 / 200 is the float4 kernel's
    assert used['bias_stage1_v4'] == (0 if fuse == 'default' else 1), used
    _assert_exact(got[:3], _reference(spec, 3, w, x, d_out), name)


# ===================================================================== C
# standalone pad / crop / repeat / depth-to-space / concat ahead of a 1 x 1
# identity conv (so that the plan has parameters)
PAD_SHAPES = [
    # nd, spatial, lo, hi — widths 1, 2, 3, the asymmetric pad of
    # tests/test_ref_surface.py::PAD_CROP, extents down to lo + 1
    (3, (4, 5, 3), [1, 1, 1], [1, 1, 1]),
    (3, (4, 5, 3), [2, 2, 2], [2, 2, 2]),
    (3, (4, 4, 3), [3, 3, 2], [2, 2, 1]),          # every extent = lo + 1
    (3, (7, 5, 4), [3, 3, 3], [3, 3, 3]),
    (2, (6, 5), [3, 3], [3, 3]),
    (2, (3, 33), [2, 1], [1, 2]),
]


@pytest.mark.parametrize('mode', ['REFLECT', 'CONSTANT'])
@pytest.mark.parametrize('c', [1, 2, 4, 8, 64])
@pytest.mark.parametrize('nd,sp,lo,hi', PAD_SHAPES, ids=[f'{p[0]}d_{p[2]}_{p[3]}'.replace(' ', '') for p in PAD_SHAPES])
def test_standalone_pad_adjoint(nd, sp, lo, hi, c, mode):
    rng = np.random.default_rng(c * 7 + sum(lo))
    # (the skip start keeps the pad from being fused into the conv)
    spec = [_pad(nd, lo, hi, mode), {'class': 'SkipConnection', 'name': 'keep'}, _conv(nd, c, _w='identity')]
    shape = (2,) + sp + (c,)
    w = _weights(spec, c, rng, nd)
    x = _data(shape, rng)
    osp = tuple(s + a + b for s, a, b in zip(sp, lo, hi))
    d_out = _data((2,) + osp + (c,), rng, -4, 4)
    got = _run(spec, shape, w, x, d_out, options=SMALL)
    expect = [('fold_pad4', 1), ('fold_plain', 1)] if c % 4 == 0 else [('fold_gather', 1)]
    _assert_used(got[3], expect, [FOLD, FOLD_MODE, EPI])
    _assert_exact(got[:3], _reference(spec, nd, w, x, d_out), 'pad')


GATHERS = [
    ('crop3d', 3, (6, 7, 5), [{'class': 'Cropping3D', 'cropping': [[1, 2], [2, 1], [1, 1]]}], (3, 4, 3), 1),
    ('crop2d', 2, (9, 35), [{'class': 'Cropping2D', 'cropping': [[2, 1], [0, 3]]}], (6, 32), 1),
    ('repeat3', 3, (3, 5, 4), [{'class': 'SpatioTemporalExpansion', 'temporal_mult': 3,
                                'temporal_method': 'nearest'}], (3, 5, 12), 1),
    ('d2s_b2_3d', 3, (3, 5, 2), [{'class': 'SpatioTemporalExpansion', 'spatial_mult': 2}], (6, 10, 2), 4),
    ('d2s_b2_2d', 2, (7, 9), [{'class': 'SpatialExpansion', 'spatial_mult': 2}], (14, 18), 4),
    ('repeat2_d2s2', 3, (3, 4, 3), [{'class': 'SpatioTemporalExpansion', 'temporal_mult': 2, 'spatial_mult': 2,
                                     'temporal_method': 'nearest'}], (6, 8, 6), 4),
]


# (depth-to-space needs C % b^2 == 0: C = 1, 2 are no cases of it)
GATHER_CASES = [g + (c,) for g in GATHERS for c in (1, 2, 4, 8, 64) if c % g[5] == 0]


@pytest.mark.parametrize('name,nd,sp,ops,osp,div,c', GATHER_CASES, ids=[f'{g[0]}-c{g[6]}' for g in GATHER_CASES])
def test_standalone_gather_adjoints(name, nd, sp, ops, osp, div, c):
    rng = np.random.default_rng(c + len(name))
    spec = list(ops) + [_conv(nd, c // div, _w='identity')]
    shape = (2,) + sp + (c,)
    w = _weights(spec, c, rng, nd)
    x = _data(shape, rng)
    d_out = _data((2,) + osp + (c // div,), rng, -4, 4)
    got = _run(spec, shape, w, x, d_out, options=SMALL)
    _assert_used(got[3], [('fold_gather', 2 if name == 'repeat2_d2s2' else 1)], [FOLD, FOLD_MODE])
    _assert_exact(got[:3], _reference(spec, nd, w, x, d_out), name)


@pytest.mark.parametrize('c', [1, 3, 4, 64])
def test_concat_adjoint(c):
    rng = np.random.default_rng(c)
    spec = [_conv(2, c, _w='identity'), {'class': 'Sup3rConcat', 'name': 'topo'}, _conv(2, c + 1, _w='identity')]
    shape = (2, 5, 7, c)
    w = _weights(spec, c, rng, 2)
    x = _data(shape, rng)
    exo = {'topo': _data((2, 5, 7, 1), rng)}
    d_out = _data((2, 5, 7, c + 1), rng, -4, 4)
    got = _run(spec, shape, w, x, d_out, options=SMALL, exo=exo)
    # the adjoint of a concat copies channel ranges (copy_channels_kernel), which
    # is no variant of anything and has no counter: no fold, mask pass or
    # accumulation may run for it, and the two convs take their bias gradients
    # from launch_bias_grad
    n_bias = {}
    for ch in (c, c + 1):                # (70 positions)
        n_bias[_bias_kernel(ch, 70)] = n_bias.get(_bias_kernel(ch, 70), 0) + 1
    _assert_used(got[3], list(n_bias.items()), [BIAS, PARTIAL, EPI, EPI_SUMS, FOLD, FOLD_MODE, AXPY])
    _assert_exact(got[:3], _reference(spec, 2, w, x, d_out, exo), 'concat')


# frame folds inside residual blocks: 64 -> 64 reflect convs (the trunk
# geometry: 3 x 3 x 3, >= 8 time steps), fp32 plan
def _trunk(n_convs, acts, skip=None, kind='one_hot'):
    spec = []
    for i in range(n_convs):
        if skip and i == skip[0]:
            spec.append({'class': 'SkipConnection', 'name': 's'})
        spec += [_pad(3, [1, 1, 1]), _conv(3, 64, 3, _w=kind)]
        if acts[i] is not None:
            spec.append(_leaky() if acts[i] else {'class': 'ReLU'})
        if skip and i == skip[1]:
            spec.append({'class': 'SkipConnection', 'name': 's'})
    return spec


TRUNK_SHAPE = (2, 8, 8, 9, 64)          # 1 152 positions: past the few-position family


def _trunk_case(spec, shape, seed):
    rng = np.random.default_rng(seed)
    w = _weights(spec, 64, rng, 3)
    x = _data(shape, rng)
    d_out = _data(shape, rng, -4, 4)
    return w, x, d_out


@pytest.fixture(scope='module')
def trunk3():
    spec = _trunk(3, [0.25, 0.0, None])
    w, x, d_out = _trunk_case(spec, TRUNK_SHAPE, 31)
    return spec, w, x, d_out, _reference(spec, 3, w, x, d_out)


@pytest.mark.parametrize('opt', ['default', 'NO_MASK_FUSE', 'NO_BIAS_FUSE'])
def test_frame_fold_with_the_activation_fused(trunk3, opt):
    """conv -> act -> reflect conv, three deep: the folds of conv 3 and conv 2
    apply the activation adjoint of the conv below (fp32 y) and leave its bias
    gradient's channel sums, the fold of conv 1 (onto the input) is plain"""
    spec, w, x, d_out, ref = trunk3
    got = _run(spec, TRUNK_SHAPE, w, x, d_out, options=None if opt == 'default' else {opt: 1})
    assert [i['dgrad'] for i in got[4]] == ['mfma_frame'] * 3, got[4]
    if opt == 'NO_MASK_FUSE':
        expect = [('fold_pad4', 3), ('fold_plain', 3), ('epi_c4', 2), ('epi_c4_bsum', 2), ('bias_partial', 2),
                  ('bias_stage1_v4', 1)]
    elif opt == 'NO_BIAS_FUSE':
        expect = [('fold_pad4', 3), ('fold_masked', 2), ('fold_plain', 1), ('bias_stage1_v4', 3)]
    else:
        expect = [('fold_pad4', 3), ('fold_masked', 2), ('fold_plain', 1), ('bias_partial', 2), ('bias_stage1_v4', 1)]
    _assert_used(got[3], expect, [BIAS, PARTIAL, EPI, EPI_SUMS, FOLD, FOLD_MODE])
    _assert_exact(got[:3], ref, opt)


def test_frame_fold_added_to_the_first_contribution_of_a_skip_tensor():
    """s = conv0(x); y = conv2(act(conv1(s))) + s: the skip add hands s its
    first gradient contribution, the fold of conv1's frame adds the second in
    the same store (the MASK == 3 form)"""
    spec = _trunk(4, [None, 0.25, None, None], skip=(1, 2))
    w, x, d_out = _trunk_case(spec, TRUNK_SHAPE, 32)
    got = _run(spec, TRUNK_SHAPE, w, x, d_out)
    _assert_used(got[3], [('fold_pad4', 4), ('fold_add', 1), ('fold_masked', 1), ('fold_plain', 2)],
                 [FOLD, FOLD_MODE, AXPY])
    _assert_exact(got[:3], _reference(spec, 3, w, x, d_out), 'skip add')


def test_frame_fold_of_the_few_position_family():
    """<= 1 024 positions: the trunk convs run on the one-launch kernels, whose
    reflect frames go through the same folds"""
    spec = _trunk(2, [0.25, None])
    shape = (1, 4, 5, 8, 64)
    w, x, d_out = _trunk_case(spec, shape, 33)
    got = _run(spec, shape, w, x, d_out)
    _assert_used(got[3], [('fold_pad4', 2), ('fold_masked', 1), ('fold_plain', 1)], [FOLD, FOLD_MODE])
    _assert_exact(got[:3], _reference(spec, 3, w, x, d_out), 'fewpos fold')


# bf16 frames: the persistent data gradient writes its padded frame as bf16.
# Permutation filters: every frame cell is ONE bf16-exact value.  Three convs
# deep (LeakyReLU 0.25, ReLU, none) every tensor the bf16 plan stores is
# bf16-exact: the activations are multiples of 0.25 below 8; dPre of conv 2 is
# a fold of <= 8 frame cells with |d| <= 4 times 0 or 1 (integers <= 32), dPre
# of conv 1 a fold of <= 8 of those times 1 or 0.25 (<= 256 units: 8 bits) —
# so the fp32 results are still exact.  18 x 18 frames, 12 time steps, 8 samples.
BF16_SHAPE = (8, 16, 16, 12, 64)
BF16_BASE = {'PERSIST_DGRAD_MIN_TILES': 1}


@pytest.fixture(scope='module')
def trunk_bf16():
    spec = _trunk(3, [0.25, 0.0, None], kind='perm')
    w, x, d_out = _trunk_case(spec, BF16_SHAPE, 34)
    return spec, w, x, d_out, _reference(spec, 3, w, x, d_out)


# conv 3's dPre is d_out itself (fp32): its data gradient leaves an fp32 frame.
# Its fold (mask of conv 2 from the bf16 y) stores dPre of conv 2 as bf16 only,
# so conv 2 runs the persistent data gradient and its bf16 frame is folded with
# conv 1's mask (fold16x8, MASK from a bf16 y).  conv 1 reads the fp32 input of
# the plan, so its dPre stays fp32 and its frame too: the plain fold onto dx is
# the 4-channel one.  With NO_MASK_FUSE the mask passes leave bf16 copies of
# both dPre and both bf16 frames are folded plainly (fold16x8, MASK 0).
_FOLDS16 = [('fold_pad4', 2), ('fold16x8', 1), ('fold_masked', 2), ('fold_plain', 1)]
BF16_VARIANTS = [
    # name, options, fold (and mask-pass) counters expected, launches of the persistent data gradient
    ('default', {}, _FOLDS16, 1),
    ('NO_FRAME16', {'NO_FRAME16': 1}, [('fold_pad4', 3), ('fold_masked', 2), ('fold_plain', 1)], 1),
    ('NO_FOLD16', {'NO_FOLD16': 1}, _FOLDS16, 1),
    ('NO_PLAIN_FOLD16', {'NO_PLAIN_FOLD16': 1}, _FOLDS16, 1),
    # (the only place the 4-channel mask pass reads a bf16 y and leaves the bf16 copy)
    ('NO_MASK_FUSE', {'NO_MASK_FUSE': 1}, [('fold_pad4', 1), ('fold16x8', 2), ('fold_plain', 3), ('epi_c4', 2),
                                           ('epi_c4_bsum', 2)], 2),
    # (without its channel sums a dPre is not stored as bf16 only: fp32 frames throughout)
    ('NO_BIAS_FUSE', {'NO_BIAS_FUSE': 1}, [('fold_pad4', 3), ('fold_masked', 2), ('fold_plain', 1)], 0),
]


@pytest.mark.parametrize('name,opts,expect,n_persist', BF16_VARIANTS, ids=[v[0] for v in BF16_VARIANTS])
def test_bf16_frame_fold(trunk_bf16, name, opts, expect, n_persist):
    spec, w, x, d_out, ref = trunk_bf16
    got = _run(spec, BF16_SHAPE, w, x, d_out, precision='bf16', options=dict(BF16_BASE, **opts))
    used = got[3]
    print('counters:', {k: v for k, v in used.items() if v}, [i['dgrad'] + '/' + i['wgrad'] for i in got[4]])
    assert used['persist_dgrad'] == n_persist, used
    _assert_used(used, expect, [FOLD, FOLD_MODE, EPI, EPI_SUMS])
    if name == 'NO_BIAS_FUSE':
        assert sum(used[k] for k in PARTIAL) == 0 and used['bias_stage1_v4'] == 3, used
    else:
        # conv 2 and conv 1 (the last conv the backward walk visits) take their
        # bias gradients from riding sums, and the job rides along the reduction
        # of the bf16 trunk weight gradient that follows it (ConvBwd::bias): db
        # of conv 1 must be there when backward returns
        assert used['bias_partial_ride'] == 2 and used['bias_partial'] == 0 and used['bias_partial_flush'] == 0, used
        assert used['bias_stage1_v4'] == 1, used
    _assert_exact(got[:3], ref, name)


# ... and the ADD form on a bf16 frame (fold16x8, MASK 3): s = conv0(x);
# y = conv3(conv2(act(conv1(s))) + s).  conv 3's fp32 frame is folded plainly
# onto the sum (with the bf16 copy conv 2 reads), which is also s's first
# contribution; conv 2's bf16 frame is folded with conv 1's mask; conv 1's bf16
# frame is folded and ADDED to that first contribution in the same store, with
# the bf16 copy of the result (dPre of conv 0) unless NO_FOLD16 takes it away.
# With d_out in [-1, 1] every gradient the plan stores is a multiple of 0.25
# of at most 8 bits (checked on the reference, below).
def _bf16_exact(a):
    a32 = np.asarray(a, np.float32)
    return bool((a32 == a).all() and ((np.ascontiguousarray(a32).view(np.uint32) & 0xFFFF) == 0).all())


@pytest.fixture(scope='module')
def skip_bf16():
    spec = _trunk(4, [None, 0.25, None, None], skip=(1, 2), kind='perm')
    rng = np.random.default_rng(35)
    w = _weights(spec, 64, rng, 3)
    x = _data(BF16_SHAPE, rng)
    d_out = _data(BF16_SHAPE, rng, -1, 1)
    net = R.RefNet(_clean(spec), 3)
    ref = _reference(spec, 3, w, x, d_out, net=net)
    # what the bf16 plan stores — every conv's input (the activations, the skip
    # sum), what the skip add reads (the sum minus s = conv 2's output) and
    # every conv's dPre — survives the round trip through bf16 unchanged
    ins = [rec[4] for rec in net._tape if rec[0] == 'conv']
    stored = ins + [rec[1] for rec in net._tape if rec[0] == 'act'] + [ins[3] - ins[1]] + list(net.dpre)
    return spec, w, x, d_out, ref, all(_bf16_exact(t) for t in stored)


# Counters of a run with the library of the parent commit.  NO_FOLD16 takes the
# bf16 side copies away and the plan follows: conv 2 then reads an fp32 dPre
# and leaves an fp32 frame, and so does conv 0; the one bf16 frame left is
# conv 1's (its dPre is the bf16-only store of the masked fold), and its fold
# is the ADD — on the 8-wide walk in both variants, with and without the copy.
_SKIP16 = {
    # options: (fold counters, launches of the persistent data gradient)
    'default': ([('fold_pad4', 1), ('fold16x8', 3), ('fold_plain', 2), ('fold_masked', 1), ('fold_add', 1)], 3),
    'NO_FOLD16': ([('fold_pad4', 3), ('fold16x8', 1), ('fold_plain', 2), ('fold_masked', 1), ('fold_add', 1)], 1),
}


@pytest.mark.parametrize('name', list(_SKIP16))
def test_bf16_frame_fold_added_to_a_skip_tensor(skip_bf16, name):
    spec, w, x, d_out, ref, exact = skip_bf16
    assert exact, 'a tensor the bf16 plan stores is not bf16-exact: assert_array_equal would mean nothing'
    expect, n_persist = _SKIP16[name]
    got = _run(spec, BF16_SHAPE, w, x, d_out, precision='bf16',
               options=dict(BF16_BASE, **({} if name == 'default' else {name: 1})))
    used = got[3]
    print('counters:', {k: v for k, v in used.items() if v}, [i['dgrad'] + '/' + i['wgrad'] for i in got[4]])
    assert used['persist_dgrad'] == n_persist, used
    _assert_used(used, expect, [FOLD, FOLD_MODE, AXPY])
    assert used['fold_add'] == 1 and used['fold16x8'] >= 1, used
    # (two bias gradients ride along the sums a fold left, two are launch_bias_grad's)
    assert used['bias_partial_ride'] == 2 and used['bias_stage1_v4'] == 2, used
    _assert_exact(got[:3], ref, 'skip add on a bf16 frame, ' + name)


# ===================================================================== D
@pytest.mark.parametrize('c,kernel', [(3, 'axpy'), (4, 'axpy4')])
def test_skip_accumulation(c, kernel):
    """a skip tensor with two consumers that are no folds: the second
    contribution lands by y += x; 3 069 elements (odd) / 4 092 (float4)"""
    rng = np.random.default_rng(c)
    spec = [_conv(2, c), {'class': 'SkipConnection', 'name': 's'}, _conv(2, c), _leaky(),
            {'class': 'SkipConnection', 'name': 's'}, _conv(2, c)]
    shape = (1, 33, 31, 2)
    w = _weights(spec, 2, rng, 2)
    x = _data(shape, rng)
    d_out = _data((1, 33, 31, c), rng, -4, 4)
    got = _run(spec, shape, w, x, d_out, options=SMALL)
    _assert_used(got[3], [(kernel, 1)], [AXPY])
    _assert_exact(got[:3], _reference(spec, 2, w, x, d_out), kernel)


# ============================================================ C ABI, direct
def _dev():
    from sup3r_amd import _lib
    from sup3r_amd.engine import Device
    return _lib, _lib.lib(), Device.get()


REL = 2.0 ** -22     # two fp32 roundings: 1 / total (or weight / total) and the product


def _loss_cases():
    big1, big4 = 1024 * 256, 4 * 1024 * 256      # elements one sweep of the capped grids covers
    return [
        # id, n_pos, c_a, c_b, c_used, mask channels (0: none), accumulate, with gradient
        ('dense_small', 999, 4, 4, 4, 0, 0, True),
        ('dense_float4_capped', big4 // 4 + 5, 4, 4, 4, 0, 0, True),
        ('dense_accumulate', 1001, 4, 4, 4, 0, 1, True),
        ('dense_no_gradient', 1001, 4, 4, 4, 0, 0, False),
        ('scalar_odd_total', 1023, 1, 1, 1, 0, 0, True),
        ('scalar_subset_capped', big1 // 2 + 39, 3, 2, 2, 0, 0, True),
        ('scalar_subset_accumulate', 777, 3, 4, 2, 0, 1, True),
        ('scalar_masked', 1500, 2, 2, 2, 3, 0, True),
        ('scalar_masked_no_gradient', 1500, 4, 4, 4, 4, 0, False),
    ]


LOSS_CASES = _loss_cases()


def _loss_call(kind, a, b, c_used, mask, weight, d_a0, want_grad, acc=0):
    _lib, L, dev = _dev()
    ad, bd = dev.to_device(a), dev.to_device(b)
    loss = dev.empty((1,))
    da = dev.to_device(d_a0) if want_grad else None
    dap = C.c_void_p(da.data_ptr()) if want_grad else None
    n_pos = a.shape[0]
    if mask is None:
        rc = L.s3_loss_content(dev.ctx, kind, ad.data_ptr(), a.shape[1], bd.data_ptr(), b.shape[1], c_used, n_pos,
                               weight, loss.data_ptr(), dap, acc)
    else:
        md = dev.to_device(mask)
        rc = L.s3_loss_content_masked(dev.ctx, kind, ad.data_ptr(), a.shape[1], bd.data_ptr(), b.shape[1],
                                      md.data_ptr(), mask.shape[1], c_used, n_pos, weight, loss.data_ptr(), dap, acc)
    _lib.check(rc, dev.ctx, 's3_loss_content')
    dev.sync()
    return float(loss.item()), (da.cpu().numpy() if want_grad else None)


@pytest.mark.parametrize('kind', ['mae', 'mse'])
@pytest.mark.parametrize('name,n_pos,c_a,c_b,c_used,c_m,acc,want_grad', LOSS_CASES, ids=[c[0] for c in LOSS_CASES])
def test_content_loss(name, n_pos, c_a, c_b, c_used, c_m, acc, want_grad, kind):
    """integer inputs with |d| <= 2 (zeros included: gradient 0): the sum is
    exact, value and every gradient element within 2^-22 relative.  d_a starts
    from integers in [-2, 2] where the call accumulates and from a sentinel
    where it does not (the gradient is written over it); channels >= c_used
    are not the call's: they keep what they held either way"""
    _lib = _dev()[0]
    rng = np.random.default_rng(n_pos + c_a)
    a = rng.integers(-1, 2, size=(n_pos, c_a)).astype(np.float32)
    b = rng.integers(-1, 2, size=(n_pos, c_b)).astype(np.float32)
    mask = rng.choice([0.0, 0.5, 1.0], size=(n_pos, c_m)).astype(np.float32) if c_m else None
    d0 = rng.integers(-2, 3, size=a.shape).astype(np.float32) if acc else np.full(a.shape, 7.0, np.float32)
    val, grad = _loss_call({'mae': _lib.LOSS_MAE, 'mse': _lib.LOSS_MSE}[kind], a, b, c_used, mask, 0.5, d0, want_grad,
                           acc)
    ref_v, ref_g = R.content_loss(kind, a, b, c_used, mask, 0.5)
    assert (a[:, :c_used] == b[:, :c_used]).any()
    print(name, kind, 'value', val, ref_v)
    assert abs(val - ref_v) <= REL * abs(ref_v), (val, ref_v)
    if want_grad:
        ref = ref_g.copy()
        ref[:, c_used:] = d0[:, c_used:]
        if acc:
            ref[:, :c_used] += d0[:, :c_used]
        err = np.abs(grad - ref)
        print('gradient: worst error / |ref|', float((err / np.maximum(np.abs(ref), 1e-300)).max()))
        assert (err <= REL * np.abs(ref)).all()
        np.testing.assert_array_equal(grad[:, c_used:], d0[:, c_used:])


def test_content_loss_exp_capped_grid():
    """S3_LOSS_EXP uses __expf, whose error is not derived here: one capped-grid
    case at the tolerances tests/test_losses.py holds the loss kernels to"""
    _lib = _dev()[0]
    rng = np.random.default_rng(5)
    n_pos = 1024 * 256 + 41
    a = rng.standard_normal((n_pos, 4)).astype(np.float32)
    b = rng.standard_normal((n_pos, 4)).astype(np.float32)
    ref_v, ref_g = R.content_loss('exp', a, b, 4, None, 1.0)
    val, grad = _loss_call(_lib.LOSS_EXP, a, b, 4, None, 1.0, np.zeros(a.shape, np.float32), True)
    assert abs(val - ref_v) <= 2e-5 * max(1.0, abs(ref_v)), (val, ref_v)
    for _ in range(3):
        v = rng.standard_normal(a.shape)
        an, fd = float((grad.astype(np.float64) * v).sum()), float((ref_g * v).sum())
        assert abs(an - fd) <= 2e-3 * max(abs(fd), 1e-3), (an, fd)
    # ... and the scalar walk (a channel subset) at the same size
    ref_v, ref_g = R.content_loss('exp', a, b, 3, None, 1.0)
    val, grad = _loss_call(_lib.LOSS_EXP, a, b, 3, None, 1.0, np.zeros(a.shape, np.float32), True)
    assert abs(val - ref_v) <= 2e-5 * max(1.0, abs(ref_v)), (val, ref_v)
    v = rng.standard_normal(a.shape)
    an, fd = float((grad.astype(np.float64) * v).sum()), float((ref_g * v).sum())
    assert abs(an - fd) <= 2e-3 * max(abs(fd), 1e-3), (an, fd)


@pytest.mark.parametrize('n', [1, 15, 64, 255, 256, 257, 600])
def test_rel_bce(n):
    """single block of 256 lanes: n = 600 walks the in-block stride loop; the
    tolerances of tests/test_hip_parity.py::test_losses_adam_utils"""
    _lib, L, dev = _dev()
    rng = np.random.default_rng(n)
    dt = (rng.standard_normal(n) * 3).astype(np.float32)
    dg = (rng.standard_normal(n) * 3).astype(np.float32)
    loss, g_t, g_g = dev.empty((1,)), dev.empty((n,)), dev.empty((n,))
    dtd, dgd = dev.to_device(dt), dev.to_device(dg)
    rc = L.s3_loss_rel_bce(dev.ctx, dtd.data_ptr(), dgd.data_ptr(), n, 2.0, loss.data_ptr(), g_t.data_ptr(),
                           g_g.data_ptr())
    _lib.check(rc, dev.ctx, 's3_loss_rel_bce')
    rl, rt, rg = R.rel_bce(dt, dg)
    print('rel_bce', n, abs(loss.item() - rl), np.abs(g_t.cpu().numpy() - 2 * rt).max(),
          np.abs(g_g.cpu().numpy() - 2 * rg).max())
    assert abs(loss.item() - rl) < 1e-5
    np.testing.assert_allclose(g_t.cpu().numpy(), 2 * rt, atol=1e-6, rtol=0)
    np.testing.assert_allclose(g_g.cpu().numpy(), 2 * rg, atol=1e-6, rtol=0)


class _Store:
    """an s3_params store created directly from a list of sizes"""

    def __init__(self, sizes):
        self._lib, self.L, self.dev = _dev()
        self.sizes = [int(s) for s in sizes]
        arr = (C.c_int64 * len(sizes))(*self.sizes)
        self.h = C.c_void_p()
        self._lib.check(self.L.s3_params_create(self.dev.ctx, len(sizes), arr, C.byref(self.h)), self.dev.ctx,
                        's3_params_create')

    def set(self, which, arrays):
        for i, a in enumerate(arrays):
            a = np.ascontiguousarray(a, np.float32)
            assert a.size == self.sizes[i]
            self._lib.check(self.L.s3_params_set(self.h, which, i, a.ctypes.data_as(C.POINTER(C.c_float))),
                            self.dev.ctx, 's3_params_set')

    def get(self, which):
        out = []
        for i, n in enumerate(self.sizes):
            buf = np.empty(n, np.float32)
            self._lib.check(self.L.s3_params_get(self.h, which, i, buf.ctypes.data_as(C.POINTER(C.c_float))),
                            self.dev.ctx, 's3_params_get')
            out.append(buf)
        return out

    def step(self, kind, hyper, t, staged=False):
        hp = (C.c_double * len(hyper))(*[float(v) for v in hyper])
        if staged:
            self._lib.check(self.L.s3_optimizer_stage(self.h, kind, hp, len(hyper), t), self.dev.ctx, 'stage')
            self._lib.check(self.L.s3_optimizer_step_staged(self.h, kind), self.dev.ctx, 'step_staged')
        else:
            self._lib.check(self.L.s3_optimizer_step(self.h, kind, hp, len(hyper), t), self.dev.ctx, 'step')

    def close(self):
        if self.h:
            self.L.s3_params_destroy(self.h)
            self.h = None


def _store_sizes():
    """tensor sizes that are no multiples of 4, several blocks, and a total
    past the 8 * CU blocks of 256 float4 lanes of grid_for (the capped grid).
    s3_params_create pads every tensor to a multiple of 4 floats, so the
    store's total is one too and the kernels' scalar tails (n % 4 elements)
    cannot run through this ABI: what these sizes check is that a tensor's
    last, partly filled float4 and its neighbours' first are right"""
    small = [1, 3, 1021, 4099, 300007]
    cap = 8 * _cu() * 256 * 4
    return small + [cap - sum(small) + 4099]


from tests.test_optimizers import CASES as OPT_CASES   # noqa: E402

ALL_OPT = [('Adam', {'learning_rate': 1e-2})] + list(OPT_CASES)


@pytest.mark.parametrize('name,kw', ALL_OPT, ids=[f'{n}-{i}' for i, (n, _) in enumerate(ALL_OPT)])
def test_optimizer_steps_over_a_capped_grid(name, kw):
    """three steps on a store of six tensors (2.1 M elements at 256 CUs)
    against the float64 keras restatement, every tensor at the tolerances of
    tests/test_optimizers.py; the staged form is bit-identical"""
    from oracle import gan as G
    from sup3r_amd import _lib
    from sup3r_amd.optimizers import init_optimizer
    sizes = _store_sizes()
    assert sum((s + 3) // 4 * 4 for s in sizes) > 8 * _cu() * 256 * 4
    rng = np.random.default_rng(17)
    w0 = [rng.standard_normal(s).astype(np.float32) for s in sizes]
    a, b = _Store(sizes), _Store(sizes)
    try:
        a.set(_lib.BUF_W, w0)
        b.set(_lib.BUF_W, w0)
        opt = init_optimizer(dict(kw, name=name), None)
        ref = G.Adam(**kw) if name == 'Adam' else G.KerasOptimizer(name, **kw)
        w = [x.astype(np.float64) for x in w0]
        for t in range(1, 4):
            g = [(rng.standard_normal(s) * 0.3).astype(np.float32) for s in sizes]
            a.set(_lib.BUF_G, g)
            b.set(_lib.BUF_G, g)
            a.step(opt.KIND, opt.hyper(), t)
            # (Adagrad's first step creates the accumulator: not stageable)
            b.step(opt.KIND, opt.hyper(), t, staged=not (name == 'Adagrad' and t == 1))
            ref.apply_gradients([x.astype(np.float64) for x in g], w)
            got = a.get(_lib.BUF_W)
            for i, (x, y) in enumerate(zip(got, w)):
                tol = 2e-6 * max(1.0, np.abs(y).max())
                assert np.abs(x - y).max() < tol, (name, kw, t, i)
                for j in list(range(min(4, x.size))) + list(range(max(0, x.size - 4), x.size)):
                    assert abs(x[j] - y[j]) < 2e-6 * max(1.0, abs(y[j])), (name, t, i, j)
        for i, (x, y) in enumerate(zip(a.get(_lib.BUF_V), ref.v)):
            assert np.abs(x - y).max() < 1e-5 * max(1e-3, np.abs(y).max()), (name, i)
        for buf in (_lib.BUF_W, _lib.BUF_M, _lib.BUF_V):
            for x, y in zip(a.get(buf), b.get(buf)):
                np.testing.assert_array_equal(x, y)
    finally:
        a.close()
        b.close()


def test_adam_step_is_the_adam_optimizer_step():
    from oracle import gan as G
    from sup3r_amd import _lib
    sizes = _store_sizes()
    rng = np.random.default_rng(18)
    w0 = [rng.standard_normal(s).astype(np.float32) for s in sizes]
    a, b = _Store(sizes), _Store(sizes)
    try:
        ref = G.Adam(learning_rate=1e-3)
        w = [x.astype(np.float64) for x in w0]
        a.set(_lib.BUF_W, w0)
        b.set(_lib.BUF_W, w0)
        for t in range(1, 4):
            g = [(rng.standard_normal(s) * 0.3).astype(np.float32) for s in sizes]
            a.set(_lib.BUF_G, g)
            b.set(_lib.BUF_G, g)
            _lib.check(a.L.s3_adam_step(a.h, 1e-3, 0.9, 0.999, 1e-7, t), a.dev.ctx, 's3_adam_step')
            # (s3_adam_step takes floats: hand the other call the same values)
            b.step(_lib.OPT_ADAM, [np.float32(1e-3), np.float32(0.9), np.float32(0.999), np.float32(1e-7)], t)
            ref.apply_gradients([x.astype(np.float64) for x in g], w)
        for buf in (_lib.BUF_W, _lib.BUF_M, _lib.BUF_V):
            for x, y in zip(a.get(buf), b.get(buf)):
                np.testing.assert_array_equal(x, y)
        for i, (x, y) in enumerate(zip(a.get(_lib.BUF_W), w)):
            assert np.abs(x - y).max() < 2e-6 * max(1.0, np.abs(y).max()), i
            for j in list(range(min(4, x.size))) + list(range(max(0, x.size - 4), x.size)):
                assert abs(x[j] - y[j]) < 2e-6 * max(1.0, abs(y[j])), (i, j)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize('n,rel', [(2 ** 19, 2.0 ** -24), (300007, 2.0 ** -23)])
def test_params_mean_abs(n, rel):
    """integers: the sum of |p| is exact in any order.  n = 2^19 (above the
    1024 blocks of 256 lanes): 1 / n is exact, one rounding at most.  n =
    300 007 (ragged against the grid): 1 / n and the product round, 2^-23"""
    from sup3r_amd import _lib
    rng = np.random.default_rng(n)
    p = rng.integers(-2, 3, size=n).astype(np.float32)
    s = _Store([5, n, 7])
    try:
        s.set(_lib.BUF_M, [np.ones(5), p, np.ones(7)])
        v = C.c_float()
        _lib.check(s.L.s3_params_mean_abs(s.h, _lib.BUF_M, 1, C.byref(v)), s.dev.ctx, 's3_params_mean_abs')
        ref = float(np.abs(p.astype(np.float64)).sum() / n)
        print('mean_abs', n, v.value, ref)
        assert abs(v.value - ref) <= rel * ref
    finally:
        s.close()
