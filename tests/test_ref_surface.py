"""The reference's whole shipped spec surface (``sup3r/configs/**``: 16
generators + 2 discriminators, authored as data under
``sup3r_amd/configs/sup3r/`` by ``configs/author_configs.py``) through this
build, the way ``/root/reference/tests/training/test_load_configs.py:17-133``
walks it — plus what that file cannot check without an oracle: the numbers.

CPU (``-m "not gpu"``):
* every authored spec EQUALS the reference's file (by a digest of its JSON
  value, stored in ``tests/golden/reference_config_digests.json``);
* the shape contract of ``test_load_configs.py`` on every spec;
* the fused and the unfused device plan of every spec, interpreted in float64
  (``tests/plan_interp.py``), against the layer-by-layer oracle;
* ``temporal_method: depth_to_time`` with ``t_roll`` in {0, m/2, > T, < 0}:
  the oracle layer against the literal ``reshape`` + ``roll`` statement on
  exact-integer inputs, the plan ops against the oracle, and the adjoint.

GPU (``-m gpu``): every spec forward + backward through the C-ABI against the
oracle — fp32 plans: forward L-inf < 1e-4 of the output scale, every gradient
< 1e-3 of its tensor's largest value under the device's activation masks;
bf16 plans: per op teacher-forced (at most one bf16 spacing on at most 1 % of
an op's elements) + 3e-2 end to end, gradients 2e-2 — and the depth_to_time /
roll kernels bit-exactly on integers.
"""
import glob
import hashlib
import json
import os

import numpy as np
import pytest

from oracle.network import Network as OracleNet
from sup3r_amd import spec as S
from tests.plan_interp import run_plan

HERE = os.path.dirname(os.path.abspath(__file__))
SURFACE = os.path.join(HERE, '..', 'sup3r_amd', 'configs', 'sup3r')
REF_DIGESTS = os.path.join(HERE, 'golden', 'reference_config_digests.json')

# rel. path -> (low-res input shape for the numeric tests, exo name or None).
# Shapes follow test_load_configs.py's family ((1, 5, 5, 4, 2), (3, 6, 6, 8, 2),
# (n, 5, 5, 2)) with unequal s1 / s2 so that a transposed axis cannot pass;
# the discriminators get the smallest extent that survives four valid
# stride-1 and four valid stride-2 convolutions (61).
CASES = {
    'spatial/disc.json': ((2, 61, 63, 2), None),
    'spatial/gen_2x_1f.json': ((3, 7, 6, 1), None),
    'spatial/gen_2x_2f.json': ((3, 7, 6, 2), None),
    'spatial/gen_10x_2f.json': ((2, 5, 6, 2), None),
    'spatiotemporal/disc.json': ((1, 61, 62, 61, 2), None),
    'spatiotemporal/gen_2x_2x_2f.json': ((2, 5, 6, 4, 2), None),
    'spatiotemporal/gen_2x_12x_14f.json': ((1, 5, 6, 4, 14), None),
    'spatiotemporal/gen_3x_4x_1f.json': ((2, 5, 6, 4, 1), None),
    'spatiotemporal/gen_3x_4x_2f.json': ((2, 6, 5, 4, 2), None),
    'spatiotemporal/gen_3x_4x_10f.json': ((1, 5, 6, 4, 10), None),
    'spatiotemporal/gen_3x_4x_14f.json': ((1, 6, 5, 4, 14), None),
    'spatiotemporal/gen_4x_24x_3f.json': ((1, 5, 4, 4, 3), None),
    'sup3rcc/gen_solar_1x_8x_1f.json': ((2, 6, 5, 4, 3), None),
    'sup3rcc/gen_trh_1x_24x_2f.json': ((1, 5, 6, 4, 4), None),
    'sup3rcc/gen_solar_5x_1x_1f.json': ((2, 6, 5, 3), None),
    'sup3rcc/gen_wind_5x_1x_6f.json': ((2, 5, 6, 4), 'topography'),
    'sup3rcc/gen_wind_1x_24x_6f.json': ((1, 5, 4, 3, 6), None),
    'sup3rcc/gen_wind_3x_4x_2f.json': ((2, 5, 6, 4, 2), 'topography'),
}


def load_surface(rel):
    with open(os.path.join(SURFACE, rel)) as f:
        return json.load(f)


def json_digest(value):
    """SHA-256 of a parsed JSON value, independent of key order and layout"""
    text = json.dumps(value, sort_keys=True, separators=(',', ':'))
    return hashlib.sha256(text.encode()).hexdigest()


def reference_digests():
    """rel. path -> digest of every spec file the reference ships"""
    with open(REF_DIGESTS) as f:
        return json.load(f)['files']


def _enhancements(rel):
    parts = os.path.basename(rel).replace('.json', '').split('_')
    nums = [int(p[:-1]) for p in parts if p.endswith('x')]
    nf = [int(p[:-1]) for p in parts if p.endswith('f')]
    return nums, (nf[0] if nf else None)


def _exo_for(plan, name, rng, dtype):
    sh = plan.tensors[plan.inputs[name]]
    keras = tuple(sh) if plan.out_rank == 5 else \
        (sh[0], sh[1], sh[2], sh[4])
    return {name: rng.standard_normal(tuple(keras)).astype(dtype)}


def test_surface_is_complete():
    files = sorted(os.path.relpath(p, SURFACE) for p in
                   glob.glob(os.path.join(SURFACE, '*', '*.json')))
    assert files == sorted(CASES), files
    assert sum('gen_' in f for f in files) == 16
    assert sum('disc' in f for f in files) == 2


def test_authored_surface_equals_reference():
    """the authored files are the reference's spec surface, value for value,
    and the reference ships nothing else there"""
    ref = reference_digests()
    ref_files = sorted(ref)
    assert ref_files == sorted(CASES)
    for rel in ref_files:
        assert json_digest(load_surface(rel)) == ref[rel], rel


@pytest.mark.parametrize('rel', sorted(c for c in CASES if 'gen_' in c))
def test_surface_shape_contract(rel):
    """test_load_configs.py:41-133: output = enhancement x input for the
    coarse shapes that file uses, features as the file name says"""
    spec = load_surface(rel)
    layers = S.parse_layers(spec)
    nums, nf_out = _enhancements(rel)
    s_enh = int(np.prod([L._spatial_mult for L in layers]))
    t_enh = int(np.prod([L._temporal_mult for L in layers]))
    is_5d = layers[0].rank == 5
    # sup3rcc 1x/…x and …x/1x names carry both factors; spatial/ only one
    if len(nums) == 2:
        assert (s_enh, t_enh) == tuple(nums), rel
    else:
        assert (s_enh, t_enh) == (nums[0], 1), rel
    shapes = ((1, 5, 5, 4, 2), (1, 7, 7, 9, 2), (3, 6, 6, 8, 2)) if is_5d \
        else ((1, 5, 5, 2), (32, 5, 5, 2), (16, 10, 10, 2))
    table = None
    for shape in shapes:
        plan = S.build_plan(layers, shape, param_table=table)
        table = table or plan.params
        out = plan.out_shape
        assert len(out) == len(shape)
        assert out[0] == shape[0]
        assert out[1] == s_enh * shape[1] and out[2] == s_enh * shape[2]
        if is_5d:
            assert out[3] == t_enh * shape[3]
        assert out[-1] == nf_out


@pytest.mark.parametrize('rel', sorted(CASES))
@pytest.mark.parametrize('fuse', [True, False])
def test_surface_plan_matches_oracle(rel, fuse):
    """the device plan (fused: virtual pads, epilogues, d2s stores; unfused:
    one op per layer) interpreted in float64 == the layer-by-layer oracle"""
    shape, exo_name = CASES[rel]
    spec = load_surface(rel)
    rng = np.random.default_rng(7)
    x = rng.standard_normal(shape)
    layers = S.parse_layers(spec)
    plan = S.build_plan(layers, shape, fuse=fuse)
    exo = _exo_for(plan, exo_name, rng, np.float64) if exo_name else None
    net = OracleNet(spec)
    net.init_weights(x, exo, seed=3, bias_scale=0.1)
    net.cast(np.float64)
    y_ref = net.forward(x, exo)
    assert tuple(plan.out_shape) == y_ref.shape
    assert [tuple(p['shape']) for p in plan.params] == \
        [w.shape for w in net.weights]
    params = [np.asarray(w, np.float64) if p['layout'] == S.WL_CONV
              else S.keras_to_canonical(w, p['layout']).astype(np.float64)
              for w, p in zip(net.weights, plan.params)]
    inputs = {'x': x}
    inputs.update(exo or {})
    y = run_plan(plan, params, inputs)
    # ConvT canonical arrays went through float32
    np.testing.assert_allclose(y, y_ref, rtol=0,
                               atol=5e-6 * max(1.0, np.abs(y_ref).max()))
    if fuse and 'gen_' in rel:
        assert not any(op['kind'] in (S.OP_PAD, S.OP_CROP)
                       for op in plan.ops)


# ---------------------------------------------------------------- depth_to_time
def _d2t_literal(x, m, roll):
    """phygnn SpatioTemporalExpansion(temporal_method='depth_to_time'):
    ``tf.reshape(x, (n, s1, s2, t * m, c // m))`` then ``tf.roll(x, t_roll,
    axis=3)`` — out[..., (t m + j + roll) mod (T m), c'] = in[..., t,
    j (c / m) + c']"""
    n, s1, s2, t, c = x.shape
    out = np.empty((n, s1, s2, t * m, c // m), x.dtype)
    for ti in range(t):
        for j in range(m):
            out[:, :, :, (ti * m + j + roll) % (t * m)] = \
                x[:, :, :, ti, j * (c // m):(j + 1) * (c // m)]
    return out


D2T = [(4, 0), (4, 2), (8, 4), (3, 17), (6, -5), (2, 12)]   # (mult, t_roll)


@pytest.mark.parametrize('m,roll', D2T)
def test_depth_to_time_oracle_and_plan_on_integers(m, roll):
    spec = [{'class': 'SpatioTemporalExpansion', 'temporal_mult': m,
             'temporal_method': 'depth_to_time', 't_roll': roll}]
    shape = (2, 3, 4, 3, 2 * m)
    x = np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)
    want = _d2t_literal(x, m, roll)
    net = OracleNet(spec)
    y = net.forward(x)
    np.testing.assert_array_equal(y, want)
    plan = S.build_plan(S.parse_layers(spec), shape)
    kinds = [op['kind'] for op in plan.ops]
    assert kinds[0] == S.OP_VIEW
    assert (S.OP_ROLL_T in kinds) == (roll % (shape[3] * m) != 0)
    np.testing.assert_array_equal(run_plan(plan, [], {'x': x}), want)
    # adjoint: <dy, f(x)> == <f^T(dy), x>, and f^T f = identity (permutation)
    dy = np.arange(want.size, dtype=np.float64).reshape(want.shape)[::-1] + 1
    dx = net.backward(dy)
    assert dx.shape == x.shape
    assert float((dy * want).sum()) == float((dx * x).sum())
    np.testing.assert_array_equal(net.backward(want), x)


def test_depth_to_time_needs_divisible_channels():
    spec = [{'class': 'SpatioTemporalExpansion', 'temporal_mult': 4,
             'temporal_method': 'depth_to_time'}]
    with pytest.raises(RuntimeError, match='divisible by the temporal'):
        S.build_plan(S.parse_layers(spec), (1, 3, 3, 2, 6))
    with pytest.raises(KeyError, match='no kernel mapping'):
        S.build_plan(S.parse_layers([
            {'class': 'SpatioTemporalExpansion', 'temporal_mult': 2,
             'temporal_method': 'bilinear'}]), (1, 3, 3, 2, 6))


PAD_CROP = [
    # sup3rcc/gen_wind_1x_24x_6f head: pad 2 / crop 1
    ([2, 2, 2], 1, (2, 5, 6, 4, 3)),
    # sup3rcc/gen_solar_1x_8x_1f: pad [3, 3, 2] / crop [2, 2, 1]
    ([3, 3, 2], [2, 2, 1], (2, 6, 5, 3, 3)),
    # asymmetric leftover: pad 3 / crop [2, 1, 2] grows s2 by 2
    ([3, 3, 3], [2, 1, 2], (1, 5, 4, 4, 2)),
]


@pytest.mark.parametrize('pad,crop,shape', PAD_CROP)
@pytest.mark.parametrize('fuse', [True, False])
def test_pad_crop_variants_plan_matches_oracle(pad, crop, shape, fuse):
    from sup3r_amd.configs.author_configs import pcc
    spec = pcc(3, 5, pad=pad, crop=crop) + pcc(3, 4, pad=pad, crop=crop,
                                               act=False)
    rng = np.random.default_rng(3)
    x = rng.standard_normal(shape)
    net = OracleNet(spec)
    net.init_weights(x, seed=1, bias_scale=0.1)
    net.cast(np.float64)
    y_ref = net.forward(x)
    plan = S.build_plan(S.parse_layers(spec), shape, fuse=fuse)
    y = run_plan(plan, [np.asarray(w, np.float64) for w in net.weights],
                 {'x': x})
    np.testing.assert_allclose(y, y_ref, rtol=0, atol=1e-12)


# ------------------------------------------------------------------------ GPU
def _fwd_bwd(spec, shape, precision, seed, tol_y, tol_g, exo_name=None):
    from tests.test_parity_r02 import _fwd_bwd_vs_oracle
    exo_shape = None
    if exo_name:
        plan = S.build_plan(S.parse_layers(spec), shape)
        exo_shape = _exo_for(plan, exo_name, np.random.default_rng(0),
                             np.float32)[exo_name].shape
    return _fwd_bwd_vs_oracle(spec, shape, precision, seed, tol_y, tol_g,
                              exo_name=exo_name, exo_shape=exo_shape)


@pytest.mark.gpu
@pytest.mark.parametrize('rel', sorted(CASES))
def test_surface_forward_backward_fp32(rel):
    shape, exo_name = CASES[rel]
    _fwd_bwd(load_surface(rel), shape, 'f32', 41, 1e-4, 1e-3, exo_name)


# sup3rcc/gen_wind_1x_24x_6f is the one shipped generator WITHOUT residual
# connections: 37 convolutions in series.  Its forward passes the same per-op
# (teacher-forced) check as every other spec; the backward pass cannot be
# teacher-forced, and with no identity path to carry the gradient around a
# layer every bf16 rounding of dPre is amplified by all the layers upstream
# of it: the worst weight gradient sits 2.9e-2 / 2.6e-2 / 6.1e-2 (seeds 43 /
# 44 / 45; profile: ~1e-7 at the output conv, growing to the middle of the
# stack) from the fp32 oracle on the device's activations and masks, against
# <= 2e-2 for the residual nets built from the same kernels.  fp32 plans of
# this spec meet 1e-3 (test above), which pins the plumbing.
BF16_GRAD_TOL = {'sup3rcc/gen_wind_1x_24x_6f.json': 1e-1}


@pytest.mark.gpu
@pytest.mark.parametrize('rel', sorted(CASES))
def test_surface_forward_backward_bf16(rel):
    shape, exo_name = CASES[rel]
    _fwd_bwd(load_surface(rel), shape, 'bf16', 43, 3e-2,
             BF16_GRAD_TOL.get(rel, 2e-2), exo_name)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(1, 5, 4, 3, 6), (1, 12, 8, 3, 6)])
def test_no_residual_stack_bf16_backward_segment_by_segment(shape):
    """sup3rcc/gen_wind_1x_24x_6f in bf16 (the spec whose end-to-end gradient
    bound is ``BF16_GRAD_TOL`` = 1e-1): the backward kernels of EVERY layer
    at the usual 2e-2, by cutting the 37-conv stack into overlapping segments
    of 6 fused ops at the shapes the full plan gives them — each segment is a
    network of its own with a fresh output gradient, so no rounding of dPre is
    amplified by more than five layers.  Segments overlap by one op (the first
    op of a segment reads an fp32 plan input instead of the previous layer's
    bf16 cells: it may select other kernels and is the one not counted), and
    every counted op must run on the kernels the full plan selects for it —
    asserted through ``s3_plan_op_info`` (forward / weight gradient / data
    gradient)."""
    from oracle.network import expand_repeats
    from sup3r_amd.engine import Network
    from tests.test_parity_r02 import _fwd_bwd_vs_oracle
    rel = 'sup3rcc/gen_wind_1x_24x_6f.json'
    layers = expand_repeats(load_surface(rel)['hidden_layers'])
    plan = S.build_plan(S.parse_layers(layers), shape)
    assert len(plan.layer_out) == len(layers)
    ends = [li for li, (_, oi) in enumerate(plan.layer_out)
            if oi >= 0 and (li + 1 == len(layers) or
                            plan.layer_out[li + 1][1] != oi)]
    op_of_end = [plan.layer_out[li][1] for li in ends]
    assert op_of_end == sorted(set(op_of_end)) and len(ends) >= 37
    full = Network(layers, precision='bf16')
    full.build(shape, seed=0)
    phf = full.plan(shape, training=True)
    kinds = {oi: tuple(phf.op_info(oi)[f] for f in ('fwd', 'wgrad', 'dgrad'))
             for oi, op in enumerate(phf.plan.ops) if op['kind'] == S.OP_CONV}
    del phf
    full.clear_plans()
    seg, counted, worst = 6, set(), 0.0
    k = 0
    while k < len(ends):
        a = ends[k - 1] + 1 if k else 0            # first layer of the segment
        b = ends[min(k + seg, len(ends)) - 1]      # its last layer
        sub = layers[a:b + 1]
        in_shape = tuple(shape) if k == 0 else \
            tuple(plan.layer_out_shapes[a - 1])
        ph = _fwd_bwd_vs_oracle(sub, in_shape, 'bf16', 400 + k, 3e-2, 2e-2)
        sub_ops = [oi for oi, op in enumerate(ph.plan.ops)]
        first_full = op_of_end[k]
        for j in sub_ops:
            if ph.plan.ops[j]['kind'] != S.OP_CONV:
                continue
            got = tuple(ph.op_info(j)[f] for f in ('fwd', 'wgrad', 'dgrad'))
            want = kinds[first_full + j]
            if j == 0 and k > 0:
                continue                           # (fp32 input: not counted)
            # (the first op of the NETWORK has no data gradient in the full
            # plan's selection either way)
            assert got == want, (k, j, got, want)
            counted.add(first_full + j)
        del ph
        if b == ends[-1]:
            break
        k += seg - 1
    assert counted == set(kinds), sorted(set(kinds) - counted)


@pytest.mark.gpu
@pytest.mark.parametrize('rel', sorted(c for c in CASES if 'gen_' in c))
def test_surface_forward_bf16x3_meets_the_fp32_tolerance(rel):
    """the mode that owns north_star's L-inf < 1e-3: every shipped generator"""
    from tests.helpers import rel_linf
    from tests.test_parity_r02 import _hip, _oracle
    shape, exo_name = CASES[rel]
    spec = load_surface(rel)
    rng = np.random.default_rng(47)
    x = rng.standard_normal(shape).astype(np.float32)
    plan = S.build_plan(S.parse_layers(spec), shape)
    exo = _exo_for(plan, exo_name, rng, np.float32) if exo_name else None
    ref = _oracle(spec, x, exo, seed=47)
    y_ref = ref.forward(x, exo)
    net = _hip(spec, ref.weights, 'bf16x3')
    dev = net.dev
    ph = net.plan(shape, training=False)
    y = ph.forward(dev.to_device(x), {k: dev.to_device(v) for k, v in
                                      (exo or {}).items()}).cpu().numpy()
    assert rel_linf(y, y_ref) < 1e-3, rel_linf(y, y_ref)


@pytest.mark.gpu
@pytest.mark.parametrize('m,roll', D2T)
def test_depth_to_time_device_is_exact_on_integers(m, roll):
    """S3_OP_VIEW + S3_OP_ROLL_T forward and adjoint, bit-exact (integers
    below 2^24 are exact in fp32); 16-byte and scalar channel paths (C / m =
    2 and 4)"""
    from sup3r_amd.engine import Network
    for cmul in (2, 4):
        spec = [{'class': 'SpatioTemporalExpansion', 'temporal_mult': m,
                 'temporal_method': 'depth_to_time', 't_roll': roll}]
        shape = (2, 3, 4, 3, cmul * m)
        x = np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape)
        want = _d2t_literal(x, m, roll)
        for prec in ('f32', 'bf16'):
            if prec == 'bf16' and x.max() >= 256:
                # bf16 storage: integers below 2^8 only
                x_ = np.mod(x, 251.0).astype(np.float32)
                want_ = _d2t_literal(x_, m, roll)
            else:
                x_, want_ = x, want
            net = Network(spec, precision=prec)
            dev = net.dev
            ph = net.plan(shape, training=True)
            y = ph.forward(dev.to_device(x_)).cpu().numpy()
            np.testing.assert_array_equal(y, want_)
            dy = np.mod(np.arange(want.size, dtype=np.float32)[::-1] * 7,
                        241.0).reshape(want.shape)
            dx = ph.backward(dev.to_device(dy), need_dx=True).cpu().numpy()
            ref = OracleNet(spec)
            ref.forward(x_)
            np.testing.assert_array_equal(dx.reshape(shape), ref.backward(dy))


@pytest.mark.gpu
@pytest.mark.parametrize('m,roll', [(4, 2), (8, 4), (3, 17), (6, -5)])
def test_depth_to_time_between_convolutions(m, roll):
    """conv -> depth_to_time (+ roll) -> LeakyReLU -> conv, forward and every
    gradient: fp32 at 1e-4 / 1e-3, and on 64-channel MFMA convs in bf16"""
    from sup3r_amd.configs.author_configs import pcc
    tail = [{'class': 'SpatioTemporalExpansion', 'temporal_mult': m,
             'temporal_method': 'depth_to_time', 't_roll': roll},
            {'alpha': 0.2, 'class': 'LeakyReLU'}]
    spec = pcc(3, 8) + pcc(3, 3 * m, act=False) + tail + pcc(3, 2, act=False)
    _fwd_bwd(spec, (2, 5, 6, 4, 3), 'f32', 5, 1e-4, 1e-3)
    spec = pcc(3, 64) + pcc(3, 64, act=False, pad=[3, 3, 2],
                            crop=[2, 2, 1]) + \
        pcc(3, 16 * m, act=False) + tail + pcc(3, 2, act=False)
    _fwd_bwd(spec, (2, 6, 5, 4, 4), 'bf16', 5, 3e-2, 2e-2)


@pytest.mark.gpu
@pytest.mark.parametrize('pad,crop,shape', PAD_CROP)
def test_pad_crop_variants_device(pad, crop, shape):
    from sup3r_amd.configs.author_configs import pcc
    spec = pcc(3, 5, pad=pad, crop=crop) + pcc(3, 4, pad=pad, crop=crop,
                                               act=False)
    _fwd_bwd(spec, shape, 'f32', 9, 1e-4, 1e-3)
    spec = pcc(3, 64, pad=pad, crop=crop) + pcc(3, 64, pad=pad, crop=crop) + \
        pcc(3, 4, pad=pad, crop=crop, act=False)
    _fwd_bwd(spec, shape, 'bf16', 9, 3e-2, 2e-2)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(8, 54, 54, 3, 3), (16, 54, 54, 6, 3)])
def test_few_time_step_trunk_trains_at_batches_that_fill_the_persistent_dgrad(shape):
    """sup3rcc/gen_solar_1x_8x_1f (a 64-channel trunk over 3 time steps) at batch sizes whose
    padded frames have enough tiles for conv3_mfma_persist_kernel's data gradient: until the
    end of round 6 that kernel was selected there (its forward twin excludes fewer than 8 time
    steps, the data gradient did not) and the step produced non-finite gradients at 8 samples
    and a memory access fault at 16.  The gradients must be finite, the persistent data
    gradient unused, and the result that of the plan with it switched off."""
    from sup3r_amd.engine import Network
    from tests.helpers import switch
    spec = load_surface('sup3rcc/gen_solar_1x_8x_1f.json')
    rng = np.random.default_rng(3)
    x = rng.standard_normal(shape).astype(np.float32)

    def run():
        net = Network(spec, precision='bf16')
        net.build(shape, seed=2)
        ph = net.plan(shape, training=True)
        n0 = net.dev.stat('persist_dgrad')
        y = ph.forward(net.dev.to_device(x))
        dy = net.dev.to_device(
            np.random.default_rng(4).standard_normal(tuple(y.shape)).astype(np.float32))
        ph.backward(dy, need_dx=False)
        g = [np.array(a) for a in net.grads]
        used = net.dev.stat('persist_dgrad') - n0
        del ph
        net.clear_plans()
        return g, used
    g1, used1 = run()
    assert used1 == 0
    assert all(np.isfinite(a).all() for a in g1)
    switch('NO_PERSIST_DGRAD', 1)
    g0, _ = run()
    switch('NO_PERSIST_DGRAD', None)
    for a, b in zip(g1, g0):
        np.testing.assert_array_equal(a, b)
