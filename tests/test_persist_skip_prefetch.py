"""The skip-prefetch variant of the persistent trunk conv
(``conv3_mfma_persist_kernel<4, false, 0, false, false, 8, SKP = true>``): a
plain 64 -> 64 conv that adds a bf16 skip tensor requests its residual rows
before its last tap, runs that tap in a form with fewer live fragments and
waits once behind it.  Every accumulator receives the same MFMA sequence as in
the other variant, so the plan's output must be bit-identical with the variant
switched off (``NO_PERSIST_SKIPPRE``).

Plan: head conv, one residual block (pad, conv, crop, LeakyReLU, pad, conv,
crop, SkipConnection), tail conv; bf16 inference; ``PERSIST_MIN_TILES=1`` so
that the small shapes take the persistent kernel at all.
The teacher-forced oracle check runs on a training plan of two such blocks.
"""
import numpy as np
import pytest

from tests.helpers import switch

pytestmark = pytest.mark.gpu

# lo-res shapes (N, s0, s1, t) after the head conv
SHAPES = [
    (1, 4, 8, 16),      # one tile, both the first and the last of its workgroup
    (1, 6, 10, 24),     # a half-row item with an idle row pair, masked columns, ragged t
    (10, 16, 16, 64),   # 320 tiles on 256 CUs: 2 - 3 items per workgroup, the
                        # residual base changes across a sample boundary
]
FEATURES = 4
ARMS = {'skippre': {}, 'plain': {'NO_PERSIST_SKIPPRE': 1}, 'tile': {'NO_PERSIST': 1}}


def _spec():
    from sup3r_amd.configs.author_configs import pcc
    return pcc(3, 64) + [{'class': 'SkipConnection', 'name': 'a'}] + \
        pcc(3, 64) + pcc(3, 64, act=False) + \
        [{'class': 'SkipConnection', 'name': 'a'}] + pcc(3, 2, act=False)


_cache = {}


def _run(lo, arm):
    """output of the plan under one arm's options, computed once per (shape, arm);
    also what the plan and the launch counter reported"""
    key = (lo, arm)
    if key in _cache:
        return _cache[key]
    from sup3r_amd.engine import Network
    shape = tuple(lo) + (FEATURES,)
    x = np.random.default_rng(23).standard_normal(shape).astype(np.float32)
    switch('PERSIST_MIN_TILES', 1)
    for k, v in ARMS[arm].items():
        switch(k, v)
    try:
        net = Network(_spec(), precision='bf16')
        net.build(shape, seed=4)
        ph = net.plan(shape, training=False)
        infos = [ph.op_info(i) for i in range(len(ph.plan.ops))]
        n0 = net.dev.stat('persist_skippre')
        y = ph.forward(net.dev.to_device(x)).cpu().numpy()
        launched = net.dev.stat('persist_skippre') - n0
        net.clear_plans()
    finally:
        for k in ARMS[arm]:
            switch(k, None)
        switch('PERSIST_MIN_TILES', None)
    y.setflags(write=False)
    _cache[key] = (y, infos, launched)
    return _cache[key]


def _skip_convs(infos):
    return [d for d in infos if d['fwd'] == 'mfma_persist' and d['res16']]


@pytest.mark.parametrize('lo', SHAPES)
def test_skip_variant_runs_and_equals_the_plain_variant(lo):
    y, infos, launched = _run(lo, 'skippre')
    assert len(_skip_convs(infos)) == 1, infos     # the skip conv is on the persistent kernel
    assert launched == 1, launched                 # ... and on the skip-prefetch variant
    y0, infos0, launched0 = _run(lo, 'plain')
    assert len(_skip_convs(infos0)) == 1, infos0
    assert launched0 == 0, launched0
    assert np.isfinite(y0).all() and np.abs(y0).max() > 0
    print('skippre vs plain: %d of %d values differ, max |d| %.3e'
          % (int((y != y0).sum()), y.size, float(np.abs(y - y0).max())))
    assert np.array_equal(y, y0)


@pytest.mark.parametrize('lo', SHAPES)
def test_skip_variant_equals_the_tile_kernel(lo):
    y, _, launched = _run(lo, 'skippre')
    assert launched == 1, launched
    yt, infos, _ = _run(lo, 'tile')
    assert not [d for d in infos if d['fwd'] == 'mfma_persist'], infos
    print('skippre vs NO_PERSIST: %d of %d values differ, max |d| %.3e'
          % (int((y != yt).sum()), y.size, float(np.abs(y - yt).max())))
    assert np.array_equal(y, yt)


def test_skip_variant_within_the_teacher_forced_oracle_bound():
    """teacher-forced per-op forward, 3e-2 end to end, gradients <= 2e-2
    (tests/test_hip_parity.py::_tight_vs_oracle).  That check reads every
    activation, so it needs a TRAINING plan; a bf16 training plan runs the
    inference trunk forward when the trunk tensors stay bf16: two residual
    blocks and one more trunk conv (the skip tensor of the second block is
    the sum leaving the first, its output feeds a trunk conv: both bf16
    tensors; the head conv's output is kept in fp32) at 2 x 9 x 10 x 37 =
    6660 positions, ragged in every axis (the bf16 weight gradient starts at
    2048).  The second block's skip conv is then the skip-prefetch launch."""
    from sup3r_amd.configs.author_configs import pcc
    from sup3r_amd.engine import Device, Network
    from tests.test_hip_parity import _tight_vs_oracle

    def block(name):
        return [{'class': 'SkipConnection', 'name': name}] + pcc(3, 64) + \
            pcc(3, 64, act=False) + [{'class': 'SkipConnection', 'name': name}]
    # (the sum leaving block c feeds a trunk conv, so it stays a bf16 tensor too)
    spec = pcc(3, 64) + block('b') + block('c') + pcc(3, 64) + pcc(3, 2, act=False)
    shape = (2, 9, 10, 37, FEATURES)
    switch('PERSIST_MIN_TILES', 1)
    try:
        net = Network(spec, precision='bf16')
        net.build(shape, seed=4)
        ph = net.plan(shape, training=True)
        infos = [ph.op_info(i) for i in range(len(ph.plan.ops))]
        net.clear_plans()
        kinds = [(d['fwd'], d['in16'], d['out16'], d['res16']) for d in infos]
        assert len(_skip_convs(infos)) >= 1, kinds
        n0 = Device.get().stat('persist_skippre')
        _tight_vs_oracle(spec, shape, 7)
        launched = Device.get().stat('persist_skippre') - n0
        print('skip-prefetch launches under the teacher-forced check: %d' % launched)
        assert launched >= 1, launched
    finally:
        switch('PERSIST_MIN_TILES', None)


def test_skip_variant_within_the_oracle_bound_end_to_end():
    """the inference plan on the skip-prefetch variant against the oracle on
    the same weights: 3e-2 of the largest value, the bf16 mode's end-to-end
    bound (tests/test_hip_parity.py)"""
    from oracle.network import Network as OracleNet
    from sup3r_amd.engine import Network
    shape = SHAPES[1] + (FEATURES,)
    x = np.random.default_rng(29).standard_normal(shape).astype(np.float32)
    ref = OracleNet(_spec())
    ref.init_weights(x, seed=7, bias_scale=0.1)
    y_ref = ref.forward(x)
    switch('PERSIST_MIN_TILES', 1)
    try:
        net = Network(_spec(), precision='bf16')
        net.set_weights(ref.weights)
        ph = net.plan(shape, training=False)
        n0 = net.dev.stat('persist_skippre')
        y = ph.forward(net.dev.to_device(x)).cpu().numpy()
        assert net.dev.stat('persist_skippre') == n0 + 1
        net.clear_plans()
    finally:
        switch('PERSIST_MIN_TILES', None)
    err = float(np.abs(y - y_ref).max() / max(1.0, np.abs(y_ref).max()))
    print('skippre vs oracle: rel. L-inf %.3e' % err)
    assert err < 3e-2, err
