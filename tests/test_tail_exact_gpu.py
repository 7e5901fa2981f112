"""The generator's hi-res tail conv, bit for bit: the five forward kernels
(conv_tail_mfma_kernel<false> / <true>, conv_tail_slide_kernel,
conv_tail_sweep_kernel<1 / 2 / 3>, conv_tail_x3_kernel), the weight gradients
(conv_wgrad_tail_kernel<false / true>, conv_wgrad_tail_sweep_kernel,
conv_wgrad_c2_kernel<8> below the position floor) and the few-channel data
gradient over the padded frame, behind the expansion conv and its
depth-to-space store, at the edges of their tiles, planes and selection
predicates, each against the float64 reference of the same stack
(tests/support_ref.py).

The tail filter is dense (+-1 in every entry), its cells are multiples of 0.25
and d_out sits on a sparse lattice, so no sum depends on its order and the
comparison is ``assert_array_equal``: a wrong tap, plane, band row or ring slot
is a wrong integer at a coordinate the failure names.  The cases, their data
and the conditions that make this valid live in tests/tail_exact_cases.py and
are checked in the CPU suite (tests/test_tail_exact_ref_cpu.py);
profiles/tail_exact/NOTES.md has the table.

Each case asserts from ``op_info`` the kernels and the bf16 / fp32 tensors of
the expansion conv and of the tail conv, and from the launch counters which
tail variant ran and that its siblings did not."""
import numpy as np
import pytest

from tests import tail_exact_cases as T
from tests.test_train_support_gpu import _assert_exact, _clean, _cu, _run

pytestmark = pytest.mark.gpu


def _infer(spec, shape, weights, x, precision, options, counters):
    """forward of a fresh inference plan -> (y, counter deltas, op infos)"""
    from sup3r_amd.engine import Network
    net = Network(_clean(spec), precision=precision)
    net.set_weights(weights)
    ph = net.plan(shape, training=False, options=options)
    dev = net.dev
    before = {k: dev.stat(k) for k in counters}
    y = ph.forward(dev.to_device(x))
    dev.sync()
    y = y.cpu().numpy()
    used = {k: dev.stat(k) - v for k, v in before.items()}
    info = [ph.op_info(i) for i in range(len(ph.plan.ops)) if ph.plan.ops[i]['kind'] == 1]    # (OP_CONV)
    del ph
    net.clear_plans()
    return y, used, info


def first_difference(got, ref, names):
    """'' or the first coordinate at which a tensor differs from its reference, with both values"""
    for what, a, b in zip(names, got, ref):
        ne = np.argwhere(np.asarray(a) != np.asarray(b))
        if len(ne):
            at = tuple(int(v) for v in ne[0])
            return f' — {len(ne)} of {a.size} elements of {what} differ, the first at {what}{list(at)}: {a[at]}, expected {b[at]}'
    return ''


def check_selection(case, cu, used, info):
    """-> the list of what did not run where the case says it must"""
    want_info, want_used = T.expected(case, cu)
    bad = []
    for i, want in want_info.items():
        for k, v in want.items():
            if info[i][k] != v:
                bad.append(f'conv {i} {k}: {info[i][k]}, expected {v}')
    for k, n in want_used.items():
        if used[k] != n:
            bad.append(f'counter {k}: {used[k]}, expected {n}')
    return bad


@pytest.mark.parametrize('name', list(T.CASES))
def test_tail_conv_stack_is_exact(name):
    cu = _cu()
    case, shape, data = T.build(name, cu)      # (asserts the exactness conditions on the reference)
    y_ref, dx_ref, g_ref = data['ref']
    opts = case['options'] or None
    if case['training']:
        got = _run(case['spec'], shape, list(data['w']), data['x'], data['d_out'], precision=case['precision'],
                   options=opts, counters=T.COUNTERS, backwards=case['backwards'])
        used, info = got[3], got[4]
    else:
        y, used, info = _infer(case['spec'], shape, list(data['w']), data['x'], case['precision'], opts, T.COUNTERS)
    print(name, shape, case['precision'], 'training' if case['training'] else 'inference',
          [(i['fwd'], i['dgrad'], i['wgrad'], i['in16'], i['out16']) for i in info], {k: v for k, v in used.items() if v})
    bad = check_selection(case, cu, used, info)
    assert not bad, bad
    if case['training']:
        scale = float(case['backwards'])
        where = first_difference([got[0], got[1]] + list(got[2]), [y_ref, dx_ref] + [scale * g for g in g_ref],
                                 ['y', 'dx'] + [f'gradient #{i} ' for i in range(len(g_ref))])
        _assert_exact(got[:3], (y_ref, dx_ref, g_ref), name + where, scale=scale)
        assert np.abs(got[1]).max() > 0
    else:
        np.testing.assert_array_equal(y, y_ref, err_msg=f'{name}: forward' + first_difference([y], [y_ref], ['y']))
