"""The discriminator's conv kernels, bit for bit: the hand-indexed LDS-halo
kernels (conv_halo_s2_kernel and its 64-channel split, conv_halo32_kernel,
gconv_fewch_halo_kernel with its sign bytes, conv_dgrad_s2_kernel with the
bf16-only store, conv_dgrad_c2_kernel and its sliding-window form,
conv_wgrad_c2_kernel, conv_wgrad_bf16_gen, the valid-padding forms of the
halo-tile kernel) and the gather kernel they fall back to (gconv_mfma_kernel
forward / adjoint, split-K), at the edges of their tiles and of their selection
predicates, each against the float64 reference of the same stack
(tests/support_ref.py).

Every value of a case is a small integer times a power of two and every filter
one +-1 per output channel, so each output is ONE input cell (plus a bias), no
sum depends on its order and the comparison is ``assert_array_equal``: a wrong
tap, row, swizzle key, parity class, K pass or store permutation is a wrong
integer.  The cases, their data and the conditions that make this valid live in
tests/disc_exact_cases.py and are checked in the CPU suite
(tests/test_disc_exact_ref_cpu.py); profiles/disc_exact/NOTES.md has the table.

Each case asserts from ``op_info`` that the conv it is named for ran on the
kernel it is named for, and from the launch counters which in-family variant
did (64-channel split, LDS-halo walk of the few-channel conv, sign bytes,
bf16-only store, persistent data gradient, sliding window, split-K)."""
import numpy as np
import pytest

from tests import disc_exact_cases as D
from tests.test_train_support_gpu import _assert_exact, _cu, _run

pytestmark = pytest.mark.gpu


def check_selection(case, used, info):
    """-> the list of what did not run where the case says it must"""
    bad = []
    for i, want in case['kernels'].items():
        for k, v in want.items():
            if info[i][k] != v:
                bad.append(f'conv {i} {k}: {info[i][k]}, expected {v}')
    for i, want in case['io'].items():
        for k, v in want.items():
            if info[i][k] != v:
                bad.append(f'conv {i} {k}: {info[i][k]}, expected {v}')
    for k, n in case['counters'].items():
        if (used[k] <= 0) if n == '>0' else (used[k] != n):
            bad.append(f'counter {k}: {used[k]}, expected {n}')
    return bad


def run_case(name):
    case, shape, data = D.build(name, _cu())      # (asserts the exactness conditions on the reference)
    got = _run(case['spec'], shape, list(data['w']), data['x'], data['d_out'], precision=case['precision'],
               options=case['options'], counters=D.COUNTERS)
    used, info = got[3], got[4]
    print(name, shape, case['precision'], [(i['fwd'], i['dgrad'], i['wgrad'], i['in16'], i['out16']) for i in info],
          {k: v for k, v in used.items() if v})
    return case, got, data['ref'], check_selection(case, used, info)


@pytest.mark.parametrize('name', list(D.CASES))
def test_discriminator_conv_stack_is_exact(name):
    case, got, ref, bad = run_case(name)
    assert not bad, bad
    _assert_exact(got[:3], ref, name)
    assert np.abs(got[1]).max() > 0
