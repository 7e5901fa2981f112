"""The reference side of tests/test_disc_exact_gpu.py, on the CPU: every case's
data and float64 reference are built here (CU-dependent shapes for a nominal
256 CUs), which asserts the exactness conditions of tests/disc_exact_cases.py —
no case reaches a device with a tensor that does not survive bf16 or a sum that
could round."""
import numpy as np
import pytest

from tests import disc_exact_cases as D


@pytest.mark.parametrize('name', sorted({c['ref'] for c in D.CASES.values()}))
def test_reference_meets_the_exactness_conditions(name):
    case, shape, data = D.build(name)
    y, dx, grads = data['ref']
    assert y.shape == D.out_shape(case['spec'], shape) and dx.shape == shape
    # the case is no trivial one: every tensor compared has non-zero entries
    assert np.abs(y).max() > 0 and np.abs(dx).max() > 0 and all(np.abs(g).max() > 0 for g in grads)
    n_pos = max(int(np.prod(shape[:4])), int(np.prod(y.shape[:4])))
    print(name, shape, 'positions', n_pos, 'max |y|', np.abs(y).max(), 'max |dx|', np.abs(dx).max())
    assert n_pos <= 300_000, 'keep the float64 reference quick'


def test_every_leg_shares_the_data_of_its_base_case():
    for name, case in D.CASES.items():
        base = D.CASES[case['ref']]
        assert base['ref'] == case['ref'] and D._clean(base['spec']) == D._clean(case['spec']), name
        assert D.shape_of(case) == D.shape_of(base), name


@pytest.mark.parametrize('cu', [64, 256, 304])
def test_many_tile_shapes_exceed_the_cu_count_with_unequal_xcd_shares(cu):
    for name, per, tile in (('front_many_tiles', 18, (2, 4, 16)), ('back_many_tiles', 30, (2, 2, 16))):
        case = D.CASES[name]
        shape = D.shape_of(case, cu)
        # the stride-2 conv (the second) of the stack: its output tiles
        two = [s for s in case['spec'] if s['class'] == 'Conv3D'][:2]
        o = D.out_shape(two, shape)
        tiles = shape[0] * D._tiles(o[1:4], tile)
        assert D._tiles(o[1:4], tile) == per and tiles > cu and tiles % 8 != 0, (name, cu, tiles)
