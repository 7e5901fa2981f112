"""The reference side of tests/test_tail_exact_gpu.py, on the CPU: every case's
data and float64 reference are built here (CU-dependent shapes for a nominal
256 CUs), which asserts the exactness and slot-coverage conditions of
tests/tail_exact_cases.py — no case reaches a device with a tensor that does
not survive bf16, a sum that could round or a filter slot nothing shows."""
import numpy as np
import pytest

from tests import tail_exact_cases as T


@pytest.mark.parametrize('name', sorted({c['ref'] for c in T.CASES.values()}))
def test_reference_meets_the_exactness_conditions(name):
    case, shape, data = T.build(name)
    y, dx, grads = data['ref']
    assert y.shape == (shape[0],) + case['hi'] + (case['cout'],) and np.abs(y).max() > 0
    if not case['training']:       # (a forward-only base: no training plan reaches its shape with bf16 cells)
        assert T.positions(case) < T.TAIL_FLOOR and dx is None and grads is None
        return
    # the case is no trivial one: every tensor compared has non-zero entries
    assert dx.shape == shape and np.abs(dx).max() > 0 and all(np.abs(g).max() > 0 for g in grads)
    d = data['d_out']
    print(name, shape, 'hi-res positions', T.positions(case), 'non-zero d_out', int((d != 0).sum()), 'of', d.size,
          'lattices drawn again', data['redrawn'], 'max |y|', np.abs(y).max(), 'max |dx|', np.abs(dx).max())


def test_lattice_entries_of_a_channel_never_share_a_frame_cell():
    """two non-zero entries of one (sample, channel) differ by >= 3 along some axis"""
    d = T.lattice_d_out((3, 9, 10, 17, 4), np.random.default_rng(5))
    assert set(np.unique(d)) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    for n in range(d.shape[0]):
        for c in range(d.shape[4]):
            idx = np.argwhere(d[n, ..., c] != 0)
            assert len(idx) > 1
            gap = np.abs(idx[:, None, :] - idx[None, :, :]).max(axis=2)
            assert gap[~np.eye(len(idx), dtype=bool)].min() >= 3


def test_lattice_gaps_reports_the_residues_a_tensor_does_not_reach():
    """the check ``_lattice`` redraws on: nothing missing in a tensor that is non-zero everywhere, the nine
    residue pairs of a border that is emptied, the interior residues of a tensor lit on its borders only"""
    full = np.ones((1, 6, 7, 8, 1), np.float32)
    inner, faces = T.lattice_gaps(full)
    assert not inner and not any(faces.values())
    cut = full.copy()
    cut[:, :, :, 0] = 0                      # the border t = 0
    inner, faces = T.lattice_gaps(cut)
    assert not inner and len(faces[(2, 'lo')]) == 9 and not any(v for k, v in faces.items() if k != (2, 'lo'))
    shell = full.copy()
    shell[:, 1:-1, 1:-1, 1:-1] = 0
    inner, faces = T.lattice_gaps(shell)
    assert len(inner) == 27 and not any(faces.values())
    # an axis of extent 4 has interior positions 1, 2 only: residue 0 is not asked for there
    inner, faces = T.lattice_gaps(np.zeros((1, 4, 7, 8, 1), np.float32))
    assert len(inner) == 2 * 3 * 3 and all(len(v) == 9 for v in faces.values())


def test_every_leg_shares_the_data_of_its_base_case():
    for name, case in T.CASES.items():
        base = T.CASES[case['ref']]
        assert base['ref'] == case['ref'] and T._clean(base['spec']) == T._clean(case['spec']), name
        assert T.shape_of(case) == T.shape_of(base) and case['cout'] == base['cout'], name
        # what a leg accumulates over stays within the bound the reference was checked for
        assert case['backwards'] <= 2, name


def test_forced_plane_shapes_are_ones_the_launchers_take():
    """a forced shape the forward launcher refuses is an error, not another kernel; nset as the cases say"""
    assert [T.sweep_nset(v) for v in (T._F1, T._F2, T._F3, T._FW)] == [1, 2, 3, 1]
    assert [T.wsweep_ok(v) for v in (T._F1, T._F2, T._F3, T._FW)] == [False, True, False, True]
    for name, case in T.CASES.items():
        v = case['options'].get('TAIL_SWEEP_SHAPE')
        if v:
            assert T.sweep_nset(v) > 0 and case['cout'] == 2, name


def test_every_counter_is_expected_by_some_case():
    hit = dict.fromkeys(T.COUNTERS, 0)
    for name, case in T.CASES.items():
        info, counters = T.expected(case)
        assert set(counters) == set(T.COUNTERS)
        assert sum(counters[k] > 0 for k in T.FWD_COUNTERS) <= 1 and sum(counters[k] > 0 for k in T.WGRAD_COUNTERS) <= 1
        assert set(info[1]) >= {'fwd', 'in16', 'out16'} and set(info[0]) >= {'fwd', 'in16', 'out16'}, name
        if case['training']:
            assert set(info[1]) >= {'dgrad', 'wgrad'} and set(info[0]) >= {'dgrad', 'wgrad'}, name
        for k, v in counters.items():
            hit[k] += v > 0
    assert all(hit.values()), hit


@pytest.mark.parametrize('cu', [64, 256, 304])
def test_cu_dependent_shapes_exceed_the_cu_count(cu):
    for name, per, tile, mult in (('many_tiles_c2', 9, (4, 8, 64), 1), ('many_tiles_c3', 9, (4, 8, 32), 2),
                                  ('slide_many_units', 3, (4, 16, 64), 1)):
        case = T.CASES[name]
        units = T.batch_of(case, cu) * T._tiles(case['hi'], tile)
        assert T._tiles(case['hi'], tile) == per and units > mult * cu, (name, cu, units)
        assert T.positions(case, cu) >= T.TAIL_FLOOR
    # (the batch the CU count asks for, not the position floor, at the nominal count: unequal XCD shares)
    for name, per in (('many_tiles_c2', 9), ('many_tiles_c3', 9), ('slide_many_units', 3)):
        assert (T.batch_of(T.CASES[name]) * per) % 8 != 0, name
    # 4 x 16 planes of the forced sweep over 4 x 34 x 16: 1 x 9 x 1 units per sample
    assert T.batch_of(T.CASES['sweep_many_units'], cu) * 9 > cu
