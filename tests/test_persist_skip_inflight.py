"""The skip-prefetch variant of the persistent trunk conv keeps eight
hand-issued 16-B loads per lane in flight across its last tap
(kernels_conv_mfma_persist.hip, ``SKP``).  The compiler's waitcnt pass sees
neither the loads nor the one ``s_waitcnt vmcnt(0)`` behind tap 26:
``tools/check_skip_prefetch.py`` walks the control-flow graph of the compiled
kernel and finds every instruction between a load and that wait that names
the load's destination registers (a register-allocator copy, a spill or an
early use would move a value that has not arrived)."""
import os
import shutil
import subprocess
import sys

import pytest


def test_skip_rows_in_flight_are_not_touched():
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    root = os.path.join(os.path.dirname(__file__), '..')
    out = subprocess.run([sys.executable, os.path.join(root, 'tools', 'check_skip_prefetch.py')],
                         capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, HIPCC=hipcc))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert '1 kernels, 8 skip-row loads, 0 problems' in out.stdout, out.stdout
