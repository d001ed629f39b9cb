"""-m gpu: the SHAKE entries under CONP_GUARD=1 in a fresh child process (as tests/test_gpu_integrate_guard.py): every device buffer
of the library sits between two zones of a known byte pattern, and no kernel of conp_shake.hip stores outside its buffers -- over
the edge sizes of the ladder for every flag, the mixed case with setup, correct and check, and the constructed determinants."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import sys
sys.path[:0] = [{tests!r}, {pkg!r}, {oracle!r}, {root!r}]
import torch
torch.cuda.init()
import shake_ref as sr
import test_gpu_shake as ts
from conp_amd import capi
lib = capi.load_library()
lib.conp_debug_check_guards.restype = int
assert lib.conp_debug_check_guards() == 0, "guard zones are off"
for flag in (1, 3, 2):
    for n in (1, sr.BLOCK - 1, sr.BLOCK, sr.BLOCK + 1, sr.BIG):
        ts.test_every_block_edge_per_flag(flag, n)
        bad = lib.conp_debug_check_guards()
        assert bad == 0, (flag, n, bad, lib.conp_last_error().decode())
ts.test_mixed_flags_interleaved_in_one_call()
ts.test_setup_is_post_force_at_half_dtfsq_and_correct_moves_only_cluster_atoms()
ts.test_zero_and_negative_determinants_are_counted()
bad = lib.conp_debug_check_guards()
assert bad == 0, ("mixed", bad, lib.conp_last_error().decode())
print("GUARD_OK")
'''


def test_no_store_outside_the_buffers(tmp_path):
    script = tmp_path / "guard_child.py"
    script.write_text(CHILD.format(tests=os.path.join(ROOT, "tests"), pkg=os.path.join(ROOT, "lammps-user-conp2_amd"),
                                   oracle=os.path.join(ROOT, "oracle"), root=ROOT))
    env = dict(os.environ, CONP_GUARD="1")
    p = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "GUARD_OK" in p.stdout
