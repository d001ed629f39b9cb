"""-m gpu: the conp_efield_* and conp_observe_* entries under CONP_GUARD=1 in a fresh child process (as tests/test_gpu_shake_guard.py):
every device buffer of the library sits between two zones of a known byte pattern, and no kernel of conp_efield.hip stores outside
its buffers -- over the edge sizes of the ladder of both entries, the 16-group case and the coupled case."""
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
import field_ref as fr
import test_gpu_efield as te
import test_gpu_observe as to
from conp_amd import capi
lib = capi.load_library()
lib.conp_debug_check_guards.restype = int
assert lib.conp_debug_check_guards() == 0, "guard zones are off"
for n in (1, fr.B - 1, fr.B, fr.B + 1, fr.BIG):
    te.test_every_block_edge(n)
    bad = lib.conp_debug_check_guards()
    assert bad == 0, ("efield", n, bad, lib.conp_last_error().decode())
    for shape in ("one", "sixteen"):
        to.test_every_block_edge_per_group_shape(shape, n)
        bad = lib.conp_debug_check_guards()
        assert bad == 0, ("observe", shape, n, bad, lib.conp_last_error().decode())
to.test_sixteen_groups_and_every_atom_in_all_of_them(fr.B + 1)
te.test_the_field_follows_the_fix_scalar_of_the_same_update("conq")
bad = lib.conp_debug_check_guards()
assert bad == 0, ("sixteen groups, coupled", bad, lib.conp_last_error().decode())
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
