"""-m gpu: the dihedral entries under CONP_GUARD=1 in a fresh child process (as tests/test_gpu_bonded_guard.py): every device buffer
of the library sits between two zones of a known byte pattern, and no kernel of conp_dihedral.hip stores outside its buffers."""
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
import dihedral_ref as dr
import test_gpu_dihedral as td
from conp_amd import capi
lib = capi.load_library()
lib.conp_debug_check_guards.restype = int
assert lib.conp_debug_check_guards() == 0, "guard zones are off"
for c in dr.gpu_cases():             # every case of tests/test_gpu_dihedral.py
    td.run_case(c)
    bad = lib.conp_debug_check_guards()
    assert bad == 0, (c.tag, bad, lib.conp_last_error().decode())
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
