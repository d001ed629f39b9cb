"""-m gpu: the device list build under CONP_GUARD=1 in a fresh child process (as tests/test_gpu_pair_guard.py): every device buffer of
the library sits between two zones of a known byte pattern, and no kernel of conp_neigh.hip -- nor the pair kernels reading the list
it built -- stores outside its buffers."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import sys
sys.path[:0] = [{tests!r}, {pkg!r}, {oracle!r}, {root!r}]
import numpy as np
import torch
torch.cuda.init()
import test_gpu_pair_build_list as tb
import test_gpu_pair_device as td
import test_gpu_pair_forces as th
from conp_amd import capi
lib = capi.load_library()
lib.conp_debug_check_guards.restype = int
assert lib.conp_debug_check_guards() == 0, "guard zones are off"
flag = torch.zeros(1, dtype=torch.int32, device="cuda")
for kind, newton, special in (("small", False, True), ("small", True, False), ("sparse", True, True), ("sparse", False, False)):
    c = tb.forces_case(kind, newton, special)
    tb._same_list(kind, c.lst, c.at.nall, c.ref, c.at)
    c.fx.pair_list_moved_device(c.d_x.data_ptr(), 0.5 * c.inp.s.skin, flag.data_ptr())
    th.check(kind + " device entry on the built list", td._call(c.fx, c.d_x, c.d_q, c.at.nall), c.R)
    assert int(flag.cpu()[0]) == 0
    got, nall = tb._build(c.fx, c.inp, c.d_x, special)                   # a second build into the buffers of the first
    tb._same_list(kind + " again", got, nall, c.ref, c.at)
    bad = lib.conp_debug_check_guards()
    assert bad == 0, (kind, newton, special, bad, lib.conp_last_error().decode())
tb.test_a_grid_with_capped_cells_and_an_empty_build()
bad = lib.conp_debug_check_guards()
assert bad == 0, (bad, lib.conp_last_error().decode())
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
