"""-m gpu: conp_fix_post_neighbor_device under CONP_GUARD=1 in a fresh child process (as tests/test_gpu_ghosts_guard.py): every
device buffer of the library sits between two zones of a known byte pattern, and no kernel of conp_reneigh.hip -- nor the b-row
regrouping and the updates that read the tables it made -- stores outside its buffers: the small, the sparse and the medium
(z-window) case of tests/test_gpu_post_neighbor_device.py, and the two re-neighbours with growing buffers."""
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
import test_gpu_post_neighbor_device as tp
from conp_amd import capi
lib = capi.load_library()
lib.conp_debug_check_guards.restype = int
assert lib.conp_debug_check_guards() == 0, "guard zones are off"
def clean(what):
    bad = lib.conp_debug_check_guards()
    assert bad == 0, (what, bad, lib.conp_last_error().decode())
for kind, newton in (("small", False), ("small127", True), ("sparse", False), ("medium", False)):
    tp.test_device_route_equals_the_host_route(kind, newton)
    clean("%s newton %d" % (kind, newton))
tp.test_two_device_reneighbours_the_second_longer()
clean("growing buffers")
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
