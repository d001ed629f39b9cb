"""-m gpu: conp_fix_post_force_device under CONP_GUARD=1 in a fresh child process (as tests/test_gpu_post_neighbor_guard.py): every
device buffer of the library sits between two zones of a known byte pattern, and neither post_force_device_kernel nor
post_force_finish_kernel stores outside the library's buffers: the oracle's box under both newton settings, the owner count that is
no multiple of four, and the call behind the device re-neighbour of tests/test_gpu_post_force_device.py."""
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
import test_gpu_post_force_device as tf
from conp_amd import capi
lib = capi.load_library()
lib.conp_debug_check_guards.restype = int
assert lib.conp_debug_check_guards() == 0, "guard zones are off"
def clean(what):
    bad = lib.conp_debug_check_guards()
    assert bad == 0, (what, bad, lib.conp_last_error().decode())
for newton in (False, True):
    tf.test_matches_the_oracle_and_the_host_entry(newton)
    clean("oracle box, newton %d" % newton)
tf.test_an_owner_count_that_is_no_multiple_of_four()
clean("ragged owner count")
tf.test_after_the_device_reneighbour()
clean("after the device re-neighbour")
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
