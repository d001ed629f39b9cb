"""-m gpu: conp_potential_atom_device under CONP_GUARD=1 in a fresh child process (as tests/test_gpu_field_guard.py): every device
buffer of the library sits between two zones of a known byte pattern, and neither the kernels of conp_potatom.hip nor the provider
kernels the entry strings together store outside their buffers -- over the edge cases of tests/test_gpu_potential_device.py: the
target counts 1, 63, 64, 65, 129 in one and in several blocks, the crafted list's rows and segments, every selection on the small box
with both newton settings and both list routes, the reuse paths of both providers and the refusals."""
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
import test_gpu_potential_device as tp
from conp_amd import capi
lib = capi.load_library()
lib.conp_debug_check_guards.restype = int
assert lib.conp_debug_check_guards() == 0, "guard zones are off"

def clean(what):
    torch.cuda.synchronize()
    bad = lib.conp_debug_check_guards()
    assert bad == 0, (what, bad, lib.conp_last_error().decode())

for count in (1, 63, 64, 65, 129):
    tp.test_target_counts_at_the_block_edges(count)
    clean(("targets", count))
for newton in (False, True):
    tp.test_the_crafted_list_with_real_coordinates(newton)
    clean(("crafted list", newton))
    for built in (False, True):
        tp.test_pair_part_and_full_result("small", "ffield", newton, built)
        clean(("small", newton, built))
tp.test_reuse_after_the_ewald_force_entry_is_byte_identical("dilute", "slab")
clean("reuse, Ewald")
tp.test_reuse_on_a_pppm_handle_agrees_to_the_spread_s_rounding()
clean("reuse, pppm")
tp.test_reuse_without_a_valid_bit_is_refused()
tp.test_refusals()
clean("refusals")
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
