"""-m gpu: conp_pair_build_list_exclude_device and the conp_zmirror_* entries under CONP_GUARD=1 in a fresh child process (as
tests/test_gpu_field_guard.py): every device buffer of the library sits between two zones of a known byte pattern, and no kernel
stores outside its buffers -- over the compaction-edge ladder, the case of 16 group and 16 molecule rules, and the mirror ladder."""
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
import test_gpu_pair_exclude as tx
import test_gpu_zmirror as tz
from conp_amd import capi
lib = capi.load_library()
lib.conp_debug_check_guards.restype = int
assert lib.conp_debug_check_guards() == 0, "guard zones are off"
for n in (63, 64, 65, 129, 257):
    for newton in (False, True):
        tx.test_compaction_edges_in_one_long_cell(n, newton)
        bad = lib.conp_debug_check_guards()
        assert bad == 0, ("compaction edges", n, newton, bad, lib.conp_last_error().decode())
tx.test_two_builds_null_rules_and_replaced_rules()
bad = lib.conp_debug_check_guards()
assert bad == 0, ("16 + 16 rules", bad, lib.conp_last_error().decode())
for n in tz.PAIRS:
    for layout in ("interleaved", "shuffled"):
        tz.test_ladder_map_and_copy(n, layout)
        bad = lib.conp_debug_check_guards()
        assert bad == 0, ("mirror", n, layout, bad, lib.conp_last_error().decode())
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
