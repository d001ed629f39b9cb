"""-m gpu: the stream-ordered MD loop of tests/md_loop_ref.py under CONP_GUARD=1 in a fresh child process (as
tests/test_gpu_shake_guard.py): every device buffer of the library sits between two zones of a known byte pattern, and no kernel
stores outside its buffers while the ghost count shrinks and grows from one re-neighbouring to the next.  The zones are checked
after every re-neighbouring and at the end."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("A", "E")

CHILD = r'''
import sys
sys.path[:0] = [{tests!r}, {pkg!r}, {oracle!r}, {root!r}]
import torch
torch.cuda.init()
import md_loop_ref as ml
from conp_amd import capi
lib = capi.load_library()
lib.conp_debug_check_guards.restype = int
assert lib.conp_debug_check_guards() == 0, "guard zones are off"
for variant in {variants!r}:
    fx = ml.new_handle(variant)
    L = ml.Loop(fx, variant, ml.STEPS, False)
    L.start()
    seen = 1
    for k in range(ml.STEPS):
        L.step(k)
        if len(L.builds) != seen:
            seen = len(L.builds)
            bad = lib.conp_debug_check_guards()
            assert bad == 0, (variant, k, bad, lib.conp_last_error().decode())
    res = L.result()
    bad = lib.conp_debug_check_guards()
    assert bad == 0, (variant, "end", bad, lib.conp_last_error().decode())
    ref = ml.reference_trajectory(variant)
    assert res.flags == ref.flags and res.nghost == ref.nghost and sum(res.flags) >= 2 and len(set(res.nghost)) >= 3
    print("GUARD_RUN", variant, res.nghost[0], sorted(set(res.nghost)))
    fx.close()
print("GUARD_OK")
'''


def test_no_store_outside_the_buffers(tmp_path):
    script = tmp_path / "guard_child.py"
    script.write_text(CHILD.format(tests=os.path.join(ROOT, "tests"), pkg=os.path.join(ROOT, "lammps-user-conp2_amd"),
                                   oracle=os.path.join(ROOT, "oracle"), root=ROOT, variants=VARIANTS))
    env = dict(os.environ, CONP_GUARD="1")
    p = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "GUARD_OK" in p.stdout
    print(p.stdout)
