"""-m gpu: the transposed lists and the two ordered entries under CONP_GUARD=1 in a fresh child process (as
tests/test_gpu_guard.py): every device buffer of the library sits between two zones of a known byte pattern, and no kernel of
conp_transpose.hip, no pair_ordered_kernel and no post_force_ordered_kernel stores outside its buffers -- on the crafted list and the
small box, each output alone."""
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
import test_gpu_pair_forces as th
import test_gpu_pair_ordered as to
import test_gpu_post_force_device as tp
import test_gpu_post_force_ordered as tpo
import transpose_ref as tr
import pair_force_ref as pref
from conp_amd import capi
lib = capi.load_library()
lib.conp_debug_check_guards.restype = int
assert lib.conp_debug_check_guards() == 0, "guard zones are off"

def clean(tag):
    bad = lib.conp_debug_check_guards()
    assert bad == 0, (tag, bad, lib.conp_last_error().decode())

for newton in (False, True):
    c = th.case("small", newton, special=True)
    for name, lst in (("small box", c.lst), ("crafted list", tr.crafted_list(c.at.nall, targets=tr.central_targets(c.at.x, c.at.nlocal)))):
        tag = f"{{name}}, newton {{int(newton)}}"
        fx = to.fresh(c, lst)                                          # (pair_transpose_list_device inside)
        clean(tag + ": transposition")
        got = fx.pair_get_transposed_list(0)
        want = tr.transpose(lst, c.at.nall)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), tag
        R = c.R if lst is c.lst else pref.for_atoms(c.at, lst, c.p, c.s, newton, c.sl, c.sc)
        th.check(tag + ": all outputs", to.as_check(to.call(fx, c)[0]), R)
        clean(tag + ": all outputs")
        for only in to.NAMES:
            th.check(tag + ": " + only + " alone", to.as_check(to.call(fx, c, on=(only,))[0]), R)
            clean(tag + ": " + only + " alone")
        fx.fix_transpose_list_device()                                 # the fix's list of the host setup
        clean(tag + ": the fix's transposition")
        fx.close()
        clean(tag + ": released")
    # a 401-atom crafted list through pair_set_list alone (no compute: the handle's atoms are another count)
    fx = to.fresh(c)
    small = tr.crafted_list(401)
    fx.pair_set_list(small, 401)
    fx.pair_transpose_list_device()
    assert all(np.array_equal(g, w) for g, w in zip(fx.pair_get_transposed_list(0), tr.transpose(small, 401)))
    fx.close()
    clean("crafted list of 401 atoms")
    # the Gaussian twin, each output alone
    oc = tp.oracle_case(newton)
    oc.fx.fix_transpose_list_device()
    clean("the pushed box: transposition")
    f_a, (out_a,) = tp.call(oc.fx, oc.d_x, oc.d_q, oc.at.nall)
    for f, out in ((True, True), (True, False), (False, True)):
        fs, outs = tpo.call_ordered(oc.fx, oc.d_x, oc.d_q, oc.at.nall, f=f, out=out)
        if out:
            assert outs[0].tobytes() == out_a.tobytes()
        if f:
            tp.compare("ordered Gaussian forces under the guard", fs[0], None, f_a, 0, 0, 0, tp.HOST)
        clean(f"the pushed box, newton {{int(newton)}}: f {{f}}, out {{out}}")
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
