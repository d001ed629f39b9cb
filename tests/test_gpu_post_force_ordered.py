"""-m gpu: conp_fix_post_force_ordered_device -- the Gaussian correction's forces without a float atomic, on
the inputs of tests/test_gpu_post_force_device.py and to that module's bounds: d_out byte-equal to the atomic entry's; the forces
within 1e-9 of the oracle and 1e-12 of the atomic entry (and of the host entry); byte-identical over three calls and two handles;
after the host post_neighbor and after conp_fix_post_neighbor_device; refused without the fix's transposed index."""
import dataclasses

import numpy as np
import pytest

from conp_amd import ConpError, FixConp, neighbor
from test_gpu_post_force_device import (HOST, ORACLE, _dev, _device_and_host_handles, call, check_against_oracle_and_host, compare,
                                        oracle_case)

pytestmark = pytest.mark.gpu


def call_ordered(fx, d_x, d_q, nall, f=True, out=True, pre=None, times=1):
    """test_gpu_post_force_device.call for the ordered entry, every call with its own d_f -> ([d_f], [d_out])"""
    import torch
    fs, outs = [], []
    for _ in range(times):
        d_f = None if not f else _dev(np.zeros((nall, 3)) if pre is None else pre)
        d_o = torch.full((10,), float("nan"), dtype=torch.float64, device="cuda") if out else None
        if out:
            d_o[9] = -77.0
        torch.cuda.synchronize()
        fx.post_force_ordered_device(d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr() if f else 0, d_o.data_ptr() if out else 0)
        fs.append(d_f); outs.append(d_o)
    torch.cuda.synchronize()
    for o in outs:
        assert o is None or float(o[9]) == -77.0
    return [None if t is None else t.cpu().numpy() for t in fs], [None if o is None else o.cpu().numpy()[:9] for o in outs]


def second_handle(c):
    """a fresh handle with the case's setup and the fix's transposed index"""
    _, alist, _ = neighbor.build_lists(c.s)
    at = dataclasses.replace(c.at, q=c.at.q.copy())
    fx = FixConp(c.s)
    fx.init_lists(alist, c.lst)
    fx.setup_post_neighbor(at)
    fx.setup_pre_force(at, 0, c.s.potdiff)
    fx.fix_transpose_list_device()
    return fx


@pytest.mark.parametrize("newton,kind", [(False, "pushed"), (True, "pushed"), (False, "ragged"), (False, "plain")])
def test_matches_the_oracle_the_atomic_entry_and_itself(newton, kind):
    c = oracle_case(newton, kind)
    nall = c.at.nall
    c.fx.fix_transpose_list_device()                                 # behind the host post_neighbor of the setup
    pre = np.random.default_rng(3).normal(size=(nall, 3))
    f_a, (out_a,) = call(c.fx, c.d_x, c.d_q, nall, pre=pre)          # the atomic entry
    fs, outs = call_ordered(c.fx, c.d_x, c.d_q, nall, pre=pre, times=3)
    fx2 = second_handle(c)
    fs2, outs2 = call_ordered(fx2, c.d_x, c.d_q, nall, pre=pre, times=3)
    fx2.close()
    for f, o in zip(fs + fs2, outs + outs2):
        assert o.tobytes() == out_a.tobytes()                        # d_out: the atomic entry's bytes
        assert f.tobytes() == fs[0].tobytes()                        # forces: byte-identical over three calls and two handles
    tag = f"ordered, {kind}, newton {int(newton)}"
    if kind == "plain":
        assert out_a[8] == 0 and fs[0].tobytes() == pre.tobytes()    # no pair inside the gate: nothing is written
        return
    assert out_a[8] >= 4                                             # the gate is open
    check_against_oracle_and_host(tag, c, fs[0] - pre, outs[0])
    compare(tag + ": against the atomic entry", fs[0] - pre, None, f_a - pre, 0, 0, 0, HOST)
    # exactly the rows the atomic entry changes are changed, every other row keeps its bytes
    assert np.array_equal(np.any(fs[0] != pre, axis=1), np.any(f_a != pre, axis=1))
    # each output alone
    (f_only,), _ = call_ordered(c.fx, c.d_x, c.d_q, nall, out=False, pre=pre)
    _, (out_only,) = call_ordered(c.fx, c.d_x, c.d_q, nall, f=False)
    assert f_only.tobytes() == fs[0].tobytes() and out_only.tobytes() == out_a.tobytes()
    c.fx.post_force_ordered_device(c.d_x.data_ptr(), c.d_q.data_ptr(), 0, 0)       # CONP_OK (anything else raises), nothing done


def test_ehgo_box():
    c = oracle_case(False, "ehgo")
    c.fx.fix_transpose_list_device()
    pre = np.random.default_rng(4).normal(size=(c.at.nall, 3))
    f_a, (out_a,) = call(c.fx, c.d_x, c.d_q, c.at.nall, pre=pre)
    fs, outs = call_ordered(c.fx, c.d_x, c.d_q, c.at.nall, pre=pre, times=3)
    assert all(o.tobytes() == out_a.tobytes() for o in outs) and all(f.tobytes() == fs[0].tobytes() for f in fs)
    assert out_a[8] > 0
    check_against_oracle_and_host("ordered, ehgo", c, fs[0] - pre, outs[0])
    compare("ordered, ehgo: against the atomic entry", fs[0] - pre, None, f_a - pre, 0, 0, 0, HOST)


@pytest.mark.parametrize("newton", [False, True])
def test_after_the_device_reneighbour_and_the_refusal_without_the_index(newton):
    c, fd, fh, b, d_q = _device_and_host_handles(newton)
    fd.pre_force_device(b.d_x.data_ptr(), d_q.data_ptr(), c.s.potdiff)
    with pytest.raises(ConpError) as e:                              # conp_fix_post_neighbor_device left no index
        fd.post_force_ordered_device(b.d_x.data_ptr(), d_q.data_ptr(), 0, 0)
    assert e.value.code == -2 and "conp_fix_transpose_list_device" in str(e.value)
    fd.fix_transpose_list_device()
    f_a, (out_a,) = call(fd, b.d_x, d_q, b.nall)
    fs, outs = call_ordered(fd, b.d_x, d_q, b.nall, times=3)
    assert out_a[8] >= 4 and np.abs(f_a).max() > 0
    assert all(o.tobytes() == out_a.tobytes() for o in outs) and all(f.tobytes() == fs[0].tobytes() for f in fs)
    compare(f"ordered after the device re-neighbour, newton {int(newton)}: against the atomic entry", fs[0], None, f_a, 0, 0, 0, HOST)
    assert np.array_equal(np.any(fs[0] != 0.0, axis=1), np.any(f_a != 0.0, axis=1))
    if newton:
        assert np.any(fs[0][b.n:] != 0.0)                            # the term lands on ghost rows too
    # the refusals of the atomic entry, before anything else
    for d_x, d_qp in ((0, d_q.data_ptr()), (b.d_x.data_ptr(), 0)):
        with pytest.raises(ConpError) as e:
            fd.post_force_ordered_device(d_x, d_qp, 0, 0)
        assert e.value.code == -1
    fd.close(); fh.close()


def test_before_setup():
    c = oracle_case(False)
    fx = FixConp(c.s)
    with pytest.raises(ConpError) as e:
        fx.post_force_ordered_device(c.d_x.data_ptr(), c.d_q.data_ptr(), 0, 0)
    assert e.value.code == -2 and "post_force before setup" in str(e.value)
    fx.close()
