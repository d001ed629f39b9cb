"""-m gpu: the transposed half list -- conp_pair_transpose_list_device, conp_fix_transpose_list_device and the
download conp_pair_get_transposed_list against the numpy index of tests/transpose_ref.py (a stable argsort of the listed slots by j;
tests/test_transpose_ref_math.py checks it and the crafted list without a GPU).

Exactness: all three arrays equal the numpy index, on the crafted list (rows and segments of 0, 1, 63 .. 129 and 300+ entries, an
owner missing from ilist, rows in shuffled order), the three inputs of tests/test_gpu_pair_forces.py, and the device build with and
without an exclusion rule (variants A and E of tests/md_loop_ref.py), there for the fix's own list (which = 1) too.  Determinism:
byte-identical over three builds.  Refusals and the lifetime of both indices."""
import dataclasses

import numpy as np
import pytest

import md_loop_ref as ml
import transpose_ref as tr
from conp_amd import ConpError, FixConp
from test_gpu_pair_forces import case

pytestmark = pytest.mark.gpu


def same(got, want, tag):
    for name, g, w in zip(("own_row", "tr_ptr", "tr_entry"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (tag, name)


def three_builds(fx, lst, nall, tag, which=0):
    want = tr.transpose(lst, nall)
    build = fx.fix_transpose_list_device if which else fx.pair_transpose_list_device
    got = []
    for _ in range(3):
        build()
        got.append(fx.pair_get_transposed_list(which))
        same(got[-1], want, tag)
    for g in got[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(g, got[0])), tag
    return want


def test_the_crafted_list():
    c = case("small", False)
    nall = 401
    lst = tr.crafted_list(nall)
    c.fx.pair_set_list(lst, nall)
    try:
        own_row, tr_ptr, _ = three_builds(c.fx, lst, nall, "crafted list")
        assert own_row[tr.MISSING] == -1 and tr_ptr[-1] == lst.numneigh[lst.ilist].sum()
    finally:
        c.fx.pair_set_list(c.lst, c.at.nall)                         # (the shared handle gets its list back)


@pytest.mark.parametrize("kind,newton", [("small", False), ("small", True), ("sparse", True), ("il_onelayer", False)])
def test_the_uploaded_lists(kind, newton):
    c = case(kind, newton)
    c.fx.pair_set_list(c.lst, c.at.nall)
    _, tr_ptr, _ = three_builds(c.fx, c.lst, c.at.nall, c.tag)
    assert tr_ptr[-1] == c.lst.neigh.size
    # the fix's own list, after the host post_neighbor of the setup (the same list: init_lists(lst, lst))
    three_builds(c.fx, c.lst, c.at.nall, c.tag + ", the fix's list", which=1)


@pytest.mark.parametrize("variant", ["A", "E"])                       # E: built with `neigh_modify exclude`
def test_the_device_build_and_the_fix_list_and_their_lifetimes(variant):
    fx = ml.new_handle(variant)
    L = ml.Loop(fx, variant, 0, False)
    L.start()                                                        # the re-neighbouring sequence, post_neighbor_device included
    lst, nall = fx.pair_get_list()
    assert (ml.system(variant).mirror is not None) == (variant == "E") and lst.neigh.size > 0
    want = three_builds(fx, lst, nall, f"variant {variant}: built list")
    three_builds(fx, lst, nall, f"variant {variant}: the fix's list after post_neighbor_device", which=1)
    # a later pair-list build replaces the pair style's list and drops ITS index; the fix keeps its list and its index (section 19)
    L.build_list()
    with pytest.raises(ConpError) as e:
        fx.pair_get_transposed_list(0)
    assert e.value.code == -2
    with pytest.raises(ConpError) as e:
        fx.pair_compute_ordered_device(L.d_x.data_ptr(), L.d_q.data_ptr(), L.d_f.data_ptr(), 0, 0, 0)
    assert e.value.code == -2 and "conp_pair_transpose_list_device" in str(e.value)
    same(fx.pair_get_transposed_list(1), want, "the fix's index behind a pair-list build")
    fx.post_force_ordered_device(L.d_x.data_ptr(), L.d_q.data_ptr(), L.d_f.data_ptr(), 0)        # still served
    # the fix's re-neighbouring drops the fix's index
    fx.post_neighbor_device(L.d_x.data_ptr(), L.d_q.data_ptr())
    with pytest.raises(ConpError) as e:
        fx.pair_get_transposed_list(1)
    assert e.value.code == -2
    with pytest.raises(ConpError) as e:
        fx.post_force_ordered_device(L.d_x.data_ptr(), L.d_q.data_ptr(), L.d_f.data_ptr(), 0)
    assert e.value.code == -2 and "conp_fix_transpose_list_device" in str(e.value)
    fx.fix_transpose_list_device()
    same(fx.pair_get_transposed_list(1), want, "rebuilt")
    fx.close()


def test_refusals():
    c = case("small", False)
    fx = FixConp(c.s)
    with pytest.raises(ConpError) as e:                              # no list
        fx.pair_transpose_list_device()
    assert e.value.code == -2 and "conp_pair_set_list" in str(e.value)
    with pytest.raises(ConpError) as e:                              # before the fix has a list
        fx.fix_transpose_list_device()
    assert e.value.code == -2
    for which in (0, 1):
        with pytest.raises(ConpError) as e:
            fx.pair_get_transposed_list(which)
        assert e.value.code == -2
    fx.init_lists(c.lst, c.lst)
    fx.setup_post_neighbor(c.at)
    fx.pair_set_params(c.p.cutsq, c.p.cut_coul, c.p.lj)
    fx.pair_set_list(c.lst, c.at.nall)
    with pytest.raises(ConpError) as e:                              # a list, no index yet
        fx.pair_compute_ordered_device(1, 1, 1, 0, 0, 0)
    assert e.value.code == -2
    fx.pair_transpose_list_device()
    fx.fix_transpose_list_device()
    with pytest.raises(ConpError) as e:
        fx.pair_get_transposed_list(2)
    assert e.value.code == -1
    want = tr.transpose(c.lst, c.at.nall)
    same(fx.pair_get_transposed_list(0), want, "before the second set_list")
    # an owner twice in ilist: refused, and no index is left
    dup = dataclasses.replace(c.lst, ilist=np.ascontiguousarray(np.concatenate([c.lst.ilist[:-1], c.lst.ilist[:1]])))
    fx.pair_set_list(dup, c.at.nall)
    with pytest.raises(ConpError) as e:
        fx.pair_transpose_list_device()
    assert e.value.code == -1 and "twice" in str(e.value)
    with pytest.raises(ConpError) as e:
        fx.pair_get_transposed_list(0)
    assert e.value.code == -2
    # a stale index: pair_set_list replaces the list
    fx.pair_set_list(c.lst, c.at.nall)
    fx.pair_transpose_list_device()
    fx.pair_set_list(c.lst, c.at.nall)
    with pytest.raises(ConpError) as e:
        fx.pair_get_transposed_list(0)
    assert e.value.code == -2
    with pytest.raises(ConpError) as e:
        fx.pair_compute_ordered_device(1, 1, 1, 0, 0, 0)
    assert e.value.code == -2
    same(fx.pair_get_transposed_list(1), want, "the fix's index is not the pair style's")
    # the host post_neighbor drops the fix's index
    fx.post_neighbor(c.at)
    with pytest.raises(ConpError) as e:
        fx.pair_get_transposed_list(1)
    assert e.value.code == -2
    fx.close()
