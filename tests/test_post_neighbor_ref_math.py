"""no GPU needed: tests/post_neighbor_ref.py, the numpy restatement of the tables conp_fix_post_neighbor_device rebuilds (DESIGN.md
section 19), on hand-made cases whose answers are written down here, and the margins of the GPU tests' inputs: no listed atom of
theirs sits within 1e-9 of a cell boundary or of a window-origin step, so no rounding could move it."""
import numpy as np
import pytest

import neigh_ref as nref
import post_neighbor_ref as pnr
from conp_amd import capi


def _counting_sort(keys, n):
    """stable counting sort written as loops: position of every element"""
    start = np.zeros(n + 1, int)
    for k in keys:
        start[k + 1] += 1
    start = np.cumsum(start)
    nxt = start[:-1].copy()
    pos = np.zeros(len(keys), int)
    for i, k in enumerate(keys):
        pos[i] = nxt[k]
        nxt[k] += 1
    order = np.zeros(len(keys), int)
    order[pos] = np.arange(len(keys))
    return order


def test_three_equally_long_empty_runs_and_the_stable_order():
    """n = 64 cells of width 1.  Occupied: cells 0-11, 22-33, 44-53; empty: 12-21, 34-43, 54-63, ten cells each.  The walk from cell 0
    meets 12-21 first, so the list starts at cell 22.  38 atoms: one per occupied cell in DESCENDING cell order, then four more in cells
    25, 25, 3, 48 -- atoms of one cell keep their list order."""
    n, lz = 64, 64.0
    cells = [c for c in range(53, 43, -1)] + [c for c in range(33, 21, -1)] + [c for c in range(11, -1, -1)] + [25, 25, 3, 48]
    assert len(cells) == 38
    z = np.array(cells, float) + np.linspace(0.11, 0.83, len(cells))
    r = pnr.z_order(z, n, lz)
    assert np.array_equal(r.cell, cells) and r.c_start == 22
    assert r.occ[25] == 3 and r.occ[3] == 2 and r.occ[48] == 2 and r.occ[12:22].sum() == 0
    key = (np.array(cells) - 22) % 64
    assert np.array_equal(r.order, _counting_sort(key, 64))
    sorted_cells = np.array(cells)[r.order]
    assert sorted_cells[0] == 22 and sorted_cells[-1] == 11            # 22 .. 33, 44 .. 53, then 0 .. 11 behind the wrap
    at25 = [k for k in r.order if cells[k] == 25]
    assert at25 == sorted(at25) and len(at25) == 3                      # list order inside a cell
    # chunk bounds by hand: ur = u - 22 (+ 64), i0 = ceil(ur - 7.5)
    ur = np.where(z - 22 < 0, z - 22 + 64, z - 22)
    i0 = np.ceil(ur - 7.5).astype(int)[r.order]
    assert np.array_equal(r.ch_lo, [i0[:16].min(), i0[16:32].min(), i0[32:].min()])
    assert np.array_equal(r.ch_hi, [i0[:16].max(), i0[16:32].max(), i0[32:].max()])
    assert np.all(np.diff(i0) >= -1)                                    # the sorted list climbs through the grid without wrapping
    assert r.margin > 1e-4                                              # (the offsets 0.11 .. 0.83 pass 0.5 between two atoms)


def test_a_tie_across_cell_zero_and_a_full_box():
    # empty runs 2-3 and 6-7 (and none across 0): the first wins -> start 4; the ring is walked twice: runs 7-0 and 3-4 tie -> 7-0 is
    # met first only on the second lap, 3-4 on the first -> start 5
    assert pnr.start_cell(np.array([1, 1, 0, 0, 1, 1, 0, 0])) == 4
    assert pnr.start_cell(np.array([0, 1, 1, 0, 0, 1, 1, 0])) == 5
    assert pnr.start_cell(np.array([0, 0, 1, 1, 0, 1, 1, 0])) == 2      # 7-0-1 is the longest (3): the list starts at 2
    assert pnr.start_cell(np.ones(8, int)) == 0                         # no empty cell
    assert pnr.start_cell(np.zeros(8, int)) == 0                        # all empty: a run of n ends at n - 1
    # a full box of 8 cells, two atoms per cell in scrambled order: start 0, sorted by cell, list order inside a cell
    cells = np.array([3, 7, 0, 3, 5, 1, 6, 2, 4, 0, 7, 1, 2, 6, 5, 4])
    r = pnr.z_order(cells + 0.4, 8, 8.0)
    assert r.c_start == 0 and np.array_equal(r.order, [2, 9, 5, 11, 7, 12, 0, 3, 8, 15, 4, 14, 6, 13, 1, 10])


def test_u_that_rounds_to_n_is_clamped_into_the_last_cell():
    n, lz = 64, 64.0
    u, c = pnr.z_cells(np.array([-1e-15, 0.0, 63.999, 64.0, 128.5, -0.5]), n, lz)
    assert np.array_equal(c, [63, 0, 63, 0, 0, 63])
    assert u[0] == np.nextafter(64.0, 0.0) and u[3] == 0.0 and u[4] == 0.5 and u[5] == 63.5
    r = pnr.z_order(np.array([-1e-15, 10.2, 11.7]), n, lz)
    assert r.c_start == 63 and np.array_equal(r.order, [0, 1, 2])       # empty 12 .. 62: the list starts behind that run, at cell 63
    assert r.i0[0] == -6 and np.array_equal(r.key, [0, 11, 12])         # ur = nextafter(64, 0) - 63: just below 1


def test_scatter_lists_and_electrolyte_list_on_a_hand_made_rank():
    # six owned atoms: rows 0, 1, 2 for atoms 1, 3, 4; ghosts (owner): 3, 0, 1, 3, 5, 1
    echeck = np.array([0, 1, 0, -1, 1, 0])
    q = np.array([0.5, 0.0, 0.0, 0.0, 0.1, -0.5])
    a2e = pnr.rows_of_owned(echeck)
    assert np.array_equal(a2e, [-1, 0, -1, 1, 2, -1])
    owner = np.array([3, 0, 1, 3, 5, 1])
    sc = pnr.scatter_lists(a2e, owner, 3)
    assert np.array_equal(sc.ele_pairs, [[1, 0], [3, 1], [4, 2], [6, 1], [8, 0], [9, 1], [11, 0]])
    assert np.array_equal(sc.csr_ptr, [0, 3, 6, 7])
    assert np.array_equal(sc.csr_of, [1, 8, 11, 3, 6, 9, 4]) and np.array_equal(sc.csr_row, [0, 0, 0, 1, 1, 1, 2])
    assert np.array_equal(pnr.elyte_list(a2e, q), [0, 5])                # atom 2 has no charge, atom 4 is an electrode atom


@pytest.mark.parametrize("kind", pnr.SMALL)
@pytest.mark.parametrize("newton", [False, True])
def test_b_rows_equal_the_host_regrouping(kind, newton):
    inp = nref.inputs(kind, newton)
    at = inp.at
    lst = nref.reference(inp)[0]
    a2e_owned = pnr.rows_of_owned(at.echeck[:at.nlocal])
    a2e = np.concatenate([a2e_owned, a2e_owned[at.owner[at.nlocal:]]])
    ne = int((at.echeck[:at.nlocal] != 0).sum())
    got = pnr.b_rows(lst, a2e, at.nlocal, newton, ne)
    want = capi.host_pair_rows(1, lst, at, newton)
    assert want["npairs"] > 0
    assert np.array_equal(got.b_rowptr, want["row_ptr"]) and np.array_equal(got.b_ele, want["ele_atom"])
    assert np.array_equal(got.b_oth, want["oth_atom"])
    # the scatter lists against a plain walk over all atoms
    sc = pnr.scatter_lists(a2e_owned, at.owner[at.nlocal:], ne)
    atoms = np.nonzero(a2e >= 0)[0]
    assert np.array_equal(sc.ele_pairs[:, 0], atoms) and np.array_equal(sc.ele_pairs[:, 1], a2e[atoms])
    by_row = atoms[np.lexsort((atoms, a2e[atoms]))]
    assert np.array_equal(sc.csr_of, by_row) and np.array_equal(sc.csr_row, a2e[by_row])
    assert np.array_equal(np.diff(sc.csr_ptr), np.bincount(a2e[atoms], minlength=ne))


@pytest.mark.parametrize("kind", pnr.MEDIUM)
def test_gpu_inputs_keep_their_distance_from_every_rounding_edge(kind):
    c = pnr.case(kind)
    n, lz = pnr.zn_setup(c)
    el = pnr.elyte_list(c.a2e, c.own.q)
    assert len(el) >= 8192                                               # the z-window is taken
    r = pnr.z_order(c.xw[el, 2], n, lz)
    print(f"{kind}: {len(el)} listed atoms, n = {n}, start cell {r.c_start}, margin {r.margin:.3e}")
    assert r.margin >= 1e-9
    assert sorted(r.order.tolist()) == list(range(len(el)))
    if kind == "ragged":
        assert len(el) == 16379 and r.c_start != 0
