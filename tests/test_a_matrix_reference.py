"""CPU: the definitional reference for single entries of the electrode matrix (helpers.a_entries_from_definitions) against the
oracle's full A (orc_fix_a_cal: electrode tables by recurrence, the (planar, kz) expansion, the neighbour list) on every entry of
the small decks.  This is what lets tests/test_gpu_setup_sizes.py trust the helper where the oracle's full matrix is out of reach."""
import numpy as np
import pytest

from conp_amd import capi, neighbor, systems
from helpers import OracleRun, a_entries_from_definitions
from test_gpu_parity import rough

# two independent evaluations of the same ~1e4-term sums, one of them in extended precision: measured worst case over the ten
# decks below 2.6e-14 of the largest entry (dilute_slab_rough, K = 22687); asserted at 10 x that
MEASURED_WORST = 2.6e-14
BOUND = 10 * MEASURED_WORST

DECKS = {
    "dilute_ffield": lambda: systems.deck("dilute", "ffield", etypes=True),
    "dilute_slab": lambda: systems.deck("dilute", "slab", etypes=True),
    "small_ffield": lambda: systems.small_random(ne_side=4, n_elyte=96, lz=60.0),
    "small_slab": lambda: systems.small_random(ne_side=4, n_elyte=96, lz=60.0, mode="slab"),
    "small_tall_slab": lambda: systems.small_random(ne_side=4, n_elyte=96, lz=400.0, mode="slab"),
}
CASES = [(d, r) for d in DECKS for r in (False, True)]


@pytest.mark.parametrize("deck,is_rough", CASES, ids=[d + ("_rough" if r else "") for d, r in CASES])
def test_definitions_reproduce_every_entry_of_the_oracles_matrix(oracle, deck, is_rough):
    """every entry of A, both triangles and the diagonal.  Measured (10 decks): worst |helper - oracle| / max|A| = 2.6e-14 (dilute_slab_rough; 1e-15 .. 2e-14 on the others);
    the bound is 10 x that.  1e-12 or worse would mean the helper's conventions (V with slab_volfactor, raw z in the slab
    term, ug_tot = sum 2 ug, the polynomial erfc and its cuts, no qqrd2e) or the oracle are wrong."""
    s = DECKS[deck]()
    if is_rough:
        s = rough(s)
    at, alist, blist = neighbor.build_lists(s)
    o = OracleRun(oracle, s, at, alist, blist)
    oracle.orc_fix_a_cal(o.fx.h)
    A_o = o.fx.matrix()
    ne = A_o.shape[0]
    kt = capi.host_ktables(s)                               # pinned bit-exact to the oracle's by test_host_logic.py
    assert np.array_equal(kt["ug"], o.fx.ks.ug) and np.array_equal(kt["kzvecs"], o.fx.ks.kzvecs)
    pairs = np.stack(np.meshgrid(np.arange(ne), np.arange(ne), indexing="ij"), -1).reshape(-1, 2)
    A_d = a_entries_from_definitions(s, at, kt, o.fx.ks, pairs, eleall2tag=o.fx.maps()["eleall2tag"]).reshape(ne, ne)
    err = np.abs(A_d - A_o).max() / np.abs(A_o).max()
    print(f"{deck}{'_rough' if is_rough else ''}: Ne {ne} K {kt['kcount']}: definitions vs oracle {err:.2e} of max|A|")
    assert err < BOUND
    o.fx.close()
