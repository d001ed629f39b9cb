"""-m gpu: the small kernels behind the structure-factor contraction (conp_kernels.hip) on both of their forms.

b_zc_final_kernel takes the electrode phase rows of its 16 atoms from LDS (staged beside the class table) or, where table + rows
exceed a workgroup's LDS and under CONP_PATH_ZC_PHASE_LOADS, loads them per thread; hc_sum_kernel / hc_sum_wide_kernel form the
addresses of the z-window form's pieces themselves or, for any other list and under CONP_PATH_HC_TABLES, read them from the piece
lists.  Both forms of either kernel do the same additions and products in the same order: b must come out bit for bit the same
(np.array_equal), and within 1e-10 of the oracle's (tests/test_gpu_decks.py's bar for b).  Every case first asserts on the host
side (fx.info()) that it takes the path and has the property it is named for, and skips with a message otherwise."""
import functools

import numpy as np
import pytest

from conp_amd import FixConp, capi, neighbor, systems
from helpers import oracle_sk_and_b, rel_err

pytestmark = pytest.mark.gpu
B_BAR = 1e-10                                              # tests/test_gpu_decks.py: b against the oracle


def _medium(mode="ffield", seed=7, **kw):
    """tests/test_gpu_zn_gemm_epilogue.py's box: 16 x 8 cells, 16384 electrolyte atoms, the z-window path"""
    a = dict(n_cells_x=16, n_cells_y=8, lz=300.0, n_elyte=16384, cutoff=12.0, accuracy_relative=1e-6, g_ewald=0.26, mode=mode,
             seed=seed)
    a.update(kw)
    return systems.synthetic_fast(**a)


def _one_plane():
    """both electrodes in ONE plane (the second one moved onto the first one's z, half a lattice spacing aside): one z class"""
    s = _medium(seed=83)
    a, b = s.echeck == 1, s.echeck == -1
    d = np.sort(np.unique(np.round(s.x[a, 0], 6)))
    s.x[b, 2] = s.x[a, 2][0]
    s.x[b, 0] += 0.5 * (d[1] - d[0])
    return s


def _needle():
    """a box 1200 cells long and two wide with one z class: kxmax is near 500 while the planar vectors fill some 40 row tiles, so the
    class table (1 KB per tile) fits the finishing kernel but table + (kxmax + kymax + 3) rows of 256 B exceed a workgroup's 160 KB
    of LDS (1100 cells: kxmax 452, 36 tiles -- 150.5 of the 151.3 KB, still staged)"""
    s = _medium(n_cells_x=1200, n_cells_y=2, lz=60.0, n_elyte=8192, cutoff=2.0, seed=61)
    a, b = s.echeck == 1, s.echeck == -1
    d = np.sort(np.unique(np.round(s.x[a, 0], 6)))
    s.x[b, 2] = s.x[a, 2][0]
    s.x[b, 0] += 0.5 * (d[1] - d[0])
    return s


SYSTEMS = {
    "il_onelayer": lambda: systems.deck("il_onelayer", "ffield", etypes=True),
    "medium": _medium,
    "slab": lambda: _medium(mode="slab", n_cells_x=32, n_cells_y=16, lz=100.0, n_elyte=8192, seed=67),
    "ne_not_16": lambda: _medium(n_cells_x=15, n_cells_y=9, seed=71),
    "one_class": _one_plane,
    "eight_classes": lambda: _medium(layers=4, seed=43),
    "needle": _needle,
    "few_ranges": lambda: _medium(n_cells_x=32, n_cells_y=16, lz=60.0, n_elyte=8192, g_ewald=0.5, seed=73),
}


@functools.lru_cache(maxsize=None)
def _system(name):
    s = SYSTEMS[name]()
    return (s,) + tuple(neighbor.build_lists(s))


def _b(name, mask=0, rank=0, nranks=1):
    s, at, alist, blist = _system(name)
    with capi.test_paths(mask):
        fx = FixConp(s, rank=rank, nranks=nranks)
        fx.init_lists(alist, blist)
        fx.setup_post_neighbor(at)
        fx.b_cal(at)
        b = fx.vectors()[0].copy()
        info = fx.info()
        fx.close()
    return b, info


def _describe(label, i):
    print(f"{label}: Ne {i.elenum_all} kxmax {i.kxmax} kymax {i.kymax} nzc {i.n_zclasses} zn_cols {i.zn_cols} ranges {i.zn_ranges} "
          f"arithmetic {i.hc_arithmetic} zc_final {i.zc_final} over {i.zc_row_tiles} row tiles")


# ---- b_zc_final_kernel: phase rows from LDS against the per-thread loads, and against the oracle ---------------------------------
@pytest.mark.parametrize("name", ["il_onelayer", "medium", "slab", "ne_not_16", "one_class", "eight_classes", "needle"])
def test_finishing_dot_staged_rows_keep_the_bits(name):
    """il_onelayer: sk_gemm's few pieces per row tile, added by the kernel itself (slot lists).  medium: the z-window's pieces,
    summed by hc_sum_wide first.  slab: the fin_z / sc terms, and the 32 x 16 cell sheet at g = 0.26 plans eleven row tiles (the
    k0 = 8 loop).  ne_not_16: 1080 electrode atoms, lanes i >= ne in the last workgroup.  one_class / eight_classes: nzc = 1
    and SK_HC_MAX.  needle: table + rows exceed the LDS bound, the default path IS the loads."""
    b, i = _b(name)
    _describe(name, i)
    if i.zc_final == 0:
        pytest.skip(f"{name}: the finishing dot kernel is not used (nzc {i.n_zclasses}, {i.zn_rows // 128} row tiles)")
    want_form = 1 if name == "needle" else 2
    if i.zc_final != want_form:
        pytest.skip(f"{name}: the default path took form {i.zc_final} of the kernel, the case needs {want_form} "
                    f"(kxmax {i.kxmax} kymax {i.kymax}, {i.zc_row_tiles} row tiles, {i.n_zclasses} classes)")
    if name == "il_onelayer":
        assert i.zn_cols == 0 and i.elenum_all == 832
    if name == "medium":
        assert i.zn_cols in (32, 48)
    if name == "slab":
        s = _system(name)[0]
        assert s.slabflag == 1
        if i.zc_row_tiles <= 8:
            pytest.skip(f"slab: {i.zc_row_tiles} row tiles, the loop behind the first eight does not run")
    if name == "ne_not_16":
        assert i.elenum_all == 1080 and i.elenum_all % 16 != 0
    if name == "one_class":
        assert i.n_zclasses == 1
    if name == "eight_classes":
        assert i.n_zclasses == 8
    if name == "needle":
        assert i.zc_row_tiles * 128 * i.n_zclasses * 8 + (i.kxmax + i.kymax + 3) * 256 > 160 * 1024 - 64 * 17 * 8
    b_l, i_l = _b(name, capi.PATH_ZC_PHASE_LOADS)
    assert i_l.zc_final == 1, "the test path did not select the per-thread loads"
    assert np.abs(b).max() > 0
    assert np.array_equal(b, b_l), (name, rel_err(b, b_l))
    s, at, alist, blist = _system(name)
    _, _, b_o, ks = oracle_sk_and_b(s, at, alist, blist)
    ks.close()
    e = rel_err(b, b_o)
    print(f"{name}: b {e:.2e} of max against the oracle")
    assert e < B_BAR, (name, e)


# ---- hc_sum_kernel / hc_sum_wide_kernel: arithmetic piece addresses against the lists --------------------------------------------
def _arith_against_tables(name, rank=0, nranks=1, wide=None):
    b, i = _b(name, 0, rank, nranks)
    _describe(f"{name} rank {rank} of {nranks}", i)
    if i.zn_cols == 0 or i.n_zclasses == 0:
        pytest.skip(f"{name}: not on the projecting z-window path (zn_cols {i.zn_cols}, nzc {i.n_zclasses})")
    if wide is not None and (i.zn_ranges > 32) != wide:
        pytest.skip(f"{name}: {i.zn_ranges} ranges, the case needs {'more than' if wide else 'at most'} 32")
    assert i.hc_arithmetic == 1, "the z-window form's lists are arithmetic on a rank that owns every row tile"
    b_t, i_t = _b(name, capi.PATH_HC_TABLES, rank, nranks)
    assert i_t.hc_arithmetic == 0 and i_t.zn_ranges == i.zn_ranges
    assert np.abs(b).max() > 0
    assert np.array_equal(b, b_t), (name, rank, nranks, rel_err(b, b_t))
    return i


def test_wide_piece_sum_arithmetic_addresses_keep_the_bits():
    """more than 32 ranges: hc_sum_wide_kernel, 32 threads per element"""
    _arith_against_tables("medium", wide=True)


def test_piece_sum_arithmetic_addresses_keep_the_bits():
    """at most 32 ranges on one rank: the planner deals four workgroup slots per CU to the row tiles, so a plan of many row tiles
    (a large sheet at g = 0.5: 35 tiles, 29 ranges on 256 CUs, if those fit 32 window columns -- a thin, dense liquid) gets few
    ranges each -- hc_sum_kernel, eight threads per element.  (The shares of eight ranks below take that kernel too: 21 ranges.)"""
    _arith_against_tables("few_ranges", wide=False)


def test_rank_shares_with_different_range_counts_keep_the_bits():
    """two ranks and eight: a rank's share of the chunk axis is cut into its own number of ranges (one per six chunks at most),
    every rank passes its own count"""
    counts = set()
    for world in (2, 8):
        for rank in (0, world - 1):
            counts.add(_arith_against_tables("medium", rank, world).zn_ranges)
    assert len(counts) > 1, counts


def test_full_form_keeps_the_tables():
    """CONP_PATH_SK_CLASSIC: sk_gemm's band-local pieces are no arithmetic list"""
    _, i = _b("medium", capi.PATH_SK_CLASSIC)
    assert i.zn_cols == 0 and i.zn_ranges == 0 and i.hc_arithmetic == 0
