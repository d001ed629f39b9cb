"""-m gpu: the dense inverse (conp_inverse.hip, invert_device in conp_fix.cpp) at every block edge, panel tier and pivot row, through
conp_invert on matrices the test chose (tests/inv_ref.py makes them and their references; tests/test_inv_ref_math.py checks those
without a GPU).  One small handle serves the module; the paths are switched through the knobs invert_device reads per call
(CONP_PANEL_SINGLE, CONP_PANEL_MAXG, CONP_PANEL_SPIN, conp_debug_set_paths(PATH_INV_PIVOTED)), all restored in `finally`.

References.  Dense matrices (n <= 321) against inv_ref.inverse_ld (long double Gauss-Jordan plus one Newton step); kms, kms_general,
second_difference and kms_bumped against their closed forms evaluated in long double, at any n; generalized permutations, the
exchange matrix and the zeros of a block-diagonal matrix to the bit.

Bound.  max|inv - ref| / max|ref| <= 16 max(e_lapack, n 2^-53), e_lapack being the same measure for np.linalg.inv of the same matrix
(inv_ref.error_bound).  Nothing in it comes from what the GPU gives.  Every case prints its error as a fraction of that bound, and a
failure names the 128 x 128 tile of the output that is worst.

What the kernels do NOT promise: an exactly symmetric result on the positive-definite path.  inv_block_spd_kernel forms entry (r, c)
as B[r][c] - B[r][j] (B[j][c] / p) and entry (c, r) as B[c][r] - B[c][j] (B[j][r] / p), and inv_prep / inv_update / inv_fixup sum
C Dinv M[K, :] in another order on the two sides of the diagonal: the two roundings differ.  The module asserts |S - S'| within the
error bound, not equality.

Sizes and what each reaches (test_sizes_reach_what_they_are_for asserts it from inv_ref.panel_plan and the device's CU count):
    1, 2 one ragged block, ld 128     63 / 64 / 65 last block step of width 63 / 64 / 1; 65: two workgroups, the second with one row
    127 / 128 / 129 ld 128 / 128 / 256: 129 is one live row and column in a tile row and column of padding
    191 / 192 / 193, 255 / 256 / 257, 321 the same edges one and two tiles further; 321 = 5 x 64 + 1, ld 384
    65, 129, 200, 321 pivot rows by construction: 2, 3, 4, 6 workgroups of 64 rows, the last holding 1, 1, 8, 1
    700 cap 5: rpw 144, 128, 128, 112, 96, 80, 64 ...: up to three rows per lane in the candidate search
    1100 cap 4: rpw 288, 150336 B of LDS, the largest that fits     1200 cap 4: rpw 304 does not fit -> one one-workgroup panel,
    cooperative from m = 1136 on: both forms inside one inverse     2500: 40 workgroups of 64 rows, 40 panels
Out of scope: n >= 16384 (the only size with rpw > 64 without a cap), several ranks, inv_project and sym_pack.

Measured on one MI355X (256 CUs): worst error / bound per case group (every tier above is the one the device's plan gave).
  1. edges, worst of the six runs per n:
        n      1     2    63    64    65   127   128   129   191   192   193   255   256   257   321
           0.024 0.019 0.026 0.057 0.040 0.064 0.060 0.055 0.117 0.117 0.018 0.153 0.041 0.347 0.180
     The worst run of each n is a Gaussian matrix on the panel (e_lapack 1e-14 ... 4e-14 there); kms and the dense positive definite
     matrix stay below 0.01 on both paths.
  2. pivot rows: 0.005 / 0.008 / 0.002 / 0.006 at n = 65 / 129 / 200 / 321 over all permutations, the scaled case and the three panels
  3. tiers (700 cap 5, 1100 cap 4, 1200 cap 4, 2500): below 0.001 each; two calls gave the same bytes
  4. n = 2500: kms below 0.001 on both paths; second_difference 0.062 on both paths (e_lapack 1.05e-12), |S - S'| below 0.001 of it
  5. kms_bumped below 0.001; one ulp off symmetric 0.005 (n = 129), 0.003 (n = 200)      6. block diagonal 0.004 on both paths
The closed-form cases sit far inside their bound because it is the floor n 2^-53 that rules there (e_lapack is 8.9e-17 for kms at
every size) and a banded inverse collects far fewer than n roundings per entry.  What the module would catch and would not, tried on
scratch builds: reading `rowj` of the wrong parity in inv_panel_coop_kernel fails 32 of the 42 cases (first: n = 2, gauss, default
panel); dropping the `!(j >= k0 && j < k0 + nbw)` exclusion of Wb in inv_prep_kernel fails none, and cannot: inv_fixup_kernel
overwrites every entry those columns of Wb reach.  tests/test_inv_ref_math.py shows on the CPU that one lost rank-one update of one
tile is more than 100 bounds away.  Wall time of the module: 11 s."""
import os

import numpy as np
import pytest

import inv_ref as ir
from conp_amd import FixConp, capi, neighbor, systems

pytestmark = pytest.mark.gpu

KNOBS = ("CONP_PANEL_SINGLE", "CONP_PANEL_MAXG", "CONP_PANEL_SPIN")
DEFAULT, SINGLE, MAXG2 = {}, {"CONP_PANEL_SINGLE": "1"}, {"CONP_PANEL_MAXG": "2"}


@pytest.fixture(scope="module")
def fx():
    s = systems.small_random()
    at, alist, blist = neighbor.build_lists(s)
    f = FixConp(s)
    f.init_lists(alist, blist)
    f.setup_post_neighbor(at)
    assert not any(k in os.environ for k in KNOBS)
    yield f
    f.close()


def _num_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _invert(fx, a, env=DEFAULT, pivoted=False):
    """conp_invert with the panel knobs of `env` set and, if asked, the pivoted elimination forced; everything restored behind it"""
    lib = capi.load_library()
    os.environ.update(env)
    try:
        if pivoted:
            lib.conp_debug_set_paths(capi.PATH_INV_PIVOTED)
        return fx.invert(a)
    finally:
        lib.conp_debug_set_paths(0)
        for k in env:
            del os.environ[k]


def _check(tag, inv, key):
    """the result of one call against the case's reference: finite, inside the bound in every 128 x 128 tile"""
    ref, bound = ir.reference(key), ir.bound(key)
    assert np.isfinite(inv).all(), tag
    te = ir.tile_errors(inv, ref)
    groups, worst = ir.tile_report(te, bound)
    frac = float(te.max()) / bound
    print(f"  {tag}: e_lapack {ir.e_lapack(key):.2e}, bound {bound:.2e}, error / bound = {frac:.3g}  [" +
          ", ".join(f"{k} {v:.2g}" for k, v in groups.items()) + "]")
    assert frac <= 1.0, (tag, worst, groups)
    return frac


def _agree(tag, a, b, key):
    """two runs of one matrix on different panel forms agree within the bound (they take the same pivots: mostly to the bit)"""
    d = float(np.max(np.abs(a - b))) / float(np.max(np.abs(ir.reference(key))))
    assert d <= ir.bound(key), (tag, d / ir.bound(key))
    return d / ir.bound(key)


def test_sizes_reach_what_they_are_for():
    """the tiers and edges the cases below name, from the restated arithmetic and THIS device's compute-unit count"""
    ncu = _num_cus()
    assert ncu >= 40 and capi.PATH_INV_PIVOTED == 4
    assert [ir.leading_dimension(n) for n in (1, 2, 63, 64, 65, 127, 128, 129, 256, 257, 321)] == [128] * 7 + [256, 256, 384, 384]
    assert [ir.panel_plan(n, ncu)[-1].nbw for n in ir.EDGE_SIZES] == [1, 2, 63, 64, 1, 63, 64, 1, 63, 64, 1, 63, 64, 1, 1]
    for n, G, last in ((65, 2, 1), (129, 3, 1), (200, 4, 8), (321, 6, 1)):
        p = ir.panel_plan(n, ncu)[0]
        assert (p.rpw, p.G, p.m - (p.G - 1) * p.rpw, p.coop) == (64, G, last, True)
        p = ir.panel_plan(n, ncu, 2)[0]                        # CONP_PANEL_MAXG=2: two workgroups, more than 64 rows each above 128
        assert p.G == 2 and p.coop and p.rpw == {65: 64, 129: 80, 200: 112, 321: 176}[n]


# ---- 1. block and padding edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ir.EDGE_SIZES)
def test_block_and_padding_edges(fx, n):
    """the positive-definite path, the same matrices pivoted, and a general matrix on the cooperative and the one-workgroup panel"""
    worst = 0.0
    for kind in ("kms", "spd"):
        key = (kind, n)
        inv = _invert(fx, ir.matrix(key))
        assert fx.info().inverse_path == 1 and fx.info().inverse_retries == 0, key
        worst = max(worst, _check(f"n={n} {kind} positive-definite path", inv, key))
        sym = float(np.max(np.abs(inv - inv.T))) / float(np.max(np.abs(ir.reference(key))))
        assert sym <= ir.bound(key), (key, sym / ir.bound(key))            # (not promised exact: module docstring)
        piv = _invert(fx, ir.matrix(key), pivoted=True)
        assert fx.info().inverse_path == 2 and fx.info().inverse_retries == 0, key
        worst = max(worst, _check(f"n={n} {kind} pivoted", piv, key))
    key = ("gauss", n)
    got = []
    for env in (DEFAULT, SINGLE):
        got.append(_invert(fx, ir.matrix(key), env))
        # (a 1 x 1 matrix is symmetric: it takes path 1 when its entry is positive)
        assert fx.info().inverse_retries == 0 and (fx.info().inverse_path == 2 or n == 1), (key, env)
        worst = max(worst, _check(f"n={n} gauss {'one-workgroup' if env else 'default'} panel", got[-1], key))
    _agree(f"n={n} gauss default / one-workgroup", got[0], got[1], key)
    print(f"  n={n}: worst fraction {worst:.3g}")


# ---- 2. pivot rows by construction ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ir.PIVOT_SIZES)
def test_pivot_rows_by_construction(fx, n):
    """K[perm, :]: the row permutation is the pivot sequence (test_inv_ref_math), so the winner of every column is where the
    permutation put it -- in row j's workgroup, in another, in the ragged last one, row j itself, the only row left"""
    plan = ir.panel_plan(n, _num_cus())
    seen = set()
    worst = 0.0
    for name, perm in ir.row_perms(n).items():
        places = ir.pivot_places(ir.pivot_sequence(perm), plan)
        seen |= {k for k, v in places.items() if v}
        key = ("pivot", n, name)
        # (the identity leaves K itself, which would take path 1: forced onto the panel.  The reversal is symmetric too, a Hankel
        #  matrix, but indefinite: it reaches the panel through the rejection of the positive-definite attempt.)
        runs = [_invert(fx, ir.matrix(key), env, pivoted=name == "identity") for env in (DEFAULT, SINGLE, MAXG2)]
        assert fx.info().inverse_path == 2 and fx.info().inverse_retries == 0
        for form, inv in zip(("default", "one-workgroup", "two-workgroup"), runs):
            worst = max(worst, _check(f"n={n} rows {name} {form} panel", inv, key))
        _agree(f"n={n} {name} default / one-workgroup", runs[0], runs[1], key)
        _agree(f"n={n} {name} default / two-workgroup", runs[0], runs[2], key)
    assert seen == set(ir.PLACES) - (set() if n != 200 else {"ragged_single_row"})
    key = ("scaled", n)                                        # rows and columns scaled by 2^+-3, columns permuted: order not predicted
    runs = [_invert(fx, ir.matrix(key), env) for env in (DEFAULT, SINGLE, MAXG2)]
    assert fx.info().inverse_path == 2
    for form, inv in zip(("default", "one-workgroup", "two-workgroup"), runs):
        worst = max(worst, _check(f"n={n} scaled {form} panel", inv, key))
    _agree(f"n={n} scaled default / one-workgroup", runs[0], runs[1], key)
    _agree(f"n={n} scaled default / two-workgroup", runs[0], runs[2], key)
    print(f"  n={n}: worst fraction {worst:.3g}")


# ---- 3. panel tiers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("perm", ["reversal", "random"])
@pytest.mark.parametrize("n,cap", ir.TIERS)
def test_panel_tiers(fx, n, cap, perm):
    ncu = _num_cus()
    plan = ir.panel_plan(n, ncu, cap)
    if (n, cap) == (700, 5):                                   # more than one row per lane in the candidate search
        assert [p.rpw for p in plan] == [144, 128, 128, 112, 96, 80, 64, 64, 64, 64, 64] and all(p.coop for p in plan)
    elif (n, cap) == (1100, 4):                                # the LDS limit
        assert (plan[0].rpw, plan[0].lds, plan[0].G, plan[0].coop) == (288, 150336, 4, True) and all(p.coop for p in plan)
    elif (n, cap) == (1200, 4):                                # both forms inside one inverse
        assert (plan[0].rpw, plan[0].coop) == (304, False) and [p.coop for p in plan[1:]] == [True] * (len(plan) - 1)
        assert plan[1].m == 1136 <= 1152 and plan[1].rpw == 288
    else:
        assert (n, cap) == (2500, 0) and plan[0].G == 40 and all(p.rpw == 64 and p.coop for p in plan) and len(plan) == 40
    env = {"CONP_PANEL_MAXG": str(cap)} if cap else DEFAULT
    key = ("pivot", n, perm)
    places = ir.pivot_places(ir.pivot_sequence(ir.row_perms(n)[perm]), plan)
    assert places["other_wg"] and places["last_ragged_wg"] and places["self"]
    a = ir.matrix(key)
    first = _invert(fx, a, env)
    assert fx.info().inverse_path == 2 and fx.info().inverse_retries == 0
    second = _invert(fx, a, env)
    assert np.array_equal(ir.bits(first), ir.bits(second)), (n, cap, perm)          # two calls, the same bytes
    _check(f"n={n} cap {cap} rows {perm}", first, key)


# ---- 4. the positive-definite path at size and under bad conditioning ----------------------------------------------------------------
@pytest.mark.parametrize("kind", ["kms", "second_difference"])
def test_positive_definite_path_at_size(fx, kind):
    key = (kind, 2500)
    a = ir.matrix(key)
    inv = _invert(fx, a)
    assert fx.info().inverse_path == 1
    _check(f"n=2500 {kind} positive-definite path", inv, key)
    sym = float(np.max(np.abs(inv - inv.T))) / float(np.max(np.abs(ir.reference(key))))
    print(f"  n=2500 {kind}: |S - S'| / bound = {sym / ir.bound(key):.3g}")
    assert sym <= ir.bound(key)
    piv = _invert(fx, a, pivoted=True)
    assert fx.info().inverse_path == 2 and fx.info().inverse_retries == 0
    _check(f"n=2500 {kind} pivoted", piv, key)


# ---- 5. rejections of the positive-definite attempt ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 129, 200])
def test_exchange_matrix_is_rejected_in_the_first_column_and_inverted_exactly(fx, n):
    e = ir.exchange(n)
    for env in (DEFAULT, SINGLE):
        inv = _invert(fx, e, env)
        assert fx.info().inverse_path == 2 and fx.info().inverse_retries == 0
        assert np.array_equal(inv, e), (n, env, np.argwhere(inv != e)[:5])


@pytest.mark.parametrize("n", [129, 200])
def test_non_positive_pivot_in_the_last_column_of_the_last_block(fx, n):
    """kms_bumped: every pivot of the positive-definite attempt is positive but the last one, -0.125, in the last column of the
    ragged last block (width 1 at n = 129, 8 at n = 200): info = -8 there, the matrix restored, the pivoted result right"""
    key = ("kms_bumped", n)
    a = ir.matrix(key)
    assert np.array_equal(a, a.T) and ir.panel_plan(n)[-1].nbw == (1 if n == 129 else 8)
    inv = _invert(fx, a)
    assert fx.info().inverse_path == 2 and fx.info().inverse_retries == 0
    _check(f"n={n} kms_bumped after the rejection", inv, key)
    forced = _invert(fx, a, pivoted=True)                      # the restored matrix was the matrix: the same bytes as without the attempt
    assert np.array_equal(ir.bits(inv), ir.bits(forced))


@pytest.mark.parametrize("n", [129, 200])
def test_one_ulp_off_symmetric_never_tries_the_positive_definite_path(fx, n):
    key = ("ulp", n)
    a = ir.matrix(key)
    inv = _invert(fx, a)
    assert fx.info().inverse_path == 2
    forced = _invert(fx, a, pivoted=True)
    assert fx.info().inverse_path == 2
    assert np.array_equal(ir.bits(inv), ir.bits(forced))
    _check(f"n={n} one ulp off symmetric", inv, key)
    sym = _invert(fx, ir.matrix(("spd", n)))                   # and the symmetric matrix next to it does take path 1
    assert fx.info().inverse_path == 1 and not np.array_equal(sym, inv)


# ---- 6. exact cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 129, 321])
def test_generalized_permutations_are_inverted_exactly(fx, n):
    rng = np.random.default_rng(9000 + n)
    for name, perm in ir.row_perms(n).items():
        if name in ("identity", "shift"):
            continue
        a = ir.generalized_permutation(n, perm, rng.integers(-20, 21, size=n), rng.choice([-1.0, 1.0], size=n))
        want = ir.generalized_permutation_inverse(a)
        for env in (DEFAULT, SINGLE):
            inv = _invert(fx, a, env)
            assert np.array_equal(inv, want), (n, name, env, np.argwhere(inv != want)[:5])


def test_block_diagonal_keeps_exact_zeros_on_both_paths(fx):
    key = ("block_diagonal",)
    a = ir.matrix(key)
    mask = ir.block_mask(ir.BLOCK_SIZES)
    for pivoted, env in ((False, DEFAULT), (True, DEFAULT), (True, SINGLE)):
        inv = _invert(fx, a, env, pivoted=pivoted)
        assert fx.info().inverse_path == (2 if pivoted else 1)
        off = np.argwhere((inv != 0) & ~mask)
        assert len(off) == 0, (pivoted, env, off[:5])
        _check(f"block diagonal {ir.BLOCK_SIZES} {'pivoted' if pivoted else 'positive-definite path'}", inv, key)


# ---- 7. the barrier fallback, once ---------------------------------------------------------------------------------------------------
def test_barrier_time_out_falls_back_to_the_one_workgroup_panel(fx):
    """CONP_PANEL_SPIN=0 is the library's forced time-out: no poll allowed, every wave ends by construction, info = -7"""
    key = ("pivot", 321, "reversal")
    a = ir.matrix(key)
    single = _invert(fx, a, SINGLE)
    assert fx.info().inverse_retries == 0
    fx.mesg_drain()
    inv = _invert(fx, a, {"CONP_PANEL_SPIN": "0"})
    assert "timed out at its grid barrier" in fx.mesg_drain()
    assert fx.info().inverse_retries == 1 and fx.info().inverse_path == 2
    assert np.array_equal(ir.bits(inv), ir.bits(single))
    _check("n=321 rows reversal after the time-out", inv, key)
    again = _invert(fx, a)
    assert fx.info().inverse_retries == 0 and "timed out" not in fx.mesg_drain()
    _agree("n=321 reversal default / one-workgroup", again, single, key)
