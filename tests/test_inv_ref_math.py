"""no GPU needed: the helpers of tests/test_gpu_inverse_sizes.py (tests/inv_ref.py) -- the long double inverse against the identity
and against every closed form, the closed forms' pivot sequence against a plain elimination, the exact cases through an unblocked
float64 Gauss-Jordan, the restated tier arithmetic of launch_inverse against the kernel source and hand-worked values, where the
pivots of each row permutation fall in that plan, and the property of the inputs the bound relies on: an elimination that forgets
one low-order update is hundreds of bounds away."""
import os

import numpy as np
import pytest

import inv_ref as ir

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lammps-user-conp2_amd", "csrc")
SMALL = (5, 64, 129)


def _closed_forms(n):
    rng = np.random.default_rng(n)
    g = dict(row_perm=rng.permutation(n), col_perm=rng.permutation(n), row_pow2=rng.integers(-3, 4, size=n),
             col_pow2=rng.integers(-3, 4, size=n))
    return {"kms": (ir.kms(n), ir.kms_inverse(n)),
            "kms rho 0.3": (ir.kms(n, 0.3), ir.kms_inverse(n, 0.3)),
            "kms_general": (ir.kms_general(n, **g), ir.kms_general_inverse(n, **g)),
            "second_difference": (ir.second_difference(n), ir.second_difference_inverse(n)),
            "kms_bumped": (ir.kms_bumped(n), ir.kms_bumped_inverse(n))}


def _residual(a, x):
    return float(np.max(np.abs(a.astype(ir.LD) @ x - np.eye(a.shape[0], dtype=ir.LD))))


def test_restated_constants_are_the_kernels():
    """inv_ref restates constants and the tier arithmetic of conp_inverse.hip: whoever changes one there is sent here"""
    k = open(os.path.join(CSRC, "conp_inverse.hip")).read()
    assert f"constexpr int INV_NB = {ir.NB};" in k and f"constexpr int PC_MAXG = {ir.PC_MAXG};" in k
    assert "constexpr int PC_LD = INV_NB + 1;" in k
    assert "const int ld = (n + 127) / 128 * 128;" in k
    li = k[k.index("bool launch_inverse("):k.index("void launch_symmetry_check(")]
    assert "int maxg = ncu < PC_MAXG ? ncu : PC_MAXG;" in li and "if (maxg_env >= 1 && maxg_env < maxg) maxg = maxg_env;" in li
    assert "int rpw = (m + maxg - 1) / maxg;" in li and "rpw = rpw < 64 ? 64 : (rpw + 15) / 16 * 16;" in li
    assert "const int G = (m + rpw - 1) / rpw;" in li
    assert "const size_t lds = ((size_t)rpw * PC_LD + INV_NB + 4) * sizeof(double) + 8 * sizeof(int);" in li
    assert "bool fits = lds <= 150 * 1024 && G <= ncu;" in li
    assert "const int r0 = wg * rpw;" in k                      # pivot_places: workgroup w holds panel rows [w rpw, (w + 1) rpw)


@pytest.mark.parametrize("n", SMALL)
def test_inverse_ld_gives_the_identity_and_the_closed_forms(n):
    """A X = I to 1e-17 n, and then |X - A^-1| = |A^-1 (A X - I)| <= ||A^-1||_inf max|A X - I|: every closed form within that of
    inverse_ld (plus its own few roundings at 2^-63)"""
    for name, (a, closed) in _closed_forms(n).items():
        x = ir.inverse_ld(a)
        res = _residual(a, x)
        assert res <= 1e-17 * n, (name, n, res)
        assert _residual(a, closed) <= 1e-17 * n, (name, n)
        norm_inf = float(np.abs(closed).sum(axis=1).max())
        scale = float(np.max(np.abs(closed)))
        err = float(np.max(np.abs(x - closed)))
        assert err <= norm_inf * 1e-17 * n + 8 * 2.0 ** -63 * scale, (name, n, err / scale)
    for seed in (1, 2):                                        # and general dense matrices
        a = np.random.default_rng(seed).standard_normal((n, n))
        assert _residual(a, ir.inverse_ld(a)) <= 1e-17 * n
    # e_lapack, the float64 figure the GPU bound is built on, is far above what the reference itself is off by
    a = np.random.default_rng(3).standard_normal((n, n))
    x = ir.inverse_ld(a)
    assert ir.rel_error(np.linalg.inv(a), x) > 100 * _residual(a, x) * float(np.abs(x).sum(axis=1).max() / np.abs(x).max())


def test_closed_form_values():
    k = ir.kms_inverse(4)
    t = ir.LD(1) / 3
    want = np.array([[4, -2, 0, 0], [-2, 5, -2, 0], [0, -2, 5, -2], [0, 0, -2, 4]], ir.LD) * t
    assert float(np.max(np.abs(k - want))) <= 2.0 ** -62
    assert np.array_equal(ir.kms(3), [[1, .5, .25], [.5, 1, .5], [.25, .5, 1]])
    assert np.array_equal(ir.kms_inverse(1), [[1]]) and np.array_equal(ir.kms(1), [[1]])
    s = ir.second_difference_inverse(3)
    assert float(np.max(np.abs(s - np.array([[3, 2, 1], [2, 4, 2], [1, 2, 3]], ir.LD) / 4))) == 0.0
    # condition numbers: below 9 for kms at any n; 4 (n + 1)^2 / pi^2 for the second difference, 2.5e6 at n = 2500
    assert np.linalg.cond(ir.kms(300)) < 9.0
    assert np.linalg.cond(ir.second_difference(300)) == pytest.approx(4 * 301 ** 2 / np.pi ** 2, rel=1e-3)
    assert 2.4e6 < 4 * 2501 ** 2 / np.pi ** 2 < 2.6e6
    b = ir.kms_bumped(200)
    assert np.array_equal(b, b.T) and b[199, 199] == 0.125
    # the general form really permutes and scales: row i is 2^r_i times row perm[i] of K, column j likewise
    rp, cp = np.array([2, 0, 1]), np.array([1, 2, 0])
    a = ir.kms_general(3, row_perm=rp, col_perm=cp, row_pow2=[1, 0, -1], col_pow2=[0, 2, 0])
    assert np.array_equal(a, [[1.0, 2 * 4, .5], [.5, .25 * 4, 1.0], [.5, .25 * 4, .25]])


@pytest.mark.parametrize("n", ir.PIVOT_SIZES)
def test_the_row_permutation_is_the_pivot_sequence(n):
    """a plain float64 elimination with partial pivoting on K[perm, :] takes exactly the rows pivot_sequence says, and in every
    column the winner is at least twice the runner-up (1 - rho^2 against rho (1 - rho^2)): no ties, no near-ties"""
    for name, perm in ir.row_perms(n).items():
        want = ir.pivot_sequence(perm)
        a = ir.kms_general(n, row_perm=perm).copy()
        for j in range(n):
            col = np.abs(a[j:, j])
            order = np.argsort(-col, kind="stable")
            p = j + int(order[0])
            assert p == want[j], (name, n, j)
            if len(col) > 1:
                assert col[order[0]] >= 2.0 * col[order[1]] * (1 - 1e-12), (name, n, j)
            a[[j, p]] = a[[p, j]]
            a[j + 1:] -= (a[j + 1:, j] / a[j, j])[:, None] * a[j][None, :]
        # and the inverse of the permuted matrix is the closed form
        if n <= 129:
            m = ir.kms_general(n, row_perm=perm)
            assert _residual(m, ir.kms_general_inverse(n, row_perm=perm)) <= 1e-17 * n


def test_pivot_sequence_hand_worked():
    assert list(ir.pivot_sequence([0, 1, 2, 3])) == [0, 1, 2, 3]
    assert list(ir.pivot_sequence([3, 2, 1, 0])) == [3, 2, 2, 3]          # after two swaps everything is in place
    assert list(ir.pivot_sequence([3, 0, 1, 2])) == [1, 2, 3, 3]          # the shift: always the next row
    assert list(ir.pivot_sequence([0, 2, 1, 3])) == [0, 2, 2, 3]


@pytest.mark.parametrize("n", ir.PIVOT_SIZES)
def test_the_permutations_put_a_pivot_in_every_named_place(n):
    """on the default panel (no cap) these sizes run with 2, 3, 4 and 6 workgroups of 64 rows, the last holding 1, 1, 8 and 1"""
    plan = ir.panel_plan(n, 256, 0)
    G = {65: 2, 129: 3, 200: 4, 321: 6}[n]
    last = {65: 1, 129: 1, 200: 8, 321: 1}[n]
    assert (plan[0].rpw, plan[0].G, plan[0].m - (plan[0].G - 1) * 64) == (64, G, last) and all(p.coop for p in plan)
    perms = ir.row_perms(n)
    assert ("swap_64_last" in perms) == (n != 65) and len(perms) == (8 if n != 65 else 7)
    places = {name: ir.pivot_places(ir.pivot_sequence(p), plan) for name, p in perms.items()}
    for name, pl in places.items():
        assert pl["only_row_left"] == [n - 1], name            # the last column: no choice left, whatever came before
    ident = places["identity"]
    assert ident["self"] == list(range(n)) and not ident["same_wg"] and not ident["other_wg"]
    rev = places["reversal"]
    assert rev["last_ragged_wg"][0] == 0 and rev["other_wg"][0] == 0                # the ragged last workgroup wins first
    assert (0 in rev["ragged_single_row"]) == (last == 1)
    # towards the middle the partner is in row j's own workgroup (not at n = 129, where the first panel ends before the partners
    # come that close and the second starts in place); then everything is in place
    assert bool(rev["same_wg"]) == (n != 129) and rev["self"]
    sh = places["shift"]
    assert sh["same_wg"][:3] == [0, 1, 2] and 63 in sh["other_wg"] and sh["self"] == [n - 1]
    assert places["swap_63_64"]["other_wg"] == [63] and places["swap_63_64"]["same_wg"] == []
    assert places["swap_0_last"]["last_ragged_wg"] == [0] and places["swap_0_last"]["other_wg"] == [0]
    assert places["swap_1_2"]["same_wg"] == [1] and places["swap_1_2"]["other_wg"] == []
    if n != 65:                                                # a swap inside a later panel: row 64 is row 0 of panel 1
        want_wg = "same_wg" if n - 1 - 64 < 64 else "other_wg"
        assert places["swap_64_last"][want_wg] == [64]
        assert places["swap_64_last"]["last_ragged_wg"] == ([64] if n - 64 > 64 else [])
    rnd = places["random"]
    assert rnd["other_wg"] and rnd["same_wg"] and rnd["last_ragged_wg"]
    every = set()
    for pl in places.values():
        every |= {k for k, v in pl.items() if v}
    assert every == set(ir.PLACES) - (set() if last == 1 else {"ragged_single_row"})


def test_panel_plan_values():
    for n in (1, 63, 64, 65, 700, 2500, 16383):                # without a cap every panel has 64 rows per workgroup below 16384
        assert all(p.rpw == 64 and p.coop and p.G == (p.m + 63) // 64 for p in ir.panel_plan(n, 256, 0)), n
    assert ir.panel_plan(16385, 256, 0)[0].rpw == 80
    p = ir.panel_plan(65, 256, 0)
    assert [(q.k0, q.m, q.nbw, q.G) for q in p] == [(0, 65, 64, 2), (64, 1, 1, 1)]
    assert ir.panel_plan(2500, 256, 0)[0].G == 40 and len(ir.panel_plan(2500, 256, 0)) == 40
    assert ir.panel_plan(2500, 256, 0)[-1][:3] == (2496, 4, 4)
    p = ir.panel_plan(700, 256, 5)
    assert [q.rpw for q in p] == [144, 128, 128, 112, 96, 80, 64, 64, 64, 64, 64] and all(q.coop and q.G <= 5 for q in p)
    p = ir.panel_plan(1100, 256, 4)
    assert (p[0].rpw, p[0].lds, p[0].G, p[0].coop) == (288, 150336, 4, True) and all(q.coop for q in p)
    assert p[0].lds <= ir.LDS_LIMIT < ir.panel_plan(1153, 256, 4)[0].lds           # the largest that fits
    p = ir.panel_plan(1200, 256, 4)
    assert (p[0].rpw, p[0].coop, p[0].lds) == (304, False, 158656)
    assert [q.coop for q in p] == [q.m <= 1152 for q in p] and p[0].m == 1200 and p[1].m == 1136 and p[1].coop
    p = ir.panel_plan(2500, 256, 5)                            # the existing test's capped run: one-workgroup panels down to m = 1408
    assert [q.coop for q in p] == [q.m <= 1440 for q in p] and sum(not q.coop for q in p) == 17 and p[0].rpw == 512
    assert ir.panel_plan(300, 2, 0)[0][3:] == (160, 2, (160 * 65 + 68) * 8 + 32, True)      # a device of two compute units
    assert [ir.leading_dimension(n) for n in (1, 127, 128, 129, 256, 257)] == [128, 128, 128, 256, 256, 384]
    for n, cap in ir.TIERS:
        assert len(ir.panel_plan(n, 256, cap)) == (n + 63) // 64


@pytest.mark.parametrize("n", [5, 64, 65, 129, 200])
def test_exact_cases_through_a_plain_float64_elimination(n):
    """one unblocked float64 Gauss-Jordan returns each exact case to the bit (-0.0 counts as 0.0)"""
    rng = np.random.default_rng(n)
    for name, perm in ir.row_perms(n).items():
        a = ir.generalized_permutation(n, perm, rng.integers(-20, 21, size=n), rng.choice([-1.0, 1.0], size=n))
        assert np.count_nonzero(a) == n and (np.count_nonzero(a, axis=0) == 1).all() and (np.count_nonzero(a, axis=1) == 1).all()
        want = ir.generalized_permutation_inverse(a)
        assert np.array_equal(want @ a, np.eye(n)) and np.array_equal(a @ want, np.eye(n))
        got, _piv = ir.gauss_jordan(a, np.float64)
        assert np.array_equal(got, want), (name, n)
    e = ir.exchange(n)
    got, piv = ir.gauss_jordan(e, np.float64)
    assert np.array_equal(e, e.T) and e[0, 0] == 0.0 and np.array_equal(got, e)
    assert list(piv[:n // 2]) == list(range(n - 1, n - 1 - n // 2, -1))         # every pivot from the current last rows


def test_block_diagonal_keeps_exact_zeros():
    a = ir.matrix(("block_diagonal",))
    mask = ir.block_mask(ir.BLOCK_SIZES)
    n = sum(ir.BLOCK_SIZES)
    assert a.shape == (n, n) and np.array_equal(a, a.T) and not a[~mask].any() and (a[mask] != 0).all()
    assert all(b % ir.NB for b in np.cumsum(ir.BLOCK_SIZES)) and np.linalg.cond(a) < 10 and np.linalg.eigvalsh(a)[0] >= 1.0
    got, _piv = ir.gauss_jordan(a, np.float64)
    assert not got[~mask].any()
    ref = ir.reference(("block_diagonal",))
    assert not ref[~mask].any() and _residual(a, ref) <= 1e-17 * n
    assert ir.rel_error(got, ref) <= ir.bound(("block_diagonal",))


def test_the_cases_by_key():
    """matrix / reference / e_lapack / bound of the GPU module's keys: seeded, cached, and what they say they are"""
    for n in (2, 65, 129):
        s = ir.matrix(("spd", n))
        assert np.array_equal(s, s.T) and np.linalg.eigvalsh(s)[0] >= 1.0 and ir.matrix(("spd", n)) is s
        g = ir.matrix(("gauss", n))
        assert not np.array_equal(g, g.T)
        u = ir.matrix(("ulp", n))
        d = np.argwhere(u != u.T)
        assert sorted(map(tuple, d)) == [(n - 2, n - 1), (n - 1, n - 2)] and u[n - 2, n - 1] == np.nextafter(u[n - 1, n - 2], np.inf)
        for key in (("spd", n), ("gauss", n), ("ulp", n), ("kms", n), ("kms_bumped", n), ("second_difference", n), ("scaled", n)):
            assert _residual(ir.matrix(key), ir.reference(key)) <= 1e-17 * n * max(1.0, float(np.abs(ir.matrix(key)).max())), key
            assert ir.bound(key) == 16 * max(ir.e_lapack(key), n * 2.0 ** -53) and ir.e_lapack(key) < 1e-11
    sc = ir.matrix(("scaled", 129))
    args = ir._scaled_args(129)
    plain = ir.kms_general(129, row_perm=args["row_perm"], col_perm=args["col_perm"])
    assert set(np.unique(np.log2(sc / plain))) == {-6.0, 0.0, 6.0}         # both scalings are 2^+-3, nothing else differs
    assert not np.array_equal(args["col_perm"], np.arange(129)) and not np.array_equal(args["row_perm"], args["col_perm"])
    assert ir.error_bound(100, 0.0) == 1600 * 2.0 ** -53 and ir.error_bound(100, 1e-12) == 16e-12
    with pytest.raises(ValueError):
        ir.matrix(("kms", 5))[0, 0] = 2.0                       # shared between tests: read-only


def test_tile_report_names_the_tile():
    ref = np.ones((130, 130), ir.LD)
    got = np.ones((130, 130))
    got[129, 3] += 4e-13
    got[5, 5] += 1e-13
    te = ir.tile_errors(got, ref)
    assert te.shape == (2, 2) and te[1, 0] == pytest.approx(4e-13, rel=1e-3) and te[0, 0] == pytest.approx(1e-13, rel=1e-3)
    assert te[0, 1] == 0.0 and te[1, 1] == 0.0
    groups, worst = ir.tile_report(te, 1e-12)
    assert groups["last_row"] == pytest.approx(0.4, rel=1e-3) and groups["first"] == pytest.approx(0.1, rel=1e-3)
    assert worst.startswith("tile (1, 0) of 2 x 2")


def test_a_lost_low_order_update_is_far_outside_the_bound():
    """what the old test's 1e-9 let pass: a blocked elimination that skips ONE rank-one contribution to one 128 x 128 tile of the
    matrix (the update of tile (1, 1) from the last pivot of the second 64-column step, the row next to that tile), on the
    matrices of the edge cases at n = 257.  It lands hundreds of bounds away for the closed form and for the dense matrices."""
    n = 257
    for key in (("kms", n), ("spd", n), ("gauss", n)):
        a = ir.matrix(key)
        ref, bound = ir.reference(key), ir.bound(key)
        good, _p = ir.gauss_jordan(a, np.float64)
        assert ir.rel_error(good, ref) <= bound, key              # an honest float64 Gauss-Jordan is inside

        m = np.zeros((n, 2 * n))
        m[:, :n] = a
        m[np.arange(n), n + np.arange(n)] = 1.0
        for j in range(n):
            p = j + int(np.argmax(np.abs(m[j:, j])))
            m[[j, p]] = m[[p, j]]
            m[j] /= m[j, j]
            f = m[:, j].copy()
            f[j] = 0.0
            upd = f[:, None] * m[j][None, :]
            if j == 127:
                upd[128:256, 128:256] = 0.0                    # the lost update
            m -= upd
        miss = ir.rel_error(m[:, n:], ref)
        print(f"  {key}: e_lapack {ir.e_lapack(key):.2e}, bound {bound:.2e}, honest float64 {ir.rel_error(good, ref) / bound:.3f}, "
              f"lost update {miss / bound:.0f} bounds")
        assert miss >= 100 * bound, (key, miss / bound)
