"""no GPU needed: the helpers of tests/test_gpu_cg_sizes.py (tests/cg_ref.py) -- the float128 projected CG against a direct solve of
the constrained system, the matrices' Gershgorin bound against their eigenvalues, the iteration counts they were tuned for, the
restated loop and launch structure against the kernel source and against hand-worked cases, and the property of the inputs the
entry-wise bound relies on: a dropped column of the smallest tile is thousands of bounds away."""
import os
import re

import numpy as np
import pytest

import cg_ref as cr

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lammps-user-conp2_amd", "csrc")
SMALL = (62, 130, 449, 961, 1025)


@pytest.fixture(scope="module")
def small():
    out = {}
    for ne in SMALL:
        A, g = cr.spd_matrix(ne, cr.seed_matrix(ne))
        out[ne] = (A, g, cr.vectors(A, cr.seed_vectors(ne)))
    return out


def test_sizes_reach_what_they_are_for():
    cr.check_sizes()


def test_restated_constants_are_the_kernels():
    """cg_ref restates loop bounds and thresholds of conp_kernels.hip / conp_fix.cpp: whoever changes one there is sent here"""
    k = open(os.path.join(CSRC, "conp_kernels.hip")).read()
    f = open(os.path.join(CSRC, "conp_fix.cpp")).read()
    dot = k[k.index("double cg_row_dot("):k.index("void gemv_rows_guarded_kernel(")]
    assert re.findall(r"for \(; (j(?: \+ \d+)?) < n; j \+= (\d+)\)", dot) == [("j + 960", "1024"), ("j + 448", "512"), ("j", "64")]
    assert "a[u] = srow[j + 64 * u]; x[u] = p[j + 64 * u];" in dot
    assert f"const bool keep = n <= {cr.KEEP_MAX};" in k
    assert "const int rpb = n <= 4096 ? 8 : 16;" in k and "dim3(mode == 4 ? 1 : (n + rpb - 1) / rpb), dim3(1024), lds" in k
    assert "bool cg_step_fits(int n) { return n > 0 && (size_t)n * sizeof(double) <= 128 * 1024; }" in k
    assert "const size_t lds = (size_t)n * sizeof(double);" in k[k.index("void launch_cg_step("):]
    assert "const int so = mode == 4 ? (iter + 1) & 1 : iter & 1;" in k
    cg = f[f.index("  void cg() {"):f.index("  // fix_conp.cpp:698-718 equation_solve")]
    assert "int cg_batch = 8;" in f and "batch = std::max(2, std::min(16, cg_batch));" in cg and cg.count("batch = 4;") == 2
    assert "const bool two_launch = cg_unfused || !cg_step_fits(ne) || args.maxiter <= 1;" in cg
    assert "const int last = std::min(args.maxiter - 1, iter + batch - 1);" in cg and "for (; iter < last; ++iter) step(iter + 1, 2);" in cg
    assert "step(iter, 4);" in cg and "step(iter, 3);" in cg and "if (done || iter + 1 >= args.maxiter) break;" in cg
    assert "if (done) cg_batch = cg_iterations;" in cg and "cg_iterations = done ? (int)ctl[6] : 0;" in cg


def test_lane_tiers():
    every = list(range(64))
    # n = 449: lane 0 alone has j + 448 < n and takes the 8-wide tier (8 elements); the others step seven times singly
    assert cr.lane_tiers(449, 0) == dict(w16=0, w8=1, w1=0) and cr.lane_tiers(449, 1) == dict(w16=0, w8=0, w1=7)
    assert cr.lanes_with(449, w8=1) == [0]
    assert cr.lanes_with(512, w8=1, w1=0) == every and cr.lanes_with(511, w8=1) == every[:63]
    assert cr.lane_tiers(961, 0) == dict(w16=1, w8=0, w1=0) and cr.lane_tiers(961, 1) == dict(w16=0, w8=1, w1=7)
    assert cr.lane_tiers(961, 63) == dict(w16=0, w8=1, w1=7) and cr.lanes_with(961, w16=1) == [0]
    assert cr.lanes_with(1024, w16=1, w8=0, w1=0) == every
    assert cr.lanes_with(62, w1=0, w8=0, w16=0) == [62, 63] and cr.lanes_with(62, w1=1) == every[:62]
    for n in (62, 449, 961, 1025, 1664, 8200):                # every element is some lane's, once
        assert sum(16 * t["w16"] + 8 * t["w8"] + t["w1"] for t in (cr.lane_tiers(n, l) for l in range(64))) == n
    assert cr.lane_tiers(1664, 5) == dict(w16=1, w8=1, w1=2)


def test_launch_shapes():
    assert [cr.rows_per_block(n) for n in (1, 4096, 4097, 16384)] == [8, 8, 16, 16]
    assert [cr.n_workgroups(n) for n in (62, 4096, 4097, 6151, 8200)] == [8, 512, 257, 385, 513]
    assert [cr.last_workgroup_rows(n) for n in (62, 4096, 4097, 6151, 8200)] == [6, 8, 1, 7, 8]
    assert cr.keeps_registers(4096) and not cr.keeps_registers(4097)
    assert cr.lds_bytes(8200) == 65600 > cr.LDS_DEFAULT and cr.lds_bytes(16384) == cr.LDS_MAX


def test_batch_schedule_hand_worked():
    """(iteration, mode) of every launch: 1 = start + matvec 1, 2 = update(k - 1) + matvec(k), 4 = update(k) alone + control block to
    the host, 3 = matvec(k) alone at the head of a later batch"""
    def run(k0, k1):
        return [(k0, 3)] + [(k, 2) for k in range(k0 + 1, k1 + 1)] + [(k1, 4)]
    first8 = [(1, 1)] + [(k, 2) for k in range(2, 9)] + [(8, 4)]
    s = cr.batch_schedule(8, 5, 100)
    assert s.batches == [first8] and (s.iterations, s.converged, s.next_prev, s.where) == (5, True, 5, "inside") and not s.two_launch
    s = cr.batch_schedule(8, 8, 100)
    assert s.batches == [first8] and (s.iterations, s.converged, s.next_prev, s.where) == (8, True, 8, "last")
    s = cr.batch_schedule(8, 9, 100)
    assert s.batches == [first8, run(9, 12)] and (s.iterations, s.next_prev, s.where) == (9, 9, "inside")
    s = cr.batch_schedule(8, 23, 100)
    assert s.batches == [first8, run(9, 12), run(13, 16), run(17, 20), run(21, 24)] and (s.iterations, s.where) == (23, "inside")
    s = cr.batch_schedule(5, 5, 100)
    assert s.batches == [[(1, 1), (2, 2), (3, 2), (4, 2), (5, 2), (5, 4)]] and s.where == "last"
    s = cr.batch_schedule(23, 23, 100)
    first16 = [(1, 1)] + [(k, 2) for k in range(2, 17)] + [(16, 4)]
    assert s.batches == [first16, run(17, 20), run(21, 24)] and s.where == "inside" and s.next_prev == 23
    assert cr.batch_schedule(23, 24, 100).where == "last" and len(cr.batch_schedule(23, 24, 100).batches) == 3
    assert cr.batch_schedule(1, 3, 100).batches == [[(1, 1), (2, 2), (2, 4)], run(3, 6)]            # a first batch is never shorter than 2
    # maxiter: 1 = no iteration at all, in the two-launch form; 2 = one iteration; 3 = two
    s = cr.batch_schedule(8, None, 1)
    assert s.two_launch and s.batches == [] and (s.iterations, s.converged, s.next_prev) == (0, False, 8)
    s = cr.batch_schedule(8, None, 2)
    assert s.batches == [[(1, 1), (1, 4)]] and (s.iterations, s.converged, s.next_prev) == (1, False, 8)
    s = cr.batch_schedule(8, None, 3)
    assert s.batches == [[(1, 1), (2, 2), (2, 4)]] and (s.iterations, s.converged) == (2, False)
    s = cr.batch_schedule(8, 9, 9)                           # maxiter = the needed count: eight iterations, one batch, not converged
    assert s.batches == [first8] and (s.iterations, s.converged, s.next_prev) == (8, False, 8)
    s = cr.batch_schedule(8, 9, 10)
    assert s.batches == [first8, [(9, 3), (9, 4)]] and (s.iterations, s.converged, s.where) == (9, True, "last")
    s = cr.batch_schedule(6, None, 32)                       # ran out: 31 iterations
    assert [len(b) for b in s.batches] == [7] + [5] * 6 + [2] and s.batches[-1] == [(31, 3), (31, 4)] and s.iterations == 31


def test_matrix(small):
    for ne in SMALL:
        A, g, _v = small[ne]
        assert np.array_equal(A, A.T) and np.isfinite(A).all() and g >= cr.G
        lam = np.linalg.eigvalsh(A)
        assert g <= lam[0] and lam[-1] <= cr.G + 2.0 + cr.SPREAD      # g really is a lower bound; the discs' upper end
        d = np.diag(A)
        R = np.abs(A).sum(axis=1) - d
        assert np.all(d - R >= g) and R.max() == pytest.approx(1.0, rel=1e-12)
        assert not np.array_equal(cr.spd_matrix(ne, 7)[0], A)
    A = small[1025][0]
    off = A - np.diag(np.diag(A))
    nb = cr.n_tiles(1025)
    tile = np.array([[np.abs(off[i * 128:(i + 1) * 128, j * 128:(j + 1) * 128]).mean() for j in range(nb)] for i in range(nb)])
    assert tile[nb - 1, nb - 1] == 0.0                           # (the last diagonal tile is one element, the diagonal's)
    tile[nb - 1, nb - 1] = tile[0, 0]
    assert tile.max() / tile.min() > 1e3                       # the tiles differ by more than three decades
    t = cr.tile_scales(1025, cr.seed_matrix(1025) + 1)
    assert np.array_equal(t, t.T) and (t > 0).any() and (t < 0).any() and np.abs(t).max() / np.abs(t).min() == pytest.approx(10 ** 3.5)
    assert np.array_equal(np.sign(off[:128, 1024:]), np.sign(off[1024:, :128].T))
    for I in range(nb):
        for J in range(nb):
            blk = off[I * 128:(I + 1) * 128, J * 128:(J + 1) * 128]
            h = blk / t[I, J]
            assert blk.size == 1 or (h > 0).any() and (h < 0).any()            # the tile's sign multiplies a symmetric random part of both signs


def test_cg_ref_solves_the_constrained_system(small):
    """against a direct solve of [A 1; 1' 0] [q; lambda] = [b; 0], refined with float128 residuals"""
    for ne in (62, 130):
        A, g, v = small[ne]
        for name in ("dense", "unit_last"):
            # (the unit vector leaves a multiplier of order 1 / n: the recursion's floor, 2^-64 n multiplier^2, is above TOL_REF)
            tol = cr.TOL_REF if name == "dense" else 1e-18
            r = cr.cg_ref(A, v[name], tol, 80)
            assert r.converged and r.iterations < 60
            q = cr.kkt_solve(A, v[name])
            resid = np.asarray(v[name], cr.LD) - cr.matvec_ld(A, q)
            assert float(np.max(np.abs(resid - resid.mean()))) < 1e-17 * float(np.max(np.abs(v[name])))     # q is the solution
            assert abs(float(q.sum())) < 1e-17
            if name == "dense":                               # the constant the residual converges to
                assert float(resid.mean()) == pytest.approx(cr.MULTIPLIER, rel=1e-4)
            err = float(np.sqrt(((r.q - q) ** 2).sum()))
            assert err <= np.sqrt(ne * tol) / g, (ne, name, err)
            assert abs(float(r.q.sum())) < 4 * r.iterations * ne * 2.0 ** -64 * float(np.max(np.abs(r.q)))   # the sum the algorithm implies: 0
            assert abs(float(r.net - r.q.sum())) == 0.0


def test_history_snapshots_and_stop_rule(small):
    A, g, v = small[130]
    b = v["dense"]
    full = cr.cg_ref(A, b, 0.0, 12, keep=(1, 2, 5))
    assert full.iterations == 11 and not full.converged and len(full.hist) == 12 and set(full.snaps) == {0, 1, 2, 5}
    assert not full.snaps[0].any()
    for k in (1, 2, 5):                                        # maxiter = k + 1 runs k iterations and ends where the longer run passed
        cut = cr.cg_ref(A, b, 0.0, k + 1)
        assert cut.iterations == k and np.array_equal(cut.q, full.snaps[k]) and np.array_equal(cut.hist, full.hist[:k + 1])
    nd = cr.needed(full.hist, 130, 1e-6)
    stop = cr.cg_ref(A, b, 1e-6, 100)
    assert stop.converged and stop.iterations == nd and float(stop.hist[nd]) / 130 < 1e-6 <= float(stop.hist[nd - 1]) / 130
    assert cr.cg_ref(A, b, 1e-6, 1).iterations == 0 and not cr.cg_ref(A, b, 1e-6, 1).q.any()
    # b scaled by s: the same iterates scaled, so the history of b tells where s b stops
    s = 2.0 ** -9
    assert cr.cg_ref(A, s * b, 1e-6, 100).iterations == cr.needed(full.hist, 130, 1e-6, s) < nd


ITERS = {62: (9, 24), 130: (9, 25), 449: (9, 26), 961: (9, 26), 1025: (9, 26), 1664: (9, 26), 2049: (9, 26), 4096: (9, 26),
         4097: (9, 26), 6151: (9, 26), 8200: (9, 26)}


@pytest.mark.parametrize("ne", cr.SIZES)
def test_iteration_counts_are_the_tuned_ones(ne):
    """the default tolerance takes 6 to 12 iterations, the tight one more than 20 (float128 at the small sizes, float64 with a BLAS
    product above: the counts agree, test_f64_stays_inside_the_bounds)"""
    A, g = cr.spd_matrix(ne, cr.seed_matrix(ne))
    b = cr.vectors(A, cr.seed_vectors(ne))["dense"]
    if ne <= 1025:
        hist = cr.cg_ref(A, b, cr.TOL_REF, 61).hist
    else:
        hist = cr.cg_f64(A, b, cr.TOL_TIGHT, 61, matvec=lambda M, p: M @ p).hist
    got = (cr.needed(hist, ne, cr.TOL_DEFAULT), cr.needed(hist, ne, cr.TOL_TIGHT))
    assert got == ITERS[ne] == cr.ITERS[ne] and 6 <= got[0] <= 12 and got[1] > 20


def test_f64_stays_inside_the_bounds(small):
    """what the GPU tests allow, tried on an honest float64 implementation with numpy's summation order: the converged bound, the
    iteration counts, the six digits of every logged residual, the sum of the charges"""
    for ne in SMALL:
        A, g, v = small[ne]
        b = v["dense"]
        ref = cr.cg_ref(A, b, cr.TOL_REF, 61)
        assert ref.converged
        for tol in (cr.TOL_DEFAULT, cr.TOL_TIGHT):
            f = cr.cg_f64(A, b, tol, 61)
            assert f.converged and f.iterations == cr.needed(ref.hist, ne, tol)
            frac = float(np.sqrt(((f.q - ref.q) ** 2).sum())) / cr.converged_bound(ne, tol, g)
            assert frac < 1.0, (ne, tol, frac)
            assert ["%g" % x for x in f.hist] == ["%g" % float(x) for x in ref.hist[:f.iterations + 1]]
            assert abs(float(np.asarray(f.q, cr.LD).sum())) <= cr.sum_bound(ne, f.iterations, np.abs(f.q).max())


def test_a_dropped_column_of_the_smallest_tile_is_far_outside_the_bound(small):
    """the entry-wise bound of the cut-off solves is 16 e64; a product that leaves out ONE column of the tile with the smallest
    magnitude, in the rows of that tile, lands at least 1000 bounds away after one iteration"""
    for ne in (449, 961, 1025):
        A, g, v = small[ne]
        t = np.abs(cr.tile_scales(ne, cr.seed_matrix(ne) + 1))
        I, J = np.unravel_index(np.argmin(t + 1e9 * np.eye(len(t))), t.shape)
        col = min(J * 128 + 5, ne - 1)

        def dropped(M, p):
            y = cr.matvec_f64(M, p)
            rows = slice(I * 128, min(ne, (I + 1) * 128))
            y[rows] -= M[rows, col] * p[col]
            return y
        for name in ("dense", "unit_last"):
            b = v[name]
            ref = cr.cg_ref(A, b, 0.0, 3, keep=(1, 2))
            good = cr.cg_f64(A, b, 0.0, 3, keep=(1, 2))
            bad = cr.cg_f64(A, b, 0.0, 3, keep=(1, 2), matvec=dropped)
            k = 2                                            # (the first matvec changes alpha_1 only: q_1 = alpha_1 p_0 moves as a whole)
            e64 = float(np.max(np.abs(good.snaps[k] - ref.snaps[k])))
            bound = cr.error_bound(e64, float(np.max(np.abs(ref.snaps[k]))))
            miss = float(np.max(np.abs(bad.snaps[k] - ref.snaps[k])))
            assert e64 <= bound / 16 and miss >= 1e3 * bound, (ne, name, miss / bound)


def test_error_bound():
    assert cr.error_bound(1e-15, 1.0) == 16e-15
    assert cr.error_bound(0.0, 3.0) == 16 * 2.0 ** -53 * 3.0        # the floor: exact agreement on the CPU does not ask it of the GPU
    assert cr.converged_bound(100, 1e-6, 2.0) == pytest.approx(1e-2)
