"""Helpers of tests/test_gpu_cg_sizes.py, none of which needs a GPU (tests/test_cg_ref_math.py checks them):
  * spd_matrix: an exactly symmetric positive definite matrix whose off-diagonal 128 x 128 tiles each have a magnitude (spread over
    more than three decades) and a sign of their own, with every Gershgorin disc above a known g;
  * cg_ref: the projected conjugate gradient of the reference (fix_conp.cpp:864-930) in float128 (x86 long double), with the
    arithmetic of cg_init_kernel / cg_update_kernel; cg_f64: the same in float64 with numpy's pairwise sums, which exists only to
    measure how far an honest float64 implementation with another summation order lands from cg_ref (the e64 of error_bound);
  * the loop and launch structure of cg_row_dot, cg_step_kernel, launch_cg_step (conp_kernels.hip section 8) and of cg()
    (conp_fix.cpp) restated as arithmetic, so that the GPU module can assert that its sizes and cases reach what they claim."""
import collections
import concurrent.futures

import numpy as np

SIZES = (62, 130, 449, 961, 1025, 1664, 2049, 4096, 4097, 6151, 8200)
TILE = 128
KEEP_MAX = 4096               # cg_step_kernel keeps up to four elements per thread in registers up to here
LDS_DEFAULT = 64 * 1024       # dynamic LDS a kernel gets without asking
LDS_MAX = 128 * 1024          # cg_step_fits
G = 1.0                       # every Gershgorin disc of spd_matrix stays above this
SPREAD = 8.0                  # the diagonal lies in [G + 1, G + 1 + SPREAD]: sets the condition number
TOL_DEFAULT, TOL_TIGHT, TOL_NEVER = 1e-6, 1e-20, 1e-300
TOL_REF = 1e-26               # cg_ref "run to its floor": q* is taken here, 1000 times closer to the solution than the tight bound asks
LD = np.longdouble
U = 2.0 ** -53


# ---- the loop and launch structure ---------------------------------------------------------------------------------------------------
def lane_tiers(n, lane):
    """trip counts of cg_row_dot's three loops for one lane: dict(w16, w8, w1)"""
    j, w16, w8, w1 = lane, 0, 0, 0
    while j + 960 < n:
        j += 1024; w16 += 1
    while j + 448 < n:
        j += 512; w8 += 1
    while j < n:
        j += 64; w1 += 1
    return dict(w16=w16, w8=w8, w1=w1)


def lanes_with(n, **want):
    return [l for l in range(64) if all(lane_tiers(n, l)[k] == v for k, v in want.items())]


def rows_per_block(n):
    return 8 if n <= 4096 else 16


def n_workgroups(n):
    return (n + rows_per_block(n) - 1) // rows_per_block(n)


def last_workgroup_rows(n):
    return n - (n_workgroups(n) - 1) * rows_per_block(n)


def keeps_registers(n):
    return n <= KEEP_MAX


def lds_bytes(n):
    return 8 * n


Schedule = collections.namedtuple("Schedule", "two_launch batches iterations converged next_prev where")


def batch_schedule(prev_iters, iters_needed, maxiter):
    """the launches cg() issues for one solve in its one-launch-per-iteration form: `batches` is a list of lists of (iter, mode).
    prev_iters: the iteration count of the last solve of this handle that converged (8 on a new handle); iters_needed: the
    iteration at which the stop rule triggers (None: never).  `where` says where in its batch convergence fell: "last" (found by the
    mode-4 launch that ends a batch), "inside", or None; `next_prev` is what the next solve will be given as prev_iters."""
    if maxiter <= 1:                                         # the two-launch form with no iteration at all
        return Schedule(True, [], 0, False, prev_iters, None)
    batch = max(2, min(16, prev_iters))
    it, batches, cur = 1, [], [(1, 1)]
    while True:
        last = min(maxiter - 1, it + batch - 1)
        while it < last:
            it += 1
            cur.append((it, 2))
        cur.append((it, 4))
        batches.append(cur)
        done = iters_needed is not None and iters_needed <= it
        if done or it + 1 >= maxiter:
            break
        it += 1
        cur = [(it, 3)]
        batch = 4
    where = None
    if done:
        where = "last" if iters_needed == it else "inside"
    return Schedule(False, batches, iters_needed if done else it, done, iters_needed if done else prev_iters, where)


def check_sizes():
    """what each of SIZES is there for, asserted from the restated loop bounds and thresholds"""
    every = list(range(64))
    assert lanes_with(62, w1=1, w8=0, w16=0) == every[:62] and lanes_with(62, w1=0, w8=0, w16=0) == [62, 63]      # two empty lanes
    assert lanes_with(130, w1=3) == [0, 1] and lanes_with(130, w1=2, w8=0) == every[2:]
    assert lanes_with(449, w8=1, w1=0) == [0] and lanes_with(449, w8=0, w1=7) == every[1:]                    # the 8-wide tier split
    assert lanes_with(512, w8=1, w1=0, w16=0) == every
    assert lanes_with(961, w16=1, w8=0, w1=0) == [0] and lanes_with(961, w16=0, w8=1, w1=7) == every[1:]      # the 16-wide tier split
    assert lanes_with(1024, w16=1, w8=0, w1=0) == every
    assert lanes_with(1025, w16=1, w8=0, w1=1) == [0] and lanes_with(1025, w16=1, w8=0, w1=0) == every[1:]
    assert lanes_with(1664, w16=1, w8=1, w1=2) == every                                                       # 1024 + 512 + 128
    assert lanes_with(2049, w16=2, w8=0, w1=1) == [0] and lanes_with(2049, w16=2, w1=0) == every[1:]
    assert lanes_with(4096, w16=4, w8=0, w1=0) == every
    assert lanes_with(8200, w16=8, w8=0, w1=1) == every[:8] and lanes_with(8200, w16=8, w8=0, w1=0) == every[8:]
    assert [keeps_registers(n) for n in (4096, 4097)] == [True, False]
    assert (rows_per_block(4096), n_workgroups(4096), last_workgroup_rows(4096)) == (8, 512, 8)
    assert (rows_per_block(4097), n_workgroups(4097), last_workgroup_rows(4097)) == (16, 257, 1)
    assert (rows_per_block(6151), n_workgroups(6151), last_workgroup_rows(6151)) == (16, 385, 7)
    assert (rows_per_block(8200), n_workgroups(8200), last_workgroup_rows(8200)) == (16, 513, 8)
    assert {n: last_workgroup_rows(n) for n in (62, 130, 449, 961, 1025, 1664, 2049)} == {62: 6, 130: 2, 449: 1, 961: 1, 1025: 1,
                                                                                           1664: 8, 2049: 1}
    assert lds_bytes(8192) == LDS_DEFAULT < lds_bytes(8200) == 65600 <= LDS_MAX == lds_bytes(16384)
    assert all(lds_bytes(n) <= LDS_DEFAULT for n in SIZES if n != 8200)


def seed_matrix(ne):
    return 1000 + ne


def seed_vectors(ne):
    return 2000 + ne


# ---- matrices and vectors ------------------------------------------------------------------------------------------------------------
def n_tiles(ne):
    return (ne + TILE - 1) // TILE


def tile_scales(ne, seed):
    """[nb, nb] symmetric: the magnitude and sign of every tile, +-10^u with u uniform in [-1.75, 1.75]"""
    rng = np.random.default_rng(seed)
    nb = n_tiles(ne)
    t = rng.choice([-1.0, 1.0], size=(nb, nb)) * 10.0 ** rng.uniform(-1.75, 1.75, size=(nb, nb))
    t = np.triu(t) + np.triu(t, 1).T
    if nb >= 3:                                              # the extremes are there at every size: three and a half decades
        t[0, nb - 1] = t[nb - 1, 0] = 10.0 ** -1.75
        t[1, nb - 1] = t[nb - 1, 1] = -10.0 ** 1.75
    return t


def spd_matrix(ne, seed):
    """-> (A, g).  Off the diagonal A_ij = t_IJ h_ij / max_i R_i with h symmetric standard normal, t the tile scales and R_i the
    row's off-diagonal absolute sum, so that the largest such sum is 1.  A_ii = G + 1 + SPREAD v_i with v_i uniform in [0, 1]: the
    Gershgorin disc of row i is [A_ii - R_i, A_ii + R_i], and g = min_i (A_ii - R_i) >= G bounds the smallest eigenvalue from
    below, also on the zero-sum subspace.  The diagonal's range [G + 1, G + 1 + SPREAD] sets the condition number, and with it the
    iteration counts, at every size alike."""
    rng = np.random.default_rng(seed)
    H = rng.standard_normal((ne, ne))
    H = np.triu(H, 1)
    H += H.T
    t = tile_scales(ne, seed + 1)
    H *= np.repeat(np.repeat(t, TILE, axis=0), TILE, axis=1)[:ne, :ne]
    H /= np.abs(H).sum(axis=1).max()
    R = np.abs(H).sum(axis=1)
    d = G + 1.0 + SPREAD * rng.uniform(0.0, 1.0, size=ne)
    H[np.arange(ne), np.arange(ne)] = d
    g = float(np.min(d - R * (1.0 + 2.0 ** -20)))            # (the rounding of R's sum is far inside the 2^-20)
    assert g >= G
    return np.ascontiguousarray(H), g


MULTIPLIER = 2.0 ** -30


def vectors(A, seed):
    """the b vectors: two dense ones and a unit vector in the last column.  A dense one is A x0 + MULTIPLIER with x0 random of zero
    sum, so the residual b - A q of the constrained solution is the constant MULTIPLIER, not zero.  It is small on purpose: the
    kernels' lg = sum r^2 - netr ave cancels to about 2^-53 n MULTIPLIER^2 of rounding, which has to stay far below n * 1e-20 for
    the tight tolerance to be reachable in float64 and for the logged residuals to keep their six digits down to it."""
    ne = A.shape[0]
    rng = np.random.default_rng(seed)
    out = {}
    for name in ("dense", "dense2"):
        x0 = rng.standard_normal(ne)
        out[name] = matvec_f64(A, x0 - x0.mean()) + MULTIPLIER
    e = np.zeros(ne)
    e[ne - 1] = 1.0
    out["unit_last"] = e
    return out


# ---- the solver ----------------------------------------------------------------------------------------------------------------------
def matvec_ld(A, p, chunk=128):
    """A p in float128 by row chunks (no long-double copy of the matrix): a product of two doubles is rounded once (2^-64), numpy
    sums a row pairwise.  The chunks are spread over a few threads; each row's arithmetic does not depend on that."""
    assert np.finfo(LD).nmant >= 63, "no extended precision on this platform"
    n = A.shape[0]
    p = np.asarray(p, LD)
    out = np.zeros(n, LD)

    def rows(r):
        out[r:r + chunk] = (A[r:r + chunk].astype(LD) * p).sum(axis=1)
    starts = range(0, n, chunk)
    if n < 1024:
        for r in starts:
            rows(r)
    else:
        with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
            list(pool.map(rows, starts))
    return out


def matvec_f64(A, p, chunk=512):
    """A p in float64 with numpy's pairwise row sums (no BLAS: the same on every machine)"""
    n = A.shape[0]
    out = np.zeros(n)
    for r in range(0, n, chunk):
        out[r:r + chunk] = (A[r:r + chunk] * p).sum(axis=1)
    return out


Solve = collections.namedtuple("Solve", "q hist iterations net converged snaps")


def _cg(A, b, tol, maxiter, dtype, matvec, keep):
    n = len(b)
    res = np.asarray(b, dtype).copy()
    q = np.zeros(n, dtype)
    netr, l2 = res.sum(), (res * res).sum()
    ave = netr / n
    p = res - ave
    lr = l2 - netr * ave
    lg = lr
    hist, snaps, it, net, conv = [lr], {0: q.copy()}, 0, dtype(0), False
    for it in range(1, maxiter):
        ap = matvec(A, p)
        ptap = (p * ap).sum()
        alpha = lr / ptap
        gamma = lg
        q = q + alpha * p
        res = res - alpha * ap
        lg, netr = (res * res).sum(), res.sum()
        ave = netr / n
        lg = lg - netr * ave
        beta = lg / gamma
        p = beta * p + res - ave
        lr = (res * p).sum()
        hist.append(lr)
        if it in keep:
            snaps[it] = q.copy()
        if lr / n < tol:
            net, conv = q.sum(), True
            break
    return Solve(q, np.array(hist), it, net, conv, snaps)


def cg_ref(A, b, tol, maxiter, keep=()):
    """-> Solve(q, hist[0 .. iterations], iterations, net charge, converged, snaps): float128; hist[k] is the `res` of the log line
    of iteration k (hist[0]: the start value), snaps[k] the charges after iteration k for k in `keep`"""
    return _cg(A, b, tol, maxiter, LD, matvec_ld, keep)


def cg_f64(A, b, tol, maxiter, keep=(), matvec=matvec_f64):
    """the same algorithm in plain float64 numpy: measures e64, never compared with the GPU"""
    return _cg(A, b, tol, maxiter, np.float64, matvec, keep)


def needed(hist, n, tol, scale=1.0):
    """the iteration at which the stop rule triggers for scale * b, from the history of b (the iteration is linear in b up to the
    stop rule: the history scales with scale^2); None if it does not within the history"""
    for k in range(1, len(hist)):
        if float(hist[k]) * scale * scale / n < tol:
            return k
    return None


def scale_to_need(hist, n, tol, k):
    """a power of two s such that s * b stops at iteration k: the stop level n tol is put midway (in the logarithm) between
    s^2 hist[k - 1] and s^2 hist[k], as far from both as a power of two allows"""
    s2 = n * tol / np.sqrt(float(hist[k]) * float(hist[k - 1]))
    s = 2.0 ** round(0.5 * np.log2(s2))
    assert needed(hist, n, tol, s) == k
    return s


def kkt_solve(A, b):
    """the constrained minimum directly: [A 1; 1' 0] [q; lambda] = [b; 0], float64 LU with float128 residual refinement -> q float128"""
    n = len(b)
    K = np.zeros((n + 1, n + 1))
    K[:n, :n] = A
    K[:n, n] = K[n, :n] = 1.0
    rhs = np.zeros(n + 1, LD)
    rhs[:n] = b
    x = np.zeros(n + 1, LD)
    for _ in range(6):
        r = rhs - matvec_ld(K, x)
        x = x + np.linalg.solve(K, r.astype(np.float64))
    return x[:n]


def error_bound(e64, qmax):
    """the entry-wise bound of a solve cut off after k iterations: 16 x the float64 figure e64 = max |cg_f64 - cg_ref| measured on
    the CPU for the same matrix, vector and k, at least 16 x 2^-53 max|q|.  (The GPU's summation trees are not numpy's: 64-lane
    strided fma chains, wave and block reductions.)"""
    return max(16.0 * e64, 16.0 * U * qmax)


def sum_bound(ne, iterations, qmax):
    """|sum q| at rounding level.  Exactly, every direction p_k has zero sum and so has q = sum alpha_k p_k.  In float64 each element of
    p_k = beta p + r - ave is rounded three times and ave once, so |sum p_k| <= 4 n 2^-53 max|p_k| grows by that much per iteration
    (beta < 1 here), and q_i += alpha p_i rounds every element once more: per iteration at most 4 n 2^-53 max|q| in all"""
    return 4.0 * max(iterations, 1) * ne * U * qmax


def converged_bound(ne, tol, g=G):
    """||q - q*||_2 <= 2 sqrt(n tol) / g.  With r = b - A q and P the projection on the zero-sum vectors, P r = P A (q* - q) and
    q* - q has zero sum, so ||P r|| >= lambda_min ||q* - q|| >= g ||q* - q||; at the stop ||P r||^2 ~ lr < n tol, and the factor 2
    covers the drift between the recursive lr and the true projected residual"""
    return 2.0 * np.sqrt(ne * tol) / g


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# the iterations the dense vectors need at TOL_DEFAULT and TOL_TIGHT (tests/test_cg_ref_math.py pins them with the solvers above)
ITERS = {62: (9, 24), 130: (9, 25), 449: (9, 26), 961: (9, 26), 1025: (9, 26), 1664: (9, 26), 2049: (9, 26), 4096: (9, 26),
         4097: (9, 26), 6151: (9, 26), 8200: (9, 26)}
