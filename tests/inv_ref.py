"""Helpers of tests/test_gpu_inverse_sizes.py, none of which needs a GPU (tests/test_inv_ref_math.py checks them):
  * inverse_ld: the inverse in x86 long double (Gauss-Jordan with partial pivoting and one Newton step), for n <= LD_MAX;
  * matrices whose inverse is known in closed form at any n -- kms (rho^|i-j|, tridiagonal inverse), kms_general (rows and columns
    of it permuted and scaled by powers of two: the row permutation IS the pivot sequence), second_difference (the ill-conditioned
    positive definite one), kms_bumped (symmetric, every pivot positive but the last);
  * matrices whose inverse a correct elimination returns to the bit -- generalized_permutation, exchange, and block_diagonal, whose
    inverse has exact zeros outside its blocks;
  * panel_plan: the tier arithmetic of launch_inverse (conp_inverse.hip) restated, and pivot_places: where the pivots of a row
    permutation fall in the workgroups of that plan, so that a case can assert that it reaches what it names;
  * the cases of the GPU module by key (matrix, reference, e_lapack, bound), made once and cached."""
import collections
import functools

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
NB = 64                       # INV_NB: columns per block step
TILE = 128                    # inv_update_kernel's workgroup tile; ld = n rounded up to it
PC_MAXG = 256                 # most workgroups of the cooperative panel
PC_LD = NB + 1                # its LDS row stride
LDS_LIMIT = 150 * 1024        # launch_inverse: `lds <= 150 * 1024`
LD_MAX = 321                  # inverse_ld is used up to here (0.7 s; 7.6 s at n = 700)
RHO = 0.5


# ---- extended-precision inverse ------------------------------------------------------------------------------------------------------
def gauss_jordan(a, dtype):
    """unblocked Gauss-Jordan on [A | I] with partial pivoting (first largest |value|, like idamax) -> (inverse, pivot rows)"""
    a = np.asarray(a)
    n = a.shape[0]
    m = np.zeros((n, 2 * n), dtype)
    m[:, :n] = a
    m[np.arange(n), n + np.arange(n)] = 1
    piv = np.zeros(n, np.int64)
    for j in range(n):
        p = j + int(np.argmax(np.abs(m[j:, j])))
        piv[j] = p
        if m[p, j] == 0 or not np.isfinite(m[p, j]):
            raise ZeroDivisionError(f"no pivot in column {j}")
        if p != j:
            m[[j, p]] = m[[p, j]]
        m[j] = m[j] / m[j, j]
        f = m[:, j].copy()
        f[j] = 0
        m -= f[:, None] * m[j][None, :]
    return m[:, n:].copy(), piv


def inverse_ld(a):
    """long double Gauss-Jordan with partial pivoting, then one Newton step X + X (I - A X) in long double"""
    assert np.finfo(LD).nmant >= 63, "no extended precision on this platform"
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert a.shape[0] <= LD_MAX, a.shape
    al = a.astype(LD)
    x, _piv = gauss_jordan(al, LD)
    r = np.eye(a.shape[0], dtype=LD) - al @ x
    return x + x @ r


# ---- closed forms --------------------------------------------------------------------------------------------------------------------
def kms(n, rho=RHO):
    """rho^|i-j| (Kac-Murdock-Szego): symmetric positive definite, condition number below ((1 + rho) / (1 - rho))^2 = 9 at rho = 0.5,
    where every entry is a power of two (zero beyond |i-j| = 1074)"""
    i = np.arange(n)
    return np.ascontiguousarray(np.float64(rho) ** np.abs(i[:, None] - i[None, :]).astype(np.float64))


def kms_inverse(n, rho=RHO):
    """tridiagonal: (1 + rho^2) / (1 - rho^2) on the diagonal, 1 / (1 - rho^2) at its two ends, -rho / (1 - rho^2) beside it"""
    r = LD(rho)
    out = np.zeros((n, n), LD)
    if n == 1:
        out[0, 0] = 1
        return out
    d = 1 - r * r
    i = np.arange(n)
    out[i, i] = (1 + r * r) / d
    out[0, 0] = out[n - 1, n - 1] = 1 / d
    out[i[:-1], i[:-1] + 1] = out[i[:-1] + 1, i[:-1]] = -r / d
    return out


def _pow2(e, n):
    return np.ones(n) if e is None else 2.0 ** np.asarray(e, np.float64)


def kms_general(n, rho=RHO, row_perm=None, col_perm=None, row_pow2=None, col_pow2=None):
    """D_r P K Q D_c: entry (i, j) is 2^row_pow2[i] K[row_perm[i], col_perm[j]] 2^col_pow2[j]; exact in float64 at rho = 0.5"""
    rp = np.arange(n) if row_perm is None else np.asarray(row_perm)
    cp = np.arange(n) if col_perm is None else np.asarray(col_perm)
    a = kms(n, rho)[np.ix_(rp, cp)] * _pow2(row_pow2, n)[:, None] * _pow2(col_pow2, n)[None, :]
    return np.ascontiguousarray(a)


def kms_general_inverse(n, rho=RHO, row_perm=None, col_perm=None, row_pow2=None, col_pow2=None):
    """D_c^-1 Q' K^-1 P' D_r^-1: exact permutations and exact scalings of the closed form"""
    rp = np.arange(n) if row_perm is None else np.asarray(row_perm)
    cp = np.arange(n) if col_perm is None else np.asarray(col_perm)
    b = kms_inverse(n, rho)[np.ix_(cp, rp)]
    return b / _pow2(col_pow2, n).astype(LD)[:, None] / _pow2(row_pow2, n).astype(LD)[None, :]


def second_difference(n):
    """tridiag(-1, 2, -1): positive definite, condition number 4 (n + 1)^2 / pi^2 (2.5e6 at n = 2500)"""
    a = 2.0 * np.eye(n)
    i = np.arange(n - 1)
    a[i, i + 1] = a[i + 1, i] = -1.0
    return a


def second_difference_inverse(n):
    """min(i, j) (n + 1 - max(i, j)) / (n + 1), i and j counted from 1"""
    i = np.arange(1, n + 1).astype(LD)
    return np.minimum(i[:, None], i[None, :]) * (n + 1 - np.maximum(i[:, None], i[None, :])) / LD(n + 1)


BUMP = -0.875                 # kms_bumped: a_nn = 0.125, last Schur pivot a_nn - rho^2 = -0.125


def kms_bumped(n, rho=RHO, delta=BUMP):
    """K + delta e_n e_n': symmetric; the Schur pivots are 1, 1 - rho^2, ..., 1 - rho^2 and last 1 + delta - rho^2"""
    a = kms(n, rho)
    a[n - 1, n - 1] += delta
    return a


def kms_bumped_inverse(n, rho=RHO, delta=BUMP):
    """Sherman-Morrison: K^-1 - delta (K^-1 e_n)(K^-1 e_n)' / (1 + delta (K^-1)_nn)"""
    k = kms_inverse(n, rho)
    u = k[:, n - 1].copy()
    return k - LD(delta) * u[:, None] * u[None, :] / (1 + LD(delta) * k[n - 1, n - 1])


# ---- exact cases ---------------------------------------------------------------------------------------------------------------------
def generalized_permutation(n, perm, exponents, signs=None):
    """entry (i, perm[i]) = signs[i] 2^exponents[i], |exponent| <= 20: every multiplier of an elimination is an exact zero and every
    reciprocal a power of two"""
    exponents = np.asarray(exponents)
    assert np.abs(exponents).max() <= 20 and sorted(perm) == list(range(n))
    a = np.zeros((n, n))
    a[np.arange(n), perm] = (np.ones(n) if signs is None else np.asarray(signs, np.float64)) * 2.0 ** exponents.astype(np.float64)
    return a


def generalized_permutation_inverse(a):
    """the transposed pattern with reciprocal entries (float64: exact)"""
    out = np.zeros_like(a.T)
    nz = a.T != 0
    out[nz] = 1.0 / a.T[nz]
    return out


def exchange(n):
    """the anti-diagonal matrix: symmetric, M[0][0] = 0 (for n > 1), its own inverse; every pivot comes from the current last rows"""
    return np.ascontiguousarray(np.eye(n)[::-1])


BLOCK_SIZES = (50, 100, 43)   # boundaries at 50, 150, 193: none a multiple of 64


def block_mask(sizes):
    n = sum(sizes)
    mask = np.zeros((n, n), bool)
    o = 0
    for s in sizes:
        mask[o:o + s, o:o + s] = True
        o += s
    return mask


def block_diagonal(sizes=BLOCK_SIZES, seed=77):
    """dense symmetric positive definite blocks G G' / s + I (condition number below 10) on the diagonal, exact zeros elsewhere"""
    rng = np.random.default_rng(seed)
    n = sum(sizes)
    a = np.zeros((n, n))
    o = 0
    for s in sizes:
        g = rng.standard_normal((s, s))
        a[o:o + s, o:o + s] = spd_from(g)
        o += s
    return a


def block_diagonal_inverse(a, sizes=BLOCK_SIZES):
    out = np.zeros(a.shape, LD)
    o = 0
    for s in sizes:
        out[o:o + s, o:o + s] = inverse_ld(a[o:o + s, o:o + s])
        o += s
    return out


def spd_from(g):
    """G G' / n + I, symmetrised exactly"""
    n = g.shape[0]
    a = g @ g.T / n + np.eye(n)
    return np.ascontiguousarray((a + a.T) / 2)


# ---- launch_inverse's panel tiers ----------------------------------------------------------------------------------------------------
Panel = collections.namedtuple("Panel", "k0 m nbw rpw G lds coop")


def panel_plan(n, num_cus=256, max_wg=0):
    """per 64-column panel of the pivoted elimination: rows m = n - k0 below its top, width nbw, rows per workgroup rpw, workgroups
    G, dynamic LDS bytes of the cooperative kernel and whether that form is eligible (lds <= 150 KB, G <= num_cus).  max_wg is
    CONP_PANEL_MAXG (0: none)."""
    ncu = num_cus if num_cus > 0 else 1
    cap = max_wg if max_wg > 0 else PC_MAXG
    out = []
    for k0 in range(0, n, NB):
        m = n - k0
        maxg = min(ncu, PC_MAXG)
        if 1 <= cap < maxg:
            maxg = cap
        rpw = (m + maxg - 1) // maxg
        rpw = 64 if rpw < 64 else (rpw + 15) // 16 * 16
        G = (m + rpw - 1) // rpw
        lds = (rpw * PC_LD + NB + 4) * 8 + 8 * 4
        out.append(Panel(k0, m, min(NB, m), rpw, G, lds, lds <= LDS_LIMIT and G <= ncu))
    return out


def leading_dimension(n):
    return (n + TILE - 1) // TILE * TILE


def pivot_sequence(row_perm):
    """the rows a partial-pivoting elimination of K[row_perm, :] takes (absolute, as LAPACK's ipiv counted from 0): in column j the
    row that holds row j of K, wherever the swaps so far have left it"""
    cur = np.asarray(row_perm).copy()          # cur[position] = row of K now there
    pos = np.argsort(cur)                      # pos[row of K] = position
    piv = np.zeros(len(cur), np.int64)
    for j in range(len(cur)):
        p = pos[j]
        piv[j] = p
        other = cur[j]
        cur[j], cur[p] = j, other
        pos[j], pos[other] = j, p
    return piv


PLACES = ("self", "same_wg", "other_wg", "last_ragged_wg", "ragged_single_row", "only_row_left")


def pivot_places(piv, plan):
    """-> {place: [columns]}.  For column j of panel k0 the cooperative kernel's workgroup w holds panel rows [w rpw, (w + 1) rpw):
    row j itself is always in workgroup 0 (rpw >= 64).  `last_ragged_wg`: the winner is in the last workgroup, which holds fewer
    than rpw rows; `ragged_single_row`: that workgroup holds one row; `only_row_left`: no other candidate exists (j = n - 1)."""
    n = len(piv)
    out = {k: [] for k in PLACES}
    for pl in plan:
        last_rows = pl.m - (pl.G - 1) * pl.rpw
        for j in range(pl.k0, pl.k0 + pl.nbw):
            p = int(piv[j])
            w = (p - pl.k0) // pl.rpw
            if p == j:
                out["self"].append(j)
            elif w == 0:
                out["same_wg"].append(j)
            else:
                out["other_wg"].append(j)
            if pl.G > 1 and w == pl.G - 1 and last_rows < pl.rpw:
                out["last_ragged_wg"].append(j)
                if last_rows == 1:
                    out["ragged_single_row"].append(j)
            if j == n - 1:
                out["only_row_left"].append(j)
    return out


def row_perms(n, seed=None):
    """the row permutations of the pivot cases: name -> perm (row i of the matrix is row perm[i] of K).  A transposition that
    degenerates to the identity at this n is left out."""
    ident = np.arange(n)

    def swap(a, b):
        p = ident.copy()
        p[a], p[b] = b, a
        return p
    out = {"identity": ident, "reversal": ident[::-1].copy(), "shift": np.roll(ident, 1)}
    for name, (a, b) in (("swap_63_64", (63, 64)), ("swap_0_last", (0, n - 1)), ("swap_64_last", (64, n - 1)), ("swap_1_2", (1, 2))):
        if a != b and max(a, b) < n:
            out[name] = swap(a, b)
    out["random"] = np.random.default_rng(4000 + n if seed is None else seed).permutation(n)
    return out


# ---- errors and bounds ---------------------------------------------------------------------------------------------------------------
def rel_error(got, ref):
    """max |got - ref| / max |ref|"""
    return float(np.max(np.abs(np.asarray(got, LD) - ref)) / np.max(np.abs(ref)))


def tile_errors(got, ref):
    """[T, T]: max |got - ref| / max |ref| over each 128 x 128 tile of the output"""
    n = ref.shape[0]
    t = (n + TILE - 1) // TILE
    d = np.zeros((t * TILE, t * TILE), LD)
    d[:n, :n] = np.abs(np.asarray(got, LD) - ref)
    return (d.reshape(t, TILE, t, TILE).max(axis=(1, 3)) / np.max(np.abs(ref))).astype(np.float64)


def tile_report(te, bound):
    """fraction of the bound in the first tile, the last tile, the rest of the last row and column of tiles (the ragged ones when n is
    no multiple of 128) and the interior; and the worst tile by name"""
    t = te.shape[0]
    groups = {"first": te[0, 0], "last": te[t - 1, t - 1]}
    if t > 1:
        groups["last_row"] = te[t - 1, :t - 1].max()
        groups["last_col"] = te[:t - 1, t - 1].max()
    if t > 2:
        inner = te[:t - 1, :t - 1].copy()
        inner[0, 0] = 0.0
        groups["interior"] = inner.max()
    i, j = np.unravel_index(np.argmax(te), te.shape)
    return {k: float(v) / bound for k, v in groups.items()}, f"tile ({i}, {j}) of {t} x {t}: {float(te[i, j]) / bound:.3f} of the bound"


def error_bound(n, e_lapack):
    """16 x max(e_lapack, n 2^-53): e_lapack is max |inv - ref| / max |ref| of np.linalg.inv (dgetrf / dgetri, what the reference
    program calls) for the same matrix; an entry of the inverse is the end of n rank-one contributions, each rounded once: the
    floor; 16 is the margin the CG module gives the GPU's summation order over float64 numpy"""
    return 16.0 * max(e_lapack, n * U)


# ---- the cases of the GPU module, by key ---------------------------------------------------------------------------------------------
EDGE_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 321)
PIVOT_SIZES = (65, 129, 200, 321)
TIERS = ((700, 5), (1100, 4), (1200, 4), (2500, 0))            # (n, CONP_PANEL_MAXG)


def _seed(kind, n):
    return {"spd": 5000, "gauss": 6000, "scaled": 7000, "ulp": 8000}[kind] + n


def _scaled_args(n):
    rng = np.random.default_rng(_seed("scaled", n))
    return dict(row_perm=rng.permutation(n), col_perm=rng.permutation(n), row_pow2=rng.choice([-3, 3], size=n),
                col_pow2=rng.choice([-3, 3], size=n))


@functools.lru_cache(maxsize=4)
def _matrix_large(key):
    return _make_matrix(key)


@functools.lru_cache(maxsize=None)
def _matrix_small(key):
    return _make_matrix(key)


def matrix(key):
    """the float64 matrix of a case: ("kms", n), ("second_difference", n), ("kms_bumped", n), ("spd", n), ("gauss", n),
    ("pivot", n, name of a row permutation), ("scaled", n), ("ulp", n), ("block_diagonal",).  Treat it as read-only."""
    m = (_matrix_small if _size(key) <= LD_MAX else _matrix_large)(key)
    m.setflags(write=False)
    return m


def _size(key):
    return sum(BLOCK_SIZES) if key[0] == "block_diagonal" else key[1]


def _make_matrix(key):
    kind = key[0]
    if kind == "block_diagonal":
        return block_diagonal()
    n = key[1]
    if kind == "kms":
        return kms(n)
    if kind == "second_difference":
        return second_difference(n)
    if kind == "kms_bumped":
        return kms_bumped(n)
    if kind == "spd":
        return spd_from(np.random.default_rng(_seed(kind, n)).standard_normal((n, n)))
    if kind == "gauss":
        return np.random.default_rng(_seed(kind, n)).standard_normal((n, n))
    if kind == "pivot":
        return kms_general(n, row_perm=row_perms(n)[key[2]])
    if kind == "scaled":
        return kms_general(n, **_scaled_args(n))
    if kind == "ulp":                                           # positive definite but for one ulp in one entry above the diagonal
        a = spd_from(np.random.default_rng(_seed(kind, n)).standard_normal((n, n)))
        a[n - 2, n - 1] = np.nextafter(a[n - 2, n - 1], np.inf)
        return a
    raise KeyError(key)


def _make_reference(key):
    kind = key[0]
    if kind == "block_diagonal":
        return block_diagonal_inverse(matrix(key))
    n = key[1]
    if kind == "kms":
        return kms_inverse(n)
    if kind == "second_difference":
        return second_difference_inverse(n)
    if kind == "kms_bumped":
        return kms_bumped_inverse(n)
    if kind == "pivot":
        return kms_general_inverse(n, row_perm=row_perms(n)[key[2]])
    if kind == "scaled":
        return kms_general_inverse(n, **_scaled_args(n))
    return inverse_ld(matrix(key))                              # the dense ones: n <= LD_MAX


@functools.lru_cache(maxsize=2)
def _reference_large(key):
    return _make_reference(key)


@functools.lru_cache(maxsize=None)
def _reference_small(key):
    return _make_reference(key)


def reference(key):
    """the long double inverse of matrix(key): closed form where there is one, inverse_ld otherwise.  Cached; read-only."""
    r = (_reference_small if _size(key) <= LD_MAX else _reference_large)(key)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def e_lapack(key):
    return rel_error(np.linalg.inv(matrix(key)), reference(key))


def bound(key):
    return error_bound(_size(key), e_lapack(key))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
