"""Host restatement of the lattice form of the solve (conp_host.cpp find_lattice, conp_kernels.hip lat_gemv_kernel) for
tests/test_gpu_solve_lattice.py: the translation search with numpy, the launch shape and its counted rounding chain, and exactly
block-circulant matrices."""
import numpy as np

U = 2.0 ** -53
TOL = 1e-4                    # A: the matching tolerance of the search
LDS = 65536                   # bytes the table slab and the b vector of one basis atom may take
LDS_MAX = 147456              # bytes of a stage
THREADS = 512


def system(ncx, ncy, layers=1, seed=12345):
    from conp_amd import systems
    return systems.synthetic_fast(ncx, ncy, lz=80, n_elyte=256, layers=layers, cutoff=8.0, g_ewald=0.35, accuracy_relative=1e-6,
                                  seed=seed)


def _perm(x, shift, lx, ly):
    """p with x[p[i]] = x[i] + shift (periodic in x and y, within TOL), or None when the set does not map onto itself"""
    d = x[None, :, :] - (x[:, None, :] + np.asarray(shift)[None, None, :])
    d[:, :, 0] -= lx * np.round(d[:, :, 0] / lx)
    d[:, :, 1] -= ly * np.round(d[:, :, 1] / ly)
    ok = (np.abs(d) < TOL).all(axis=2)
    if not ((ok.sum(axis=1) == 1).all() and (ok.sum(axis=0) == 1).all()):
        return None
    return ok.argmax(axis=1)


def _smallest(x, axis, lx, ly):
    """the smallest translation along `axis` that maps the atoms onto themselves, from the atoms in line with atom 0"""
    L = (lx, ly)[axis]
    o = 1 - axis
    d = x - x[0]
    d[:, 0] -= lx * np.round(d[:, 0] / lx)
    d[:, 1] -= ly * np.round(d[:, 1] / ly)
    line = (np.abs(d[:, o]) < TOL) & (np.abs(d[:, 2]) < TOL)
    cand = np.sort(np.mod(d[line, axis], L))
    cand = cand[(cand > TOL) & (cand < L - TOL)]
    for t in list(cand) + [L]:
        n = int(round(L / t))
        if n < 1 or abs(n * t - L) > TOL:
            continue
        shift = [0.0, 0.0, 0.0]
        shift[axis] = L / n
        p = _perm(x, shift, lx, ly)
        if p is not None:
            return L / n, n, p
    raise AssertionError("the identity was not found")


def find(x, lx, ly):
    """x: electrode positions in eleall order.  dict(a, b, nx, ny, nbasis, px, py, basis, row[beta, cx, cy], beta[i], cx[i], cy[i])"""
    x = np.asarray(x, float)
    ne = len(x)
    a, nx, px = _smallest(x, 0, lx, ly)
    b, ny, py = _smallest(x, 1, lx, ly)
    nbasis = ne // (nx * ny)
    # cell (0, 0) is atom 0's: the atoms within [0, a) x [0, b) of it (a margin of 10 TOL below), by eleall index
    m = 10 * TOL
    dx = np.mod(x[:, 0] - x[0, 0] + m, lx)
    dy = np.mod(x[:, 1] - x[0, 1] + m, ly)
    basis = np.nonzero((dx < a) & (dy < b))[0]
    assert len(basis) == nbasis and basis[0] == 0
    row = np.zeros((nbasis, nx, ny), np.int64)
    cur = basis.copy()
    for cx in range(nx):
        c = cur.copy()
        for cy in range(ny):
            row[:, cx, cy] = c
            c = py[c]
        cur = px[cur]
    beta = np.full(ne, -1); cxs = np.full(ne, -1); cys = np.full(ne, -1)
    bb, xx, yy = np.meshgrid(np.arange(nbasis), np.arange(nx), np.arange(ny), indexing="ij")
    beta[row.ravel()] = bb.ravel(); cxs[row.ravel()] = xx.ravel(); cys[row.ravel()] = yy.ravel()
    return dict(a=a, b=b, nx=nx, ny=ny, nbasis=nbasis, px=px, py=py, basis=basis, row=row, beta=beta, cx=cxs, cy=cys)


def check_maps(lat, ne):
    """the (basis, cell) -> row map is a bijection and the two generators commute"""
    assert np.array_equal(np.sort(lat["row"].ravel()), np.arange(ne))
    assert (lat["beta"] >= 0).all()
    px, py = lat["px"], lat["py"]
    assert np.array_equal(px[py], py[px])
    assert np.array_equal(np.sort(px), np.arange(ne)) and np.array_equal(np.sort(py), np.arange(ne))
    r = lat["row"]
    assert np.array_equal(px[r], np.roll(r, -1, axis=1)) and np.array_equal(py[r], np.roll(r, -1, axis=2))


def shape(nx, ny, nb, stage_cap=0):
    """the launch shape lat_gemv takes (conp_kernels.hip lat_shape): dict(R, sy, G, CB) or None when a stage does not fit"""
    R = 4 if ny % 4 == 0 else 1
    sy = ny + 2 if R == 4 else ny | 1
    if 16 * nx * sy > LDS:
        sy = ny
    if 16 * nx * sy > LDS or nx * ny < 16:
        return None
    G = min(nb, LDS_MAX // (16 * nx * sy))
    if stage_cap > 0:
        G = min(G, stage_cap)
    ncell = nx * ny
    CB = R
    while 2 * CB <= 64 * R and 2 * CB <= ncell and nb * -(-ncell // (2 * CB)) >= 256:
        CB *= 2
    return dict(R=R, sy=sy, G=G, CB=CB)


def chain(nx, ny, nb, stage_cap=0):
    """the longest chain of dependent roundings of a term: a thread's fmas (the first one rounds the product, every later one the
    running sum; part 0 takes the most items of every stage), the shuffle-adds over the parts of a wavefront, and the fixed tree
    ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)) over the eight wavefronts"""
    s = shape(nx, ny, nb, stage_cap)
    nrg = s["CB"] // s["R"]
    P = THREADS // nrg
    items = sum(-(-min(s["G"], nb - g0) * nx // P) for g0 in range(0, nb, s["G"]))
    return items * ny + int(np.log2(64 // nrg)) + 3


def circulant_table(lat, seed):
    """T[beta, beta', dx, dy] of small integers times powers of two with T[b, b', d] = T[b', b, -d]: the matrix below is exactly
    symmetric and exactly block-circulant, and every sum of two of its entries is exact"""
    nb, nx, ny = lat["nbasis"], lat["nx"], lat["ny"]
    rng = np.random.default_rng(seed)
    t = rng.integers(-8, 9, size=(nb, nb, nx, ny)).astype(float)
    neg = np.roll(np.flip(t, axis=(2, 3)), 1, axis=(2, 3))            # neg[b, b', d] = t[b, b', -d]
    t = t + neg.transpose(1, 0, 2, 3)
    e = rng.integers(-6, 7, size=nb)
    return t * np.exp2(e[:, None] + e[None, :])[:, :, None, None]


def circulant_matrix(lat, T):
    b, cx, cy = lat["beta"], lat["cx"], lat["cy"]
    nx, ny = lat["nx"], lat["ny"]
    return T[b[:, None], b[None, :], (cx[None, :] - cx[:, None]) % nx, (cy[None, :] - cy[:, None]) % ny]


def ref_product(M, b):
    """(M b in float128, A_i = sum_j |M_ij| |b_j|): x86 long double, its own error below 0.01 * 2^-53 * A_i"""
    assert np.finfo(np.longdouble).nmant >= 63, "no extended precision on this platform"
    n = M.shape[0]
    bl = np.asarray(b, np.longdouble)
    ref, A = np.zeros(n, np.longdouble), np.zeros(n)
    for r in range(0, n, 256):
        P = M[r:r + 256].astype(np.longdouble) * bl
        ref[r:r + 256] = P.sum(axis=1)
        A[r:r + 256] = np.abs(P).sum(axis=1).astype(np.float64)
    return ref, A


def mixed_vector(ne, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(ne) * np.exp2(rng.integers(-20, 21, size=ne))
