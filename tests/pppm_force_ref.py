"""numpy reference of the PPPM reciprocal-space forces, energy, virial and per-atom energies with ik differentiation (DESIGN.md
section 13), straight from the definitions: np.fft for the transforms, the oracle's own tables (rho_coeff, greensfn of
oracle_py.Pppm) and a stencil of its own.  tests/test_pppm_force_math.py checks the stencil against the oracle's bricks and potentials
and measures the mesh error against the exact sum (tests/ewald_force_ref.py) before the GPU tests use this module to judge
conp_pppm_compute_forces.

Like PPPM::poisson_ik the reference does FOUR backward transforms and keeps their real parts; the library packs two fields into
one complex transform after zeroing each gradient's own-axis Nyquist plane.  That the two agree to rounding is part of what the GPU
tests show."""
import ctypes as C

import numpy as np

OFFSET = 16384


def tables(lib, pp, s, mesh, order):
    """everything the definitions need for a system `s` on `mesh` at stencil `order`; pp: an oracle_py.Pppm of the same arguments"""
    from conp_amd import systems
    nx, ny, nz = (int(m) for m in mesh)
    dp = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
    lib.orc_pppm_tables.argtypes = [C.c_void_p, dp, dp]
    lib.orc_pppm_tables.restype = None
    rc, gf = np.zeros(order * order), np.zeros(nx * ny * nz)
    lib.orc_pppm_tables(pp.h, rc, gf)
    prd = np.array([s.prd[0], s.prd[1], s.prd[2] * s.slab_volfactor], float)
    delinv = np.array([nx, ny, nz]) / prd
    return dict(mesh=(nx, ny, nz), order=order, nlower=-((order - 1) // 2), shift=OFFSET + 0.5 if order % 2 else float(OFFSET),
                shiftone=0.0 if order % 2 else 0.5, delinv=delinv, delvolinv=delinv[0] * delinv[1] * delinv[2],
                boxlo=np.asarray(s.boxlo, float), prd=prd, V=float(prd.prod()), g=float(s.g_ewald), qs=systems.QQRD2E,
                slab=bool(s.slabflag), L=float(prd[2]), rho_coeff=rc.reshape(order, order), greensfn=gf.reshape(nz, ny, nx))


def stencil(x, T):
    """(mesh indices [n][3][order], wrapped; weights [n][3][order]) of the atoms at x: particle_map + compute_rho1d"""
    o = T["order"]
    xs = (np.asarray(x, float) - T["boxlo"]) * T["delinv"]
    g = (xs + T["shift"]).astype(np.int64) - OFFSET
    dx = g + T["shiftone"] - xs
    w = np.zeros(x.shape + (o,))
    for k in range(o):
        r = np.zeros(x.shape)
        for l in range(o - 1, -1, -1):
            r = T["rho_coeff"][l, k] + r * dx
        w[..., k] = r
    idx = (g[..., None] + T["nlower"] + np.arange(o)) % np.array(T["mesh"])[None, :, None]
    return idx, w


def _points(idx, w, a):
    """flattened (z, y, x) indices and weight products of the order^3 stencil points of the atoms a"""
    iz, iy, ix = idx[a, 2][:, :, None, None], idx[a, 1][:, None, :, None], idx[a, 0][:, None, None, :]
    wz, wy, wx = w[a, 2][:, :, None, None], w[a, 1][:, None, :, None], w[a, 0][:, None, None, :]
    shape = np.broadcast(iz, iy, ix).shape
    return (np.broadcast_to(iz, shape), np.broadcast_to(iy, shape), np.broadcast_to(ix, shape)), wz, wy, wx


def spread(x, q, T, chunk=4096):
    """density brick [nz][ny][nx] of the charged atoms (make_rho)"""
    nx, ny, nz = T["mesh"]
    rho = np.zeros((nz, ny, nx))
    src = np.nonzero(q != 0)[0]
    idx, w = stencil(x[src], T)
    for a0 in range(0, len(src), chunk):
        a = np.arange(a0, min(a0 + chunk, len(src)))
        pts, wz, wy, wx = _points(idx, w, a)
        val = ((T["delvolinv"] * q[src[a]])[:, None, None, None] * wz) * wy * wx
        np.add.at(rho, pts, val)
    return rho


def gather(bricks, x, T, chunk=4096):
    """sum over the stencil of w * brick for every brick, at the atoms x: [len(bricks)][n]"""
    idx, w = stencil(x, T)
    out = np.zeros((len(bricks), len(x)))
    for a0 in range(0, len(x), chunk):
        a = np.arange(a0, min(a0 + chunk, len(x)))
        pts, wz, wy, wx = _points(idx, w, a)
        ww = (wz * wy) * wx
        for b, brick in enumerate(bricks):
            out[b, a] = (ww * brick[pts]).sum(axis=(1, 2, 3))
    return out


def kvectors(T):
    """(kx [nx], ky [ny], kz [nz]): 2 pi / L times m = i - n floor(2 i / n)"""
    out = []
    for n, L in zip(T["mesh"], T["prd"]):
        i = np.arange(n)
        out.append(2 * np.pi / L * (i - n * (2 * i // n)))
    return out


def solve(rho, T):
    """the mesh part: dict(esum = (V / 2) sum G |rho^|^2 / N^2, wsum[6] likewise with the virial weights, u = the mesh potential
    brick, field = the three field bricks); without qqrd2e"""
    nx, ny, nz = T["mesh"]
    N = nx * ny * nz
    kx, ky, kz = kvectors(T)
    KZ, KY, KX = np.meshgrid(kz, ky, kx, indexing="ij")
    rh = np.fft.fftn(rho)
    G = T["greensfn"]
    ek = 0.5 * T["V"] * G * (rh.real ** 2 + rh.imag ** 2) / (float(N) * N)
    k2 = KX * KX + KY * KY + KZ * KZ
    with np.errstate(divide="ignore", invalid="ignore"):
        vt = np.where(k2 > 0, -2.0 * (1.0 / k2 + 0.25 / T["g"] ** 2), 0.0)
    ek = np.where(k2 > 0, ek, 0.0)
    K = (KX, KY, KZ)
    wsum = np.array([(ek * (1.0 + vt * K[a] * K[b])).sum() if a == b else (ek * vt * K[a] * K[b]).sum()
                     for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))])
    phi = G * rh                                   # ifftn divides by N
    u = np.fft.ifftn(phi).real
    field = [np.fft.ifftn(-1j * k * phi).real for k in K]        # E = - grad u; the real part as PPPM::poisson_ik keeps it
    return dict(esum=float(ek.sum()), wsum=wsum, u=u, field=field, k2sum=float((ek * (1.0 - k2 / (2 * T["g"] ** 2))).sum()))


def energy_virial(sol, x, q, T):
    g, V = T["g"], T["V"]
    Q, Q2 = q.sum(), (q * q).sum()
    E = sol["esum"] - g * Q2 / np.sqrt(np.pi) - 0.5 * np.pi * Q * Q / (g * g * V)
    if T["slab"]:
        M, M2, L = (q * x[:, 2]).sum(), (q * x[:, 2] ** 2).sum(), T["L"]
        E += 2 * np.pi * (M * M - Q * M2 - Q * Q * L * L / 12.0) / V
    return T["qs"] * E, T["qs"] * sol["wsum"]


def forces_eatom(sol, x, q, T, targets):
    """f_i and e_i of the atoms `targets`; x, q: every owned atom (the slab sums run over all of them)"""
    targets = np.asarray(targets)
    g, V = T["g"], T["V"]
    ex, ey, ez, u = gather(sol["field"] + [sol["u"]], x[targets], T)
    qt, zt = q[targets], x[targets, 2]
    Q = q.sum()
    f = np.stack([ex, ey, ez], 1) * qt[:, None]
    e = 0.5 * qt * u - g * qt * qt / np.sqrt(np.pi) - 0.5 * np.pi * qt * Q / (g * g * V)
    if T["slab"]:
        M, M2, L = (q * x[:, 2]).sum(), (q * x[:, 2] ** 2).sum(), T["L"]
        f[:, 2] += (-4 * np.pi / V) * qt * (M - Q * zt)
        e += (2 * np.pi / V) * qt * (zt * M - 0.5 * (M2 + Q * zt * zt) - Q * L * L / 12.0)
    f[qt == 0] = 0.0
    e[qt == 0] = 0.0
    return T["qs"] * f, T["qs"] * e


def reference(lib, s, at, mesh, order, targets=None, fast=True):
    """(f, E, W, e, scale, T) of the owned atoms of `at` (forces and eatom at `targets`, default all)"""
    import oracle_py
    pp = oracle_py.Pppm(lib, s, mesh, order, fast=fast)
    T = tables(lib, pp, s, mesh, order)
    pp.close()
    n = at.nlocal
    x, q = np.ascontiguousarray(at.x[:n]), np.ascontiguousarray(at.q[:n])
    sol = solve(spread(x, q, T), T)
    E, W = energy_virial(sol, x, q, T)
    f, e = forces_eatom(sol, x, q, T, np.arange(n) if targets is None else targets)
    return f, E, W, e, T["qs"] * sol["esum"], T


# The mesh error of THIS reference against the exact Ewald sum (tests/ewald_force_ref.py over the host k tables), measured on the CPU
# by tests/test_pppm_force_math.py with the electrode charges the oracle's pre_force leaves: (deck, mode, mesh, order) ->
# (RMS force error / RMS |f|, |E - E_exact| / unsubtracted scale).  The GPU tests allow the library twice these against the exact sum.
ROWS = [("dilute", "ffield", (27, 24, 144), 5), ("il_onelayer", "ffield", (36, 40, 150), 4), ("dilute", "ffield", (32, 25, 160), 7),
        ("dilute", "slab", (27, 24, 432), 5)]
MEASURED = {
    ("dilute", "ffield", (27, 24, 144), 5): (1.379e-4, 1.258e-5),
    ("il_onelayer", "ffield", (36, 40, 150), 4): (9.483e-5, 8.817e-6),
    ("dilute", "ffield", (32, 25, 160), 7): (7.432e-5, 1.698e-5),
    ("dilute", "slab", (27, 24, 432), 5): (4.493e-4, 1.027e-4),
}


def exact(s, x, q, T, targets):
    """(f, E, W, e, scale) of the exact Ewald sum over the host k tables of `s` (tests/ewald_force_ref.py)"""
    import ewald_force_ref as eref
    from conp_amd import capi
    kt = capi.host_ktables(s)
    kv = np.stack([kt["kxvecs"], kt["kyvecs"], kt["kzvecs"]], 1) * (2 * np.pi / T["prd"])
    S = eref.structure_factor(x, q, kv)
    E, W = eref.energy_virial(S, x, q, kv, kt["ug"], T["g"], T["V"], T["qs"], T["slab"], T["L"])
    f, e = eref.forces_eatom(S, x, q, kv, kt["ug"], T["g"], T["V"], T["qs"], targets, T["slab"], T["L"])
    return f, E, W, e, T["qs"] * eref.ksum(S, kt["ug"])


def rms(a):
    a = np.asarray(a)
    return float(np.sqrt((a * a).sum() / len(a)))
