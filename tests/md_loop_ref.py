"""The device-resident MD loop of INTEGRATION.md as one system, one driver and one composed reference.

System: bonded_ref.molecule_system() -- systems.small_random(ne_side=4, n_elyte=64) with 21 bent three-atom molecules, seven of them on
periodic faces and an edge -- with SHAKE clusters on nine molecules (flags 1 / 3 / 2 in turn, four of them face molecules), harmonic
bonds and angles on what SHAKE leaves free (shake_ref.step_case's rule: a constrained bond carries no spring), `special_bonds` over
every molecule, the electrolyte as the one integrator group, `fix efield` on the electrolyte.  The constraint lengths are the starting
geometry's own, rounded to 1e-3 A, so that conp_shake_correct_device has work to do and converges.

The start is separated_start(): molecule_system() places its outer atoms at random, its closest intermolecular pair lies 0.66 A apart,
and with pair_force_ref.lj_tables (sigma 2.5 - 3.5 A) the r^-12 force of that pair is 10^7 kcal/mol/A, which no time step integrates.
Every molecule is therefore moved as a rigid body until no two atoms of different molecules are closer than R_SEPARATE; bond lengths,
angles and the face molecules stay molecule_system()'s.  min_start() is the smallest listed distance of that start (0.762 A, a 1-3
distance inside a rigid molecule): the floor of the reference trajectory's condition.

Driver: run(...) issues the two documented call sequences on torch's current stream.  Composed reference: class Ref evaluates every
entry from the suite's own references (ghost_ref, neigh_ref, post_neighbor_ref, pair_force_ref, ewald_force_ref, bonded_ref, field_ref,
pppm_force_ref, shake_ref, integrate_ref, exclude_ref and the CPU oracle); reference_entry(...) applies it at the arrays a device entry read, reference_trajectory(...)
runs the whole loop with its own decisions, in float64 or -- where the suite has a longdouble reference -- in np.longdouble."""
import dataclasses
import functools
from types import SimpleNamespace

import numpy as np

import bonded_ref as br
import ewald_force_ref as efr
import field_ref as fr
import ghost_ref as gref
import integrate_ref as ir
import neigh_ref as nref
import pair_force_ref as pref
import pppm_force_ref as pfr
import post_neighbor_ref as pnr
import exclude_ref as xref
import shake_ref as sr
from conp_amd import neighbor, systems

LD = np.longdouble
R_SEPARATE = 2.0                     # A: no two atoms of different molecules start closer (separated_start)
ETA_OPEN = 0.45                      # eta^2 r^2 < 5.8 up to r = 5.35 A: the Gaussian gate of conp_fix_post_force_device is open
VARIANTS = {
    "A": dict(style="conp", newton=True, nvt=True, couple=0, eta=None),
    "B": dict(style="conq", newton=False, nvt=False, couple=1, eta=None),
    "C": dict(style="conp", newton=True, nvt=False, couple=0, eta=ETA_OPEN),
    "D": dict(style="conp", newton=True, nvt=False, couple=0, eta=None, pppm=((27, 24, 144), 5)),
    "E": dict(style="conq", newton=False, nvt=False, couple=1, eta=None, mirror=True),
}
# variant E: `fix zmirror` sends molecules 16, 17 (harmonic, off the faces) onto molecules 18, 19, which leave the integrator group; the
# mirror plane is put where the images lie in the empty part of the box, well inside its upper z face; `neigh_modify exclude group recv
# all` takes the images out of the pair list, as the deck's rule takes out its mirrored half (tests/test_gpu_pair_exclude.zmirror_box)
ALL, SEND, RECV = 1, 2, 4
SEND_MOLS, RECV_MOLS = (16, 17), (18, 19)
MIRROR_CENTRE = 13.0
GATE_OPEN = ("C",)
SHAKE_MOLS = ((0, 1), (2, 3), (4, 2), (5, 1), (6, 1), (7, 3), (8, 2), (9, 3), (10, 1), (11, 2), (13, 1), (15, 1))     # (molecule, flag)
FACE_MOLS = tuple(range(7))          # molecule_system(): six on the faces of x, y, z, one on an edge
SPECIAL_COUL = (1.0, 0.0, 0.0, 0.5)
SPECIAL_LJ = (1.0, 0.0, 0.0, 0.5)
MAXSPECIAL = 4
DT = 2.0
T_TARGET = 1500.0
T_PERIOD = 4000.0                    # fs: SHAKE ignores the thermostat's scaling; a gentle chain keeps the deviation below a tenth of the tolerance
V_SCALE = 1.0
SEED = 5
STEPS = 24
CONQ_CHARGE = 0.05
BONDED = SimpleNamespace(bond_k=br.PARAMS.bond_k.copy(), bond_r0=np.array([1.25, 1.3, 1.35]), angle_k=br.PARAMS.angle_k.copy(),
                         angle_theta0=br.PARAMS.angle_theta0.copy())
SHAKE_TOLERANCE, SHAKE_MAX_ITER = sr.TOLERANCE, 20


# ---- the system -----------------------------------------------------------------------------------------------------------------------
FACE_DIMS = {0: (0,), 1: (0,), 2: (1,), 3: (1,), 4: (2,), 5: (2,), 6: (0, 1)}    # molecule_system(): the faces its first 7 molecules lie on


@functools.lru_cache(maxsize=None)
def separated_start():
    """molecule_system() with its overlaps taken out: every molecule is moved as a rigid body (the face molecules along their faces
    only, electrode atoms not at all) until no two atoms of different molecules are closer than R_SEPARATE.  Bond lengths, angles and
    which molecule straddles which face stay molecule_system()'s.  -> (system, bonds, angles)"""
    from scipy.spatial import cKDTree
    s, bonds, angles = br.molecule_system()
    n = s.natoms
    el = np.nonzero(s.echeck == 0)[0]
    body = np.full(n, -1)
    body[el[:63]] = np.repeat(np.arange(21), 3)
    body[el[63]] = 21
    boxlo, boxhi, periodic, _ = gref.box_of(s)
    free = np.ones((22, 3))
    for m, dims in FACE_DIMS.items():
        free[m, list(dims)] = 0.0
    x = s.x.copy()
    for _ in range(400):
        g = gref.build(x, boxlo, boxhi, periodic, R_SEPARATE + 0.5)
        owner = np.concatenate([np.arange(n), g.owner])
        p = cKDTree(g.x).query_pairs(R_SEPARATE, output_type="ndarray")
        i, j = p[:, 0], p[:, 1]
        bi, bj = body[owner[i]], body[owner[j]]
        keep = ((i < n) | (j < n)) & (bi != bj)
        i, j, bi, bj = i[keep], j[keep], bi[keep], bj[keep]
        if not len(i):
            break
        d = g.x[i] - g.x[j]
        r = np.sqrt((d * d).sum(axis=1))
        push = d / r[:, None] * ((R_SEPARATE - r) * np.where((bi < 0) | (bj < 0), 1.0, 0.5) + 0.01)[:, None]
        move = np.zeros((22, 3))
        for b, sign, own in ((bi, 1.0, i < n), (bj, -1.0, j < n)):
            ok = (b >= 0) & own
            np.add.at(move, b[ok], sign * push[ok])
        move *= free
        norm = np.linalg.norm(move, axis=1)
        move *= np.minimum(1.0, 0.25 / np.maximum(norm, 1e-300))[:, None]
        x[body >= 0] += move[body[body >= 0]]
        x, _ = gref.wrap(x, boxlo, boxhi, periodic)
    else:
        raise AssertionError("the molecules could not be separated")
    return dataclasses.replace(s, x=np.ascontiguousarray(x)), bonds, angles


@functools.lru_cache(maxsize=None)
def system(variant):
    V = VARIANTS[variant]
    s0, bonds_all, angles_all = separated_start()
    s = dataclasses.replace(s0, newton=V["newton"], eletypes=None, eta=s0.eta if V["eta"] is None else V["eta"])
    n = s.natoms
    el = np.nonzero(s.echeck == 0)[0]
    mol = el[:63].reshape(21, 3)                               # (outer, centre, outer)
    prd = np.where(s.periodic, s.prd, 0.0)
    flag_of = dict(SHAKE_MOLS)
    group = np.where(s.echeck == 0, 0, -1).astype(np.int32)
    mirror = None
    if V.get("mirror"):
        mask = np.full(n, ALL, np.int32)
        mask[mol[list(SEND_MOLS)].ravel()] |= SEND
        mask[mol[list(RECV_MOLS)].ravel()] |= RECV
        src, dst = xref.mirror_map(s.tag, mask, SEND, RECV)
        zs = s.x[src, 2]
        zoffset = float(np.round(2.0 * (MIRROR_CENTRE + 0.5 * (zs.min() + zs.max()))) / 2.0)
        zprd = float(s.prd[2])
        molecule = np.zeros(n, np.int32)
        molecule[mol.ravel()] = np.repeat(np.arange(1, 22), 3)
        s = dataclasses.replace(s, x=np.ascontiguousarray(xref.mirror_apply(s.x, src, dst, zoffset)))
        assert s.x[dst, 2].min() > s.boxlo[2] + 1.0 and s.x[dst, 2].max() < s.boxhi[2] - 1.0
        group[dst] = -1
        mirror = SimpleNamespace(src=src, dst=dst, mask=mask, molecule=molecule, zoffset=zoffset, boxlo_z=0.5 * (zoffset - zprd), zprd=zprd,
                                 rule=xref.rules(group_pairs=[(RECV, ALL)]))
        assert 2.0 * mirror.boxlo_z + mirror.zprd == zoffset
    # harmonic terms on what SHAKE leaves free
    bonds, angles = [], []
    for m in range(21):
        fl = flag_of.get(m, 0)
        if fl == 0:
            bonds += [bonds_all[2 * m], bonds_all[2 * m + 1]]
        if fl == 2:
            bonds += [bonds_all[2 * m + 1]]
        if fl != 1:
            angles += [angles_all[m]]
    bonds, angles = np.array(bonds, dtype=np.int32), np.array(angles, dtype=np.int32)
    # the clusters: i0 the centre; one bond type (and angle type) per constraint, its length the starting one

    def dist(i, j):
        d = s.x[i] - s.x[j]
        d -= np.where(prd > 0, prd * np.round(d / np.where(prd > 0, prd, 1.0)), 0.0)
        return float(np.round(np.sqrt(d @ d), 3))
    cluster, bond_d, angle_d = [], [], []
    for m, fl in SHAKE_MOLS:
        a0, c0, a2 = (int(v) for v in mol[m])
        row = [fl, c0, a0, -7, 99, 99, 99]
        bond_d.append(dist(c0, a0)); row[4] = len(bond_d)
        if fl != 2:
            row[3] = a2
            bond_d.append(dist(c0, a2)); row[5] = len(bond_d)
        if fl == 1:
            angle_d.append(dist(a0, a2)); row[6] = len(angle_d)
        cluster.append(row)
    cluster = np.array(cluster, dtype=np.int32)
    nconstraint = int(np.where(cluster[:, 0] == 2, 1, np.where(cluster[:, 0] == 3, 2, 3)).sum())
    member = np.zeros(n, dtype=bool)
    for row in cluster:
        member[row[1:3]] = True
        if row[0] != 2:
            member[row[3]] = True
    shake = SimpleNamespace(tag="md loop", nlocal=n, ncluster=len(cluster), type=s.type.astype(np.int32), mass=ir.MASS.copy(),
                            bond_d=np.array(bond_d), angle_d=np.array(angle_d), cluster=cluster, tolerance=SHAKE_TOLERANCE,
                            max_iter=SHAKE_MAX_ITER, dt=DT, ftm2v=ir.FTM2V, prd=prd.copy(), member=member)
    integ = SimpleNamespace(type=s.type.astype(np.int32), group=group, mass=ir.MASS.copy(), style=np.array([1 if V["nvt"] else 0], dtype=np.int32),
                            dof=np.array([3.0 * int((group == 0).sum()) - 3.0 - nconstraint]), t_period=np.array([T_PERIOD]), dt=DT, ftm2v=ir.FTM2V,
                            mvv2e=ir.MVV2E, boltz=ir.BOLTZ, t_target=np.array([T_TARGET]))
    rng = np.random.default_rng(SEED)
    v0 = rng.normal(size=(n, 3)) * np.sqrt(ir.BOLTZ * T_TARGET / (ir.MASS[s.type - 1] * ir.MVV2E))[:, None] * V_SCALE
    v0[group < 0] = 0.0
    # special_bonds: 1-2 and 1-3 partners of every molecule, by tag
    nspecial = np.zeros((n, 3), dtype=np.int32)
    special = np.zeros((n, MAXSPECIAL), dtype=np.int32)
    for a0, c0, a2 in mol:
        for i, one_two, one_three in ((a0, [c0], [a2]), (c0, [a0, a2], []), (a2, [c0], [a0])):
            row = [s.tag[j] for j in one_two + one_three]
            nspecial[i] = (len(one_two), len(row), len(row))
            special[i, :len(row)] = row
    boxlo, boxhi, periodic, cut = gref.box_of(s)
    lz = float(s.prd[2])
    potdiff = CONQ_CHARGE if V["style"] == "conq" else float(s.potdiff)
    e = (0.0, 0.0, 0.0) if V["couple"] else (0.0, 0.0, -potdiff / lz)
    return SimpleNamespace(variant=variant, V=V, s=s, n=n, mol=mol, bonds=bonds, angles=angles, bonded=BONDED, shake=shake, integ=integ,
                           v0=np.ascontiguousarray(v0), nspecial=nspecial, special=special, specials=(nspecial, special),
                           p=pref.lj_tables(s.ntypes, s.cutoff), box=(boxlo, boxhi, periodic, cut), cutneigh=cut,
                           prd=prd, prd_half=np.where(np.asarray(periodic), 0.5 * np.asarray(s.prd), 0.0), trigger=0.5 * float(s.skin),
                           sel=(s.echeck == 0).astype(np.int32), potdiff=potdiff, e=e, couple=V["couple"], couple_scale=-1.0 / lz,
                           a2e=pnr.rows_of_owned(s.echeck), ne=int((s.echeck != 0).sum()), newton=bool(V["newton"]), mirror=mirror)


@functools.lru_cache(maxsize=None)
def min_start():
    """the smallest listed distance of the starting system"""
    c = system("B")
    nb = neighbouring(c, c.s.x)
    i, j = pref.pairs_of(nb.lst)
    d = nb.x[i] - nb.x[j & pref.NEIGHMASK]
    return float(np.sqrt((d * d).sum(axis=1)).min())


# ---- a neighbouring in numpy ------------------------------------------------------------------------------------------------------------
def neighbouring(c, x_owned_wrapped):
    """ghost map, filled coordinates and the half list (rows sorted, special bits) of owned coordinates that lie inside the box"""
    boxlo, boxhi, periodic, cut = c.box
    g = gref.build(x_owned_wrapped, boxlo, boxhi, periodic, cut)
    full = np.concatenate([np.arange(c.n), g.owner]).astype(np.int64)
    s = c.s
    at = neighbor.Atoms(nlocal=c.n, nghost=g.nghost, x=g.x, q=s.q[full].copy(), type=s.type[full].copy(), tag=s.tag[full].copy(),
                        echeck=s.echeck[full].copy(), owner=full.astype(np.int32))
    inp = SimpleNamespace(at=at, cutneigh=c.cutneigh, newton=c.newton, prd_half=c.prd_half)
    lst, _ = nref.reference(inp, c.specials, SPECIAL_LJ, SPECIAL_COUL)
    npairs_plain = lst.neigh.size
    if c.mirror is not None:
        m = c.mirror
        lst = xref.filter_list(lst, m.rule, s.type[full], m.mask[full], m.molecule[full])
    return SimpleNamespace(owner=g.owner, img=g.img, nghost=g.nghost, nall=c.n + g.nghost, ghost_margin=g.margin, x=g.x, lst=lst, full=full,
                           xhold=np.array(x_owned_wrapped, copy=True), inp=inp, gprd=g.prd,
                           npairs_plain=npairs_plain)


def fill(c, nb, x_owned, q_owned=None):
    x = gref.fill(x_owned, nb.owner, nb.img, nb.gprd)
    return x if q_owned is None else (x, np.concatenate([q_owned, q_owned[nb.owner]]))


def mirrored(c, x):
    """conp_zmirror_post_integrate_device on x (any float type): x[dst] = (x[src][0], x[src][1], zoffset - x[src][2])"""
    m = c.mirror
    out = np.array(x, copy=True)
    s = out[m.src].copy()
    out[m.dst, 0], out[m.dst, 1] = s[:, 0], s[:, 1]
    out[m.dst, 2] = out.dtype.type(m.zoffset) - s[:, 2]
    return out


def moved(c, nb, x_owned):
    """Neighbor::check_distance -> (flag, largest displacement since the build)"""
    d = np.asarray(x_owned, np.float64)[:c.n] - nb.xhold
    rsq = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    return int(rsq.max() > c.trigger * c.trigger), float(np.sqrt(rsq.max()))


def atoms_of(c, nb, x_all, q_all):
    s = c.s
    return neighbor.Atoms(nlocal=c.n, nghost=nb.nghost, x=np.ascontiguousarray(x_all, dtype=np.float64), q=np.ascontiguousarray(q_all, dtype=np.float64),
                          type=s.type[nb.full].copy(), tag=s.tag[nb.full].copy(), echeck=s.echeck[nb.full].copy(), owner=nb.full.astype(np.int32))


def straddlers(c, x_owned):
    """the molecules whose members lie on both sides of a periodic face"""
    out = []
    for m, (a0, c0, a2) in enumerate(c.mol):
        for j in (a0, a2):
            if np.any((c.prd > 0) & (np.abs(x_owned[c0] - x_owned[j]) > 0.5 * np.where(c.prd > 0, c.prd, np.inf))):
                out.append(m)
                break
    return out


# ---- the entries' references ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_lib():
    import oracle_py
    return oracle_py.load()


@functools.lru_cache(maxsize=None)
def ktables(variant):
    """(kv, ug, g, V, qs) from the oracle's KSpace of the starting system"""
    import oracle_py
    s = system(variant).s
    ks = oracle_py.KSpace.from_system(_oracle_lib(), s)
    kv = np.stack([ks.kxvecs, ks.kyvecs, ks.kzvecs], 1) * ks.unitk
    out = dict(kv=kv, ug=ks.ug.copy(), g=float(s.g_ewald), V=float(s.prd[0] * s.prd[1] * s.prd[2] * s.slab_volfactor), qs=systems.QQRD2E)
    ks.close()
    return out


@functools.lru_cache(maxsize=None)
def pppm_tables(variant):
    """(the oracle's Pppm of the variant's mesh, the tables of tests/pppm_force_ref.py)"""
    import oracle_py
    s = system(variant).s
    mesh, order = VARIANTS[variant]["pppm"]
    pp = oracle_py.Pppm(_oracle_lib(), s, mesh, order, fast=True)
    return pp, pfr.tables(_oracle_lib(), pp, s, mesh, order)


class Ref:
    """every entry of the loop from the suite's references, in float64 (kind "f64") or longdouble where the suite has one ("ld")"""

    def __init__(self, variant, kind="f64"):
        self.c = system(variant)
        self.kind = kind
        self.T = LD if kind == "ld" else np.float64

    # the charge update and the Gaussian correction: the CPU oracle on the neighbouring's list
    def oracle(self, nb, x_all, q_all):
        """-> (q [nall] with the electrode charges written, the fix scalar, the open oracle run)"""
        from helpers import OracleRun
        c = self.c
        at = atoms_of(c, nb, x_all, q_all)
        o = OracleRun(_oracle_lib(), c.s, at, nb.lst, nb.lst)
        o.setup()
        if c.V["style"] == "conq":
            scalar = float(o.fx.pre_force_conq(c.potdiff))
        else:
            o.pre_force(c.potdiff)
            scalar = float(o.fx.scalars()["scalar_output"])
        if c.V.get("pppm"):
            scalar = self._mesh_charges(o, at)
        return o.q.copy(), scalar, o

    def _mesh_charges(self, o, at):
        """the update of a `pppm` handle from the oracle's pieces: its projected inverse and its b (pppm_conp.cpp keeps the Ewald
        matrix), with the k-space part of b taken from oracle_py.Pppm.b_cal in place of the exact sum's; the update is linear in b
        (orc_fix_update_charge): q = S b + potdiff setq.  Writes o.q -> the fix scalar"""
        import oracle_py
        c, n = self.c, self.c.n
        m = o.fx.maps()
        loc = {int(t): i for i, t in enumerate(at.tag[:n])}
        xele = np.ascontiguousarray(at.x[[loc[int(t)] for t in m["eleall2tag"]]])
        ks = oracle_py.KSpace.from_system(_oracle_lib(), c.s)
        sr_, si_ = ks.sincos_b(at.x, o.q, at.echeck, n)
        csk, snk = ks.ele_trig(xele)
        b_exact = ks.bbb(csk, snk, sr_, si_)
        ks.close()
        pp, _ = pppm_tables(c.variant)
        b_mesh = pp.b_cal(at.x, o.q, at.echeck, n, xele)
        b_all, _, setq = o.fx.vectors()
        eleallq = o.fx.matrix() @ (b_all - b_exact + b_mesh)
        ele = np.nonzero(at.echeck != 0)[0]
        row = m["tag2eleall"][at.tag[ele]]
        o.q[ele] = eleallq[row] + c.potdiff * setq[row]
        return float(c.potdiff * o.fx.scalars()["totsetq"] + eleallq[m["elecheck_eleall"] == 1].sum())

    def gaussian(self, o, q_all):
        """the oracle's post_force at the charges given -> (f [nall][3], out [8])"""
        o.q[:] = q_all
        return o.fx.post_force()

    def gate(self, nb, x_all):
        """the listed pairs inside the Gaussian gate (test_gpu_post_force_device.contributing's rule)"""
        c = self.c
        i, j = pref.pairs_of(nb.lst)
        j = j & pref.NEIGHMASK
        ech = c.s.echeck[nb.full]
        one = (ech[i] != 0) != (ech[j] != 0)
        i, j = i[one], j[one]
        d = x_all[i] - x_all[j]
        rsq = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        keep = (rsq < c.s.cutoff * c.s.cutoff) & (c.s.eta * c.s.eta * rsq < 5.8)
        return int(keep.sum())

    def ewald(self, x_all, q_all):
        c, k = self.c, ktables(self.c.variant)
        x, q = np.ascontiguousarray(x_all[:c.n], np.float64), np.ascontiguousarray(q_all[:c.n], np.float64)
        if c.V.get("pppm"):                                              # the mesh reference of tests/pppm_force_ref.py
            _, T = pppm_tables(c.variant)
            return pfr.forces_eatom(pfr.solve(pfr.spread(x, q, T), T), x, q, T, np.arange(c.n))[0]
        S = efr.structure_factor(x, q, k["kv"])
        return efr.forces_eatom(S, x, q, k["kv"], k["ug"], k["g"], k["V"], k["qs"], np.arange(c.n))[0]

    def pair(self, nb, x_all, q_all):
        c = self.c
        return pref.reference(x_all, q_all, c.s.type[nb.full], c.n, nb.lst, c.p, c.s.g_ewald, systems.QQRD2E, c.newton, SPECIAL_LJ, SPECIAL_COUL)

    def bonded_terms(self, x_all):
        c = self.c
        return br.reference(np.asarray(x_all[:c.n], np.float64), c.n, c.bonds, c.angles, c.bonded, True, c.prd)

    def field(self, kind, x_all, q_all, image, f_before, scalar):
        c = self.c
        case = SimpleNamespace(nlocal=c.n, sel=c.sel, x=np.asarray(x_all[:c.n], np.float64), image=image, qe2f=systems.QE2F,
                               q=np.asarray(q_all[:c.n], np.float64), prd=tuple(float(p) for p in c.prd), f=np.asarray(f_before[:c.n], np.float64))
        return fr.efield(kind, case, c.e, couple=c.couple, couple_scale=c.couple_scale, s=scalar)

    def force_terms(self, nb, x_all, q_all, image, scalar, o):
        """the step's terms at x, q -> dict name -> [nall][3] in the kind's type, unfolded; `o`: the oracle run of this x"""
        c, T = self.c, self.T
        z = lambda: np.zeros((nb.nall, 3), dtype=T)
        t = {}
        t["ewald"] = z(); t["ewald"][:c.n] = self.ewald(x_all, q_all)
        t["pair"] = self.pair(nb, x_all, q_all).f.astype(T)
        t["bonded"] = z(); t["bonded"][:c.n] = self.bonded_terms(x_all).f.astype(T)
        t["gaussian"] = self.gaussian(o, np.asarray(q_all, np.float64))[0].astype(T)
        add = self.field("ld", x_all, q_all, image, np.zeros((c.n, 3)), scalar).add.v
        t["field"] = z(); t["field"][:c.n] = add.astype(T)
        return t

    def folded(self, nb, terms, without=None):
        c = self.c
        tot = sum(v for k, v in terms.items() if k != without)
        out = np.array(tot[:c.n], copy=True)
        if c.newton:
            np.add.at(out, nb.owner, tot[c.n:])
        return out


def shake_rule(c, kind):
    with sr.first_order_integrator():
        return sr.Rule(kind, c.shake)


def integ_rule(c, kind):
    with sr.first_order_integrator():
        return ir.Rule(kind, c.integ)


def _val(a):
    return a.v if isinstance(a, ir.Mag) else a


# ---- the reference trajectory -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference_trajectory(variant, steps=STEPS, kind="f64"):
    """the loop on the CPU with its own decisions -> SimpleNamespace(x, v, q, f, image, flags, nghost, builds, and what
    tests/test_md_loop_ref_math.py asserts of it: per step the displacement, per build the margins and the straddling molecules,
    the SHAKE counters, the smallest listed distance, the gate counts)"""
    c = system(variant)
    R = Ref(variant, kind)
    T = R.T
    n = c.n
    boxlo, boxhi, periodic, _ = c.box
    S, I = shake_rule(c, kind), integ_rule(c, kind)
    ld = kind == "ld"
    cast = (lambda a: np.asarray(_val(a), dtype=LD)) if ld else (lambda a: np.asarray(_val(a), dtype=np.float64))
    rec = SimpleNamespace(flags=[], nghost=[], builds=[], disp=[], shake=[], rmin=[], gate=[], near=np.inf, scalar=[], fmax=[], check=[], t_current=[])
    image = np.zeros((n, 3), np.int32)

    def reneighbour(x, step):
        nonlocal image
        x64 = np.asarray(x, np.float64)
        xw, image_new = gref.wrap(x64, boxlo, boxhi, periodic, image)
        changed = np.nonzero(np.any(image_new != image, axis=1))[0]
        if ld:                                       # the wrap's shift applied to the longdouble coordinates
            x = x + (xw - x64).astype(LD)
        else:
            x = xw
        image = image_new
        nb = neighbouring(c, xw)
        st = straddlers(c, xw)
        rec.builds.append(SimpleNamespace(step=step, nghost=nb.nghost, ghost_margin=nb.ghost_margin, cutoff_margin=nref.cutoff_margin(nb.inp),
                                          changed=changed, image=image.copy(), straddlers=st))
        return x, nb

    def forces(x, q_own, nb):
        x64 = np.asarray(x, np.float64)
        x_all, q_all = fill(c, nb, x64, q_own)
        q_new, scalar, o = R.oracle(nb, x_all, q_all)
        xa = fill(c, nb, x) if ld else x_all         # longdouble coordinates for the longdouble entries
        terms = R.force_terms(nb, xa, q_new.astype(T), image, scalar, o)
        o.fx.close()
        i, j = pref.pairs_of(nb.lst)
        d = x_all[i] - x_all[j & pref.NEIGHMASK]
        rec.rmin.append(float(np.sqrt((d * d).sum(axis=1)).min()))
        rec.gate.append(R.gate(nb, x_all))
        rec.scalar.append(scalar)
        total = R.folded(nb, terms)
        rec.fmax.append(float(np.abs(total).max()))
        return total, q_new[:n]

    def note_shake(res):
        rec.shake.append((res.unconverged, res.bad_determ, res.niter_max))

    x = cast(S.solve(c.s.x.astype(T), None, None, correct=True).out)
    x, nb = reneighbour(x, -1)
    q = c.s.q.copy()
    f, q = forces(x, q, nb)
    v = c.v0.astype(T)
    res = S.solve(x, v, f, half=True)
    note_shake(res)
    f = cast(res.out)
    with sr.first_order_integrator():
        I.setup(v, c.integ.t_target)
    for step in range(steps):
        with sr.first_order_integrator():
            x, v = (cast(a) for a in I.initial(x, v, f, c.integ.t_target))
        if c.mirror is not None:
            x = mirrored(c, x)
        rec.check.append(tuple(float(d) for d in S.check(x)))
        flag, disp = moved(c, nb, x)
        rec.flags.append(flag); rec.disp.append(disp)
        if flag:
            x, nb = reneighbour(x, step)
        rec.nghost.append(nb.nghost)
        f, q = forces(x, q, nb)
        res = S.solve(x, v, f)
        note_shake(res)
        f = cast(res.out)
        with sr.first_order_integrator():
            v, rows = I.final(v, f)
            v = cast(v)
        rec.t_current.append(float(_val(rows[0][0])))
    rec.near = sr.clear_of_the_tolerance(S, c.shake.tolerance)
    rec.x, rec.v, rec.q, rec.f, rec.image = x, v, q, f, image
    rec.state = I.get_state()[0]
    return rec


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------
def new_handle(variant, x_owned=None, q_owned=None, before_setup=None):
    """a handle after the once-per-run calls: the host setup at the owned coordinates given (the start's by default; wrapped here),
    pair tables, bonded and SHAKE lists, integrator and field parameters"""
    from conp_amd import FixConp
    c = system(variant)
    s = c.s
    boxlo, boxhi, periodic, _ = c.box
    xw, _ = gref.wrap(s.x if x_owned is None else x_owned, boxlo, boxhi, periodic)
    nb = neighbouring(c, xw)
    q = s.q if q_owned is None else np.asarray(q_owned, np.float64)
    at0 = atoms_of(c, nb, nb.x, np.concatenate([q, q[nb.owner]]))
    mesh = dict(extra_args=["pppm"], pppm_mesh=c.V["pppm"][0], pppm_order=c.V["pppm"][1]) if c.V.get("pppm") else {}
    fx = FixConp(s, style=c.V["style"], **mesh)
    fx.pair_set_params(c.p.cutsq, c.p.cut_coul, c.p.lj, SPECIAL_LJ, SPECIAL_COUL)
    if before_setup is not None:
        before_setup(fx)                                                 # (what a test issues on the handle before its first update)
    fx.init_lists(nb.lst, nb.lst)
    fx.setup_post_neighbor(at0)
    fx.setup_pre_force(at0, 0, c.potdiff)
    sh, g = c.shake, c.integ
    fx.shake_set_params(sh.type, sh.mass, sh.bond_d, sh.angle_d, sh.cluster, sh.tolerance, sh.max_iter, sh.dt, sh.ftm2v, sh.prd)
    fx.integrate_set_params(g.type, g.group, g.mass, g.style, g.dof, g.t_period, g.dt, g.ftm2v, g.mvv2e, g.boltz)
    fx.bonded_set_params(c.bonded.bond_k, c.bonded.bond_r0, c.bonded.angle_k, c.bonded.angle_theta0, newton_bond=True)
    fx.bonded_set_lists(c.n, c.n, c.bonds, c.angles, c.prd)
    fx.efield_set_params(c.sel, systems.QE2F, c.prd)
    if c.mirror is not None:
        m = c.mirror
        fx.pair_set_exclusions(group_pairs=m.rule.group_pairs)
        fx.zmirror_set_params(s.tag, m.mask, SEND, RECV, 1, m.boxlo_z, m.zprd)
    return fx


class Loop:
    """the two call sequences of INTEGRATION.md on torch's current stream.  checked=False: nothing synchronises but what the
    re-neighbouring entries do themselves and the one read of the moved flag per step; checked=True: after every entry the arrays are
    downloaded into self.rec (a list of (step, entry, arrays))"""

    def __init__(self, fx, variant, steps, checked):
        import torch
        self.torch, self.fx, self.c, self.checked, self.steps = torch, fx, system(variant), checked, steps
        c = self.c
        fx.set_stream(torch.cuda.current_stream().cuda_stream)           # torch's zero_() and copies are ordered with the entries
        nan = float("nan")
        dev = lambda shape, fill, dt=torch.float64: torch.full(shape, fill, dtype=dt, device="cuda")
        rows = steps + 2                                                 # row 0: the start, row k + 1: step k, the last: spare
        self.o_gauss, self.o_shake, self.o_field = dev((rows, 9), nan), dev((rows, 9), nan), dev((rows, fr.EFIELD_W), nan)
        self.o_integ, self.o_check, self.o_pair = dev((rows, 4), nan), dev((rows, 2), nan), dev((rows, 8), nan)
        self.d_flag = dev((1,), -1, torch.int32)
        self.d_nspecial = torch.from_numpy(c.nspecial.copy()).cuda()
        self.d_special = torch.from_numpy(c.special.copy()).cuda()
        self.flags, self.nghost, self.rec, self.builds = [], [], [], []
        self.nall = 0
        self.step_no = -1

    # -- arrays ------------------------------------------------------------------------------------------------------------------------
    def upload(self, x, v, q, image):
        torch, n = self.torch, self.c.n
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
        self.d_x, self.d_v, self.d_q = t(x[:n], np.float64), t(v[:n], np.float64), t(q[:n], np.float64)
        self.d_image = t(image, np.int32)
        self.d_f = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
        self.d_tag = t(self.c.s.tag, np.int32)
        m = self.c.mirror
        self.d_cls = [] if m is None else [t(self.c.s.type, np.int32), t(m.mask, np.int32), t(m.molecule, np.int32)]
        self.nall = n

    def resize(self, nall):
        """arrays for the new nlocal + nghost, the owned rows copied over; ghost rows start as NaN (tag: -1)"""
        torch, n = self.torch, self.c.n
        nan = float("nan")
        new = lambda old, shape, fill: torch.full(shape, fill, dtype=old.dtype, device="cuda")
        x, q, f, tag = new(self.d_x, (nall, 3), nan), new(self.d_q, (nall,), nan), new(self.d_f, (nall, 3), 0.0), new(self.d_tag, (nall,), -1)
        x[:n], q[:n], f[:n], tag[:n] = self.d_x[:n], self.d_q[:n], self.d_f[:n], self.d_tag[:n]
        cls = [new(a, (nall,), -1) for a in self.d_cls]
        for a, b in zip(cls, self.d_cls):
            a[:n] = b[:n]
        self.d_x, self.d_q, self.d_f, self.d_tag, self.d_cls, self.nall = x, q, f, tag, cls, nall

    def snap(self, entry, **extra):
        if not self.checked:
            return
        self.torch.cuda.synchronize()
        h = lambda t: t.cpu().numpy().copy()
        a = dict(x=h(self.d_x), v=h(self.d_v), q=h(self.d_q), f=h(self.d_f), image=h(self.d_image), nall=self.nall)
        a.update(extra)
        self.rec.append((self.step_no, entry, a))

    # -- the re-neighbouring sequence ------------------------------------------------------------------------------------------------
    def build_list(self):
        fx, c = self.fx, self.c
        special = dict(d_tag=self.d_tag.data_ptr(), d_nspecial=self.d_nspecial.data_ptr(), d_special=self.d_special.data_ptr(),
                       maxspecial=MAXSPECIAL, prd_half=c.prd_half)
        if c.mirror is None:
            fx.pair_build_list_device(self.d_x.data_ptr(), c.n, self.nall, c.cutneigh, **special)
        else:
            ty, mk, ml_ = (a.data_ptr() for a in self.d_cls)
            fx.pair_build_list_exclude_device(self.d_x.data_ptr(), c.n, self.nall, c.cutneigh, d_type=ty, d_mask=mk, d_molecule=ml_, **special)

    def reneighbour(self, post_neighbor=True):
        """post_neighbor=False: the sequence without its last call (the lifetime rule of DESIGN.md section 19)"""
        fx, c = self.fx, self.c
        boxlo, boxhi, periodic, cut = c.box
        fx.atoms_wrap_device(self.d_x.data_ptr(), c.n, boxlo, boxhi, periodic, self.d_image.data_ptr())
        self.snap("wrap")
        ng = fx.ghost_build_device(self.d_x.data_ptr(), c.n, boxlo, boxhi, periodic, cut)
        self.resize(c.n + ng)
        fx.ghost_fill_device(self.d_x.data_ptr(), self.d_q.data_ptr())
        fx.ghost_fill_int_device(self.d_tag.data_ptr(), 1)
        for a in self.d_cls:
            fx.ghost_fill_int_device(a.data_ptr(), 1)
        self.snap("fill", tag=None if not self.checked else self.d_tag.cpu().numpy(),
                  cls=None if not self.checked else [a.cpu().numpy() for a in self.d_cls])
        self.build_list()
        if post_neighbor:
            fx.post_neighbor_device(self.d_x.data_ptr(), self.d_q.data_ptr())
        if not post_neighbor:
            return
        self.builds.append(self.step_no)
        if self.checked:
            lst, nall = fx.pair_get_list()
            _, ngh, owner, img = fx.ghost_get()
            self.snap("neighbour", lst=lst, list_nall=nall, owner=owner.copy(), img=img.copy(), nghost=ngh, tables=fx.step_tables())

    # -- the force phase of a step ---------------------------------------------------------------------------------------------------
    def force_phase(self, row):
        fx, c = self.fx, self.c
        X, Q = self.d_x.data_ptr(), self.d_q.data_ptr()
        self.d_f.zero_()
        F = self.d_f.data_ptr()
        fx.pre_force_device(X, Q, c.potdiff)
        self.snap("update", scalar=fx.compute_scalar() if self.checked else None)
        (fx.pppm_forces_device if c.V.get("pppm") else fx.ewald_forces_device)(X, Q, F, 0, 0)
        self.snap("kspace")
        fx.pair_compute_device(X, Q, F, self.o_pair[row].data_ptr(), 0, 0)
        self.snap("pair")
        fx.bonded_compute_device(X, F, 0, 0, 0)
        self.snap("bonded")
        fx.post_force_device(X, Q, F, self.o_gauss[row].data_ptr())
        self.snap("gaussian")
        fx.efield_post_force_device(X, Q, F, c.e, d_image=self.d_image.data_ptr(), couple=c.couple, couple_scale=c.couple_scale,
                                    d_out=self.o_field[row].data_ptr())
        self.snap("field")
        if c.newton:
            fx.ghost_fold_device(F, 3)
        self.snap("fold")

    # -- the run ------------------------------------------------------------------------------------------------------------------------
    def start(self):
        """conp_shake_correct_device -> the re-neighbouring sequence -> the force entries -> conp_shake_setup_device ->
        conp_integrate_setup_device, from the system's starting arrays"""
        c = self.c
        self.upload(c.s.x, c.v0, c.s.q, np.zeros((c.n, 3), np.int32))
        self.fx.shake_correct_device(self.d_x.data_ptr())
        self.snap("correct")
        self.resume(setup_chains=True)

    def resume(self, setup_chains=False):
        """what a run's start makes of arrays that are already on the device: a full re-neighbouring, the force entries and the SHAKE
        setup; the chains are set up only at a first start (a restart hands them over with conp_integrate_set_state)"""
        self.reneighbour()
        self.force_phase(0)
        self.fx.shake_setup_device(self.d_x.data_ptr(), self.d_v.data_ptr(), self.d_f.data_ptr(), self.o_shake[0].data_ptr())
        self.snap("shake")
        if setup_chains:
            self.fx.integrate_setup_device(self.d_v.data_ptr(), self.c.integ.t_target)

    def step(self, k):
        fx, c = self.fx, self.c
        self.step_no = k
        row = k + 1
        self.snap("begin", state=fx.integrate_get_state() if self.checked else None)
        fx.integrate_initial_device(self.d_x.data_ptr(), self.d_v.data_ptr(), self.d_f.data_ptr(), c.integ.t_target)
        self.snap("initial", state=fx.integrate_get_state() if self.checked else None)
        if c.mirror is not None:
            fx.zmirror_post_integrate_device(self.d_x.data_ptr(), k)
            self.snap("mirror")
        fx.shake_check_device(self.d_x.data_ptr(), self.o_check[row].data_ptr())
        fx.pair_list_moved_device(self.d_x.data_ptr(), c.trigger, self.d_flag.data_ptr())
        flag = int(self.d_flag.item())                                   # the one read per step
        self.flags.append(flag)
        if flag:
            self.reneighbour()
        else:
            fx.ghost_fill_device(self.d_x.data_ptr(), self.d_q.data_ptr())
            self.snap("fill")
        self.nghost.append(self.nall - c.n)
        self.force_phase(row)
        fx.shake_post_force_device(self.d_x.data_ptr(), self.d_v.data_ptr(), self.d_f.data_ptr(), self.o_shake[row].data_ptr(), 0)
        self.snap("shake")
        fx.integrate_final_device(self.d_v.data_ptr(), self.d_f.data_ptr(), self.o_integ[row].data_ptr())
        self.snap("final", state=fx.integrate_get_state() if self.checked else None)

    def result(self):
        """the final synchronisation -> the arrays and per-step outputs on the host"""
        self.torch.cuda.synchronize()
        h = lambda t: t.cpu().numpy().copy()
        n = self.c.n
        return SimpleNamespace(x=h(self.d_x)[:n], v=h(self.d_v), q=h(self.d_q)[:n], f=h(self.d_f)[:n], image=h(self.d_image),
                               state=self.fx.integrate_get_state().copy(), flags=list(self.flags), nghost=list(self.nghost),
                               builds=list(self.builds), gauss=h(self.o_gauss), shake=h(self.o_shake), field=h(self.o_field),
                               integ=h(self.o_integ), check=h(self.o_check), pair=h(self.o_pair), rec=self.rec)


def run(fx, variant, steps=STEPS, checked=False):
    """the loop from the system's start -> Loop.result()"""
    L = Loop(fx, variant, steps, checked)
    L.start()
    for k in range(steps):
        L.step(k)
    return L.result()


def same_bytes(a, b, names=("x", "v", "q", "f", "image", "state")):
    """the arrays of two results that differ, and whether the sequences of flags and ghost counts are equal"""
    bad = [k for k in names if getattr(a, k).tobytes() != getattr(b, k).tobytes()]
    if a.flags != b.flags:
        bad.append("flags")
    if a.nghost != b.nghost:
        bad.append("nghost")
    return bad


def first_difference(a, b):
    """per per-step output the first row (0: the start, k + 1: step k) whose bytes differ between two results, for a failure message"""
    out = {}
    for name in ("pair", "gauss", "field", "shake", "integ", "check"):
        u, v = getattr(a, name), getattr(b, name)
        rows = [r for r in range(min(len(u), len(v))) if u[r].tobytes() != v[r].tobytes()]
        out[name] = rows[0] if rows else None
    return out
