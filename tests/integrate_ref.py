"""numpy restatements of the integration rule of include/conp_hip.h (conp_integrate_*; LAMMPS FixNH, FixNVE, ComputeTemp @ 27May2021
at tchain 3, tloop 1, drag 0), and the inputs of the GPU tests.

The rule is written ONCE (class Rule) over a number type:
  - Rule("ld"): np.longdouble values that carry their cancellation-free magnitude (class Mag): every term replaced by its absolute
    value and every difference by the sum of its operands' magnitudes; a product's magnitude is the product of the magnitudes, a
    quotient's m_a m_b / b^2, and exp(u) has exp(u) (1 + m_u) -- what an error of m_u in u moves it by, beside its own rounding.
    The GPU tests bound |got - value| by TOL * magnitude, entry-wise; magnitudes accumulate over a sequence of steps because the
    state, v and x stay Mag from step to step.
  - Rule("f64"): plain float64 in the written order, sums over atoms in ascending i: bit for bit what the kernels do wherever no exp
    and no sum over atoms is involved (the nve path).
"""
from types import SimpleNamespace

import numpy as np

LD = np.longdouble
TOL = 1e-12
# launch shapes of conp_integrate.hip, restated (tests/test_integrate_ref_math.py compares them with csrc/conp_kernels.h)
BLOCK = 256       # threads of a workgroup: one atom each
FINISH = 256      # threads of the finishing workgroup: from BLOCK * FINISH + 1 atoms on a thread adds a second row of partial sums
MAX_GROUPS = 8
SENTINELS = 64    # rows behind nlocal in x, v, f of every case
# LAMMPS `units real`
FTM2V = 1.0 / 48.88821291 / 48.88821291
MVV2E = 48.88821291 * 48.88821291
BOLTZ = 0.0019872067
MASS = np.array([67.07, 15.04, 57.12, 144.96, 12.001])      # the IL decks' types; 5 is the electrode
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000, 4097)
BIG = BLOCK * FINISH + 1                                     # 257 rows of partial sums: one more than a round of the finish consumes


def tol_of(n):
    """1e-12, or n 2^-53 where that is larger: what a sum of n positive terms can lose in any order"""
    return max(TOL, n * 2.0 ** -53)


class Mag:
    """a longdouble value (scalar or array) with its cancellation-free magnitude"""
    __slots__ = ("v", "m")
    __array_ufunc__ = None          # numpy operands defer to the methods below

    def __init__(self, v, m=None):
        self.v = np.asarray(v, dtype=LD)
        self.m = np.abs(self.v) if m is None else np.asarray(m, dtype=LD)

    @staticmethod
    def of(x):
        return x if isinstance(x, Mag) else Mag(x)

    def __add__(self, o):
        o = Mag.of(o)
        return Mag(self.v + o.v, self.m + o.m)
    __radd__ = __add__

    def __sub__(self, o):
        o = Mag.of(o)
        return Mag(self.v - o.v, self.m + o.m)

    def __rsub__(self, o):
        return Mag.of(o) - self

    def __neg__(self):
        return Mag(-self.v, self.m)

    def __mul__(self, o):
        o = Mag.of(o)
        return Mag(self.v * o.v, self.m * o.m)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Mag.of(o)
        return Mag(self.v / o.v, self.m * o.m / (o.v * o.v))

    def __getitem__(self, k):
        return Mag(self.v[k], self.m[k])


def _exp(u):
    if isinstance(u, Mag):
        e = np.exp(u.v)
        return Mag(e, e * (1 + u.m))
    return np.exp(u)


def _where(mask, a, b):
    if isinstance(a, Mag) or isinstance(b, Mag):
        a, b = Mag.of(a), Mag.of(b)
        return Mag(np.where(mask, a.v, b.v), np.where(mask, a.m, b.m))
    return np.where(mask, a, b)


def _take(table, idx):
    """table[idx] for a list of per-group scalars (index -1: the last entry)"""
    if isinstance(table[0], Mag):
        return Mag(np.array([t.v for t in table], dtype=LD)[idx], np.array([t.m for t in table], dtype=LD)[idx])
    return np.array(table, dtype=np.float64)[idx]


class Rule:
    def __init__(self, kind, c):
        """c: a case (below).  The state is kept per group: eta[3], ed[4] (ed[3] = 0), edd[3], t_current, t_target"""
        self.ld = kind == "ld"
        self.num = (lambda x: Mag(x)) if self.ld else (lambda x: np.asarray(x, dtype=np.float64)[()])
        n = self.num
        self.c = c
        self.G = len(c.style)
        self.style = list(c.style)
        self.group = np.asarray(c.group)
        self.dtv = n(c.dt)
        self.dtf = n(0.5) * n(c.dt) * n(c.ftm2v)
        self.dthalf, self.dt4, self.dt8 = n(0.5) * n(c.dt), n(0.25) * n(c.dt), n(0.125) * n(c.dt)
        self.mvv2e, self.boltz = n(c.mvv2e), n(c.boltz)
        self.dof = [n(d) for d in c.dof]
        self.t_freq = [n(1.0) / n(t) if s else n(0.0) for t, s in zip(c.t_period, c.style)]
        mass_of = np.concatenate([[0.0], c.mass])[c.type]
        self.m_atom = n(mass_of)                                               # [nlocal]
        self.on = self.group >= 0
        z = n(0.0)
        self.S = [SimpleNamespace(eta=[z, z, z], ed=[z, z, z, z], edd=[z, z, z], t_current=z, t_target=z) for _ in range(self.G)]

    # ---- state ----------------------------------------------------------------------------------------------------------------
    def set_state(self, state8):
        """rows eta[3], eta_dot[3], t_current, t_target; eta_dotdot[k >= 1] as setup forms it; nve rows: eta, eta_dot = 0"""
        n = self.num
        for g, row in enumerate(np.asarray(state8, dtype=np.float64).reshape(self.G, 8)):
            s = self.S[g]
            nvt = self.style[g]
            s.eta = [n(row[k] if nvt else 0.0) for k in range(3)]
            s.ed = [n(row[3 + k] if nvt else 0.0) for k in range(3)] + [n(0.0)]
            s.edd = [n(0.0)] * 3
            s.t_current, s.t_target = n(row[6]), n(row[7])
            if nvt:
                self._eta_dotdot_setup(g)

    def get_state(self):
        """-> ([G][8] values, [G][8] magnitudes) (f64: the magnitudes are None)"""
        rows = [s.eta + s.ed[:3] + [s.t_current, s.t_target] for s in self.S]
        if self.ld:
            return (np.array([[q.v for q in r] for r in rows], dtype=LD), np.array([[q.m for q in r] for r in rows], dtype=LD))
        return np.array(rows, dtype=np.float64), None

    def _masses(self, g):
        s = self.S[g]
        kt = self.boltz * s.t_target
        tf2 = self.t_freq[g] * self.t_freq[g]
        return kt, [self.dof[g] * kt / tf2, kt / tf2, kt / tf2]

    def _eta_dotdot_setup(self, g):
        s = self.S[g]
        kt, em = self._masses(g)
        s.edd = list(s.edd)
        for k in (1, 2):
            s.edd[k] = (em[k - 1] * s.ed[k - 1] * s.ed[k - 1] - kt) / em[k]

    # ---- the pieces of the rule -------------------------------------------------------------------------------------------------
    def temp(self, v):
        """-> per group (t = sum m v^2, t_current)"""
        out = []
        for g in range(self.G):
            idx = np.nonzero(self.group == g)[0]
            w = v[idx]
            term = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2]) * self.m_atom[idx]
            if self.ld:
                t = Mag(term.v.sum(), term.m.sum())
            else:
                t = np.float64(np.cumsum(term)[-1]) if len(idx) else np.float64(0.0)          # ascending i, one at a time
            out.append((t, t * (self.mvv2e / (self.dof[g] * self.boltz))))
        return out

    def nve_v(self, v, f):
        dtfm = self.dtf / self.m_atom
        return _where(self.on[:, None], v + dtfm[:, None] * f, v)

    def nve_x(self, x, v):
        return _where(self.on[:, None], x + self.dtv * v, x)

    def chain_half_step(self, g):
        """steps 1-10 -> factor_eta"""
        s = self.S[g]
        dof, bz = self.dof[g], self.boltz
        kt, em = self._masses(g)
        ke_target = dof * kt
        eta, ed, edd = list(s.eta), list(s.ed), list(s.edd)
        edd[0] = (dof * bz * s.t_current - ke_target) / em[0]
        for k in (2, 1):
            e = _exp(-self.dt8 * ed[k + 1])
            ed[k] = ed[k] * e
            ed[k] = ed[k] + edd[k] * self.dt4
            ed[k] = ed[k] * e
        e = _exp(-self.dt8 * ed[1])
        ed[0] = ed[0] * e
        ed[0] = ed[0] + edd[0] * self.dt4
        ed[0] = ed[0] * e
        factor = _exp(-self.dthalf * ed[0])
        s.t_current = s.t_current * (factor * factor)
        edd[0] = (dof * bz * s.t_current - ke_target) / em[0]
        for k in range(3):
            eta[k] = eta[k] + self.dthalf * ed[k]
        ed[0] = ed[0] * e
        ed[0] = ed[0] + edd[0] * self.dt4
        ed[0] = ed[0] * e
        for k in (1, 2):
            e = _exp(-self.dt8 * ed[k + 1])
            ed[k] = ed[k] * e
            edd[k] = (em[k - 1] * ed[k - 1] * ed[k - 1] - kt) / em[k]
            ed[k] = ed[k] + edd[k] * self.dt4
            ed[k] = ed[k] * e
        s.eta, s.ed, s.edd = eta, ed, edd
        return factor

    def energy(self, g):
        s = self.S[g]
        kt, em = self._masses(g)
        ke_target = self.dof[g] * kt
        en = ke_target * s.eta[0] + self.num(0.5) * em[0] * s.ed[0] * s.ed[0]
        for k in (1, 2):
            en = en + (kt * s.eta[k] + self.num(0.5) * em[k] * s.ed[k] * s.ed[k])
        return en

    def _scale(self, v, factors):
        """v *= factor of the atom's group (nve groups and -1 atoms: untouched)"""
        one = self.num(1.0)
        table = [f if f is not None else one for f in factors] + [one]
        fa = _take(table, self.group)
        touched = np.array([f is not None for f in factors] + [False])[self.group]
        return _where(touched[:, None], v * fa[:, None], v)

    def _out(self, g, t, t_current, factor=None):
        ke = self.num(0.5) * self.mvv2e * t
        if factor is not None:
            ke = ke * (factor * factor)
        z = self.num(0.0)
        return [t_current, ke, self.energy(g) if self.style[g] else z, self.S[g].ed[0] if self.style[g] else z]

    # ---- the entries --------------------------------------------------------------------------------------------------------------
    def lift(self, a):
        """a float64 input array in the rule's number type"""
        return Mag(a) if self.ld and not isinstance(a, Mag) else a

    def temperature(self, v):
        return [self._out(g, t, tc) for g, (t, tc) in enumerate(self.temp(self.lift(v)))]

    def setup(self, v, t_target):
        for g, (t, tc) in enumerate(self.temp(self.lift(v))):
            self.S[g].t_current = tc
            if self.style[g]:
                self.S[g].t_target = self.num(t_target[g])
                self._eta_dotdot_setup(g)

    def initial(self, x, v, f, t_target):
        x, v, f = self.lift(x), self.lift(v), self.lift(f)
        factors = [None] * self.G
        for g in range(self.G):
            if self.style[g]:
                self.S[g].t_target = self.num(t_target[g])
                factors[g] = self.chain_half_step(g)
        v = self._scale(v, factors)
        v = self.nve_v(v, f)
        return self.nve_x(x, v), v

    def final(self, v, f):
        """-> (v, the d_out rows)"""
        v = self.nve_v(self.lift(v), self.lift(f))
        factors, out = [None] * self.G, []
        for g, (t, tc) in enumerate(self.temp(v)):
            self.S[g].t_current = tc
            if self.style[g]:
                factors[g] = self.chain_half_step(g)
            out.append(self._out(g, t, self.S[g].t_current, factors[g]))
        return self._scale(v, factors), out


def out_arrays(out):
    """the d_out rows of a Rule("ld") entry -> ([G][4] values, [G][4] magnitudes)"""
    return (np.array([[q.v for q in r] for r in out], dtype=LD), np.array([[q.m for q in r] for r in out], dtype=LD))


def frac(tag, got, want, bound):
    """largest |got - want| / bound over the entries (0 / 0 counts as 0: an entry of magnitude 0 must be exact)"""
    err = np.abs(np.asarray(got, dtype=LD) - want)
    bound = np.asarray(bound, dtype=LD) * np.ones_like(err)
    assert np.all(err[bound == 0] == 0), tag
    fr = float((err[bound > 0] / bound[bound > 0]).max()) if np.any(bound > 0) else 0.0
    print(f"{tag}: {fr:.3g} of the bound")
    return fr


# ---- input builders -----------------------------------------------------------------------------------------------------------------
def case(tag, nlocal, styles, seed=0, minus=0.1, one_atom=None, empty=None, confined=None, t_target=None, dt=2.0):
    """nlocal atoms with random group ids 0..len(styles)-1 interleaved, a fraction `minus` of them -1 (at least one where nlocal >= 8).
    one_atom: a group with exactly one atom; empty: a group without atoms; confined: a group whose atoms all lie in rows
    BLOCK .. 2 BLOCK - 1 (one workgroup's).  x, v, f carry SENTINELS rows behind nlocal.  Real units: x in A, v thermal at 400 K,
    f of the size of a deck's forces.  state0: a chain state mid-run to seed the handle and the reference with"""
    rng = np.random.default_rng(1000 + seed)
    G = len(styles)
    free = [g for g in range(G) if g not in (one_atom, empty, confined)]
    group = rng.choice(free, size=nlocal).astype(np.int32)
    if nlocal >= 8:
        k = rng.random(nlocal) < minus
        k[rng.integers(0, nlocal)] = True
        group[k] = -1
    if confined is not None:
        assert nlocal >= 2 * BLOCK
        group[BLOCK + rng.choice(BLOCK, size=40, replace=False)] = confined
    if one_atom is not None:
        pick = int(rng.choice(np.nonzero(group == free[0])[0]))
        group[pick] = one_atom
    typ = rng.integers(1, 5, nlocal).astype(np.int32)
    typ[group == -1] = 5
    count = np.array([(group == g).sum() for g in range(G)])
    dof = np.where(count >= 2, 3.0 * count - 3.0, 3.0)
    n = nlocal + SENTINELS
    t_target = np.array([400.0 + 10.0 * g for g in range(G)]) if t_target is None else np.asarray(t_target, dtype=np.float64)
    m_all = np.concatenate([MASS[typ - 1], np.full(SENTINELS, MASS[0])])
    v = rng.normal(size=(n, 3)) * np.sqrt(BOLTZ * 400.0 / (m_all * MVV2E))[:, None]
    x = rng.uniform(0.0, 40.0, (n, 3))
    f = rng.normal(size=(n, 3)) * 10.0
    state0 = np.zeros((G, 8))
    state0[:, 0:3] = rng.normal(size=(G, 3)) * 0.05                     # eta
    state0[:, 3:6] = rng.normal(size=(G, 3)) * 3e-3                     # eta_dot, 1 / fs: of the size of t_freq
    state0[:, 6] = t_target * rng.uniform(0.9, 1.1, G)                  # t_current
    state0[:, 7] = t_target
    return SimpleNamespace(tag=tag, nlocal=int(nlocal), type=typ, group=group, mass=MASS.copy(), style=np.asarray(styles, dtype=np.int32),
                           dof=dof, t_period=np.full(G, 100.0), dt=float(dt), ftm2v=FTM2V, mvv2e=MVV2E, boltz=BOLTZ, count=count,
                           x=np.ascontiguousarray(x), v=np.ascontiguousarray(v), f=np.ascontiguousarray(f), t_target=t_target,
                           state0=state0, seed=seed)


def fresh_forces(c, step):
    """the random f of step `step` of a sequence on case c ([nlocal + SENTINELS][3])"""
    return np.random.default_rng(5000 + 17 * c.seed + step).normal(size=c.f.shape) * 10.0


def nve_case(n):
    return case(f"nve, {n} atoms", n, [0, 0], seed=n % 1000)


def nvt_one():
    return case("nvt, 1 group, 1000 atoms", 1000, [1], seed=1)


def nvt_two():
    return case("nvt, 2 groups, 257 atoms", 257, [1, 1], seed=2)


def nvt_eight():
    """8 groups over 4097 atoms: group 3 has one atom, group 5 none, group 6 lies in the second workgroup's rows only"""
    return case("nvt, 8 groups, 4097 atoms", 4097, [1] * 8, seed=8, one_atom=3, empty=5, confined=6)


def nvt_big():
    return case(f"nvt, 2 groups, {BIG} atoms", BIG, [1, 1], seed=9)


def mixed():
    return case("one nve and one nvt group, 1000 atoms", 1000, [0, 1], seed=3)


def as_nve(c):
    """the same case with every group nve"""
    d = SimpleNamespace(**vars(c))
    d.style = np.zeros_like(c.style)
    d.tag = c.tag + ", all nve"
    return d


def nvt_cases():
    return [nvt_one(), nvt_two(), nvt_eight(), nvt_big()]
