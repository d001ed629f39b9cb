"""numpy restatements of the two rules of DESIGN.md section 24 as include/conp_hip.h states them -- conp_efield_* (`fix efield` with
a constant field, optionally coupled to the fix scalar) and conp_observe_* (per-group sums of overlapping groups) -- and the inputs of
the GPU tests.

Both rules are written ONCE over a number type (kind), as tests/integrate_ref.py does:
  - "f64": plain float64 in the written order: bit for bit what the kernels do per atom (nothing but + - * and conversions).  Its
    sums over atoms use numpy's order, not the kernels' trees: sums are compared through the bound only.
  - "ld": np.longdouble values that carry the sum of the magnitudes of their terms (integrate_ref.Mag: |a| + |b| for a sum,
    m_a m_b for a product).  The GPU tests bound |got - value| by TOL * magnitude, entry-wise; sums over more than 2^13 atoms by
    n 2^-53 of the magnitude (tol_of), the convention of sections 22 and 23.
"""
import os
import re
from types import SimpleNamespace

import numpy as np

from integrate_ref import BOLTZ, FTM2V, LD, MVV2E, SENTINELS, TOL, Mag, frac, tol_of  # noqa: F401

# launch shapes of conp_efield.hip, restated (test_launch_shapes_restated below compares them with csrc/conp_kernels.h)
B = 256           # threads of a workgroup of both atom kernels: one atom each
F = 256           # threads of a finishing workgroup: from B * F + 1 atoms on a thread adds a second row of partial sums
BIG = B * F + 1
SIZES = (1, B - 1, B, B + 1, 1000, BIG)
EFIELD_W, OBSERVE_W, MAX_GROUPS = 11, 10, 16
QE2F = 23.060549                                              # LAMMPS `units real`
MASS = np.array([67.07, 15.04, 57.12, 144.96, 12.001])        # the IL decks' types; 5 is the electrode
PRD = (32.2, 34.4, 136.0)                                     # the IL decks' box
NAN = float("nan")
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lammps-user-conp2_amd", "csrc")


def test_launch_shapes_restated():
    k = open(os.path.join(CSRC, "conp_kernels.h")).read()
    val = lambda name: int(re.search(rf"constexpr int {name} = (\d+);", k).group(1))
    assert (val("EFIELD_BLOCK"), val("EFIELD_FINISH"), val("OBSERVE_BLOCK"), val("OBSERVE_FINISH")) == (B, F, B, F)
    assert val("EFIELD_W") == EFIELD_W
    hdr = open(os.path.join(CSRC, "..", "..", "include", "conp_hip.h")).read()
    assert re.search(rf"#define CONP_OBSERVE_MAX_GROUPS {MAX_GROUPS}\b", hdr) and re.search(rf"#define CONP_OBSERVE_W {OBSERVE_W}\b", hdr)
    src = open(os.path.join(CSRC, "conp_efield.hip")).read()
    assert "r += EFIELD_FINISH" in src and "r += OBSERVE_FINISH" in src
    assert "blockIdx.x * EFIELD_BLOCK + threadIdx.x" in src and "blockIdx.x * OBSERVE_BLOCK + threadIdx.x" in src
    assert BIG == B * F + 1 and BIG <= 100000 and SIZES == (1, B - 1, B, B + 1, 1000, BIG)


# ---- the number types -----------------------------------------------------------------------------------------------------------------
def _lift(kind, a):
    return Mag(a) if kind == "ld" else np.asarray(a, dtype=np.float64)[()]


def _val(a):
    return a.v if isinstance(a, Mag) else a


def _sum(a, rows):
    """the sum over the rows under the mask (a Mag keeps the sum of the magnitudes)"""
    if isinstance(a, Mag):
        return Mag(a.v[rows].sum(), a.m[rows].sum())
    return a[rows].sum()


def _stack(cols):
    if isinstance(cols[0], Mag):
        return Mag(np.stack([c.v for c in cols], axis=-1), np.stack([c.m for c in cols], axis=-1))
    return np.stack(cols, axis=-1)


def _masked(a, rows):
    """a with the rows outside the mask set to exactly 0"""
    if isinstance(a, Mag):
        return Mag(np.where(rows, a.v, 0), np.where(rows, a.m, 0))
    return np.where(rows, a, 0.0)


def unwrapped(kind, x, image, prd):
    """u_c = x_c + ((double)image_c prd_c) per column; image None: u_c = x_c"""
    out = []
    for c in range(3):
        u = _lift(kind, x[:, c])
        if image is not None:
            u = u + (_lift(kind, image[:, c].astype(np.float64)) * _lift(kind, prd[c]))
        out.append(u)
    return out


# ---- rule 1: the field ----------------------------------------------------------------------------------------------------------------
def field_of(kind, e, qe2f=QE2F, couple=0, couple_scale=0.0, s=0.0):
    n = lambda v: _lift(kind, v)
    ex, ey = n(qe2f) * n(e[0]), n(qe2f) * n(e[1])
    ez = n(qe2f) * (n(e[2]) + n(couple_scale) * n(s)) if couple else n(qe2f) * n(e[2])
    return ex, ey, ez


def efield(kind, c, e, image=True, sel=None, couple=0, couple_scale=0.0, s=0.0, x=None, img=None):
    """-> f (the force array behind the call; "ld": the added force), add [n][3], vatom [n][6], out [11], E = (ex, ey, ez)"""
    nl = c.nlocal
    sel = (c.sel if sel is None else np.asarray(sel))[:nl] != 0
    x = (c.x if x is None else x)[:nl]
    img = ((c.image if img is None else img)[:nl]) if image else None
    ex, ey, ez = field_of(kind, e, c.qe2f, couple, couple_scale, s)
    q = _lift(kind, c.q[:nl])
    u = unwrapped(kind, x, img, c.prd)
    fx, fy, fz = q * ex, q * ey, q * ez
    energy = -((fx * u[0] + fy * u[1]) + fz * u[2])
    v = [fx * u[0], fy * u[1], fz * u[2], fx * u[1], fx * u[2], fy * u[2]]
    add = _stack([_masked(t, sel) for t in (fx, fy, fz)])
    vatom = _stack([_masked(t, sel) for t in v])
    cols = [energy, fx, fy, fz] + v
    out = [_sum(t, sel) for t in cols] + [_lift(kind, float(sel.sum()))]
    if kind == "ld":
        out = Mag(np.array([t.v for t in out], dtype=LD), np.array([t.m for t in out], dtype=LD))
        f = add
    else:
        out = np.array(out, dtype=np.float64)
        f = c.f[:nl].copy()
        f[sel] = f[sel] + add[sel]
    return SimpleNamespace(f=f, add=add, vatom=vatom, out=out, E=(ex, ey, ez), nsel=int(sel.sum()))


# ---- rule 2: the per-group sums ---------------------------------------------------------------------------------------------------------
def observe(kind, c, with_v=True, image=True, mask=None, ngroups=None, x=None, img=None):
    """-> out [ngroups][10]"""
    nl = c.nlocal
    mask = (c.mask if mask is None else np.asarray(mask))[:nl]
    G = c.ngroups if ngroups is None else ngroups
    x = (c.x if x is None else x)[:nl]
    img = ((c.image if img is None else img)[:nl]) if image else None
    q = _lift(kind, c.q[:nl])
    m = _lift(kind, c.mass[c.type[:nl] - 1])
    u = unwrapped(kind, x, img, c.prd)
    one = _lift(kind, np.ones(nl))
    zero = _lift(kind, np.zeros(nl))
    cols = [one, q, q * u[0], q * u[1], q * u[2]]
    if with_v:
        vx, vy, vz = (_lift(kind, c.v[:nl, k]) for k in range(3))
        cols += [m * ((vx * vx + vy * vy) + vz * vz), m * vx, m * vy, m * vz]
    else:
        cols += [zero] * 4
    cols.append(m)
    rows = []
    for g in range(G):
        member = ((mask >> g) & 1) != 0
        rows.append([_sum(t, member) for t in cols])
    if kind == "ld":
        return Mag(np.array([[t.v for t in r] for r in rows], dtype=LD), np.array([[t.m for t in r] for r in rows], dtype=LD))
    return np.array(rows, dtype=np.float64)


# ---- input builders ---------------------------------------------------------------------------------------------------------------------
def _pad(a, fill):
    tail = np.full((SENTINELS,) + a.shape[1:], fill, dtype=a.dtype)
    return np.ascontiguousarray(np.concatenate([a, tail]))


def case(tag, nlocal, seed=0, masks="nested", unselected=0.1, prd=PRD):
    """nlocal owned atoms in real units: wrapped x in the IL box with image counters in -2 .. 2, charges of the decks' size, thermal
    v at 400 K, forces of a deck's size; a fraction `unselected` of the atoms outside the field's group (at least one where
    nlocal >= 8).  x, q, v, f carry SENTINELS rows of NaN behind nlocal, image rows of a large counter.
    masks: "one" (1 group, a tenth of the atoms in none), "nested" (3 groups, 2 in 1 in 0, a quarter of the atoms in none), "sixteen"
    (16 random groups: group 11 is empty, a tenth of the atoms are in no group, one atom is in all the others)"""
    rng = np.random.default_rng(2400 + seed)
    prd = np.asarray(prd, dtype=np.float64)
    x = rng.uniform(0.0, 1.0, (nlocal, 3)) * prd
    image = rng.integers(-2, 3, (nlocal, 3)).astype(np.int32)
    typ = rng.integers(1, len(MASS) + 1, nlocal).astype(np.int32)
    q = np.round(rng.normal(size=nlocal) * 0.5, 4)
    q[rng.random(nlocal) < 0.2] = 0.0
    v = rng.normal(size=(nlocal, 3)) * np.sqrt(BOLTZ * 400.0 / (MASS[typ - 1] * MVV2E))[:, None]
    f = rng.normal(size=(nlocal, 3)) * 10.0
    sel = np.ones(nlocal, dtype=np.int32)
    if nlocal >= 8:
        k = rng.random(nlocal) < unselected
        if unselected > 0:
            k[rng.integers(0, nlocal)] = True
        sel[k] = 0
    if masks == "one":
        G = 1
        mask = (rng.random(nlocal) >= 0.1).astype(np.int32)
    elif masks == "nested":
        G = 3
        depth = rng.integers(0, 4, nlocal)                     # 0: in no group; d: in groups 0 .. d - 1
        mask = ((1 << depth) - 1).astype(np.int32)
    elif masks == "sixteen":
        G = 16
        mask = rng.integers(0, 1 << 16, nlocal).astype(np.int32)
        mask[rng.random(nlocal) < 0.1] = 0
        mask &= ~(1 << 11)                                     # group 11 is empty ...
        mask[nlocal // 2] = (1 << 16) - 1 - (1 << 11)          # ... and one atom holds every other bit
    else:
        raise ValueError(masks)
    if nlocal == 1 and masks != "sixteen":
        mask[0] = (1 << G) - 1
    return SimpleNamespace(tag=f"{tag}, n {nlocal}", nlocal=nlocal, qe2f=QE2F, prd=tuple(float(p) for p in prd), type=typ, mass=MASS.copy(),
                           sel=sel, mask=mask, ngroups=G, x=_pad(x, NAN), q=_pad(q, NAN), v=_pad(v, NAN), f=_pad(f, NAN),
                           image=_pad(image, 1 << 20))


def full_mask_case(nlocal, seed=0):
    """16 groups and every atom holds every bit"""
    c = case("16 groups, every bit", nlocal, seed=seed, masks="sixteen")
    c.mask[:] = (1 << 16) - 1
    return c


def with_(c, **k):
    d = dict(vars(c))
    d.update(k)
    return SimpleNamespace(**d)


FIELDS = {"x": (0.013, 0.0, 0.0), "y": (0.0, -0.021, 0.0), "z": (0.0, 0.0, -1.0 / PRD[2]), "xyz": (0.013, -0.021, -0.0147)}


def _golden(name):
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name))


def dilute_case():
    """tests/golden/deck_dilute.npz: all 432 atoms owned and selected, e = (0, 0, -potdiff / lz) with the deck's potdiff 1.0; the file
    carries no image counters: 0"""
    d = _golden("deck_dilute.npz")
    n = len(d["type"])
    prd = d["boxhi"] - d["boxlo"]
    rng = np.random.default_rng(432)
    mass = np.array([15.9994, 1.008, 12.011, 22.98977])
    typ = d["type"].astype(np.int32)
    v = rng.normal(size=(n, 3)) * np.sqrt(BOLTZ * 298.0 / (mass[typ - 1] * MVV2E))[:, None]
    c = SimpleNamespace(tag="the dilute deck", nlocal=n, qe2f=QE2F, prd=tuple(float(p) for p in prd), type=typ, mass=mass,
                        sel=np.ones(n, dtype=np.int32), mask=np.ones(n, dtype=np.int32), ngroups=1, x=_pad(d["x"].copy(), NAN),
                        q=_pad(d["q"].copy(), NAN), v=_pad(v, NAN), f=_pad(rng.normal(size=(n, 3)) * 10.0, NAN),
                        image=_pad(np.zeros((n, 3), dtype=np.int32), 1 << 20))
    c.e = (0.0, 0.0, -1.0 / c.prd[2])
    return c


IL_GROUPS = ("sol", "eleleft", "eleright", "ele", "all")


def il_case():
    """tests/golden/deck_il.npz with the decks' groups: sol (types 1-4), eleleft (molecule 641), eleright (642), ele (type 5), all"""
    d = _golden("deck_il.npz")
    typ, mol = d["type"].astype(np.int32), d["mol"]
    n = len(typ)
    prd = d["boxhi"] - d["boxlo"]
    rng = np.random.default_rng(3776)
    members = [typ <= 4, mol == 641, mol == 642, typ == 5, np.ones(n, dtype=bool)]
    mask = np.zeros(n, dtype=np.int32)
    for g, mem in enumerate(members):
        mask |= mem.astype(np.int32) << g
    v = rng.normal(size=(n, 3)) * np.sqrt(BOLTZ * 400.0 / (MASS[typ - 1] * MVV2E))[:, None]
    v[typ == 5] = 0.0
    return SimpleNamespace(tag="the IL deck", nlocal=n, qe2f=QE2F, prd=tuple(float(p) for p in prd), type=typ, mass=MASS.copy(),
                           sel=(typ <= 4).astype(np.int32), mask=mask, ngroups=len(members), x=_pad(d["x"].copy(), NAN),
                           q=_pad(d["q"].copy(), NAN), v=_pad(v, NAN), f=_pad(rng.normal(size=(n, 3)) * 10.0, NAN),
                           image=_pad(rng.integers(-2, 3, (n, 3)).astype(np.int32), 1 << 20))


def efield_cases():
    """every input the GPU test of the field runs: (case, e, options of efield())"""
    out = []
    for n in SIZES:
        out.append((case("ladder", n, seed=n % 97), FIELDS["xyz"], {}))
    c = case("axes", 1000, seed=5)
    for k in ("x", "y", "z"):
        out.append((c, FIELDS[k], {}))
    out.append((c, FIELDS["xyz"], dict(image=False)))
    out.append((with_(c, tag="all selected", sel=np.ones(c.nlocal, dtype=np.int32)), FIELDS["xyz"], {}))
    out.append((with_(c, tag="none selected", sel=np.zeros(c.nlocal, dtype=np.int32)), FIELDS["xyz"], {}))
    out.append((with_(c, tag="zero charges", q=_pad(np.zeros(c.nlocal), NAN)), FIELDS["xyz"], {}))
    d = dilute_case()
    out.append((d, d.e, {}))
    return out


MASK_SHAPES = ("one", "nested", "sixteen")


def observe_cases():
    """every input the GPU test of the sums runs"""
    out = [case(f"ladder, {m}", n, seed=n % 89 + 7 * k, masks=m) for n in SIZES for k, m in enumerate(MASK_SHAPES)]
    out += [full_mask_case(n, seed=3) for n in (B + 1, 1000)]
    out.append(il_case())
    return out
