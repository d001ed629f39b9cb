"""The boxes of tests/test_gpu_ewald_shapes.py and the host rules that decide which code a call of the exact Ewald entries runs,
restated: tests/test_ewald_shape_cases_math.py checks on the CPU (capi.host_ktables) that every box reaches the shape it is named
for, the GPU tests assert the same from the handle (fx.info(), fx.ktables()) and the device's CU count before they compare.

Restated rules:
  KPlan::build (conp_host.cpp):  nz = kzmax + 1, n_col_tiles = ceil(ceil(nz / 16) / 10), kzt = ceil(ceil(nz / n_col_tiles) / 8) * 8;
      np = the distinct planar vectors (kx, +-ky) of the k list, origin included; n_row_tiles = ceil(np / 64),
      R_pad = 128 n_row_tiles, C_pad = 320 n_col_tiles.
  EwaldQuery::block (conp_ewaldquery.cpp):  min(cap, max(64, 64 ceil(n / 64))), cap = max(64, min(8192, 64 floor(80 MiB / per_atom / 64))) or the
      width of conp_debug_set_ew_block, per_atom = 8 (R_pad + C_pad + 6 + 2 (kxmax + 2) + 2 (kymax + 1)) bytes.
  EwaldQuery::nsplit (conp_ewaldquery.cpp):  max(1, min(6 CUs / workgroups + 1, 32, nb_pad / 64)), workgroups = C_pad / 64 * n_row_tiles, lowered
      while nsplit slices of R_pad C_pad doubles exceed 40 MiB.
  launch_ew_sk (conp_potential.hip):  per_split = 16 ceil(ceil(nb_pad / nsplit) / 16); split z takes the columns
      [z per_split, min(nb_pad, (z + 1) per_split)) of the block, an empty range returns at once.
  kspace_four_sums / ew_energy_virial: min(256, ceil(n / 256)) workgroups of 256 threads, strided beyond 65 536 entries."""
import dataclasses
import functools

import numpy as np

from conp_amd import capi, neighbor, systems

EW_TABLES, EW_SLICES = 80 << 20, 40 << 20
CUS = 256                                        # an MI355X; the GPU tests take the device's own count


def _sr(**kw):
    return lambda mode: systems.small_random(mode=mode, **kw)


def _sf(**kw):
    return lambda mode: systems.synthetic_fast(mode=mode, **kw)


# name -> (maker(mode), modes).  lz of an ffield box is three times that of its slab twin: the same z period, the same k list.
#   tiny    one row tile, np < 64, K <= 256 (one workgroup of ew_energy_virial_kernel), kzmax < 80: no second half of a column tile
#   half2   one column tile, 80 <= kzmax <= 159 (h = 1 of the force kernels), kzt % 16 == 8
#   cols2   two column tiles, kzt % 16 == 8, >= 3 row tiles; the 64 planar vectors of largest |k_p| list no kz in column tile 1
#   cols3   three column tiles, fewer than 200 atoms
#   wide    >= 5 row tiles, the last ragged, kzmax < 160
#   uneven  about 2100 atoms on a small plan: nb_pad 2112 over 32 splits of 80 columns, a partial split and empty trailing ones
#   bigN    > 65 536 charged owned atoms, ew_block at its hard cap 8192, a ragged last block, 32 splits, K ~ 1500
# check_declared_shape asserts exactly this.
BOXES = {
    "tiny": (_sr(ne_side=4, n_elyte=96, lz=40.0, g_ewald=0.25, accuracy_relative=1e-3), ("ffield", "slab")),
    "half2": (lambda mode: systems.small_random(ne_side=4, n_elyte=96, lz=148.0 if mode == "slab" else 444.0, mode=mode), ("slab", "ffield")),
    # (the sphere of listed k is cut by kzmax: only a thin outer ring of planar vectors stays below kzt, so np is several hundred)
    "cols2": (lambda mode: systems.small_random(ne_side=6, n_elyte=64, lz=60.0 if mode == "slab" else 180.0, g_ewald=1.0,
                                                accuracy_relative=1e-7, mode=mode), ("slab", "ffield")),
    "cols3": (lambda mode: systems.small_random(ne_side=4, n_elyte=64, lz=700.0 if mode == "slab" else 2100.0, g_ewald=0.6, mode=mode),
              ("slab", "ffield")),
    "wide": (_sr(ne_side=8, n_elyte=32, lz=40.0, g_ewald=0.8), ("ffield",)),
    # 2112 = 33 x 64 owned atoms, 2048 of them electrolyte sites: case (d), the uneven splits
    "uneven": (_sf(n_cells_x=4, n_cells_y=2, lz=100.0, n_elyte=2048, cutoff=6.0, accuracy_relative=1e-4, g_ewald=0.3), ("slab",)),
    # 66 000 electrolyte sites far denser than a liquid over 2 x 128 electrode atoms: only k-space is under test
    "bigN": (_sf(n_cells_x=8, n_cells_y=4, lz=140.0, n_elyte=66000, cutoff=4.0, accuracy_relative=1e-3, g_ewald=0.22), ("slab",)),
}
SMALL = ("tiny", "half2", "cols2", "cols3", "wide")
SMALL_CASES = [(name, mode) for name in SMALL for mode in BOXES[name][1]]


def _without_last_elyte(s, k):
    """the box without its last k electrolyte sites, tags renumbered (an odd atom count: 64 electrode atoms + 4 m sites is even)"""
    keep = np.ones(s.natoms, bool)
    keep[np.nonzero(s.echeck == 0)[0][-k:]] = False
    n = int(keep.sum())
    return dataclasses.replace(s, name=f"{s.name}-{k}", x=s.x[keep].copy(), q=s.q[keep].copy(), type=s.type[keep].copy(),
                               tag=np.arange(1, n + 1, dtype=np.int32), echeck=s.echeck[keep].copy())


# case (c): 192 = 3 x 64 and 193 owned atoms on the plan of the sibling tests' `small` box
BOXES["blocks192"] = (_sr(ne_side=4, n_elyte=128, lz=60.0), ("slab",))
BOXES["blocks193"] = (lambda mode: _without_last_elyte(systems.small_random(ne_side=4, n_elyte=132, lz=60.0, mode=mode), 3), ("slab",))

# case (b) on `tiny` (160 owned atoms): the selections of the potential entry and the charged-atom counts of the force entries
B_BOX = ("tiny", "ffield")
B_TARGETS = (1, 63, 64, 65, 129)
B_CHARGED = (127, 128, 129)                      # 64 m - 1, 64 m, 64 m + 1 at m = 2

# case (c): (box, width of conp_debug_set_ew_block, charged atoms) -> what the host entries' force blocks (n = the charged atoms) and
# the device entries' (n = the owned atoms) look like: "full" the last block is exactly full, "one" it holds one atom, "single" one
# block takes everything; and the splits of a block
C_CASES = {
    ("blocks192", 64, 128): dict(host="full", device="full", nsplit=1),
    ("blocks192", 128, 128): dict(host="single", device=None, nsplit=2),
    ("blocks192", 192, 188): dict(host="single", device="single", nsplit=3),
    ("blocks193", 64, 129): dict(host="one", device="one", nsplit=1),
    ("blocks193", 128, 129): dict(host="one", device=None, nsplit=2),
    ("blocks193", 192, 189): dict(host="single", device="one", nsplit=3),
}
D_BOX = ("uneven", "slab")
F_BOXES = (("tiny", "ffield"), ("half2", "slab"))           # case (f): a net charge of 1 e
G_BOX = ("half2", "slab")                                   # case (g): 160 owned atoms, blocks of 64 and 128 differ
# case (i): a live handle re-planned between calls.  The k list follows sum q^2 through the accuracy estimate alone (KTables::build:
# the axis cut-offs are integers, nothing else reads it), so a twentieth of the box's own sum is a smaller plan of the same box:
# K 83 -> 5, planar rows 7 -> 3, kz columns 8 -> 2, kxmax = kymax 2 -> 1, inside the same padded sizes (one row tile, one column tile)
I_BOX = ("tiny", "slab")
I_QSQ_FACTOR = 0.05


def situation(t):
    """the block situation of a tier: "full", "one", "single" (a single block that is exactly full counts as single) or None"""
    if t["blocks"] == 1:
        return "single"
    return "full" if t["last"] == t["nb_pad"] else "one" if t["last"] == 1 else None


@functools.lru_cache(maxsize=None)
def system(name, mode):
    """the box; callers copy what they change"""
    make, modes = BOXES[name]
    assert mode in modes, (name, mode)
    return make(mode)


def with_qsqsum_factor(s, factor):
    """the box with every charge scaled so that sum q^2 is `factor` times its own"""
    return dataclasses.replace(s, name=f"{s.name}*{factor}", q=s.q * np.sqrt(factor))


def plan_shape(kxvecs, kyvecs, kzvecs, kcount_dims, unitk=None):
    """the figures of KPlan::build that the Ewald entries' launches depend on, from a k list"""
    kx, ky, kz = (np.asarray(a).astype(np.int64) for a in (kxvecs, kyvecs, kzvecs))
    nz = int(kcount_dims[2]) + 1
    n_col_tiles = -(-(-(-nz // 16)) // 10)
    kzt = -(-(-(-nz // n_col_tiles)) // 8) * 8
    planar = {(0, 0): 0}
    for a, b, c in zip(kx.tolist(), ky.tolist(), np.abs(kz).tolist()):
        planar[(a, b)] = max(planar.get((a, b), 0), c)
    planar[(0, 0)] = nz - 1                                     # the z axis: every kz up to kzmax
    npl = len(planar)
    n_row_tiles = -(-npl // 64)
    out = dict(K=len(kx), nz=nz, n_col_tiles=n_col_tiles, kzt=kzt, np=npl, n_row_tiles=n_row_tiles, R_pad=128 * n_row_tiles,
               C_pad=320 * n_col_tiles, kxmax=int(kcount_dims[0]), kymax=int(kcount_dims[1]))
    if unitk is not None:
        # the largest listed kz of the 64 planar vectors of largest |k_p|^2 (the sphere cut: the outermost row tile is the shortest)
        key = sorted(planar, key=lambda p: (p[0] * unitk[0]) ** 2 + (p[1] * unitk[1]) ** 2)
        out["kz_outer64"] = max(planar[p] for p in key[-64:])
        out["kz_reach"] = max(planar.values())
    return out


def host_shape(s):
    kt = capi.host_ktables(s)
    assert int(kt["kcount_dims"][2]) == kt["kzmax"]              # nz = kzmax + 1
    return plan_shape(kt["kxvecs"], kt["kyvecs"], kt["kzvecs"], kt["kcount_dims"], 2 * np.pi / np.asarray(s.prd[:2]))


def handle_shape(fx):
    kt, info = fx.ktables(), fx.info()
    assert int(info.kcount_dims[2]) == info.kzmax
    return plan_shape(kt["kxvecs"], kt["kyvecs"], kt["kzvecs"], list(info.kcount_dims), list(info.unitk)[:2])


def ew_block(sh, n, debug=0):
    per_atom = 8 * (sh["R_pad"] + sh["C_pad"] + 6 + 2 * (sh["kxmax"] + 2) + 2 * (sh["kymax"] + 1))
    cap = max(64, min(8192, EW_TABLES // per_atom // 64 * 64))
    if debug > 0:
        cap = (debug + 63) // 64 * 64
    return min(cap, max(64, (n + 63) // 64 * 64))


def ew_nsplit(sh, nb_pad, num_cus=CUS):
    wgs = max(1, sh["C_pad"] // 64 * sh["n_row_tiles"])
    nsplit = max(1, min(6 * num_cus // wgs + 1, 32, nb_pad // 64))
    while nsplit > 1 and nsplit * sh["R_pad"] * sh["C_pad"] * 8 > EW_SLICES:
        nsplit -= 1
    return nsplit


def per_split(nb_pad, nsplit):
    return ((nb_pad + nsplit - 1) // nsplit + 15) // 16 * 16


def tier(sh, n, num_cus=CUS, debug=0):
    """what a call over n atoms (columns, or targets) runs: block width, blocks, atoms of the last block, splits of a block and how
    the block's columns fall onto them"""
    nb_pad = ew_block(sh, n, debug)
    nsplit = ew_nsplit(sh, nb_pad, num_cus)
    ps = per_split(nb_pad, nsplit)
    used = -(-nb_pad // ps)                                     # splits with columns; the last of them holds `partial` columns
    return dict(nb_pad=nb_pad, blocks=max(1, -(-n // nb_pad)), last=n - (max(1, -(-n // nb_pad)) - 1) * nb_pad, nsplit=nsplit,
                per_split=ps, splits_used=used, empty_splits=nsplit - used, partial=nb_pad - (used - 1) * ps,
                n_col_tiles=sh["n_col_tiles"], kzt=sh["kzt"], n_row_tiles=sh["n_row_tiles"])


def describe(t):
    return (f"nb_pad {t['nb_pad']}, {t['blocks']} block(s), last {t['last']}, nsplit {t['nsplit']}, per_split {t['per_split']} "
            f"({t['empty_splits']} empty), n_col_tiles {t['n_col_tiles']}, kzt {t['kzt']}, {t['n_row_tiles']} row tile(s)")


def four_sums_workgroups(n):
    return max(1, min(256, (n + 255) // 256))


def check_declared_shape(name, sh, n_owned, n_charged, num_cus=CUS):
    """the shape the box is named for"""
    if name == "tiny":
        assert sh["n_row_tiles"] == 1 and sh["np"] < 64 and sh["K"] <= 256 and sh["nz"] - 1 < 80
    elif name == "half2":
        assert sh["n_col_tiles"] == 1 and 80 <= sh["nz"] - 1 <= 159 and sh["kzt"] % 16 == 8
    elif name == "cols2":
        assert sh["n_col_tiles"] == 2 and sh["kzt"] % 16 == 8 and sh["n_row_tiles"] >= 3
        assert sh["kz_reach"] >= sh["kzt"] > sh["kz_outer64"], (sh["kz_reach"], sh["kzt"], sh["kz_outer64"])
    elif name == "cols3":
        assert sh["n_col_tiles"] == 3 and n_owned < 200
    elif name == "wide":
        assert sh["n_row_tiles"] >= 5 and sh["np"] % 64 != 0 and sh["nz"] - 1 < 160
    elif name == "uneven":
        t = tier(sh, n_charged, num_cus)
        if num_cus == CUS:
            assert (t["nb_pad"], t["nsplit"], t["per_split"]) == (2112, 32, 80), t
            assert (t["splits_used"], t["partial"], t["empty_splits"]) == (27, 32, 5), t
        assert t["nb_pad"] % (t["nsplit"] * 16) != 0 and t["empty_splits"] >= 1 and t["blocks"] == 1, t
    elif name == "bigN":
        t = tier(sh, n_charged, num_cus)
        assert n_charged > 65536 and t["nb_pad"] == 8192 and t["blocks"] >= 9 and t["last"] < 8192, t
        assert sh["K"] <= 4000
        assert four_sums_workgroups(n_owned) == 256 and n_owned > 256 * 256
        if num_cus == CUS:
            assert t["nsplit"] == 32, t
    else:
        raise KeyError(name)
    if name in SMALL:
        assert n_owned <= 300, n_owned


# ---- atoms ----------------------------------------------------------------------------------------------------------------
def shift_net_charge(at, Q=1.0):
    """the charged electrolyte atoms shifted by one constant so that the owned atoms' charges sum to Q (ghosts follow)"""
    n = at.nlocal
    ely = np.nonzero((at.echeck[:n] == 0) & (at.q[:n] != 0))[0]
    q = at.q[:n].copy()
    q[ely] += (Q - q.sum()) / len(ely)
    assert np.all(q[ely] != 0)
    at.q[:] = q[at.owner]


def seed_electrode_charges(at, seed=5, scale=0.02):
    """small seeded charges on the electrode atoms in place of an update (bigN: only the k tables of the handle are needed)"""
    n = at.nlocal
    ele = np.nonzero(at.echeck[:n] != 0)[0]
    q = at.q[:n].copy()
    q[ele] = np.random.default_rng(seed).normal(scale=scale, size=len(ele))
    at.q[:] = q[at.owner]


def build_atoms(s):
    return neighbor.build_lists(s)


def zero_charges_to(at, n_charged, seed=17):
    """seeded electrolyte atoms lose their charge until n_charged owned atoms carry one (ghosts follow): the host entries then see
    fewer columns and targets, the device entries the same atoms with zero charge"""
    n = at.nlocal
    q = at.q[:n].copy()
    ely = np.nonzero((at.echeck[:n] == 0) & (q != 0))[0]
    drop = int((q != 0).sum()) - n_charged
    assert 0 <= drop <= len(ely), (drop, len(ely))
    q[np.random.default_rng(seed).choice(ely, drop, replace=False)] = 0.0
    at.q[:] = q[at.owner]
    assert int((at.q[:n] != 0).sum()) == n_charged
