"""No GPU: the boxes of tests/ewald_shape_cases.py reach the plan shapes they are named for, the restated host rules (ew_block,
ew_nsplit, per_split) put every case of tests/test_gpu_ewald_shapes.py on the tier it claims (256 CUs here; the GPU tests repeat
the assertion with the device's own count), and the numpy references carry the net-charge terms the GPU tests rely on."""
import numpy as np
import pytest

import ewald_force_ref as ref
import ewald_shape_cases as sc

PROBES = 4
ALL_CASES = sc.SMALL_CASES + [("uneven", "slab"), ("bigN", "slab"), ("blocks192", "slab"), ("blocks193", "slab")]


@pytest.mark.parametrize("name,mode", ALL_CASES)
def test_every_box_reaches_its_declared_shape(name, mode):
    s = sc.system(name, mode)
    sh = sc.host_shape(s)
    n = s.natoms
    print(name, mode, sh, sc.describe(sc.tier(sh, n - PROBES)))
    assert set(np.unique(s.echeck)) == {-1, 0, 1}
    if name.startswith("blocks"):
        assert n == int(name[6:]) and sh["n_col_tiles"] == 1 and sh["n_row_tiles"] == 1
        return
    sc.check_declared_shape(name, sh, n, n - PROBES)             # after an update every atom but the probes carries charge


def test_the_modes_required_are_there():
    modes = {name: set(sc.BOXES[name][1]) for name in sc.BOXES}
    assert modes["cols2"] == modes["cols3"] == {"ffield", "slab"}
    assert "slab" in modes["bigN"] and "slab" in modes["uneven"]
    for name in ("cols2", "cols3", "half2"):                      # the two modes of a box share their k list
        a, b = (sc.host_shape(sc.system(name, m)) for m in ("slab", "ffield"))
        assert a == b


def test_the_three_tiers_of_ew_block():
    sh = sc.host_shape(sc.system("bigN", "slab"))
    assert sc.ew_block(sh, 1) == 64 and sc.ew_block(sh, 64) == 64 and sc.ew_block(sh, 65) == 128          # 64 up to the atom count
    assert sc.ew_block(sh, 8192) == 8192 and sc.ew_block(sh, 8193) == 8192 and sc.ew_block(sh, 10 ** 6) == 8192   # the hard cap
    big = dict(sh, R_pad=128 * 11, C_pad=960, n_row_tiles=11)      # the headline plan: the cap from EW_TABLES / per_atom
    cap = sc.ew_block(big, 10 ** 6)
    assert 64 < cap < 8192 and cap % 64 == 0
    assert sc.ew_block(sh, 300, debug=100) == 128 and sc.ew_block(sh, 100, debug=192) == 128


def test_case_b_counts():
    s = sc.system(*sc.B_BOX)
    sh = sc.host_shape(s)
    n = s.natoms
    assert n >= max(sc.B_TARGETS) and n - PROBES >= max(sc.B_CHARGED)
    assert [sc.tier(sh, m)["nb_pad"] for m in sc.B_TARGETS] == [64, 64, 64, 128, 192]
    assert [sc.tier(sh, m)["nb_pad"] for m in sc.B_CHARGED] == [128, 128, 192]
    assert sc.tier(sh, n)["nb_pad"] == 192                       # the device entries: every owned atom, whatever its charge


def test_case_c_reaches_every_block_situation_and_split_count():
    seen = {"host": set(), "device": set()}
    nsplits = set()
    for (box, width, charged), want in sc.C_CASES.items():
        s = sc.system(box, "slab")
        sh = sc.host_shape(s)
        assert charged <= s.natoms - PROBES
        th, td = sc.tier(sh, charged, debug=width), sc.tier(sh, s.natoms, debug=width)
        assert sc.situation(th) == want["host"] and sc.situation(td) == want["device"], (box, width, charged, th, td)
        assert th["nsplit"] == want["nsplit"] and th["nb_pad"] == min(width, (charged + 63) // 64 * 64)
        assert th["per_split"] == 64 and th["empty_splits"] == 0                                        # even splits here
        seen["host"].add(want["host"]); seen["device"].add(want["device"]); nsplits.add(th["nsplit"])
    assert seen["host"] == {"full", "one", "single"} and seen["device"] >= {"full", "one", "single"}
    assert nsplits == {1, 2, 3} and {w for _, w, _ in sc.C_CASES} == {64, 128, 192}


def test_case_d_splits_are_uneven():
    s = sc.system(*sc.D_BOX)
    sh = sc.host_shape(s)
    for n in (s.natoms - PROBES, s.natoms):                       # host entries, device entries
        t = sc.tier(sh, n)
        assert (t["nb_pad"], t["nsplit"], t["per_split"], t["splits_used"], t["partial"], t["empty_splits"]) == (2112, 32, 80, 27, 32, 5)
    # ... and at other CU counts the box still leaves an empty trailing split (the rule the GPU test asserts there)
    for cus in (64, 80, 104, 120, 228, 304):
        sc.check_declared_shape("uneven", sh, s.natoms, s.natoms - PROBES, cus)


def test_case_e_tier():
    s = sc.system("bigN", "slab")
    sh = sc.host_shape(s)
    for n in (s.natoms - PROBES, s.natoms):
        t = sc.tier(sh, n)
        assert t["nb_pad"] == 8192 and t["blocks"] == 9 and 0 < t["last"] < 8192 and t["nsplit"] == 32 and t["per_split"] == 256
    assert sc.four_sums_workgroups(s.natoms) == 256 and s.natoms > 65536
    assert 5e7 <= s.natoms * sh["K"] <= 2e8                       # the reference's one O(N K) structure factor


def test_case_i_second_plan_is_smaller_in_rows_and_columns():
    s = sc.system(*sc.I_BOX)
    a, b = sc.host_shape(s), sc.host_shape(sc.with_qsqsum_factor(s, sc.I_QSQ_FACTOR))
    print(a, b)
    assert b["K"] < a["K"] and b["np"] < a["np"] and b["nz"] < a["nz"] and b["kxmax"] < a["kxmax"] and b["kymax"] < a["kymax"]
    assert (b["R_pad"], b["C_pad"]) == (a["R_pad"], a["C_pad"])  # the smaller plan lies inside the larger one's buffers
    for f in (sc.I_QSQ_FACTOR / 2, sc.I_QSQ_FACTOR * 1.5):        # (and the choice is not at a step of the accuracy estimate)
        assert sc.host_shape(sc.with_qsqsum_factor(s, f)) == b


# ---- the references carry the Q terms (case (f)) --------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", sc.F_BOXES)
def test_references_carry_the_net_charge_terms(name, mode):
    s = sc.system(name, mode)
    at, alist, blist = sc.build_atoms(s)
    sc.seed_electrode_charges(at)
    n = at.nlocal
    x = np.ascontiguousarray(at.x[:n])
    q0 = at.q[:n].copy()
    sc.shift_net_charge(at, 1.0)
    q1 = at.q[:n].copy()
    assert abs(q1.sum() - 1.0) < 1e-12 and abs(q0.sum()) < 0.5
    kt = sc.capi.host_ktables(s)
    kv = np.stack([kt["kxvecs"], kt["kyvecs"], kt["kzvecs"]], 1) * (2 * np.pi / (s.prd * np.array([1.0, 1.0, s.slab_volfactor])))
    ug, g, qs = np.asarray(kt["ug"]), float(s.g_ewald), sc.systems.QQRD2E
    L = float(s.prd[2] * s.slab_volfactor)
    V = float(s.prd[0] * s.prd[1] * L)
    slab = bool(s.slabflag)
    # at a FIXED structure factor the energy moves by the self and net-charge terms alone: the analytic amount
    S = ref.structure_factor(x, q1, kv)
    E0 = ref.energy_virial(S, x, q0, kv, ug, g, V, qs, slab, L)[0]
    E1 = ref.energy_virial(S, x, q1, kv, ug, g, V, qs, slab, L)[0]
    Q0, Q1 = q0.sum(), q1.sum()
    z = x[:, 2]
    want = -g * ((q1 * q1).sum() - (q0 * q0).sum()) / np.sqrt(np.pi) - 0.5 * np.pi * (Q1 * Q1 - Q0 * Q0) / (g * g * V)
    neutral = -0.5 * np.pi * (Q1 * Q1 - Q0 * Q0) / (g * g * V)
    if slab:
        M0, M1, N0, N1 = (q0 * z).sum(), (q1 * z).sum(), (q0 * z * z).sum(), (q1 * z * z).sum()
        dslab = 2 * np.pi / V * ((M1 * M1 - Q1 * N1 - Q1 * Q1 * L * L / 12) - (M0 * M0 - Q0 * N0 - Q0 * Q0 * L * L / 12))
        want += dslab
        neutral += 2 * np.pi / V * (-(Q1 - Q0) * N1 - (Q1 * Q1 - Q0 * Q0) * L * L / 12)
    scale = qs * ref.ksum(S, ug)
    assert abs((E1 - E0) - qs * want) <= 1e-12 * max(scale, abs(qs * want))
    assert abs(qs * neutral) > 1e-6 * scale                      # the Q terms are far above the GPU tests' 1e-11 of the scale
    # the per-atom energies carry them too: they sum to the energy, and without Q they do not
    tg = np.arange(n)
    e1 = ref.forces_eatom(S, x, q1, kv, ug, g, V, qs, tg, slab, L)[1]
    assert abs(e1.sum() - E1) <= 1e-12 * max(scale, abs(E1))
    qn = q1 - Q1 / n                                              # (the same atoms made neutral: every Q term gone)
    en = ref.forces_eatom(S, x, qn, kv, ug, g, V, qs, tg, slab, L)[1]
    assert abs(en.sum() - e1.sum()) > 1e-6 * scale
    if slab:
        # the slab force's Q z term: f_z is minus the z derivative of the energy, S re-formed at the moved atom
        f1 = ref.forces_eatom(S, x, q1, kv, ug, g, V, qs, tg, slab, L)[0]
        i = int(np.argmax(np.abs(q1 * z)))
        h = 1e-4
        ep = []
        for d in (h, -h):
            xm = x.copy()
            xm[i, 2] += d
            ep.append(ref.energy_virial(ref.structure_factor(xm, q1, kv), xm, q1, kv, ug, g, V, qs, slab, L)[0])
        fd = -(ep[0] - ep[1]) / (2 * h)
        assert abs(f1[i, 2] - fd) <= 1e-6 * np.abs(f1).max()
        assert abs(qs * 4 * np.pi / V * q1[i] * Q1 * z[i]) > 1e-6 * np.abs(f1).max()       # (the term is not negligible there)
