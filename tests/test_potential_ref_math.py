"""no GPU: the longdouble restatements of tests/potential_ref.py against each other -- the reference's pair loop over a half list,
the gather form of conp_potential_atom_device (own row, then transposed entries, per selected row) and the definition without any
list (every image of every owned atom) -- with newton on after folding the ghost rows onto their owners and with newton off; the
rsq floor, the three eta branches, the special bits; and the finishing formula on numbers worked by hand.  The three forms differ
in the order of their sums only: a row sums fewer than 1024 terms, so two orders differ by less than 1024 longdouble roundings of
the cancellation-free magnitude A (1.1e-16 A: four orders below the 1e-12 A of the GPU tests)."""
import dataclasses

import numpy as np
import pytest

import potential_ref as pr
import transpose_ref as tr
from conp_amd import neighbor, systems
from pair_force_ref import LD

TOL = 1024 * float(np.finfo(LD).eps)     # of A: n eps sum |term| bounds a sum of n terms taken in another order
# Against the definition without a list the pairs' geometry is not the same bits: with newton on a pair may be listed as (b, ghost of
# a), whose float64 ghost coordinate x_a + L carries a rounding of up to 2^-53 |x| <= 4.5e-15 A that x_b - L does not.  A term
# q dudq(r) changes by (1 / r + 2 g^2 r + ...) dr < 5 / A * 4.5e-15 A at the listed distances (r > 0.5 A): 2.5e-14 of the term.
TOL_DIRECT = 1e-13


def small(newton, eta_on=True, seed=7):
    """systems.small_random with four zero-charge probes (one exactly on an electrolyte atom), half lists with special bits"""
    s = dataclasses.replace(systems.small_random(ne_side=4, n_elyte=96, seed=seed), newton=newton, eletypes=None)
    n = s.natoms
    el = np.nonzero((s.echeck == 0) & (s.q != 0))[0]
    q, x = s.q.copy(), s.x.copy()
    centre = s.boxlo + 0.5 * np.asarray(s.prd)
    for k, i in enumerate(el[:4]):
        q[i] = 0.0
        x[i] = centre + np.array([0.37 * k, -0.21 * k, 0.53 * k - 0.8])
    x[el[3]] = x[el[10]]                                            # the rsq floor
    s = dataclasses.replace(s, q=q, x=x)
    at, lst, _ = neighbor.build_lists(s, special_frac=0.2)
    rng = np.random.default_rng(3)
    sel_owned = rng.random(n) < 0.5
    sel_owned[el[:4]] = True
    sel_owned[np.nonzero(s.echeck != 0)[0][:5]] = True
    eta_owned = (s.echeck != 0) if eta_on else np.zeros(n, bool)
    flags = (sel_owned.astype(np.int32) | (eta_owned.astype(np.int32) << 1))[at.owner]
    return s, at, lst, flags, el[:4]


def args_of(s, at, flags, lst, eta, newton):
    return (at.x, at.q, at.type, flags, at.nlocal, lst, s.cutsq_table(), pr.cut_coulsq_of(s.cutoff, s.g_ewald), s.g_ewald, eta, newton)


@pytest.mark.parametrize("newton", [False, True])
@pytest.mark.parametrize("eta_on", [False, True])
def test_loop_gather_and_definition_agree(newton, eta_on):
    s, at, lst, flags, probes = small(newton, eta_on)
    eta = s.eta if eta_on else 0.0
    n = at.nlocal
    a = args_of(s, at, flags, lst, eta, newton)
    loop, A_loop = pr.pair_loop(*a)
    gath, A_gath = pr.pair_gather(*a)
    sel = (flags & 1) != 0
    ntotal = at.nall if newton else n
    assert np.all(gath[~sel] == 0) and np.all(gath[ntotal:] == 0)
    rows = np.nonzero(sel[:ntotal])[0]
    assert np.abs(loop[rows] - gath[rows]).max() <= TOL * A_loop.max() and np.all(np.abs(A_loop[rows] - A_gath[rows]) <= TOL * A_loop[rows])
    if newton:
        assert np.any(gath[n:] != 0)                                # ghost rows carry partial sums that the fold adds
    direct, A_dir = pr.pair_direct(at.x[:n], at.q[:n], at.type[:n], flags[:n], s.boxlo, s.prd, s.periodic, s.cutsq_table(),
                                   pr.cut_coulsq_of(s.cutoff, s.g_ewald), s.g_ewald, eta)
    for name, (p, A) in dict(loop=(loop, A_loop), gather=(gath, A_gath)).items():
        pf, Af = pr.fold(p, at.owner, n), pr.fold(A, at.owner, n)
        if not newton:
            pf, Af = p[:n], A[:n]
        own = np.nonzero(sel[:n])[0]
        assert np.all(np.abs(pf[own] - direct[own]) <= TOL_DIRECT * A_dir[own]), name
        assert np.all(np.abs(Af[own] - A_dir[own]) <= TOL_DIRECT * A_dir[own]), name
    # the probe on an atom: its pair with that atom sits at the floor, r = 1e-5
    assert A_dir[probes[3]] > 0.5e5 * np.abs(at.q[:n]).min()
    if eta_on:                                                      # 0, 1 and 2 eta members occur among the listed pairs
        i, jraw = pr.pairs_of(lst)
        eb = (flags >> 1) & 1
        assert {0, 1, 2} == set(np.unique(eb[i] + eb[jraw & pr.NEIGHMASK]))


def test_special_bits_and_zero_charges_change_nothing():
    s, at, lst, flags, probes = small(True)
    a = args_of(s, at, flags, lst, s.eta, True)
    bare = dataclasses.replace(lst, neigh=(lst.neigh & pr.NEIGHMASK).astype(np.int32))
    assert np.any(lst.neigh != bare.neigh)
    for form in (pr.pair_loop, pr.pair_gather):
        p0, A0 = form(*a)
        p1, A1 = form(*args_of(s, at, flags, bare, s.eta, True))
        assert p0.tobytes() == p1.tobytes() and A0.tobytes() == A1.tobytes()
    # a probe's own row adds nothing to anybody else: with only the probes selected, every term is a charged partner's
    only = np.zeros(at.nlocal, np.int32)
    only[probes] = 1
    only = only[at.owner]
    p, A = pr.pair_gather(*args_of(s, at, only, lst, 0.0, True))
    lp, lA = pr.pair_loop(*args_of(s, at, only, lst, 0.0, True))
    rows = np.nonzero(only)[0]
    assert np.count_nonzero(A[:at.nlocal]) >= 4 and np.all(np.abs(p[rows] - lp[rows]) <= TOL * lA[rows])


def test_the_crafted_list_with_real_coordinates():
    """the gather form walks rows and segments of 0, 1, 63, 64, 65 and 129 entries, and a row that is empty while its segment is not"""
    s, at, _, flags, _ = small(True)
    nall = at.nall
    assert nall >= tr.N_OWN + tr.N_TARGET + 40
    lst = tr.crafted_list(nall, targets=tr.central_targets(at.x, at.nlocal))
    rows, segs = tr.segment_lengths(lst, nall)
    assert np.any((rows == 0) & (segs > 0))
    allsel = flags | 1
    a = args_of(s, at, allsel, lst, s.eta, True)
    loop, A = pr.pair_loop(*a)
    gath, A2 = pr.pair_gather(*a)
    assert np.all(np.abs(loop - gath) <= TOL * A) and np.all(np.abs(A - A2) <= TOL * A) and np.count_nonzero(A) > 300


def test_the_finish_formula():
    evs, V = 14.399645, 1000.0
    pi2vol = 2 * np.pi / V
    pair, u, q, z = np.array([2.0, -1.0]), np.array([0.5, 0.25]), np.array([0.3, -0.2]), np.array([4.0, -3.0])
    etabit, eta, Q, M = np.array([1, 0]), 1.979, 0.7, -1.3
    base = pair - u + np.array([eta * 0.3 * np.sqrt(2.0) / np.sqrt(np.pi), 0.0])
    slab = z * (2 * pi2vol * M)
    qs = pi2vol * Q * z * z
    for slabflag, qsumflag, want in ((0, 1, base), (1, 0, base + slab), (1, 1, base + slab - qs)):
        got = pr.finish(pair, u, q, z, etabit, eta, slabflag, qsumflag, V, Q, M, evs)
        assert np.abs(got.astype(float) - evs * want).max() <= 1e-14 * np.abs(evs * want).max()
    got = pr.finish(pair, u, q, z, etabit, 0.0, 0, 0, V, Q, M, evs)
    assert np.abs(got.astype(float) - evs * (pair - u)).max() <= 1e-15 * evs * 2
