"""-m gpu: the device-resident MD loop of INTEGRATION.md, executed as written -- the per-step sequence and, whenever the device's own
moved flag asks for it, the re-neighbouring sequence -- on the system, driver and composed reference of tests/md_loop_ref.py.

(a) the checked run: after every entry the arrays are downloaded and the entry is held to its own reference at the arrays it read, to
    the bounds of the entry's own test module (named at each check);
(b) the stream-ordered run (nothing synchronises but the re-neighbouring entries and one read of the moved flag per step) takes the
    decisions of the checked run and of a second stream-ordered run on a fresh handle and agrees with them to 16 times the reference's own float64 error -- not
    in bytes: the pair entry's forces are atomic sums (see the test);
(c) the device trajectory takes the decisions of the CPU reference trajectory and ends within its bound of it;
(d) a forced re-neighbouring at unchanged coordinates changes the force phase by rounding only;
(e) a restart from the downloaded state continues like the run that goes on (variants A and C), to the bound of (b);
(f) the lifetime rule of the fix's tables and the refusal of a coupled field before the first update, inside the loop.
tests/test_md_loop_ref_math.py asserts, without a GPU, that the reference trajectory has the properties these checks rely on."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from conp_amd import ConpError
import field_ref as fr
import exclude_ref as xref
import ghost_ref as gref
import integrate_ref as ir
import md_loop_ref as ml
import neigh_ref as nref
import post_neighbor_ref as pnr
import shake_ref as sr
from helpers import rel_err

pytestmark = pytest.mark.gpu

TOL_Q = 1e-8              # tests/test_gpu_parity.py, tests/test_gpu_post_neighbor_device.py: charges, relative to the largest entry
ORACLE = 1e-9             # tests/test_gpu_post_force_device.py: the whole step's folded force, relative to the largest entry


class Worst(dict):
    def note(self, key, fr_):
        self[key] = max(self.get(key, 0.0), float(fr_))

    def line(self, tag):
        print(f"{tag}: largest fraction of the bound: " + ", ".join(f"{k} {v:.3g}" for k, v in self.items()))
        assert max(self.values()) <= 1.0, (tag, dict(self))


@functools.lru_cache(maxsize=None)
def checked_run(variant):
    fx = ml.new_handle(variant)
    res = ml.run(fx, variant, checked=True)
    fx.close()
    return res


@functools.lru_cache(maxsize=None)
def stream_run(variant, which=0):
    fx = ml.new_handle(variant)
    res = ml.run(fx, variant, checked=False)
    fx.close()
    return res


def by_step(rec):
    out = {}
    for step, entry, a in rec:
        assert entry not in out.setdefault(step, {}), (step, entry)
        out[step][entry] = SimpleNamespace(**a)
    return out


# ---- (a): every entry against its reference at the arrays it read ------------------------------------------------------------------------
def check_neighbouring(c, E, before, tag):
    """the re-neighbouring sequence from the arrays `before` (x, image): wrap, ghost map, fill, list, step tables -> the numpy
    neighbouring of the device's own wrapped coordinates"""
    n = c.n
    boxlo, boxhi, periodic, _ = c.box
    xw, image = gref.wrap(before.x[:n], boxlo, boxhi, periodic, before.image)
    W, Fl, N = E["wrap"], E["fill"], E["neighbour"]
    assert W.x[:n].tobytes() == xw.tobytes() and np.array_equal(W.image, image), tag          # tests/test_gpu_ghosts.py: bit for bit
    nb = ml.neighbouring(c, xw)
    assert nb.ghost_margin >= 1e-9 and nref.cutoff_margin(nb.inp) >= 1e-9, tag
    assert N.nghost == nb.nghost and np.array_equal(N.owner, nb.owner) and np.array_equal(N.img, nb.img), tag
    assert Fl.nall == nb.nall and Fl.x.tobytes() == nb.x.tobytes(), tag
    assert Fl.q[n:].tobytes() == Fl.q[nb.owner].tobytes() and np.array_equal(Fl.tag, c.s.tag[nb.full]), tag
    # the list: tests/test_gpu_pair_build_list.py::_same_list
    got, ref = N.lst, nb.lst
    assert N.list_nall == nb.nall and got.inum == n and np.array_equal(got.ilist, np.arange(n)), tag
    assert np.array_equal(got.numneigh, ref.numneigh) and got.neigh.size == ref.neigh.size, tag
    assert np.array_equal(nref.sort_rows(n, got.numneigh, got.neigh), ref.neigh), tag
    assert np.any((ref.neigh.astype(np.int64) & 0xFFFFFFFF) >> 30), tag                        # special bits are in it
    if c.mirror is not None:                                                                   # the rule dropped pairs and left pairs
        m = c.mirror
        assert 0 < ref.neigh.size < nb.npairs_plain, tag
        assert all(np.array_equal(a, b[nb.full]) for a, b in zip(Fl.cls, (c.s.type, m.mask, m.molecule))), tag
        i, j = ml.pref.pairs_of(got)
        assert not np.any((m.mask[nb.full][i] | m.mask[nb.full][j & ml.pref.NEIGHMASK]) & ml.RECV), tag
    # the fix's tables: tests/test_gpu_post_neighbor_device.py::_against_reference
    t = N.tables
    sc = pnr.scatter_lists(c.a2e, nb.owner, c.ne)
    el = pnr.elyte_list(c.a2e, Fl.q[:n])
    rows = pnr.b_rows(got, np.concatenate([c.a2e, c.a2e[nb.owner]]), n, c.newton, c.ne)
    assert t["nall"] == nb.nall and t["ne"] == c.ne and t["nl"] == len(el) and t["n_ele_atoms"] == len(sc.ele_pairs), tag
    for k in ("ele_pairs", "csr_ptr", "csr_of", "csr_row"):
        assert np.array_equal(t[k], getattr(sc, k)), (tag, k)
    for k in ("b_rowptr", "b_ele", "b_oth"):
        assert np.array_equal(t[k], getattr(rows, k)), (tag, k)
    assert t["n_b_pairs"] == len(rows.b_ele) > 0 and t["zn_listed"] == 0 and np.array_equal(t["elyte_idx"], el), tag
    return nb, image


def check_forces(R, c, E, nb, q_before, out_gauss, out_field, w, tag):
    """the update and the force entries of one step: charges and scalar against the oracle, the folded sum against the sum of the
    entries' references with every term left out in turn, the field bit for bit"""
    n = c.n
    U = E["update"]
    ele = c.s.echeck[nb.full] != 0
    q_o, scalar_o, o = R.oracle(nb, U.x, q_before)
    scale = np.abs(q_o[ele]).max()
    assert scale > 0 and U.q[~ele].tobytes() == q_before[~ele].tobytes(), tag                  # only electrode atoms were written
    w.note("charges", np.abs(U.q[ele] - q_o[ele]).max() / (TOL_Q * scale))
    w.note("fix scalar", abs(U.scalar - scalar_o) / (TOL_Q * max(abs(scalar_o), scale)))
    terms = R.force_terms(nb, U.x, U.q, U.image, U.scalar, o)
    o.fx.close()
    got = E["fold"].f[:n]
    want = R.folded(nb, terms)
    w.note("folded force", rel_err(got, want) / ORACLE)
    open_gate = c.variant in ml.GATE_OPEN
    for name in terms:
        if name == "gaussian" and not open_gate:
            assert out_gauss[8] == 0 and not terms[name].any(), tag
            continue
        assert rel_err(got, R.folded(nb, terms, without=name)) > 1e3 * ORACLE, (tag, name)     # every term acted
    if open_gate:
        assert out_gauss[8] == R.gate(nb, U.x) >= 4, tag
    if c.newton:
        assert np.any(E["field"].f[n:] != 0.0) and E["fold"].f[n:].tobytes() == E["field"].f[n:].tobytes(), tag
    for a, b in (("update", "kspace"), ("kspace", "pair"), ("pair", "bonded"), ("bonded", "gaussian"), ("gaussian", "field"), ("field", "fold")):
        assert E[a].x.tobytes() == E[b].x.tobytes() and E[a].q.tobytes() == E[b].q.tobytes() and E[a].v.tobytes() == E[b].v.tobytes(), (tag, b)
    # the field: tests/test_gpu_efield.py::compare
    G, Fd = E["gaussian"], E["field"]
    D, L = R.field("f64", U.x, U.q, U.image, G.f, U.scalar), R.field("ld", U.x, U.q, U.image, G.f, U.scalar)
    assert Fd.f[:n].tobytes() == D.f.tobytes() and Fd.f[n:].tobytes() == G.f[n:].tobytes(), tag
    w.note("field energy", fr.frac(f"{tag}: field energy", out_field[0], L.out.v[0], fr.tol_of(n) * L.out.m[0]))
    w.note("field sum f", fr.frac(f"{tag}: field sum f", out_field[1:4], L.out.v[1:4], fr.tol_of(n) * L.out.m[1:4]))
    w.note("field virial", fr.frac(f"{tag}: field virial", out_field[4:10], L.out.v[4:10], fr.tol_of(n) * L.out.m[4:10]))
    assert out_field[10] == L.nsel == 64, tag


def check_shake(c, before, after, out, half, w, tag):
    """tests/test_gpu_shake.py::compare: flags 1 and 3 bit for bit, everything to TOL of the magnitudes, the counters equal"""
    n, sh = c.n, c.shake
    L, F = sr.Rule("ld", sh), sr.Rule("f64", sh)
    a, b = L.solve(before.x[:n], before.v, before.f[:n], half=half), F.solve(before.x[:n], before.v, before.f[:n], half=half)
    assert sr.clear_of_the_tolerance(L, sh.tolerance) > 1e-9, tag
    bw = np.zeros(n, dtype=bool)
    for row in sh.cluster:
        if row[0] != 2:
            bw[row[1:4]] = True
    f = after.f
    assert f[:n][bw].tobytes() == b.out[bw].tobytes(), tag
    w.note("shake f", sr.frac(f"{tag}: shake f", f[:n], a.out.v, sr.TOL * a.out.m))
    assert f[:n][~sh.member].tobytes() == before.f[:n][~sh.member].tobytes() and f[n:].tobytes() == before.f[n:].tobytes(), tag
    assert after.x.tobytes() == before.x.tobytes() and after.v.tobytes() == before.v.tobytes(), tag
    val, mag = L.d_out(a)
    w.note("shake virial", sr.frac(f"{tag}: shake virial", out[:6], val[:6], sr.tol_of(sh.ncluster) * mag[:6]))
    assert tuple(out[6:]) == tuple(float(v) for v in val[6:]) == tuple(F.d_out(b)[0][6:]), (tag, out[6:], val[6:])
    assert out[6] == 0 and out[7] == 0, tag


def check_integrator(c, B, I, S, Fi, out, w, tag):
    """tests/test_gpu_integrate.py: nve rows bit for bit the float64 restatement, nvt rows, d_out and the chain to TOL of the magnitudes"""
    n, g = c.n, c.integ
    tol = ir.tol_of(n)
    on = g.group >= 0
    L = ir.Rule("ld", g); L.set_state(B.state)
    xr, vr = L.initial(B.x[:n], B.v, B.f[:n], g.t_target)
    if g.style[0] == 0:
        F = ir.Rule("f64", g)
        x1, v1 = F.initial(B.x[:n], B.v, B.f[:n], g.t_target)
        assert I.x[:n].tobytes() == x1.tobytes() and I.v.tobytes() == v1.tobytes(), tag
    w.note("initial x", ir.frac(f"{tag}: initial x", I.x[:n], xr.v, tol * xr.m))
    w.note("initial v", ir.frac(f"{tag}: initial v", I.v, vr.v, tol * vr.m))
    assert I.x[:n][~on].tobytes() == B.x[:n][~on].tobytes() and I.v[~on].tobytes() == B.v[~on].tobytes() and I.x[n:].tobytes() == B.x[n:].tobytes(), tag
    val, mag = L.get_state()
    w.note("chain", ir.frac(f"{tag}: chain after initial", I.state, val, tol * mag))
    L = ir.Rule("ld", g); L.set_state(I.state)
    vr, rows = L.final(S.v, S.f[:n])
    if g.style[0] == 0:
        v1, _ = ir.Rule("f64", g).final(S.v, S.f[:n])
        assert Fi.v.tobytes() == v1.tobytes(), tag
    w.note("final v", ir.frac(f"{tag}: final v", Fi.v, vr.v, tol * vr.m))
    val, mag = ir.out_arrays(rows)
    w.note("integrate d_out", ir.frac(f"{tag}: integrate d_out", out.reshape(1, 4), val, tol * mag))
    val, mag = L.get_state()
    w.note("chain", ir.frac(f"{tag}: chain after final", Fi.state, val, tol * mag))
    assert Fi.v[~on].tobytes() == S.v[~on].tobytes() and Fi.x.tobytes() == S.x.tobytes() and Fi.f.tobytes() == S.f.tobytes(), tag


@pytest.mark.parametrize("variant", sorted(ml.VARIANTS))
def test_every_entry_of_the_checked_run(variant):
    c = ml.system(variant)
    R = ml.Ref(variant)
    res = checked_run(variant)
    steps = by_step(res.rec)
    n = c.n
    w = Worst()
    # the start: correct -> re-neighbouring -> forces -> shake setup
    E = steps[-1]
    x0 = sr.Rule("f64", c.shake).solve(c.s.x, None, None, correct=True).out
    bw = np.zeros(n, dtype=bool)
    for row in c.shake.cluster:
        if row[0] != 2:
            bw[row[1:4]] = True
    xl = sr.Rule("ld", c.shake).solve(c.s.x, None, None, correct=True).out
    assert E["correct"].x[bw].tobytes() == x0[bw].tobytes() and E["correct"].x[~c.shake.member].tobytes() == c.s.x[~c.shake.member].tobytes()
    w.note("correct", sr.frac("correct: x", E["correct"].x, xl.v, sr.TOL * xl.m))
    nb, image = check_neighbouring(c, E, E["correct"], "start")
    check_forces(R, c, E, nb, E["fill"].q, res.gauss[0], res.field[0], w, "start")
    check_shake(c, E["fold"], E["shake"], res.shake[0], True, w, "start")
    builds = [-1]
    for k in range(ml.STEPS):
        E, tag = steps[k], f"step {k}"
        B, I = E["begin"], E["initial"]
        P = I                                                                                  # the arrays behind the post-integrate entries
        assert res.check[k + 1][0] < 0.1 * c.shake.tolerance and res.check[k + 1][1] < 0.1 * c.shake.tolerance, (tag, res.check[k + 1])
        if c.mirror is not None:                                                               # tests/test_gpu_zmirror.py: bit for bit
            M, m = E["mirror"], c.mirror
            assert M.x[:n].tobytes() == xref.mirror_apply(I.x[:n], m.src, m.dst, m.zoffset).tobytes() and M.x[n:].tobytes() == I.x[n:].tobytes(), tag
            assert M.x[m.dst, 0].tobytes() == M.x[m.src, 0].tobytes() and np.array_equal(M.x[m.dst, 2], m.zoffset - M.x[m.src, 2]), tag
            assert all(getattr(M, k).tobytes() == getattr(I, k).tobytes() for k in ("v", "q", "f", "image")), tag
            P = M
        flag, disp = ml.moved(c, nb, P.x)
        assert abs(disp - c.trigger) >= 1e-6 and res.flags[k] == flag, (tag, disp, res.flags[k])
        if flag:
            nb, image = check_neighbouring(c, E, P, tag)
            builds.append(k)
        else:
            Fl = E["fill"]
            x_all, q_all = ml.fill(c, nb, P.x[:n], P.q[:n])
            assert Fl.x.tobytes() == x_all.tobytes() and Fl.q.tobytes() == q_all.tobytes() and np.array_equal(Fl.image, P.image), tag
        assert res.nghost[k] == nb.nghost, tag
        check_forces(R, c, E, nb, E["fill"].q, res.gauss[k + 1], res.field[k + 1], w, tag)
        check_shake(c, E["fold"], E["shake"], res.shake[k + 1], False, w, tag)
        check_integrator(c, B, I, E["shake"], E["final"], res.integ[k + 1], w, tag)
    assert res.builds == builds and len(builds) >= 3
    w.line(f"variant {variant}, the checked run")


# ---- (c): the reference trajectory --------------------------------------------------------------------------------------------------------
def accumulated_bound(c, ref):
    """what the per-step bounds of (a) allow after the run: every step's force may be off by ORACLE of its largest entry, and by what
    charges off by TOL_Q make of a force that is bilinear in them (2 TOL_Q of the largest entry); two half kicks of dtf / m per step
    carry that into v, and dt v into x -> (bound on x, bound on v)"""
    g = c.integ
    dtfm = 0.5 * g.dt * g.ftm2v / g.mass[c.s.type[g.group >= 0] - 1].min()
    dv = dx = 0.0
    for fmax in ref.fmax:
        dv += 2.0 * dtfm * (ORACLE + 2.0 * TOL_Q) * fmax
        dx += g.dt * dv
    return dx, dv


@pytest.mark.parametrize("variant", sorted(ml.VARIANTS))
def test_the_device_trajectory_follows_the_reference_trajectory(variant):
    c = ml.system(variant)
    dev = stream_run(variant, 0)
    ref, ld = ml.reference_trajectory(variant), ml.reference_trajectory(variant, kind="ld")
    assert dev.flags == ref.flags == ld.flags and dev.nghost == ref.nghost == ld.nghost
    assert dev.builds == [b.step for b in ref.builds]
    assert np.array_equal(dev.image, ref.image) and np.array_equal(ref.image, ld.image) and ref.image.any()
    chk = by_step(checked_run(variant).rec)
    for b in ref.builds:
        assert np.array_equal(chk[b.step]["wrap"].image, b.image), b.step                      # every wrapped atom's counter, at every build
    fx_, fv_ = accumulated_bound(c, ref)
    for name, floor in (("x", fx_), ("v", fv_)):
        own = np.abs(getattr(ref, name) - getattr(ld, name).astype(np.float64)).max()
        bound = max(16.0 * own, floor)
        err = np.abs(getattr(dev, name) - getattr(ref, name)).max()
        print(f"variant {variant}: final {name}: device against the reference {err:.3e}, the reference against longdouble {own:.3e} "
              f"({err / (16.0 * own):.3g} of 16 times that), accumulated per-step bound {floor:.3e}: fraction of the bound {err / bound:.3g}")
        assert err <= bound, (variant, name)


# ---- (b): the stream-ordered run ----------------------------------------------------------------------------------------------------------
def within_the_rounding_of_the_trajectory(variant, a, b, tag):
    """x and v of two DEVICE results: both sides are the same code on the same inputs and differ only by the order in which the pair
    entry's atomic adds arrive, so the accumulated per-step bound of (c) has no place here: 16 times what the float64 reference
    trajectory differs from its longdouble twin -> the fractions"""
    ref, ld = ml.reference_trajectory(variant), ml.reference_trajectory(variant, kind="ld")
    fr_ = {}
    for name in ("x", "v"):
        own = np.abs(getattr(ref, name) - getattr(ld, name).astype(np.float64)).max()
        fr_[name] = float(np.abs(getattr(a, name) - getattr(b, name)).max() / (16.0 * own))
    if ml.system(variant).integ.style[0]:                                                       # the chain of an nvt group, likewise
        own = np.abs(ref.state - np.asarray(ld.state, dtype=np.float64))
        fr_["chain"] = float((np.abs(a.state - b.state)[own > 0] / (16.0 * own[own > 0])).max())
        assert np.array_equal(a.state[own == 0], b.state[own == 0])
    print(f"variant {variant}: {tag}: fraction of 16 times the reference's own float64 error: " + ", ".join(f"{k} {v:.3g}" for k, v in fr_.items()))
    assert max(fr_.values()) <= 1.0, (variant, tag, fr_)
    return fr_


def no_atomic_outputs_equal(variant, a, b, tag):
    """what no float atomic has reached is equal byte for byte: every per-step output of the run's start before the pair forces act
    (the update's self energy, the pair entry's energies and virial -- DESIGN.md section 16: a fixed order --, the field's sums), and
    the counters of every step"""
    rows = ml.STEPS + 1
    assert a.pair[0].tobytes() == b.pair[0].tobytes() and a.field[0].tobytes() == b.field[0].tobytes(), tag
    if variant not in ml.GATE_OPEN:
        assert a.gauss[0].tobytes() == b.gauss[0].tobytes(), tag
    assert np.array_equal(a.shake[:rows, 6:], b.shake[:rows, 6:]) and np.array_equal(a.gauss[:rows, 8], b.gauss[:rows, 8]), tag
    assert np.array_equal(a.field[:rows, 10], b.field[:rows, 10]) and np.array_equal(a.image, b.image), tag


@pytest.mark.parametrize("variant", [v for v in sorted(ml.VARIANTS) if not ml.VARIANTS[v].get("pppm")])      # (D: covered by (a) and (c))
def test_the_stream_ordered_run_is_the_checked_run(variant):
    """Byte identity of x, v, q and f cannot be asked of any variant: the pair entry adds its forces with float atomics (DESIGN.md
    section 16: "forces ... are atomic sums and reproduce to rounding"), and on an MI355X two CHECKED runs on fresh handles already
    differ in their last bits from step 0 on (measured: the first differing per-step output is conp_integrate_final_device's d_out of
    step 0).  So every variant is compared the way the atomics of the Gaussian correction and of the mesh spread demand: what no
    atomic reaches -- the decisions, the ghost counts, the image counters, the SHAKE counters, the outputs of the run's start -- is
    equal byte for byte, and x and v agree to 16 times the float64 reference trajectory's own distance from its longdouble twin, between the stream-ordered and the checked run and between two stream-ordered runs on fresh handles"""
    a, b, chk = stream_run(variant, 0), stream_run(variant, 1), checked_run(variant)
    rows = ml.STEPS + 1
    for r in (a, b, chk):
        assert not np.isnan(r.gauss[:rows]).any() and not np.isnan(r.integ[1:rows]).any() and not np.isnan(r.field[:rows]).any()
        if variant not in ml.GATE_OPEN:
            assert not r.gauss[:rows, 8].any()                                                  # no pair inside the gate
    assert sum(a.flags) >= 2 and len(set(a.nghost)) >= 2
    for r, tag in ((chk, "stream-ordered against checked"), (b, "two stream-ordered runs")):
        assert a.flags == r.flags and a.nghost == r.nghost and a.builds == r.builds, (tag, ml.first_difference(a, r))
        no_atomic_outputs_equal(variant, a, r, tag)
        within_the_rounding_of_the_trajectory(variant, a, r, tag)
        scale = np.abs(r.q).max()
        assert np.abs(a.q - r.q).max() <= 2.0 * TOL_Q * scale, tag                             # each is within TOL_Q of the oracle (a)


# ---- (e): restart -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["A", "C"])
def test_a_restart_continues_the_run(variant):
    """after K steps x, v, q, the image counters and the chains go to the host; a fresh handle gets the host setup at those
    coordinates, conp_integrate_set_state and the start of a run (re-neighbouring, forces, SHAKE setup), and runs K more steps.  The
    original handle makes the same start from its own arrays (the forced re-neighbouring at step K) and runs on.  Both ends agree in
    every decision and counter and to the bound of (b) in x and v (not in bytes: the pair forces are atomic sums, see (b))"""
    K = 8
    c = ml.system(variant)
    fx = ml.new_handle(variant)
    L = ml.Loop(fx, variant, 2 * K, False)
    L.start()
    for k in range(K):
        L.step(k)
    mid = L.result()
    L.resume()
    for k in range(K, 2 * K):
        L.step(k)
    end = L.result()
    fx.close()
    # (the host setup sees the run's starting charges: the library takes its k-space cutoff from the sum of q^2 of the setup's atoms, as
    #  LAMMPS' Ewald::init does, and the electrode charges of variant C -- up to 2.9 e -- would move it from 414 to 629 k vectors)
    fx2 = ml.new_handle(variant, mid.x)
    assert fx2.info().kcount == ml.ktables(variant)["kv"].shape[0]
    fx2.integrate_set_state(mid.state)
    L2 = ml.Loop(fx2, variant, 2 * K, False)
    L2.upload(mid.x, mid.v, mid.q, mid.image)
    L2.resume()
    for k in range(K, 2 * K):
        L2.step(k)
    end2 = L2.result()
    fx2.close()
    assert sum(end2.flags) >= 1 and np.abs(end.x - mid.x).max() > 0.1
    assert end.flags[K:] == end2.flags and end.nghost[K:] == end2.nghost and np.array_equal(end.image, end2.image)
    within_the_rounding_of_the_trajectory(variant, end, end2, f"restart after {K} steps")
    if c.integ.style[0]:
        assert end.state[0, 3] != 0.0 and end2.state[0, 3] != 0.0                             # the chain was handed over and acts


# ---- (d): a re-neighbouring changes nothing but orders ------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["A", "B"])
def test_a_forced_reneighbouring_changes_nothing_but_orders(variant):
    """after three steps without a re-neighbouring (the atoms have moved 0.5 A since the build) the force phase runs twice at the same
    coordinates: on the old neighbouring, and behind a forced full re-neighbouring sequence -- another ghost map, another list order,
    other tables; bonded and SHAKE lists are not passed again.  (The run is a stream-ordered one, not the checked run's state; the first
    force phase leaves its electrode charges in d_q and the second update starts from them, which the inverse solve does not read.)  Both folded forces satisfy (a), so they agree within 2 ORACLE of the
    largest entry, the charges within 2 TOL_Q of the largest"""
    c = ml.system(variant)
    n, K = c.n, 3
    fx = ml.new_handle(variant)
    L = ml.Loop(fx, variant, K, False)
    L.start()
    for k in range(K):
        L.step(k)
    assert L.flags == [0] * K
    old_list, _ = fx.pair_get_list()
    ghosts_a, tab_a = fx.ghost_get(), fx.step_tables()
    L.force_phase(K + 1)
    a = L.result()
    L.reneighbour()
    L.force_phase(K + 1)
    b = L.result()
    new_list, _ = fx.pair_get_list()
    ghosts_b, tab_b = fx.ghost_get(), fx.step_tables()
    fx.close()
    assert not np.array_equal(old_list.numneigh[:n], new_list.numneigh[:n])                    # another list
    assert not np.array_equal(ghosts_a[2], ghosts_b[2]) and any(tab_a[k].tobytes() != tab_b[k].tobytes() for k in ("b_ele", "b_oth"))
    fr_f = rel_err(b.f, a.f) / (2.0 * ORACLE)
    fr_q = np.abs(b.q - a.q).max() / (2.0 * TOL_Q * np.abs(a.q).max())
    print(f"variant {variant}: a forced re-neighbouring: fraction of the bound: force {fr_f:.3g}, charges {fr_q:.3g}")
    assert fr_f <= 1.0 and fr_q <= 1.0 and np.abs(a.f).max() > 1.0


# ---- (f): preconditions inside the loop -------------------------------------------------------------------------------------------------
def _steps(L, first, last):
    for k in range(first, last):
        L.step(k)
    return L.result()


def test_a_list_build_without_the_fix_entry_runs_on_the_previous_tables():
    """DESIGN.md section 19, the lifetime rule: after three steps the re-neighbouring sequence is issued WITHOUT its last call, on
    copies of the arrays -- the pair style has a new list and the handle a new ghost map, the fix has not.  The update and the
    Gaussian correction on the arrays of the previous neighbouring give the bytes they gave before (neither meets an atomic with a
    closed gate), and the step tables are unchanged.  (Not a whole step, as the issue words it: the pair entry would walk a list of the
    new nall over arrays of the old one; the two entries issued are the ones that read the fix's own copies.)  Then the sequence is issued in full and the run goes on like a run that was
    re-neighboured there without the detour"""
    import torch
    variant, K = "B", 3
    c = ml.system(variant)
    runs = []
    for detour in (False, True):
        fx = ml.new_handle(variant)
        L = ml.Loop(fx, variant, ml.STEPS, False)
        L.start()
        _steps(L, 0, K)
        if detour:
            def update():
                q, out = L.d_q.clone(), torch.full((9,), float("nan"), dtype=torch.float64, device="cuda")
                fx.pre_force_device(L.d_x.data_ptr(), q.data_ptr(), c.potdiff)
                fx.post_force_device(L.d_x.data_ptr(), q.data_ptr(), 0, out.data_ptr())
                torch.cuda.synchronize()
                return q.cpu().numpy(), out.cpu().numpy(), fx.compute_scalar()
            before, tables = update(), fx.step_tables()
            keep = (L.d_x, L.d_q, L.d_f, L.d_tag, L.d_cls, L.d_image, L.nall)
            L.d_x, L.d_q, L.d_image = L.d_x.clone(), L.d_q.clone(), L.d_image.clone()
            L.reneighbour(post_neighbor=False)
            new_nall = L.nall
            L.d_x, L.d_q, L.d_f, L.d_tag, L.d_cls, L.d_image, L.nall = keep
            after, tables2 = update(), fx.step_tables()
            assert fx.pair_get_list()[1] == new_nall and tables2["nall"] == tables["nall"] == L.nall
            assert all(np.asarray(tables[k]).tobytes() == np.asarray(tables2[k]).tobytes() for k in tables)
            assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes() and before[2] == after[2]
        L.reneighbour()
        runs.append(_steps(L, K, ml.STEPS))
        fx.close()
    a, b = runs
    assert a.flags == b.flags and a.nghost == b.nghost and np.array_equal(a.image, b.image) and sum(a.flags) >= 1
    within_the_rounding_of_the_trajectory(variant, a, b, "behind a list build without the fix entry")


def test_a_coupled_field_before_the_first_update_is_refused_and_changes_nothing():
    """a fresh conq handle with its field parameters set and no update yet: the coupled call is out of order (CONP_ERR_STATE); the
    handle is then set up and runs the loop like a handle that was never asked"""
    import torch
    variant = "B"
    c = ml.system(variant)
    seen = []

    def ask(fx):
        fx.efield_set_params(c.sel, ml.systems.QE2F, c.prd)
        d_x = torch.from_numpy(np.ascontiguousarray(c.s.x)).cuda()
        d_q, d_f = torch.from_numpy(c.s.q.copy()).cuda(), torch.full((c.n, 3), 2.5, dtype=torch.float64, device="cuda")
        with pytest.raises(ConpError) as e:
            fx.efield_post_force_device(d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), c.e, couple=1, couple_scale=c.couple_scale)
        torch.cuda.synchronize()
        assert e.value.code == -2 and np.all(d_f.cpu().numpy() == 2.5)
        seen.append(e.value.code)
    fx = ml.new_handle(variant, before_setup=ask)
    got = ml.run(fx, variant)
    fx.close()
    ref = stream_run(variant, 0)
    assert seen == [-2] and got.flags == ref.flags and got.nghost == ref.nghost
    no_atomic_outputs_equal(variant, got, ref, "behind a refused coupled call")
    within_the_rounding_of_the_trajectory(variant, got, ref, "behind a refused coupled call")
