"""-m gpu: the CG solver (`fix conp ... cg`: cg() in conp_fix.cpp, cg_step_kernel / cg_row_dot / cg_update_kernel in conp_kernels.hip
section 8) at every size tier, batch schedule and launch form, with a matrix and b vectors the test chose (tests/cg_ref.py makes them;
tests/test_cg_ref_math.py checks the helpers without a GPU).

A handle is made with extra_args = ["cg", ...] and goes through its normal setup; conp_fix_set_matrix then replaces A by
cg_ref.spd_matrix (exactly symmetric, every off-diagonal 128 x 128 tile with a magnitude and sign of its own over 3.5 decades, every
Gershgorin disc above a known g) with the runstage the handle has, and the test binds its own b and q vectors (Ne + 512 long, NaN
behind the first Ne entries).  conp_fix_solve_device runs cg() on the bound b.  The tolerance and maxiter of a handle are fixed when
it is created, and so is its launch form (CONP_PATH_CG_TWO_LAUNCH): a (size, keywords, form) is one handle, kept for the module.

Sizes and what each reaches (cg_ref.check_sizes asserts it from the restated loop bounds):
    62 lanes 62, 63 of cg_row_dot hold nothing     130 small general case     449 lane 0 alone in the 8-wide tier
    961 lane 0 alone in the 16-wide tier     1025 first tier boundary plus one     1664 the deck's size     2049 two boundaries plus one
    4096 last size whose update stays in registers, 512 full workgroups of 8 rows
    4097 first size that re-reads p, Ap, res; 16 rows per workgroup, one live row in the last
    6151 16 rows per workgroup, 7 live rows in the last     8200 65.6 KB of dynamic LDS, above the 64 KB a kernel gets unasked
Ne = 16384 and 16385 (the cg_step_fits edge, 128 KB) are out of scope: each is a 2.1 GB matrix.  The two-launch form they would fall
back to is reached through CONP_PATH_CG_TWO_LAUNCH at every size above.  Not covered either: more than one rank.

Bounds.  None comes from what the GPU gives.
  (a), (e)  a solve cut off after k iterations, entry-wise against cg_ref (float128) after the same k: 16 x e64, at least
            16 x 2^-53 max|q|, where e64 = max |cg_f64 - cg_ref| is measured on the CPU for the same matrix, vector and k (float64
            with numpy's pairwise sums -- another summation order than the kernels' 64-lane strided fma chains and wave / block trees).
            A column of the smallest tile left out is at least 1000 bounds away (test_cg_ref_math).
  (b)       converged solves: ||q - q*||_2 <= 2 sqrt(n tol) / g (cg_ref.converged_bound has the derivation), q* = cg_ref run to
            lr / n < 1e-26; |sum q| <= 4 k n 2^-53 max|q| (cg_ref.sum_bound); iterations within 1 of cg_ref's; every logged residual
            equal to cg_ref's in the digits %g prints (cg_ref is still descending at 1e-26, so every logged value is more than 1e6
            times its floor).
  (c), (d)  bytes against bytes.

Measured (CPU: e64 in units of 2^-53 max|q|, dense vector, k = 1, 2, 5, 8, 9; iterations of the dense vector at tol 1e-6 / 1e-20.
GPU, MI355X: worst fraction of the (a) bound over both vectors and k = 1, 2, 5; of the (b) bound at tol 1e-6 / 1e-20):
      Ne   e64 at k = 1     2     5     8     9   iterations   (a)     (b) 1e-6  1e-20
      62           2.06  2.44  3.22  3.43  3.62     9 / 24    0.271     0.085  0.076
     130           2.96  3.75  2.72  3.16  3.46     9 / 25    0.128     0.077  0.118
     449           0.76  5.32  2.56  3.39  3.90     9 / 26    0.068     0.124  0.085
     961           1.21  4.60  3.56  3.95  4.03     9 / 26    0.243     0.102  0.079
    1025           0.98  7.58  4.03  4.24  4.16     9 / 26    0.230     0.101  0.075
    1664           2.27  7.18  4.23  4.82  5.03     9 / 26    0.231     0.103  0.081
    2049           2.36  7.23  5.28  5.64  5.56     9 / 26    0.094     0.110  0.089
    4096           0.92  7.42  3.80  4.46  4.80     9 / 26    0.356     0.109  0.085
    4097           0.74  5.44  4.38  4.74  5.08     9 / 26    0.084     0.111  0.086
    6151           0.78  6.50  4.00  3.54  3.55     9 / 26    0.189     0.100  0.080
    8200           1.07  6.60  3.63  4.09  4.10     9 / 26    0.132     0.108  0.085
The GPU's iteration counts are cg_ref's at every size; |sum q| stays below 0.003 of its bound; max|q| is 2 to 4.5 for the dense vector.
The (b) fractions are those of cg_f64 on the CPU to the digits shown: what is left at the stop is the iteration's own error.
Setting up the Ne = 8200 case (system, lists, matrix, float128 references) takes about 4 s on a 16-core host (10 s on an 8-core one), once per module; a handle's setup at that size takes less than 0.1 s."""
import dataclasses
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import cg_ref as cr
import solve_ref as sr
from conp_amd import FixConp, capi, neighbor

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DV = 1.7                      # not the potential difference of the setup
NEVER = ("cg", "tol", "1e-300")
DEFAULT = ("cg",)
TIGHT = ("cg", "tol", "1e-20", "maxiter", "60")
THREE = ("cg", "maxiter", "3")
SCHED = ("cg", "tol", "1e-20", "maxiter", "32")


def _maxiter(extra):
    return int(extra[extra.index("maxiter") + 1]) if "maxiter" in extra else 100


def _tol(extra):
    return float(extra[extra.index("tol") + 1]) if "tol" in extra else cr.TOL_DEFAULT


class Case:
    """one electrode count: the system, its lists, the matrix, the b vectors, the float128 and float64 CPU solves -- made once"""

    def __init__(self, ne, references=True):
        t0 = time.time()
        self.ne = ne
        self.s = sr.system(ne)
        self.at, self.alist, self.blist = neighbor.build_lists(self.s)
        self.A, self.g = cr.spd_matrix(ne, cr.seed_matrix(ne))
        self.b = cr.vectors(self.A, cr.seed_vectors(ne))
        self.ele_atoms = np.nonzero(self.at.echeck != 0)[0]              # owned and ghost copies of electrode atoms
        assert np.count_nonzero(self.ele_atoms >= self.at.nlocal) > 0
        self.handles = {}
        self.ele_row = None                                              # eleall index of each of ele_atoms (from the first handle)
        if not references:                                               # (the guard-zone child compares the GPU with itself)
            return
        nd, nt = cr.ITERS[ne]
        ks = (1, 2, 5, nd - 1, nd)
        self.ref = {"dense": cr.cg_ref(self.A, self.b["dense"], cr.TOL_REF, 61, keep=ks),
                    "unit_last": cr.cg_ref(self.A, self.b["unit_last"], 0.0, 6, keep=(1, 2, 5))}
        f64 = {"dense": cr.cg_f64(self.A, self.b["dense"], 0.0, nd + 1, keep=ks),
               "unit_last": cr.cg_f64(self.A, self.b["unit_last"], 0.0, 6, keep=(1, 2, 5))}
        self.e64 = {(name, k): float(np.max(np.abs(f64[name].snaps[k] - self.ref[name].snaps[k])))
                    for name in f64 for k in f64[name].snaps if k}
        hist = self.ref["dense"].hist
        assert self.ref["dense"].converged and (cr.needed(hist, ne, cr.TOL_DEFAULT), cr.needed(hist, ne, cr.TOL_TIGHT)) == (nd, nt)
        self.seconds = time.time() - t0
        print(f"  Ne={ne}: case made in {self.seconds:.1f} s; e64 / (2^-53 max|q|), dense: " +
              ", ".join(f"k={k}: {self.e64[('dense', k)] / (cr.U * float(np.max(np.abs(self.ref['dense'].snaps[k])))):.2f}" for k in ks))

    def atoms(self):
        return dataclasses.replace(self.at, q=self.at.q.copy())

    def bound(self, name, k):
        return cr.error_bound(self.e64[(name, k)], float(np.max(np.abs(self.ref[name].snaps[k]))))


Record = dataclasses.make_dataclass("Record", ["q", "iterations", "lines", "res", "schedule"])


class Handle:
    def __init__(self, case, fx, at, extra, two_launch):
        import torch
        self.case, self.fx, self.at, self.ne, self.extra, self.two_launch = case, fx, at, case.ne, extra, two_launch
        self.maxiter, self.tol = _maxiter(extra), _tol(extra)
        assert fx.info().elenum_all == case.ne and fx.args.maxiter == self.maxiter and fx.args.tolerance == self.tol
        if case.ele_row is None:
            case.ele_row = fx.maps()["tag2eleall"][case.at.tag[case.ele_atoms]].astype(np.int64)
            assert case.ele_row.min() == 0 and case.ele_row.max() == case.ne - 1
        # what cg() will take as the length of its next first batch: the iteration count of the last solve that converged
        conv = re.findall(r"\*\*\*\*\* Converged at iteration (\d+)\.", fx.log_drain())
        self.prev = int(conv[-1]) if conv else 8
        self.big_b = torch.full((case.ne + 512,), float("nan"), dtype=torch.float64, device="cuda")
        self.big_q = torch.full((case.ne + 512,), float("nan"), dtype=torch.float64, device="cuda")
        fx.bind_device_buffers(self.big_b.data_ptr(), self.big_q.data_ptr())
        self.d_x = torch.from_numpy(np.ascontiguousarray(at.x)).cuda()
        self.d_q = torch.zeros(at.nall, dtype=torch.float64, device="cuda")

    def inject(self, b):
        import torch
        self.big_b[:self.ne] = torch.from_numpy(np.ascontiguousarray(b)).cuda()
        torch.cuda.synchronize()

    def q(self):
        import torch
        torch.cuda.synchronize()
        return self.big_q[:self.ne].cpu().numpy().copy()

    def tails_are_nan(self):
        import torch
        torch.cuda.synchronize()
        return bool(torch.isnan(self.big_b[self.ne:]).all() and torch.isnan(self.big_q[self.ne:]).all())

    def record(self):
        """what the last cg() left: charges, iteration count, log lines, and the launches it must have issued (cg_ref.batch_schedule)"""
        it = self.fx.info().cg_iterations
        lines = [l for l in self.fx.log_drain().splitlines() if l.startswith(("Iteration", "*****"))]
        res = []
        for k, l in enumerate(lines, start=1):
            m = re.fullmatch(r"(?:Iteration (\d+):|\*\*\*\*\* Converged at iteration (\d+)\.) res = (\S+)(?: netcharge = \S+)?", l)
            assert m and int(m.group(1) or m.group(2)) == k, l
            assert (m.group(2) is not None) == (it > 0 and k == len(lines)), l          # the converged line is the last one, if any
            res.append(m.group(3))
        sched = cr.batch_schedule(self.prev, it if it > 0 else None, self.maxiter)
        assert len(lines) == sched.iterations, (len(lines), sched)
        self.prev = sched.next_prev
        return Record(self.q(), it, lines, res, sched)

    def solve(self, b):
        """conp_fix_solve_device on an injected b"""
        self.inject(b)
        self.fx.solve_device(DV)
        return self.record()

    def random_charges(self, seed, everywhere):
        """the caller's atom charges before a write: arbitrary bit patterns in every entry, or (where the update forms b from the
        electrolyte's charges first) in every copy of an electrode atom"""
        import torch
        before = self.at.q.copy()
        rnd = np.random.default_rng(seed).integers(-2 ** 63, 2 ** 63 - 1, size=self.at.nall, dtype=np.int64).view(np.float64)
        if everywhere:
            before = rnd
        else:
            before[self.case.ele_atoms] = rnd[self.case.ele_atoms]
        self.d_q.copy_(torch.from_numpy(before.view(np.int64).copy()).cuda().view(torch.float64))
        torch.cuda.synchronize()
        return before

    def want_charges(self, before, dV):
        """every copy of electrode atom e holds q[e] + dV setq[e] (vectors(): what the solve and the setup left), the rest its bits"""
        _b, q, setq = self.fx.vectors()
        assert np.isfinite(q).all() and np.isfinite(setq).all() and np.abs(setq).max() > 0
        out = before.copy()
        out[self.case.ele_atoms] = sr.charges(q, dV, setq)[self.case.ele_row]
        return out

    def atom_charges(self):
        import torch
        torch.cuda.synchronize()
        return self.d_q.cpu().numpy()


def _handle(case, extra, two_launch=False, tag=None):
    key = (tuple(extra), two_launch, tag)
    if key in case.handles:
        return case.handles[key]
    s, at = case.s, case.atoms()
    t0 = time.time()
    with capi.test_paths(capi.PATH_CG_TWO_LAUNCH if two_launch else 0):
        fx = FixConp(s, extra_args=list(extra))
        fx.init_lists(case.alist, case.blist)
        fx.setup_post_neighbor(at)
        fx.setup_pre_force(at, 0, s.potdiff)
    assert fx.row_range() == (0, case.ne)
    fx.set_matrix(case.A, fx.info().runstage)
    h = Handle(case, fx, at, tuple(extra), two_launch)
    if case.ne == 8200:
        print(f"  Ne=8200 handle {' '.join(extra)}{' (two launches)' if two_launch else ''}: {time.time() - t0:.1f} s")
    case.handles[key] = h
    return h


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(ne):
        if ne not in made:
            made[ne] = Case(ne)
        return made[ne]
    yield get
    for c in made.values():
        for h in c.handles.values():
            h.fx.close()


def _frac(q, ref_q, bound):
    return float(np.max(np.abs(np.asarray(q, cr.LD) - ref_q))) / bound


def _assert_cut_off(tag, case, rec, name, k, converged=False):
    """a solve that ran k iterations against cg_ref after the same k: entry-wise bound, log lines"""
    ref = case.ref[name]
    frac = _frac(rec.q, ref.snaps[k], case.bound(name, k))
    print(f"  {tag}: k = {k}, e64 = {case.e64[(name, k)]:.3e}, worst |q - ref| / bound = {frac:.3f}")
    assert rec.iterations == (k if converged else 0) and len(rec.lines) == k, (tag, rec.iterations, rec.lines)
    assert rec.res == ["%g" % float(x) for x in ref.hist[1:k + 1]], (tag, rec.res)
    assert np.isfinite(rec.q).all() and frac <= 1.0, (tag, frac)
    return frac


def test_sizes_reach_what_they_are_for():
    """the properties of the sizes the other tests rely on: a change of a kernel constant shows here, not as a hollow pass there"""
    cr.check_sizes()
    assert capi.PATH_CG_TWO_LAUNCH == 8


@pytest.mark.parametrize("ne", cr.SIZES)
def test_fixed_iteration_counts_entry_wise(cases, ne):
    """(a) a tolerance that never triggers, maxiter 2, 3 and 6: after 1, 2 and 5 iterations nothing has converged, so an error of the
    first products cannot be absorbed by later iterations"""
    case = cases(ne)
    worst = 0.0
    for maxiter in (2, 3, 6):
        h = _handle(case, NEVER + ("maxiter", str(maxiter)))
        for name in ("dense", "unit_last"):
            rec = h.solve(case.b[name])
            worst = max(worst, _assert_cut_off(f"Ne={ne} maxiter {maxiter} b={name}", case, rec, name, maxiter - 1))
            assert not rec.schedule.two_launch and sum(len(b) for b in rec.schedule.batches) == maxiter
        assert h.tails_are_nan()
    print(f"  Ne={ne}: (a) worst fraction {worst:.3f}")


@pytest.mark.parametrize("ne", cr.SIZES)
def test_converged_solves_within_the_derived_bound(cases, ne):
    """(b) tol 1e-20 (more than 20 iterations) and the default 1e-6"""
    case = cases(ne)
    ref = case.ref["dense"]
    for extra in (DEFAULT, TIGHT):
        h = _handle(case, extra)
        rec = h.solve(case.b["dense"])
        want = cr.needed(ref.hist, ne, h.tol)
        bound = cr.converged_bound(ne, h.tol, case.g)
        err = float(np.sqrt(((np.asarray(rec.q, cr.LD) - ref.q) ** 2).sum()))
        net = abs(float(np.asarray(rec.q, cr.LD).sum()))
        nb = cr.sum_bound(ne, rec.iterations, float(np.abs(rec.q).max()))
        print(f"  Ne={ne} tol {h.tol:g}: {rec.iterations} iterations (cg_ref {want}), ||q - q*|| / bound = {err / bound:.3f}, "
              f"|sum q| / bound = {net / nb:.3f}")
        assert np.isfinite(rec.q).all() and rec.iterations > 0 and abs(rec.iterations - want) <= 1
        assert want == cr.ITERS[ne][extra is TIGHT] and (want > 20 if extra is TIGHT else 6 <= want <= 12)
        assert err <= bound and net <= nb
        assert rec.res == ["%g" % float(x) for x in ref.hist[1:rec.iterations + 1]], rec.res
        m = re.search(r"netcharge = (\S+)$", rec.lines[-1])
        assert m and abs(float(m.group(1))) <= nb
        assert h.tails_are_nan()


@pytest.mark.parametrize("ne", cr.SIZES)
def test_one_launch_and_two_launch_forms_give_the_same_bytes(cases, ne):
    """(c) cg_step_kernel against gemv_rows_guarded_kernel + cg_update_kernel: converged inside the first batch, over several
    batches, and cut off by maxiter"""
    case = cases(ne)
    for extra in (DEFAULT, TIGHT, THREE):
        one, two = _handle(case, extra), _handle(case, extra, two_launch=True)
        assert not one.two_launch and two.two_launch
        for name in ("dense", "dense2", "unit_last"):
            a, b = one.solve(case.b[name]), two.solve(case.b[name])
            assert a.iterations == b.iterations and a.lines == b.lines and len(a.lines) > 0, (ne, extra, name, a.lines, b.lines)
            assert np.array_equal(cr.bits(a.q), cr.bits(b.q)), (ne, extra, name)
        assert one.tails_are_nan() and two.tails_are_nan()
    assert len(_handle(case, TIGHT).solve(case.b["dense"]).schedule.batches) >= 3


@pytest.mark.parametrize("ne", [1664, 4097, 8200])
def test_the_batch_schedule_cannot_change_the_answer(cases, ne):
    """(d) the first batch is as long as the last converged solve was (2 to 16), later ones 4: every solve of the same b gives the
    same bytes and the same history whatever the solve before it was, one that ran out of maxiter included"""
    case = cases(ne)
    hist = case.ref["dense"].hist
    tol, maxiter = _tol(SCHED), _maxiter(SCHED)
    b = {"b1": cr.scale_to_need(hist, ne, tol, 22) * case.b["dense"],           # more than 16 iterations
         "b2": cr.scale_to_need(hist, ne, tol, 6) * case.b["dense2"],           # 5 to 8
         "b0": 2.0 ** 20 * case.b["dense"]}                                      # more than maxiter allows
    assert cr.needed(hist, ne, tol, 2.0 ** 20) is None and len(hist) > maxiter
    seen = {k: [] for k in b}
    for tag, order in (("first", ("b1", "b1", "b2", "b2", "b1", "b0", "b2")), ("second", ("b2", "b1", "b1", "b0", "b1"))):
        h = _handle(case, SCHED, tag=tag)
        for name in order:
            seen[name].append(h.solve(b[name]))
        assert h.tails_are_nan()
    for name, recs in seen.items():
        for r in recs[1:]:
            assert r.iterations == recs[0].iterations and r.lines == recs[0].lines, (ne, name)
            assert np.array_equal(cr.bits(r.q), cr.bits(recs[0].q)), (ne, name)
    n1, n2 = seen["b1"][0].iterations, seen["b2"][0].iterations
    print(f"  Ne={ne}: b1 {n1} iterations, b2 {n2}, b0 {len(seen['b0'][0].lines)} without converging; first batches of b1 "
          f"{[len(r.schedule.batches[0]) - 1 for r in seen['b1']]}, of b2 {[len(r.schedule.batches[0]) - 1 for r in seen['b2']]}")
    assert 21 <= n1 <= 24 and 5 <= n2 <= 8
    assert all(r.iterations == 0 and len(r.lines) == maxiter - 1 and np.isfinite(r.q).all() for r in seen["b0"])
    # the sequences of launches really differ, and between them convergence fell on the last iteration of a batch, inside a batch
    # and in a third batch
    for name in ("b1", "b2"):                                # (first batches of 16, of b2's count, and of what the setup left)
        assert len({str(r.schedule.batches) for r in seen[name]}) >= 2, name
    every = seen["b1"] + seen["b2"]
    assert {"last", "inside"} <= {r.schedule.where for r in every}
    assert any(len(r.schedule.batches) == 3 for r in every) and any(len(r.schedule.batches) == 1 for r in every)
    assert any(len(r.schedule.batches) > 3 for r in every)
    # and each is what cg_ref gives, scaled
    ref = case.ref["dense"]
    s1 = cr.scale_to_need(hist, ne, tol, 22)
    assert seen["b1"][0].res == ["%g" % float(s1 * s1 * x) for x in ref.hist[1:n1 + 1]]
    err = float(np.sqrt(((np.asarray(seen["b1"][0].q, cr.LD) - s1 * ref.q) ** 2).sum()))
    assert err <= cr.converged_bound(ne, tol, case.g)


@pytest.mark.parametrize("ne", cr.SIZES)
def test_maxiter_edges(cases, ne):
    """(e) maxiter 1: no iteration (the two-launch form's start kernel alone); 2: one iteration; the needed count: one short of
    converging; the needed count + 1: converged by the last launch it was allowed"""
    case = cases(ne)
    nd = cr.ITERS[ne][0]
    b = case.b["dense"]
    h = _handle(case, ("cg", "maxiter", "1"))
    h.big_q.fill_(float("nan"))
    rec = h.solve(b)
    assert rec.schedule.two_launch and rec.iterations == 0 and rec.lines == [] and not rec.q.any() and not np.signbit(rec.q).any()
    assert h.tails_are_nan()
    rec = _handle(case, ("cg", "maxiter", "2")).solve(b)
    _assert_cut_off(f"Ne={ne} maxiter 2", case, rec, "dense", 1)
    assert rec.schedule.batches == [[(1, 1), (1, 4)]]
    rec = _handle(case, ("cg", "maxiter", str(nd))).solve(b)
    _assert_cut_off(f"Ne={ne} maxiter {nd}", case, rec, "dense", nd - 1)
    h = _handle(case, ("cg", "maxiter", str(nd + 1)))
    rec = h.solve(b)
    _assert_cut_off(f"Ne={ne} maxiter {nd + 1}", case, rec, "dense", nd, converged=True)
    assert rec.schedule.converged and rec.schedule.batches[-1][-1] == (nd, 4)
    rec2 = h.solve(b)                                        # again, now with a first batch of exactly the needed length
    assert len(rec2.schedule.batches) == 1 and rec2.schedule.where == "last"
    assert rec2.lines == rec.lines and np.array_equal(cr.bits(rec2.q), cr.bits(rec.q))
    assert h.tails_are_nan()


@pytest.mark.parametrize("ne", [1664, 4097])
def test_charge_write_of_a_cg_update(cases, ne):
    """(f) conp_fix_pre_force_device on one rank enqueues the charge write behind every batch before it knows whether the batch
    converged (update_direct's spec_dq): when the first batch does not converge, charges of an unconverged q are written and must
    be replaced after the last batch.  The update forms b itself, from the electrolyte's charges."""
    case = cases(ne)
    hist = case.ref["dense"].hist
    for extra, prime, several in ((TIGHT, cr.scale_to_need(hist, ne, cr.TOL_TIGHT, 6) * case.b["dense2"], True),
                                  (DEFAULT, cr.scale_to_need(hist, ne, cr.TOL_DEFAULT, 18) * case.b["dense"], False)):
        h = _handle(case, extra)
        p = h.solve(prime)                                   # sets the length of the next first batch: 5 to 8, or 16
        assert p.iterations > 0 and (5 <= p.iterations <= 8 if several else p.iterations > 16)
        before = h.random_charges(11, everywhere=False)
        h.fx.pre_force_device(h.d_x.data_ptr(), h.d_q.data_ptr(), DV)
        rec = h.record()
        b_own = h.big_b[:ne].cpu().numpy()
        assert np.isfinite(b_own).all() and np.abs(b_own).max() > 0 and rec.iterations > 0
        print(f"  Ne={ne} {' '.join(extra)}: its own b took {rec.iterations} iterations in {len(rec.schedule.batches)} batch(es), "
              f"the first of {len(rec.schedule.batches[0]) - 1}")
        assert (len(rec.schedule.batches) > 1) == several    # a speculative write of an unconverged q happened / the first write is the final one
        assert np.array_equal(cr.bits(h.atom_charges()), cr.bits(h.want_charges(before, DV)))
        # q really is the solution of the loaded matrix for that b.  The square of the true projected residual is the recursive
        # lr < n tol (factor 2 in the norm as in cg_ref.converged_bound) as far as float64 resolves it: this b has a mean of the
        # size of its entries, and lg = sum r^2 - netr ave and lr = sum r p then cancel n terms of the size of b_i^2, each rounded
        # at 2^-53 -- over k iterations squared residuals below 4 k 2^-53 sum b^2 are not told apart (cg_f64 shows the same floor)
        r = np.asarray(b_own, cr.LD) - cr.matvec_ld(case.A, rec.q)
        pr = float(np.sqrt(((r - r.mean()) ** 2).sum()))
        allowed = float(np.sqrt(4.0 * ne * h.tol + 4.0 * rec.iterations * cr.U * (b_own ** 2).sum()))
        print(f"  Ne={ne}: ||P (b - A q)|| = {pr:.3e}, allowed {allowed:.3e} (2 sqrt(n tol) = {2.0 * np.sqrt(ne * h.tol):.3e}), max|b| = {np.abs(b_own).max():.3e}")
        assert pr <= allowed
        # and the same b through conp_fix_solve_device, which starts with another first batch: the same history and bytes
        again = h.solve(b_own)
        assert again.lines == rec.lines and np.array_equal(cr.bits(again.q), cr.bits(rec.q))
        assert again.schedule.batches != rec.schedule.batches
        # the unfused pair of entries, on an injected b
        before = h.random_charges(12, everywhere=True)
        rec = h.solve(case.b["dense"])
        h.fx.scatter_device(h.d_q.data_ptr(), -0.9)
        assert rec.iterations > 0
        assert np.array_equal(cr.bits(h.atom_charges()), cr.bits(h.want_charges(before, -0.9)))
        assert np.array_equal(cr.bits(h.fx.vectors()[1]), cr.bits(rec.q)) and h.tails_are_nan()


GUARD_CHILD = r'''
import sys, numpy as np
sys.path.insert(0, {pkg!r}); sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import torch
torch.cuda.init()
import cg_ref as cr, test_gpu_cg_sizes as t
from conp_amd import capi
lib = capi.load_library()
lib.conp_debug_check_guards.restype = int
assert lib.conp_debug_check_guards() == 0, "guard zones are off"
for ne in (4097, 8200):
    case = t.Case(ne, references=False)
    for extra in (t.DEFAULT, t.TIGHT):
        got = []
        for two in (False, True):
            h = t._handle(case, extra, two_launch=two)
            got.append(h.solve(case.b["dense"]))
            bad = lib.conp_debug_check_guards()
            assert bad == 0, (ne, extra, two, bad, lib.conp_last_error().decode())
            assert got[-1].iterations == cr.ITERS[ne][extra is t.TIGHT] and h.tails_are_nan()
        assert np.array_equal(cr.bits(got[0].q), cr.bits(got[1].q))
    for h in case.handles.values():
        h.fx.close()
    assert lib.conp_debug_check_guards() == 0
print("GUARD_OK")
'''


def test_no_cg_kernel_stores_outside_its_buffers(tmp_path):
    """(g) the sizes above 4096 in both launch forms, in a child process with guard zones around every device buffer of the library"""
    script = tmp_path / "cg_guard_child.py"
    script.write_text(GUARD_CHILD.format(pkg=os.path.join(ROOT, "lammps-user-conp2_amd"), root=ROOT, tests=os.path.join(ROOT, "tests")))
    env = dict(os.environ, CONP_GUARD="1")
    p = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "GUARD_OK" in p.stdout
