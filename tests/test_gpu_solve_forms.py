"""-m gpu: the last stage of every charge update, q = S b + dV setq (+ qinit) written to every copy of each electrode atom, in each
of its forms, with a matrix and a b vector the test chose (tests/solve_ref.py makes them and counts the roundings).

A handle goes through its normal setup; conp_fix_set_matrix then replaces the solve matrix by M = R + R.T (exactly symmetric, every
128 x 128 tile with a magnitude and sign of its own), the test binds its own b and q vectors (Ne + 512 long, NaN behind the first
Ne entries) and writes b into the first Ne entries.  setq stays what the setup left.  Forms:
  fused     conp_fix_update_charge on a one-rank `fix conp` handle: gemv_finish_kernel below 2048 electrode atoms, the packed
            symmetric kernels (sym_pack / sym_gemv / sym_finish) from 2048 up;
  rows      the same entry on a handle created under CONP_PATH_GEMV_ROWS: gemv_finish_kernel at every size;
  unfused   conp_fix_solve_device + conp_fix_scatter_device: gemv_rows_kernel, then charge_finish_kernel.
conp_fix_pre_force_device forms b itself and cannot take an injected one: its charge write is checked with the b it computed,
read back with vectors().  Every other entry takes the injected b.

The constant c of the entry-wise bound |y_i - ref_i| <= c 2^-53 sum_j |M_ij| |b_j| is the longest chain of dependent roundings a
term passes through, counted from the kernels (solve_ref.rows_chain / packed_chain; tests/test_solve_ref_math.py pins the numbers):

  rows form (gemv_row_dot + wave_sum).  Even n: a lane's accumulators s0 / s1 take 4 fmas per 8-wide trip, 2 per 4-wide trip and 1
  per 1-wide trip, t0 / t1 the same without the 1-wide ones; the first fma of an accumulator rounds the product, each later one
  rounds the running sum.  Then s0 += t0 (one rounding where a wide loop ran), s0 + s1 (one), and six shuffle-adds (one each where
  the partner lanes hold something).  Odd n: one accumulator, ceil((n - lane) / 64) fmas, s0 + s1 adds an exact zero.
      n = 4232: 4 trips 8-wide + 2 trips 1-wide in lanes 0-3 = 18 fmas, + 1 + 1 + 6 = 26
      n = 2049: 33 + 6 = 39    2048: 8 + 1 + 1 + 6 = 16    2047: 32 + 6 = 38    1026: 4 + 1 + 1 + 1 + 6 = 13    962: 13    961: 16 + 6 = 22
      n = 450: 2 + 1 + 1 + 6 = 10    130: 2 + 1 + 6 = 9    62: 1 + 1 + 5 = 7 (31 lanes hold an element: five shuffle-adds round)
  packed form.  A direct slot (source tile on or left of the diagonal): x * b0 rounded, y * b1 fma'd onto it, six butterfly adds
  = 8.  A transposed slot: 32 fmas down the wavefront's rows, then (tr0 + tr1) + (tr2 + tr3) = 34.  sym_finish_kernel's thread g adds
  the slots g, g + 4, ... in order, the first one onto 0.0 (exact), then (p0 + p1) + (p2 + p3) = 2.  The longest chain is a
  transposed slot at the head of the longest run:
      nb = 16 (2048): 34 + 3 + 2 = 39    nb = 17 (2049): 34 + 4 + 2 = 40 (slot 4 of a row of block 0: four later adds of thread 0)
      nb = 34 (4232): 34 + 8 + 2 = 44 (slot 1 of a row of block 0: thread 1 adds nine slots, 1, 5, ... 33, the last in its second pass)
  fix scalar.  dV totsetq + sum of y over the group-1 rows: the summation tree's chain (solve_ref.left_chain_1024 for
  left_sum_kernel / results_out_kernel, left_chain_4096 for charge_finish_kernel's last block, both from the actual group-1 rows),
  plus one for the final add; the product dV totsetq is rounded twice.  fix conq: the tree, one subtraction, one division.

The reference is the float128 product (x86 long double: its own error is below 0.01 * 2^-53 * A_i).  Every test prints the worst
fraction of its bound."""
import dataclasses

import numpy as np
import pytest

import solve_ref as sr
from conp_amd import FixConp, capi, neighbor

pytestmark = pytest.mark.gpu

DV = 1.7                      # not the potential difference of the setup


class Case:
    """one electrode count: the system, its lists, the matrix, the b vectors and their float128 products -- made once"""

    def __init__(self, ne):
        self.ne = ne
        self.s = sr.system(ne)
        self.at, self.alist, self.blist = neighbor.build_lists(self.s)
        self.M = sr.matrix(ne, 1000 + ne)
        self.b = sr.vectors(ne, 2000 + ne)
        self.ref = {k: sr.ref_product(self.M, v) for k, v in self.b.items()}
        self.ele_atoms = np.nonzero(self.at.echeck != 0)[0]              # owned and ghost copies of electrode atoms
        assert np.count_nonzero(self.ele_atoms >= self.at.nlocal) > 400
        self.handles = {}
        self.ele_row = None                                              # eleall index of each of ele_atoms (from the first handle)
        self.left = None                                                 # group-1 rows

    def atoms(self, q=None):
        """the atom arrays with a charge array of their own: a handle's updates write into it"""
        return dataclasses.replace(self.at, q=(self.at.q if q is None else q).copy())


class Handle:
    def __init__(self, case, fx, at, qinit=None):
        import torch
        self.case, self.fx, self.at, self.ne, self.qinit = case, fx, at, case.ne, qinit
        assert fx.info().elenum_all == case.ne
        m = fx.maps()
        if case.ele_row is None:
            case.ele_row = m["tag2eleall"][case.at.tag[case.ele_atoms]].astype(np.int64)
            case.left = m["elecheck_eleall"] == 1
            assert case.ele_row.min() == 0 and case.ele_row.max() == case.ne - 1
        self.big_b = torch.full((case.ne + 512,), float("nan"), dtype=torch.float64, device="cuda")
        self.big_q = torch.full((case.ne + 512,), float("nan"), dtype=torch.float64, device="cuda")
        fx.bind_device_buffers(self.big_b.data_ptr(), self.big_q.data_ptr())
        self.setq = fx.vectors()[2].copy()
        self.totsetq = fx.info().totsetq
        self.d_x = torch.from_numpy(np.ascontiguousarray(at.x)).cuda()
        self.d_q = torch.zeros(at.nall, dtype=torch.float64, device="cuda")

    def inject(self, b):
        import torch
        self.big_b[:self.ne] = torch.from_numpy(np.ascontiguousarray(b)).cuda()

    def y(self):
        import torch
        torch.cuda.synchronize()
        return self.big_q[:self.ne].cpu().numpy().copy()

    def tails_are_nan(self):
        import torch
        torch.cuda.synchronize()
        return bool(torch.isnan(self.big_b[self.ne:]).all() and torch.isnan(self.big_q[self.ne:]).all())

    def fused(self, b, dV=DV):
        """conp_fix_update_charge -> (y, atom charges before, atom charges after)"""
        self.inject(b)
        before = self.at.q.copy()
        self.fx.update_charge(self.at, dV)
        return self.y(), before, self.at.q.copy()

    def unfused(self, b, dV=DV, seed=7):
        """conp_fix_solve_device + conp_fix_scatter_device into an atom charge array of arbitrary bit patterns"""
        import torch
        self.inject(b)
        before = np.random.default_rng(seed).integers(-2 ** 63, 2 ** 63 - 1, size=self.at.nall, dtype=np.int64).view(np.float64)
        self.d_q.copy_(torch.from_numpy(before.view(np.int64)).cuda().view(torch.float64))
        self.fx.solve_device(dV)
        self.fx.scatter_device(self.d_q.data_ptr(), dV)
        y = self.y()
        return y, before, self.d_q.cpu().numpy()

    def want_charges(self, y, before, dV):
        """the atom charge array after the write: every copy of electrode atom e holds y[e] + dV setq[e] (+ qinit[e]), the rest its bits"""
        v = sr.charges(y, dV, self.setq, self.qinit)
        out = before.copy()
        out[self.case.ele_atoms] = v[self.case.ele_row]
        return out


def _handle(case, kind):
    """kinds: "fused" (the library's choice of form), "rows" (CONP_PATH_GEMV_ROWS), "conq", "qinit", ("rank", r, nranks)"""
    if kind in case.handles:
        return case.handles[kind]
    s, ne = case.s, case.ne
    qinit = None
    if kind == "qinit":
        s, by_tag = sr.with_electrode_charges(case.s, 3000 + ne)
        at = case.atoms(q=by_tag[case.at.tag])
    else:
        at = case.atoms()
    if isinstance(kind, tuple):
        fx = FixConp(s, rank=kind[1], nranks=kind[2])
        fx.init_lists(case.alist, case.blist)
        fx.setup_post_neighbor(at)
        fx.linalg_setup(at)                          # replicated atoms, no communicator: the host would do the two collectives
    else:
        with capi.test_paths(capi.PATH_GEMV_ROWS if kind == "rows" else 0):
            fx = FixConp(s, style="conq" if kind == "conq" else "conp", extra_args=("qinit",) if kind == "qinit" else ())
            fx.init_lists(case.alist, case.blist)
            fx.setup_post_neighbor(at)
            fx.setup_pre_force(at, 0, 0.05 if kind == "conq" else s.potdiff)
        assert fx.row_range() == (0, ne)
    fx.set_matrix(case.M, 3)
    h = Handle(case, fx, at)
    if kind == "qinit":
        h.qinit = by_tag[fx.maps()["eleall2tag"]]
        assert fx.args.qinit == 1 and np.count_nonzero(h.qinit) == ne
    case.handles[kind] = h
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


def _forms(case):
    """(name, handle, entry, c) of every form the solve has at this size"""
    ne = case.ne
    f = _handle(case, "fused")
    out = [("packed" if sr.packed(ne) else "rows", f, f.fused, sr.packed_chain(ne) if sr.packed(ne) else sr.rows_chain(ne)),
           ("unfused", f, f.unfused, sr.rows_chain(ne))]
    if sr.packed(ne):
        r = _handle(case, "rows")
        out.insert(1, ("rows", r, r.fused, sr.rows_chain(ne)))
    return out


def _assert_bound(tag, y, ref, A, c):
    frac = sr.worst_fraction(y, ref, A, c)
    print(f"  {tag}: c = {c}, worst |y - ref| / (c 2^-53 A) = {frac:.3f}")
    assert np.isfinite(y).all() and frac <= 1.0, (tag, frac)


def _assert_columns(tag, entry, M, js):
    ne = M.shape[0]
    for j in js:
        e = np.zeros(ne)
        e[j] = 1.0
        y = entry(e)[0]
        bad = np.nonzero(y != M[:, j])[0]
        assert bad.size == 0, (tag, j, bad[:8], y[bad[:8]], M[bad[:8], j])


def test_sizes_reach_what_they_are_for():
    """the properties of the sizes the other tests rely on: a change of a kernel constant shows here, not as a hollow pass there"""
    sr.check_sizes()
    assert (capi.PATH_GEMV_ROWS, sr.SG_T, sr.SF_R, sr.SYM_FROM) == (16, 128, 32, 2048)


@pytest.mark.parametrize("ne", sr.SIZES)
def test_unit_vectors_give_exact_columns(cases, ne):
    """b = e_j: every product is by 1 or 0 and every sum has one non-zero term, so y is column j of M to the bit, in every form"""
    case = cases(ne)
    js = sr.column_indices(ne)
    for name, h, entry, _c in _forms(case):
        _assert_columns(f"Ne={ne} {name}", entry, case.M, js)
        assert h.tails_are_nan()
    print(f"  Ne={ne}: {len(js)} columns x {[f[0] for f in _forms(case)]}")


@pytest.mark.parametrize("ne", sr.SIZES)
def test_every_row_within_its_rounding_bound(cases, ne):
    case = cases(ne)
    for name, _h, entry, c in _forms(case):
        for bname, b in case.b.items():
            ref, A = case.ref[bname]
            _assert_bound(f"Ne={ne} {name} b={bname}", entry(b)[0], ref, A, c)
    if sr.packed(ne):
        assert "not symmetric" not in _handle(case, "fused").fx.mesg_drain()


@pytest.mark.parametrize("ne", sr.SIZES)
def test_charge_write_bit_for_bit(cases, ne):
    """every owned and ghost copy of electrode atom e holds the float64 value y[e] + dV setq[e]; nothing else changes"""
    import torch
    case = cases(ne)
    b = case.b["scaled0"]
    for name, h, entry, _c in _forms(case):
        y, before, after = entry(b)
        assert np.array_equal(sr.bits(after), sr.bits(h.want_charges(y, before, DV))), (ne, name)
        assert h.tails_are_nan()
    # conp_fix_pre_force_device forms b itself: the b it computed, and the charges it wrote into the caller's device array
    h = _handle(case, "fused")
    before = h.at.q.copy()
    h.d_q.copy_(torch.from_numpy(before).cuda())
    h.fx.pre_force_device(h.d_x.data_ptr(), h.d_q.data_ptr(), DV)
    y = h.y()
    b_own = h.big_b[:ne].cpu().numpy()
    assert np.isfinite(b_own).all() and np.abs(b_own).max() > 0
    assert np.array_equal(sr.bits(h.d_q.cpu().numpy()), sr.bits(h.want_charges(y, before, DV)))
    ref, A = sr.ref_product(case.M, b_own)
    _assert_bound(f"Ne={ne} pre_force_device (its own b)", y, ref, A, sr.packed_chain(ne) if sr.packed(ne) else sr.rows_chain(ne))
    assert h.tails_are_nan()


def test_charge_write_with_qinit(cases):
    case = cases(2049)
    h = _handle(case, "qinit")
    b = case.b["scaled1"]
    for name, entry in (("packed", h.fused), ("unfused", h.unfused)):
        y, before, after = entry(b)
        want = h.want_charges(y, before, DV)
        assert np.array_equal(sr.bits(after), sr.bits(want)), name
        assert np.any(want[case.ele_atoms] != (y + DV * h.setq)[case.ele_row])       # (qinit took part)
    ref, A = case.ref["scaled1"]
    _assert_bound("Ne=2049 qinit packed", h.fused(b)[0], ref, A, sr.packed_chain(2049))
    assert h.tails_are_nan()


@pytest.mark.parametrize("ne", sr.SIZES)
def test_fused_and_unfused_rows_forms_give_the_same_bytes(cases, ne):
    """gemv_finish_kernel against gemv_rows_kernel + charge_finish_kernel (at 4232 both in their non-temporal variants)"""
    case = cases(ne)
    h = _handle(case, "rows" if sr.packed(ne) else "fused")
    assert sr.nontemporal(ne, ne) == (ne == 4232)
    for bname, b in case.b.items():
        yf, _, qf = h.fused(b)
        yu, _, qu = h.unfused(b)
        assert np.array_equal(sr.bits(yf), sr.bits(yu)), (ne, bname)
        assert np.array_equal(sr.bits(qf[case.ele_atoms]), sr.bits(qu[case.ele_atoms])), (ne, bname)


@pytest.mark.parametrize("ne", [961, 4232])
def test_row_shards_of_three_ranks(cases, ne):
    """conp_fix_solve_device on rank r of 3 writes the rows [r ceil(Ne / 3), ...) with the bits of the one-rank rows form and
    nothing else (at 4232 a shard streams 48 MB: the plain kernel, against the non-temporal one of the one-rank handle)"""
    import torch
    case = cases(ne)
    one = _handle(case, "rows" if sr.packed(ne) else "fused")
    b = case.b["scaled0"]
    y1 = one.unfused(b)[0]
    assert not sr.nontemporal(-(-ne // 3), ne)
    covered = np.zeros(ne, int)
    for r in range(3):
        h = _handle(case, ("rank", r, 3))
        r0, r1 = h.fx.row_range()
        assert (r0, r1) == sr.row_range(ne, r, 3)
        h.big_q.fill_(float("nan"))
        h.inject(b)
        h.fx.solve_device(DV)
        torch.cuda.synchronize()
        q = h.big_q.cpu().numpy()
        assert np.array_equal(sr.bits(q[r0:r1]), sr.bits(y1[r0:r1]))
        assert np.isnan(q[:r0]).all() and np.isnan(q[r1:]).all()
        covered[r0:r1] += 1
    assert np.all(covered == 1)


def test_a_rank_without_rows_writes_nothing(cases):
    import torch
    case = cases(130)
    h = _handle(case, ("rank", 63, 64))
    assert h.fx.row_range() == (130, 130) == sr.row_range(130, 63, 64)
    h.big_q.fill_(float("nan"))
    h.inject(case.b["ones"])
    h.fx.solve_device(DV)                        # (a status other than CONP_OK raises)
    torch.cuda.synchronize()
    assert torch.isnan(h.big_q).all()


def _scalar_bound(tag, got, y, left, dV, totsetq, c):
    ref = np.longdouble(dV) * np.longdouble(totsetq) + np.asarray(y[left], np.longdouble).sum()
    A = float(np.abs(y[left]).sum() + abs(dV * totsetq))
    frac = float(abs(np.longdouble(got) - ref)) / (c * sr.U * A)
    print(f"  {tag}: c = {c}, |scalar - ref| / (c 2^-53 A) = {frac:.3f}")
    assert np.isfinite(got) and frac <= 1.0, (tag, got, float(ref), frac)
    return A


@pytest.mark.parametrize("ne", sr.SIZES)
def test_fix_scalar_of_both_routes(cases, ne):
    """compute_scalar() = dV totsetq + the sum of y over the group-1 rows, after the fused update (results_out_kernel's tree) and
    after the unfused one (charge_finish_kernel's 4096-stride tree; at 4232 the group-1 rows reach into its second round)"""
    case = cases(ne)
    h = _handle(case, "fused")
    b = case.b["scaled1"]
    cf, cu = max(sr.left_chain_1024(case.left) + 1, 2), max(sr.left_chain_4096(case.left) + 1, 2)
    y = h.fused(b)[0]
    sf = h.fx.compute_scalar()
    A = _scalar_bound(f"Ne={ne} fused", sf, y, case.left, DV, h.totsetq, cf)
    # another vector and another potential on the other route: a scalar left over from the update before cannot pass
    b2, dV2 = case.b["scaled0"], -0.9
    y2 = h.unfused(b2, dV2)[0]
    _scalar_bound(f"Ne={ne} unfused, second input", h.fx.compute_scalar(), y2, case.left, dV2, h.totsetq, cu)
    y = h.unfused(b)[0]
    su = h.fx.compute_scalar()
    _scalar_bound(f"Ne={ne} unfused", su, y, case.left, DV, h.totsetq, cu)
    y2 = h.fused(b2, dV2)[0]
    _scalar_bound(f"Ne={ne} fused, second input", h.fx.compute_scalar(), y2, case.left, dV2, h.totsetq, cf)
    if not sr.packed(ne):                        # the same y: the two trees agree within the sum of their bounds
        assert abs(sf - su) <= (cf + cu) * sr.U * A
    else:
        r = _handle(case, "rows")
        yr = r.fused(b)[0]
        sfr = r.fx.compute_scalar()
        Ar = _scalar_bound(f"Ne={ne} rows", sfr, yr, case.left, DV, r.totsetq, cf)
        assert np.array_equal(sr.bits(yr), sr.bits(y)) and abs(sfr - su) <= (cf + cu) * sr.U * Ar


@pytest.mark.parametrize("ne", [2049, 4232])
def test_conq_scalar_and_charges(cases, ne):
    """fix conq (unfused, rows form): the scalar is the potential difference -(Q + sum_left y) / totsetq from left_sum_kernel's
    tree, one subtraction and one division; the charges are y + scalar * setq to the bit"""
    case = cases(ne)
    h = _handle(case, "conq")
    assert h.fx.args.conq == 1
    Q = 0.37
    b = case.b["scaled0"]
    y, before, after = h.fused(b, Q)
    dv = h.fx.compute_scalar()
    ref, A = case.ref["scaled0"]
    _assert_bound(f"Ne={ne} conq rows", y, ref, A, sr.rows_chain(ne))
    left = case.left
    want = -(np.longdouble(Q) + np.asarray(y[left], np.longdouble).sum()) / np.longdouble(h.totsetq)
    c = sr.left_chain_1024(left) + 2
    bound = c * sr.U * float(np.abs(y[left]).sum() + abs(Q)) / abs(h.totsetq)
    frac = float(abs(np.longdouble(dv) - want)) / bound
    print(f"  Ne={ne} conq: c = {c}, |scalar - ref| / bound = {frac:.3f}")
    assert np.isfinite(dv) and frac <= 1.0
    assert np.array_equal(sr.bits(after), sr.bits(h.want_charges(y, before, dv)))
    assert h.tails_are_nan()


def test_the_packed_copy_follows_the_matrix(cases):
    """conp_fix_set_matrix twice on one handle: the second update multiplies with the second matrix.  A third matrix, unsymmetric
    above the 1e-10 gate in one element, is multiplied by full rows, and the log says so once."""
    case = cases(2049)
    ne = 2049
    s, at = case.s, case.atoms()
    fx = FixConp(s)
    fx.init_lists(case.alist, case.blist)
    fx.setup_post_neighbor(at)
    fx.setup_pre_force(at, 0, s.potdiff)
    fx.set_matrix(case.M, 3)
    h = Handle(case, fx, at)
    case.handles["generation"] = h
    c = sr.packed_chain(ne)
    ref, A = case.ref["scaled0"]
    _assert_bound("first matrix", h.fused(case.b["scaled0"])[0], ref, A, c)
    M2 = sr.matrix(ne, 4000 + ne)
    fx.set_matrix(M2, 3)
    js = sr.column_indices(ne)
    _assert_columns("second matrix", h.fused, M2, js)
    for bname, b in case.b.items():
        ref2, A2 = sr.ref_product(M2, b)
        y2 = h.fused(b)[0]
        _assert_bound(f"second matrix b={bname}", y2, ref2, A2, c)
    assert "not symmetric" not in fx.mesg_drain()
    M3 = M2.copy()
    M3[ne - 1, 0] += 1e-8 * np.abs(M2).max()
    assert M3[ne - 1, 0] != M3[0, ne - 1]
    fx.set_matrix(M3, 3)
    ones = case.b["ones"]
    y3 = h.fused(ones)[0]
    assert fx.mesg_drain().count("not symmetric") == 1
    cr = sr.rows_chain(ne)
    ref3, A3 = sr.ref_product(M3, ones)
    _assert_bound("unsymmetric matrix, full rows", y3, ref3, A3, cr)
    sym = sr.ref_product(sr.lower_symmetrised(M3), ones)[0]
    gap = float(abs(np.longdouble(y3[0]) - sym[0]))
    print(f"  row 0 against the symmetrised product: {gap / (cr * sr.U * A3[0]):.3g} bounds")
    assert gap > 100 * cr * sr.U * A3[0]
    _assert_columns("unsymmetric matrix", h.fused, M3, [0, ne - 1])           # the upper and the lower corner, each as loaded
    h.fused(case.b["scaled0"])
    assert "not symmetric" not in fx.mesg_drain()                            # said once per matrix, not once per update
    assert h.tails_are_nan()
