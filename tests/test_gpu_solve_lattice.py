"""The lattice form of the solve (conp_kernels.hip lat_gemv_kernel): electrodes that are perfect lattices multiply a table
T[basis_i][basis_j][cell_j - cell_i] of Ne * nbasis numbers instead of the packed matrix, and one launch writes the charges.

Boxes: synthetic_fast(..., lz=80, n_elyte=256, cutoff=8.0, g_ewald=0.35, accuracy_relative=1e-6), the smallest that reach the path
(Ne >= 2048):
  A  32 x 8 cells, 1 layer    Ne 2048, nx != ny, 8 basis atoms
  B  13 x 20 cells, 1 layer   Ne 2080, odd nx, Ne no multiple of 128, a ragged last block of cells, a wrap in every block
  C  16 x 8 cells, 2 layers   Ne 2048, 16 basis atoms
  D  20 x 13 cells, 1 layer   Ne 2080, ny no multiple of 4: the kernel's one-row-per-thread instantiation
A handle goes through its normal setup; the tests bind their own b and q vectors (Ne + 512 long, NaN behind the first Ne entries: a
b entry beyond Ne that is read shows) and drive conp_fix_update_charge as tests/test_gpu_solve_forms.py does.

Bound of a row against the float128 product with the matrix read back through matrix():
    |y_i - (S b)_i| <= c 2^-53 sum_j |S_ij| |b_j| + dev sum_j |b_j|
c: the kernel's counted chain of dependent roundings (lattice_ref.chain restates the launch shape and the count); dev = max |S_ij -
T[..]| as the library measured and reports it (conp_fix_get_solve_form) -- the table is what is multiplied, S is what it is compared
with.  Every test prints the worst fraction of its bound."""
import dataclasses

import numpy as np
import pytest

import lattice_ref as lr
import solve_ref as sr
from conp_amd import FixConp, capi, neighbor

gpu = pytest.mark.gpu

CELLS = {"A": (32, 8, 1), "B": (13, 20, 1), "C": (16, 8, 2), "D": (20, 13, 1)}
DV = 1.7                      # not the potential difference of the setup


def _electrode_x(s):
    return s.x[s.echeck != 0]


def test_host_restatement_of_the_lattice_search():
    """no GPU: numpy finds (a, b, nx, ny, basis, cell maps), the maps are a bijection and the two permutations commute; the library's
    host search (conp_host_find_lattice) gives the same map, also with the atoms in another order"""
    for name, (cx, cy, layers) in CELLS.items():
        s = lr.system(cx, cy, layers)
        x = _electrode_x(s)
        for order in (np.arange(len(x)), np.random.default_rng(len(x)).permutation(len(x))):
            lat = lr.find(x[order], s.prd[0], s.prd[1])
            assert (lat["nx"], lat["ny"], lat["nbasis"]) == (cx, cy, 8 * layers), name
            assert abs(lat["a"] - 32.2 / 13.0) < 1e-9 and abs(lat["b"] - 34.4 / 8.0) < 1e-9
            lr.check_maps(lat, len(x))
            got = capi.find_lattice(x[order], s.prd[0], s.prd[1])
            assert got is not None and (got["nx"], got["ny"], got["nbasis"]) == (cx, cy, 8 * layers)
            assert np.array_equal(got["row"], lat["row"])
            assert np.array_equal(got["pos"], np.stack([lat["beta"], lat["cx"], lat["cy"]], 1))
        x2 = x.copy()
        x2[5, 0] += 1e-3                                      # ten tolerances: only the identity is left
        got = capi.find_lattice(x2, s.prd[0], s.prd[1])
        assert got is not None and (got["nx"], got["ny"], got["nbasis"]) == (1, 1, len(x))
        assert lr.shape(1, 1, len(x)) is None
    assert lr.shape(32, 16, 8) == dict(R=4, sy=18, G=8, CB=16) and lr.chain(32, 16, 8) == 39          # the headline box
    assert lr.shape(64, 32, 8) == dict(R=4, sy=34, G=4, CB=64) and lr.chain(64, 32, 8) == 517         # the 16384-atom box
    assert lr.shape(80, 64, 8) is None                                                                # 16 nx ny bytes > 64 KB


class Box:
    """one system: its lists, and the handles made on it"""

    def __init__(self, s):
        self.s = s
        self.ne = int(np.count_nonzero(s.echeck))
        self.at, self.alist, self.blist = neighbor.build_lists(s)
        self.ele_atoms = np.nonzero(self.at.echeck != 0)[0]
        assert np.count_nonzero(self.ele_atoms >= self.at.nlocal) > 400
        self.handles = {}
        self.lat = None

    def handle(self, kind="lat"):
        """kinds: "lat" (the library's choice), "packed" (CONP_PATH_SOLVE_NO_LATTICE), "qinit" """
        if kind not in self.handles:
            self.handles[kind] = Handle(self, kind)
        return self.handles[kind]

    def close(self):
        for h in self.handles.values():
            h.fx.close()


class Handle:
    def __init__(self, box, kind):
        import torch
        s, self.qinit = box.s, None
        if kind == "qinit":
            s, by_tag = sr.with_electrode_charges(box.s, 77)
            self.at = dataclasses.replace(box.at, q=by_tag[box.at.tag].copy())
        else:
            self.at = dataclasses.replace(box.at, q=box.at.q.copy())
        with capi.test_paths(capi.PATH_SOLVE_NO_LATTICE if kind == "packed" else 0):
            fx = FixConp(s, extra_args=("qinit",) if kind == "qinit" else ())
            fx.init_lists(box.alist, box.blist)
            fx.setup_post_neighbor(self.at)
            fx.setup_pre_force(self.at, 0, s.potdiff)
        self.box, self.fx, self.ne = box, fx, box.ne
        assert fx.info().elenum_all == box.ne and fx.row_range() == (0, box.ne)
        m = fx.maps()
        self.ele_row = m["tag2eleall"][box.at.tag[box.ele_atoms]].astype(np.int64)
        if kind == "qinit":
            self.qinit = by_tag[m["eleall2tag"]]
            assert fx.args.qinit == 1 and np.count_nonzero(self.qinit) == box.ne
        if box.lat is None:
            by_tag_x = np.zeros((int(s.tag.max()) + 1, 3))
            by_tag_x[s.tag] = s.x
            box.lat = lr.find(by_tag_x[m["eleall2tag"]], s.prd[0], s.prd[1])          # eleall order: the library's own numbering
        self.big_b = torch.full((box.ne + 512,), float("nan"), dtype=torch.float64, device="cuda")
        self.big_q = torch.full((box.ne + 512,), float("nan"), dtype=torch.float64, device="cuda")
        fx.bind_device_buffers(self.big_b.data_ptr(), self.big_q.data_ptr())
        self.setq = fx.vectors()[2].copy()
        self.S = fx.matrix()                          # the library's own projected inverse
        self.holds = "S"
        self.d_x = torch.from_numpy(np.ascontiguousarray(self.at.x)).cuda()
        self.d_q = torch.zeros(self.at.nall, dtype=torch.float64, device="cuda")

    def use(self, tag, M=None):
        """the solve matrix: "S" (the library's own, put back as read) or a matrix of the test's under a tag of its own"""
        if self.holds != tag:
            self.fx.set_matrix(self.S if tag == "S" else M, 3)
            self.holds = tag

    def fused(self, b, dV=DV, q_before=None):
        """conp_fix_update_charge -> (y, atom charges before, atom charges after)"""
        import torch
        self.big_b[:self.ne] = torch.from_numpy(np.ascontiguousarray(b)).cuda()
        if q_before is not None:
            self.at.q[:] = q_before
        before = self.at.q.copy()
        self.fx.update_charge(self.at, dV)
        torch.cuda.synchronize()
        return self.big_q[:self.ne].cpu().numpy().copy(), before, self.at.q.copy()

    def tails_are_nan(self):
        import torch
        torch.cuda.synchronize()
        return bool(torch.isnan(self.big_b[self.ne:]).all() and torch.isnan(self.big_q[self.ne:]).all())

    def want_charges(self, y, before, dV):
        v = sr.charges(y, dV, self.setq, self.qinit)
        out = before.copy()
        out[self.box.ele_atoms] = v[self.ele_row]
        return out

    def form(self):
        return self.fx.solve_form()


@pytest.fixture(scope="module")
def boxes():
    made = {}

    def get(name, variant=None):
        key = (name, variant)
        if key not in made:
            s = lr.system(*CELLS[name])
            ele = np.nonzero(s.echeck != 0)[0]
            if variant == "moved":                       # one electrode atom off its site by ten matching tolerances
                s.x[ele[5], 0] += 1e-3
            elif variant == "rough":                     # every electrode atom its own z, as bench.py's headline_rough
                s.x[ele, 2] += np.random.default_rng(4).uniform(-0.05, 0.05, size=len(ele))
            made[key] = Box(s)
        return made[key]
    yield get
    capi.set_lat_stage(0)
    for b in made.values():
        b.close()


def _bound(box, stage_cap=0):
    lat = box.lat
    return lr.chain(lat["nx"], lat["ny"], lat["nbasis"], stage_cap)


def _assert_rows(tag, y, M, b, c, dev):
    ref, A = lr.ref_product(M, b)
    bound = c * lr.U * A + dev * np.abs(b).sum()
    frac = float(np.max(np.abs(np.asarray(y, np.longdouble) - ref).astype(np.float64) / bound))
    print(f"  {tag}: c = {c}, dev = {dev:.3g}, worst |y - ref| / bound = {frac:.3f}")
    assert np.isfinite(y).all() and frac <= 1.0, (tag, frac)


def _columns(box):
    """one j per basis atom (each in another cell), the first and the last cell of a row of cells, the last eleall index"""
    lat = box.lat
    nb, nx, ny = lat["nbasis"], lat["nx"], lat["ny"]
    js = [int(lat["row"][be, (3 * be + 1) % nx, (5 * be + 2) % ny]) for be in range(nb)]
    js += [int(lat["row"][1, nx - 1, 0]), int(lat["row"][1, nx - 1, ny - 1]), int(lat["row"][0, 0, ny - 1]), box.ne - 1]
    return sorted(set(js))


def _assert_columns(tag, h, M, js):
    for j in js:
        e = np.zeros(h.ne)
        e[j] = 1.0
        y = h.fused(e)[0]
        bad = np.nonzero(y != M[:, j])[0]
        assert bad.size == 0, (tag, j, bad[:8], y[bad[:8]], M[bad[:8], j])


@gpu
@pytest.mark.parametrize("name", list(CELLS))
def test_the_lattice_form_is_taken(boxes, name):
    box = boxes(name)
    h = box.handle()
    h.use("S")
    h.fused(np.ones(box.ne))
    f = h.form()
    cx, cy, layers = CELLS[name]
    assert (f["form"], f["nx"], f["ny"], f["nbasis"]) == ("lattice", cx, cy, 8 * layers), f
    print(f"  {name}: dev = {f['dev']:.3g}, max |S| = {f['smax']:.3g}, dev / max = {f['dev'] / f['smax']:.3g}")
    assert f["smax"] > 0 and f["dev"] <= 1e-12 * f["smax"], f"dev = {f['dev']:.3g}, max |S| = {f['smax']:.3g}"
    assert "lattice" not in h.fx.mesg_drain()
    # the table the library confirmed is the one the restated map gives: S against its own cell-(0, 0) rows
    lat = box.lat
    T = h.S[lat["row"][:, 0, 0]][:, lat["row"]]                      # [beta, beta', cx, cy]
    assert abs(np.abs(h.S - lr.circulant_matrix(lat, T)).max() - f["dev"]) <= 1e-3 * f["dev"] + 1e-300
    assert np.abs(h.S).max() == f["smax"]


@gpu
@pytest.mark.parametrize("name", list(CELLS))
def test_every_row_against_float128(boxes, name):
    box = boxes(name)
    h = box.handle()
    h.use("S")
    c = _bound(box)
    for seed in (1, 2):
        b = lr.mixed_vector(box.ne, 100 * seed + box.ne)
        y = h.fused(b)[0]
        f = h.form()
        assert f["form"] == "lattice"
        _assert_rows(f"{name} b{seed}", y, h.S, b, c, f["dev"])
    assert h.tails_are_nan()


@gpu
@pytest.mark.parametrize("name", list(CELLS))
def test_unit_vectors_give_exact_columns(boxes, name):
    """an exactly block-circulant, exactly symmetric matrix of small integers times powers of two: dev = 0, and b = e_j returns column
    j to the bit (every product is by 1 or 0, every sum has one non-zero term)"""
    box = boxes(name)
    h = box.handle()
    M = lr.circulant_matrix(box.lat, lr.circulant_table(box.lat, 11))
    assert np.array_equal(M, M.T)
    h.use("circulant", M)
    js = _columns(box)
    _assert_columns(name, h, M, js)
    f = h.form()
    assert f["form"] == "lattice" and f["dev"] == 0.0 and f["smax"] == np.abs(M).max(), f
    assert h.tails_are_nan()
    print(f"  {name}: {len(js)} columns")


@gpu
def test_several_stages(boxes):
    """C's 16 basis atoms staged three at a time (3 + 3 + 3 + 3 + 3 + 1): the accumulators carry over, the chain grows as counted"""
    box = boxes("C")
    h = box.handle()
    M = lr.circulant_matrix(box.lat, lr.circulant_table(box.lat, 12))
    capi.set_lat_stage(3)
    try:
        h.use("circulant, staged", M)
        _assert_columns("C staged", h, M, _columns(box))
        assert h.form()["form"] == "lattice"
        h.use("S")
        b = lr.mixed_vector(box.ne, 5)
        y = h.fused(b)[0]
        c = _bound(box, 3)
        assert c > _bound(box)
        _assert_rows("C staged", y, h.S, b, c, h.form()["dev"])
    finally:
        capi.set_lat_stage(0)
        h.holds = None
    h.use("S")
    y1 = h.fused(b)[0]
    _assert_rows("C, one stage again", y1, h.S, b, _bound(box), h.form()["dev"])


@gpu
@pytest.mark.parametrize("kind", ["lat", "qinit"])
def test_charge_write_bit_for_bit(boxes, kind):
    """q_ele = y + dV setq (+ qinit) to the bit, in every owned and ghost copy; every other entry of the atom array keeps its bits;
    two calls give the same bytes"""
    import torch
    box = boxes("A")
    h = box.handle(kind)
    h.use("S")
    b = lr.mixed_vector(box.ne, 9)
    junk = np.random.default_rng(7).integers(-2 ** 63, 2 ** 63 - 1, size=h.at.nall, dtype=np.int64).view(np.float64)
    y, before, after = h.fused(b, q_before=junk)
    assert h.form()["form"] == "lattice"
    want = h.want_charges(y, before, DV)
    assert np.array_equal(sr.bits(after), sr.bits(want))
    if kind == "qinit":
        assert np.any(want[box.ele_atoms] != (y + DV * h.setq)[h.ele_row])       # (qinit took part)
    y2, _, after2 = h.fused(b, q_before=junk)
    assert np.array_equal(sr.bits(y), sr.bits(y2)) and np.array_equal(sr.bits(after), sr.bits(after2))
    _assert_rows(f"A {kind}", y, h.S, b, _bound(box), h.form()["dev"])
    # the caller's device array (conp_fix_pre_force_device forms b itself): the kernel's own writes through the CSR lists
    if kind == "lat":
        q0 = box.at.q.copy()
        h.d_q.copy_(torch.from_numpy(q0).cuda())
        h.fx.pre_force_device(h.d_x.data_ptr(), h.d_q.data_ptr(), DV)
        torch.cuda.synchronize()
        yd = h.big_q[:box.ne].cpu().numpy()
        b_own = h.big_b[:box.ne].cpu().numpy()
        assert np.isfinite(b_own).all() and np.abs(b_own).max() > 0
        assert np.array_equal(sr.bits(h.d_q.cpu().numpy()), sr.bits(h.want_charges(yd, q0, DV)))
        _assert_rows("A pre_force_device (its own b)", yd, h.S, b_own, _bound(box), h.form()["dev"])
    assert h.tails_are_nan()


def _same_bytes(tag, h, p, b):
    y, _, q = h.fused(b)
    yp, _, qp = p.fused(b)
    assert np.array_equal(sr.bits(y), sr.bits(yp)), tag
    assert np.array_equal(sr.bits(q[h.box.ele_atoms]), sr.bits(qp[h.box.ele_atoms])), tag


@gpu
@pytest.mark.parametrize("variant", ["moved", "rough"])
def test_no_lattice_in_the_positions_keeps_the_packed_form(boxes, variant):
    """(a) one electrode atom moved by 1e-3 A in x, (b) electrode z jittered: the packed form, with the bytes of a handle forced to it"""
    box = boxes("A", variant)
    h, p = box.handle(), box.handle("packed")
    b = lr.mixed_vector(box.ne, 21)
    _same_bytes(variant, h, p, b)
    for x in (h, p):
        f = x.form()
        assert (f["form"], f["nx"], f["ny"], f["nbasis"]) == ("packed", 0, 0, 0), f
        assert "lattice" not in x.fx.mesg_drain()
    _assert_rows(f"A {variant}, packed", h.fused(b)[0], sr.lower_symmetrised(h.S), b, sr.packed_chain(box.ne), 0.0)


@gpu
def test_a_matrix_off_the_lattice_keeps_the_packed_form(boxes):
    """(c) conp_fix_set_matrix with a symmetric matrix that is not block-circulant: said once, packed tiles multiplied, the bytes of a
    handle forced to the packed path; a circulant matrix after it returns to the table; (d) the path bit itself"""
    box = boxes("A")
    h, p = box.handle(), box.handle("packed")
    b = lr.mixed_vector(box.ne, 22)
    h.use("S"); p.use("S")
    h.fx.mesg_drain()
    yl = h.fused(b)[0]
    yp = p.fused(b)[0]
    f = p.form()
    assert (f["form"], f["nx"], f["ny"], f["nbasis"]) == ("packed", 0, 0, 0) and h.form()["form"] == "lattice"       # (d)
    _assert_rows("A packed by the path bit", yp, sr.lower_symmetrised(p.S), b, sr.packed_chain(box.ne), 0.0)
    assert np.array_equal(sr.bits(h.S), sr.bits(p.S))
    M = sr.matrix(box.ne, 1000 + box.ne)
    h.use("general", M); p.use("general", M)
    _same_bytes("general matrix", h, p, b)
    f = h.form()
    assert (f["form"], f["nx"], f["ny"], f["nbasis"]) == ("packed", 32, 8, 8), f
    assert f["dev"] > 1e-10 * f["smax"] and f["smax"] == np.abs(M).max()
    msg = h.fx.mesg_drain()
    assert msg.count("does not follow the electrode lattice") == 1 and f"{f['dev']:.3g}" in msg and "not symmetric" not in msg
    h.fused(b)
    assert "lattice" not in h.fx.mesg_drain()                       # said once per matrix, not once per update
    _assert_rows("general matrix, packed", h.fused(b)[0], M, b, sr.packed_chain(box.ne), 0.0)
    C = lr.circulant_matrix(box.lat, lr.circulant_table(box.lat, 13))
    h.use("circulant 13", C)
    _assert_columns("after the general matrix", h, C, _columns(box)[:3])
    assert h.form()["form"] == "lattice" and "lattice" not in h.fx.mesg_drain()
    h.use("S"); p.use("S")
    assert np.array_equal(sr.bits(h.fused(b)[0]), sr.bits(yl)) and np.array_equal(sr.bits(p.fused(b)[0]), sr.bits(yp))


@gpu
def test_lattice_form_against_packed_form(boxes):
    """the library's own S on A: the two forms differ by no more than the sum of their bounds (the packed form multiplies the mirrored
    lower triangle: max |S_ij - S_ji| sum |b| on top of its chain; the charges add one rounding of y + dV setq each)"""
    box = boxes("A")
    h, p = box.handle(), box.handle("packed")
    h.use("S"); p.use("S")
    b = lr.mixed_vector(box.ne, 23)
    yl, _, ql = h.fused(b)
    yp, _, qp = p.fused(b)
    f = h.form()
    assert f["form"] == "lattice" and p.form()["form"] == "packed"
    _ref, A = lr.ref_product(h.S, b)
    sb = np.abs(b).sum()
    asym = np.abs(h.S - h.S.T).max()
    bound = (_bound(box) + sr.packed_chain(box.ne)) * lr.U * A + (f["dev"] + asym) * sb
    frac = float(np.max(np.abs(yl - yp) / bound))
    print(f"  A: worst |y_lat - y_packed| / (sum of both bounds) = {frac:.3f}; max |dy| / max |y| = {np.abs(yl - yp).max() / np.abs(yl).max():.3g}")
    assert frac <= 1.0
    ea = box.ele_atoms
    qbound = bound[h.ele_row] + 2 * lr.U * np.abs(ql[ea])
    assert np.all(np.abs(ql[ea] - qp[ea]) <= qbound)
