"""-m gpu: the once-per-run setup (a_cal -> inverse -> inv_project -> sym_pack -> solve) at production sizes.

(1) A fixed, seeded sample of entries of the A matrix -- random pairs, diagonals, the fragments that straddle tile boundaries, the
    last row and column, pairs inside the real-space cutoff, left-right pairs, the upper triangle -- against
    helpers.a_entries_from_definitions (pinned to the oracle's full matrix on the small decks by test_a_matrix_reference.py), on
    boxes that reach every A kernel with many tiles: the z-class SYRK with 2 / 4 / 8 classes, its a_wz over three kz column
    tiles, the general kernel with its four-way kz split and a_parts_sum, a ragged last tile, planar electrodes with ten
    classes on the general kernel, and the 16384-atom box (8256 tiles, K ~ 1e6).  Beside it, the k-space part of a 96-row block
    that crosses the first tile boundary against the oracle's own aaa_from_sincos_a (same operation order as the reference).
(2) The whole chain at Ne = 16384: probes through the projected inverse and the plain inverse, the projection formula, the
    symmetry and the zero row sums of S, one device-resident update through the packed symmetric solve.

Measured on an MI355X: worst of the 5237 sampled entries against the definitions, of the largest entry (bound TOL_A = 1e-11), and
the float64 floor = the oracle's k-space block against the definitions:
    box                          Ne     K        kernel    tiles  nsplit  library   floor
    headline_ffield              4096   99773    z-class 2   528    -     2.0e-15   8.1e-15
    headline_slab                4096   287162   z-class 2   528    -     2.9e-14   2.9e-14     (kzmax 342: three kz column tiles)
    ragged_2288                  2288   14499    z-class 2   171    -     2.0e-15   2.2e-15
    layers2                      8192   82547    z-class 4   2080   -     3.3e-15   8.8e-15
    layers4                      16384  81941    z-class 8   8256   -     3.5e-15   8.8e-15
    layers5                      5120   24956    general     820    4     8.2e-15   8.4e-15     (ten classes)
    headline_rough               4096   99773    general     528    4     3.8e-15   1.0e-14
    ragged_2288_rough_tall_slab  2288   113963   general     171    4     1.0e-14   2.5e-14     (kzmax 186: two kz column tiles)
    big_16384                    16384  1018594  z-class 2   8256   -     3.3e-14   3.2e-14     (bound max(10 x floor, TOL_A) = 1e-11)
Chain at Ne = 16384: probes 9.4e-15 / 1.3e-14 / 2.9e-15 (bound 1e-8, no LAPACK comparison needed), S - S^T 6.4e-16, S e 4.0e-15 of
max|S|, update 5.3e-13 (1e-11), charge sum 7.9e-12, inverse_path 1, inverse_retries 0.  Wall time of the module: 68 s."""
import time

import numpy as np
import pytest

import oracle_py
from conp_amd import FixConp, neighbor, systems
from helpers import a_entries_from_definitions
from test_gpu_parity import TOL_A, rough

pytestmark = pytest.mark.gpu

BIG = dict(n_cells_x=64, n_cells_y=32, lz=1200.0, n_elyte=262144, cutoff=12.0, accuracy_relative=1e-6, g_ewald=0.2554)
MID = dict(n_cells_x=22, n_cells_y=13, n_elyte=2048, cutoff=10.0, accuracy_relative=1e-5, g_ewald=0.30)     # 2288 = 17 x 128 + 112

# box -> (system, Ne, n_zclasses, what else must hold for the row of the table in the module docstring to be true)
BOXES = {
    "headline_ffield": (lambda: systems.synthetic_fast(), 4096, 2, {}),
    "headline_slab": (lambda: systems.synthetic_fast(mode="slab"), 4096, 2, dict(kz_col_tiles=3)),
    "ragged_2288": (lambda: systems.synthetic_fast(lz=120.0, **MID), 2288, 2, {}),
    "layers2": (lambda: systems.synthetic_fast(layers=2, n_elyte=4096), 8192, 4, {}),
    "layers4": (lambda: systems.synthetic_fast(layers=4, n_elyte=4096), 16384, 8, {}),
    # ten classes: more than the z-class kernel takes -> planar electrodes on the general kernel (16 x 8 cells keep the list small)
    "layers5": (lambda: systems.synthetic_fast(n_cells_x=16, n_cells_y=8, layers=5, n_elyte=2048), 5120, 10, dict(nsplit=4)),
    "headline_rough": (lambda: rough(systems.synthetic_fast()), 4096, 0, dict(nsplit=4, tiles=528)),
    "ragged_2288_rough_tall_slab": (lambda: rough(systems.synthetic_fast(lz=400.0, mode="slab", **MID)), 2288, 0,
                                    dict(nsplit=4, kz_col_tiles=2)),
    "big_16384": (lambda: systems.synthetic_fast(**BIG), 16384, 2, dict(tiles=8256)),
}

KZ_PER_CHUNK, CHUNKS_PER_COL_TILE = 16, 10          # a_kspace_lds_kernel: AK_TC = 32 t rows = 16 kz; ten chunks per kz column tile


def a_kspace_nsplit(ne_pad, num_cus, nchunk, nranks=1):
    """conp_kernels.hip a_kspace_nsplit restated: how many ways the general kernel splits the kz chunks of a tile"""
    nb = ne_pad // 128
    ntiles, slots = (nb * (nb + 1) // 2 + nranks - 1) // nranks, 2 * num_cus
    if ntiles >= 6 * slots or nchunk < 2:
        return 1
    return 4 if nchunk >= 4 else 2


def assert_path(info, ne, nzc, expect):
    """which A kernel ran (km_a_cal_device: 1..8 classes -> a_wz + a_kspace_zc_kernel, else a_kspace_lds_kernel (+ a_parts_sum)),
    with how many tiles and which split"""
    import torch
    assert info.elenum_all == ne and info.n_zclasses == nzc, (info.elenum_all, info.n_zclasses)
    general = not (0 < nzc <= 8)
    nb = (ne + 127) // 128
    tiles = nb * (nb + 1) // 2
    nchunk = -(-info.kzmax // KZ_PER_CHUNK)                      # chunks the sphere cut reaches (one more if kz = 0 has a row: >= 4 all the same)
    nsplit = a_kspace_nsplit(nb * 128, torch.cuda.get_device_properties(0).multi_processor_count, nchunk) if general else 0
    assert ("nsplit" in expect) == general
    if general:
        assert nsplit == expect["nsplit"] and nchunk >= 4, (nsplit, nchunk)
    if "tiles" in expect:
        assert tiles == expect["tiles"]
    if "kz_col_tiles" in expect:
        assert -(-info.kzmax // (KZ_PER_CHUNK * CHUNKS_PER_COL_TILE)) == expect["kz_col_tiles"], info.kzmax
    return ("general" if general else "z-class"), tiles, nsplit


def sample_pairs(s, xe, ech, seed=2024):
    """the sample of (i, j), the same recipe and seed for every box; xe / ech: positions and electrode sign in the permanent numbering"""
    ne = len(xe)
    rng = np.random.default_rng(seed)
    parts = {"random": rng.integers(0, ne, size=(2000, 2))}
    d = rng.choice(ne, 64, replace=False)
    parts["diagonal"] = np.stack([d, d], 1)
    last = (ne - 1) // 128                                         # 128 * last is the last tile boundary with atoms on both sides
    frag = [np.arange(128 * m - 8, min(128 * m + 8, ne)) for m in (1, max(2, last // 2), last)]
    parts["tile boundaries"] = np.concatenate([np.stack(np.meshgrid(a, b, indexing="ij"), -1).reshape(-1, 2) for a in frag for b in frag])
    other = rng.integers(0, ne, size=32)
    parts["last row and column"] = np.concatenate([[[ne - 1, ne - 1], [ne - 1, 0], [0, ne - 1], [ne - 1, ne - 2], [ne - 2, ne - 1]],
                                                   np.stack([np.full(32, ne - 1), other], 1), np.stack([other, np.full(32, ne - 1)], 1)])
    near = []
    prd = s.prd
    for i in rng.choice(ne, 48, replace=False):                   # minimum-image distances from the positions, not from a list
        dd = xe - xe[i]
        for c in range(3):
            if s.periodic[c]:
                dd[:, c] -= prd[c] * np.round(dd[:, c] / prd[c])
        r2 = (dd * dd).sum(1)
        r2[i] = np.inf
        close = np.argsort(r2)[:6]
        near += [(i, j) if k % 2 else (j, i) for k, j in enumerate(close) if r2[j] < s.cutoff ** 2]
    parts["inside the cutoff"] = np.array(near)
    left, right = np.nonzero(ech == 1)[0], np.nonzero(ech == -1)[0]
    lr = np.stack([rng.choice(left, 256), rng.choice(right, 256)], 1)
    lr[::2] = lr[::2, ::-1]
    parts["left-right"] = lr
    up = rng.integers(0, ne, size=(400, 2))
    up = np.sort(up[up[:, 0] != up[:, 1]], axis=1)[:256]
    parts["upper triangle"] = up
    assert len(parts["inside the cutoff"]) >= 200 and len(lr) >= 200 and len(up) >= 200 and len(parts["tile boundaries"]) == 9 * 256
    return parts


def electrode_geometry(fx, at):
    m = fx.maps()
    loc = {int(t): i for i, t in enumerate(at.tag[:at.nlocal])}
    rows = np.array([loc[int(t)] for t in m["eleall2tag"]])
    return m["eleall2tag"], at.x[rows].copy(), at.echeck[rows].copy()


def sym(a):
    """either orientation of a pair may carry the k-space value before fix_conp.cpp:826-831 symmetrises"""
    lo, up = np.tril(a, -1), np.triu(a, 1)
    return lo + lo.T + up + up.T + np.diag(np.diag(a))


def kspace_block(fx, s, at, kt, xe, tags, rows):
    """k-space part of the block rows x rows: the library's km_a_cal, the oracle's aaa_from_sincos_a on the electrode tables of
    fx.ele_trig(), and the definitions"""
    lib = oracle_py.load(fast=True)
    lib.orc_set_threads(16)
    a_g = fx.km_a_cal(at)
    a_g = sym(a_g[np.ix_(rows, rows)])
    c_g, s_g = fx.ele_trig()                                     # bit-exact with the oracle's own (test_full_chain_matches_oracle)
    csk, snk = np.ascontiguousarray(c_g[rows]), np.ascontiguousarray(s_g[rows])
    del c_g, s_g
    ks = oracle_py.KSpace.from_system(lib, s)
    a_o = sym(ks.aaa(csk, snk, xe[rows]))
    ks.close()
    pairs = np.stack(np.meshgrid(rows, rows, indexing="ij"), -1).reshape(-1, 2)
    a_d = a_entries_from_definitions(s, at, kt, fx.info(), pairs, eleall2tag=tags, kspace_only=True).reshape(len(rows), -1)
    return a_g, a_o, a_d


@pytest.mark.parametrize("box", list(BOXES))
def test_sampled_entries_of_a_match_the_definitions(box):
    make, ne, nzc, expect = BOXES[box]
    t0 = time.time()
    s = make()
    at, alist, blist = neighbor.build_lists(s)
    fx = FixConp(s)
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    tags, xe, ech = electrode_geometry(fx, at)
    kt = fx.ktables()
    # ---- k-space part alone, rows [96, 192): library vs the oracle's operation order vs the definitions
    rows = np.arange(96, 192)
    a_g, a_o, a_d = kspace_block(fx, s, at, kt, xe, tags, rows)
    # ---- the whole matrix
    fx.a_cal(at)
    info = fx.info()                                              # (the z classes are found when the electrode tables are made)
    kernel, tiles, nsplit = assert_path(info, ne, nzc, expect)
    A = fx.matrix()
    fx.close()
    for r0 in range(0, ne, 2048):                                                     # A == A.T without a second copy of A
        assert np.array_equal(A[r0:r0 + 2048], A[:, r0:r0 + 2048].T)
    parts = sample_pairs(s, xe, ech)
    pairs = np.concatenate(list(parts.values()))
    ref = a_entries_from_definitions(s, at, kt, info, pairs, eleall2tag=tags)
    got = A[pairs[:, 0], pairs[:, 1]]
    scale = np.abs(ref).max()
    floor = np.abs(a_o - a_d).max() / scale                                           # a faithful float64 evaluation vs the definitions
    e_block_o, e_block_d = np.abs(a_g - a_o).max() / scale, np.abs(a_g - a_d).max() / scale
    err = np.abs(got - ref) / scale
    tol = max(10 * floor, TOL_A) if box == "big_16384" else TOL_A
    print(f"{box}: Ne {ne} K {info.kcount} kzmax {info.kzmax} nzc {nzc}: {kernel} kernel, {tiles} tiles, nsplit {nsplit}; "
          f"{len(pairs)} sampled entries: worst {err.max():.2e} of max|A| (bound {tol:.1e}); k-space block [96,192): library vs oracle "
          f"{e_block_o:.2e}, library vs definitions {e_block_d:.2e}, oracle vs definitions (floor) {floor:.2e}; {time.time() - t0:.0f} s")
    o = 0
    for name, p in parts.items():                                                     # a failure names its group and its worst entries
        e = err[o:o + len(p)]
        worst = np.argsort(e)[::-1][:8]
        assert e.max() < tol, (box, name, [(int(p[w, 0]), int(p[w, 1]), float(e[w])) for w in worst])
        o += len(p)
    assert e_block_o < tol and e_block_d < tol


# ---- the chain at Ne = 16384 ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_chain():
    s = systems.synthetic_fast(**BIG)
    at, alist, blist = neighbor.build_lists(s)
    fx = FixConp(s)
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    t0 = time.time()
    fx.linalg_setup(at)
    print(f"Ne 16384: linalg_setup {time.time() - t0:.1f} s, inverse_path {fx.info().inverse_path}, inverse_retries {fx.info().inverse_retries}")
    yield s, at, alist, blist, fx
    fx.close()


def test_big_inverse_really_inverts_and_is_projected(big_chain):
    """test_headline_inverse_really_inverts and the matrix half of test_headline_properties at Ne = 16384, same tolerances:
    S (A v) = v for zero-sum v, conp_invert(A) (A v) = v, the projection formula on the probes, S symmetric, S e = 0"""
    s, at, alist, blist, fx = big_chain
    info = fx.info()
    assert info.elenum_all == 16384 and info.inverse_path == 1
    fa = FixConp(s)
    fa.init_lists(alist, blist)
    fa.setup_post_neighbor(at)
    fa.a_cal(at)
    A = fa.matrix()
    n = A.shape[0]
    assert np.all(np.diag(A) > 0)
    rng = np.random.default_rng(11)
    V = rng.normal(size=(n, 6))
    V0 = V - V.mean(axis=0)
    AV, AV0 = A @ V, A @ V0
    inv = fa.invert(A)
    assert fa.info().inverse_path == 1
    fa.close()
    e_inv = np.abs(inv @ AV - V).max() / np.abs(V).max()
    ainve = inv.sum(axis=1)
    Sref_V = inv @ V - np.outer(ainve, ainve @ V) / ainve.sum()          # fix_conp.cpp:1011-1020 applied to the probes
    del inv
    S = fx.matrix()
    e_s = np.abs(S @ AV0 - V0).max() / np.abs(V0).max()
    e_proj = np.abs(S @ V - Sref_V).max() / np.abs(Sref_V).max()
    smax = np.abs(S).max()
    asym = max(np.abs(S[r0:r0 + 2048] - S[:, r0:r0 + 2048].T).max() for r0 in range(0, n, 2048)) / smax
    rowsum = np.abs(S.sum(axis=1)).max() / smax
    del S
    print(f"Ne 16384: S(A v0) - v0 {e_s:.2e}, inv(A v) - v {e_inv:.2e}, projection {e_proj:.2e} (bound 1e-8); "
          f"S - S^T {asym:.2e} (1e-12), S e {rowsum:.2e} (1e-9) of max|S|; inverse_retries {info.inverse_retries}")
    assert e_s < 1e-8 and e_inv < 1e-8 and e_proj < 1e-8
    assert asym <= 1e-12 and rowsum < 1e-9


def test_big_device_update_is_the_product_of_the_projected_inverse_with_b(big_chain):
    """one device-resident update at Ne = 16384 (the packed symmetric solve, 8256 tiles): the bound q equals S b + dV S d computed
    by numpy from the matrix the library hands out, and the electrode is neutral"""
    import torch
    s, at, alist, blist, fx = big_chain
    d_x = torch.from_numpy(np.ascontiguousarray(at.x)).cuda(); d_q = torch.from_numpy(at.q.copy()).cuda()
    fx.pre_force_device(d_x.data_ptr(), d_q.data_ptr(), s.potdiff)
    torch.cuda.synchronize()
    b, y, setq = fx.vectors()
    S = fx.matrix()
    want = S @ b
    del S
    e_y = np.abs(y - want).max() / np.abs(want).max()
    q = d_q.cpu().numpy()
    tags, _, _ = electrode_geometry(fx, at)
    loc = {int(t): i for i, t in enumerate(at.tag[:at.nlocal])}
    qe = np.array([q[loc[int(t)]] for t in tags])
    e_q = np.abs(qe - (want + s.potdiff * setq)).max() / np.abs(qe).max()
    print(f"Ne 16384: S b {e_y:.2e}, charges {e_q:.2e} of max (bound 1e-11); sum of the electrode charges {qe.sum():.2e}")
    assert e_y <= 1e-11 and e_q <= 1e-11
    assert abs(qe.sum()) < 1e-9
    sol = at.echeck == 0
    assert np.array_equal(q[sol], at.q[sol])
