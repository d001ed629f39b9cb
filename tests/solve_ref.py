"""Helpers of tests/test_gpu_solve_forms.py, none of which needs a GPU (tests/test_solve_ref_math.py checks them):
  * systems of any electrode count, matrices and b vectors with 128-block scales, the float128 reference product;
  * the loop structure of the solve kernels (conp_kernels.hip section 5) restated as arithmetic on n: which tier of gemv_row_dot a
    lane takes, the tile counts of the packed form, the non-temporal threshold;
  * the length of the longest chain of dependent roundings of every form -- the constant c of the entry-wise bound
    |y_i - ref_i| <= c 2^-53 sum_j |M_ij| |b_j|.  A term that passes through c roundings (1 + d_k), |d_k| <= 2^-53, is off by
    ((1 + 2^-53)^c - 1) |term| = c 2^-53 |term| (1 + O(c 2^-53)), so the sum of the terms is off by c 2^-53 sum |term|.
    Depths are propagated through the kernels' own summation trees: -1 marks an exact zero (x + 0 rounds nothing), a product of
    two doubles has depth 0 until something rounds it, and add / fma give max(depth) + 1."""

import numpy as np

SIZES = (62, 130, 450, 961, 962, 1026, 2047, 2048, 2049, 4232)
SG_T = 128                    # tile edge of the packed form
SF_R = 32                     # rows per block of sym_finish_kernel; its slot loop strides by 32 = 4 groups x 8 slots in flight
SYM_FROM = 2048               # first electrode count that takes the packed form
RESIDENT_BYTES = 64 << 20     # the rows kernels stream more than this with non-temporal loads
U = 2.0 ** -53


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------
def lane_trips(n, lane):
    """trip counts of gemv_row_dot's loops for one lane: dict(scalar, w8, w4, w1)"""
    if n & 1:
        return dict(scalar=len(range(lane, n, 64)), w8=0, w4=0, w1=0)
    h, j, w8, w4, w1 = n // 2, lane, 0, 0, 0
    while j + 448 < h:
        j += 512; w8 += 1
    while j + 192 < h:
        j += 256; w4 += 1
    while j < h:
        j += 64; w1 += 1
    return dict(scalar=0, w8=w8, w4=w4, w1=w1)


def lanes_with(n, **want):
    """the lanes whose trip counts match, e.g. lanes_with(962, w8=1)"""
    return [l for l in range(64) if all(lane_trips(n, l)[k] == v for k, v in want.items())]


def n_blocks(ne):
    return (ne + SG_T - 1) // SG_T


def last_block_rows(ne):
    return ne - (n_blocks(ne) - 1) * SG_T


def packed(ne):
    return ne >= SYM_FROM


def nontemporal(rows, ne):
    return rows * ne * 8 > RESIDENT_BYTES


def row_range(ne, rank, nranks):
    per = (ne + nranks - 1) // nranks
    r0 = min(ne, rank * per)
    return r0, min(ne, r0 + per)


def column_indices(ne):
    """the unit vectors of the exact-column test: the fixed ones and the first and last index of every row block"""
    js = {0, 63, 64, 127, 128, ne - 2, ne - 1}
    for k in range(n_blocks(ne)):
        js |= {k * SG_T, min(ne, (k + 1) * SG_T) - 1}
    return sorted(j for j in js if 0 <= j < ne)


# ---- rounding chains -----------------------------------------------------------------------------------------------------------------
def _add(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.where(a < 0, b, np.where(b < 0, a, np.maximum(a, b) + 1))


def _fma(acc):
    """fma(x, y, acc) with x y != 0: one rounding of the exact x y + acc"""
    return 1 if acc < 0 else acc + 1


def _wave(v):
    """wave_sum: v += shfl_down(v, off) for off = 32 .. 1, lane 0's result; v [..., 64]"""
    v = np.array(v)
    for off in (32, 16, 8, 4, 2, 1):
        v[..., :off] = _add(v[..., :off], v[..., off:2 * off])
    return v[..., 0]


def rows_chain(n):
    """gemv_row_dot + wave_sum (gemv_rows_kernel, gemv_finish_kernel) with every b_j != 0"""
    lanes = np.full(64, -1)
    for lane in range(64):
        t = lane_trips(n, lane)
        s = tt = -1
        for _ in range(t["scalar"]):
            s = _fma(s)
        for _ in range(4 * t["w8"] + 2 * t["w4"]):          # s and t take turns: 4 fmas each per 8-wide trip, 2 per 4-wide trip
            s, tt = _fma(s), _fma(tt)
        for _ in range(t["w1"]):
            s = _fma(s)
        s = _add(s, tt)                                      # s0 += t0 (and s1 += t1, the same depth)
        lanes[lane] = _add(s, s) if (n & 1) == 0 and s >= 0 else s      # s0 + s1; odd n: s1 stays 0.0
    return int(_wave(lanes))


def packed_chain(ne):
    """sym_gemv_kernel + sym_finish_kernel, tiles taken as full (a padded row or column only replaces roundings by exact steps).
    A slot kb <= bi of row block bi is a direct product: x * b0 rounded, fma of y * b1 onto it, six butterfly adds = 8.  A slot
    kb > bi is a transposed one: 32 fmas down the wavefront's rows, then (tr0 + tr1) + (tr2 + tr3) = 34.  The finishing thread g
    adds its slots g, g + 4, ... in order, the first onto 0.0, and the four threads of a row are combined as (p0 + p1) + (p2 + p3)."""
    nb = n_blocks(ne)
    worst = 0
    for bi in range(nb):
        parts = []
        for g in range(4):
            s = -1
            for kb in range(g, nb, 4):
                s = int(_add(s, 8 if kb <= bi else 34))
            parts.append(s)
        worst = max(worst, int(_add(_add(parts[0], parts[1]), _add(parts[2], parts[3]))))
    return worst


def left_chain_1024(mask):
    """left_sum_kernel / results_out_kernel: thread t adds v[t], v[t + 1024], ... of the group-1 rows, wave_sum, then the 16
    wavefront sums one after the other onto 0.0"""
    mask = np.asarray(mask, bool)
    d = np.full(1024, -1)
    for k in range(0, len(mask), 1024):
        term = np.full(1024, -1)
        term[:len(mask[k:k + 1024])] = np.where(mask[k:k + 1024], 0, -1)
        d = _add(d, term)
    red = _wave(d.reshape(16, 64))
    tot = -1
    for k in range(16):
        tot = int(_add(tot, red[k]))
    return tot


def left_chain_4096(mask):
    """the last block of charge_finish_kernel: 16 accumulators per thread over rounds of 4096, combined 16 -> 4 -> 1 pairwise,
    wave_sum, (red0 + red1) + (red2 + red3)"""
    mask = np.asarray(mask, bool)
    s16 = np.full((16, 256), -1)
    for k in range(0, len(mask), 4096):
        term = np.full(4096, -1)
        term[:len(mask[k:k + 4096])] = np.where(mask[k:k + 4096], 0, -1)
        s16 = _add(s16, term.reshape(16, 256))
    s4 = [_add(_add(s16[u], s16[u + 4]), _add(s16[u + 8], s16[u + 12])) for u in range(4)]
    s = _add(_add(s4[0], s4[1]), _add(s4[2], s4[3]))
    red = _wave(s.reshape(4, 64))
    return int(_add(_add(red[0], red[1]), _add(red[2], red[3])))


ROWS_CHAIN = {62: 7, 130: 9, 450: 10, 961: 22, 962: 13, 1026: 13, 2047: 38, 2048: 16, 2049: 39, 4232: 26}
PACKED_CHAIN = {2048: 39, 2049: 40, 4232: 44}


def check_sizes():
    """what each of SIZES is there for, asserted from the restated loop bounds and thresholds"""
    every = list(range(64))
    assert lanes_with(62, w1=1, w4=0, w8=0) == every[:31] and lanes_with(62, w1=0, w4=0, w8=0) == every[31:]      # lanes without an element
    assert lanes_with(130, w1=2) == [0] and lanes_with(130, w1=1, w4=0, w8=0) == every[1:]            # lane 0 alone steps twice
    assert lanes_with(450, w4=1, w8=0) == every[:33] and lanes_with(450, w4=0, w8=0) == every[33:]
    assert [lane_trips(961, l)["scalar"] for l in (0, 1, 63)] == [16, 15, 15] and lanes_with(961, w8=0, w4=0, w1=0) == every
    assert lanes_with(962, w8=1, w4=0) == every[:33] and lanes_with(962, w8=0, w4=1) == every[33:]
    assert lanes_with(1026, w8=1, w4=0) == every and lanes_with(1026, w1=1) == [0] and lanes_with(1026, w1=0) == every[1:]
    assert not packed(2047) and 2047 & 1 and lane_trips(2047, 0)["scalar"] == 32
    assert packed(2048) and (n_blocks(2048), last_block_rows(2048)) == (16, 128)                    # every tile full
    assert packed(2049) and (n_blocks(2049), last_block_rows(2049)) == (17, 1) and 2049 & 1           # one row in the last block
    assert (n_blocks(4232), last_block_rows(4232)) == (34, 8)
    assert len(range(0, 34, 4)) == 9 > SF_R // 4 >= len(range(0, n_blocks(4096), 4))                  # a second pass of the slot loop
    assert 4232 > 4096 >= 2049                                                                          # a second round of the 4096-stride sum
    assert nontemporal(4232, 4232) and not nontemporal(2049, 2049) and not nontemporal(4096, 2048)      # 143 MB / 34 MB against 64 MiB
    assert row_range(4232, 2, 3) == (2822, 4232) and not nontemporal(1411, 4232)                        # a shard of three stays resident
    assert row_range(961, 0, 3) == (0, 321) and row_range(961, 2, 3) == (642, 961) and row_range(130, 63, 64) == (130, 130)
    assert {n: rows_chain(n) for n in SIZES} == ROWS_CHAIN
    assert {n: packed_chain(n) for n in SIZES if packed(n)} == PACKED_CHAIN


# ---- systems -------------------------------------------------------------------------------------------------------------------------
def cells_for(ne):
    """(nx, ny, k): a sheet of 4 nx ny atoms per electrode, 8 nx ny >= ne, from which k atoms are taken out; at most 64 spare
    atoms, the box at least 4 x 2 cells, as square as that allows"""
    a, b = 32.2 / 13.0, 34.4 / 8.0
    best = None
    for nx in range(4, 80):
        for ny in range(2, 80):
            k = 8 * nx * ny - ne
            if 0 <= k <= 64:
                key = (abs(nx * a - ny * b), k)
                if best is None or key < best[0]:
                    best = (key, (nx, ny, k))
    return best[1]


def system(ne):
    """synthetic_fast with exactly `ne` electrode atoms: the last k // 2 atoms of the first sheet and the last k - k // 2 of the second
    leave the electrode groups (echeck 0, charge 0, a non-electrode type).  Group 1 is the SECOND sheet here, so that the rows the
    fix scalar sums are the last ones -- the ones beyond index 4096 at the largest size."""
    from conp_amd import systems
    nx, ny, k = cells_for(ne)
    s = systems.synthetic_fast(n_cells_x=nx, n_cells_y=ny, lz=120.0, n_elyte=256, cutoff=10.0, accuracy_relative=1e-4, g_ewald=0.30)
    s.echeck = -s.echeck
    first, second = np.nonzero(s.echeck == -1)[0], np.nonzero(s.echeck == 1)[0]
    out = np.concatenate([first[len(first) - k // 2:], second[len(second) - (k - k // 2):]])
    s.echeck[out] = 0
    s.q[out] = 0.0
    s.type[out] = 4
    assert int(np.count_nonzero(s.echeck)) == ne
    return s


def with_electrode_charges(s, seed):
    """a copy whose electrode atoms carry charges (what the `qinit` keyword keeps adding); -> (system, charges by tag)"""
    s2 = s.copy()
    rng = np.random.default_rng(seed)
    ele = s2.echeck != 0
    s2.q[ele] = 0.01 * rng.standard_normal(int(ele.sum()))
    by_tag = np.zeros(int(s2.tag.max()) + 1)
    by_tag[s2.tag] = s2.q
    return s2, by_tag


# ---- matrices and vectors ------------------------------------------------------------------------------------------------------------
def block_scales(ne, rng, decades=3.0):
    """one scale per 128-block, +-10^u with u uniform in [-decades, decades]: [ne]"""
    nb = n_blocks(ne)
    sc = rng.choice([-1.0, 1.0], size=nb) * 10.0 ** rng.uniform(-decades, decades, size=nb)
    return np.repeat(sc, SG_T)[:ne]


def matrix(ne, seed):
    """R + R.T with R_ij = g_ij r_i c_j, r and c block scales: exactly symmetric, every 128 x 128 tile of its own magnitude and sign"""
    rng = np.random.default_rng(seed)
    R = rng.standard_normal((ne, ne))
    R *= block_scales(ne, rng)[:, None]
    R *= block_scales(ne, rng)[None, :]
    return np.ascontiguousarray(R + R.T)


def vectors(ne, seed):
    """the b vectors of the entry-wise bound: two block-scaled random ones and all ones -> dict name -> [ne]"""
    rng = np.random.default_rng(seed)
    return {"scaled0": rng.standard_normal(ne) * block_scales(ne, rng), "scaled1": rng.standard_normal(ne) * block_scales(ne, rng),
            "ones": np.ones(ne)}


def ref_product(M, b, chunk=256):
    """(M b in float128, A_i = sum_j |M_ij| |b_j| in float64).  x86 long double has a 64-bit mantissa: a product of two doubles is
    rounded once (2^-64), numpy sums a row pairwise (about log2(n) further roundings): < 0.01 * 2^-53 * A_i, against c >= 7."""
    assert np.finfo(np.longdouble).nmant >= 63, "no extended precision on this platform"
    n = M.shape[0]
    bl = np.asarray(b, np.longdouble)
    ref, A = np.zeros(n, np.longdouble), np.zeros(n)
    for r in range(0, n, chunk):
        P = M[r:r + chunk].astype(np.longdouble) * bl
        ref[r:r + chunk] = P.sum(axis=1)
        A[r:r + chunk] = np.abs(P).sum(axis=1).astype(np.float64)
    return ref, A


def worst_fraction(y, ref, A, c):
    """max_i |y_i - ref_i| / (c 2^-53 A_i): the bound holds when this is <= 1"""
    err = np.abs(np.asarray(y, np.longdouble) - ref).astype(np.float64)
    return float(np.max(err / (c * U * A)))


def lower_symmetrised(M):
    """what the packed form multiplies with: the lower triangle mirrored"""
    L = np.tril(M)
    return L + np.tril(M, -1).T


def charges(y, dV, setq, qinit=None):
    """the float64 value the charge write stores: products and sums are uncontracted on the device, so numpy gives the same bits"""
    v = y + dV * setq
    return v if qinit is None else v + qinit


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
