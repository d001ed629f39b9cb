"""no GPU needed: the helpers of tests/test_gpu_solve_forms.py (tests/solve_ref.py) -- the sizes and what each reaches, the constants
restated from the kernels against the kernel source, the rounding-chain counts on hand-made cases, the systems, matrices and the
float128 reference."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import solve_ref as sr
from conp_amd import neighbor

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lammps-user-conp2_amd", "csrc")


def test_sizes_reach_what_they_are_for():
    sr.check_sizes()


def test_restated_constants_are_the_kernels():
    """solve_ref restates loop bounds and thresholds of conp_kernels.hip / conp_fix.cpp: whoever changes one there is sent here"""
    k = open(os.path.join(CSRC, "conp_kernels.hip")).read()
    f = open(os.path.join(CSRC, "conp_fix.cpp")).read()
    dot = k[k.index("double gemv_row_dot("):k.index("void gemv_rows_kernel(")]
    assert re.findall(r"for \(; (j(?: \+ \d+)?) < n / 2; j \+= (\d+)\)", dot) == [("j + 448", "512"), ("j + 192", "256"), ("j", "64")]
    assert "for (int j = lane; j < n; j += 64) s0 = fma(srow[j], b[j], s0);" in dot and "if ((n & 1) == 0)" in dot
    assert "constexpr size_t GEMV_RESIDENT_BYTES = (size_t)64 << 20;" in k and "return matrix_bytes > GEMV_RESIDENT_BYTES;" in k
    assert f"constexpr int SG_T = {sr.SG_T};" in k and f"constexpr int SF_R = {sr.SF_R};" in k
    fin = k[k.index("void sym_finish_kernel("):k.index("size_t sym_packed_doubles(")]
    assert "for (int kb = g; kb < nb; kb += 32)" in fin and "kb + 4 * u < nb" in fin and "for (int u = 0; u < 8; ++u) s += w[u];" in fin
    assert "(part[0][rl] + part[1][rl]) + (part[2][rl] + part[3][rl])" in fin
    assert "for (int i0 = threadIdx.x; i0 < ne; i0 += 4096)" in k
    assert "for (int i = threadIdx.x; i < ne; i += 1024) if (elecheck[i] == 1) s += v[i];" in k
    assert f"return !gemv_rows && idx.elenum_all >= {sr.SYM_FROM};" in f and "spk_symmetric = md <= 1e-10 * mx;" in f
    assert "rows_per = (ne + env.nranks - 1) / env.nranks;" in f


def test_chain_arithmetic():
    assert int(sr._add(-1, 5)) == 5 and int(sr._add(5, -1)) == 5 and int(sr._add(2, 5)) == 6 and int(sr._add(-1, -1)) == -1
    assert sr._fma(-1) == 1 and sr._fma(3) == 4
    lanes = np.full(64, -1); lanes[0] = 2
    assert int(sr._wave(lanes)) == 2                                    # 63 exact zeros
    assert int(sr._wave(np.zeros(64, int))) == 6
    lanes = np.full(64, -1); lanes[:31] = 0
    assert int(sr._wave(lanes)) == 5
    every = np.ones(4232, bool)
    assert sr.left_chain_1024(every) == (5 - 1) + 6 + 15                # five terms per thread, the wave, sixteen sums in sequence
    assert sr.left_chain_4096(every) == 1 + 2 + 2 + 6 + 2               # a second round, 16 -> 4 -> 1, the wave, four sums pairwise
    assert sr.left_chain_4096(np.ones(4096, bool)) == 2 + 2 + 6 + 2
    one = np.zeros(500, bool); one[77] = True
    assert sr.left_chain_1024(one) == 0 == sr.left_chain_4096(one)      # one term: nothing rounds
    assert sr.rows_chain(64) == 1 + 1 + 5 and sr.rows_chain(63) == 1 + 6 and sr.rows_chain(2) == 2


def test_systems_have_the_electrode_count_and_group_1_last():
    for ne in sr.SIZES:
        s = sr.system(ne)
        ele = s.echeck != 0
        assert ele.sum() == ne and np.all(s.type[ele] == 5) and np.all(s.type[~ele] != 5) and np.all(s.q[ele] == 0)
        rows = s.echeck[ele]                                            # electrode rows in atom order
        assert abs(int((rows == 1).sum()) - int((rows == -1).sum())) <= 1
        assert np.all(np.diff((rows == 1).astype(int)) >= 0)            # group 1 is the tail
        if ne == 4232:
            assert np.nonzero(rows == 1)[0].max() >= 4096               # the second round of the 4096-stride sum adds something
    s = sr.system(961)
    at, alist, blist = neighbor.build_lists(s)
    assert np.count_nonzero(at.echeck[at.nlocal:]) > 1500 and alist.inum == 961
    s2, by_tag = sr.with_electrode_charges(s, 5)
    assert np.count_nonzero(s2.q[s2.echeck != 0]) == 961 and np.array_equal(by_tag[s2.tag], s2.q) and np.all(s.q[s.echeck != 0] == 0)


def test_matrix_and_vectors():
    ne = 450
    M = sr.matrix(ne, 3)
    assert np.array_equal(M, M.T) and np.isfinite(M).all()
    tile = np.array([[np.abs(M[i:i + 128, j:j + 128]).max() for j in range(0, ne, 128)] for i in range(0, ne, 128)])
    assert tile.max() / tile.min() > 1e3                                # tiles differ by decades
    assert (M > 0).any() and (M < 0).any()
    assert not np.array_equal(sr.matrix(ne, 4), M)
    v = sr.vectors(ne, 9)
    assert set(v) == {"scaled0", "scaled1", "ones"} and np.all(v["ones"] == 1.0) and not np.array_equal(v["scaled0"], v["scaled1"])
    blocks = [np.abs(v["scaled0"][i:i + 128]).max() for i in range(0, ne, 128)]
    assert max(blocks) / min(blocks) > 10
    assert sr.column_indices(300) == [0, 63, 64, 127, 128, 255, 256, 298, 299]
    assert sr.column_indices(62) == [0, 60, 61]
    U3 = np.arange(9.0).reshape(3, 3)
    assert np.array_equal(sr.lower_symmetrised(U3), [[0, 3, 6], [3, 4, 7], [6, 7, 8]])


def test_reference_product_and_bound():
    rng = np.random.default_rng(2)
    n = 40
    M, b = sr.matrix(n, 6), rng.standard_normal(n)
    ref, A = sr.ref_product(M, b, chunk=16)
    for i in (0, 17, 39):
        exact = sum(Fraction(float(M[i, j])) * Fraction(float(b[j])) for j in range(n))
        a = sum(abs(Fraction(float(M[i, j])) * Fraction(float(b[j]))) for j in range(n))
        hi = float(ref[i])
        got = Fraction(hi) + Fraction(float(ref[i] - np.longdouble(hi)))          # the extended value, exactly
        assert abs(got - exact) <= Fraction(1, 2 ** 60) * a          # float128 reference: far below 2^-53 A
        assert abs(Fraction(float(A[i])) - a) <= Fraction(1, 2 ** 45) * a
    y = M @ b
    assert sr.worst_fraction(y, ref, A, n) <= 1.0                       # any float64 order of n terms stays inside n 2^-53 A
    y2 = y.copy(); y2[5] += 64 * n * sr.U * A[5]
    assert sr.worst_fraction(y2, ref, A, n) > 1.0
    # a wrong SMALL component: invisible to a max-norm bound, caught by the entry-wise one
    k = int(np.argmin(np.abs(y)))
    y3 = y.copy(); y3[k] += 0.5e-11 * np.abs(y).max()
    assert np.abs(y3 - y).max() <= 1e-11 * np.abs(y).max() and sr.worst_fraction(y3, ref, A, n) > 1.0


def test_charges_and_bits():
    y, sq, qi = np.array([0.1, -3.0]), np.array([0.7, 1e-3]), np.array([1e-17, 2.0])
    assert np.array_equal(sr.charges(y, 1.7, sq), y + 1.7 * sq)
    assert np.array_equal(sr.charges(y, 1.7, sq, qi), (y + 1.7 * sq) + qi)
    assert sr.bits(np.array([0.0]))[0] != sr.bits(np.array([-0.0]))[0]
    nan = np.array([np.nan])
    assert np.array_equal(sr.bits(nan), sr.bits(nan.copy()))
