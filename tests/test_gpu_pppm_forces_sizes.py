"""-m gpu: conp_pppm_compute_forces over the kernel table of DESIGN.md section 8 -- the transforms are picked by mesh size, as
tests/test_gpu_pppm_sizes.py covers for b: a plane-path mesh, a line-path mesh beyond the LDS plane limit, meshes with one length
that is not 2,3,5-smooth (plain DFT, stand-alone k-space launch on un-fused transforms), an even and an odd length on every axis (the
Nyquist planes of the packed gradient spectra), stencil orders 2-7, atoms outside the box, and the headline box on its mesh.
Everything against the numpy mesh reference (tests/pppm_force_ref.py) with the bounds of tests/test_gpu_pppm_forces.py: forces 1e-10
max|f|; energy, virial, per-atom energies 1e-11 of the unsubtracted scale.  The electrode charges are seeded, not solved (a net
charge: the Q terms count)."""
import numpy as np
import pytest

from conp_amd import systems
from helpers import push_outside
from test_gpu_pppm_forces import check_against_reference
from test_gpu_pppm_sizes import PLANE_LDS_MAX, _charge_electrodes, _handle, plane_lds, radices

pytestmark = pytest.mark.gpu


def axes_of(mesh):
    """the transforms of conp_pppm_compute_forces (dft3_complex): x and y of a z-plane in one workgroup whenever both are smooth and
    the plane fits (whatever z is), else per axis; the radix kernel for a smooth length, the plain DFT otherwise"""
    nx, ny, nz = mesh
    planes = bool(radices(nx)) and bool(radices(ny)) and plane_lds(nx, ny) <= PLANE_LDS_MAX
    return tuple("plane" if planes and c < 2 else ("fft" if radices(n) else "dft") for c, n in enumerate(mesh))


def _run(oracle, s, mesh, order, tag, targets=None, prepare=None):
    at, fx = _handle(s, mesh, order)
    _charge_electrodes(at)
    if prepare:
        prepare(s, at)
    check_against_reference(tag, oracle, s, at, fx, mesh, order, targets)
    fx.close()
    return at


@pytest.mark.parametrize("mesh,order,axes", [
    ((27, 24, 144), 5, ("plane", "plane", "fft")),       # x odd, y even, z even
    ((32, 25, 135), 5, ("plane", "plane", "fft")),       # x even, y odd, z odd
    ((24, 27, 150), 4, ("plane", "plane", "fft")),       # even order on the other parities
    ((27, 24, 154), 5, ("plane", "plane", "dft")),       # 154 = 2 7 11: plain DFT along z (even)
    ((27, 22, 144), 5, ("fft", "dft", "fft")),           # 22 = 2 11 along y (even)
    ((28, 24, 143), 5, ("dft", "fft", "dft")),           # 28 = 4 7 along x (even: real input through the plain DFT), 143 = 11 13 (odd)
])
def test_transform_paths_and_nyquist_planes(oracle, mesh, order, axes):
    s = systems.deck("dilute", "ffield", etypes=True)
    assert axes_of(mesh) == axes
    _run(oracle, s, mesh, order, "dilute %dx%dx%d order %d" % (*mesh, order))


def test_line_path_beyond_the_lds_plane_limit(oracle):
    """81 x 50: the first plane pppm_fft_xy_kernel does not take (131696 bytes): x, y and z through pppm_fft_kernel, one launch each"""
    s = systems.synthetic_fast(n_cells_x=16, n_cells_y=8, lz=120.0, n_elyte=4096)
    mesh = (81, 50, 120)
    assert plane_lds(81, 50) > PLANE_LDS_MAX and axes_of(mesh) == ("fft", "fft", "fft")
    _run(oracle, s, mesh, 5, "boundary 81x50x120")


@pytest.mark.parametrize("order", [2, 3, 4, 5, 6, 7])
def test_stencil_orders(oracle, order):
    s = systems.deck("dilute", "ffield", etypes=True)
    _run(oracle, s, (27, 24, 144), order, f"dilute order {order}")


def test_slab_geometry_with_seeded_charges(oracle):
    s = systems.deck("dilute", "slab", etypes=True)
    _run(oracle, s, (27, 24, 432), 5, "dilute slab, net charge")


def test_atoms_outside_the_box_and_on_its_upper_face(oracle):
    """a dozen electrolyte atoms up to 1 A outside in x, y and z, unwrapped, and one exactly on boxhi in each direction: the gather
    wraps its stencil like the spread"""
    s = systems.deck("dilute", "ffield", etypes=True)
    moved = []

    def prepare(s, at):
        moved.extend(push_outside(s, at))
    at = _run(oracle, s, (27, 24, 144), 5, "dilute outside", prepare=prepare)
    n = at.nlocal
    assert len(moved) == 15 and (np.any(at.x[:n] > s.boxhi, axis=1) | np.any(at.x[:n] < s.boxlo, axis=1)).sum() == 12


def test_headline_box(oracle):
    """4096 electrode / 32768 electrolyte atoms on 72 x 64 x 540, order 5 (the line path; 16 spreading passes): forces and per-atom
    energies of 256 electrode and 256 electrolyte atoms, E and W; the library computes all 36 864 atoms in the call"""
    s = systems.synthetic_fast()
    mesh, order = (72, 64, 540), 5
    at, fx = _handle(s, mesh, order)
    _charge_electrodes(at)
    n = at.nlocal
    assert axes_of(mesh) == ("fft", "fft", "fft")
    rng = np.random.default_rng(3)
    ele = np.nonzero(at.echeck[:n] != 0)[0]
    ely = np.nonzero((at.echeck[:n] == 0) & (at.q[:n] != 0))[0]
    tg = np.concatenate([rng.choice(ele, 256, replace=False), rng.choice(ely, 256, replace=False)])
    check_against_reference("headline 72x64x540", oracle, s, at, fx, mesh, order, tg)
    fx.close()
