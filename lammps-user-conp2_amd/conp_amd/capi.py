"""ctypes binding of include/conp_hip.h and a thin driver that calls the hooks in the order LAMMPS does."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

from . import systems as _systems

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class ConpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[conp status {code}] {msg}")
        self.code = code
        self.msg = msg


def library_path():
    return os.environ.get("CONP_LIB") or os.path.join(HERE, "libconp_hip.so")


class conp_fix_args(C.Structure):
    _fields_ = [("everynum", C.c_int), ("eta", C.c_double), ("potdiff", C.c_double), ("potdiff_is_variable", C.c_int),
                ("ff_flag", C.c_int), ("zneutr", C.c_int), ("matout", C.c_int), ("pppm", C.c_int), ("split", C.c_int),
                ("qinit", C.c_int), ("lowmem", C.c_int), ("nullneutral", C.c_int), ("ehgo", C.c_int),
                ("a_matrix_f", C.c_int), ("a_matrix_file", C.c_char * 512), ("smartlist", C.c_int),
                ("eletypenum", C.c_int), ("eletypes", C.c_int * 32), ("minimizer", C.c_int), ("maxiter", C.c_int),
                ("tolerance", C.c_double), ("logfile", C.c_char * 512), ("group2", C.c_char * 128), ("potdiff_var", C.c_char * 128), ("conq", C.c_int), ("cond", C.c_int)]


class conp_env(C.Structure):
    _fields_ = [("qqrd2e", C.c_double), ("qqr2e", C.c_double), ("qe2f", C.c_double), ("dielectric", C.c_double),
                ("newton_pair", C.c_int), ("g_ewald", C.c_double), ("accuracy", C.c_double),
                ("slab_volfactor", C.c_double), ("slabflag", C.c_int), ("xprd", C.c_double), ("yprd", C.c_double),
                ("zprd", C.c_double), ("boxlo_z", C.c_double), ("boxlo_x", C.c_double), ("boxlo_y", C.c_double), ("ntypes", C.c_int), ("cutsq", C.POINTER(C.c_double)),
                ("cut_coul", C.c_double), ("one_electrode", C.c_int), ("device", C.c_int), ("rank", C.c_int),
                ("nranks", C.c_int), ("pppm_nx", C.c_int), ("pppm_ny", C.c_int), ("pppm_nz", C.c_int), ("pppm_order", C.c_int),
                ("ghost_images", C.c_int)]


class conp_atoms(C.Structure):
    _fields_ = [("nlocal", C.c_int), ("nghost", C.c_int), ("x", C.POINTER(C.c_double)), ("q", C.POINTER(C.c_double)),
                ("type", C.POINTER(C.c_int)), ("tag", C.POINTER(C.c_int)), ("echeck", C.POINTER(C.c_int))]


class conp_neighlist(C.Structure):
    _fields_ = [("inum", C.c_int), ("ilist", C.POINTER(C.c_int)), ("numneigh", C.POINTER(C.c_int)),
                ("first", C.POINTER(C.c_int)), ("neigh", C.POINTER(C.c_int)), ("nneigh", C.c_int64)]


_CB_SUM = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int64)
_CB_MAXI = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_int)
_CB_GATHER_INT = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int))
_CB_GATHERV = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64))


class conp_comm(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("rank", C.c_int), ("nranks", C.c_int), ("allreduce_sum", _CB_SUM),
                ("allreduce_max_int", _CB_MAXI), ("allgather_int", _CB_GATHER_INT), ("allgatherv", _CB_GATHERV)]


class conp_potential_args(C.Structure):
    _fields_ = [("pairflag", C.c_int), ("kspaceflag", C.c_int), ("qsumflag", C.c_int), ("eta", C.c_double)]


class conp_pair_params(C.Structure):
    _fields_ = [("ntypes", C.c_int), ("cutsq", C.POINTER(C.c_double)), ("cut_coul", C.c_double),
                ("cut_ljsq", C.POINTER(C.c_double)), ("lj1", C.POINTER(C.c_double)), ("lj2", C.POINTER(C.c_double)),
                ("lj3", C.POINTER(C.c_double)), ("lj4", C.POINTER(C.c_double)), ("offset", C.POINTER(C.c_double)),
                ("special_lj", C.c_double * 4), ("special_coul", C.c_double * 4)]


class conp_pair_build_args(C.Structure):
    _fields_ = [("nlocal", C.c_int), ("nall", C.c_int), ("cutneigh", C.c_double), ("d_tag", C.c_void_p), ("d_nspecial", C.c_void_p),
                ("d_special", C.c_void_p), ("maxspecial", C.c_int), ("prd_half", C.c_double * 3)]


class conp_ghost_build_args(C.Structure):
    _fields_ = [("nlocal", C.c_int), ("boxlo", C.c_double * 3), ("boxhi", C.c_double * 3), ("periodic", C.c_int * 3),
                ("cutghost", C.c_double)]


class conp_bonded_params(C.Structure):
    _fields_ = [("nbondtypes", C.c_int), ("nangletypes", C.c_int), ("bond_k", C.POINTER(C.c_double)), ("bond_r0", C.POINTER(C.c_double)),
                ("angle_k", C.POINTER(C.c_double)), ("angle_theta0", C.POINTER(C.c_double)), ("newton_bond", C.c_int)]


class conp_integrate_params(C.Structure):
    _fields_ = [("nlocal", C.c_int), ("ntypes", C.c_int), ("ngroups", C.c_int), ("type", C.POINTER(C.c_int)), ("group", C.POINTER(C.c_int)),
                ("mass", C.POINTER(C.c_double)), ("style", C.POINTER(C.c_int)), ("dof", C.POINTER(C.c_double)),
                ("t_period", C.POINTER(C.c_double)), ("dt", C.c_double), ("ftm2v", C.c_double), ("mvv2e", C.c_double), ("boltz", C.c_double)]


class conp_shake_params(C.Structure):
    _fields_ = [("nlocal", C.c_int), ("ntypes", C.c_int), ("type", C.POINTER(C.c_int)), ("mass", C.POINTER(C.c_double)),
                ("nbondtypes", C.c_int), ("nangletypes", C.c_int), ("bond_distance", C.POINTER(C.c_double)),
                ("angle_distance", C.POINTER(C.c_double)), ("ncluster", C.c_int), ("cluster", C.POINTER(C.c_int)),
                ("tolerance", C.c_double), ("max_iter", C.c_int), ("dt", C.c_double), ("ftm2v", C.c_double), ("prd", C.c_double * 3)]


OBSERVE_MAX_GROUPS, OBSERVE_W = 16, 10      # CONP_OBSERVE_MAX_GROUPS, CONP_OBSERVE_W


class conp_efield_params(C.Structure):
    _fields_ = [("nlocal", C.c_int), ("sel", C.POINTER(C.c_int)), ("qe2f", C.c_double), ("prd", C.c_double * 3)]


class conp_observe_params(C.Structure):
    _fields_ = [("nlocal", C.c_int), ("ntypes", C.c_int), ("ngroups", C.c_int), ("type", C.POINTER(C.c_int)),
                ("mask", C.POINTER(C.c_int)), ("mass", C.POINTER(C.c_double)), ("prd", C.c_double * 3)]


class conp_pair_exclusions(C.Structure):
    _fields_ = [("ntypes", C.c_int), ("ntype_pairs", C.c_int), ("type_i", C.POINTER(C.c_int)), ("type_j", C.POINTER(C.c_int)),
                ("ngroup_pairs", C.c_int), ("group_bit1", C.POINTER(C.c_int)), ("group_bit2", C.POINTER(C.c_int)),
                ("nmol", C.c_int), ("mol_bit", C.POINTER(C.c_int)), ("mol_intra", C.POINTER(C.c_int))]


class conp_pair_exclude_atoms(C.Structure):
    _fields_ = [("d_type", C.c_void_p), ("d_mask", C.c_void_p), ("d_molecule", C.c_void_p)]


class conp_zmirror_params(C.Structure):
    _fields_ = [("nlocal", C.c_int), ("tag", C.POINTER(C.c_int)), ("mask", C.POINTER(C.c_int)), ("groupbit", C.c_int),
                ("jgroupbit", C.c_int), ("nevery", C.c_int), ("boxlo_z", C.c_double), ("zprd", C.c_double)]


def shake_angle_distance(d1, d2, theta0_rad):
    """the 1-2 distance `fix shake` constrains for an angle type: sqrt(d1^2 + d2^2 - 2 d1 d2 cos(theta0)), the two bond lengths and
    the angle's theta0 in radians -> conp_shake_params.angle_distance"""
    return float(np.sqrt(d1 * d1 + d2 * d2 - 2.0 * d1 * d2 * np.cos(theta0_rad)))


class conp_bonded_lists(C.Structure):
    _fields_ = [("nlocal", C.c_int), ("nall", C.c_int), ("nbond", C.c_int), ("bond", C.POINTER(C.c_int)), ("nangle", C.c_int),
                ("angle", C.POINTER(C.c_int)), ("prd", C.c_double * 3)]


class conp_dihedral_params(C.Structure):
    _fields_ = [("dihedral_style", C.c_int), ("ndihedraltypes", C.c_int), ("dihedral_coef", C.POINTER(C.c_double)),
                ("improper_style", C.c_int), ("nimpropertypes", C.c_int), ("improper_coef", C.POINTER(C.c_double)),
                ("newton_bond", C.c_int)]


class conp_dihedral_lists(C.Structure):
    _fields_ = [("nlocal", C.c_int), ("nall", C.c_int), ("ndihedral", C.c_int), ("dihedral", C.POINTER(C.c_int)),
                ("nimproper", C.c_int), ("improper", C.POINTER(C.c_int)), ("prd", C.c_double * 3)]


class conp_info(C.Structure):
    _fields_ = [("elenum", C.c_int), ("elenum_all", C.c_int), ("elytenum", C.c_int), ("maxtag_all", C.c_int),
                ("runstage", C.c_int), ("kcount", C.c_int), ("kcount_flat", C.c_int), ("kcount_expand", C.c_int),
                ("kxmax", C.c_int), ("kymax", C.c_int), ("kzmax", C.c_int), ("kmax", C.c_int), ("kmax3d", C.c_int),
                ("kcount_dims", C.c_int * 7), ("cg_iterations", C.c_int), ("n_zclasses", C.c_int), ("unitk", C.c_double * 3),
                ("volume", C.c_double), ("gsqmx", C.c_double), ("ug_tot", C.c_double), ("totsetq", C.c_double),
                ("scalar_output", C.c_double), ("totinve", C.c_double), ("slabcorr", C.c_double),
                ("n_blist_pairs", C.c_int64), ("n_alist_pairs", C.c_int64), ("n_elyte_charged", C.c_int64),
                ("inverse_path", C.c_int), ("inverse_retries", C.c_int), ("pppm_elyte_spreads", C.c_int), ("zn_cols", C.c_int), ("zn_grid", C.c_int), ("zn_rows", C.c_int),
                ("zn_ranges", C.c_int), ("hc_arithmetic", C.c_int), ("zc_final", C.c_int), ("zc_row_tiles", C.c_int)]


# every symbol include/conp_hip.h declares (checked by tests/test_capi_symbols.py without a GPU)
SYMBOLS = [
    "conp_parse_fix_args", "conp_fix_create", "conp_fix_destroy", "conp_last_error", "conp_abi_version",
    "conp_fix_init_list", "conp_fix_setup_post_neighbor", "conp_fix_setup_pre_force", "conp_fix_post_neighbor",
    "conp_fix_pre_force", "conp_fix_compute_scalar", "conp_fix_post_force", "conp_fix_post_force_step", "conp_fix_modify_param", "conp_fix_linalg_setup", "conp_fix_a_cal", "conp_fix_b_cal",
    "conp_fix_equation_solve", "conp_fix_update_charge", "conp_km_conp_setup", "conp_km_a_cal", "conp_km_b_cal",
    "conp_fix_info", "conp_fix_get_ktables", "conp_fix_get_maps", "conp_fix_get_matrix", "conp_fix_set_matrix",
    "conp_fix_get_vectors", "conp_fix_get_sfac", "conp_fix_get_ele_trig", "conp_inv_project", "conp_invert",
    "conp_host_ktables", "conp_host_index", "conp_host_pair_rows", "conp_fix_write_matrix_file", "conp_fix_read_matrix_file",
    "conp_fix_set_stream",
    "conp_fix_bind_device_buffers", "conp_fix_row_range", "conp_fix_b_cal_device", "conp_fix_solve_device",
    "conp_fix_scatter_device", "conp_fix_pre_force_device", "conp_fix_profile", "conp_fix_profile_read", "conp_debug_check_guards",
    "conp_debug_set_paths", "conp_debug_set_sk_workgroups", "conp_debug_set_ew_block", "conp_debug_set_lat_stage",
    "conp_fix_get_solve_form", "conp_host_find_lattice",
    "conp_fix_pin_host_arrays", "conp_fix_unpin_host_arrays", "conp_host_alloc", "conp_host_free",
    "conp_fix_write_timing", "conp_fix_log_drain", "conp_fix_mesg_drain",
    "conp_fix_set_comm", "conp_rccl_unique_id", "conp_fix_comm_init_rccl", "conp_rccl_available", "conp_fix_comm_destroy_rccl",
    "conp_pppm_make_rho", "conp_pppm_compute_group_potential", "conp_pppm_compute_particle_potential",
    "conp_pppm_keep_density", "conp_pppm_compute",
    "conp_ewald_compute", "conp_ewald_compute_group_potential", "conp_ewald_compute_particle_potential",
    "conp_ewald_compute_forces", "conp_pppm_compute_forces",
    "conp_ewald_compute_forces_device", "conp_pppm_compute_forces_device",
    "conp_ewald_compute_forces_vatom", "conp_pppm_compute_forces_vatom",
    "conp_ewald_compute_forces_vatom_device", "conp_pppm_compute_forces_vatom_device",
    "conp_compute_potential_atom",
    "conp_pair_set_params", "conp_pair_set_list", "conp_pair_compute", "conp_pair_compute_device",
    "conp_pair_build_list_device", "conp_pair_list_moved_device", "conp_pair_get_list",
    "conp_ghost_build_device", "conp_ghost_fill_device", "conp_ghost_fill_int_device", "conp_ghost_fold_device", "conp_ghost_get",
    "conp_atoms_wrap_device",
    "conp_fix_post_neighbor_device", "conp_fix_get_step_tables",
    "conp_fix_post_force_device",
    "conp_bonded_set_params", "conp_bonded_set_lists", "conp_bonded_compute", "conp_bonded_compute_device",
    "conp_dihedral_set_params", "conp_dihedral_set_lists", "conp_dihedral_compute", "conp_dihedral_compute_device",
    "conp_integrate_set_params", "conp_integrate_setup_device", "conp_integrate_initial_device", "conp_integrate_final_device",
    "conp_integrate_temperature_device", "conp_integrate_get_state", "conp_integrate_set_state",
    "conp_shake_set_params", "conp_shake_correct_device", "conp_shake_setup_device", "conp_shake_post_force_device",
    "conp_shake_check_device",
    "conp_efield_set_params", "conp_efield_post_force_device", "conp_observe_set_params", "conp_observe_device",
    "conp_pair_set_exclusions", "conp_pair_build_list_exclude_device",
    "conp_zmirror_set_params", "conp_zmirror_post_integrate_device", "conp_zmirror_get_map",
    "conp_pair_transpose_list_device", "conp_fix_transpose_list_device", "conp_pair_get_transposed_list",
    "conp_pair_compute_ordered_device", "conp_fix_post_force_ordered_device",
    "conp_potential_atom_device",
]


# test hooks of the ABI (include/conp_hip.h, CONP_PATH_*): alternative code paths the parity tests compare the default ones with
PATH_PARTIAL_TILES, PATH_A_GENERAL, PATH_INV_PIVOTED, PATH_CG_TWO_LAUNCH, PATH_GEMV_ROWS = 1, 2, 4, 8, 16
PATH_PHASE_LAUNCH, PATH_PPPM_SPREAD_LAUNCH, PATH_ROWS_HOST, PATH_TIME_SPLIT = 32, 64, 128, 256
PATH_SK_CLASSIC = 4096      # (512, 1024, 2048: retired test paths, ignored by the library)
PATH_ZN_WIDE = 8192         # z-window: 48 window columns also where 32 would do
PATH_ZC_PHASE_LOADS = 16384     # finishing dot kernel: electrode phases loaded per thread, not staged in LDS
PATH_HC_TABLES = 32768          # z-window: the piece sums read their piece lists, not arithmetic addresses
PATH_SOLVE_NO_LATTICE = 65536   # solve: packed symmetric tiles also where the electrodes are a lattice
SOLVE_FORMS = {-1: "undecided", 0: "rows", 1: "packed", 2: "lattice"}


class test_paths:
    """with capi.test_paths(capi.PATH_PARTIAL_TILES): ...   -- process-wide; handles created inside take the alternative path"""

    def __init__(self, mask=0, sk_workgroups=0):
        self.mask, self.nwg = mask, sk_workgroups

    def __enter__(self):
        lib = load_library()
        if not hasattr(lib, "conp_debug_set_paths"):
            raise RuntimeError("this library build has no test hooks (a comparison build of an earlier round?)")
        lib.conp_debug_set_paths(self.mask)
        lib.conp_debug_set_sk_workgroups(self.nwg)
        return self

    def __exit__(self, *a):
        lib = load_library()
        lib.conp_debug_set_paths(0)
        lib.conp_debug_set_sk_workgroups(0)
        return False


def set_ew_block(n: int):
    """test hook (conp_debug_set_ew_block): cap of the atom block of the conp_ewald_* entries, rounded up to a multiple of 64;
    0 = the library's choice.  Process-wide, read at every call"""
    load_library().conp_debug_set_ew_block(int(n))


def set_lat_stage(n: int):
    """test hook (conp_debug_set_lat_stage): cap of the basis atoms the lattice solve stages at a time; 0 = as many as fit.
    Process-wide, read once per matrix"""
    load_library().conp_debug_set_lat_stage(int(n))


def find_lattice(x, lx, ly):
    """the library's host lattice search (no device): None, or dict(nx, ny, nbasis, row[nbasis, nx, ny], pos[n, 3])"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = len(x)
    dims, row, pos = np.zeros(3, np.int32), np.zeros(n, np.int32), np.zeros((n, 3), np.int32)
    if not load_library().conp_host_find_lattice(n, _dptr(x), float(lx), float(ly), _iptr(dims), _iptr(row), _iptr(pos)):
        return None
    nx, ny, nb = (int(v) for v in dims)
    return dict(nx=nx, ny=ny, nbasis=nb, row=row.reshape(nb, nx, ny), pos=pos)


def load_library():
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = C.CDLL(path)
    vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)
    lib.conp_last_error.restype = C.c_char_p
    lib.conp_parse_fix_args.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_int, C.POINTER(conp_fix_args)]
    lib.conp_fix_create.argtypes = [C.POINTER(conp_fix_args), C.POINTER(conp_env), C.POINTER(vp)]
    lib.conp_fix_destroy.argtypes = [vp]
    lib.conp_fix_destroy.restype = None
    if hasattr(lib, "conp_fix_pin_host_arrays"):      # (comparison builds of earlier rounds, loaded through CONP_LIB, lack these)
        lib.conp_fix_pin_host_arrays.argtypes = [vp, dp, dp, C.c_int]
        lib.conp_fix_unpin_host_arrays.argtypes = [vp]
        lib.conp_host_alloc.argtypes = [C.c_size_t]
        lib.conp_host_alloc.restype = C.c_void_p
        lib.conp_host_free.argtypes = [C.c_void_p]
        lib.conp_host_free.restype = None
    if hasattr(lib, "conp_debug_set_paths"):
        lib.conp_debug_set_paths.argtypes = [C.c_uint]
        lib.conp_debug_set_paths.restype = None
        lib.conp_debug_set_sk_workgroups.argtypes = [C.c_int]
        lib.conp_debug_set_sk_workgroups.restype = None
    lib.conp_fix_init_list.argtypes = [vp, C.c_int, C.POINTER(conp_neighlist)]
    for n in ("conp_fix_setup_post_neighbor", "conp_fix_post_neighbor", "conp_fix_linalg_setup", "conp_fix_a_cal",
              "conp_fix_b_cal"):
        getattr(lib, n).argtypes = [vp, C.POINTER(conp_atoms)]
    for n in ("conp_fix_setup_pre_force", "conp_fix_pre_force"):
        getattr(lib, n).argtypes = [vp, C.POINTER(conp_atoms), C.c_int64, C.c_double]
    lib.conp_fix_compute_scalar.argtypes = [vp]
    lib.conp_fix_compute_scalar.restype = C.c_double
    lib.conp_fix_post_force.argtypes = [vp, C.POINTER(conp_atoms), dp, dp, dp, dp]
    lib.conp_fix_post_force_step.argtypes = [vp, C.POINTER(conp_atoms), C.c_int64, dp, dp, dp, dp]
    lib.conp_fix_modify_param.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), ip]
    lib.conp_fix_equation_solve.argtypes = [vp]
    lib.conp_fix_update_charge.argtypes = [vp, C.POINTER(conp_atoms), C.c_double]
    lib.conp_km_conp_setup.argtypes = [vp, C.c_double, C.c_int64]
    lib.conp_km_a_cal.argtypes = [vp, C.POINTER(conp_atoms), dp]
    lib.conp_km_b_cal.argtypes = [vp, C.POINTER(conp_atoms), dp]
    lib.conp_fix_info.argtypes = [vp, C.POINTER(conp_info)]
    lib.conp_fix_get_ktables.argtypes = [vp, ip, ip, ip, dp, ip, ip]
    lib.conp_fix_get_maps.argtypes = [vp, ip, ip, ip, ip, ip, ip, ip]
    lib.conp_fix_get_matrix.argtypes = [vp, dp]
    lib.conp_fix_set_matrix.argtypes = [vp, dp, C.c_int]
    lib.conp_fix_get_vectors.argtypes = [vp, dp, dp, dp]
    if hasattr(lib, "conp_fix_get_solve_form"):       # (comparison builds of earlier rounds lack the lattice form)
        lib.conp_fix_get_solve_form.argtypes = [vp, ip, dp]
        lib.conp_host_find_lattice.argtypes = [C.c_int, dp, C.c_double, C.c_double, ip, ip, ip]
        lib.conp_debug_set_lat_stage.argtypes = [C.c_int]
        lib.conp_debug_set_lat_stage.restype = None
    lib.conp_fix_get_sfac.argtypes = [vp, dp, dp]
    lib.conp_fix_get_ele_trig.argtypes = [vp, dp, dp]
    lib.conp_inv_project.argtypes = [vp, C.c_int, dp, C.c_int, C.c_int, dp, C.c_double, dp]
    lib.conp_invert.argtypes = [vp, C.c_int, dp]
    lib.conp_host_ktables.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                      C.c_int64, C.c_double, C.c_double, ip, ip, ip, ip, dp, ip, ip, ip, ip, ip]
    lib.conp_host_index.argtypes = [C.c_int, ip, ip, C.c_int, ip, ip, ip, ip, ip, ip, ip, ip, ip]
    lib.conp_host_pair_rows.argtypes = [C.c_int, C.POINTER(conp_neighlist), C.POINTER(conp_atoms), C.c_int, ip, ip, ip, ip]
    lib.conp_host_pair_rows.restype = C.c_int64
    lib.conp_fix_write_matrix_file.argtypes = [vp, C.c_char_p, C.c_int]
    lib.conp_fix_read_matrix_file.argtypes = [vp, C.POINTER(conp_atoms), C.c_char_p]
    lib.conp_fix_set_stream.argtypes = [vp, vp]
    lib.conp_fix_bind_device_buffers.argtypes = [vp, vp, vp]
    lib.conp_fix_row_range.argtypes = [vp, ip, ip]
    lib.conp_fix_b_cal_device.argtypes = [vp, vp, vp]
    lib.conp_fix_solve_device.argtypes = [vp, C.c_double]
    lib.conp_fix_scatter_device.argtypes = [vp, vp, C.c_double]
    lib.conp_fix_pre_force_device.argtypes = [vp, vp, vp, C.c_double]
    lib.conp_fix_profile.argtypes = [vp, C.c_int]
    lib.conp_fix_profile_read.argtypes = [vp, ip, C.POINTER(C.c_char_p), dp, ip]
    lib.conp_fix_write_timing.argtypes = [vp]
    lib.conp_fix_log_drain.argtypes = [vp]
    lib.conp_fix_log_drain.restype = C.c_char_p
    lib.conp_fix_mesg_drain.argtypes = [vp]
    lib.conp_fix_mesg_drain.restype = C.c_char_p
    lib.conp_pppm_make_rho.argtypes = [vp, C.POINTER(conp_atoms), dp, dp, dp]
    lib.conp_pppm_compute_group_potential.argtypes = [vp, C.POINTER(conp_atoms), ip, dp]
    lib.conp_pppm_compute_particle_potential.argtypes = [vp, C.POINTER(conp_atoms), C.c_int, dp]
    if hasattr(lib, "conp_pppm_compute"):
        lib.conp_pppm_compute.argtypes = [vp, C.POINTER(conp_atoms)]
        lib.conp_pppm_keep_density.argtypes = [vp, C.c_int]
    lib.conp_ewald_compute.argtypes = [vp, C.POINTER(conp_atoms)]
    lib.conp_ewald_compute_group_potential.argtypes = [vp, C.POINTER(conp_atoms), ip, dp]
    lib.conp_ewald_compute_particle_potential.argtypes = [vp, C.POINTER(conp_atoms), C.c_int, dp]
    lib.conp_ewald_compute_forces.argtypes = [vp, C.POINTER(conp_atoms), dp, dp, dp, dp]
    lib.conp_pppm_compute_forces.argtypes = [vp, C.POINTER(conp_atoms), dp, dp, dp, dp]
    if hasattr(lib, "conp_ewald_compute_forces_device"):      # (comparison builds loaded through CONP_LIB lack these)
        lib.conp_ewald_compute_forces_device.argtypes = [vp, vp, vp, vp, vp, vp]
        lib.conp_pppm_compute_forces_device.argtypes = [vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "conp_ewald_compute_forces_vatom"):
        lib.conp_ewald_compute_forces_vatom.argtypes = [vp, C.POINTER(conp_atoms), dp, dp, dp, dp, dp]
        lib.conp_pppm_compute_forces_vatom.argtypes = [vp, C.POINTER(conp_atoms), dp, dp, dp, dp, dp]
        lib.conp_ewald_compute_forces_vatom_device.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        lib.conp_pppm_compute_forces_vatom_device.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        lib.conp_debug_set_ew_block.argtypes = [C.c_int]
        lib.conp_debug_set_ew_block.restype = None
    if hasattr(lib, "conp_pair_compute"):                      # (comparison builds loaded through CONP_LIB lack these)
        lib.conp_pair_set_params.argtypes = [vp, C.POINTER(conp_pair_params)]
        lib.conp_pair_set_list.argtypes = [vp, C.POINTER(conp_neighlist), C.c_int]
        lib.conp_pair_compute.argtypes = [vp, C.POINTER(conp_atoms), dp, dp, dp, dp, dp]
        lib.conp_pair_compute_device.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "conp_pair_build_list_device"):
        lib.conp_pair_build_list_device.argtypes = [vp, vp, C.POINTER(conp_pair_build_args)]
        lib.conp_pair_list_moved_device.argtypes = [vp, vp, C.c_double, vp]
        lib.conp_pair_get_list.argtypes = [vp, ip, ip, C.POINTER(C.c_int64), ip, ip, ip, ip]
    if hasattr(lib, "conp_ghost_build_device"):                # (comparison builds loaded through CONP_LIB lack these)
        lib.conp_ghost_build_device.argtypes = [vp, vp, C.POINTER(conp_ghost_build_args), ip]
        lib.conp_ghost_fill_device.argtypes = [vp, vp, vp]
        lib.conp_ghost_fill_int_device.argtypes = [vp, vp, C.c_int]
        lib.conp_ghost_fold_device.argtypes = [vp, vp, C.c_int]
        lib.conp_ghost_get.argtypes = [vp, ip, ip, ip, ip]
        lib.conp_atoms_wrap_device.argtypes = [vp, vp, C.c_int, dp, dp, ip, vp]
    if hasattr(lib, "conp_fix_post_neighbor_device"):          # (comparison builds loaded through CONP_LIB lack these)
        lib.conp_fix_post_neighbor_device.argtypes = [vp, vp, vp]
        lib.conp_fix_get_step_tables.argtypes = [vp, C.POINTER(C.c_int64)] + [ip] * 9
    if hasattr(lib, "conp_fix_post_force_device"):
        lib.conp_fix_post_force_device.argtypes = [vp, vp, vp, vp, vp]
    if hasattr(lib, "conp_bonded_compute"):                    # (comparison builds loaded through CONP_LIB lack these)
        lib.conp_bonded_set_params.argtypes = [vp, C.POINTER(conp_bonded_params)]
        lib.conp_bonded_set_lists.argtypes = [vp, C.POINTER(conp_bonded_lists)]
        lib.conp_bonded_compute.argtypes = [vp, C.POINTER(conp_atoms), dp, dp, dp, dp, dp]
        lib.conp_bonded_compute_device.argtypes = [vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "conp_dihedral_compute"):
        lib.conp_dihedral_set_params.argtypes = [vp, C.POINTER(conp_dihedral_params)]
        lib.conp_dihedral_set_lists.argtypes = [vp, C.POINTER(conp_dihedral_lists)]
        lib.conp_dihedral_compute.argtypes = [vp, C.POINTER(conp_atoms), dp, dp, dp, dp, dp]
        lib.conp_dihedral_compute_device.argtypes = [vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "conp_integrate_set_params"):
        lib.conp_integrate_set_params.argtypes = [vp, C.POINTER(conp_integrate_params)]
        lib.conp_integrate_setup_device.argtypes = [vp, vp, dp]
        lib.conp_integrate_initial_device.argtypes = [vp, vp, vp, vp, dp]
        lib.conp_integrate_final_device.argtypes = [vp, vp, vp, vp]
        lib.conp_integrate_temperature_device.argtypes = [vp, vp, vp]
        lib.conp_integrate_get_state.argtypes = [vp, dp]
        lib.conp_integrate_set_state.argtypes = [vp, dp]
    if hasattr(lib, "conp_shake_set_params"):
        lib.conp_shake_set_params.argtypes = [vp, C.POINTER(conp_shake_params)]
        lib.conp_shake_correct_device.argtypes = [vp, vp]
        lib.conp_shake_setup_device.argtypes = [vp, vp, vp, vp, vp]
        lib.conp_shake_post_force_device.argtypes = [vp, vp, vp, vp, vp, vp]
        lib.conp_shake_check_device.argtypes = [vp, vp, vp]
    if hasattr(lib, "conp_efield_set_params"):
        lib.conp_efield_set_params.argtypes = [vp, C.POINTER(conp_efield_params)]
        lib.conp_efield_post_force_device.argtypes = [vp, vp, vp, vp, vp, dp, C.c_int, C.c_double, vp, vp]
        lib.conp_observe_set_params.argtypes = [vp, C.POINTER(conp_observe_params)]
        lib.conp_observe_device.argtypes = [vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "conp_pair_set_exclusions"):
        lib.conp_pair_set_exclusions.argtypes = [vp, C.POINTER(conp_pair_exclusions)]
        lib.conp_pair_build_list_exclude_device.argtypes = [vp, vp, C.POINTER(conp_pair_build_args), C.POINTER(conp_pair_exclude_atoms)]
        lib.conp_zmirror_set_params.argtypes = [vp, C.POINTER(conp_zmirror_params)]
        lib.conp_zmirror_post_integrate_device.argtypes = [vp, vp, C.c_longlong]
        lib.conp_zmirror_get_map.argtypes = [vp, ip, ip, ip]
    if hasattr(lib, "conp_pair_compute_ordered_device"):
        lib.conp_pair_transpose_list_device.argtypes = [vp]
        lib.conp_fix_transpose_list_device.argtypes = [vp]
        lib.conp_pair_get_transposed_list.argtypes = [vp, C.c_int, ip, C.POINTER(C.c_int64), ip, ip, ip]
        lib.conp_pair_compute_ordered_device.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        lib.conp_fix_post_force_ordered_device.argtypes = [vp, vp, vp, vp, vp]
    lib.conp_compute_potential_atom.argtypes = [vp, C.POINTER(conp_atoms), C.POINTER(conp_neighlist), ip, ip,
                                                C.POINTER(conp_potential_args), dp]
    if hasattr(lib, "conp_potential_atom_device"):
        lib.conp_potential_atom_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, C.POINTER(conp_potential_args), C.c_int, vp]
    lib.conp_fix_set_comm.argtypes = [vp, C.POINTER(conp_comm)]
    lib.conp_rccl_unique_id.argtypes = [C.c_void_p]
    lib.conp_fix_comm_init_rccl.argtypes = [vp, C.c_void_p]
    _LIB = lib
    return lib


def potential_selection(sel, etasel, nlocal):
    """(flags, targets, ntargets) of conp_potential_atom_device from the host entry's selections: sel, etasel [nall] (nonzero: the
    row is selected / an eta_check atom; etasel None: nobody).  flags [nall] int32 -- bit 0 selected, bit 1 eta_check; targets
    int32 -- the selected rows below nlocal, ascending (one entry, unused, when there is none: an array to upload)"""
    sel = np.asarray(sel).reshape(-1)
    flags = (sel != 0).astype(np.int32)
    if etasel is not None:
        es = np.asarray(etasel).reshape(-1)
        if es.size != sel.size:
            raise ValueError("sel and etasel differ in length")
        flags |= (es != 0).astype(np.int32) << 1
    if not 0 <= int(nlocal) <= sel.size:
        raise ValueError("nlocal outside [0, len(sel)]")
    targets = np.flatnonzero(flags[:int(nlocal)] & 1).astype(np.int32)
    ntargets = int(targets.size)
    if ntargets == 0:
        targets = np.zeros(1, np.int32)
    return np.ascontiguousarray(flags), targets, ntargets


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def parse_fix_command(tokens: Sequence[str], ntypes: int) -> conp_fix_args:
    """tokens = the whole `fix` command split on whitespace: ID group1 conp Nevery group2 eta DV logfile [keywords]"""
    lib = load_library()
    arr = (C.c_char_p * len(tokens))(*[t.encode() for t in tokens])
    out = conp_fix_args()
    rc = lib.conp_parse_fix_args(len(tokens), arr, ntypes, C.byref(out))
    if rc != 0:
        raise ConpError(rc, lib.conp_last_error().decode())
    return out


def fix_command_for(s: "_systems.System", extra: Sequence[str] = (), style: str = "conp") -> list:
    """the fix command the reference's decks would use for this system"""
    toks = ["e", "eleleft", style, "1", "eleright", repr(float(s.eta)), repr(float(s.potdiff)), "log_conp"]
    if s.eletypes is not None:
        toks += ["etypes", str(len(s.eletypes))] + [str(t) for t in s.eletypes]
    if s.ff_flag == 1:
        toks.append("ffield")
    elif s.ff_flag == 2:
        toks.append("noslab")
    if s.zneutr:
        toks.append("zneutr")
    return toks + list(extra)


class FixConp:
    """Drives one `fix conp` instance through the C ABI the way LAMMPS' Modify drives the reference fix:
    init_list -> setup_post_neighbor -> setup_pre_force -> [post_neighbor] -> pre_force ...."""

    def __init__(self, s: "_systems.System", extra_args: Sequence[str] = (), device: int = 0, rank: int = 0,
                 nranks: int = 1, one_electrode: bool = False, style: str = "conp", pppm_mesh=None, pppm_order: int = 5,
                 ghost_images: bool = False):
        self.lib = load_library()
        self.s = s
        self.args = parse_fix_command(fix_command_for(s, extra_args, style), s.ntypes)
        self._cutsq = np.ascontiguousarray(s.cutsq_table())
        env = conp_env(qqrd2e=_systems.QQRD2E, qqr2e=_systems.QQR2E, qe2f=_systems.QE2F, dielectric=1.0,
                       newton_pair=int(s.newton), g_ewald=s.g_ewald, accuracy=s.accuracy,
                       slab_volfactor=s.slab_volfactor, slabflag=s.slabflag, xprd=float(s.prd[0]), yprd=float(s.prd[1]),
                       zprd=float(s.prd[2]), boxlo_z=float(s.boxlo[2]), ntypes=s.ntypes, cutsq=_dptr(self._cutsq),
                       cut_coul=s.cutoff, one_electrode=int(one_electrode), device=device, rank=rank, nranks=nranks,
                       boxlo_x=float(s.boxlo[0]), boxlo_y=float(s.boxlo[1]),
                       pppm_nx=pppm_mesh[0] if pppm_mesh else 0, pppm_ny=pppm_mesh[1] if pppm_mesh else 0,
                       pppm_nz=pppm_mesh[2] if pppm_mesh else 0, pppm_order=pppm_order if pppm_mesh else 0,
                       ghost_images=int(ghost_images))
        self.h = C.c_void_p()
        self._check(self.lib.conp_fix_create(C.byref(self.args), C.byref(env), C.byref(self.h)))
        self._keep = {}

    def _check(self, rc):
        if rc != 0:
            raise ConpError(rc, self.lib.conp_last_error().decode())

    # -- views -----------------------------------------------------------------------------------
    def atoms_view(self, at) -> conp_atoms:
        x = np.ascontiguousarray(at.x, dtype=np.float64)
        self._keep["atoms"] = (x, at.q, at.type, at.tag, at.echeck)
        return conp_atoms(nlocal=at.nlocal, nghost=at.nghost, x=_dptr(x), q=_dptr(at.q), type=_iptr(at.type),
                          tag=_iptr(at.tag), echeck=_iptr(at.echeck))

    def init_list(self, which: int, lst):
        neigh = lst.neigh if lst.neigh.size else np.zeros(1, np.int32)
        self._keep[f"list{which}"] = (lst.ilist, lst.numneigh, lst.first, neigh)
        v = conp_neighlist(inum=lst.inum, ilist=_iptr(lst.ilist), numneigh=_iptr(lst.numneigh), first=_iptr(lst.first),
                           neigh=_iptr(neigh), nneigh=int(lst.neigh.size))
        self._check(self.lib.conp_fix_init_list(self.h, which, C.byref(v)))

    def init_lists(self, alist, blist):
        if alist is blist:
            self.init_list(2, alist)
        else:
            self.init_list(0, alist)
            self.init_list(1, blist)

    # -- hooks (same names as the reference's Fix methods) ---------------------------------------------
    def setup_post_neighbor(self, at):
        self._check(self.lib.conp_fix_setup_post_neighbor(self.h, C.byref(self.atoms_view(at))))

    def setup_pre_force(self, at, ntimestep=0, potdiff=None):
        pd = self.s.potdiff if potdiff is None else potdiff
        self._check(self.lib.conp_fix_setup_pre_force(self.h, C.byref(self.atoms_view(at)), ntimestep, pd))

    def linalg_setup(self, at):
        self._check(self.lib.conp_fix_linalg_setup(self.h, C.byref(self.atoms_view(at))))

    def post_neighbor(self, at):
        self._check(self.lib.conp_fix_post_neighbor(self.h, C.byref(self.atoms_view(at))))

    def pre_force(self, at, ntimestep=0, potdiff=None):
        pd = self.s.potdiff if potdiff is None else potdiff
        self._check(self.lib.conp_fix_pre_force(self.h, C.byref(self.atoms_view(at)), ntimestep, pd))

    def a_cal(self, at):
        self._check(self.lib.conp_fix_a_cal(self.h, C.byref(self.atoms_view(at))))

    def b_cal(self, at):
        self._check(self.lib.conp_fix_b_cal(self.h, C.byref(self.atoms_view(at))))

    def equation_solve(self):
        self._check(self.lib.conp_fix_equation_solve(self.h))

    def update_charge(self, at, potdiff=None):
        pd = self.s.potdiff if potdiff is None else potdiff
        self._check(self.lib.conp_fix_update_charge(self.h, C.byref(self.atoms_view(at)), pd))

    def modify_param(self, *tokens):
        """fix_modify ID <tokens>, e.g. modify_param("ehgo", "coeff", "5", "1.979", "auto")"""
        arr = (C.c_char_p * len(tokens))(*[str(t).encode() for t in tokens])
        n = C.c_int()
        self._check(self.lib.conp_fix_modify_param(self.h, len(tokens), arr, C.byref(n)))
        return n.value

    def post_force(self, at):
        f = np.zeros((at.nlocal + at.nghost, 3)); ek = C.c_double(); ec = C.c_double(); vir = np.zeros(6)
        self._check(self.lib.conp_fix_post_force(self.h, C.byref(self.atoms_view(at)), _dptr(f), C.byref(ek), C.byref(ec), _dptr(vir)))
        return f, ek.value, ec.value, vir

    def post_force_step(self, at, ntimestep):
        f = np.zeros((at.nlocal + at.nghost, 3)); ek = C.c_double(); ec = C.c_double(); vir = np.zeros(6)
        self._check(self.lib.conp_fix_post_force_step(self.h, C.byref(self.atoms_view(at)), C.c_int64(ntimestep), _dptr(f),
                                                      C.byref(ek), C.byref(ec), _dptr(vir)))
        return f, ek.value, ec.value, vir

    def compute_scalar(self):
        return float(self.lib.conp_fix_compute_scalar(self.h))

    # -- provider surface ------------------------------------------------------------------------
    def km_conp_setup(self, qsqsum, natoms):
        self._check(self.lib.conp_km_conp_setup(self.h, qsqsum, natoms))

    def km_b_cal(self, at):
        b = np.zeros(self.info().elenum_all)
        self._check(self.lib.conp_km_b_cal(self.h, C.byref(self.atoms_view(at)), _dptr(b)))
        return b

    def km_a_cal(self, at):
        ne = self.info().elenum_all
        a = np.zeros((ne, ne))
        self._check(self.lib.conp_km_a_cal(self.h, C.byref(self.atoms_view(at)), _dptr(a)))
        return a

    # -- read-back -------------------------------------------------------------------------------
    def info(self) -> conp_info:
        o = conp_info()
        self._check(self.lib.conp_fix_info(self.h, C.byref(o)))
        return o

    def ktables(self):
        i = self.info()
        K, E = i.kcount, max(i.kcount_expand, 1)
        kx, ky, kz = (np.zeros(K, np.int32) for _ in range(3))
        ug = np.zeros(K); kxy = np.zeros(E, np.int32); kzl = np.zeros(E, np.int32)
        self._check(self.lib.conp_fix_get_ktables(self.h, _iptr(kx), _iptr(ky), _iptr(kz), _dptr(ug), _iptr(kxy), _iptr(kzl)))
        return dict(kxvecs=kx, kyvecs=ky, kzvecs=kz, ug=ug, kxy_list=kxy[:i.kcount_expand], kz_list=kzl[:i.kcount_expand])

    def maps(self):
        i = self.info()
        n, na, mt = i.elenum, i.elenum_all, i.maxtag_all
        m = dict(ele2tag=np.zeros(n, np.int32), ele2eleall=np.zeros(n, np.int32), eleall2tag=np.zeros(na, np.int32),
                 eleall2ele=np.zeros(na + 1, np.int32), elecheck_eleall=np.zeros(na, np.int32),
                 elebuf2eleall=np.zeros(na, np.int32), tag2eleall=np.zeros(mt + 1, np.int32))
        self._check(self.lib.conp_fix_get_maps(self.h, *[_iptr(m[k]) for k in (
            "ele2tag", "ele2eleall", "eleall2tag", "eleall2ele", "elecheck_eleall", "elebuf2eleall", "tag2eleall")]))
        return m

    def matrix(self):
        ne = self.info().elenum_all
        a = np.zeros((ne, ne))
        self._check(self.lib.conp_fix_get_matrix(self.h, _dptr(a)))
        return a

    def set_matrix(self, a, runstage):
        a = np.ascontiguousarray(a, dtype=np.float64)
        self._check(self.lib.conp_fix_set_matrix(self.h, _dptr(a), runstage))

    def solve_form(self):
        """dict(form="rows" | "packed" | "lattice" | "undecided", nx, ny, nbasis, dev, smax): conp_fix_get_solve_form"""
        f, d = np.zeros(4, np.int32), np.zeros(2)
        self._check(self.lib.conp_fix_get_solve_form(self.h, _iptr(f), _dptr(d)))
        return dict(form=SOLVE_FORMS[int(f[0])], nx=int(f[1]), ny=int(f[2]), nbasis=int(f[3]), dev=float(d[0]), smax=float(d[1]))

    def vectors(self):
        ne = self.info().elenum_all
        b, q, sq = np.zeros(ne), np.zeros(ne), np.zeros(ne)
        self._check(self.lib.conp_fix_get_vectors(self.h, _dptr(b), _dptr(q), _dptr(sq)))
        return b, q, sq

    def sfac(self):
        K = self.info().kcount
        sr, si = np.zeros(K), np.zeros(K)
        self._check(self.lib.conp_fix_get_sfac(self.h, _dptr(sr), _dptr(si)))
        return sr, si

    def ele_trig(self):
        i = self.info()
        c = np.zeros((i.elenum_all, i.kcount_flat)); s = np.zeros((i.elenum_all, i.kcount_flat))
        self._check(self.lib.conp_fix_get_ele_trig(self.h, _dptr(c), _dptr(s)))
        return c, s

    def inv_project(self, a, nullneutral=True, zneutr=False, eleallz=None, zhalf=0.0):
        a = np.ascontiguousarray(a, dtype=np.float64).copy()
        n = a.shape[0]
        z = np.zeros(n) if eleallz is None else np.ascontiguousarray(eleallz, dtype=np.float64)
        tot = C.c_double()
        self._check(self.lib.conp_inv_project(self.h, n, _dptr(a), int(nullneutral), int(zneutr), _dptr(z), zhalf, C.byref(tot)))
        return a, tot.value

    def write_matrix_file(self, path, which):
        self._check(self.lib.conp_fix_write_matrix_file(self.h, str(path).encode(), which))

    def read_matrix_file(self, at, path):
        self._check(self.lib.conp_fix_read_matrix_file(self.h, C.byref(self.atoms_view(at)), str(path).encode()))

    def invert(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64).copy()
        self._check(self.lib.conp_invert(self.h, a.shape[0], _dptr(a)))
        return a

    # -- PPPM coupling beyond b, compute potential/atom ---------------------------------------------
    def pppm_keep_density(self, on=True):
        self._check(self.lib.conp_pppm_keep_density(self.h, 1 if on else 0))

    def pppm_compute(self, at):
        """collective: the mesh potential of the total density (u_brick) formed and cached"""
        self._check(self.lib.conp_pppm_compute(self.h, C.byref(self.atoms_view(at))))

    def pppm_make_rho(self, at, nfft):
        d, e, l = np.zeros(nfft), np.zeros(nfft), np.zeros(nfft)
        self._check(self.lib.conp_pppm_make_rho(self.h, C.byref(self.atoms_view(at)), _dptr(d), _dptr(e), _dptr(l)))
        return d, e, l

    def pppm_group_potential(self, at, sel):
        sel = np.ascontiguousarray(sel, np.int32)
        out = np.zeros(at.nlocal)
        self._check(self.lib.conp_pppm_compute_group_potential(self.h, C.byref(self.atoms_view(at)), _iptr(sel), _dptr(out)))
        return out

    def pppm_particle_potential(self, at, i):
        u = C.c_double()
        self._check(self.lib.conp_pppm_compute_particle_potential(self.h, C.byref(self.atoms_view(at)), int(i), C.byref(u)))
        return u.value

    # -- Ewald per-atom potential (the exact k sum; the `pppm_*` trio's twins for the Ewald provider) ---------------------------
    def ewald_compute(self, at):
        """collective under decomposed ranks: the structure factor of every charged owned atom, formed and cached"""
        self._check(self.lib.conp_ewald_compute(self.h, C.byref(self.atoms_view(at))))

    def ewald_group_potential(self, at, sel):
        """collective: g_i = - sum_k 2 ug_k [cos(k r_i) Re S_k + sin(k r_i) Im S_k] for owned atoms with sel[i] != 0 (others 0)"""
        sel = np.ascontiguousarray(sel, np.int32)
        out = np.zeros(at.nlocal)
        self._check(self.lib.conp_ewald_compute_group_potential(self.h, C.byref(self.atoms_view(at)), _iptr(sel), _dptr(out)))
        return out

    def ewald_particle_potential(self, at, i):
        """rank-local: u_i = g_i + 2 g_ewald q_i / sqrt(pi) from the cached structure factor"""
        u = C.c_double()
        self._check(self.lib.conp_ewald_compute_particle_potential(self.h, C.byref(self.atoms_view(at)), int(i), C.byref(u)))
        return u.value

    def ewald_forces(self, at, energy=True, virial=True, eatom=False, f=None):
        """collective under decomposed ranks: reciprocal-space forces [nlocal][3] (added to `f`, zeros by default), energy, virial
        (xx, yy, zz, xy, xz, yz) and per-atom energies of the owned atoms -> (f, E, W, e); what was not asked for is None"""
        return self._forces_vatom(self.lib.conp_ewald_compute_forces, at, energy, virial, eatom, f, True, vatom=False)[:4]

    def pppm_compute_forces(self, at, energy=True, virial=True, eatom=False, f=None, forces=True):
        """the mesh twin of ewald_forces (`pppm` handles; collective under decomposed ranks): PPPM reciprocal-space forces [nlocal][3]
        (added to `f`, zeros by default; forces=False: none), energy, virial (xx, yy, zz, xy, xz, yz) and per-atom energies of the owned
        atoms -> (f, E, W, e); what was not asked for is None"""
        return self._forces_vatom(self.lib.conp_pppm_compute_forces, at, energy, virial, eatom, f, forces, vatom=False)[:4]

    def _forces_vatom(self, entry, at, energy, virial, eatom, f, forces, vatom):
        """the output arrays of a host force entry and the call; `entry` with or without the trailing vatom parameter"""
        if forces:
            f = np.zeros((at.nlocal, 3)) if f is None else f
            assert f.dtype == np.float64 and f.flags.c_contiguous and f.shape == (at.nlocal, 3)
        else:
            f = None
        en = C.c_double() if energy else None
        w = np.zeros(6) if virial else None
        e = np.zeros(at.nlocal) if eatom else None
        v = np.full((at.nlocal, 6), np.nan) if vatom else None        # (overwritten by the entry, zero-charge rows included)
        args = [_dptr(f) if forces else None, C.byref(en) if energy else None, _dptr(w) if virial else None, _dptr(e) if eatom else None,
                _dptr(v) if vatom else None]
        self._check(entry(self.h, C.byref(self.atoms_view(at)), *args[:len(entry.argtypes) - 2]))
        return f, (en.value if energy else None), w, e, v

    def ewald_forces_vatom(self, at, energy=True, virial=True, eatom=False, f=None, forces=True, vatom=True):
        """conp_ewald_compute_forces_vatom: ewald_forces with the per-atom virial [nlocal][6] (xx, yy, zz, xy, xz, yz) as one more
        output -> (f, E, W, e, v); what was not asked for is None"""
        return self._forces_vatom(self.lib.conp_ewald_compute_forces_vatom, at, energy, virial, eatom, f, forces, vatom)

    def pppm_forces_vatom(self, at, energy=True, virial=True, eatom=False, f=None, forces=True, vatom=True):
        """conp_pppm_compute_forces_vatom: the mesh twin of ewald_forces_vatom (`pppm` handles)"""
        return self._forces_vatom(self.lib.conp_pppm_compute_forces_vatom, at, energy, virial, eatom, f, forces, vatom)

    def compute_potential_atom(self, at, pairlist, sel, etasel=None, eta=0.0, pair=True, kspace=True, qsum=True):
        sel = np.ascontiguousarray(sel, np.int32)
        es = None if etasel is None else np.ascontiguousarray(etasel, np.int32)
        pot = np.zeros(at.nlocal + at.nghost)
        pa = conp_potential_args(pairflag=int(pair), kspaceflag=int(kspace), qsumflag=int(qsum), eta=float(eta))
        neigh = pairlist.neigh if pairlist.neigh.size else np.zeros(1, np.int32)
        lv = conp_neighlist(inum=pairlist.inum, ilist=_iptr(pairlist.ilist), numneigh=_iptr(pairlist.numneigh),
                            first=_iptr(pairlist.first), neigh=_iptr(neigh), nneigh=int(pairlist.neigh.size))
        self._check(self.lib.conp_compute_potential_atom(self.h, C.byref(self.atoms_view(at)), C.byref(lv), _iptr(sel),
                                                         _iptr(es) if es is not None else C.POINTER(C.c_int)(), C.byref(pa), _dptr(pot)))
        return pot

    # -- several ranks ---------------------------------------------------------------------------
    def set_comm_torch(self, group=None):
        """conp_fix_set_comm with callbacks on torch.distributed (any backend that moves CPU tensors, e.g. gloo): the atoms and
        lists handed to the hooks from now on are THIS RANK's sub-domain -- the role MPI plays for the LAMMPS glue"""
        import torch
        import torch.distributed as dist
        rank, world = dist.get_rank(group), dist.get_world_size(group)

        def cb_sum(_ctx, buf, n):
            a = np.ctypeslib.as_array(buf, shape=(n,))
            t = torch.from_numpy(a)
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
            return 0

        def cb_maxi(_ctx, buf, n):
            a = np.ctypeslib.as_array(buf, shape=(n,))
            t = torch.from_numpy(a)
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
            return 0

        def cb_gather_int(_ctx, v, out):
            t = torch.tensor([v], dtype=torch.int32)
            outs = [torch.zeros(1, dtype=torch.int32) for _ in range(world)]
            dist.all_gather(outs, t, group=group)
            for r in range(world):
                out[r] = int(outs[r][0])
            return 0

        def cb_gatherv(_ctx, send, nbytes, recv, counts, displs):
            mine = torch.from_numpy(np.frombuffer((C.c_char * nbytes).from_address(send), dtype=np.uint8).copy()) if nbytes else torch.zeros(0, dtype=torch.uint8)
            outs = [torch.zeros(int(counts[r]), dtype=torch.uint8) for r in range(world)]
            dist.all_gather(outs, mine, group=group) if len({int(counts[r]) for r in range(world)}) == 1 else _uneven_all_gather(outs, mine, group, world)
            for r in range(world):
                n = int(counts[r])
                if n:
                    C.memmove(recv + int(displs[r]), outs[r].numpy().ctypes.data, n)
            return 0

        self._comm_cbs = (_CB_SUM(cb_sum), _CB_MAXI(cb_maxi), _CB_GATHER_INT(cb_gather_int), _CB_GATHERV(cb_gatherv))
        self._comm = conp_comm(ctx=None, rank=rank, nranks=world, allreduce_sum=self._comm_cbs[0], allreduce_max_int=self._comm_cbs[1],
                               allgather_int=self._comm_cbs[2], allgatherv=self._comm_cbs[3])
        self._check(self.lib.conp_fix_set_comm(self.h, C.byref(self._comm)))

    def comm_init_rccl(self, group=None):
        """One RCCL communicator inside the library (one rank per GPU): rank 0 makes the id, torch.distributed carries its 128 bytes.
        Returns True when EVERY rank has its communicator, False when every rank is without one (all ranks take the same branch):
          1. each rank probes librccl locally (conp_rccl_available) and the ranks agree (MIN) before anything collective is
             entered -- a rank that cannot load RCCL never leaves its partners inside ncclCommInitRank;
          2. rank 0's id (or the news that it could not make one) is broadcast;
          3. after ncclCommInitRank the ranks agree again; on any failure every rank destroys its communicator."""
        import torch
        import torch.distributed as dist

        def all_ok(ok):
            dev = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
            flag = torch.tensor([1 if ok else 0], device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
            return int(flag.item()) == 1

        if not all_ok(self.lib.conp_rccl_available() == 0):
            return False
        buf = (C.c_char * 128)()
        obj = [None]
        if dist.get_rank(group) == 0:
            if self.lib.conp_rccl_unique_id(buf) == 0:
                obj = [bytes(buf.raw)]
        dist.broadcast_object_list(obj, src=0, group=group)
        if obj[0] is None:
            return False
        idb = (C.c_char * 128).from_buffer_copy(obj[0])
        rc = self.lib.conp_fix_comm_init_rccl(self.h, idb)
        if all_ok(rc == 0):
            return True
        self.lib.conp_fix_comm_destroy_rccl(self.h)
        return False

    def pin_host_arrays(self, at):
        """page-lock at.x / at.q in place (conp_fix_pin_host_arrays): the host-buffer hooks then upload by asynchronous DMA"""
        self._pinned = (at.x, at.q)                 # keep them alive and in place
        self._check(self.lib.conp_fix_pin_host_arrays(self.h, _dptr(at.x), _dptr(at.q), int(at.nlocal + at.nghost)))

    def unpin_host_arrays(self):
        self._check(self.lib.conp_fix_unpin_host_arrays(self.h))
        self._pinned = None

    # -- device-resident path --------------------------------------------------------------------
    def set_stream(self, stream_ptr: int):
        self._check(self.lib.conp_fix_set_stream(self.h, C.c_void_p(stream_ptr)))

    def bind_device_buffers(self, d_b: Optional[int], d_q: Optional[int]):
        self._check(self.lib.conp_fix_bind_device_buffers(self.h, C.c_void_p(d_b or 0), C.c_void_p(d_q or 0)))

    def row_range(self):
        a, b = C.c_int(), C.c_int()
        self._check(self.lib.conp_fix_row_range(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def b_cal_device(self, d_x: int, d_q: int):
        self._check(self.lib.conp_fix_b_cal_device(self.h, C.c_void_p(d_x), C.c_void_p(d_q)))

    def solve_device(self, potdiff):
        self._check(self.lib.conp_fix_solve_device(self.h, potdiff))

    def scatter_device(self, d_q_atoms: int, potdiff):
        self._check(self.lib.conp_fix_scatter_device(self.h, C.c_void_p(d_q_atoms), potdiff))

    def pre_force_device(self, d_x: int, d_q: int, potdiff):
        self._check(self.lib.conp_fix_pre_force_device(self.h, C.c_void_p(d_x), C.c_void_p(d_q), potdiff))

    def _forces_device(self, entry, *ptrs):
        self._check(entry(self.h, *[C.c_void_p(p) for p in ptrs]))

    def ewald_forces_device(self, d_x: int, d_q: int, d_f: int = 0, d_ev: int = 0, d_eatom: int = 0):
        """conp_ewald_compute_forces_device: raw device pointers (0 = NULL), enqueued on the handle's stream, no synchronisation;
        d_f [nlocal][3] is added to, d_ev [7] (energy, virial xx, yy, zz, xy, xz, yz) and d_eatom [nlocal] are overwritten"""
        self._forces_device(self.lib.conp_ewald_compute_forces_device, d_x, d_q, d_f, d_ev, d_eatom)

    def pppm_forces_device(self, d_x: int, d_q: int, d_f: int = 0, d_ev: int = 0, d_eatom: int = 0):
        """conp_pppm_compute_forces_device: the mesh twin of ewald_forces_device (`pppm` handles)"""
        self._forces_device(self.lib.conp_pppm_compute_forces_device, d_x, d_q, d_f, d_ev, d_eatom)

    def ewald_forces_vatom_device(self, d_x: int, d_q: int, d_f: int = 0, d_ev: int = 0, d_eatom: int = 0, d_vatom: int = 0):
        """conp_ewald_compute_forces_vatom_device: ewald_forces_device with d_vatom [nlocal][6] (xx, yy, zz, xy, xz, yz), overwritten"""
        self._forces_device(self.lib.conp_ewald_compute_forces_vatom_device, d_x, d_q, d_f, d_ev, d_eatom, d_vatom)

    def pppm_forces_vatom_device(self, d_x: int, d_q: int, d_f: int = 0, d_ev: int = 0, d_eatom: int = 0, d_vatom: int = 0):
        """conp_pppm_compute_forces_vatom_device: the mesh twin of ewald_forces_vatom_device (`pppm` handles)"""
        self._forces_device(self.lib.conp_pppm_compute_forces_vatom_device, d_x, d_q, d_f, d_ev, d_eatom, d_vatom)

    # -- pair forces of lj/cut/coul/long: set_params -> set_list -> compute / compute_device ----------------
    def pair_set_params(self, cutsq, cut_coul, lj=None, special_lj=(1.0, 1.0, 1.0, 1.0), special_coul=(1.0, 1.0, 1.0, 1.0)):
        """conp_pair_set_params: cutsq [(ntypes+1)^2] and, with the LJ part, lj = dict(cut_ljsq, lj1, lj2, lj3, lj4, offset) of arrays
        of the same shape (None: coul/long); copied by the library"""
        nt1 = self.s.ntypes + 1
        arr = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(nt1 * nt1))
        null = C.POINTER(C.c_double)()
        cs = arr(cutsq)
        tabs = {k: arr(lj[k]) for k in ("cut_ljsq", "lj1", "lj2", "lj3", "lj4", "offset")} if lj is not None else {}
        p = conp_pair_params(ntypes=self.s.ntypes, cutsq=_dptr(cs), cut_coul=float(cut_coul),
                             special_lj=(C.c_double * 4)(*special_lj), special_coul=(C.c_double * 4)(*special_coul),
                             **{k: (_dptr(tabs[k]) if lj is not None else null) for k in ("cut_ljsq", "lj1", "lj2", "lj3", "lj4", "offset")})
        self._check(self.lib.conp_pair_set_params(self.h, C.byref(p)))

    def pair_set_list(self, lst, nall):
        """conp_pair_set_list: the pair style's half list (uploaded) and the atom count it indexes"""
        neigh = lst.neigh if lst.neigh.size else np.zeros(1, np.int32)
        v = conp_neighlist(inum=lst.inum, ilist=_iptr(lst.ilist), numneigh=_iptr(lst.numneigh), first=_iptr(lst.first),
                           neigh=_iptr(neigh), nneigh=int(lst.neigh.size))
        self._check(self.lib.conp_pair_set_list(self.h, C.byref(v), int(nall)))

    def pair_compute(self, at, forces=True, eng=True, virial=True, eatom=True, vatom=True, f=None):
        """conp_pair_compute on host arrays -> (f [nall][3] (added to `f`, zeros by default), eng [2], W [6], eatom [nall],
        vatom [nall][6]); what was not asked for is None"""
        n = at.nlocal + at.nghost
        if forces:
            f = np.zeros((n, 3)) if f is None else f
            assert f.dtype == np.float64 and f.flags.c_contiguous and f.shape == (n, 3)
        else:
            f = None
        e2 = np.full(2, np.nan) if eng else None
        w = np.full(6, np.nan) if virial else None
        ea = np.full(n, np.nan) if eatom else None
        va = np.full((n, 6), np.nan) if vatom else None
        ptr = lambda a: _dptr(a) if a is not None else None
        self._check(self.lib.conp_pair_compute(self.h, C.byref(self.atoms_view(at)), ptr(f), ptr(e2), ptr(w), ptr(ea), ptr(va)))
        return f, e2, w, ea, va

    def pair_compute_device(self, d_x: int, d_q: int, d_f: int = 0, d_ev: int = 0, d_eatom: int = 0, d_vatom: int = 0):
        """conp_pair_compute_device: raw device pointers (0 = NULL), enqueued on the handle's stream, no synchronisation; d_f [nall][3]
        is added to, d_ev [8] (eng_vdwl, eng_coul, virial xx, yy, zz, xy, xz, yz), d_eatom [nall], d_vatom [nall][6] are overwritten"""
        self._check(self.lib.conp_pair_compute_device(self.h, C.c_void_p(d_x), C.c_void_p(d_q), C.c_void_p(d_f), C.c_void_p(d_ev),
                                                      C.c_void_p(d_eatom), C.c_void_p(d_vatom)))

    def pair_build_list_device(self, d_x: int, nlocal: int, nall: int, cutneigh: float, d_tag: int = 0, d_nspecial: int = 0,
                               d_special: int = 0, maxspecial: int = 0, prd_half=(0.0, 0.0, 0.0)):
        """conp_pair_build_list_device: the half list of d_x [nall][3] (raw device pointer) built on the device, in place of
        pair_set_list; d_tag [nall], d_nspecial [nlocal][3], d_special [nlocal][maxspecial] (device pointers, all or none): special
        bonds; prd_half: half the box lengths, 0 for a non-periodic dimension.  May allocate and synchronise"""
        a = conp_pair_build_args(nlocal=int(nlocal), nall=int(nall), cutneigh=float(cutneigh), d_tag=d_tag or None,
                                 d_nspecial=d_nspecial or None, d_special=d_special or None, maxspecial=int(maxspecial),
                                 prd_half=(C.c_double * 3)(*[float(v) for v in prd_half]))
        self._check(self.lib.conp_pair_build_list_device(self.h, C.c_void_p(d_x), C.byref(a)))

    # -- neigh_modify exclude in the device build --------------------------------------------------
    def pair_set_exclusions(self, ntypes=0, type_pairs=(), group_pairs=(), molecule=(), clear=False):
        """conp_pair_set_exclusions: type_pairs [(ti, tj)] 1-based, group_pairs [(bit1, bit2)] LAMMPS group bit masks, molecule
        [(bit, intra)] (intra True: molecule/intra, False: molecule/inter); clear=True passes NULL (every rule cleared)"""
        if clear:
            self._check(self.lib.conp_pair_set_exclusions(self.h, None))
            return
        arr = lambda rows, k: np.ascontiguousarray([int(r[k]) for r in rows], dtype=np.int32)
        ti, tj = arr(type_pairs, 0), arr(type_pairs, 1)
        g1, g2 = arr(group_pairs, 0), arr(group_pairs, 1)
        mb, mi = arr(molecule, 0), arr(molecule, 1)
        ptr = lambda a: _iptr(a) if a.size else None
        e = conp_pair_exclusions(ntypes=int(ntypes), ntype_pairs=ti.size, type_i=ptr(ti), type_j=ptr(tj), ngroup_pairs=g1.size,
                                 group_bit1=ptr(g1), group_bit2=ptr(g2), nmol=mb.size, mol_bit=ptr(mb), mol_intra=ptr(mi))
        self._check(self.lib.conp_pair_set_exclusions(self.h, C.byref(e)))

    def pair_build_list_exclude_device(self, d_x: int, nlocal: int, nall: int, cutneigh: float, d_type: int = 0, d_mask: int = 0,
                                       d_molecule: int = 0, d_tag: int = 0, d_nspecial: int = 0, d_special: int = 0,
                                       maxspecial: int = 0, prd_half=(0.0, 0.0, 0.0)):
        """conp_pair_build_list_exclude_device: pair_build_list_device without the pairs the rules of pair_set_exclusions drop;
        d_type, d_mask, d_molecule [nall] (device pointers, 0 = NULL where no rule in force reads it).  May allocate and synchronise"""
        a = conp_pair_build_args(nlocal=int(nlocal), nall=int(nall), cutneigh=float(cutneigh), d_tag=d_tag or None,
                                 d_nspecial=d_nspecial or None, d_special=d_special or None, maxspecial=int(maxspecial),
                                 prd_half=(C.c_double * 3)(*[float(v) for v in prd_half]))
        at = conp_pair_exclude_atoms(d_type=d_type or None, d_mask=d_mask or None, d_molecule=d_molecule or None)
        self._check(self.lib.conp_pair_build_list_exclude_device(self.h, C.c_void_p(d_x), C.byref(a), C.byref(at)))

    # -- fix zmirror ------------------------------------------------------------------------------
    def zmirror_set_params(self, tag, mask, groupbit, jgroupbit, nevery, boxlo_z, zprd):
        """conp_zmirror_set_params: tag, mask [nlocal] (host); groupbit: the sending group, jgroupbit: the receiving group"""
        tg, mk = np.ascontiguousarray(tag, dtype=np.int32), np.ascontiguousarray(mask, dtype=np.int32)
        p = conp_zmirror_params(nlocal=tg.size, tag=_iptr(tg), mask=_iptr(mk), groupbit=int(groupbit), jgroupbit=int(jgroupbit),
                                nevery=int(nevery), boxlo_z=float(boxlo_z), zprd=float(zprd))
        self._check(self.lib.conp_zmirror_set_params(self.h, C.byref(p)))

    def zmirror_post_integrate_device(self, d_x: int, ntimestep: int = 0):
        """conp_zmirror_post_integrate_device: x[dst] = (x[src][0], x[src][1], zoffset - x[src][2]) on d_x when ntimestep % nevery == 0;
        enqueued on the handle's stream, no synchronisation"""
        self._check(self.lib.conp_zmirror_post_integrate_device(self.h, C.c_void_p(d_x), int(ntimestep)))

    def zmirror_get_map(self):
        """conp_zmirror_get_map -> (src [npairs], dst [npairs]) owned indices, ascending source index"""
        n = C.c_int()
        null = C.POINTER(C.c_int)()
        self._check(self.lib.conp_zmirror_get_map(self.h, C.byref(n), null, null))
        src, dst = np.zeros(max(n.value, 1), np.int32), np.zeros(max(n.value, 1), np.int32)
        self._check(self.lib.conp_zmirror_get_map(self.h, C.byref(n), _iptr(src), _iptr(dst)))
        return src[:n.value], dst[:n.value]

    def pair_list_moved_device(self, d_x: int, trigger: float, d_flag: int):
        """conp_pair_list_moved_device: *d_flag (a device int, overwritten) = an owned atom moved further than `trigger` since the
        build; enqueued on the handle's stream, no synchronisation"""
        self._check(self.lib.conp_pair_list_moved_device(self.h, C.c_void_p(d_x), float(trigger), C.c_void_p(d_flag)))

    def pair_get_list(self):
        """conp_pair_get_list: the list the handle holds, built or uploaded -> (neighbor.NeighList, nall); synchronous"""
        from .neighbor import NeighList
        inum, nall, nn = C.c_int(), C.c_int(), C.c_int64()
        null = C.POINTER(C.c_int)()
        self._check(self.lib.conp_pair_get_list(self.h, C.byref(inum), C.byref(nall), C.byref(nn), null, null, null, null))
        ilist, neigh = np.zeros(max(inum.value, 1), np.int32), np.zeros(max(nn.value, 1), np.int32)
        numneigh, first = np.zeros(max(nall.value, 1), np.int32), np.zeros(max(nall.value, 1), np.int32)
        self._check(self.lib.conp_pair_get_list(self.h, C.byref(inum), C.byref(nall), C.byref(nn), _iptr(ilist), _iptr(numneigh),
                                                _iptr(first), _iptr(neigh)))
        return NeighList(inum=inum.value, ilist=ilist[:inum.value], numneigh=numneigh[:nall.value], first=first[:nall.value],
                         neigh=neigh[:nn.value]), nall.value

    # -- ghost atoms on the device: wrap -> build -> fill / fill_int -> .. -> fold ----------------
    def ghost_build_device(self, d_x: int, nlocal: int, boxlo, boxhi, periodic, cutghost: float) -> int:
        """conp_ghost_build_device: the ghosts of the owned atoms d_x [nlocal][3] (raw device pointer) by the rule of
        neighbor.make_ghosts -> nghost.  May allocate and synchronise"""
        a = conp_ghost_build_args(nlocal=int(nlocal), boxlo=(C.c_double * 3)(*[float(v) for v in boxlo]),
                                  boxhi=(C.c_double * 3)(*[float(v) for v in boxhi]),
                                  periodic=(C.c_int * 3)(*[int(bool(v)) for v in periodic]), cutghost=float(cutghost))
        n = C.c_int(-1)
        self._check(self.lib.conp_ghost_build_device(self.h, C.c_void_p(d_x), C.byref(a), C.byref(n)))
        return n.value

    def ghost_fill_device(self, d_x: int, d_q: int = 0):
        """conp_ghost_fill_device: ghost rows of d_x [nall][3] (and d_q [nall], 0 = NULL) from their owners; enqueued, no synchronisation"""
        self._check(self.lib.conp_ghost_fill_device(self.h, C.c_void_p(d_x), C.c_void_p(d_q)))

    def ghost_fill_int_device(self, d_v: int, width: int = 1):
        """conp_ghost_fill_int_device: ghost rows of the int array d_v [nall][width] (tag, type, mask) from their owners; enqueued"""
        self._check(self.lib.conp_ghost_fill_int_device(self.h, C.c_void_p(d_v), int(width)))

    def ghost_fold_device(self, d_v: int, width: int):
        """conp_ghost_fold_device: ghost rows of d_v [nall][width] (1 eatom, 3 f, 6 vatom) added onto their owners in ascending ghost
        index; ghost rows stay; enqueued, no synchronisation"""
        self._check(self.lib.conp_ghost_fold_device(self.h, C.c_void_p(d_v), int(width)))

    def ghost_get(self):
        """conp_ghost_get -> (nlocal, nghost, owner [nghost], img [nghost][3]); synchronous"""
        nl, ng = C.c_int(), C.c_int()
        null = C.POINTER(C.c_int)()
        self._check(self.lib.conp_ghost_get(self.h, C.byref(nl), C.byref(ng), null, null))
        owner, img = np.zeros(max(ng.value, 1), np.int32), np.zeros((max(ng.value, 1), 3), np.int32)
        self._check(self.lib.conp_ghost_get(self.h, C.byref(nl), C.byref(ng), _iptr(owner), _iptr(img)))
        return nl.value, ng.value, owner[:ng.value], img[:ng.value]

    def atoms_wrap_device(self, d_x: int, nlocal: int, boxlo, boxhi, periodic, d_image: int = 0):
        """conp_atoms_wrap_device: owned atoms d_x [nlocal][3] remapped into the box, d_image [nlocal][3] int counters (0 = NULL);
        enqueued, no synchronisation"""
        lo, hi = np.ascontiguousarray(boxlo, dtype=np.float64), np.ascontiguousarray(boxhi, dtype=np.float64)
        per = np.ascontiguousarray([int(bool(v)) for v in periodic], dtype=np.int32)
        self._check(self.lib.conp_atoms_wrap_device(self.h, C.c_void_p(d_x), int(nlocal), _dptr(lo), _dptr(hi), _iptr(per),
                                                    C.c_void_p(d_image)))

    # -- the fix re-neighboured on the device ------------------------------------------------------
    def post_neighbor_device(self, d_x: int, d_q: int):
        """conp_fix_post_neighbor_device: the fix's tables rebuilt from the handle's own list and ghost map and the owned rows of
        d_x [nall][3], d_q [nall] (raw device pointers); synchronous"""
        self._check(self.lib.conp_fix_post_neighbor_device(self.h, C.c_void_p(d_x), C.c_void_p(d_q)))

    # -- the Gaussian correction on the device ------------------------------------------------------
    def post_force_device(self, d_x: int, d_q: int, d_f: int = 0, d_out: int = 0):
        """conp_fix_post_force_device: raw device pointers (0 = NULL), enqueued on the handle's stream, no synchronisation; d_f [nall][3]
        is added to, d_out [9] (self energy, eng_coul, virial xx, yy, zz, xy, xz, yz, contributing pairs) is overwritten"""
        self._check(self.lib.conp_fix_post_force_device(self.h, C.c_void_p(d_x), C.c_void_p(d_q), C.c_void_p(d_f), C.c_void_p(d_out)))

    # -- the transposed lists and the atomic-free twins of the two pair entries ----------------------
    def pair_transpose_list_device(self):
        """conp_pair_transpose_list_device: the transposed index of the pair style's list, after every pair_set_list or list build;
        may allocate and synchronise"""
        self._check(self.lib.conp_pair_transpose_list_device(self.h))

    def fix_transpose_list_device(self):
        """conp_fix_transpose_list_device: the transposed index of the fix's own half list, after every (setup_)post_neighbor or
        post_neighbor_device; may allocate and synchronise"""
        self._check(self.lib.conp_fix_transpose_list_device(self.h))

    def pair_get_transposed_list(self, which: int = 0):
        """conp_pair_get_transposed_list: which 0 the pair style's index, 1 the fix's -> (own_row [nall], tr_ptr [nall + 1],
        tr_entry [n]); synchronous"""
        nall, n = C.c_int(), C.c_int64()
        null = C.POINTER(C.c_int)()
        self._check(self.lib.conp_pair_get_transposed_list(self.h, int(which), C.byref(nall), C.byref(n), null, null, null))
        own, ptr = np.zeros(max(nall.value, 1), np.int32), np.zeros(nall.value + 1, np.int32)
        ent = np.zeros(max(n.value, 1), np.int32)
        self._check(self.lib.conp_pair_get_transposed_list(self.h, int(which), C.byref(nall), C.byref(n), _iptr(own), _iptr(ptr),
                                                           _iptr(ent)))
        return own[:nall.value], ptr, ent[:n.value]

    def pair_compute_ordered_device(self, d_x: int, d_q: int, d_f: int = 0, d_ev: int = 0, d_eatom: int = 0, d_vatom: int = 0):
        """conp_pair_compute_ordered_device: pair_compute_device without a float atomic -- every output byte-identical from call to
        call; needs pair_transpose_list_device after the list"""
        self._check(self.lib.conp_pair_compute_ordered_device(self.h, C.c_void_p(d_x), C.c_void_p(d_q), C.c_void_p(d_f),
                                                              C.c_void_p(d_ev), C.c_void_p(d_eatom), C.c_void_p(d_vatom)))

    def post_force_ordered_device(self, d_x: int, d_q: int, d_f: int = 0, d_out: int = 0):
        """conp_fix_post_force_ordered_device: post_force_device without a float atomic; needs fix_transpose_list_device after the
        fix's re-neighbouring"""
        self._check(self.lib.conp_fix_post_force_ordered_device(self.h, C.c_void_p(d_x), C.c_void_p(d_q), C.c_void_p(d_f),
                                                                C.c_void_p(d_out)))

    # -- compute potential/atom on the device ---------------------------------------------------------
    def potential_atom_device(self, d_x: int, d_q: int, d_flags: int, ntargets: int, d_targets: int, d_pot: int, eta=0.0, pair=True,
                              kspace=True, qsum=True, reuse_kspace=False):
        """conp_potential_atom_device: compute_potential_atom on device arrays, enqueued on the handle's stream.  d_flags [nall]
        int32 (bit 0 selected, bit 1 eta_check), d_targets [ntargets] int32 the selected owned rows ascending (potential_selection
        makes both); d_pot [ntotal] float64 overwritten.  reuse_kspace: project from what the last device k-space force entry left.
        With newton on the caller folds: ghost_fold_device(d_pot, 1)"""
        pa = conp_potential_args(pairflag=int(pair), kspaceflag=int(kspace), qsumflag=int(qsum), eta=float(eta))
        self._check(self.lib.conp_potential_atom_device(self.h, C.c_void_p(d_x), C.c_void_p(d_q), C.c_void_p(d_flags), int(ntargets),
                                                        C.c_void_p(d_targets), C.byref(pa), int(bool(reuse_kspace)), C.c_void_p(d_pot)))

    STEP_TABLES = ("elyte_idx", "ele_pairs", "csr_ptr", "csr_of", "csr_row", "b_rowptr", "b_ele", "b_oth", "g0c")

    # -- harmonic bonds and angles: set_params -> set_lists -> compute / compute_device ----------
    def bonded_set_params(self, bond_k=(), bond_r0=(), angle_k=(), angle_theta0=(), newton_bond=True):
        """conp_bonded_set_params: per-type coefficients WITHOUT the unused entry 0 (bond type t reads bond_k[t - 1]); theta0 in
        radians; copied by the library.  Drops the handle's bonded lists"""
        tab = lambda a: np.ascontiguousarray(np.concatenate([[0.0], np.asarray(a, dtype=np.float64).reshape(-1)]))
        bk, br, ak, a0 = tab(bond_k), tab(bond_r0), tab(angle_k), tab(angle_theta0)
        assert bk.size == br.size and ak.size == a0.size
        p = conp_bonded_params(nbondtypes=bk.size - 1, nangletypes=ak.size - 1, bond_k=_dptr(bk), bond_r0=_dptr(br),
                               angle_k=_dptr(ak), angle_theta0=_dptr(a0), newton_bond=int(newton_bond))
        self._check(self.lib.conp_bonded_set_params(self.h, C.byref(p)))

    def bonded_set_lists(self, nlocal, nall, bonds=None, angles=None, prd=(0.0, 0.0, 0.0)):
        """conp_bonded_set_lists: bonds [nbond][3] (i1, i2, type), angles [nangle][4] (i1, i2, i3, type; i2 the centre), local
        indices below nall; prd > 0: closest image along that dimension.  Copied and uploaded; may allocate and synchronise"""
        b = np.ascontiguousarray(np.zeros((0, 3)) if bonds is None else bonds, dtype=np.int32).reshape(-1, 3)
        a = np.ascontiguousarray(np.zeros((0, 4)) if angles is None else angles, dtype=np.int32).reshape(-1, 4)
        l = conp_bonded_lists(nlocal=int(nlocal), nall=int(nall), nbond=b.shape[0], bond=_iptr(b) if b.size else None,
                              nangle=a.shape[0], angle=_iptr(a) if a.size else None, prd=(C.c_double * 3)(*prd))
        self._check(self.lib.conp_bonded_set_lists(self.h, C.byref(l)))

    def bonded_compute(self, at, forces=True, eng=True, virial=True, eatom=True, vatom=True, f=None):
        """conp_bonded_compute on host arrays (only at.x is read) -> (f [nall][3] (added to `f`, zeros by default), eng [2] = ebond,
        eangle, W [6], eatom [nall], vatom [nall][6]); what was not asked for is None"""
        n = at.nlocal + at.nghost
        if forces:
            f = np.zeros((n, 3)) if f is None else f
            assert f.dtype == np.float64 and f.flags.c_contiguous and f.shape == (n, 3)
        else:
            f = None
        e2 = np.full(2, np.nan) if eng else None
        w = np.full(6, np.nan) if virial else None
        ea = np.full(n, np.nan) if eatom else None
        va = np.full((n, 6), np.nan) if vatom else None
        ptr = lambda a: _dptr(a) if a is not None else None
        self._check(self.lib.conp_bonded_compute(self.h, C.byref(self.atoms_view(at)), ptr(f), ptr(e2), ptr(w), ptr(ea), ptr(va)))
        return f, e2, w, ea, va

    def bonded_compute_device(self, d_x: int, d_f: int = 0, d_ev: int = 0, d_eatom: int = 0, d_vatom: int = 0):
        """conp_bonded_compute_device: raw device pointers (0 = NULL), enqueued on the handle's stream, no synchronisation; d_f [nall][3]
        is added to, d_ev [8] (ebond, eangle, virial xx, yy, zz, xy, xz, yz), d_eatom [nall], d_vatom [nall][6] are overwritten"""
        self._check(self.lib.conp_bonded_compute_device(self.h, C.c_void_p(d_x), C.c_void_p(d_f), C.c_void_p(d_ev),
                                                        C.c_void_p(d_eatom), C.c_void_p(d_vatom)))

    # -- dihedrals (opls, harmonic) and impropers (harmonic, cvff): set_params -> set_lists -> compute / compute_device (section 28) --
    DIHEDRAL_STYLES = {None: 0, "none": 0, "opls": 1, "harmonic": 2}
    IMPROPER_STYLES = {None: 0, "none": 0, "harmonic": 1, "cvff": 2}

    def dihedral_set_params(self, dihedral_style=None, dihedral_coef=(), improper_style=None, improper_coef=(), newton_bond=True):
        """conp_dihedral_set_params: styles by name (None: no such terms); the coefficient rows WITHOUT the unused row 0 and without
        the padding to four columns (dihedral type t reads dihedral_coef[t - 1]): opls K1 K2 K3 K4, harmonic and cvff K d n, improper
        harmonic K chi0 in radians; copied by the library.  Drops the handle's dihedral lists"""
        def tab(rows):
            r = np.asarray(rows, dtype=np.float64)
            r = r.reshape(-1, r.shape[-1] if r.ndim == 2 else 4)
            t = np.zeros((len(r) + 1, 4))
            t[1:, :r.shape[1]] = r
            return np.ascontiguousarray(t)
        dc, ic = tab(dihedral_coef), tab(improper_coef)
        p = conp_dihedral_params(dihedral_style=self.DIHEDRAL_STYLES[dihedral_style], ndihedraltypes=len(dc) - 1, dihedral_coef=_dptr(dc),
                                 improper_style=self.IMPROPER_STYLES[improper_style], nimpropertypes=len(ic) - 1, improper_coef=_dptr(ic),
                                 newton_bond=int(newton_bond))
        self._check(self.lib.conp_dihedral_set_params(self.h, C.byref(p)))

    def dihedral_set_lists(self, nlocal, nall, dihedrals=None, impropers=None, prd=(0.0, 0.0, 0.0)):
        """conp_dihedral_set_lists: dihedrals and impropers [n][5] (i1, i2, i3, i4, type), local indices below nall; prd > 0: closest
        image along that dimension.  Copied and uploaded; may allocate and synchronise"""
        d = np.ascontiguousarray(np.zeros((0, 5)) if dihedrals is None else dihedrals, dtype=np.int32).reshape(-1, 5)
        i = np.ascontiguousarray(np.zeros((0, 5)) if impropers is None else impropers, dtype=np.int32).reshape(-1, 5)
        l = conp_dihedral_lists(nlocal=int(nlocal), nall=int(nall), ndihedral=d.shape[0], dihedral=_iptr(d) if d.size else None,
                                nimproper=i.shape[0], improper=_iptr(i) if i.size else None, prd=(C.c_double * 3)(*prd))
        self._check(self.lib.conp_dihedral_set_lists(self.h, C.byref(l)))

    def dihedral_compute(self, at, forces=True, eng=True, virial=True, eatom=True, vatom=True, f=None):
        """conp_dihedral_compute on host arrays (only at.x is read) -> (f [nall][3] (added to `f`, zeros by default), eng [2] =
        edihedral, eimproper, W [6], eatom [nall], vatom [nall][6]); what was not asked for is None"""
        n = at.nlocal + at.nghost
        if forces:
            f = np.zeros((n, 3)) if f is None else f
            assert f.dtype == np.float64 and f.flags.c_contiguous and f.shape == (n, 3)
        else:
            f = None
        e2 = np.full(2, np.nan) if eng else None
        w = np.full(6, np.nan) if virial else None
        ea = np.full(n, np.nan) if eatom else None
        va = np.full((n, 6), np.nan) if vatom else None
        ptr = lambda a: _dptr(a) if a is not None else None
        self._check(self.lib.conp_dihedral_compute(self.h, C.byref(self.atoms_view(at)), ptr(f), ptr(e2), ptr(w), ptr(ea), ptr(va)))
        return f, e2, w, ea, va

    def dihedral_compute_device(self, d_x: int, d_f: int = 0, d_ev: int = 0, d_eatom: int = 0, d_vatom: int = 0):
        """conp_dihedral_compute_device: raw device pointers (0 = NULL), enqueued on the handle's stream, no synchronisation; d_f
        [nall][3] is added to, d_ev [8] (edihedral, eimproper, virial xx, yy, zz, xy, xz, yz), d_eatom [nall], d_vatom [nall][6] are
        overwritten"""
        self._check(self.lib.conp_dihedral_compute_device(self.h, C.c_void_p(d_x), C.c_void_p(d_f), C.c_void_p(d_ev),
                                                          C.c_void_p(d_eatom), C.c_void_p(d_vatom)))

    # -- SHAKE constraints: set_params -> correct_device at a run's start, setup_device, post_force_device per step (section 23) ------
    def shake_set_params(self, type, mass, bond_distance, angle_distance, cluster, tolerance, max_iter, dt, ftm2v, prd=(0.0, 0.0, 0.0)):
        """conp_shake_set_params: type [nlocal] (1..ntypes); mass, bond_distance, angle_distance per type WITHOUT the unused entry 0;
        cluster [ncluster][7] = flag, i0, i1, i2, t0, t1, t2 (flag 2: one bond, 3: two bonds, 1: two bonds and the angle).  Copied and
        uploaded; may allocate and synchronise"""
        ty = np.ascontiguousarray(type, dtype=np.int32).reshape(-1)
        lead = lambda a: np.ascontiguousarray(np.concatenate([[0.0], np.asarray(a, dtype=np.float64).reshape(-1)]))
        m, bd, ad = lead(mass), lead(bond_distance), lead(angle_distance)
        cl = np.ascontiguousarray(cluster, dtype=np.int32).reshape(-1, 7)
        p = conp_shake_params(nlocal=ty.size, ntypes=m.size - 1, type=_iptr(ty) if ty.size else None, mass=_dptr(m),
                              nbondtypes=bd.size - 1, nangletypes=ad.size - 1, bond_distance=_dptr(bd), angle_distance=_dptr(ad),
                              ncluster=cl.shape[0], cluster=_iptr(cl) if cl.size else None, tolerance=tolerance, max_iter=int(max_iter),
                              dt=dt, ftm2v=ftm2v, prd=(C.c_double * 3)(*prd))
        self._check(self.lib.conp_shake_set_params(self.h, C.byref(p)))

    def shake_correct_device(self, d_x: int):
        """conp_shake_correct_device: moves the cluster atoms of d_x [nlocal][3] onto the constraints (to the tolerance); one launch"""
        self._check(self.lib.conp_shake_correct_device(self.h, C.c_void_p(d_x)))

    def shake_setup_device(self, d_x: int, d_v: int, d_f: int, d_out: int = 0):
        """conp_shake_setup_device: the constraint force of a run's start (dtfsq = 0.5 dt dt ftm2v) added to d_f; d_out [9] or 0"""
        self._check(self.lib.conp_shake_setup_device(self.h, C.c_void_p(d_x), C.c_void_p(d_v), C.c_void_p(d_f), C.c_void_p(d_out)))

    def shake_post_force_device(self, d_x: int, d_v: int, d_f: int, d_out: int = 0, d_vatom: int = 0):
        """conp_shake_post_force_device: the constraint force added to d_f [nlocal][3]; d_out [9] (virial xx, yy, zz, xy, xz, yz,
        unconverged clusters, bad determinants, largest niter) and d_vatom [nlocal][6] are overwritten (0 = NULL); no synchronisation"""
        self._check(self.lib.conp_shake_post_force_device(self.h, C.c_void_p(d_x), C.c_void_p(d_v), C.c_void_p(d_f), C.c_void_p(d_out),
                                                          C.c_void_p(d_vatom)))

    def shake_check_device(self, d_x: int, d_out: int):
        """conp_shake_check_device: d_out [2] = largest |r - d| / d over the bonds, over the 1-2 distances of the flag-1 clusters"""
        self._check(self.lib.conp_shake_check_device(self.h, C.c_void_p(d_x), C.c_void_p(d_out)))

    # -- fix efield and the per-group thermo sums: set_params once, the device entries per step / per thermo output (section 24) ------
    def efield_set_params(self, sel, qe2f, prd=(0.0, 0.0, 0.0)):
        """conp_efield_set_params: sel [nlocal] 0 / 1 (the atoms the field acts on), force->qe2f, the box lengths d_image counts.
        Copied and uploaded; may allocate and synchronise"""
        se = np.ascontiguousarray(sel, dtype=np.int32).reshape(-1)
        p = conp_efield_params(nlocal=se.size, sel=_iptr(se) if se.size else None, qe2f=qe2f, prd=(C.c_double * 3)(*prd))
        self._check(self.lib.conp_efield_set_params(self.h, C.byref(p)))

    def efield_post_force_device(self, d_x: int, d_q: int, d_f: int, e, d_image: int = 0, couple: int = 0, couple_scale: float = 0.0,
                                 d_out: int = 0, d_vatom: int = 0):
        """conp_efield_post_force_device: q E added to the selected rows of d_f [nlocal][3]; e = (ex, ey, ez) on the host, V / length;
        couple 1: ez = qe2f (e[2] + couple_scale s) with s the fix scalar the last update of this conq / cond handle left on the
        device.  d_out [11] (energy, sum f [3], virial [6], selected atoms) and d_vatom [nlocal][6] are overwritten (0 = NULL);
        enqueued, no synchronisation"""
        ev = np.ascontiguousarray(e, dtype=np.float64).reshape(3)
        self._check(self.lib.conp_efield_post_force_device(self.h, C.c_void_p(d_x), C.c_void_p(d_q), C.c_void_p(d_image), C.c_void_p(d_f),
                                                           _dptr(ev), int(couple), float(couple_scale), C.c_void_p(d_out),
                                                           C.c_void_p(d_vatom)))

    def observe_set_params(self, type, mask, mass, ngroups, prd=(0.0, 0.0, 0.0)):
        """conp_observe_set_params: type [nlocal] (1..ntypes), mask [nlocal] (bit g = member of group g; groups may overlap), mass per
        type WITHOUT the unused entry 0.  Copied and uploaded; may allocate and synchronise"""
        ty = np.ascontiguousarray(type, dtype=np.int32).reshape(-1)
        mk = np.ascontiguousarray(mask, dtype=np.int32).reshape(-1)
        assert ty.size == mk.size
        m = np.ascontiguousarray(np.concatenate([[0.0], np.asarray(mass, dtype=np.float64).reshape(-1)]))
        p = conp_observe_params(nlocal=ty.size, ntypes=m.size - 1, ngroups=int(ngroups), type=_iptr(ty) if ty.size else None,
                                mask=_iptr(mk) if mk.size else None, mass=_dptr(m), prd=(C.c_double * 3)(*prd))
        self._check(self.lib.conp_observe_set_params(self.h, C.byref(p)))

    def observe_device(self, d_x: int, d_q: int, d_out: int, d_v: int = 0, d_image: int = 0):
        """conp_observe_device: d_out [ngroups][10] = per group the member count, sum q, sum q u [3], sum m v.v, sum m v [3], sum m
        (u unwrapped with d_image; columns 5-8 are 0.0 without d_v); enqueued, no synchronisation"""
        self._check(self.lib.conp_observe_device(self.h, C.c_void_p(d_x), C.c_void_p(d_q), C.c_void_p(d_v), C.c_void_p(d_image),
                                                 C.c_void_p(d_out)))

    # -- velocity Verlet and Nose-Hoover chains: set_params -> setup_device -> initial / final per step ------
    def integrate_set_params(self, type, group, mass, style, dof, t_period, dt, ftm2v, mvv2e, boltz):
        """conp_integrate_set_params: type [nlocal] (1..ntypes), group [nlocal] (-1 = not integrated), mass per type WITHOUT the unused
        entry 0, style / dof / t_period per group (style 0 = nve, 1 = nvt).  Copied and uploaded; zeroes every chain"""
        ty = np.ascontiguousarray(type, dtype=np.int32).reshape(-1)
        gr = np.ascontiguousarray(group, dtype=np.int32).reshape(-1)
        assert ty.size == gr.size
        m = np.ascontiguousarray(np.concatenate([[0.0], np.asarray(mass, dtype=np.float64).reshape(-1)]))
        st = np.ascontiguousarray(style, dtype=np.int32).reshape(-1)
        df = np.ascontiguousarray(dof, dtype=np.float64).reshape(-1)
        tp = np.ascontiguousarray(t_period, dtype=np.float64).reshape(-1)
        assert st.size == df.size == tp.size
        p = conp_integrate_params(nlocal=ty.size, ntypes=m.size - 1, ngroups=st.size, type=_iptr(ty), group=_iptr(gr), mass=_dptr(m),
                                  style=_iptr(st), dof=_dptr(df), t_period=_dptr(tp), dt=dt, ftm2v=ftm2v, mvv2e=mvv2e, boltz=boltz)
        self._integrate_ngroups = 0
        self._check(self.lib.conp_integrate_set_params(self.h, C.byref(p)))
        self._integrate_ngroups = int(st.size)

    def _integrate_targets(self, t_target):
        if t_target is None:
            return None, None
        t = np.ascontiguousarray(t_target, dtype=np.float64).reshape(-1)
        assert t.size == getattr(self, "_integrate_ngroups", t.size)
        return t, _dptr(t)

    def integrate_setup_device(self, d_v: int, t_target=None):
        """conp_integrate_setup_device: raw device pointer d_v [nlocal][3], t_target a host array [ngroups]; enqueued, no synchronisation"""
        keep, tp = self._integrate_targets(t_target)
        self._check(self.lib.conp_integrate_setup_device(self.h, C.c_void_p(d_v), tp))

    def integrate_initial_device(self, d_x: int, d_v: int, d_f: int, t_target=None):
        """conp_integrate_initial_device: chain half-step, v *= factor_eta, v += dtfm f, x += dtv v; one launch, no synchronisation"""
        keep, tp = self._integrate_targets(t_target)
        self._check(self.lib.conp_integrate_initial_device(self.h, C.c_void_p(d_x), C.c_void_p(d_v), C.c_void_p(d_f), tp))

    def integrate_final_device(self, d_v: int, d_f: int, d_out: int = 0):
        """conp_integrate_final_device: v += dtfm f, temperature, chain half-step, v *= factor_eta; d_out [ngroups][4] (t_current, ke,
        thermostat energy, eta_dot[0]) is overwritten (0 = NULL); no synchronisation"""
        self._check(self.lib.conp_integrate_final_device(self.h, C.c_void_p(d_v), C.c_void_p(d_f), C.c_void_p(d_out)))

    def integrate_temperature_device(self, d_v: int, d_out: int):
        """conp_integrate_temperature_device: d_out [ngroups][4] of d_v and the chains as they are; nothing is stored"""
        self._check(self.lib.conp_integrate_temperature_device(self.h, C.c_void_p(d_v), C.c_void_p(d_out)))

    def integrate_get_state(self):
        """conp_integrate_get_state -> [ngroups][8]: eta[3], eta_dot[3], t_current, t_target per group (synchronises)"""
        st = np.full((max(getattr(self, "_integrate_ngroups", 0), 1), 8), np.nan)
        self._check(self.lib.conp_integrate_get_state(self.h, _dptr(st)))
        return st[:self._integrate_ngroups]

    def integrate_set_state(self, state):
        """conp_integrate_set_state: [ngroups][8] as integrate_get_state returns it; counts as the setup (synchronises)"""
        st = np.ascontiguousarray(state, dtype=np.float64).reshape(-1, 8)
        assert st.shape[0] == getattr(self, "_integrate_ngroups", st.shape[0])
        self._check(self.lib.conp_integrate_set_state(self.h, _dptr(st)))

    def step_tables(self):
        """conp_fix_get_step_tables -> dict of the sizes (nl, n_ele_atoms, ne, n_b_pairs, n_chunks, zn_listed, nall, c_start) and the
        arrays of STEP_TABLES, after a host or a device post_neighbor; synchronous"""
        sizes = np.zeros(8, np.int64)
        sp = sizes.ctypes.data_as(C.POINTER(C.c_int64))
        null = C.POINTER(C.c_int)()
        self._check(self.lib.conp_fix_get_step_tables(self.h, sp, *([null] * 9)))
        nl, nea, ne, nbp, nch = (int(v) for v in sizes[:5])
        lens = dict(elyte_idx=nl, ele_pairs=2 * nea, csr_ptr=ne + 1, csr_of=nea, csr_row=nea, b_rowptr=ne + 1, b_ele=nbp, b_oth=nbp, g0c=nch)
        arr = {k: np.full(max(lens[k], 1), -7, np.int32) for k in self.STEP_TABLES}
        self._check(self.lib.conp_fix_get_step_tables(self.h, sp, *[_iptr(arr[k]) for k in self.STEP_TABLES]))
        out = {k: arr[k][:lens[k]] for k in self.STEP_TABLES}
        out["ele_pairs"] = out["ele_pairs"].reshape(-1, 2)
        out.update(nl=nl, n_ele_atoms=nea, ne=ne, n_b_pairs=nbp, n_chunks=nch, zn_listed=int(sizes[5]), nall=int(sizes[6]),
                   c_start=int(sizes[7]))
        return out

    def profile(self, enable):
        """0 off, 1 events around every kernel, 2 around the dominant kernel only (conp_hip.h)"""
        self._check(self.lib.conp_fix_profile(self.h, int(enable)))

    def profile_read(self):
        n = C.c_int()
        names = (C.c_char_p * 16)()
        ms = (C.c_double * 16)()
        cnt = (C.c_int * 16)()
        self._check(self.lib.conp_fix_profile_read(self.h, C.byref(n), names, ms, cnt))
        return {names[i].decode(): (ms[i], cnt[i]) for i in range(n.value)}

    def write_timing(self):
        """the three timing lines of fix_conp.cpp:564-566 go to the log buffer"""
        self._check(self.lib.conp_fix_write_timing(self.h))

    def log_drain(self):
        """text the reference would have printed to its log file (fix_conp.cpp:119) since the last drain"""
        return self.lib.conp_fix_log_drain(self.h).decode()

    def mesg_drain(self):
        """the `conp output: <e,e>` / `<d,d>` lines of fix_conp.cpp:1006-1009, 458-461"""
        return self.lib.conp_fix_mesg_drain(self.h).decode()

    def close(self):
        if self.h:
            self.lib.conp_fix_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _uneven_all_gather(outs, mine, group, world):
    """all_gather with different lengths per rank: pad to the longest (the collectives want equal sizes), trim after"""
    import torch
    import torch.distributed as dist
    nmax = max(o.numel() for o in outs)
    pad = torch.zeros(nmax, dtype=torch.uint8)
    pad[: mine.numel()] = mine
    bufs = [torch.zeros(nmax, dtype=torch.uint8) for _ in range(world)]
    dist.all_gather(bufs, pad, group=group)
    for r in range(world):
        outs[r].copy_(bufs[r][: outs[r].numel()])


# ---- host-only helpers (no GPU needed) -----------------------------------------------------------------------------
def host_ktables(s: "_systems.System"):
    lib = load_library()
    info = np.zeros(16, np.int32)
    args = (s.g_ewald, s.accuracy, s.slab_volfactor, int(s.slabflag), float(s.prd[0]), float(s.prd[1]), float(s.prd[2]), s.qsqsum,
            int(s.natoms), _systems.QQRD2E, 1.0)
    null_i, null_d = C.POINTER(C.c_int)(), C.POINTER(C.c_double)()
    rc = lib.conp_host_ktables(*args, _iptr(info), null_i, null_i, null_i, null_d, null_i, null_i, null_i, null_i, null_i)
    if rc:
        raise ConpError(rc, lib.conp_last_error().decode())
    K, E = int(info[0]), max(int(info[2]), 1)
    out = dict(kxvecs=np.zeros(K, np.int32), kyvecs=np.zeros(K, np.int32), kzvecs=np.zeros(K, np.int32), ug=np.zeros(K),
               kxy_list=np.zeros(E, np.int32), kz_list=np.zeros(E, np.int32), plan_p=np.zeros(K, np.int32),
               plan_m=np.zeros(K, np.int32), plan_sign=np.zeros(K, np.int32))
    rc = lib.conp_host_ktables(*args, _iptr(info), _iptr(out["kxvecs"]), _iptr(out["kyvecs"]), _iptr(out["kzvecs"]), _dptr(out["ug"]),
                               _iptr(out["kxy_list"]), _iptr(out["kz_list"]), _iptr(out["plan_p"]), _iptr(out["plan_m"]),
                               _iptr(out["plan_sign"]))
    if rc:
        raise ConpError(rc, lib.conp_last_error().decode())
    out["kxy_list"] = out["kxy_list"][:int(info[2])]; out["kz_list"] = out["kz_list"][:int(info[2])]
    out.update(kcount=K, kcount_flat=int(info[1]), kcount_expand=int(info[2]), kxmax=int(info[3]), kymax=int(info[4]),
               kzmax=int(info[5]), kmax=int(info[6]), kmax3d=int(info[7]), kcount_dims=info[8:15].copy(), n_planar=int(info[15]))
    return out


def host_index(tag0, echeck0, tag1=None, echeck1=None):
    lib = load_library()
    tag0 = np.ascontiguousarray(tag0, np.int32); echeck0 = np.ascontiguousarray(echeck0, np.int32)
    if tag1 is None:
        tag1, echeck1, n1 = tag0, echeck0, 0
    else:
        tag1 = np.ascontiguousarray(tag1, np.int32); echeck1 = np.ascontiguousarray(echeck1, np.int32); n1 = len(tag1)
    ne = int((echeck0 != 0).sum()); mt = int(tag0.max())
    sizes = np.zeros(4, np.int32)
    m = dict(ele2tag=np.zeros(ne, np.int32), ele2eleall=np.zeros(ne, np.int32), eleall2tag=np.zeros(ne, np.int32),
             eleall2ele=np.zeros(ne + 1, np.int32), elebuf2eleall=np.zeros(ne, np.int32), tag2eleall=np.zeros(mt + 1, np.int32))
    rc = lib.conp_host_index(len(tag0), _iptr(tag0), _iptr(echeck0), n1, _iptr(tag1), _iptr(echeck1), _iptr(sizes),
                             *[_iptr(m[k]) for k in ("ele2tag", "ele2eleall", "eleall2tag", "eleall2ele", "elebuf2eleall", "tag2eleall")])
    if rc:
        raise ConpError(rc, lib.conp_last_error().decode())
    m["sizes"] = sizes
    return m


def host_pair_rows(which, lst, at, newton=False):
    lib = load_library()
    x = np.ascontiguousarray(at.x, dtype=np.float64)
    neigh = lst.neigh if lst.neigh.size else np.zeros(1, np.int32)
    av = conp_atoms(nlocal=at.nlocal, nghost=at.nghost, x=_dptr(x), q=_dptr(at.q), type=_iptr(at.type), tag=_iptr(at.tag),
                    echeck=_iptr(at.echeck))
    lv = conp_neighlist(inum=lst.inum, ilist=_iptr(lst.ilist), numneigh=_iptr(lst.numneigh), first=_iptr(lst.first),
                        neigh=_iptr(neigh), nneigh=int(lst.neigh.size))
    null_i = C.POINTER(C.c_int)()
    n = lib.conp_host_pair_rows(which, C.byref(lv), C.byref(av), int(newton), null_i, null_i, null_i, null_i)
    if n < 0:
        raise ConpError(-2, lib.conp_last_error().decode())
    ne = int((at.echeck[:at.nlocal] != 0).sum())
    out = dict(row_ptr=np.zeros(ne + 1, np.int32), ele_atom=np.zeros(max(n, 1), np.int32), oth_atom=np.zeros(max(n, 1), np.int32),
               col=np.zeros(max(n, 1), np.int32))
    lib.conp_host_pair_rows(which, C.byref(lv), C.byref(av), int(newton), _iptr(out["row_ptr"]), _iptr(out["ele_atom"]),
                            _iptr(out["oth_atom"]), _iptr(out["col"]))
    for k in ("ele_atom", "oth_atom", "col"):
        out[k] = out[k][:n]
    out["npairs"] = int(n)
    return out
