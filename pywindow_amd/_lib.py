"""ctypes binding of libpywindow_hip.so (C ABI in include/pywindow_amd.h).

There is no CPU fallback: importing this module only loads the shared library;
every compute call needs a HIP device and raises :class:`PwHipError` otherwise.
"""

from __future__ import annotations

import ctypes
import pathlib

import numpy as np

W_MAX = 16
P_MAX = 2048

STAGE_BASIC = 1
STAGE_AVG = 2
STAGE_OPT = 4
STAGE_WINDOWS = 8
STAGE_ALL = 15

ST_NEGATIVE_PORE = 1
ST_WINDOW_OVERFLOW = 2
ST_POINTS_OVERFLOW = 4
ST_WINDOW_DROPPED = 8
ST_WINDOW_NEGATIVE = 16
ST_Z_BOUNDS = 32
ST_TOO_FEW_POINTS = 64
ST_PATH_TOO_LONG = 128

E_RETRY = -6
E_HIP = -3
E_TIMEOUT = -7
DBSCAN_MAX = 8192

_PKG = pathlib.Path(__file__).resolve().parent
LIB_PATH = _PKG / "libpywindow_hip.so"


class PwHipError(RuntimeError):
    """The HIP engine is missing, has no device, or a call failed."""


class PwRetry(PwHipError):
    """``PW_E_RETRY``: a capacity was grown for this batch; launch the analysis again."""


class PwTimeoutError(PwHipError):
    """``PW_E_TIMEOUT``: a launch of the pipeline gave up waiting for another one; the records are incomplete."""


class BatchIn(ctypes.Structure):
    _fields_ = [
        ("n_units", ctypes.c_int64),
        ("atom_offset", ctypes.POINTER(ctypes.c_int64)),
        ("xyz", ctypes.POINTER(ctypes.c_double)),
        ("vdw", ctypes.POINTER(ctypes.c_double)),
        ("mass", ctypes.POINTER(ctypes.c_double)),
        ("template_atoms", ctypes.c_int64),
    ]


class Params(ctypes.Structure):
    """``pw_params``: knobs of find_windows / find_average_diameter (reference defaults)."""

    _fields_ = [
        ("adjust_windows", ctypes.c_double),
        ("adjust_average", ctypes.c_double),
        ("increment", ctypes.c_double),
        ("pore_opt", ctypes.c_int32),
        ("opt_flags", ctypes.c_int32),
        ("opt_x0", ctypes.c_double * 3),
        ("opt_lo", ctypes.c_double * 3),
        ("opt_hi", ctypes.c_double * 3),
        ("increment2", ctypes.c_double),
        ("z_lo", ctypes.c_double),
        ("z_hi", ctypes.c_double),
        ("lb_z", ctypes.c_int32),
        ("z_second_mini", ctypes.c_int32),
    ]

    def __init__(self, adjust_windows=1.0, adjust_average=1.0, increment=1.0, pore_opt=True, opt_start=None,
                 opt_bounds=None, increment2=0.1, z_bounds=None, lb_z=True, z_second_mini=False):
        """``opt_start``: (3,) start of opt_pore_diameter; ``opt_bounds``: three (lo, hi) pairs, ``None``
        for an open side (scipy.optimize.minimize's ``bounds`` convention).  ``increment2``,
        ``z_bounds`` (a (lo, hi) pair), ``lb_z``, ``z_second_mini``: window_analysis's keywords
        (utilities.py:1191-1200)."""
        flags = 0
        x0 = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
        lo = (ctypes.c_double * 3)(-np.inf, -np.inf, -np.inf)
        hi = (ctypes.c_double * 3)(np.inf, np.inf, np.inf)
        if opt_start is not None:
            flags |= 1
            for k in range(3):
                x0[k] = float(opt_start[k])
        if opt_bounds is not None:
            flags |= 2
            for k in range(3):
                a, b = opt_bounds[k]
                lo[k] = -np.inf if a is None else float(a)
                hi[k] = np.inf if b is None else float(b)
        z_lo, z_hi = (None, None) if z_bounds is None else z_bounds
        super().__init__(float(adjust_windows), float(adjust_average), float(increment), 1 if pore_opt else 0,
                         flags, x0, lo, hi, float(increment2),
                         -np.inf if z_lo is None else float(z_lo), np.inf if z_hi is None else float(z_hi),
                         1 if lb_z else 0, 0 if z_second_mini is False else 1)


class CellIn(ctypes.Structure):
    """``pw_cell_in``: frames of one system for ``pw_discrete_molecules``."""

    _fields_ = [
        ("n_frames", ctypes.c_int64),
        ("n_atoms", ctypes.c_int32),
        ("rebuild", ctypes.c_int32),
        ("xyz", ctypes.c_void_p),
        ("lattice", ctypes.c_void_p),
        ("lattice_inv", ctypes.c_void_p),
        ("cov", ctypes.c_void_p),
        ("mass", ctypes.c_void_p),
        ("terminal", ctypes.c_void_p),
        ("max_dist", ctypes.c_double),
        ("tol", ctypes.c_double),
    ]


class CellOut(ctypes.Structure):
    """``pw_cell_out``: caller-allocated result arrays of ``pw_discrete_molecules``."""

    _fields_ = [
        ("atoms_cap", ctypes.c_int32),
        ("mols_cap", ctypes.c_int32),
        ("n_mol", ctypes.c_void_p),
        ("status", ctypes.c_void_p),
        ("mol_offset", ctypes.c_void_p),
        ("src_atom", ctypes.c_void_p),
        ("src_image", ctypes.c_void_p),
        ("xyz", ctypes.c_void_p),
    ]


# PW_RB_NB_CAP of the header = RB_NB_CAP of csrc/pw_rebuild.hpp (a static_assert in pw_rebuild.hip ties those two;
# tests/test_rebuild_edges.py::test_status_text_states_the_constants ties this copy to them)
RB_NB_CAP = 16
RB_NB_OVERFLOW = 1
RB_SEG_OVERFLOW = 2
RB_ATOMS_OVERFLOW = 4
RB_MOLS_OVERFLOW = 8
RB_THIN_CELL = 16


def rb_status_text(bits: int) -> str:
    """What the PW_RB_* bits of a refused frame say (include/pywindow_amd.h)."""
    names = ((RB_NB_OVERFLOW, f"{RB_NB_OVERFLOW} = more than {RB_NB_CAP} candidate partners of one atom"),
             (RB_SEG_OVERFLOW, f"{RB_SEG_OVERFLOW} = more than {2 * RB_NB_CAP} hits of one atom in one layer"),
             (RB_THIN_CELL, f"{RB_THIN_CELL} = a perpendicular height of the cell is below the bond cut-off"))
    said = [text for bit, text in names if bits & bit]
    return f"status bits {bits}: " + "; ".join(said or ["unknown"])

#: numpy mirror of ``pw_unit_out`` (natural C alignment)
UNIT_OUT_DTYPE = np.dtype(
    [
        ("n_atoms", np.int32),
        ("status", np.int32),
        ("mw", np.float64),
        ("com", np.float64, (3,)),
        ("maxd", np.float64),
        ("maxd_i", np.int32),
        ("maxd_j", np.int32),
        ("avg_d", np.float64),
        ("pore_d", np.float64),
        ("pore_atom", np.int32),
        ("pore_opt_atom", np.int32),
        ("pore_vol", np.float64),
        ("pore_opt_d", np.float64),
        ("pore_opt_c", np.float64, (3,)),
        ("pore_vol_opt", np.float64),
        ("n_windows", np.int32),
        ("n_clusters", np.int32),
        ("win_d", np.float64, (W_MAX,)),
        ("win_c", np.float64, (W_MAX, 3)),
        ("n_points", np.int32),
        ("n_points_avg", np.int32),
        ("n_survivors", np.int32),
        ("opt_nit", np.int32),
        ("opt_nfev", np.int32),
        ("opt_task", np.int32),
        ("opt_msg", np.int32),
        ("n_eval", np.int32),
        ("eps", np.float64),
        ("sphere_r", np.float64),
    ],
    align=True,
)

#: numpy mirror of ``pw_kde_job``
KDE_JOB_DTYPE = np.dtype(
    [("sample_first", np.int64), ("n_samples", np.int64), ("point_first", np.int64), ("n_points", np.int64),
     ("inv_bandwidth", np.float64)]
)

#: numpy mirror of ``pw_kde2_job``
KDE2_JOB_DTYPE = np.dtype(
    [("sample_first", np.int64), ("n_samples", np.int64), ("point_first", np.int64), ("n_points", np.int64),
     ("w00", np.float64), ("w10", np.float64), ("w11", np.float64)]
)

#: numpy mirror of ``pw_kdew_job``
KDEW_JOB_DTYPE = np.dtype(
    [("n_samples", np.int64), ("n_points", np.int64), ("n_replicas", np.int64), ("sample_first", np.int64),
     ("point_first", np.int64), ("weight_first", np.int64), ("out_first", np.int64), ("inv_bandwidth", np.float64)]
)

#: numpy mirror of ``pw_corr_job``
CORR_JOB_DTYPE = np.dtype(
    [("a_first", np.int64), ("b_first", np.int64), ("n", np.int64), ("out_first", np.int64), ("n_lags", np.int64)]
)

#: numpy mirror of ``pw_dft_job``
DFT_JOB_DTYPE = np.dtype(
    [("a_first", np.int64), ("n", np.int64), ("period", np.int64), ("j_first", np.int64), ("j_step", np.int64),
     ("n_freq", np.int64), ("out_first", np.int64)]
)

#: numpy mirror of ``pw_gate_job``
GATE_JOB_DTYPE = np.dtype(
    [("a_first", np.int64), ("n", np.int64), ("d_first", np.int64), ("n_thr", np.int64), ("out_first", np.int64)]
)
#: the columns of a row of ``pw_gate_counts`` (``PW_GATE_FIELDS``)
GATE_FIELDS = ("n_open", "n_closed", "open_runs", "closed_runs", "longest_open", "longest_closed", "openings", "closings",
               "complete_open_runs", "complete_closed_runs", "complete_open_frames", "complete_closed_frames")

#: numpy mirror of ``pw_trans_job``
TRANS_JOB_DTYPE = np.dtype(
    [("a_first", np.int64), ("n", np.int64), ("e_first", np.int64), ("n_edges", np.int64), ("lag_first", np.int64),
     ("lag_step", np.int64), ("n_lags", np.int64), ("out_first", np.int64)]
)
#: ``PW_TRANS_MAX_STATES``
TRANS_MAX_STATES = 16

#: numpy mirror of ``pw_superpose_job``
SUPERPOSE_JOB_DTYPE = np.dtype(
    [("mobile_first", np.int64), ("target_first", np.int64), ("weight_first", np.int64), ("n", np.int64), ("out", np.int64)]
)
#: numpy mirror of ``pw_superpose_out``
SUPERPOSE_OUT_DTYPE = np.dtype(
    [("rotation", np.float64, (3, 3)), ("centre_mobile", np.float64, (3,)), ("centre_target", np.float64, (3,)),
     ("rmsd", np.float64), ("lambda", np.float64, (2,)), ("sweeps", np.int32), ("reserved", np.int32)],
)
assert SUPERPOSE_OUT_DTYPE.itemsize == 152

#: numpy mirror of ``pw_cluster_job``
CLUSTER_JOB_DTYPE = np.dtype(
    [("d_first", np.int64), ("n", np.int64), ("cutoff", np.float64), ("out_first", np.int64)]
)
#: ``PW_CLUSTER_MAX_N``
CLUSTER_MAX_N = 32768

#: numpy mirror of ``pw_cov_job``
COV_JOB_DTYPE = np.dtype(
    [("x_first", np.int64), ("T", np.int64), ("D", np.int64), ("transform_first", np.int64), ("mean_first", np.int64),
     ("s_first", np.int64)]
)
#: numpy mirror of ``pw_project_job``
PROJECT_JOB_DTYPE = np.dtype(
    [("x_first", np.int64), ("T", np.int64), ("D", np.int64), ("transform_first", np.int64), ("mean_first", np.int64),
     ("v_first", np.int64), ("k", np.int64), ("p_first", np.int64)]
)
#: ``PW_COV_CHUNK``, ``PW_COV_MAX_D``
COV_CHUNK = 256
COV_MAX_D = 3072

#: numpy mirror of ``pw_cavity_job``
CAVITY_JOB_DTYPE = np.dtype(
    [("atom_first", np.int64), ("n", np.int64), ("radius_first", np.int64), ("plane_first", np.int64), ("m", np.int64),
     ("mask_first", np.int64), ("out", np.int64), ("origin", np.float64, (3,)), ("spacing", np.float64),
     ("probe", np.float64), ("nx", np.int32), ("ny", np.int32), ("nz", np.int32), ("seed", np.int32, (3,))]
)
#: numpy mirror of ``pw_cavity_out``
CAVITY_OUT_DTYPE = np.dtype(
    [("n_voxels", np.int64), ("n_open", np.int64), ("n_surface", np.int64), ("n_face", np.int64),
     ("first", np.int64, (3,)), ("second", np.int64, (6,)), ("box", np.int32, (6,)), ("flags", np.int32),
     ("reserved", np.int32)]
)
assert CAVITY_JOB_DTYPE.itemsize == 120 and CAVITY_OUT_DTYPE.itemsize == 136
#: ``PW_CAVITY_MAX_G``, ``PW_CAV_SEED_CLOSED``
CAVITY_MAX_G = 64
CAV_SEED_CLOSED = 1

#: numpy mirror of ``pw_sasa_job``
SASA_JOB_DTYPE = np.dtype(
    [("atom_first", np.int64), ("n", np.int64), ("radius_first", np.int64), ("count_first", np.int64),
     ("word_first", np.int64), ("out", np.int64), ("origin", np.float64, (3,)), ("spacing", np.float64),
     ("probe", np.float64), ("nx", np.int32), ("ny", np.int32), ("nz", np.int32), ("reserved", np.int32)]
)
#: numpy mirror of ``pw_sasa_out``
SASA_OUT_DTYPE = np.dtype([("exposed", np.int64), ("inside", np.int64), ("flags", np.int32), ("reserved", np.int32)])
assert SASA_JOB_DTYPE.itemsize == 104 and SASA_OUT_DTYPE.itemsize == 24
#: ``PW_SASA_MAX_POINTS``, ``PW_SASA_GRID``
SASA_MAX_POINTS = 4096
SASA_GRID = 1

#: numpy mirror of ``pw_pores_job``
PORES_JOB_DTYPE = np.dtype(
    [("atom_first", np.int64), ("n", np.int64), ("radius_first", np.int64), ("plane_first", np.int64), ("m", np.int64),
     ("probe_first", np.int64), ("n_levels", np.int64), ("level_first", np.int64), ("mask_first", np.int64),
     ("out", np.int64), ("origin", np.float64, (3,)), ("spacing", np.float64), ("nx", np.int32), ("ny", np.int32),
     ("nz", np.int32), ("seed", np.int32, (3,))]
)
#: numpy mirrors of ``pw_pores_level`` and ``pw_pores_out``
PORES_LEVEL_DTYPE = np.dtype([("n_reach", np.int64), ("n_face", np.int64), ("n_swept", np.int64), ("n_largest", np.int64),
                              ("k2", np.int32), ("flags", np.int32)])
PORES_OUT_DTYPE = np.dtype([("n_domain", np.int64), ("n_none", np.int64), ("n_levels", np.int64)])
assert PORES_JOB_DTYPE.itemsize == 136 and PORES_LEVEL_DTYPE.itemsize == 40 and PORES_OUT_DTYPE.itemsize == 24
#: ``PW_PORES_MAX_LEVELS``, ``PW_PORES_MAX_K2``
PORES_MAX_LEVELS = 64
PORES_MAX_K2 = 3 * 63 * 63

#: numpy mirror of ``pw_affinity_job``
AFFINITY_JOB_DTYPE = np.dtype(
    [("atom_first", np.int64), ("n", np.int64), ("coef_first", np.int64), ("word_first", np.int64),
     ("beta_first", np.int64), ("n_betas", np.int64), ("edge_first", np.int64), ("n_edges", np.int64),
     ("level_first", np.int64), ("hist_first", np.int64), ("energy_first", np.int64), ("out", np.int64),
     ("origin", np.float64, (3,)), ("spacing", np.float64), ("core2", np.float64), ("cutoff2", np.float64),
     ("nx", np.int32), ("ny", np.int32), ("nz", np.int32), ("reserved", np.int32)]
)
#: numpy mirrors of ``pw_affinity_level`` and ``pw_affinity_out``
AFFINITY_LEVEL_DTYPE = np.dtype([("z", np.float64), ("e", np.float64)])
AFFINITY_OUT_DTYPE = np.dtype([("n_voxels", np.int64), ("n_blocked", np.int64), ("u_min", np.float64),
                               ("min_voxel", np.int32, (3,)), ("flags", np.int32)])
assert AFFINITY_JOB_DTYPE.itemsize == 160 and AFFINITY_LEVEL_DTYPE.itemsize == 16 and AFFINITY_OUT_DTYPE.itemsize == 40
#: ``PW_AFF_MAX_LEVELS``, ``PW_AFF_MAX_EDGES``, ``PW_AFF_CLAMPED``
AFF_MAX_LEVELS = 8
AFF_MAX_EDGES = 16
AFF_CLAMPED = 1

#: numpy mirrors of ``pw_rigid_job`` and ``pw_rigid_out``; the levels are ``AFFINITY_LEVEL_DTYPE`` rows
RIGID_JOB_DTYPE = np.dtype(
    [("atom_first", np.int64), ("n", np.int64), ("coef_first", np.int64), ("word_first", np.int64),
     ("beta_first", np.int64), ("n_betas", np.int64), ("site_first", np.int64), ("n_sites", np.int64),
     ("dir_first", np.int64), ("n_dirs", np.int64), ("level_first", np.int64), ("map_first", np.int64), ("out", np.int64),
     ("origin", np.float64, (3,)), ("spacing", np.float64), ("core2", np.float64), ("cutoff2", np.float64),
     ("nx", np.int32), ("ny", np.int32), ("nz", np.int32), ("charged", np.int32), ("map_level", np.int32),
     ("reserved", np.int32)]
)
RIGID_OUT_DTYPE = np.dtype([("n_voxels", np.int64), ("n_blocked_poses", np.int64), ("n_dead", np.int64),
                            ("u_min", np.float64), ("min_voxel", np.int32, (3,)), ("min_dir", np.int32),
                            ("flags", np.int32), ("reserved", np.int32)])
assert RIGID_JOB_DTYPE.itemsize == 176 and RIGID_OUT_DTYPE.itemsize == 56
#: ``PW_RIGID_MAX_SITES``, ``PW_RIGID_MAX_DIRS``
RIGID_MAX_SITES = 8
RIGID_MAX_DIRS = 1024

#: numpy mirror of ``pw_rigid_body_job``; the result rows are ``RIGID_OUT_DTYPE`` and ``AFFINITY_LEVEL_DTYPE``
RIGID_BODY_JOB_DTYPE = np.dtype(
    [("atom_first", np.int64), ("n", np.int64), ("coef_first", np.int64), ("word_first", np.int64),
     ("beta_first", np.int64), ("n_betas", np.int64), ("pose_first", np.int64), ("n_sites", np.int64), ("n_dirs", np.int64),
     ("level_first", np.int64), ("map_first", np.int64), ("out", np.int64),
     ("origin", np.float64, (3,)), ("spacing", np.float64), ("core2", np.float64), ("cutoff2", np.float64),
     ("nx", np.int32), ("ny", np.int32), ("nz", np.int32), ("charged", np.int32), ("map_level", np.int32),
     ("reserved", np.int32)]
)
assert RIGID_BODY_JOB_DTYPE.itemsize == 168

#: numpy mirror of ``pw_rigid_cell_job``; the result rows are ``RIGID_OUT_DTYPE`` and ``AFFINITY_LEVEL_DTYPE``
RIGID_CELL_JOB_DTYPE = np.dtype(
    [("atom_first", np.int64), ("n", np.int64), ("coef_first", np.int64), ("beta_first", np.int64), ("n_betas", np.int64),
     ("site_first", np.int64), ("n_sites", np.int64), ("dir_first", np.int64), ("n_dirs", np.int64), ("level_first", np.int64),
     ("map_first", np.int64), ("out", np.int64), ("origin", np.float64, (3,)), ("step", np.float64, (6,)),
     ("core2", np.float64), ("cutoff2", np.float64), ("nx", np.int32), ("ny", np.int32), ("nz", np.int32), ("reserved", np.int32)]
)
assert RIGID_CELL_JOB_DTYPE.itemsize == 200

#: numpy mirror of ``pw_rigid_cell_ewald_job``: ``cell`` is a ``RIGID_CELL_JOB_DTYPE`` record
RIGID_CELL_EWALD_JOB_DTYPE = np.dtype(
    [("cell", RIGID_CELL_JOB_DTYPE), ("charge_first", np.int64), ("cell_first", np.int64), ("n_cell", np.int64),
     ("k_first", np.int64), ("n_k", np.int64), ("alpha", np.float64), ("charged", np.int32), ("reserved", np.int32)]
)
assert RIGID_CELL_EWALD_JOB_DTYPE.itemsize == 256
#: ``PW_EWALD_MAX_K``, ``PW_EWALD_MAX_INDEX``
EWALD_MAX_K = 4096
EWALD_MAX_INDEX = 64

#: numpy mirrors of ``pw_charges_job`` and ``pw_charges_out``
CHARGES_JOB_DTYPE = np.dtype(
    [("xyz_first", np.int64), ("param_first", np.int64), ("n", np.int64), ("total_charge", np.float64),
     ("coulomb", np.float64), ("tol", np.float64), ("max_iter", np.int64), ("charge_first", np.int64), ("out", np.int64)]
)
CHARGES_OUT_DTYPE = np.dtype(
    [("mu", np.float64), ("sum_s", np.float64), ("sum_t", np.float64), ("energy", np.float64), ("dipole", np.float64, (3,)),
     ("q_min", np.float64), ("q_max", np.float64), ("iterations", np.int32, (2,)), ("flags", np.int32), ("reserved", np.int32)]
)
assert CHARGES_JOB_DTYPE.itemsize == 72 and CHARGES_OUT_DTYPE.itemsize == 88
#: ``PW_CHG_NOT_CONVERGED``, ``PW_CHG_BREAKDOWN``, ``PW_CHG_NO_SUM``
CHG_NOT_CONVERGED = 1
CHG_BREAKDOWN = 2
CHG_NO_SUM = 4

#: numpy mirrors of ``pw_charges_cell_job`` and ``pw_charges_cell_out``
CHARGES_CELL_JOB_DTYPE = np.dtype(
    [("xyz_first", np.int64), ("param_first", np.int64), ("n", np.int64), ("k_first", np.int64), ("n_k", np.int64),
     ("edges", np.float64, (6,)), ("coulomb", np.float64), ("alpha", np.float64), ("cutoff2", np.float64),
     ("shield_on2", np.float64), ("shield_off2", np.float64), ("tol", np.float64), ("max_iter", np.int64),
     ("charge_first", np.int64), ("out", np.int64)]
)
CHARGES_CELL_OUT_DTYPE = np.dtype(
    [("mu", np.float64), ("energy", np.float64), ("q_min", np.float64), ("q_max", np.float64), ("iterations", np.int32),
     ("flags", np.int32)]
)
assert CHARGES_CELL_JOB_DTYPE.itemsize == 160 and CHARGES_CELL_OUT_DTYPE.itemsize == 40
#: the solver's vectors of a ``pw_charges_cell`` job stay in LDS up to so many atoms (pw_charges_cell.hpp: CHC_LDS_ATOMS)
CHARGES_CELL_LDS_ATOMS = 1536

#: numpy mirrors of ``pw_channels_job``, ``pw_channels_comp`` and ``pw_channels_out``
CHANNELS_JOB_DTYPE = np.dtype(
    [("atom_first", np.int64), ("n", np.int64), ("radius_first", np.int64), ("comp_first", np.int64),
     ("mask_first", np.int64), ("label_first", np.int64), ("out", np.int64), ("origin", np.float64, (3,)),
     ("step", np.float64, (6,)), ("probe", np.float64), ("nx", np.int32), ("ny", np.int32), ("nz", np.int32),
     ("c_max", np.int32)]
)
CHANNELS_COMP_DTYPE = np.dtype(
    [("first", np.int64), ("n_voxels", np.int64), ("n_cross", np.int64, (3,)), ("wraps", np.int32), ("rank", np.int32)]
)
CHANNELS_OUT_DTYPE = np.dtype(
    [("n_open", np.int64), ("n_components", np.int64), ("n_recorded", np.int64), ("n_voxels_by_rank", np.int64, (4,)),
     ("n_components_by_rank", np.int64, (4,)), ("flags", np.int32), ("reserved", np.int32)]
)
assert CHANNELS_JOB_DTYPE.itemsize == 152 and CHANNELS_COMP_DTYPE.itemsize == 48 and CHANNELS_OUT_DTYPE.itemsize == 96
#: ``PW_CHAN_MAX_COMPONENTS``, ``PW_CHAN_TRUNCATED``; the labels of a component beyond the cap and of a closed voxel
CHAN_MAX_COMPONENTS = 254
CHAN_TRUNCATED = 1
CHAN_LABEL_BEYOND = 254
CHAN_LABEL_CLOSED = 255

#: numpy mirrors of ``pw_percolation_job``, ``pw_percolation_level`` and ``pw_percolation_out``
PERCOLATION_JOB_DTYPE = np.dtype(
    [("atom_first", np.int64), ("n", np.int64), ("coef_first", np.int64), ("field_first", np.int64), ("map_first", np.int64),
     ("level_first", np.int64), ("out", np.int64), ("origin", np.float64, (3,)), ("step", np.float64, (6,)),
     ("core2", np.float64), ("cutoff2", np.float64), ("nx", np.int32), ("ny", np.int32), ("nz", np.int32), ("reserved", np.int32)]
)
PERCOLATION_LEVEL_DTYPE = np.dtype(
    [("level", np.float64), ("well", np.float64), ("first", np.int64), ("n_voxels", np.int64), ("n_allowed", np.int64),
     ("saddle", np.int32, (3,)), ("well_voxel", np.int32, (3,)), ("wraps", np.int32), ("rank", np.int32), ("flags", np.int32),
     ("reserved", np.int32)]
)
PERCOLATION_OUT_DTYPE = np.dtype(
    [("n_blocked", np.int64), ("u_min", np.float64), ("u_min_voxel", np.int32, (3,)), ("flags", np.int32)]
)
assert PERCOLATION_JOB_DTYPE.itemsize == 160 and PERCOLATION_LEVEL_DTYPE.itemsize == 80 and PERCOLATION_OUT_DTYPE.itemsize == 32
#: ``PW_PERC_CRITERIA``, ``PW_PERC_NEVER``
PERC_CRITERIA = 6
PERC_NEVER = 1

#: numpy mirrors of ``pw_basins_job``, ``pw_basins_basin``, ``pw_basins_edge``, ``pw_basins_label`` and ``pw_basins_out``
BASINS_JOB_DTYPE = np.dtype(
    [("atom_first", np.int64), ("n", np.int64), ("coef_first", np.int64), ("field_first", np.int64), ("map_first", np.int64),
     ("basin_first", np.int64), ("edge_first", np.int64), ("label_first", np.int64), ("out", np.int64), ("b_cap", np.int64),
     ("e_cap", np.int64), ("origin", np.float64, (3,)), ("step", np.float64, (6,)), ("core2", np.float64),
     ("cutoff2", np.float64), ("cap", np.float64), ("betas", np.float64, (8,)), ("nx", np.int32), ("ny", np.int32),
     ("nz", np.int32), ("n_betas", np.int32)]
)
BASINS_BASIN_DTYPE = np.dtype(
    [("root", np.int64), ("n_voxels", np.int64), ("u_min", np.float64), ("z", np.float64, (8,)), ("e", np.float64, (8,))]
)
BASINS_EDGE_DTYPE = np.dtype(
    [("a", np.int32), ("b", np.int32), ("d", np.int32, (3,)), ("saddle_k", np.int32), ("n_faces", np.int64),
     ("saddle_voxel", np.int64), ("saddle", np.float64), ("s", np.float64, (8, 3))]
)
BASINS_LABEL_DTYPE = np.dtype([("basin", np.int32), ("o", np.int32, (3,))])
BASINS_OUT_DTYPE = np.dtype(
    [("n_basins", np.int64), ("n_edges", np.int64), ("n_basins_written", np.int64), ("n_edges_written", np.int64),
     ("n_blocked", np.int64), ("n_allowed", np.int64), ("u_min", np.float64), ("u_min_voxel", np.int32, (3,)), ("flags", np.int32)]
)
assert (BASINS_JOB_DTYPE.itemsize == 264 and BASINS_BASIN_DTYPE.itemsize == 152 and BASINS_EDGE_DTYPE.itemsize == 240
        and BASINS_LABEL_DTYPE.itemsize == 16 and BASINS_OUT_DTYPE.itemsize == 72)
#: ``PW_BAS_MAX_BETAS``, ``PW_BAS_MAX_OFFSET``, ``PW_BAS_OVERFLOW``, ``PW_BAS_CLAMPED``, ``PW_BAS_RANGE``
BAS_MAX_BETAS = 8
BAS_MAX_OFFSET = 255
BAS_OVERFLOW = 1
BAS_CLAMPED = 2
BAS_RANGE = 4

#: numpy mirror of ``pw_passage_job``
PASSAGE_JOB_DTYPE = np.dtype(
    [("atom_first", np.int64), ("n", np.int64), ("coef_first", np.int64), ("plane_first", np.int64), ("m", np.int64),
     ("field_first", np.int64), ("out_first", np.int64), ("origin", np.float64, (3,)), ("spacing", np.float64),
     ("core2", np.float64), ("cutoff2", np.float64), ("nx", np.int32), ("ny", np.int32), ("nz", np.int32),
     ("seed", np.int32, (3,))]
)
#: numpy mirror of ``pw_passage_out``
PASSAGE_OUT_DTYPE = np.dtype(
    [("barrier", np.float64), ("well", np.float64), ("u_seed", np.float64), ("n_fill", np.int64), ("n_basin", np.int64),
     ("saddle", np.int32, (3,)), ("well_voxel", np.int32, (3,)), ("flags", np.int32), ("reserved", np.int32)]
)
assert PASSAGE_JOB_DTYPE.itemsize == 128 and PASSAGE_OUT_DTYPE.itemsize == 72
#: ``PW_PAS_SEED_CLOSED``, ``PW_PAS_NO_EXIT``
PAS_SEED_CLOSED = 1
PAS_NO_EXIT = 2

#: numpy mirror of ``pw_hop_job``
HOP_JOB_DTYPE = np.dtype(
    [("atom_first", np.int64), ("n", np.int64), ("coef_first", np.int64), ("plane_first", np.int64), ("m", np.int64),
     ("field_first", np.int64), ("beta_first", np.int64), ("n_betas", np.int64), ("slab_first", np.int64),
     ("sum_first", np.int64), ("word_first", np.int64), ("out", np.int64), ("origin", np.float64, (3,)),
     ("spacing", np.float64), ("core2", np.float64), ("cutoff2", np.float64), ("cap", np.float64), ("nx", np.int32),
     ("ny", np.int32), ("nz", np.int32), ("seed", np.int32, (2,)), ("reserved", np.int32)]
)
#: numpy mirrors of ``pw_hop_slab`` and ``pw_hop_out``; the sums are ``AFFINITY_LEVEL_DTYPE`` rows
HOP_SLAB_DTYPE = np.dtype([("n", np.int64), ("n_face", np.int64), ("u_min", np.float64), ("min_i", np.int32),
                           ("min_j", np.int32)])
HOP_OUT_DTYPE = np.dtype([("n", np.int64), ("flags", np.int32), ("reserved", np.int32)])
assert HOP_JOB_DTYPE.itemsize == 176 and HOP_SLAB_DTYPE.itemsize == 32 and HOP_OUT_DTYPE.itemsize == 16
#: ``PW_HOP_CLAMPED``
HOP_CLAMPED = 1

#: numpy mirror of ``pw_extra_window``: a window beyond the W_MAX a record holds
EXTRA_WINDOW_DTYPE = np.dtype(
    [("unit", np.int64), ("index", np.int32), ("reserved", np.int32), ("d", np.float64), ("c", np.float64, (3,))],
    align=True,
)

#: numpy mirror of ``pw_unit_debug`` (stage capture of find_windows, ``Context.analyse_debug``)
UNIT_DEBUG_DTYPE = np.dtype(
    [
        ("n_survivors", np.int32),
        ("n_clusters", np.int32),
        ("pass_idx", np.int32, (P_MAX,)),
        ("labels", np.int32, (P_MAX,)),
        ("gap2", np.float64, (P_MAX,)),
        ("win", np.float64, (W_MAX, 12)),
    ],
    align=True,
)
#: columns of ``UNIT_DEBUG_DTYPE["win"]``
DEBUG_WIN_COLS = ("vx", "vy", "vz", "angle_1", "angle_2", "new_z", "d0", "z_x", "xy_x", "xy_y", "diam", "n_eval")

#: numpy mirror of ``pw_shape_out``
SHAPE_OUT_DTYPE = np.dtype(
    [
        ("gyration", np.float64, (3, 3)),
        ("inertia", np.float64, (3, 3)),
        ("eigenvalues", np.float64, (3,)),
        ("asphericity", np.float64),
        ("acylidricity", np.float64),
        ("relative_shape_anisotropy", np.float64),
    ],
    align=True,
)

#: every symbol include/pywindow_amd.h declares (checked by the CPU test-suite)
EXPORTED_SYMBOLS = [
    "pw_device_count",
    "pw_version",
    "pw_last_error",
    "pw_context_create",
    "pw_context_destroy",
    "pw_context_host_threads",
    "pw_context_pinned",
    "pw_params_default",
    "pw_context_set_params",
    "pw_analysis_batch",
    "pw_context_extra_windows",
    "pw_context_point_capacity",
    "pw_context_reserve_points",
    "pw_context_pipelined",
    "pw_context_gate_timeouts",
    "pw_context_retries",
    "pw_context_count_retry",
    "pw_retries_total",
    "pw_context_queue_state",
    "pw_analysis_debug",
    "pw_point_gaps",
    "pw_pairwise_sum",
    "pw_dbscan",
    "pw_resident_upload",
    "pw_resident_stream_begin",
    "pw_resident_stream_append",
    "pw_resident_launch",
    "pw_resident_sync",
    "pw_resident_download",
    "pw_resident_free",
    "pw_resident_time",
    "pw_resident_stage_times",
    "pw_resident_device_results",
    "pw_resident_extra_windows",
    "pw_resident_results_ready",
    "pw_resident_results_release",
    "pw_resident_units",
    "pw_context_stream",
    "pw_context_device",
    "pw_discrete_molecules",
    "pw_resident_from_cells",
    "pw_shape_batch",
    "pw_circumcircle",
    "pw_kde_sums",
    "pw_kde2_sums",
    "pw_kde_wsums",
    "pw_corr_sums",
    "pw_dft_sums",
    "pw_gate_counts",
    "pw_trans_counts",
    "pw_superpose",
    "pw_cluster_gromos",
    "pw_covariance",
    "pw_project",
    "pw_cavity",
    "pw_sasa",
    "pw_pore_sizes",
    "pw_affinity",
    "pw_passage",
    "pw_hop",
    "pw_rigid_affinity",
    "pw_rigid_body_affinity",
    "pw_rigid_cell",
    "pw_rigid_cell_ewald",
    "pw_charges",
    "pw_charges_cell",
    "pw_channels",
    "pw_percolation",
    "pw_basins",
    "pw_history_open",
    "pw_history_frames",
    "pw_history_atoms",
    "pw_history_keytrj",
    "pw_history_imcon",
    "pw_history_atom_keys",
    "pw_history_read",
    "pw_history_frame_info",
    "pw_history_reader_threads",
    "pw_history_stream_read",
    "pw_history_close",
]

_lib = None


def _share_torch_hip_runtime() -> None:
    """One HIP / HSA runtime per process.  PyTorch-ROCm ships its own ``libamdhip64`` (same SONAME as
    the system one this library links to).  If torch is imported first the loader gives this library
    torch's copy; the other way round the process would end up with two runtimes, and the second
    (torch's) finds no GPU.  So when torch is installed its copy is loaded first, without importing
    torch.  ``PW_SYSTEM_HIP=1`` keeps the system runtime."""
    import importlib.util
    import os
    import sys

    if os.environ.get("PW_SYSTEM_HIP") == "1" or "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.submodule_search_locations:
        return
    cand = pathlib.Path(list(spec.submodule_search_locations)[0]) / "lib" / "libamdhip64.so"
    if cand.exists():
        try:
            ctypes.CDLL(str(cand), mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def load():
    """Load libpywindow_hip.so (built by ``__graft_entry__.build()``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise PwHipError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950).  There is no CPU fallback."
        )
    # the pipeline runs several kernels side by side: give the runtime enough hardware queues
    import os

    os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
    _share_torch_hip_runtime()
    try:
        L = ctypes.CDLL(str(LIB_PATH))
    except OSError as exc:  # pragma: no cover - depends on the machine
        raise PwHipError(f"cannot load {LIB_PATH}: {exc}") from exc
    vp = ctypes.c_void_p
    L.pw_device_count.restype = ctypes.c_int
    L.pw_version.restype = ctypes.c_char_p
    L.pw_last_error.restype = ctypes.c_char_p
    L.pw_context_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.pw_context_host_threads.argtypes = [vp, ctypes.c_int]
    L.pw_context_pinned.argtypes = [vp, ctypes.c_size_t, ctypes.POINTER(vp)]
    L.pw_context_destroy.argtypes = [vp]
    L.pw_context_destroy.restype = None
    L.pw_params_default.argtypes = [ctypes.POINTER(Params)]
    L.pw_params_default.restype = None
    L.pw_context_set_params.argtypes = [vp, ctypes.POINTER(Params)]
    L.pw_analysis_batch.argtypes = [vp, ctypes.POINTER(BatchIn), ctypes.c_uint32, vp]
    L.pw_analysis_debug.argtypes = [vp, ctypes.POINTER(BatchIn), ctypes.c_uint32, vp, vp]
    L.pw_context_extra_windows.argtypes = [vp, vp, ctypes.c_int64]
    L.pw_context_extra_windows.restype = ctypes.c_int64
    L.pw_context_point_capacity.argtypes = [vp]
    L.pw_context_reserve_points.argtypes = [vp, ctypes.c_int64]
    L.pw_context_pipelined.argtypes = [vp]
    L.pw_context_gate_timeouts.argtypes = [vp, vp]
    L.pw_context_retries.argtypes = [vp, vp]
    L.pw_context_count_retry.argtypes = [vp]
    L.pw_retries_total.argtypes = []
    L.pw_retries_total.restype = ctypes.c_uint64
    L.pw_context_queue_state.argtypes = [vp, vp, ctypes.c_int]
    L.pw_point_gaps.argtypes = [vp, ctypes.POINTER(BatchIn), vp, vp, ctypes.c_int64, vp, vp]
    L.pw_pairwise_sum.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_int, vp]
    L.pw_dbscan.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_double, ctypes.c_int, vp, vp]
    L.pw_resident_upload.argtypes = [vp, ctypes.POINTER(BatchIn), ctypes.POINTER(vp)]
    L.pw_resident_stream_begin.argtypes = [vp, ctypes.c_int64, ctypes.c_int64, vp, vp, ctypes.POINTER(vp)]
    L.pw_resident_stream_append.argtypes = [vp, vp, vp, ctypes.c_int64, ctypes.c_int64]
    L.pw_resident_launch.argtypes = [vp, vp, ctypes.c_uint32]
    L.pw_resident_sync.argtypes = [vp]
    L.pw_resident_download.argtypes = [vp, vp, vp]
    L.pw_resident_free.argtypes = [vp, vp]
    L.pw_resident_free.restype = None
    L.pw_resident_time.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
    L.pw_resident_stage_times.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_float)]
    L.pw_resident_extra_windows.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_int64)]
    L.pw_resident_device_results.argtypes = [vp]
    L.pw_resident_device_results.restype = vp
    L.pw_resident_results_ready.argtypes = [vp, vp, vp, ctypes.POINTER(vp)]
    L.pw_resident_results_release.argtypes = [vp, vp, vp]
    L.pw_resident_units.argtypes = [vp]
    L.pw_resident_units.restype = ctypes.c_int64
    L.pw_context_stream.argtypes = [vp]
    L.pw_context_stream.restype = vp
    L.pw_context_device.argtypes = [vp]
    L.pw_discrete_molecules.argtypes = [vp, ctypes.POINTER(CellIn), ctypes.POINTER(CellOut)]
    L.pw_resident_from_cells.argtypes = [vp, ctypes.POINTER(CellIn), vp, ctypes.c_int32, ctypes.c_int32,
                                         ctypes.POINTER(vp), vp, vp]
    L.pw_shape_batch.argtypes = [vp, ctypes.POINTER(BatchIn), vp]
    L.pw_circumcircle.argtypes = [vp, vp, ctypes.c_int64, vp, ctypes.c_int64, vp, vp]
    L.pw_kde_sums.argtypes = [vp, vp, ctypes.c_int64, vp, vp, vp]
    L.pw_kde2_sums.argtypes = [vp, vp, ctypes.c_int64, vp, vp, vp]
    L.pw_kde_wsums.argtypes = [vp, vp, ctypes.c_int64, vp, vp, vp, vp]
    L.pw_corr_sums.argtypes = [vp, vp, ctypes.c_int64, vp, vp]
    L.pw_dft_sums.argtypes = [vp, vp, ctypes.c_int64, vp, vp, vp]
    L.pw_gate_counts.argtypes = [vp, vp, ctypes.c_int64, vp, vp, ctypes.c_int64, vp, vp]
    L.pw_trans_counts.argtypes = [vp, vp, ctypes.c_int64, vp, vp, ctypes.c_int64, vp]
    L.pw_superpose.argtypes = [vp, vp, ctypes.c_int64, vp, vp, ctypes.c_int64, vp]
    L.pw_cluster_gromos.argtypes = [vp, vp, ctypes.c_int64, vp, ctypes.c_int64, vp, vp, vp, vp]
    i64, fp = ctypes.c_int64, ctypes.POINTER(ctypes.c_float)
    # the grid, charge and crystal entries take the context, the jobs and n (pointer, length) pairs; the measurement entry of
    # each takes the same and a tail
    open_words, counters, pair_counts = [vp, vp, i64, i64, fp], [i64, fp, vp, vp], [i64, fp, vp, ctypes.c_int, vp]
    for name, n, tail in (("covariance", 4, [i64, fp]), ("project", 5, [fp]), ("cavity", 5, open_words),
                          ("pore_sizes", 7, open_words), ("affinity", 9, [i64, fp]), ("passage", 5, [i64, fp, vp, ctypes.c_int]),
                          ("hop", 9, [i64, fp]), ("rigid_affinity", 9, [i64, fp]), ("rigid_body_affinity", 8, [i64, fp]),
                          ("rigid_cell", 8, pair_counts),
                          ("rigid_cell_ewald", 11, pair_counts), ("channels", 6, open_words), ("percolation", 6, counters),
                          ("basins", 8, counters)):
        getattr(L, "pw_" + name).argtypes = [vp, vp, i64] + [vp, i64] * n
        getattr(L, "pw_internal_" + name).argtypes = [vp, vp, i64] + [vp, i64] * n + tail
    # (no pure pairs: the two counts of pw_sasa share a length, as do xyz, params and the charges of the charges pair)
    sasa = [vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, vp, vp, i64, vp, i64]
    L.pw_sasa.argtypes, L.pw_internal_sasa.argtypes = sasa, sasa + [i64, i64, i64, fp]
    L.pw_internal_erfc.argtypes = [vp, vp, i64, vp]
    charges, charges_cell = [vp, vp, i64, vp, vp, i64, vp, vp], [vp, vp, i64, vp, vp, i64, vp, i64, vp, vp]
    L.pw_charges.argtypes, L.pw_internal_charges.argtypes = charges, charges + [i64, fp]
    L.pw_charges_cell.argtypes, L.pw_internal_charges_cell.argtypes = charges_cell, charges_cell + [i64, vp]
    L.pw_internal_sincos.argtypes = [vp, i64, vp, vp]
    L.pw_internal_sincos.restype = None
    L.pw_history_open.argtypes = [ctypes.c_char_p, ctypes.POINTER(vp)]
    L.pw_history_frames.argtypes = [vp]
    L.pw_history_frames.restype = ctypes.c_int64
    L.pw_history_atoms.argtypes = [vp]
    L.pw_history_atoms.restype = ctypes.c_int64
    L.pw_history_keytrj.argtypes = [vp]
    L.pw_history_imcon.argtypes = [vp]
    L.pw_history_atom_keys.argtypes = [vp, ctypes.c_char_p, ctypes.c_int64]
    L.pw_history_atom_keys.restype = ctypes.c_int64
    L.pw_history_read.argtypes = [vp, ctypes.c_int64, ctypes.c_int64, vp, vp]
    L.pw_history_frame_info.argtypes = [vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)]
    L.pw_history_reader_threads.argtypes = []
    L.pw_history_stream_read.argtypes = [vp, ctypes.c_int64, ctypes.c_int64, vp, vp, ctypes.c_int64, vp, ctypes.c_int64, vp]
    L.pw_history_close.argtypes = [vp]
    L.pw_history_close.restype = None
    _lib = L
    return L


def _check(rc: int, what: str):
    if rc != 0:
        msg = load().pw_last_error().decode(errors="replace")
        if rc == E_TIMEOUT:
            raise PwTimeoutError(f"{what} failed with code {rc}: {msg}")
        raise PwHipError(f"{what} failed with code {rc}: {msg}")


def timeout_repeats() -> int:
    """How often an analysis is repeated after ``PW_E_TIMEOUT`` before the error is raised (``PW_TIMEOUT_REPEATS``,
    default 2; the library's ``pw_analysis_batch`` reads the same variable)."""
    import os

    try:
        return max(0, int(os.environ.get("PW_TIMEOUT_REPEATS", "2")))
    except ValueError:
        return 2


def retries_total() -> int:
    """Analyses repeated after a launch gave up waiting for another one (``PW_E_TIMEOUT``), over every context
    of this process.  Zero on a healthy device."""
    return int(load().pw_retries_total())


def _dptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


# ---- what the wrappers of the statistical entries (Context.kde_sums ... Context.project) share ----------

def _span_inside(jobs, first: str, count: str, limit: int, what: str) -> None:
    """Every job's entries ``[first, first + count)`` lie inside the array ``what`` of ``limit`` entries."""
    if ((jobs[first] < 0) | (jobs[count] < 0) | (jobs[first] + jobs[count] > limit)).any():
        raise IndexError(f"a job reaches outside `{what}`")


def _writes_from_start(jobs, first: str, what: str, error=IndexError) -> None:
    if (jobs[first] < 0).any():
        raise error(f"a job writes before the start of the {what}")


def _stat_call(name: str, *args) -> None:
    """The entry ``name`` of the library: a refused argument (``PW_E_BAD_ARG``) is a ``ValueError`` with the
    library's message, any other failure a ``PwHipError``."""
    rc = getattr(load(), name)(*args)
    if rc == -2:
        raise ValueError(load().pw_last_error().decode(errors="replace"))
    _check(rc, name)


# ---- what the wrappers of the grid, charge and crystal entries (Context.covariance ... Context.hop) share ------------

def _rows(a, width=None, dtype=np.float64, optional=False):
    """``a`` as a contiguous array of ``dtype``, flat or in rows of ``width``.  With ``optional``, ``None`` is the array
    of no rows: the library gets a pointer that is not null, and the length 0."""
    if a is None and optional:
        return np.zeros(0 if width is None else (0, width), dtype=dtype)
    return np.ascontiguousarray(a, dtype=dtype).reshape(-1 if width is None else (-1, width))


def _furthest(ends) -> int:
    """The furthest of the jobs' ends, 0 without jobs."""
    return int(ends.max()) if len(ends) else 0


def _result(given, dtype, what, size):
    """The result array ``what``: ``given``, checked, or zeros up to ``size`` entries."""
    if given is None:
        return np.zeros(max(int(size), 0), dtype=dtype)
    if given.dtype != dtype or not given.flags.c_contiguous or given.ndim != 1:
        raise ValueError(f"{what}: a C-contiguous one-dimensional {np.dtype(dtype).name} array")
    return given


def _result_if_any(given, dtype, what, first, count):
    """:func:`_result` for a result that only the jobs with ``first >= 0`` have, ``count`` entries each from there:
    ``None`` unless it is given or a job has one."""
    has = first >= 0
    if given is None and not has.any():
        return None
    return _result(given, dtype, what, _furthest((first + count)[has]))


def _pl(a):
    """(pointer, length) of an array; the null pointer and 0 for ``None``."""
    return (None, 0) if a is None else (a.ctypes.data, len(a))


def _pls(*arrays) -> list:
    return [v for a in arrays for v in _pl(a)]


def _open_words(open_words, open_first, n_jobs: int):
    """Ready-made open words (uint64) and where each job's begin (int64, one a job): both arrays, or ``None`` twice."""
    w = None if open_words is None else _rows(open_words, dtype=np.uint64)
    f = None if open_first is None else _rows(open_first, dtype=np.int64)
    if (w is None) != (f is None) or (f is not None and len(f) != n_jobs):
        raise ValueError("open_words and open_first: both, with one entry of open_first per job")
    return w, f


def _measured(name: str, args, before, kernel_ms, after=(), n_ms: int = 1) -> None:
    """The measurement entry ``pw_internal_<name>``: ``args``, ``before``, the ``n_ms`` floats that receive the times of
    the device work, ``after``.  ``kernel_ms``, a list or ``None``, receives the time: a float, or a tuple of ``n_ms``."""
    ms = (ctypes.c_float * n_ms)()
    _stat_call("pw_internal_" + name, *args, *before, ms, *after)
    if kernel_ms is not None:
        kernel_ms.append(float(ms[0]) if n_ms == 1 else tuple(float(v) for v in ms))


class Batch:
    """Host-side description of a ragged batch of molecules (keeps arrays alive)."""

    def __init__(self, atom_offset, xyz, vdw, mass, template_atoms: int = 0):
        """``template_atoms`` = T > 0: every unit has T atoms and ``vdw`` / ``mass`` are one template
        of T entries (``pw_batch_in.template_atoms``); 0: one entry per atom of the batch."""
        self.atom_offset = np.ascontiguousarray(atom_offset, dtype=np.int64)
        self.xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        self.vdw = np.ascontiguousarray(vdw, dtype=np.float64)
        self.mass = np.ascontiguousarray(mass, dtype=np.float64)
        n_atoms = int(self.atom_offset[-1]) if len(self.atom_offset) else 0
        n_const = int(template_atoms) if template_atoms else n_atoms
        if len(self.xyz) != n_atoms or len(self.vdw) != n_const or len(self.mass) != n_const:
            raise ValueError("atom_offset does not match the per-atom arrays")
        self.n_units = len(self.atom_offset) - 1
        self.template_atoms = int(template_atoms)
        self.c = BatchIn(
            self.n_units,
            self.atom_offset.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
            _dptr(self.xyz),
            _dptr(self.vdw),
            _dptr(self.mass),
            self.template_atoms,
        )

    @classmethod
    def uniform(cls, coords, vdw, mass):
        """``coords`` (U, N, 3) of one molecule type; ``vdw``/``mass`` (N,): the constants of the
        trajectory travel once, as a template."""
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        u, n, _ = coords.shape
        off = np.arange(u + 1, dtype=np.int64) * n
        return cls(off, coords.reshape(-1, 3), vdw, mass, template_atoms=n)


class Context:
    """One GPU: stream + workspace.  ``device`` is the HIP ordinal; ``-1`` is the explicit host path
    (the same kernel source run by host threads, ``host_threads`` of them) -- never chosen implicitly."""

    def __init__(self, device: int = 0, host_threads: int = 0):
        L = load()
        h = ctypes.c_void_p()
        _check(L.pw_context_create(device, ctypes.byref(h)), "pw_context_create")
        self._h = h
        self.device = device
        if device < 0 and host_threads > 0:
            L.pw_context_host_threads(h, int(host_threads))
        # params live on the context between set and reset: one analysis with params at a time
        import threading

        #: held across the multi-call protocols that go through per-context state -- the page-locked staging
        #: buffer (pinned_array -> upload), "the records fetched last" (download -> extra_windows), the capacities
        #: a repeated launch relies on.  The C library serialises single calls on a context by itself
        #: (include/pywindow_amd.h, "Threads"); what belongs together is the caller's to keep together.
        self.lock = threading.RLock()
        self._params_lock = self.lock           # (params live on the context between set and reset: the same sequences)

    def close(self):
        if self._h:
            load().pw_context_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, params: "Params | None" = None) -> None:
        """Knobs used by every later launch on this context (``None`` = reference defaults)."""
        p = params if params is not None else Params()
        _check(load().pw_context_set_params(self._h, ctypes.byref(p)), "pw_context_set_params")

    def extra_windows(self) -> np.ndarray:
        """Windows beyond ``W_MAX`` of the records fetched last on this context (``EXTRA_WINDOW_DTYPE``,
        ordered by unit and position): the reference has no limit on the number of windows."""
        n = load().pw_context_extra_windows(self._h, None, 0)
        buf = np.zeros(n, dtype=EXTRA_WINDOW_DTYPE)
        if n:
            load().pw_context_extra_windows(self._h, buf.ctypes.data, n)
        return buf

    def pinned_array(self, shape) -> np.ndarray:
        """float64 array of ``shape`` in the context's page-locked staging buffer (``pw_context_pinned``):
        decode frames into it and the upload copies by DMA.  ONE buffer per context: the array is valid
        until the next call; an upload has finished with it when it returns.  Host contexts: a plain array."""
        n = int(np.prod(shape))
        if self.device < 0 or n == 0:
            return np.empty(shape, dtype=np.float64)
        ptr = ctypes.c_void_p()
        _check(load().pw_context_pinned(self._h, n * 8, ctypes.byref(ptr)), "pw_context_pinned")
        buf = (ctypes.c_double * n).from_address(ptr.value)
        arr = np.frombuffer(buf, dtype=np.float64, count=n).reshape(shape)
        return arr

    @property
    def pipelined(self) -> bool:
        """Whether analyses run as the overlapped pipeline (needs ``GPU_MAX_HW_QUEUES`` >= 10 exported before
        the process first initialised HIP; measured at context creation) or as single launches."""
        return bool(load().pw_context_pipelined(self._h))

    @property
    def gate_timeouts(self) -> dict:
        """Diagnostic: pacing gates of the pipeline that gave up waiting since the context was created (a gate is
        never a dependency: 20 ms lost, no result changed).  All zero on a healthy device."""
        v = ctypes.c_uint64(0)
        _check(load().pw_context_gate_timeouts(self._h, ctypes.byref(v)), "pw_context_gate_timeouts")
        return {"tail": int(v.value & 0xffff), "head": int((v.value >> 16) & 0xffff), "residency": int(v.value >> 32)}

    @property
    def retries(self) -> int:
        """Analyses repeated on this context after ``PW_E_TIMEOUT`` (by the library or by this binding)."""
        v = ctypes.c_uint64(0)
        _check(load().pw_context_retries(self._h, ctypes.byref(v)), "pw_context_retries")
        return int(v.value)

    def queue_state(self) -> list:
        """Diagnostic: the hand-off queues of the pipeline's sets as they are now."""
        buf = (ctypes.c_uint64 * 16)()
        _check(load().pw_context_queue_state(self._h, buf, 16), "pw_context_queue_state")
        return [{"set": b, "taken": int(buf[4 * b]), "published": int(buf[4 * b + 1]), "started": int(buf[4 * b + 2]),
                 "error": int(buf[4 * b + 3])} for b in range(4)]

    def reserve_points(self, n_points: int) -> None:
        """At least ``n_points`` sampling vectors per molecule in the workspaces of every later launch
        (``pw_context_reserve_points``): what ``pw_analysis_batch`` does by itself when a unit asks for more
        than the ``adjust`` knobs imply, for callers of the resident entry points."""
        _check(load().pw_context_reserve_points(self._h, int(n_points)), "pw_context_reserve_points")

    @property
    def point_capacity(self) -> int:
        """Sampling vectors per molecule the workspaces hold at present (follows the ``adjust`` knobs)."""
        return int(load().pw_context_point_capacity(self._h))

    def analyse(self, batch: Batch, stages: int = STAGE_ALL, params: "Params | None" = None, extra=None) -> np.ndarray:
        """``extra``: a list that receives the ``EXTRA_WINDOW_DTYPE`` array of this analysis (windows
        beyond ``W_MAX``; read under the same lock as the analysis)."""
        out = np.zeros(batch.n_units, dtype=UNIT_OUT_DTYPE)
        if batch.n_units == 0:
            return out
        with self._params_lock:
            if params is not None:
                self.set_params(params)
            try:
                _check(
                    load().pw_analysis_batch(self._h, ctypes.byref(batch.c), stages, out.ctypes.data),
                    "pw_analysis_batch",
                )
                if extra is not None and (out["status"] & ST_WINDOW_OVERFLOW).any():
                    extra.append(self.extra_windows())
            finally:
                if params is not None:
                    self.set_params(None)
        return out

    def analyse_debug(self, batch: Batch, stages: int = STAGE_ALL):
        """``pw_analysis_debug``: ``(records, stage captures)`` -- the intermediate results of
        find_windows per unit (``UNIT_DEBUG_DTYPE``), for the parity tests."""
        out = np.zeros(batch.n_units, dtype=UNIT_OUT_DTYPE)
        dbg = np.zeros(batch.n_units, dtype=UNIT_DEBUG_DTYPE)
        if batch.n_units:
            with self._params_lock:
                _check(load().pw_analysis_debug(self._h, ctypes.byref(batch.c), stages, out.ctypes.data,
                                                dbg.ctypes.data), "pw_analysis_debug")
        return out, dbg

    def point_gaps(self, batch: Batch, unit_of_point, points):
        """min_i(|r_i - p| - vdw_i), argmin for each point (objective of the optimisers)."""
        u = np.ascontiguousarray(unit_of_point, dtype=np.int64)
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        gap = np.zeros(len(p))
        arg = np.zeros(len(p), dtype=np.int32)
        _check(
            load().pw_point_gaps(self._h, ctypes.byref(batch.c), u.ctypes.data, p.ctypes.data, len(p),
                                 gap.ctypes.data, arg.ctypes.data),
            "pw_point_gaps",
        )
        return gap, arg

    def dbscan(self, points, eps: float, one_wave: bool = False, global_memory: bool = False):
        """``DBSCAN(eps, min_samples=5).fit(points).labels_`` by one team on the GPU -> (labels, n_clusters)."""
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        labels = np.zeros(len(p), dtype=np.int32)
        k = ctypes.c_int32(0)
        _check(load().pw_dbscan(self._h, p.ctypes.data, len(p), float(eps), int(one_wave) | (int(global_memory) << 1),
                                labels.ctypes.data, ctypes.byref(k)), "pw_dbscan")
        return labels, k.value

    def pairwise_sum(self, values, one_wave: bool = False, global_scratch: bool = False) -> float:
        """``np.add.reduce`` of a float64 array in numpy's order, computed by one team on the GPU."""
        a = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        out = ctypes.c_double(0.0)
        _check(load().pw_pairwise_sum(self._h, a.ctypes.data, len(a), int(one_wave) | (int(global_scratch) << 1),
                                      ctypes.byref(out)), "pw_pairwise_sum")
        return out.value

    def shape(self, batch: Batch) -> np.ndarray:
        """``pw_shape_batch``: gyration / inertia tensors, sorted eigenvalues and the three shape
        descriptors of every unit (``SHAPE_OUT_DTYPE`` records)."""
        out = np.zeros(batch.n_units, dtype=SHAPE_OUT_DTYPE)
        if batch.n_units:
            _check(load().pw_shape_batch(self._h, ctypes.byref(batch.c), out.ctypes.data), "pw_shape_batch")
        return out

    def kde_sums(self, jobs, samples, points) -> np.ndarray:
        """``pw_kde_sums``: the raw Gaussian kernel sums of a batch of jobs (``KDE_JOB_DTYPE`` records indexing the
        float64 arrays ``samples`` and ``points``); returns the sums, laid out like ``points``.  A bandwidth that
        is not positive, or a NaN / infinity anywhere, raises ``ValueError``."""
        jobs = np.ascontiguousarray(jobs, dtype=KDE_JOB_DTYPE).reshape(-1)
        x = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1)
        g = np.ascontiguousarray(points, dtype=np.float64).reshape(-1)
        _span_inside(jobs, "sample_first", "n_samples", len(x), "samples")
        _span_inside(jobs, "point_first", "n_points", len(g), "points")
        sums = np.zeros(len(g))
        _stat_call("pw_kde_sums", self._h, jobs.ctypes.data, len(jobs), x.ctypes.data, g.ctypes.data, sums.ctypes.data)
        return sums

    def kde2_sums(self, jobs, samples, points) -> np.ndarray:
        """``pw_kde2_sums``: the raw sums of a batch of two-dimensional Gaussian kernel jobs (``KDE2_JOB_DTYPE``
        records indexing the rows of the float64 arrays ``samples`` (N, 2) and ``points`` (M, 2) -- any list of
        points, not only a mesh); returns the M sums.  Factors that are not finite with a positive diagonal, or a
        NaN / infinity anywhere, raise ``ValueError``."""
        jobs = np.ascontiguousarray(jobs, dtype=KDE2_JOB_DTYPE).reshape(-1)
        x = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1, 2)
        g = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
        _span_inside(jobs, "sample_first", "n_samples", len(x), "samples")
        _span_inside(jobs, "point_first", "n_points", len(g), "points")
        sums = np.zeros(len(g))
        _stat_call("pw_kde2_sums", self._h, jobs.ctypes.data, len(jobs), x.ctypes.data, g.ctypes.data, sums.ctypes.data)
        return sums

    def kde_wsums(self, jobs, samples, points, weights) -> np.ndarray:
        """``pw_kde_wsums``: the raw Gaussian kernel sums of a batch of jobs under many weight vectors each
        (``KDEW_JOB_DTYPE`` records indexing the float64 arrays ``samples``, ``points`` and ``weights`` -- sample-major,
        ``w[i * n_replicas + b]`` -- and the result, replica-major ``S[b * n_points + j]``); returns the sums, as long
        as the furthest ``out_first + n_replicas * n_points`` of a job (entries no job writes are zero).  No replica,
        a bandwidth that is not positive, a negative weight, or a NaN / infinity anywhere, raises ``ValueError``."""
        jobs = np.ascontiguousarray(jobs, dtype=KDEW_JOB_DTYPE).reshape(-1)
        x = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1)
        g = np.ascontiguousarray(points, dtype=np.float64).reshape(-1)
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        _span_inside(jobs, "sample_first", "n_samples", len(x), "samples")
        _span_inside(jobs, "point_first", "n_points", len(g), "points")
        replicas = np.maximum(jobs["n_replicas"], 0)
        if ((jobs["weight_first"] < 0) | (jobs["weight_first"] + jobs["n_samples"] * replicas > len(w))).any():
            raise IndexError("a job reaches outside `weights`")
        _writes_from_start(jobs, "out_first", "sums")
        sums = np.zeros(int((jobs["out_first"] + replicas * jobs["n_points"]).max()) if len(jobs) else 0)
        _stat_call("pw_kde_wsums", self._h, jobs.ctypes.data, len(jobs), x.ctypes.data, g.ctypes.data, w.ctypes.data,
                   sums.ctypes.data)
        return sums

    def corr_sums(self, jobs, series) -> np.ndarray:
        """``pw_corr_sums``: the raw lagged sums ``S[k] = sum_t a[t] b[t + k]`` of a batch of jobs (``CORR_JOB_DTYPE``
        records indexing the float64 array ``series`` and the result); returns the sums, as long as the furthest
        ``out_first + n_lags`` of a job (entries no job writes are zero).  ``n_lags`` outside ``1 .. n``, or a NaN /
        infinity in a series, raises ``ValueError``."""
        jobs = np.ascontiguousarray(jobs, dtype=CORR_JOB_DTYPE).reshape(-1)
        x = np.ascontiguousarray(series, dtype=np.float64).reshape(-1)
        _span_inside(jobs, "a_first", "n", len(x), "series")
        _span_inside(jobs, "b_first", "n", len(x), "series")
        _writes_from_start(jobs, "out_first", "sums")
        live = jobs[jobs["n"] > 0]
        sums = np.zeros(int(max(0, (live["out_first"] + live["n_lags"]).max())) if len(live) else 0)
        _stat_call("pw_corr_sums", self._h, jobs.ctypes.data, len(jobs), x.ctypes.data, sums.ctypes.data)
        return sums

    def dft_sums(self, jobs, series) -> np.ndarray:
        """``pw_dft_sums``: the raw sums ``sum_t a[t] exp(2 pi i j t / M)`` of a batch of jobs (``DFT_JOB_DTYPE`` records
        indexing the float64 array ``series`` and the result) as one complex array ``re + 1j * im``, as long as the
        furthest ``out_first + n_freq`` of a job (entries no job writes are zero).  A period outside ``2 .. 2^31``, a
        frequency outside ``0 .. period - 1``, ``j_step < 1`` or a NaN / infinity in a series raises ``ValueError``."""
        jobs = np.ascontiguousarray(jobs, dtype=DFT_JOB_DTYPE).reshape(-1)
        x = np.ascontiguousarray(series, dtype=np.float64).reshape(-1)
        _span_inside(jobs, "a_first", "n", len(x), "series")
        _writes_from_start(jobs, "out_first", "sums")
        live = jobs[(jobs["n"] > 0) & (jobs["n_freq"] > 0)]
        size = int(max(0, (live["out_first"] + live["n_freq"]).max())) if len(live) else 0
        re, im = np.zeros(size), np.zeros(size)      # (the entry wants two arrays; the result carries their bits)
        _stat_call("pw_dft_sums", self._h, jobs.ctypes.data, len(jobs), x.ctypes.data, re.ctypes.data, im.ctypes.data)
        out = np.empty(size, dtype=np.complex128)
        out.real, out.imag = re, im
        return out

    def gate_counts(self, jobs, series, thresholds, n_bins: int = 0):
        """``pw_gate_counts``: the gating statistics of a batch of jobs (``GATE_JOB_DTYPE`` records indexing the float64
        arrays ``series`` -- a NaN is a gap -- and ``thresholds``, and the rows of the result): ``(counts (R, 12) int64,
        hist (R, 2, n_bins) int64)``, the columns of ``counts`` as ``GATE_FIELDS`` names them, ``hist[r, 0]`` / ``[r, 1]``
        the lengths of the complete open / closed runs (the last bin takes every length ``>= n_bins``), ``R`` the
        furthest ``out_first + n_thr`` of a job (rows no job writes are zero).  An infinity in a series, a NaN or an
        infinity among the thresholds, or a negative ``n_bins`` raises ``ValueError``."""
        jobs = np.ascontiguousarray(jobs, dtype=GATE_JOB_DTYPE).reshape(-1)
        x = np.ascontiguousarray(series, dtype=np.float64).reshape(-1)
        d = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
        n_bins = int(n_bins)
        _span_inside(jobs, "a_first", "n", len(x), "series")
        _span_inside(jobs, "d_first", "n_thr", len(d), "thresholds")
        _writes_from_start(jobs, "out_first", "counts")
        live = jobs[(jobs["n"] > 0) & (jobs["n_thr"] > 0)]
        rows = int((live["out_first"] + live["n_thr"]).max()) if len(live) else 0
        counts = np.zeros((rows, len(GATE_FIELDS)), dtype=np.int64)
        hist = np.zeros((rows, 2, max(n_bins, 0)), dtype=np.int64)
        _stat_call("pw_gate_counts", self._h, jobs.ctypes.data, len(jobs), x.ctypes.data, d.ctypes.data, n_bins,
                   counts.ctypes.data, hist.ctypes.data)
        return counts, hist

    def trans_counts(self, jobs, series, edges, n_states: int) -> np.ndarray:
        """``pw_trans_counts``: the lagged state-transition counts of a batch of jobs (``TRANS_JOB_DTYPE`` records indexing
        the float64 arrays ``series`` -- a NaN is a gap -- and ``edges``, and the rows of the result): ``counts (R,
        n_states, n_states) int64`` with ``counts[out_first + q, i, j]`` the number of pairs ``s[t] = i, s[t + k_q] = j``,
        ``R`` the furthest ``out_first + n_lags`` of a job (rows no job writes are zero).  An infinity in a series, edges
        that are not finite and strictly increasing, ``n_edges >= n_states``, ``lag_step < 1`` or ``n_states`` outside
        ``1 .. 16`` raises ``ValueError``."""
        jobs = np.ascontiguousarray(jobs, dtype=TRANS_JOB_DTYPE).reshape(-1)
        x = np.ascontiguousarray(series, dtype=np.float64).reshape(-1)
        e = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        n_states = int(n_states)
        _span_inside(jobs, "a_first", "n", len(x), "series")
        _span_inside(jobs, "e_first", "n_edges", len(e), "edges")
        _writes_from_start(jobs, "out_first", "counts")
        live = jobs[(jobs["n"] > 0) & (jobs["n_lags"] > 0)]
        rows = int((live["out_first"] + live["n_lags"]).max()) if len(live) else 0
        side = min(max(n_states, 0), TRANS_MAX_STATES)
        counts = np.zeros((rows, side, side), dtype=np.int64)
        _stat_call("pw_trans_counts", self._h, jobs.ctypes.data, len(jobs), x.ctypes.data, e.ctypes.data, n_states,
                   counts.ctypes.data)
        return counts

    def superpose(self, jobs, xyz, weights=None, out=None) -> np.ndarray:
        """``pw_superpose``: the least-squares superposition of a batch of jobs (``SUPERPOSE_JOB_DTYPE`` records indexing
        the rows of ``xyz`` (M, 3) float64 and the entries of ``weights`` (M) float64, ``weight_first = -1`` for weights
        of one): a ``SUPERPOSE_OUT_DTYPE`` array with row ``out`` of every job filled in -- ``out`` given, or zeros up to
        the furthest row of a job; rows no job writes stay as they are.  ``n < 1``, a coordinate that is not finite, a
        weight that is negative or not finite, weights that sum to 0 or a range outside the arrays raise
        ``ValueError``."""
        jobs = np.ascontiguousarray(jobs, dtype=SUPERPOSE_JOB_DTYPE).reshape(-1)
        x = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if w is not None and len(w) != len(x):
            raise ValueError("one weight per row of xyz")
        _writes_from_start(jobs, "out", "result", error=ValueError)
        rows = int(jobs["out"].max()) + 1 if len(jobs) else 0
        if out is None:
            out = np.zeros(rows, dtype=SUPERPOSE_OUT_DTYPE)
        elif out.dtype != SUPERPOSE_OUT_DTYPE or not out.flags.c_contiguous or out.ndim != 1 or len(out) < rows:
            raise ValueError("out: a contiguous SUPERPOSE_OUT_DTYPE array with a row for every job")
        _stat_call("pw_superpose", self._h, jobs.ctypes.data, len(jobs), x.ctypes.data, None if w is None else w.ctypes.data,
                   len(x), out.ctypes.data)
        return out

    def cluster_gromos(self, jobs, dist, labels=None, centres=None, sizes=None):
        """``pw_cluster_gromos``: the gromos clustering of a batch of jobs (``CLUSTER_JOB_DTYPE`` records indexing the
        float64 array ``dist`` -- ``n * n`` row-major entries from ``d_first``, of which only the strict upper triangle is
        read -- and the entries of the results): ``(labels, centres, sizes, n_clusters)``, the first three int32 with the
        ``n`` entries from ``out_first`` of every job filled in -- given, or ``-1``, ``-1`` and ``0`` up to the furthest
        entry of a job; entries no job owns stay as they are -- and ``n_clusters`` int64, one per job.  A NaN in the strict
        upper triangle, a NaN cutoff or ``n`` above ``CLUSTER_MAX_N`` raises ``ValueError``; a matrix that reaches outside
        ``dist`` or results too short for a job ``IndexError``."""
        jobs = np.ascontiguousarray(jobs, dtype=CLUSTER_JOB_DTYPE).reshape(-1)
        d = np.ascontiguousarray(dist, dtype=np.float64).reshape(-1)
        if ((jobs["d_first"] < 0) | (jobs["n"] < 0) | (jobs["d_first"] + jobs["n"] * jobs["n"] > len(d))).any():
            raise IndexError("a job reaches outside `dist`")
        _writes_from_start(jobs, "out_first", "results")
        size = int((jobs["out_first"] + jobs["n"]).max()) if len(jobs) else 0
        out = []
        for given, fill, what in ((labels, -1, "labels"), (centres, -1, "centres"), (sizes, 0, "sizes")):
            if given is None:
                given = np.full(size, fill, dtype=np.int32)
            elif given.dtype != np.int32 or not given.flags.c_contiguous or given.ndim != 1 or len(given) < size:
                raise IndexError(f"{what}: a contiguous int32 array with an entry for every frame of every job")
            out.append(given)
        n_clusters = np.zeros(len(jobs), dtype=np.int64)
        _stat_call("pw_cluster_gromos", self._h, jobs.ctypes.data, len(jobs), d.ctypes.data, len(d), out[0].ctypes.data,
                   out[1].ctypes.data, out[2].ctypes.data, n_clusters.ctypes.data)
        return out[0], out[1], out[2], n_clusters

    def covariance(self, jobs, data, transforms=None, mean=None, scatter=None, workspace_bytes=None, kernel_ms=None):
        """``pw_covariance``: the column mean and the scatter matrix of a batch of jobs (``COV_JOB_DTYPE`` records indexing
        the float64 array ``data``, the ``SUPERPOSE_OUT_DTYPE`` rows ``transforms`` and the entries of the results):
        ``(mean, scatter)``, float64, with the ``D`` entries from ``mean_first`` and the ``D * D`` from ``s_first`` of every
        job filled in -- given, or zeros up to the furthest entry of a job; entries no job owns stay as they are.
        ``s_first = -1``: the mean only.  ``workspace_bytes`` (the budget of the partial sums; the result may not depend
        on it) and ``kernel_ms`` (a list that receives the kernels' time by HIP events) go through the hook
        ``pw_internal_covariance``.  Whatever the library refuses (include/pywindow_amd.h) raises ``ValueError``."""
        jobs = _rows(jobs, dtype=COV_JOB_DTYPE)
        x = _rows(data)
        tr = None if transforms is None else _rows(transforms, dtype=SUPERPOSE_OUT_DTYPE)
        wanted = jobs["s_first"] >= 0
        mean = _result(mean, np.float64, "mean", _furthest(jobs["mean_first"] + jobs["D"]))
        scatter = _result(scatter, np.float64, "scatter", _furthest((jobs["s_first"] + jobs["D"] * jobs["D"])[wanted]))
        args = [self._h] + _pls(jobs, x, tr, mean, scatter)
        if workspace_bytes is None and kernel_ms is None:
            _stat_call("pw_covariance", *args)
        else:
            _measured("covariance", args, [int(workspace_bytes or 0)], kernel_ms)
        return mean, scatter

    def project(self, jobs, data, mean, vectors, transforms=None, proj=None, kernel_ms=None):
        """``pw_project``: the projections of the centred rows of a batch of jobs (``PROJECT_JOB_DTYPE`` records indexing
        ``data``, ``transforms``, ``mean`` and ``vectors`` as :meth:`covariance` does) on their ``k`` vectors: ``proj``,
        float64, with the ``T * k`` entries from ``p_first`` of every job filled in -- given, or zeros up to the furthest
        entry of a job.  Whatever the library refuses raises ``ValueError``."""
        jobs = _rows(jobs, dtype=PROJECT_JOB_DTYPE)
        x, m, v = _rows(data), _rows(mean), _rows(vectors)
        tr = None if transforms is None else _rows(transforms, dtype=SUPERPOSE_OUT_DTYPE)
        ok = (jobs["T"] > 0) & (jobs["k"] > 0) & (jobs["p_first"] >= 0)
        proj = _result(proj, np.float64, "proj", _furthest((jobs["p_first"] + jobs["T"] * jobs["k"])[ok]))
        args = [self._h] + _pls(jobs, x, tr, m, v, proj)
        if kernel_ms is None:
            _stat_call("pw_project", *args)
        else:
            _measured("project", args, [], kernel_ms)
        return proj

    def cavity(self, jobs, xyz, radii, planes=None, out=None, mask=None, open_words=None, open_first=None,
               workspace_bytes=None, kernel_ms=None):
        """``pw_cavity``: the voxel flood fill of a batch of jobs (``CAVITY_JOB_DTYPE`` records indexing the rows of
        ``xyz`` (rows of three), the entries of ``radii``, the rows of ``planes`` (rows of four), the rows of the result
        and the words of ``mask``): ``(out, mask)``, ``out`` a ``CAVITY_OUT_DTYPE`` array -- ``out`` given: filled in
        place, rows no job owns stay as they are -- and ``mask`` the uint64 words of the jobs with ``mask_first >= 0``
        (``None`` when no job has one).  Whatever the entry refuses -- a value that is not finite, ``spacing <= 0``, a
        negative radius or probe, a dimension outside ``1 .. CAVITY_MAX_G``, a seed outside the grid, a range outside
        an array, jobs that share outputs --: ``ValueError`` with the library's message.  ``open_words`` /
        ``open_first`` / ``workspace_bytes`` / ``kernel_ms`` (a list that receives the time of the
        device work by HIP events) go through the library's measurement entry."""
        jobs = _rows(jobs, dtype=CAVITY_JOB_DTYPE)
        x, r, p = _rows(xyz, 3), _rows(radii), _rows(planes, 4, optional=True)
        out = _result(out, CAVITY_OUT_DTYPE, "out", _furthest(jobs["out"] + 1))
        mask = _result_if_any(mask, np.uint64, "mask", jobs["mask_first"], jobs["ny"].astype(np.int64) * jobs["nz"])
        args = [self._h] + _pls(jobs, x, r, p, out, mask)
        if open_words is None and workspace_bytes is None and kernel_ms is None:
            _stat_call("pw_cavity", *args)
        else:
            w, f = _open_words(open_words, open_first, len(jobs))
            _measured("cavity", args, [_pl(w)[0], _pl(f)[0], _pl(w)[1], int(workspace_bytes or 0)], kernel_ms)
        return out, mask

    def sasa(self, jobs, xyz, radii, directions, words=None, out=None, exposed=None, inside=None, list_capacity=None,
             lds_words=None, block_atoms=None, kernel_ms=None):
        """``pw_sasa``: the exposed and the inside test points of every atom of a batch of jobs (``SASA_JOB_DTYPE``
        records indexing the rows of ``xyz`` (rows of three), the entries of ``radii``, of ``words`` (uint64, a grid in
        the layout of ``pw_cavity``'s mask; ``word_first = -1``: no grid), of ``exposed`` / ``inside`` and the rows of
        the result) for the ``(P, 3)`` unit ``directions`` the jobs share: ``(out, exposed, inside)``, ``out`` a
        ``SASA_OUT_DTYPE`` array and the counts int32 -- given: filled in place, entries no job owns stay as they are.
        Whatever the entry refuses -- a value that is not finite, a negative radius or probe, ``spacing <= 0``, a
        dimension outside ``1 .. CAVITY_MAX_G``, ``P`` outside ``1 .. SASA_MAX_POINTS``, a direction that is not a
        unit vector to ``1e-9``, a range outside an array, jobs that share outputs --: ``ValueError`` with the
        library's message.  ``list_capacity`` / ``lds_words`` / ``block_atoms`` / ``kernel_ms`` (a list that receives
        the time of the kernel by HIP events) go through the library's measurement entry."""
        jobs = _rows(jobs, dtype=SASA_JOB_DTYPE)
        x, r, u = _rows(xyz, 3), _rows(radii), _rows(directions, 3)
        w = _rows(words, dtype=np.uint64, optional=True)
        out = _result(out, SASA_OUT_DTYPE, "out", _furthest(jobs["out"] + 1))
        size = _furthest(jobs["count_first"] + jobs["n"])
        exposed, inside = _result(exposed, np.int32, "exposed", size), _result(inside, np.int32, "inside", size)
        if len(exposed) != len(inside):
            raise ValueError("exposed and inside: the same length")
        args = [self._h] + _pls(jobs, x, r, u, w) + [exposed.ctypes.data, inside.ctypes.data, len(exposed)] + _pls(out)
        if list_capacity is None and lds_words is None and block_atoms is None and kernel_ms is None:
            _stat_call("pw_sasa", *args)
        else:
            _measured("sasa", args, [int(list_capacity or 0), int(lds_words or 0), int(block_atoms or 0)], kernel_ms)
        return out, exposed, inside

    def pore_sizes(self, jobs, xyz, radii, probes, planes=None, levels=None, out=None, mask=None, open_words=None,
                   open_first=None, workspace_bytes=None, kernel_ms=None):
        """``pw_pore_sizes``: the probe-swept cavity of a batch of jobs for their ladders of probes
        (``PORES_JOB_DTYPE`` records indexing the rows of ``xyz`` (rows of three), the entries of ``radii`` and of
        ``probes``, the rows of ``planes`` (rows of four), the rows of the two results and the words of ``mask``):
        ``(levels, out, mask)``, ``levels`` a ``PORES_LEVEL_DTYPE`` array with ``n_levels`` rows a job from its
        ``level_first``, ``out`` a ``PORES_OUT_DTYPE`` array -- given: filled in place, rows no job owns stay as they
        are -- and ``mask`` the uint64 words of the jobs with ``mask_first >= 0``, ``n_levels * ny * nz`` a job, level
        after level (``None`` when no job has one).  Whatever the entry refuses -- what ``pw_cavity`` refuses,
        ``n_levels`` outside ``1 .. PORES_MAX_LEVELS``, a probe that is not finite or negative, probes that do not
        ascend strictly, a range outside an array, jobs that share outputs --: ``ValueError`` with the library's
        message.  ``open_words`` / ``open_first`` (ready-made open words, ``n_levels * ny * nz`` a job) /
        ``workspace_bytes`` / ``kernel_ms`` (a list that receives the time of the device work by HIP events) go through
        the library's measurement entry."""
        jobs = _rows(jobs, dtype=PORES_JOB_DTYPE)
        x, r, q, p = _rows(xyz, 3), _rows(radii), _rows(probes), _rows(planes, 4, optional=True)
        out = _result(out, PORES_OUT_DTYPE, "out", _furthest(jobs["out"] + 1))
        levels = _result(levels, PORES_LEVEL_DTYPE, "levels", _furthest(jobs["level_first"] + jobs["n_levels"]))
        mask = _result_if_any(mask, np.uint64, "mask", jobs["mask_first"],
                              jobs["n_levels"] * jobs["ny"].astype(np.int64) * jobs["nz"])
        args = [self._h] + _pls(jobs, x, r, p, q, levels, out, mask)
        if open_words is None and workspace_bytes is None and kernel_ms is None:
            _stat_call("pw_pore_sizes", *args)
        else:
            w, f = _open_words(open_words, open_first, len(jobs))
            _measured("pore_sizes", args, [_pl(w)[0], _pl(f)[0], _pl(w)[1], int(workspace_bytes or 0)], kernel_ms)
        return levels, out, mask

    def affinity(self, jobs, xyz, coef, betas, words=None, edges=None, out=None, levels=None, hist=None, energies=None,
                 workspace_bytes=None, kernel_ms=None):
        """``pw_affinity``: the Lennard-Jones energy map of the regions of a batch of jobs and its Boltzmann sums
        (``AFFINITY_JOB_DTYPE`` records indexing the rows of ``xyz`` (rows of three) and of ``coef`` (rows ``(A, B)``),
        the entries of ``words`` (uint64, a region in the layout of ``pw_cavity``'s mask; ``word_first = -1``: every
        voxel), of ``betas`` and of ``edges``, and the rows and entries of the results):
        ``(out, levels, hist, energies)`` -- ``out`` an ``AFFINITY_OUT_DTYPE`` array, ``levels`` an
        ``AFFINITY_LEVEL_DTYPE`` array with ``n_betas`` rows a job from its ``level_first``, ``hist`` int64 with
        ``n_edges`` counts a job from its ``hist_first`` and ``energies`` float64 (given: filled in place, entries no
        job owns stay as they are; a job with ``energy_first >= 0`` needs ``energies`` given, since only the library
        counts the voxels of a region).  Whatever the entry refuses -- a value that is not finite or outside its
        bounds, a count or a dimension outside its range, a range outside an array, jobs that share outputs --:
        ``ValueError`` with the library's message.  ``workspace_bytes`` / ``kernel_ms`` (a list that receives the time
        of the device work by HIP events) go through the library's measurement entry."""
        jobs = _rows(jobs, dtype=AFFINITY_JOB_DTYPE)
        x, c, b = _rows(xyz, 3), _rows(coef, 2), _rows(betas)
        w, e = _rows(words, dtype=np.uint64, optional=True), _rows(edges, optional=True)
        out = _result(out, AFFINITY_OUT_DTYPE, "out", _furthest(jobs["out"] + 1))
        levels = _result(levels, AFFINITY_LEVEL_DTYPE, "levels", _furthest(jobs["level_first"] + jobs["n_betas"]))
        hist = _result(hist, np.int64, "hist", _furthest(jobs["hist_first"] + jobs["n_edges"]))
        energies = _result(energies, np.float64, "energies", 0)
        args = [self._h] + _pls(jobs, x, c, w, b, e, energies, levels, hist, out)
        if workspace_bytes is None and kernel_ms is None:
            _stat_call("pw_affinity", *args)
        else:
            _measured("affinity", args, [int(workspace_bytes or 0)], kernel_ms)
        return out, levels, hist, energies

    def rigid_affinity(self, jobs, xyz, coef, offsets, dirs, betas, words=None, out=None, levels=None, maps=None,
                       workspace_bytes=None, kernel_ms=None):
        """``pw_rigid_affinity``: the orientation-averaged affinity of the regions of a batch of jobs for a rigid linear
        guest (``RIGID_JOB_DTYPE`` records indexing the rows of ``xyz`` (rows of three), of ``coef`` (rows
        ``(A, B, C)``, row ``s * n + a`` of a job) and of ``dirs`` (rows of three), the entries of ``offsets``, of
        ``words`` (uint64, a region in the layout of ``pw_cavity``'s mask; ``word_first = -1``: every voxel) and of
        ``betas``, and the rows and entries of the results): ``(out, levels, maps)`` -- ``out`` a ``RIGID_OUT_DTYPE``
        array, ``levels`` an ``AFFINITY_LEVEL_DTYPE`` array with ``n_betas`` rows a job from its ``level_first`` and
        ``maps`` float64, two entries a voxel of a job with ``map_level >= 0`` (given: filled in place, entries no job
        owns stay as they are; such a job needs ``maps`` given, since only the library counts the voxels of a
        region).  Whatever the entry refuses: ``ValueError`` with the library's message.  ``workspace_bytes`` /
        ``kernel_ms`` (a list that receives the time of the device work by HIP events) go through the library's
        measurement entry."""
        jobs = _rows(jobs, dtype=RIGID_JOB_DTYPE)
        x, c, t, d, b = _rows(xyz, 3), _rows(coef, 3), _rows(offsets), _rows(dirs, 3), _rows(betas)
        w = _rows(words, dtype=np.uint64, optional=True)
        out = _result(out, RIGID_OUT_DTYPE, "out", _furthest(jobs["out"] + 1))
        levels = _result(levels, AFFINITY_LEVEL_DTYPE, "levels", _furthest(jobs["level_first"] + jobs["n_betas"]))
        maps = _result(maps, np.float64, "maps", 0)
        args = [self._h] + _pls(jobs, x, c, t, d, w, b, maps, levels, out)
        if workspace_bytes is None and kernel_ms is None:
            _stat_call("pw_rigid_affinity", *args)
        else:
            _measured("rigid_affinity", args, [int(workspace_bytes or 0)], kernel_ms)
        return out, levels, maps

    def rigid_body_affinity(self, jobs, xyz, coef, poses, betas, words=None, out=None, levels=None, maps=None,
                            workspace_bytes=None, kernel_ms=None):
        """``pw_rigid_body_affinity``: :meth:`rigid_affinity` for a guest that is a rigid body
        (``RIGID_BODY_JOB_DTYPE`` records): instead of offsets and directions the jobs index the rows of ``poses`` (rows of
        three), ``n_dirs * n_sites`` a job from its ``pose_first``, row ``o * n_sites + s`` the displacement of site ``s``
        from the guest's centre in pose ``o``.  The rows are data.  The results, the refusals (``ValueError`` with the
        library's message) and the measurement arguments are :meth:`rigid_affinity`'s."""
        jobs = _rows(jobs, dtype=RIGID_BODY_JOB_DTYPE)
        x, c, p, b = _rows(xyz, 3), _rows(coef, 3), _rows(poses, 3), _rows(betas)
        w = _rows(words, dtype=np.uint64, optional=True)
        out = _result(out, RIGID_OUT_DTYPE, "out", _furthest(jobs["out"] + 1))
        levels = _result(levels, AFFINITY_LEVEL_DTYPE, "levels", _furthest(jobs["level_first"] + jobs["n_betas"]))
        maps = _result(maps, np.float64, "maps", 0)
        args = [self._h] + _pls(jobs, x, c, p, w, b, maps, levels, out)
        if workspace_bytes is None and kernel_ms is None:
            _stat_call("pw_rigid_body_affinity", *args)
        else:
            _measured("rigid_body_affinity", args, [int(workspace_bytes or 0)], kernel_ms)
        return out, levels, maps

    def _rigid_cell(self, name, jobs, cell, inputs, out, levels, maps, workspace_bytes, kernel_ms, diagnostics, skip):
        """What :meth:`rigid_cell` and :meth:`rigid_cell_ewald` share: the results sized on ``cell``, the ``pw_rigid_cell``
        records of the jobs, the call of ``pw_<name>`` or of its measurement entry, and the diagnostics."""
        voxels = np.int64(1) * cell["nx"] * cell["ny"] * cell["nz"]
        out = _result(out, RIGID_OUT_DTYPE, "out", _furthest(cell["out"] + 1))
        levels = _result(levels, AFFINITY_LEVEL_DTYPE, "levels", _furthest(cell["level_first"] + cell["n_betas"]))
        maps = _result_if_any(maps, np.float64, "maps", cell["map_first"], (cell["n_betas"] + 1) * voxels)
        args = [self._h] + _pls(jobs, *inputs, maps, levels, out)
        if workspace_bytes is None and kernel_ms is None and diagnostics is None and skip:
            _stat_call("pw_" + name, *args)
            return out, levels, maps
        n_pairs, instances = np.zeros(len(jobs), dtype=np.int64), np.zeros(1, dtype=np.int32)
        _measured(name, args, [int(workspace_bytes or 0)], kernel_ms,
                  [n_pairs.ctypes.data, 1 if skip else 0, instances.ctypes.data])
        if diagnostics is not None:
            diagnostics.append((n_pairs, int(instances[0])))
        return out, levels, maps

    def rigid_cell(self, jobs, xyz, coef, offsets, dirs, betas, out=None, levels=None, maps=None, workspace_bytes=None,
                   kernel_ms=None, diagnostics=None, skip=True):
        """``pw_rigid_cell``: the orientation-averaged Boltzmann factor of a rigid linear guest at every voxel of the
        periodic cells of a batch of jobs (``RIGID_CELL_JOB_DTYPE`` records indexing the rows of ``xyz`` (rows of three),
        of ``coef`` (rows ``(A, B)``, row ``s * n + a`` of a job) and of ``dirs`` (rows of three), the entries of
        ``offsets`` and of ``betas``, and the rows and entries of the results): ``(out, levels, maps)`` -- ``out`` a
        ``RIGID_OUT_DTYPE`` array, ``levels`` an ``AFFINITY_LEVEL_DTYPE`` array with ``n_betas`` rows a job from its
        ``level_first`` and ``maps`` float64, ``n_betas + 1`` planes of ``nx * ny * nz`` entries -- ``zbar`` at every
        beta, then the lowest pose energy -- from ``map_first`` of a job that has one (``None`` when no job has one);
        given: filled in place, entries no job owns stay as they are.  Whatever the entry refuses: ``ValueError`` with
        the library's message.  ``workspace_bytes`` / ``kernel_ms`` (a list that receives the time of the device work by
        HIP events) / ``diagnostics`` (a list that receives ``(n_pairs, instances)``: the pair terms evaluated per job
        and a bit per instance of the main kernel that was launched; no part of the defined result) / ``skip=False`` (no
        atom is left out: the same bytes) go through the library's measurement entry."""
        jobs = _rows(jobs, dtype=RIGID_CELL_JOB_DTYPE)
        inputs = [_rows(xyz, 3), _rows(coef, 2), _rows(offsets), _rows(dirs, 3), _rows(betas)]
        return self._rigid_cell("rigid_cell", jobs, jobs, inputs, out, levels, maps, workspace_bytes, kernel_ms, diagnostics, skip)

    def rigid_cell_ewald(self, jobs, xyz, coef, offsets, dirs, betas, site_q, cell, kvecs, out=None, levels=None, maps=None,
                         workspace_bytes=None, kernel_ms=None, diagnostics=None, skip=True):
        """``pw_rigid_cell_ewald``: :meth:`rigid_cell` for jobs that may be charged (``RIGID_CELL_EWALD_JOB_DTYPE`` records,
        whose ``cell`` is the ``pw_rigid_cell`` job): the rows of ``coef`` are ``(A, B, C)``; ``site_q`` the site charges,
        ``cell`` rows ``(x, y, z, q)`` of the primary cell's atoms and ``kvecs`` rows ``(h, k, l, w)`` of the reciprocal
        sum (:func:`pywindow_amd.ewald_parameters`).  The results and the measurement arguments are :meth:`rigid_cell`'s."""
        jobs = _rows(jobs, dtype=RIGID_CELL_EWALD_JOB_DTYPE)
        inputs = [_rows(xyz, 3), _rows(coef, 3), _rows(offsets), _rows(dirs, 3), _rows(betas), _rows(site_q), _rows(cell, 4),
                  _rows(kvecs, 4)]
        return self._rigid_cell("rigid_cell_ewald", jobs, jobs["cell"], inputs, out, levels, maps, workspace_bytes, kernel_ms,
                                diagnostics, skip)

    def erfc(self, x):
        """The library's ``pw_erfc`` (pw_math.hpp) element by element on this context (test instrumentation): float64."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        out = np.zeros(len(x), dtype=np.float64)
        _stat_call("pw_internal_erfc", self._h, x.ctypes.data, len(x), out.ctypes.data)
        return out

    @staticmethod
    def sincos(x):
        """The library's ``ewald_sincos`` (pw_ewald.hpp: ``pw_sincos``, NaN beyond its range) element by element on the host
        (test instrumentation): ``(sin, cos)``, float64."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        s, c = np.zeros(len(x)), np.zeros(len(x))
        load().pw_internal_sincos(x.ctypes.data, len(x), s.ctypes.data, c.ctypes.data)
        return s, c

    def charges(self, jobs, xyz, params, out=None, workspace_bytes=None, kernel_ms=None):
        """``pw_charges``: charge equilibration of a batch of jobs (``CHARGES_JOB_DTYPE`` records indexing the rows of
        ``xyz`` (rows of three), the rows of ``params`` (rows ``(chi, J)`` in eV), the entries of the charges and the
        rows of the result): ``(charges, out)`` -- ``charges`` float64, zeros up to the furthest entry of a job with the
        ``n`` entries from ``charge_first`` of every job filled in, and ``out`` a ``CHARGES_OUT_DTYPE`` array with row
        ``out`` of every job (given: filled in place, rows no job owns stay as they are).  The library takes one length
        for ``xyz``, ``params`` and the charges: the shorter ones are extended here (parameter rows of zeros, which no
        job may read).  Whatever the entry refuses: ``ValueError`` with the library's message.  ``workspace_bytes`` /
        ``kernel_ms`` (a list that receives the time of the kernels by HIP events) go through the library's
        measurement entry."""
        return self._charges("charges", _rows(jobs, dtype=CHARGES_JOB_DTYPE), xyz, params, None, out, CHARGES_OUT_DTYPE,
                             workspace_bytes, kernel_ms, 1)

    def _charges(self, name, jobs, xyz, params, kvecs, out, out_dtype, workspace_bytes, kernel_ms, n_ms):
        """What :meth:`charges` and :meth:`charges_cell` share: ``xyz``, ``params`` and the charges brought to one length,
        the rows of ``out`` and the call of ``pw_<name>`` (with the rows of ``kvecs``, if any) or of its measurement
        entry, which has ``n_ms`` timers."""
        x, p = _rows(xyz, 3), _rows(params, 2)
        rows = max(_furthest(jobs["out"] + 1), 0)
        out = _result(out, out_dtype, "out", rows)
        if len(out) < rows:
            raise ValueError("out: a row for every job")
        size = max(_furthest(jobs["charge_first"] + jobs["n"]), 0)
        n_points = max(len(x), len(p), size)
        if len(x) < n_points:
            x = np.concatenate([x, np.zeros((n_points - len(x), 3))])
        if len(p) < n_points:
            p = np.concatenate([p, np.zeros((n_points - len(p), 2))])
        q = np.zeros(n_points)
        args = [self._h, *_pl(jobs), x.ctypes.data, p.ctypes.data, n_points, *(() if kvecs is None else _pl(kvecs)),
                q.ctypes.data, out.ctypes.data]
        if workspace_bytes is None and kernel_ms is None:
            _stat_call("pw_" + name, *args)
        else:
            _measured(name, args, [int(workspace_bytes or 0)], kernel_ms, n_ms=n_ms)
        return q[:size], out

    def charges_cell(self, jobs, xyz, params, kvecs, out=None, workspace_bytes=None, kernel_ms=None):
        """``pw_charges_cell``: charge equilibration on a periodic cell of a batch of jobs (``CHARGES_CELL_JOB_DTYPE``
        records indexing the rows of ``xyz`` (rows of three, in the triangular frame of the job's edges and wrapped by the
        caller), the rows of ``params`` (rows ``(chi, J)`` in eV), the rows of ``kvecs`` (rows ``(h, k, l, w)``, ``w`` in
        eV), the entries of the charges and the rows of the result): ``(charges, out)`` as :meth:`charges` returns them,
        ``out`` a ``CHARGES_CELL_OUT_DTYPE`` array.  Whatever the entry refuses: ``ValueError`` with the library's message.
        ``workspace_bytes`` / ``kernel_ms`` (a list that receives ``(count, rows, solver)``, the times of the three kinds
        of kernel in ms by HIP events) go through the library's measurement entry."""
        return self._charges("charges_cell", _rows(jobs, dtype=CHARGES_CELL_JOB_DTYPE), xyz, params, _rows(kvecs, 4), out,
                             CHARGES_CELL_OUT_DTYPE, workspace_bytes, kernel_ms, 3)

    def channels(self, jobs, xyz, radii, out=None, comps=None, mask=None, labels=None, open_words=None, open_first=None,
                 workspace_bytes=None, kernel_ms=None):
        """``pw_channels``: the periodic void components of a batch of jobs and how each winds through the cell
        (``CHANNELS_JOB_DTYPE`` records indexing the rows of ``xyz`` (rows of three), the entries of ``radii``, the rows
        of the result and of the component table, the words of ``mask`` and the bytes of ``labels``):
        ``(out, comps, mask, labels)`` -- ``out`` a ``CHANNELS_OUT_DTYPE`` array, ``comps`` a ``CHANNELS_COMP_DTYPE`` array
        with ``c_max`` rows a job from its ``comp_first``, ``mask`` the uint64 accessible words of the jobs with
        ``mask_first >= 0`` and ``labels`` the uint8 labels of the jobs with ``label_first >= 0`` (``None`` when no job
        has one).  An array that is given is filled in place, and entries no job owns stay as they are.  Whatever the
        entry refuses -- a value that is not finite, ``ax``, ``by`` or ``cz <= 0``, a negative radius or probe, a
        dimension outside ``1 .. CAVITY_MAX_G``, ``c_max`` outside ``0 .. CHAN_MAX_COMPONENTS``, a range outside an
        array, jobs that share outputs --: ``ValueError`` with the library's message.  ``open_words`` / ``open_first``
        / ``workspace_bytes`` / ``kernel_ms`` (a list that receives the time of the device work by HIP events) go
        through the library's measurement entry."""
        jobs = _rows(jobs, dtype=CHANNELS_JOB_DTYPE)
        x, r = _rows(xyz, 3), _rows(radii)
        rows = np.int64(1) * jobs["ny"] * jobs["nz"]
        c_max, voxels = jobs["c_max"].astype(np.int64), rows * jobs["nx"]
        out = _result(out, CHANNELS_OUT_DTYPE, "out", _furthest(jobs["out"] + 1))
        # (a job that would write nothing of a result counts as having none)
        comps = _result_if_any(comps, CHANNELS_COMP_DTYPE, "comps", np.where(c_max > 0, jobs["comp_first"], -1), c_max)
        mask = _result_if_any(mask, np.uint64, "mask", np.where(rows > 0, jobs["mask_first"], -1), rows)
        labels = _result_if_any(labels, np.uint8, "labels", np.where(voxels > 0, jobs["label_first"], -1), voxels)
        args = [self._h] + _pls(jobs, x, r, out, comps, mask, labels)
        if open_words is None and workspace_bytes is None and kernel_ms is None:
            _stat_call("pw_channels", *args)
        else:
            w, f = _open_words(open_words, open_first, len(jobs))
            _measured("channels", args, [_pl(w)[0], _pl(f)[0], _pl(w)[1], int(workspace_bytes or 0)], kernel_ms)
        return out, comps, mask, labels

    def percolation(self, jobs, xyz=None, coef=None, field=None, levels=None, out=None, maps=None, workspace_bytes=None,
                    kernel_ms=None, diagnostics=None):
        """``pw_percolation``: for every job of a batch (one periodic cell, one guest) the six energy levels at which the
        sub-level sets of the guest's landscape connect (``PERCOLATION_JOB_DTYPE`` records indexing the rows of ``xyz``
        (rows of three) and of ``coef`` (rows ``(A, B)``), the entries of ``field`` and of the maps and the rows of the
        results): ``(levels, out, maps)`` -- ``levels`` a ``PERCOLATION_LEVEL_DTYPE`` array with six rows a job from its
        ``level_first``, ``out`` a ``PERCOLATION_OUT_DTYPE`` array and ``maps`` the float64 fields of the jobs with
        ``map_first >= 0`` (``None`` when no job has one); given: filled in place, entries no job owns stay as they
        are.  Whatever the entry refuses -- what ``pw_channels`` refuses of a grid and ``pw_passage`` of atoms,
        coefficients and a field, a range outside an array, jobs that share outputs --: ``ValueError`` with the
        library's message.  ``workspace_bytes`` / ``kernel_ms`` (a list that receives the time of the device work by
        HIP events) / ``diagnostics`` (a list that receives ``(n_evaluations, n_fills)``, two int32 arrays over the
        jobs; they are no part of the defined result and differ between device and host) go through the library's
        measurement entry."""
        jobs = _rows(jobs, dtype=PERCOLATION_JOB_DTYPE)
        x, c, f = _rows(xyz, 3, optional=True), _rows(coef, 2, optional=True), _rows(field, optional=True)
        voxels = np.int64(1) * jobs["nx"] * jobs["ny"] * jobs["nz"]
        levels = _result(levels, PERCOLATION_LEVEL_DTYPE, "levels", _furthest(jobs["level_first"] + PERC_CRITERIA))
        out = _result(out, PERCOLATION_OUT_DTYPE, "out", _furthest(jobs["out"] + 1))
        maps = _result_if_any(maps, np.float64, "maps", jobs["map_first"], voxels)
        args = [self._h] + _pls(jobs, x, c, f, maps, levels, out)
        if workspace_bytes is None and kernel_ms is None and diagnostics is None:
            _stat_call("pw_percolation", *args)
            return levels, out, maps
        n_eval, n_fill = np.zeros(len(jobs), dtype=np.int32), np.zeros(len(jobs), dtype=np.int32)
        _measured("percolation", args, [int(workspace_bytes or 0)], kernel_ms, [n_eval.ctypes.data, n_fill.ctypes.data])
        if diagnostics is not None:
            diagnostics.append((n_eval, n_fill))
        return levels, out, maps

    def basins(self, jobs, xyz=None, coef=None, field=None, out=None, basins=None, edges=None, maps=None, labels=None,
               workspace_bytes=None, kernel_ms=None, diagnostics=None):
        """``pw_basins``: for every job of a batch (one periodic cell, one guest, up to eight inverse temperatures and an
        energy cap) the basins of steepest descent of the guest's landscape, the dividing surfaces between them with
        their integer cell offsets, and the Boltzmann sums over both (``BASINS_JOB_DTYPE`` records indexing the rows of
        ``xyz`` (rows of three) and of ``coef`` (rows ``(A, B)``), the entries of ``field``, of the maps and of the
        labels and the rows of the results): ``(out, basins, edges, maps, labels)`` -- ``out`` a ``BASINS_OUT_DTYPE``
        array, ``basins`` a ``BASINS_BASIN_DTYPE`` array with ``n_basins_written`` rows a job from its ``basin_first``,
        ``edges`` a ``BASINS_EDGE_DTYPE`` array with ``n_edges_written`` rows a job from its ``edge_first``, ``maps``
        the float64 fields of the jobs with ``map_first >= 0`` and ``labels`` the ``BASINS_LABEL_DTYPE`` entries of the
        jobs with ``label_first >= 0`` (``None`` when no job has one); given: filled in place, entries no job writes
        stay as they are.  Whatever the entry refuses -- what ``pw_percolation`` refuses, a negative capacity,
        ``n_betas`` outside 1 .. 8, a beta that is not positive, a cap that is no number --: ``ValueError`` with the
        library's message.  ``workspace_bytes`` / ``kernel_ms`` (a list that receives the time of the device work by HIP
        events) / ``diagnostics`` (a list that receives ``(n_rounds, n_faces)``, two int32 arrays over the jobs; they
        are no part of the defined result) go through the library's measurement entry."""
        jobs = _rows(jobs, dtype=BASINS_JOB_DTYPE)
        x, c, f = _rows(xyz, 3, optional=True), _rows(coef, 2, optional=True), _rows(field, optional=True)
        voxels = np.int64(1) * jobs["nx"] * jobs["ny"] * jobs["nz"]
        out = _result(out, BASINS_OUT_DTYPE, "out", _furthest(jobs["out"] + 1))
        basins = _result(basins, BASINS_BASIN_DTYPE, "basins", _furthest(jobs["basin_first"] + jobs["b_cap"]))
        edges = _result(edges, BASINS_EDGE_DTYPE, "edges", _furthest(jobs["edge_first"] + jobs["e_cap"]))
        maps = _result_if_any(maps, np.float64, "maps", jobs["map_first"], voxels)
        labels = _result_if_any(labels, BASINS_LABEL_DTYPE, "labels", jobs["label_first"], voxels)
        args = [self._h] + _pls(jobs, x, c, f, maps, basins, edges, labels, out)
        if workspace_bytes is None and kernel_ms is None and diagnostics is None:
            _stat_call("pw_basins", *args)
            return out, basins, edges, maps, labels
        n_rounds, n_faces = np.zeros(len(jobs), dtype=np.int32), np.zeros(len(jobs), dtype=np.int32)
        _measured("basins", args, [int(workspace_bytes or 0)], kernel_ms, [n_rounds.ctypes.data, n_faces.ctypes.data])
        if diagnostics is not None:
            diagnostics.append((n_rounds, n_faces))
        return out, basins, edges, maps, labels

    def passage(self, jobs, xyz=None, coef=None, planes=None, field=None, out=None, workspace_bytes=None, kernel_ms=None,
                fills=None, grids=None):
        """``pw_passage``: the barrier between the seed voxel and the faces of the box of every job of a batch, one row
        per plane left out (``PASSAGE_JOB_DTYPE`` records indexing the rows of ``xyz`` (rows of three), of ``coef``
        (rows ``(A, B)``) and of ``planes`` (rows of four), the entries of ``field`` and the rows of the result): a
        ``PASSAGE_OUT_DTYPE`` array with ``max(m, 1)`` rows a job from its ``out_first`` -- ``out`` given: filled in
        place, rows no job owns stay as they are.  Whatever the entry refuses -- what ``pw_cavity`` and ``pw_affinity``
        refuse for the same fields, a field value that is ``-inf`` or not a number, a range outside an array, jobs that
        share rows --: ``ValueError`` with the library's message.  ``workspace_bytes`` / ``kernel_ms`` (a list that
        receives the time of the device work by HIP events) / ``fills`` (an int32 array as long as ``out`` that
        receives the number of flood fills of every row) / ``grids`` (3: the kernel without its fourth bit grid, for
        the measurement of what that grid buys; the result does not depend on it) go through the library's measurement
        entry."""
        jobs = _rows(jobs, dtype=PASSAGE_JOB_DTYPE)
        x, c = _rows(xyz, 3, optional=True), _rows(coef, 2, optional=True)
        p, f = _rows(planes, 4, optional=True), _rows(field, optional=True)
        out = _result(out, PASSAGE_OUT_DTYPE, "out", _furthest(jobs["out_first"] + np.maximum(jobs["m"], 1)))
        args = [self._h] + _pls(jobs, x, c, p, f, out)
        if workspace_bytes is None and kernel_ms is None and fills is None and grids is None:
            _stat_call("pw_passage", *args)
            return out
        if fills is not None and (fills.dtype != np.int32 or not fills.flags.c_contiguous or fills.shape != out.shape):
            raise ValueError("fills: a C-contiguous int32 array as long as out")
        _measured("passage", args, [int(workspace_bytes or 0)], kernel_ms, [_pl(fills)[0], int(grids or 0)])
        return out

    def hop(self, jobs, betas, xyz=None, coef=None, planes=None, field=None, slabs=None, sums=None, out=None, words=None,
            workspace_bytes=None, kernel_ms=None):
        """``pw_hop``: per slab of the grid of every job of a batch, the 2-D component of allowed voxels round the seed
        column and its Boltzmann sums (``HOP_JOB_DTYPE`` records indexing the rows of ``xyz`` (rows of three), of ``coef``
        (rows ``(A, B)``) and of ``planes`` (rows of four), the entries of ``field`` and of ``betas`` and the rows and
        entries of the results): ``(slabs, sums, out, words)`` -- ``slabs`` a ``HOP_SLAB_DTYPE`` array with ``nz`` rows
        a job from its ``slab_first``, ``sums`` an ``AFFINITY_LEVEL_DTYPE`` array with ``nz * n_betas`` rows a job from
        its ``sum_first``, ``out`` a ``HOP_OUT_DTYPE`` array and ``words`` the uint64 words of the jobs with
        ``word_first >= 0``, ``ny * nz`` a job (``None`` when no job has one); given: filled in place, entries no job
        owns stay as they are.  Whatever the entry refuses -- what ``pw_passage`` refuses for the same fields, a cap
        that is not finite, a seed column outside the grid, a beta that is negative or not finite, a range outside an
        array, jobs that share outputs --: ``ValueError`` with the library's message.  ``workspace_bytes`` /
        ``kernel_ms`` (a list that receives ``(total, field kernels, slab kernels)`` in ms by HIP events) go through the
        library's measurement entry."""
        jobs = _rows(jobs, dtype=HOP_JOB_DTYPE)
        b, x, c = _rows(betas), _rows(xyz, 3, optional=True), _rows(coef, 2, optional=True)
        p, f = _rows(planes, 4, optional=True), _rows(field, optional=True)
        nz = jobs["nz"].astype(np.int64)
        slabs = _result(slabs, HOP_SLAB_DTYPE, "slabs", _furthest(jobs["slab_first"] + nz))
        sums = _result(sums, AFFINITY_LEVEL_DTYPE, "sums", _furthest(jobs["sum_first"] + nz * jobs["n_betas"]))
        out = _result(out, HOP_OUT_DTYPE, "out", _furthest(jobs["out"] + 1))
        words = _result_if_any(words, np.uint64, "words", jobs["word_first"], jobs["ny"].astype(np.int64) * jobs["nz"])
        args = [self._h] + _pls(jobs, x, c, p, f, b, slabs, sums, out, words)
        if workspace_bytes is None and kernel_ms is None:
            _stat_call("pw_hop", *args)
        else:
            _measured("hop", args, [int(workspace_bytes or 0)], kernel_ms, n_ms=3)
        return slabs, sums, out, words

    def circumcircle(self, coordinates, atom_sets):
        """``pw_circumcircle``: (diameters (K,), centres (K, 3)) for K atom triples of one molecule."""
        xyz = np.ascontiguousarray(coordinates, dtype=np.float64).reshape(-1, 3)
        sets = np.array(atom_sets, dtype=np.int32).reshape(-1, 3)
        sets = np.ascontiguousarray(np.where((sets < 0) & (sets >= -len(xyz)), sets + len(xyz), sets))   # Python indexing
        d = np.zeros(len(sets))
        c = np.zeros((len(sets), 3))
        rc = load().pw_circumcircle(self._h, xyz.ctypes.data, len(xyz), sets.ctypes.data, len(sets),
                                    d.ctypes.data, c.ctypes.data)
        if rc == -2 and len(sets) and ((sets < 0) | (sets >= len(xyz))).any():
            raise IndexError("atom index out of range")      # what indexing the array raises in the reference
        _check(rc, "pw_circumcircle")
        return d, c

    def discrete_molecules(self, topology, coords, lattice, lattice_inv, rebuild: bool, atoms_cap=None):
        """``pw_discrete_molecules`` on F frames of one topology (see pywindow_amd/rebuild.py).
        Returns ``(n_mol, mol_offset, src_atom, src_image, xyz, status)``; output capacity grows
        automatically when a frame reports an overflow."""
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        f, n, _ = coords.shape
        if n != topology.n:
            raise ValueError("coordinates do not match the topology")
        cap = int(atoms_cap) if atoms_cap else (2 * n if rebuild else n)
        mols = min(cap, n)
        for _attempt in range(6):
            n_mol = np.zeros(f, np.int32)
            status = np.zeros(f, np.int32)
            off = np.zeros((f, mols + 1), np.int32)
            src = np.zeros((f, cap), np.int32)
            img = np.zeros((f, cap), np.int8)
            xyz = np.zeros((f, cap, 3))
            cin = CellIn(f, n, 1 if rebuild else 0, coords.ctypes.data,
                         None if lattice is None else lattice.ctypes.data,
                         None if lattice_inv is None else lattice_inv.ctypes.data,
                         topology.cov.ctypes.data, topology.mass.ctypes.data, topology.terminal.ctypes.data,
                         topology.max_dist, topology.tol)
            cout = CellOut(cap, mols, n_mol.ctypes.data, status.ctypes.data, off.ctypes.data, src.ctypes.data,
                           img.ctypes.data, xyz.ctypes.data)
            _check(load().pw_discrete_molecules(self._h, ctypes.byref(cin), ctypes.byref(cout)),
                   "pw_discrete_molecules")
            if not (status & (RB_ATOMS_OVERFLOW | RB_MOLS_OVERFLOW)).any():
                break
            cap *= 4
            mols = min(cap, 4 * mols)
        else:
            raise PwHipError("pw_discrete_molecules: output does not fit (molecule larger than 2048 x the cell?)")
        bad = status & ~(RB_ATOMS_OVERFLOW | RB_MOLS_OVERFLOW)
        if bad.any():
            raise PwHipError(f"pw_discrete_molecules: unsupported input ({rb_status_text(int(np.bitwise_or.reduce(bad)))})")
        return n_mol, off, src, img, xyz

    def resident_from_cells(self, topology, vdw, coords, lattice, lattice_inv, rebuild: bool):
        """Frames -> discrete molecules -> ONE resident batch, all on the device
        (``pw_resident_from_cells``).  Returns ``(resident or None, n_mol per frame)``."""
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        vdw = np.ascontiguousarray(vdw, dtype=np.float64)
        f, n, _ = coords.shape
        if n != topology.n or len(vdw) != n:
            raise ValueError("coordinates / radii do not match the topology")
        cap = 2 * n if rebuild else n
        mols = min(cap, n)
        for _attempt in range(6):
            n_mol = np.zeros(f, np.int32)
            status = np.zeros(f, np.int32)
            cin = CellIn(f, n, 1 if rebuild else 0, coords.ctypes.data,
                         None if lattice is None else lattice.ctypes.data,
                         None if lattice_inv is None else lattice_inv.ctypes.data,
                         topology.cov.ctypes.data, topology.mass.ctypes.data, topology.terminal.ctypes.data,
                         topology.max_dist, topology.tol)
            h = ctypes.c_void_p()
            rc = load().pw_resident_from_cells(self._h, ctypes.byref(cin), vdw.ctypes.data, cap, mols,
                                               ctypes.byref(h), n_mol.ctypes.data, status.ctypes.data)
            if rc == -4:                 # PW_E_TOO_LARGE: a frame needs more room
                cap *= 4
                mols = min(cap, 4 * mols)
                continue
            _check(rc, "pw_resident_from_cells")
            break
        else:
            raise PwHipError("pw_resident_from_cells: output does not fit")
        bad = status & ~(RB_ATOMS_OVERFLOW | RB_MOLS_OVERFLOW)
        if bad.any():
            if h:
                load().pw_resident_free(self._h, h)
            raise PwHipError(f"pw_resident_from_cells: unsupported input ({rb_status_text(int(np.bitwise_or.reduce(bad)))})")
        res = Resident._adopt(self, h, int(n_mol.sum())) if h else None
        return res, n_mol

    def upload(self, batch: Batch) -> "Resident":
        return Resident(self, batch)

    def stream_begin(self, n_units: int, vdw, mass) -> "Resident":
        """A batch of ``n_units`` molecules of one type whose coordinates will arrive in pieces
        (``pw_resident_stream_begin``): launch it at once, then ``append`` the coordinates in unit order."""
        vdw = np.ascontiguousarray(vdw, dtype=np.float64)
        mass = np.ascontiguousarray(mass, dtype=np.float64)
        if len(vdw) != len(mass) or not len(vdw):
            raise ValueError("one radius and one mass per atom of the molecule")
        h = ctypes.c_void_p()
        _check(load().pw_resident_stream_begin(self._h, int(n_units), len(vdw), vdw.ctypes.data, mass.ctypes.data,
                                               ctypes.byref(h)), "pw_resident_stream_begin")
        res = Resident._adopt(self, h, int(n_units))
        res.atoms = len(vdw)
        res.appended = 0
        return res

    @property
    def stream(self) -> int:
        return load().pw_context_stream(self._h) or 0


class Resident:
    """A batch kept in HBM across launches."""

    def __init__(self, ctx: Context, batch: Batch):
        self.ctx = ctx
        self.n_units = batch.n_units
        h = ctypes.c_void_p()
        _check(load().pw_resident_upload(ctx._h, ctypes.byref(batch.c), ctypes.byref(h)), "pw_resident_upload")
        self._h = h

    @classmethod
    def _adopt(cls, ctx: Context, handle, n_units: int) -> "Resident":
        obj = cls.__new__(cls)
        obj.ctx = ctx
        obj.n_units = n_units
        obj._h = handle
        return obj

    def append(self, coords) -> None:
        """Coordinates ``(count, atoms, 3)`` of the next units of a streamed batch (``Context.stream_begin``).
        ``coords`` should lie in the context's page-locked buffer (``Context.pinned_array``: the copy is then a DMA);
        the call returns when they are on the device."""
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        if coords.ndim != 3 or coords.shape[1:] != (self.atoms, 3):
            raise ValueError("coordinates must be (count, atoms, 3)")
        _check(load().pw_resident_stream_append(self.ctx._h, self._h, coords.ctypes.data, self.appended, len(coords)),
               "pw_resident_stream_append")
        self.appended += len(coords)

    def append_from_history(self, history_handle, first_frame: int, staging, min_append: int = 64) -> tuple[float, float]:
        """Frames ``first_frame ..`` of an open HISTORY (``pw_history*``) decoded into ``staging`` (``(count, atoms, 3)``,
        page-locked) and appended as the next units WHILE they are decoded (``pw_history_stream_read``).  Returns
        (ms until the last frame was decoded, ms from there until the last append had returned)."""
        if staging.ndim != 3 or staging.shape[1:] != (self.atoms, 3) or not staging.flags.c_contiguous or staging.dtype != np.float64:
            raise ValueError("staging must be a C-contiguous float64 (count, atoms, 3) array")
        legs = (ctypes.c_double * 2)()
        _check(load().pw_history_stream_read(history_handle, int(first_frame), len(staging), self.ctx._h, self._h, self.appended,
                                             staging.ctypes.data, int(min_append), legs), "pw_history_stream_read")
        self.appended += len(staging)
        return float(legs[0]), float(legs[1])

    def launch(self, stages: int = STAGE_ALL):
        self._stages = stages
        _check(load().pw_resident_launch(self.ctx._h, self._h, stages), "pw_resident_launch")

    def sync(self):
        _check(load().pw_resident_sync(self.ctx._h), "pw_resident_sync")

    def download(self, extra=None) -> np.ndarray:
        """Records of the latest launch.  ``extra``: a list that receives the windows beyond ``W_MAX``
        (``EXTRA_WINDOW_DTYPE``) when a unit has any.  The device list for those only exists once a launch
        has asked for it (``PW_E_RETRY``): the analysis is then launched once more, here."""
        out = np.zeros(self.n_units, dtype=UNIT_OUT_DTYPE)
        if self.n_units:
            with self.ctx.lock:       # (the records and "the windows beyond W_MAX of the records fetched last" belong together)
                rc = load().pw_resident_download(self.ctx._h, self._h, out.ctypes.data)
                if rc == E_RETRY:
                    self.launch(getattr(self, "_stages", STAGE_ALL))
                    rc = load().pw_resident_download(self.ctx._h, self._h, out.ctypes.data)
                repeats = 0
                while rc == E_TIMEOUT and repeats < timeout_repeats():
                    # a launch that saw another launch of the same analysis make no progress for a whole limit
                    # (PW_WAIT_LIMIT_MS, 250 ms): the analysis is repeated, up to PW_TIMEOUT_REPEATS (2) times -- the
                    # next time-out is raised -- and every repeat is COUNTED (Context.retries, retries_total(): the
                    # bench line and the suite's last test look at them) and logged
                    import logging

                    logging.getLogger("pywindow_amd").warning("analysis repeated after: %s", load().pw_last_error().decode(errors="replace"))
                    load().pw_context_count_retry(self.ctx._h)
                    repeats += 1
                    self.launch(getattr(self, "_stages", STAGE_ALL))
                    rc = load().pw_resident_download(self.ctx._h, self._h, out.ctypes.data)
                _check(rc, "pw_resident_download")
                if extra is not None and (out["status"] & ST_WINDOW_OVERFLOW).any():
                    extra.append(self.ctx.extra_windows())
        return out

    def download_settled(self, extra=None) -> np.ndarray:
        """``download`` for the resident path with what ``pw_analysis_batch`` does for the one-call path: a
        unit that wanted more sampling vectors than the launch's workspace held (``PW_ST_POINTS_OVERFLOW``:
        a sphere of thousands of angstroms) raises the context's capacity and the analysis is launched again,
        so no capacity of the engine shows in a result.  Download and extra windows under the context's lock."""
        with self.ctx.lock:
            attempt = 0
            while True:
                mine = []
                out = self.download(mine)
                flagged = out[(out["status"] & ST_POINTS_OVERFLOW) != 0]
                want = int(max(flagged["n_points"].max(), flagged["n_points_avg"].max())) if len(flagged) else 0
                attempt += 1
                # (no launch after the last download: what is returned is what the latest launch wrote)
                if want <= self.ctx.point_capacity or attempt >= 3:
                    break
                self.ctx.reserve_points(want)
                self.launch(getattr(self, "_stages", STAGE_ALL))
            if extra is not None:
                extra.extend(mine)
            return out

    def check(self) -> np.ndarray:
        """For callers that read the records on the device: wait for the latest launch, raise if its
        window launch timed out, and return its windows beyond ``W_MAX`` (``EXTRA_WINDOW_DTYPE``; empty
        for all but unusual molecules).  ``PW_E_RETRY`` (the device list for such windows had to be
        allocated first) is passed on as :class:`PwRetry`: launch again."""
        n = ctypes.c_int64(0)
        rc = load().pw_resident_extra_windows(self.ctx._h, self._h, ctypes.byref(n))
        if rc == E_RETRY:
            raise PwRetry(load().pw_last_error().decode(errors="replace"))
        _check(rc, "pw_resident_extra_windows")
        return self.ctx.extra_windows() if n.value else np.zeros(0, dtype=EXTRA_WINDOW_DTYPE)

    def time_launches(self, iters: int, stages: int = STAGE_ALL) -> float:
        ms = ctypes.c_float()
        _check(load().pw_resident_time(self.ctx._h, self._h, stages, iters, ctypes.byref(ms)), "pw_resident_time")
        return float(ms.value)

    def stage_times(self) -> dict:
        """Milliseconds of the two launches of ONE analysis run on its own (HIP events on each launch's stream):
        ``{"chains", "windows"}`` -- the average diameter is a stage of the window teams."""
        ms = (ctypes.c_float * 3)()
        _check(load().pw_resident_stage_times(self.ctx._h, self._h, ms), "pw_resident_stage_times")
        return {"chains": float(ms[0]), "windows": float(ms[2])}

    @property
    def device_results_ptr(self) -> int:
        return load().pw_resident_device_results(self._h) or 0

    def results_ready(self, stream: int = 0) -> int:
        """Make HIP stream ``stream`` (a ``hipStream_t`` as an integer; 0 = the default stream) wait
        for the latest launch; returns the device address of its records."""
        ptr = ctypes.c_void_p()
        _check(load().pw_resident_results_ready(self.ctx._h, self._h, ctypes.c_void_p(stream or None),
                                                ctypes.byref(ptr)), "pw_resident_results_ready")
        return ptr.value or 0

    def results_release(self, stream: int = 0) -> None:
        """The launch that next overwrites the records waits for what ``stream`` holds so far."""
        _check(load().pw_resident_results_release(self.ctx._h, self._h, ctypes.c_void_p(stream or None)),
               "pw_resident_results_release")

    def free(self):
        if self._h:
            load().pw_resident_free(self.ctx._h, self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.free()
        except Exception:
            pass
