"""ctypes mirror of include/hsddp.h (struct layouts + prototypes).

Used by the product wrapper (`MultiPhaseDDP` in __init__.py, bound to libhsddp_hip.so) and by the
tests to drive the CPU checker library through the *same* ABI (the tests pass its path in).  Nothing here computes anything.
"""
import ctypes as C
import numpy as np

MODEL_WB, MODEL_SRB, MODEL_HKD = 0, 1, 2
MODEL_DIMS = {MODEL_WB: (36, 12, 12), MODEL_SRB: (12, 12, 0), MODEL_HKD: (24, 24, 0)}

FIELDS = ["X", "XBAR", "XSIM", "DEFECT", "DX", "G", "U", "UBAR", "DU", "QU", "Y", "K", "QUX", "QUU",
          "A", "B", "C", "D", "L", "LX", "LU", "LY", "LXX", "LUX", "LUU", "LYY", "PHI", "PHIX", "PHIXX", "H0",
          "REB_EPS", "REB_DELTA", "AL_SIGMA", "AL_LAMBDA"]
FIELD_ID = {n: i for i, n in enumerate(FIELDS)}


class Option(C.Structure):
    """HSDDP_OPTION (HSDDPSolver/common/HSDDP_CompoundTypes.h:13-36); defaults = the struct defaults there."""
    _fields_ = [(n, C.c_double) for n in ("alpha", "gamma", "update_penalty", "update_relax", "update_regularization", "update_ReB")] + \
               [(n, C.c_int) for n in ("max_DDP_iter", "max_AL_iter", "max_DDP_iter_runtime", "max_AL_iter_runtime")] + \
               [(n, C.c_double) for n in ("cost_thresh", "tconstr_thresh", "pconstr_thresh", "dynamics_feas_thresh",
                                          "merit_rho", "merit_scale", "merit_offset")] + \
               [(n, C.c_int) for n in ("AL_active", "ReB_active", "smooth_active", "MS", "nsteps_per_node")]

    def __init__(self, **kw):
        super().__init__()
        d = dict(alpha=0.1, gamma=0.1, update_penalty=8, update_relax=0.1, update_regularization=2, update_ReB=7,
                 max_DDP_iter=3, max_AL_iter=2, max_DDP_iter_runtime=1, max_AL_iter_runtime=2, cost_thresh=1e-3,
                 tconstr_thresh=1e-3, pconstr_thresh=1e-3, dynamics_feas_thresh=1e-3, merit_rho=1e4, merit_scale=0.2,
                 merit_offset=10, AL_active=1, ReB_active=1, smooth_active=0, MS=1, nsteps_per_node=1)
        d.update(kw)
        for k, v in d.items():
            setattr(self, k, v)


def mhpc_ddp_setting(**kw):
    """MHPC/settings/ddp_setting.info as loadHSDDPSetting reads it (update_regularization is NOT read: quirk xiii)."""
    d = dict(alpha=0.5, gamma=0.1, update_penalty=5, update_relax=1, update_ReB=1, update_regularization=2,
             max_DDP_iter=10, max_AL_iter=20, max_DDP_iter_runtime=1, max_AL_iter_runtime=4, cost_thresh=1e-2,
             tconstr_thresh=1e-3, pconstr_thresh=1e-3, dynamics_feas_thresh=1e-3, merit_rho=1e3, merit_scale=0.2,
             merit_offset=1, AL_active=1, ReB_active=1, smooth_active=0, MS=1, nsteps_per_node=1)
    d.update(kw)
    return Option(**d)


class Reb(C.Structure):
    _fields_ = [("delta", C.c_double), ("delta_min", C.c_double), ("eps", C.c_double)]


class Al(C.Structure):
    _fields_ = [("sigma", C.c_double), ("lambda_", C.c_double), ("sigma_max", C.c_double)]


DP = C.POINTER(C.c_double)
IP = C.POINTER(C.c_int)


class PhaseDesc(C.Structure):
    _fields_ = [("model", C.c_int), ("horizon", C.c_int), ("dt", C.c_double), ("t_offset", C.c_double),
                ("contact", C.c_int * 4), ("next_contact", C.c_int * 4), ("next_model", C.c_int), ("shooting", C.c_int),
                ("BG_alpha", C.c_double),
                ("q", C.c_double * 36), ("r", C.c_double * 24), ("qf", C.c_double * 36),
                ("w_foot_reg", C.c_double * 3), ("w_swing_pos", C.c_double * 3), ("w_swing_vel", C.c_double * 3),
                ("w_td_vel", C.c_double),
                ("c_torque", C.c_int), ("c_joint", C.c_int), ("c_minheight", C.c_int), ("c_grf", C.c_int),
                ("torque_limit", C.c_double), ("joint_lb", C.c_double * 3), ("joint_ub", C.c_double * 3),
                ("h_min", C.c_double), ("mu", C.c_double),
                ("reb_torque", Reb), ("reb_joint", Reb), ("reb_minheight", Reb), ("reb_grf", Reb),
                ("c_jointspeed", C.c_int), ("jointspeed_lb", C.c_double), ("jointspeed_ub", C.c_double), ("reb_jointspeed", Reb),
                ("c_touchdown", C.c_int), ("ground_height", C.c_double), ("al_td", Al),
                ("xr", DP), ("ur", DP), ("yr", DP), ("foot_pos", DP), ("foot_vel", DP), ("body_pos", DP),
                ("ref_contact", IP)]


class ModelParam(C.Structure):
    _fields_ = [("psi_dyn", C.c_double), ("psi_kin", C.c_double)]


class Info(C.Structure):
    _fields_ = [("actual_cost", C.c_double), ("dyn_feas", C.c_double), ("max_tconstr", C.c_double), ("max_pconstr", C.c_double),
                ("n_iters", C.c_int), ("n_ls_iters", C.c_int), ("n_reg_iters", C.c_int), ("status", C.c_int)]


PREC_F64, PREC_F32 = 0, 1

EXPORTS = ["hsddp_create", "hsddp_create_ex", "hsddp_precision", "hsddp_destroy", "hsddp_set_initial_condition", "hsddp_set_nominal", "hsddp_solve",
           "hsddp_hybrid_rollout", "hsddp_compute_cost", "hsddp_LQ_approximation", "hsddp_backward_sweep",
           "hsddp_linear_rollout", "hsddp_update_nominal_trajectory", "hsddp_get_exp_cost_change",
           "hsddp_measure_dynamics_feasibility", "hsddp_get_info", "hsddp_get_field", "hsddp_field_shape",
           "hsddp_get_solve_time_ms", "hsddp_get_kernel_times", "hsddp_get_kernel_units", "hsddp_reset_kernel_times", "hsddp_get_history",
           "hsddp_export_mpc_command", "hsddp_warm_start_phase", "hsddp_reconfigure", "hsddp_set_control_knot", "hsddp_export_solver_info", "hsddp_debug_malloc_count", "hsddp_backend_name"]


def bind(lib):
    """Attach argtypes/restypes for every entry point of include/hsddp.h to a loaded CDLL."""
    H = C.c_void_p
    OP = C.POINTER(Option)
    lib.hsddp_create.argtypes = [C.POINTER(H), C.c_int, C.POINTER(PhaseDesc), C.POINTER(ModelParam), C.c_int, C.c_int]
    lib.hsddp_create_ex.argtypes = [C.POINTER(H), C.c_int, C.POINTER(PhaseDesc), C.POINTER(ModelParam), C.c_int, C.c_int, C.c_int]
    lib.hsddp_precision.argtypes = [H]
    lib.hsddp_destroy.argtypes = [H]
    lib.hsddp_destroy.restype = None
    lib.hsddp_set_initial_condition.argtypes = [H, DP]
    lib.hsddp_set_nominal.argtypes = [H, C.c_int, DP, DP, C.c_int]
    lib.hsddp_solve.argtypes = [H, OP, C.c_float]
    lib.hsddp_hybrid_rollout.argtypes = [H, C.c_double, OP]
    lib.hsddp_compute_cost.argtypes = [H, OP]
    lib.hsddp_LQ_approximation.argtypes = [H, OP]
    lib.hsddp_backward_sweep.argtypes = [H, C.c_double, IP]
    lib.hsddp_linear_rollout.argtypes = [H, C.c_double, OP]
    lib.hsddp_update_nominal_trajectory.argtypes = [H]
    lib.hsddp_get_exp_cost_change.argtypes = [H, DP, DP]
    lib.hsddp_measure_dynamics_feasibility.argtypes = [H, DP]
    lib.hsddp_get_info.argtypes = [H, C.POINTER(Info)]
    lib.hsddp_get_field.argtypes = [H, C.c_int, C.c_int, C.c_int, C.c_int, DP]
    lib.hsddp_field_shape.argtypes = [H, C.c_int, C.c_int, IP, IP]
    lib.hsddp_get_solve_time_ms.argtypes = [H]
    lib.hsddp_get_solve_time_ms.restype = C.c_float
    lib.hsddp_get_kernel_times.argtypes = [H, C.c_int, DP, C.POINTER(C.c_longlong), C.c_char_p, C.c_int]
    lib.hsddp_get_kernel_units.argtypes = [H, C.c_char_p, C.POINTER(C.c_longlong)]
    lib.hsddp_reset_kernel_times.argtypes = [H]
    FP = C.POINTER(C.c_float)
    lib.hsddp_get_history.argtypes = [H, C.c_int, C.c_int, FP, FP, FP, FP, IP]
    lib.hsddp_export_mpc_command.argtypes = [H, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_float), C.POINTER(C.c_uint)]
    lib.hsddp_warm_start_phase.argtypes = [H, C.c_int, H, C.c_int, C.c_int]
    lib.hsddp_reconfigure.argtypes = [H, C.c_int, C.POINTER(PhaseDesc), IP, IP]
    lib.hsddp_set_control_knot.argtypes = [H, C.c_int, C.c_int, C.c_void_p]
    lib.hsddp_export_solver_info.argtypes = [H, C.c_int, C.c_void_p]
    lib.hsddp_debug_malloc_count.argtypes = []
    lib.hsddp_debug_malloc_count.restype = C.c_longlong
    lib.hsddp_backend_name.argtypes = []
    lib.hsddp_backend_name.restype = C.c_char_p
    return lib


# include/hsddp_ensemble.h: a header of its own (hsddp.h and EXPORTS above are the single-handle ABI both libraries export)
ENSEMBLE_EXPORTS = ["hsddp_ensemble_create", "hsddp_ensemble_destroy", "hsddp_ensemble_solve", "hsddp_ensemble_select",
                    "hsddp_ensemble_export_mpc_commands"]


def bind_ensemble(lib):
    """Attach argtypes/restypes for the entry points of include/hsddp_ensemble.h.  Raises if the library lacks any of them."""
    missing = [s for s in ENSEMBLE_EXPORTS if not hasattr(lib, s)]
    if missing:
        raise RuntimeError(f"library lacks the ensemble entry points {missing}")
    H = C.c_void_p
    lib.hsddp_ensemble_create.argtypes = [C.POINTER(H), C.c_int, C.POINTER(H)]
    lib.hsddp_ensemble_destroy.argtypes = [H]
    lib.hsddp_ensemble_destroy.restype = None
    lib.hsddp_ensemble_solve.argtypes = [H, C.POINTER(Option), C.c_float, C.c_int]
    lib.hsddp_ensemble_select.argtypes = [H, C.POINTER(Option), IP, C.c_void_p]
    lib.hsddp_ensemble_export_mpc_commands.argtypes = [H, C.c_int, IP, IP, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int]
    return lib


# include/hsddp_hkd.h: the HKD-MPC command export (libhsddp_hip.so only; EXPORTS above stay the ABI both libraries share)
HKD_EXPORTS = ["hsddp_export_hkd_commands", "hsddp_export_hkd_command"]
HKD_CMD_WORDS = 1954      # HSDDP_HKD_CMD_WORDS
HKD_MAX_STEPS = 10        # HSDDP_HKD_MAX_STEPS


def bind_hkd(lib):
    """Attach argtypes/restypes for the entry points of include/hsddp_hkd.h.  Raises if the library lacks any of them."""
    missing = [s for s in HKD_EXPORTS if not hasattr(lib, s)]
    if missing:
        raise RuntimeError(f"library lacks the HKD export entry points {missing}")
    H = C.c_void_p
    lib.hsddp_export_hkd_commands.argtypes = [H, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.hsddp_export_hkd_command.argtypes = [H, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


# include/hsddp_refs.h: per-problem tracking references (libhsddp_hip.so only)
REFS_EXPORTS = ["hsddp_set_references", "hsddp_get_references"]
REF_FIELDS = ("xr", "ur", "yr", "foot_pos", "foot_vel", "body_pos", "ref_contact")     # hsddp_refs_t order


class Refs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in REF_FIELDS]


def ref_widths(model):
    """Row widths of the seven reference arrays of a phase of `model` (those of hsddp_phase_desc_t)."""
    n, m, p = MODEL_DIMS[model]
    return dict(xr=n, ur=m, yr=p, foot_pos=12, foot_vel=12, body_pos=3, ref_contact=4)


def bind_refs(lib):
    """Attach argtypes/restypes for the entry points of include/hsddp_refs.h.  Raises if the library lacks any of them."""
    missing = [s for s in REFS_EXPORTS if not hasattr(lib, s)]
    if missing:
        raise RuntimeError(f"library lacks the per-problem reference entry points {missing}")
    H = C.c_void_p
    lib.hsddp_set_references.argtypes = [H, C.c_int, C.c_int, C.c_int, C.POINTER(Refs), C.c_int]
    lib.hsddp_get_references.argtypes = [H, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7
    return lib


# include/hsddp_sim.h: closed-loop rollouts of the solved policy from perturbed initial states (libhsddp_hip.so only)
SIM_EXPORTS = ["hsddp_sim_create", "hsddp_sim_run", "hsddp_sim_get_rows", "hsddp_sim_get_traj", "hsddp_sim_device_final",
               "hsddp_sim_get_kernel_time_ms", "hsddp_sim_destroy"]


class SimRow(C.Structure):
    """hsddp_sim_row_t"""
    _fields_ = [("dev_q", C.c_double), ("dev_v", C.c_double), ("min_height", C.c_double), ("max_torque", C.c_double),
                ("first_bad", C.c_int), ("pad", C.c_int)]


SIM_ROW_DTYPE = np.dtype([("dev_q", "<f8"), ("dev_v", "<f8"), ("min_height", "<f8"), ("max_torque", "<f8"), ("first_bad", "<i4"), ("pad", "<i4")])


def bind_sim(lib):
    """Attach argtypes/restypes for the entry points of include/hsddp_sim.h.  Raises if the library lacks any of them."""
    missing = [s for s in SIM_EXPORTS if not hasattr(lib, s)]
    if missing:
        raise RuntimeError(f"library lacks the simulation entry points {missing}")
    H = C.c_void_p
    lib.hsddp_sim_create.argtypes = [H, C.c_int, C.c_int, C.c_int, C.POINTER(H)]
    lib.hsddp_sim_run.argtypes = [H, C.c_void_p, C.c_int]
    lib.hsddp_sim_get_rows.argtypes = [H, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.hsddp_sim_get_traj.argtypes = [H, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.hsddp_sim_device_final.argtypes = [H]
    lib.hsddp_sim_device_final.restype = C.c_void_p
    lib.hsddp_sim_get_kernel_time_ms.argtypes = [H, C.POINTER(C.c_float)]
    lib.hsddp_sim_destroy.argtypes = [H]
    lib.hsddp_sim_destroy.restype = None
    return lib


# include/hsddp_mc.h: disturbed runs of a simulation object (libhsddp_hip.so only)
MC_EXPORTS = ["hsddp_mc_run", "hsddp_mc_get_extra"]


class McDist(C.Structure):
    """hsddp_mc_dist_t"""
    _fields_ = [("seed", C.c_ulonglong), ("sigma_u", C.c_double), ("sigma_q", C.c_double), ("sigma_v", C.c_double), ("u_max", C.c_double),
                ("fall_height", C.c_double), ("kick_step", C.c_int), ("first_problem", C.c_int)]


class McExtra(C.Structure):
    """hsddp_mc_extra_t"""
    _fields_ = [("first_fall", C.c_int), ("n_sat", C.c_int)]


MC_EXTRA_DTYPE = np.dtype([("first_fall", "<i4"), ("n_sat", "<i4")])


def bind_mc(lib):
    """Attach argtypes/restypes for the entry points of include/hsddp_mc.h (and of hsddp_sim.h, which they work on).  Raises if the library lacks any."""
    missing = [s for s in MC_EXPORTS if not hasattr(lib, s)]
    if missing:
        raise RuntimeError(f"library lacks the disturbed-simulation entry points {missing}")
    bind_sim(lib)
    H = C.c_void_p
    lib.hsddp_mc_run.argtypes = [H, C.c_void_p, C.c_int, C.POINTER(McDist), C.c_void_p, C.c_int]
    lib.hsddp_mc_get_extra.argtypes = [H, C.c_int, C.c_int, C.c_void_p]
    return lib


# include/hsddp_grf.h: ground-reaction-force records of a simulation object (libhsddp_hip.so only)
GRF_EXPORTS = ["hsddp_grf_set", "hsddp_grf_get"]


class GrfRow(C.Structure):
    """hsddp_grf_row_t"""
    _fields_ = [("min_fz", C.c_double), ("min_cone", C.c_double), ("max_fz", C.c_double), ("first_slip", C.c_int), ("n_slip", C.c_int)]


GRF_ROW_DTYPE = np.dtype([("min_fz", "<f8"), ("min_cone", "<f8"), ("max_fz", "<f8"), ("first_slip", "<i4"), ("n_slip", "<i4")])


def bind_grf(lib):
    """Attach argtypes/restypes for the entry points of include/hsddp_grf.h (and of hsddp_sim.h, which they work on).  Raises if the library lacks any."""
    missing = [s for s in GRF_EXPORTS if not hasattr(lib, s)]
    if missing:
        raise RuntimeError(f"library lacks the contact-force record entry points {missing}")
    bind_sim(lib)
    H = C.c_void_p
    lib.hsddp_grf_set.argtypes = [H, C.c_double, C.c_double]
    lib.hsddp_grf_get.argtypes = [H, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return lib


# include/hsddp_substep.h: sub-stepped integration of a simulation object (libhsddp_hip.so only).  A list and a binder of their own: the lists
# and binders above are those of their headers and stay as they are.
SUBSTEP_EXPORTS = ["hsddp_substep_set", "hsddp_substep_get"]
SUBSTEP_MAX = 64          # HSDDP_SUBSTEP_MAX


def bind_substep(lib):
    """Attach argtypes/restypes for the entry points of include/hsddp_substep.h (and of hsddp_sim.h, which they work on).  Raises if the library lacks any."""
    missing = [s for s in SUBSTEP_EXPORTS if not hasattr(lib, s)]
    if missing:
        raise RuntimeError(f"library lacks the substep entry points {missing}")
    bind_sim(lib)
    H = C.c_void_p
    lib.hsddp_substep_set.argtypes = [H, C.c_int]
    lib.hsddp_substep_get.argtypes = [H, IP]
    return lib


# include/hsddp_contact.h: unilateral ground contact in a simulation object (libhsddp_hip.so only).  A list and a binder of their own, as above.
CONTACT_EXPORTS = ["hsddp_contact_set", "hsddp_contact_get_params", "hsddp_contact_get"]
# hsddp_contact_row_t
CONTACT_ROW_DTYPE = np.dtype([("first_release", "<i4"), ("n_release", "<i4"), ("n_land", "<i4"), ("n_free", "<i4"), ("free_final", "<i4"), ("pad", "<i4"),
                              ("max_lift", "<f8")])


def bind_contact(lib):
    """Attach argtypes/restypes for the entry points of include/hsddp_contact.h (and of hsddp_sim.h, which they work on).  Raises if the library lacks any."""
    missing = [s for s in CONTACT_EXPORTS if not hasattr(lib, s)]
    if missing:
        raise RuntimeError(f"library lacks the contact entry points {missing}")
    bind_sim(lib)
    H = C.c_void_p
    lib.hsddp_contact_set.argtypes = [H, C.c_int, C.c_double, C.c_double]
    lib.hsddp_contact_get_params.argtypes = [H, IP, DP, DP]
    lib.hsddp_contact_get.argtypes = [H, C.c_int, C.c_int, C.c_void_p]
    return lib


# include/hsddp_terrain.h: terrain height maps and early swing-foot touchdown in a simulation object (libhsddp_hip.so only).  A list and a binder of
# their own, as above.
TERRAIN_EXPORTS = ["hsddp_terrain_set", "hsddp_terrain_get_params", "hsddp_terrain_get"]
# hsddp_terrain_row_t
TERRAIN_ROW_DTYPE = np.dtype([("first_early", "<i4"), ("n_early", "<i4"), ("n_early_release", "<i4"), ("n_held", "<i4"), ("early_final", "<i4"), ("pad", "<i4"),
                              ("max_pen", "<f8")])


class TerrainParams(C.Structure):
    """hsddp_terrain_t"""
    _fields_ = [("nx", C.c_int), ("ny", C.c_int), ("n_maps", C.c_int), ("early", C.c_int),
                ("x0", C.c_double), ("y0", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("w_td", C.c_double)]


def bind_terrain(lib):
    """Attach argtypes/restypes for the entry points of include/hsddp_terrain.h (and of hsddp_contact.h, which they extend).  Raises if the library lacks any."""
    missing = [s for s in TERRAIN_EXPORTS if not hasattr(lib, s)]
    if missing:
        raise RuntimeError(f"library lacks the terrain entry points {missing}")
    bind_contact(lib)
    H = C.c_void_p
    lib.hsddp_terrain_set.argtypes = [H, C.c_int, C.POINTER(TerrainParams), C.c_void_p, C.c_void_p]
    lib.hsddp_terrain_get_params.argtypes = [H, IP, C.POINTER(TerrainParams)]
    lib.hsddp_terrain_get.argtypes = [H, C.c_int, C.c_int, C.c_void_p]
    return lib


# include/hsddp_plant.h: per-sample plant-model mismatch in a simulation object (libhsddp_hip.so only).  A list and a binder of their own, as above.
PLANT_EXPORTS = ["hsddp_plant_set", "hsddp_plant_get_params", "hsddp_plant_get_table"]
PLANT_ROW = 46        # HSDDP_PLANT_ROW
PLANT_MAX = 65536     # HSDDP_PLANT_MAX
# the slices of a row: trunk mass | trunk CoM | trunk inertia about the CoM (xx, xy, xz, yy, yz, zz) | link_scale | tau_gain | damping
PLANT_SLICES = dict(mass=slice(0, 1), com=slice(1, 4), inertia=slice(4, 10), link_scale=slice(10, 22), tau_gain=slice(22, 34), damping=slice(34, 46))
PLANT_NOMINAL = (3.3, 0.0, 0.0, 0.0, 0.011253, 0.0, 0.0, 0.036203, 0.0, 0.042673) + (1.0,) * 24 + (0.0,) * 12


def bind_plant(lib):
    """Attach argtypes/restypes for the entry points of include/hsddp_plant.h (and of hsddp_terrain.h, which it includes).  Raises if the library lacks any."""
    missing = [s for s in PLANT_EXPORTS if not hasattr(lib, s)]
    if missing:
        raise RuntimeError(f"library lacks the plant entry points {missing}")
    bind_terrain(lib)
    H = C.c_void_p
    lib.hsddp_plant_set.argtypes = [H, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.hsddp_plant_get_params.argtypes = [H, IP, IP]
    lib.hsddp_plant_get_table.argtypes = [H, C.c_int, C.c_int, C.c_void_p]
    return lib


# include/hsddp_friction.h: Coulomb friction in a simulation object (libhsddp_hip.so only).  A list and a binder of their own, as above.
FRICTION_EXPORTS = ["hsddp_friction_set", "hsddp_friction_get_params", "hsddp_friction_get"]
# hsddp_friction_row_t
FRICTION_ROW_DTYPE = np.dtype([("first_slide", "<i4"), ("n_onset", "<i4"), ("n_slide", "<i4"), ("n_restick", "<i4"), ("slide_final", "<i4"), ("pad", "<i4"),
                               ("max_speed", "<f8"), ("distance", "<f8")])


class FrictionParams(C.Structure):
    """hsddp_friction_t"""
    _fields_ = [("v_stick", C.c_double), ("n_mu", C.c_int), ("pad", C.c_int)]


def bind_friction(lib):
    """Attach argtypes/restypes for the entry points of include/hsddp_friction.h (and of hsddp_terrain.h, which it includes).  Raises if the library lacks any."""
    missing = [s for s in FRICTION_EXPORTS if not hasattr(lib, s)]
    if missing:
        raise RuntimeError(f"library lacks the friction entry points {missing}")
    bind_terrain(lib)
    H = C.c_void_p
    lib.hsddp_friction_set.argtypes = [H, C.c_int, C.POINTER(FrictionParams), C.c_void_p, C.c_void_p]
    lib.hsddp_friction_get_params.argtypes = [H, IP, C.POINTER(FrictionParams)]
    lib.hsddp_friction_get.argtypes = [H, C.c_int, C.c_int, C.c_void_p]
    return lib


# include/hsddp_episode.h: batched closed-loop MPC episodes (libhsddp_hip.so only)
EPISODE_EXPORTS = ["hsddp_episode_create", "hsddp_episode_destroy", "hsddp_episode_reset", "hsddp_episode_advance", "hsddp_episode_get_rows",
                   "hsddp_episode_get_log", "hsddp_episode_device_state", "hsddp_episode_sim", "hsddp_episode_status"]


class EpisodeRow(C.Structure):
    """hsddp_episode_row_t"""
    _fields_ = [(n, C.c_double) for n in ("dev_q", "dev_v", "min_height", "max_torque", "min_fz", "min_cone", "max_fz", "track_cost")] + \
               [(n, C.c_int) for n in ("n_sat", "n_slip", "first_slip", "steps", "bad_solves", "end_reason", "end_step", "pad")]


EPISODE_ROW_DTYPE = np.dtype([(n, "<f8" if t is C.c_double else "<i4") for n, t in EpisodeRow._fields_])


def bind_episode(lib):
    """Attach argtypes/restypes for the entry points of include/hsddp_episode.h (and of the simulation headers it builds on).  Raises if the library
    lacks any."""
    missing = [s for s in EPISODE_EXPORTS if not hasattr(lib, s)]
    if missing:
        raise RuntimeError(f"library lacks the episode entry points {missing}")
    bind_mc(lib); bind_grf(lib)
    H = C.c_void_p
    lib.hsddp_episode_create.argtypes = [H, C.c_int, C.c_int, C.c_int, C.POINTER(H)]
    lib.hsddp_episode_destroy.argtypes = [H]
    lib.hsddp_episode_destroy.restype = None
    lib.hsddp_episode_reset.argtypes = [H, C.c_void_p, C.c_int]
    lib.hsddp_episode_advance.argtypes = [H, C.POINTER(McDist), C.c_void_p, C.c_int]
    lib.hsddp_episode_get_rows.argtypes = [H, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.hsddp_episode_get_log.argtypes = [H, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hsddp_episode_device_state.argtypes = [H]
    lib.hsddp_episode_device_state.restype = C.c_void_p
    lib.hsddp_episode_sim.argtypes = [H]
    lib.hsddp_episode_sim.restype = C.c_void_p
    lib.hsddp_episode_status.argtypes = [H, IP, IP, IP]
    return lib


# include/hsddp_latency.h: per-robot policy latency of the episodes (libhsddp_hip.so only)
LATENCY_EXPORTS = ["hsddp_latency_set", "hsddp_latency_get", "hsddp_latency_get_policy"]
LATENCY_ROW = 516      # doubles of a policy row: Xbar[k] | Xbar[k+1] | Ubar[k] | K[k]


class LatencyRow(C.Structure):
    """hsddp_latency_row_t"""
    _fields_ = [("delay", C.c_int), ("n_stale", C.c_int)]


LATENCY_ROW_DTYPE = np.dtype([(n, "<i4") for n, _ in LatencyRow._fields_])


def bind_latency(lib):
    """Attach argtypes/restypes for the entry points of include/hsddp_latency.h (and of hsddp_episode.h, which it builds on).  Raises if the library
    lacks any."""
    missing = [s for s in LATENCY_EXPORTS if not hasattr(lib, s)]
    if missing:
        raise RuntimeError(f"library lacks the latency entry points {missing}")
    bind_episode(lib)
    H = C.c_void_p
    lib.hsddp_latency_set.argtypes = [H, C.c_int, C.c_void_p, C.c_int]
    lib.hsddp_latency_get.argtypes = [H, C.c_int, C.c_int, C.c_void_p]
    lib.hsddp_latency_get_policy.argtypes = [H, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


# include/hsddp_touchdown.h: per-problem, per-foot touchdown heights and terrain-aware planning (libhsddp_hip.so only)
TOUCHDOWN_EXPORTS = ["hsddp_touchdown_set", "hsddp_touchdown_get", "hsddp_touchdown_clear", "hsddp_touchdown_from_terrain", "hsddp_episode_plan_terrain"]


def bind_touchdown(lib):
    """Attach argtypes/restypes for the entry points of include/hsddp_touchdown.h (and of hsddp_terrain.h and hsddp_episode.h, which it includes).
    Raises if the library lacks any."""
    missing = [s for s in TOUCHDOWN_EXPORTS if not hasattr(lib, s)]
    if missing:
        raise RuntimeError(f"library lacks the touchdown-height entry points {missing}")
    bind_terrain(lib); bind_episode(lib)
    H = C.c_void_p
    lib.hsddp_touchdown_set.argtypes = [H, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.hsddp_touchdown_get.argtypes = [H, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.hsddp_touchdown_clear.argtypes = [H, C.c_int]
    lib.hsddp_touchdown_from_terrain.argtypes = [H, C.POINTER(TerrainParams), C.c_void_p, C.c_void_p, C.c_double, C.c_int]
    lib.hsddp_episode_plan_terrain.argtypes = [H]
    for s in TOUCHDOWN_EXPORTS:
        getattr(lib, s).restype = C.c_int
    return lib


# include/hsddp_weights.h: per-problem cost-weight scales of whole-body phases (libhsddp_hip.so only)
WEIGHTS_EXPORTS = ["hsddp_weights_set", "hsddp_weights_get", "hsddp_weights_clear"]
WEIGHTS_ROW = 84      # sq[36] | sr[12] | sqf[36]


def bind_weights(lib):
    """Attach argtypes/restypes for the entry points of include/hsddp_weights.h.  Raises if the library lacks any."""
    missing = [s for s in WEIGHTS_EXPORTS if not hasattr(lib, s)]
    if missing:
        raise RuntimeError(f"library lacks the weight-scale entry points {missing}")
    H = C.c_void_p
    lib.hsddp_weights_set.argtypes = [H, C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.hsddp_weights_get.argtypes = [H, C.c_int, C.c_int, C.c_void_p]
    lib.hsddp_weights_clear.argtypes = [H]
    for s in WEIGHTS_EXPORTS:
        getattr(lib, s).restype = C.c_int
    return lib


def pack_weight_scales(sq, sr, sqf, nb=None):
    """Rows [nb, 84] = sq[36] | sr[12] | sqf[36] from three arrays, each one row ([36] / [12] / [36], broadcast to nb problems) or [nb, width]."""
    parts = [np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (sq, sr, sqf)]
    for a, w, n in zip(parts, (36, 12, 36), ("sq", "sr", "sqf")):
        if a.ndim != 2 or a.shape[1] != w:
            raise ValueError(f"{n}: shape {a.shape}, need [{w}] or [nb, {w}]")
    rows = max(a.shape[0] for a in parts) if nb is None else nb
    for a, n in zip(parts, ("sq", "sr", "sqf")):
        if a.shape[0] not in (1, rows):
            raise ValueError(f"{n}: {a.shape[0]} rows, need 1 or {rows}")
    return np.ascontiguousarray(np.concatenate([np.broadcast_to(a, (rows, a.shape[1])) for a in parts], axis=1))


# include/hsddp_limits.h: per-problem constraint limits of whole-body phases (libhsddp_hip.so only)
LIMITS_EXPORTS = ["hsddp_limits_set", "hsddp_limits_get", "hsddp_limits_clear", "hsddp_episode_plan_friction"]
LIMITS_ROW = 12      # torque_limit | joint_lb[3] | joint_ub[3] | h_min | mu | jointspeed_lb | jointspeed_ub | pad
LIMITS_FIELDS = {"torque_limit": (0, 1), "joint_lb": (1, 3), "joint_ub": (4, 3), "h_min": (7, 1), "mu": (8, 1), "jointspeed_lb": (9, 1), "jointspeed_ub": (10, 1)}


def bind_limits(lib):
    """Attach argtypes/restypes for the entry points of include/hsddp_limits.h.  Raises if the library lacks any."""
    missing = [s for s in LIMITS_EXPORTS if not hasattr(lib, s)]
    if missing:
        raise RuntimeError(f"library lacks the constraint-limit entry points {missing}")
    H = C.c_void_p
    lib.hsddp_limits_set.argtypes = [H, C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.hsddp_limits_get.argtypes = [H, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.hsddp_limits_clear.argtypes = [H]
    lib.hsddp_episode_plan_friction.argtypes = [H, C.c_double]
    for s in LIMITS_EXPORTS:
        getattr(lib, s).restype = C.c_int
    return lib


def pack_limits(nb=None, **fields):
    """Rows [nb, 12] from keyword arguments named like LIMITS_FIELDS: each None (NaN: the descriptor's value), a scalar (joint_lb / joint_ub: or one
    [3]) that is broadcast to nb problems, or a per-problem array [nb] ([nb, 3])."""
    unknown = set(fields) - set(LIMITS_FIELDS)
    if unknown:
        raise ValueError(f"unknown limits {sorted(unknown)}")
    vals, rows = {}, 1 if nb is None else nb
    for n, v in fields.items():
        if v is None:
            continue
        w = LIMITS_FIELDS[n][1]
        a = np.asarray(v, dtype=np.float64)
        if w == 1:
            if a.ndim > 1:
                raise ValueError(f"{n}: shape {a.shape}, need a scalar or [nb]")
            a = a.reshape(-1, 1)
        else:
            if a.ndim == 0:
                a = np.full((1, w), float(a))
            elif a.ndim == 1 and a.shape[0] == w:
                a = a.reshape(1, w)
            if a.ndim != 2 or a.shape[1] != w:
                raise ValueError(f"{n}: shape {a.shape}, need a scalar, [{w}] or [nb, {w}]")
        vals[n] = a
        if nb is None:
            rows = max(rows, a.shape[0])
    out = np.full((rows, LIMITS_ROW), np.nan)
    for n, a in vals.items():
        if a.shape[0] not in (1, rows):
            raise ValueError(f"{n}: {a.shape[0]} rows, need 1 or {rows}")
        o, w = LIMITS_FIELDS[n]
        out[:, o:o + w] = a
    return out


def _dp(a):
    return a.ctypes.data_as(DP)


class Solver:
    """Thin object wrapper over one hsddp handle of a bound library (either backend).

    Mirrors MultiPhaseDDP<T> (HSDDPSolver/header/MultiPhaseDDP.h:31-93): set_multiPhaseProblem happens in
    the constructor (descriptors instead of closures), then set_initial_condition / solve / get_*.
    """

    def __init__(self, lib, phases, batch=1, device=0, psi_dyn=3.1415, psi_kin=np.pi, precision=PREC_F64):
        self.lib = lib
        self.phases = phases            # list of dicts produced by problems.py (keeps numpy buffers alive)
        self.batch = batch
        n = len(phases)
        arr = (PhaseDesc * n)(*[p["desc"] for p in phases])
        mp = ModelParam(psi_dyn, psi_kin)
        self.h = C.c_void_p()
        rc = lib.hsddp_create_ex(C.byref(self.h), n, arr, C.byref(mp), batch, device, precision)
        if rc != 0:
            raise RuntimeError(f"hsddp_create_ex failed rc={rc}")
        self.precision = precision
        self.dims = [MODEL_DIMS[p["desc"].model] for p in phases]
        self.horizons = [p["desc"].horizon for p in phases]

    def close(self):
        if self.h:
            self.lib.hsddp_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed rc={rc}")

    def set_initial_condition(self, x0):
        x0 = np.ascontiguousarray(np.broadcast_to(np.asarray(x0, dtype=np.float64), (self.batch, self.dims[0][0])))
        self._ck(self.lib.hsddp_set_initial_condition(self.h, _dp(x0)), "set_initial_condition")

    def set_nominal(self, phase, Xbar, Ubar):
        Xbar = np.ascontiguousarray(Xbar, dtype=np.float64)
        Ubar = np.ascontiguousarray(Ubar, dtype=np.float64)
        per = 1 if Xbar.ndim == 3 else 0
        self._ck(self.lib.hsddp_set_nominal(self.h, phase, _dp(Xbar), _dp(Ubar), per), "set_nominal")

    def solve(self, opt, max_cputime_ms=1e6):
        self._ck(self.lib.hsddp_solve(self.h, C.byref(opt), C.c_float(max_cputime_ms)), "solve")

    def hybrid_rollout(self, eps, opt):
        self._ck(self.lib.hsddp_hybrid_rollout(self.h, eps, C.byref(opt)), "hybrid_rollout")

    def compute_cost(self, opt):
        self._ck(self.lib.hsddp_compute_cost(self.h, C.byref(opt)), "compute_cost")

    def LQ_approximation(self, opt):
        self._ck(self.lib.hsddp_LQ_approximation(self.h, C.byref(opt)), "LQ_approximation")

    def backward_sweep(self, reg):
        ok = np.zeros(self.batch, dtype=np.int32)
        self._ck(self.lib.hsddp_backward_sweep(self.h, reg, ok.ctypes.data_as(IP)), "backward_sweep")
        return ok

    def linear_rollout(self, eps, opt):
        self._ck(self.lib.hsddp_linear_rollout(self.h, eps, C.byref(opt)), "linear_rollout")

    def update_nominal_trajectory(self):
        self._ck(self.lib.hsddp_update_nominal_trajectory(self.h), "update_nominal_trajectory")

    def get_exp_cost_change(self):
        a = np.zeros(self.batch)
        b = np.zeros(self.batch)
        self._ck(self.lib.hsddp_get_exp_cost_change(self.h, _dp(a), _dp(b)), "get_exp_cost_change")
        return a, b

    def measure_dynamics_feasibility(self):
        a = np.zeros(self.batch)
        self._ck(self.lib.hsddp_measure_dynamics_feasibility(self.h, _dp(a)), "measure_dynamics_feasibility")
        return a

    def get_info(self):
        info = (Info * self.batch)()
        self._ck(self.lib.hsddp_get_info(self.h, info), "get_info")
        return info

    def info_arrays(self):
        info = self.get_info()
        return {k: np.array([getattr(i, k) for i in info]) for k, _ in Info._fields_}

    def field(self, phase, name, b0=0, nb=None):
        """Trajectory field as numpy [nb, count, ...] with matrices in (rows, cols) numpy order."""
        nb = self.batch - b0 if nb is None else nb
        cnt, el = C.c_int(), C.c_int()
        fid = FIELD_ID[name]
        self._ck(self.lib.hsddp_field_shape(self.h, phase, fid, C.byref(cnt), C.byref(el)), "field_shape")
        out = np.zeros((nb, cnt.value, el.value))
        if out.size:
            self._ck(self.lib.hsddp_get_field(self.h, phase, fid, b0, nb, _dp(out)), "get_field")
        n, m, p = self.dims[phase]
        shp = {"K": (m, n), "QUX": (m, n), "QUU": (m, m), "A": (n, n), "B": (n, m), "C": (p, n), "D": (p, m),
               "LXX": (n, n), "LUX": (m, n), "LUU": (m, m), "LYY": (p, p), "PHIXX": (n, n), "H0": (n, n)}.get(name)
        if shp is not None and out.size:
            out = out.reshape(nb, cnt.value, shp[1], shp[0]).transpose(0, 1, 3, 2)  # column-major -> numpy
        return out

    def solve_time_ms(self):
        return float(self.lib.hsddp_get_solve_time_ms(self.h))

    def warm_start_phase(self, dphase, src, sphase, shift):
        """Receding-horizon shift of one phase's nominal trajectory from another solver of the same backend (device to device)."""
        self._ck(self.lib.hsddp_warm_start_phase(self.h, dphase, src.h if src is not None else None, sphase, shift), "warm_start_phase")

    def reconfigure(self, phases, src_phase, shift):
        """Receding-horizon update in place (include/hsddp.h hsddp_reconfigure): new phase table, warm start + constraint parameters moved
        inside the handle, allocations reused."""
        n = len(phases)
        arr = (PhaseDesc * n)(*[p["desc"] for p in phases])
        sp = np.ascontiguousarray(src_phase, dtype=np.int32); sh = np.ascontiguousarray(shift, dtype=np.int32)
        assert sp.size == n and sh.size == n
        self._ck(self.lib.hsddp_reconfigure(self.h, n, arr, sp.ctypes.data_as(IP), sh.ctypes.data_as(IP)), "reconfigure")
        self.phases = phases
        self.dims = [MODEL_DIMS[p["desc"].model] for p in phases]
        self.horizons = [p["desc"].horizon for p in phases]

    def export_solver_info(self, problem=0):
        """solver_info_lcmt content (MHPCLocomotion.cpp:74-79) of one problem: dict + the eight raw 32-bit words."""
        w = np.zeros(8, dtype=np.uint32)
        self._ck(self.lib.hsddp_export_solver_info(self.h, problem, w.ctypes.data_as(C.c_void_p)), "export_solver_info")
        f = w[3:].view(np.float32)
        return {"n_iter": int(w[0].view(np.int32)), "n_ls_iter": int(w[1].view(np.int32)), "n_reg_iter": int(w[2].view(np.int32)), "solve_time": float(f[0]), "cost": float(f[1]),
                "dyn_feas": float(f[2]), "ineq_violation": float(f[3]), "eq_violation": float(f[4]), "raw": w}

    def set_control_knot(self, phase, k, u=None):
        """Trajectory::Ubar[k] (and U[k]) of one phase for the whole batch; u: [batch, m] or None for zeros (HKDProblem.cpp:220)."""
        if u is not None:
            u = np.ascontiguousarray(u, dtype=np.float64); assert u.shape == (self.batch, self.dims[phase][1])
        self._ck(self.lib.hsddp_set_control_knot(self.h, phase, k, u.ctypes.data_as(C.c_void_p) if u is not None else None), "set_control_knot")

    CMD_FIELDS = (("mpc_times", 1, "f"), ("torque", 12, "f"), ("eul", 3, "f"), ("pos", 3, "f"), ("qJ", 12, "f"), ("vWorld", 3, "f"),
                  ("eulrate", 3, "f"), ("qJd", 12, "f"), ("GRF", 12, "f"), ("feedback", 432, "f"), ("Qu", 12, "f"), ("Quu", 144, "f"),
                  ("Qux", 432, "f"), ("contacts", 4, "i"), ("statusTimes", 4, "f"))

    def export_mpc_command(self, problem=0, n_steps=8, mpc_time=0.0, dt=0.01, status_times=None):
        """MHPC_Command_lcmt content (MHPCLocomotion.cpp:190-287) of one problem as a dict of fp32/int32 arrays + the raw words."""
        words = np.zeros(1 + n_steps * 1089, dtype=np.uint32)
        st = None
        if status_times is not None:
            st = np.ascontiguousarray(status_times, dtype=np.float32); assert st.shape == (len(self.phases), 4)
        rc = self.lib.hsddp_export_mpc_command(self.h, problem, n_steps, float(mpc_time), float(dt),
                                               st.ctypes.data_as(C.POINTER(C.c_float)) if st is not None else None,
                                               words.ctypes.data_as(C.POINTER(C.c_uint)))
        if rc != 0:
            raise RuntimeError(f"hsddp_export_mpc_command failed: {rc}")
        out = {"N_mpcsteps": int(words[0].view(np.int32)), "raw": words}
        pos = 1
        for name, w, kind in self.CMD_FIELDS:
            seg = words[pos:pos + n_steps * w]; pos += n_steps * w
            out[name] = seg.view(np.float32 if kind == "f" else np.int32).reshape(n_steps, w).copy()
        return out

    def _hkd_args(self, nb, n_steps, status_times, pf):
        if not getattr(self, "_hkd_bound", False):
            bind_hkd(self.lib); self._hkd_bound = True      # raises on a library without include/hsddp_hkd.h (the CPU checker)
        st = None
        if status_times is not None:
            st = np.ascontiguousarray(status_times, dtype=np.float64); assert st.shape == (len(self.phases), 4)
        pfa = None
        if pf is not None:
            pfa = np.ascontiguousarray(np.broadcast_to(np.asarray(pf, dtype=np.float32), (nb, 12)))
        return st, pfa

    def export_hkd_command(self, problem=0, n_steps=9, mpc_time=0.0, dt=0.01, status_times=None, pf=None):
        """hkd_command_lcmt content (HKDMPC.cpp:207-297, include/hsddp_hkd.h) of one problem: a dict of decoded fields + the raw words.
        status_times: n_phases x 4 contact durations (HKDProblemData describe()["status_durations"]); pf: the current footholds (12)."""
        from . import hkd_command
        st, pfa = self._hkd_args(1, n_steps, status_times, pf)
        w = np.zeros(HKD_CMD_WORDS, dtype=np.uint32)
        rc = self.lib.hsddp_export_hkd_command(self.h, problem, n_steps, float(mpc_time), float(dt), st.ctypes.data if st is not None else None,
                                               pfa.ctypes.data if pfa is not None else None, w.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"hsddp_export_hkd_command failed: {rc}")
        return hkd_command.decode(w)

    def export_hkd_commands(self, b0=0, nb=None, n_steps=9, mpc_time=0.0, dt=0.01, status_times=None, pf=None, out=None):
        """Rows [nb, HKD_CMD_WORDS] (uint32) of problems b0 .. b0+nb-1 in one launch.  pf: [nb, 12] current footholds or None.  out: None (numpy
        result), a contiguous torch tensor of nb x HKD_CMD_WORDS 32-bit elements on the handle's device, or a raw device address of that many
        words (written in place and returned)."""
        nb = self.batch - b0 if nb is None else nb
        st, pfa = self._hkd_args(nb, n_steps, status_times, pf)
        args = (self.h, b0, nb, n_steps, float(mpc_time), float(dt), st.ctypes.data if st is not None else None, pfa.ctypes.data if pfa is not None else None)
        if out is None:
            rows = np.zeros((nb, HKD_CMD_WORDS), dtype=np.uint32)
            rc = self.lib.hsddp_export_hkd_commands(*args, rows.ctypes.data, 0)
        elif isinstance(out, int):
            rows = out
            rc = self.lib.hsddp_export_hkd_commands(*args, out, 1)
        else:
            assert out.device.type == "cuda" and out.is_contiguous() and out.element_size() == 4 and out.numel() == nb * HKD_CMD_WORDS
            rows = out
            rc = self.lib.hsddp_export_hkd_commands(*args, out.data_ptr(), 1)
        if rc != 0:
            raise RuntimeError(f"hsddp_export_hkd_commands failed: {rc}")
        return rows

    def _refs_bound(self):
        if not getattr(self, "_refs_ok", False):
            bind_refs(self.lib); self._refs_ok = True      # raises on a library without include/hsddp_refs.h (the CPU checker)

    def set_references(self, phase, b0=0, **arrays):
        """Per-problem tracking references of one phase (include/hsddp_refs.h) for problems b0 .. b0+nb-1.  Keywords: any of xr, ur, yr, foot_pos,
        foot_vel, body_pos (float64) and ref_contact (int32), each [nb, h+1, width]; fields left out keep their values.  All numpy arrays (copied
        through host staging) or all torch tensors on the handle's device (read in place)."""
        self._refs_bound()
        unknown = set(arrays) - set(REF_FIELDS)
        if unknown or not arrays:
            raise ValueError(f"set_references takes some of {REF_FIELDS}, got {sorted(arrays)}")
        if not 0 <= phase < len(self.phases):
            raise ValueError(f"phase {phase} out of range")
        w, h1 = ref_widths(self.phases[phase]["desc"].model), self.horizons[phase] + 1
        is_t = [type(a).__module__.startswith("torch") for a in arrays.values()]
        if any(is_t) and not all(is_t):
            raise ValueError("set_references: pass all numpy arrays or all torch tensors")
        nb = next(iter(arrays.values())).shape[0]
        refs, keep = Refs(), []
        for name, a in arrays.items():
            shape = (nb, h1, w[name])
            if is_t[0]:
                import torch
                want = torch.int32 if name == "ref_contact" else torch.float64
                if a.dtype != want or not a.is_contiguous() or a.device.type != "cuda" or tuple(a.shape) != shape:
                    raise ValueError(f"{name}: need a contiguous {want} tensor of shape {shape} on the handle's device, got {a.dtype} "
                                     f"{tuple(a.shape)} on {a.device} (contiguous={a.is_contiguous()})")
                setattr(refs, name, a.data_ptr())
            else:
                a = np.ascontiguousarray(a, dtype=np.int32 if name == "ref_contact" else np.float64)
                if a.shape != shape:
                    raise ValueError(f"{name}: shape {a.shape}, need {shape}")
                keep.append(a); setattr(refs, name, a.ctypes.data)
        self._ck(self.lib.hsddp_set_references(self.h, phase, b0, nb, C.byref(refs), 1 if is_t[0] else 0), "set_references")

    def get_references(self, phase, b0=0, nb=None):
        """The references problems b0 .. b0+nb-1 of a phase track: dict of [nb, h+1, width] arrays (yr only where p > 0)."""
        self._refs_bound()
        nb = self.batch - b0 if nb is None else nb
        w, h1 = ref_widths(self.phases[phase]["desc"].model), self.horizons[phase] + 1
        out = {n: np.zeros((nb, h1, w[n]), dtype=np.int32 if n == "ref_contact" else np.float64) for n in REF_FIELDS if w[n] > 0}
        self._ck(self.lib.hsddp_get_references(self.h, phase, b0, nb, *[out[n].ctypes.data if n in out else None for n in REF_FIELDS]),
                 "get_references")
        return out

    def set_touchdown_heights(self, phase, heights, b0=0):
        """Touchdown heights of problems b0 .. b0+nb-1 of a whole-body phase (include/hsddp_touchdown.h): heights [nb, 4] by leg FL FR HL HR - a
        numpy array (copied) or a float64 torch tensor on the handle's device (read in place).  The touchdown constraint of leg l of problem b
        becomes foot_z - heights[b, l]."""
        lib = bind_touchdown(self.lib)
        if type(heights).__module__.startswith("torch"):
            import torch
            if heights.dtype != torch.float64 or not heights.is_contiguous() or heights.device.type != "cuda" or heights.dim() != 2 or heights.shape[1] != 4:
                raise ValueError(f"heights: need a contiguous float64 tensor [nb, 4] on the handle's device, got {heights.dtype} {tuple(heights.shape)} on {heights.device}")
            self._ck(lib.hsddp_touchdown_set(self.h, phase, b0, heights.shape[0], heights.data_ptr(), 1), "touchdown_set")
            return
        a = np.ascontiguousarray(heights, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 4:
            raise ValueError(f"heights: shape {a.shape}, need [nb, 4]")
        self._ck(lib.hsddp_touchdown_set(self.h, phase, b0, a.shape[0], a.ctypes.data, 0), "touchdown_set")

    def touchdown(self, phase, b0=0, nb=None):
        """(heights, values) of problems b0 .. b0+nb-1 of a phase, each [nb, 4] by leg: the touchdown heights in use (the descriptor's ground_height
        when the phase has none of its own) and the constraint values the last writing rollout stored (NaN for legs without a touchdown)."""
        lib = bind_touchdown(self.lib)
        nb = self.batch - b0 if nb is None else nb
        hts, val = np.zeros((max(nb, 0), 4)), np.zeros((max(nb, 0), 4))
        self._ck(lib.hsddp_touchdown_get(self.h, phase, b0, nb, hts.ctypes.data, val.ctypes.data), "touchdown_get")
        return hts, val

    def clear_touchdown_heights(self, phase=-1):
        """Return a phase (-1: every phase) to the shared ground_height of its descriptor."""
        self._ck(bind_touchdown(self.lib).hsddp_touchdown_clear(self.h, phase), "touchdown_clear")

    def set_weight_scales(self, sq, sr, sqf, b0=0, nb=None):
        """Cost-weight scales of problems b0 .. b0+nb-1 (include/hsddp_weights.h): in every whole-body phase problem b plans with q * sq[b], r * sr[b]
        and qf * sqf[b].  sq [nb, 36], sr [nb, 12], sqf [nb, 36], or one row each that is broadcast to nb problems (default: b0 to the end of the
        batch when every argument is one row).  A float64 torch tensor [nb, 84] on the handle's device passed as sq (sr = sqf = None) is read in place.
        The scales stay across reconfigure; the foot costs, constraints, reduced-model phases and the episodes' track_cost are not scaled."""
        lib = bind_weights(self.lib)
        if type(sq).__module__.startswith("torch"):
            import torch
            if sr is not None or sqf is not None or sq.dtype != torch.float64 or not sq.is_contiguous() or sq.device.type != "cuda" or sq.dim() != 2 or sq.shape[1] != WEIGHTS_ROW:
                raise ValueError("set_weight_scales: a device source is one contiguous float64 tensor [nb, 84] on the handle's device (sr = sqf = None)")
            self._ck(lib.hsddp_weights_set(self.h, b0, sq.shape[0], sq.data_ptr(), 1), "weights_set")
            return
        one = all(np.asarray(a).ndim == 1 for a in (sq, sr, sqf))
        rows = pack_weight_scales(sq, sr, sqf, nb=(self.batch - b0) if (one and nb is None) else nb)
        self._ck(lib.hsddp_weights_set(self.h, b0, rows.shape[0], rows.ctypes.data, 0), "weights_set")

    def weight_scales(self, b0=0, nb=None):
        """(sq [nb, 36], sr [nb, 12], sqf [nb, 36]) in use for problems b0 .. b0+nb-1: ones when none are set."""
        nb = self.batch - b0 if nb is None else nb
        rows = np.zeros((max(nb, 0), WEIGHTS_ROW))
        self._ck(bind_weights(self.lib).hsddp_weights_get(self.h, b0, nb, rows.ctypes.data), "weights_get")
        return rows[:, :36].copy(), rows[:, 36:48].copy(), rows[:, 48:].copy()

    def clear_weight_scales(self):
        """Back to the descriptors' weights for every problem: the kernels of a handle that never had scales."""
        self._ck(bind_weights(self.lib).hsddp_weights_clear(self.h), "weights_clear")

    def set_limits(self, torque_limit=None, joint_lb=None, joint_ub=None, h_min=None, mu=None, jointspeed_lb=None, jointspeed_ub=None, b0=0, nb=None):
        """Constraint limits of problems b0 .. b0+nb-1 (include/hsddp_limits.h): in every whole-body phase problem b plans with its own torque limit,
        joint and joint-speed box, minimum height and friction coefficient - absolute values.  Each argument: None (the descriptors' value goes on
        being used), a scalar for all nb problems, or a per-problem array [nb] (joint_lb / joint_ub: [3] or [nb, 3]); nb defaults to the arrays'
        length, or b0 to the end of the batch when every argument is a scalar.  A float64 torch tensor [nb, 12] on the handle's device passed as
        torque_limit (everything else None) is read in place as whole rows, NaN where unset.  The limits stay across reconfigure."""
        lib = bind_limits(self.lib)
        rest = (joint_lb, joint_ub, h_min, mu, jointspeed_lb, jointspeed_ub)
        if type(torque_limit).__module__.startswith("torch"):
            import torch
            t = torque_limit
            if any(a is not None for a in rest) or t.dtype != torch.float64 or not t.is_contiguous() or t.device.type != "cuda" or t.dim() != 2 or t.shape[1] != LIMITS_ROW:
                raise ValueError("set_limits: a device source is one contiguous float64 tensor [nb, 12] on the handle's device (every other argument None)")
            self._ck(lib.hsddp_limits_set(self.h, b0, t.shape[0], t.data_ptr(), 1), "limits_set")
            return
        fields = dict(torque_limit=torque_limit, joint_lb=joint_lb, joint_ub=joint_ub, h_min=h_min, mu=mu, jointspeed_lb=jointspeed_lb, jointspeed_ub=jointspeed_ub)
        rows = pack_limits(nb=nb, **fields)
        if nb is None and rows.shape[0] == 1:
            rows = np.ascontiguousarray(np.broadcast_to(rows, (self.batch - b0, LIMITS_ROW)))
        self._ck(lib.hsddp_limits_set(self.h, b0, rows.shape[0], rows.ctypes.data, 0), "limits_set")

    def limits(self, phase, b0=0, nb=None):
        """The limits in use in `phase` for problems b0 .. b0+nb-1, a dict of arrays named like set_limits' arguments ([nb], joint_lb / joint_ub
        [nb, 3]): the descriptor's values where nothing is set."""
        nb = self.batch - b0 if nb is None else nb
        rows = np.zeros((max(nb, 0), LIMITS_ROW))
        self._ck(bind_limits(self.lib).hsddp_limits_get(self.h, phase, b0, nb, rows.ctypes.data), "limits_get")
        return {n: (rows[:, o].copy() if w == 1 else rows[:, o:o + w].copy()) for n, (o, w) in LIMITS_FIELDS.items()}

    def clear_limits(self):
        """Back to the descriptors' limits for every problem: the kernels of a handle that never had limits."""
        self._ck(bind_limits(self.lib).hsddp_limits_clear(self.h), "limits_clear")

    def plan_terrain(self, terrain, map_of=None, z_ground=0.0):
        """Touchdown heights of every whole-body phase with a touchdown constraint from a sim.Terrain: z_ground + the grid's height at the phase's
        terminal reference foothold of each leg (hsddp_touchdown_from_terrain; problems.touchdown_heights_from_terrain is the definition).
        terrain.H and map_of (int [batch] or None: map 0; default terrain.map_of[:, 0]) are numpy arrays, or both torch tensors on the handle's
        device."""
        lib = bind_touchdown(self.lib)
        if map_of is None and terrain.map_of is not None:
            map_of = np.asarray(terrain.map_of).reshape(self.batch, -1)[:, 0]
        if type(terrain.H).__module__.startswith("torch"):
            import torch
            H = terrain.H if terrain.H.dim() == 3 else terrain.H[None]
            if H.dtype != torch.float64 or not H.is_contiguous() or H.device.type != "cuda":
                raise ValueError("plan_terrain: a device grid is a contiguous float64 tensor on the handle's device")
            if map_of is not None and (not type(map_of).__module__.startswith("torch") or map_of.dtype != torch.int32 or not map_of.is_contiguous()
                                       or map_of.device.type != "cuda" or tuple(map_of.shape) != (self.batch,)):
                raise ValueError("plan_terrain: with a device grid map_of is a contiguous int32 tensor [batch] on the handle's device")
            t = TerrainParams(H.shape[2], H.shape[1], H.shape[0], 1 if terrain.early else 0, terrain.x0, terrain.y0, terrain.cx, terrain.cy, terrain.w_td)
            self._ck(lib.hsddp_touchdown_from_terrain(self.h, C.byref(t), H.data_ptr(), None if map_of is None else map_of.data_ptr(), float(z_ground), 1), "touchdown_from_terrain")
            return
        H, t = terrain.grid(), terrain.to_c()
        mo = None
        if map_of is not None:
            mo = np.ascontiguousarray(map_of, dtype=np.int32)
            if mo.shape != (self.batch,):
                raise ValueError(f"plan_terrain: map_of has shape {mo.shape}, need ({self.batch},)")
        self._ck(lib.hsddp_touchdown_from_terrain(self.h, C.byref(t), H.ctypes.data, None if mo is None else mo.ctypes.data, float(z_ground), 0), "touchdown_from_terrain")

    def simulate(self, x0, n_steps, keep_traj=False, dist=None, kick=None, grf=None, substeps=1, contact=None, terrain=None, plant=None, friction=None):
        """Closed-loop rollouts of the current policy from the initial states x0 [batch, R, 36] (numpy, or a torch tensor on the handle's device)
        over the first n_steps whole-body control knots (include/hsddp_sim.h): dict with rows (structured array [batch, R] of dev_q, dev_v,
        min_height, max_torque, first_bad), x_final [batch, R, 36] and, with keep_traj, X [batch, R, n_steps + 1, 36] and U [batch, R, n_steps, 12].
        sim.Simulation keeps the device object across calls.  dist (sim.Disturbance) / kick [batch, R, 36]: a disturbed run (include/hsddp_mc.h),
        which also returns extra (structured array [batch, R] of first_fall, n_sat).  grf = (mu, fz_min): contact-force records
        (include/hsddp_grf.h), grf (structured array [batch, R] of min_fz, min_cone, max_fz, first_slip, n_slip) and, with keep_traj, Y
        [batch, R, n_steps, 12].  substeps = S > 1: every control knot is S forward-Euler steps of dt / S under the knot's torque
        (include/hsddp_substep.h); shapes and meanings stay, n_slip counts (foot, substep) pairs.  contact = (fz_rel, z_ground):
        unilateral ground contact (include/hsddp_contact.h), which also returns contact (structured array [batch, R] of first_release, n_release,
        n_land, n_free, free_final, max_lift).  terrain = sim.Terrain(...), with contact: height maps and early swing-foot touchdown
        (include/hsddp_terrain.h), which also returns terrain (structured array [batch, R] of first_early, n_early, n_early_release, n_held,
        early_final, max_pen).  plant = sim.Plant(...): a plant row per sample - trunk and link inertias, torque gain, joint friction
        (include/hsddp_plant.h); no new output, the existing ones show the effect."""
        from . import sim
        return sim.simulate(self, x0, n_steps, keep_traj, dist=dist, kick=kick, grf=grf, substeps=substeps, contact=contact, terrain=terrain, plant=plant, friction=friction)

    def episode(self, n_exec, max_ticks, keep_log=False):
        """An episode.Episode on this solver (include/hsddp_episode.h): batched closed-loop MPC ticks with the simulated state handed to the next
        solve on the device.  Close it before the solver."""
        from . import episode
        return episode.Episode(self, n_exec, max_ticks, keep_log)

    def get_history(self, problem=0, cap=4096):
        """MultiPhaseDDP::get_solver_info(cost, dyn_feas, eqn_feas, ineq_feas) (MultiPhaseDDP.h:85): the four float history buffers."""
        bufs = [np.zeros(cap, dtype=np.float32) for _ in range(4)]
        n = C.c_int()
        FP = C.POINTER(C.c_float)
        self._ck(self.lib.hsddp_get_history(self.h, problem, cap, *[b.ctypes.data_as(FP) for b in bufs], C.byref(n)), "get_history")
        m = min(n.value, cap)
        return {k: b[:m].copy() for k, b in zip(("cost", "dyn_feas", "eqn_feas", "ineq_feas"), bufs)}

    def kernel_units(self):
        out = {}
        for k in ("k_rollout", "k_lq", "k_sweep", "k_ls_probe"):
            v = C.c_longlong()
            if self.lib.hsddp_get_kernel_units(self.h, k.encode(), C.byref(v)) == 0:
                out[k] = int(v.value)
        return out

    def kernel_times(self, max_n=32):
        ms = np.zeros(max_n)
        cnt = np.zeros(max_n, dtype=np.int64)
        buf = C.create_string_buffer(2048)
        n = self.lib.hsddp_get_kernel_times(self.h, max_n, _dp(ms), cnt.ctypes.data_as(C.POINTER(C.c_longlong)), buf, 2048)
        names = [s.decode() for s in buf.raw.split(b"\0") if s][:n]
        return {names[i]: (float(ms[i]), int(cnt[i])) for i in range(min(n, len(names)))}
