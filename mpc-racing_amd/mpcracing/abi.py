"""ctypes mirror of ``include/mpcracing.h`` (the C ABI of libmpcracing.so)."""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.abspath(os.path.join(HERE, "..", "csrc"))
PRODUCT_LIB = os.path.join(CSRC, "libmpcracing.so")
HOST_TWIN_LIB = os.path.join(CSRC, "libmpcracing_host.so")
PROBE_LIB = os.path.join(CSRC, "libmpcracing_probe.so")  # TEST-ONLY (csrc/mr_probe.hip), not part of the C ABI

ABI_VERSION = 103  # MR_ABI_VERSION of include/mpcracing.h
MR_MODEL = {"kin": 0, "dyn": 1, "blend": 2, "blend_pacejka": 3, "dyn_pacejka": 4}
MR_PREC = {"fp64": 0, "fp32": 1}
MR_TYRE = {"linear": 0, "pacejka": 1}
MR_PLANT = {"kin": 0, "dyn": 1, "blend": 2}
MR_PLANT_NPAR = 22  # include/mpcracing.h
MR_PID_NGAIN, MR_PID_NMEM, MR_PID_NOUT, MR_PID_NLOG = 8, 4, 8, 14  # include/mpcracing.h
MR_GA_P_MAX, MR_GA_K_MAX, MR_GA_D_MAX = 64, 64, 16  # csrc/mr_ga.h
MR_MPCSEG_NMEM = 6  # include/mpcracing.h
MR_OPT = {"sgd": 0, "adam": 1, "adamw": 2}
STATUS = {0: "solved", 1: "acceptable", 2: "max_iter", 3: "failed", 4: "infeasible"}

_I32 = ctypes.c_int32
_D = ctypes.c_double
_U64 = ctypes.c_uint64
_PD = ctypes.POINTER(ctypes.c_double)
_PI32 = ctypes.POINTER(ctypes.c_int32)


class MRConfig(ctypes.Structure):
    _fields_ = [(n, _I32) for n in ("N", "model", "precision", "lane_bounds", "max_batch", "device",
                                    "max_iter", "acceptable_iter")] + \
               [(n, _D) for n in ("Ts", "tol", "acceptable_tol",
                                  "lambda_s", "alpha_L", "min_steer", "max_steer", "min_throttle",
                                  "max_steer_delta", "min_steer_delta", "max_throttle_delta",
                                  "min_throttle_delta", "q_v_max", "v_max", "min_s_delta",
                                  "m", "Iz", "lf", "lr", "Cf", "Cr", "T_max", "r_wheel", "C_wheel", "R",
                                  "rho", "C_d", "A_f", "C_roll", "g", "max_steer_deg", "Vblendmin",
                                  "Vblendmax")] + [("dispatch_order", _I32)]


class MRInputs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("state0", "s0", "cx", "cy", "max_error", "runtime", "u_init",
                                               "order_hint")]


class MROutputs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("X", "U", "S", "eC", "eL", "status", "iters", "obj", "kkt",
                                               "trace")] + [("trace_instance", _I32), ("trace_cap", _I32),
                                                           ("lam_g", ctypes.c_void_p), ("timeline", ctypes.c_void_p),
                                                           ("constr_viol", ctypes.c_void_p)]


class MRWarm(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("x_init", "s_init", "use", "used")]


class MRTyrefitConfig(ctypes.Structure):
    _fields_ = [(n, _I32) for n in ("kind", "optimizer", "epochs", "patience")] + \
               [(n, _D) for n in ("factor", "m", "Iz", "lf", "lr", "T_max", "r_wheel", "C_wheel", "R", "rho", "C_d",
                                  "A_f", "C_roll", "g", "max_steer_deg")]


# every symbol declared in include/mpcracing.h (checked by tests/test_abi.py)
EXPORTS = ["mr_version", "mr_last_error", "mr_config_default", "mr_create", "mr_destroy", "mr_set_tyres",
           "mr_solve_batch", "mr_workspace_bytes_per_instance", "mr_eval_dynamics",
           "mr_track_create", "mr_track_destroy", "mr_track_eval", "mr_track_frame", "mr_track_error_sign",
           "mr_track_polyfit", "mr_track_polyfit_deg", "mr_track_lookup_error", "mr_track_projection", "mr_track_prep",
           "mr_spline_from_waypoints", "mr_track_lane_table", "mr_agent_sense", "mr_plant_step",
           "mr_tyrefit_config_default", "mr_tyre_loss_grad", "mr_tyre_fit", "mr_vehicle_step", "mr_tyre_rollout",
           "mr_plant_params_default", "mr_plant_step_params", "mr_plant_rollout",
           "mr_pid_gains_default", "mr_pid_control", "mr_pid_drive", "mr_pid_segment_times", "mr_ga_random",
           "mr_ga_breed", "mr_solve_batch_horizons", "mr_solve_batch_warm", "mr_warm_shift",
           "mr_mpcseg_runtime", "mr_mpcseg_inputs", "mr_mpcseg_apply"]


def _bind_product(lib):
    lib.mr_version.restype = ctypes.c_int
    lib.mr_last_error.restype = ctypes.c_char_p
    lib.mr_config_default.argtypes = [ctypes.POINTER(MRConfig)]
    lib.mr_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(MRConfig)]
    lib.mr_destroy.argtypes = [ctypes.c_void_p]
    lib.mr_set_tyres.argtypes = [ctypes.c_void_p, _PD, _D, _PD, _D]
    lib.mr_solve_batch.argtypes = [ctypes.c_void_p, _I32, ctypes.POINTER(MRInputs), ctypes.POINTER(MROutputs),
                                   ctypes.c_void_p]
    lib.mr_solve_batch_horizons.argtypes = [ctypes.c_void_p, _I32, ctypes.POINTER(MRInputs),
                                            ctypes.POINTER(MROutputs), ctypes.c_void_p, ctypes.c_void_p]
    lib.mr_solve_batch_warm.argtypes = [ctypes.c_void_p, _I32, ctypes.POINTER(MRInputs), ctypes.POINTER(MROutputs),
                                        ctypes.c_void_p, ctypes.POINTER(MRWarm), ctypes.c_void_p]
    lib.mr_warm_shift.argtypes = [ctypes.c_void_p, _I32] + [ctypes.c_void_p] * 13
    lib.mr_eval_dynamics.argtypes = [ctypes.c_void_p, _I32] + [ctypes.c_void_p] * 7
    lib.mr_workspace_bytes_per_instance.argtypes = [ctypes.c_void_p]
    lib.mr_workspace_bytes_per_instance.restype = ctypes.c_int64
    V = ctypes.c_void_p
    lib.mr_track_create.argtypes = [ctypes.POINTER(V), _I32, _PD, _I32, _PD, _PD, _I32, _D, _PD, _PD, _I32]
    lib.mr_track_destroy.argtypes = [V]
    lib.mr_track_eval.argtypes = [V, _I32, V, V, V, V]
    lib.mr_track_frame.argtypes = [V, _I32, V, V, V, V, V, _D, V, V]
    lib.mr_track_error_sign.argtypes = [V, _I32, V, V, V, V, V]
    lib.mr_track_polyfit.argtypes = [V, _I32, V, V, V, V, V]
    lib.mr_track_polyfit_deg.argtypes = [V, _I32, V, V, _I32, V, V, V]
    lib.mr_track_lookup_error.argtypes = [V, _I32, V, V, V, V, V, V, V]
    lib.mr_track_projection.argtypes = [V, _I32, V, V, V, V, V, V, V, V]
    lib.mr_track_prep.argtypes = [V, _I32, V, V, V, V, _D, _D, _D, V, V, V, V, V, V]
    lib.mr_spline_from_waypoints.argtypes = [_PD, _PD, _I32, _I32, _PD, _PD, _PD, _PI32, _PD]
    lib.mr_track_lane_table.argtypes = [V, V, _I32, V, V, V, V]
    lib.mr_agent_sense.argtypes = [V, _I32, V, V, V, _D, _D, _D, V, V, V, V, V, V]
    lib.mr_plant_step.argtypes = [_I32, _I32, V, V, _D, V, V]
    TC = ctypes.POINTER(MRTyrefitConfig)
    lib.mr_tyrefit_config_default.argtypes = [TC]
    lib.mr_tyre_loss_grad.argtypes = [TC, _I32, V, _I32, V, V, V, V, V]
    lib.mr_tyre_fit.argtypes = [TC, _I32, V, _I32, V, _I32, V, V, V, V, ctypes.c_int64, V, V, V, V, V, V, V, V]
    lib.mr_vehicle_step.argtypes = [TC, _I32, V, V, _D, _I32, V, V, V, V]
    lib.mr_tyre_rollout.argtypes = [TC, _I32, V, _I32, V, _I32, _I32, V, V, V, V, V, V]
    lib.mr_plant_params_default.argtypes = [_PD]
    lib.mr_plant_step_params.argtypes = [_I32, _I32, V, V, _D, _I32, V, V, V]
    lib.mr_plant_rollout.argtypes = [_I32, _I32, V, _I32, V, _I32, _I32, V, V, V, V, V, V]
    lib.mr_pid_gains_default.argtypes = [_PD]
    lib.mr_pid_control.argtypes = [V, _I32, V, V, _I32, V, _D, V, V]
    lib.mr_pid_drive.argtypes = [V, _I32, _I32, _I32, _D, V, V, _I32, V, _I32, V, ctypes.c_uint32, V, V, V]
    lib.mr_pid_segment_times.argtypes = [V, _I32, _I32, _I32, _I32, _D, V, V, V, V, _I32, V, V, V, V]
    lib.mr_ga_random.argtypes = [_U64, _U64, _U64, _U64, ctypes.c_int64, V]
    lib.mr_ga_breed.argtypes = [_I32] * 5 + [V, _I32, _PI32] + [V] * 4 + [_D] * 3 + [_U64] * 3 + [V] * 5
    lib.mr_mpcseg_runtime.argtypes = [_I32, _I32, V, V, V, _D, V, V]
    lib.mr_mpcseg_inputs.argtypes = [_I32] * 4 + [_D, _D] + [V] * 8 + [_D, _D, _I32] + [V] * 7
    lib.mr_mpcseg_apply.argtypes = [_I32] * 4 + [_D, _D] + [V] * 6 + [_I32, V, V]
    return lib


_product = None


def load_product(path=None):
    """Load the gfx950 library. There is no fallback: a missing library is an error.
    MR_PRODUCT_LIB may name another build of the same source (developer A/B runs)."""
    global _product
    path = path or os.environ.get("MR_PRODUCT_LIB") or PRODUCT_LIB
    if _product is None:
        if not os.path.exists(path):
            raise RuntimeError(f"libmpcracing.so not built ({path}); run `python __graft_entry__.py build`")
        lib = _bind_product(ctypes.CDLL(path))
        if lib.mr_version() != ABI_VERSION:
            raise RuntimeError(f"{path}: ABI version {lib.mr_version()}, this binding expects {ABI_VERSION} "
                               "(rebuild with `python __graft_entry__.py build`)")
        _product = lib
    return _product


# operations of mrp_math_f32 (csrc/mr_probe.hip MathOp)
MRP_OP = {"sin": 0, "cos": 1, "tan": 2, "atan": 3, "atan2": 4, "sqrt": 5, "exp": 6, "log": 7, "rsqrt": 8, "div": 9,
          "rcp": 10}
_probe = None


def load_probe(path=None):
    """TEST-ONLY gfx950 probes of the device-only fp32 functions and the wave primitives (csrc/mr_probe.hip,
    the product's compiler flags).  Like the product: a missing library is an error, there is no fallback."""
    global _probe
    path = path or os.environ.get("MR_PROBE_LIB") or PROBE_LIB
    if _probe is None:
        if not os.path.exists(path):
            raise RuntimeError(f"libmpcracing_probe.so not built ({path}); run `python __graft_entry__.py build`")
        lib = ctypes.CDLL(path)
        V, I = ctypes.c_void_p, _I32
        lib.mrp_last_error.restype = ctypes.c_char_p
        lib.mrp_layout.argtypes = [_PI32]
        lib.mrp_layout.restype = None
        lib.mrp_math_f32.argtypes = [I, I, V, V, V, V]
        lib.mrp_eval_dynamics_f32.argtypes = [ctypes.POINTER(MRConfig), _PD, _D, _PD, _D, I, V, V, V, V, V, V, V]
        lib.mrp_chol3_f32.argtypes = [I, V, V, V, V, V, V, V]
        for t in ("f32", "f64", "i32"):
            getattr(lib, "mrp_wave_prims_" + t).argtypes = [I, V, V, V]
        for t in ("f32", "f64"):
            getattr(lib, "mrp_wave_mfma_" + t).argtypes = [I, V, V, V, V, V]
        _probe = lib
    return _probe


def load_host_twin(path=HOST_TWIN_LIB):
    """TEST-ONLY host build of the same solver source (never used by the product path)."""
    lib = ctypes.CDLL(path)
    lib.mrh_config_default.argtypes = [ctypes.POINTER(MRConfig)]
    lib.mrh_solve_batch.argtypes = [ctypes.POINTER(MRConfig), _PD, _D, _PD, _D, ctypes.c_int,
                                    ctypes.POINTER(MRInputs), ctypes.POINTER(MROutputs), ctypes.c_int]
    lib.mrh_solve_batch_scalar.argtypes = lib.mrh_solve_batch.argtypes
    lib.mrh_solve_batch_horizons.argtypes = lib.mrh_solve_batch.argtypes[:-1] + [_PI32, ctypes.c_int]  # host horizon [B]
    lib.mrh_solve_batch_scalar_horizons.argtypes = lib.mrh_solve_batch_horizons.argtypes
    # host horizon [B], then the guess (host arrays in an MRWarm) or NULL
    lib.mrh_solve_batch_warm.argtypes = lib.mrh_solve_batch.argtypes[:-1] + [_PI32, ctypes.POINTER(MRWarm), ctypes.c_int]
    lib.mrh_solve_batch_scalar_warm.argtypes = lib.mrh_solve_batch_warm.argtypes
    lib.mrh_warm_shift.argtypes = [ctypes.POINTER(MRConfig), _PD, _D, _PD, _D, ctypes.c_int] + [ctypes.c_void_p] * 12
    lib.mrh_eval_dynamics.argtypes = [ctypes.POINTER(MRConfig), _PD, _D, _PD, _D, _PD, _PD, _PD, _PD, _PD, _PD]
    lib.mrh_pacejka.argtypes = [_PD, _D, _D, ctypes.c_int, _PD]
    V, I = ctypes.c_void_p, ctypes.c_int
    lib.mrh_track_blob_size.argtypes = [I, I]
    lib.mrh_track_build.argtypes = [V, I, V, V, I, V, V, I, V]
    lib.mrh_track_eval.argtypes = [V, I, _D, I, I, V, V, V]
    lib.mrh_track_frame.argtypes = [V, I, _D, I, I, V, V, V, V, V, _D, V]
    lib.mrh_track_sign.argtypes = [V, I, _D, I, I, V, V, V, V]
    lib.mrh_track_polyfit.argtypes = [V, I, _D, I, I, V, V, V, V]
    lib.mrh_track_polyfit_deg.argtypes = [V, I, _D, I, I, V, V, I, V, V]
    lib.mrh_track_lookup.argtypes = [V, I, _D, I, I, V, V, V, V, V, V]
    lib.mrh_track_projection.argtypes = [V, I, _D, I, I, V, V, V, V, V, V, V]
    lib.mrh_spline_from_waypoints.argtypes = [_PD, _PD, I, I, _PD, _PD, _PD, _PI32, _PD]
    lib.mrh_lane_table.argtypes = [V, I, _D, I, V, I, _D, I, V, V, V]
    lib.mrh_agent_sense.argtypes = [V, I, _D, I, I, V, V, V, _D, _D, _D, V, V, V, V, V]
    lib.mrh_plant_step.argtypes = [I, I, V, V, _D, V]
    TC = ctypes.POINTER(MRTyrefitConfig)
    lib.mrh_tyrefit_config_default.argtypes = [TC]
    lib.mrh_tyre_loss_grad.argtypes = [TC, I, V, I, V, V, V, V]
    lib.mrh_tyre_fit.argtypes = [TC, I, V, I, V, I, V, V, V, V, ctypes.c_int64, V, V, V, V, V, V, V, I]
    lib.mrh_tyrefit_last_error.restype = ctypes.c_char_p
    lib.mrh_vehicle_step.argtypes = [TC, I, V, V, _D, I, V, V, V]
    lib.mrh_tyre_rollout.argtypes = [TC, I, V, I, V, I, I, V, V, V, V, V, I]
    lib.mrh_plant_params_default.argtypes = [_PD]
    lib.mrh_plant_step_params.argtypes = [I, I, V, V, _D, I, V, V]
    lib.mrh_plant_rollout.argtypes = [I, I, V, I, V, I, I, V, V, V, V, V, I]
    lib.mrh_pid_gains_default.argtypes = [_PD]
    lib.mrh_pid_control.argtypes = [V, I, _D, I, I, V, V, I, V, _D, V]
    lib.mrh_pid_drive.argtypes = [V, I, _D, I, I, I, I, _D, V, V, I, V, I, V, ctypes.c_uint32, V, V, I]
    lib.mrh_pid_segment_times.argtypes = [V, I, _D, I, I, I, I, I, _D, V, V, V, V, I, V, V, V, I]
    lib.mrh_ga_random.argtypes = [_U64, _U64, _U64, _U64, ctypes.c_int64, V]
    lib.mrh_ga_breed.argtypes = [I] * 5 + [V, I, _PI32] + [V] * 4 + [_D] * 3 + [_U64] * 3 + [V] * 4
    lib.mrh_mpcseg_runtime.argtypes = [I, I, V, V, V, _D, V]
    lib.mrh_mpcseg_inputs.argtypes = [I] * 4 + [_D, _D] + [V] * 8 + [_D, _D, I] + [V] * 6
    lib.mrh_mpcseg_apply.argtypes = [I] * 4 + [_D, _D] + [V] * 6 + [I, V]
    lib.mrh_pacejka_dparams.argtypes = [_PD, _D, _D, _PD, _PD]
    lib.mrh_probe_layout.argtypes = [_PI32]
    lib.mrh_probe_layout.restype = None
    for t in ("f32", "f64", "i32"):
        getattr(lib, "mrh_wave_prims_" + t).argtypes = [I, V, V]
    for t in ("f32", "f64"):
        getattr(lib, "mrh_wave_mfma_" + t).argtypes = [I, V, V, V, V]
    lib.mrh_eval_dynamics_f32.argtypes = [ctypes.POINTER(MRConfig), _PD, _D, _PD, _D, I, V, V, V, V, V, V]
    lib.mrh_chol3_f32.argtypes = [I, V, V, V, V, V, V]
    return lib
