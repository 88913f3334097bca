"""ctypes binding of libfasta_hip.so (C ABI: include/fasta_hip.h).

This is the only module that talks to the GPU, and nothing in it falls back: if the shared library is missing or
no MI355X is visible, `load_library()` / `HipContext()` raise.
"""

import collections
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# $FASTA_HIP_LIB names another build of the SAME C ABI (the test job of the experimental stencil forms points it at
# libfasta_hip_experimental.so, csrc/fh_experimental.h); it is never a fallback: a path that does not exist is an error
LIB_PATH = os.environ.get("FASTA_HIP_LIB") or os.path.join(_HERE, "libfasta_hip.so")

# enums mirrored from include/fasta_hip.h ---------------------------------------------------------
PROX_IDENTITY, PROX_SHRINK, PROX_NONNEG, PROX_LINF, PROX_L1BALL, PROX_TVBALL, PROX_BOX, PROX_GROUP, PROX_ROWBALL, PROX_ROWSPLIT = range(10)
PROX_NUCLEAR = 10                  # singular-value soft-threshold, identity operator only (fh_set_identity, csrc/fh_nuclear.h)
PROX_NUCBALL = 11                  # projection onto the nuclear-norm ball of radius mu, identity operator only (csrc/fh_nuclear.h: k_nuc_ball)
MAX_RHS = 16                       # columns of a matrix unknown (fh_set_rhs, fh_set_matrix_csr_rhs, fh_set_quadratic, fh_set_factorization)
(VEC_X0, VEC_G0, VEC_XHAT, VEC_XPROX, VEC_X1, VEC_G1, VEC_BEST, VEC_B, VEC_Z,
 VEC_T0, VEC_T1, VEC_T2, VEC_T3) = range(13)
(S_FSQ, S_DXG0, S_DX2, S_XH2, S_G02, S_GSUM, S_GMAX, S_RDOT, S_DXDG, S_DG2, S_FSQ_ADJ, S_XH2_ADJ,
 S_GSUM_ADJ, S_GMAX_ADJ, S_ALPHA) = range(15)
NSCALARS = 16
K_FWD, K_ADJ, K_AUX, K_COMM, K_FUSED, K_HOST_ISSUE, K_LEVEL = range(7)
(TUNE_FWD_ROWS, TUNE_FWD_GRID_CAP, TUNE_ADJ_SLAB_ROWS, TUNE_ADJ_CPT, TUNE_LD_PAD, TUNE_NT_LOADS,
 TUNE_TV_U, TUNE_TV_ROWS, TUNE_TV_NT, TUNE_FUSED_VARIANT, TUNE_TV_ZFREE, TUNE_TV_PIPE, TUNE_TV_XCD, TUNE_TV_LDS_PAD,
 TUNE_TV_RING, TUNE_TV_SLOTS, TUNE_FUSED_CUS, TUNE_RUN_MAX_N, TUNE_SEQ_POLL, TUNE_RUN_CHAIN, TUNE_ADJ_CYCLIC, TUNE_TV3_PLANES, TUNE_DCT_ROW_CAP) = range(23)
TUNE_NUC_BLOCK_ROWS = 23           # rows per block of the nuclear-norm prox's Jacobi steps: 0 (auto = 1), 1, 2, 4, 8; read when the prox is set
# keys 10, 13, 14, 15 (TUNE_TV_ZFREE / _LDS_PAD / _RING / _SLOTS) are NOT in include/fasta_hip.h: experimental forms of the stencil sweep,
# accepted only by libfasta_hip_experimental.so (csrc/fh_experimental.h); the shipped library answers FH_E_ARG
EXPERIMENTAL_KEYS = (TUNE_TV_ZFREE, TUNE_TV_LDS_PAD, TUNE_TV_RING, TUNE_TV_SLOTS)
TUNE_TEST_HOOKS = 0x7E57             # tests only (csrc/fh_experimental.h): 1 = a withheld team partial, 2 = the co-residency probe says no,
#                                      4 = the level search's last workgroup withholds its record, 8 = ... and its fall-back is off,
#                                      attempt << 8 = fh_run's last workgroup stays away from that attempt's first grid barrier
HOOK_WITHHOLD_PARTIAL, HOOK_PROBE_SAYS_NO, HOOK_LEVEL_WITHHOLD, HOOK_LEVEL_NO_FALLBACK = 1, 2, 4, 8
HOOK_RUN_ATTEMPT_SHIFT = 8
E_ARG, E_STATE, E_RCCL, E_TIMEOUT = 10001, 10002, 10003, 10004
E_NOCONV = 10005                   # FH_PROX_NUCLEAR: the Jacobi sweeps did not settle within 30 sweeps (xprox is NaN)
LAUNCH_SEPARATE, LAUNCH_ONEPASS_ALWAYS, LAUNCH_ONEPASS_SPECULATIVE, LAUNCH_PAIR = range(4)     # fh_run_opts.launch_mode (fh_iterate)
LAUNCH_MODES = {None: LAUNCH_SEPARATE, "always": LAUNCH_ONEPASS_ALWAYS, "speculative": LAUNCH_ONEPASS_SPECULATIVE, "pair": LAUNCH_PAIR}
RECOVERED_LEVEL_FALLBACK, RECOVERED_LEVEL_FAILED, RECOVERED_RUN_TIMEOUT = range(3)
UNIQUE_ID_BYTES = 128
DTYPE_F64, DTYPE_F32_STORAGE = 0, 1
CREATE_RCCL_SHELL = 0x100          # or'ed into the dtype of fh_create_ex: the multi-device (RCCL) form even for a single device
STORAGE = {"f64": DTYPE_F64, "f32": DTYPE_F32_STORAGE}

_u64, _i32, _dbl = C.c_uint64, C.c_int, C.c_double
_ctx = C.c_void_p
_pd = C.POINTER(C.c_double)

RUN_HIST, RUN_WINDOW_MAX = 8, 64
STOP_RULES = ("residual", "norm_residual", "ratio_residual", "hybrid_residual")      # fh_run_opts.stop_rule = index (fasta/stopping.py:6-51)


class RunOpts(C.Structure):                 # fh_run_opts
    _fields_ = [(k, _i32) for k in ("adaptive", "accelerate", "backtrack", "restart", "evaluate_objective", "stop_rule", "window",
                                    "max_backtracks")] + [("stepsize_shrink", _dbl), ("tolerance", _dbl), ("launch_mode", _i32), ("reserved", _i32)]


class RunState(C.Structure):                # fh_run_state
    _fields_ = [("tau_next", _dbl), ("alpha1", _dbl), ("max_residual", _dbl), ("best_quality", _dbl), ("iteration", _u64), ("backtracks", _u64),
                ("stopped", _i32), ("reserved", _i32), ("f_window", _dbl * RUN_WINDOW_MAX),
                ("spec_cooldown", _i32), ("onepass_backoff", _i32), ("onepass_off_until", C.c_int64),
                ("onepass_launches", _u64), ("pair_launches", _u64), ("onepass_timeouts", _u64)]



# every exported symbol with its signature; tests assert the .so exports exactly these ------------
GAP_NOUT = 8            # FH_GAP_NOUT: P, D, gap, f(z), Omega(x0), Omega°(g0), s, f(0)
SCREEN_NOUT = 4         # FH_SCREEN_NOUT: rho, features kept, gap_safe, mu
SCREEN_SHAPE_LEN = 6    # FH_SCREEN_SHAPE_LEN: rows per slab, slabs, columns per tile, tiles, workgroups of the norms kernel, kappa

SIGNATURES = {
    "fh_last_error": (C.c_char_p, []),
    "fh_device_count": (_i32, [C.POINTER(_i32)]),
    "fh_create": (_i32, [_i32, C.POINTER(_ctx)]),
    "fh_create_ex": (_i32, [_i32, C.POINTER(_i32), _i32, C.POINTER(_ctx)]),
    "fh_shard_count": (_i32, [_ctx, C.POINTER(_i32)]),
    "fh_shard": (_i32, [_ctx, _i32, C.POINTER(_ctx), C.POINTER(_u64), C.POINTER(_u64)]),
    "fh_last_scalars": (_i32, [_ctx, _pd]),
    "fh_destroy": (_i32, [_ctx]),
    "fh_sync": (_i32, [_ctx]),
    "fh_set_tuning": (_i32, [_ctx, _i32, C.c_longlong]),
    "fh_set_matrix": (_i32, [_ctx, _pd, _u64, _u64, _u64]),
    "fh_set_matrix_f32": (_i32, [_ctx, C.POINTER(C.c_float), _u64, _u64, _u64]),
    "fh_generate_matrix": (_i32, [_ctx, _u64, _u64, _u64, _u64, _dbl]),
    "fh_get_matrix_rows": (_i32, [_ctx, _u64, _u64, _pd]),
    "fh_set_matrix_csr": (_i32, [_ctx, _u64, _u64, _u64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _pd]),
    "fh_set_matrix_csr_rhs": (_i32, [_ctx, _u64, _u64, _u64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _pd, C.c_uint32]),
    "fh_nnz": (_i32, [_ctx, C.POINTER(_u64)]),
    "fh_sparse_lanes": (_i32, [_ctx, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "fh_set_stencil": (_i32, [_ctx, _u64, _u64]),
    "fh_set_stencil3d": (_i32, [_ctx, _u64, _u64, _u64]),
    "fh_tv3d_shape": (_i32, [_ctx, C.POINTER(C.c_uint32)]),
    "fh_tv3d_shape_for": (_i32, [_u64, _u64, _u64, _i32, _i32, C.POINTER(C.c_uint32)]),
    "fh_set_dct": (_i32, [_ctx, _u64, _pd]),
    "fh_dct_shape": (_i32, [_ctx, C.POINTER(C.c_uint32)]),
    "fh_dct_shape_for": (_i32, [_u64, _i32, _i32, C.POINTER(C.c_uint32)]),
    "fh_set_dct2": (_i32, [_ctx, _u64, _u64, _pd]),
    "fh_dct2_shape": (_i32, [_ctx, C.POINTER(C.c_uint32)]),
    "fh_dct2_shape_for": (_i32, [_u64, _u64, _i32, _i32, C.POINTER(C.c_uint32)]),
    "fh_set_conv2d": (_i32, [_ctx, _u64, _u64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _pd, _pd]),
    "fh_conv_shape": (_i32, [_ctx, C.POINTER(C.c_uint32)]),
    "fh_conv_shape_for": (_i32, [_u64, _u64, C.c_uint32, C.c_uint32, _i32, C.POINTER(C.c_uint32)]),
    "fh_shape": (_i32, [_ctx, C.POINTER(_u64), C.POINTER(_u64)]),
    "fh_set_identity": (_i32, [_ctx, _u64, _u64]),
    "fh_set_prox_nuclear": (_i32, [_ctx, _dbl, _i32]),
    "fh_nuclear_shape": (_i32, [_ctx, C.POINTER(_u64)]),
    "fh_nuclear_shape_for": (_i32, [_u64, _u64, _i32, _i32, C.POINTER(_u64)]),
    "fh_nuclear_info": (_i32, [_ctx, C.POINTER(_u64)]),
    "fh_set_quadratic": (_i32, [_ctx, _pd, _u64, _u64, _pd, C.c_uint32]),
    "fh_quad_shape": (_i32, [_ctx, C.POINTER(C.c_uint32)]),
    "fh_quad_shape_for": (_i32, [_u64, C.c_uint32, C.c_longlong, _i32, C.POINTER(C.c_uint32)]),
    "fh_set_factorization": (_i32, [_ctx, _pd, _u64, _u64, _u64, C.c_uint32]),
    "fh_set_prox_split": (_i32, [_ctx, _u64, _i32, C.c_double, C.c_double, C.c_double, _i32, C.c_double, C.c_double]),
    "fh_bilinear_shape": (_i32, [_ctx, C.POINTER(C.c_uint32)]),
    "fh_bilinear_shape_for": (_i32, [_u64, _u64, C.c_uint32, C.c_longlong, _i32, C.POINTER(C.c_uint32)]),
    "fh_set_rhs": (_i32, [_ctx, C.c_uint32]),
    "fh_rhs": (_i32, [_ctx, C.POINTER(C.c_uint32)]),
    "fh_multi_shape": (_i32, [_ctx, C.POINTER(C.c_uint32)]),
    "fh_multi_shape_for": (_i32, [_u64, _u64, C.c_uint32, _i32, C.c_longlong, _i32, C.POINTER(C.c_uint32)]),
    "fh_set_loss_lsq": (_i32, [_ctx, _pd, _u64]),
    "fh_set_loss_logistic": (_i32, [_ctx, _pd, _u64]),
    "fh_set_loss_weights": (_i32, [_ctx, _pd]),
    "fh_set_loss_softmax": (_i32, [_ctx, C.POINTER(C.c_int32), _u64]),
    "fh_set_prox": (_i32, [_ctx, _i32, _dbl, _dbl, _dbl]),
    "fh_level_shape_for": (_i32, [_u64, C.POINTER(C.c_uint32)]),
    "fh_set_vector": (_i32, [_ctx, _i32, _pd, _u64]),
    "fh_get_vector": (_i32, [_ctx, _i32, _pd, _u64]),
    "fh_init": (_i32, [_ctx, _pd]),
    "fh_setup": (_i32, [_ctx, _pd]),
    "fh_gradient_at": (_i32, [_ctx, _i32, _i32]),
    "fh_diff_norm": (_i32, [_ctx, _i32, _i32, _pd]),
    "fh_fwd": (_i32, [_ctx, _dbl, _pd]),
    "fh_adj": (_i32, [_ctx, _dbl, _i32, _dbl, _pd]),
    "fh_commit": (_i32, [_ctx, _i32]),
    "fh_dual_gap": (_i32, [_ctx, _pd]),
    "fh_column_norms": (_i32, [_ctx, _pd]),
    "fh_screen": (_i32, [_ctx, _pd, C.POINTER(C.c_uint8)]),
    "fh_gather_columns": (_i32, [_ctx, _ctx, C.POINTER(C.c_int32), _u64]),
    "fh_screen_shape_for": (_i32, [_u64, _u64, C.c_uint32, _i32, _i32, C.POINTER(C.c_uint32)]),
    "fh_standardize": (_i32, [_ctx, _i32, _i32, _pd, _pd]),
    "fh_abi_sizes": (_i32, [C.POINTER(_u64)]),
    "fh_run_supported": (_i32, [_ctx, C.POINTER(_i32)]),
    "fh_run": (_i32, [_ctx, _i32, C.POINTER(RunOpts), C.POINTER(RunState), _pd, C.POINTER(_i32)]),
    "fh_run_shape": (_i32, [_ctx, C.POINTER(C.c_uint32)]),
    "fh_run_shape_for": (_i32, [_u64, _u64, _i32, _i32, _i32, _i32, C.POINTER(C.c_uint32)]),
    "fh_iterate": (_i32, [_ctx, _i32, C.POINTER(RunOpts), C.POINTER(RunState), _pd, C.POINTER(_i32)]),
    "fh_recovered_count": (_i32, [_ctx, _i32, C.POINTER(_u64)]),
    "fh_fused_supported": (_i32, [_ctx, C.POINTER(_i32)]),
    "fh_fused_agree": (_i32, [_ctx, C.POINTER(_i32)]),
    "fh_coresident_probe": (_i32, [_ctx, _i32, C.POINTER(_i32)]),
    "fh_fused_shape": (_i32, [_u64, _i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32)]),
    "fh_fused_launch_shape": (_i32, [_ctx, C.POINTER(C.c_uint32)]),
    "fh_fused_launch_shape_for": (_i32, [_u64, _u64, _i32, _i32, _i32, _i32, _i32, C.POINTER(C.c_uint32)]),
    "fh_setup_shape": (_i32, [_ctx, C.POINTER(C.c_uint32)]),
    "fh_setup_shape_for": (_i32, [_u64, _u64, _i32, _i32, _i32, _i32, _i32, C.POINTER(C.c_uint32)]),
    "fh_fwd_adj": (_i32, [_ctx, _dbl, _pd]),
    "fh_step": (_i32, [_ctx, _dbl, _pd]),
    "fh_step_begin": (_i32, [_ctx, _dbl]),
    "fh_step_end": (_i32, [_ctx, _pd]),
    "fh_step_accel": (_i32, [_ctx, _dbl, _dbl, _i32, _pd]),
    "fh_apply": (_i32, [_ctx, _i32, _pd, _pd]),
    "fh_comm_unique_id": (_i32, [C.c_void_p]),
    "fh_comm_init": (_i32, [_ctx, _i32, _i32, C.c_void_p]),
    "fh_comm_count": (_i32, [_ctx, C.POINTER(_i32)]),
    "fh_comm_destroy": (_i32, [_ctx]),
    "fh_comm_library": (C.c_char_p, []),
    "fh_comm_version": (_i32, [C.POINTER(_i32)]),
    "fh_alloc_settle": (_i32, [_i32]),
    "fh_alloc_settle_waited": (_i32, [C.POINTER(_dbl)]),
    "fh_alloc_cache": (_i32, [_i32]),
    "fh_release_cached": (_i32, [_i32]),
    "fh_alloc_cache_hits": (_i32, [C.POINTER(_u64)]),
    "fh_comm_selftest": (_i32, [_ctx, _u64, _pd, C.POINTER(_i32)]),
    "fh_cu_count": (_i32, [_ctx, C.POINTER(_i32), C.POINTER(_i32)]),
    "fh_timing_enable": (_i32, [_ctx, _i32]),
    "fh_timing_get": (_i32, [_ctx, _i32, _pd, C.POINTER(_u64)]),
    "fh_timing_reset": (_i32, [_ctx]),
    "fh_timing_overlap": (_i32, [_ctx, _ctx, _i32, _pd, _pd, _pd]),
    "fh_stream_read_ms": (_i32, [_ctx, _i32, _pd, C.POINTER(_u64)]),
}

_lib = None


class HipError(RuntimeError):
    """Non-zero status from libfasta_hip.so (message = fh_last_error())."""


class HipTimeout(HipError):
    """A bounded in-launch hand-off ran out: the one-pass kernel's spins (scalar word 15 of the launch: the launch itself succeeded and
    left the solver state untouched, the caller may fall back to K-fwd / K-adj), or status FH_E_TIMEOUT -- the clipping-level search of the
    l-infinity prox / l1-ball projection found no level even alone (the step's outputs are NaN; a second failure on the two-launch path
    propagates out of fasta()).  The ONLY HipError a solver may recover from: every other non-zero status (device fault, RCCL error,
    bad state) must propagate.  `partial`: history records of the iterations an fh_iterate call completed before it failed."""
    partial = None


def load_library(path=None):
    """dlopen libfasta_hip.so and bind every entry point.  Raises if it is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise HipError(f"{path} is missing -- build it with `python __graft_entry__.py` "
                       "(hipcc --offload-arch=gfx950); this package has no CPU fallback")
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so lacks a declared symbol
        fn.restype, fn.argtypes = res, args
    # the structs that cross the boundary by pointer: this binding's layouts must be the library's (a stale .so next to a newer hip.py, or the
    # other way round, would otherwise read and write past each other's fields)
    sizes = (_u64 * 4)()
    _check(lib, lib.fh_abi_sizes(sizes))
    if tuple(sizes) != (C.sizeof(RunOpts), C.sizeof(RunState), RUN_HIST, RUN_WINDOW_MAX):
        raise HipError(f"{path}: fh_run_opts / fh_run_state / history layout {tuple(sizes)} does not match this binding's "
                       f"{(C.sizeof(RunOpts), C.sizeof(RunState), RUN_HIST, RUN_WINDOW_MAX)} -- rebuild the library (python __graft_entry__.py)")
    _lib = lib
    return lib


def _check(lib, status):
    if status != 0:
        raise (HipTimeout if status == E_TIMEOUT else HipError)(f"[{status}] " + lib.fh_last_error().decode(errors="replace"))


def _as_f64(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(_pd)


def device_count():
    lib = load_library()
    n = _i32(0)
    _check(lib, lib.fh_device_count(C.byref(n)))
    return n.value


def device_cus(device=0):
    """Compute units device `device` reports (a throw-away context asks the runtime)."""
    with HipContext(int(device)) as c:
        return c.cu_count()[0]


def fused_shape(n, storage="f64", variant=2, ncu=256):
    """((pieces per lane, posting distance, team members, x slice in LDS, row buffers), instantiated) of the one-pass kernel for
    rows of n columns; all zeros = no one-pass kernel for that width.  Host-only (works without a GPU)."""
    lib = load_library()
    shape = (_i32 * 5)()
    inst = _i32(0)
    _check(lib, lib.fh_fused_shape(int(n), STORAGE[storage], int(variant), int(ncu), shape, C.byref(inst)))
    return tuple(shape), bool(inst.value)


FUSED_LAUNCH_SHAPE_LEN = SETUP_SHAPE_LEN = 13
FusedLaunchShape = collections.namedtuple("FusedLaunchShape", "PPT PIPE TEAM XLDS NBO F32 wpc nteams rows_per_team grid variant ld2 nv2")
SetupShape = collections.namedtuple("SetupShape", "MPP PIPE TEAM threads NR F32 wpc nteams rows_per_team grid variant ld2 nv2")


def fused_launch_shape_for(m, n, storage="f64", variant_word=34, variant_auto=True, cus=256, min_rows=16):
    """FusedLaunchShape of a one-pass step launch (csrc/fh_fused.h) for an (m, n) dense matrix on `cus` CUs: the template key, workgroups per
    CU, teams, rows per team, grid, the scheduling word the kernel receives (variant_auto: nobody set FH_TUNE_FUSED_VARIANT, the host clears
    the cyclic bit below 128 rows per team), ld2, nv2 -- fh_fused_launch_shape_for, the rule the launcher itself calls.  Host-only."""
    lib = load_library()
    out = (C.c_uint32 * FUSED_LAUNCH_SHAPE_LEN)()
    _check(lib, lib.fh_fused_launch_shape_for(int(m), int(n), STORAGE[storage], int(variant_word), 1 if variant_auto else 0, int(cus), int(min_rows), out))
    return FusedLaunchShape(*(int(v) for v in out))


def setup_shape_for(m, n, storage="f64", variant_word=34, variant_auto=True, cus=256, min_rows=16):
    """SetupShape of fh_setup's one-read launch (csrc/fh_setup.h) for an (m, n) dense least-squares problem: fh_setup_shape_for, the rule the
    launcher itself calls (E_STATE where fh_setup takes the three passes).  Host-only."""
    lib = load_library()
    out = (C.c_uint32 * SETUP_SHAPE_LEN)()
    _check(lib, lib.fh_setup_shape_for(int(m), int(n), STORAGE[storage], int(variant_word), 1 if variant_auto else 0, int(cus), int(min_rows), out))
    return SetupShape(*(int(v) for v in out))


ScreenShape = collections.namedtuple("ScreenShape", "slab nslab tile_cols tiles grid kappa")


def screen_shape_for(m, n, L=0, storage="f64", ncu=256):
    """ScreenShape of fh_column_norms' launch on an (m, n) dense matrix and kappa, the longest addition chain of the certificate's sums for an
    unknown of L columns (0 = a vector): fh_screen_shape_for, the rule the launchers themselves call.  Host-only."""
    lib = load_library()
    out = (C.c_uint32 * SCREEN_SHAPE_LEN)()
    _check(lib, lib.fh_screen_shape_for(int(m), int(n), int(L), STORAGE[storage], int(ncu), out))
    return ScreenShape(*(int(v) for v in out))


MULTI_SHAPE_LEN = 14
MultiShape = collections.namedtuple("MultiShape", "LB CH R NT fwd_grid nrg ntrip npro slab_rows nslab last_slab_rows SB stages ncc")


def multi_shape(m, n, L, slab_rows=0, grid_cap=0, nt_loads=-1):
    """MultiShape of the multi-column dense launches for an (m, n) matrix and L columns under the tuning values FH_TUNE_ADJ_SLAB_ROWS,
    FH_TUNE_FWD_GRID_CAP (0 = auto) and FH_TUNE_NT_LOADS (-1 = auto): fh_multi_shape_for, the rule the launchers call.  Host-only."""
    lib = load_library()
    out = (C.c_uint32 * MULTI_SHAPE_LEN)()
    _check(lib, lib.fh_multi_shape_for(int(m), int(n), int(L), int(slab_rows), int(grid_cap), int(nt_loads), out))
    return MultiShape(*(int(v) for v in out))


QUAD_SHAPE_LEN = 12
QuadShape = collections.namedtuple("QuadShape", "LB CH R NT fwd_grid nrg ntrip last_live pass_max pass_min npro ngrad")


def quad_shape(n, L, grid_cap=0, nt_loads=-1):
    """QuadShape of the quadratic launches (csrc/fh_quad.h) for an (n, n) matrix and L columns under FH_TUNE_FWD_GRID_CAP (0 = auto) and
    FH_TUNE_NT_LOADS (-1 = auto): fh_quad_shape_for, the rule the launchers call.  Host-only."""
    lib = load_library()
    out = (C.c_uint32 * QUAD_SHAPE_LEN)()
    _check(lib, lib.fh_quad_shape_for(int(n), int(L), int(grid_cap), int(nt_loads), out))
    return QuadShape(*(int(v) for v in out))


BILINEAR_SHAPE_LEN = 17
BilinearShape = collections.namedtuple("BilinearShape", "LB NT tile_rows tile_cols row_panels col_tiles RB trips last_rows last_live_rows "
                                       "last_live_lanes grid tiles_max tiles_min nelem gx_bytes gy_bytes")


def bilinear_shape(m, n, K, grid_cap=0, nt_loads=-1):
    """BilinearShape of the bilinear launches (csrc/fh_bilinear.h) for an (m, n) matrix S and K columns of the factors under
    FH_TUNE_FWD_GRID_CAP (0 = auto) and FH_TUNE_NT_LOADS (-1 = auto): fh_bilinear_shape_for, the rule the launchers call.  Host-only."""
    lib = load_library()
    out = (C.c_uint32 * BILINEAR_SHAPE_LEN)()
    _check(lib, lib.fh_bilinear_shape_for(int(m), int(n), int(K), int(grid_cap), int(nt_loads), out))
    return BilinearShape(*(int(v) for v in out))


RUN_SHAPE_LEN = 15
RunShape = collections.namedtuple("RunShape", "PPT need XLDS BIG NB G rows_per_team empty_wgs last_rows share slices tps trips NT ld2")


def run_shape_for(m, n, cus=256, min_rows=16, run_max_n=0, nt_loads=-1):
    """RunShape of fh_run's persistent launch (csrc/fh_run.h) for an (m, n) dense float64 matrix on `cus` CUs (FH_TUNE_FUSED_CUS capped by the
    device's count) under the rows-per-team floor `min_rows` (the high half of FH_TUNE_FUSED_VARIANT; 16 by default, 0 = none),
    FH_TUNE_RUN_MAX_N and FH_TUNE_NT_LOADS (-1 = auto): fh_run_shape_for, the rule fh_run itself calls.  Host-only."""
    lib = load_library()
    out = (C.c_uint32 * RUN_SHAPE_LEN)()
    _check(lib, lib.fh_run_shape_for(int(m), int(n), int(cus), int(min_rows), int(run_max_n), int(nt_loads), out))
    return RunShape(*(int(v) for v in out))


TV3D_SHAPE_LEN = 8
Tv3dShape =collections.namedtuple("Tv3dShape", "tile_h tile_w planes tiles_h tiles_w chunks grid NT")


def tv3d_shape(D, H, W, planes=0, ncu=256):
    """Tv3dShape of the 3-D stencil launches for a (D, H, W) volume under FH_TUNE_TV3_PLANES = planes (0 = auto) on a device of ncu compute
    units: fh_tv3d_shape_for, the rule both launchers call.  Host-only."""
    lib = load_library()
    out = (C.c_uint32 * TV3D_SHAPE_LEN)()
    _check(lib, lib.fh_tv3d_shape_for(int(D), int(H), int(W), int(planes), int(ncu), out))
    return Tv3dShape(*(int(v) for v in out))


DCT_SHAPE_LEN = 40
DCT_ROW_CAP = 2048
DctShape = collections.namedtuple("DctShape", "levels N1 N2 cap radices1 radices2 lds1 rows1 grid1 lds2 rows2 grid2 threads lds_bytes tiles launches")


def _dct_shape(out):
    v = [int(k) for k in out]
    return DctShape(v[0], v[1], v[2], v[3], tuple(v[5:5 + v[4]]), tuple(v[18:18 + v[17]]), *v[30:40])


def dct_shape(N, row_cap=0, ncu=256):
    """DctShape of the DCT operator's launches for length N under FH_TUNE_DCT_ROW_CAP = row_cap (0 = 2048) on a device of ncu compute units:
    fh_dct_shape_for, the rule the launchers call.  Host-only.  HipError with the library's sentence for an N the device refuses."""
    lib = load_library()
    out = (C.c_uint32 * DCT_SHAPE_LEN)()
    _check(lib, lib.fh_dct_shape_for(int(N), int(row_cap), int(ncu), out))
    return _dct_shape(out)


def dct_refusal(N, row_cap=0, ncu=256):
    """None when the device serves length N under that row cap, else the library's sentence about N (N = 0, a prime factor above 5, no split
    within the cap).  Only those are refusals: a row cap out of range, a library that is missing or does not load, or any other status raises."""
    lib = load_library()
    out = (C.c_uint32 * DCT_SHAPE_LEN)()
    status = lib.fh_dct_shape_for(int(N), int(row_cap), int(ncu), out)
    if status == E_ARG and out[3] != 0:                  # (the cap was accepted -- the rule reports it -- so the sentence is about N)
        return f"[{status}] " + lib.fh_last_error().decode(errors="replace")
    _check(lib, status)
    return None


Dct2Shape = collections.namedtuple("Dct2Shape", "served H W cap radices_h radices_w lds_h rows_h grid_h lds_w rows_w grid_w threads lds_bytes tiles launches")


def _dct2_shape(out):
    v = [int(k) for k in out]
    return Dct2Shape(v[0], v[1], v[2], v[3], tuple(v[5:5 + v[4]]), tuple(v[18:18 + v[17]]), *v[30:40])


def dct2_shape(H, W, row_cap=0, ncu=256):
    """Dct2Shape of the 2-D DCT operator's launches for an (H, W) image under FH_TUNE_DCT_ROW_CAP = row_cap (0 = 2048) on a device of ncu compute
    units: fh_dct2_shape_for, the rule the launchers call.  Suffix _h: the W rows of length H, _w: the H rows of length W.  Host-only.  HipError
    with the library's sentence for a shape the device refuses."""
    lib = load_library()
    out = (C.c_uint32 * DCT_SHAPE_LEN)()
    _check(lib, lib.fh_dct2_shape_for(int(H), int(W), int(row_cap), int(ncu), out))
    return _dct2_shape(out)


def dct2_refusal(H, W, row_cap=0, ncu=256):
    """None when the device serves the shape (H, W) under that row cap, else the library's sentence about the shape (an empty axis, a prime factor
    above 5, an axis beyond the cap).  Only those are refusals: a row cap out of range, a library that is missing or does not load, or any other
    status raises."""
    lib = load_library()
    out = (C.c_uint32 * DCT_SHAPE_LEN)()
    status = lib.fh_dct2_shape_for(int(H), int(W), int(row_cap), int(ncu), out)
    if status == E_ARG and out[3] != 0:                  # (the cap was accepted -- the rule reports it -- so the sentence is about the shape)
        return f"[{status}] " + lib.fh_last_error().decode(errors="replace")
    _check(lib, status)
    return None


NUCLEAR_SHAPE_LEN = 13
NuclearShape = collections.namedtuple("NuclearShape", "transposed p q Bk P nb steps_per_sweep wgs_per_step column_chunk chunks_per_row ld bytes lds_bytes")
NuclearInfo = collections.namedtuple("NuclearInfo", "sweeps steps rotations rank")


def nuclear_shape(M, N, block_rows=0, ncu=256):
    """NuclearShape of the nuclear-norm prox's launches for an (M, N) unknown under FH_TUNE_NUC_BLOCK_ROWS = block_rows (0 = auto = 1):
    fh_nuclear_shape_for, the rule the launchers call.  Host-only.  HipError with the library's sentence for a shape the device refuses."""
    lib = load_library()
    out = (_u64 * NUCLEAR_SHAPE_LEN)()
    _check(lib, lib.fh_nuclear_shape_for(int(M), int(N), int(block_rows), int(ncu), out))
    return NuclearShape(*(int(v) for v in out))


LEVEL_SHAPE_LEN = 4
LevelShape = collections.namedtuple("LevelShape", "multi threads ept workgroups")


def level_shape_for(n):
    """LevelShape of the clipping-level search (csrc/fh_prox.h) for an unknown of n entries: several workgroups or one, threads per workgroup,
    entries a thread keeps in registers (0: re-read in every pass), workgroups -- fh_level_shape_for, the rule the launcher calls.  Host-only."""
    lib = load_library()
    out = (C.c_uint32 * LEVEL_SHAPE_LEN)()
    _check(lib, lib.fh_level_shape_for(int(n), out))
    return LevelShape(*(int(v) for v in out))


CONV_SHAPE_LEN = 8
CONV_MAX_TAPS = 16
ConvShape = collections.namedtuple("ConvShape", "tile_h tile_w tiles_h tiles_w grid run threads lds_bytes")


def conv_shape(H, W, kh, kw, ncu=256):
    """ConvShape of the convolution operator's launches for an (H, W) image and a (kh, kw) kernel on a device of ncu compute units:
    fh_conv_shape_for, the rule both launchers call.  Host-only.  HipError with the library's sentence for what the device refuses."""
    lib = load_library()
    out = (C.c_uint32 * CONV_SHAPE_LEN)()
    _check(lib, lib.fh_conv_shape_for(int(H), int(W), int(kh), int(kw), int(ncu), out))
    return ConvShape(*(int(v) for v in out))


def conv_refusal(H, W, kh, kw, ncu=256):
    """None when the device serves an (H, W) image under a (kh, kw) kernel, else the library's sentence (a zero dimension, more than 16 taps
    along an axis, H * W >= 2^31).  A library that is missing or does not load, or any other status, raises."""
    lib = load_library()
    out = (C.c_uint32 * CONV_SHAPE_LEN)()
    status = lib.fh_conv_shape_for(int(H), int(W), int(kh), int(kw), int(ncu), out)
    if status == E_ARG:
        return f"[{status}] " + lib.fh_last_error().decode(errors="replace")
    _check(lib, status)
    return None


def comm_library():
    """Path of the library the collectives come from ("" before the first communicator): the system's RCCL or $FASTA_RCCL_LIB."""
    return load_library().fh_comm_library().decode(errors="replace")


def comm_version():
    """RCCL's version code (e.g. 22203), or -1 before the first communicator / when the loaded library does not export it."""
    lib = load_library()
    v = _i32(-1)
    _check(lib, lib.fh_comm_version(C.byref(v)))
    return int(v.value)


def alloc_settle(enable=True):
    """Process-wide: wait with a large (>= 1 GiB) matrix allocation that no kept block serves until the device's earlier large frees have
    been cleared by the driver (default OFF since the one-pass kernel deals its rows cyclically and no longer depends on the mapping; see
    include/fasta_hip.h, profiles/r06_alloc_settle.txt and profiles/r06_placement.txt)."""
    lib = load_library()
    _check(lib, lib.fh_alloc_settle(1 if enable else 0))


def alloc_cache(enable=True):
    """Process-wide: keep the matrix block (>= 1 GiB) a context gives up -- one per device -- for the next matrix on that device that fits it
    (default on: no clearing, no new mapping, no waiting; include/fasta_hip.h).  False also returns the kept blocks to the driver."""
    lib = load_library()
    _check(lib, lib.fh_alloc_cache(1 if enable else 0))


def release_cached(device=-1):
    """Return the kept matrix block of `device` (-1: of every device) to the driver."""
    lib = load_library()
    _check(lib, lib.fh_release_cached(int(device)))


def alloc_cache_hits():
    lib = load_library()
    n = _u64(0)
    _check(lib, lib.fh_alloc_cache_hits(C.byref(n)))
    return int(n.value)


def alloc_settle_waited():
    """Seconds the library has spent in that wait so far (process-wide)."""
    lib = load_library()
    v = _dbl(0.0)
    _check(lib, lib.fh_alloc_settle_waited(C.byref(v)))
    return float(v.value)


def comm_unique_id():
    lib = load_library()
    buf = C.create_string_buffer(UNIQUE_ID_BYTES)
    _check(lib, lib.fh_comm_unique_id(buf))
    return buf.raw


class HipContext:
    """One context (stream, device-resident A, vectors, workspace) on one device -- or, with `devices=[...]`, one context over
    several row blocks of A driven from this process (fh_create_ex, ndev > 1).  Not thread-safe."""

    def __init__(self, device=0, storage="f64", devices=None, rccl_shell=False):
        """storage: "f64" (default) or "f32" -- the device copy of a dense A in float32 (opt-in throughput mode; vectors,
        accumulation and scalars stay float64).
        devices: list of device ids, one per row block (in-process row sharding): all different = one GPU each, sums over RCCL;
        all equal = every block on that one GPU, sums by an in-library kernel (what a one-GPU box can run)."""
        self.lib = load_library()
        self._h = _ctx()
        if storage not in STORAGE:
            raise ValueError('storage must be "f64" or "f32"')
        if devices is not None:
            devices = [int(d) for d in devices]
            if not devices:
                raise ValueError("devices must name at least one device")
            ids = (_i32 * len(devices))(*devices)
            flags = CREATE_RCCL_SHELL if rccl_shell else 0      # tests: the RCCL branch with one device / a repeated device id
            _check(self.lib, self.lib.fh_create_ex(len(devices), ids, STORAGE[storage] | flags, C.byref(self._h)))
            device = devices[0]
        elif storage == "f64":
            _check(self.lib, self.lib.fh_create(int(device), C.byref(self._h)))
        else:
            ids = (_i32 * 1)(int(device))
            _check(self.lib, self.lib.fh_create_ex(1, ids, STORAGE[storage], C.byref(self._h)))
        self.device = int(device)
        self.devices = devices
        self.storage = storage
        self._scal = np.zeros(NSCALARS)
        self._scal_p = self._scal.ctypes.data_as(_pd)
        self.sharded = False            # True once a multi-rank communicator is attached (comm_init)

    @classmethod
    def _borrowed(cls, lib, handle, device, storage):
        """A view of a shard of a multi-device context (fh_shard): same methods, never destroyed from here."""
        self = cls.__new__(cls)
        self.lib, self._h, self.device, self.devices, self.storage = lib, handle, device, None, storage
        self._scal = np.zeros(NSCALARS)
        self._scal_p = self._scal.ctypes.data_as(_pd)
        self.sharded = False
        self._view = True
        return self

    def shard_count(self):
        n = _i32(0)
        self._call("fh_shard_count", C.byref(n))
        return int(n.value)

    def shard(self, k):
        """(context view, row0, rows) of row block k; the view is valid while this context lives."""
        h, r0, rows = _ctx(), _u64(0), _u64(0)
        self._call("fh_shard", int(k), C.byref(h), C.byref(r0), C.byref(rows))
        dev = self.devices[k] if self.devices else self.device
        return HipContext._borrowed(self.lib, h, dev, self.storage), int(r0.value), int(rows.value)

    def last_scalars(self):
        """The FH_S_* block the latest call left on this context (fh_last_scalars): of a shard view, that shard's own copy."""
        out = np.empty(NSCALARS)
        self._call("fh_last_scalars", out.ctypes.data_as(_pd))
        return out

    # ---- lifetime ------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_view", False):           # a borrowed shard: owned by its multi-device context
            self._h = _ctx()
            return
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.fh_destroy(self._h)
            self._h = _ctx()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, name, *args):
        _check(self.lib, getattr(self.lib, name)(self._h, *args))

    # ---- operator / problem data -----------------------------------------------------------------
    def set_tuning(self, key, value):
        self._call("fh_set_tuning", int(key), int(value))

    def set_matrix(self, A):
        assert A.ndim == 2
        if self.storage == "f32" and A.dtype == np.float32:           # float32 data into float32 storage: no float64 detour
            A = np.ascontiguousarray(A)
            m, n = A.shape
            self._call("fh_set_matrix_f32", A.ctypes.data_as(C.POINTER(C.c_float)), m, n, n)
            return
        if A.dtype != np.float64 or not A.flags.c_contiguous:
            A = np.ascontiguousarray(A, dtype=np.float64)
        m, n = A.shape
        self._call("fh_set_matrix", A.ctypes.data_as(_pd), m, n, n)

    def set_matrix_csr(self, indptr, indices, data, shape, rhs=None):
        """Sparse operator from canonical CSR arrays (sorted, duplicates summed; fh_set_matrix_csr checks and names the first bad row).
        rhs=L: fh_set_matrix_csr_rhs, the operator and the multi-column form in one call (see set_matrix_csr_rhs)."""
        m, n = (int(k) for k in shape)
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.asarray(indices)
        if indices.dtype != np.int32:                  # narrowing must be exact: a wide column number may not wrap into the valid range
            if indices.dtype.kind not in "iu":
                raise TypeError("CSR indices must be integers")
            if indices.size and (int(indices.min()) < 0 or int(indices.max()) >= min(n, 2 ** 31)):
                raise ValueError(f"CSR column index out of range for {n} columns (32-bit column numbers)")
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        data = np.ascontiguousarray(data, dtype=np.float64)
        if indptr.size != m + 1 or indices.size != data.size:
            raise ValueError(f"CSR arrays do not fit shape {(m, n)}: indptr {indptr.size}, indices {indices.size}, data {data.size}")
        args = (m, n, int(data.size), indptr.ctypes.data_as(C.POINTER(C.c_int64)), indices.ctypes.data_as(C.POINTER(C.c_int32)), data.ctypes.data_as(_pd))
        if rhs is None:
            self._call("fh_set_matrix_csr", *args)
        else:
            self._call("fh_set_matrix_csr_rhs", *args, int(rhs))

    def set_matrix_csr_rhs(self, indptr, indices, data, shape, L):
        """Sparse operator for a matrix unknown (csrc/fh_spmulti.h): the unknown is (n, L), b and z are (m, L), L in 1..16; L = 0 is
        set_matrix_csr.  The lanes per row and the row ranges depend on L, so the column count is fixed here (set_rhs refuses a sparse context)."""
        self.set_matrix_csr(indptr, indices, data, shape, rhs=int(L))

    def nnz(self):
        """Stored entries of the sparse operator (0 for a dense matrix or the stencil)."""
        k = _u64(0)
        self._call("fh_nnz", C.byref(k))
        return int(k.value)

    def sparse_lanes(self, side):
        """(G, nwg, nlong) of one copy of the sparse operator (side 0: A by rows, 1: A^T by rows): the lanes per row -- which kernel
        instantiation a launch takes -- the workgroups that share the ordinary rows, and the long rows that get a workgroup each."""
        g, nwg, nlong = C.c_int(0), C.c_uint32(0), C.c_uint32(0)
        self._call("fh_sparse_lanes", int(side), C.byref(g), C.byref(nwg), C.byref(nlong))
        return int(g.value), int(nwg.value), int(nlong.value)

    def generate_matrix(self, m, n, row0, seed, coef):
        self._call("fh_generate_matrix", int(m), int(n), int(row0), int(seed), float(coef))

    def get_matrix_rows(self, row0, nrows):
        m, n = self.shape()
        out = np.empty((nrows, n))
        self._call("fh_get_matrix_rows", int(row0), int(nrows), out.ctypes.data_as(_pd))
        return out

    def set_stencil(self, H, W):
        self._call("fh_set_stencil", int(H), int(W))

    def set_stencil3d(self, D, H, W):
        """A = div : (D, H, W, 3) -> (D, H, W), A^H = grad, periodic (csrc/fh_tv3d.h)."""
        self._call("fh_set_stencil3d", int(D), int(H), int(W))

    def tv3d_shape(self):
        """Tv3dShape the next fwd / adj of this context launches with (fh_tv3d_shape).  E_STATE without a 3-D stencil operator."""
        out = (C.c_uint32 * TV3D_SHAPE_LEN)()
        self._call("fh_tv3d_shape", out)
        return Tv3dShape(*(int(v) for v in out))

    def set_quadratic(self, Q, c=None, L=1):
        """Operator and loss in one call (fh_set_quadratic): f(X) = .5 <X, Q X> + <c, X> with Q (n, n) float64 and EXACTLY symmetric, the unknown
        (n, L), L in 1..16 (a vector unknown is L = 1), c of the unknown's shape or None.  The context takes the multi-column layout."""
        Q = np.asarray(Q)
        assert Q.ndim == 2 and Q.shape[0] == Q.shape[1]
        if Q.dtype != np.float64 or not Q.flags.c_contiguous:
            Q = np.ascontiguousarray(Q, dtype=np.float64)
        n = Q.shape[0]
        cp = None
        if c is not None:
            c, cp = _as_f64(np.ravel(c))
            assert c.size == n * int(L)
        self._call("fh_set_quadratic", Q.ctypes.data_as(_pd), n, n, cp, int(L))

    def quad_shape(self):
        """QuadShape the next fwd / adj of this context launches with (fh_quad_shape).  E_STATE without a quadratic operator."""
        out = (C.c_uint32 * QUAD_SHAPE_LEN)()
        self._call("fh_quad_shape", out)
        return QuadShape(*(int(v) for v in out))

    def set_factorization(self, S, K):
        """Operator and loss in one call (fh_set_factorization): f(Z) = .5 ||S - X Y^T||_F^2 with S (m, n) float64 and the unknown
        Z = [X; Y] of shape (m + n, K), K in 1..16.  The context takes the multi-column layout."""
        S = np.asarray(S)
        assert S.ndim == 2
        if S.dtype != np.float64 or not S.flags.c_contiguous:
            S = np.ascontiguousarray(S, dtype=np.float64)
        self._call("fh_set_factorization", S.ctypes.data_as(_pd), S.shape[0], S.shape[1], S.shape[1], int(K))

    def set_prox_split(self, split, kind_top, mu_top=0.0, lo_top=0.0, hi_top=0.0, kind_bottom=PROX_IDENTITY, lo_bottom=0.0, hi_bottom=0.0):
        """FH_PROX_ROWSPLIT (fh_set_prox_split): rows [0, split) take kind_top, the other rows kind_bottom.  Bilinear operator only."""
        self._call("fh_set_prox_split", int(split), int(kind_top), float(mu_top), float(lo_top), float(hi_top),
                   int(kind_bottom), float(lo_bottom), float(hi_bottom))

    def bilinear_shape(self):
        """BilinearShape the next fwd / adj of this context launches with (fh_bilinear_shape).  E_STATE without a bilinear operator."""
        out = (C.c_uint32 * BILINEAR_SHAPE_LEN)()
        self._call("fh_bilinear_shape", out)
        return BilinearShape(*(int(v) for v in out))

    def set_dct(self, N, diag=None):
        """A = diag(d) * C, A^H = C^T * diag(d), C the orthonormal DCT-II of length N (csrc/fh_dct.h); diag=None: all ones."""
        if diag is None:
            self._call("fh_set_dct", int(N), None)
            return
        d, pd = _as_f64(diag)
        if d.shape != (int(N),):
            raise ValueError(f"diag has shape {d.shape}, the DCT operator of length {int(N)} takes ({int(N)},)")
        self._call("fh_set_dct", int(N), pd)

    def dct_shape(self):
        """DctShape the next fwd / adj of this context launches with (fh_dct_shape).  E_STATE without a DCT operator."""
        out = (C.c_uint32 * DCT_SHAPE_LEN)()
        self._call("fh_dct_shape", out)
        return _dct_shape(out)

    def set_dct2(self, H, W, diag=None):
        """A x = d * (C_H X C_W^T), A^H w = C_H^T (d * w) C_W on an (H, W) image, C_L the orthonormal DCT-II of length L (csrc/fh_dct2.h);
        diag=None: all ones."""
        if diag is None:
            self._call("fh_set_dct2", int(H), int(W), None)
            return
        d, pd = _as_f64(diag)
        if d.shape != (int(H), int(W)):
            raise ValueError(f"diag has shape {d.shape}, the DCT operator on an image of shape ({int(H)}, {int(W)}) takes ({int(H)}, {int(W)})")
        self._call("fh_set_dct2", int(H), int(W), pd)

    def dct2_shape(self):
        """Dct2Shape the next fwd / adj of this context launches with (fh_dct2_shape).  E_STATE without a 2-D DCT operator."""
        out = (C.c_uint32 * DCT_SHAPE_LEN)()
        self._call("fh_dct2_shape", out)
        return _dct2_shape(out)

    def set_identity(self, M, N):
        """The identity operator on an (M, N) matrix unknown with an elementwise loss (csrc/fh_nuclear.h): m = n = M * N; set the loss
        afterwards (set_loss_lsq / set_loss_logistic with M * N entries)."""
        self._call("fh_set_identity", int(M), int(N))

    def set_prox_nuclear(self, mu, objective=True):
        """FH_PROX_NUCLEAR on the identity operator; objective=False skips the values-only decompositions that g(x0) and g at an
        extrapolated x1 cost (S_GSUM of init() and S_GSUM_ADJ of an accelerated adj() are then NaN)."""
        self._call("fh_set_prox_nuclear", float(mu), 1 if objective else 0)

    def nuclear_shape(self):
        """NuclearShape the next thresholding of this context launches with (fh_nuclear_shape)."""
        out = (_u64 * NUCLEAR_SHAPE_LEN)()
        self._call("fh_nuclear_shape", out)
        return NuclearShape(*(int(v) for v in out))

    def nuclear_info(self):
        """NuclearInfo of the latest thresholding: sweeps, steps launched, rotations, rank kept (fh_nuclear_info)."""
        out = (_u64 * 4)()
        self._call("fh_nuclear_info", out)
        return NuclearInfo(*(int(v) for v in out))

    def set_conv2d(self, shape, kernel, origin=None, diag=None):
        """A x = d * (K conv x), A^H w = K corr (d * w), periodic, on an (H, W) image (csrc/fh_conv.h); origin=None: (kh // 2, kw // 2);
        diag=None: all ones."""
        H, W = (int(k) for k in shape)
        k, pk = _as_f64(kernel)
        if k.ndim != 2:
            raise ValueError(f"the kernel of a convolution operator is 2-D (got {k.ndim} dimensions)")
        kh, kw = k.shape
        oh, ow = (kh // 2, kw // 2) if origin is None else (int(origin[0]), int(origin[1]))
        if oh < 0 or ow < 0:
            raise ValueError(f"the origin ({oh}, {ow}) lies outside the {kh} x {kw} kernel")
        if diag is None:
            self._call("fh_set_conv2d", H, W, kh, kw, oh, ow, pk, None)
            return
        d, pd = _as_f64(diag)
        if d.shape != (H, W):
            raise ValueError(f"diag has shape {d.shape}, the convolution operator on an ({H}, {W}) image takes ({H}, {W})")
        self._call("fh_set_conv2d", H, W, kh, kw, oh, ow, pk, pd)

    def conv_shape(self):
        """ConvShape the next fwd / adj of this context launches with (fh_conv_shape).  E_STATE without a convolution operator."""
        out = (C.c_uint32 * CONV_SHAPE_LEN)()
        self._call("fh_conv_shape", out)
        return ConvShape(*(int(v) for v in out))

    def shape(self):
        m, n = _u64(0), _u64(0)
        self._call("fh_shape", C.byref(m), C.byref(n))
        return m.value, n.value

    def set_rhs(self, L):
        """Multi-column form: the unknown becomes an (n, L) matrix, b and z (m, L) matrices, L in 1..16 (0: back to the vector form).
        Plain single-device context with a dense float64 operator; vectors restart as zeros and the loss has to be set again."""
        self._call("fh_set_rhs", int(L))

    @property
    def rhs(self):
        """Columns of the matrix unknown (0 in the vector form)."""
        L = C.c_uint32(0)
        self._call("fh_rhs", C.byref(L))
        return int(L.value)

    def multi_shape(self):
        """MultiShape the next fwd / adj of this context launches with (fh_multi_shape): which instantiation, how many passes, trips, slabs,
        stages and column chunks.  E_STATE unless the context is in multi-column dense form."""
        out = (C.c_uint32 * MULTI_SHAPE_LEN)()
        self._call("fh_multi_shape", out)
        return MultiShape(*(int(v) for v in out))

    def set_loss_lsq(self, b):
        b, p = _as_f64(np.ravel(b))
        self._call("fh_set_loss_lsq", p, b.size)

    def set_loss_logistic(self, labels):
        labels, p = _as_f64(np.ravel(labels))
        self._call("fh_set_loss_logistic", p, labels.size)

    def set_loss_weights(self, w):
        """Observation weights of the elementwise loss on the identity operator (fh_set_loss_weights): f(X) = sum_j w_j * loss(x_j, b_j); an array of
        B's size, every entry finite and >= 0, set AFTER the loss; None removes them."""
        if w is None:
            self._call("fh_set_loss_weights", None)
            return
        w, p = _as_f64(np.ravel(w))
        if w.size != self.shape()[1]:
            raise ValueError(f"weights have {w.size} entries, the unknown has {self.shape()[1]}")
        self._call("fh_set_loss_weights", p)

    def set_loss_softmax(self, labels):
        """Softmax loss over the L columns of a matrix unknown (csrc/fh_softmax.h): integer class labels in [0, L), one per row of the operator.
        The context must be in multi-column form with L >= 2 (set_rhs on a dense operator, or a sparse operator set with rhs=L)."""
        raw = np.asarray(labels)
        if raw.dtype.kind not in "iu":
            raise ValueError(f"softmax labels must be integers (got dtype {raw.dtype})")
        if raw.size and (raw.min() < -2**31 or raw.max() >= 2**31):
            raise ValueError("softmax labels do not fit 32 bits")
        lab = np.ascontiguousarray(np.ravel(raw), dtype=np.int32)
        self._call("fh_set_loss_softmax", lab.ctypes.data_as(C.POINTER(C.c_int32)), lab.size)

    def set_prox(self, kind, mu=0.0, lo=0.0, hi=0.0):
        self._call("fh_set_prox", int(kind), float(mu), float(lo), float(hi))

    def set_vector(self, which, v):
        v, p = _as_f64(np.ravel(v))
        self._call("fh_set_vector", int(which), p, v.size)

    def get_vector(self, which, length):
        out = np.empty(int(length))
        self._call("fh_get_vector", int(which), out.ctypes.data_as(_pd), out.size)
        return out

    # ---- solver steps (scalars come back as a fresh copy of the FH_S_* block) ---------------------
    def init(self):
        self._call("fh_init", self._scal_p)
        return self._scal.copy()

    def setup(self):
        """fh_setup: the two Lipschitz probes (in VEC_T0 / VEC_T1) and init() in one call -- one read of a dense least-squares A where the
        one-read kernel has a shape.  Scalars as init(), plus S_DG2 = ||grad(T0) - grad(T1)||^2 and S_DX2 = ||T0 - T1||^2 (VEC_T2 / T3: scratch)."""
        self._call("fh_setup", self._scal_p)
        return self._scal.copy()

    def gradient_at(self, src, dst):
        self._call("fh_gradient_at", int(src), int(dst))

    def diff_norm(self, a, b):
        out = _dbl(0.0)
        self._call("fh_diff_norm", int(a), int(b), C.byref(out))
        return out.value

    def fwd(self, tau):
        self._call("fh_fwd", float(tau), self._scal_p)
        return self._scal.copy()

    def adj(self, tau, accel=False, coef=0.0):
        self._call("fh_adj", float(tau), 1 if accel else 0, float(coef), self._scal_p)
        return self._scal.copy()

    def fwd_adj(self, tau):
        """K-fwd + K-adj (no acceleration) under one synchronisation: both halves of the scalar block."""
        self._call("fh_fwd_adj", float(tau), self._scal_p)
        return self._scal.copy()

    def fused_supported(self):
        """0 = none; 1 = dense one-pass kernel, recommended; 3 = dense, available but not recommended (small matrix: n < 16384 and fewer than 8 Mi elements);
        2 = stencil (one sweep replaces both launches)."""
        yes = _i32(0)
        self._call("fh_fused_supported", C.byref(yes))
        return int(yes.value)

    def fused_agree(self):
        """The one-pass verdict of fused_supported() settled over the ranks of the attached communicator (any 0 wins, else any 3):
        a COLLECTIVE call when the context has a communicator -- every rank calls it at the same point; the local query otherwise."""
        yes = _i32(0)
        self._call("fh_fused_agree", C.byref(yes))
        return int(yes.value)

    def coresident_probe(self, workgroups):
        """True if `workgroups` whole-CU workgroups run side by side on this device (what the dense one-pass kernel needs of #CUs)."""
        ok = _i32(0)
        self._call("fh_coresident_probe", int(workgroups), C.byref(ok))
        return bool(ok.value)

    def fused_launch_shape(self):
        """FusedLaunchShape the next step() / step_accel() of this context launches with (fh_fused_launch_shape).  E_STATE where the one-pass
        kernel has no shape for the context."""
        out = (C.c_uint32 * FUSED_LAUNCH_SHAPE_LEN)()
        self._call("fh_fused_launch_shape", out)
        return FusedLaunchShape(*(int(v) for v in out))

    def setup_shape(self):
        """SetupShape the one-read launch of setup() takes on this context (fh_setup_shape).  E_STATE where setup() runs the three passes."""
        out = (C.c_uint32 * SETUP_SHAPE_LEN)()
        self._call("fh_setup_shape", out)
        return SetupShape(*(int(v) for v in out))

    def step(self, tau):
        """One-pass K-fwd + K-adj (no acceleration).  Raises HipTimeout if the bounded spins timed out."""
        self._call("fh_step", float(tau), self._scal_p)
        if self._scal[15] != 0.0:
            raise HipTimeout("fused one-pass kernel: team hand-off timed out (workgroups not co-resident?)")
        return self._scal.copy()

    def step_begin(self, tau):
        """Issue step(tau) without waiting for it: the host may drive other contexts until step_end()."""
        self._call("fh_step_begin", float(tau))

    def step_end(self):
        """Wait for the step issued by step_begin and return its scalars (HipTimeout as step())."""
        self._call("fh_step_end", self._scal_p)
        if self._scal[15] != 0.0:
            raise HipTimeout("fused one-pass kernel: team hand-off timed out (workgroups not co-resident?)")
        return self._scal.copy()

    def step_accel(self, tau, coef, restart):
        """One-pass K-fwd + K-adj with FISTA extrapolation: `coef` applies unless `restart` and this step's restart
        dot (returned in S_RDOT) exceeds 1e-30.  Dense operator."""
        self._call("fh_step_accel", float(tau), float(coef), 1 if restart else 0, self._scal_p)
        if self._scal[15] != 0.0:
            raise HipTimeout("fused one-pass kernel: team hand-off timed out (workgroups not co-resident?)")
        return self._scal.copy()

    def run_supported(self):
        """True if fh_run (the loop on the device, csrc/fh_run.h) has a kernel for this context's operator, loss and prox."""
        yes = _i32(0)
        self._call("fh_run_supported", C.byref(yes))
        return bool(yes.value)

    def run_shape(self):
        """RunShape the next run() of this context launches with (fh_run_shape): which instantiation, the grid, the row blocks and phase B's
        split.  E_STATE where the persistent launch has no kernel for the context."""
        out = (C.c_uint32 * RUN_SHAPE_LEN)()
        self._call("fh_run_shape", out)
        return RunShape(*(int(v) for v in out))

    def run(self, max_steps, opts, state):
        """Up to `max_steps` FBS iterations in one persistent launch.  `opts`: RunOpts, `state`: RunState (updated in place).
        Returns the (steps, RUN_HIST) history block: residual, norm_residual, stepsize, f, objective, backtracks, alpha0,
        became-best (+ 2: acceleration restarted).  A grid-barrier timeout of the launch (FH_E_TIMEOUT) is NOT raised: the block then holds
        the iterations completed before it, `state.stopped == 3`, and context and state are those of the last completed iteration --
        the caller carries on with `iterate()` / `step()`."""
        hist = np.empty((int(max_steps), RUN_HIST))
        done = _i32(0)
        status = self.lib.fh_run(self._h, int(max_steps), C.byref(opts), C.byref(state), hist.ctypes.data_as(_pd), C.byref(done))
        if status != 0 and not (status == E_TIMEOUT and state.stopped == 3):
            _check(self.lib, status)
        return hist[:done.value]

    def iterate(self, max_steps, opts, state):
        """Up to `max_steps` FBS iterations driven by the library's host-side loop (fh_iterate, csrc/fh_host_iterate.h): every operator,
        loss, prox and sharding form; same arguments and history block as run().  If an iteration fails, the exception carries the records
        of the iterations completed before it as `.partial` (state and context are those of the last completed iteration)."""
        hist = np.empty((int(max_steps), RUN_HIST))
        done = _i32(0)
        status = self.lib.fh_iterate(self._h, int(max_steps), C.byref(opts), C.byref(state), hist.ctypes.data_as(_pd), C.byref(done))
        if status != 0:
            try:
                _check(self.lib, status)
            except HipError as exc:
                exc.partial = hist[:done.value]
                raise
        return hist[:done.value]

    def recovered_count(self, what):
        """In-launch timeouts this context got over: RECOVERED_LEVEL_FALLBACK / RECOVERED_LEVEL_FAILED / RECOVERED_RUN_TIMEOUT."""
        n = _u64(0)
        self._call("fh_recovered_count", int(what), C.byref(n))
        return int(n.value)

    def commit(self, save_best=False):
        self._call("fh_commit", 1 if save_best else 0)

    def dual_gap(self):
        """fh_dual_gap: the duality-gap certificate of the committed iterate x0 from x0, g0, z = A x0 and b as they lie in device memory, with the
        mu and the prox kind the context holds -- a certificates.Certificate (primal, dual, gap, f, omega, dual_norm, scale, f0).  Changes nothing
        in the context; HipError with the library's sentence where the certificate is not served."""
        from .certificates import Certificate
        out = np.empty(GAP_NOUT)
        self._call("fh_dual_gap", out.ctypes.data_as(_pd))
        return Certificate(*(float(v) for v in out))

    def _columns(self):
        """n, or 0 where the context holds no operator (the call that follows then answers with the library's own sentence)."""
        try:
            return self.shape()[1]
        except HipError:
            return 0

    def column_norms(self):
        """fh_column_norms: the squared column norms of the dense or sparse operator, n doubles; the context keeps them until the operator goes
        (a second call launches nothing)."""
        out = np.empty(self._columns())
        self._call("fh_column_norms", out.ctypes.data_as(_pd) if out.size else None)
        return out

    def screen(self):
        """fh_screen: the gap-safe test at the committed iterate -- (keep: n booleans, report: rho, features kept, gap_safe, mu).  Changes nothing
        in the context but the workspace and the kept norms; HipError with the library's sentence where it is not served."""
        keep = np.empty(self._columns(), dtype=np.uint8)
        report = np.empty(SCREEN_NOUT)
        self._call("fh_screen", report.ctypes.data_as(_pd), keep.ctypes.data_as(C.POINTER(C.c_uint8)))
        return keep.astype(bool), report

    def gather_columns(self, src, idx):
        """fh_gather_columns: this context <- the columns idx (strictly increasing) of the dense matrix `src` holds, device to device; it comes out
        as after a dense setter, in vector form."""
        idx = np.ascontiguousarray(idx)
        if idx.dtype != np.int32:
            if idx.dtype.kind not in "iu" or (idx.size and (int(idx.min()) < -2 ** 31 or int(idx.max()) >= 2 ** 31)):
                raise TypeError("gather_columns: idx must be integers that fit 32 bits")
            idx = idx.astype(np.int32)
        _check(self.lib, self.lib.fh_gather_columns(self._h, src._h, idx.ctypes.data_as(C.POINTER(C.c_int32)), int(idx.size)))

    def standardize(self, center=True, scale=True):
        """fh_standardize: the dense or sparse matrix the context holds rewritten in place as (a - mean) / scale per column (csrc/fh_standardize.h;
        the host statement is preprocess.standardize) -- (means, scales), n doubles each.  A sparse operator is served with center=False.  The
        context comes out as after an operator setter: init() before the next certificate; prox kind, loss, b, x0 and the column count stay."""
        n = self._columns()
        means, scales = np.empty(n), np.empty(n)
        self._call("fh_standardize", 1 if center else 0, 1 if scale else 0,
                   means.ctypes.data_as(_pd) if n else None, scales.ctypes.data_as(_pd) if n else None)
        return means, scales

    def apply(self, v, adjoint=False):
        m, n = self.shape()
        L = self.rhs or 1                              # multi-column form: (n, L) / (m, L) row-major, flattened
        v, p = _as_f64(np.ravel(v))
        assert v.size == (m if adjoint else n) * L
        out = np.empty((n if adjoint else m) * L)
        self._call("fh_apply", 1 if adjoint else 0, p, out.ctypes.data_as(_pd))
        return out

    def sync(self):
        self._call("fh_sync")

    # ---- row sharding ---------------------------------------------------------------------------
    def comm_init(self, nranks, rank, unique_id):
        assert len(unique_id) == UNIQUE_ID_BYTES
        buf = C.create_string_buffer(bytes(unique_id), UNIQUE_ID_BYTES)
        self._call("fh_comm_init", int(nranks), int(rank), buf)
        self.sharded = True

    def comm_count(self):
        """Ranks in the attached communicator as RCCL reports them (1 without one)."""
        n = _i32(0)
        self._call("fh_comm_count", C.byref(n))
        return int(n.value)

    def comm_selftest(self, count):
        """(max |error|, blocks summed over) of this context's exchange on a known pattern of `count` doubles (collective with a communicator)."""
        err, nb = _dbl(-1.0), _i32(0)
        self._call("fh_comm_selftest", int(count), C.byref(err), C.byref(nb))
        return err.value, int(nb.value)

    def comm_destroy(self):
        self._call("fh_comm_destroy")
        self.sharded = False

    def cu_count(self):
        """(CUs the device reports, CUs the dense one-pass kernel is launched on -- TUNE_FUSED_CUS)."""
        dev, used = _i32(0), _i32(0)
        self._call("fh_cu_count", C.byref(dev), C.byref(used))
        return int(dev.value), int(used.value)

    # ---- measurement ----------------------------------------------------------------------------
    def timing_enable(self, on=True):
        self._call("fh_timing_enable", 1 if on else 0)

    def timing_reset(self):
        self._call("fh_timing_reset")

    def timing_get(self, kernel_id):
        ms, cnt = _dbl(0.0), _u64(0)
        self._call("fh_timing_get", int(kernel_id), C.byref(ms), C.byref(cnt))
        return ms.value, cnt.value

    def timing_overlap(self, other, kernel_id):
        """(ms this context's latest timed launch of `kernel_id` ran, ms `other`'s ran, ms BOTH were running; <= 0: one after the other)."""
        a, b, both = _dbl(0.0), _dbl(0.0), _dbl(0.0)
        _check(self.lib, self.lib.fh_timing_overlap(self._h, other._h, int(kernel_id), C.byref(a), C.byref(b), C.byref(both)))
        return a.value, b.value, both.value

    def stream_read_ms(self, reps=3):
        ms, nbytes = _dbl(0.0), _u64(0)
        self._call("fh_stream_read_ms", int(reps), C.byref(ms), C.byref(nbytes))
        return ms.value, nbytes.value
