"""The loop's controller as it ships -- fasta_python_amd/csrc/fh_controller.h, the header fh_iterate and the two device-side loops call -- built
for the host from tests/csrc/controller_shim.cpp and loaded with ctypes, so that the CPU tier checks the C++ itself and not a restatement.
TEST INFRASTRUCTURE: built once per session (`build`), with UndefinedBehaviorSanitizer; a missing compiler is an error, not a skip."""
import ctypes as C
import os
import subprocess

from fasta_python_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G_KIND = {hip.PROX_SHRINK: 1, hip.PROX_LINF: 2}         # FC_G_SUM, FC_G_MAX of fh_controller.h; every other prox kind: FC_G_NONE = 0
_pd = C.POINTER(C.c_double)


class Opts(C.Structure):                    # RunOpts of csrc/fh_loop.h
    _fields_ = [(k, C.c_int) for k in ("adaptive", "accelerate", "backtrack", "restart", "evaluate_objective", "stop_rule", "window",
                                       "max_backtracks")] + [("stepsize_shrink", C.c_double), ("tolerance", C.c_double)]


class State(C.Structure):                   # RunState of csrc/fh_loop.h
    _fields_ = [(k, C.c_double) for k in ("tau_next", "alpha1", "max_residual", "best_quality")] + \
               [("iteration", C.c_ulonglong), ("backtracks", C.c_ulonglong)] + \
               [(k, C.c_int) for k in ("stopped", "xi", "ti", "bi", "pc", "gc", "zc", "last_accel")] + \
               [("perm", C.c_int * 5), ("f_window", C.c_double * hip.RUN_WINDOW_MAX)]


class Decision(C.Structure):                # FcDecision of csrc/fh_controller.h
    _fields_ = [(k, C.c_bool) for k in ("better", "stop", "restarted")] + \
               [(k, C.c_double) for k in ("tau_next", "alpha0", "alpha1", "coef", "f1", "max_residual", "best_quality")]


_lib = None


def build(directory):
    """Compile the shim into `directory` with the host C++ compiler ($CXX, else c++) and load it; later calls return the loaded library."""
    global _lib
    if _lib is not None:
        return _lib
    out = os.path.join(str(directory), "controller_shim.so")
    cmd = [os.environ.get("CXX") or "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-fsanitize=undefined", "-fno-sanitize-recover=all",
           "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "fasta_python_amd", "csrc"),
           "-o", out, os.path.join(ROOT, "tests", "csrc", "controller_shim.cpp")]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(out)
    lib.fc_shim_sizes.restype, lib.fc_shim_sizes.argtypes = None, [C.POINTER(C.c_ulonglong)]
    lib.fc_shim_backtrack.restype = C.c_int
    lib.fc_shim_backtrack.argtypes = [C.POINTER(Opts), C.POINTER(State), C.c_int, _pd, C.c_double, C.c_int]
    lib.fc_shim_decide.restype = None
    lib.fc_shim_decide.argtypes = [C.POINTER(Opts), C.POINTER(State), C.c_int, C.c_int, C.c_double, _pd, C.c_double, C.c_int, _pd, C.POINTER(Decision)]
    lib.fc_shim_backtrack_mul.restype, lib.fc_shim_backtrack_mul.argtypes = C.c_int, lib.fc_shim_backtrack.argtypes
    lib.fc_shim_decide_mul.restype, lib.fc_shim_decide_mul.argtypes = None, lib.fc_shim_decide.argtypes
    lib.fc_shim_alpha_mul.restype, lib.fc_shim_alpha_mul.argtypes = None, [C.POINTER(Opts), C.c_double, C.c_double, _pd]
    lib.fc_shim_rotate.restype, lib.fc_shim_rotate.argtypes = None, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    sizes = (C.c_ulonglong * 3)()
    lib.fc_shim_sizes(sizes)
    assert list(sizes) == [C.sizeof(Opts), C.sizeof(State), C.sizeof(Decision)], "struct layouts of fh_loop.h / fh_controller.h moved"
    _lib = lib
    return lib


def get():
    if _lib is None:
        raise RuntimeError("tests.controller_shim.build(directory) has not run in this session")
    return _lib


def opts_of(o):
    """RunOpts from the solver's options (hip.RunOpts, or anything with the same attributes)"""
    return Opts(**{k: getattr(o, k) for k, _ in Opts._fields_})


def backtrack(o, st, lsq, scalars, tau, bt, mul=False):
    """the accept test: True = reject this attempt (mul: squares as the device forms them, FcSqMul)"""
    s = (C.c_double * len(scalars))(*scalars)
    fn = get().fc_shim_backtrack_mul if mul else get().fc_shim_backtrack
    return bool(fn(C.byref(o), C.byref(st), int(lsq), s, float(tau), int(bt)))


def decide(o, st, lsq, g_kind, mu, scalars, tau, bt, mul=False):
    """the decision after an accepted attempt: advances `st`, returns (Decision, history record)"""
    s = (C.c_double * len(scalars))(*scalars)
    rec, d = (C.c_double * hip.RUN_HIST)(), Decision()
    fn = get().fc_shim_decide_mul if mul else get().fc_shim_decide
    fn(C.byref(o), C.byref(st), int(lsq), int(g_kind), float(mu), s, float(tau), int(bt), rec, C.byref(d))
    return d, list(rec)


def alpha_mul(o, alpha1, rdot):
    """(alpha0, alpha1, coef) of fc_alpha with the device's square"""
    out = (C.c_double * 3)()
    get().fc_shim_alpha_mul(C.byref(o), float(alpha1), float(rdot), out)
    return tuple(out)


def rotate(accelerate, better, roles, perm):
    """fc_rotate on roles = [xi, ti, bi, pc, gc, zc, last_accel] and perm[5]: the new (roles, perm)"""
    r, p = (C.c_int * 7)(*roles), (C.c_int * 5)(*perm)
    get().fc_shim_rotate(int(accelerate), int(better), r, p)
    return list(r), list(p)
