"""What tests/test_refusals_cpu.py, tests/test_gpu_refusals.py and scripts/make_refusal_golden.py share about what a context ACCEPTS: the list of
calls to the C ABI whose answer -- the status and the text of fh_last_error, 0 and "" on success -- is pinned in
tests/golden/refusals/c_abi.json.  The host text of the library decides every one of them: which prox kinds, losses and column counts an
operator form serves, which context states an operator setter refuses, and what a change of operator keeps.  The fixture is taken once, on
the GPU, and compared with `==`; it must be taken again (scripts/make_refusal_golden.py) whenever a kind, a setter or a sentence is added.

A case is (id, state, calls).  `state` names how the context is made (STATES); `calls` is a tuple of (entry point, arguments) in order.  Every
call of a case is recorded.  Arguments are plain Python values: numbers, None (a NULL pointer), ("f64" | "i64" | "i32" | "f32", values) for an
array, ("out", count) for `count` doubles the library writes and ("struct", name, fields) for one of hip.py's structures (fh_run's two); `marshal`
turns them into ctypes by the entry point's row in hip.SIGNATURES.

The shapes are the smallest each setter accepts, a few rows and a few columns: the calls either return from host code or run one tiny launch of
the kind the operator's own suite runs (init and one forward step).  The family entry/<form>/<entry point> asks every entry point that answers
by operator form -- the one-pass step, the device-side loop, row sharding, the dense rows, fh_apply, the read-only reports -- on every form, one
pair per context; where the form serves the call it runs at the shape the suite of that launch runs (DENSE_SERVED_AT)."""
import ctypes as C
import json
import os

import numpy as np

from fasta_python_amd import hip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refusals", "c_abi.json")

# ---- the constants the list is built from --------------------------------------------------------------------------------------------------------
KINDS = sorted(v for k, v in vars(hip).items() if k.startswith("PROX_") and isinstance(v, int))      # every FH_PROX_* hip.py mirrors
assert KINDS == list(range(hip.PROX_IDENTITY, hip.PROX_NUCBALL + 1))
KIND_NAMES = {v: k[5:].lower() for k, v in vars(hip).items() if k.startswith("PROX_") and isinstance(v, int)}
KINDS_AND_BEYOND = [KINDS[0] - 1] + KINDS + [KINDS[-1] + 1]

# every fh_set_* / matrix entry point of the ABI is either an operator setter (it appears in SETTERS below) or one of these
NOT_OPERATOR_SETTERS = {"fh_set_tuning", "fh_set_vector", "fh_set_prox", "fh_set_prox_split", "fh_set_prox_nuclear",
                        "fh_set_loss_lsq", "fh_set_loss_logistic", "fh_set_loss_softmax", "fh_set_loss_weights"}


def f64(*v):
    return ("f64", tuple(float(x) for x in v))


def ones(count):
    return f64(*([1.0] * count))


M, N = 3, 5                                         # the dense and the sparse matrix
A_DENSE = f64(*[((7 * i) % 5 - 2) / 4.0 for i in range(M * N)])
CSR = (("i64", (0, 2, 3, 5)), ("i32", (0, 3, 1, 2, 4)), f64(1.0, -0.5, 2.0, 0.25, -1.0))      # canonical, 5 entries
Q4 = f64(2, 1, 0, 0, 1, 2, 1, 0, 0, 1, 2, 1, 0, 0, 1, 2)                                         # symmetric
S34 = f64(*[((5 * i) % 7) / 4.0 for i in range(12)])
TAPS = f64(1.0, 0.5, -0.5, 0.25)
IN_FLIGHT_M, IN_FLIGHT_N = 9, 100                   # the step-in-flight states: the smallest problem the one-pass suite (tests/test_gpu_fused.py) steps;
#                                                     csrc/fh_host_launch.h:fused_shape_for has a kernel for every n >= 1 in either storage, so step_body accepts it

_set_matrix = ("fh_set_matrix", (A_DENSE, M, N, N))
_set_csr = ("fh_set_matrix_csr", (M, N, 5) + CSR)
# name -> (calls that put the form into a context, rows m, columns n, columns of the unknown L)
FORMS = {
    "dense": ((_set_matrix,), M, N, 1),
    "dense_rhs2": ((_set_matrix, ("fh_set_rhs", (2,))), M, N, 2),
    "csr": ((_set_csr,), M, N, 1),
    "csr_rhs2": ((("fh_set_matrix_csr_rhs", (M, N, 5) + CSR + (2,)),), M, N, 2),
    "stencil": ((("fh_set_stencil", (3, 4)),), 12, 24, 1),
    "stencil3d": ((("fh_set_stencil3d", (2, 2, 2)),), 8, 24, 1),
    "dct": ((("fh_set_dct", (8, None)),), 8, 8, 1),
    "dct2": ((("fh_set_dct2", (2, 3, None)),), 6, 6, 1),
    "conv": ((("fh_set_conv2d", (3, 4, 2, 2, 0, 0, TAPS, None)),), 12, 12, 1),
    "identity": ((("fh_set_identity", (3, 5)),), 15, 15, 1),
    "quad1": ((("fh_set_quadratic", (Q4, 4, 4, None, 1)),), 4, 4, 1),
    "quad2": ((("fh_set_quadratic", (Q4, 4, 4, None, 2)),), 4, 4, 2),
    "factor": ((("fh_set_factorization", (S34, 3, 4, 4, 2)),), 7, 7, 2),
}
assert len(FORMS) == 13                             # twelve forms, the quadratic one with L = 1 and L = 2
# the other two ways into the dense form (csrc/fasta_hip.hip: setup_dense): swept over the context states with the forms
SETTERS = dict(FORMS)
SETTERS["dense_generated"] = ((("fh_generate_matrix", (M, N, 0, 7, 0.5)),), M, N, 1)
SETTERS["dense_f32_host"] = ((("fh_set_matrix_f32", (("f32", A_DENSE[1]), M, N, N)),), M, N, 1)
OPERATOR_SETTERS = sorted({name for calls, _, _, _ in SETTERS.values() for name, _ in calls})
# the OP_* form (csrc/fh_host_ctx.h) behind each entry: test_refusals_cpu.py wants a refusal recorded for every one of them
OP_OF = {"dense": "OP_DENSE", "dense_rhs2": "OP_DENSE", "csr": "OP_SPARSE", "csr_rhs2": "OP_SPARSE", "stencil": "OP_STENCIL", "stencil3d": "OP_STENCIL3D",
         "dct": "OP_DCT", "dct2": "OP_DCT", "conv": "OP_CONV", "identity": "OP_IDENTITY", "quad1": "OP_QUAD", "quad2": "OP_QUAD", "factor": "OP_BILINEAR"}

# float64; float32 storage; two blocks on one device; a one-rank communicator; fh_step_begin issued; ... on float32 storage (which of the two a setter names first)
STATES = ("plain", "f32", "shell", "comm", "in_flight", "f32_in_flight")
HOME_OF = {hip.PROX_GROUP: "dense_rhs2", hip.PROX_ROWBALL: "quad2", hip.PROX_ROWSPLIT: "factor", hip.PROX_NUCLEAR: "identity", hip.PROX_NUCBALL: "identity"}

SCALARS = ("out", hip.NSCALARS)
TAU = 0.5


def set_prox(kind):
    return ("fh_set_prox", (kind, 0.5, -1.0, 1.0))


SET_PROX_SPLIT = ("fh_set_prox_split", (3, hip.PROX_SHRINK, 0.5, 0.0, 0.0, hip.PROX_NONNEG, 0.0, 0.0))       # 3 = the rows of the first factor of "factor"
SET_PROX_NUCLEAR = ("fh_set_prox_nuclear", (0.5, 1))


def home_prox(kind):
    """The call that sets `kind` on the form that serves it."""
    return SET_PROX_SPLIT if kind == hip.PROX_ROWSPLIT else set_prox(kind)


def loss_calls(form):
    """Every loss entry point on a form, in an order in which each meets the state it checks: weights before any loss, then after one."""
    _, m, n, L = FORMS[form]
    b, w, labels = ones(m * L), ones(n), ("i32", (0,) * m)
    return (("fh_set_loss_weights", (w,)), ("fh_set_loss_weights", (None,)), ("fh_set_loss_lsq", (b, m * L)), ("fh_set_loss_weights", (w,)),
            ("fh_set_loss_weights", (None,)), ("fh_set_loss_logistic", (b, m * L)), ("fh_set_loss_weights", (w,)), ("fh_set_loss_softmax", (labels, m)))


def launch_calls(form, L=None):
    """A loss where the form takes one, then fh_init and one forward step from x0 = 0: the launch-time refusals, or one tiny launch each."""
    m, L = FORMS[form][1], L or FORMS[form][3]
    loss = () if OP_OF[form] in ("OP_QUAD", "OP_BILINEAR") else (("fh_set_loss_lsq", (ones(m * L), m * L)),)
    return loss + (("fh_init", (SCALARS,)), ("fh_fwd", (TAU, SCALARS)))


def dense_at(m, n):
    """The dense form at a shape at which a launch that serves it runs (the matrix of the in-flight states, and of fh_run)."""
    return ("fh_set_matrix", (f64(*[((3 * i) % 11 - 5) / 64.0 for i in range(m * n)]), m, n, n))


# ---- the entry points that answer by operator form: no one-pass kernel, no device-side loop, no row sharding, no dense rows, ... --------------------
RUN_M, RUN_N = 20, 600                              # the smallest problem the device loop's suite runs (tests/run_paths.py: stale_best)
ROOM = 128                                          # doubles / words behind every pointer: more than any report or vector of these shapes takes
WORDS, WORDS64 = ("i32", (0,) * ROOM), ("i64", (0,) * ROOM)
RUN_OPTS = ("struct", "RunOpts", (("window", 1), ("max_backtracks", 20), ("stepsize_shrink", 0.5)))
RUN_STATE = ("struct", "RunState", (("tau_next", 0.25), ("alpha1", 1.0), ("max_residual", float("-inf")), ("best_quality", float("inf"))))
SHAPE_EXPORTS = ("fh_multi_shape", "fh_quad_shape", "fh_bilinear_shape", "fh_tv3d_shape", "fh_conv_shape", "fh_dct_shape", "fh_dct2_shape", "fh_nuclear_shape")
# name in the case's id -> the calls, with valid arguments: the answer is the form's own.  ("uid",): replay puts a fresh RCCL id there.
ENTRIES = {
    "fh_step": (("fh_step", (TAU, SCALARS)),),
    "fh_step_begin": (("fh_step_begin", (TAU,)), ("fh_step_end", (SCALARS,))),
    "fh_step_accel": (("fh_step_accel", (TAU, 0.0, 0, SCALARS)),),
    "fh_run": (("fh_run", (1, RUN_OPTS, RUN_STATE, ("out", hip.RUN_HIST), ("i32", (0,)))),),
    "fh_comm_init": (("fh_comm_init", (1, 0, ("uid",))),),
    "fh_get_matrix_rows": (("fh_get_matrix_rows", (0, 1, ("out", ROOM))),),
    "fh_stream_read_ms": (("fh_stream_read_ms", (1, ("out", 1), ("i64", (0,)))),),
    "fh_apply_forward": (("fh_apply", (0, ones(ROOM), ("out", ROOM))),),
    "fh_apply_adjoint": (("fh_apply", (1, ones(ROOM), ("out", ROOM))),),
    "fh_sparse_lanes": (("fh_sparse_lanes", (0, WORDS, WORDS, WORDS)),),
}
ENTRIES.update({name: ((name, (WORDS64 if name == "fh_nuclear_shape" else WORDS,)),) for name in SHAPE_EXPORTS})
assert len(ENTRIES) == 18
# the dense form serves these: they run at the shape the suite of the launch runs them
DENSE_SERVED_AT = {"fh_step": (IN_FLIGHT_M, IN_FLIGHT_N), "fh_step_begin": (IN_FLIGHT_M, IN_FLIGHT_N), "fh_step_accel": (IN_FLIGHT_M, IN_FLIGHT_N),
                   "fh_run": (RUN_M, RUN_N)}


def entry_cases():
    """entry/<form>/<entry point>: the form, a loss where it takes one, fh_init, then the one call (fh_step_begin: and fh_step_end), each pair on a
    context of its own."""
    out = []
    for form, (setup, m, _, _) in FORMS.items():
        for entry, calls in ENTRIES.items():
            if form == "dense" and entry in DENSE_SERVED_AT:
                m_at, n_at = DENSE_SERVED_AT[entry]
                prelude = (dense_at(m_at, n_at), ("fh_set_loss_lsq", (ones(m_at), m_at)), ("fh_init", (SCALARS,)))
            else:
                prelude = setup + launch_calls(form)[:-1]          # (without the forward step)
            out.append((f"entry/{form}/{entry}", "plain", prelude + calls))
    return out


def cases():
    out = []
    for form, (setup, m, n, L) in FORMS.items():
        # per form: every prox call, every loss call, every column count
        out.append((f"form/{form}/prox", "plain", setup + tuple(set_prox(k) for k in KINDS_AND_BEYOND) + (SET_PROX_SPLIT, SET_PROX_NUCLEAR)))
        out.append((f"form/{form}/loss", "plain", setup + loss_calls(form)))
        out.append((f"form/{form}/rhs", "plain", setup + (("fh_set_rhs", (17,)), ("fh_set_rhs", (0,)), ("fh_set_rhs", (2,)), ("fh_rhs", ()))))
    # the dense forms: what fh_set_rhs makes of the prox and the loss the context holds (a launch in the vector form shows what it kept)
    for form in ("dense", "dense_rhs2"):
        setup, m, _, L = FORMS[form]
        for kind in KINDS:
            out.append((f"form/{form}/rhs_with_{KIND_NAMES[kind]}", "plain",
                        setup + (set_prox(kind), ("fh_set_rhs", (2,)), ("fh_set_rhs", (0,))) + launch_calls(form, L=1)))
        out.append((f"form/{form}/rhs_with_logistic", "plain", setup + (("fh_set_loss_logistic", (ones(m * L), m * L)), ("fh_set_rhs", (2,)))))
    # per context state: every setter
    for state in STATES:
        if state == "comm":             # (a communicator takes a second to attach: one context meets every setter in turn; the dense ones succeed, the others leave it as it was)
            out.append(("state/comm/every_setter", state, tuple(call for setup, _, _, _ in SETTERS.values() for call in setup)))
            continue
        for name, (setup, _, _, _) in SETTERS.items():
            out.append((f"state/{state}/{name}", state, setup))
    # what survives a change of operator: a kind set on an empty context (or, the kinds one form alone serves, on that form), then each form, then a launch
    for kind in KINDS:
        for form, (setup, _, _, _) in FORMS.items():
            out.append((f"survive/{KIND_NAMES[kind]}/{form}", "plain", (set_prox(kind),) + setup + launch_calls(form)))
    for kind, home in HOME_OF.items():
        for form, (setup, _, _, _) in FORMS.items():
            out.append((f"carry/{KIND_NAMES[kind]}_from_{home}/{form}", "plain", FORMS[home][0] + (home_prox(kind),) + setup + launch_calls(form)))
    # weights held on an identity context, then every other setter
    held = FORMS["identity"][0] + (("fh_set_loss_lsq", (ones(15), 15)), ("fh_set_loss_weights", (ones(15),)))
    for name, (setup, _, _, _) in SETTERS.items():
        out.append((f"weights/{name}", "plain", held + setup + (("fh_set_loss_weights", (None,)),)))
    return out + entry_cases()


CASES = cases()
IDS = [c[0] for c in CASES]
assert len(set(IDS)) == len(IDS)


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


# ---- replay (GPU) -----------------------------------------------------------------------------------------------------------------------------------
_NP = {"f64": np.float64, "i64": np.int64, "i32": np.int32, "f32": np.float32}


def marshal(name, args, keep):
    """ctypes arguments of one call (without the context); the arrays are appended to `keep` so that they outlive the call."""
    types = hip.SIGNATURES[name][1][1:]
    assert len(types) == len(args), (name, args)
    out = []
    for t, a in zip(types, args):
        if a is None:
            out.append(None)
        elif isinstance(a, tuple) and a[0] == "struct":
            keep.append(getattr(hip, a[1])(**dict(a[2])))
            out.append(C.byref(keep[-1]))
        elif isinstance(a, tuple):
            arr = np.zeros(a[1]) if a[0] == "out" else np.array(a[1], dtype=_NP[a[0]])
            keep.append(arr)
            out.append(arr.ctypes.data_as(t))
        else:
            out.append(a)
    return out


def _open(lib, state):
    """(handle, calls to make before the handle is destroyed) of a context in `state`; whatever prepares the state must succeed."""
    h = C.c_void_p()

    def must(status):
        assert status == 0, (state, status, lib.fh_last_error().decode())
    if state == "plain":
        must(lib.fh_create(0, C.byref(h)))
    elif state == "f32":
        must(lib.fh_create_ex(1, (C.c_int * 1)(0), hip.DTYPE_F32_STORAGE, C.byref(h)))
    elif state == "shell":
        must(lib.fh_create_ex(2, (C.c_int * 2)(0, 0), hip.DTYPE_F64, C.byref(h)))
    elif state == "comm":               # as tests/test_gpu_sharded.py attaches one: a communicator of one rank
        must(lib.fh_create(0, C.byref(h)))
        must(lib.fh_comm_init(h, 1, 0, C.create_string_buffer(hip.comm_unique_id(), hip.UNIQUE_ID_BYTES)))
    elif state in ("in_flight", "f32_in_flight"):
        must(lib.fh_create(0, C.byref(h)) if state == "in_flight" else lib.fh_create_ex(1, (C.c_int * 1)(0), hip.DTYPE_F32_STORAGE, C.byref(h)))
        keep = []
        m = IN_FLIGHT_M
        for name, args in (dense_at(m, IN_FLIGHT_N), ("fh_set_loss_lsq", (ones(m), m)), set_prox(hip.PROX_SHRINK), ("fh_init", (SCALARS,)),
                           ("fh_step_begin", (0.25,))):
            must(getattr(lib, name)(h, *marshal(name, args, keep)))
    else:
        raise ValueError(state)
    return h


def replay(lib, case):
    """[[status, text], ...] of the calls of one case on a fresh context.  A case in the in-flight state ends with fh_step_end (recorded as well)."""
    _, state, calls = case
    h = _open(lib, state)
    keep, got = [], []
    try:
        if state.endswith("in_flight"):
            calls = calls + (("fh_step_end", (SCALARS,)),)
        for name, args in calls:
            if name == "fh_rhs":       # the column count the context reports, in place of a text
                L = C.c_uint32(99)
                status = lib.fh_rhs(h, C.byref(L))
                got.append([int(status), f"L = {L.value}"])
                continue
            if name == "fh_comm_init":  # a one-rank communicator as the state "comm" makes it: the id is RCCL's, fresh per call
                keep.append(C.create_string_buffer(hip.comm_unique_id(), hip.UNIQUE_ID_BYTES))
                args = args[:2] + (keep[-1],)
            status = getattr(lib, name)(h, *marshal(name, args, keep))
            got.append([int(status), lib.fh_last_error().decode() if status else ""])
    finally:
        lib.fh_destroy(h)
    return got
