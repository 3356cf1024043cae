"""The gate program of the MPS builders as the C libraries take it: ctypes mirrors of ``qk_program`` and ``qk_build_run``
(``include/qkgram.h``: the device builder, ``qk_build_program``) and of ``qkb_run`` and ``qkb_result`` (``csrc/qk_builder.h``: the
native host builder, ``qkb_simulate_program``), and the one function that fills a ``qk_program`` from arrays."""
import ctypes as C

_P = C.c_void_p


class QkProgram(C.Structure):
    _fields_ = [("size", C.c_uint32), ("n_states", C.c_int32), ("n_qubits", C.c_int32), ("n_ops", C.c_int32), ("op", _P), ("q0", _P), ("alpha", _P),
                ("n_mats", C.c_int32), ("mats_state_stride", C.c_int32), ("mats", _P), ("mat", _P),
                ("n_channels", C.c_int32), ("n_channels2", C.c_int32), ("kraus", _P), ("n_kraus", _P), ("kraus2", _P), ("n_kraus2", _P), ("channel", _P), ("branch", _P),
                ("branch_state_stride", C.c_int32), ("first_gate", C.c_uint32), ("seed", C.c_uint64), ("state_index", _P), ("trajectory", _P),
                ("cond_gate", _P), ("cond_mask", _P)]


class QkBuildRun(C.Structure):
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("trunc_budget", C.c_double), ("value_of_zero", C.c_double), ("max_bond", C.c_int32),
                ("n_checkpoints", C.c_int32), ("checkpoints", _P), ("initial", _P), ("initial_snapshot", C.c_int32)]


class QkbRun(C.Structure):
    _fields_ = [("size", C.c_uint32), ("max_bond", C.c_int32), ("trunc_budget", C.c_double), ("value_of_zero", C.c_double), ("init_dims", _P), ("init_tensors", _P),
                ("init_centre", C.c_int32), ("init_fidelity", C.c_double), ("init_logw", C.c_double)]


class QkbResult(C.Structure):
    _fields_ = [("size", C.c_uint32), ("dims", _P), ("branches", _P), ("tensors", _P), ("n_complex", C.c_int64), ("fidelity", C.c_double), ("logw", C.c_double),
                ("margin", C.c_double)]


def sized(cls, **fields):
    """An instance of one of the structs above with its ``size`` set."""
    return cls(size=C.sizeof(cls), **fields)


def check_sizes(lib, exports):
    """Refuse a library whose structs are not the ones mirrored here: ``exports`` maps the name of a ``uint32_t f(void)`` of ``lib``
    to the class whose size it must return."""
    for name, cls in exports.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = C.c_uint32, []
        if f() != C.sizeof(cls):
            raise ImportError(f"{name}() = {f()}, but {cls.__name__} here has {C.sizeof(cls)} bytes: the library and this module are of different builds")


def _ptr(a):
    return None if a is None else a.ctypes.data


def fill_program(n_states, n_qubits, op, q0, alpha, mats=None, mat=None, mats_state_stride=0, kraus=None, n_kraus=None, kraus2=None, n_kraus2=None, channel=None,
                 branch=None, branch_state_stride=0, seed=0, state_index=None, trajectory=None, first_gate=0, cond_gate=None, cond_mask=None):
    """A ``qk_program`` over numpy arrays that are already C-contiguous and of the field's type (int8 op; int32 q0, mat, counts, channel,
    branch, cond_gate; float64 alpha; complex128 tables; uint32 state_index, trajectory, cond_mask).  A table given as ``None`` is
    absent (count 0); the counts are the tables' leading extents (``mats`` is [n_mats][4][4], or [n_states][n_mats][4][4] with
    ``mats_state_stride = n_mats``).  The struct keeps the arrays alive."""
    p = sized(QkProgram, n_states=int(n_states), n_qubits=int(n_qubits), n_ops=int(op.shape[0]), op=_ptr(op), q0=_ptr(q0), alpha=_ptr(alpha),
              n_mats=0 if mats is None else int(mats.shape[-3]), mats_state_stride=int(mats_state_stride), mats=_ptr(mats), mat=_ptr(mat),
              n_channels=0 if kraus is None else int(kraus.shape[0]), n_channels2=0 if kraus2 is None else int(kraus2.shape[0]), kraus=_ptr(kraus), n_kraus=_ptr(n_kraus),
              kraus2=_ptr(kraus2), n_kraus2=_ptr(n_kraus2), channel=_ptr(channel), branch=_ptr(branch), branch_state_stride=int(branch_state_stride),
              first_gate=int(first_gate), seed=int(seed), state_index=_ptr(state_index), trajectory=_ptr(trajectory), cond_gate=_ptr(cond_gate), cond_mask=_ptr(cond_mask))
    p.arrays = (op, q0, alpha, mats, mat, kraus, n_kraus, kraus2, n_kraus2, channel, branch, state_index, trajectory, cond_gate, cond_mask)
    return p
