"""ctypes binding of libescgnn_hip.so (C ABI declared in include/escgnn_hip.h).

The library is the product: there is NO fallback.  If the shared object is missing or a symbol
cannot be resolved, importing/using the hot path raises immediately.
"""
import ctypes
import os
from ctypes import c_double, c_int64

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libescgnn_hip.so")


class NativeLibraryError(ImportError):
    pass


# Everything below is derived from the header (_abi.py): editing the header is editing the binding.
try:
    _ABI = _abi.load()
except OSError as exc:
    raise NativeLibraryError("esc_gnn_amd: cannot read the C header %s the binding is derived from (%s)" % (_abi.HEADER, exc)) from exc


def const(name):
    """the value of a `#define ESC_*` or of an enum member of the header"""
    return _ABI.constants[name]


def struct(name):
    """the ctypes.Structure class of a `typedef struct` of the header"""
    return _ABI.structs[name]


def callback(name):
    """the CFUNCTYPE of a function-pointer typedef of the header"""
    return _ABI.callbacks[name]


members = _abi.members                      # [(name, offset, size)] of a struct class, in declaration order
ABI_VERSION = const("ESC_ABI_VERSION")
ESC_ERANGE = const("ESC_ERANGE")            # the status of an input outside the encodable range (cycles, graphlets, features)
SIGNATURES = {name: args for name, (args, _) in _ABI.functions.items()}     # name -> argtypes
_RET = {name: ret for name, (_, ret) in _ABI.functions.items()}
# the entry points of the extension header (escgnn_subgraphs.h: the NGNN baseline), derived the same way and bound beside them
EXTENSION_HEADER = os.path.join(os.path.dirname(_abi.HEADER), "escgnn_subgraphs.h")
try:
    _EXT = _abi.load(EXTENSION_HEADER)
except OSError as exc:
    raise NativeLibraryError("esc_gnn_amd: cannot read the C header %s the binding is derived from (%s)" % (EXTENSION_HEADER, exc)) from exc
EXTENSION_SIGNATURES = {name: args for name, (args, _) in _EXT.functions.items()}
_RET.update({name: ret for name, (_, ret) in _EXT.functions.items()})
# the second extension header (escgnn_i2gnn.h: the I2GNN baseline's expansion, pooling and gate), under names of its own
I2GNN_HEADER = os.path.join(os.path.dirname(_abi.HEADER), "escgnn_i2gnn.h")
try:
    _I2 = _abi.load(I2GNN_HEADER)
except OSError as exc:
    raise NativeLibraryError("esc_gnn_amd: cannot read the C header %s the binding is derived from (%s)" % (I2GNN_HEADER, exc)) from exc
I2GNN_SIGNATURES = {name: args for name, (args, _) in _I2.functions.items()}
_RET.update({name: ret for name, (_, ret) in _I2.functions.items()})
# the third extension header (escgnn_gineplus.h: the GINE+ baseline's multi-hop expansion and its one-launch aggregate)
GINEPLUS_HEADER = os.path.join(os.path.dirname(_abi.HEADER), "escgnn_gineplus.h")
try:
    _GP = _abi.load(GINEPLUS_HEADER)
except OSError as exc:
    raise NativeLibraryError("esc_gnn_amd: cannot read the C header %s the binding is derived from (%s)" % (GINEPLUS_HEADER, exc)) from exc
GINEPLUS_SIGNATURES = {name: args for name, (args, _) in _GP.functions.items()}
_RET.update({name: ret for name, (_, ret) in _GP.functions.items()})
# the fourth extension header (escgnn_gps.h: the graph transformer's ragged multi-head attention)
GPS_HEADER = os.path.join(os.path.dirname(_abi.HEADER), "escgnn_gps.h")
try:
    _GPS = _abi.load(GPS_HEADER)
except OSError as exc:
    raise NativeLibraryError("esc_gnn_amd: cannot read the C header %s the binding is derived from (%s)" % (GPS_HEADER, exc)) from exc
GPS_SIGNATURES = {name: args for name, (args, _) in _GPS.functions.items()}
_RET.update({name: ret for name, (_, ret) in _GPS.functions.items()})
# the fifth extension header (escgnn_lappe.h: the Laplacian eigen-solver, the PE table gather and the DeepSet LapPE encoder)
LAPPE_HEADER = os.path.join(os.path.dirname(_abi.HEADER), "escgnn_lappe.h")
try:
    _LAPPE = _abi.load(LAPPE_HEADER)
except OSError as exc:
    raise NativeLibraryError("esc_gnn_amd: cannot read the C header %s the binding is derived from (%s)" % (LAPPE_HEADER, exc)) from exc
LAPPE_SIGNATURES = {name: args for name, (args, _) in _LAPPE.functions.items()}
_RET.update({name: ret for name, (_, ret) in _LAPPE.functions.items()})
# the sixth extension header (escgnn_rwse.h: the random-walk landing probabilities and the gather from their resident table)
RWSE_HEADER = os.path.join(os.path.dirname(_abi.HEADER), "escgnn_rwse.h")
try:
    _RWSE = _abi.load(RWSE_HEADER)
except OSError as exc:
    raise NativeLibraryError("esc_gnn_amd: cannot read the C header %s the binding is derived from (%s)" % (RWSE_HEADER, exc)) from exc
RWSE_SIGNATURES = {name: args for name, (args, _) in _RWSE.functions.items()}
_RET.update({name: ret for name, (_, ret) in _RWSE.functions.items()})
# the seventh extension header (escgnn_step.h: the optimiser step on the counting engine's two streams and its fast seam)
STEP_HEADER = os.path.join(os.path.dirname(_abi.HEADER), "escgnn_step.h")
try:
    _STEP = _abi.load(STEP_HEADER)
except OSError as exc:
    raise NativeLibraryError("esc_gnn_amd: cannot read the C header %s the binding is derived from (%s)" % (STEP_HEADER, exc)) from exc
STEP_SIGNATURES = {name: args for name, (args, _) in _STEP.functions.items()}
_RET.update({name: ret for name, (_, ret) in _STEP.functions.items()})
# the eighth extension header (escgnn_gatedgcn.h: the gate of the GatedGCN local layer, forward and backward)
GATEDGCN_HEADER = os.path.join(os.path.dirname(_abi.HEADER), "escgnn_gatedgcn.h")
try:
    _GATED = _abi.load(GATEDGCN_HEADER)
except OSError as exc:
    raise NativeLibraryError("esc_gnn_amd: cannot read the C header %s the binding is derived from (%s)" % (GATEDGCN_HEADER, exc)) from exc
GATEDGCN_SIGNATURES = {name: args for name, (args, _) in _GATED.functions.items()}
_RET.update({name: ret for name, (_, ret) in _GATED.functions.items()})
# the ninth extension header (escgnn_pna.h: the mean | max | sum aggregate of the PNA local layer, forward and backward)
PNA_HEADER = os.path.join(os.path.dirname(_abi.HEADER), "escgnn_pna.h")
try:
    _PNA = _abi.load(PNA_HEADER)
except OSError as exc:
    raise NativeLibraryError("esc_gnn_amd: cannot read the C header %s the binding is derived from (%s)" % (PNA_HEADER, exc)) from exc
PNA_SIGNATURES = {name: args for name, (args, _) in _PNA.functions.items()}
_RET.update({name: ret for name, (_, ret) in _PNA.functions.items()})
# the tenth extension header (escgnn_spd.h: all-pairs shortest-path distances, their table gather and the biased ragged attention)
SPD_HEADER = os.path.join(os.path.dirname(_abi.HEADER), "escgnn_spd.h")
try:
    _SPD = _abi.load(SPD_HEADER)
except OSError as exc:
    raise NativeLibraryError("esc_gnn_amd: cannot read the C header %s the binding is derived from (%s)" % (SPD_HEADER, exc)) from exc
SPD_SIGNATURES = {name: args for name, (args, _) in _SPD.functions.items()}
_RET.update({name: ret for name, (_, ret) in _SPD.functions.items()})
# the eleventh extension header (escgnn_layernorm.h: the per-graph LayerNorm of the GPS layer, forward and backward)
LAYERNORM_HEADER = os.path.join(os.path.dirname(_abi.HEADER), "escgnn_layernorm.h")
try:
    _LN = _abi.load(LAYERNORM_HEADER)
except OSError as exc:
    raise NativeLibraryError("esc_gnn_amd: cannot read the C header %s the binding is derived from (%s)" % (LAYERNORM_HEADER, exc)) from exc
LAYERNORM_SIGNATURES = {name: args for name, (args, _) in _LN.functions.items()}
_RET.update({name: ret for name, (_, ret) in _LN.functions.items()})
KIND = {name[len("ESC_K_"):].lower(): v for name, v in _ABI.enum.items() if name != "ESC_K_COUNT"}

CollateArgs = struct("esc_collate_args")
BnFuse = struct("esc_bn_fuse")
BnFold = struct("esc_bn_fold")              # a BatchNorm still in partial form, merged by its consumer
BnBwdFused = struct("esc_bn_bwd_fused")     # a BatchNorm(+ReLU) backward applied to the dY operand of a Linear backward
BnBwdNext = struct("esc_bn_bwd_next")       # column sums of the NEXT BatchNorm backward from the dX tiles
SumJob = struct("esc_sum_job")
ReduceJob = struct("esc_reduce_job")

_lib = None


def lib():
    """Load (once) and return the ctypes handle; raise loudly if the HIP library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            "esc_gnn_amd: %s not found. The HIP hot path has no fallback — build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C esc-gnn_amd/csrc`." % LIB_PATH)
    h = ctypes.CDLL(LIB_PATH)
    for name, args in list(SIGNATURES.items()) + list(EXTENSION_SIGNATURES.items()) + list(I2GNN_SIGNATURES.items()) + list(GINEPLUS_SIGNATURES.items()) + list(GPS_SIGNATURES.items()) + list(LAPPE_SIGNATURES.items()) + list(RWSE_SIGNATURES.items()) + list(STEP_SIGNATURES.items()) + list(GATEDGCN_SIGNATURES.items()) + list(PNA_SIGNATURES.items()) + list(SPD_SIGNATURES.items()) + list(LAYERNORM_SIGNATURES.items()):
        try:
            fn = getattr(h, name)
        except AttributeError as exc:
            raise NativeLibraryError("esc_gnn_amd: %s lacks symbol %s (stale build?)" % (LIB_PATH, name)) from exc
        fn.argtypes = args
        fn.restype = _RET[name]
    if h.esc_abi_version() != ABI_VERSION:
        raise NativeLibraryError("esc_gnn_amd: ABI version mismatch (library %d, header %d) — rebuild"
                                 % (h.esc_abi_version(), ABI_VERSION))
    _lib = h
    return h


def call(name, *args):
    """Invoke an int-returning entry point; raise RuntimeError with the library's message on failure."""
    h = lib()
    rc = getattr(h, name)(*args)
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (name, rc, h.esc_last_error().decode()))


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def prof_enable(kind, on=True):
    call("esc_prof_enable", KIND[kind], int(on))


def prof_reset(kind):
    call("esc_prof_reset", KIND[kind])


def prof_read(kind):
    n, ms = c_int64(0), c_double(0.0)
    call("esc_prof_read", KIND[kind], ctypes.byref(n), ctypes.byref(ms))
    return n.value, ms.value


def prof_span_arm(kind, launches):
    """also stamp the in-kernel execution window of the next `launches` profiled launches (kernels with a span argument)"""
    call("esc_prof_span_arm", KIND[kind], int(launches), stream())


def prof_span_read(kind, cap=1 << 16):
    """execution windows (us) of the armed launches, in launch order — call after a device synchronise"""
    buf = (c_double * cap)()
    n = lib().esc_prof_span_read(KIND[kind], buf, cap)
    return [buf[i] for i in range(n)]


def prof_read_all(kind, cap=1 << 16):
    """per-launch durations (ms) of the recorded launches of a kernel family, in launch order"""
    buf = (c_double * cap)()
    n = lib().esc_prof_read_all(KIND[kind], buf, cap)
    return [buf[i] for i in range(n)]
