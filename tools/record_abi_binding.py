"""Record the ctypes binding of libescgnn_hip.so as the package presents it: tests/golden/abi_binding.json, the fixture of
tests/test_abi_binding_cpu.py.  Run it at the commit whose binding is the yardstick (the parent of a change to how the binding
is made), on the CPU with the library built: per entry point the category of every parameter and of the return value as
`lib()` has them set (`ptr i64 -> i32`), per struct class `size: name:offset:size ...` over its members, and the constants the
package names; one line per entry point and per struct.  Categories: ptr (c_void_p and every POINTER(...)), i32, i64, u64, f32, f64, cstr.

    python tools/record_abi_binding.py [--out tests/golden/abi_binding.json]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

CATEGORY = {ctypes.c_void_p: "ptr", ctypes.c_char_p: "cstr", ctypes.c_int: "i32", ctypes.c_int32: "i32", ctypes.c_int64: "i64",
            ctypes.c_uint64: "u64", ctypes.c_float: "f32", ctypes.c_double: "f64"}
# the struct classes by the names the package keeps for them
NATIVE_STRUCTS = ("CollateArgs", "BnFuse", "BnFold", "BnBwdFused", "BnBwdNext")
ENGINE_STRUCTS = ("_Linear", "_BN", "_MLP", "_Conv", "_Model", "_Batch", "_Embed", "_ZincModel", "_MolBatch", "_TableList",
                  "_OgbLayer", "_OgbModel", "_BagPlan", "_OgbBatch")


def category(t):
    if isinstance(t, type) and issubclass(t, ctypes._Pointer):
        return "ptr"
    return CATEGORY[t]


def layout(cls):
    """size of a ctypes.Structure subclass and its members `name:offset:size` in declaration order (the class body's own order;
    a member is what carries an offset and a size)"""
    found = [(name, d) for name, d in vars(cls).items() if hasattr(d, "offset") and hasattr(d, "size")]
    return "%d: %s" % (ctypes.sizeof(cls), " ".join("%s:%d:%d" % (name, d.offset, d.size) for name, d in found))


def record():
    from esc_gnn_amd import _native as nv, cycles, engine, graphlets, utils_edge_efficient
    h = nv.lib()
    out = {"functions": {}, "structs": {}}
    for name in sorted(nv.SIGNATURES):
        fn = getattr(h, name)
        out["functions"][name] = "%s -> %s" % (" ".join(category(t) for t in fn.argtypes), category(fn.restype))
    for mod, names in ((nv, NATIVE_STRUCTS), (engine, ENGINE_STRUCTS)):
        for name in names:
            out["structs"]["%s.%s" % (mod.__name__.rsplit(".", 1)[-1], name)] = layout(getattr(mod, name))
    out["KIND"] = dict(nv.KIND)
    out["ABI_VERSION"] = nv.ABI_VERSION
    out["constants"] = {"engine.MAX_LAYERS": engine.MAX_LAYERS, "engine.MAX_BN_COUNTERS": engine.MAX_BN_COUNTERS,
                        "engine.MAX_TABLES": engine.MAX_TABLES, "engine._PLAN_FIELDS": " ".join(engine._PLAN_FIELDS),
                        "cycles.ESC_ERANGE": cycles.ESC_ERANGE, "graphlets.ESC_ERANGE": graphlets.ESC_ERANGE,
                        "utils_edge_efficient.ESC_ERANGE": utils_edge_efficient.ESC_ERANGE}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "abi_binding.json"))
    args = ap.parse_args()
    with open(args.out, "w") as f:
        json.dump(record(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s" % args.out)
