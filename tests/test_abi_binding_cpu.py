"""The ctypes binding is derived from include/escgnn_hip.h (esc-gnn_amd/_abi.py).  Checked here, without a GPU:
  1. the loaded binding equals the hand-written one it replaced, entry for entry: tests/golden/abi_binding.json, recorded by
     tools/record_abi_binding.py at the last commit that wrote the binding out by hand;
  2. every derived struct, member and constant equals what the host C++ compiler reports for the header;
  3. the reader refuses, quoting it, what its grammar does not cover;
  4. no hand-kept copy of a struct or of an argument list is left in the package or the tools.
"""
import ctypes
import glob
import importlib.util
import json
import os
import re
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from test_linear_plan_cpu import _host_compiler

_spec = importlib.util.spec_from_file_location("record_abi_binding", os.path.join(ROOT, "tools", "record_abi_binding.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

HEADER = os.path.join(ROOT, "include", "escgnn_hip.h")


def _abi():
    from esc_gnn_amd import _abi
    return _abi


def _header_text():
    with open(HEADER) as f:
        return f.read()


# ---- 1. the binding the package had when it was written by hand ---------------------------------------------------------
def test_binding_equals_the_recorded_hand_written_one():
    with open(os.path.join(GOLDEN, "abi_binding.json")) as f:
        want = json.load(f)
    got = json.loads(json.dumps(rec.record()))
    assert sorted(got) == sorted(want)
    for part in ("functions", "structs", "constants"):
        assert sorted(got[part]) == sorted(want[part]), part
        for name in want[part]:
            assert got[part][name] == want[part][name], (part, name)
    assert got["KIND"] == want["KIND"]
    assert got["ABI_VERSION"] == want["ABI_VERSION"]


def test_the_two_job_structs_have_their_classes():
    from esc_gnn_amd import _native as nv
    assert [m[0] for m in nv.members(nv.SumJob)] == ["v", "n", "out"]
    assert [m[0] for m in nv.members(nv.ReduceJob)] == ["slabs", "n", "splits", "cols", "dw", "ld_dw", "db_part", "rows", "db"]


def test_allreduce_callback_is_the_headers_typedef():
    from esc_gnn_amd import _native as nv, engine
    t = engine._ALLREDUCE_T
    assert t._restype_ is ctypes.c_int
    assert tuple(t._argtypes_) == (ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p)
    derived = nv.callback("esc_allreduce_fn")
    assert (t._restype_, tuple(t._argtypes_), t._flags_) == (derived._restype_, tuple(derived._argtypes_), derived._flags_)
    assert re.search(r"typedef\s+int\s*\(\*esc_allreduce_fn\)\(float\* buf, int64_t n, void\* stream, void\* user\);", _header_text())


def test_missing_header_is_a_native_library_error_naming_the_path(monkeypatch, tmp_path):
    from esc_gnn_amd import _native as nv
    missing = str(tmp_path / "no_such_header.h")
    monkeypatch.setattr(_abi(), "HEADER", missing)
    spec = importlib.util.spec_from_file_location("esc_gnn_amd._native_without_header", nv.__file__)
    with pytest.raises(ImportError, match=re.escape(missing)) as err:
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert type(err.value).__name__ == "NativeLibraryError"


# ---- 2. the C compiler's layout -----------------------------------------------------------------------------------------
def test_layout_and_constants_equal_the_c_compilers(tmp_path):
    abi, members = _abi().load(), _abi().members
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "escgnn_hip.h"', 'int main() {']
    expect = []
    for name, cls in abi.structs.items():
        lines.append('  std::printf("sizeof %s %%zu\\n", sizeof(%s));' % (name, name))
        expect.append("sizeof %s %d" % (name, ctypes.sizeof(cls)))
        for member, offset, size in members(cls):
            lines.append('  std::printf("member %s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % ((name, member) * 3))
            expect.append("member %s.%s %d %d" % (name, member, offset, size))
    for name, value in abi.constants.items():
        lines.append('  std::printf("constant %s %%lld\\n", (long long)(%s));' % (name, name))
        expect.append("constant %s %d" % (name, value))
    lines += ['  return 0;', '}']
    src, exe = str(tmp_path / "abi_layout.cpp"), str(tmp_path / "abi_layout")
    with open(src, "w") as f:
        f.write("\n".join(lines) + "\n")
    subprocess.run([_host_compiler(), "-std=c++17", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), src, "-o", exe],
                   check=True)
    got = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.split("\n")
    got = [g for g in got if g]
    assert len(got) == len(expect)
    for g, e in zip(got, expect):
        assert g == e
    # nothing of the header is missing from what was compared: find its declarations without the reader (a member the reader
    # lost shows above, in the sizes and offsets behind it)
    text = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    assert list(abi.structs) == re.findall(r"\btypedef\s+struct\s+(\w+)", text)
    assert sorted(abi.functions) == sorted(set(re.findall(r"\b(esc_[a-z0-9_]+)\s*\(", text)))
    assert sorted(n for n in abi.constants if n not in abi.enum) == sorted(re.findall(r"#define\s+(ESC_\w+)", text))


# ---- 3. strictness -------------------------------------------------------------------------------------------------------
EXTRA = {
    "bit-field": ("typedef struct esc_extra_t { int32_t flags : 3; int32_t rest; } esc_extra_t;", "flags : 3"),
    "struct by value": ("int esc_extra(esc_bn_fuse bn, void* stream);", "esc_bn_fuse bn"),
    "unknown scalar": ("int esc_extra(long n, void* stream);", "long n"),
    "no semicolon": ("int esc_extra(int64_t n, void* stream)", "int esc_extra(int64_t n, void* stream)"),
}
ANCHORS = ("int esc_prof_enable(int kind, int on);", "#ifdef __cplusplus\n}")      # in the middle of the header, and at its end


def test_the_header_itself_is_accepted():
    abi = _abi().parse(_header_text())
    assert abi.constants["ESC_MAX_BN_COUNTERS"] == 2 * abi.constants["ESC_MAX_LAYERS"] + 8 and abi.constants["ESC_K_COUNT"] == len(abi.enum) - 1


@pytest.mark.parametrize("anchor", range(len(ANCHORS)))
@pytest.mark.parametrize("case", sorted(EXTRA))
def test_reader_refuses_and_quotes(case, anchor):
    text, (extra, quoted) = _header_text(), EXTRA[case]
    assert text.count(ANCHORS[anchor]) == 1
    text = text.replace(ANCHORS[anchor], extra + "\n" + ANCHORS[anchor])
    with pytest.raises(_abi().HeaderError) as err:
        _abi().parse(text)
    assert quoted in str(err.value), str(err.value)


# ---- 4. no hand-kept copies ------------------------------------------------------------------------------------------------
def test_no_hand_kept_struct_or_argument_list_is_left():
    word = "_fields" + "_"
    sources = [p for d in ("esc-gnn_amd", "tools") for p in glob.glob(os.path.join(ROOT, d, "**", "*"), recursive=True)
               if os.path.isfile(p) and "__pycache__" not in p and os.path.splitext(p)[1] in (".py", ".hip", ".h", ".cpp", "")]
    assert len(sources) > 50
    for p in sources:
        with open(p, errors="replace") as f:
            assert word not in f.read(), p
    with open(os.path.join(ROOT, "esc-gnn_amd", "_native.py")) as f:
        native = f.read()
    assert not re.search(r"[\[,]\s*(P|I32|I64|F32|c_\w+|ctypes\.c_\w+|POINTER\([^)]*\))\s*[,\]]", native)
    assert "SIGNATURES = {name: args for name, (args, _) in _ABI.functions.items()}" in native
