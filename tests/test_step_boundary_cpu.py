"""The step boundary without a GPU: the binding of include/escgnn_step.h, and the host-side state of the fast seam where no
launch is involved — a claim with no split optimiser step in front of it is not taken, the counters start at zero."""
import ctypes


def _want():
    p, i64, i, d = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
    return {
        "esc_engine_adam_step": ([p, p, p, p, i64, i64, d, d, d, d, i64, p], i),
        "esc_engine_claim_fast_seam": ([], i),
        "esc_engine_drop_fast_seam": ([], i),
        "esc_engine_seam_count": ([i], i64),
    }


def test_header_declares_exactly_the_new_entry_points():
    from esc_gnn_amd import _abi, _native as nv
    abi = _abi.load(nv.STEP_HEADER)
    assert not abi.structs and not abi.constants and not abi.callbacks
    want = _want()
    assert {k: (list(a), r) for k, (a, r) in abi.functions.items()} == want
    assert set(nv.STEP_SIGNATURES) == set(want)
    others = [nv.SIGNATURES, nv.EXTENSION_SIGNATURES, nv.I2GNN_SIGNATURES, nv.GINEPLUS_SIGNATURES, nv.GPS_SIGNATURES, nv.LAPPE_SIGNATURES,
              nv.RWSE_SIGNATURES]
    assert not any(set(want) & set(o) for o in others)
    assert nv.ABI_VERSION == nv.const("ESC_ABI_VERSION")


def test_every_declared_symbol_is_exported_by_the_built_library():
    from esc_gnn_amd import _native as nv
    h = ctypes.CDLL(nv.LIB_PATH)
    for name in _want():
        assert hasattr(h, name), name


def test_a_claim_without_a_split_optimiser_step_is_not_kept():
    from esc_gnn_amd import _native as nv
    h = nv.lib()
    before = (h.esc_engine_seam_count(0), h.esc_engine_seam_count(1))
    nv.call("esc_engine_claim_fast_seam")
    nv.call("esc_engine_drop_fast_seam")
    nv.call("esc_engine_set_side_stream", 256 | 2)
    nv.call("esc_engine_claim_fast_seam")
    nv.call("esc_engine_set_side_stream", 2)
    assert (h.esc_engine_seam_count(0), h.esc_engine_seam_count(1)) == before
    assert h.esc_engine_seam_count(2) == -1


def test_adam_entry_refuses_bad_extents_before_any_launch():
    from esc_gnn_amd import _native as nv
    import pytest
    buf = (ctypes.c_float * 4)()
    a = ctypes.addressof(buf)
    for n, k, step in ((4, 5, 1), (4, -1, 1), (-1, 0, 1), (4, 2, 0)):
        with pytest.raises(RuntimeError, match="esc_engine_adam_step"):
            nv.call("esc_engine_adam_step", a, a, a, a, n, k, 1e-3, 0.9, 0.999, 1e-8, step, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        nv.call("esc_engine_adam_step", None, a, a, a, 4, 2, 1e-3, 0.9, 0.999, 1e-8, 1, None)
