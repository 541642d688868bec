"""The C-ABI library loads and exports every symbol include/fhe_rocm.h declares (no GPU calls)."""
import ctypes
import os
import re

from conftest import ROOT
from fhe_sign import _lib


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "fhe_rocm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fhe_[a-z0-9_]+)\s*\(", text)))


def test_library_loads_and_exports_header_symbols():
    lib = _lib.load()
    syms = _header_symbols()
    assert len(syms) >= 20
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing


def test_binding_covers_header():
    assert sorted(_lib.declared_symbols()) == _header_symbols()


def test_launch_trace_entry_points():
    """the launch trace and its read-only hooks at the C boundary, on a simulated context: null arguments and unknown
    ids are refused, the trace is off until asked for, a size query writes nothing, the device table is a device
    context's"""
    C = ctypes
    from fhe_sign import FheUint, SimContext, SimKey, set_server_key
    lib = _lib.load()
    for name in ("fhe_ctx_trace", "fhe_ctx_trace_read", "fhe_radix_block_addrs", "fhe_biguint_block_addrs",
                 "fhe_ctx_lut_table", "fhe_ctx_export_luts", "fhe_ctx_pending_info", "fhe_host_set_tuning"):
        assert name in _lib.declared_symbols() and hasattr(lib, name)
    # the fault point's keys exist and are off: no site enabled, nothing armed, nothing counted
    prev = C.c_int64(-1)
    assert lib.fhe_host_set_tuning(7, 0, C.byref(prev)) == 0 and prev.value == 0  # FHE_TUNE_FAULT_SITES
    assert lib.fhe_host_set_tuning(8, 0, C.byref(prev)) == 0 and prev.value == 0  # FHE_TUNE_FAULT_AFTER
    assert lib.fhe_host_set_tuning(9, 0, C.byref(prev)) != 0
    assert lib.fhe_ctx_pending_info(None, (C.c_uint64 * 3)()) != 0
    n, kind, entries = C.c_size_t(7), C.c_int(), (C.c_int32 * 16)()
    assert lib.fhe_ctx_trace(None, 1) != 0
    assert lib.fhe_ctx_trace_read(None, None, 0, C.byref(n), 0) != 0
    ctx = SimContext()
    set_server_key(ctx)
    try:
        assert lib.fhe_ctx_trace_read(ctx.handle, None, 0, None, 0) != 0
        x = FheUint.try_encrypt(0x1B, SimKey(), bits=6)
        y = x + x
        assert y.decrypt(SimKey()) == 0x36
        assert lib.fhe_ctx_trace_read(ctx.handle, None, 0, C.byref(n), 0) == 0 and n.value == 0  # off by default
        assert lib.fhe_radix_block_addrs(ctx.handle, y.handle, None, None, 0, C.byref(n)) == 0 and n.value == 3
        addrs = (C.c_uint64 * 3)()
        assert lib.fhe_radix_block_addrs(ctx.handle, y.handle, addrs, None, 2, C.byref(n)) != 0  # too small
        assert lib.fhe_radix_block_addrs(ctx.handle, y.handle, addrs, None, 3, C.byref(n)) == 0
        assert len(set(addrs)) == 3 and all(addrs)
        assert lib.fhe_radix_block_addrs(ctx.handle, None, addrs, None, 3, C.byref(n)) != 0
        assert lib.fhe_ctx_lut_table(ctx.handle, 0, C.byref(kind), entries) == 0 and kind.value == 0
        assert lib.fhe_ctx_lut_table(ctx.handle, 1 << 20, C.byref(kind), entries) != 0
        assert lib.fhe_ctx_lut_table(ctx.handle, 0, None, entries) != 0
        assert lib.fhe_ctx_export_luts(ctx.handle, 0, 1, (C.c_uint64 * 2048)()) != 0
        assert b"simulated context" in lib.fhe_last_error()
    finally:
        set_server_key(None)
        ctx.close()


def test_params_default():
    from fhe_sign import default_params
    p = default_params()
    assert (p.lwe_dimension, p.polynomial_size, p.glwe_dimension) == (834, 2048, 1)
    assert (p.pbs_base_log, p.pbs_level, p.ks_base_log, p.ks_level) == (23, 1, 3, 5)
    assert (p.message_modulus, p.carry_modulus) == (4, 4)


def test_no_gpu_context_errors_loudly():
    """Without a GPU the product must refuse, never fall back to CPU arithmetic."""
    import pytest
    from fhe_sign import Context, FheError
    try:
        ctx = Context(0)
    except FheError as e:
        assert "GPU" in str(e) or "hip" in str(e).lower()
        return
    ctx.close()
    pytest.skip("GPU present: nothing to refuse")
