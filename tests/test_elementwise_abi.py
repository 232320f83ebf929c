"""The element-wise / gated entry points across the three places that must agree (no GPU needed):
the built library exports them, shim/lk_hip.def hands their header to cinterop and the Kotlin shim
sends its element-wise nodes through lk_graph_create_ops, and ggml_hip/_lib.py binds them with the arity include/lk_hip.h declares. Their
validation (no device work) returns what the Kotlin operators throw."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lk_hip.h")
SHIM = os.path.join(ROOT, "llama.kotlin_amd", "shim")

NEW = ("lk_binary_device", "lk_unary_device", "lk_mul_mat_gated_device", "lk_plan_create_gated",
       "lk_graph_create_ops", "lk_graph_num_fused")


@pytest.fixture(scope="module")
def lib():
    import ggml_hip._lib as L
    if not os.path.exists(L.LIB_PATH):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "llama.kotlin_amd")], check=True)
    return L.load()


def header_arity():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(lk_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_exported_declared_and_bound_with_matching_arity(lib):
    import ggml_hip._lib as L
    arity = header_arity()
    for n in NEW:
        assert n in arity, f"{n} not declared in include/lk_hip.h"
        assert hasattr(lib, n), f"{n} not exported by the built library"
        assert n in L.EXPORTED_SYMBOLS
        assert len(getattr(lib, n).argtypes) == arity[n], (n, arity[n])
    assert arity["lk_binary_device"] == 5 and arity["lk_unary_device"] == 4 and arity["lk_mul_mat_gated_device"] == 6
    assert arity["lk_plan_create_gated"] == 8 and arity["lk_graph_create_ops"] == 8


def test_shim_reaches_the_new_entry_points():
    """A text check of the shim sources only: nothing here runs cinterop or Kotlin, so it shows that the
    shim names the entry points, not that a Kotlin build binds them (the .def binds the whole header
    through its `headers` line; the names it lists are a comment)."""
    d = open(os.path.join(SHIM, "lk_hip.def")).read()
    assert "lk_hip.h" in d  # cinterop binds every declaration of the header
    for n in NEW:
        assert n in d, f"{n} missing from shim/lk_hip.def"
    kt = open(os.path.join(SHIM, "GGMLHipBackend.kt")).read()
    # the Kotlin backend works on host ByteArrays: its element-wise nodes go through the resident graph
    assert "lk_graph_create_ops" in kt, "lk_graph_create_ops not used by shim/GGMLHipBackend.kt"
    for c in ("LK_OP_ADD", "LK_OP_MUL", "LK_OP_GELU", "LK_OP_SILU", "LK_OP_MUL_MAT"):
        assert c in kt, c
    for op in ("GGMLOp.ADD", "GGMLOp.MUL", "GGMLOp.GELU", "GGMLOp.SILU"):
        assert op in kt


def test_new_kernels_are_in_the_code_object(lib):
    import ggml_hip._lib as L
    blob = open(L.LIB_PATH, "rb").read()
    for k in (b"_ZN2lk5ew_v4", b"_ZN2lk10ew_strided", b"_ZN2lk17gemv_stream_gated"):
        assert k in blob, k


def test_enum_values_match_the_mirror():
    import ggml_hip as G
    src = open(HEADER).read()
    assert re.search(r"LK_BINARY_ADD = 1, LK_BINARY_MUL = 2", src)
    assert re.search(r"LK_ACT_NONE = 0, LK_ACT_GELU = 1, LK_ACT_SILU = 2", src)
    assert (G.Act.NONE, G.Act.GELU, G.Act.SILU) == (0, 1, 2)
    from ggml_hip.ops import LK_OP
    for op, v in LK_OP.items():
        assert re.search(rf"LK_OP_{op.name} = {v}\b", src), op


def _t(L, type_, ne, buf=None, nb=None, off=0):
    t = L.LkTensor()
    t.type = type_
    ne = list(ne) + [1] * (4 - len(ne))
    es = 4
    for i in range(4):
        t.ne[i] = ne[i]
        t.nb[i] = nb[i] if nb else es
        es *= max(ne[i], 1)
    if buf is not None:
        t.data = buf.ctypes.data
        t.buf_bytes = buf.size
    t.data_offset = off
    return t


def test_validation_statuses_without_a_device(lib):
    """Everything these calls refuse is refused before any device work."""
    import ggml_hip._lib as L
    buf = np.zeros(256, np.uint8)
    B = ctypes.byref
    a, b, d = (_t(L, 0, [8, 2], buf) for _ in range(3))
    assert lib.lk_binary_device(1, B(a), B(_t(L, 0, [8, 3], buf)), B(d), None) == L.LK_ERR_INVALID_ARG
    assert lib.lk_binary_device(2, B(a), B(b), B(_t(L, 0, [4, 4], buf)), None) == L.LK_ERR_INVALID_ARG
    assert lib.lk_binary_device(1, B(a), B(b), B(_t(L, 1, [8, 2], buf)), None) == L.LK_ERR_INVALID_ARG
    q = _t(L, 2, [32, 2], buf)
    assert lib.lk_binary_device(1, B(q), B(q), B(q), None) == L.LK_ERR_NOT_IMPLEMENTED
    assert lib.lk_unary_device(1, B(q), B(q), None) == L.LK_ERR_NOT_IMPLEMENTED
    assert lib.lk_binary_device(1, B(a), B(b), B(_t(L, 0, [8, 2], buf, off=2)), None) == L.LK_ERR_NOT_IMPLEMENTED
    assert lib.lk_binary_device(1, B(a), B(b), B(_t(L, 0, [8, 2], buf, off=4)), None) == L.LK_ERR_NOT_IMPLEMENTED  # overlap
    assert lib.lk_binary_device(1, B(a), B(b), B(_t(L, 0, [8, 2], None)), None) == L.LK_ERR_NO_BUFFER
    assert lib.lk_binary_device(1, B(a), B(b), B(_t(L, 0, [8, 2], buf[:32])), None) == L.LK_ERR_OUT_OF_BOUNDS
    e = _t(L, 0, [0, 4], None)
    assert lib.lk_binary_device(1, B(e), B(e), B(e), None) == L.LK_OK
    assert lib.lk_unary_device(2, B(e), B(e), None) == L.LK_OK
    assert lib.lk_binary_device(7, B(a), B(b), B(d), None) == L.LK_ERR_INVALID_ARG
    assert lib.lk_unary_device(0, B(a), B(d), None) == L.LK_ERR_INVALID_ARG
    # the gated product: act, gate/up shapes, K against A, gate type — in that order
    w = _t(L, 2, [64, 2], np.zeros(2 * 2 * 18, np.uint8))
    w.nb[0] = 18
    g, u, o = _t(L, 0, [1, 64], buf), _t(L, 0, [1, 64], buf), _t(L, 0, [1, 2], buf)
    assert lib.lk_mul_mat_gated_device(B(w), B(g), B(u), 0, B(o), None) == L.LK_ERR_INVALID_ARG
    assert lib.lk_mul_mat_gated_device(B(w), B(g), B(_t(L, 0, [1, 32], buf)), 1, B(o), None) == L.LK_ERR_INVALID_ARG
    g32 = _t(L, 0, [1, 32], buf)
    assert lib.lk_mul_mat_gated_device(B(w), B(g32), B(g32), 1, B(o), None) == L.LK_ERR_INVALID_ARG
    assert lib.lk_mul_mat_gated_device(B(w), B(_t(L, 1, [1, 64], buf)), B(u), 1, B(o), None) == L.LK_ERR_NOT_IMPLEMENTED
    ops = (ctypes.c_int32 * 1)(3)  # ADD1: not an op the graph takes
    h = ctypes.c_void_p()
    st = lib.lk_graph_create_ops(ops, B(a), B(b), B(d), 1, None, 0, ctypes.byref(h))
    assert st == L.LK_ERR_NOT_IMPLEMENTED and not h.value
