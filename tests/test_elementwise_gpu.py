"""F32 element-wise ops on the device (lk_binary_device / lk_unary_device): computeAdd, computeMul,
computeGelu and the explicit SiLU, against the numpy restatement in tests/_elementwise.py.

ADD / MUL are single IEEE operations: bit-identical to numpy float32 (NaN where numpy has NaN).
GELU / SiLU go through the device library's tanhf / expf: two gates, the project's F32 bar
(parity_ok) and the tight bar |dev - ref| <= 8 * 2^-24 * |x| (the reference's own float32 evaluation
is within 1.63 of those units of float64, two libm-grade float32 tanh differ by up to 1.96; the
device library's documented error is unknown, so it gets 4x the latter)."""
import numpy as np
import pytest

import _elementwise as E
from _util import parity_ok

pytestmark = pytest.mark.gpu

F32 = 0


def _tensor(G, ga, ne, nb=None, offset_extra=0, count=None):
    """An F32 tensor in a buffer of its own; storage for `count` floats (default: its elements)."""
    ne4 = list(ne) + [1] * (4 - len(ne))
    n = count if count is not None else int(np.prod(ne4))
    buf = ga.addBuffer(4 * n + 64 + offset_extra)
    return G.GGMLTensor(G.GGMLType.F32, ne4, nb=nb, bufferId=buf, dataOffset=offset_extra)


def _put(ga, t, flat):
    """Store the float32 array `flat` at t's storage start (physical order)."""
    ga.setTensorBytes(t, np.ascontiguousarray(flat, np.float32).view(np.uint8))


def _get(ga, t, n):
    return ga.tensorBytes(t, 4 * n).cpu().numpy().view(np.float32).copy()


CASES = ["contig", "transposed_a", "one", "tail4099", "offset4", "alias_a"]


@pytest.mark.parametrize("op", ["add", "mul"])
@pytest.mark.parametrize("case", CASES)
def test_binary_bits(gpu, op, case):
    import torch
    import ggml_hip as G
    ga = G.GGMLGraphAllocator(device="cuda", defaultBufferSize=16)
    ne = {"one": [1, 1, 1, 1], "tail4099": [4099, 1, 1, 1]}.get(case, [5, 3, 2, 1])
    n = int(np.prod(ne))
    av, bv = E.values(n, 11), E.values(n, 12)
    extra = 4 if case == "offset4" else 0
    b = _tensor(G, ga, ne, offset_extra=extra)
    _put(ga, b, bv)
    if case == "transposed_a":
        # a's storage is [i2][i0][i1]: element (i0, i1, i2) at 4 * (i1 + 3 * i0 + 15 * i2)
        a = _tensor(G, ga, ne, nb=[12, 4, 60, 120])
        phys = av.reshape(2, 3, 5).transpose(0, 2, 1)  # logical [i2][i1][i0] -> physical [i2][i0][i1]
        _put(ga, a, phys.reshape(-1))
    else:
        a = _tensor(G, ga, ne, offset_extra=extra)
        _put(ga, a, av)
    d = a if case == "alias_a" else _tensor(G, ga, ne, offset_extra=extra)
    G.debugRoute()
    (G.computeAdd if op == "add" else G.computeMul)(ga, ga.context, a, b, d)
    torch.cuda.synchronize()
    route = G.debugRoute()
    want_route = f"ew{op}:" + ("g" if case in ("transposed_a", "offset4") else "v4")
    assert route == want_route, route
    ref = (E.add_ref if op == "add" else E.mul_ref)(av, bv)
    got = _get(ga, d, n)
    assert E.same_bits(got, ref), (case, op, np.flatnonzero(got.view(np.uint32) != ref.view(np.uint32))[:8])
    if case != "alias_a":  # inputs are never mutated
        assert np.array_equal(_get(ga, b, n).view(np.uint32), bv.view(np.uint32))


def test_status_codes(gpu):
    """Kotlin's order: a.ne != b.ne, a.ne != dst.ne, dst.type != a.type (IllegalArgumentException); a
    type other than F32 (NotImplementedError: CPU path); then the device path's own: unaligned base or
    stride, a partial overlap (NotImplementedError), a missing buffer (IllegalStateException), an
    element past its buffer (IndexOutOfBoundsException); empty tensors do nothing."""
    import torch
    import ggml_hip as G
    ga = G.GGMLGraphAllocator(device="cuda", defaultBufferSize=16)
    T = G.GGMLType
    a, b, d = (_tensor(G, ga, [8, 2]) for _ in range(3))
    with pytest.raises(G.IllegalArgumentException):
        G.computeAdd(ga, None, a, _tensor(G, ga, [8, 3]), d)
    with pytest.raises(G.IllegalArgumentException):
        G.computeMul(ga, None, a, b, _tensor(G, ga, [4, 4]))
    with pytest.raises(G.IllegalArgumentException):
        G.computeAdd(ga, None, a, b, G.GGMLTensor(T.F16, [8, 2], bufferId=d.bufferId))
    with pytest.raises(G.IllegalArgumentException):
        G.computeGelu(ga, None, a, _tensor(G, ga, [2, 8]))
    q = [G.GGMLTensor(T.Q4_0, [32, 2], bufferId=ga.addBuffer(64)) for _ in range(3)]
    with pytest.raises(NotImplementedError):
        G.computeAdd(ga, None, q[0], q[1], q[2])
    with pytest.raises(NotImplementedError):
        G.computeGelu(ga, None, q[0], q[2])
    with pytest.raises(NotImplementedError):  # base not a multiple of 4
        G.computeAdd(ga, None, a, b, _tensor(G, ga, [8, 2], offset_extra=2))
    with pytest.raises(NotImplementedError):  # stride not a multiple of 4
        G.computeAdd(ga, None, a, b, _tensor(G, ga, [8, 2], nb=[4, 34, 68, 68], count=20))
    big = ga.addBuffer(4 * 32)
    x = G.GGMLTensor(T.F32, [8, 2], bufferId=big)
    with pytest.raises(NotImplementedError):  # dst overlaps a, shifted by one element
        G.computeAdd(ga, None, x, b, G.GGMLTensor(T.F32, [8, 2], bufferId=big, dataOffset=4))
    with pytest.raises(NotImplementedError):  # dst starts at a but with other strides
        G.computeAdd(ga, None, x, b, G.GGMLTensor(T.F32, [8, 2], nb=[4, 48, 96, 96], bufferId=big))
    with pytest.raises(G.IllegalStateException):
        G.computeAdd(ga, None, a, b, G.GGMLTensor(T.F32, [8, 2], bufferId=-1))
    with pytest.raises(G.IndexOutOfBoundsException):
        G.computeAdd(ga, None, a, b, G.GGMLTensor(T.F32, [8, 2], bufferId=ga.addBuffer(32)))
    # empty: LK_OK, nothing read or written (no buffers needed)
    e = [G.GGMLTensor(T.F32, [0, 4], bufferId=-1) for _ in range(3)]
    G.debugRoute()
    G.computeAdd(ga, None, e[0], e[1], e[2])
    G.computeGelu(ga, None, e[0], e[2])
    assert G.debugRoute() == ""
    with pytest.raises(G.IllegalArgumentException):  # unknown op / activation
        G.computeBinary(3, ga, a, b, d)
    with pytest.raises(G.IllegalArgumentException):
        G.computeUnary(G.Act.NONE, ga, a, d)
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def grid():
    x = np.linspace(-3, 4, 7001).astype(np.float32)
    return x, {1: E.gelu_ref(x), 2: E.silu_ref(x)}


@pytest.mark.parametrize("act", [1, 2], ids=["gelu", "silu"])
def test_activation_bars(gpu, grid, act):
    """Both gates per activation. Measured on an MI355X: max |dev - ref| = 1.80 (GELU)
    and 2.61 (SILU) units of 2^-24 |x|, against the bar of 8; the figure is printed before it is
    asserted."""
    import torch
    import ggml_hip as G
    x, refs = grid
    ref = refs[act]
    # the floor of the F32 bar must not hide a wrong tail: few reference points lie under it
    share = E.floor_share(ref)
    print(f"act {act}: share of points under the F32 bar's floor = {share:.4f}")
    assert share <= 0.02
    ga = G.GGMLGraphAllocator(device="cuda", defaultBufferSize=16)
    a, d = _tensor(G, ga, [x.size]), _tensor(G, ga, [x.size])
    _put(ga, a, x)
    G.debugRoute()
    G.computeUnary(act, ga, a, d)
    torch.cuda.synchronize()
    assert G.debugRoute() == "ewact:v4"
    got = _get(ga, d, x.size)
    ok, msg = parity_ok(got, ref)
    units = E.tight_units(got, ref, x)
    print(f"act {act}: parity {msg}; max |dev - ref| = {units:.3f} x 2^-24 |x|")
    assert ok, msg
    assert units <= 8.0, units
    assert got[x == 0].tolist() == ref[x == 0].tolist()
    if act == 1:  # computeSilu is the reference's GELU fallback
        G.computeSilu(ga, None, a, d)
        torch.cuda.synchronize()
        assert np.array_equal(_get(ga, d, x.size).view(np.uint32), got.view(np.uint32))


def test_gelu_specials(gpu):
    """NaN / Inf pattern only: gelu(-Inf) is NaN in Kotlin (-Inf * 0), gelu(+Inf) = +Inf."""
    import torch
    import ggml_hip as G
    x = np.array([np.inf, -np.inf, np.nan, 1e20, -1e20], np.float32)
    ref = E.gelu_ref(x)
    ga = G.GGMLGraphAllocator(device="cuda", defaultBufferSize=16)
    a, d = _tensor(G, ga, [x.size]), _tensor(G, ga, [x.size])
    _put(ga, a, x)
    G.computeGelu(ga, None, a, d)
    torch.cuda.synchronize()
    got = _get(ga, d, x.size)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), got
    assert np.array_equal(np.isinf(got), np.isinf(ref)) and np.array_equal(np.sign(got[np.isinf(got)]), np.sign(ref[np.isinf(ref)])), got
    assert np.isnan(got[1]) and got[0] == np.inf and np.isfinite(got[3]) and np.isfinite(got[4])
