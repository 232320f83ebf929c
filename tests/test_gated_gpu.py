"""The gated product dst = A · (act(gate) ⊙ up) (lk_mul_mat_gated_device): the stream kernel's gated
intake (route stream_gated<qt,cpl>) and the composition (one element-wise launch into scratch, then
the ordinary route) must both hold the bits of the three calls computeUnary -> computeMul ->
computeMatMul on the device, and meet the parity bar against the oracle on the device-produced h.

Weights come from O.quantize; Q4_K and Q2_K, which the reference has no quantizer for, from random
super-blocks (tests/_kquant.py)."""
import numpy as np
import pytest

import oracle as O
from _kquant import random_kblocks
from _util import parity_ok, random_acts, random_weights

pytestmark = pytest.mark.gpu

ROW_BYTES = {2: (32, 18), 3: (32, 20), 6: (32, 34), 10: (256, 144)}


def _weights(qt, M, K, seed):
    if qt in (8, 10):
        return random_kblocks(qt, M * K // 256, seed)
    return O.quantize(qt, random_weights(M * K, seed, std=1.0 / np.sqrt(K)))


def _setup(G, qt, M, K, N=1, gate_offset=0, seed=5):
    """(ga, a, gate, up, t, h, dst_fused, dst_ref, q) on device buffers of their own."""
    ga = G.GGMLGraphAllocator(device="cuda", defaultBufferSize=16)
    q = _weights(qt, M, K, seed)
    a = G.GGMLTensor(G.GGMLType(qt), [K, M], bufferId=ga.addBuffer(q.size + 256))
    ga.setTensorBytes(a, q)

    def f32(ne, off=0):
        return G.GGMLTensor(G.GGMLType.F32, ne, bufferId=ga.addBuffer(4 * ne[0] * ne[1] + 64 + off), dataOffset=off)

    gate, up = f32([N, K], gate_offset), f32([N, K])
    ga.setTensorBytes(gate, random_acts(N * K, seed + 1).view(np.uint8))
    ga.setTensorBytes(up, random_acts(N * K, seed + 2).view(np.uint8))
    return ga, a, gate, up, f32([N, K]), f32([N, K]), f32([N, M]), f32([N, M]), q


def _run_both(G, qt, M, K, act, N=1, gate_offset=0):
    import torch
    ga, a, gate, up, t, h, d1, d0, q = _setup(G, qt, M, K, N, gate_offset)
    G.computeUnary(act, ga, gate, t)
    G.computeMul(ga, None, t, up, h)
    G.computeMatMul(ga, None, a, h, d0)
    ga.tensorBytes(d1).fill_(0xFF)
    G.debugRoute()
    G.computeMatMulGated(ga, None, a, gate, up, act, d1)
    torch.cuda.synchronize()
    route = G.debugRoute()
    got = ga.tensorBytes(d1).cpu().numpy().view(np.float32).copy()
    ref = ga.tensorBytes(d0).cpu().numpy().view(np.float32).copy()
    hv = ga.tensorBytes(h).cpu().numpy().view(np.float32).copy()
    return route, got, ref, hv, q


# the last two: Q2_K, which the stream kernel also carries (one and three units per row)
FUSED = [(2, 256, 1), (2, 4096, 9), (2, 4352, 520), (2, 8448, 64), (3, 128, 7), (6, 256, 33), (10, 4096, 16),
         (8, 4096, 16), (8, 9216, 8)]


@pytest.mark.parametrize("act", [1, 2], ids=["gelu", "silu"])
@pytest.mark.parametrize("case", FUSED, ids=lambda c: f"q{c[0]}-K{c[1]}-M{c[2]}")
def test_fused_equals_composition(gpu, case, act):
    import ggml_hip as G
    qt, K, M = case
    route, got, ref, hv, q = _run_both(G, qt, M, K, act)
    assert "stream_gated<" in route, route
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), np.flatnonzero(got != ref)[:8]
    if act == 1:  # one fused shape per quant type against the oracle would do; these are all small
        want = O.mat_mul_q(qt, q, M, K, hv.reshape(K, 1))
        ok, msg = parity_ok(got.reshape(M, 1), want)
        assert ok, msg


# (qt, K, M, N, gate data offset): K % 64 != 0, batches, a misaligned gate
COMPOSED = [(2, 96, 5, 1, 0), (2, 256, 33, 4, 0), (2, 512, 64, 32, 0), (2, 256, 33, 1, 4),
            (3, 96, 5, 1, 0), (6, 96, 5, 1, 0), (10, 256, 8, 2, 0)]


@pytest.mark.parametrize("case", COMPOSED, ids=lambda c: f"q{c[0]}-K{c[1]}-M{c[2]}-N{c[3]}-off{c[4]}")
def test_composition_route(gpu, case):
    import ggml_hip as G
    qt, K, M, N, off = case
    route, got, ref, hv, q = _run_both(G, qt, M, K, 1, N=N, gate_offset=off)
    assert "stream_gated<" not in route and route.startswith("ewactmul:"), route
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    want = O.mat_mul_q(qt, q, M, K, hv.reshape(K, N))
    from test_gpu_parity import noise_for
    ok, msg = parity_ok(got.reshape(M, N), want, noise=noise_for(O, qt, q, M, K, hv.reshape(K, N)) if qt != 10 else None)
    assert ok, msg


def test_validation(gpu):
    import ggml_hip as G
    ga, a, gate, up, t, h, d1, d0, q = _setup(G, 2, 16, 256)
    T = G.GGMLType

    def f32(ne):
        return G.GGMLTensor(T.F32, ne, bufferId=ga.addBuffer(4 * ne[0] * ne[1] + 64))

    with pytest.raises(G.IllegalArgumentException):  # gate.ne != up.ne
        G.computeMatMulGated(ga, None, a, gate, f32([1, 128]), 1, d1)
    with pytest.raises(G.IllegalArgumentException):  # K mismatch: gate and up agree, a does not
        G.computeMatMulGated(ga, None, a, f32([1, 128]), f32([1, 128]), 1, d1)
    with pytest.raises(G.IllegalArgumentException):  # act = 0
        G.computeMatMulGated(ga, None, a, gate, up, 0, d1)
    with pytest.raises(NotImplementedError):  # non-F32 gate (and up, so the type check is what fires)
        g16 = G.GGMLTensor(T.F16, [1, 256], bufferId=gate.bufferId)
        G.computeMatMulGated(ga, None, a, g16, up, 1, d1)
    with pytest.raises(G.IllegalArgumentException):  # dst shape
        G.computeMatMulGated(ga, None, a, gate, up, 1, f32([1, 17]))
