"""Gated nodes in plans (lk_plan_create_gated): the second half of a Llama layer, {gate, up} -> gated
down, as ONE launch of two stages — the down stage reads gate and up through the chain's grid
barrier (write-through outputs, sc1 loads) and applies act(gate) ⊙ up on its way into the activation
image. Results must hold the bits of the nodes run one by one with the unfused ops, launch after
launch, also replayed from a HIP graph."""
import numpy as np
import pytest

import oracle as O
from _util import random_acts, random_weights

pytestmark = pytest.mark.gpu


def _mlp(G, qt, H, F, D, seed):
    """x [H] -> gate, up [F] (stage 0) -> down [D] gated (stage 1). Returns ga, nodes, stages and
    the tensors the unfused path needs."""
    ga = G.GGMLGraphAllocator(device="cuda", defaultBufferSize=16)

    def f32(n):
        return G.GGMLTensor(G.GGMLType.F32, [1, n], bufferId=ga.addBuffer(4 * n + 64))

    def weight(K, M, s):
        q = O.quantize(qt, random_weights(M * K, s, std=1.0 / np.sqrt(K)))
        a = G.GGMLTensor(G.GGMLType(qt), [K, M], bufferId=ga.addBuffer(q.size + 256))
        ga.setTensorBytes(a, q)
        return a

    x = f32(H)
    ga.setTensorBytes(x, random_acts(H, seed).view(np.uint8))
    wg, wu, wd = weight(H, F, seed + 1), weight(H, F, seed + 2), weight(F, D, seed + 3)
    g, u, t, h, d = f32(F), f32(F), f32(F), f32(F), f32(D)
    nodes = [(wg, x, g), (wu, x, u), (wd, g, d, u, G.Act.GELU)]
    return ga, nodes, [0, 0, 1], (wg, wu, wd, x, g, u, t, h, d)


def _unfused(G, ga, ts, act=1):
    import torch
    wg, wu, wd, x, g, u, t, h, d = ts
    G.computeMatMul(ga, None, wg, x, g)
    G.computeMatMul(ga, None, wu, x, u)
    G.computeUnary(act, ga, g, t)
    G.computeMul(ga, None, t, u, h)
    G.computeMatMul(ga, None, wd, h, d)
    torch.cuda.synchronize()
    return [ga.tensorBytes(v).cpu().numpy().copy() for v in (g, u, d)]


CHAINS = [(2, 512, 1024, 256), (2, 4096, 11008, 4096), (6, 256, 512, 256)]


@pytest.mark.parametrize("case", CHAINS, ids=lambda c: f"q{c[0]}-{c[1]}-{c[2]}-{c[3]}")
def test_gated_chain_equals_unfused(gpu, case):
    import torch
    import ggml_hip as G
    qt, H, F, D = case
    ga, nodes, stages, ts = _mlp(G, qt, H, F, D, seed=3 * qt + 1)
    ref = _unfused(G, ga, ts)
    outs = (ts[4], ts[5], ts[8])
    G.debugRoute()
    plan = G.MulMatPlan(ga, nodes, stages=stages)
    assert plan.numLaunches == 1
    for rep in range(3):
        for v in outs:
            ga.tensorBytes(v).fill_(0xFF)
        plan.launch()
        torch.cuda.synchronize()
        assert not plan.timedOut()
        for i, v in enumerate(outs):
            assert np.array_equal(ga.tensorBytes(v).cpu().numpy(), ref[i]), (rep, i)
    assert "stream_gated<" in G.debugRoute()
    # one HIP-graph capture and replay
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        plan.launch(stream=s)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=s):
        plan.launch(stream=s)
    for v in outs:
        ga.tensorBytes(v).zero_()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        cg.replay()
    torch.cuda.synchronize()
    for i, v in enumerate(outs):
        assert np.array_equal(ga.tensorBytes(v).cpu().numpy(), ref[i]), ("replay", i)
    assert not plan.timedOut()
    plan.close()


def test_gated_chain_with_a_reused_output_buffer(gpu):
    """A plain node and the gated node of a later stage write the SAME buffer (an allocator reusing
    o's storage for down: the barrier orders the writes), and a second gated node shares that dst
    too with another up. Each segment must keep its own node's gate: o stays a plain product."""
    import torch
    import ggml_hip as G
    H, F = 512, 1024
    ga = G.GGMLGraphAllocator(device="cuda", defaultBufferSize=16)

    def f32(n, seed=None):
        t = G.GGMLTensor(G.GGMLType.F32, [1, n], bufferId=ga.addBuffer(4 * n + 64))
        if seed is not None:
            ga.setTensorBytes(t, random_acts(n, seed).view(np.uint8))
        return t

    def weight(K, M, s):
        q = O.quantize(2, random_weights(M * K, s, std=1.0 / np.sqrt(K)))
        a = G.GGMLTensor(G.GGMLType.Q4_0, [K, M], bufferId=ga.addBuffer(q.size + 256))
        ga.setTensorBytes(a, q)
        return a

    x, r, g, u, u2, t, h, keep = f32(H, 1), f32(H), f32(F), f32(F), f32(F, 2), f32(F), f32(F), f32(H)
    wo, wg, wu, wd, wd2 = weight(H, H, 3), weight(H, F, 4), weight(H, F, 5), weight(F, H, 6), weight(F, H, 7)
    # stage 0: o = wo·x -> r;  stage 1: gate, up from r;  stage 2: gated down -> r again;
    # stage 3: a second gated node, other weights and another up, -> r once more
    nodes = [(wo, x, r), (wg, r, g), (wu, r, u), (wd, g, r, u, G.Act.GELU), (wd2, g, r, u2, G.Act.SILU)]
    stages = [0, 1, 1, 2, 3]
    G.computeMatMul(ga, None, wo, x, r)
    G.computeMatMul(ga, None, wg, r, g)
    G.computeMatMul(ga, None, wu, r, u)
    G.computeMatMulGated(ga, None, wd, g, u, G.Act.GELU, keep)
    G.computeUnary(G.Act.SILU, ga, g, t)
    G.computeMul(ga, None, t, u2, h)
    G.computeMatMul(ga, None, wd2, h, r)
    torch.cuda.synchronize()
    ref = [ga.tensorBytes(v).cpu().numpy().copy() for v in (g, u, r)]
    plan = G.MulMatPlan(ga, nodes, stages=stages)
    assert plan.numLaunches == 1
    for rep in range(2):
        for v in (g, u, r):
            ga.tensorBytes(v).fill_(0xFF)
        plan.launch()
        torch.cuda.synchronize()
        assert not plan.timedOut()
        for i, v in enumerate((g, u, r)):
            assert np.array_equal(ga.tensorBytes(v).cpu().numpy(), ref[i]), (rep, i)
    plan.close()
    # the same sharing in an independent plan of gated nodes only differing in up: each keeps its own
    d1, d2 = f32(H), f32(H)
    G.computeMatMulGated(ga, None, wd, g, u, G.Act.GELU, d1)
    G.computeMatMulGated(ga, None, wd, g, u2, G.Act.GELU, d2)
    e1, e2 = f32(H), f32(H)
    p2 = G.MulMatPlan(ga, [(wd, g, e1, u, G.Act.GELU), (wd, g, e2, u2, G.Act.GELU)])
    p2.launch()
    torch.cuda.synchronize()
    assert np.array_equal(ga.tensorBytes(e1).cpu().numpy(), ga.tensorBytes(d1).cpu().numpy())
    assert np.array_equal(ga.tensorBytes(e2).cpu().numpy(), ga.tensorBytes(d2).cpu().numpy())
    p2.close()


def test_gated_chain_refuses_what_cannot_stream(gpu):
    """A gated chain node with K % 64 != 0 is no streaming node: NotImplementedError, like any other."""
    import ggml_hip as G
    ga, nodes, stages, ts = _mlp(G, 2, 256, 96, 64, seed=9)
    with pytest.raises(NotImplementedError):
        G.MulMatPlan(ga, nodes, stages=stages)


def test_independent_gated_plan_equals_single_calls(gpu):
    """stages=None: two gated nodes (one streams, one runs the composition) and a plain node."""
    import torch
    import ggml_hip as G
    ga = G.GGMLGraphAllocator(device="cuda", defaultBufferSize=16)

    def f32(n, seed=None):
        t = G.GGMLTensor(G.GGMLType.F32, [1, n], bufferId=ga.addBuffer(4 * n + 64))
        if seed is not None:
            ga.setTensorBytes(t, random_acts(n, seed).view(np.uint8))
        return t

    def weight(K, M, s):
        q = O.quantize(2, random_weights(M * K, s, std=1.0 / np.sqrt(K)))
        a = G.GGMLTensor(G.GGMLType.Q4_0, [K, M], bufferId=ga.addBuffer(q.size + 256))
        ga.setTensorBytes(a, q)
        return a

    g1, u1, g2, u2, x = f32(1024, 1), f32(1024, 2), f32(96, 3), f32(96, 4), f32(1024, 5)
    w1, w2, w3 = weight(1024, 300, 6), weight(96, 40, 7), weight(1024, 128, 8)
    d1, d2, d3, r1, r2, r3 = f32(300), f32(40), f32(128), f32(300), f32(40), f32(128)
    G.computeMatMulGated(ga, None, w1, g1, u1, G.Act.GELU, r1)
    G.computeMatMulGated(ga, None, w2, g2, u2, G.Act.SILU, r2)
    G.computeMatMul(ga, None, w3, x, r3)
    plan = G.MulMatPlan(ga, [(w1, g1, d1, u1, G.Act.GELU), (w2, g2, d2, u2, G.Act.SILU), (w3, x, d3)])
    G.debugRoute()
    plan.launch()
    torch.cuda.synchronize()
    route = G.debugRoute()
    assert "stream_gated<" in route and "ewactmul:" in route and "stream<" in route, route
    for d, r in ((d1, r1), (d2, r2), (d3, r3)):
        assert np.array_equal(ga.tensorBytes(d).cpu().numpy(), ga.tensorBytes(r).cpu().numpy())
    plan.close()
