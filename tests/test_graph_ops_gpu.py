"""Resident graphs with F32 element-wise nodes (lk_graph_create_ops): a Llama MLP with its residual
on host buffers — gate, up, SILU(gate), MUL, down, ADD(x, down) — kept in HBM between nodes, with
MUL_MAT(W, MUL(ACT(g), u)) fused into one gated node when nothing else wants the intermediates.
Every result must hold the bits of the six nodes run one by one on a device allocator."""
import numpy as np
import pytest

from _util import random_acts, random_weights

pytestmark = pytest.mark.gpu

H, F = 256, 512


def _mlp(G, oracle, device, swap_mul=False):
    ga = G.GGMLGraphAllocator(device=device, defaultBufferSize=1 << 20)
    T, Op = G.GGMLType, G.GGMLOp

    def weight(k, m, s):
        t = ga.allocateTensor(T.Q4_0, [k, m])
        ga.setTensorBytes(t, oracle.quantize(2, random_weights(k * m, s, std=1.0 / np.sqrt(k))))
        return t

    def node(op, m, a, b=None):
        d = ga.allocateTensor(T.F32, [1, m])
        d.op, d.src = op, [a, b]
        return d

    x = ga.allocateTensor(T.F32, [1, H])
    ga.setTensorBytes(x, random_acts(H, 21))
    wg, wu, wd = weight(H, F, 22), weight(H, F, 23), weight(F, H, 24)
    g = node(Op.MUL_MAT, F, wg, x)
    u = node(Op.MUL_MAT, F, wu, x)
    t = node(Op.SILU, F, g)
    h = node(Op.MUL, F, u, t) if swap_mul else node(Op.MUL, F, t, u)
    o = node(Op.MUL_MAT, H, wd, h)
    y = node(Op.ADD, H, x, o)
    return ga, [g, u, t, h, o, y]


def _bytes(ga, nodes):
    out = []
    for n in nodes:
        b = ga.tensorBytes(n)
        out.append(bytes(b.cpu().numpy()) if hasattr(b, "cpu") else bytes(b))
    return out


@pytest.fixture(scope="module")
def reference(gpu, oracle):
    """The six nodes one by one on a device allocator (computed once, shared, never changed)."""
    import torch
    import ggml_hip as G
    ga, nodes = _mlp(G, oracle, "cuda")
    g, u, t, h, o, y = nodes
    G.computeMatMul(ga, None, g.src[0], g.src[1], g)
    G.computeMatMul(ga, None, u.src[0], u.src[1], u)
    G.computeSilu(ga, None, g, t)
    G.computeMul(ga, None, t, u, h)
    G.computeMatMul(ga, None, o.src[0], h, o)
    G.computeAdd(ga, None, y.src[0], o, y)
    torch.cuda.synchronize()
    return _bytes(ga, nodes)


def _graph(G, ga, nodes, outputs):
    return G.ResidentGraph(ga, [(n.src[0], n.src[1], n) for n in nodes], outputs=outputs, ops=[n.op for n in nodes])


@pytest.mark.parametrize("swap", [False, True], ids=["mul_t_u", "mul_u_t"])
def test_only_last_node_output_fuses(gpu, oracle, reference, swap):
    import ggml_hip as G
    ga, nodes = _mlp(G, oracle, "host", swap_mul=swap)
    gr = _graph(G, ga, nodes, [False] * 5 + [True])
    assert gr.numFused == 1
    for _ in range(3):  # eager, captured, replayed
        ga.tensorBytes(nodes[-1])[:] = 0xFF
        gr.compute()
        assert bytes(ga.tensorBytes(nodes[-1])) == reference[-1]
    assert gr.transferBytes(False) == 4 * H  # the ADD node's bytes, nothing else comes back
    # the fused intermediates were never written (host bytes still zero)
    assert not np.any(ga.tensorBytes(nodes[2])) and not np.any(ga.tensorBytes(nodes[3]))
    gr.close()


def test_every_node_output_does_not_fuse(gpu, oracle, reference):
    import ggml_hip as G
    ga, nodes = _mlp(G, oracle, "host")
    gr = _graph(G, ga, nodes, [True] * 6)
    assert gr.numFused == 0
    for _ in range(2):
        gr.compute()
        assert _bytes(ga, nodes) == reference
    gr.close()
    gr = _graph(G, ga, nodes, None)  # outputs = None: all
    assert gr.numFused == 0
    gr.compute()
    assert _bytes(ga, nodes) == reference
    gr.close()


def test_intermediate_read_elsewhere_does_not_fuse(gpu, oracle, reference):
    """t = SILU(g) also feeds a second node: it must exist, so nothing is fused."""
    import ggml_hip as G
    ga, nodes = _mlp(G, oracle, "host")
    extra = ga.allocateTensor(G.GGMLType.F32, [1, F])
    extra.op, extra.src = G.GGMLOp.ADD, [nodes[2], nodes[1]]
    allnodes = nodes + [extra]
    gr = _graph(G, ga, allnodes, [False] * 5 + [True, True])
    assert gr.numFused == 0
    gr.compute()
    assert bytes(ga.tensorBytes(nodes[-1])) == reference[-1]
    gr.close()


@pytest.mark.parametrize("whole", [False, True])
def test_backend_graph_compute(gpu, oracle, reference, whole):
    import ggml_hip as G
    ga, nodes = _mlp(G, oracle, "host")
    be = G.GGMLHipBackend(ga, wholeGraphs=whole)
    assert all(be.supportsOp(n) for n in nodes)
    for _ in range(2):
        assert be.graphCompute(G.GGMLCGraph(nodes, ga)) == G.GGMLStatus.SUCCESS
    assert bytes(ga.tensorBytes(nodes[-1])) == reference[-1]
    if not whole:
        assert _bytes(ga, nodes) == reference
    be.free()
    # device allocator: node by node through the per-op calls (gated when whole graphs are passed)
    gd, dn = _mlp(G, oracle, "cuda")
    bd = G.GGMLHipBackend(gd, wholeGraphs=whole)
    G.debugRoute()
    assert bd.graphCompute(G.GGMLCGraph(dn, gd)) == G.GGMLStatus.SUCCESS
    bd.synchronize()
    assert ("stream_gated<" in G.debugRoute()) == whole
    assert _bytes(gd, dn)[-1] == reference[-1]


def test_supports_op_kept_behaviour(gpu, oracle):
    import ggml_hip as G
    ga, nodes = _mlp(G, oracle, "host")
    be = G.GGMLHipBackend(ga)
    T = G.GGMLType
    a16 = G.GGMLTensor(T.F16, [1, 8])
    n16 = G.GGMLTensor(T.F16, [1, 8], op=G.GGMLOp.ADD, src=[a16, a16])
    assert not be.supportsOp(n16)
    mixed = G.GGMLTensor(T.F32, [1, 8], op=G.GGMLOp.MUL, src=[G.GGMLTensor(T.F32, [1, 8]), a16])
    assert not be.supportsOp(mixed)
    assert not be.supportsOp(G.GGMLTensor(T.F32, [1, 8], op=G.GGMLOp.GELU, src=[None, None]))
    sharded = G.GGMLHipBackend(ga, shardDevices=[0])
    try:
        assert not any(sharded.supportsOp(n) for n in nodes if n.op != G.GGMLOp.MUL_MAT)
        assert all(sharded.supportsOp(n) for n in nodes if n.op == G.GGMLOp.MUL_MAT)
    finally:
        sharded.close()
