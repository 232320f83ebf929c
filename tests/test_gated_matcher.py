"""GGMLHipBackend's device-allocator matcher for MUL_MAT(W, MUL(ACT(g), u)) (no GPU needed): it
applies the conditions of lk_graph_create_ops' fusion pass, on byte ranges."""
import ggml_hip as G
from ggml_hip.backend import matchGated

T, Op = G.GGMLType, G.GGMLOp
F, H = 8, 64


def f32(n, off, op=Op.NONE, src=None, flags=0):
    return G.GGMLTensor(T.F32, [1, n], bufferId=0, dataOffset=off, op=op, src=src, flags=flags)


def mlp(swap=False):
    x = f32(H, 0)
    wg, wu = (G.GGMLTensor(T.Q4_0, [H, F], bufferId=b) for b in (1, 2))
    wd = G.GGMLTensor(T.Q4_0, [F, H], bufferId=3)
    g = f32(F, 1000, Op.MUL_MAT, [wg, x])
    u = f32(F, 2000, Op.MUL_MAT, [wu, x])
    t = f32(F, 3000, Op.SILU, [g, None])
    h = f32(F, 4000, Op.MUL, [u, t] if swap else [t, u])
    o = f32(H, 5000, Op.MUL_MAT, [wd, h])
    return x, g, u, t, h, o


def test_matches_the_pattern_either_operand_order():
    for swap in (False, True):
        x, g, u, t, h, o = mlp(swap)
        m = matchGated([g, u, t, h, o], 4)
        assert m is not None and m[:2] == (2, 3) and m[2] is g and m[3] is u
        assert matchGated([g, u, t, h, o], 0) is None


def test_refuses_when_an_intermediate_is_wanted_or_touched():
    x, g, u, t, h, o = mlp()
    extra = f32(F, 6000, Op.ADD, [t, u])                      # another reader of t
    assert matchGated([g, u, t, h, extra, o], 5) is None
    x, g, u, t, h, o = mlp()
    clobber = f32(F, 4000, Op.GELU, [u, None])                 # another writer of h's bytes
    assert matchGated([g, u, t, h, clobber, o], 5) is None
    x, g, u, t, h, o = mlp()
    t.flags = 1  # GGML_TENSOR_FLAG_OUTPUT
    assert matchGated([g, u, t, h, o], 4) is None


def test_refuses_when_gate_or_up_is_rewritten_in_between():
    x, g, u, t, h, o = mlp()
    inplace_u = f32(F, 2000, Op.ADD, [u, g])                   # u += g, in place, after t was taken
    assert matchGated([g, u, t, inplace_u, h, o], 5) is None
    x, g, u, t, h, o = mlp()
    inplace_g = f32(F, 1000, Op.MUL, [g, u])                   # g *= u between the MUL and the MUL_MAT
    assert matchGated([g, u, t, h, inplace_g, o], 5) is None
    x, g, u, t, h, o = mlp()
    before = f32(F, 2000, Op.ADD, [u, g])                      # before the activation: harmless
    assert matchGated([g, u, before, t, h, o], 5) is not None
