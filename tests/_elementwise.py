"""numpy restatement of the F32 element-wise arithmetic the backend offloads (test infrastructure).

  ADD   computeAdd   core/GGMLComputeOps.kt:735-759    a + b
  MUL   computeMul   :811 ff.                          a * b
  GELU  computeGelu  :1581-1594   x*0.5f*(1.0f+tanh(0.797885f*(x+0.044715f*x*x*x)))
  SILU  as a graph node: computeSilu (:2633-2638) calls computeGelu, so it is GELU
  Act.SILU (explicit API only, the reference's TODO)   x / (1.0f + exp(-x))

Every product, sum and quotient is rounded to float32 on its own, in the Kotlin order. tanh and exp
are evaluated in float64 on the float32 argument and rounded once: the correctly rounded value a
float32 libm approximates.
"""
import numpy as np

f32 = np.float32
ULP24 = 2.0 ** -24


def add_ref(a, b):
    with np.errstate(all="ignore"):
        return (np.asarray(a, f32) + np.asarray(b, f32)).astype(f32)


def mul_ref(a, b):
    with np.errstate(all="ignore"):
        return (np.asarray(a, f32) * np.asarray(b, f32)).astype(f32)


def gelu_ref(x):
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):
        c = ((f32(0.044715) * x) * x) * x
        arg = f32(0.797885) * (x + c)
        t = np.tanh(arg.astype(np.float64)).astype(f32)
        return ((x * f32(0.5)) * (f32(1.0) + t)).astype(f32)


def silu_ref(x):
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):
        e = np.exp((-x).astype(np.float64)).astype(f32)
        return (x / (f32(1.0) + e)).astype(f32)


def act_ref(act, x):
    return gelu_ref(x) if act == 1 else silu_ref(x)


def gelu_f64(x):
    """The same expression in float64 throughout (how far the float32 steps are from exact)."""
    x = np.asarray(x, f32).astype(np.float64)
    return x * 0.5 * (1.0 + np.tanh(np.float64(f32(0.797885)) * (x + np.float64(f32(0.044715)) * x * x * x)))


def silu_f64(x):
    x = np.asarray(x, f32).astype(np.float64)
    return x / (1.0 + np.exp(-x))


def tight_units(got, ref, x):
    """max |got - ref| / (2^-24 * |x|) over the points with x != 0."""
    got, ref, x = (np.asarray(v, np.float64) for v in (got, ref, x))
    m = x != 0
    return float(np.max(np.abs(got[m] - ref[m]) / (ULP24 * np.abs(x[m])))) if m.any() else 0.0


def floor_share(ref, rel=1e-3):
    """Share of points under the F32 bar's absolute floor rel * ||ref||_inf (tests/_util.parity_ok)."""
    r = np.abs(np.asarray(ref, np.float64))
    return float(np.mean(r < rel * r.max()))


SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.1754942e-38, -5.877472e-39,
                     3.4e38, -3.4e38, 1.0, -1.0], dtype=f32)


def values(n, seed):
    """n float32 values: normal draws with the special values (±0, ±Inf, NaN, denormals, ±3.4e38) mixed in."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n).astype(f32)
    k = min(n, SPECIALS.size)
    pos = rng.permutation(n)[:k]
    v[pos] = rng.permutation(SPECIALS)[:k]
    return v


def same_bits(got, ref):
    """Bit-identical where ref is a number; NaN exactly where ref is NaN."""
    got, ref = np.asarray(got, f32).reshape(-1), np.asarray(ref, f32).reshape(-1)
    nan = np.isnan(ref)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), ref[~nan].view(np.uint32)))
