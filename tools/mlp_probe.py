"""One Llama-7B MLP at N = 1 (hidden 4096, ffn 11008, Q4_0), timed three ways on the device:

  gated_chain   {gate, up} -> gated down as ONE launch of two stages (lk_plan_create_gated): the down
                stage applies GELU(gate) ⊙ up on its way into the activation image
  four_launch   {gate, up} plan + GELU + MUL + down: four launches, t and h through HBM
  plain_chain   the existing ungated {gate, up} -> down chain (down reads up: what the decode-chain
                benchmark runs), the yardstick for what the gated intake costs

`sets` MLPs with weights of their own are run round-robin so no launch finds its weights in the
Infinity Cache (76 MB of Q4_0 per MLP). Warm-up, then HIP events around `reps` passes over the
sets; the three forms alternate within each of `rounds` rounds and the median round is reported.
One JSON line: microseconds per MLP. Usage: python tools/mlp_probe.py [sets] [reps] [rounds]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "llama.kotlin_amd")]

HIDDEN, FFN = 4096, 11008


def main():
    import torch
    import ggml_hip as G
    sets = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    if not torch.cuda.is_available():
        raise SystemExit("mlp_probe needs a GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    T = G.GGMLType
    ga = G.GGMLGraphAllocator(device=str(dev), defaultBufferSize=16)

    def weight(K, M):
        nbytes = M * K // 32 * 18
        t = G.GGMLTensor(T.Q4_0, [K, M], bufferId=ga.addBuffer(nbytes + 256))
        ga.buffers[t.bufferId][:nbytes].copy_(G.quantizeTensor(torch.randn(M * K, device=dev) * (K ** -0.5), T.Q4_0))
        return t

    def f32(n, fill=False):
        t = G.GGMLTensor(T.F32, [1, n], bufferId=ga.addBuffer(4 * n + 64))
        if fill:
            ga.buffers[t.bufferId][: 4 * n].copy_(torch.randn(n, device=dev).view(torch.uint8))
        return t

    x = f32(HIDDEN, True)
    gated, plain, four, outs = [], [], [], []
    for _ in range(sets):
        wg, wu, wd = weight(HIDDEN, FFN), weight(HIDDEN, FFN), weight(FFN, HIDDEN)
        g, u, t, h = f32(FFN), f32(FFN), f32(FFN), f32(FFN)
        d_gated, d_four, d_plain = f32(HIDDEN), f32(HIDDEN), f32(HIDDEN)
        gated.append(G.MulMatPlan(ga, [(wg, x, g), (wu, x, u), (wd, g, d_gated, u, G.Act.GELU)], stages=[0, 0, 1]))
        plain.append(G.MulMatPlan(ga, [(wg, x, g), (wu, x, u), (wd, u, d_plain)], stages=[0, 0, 1]))
        four.append((G.MulMatPlan(ga, [(wg, x, g), (wu, x, u)]), g, u, t, h, wd, d_four))
        outs.append((d_gated, d_four))
    s = torch.cuda.Stream(device=dev)

    def run_gated():
        for p in gated:
            p.launch(stream=s)

    def run_plain():
        for p in plain:
            p.launch(stream=s)

    def run_four():
        for (p, g, u, t, h, wd, d) in four:
            p.launch(stream=s)
            G.computeGelu(ga, None, g, t, stream=s)
            G.computeMul(ga, None, t, u, h, stream=s)
            G.computeMatMul(ga, None, wd, h, d, stream=s)

    forms = {"gated_chain": run_gated, "four_launch": run_four, "plain_chain": run_plain}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(reps):
            fn()
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps / sets

    for fn in forms.values():  # warm-up: code objects loaded, scratch sized
        fn()
        fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            samples[k].append(timed(fn))
    out = {"sets": sets, "reps": reps, "rounds": rounds}
    for k, v in samples.items():
        out[f"{k}_us"] = round(statistics.median(v), 3)
        out[f"{k}_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
    out["gated_minus_plain_us"] = round(out["gated_chain_us"] - out["plain_chain_us"], 3)
    out["timed_out"] = any(p.timedOut() for p in gated + plain)
    out["gated_equals_four_launch"] = all(bool(torch.equal(ga.tensorBytes(a), ga.tensorBytes(b))) for a, b in outs)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
