"""min_p in the sampler at the serving shape ([rows, 128256] bf16 logits): top-p and
top-k sampling with min_p off (no ln(min_p) array: the launches of the sampler without
min_p) and with min_p = 0.05 on every row.  hipGraph of 100 calls, each on its own decode
step, as bench/sampler_probe.py; every configuration is timed --repeats times (the spread
is printed).  On a build whose sampler has no min_p only the "off" columns are measured.

python bench/min_p_probe.py [--rows 1,16,50,64] [--repeats 3]
python bench/min_p_probe.py --eager 20 --rows 50 --configs top_p
    (no graph: for a kernel trace, which shows samp_minp_kernel next to
    samp_stats_kernel, the pass it should cost)
"""
import argparse
import inspect
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from fasttalk_llm_microservice_amd import ops  # noqa: E402

HAS_MIN_P = "min_p" in inspect.signature(ops.sample).parameters
N_CALLS = 100


def timed(call, repeats):
    call(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(N_CALLS):
            call(i)
    g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(2):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / (2 * N_CALLS))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1,16,50,64")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--min-p", type=float, default=0.05)
    ap.add_argument("--eager", type=int, default=0, help="calls per configuration, no graph")
    ap.add_argument("--configs", default="top_p,top_k")
    a = ap.parse_args()
    v, dev = 128256, "cuda"
    print(f"min_p_probe: sampler {'with' if HAS_MIN_P else 'without'} min_p, V={v} bf16, "
          f"us per call (min / median / max of {a.repeats})", flush=True)
    for b in (int(x) for x in a.rows.split(",")):
        torch.manual_seed(0)
        logits = (torch.randn(b, v, device=dev) * 2).bfloat16()
        seeds = torch.arange(b, dtype=torch.int64, device=dev)
        steps = torch.arange(N_CALLS, dtype=torch.int32, device=dev)[:, None].repeat(1, b).contiguous()
        tt = torch.full((b,), 0.7, device=dev)
        lnmp = torch.full((b,), math.log(a.min_p), device=dev)
        for name, p, k in (("top_p 0.9", 0.9, 0), ("top_k 40", 1.0, 40)):
            if name.split()[0] not in a.configs.split(","):
                continue
            pp = torch.full((b,), p, device=dev)
            kk = torch.full((b,), k, dtype=torch.int32, device=dev)
            modes = [("off", None)] + ([("min_p", lnmp)] if HAS_MIN_P else [])
            res = {}
            for mode, mp in modes:
                kw = {} if mp is None else {"min_p": mp}

                def call(i, kw=kw):
                    ops.sample(logits, tt, pp, kk, seeds, steps[i], **kw)

                if a.eager:
                    for i in range(a.eager):
                        call(i)
                    torch.cuda.synchronize()
                    continue
                t = sorted(timed(call, a.repeats))
                res[mode] = t
                print(f"rows={b:3d} {name:10s} {mode:6s}: {t[0]:7.2f} / {t[len(t) // 2]:7.2f} / "
                      f"{t[-1]:7.2f} us", flush=True)
            if "min_p" in res:
                d = res["min_p"][len(res["min_p"]) // 2] - res["off"][len(res["off"]) // 2]
                print(f"rows={b:3d} {name:10s} added by min_p: {d:+.2f} us", flush=True)


if __name__ == "__main__":
    main()
