"""W4A16 GEMM on the int4 image (w4_packed_gemm.hip) vs packed_gemm.hip on the
dequantized bf16 image of the same weight, at Llama-3-8B / 70B projection shapes and
mixed-step / prefill row counts.  Both run the model's plan (models/llama.py
W4PG_PLAN / PG_PLAN: tile cfg, split-K; slab variants are timed with a slab_store
pass, gate_up at one split through the SiLU epilogue).  Weights are cold: a 512 MB
buffer is rewritten before every timed call, and the two kernels alternate order
from one iteration to the next.  --sweep also times every (cfg, splits) of the W4
kernel and prints the best, for tuning W4PG_PLAN.

python bench/w4pg_probe.py [--models 8b,70b] [--rows 145,300,512,1024] [--only qkv,gu]
                           [--iters 8] [--sweep]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from fasttalk_llm_microservice_amd import ops  # noqa: E402
from fasttalk_llm_microservice_amd.models.llama import pg_cfg, w4pg_cfg  # noqa: E402
from fasttalk_llm_microservice_amd.ops import quant as Q  # noqa: E402

SHAPES = {
    "8b": {"qkv": (6144, 4096), "o": (4096, 4096), "gu": (28672, 4096), "down": (4096, 14336)},
    "70b": {"qkv": (10240, 8192), "o": (8192, 8192), "gu": (57344, 8192), "down": (8192, 28672)},
}


def timed(fn, flush):
    flush()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="8b,70b")
    ap.add_argument("--rows", default="145,300,512,1024")
    ap.add_argument("--only", default="")
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(0)
    cold = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    flush = lambda: cold.fill_(1)  # noqa: E731
    ws = torch.empty(96 << 20, device="cuda")
    print("model proj   rows |  w4pg cfg/sp     us |  pg cfg/sp       us | ratio | max err")
    for model in a.models.split(","):
        for proj, (n, k) in SHAPES[model].items():
            if a.only and proj not in a.only.split(","):
                continue
            w = torch.randn(n, k, device="cuda") * 0.05
            if proj == "gu":
                w = ops.interleave_gate_up(w, 1)
            q, z, s = Q.quantize_w4(w)
            del w
            W = Q.pack_w4(q, z, s)
            del q, z, s
            wp = ops.pack_weight(Q.w4_dequant(W))
            torch.cuda.empty_cache()
            cols = n // 2 if proj == "gu" else n
            for m in [int(v) for v in a.rows.split(",")]:
                x = torch.randn(m, k, device="cuda").bfloat16()
                out_a = torch.empty(m, cols, device="cuda").bfloat16()
                out_b = torch.empty(m, cols, device="cuda").bfloat16()

                def w4(cfg, sp, out=out_a):
                    if sp > 1:
                        Q.w4_packed_gemm(x, W, ws=ws, splits=sp, epi="slab", cfg=cfg)
                        if proj == "gu":
                            ops.slab_silu(ws, sp, m, cols, out, interleaved=True)
                        else:
                            ops.slab_store(ws, sp, m, n, out)
                    else:
                        Q.w4_packed_gemm(x, W, out=out, epi="silu" if proj == "gu" else "store",
                                         cfg=cfg)

                def pg(cfg, sp, out=out_b):
                    if sp > 1:
                        ops.packed_gemm(x, wp, ws=ws, splits=sp, epi="slab", cfg=cfg)
                        if proj == "gu":
                            ops.slab_silu(ws, sp, m, cols, out, interleaved=True)
                        else:
                            ops.slab_store(ws, sp, m, n, out)
                    else:
                        ops.packed_gemm(x, wp, out=out, epi="silu" if proj == "gu" else "store",
                                        cfg=cfg)

                c4, s4 = w4pg_cfg(proj, m, n, k, ws.numel())
                cp, spp = pg_cfg(proj, m, k)
                if spp > 1 and spp * m * n > ws.numel():
                    spp = 1
                fa = lambda: w4(c4, s4)  # noqa: E731
                fb = lambda: pg(cp, spp)  # noqa: E731
                fa(), fb()
                torch.cuda.synchronize()
                err = (out_a.float() - out_b.float()).abs().max().item()
                ta, tb = [], []
                for it in range(a.iters):
                    if it % 2 == 0:
                        ta.append(timed(fa, flush))
                        tb.append(timed(fb, flush))
                    else:
                        tb.append(timed(fb, flush))
                        ta.append(timed(fa, flush))
                ua, ub = statistics.median(ta), statistics.median(tb)
                line = (f"{model:4s} {proj:5s} {m:5d} |  {c4}/{s4:<2d}      {ua:8.1f} |  {cp}/{spp:<2d}"
                        f"      {ub:8.1f} | {ua / ub:5.2f} | {err:.3f}")
                if a.sweep:
                    best = None
                    for cfg in (0, 1, 2):
                        for sp in (1, 2, 4, 8, 16):
                            if k % (128 * sp) or sp * m * n > ws.numel():
                                continue
                            f = lambda cfg=cfg, sp=sp: w4(cfg, sp)  # noqa: E731
                            f()
                            us = statistics.median(timed(f, flush) for _ in range(max(3, a.iters // 2)))
                            if best is None or us < best[0]:
                                best = (us, cfg, sp)
                    line += f" | best {best[1]}/{best[2]} {best[0]:.1f} ({best[0] / ub:.2f})"
                print(line, flush=True)
            del W, wp
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
