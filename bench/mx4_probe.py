"""MXFP4 (W4A16) GEMMs against the W8A16 (fp8) kernels and the bf16 kernels the plans
select for the same shape, and against a plain streaming read of the MXFP4 image's
bytes, at Llama-3-8B / 70B projection shapes, all in one run.

* rows <= 64: mx4a16.hip per MX4_PLAN vs w8a16.hip per W8_PLAN vs skinny_gemm.hip per
  PACKED_PLAN;
* rows  > 64: mx4_packed_gemm.hip per MX4PG_PLAN vs w8_packed_gemm.hip per W8PG_PLAN vs
  packed_gemm.hip per PG_PLAN.

Every side runs what the model runs: split-K variants are timed with their slab_store
(gate_up: slab_silu) pass, unsplit gate_up through the SiLU epilogue.  Weights are cold:
every call of a hipGraph of N calls reads another copy of the image, the copies spanning
more than 768 MiB (bench/bw_read.py's method), and the three graphs alternate (each is
timed twice, in two orders; the minimum is printed).  The streaming-read column needs
bench/libbwk.so (see bench/bw_read.py); without it the column says so.  --sweep also
times every (nt, splits) / (cfg, splits) of the MXFP4 kernels and prints the best, for
picking MX4_PLAN / MX4PG_PLAN.

python bench/mx4_probe.py [--models 8b,70b] [--rows 1,16,50,64,145,300,512,1024]
                          [--only qkv,gu] [--reps 5] [--sweep]
"""
from __future__ import annotations

import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import torch  # noqa: E402

from gemm_sweep import graph_time  # noqa: E402
from w8_probe import COLD_BYTES, SHAPES, _bw_lib, stream_read_us  # noqa: E402

from fasttalk_llm_microservice_amd import ops  # noqa: E402
from fasttalk_llm_microservice_amd.models.llama import (mx4_cfg, mx4pg_cfg, packed_cfg,  # noqa: E402
                                                        pg_cfg, w8_cfg, w8pg_cfg)
from fasttalk_llm_microservice_amd.ops import quant as Q  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="8b")
    ap.add_argument("--rows", default="1,16,50,64,145,300,512,1024")
    ap.add_argument("--only", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mx4_probe needs the GPU: nothing is measured without one")
    torch.manual_seed(0)
    lib = _bw_lib()
    sink = torch.empty(4096 * 256, dtype=torch.int32, device="cuda")
    ws = torch.empty(96 << 20, device="cuda")
    rows_list = [int(v) for v in a.rows.split(",")]
    print("model proj   rows | mxfp4 plan      us |  fp8 plan        us | bf16 plan            us | "
          "mx4/fp8 mx4/bf16 | read of mxfp4 image us (mx4/read)")
    for model in a.models.split(","):
        for proj, (n, k) in SHAPES[model].items():
            if a.only and proj not in a.only.split(","):
                continue
            gu = proj == "gu"
            w = (torch.randn(n, k, device="cuda") * 0.02).bfloat16()
            X0 = Q.pack_mx4(*Q.quantize_mx4(w), gate_up=gu)
            W0 = Q.pack_w8(*Q.quantize_w8(w), gate_up=gu)
            wp0 = ops.pack_weight(ops.interleave_gate_up(w, 1) if gu else w)
            del w
            img = X0.nbytes()
            n4 = max(2, min(24, COLD_BYTES // img + 1))
            n8 = max(2, min(24, COLD_BYTES // (n * k) + 1))
            n16 = max(2, min(24, COLD_BYTES // (2 * n * k) + 1))
            X4 = [Q.MX4Weight(X0.wq.clone(), X0.sc.clone(), n, k) for _ in range(n4)]
            W8 = [Q.W8Weight(W0.wq.clone(), W0.scale.clone(), n, k) for _ in range(n8)]
            W16 = [wp0.clone() for _ in range(n16)]
            # the image and its scale bytes as one buffer per copy, for the streaming read
            R4 = [torch.cat([X.wq, X.sc]) for X in X4] if lib else []
            del X0, W0, wp0
            torch.cuda.empty_cache()
            read_us = stream_read_us(lib, R4, img, sink, a.reps) if lib else None
            del R4
            cols = n // 2 if gu else n
            for m in rows_list:
                x = torch.randn(m, k, device="cuda").bfloat16()
                out = torch.empty(m, cols, device="cuda").bfloat16()

                def tail(sp):
                    if gu:
                        ops.slab_silu(ws, sp, m, cols, out, interleaved=True)
                    else:
                        ops.slab_store(ws, sp, m, n, out)

                def quant(gemm, pgemm):
                    def run(W, c, sp):
                        if m <= 64:
                            if sp > 1:
                                gemm(x, W, ws=ws, splits=sp, nt=c)
                                tail(sp)
                            else:
                                gemm(x, W, out=out, nt=2 if gu else c, silu=gu)
                        elif sp > 1:
                            pgemm(x, W, ws=ws, splits=sp, epi="slab", cfg=c)
                            tail(sp)
                        else:
                            pgemm(x, W, out=out, epi="silu" if gu else "store", cfg=c)
                    return run

                mx4 = quant(Q.mx4_gemm, Q.mx4_packed_gemm)
                fp8 = quant(Q.w8_gemm, Q.w8_packed_gemm)

                def bf16(wp, c, sp):
                    if m <= 64:
                        nt, u = c
                        if sp > 1:
                            ops.skinny_gemm(x, wp, ws=ws, splits=sp, nt=nt, u=u)
                            tail(sp)
                        elif u in (-6, -8):
                            ops.skinny_gemm(x, wp, out=out, splits=1, nt=nt, u=u)
                        else:
                            y = ops.skinny_gemm(x, wp, splits=1, nt=nt, u=u)
                            if gu:
                                ops.silu_mul(y, out=out, interleaved=True)
                    elif sp > 1:
                        ops.packed_gemm(x, wp, ws=ws, splits=sp, epi="slab", cfg=c)
                        tail(sp)
                    else:
                        ops.packed_gemm(x, wp, out=out, epi="silu" if gu else "store", cfg=c)

                if m <= 64:
                    c4, s4 = mx4_cfg(proj, m, n, k)
                    c8, s8 = w8_cfg(proj, m, n, k)
                    nt, u, s16 = packed_cfg(proj, m, n, k)
                    c16 = (nt, u)
                else:
                    c4, s4 = mx4pg_cfg(proj, m, n, k, ws.numel())
                    c8, s8 = w8pg_cfg(proj, m, n, k, ws.numel())
                    c16, s16 = pg_cfg(proj, m, k)
                    if s16 > 1 and s16 * m * n > ws.numel():
                        s16 = 1
                graphs = {
                    "mx4": [lambda W=W: mx4(W, c4, s4) for W in X4],
                    "fp8": [lambda W=W: fp8(W, c8, s8) for W in W8],
                    "bf16": [lambda wp=wp: bf16(wp, c16, s16) for wp in W16],
                }
                times = {name: [] for name in graphs}
                for order in (("mx4", "fp8", "bf16"), ("bf16", "fp8", "mx4")):   # alternate
                    for name in order:
                        times[name].append(graph_time(graphs[name], a.reps))
                u4, u8, u16 = (min(times[name]) for name in ("mx4", "fp8", "bf16"))
                line = (f"{model:4s} {proj:5s} {m:5d} |  {str(c4):>2s}/{s4:<2d}      {u4:8.1f} | "
                        f" {str(c8):>2s}/{s8:<2d}      {u8:8.1f} | {str(c16):>9s}/{s16:<2d} {u16:8.1f} | "
                        f"  {u4 / u8:5.2f}   {u4 / u16:5.2f}  | ")
                line += f"{read_us:8.1f} ({u4 / read_us:.2f})" if read_us else "not measured (no libbwk.so)"
                if a.sweep:
                    best = None
                    cands = [(nt_, sp) for nt_ in Q.MX4_NTS for sp in (1, 2, 4, 8)] if m <= 64 else \
                        [(0, sp) for sp in (1, 2, 4, 8, 16)]
                    for c, sp in cands:
                        if k % ((256 if m <= 64 else 128) * sp) or sp * m * n > ws.numel():
                            continue
                        if gu and m <= 64 and sp == 1 and c != 2:
                            continue
                        t = graph_time([lambda W=W, c=c, sp=sp: mx4(W, c, sp) for W in X4], a.reps)
                        if best is None or t < best[0]:
                            best = (t, c, sp)
                    line += f" | best {best[1]}/{best[2]} {best[0]:.1f} ({best[0] / u8:.2f} of fp8)"
                print(line, flush=True)
            del X4, W8, W16
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
