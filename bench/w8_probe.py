"""W8A16 (fp8 e4m3 weights) GEMMs against the bf16 kernels the plan selects for the same
shape, and against a plain streaming read of the fp8 image's bytes, at Llama-3-8B / 70B
projection shapes.

* rows <= 64: w8a16.hip per W8_PLAN vs skinny_gemm.hip per PACKED_PLAN;
* rows  > 64: w8_packed_gemm.hip per W8PG_PLAN vs packed_gemm.hip per PG_PLAN.

Both sides run what the model runs: split-K variants are timed with their slab_store
(gate_up: slab_silu) pass, unsplit gate_up through the SiLU epilogue.  Weights are cold:
every call of a hipGraph of N calls reads another copy of the image, the copies spanning
more than 768 MiB (bench/bw_read.py's method), and the fp8 and bf16 graphs alternate.
The streaming-read column needs bench/libbwk.so (see bench/bw_read.py); without it the
column says so.  --sweep also times every (nt, splits) / (cfg, splits) of the fp8
kernels and prints the best, for picking W8_PLAN / W8PG_PLAN.

python bench/w8_probe.py [--models 8b,70b] [--rows 1,16,50,64,145,300,512,1024]
                         [--only qkv,gu] [--reps 5] [--sweep]
"""
from __future__ import annotations

import argparse
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import torch  # noqa: E402

from gemm_sweep import graph_time  # noqa: E402

from fasttalk_llm_microservice_amd import ops  # noqa: E402
from fasttalk_llm_microservice_amd.models.llama import (packed_cfg, pg_cfg, w8_cfg,  # noqa: E402
                                                        w8pg_cfg)
from fasttalk_llm_microservice_amd.ops import quant as Q  # noqa: E402

SHAPES = {
    "8b": {"qkv": (6144, 4096), "o": (4096, 4096), "gu": (28672, 4096), "down": (4096, 14336)},
    "70b": {"qkv": (10240, 8192), "o": (8192, 8192), "gu": (57344, 8192), "down": (8192, 28672)},
}
COLD_BYTES = 768 << 20


def _bw_lib():
    path = os.path.join(HERE, "libbwk.so")
    if not os.path.exists(path):
        return None
    lib = ctypes.CDLL(path)
    lib.bw_read.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int,
                            ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return lib


def stream_read_us(lib, bufs, nbytes, sink, reps):
    """Best time of a plain read of ``nbytes`` over a few grid sizes / loads in flight."""
    best = None
    for blocks in (512, 1024, 2048):
        for unroll in (4, 8):
            calls = [lambda b=b: lib.bw_read(b.data_ptr(), nbytes, sink.data_ptr(), blocks, unroll, 0,
                                             torch.cuda.current_stream().cuda_stream) for b in bufs]
            t = graph_time(calls, reps)
            best = t if best is None else min(best, t)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="8b")
    ap.add_argument("--rows", default="1,16,50,64,145,300,512,1024")
    ap.add_argument("--only", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("w8_probe needs the GPU: nothing is measured without one")
    torch.manual_seed(0)
    lib = _bw_lib()
    sink = torch.empty(4096 * 256, dtype=torch.int32, device="cuda")
    ws = torch.empty(96 << 20, device="cuda")
    rows_list = [int(v) for v in a.rows.split(",")]
    print("model proj   rows |  fp8 plan        us | bf16 plan            us | fp8/bf16 | "
          "read of fp8 image us (fp8/read)")
    for model in a.models.split(","):
        for proj, (n, k) in SHAPES[model].items():
            if a.only and proj not in a.only.split(","):
                continue
            gu = proj == "gu"
            w = (torch.randn(n, k, device="cuda") * 0.02).bfloat16()
            q, s = Q.quantize_w8(w)
            W0 = Q.pack_w8(q, s, gate_up=gu)
            wp0 = ops.pack_weight(ops.interleave_gate_up(w, 1) if gu else w)
            del w, q, s
            n8 = max(2, min(24, COLD_BYTES // (n * k) + 1))
            n16 = max(2, min(24, COLD_BYTES // (2 * n * k) + 1))
            W8 = [Q.W8Weight(W0.wq.clone(), W0.scale.clone(), n, k) for _ in range(n8)]
            W16 = [wp0.clone() for _ in range(n16)]
            del W0, wp0
            torch.cuda.empty_cache()
            read_us = stream_read_us(lib, [W.wq for W in W8], n * k, sink, a.reps) if lib else None
            cols = n // 2 if gu else n
            for m in rows_list:
                x = torch.randn(m, k, device="cuda").bfloat16()
                out = torch.empty(m, cols, device="cuda").bfloat16()

                def tail(sp):
                    if gu:
                        ops.slab_silu(ws, sp, m, cols, out, interleaved=True)
                    else:
                        ops.slab_store(ws, sp, m, n, out)

                def fp8(W, c, sp):
                    if m <= 64:
                        if sp > 1:
                            Q.w8_gemm(x, W, ws=ws, splits=sp, nt=c)
                            tail(sp)
                        else:
                            Q.w8_gemm(x, W, out=out, nt=2 if gu else c, silu=gu)
                    elif sp > 1:
                        Q.w8_packed_gemm(x, W, ws=ws, splits=sp, epi="slab", cfg=c)
                        tail(sp)
                    else:
                        Q.w8_packed_gemm(x, W, out=out, epi="silu" if gu else "store", cfg=c)

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
                    c8, s8 = w8_cfg(proj, m, n, k)
                    nt, u, s16 = packed_cfg(proj, m, n, k)
                    c16 = (nt, u)
                else:
                    c8, s8 = w8pg_cfg(proj, m, n, k, ws.numel())
                    c16, s16 = pg_cfg(proj, m, k)
                    if s16 > 1 and s16 * m * n > ws.numel():
                        s16 = 1
                calls8 = [lambda W=W: fp8(W, c8, s8) for W in W8]
                calls16 = [lambda wp=wp: bf16(wp, c16, s16) for wp in W16]
                t8, t16 = [], []
                for it in range(2):        # alternate the two builds of the graph
                    first, second = (calls8, calls16) if it == 0 else (calls16, calls8)
                    ta, tb = graph_time(first, a.reps), graph_time(second, a.reps)
                    t8.append(ta if it == 0 else tb)
                    t16.append(tb if it == 0 else ta)
                u8, u16 = min(t8), min(t16)
                line = (f"{model:4s} {proj:5s} {m:5d} |  {str(c8):>2s}/{s8:<2d}      {u8:8.1f} | "
                        f"{str(c16):>9s}/{s16:<2d} {u16:8.1f} |   {u8 / u16:5.2f}  | ")
                line += f"{read_us:8.1f} ({u8 / read_us:.2f})" if read_us else "not measured (no libbwk.so)"
                if a.sweep:
                    best = None
                    cands = [(nt_, sp) for nt_ in Q.W8_NTS for sp in (1, 2, 4, 8)] if m <= 64 else \
                        [(0, sp) for sp in (1, 2, 4, 8, 16)]
                    for c, sp in cands:
                        if k % ((256 if m <= 64 else 64) * sp) or sp * m * n > ws.numel():
                            continue
                        if gu and m <= 64 and sp == 1 and c != 2:
                            continue
                        t = graph_time([lambda W=W, c=c, sp=sp: fp8(W, c, sp) for W in W8], a.reps)
                        if best is None or t < best[0]:
                            best = (t, c, sp)
                    line += f" | best {best[1]}/{best[2]} {best[0]:.1f} ({best[0] / u16:.2f} of bf16)"
                print(line, flush=True)
            del W8, W16
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
