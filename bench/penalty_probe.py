"""penalty_apply (csrc/kernels/penalties.hip) at decode shapes: 1, 16, 50 and 64 rows of
V = 128,256 bf16 logits, out of place as the decode graph runs it, every row penalised,
cold (each call reads other logits and other table rows; 768 MB in rotation).  The
yardstick is bw_probe's plain streaming read of the same byte count -- 6 B per element:
2 B logits + 2 B table read, 2 B written -- in the same run; the aim is within 2x of it
(a third of the traffic is stores, and at 0.8-50 MB the kernel is all launch ramp)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bw_probe import read_time  # noqa: E402
from gemm_sweep import graph_time  # noqa: E402

from fasttalk_llm_microservice_amd import ops  # noqa: E402

V = 128256
SLOTS = 256


def main():
    dev = "cuda"
    torch.manual_seed(0)
    table, bias_ids, bias_vals = ops.penalty_state(SLOTS, V, dev)
    # a realistic row: ~600 prompt tokens, ~200 generated ones, 8 biased tokens
    for s in range(SLOTS):
        cols = torch.randint(0, V, (800,), device=dev)
        table[s, cols[:600]] = -32768   # bit 15
        table[s, cols[600:]] = 2
        bias_ids[s, :8] = torch.randint(0, V, (8,), device=dev, dtype=torch.int32)
    bias_vals.uniform_(-5, 5)
    for rows in (1, 16, 50, 64):
        nbytes = 6 * rows * V
        ncopy = max(2, min(64, (768 << 20) // (2 * rows * V)))
        logits = [torch.randn(rows, V, device=dev).bfloat16() for _ in range(ncopy)]
        out = torch.empty(rows, V, device=dev, dtype=torch.bfloat16)
        nslot = SLOTS // rows
        slots = [(torch.arange(rows, device=dev, dtype=torch.int32) + rows * (i % nslot))
                 for i in range(ncopy)]
        rep = torch.full((rows,), 1.3, device=dev)
        pres = torch.full((rows,), 0.5, device=dev)
        freq = torch.full((rows,), 1.0, device=dev)
        calls = 24
        t = graph_time([lambda i=i: ops.penalty_apply(
            logits[i % ncopy], slots[i % ncopy], rep, pres, freq, table, bias_ids, bias_vals, out=out)
            for i in range(calls)])
        del logits
        torch.cuda.empty_cache()
        t_read = read_time(nbytes, calls)
        print(f"rows {rows:3d}: penalty_apply {t:7.2f} us ({nbytes / t / 1e3:5.0f} GB/s of 6 B/elem)   "
              f"plain read of {nbytes / 1e6:5.1f} MB {t_read:7.2f} us ({nbytes / t_read / 1e3:5.0f} GB/s)   "
              f"ratio {t / t_read:4.2f}", flush=True)


if __name__ == "__main__":
    main()
