"""ops.logprobs (csrc/kernels/logprobs.hip) at decode shapes: 1, 16, 50 and 64 rows of
V = 128,256 bf16 logits, every row wanting 20 alternatives, cold (each call reads other
logits; 768 MB in rotation).  Yardsticks in the same run: bw_probe's plain streaming read
of the same bytes (2 B per element), and torch.log_softmax + torch.topk(20) on the same
logits -- what the op would cost without a kernel of its own."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bw_probe import read_time  # noqa: E402
from gemm_sweep import graph_time  # noqa: E402

from fasttalk_llm_microservice_amd import ops  # noqa: E402

V = 128256


def main():
    dev = "cuda"
    torch.manual_seed(0)
    for rows in (1, 16, 50, 64):
        nbytes = 2 * rows * V
        ncopy = max(2, min(64, (768 << 20) // nbytes))
        logits = [torch.randn(rows, V, device=dev).bfloat16() for _ in range(ncopy)]
        sampled = torch.randint(0, V, (rows,), device=dev, dtype=torch.int32)
        want = torch.full((rows,), ops.LOGPROBS_MAX, device=dev, dtype=torch.int32)
        out_lp = torch.zeros(rows, 1 + ops.LOGPROBS_MAX, device=dev)
        out_id = torch.zeros(rows, 1 + ops.LOGPROBS_MAX, device=dev, dtype=torch.int32)
        calls = 24
        t = graph_time([lambda i=i: ops.logprobs(logits[i % ncopy], sampled, want, out_lp, out_id)
                        for i in range(calls)])
        t_torch = graph_time([lambda i=i: torch.topk(torch.log_softmax(logits[i % ncopy].float(), dim=-1),
                                                     ops.LOGPROBS_MAX, dim=-1) for i in range(calls)])
        del logits
        torch.cuda.empty_cache()
        t_read = read_time(nbytes, calls)
        print(f"rows {rows:3d}: logprobs {t:7.2f} us ({nbytes / t / 1e3:5.0f} GB/s of 2 B/elem)   "
              f"plain read of {nbytes / 1e6:5.1f} MB {t_read:7.2f} us   ratio {t / t_read:5.2f}   "
              f"log_softmax + topk {t_torch:8.2f} us ({t_torch / t:5.1f}x)", flush=True)


if __name__ == "__main__":
    main()
