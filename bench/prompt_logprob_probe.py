"""ops.prompt_logprobs (csrc/kernels/logprobs.hip, ft_prompt_logprobs) at prefill shapes:
64, 256 and 512 rows of V = 128,256 bf16 logits, every row wanting 0 or 20 alternatives,
cold (each call reads other logits; 768 MB in rotation).  Yardsticks in the same run:
ops.logprobs on the same rows (the difference is what the rank count costs), and
torch.log_softmax + gather + topk(20) on the same logits -- what the op would cost
without a kernel of its own (it computes no rank)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gemm_sweep import graph_time  # noqa: E402

from fasttalk_llm_microservice_amd import ops  # noqa: E402

V = 128256


def main():
    dev = "cuda"
    torch.manual_seed(0)
    cols = 1 + ops.LOGPROBS_MAX
    for rows in (64, 256, 512):
        nbytes = 2 * rows * V
        ncopy = max(2, min(64, (768 << 20) // nbytes))
        logits = [torch.randn(rows, V, device=dev).bfloat16() for _ in range(ncopy)]
        targets = torch.randint(0, V, (rows,), device=dev, dtype=torch.int32)
        tl = targets.long().view(-1, 1)
        out_lp = torch.zeros(rows, cols, device=dev)
        out_id = torch.zeros(rows, cols, device=dev, dtype=torch.int32)
        out_rank = torch.zeros(rows, device=dev, dtype=torch.int32)
        calls = 12
        for k in (0, ops.LOGPROBS_MAX):
            want = torch.full((rows,), k, device=dev, dtype=torch.int32)
            t = graph_time([lambda i=i: ops.prompt_logprobs(logits[i % ncopy], targets, want, out_lp,
                                                            out_id, out_rank) for i in range(calls)])
            t_lp = graph_time([lambda i=i: ops.logprobs(logits[i % ncopy], targets, want, out_lp, out_id)
                               for i in range(calls)])

            def torch_way(i):
                lp = torch.log_softmax(logits[i % ncopy].float(), dim=-1)
                lp.gather(1, tl)
                if k:
                    torch.topk(lp, k, dim=-1)

            t_torch = graph_time([lambda i=i: torch_way(i) for i in range(calls)])
            print(f"rows {rows:3d} want {k:2d}: prompt_logprobs {t:8.2f} us ({nbytes / t / 1e3:5.0f} GB/s "
                  f"of 2 B/elem)   logprobs {t_lp:8.2f} us   rank count {t - t_lp:+7.2f} us "
                  f"({100 * (t - t_lp) / t_lp:+5.1f}%)   log_softmax + gather + topk {t_torch:9.2f} us "
                  f"({t_torch / t:5.1f}x)", flush=True)
        del logits
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
