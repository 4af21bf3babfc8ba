"""Teacher-forced scoring with the serving engine, in process: the text (or ``--synthetic
N`` seeded token ids) is cut into windows of ``--window`` tokens, each window is sent with
``prompt_logprobs=0, max_tokens=1``, and one JSON line reports the tokens scored, the mean
negative log-likelihood, the perplexity and the share of tokens the model ranked first.

    python bench/score.py --model llama3.1-8b --synthetic 16384 --save bf16.npy
    ENGINE_KV_CACHE_DTYPE=fp8 ENGINE_KV_SCALES=calibrate \\
        python bench/score.py --model llama3.1-8b --synthetic 16384 --compare bf16.npy

``--save`` writes the per-token logprobs, ``--compare`` adds the mean and max |delta
logprob| and the delta of the mean NLL against such a file: the cost of another ENGINE_*
configuration (KV-cache dtype and scales, quantization, batch-invariant plans ...) on the
same weights and seed.  Engine knobs come from the environment (EngineConfig.from_env).
On random-init weights the absolute numbers mean nothing (perplexity ~ the vocabulary
size); the differences between two configurations do."""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from fasttalk_llm_microservice_amd.engine.config import EngineConfig  # noqa: E402
from fasttalk_llm_microservice_amd.engine.engine import LLMEngine  # noqa: E402
from fasttalk_llm_microservice_amd.engine.sampling_params import SamplingParams  # noqa: E402


def windows(ids, size):
    """Consecutive windows of ``size`` tokens (the last one shorter; a 1-token tail has
    nothing to score and is dropped)."""
    return [w for w in (ids[i:i + size] for i in range(0, len(ids), size)) if len(w) > 1]


def score(eng, wins):
    """(logprobs fp32, ranks int32) of every scored token: window by window, each window's
    tokens 1.. given the tokens before them in that window."""
    got = {}

    def keep(i, o):
        if o.prompt_logprobs is not None:
            got[i] = o.prompt_logprobs
        if o.finished and o.finish_reason == "error":
            raise RuntimeError(f"window {i}: {o.error}")

    sp = SamplingParams(temperature=0.0, max_tokens=1, ignore_eos=True, prompt_logprobs=0)
    for i, w in enumerate(wins):
        eng.add_request(f"w{i}", w, sp, on_output=lambda o, i=i: keep(i, o))
    while eng.has_work():
        eng.step()
    lps, ranks = [], []
    for i, w in enumerate(wins):
        entries = got[i]
        assert len(entries) == len(w) and entries[0] is None
        assert [e[0] for e in entries[1:]] == list(w[1:])
        lps += [e[1] for e in entries[1:]]
        ranks += [e[2] for e in entries[1:]]
    return np.asarray(lps, np.float32), np.asarray(ranks, np.int32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("text", nargs="?", help="text file to score (UTF-8)")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="score N seeded random token ids")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--window", type=int, default=2048)
    ap.add_argument("--model", default=None)
    ap.add_argument("--device", default="auto")
    ap.add_argument("--save", metavar="FILE.npy")
    ap.add_argument("--compare", metavar="FILE.npy")
    a = ap.parse_args()
    if bool(a.text) == bool(a.synthetic):
        ap.error("give a text file or --synthetic N")
    if a.window < 2:
        ap.error("--window must be at least 2")
    cfg = EngineConfig.from_env(model=a.model, device=a.device,
                                max_model_len=max(a.window + 8, 64))
    eng = LLMEngine(cfg)
    if a.synthetic:
        hi = min(eng.model_cfg.vocab_size, 120000)
        ids = np.random.default_rng(a.seed).integers(0, hi, a.synthetic).tolist()
    else:
        with open(a.text, encoding="utf-8") as f:
            ids = [eng.tokenizer.bos_id] + eng.tokenizer.encode(f.read())
    wins = windows(ids, a.window)
    t0 = time.perf_counter()
    lps, ranks = score(eng, wins)
    dt = time.perf_counter() - t0
    fin = np.isfinite(lps)
    nll = float(-lps[fin].astype(np.float64).mean()) if fin.any() else float("nan")
    res = {"tokens": int(lps.size), "windows": len(wins), "window": a.window,
           "mean_nll": nll, "perplexity": math.exp(min(nll, 700.0)),
           "rank1_share": float((ranks == 1).mean()) if lps.size else 0.0,
           "neg_inf_tokens": int((~fin).sum()), "seconds": round(dt, 3),
           "model": eng.model_cfg.name if hasattr(eng.model_cfg, "name") else str(a.model),
           "kv_cache_dtype": cfg.kv_cache_dtype, "kv_scales": cfg.kv_scales,
           "quantization": cfg.quantization, "batch_invariant": cfg.batch_invariant}
    if a.compare:
        base = np.load(a.compare)
        if base.shape != lps.shape:
            raise SystemExit(f"--compare: {a.compare} holds {base.shape[0]} logprobs, this run {lps.size}")
        both = fin & np.isfinite(base)
        d = np.abs(lps[both].astype(np.float64) - base[both].astype(np.float64))
        res.update(delta_mean_abs_logprob=float(d.mean()), delta_max_abs_logprob=float(d.max()),
                   delta_mean_nll=float(nll + base[both].astype(np.float64).mean()),
                   compared_with=a.compare)
    if a.save:
        np.save(a.save, lps)
    eng.shutdown()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
