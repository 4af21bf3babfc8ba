"""TP=2 W4A16 in w4_prefill="int4" mode on ONE MI355X (rank 0 this process, rank 1 a
spawned worker, both on cuda:0 as in test_tp_share_gpu.py): the logits of a 100-token
prefill -- every shard projection through the W4 GEMM on its int4 image, partial sums
through the custom all-reduce -- against TP=1 in the same mode on the same weights."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _cfg(**kw):
    from fasttalk_llm_microservice_amd.engine.config import EngineConfig

    base = dict(model="tiny-2k", device="cuda", num_kv_blocks=512, max_model_len=1024,
                max_num_seqs=8, max_num_batched_tokens=256, graph_batch_sizes=(1, 2, 4, 8),
                enable_prefix_caching=False, quantization="w4", w4_prefill="int4")
    base.update(kw)
    return EngineConfig(**base)


def _prefill_logits(eng, prompt):
    """Logits of the prompt's last row from one eager prefill step (the runner's tap)."""
    from fasttalk_llm_microservice_amd.engine.sampling_params import SamplingParams

    eng.runner.logits_tap = []
    eng.generate([prompt], SamplingParams(temperature=0, max_tokens=1, ignore_eos=True))
    row = eng.runner.logits_tap[-1][-1]
    eng.runner.logits_tap = None
    return row.float().cpu()


def test_tp2_int4_prefill_logits_match_tp1(monkeypatch):
    import torch

    from fasttalk_llm_microservice_amd.engine.engine import LLMEngine
    from fasttalk_llm_microservice_amd.parallel.tp import spawn_tp_engine

    monkeypatch.setenv("FT_CONSISTENT_INIT", "1")
    monkeypatch.delenv("FT_FAULT_TP_STALL", raising=False)
    monkeypatch.delenv("FT_W4_PREFILL_IMAGE", raising=False)
    prompt = np.random.default_rng(5).integers(0, 120000, 100).tolist()
    eng1 = LLMEngine(_cfg())
    assert eng1.runner.model.w4_int4 and eng1.metrics()["w4_prefill"] == "int4"
    ref = _prefill_logits(eng1, prompt)
    del eng1
    torch.cuda.empty_cache()
    eng = spawn_tp_engine(_cfg(tp_size=2, tp_share_device=True, custom_allreduce=True))
    try:
        m = eng.runner.model
        assert m.tp == 2 and m.w4_int4 and all(L.wqkv_pk is None for L in m.layers)
        got = _prefill_logits(eng, prompt)
        assert m._w4_scratch is None
    finally:
        eng.shutdown()
    cos = torch.nn.functional.cosine_similarity(got, ref, dim=-1).item()
    print(f"TP2 int4 vs TP1 int4, 100-token prefill: cosine {cos:.6f}")
    assert cos > 0.999, cos
