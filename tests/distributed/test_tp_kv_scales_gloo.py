"""fp8 KV scales under tensor parallelism (CPU, gloo): every rank slices the
checkpoint's per-head scales with weights.kv_head_range, so TP=2 must reproduce TP=1
token for token.  The scales differ per head and sit near 2 * absmax / 448 of weights
whose K / V are 1024x the random-init ones: a rank that took the other head's scale
(or none) would quantise differently."""
import numpy as np
import torch

from fasttalk_llm_microservice_amd.engine.config import EngineConfig
from fasttalk_llm_microservice_amd.engine.engine import LLMEngine
from fasttalk_llm_microservice_amd.engine.sampling_params import SamplingParams
from fasttalk_llm_microservice_amd.models import weights as W
from fasttalk_llm_microservice_amd.models.config import MODELS

C = 1024.0


def _cfg(**kw):
    base = dict(model="tiny", device="cpu", num_kv_blocks=256, max_model_len=1024, max_num_seqs=8,
                max_num_batched_tokens=64, kv_cache_dtype="fp8")
    base.update(kw)
    return EngineConfig(**base)


def _ckpt(path):
    cfg = MODELS["tiny"]
    g = torch.Generator().manual_seed(3)
    layers = [W.random_full_layer(cfg, g, 0.02, torch.bfloat16) for _ in range(cfg.num_layers)]
    for L in layers:
        L["q"], L["o"] = (L["q"].float() / C).bfloat16(), (L["o"].float() / C).bfloat16()
        L["k"], L["v"] = (L["k"].float() * C).bfloat16(), (L["v"].float() * C).bfloat16()
    embed = (torch.randn(cfg.vocab_size, cfg.hidden_size, generator=g) * 0.02).bfloat16()
    # head 1's scales are 4x head 0's: far enough apart that a swap changes the cache
    k = torch.tensor([[8.0, 33.0], [9.5, 37.0]])
    v = torch.tensor([[10.0, 41.0], [12.5, 45.0]])
    W.save_hf_checkpoint(cfg, layers, embed, torch.ones(cfg.hidden_size).bfloat16(), None, str(path),
                         kv_scales={"k": list(k), "v": list(v)})
    return str(path), k, v


def test_tp2_checkpoint_kv_scales_match_tp1(tmp_path):
    from fasttalk_llm_microservice_amd.parallel.tp import spawn_tp_engine

    ck, k, v = _ckpt(tmp_path / "ck")
    rng = np.random.default_rng(2)
    prompts = [rng.integers(0, 120000, n).tolist() for n in (12, 70, 30)]
    sp = SamplingParams(temperature=0, max_tokens=6, ignore_eos=True)
    one = LLMEngine(_cfg(weights=ck))
    assert one.metrics()["kv_scales"]["source"] == "checkpoint"
    ref = one.generate(prompts, sp)
    # the scales matter: the same checkpoint at scale 1.0 clips and decodes differently
    assert LLMEngine(_cfg(weights=ck, kv_scales="one")).generate(prompts, sp) != ref
    eng = spawn_tp_engine(_cfg(weights=ck, tp_size=2))
    try:
        m = eng.runner.model
        assert m.nkv == 1
        # rank 0 holds kv head 0 of every layer
        assert torch.equal(torch.stack([s[0] for s in m.kv_scales]), k[:, 0:1])
        assert torch.equal(torch.stack([s[1] for s in m.kv_scales]), v[:, 0:1])
        out = eng.generate(prompts, sp)
    finally:
        eng.shutdown()
    assert out == ref


def test_tp2_json_kv_scales_match_tp1(tmp_path):
    from fasttalk_llm_microservice_amd.parallel.tp import spawn_tp_engine

    ck, k, v = _ckpt(tmp_path / "ck")
    rng = np.random.default_rng(4)
    prompts = [rng.integers(0, 120000, n).tolist() for n in (20, 45)]
    sp = SamplingParams(temperature=0, max_tokens=6, ignore_eos=True)
    one = LLMEngine(_cfg(weights=ck, kv_scales="calibrate"))
    p = str(tmp_path / "scales.json")
    one.save_kv_scales(p)
    ref = LLMEngine(_cfg(weights=ck, kv_scales=p)).generate(prompts, sp)
    assert ref == one.generate(prompts, sp)
    eng = spawn_tp_engine(_cfg(weights=ck, kv_scales=p, tp_size=2))
    try:
        assert eng.metrics()["kv_scales"]["source"] == "file"
        out = eng.generate(prompts, sp)
    finally:
        eng.shutdown()
    assert out == ref
