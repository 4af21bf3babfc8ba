"""W4A16 engines in w4_prefill="int4" mode: every W4 projection above 64 rows runs
the W4 GEMM on the int4 image (csrc/kernels/w4_packed_gemm.hip) -- no dequantized
bf16 prefill image, no per-step scratch, no dense fallback."""
import dataclasses

import numpy as np
import pytest
import torch

from fasttalk_llm_microservice_amd.engine.config import EngineConfig
from fasttalk_llm_microservice_amd.engine.engine import LLMEngine
from fasttalk_llm_microservice_amd.engine.sampling_params import SamplingParams
from fasttalk_llm_microservice_amd.models.config import MODELS
from fasttalk_llm_microservice_amd.models.llama import _ATTR, AttnMeta, LlamaModel

pytestmark = pytest.mark.gpu


def _prefill_inputs(m, T, bs=16):
    """ids and metadata of a T-token prefill on an empty cache (the construction of
    test_gpu_logits_match_cpu_reference)."""
    nblk = max(8, -(-T // bs))
    dev = m.device
    ids = torch.arange(100, 100 + T, dtype=torch.int32, device=dev)
    meta = AttnMeta(
        positions=torch.arange(T, dtype=torch.int32, device=dev),
        slot_mapping=torch.arange(T, dtype=torch.int32, device=dev),
        block_tables=torch.arange(nblk, dtype=torch.int32, device=dev)[None],
        seq_lens=torch.tensor([T], dtype=torch.int32, device=dev),
        logits_indices=torch.arange(T, device=dev),
        q_start_loc=torch.tensor([0, T], dtype=torch.int32,
                                 device=dev if dev.type == "cuda" else "cpu"),
        tile_info=torch.tensor([[0, s, 0xFFFF, -1] for s in range(0, T, 16)], dtype=torch.int32,
                               device=dev).flatten(),
        num_tiles=len(range(0, T, 16)))
    return ids, meta, nblk


def _prefill_logits(m, T, bs=16):
    ids, meta, nblk = _prefill_inputs(m, T, bs)
    kv = m.allocate_kv_cache(nblk, bs)
    return m.compute_logits(m.forward(ids, meta, kv)).float().cpu()


def _forbid_other_paths(m, monkeypatch):
    """In int4 mode neither the per-step scratch nor the dense fallback is reachable."""
    def boom(*a, **k):
        raise AssertionError("int4 mode reached a dequantizing path")
    monkeypatch.setattr(m, "_w4_packed", boom)
    from fasttalk_llm_microservice_amd.ops import quant as Q
    monkeypatch.setattr(Q, "w4_dequant", boom)


@pytest.mark.parametrize("model,T", [("tiny-2k", 100), ("tiny-2k", 300), ("tiny", 100)])
def test_int4_prefill_logits_match_cpu_reference(model, T, monkeypatch):
    monkeypatch.delenv("FT_W4_PREFILL_IMAGE", raising=False)
    cfg = MODELS[model]
    g = LlamaModel(cfg, torch.device("cuda"), torch.bfloat16, max_model_len=512,
                   quantization="w4", w4_prefill="int4").init_random(3, consistent=True)
    c = LlamaModel(cfg, torch.device("cpu"), torch.float32, max_model_len=512, quantization="w4")
    c.init_random(3, consistent=True)
    assert g.w4_int4 and g.w4_prefill_mode() == "int4"
    for L in g.layers:
        assert L.q4 and set(L.q4) == set(_ATTR)
        assert all(getattr(L, a + "_pk") is None and getattr(L, a) is None for a in _ATTR.values())
    _forbid_other_paths(g, monkeypatch)
    a = _prefill_logits(g, T)
    b = _prefill_logits(c, T)
    assert g._w4_scratch is None
    cos = torch.nn.functional.cosine_similarity(a, b, dim=-1)
    print(f"{model} T={T}: min cosine {cos.min().item():.6f}")
    assert cos.min().item() > 0.99, cos.min().item()
    agree = (a.argmax(-1) == b.argmax(-1)).float().mean().item()
    assert agree > 0.9


def test_env_variable_selects_int4_when_field_is_auto(monkeypatch):
    monkeypatch.setenv("FT_W4_PREFILL_IMAGE", "int4")
    g = LlamaModel(MODELS["tiny"], torch.device("cuda"), torch.bfloat16, max_model_len=256,
                   quantization="w4").init_random(3, consistent=True)
    assert g.w4_int4 and g.w4_prefill_mode() == "int4" and g.layers[0].wqkv_pk is None
    g2 = LlamaModel(MODELS["tiny"], torch.device("cuda"), torch.bfloat16, max_model_len=256,
                    quantization="w4", w4_prefill="image").init_random(3, consistent=True)
    assert not g2.w4_int4 and g2.w4_prefill_mode() == "image" and g2.layers[0].wqkv_pk is not None


# ------------------------------------------------------------------ 8B-shaped layers

ROWS_8B = 300


@pytest.fixture(scope="module")
def shape8b():
    """A 2-layer Llama-3-8B-shaped W4 model: the int4-mode GPU model and the fp32 CPU
    reference logits of one 300-token prefill, computed once and left unchanged."""
    cfg = dataclasses.replace(MODELS["llama3-8b"], name="llama3-8b-2l", num_layers=2)
    c = LlamaModel(cfg, torch.device("cpu"), torch.float32, max_model_len=512, quantization="w4")
    c.init_random(5, consistent=True)
    ref = _prefill_logits(c, ROWS_8B)
    del c
    g = LlamaModel(cfg, torch.device("cuda"), torch.bfloat16, max_model_len=512,
                   quantization="w4", w4_prefill="int4").init_random(5, consistent=True)
    yield cfg, g, ref
    del g
    torch.cuda.empty_cache()


def test_llama3_shape_prefill_matches_cpu_fp32(shape8b):
    """300 rows through every projection of the 8B shape (split-K slabs into the fused
    norms / RoPE, the SiLU epilogue) against the fp32 CPU model on the same weights.
    Bar: cosine 0.9995 as in test_llama3_shape_decode_matches_cpu_fp32."""
    cfg, g, ref = shape8b
    assert g.w4_int4 and all(L.wqkv_pk is None and L.wd_pk is None for L in g.layers)
    a = _prefill_logits(g, ROWS_8B)
    assert g._w4_scratch is None
    cos = torch.nn.functional.cosine_similarity(a, ref, dim=-1)
    print(f"llama3-8b-2l int4 T={ROWS_8B}: min cosine {cos.min().item():.6f}")
    assert cos.min().item() > 0.9995, cos.min().item()


def test_footprint_is_the_int4_image(shape8b):
    cfg, g, _ = shape8b
    bf16 = lambda t: t.numel() * 2  # noqa: E731
    q4_bytes = sum(q.nbytes() for L in g.layers for q in L.q4.values())
    norms = sum(bf16(L.ln1) + bf16(L.ln2) for L in g.layers) + bf16(g.norm)
    want = q4_bytes + bf16(g.embed) + bf16(g.lm_head_pk) + norms
    assert g.weights_resident_bytes() == want
    proj_bf16 = sum(q.n * q.k * 2 for L in g.layers for q in L.q4.values())
    img = LlamaModel(cfg, torch.device("cuda"), torch.bfloat16, max_model_len=512,
                     quantization="w4", w4_prefill="image").init_random(5, consistent=True)
    assert img.w4_prefill_mode() == "image"
    assert img.weights_resident_bytes() - g.weights_resident_bytes() == proj_bf16
    del img
    torch.cuda.empty_cache()
    # a second 300-row forward (the layers; the [300, vocab] logits alone would exceed
    # the bound) allocates activations only: less than the bf16 size of the smallest
    # layer projection, so no dequantized weight is materialised
    ids, meta, nblk = _prefill_inputs(g, ROWS_8B)
    kv = g.allocate_kv_cache(nblk, 16)
    g.forward(ids, meta, kv)
    torch.cuda.synchronize()
    smallest = min(q.n * q.k * 2 for q in g.layers[0].q4.values())
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    h = g.forward(ids, meta, kv)
    torch.cuda.synchronize()
    assert torch.isfinite(h.float()).all()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"peak over the forward {peak / 1e6:.1f} MB, smallest projection {smallest / 1e6:.1f} MB")
    assert peak < smallest
    assert g._w4_scratch is None


# ------------------------------------------------------------------ engine

def _engine(**kw):
    base = dict(model="tiny", device="cuda", num_kv_blocks=512, max_model_len=2048,
                max_num_seqs=16)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def test_engine_int4_end_to_end(monkeypatch):
    """Chunked prefill (600 tokens over a 512 chunk), mixed steps with decode rows and
    graph decode in int4 mode; eager and graph engines agree on the greedy tokens."""
    monkeypatch.delenv("FT_W4_PREFILL_IMAGE", raising=False)
    rng = np.random.default_rng(0)
    prompts = [rng.integers(0, 120000, n).tolist() for n in (5, 70, 200, 600)]
    sp = SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True)
    outs = []
    for eager in (True, False):
        e = _engine(model="tiny-2k", quantization="w4", w4_prefill="int4", enforce_eager=eager)
        m = e.runner.model
        assert m.w4_int4 and all(L.wqkv_pk is None for L in m.layers)
        out = e.generate(prompts, sp)
        assert all(len(o) == 24 for o in out)
        st = e.metrics()
        assert st["w4_prefill"] == "int4" and st["weights_resident_gb"] > 0
        assert m._w4_scratch is None
        outs.append(out)
        del e
        torch.cuda.empty_cache()
    assert outs[0] == outs[1]


def test_stats_report_resolved_mode(monkeypatch):
    monkeypatch.delenv("FT_W4_PREFILL_IMAGE", raising=False)
    e = _engine(quantization="w4")                       # auto: the image fits
    assert e.metrics()["w4_prefill"] == "image"
    img_gb = e.metrics()["weights_resident_gb"]
    e = _engine(quantization="w4", w4_prefill="scratch")
    assert e.metrics()["w4_prefill"] == "scratch" and e.metrics()["weights_resident_gb"] < img_gb
    e = _engine()                                        # bf16: the resident figure only
    assert "w4_prefill" not in e.metrics() and e.metrics()["weights_resident_gb"] > 0
