"""MXFP4 weights through the model and the engine on the GPU: every layer projection
runs mx4a16.hip (<= 64 rows) or mx4_packed_gemm.hip (above) on the MXFP4 image, which is
the only resident copy of a projection.  The references are fp32 CPU models holding the
same codes and scale bytes (quantization happens from the same bf16 values on both), so
both sides compute on identical dequantized weights and the bars are those of
tests/test_w8_engine_gpu.py."""
import dataclasses

import numpy as np
import pytest
import torch

from fasttalk_llm_microservice_amd import ops
from fasttalk_llm_microservice_amd.engine.config import EngineConfig
from fasttalk_llm_microservice_amd.engine.engine import LLMEngine
from fasttalk_llm_microservice_amd.engine.sampling_params import SamplingParams
from fasttalk_llm_microservice_amd.models.config import MODELS
from fasttalk_llm_microservice_amd.models.llama import _ATTR, AttnMeta, LlamaModel
from fasttalk_llm_microservice_amd.ops import quant as Q

pytestmark = pytest.mark.gpu


def _prefill_inputs(m, T, bs=16):
    """ids and metadata of a T-token prefill on an empty cache."""
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


def _pair(cfg, seed, max_len=512):
    g = LlamaModel(cfg, torch.device("cuda"), torch.bfloat16, max_model_len=max_len,
                   quantization="mxfp4").init_random(seed, consistent=True)
    c = LlamaModel(cfg, torch.device("cpu"), torch.float32, max_model_len=max_len,
                   quantization="mxfp4").init_random(seed, consistent=True)
    return g, c


def _only_mx4_resident(g):
    for L in g.layers:
        assert L.q4x and set(L.q4x) == set(_ATTR) and not L.q4 and not L.q8
        assert all(getattr(L, a + "_pk") is None and getattr(L, a) is None for a in _ATTR.values())
        assert L.fqkv is None and L.fo is None and L.fgu is None and L.fd is None
        for q in L.q4x.values():
            assert q.wq.dtype == torch.uint8 and q.sc.dtype == torch.uint8
    assert not g.fused and not g.block


# ------------------------------------------------------------------ tiny model
@pytest.fixture(scope="module")
def tiny_pair():
    g, c = _pair(MODELS["tiny"], 3)
    yield g, c
    del g
    torch.cuda.empty_cache()


def test_gpu_and_cpu_hold_the_same_codes_and_scales(tiny_pair):
    g, c = tiny_pair
    _only_mx4_resident(g)
    for Lg, Lc in zip(g.layers, c.layers):
        for proj, attr in _ATTR.items():
            c_, s = Q.unpack_mx4(Lg.q4x[proj], gate_up=proj == "gu")
            assert torch.equal(Q.dequantize_mx4(c_.cpu(), s.cpu()), getattr(Lc, attr))


@pytest.mark.parametrize("T", [1, 50, 64, 65, 300])
def test_tiny_prefill_logits_match_cpu_reference(tiny_pair, T):
    g, c = tiny_pair
    a, b = _prefill_logits(g, T), _prefill_logits(c, T)
    cos = torch.nn.functional.cosine_similarity(a, b, dim=-1)
    agree = (a.argmax(-1) == b.argmax(-1)).float().mean().item()
    print(f"tiny mxfp4 T={T}: min cosine {cos.min().item():.6f}, greedy agreement {agree:.3f}")
    assert cos.min().item() > 0.99, cos.min().item()
    assert agree > 0.9


# ------------------------------------------------------------------ 8B-shaped layers
ROWS_DEC, ROWS_PRE = 50, 300


def _decode_case(rows, bs=16):
    rng = np.random.default_rng(rows)
    lens = rng.integers(16, 400, rows)
    lens[0] = 400
    nblk = [int(-(-n // bs)) for n in lens]
    perm = torch.from_numpy(rng.permutation(sum(nblk)).astype(np.int32))
    bt = torch.zeros(rows, max(nblk), dtype=torch.int32)
    o = 0
    for i, nb in enumerate(nblk):
        bt[i, :nb] = perm[o:o + nb]
        o += nb
    ids = torch.from_numpy(rng.integers(0, 120000, rows).astype(np.int32))
    pos = torch.from_numpy((lens - 1).astype(np.int32))
    slots = torch.tensor([int(bt[i, (lens[i] - 1) // bs]) * bs + (lens[i] - 1) % bs
                          for i in range(rows)], dtype=torch.int32)
    return sum(nblk), bt, ids, pos, slots


def _decode_meta(rows, bt, pos, slots, dev, tmp=None):
    m = AttnMeta(positions=pos.to(dev), slot_mapping=slots.to(dev),
                 logits_indices=torch.arange(rows, device=dev), num_decode=rows,
                 dec_block_tables=bt.to(dev), dec_seq_lens=(pos + 1).to(dev))
    if tmp is not None:
        m.tmp_out, m.tmp_ml = tmp
    return m


@pytest.fixture(scope="module")
def shape8b():
    """A 2-layer Llama-3-8B-shaped MXFP4 model on the GPU and the fp32 CPU model's logits
    of one 300-token prefill and one 50-row decode step over random KV caches, computed
    once and left unchanged."""
    cfg = dataclasses.replace(MODELS["llama3-8b"], name="llama3-8b-2l", num_layers=2)
    g, c = _pair(cfg, 5, max_len=1024)
    ref_pre = _prefill_logits(c, ROWS_PRE)
    total, bt, ids, pos, slots = _decode_case(ROWS_DEC)
    kv_c = c.allocate_kv_cache(total, 16)
    gen = torch.Generator().manual_seed(1)
    kv_vals = []
    for kc, vc in kv_c:
        kc.copy_(torch.randn(kc.shape, generator=gen).bfloat16().float())
        vc.copy_(torch.randn(vc.shape, generator=gen).bfloat16().float())
        kv_vals.append((kc.bfloat16(), vc.bfloat16()))
    ref_dec = c.compute_logits(c.forward(ids, _decode_meta(ROWS_DEC, bt, pos, slots, "cpu"), kv_c)).float()
    del c, kv_c
    yield cfg, g, ref_pre, ref_dec, (total, bt, ids, pos, slots, kv_vals)
    del g
    torch.cuda.empty_cache()


def test_llama3_shape_prefill_matches_cpu_fp32(shape8b):
    """300 rows through every projection of the 8B shape (split-K slabs into the fused
    norms / RoPE, the SiLU epilogue).  Bar: cosine 0.9995 (bf16 activations against fp32
    on equal weights; test_llama3_shape_decode_matches_cpu_fp32)."""
    _, g, ref_pre, _, _ = shape8b
    _only_mx4_resident(g)
    a = _prefill_logits(g, ROWS_PRE)
    cos = torch.nn.functional.cosine_similarity(a, ref_pre, dim=-1)
    print(f"llama3-8b-2l mxfp4 prefill T={ROWS_PRE}: min cosine {cos.min().item():.6f}")
    assert cos.min().item() > 0.9995, cos.min().item()


def test_llama3_shape_decode_matches_cpu_fp32_eager_and_graph(shape8b):
    """50 decode rows (the 64-row bucket of MX4_PLAN: split-K slabs into slab_rope_kv and
    the add + RMSNorm, gate_up's own SiLU epilogue), eager and replayed from a hipGraph."""
    _, g, _, ref, (total, bt, ids, pos, slots, kv_vals) = shape8b
    rows = ROWS_DEC
    kv_g = g.allocate_kv_cache(total, 16)
    for (kg, vg), (kc, vc) in zip(kv_g, kv_vals):
        kg.copy_(kc)
        vg.copy_(vc)
    n_out, n_ml = ops.decode_workspace(rows, g.nq, g.nkv, g.d)
    tmp = (torch.empty(n_out, device="cuda"), torch.empty(n_ml, device="cuda"))
    mg = _decode_meta(rows, bt, pos, slots, "cuda", tmp)
    idg = ids.cuda()
    with torch.inference_mode():
        eager = g.compute_logits(g.forward(idg, mg, kv_g)).float().cpu()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            g.compute_logits(g.forward(idg, mg, kv_g))
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = g.compute_logits(g.forward(idg, mg, kv_g))
        graph.replay()
        torch.cuda.synchronize()
        replayed = out.float().cpu()
    for name, a in (("eager", eager), ("graph", replayed)):
        cos = torch.nn.functional.cosine_similarity(a, ref, dim=-1)
        print(f"llama3-8b-2l mxfp4 decode rows {rows} {name}: min cosine {cos.min().item():.6f}")
        assert cos.min().item() > 0.9995, (name, cos.min().item())
    assert torch.equal(eager, replayed)


def test_footprint_is_the_mx4_image(shape8b):
    cfg, g, *_ = shape8b
    H, I = cfg.hidden_size, cfg.intermediate_size
    nqkv = (cfg.num_heads + 2 * cfg.num_kv_heads) * cfg.head_dim
    shapes = [(nqkv, H), (H, cfg.num_heads * cfg.head_dim), (2 * I, H), (H, I)]
    proj = cfg.num_layers * sum(n * k // 2 + n * k // 32 for n, k in shapes)
    bf16 = 2 * (cfg.vocab_size * H * (1 if cfg.tie_word_embeddings else 2)
                + cfg.num_layers * 2 * H + H)
    assert g.weights_resident_bytes() == proj + bf16
    assert sum(q.nbytes() for L in g.layers for q in L.q4x.values()) == proj


# ------------------------------------------------------------------ engine
def _engine(**kw):
    base = dict(model="tiny-2k", device="cuda", num_kv_blocks=512, max_model_len=2048,
                max_num_seqs=16)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def _prompts():
    rng = np.random.default_rng(0)
    return [rng.integers(0, 120000, n).tolist() for n in (5, 70, 200, 600)]


def test_engine_mxfp4_graph_decode_equals_eager_and_stats():
    """Chunked prefill, mixed steps and decode: the graph engine and the eager engine
    agree on the greedy tokens; /stats names the quantization and the MXFP4 footprint."""
    sp = SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True)
    outs = []
    for eager in (True, False):
        e = _engine(quantization="mxfp4", enforce_eager=eager)
        _only_mx4_resident(e.runner.model)
        out = e.generate(_prompts(), sp)
        assert all(len(o) == 24 for o in out)
        st = e.metrics()
        assert st["quantization"] == "mxfp4" and "w4_prefill" not in st
        assert st["weights_resident_gb"] == round(e.runner.model.weights_resident_bytes() / 1e9, 6)
        if not eager:
            assert e.runner.stats["graph_replays"] > 0, e.runner.stats
        outs.append(out)
        del e
        torch.cuda.empty_cache()
    assert outs[0] == outs[1]


def test_engine_mxfp4_seeded_runs_repeat_and_fp8_kv_combines():
    sp = SamplingParams(temperature=0.8, top_p=0.9, seed=7, max_tokens=16, ignore_eos=True)
    a = _engine(quantization="mxfp4").generate(_prompts(), sp)
    torch.cuda.empty_cache()
    b = _engine(quantization="mxfp4").generate(_prompts(), sp)
    assert a == b and all(len(o) == 16 for o in a)
    torch.cuda.empty_cache()
    e = _engine(quantization="mxfp4", kv_cache_dtype="fp8")
    out = e.generate(_prompts(), SamplingParams(temperature=0.0, max_tokens=16, ignore_eos=True))
    assert all(len(o) == 16 for o in out)
    st = e.metrics()
    assert st["quantization"] == "mxfp4" and st["kv_cache_dtype"] == "fp8"
    m = e.runner.model
    ids, meta, nblk = _prefill_inputs(m, 80)
    kv = m.allocate_kv_cache(nblk, 16, torch.float8_e4m3fn)
    assert bool(torch.isfinite(m.compute_logits(m.forward(ids, meta, kv)).float()).all())


def test_engine_without_the_setting_is_unchanged():
    plain = _engine()
    mx4 = _engine(quantization="mxfp4")
    sp = SamplingParams(temperature=0.0, max_tokens=4, ignore_eos=True)
    plain.generate(_prompts()[:2], sp)
    again = _engine()
    assert plain.generate(_prompts()[:2], sp) == again.generate(_prompts()[:2], sp)
    mx4.generate(_prompts()[:2], sp)
    mp, mf = plain.metrics(), mx4.metrics()
    assert "quantization" not in mp and set(mf) - set(mp) == {"quantization"} and set(mp) <= set(mf)
    m = plain.runner.model
    assert m.quant is None and all(L.q4x is None and L.q8 is None and L.q4 is None for L in m.layers)
    assert all(L.wqkv_pk is not None for L in m.layers)
    assert mf["weights_resident_gb"] < mp["weights_resident_gb"]


def test_mxfp4_refused_with_tensor_parallel_and_batch_invariant():
    with pytest.raises(ValueError, match="tensor parallel"):
        EngineConfig(model="tiny", quantization="mxfp4", tp_size=2)
    with pytest.raises(ValueError, match="batch-invariant"):
        EngineConfig(model="tiny", quantization="mxfp4", batch_invariant=True)
