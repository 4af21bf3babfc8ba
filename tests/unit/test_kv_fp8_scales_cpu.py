"""Per-head scales of the fp8 KV cache on the CPU backend: the kv_scales setting, the
reference write / read (ops/reference.py), checkpoint and JSON scales, calibration."""
import json

import pytest
import torch

from fasttalk_llm_microservice_amd import ops
from fasttalk_llm_microservice_amd.engine import kv_calibrate
from fasttalk_llm_microservice_amd.engine.chat_template import ChatTemplate
from fasttalk_llm_microservice_amd.engine.config import EngineConfig
from fasttalk_llm_microservice_amd.engine.engine import LLMEngine
from fasttalk_llm_microservice_amd.engine.sampling_params import SamplingParams
from fasttalk_llm_microservice_amd.engine.tokenizer import get_tokenizer
from fasttalk_llm_microservice_amd.models import weights as W
from fasttalk_llm_microservice_amd.models.config import MODELS
from fasttalk_llm_microservice_amd.models.llama import AttnMeta, LlamaModel
from fasttalk_llm_microservice_amd.ops import reference as ref

F8 = torch.float8_e4m3fn
C = 1024.0


# ------------------------------------------------------------------------- config

def test_kv_scales_setting_parses(monkeypatch, tmp_path):
    assert EngineConfig().kv_scales == "auto"
    assert EngineConfig(kv_cache_dtype="fp8", kv_scales="one").check_kv_scales() == "one"
    assert EngineConfig(kv_cache_dtype="fp8", kv_scales="calibrate").check_kv_scales() == "calibrate"
    p = str(tmp_path / "s.json")
    assert EngineConfig(kv_cache_dtype="fp8", kv_scales=p).check_kv_scales() == "file"
    assert EngineConfig(kv_scales="one").check_kv_scales() == "one"    # bf16 + one is today's path
    with pytest.raises(ValueError):
        EngineConfig(kv_cache_dtype="fp8", kv_scales="sometimes")
    with pytest.raises(ValueError):
        EngineConfig(kv_scales="calibrate")                             # bf16 KV
    with pytest.raises(ValueError):
        EngineConfig(kv_scales=p)
    monkeypatch.setenv("ENGINE_KV_CACHE_DTYPE", "fp8")
    monkeypatch.setenv("ENGINE_KV_SCALES", "calibrate")
    c = EngineConfig.from_env(model="tiny")
    assert c.kv_scales == "calibrate" and c.kv_cache_dtype == "fp8"
    monkeypatch.setenv("ENGINE_KV_CACHE_DTYPE", "auto")
    with pytest.raises(ValueError):
        EngineConfig.from_env(model="tiny")
    assert kv_calibrate.parse_setting(None) == ("auto", None)
    with pytest.raises(ValueError):
        kv_calibrate.parse_setting("scales.yaml")


def test_headroom_and_token_cap_knobs(monkeypatch):
    assert kv_calibrate.headroom() == 2.0
    monkeypatch.setenv("ENGINE_KV_SCALE_HEADROOM", "1.5")
    assert kv_calibrate.headroom() == 1.5
    s = kv_calibrate.scales_from_absmax(torch.tensor([[448.0, 0.0]]))
    assert s[0, 0].item() == 1.5 and 0 < s[0, 1].item() == kv_calibrate.SCALE_TINY
    monkeypatch.setenv("ENGINE_KV_SCALE_HEADROOM", "-1")
    with pytest.raises(ValueError):
        kv_calibrate.headroom()
    tmpl = ChatTemplate(get_tokenizer(None))
    ids = kv_calibrate.calibration_prompt_ids(tmpl)
    assert 256 <= len(ids) <= kv_calibrate.DEFAULT_CALIB_TOKENS
    monkeypatch.setenv("ENGINE_KV_CALIB_TOKENS", "64")
    assert len(kv_calibrate.calibration_prompt_ids(tmpl)) == 64


# ---------------------------------------------------------------- reference write / read

def test_reference_write_read_roundtrip_with_scales():
    nq, nkv, d, t, bs, nblocks = 8, 4, 64, 37, 16, 6
    torch.manual_seed(0)
    ks = 0.37 * (torch.arange(nkv).float() + 1) + 2.0
    vs = 2.0 ** (torch.arange(nkv) % 4 - 1).float() * 1.1 + 2.0
    qkv = torch.randn(t, (nq + 2 * nkv) * d) * 192
    pos = torch.arange(t, dtype=torch.int32)
    cs = ref.rope_cos_sin(d, 64, 500000.0, None)
    slots = torch.randperm(nblocks * bs)[:t].int()
    k = torch.zeros(nblocks, nkv, bs, d).to(F8)
    v = torch.zeros(nblocks, nkv, d, bs).to(F8)
    x = qkv.clone()
    ops.rope_kv_write(x, pos, cs, slots, k, v, nq, nkv, d, k_scale=ks, v_scale=vs)
    blk, off = slots.long() // bs, slots.long() % bs
    k_true = ref.apply_rope(qkv[:, nq * d:(nq + nkv) * d].view(t, nkv, d), pos, cs)
    v_true = qkv[:, (nq + nkv) * d:].view(t, nkv, d)
    for stored, true, sc in ((k[blk, :, off, :], k_true, ks), (v[blk, :, :, off], v_true, vs)):
        got = stored.float() * sc.view(1, -1, 1)
        # half an e4m3 step: 1/16 relative (normal), 2^-10 stored units (subnormal)
        tol = true.abs() * (1 / 16 + 1e-5) + sc.view(1, -1, 1) * 2.0 ** -10
        assert bool(((got - true).abs() <= tol).all())
        assert stored.float().abs().max().item() < 448
    # the same rows at scale 1.0 clip: the clamp comes after the scaling
    k1, v1 = torch.zeros_like(k), torch.zeros_like(v)
    ops.rope_kv_write(qkv.clone(), pos, cs, slots, k1, v1, nq, nkv, d)
    assert k1.float().abs().max().item() == 448 and v1.float().abs().max().item() == 448
    big = ref.to_cache(torch.full((1, nkv, 2), 1e6), k, 1.0 / ks)
    assert torch.equal(big.float(), torch.full((1, nkv, 2), 448.0))
    assert torch.isfinite(big.float()).all()
    # read: paged_attention with the scales == paged_attention over the dequantised cache
    q = torch.randn(t, nq, d)
    bt = torch.arange(nblocks, dtype=torch.int32)[None]
    k2 = torch.zeros_like(k)
    v2 = torch.zeros_like(v)
    seq = torch.arange(t, dtype=torch.int32)
    ops.rope_kv_write(qkv.clone(), pos, cs, seq, k2, v2, nq, nkv, d, k_scale=ks, v_scale=vs)
    sl, qsl = torch.tensor([t], dtype=torch.int32), torch.tensor([0, t], dtype=torch.int32)
    a = ref.paged_attention(q, k2, v2, bt, sl, qsl, d ** -0.5, ks, vs)
    b = ref.paged_attention(q, k2.float() * ks.view(1, -1, 1, 1), v2.float() * vs.view(1, -1, 1, 1),
                            bt, sl, qsl, d ** -0.5)
    assert torch.allclose(a, b, rtol=1e-5, atol=1e-5)
    with pytest.raises(ValueError):   # scales are for fp8 caches only
        ref.to_cache(torch.zeros(1, nkv, 2), torch.zeros(1), 1.0 / ks)


def test_unit_scales_match_absent_scales_reference():
    nq, nkv, d, t, bs = 4, 2, 64, 20, 16
    torch.manual_seed(1)
    one = torch.ones(nkv)
    qkv = torch.randn(t, (nq + 2 * nkv) * d) * 3
    pos = torch.arange(t, dtype=torch.int32)
    cs = ref.rope_cos_sin(d, 64, 500000.0, None)
    slots = torch.arange(t, dtype=torch.int32)
    ka, va = torch.zeros(2, nkv, bs, d).to(F8), torch.zeros(2, nkv, d, bs).to(F8)
    kb, vb = ka.clone(), va.clone()
    ops.rope_kv_write(qkv.clone(), pos, cs, slots, ka, va, nq, nkv, d)
    ops.rope_kv_write(qkv.clone(), pos, cs, slots, kb, vb, nq, nkv, d, k_scale=one, v_scale=one)
    assert torch.equal(ka.view(torch.uint8), kb.view(torch.uint8))
    assert torch.equal(va.view(torch.uint8), vb.view(torch.uint8))


# ------------------------------------------------------------------ checkpoint scales

def _layers(cfg, seed=3, outliers=False, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    layers = [W.random_full_layer(cfg, g, 0.02, dtype) for _ in range(cfg.num_layers)]
    if outliers:   # K / V 1024x larger, same function (exact: a power of two)
        for L in layers:
            L["q"], L["o"] = L["q"] / C, L["o"] / C
            L["k"], L["v"] = L["k"] * C, L["v"] * C
    embed = (torch.randn(cfg.vocab_size, cfg.hidden_size, generator=g) * 0.02).to(dtype)
    return layers, embed


def _save(cfg, path, kv_scales=None, outliers=False):
    layers, embed = _layers(cfg, outliers=outliers, dtype=torch.bfloat16)
    W.save_hf_checkpoint(cfg, layers, embed, torch.ones(cfg.hidden_size).bfloat16(), None,
                         str(path), kv_scales=kv_scales)
    return str(path)


def test_checkpoint_scale_forms_load(tmp_path):
    cfg = MODELS["tiny"]
    nl, nkv = cfg.num_layers, cfg.num_kv_heads
    per_head = [torch.tensor([1.5 + li + 0.25 * h for h in range(nkv)]) for li in range(nl)]
    d1 = _save(cfg, tmp_path / "a", {"k": [2.5, 3.5][:nl], "v": per_head})
    k, v = W.load_kv_scales(cfg, W.SafetensorsIndex(d1))
    assert torch.equal(k, torch.tensor([[2.5] * nkv, [3.5] * nkv][:nl]))     # scalar: broadcast
    assert torch.equal(v, torch.stack(per_head))                             # [nkv]
    d2 = _save(cfg, tmp_path / "b", {"kv": [torch.tensor([0.75])] * nl})      # legacy, one element
    k, v = W.load_kv_scales(cfg, W.SafetensorsIndex(d2))
    assert torch.equal(k, torch.full((nl, nkv), 0.75)) and torch.equal(v, k)
    d3 = _save(cfg, tmp_path / "c")
    assert W.load_kv_scales(cfg, W.SafetensorsIndex(d3)) is None
    m = LlamaModel(cfg, torch.device("cpu"), torch.float32, max_model_len=64).load_checkpoint(d1)
    assert torch.equal(m.ckpt_kv_scales[1], torch.stack(per_head)) and m.kv_scales is None
    # TP rank 1 of 2 holds kv head 1
    assert torch.equal(W.shard_kv_scales(cfg, torch.stack(per_head), 1, 2),
                       torch.stack(per_head)[:, 1:2])
    with pytest.raises(ValueError):
        W.save_hf_checkpoint(cfg, [], torch.zeros(1), torch.zeros(1), None, str(tmp_path / "x"),
                             kv_scales={"q": [1.0]})


@pytest.mark.parametrize("bad", [0.0, float("nan"), -1.0, float("inf")])
def test_checkpoint_bad_scale_raises(tmp_path, bad):
    cfg = MODELS["tiny"]
    d = _save(cfg, tmp_path / "bad", {"k": [1.0, bad], "v": [1.0, 1.0]})
    with pytest.raises(ValueError):
        LlamaModel(cfg, torch.device("cpu"), torch.float32, max_model_len=64).load_checkpoint(d)
    m = LlamaModel(cfg, torch.device("cpu"), torch.float32, max_model_len=64)
    with pytest.raises(ValueError):
        m.set_kv_scales(torch.full((cfg.num_layers, cfg.num_kv_heads), bad),
                        torch.ones(cfg.num_layers, cfg.num_kv_heads))
    with pytest.raises(ValueError):   # wrong shape
        m.set_kv_scales(torch.ones(cfg.num_layers, cfg.num_kv_heads + 1),
                        torch.ones(cfg.num_layers, cfg.num_kv_heads))


def test_set_kv_scales_copies_in_place():
    cfg = MODELS["tiny"]
    m = LlamaModel(cfg, torch.device("cpu"), torch.float32, max_model_len=64)
    shape = (cfg.num_layers, cfg.num_kv_heads)
    m.set_kv_scales(torch.full(shape, 2.0), torch.full(shape, 3.0))
    ptrs = [t.data_ptr() for s in m.kv_scales for t in s]
    m.set_kv_scales(torch.full(shape, 5.0), torch.full(shape, 7.0))
    assert ptrs == [t.data_ptr() for s in m.kv_scales for t in s]   # graphs capture these
    ks, vs, ki, vi = m.kv_scales[1]
    assert ks[0].item() == 5.0 and vs[0].item() == 7.0
    assert ki[0].item() == (1.0 / torch.tensor(5.0)).item() and vi[0].item() == (1.0 / torch.tensor(7.0)).item()


# --------------------------------------------------------------------- engine, JSON

def _engine(**kw):
    base = dict(model="tiny", device="cpu", num_kv_blocks=256, max_model_len=1024, max_num_seqs=4)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def test_engine_auto_uses_checkpoint_scales_and_json_roundtrips(tmp_path):
    cfg = MODELS["tiny"]
    nkv = cfg.num_kv_heads
    k = torch.stack([9.0 + li + 0.37 * (torch.arange(nkv).float() + 1) for li in range(cfg.num_layers)])
    v = k + 2.0
    ck = _save(cfg, tmp_path / "ck", {"k": list(k), "v": list(v)}, outliers=True)
    e = _engine(weights=ck, kv_cache_dtype="fp8")          # kv_scales defaults to auto
    m = e.runner.model
    assert torch.equal(torch.stack([s[0] for s in m.kv_scales]), k)
    assert torch.equal(torch.stack([s[1] for s in m.kv_scales]), v)
    info = e.metrics()["kv_scales"]
    assert info["source"] == "checkpoint" and info["k_min"] == k.min().item() \
        and info["v_max"] == v.max().item()
    sp = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)
    prompt = [list(range(100, 150))]
    out = e.generate(prompt, sp)
    p = str(tmp_path / "scales.json")
    e.save_kv_scales(p)
    with open(p) as f:
        d = json.load(f)
    assert set(d) == {"k", "v"} and len(d["k"]) == cfg.num_layers and len(d["k"][0]) == nkv
    # the JSON file overrides what the checkpoint carries, and reproduces the tokens
    ck2 = _save(cfg, tmp_path / "ck2", None, outliers=True)
    e2 = _engine(weights=ck2, kv_cache_dtype="fp8", kv_scales=p)
    assert e2.metrics()["kv_scales"]["source"] == "file"
    assert torch.equal(torch.stack([s[0] for s in e2.runner.model.kv_scales]), k)
    assert torch.equal(torch.stack([s[1] for s in e2.runner.model.kv_scales]), v)
    assert e2.generate(prompt, sp) == out
    # auto without checkpoint scales, and "one" with them: scale 1.0, no scale tensors
    assert _engine(weights=ck2, kv_cache_dtype="fp8").runner.model.kv_scales is None
    e3 = _engine(weights=ck, kv_cache_dtype="fp8", kv_scales="one")
    assert e3.runner.model.kv_scales is None and e3.metrics()["kv_scales"]["source"] == "one"
    # a bf16 / fp32 cache never takes scales, whatever the checkpoint carries
    assert _engine(weights=ck).runner.model.kv_scales is None
    bad = str(tmp_path / "bad.json")
    with open(bad, "w") as f:
        json.dump({"k": [[1.0] * nkv] * cfg.num_layers, "v": [[0.0] * nkv] * cfg.num_layers}, f)
    with pytest.raises(ValueError):
        _engine(weights=ck2, kv_cache_dtype="fp8", kv_scales=bad)


def _prefill_logits(m, T, kv):
    bs = 16
    nblk = max(8, -(-T // bs))
    ids = torch.arange(100, 100 + T, dtype=torch.int32)
    tiles, _ = ops.build_prefill_tiles([T], ops.prefill_tile_tokens(m.nq, m.nkv))
    meta = AttnMeta(
        positions=torch.arange(T, dtype=torch.int32), slot_mapping=torch.arange(T, dtype=torch.int32),
        block_tables=torch.arange(nblk, dtype=torch.int32)[None],
        seq_lens=torch.tensor([T], dtype=torch.int32), logits_indices=torch.arange(T),
        q_start_loc=torch.tensor([0, T], dtype=torch.int32),
        tile_info=torch.tensor(tiles, dtype=torch.int32).flatten(), num_tiles=len(tiles))
    return m.compute_logits(m.forward(ids, meta, kv)).float()


def test_cpu_model_calibrated_scales_recover_outlier_heads(tmp_path):
    """tiny with K / V 1024x the random-init ones, 200-token prefill: fp8 KV at scale
    1.0 clips (cosine against fp32 KV far below 0.9), calibrated scales restore it."""
    cfg = MODELS["tiny"]
    T, bs = 200, 16
    nblk = max(8, -(-T // bs))
    ck = _save(cfg, tmp_path / "ck", None, outliers=True)
    m = LlamaModel(cfg, torch.device("cpu"), torch.float32, max_model_len=512).load_checkpoint(ck)
    kv = m.allocate_kv_cache(nblk, bs)
    truth = _prefill_logits(m, T, kv)
    assert min(min(k.abs().max().item(), v.abs().max().item()) for k, v in kv) > 4 * 448
    cos = lambda a: torch.nn.functional.cosine_similarity(a, truth, dim=-1).min().item()  # noqa: E731
    one = cos(_prefill_logits(m, T, m.allocate_kv_cache(nblk, bs, F8)))
    assert one < 0.9, one
    prompt = kv_calibrate.calibration_prompt_ids(ChatTemplate(get_tokenizer(None)),
                                                 vocab=cfg.vocab_size)
    ks, vs = kv_calibrate.calibrate(m, prompt)
    assert ks.shape == (cfg.num_layers, cfg.num_kv_heads) and ks.min().item() > 1
    got = _prefill_logits(m, T, m.allocate_kv_cache(nblk, bs, F8))
    assert cos(got) > 0.99, cos(got)
    agree = (got.argmax(-1) == truth.argmax(-1)).float().mean().item()
    assert agree >= 0.7, agree


def test_cpu_engine_serves_with_calibrate_and_prefix_cache(tmp_path):
    cfg = MODELS["tiny"]
    ck = _save(cfg, tmp_path / "ck", None, outliers=True)
    sp = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True)
    e = _engine(weights=ck, kv_cache_dtype="fp8", kv_scales="calibrate",
                enable_prefix_caching=True)
    info = e.metrics()["kv_scales"]
    assert info["source"] == "calibrate" and info["k_min"] > 1 and info["v_min"] > 1
    assert e.bm.num_free() == e.bm.num_blocks      # calibration left nothing in the pool
    base = list(range(1000, 1070))
    first = e.generate([base], sp)[0]
    turn2 = base + first + [128009, 128006, 882, 128007, 271, 40, 41, 42]
    with_cache = e.generate([turn2], sp)[0]
    assert e.bm.hits > 0
    e2 = _engine(weights=ck, kv_cache_dtype="fp8", kv_scales="calibrate",
                 enable_prefix_caching=False)
    assert e2.generate([turn2], sp)[0] == with_cache
    # TP > 1 asks for a calibration done once at TP=1
    m = LlamaModel(cfg, torch.device("cpu"), torch.float32, max_model_len=64)
    m.tp = 2
    with pytest.raises(ValueError, match="TP=1"):
        kv_calibrate.resolve(EngineConfig(kv_cache_dtype="fp8", kv_scales="calibrate"), cfg, m,
                             F8, 64)
