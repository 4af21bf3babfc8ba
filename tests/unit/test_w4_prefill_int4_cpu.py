"""W4A16 prefill on the int4 image, the parts that need no GPU: the CPU branch of
ops.quant.w4_packed_gemm, the EngineConfig.w4_prefill setting, the split plan of
models.llama.w4pg_cfg, and a CPU engine in int4 mode (the CPU backend holds
dequantized weights in every mode, so the tokens do not change)."""
import pytest
import torch

from fasttalk_llm_microservice_amd import ops
from fasttalk_llm_microservice_amd.engine.config import EngineConfig
from fasttalk_llm_microservice_amd.engine.engine import LLMEngine
from fasttalk_llm_microservice_amd.engine.sampling_params import SamplingParams
from fasttalk_llm_microservice_amd.models import llama
from fasttalk_llm_microservice_amd.models.config import MODELS
from fasttalk_llm_microservice_amd.ops import quant as Q


def _w4(n, k, seed=0, interleave=False):
    w = torch.randn(n, k, generator=torch.Generator().manual_seed(seed)) * 0.05
    if interleave:
        w = ops.interleave_gate_up(w, 1)
    q, z, s = Q.quantize_w4(w)
    return Q.pack_w4(q, z, s), Q.dequantize_w4(q, z, s)


def test_cpu_store_equals_dequant_matmul():
    W, wd = _w4(48, 256)
    x = torch.randn(70, 256, generator=torch.Generator().manual_seed(1))
    y = Q.w4_packed_gemm(x, W)
    assert y.shape == (70, 48) and y.dtype == x.dtype
    assert torch.allclose(y, x @ wd.t(), atol=1e-5, rtol=1e-5)
    out = torch.zeros(70, 64)
    assert Q.w4_packed_gemm(x, W, out=out[:, :48]) is not None
    assert torch.allclose(out[:, :48], x @ wd.t(), atol=1e-5, rtol=1e-5) and torch.all(out[:, 48:] == 0)


@pytest.mark.parametrize("splits", [1, 2])
def test_cpu_slabs_sum_to_dequant_matmul(splits):
    W, wd = _w4(32, 256, seed=2)
    x = torch.randn(66, 256, generator=torch.Generator().manual_seed(3))
    ws = torch.full((splits * 66 * 32 + 5,), float("nan"))
    r = Q.w4_packed_gemm(x, W, ws=ws, splits=splits, epi="slab")
    assert r is ws
    slabs = ws[:splits * 66 * 32].view(splits, 66, 32)
    assert torch.allclose(slabs.sum(0), x @ wd.t(), atol=1e-5, rtol=1e-5)


def test_cpu_silu_pairs_16_row_groups():
    inter = 48
    W, wd = _w4(2 * inter, 128, seed=4, interleave=True)
    x = torch.randn(65, 128, generator=torch.Generator().manual_seed(5))
    y = x @ wd.t()
    g, u = y.view(65, -1, 2, 16).unbind(2)
    ref = (torch.nn.functional.silu(g) * u).reshape(65, inter)
    h = Q.w4_packed_gemm(x, W, epi="silu")
    assert h.shape == (65, inter)
    assert torch.allclose(h, ref, atol=1e-5, rtol=1e-5)
    # the same pairing as w4_gemm's CPU branch
    assert torch.allclose(h, Q.w4_gemm(x, W, silu=True), atol=1e-5, rtol=1e-5)


def test_cpu_rejects_bad_arguments():
    W, _ = _w4(48, 256)
    x = torch.randn(3, 256)
    with pytest.raises(ValueError):
        Q.w4_packed_gemm(x, W, ws=torch.empty(3 * 3 * 48), splits=3, epi="slab")
    with pytest.raises(ValueError):
        Q.w4_packed_gemm(x, W, epi="silu")       # 48 % 32
    with pytest.raises(ValueError):
        Q.w4_packed_gemm(x, W, epi="slab")       # no workspace
    with pytest.raises(ValueError):
        Q.w4_packed_gemm(x, W, splits=2)         # splits without slabs


# --------------------------------------------------------------------- config

@pytest.mark.parametrize("mode", ["auto", "image", "scratch", "int4"])
def test_config_accepts_modes(mode):
    assert EngineConfig(w4_prefill=mode).w4_prefill == mode
    assert EngineConfig(w4_prefill=mode.upper()).w4_prefill == mode


@pytest.mark.parametrize("bad", ["bf16", "1", "int8", ""])
def test_config_rejects_other_values(bad):
    if bad == "":
        assert EngineConfig(w4_prefill=bad).w4_prefill == "auto"   # unset = default
        return
    with pytest.raises(ValueError):
        EngineConfig(w4_prefill=bad)


def test_default_is_auto():
    assert EngineConfig().w4_prefill == "auto"


def test_from_env_reads_engine_w4_prefill(monkeypatch):
    monkeypatch.delenv("ENGINE_W4_PREFILL", raising=False)
    assert EngineConfig.from_env(model="tiny").w4_prefill == "auto"
    monkeypatch.setenv("ENGINE_W4_PREFILL", "int4")
    assert EngineConfig.from_env(model="tiny").w4_prefill == "int4"
    assert EngineConfig.from_env(model="tiny", w4_prefill="scratch").w4_prefill == "scratch"
    monkeypatch.setenv("ENGINE_W4_PREFILL", "nope")
    with pytest.raises(ValueError):
        EngineConfig.from_env(model="tiny")
    monkeypatch.delenv("ENGINE_W4_PREFILL")
    with pytest.raises(ValueError):
        EngineConfig.from_env(model="tiny", w4_prefill="nope")


def test_model_resolves_mode(monkeypatch):
    cfg = MODELS["tiny"]
    monkeypatch.delenv("FT_W4_PREFILL_IMAGE", raising=False)
    mk = lambda **kw: llama.LlamaModel(cfg, torch.device("cpu"), torch.float32,  # noqa: E731
                                       max_model_len=64, quantization="w4", **kw)
    assert mk().w4_prefill == "auto"
    assert mk(w4_prefill="int4").w4_prefill == "int4"
    monkeypatch.setenv("FT_W4_PREFILL_IMAGE", "int4")
    assert mk().w4_prefill == "int4"
    assert mk(w4_prefill="image").w4_prefill == "image"    # the field wins over the variable
    monkeypatch.setenv("FT_W4_PREFILL_IMAGE", "0")
    assert mk().w4_prefill == "auto"
    with pytest.raises(ValueError):
        mk(w4_prefill="nope")
    # CPU backend: dequantized weights, no W4 mode to report
    m = mk(w4_prefill="int4").init_random(1, consistent=True)
    assert m.w4_prefill_mode() is None and not m.w4_int4 and m.layers[0].q4 is None


# --------------------------------------------------------------------- plan

def _proj_shapes(name, tp=1):
    c = MODELS[name]
    H, I = c.hidden_size, c.intermediate_size
    nqkv = (c.num_heads + 2 * c.num_kv_heads) * c.head_dim // tp
    return {"qkv": (nqkv, H), "o": (H, c.num_heads * c.head_dim // tp),
            "gu": (2 * I // tp, H), "down": (H, I // tp)}


@pytest.mark.parametrize("rows", [65, 145, 300, 512, 1024, 4096])
@pytest.mark.parametrize("name,tp", [("llama3-8b", 1), ("llama3-70b", 1), ("llama3-70b", 2),
                                     ("llama3-70b", 4), ("llama3-70b", 8)])
def test_w4pg_cfg_splits_divide_k_into_groups(name, tp, rows):
    for proj, (n, k) in _proj_shapes(name, tp).items():
        assert n % 16 == 0 and k % 128 == 0
        cfg, sp = llama.w4pg_cfg(proj, rows, n, k)
        assert cfg in (0, 1, 2) and sp >= 1 and k % (128 * sp) == 0, (proj, n, k, cfg, sp)
        # a workspace too small for the slabs halves the splits down to the store path
        cfg2, sp2 = llama.w4pg_cfg(proj, rows, n, k, ws_elems=rows * n)
        assert cfg2 == cfg and sp2 == 1
        cfg3, sp3 = llama.w4pg_cfg(proj, rows, n, k, ws_elems=2 * rows * n)
        assert sp3 <= 2 and k % (128 * sp3) == 0


def test_plan_rows_cover_everything():
    for proj, plan in llama.W4PG_PLAN.items():
        lims = [lim for lim, _, _ in plan]
        assert lims == sorted(lims) and lims[-1] >= 1 << 30, proj
        assert all(cfg in (0, 1, 2) and sp >= 1 and sp & (sp - 1) == 0 for _, cfg, sp in plan)


# --------------------------------------------------------------------- engine

def _engine(**kw):
    base = dict(model="tiny", device="cpu", num_kv_blocks=256, max_model_len=1024, max_num_seqs=4)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def test_cpu_engine_int4_mode_same_tokens_as_auto():
    sp = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)
    prompts = [list(range(100, 170)), list(range(300, 305))]
    a = _engine(quantization="w4")
    b = _engine(quantization="w4", w4_prefill="int4")
    assert a.generate(prompts, sp) == b.generate(prompts, sp)
    ma, mb = a.metrics(), b.metrics()
    assert "w4_prefill" not in ma and "w4_prefill" not in mb      # GPU W4 engines only
    assert ma["weights_resident_gb"] == mb["weights_resident_gb"] > 0
    m = b.runner.model
    want = sum(t.numel() * t.element_size() for L in m.layers
               for t in (L.wqkv, L.wo, L.wgu, L.wd, L.ln1, L.ln2))
    want += m.embed.numel() * m.embed.element_size() + m.norm.numel() * m.norm.element_size()
    if m.lm_head.untyped_storage().data_ptr() != m.embed.untyped_storage().data_ptr():
        want += m.lm_head.numel() * m.lm_head.element_size()
    assert m.weights_resident_bytes() == want
