"""W8A16 (fp8 e4m3 weights, per-channel scales) without a GPU: quantization and its error
bound, the fragment image round trip, the CPU fallbacks against the numerics contract
(y = s[n] * sum_k x q, reference x.double() @ (q.double() * s.double()[:, None]).t()),
the fp8 checkpoint loader, the plans, and the tiny CPU engine."""
import pytest
import torch

from fasttalk_llm_microservice_amd import ops
from fasttalk_llm_microservice_amd.engine.config import EngineConfig
from fasttalk_llm_microservice_amd.engine.engine import LLMEngine
from fasttalk_llm_microservice_amd.engine.sampling_params import SamplingParams
from fasttalk_llm_microservice_amd.models import llama
from fasttalk_llm_microservice_amd.models import weights as W
from fasttalk_llm_microservice_amd.models.config import MODELS
from fasttalk_llm_microservice_amd.ops import exact as E
from fasttalk_llm_microservice_amd.ops import quant as Q


def _rand(n, k, seed=0, std=0.05):
    return torch.randn(n, k, generator=torch.Generator().manual_seed(seed)) * std


# --------------------------------------------------------------------- format facts
def test_every_e4m3_value_is_exact_in_bf16_and_integers_to_16():
    b = torch.arange(256, dtype=torch.uint8)
    finite = b[~Q.fp8_nan_bytes(b)]
    assert finite.numel() == 254
    v = finite.view(Q.FP8).double()
    assert torch.equal(v.to(torch.bfloat16).double(), v)
    assert float(v.abs().max()) == Q.FP8_MAX
    ints = torch.arange(-16, 17).double()
    assert torch.equal(ints.to(Q.FP8).double(), ints)


# --------------------------------------------------------------------- quantize
def test_quantize_error_bound_extremes_zero_rows_and_no_nan():
    w = _rand(96, 256, seed=1)
    w[5] = 0.0                                   # an all-zero row
    w[6] *= 1e-6                                 # tiny values: subnormal q
    w[7, 3] = 40.0                               # one outlier: the rest of the row near zero
    w[8] = 1e30                                  # far outside the format before scaling
    q, s = Q.quantize_w8(w)
    assert q.dtype == Q.FP8 and s.dtype == torch.float32 and s.shape == (96,)
    assert not bool(Q.fp8_nan_bytes(q).any())
    assert bool(torch.isfinite(s).all()) and bool((s > 0).all())
    assert float(s[5]) == 1.0 and bool((q[5].float() == 0).all())
    wd, sd = w.double(), s.double().unsqueeze(-1)
    err = (wd - q.double() * sd).abs()
    # 3 mantissa bits (half an ulp of a normal: 2**-4 relative) and a smallest subnormal
    # of 2**-9 (half a step: 2**-10 of the scale)
    bound = 2.0 ** -4 * wd.abs() + 2.0 ** -10 * sd
    assert bool((err <= bound).all()), float((err - bound).max())
    # rows holding +-absmax map to +-448
    qa = q.double().abs().amax(-1)
    nz = wd.abs().amax(-1) > 0
    assert bool((qa[nz] == Q.FP8_MAX).all())
    i = wd.abs().argmax(-1)
    assert torch.equal(torch.sign(q.double()[torch.arange(96), i])[nz],
                       torch.sign(wd[torch.arange(96), i])[nz])
    # s = absmax / 448 in fp64, rounded to fp32
    assert torch.equal(s[nz], (wd.abs().amax(-1) / 448.0).float()[nz])


def test_quantize_from_bf16_and_fp32_inputs_agree_on_equal_values():
    w = _rand(32, 128, seed=2).bfloat16()
    qa, sa = Q.quantize_w8(w)
    qb, sb = Q.quantize_w8(w.float())
    assert torch.equal(qa.view(torch.uint8), qb.view(torch.uint8)) and torch.equal(sa, sb)


# --------------------------------------------------------------------- image
@pytest.mark.parametrize("gate_up", [False, True])
def test_pack_unpack_round_trip_bit_for_bit(gate_up):
    n, k = 96, 192
    q = torch.randint(0, 256, (n, k), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    q[Q.fp8_nan_bytes(q)] = 0
    s = torch.rand(n, generator=torch.Generator().manual_seed(4)) + 0.5
    w = Q.pack_w8(q.view(Q.FP8), s, gate_up=gate_up)
    assert w.wq.dtype == torch.uint8 and w.wq.numel() == n * k and w.shape == (n, k)
    assert w.nbytes() == n * k + 4 * n
    q2, s2 = Q.unpack_w8(w, gate_up=gate_up)
    assert torch.equal(q2.view(torch.uint8), q) and torch.equal(s2, s)
    if gate_up:   # the image rows are interleave_gate_up(w, 1)'s, scales alike
        qi, si = Q.unpack_w8(w)
        assert torch.equal(qi.view(torch.uint8), ops.interleave_gate_up(q, 1))
        assert torch.equal(si, ops.interleave_gate_up(s.view(-1, 1), 1).view(-1))


def test_image_layout_is_the_documented_one():
    """Byte 8 * half + e of lane (g, r) in block (tile, step) is q[16 tile + r,
    64 step + 16 g + 8 half + e]: a lane's 16 bytes are 16 consecutive k."""
    n, k = 32, 128
    q = (torch.arange(n * k) % 251).to(torch.uint8).view(n, k)
    q[Q.fp8_nan_bytes(q)] = 1
    img = Q.pack_w8(q.view(Q.FP8), torch.ones(n)).wq.view(n // 16, k // 64, 4, 16, 16)
    for tile, step, g, r in [(0, 0, 0, 0), (1, 1, 3, 15), (0, 1, 2, 7), (1, 0, 1, 9)]:
        k0 = 64 * step + 16 * g
        assert torch.equal(img[tile, step, g, r], q[16 * tile + r, k0:k0 + 16])


@pytest.mark.parametrize("n,k", [(24, 128), (32, 96), (8, 64), (32, 32)])
def test_pack_rejects_shapes_the_image_cannot_hold(n, k):
    with pytest.raises(ValueError):
        Q.pack_w8(torch.zeros(n, k).to(Q.FP8), torch.ones(n))


def test_pack_rejects_other_dtypes_and_odd_gate_up():
    with pytest.raises(ValueError):
        Q.pack_w8(torch.zeros(32, 64, dtype=torch.uint8), torch.ones(32))
    with pytest.raises(ValueError):
        Q.pack_w8(torch.zeros(48, 64).to(Q.FP8), torch.ones(48), gate_up=True)


# --------------------------------------------------------------------- CPU GEMMs
def _contract(x, q, s):
    return x.double() @ (q.double() * s.double().unsqueeze(-1)).t()


@pytest.mark.parametrize("fn", ["decode", "packed"])
def test_cpu_gemms_match_the_contract_for_every_epilogue(fn):
    m = 33 if fn == "decode" else 150
    n, k, inter = 272, 512, 272
    x = _rand(m, k, seed=5, std=1.0).bfloat16()
    q, s = Q.quantize_w8(_rand(n, k, seed=6))
    Wt = Q.pack_w8(q, s)
    ref = _contract(x, q, s)
    gemm = Q.w8_gemm if fn == "decode" else Q.w8_packed_gemm
    slab_kw = (lambda ws, sp: dict(ws=ws, splits=sp)) if fn == "decode" else \
        (lambda ws, sp: dict(ws=ws, splits=sp, epi="slab"))
    y = gemm(x, Wt)
    assert y.dtype == torch.bfloat16 and y.shape == (m, n)
    # fp32 contract + one bf16 rounding: 2**-8 relative, on |ref| <= ~20
    assert float((y.double() - ref).abs().max()) <= 2.0 ** -8 * float(ref.abs().max()) + 1e-3
    for sp in (1, 2):
        ws = torch.full((sp * m * n + 7,), float("nan"))
        r = gemm(x, Wt, **slab_kw(ws, sp))
        assert r is ws and bool(torch.isnan(ws[sp * m * n:]).all())
        got = ws[:sp * m * n].view(sp, m, n).sum(0).double()
        assert float((got - ref).abs().max()) <= 1e-3 * float(ref.abs().max()) + 1e-3
    qg, sg = Q.quantize_w8(_rand(2 * inter, k, seed=7))
    Wg = Q.pack_w8(qg, sg, gate_up=True)
    yg = _contract(x, qg, sg)
    href = (torch.nn.functional.silu(yg[:, :inter]) * yg[:, inter:])
    h = gemm(x, Wg, nt=2, silu=True) if fn == "decode" else gemm(x, Wg, epi="silu")
    assert h.shape == (m, inter) and h.dtype == torch.bfloat16
    assert float((h.double() - href).abs().max()) <= 2e-2 * float(href.abs().max()) + 1e-2
    out = torch.zeros(m + 3, n + 8, dtype=torch.bfloat16)
    r = gemm(x, Wt, out=out)
    assert r is out and torch.equal(out[:m, :n], y) and bool((out[m:] == 0).all())


def test_cpu_gemms_are_exact_on_integer_operands():
    x, q, s, exact = E.w8_int_operands(40, 272, 1024, seed=9)
    assert len(set(s.tolist())) == 3
    Wt = Q.pack_w8(q, s)
    ws = torch.empty(2 * 40 * 272)
    Q.w8_gemm(x, Wt, ws=ws, splits=2)
    assert torch.equal(ws.view(2, 40, 272).sum(0).double(), exact)
    assert torch.equal(Q.w8_packed_gemm(x, Wt), exact.to(torch.bfloat16))


def test_gemm_wrappers_reject_bad_arguments():
    x = torch.zeros(8, 512, dtype=torch.bfloat16)
    q, s = Q.quantize_w8(_rand(528, 512))
    Wt = Q.pack_w8(q, s)
    ws = torch.zeros(4 * 65 * 528)
    for kw in (dict(splits=3, ws=ws), dict(splits=4, ws=ws), dict(nt=3), dict(splits=2),
               dict(silu=True), dict(silu=True, nt=4), dict(ws=ws[:100])):
        with pytest.raises(ValueError):
            Q.w8_gemm(x, Wt, **kw)
    with pytest.raises(ValueError):
        Q.w8_gemm(torch.zeros(65, 512, dtype=torch.bfloat16), Wt)
    for kw in (dict(splits=16, ws=ws, epi="slab"), dict(splits=2), dict(epi="slab"), dict(epi="silu"),
               dict(cfg=1), dict(ws=ws[:100], epi="slab")):
        with pytest.raises(ValueError):
            Q.w8_packed_gemm(x, Wt, **kw)


# --------------------------------------------------------------------- plans
def _proj_shapes(name):
    c = MODELS[name]
    H, I = c.hidden_size, c.intermediate_size
    return {"qkv": ((c.num_heads + 2 * c.num_kv_heads) * c.head_dim, H), "o": (H, c.num_heads * c.head_dim),
            "gu": (2 * I, H), "down": (H, I)}


@pytest.mark.parametrize("name", ["tiny", "tiny-2k", "llama3-8b", "llama3-70b"])
def test_plans_fit_the_kernels(name):
    for proj, (n, k) in _proj_shapes(name).items():
        assert n % 16 == 0 and k % 256 == 0
        for rows in (1, 8, 9, 16, 32, 50, 64):
            nt, sp = llama.w8_cfg(proj, rows, n, k)
            assert nt in Q.W8_NTS and sp >= 1 and k % (256 * sp) == 0
            assert proj != "gu" or (nt, sp) == (2, 1)       # the SiLU epilogue
        for rows in (65, 145, 300, 512, 1024, 4096):
            cfg, sp = llama.w8pg_cfg(proj, rows, n, k)
            assert cfg == 0 and sp >= 1 and k % (64 * sp) == 0
            assert llama.w8pg_cfg(proj, rows, n, k, ws_elems=rows * n)[1] == 1
    for plan in llama.W8PG_PLAN.values():
        lims = [lim for lim, _, _ in plan]
        assert lims == sorted(lims) and lims[-1] >= 1 << 30


# --------------------------------------------------------------------- checkpoints
def _tiny_full(seed=0):
    cfg = MODELS["tiny"]
    g = torch.Generator().manual_seed(seed)
    layers = [W.random_full_layer(cfg, g, 0.02, torch.bfloat16) for _ in range(cfg.num_layers)]
    embed = (torch.randn(cfg.vocab_size, cfg.hidden_size, generator=g) * 0.02).bfloat16()
    norm = torch.ones(cfg.hidden_size, dtype=torch.bfloat16)
    return cfg, layers, embed, norm


def test_fp8_checkpoint_round_trip_channel_scales(tmp_path):
    cfg, layers, embed, norm = _tiny_full()
    W.save_fp8_checkpoint(cfg, layers, embed, norm, None, str(tmp_path), input_scale=True)
    idx = W.SafetensorsIndex(str(tmp_path))
    assert W.is_fp8_checkpoint(idx) and not W.is_awq_checkpoint(idx)
    for li, L in enumerate(layers):
        sh = W.load_fp8_layer(cfg, idx, li)
        for attr, names in (("wqkv", "qkv"), ("wo", "o"), ("wgu", ("gate", "up")), ("wd", ("down",))):
            qs = [Q.quantize_w8(L[n]) for n in names]
            q, s = sh[attr]
            assert q.dtype == Q.FP8 and s.dtype == torch.float32 and s.shape == (q.shape[0],)
            assert torch.equal(q.view(torch.uint8), torch.cat([a.view(torch.uint8) for a, _ in qs]))
            assert torch.equal(s, torch.cat([b for _, b in qs]))
        assert torch.equal(sh["ln1"], L["ln1"])


@pytest.mark.parametrize("form", ["channel2d", "tensor", "tensor1"])
def test_fp8_scale_forms_broadcast_to_channels(tmp_path, form):
    cfg, layers, embed, norm = _tiny_full(1)
    for i, n in enumerate(("q", "k", "v")):          # three different per-tensor scales
        layers[0][n] = layers[0][n] * (1.0 + i)
    W.save_fp8_checkpoint(cfg, layers, embed, norm, None, str(tmp_path), scale_form=form)
    idx = W.SafetensorsIndex(str(tmp_path))
    raw = idx.get("model.layers.0.self_attn.q_proj.weight_scale")
    assert tuple(raw.shape) == {"channel2d": (512, 1), "tensor": (), "tensor1": (1,)}[form]
    q, s = W.load_fp8_layer(cfg, idx, 0)["wqkv"]
    assert s.shape == (768,) and q.shape == (768, 512)
    if form != "channel2d":
        parts = [float(idx.get(f"model.layers.0.self_attn.{n}_proj.weight_scale").flatten()[0])
                 for n in "qkv"]
        assert len(set(parts)) == 3
        want = torch.cat([torch.full((512,), parts[0]), torch.full((128,), parts[1]),
                          torch.full((128,), parts[2])])
        assert torch.equal(s, want)
    # the fused weights still dequantize to the originals within the format's error
    w = torch.cat([layers[0][n] for n in "qkv"]).double()
    err = (w - Q.dequantize_w8(q, s, torch.float64)).abs()
    assert bool((err <= 2.0 ** -4 * w.abs() + 2.0 ** -10 * s.double().unsqueeze(-1)).all())


def _rewrite(tmp_path, name, fn):
    from safetensors.torch import load_file, save_file

    path = str(tmp_path / "model.safetensors")
    t = load_file(path)
    t[name] = fn(t[name])
    save_file(t, path)


def test_fp8_loader_refuses_bad_scales_and_nan_bytes(tmp_path):
    cfg, layers, embed, norm = _tiny_full(2)
    W.save_fp8_checkpoint(cfg, layers, embed, norm, None, str(tmp_path))
    name = "model.layers.1.mlp.down_proj.weight_scale"
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        def poke(t, bad=bad):
            t = t.clone()
            t[3] = bad
            return t
        _rewrite(tmp_path, name, poke)
        with pytest.raises(ValueError, match="finite and positive"):
            W.load_fp8_layer(cfg, W.SafetensorsIndex(str(tmp_path)), 1)
    _rewrite(tmp_path, name, lambda t: torch.ones_like(t))
    W.load_fp8_layer(cfg, W.SafetensorsIndex(str(tmp_path)), 1)
    _rewrite(tmp_path, name, lambda t: torch.ones(7))
    with pytest.raises(ValueError, match="expected 1 or"):
        W.load_fp8_layer(cfg, W.SafetensorsIndex(str(tmp_path)), 1)
    _rewrite(tmp_path, name, lambda t: torch.ones(512))

    def nan_byte(t):
        b = t.view(torch.uint8).clone()
        b[2, 5] = 0x7F
        return b.view(Q.FP8)
    _rewrite(tmp_path, "model.layers.1.self_attn.o_proj.weight", nan_byte)
    with pytest.raises(ValueError, match="NaN"):
        W.load_fp8_layer(cfg, W.SafetensorsIndex(str(tmp_path)), 1)


def test_model_loads_fp8_checkpoint_and_selects_fp8(tmp_path):
    cfg, layers, embed, norm = _tiny_full(3)
    W.save_fp8_checkpoint(cfg, layers, embed, norm, None, str(tmp_path))
    m = llama.LlamaModel(cfg, torch.device("cpu"), torch.float32, max_model_len=64)
    assert m.quant is None
    m.load_checkpoint(str(tmp_path))
    assert m.quant == "fp8" and m.layers[0].q8 is None          # CPU: dequantized weights
    q, s = Q.quantize_w8(torch.cat([layers[0][n] for n in "qkv"]))
    assert torch.equal(m.layers[0].wqkv, Q.dequantize_w8(q, s))
    # the same weights as quantizing the bf16 checkpoint at load time
    r = llama.LlamaModel(cfg, torch.device("cpu"), torch.float32, max_model_len=64, quantization="fp8")
    r._set_layers([W.shard_full_layer(cfg, L, 0, 1) for L in layers])
    r._quantize_layers()
    for a, b in zip(m.layers, r.layers):
        for attr in ("wqkv", "wo", "wgu", "wd"):
            assert torch.equal(getattr(a, attr), getattr(b, attr))
    with pytest.raises(ValueError):   # an fp8 checkpoint under another quantization
        llama.LlamaModel(cfg, torch.device("cpu"), torch.float32, max_model_len=64,
                         quantization="w4").load_checkpoint(str(tmp_path))


def test_unknown_quantization_raises():
    with pytest.raises(ValueError, match="unsupported quantization"):
        llama.LlamaModel(MODELS["tiny"], torch.device("cpu"), torch.float32, quantization="fp4")
    with pytest.raises(ValueError, match="unsupported quantization"):
        llama.LlamaModel(MODELS["tiny"], torch.device("cpu"), torch.float32, quantization="int8")


# --------------------------------------------------------------------- engine
def _engine(**kw):
    base = dict(model="tiny", device="cpu", num_kv_blocks=256, max_model_len=1024, max_num_seqs=4)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def test_cpu_engine_fp8_generates_deterministically_and_reports_it():
    prompts = [list(range(100, 170)), list(range(300, 305))]
    greedy = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)
    seeded = SamplingParams(temperature=0.8, top_p=0.9, seed=11, max_tokens=6, ignore_eos=True)
    a, b, plain = _engine(quantization="fp8"), _engine(quantization="FP8"), _engine()
    out = a.generate(prompts, greedy)
    assert all(len(o) == 6 for o in out) and out == b.generate(prompts, greedy)
    assert a.generate(prompts, seeded) == b.generate(prompts, seeded)
    assert all(len(o) == 6 for o in plain.generate(prompts, greedy))
    ma, mp = a.metrics(), plain.metrics()
    assert ma["quantization"] == "fp8" and "quantization" not in mp
    assert set(ma) - set(mp) == {"quantization"}
    assert ma["weights_resident_gb"] > 0
    m = a.runner.model
    assert m.quant == "fp8" and all(L.q8 is None for L in m.layers)
    # the CPU backend holds dequantize_w8 of the quantized bf16 weights
    p = plain.runner.model
    q, s = Q.quantize_w8(p.layers[1].wd.to(torch.bfloat16))
    assert torch.equal(m.layers[1].wd, Q.dequantize_w8(q, s).to(m.dtype))
    assert plain.runner.model.quant is None and all(L.q8 is None for L in p.layers)


def test_fp8_refuses_tensor_parallel_and_batch_invariant(monkeypatch):
    with pytest.raises(ValueError, match="tensor parallel"):
        EngineConfig(model="tiny", device="cpu", quantization="fp8", tp_size=2)
    with pytest.raises(ValueError, match="batch-invariant"):
        EngineConfig(model="tiny", device="cpu", quantization="fp8", batch_invariant=True)
    monkeypatch.setenv("ENGINE_QUANTIZATION", "fp8")
    assert EngineConfig.from_env(model="tiny").quantization == "fp8"
    monkeypatch.setenv("ENGINE_BATCH_INVARIANT", "1")
    with pytest.raises(ValueError, match="batch-invariant"):
        EngineConfig.from_env(model="tiny")
    monkeypatch.delenv("ENGINE_BATCH_INVARIANT")
    monkeypatch.delenv("ENGINE_QUANTIZATION")
    monkeypatch.setenv("VLLM_QUANTIZATION", "fp8")
    with pytest.raises(ValueError, match="tensor parallel"):
        EngineConfig.from_env(model="tiny", tp_size=2)
    m = llama.LlamaModel(MODELS["tiny"], torch.device("cpu"), torch.float32, quantization="fp8")
    m.init_random(1, consistent=True)
    with pytest.raises(ValueError):
        m.set_batch_invariant(64)
