"""MXFP4 (OCP MX e2m1 weights, one e8m0 scale per 32 k-values) without a GPU: the format's
exactness in bf16, the quantizer (OCP MX rule, ties to even, saturation), the fragment
image against its documented formula, the CPU fallbacks against the numerics contract
(y = x dequant(W)^T, reference in fp64), the checkpoint loader, the plans, and the tiny
CPU engine."""
import pytest
import torch

from fasttalk_llm_microservice_amd.engine.config import EngineConfig
from fasttalk_llm_microservice_amd.engine.engine import LLMEngine
from fasttalk_llm_microservice_amd.engine.sampling_params import SamplingParams
from fasttalk_llm_microservice_amd.models import llama
from fasttalk_llm_microservice_amd.models import weights as W
from fasttalk_llm_microservice_amd.models.config import MODELS
from fasttalk_llm_microservice_amd.ops import exact as E
from fasttalk_llm_microservice_amd.ops import quant as Q

GRID = torch.tensor(Q.MX4_GRID, dtype=torch.float64)


def _rand(n, k, seed=0, std=0.05):
    return torch.randn(n, k, generator=torch.Generator().manual_seed(seed)) * std


# --------------------------------------------------------------------- format facts
def test_constants():
    assert Q.MX4_BLOCK == 32 and Q.MX4_KSTEP == 128 and llama.MX4_ROWS == 64


def test_every_code_times_every_edge_scale_is_exact_in_bf16():
    sbs = [2, 100, 127, 140, 252]
    codes = (torch.arange(32) % 16).to(torch.uint8).repeat(len(sbs), 1)       # [5, 32]
    sb = torch.tensor(sbs, dtype=torch.uint8).view(-1, 1)
    v = Q.dequantize_mx4(codes, sb, torch.float64)
    want = torch.cat([GRID, -GRID]).repeat(2).unsqueeze(0) * torch.pow(
        2.0, torch.tensor(sbs, dtype=torch.float64) - 127).unsqueeze(-1)
    assert torch.equal(v, want)
    assert bool(torch.isfinite(v).all())
    b = v.to(torch.bfloat16)
    assert torch.equal(b.double(), v)                       # exact in bf16
    assert torch.equal(Q.dequantize_mx4(codes, sb, torch.bfloat16), b)
    assert torch.equal(Q.dequantize_mx4(codes, sb).double(), v)
    # normal, not denormal: the smallest non-zero magnitude is 2^-126
    assert float(v[0].abs()[v[0] != 0].min()) == 2.0 ** -126
    assert Q.MX4Weight(torch.zeros(64, dtype=torch.uint8), torch.zeros(8, dtype=torch.uint8), 16, 8).nbytes() == 72


# --------------------------------------------------------------------- quantize
def test_quantizer_error_bound_scale_rule_and_saturation():
    w = _rand(96, 256, seed=1).double()
    w[7, 3] = 40.0                               # an outlier: its block's scale follows it
    codes, sb = Q.quantize_mx4(w)
    assert codes.dtype == torch.uint8 and sb.dtype == torch.uint8
    assert codes.shape == (96, 256) and sb.shape == (96, 8) and int(codes.max()) <= 15
    blk = w.view(96, 8, 32)
    amax = blk.abs().amax(-1)
    e = torch.floor(torch.log2(amax)) - 2        # the OCP MX rule
    assert torch.equal(sb.double() - 127, e)
    scale = torch.pow(2.0, e).unsqueeze(-1)
    d = Q.dequantize_mx4(codes, sb, torch.float64).view(96, 8, 32)
    a = blk.abs() / scale
    # inside +-6 scale: at most half a grid step (0.25 below 2, 0.5 below 4, 1 up to 6)
    half = torch.where(a <= 2, 0.25, torch.where(a <= 4, 0.5, 1.0)) * scale
    inside = a <= 6
    assert bool(((d - blk).abs()[inside] <= half[inside]).all())
    # (6, 8) scale saturates to +-6 scale
    assert bool((~inside).any())
    assert torch.equal(d[~inside], (torch.sign(blk) * 6 * scale)[~inside])
    # about 11% relative error on Gaussian weights
    g = _rand(256, 512, seed=2).double()
    r = (Q.dequantize_mx4(*Q.quantize_mx4(g), torch.float64) - g).norm() / g.norm()
    assert 0.08 < float(r) < 0.14


def test_quantizer_zero_blocks_ties_clamped_exponents_and_input_dtypes():
    w = torch.zeros(2, 64, dtype=torch.float64)
    # block (0, 0): absmax 5 -> exponent 0; the seven midpoints of the grid, then plain values
    w[0, :8] = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 4.0])
    w[0, 8:16] = -w[0, :8]
    codes, sb = Q.quantize_mx4(w)
    assert sb.tolist() == [[127, 127], [127, 127]]                      # zero blocks: byte 127
    assert codes[0, :8].tolist() == [0, 2, 2, 4, 4, 6, 6, 6]            # ties to the even code
    assert codes[0, 8:16].tolist() == [0, 10, 10, 12, 12, 14, 14, 14]   # a rounded-away -0.25 is +0
    assert int(codes[1].max()) == 0 and int(codes[0, 16:].max()) == 0
    # exponents beyond the accepted byte range are clamped into it
    tiny = torch.full((1, 32), 2.0 ** -140, dtype=torch.float64)
    huge = torch.full((1, 32), 1.75 * 2.0 ** 127, dtype=torch.float32)   # 7 * 2^125: saturates
    assert Q.quantize_mx4(tiny)[1].tolist() == [[2]]
    c, s = Q.quantize_mx4(huge)
    assert s.tolist() == [[252]] and int(c.max()) == 7
    # bf16 and fp32 inputs of equal value agree
    wb = _rand(32, 128, seed=4).bfloat16()
    a, b = Q.quantize_mx4(wb), Q.quantize_mx4(wb.float())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for bad in (float("nan"), float("inf"), -float("inf")):
        w = _rand(16, 64)
        w[3, 5] = bad
        with pytest.raises(ValueError, match="NaN or Inf"):
            Q.quantize_mx4(w)
    with pytest.raises(ValueError):
        Q.quantize_mx4(torch.zeros(4, 48))


# --------------------------------------------------------------------- image
@pytest.mark.parametrize("gate_up", [False, True])
def test_pack_unpack_round_trip(gate_up):
    codes, sb = Q.quantize_mx4(_rand(64, 384, seed=5))
    Wt = Q.pack_mx4(codes, sb, gate_up=gate_up)
    assert Wt.wq.dtype == torch.uint8 and Wt.wq.numel() == 64 * 384 // 2
    assert Wt.sc.dtype == torch.uint8 and Wt.sc.numel() == 64 * 384 // 32
    assert Wt.nbytes() == 64 * 384 // 2 + 64 * 384 // 32 and Wt.shape == (64, 384)
    c2, s2 = Q.unpack_mx4(Wt, gate_up=gate_up)
    assert torch.equal(c2, codes) and torch.equal(s2, sb)
    if gate_up:   # image row 16 + r is up row r
        c3, s3 = Q.unpack_mx4(Wt)
        assert torch.equal(c3[16:32], codes[32:48]) and torch.equal(s3[16:32], sb[32:48])
        assert torch.equal(c3[32:48], codes[16:32])


def test_image_layout_matches_the_documented_formula():
    n, k = 32, 256
    g = torch.Generator().manual_seed(6)
    codes = torch.randint(0, 16, (n, k), generator=g, dtype=torch.uint8)
    sb = torch.randint(2, 253, (n, k // 32), generator=g, dtype=torch.uint8)
    Wt = Q.pack_mx4(codes, sb)
    wq = Wt.wq.view(n // 16, k // 128, 64, 16)
    sc = Wt.sc.view(n // 16, k // 128, 64)
    for tile in range(n // 16):
        for st in range(k // 128):
            for lane in range(64):
                gg, r = lane >> 4, lane & 15
                col = 16 * tile + r
                assert int(sc[tile, st, lane]) == int(sb[col, 4 * st + gg])
                for j in range(4):
                    for e in range(8):
                        kk = 128 * st + 32 * gg + 8 * j + e
                        byte = int(wq[tile, st, lane, 4 * j + e // 2])
                        nib = (byte >> 4) if e & 1 else (byte & 0xF)   # low nibble first
                        assert nib == int(codes[col, kk]), (tile, st, lane, j, e)


def test_pack_refuses_bad_shapes_and_scale_bytes():
    c = torch.zeros(32, 256, dtype=torch.uint8)
    s = torch.full((32, 8), 127, dtype=torch.uint8)
    Q.pack_mx4(c, s)
    with pytest.raises(ValueError, match="N % 16"):
        Q.pack_mx4(c[:24], s[:24])
    with pytest.raises(ValueError, match="K % 128"):
        Q.pack_mx4(c[:, :192], s[:, :6])
    with pytest.raises(ValueError, match="gate_up"):
        Q.pack_mx4(c[:16], s[:16], gate_up=True)
    with pytest.raises(ValueError):
        Q.pack_mx4(c, s[:, :7])
    with pytest.raises(ValueError):
        Q.pack_mx4(c + 16, s)
    for bad in (0, 1, 253, 255):
        sbad = s.clone()
        sbad[5, 3] = bad
        with pytest.raises(ValueError, match=r"down_proj\.weight_scale.*byte " + str(bad)):
            Q.pack_mx4(c, sbad, name="down_proj.weight_scale")
    for ok in (2, 252):
        sok = s.clone()
        sok[5, 3] = ok
        Q.pack_mx4(c, sok)


def test_checkpoint_layout_conversion():
    codes, sb = Q.quantize_mx4(_rand(16, 64, seed=7))
    wb, s2 = Q.mx4_to_packed(codes, sb)
    assert wb.shape == (16, 32) and wb.dtype == torch.uint8
    assert torch.equal(wb & 0xF, codes[:, 0::2]) and torch.equal(wb >> 4, codes[:, 1::2])
    c2, s3 = Q.mx4_from_packed(wb, s2)
    assert torch.equal(c2, codes) and torch.equal(s3, sb)
    c4, s4 = Q.mx4_from_packed(wb.view(torch.float4_e2m1fn_x2), s2.view(torch.float8_e8m0fnu))
    assert torch.equal(c4, codes) and torch.equal(s4, sb) and s4.dtype == torch.uint8


# --------------------------------------------------------------------- CPU GEMMs
def test_cpu_gemms_match_the_contract_for_every_epilogue():
    m, inter, k = 9, 48, 512
    codes, sb = Q.quantize_mx4(_rand(2 * inter, k, seed=8))
    x = _rand(m, k, seed=9, std=1.0).bfloat16()
    ref = x.double() @ Q.dequantize_mx4(codes, sb, torch.float64).t()
    Wt = Q.pack_mx4(codes, sb)
    for fn, kw in ((Q.mx4_gemm, {}), (Q.mx4_packed_gemm, {})):
        y = fn(x, Wt, **kw)
        assert y.dtype == torch.bfloat16 and y.shape == (m, 2 * inter)
        assert float((y.double() - ref).abs().max()) <= 2.0 ** -8 * float(ref.abs().max()) + 1e-6
    ws = torch.full((4 * m * 2 * inter + 5,), float("nan"))
    assert Q.mx4_gemm(x, Wt, ws=ws, splits=2) is ws
    slabs = ws[:2 * m * 2 * inter].view(2, m, 2 * inter)
    assert float((slabs.sum(0).double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    ws.fill_(float("nan"))
    assert Q.mx4_packed_gemm(x, Wt, ws=ws, splits=4, epi="slab") is ws
    assert float((ws[:4 * m * 2 * inter].view(4, m, -1).sum(0).double() - ref).abs().max()) <= \
        1e-5 * float(ref.abs().max())
    assert bool(torch.isnan(ws[4 * m * 2 * inter:]).all())
    Wg = Q.pack_mx4(codes, sb, gate_up=True)
    gt, up = ref[:, :inter], ref[:, inter:]
    href = gt / (1.0 + torch.exp(-gt)) * up
    out = torch.zeros(m + 2, inter + 3, dtype=torch.bfloat16)
    for h in (Q.mx4_gemm(x, Wg, nt=2, silu=True), Q.mx4_packed_gemm(x, Wg, epi="silu"),
              Q.mx4_gemm(x, Wg, out=out, nt=2, silu=True)[:m, :inter]):
        assert h.shape == (m, inter)
        assert float((h.double() - href).abs().max()) <= 2.0 ** -7 * float(href.abs().max()) + 1e-6
    assert float(out[m:].abs().max()) == 0 and float(out[:, inter:].abs().max()) == 0


def test_cpu_gemms_are_exact_on_integer_operands():
    x, c, s, exact = E.mx4_int_operands(40, 272, 1024, seed=9)
    assert sorted(set(s.flatten().tolist())) == [125, 127, 129]          # two octaves apart
    assert sorted(set(c.flatten().tolist())) == list(range(16))
    Wt = Q.pack_mx4(c, s)
    ws = torch.empty(2 * 40 * 272)
    Q.mx4_gemm(x, Wt, ws=ws, splits=2)
    assert torch.equal(ws.view(2, 40, 272).sum(0).double(), exact)
    assert torch.equal(Q.mx4_packed_gemm(x, Wt), exact.to(torch.bfloat16))


@pytest.mark.parametrize("m,n,k", [(64, 272, 2048), (300, 528, 1024), (1, 272, 256), (65, 272, 128)])
def test_exact_bound_holds_at_the_shapes_the_gpu_tests_use(m, n, k):
    x, c, s, exact = E.mx4_int_operands(m, n, k, seed=m + n + k)
    wd = Q.dequantize_mx4(c, s, torch.float64)
    assert E.assert_exact_bound(x, wd, 0.125) < E.EXACT_LIMIT
    assert k * 7 * 24 / 0.125 < E.EXACT_LIMIT or k > 2048     # the worst case, not just the draw
    assert torch.equal(exact, x.double() @ wd.t())


def test_gemm_wrappers_reject_bad_arguments():
    x = torch.zeros(8, 512, dtype=torch.bfloat16)
    Wt = Q.pack_mx4(*Q.quantize_mx4(_rand(528, 512)))
    ws = torch.zeros(4 * 65 * 528)
    for kw in (dict(splits=3, ws=ws), dict(splits=4, ws=ws), dict(nt=3), dict(splits=2),
               dict(silu=True), dict(silu=True, nt=4), dict(ws=ws[:100])):
        with pytest.raises(ValueError):
            Q.mx4_gemm(x, Wt, **kw)
    with pytest.raises(ValueError):
        Q.mx4_gemm(torch.zeros(65, 512, dtype=torch.bfloat16), Wt)
    for kw in (dict(splits=8, ws=ws, epi="slab"), dict(splits=2), dict(epi="slab"), dict(epi="silu"),
               dict(cfg=1), dict(ws=ws[:100], epi="slab")):
        with pytest.raises(ValueError):
            Q.mx4_packed_gemm(x, Wt, **kw)


# --------------------------------------------------------------------- plans
def _proj_shapes(name):
    c = MODELS[name]
    H, I = c.hidden_size, c.intermediate_size
    return {"qkv": ((c.num_heads + 2 * c.num_kv_heads) * c.head_dim, H), "o": (H, c.num_heads * c.head_dim),
            "gu": (2 * I, H), "down": (H, I)}


@pytest.mark.parametrize("name", ["tiny", "llama3-8b", "llama3-70b"])
def test_plans_fit_the_kernels(name):
    for proj, (n, k) in _proj_shapes(name).items():
        assert n % 16 == 0 and k % 256 == 0
        for rows in (1, 8, 9, 16, 32, 50, 64):
            nt, sp = llama.mx4_cfg(proj, rows, n, k)
            assert nt in Q.MX4_NTS and sp >= 1 and k % (256 * sp) == 0
            assert proj != "gu" or (nt, sp) == (2, 1)       # the SiLU epilogue
        for rows in (65, 145, 300, 512, 1024, 4096):
            cfg, sp = llama.mx4pg_cfg(proj, rows, n, k)
            assert cfg == 0 and sp >= 1 and k % (128 * sp) == 0
            assert llama.mx4pg_cfg(proj, rows, n, k, ws_elems=rows * n)[1] == 1
    for per in llama.MX4_PLAN.values():
        assert sorted(per) == [1, 8, 16, 32, 64]
    for plan in llama.MX4PG_PLAN.values():
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


@pytest.mark.parametrize("typed", [False, True])
def test_mx4_checkpoint_round_trip_both_dtype_spellings(tmp_path, typed):
    cfg, layers, embed, norm = _tiny_full()
    for i, n in enumerate(("q", "k", "v")):          # q / k / v blocks carry different scales
        layers[0][n] = layers[0][n] * 4.0 ** i
    W.save_mx4_checkpoint(cfg, layers, embed, norm, None, str(tmp_path), typed=typed, input_scale=True)
    idx = W.SafetensorsIndex(str(tmp_path))
    assert W.is_mx4_checkpoint(idx) and not W.is_awq_checkpoint(idx) and not W.is_fp8_checkpoint(idx)
    raw = idx.get("model.layers.0.self_attn.q_proj.weight")
    assert raw.dtype == (torch.float4_e2m1fn_x2 if typed else torch.uint8)
    assert idx.get("model.layers.0.self_attn.q_proj.weight_scale").dtype == \
        (torch.float8_e8m0fnu if typed else torch.uint8)
    for li, L in enumerate(layers):
        sh = W.load_mx4_layer(cfg, idx, li)
        for attr, names in (("wqkv", "qkv"), ("wo", "o"), ("wgu", ("gate", "up")), ("wd", ("down",))):
            qs = [Q.quantize_mx4(L[n]) for n in names]
            c, s = sh[attr]
            assert c.dtype == torch.uint8 and s.dtype == torch.uint8
            assert s.shape == (c.shape[0], c.shape[1] // 32)
            assert torch.equal(c, torch.cat([a for a, _ in qs]))
            assert torch.equal(s, torch.cat([b for _, b in qs]))
        assert torch.equal(sh["ln1"], L["ln1"])
    s = W.load_mx4_layer(cfg, idx, 0)["wqkv"][1].double()
    assert s[:512].mean() + 1.5 < s[512:640].mean() < s[640:].mean() - 1.5     # scales followed their rows


def test_other_checkpoints_are_not_detected_as_mx4(tmp_path):
    cfg, layers, embed, norm = _tiny_full(1)
    a, b = tmp_path / "fp8", tmp_path / "bf16"
    W.save_fp8_checkpoint(cfg, layers, embed, norm, None, str(a))
    W.save_hf_checkpoint(cfg, layers, embed, norm, None, str(b))
    assert not W.is_mx4_checkpoint(W.SafetensorsIndex(str(a)))
    assert not W.is_mx4_checkpoint(W.SafetensorsIndex(str(b)))


def _rewrite(tmp_path, name, fn):
    from safetensors.torch import load_file, save_file

    path = str(tmp_path / "model.safetensors")
    t = load_file(path)
    t[name] = fn(t[name])
    save_file(t, path)


def test_mx4_loader_refuses_bad_scale_bytes_and_shapes(tmp_path):
    cfg, layers, embed, norm = _tiny_full(2)
    W.save_mx4_checkpoint(cfg, layers, embed, norm, None, str(tmp_path))
    name = "model.layers.1.mlp.down_proj.weight_scale"
    for bad in (0, 1, 253, 255):
        def poke(t, bad=bad):
            t = t.clone()
            t[3, 1] = bad
            return t
        _rewrite(tmp_path, name, poke)
        with pytest.raises(ValueError, match=r"layers\.1\.mlp\.down_proj\.weight_scale"):
            W.load_mx4_layer(cfg, W.SafetensorsIndex(str(tmp_path)), 1)
    _rewrite(tmp_path, name, lambda t: torch.full_like(t, 120))
    W.load_mx4_layer(cfg, W.SafetensorsIndex(str(tmp_path)), 1)
    _rewrite(tmp_path, name, lambda t: t[:, :-1].contiguous())
    with pytest.raises(ValueError, match="weight_scale"):
        W.load_mx4_layer(cfg, W.SafetensorsIndex(str(tmp_path)), 1)
    _rewrite(tmp_path, name, lambda t: torch.full((t.shape[0], t.shape[1] + 1), 120, dtype=torch.uint8))
    _rewrite(tmp_path, "model.layers.1.self_attn.o_proj.weight", lambda t: t.float())
    with pytest.raises(ValueError, match=r"o_proj\.weight"):
        W.load_mx4_layer(cfg, W.SafetensorsIndex(str(tmp_path)), 1)


def test_model_loads_mx4_checkpoint_and_selects_mxfp4(tmp_path):
    cfg, layers, embed, norm = _tiny_full(3)
    W.save_mx4_checkpoint(cfg, layers, embed, norm, None, str(tmp_path))
    m = llama.LlamaModel(cfg, torch.device("cpu"), torch.float32, max_model_len=64)
    assert m.quant is None
    m.load_checkpoint(str(tmp_path))
    assert m.quant == "mxfp4" and m.layers[0].q4x is None        # CPU: dequantized weights
    c, s = Q.quantize_mx4(torch.cat([layers[0][n] for n in "qkv"]))
    assert torch.equal(m.layers[0].wqkv, Q.dequantize_mx4(c, s))
    # the same weights as quantizing the bf16 checkpoint at load time
    r = llama.LlamaModel(cfg, torch.device("cpu"), torch.float32, max_model_len=64, quantization="mxfp4")
    r._set_layers([W.shard_full_layer(cfg, L, 0, 1) for L in layers])
    r._quantize_layers()
    for a, b in zip(m.layers, r.layers):
        for attr in ("wqkv", "wo", "wgu", "wd"):
            assert torch.equal(getattr(a, attr), getattr(b, attr))
    for other in ("w4", "fp8"):   # an MXFP4 checkpoint under another quantization
        with pytest.raises(ValueError, match="MXFP4 checkpoint"):
            llama.LlamaModel(cfg, torch.device("cpu"), torch.float32, max_model_len=64,
                             quantization=other).load_checkpoint(str(tmp_path))


def test_unknown_quantization_still_raises():
    for name in ("fp4", "int8", "mxfp6", "nvfp4"):
        with pytest.raises(ValueError, match="unsupported quantization"):
            llama.LlamaModel(MODELS["tiny"], torch.device("cpu"), torch.float32, quantization=name)
    llama.LlamaModel(MODELS["tiny"], torch.device("cpu"), torch.float32, quantization="MXFP4")


# --------------------------------------------------------------------- engine
def _engine(**kw):
    base = dict(model="tiny", device="cpu", num_kv_blocks=256, max_model_len=1024, max_num_seqs=4)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def test_cpu_engine_mxfp4_generates_deterministically_and_reports_it():
    prompts = [list(range(100, 170)), list(range(300, 305))]
    greedy = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)
    seeded = SamplingParams(temperature=0.8, top_p=0.9, seed=11, max_tokens=6, ignore_eos=True)
    a, b, plain = _engine(quantization="mxfp4"), _engine(quantization="MXFP4"), _engine()
    out = a.generate(prompts, greedy)
    assert all(len(o) == 6 for o in out) and out == b.generate(prompts, greedy)
    assert a.generate(prompts, seeded) == b.generate(prompts, seeded)
    assert all(len(o) == 6 for o in plain.generate(prompts, greedy))
    ma, mp = a.metrics(), plain.metrics()
    assert ma["quantization"] == "mxfp4" and "quantization" not in mp
    assert set(ma) - set(mp) == {"quantization"}
    assert ma["weights_resident_gb"] > 0
    m = a.runner.model
    assert m.quant == "mxfp4" and all(L.q4x is None for L in m.layers)
    # the CPU backend holds dequantize_mx4 of the quantized bf16 weights
    p = plain.runner.model
    for attr in ("wqkv", "wo", "wgu", "wd"):
        c, s = Q.quantize_mx4(getattr(p.layers[1], attr).to(torch.bfloat16))
        assert torch.equal(getattr(m.layers[1], attr), Q.dequantize_mx4(c, s).to(m.dtype))
    assert p.quant is None and all(L.q4x is None for L in p.layers)


def test_mxfp4_refuses_tensor_parallel_and_batch_invariant(monkeypatch):
    with pytest.raises(ValueError, match="tensor parallel"):
        EngineConfig(model="tiny", device="cpu", quantization="mxfp4", tp_size=2)
    with pytest.raises(ValueError, match="batch-invariant"):
        EngineConfig(model="tiny", device="cpu", quantization="mxfp4", batch_invariant=True)
    monkeypatch.setenv("ENGINE_QUANTIZATION", "mxfp4")
    assert EngineConfig.from_env(model="tiny").quantization == "mxfp4"
    monkeypatch.setenv("ENGINE_BATCH_INVARIANT", "1")
    with pytest.raises(ValueError, match="batch-invariant"):
        EngineConfig.from_env(model="tiny")
    monkeypatch.delenv("ENGINE_BATCH_INVARIANT")
    monkeypatch.delenv("ENGINE_QUANTIZATION")
    monkeypatch.setenv("VLLM_QUANTIZATION", "mxfp4")
    assert EngineConfig.from_env(model="tiny").quantization == "mxfp4"
    with pytest.raises(ValueError, match="tensor parallel"):
        EngineConfig.from_env(model="tiny", tp_size=2)
    m = llama.LlamaModel(MODELS["tiny"], torch.device("cpu"), torch.float32, quantization="mxfp4")
    m.init_random(1, consistent=True)
    with pytest.raises(ValueError):
        m.set_batch_invariant(64)
