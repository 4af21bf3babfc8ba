"""W4A16 GEMM above the decode row counts (csrc/kernels/w4_packed_gemm.hip,
ops.quant.w4_packed_gemm) against x.float() @ dequantize_w4(q, z, s).t() on the CPU:
every tile shape (cfg) at the smallest sizes that reach each edge -- row clamp, one /
two / partial row tiles, a column tail past a 256-column tile, an odd column-tile
count, 2 to 8 quantization groups -- for the three epilogues, split-K slabs, TP shard
shapes, strided operands, rejected arguments, graph replay and run-to-run equality.

Tolerances: bf16 output atol 3e-2 / rtol 2e-2 (the packed_gemm tests'); fp32 slabs
1e-3 * max|ref| + 1e-3 (the W4 decode kernels'), which only exact (q - z) * s weights
meet -- bf16-rounded dequantized weights miss it by 1.4-2x."""
import functools

import pytest
import torch

from fasttalk_llm_microservice_amd import ops
from fasttalk_llm_microservice_amd.ops import quant as Q

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFGS = (0, 1, 2)


def _close(a, b, atol, rtol=0.0, msg=""):
    a = a.float().cpu()
    b = b.float().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol).sum().item()
    assert bad == 0, f"{msg}: {bad} elems out of tol, max err {err.max().item():.4g}"


def _slab_close(y, ref, msg=""):
    err = (y.float().cpu() - ref).abs().max().item()
    tol = 1e-3 * ref.abs().max().item() + 1e-3
    print(f"{msg}: slab max err {err:.3e} (tol {tol:.3e})")
    assert err < tol, f"{msg}: slab max err {err:.4g} >= {tol:.4g}"


@pytest.fixture(autouse=True)
def _native_loaded():
    ops.native()  # fail loudly if the extension is missing


@functools.lru_cache(maxsize=None)
def _w4(n, k, seed=0):
    """(packed image on the GPU, dequantized fp32 weight on the CPU); read-only."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k, generator=g) * 0.05
    q, z, s = Q.quantize_w4(w)
    return Q.pack_w4(q.to(DEV), z.to(DEV), s.to(DEV)), Q.dequantize_w4(q, z, s)


@functools.lru_cache(maxsize=None)
def _x(m, k, seed=7):
    return torch.randn(m, k, generator=torch.Generator().manual_seed(seed)).bfloat16()


@functools.lru_cache(maxsize=None)
def _ref(m, n, k):
    return _x(m, k).float() @ _w4(n, k)[1].t()


def _splits_for(k):
    return [s for s in (1, 2, 4) if k % (128 * s) == 0]


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("n,k", [(272, 256), (528, 512), (1040, 1024)])
@pytest.mark.parametrize("m", [1, 65, 129, 257, 300])
def test_store_and_slabs_match_fp32(m, n, k, cfg):
    W, _ = _w4(n, k)
    ref = _ref(m, n, k)
    xd = _x(m, k).to(DEV)
    y = Q.w4_packed_gemm(xd, W, cfg=cfg)
    assert y.shape == (m, n) and y.dtype == torch.bfloat16
    _close(y, ref, 3e-2, 2e-2, f"store m={m} n={n} k={k} cfg={cfg}")
    for sp in _splits_for(k):
        ws = torch.full((sp * m * n,), float("nan"), device=DEV)
        r = Q.w4_packed_gemm(xd, W, ws=ws, splits=sp, epi="slab", cfg=cfg)
        assert r is ws
        _slab_close(ws.view(sp, m, n).sum(0), ref, f"m={m} n={n} k={k} cfg={cfg} splits={sp}")
        out = torch.empty(m, n, dtype=torch.bfloat16, device=DEV)
        ops.slab_store(ws, sp, m, n, out)
        _close(out, ref, 3e-2, 2e-2, f"slab_store m={m} n={n} k={k} cfg={cfg} splits={sp}")


@pytest.mark.parametrize("cfg", CFGS)
def test_silu_epilogue(cfg):
    """gate_up quantized with its rows interleaved in 16-row groups (inter 272: 17
    gate/up tile pairs, a tail past every tile width): h = silu(gate) * up."""
    inter, k, m = 272, 512, 150
    g = torch.Generator().manual_seed(11)
    w = torch.randn(2 * inter, k, generator=g) * 0.05
    q, z, s = Q.quantize_w4(ops.interleave_gate_up(w, 1))
    W = Q.pack_w4(q.to(DEV), z.to(DEV), s.to(DEV))
    x = _x(m, k, seed=3)
    y = x.float() @ Q.dequantize_w4(q, z, s).t()
    gt, up = y.view(m, -1, 2, 16).unbind(2)
    ref = (torch.nn.functional.silu(gt) * up).reshape(m, inter)
    h = Q.w4_packed_gemm(x.to(DEV), W, epi="silu", cfg=cfg).float().cpu()
    assert h.shape == (m, inter)
    err = (h - ref).abs().max().item()
    tol = 2e-2 * ref.abs().max().item() + 1e-2
    print(f"silu cfg={cfg}: max err {err:.3e} (tol {tol:.3e})")
    assert err < tol


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("n,k,splits", [(1280, 8192, 4), (8192, 3584, 7), (7168, 512, 1)])
def test_tp_shard_shapes(n, k, splits, cfg):
    """Llama-3-70B shards at TP=8 (qkv; down with 28 groups in 7 splits) and a gate_up
    shard width, 65 rows: slabs and the bf16 store."""
    m = 65
    W, _ = _w4(n, k)
    ref = _ref(m, n, k)
    xd = _x(m, k).to(DEV)
    ws = torch.full((splits * m * n,), float("nan"), device=DEV)
    Q.w4_packed_gemm(xd, W, ws=ws, splits=splits, epi="slab", cfg=cfg)
    _slab_close(ws.view(splits, m, n).sum(0), ref, f"n={n} k={k} cfg={cfg} splits={splits}")
    _close(Q.w4_packed_gemm(xd, W, cfg=cfg), ref, 3e-2, 2e-2, f"store n={n} k={k} cfg={cfg}")


@pytest.mark.parametrize("cfg", CFGS)
def test_strided_x_and_out(cfg):
    m, n, k = 129, 528, 512
    W, _ = _w4(n, k)
    ref = _ref(m, n, k)
    big = torch.zeros(m, k + 64, dtype=torch.bfloat16, device=DEV)
    big[:, :k] = _x(m, k).to(DEV)
    big[:, k:] = float("nan")            # never read
    x = big[:, :k]
    assert x.stride(0) == k + 64
    wide = torch.full((m, n + 40), 7.0, dtype=torch.bfloat16, device=DEV)
    out = wide[:, :n]
    r = Q.w4_packed_gemm(x, W, out=out, cfg=cfg)
    assert r is out
    _close(out, ref, 3e-2, 2e-2, f"strided cfg={cfg}")
    assert torch.all(wide[:, n:] == 7.0)  # nothing stored past the output columns


def test_rejected_arguments_raise():
    m = 65
    x512 = _x(m, 512).to(DEV)
    W, _ = _w4(528, 512)
    canary = torch.full((4 * m * 528,), 3.0, device=DEV)
    with pytest.raises((RuntimeError, ValueError)):   # K % (128 * splits) != 0: 512 / 8 = 64
        Q.w4_packed_gemm(x512, W, ws=canary, splits=8, epi="slab")
    with pytest.raises((RuntimeError, ValueError)):   # 3 splits of 512
        Q.w4_packed_gemm(x512, W, ws=canary, splits=3, epi="slab")
    with pytest.raises((RuntimeError, ValueError)):   # SiLU needs N % 32 == 0 (528 = 16 * 33)
        Q.w4_packed_gemm(x512, W, epi="silu")
    with pytest.raises((RuntimeError, ValueError)):   # slabs without a workspace
        Q.w4_packed_gemm(x512, W, splits=2, epi="slab")
    with pytest.raises((RuntimeError, ValueError)):   # splits > 1 with the bf16 store
        Q.w4_packed_gemm(x512, W, splits=2)
    with pytest.raises((RuntimeError, ValueError)):   # unknown tile shape
        Q.w4_packed_gemm(x512, W, cfg=9)
    torch.cuda.synchronize()
    assert torch.all(canary == 3.0)                   # nothing was launched


@pytest.mark.parametrize("cfg", CFGS)
def test_graph_replay_and_repeat_bit_equal(cfg):
    """Two eager calls agree bit for bit (no atomics, no order dependence), and a
    captured call replays to the same bits."""
    m, n, k, sp = 300, 1040, 1024, 2
    W, _ = _w4(n, k)
    xd = _x(m, k).to(DEV)
    a = Q.w4_packed_gemm(xd, W, cfg=cfg)
    b = Q.w4_packed_gemm(xd, W, cfg=cfg)
    assert torch.equal(a, b)
    ws_a = torch.full((sp * m * n,), float("nan"), device=DEV)
    ws_b = torch.full((sp * m * n,), float("nan"), device=DEV)
    Q.w4_packed_gemm(xd, W, ws=ws_a, splits=sp, epi="slab", cfg=cfg)
    Q.w4_packed_gemm(xd, W, ws=ws_b, splits=sp, epi="slab", cfg=cfg)
    assert torch.equal(ws_a, ws_b)
    out = torch.zeros(m, n, dtype=torch.bfloat16, device=DEV)
    ws_g = torch.zeros(sp * m * n, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        Q.w4_packed_gemm(xd, W, out=out, cfg=cfg)   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        Q.w4_packed_gemm(xd, W, out=out, cfg=cfg)
        Q.w4_packed_gemm(xd, W, ws=ws_g, splits=sp, epi="slab", cfg=cfg)
    out.zero_()
    ws_g.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, a)
    assert torch.equal(ws_g, ws_a)
