"""W8A16 GEMM above the decode row counts (csrc/kernels/w8_packed_gemm.hip,
ops.quant.w8_packed_gemm) against the fp64 reference x.double() @ (q.double() *
s.double()[:, None]).t() on the CPU: the plan of tests/test_w4_packed_gemm_gpu.py --
row clamp, one / two / partial row tiles, a column tail past a 256-column tile, an odd
column-tile count, 4 to 16 k-steps -- for the three epilogues, split-K slabs,
slab_store, exact integer operands, guarded buffers, strided operands, rejected
arguments, graph replay and run-to-run equality, and bit equality with the decode
kernel on shared rows.

Tolerances: bf16 output atol 3e-2 / rtol 2e-2; fp32 slabs 1e-3 * max|ref| + 1e-3, which
only exact q * s weights meet."""
import functools

import pytest
import torch

from fasttalk_llm_microservice_amd import ops
from fasttalk_llm_microservice_amd.ops import exact as E
from fasttalk_llm_microservice_amd.ops import quant as Q

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFGS = (0,)


def _close(a, b, atol, rtol=0.0, msg=""):
    a = a.double().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol).sum().item()
    assert bad == 0, f"{msg}: {bad} elems out of tol, max err {err.max().item():.4g}"


def _slab_close(y, ref, msg=""):
    err = (y.double().cpu() - ref).abs().max().item()
    tol = 1e-3 * ref.abs().max().item() + 1e-3
    print(f"{msg}: slab max err {err:.3e} (tol {tol:.3e})")
    assert err < tol, f"{msg}: slab max err {err:.4g} >= {tol:.4g}"


@pytest.fixture(autouse=True)
def _native_loaded():
    ops.native()  # fail loudly if the extension is missing


def _poisoned(q, s, gate_up=False):
    """pack_w8 with the image followed by 4 KiB of 0x7F (e4m3 NaN) and the scale vector
    by NaN: an over-read that is used poisons an output."""
    w = Q.pack_w8(q, s, gate_up=gate_up)
    img = torch.full((w.wq.numel() + 4096,), 0x7F, dtype=torch.uint8, device=DEV)
    img[:w.wq.numel()] = w.wq.to(DEV)
    sc = torch.full((w.n + 1024,), float("nan"), device=DEV)
    sc[:w.n] = w.scale.to(DEV)
    return Q.W8Weight(img[:w.wq.numel()], sc[:w.n], w.n, w.k)


@functools.lru_cache(maxsize=None)
def _w8(n, k, seed=0):
    """(poisoned image on the GPU, fp64 q * s on the CPU); read-only."""
    g = torch.Generator().manual_seed(seed)
    q, s = Q.quantize_w8(torch.randn(n, k, generator=g) * 0.05)
    return _poisoned(q, s), Q.dequantize_w8(q, s, torch.float64)


@functools.lru_cache(maxsize=None)
def _x(m, k, seed=7):
    return torch.randn(m, k, generator=torch.Generator().manual_seed(seed)).bfloat16()


@functools.lru_cache(maxsize=None)
def _ref(m, n, k):
    return _x(m, k).double() @ _w8(n, k)[1].t()


def _splits_for(k):
    return [s for s in (1, 2, 4) if k % (64 * s) == 0]


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("n,k", [(272, 256), (528, 512), (1040, 1024)])
@pytest.mark.parametrize("m", [1, 65, 129, 257, 300])
def test_store_and_slabs_match_fp64(m, n, k, cfg):
    W, _ = _w8(n, k)
    ref = _ref(m, n, k)
    xd = _x(m, k).to(DEV)
    y = Q.w8_packed_gemm(xd, W, cfg=cfg)
    assert y.shape == (m, n) and y.dtype == torch.bfloat16
    _close(y, ref, 3e-2, 2e-2, f"store m={m} n={n} k={k} cfg={cfg}")
    for sp in _splits_for(k):
        ws = torch.full((sp * m * n,), float("nan"), device=DEV)
        r = Q.w8_packed_gemm(xd, W, ws=ws, splits=sp, epi="slab", cfg=cfg)
        assert r is ws
        _slab_close(ws.view(sp, m, n).sum(0), ref, f"m={m} n={n} k={k} cfg={cfg} splits={sp}")
        out = torch.empty(m, n, dtype=torch.bfloat16, device=DEV)
        ops.slab_store(ws, sp, m, n, out)
        _close(out, ref, 3e-2, 2e-2, f"slab_store m={m} n={n} k={k} cfg={cfg} splits={sp}")


@pytest.mark.parametrize("cfg", CFGS)
def test_silu_epilogue(cfg):
    """gate_up image interleaved in 16-row groups (inter 272: 17 gate/up tile pairs, a
    tail past the tile width): h = silu(gate) * up."""
    inter, k, m = 272, 512, 150
    g = torch.Generator().manual_seed(11)
    q, s = Q.quantize_w8(torch.randn(2 * inter, k, generator=g) * 0.05)
    W = _poisoned(q, s, gate_up=True)
    x = _x(m, k, seed=3)
    y = x.double() @ Q.dequantize_w8(q, s, torch.float64).t()
    gt, up = y[:, :inter], y[:, inter:]
    ref = gt / (1.0 + torch.exp(-gt)) * up
    h = Q.w8_packed_gemm(x.to(DEV), W, epi="silu", cfg=cfg)
    assert h.shape == (m, inter)
    err = (h.double().cpu() - ref).abs().max().item()
    tol = 2e-2 * ref.abs().max().item() + 1e-2
    print(f"silu cfg={cfg}: max err {err:.3e} (tol {tol:.3e})")
    assert err < tol


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("m,n,k,sp", [(65, 272, 256, 4), (129, 528, 1024, 1), (300, 1040, 1024, 2),
                                      (65, 272, 8192, 4)])
def test_exact_integer_operands(m, n, k, sp, cfg):
    """Integer x and q, three power-of-two scales: slabs summed in either order equal the
    fp64 product bit for bit and the bf16 store is its one rounding; NaN around x, a
    pattern around out, NaN behind the slabs."""
    x, q, s, exact = E.w8_int_operands(m, n, k, seed=m + n + k)
    W = _poisoned(q, s)
    gx = E.guarded_from(x.to(DEV))
    gws = E.guarded_flat(sp * m * n, device=DEV)
    Q.w8_packed_gemm(gx.view, W, ws=gws.buf, splits=sp, epi="slab", cfg=cfg)
    torch.cuda.synchronize()
    gws.check("slab workspace")
    slabs = gws.view.view(sp, m, n).cpu()
    for order in (range(sp), reversed(range(sp))):
        acc = torch.zeros(m, n)
        for i in order:
            acc = acc + slabs[i]
        assert torch.equal(acc.double(), exact), "slabs differ from the exact product"
    gout = E.guarded(m, n, device=DEV)
    Q.w8_packed_gemm(gx.view, W, out=gout.view, cfg=cfg)
    torch.cuda.synchronize()
    gout.check("bf16 out")
    assert torch.equal(gout.view.cpu(), exact.to(torch.bfloat16))


def test_onehot_rows_name_a_misread_k():
    m, n, k, sp = 130, 272, 1024, 2
    _, q, s, _ = E.w8_int_operands(1, n, k, seed=3)
    ks = E.onehot_ks(k, 64, k // sp, m)
    x, exact = E.onehot_operands(m, ks, Q.dequantize_w8(q, s, torch.float64))
    ws = torch.full((sp * m * n,), float("nan"), device=DEV)
    Q.w8_packed_gemm(x.to(DEV), _poisoned(q, s), ws=ws, splits=sp, epi="slab")
    y = ws.view(sp, m, n).sum(0).cpu()
    assert torch.equal(y.double(), exact), E.explain_onehot(y, exact, ks)


def test_exact_silu_epilogue_within_one_ulp():
    m, inter, k = 150, 272, 512
    x, q, s, y = E.w8_int_operands(m, 2 * inter, k, s_exp=-9, seed=2)
    ref = E.silu_ref(y[:, :inter], y[:, inter:])
    gout = E.guarded(m, inter, device=DEV)
    Q.w8_packed_gemm(x.to(DEV), _poisoned(q, s, gate_up=True), out=gout.view, epi="silu")
    torch.cuda.synchronize()
    gout.check("silu out")
    E.assert_ulp1(gout.view.cpu(), ref, "w8 packed silu")


@pytest.mark.parametrize("sp", [1, 2])
def test_same_rows_bit_equal_to_decode_kernel(sp):
    """The same 64 x rows through w8_gemm and (plus one more row) w8_packed_gemm on
    integer operands: bit-equal slabs, so rows below and above 64 see the same weights."""
    n, k = 528, 1024
    x, q, s, _ = E.w8_int_operands(65, n, k, seed=8)
    W = _poisoned(q, s)
    xd = x.to(DEV)
    ws_d = torch.full((sp * 64 * n,), float("nan"), device=DEV)
    ws_p = torch.full((sp * 65 * n,), float("nan"), device=DEV)
    Q.w8_gemm(xd[:64], W, ws=ws_d, splits=sp, nt=2)
    Q.w8_packed_gemm(xd, W, ws=ws_p, splits=sp, epi="slab")
    assert torch.equal(ws_d.view(sp, 64, n), ws_p.view(sp, 65, n)[:, :64])


def test_strided_x_and_out():
    m, n, k = 129, 528, 512
    W, _ = _w8(n, k)
    ref = _ref(m, n, k)
    big = torch.zeros(m, k + 64, dtype=torch.bfloat16, device=DEV)
    big[:, :k] = _x(m, k).to(DEV)
    big[:, k:] = float("nan")            # never read
    x = big[:, :k]
    assert x.stride(0) == k + 64
    wide = torch.full((m, n + 40), 7.0, dtype=torch.bfloat16, device=DEV)
    out = wide[:, :n]
    r = Q.w8_packed_gemm(x, W, out=out)
    assert r is out
    _close(out, ref, 3e-2, 2e-2, "strided")
    assert torch.all(wide[:, n:] == 7.0)  # nothing stored past the output columns


def test_rejected_arguments_return_codes_and_launch_nothing():
    C = ops.native()
    m, n, k = 65, 528, 512
    x = _x(m, k).to(DEV)
    W, _ = _w8(n, k)
    canary = torch.full((16 * m * n,), 3.0, device=DEV)
    canary_out = torch.full((m, n), 5.0, dtype=torch.bfloat16, device=DEV)
    odd = Q.W8Weight(W.wq[:24 * k], W.scale[:24], 24, k)
    rc = lambda w_, out, ws, sp, epi, cfg: C.w8_packed_gemm_rc(x, w_.wq, w_.scale, w_.n, out, ws, sp, epi, cfg)
    assert rc(odd, canary_out, None, 1, 0, 0) == -2          # N % 16
    assert rc(W, canary_out, None, 1, 2, 0) == -2            # SiLU needs N % 32 (528 = 16 * 33)
    assert rc(W, None, canary, 16, 1, 0) == -3               # K % (64 * 16): 512 / 16 = 32
    assert rc(W, None, canary, 3, 1, 0) == -3                # 3 splits of 512
    assert rc(W, canary_out, None, 1, 3, 0) == -4            # unknown epilogue
    assert rc(W, canary_out, None, 2, 1, 0) == -4            # slabs without a workspace
    assert rc(W, canary_out, None, 2, 0, 0) == -4            # splits > 1 with the bf16 store
    assert rc(W, canary_out, None, 1, 0, 9) == -5            # unknown tile shape
    assert rc(W, None, canary[:2 * m * n - 1], 2, 1, 0) == -8   # workspace too small
    for bad in (dict(ws=canary, splits=16, epi="slab"), dict(ws=canary, splits=3, epi="slab"),
                dict(epi="silu"), dict(splits=2, epi="slab"), dict(splits=2), dict(cfg=9),
                dict(ws=canary[:m * n - 1], epi="slab")):
        with pytest.raises((RuntimeError, ValueError)):
            Q.w8_packed_gemm(x, W, **bad)
    torch.cuda.synchronize()
    assert torch.all(canary == 3.0) and torch.all(canary_out == 5.0)   # nothing was launched


def test_graph_replay_and_repeat_bit_equal():
    """Two eager calls agree bit for bit (no atomics, no order dependence), and a
    captured call replays to the same bits."""
    m, n, k, sp = 300, 1040, 1024, 2
    W, _ = _w8(n, k)
    xd = _x(m, k).to(DEV)
    a = Q.w8_packed_gemm(xd, W)
    b = Q.w8_packed_gemm(xd, W)
    assert torch.equal(a, b)
    ws_a = torch.full((sp * m * n,), float("nan"), device=DEV)
    ws_b = torch.full((sp * m * n,), float("nan"), device=DEV)
    Q.w8_packed_gemm(xd, W, ws=ws_a, splits=sp, epi="slab")
    Q.w8_packed_gemm(xd, W, ws=ws_b, splits=sp, epi="slab")
    assert torch.equal(ws_a, ws_b)
    out = torch.zeros(m, n, dtype=torch.bfloat16, device=DEV)
    ws_g = torch.zeros(sp * m * n, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        Q.w8_packed_gemm(xd, W, out=out)   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        Q.w8_packed_gemm(xd, W, out=out)
        Q.w8_packed_gemm(xd, W, ws=ws_g, splits=sp, epi="slab")
    out.zero_()
    ws_g.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, a)
    assert torch.equal(ws_g, ws_a)
