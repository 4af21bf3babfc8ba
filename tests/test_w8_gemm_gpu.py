"""W8A16 decode GEMM (csrc/kernels/w8a16.hip, ops.quant.w8_gemm), 1..64 rows, against the
fp64 reference x.double() @ (q.double() * s.double()[:, None]).t() on the CPU.

Shapes: 17 / 33 / 65 column tiles (a tail past every workgroup span of 4, 8 and 16
tiles) at K = 256 / 512 / 1024 (one, two and several 256-wide K chunks; K slices that
are a multiple of 512 run the kernel's 512-wide chunk form, and the exact cases add
slices of three and seven 256-wide chunks), every row-tile count, every nt the plan can
select, split-K including a slice of one chunk.

Tolerances: bf16 output atol 3e-2 / rtol 2e-2, fp32 slabs 1e-3 * max|ref| + 1e-3 (the W4
kernel tests' values; only exact q * s weights meet the slab bound).  The exact cases
need no tolerance: integer operands and power-of-two scales (ops/exact.py)."""
import functools

import pytest
import torch

from fasttalk_llm_microservice_amd import ops
from fasttalk_llm_microservice_amd.models import llama as LM
from fasttalk_llm_microservice_amd.ops import exact as E
from fasttalk_llm_microservice_amd.ops import quant as Q

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(272, 256), (528, 512), (1040, 1024)]
ROWS = [1, 15, 16, 17, 33, 64]
PLAN_NTS = {nt for per in LM.W8_PLAN.values() for nt, _ in per.values()}
NTS = sorted(PLAN_NTS | set(Q.W8_NTS))     # every nt the plan can select, and every one built


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
    w = torch.randn(n, k, generator=g) * 0.05
    q, s = Q.quantize_w8(w)
    return _poisoned(q, s), Q.dequantize_w8(q, s, torch.float64)


@functools.lru_cache(maxsize=None)
def _x(m, k, seed=7):
    return torch.randn(m, k, generator=torch.Generator().manual_seed(seed)).bfloat16()


@functools.lru_cache(maxsize=None)
def _ref(m, n, k):
    return _x(m, k).double() @ _w8(n, k)[1].t()


def _splits_for(k):
    return [s for s in (1, 2, 4) if k % (256 * s) == 0]


def test_plan_nts_are_built():
    assert PLAN_NTS <= set(Q.W8_NTS) and NTS == [1, 2, 4]


@pytest.mark.parametrize("nt", NTS)
@pytest.mark.parametrize("n,k", SHAPES)
@pytest.mark.parametrize("m", ROWS)
def test_store_and_slabs_match_fp64(m, n, k, nt):
    W, _ = _w8(n, k)
    ref = _ref(m, n, k)
    xd = _x(m, k).to(DEV)
    y = Q.w8_gemm(xd, W, nt=nt)
    assert y.shape == (m, n) and y.dtype == torch.bfloat16
    _close(y, ref, 3e-2, 2e-2, f"store m={m} n={n} k={k} nt={nt}")
    for sp in _splits_for(k):
        ws = torch.full((sp * m * n,), float("nan"), device=DEV)
        r = Q.w8_gemm(xd, W, ws=ws, splits=sp, nt=nt)
        assert r is ws
        _slab_close(ws.view(sp, m, n).sum(0), ref, f"m={m} n={n} k={k} nt={nt} splits={sp}")


@pytest.mark.parametrize("m", [1, 17, 50])
def test_silu_epilogue(m):
    """gate_up image interleaved in 16-row groups (inter 272: 17 gate/up tile pairs)."""
    inter, k = 272, 512
    g = torch.Generator().manual_seed(11)
    q, s = Q.quantize_w8(torch.randn(2 * inter, k, generator=g) * 0.05)
    W = _poisoned(q, s, gate_up=True)
    x = _x(m, k, seed=3)
    y = x.double() @ Q.dequantize_w8(q, s, torch.float64).t()
    gt, up = y[:, :inter], y[:, inter:]
    ref = gt / (1.0 + torch.exp(-gt)) * up
    h = Q.w8_gemm(x.to(DEV), W, nt=2, silu=True)
    assert h.shape == (m, inter) and h.dtype == torch.bfloat16
    err = (h.double().cpu() - ref).abs().max().item()
    tol = 2e-2 * ref.abs().max().item() + 1e-2       # the W4 SiLU tests' bound
    print(f"silu m={m}: max err {err:.3e} (tol {tol:.3e})")
    assert err < tol
    # the split-K route to the same h: slabs of the interleaved image -> slab_silu
    ws = torch.full((2 * m * 2 * inter,), float("nan"), device=DEV)
    Q.w8_gemm(x.to(DEV), W, ws=ws, splits=2, nt=2)
    h2 = torch.empty(m, inter, dtype=torch.bfloat16, device=DEV)
    ops.slab_silu(ws, 2, m, inter, h2, interleaved=True)
    assert (h2.double().cpu() - ref).abs().max().item() < tol


@pytest.mark.parametrize("proj,n,k,m", [("qkv", 6144, 4096, 50), ("down", 4096, 14336, 50),
                                         ("down", 4096, 14336, 16)])
def test_real_shape_with_plan_config(proj, n, k, m):
    """The plan's own (nt, splits): 50 rows, and down at 16 rows, whose K slice of 1792 runs
    seven 256-wide chunks."""
    nt, sp = LM.w8_cfg(proj, m, n, k)
    g = torch.Generator().manual_seed(5)
    q, s = Q.quantize_w8((torch.randn(n, k, generator=g) * 0.02).bfloat16())
    W = _poisoned(q, s)
    x = _x(m, k, seed=9)
    ref = x.double() @ Q.dequantize_w8(q, s, torch.float64).t()
    ws = torch.full((sp * m * n,), float("nan"), device=DEV)
    Q.w8_gemm(x.to(DEV), W, ws=ws, splits=sp, nt=nt)
    _slab_close(ws.view(sp, m, n).sum(0), ref, f"{proj} nt={nt} splits={sp}")
    out = torch.empty(m, n, dtype=torch.bfloat16, device=DEV)
    ops.slab_store(ws, sp, m, n, out)
    _close(out, ref, 3e-2, 2e-2, f"{proj} slab_store")


# ------------------------------------------------------------------ exact cases
def _sum_slabs(ws, sp, m, n, reverse):
    slabs = ws[:sp * m * n].view(sp, m, n).cpu()
    acc = torch.zeros(m, n)
    for i in (reversed(range(sp)) if reverse else range(sp)):
        acc = acc + slabs[i]            # fp32 sums in a fixed order
    return acc


@pytest.mark.parametrize("nt", NTS)
@pytest.mark.parametrize("m,n,k,sp", [(1, 272, 256, 1), (17, 528, 1024, 4), (64, 1040, 1024, 2),
                                      (33, 272, 8192, 4), (64, 272, 8192, 1), (40, 272, 768, 1),
                                      (16, 528, 3584, 2)])
def test_exact_integer_operands(m, n, k, sp, nt):
    """Integer x (|x| <= 7) and q (|q| <= 15), three power-of-two scales: slabs summed in
    either order equal the fp64 product bit for bit, the bf16 output its one rounding.
    Buffers are guarded: NaN around x, a pattern around out, NaN behind the slabs."""
    x, q, s, exact = E.w8_int_operands(m, n, k, seed=m + n + k)
    assert len(set(s.tolist())) == 3
    W = _poisoned(q, s)
    gx = E.guarded_from(x.to(DEV))
    gws = E.guarded_flat(sp * m * n, device=DEV)
    Q.w8_gemm(gx.view, W, ws=gws.buf, splits=sp, nt=nt)
    torch.cuda.synchronize()
    gws.check("slab workspace")
    for rev in (False, True):
        got = _sum_slabs(gws.buf, sp, m, n, rev).double()
        assert torch.equal(got, exact), f"slabs (reverse={rev}) differ from the exact product"
    gout = E.guarded(m, n, device=DEV)
    Q.w8_gemm(gx.view, W, out=gout.view, nt=nt)
    torch.cuda.synchronize()
    gout.check("bf16 out")
    assert torch.equal(gout.view.cpu(), exact.to(torch.bfloat16))


@pytest.mark.parametrize("m,n,k,sp,nt", [(64, 272, 1024, 2, 1), (20, 528, 2048, 1, 2),
                                          (64, 272, 512, 1, 4)])
def test_onehot_rows_name_a_misread_k(m, n, k, sp, nt):
    _, q, s, _ = E.w8_int_operands(1, n, k, seed=3)
    W = _poisoned(q, s)
    k_slice = k // sp
    ks = E.onehot_ks(k, 512 if k_slice % 512 == 0 else 256, k_slice, m)
    x, exact = E.onehot_operands(m, ks, Q.dequantize_w8(q, s, torch.float64))
    y = Q.w8_gemm(x.to(DEV), W, nt=nt) if sp == 1 else None
    if sp > 1:
        ws = torch.full((sp * m * n,), float("nan"), device=DEV)
        Q.w8_gemm(x.to(DEV), W, ws=ws, splits=sp, nt=nt)
        y = ws.view(sp, m, n).sum(0)
    assert torch.equal(y.double().cpu(), exact), E.explain_onehot(y.cpu(), exact, ks)


def test_exact_silu_epilogue_within_one_ulp():
    m, inter, k = 50, 272, 512
    x, q, s, y = E.w8_int_operands(m, 2 * inter, k, s_exp=-9, seed=2)
    ref = E.silu_ref(y[:, :inter], y[:, inter:])
    gout = E.guarded(m, inter, device=DEV)
    Q.w8_gemm(x.to(DEV), _poisoned(q, s, gate_up=True), out=gout.view, nt=2, silu=True)
    torch.cuda.synchronize()
    gout.check("silu out")
    # gate and up sums are exact; __expf and the division are not correctly rounded, so
    # the one rounding may land a step off (the bound of tests/test_gemm_exact_gpu.py)
    E.assert_ulp1(gout.view.cpu(), ref, "w8 silu")


# ------------------------------------------------------------------ operands, arguments
def test_strided_x_and_out():
    m, n, k = 33, 528, 512
    W, _ = _w8(n, k)
    ref = _ref(m, n, k)
    big = torch.zeros(m, k + 64, dtype=torch.bfloat16, device=DEV)
    big[:, :k] = _x(m, k).to(DEV)
    big[:, k:] = float("nan")            # never read
    x = big[:, :k]
    wide = torch.full((m, n + 40), 7.0, dtype=torch.bfloat16, device=DEV)
    out = wide[:, :n]
    r = Q.w8_gemm(x, W, out=out, nt=2)
    assert r is out
    _close(out, ref, 3e-2, 2e-2, "strided")
    assert torch.all(wide[:, n:] == 7.0)  # nothing stored past the output columns


def test_rejected_arguments_return_codes_and_launch_nothing():
    C = ops.native()
    n, k, m = 528, 512, 16
    W, _ = _w8(n, k)
    x = _x(m, k).to(DEV)
    x65 = _x(65, k).to(DEV)
    canary_ws = torch.full((4 * 65 * n,), 3.0, device=DEV)
    canary_out = torch.full((65, n), 5.0, dtype=torch.bfloat16, device=DEV)
    odd = Q.W8Weight(W.wq[:24 * k], W.scale[:24], 24, k)   # N % 16 != 0
    rc = lambda x_, w_, out, ws, sp, nt, silu: C.w8_gemm_rc(x_, w_.wq, w_.scale, w_.n, out, ws, sp, nt, silu)
    assert rc(x65, W, canary_out, None, 1, 1, False) == -1      # M > 64
    assert rc(x, W, canary_out, None, 0, 1, False) == -1        # splits < 1
    assert rc(x, odd, canary_out, None, 1, 1, False) == -2      # N % 16
    assert rc(x, W, canary_out, None, 1, 2, True) == -2         # SiLU: N % 32 (528 = 16 * 33)
    assert rc(x, W, None, canary_ws, 3, 1, False) == -3         # K % (256 * 3)
    assert rc(x, W, None, canary_ws, 4, 1, False) == -3         # K / 4 = 128 < one chunk
    assert rc(x, W, canary_out, None, 2, 1, False) == -4        # splits > 1 without a workspace
    assert rc(x, W, canary_out, None, 1, 3, False) == -5        # nt
    assert rc(x, W, None, None, 1, 1, False) == -6              # nowhere to write
    W32, _ = _w8(1040 - 16, 256)
    x256 = _x(m, 256).to(DEV)
    assert rc(x256, W32, canary_out, None, 1, 4, True) == -7    # SiLU is nt 2
    assert rc(x, W, None, canary_ws[:2 * m * n - 1], 2, 1, False) == -8   # workspace too small
    for bad in (dict(splits=3, ws=canary_ws), dict(nt=3), dict(splits=2), dict(silu=True, nt=4),
                dict(ws=canary_ws[:m * n - 1])):
        with pytest.raises((RuntimeError, ValueError)):
            Q.w8_gemm(x, W, **bad)
    with pytest.raises((RuntimeError, ValueError)):
        Q.w8_gemm(x65, W)
    with pytest.raises(ValueError):
        Q.pack_w8(torch.zeros(24, 256).to(Q.FP8), torch.ones(24))
    with pytest.raises(ValueError):
        Q.pack_w8(torch.zeros(32, 96).to(Q.FP8), torch.ones(32))
    torch.cuda.synchronize()
    assert torch.all(canary_ws == 3.0) and torch.all(canary_out == 5.0)   # nothing was launched


def test_graph_replay_and_repeat_bit_equal():
    m, n, k, sp = 50, 1040, 1024, 2
    W, _ = _w8(n, k)
    xd = _x(m, k).to(DEV)
    a = Q.w8_gemm(xd, W, nt=2)
    b = Q.w8_gemm(xd, W, nt=2)
    assert torch.equal(a, b)
    ws_a = torch.full((sp * m * n,), float("nan"), device=DEV)
    ws_b = torch.full((sp * m * n,), float("nan"), device=DEV)
    Q.w8_gemm(xd, W, ws=ws_a, splits=sp, nt=1)
    Q.w8_gemm(xd, W, ws=ws_b, splits=sp, nt=1)
    assert torch.equal(ws_a, ws_b)
    out = torch.zeros(m, n, dtype=torch.bfloat16, device=DEV)
    ws_g = torch.zeros(sp * m * n, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        Q.w8_gemm(xd, W, out=out, nt=2)   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        Q.w8_gemm(xd, W, out=out, nt=2)
        Q.w8_gemm(xd, W, ws=ws_g, splits=sp, nt=1)
    out.zero_()
    ws_g.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, a)
    assert torch.equal(ws_g, ws_a)
