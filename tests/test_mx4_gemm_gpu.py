"""MXFP4 decode GEMM (csrc/kernels/mx4a16.hip, ops.quant.mx4_gemm), 1..64 rows.

Every product fp4 * 2^e is exact in bf16 and the kernel accumulates bf16 products in fp32,
so on integer operands (ops/exact.mx4_int_operands) the slabs and their sum in any order
equal the fp64 product bit for bit and the bf16 output is its one rounding: no tolerance.
The weight-recovery test reads every weight back through the kernel with one-hot rows,
which pins the nibble order, byte_sel, the scale operand and the image.

Shapes: 17 / 33 / 65 column tiles (a tail past every workgroup span of 4, 8 and 16 tiles)
at K = 256 / 1024 / 2048 (one 256-wide chunk, 256-wide slices under split-K, 512-wide
chunks), 1..4 row tiles, every nt built."""
import functools

import pytest
import torch

from fasttalk_llm_microservice_amd import ops
from fasttalk_llm_microservice_amd.models import llama as LM
from fasttalk_llm_microservice_amd.ops import exact as E
from fasttalk_llm_microservice_amd.ops import quant as Q

pytestmark = pytest.mark.gpu
DEV = "cuda"
PLAN_NTS = {nt for per in LM.MX4_PLAN.values() for nt, _ in per.values()}
NTS = sorted(PLAN_NTS | set(Q.MX4_NTS))


@pytest.fixture(autouse=True)
def _native_loaded():
    ops.native()  # fail loudly if the extension is missing


def _poisoned(codes, sb, gate_up=False):
    """pack_mx4 with the image followed by 4 KiB of 0xFF (-6, -6) and the scale bytes by
    1 KiB of 255 (NaN in e8m0): an over-read that is used poisons an output."""
    w = Q.pack_mx4(codes, sb, gate_up=gate_up)
    img = torch.full((w.wq.numel() + 4096,), 0xFF, dtype=torch.uint8, device=DEV)
    img[:w.wq.numel()] = w.wq.to(DEV)
    sc = torch.full((w.sc.numel() + 1024,), 255, dtype=torch.uint8, device=DEV)
    sc[:w.sc.numel()] = w.sc.to(DEV)
    return Q.MX4Weight(img[:w.wq.numel()], sc[:w.sc.numel()], w.n, w.k)


@functools.lru_cache(maxsize=None)
def _ops(m, n, k):
    """(x on the GPU, poisoned image, exact fp64 product on the CPU); read-only."""
    x, c, s, exact = E.mx4_int_operands(m, n, k, seed=m + n + k)
    assert sorted(set(c.flatten().tolist())) == list(range(16)) and len(set(s.flatten().tolist())) == 3
    return x.to(DEV), _poisoned(c, s), exact


def _sum_slabs(ws, sp, m, n, reverse):
    slabs = ws[:sp * m * n].view(sp, m, n).cpu()
    acc = torch.zeros(m, n)
    for i in (reversed(range(sp)) if reverse else range(sp)):
        acc = acc + slabs[i]            # fp32 sums in a fixed order
    return acc


def test_plan_nts_are_built():
    assert PLAN_NTS <= set(Q.MX4_NTS) and NTS == [1, 2, 4]


def test_weight_recovery_through_the_kernel():
    """One-hot rows of 1.0 read every weight of a 272 x 256 image back, 64 k per call:
    the outputs equal dequantize_mx4 in every bit (a weight of -0 comes back as +0: the
    fp32 accumulator starts at +0 and +0 + -0 = +0).  Every code, and the scale bytes at
    both ends of the accepted range, are spread over the blocks."""
    n, k = 272, 256
    g = torch.Generator().manual_seed(0)
    codes = torch.randint(0, 16, (n, k), generator=g, dtype=torch.uint8)
    codes.view(-1)[:16] = torch.arange(16, dtype=torch.uint8)
    pool = torch.tensor([2, 64] + list(range(120, 135)) + [200, 252], dtype=torch.uint8)
    sb = pool[torch.arange(n * k // 32) % len(pool)].view(n, k // 32)
    W = _poisoned(codes, sb)
    want = (Q.dequantize_mx4(codes, sb, torch.float32) + 0.0).to(torch.bfloat16)
    assert torch.equal(want.double(), Q.dequantize_mx4(codes, sb, torch.float64))
    for c in range(4):
        ks = list(range(64 * c, 64 * c + 64))
        x, _ = E.onehot_operands(64, ks, want)
        y = Q.mx4_gemm(x.to(DEV), W, nt=2).cpu()
        exp = want[:, 64 * c:64 * c + 64].t().contiguous()
        assert torch.equal(y.view(torch.int16), exp.view(torch.int16)), \
            E.explain_onehot(y, exp.double(), ks)


@pytest.mark.parametrize("nt", NTS)
@pytest.mark.parametrize("n,k,sp", [(272, 256, 1), (528, 1024, 4), (1040, 1024, 2), (272, 2048, 1)])
@pytest.mark.parametrize("m", [1, 17, 50, 64])
def test_store_and_slabs_equal_fp64(m, n, k, sp, nt):
    """Slabs summed in either order equal the fp64 product bit for bit, the bf16 output its
    one rounding.  Buffers are guarded: NaN around x, a pattern around out, NaN behind
    the slabs."""
    x, W, exact = _ops(m, n, k)
    gx = E.guarded_from(x)
    gws = E.guarded_flat(sp * m * n, device=DEV)
    r = Q.mx4_gemm(gx.view, W, ws=gws.buf, splits=sp, nt=nt)
    assert r is gws.buf
    torch.cuda.synchronize()
    gws.check("slab workspace")
    for rev in (False, True):
        got = _sum_slabs(gws.buf, sp, m, n, rev).double()
        assert torch.equal(got, exact), f"slabs (reverse={rev}) differ from the exact product"
    gout = E.guarded(m, n, device=DEV)
    Q.mx4_gemm(gx.view, W, out=gout.view, nt=nt)
    torch.cuda.synchronize()
    gout.check("bf16 out")
    assert torch.equal(gout.view.cpu(), exact.to(torch.bfloat16))


@pytest.mark.parametrize("m,n,k,sp,nt", [(64, 272, 1024, 2, 1), (20, 528, 2048, 1, 2),
                                          (64, 272, 512, 1, 4)])
def test_onehot_rows_name_a_misread_k(m, n, k, sp, nt):
    _, c, s, _ = E.mx4_int_operands(1, n, k, seed=3)
    W = _poisoned(c, s)
    k_slice = k // sp
    ks = E.onehot_ks(k, 512 if k_slice % 512 == 0 else 256, k_slice, m)
    ks = ks[:m - 4] + [v for v in (31, 32, 127, 128) if v not in ks[:m - 4]][:4] if m > 8 else ks
    x, exact = E.onehot_operands(len(ks), ks, Q.dequantize_mx4(c, s, torch.float64))
    if sp == 1:
        y = Q.mx4_gemm(x.to(DEV), W, nt=nt)
    else:
        ws = torch.full((sp * len(ks) * n,), float("nan"), device=DEV)
        Q.mx4_gemm(x.to(DEV), W, ws=ws, splits=sp, nt=nt)
        y = ws.view(sp, len(ks), n).sum(0)
    assert torch.equal(y.double().cpu(), exact), E.explain_onehot(y.cpu(), exact, ks)


@pytest.mark.parametrize("m", [1, 17, 50])
def test_silu_epilogue_within_one_ulp(m):
    """gate_up image interleaved in 16-row groups (inter 272: 17 gate/up tile pairs); gate
    and up sums are exact, __expf and the division are not correctly rounded, so the one
    rounding may land a step off (the bound of tests/test_gemm_exact_gpu.py)."""
    inter, k = 272, 512
    x, c, s, y = E.mx4_int_operands(m, 2 * inter, k, s_exps=(-9, -7, -5), seed=2 + m)
    ref = E.silu_ref(y[:, :inter], y[:, inter:])
    gout = E.guarded(m, inter, device=DEV)
    W = _poisoned(c, s, gate_up=True)
    Q.mx4_gemm(x.to(DEV), W, out=gout.view, nt=2, silu=True)
    torch.cuda.synchronize()
    gout.check("silu out")
    E.assert_ulp1(gout.view.cpu(), ref, "mx4 silu")
    # the split-K route to the same h: slabs of the interleaved image -> slab_silu
    ws = torch.full((2 * m * 2 * inter,), float("nan"), device=DEV)
    Q.mx4_gemm(x.to(DEV), W, ws=ws, splits=2, nt=2)
    h2 = torch.empty(m, inter, dtype=torch.bfloat16, device=DEV)
    ops.slab_silu(ws, 2, m, inter, h2, interleaved=True)
    E.assert_ulp1(h2.cpu(), ref, "mx4 slabs + slab_silu")


def test_strided_x_and_out():
    m, n, k = 17, 528, 1024
    x, W, exact = _ops(m, n, k)
    big = torch.zeros(m, k + 64, dtype=torch.bfloat16, device=DEV)
    big[:, :k] = x
    big[:, k:] = float("nan")            # never read
    wide = torch.full((m, n + 40), 7.0, dtype=torch.bfloat16, device=DEV)
    out = wide[:, :n]
    r = Q.mx4_gemm(big[:, :k], W, out=out, nt=2)
    assert r is out
    assert torch.equal(out.cpu(), exact.to(torch.bfloat16))
    assert torch.all(wide[:, n:] == 7.0)  # nothing stored past the output columns


def test_rejected_arguments_return_codes_and_launch_nothing():
    C = ops.native()
    n, k, m = 528, 1024, 17
    x, W, _ = _ops(m, n, k)
    x65 = torch.zeros(65, k, dtype=torch.bfloat16, device=DEV)
    canary_ws = torch.full((4 * 65 * n,), 3.0, device=DEV)
    canary_out = torch.full((65, n), 5.0, dtype=torch.bfloat16, device=DEV)
    odd = Q.MX4Weight(W.wq[:24 * k // 2], W.sc[:24 * k // 32], 24, k)   # N % 16 != 0
    rc = lambda x_, w_, out, ws, sp, nt, silu: C.mx4_gemm_rc(x_, w_.wq, w_.sc, w_.n, out, ws, sp, nt, silu)
    assert rc(x65, W, canary_out, None, 1, 1, False) == -1      # M > 64
    assert rc(x, W, canary_out, None, 0, 1, False) == -1        # splits < 1
    assert rc(x, odd, canary_out, None, 1, 1, False) == -2      # N % 16
    assert rc(x, W, canary_out, None, 1, 2, True) == -2         # SiLU: N % 32 (528 = 16 * 33)
    assert rc(x, W, None, canary_ws, 3, 1, False) == -3         # K % (256 * 3)
    assert rc(x, W, None, canary_ws, 8, 1, False) == -3         # K / 8 = 128 < one chunk
    assert rc(x, W, canary_out, None, 2, 1, False) == -4        # splits > 1 without a workspace
    assert rc(x, W, canary_out, None, 1, 3, False) == -5        # nt
    assert rc(x, W, None, None, 1, 1, False) == -6              # nowhere to write
    x1, W32, _ = _ops(1, 272 - 16, 256)
    assert rc(x1, W32, canary_out, None, 1, 4, True) == -7      # SiLU is nt 2
    assert rc(x, W, None, canary_ws[:2 * m * n - 1], 2, 1, False) == -8   # workspace too small
    for bad in (dict(splits=3, ws=canary_ws), dict(nt=3), dict(splits=2), dict(silu=True, nt=4),
                dict(ws=canary_ws[:m * n - 1])):
        with pytest.raises((RuntimeError, ValueError)):
            Q.mx4_gemm(x, W, **bad)
    with pytest.raises((RuntimeError, ValueError)):
        Q.mx4_gemm(x65, W)
    torch.cuda.synchronize()
    assert torch.all(canary_ws == 3.0) and torch.all(canary_out == 5.0)   # nothing was launched


def _slab_close(y, ref, msg=""):
    err = (y.double().cpu() - ref).abs().max().item()
    tol = 1e-3 * ref.abs().max().item() + 1e-3      # fp32 accumulation of exact products (the W8 tests' bound)
    print(f"{msg}: slab max err {err:.3e} (tol {tol:.3e})")
    assert err < tol, f"{msg}: slab max err {err:.4g} >= {tol:.4g}"


@pytest.mark.parametrize("proj,n,k,m", [("qkv", 6144, 4096, 50), ("down", 4096, 14336, 50)])
def test_real_shape_with_plan_config(proj, n, k, m):
    """The plan's own (nt, splits) at 50 rows on quantized Gaussian weights, against fp64
    on the dequantized weights."""
    nt, sp = LM.mx4_cfg(proj, m, n, k)
    g = torch.Generator().manual_seed(5)
    c, s = Q.quantize_mx4((torch.randn(n, k, generator=g) * 0.02).bfloat16())
    W = _poisoned(c, s)
    x = torch.randn(m, k, generator=torch.Generator().manual_seed(9)).bfloat16()
    ref = x.double() @ Q.dequantize_mx4(c, s, torch.float64).t()
    ws = torch.full((sp * m * n,), float("nan"), device=DEV)
    Q.mx4_gemm(x.to(DEV), W, ws=ws, splits=sp, nt=nt)
    _slab_close(ws.view(sp, m, n).sum(0), ref, f"{proj} nt={nt} splits={sp}")


def test_graph_replay_and_repeat_bit_equal():
    m, n, k, sp = 50, 1040, 1024, 2
    xd, W, _ = _ops(m, n, k)
    a = Q.mx4_gemm(xd, W, nt=2)
    b = Q.mx4_gemm(xd, W, nt=2)
    assert torch.equal(a, b)
    ws_a = torch.full((sp * m * n,), float("nan"), device=DEV)
    ws_b = torch.full((sp * m * n,), float("nan"), device=DEV)
    Q.mx4_gemm(xd, W, ws=ws_a, splits=sp, nt=1)
    Q.mx4_gemm(xd, W, ws=ws_b, splits=sp, nt=1)
    assert torch.equal(ws_a, ws_b)
    out = torch.zeros(m, n, dtype=torch.bfloat16, device=DEV)
    ws_g = torch.zeros(sp * m * n, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        Q.mx4_gemm(xd, W, out=out, nt=2)   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        Q.mx4_gemm(xd, W, out=out, nt=2)
        Q.mx4_gemm(xd, W, ws=ws_g, splits=sp, nt=1)
    out.zero_()
    ws_g.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, a)
    assert torch.equal(ws_g, ws_a)
