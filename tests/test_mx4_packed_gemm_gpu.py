"""MXFP4 GEMM above the decode row counts (csrc/kernels/mx4_packed_gemm.hip,
ops.quant.mx4_packed_gemm) on integer operands (ops/exact.mx4_int_operands): slabs in any
order equal the fp64 product bit for bit, the bf16 output is its one rounding, the SiLU
epilogue lands within one bf16 ULP of fp64.

Shapes: 65 / 129 / 300 rows (one row past a 64-row wave tile, one past the 128-row
workgroup tile, a third partial tile), 17 / 33 column tiles (a tail inside the first and
inside the third 256-column tile), K = 128 (one stage, shorter than the ring), 512 under
four splits (one stage per split) and 1024 under two (more stages than ring slots)."""
import functools

import pytest
import torch

from fasttalk_llm_microservice_amd import ops
from fasttalk_llm_microservice_amd.ops import exact as E
from fasttalk_llm_microservice_amd.ops import quant as Q

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _native_loaded():
    ops.native()  # fail loudly if the extension is missing


def _poisoned(codes, sb, gate_up=False):
    """The image followed by 4 KiB of 0xFF and the scale bytes by 1 KiB of 255 (NaN in
    e8m0): an over-read that is used poisons an output."""
    w = Q.pack_mx4(codes, sb, gate_up=gate_up)
    img = torch.full((w.wq.numel() + 4096,), 0xFF, dtype=torch.uint8, device=DEV)
    img[:w.wq.numel()] = w.wq.to(DEV)
    sc = torch.full((w.sc.numel() + 1024,), 255, dtype=torch.uint8, device=DEV)
    sc[:w.sc.numel()] = w.sc.to(DEV)
    return Q.MX4Weight(img[:w.wq.numel()], sc[:w.sc.numel()], w.n, w.k)


@functools.lru_cache(maxsize=None)
def _ops(m, n, k):
    x, c, s, exact = E.mx4_int_operands(m, n, k, seed=m + n + k)
    return x.to(DEV), _poisoned(c, s), exact


def _sum_slabs(ws, sp, m, n, reverse):
    slabs = ws[:sp * m * n].view(sp, m, n).cpu()
    acc = torch.zeros(m, n)
    for i in (reversed(range(sp)) if reverse else range(sp)):
        acc = acc + slabs[i]
    return acc


@pytest.mark.parametrize("k,sp", [(128, 1), (512, 4), (1024, 2)])
@pytest.mark.parametrize("n", [272, 528])
@pytest.mark.parametrize("m", [65, 129, 300])
def test_store_and_slabs_equal_fp64(m, n, k, sp):
    x, W, exact = _ops(m, n, k)
    gx = E.guarded_from(x)
    gws = E.guarded_flat(sp * m * n, device=DEV)
    r = Q.mx4_packed_gemm(gx.view, W, ws=gws.buf, splits=sp, epi="slab")
    assert r is gws.buf
    torch.cuda.synchronize()
    gws.check("slab workspace")
    for rev in (False, True):
        got = _sum_slabs(gws.buf, sp, m, n, rev).double()
        assert torch.equal(got, exact), f"slabs (reverse={rev}) differ from the exact product"
    gout = E.guarded(m, n, device=DEV)
    Q.mx4_packed_gemm(gx.view, W, out=gout.view)
    torch.cuda.synchronize()
    gout.check("bf16 out")
    assert torch.equal(gout.view.cpu(), exact.to(torch.bfloat16))


@pytest.mark.parametrize("m,inter,k", [(65, 272, 128), (300, 272, 512)])
def test_silu_epilogue_within_one_ulp(m, inter, k):
    x, c, s, y = E.mx4_int_operands(m, 2 * inter, k, s_exps=(-9, -7, -5), seed=m)
    ref = E.silu_ref(y[:, :inter], y[:, inter:])
    gout = E.guarded(m, inter, device=DEV)
    Q.mx4_packed_gemm(x.to(DEV), _poisoned(c, s, gate_up=True), out=gout.view, epi="silu")
    torch.cuda.synchronize()
    gout.check("silu out")
    E.assert_ulp1(gout.view.cpu(), ref, "mx4 packed silu")


def test_row_64_slabs_equal_the_decode_kernels():
    """Both kernels sum the same exact bf16 products: at 64 rows their slabs are bit-equal."""
    m, n, k, sp = 64, 528, 1024, 2
    x, W, exact = _ops(m, n, k)
    a = torch.full((sp * m * n,), float("nan"), device=DEV)
    b = torch.full((sp * m * n,), float("nan"), device=DEV)
    Q.mx4_gemm(x, W, ws=a, splits=sp, nt=2)
    Q.mx4_packed_gemm(x, W, ws=b, splits=sp, epi="slab")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(a.view(sp, m, n).sum(0).double().cpu(), exact)


def test_rejected_arguments_return_codes_and_launch_nothing():
    C = ops.native()
    m, n, k = 65, 528, 512
    x, W, _ = _ops(m, n, k)
    canary_ws = torch.full((4 * m * n,), 3.0, device=DEV)
    canary_out = torch.full((m, n), 5.0, dtype=torch.bfloat16, device=DEV)
    odd = Q.MX4Weight(W.wq[:24 * k // 2], W.sc[:24 * k // 32], 24, k)
    rc = lambda w_, out, ws, sp, epi, cfg: C.mx4_packed_gemm_rc(x, w_.wq, w_.sc, w_.n, out, ws, sp, epi, cfg)
    assert rc(odd, canary_out, None, 1, 0, 0) == -2              # N % 16
    assert rc(W, canary_out, None, 1, 2, 0) == -2                # SiLU: N % 32 (528 = 16 * 33)
    assert rc(W, None, canary_ws, 3, 1, 0) == -3                 # K % (128 * 3)
    assert rc(W, None, canary_ws, 8, 1, 0) == -3                 # K / 8 = 64 < one k-step
    assert rc(W, None, canary_ws, 0, 1, 0) == -3                 # splits < 1
    assert rc(W, canary_out, None, 1, 3, 0) == -4                # epilogue code
    assert rc(W, canary_out, None, 1, 1, 0) == -4                # slabs without a workspace
    assert rc(W, canary_out, None, 2, 0, 0) == -4                # bf16 out under split-K
    assert rc(W, None, None, 1, 0, 0) == -4                      # nowhere to write
    assert rc(W, canary_out, None, 1, 0, 1) == -5                # tile cfg
    assert rc(W, None, canary_ws[:2 * m * n - 1], 2, 1, 0) == -8  # workspace too small
    for bad in (dict(splits=3, ws=canary_ws, epi="slab"), dict(splits=2), dict(epi="slab"),
                dict(epi="silu"), dict(cfg=1), dict(ws=canary_ws[:m * n - 1], epi="slab")):
        with pytest.raises((RuntimeError, ValueError)):
            Q.mx4_packed_gemm(x, W, **bad)
    torch.cuda.synchronize()
    assert torch.all(canary_ws == 3.0) and torch.all(canary_out == 5.0)   # nothing was launched
