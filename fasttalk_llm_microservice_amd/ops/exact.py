"""Operands and comparisons for bit-exact GEMM tests and one-step-exact attention tests
(plain PyTorch, no native code).

A GEMM whose operands are small integers times a power of two has an exactly
representable result at every stage: bf16 x bf16 products are exact in fp32 and fp32
sums of integers below 2**24 are exact in ANY order, on any tiling, with any split-K.
For such operands a kernel's output must equal the fp64 product bit for bit, so the
tests built on this module need no tolerance and survive every re-tiling of a kernel.

* :func:`int_operands` / :func:`w4_int_operands` / :func:`w8_int_operands` /
  :func:`mx4_int_operands` / :func:`onehot_operands` / :func:`silu_operands` build the
  operands and ASSERT the exactness bound.
* :func:`bf16_ulp_diff` measures bf16 outputs that cannot be exact (SiLU, norms).
* :func:`guarded` / :func:`guarded_flat` embed a buffer in a larger allocation with a
  fixed bit pattern and check that a launch left everything outside it untouched.
* The attention section at the end (:func:`attn_operands`, :func:`attn_reference`,
  :func:`attn_self_check`, :func:`attn_model`, :func:`assert_attn`, the case tables) makes
  the whole softmax exactly predictable while every key stays visible in a bf16 output.
"""
from __future__ import annotations

import dataclasses
import math
from typing import List, Optional, Tuple

import torch

EXACT_LIMIT = 1 << 24          # fp32 holds every integer of smaller magnitude
NAN_BF16 = 0x7FC1              # quiet NaNs with a payload: a fill no kernel produces
NAN_F32 = 0x7FC00A5A
PAD_BF16 = 0x5AA5              # a large finite bf16 (~2.3e16) for output pads
MAX_GATE = 60.0                # |g| the SiLU references accept (exp stays in fp32 range)


# The parameter sets the GPU tests ship (tests/test_gemm_exact_gpu.py): the largest K
# each is used at.  tests/unit/test_exact_operands_cpu.py shows on the CPU that every
# one of them is order-independent in fp32.
BF16_SETS = {
    # 14336 * 7 * 15 = 1.5 M units; a residual of <= 256 units on top stays far below 2**24
    "gemm": dict(k=14336, x_max=7, w_max=15, w_shift=6),
}
W4_SETS = {
    # sum |x| (128 + q) s in units of 2**-7 (mean |x| 1.2, mean scale 2.3 units): ~1.6 M
    # at K = 4096, ~5.5 M at K = 14336; the assertion measures the drawn operands
    "gemm": dict(k=14336, x_max=2, s_exp=-7, n_scales=3),
}


# ---------------------------------------------------------------------------------
# the exactness bound
# ---------------------------------------------------------------------------------

def exact_product(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """x w^T in fp64 (a BLAS matmul: exact for operands inside the bound)."""
    return x.double() @ w.double().t()


def assert_bf16_exact(t: torch.Tensor, name: str = "operand") -> None:
    d = t.double()
    assert torch.equal(d.to(torch.bfloat16).double(), d), f"{name} does not round-trip through bf16"


def assert_exact_bound(x: torch.Tensor, w: torch.Tensor, unit: float) -> float:
    """Asserts that sum_k |x[m,k]| |w[n,k]| / unit < 2**24 for every (m, n), that x is
    integer-valued and w an integer multiple of ``unit``: then every partial sum of
    x w^T, in any order, is an integer multiple of ``unit`` that fp32 holds exactly.
    Returns the worst case in units."""
    xd, wd = x.double(), w.double() / unit
    assert torch.equal(xd, xd.round()), "x is not integer-valued"
    assert torch.equal(wd, wd.round()), "w is not an integer multiple of the unit"
    worst = float((xd.abs() @ wd.abs().t()).max())
    assert worst < EXACT_LIMIT, (f"exactness bound violated: worst |x| |w|^T = {worst:.0f} units "
                                 f">= 2**24 (K = {x.shape[1]})")
    return worst


def _randint(lo: int, hi: int, shape, g: torch.Generator) -> torch.Tensor:
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int64)


def int_operands(m: int, n: int, k: int, x_max: int = 7, w_max: int = 15, w_shift: int = 6,
                 seed: int = 0, device="cpu"):
    """(x [m, k] bf16, w [n, k] bf16, exact [m, n] fp64): x integers in [-x_max, x_max],
    w integers in [-w_max, w_max] times 2**-w_shift, exact = x w^T.  Seeded random
    integers: rows differ from each other and so do columns, so a swapped row or column
    tile shows.  Asserts the exactness bound and the bf16 round trip."""
    g = torch.Generator().manual_seed(seed)
    unit = 2.0 ** -w_shift
    xd = _randint(-x_max, x_max, (m, k), g).double()
    wd = _randint(-w_max, w_max, (n, k), g).double() * unit
    assert_bf16_exact(xd, "x")
    assert_bf16_exact(wd, "w")
    x, w = xd.to(torch.bfloat16).to(device), wd.to(torch.bfloat16).to(device)
    assert_exact_bound(x, w, unit)
    return x, w, exact_product(x, w)


def int_residual(m: int, n: int, r_max: int = 200, w_shift: int = 6, seed: int = 1, device="cpu"):
    """bf16 [m, n] residual, integer-valued in units of 2**-w_shift (|r| <= r_max <= 256,
    so bf16 holds it and res + x w^T stays inside the bound checked by the caller)."""
    assert r_max <= 256
    g = torch.Generator().manual_seed(seed)
    r = _randint(-r_max, r_max, (m, n), g).double() * 2.0 ** -w_shift
    assert_bf16_exact(r, "residual")
    return r.to(torch.bfloat16).to(device)


# ---------------------------------------------------------------------------------
# W4A16: q, z in 0..15, power-of-two scales
# ---------------------------------------------------------------------------------

W4_GROUP = 128


def w4_dequant_exact(q, z, s) -> torch.Tensor:
    """(q - z) * s in fp64, [N, K]."""
    n, k = q.shape
    w = (q.double().view(n, k // W4_GROUP, W4_GROUP) - z.double().unsqueeze(-1)) * s.double().unsqueeze(-1)
    return w.view(n, k)


def assert_w4_bound(x, q, z, s) -> float:
    """The W4 kernels accumulate x (128 + q) per group, scale it by s and subtract
    s (128 + z) sum(x): asserts sum_k |x| (128 + max(q, z)) s, in units of the smallest
    scale, below 2**24 and the scales powers of two.  Returns the worst case in units."""
    sd = s.double()
    assert torch.equal(torch.log2(sd), torch.log2(sd).round()), "scales must be powers of two"
    n, k = q.shape
    unit = float(sd.min())
    xd = x.double()
    assert torch.equal(xd, xd.round()), "x is not integer-valued"
    qz = torch.maximum(q.double().view(n, k // W4_GROUP, W4_GROUP), z.double().unsqueeze(-1))
    mag = ((128.0 + qz) * (sd / unit).unsqueeze(-1)).view(n, k)
    worst = float((xd.abs() @ mag.t()).max())
    assert worst < EXACT_LIMIT, (f"exactness bound violated: worst sum |x| (128 + q) s = "
                                 f"{worst:.0f} units >= 2**24 (K = {k})")
    return worst


def w4_int_operands(m: int, n: int, k: int, x_max: int = 2, s_exp: int = -7, n_scales: int = 3,
                    seed: int = 0, device="cpu"):
    """(x [m, k] bf16, q uint8 [n, k], z uint8 [n, k/128], s fp32 [n, k/128], exact fp64):
    x integers in [-x_max, x_max]; q, z in 0..15; s per (row, group) one of ``n_scales``
    adjacent powers of two from 2**s_exp; exact = x ((q - z) s)^T.  Asserts the bound of
    :func:`assert_w4_bound`.  Pack with ``quant.pack_w4(q, z, s)``."""
    assert k % W4_GROUP == 0
    g = torch.Generator().manual_seed(seed)
    xd = _randint(-x_max, x_max, (m, k), g).double()
    q = _randint(0, 15, (n, k), g).to(torch.uint8)
    z = _randint(0, 15, (n, k // W4_GROUP), g).to(torch.uint8)
    s = torch.pow(2.0, (s_exp + _randint(0, n_scales - 1, (n, k // W4_GROUP), g)).double()).float()
    assert_bf16_exact(xd, "x")
    x = xd.to(torch.bfloat16).to(device)
    q, z, s = q.to(device), z.to(device), s.to(device)
    assert_w4_bound(x, q, z, s)
    return x, q, z, s, x.double() @ w4_dequant_exact(q, z, s).t()


# ---------------------------------------------------------------------------------
# W8A16: fp8 e4m3 q holding small integers, power-of-two channel scales
# ---------------------------------------------------------------------------------

def w8_int_operands(m: int, n: int, k: int, x_max: int = 7, q_max: int = 15, s_exp: int = -6,
                    n_scales: int = 3, seed: int = 0, device="cpu"):
    """(x [m, k] bf16, q float8_e4m3fn [n, k], s fp32 [n], exact [m, n] fp64): x integers in
    [-x_max, x_max], q integers in [-q_max, q_max] (e4m3 holds every integer up to 16
    exactly; asserted), s per output channel one of ``n_scales`` adjacent powers of two
    from 2**s_exp, all of them used; exact = x (q s)^T.  The W8 kernels accumulate
    sum_k x q (integers below 2**24, asserted) and scale the sum once by a power of two,
    so slabs and their sum in any order are exact.  Pack with ``quant.pack_w8(q, s)``."""
    assert q_max <= 16 and n >= n_scales
    g = torch.Generator().manual_seed(seed)
    xd = _randint(-x_max, x_max, (m, k), g).double()
    qd = _randint(-q_max, q_max, (n, k), g).double()
    e = _randint(0, n_scales - 1, (n,), g)
    e[:n_scales] = torch.arange(n_scales)
    s = torch.pow(2.0, (s_exp + e).double()).float()
    q = qd.to(torch.float8_e4m3fn)
    assert torch.equal(q.double(), qd), "q does not round-trip through e4m3"
    assert_bf16_exact(xd, "x")
    x = xd.to(torch.bfloat16).to(device)
    assert_exact_bound(x, qd.to(device), 1.0)
    q, s = q.to(device), s.to(device)
    return x, q, s, x.double() @ (q.double() * s.double().unsqueeze(-1)).t()


# ---------------------------------------------------------------------------------
# MXFP4: e2m1 codes (multiples of 0.5 up to 6), power-of-two block scales
# ---------------------------------------------------------------------------------

def mx4_int_operands(m: int, n: int, k: int, x_max: int = 7, s_exps=(-2, 0, 2), seed: int = 0,
                     device="cpu"):
    """(x [m, k] bf16, codes uint8 [n, k], sb uint8 [n, k / 32], exact [m, n] fp64): x
    integers in [-x_max, x_max], every e2m1 code 0..15 used, each 32-block scaled by
    2**e with e one of ``s_exps`` (three exponents two octaves apart, all used); exact =
    x dequant^T in fp64.  Every weight is an integer multiple of 0.5 * 2**min(s_exps), and
    the bound sum |x| |w| / unit < 2**24 is asserted on the drawn operands (worst case
    K * x_max * 12 * 2**(max - min): 2.75 M units at K = 2048), so the fp32 sums of the
    MX4 kernels are exact in any order.  Pack with ``quant.pack_mx4(codes, sb)``."""
    from .quant import MX4_BLOCK, dequantize_mx4

    nb = n * (k // MX4_BLOCK)
    assert k % MX4_BLOCK == 0 and nb >= len(s_exps) and n * k >= 16
    g = torch.Generator().manual_seed(seed)
    xd = _randint(-x_max, x_max, (m, k), g).double()
    codes = _randint(0, 15, (n, k), g).to(torch.uint8)
    codes.view(-1)[:16] = torch.arange(16, dtype=torch.uint8)
    pick = _randint(0, len(s_exps) - 1, (nb,), g)
    pick[:len(s_exps)] = torch.arange(len(s_exps))
    sb = (torch.tensor(s_exps, dtype=torch.int64)[pick] + 127).to(torch.uint8).view(n, k // MX4_BLOCK)
    wd = dequantize_mx4(codes, sb, torch.float64)
    assert_bf16_exact(xd, "x")
    assert_bf16_exact(wd, "dequantized weight")
    x = xd.to(torch.bfloat16).to(device)
    assert_exact_bound(x, wd.to(device), 0.5 * 2.0 ** min(s_exps))
    return x, codes.to(device), sb.to(device), x.double() @ wd.to(device).t()


# ---------------------------------------------------------------------------------
# one-hot rows: y[i, :] == w[:, k_i], so a failure names the (row, k, column) mis-read
# ---------------------------------------------------------------------------------

def onehot_ks(k: int, chunk: int, k_slice: int, rows: int) -> List[int]:
    """``rows`` distinct k indices, edges first: first / last element of an 8-vector, of
    a 16-wide MFMA k-step, of a 64-k fragment, of the kernel's K chunk, of a split's K
    slice (at the first, an inner and the last split), and K - 1."""
    want = [0, 7, 8, 15, 16, 63, 64, chunk - 1, chunk, k_slice - 1, k - 1, k - 8, k - 16, k - 64,
            k - chunk, k - k_slice, k_slice, 2 * chunk - 1, 2 * k_slice - 1, k - k_slice - 1]
    ks: List[int] = []
    for v in want:
        if 0 <= v < k and v not in ks:
            ks.append(v)
    step = max(1, k // (rows + 1)) | 1           # fill up with a spread of other columns
    v = 1
    while len(ks) < rows:
        if v % k not in ks:
            ks.append(v % k)
        v += step
    return ks[:rows]


def onehot_operands(m: int, ks: List[int], w: torch.Tensor):
    """(x [m, K] bf16 with x[i, ks[i]] = 1 and zeros elsewhere, exact [m, N] fp64 =
    w[:, ks]^T) for weights ``w`` [N, K] (bf16, or the fp64 dequantized W4 weights)."""
    assert len(ks) >= m
    x = torch.zeros(m, w.shape[1], dtype=torch.bfloat16, device=w.device)
    idx = torch.tensor(ks[:m], device=w.device)
    x[torch.arange(m, device=w.device), idx] = 1.0
    return x, w.double()[:, idx].t().contiguous()


def explain_onehot(got: torch.Tensor, exact: torch.Tensor, ks: List[int]) -> str:
    bad = (got.double() != exact).nonzero()
    if bad.numel() == 0:
        return "ok"
    r, c = (int(v) for v in bad[0])
    return (f"{bad.shape[0]} wrong; first: row {r} (one-hot at k = {ks[r]}), column {c}: got "
            f"{float(got[r, c])}, weight is {float(exact[r, c])}")


# ---------------------------------------------------------------------------------
# SiLU / norm epilogues: exact gate and up sums, fp64 reference, 1-ULP comparison
# ---------------------------------------------------------------------------------

def row_rms_scale(x: torch.Tensor, eps: float) -> torch.Tensor:
    """rsqrt(mean(x^2) + eps) per row in fp64, [m, 1]."""
    return torch.rsqrt(x.double().pow(2).mean(-1, keepdim=True) + eps)


def silu_ref(gate: torch.Tensor, up: torch.Tensor, row_scale: Optional[torch.Tensor] = None):
    """bf16(silu(g) u) of exact fp64 gate / up sums (``row_scale`` [m, 1] applied to both
    first: the fused-norm kernels), computed in fp64 and rounded once.  Asserts
    max |g| < MAX_GATE."""
    g, u = gate.double(), up.double()
    if row_scale is not None:
        g, u = g * row_scale, u * row_scale
    assert float(g.abs().max()) < MAX_GATE, f"max |g| = {float(g.abs().max())} >= {MAX_GATE}"
    return (g / (1.0 + torch.exp(-g)) * u).to(torch.bfloat16)


def silu_operands(m: int, inter: int, k: int, x_max: int = 7, w_max: int = 15, seed: int = 0,
                  norm_eps: Optional[float] = None, hot: int = 4, device="cpu"):
    """(x [m, k], w [2 inter, k] gate rows then up rows, gate, up): integer operands for
    the SiLU epilogues.  w_shift is picked so the gates have a standard deviation of
    about 3 (most in [-8, 8]; after the row RMS scale when ``norm_eps`` is given); the
    first ``hot`` gate columns are scaled by a power of two so their largest |g| lies in
    [30, 60), with alternating signs, where exp over- or underflows its useful range.
    gate / up are the exact fp64 sums (without the row scale)."""
    g = torch.Generator().manual_seed(seed)
    xd = _randint(-x_max, x_max, (m, k), g).double()
    wi = _randint(-w_max, w_max, (2 * inter, k), g).double()
    rs = row_rms_scale(xd, norm_eps) if norm_eps is not None else torch.ones(m, 1, dtype=torch.float64)
    gi = (xd @ wi[:inter].t()) * rs                       # gates in integer units
    std = float(gi[:, hot:].std()) if gi[:, hot:].numel() > 1 else float(gi.abs().max())
    w_shift = max(0, round(math.log2(max(std, 1.0) / 3.0)))
    unit = 2.0 ** -w_shift
    wd = wi * unit
    gate = gi * unit
    for j in range(min(hot, inter)):
        col = gate[:, j]
        top = int(col.abs().argmax())
        scale = 2.0 ** math.floor(math.log2(0.999 * MAX_GATE / float(col[top].abs())))
        assert scale >= 1.0, "hot column already past the range"
        if (col[top] > 0) != (j % 2 == 0):
            scale = -scale
        wd[j] *= scale
    assert_bf16_exact(xd, "x")
    assert_bf16_exact(wd, "w")
    x, w = xd.to(torch.bfloat16).to(device), wd.to(torch.bfloat16).to(device)
    assert_exact_bound(x, w, unit)
    y = exact_product(x, w)
    gate, up = y[:, :inter], y[:, inter:]
    if hot >= 2 and inter >= 2:
        gs = gate * rs.to(device)
        assert float(gs.max()) >= 30.0 and float(gs.min()) <= -30.0, "hot columns miss +-30"
    return x, w, gate, up


def w4_silu_operands(m: int, inter: int, k: int, x_max: int = 2, seed: int = 0, hot: int = 4,
                     device="cpu"):
    """(x, q [2 inter, k], z, s, gate, up) for the W4 SiLU epilogues: as
    :func:`w4_int_operands` with gate rows then up rows; the three adjacent scales start
    at the power of two that gives the gates a standard deviation of about 3, and the
    first ``hot`` gate rows get a larger power-of-two scale (and q -> 15 - q, z -> 15 - z
    to flip the sign) so their largest |g| lies in [30, 60) with alternating signs."""
    g = torch.Generator().manual_seed(seed)
    n, ng = 2 * inter, k // W4_GROUP
    xd = _randint(-x_max, x_max, (m, k), g).double()
    q = _randint(0, 15, (n, k), g).to(torch.uint8)
    z = _randint(0, 15, (n, ng), g).to(torch.uint8)
    e = _randint(0, 2, (n, ng), g).double()
    gi = xd @ w4_dequant_exact(q[:inter], z[:inter], torch.pow(2.0, e[:inter])).t()
    std = float(gi[:, hot:].std()) if gi[:, hot:].numel() > 1 else float(gi.abs().max())
    s_exp = -max(0, round(math.log2(max(std, 1.0) / 3.0)))
    e = e + s_exp
    gate = gi * 2.0 ** s_exp
    for j in range(min(hot, inter)):
        col = gate[:, j]
        top = int(col.abs().argmax())
        shift = math.floor(math.log2(0.999 * MAX_GATE / float(col[top].abs())))
        assert shift >= 0, "hot column already past the range"
        e[j] += shift
        if (col[top] > 0) != (j % 2 == 0):
            q[j], z[j] = 15 - q[j], 15 - z[j]
    s = torch.pow(2.0, e).float()
    assert_bf16_exact(xd, "x")
    x = xd.to(torch.bfloat16).to(device)
    q, z, s = q.to(device), z.to(device), s.to(device)
    assert_w4_bound(x, q, z, s)
    y = x.double() @ w4_dequant_exact(q, z, s).t()
    gate, up = y[:, :inter], y[:, inter:]
    if hot >= 2 and inter >= 2:
        assert float(gate.max()) >= 30.0 and float(gate.min()) <= -30.0, "hot columns miss +-30"
    return x, q, z, s, gate, up


def bf16_ulp_diff(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Element-wise distance of two bf16 tensors in bf16 steps (int32): the int16 bit
    patterns mapped to a monotone integer, so +0 and -0 coincide and the distance runs
    across powers of two and the sign change.  A NaN on either side counts 1 << 16."""
    assert a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16 and a.shape == b.shape

    def key(t):
        bits = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
        mag = bits & 0x7FFF
        return torch.where(bits >= 0x8000, -mag, mag)

    d = (key(a) - key(b)).abs()
    return torch.where(torch.isnan(a.float()) | torch.isnan(b.float()), torch.full_like(d, 1 << 16), d)


def assert_ulp1(got: torch.Tensor, ref: torch.Tensor, what: str) -> float:
    """Every element within one bf16 step of ``ref``; prints (does not assert on) the
    share of elements one step off and returns it."""
    d = bf16_ulp_diff(got, ref)
    worst = int(d.max())
    share = float((d == 1).double().mean())
    print(f"{what}: {100.0 * share:.3f}% of {d.numel()} elements one bf16 step off, max {worst}")
    if worst > 1:
        idx = tuple(int(v) for v in (d > 1).nonzero()[0])
        raise AssertionError(f"{what}: {int((d > 1).sum())} elements more than one bf16 step off, "
                             f"max {worst}; first at {idx}: got {float(got[idx])}, "
                             f"reference {float(ref[idx])}")
    return share


# ---------------------------------------------------------------------------------
# guarded buffers
# ---------------------------------------------------------------------------------

_BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32,
         torch.int32: torch.int32}
LEAD_COLS = 8   # elements in front of every row of a guarded view (>= 16 bytes)


def _fill_bits(buf: torch.Tensor, fill: int) -> None:
    bits = buf.view(_BITS[buf.dtype])
    if bits.dtype == torch.int16 and fill >= 0x8000:
        fill -= 0x10000
    if bits.dtype == torch.int32 and fill >= 0x80000000:
        fill -= 0x100000000
    bits.fill_(fill)


@dataclasses.dataclass
class Guarded:
    """``view`` [rows, cols] inside ``buf``; everything else holds the fill pattern."""
    buf: torch.Tensor
    view: torch.Tensor
    region: Tuple[slice, ...]
    fill: int

    def check(self, what: str = "buffer") -> None:
        """Asserts, by bit pattern, that nothing outside the view has changed."""
        bits = self.buf.view(_BITS[self.buf.dtype]).clone()
        ref = torch.empty_like(self.buf)
        _fill_bits(ref, self.fill)
        ref = ref.view(_BITS[self.buf.dtype])
        bits[self.region] = ref[self.region]
        bad = (bits != ref).nonzero()
        if bad.numel():
            where = tuple(int(v) for v in bad[0])
            inside = tuple((sl.start, sl.stop) for sl in self.region)
            raise AssertionError(f"{what}: {bad.shape[0]} elements outside the view changed; first "
                                 f"at buffer index {where} (view spans {inside})")


def guarded(rows: int, cols: int, pad_rows: int = 16, pad_cols: int = 64,
            dtype: torch.dtype = torch.bfloat16, fill: int = PAD_BF16, device="cpu",
            lead_cols: int = LEAD_COLS) -> Guarded:
    """A [rows, cols] view with ``pad_rows`` rows above and below, ``lead_cols`` elements
    in front of and >= ``pad_cols`` elements behind every row, all holding the bit pattern
    ``fill``.  The row stride is a multiple of 8 elements and the view's base 16-byte
    aligned (what the bindings require of strided operands).  ``pad_cols = lead_cols = 0``
    with ``cols % 8 == 0`` gives a contiguous view guarded by rows alone."""
    assert lead_cols % 8 == 0
    stride = (lead_cols + cols + pad_cols + 7) // 8 * 8
    buf = torch.empty(rows + 2 * pad_rows, stride, dtype=dtype, device=device)
    _fill_bits(buf, fill)
    region = (slice(pad_rows, pad_rows + rows), slice(lead_cols, lead_cols + cols))
    view = buf[region]
    assert view.stride(0) % 8 == 0 and view.data_ptr() % 16 == 0
    return Guarded(buf, view, region, fill)


def guarded_from(t: torch.Tensor, pad_rows: int = 16, pad_cols: int = 64,
                 fill: Optional[int] = None) -> Guarded:
    """:func:`guarded` holding a copy of the 2-D tensor ``t`` (default fill: NaN)."""
    if fill is None:
        fill = NAN_F32 if t.dtype == torch.float32 else NAN_BF16
    g = guarded(t.shape[0], t.shape[1], pad_rows, pad_cols, t.dtype, fill, t.device)
    g.view.copy_(t)
    return g


def guarded_flat(n: int, tail: int = 4096, dtype: torch.dtype = torch.float32,
                 fill: int = NAN_F32, device="cpu") -> Guarded:
    """A flat contiguous buffer of ``n + tail`` elements, ALL pre-filled with ``fill``
    (NaN by default: a workspace element no kernel wrote stays NaN); ``view`` is the
    first ``n``, ``check()`` covers the tail.  Pass ``buf`` to the kernel."""
    buf = torch.empty(n + tail, dtype=dtype, device=device)
    _fill_bits(buf, fill)
    region = (slice(0, n),)
    return Guarded(buf, buf[region], region, fill)


# ---------------------------------------------------------------------------------
# attention: an exactly predictable softmax in which every key stays visible
# ---------------------------------------------------------------------------------
#
# Scores are integers in log2 units (integer q and K, softmax scale ln 2), so every
# p = exp2(score - max) is a power of two; V is one-hot per key (key j holds one small
# integer v_j in one dim, its CHANNEL) and the keys of a channel share one score level,
# so every output element is (sum of v over the visible keys of its channel) * 2**level
# / l: each key carries v_j / sum(v) of one element, several bf16 steps, however far
# below the row maximum its channel lies.
#
# * key family: channel of key j = (class (j + h) % G, dim (j // G + 37 h) % D); head r
#   sees class-r keys at their level and every other key ATTN_S levels lower.
# * tile family: the 16 keys of a 16-token tile share channel (tile + 7 h) % D; levels
#   swing by more than the kernels' rescale threshold (8) between neighbouring tiles
#   and between neighbouring 8-tile ranges; even heads read them with q = +1, odd heads
#   with q = -1, so heads that share a wave-wide rescale ballot have opposite histories.
#
# Per kv head the special dims sit at different places (a seeded permutation); the
# other K dims hold random integers where q is zero and the other q dims where K is
# zero (decoys: a misaligned dim pairing shows).  Every cache slot outside a sequence
# (positions >= L, unreferenced blocks, a poison block behind every table row) holds
# FINITE poison: K = ATTN_POISON in a dim where every q is +1, V = 3 in every dim.

ATTN_S = 40                 # class separation: >= level span (12) + 24; 40 / 2**k is e4m3-exact
ATTN_POISON = 40            # score of an admitted poison key (valid scores stay <= 22)
ATTN_SCALE = math.log(2.0)  # the softmax scale the launches pass: scale * log2(e) = 1
ATTN_MIN_SHARE = 3.0 * 2.0 ** -7   # visibility: one step of error, one allowed, one margin
ATTN_FAMILIES = ("key", "tile")
_TILE_A = (-10, 6, -12, 8)                    # per 8-tile range
_TILE_B = (0, 10, -10, 9, -1, 10, -9, 2)      # per tile of a range: the sum spans -22 .. +18
ATTN_K_SCALES = (0.5, 1.0, 2.0, 4.0)
ATTN_V_SCALES = (2.0, 0.25, 1.0, 0.5)


def _hash(x: torch.Tensor) -> torch.Tensor:
    """A small integer hash (int64 in, int64 in [0, 2**16) out)."""
    x = (x * 2654435761 + 12345) & 0xFFFFFFFF
    x = (x ^ (x >> 13)) * 1274126177 & 0xFFFFFFFF
    return (x >> 9) & 0xFFFF


def attn_key_channel(j: torch.Tensor, h: int, g: int, d: int):
    """(class, dim) of key j of kv head h in the key family."""
    return (j + h) % g, (j // g + 37 * h) % d


def attn_key_level(cls: torch.Tensor, dim: torch.Tensor, h: int) -> torch.Tensor:
    """Level of a key-family channel, in [-6, 6]."""
    return _hash(cls * 1009 + dim * 31 + h * 7919) % 13 - 6


def attn_tile_channel(tile: torch.Tensor, h: int, d: int) -> torch.Tensor:
    return (tile + 7 * h) % d


def attn_tile_level(chan: torch.Tensor, h: int, d: int) -> torch.Tensor:
    """Level of a tile-family channel, in [-22, 18]."""
    c = (chan + 3 * h) % d
    a = torch.tensor(_TILE_A, dtype=torch.int64)
    b = torch.tensor(_TILE_B, dtype=torch.int64)
    return a[(c // 8) % 4] + b[c % 8]


def attn_v_max(family: str, max_len: int, g: int, d: int) -> int:
    """Largest v range 1..v_max for which every key of a ``max_len`` sequence carries at
    least ATTN_MIN_SHARE of its channel: a key-family channel holds n = ceil(L / (G D))
    keys, the smallest share is 1 / (1 + v_max (n - 1)); a tile-family channel is judged
    per tile (the weight of a whole tile is the unit there), n = ceil(tiles / D)."""
    n = -(-max_len // (g * d)) if family == "key" else -(-(-(-max_len // 16)) // d)
    for v in (3, 2, 1):
        if 1.0 / (1 + v * (n - 1)) >= ATTN_MIN_SHARE:
            return v
    raise AssertionError(f"{family} family: {n} keys per channel at L = {max_len}, G = {g}, "
                         f"D = {d} cannot meet the visibility condition")


@dataclasses.dataclass(frozen=True)
class AttnCase:
    """One attention test case.  ``lens``: total tokens per sequence; ``q_lens``: new
    tokens per sequence (prefill) or None (decode: one query per sequence)."""
    family: str
    lens: Tuple[int, ...]
    nq: int
    nkv: int
    d: int
    block_size: int = 16
    q_lens: Optional[Tuple[int, ...]] = None
    kv8: bool = False
    scales: bool = False
    q_pad: int = 0            # extra elements per q row (q read out of a wider buffer)

    @property
    def g(self) -> int:
        return self.nq // self.nkv

    @property
    def name(self) -> str:
        kind = "decode" if self.q_lens is None else "prefill"
        kv = ("fp8s" if self.scales else "fp8") if self.kv8 else "bf16"
        lens = ",".join(map(str, self.lens)) if len(self.lens) <= 12 else f"{len(self.lens)}seqs"
        return f"{kind}-{self.family}-d{self.d}g{self.g}kv{self.nkv}-bs{self.block_size}-{kv}-[{lens}]"


@dataclasses.dataclass
class AttnOperands:
    case: AttnCase
    q_buf: torch.Tensor          # bf16 [T + 2, q_pad_lead + nq d + q_pad] NaN outside q
    q: torch.Tensor              # view [T, nq d], row stride > nq d when q_pad
    k_cache: torch.Tensor        # [blocks, nkv, bs, d] bf16 or float8_e4m3fn
    v_cache: torch.Tensor        # [blocks, nkv, d, bs]
    block_tables: torch.Tensor   # int32 [B, max blocks + 2], poison block past a row's end
    seq_lens: torch.Tensor       # int32 [B]
    q_start_loc: torch.Tensor    # int32 [B + 1]
    k_scale: Optional[torch.Tensor]
    v_scale: Optional[torch.Tensor]
    poison_block: int
    free_blocks: List[int]       # unreferenced blocks (poison)
    dims: torch.Tensor           # int64 [nkv, G + 4]: class dims, A0, A1, B, P per kv head
    v_max: int

    def to(self, device) -> "AttnOperands":
        o = dataclasses.replace(self)
        for f in ("q_buf", "k_cache", "v_cache", "block_tables", "seq_lens", "q_start_loc",
                  "k_scale", "v_scale"):
            t = getattr(self, f)
            setattr(o, f, None if t is None else t.to(device))
        lead = LEAD_COLS if self.case.q_pad else 0
        nqd = self.case.nq * self.case.d
        o.q = o.q_buf[1:-1, lead: lead + nqd]
        return o


def _f8_store(x: torch.Tensor, name: str) -> torch.Tensor:
    s = x.to(torch.float8_e4m3fn)
    assert torch.equal(s.float(), x.float()), f"{name} does not round-trip through e4m3"
    return s


def attn_operands(case: AttnCase, seed: int = 0) -> AttnOperands:
    """Operands of ``case`` on the CPU (see the section comment).  Asserts that every
    stored value round-trips through its format."""
    c = case
    assert c.family in ATTN_FAMILIES and c.nq % c.nkv == 0
    g, d, bs, nkv = c.g, c.d, c.block_size, c.nkv
    assert g + 4 <= d // 4
    gen = torch.Generator().manual_seed(seed * 7919 + 13)
    nseq = len(c.lens)
    q_lens = [1] * nseq if c.q_lens is None else list(c.q_lens)
    assert len(q_lens) == nseq and all(0 <= a <= l or c.q_lens is None for a, l in zip(q_lens, c.lens))
    v_max = attn_v_max(c.family, max(max(c.lens), 1), g, d)
    if c.scales:
        assert c.kv8
        ks = torch.tensor([ATTN_K_SCALES[h % 4] for h in range(nkv)], dtype=torch.float32)
        vs = torch.tensor([ATTN_V_SCALES[h % 4] for h in range(nkv)], dtype=torch.float32)
    else:
        ks = vs = None
    ksd = ks.double() if ks is not None else torch.ones(nkv, dtype=torch.float64)
    vsd = vs.double() if vs is not None else torch.ones(nkv, dtype=torch.float64)

    # dims per kv head: a seeded permutation; the first G + 4 are special, of the rest
    # the even-indexed hold K decoys (q = 0), the odd-indexed q decoys (K = 0)
    perm = torch.stack([torch.randperm(d, generator=gen) for _ in range(nkv)])
    dims = perm[:, : g + 4]
    k_dec, q_dec = perm[:, g + 4:][:, 0::2], perm[:, g + 4:][:, 1::2]
    a0, a1, bd, pd = (dims[:, g + i] for i in range(4))

    # ---- caches: poison everywhere, then the sequences' keys --------------------------
    nb = [-(-l // bs) for l in c.lens]
    n_free = 3
    total = sum(nb) + n_free + 1
    ids = torch.randperm(total, generator=gen)
    poison_block = int(ids[-1])
    free_blocks = [int(v) for v in ids[sum(nb): sum(nb) + n_free]]
    kc = torch.zeros(total, nkv, bs, d, dtype=torch.float32)      # small integers: fp32 holds them
    vc = torch.full((total, nkv, d, bs), 3.0, dtype=torch.float32)
    hh = torch.arange(nkv)
    kc[:, hh, :, pd] = float(ATTN_POISON)
    bt = torch.full((nseq, max(nb + [0]) + 2), poison_block, dtype=torch.int32)
    at = 0
    for b, l in enumerate(c.lens):
        bt[b, : nb[b]] = ids[at: at + nb[b]].int()
        at += nb[b]
        if l == 0:
            continue
        j = torch.arange(l)
        blk, off = bt[b, j // bs].long(), j % bs
        for h in range(nkv):
            rows = torch.zeros(l, d, dtype=torch.float32)
            rows[:, k_dec[h]] = _randint(-8, 8, (l, k_dec.shape[1]), gen).float()
            if c.family == "key":
                cls, dim = attn_key_channel(j, h, g, d)
                lvl = attn_key_level(cls, dim, h)
                rows[j, dims[h, cls]] = float(ATTN_S)
                rows[:, bd[h]] = -float(ATTN_S)
            else:
                dim = attn_tile_channel(j // 16, h, d)
                lvl = attn_tile_level(dim, h, d)
            rows[:, a0[h]] = (lvl // 2).float()
            rows[:, a1[h]] = (lvl - lvl // 2).float()
            val = 1 + _hash(j * 131 + h * 17 + b * 7) % v_max
            kc[blk, h, off] = rows
            vc[blk, h, :, off] = 0.0
            vc[blk, h, dim, off] = val.float()
    kst = kc.div_(ksd.float().view(1, nkv, 1, 1))   # powers of two: exact
    vst = vc.div_(vsd.float().view(1, nkv, 1, 1))
    if c.kv8:
        k_cache, v_cache = _f8_store(kst, "K cache"), _f8_store(vst, "V cache")
    else:
        assert_bf16_exact(kst, "K cache")
        assert_bf16_exact(vst, "V cache")
        k_cache, v_cache = kst.to(torch.bfloat16), vst.to(torch.bfloat16)

    # ---- q: [T, nq, d] ---------------------------------------------------------------
    t = sum(q_lens)
    qd = torch.zeros(t, nkv, g, d, dtype=torch.float64)
    for h in range(nkv):
        qd[:, h][:, :, q_dec[h]] = _randint(-8, 8, (t, g, q_dec.shape[1]), gen).double()
        qd[:, h, :, pd[h]] = 1.0
        if c.family == "key":
            qd[:, h, torch.arange(g), dims[h, :g]] = 1.0
            sign = torch.ones(g, dtype=torch.float64)
            qd[:, h, :, bd[h]] = 1.0
        else:
            sign = torch.tensor([1.0 if r % 2 == 0 else -1.0 for r in range(g)], dtype=torch.float64)
        qd[:, h, :, a0[h]] = sign
        qd[:, h, :, a1[h]] = sign
    assert_bf16_exact(qd, "q")
    lead = LEAD_COLS if c.q_pad else 0
    q_buf = torch.empty(t + 2, lead + c.nq * d + c.q_pad, dtype=torch.bfloat16)
    _fill_bits(q_buf, NAN_BF16)
    q = q_buf[1:-1, lead: lead + c.nq * d]
    q.copy_(qd.view(t, c.nq * d).to(torch.bfloat16))
    qsl = torch.tensor([0] + list(torch.tensor(q_lens).cumsum(0)), dtype=torch.int32)
    return AttnOperands(c, q_buf, q, k_cache, v_cache, bt, torch.tensor(c.lens, dtype=torch.int32),
                        qsl, ks, vs, poison_block, free_blocks, dims, v_max)


# ---- the fp64 paged reference (with hooks for the mutation catalogue) ---------------------

@dataclasses.dataclass
class AttnMutation:
    """A deliberate fault of the fp64 reference (tests/unit/test_exact_attention_cpu.py:
    the proof that the comparison can fail).  ``seq`` / ``kvh`` select the segment."""
    seq: int = 0
    kvh: int = 0
    drop: Tuple[int, ...] = ()           # key positions left out
    dup: Tuple[int, ...] = ()            # key positions read twice
    admit_len: bool = False              # position L let through the mask
    admit_free: bool = False             # a key of an unreferenced block read as position 0's twin
    swap_blocks: Optional[Tuple[int, int]] = None   # two table entries exchanged
    read_kvh: Optional[int] = None       # K and V of another kv head
    k_scale_of: Optional[int] = None     # another head's k_scale
    v_scale_of: Optional[int] = None
    causal: int = 0                      # +1 / -1 on the causal limit (prefill)
    merge_m_from_head: Optional[Tuple[int, int]] = None  # (partial tile range start, length): alpha of head r + 1
    merge_twice: Optional[Tuple[int, int]] = None        # partial [start, start + n) keys merged twice
    masked_weight_one: bool = False      # keys past the causal limit of the last 64-tile added with weight 1
    skip_rescale_at: Optional[int] = None  # first key of a tile whose upward jump is not applied to l and O


def _attn_gather(o: AttnOperands, b: int, h: int, pos: torch.Tensor, table: torch.Tensor,
                 ks: float, vs: float):
    bs = o.case.block_size
    blk, off = table[pos // bs].long(), pos % bs
    k = o.k_cache[blk, h, off].double() * ks
    v = o.v_cache[blk, h, :, off].double() * vs
    return k, v


def attn_reference(o: AttnOperands, mut: Optional[AttnMutation] = None,
                   return_scores: bool = False):
    """out [T, nq d] bf16: fp64 attention through the block tables, exact integer scores,
    exp2, sum, divide, one RNE to bf16.  Decode rows see positions < L, prefill row i of a
    sequence positions <= L - q_len + i.  Empty rows are zero."""
    c = o.case
    g, d, nkv = c.g, c.d, c.nkv
    cpu = lambda x: None if x is None else x.cpu()
    o = dataclasses.replace(o, k_cache=o.k_cache.cpu(), v_cache=o.v_cache.cpu())
    q = o.q.cpu().double().view(-1, nkv, g, d)
    bt, sl, qsl = cpu(o.block_tables), cpu(o.seq_lens), cpu(o.q_start_loc)
    ks = cpu(o.k_scale).double() if o.k_scale is not None else torch.ones(nkv, dtype=torch.float64)
    vs = cpu(o.v_scale).double() if o.v_scale is not None else torch.ones(nkv, dtype=torch.float64)
    out = torch.zeros(q.shape[0], nkv, g, d, dtype=torch.float64)
    scores = {}
    for b in range(len(c.lens)):
        L, q0, q1 = int(sl[b]), int(qsl[b]), int(qsl[b + 1])
        if L == 0 or q1 == q0:
            continue
        # position limit (exclusive) of every query row
        if c.q_lens is None:
            lim = torch.full((1,), L, dtype=torch.int64)
        else:
            lim = L - (q1 - q0) + torch.arange(q1 - q0) + 1
        for h in range(nkv):
            m = mut if (mut is not None and mut.seq == b and mut.kvh == h) else None
            pos = torch.arange(L)
            table = bt[b].clone()
            rh, kh, vh = h, h, h
            always = torch.zeros(L, dtype=torch.bool)    # entries no mask applies to
            if m is not None:
                if m.drop:
                    keep = torch.ones(L, dtype=torch.bool)
                    keep[list(m.drop)] = False
                    pos, always = pos[keep], always[keep]
                if m.dup:
                    pos = torch.cat([pos, torch.tensor(m.dup)])
                    always = torch.cat([always, torch.zeros(len(m.dup), dtype=torch.bool)])
                if m.admit_len:
                    pos = torch.cat([pos, torch.tensor([L])])
                    always = torch.cat([always, torch.ones(1, dtype=torch.bool)])
                if m.swap_blocks is not None:
                    i0, i1 = m.swap_blocks
                    table[i0], table[i1] = bt[b, i1], bt[b, i0]
                if m.read_kvh is not None:
                    rh = m.read_kvh
                if m.k_scale_of is not None:
                    kh = m.k_scale_of
                if m.v_scale_of is not None:
                    vh = m.v_scale_of
            k, v = _attn_gather(o, b, rh, pos, table, float(ks[kh]), float(vs[vh]))
            if m is not None and m.admit_free:
                fk = o.k_cache[o.free_blocks[0], rh, 0].double() * float(ks[kh])
                fv = o.v_cache[o.free_blocks[0], rh, :, 0].double() * float(vs[vh])
                k, v = torch.cat([k, fk[None]]), torch.cat([v, fv[None]])
                pos = torch.cat([pos, torch.tensor([0])])
                always = torch.cat([always, torch.ones(1, dtype=torch.bool)])
            s = torch.einsum("tgd,nd->tgn", q[q0:q1, h], k)          # [rows, g, n] exact integers
            if m is None:
                assert torch.equal(s, s.round()), "scores are not integers"
            lm = lim + (m.causal if m is not None else 0)
            vis = (pos[None, :] < lm[:, None]) | always[None, :]     # [rows, n]
            if return_scores:
                scores[(b, h)] = (s, vis, pos)
            s = s.masked_fill(~vis[:, None, :], float("-inf"))
            mx = s.max(-1, keepdim=True).values
            if m is not None and (m.merge_m_from_head or m.merge_twice or m.masked_weight_one
                                  or m.skip_rescale_at is not None):
                num, den = _attn_mutant_merge(s, v, pos, vis, m, g)
            else:
                p = torch.exp2(s - mx)
                num, den = p @ v, p.sum(-1, keepdim=True)
            out[q0:q1, h] = num / den
    ref = out.view(-1, c.nq * d).to(torch.bfloat16)
    return (ref, scores) if return_scores else ref


def _attn_mutant_merge(s, v, pos, vis, m: AttnMutation, g: int):
    """(numerator [rows, g, d], denominator [rows, g, 1]) of a softmax whose partial
    merge is faulty.  ``s`` is already masked."""
    def part(sel, ss=None):
        ss = s if ss is None else ss
        sp = ss[:, :, sel]
        mp = sp.max(-1, keepdim=True).values
        mp0 = torch.where(torch.isinf(mp), torch.zeros_like(mp), mp)
        p = torch.exp2(sp - mp0)
        return mp, p @ v[sel], p.sum(-1, keepdim=True)

    if m.merge_m_from_head is not None or m.merge_twice is not None:
        lo, n = m.merge_m_from_head if m.merge_m_from_head is not None else m.merge_twice
        inside = (pos >= lo) & (pos < lo + n)
        m1, o1, l1 = part(inside)
        m0, o0, l0 = part(~inside)
        if m.merge_m_from_head is not None:
            m1w = torch.roll(m1, -1, dims=1)   # the weight uses the neighbouring head's m
        else:
            m1w = m1
        big = torch.maximum(m0, m1w)
        e0, e1 = torch.exp2(m0 - big), torch.exp2(m1w - big)
        e0, e1 = torch.nan_to_num(e0), torch.nan_to_num(e1)
        if m.merge_twice is not None:
            e1 = 2.0 * e1
        return e0 * o0 + e1 * o1, e0 * l0 + e1 * l1
    if m.masked_weight_one:
        # the keys of the last 64-token tile that the row's causal mask hides, as a
        # partial of their own computed without the mask and merged with weight 1
        last = (int(pos.max()) // 64) * 64
        mx = s.max(-1, keepdim=True).values
        p = torch.exp2(s - mx)
        num, den = p @ v, p.sum(-1, keepdim=True)
        hidden = (~vis) & (pos >= last)[None, :]                      # [rows, n]
        return num + hidden.double()[:, None, :] @ v, den + hidden.double().sum(-1)[:, None, None]
    # skip_rescale_at: sequential tiles of 16 keys; at the tile that starts at this key
    # the reference max moves up but l and O keep their old scale
    order = torch.argsort(pos, stable=True)
    rows = s.shape[0]
    mr = torch.full((rows, g, 1), float("-inf"), dtype=torch.float64)
    lr = torch.zeros(rows, g, 1, dtype=torch.float64)
    orr = torch.zeros(rows, g, v.shape[1], dtype=torch.float64)
    for t0 in range(0, int(pos.max()) + 1, 16):
        sel = order[(pos[order] >= t0) & (pos[order] < t0 + 16)]
        st = s[:, :, sel]
        mn = torch.maximum(mr, st.max(-1, keepdim=True).values)
        alpha = torch.nan_to_num(torch.exp2(mr - mn))
        alpha = torch.where(torch.isinf(mn), torch.ones_like(alpha), alpha)
        if t0 == m.skip_rescale_at:
            alpha = torch.ones_like(alpha)
        mn0 = torch.where(torch.isinf(mn), torch.zeros_like(mn), mn)
        p = torch.exp2(st - mn0)
        lr = lr * alpha + p.sum(-1, keepdim=True)
        orr = orr * alpha + p @ v[sel]
        mr = mn
    return orr, lr


# ---- self-checks -----------------------------------------------------------------------------

def attn_self_check(o: AttnOperands) -> float:
    """Asserts the operand design on the drawn operands: every valid score is the integer
    the design predicts (own level; ATTN_S lower for another class; -level for odd heads
    of the tile family), so the decoys pair with zeros and a level depends on the channel
    only; poison scores ATTN_POISON and holds V = 3; the visibility condition.  Returns
    the smallest share (of a key in the key family, of a tile in the tile family)."""
    c = o.case
    g, d, nkv = c.g, c.d, c.nkv
    assert_bf16_exact(o.q.double(), "q")
    _, info = attn_reference(o, return_scores=True)
    worst = 1.0
    for (b, h), (s, vis, pos) in info.items():
        L = int(o.seq_lens[b])
        s = s[-1]                                  # the row that sees every key: [g, L]
        assert bool(vis[-1].all())
        r = torch.arange(g)[:, None]
        if c.family == "key":
            cls, dim = attn_key_channel(pos, h, g, d)
            lvl = attn_key_level(cls, dim, h)
            want = lvl[None, :] - ATTN_S * (cls[None, :] != r).long()
            chan, unit = cls * d + dim, pos
        else:
            dim = attn_tile_channel(pos // 16, h, d)
            lvl = attn_tile_level(dim, h, d)
            want = lvl[None, :] * torch.where(r % 2 == 0, 1, -1)
            chan, unit = dim, pos // 16
        assert torch.equal(s, want.double()), f"scores of sequence {b}, kv head {h} differ from the design"
        # one level per channel
        lo = torch.full((int(chan.max()) + 1,), 1 << 20).scatter_reduce(0, chan, lvl, "amin")
        hi = torch.full((int(chan.max()) + 1,), -(1 << 20)).scatter_reduce(0, chan, lvl, "amax")
        assert bool((lo[chan] == hi[chan]).all()), "a channel holds keys of two levels"
        # shares: v of a key (of a tile) over the v of its channel
        bs = c.block_size
        blk, off = o.block_tables[b, pos // bs].long(), pos % bs
        vrow = o.v_cache[blk, h, :, off].double() * (float(o.v_scale[h]) if o.v_scale is not None else 1.0)
        val = vrow.sum(-1)
        assert bool((vrow[torch.arange(L), dim] == val).all()) and bool((val >= 1).all()) and bool((val <= 3).all())
        csum = torch.zeros(int(chan.max()) + 1, dtype=torch.float64).scatter_add(0, chan, val)
        if c.family == "key":
            share = val / csum[chan]
        else:
            usum = torch.zeros(int(unit.max()) + 1, dtype=torch.float64).scatter_add(0, unit, val)
            share = usum[unit] / csum[chan]
        worst = min(worst, float(share.min()))
    assert worst >= ATTN_MIN_SHARE, (f"{c.name}: a {'key' if c.family == 'key' else 'tile'} carries only "
                                     f"{100 * worst:.2f}% of its output element")
    # poison: score ATTN_POISON against every head, V = 3 in every dim
    pk = o.k_cache[o.poison_block].double()        # [nkv, bs, d]
    pv = o.v_cache[o.poison_block].double()
    ks = o.k_scale.double() if o.k_scale is not None else torch.ones(nkv, dtype=torch.float64)
    vs = o.v_scale.double() if o.v_scale is not None else torch.ones(nkv, dtype=torch.float64)
    q = o.q.double().view(-1, nkv, g, d)
    sp = torch.einsum("thgd,hnd->thgn", q, pk * ks.view(nkv, 1, 1))
    assert bool((sp == ATTN_POISON).all()) and bool((pv * vs.view(nkv, 1, 1) == 3.0).all())
    for blk in o.free_blocks:
        assert torch.equal(o.k_cache[blk].double(), pk) and torch.equal(o.v_cache[blk].double(), pv)
    return worst


# ---- case tables (tests/unit/test_exact_attention_cpu.py and tests/test_attention_exact_gpu.py) ------

def attn_instantiated(kind: str) -> List[Tuple[int, int]]:
    """(D, G) pairs the ``decode`` / ``prefill`` dispatcher instantiates, read from its
    source (csrc/kernels): the tests cover the list itself, not a copy."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    name, pat = {"decode": ("attn_decode.hip", r"^\s*FT_DEC_CASE\((\d+), (\d+), 2\)"),
                 "prefill": ("attn_prefill.hip", r"^\s*FT_PF_CASE\((\d+), (\d+)\)")}[kind]
    with open(os.path.join(root, "csrc", "kernels", name)) as f:
        pairs = [(int(a), int(b)) for a, b in re.findall(pat, f.read(), re.M)]
    assert pairs, f"no instantiations found in {name}"
    return pairs


ATTN_BASE_LENS = (0, 1, 15, 16, 17, 255, 256, 257, 1000, 2100)
ATTN_DECODE_LENS = (ATTN_BASE_LENS, ATTN_BASE_LENS[::-1], (1,), (16,), (2100,))
ATTN_DECODE_BLOCKS = (16, 32, 64, 128)
ATTN_PREFILL_SEQS = ((1, 0), (5, 0), (64, 0), (65, 0), (77, 33), (16, 300), (130, 1), (3, 500),
                     (1, 63), (1, 64), (9, 2039))     # (new tokens, cached prefix)
ATTN_MANY_LENS = tuple(1 + (7 * i) % 40 for i in range(130))   # the prefix scan walks 64 at a time
ATTN_LONG_LENS = (4100,) * 16      # with nkv = 8: 32896 tiles > 64 x the 512 waves of the bf16 grid
ATTN_KINDS = (("bf16", False, False), ("fp8", True, False), ("fp8s", True, True))


def attn_decode_base_cases() -> List[AttnCase]:
    return [AttnCase(f, lens, 2 * g, 2, d, bs)
            for d, g in attn_instantiated("decode") for f in ATTN_FAMILIES
            for lens in ATTN_DECODE_LENS for bs in ATTN_DECODE_BLOCKS]


def attn_decode_path_cases() -> List[AttnCase]:
    """Cases every decode path (combine kernel, fused combine, pieces) runs: each cache
    kind at G = 4, D = 128, and the fp8 kinds at D = 64 too (one 64-dim pair per row)."""
    return [AttnCase(f, ATTN_BASE_LENS, 2 * g, 2, d, 16, None, kv8, sc)
            for f in ATTN_FAMILIES for _, kv8, sc in ATTN_KINDS
            for d, g in (((128, 4), (64, 8)) if kv8 else ((128, 4),))]


def attn_decode_special_cases() -> List[AttnCase]:
    return ([AttnCase(f, ATTN_MANY_LENS, 8, 2, 128) for f in ATTN_FAMILIES] +
            [AttnCase(f, ATTN_LONG_LENS, 32, 8, 128) for f in ATTN_FAMILIES] +
            [AttnCase(f, ATTN_BASE_LENS, 32, 8, 128) for f in ATTN_FAMILIES])


def attn_decode_footprint_cases() -> List[AttnCase]:
    """q with a row stride and NaN all around it, on a bf16 and a scaled fp8 cache."""
    return [AttnCase("tile", ATTN_BASE_LENS, 8, 2, 128, 16, None, kv8, kv8, q_pad=64) for kv8 in (False, True)]


def attn_prefill_case(f, g, d, bs=16, kv8=False, sc=False, q_pad=0, seqs=ATTN_PREFILL_SEQS, nkv=2):
    return AttnCase(f, tuple(a + p for a, p in seqs), nkv * g, nkv, d, bs, tuple(a for a, _ in seqs),
                    kv8, sc, q_pad)


def attn_prefill_base_cases() -> List[AttnCase]:
    return [attn_prefill_case(f, g, d) for d, g in attn_instantiated("prefill") for f in ATTN_FAMILIES]


def attn_prefill_path_cases() -> List[AttnCase]:
    """Cases every prefill path (unsplit, split-KV, invariant) runs: every cache kind at
    block sizes 16 and 32, q read with a row stride out of a fused-QKV-shaped buffer."""
    return [attn_prefill_case(f, 4, 128, bs, kv8, sc, q_pad=2 * 2 * 128)
            for f in ATTN_FAMILIES for _, kv8, sc in ATTN_KINDS for bs in (16, 32)]


def attn_all_cases() -> List[AttnCase]:
    """Every case of the tables, once (the bf16 path cases are base cases too)."""
    every = (attn_decode_base_cases() + attn_decode_path_cases() + attn_decode_special_cases() +
             attn_decode_footprint_cases() + attn_prefill_base_cases() + attn_prefill_path_cases())
    return list(dict.fromkeys(every))


# ---- fp32 model of the kernels' arithmetic ------------------------------------------------

def attn_model(o: AttnOperands, tile: int, span: int, thr: float = 8.0, per_row: bool = False) -> torch.Tensor:
    """bf16 [T, nq d]: the kernels' arithmetic in fp32 -- tiles of ``tile`` keys, a running
    state per range of ``span`` tiles with the deferred rescale (threshold ``thr``, decided
    by a ballot over the G heads of a decode row / 16 rows of a prefill block, or per row),
    p = exp2(fma(s, scale_log2, -m scale_log2)) in fp32, P rounded to bf16 for PV, fp32
    O and l, then the online merge of the ranges' partials.  Keeps the tolerance of the
    GPU tests honest: it must stay within one bf16 step of :func:`attn_reference`."""
    c = o.case
    g, d, nkv = c.g, c.d, c.nkv
    f32 = torch.float32
    sl2 = torch.tensor(ATTN_SCALE, dtype=f32) * torch.tensor(1.4426950408889634, dtype=f32)
    _, info = attn_reference(o, return_scores=True)
    out = torch.zeros(int(o.q_start_loc[-1]), nkv, g, d, dtype=f32)
    step = tile * span
    for (b, h), (s, vis, pos) in info.items():
        q0, q1 = int(o.q_start_loc[b]), int(o.q_start_loc[b + 1])
        ksv = float(o.k_scale[h]) if o.k_scale is not None else 1.0
        vsv = float(o.v_scale[h]) if o.v_scale is not None else 1.0
        scale = (sl2 * ksv).to(f32)
        thr_raw = (torch.tensor(thr, dtype=f32) / scale).to(f32)
        bs = c.block_size
        blk, off = o.block_tables[b, pos // bs].long(), pos % bs
        vrow = o.v_cache[blk, h, :, off].float()                 # stored units
        chan, val = vrow.argmax(-1), vrow.amax(-1)
        rows, n = s.shape[0], s.shape[2]
        raw = (s / ksv).masked_fill(~vis[:, None, :], float("-inf")).reshape(rows * g, n).to(f32)
        npad = -(-n // step) * step
        raw = torch.nn.functional.pad(raw, (0, npad - n), value=float("-inf"))
        chan = torch.nn.functional.pad(chan, (0, npad - n)).view(-1, span, tile)
        val = torch.nn.functional.pad(val, (0, npad - n)).view(-1, span, tile)
        nr, N = npad // step, rows * g
        raw = raw.view(N, nr, span, tile)
        m_run = torch.full((N, nr), float("-inf"), dtype=f32)
        l_run = torch.zeros(N, nr, dtype=f32)
        acc = torch.zeros(N, nr, d, dtype=f32)
        nbias = torch.zeros(N, nr, dtype=f32)
        for t in range(span):
            st = raw[:, :, t]                                     # [N, nr, tile]
            tm = st.amax(-1)
            up = tm > m_run + thr_raw
            if not per_row:
                if c.q_lens is None:
                    up = up.view(rows, g, nr).any(1, keepdim=True).expand(rows, g, nr).reshape(N, nr)
                else:
                    pad = -N % 16
                    u = torch.nn.functional.pad(up, (0, 0, 0, pad)).view(-1, 16, nr)
                    up = u.any(1, keepdim=True).expand(-1, 16, nr).reshape(-1, nr)[:N]
            mn = torch.maximum(m_run, tm)
            alpha = torch.exp2(((m_run - mn) * scale).to(f32))
            alpha = torch.where(torch.isnan(alpha), torch.ones_like(alpha), alpha)   # -inf - -inf: nothing to scale
            alpha = torch.where(up, alpha, torch.ones_like(alpha))
            m_run = torch.where(up, mn, m_run)
            nb_new = torch.where(torch.isinf(m_run), torch.zeros_like(m_run), -m_run * scale)
            nbias = torch.where(up, nb_new, nbias)
            l_run, acc = l_run * alpha, acc * alpha[..., None]
            arg = (st.double() * scale.double() + nbias.double()[..., None]).to(f32)   # one rounding: fma
            p = torch.exp2(arg)
            l_run = l_run + p.sum(-1)
            pv = p.to(torch.bfloat16).float() * val[:, t][None]
            acc.scatter_add_(2, chan[:, t][None].expand(N, nr, tile), pv)
        mp = torch.where(torch.isinf(m_run), m_run, m_run * scale)
        big = torch.full((N,), float("-inf"), dtype=f32)
        den = torch.zeros(N, dtype=f32)
        num = torch.zeros(N, d, dtype=f32)
        for k in range(nr):
            live = ~torch.isinf(mp[:, k])
            mn = torch.maximum(big, mp[:, k])
            a = torch.nan_to_num(torch.exp2(big - mn))
            e = torch.where(live, torch.exp2(mp[:, k] - mn), torch.zeros_like(mn))
            den = den * a + e * l_run[:, k]
            num = num * a[:, None] + e[:, None] * acc[:, k]
            big = mn
        inv = (1.0 / den * vsv).to(f32)
        out[q0:q1, h] = (num * inv[:, None]).view(rows, g, d)
    return out.view(-1, c.nq * d).to(torch.bfloat16)


# ---- comparison -----------------------------------------------------------------------------------

def explain_attn(o: AttnOperands, got: torch.Tensor, ref: torch.Tensor) -> str:
    """Names the first element more than one step off: sequence, query row, kv head, head,
    dim, and the keys / tiles of that element's channel with the weight it carries."""
    c = o.case
    g, d = c.g, c.d
    got, ref = got.cpu(), ref.cpu()
    dist = bf16_ulp_diff(got.contiguous(), ref.contiguous())
    bad = (dist > 1) | ((ref == 0) & (got != 0))
    if not bool(bad.any()):
        return "ok"
    # the element farthest off: the channel of the fault itself, not one that only felt l move
    dist = torch.where((ref == 0) & (got != 0), torch.full_like(dist, 1 << 17), dist)
    t, col = divmod(int(dist.argmax()), dist.shape[1])
    qsl = o.q_start_loc.cpu().tolist()
    b = max(i for i in range(len(c.lens)) if qsl[i] <= t)
    row, head, dim = t - qsl[b], col // d, col % d
    h, r = head // g, head % g
    L = int(o.seq_lens[b])
    lim = L if c.q_lens is None else L - (qsl[b + 1] - qsl[b]) + row + 1
    j = torch.arange(lim)
    if c.family == "key":
        cls, kd = attn_key_channel(j, h, g, d)
        mine = j[(cls == r) & (kd == dim)].tolist()
        units = f"keys {mine}" if mine else "no key of this head's class (other classes' keys only)"
    else:
        tl = torch.arange(-(-lim // 16))
        units = f"tiles {tl[attn_tile_channel(tl, h, d) == dim].tolist()}"
    gv, rv = float(got[t, col]), float(ref[t, col])
    ratio = f"{gv / rv:.4g}x its weight" if rv != 0 else "a weight where none is due"
    return (f"{int(bad.sum())} elements wrong; worst: sequence {b} (L = {L}), query row {row} (sees "
            f"positions < {lim}), kv head {h}, head {r}, dim {dim}: got {gv:.6g}, reference {rv:.6g}: "
            f"{units} of sequence {b} carry {ratio}")


def assert_attn(o: AttnOperands, got: torch.Tensor, ref: torch.Tensor, what: str) -> float:
    """Exact zeros of the reference are exactly zero and every element lies within one bf16
    step (:func:`assert_ulp1`: prints the share one step off and returns it); a failure
    names the sequence, heads, dim and the keys or tiles of the channel."""
    got, ref = got.cpu().contiguous(), ref.cpu().contiguous()
    zeros_ok = bool((got[ref == 0] == 0).all())
    try:
        share = assert_ulp1(got, ref, what)
    except AssertionError as e:
        raise AssertionError(f"{e}\n{what}: {explain_attn(o, got, ref)}") from None
    assert zeros_ok, f"{what}: {explain_attn(o, got, ref)}"
    return share

