"""Operands and comparisons for bit-exact GEMM tests (plain PyTorch, no native code).

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
