"""W4A16 weight quantization (E9 / K14): AWQ-format int4, group 128, with zero points.

Replaces vLLM's ``--quantization awq`` (``docker-compose.vllm.yml:45-46``), which the
reference's default model needs (``hugging-quants/Meta-Llama-3.1-8B-Instruct-AWQ-INT4``,
``app/utils/config.py:93-96``).

* :func:`quantize_w4`: round-to-nearest asymmetric int4 per (row, 128-group), for
  random-init weights (and any bf16 checkpoint, ``ENGINE_QUANTIZATION=w4``).
* :func:`awq_unpack` / :func:`awq_pack`: the AutoAWQ "GEMM" checkpoint layout
  (``qweight`` [K, N/8] int32, ``qzeros`` [K/G, N/8] int32, ``scales`` [K/G, N] fp16,
  nibble i of a packed word = column 8c + (0, 2, 4, 6, 1, 3, 5, 7)[i]).  No AWQ
  checkpoint is available offline, so parity with a real one is unpinned; the
  round trip is tested against :func:`awq_pack`.
* :func:`pack_w4`: (q, z, s) -> the MFMA-fragment image ``w4a16.hip`` streams.
* :class:`W4Weight` holds one packed projection; :func:`w4_gemm` / :func:`w4_dequant`
  dispatch to the HIP kernels, or to a dequantize + matmul reference on the CPU.

W8A16 (fp8 e4m3 weights, one fp32 scale per output channel; vLLM's
``--quantization fp8``) follows below with the same shape of API:
:func:`quantize_w8` / :func:`dequantize_w8`, :func:`pack_w8` / :func:`unpack_w8`,
:class:`W8Weight`, :func:`w8_gemm` (M <= 64) and :func:`w8_packed_gemm` (any M).

MXFP4 (OCP MX e2m1 weights, one e8m0 scale per 32 k-values; AMD Quark MXFP4 exports)
is the third: :func:`quantize_mx4` / :func:`dequantize_mx4`, :func:`pack_mx4` /
:func:`unpack_mx4`, :func:`mx4_from_packed`, :class:`MX4Weight`, :func:`mx4_gemm`
(M <= 64) and :func:`mx4_packed_gemm` (any M).
"""
from __future__ import annotations

import dataclasses
from typing import Optional, Tuple

import torch

GROUP = 128
AWQ_ORDER = (0, 2, 4, 6, 1, 3, 5, 7)   # nibble i of an AWQ word holds column AWQ_ORDER[i]
_NIBBLE_K = (0, 2, 4, 6, 1, 3, 5, 7)   # nibble p of one of our words holds k offset _NIBBLE_K[p]


@dataclasses.dataclass
class W4Weight:
    wq: torch.Tensor   # int32 [N/16 * K/128 * 64 * 4]  packed nibbles
    sz: torch.Tensor   # fp32 [N/16, K/128, 16, 2]      (scale, 128 + zero)
    n: int
    k: int

    @property
    def shape(self) -> Tuple[int, int]:
        return (self.n, self.k)

    def nbytes(self) -> int:
        return self.wq.numel() * 4 + self.sz.numel() * 4


def quantize_w4(w: torch.Tensor, group: int = GROUP):
    """[N, K] float -> (q uint8 [N, K], z uint8 [N, K/g], s fp32 [N, K/g]) with
    w ~= (q - z) * s (round to nearest, asymmetric per row and group)."""
    n, k = w.shape
    assert k % group == 0
    # fp64: correctly rounded on every backend, so a GPU and a CPU quantization of
    # the same weights agree bit for bit
    wf = w.double().view(n, k // group, group)
    mn = wf.amin(-1).clamp(max=0.0)
    mx = wf.amax(-1).clamp(min=0.0)
    s = ((mx - mn) / 15.0).clamp(min=1e-8).float().double()
    z = torch.round(-mn / s).clamp(0, 15)
    q = (torch.round(wf / s.unsqueeze(-1)) + z.unsqueeze(-1)).clamp(0, 15)
    return q.view(n, k).to(torch.uint8), z.to(torch.uint8), s.float()


def dequantize_w4(q: torch.Tensor, z: torch.Tensor, s: torch.Tensor, group: int = GROUP):
    n, k = q.shape
    w = (q.float().view(n, k // group, group) - z.float().unsqueeze(-1)) * s.float().unsqueeze(-1)
    return w.view(n, k)


def _to_i32(v: torch.Tensor) -> torch.Tensor:
    """int64 holding uint32 bit patterns -> int32 with the same bits."""
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)


def _nibbles(words: torch.Tensor) -> torch.Tensor:
    """int32 [...] -> int64 [..., 8] nibbles (nibble i = bits 4i..4i+3)."""
    w = words.to(torch.int64) & 0xFFFFFFFF
    shifts = torch.arange(0, 32, 4, device=words.device)
    return (w.unsqueeze(-1) >> shifts) & 15


def _pack_nibbles(nib: torch.Tensor) -> torch.Tensor:
    """int [..., 8] (values 0..15, nibble i at bits 4i) -> int32 [...]."""
    shifts = torch.arange(0, 32, 4, device=nib.device)
    return _to_i32((nib.to(torch.int64) << shifts).sum(-1))


def pack_w4(q: torch.Tensor, z: torch.Tensor, s: torch.Tensor) -> W4Weight:
    """(q, z, s) -> the kernel image.  wq[tile][grp][lane][word], lane = g*16 + r,
    word = 2*step + half, nibble p = k offset 128 grp + 64 step + 16 g + 8 half +
    _NIBBLE_K[p] of column 16 tile + r."""
    n, k = q.shape
    assert n % 16 == 0 and k % GROUP == 0, "W4 needs N % 16 == 0 and K % 128 == 0"
    dev = q.device
    # (tile, r, grp, step, g, half, e) -> (tile, grp, g, r, step, half, e)
    t = q.to(torch.int64).view(n // 16, 16, k // 128, 2, 4, 2, 8).permute(0, 2, 4, 1, 3, 5, 6)
    t = t[..., list(_NIBBLE_K)]
    wq = _pack_nibbles(t).contiguous().view(-1)
    sz = torch.stack([s.float(), z.float() + 128.0], -1)          # [N, G, 2]
    sz = sz.view(n // 16, 16, k // 128, 2).permute(0, 2, 1, 3).contiguous()
    return W4Weight(wq.to(dev), sz.to(dev), n, k)


def unpack_w4(w: W4Weight):
    """Inverse of :func:`pack_w4` (tests, checkpoint export)."""
    n, k = w.n, w.k
    nib = _nibbles(w.wq.view(n // 16, k // 128, 4, 16, 2, 2))      # (tile, grp, g, r, step, half, p)
    inv = [0] * 8
    for p, off in enumerate(_NIBBLE_K):
        inv[off] = p
    nib = nib[..., inv]                                             # e order
    q = nib.permute(0, 3, 1, 4, 2, 5, 6).contiguous().view(n, k).to(torch.uint8)
    sz = w.sz.view(n // 16, k // 128, 16, 2).permute(0, 2, 1, 3).reshape(n, k // 128, 2)
    return q, (sz[..., 1] - 128.0).round().to(torch.uint8), sz[..., 0].contiguous()


# ------------------------------------------------------------------ AutoAWQ layout
def awq_unpack(qweight: torch.Tensor, qzeros: torch.Tensor, scales: torch.Tensor):
    """AutoAWQ GEMM tensors of one linear (in K, out N) -> (q [N, K], z [N, G], s [N, G])."""
    kk, n8 = qweight.shape
    inv = [0] * 8
    for i, col in enumerate(AWQ_ORDER):
        inv[col] = i
    q = _nibbles(qweight)[..., inv].reshape(kk, n8 * 8)            # [K, N]
    z = _nibbles(qzeros)[..., inv].reshape(qzeros.shape[0], n8 * 8)  # [G, N]
    return (q.t().contiguous().to(torch.uint8), z.t().contiguous().to(torch.uint8),
            scales.float().t().contiguous())


def awq_pack(q: torch.Tensor, z: torch.Tensor, s: torch.Tensor):
    """(q [N, K], z [N, G], s [N, G]) -> AutoAWQ (qweight, qzeros, scales fp16)."""
    n, k = q.shape
    qk = q.t().to(torch.int64).reshape(k, n // 8, 8)[..., list(AWQ_ORDER)]
    zg = z.t().to(torch.int64).reshape(z.shape[1], n // 8, 8)[..., list(AWQ_ORDER)]
    return _pack_nibbles(qk), _pack_nibbles(zg), s.t().contiguous().to(torch.float16)


# ------------------------------------------------------------------ compute
def w4_dequant(w: W4Weight, out: Optional[torch.Tensor] = None,
               dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    if w.wq.is_cuda:
        from . import native

        if out is None:
            out = torch.empty(w.n, w.k, dtype=torch.bfloat16, device=w.wq.device)
        native().w4_dequant(w.wq, w.sz, out)
        return out
    q, z, s = unpack_w4(w)
    r = dequantize_w4(q, z, s).to(dtype)
    if out is not None:
        out.copy_(r)
        return out
    return r


def w4_gemm(x: torch.Tensor, w: W4Weight, out=None, ws=None, splits: int = 1, nt: int = 1,
            xr: int = 0, silu: bool = False):
    """y = x dequant(w)^T for M <= 64 rows.  With ``ws`` the kernel leaves fp32
    slabs ([splits, M, N]) for a fused epilogue; otherwise returns bf16 ``out``.
    ``xr`` picks the kernel (w4a16.hip): 0 the register kernel, 1 "xr" (x chunks in
    LDS, 17..64 rows), 4 / 5 "mh" (two tiles per wave, rows over wave pairs; weight
    ring 2 with two x chunks in flight / ring 3).  ``silu``: the LDS kernels' SiLU
    epilogue on a gate/up image interleaved in 16-row groups (h = silu(gate) * up)."""
    if not x.is_cuda:
        y = x @ w4_dequant(w, dtype=x.dtype).t()
        if silu:
            g, u = y.view(y.shape[0], -1, 2, 16).unbind(2)
            y = (torch.nn.functional.silu(g.float()) * u.float()).to(x.dtype).reshape(y.shape[0], -1)
        return y
    from . import native

    if ws is None and out is None:
        out = torch.empty(x.shape[0], w.n // 2 if silu else w.n, dtype=x.dtype, device=x.device)
    native().w4_gemm(x, w.wq, w.sz, w.n, out, ws, splits, nt, int(xr), silu)
    return out if ws is None else ws


_W4PG_EPI = {"store": 0, "slab": 1, "silu": 2}


def w4_packed_gemm(x: torch.Tensor, w: W4Weight, out=None, ws=None, splits: int = 1,
                   epi: str = "store", cfg: int = 0):
    """y = x dequant(w)^T for any row count on the int4 image
    (csrc/kernels/w4_packed_gemm.hip), with the decode kernels' numerics: exact
    (q - z) * s weights, fp32 accumulation.  epi "store": bf16 [M, N]; "slab": fp32
    slabs [splits, M, N] in ``ws`` (any split count); "silu": silu(gate) * up of an
    image interleaved in 16-row groups -> [M, N / 2].  cfg: 0 = 128 x 256 tile,
    1 = 256 x 128, 2 = 128 x 128.  Returns ``ws`` for slabs, else ``out``."""
    code = _W4PG_EPI[epi]
    if splits < 1 or w.k % (GROUP * splits):
        raise ValueError(f"w4_packed_gemm: K {w.k} is not a multiple of 128 * splits ({splits})")
    if code != 1 and splits != 1:
        raise ValueError("w4_packed_gemm: splits > 1 leaves slabs (epi='slab')")
    if code == 2 and w.n % 32:
        raise ValueError(f"w4_packed_gemm: the SiLU epilogue needs N % 32 == 0 (N = {w.n})")
    if code == 1 and ws is None:
        raise ValueError("w4_packed_gemm: slabs need a workspace")
    if not x.is_cuda:
        m = x.shape[0]
        y = x.float() @ w4_dequant(w, dtype=torch.float32).t()
        if code == 1:   # the whole product in slab 0
            slabs = ws.view(-1)[:splits * m * w.n].view(splits, m, w.n)
            slabs.zero_()
            slabs[0].copy_(y)
            return ws
        if code == 2:
            g, u = y.view(m, -1, 2, 16).unbind(2)
            y = (torch.nn.functional.silu(g) * u).reshape(m, -1)
        y = y.to(x.dtype)
        if out is not None:
            out[:m, :y.shape[1]].copy_(y)
            return out
        return y
    from . import native

    if code != 1 and out is None:
        out = torch.empty(x.shape[0], w.n // 2 if code == 2 else w.n, dtype=x.dtype, device=x.device)
    native().w4_packed_gemm(x, w.wq, w.sz, w.n, out, ws, splits, code, cfg)
    return ws if code == 1 else out


# ==================================================================================
# W8A16: fp8 e4m3 (OCP, torch.float8_e4m3fn) weights, one fp32 scale per output channel
# ==================================================================================
# The numerics every kernel, CPU fallback and test uses:
#   y[m, n] = s[n] * sum_k x[m, k] * q[n, k]
# q widened to bf16 (every e4m3 value is exact in bf16), products on the bf16 MFMA with
# fp32 accumulation, the scale applied once to the fp32 accumulator (to each slab under
# split-K), then one rounding to bf16 (or SiLU * up in fp32, then one rounding).  No
# per-weight multiply, no bf16-rounded q * s.
FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0
W8_KSTEP = 64          # k-values per image block: two 16x16x32 MFMAs


@dataclasses.dataclass
class W8Weight:
    wq: torch.Tensor      # uint8 [N/16 * K/64 * 64 * 16]  fp8 bytes in fragment order
    scale: torch.Tensor   # fp32 [N]  (image row order)
    n: int
    k: int

    @property
    def shape(self) -> Tuple[int, int]:
        return (self.n, self.k)

    def nbytes(self) -> int:
        return self.wq.numel() + self.scale.numel() * 4


def fp8_nan_bytes(q: torch.Tensor) -> torch.Tensor:
    """bool mask of the e4m3 NaN encodings (0x7F, 0xFF) in an fp8 / uint8 tensor."""
    return (q.view(torch.uint8) & 0x7F) == 0x7F


def quantize_w8(w: torch.Tensor):
    """[N, K] float -> (q float8_e4m3fn [N, K], s fp32 [N]) with w ~= q * s[:, None]:
    round to nearest, s = absmax / 448 per row (1 for an all-zero row)."""
    # fp64: correctly rounded on every backend, so a GPU and a CPU quantization of
    # the same weights agree bit for bit (as quantize_w4)
    wd = w.double()
    amax = wd.abs().amax(-1)
    s = (amax / FP8_MAX).float()
    s = torch.where(s > 0, s, torch.ones_like(s))
    # clamp BEFORE the cast: an out-of-range value becomes NaN, not the maximum
    q = (wd / s.double().unsqueeze(-1)).clamp(-FP8_MAX, FP8_MAX).to(FP8)
    return q, s


def dequantize_w8(q: torch.Tensor, s: torch.Tensor, dtype: torch.dtype = torch.float32):
    """q * s[:, None]; exact in fp64, one rounding in any other dtype."""
    if dtype == torch.float64:
        return q.double() * s.double().unsqueeze(-1)
    return (q.float() * s.float().unsqueeze(-1)).to(dtype)


def _interleave16(t: torch.Tensor) -> torch.Tensor:
    """Gate rows then up rows -> 16 gate rows, their 16 up rows, ... (ops.interleave_gate_up
    with nh = 1) along dim 0 of a [2I, ...] tensor."""
    two_i = t.shape[0]
    inter = two_i // 2
    assert inter % 16 == 0, "the gate_up interleave needs inter % 16 == 0"
    g = t[:inter].reshape(inter // 16, 16, *t.shape[1:])
    u = t[inter:].reshape(inter // 16, 16, *t.shape[1:])
    return torch.stack([g, u], dim=1).reshape(t.shape)


def _deinterleave16(t: torch.Tensor) -> torch.Tensor:
    two_i = t.shape[0]
    v = t.reshape(two_i // 32, 2, 16, *t.shape[1:])
    return torch.cat([v[:, 0].reshape(two_i // 2, *t.shape[1:]),
                      v[:, 1].reshape(two_i // 2, *t.shape[1:])], 0)


def pack_w8(q: torch.Tensor, s: torch.Tensor, gate_up: bool = False) -> W8Weight:
    """(q, s) -> the kernel image.  wq[tile][step][lane][16], lane = g * 16 + r: byte
    8 * half + e of a lane's 16 is k = 64 step + 16 g + 8 half + e of column 16 tile + r,
    so one 16-byte load per lane holds the 16 k-values the lane feeds to the two
    v_mfma_f32_16x16x32_bf16 (half 0, half 1) of a 64-wide k-step, a wave instruction
    reads the 1 KiB block of one (tile, step), and a column tile's blocks follow each
    other along K.  ``scale`` is s in image row order.  ``gate_up``: rows (gate then up)
    and their scales are first interleaved in 16-row groups (ops.interleave_gate_up(w, 1)),
    the order the SiLU epilogues and slab_silu(interleaved=True) expect."""
    n, k = q.shape
    if n % 16 or k % W8_KSTEP:
        raise ValueError(f"W8 needs N % 16 == 0 and K % 64 == 0 (N = {n}, K = {k})")
    if q.dtype != FP8:
        raise ValueError(f"pack_w8: q must be float8_e4m3fn, not {q.dtype}")
    if gate_up and n % 32:
        raise ValueError(f"pack_w8: a gate_up image needs N % 32 == 0 (N = {n})")
    b = q.view(torch.uint8)
    s = s.float().reshape(n)
    if gate_up:
        b, s = _interleave16(b), _interleave16(s)
    # (tile, r, step, g, byte) -> (tile, step, g, r, byte)
    wq = b.reshape(n // 16, 16, k // 64, 4, 16).permute(0, 2, 3, 1, 4).contiguous().view(-1)
    return W8Weight(wq, s.contiguous(), n, k)


def unpack_w8(w: W8Weight, gate_up: bool = False):
    """Inverse of :func:`pack_w8` (tests, checkpoint export): (q float8_e4m3fn [N, K], s)."""
    n, k = w.n, w.k
    b = w.wq.view(n // 16, k // 64, 4, 16, 16).permute(0, 3, 1, 2, 4).contiguous().view(n, k)
    s = w.scale
    if gate_up:
        b, s = _deinterleave16(b), _deinterleave16(s)
    return b.contiguous().view(FP8), s.contiguous()


W8_NTS = (1, 2, 4)     # column tiles per wave the decode kernel is built for


def _w8_ref(x: torch.Tensor, w: W8Weight) -> torch.Tensor:
    """The contract in fp32 on the CPU: s[n] * sum_k x q, image row order."""
    q, s = unpack_w8(w)
    return (x.float() @ q.float().t()) * s.float()


def w8_gemm(x: torch.Tensor, w: W8Weight, out=None, ws=None, splits: int = 1, nt: int = 2,
            silu: bool = False):
    """y = s * (x q^T) for M <= 64 rows (csrc/kernels/w8a16.hip).  With ``ws`` the kernel
    leaves fp32 slabs ([splits, M, N], each already scaled) for a fused epilogue and
    returns ``ws``; otherwise it returns bf16 ``out``.  ``nt``: 16-column tiles per wave
    (1, 2, 4).  ``silu``: h = silu(gate) * up of a ``pack_w8(..., gate_up=True)`` image,
    [M, N / 2] (nt 2, one split, no workspace)."""
    m = x.shape[0]
    if m > 64:
        raise ValueError(f"w8_gemm: M = {m} > 64 (use w8_packed_gemm)")
    if nt not in W8_NTS:
        raise ValueError(f"w8_gemm: nt {nt} not in {W8_NTS}")
    if splits < 1 or w.k % (256 * splits):
        raise ValueError(f"w8_gemm: K {w.k} is not a multiple of 256 * splits ({splits})")
    if silu and (ws is not None or splits != 1 or nt != 2 or w.n % 32):
        raise ValueError("w8_gemm: the SiLU epilogue is nt 2, one split, bf16 out, N % 32 == 0")
    if splits > 1 and ws is None:
        raise ValueError("w8_gemm: splits > 1 needs a workspace")
    if ws is not None and ws.numel() < splits * m * w.n:
        raise ValueError(f"w8_gemm: workspace too small ({ws.numel()} < {splits * m * w.n})")
    if not x.is_cuda:
        y = _w8_ref(x, w)
        if ws is not None:   # the whole product in slab 0
            slabs = ws.view(-1)[:splits * m * w.n].view(splits, m, w.n)
            slabs.zero_()
            slabs[0].copy_(y)
            return ws
        if silu:
            g, u = y.view(m, -1, 2, 16).unbind(2)
            y = (torch.nn.functional.silu(g) * u).reshape(m, -1)
        y = y.to(x.dtype)
        if out is not None:
            out[:m, :y.shape[1]].copy_(y)
            return out
        return y
    from . import native

    if ws is None and out is None:
        out = torch.empty(m, w.n // 2 if silu else w.n, dtype=x.dtype, device=x.device)
    native().w8_gemm(x, w.wq, w.scale, w.n, out, ws, splits, nt, silu)
    return out if ws is None else ws


def w8_packed_gemm(x: torch.Tensor, w: W8Weight, out=None, ws=None, splits: int = 1,
                   epi: str = "store", cfg: int = 0):
    """y = s * (x q^T) for any row count on the fp8 image
    (csrc/kernels/w8_packed_gemm.hip), with the decode kernel's numerics.  epi "store":
    bf16 [M, N]; "slab": fp32 slabs [splits, M, N] in ``ws`` (any split count, each
    scaled); "silu": silu(gate) * up of a gate_up image -> [M, N / 2].  cfg 0 = the
    128 x 256 tile.  Returns ``ws`` for slabs, else ``out``."""
    code = _W4PG_EPI[epi]
    m = x.shape[0]
    if cfg != 0:
        raise ValueError(f"w8_packed_gemm: unknown tile shape cfg {cfg}")
    if splits < 1 or w.k % (W8_KSTEP * splits):
        raise ValueError(f"w8_packed_gemm: K {w.k} is not a multiple of 64 * splits ({splits})")
    if code != 1 and splits != 1:
        raise ValueError("w8_packed_gemm: splits > 1 leaves slabs (epi='slab')")
    if code == 2 and w.n % 32:
        raise ValueError(f"w8_packed_gemm: the SiLU epilogue needs N % 32 == 0 (N = {w.n})")
    if code == 1 and ws is None:
        raise ValueError("w8_packed_gemm: slabs need a workspace")
    if code == 1 and ws.numel() < splits * m * w.n:
        raise ValueError(f"w8_packed_gemm: workspace too small ({ws.numel()} < {splits * m * w.n})")
    if not x.is_cuda:
        y = _w8_ref(x, w)
        if code == 1:   # the whole product in slab 0
            slabs = ws.view(-1)[:splits * m * w.n].view(splits, m, w.n)
            slabs.zero_()
            slabs[0].copy_(y)
            return ws
        if code == 2:
            g, u = y.view(m, -1, 2, 16).unbind(2)
            y = (torch.nn.functional.silu(g) * u).reshape(m, -1)
        y = y.to(x.dtype)
        if out is not None:
            out[:m, :y.shape[1]].copy_(y)
            return out
        return y
    from . import native

    if code != 1 and out is None:
        out = torch.empty(m, w.n // 2 if code == 2 else w.n, dtype=x.dtype, device=x.device)
    native().w8_packed_gemm(x, w.wq, w.scale, w.n, out, ws, splits, code, cfg)
    return ws if code == 1 else out


# ==================================================================================
# MXFP4 (W4A16): OCP MX e2m1 weights, one e8m0 (power-of-two) scale per 32 k-values
# ==================================================================================
# The numerics every kernel, CPU fallback and test uses:
#   y[m, n] = sum_k x[m, k] * fp4(code[n, k]) * 2^(sb[n, k // 32] - 127)
# A code is 4 bits: sign in bit 3, magnitude MX4_GRID[code & 7].  With a scale byte in
# [MX4_SB_MIN, MX4_SB_MAX] every product fp4 * 2^e is a finite NORMAL bf16 (0.5 * 2^-125
# = 2^-126 is the smallest normal, 6 * 2^125 is finite), so the kernels widen and scale
# in registers (v_cvt_scalef32_pk_bf16_fp4) and run a plain bf16 MFMA GEMM into fp32 on
# the dequantized weights: no epilogue scale.  Bytes outside the range are refused
# (0.5 * 2^(b - 127) goes denormal below, 6 * 2^(b - 127) overflows above, 255 is NaN).
MX4_BLOCK = 32         # k-values per scale
MX4_KSTEP = 128        # k-values per image block: four 16x16x32 MFMAs, 4 MX blocks
MX4_SB_MIN, MX4_SB_MAX = 2, 252
MX4_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
MX4_NTS = (1, 2, 4)    # column tiles per wave the decode kernel is built for


@dataclasses.dataclass
class MX4Weight:
    wq: torch.Tensor      # uint8 [N/16 * K/128 * 64 * 16]  e2m1 nibbles in fragment order
    sc: torch.Tensor      # uint8 [N/16 * K/128 * 64]       the lanes' e8m0 scale bytes
    n: int
    k: int

    @property
    def shape(self) -> Tuple[int, int]:
        return (self.n, self.k)

    def nbytes(self) -> int:
        return self.wq.numel() + self.sc.numel()


def mx4_check_scale_bytes(sb: torch.Tensor, name: str = "scale bytes") -> None:
    """ValueError (naming ``name``) unless every e8m0 byte lies in [2, 252]."""
    b = sb.view(torch.uint8)
    bad = (b < MX4_SB_MIN) | (b > MX4_SB_MAX)
    if bool(bad.any()):
        v = int(b[bad].flatten()[0])
        raise ValueError(f"{name}: e8m0 scale byte {v} outside [{MX4_SB_MIN}, {MX4_SB_MAX}] "
                         f"({int(bad.sum())} such bytes; fp4 * 2^(b - 127) would leave the normal "
                         "bf16 range, 255 is NaN)")


def quantize_mx4(w: torch.Tensor):
    """[N, K] float (K % 32 == 0) -> (codes uint8 [N, K] in 0..15, sb uint8 [N, K/32]).
    Per 32-block the OCP MX rule: exponent floor(log2(absmax)) - 2, byte = exponent + 127
    clamped to [2, 252] (127 for an all-zero block); w / 2^e clamped to +-6 and rounded to
    the nearest e2m1 value, ties to the even code.  NaN / Inf raise."""
    if w.dim() != 2 or w.shape[1] % MX4_BLOCK:
        raise ValueError(f"quantize_mx4: needs [N, K] with K % 32 == 0, got {tuple(w.shape)}")
    # fp64: exact on every backend, so a GPU and a CPU quantization agree bit for bit
    wd = w.double()
    if not bool(torch.isfinite(wd).all()):
        raise ValueError("quantize_mx4: the weight holds NaN or Inf")
    n, k = wd.shape
    blk = wd.view(n, k // MX4_BLOCK, MX4_BLOCK)
    amax = blk.abs().amax(-1)
    _, ex = torch.frexp(amax)                    # amax = m 2^ex, m in [0.5, 1)
    e = ex.to(torch.int64) - 1 - 2               # floor(log2(amax)) - 2
    sb = torch.where(amax > 0, (e + 127).clamp(MX4_SB_MIN, MX4_SB_MAX), torch.full_like(e, 127))
    scale = torch.ldexp(torch.ones_like(amax), (sb - 127).to(torch.int32))
    a = (blk / scale.unsqueeze(-1)).clamp(-6.0, 6.0)
    m = a.abs()
    # midpoints of the grid; a tie goes to the even code of its two neighbours
    mag = ((m > 0.25).to(torch.uint8) + (m >= 0.75).to(torch.uint8) + (m > 1.25).to(torch.uint8)
           + (m >= 1.75).to(torch.uint8) + (m > 2.5).to(torch.uint8) + (m >= 3.5).to(torch.uint8)
           + (m > 5.0).to(torch.uint8))
    sign = ((a < 0) & (mag > 0)).to(torch.uint8) << 3
    return (mag | sign).view(n, k).contiguous(), sb.to(torch.uint8).contiguous()


def dequantize_mx4(codes: torch.Tensor, sb: torch.Tensor, dtype: torch.dtype = torch.float32):
    """fp4(code) * 2^(sb - 127) per 32-block; exact in fp64, fp32 and (scale bytes in
    [2, 252]) bf16."""
    n, k = codes.shape
    lut = torch.tensor(MX4_GRID + tuple(-v for v in MX4_GRID), dtype=torch.float64, device=codes.device)
    v = lut[codes.long()].view(n, k // MX4_BLOCK, MX4_BLOCK)
    e = sb.view(torch.uint8).to(torch.int32) - 127
    s = torch.ldexp(torch.ones(e.shape, dtype=torch.float64, device=codes.device), e)
    return (v * s.unsqueeze(-1)).view(n, k).to(dtype)


def mx4_from_packed(wbytes: torch.Tensor, scales: torch.Tensor):
    """Checkpoint layout (wbytes [N, K/2] uint8 / float4_e2m1fn_x2: two codes per byte, the
    even k in the LOW nibble; scales [N, K/32] uint8 / float8_e8m0fnu) -> (codes, sb)."""
    b = wbytes.view(torch.uint8)
    codes = torch.stack([b & 0xF, b >> 4], dim=-1).reshape(b.shape[0], b.shape[1] * 2)
    return codes.contiguous(), scales.view(torch.uint8).contiguous()


def mx4_to_packed(codes: torch.Tensor, sb: torch.Tensor):
    """Inverse of :func:`mx4_from_packed`: (wbytes uint8 [N, K/2], scales uint8 [N, K/32])."""
    c = codes.view(codes.shape[0], -1, 2)
    return (c[..., 0] | (c[..., 1] << 4)).contiguous(), sb.contiguous()


def pack_mx4(codes: torch.Tensor, sb: torch.Tensor, gate_up: bool = False,
             name: str = "scale bytes") -> MX4Weight:
    """(codes, sb) -> the kernel image (csrc/kernels/mx4a16.hip documents it).
    wq[tile][step][lane][16 B], lane = g * 16 + r: column 16 tile + r, k = 128 step + 32 g
    + 0..31 (MX block 4 step + g, so ONE scale byte per 16-byte load); dword j holds k =
    128 step + 32 g + 8 j + e in nibble e, the low nibble of byte e / 2 first, and is the
    B fragment of the step's j-th 16x16x32 MFMA.  sc[tile][step][lane] is the lane's scale
    byte.  ``gate_up``: rows (gate then up) and their scale rows are first interleaved in
    16-row groups, the order the SiLU epilogues expect.  Scale bytes outside [2, 252]
    raise, naming ``name``."""
    n, k = codes.shape
    if n % 16 or k % MX4_KSTEP:
        raise ValueError(f"MX4 needs N % 16 == 0 and K % 128 == 0 (N = {n}, K = {k})")
    if codes.dtype != torch.uint8 or sb.dtype != torch.uint8:
        raise ValueError(f"pack_mx4: codes and scale bytes must be uint8, not {codes.dtype} / {sb.dtype}")
    if tuple(sb.shape) != (n, k // MX4_BLOCK):
        raise ValueError(f"pack_mx4: scale bytes {tuple(sb.shape)}, expected {(n, k // MX4_BLOCK)}")
    if bool((codes > 15).any()):
        raise ValueError("pack_mx4: codes must lie in 0..15")
    if gate_up and n % 32:
        raise ValueError(f"pack_mx4: a gate_up image needs N % 32 == 0 (N = {n})")
    mx4_check_scale_bytes(sb, name)
    if gate_up:
        codes, sb = _interleave16(codes), _interleave16(sb)
    b, _ = mx4_to_packed(codes, sb)              # [N, K/2], 64 bytes per k-step, 16 per g
    # (tile, r, step, g, byte) -> (tile, step, g, r, byte)
    wq = b.reshape(n // 16, 16, k // 128, 4, 16).permute(0, 2, 3, 1, 4).contiguous().view(-1)
    sc = sb.reshape(n // 16, 16, k // 128, 4).permute(0, 2, 3, 1).contiguous().view(-1)
    return MX4Weight(wq, sc, n, k)


def unpack_mx4(w: MX4Weight, gate_up: bool = False):
    """Inverse of :func:`pack_mx4`: (codes uint8 [N, K], sb uint8 [N, K/32])."""
    n, k = w.n, w.k
    b = w.wq.view(n // 16, k // 128, 4, 16, 16).permute(0, 3, 1, 2, 4).contiguous().view(n, k // 2)
    sb = w.sc.view(n // 16, k // 128, 4, 16).permute(0, 3, 1, 2).contiguous().view(n, k // 32)
    codes, sb = mx4_from_packed(b, sb)
    if gate_up:
        codes, sb = _deinterleave16(codes), _deinterleave16(sb)
    return codes.contiguous(), sb.contiguous()


def _mx4_ref(x: torch.Tensor, w: MX4Weight) -> torch.Tensor:
    """The contract in fp32 on the CPU: x dequant(W)^T, image row order."""
    return x.float() @ dequantize_mx4(*unpack_mx4(w)).t()


def _mx4_cpu_out(y: torch.Tensor, x, m: int, n: int, ws, splits: int, out, slab: bool, silu: bool):
    if slab:   # the whole product in slab 0
        slabs = ws.view(-1)[:splits * m * n].view(splits, m, n)
        slabs.zero_()
        slabs[0].copy_(y)
        return ws
    if silu:
        g, u = y.view(m, -1, 2, 16).unbind(2)
        y = (torch.nn.functional.silu(g) * u).reshape(m, -1)
    y = y.to(x.dtype)
    if out is not None:
        out[:m, :y.shape[1]].copy_(y)
        return out
    return y


def mx4_gemm(x: torch.Tensor, w: MX4Weight, out=None, ws=None, splits: int = 1, nt: int = 2,
             silu: bool = False):
    """y = x dequant(W)^T for M <= 64 rows (csrc/kernels/mx4a16.hip).  With ``ws`` the
    kernel leaves fp32 slabs ([splits, M, N]) for a fused epilogue and returns ``ws``;
    otherwise it returns bf16 ``out``.  ``nt``: 16-column tiles per wave (1, 2, 4).
    ``silu``: h = silu(gate) * up of a ``pack_mx4(..., gate_up=True)`` image, [M, N / 2]
    (nt 2, one split, no workspace)."""
    m = x.shape[0]
    if m > 64:
        raise ValueError(f"mx4_gemm: M = {m} > 64 (use mx4_packed_gemm)")
    if nt not in MX4_NTS:
        raise ValueError(f"mx4_gemm: nt {nt} not in {MX4_NTS}")
    if splits < 1 or w.k % (256 * splits):
        raise ValueError(f"mx4_gemm: K {w.k} is not a multiple of 256 * splits ({splits})")
    if silu and (ws is not None or splits != 1 or nt != 2 or w.n % 32):
        raise ValueError("mx4_gemm: the SiLU epilogue is nt 2, one split, bf16 out, N % 32 == 0")
    if splits > 1 and ws is None:
        raise ValueError("mx4_gemm: splits > 1 needs a workspace")
    if ws is not None and ws.numel() < splits * m * w.n:
        raise ValueError(f"mx4_gemm: workspace too small ({ws.numel()} < {splits * m * w.n})")
    if not x.is_cuda:
        return _mx4_cpu_out(_mx4_ref(x, w), x, m, w.n, ws, splits, out, ws is not None, silu)
    from . import native

    if ws is None and out is None:
        out = torch.empty(m, w.n // 2 if silu else w.n, dtype=x.dtype, device=x.device)
    native().mx4_gemm(x, w.wq, w.sc, w.n, out, ws, splits, nt, silu)
    return out if ws is None else ws


def mx4_packed_gemm(x: torch.Tensor, w: MX4Weight, out=None, ws=None, splits: int = 1,
                    epi: str = "store", cfg: int = 0):
    """y = x dequant(W)^T for any row count on the same image
    (csrc/kernels/mx4_packed_gemm.hip), with the decode kernel's numerics.  epi "store":
    bf16 [M, N]; "slab": fp32 slabs [splits, M, N] in ``ws`` (any split count); "silu":
    silu(gate) * up of a gate_up image -> [M, N / 2].  cfg 0 = the 128 x 256 tile.
    Returns ``ws`` for slabs, else ``out``."""
    code = _W4PG_EPI[epi]
    m = x.shape[0]
    if cfg != 0:
        raise ValueError(f"mx4_packed_gemm: unknown tile shape cfg {cfg}")
    if splits < 1 or w.k % (MX4_KSTEP * splits):
        raise ValueError(f"mx4_packed_gemm: K {w.k} is not a multiple of 128 * splits ({splits})")
    if code != 1 and splits != 1:
        raise ValueError("mx4_packed_gemm: splits > 1 leaves slabs (epi='slab')")
    if code == 2 and w.n % 32:
        raise ValueError(f"mx4_packed_gemm: the SiLU epilogue needs N % 32 == 0 (N = {w.n})")
    if code == 1 and ws is None:
        raise ValueError("mx4_packed_gemm: slabs need a workspace")
    if code == 1 and ws.numel() < splits * m * w.n:
        raise ValueError(f"mx4_packed_gemm: workspace too small ({ws.numel()} < {splits * m * w.n})")
    if not x.is_cuda:
        return _mx4_cpu_out(_mx4_ref(x, w), x, m, w.n, ws, splits, out, code == 1, code == 2)
    from . import native

    if code != 1 and out is None:
        out = torch.empty(m, w.n // 2 if code == 2 else w.n, dtype=x.dtype, device=x.device)
    native().mx4_packed_gemm(x, w.wq, w.sc, w.n, out, ws, splits, code, cfg)
    return ws if code == 1 else out
