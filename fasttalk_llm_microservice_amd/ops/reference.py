"""Plain-PyTorch fp32 reference implementations of every native op.

They define the semantics the gfx950 kernels in ``csrc/kernels`` must match
(numerics tests compare the two), and they are the compute path of the CPU
backend (BASELINE config 1: a llama3.2-1b-shaped model streaming over /ws/llm
with no GPU).  All math is done in fp32 and rounded once to the storage dtype,
mirroring the kernels.
"""
from __future__ import annotations

import math
from typing import Optional

import torch


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    inv = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    n = (xf * inv).to(x.dtype)
    return (n.float() * w.float()).to(x.dtype)


def fused_add_rmsnorm(x: torch.Tensor, residual: torch.Tensor, w: torch.Tensor, eps: float):
    r = (x.float() + residual.float()).to(x.dtype)
    return rmsnorm(r, w, eps), r


def silu_mul(gu: torch.Tensor) -> torch.Tensor:
    inter = gu.shape[-1] // 2
    g = gu[..., :inter].float()
    u = gu[..., inter:].float()
    return (g * torch.sigmoid(g) * u).to(gu.dtype)


def rope_cos_sin(head_dim: int, max_pos: int, theta: float, scaling: Optional[dict] = None,
                 device=None) -> torch.Tensor:
    """fp32 [max_pos, head_dim] table = [cos | sin] of the rotate_half convention.

    ``scaling`` follows the Llama-3.1 "llama3" rope_scaling dict (factor,
    low_freq_factor, high_freq_factor, original_max_position_embeddings).
    """
    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    if scaling:
        factor = scaling.get("factor", 8.0)
        lo = scaling.get("low_freq_factor", 1.0)
        hi = scaling.get("high_freq_factor", 4.0)
        old = scaling.get("original_max_position_embeddings", 8192)
        lo_wl, hi_wl = old / lo, old / hi
        wl = 2 * math.pi / inv_freq
        scaled = torch.where(wl > lo_wl, inv_freq / factor, inv_freq)
        smooth = (old / wl - lo) / (hi - lo)
        mid = (1 - smooth) * scaled / factor + smooth * scaled
        is_mid = (wl <= lo_wl) & (wl >= hi_wl)
        inv_freq = torch.where(is_mid, mid, scaled)
    t = torch.arange(max_pos, dtype=torch.float64)
    freqs = torch.outer(t, inv_freq)
    return torch.cat([freqs.cos(), freqs.sin()], dim=-1).float().to(device)


def apply_rope(x: torch.Tensor, positions: torch.Tensor, cos_sin: torch.Tensor) -> torch.Tensor:
    """x: [T, H, D] -> rotated (fp32 math, x.dtype output)."""
    d = x.shape[-1]
    half = d // 2
    cs = cos_sin[positions.long()]  # [T, D]
    cos = cs[:, None, :half]
    sin = cs[:, None, half:]
    xf = x.float()
    x1, x2 = xf[..., :half], xf[..., half:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1).to(x.dtype)


FP8_MAX = 448.0   # float8_e4m3fn's largest finite value


def kv_scale_inv(scale: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """fp32 reciprocals of a per-head fp8 KV scale tensor, computed on the host (IEEE
    division) so the kernels' writers and this reference multiply by the same bits."""
    if scale is None:
        return None
    return (1.0 / scale.detach().to("cpu", torch.float32)).to(scale.device)


def to_cache(x: torch.Tensor, cache: torch.Tensor, inv: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x in the cache's dtype; fp8 caches clamp to the format's range first (a plain
    cast turns an out-of-range value into NaN, as gfx950's converter does).  ``inv``
    (fp8 caches): fp32 per-head reciprocal scales [nkv] for x [T, nkv, D]; stored =
    clamp(x * inv, +-448) -- the clamp comes after the scaling."""
    if cache.dtype == torch.float8_e4m3fn:
        xf = x.float()
        if inv is not None:
            xf = xf * inv.float().view(1, -1, 1)
        return xf.clamp(-FP8_MAX, FP8_MAX).to(cache.dtype)
    if inv is not None:
        raise ValueError("KV scales are given only with float8_e4m3fn caches")
    return x.to(cache.dtype)


def rope_kv_write(qkv, positions, cos_sin, slot_mapping, k_cache, v_cache, nq, nkv, head_dim,
                  k_scale=None, v_scale=None, k_inv=None, v_inv=None):
    """In place: rotate q inside ``qkv``; write rotated k and v into the paged caches.
    ``k_scale`` / ``v_scale``: per-head fp8 scales [nkv] (stored = x / scale); their
    reciprocals may be passed ready-made as ``k_inv`` / ``v_inv``."""
    if k_inv is None:
        k_inv = kv_scale_inv(k_scale)
    if v_inv is None:
        v_inv = kv_scale_inv(v_scale)
    t = qkv.shape[0]
    if t == 0:
        return
    d = head_dim
    q = qkv[:, : nq * d].view(t, nq, d)
    k = qkv[:, nq * d: (nq + nkv) * d].view(t, nkv, d)
    v = qkv[:, (nq + nkv) * d: (nq + 2 * nkv) * d].view(t, nkv, d)
    q.copy_(apply_rope(q, positions, cos_sin))
    kr = apply_rope(k, positions, cos_sin)
    slots = slot_mapping[:t].long()
    keep = slots >= 0
    if keep.any():
        bs = k_cache.shape[2]
        s = slots[keep]
        blk, off = s // bs, s % bs
        k_cache[blk, :, off, :] = to_cache(kr[keep], k_cache, k_inv)
        v_cache[blk, :, :, off] = to_cache(v[keep], v_cache, v_inv)   # V blocks transposed: [blocks, nkv, D, bs]


def _gather_kv(cache, table_row, length, transposed: bool = False):
    """[length, H, D] rows of one sequence; ``transposed``: V blocks [H, D, bs]."""
    if transposed:
        cache = cache.transpose(2, 3)
    bs = cache.shape[2]
    nblk = (length + bs - 1) // bs
    blocks = table_row[:nblk].long()
    kv = cache[blocks]  # [nblk, H, bs, D]
    kv = kv.permute(0, 2, 1, 3).reshape(nblk * bs, cache.shape[1], cache.shape[3])
    return kv[:length]


def paged_attention(q: torch.Tensor, k_cache, v_cache, block_tables, seq_lens, q_start_loc,
                    scale: float, k_scale=None, v_scale=None) -> torch.Tensor:
    """Causal varlen attention over the paged cache (K blocks [nkv, bs, D], V
    blocks transposed [nkv, D, bs]).

    q: [T, nq, D] (new tokens of every sequence, packed by q_start_loc)
    Each sequence b attends to kv positions [0, seq_lens[b]); its new tokens
    sit at the end (positions seq_len - q_len ...).  Returns [T, nq, D].
    ``k_scale`` / ``v_scale``: per-head fp8 scales [nkv]; the cache is dequantised as
    stored * scale.
    """
    t, nq, d = q.shape
    out = torch.empty_like(q)
    nkv = k_cache.shape[1]
    g = nq // nkv
    qsl = q_start_loc.tolist()
    sl = seq_lens.tolist()
    for b in range(len(sl)):
        q0, q1 = qsl[b], qsl[b + 1]
        if q1 == q0:
            continue
        L = sl[b]
        k = _gather_kv(k_cache, block_tables[b], L).float()  # [L, nkv, D]
        v = _gather_kv(v_cache, block_tables[b], L, transposed=True).float()
        if k_scale is not None:
            k = k * k_scale.float().view(1, -1, 1)
        if v_scale is not None:
            v = v * v_scale.float().view(1, -1, 1)
        qq = q[q0:q1].float()  # [ql, nq, D]
        ql = q1 - q0
        k = k.repeat_interleave(g, dim=1)
        v = v.repeat_interleave(g, dim=1)
        s = torch.einsum("qhd,khd->hqk", qq, k) * scale
        qpos = torch.arange(L - ql, L, device=q.device)[:, None]
        kpos = torch.arange(L, device=q.device)[None, :]
        s = s.masked_fill((kpos > qpos)[None], float("-inf"))
        p = torch.softmax(s, dim=-1)
        out[q0:q1] = torch.einsum("hqk,khd->qhd", p, v).to(q.dtype)
    return out


def apply_penalties(logits: torch.Tensor, prompt_mask: torch.Tensor, counts: torch.Tensor,
                    rep, pres, freq, bias_ids=None, bias_vals=None) -> torch.Tensor:
    """Logit processors of the sampler (SamplingParams.repetition_penalty /
    presence_penalty / frequency_penalty / logit_bias), the reference of
    csrc/kernels/penalties.hip.  Per row, with raw logits ``l``, the set ``prompt_mask``
    [B, V] (bool) of prompt tokens and the output counts ``counts`` [B, V]:

    1. repetition (prompt and output tokens): ``l = l / rep if l > 0 else l * rep``
    2. frequency / presence (output tokens): ``l -= freq * c + pres * (c > 0)``
    3. bias: ``l[bias_ids] += bias_vals`` (``bias_ids`` [B, K], -1 = no entry)

    ``rep`` / ``pres`` / ``freq``: [B].  fp32 throughout, each operation rounded on its
    own, one rounding to the logits' dtype at the end; an element that is in no set and
    has no bias keeps its input bits."""
    x = logits.float()
    b, v = x.shape
    f32 = dict(dtype=torch.float32, device=x.device)
    rep = torch.as_tensor(rep, **f32).reshape(b, 1)
    pres = torch.as_tensor(pres, **f32).reshape(b, 1)
    freq = torch.as_tensor(freq, **f32).reshape(b, 1)
    c = counts.to(torch.float32)
    seen = prompt_mask.bool() | (counts > 0)
    y = torch.where(x > 0, x / rep, x * rep)
    y = y - (freq * c + torch.where(counts > 0, pres, torch.zeros_like(pres)))
    y = torch.where(seen, y, x)
    touched = seen
    if bias_ids is not None and bias_ids.numel():
        ids = bias_ids.to(torch.int64)
        valid = ids >= 0
        add = torch.zeros_like(y)
        hit = torch.zeros_like(seen)
        rows = torch.arange(b, device=x.device).view(b, 1).expand_as(ids)
        add[rows[valid], ids[valid]] = bias_vals.to(torch.float32)[valid]
        hit[rows[valid], ids[valid]] = True
        y = torch.where(hit, y + add, y)
        touched = touched | hit
    return torch.where(touched, y.to(logits.dtype), logits)


LOGPROBS_MAX = 20   # OpenAI's cap on top_logprobs (csrc/kernels/logprobs.hip kLpMax)


def token_logprobs(logits: torch.Tensor, sampled, want, out_lp: Optional[torch.Tensor] = None,
                   out_id: Optional[torch.Tensor] = None):
    """Per-token logprobs of a step (SamplingParams.logprobs), the reference of
    csrc/kernels/logprobs.hip: ``(out_lp fp32, out_id int32)``, both [B, 1 + 20].

    ``logits`` [B, V] are the RAW logits (before penalties, bias, mask, temperature,
    top-k / top-p), widened to fp32; ``logprob = log_softmax(x)``.  Per row with
    ``want[r] >= 0``: column 0 holds the sampled id and its logprob, columns
    1..want[r] the want[r] most likely tokens (logit descending, ties to the lower
    id), the rest id -1 / logprob 0.0.  Rows with ``want[r] == -1`` asked for nothing:
    their output rows are left as they are (new outputs: id -1, logprob 0.0)."""
    x = logits.float()
    b, _ = x.shape
    cols = 1 + LOGPROBS_MAX
    if out_lp is None:
        out_lp = torch.zeros(b, cols, dtype=torch.float32, device=x.device)
    if out_id is None:
        out_id = torch.full((b, cols), -1, dtype=torch.int32, device=x.device)
    want = torch.as_tensor(want, dtype=torch.int64, device=x.device).reshape(-1)[:b]
    sampled = torch.as_tensor(sampled, dtype=torch.int64, device=x.device).reshape(-1)[:b]
    rows = torch.nonzero(want >= 0).flatten()
    if not rows.numel():
        return out_lp, out_id
    if int(want.max()) > LOGPROBS_MAX:
        raise ValueError(f"token_logprobs: more than {LOGPROBS_MAX} alternatives asked")
    xr = x[rows]
    lp = torch.log_softmax(xr, dim=-1)
    # a -inf logit has logprob -inf also in a row that is -inf throughout (never NaN)
    lp = torch.where(xr == float("-inf"), xr, lp)
    # +0.0 so that -0.0 and 0.0 tie (the id decides), as they compare equal
    order = torch.sort(xr + 0.0, dim=-1, descending=True, stable=True).indices[:, :LOGPROBS_MAX]
    k = order.shape[1]
    s = sampled[rows]
    res_lp = torch.zeros(rows.numel(), cols, dtype=torch.float32, device=x.device)
    res_id = torch.full((rows.numel(), cols), -1, dtype=torch.int32, device=x.device)
    res_lp[:, 0] = lp.gather(1, s.view(-1, 1)).flatten()
    res_id[:, 0] = s.to(torch.int32)
    keep = torch.arange(k, device=x.device).view(1, -1) < want[rows].view(-1, 1)
    res_lp[:, 1:1 + k] = torch.where(keep, lp.gather(1, order), torch.zeros(()))
    res_id[:, 1:1 + k] = torch.where(keep, order.to(torch.int32), torch.full((), -1, dtype=torch.int32))
    out_lp[rows] = res_lp
    out_id[rows] = res_id
    return out_lp, out_id


def prompt_logprobs(logits: torch.Tensor, targets, want, out_lp: Optional[torch.Tensor] = None,
                    out_id: Optional[torch.Tensor] = None,
                    out_rank: Optional[torch.Tensor] = None):
    """Prompt logprobs (SamplingParams.prompt_logprobs), the reference of
    csrc/kernels/logprobs.hip ft_prompt_logprobs and the CPU backend:
    ``(out_lp fp32 [B, 1 + 20], out_id int32 [B, 1 + 20], out_rank int32 [B])``.

    As :func:`token_logprobs` with the GIVEN id ``targets[r]`` in column 0, plus
    ``out_rank[r] = 1 + #{ids whose logit is greater than the target's}``: compared on the
    logits widened to fp32, -0.0 equal to +0.0, ties sharing a rank.  A -inf target has
    logprob -inf and the rank that definition gives (1 + the finite ids).  A target
    outside [0, V) reads nothing: id -1, logprob 0.0, rank 0.  Rows with ``want[r] == -1``
    are left as they are (new outputs: id -1, logprob 0.0, rank 0)."""
    x = logits.float()
    b, v = x.shape
    dev = x.device
    if out_rank is None:
        out_rank = torch.zeros(b, dtype=torch.int32, device=dev)
    want_t = torch.as_tensor(want, dtype=torch.int64, device=dev).reshape(-1)[:b]
    tgt = torch.as_tensor(targets, dtype=torch.int64, device=dev).reshape(-1)[:b]
    ok = (tgt >= 0) & (tgt < v)
    out_lp, out_id = token_logprobs(x, torch.where(ok, tgt, torch.zeros_like(tgt)), want_t,
                                    out_lp, out_id)
    rows = torch.nonzero(want_t >= 0).flatten()
    if not rows.numel():
        return out_lp, out_id, out_rank
    okr = ok[rows]
    tv = x[rows].gather(1, tgt[rows].clamp(0, v - 1).view(-1, 1))
    rank = 1 + (x[rows] > tv).sum(dim=-1)
    out_rank[rows] = torch.where(okr, rank, torch.zeros_like(rank)).to(torch.int32)
    bad = rows[~okr]
    if bad.numel():
        out_lp[bad, 0] = 0.0
        out_id[bad, 0] = -1
    return out_lp, out_id, out_rank


def sample(logits: torch.Tensor, temperature, top_p, top_k, seeds, steps,
           mask: Optional[torch.Tensor] = None,
           min_p: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Reference sampler (CPU backend).  Same contract as the HIP kernel:
    temperature <= 0 -> argmax (lowest id on ties); else top-k, then top-p over
    the survivors, then a draw from the renormalised distribution.  The draw is
    seeded by (seed, step) so it is reproducible, but it does not reproduce the
    kernel's random stream bit for bit (tests compare distributions).

    ``min_p``: None, or per-row fp32 **ln(min_p)** (-inf = off).  When given, the
    logits are first rounded to bf16, as the kernels see them, and a row with
    temperature > 0 and a finite entry keeps a token iff
    ``x >= M + temperature * ln(min_p)``: M the largest allowed logit, the product and
    the sum each rounded to fp32.  Top-k is unaffected by the order (the result is
    top-k n kept); top-p takes its nucleus over the kept set, renormalised."""
    x = logits.float().clone()
    if min_p is not None:
        x = logits.bfloat16().float().clone()
        min_p = torch.as_tensor(min_p, dtype=torch.float32).reshape(-1).cpu()
    b, v = x.shape
    if mask is not None:
        bits = mask[:b].to(torch.int64) & 0xFFFFFFFF
        ids = torch.arange(v, device=x.device)
        allowed = ((bits[:, ids // 32] >> (ids % 32)) & 1).bool()
        x = x.masked_fill(~allowed, float("-inf"))
    out = torch.empty(b, dtype=torch.int32, device=x.device)
    for i in range(b):
        row = x[i]
        t = float(temperature[i])
        if t <= 0:
            out[i] = int(torch.argmax(row))
            continue
        z = (row - row.max()) / t
        k = int(top_k[i])
        keep = torch.isfinite(z)
        if 0 < k < v:
            kth = torch.topk(row, k).values[-1]
            keep &= row >= kth
        if min_p is not None and float(min_p[i]) > float("-inf"):
            t32 = torch.tensor(t, dtype=torch.float32)
            keep &= row >= row.max() + t32 * min_p[i]   # fp32: product, then sum
        p = float(top_p[i])
        if p < 1.0:
            pr = torch.softmax(z.masked_fill(~keep, float("-inf")), dim=-1)
            sp, si = torch.sort(pr, descending=True)
            cum = torch.cumsum(sp, 0)
            n_keep = int(torch.searchsorted(cum, torch.tensor(p, dtype=cum.dtype)).item()) + 1
            thr = sp[min(n_keep, v) - 1]
            keep &= pr >= thr
        probs = torch.softmax(z.masked_fill(~keep, float("-inf")), dim=-1)
        gen = torch.Generator(device="cpu")
        gen.manual_seed((int(seeds[i]) * 1000003 + int(steps[i])) & 0x7FFFFFFFFFFFFFFF)
        out[i] = int(torch.multinomial(probs.cpu(), 1, generator=gen).item())
    return out
