"""Weights: deterministic random init and (TP-sharded) safetensors loading.

Layout produced here and handed to :class:`LlamaModel` (all
``[out_features, in_features]``; on the GPU the model re-lays every projection out
into the MFMA-fragment image the hand-written GEMMs stream, ``ops.pack_weight``, and
drops these row-major tensors; the CPU backend keeps them for ``F.linear``):

* ``wqkv``  [ (nq + 2 nkv)/tp * D, H ]   column parallel, q|k|v fused
* ``wo``    [ H, nq/tp * D ]             row parallel (all-reduce after)
* ``wgu``   [ 2 I/tp, H ]                column parallel, gate|up fused
* ``wd``    [ H, I/tp ]                  row parallel (all-reduce after)
* ``embed`` [ V, H ] replicated; ``lm_head`` [ V/tp, H ] vocab parallel.

E14 in SURVEY.md §2.3 (model weights cache -> random-init or local checkpoint).
"""
from __future__ import annotations

import glob
import json
import os
from typing import Dict, Optional

import torch

from .config import ModelConfig


def tp_heads(cfg: ModelConfig, tp: int):
    assert cfg.num_heads % tp == 0, "num_heads must divide by tp"
    nq = cfg.num_heads // tp
    if cfg.num_kv_heads >= tp:
        assert cfg.num_kv_heads % tp == 0
        nkv = cfg.num_kv_heads // tp
    else:
        assert tp % cfg.num_kv_heads == 0
        nkv = 1
    return nq, nkv


def kv_head_range(cfg: ModelConfig, tp: int, rank: int):
    nq, nkv = tp_heads(cfg, tp)
    if cfg.num_kv_heads >= tp:
        return rank * nkv, (rank + 1) * nkv
    rep = tp // cfg.num_kv_heads
    h = rank // rep
    return h, h + 1


def _shard_rows(t: torch.Tensor, rank: int, tp: int) -> torch.Tensor:
    n = t.shape[0] // tp
    return t[rank * n:(rank + 1) * n]


def _shard_cols(t: torch.Tensor, rank: int, tp: int) -> torch.Tensor:
    n = t.shape[1] // tp
    return t[:, rank * n:(rank + 1) * n]


def shard_full_layer(cfg: ModelConfig, full: Dict[str, torch.Tensor], rank: int, tp: int):
    """Full (unsharded) HF-layout layer tensors -> this rank's fused shards."""
    d = cfg.head_dim
    q = full["q"].view(cfg.num_heads, d, -1)
    k = full["k"].view(cfg.num_kv_heads, d, -1)
    v = full["v"].view(cfg.num_kv_heads, d, -1)
    nq, _ = tp_heads(cfg, tp)
    k0, k1 = kv_head_range(cfg, tp, rank)
    qs = q[rank * nq:(rank + 1) * nq].reshape(-1, q.shape[-1])
    ks = k[k0:k1].reshape(-1, k.shape[-1])
    vs = v[k0:k1].reshape(-1, v.shape[-1])
    gate = _shard_rows(full["gate"], rank, tp)
    up = _shard_rows(full["up"], rank, tp)
    return {
        "wqkv": torch.cat([qs, ks, vs], 0).contiguous(),
        "wo": _shard_cols(full["o"], rank, tp).contiguous(),
        "wgu": torch.cat([gate, up], 0).contiguous(),
        "wd": _shard_cols(full["down"], rank, tp).contiguous(),
        "ln1": full["ln1"].contiguous(),
        "ln2": full["ln2"].contiguous(),
    }


def random_full_layer(cfg: ModelConfig, gen: torch.Generator, std: float, dtype):
    h, i, d = cfg.hidden_size, cfg.intermediate_size, cfg.head_dim

    def rn(*shape):
        return (torch.randn(*shape, generator=gen, device=gen.device) * std).to(dtype)

    return {
        "q": rn(cfg.num_heads * d, h), "k": rn(cfg.num_kv_heads * d, h),
        "v": rn(cfg.num_kv_heads * d, h), "o": rn(h, cfg.num_heads * d),
        "gate": rn(i, h), "up": rn(i, h), "down": rn(h, i),
        "ln1": torch.ones(h, dtype=dtype), "ln2": torch.ones(h, dtype=dtype),
    }


def random_layer_fast(cfg: ModelConfig, rank: int, tp: int, layer: int, seed: int, std: float,
                      dtype, device) -> Dict[str, torch.Tensor]:
    """Per-shard random init generated directly on ``device`` (large models).

    Not TP-consistent (a TP=2 shard is not a slice of the TP=1 tensor) but
    statistically identical; used for benchmarking where the full unsharded
    tensors would be wasted work.
    """
    h, i, d = cfg.hidden_size, cfg.intermediate_size, cfg.head_dim
    nq, nkv = tp_heads(cfg, tp)
    g = torch.Generator(device=device)
    g.manual_seed(seed * 1000003 + layer * 9176 + rank * 31 + 1)

    def rn(*shape):
        t = torch.empty(*shape, dtype=dtype, device=device)
        t.normal_(0.0, std, generator=g)
        return t

    return {
        "wqkv": rn((nq + 2 * nkv) * d, h), "wo": rn(h, nq * d),
        "wgu": rn(2 * (i // tp), h), "wd": rn(h, i // tp),
        "ln1": torch.ones(h, dtype=dtype, device=device),
        "ln2": torch.ones(h, dtype=dtype, device=device),
    }


# --------------------------------------------------------------------------------------
# safetensors checkpoints (HF Llama naming)
# --------------------------------------------------------------------------------------

class SafetensorsIndex:
    def __init__(self, ckpt_dir: str):
        from safetensors import safe_open  # noqa: F401

        self.dir = ckpt_dir
        idx = os.path.join(ckpt_dir, "model.safetensors.index.json")
        self.map: Dict[str, str] = {}
        if os.path.exists(idx):
            with open(idx) as f:
                self.map = {k: os.path.join(ckpt_dir, v) for k, v in json.load(f)["weight_map"].items()}
        else:
            from safetensors import safe_open

            for fn in sorted(glob.glob(os.path.join(ckpt_dir, "*.safetensors"))):
                with safe_open(fn, framework="pt") as f:
                    for k in f.keys():
                        self.map[k] = fn
        self._open: Dict[str, object] = {}

    def has(self, name: str) -> bool:
        return name in self.map

    def get(self, name: str) -> torch.Tensor:
        from safetensors import safe_open

        fn = self.map[name]
        if fn not in self._open:
            self._open[fn] = safe_open(fn, framework="pt")
        return self._open[fn].get_tensor(name)


def load_full_layer(idx: SafetensorsIndex, layer: int, dtype) -> Dict[str, torch.Tensor]:
    p = f"model.layers.{layer}."
    names = {
        "q": "self_attn.q_proj.weight", "k": "self_attn.k_proj.weight",
        "v": "self_attn.v_proj.weight", "o": "self_attn.o_proj.weight",
        "gate": "mlp.gate_proj.weight", "up": "mlp.up_proj.weight", "down": "mlp.down_proj.weight",
        "ln1": "input_layernorm.weight", "ln2": "post_attention_layernorm.weight",
    }
    return {k: idx.get(p + v).to(dtype) for k, v in names.items()}


# --------------------------------------------------------------------------------------
# fp8 KV-cache scales carried by a checkpoint
# --------------------------------------------------------------------------------------
# Accepted per-layer tensor names (suffix after "model.layers.N."): key -> which of
# (K, V) it sets.  vLLM's fp8-KV checkpoints use k_scale / v_scale; the legacy form is
# one kv_scale for both.  No real fp8-KV checkpoint was at hand to check this list
# against, so it is kept in this one table.
KV_SCALE_NAMES = {
    "self_attn.k_scale": ("k",),
    "self_attn.v_scale": ("v",),
    "self_attn.kv_scale": ("k", "v"),
}


def check_kv_scales(t: torch.Tensor, what: str) -> torch.Tensor:
    """fp32 copy of a scale tensor; raises unless every value is finite and > 0."""
    t = torch.as_tensor(t, dtype=torch.float32)
    if not bool(torch.isfinite(t).all()) or not bool((t > 0).all()):
        raise ValueError(f"{what}: KV scales must be finite and positive, got {t.flatten().tolist()}")
    return t


def load_kv_scales(cfg: ModelConfig, idx: "SafetensorsIndex"):
    """(k, v) fp32 [num_layers, num_kv_heads] from a checkpoint's per-layer scale
    tensors (KV_SCALE_NAMES; a scalar / one element is broadcast over the heads, or
    [num_kv_heads]); None when the checkpoint has none.  Layers without a tensor keep
    1.0.  A non-finite or non-positive scale raises."""
    out = {"k": torch.ones(cfg.num_layers, cfg.num_kv_heads),
           "v": torch.ones(cfg.num_layers, cfg.num_kv_heads)}
    found = False
    for li in range(cfg.num_layers):
        for suffix, targets in KV_SCALE_NAMES.items():
            name = f"model.layers.{li}.{suffix}"
            if not idx.has(name):
                continue
            t = check_kv_scales(idx.get(name), name).flatten()
            if t.numel() not in (1, cfg.num_kv_heads):
                raise ValueError(f"{name}: {t.numel()} elements, expected 1 or {cfg.num_kv_heads}")
            for which in targets:
                out[which][li] = t   # one element broadcasts over the heads
            found = True
    return (out["k"], out["v"]) if found else None


def shard_kv_scales(cfg: ModelConfig, full: torch.Tensor, rank: int, tp: int) -> torch.Tensor:
    """[num_layers, num_kv_heads] -> this rank's kv heads [num_layers, nkv]."""
    k0, k1 = kv_head_range(cfg, tp, rank)
    return full[:, k0:k1].contiguous()


# --------------------------------------------------------------------------------------
# AWQ (W4A16) checkpoints: AutoAWQ "GEMM" tensors per projection
# --------------------------------------------------------------------------------------
_HF_PROJ = {"q": "self_attn.q_proj", "k": "self_attn.k_proj", "v": "self_attn.v_proj",
            "o": "self_attn.o_proj", "gate": "mlp.gate_proj", "up": "mlp.up_proj",
            "down": "mlp.down_proj"}


def is_awq_checkpoint(idx: SafetensorsIndex) -> bool:
    cfg_path = os.path.join(idx.dir, "config.json")
    if os.path.exists(cfg_path):
        with open(cfg_path) as f:
            qc = json.load(f).get("quantization_config") or {}
        if str(qc.get("quant_method", "")).lower() == "awq":
            if int(qc.get("bits", 4)) != 4 or int(qc.get("group_size", 128)) != 128:
                raise ValueError("only 4-bit AWQ with group size 128 is supported")
            return True
    return idx.has("model.layers.0.self_attn.q_proj.qweight")


def load_awq_layer_shard(cfg: ModelConfig, idx: SafetensorsIndex, layer: int, rank: int, tp: int):
    """One layer of an AWQ checkpoint -> this rank's fused shards as (q, z, s)
    triples ([N, K] uint8, [N, K/128] uint8, [N, K/128] fp32).  The head / row /
    column slicing is the bf16 path's (:func:`shard_full_layer`) applied to q, z
    and s alike: groups run along K, so a row-parallel shard of K/tp columns
    (a multiple of 128) keeps whole groups."""
    from ..ops.quant import awq_unpack

    p = f"model.layers.{layer}."
    parts = {"q": {}, "z": {}, "s": {}}
    for name, hf in _HF_PROJ.items():
        q, z, s = awq_unpack(idx.get(p + hf + ".qweight"), idx.get(p + hf + ".qzeros"),
                             idx.get(p + hf + ".scales"))
        parts["q"][name], parts["z"][name], parts["s"][name] = q, z, s
    ln = {"ln1": idx.get(p + "input_layernorm.weight"),
          "ln2": idx.get(p + "post_attention_layernorm.weight")}
    sh = {k: shard_full_layer(cfg, dict(v, **ln), rank, tp) for k, v in parts.items()}
    out = {a: (sh["q"][a], sh["z"][a], sh["s"][a]) for a in ("wqkv", "wo", "wgu", "wd")}
    out.update(ln1=ln["ln1"], ln2=ln["ln2"])
    return out


def save_awq_checkpoint(cfg: ModelConfig, full_layers, embed, norm, lm_head, out_dir: str):
    """Quantize full-precision layers (RTN, group 128) and write them in the
    AutoAWQ GEMM layout with an HF ``quantization_config`` (tests and tooling)."""
    from safetensors.torch import save_file

    from ..ops.quant import awq_pack, quantize_w4

    save_hf_checkpoint(cfg, [], embed, norm, lm_head, out_dir)
    path = os.path.join(out_dir, "model.safetensors")
    from safetensors.torch import load_file

    t = load_file(path)
    for li, L in enumerate(full_layers):
        p = f"model.layers.{li}."
        for name, hf in _HF_PROJ.items():
            qw, qz, sc = awq_pack(*quantize_w4(L[name].to(torch.bfloat16)))
            t[p + hf + ".qweight"], t[p + hf + ".qzeros"], t[p + hf + ".scales"] = qw, qz, sc
        t[p + "input_layernorm.weight"] = L["ln1"].contiguous()
        t[p + "post_attention_layernorm.weight"] = L["ln2"].contiguous()
    save_file(t, path)
    with open(os.path.join(out_dir, "config.json")) as f:
        hf_cfg = json.load(f)
    hf_cfg["quantization_config"] = {"quant_method": "awq", "bits": 4, "group_size": 128,
                                     "zero_point": True, "version": "gemm"}
    with open(os.path.join(out_dir, "config.json"), "w") as f:
        json.dump(hf_cfg, f, indent=1)


# --------------------------------------------------------------------------------------
# fp8 (W8A16) checkpoints: float8_e4m3fn weights with per-channel or per-tensor scales
# --------------------------------------------------------------------------------------
# Accepted tensor names per projection (suffix after "model.layers.N.<proj>"): what vLLM
# writes for --quantization fp8 and AMD Quark FP8 exports.  No real fp8 checkpoint was
# at hand to check this list against, so parity with one is unpinned and the names are
# kept in this one table.
FP8_NAMES = {
    "weight": ".weight",              # float8_e4m3fn [N, K]
    "scale": ".weight_scale",         # fp32 scalar, [1], [N] or [N, 1]
    "ignored": (".input_scale",),     # static activation scales of W8A8 checkpoints
}
_FP8_FUSED = {"wqkv": ("q", "k", "v"), "wo": ("o",), "wgu": ("gate", "up"), "wd": ("down",)}
_fp8_logged_input_scale = False


def is_fp8_checkpoint(idx: SafetensorsIndex) -> bool:
    """The first q_proj weight is float8_e4m3fn and has a weight_scale (with or without
    a ``quantization_config`` naming quant_method fp8)."""
    p = "model.layers.0." + _HF_PROJ["q"]
    if not (idx.has(p + FP8_NAMES["weight"]) and idx.has(p + FP8_NAMES["scale"])):
        return False
    return idx.get(p + FP8_NAMES["weight"]).dtype == torch.float8_e4m3fn


def _fp8_proj(idx: SafetensorsIndex, base: str):
    """(q float8_e4m3fn [N, K], s fp32 [N]) of one projection; raises on NaN weight bytes
    and on scales that are not finite and positive."""
    from ..ops.quant import fp8_nan_bytes

    q = idx.get(base + FP8_NAMES["weight"])
    if q.dtype != torch.float8_e4m3fn or q.dim() != 2:
        raise ValueError(f"{base}{FP8_NAMES['weight']}: expected a 2-D float8_e4m3fn tensor, "
                         f"got {q.dtype} {tuple(q.shape)}")
    if bool(fp8_nan_bytes(q).any()):
        raise ValueError(f"{base}{FP8_NAMES['weight']}: holds NaN bytes")
    n = q.shape[0]
    s = idx.get(base + FP8_NAMES["scale"]).float().flatten()
    if s.numel() not in (1, n):
        raise ValueError(f"{base}{FP8_NAMES['scale']}: {s.numel()} elements, expected 1 or {n}")
    if not bool(torch.isfinite(s).all()) or not bool((s > 0).all()):
        raise ValueError(f"{base}{FP8_NAMES['scale']}: scales must be finite and positive")
    return q.contiguous(), s.expand(n).contiguous()


def load_fp8_layer(cfg: ModelConfig, idx: SafetensorsIndex, layer: int):
    """One layer of an fp8 checkpoint (TP=1) -> fused projections as (q, s) pairs
    ([N, K] float8_e4m3fn, [N] fp32) plus the norm weights.  Scales are broadcast to one
    per output channel, so fusing q/k/v (or gate/up) that carry different per-tensor
    scales is the concatenation of their channel vectors.  ``input_scale`` tensors are
    ignored (the activations stay bf16), with one log line."""
    global _fp8_logged_input_scale
    p = f"model.layers.{layer}."
    parts = {}
    for name, hf in _HF_PROJ.items():
        parts[name] = _fp8_proj(idx, p + hf)
        if not _fp8_logged_input_scale and any(idx.has(p + hf + sfx) for sfx in FP8_NAMES["ignored"]):
            _fp8_logged_input_scale = True
            import logging

            logging.getLogger(__name__).info(
                "fp8 checkpoint carries input_scale tensors (static W8A8 activation scales): "
                "ignored, activations stay bf16")
    out = {}
    for attr, names in _FP8_FUSED.items():
        out[attr] = (torch.cat([parts[m][0].view(torch.uint8) for m in names], 0)
                     .view(torch.float8_e4m3fn).contiguous(),
                     torch.cat([parts[m][1] for m in names], 0).contiguous())
    out["ln1"] = idx.get(p + "input_layernorm.weight")
    out["ln2"] = idx.get(p + "post_attention_layernorm.weight")
    return out


def save_fp8_checkpoint(cfg: ModelConfig, full_layers, embed, norm, lm_head, out_dir: str,
                        scale_form: str = "channel", input_scale: bool = False):
    """Quantize full-precision layers to fp8 e4m3 (ops.quant.quantize_w8) and write them
    as ``<proj>.weight`` / ``<proj>.weight_scale`` with an HF ``quantization_config``
    (tests and tooling).  ``scale_form``: "channel" ([N]), "channel2d" ([N, 1]), or one
    scale per tensor as "tensor" (a scalar) / "tensor1" ([1]).  ``input_scale`` also
    writes a W8A8-style static activation scale per projection."""
    from safetensors.torch import load_file, save_file

    from ..ops.quant import FP8, FP8_MAX, quantize_w8

    if scale_form not in ("channel", "channel2d", "tensor", "tensor1"):
        raise ValueError(f"scale_form {scale_form!r}: channel | channel2d | tensor | tensor1")
    save_hf_checkpoint(cfg, [], embed, norm, lm_head, out_dir)
    path = os.path.join(out_dir, "model.safetensors")
    t = load_file(path)
    for li, L in enumerate(full_layers):
        p = f"model.layers.{li}."
        for name, hf in _HF_PROJ.items():
            w = L[name].to(torch.bfloat16)
            if scale_form.startswith("channel"):
                q, s = quantize_w8(w)
                s = s.view(-1, 1) if scale_form == "channel2d" else s
            else:
                amax = float(w.double().abs().max())
                s = torch.tensor(amax / FP8_MAX if amax > 0 else 1.0, dtype=torch.float32)
                q = (w.double() / s.double()).clamp(-FP8_MAX, FP8_MAX).to(FP8)
                s = s.view(1) if scale_form == "tensor1" else s
            t[p + hf + FP8_NAMES["weight"]] = q.contiguous()
            t[p + hf + FP8_NAMES["scale"]] = s.clone().contiguous()
            if input_scale:
                t[p + hf + ".input_scale"] = torch.tensor(1.0)
        t[p + "input_layernorm.weight"] = L["ln1"].contiguous()
        t[p + "post_attention_layernorm.weight"] = L["ln2"].contiguous()
    save_file(t, path)
    with open(os.path.join(out_dir, "config.json")) as f:
        hf_cfg = json.load(f)
    hf_cfg["quantization_config"] = {"quant_method": "fp8", "activation_scheme": "dynamic"}
    with open(os.path.join(out_dir, "config.json"), "w") as f:
        json.dump(hf_cfg, f, indent=1)


# --------------------------------------------------------------------------------------
# MXFP4 (W4A16) checkpoints: OCP MX e2m1 weights, one e8m0 scale per 32 k-values
# --------------------------------------------------------------------------------------
# Accepted tensors per projection (suffix after "model.layers.N.<proj>"), the layout AMD
# Quark MXFP4 exports use: two codes per byte, the EVEN k in the LOW nibble.  No real
# MXFP4 export was at hand to check this against, so the names and the nibble order of
# the checkpoint layout are unpinned; both are kept in this one table and in
# ops.quant.mx4_from_packed.
MX4_NAMES = {
    "weight": ".weight",              # uint8 or float4_e2m1fn_x2 [N, K/2]
    "scale": ".weight_scale",         # uint8 or float8_e8m0fnu [N, K/32]
    "ignored": (".input_scale", ".weight_zero_point"),
}
_mx4_logged_ignored = False


def _mx4_dtypes():
    w = {torch.uint8}
    s = {torch.uint8}
    if hasattr(torch, "float4_e2m1fn_x2"):
        w.add(torch.float4_e2m1fn_x2)
    if hasattr(torch, "float8_e8m0fnu"):
        s.add(torch.float8_e8m0fnu)
    return w, s


def is_mx4_checkpoint(idx: SafetensorsIndex) -> bool:
    """Layer 0's q_proj has a byte-typed ``weight`` [N, K/2] and a byte-typed
    ``weight_scale`` [N, K/32] (uint8 or the float4_e2m1fn_x2 / float8_e8m0fnu spellings).
    fp8 checkpoints carry float8_e4m3fn weights and AWQ ones ``qweight``: no overlap."""
    p = "model.layers.0." + _HF_PROJ["q"]
    if not (idx.has(p + MX4_NAMES["weight"]) and idx.has(p + MX4_NAMES["scale"])):
        return False
    w, s = idx.get(p + MX4_NAMES["weight"]), idx.get(p + MX4_NAMES["scale"])
    wd, sd = _mx4_dtypes()
    return (w.dtype in wd and s.dtype in sd and w.dim() == 2 and s.dim() == 2
            and w.shape[0] == s.shape[0] and w.shape[1] * 2 == s.shape[1] * 32)


def _mx4_proj(idx: SafetensorsIndex, base: str):
    """(codes uint8 [N, K], scale bytes uint8 [N, K/32]) of one projection; raises on a
    wrong dtype or shape and on scale bytes outside [2, 252], naming the tensor."""
    from ..ops.quant import mx4_check_scale_bytes, mx4_from_packed

    wd, sd = _mx4_dtypes()
    w = idx.get(base + MX4_NAMES["weight"])
    if w.dtype not in wd or w.dim() != 2:
        raise ValueError(f"{base}{MX4_NAMES['weight']}: expected a 2-D uint8 / float4_e2m1fn_x2 "
                         f"tensor, got {w.dtype} {tuple(w.shape)}")
    s = idx.get(base + MX4_NAMES["scale"])
    n, k = w.shape[0], w.shape[1] * 2
    if s.dtype not in sd or tuple(s.shape) != (n, k // 32) or k % 32:
        raise ValueError(f"{base}{MX4_NAMES['scale']}: expected uint8 / float8_e8m0fnu "
                         f"{(n, k // 32)}, got {s.dtype} {tuple(s.shape)}")
    mx4_check_scale_bytes(s, base + MX4_NAMES["scale"])
    return mx4_from_packed(w.contiguous(), s.contiguous())


def load_mx4_layer(cfg: ModelConfig, idx: SafetensorsIndex, layer: int):
    """One layer of an MXFP4 checkpoint (TP=1) -> fused projections as (codes, scale
    bytes) pairs plus the norm weights.  Blocks run along K, so fusing q/k/v (or gate/up)
    is the row concatenation of their codes and scale rows.  Other tensors of a
    projection (``input_scale``, ...) are ignored, with one log line."""
    global _mx4_logged_ignored
    p = f"model.layers.{layer}."
    parts = {}
    for name, hf in _HF_PROJ.items():
        parts[name] = _mx4_proj(idx, p + hf)
        if not _mx4_logged_ignored and any(idx.has(p + hf + sfx) for sfx in MX4_NAMES["ignored"]):
            _mx4_logged_ignored = True
            import logging

            logging.getLogger(__name__).info(
                "MXFP4 checkpoint carries extra per-projection tensors (input_scale / zero "
                "points): ignored, activations stay bf16")
    out = {}
    for attr, names in _FP8_FUSED.items():
        out[attr] = (torch.cat([parts[m][0] for m in names], 0).contiguous(),
                     torch.cat([parts[m][1] for m in names], 0).contiguous())
    out["ln1"] = idx.get(p + "input_layernorm.weight")
    out["ln2"] = idx.get(p + "post_attention_layernorm.weight")
    return out


def save_mx4_checkpoint(cfg: ModelConfig, full_layers, embed, norm, lm_head, out_dir: str,
                        typed: bool = False, input_scale: bool = False):
    """Quantize full-precision layers to MXFP4 (ops.quant.quantize_mx4) and write them as
    ``<proj>.weight`` [N, K/2] / ``<proj>.weight_scale`` [N, K/32] with an HF
    ``quantization_config`` (tests and tooling).  ``typed``: the float4_e2m1fn_x2 /
    float8_e8m0fnu spellings instead of uint8.  ``input_scale`` also writes a static
    activation scale per projection (ignored on load)."""
    from safetensors.torch import load_file, save_file

    from ..ops.quant import mx4_to_packed, quantize_mx4

    save_hf_checkpoint(cfg, [], embed, norm, lm_head, out_dir)
    path = os.path.join(out_dir, "model.safetensors")
    t = load_file(path)
    for li, L in enumerate(full_layers):
        p = f"model.layers.{li}."
        for name, hf in _HF_PROJ.items():
            wb, sb = mx4_to_packed(*quantize_mx4(L[name].to(torch.bfloat16)))
            if typed:
                wb, sb = wb.view(torch.float4_e2m1fn_x2), sb.view(torch.float8_e8m0fnu)
            t[p + hf + MX4_NAMES["weight"]] = wb.contiguous()
            t[p + hf + MX4_NAMES["scale"]] = sb.contiguous()
            if input_scale:
                t[p + hf + ".input_scale"] = torch.tensor(1.0)
        t[p + "input_layernorm.weight"] = L["ln1"].contiguous()
        t[p + "post_attention_layernorm.weight"] = L["ln2"].contiguous()
    save_file(t, path)
    with open(os.path.join(out_dir, "config.json")) as f:
        hf_cfg = json.load(f)
    hf_cfg["quantization_config"] = {"quant_method": "quark", "weight_format": "mxfp4"}
    with open(os.path.join(out_dir, "config.json"), "w") as f:
        json.dump(hf_cfg, f, indent=1)


def save_hf_checkpoint(cfg: ModelConfig, full_layers, embed, norm, lm_head: Optional[torch.Tensor],
                       out_dir: str, kv_scales: Optional[Dict[str, object]] = None):
    """Write an HF-layout safetensors checkpoint (used by tests and tooling).
    ``kv_scales``: fp8 KV-cache scales to store, {"k": per-layer values, "v": ...} or
    the legacy {"kv": ...}; each per-layer value a float or a tensor of 1 or
    num_kv_heads elements (written as self_attn.k_scale / v_scale / kv_scale)."""
    from safetensors.torch import save_file

    os.makedirs(out_dir, exist_ok=True)
    t = {"model.embed_tokens.weight": embed.contiguous(), "model.norm.weight": norm.contiguous()}
    if lm_head is not None and not cfg.tie_word_embeddings:
        t["lm_head.weight"] = lm_head.contiguous()
    inv = {"q": "self_attn.q_proj.weight", "k": "self_attn.k_proj.weight",
           "v": "self_attn.v_proj.weight", "o": "self_attn.o_proj.weight",
           "gate": "mlp.gate_proj.weight", "up": "mlp.up_proj.weight",
           "down": "mlp.down_proj.weight", "ln1": "input_layernorm.weight",
           "ln2": "post_attention_layernorm.weight"}
    for li, L in enumerate(full_layers):
        for k, v in L.items():
            t[f"model.layers.{li}.{inv[k]}"] = v.contiguous()
    for key, per_layer in (kv_scales or {}).items():
        if f"self_attn.{key}_scale" not in KV_SCALE_NAMES:
            raise ValueError(f"kv_scales key {key!r}: k | v | kv")
        for li, val in enumerate(per_layer):
            t[f"model.layers.{li}.self_attn.{key}_scale"] = \
                torch.as_tensor(val, dtype=torch.float32).clone().contiguous()
    save_file(t, os.path.join(out_dir, "model.safetensors"))
    hf = {
        "hidden_size": cfg.hidden_size, "num_hidden_layers": cfg.num_layers,
        "num_attention_heads": cfg.num_heads, "num_key_value_heads": cfg.num_kv_heads,
        "head_dim": cfg.head_dim, "intermediate_size": cfg.intermediate_size,
        "vocab_size": cfg.vocab_size, "rope_theta": cfg.rope_theta,
        "rope_scaling": cfg.rope_scaling, "rms_norm_eps": cfg.rms_norm_eps,
        "tie_word_embeddings": cfg.tie_word_embeddings,
        "max_position_embeddings": cfg.max_position_embeddings,
        "bos_token_id": cfg.bos_token_id, "eos_token_id": list(cfg.eos_token_ids),
        "architectures": ["LlamaForCausalLM"],
    }
    with open(os.path.join(out_dir, "config.json"), "w") as f:
        json.dump(hf, f, indent=1)
