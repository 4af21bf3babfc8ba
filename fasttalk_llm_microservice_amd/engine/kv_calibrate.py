"""Per-head scales for the fp8 (e4m3) KV cache.

Storage convention (vLLM's): ``stored = clamp(x / scale, +-448)``, ``x ~= stored *
scale``, one scale per layer and kv head, separately for K and V.  This module turns
the ``EngineConfig.kv_scales`` setting into those scales:

* ``auto``      the checkpoint's scales when it carries them, else 1.0
* ``one``       always 1.0 (the cache exactly as it was before scales existed)
* ``calibrate`` one eager prefill of a built-in chat prompt into a small temporary
                cache in the compute dtype; the per-head absmax of K (post-RoPE) and V
                is read straight from the blocks it wrote
* a ``.json``   ``{"k": [[nkv floats] per layer], "v": [...]}`` for all unsharded kv
                heads (``save_kv_scales`` writes it): calibrate once, reuse

``calibrate`` works on a bare :class:`LlamaModel`; ``resolve`` is what the runner calls.
"""
from __future__ import annotations

import json
import logging
import os
from typing import List, Optional, Sequence, Tuple

import torch

from .. import ops
from ..models import weights as W
from ..models.llama import AttnMeta, LlamaModel

log = logging.getLogger(__name__)

FP8_MAX = 448.0
# scale = headroom * absmax / 448.  2.0 is a design default, not a measured one: on
# random-init weights 1.0 and 2.0 give the same logits (cosine 0.99911 / 0.99811 against
# fp32 KV on tiny / tiny-2k), and nobody has measured either on a real checkpoint.  It
# trades one bit of e4m3 resolution for K / V twice as large as the calibration prompt
# showed before anything clips.
DEFAULT_HEADROOM = 2.0
# floor of a calibrated scale: an all-zero head must not produce a zero scale
SCALE_TINY = 2.0 ** -20
DEFAULT_CALIB_TOKENS = 512
MIN_CALIB_TOKENS = 256

# ordinary chat text for the calibration prefill (rendered through the chat template)
_CALIB_CHAT = [
    ("system", "You are a friendly voice assistant. Keep answers short, clear and spoken in "
               "plain language, because they are read aloud."),
    ("user", "Hi! I just got home and I'm trying to decide what to cook tonight. I have rice, "
             "eggs, a few carrots, some frozen peas and half an onion."),
    ("assistant", "That sounds like fried rice to me. Scramble the eggs first, set them aside, "
                  "then fry the onion and carrots, add the rice and peas, and stir the eggs "
                  "back in with a little soy sauce."),
    ("user", "Nice. How long does that take, roughly? I have a call at 7:30 and it's 6:45 now."),
    ("assistant", "About twenty minutes if the rice is already cooked, thirty-five if not. You "
                  "will make your call either way, but start the rice now."),
    ("user", "Okay. Can you also remind me what the weather is supposed to be tomorrow? I need "
             "to bike to work, it's about 9 kilometres."),
    ("assistant", "I can't see a live forecast, but if you tell me your city I can say what is "
                  "typical for this time of year and what to pack just in case."),
    ("user", "It's Gothenburg, early October. And what is 9 km in miles, by the way?"),
    ("assistant", "Nine kilometres is about 5.6 miles. Early October in Gothenburg is usually "
                  "10 to 13 degrees with a good chance of rain and wind from the sea, so bring "
                  "a shell jacket and lights for the ride home."),
    ("user", "Thanks! Last thing: set a timer for the rice, 18 minutes, and tell me a fun fact "
             "while I chop the carrots."),
]


def calibration_messages() -> List[dict]:
    return [{"role": r, "content": c} for r, c in _CALIB_CHAT]


def calib_token_cap() -> int:
    """``ENGINE_KV_CALIB_TOKENS``: the longest calibration prompt (default 512)."""
    try:
        return max(1, int(os.environ.get("ENGINE_KV_CALIB_TOKENS", DEFAULT_CALIB_TOKENS)))
    except ValueError:
        return DEFAULT_CALIB_TOKENS


def headroom() -> float:
    """``ENGINE_KV_SCALE_HEADROOM`` (default 2.0, see DEFAULT_HEADROOM)."""
    try:
        h = float(os.environ.get("ENGINE_KV_SCALE_HEADROOM", DEFAULT_HEADROOM))
    except ValueError:
        return DEFAULT_HEADROOM
    if not (h > 0 and h < float("inf")):
        raise ValueError(f"ENGINE_KV_SCALE_HEADROOM must be a positive number, got {h}")
    return h


def calibration_prompt_ids(template, max_tokens: Optional[int] = None, max_len: int = 0,
                           vocab: int = 0) -> List[int]:
    """The built-in chat rendered through ``template`` (a ChatTemplate), repeated until
    it has at least 256 tokens, cut to ``max_tokens`` (default: ENGINE_KV_CALIB_TOKENS)
    and to the model's context."""
    cap = max_tokens or calib_token_cap()
    if max_len > 0:
        cap = min(cap, max_len)
    msgs = calibration_messages()
    ids = list(template.render(msgs))
    while len(ids) < min(cap, MIN_CALIB_TOKENS):
        msgs = msgs + calibration_messages()[1:]
        more = list(template.render(msgs))
        if len(more) <= len(ids):
            break
        ids = more
    ids = ids[:cap]
    if vocab > 0:
        ids = [i % vocab for i in ids]
    return ids


def default_prompt_ids(cfg, model_cfg, max_len: int) -> List[int]:
    """Calibration prompt for an engine configuration: its tokenizer and chat template."""
    from .chat_template import ChatTemplate
    from .tokenizer import get_tokenizer

    tok_path = cfg.tokenizer
    if tok_path is None and cfg.weights not in ("random", None, ""):
        tok_path = cfg.weights
    return calibration_prompt_ids(ChatTemplate(get_tokenizer(tok_path)), max_len=max_len,
                                  vocab=model_cfg.vocab_size)


@torch.no_grad()
def measure_absmax(model: LlamaModel, token_ids: Sequence[int],
                   block_size: int = 16) -> Tuple[torch.Tensor, torch.Tensor]:
    """(k_absmax, v_absmax) fp32 [num_layers, nkv] of this rank's kv heads over one eager
    prefill of ``token_ids`` through the model's own kernels, read from a temporary
    cache in the compute dtype (freed on return)."""
    t = len(token_ids)
    if t == 0:
        raise ValueError("calibration needs at least one token")
    dev = model.device
    nblk = -(-t // block_size)
    kv = model.allocate_kv_cache(nblk, block_size)   # compute dtype: nothing is scaled
    qlens = [t]
    tiles, comb = ops.build_prefill_tiles(qlens, ops.prefill_tile_tokens(model.nq, model.nkv))
    assert not comb
    meta = AttnMeta(
        positions=torch.arange(t, dtype=torch.int32, device=dev),
        slot_mapping=torch.arange(t, dtype=torch.int32, device=dev),
        block_tables=torch.arange(nblk, dtype=torch.int32, device=dev)[None].contiguous(),
        seq_lens=torch.tensor([t], dtype=torch.int32, device=dev),
        logits_indices=torch.tensor([t - 1], device=dev),
        q_start_loc=torch.tensor([0, t], dtype=torch.int32,
                                 device=dev if dev.type == "cuda" else "cpu"),
        tile_info=torch.tensor(tiles, dtype=torch.int32, device=dev).flatten(),
        num_tiles=len(tiles))
    ids = torch.tensor(list(token_ids), dtype=torch.int32, device=dev)
    saved = model.kv_scales
    model.kv_scales = None
    try:
        model.forward(ids, meta, kv)
    finally:
        model.kv_scales = saved
    # K blocks [blocks, nkv, bs, D], V blocks [blocks, nkv, D, bs]; unwritten slots are 0
    k_abs = torch.stack([kc.float().abs().amax(dim=(0, 2, 3)) for kc, _ in kv]).cpu()
    v_abs = torch.stack([vc.float().abs().amax(dim=(0, 2, 3)) for _, vc in kv]).cpu()
    del kv
    return k_abs, v_abs


def scales_from_absmax(absmax: torch.Tensor, headroom_: Optional[float] = None) -> torch.Tensor:
    h = headroom() if headroom_ is None else headroom_
    return torch.clamp(absmax.float() * (h / FP8_MAX), min=SCALE_TINY)


def calibrate(model: LlamaModel, token_ids: Sequence[int], headroom_: Optional[float] = None,
              block_size: int = 16) -> Tuple[torch.Tensor, torch.Tensor]:
    """Measures and installs calibrated scales on ``model``; returns (k, v) [layers, nkv]."""
    k_abs, v_abs = measure_absmax(model, token_ids, block_size)
    if not bool(torch.isfinite(k_abs).all()) or not bool(torch.isfinite(v_abs).all()):
        raise ValueError("KV calibration saw a non-finite K or V value")
    k, v = scales_from_absmax(k_abs, headroom_), scales_from_absmax(v_abs, headroom_)
    model.set_kv_scales(k, v, source="calibrate")
    return k, v


# ---------------------------------------------------------------------------------
# the kv_scales setting
# ---------------------------------------------------------------------------------

def parse_setting(value: Optional[str]) -> Tuple[str, Optional[str]]:
    """("auto" | "one" | "calibrate" | "file", path): anything else raises ValueError."""
    v = (value or "auto").strip()
    low = v.lower()
    if low in ("auto", "one", "calibrate"):
        return low, None
    if low.endswith(".json"):
        return "file", v
    raise ValueError(f"kv_scales {value!r}: auto | one | calibrate | a path to a .json file")


def load_scales_json(path: str, model_cfg) -> Tuple[torch.Tensor, torch.Tensor]:
    """(k, v) fp32 [num_layers, num_kv_heads] from a kv-scales JSON file."""
    with open(path) as f:
        d = json.load(f)
    out = []
    for key in ("k", "v"):
        if key not in d:
            raise ValueError(f"{path}: missing {key!r}")
        t = W.check_kv_scales(torch.tensor(d[key], dtype=torch.float32), f"{path} {key!r}")
        if tuple(t.shape) != (model_cfg.num_layers, model_cfg.num_kv_heads):
            raise ValueError(f"{path}: {key!r} has shape {tuple(t.shape)}, expected "
                             f"{(model_cfg.num_layers, model_cfg.num_kv_heads)}")
        out.append(t)
    return out[0], out[1]


def save_scales_json(path: str, k: torch.Tensor, v: torch.Tensor):
    with open(path, "w") as f:
        json.dump({"k": [[float(x) for x in row] for row in k.tolist()],
                   "v": [[float(x) for x in row] for row in v.tolist()]}, f, indent=1)


def resolve(cfg, model_cfg, model: LlamaModel, kv_dtype, max_len: int) -> str:
    """Applies ``cfg.kv_scales`` to ``model`` (before its fp8 pool exists); returns the
    scale source: one | checkpoint | calibrate | file."""
    mode, path = parse_setting(getattr(cfg, "kv_scales", "auto"))
    fp8 = kv_dtype == torch.float8_e4m3fn
    if not fp8:
        if mode not in ("auto", "one"):
            raise ValueError(f"kv_scales={cfg.kv_scales!r} needs kv_cache_dtype=fp8")
        return "one"
    if mode == "one":
        return "one"
    if mode == "auto":
        if model.ckpt_kv_scales is None:
            return "one"
        model.set_kv_scales(*model.ckpt_kv_scales, source="checkpoint")
        return "checkpoint"
    if mode == "file":
        k, v = load_scales_json(path, model_cfg)
        model.set_kv_scales(W.shard_kv_scales(model_cfg, k, model.rank, model.tp),
                            W.shard_kv_scales(model_cfg, v, model.rank, model.tp), source="file")
        return "file"
    if model.tp > 1:
        raise ValueError("kv_scales=calibrate runs on one device: calibrate once at TP=1 "
                         "(save_kv_scales), then pass the JSON")
    calibrate(model, default_prompt_ids(cfg, model_cfg, max_len))
    return "calibrate"
