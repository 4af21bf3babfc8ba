"""Sampling parameters (E10).  Mirrors what the reference forwards to its
backends: temperature / max_tokens / top_p / stop (vLLM,
``app/core/vllm_handler.py:149-164``) and top_k / num_predict (Ollama,
``app/core/ollama_handler.py:145-155``)."""
from __future__ import annotations

import dataclasses
import math
import random
from typing import Any, List, Optional


PENALTY_KEYS = ("repetition_penalty", "presence_penalty", "frequency_penalty", "logit_bias")


def pick_penalties(src) -> dict:
    """The penalty fields a request dict (an OpenAI body, a WebSocket session config)
    sets, under SamplingParams' names; Ollama's ``repeat_penalty`` is accepted for
    ``repetition_penalty``.  Validated: raises ValueError like SamplingParams does."""
    out = {k: src[k] for k in PENALTY_KEYS if src.get(k) is not None}
    if "repetition_penalty" not in out and src.get("repeat_penalty") is not None:
        out["repetition_penalty"] = src["repeat_penalty"]
    if out:
        SamplingParams(**out)
    return out


LOGPROBS_MAX = 20   # OpenAI's cap on top_logprobs (ops.LOGPROBS_MAX)


def pick_logprobs(src) -> Optional[int]:
    """OpenAI's pair ``logprobs: true`` / ``top_logprobs: n`` of a request body as
    SamplingParams.logprobs: None when the request does not ask, else n (0 without
    ``top_logprobs``).  ``top_logprobs`` without ``logprobs: true``, a non-integer or an
    n outside 0..20 raises ValueError."""
    on, top = src.get("logprobs"), src.get("top_logprobs")
    if on is not None and not isinstance(on, bool):
        raise ValueError("logprobs must be true or false")
    if top is None:
        return 0 if on else None
    if isinstance(top, bool) or not isinstance(top, int):
        raise ValueError("top_logprobs must be an integer")
    if not on:
        raise ValueError("top_logprobs requires logprobs: true")
    if not 0 <= top <= LOGPROBS_MAX:
        raise ValueError(f"top_logprobs must be in 0..{LOGPROBS_MAX}")
    return top


def pick_prompt_logprobs(src) -> Optional[int]:
    """vLLM's ``prompt_logprobs: n`` of a request body as SamplingParams.prompt_logprobs:
    None when the request does not ask, else n.  A non-integer or an n outside 0..20
    raises ValueError."""
    v = src.get("prompt_logprobs")
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, int):
        raise ValueError("prompt_logprobs must be an integer")
    if not 0 <= v <= LOGPROBS_MAX:
        raise ValueError(f"prompt_logprobs must be in 0..{LOGPROBS_MAX}")
    return v


def pick_min_p(src) -> dict:
    """``min_p`` of a request dict (an OpenAI body, a WebSocket session config) as
    SamplingParams keywords: empty when the request does not set it.  Validated: raises
    ValueError like SamplingParams does."""
    v = src.get("min_p")
    if v is None:
        return {}
    return {"min_p": SamplingParams(min_p=v).min_p}


def ln_min_p(min_p: float) -> float:
    """What the sampler takes for ``min_p``: ln(min_p) computed in float64 (rounded once
    to fp32 where it is stored), -inf for 0 = off."""
    return math.log(min_p) if min_p > 0.0 else float("-inf")


@dataclasses.dataclass
class SamplingParams:
    temperature: float = 0.7
    top_p: float = 1.0
    top_k: int = 0               # <= 0: disabled
    max_tokens: int = 2048
    min_tokens: int = 0
    stop: Optional[List[str]] = None
    stop_token_ids: Optional[List[int]] = None
    ignore_eos: bool = False
    seed: Optional[int] = None
    guided: Any = None           # engine.guided.GuidedSpec (JSON-schema constrained decoding)
    # the grammar binds only if the first generated token is a valid start of it (e.g.
    # the model chose to open a tool call with '{"'); otherwise the reply is free text
    guided_lazy: bool = False
    skip_special_tokens: bool = True
    # scheduling priority: waiting prompts of a higher priority are prefilled first
    # (an agent's post-tool re-prompt: its user has already waited through the call)
    priority: int = 0
    # logit processors, applied to the raw logits in this order before the allow-mask,
    # temperature, top-k and top-p (ops/reference.py apply_penalties):
    # repetition (HF / vLLM ``repetition_penalty``, Ollama ``repeat_penalty``): a token of
    # the prompt or the output so far has its logit divided (> 0) or multiplied (<= 0)
    repetition_penalty: float = 1.0
    # OpenAI: -= presence_penalty once / frequency_penalty per occurrence in the output
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    # OpenAI: token id (int or decimal str, as in the JSON) -> bias in [-100, 100]
    logit_bias: Optional[dict] = None
    # per-token logprobs over the RAW logits (before the processors above, the
    # allow-mask, temperature, top-k and top-p; vLLM's default): None = off, 0..20 = the
    # sampled token's logprob plus that many most likely alternatives
    logprobs: Optional[int] = None
    # vLLM / Ollama ``min_p`` in [0, 1], 0 = off: after the processors above, the
    # allow-mask and temperature, before top-k / top-p, a token is kept iff
    # p(token) >= min_p * p_max (ops/reference.py sample).  Greedy rows ignore it.
    min_p: float = 0.0
    # vLLM ``prompt_logprobs``: None = off, 0..20 = for every prompt position after the
    # first, the prompt token's logprob and rank given the tokens before it, plus that
    # many most likely alternatives -- over the raw logits, like ``logprobs``
    prompt_logprobs: Optional[int] = None

    MAX_LOGIT_BIAS = 300

    def _check_min_p(self):
        v = self.min_p
        if v is None:
            v = 0.0
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= v <= 1.0:
            raise ValueError("min_p must be a number in [0, 1]")
        self.min_p = float(v)

    def _check_logprobs(self):
        v = self.logprobs
        if v is None:
            return
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= LOGPROBS_MAX:
            raise ValueError(f"logprobs must be None or an integer in 0..{LOGPROBS_MAX}")

    def _check_prompt_logprobs(self):
        v = self.prompt_logprobs
        if v is None:
            return
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= LOGPROBS_MAX:
            raise ValueError(f"prompt_logprobs must be None or an integer in 0..{LOGPROBS_MAX}")

    @property
    def has_penalties(self) -> bool:
        return self.repetition_penalty != 1.0 or self.presence_penalty != 0.0 or \
            self.frequency_penalty != 0.0 or bool(self.logit_bias)

    def _check_penalties(self):
        def num(name, default):
            v = getattr(self, name)
            if v is None:
                v = default
            if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
                raise ValueError(f"{name} must be a number")
            setattr(self, name, float(v))
            return float(v)

        if not num("repetition_penalty", 1.0) > 0.0 or self.repetition_penalty == float("inf"):
            raise ValueError("repetition_penalty must be > 0")
        for name in ("presence_penalty", "frequency_penalty"):
            if not -2.0 <= num(name, 0.0) <= 2.0:
                raise ValueError(f"{name} must be in [-2, 2]")
        if self.logit_bias is None:
            return
        if not isinstance(self.logit_bias, dict):
            raise ValueError("logit_bias must be a map of token id -> bias")
        if len(self.logit_bias) > self.MAX_LOGIT_BIAS:
            raise ValueError(f"logit_bias holds at most {self.MAX_LOGIT_BIAS} entries")
        bias = {}
        for k, v in self.logit_bias.items():
            if isinstance(k, str) and k.strip().lstrip("+-").isdigit():
                k = int(k.strip())
            if isinstance(k, bool) or not isinstance(k, int) or k < 0:
                raise ValueError(f"logit_bias key {k!r} is not a token id")
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not -100.0 <= v <= 100.0:
                raise ValueError(f"logit_bias[{k}] must be in [-100, 100]")
            if k in bias:
                raise ValueError(f"logit_bias names token {k} twice")
            bias[k] = float(v)
        self.logit_bias = bias or None

    def __post_init__(self):
        self._check_penalties()
        self._check_logprobs()
        self._check_prompt_logprobs()
        self._check_min_p()
        if self.temperature is None:
            self.temperature = 0.7
        if self.temperature < 0:
            raise ValueError("temperature must be >= 0")
        if self.top_p is None:
            self.top_p = 1.0
        if not 0.0 < self.top_p <= 1.0:
            raise ValueError("top_p must be in (0, 1]")
        if self.top_k is None:
            self.top_k = 0
        if self.max_tokens is None or self.max_tokens < 1:
            raise ValueError("max_tokens must be >= 1")
        if self.seed is None:
            self.seed = random.getrandbits(62)
        if isinstance(self.stop, str):
            self.stop = [self.stop]
