"""Prompt logprobs (SamplingParams.prompt_logprobs) without a GPU: validation, the
reference's rank, the engine bookkeeping on the CPU backend (whole prompts, chunked
prefill, the prefix cache, recompute preemption), delivery and the refusals."""
import asyncio

import numpy as np
import pytest
import torch

from fasttalk_llm_microservice_amd import ops
from fasttalk_llm_microservice_amd.engine.config import EngineConfig
from fasttalk_llm_microservice_amd.engine.engine import EngineError, LLMEngine
from fasttalk_llm_microservice_amd.engine.sampling_params import (SamplingParams,
                                                                   pick_prompt_logprobs)
from fasttalk_llm_microservice_amd.engine.sequence import RequestOutput, coalesce
from fasttalk_llm_microservice_amd.models.llama import AttnMeta
from fasttalk_llm_microservice_amd.ops import reference as ref

K = ops.LOGPROBS_MAX
NEG_INF = float("-inf")


def test_sampling_params_prompt_logprobs():
    assert SamplingParams().prompt_logprobs is None
    assert [SamplingParams(prompt_logprobs=k).prompt_logprobs for k in (0, 5, 20)] == [0, 5, 20]
    for bad in (-1, 21, 1.5, "3", True):
        with pytest.raises(ValueError):
            SamplingParams(prompt_logprobs=bad)


def test_pick_prompt_logprobs():
    assert pick_prompt_logprobs({}) is None
    assert pick_prompt_logprobs({"prompt_logprobs": None}) is None
    assert [pick_prompt_logprobs({"prompt_logprobs": k}) for k in (0, 1, 20)] == [0, 1, 20]
    for bad in (-1, 21, 2.0, "1", True, [1]):
        with pytest.raises(ValueError):
            pick_prompt_logprobs({"prompt_logprobs": bad})


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_reference_rank_against_a_numpy_count(dtype):
    g = torch.Generator().manual_seed(11)
    v = 1003
    x = (torch.randn(8, v, generator=g) * 4).to(dtype)
    x[1, :] = 1.25                       # all equal: every id has rank 1
    x[2, 100:140] = 30.0                 # 40 ids share the maximum
    x[2, 500] = 29.5                     # just below them
    x[3, 10], x[3, 20] = -0.0, 0.0       # the two zeros compare equal
    x[4, ::3] = NEG_INF
    targets = [7, 999, 500, 10, 3, v - 1, v + 5, 0]
    want = [20, 0, 5, 1, 3, 20, 2, -1]
    lp, ids, rank = ref.prompt_logprobs(x, targets, want, torch.full((8, 1 + K), 123.0),
                                        torch.full((8, 1 + K), -77, dtype=torch.int32),
                                        torch.full((8,), -5, dtype=torch.int32))
    xf = x.float().numpy().astype(np.float64)
    for r, (t, w) in enumerate(zip(targets, want)):
        if w < 0:   # untouched
            assert rank[r] == -5 and bool((lp[r] == 123.0).all()) and bool((ids[r] == -77).all())
            continue
        if not 0 <= t < v:   # outside the row: nothing read
            assert (int(ids[r, 0]), float(lp[r, 0]), int(rank[r])) == (-1, 0.0, 0)
            continue
        assert int(rank[r]) == 1 + int((xf[r] > xf[r, t]).sum()), r
        assert int(ids[r, 0]) == t
    assert rank.tolist()[:6] == [rank[0].item(), 1, 41, rank[3].item(), 1 + int(np.isfinite(xf[4]).sum()),
                                 rank[5].item()]
    lp2, ids2, rank2 = ref.prompt_logprobs(x, [20] * 8, [0] * 8)
    assert rank2[3] == rank[3] and lp[4, 0] == NEG_INF
    # column 0 aside, it is token_logprobs; the op's CPU backend is this reference
    tl, ti = ref.token_logprobs(x, [t if 0 <= t < v else 0 for t in targets], want)
    rows = [r for r, w in enumerate(want) if w >= 0]
    assert torch.equal(ids[rows, 1:], ti[rows, 1:]) and torch.equal(lp[rows, 1:], tl[rows, 1:])
    ol, oi, orank = ops.prompt_logprobs(x, torch.tensor(targets, dtype=torch.int32),
                                        torch.tensor(want, dtype=torch.int32))
    assert torch.equal(orank[rows], rank[rows]) and torch.equal(oi[rows], ids[rows])


# ------------------------------------------------------------------------------- engine
def _engine(**kw):
    base = dict(model="tiny", device="cpu", dtype="float32", num_kv_blocks=256, max_model_len=512,
                max_num_seqs=8, enable_prefix_caching=False)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def _prompt(n, seed=0):
    return np.random.default_rng(seed).integers(0, 120000, n).tolist()


def _run(eng, reqs):
    """{request id: [RequestOutput]} of ``reqs`` = [(id, prompt, params)] run to the end."""
    outs = {}
    eng.runner.plp_tap = []
    for rid, p, sp in reqs:
        eng.add_request(rid, p, sp, on_output=lambda o: outs.setdefault(o.request_id, []).append(o))
    while eng.has_work():
        eng.step()
    return outs


def _whole_prompt_logprobs(eng, prompt):
    """float64 log_softmax of ONE forward over the whole prompt (the engine is idle: its
    KV pool is free to be written)."""
    m, T, bs = eng.runner.model, len(prompt), eng.cfg.block_size
    nblk = -(-T // bs)
    tiles, _ = ops.build_prefill_tiles([T], ops.prefill_tile_tokens(m.nq, m.nkv))
    meta = AttnMeta(
        positions=torch.arange(T, dtype=torch.int32), slot_mapping=torch.arange(T, dtype=torch.int32),
        block_tables=torch.arange(nblk, dtype=torch.int32)[None],
        seq_lens=torch.tensor([T], dtype=torch.int32), logits_indices=torch.arange(T),
        q_start_loc=torch.tensor([0, T], dtype=torch.int32),
        tile_info=torch.tensor(tiles, dtype=torch.int32).flatten(), num_tiles=len(tiles))
    with torch.inference_mode():
        logits = m.compute_logits(m.forward(torch.tensor(prompt, dtype=torch.int32), meta, eng.runner.kv))
    return torch.log_softmax(logits.double(), dim=-1)


def _tapped(eng, rid, n):
    """The raw logits the engine scored for positions 0..n-2 of request ``rid`` (the last
    tap of a position is the one that was stored)."""
    rows = {}
    for r, p0, raw in eng.runner.plp_tap:
        if r == rid:
            for k in range(raw.shape[0]):
                rows[p0 + k] = raw[k]
    assert sorted(rows) == list(range(n - 1))
    return torch.stack([rows[p] for p in range(n - 1)])


def _check_entries(plp, prompt, want, lp64, raw, tol=1e-4):
    """Logprobs within ``tol`` of ``lp64`` (float64 log_softmax of one whole-prompt
    forward); ranks exactly the count over ``raw``, the logits the engine itself scored
    (a rank is an integer: two forwards that differ by fp32 rounding order near-ties
    differently)."""
    assert len(plp) == len(prompt) and plp[0] is None
    for j in range(1, len(prompt)):
        tid, lp, rank, alts = plp[j]
        assert tid == prompt[j] and len(alts) == want
        assert abs(lp - lp64[j - 1, tid].item()) <= tol, (j, lp, lp64[j - 1, tid].item())
        assert rank == 1 + int((raw[j - 1] > raw[j - 1, tid]).sum())
        assert [a for a, _ in alts] == torch.sort(raw[j - 1] + 0.0, descending=True,
                                                  stable=True).indices[:want].tolist()
        for a, alp in alts:
            assert abs(alp - lp64[j - 1, a].item()) <= tol
        assert [alp for _, alp in alts] == sorted((alp for _, alp in alts), reverse=True)
        if alts:
            assert abs(alts[0][1] - lp64[j - 1].max().item()) <= tol


def test_cpu_engine_entries_match_one_whole_prompt_forward():
    """Three prompts, two ask (3 and 0 alternatives): one prefilled whole, one chunked
    (prefill_chunk 16 with a second prompt in the step), against log_softmax of one
    forward over the whole prompt within 1e-4 (fp32 model; the engine's chunked
    attention and the whole-prompt forward differ by fp32 rounding only)."""
    eng = _engine(max_num_batched_tokens=48)
    pa, pb, pc = _prompt(37, 1), _prompt(90, 2), _prompt(9, 3)
    sp = lambda k: SamplingParams(temperature=0.0, max_tokens=3, ignore_eos=True, prompt_logprobs=k)  # noqa: E731
    outs = _run(eng, [("a", pa, sp(3)), ("b", pb, sp(0)), ("c", pc, sp(None))])
    m = eng.metrics()
    assert m["prompt_logprob_rows"] == 36 + 89 and m["prompt_logprob_steps"] >= 3   # b is chunked
    for rid, p, k in (("a", pa, 3), ("b", pb, 0)):
        ev = outs[rid]
        assert ev[0].prompt_logprobs is not None and all(o.prompt_logprobs is None for o in ev[1:])
        _check_entries(ev[0].prompt_logprobs, p, k, _whole_prompt_logprobs(eng, p),
                       _tapped(eng, rid, len(p)))
    assert all(o.prompt_logprobs is None for o in outs["c"])
    # the tokens are those of a run where nobody asks, and that run scores nothing
    off = _engine(max_num_batched_tokens=48)
    bare = SamplingParams(temperature=0.0, max_tokens=3, ignore_eos=True)
    plain = _run(off, [("a", pa, bare), ("b", pb, bare), ("c", pc, bare)])
    for rid in "abc":
        assert [t for o in plain[rid] for t in o.token_ids] == [t for o in outs[rid] for t in o.token_ids]
    assert off.metrics()["prompt_logprob_steps"] == 0 and off.runner.d_plp is None


def test_one_token_prompt_gives_a_list_of_none():
    eng = _engine()
    outs = _run(eng, [("one", [77], SamplingParams(temperature=0.0, max_tokens=2, ignore_eos=True,
                                                   prompt_logprobs=5))])
    assert outs["one"][0].prompt_logprobs == [None]
    assert eng.metrics()["prompt_logprob_rows"] == 0


def test_prefix_cache_is_bypassed_until_every_position_is_scored():
    eng = _engine(enable_prefix_caching=True)
    p = _prompt(70, 4)
    bare = SamplingParams(temperature=0.0, max_tokens=2, ignore_eos=True)
    first = _run(eng, [("warm", p, bare)])["warm"]
    hit = _run(eng, [("hit", p, bare)])["hit"]
    assert hit[0].num_cached_tokens == 64
    ask = _run(eng, [("ask", p, SamplingParams(temperature=0.0, max_tokens=2, ignore_eos=True,
                                               prompt_logprobs=1))])["ask"]
    assert ask[0].num_cached_tokens == 0
    plp = ask[0].prompt_logprobs
    assert len(plp) == 70 and plp[0] is None and [e[0] for e in plp[1:]] == p[1:]
    assert [t for o in ask for t in o.token_ids] == [t for o in first for t in o.token_ids]
    again = _run(eng, [("again", p, bare)])["again"]
    assert again[0].num_cached_tokens == 64


def test_recompute_preemption_mid_prefill_scores_every_position_once():
    """A pool of 10 blocks: two sequences decode while a 100-token prompt that asked is
    prefilled in chunks of at most 18 tokens; the pool cannot hold all three, so the
    prompt's blocks are taken away mid-prefill (recompute: its epoch is bumped, queued
    chunks of it go stale) and it is re-admitted.  Every position is stored exactly once,
    in order, and each re-admission attaches at most plp_next // block_size cached
    blocks."""
    eng = _engine(num_kv_blocks=10, enable_prefix_caching=True, max_num_batched_tokens=18,
                  max_model_len=256)
    bs = eng.cfg.block_size
    p = _prompt(100, 5)
    stored, attach = [], []
    real_store, real_match = eng._plp_store, eng.bm.match_prefix

    def store(chunks):
        seq = eng.scheduler.by_id.get("long")
        before = seq.plp_next if seq is not None else None
        real_store(chunks)
        if seq is not None and seq.plp_next != before:
            stored.append((before, seq.plp_next))

    class BM:   # the block manager with match_prefix observed
        def __getattr__(self, name):
            return getattr(eng.bm, name)

    def match(tokens, max_blocks):
        seq = eng.scheduler.by_id.get("long")
        if seq is not None and len(tokens) == seq.n_tokens and list(tokens[:100]) == p:
            attach.append((max_blocks, seq.plp_next, seq.epoch))
        return real_match(tokens, max_blocks)

    bm = BM()
    bm.match_prefix = match
    eng._plp_store = store
    eng.scheduler.bm = bm
    dec = SamplingParams(temperature=0.0, max_tokens=40, ignore_eos=True)
    outs = _run(eng, [("d0", _prompt(20, 6), dec), ("d1", _prompt(20, 7), dec),
                      ("long", p, SamplingParams(temperature=0.0, max_tokens=2, ignore_eos=True,
                                                 prompt_logprobs=2))])
    # its KV was dropped while part of the prompt was scored, and it was admitted again
    assert any(0 < nxt < 99 and ep > 0 for _, nxt, ep in attach), attach
    assert all(mb <= nxt // bs for mb, nxt, _ in attach), attach
    # positions stored once and in order: the advances tile [0, 99) without overlap
    assert stored[0][0] == 0 and stored[-1][1] == 99
    assert all(a[1] == b[0] for a, b in zip(stored, stored[1:])), stored
    plp = outs["long"][0].prompt_logprobs
    assert len(plp) == 100 and plp[0] is None and [e[0] for e in plp[1:]] == p[1:]
    assert all(len(e[3]) == 2 for e in plp[1:])
    assert eng.metrics()["prompt_logprob_rows"] >= 99
    assert len([t for o in outs["long"] for t in o.token_ids]) == 2
    _check_entries(plp, p, 2, _whole_prompt_logprobs(eng, p), _tapped(eng, "long", 100))


def test_coalesce_keeps_the_field():
    async def run():
        q = asyncio.Queue()
        q.put_nowait(RequestOutput("r", "b", [2]))
        q.put_nowait(RequestOutput("r", "c", [3], finished=True, finish_reason="length"))
        plp = [None, (5, -1.0, 2, [(7, -0.5)])]
        return coalesce(RequestOutput("r", "a", [1], prompt_logprobs=plp), q), plp

    out, plp = asyncio.run(run())
    assert out.prompt_logprobs is plp and out.token_ids == [1, 2, 3] and out.finished


def test_refusals():
    from fasttalk_llm_microservice_amd.engine.guided import GuidedSpec

    eng = _engine()
    spec = GuidedSpec.json_schema({"type": "object", "properties": {"a": {"type": "integer"}},
                                   "required": ["a"]})
    with pytest.raises(EngineError, match="prompt_logprobs are not supported with guided decoding"):
        eng.add_request("g", [1, 2, 3], SamplingParams(max_tokens=4, guided=spec, prompt_logprobs=1))
    with pytest.raises(EngineError, match="prompt_logprobs are not supported with background"):
        eng.add_request("bg", [1, 2, 3], SamplingParams(max_tokens=1, prompt_logprobs=0),
                        background=True)
    eng.cfg.tp_size = 2
    with pytest.raises(EngineError, match="not supported with tensor parallelism yet"):
        eng.add_request("tp", [1, 2, 3], SamplingParams(max_tokens=2, prompt_logprobs=0))
    eng.cfg.tp_size = 1

    class NoOp:   # a runner without the op
        def __getattr__(self, name):
            if name == "take_prompt_logprobs":
                raise AttributeError(name)
            return getattr(runner, name)

    runner, eng.runner = eng.runner, NoOp()
    with pytest.raises(EngineError, match="not supported by this runner"):
        eng.add_request("r", [1, 2, 3], SamplingParams(max_tokens=2, prompt_logprobs=0))
    eng.runner = runner
    assert not eng._plp_reqs and not eng.runner.plp_active
    assert not eng.has_work()
