"""Per-token logprobs on the CPU backend: SamplingParams / pick_logprobs validation, the
fp32 reference ``ops.reference.token_logprobs`` against a float64 log_softmax and a stable
sort, the tiny CPU engine checked step by step against its raw logit taps, and the
refusals."""
import numpy as np
import pytest
import torch

from fasttalk_llm_microservice_amd import ops
from fasttalk_llm_microservice_amd.engine.config import EngineConfig
from fasttalk_llm_microservice_amd.engine.engine import EngineError, LLMEngine
from fasttalk_llm_microservice_amd.engine.sampling_params import SamplingParams, pick_logprobs
from fasttalk_llm_microservice_amd.ops import reference as ref

K = ops.LOGPROBS_MAX


# ------------------------------------------------------------------------- parameters
def test_sampling_params_logprobs():
    assert SamplingParams().logprobs is None
    assert [SamplingParams(logprobs=k).logprobs for k in (0, 5, 20)] == [0, 5, 20]
    for bad in (-1, 21, 1.5, "3", True):
        with pytest.raises(ValueError, match="logprobs"):
            SamplingParams(logprobs=bad)


def test_pick_logprobs():
    assert K == 20
    assert pick_logprobs({}) is None
    assert pick_logprobs({"logprobs": False}) is None
    assert pick_logprobs({"logprobs": None, "top_logprobs": None}) is None
    assert pick_logprobs({"logprobs": True}) == 0
    assert pick_logprobs({"logprobs": True, "top_logprobs": 0}) == 0
    assert pick_logprobs({"logprobs": True, "top_logprobs": 20}) == 20
    for body in ({"top_logprobs": 3}, {"logprobs": False, "top_logprobs": 3},
                 {"logprobs": True, "top_logprobs": 21}, {"logprobs": True, "top_logprobs": -1},
                 {"logprobs": True, "top_logprobs": 2.0}, {"logprobs": True, "top_logprobs": "2"},
                 {"logprobs": True, "top_logprobs": True}, {"logprobs": 1}):
        with pytest.raises(ValueError):
            pick_logprobs(body)


# ------------------------------------------------------------------------------ reference
def _expected(x, sampled, want):
    """float64 log_softmax + a stable descending sort, row by row."""
    lp = torch.log_softmax(x.double(), dim=-1)
    out = []
    for r in range(x.shape[0]):
        if want[r] < 0:
            out.append(None)
            continue
        row = x[r].double().numpy()
        order = np.lexsort((np.arange(row.size), -row))[:want[r]].tolist()   # value desc, id asc
        out.append(([sampled[r]] + order, lp[r, [sampled[r]] + order]))
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_reference_against_float64(dtype):
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(3, 1003, generator=g) * 4).to(dtype)
    x[1, 100:140] = 30.0                # 40 ids share the maximum: the lowest 20 win
    x[2, 7] = float("-inf")
    sampled, want = [0, 1002, 7], [5, 20, 0]
    lp, ids = ref.token_logprobs(x, sampled, want)
    assert lp.shape == ids.shape == (3, 1 + K) and lp.dtype == torch.float32 and ids.dtype == torch.int32
    exp = _expected(x.float(), sampled, want)
    for r, (eids, elp) in enumerate(exp):
        n = len(eids)
        assert ids[r, :n].tolist() == eids
        assert bool((ids[r, n:] == -1).all()) and bool((lp[r, n:] == 0.0).all())
        fin = torch.isfinite(elp)
        assert bool(((lp[r, :n].double() - elp)[fin].abs() <= 1e-4).all())
        assert bool((lp[r, :n][~fin] == float("-inf")).all())
    assert ids[1, 1:].tolist() == list(range(100, 120))
    assert lp[2, 0] == float("-inf")
    # rows that asked for nothing keep what the outputs held
    out_lp, out_id = torch.full((3, 1 + K), 7.0), torch.full((3, 1 + K), 9, dtype=torch.int32)
    ref.token_logprobs(x, sampled, [-1, 3, -1], out_lp, out_id)
    assert bool((out_lp[[0, 2]] == 7.0).all()) and bool((out_id[[0, 2]] == 9).all())
    assert out_id[1, :4].tolist() == [1002, 100, 101, 102] and out_id[1, 4] == -1
    assert ops.logprobs(x, sampled, want)[1].tolist() == ids.tolist()   # the CPU backend
    with pytest.raises(ValueError):
        ref.token_logprobs(x, sampled, [21, 0, 0])


# --------------------------------------------------------------------------------- engine
LENS = [6, 9, 5, 8]
ASKS = [None, 0, 5, 20]


def _engine(**kw):
    base = dict(model="tiny", device="cpu", num_kv_blocks=256, max_model_len=512, max_num_seqs=8,
                enable_prefix_caching=False)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def _run(eng, params):
    g = torch.Generator().manual_seed(2)
    prompts = [torch.randint(0, 120000, (n,), generator=g).tolist() for n in (7, 12, 5, 9)]
    r = eng.runner
    r.logits_tap, r.logits_tap_ids = [], []
    events = {}
    for i, (p, sp) in enumerate(zip(prompts, params)):
        eng.add_request(f"r{i}", p, sp, on_output=lambda o, i=i: events.setdefault(i, []).append(o))
    while eng.has_work():
        eng.step()
    tap = {}
    for logits, ids in zip(r.logits_tap, r.logits_tap_ids):
        for row, rid in enumerate(ids or []):
            tap.setdefault(rid, []).append(logits[row].float())
    r.logits_tap = r.logits_tap_ids = None
    return events, tap


def test_engine_logprobs_align_with_tokens_and_match_the_raw_taps():
    kw = [dict(temperature=0.0), dict(temperature=0.0, presence_penalty=1.5, repetition_penalty=1.3),
          dict(temperature=0.9, seed=11), dict(temperature=0.0)]
    eng = _engine()
    events, tap = _run(eng, [SamplingParams(max_tokens=n, ignore_eos=True, logprobs=a, **k)
                             for n, a, k in zip(LENS, ASKS, kw)])
    toks = {}
    for i, ask in enumerate(ASKS):
        toks[i] = [t for o in events[i] for t in o.token_ids]
        assert len(toks[i]) == LENS[i] and events[i][-1].finished
        if ask is None:
            assert all(o.logprobs is None for o in events[i])
            continue
        entries = []
        for o in events[i]:
            assert o.logprobs is not None and len(o.logprobs) == len(o.token_ids)
            assert [e[0] for e in o.logprobs] == o.token_ids
            entries += o.logprobs
        for k, (tid, lp, alts) in enumerate(entries):
            raw = tap[f"r{i}"][k].view(1, -1)
            (eids, elp), = _expected(raw, [tid], [ask])
            assert [tid] + [a[0] for a in alts] == eids
            got = torch.tensor([lp] + [a[1] for a in alts], dtype=torch.float64)
            assert bool(((got - elp).abs() <= 1e-4).all()), (i, k, got, elp)
    m = eng.metrics()
    assert m["logprob_steps"] > 0 and m["logprob_rows"] == sum(LENS[1:])

    off = _engine()
    events2, _ = _run(off, [SamplingParams(max_tokens=n, ignore_eos=True, **k) for n, k in zip(LENS, kw)])
    assert [t for o in events2[0] for t in o.token_ids] == toks[0]
    # nothing about the sampling changes for the ones that ask either
    assert all([t for o in events2[i] for t in o.token_ids] == toks[i] for i in range(1, 4))
    assert all(o.logprobs is None for ev in events2.values() for o in ev)
    assert off.metrics()["logprob_steps"] == 0 and off.metrics()["logprob_rows"] == 0


def test_the_stop_token_that_ends_a_reply_has_no_entry():
    eng = _engine()
    first = eng.generate([[5, 6, 7]], SamplingParams(temperature=0.0, max_tokens=3, ignore_eos=True))[0]
    outs = []
    eng.add_request("s", [5, 6, 7], SamplingParams(temperature=0.0, max_tokens=8, logprobs=2,
                                                   stop_token_ids=[first[2]]), on_output=outs.append)
    while eng.has_work():
        eng.step()
    assert outs[-1].finished and outs[-1].finish_reason == "stop"
    assert [t for o in outs for t in o.token_ids] == first[:first.index(first[2])]
    assert all(len(o.logprobs) == len(o.token_ids) for o in outs) and outs[-1].logprobs == []


def test_refusals():
    from fasttalk_llm_microservice_amd.engine.guided import GuidedSpec

    eng = _engine()
    spec = GuidedSpec.json_schema({"type": "object", "properties": {"n": {"type": "integer"}},
                                   "required": ["n"]})
    with pytest.raises(EngineError, match="guided"):
        eng.add_request("g", [1, 2, 3], SamplingParams(max_tokens=4, guided=spec, logprobs=1))
    with pytest.raises(EngineError, match="guided"):
        eng.add_request("gl", [1, 2, 3], SamplingParams(max_tokens=4, guided=spec, guided_lazy=True,
                                                        logprobs=1))
    eng.cfg.tp_size = 2
    with pytest.raises(EngineError, match="not supported with tensor parallelism yet"):
        eng.add_request("tp", [1, 2, 3], SamplingParams(max_tokens=2, logprobs=0))
    eng.add_request("tp-plain", [1, 2, 3], SamplingParams(max_tokens=1))
    assert not eng.runner.lp_active
