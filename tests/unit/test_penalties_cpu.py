"""Sampler penalties on the CPU backend: SamplingParams validation, the fp32 reference
``ops.reference.apply_penalties`` on hand-computed examples, the tiny CPU engine
replayed step by step on the host, and the life cycle of the state slots."""
import json

import numpy as np
import pytest
import torch

from fasttalk_llm_microservice_amd.engine.config import EngineConfig
from fasttalk_llm_microservice_amd.engine.engine import EngineError, LLMEngine
from fasttalk_llm_microservice_amd.engine.sampling_params import SamplingParams
from fasttalk_llm_microservice_amd.ops import reference as ref


# ------------------------------------------------------------------------- SamplingParams
def test_defaults_have_no_penalties():
    sp = SamplingParams()
    assert (sp.repetition_penalty, sp.presence_penalty, sp.frequency_penalty, sp.logit_bias) == \
        (1.0, 0.0, 0.0, None)
    assert not sp.has_penalties


@pytest.mark.parametrize("kw", [dict(repetition_penalty=1.1), dict(presence_penalty=-2.0),
                                dict(frequency_penalty=2.0), dict(logit_bias={"5": 1})])
def test_has_penalties(kw):
    assert SamplingParams(**kw).has_penalties


@pytest.mark.parametrize("kw", [
    dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(presence_penalty=2.01),
    dict(presence_penalty=-2.01), dict(frequency_penalty=3), dict(frequency_penalty=-2.5),
    dict(logit_bias={"5": 100.5}), dict(logit_bias={5: -101}), dict(logit_bias={"x": 1.0}),
    dict(logit_bias={-3: 1.0}), dict(logit_bias={i: 1.0 for i in range(301)}),
    dict(logit_bias=[1, 2]), dict(logit_bias={"7": 1.0, 7: 2.0})])
def test_out_of_range_values_raise(kw):
    with pytest.raises(ValueError):
        SamplingParams(**kw)


def test_bounds_and_bias_keys_are_accepted():
    sp = SamplingParams(repetition_penalty=1e-3, presence_penalty=2, frequency_penalty=-2,
                        logit_bias={"12": 100, 7: -100.0, **{1000 + i: 0.5 for i in range(298)}})
    assert sp.logit_bias[12] == 100.0 and sp.logit_bias[7] == -100.0 and len(sp.logit_bias) == 300
    assert all(isinstance(k, int) for k in sp.logit_bias)
    assert SamplingParams(logit_bias={}).logit_bias is None


# ------------------------------------------------------------------------------ reference
def _ref(l, prompt, counts, rep=1.0, pres=0.0, freq=0.0, bias=None, dtype=torch.float32):
    l = torch.tensor([l], dtype=dtype)
    pm = torch.zeros(1, 8, dtype=torch.bool)
    pm[0, prompt] = True
    bi = torch.tensor([list((bias or {}).keys()) + [-1]], dtype=torch.int32)
    bv = torch.tensor([list((bias or {}).values()) + [9.0]], dtype=torch.float32)
    return ref.apply_penalties(l, pm, torch.tensor([counts], dtype=torch.int32), [rep], [pres],
                               [freq], bi, bv)[0]


L8 = [2.0, -2.0, 4.0, -1.0, 0.5, 3.0, -3.0, 1.0]


def test_reference_repetition_on_prompt_and_output_tokens():
    # token 0 (prompt, > 0) / 2, token 1 (prompt, < 0) * 2, token 2 (output) / 2, token 3 (output) * 2
    out = _ref(L8, prompt=[0, 1], counts=[0, 0, 1, 3, 0, 0, 0, 0], rep=2.0)
    assert out.tolist() == [1.0, -4.0, 2.0, -2.0, 0.5, 3.0, -3.0, 1.0]


def test_reference_frequency_and_presence_on_output_tokens_only():
    out = _ref(L8, prompt=[0, 1], counts=[0, 0, 1, 3, 0, 0, 0, 0], pres=0.5, freq=0.25)
    assert out.tolist() == [2.0, -2.0, 4.0 - 0.75, -1.0 - 1.25, 0.5, 3.0, -3.0, 1.0]


def test_reference_bias_and_padding():
    out = _ref(L8, prompt=[], counts=[0] * 8, bias={7: -100.0, 0: 1.5})
    assert out.tolist() == [3.5, -2.0, 4.0, -1.0, 0.5, 3.0, -3.0, -99.0]


def test_reference_order_repetition_then_frequency_then_bias():
    # token 2: (4 / 2) - (1 * 2 + 0.5) + 10 = 9.5 ; in another order it would be 5.75 or 15.75
    # token 6: (-3 * 2) - (1 * 3 + 0.5) + 0 = -9.5
    out = _ref(L8, prompt=[2], counts=[0, 0, 2, 0, 0, 0, 3, 0], rep=2.0, pres=0.5, freq=1.0,
               bias={2: 10.0})
    assert out.tolist() == [2.0, -2.0, 9.5, -1.0, 0.5, 3.0, -9.5, 1.0]


def test_reference_rounds_once_to_the_logits_dtype():
    # 1.0078125 / 3 - 1/3 of a bf16 ulp apart: fp32 math then ONE rounding to bf16
    l = [1.0078125] + [0.0] * 7
    out = _ref(l, prompt=[0], counts=[0] * 8, rep=3.0, bias={0: 0.001}, dtype=torch.bfloat16)
    want = torch.tensor(np.float32(np.float32(1.0078125) / np.float32(3.0)) + np.float32(0.001)).bfloat16()
    assert out.dtype == torch.bfloat16 and out[0] == want
    assert torch.equal(out[1:], torch.zeros(7, dtype=torch.bfloat16))


# --------------------------------------------------------------------------------- engine
PROMPTS = [[(7 * i + 3 * j) % 5000 + 10 for j in range(n)] for i, n in enumerate((9, 14, 6, 11))]


def _engine(**kw):
    base = dict(model="tiny", device="cpu", max_num_seqs=4, max_model_len=256)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


@pytest.fixture(scope="module")
def eng():
    import os

    old = os.environ.get("FT_PENALTY_VERIFY")
    os.environ["FT_PENALTY_VERIFY"] = "1"
    try:
        yield _engine()
    finally:
        if old is None:
            os.environ.pop("FT_PENALTY_VERIFY", None)
        else:
            os.environ["FT_PENALTY_VERIFY"] = old


@pytest.fixture(scope="module")
def plain(eng):
    """The unpenalised greedy run every engine test compares against (computed once)."""
    return eng.generate(PROMPTS, SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True))


def test_logit_bias_forces_and_bans_a_token(eng, plain):
    t = 4242
    out = eng.generate(PROMPTS[:2], SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True,
                                                    logit_bias={t: 100}))
    assert out == [[t] * 8, [t] * 8]
    g = plain[0][0]
    out = eng.generate(PROMPTS[:1], SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True,
                                                    logit_bias={str(g): -100}))[0]
    assert g not in out and len(out) == 24


def test_engine_steps_replay_on_the_host(eng, plain):
    """repetition 1.3 + frequency 1.0: the argmax of the reference penalties over each
    step's raw logits and the host's history is the emitted token, at every step, and the
    penalties change at least one token (greedy ``tiny`` repeats heavily)."""
    sp = SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True, repetition_penalty=1.3,
                        frequency_penalty=1.0)
    r = eng.runner
    before = eng.stats["penalty_verified"]
    r.logits_tap, r.logits_tap_ids = [], []
    res = {}
    for i, p in enumerate(PROMPTS):
        eng.add_request(f"rp{i}", p, SamplingParams(**sp.__dict__),
                        on_output=lambda o, i=i: res.setdefault(i, []).extend(o.token_ids))
    while eng.has_work():
        eng.step()
    tap = {}
    for logits, ids in zip(r.logits_tap, r.logits_tap_ids):
        for row, rid in enumerate(ids or []):
            tap.setdefault(rid, []).append(logits[row])
    r.logits_tap = r.logits_tap_ids = None
    assert eng.stats["penalty_verified"] - before == 4
    differs = 0
    for i, p in enumerate(PROMPTS):
        v = tap[f"rp{i}"][0].shape[0]
        pm = torch.zeros(1, v, dtype=torch.bool)
        pm[0, p] = True
        counts = torch.zeros(1, v, dtype=torch.int32)
        assert len(res[i]) == 24 == len(tap[f"rp{i}"])
        for k, tok in enumerate(res[i]):
            raw = tap[f"rp{i}"][k].view(1, v)
            pen = ref.apply_penalties(raw, pm, counts, [1.3], [0.0], [1.0])
            assert int(pen.argmax()) == tok, (i, k)
            differs += int(raw.argmax()) != tok
            counts[0, tok] += 1
    assert differs >= 1
    assert [res[i] for i in range(4)] != plain


def test_slot_lifecycle_with_mixed_requests_and_a_preemption(monkeypatch):
    """12 requests over 4 slots, some without penalties, different lengths, and a KV pool
    small enough to force a recompute preemption: every penalised request's table is
    verified against the host at its finish, and every slot comes back."""
    monkeypatch.setenv("FT_PENALTY_VERIFY", "1")
    eng = _engine(num_kv_blocks=9, block_size=16, swap_space_gb=0.0, enable_prefix_caching=False)
    kinds = [dict(repetition_penalty=1.2), None, dict(frequency_penalty=0.7, presence_penalty=0.3),
             dict(logit_bias={11: 5.0, "12": -5.0})]
    done = {}
    n_pen = 0
    for i in range(12):
        kw = kinds[i % 4]
        n_pen += kw is not None
        p = [(11 * i + j) % 3000 + 5 for j in range(10 + i)]
        eng.add_request(f"q{i}", p, SamplingParams(temperature=0.0, max_tokens=14 + 3 * (i % 5),
                                                   ignore_eos=True, **(kw or {})),
                        on_output=lambda o: done.__setitem__(o.request_id, o) if o.finished else None)
    for _ in range(5000):
        if not eng.has_work():
            break
        eng.step()
        assert len(eng._pen_owner) + len(eng._pen_free) == 4
        # prompts completed by queued mixed steps count against max_num_seqs
        assert len(eng.scheduler.running) <= 4
    assert len(done) == 12 and all(o.finish_reason == "length" for o in done.values())
    assert eng.scheduler.num_preemptions > eng.scheduler.num_swap_out, "no recompute preemption"
    assert eng.stats["penalty_verified"] == n_pen == 9
    assert sorted(eng._pen_free) == [0, 1, 2, 3] and not eng._pen_owner
    assert eng.metrics()["penalty_slots_in_use"] == 0 and eng.metrics()["penalty_steps"] > 0


def test_abort_returns_the_slot(eng):
    eng.add_request("ab", PROMPTS[0], SamplingParams(max_tokens=50, ignore_eos=True,
                                                     repetition_penalty=1.5))
    for _ in range(3):
        eng.step()
    assert eng.metrics()["penalty_slots_in_use"] == 1
    assert eng.abort("ab")
    assert eng.metrics()["penalty_slots_in_use"] == 0 and len(eng._pen_free) == 4
    while eng.has_work():
        eng.step()


def test_guided_bound_rows_are_not_penalised_and_lazy_free_text_is(eng):
    from fasttalk_llm_microservice_amd.engine.guided import GuidedSpec, tool_call_ast

    spec = GuidedSpec.json_schema({"type": "object", "properties": {
        "city": {"type": "string", "maxLength": 8}, "n": {"type": "integer"}},
        "required": ["city", "n"]})
    pen = dict(repetition_penalty=1.4, frequency_penalty=1.0, logit_bias={5: 3.0})
    base = dict(temperature=0.0, max_tokens=40, guided=spec)
    a = eng.generate(PROMPTS[:1], SamplingParams(**base))[0]
    before = eng.stats["penalty_verified"]
    b = eng.generate(PROMPTS[:1], SamplingParams(**base, **pen))[0]
    assert a == b and eng.stats["penalty_verified"] == before   # no slot was ever held
    json.loads(eng.tokenizer.decode(b))
    # lazy grammar, free-text reply ('{' is biased away): penalised like any other row
    tools = [{"type": "function", "function": {"name": "get_current_time",
                                               "parameters": {"type": "object", "properties": {}}}}]
    brace = eng.tokenizer.encode("{")[0]
    sp = SamplingParams(temperature=0.0, max_tokens=16, ignore_eos=True, guided_lazy=True,
                        guided=GuidedSpec(tool_call_ast(tools)), frequency_penalty=2.0,
                        logit_bias={brace: -100.0})
    out = eng.generate(PROMPTS[1:2], sp)[0]
    assert len(out) == 16 and eng.stats["penalty_verified"] == before + 1
    assert eng.stats["lazy_grammar_bound"] == 0
    assert max(np.bincount(out)) <= 2, "frequency_penalty 2.0 leaves no heavy repetition"


def test_lazy_grammar_that_binds_gives_its_slot_back(eng):
    from fasttalk_llm_microservice_amd.engine.guided import GuidedSpec, tool_call_ast

    tools = [{"type": "function", "function": {"name": "get_current_time",
                                               "parameters": {"type": "object", "properties": {}}}}]
    brace = eng.tokenizer.encode("{")[0]
    sp = SamplingParams(temperature=0.0, max_tokens=40, guided_lazy=True,
                        guided=GuidedSpec(tool_call_ast(tools)), repetition_penalty=1.2,
                        logit_bias={brace: 100.0})
    out = eng.generate(PROMPTS[2:3], sp)[0]
    assert eng.stats["lazy_grammar_bound"] >= 1
    assert json.loads(eng.tokenizer.decode(out)) == {"name": "get_current_time", "parameters": {}}
    assert eng.metrics()["penalty_slots_in_use"] == 0 and len(eng._pen_free) == 4


def test_refusals(monkeypatch):
    e1 = _engine()
    with pytest.raises(ValueError, match="vocabulary"):
        e1.add_request("v", [1, 2, 3], SamplingParams(logit_bias={e1.model_cfg.vocab_size: 1.0}))
    e1.add_request("ok", [1, 2, 3], SamplingParams(logit_bias={e1.model_cfg.vocab_size - 1: 1.0},
                                                   max_tokens=1))
    e1.cfg.tp_size = 2
    with pytest.raises(EngineError, match="penalties are not supported with tensor parallelism yet"):
        e1.add_request("tp", [1, 2, 3], SamplingParams(presence_penalty=0.5))
    e1.add_request("tp-plain", [1, 2, 3], SamplingParams(max_tokens=1))
    monkeypatch.setenv("ENGINE_PENALTIES", "0")
    off = _engine()
    assert off.runner.pen_table is None and off.cfg.penalties is False
    with pytest.raises(EngineError, match="penalties are off"):
        off.add_request("p", [1, 2, 3], SamplingParams(repetition_penalty=1.1))
    assert off.generate([[1, 2, 3]], SamplingParams(temperature=0.0, max_tokens=3)) is not None


def test_reset_inflight_reseeds_live_slots(eng):
    """Dropping the queued steps (a failed step) sets every live slot back to the host's
    truth: the tokens those steps had counted are gone from the table, and the sequence
    still verifies at its finish."""
    before = eng.stats["penalty_verified"]
    res = []
    eng.add_request("rs", PROMPTS[3], SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True,
                                                     frequency_penalty=1.5),
                    on_output=lambda o: res.extend(o.token_ids))
    for _ in range(4):
        eng.step()
    seq = eng.scheduler.by_id["rs"]
    slot = seq.pen_slot
    assert slot >= 0
    # a token the host never saw, as a dropped step would have left it
    eng.runner.pen_table[slot, 77] = 5
    eng.reset_inflight()
    row = eng.runner.pen_read(slot)
    assert row[77] == 0 and int((row & 0x7FFF).sum()) == seq.num_output
    while eng.has_work():
        eng.step()
    assert len(res) == 12 and eng.stats["penalty_verified"] == before + 1


def test_more_penalised_requests_waiting_than_slots(monkeypatch):
    """Every request penalised, three times as many as slots, memory to spare, mixed steps
    chained (the default): prompts completed by a queued mixed step count against
    max_num_seqs, so no step ever needs a fifth slot or runs a fifth sequence."""
    monkeypatch.setenv("FT_PENALTY_VERIFY", "1")
    eng = _engine(num_kv_blocks=64, block_size=16)
    assert eng.mixed_chain
    done = []
    for i in range(12):
        eng.add_request(f"w{i}", [(13 * i + j) % 3000 + 5 for j in range(10 + i)],
                        SamplingParams(temperature=0.0, max_tokens=10 + 2 * (i % 4), ignore_eos=True,
                                       repetition_penalty=1.2),
                        on_output=lambda o: done.append(o.finish_reason) if o.finished else None)
    for _ in range(5000):
        if not eng.has_work():
            break
        eng.step()
        assert len(eng.scheduler.running) <= 4 and len(eng._pen_owner) <= 4
    assert done == ["length"] * 12 and eng.stats["penalty_verified"] == 12
    assert sorted(eng._pen_free) == [0, 1, 2, 3]
