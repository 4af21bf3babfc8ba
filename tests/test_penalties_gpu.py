"""Sampler penalties on the GPU (csrc/kernels/penalties.hip): the three kernels against
``ops.reference.apply_penalties`` and a host model of the table, and the engine --
hipGraph decode, pipelined, and eager -- replayed step by step on the host from the raw
logit taps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from fasttalk_llm_microservice_amd import ops
from fasttalk_llm_microservice_amd.engine.config import EngineConfig
from fasttalk_llm_microservice_amd.engine.engine import LLMEngine
from fasttalk_llm_microservice_amd.engine.sampling_params import SamplingParams
from fasttalk_llm_microservice_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 8   # slots of the kernel tests
ENTRY_VALUES = np.array([1, 2, 7, 32767, 0x8000, 0x8001, 0x8000 | 32767, 0x8000 | 3], np.uint16)


def _state(vocab, seed):
    """Device state of S slots and its host mirror: sparse random entries (counts 0, 1,
    32767, prompt-only tokens, both), columns 0 and V-1 set in some slots; bias lists of
    0, 1 and 300 entries (slot % 3), ids 0 and V-1 among them."""
    rng = np.random.default_rng(seed)
    host = np.zeros((S, vocab), np.uint16)
    for s in range(S):
        cols = rng.choice(vocab, size=min(200, vocab // 3), replace=False)
        host[s, cols] = rng.choice(ENTRY_VALUES, size=cols.shape[0])
        if s % 2:
            host[s, 0], host[s, vocab - 1] = 0x8001, 32767
    table, bias_ids, bias_vals = ops.penalty_state(S, vocab, DEV)
    table.copy_(torch.from_numpy(host.view(np.int16)))
    hb_ids = np.full((S, ops.PEN_MAX_BIAS), -1, np.int32)
    hb_vals = np.zeros((S, ops.PEN_MAX_BIAS), np.float32)
    for s in range(S):
        n = (0, 1, ops.PEN_MAX_BIAS)[s % 3]
        if n == 1:
            hb_ids[s, 0] = (0, vocab - 1)[(s // 3) % 2]
        elif n:
            ids = rng.choice(np.arange(1, vocab - 1), size=n - 2, replace=False)
            hb_ids[s, :n] = np.concatenate([[vocab - 1], ids, [0]])
        hb_vals[s, :n] = rng.uniform(-100, 100, n).astype(np.float32)
    bias_ids.copy_(torch.from_numpy(hb_ids))
    bias_vals.copy_(torch.from_numpy(hb_vals))
    return (table, bias_ids, bias_vals), (host, hb_ids, hb_vals)


def _ulp(x: torch.Tensor, mant_bits: int) -> torch.Tensor:
    """Spacing of a format with ``mant_bits`` explicit mantissa bits at |x| (fp32 math)."""
    _, e = torch.frexp(x.abs().clamp_min(torch.finfo(torch.float32).tiny))
    return torch.ldexp(torch.ones_like(x), e - 1 - mant_bits)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("vocab", [128256, 1003])
@pytest.mark.parametrize("rows", [1, 5, 64])
def test_penalty_apply_matches_reference(rows, vocab, dtype):
    """The kernel and the reference may differ by FMA contraction and nothing else: fp32
    within 4 fp32 ulps of the largest magnitude among l, freq*c, pres and bias of the
    element, bf16 within 1 bf16 ulp; untouched elements and slot -1 rows keep their bits.
    Row stride > V, non-monotone slots with -1 rows, in place and out of place."""
    (table, bias_ids, bias_vals), (host, hb_ids, hb_vals) = _state(vocab, seed=rows + vocab)
    g = torch.Generator().manual_seed(rows * 7 + vocab)
    stride = (vocab + 7) // 8 * 8 + 64
    raw_h = (torch.randn(rows, stride, generator=g) * 4).to(dtype)
    raw_h[:, ::97] = 0.0
    slots_h = np.array([-1 if (r % 4 == 1) else (r * 5 + 3) % S for r in range(rows)], np.int32)
    rep_h = np.array([(1.3, 0.7, 1.0, 2.5)[r % 4] for r in range(rows)], np.float32)
    pres_h = np.array([(0.5, -1.25, 0.0, 2.0)[r % 4] for r in range(rows)], np.float32)
    freq_h = np.array([(1.0, 0.0, -2.0, 0.3)[(r + 1) % 4] for r in range(rows)], np.float32)
    logits_h = raw_h[:, :vocab]

    live = np.nonzero(slots_h >= 0)[0]
    want = logits_h.clone()
    e = torch.from_numpy(host[slots_h[live]].astype(np.int32))
    want[live] = ref.apply_penalties(
        logits_h[live], (e & 0x8000) != 0, e & 0x7FFF, torch.from_numpy(rep_h[live]),
        torch.from_numpy(pres_h[live]), torch.from_numpy(freq_h[live]),
        torch.from_numpy(hb_ids[slots_h[live]]), torch.from_numpy(hb_vals[slots_h[live]]))

    dev = [torch.from_numpy(a).to(DEV) for a in (slots_h, rep_h, pres_h, freq_h)]
    raw_d = raw_h.to(DEV)
    out = torch.full((rows, stride), 123.0, dtype=dtype, device=DEV)[:, :vocab]
    ops.penalty_apply(raw_d[:, :vocab], *dev, table, bias_ids, bias_vals, out=out)
    inplace = raw_d.clone()
    ops.penalty_apply(inplace[:, :vocab], *dev, table, bias_ids, bias_vals)
    torch.cuda.synchronize()
    got = out.cpu()
    bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
    assert torch.equal(inplace[:, :vocab].cpu().view(bits), got.view(bits)), "in place != out of place"
    assert torch.equal(inplace[:, vocab:].cpu().view(bits), raw_h[:, vocab:].view(bits)), "row padding written"

    # per-element tolerance
    c = torch.zeros(rows, vocab)
    c[live] = (e & 0x7FFF).float()
    biasv = torch.zeros(rows, vocab)
    touched = torch.zeros(rows, vocab, dtype=torch.bool)
    touched[live] = e != 0
    for r in live:
        ids = hb_ids[slots_h[r]]
        ok = ids >= 0
        biasv[r, ids[ok]] = torch.from_numpy(hb_vals[slots_h[r]][ok])
        touched[r, ids[ok]] = True
    lf = logits_h.float()
    if dtype == torch.float32:
        mag = torch.stack([lf.abs(), (torch.from_numpy(freq_h)[:, None] * c).abs(),
                           torch.from_numpy(pres_h).abs()[:, None].expand_as(lf),
                           biasv.abs()]).amax(0)
        tol = 4 * _ulp(mag, 23)
    else:
        tol = _ulp(want.float(), 7)
    diff = (got.float() - want.float()).abs()
    print(f"rows {rows} V {vocab} {dtype}: {int(touched.sum())} touched elements, "
          f"max |diff| {diff.max().item():.3e}, mismatching bits {int((got.view(bits) != want.view(bits)).sum())}")
    assert bool((diff <= tol).all()), (diff - tol).max()
    # stricter than the bound above: the kernel rounds every operation where the reference
    # does (no FMA contraction), so the results are equal in every bit
    assert torch.equal(got.view(bits), want.view(bits)), "kernel and reference differ in some bit"
    assert torch.equal(got.view(bits)[~touched], logits_h.view(bits)[~touched]), "untouched element changed"


def test_penalty_seed_and_update():
    """Seed clears exactly its slot's row and scatters the pairs; k updates count with
    saturation at 32767 and keep the prompt bit; a -1 row is untouched."""
    vocab = 1003
    table, bias_ids, bias_vals = ops.penalty_state(4, vocab, DEV)
    table.fill_(0x1234)
    ids = np.array([0, 5, 17, 1002, 400], np.int32)
    vals = np.array([0x8000, 32766, 0x8000 | 32766, 1, 3], np.int32)
    sb_ids = np.full(ops.PEN_MAX_BIAS, -1, np.int32)
    sb_vals = np.zeros(ops.PEN_MAX_BIAS, np.float32)
    sb_ids[:3], sb_vals[:3] = [1002, 0, 7], [1.5, -100.0, 100.0]
    dev = [torch.from_numpy(a).to(DEV) for a in (ids, vals)]
    ops.penalty_seed(table, 1, dev[0], dev[1], bias_ids, bias_vals,
                     torch.from_numpy(sb_ids).to(DEV), torch.from_numpy(sb_vals).to(DEV))
    want = np.full((4, vocab), 0x1234, np.uint16)
    want[1] = 0
    want[1, ids] = vals.astype(np.uint16)
    torch.cuda.synchronize()
    assert np.array_equal(table.cpu().numpy().view(np.uint16), want), "seed"
    assert np.array_equal(bias_ids.cpu().numpy()[1], sb_ids) and (bias_ids.cpu().numpy()[[0, 2, 3]] == -1).all()
    assert np.array_equal(bias_vals.cpu().numpy()[1], sb_vals)
    slots = torch.tensor([1, -1, 2, 0], dtype=torch.int32, device=DEV)
    for k in range(3):   # rows: saturating 32766 -> 32767, untouched, sentinel + 1, prompt bit kept
        ops.penalty_update(table, slots, torch.tensor([5, 5, 9, 0], dtype=torch.int32, device=DEV))
        ops.penalty_update(table, slots[:1], torch.tensor([17], dtype=torch.int32, device=DEV))
    want[1, 5] = 32767
    want[1, 17] = 0x8000 | 32767
    want[2, 9] = 0x1234 + 3
    want[0, 0] = 0x1234 + 3
    torch.cuda.synchronize()
    assert np.array_equal(table.cpu().numpy().view(np.uint16), want), "update"


# ------------------------------------------------------------------------------- engine
PEN_PARAMS = [dict(repetition_penalty=1.3, frequency_penalty=1.0),
              dict(presence_penalty=1.5, logit_bias={"17": 4.0, 90001: -50.0}),
              dict(repetition_penalty=0.8, frequency_penalty=-0.5, presence_penalty=0.25),
              dict(frequency_penalty=2.0), None, None]
LENS = [14, 9, 12, 7, 11, 8]


def _engine(**kw):
    base = dict(model="tiny", device="cuda", num_kv_blocks=256, max_model_len=512, max_num_seqs=8,
                graph_batch_sizes=(1, 2, 4, 8))
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def _prompts():
    rng = np.random.default_rng(3)
    return [rng.integers(0, 120000, n).tolist() for n in (12, 20, 9, 17, 15, 11)]


def _run(eng, prompts, params):
    r = eng.runner
    r.logits_tap, r.logits_tap_ids = [], []
    res = {}
    for i, (p, sp) in enumerate(zip(prompts, params)):
        eng.add_request(f"r{i}", p, sp, on_output=lambda o, i=i: res.setdefault(i, []).extend(o.token_ids))
    while eng.has_work():
        eng.step()
    tap = {}
    for logits, ids in zip(r.logits_tap, r.logits_tap_ids):
        for row, rid in enumerate(ids or []):
            tap.setdefault(rid, []).append(logits[row].float().cpu())
    r.logits_tap = r.logits_tap_ids = None
    return res, tap


def _replay(prompt, out, taps, sp, dtype):
    """Per step: (reference-penalised logit of the emitted token, row max, raw argmax)
    from the raw tap and the host's history."""
    v = taps[0].shape[0]
    pm = torch.zeros(1, v, dtype=torch.bool)
    pm[0, prompt] = True
    counts = torch.zeros(1, v, dtype=torch.int32)
    bias = sp.logit_bias or {}
    bi = torch.tensor([list(bias.keys())], dtype=torch.int32).reshape(1, -1)
    bv = torch.tensor([list(bias.values())], dtype=torch.float32).reshape(1, -1)
    rows = []
    for k, tok in enumerate(out):
        raw = taps[k].to(dtype).view(1, v)
        pen = ref.apply_penalties(raw, pm, counts, [sp.repetition_penalty], [sp.presence_penalty],
                                  [sp.frequency_penalty], bi, bv).float()[0]
        rows.append((pen[tok].item(), pen.max().item(), int(raw.float().argmax())))
        counts[0, tok] += 1
    return rows


@pytest.mark.parametrize("model,invariant", [("tiny", False), ("tiny-2k", True)],
                         ids=["tiny", "tiny2k-invariant"])
@pytest.mark.parametrize("eager", [False, True], ids=["graphs", "eager"])
def test_engine_penalties_replayed_on_the_host(eager, model, invariant, monkeypatch):
    """Six concurrent greedy requests of different lengths, four penalised.  Every step
    of a penalised request, replayed on the host (reference penalties over the raw tap and
    the host's history), puts the emitted token within 2 bf16 ulps of the row's maximum;
    the device tables verify at every finish; the unpenalised requests emit what they
    emit in an engine started without penalties.  On the GPU a row's bf16 rounding
    depends on the shape of the steps it shares, so "alone" is compared bit for bit only
    in batch-invariant mode (``tiny-2k``: the mode needs its hidden size); the default
    mode compares with the same six requests run unpenalised in steps of the same shapes."""
    monkeypatch.setenv("FT_PENALTY_VERIFY", "1")
    prompts = _prompts()
    params = [SamplingParams(temperature=0.0, max_tokens=n, ignore_eos=True, **(kw or {}))
              for n, kw in zip(LENS, PEN_PARAMS)]
    cfg = dict(model=model, enforce_eager=eager, batch_invariant=invariant,
               enable_prefix_caching=False)
    eng = _engine(**cfg)
    res, tap = _run(eng, prompts, params)
    assert [len(res[i]) for i in range(6)] == LENS
    st = eng.runner.stats
    if eager:
        assert st["graph_replays"] == 0
    else:
        assert st["graph_replays"] > 0 and eng.stats["pipelined_steps"] > 0
        assert any(pen for _, pen in eng.runner.graphs), list(eng.runner.graphs)
    assert eng.stats["penalty_verified"] == 4 and eng.metrics()["penalty_steps"] > 0
    assert eng.metrics()["penalty_slots_in_use"] == 0 and len(eng._pen_free) == 8
    differs = 0
    for i in range(4):
        rows = _replay(prompts[i], res[i], tap[f"r{i}"], params[i], eng.runner.dtype)
        for k, (lt, lmax, raw_arg) in enumerate(rows):
            ulp = _ulp(torch.tensor(lmax), 7).item()
            assert lmax - lt <= 2 * ulp, (i, k, lt, lmax)
            differs += raw_arg != res[i][k]
    print(f"{model} eager={eager}: {differs} emitted tokens differ from the raw argmax")
    assert differs >= 1
    monkeypatch.setenv("ENGINE_PENALTIES", "0")
    off = _engine(**cfg)
    assert off.runner.pen_table is None
    if invariant:
        alone, _ = _run(off, prompts[4:], params[4:])
        assert [alone[0], alone[1]] == [res[4], res[5]]
    else:
        bare = [SamplingParams(temperature=0.0, max_tokens=n, ignore_eos=True) for n in LENS]
        same, _ = _run(off, prompts, bare)
        assert [same[4], same[5]] == [res[4], res[5]]


def test_engine_guided_rows_and_penalties(monkeypatch):
    """A bound json_schema request gives the same text with and without penalties (its
    rows carry no slot); a lazy-guided request whose reply is free text is penalised and
    verified like any other."""
    from fasttalk_llm_microservice_amd.engine.guided import GuidedSpec, tool_call_ast

    monkeypatch.setenv("FT_PENALTY_VERIFY", "1")
    spec = GuidedSpec.json_schema({"type": "object", "properties": {
        "city": {"type": "string", "maxLength": 8}, "n": {"type": "integer"}},
        "required": ["city", "n"]})
    tools = [{"type": "function", "function": {"name": "get_current_time",
                                               "parameters": {"type": "object", "properties": {}}}}]
    pen = dict(repetition_penalty=1.4, frequency_penalty=1.0, logit_bias={5: 3.0})
    prompts = _prompts()
    eng = _engine(enable_prefix_caching=False)   # both runs prefill the same chunks
    brace = eng.tokenizer.encode("{")[0]

    def run(with_pen):
        kw = pen if with_pen else {}
        params = [SamplingParams(temperature=0.0, max_tokens=40, guided=spec, **kw),
                  # the lazy grammar cannot bind: '{' is biased away on the first token
                  SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True, guided_lazy=True,
                                 guided=GuidedSpec(tool_call_ast(tools)),
                                 **(dict(pen, logit_bias={brace: -100.0}) if with_pen else {})),
                  SamplingParams(temperature=0.0, max_tokens=10, ignore_eos=True, **kw)]
        return _run(eng, prompts[:3], params)[0]

    plain = run(False)
    before = eng.stats["penalty_verified"]
    got = run(True)
    assert got[0] == plain[0], "a bound grammar's rows must not be penalised"
    json.loads(eng.tokenizer.decode(got[0]))
    assert len(got[1]) == 12 and brace not in got[1][:1]
    assert eng.stats["penalty_verified"] - before == 2   # the lazy free-text row and the plain one
    assert eng.metrics()["penalty_slots_in_use"] == 0


def test_more_penalised_requests_than_slots(monkeypatch):
    """Ten penalised requests over four slots on the default pipelined path (graphs, mixed
    steps chained): a prompt completed by a queued mixed step counts against max_num_seqs,
    so no step needs a fifth slot; every table verifies at its finish."""
    monkeypatch.setenv("FT_PENALTY_VERIFY", "1")
    eng = _engine(max_num_seqs=4, graph_batch_sizes=(1, 2, 4))
    rng = np.random.default_rng(11)
    prompts = [rng.integers(0, 120000, 8 + i).tolist() for i in range(10)]
    params = [SamplingParams(temperature=0.0, max_tokens=6 + 2 * (i % 3), ignore_eos=True,
                             repetition_penalty=1.2, frequency_penalty=0.5) for i in range(10)]
    res, _ = _run(eng, prompts, params)
    assert [len(res[i]) for i in range(10)] == [p.max_tokens for p in params]
    assert eng.stats["penalty_verified"] == 10 and sorted(eng._pen_free) == [0, 1, 2, 3]
    assert eng.runner.stats["graph_replays"] > 0 and eng.runner.stats["eager_decode"] == 0


def test_no_penalised_request_launches_nothing_new():
    eng = _engine()
    params = [SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True) for _ in range(3)]
    _run(eng, _prompts()[:3], params)
    assert eng.metrics()["penalty_steps"] == 0 and eng.runner.stats["graph_replays"] > 0
    assert eng.runner.graphs and not any(pen for _, pen in eng.runner.graphs)
    assert not any(pen for _, pen in eng.runner.graphs_split)


def test_checked_build_passes_this_file():
    """The bounds-checked kernel build (FT_KERNEL_CHECKS=1: slot < S, token / bias id < V)
    runs the tests above in a child process without a violation."""
    env = dict(os.environ, FT_KERNEL_CHECKS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "not checked_build", os.path.abspath(__file__)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-2000:]
