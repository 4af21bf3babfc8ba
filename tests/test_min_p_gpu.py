"""min_p in the HIP sampler (csrc/kernels/sampling.hip) and through the engine: a token
is kept iff p >= min_p * p_max after mask and temperature, and top-k / top-p work on the
kept set.  Every fixture value is exact in bf16 and every threshold lies midway between
two logit values, so nothing here depends on the last ulp.

Tolerance of every empirical-versus-expected check: 0.02 maximum absolute deviation at
8,192 seeded draws (standard deviation <= 0.0055)."""
import json
import math

import numpy as np
import pytest
import torch

from fasttalk_llm_microservice_amd import ops
from fasttalk_llm_microservice_amd.engine.config import EngineConfig
from fasttalk_llm_microservice_amd.engine.engine import LLMEngine
from fasttalk_llm_microservice_amd.engine.sampling_params import SamplingParams

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEG_INF = float("-inf")
TOL = 0.02
ROWS, STEPS = 2048, 4

V = 128256
SL = 4008                    # ids per vocabulary slice (32 slices)
M = 4.0
# six head ids in five slices, one the last id of the last slice
HEAD = [17, 3 * SL + 1001, 9 * SL + 5, 9 * SL + 3000, 20 * SL + SL - 1, V - 1]
HEAD_VAL = [M - 0.5 * i for i in range(6)]
LOW = [SL + 7, 15 * SL + 123, 31 * SL + 9]     # three ids at M - 3
BULK = M - 12.0
LNMP = -2.75                 # threshold M - 2.75: midway between M - 2.5 and M - 3


def _row(v=V):
    x = torch.full((v,), BULK)
    x[HEAD] = torch.tensor(HEAD_VAL)
    x[LOW] = M - 3.0
    return x


def _softmax_over(vals):
    e = np.exp(np.asarray(vals, np.float64) - max(vals))
    return e / e.sum()


def _draws(row, dtype=torch.bfloat16, temp=1.0, top_p=1.0, top_k=0, lnmp=LNMP, mask_off=(),
           rows=ROWS, steps=STEPS):
    """Counts per id of rows x steps seeded draws over copies of ``row``; every call is
    repeated with the same (seed, step) and must reproduce its tokens."""
    v = row.numel()
    logits = row.to(DEV).to(dtype).unsqueeze(0).repeat(rows, 1)
    t = torch.full((rows,), temp, device=DEV)
    p = torch.full((rows,), top_p, device=DEV)
    k = torch.full((rows,), top_k, dtype=torch.int32, device=DEV)
    s = torch.arange(rows, dtype=torch.int64, device=DEV) * 7919 + 11
    mp = torch.full((rows,), lnmp, device=DEV)
    mask = None
    if mask_off:
        m = np.full((v + 31) // 32, -1, np.int64)
        for i in mask_off:
            m[i // 32] &= ~(1 << (i % 32))
        m = (m & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        mask = torch.from_numpy(m).to(DEV).unsqueeze(0).repeat(rows, 1)
    counts = torch.zeros(v)
    for step in range(steps):
        st = torch.full((rows,), step, dtype=torch.int32, device=DEV)
        out = ops.sample(logits, t, p, k, s, st, mask=mask, min_p=mp)
        assert torch.equal(out, ops.sample(logits, t, p, k, s, st, mask=mask, min_p=mp))
        counts += torch.bincount(out.long().cpu(), minlength=v).float()
    return counts


def _check(counts, ids, probs, what=""):
    expect = torch.zeros(counts.numel(), dtype=torch.float64)
    expect[list(ids)] = torch.as_tensor(np.asarray(probs, np.float64))
    emp = (counts / counts.sum()).double()
    outside = counts.clone()
    outside[list(ids)] = 0
    print(what, "emp", [round(float(emp[i]), 4) for i in ids], "expect",
          [round(float(q), 4) for q in probs], "outside", int(outside.sum()))
    assert outside.sum() == 0, (what, torch.nonzero(outside).flatten()[:10].tolist())
    assert all(counts[i] > 0 for i in ids), what
    assert (emp - expect).abs().max().item() < TOL, what


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_kept_set_and_distribution(dtype):
    """No top-k, top_p = 1 (multi-workgroup path + the min_p slice kernel): the draws are
    softmax over the six head ids; the bulk, which an unfiltered draw hits a quarter of
    the time, and the three ids just below the threshold never appear."""
    _check(_draws(_row(), dtype), HEAD, _softmax_over(HEAD_VAL), f"kept {dtype}")


def test_min_p_before_top_p():
    """top_p = 0.5 over the kept set (Z = 2.415) is the first two ids; over the
    unfiltered row (Z = 3.35) it would be three."""
    _check(_draws(_row(), top_p=0.5), HEAD[:2], _softmax_over(HEAD_VAL[:2]), "top_p 0.5")


@pytest.mark.parametrize("top_k,n", [(8, 6), (100, 6), (3, 3)], ids=["mw8", "onewg100", "mw3"])
def test_top_k_and_min_p_intersect(top_k, n):
    """top_k = 8: the multi-workgroup top-k path holds the six head ids and the three
    tied ids below the threshold, which leave before Z and the ranks; top_k = 100: the
    one-workgroup kernel; top_k = 3: the first three."""
    _check(_draws(_row(), top_k=top_k), HEAD[:n], _softmax_over(HEAD_VAL[:n]), f"top_k {top_k}")


def test_one_workgroup_nucleus_fallback():
    """V = 4,096, 64 descending head logits on a 0.0625 grid, min_p keeps 40 of them,
    top_p = 0.3: about a quarter of the rows has all four candidates rejected and is
    finished by the one-workgroup kernel (rejection rounds, then the exact nucleus
    search), which must recompute the same threshold."""
    v = 4096
    ids = [(61 * i + 7) % v for i in range(64)]
    vals = [M - 0.0625 * i for i in range(64)]
    row = torch.full((v,), BULK)
    row[ids] = torch.tensor(vals)
    lnmp = -39.5 * 0.0625            # between the 40th and the 41st head value
    pk = _softmax_over(vals[:40])
    above = np.cumsum(pk) - pk
    n = int((above < 0.3).sum())
    assert abs(above[n - 1] - 0.3) > 1e-3 and (n == 40 or abs(above[n] - 0.3) > 1e-3)
    _check(_draws(row, top_p=0.3, lnmp=lnmp), ids[:n], pk[:n] / pk[:n].sum(), "fallback")


@pytest.mark.parametrize("top_k", [0, 8, 100], ids=["notopk", "mw8", "onewg100"])
def test_mask_comes_first(top_k):
    """The allow-mask forbids the global max and the id at M - 1.5: the kept set is
    measured from the allowed max M' = M - 0.5, threshold M' - 2.25 (midway between
    M' - 2 and M' - 2.5), so {M', M' - 0.5, M' - 1.5, M' - 2} stay."""
    keep = [1, 2, 4, 5]
    c = _draws(_row(), top_k=top_k, lnmp=-2.25, mask_off=(HEAD[0], HEAD[3]))
    assert c[HEAD[0]] == 0 and c[HEAD[3]] == 0
    _check(c, [HEAD[i] for i in keep], _softmax_over([HEAD_VAL[i] for i in keep]), "mask")


@pytest.mark.parametrize("top_k,top_p", [(0, 0.9), (0, 1.0), (8, 0.9), (100, 0.9)],
                         ids=["topp", "plain", "mw8", "onewg100"])
def test_off_rows_are_untouched(top_k, top_p):
    """Odd rows off (-inf), even rows on, in one call: the odd rows' tokens are those of
    the call without a min_p tensor; a tensor that is off everywhere equals None."""
    rows = 64
    torch.manual_seed(5)
    logits = (torch.randn(rows, V, device=DEV) * 2).bfloat16()
    t = torch.full((rows,), 0.9, device=DEV)
    p = torch.full((rows,), top_p, device=DEV)
    k = torch.full((rows,), top_k, dtype=torch.int32, device=DEV)
    s = torch.arange(rows, dtype=torch.int64, device=DEV) * 104729 + 5
    st = torch.full((rows,), 3, dtype=torch.int32, device=DEV)
    base = ops.sample(logits, t, p, k, s, st, min_p=None)
    off = torch.full((rows,), NEG_INF, device=DEV)
    assert torch.equal(ops.sample(logits, t, p, k, s, st, min_p=off), base)
    mixed = off.clone()
    mixed[0::2] = math.log(0.5)
    got = ops.sample(logits, t, p, k, s, st, min_p=mixed)
    assert torch.equal(got[1::2], base[1::2])
    x = logits.float()
    thr = x.max(-1).values + t * mixed
    assert bool((x.gather(1, got.long().view(-1, 1)).flatten() >= thr).all())


@pytest.mark.parametrize("top_k", [0, 8, 100], ids=["notopk", "mw8", "onewg100"])
def test_min_p_one_keeps_the_tied_maxima(top_k):
    ties = [5, 11 * SL + 77, V - 3]
    row = torch.full((V,), M - 0.0625)
    row[ties] = M
    c = _draws(row, top_k=top_k, lnmp=0.0)
    _check(c, ties, [1 / 3] * 3, "min_p = 1")


def test_greedy_rows_ignore_min_p():
    rows = 16
    torch.manual_seed(6)
    logits = torch.randn(rows, V, device=DEV).bfloat16()
    z = torch.zeros(rows, device=DEV)
    k = torch.zeros(rows, dtype=torch.int32, device=DEV)
    k[8:] = 8
    s = torch.arange(rows, dtype=torch.int64, device=DEV)
    out = ops.sample(logits, z, z + 1.0, k, s, k * 0, min_p=z + math.log(0.2))
    assert torch.equal(out.long(), logits.float().argmax(-1))


# ------------------------------------------------------------------------------- engine
MIN_P = 0.3


def _engine(**kw):
    base = dict(model="tiny", device="cuda", num_kv_blocks=256, max_model_len=512, max_num_seqs=8,
                graph_batch_sizes=(1, 2, 4, 8), enable_prefix_caching=False)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def _prompts():
    rng = np.random.default_rng(3)
    return [rng.integers(0, 120000, n).tolist() for n in (12, 20)]


def _run(eng, prompts, params):
    """({i: token ids}, {request id: [raw logits per step]})"""
    r = eng.runner
    r.logits_tap, r.logits_tap_ids = [], []
    toks = {}
    for i, (p, sp) in enumerate(zip(prompts, params)):
        eng.add_request(f"r{i}", p, sp,
                        on_output=lambda o, i=i: toks.setdefault(i, []).extend(o.token_ids))
    while eng.has_work():
        eng.step()
    tap = {}
    for logits, ids in zip(r.logits_tap, r.logits_tap_ids):
        for row, rid in enumerate(ids or []):
            tap.setdefault(rid, []).append(logits[row].float().cpu())
    r.logits_tap = r.logits_tap_ids = None
    return toks, tap


def _within(toks, taps):
    """Every sampled token: logit >= max + ln(min_p) on that step's tapped logits, after
    bf16 rounding (temperature 1)."""
    assert len(toks) <= len(taps)
    lim = torch.tensor(math.log(MIN_P), dtype=torch.float32)
    for k, tok in enumerate(toks):
        x = taps[k].bfloat16().float()
        assert x[tok] >= x.max() + lim, (k, tok, float(x[tok]), float(x.max()))


def _mp_variants(r):
    return [k for k in list(r.graphs) + list(r.graphs_split) if len(k) == 3]


def test_engine_graph_and_eager_runs_agree():
    sp = lambda: SamplingParams(temperature=1.0, min_p=MIN_P, seed=77, max_tokens=32, ignore_eos=True)
    runs = []
    for eager in (False, True):
        eng = _engine(enforce_eager=eager)
        toks, tap = _run(eng, _prompts()[:1], [sp()])
        assert len(toks[0]) == 32
        _within(toks[0], tap["r0"])
        st = eng.runner.stats
        assert eng.metrics()["min_p_steps"] > 0
        if eager:
            assert st["graph_replays"] == 0 and not _mp_variants(eng.runner)
        else:
            assert st["graph_replays"] > 0 and _mp_variants(eng.runner)
        runs.append(toks[0])
    assert runs[0] == runs[1]


def test_engine_min_p_row_next_to_a_plain_row():
    eng = _engine()
    params = [SamplingParams(temperature=1.0, min_p=MIN_P, seed=5, max_tokens=24, ignore_eos=True),
              SamplingParams(temperature=1.0, seed=6, max_tokens=16, ignore_eos=True)]
    toks, tap = _run(eng, _prompts(), params)
    assert len(toks[0]) == 24 and len(toks[1]) == 16
    _within(toks[0], tap["r0"])
    assert eng.metrics()["min_p_steps"] > 0 and not eng.runner.mp_active


def test_engine_without_min_p_counts_and_captures_nothing():
    eng = _engine()
    toks, _ = _run(eng, _prompts(), [SamplingParams(temperature=1.0, seed=s, max_tokens=12,
                                                     ignore_eos=True) for s in (5, 6)])
    assert len(toks[0]) == 12 and len(toks[1]) == 12
    assert eng.metrics()["min_p_steps"] == 0 and eng.runner.stats["graph_replays"] > 0
    assert eng.runner.graphs and not _mp_variants(eng.runner)


def test_engine_guided_request_with_min_p():
    from fasttalk_llm_microservice_amd.engine.guided import GuidedSpec

    spec = GuidedSpec.json_schema({"type": "object", "properties": {
        "city": {"type": "string", "maxLength": 8}, "n": {"type": "integer"}},
        "required": ["city", "n"]})
    eng = _engine()
    params = [SamplingParams(temperature=0.8, min_p=MIN_P, seed=9, max_tokens=48, guided=spec),
              SamplingParams(temperature=1.0, min_p=0.1, seed=4, max_tokens=12, ignore_eos=True)]
    toks, _ = _run(eng, _prompts(), params)
    json.loads(eng.tokenizer.decode(toks[0]))
    assert len(toks[1]) == 12 and eng.metrics()["min_p_steps"] > 0

