"""min_p without a GPU: SamplingParams validation, pick_min_p, the fp32 reference
sampler (ops/reference.py, the CPU backend), the CPU engine end to end and the decode
staging image (engine/runner.py).  Kernels: tests/test_min_p_gpu.py."""
import math

import numpy as np
import pytest
import torch

from fasttalk_llm_microservice_amd import ops
from fasttalk_llm_microservice_amd.engine import runner as runner_mod
from fasttalk_llm_microservice_amd.engine.config import EngineConfig
from fasttalk_llm_microservice_amd.engine.engine import EngineError, LLMEngine
from fasttalk_llm_microservice_amd.engine.sampling_params import (SamplingParams, ln_min_p,
                                                                  pick_min_p)
from fasttalk_llm_microservice_amd.ops import reference as ref

NEG_INF = float("-inf")


# ------------------------------------------------------------------ SamplingParams
def test_default_is_off():
    assert SamplingParams().min_p == 0.0
    assert ln_min_p(0.0) == NEG_INF and ln_min_p(1.0) == 0.0
    assert ln_min_p(0.05) == math.log(0.05)


@pytest.mark.parametrize("v,want", [(0, 0.0), (1, 1.0), (None, 0.0), (0.3, 0.3), (1.0, 1.0)])
def test_valid_values(v, want):
    p = SamplingParams(min_p=v)
    assert p.min_p == want and isinstance(p.min_p, float)


@pytest.mark.parametrize("v", [True, False, float("nan"), -0.1, 1.1, "0.5", float("inf")])
def test_bad_values_raise(v):
    with pytest.raises(ValueError, match="min_p"):
        SamplingParams(min_p=v)


def test_pick_min_p():
    assert pick_min_p({}) == {} and pick_min_p({"min_p": None}) == {}
    assert pick_min_p({"min_p": 0.25, "top_p": 0.9}) == {"min_p": 0.25}
    assert pick_min_p({"min_p": 0}) == {"min_p": 0.0}
    for bad in (1.5, -1, True, "x", float("nan")):
        with pytest.raises(ValueError, match="min_p"):
            pick_min_p({"min_p": bad})


# ------------------------------------------------------------------ reference sampler
# the GPU file's fixture row at V = 1,024: six head ids at M - {0 .. 2.5}, three at M - 3,
# the rest at M - 7.25 (at this V that bulk carries the 0.72 of mass, relative to the max,
# that M - 12 carries at V = 128,256); min_p = exp(-2.75) puts the threshold midway
# between M - 2.5 and M - 3
V, M = 1024, 4.0
HEAD = [17, 130, 261, 700, 901, V - 1]
HEAD_VAL = [M - 0.5 * i for i in range(6)]
LOW = [40, 500, 1000]
LNMP = -2.75
DRAWS = 600


def _row():
    x = torch.full((V,), M - 7.25)
    x[HEAD] = torch.tensor(HEAD_VAL)
    x[LOW] = M - 3.0
    return x


def _ref_draws(row, top_p=1.0, top_k=0, lnmp=LNMP, temp=1.0, mask=None, n=DRAWS):
    logits = row.unsqueeze(0).repeat(n, 1)
    t = torch.full((n,), temp)
    out = ref.sample(logits, t, torch.full((n,), top_p), torch.full((n,), top_k, dtype=torch.int32),
                     torch.arange(n, dtype=torch.int64) * 7919 + 3, torch.zeros(n, dtype=torch.int32),
                     mask=None if mask is None else mask.unsqueeze(0).repeat(n, 1),
                     min_p=torch.full((n,), lnmp))
    return set(out.tolist())


def test_reference_kept_set():
    assert _ref_draws(_row()) == set(HEAD)
    # without min_p the bulk (0.22 of the mass) and the low ids are drawn too
    n = DRAWS
    out = ref.sample(_row().unsqueeze(0).repeat(n, 1), torch.ones(n), torch.ones(n),
                     torch.zeros(n, dtype=torch.int32), torch.arange(n, dtype=torch.int64),
                     torch.zeros(n, dtype=torch.int32))
    assert set(out.tolist()) - set(HEAD)


def test_reference_min_p_before_top_p():
    """top_p = 0.5 of the kept mass (Z = 2.415): two ids; of the whole row (Z = 3.29) it
    would be three."""
    assert _ref_draws(_row(), top_p=0.5) == set(HEAD[:2])
    assert _ref_draws(_row(), top_p=0.5, lnmp=NEG_INF) == set(HEAD[:3])


def test_reference_top_k_intersects():
    assert _ref_draws(_row(), top_k=8) == set(HEAD)
    assert _ref_draws(_row(), top_k=100) == set(HEAD)
    assert _ref_draws(_row(), top_k=3) == set(HEAD[:3])


def test_reference_mask_first():
    """Global max and the id at M - 1.5 forbidden: the threshold hangs from the allowed
    max M - 0.5 (ln(min_p) = -2.25: midway between M' - 2 and M' - 2.5)."""
    bits = np.full((V + 31) // 32, -1, np.int64)
    for i in (HEAD[0], HEAD[3]):
        bits[i // 32] &= ~(1 << (i % 32))
    mask = torch.from_numpy((bits & 0xFFFFFFFF).astype(np.uint32).view(np.int32))
    assert _ref_draws(_row(), lnmp=-2.25, mask=mask) == {HEAD[1], HEAD[2], HEAD[4], HEAD[5]}


def test_reference_min_p_one_keeps_tied_maxima():
    row = torch.full((V,), M - 0.0625)
    row[[5, 400, V - 3]] = M
    assert _ref_draws(row, lnmp=0.0, n=200) == {5, 400, V - 3}


def test_reference_greedy_ignores_min_p_and_rounds_to_bf16():
    torch.manual_seed(1)
    x = torch.randn(4, V)
    z = torch.zeros(4)
    out = ref.sample(x, z, z + 1, torch.zeros(4, dtype=torch.int32), torch.arange(4), z.int(),
                     min_p=z + LNMP)
    assert out.tolist() == x.bfloat16().float().argmax(-1).tolist()
    # the edge is on bf16-rounded values: 1.2502 rounds to 1.25 and meets a 1.25 threshold
    row = _row()
    row[LOW[0]] = 1.2502
    assert LOW[0] in _ref_draws(row, temp=4.0, lnmp=-2.75 / 4.0, n=1500)


def test_reference_without_min_p_is_unchanged():
    torch.manual_seed(2)
    x = torch.randn(6, 300) * 2
    t, p = torch.full((6,), 0.8), torch.full((6,), 0.9)
    k = torch.tensor([0, 5, 0, 40, 0, 0], dtype=torch.int32)
    s, st = torch.arange(6, dtype=torch.int64) * 13, torch.arange(6, dtype=torch.int32)
    a = ref.sample(x, t, p, k, s, st)
    assert torch.equal(a, ref.sample(x, t, p, k, s, st, None, None))
    assert torch.equal(a, ops.sample(x, t, p, k, s, st))
    probs = torch.softmax(x[0] / 0.8, -1)
    sp, si = probs.sort(descending=True)
    assert int(a[0]) in set(si[: int((sp.cumsum(0) < 0.9).sum()) + 1].tolist())


# ------------------------------------------------------------------ engine (CPU backend)
PROMPTS = [[11, 22, 33, 44, 55], [7, 8, 9], [100, 200, 300, 400]]


def _engine(**kw):
    base = dict(model="tiny", device="cpu", max_num_seqs=4, max_model_len=256)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def _run_tapped(eng, prompts, params):
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


def _within(toks, taps, min_p, temp=1.0):
    assert len(toks) <= len(taps)
    lim = torch.tensor(ln_min_p(min_p), dtype=torch.float32) * torch.tensor(temp)
    for k, tok in enumerate(toks):
        x = taps[k].bfloat16().float()
        assert x[tok] >= x.max() + lim, (k, tok)


def test_cpu_engine_end_to_end():
    eng = _engine()
    sp = lambda **kw: SamplingParams(temperature=1.0, max_tokens=12, ignore_eos=True, seed=5, **kw)
    toks, tap = _run_tapped(eng, PROMPTS[:2], [sp(min_p=0.3), sp()])
    assert len(toks[0]) == 12 and len(toks[1]) == 12
    _within(toks[0], tap["r0"], 0.3)
    assert eng.metrics()["min_p_steps"] > 0 and not eng.runner.mp_active
    again, _ = _run_tapped(eng, PROMPTS[:2], [sp(min_p=0.3), sp()])
    assert again == toks
    # nobody asks: nothing is counted
    fresh = _engine()
    plain, _ = _run_tapped(fresh, PROMPTS[1:2], [sp()])
    assert len(plain[0]) == 12
    assert fresh.metrics()["min_p_steps"] == 0


def test_tp_refuses_min_p():
    e = _engine()
    e.cfg.tp_size = 2
    with pytest.raises(EngineError, match="min_p is not supported with tensor parallelism yet"):
        e.add_request("tp", [1, 2, 3], SamplingParams(min_p=0.1))
    e.add_request("tp-off", [1, 2, 3], SamplingParams(min_p=0.0, max_tokens=1))


# ------------------------------------------------------------------ staging image
def test_staging_image_layout_and_stale_values():
    """pen | min_p | inputs: a step without min_p stages the h_in words it always did
    (and the same number of them), a step with min_p writes its rows' ln(min_p) and -inf
    for the rows that are off -- also over what an earlier step left there."""
    eng = _engine()
    r = eng.runner
    for i, p in enumerate(PROMPTS):
        eng.add_request(f"s{i}", p, SamplingParams(temperature=0.9, max_tokens=8, ignore_eos=True,
                                                   seed=i))
    eng.step()                      # prefill: the sequences hold blocks now
    seqs = list(eng.scheduler.running)
    assert len(seqs) == 3
    mb = r.max_decode_batch
    pw, mw = runner_mod.pen_words(mb), runner_mod.minp_words(mb)
    assert mw == mb
    st = r.stg[0]
    assert st.h_all.numel() == pw + mw + runner_mod.input_words(mb, r.max_blocks_per_seq)
    assert st.h_in.data_ptr() == st.h_all[pw + mw:].data_ptr()
    nb = 4
    r._decode_fill(seqs, nb, st)
    before = st.h_in.clone()
    assert not st.mp and np.isneginf(st.h_minp[:nb]).all()

    seqs[1].params.min_p = 0.3
    r.mp_active = True
    st.h_minp[:] = 0.0              # stale words of an earlier step
    r._decode_fill(seqs, nb, st)
    assert st.mp
    assert torch.equal(st.h_in, before)
    assert st.h_minp[1] == np.float32(math.log(0.3))
    assert np.isneginf(st.h_minp[[0, 2, 3]]).all()
    got = st.h_all[pw:pw + mw].view(torch.float32).numpy()
    assert got[1] == np.float32(math.log(0.3))

    seqs[1].params.min_p = 0.0      # the next step: nobody asks, nothing stale stays
    r._decode_fill(seqs, nb, st)
    assert not st.mp and np.isneginf(st.h_minp[:nb]).all() and torch.equal(st.h_in, before)
    assert r._minp_array(seqs) is None
    seqs[2].params.min_p = 1.0
    a = r._minp_array(seqs)
    assert a.dtype == np.float32 and a.tolist() == [NEG_INF, NEG_INF, 0.0]
    seqs[2].params.temperature = 0.0    # greedy rows ignore it
    assert r._minp_array(seqs) is None
    r.mp_active = False
    assert r._minp_array(seqs) is None
