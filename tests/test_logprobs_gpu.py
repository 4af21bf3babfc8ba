"""Per-token logprobs on the GPU (csrc/kernels/logprobs.hip): the kernel against
``ops.reference.token_logprobs`` (ids exactly) and a float64 ``log_softmax`` (values), rows
built to break a sliced top-K, and the engine -- hipGraph decode, pipelined, and eager --
checked step by step against the raw logit taps."""
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
K = ops.LOGPROBS_MAX
COLS = 1 + K
NEG_INF = float("-inf")


def _padded(x: torch.Tensor) -> torch.Tensor:
    """``x`` [rows, V] on the device as a view of a wider buffer (row stride a multiple
    of 8 and > V, the columns behind V filled with a huge value no result may pick up)."""
    rows, v = x.shape
    stride = (v + 7) // 8 * 8 + 64
    buf = torch.full((rows, stride), 3.0e38, dtype=x.dtype, device=DEV)
    buf[:, :v] = x.to(DEV)
    return buf[:, :v]


def _run_kernel(x: torch.Tensor, sampled, want):
    """(out_lp, out_id) of the kernel on the host; the outputs are pre-filled with a
    sentinel (rows that asked for nothing must keep it)."""
    rows = x.shape[0]
    out_lp = torch.full((rows, COLS), 123.0, dtype=torch.float32, device=DEV)
    out_id = torch.full((rows, COLS), -77, dtype=torch.int32, device=DEV)
    ops.logprobs(_padded(x), torch.tensor(sampled, dtype=torch.int32, device=DEV),
                 torch.tensor(want, dtype=torch.int32, device=DEV), out_lp, out_id)
    torch.cuda.synchronize()
    return out_lp.cpu(), out_id.cpu()


def _check(x: torch.Tensor, sampled, want, got_lp, got_id, what=""):
    """Ids equal the reference exactly; logprobs are within 1e-4 absolute of a float64
    log_softmax of the same widened logits (about 50x the fp32 error of a tree sum of
    <= 131072 positive terms, one exp and one log at |lse| <~ 30).  The output is fp32:
    from |logprob| = 512 on, where half an fp32 ulp alone is 3e-5 and grows with the value,
    the bound is 2 fp32 ulps of the value (<= |v| 2^-22; only rows built with a maximum of
    3e4 get there).  A -inf logit must give exactly -inf.  Rows with want -1 keep the
    sentinel."""
    xf = x.float()
    rows = xf.shape[0]
    ref_lp, ref_id = ref.token_logprobs(xf, sampled, want,
                                        torch.full((rows, COLS), 123.0),
                                        torch.full((rows, COLS), -77, dtype=torch.int32))
    assert torch.equal(got_id, ref_id), (what, (got_id != ref_id).nonzero()[:8].tolist())
    lp64 = torch.log_softmax(xf.double(), dim=-1)
    worst = 0.0
    for r in range(rows):
        if want[r] < 0:
            assert bool((got_lp[r] == 123.0).all()) and bool((got_id[r] == -77).all()), (what, r)
            continue
        n = 1 + want[r]
        ids = ref_id[r, :n].long()
        exp = lp64[r, ids]
        got = got_lp[r, :n].double()
        assert not bool(torch.isnan(got_lp[r]).any()), (what, r, got_lp[r])
        inf = xf[r, ids] == NEG_INF
        assert bool((got[inf] == NEG_INF).all()), (what, r, got, exp)
        err = (got[~inf] - exp[~inf]).abs()
        tol = torch.where(exp[~inf].abs() <= 512.0, torch.full_like(err, 1e-4),
                          exp[~inf].abs() * 2.0 ** -22)
        assert bool((err <= tol).all()), (what, r, err.max().item(), got, exp)
        small = exp[~inf].abs() <= 512.0
        if bool(small.any()):
            worst = max(worst, err[small].max().item())
        assert bool((got_lp[r, n:] == 0.0).all()) and bool((got_id[r, n:] == -1).all()), (what, r)
    return worst


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("vocab", [128256, 1003])
@pytest.mark.parametrize("rows", [1, 5, 64])
def test_logprobs_match_reference(rows, vocab, dtype):
    """Random rows (bf16 logits tie often; a third of the fp32 ones are rounded to bf16 so
    they tie too), ``want`` mixing 20, -1, 0, 1, 5 in a batch, sampled ids 0, V - 1, the
    row's minimum (outside every top 20) and random ones."""
    g = torch.Generator().manual_seed(rows * 13 + vocab)
    x = torch.randn(rows, vocab, generator=g) * 4
    if dtype == torch.float32:
        x[:, ::3] = x[:, ::3].bfloat16().float()
    x = x.to(dtype)
    want = [(20, -1, 0, 1, 5)[r % 5] for r in range(rows)]
    rnd = torch.randint(0, vocab, (rows,), generator=g).tolist()
    low = x.float().argmin(dim=-1).tolist()
    sampled = [(vocab - 1, 0, low[r], rnd[r])[r % 4] for r in range(rows)]
    if rows >= 5:
        sampled[0], sampled[2], sampled[4] = 0, vocab - 1, low[4]   # rows that asked
    got_lp, got_id = _run_kernel(x, sampled, want)
    worst = _check(x, sampled, want, got_lp, got_id, f"rows {rows} V {vocab} {dtype}")
    print(f"rows {rows} V {vocab} {dtype}: max |logprob - float64| {worst:.3e}")


def _crafted(vocab: int, dtype):
    """Rows built to break a sliced top-K (every row wants 20)."""
    g = torch.Generator().manual_seed(vocab)
    top = 30.0 + 0.5 * torch.arange(K, dtype=torch.float32)   # exact in bf16
    base = lambda: (torch.randn(vocab, generator=g) * 3).clamp(-20, 20).to(dtype).float()  # noqa: E731
    rows, names = [], []

    def add(name, row):
        names.append(name)
        rows.append(row)

    if vocab > 6000:
        r = base()   # ids 5000..5019: one slice, one wave, three lanes of it
        r[5000:5000 + K] = top[torch.randperm(K, generator=g)]
        add("20 consecutive ids inside one slice", r)
    r = base()
    r[vocab - K:] = top[torch.randperm(K, generator=g)]
    add("the last 20 ids (tail chunk)", r)
    r = base()
    r[:K] = top
    add("ids 0..19, ascending values", r)
    add("all equal", torch.full((vocab,), 1.25))
    r = base()
    ids = torch.randperm(vocab, generator=g)[:40]
    r[ids] = 25.0
    add("40 ids share the maximum", r)
    r = base()
    r[vocab // 2] = 3.0e4
    add("maximum of 3e4", r)
    r = base()
    r[torch.randperm(vocab, generator=g)[: vocab // 3]] = NEG_INF
    add("a third of the row at -inf", r)
    r = torch.full((vocab,), NEG_INF)
    r[torch.randperm(vocab, generator=g)[:10]] = torch.randn(10, generator=g)
    add("ten finite entries, the rest -inf", r)
    return names, torch.stack(rows).to(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("vocab", [128256, 1003])
def test_rows_built_to_break_a_sliced_topk(vocab, dtype):
    names, x = _crafted(vocab, dtype)
    n = x.shape[0]
    want = [K] * n
    xf = x.float()
    row = dict(zip(names, range(n)))
    sampled = [int(xf[r].argmin()) if r % 2 else int(xf[r].argmax()) for r in range(n)]
    sampled[row["a third of the row at -inf"]] = int(xf[row["a third of the row at -inf"]].argmin())
    got_lp, got_id = _run_kernel(x, sampled, want)
    _check(x, sampled, want, got_lp, got_id, f"V {vocab} {dtype}")
    r = row["all equal"]
    assert got_id[r, 1:].tolist() == list(range(K))
    assert bool((got_lp[r] - (-np.log(vocab))).abs().max() <= 1e-4)
    r = row["40 ids share the maximum"]
    tied = sorted(torch.nonzero(xf[r] == 25.0).flatten().tolist())
    assert len(tied) == 40 and got_id[r, 1:].tolist() == tied[:K]
    r = row["ids 0..19, ascending values"]
    assert got_id[r, 1:].tolist() == list(range(K - 1, -1, -1))
    r = row["the last 20 ids (tail chunk)"]
    assert sorted(got_id[r, 1:].tolist()) == list(range(vocab - K, vocab))
    r = row["maximum of 3e4"]
    assert got_id[r, 1] == vocab // 2 and got_lp[r, 1] == 0.0 and bool(torch.isfinite(got_lp[r]).all())
    r = row["a third of the row at -inf"]
    assert got_lp[r, 0] == NEG_INF and bool(torch.isfinite(got_lp[r, 1:]).all())   # sampled: the argmin
    r = row["ten finite entries, the rest -inf"]
    assert bool(torch.isfinite(got_lp[r, 1:11]).all()) and bool((got_lp[r, 11:] == NEG_INF).all())


# ------------------------------------------------------------------------------- engine
LENS = [14, 9, 12, 7, 11, 8]
BIAS_TOKEN = 4242


def _engine(**kw):
    base = dict(model="tiny", device="cuda", num_kv_blocks=256, max_model_len=512, max_num_seqs=8,
                graph_batch_sizes=(1, 2, 4, 8), enable_prefix_caching=False)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def _prompts():
    rng = np.random.default_rng(3)
    return [rng.integers(0, 120000, n).tolist() for n in (12, 20, 9, 17, 15, 11)]


def _run(eng, prompts, params):
    """({i: token ids}, {i: logprob entries or None}, {request id: [raw logits per step]})"""
    r = eng.runner
    r.logits_tap, r.logits_tap_ids = [], []
    toks, lps = {}, {}

    def on_output(o, i):
        toks.setdefault(i, []).extend(o.token_ids)
        if o.logprobs is None:
            lps[i] = None
        else:
            assert len(o.logprobs) == len(o.token_ids), (i, o)
            lps.setdefault(i, []).extend(o.logprobs)

    for i, (p, sp) in enumerate(zip(prompts, params)):
        eng.add_request(f"r{i}", p, sp, on_output=lambda o, i=i: on_output(o, i))
    while eng.has_work():
        eng.step()
    tap = {}
    for logits, ids in zip(r.logits_tap, r.logits_tap_ids):
        for row, rid in enumerate(ids or []):
            tap.setdefault(rid, []).append(logits[row].float().cpu())
    r.logits_tap = r.logits_tap_ids = None
    return toks, lps, tap


def _check_against_tap(toks, entries, taps, want):
    """Every step of a request: the reported id is the emitted token, the alternatives
    are the reference's over that step's raw logits, every logprob within the kernel
    tests' tolerance of the float64 log_softmax of those logits."""
    assert len(entries) == len(toks) <= len(taps)
    for k, (tok, (tid, lp, alts)) in enumerate(zip(toks, entries)):
        raw = taps[k].view(1, -1)
        assert tid == tok
        got_lp = torch.tensor([[lp] + [a[1] for a in alts] + [0.0] * (K - len(alts))])
        got_id = torch.tensor([[tid] + [a[0] for a in alts] + [-1] * (K - len(alts))],
                              dtype=torch.int32)
        assert len(alts) == want
        _check(raw, [tok], [want], got_lp, got_id, f"step {k}")


@pytest.mark.parametrize("eager", [False, True], ids=["graphs", "eager"])
def test_engine_logprobs_against_the_raw_taps(eager):
    """Six concurrent requests of different lengths; three ask (0, 5 and 20 alternatives):
    one of them greedy, one with a +100 logit_bias on one token (it emits that token every
    step, and its logprobs are those of the RAW logits: about -log V, not about 0), one at
    temperature 0.8 with a seed.  The others emit what they emit when nobody asks."""
    prompts = _prompts()
    base = [dict(temperature=0.0), dict(temperature=0.0, logit_bias={BIAS_TOKEN: 100.0}),
            dict(temperature=0.8, seed=1234), dict(temperature=0.0), dict(temperature=0.0),
            dict(temperature=0.0)]
    asks = [0, 5, 20, None, None, None]
    params = [SamplingParams(max_tokens=n, ignore_eos=True, logprobs=a, **kw)
              for n, kw, a in zip(LENS, base, asks)]
    eng = _engine(enforce_eager=eager)
    toks, lps, tap = _run(eng, prompts, params)
    assert [len(toks[i]) for i in range(6)] == LENS
    st = eng.runner.stats
    if eager:
        assert st["graph_replays"] == 0
    else:
        assert st["graph_replays"] > 0 and eng.stats["pipelined_steps"] > 0
    assert all(len(k) == 2 for k in eng.runner.graphs) and all(len(k) == 2 for k in eng.runner.graphs_split)
    m = eng.metrics()
    assert m["logprob_steps"] > 0 and m["logprob_rows"] >= sum(LENS[:3])
    for i in range(3):
        _check_against_tap(toks[i], lps[i], tap[f"r{i}"], asks[i])
    assert all(lps[i] is None for i in range(3, 6))
    # the biased request: penalised logits would put its token at logprob ~ 0
    assert toks[1] == [BIAS_TOKEN] * LENS[1]
    assert all(lp < -5.0 and alts[0][0] != BIAS_TOKEN for _, lp, alts in lps[1])

    off = _engine(enforce_eager=eager)
    bare = [SamplingParams(max_tokens=n, ignore_eos=True, **kw) for n, kw in zip(LENS, base)]
    same, none, _ = _run(off, prompts, bare)
    assert [same[i] for i in range(3, 6)] == [toks[i] for i in range(3, 6)]
    assert all(v is None for v in none.values())
    assert off.metrics()["logprob_steps"] == 0 and off.metrics()["logprob_rows"] == 0


def test_engine_guided_row_next_to_a_logprob_row():
    """A bound json_schema request (its steps run the split forward | sampler graphs)
    shares its batch with a request that wants logprobs: the guided text is what it is
    without the neighbour asking, and the neighbour's logprobs match the raw taps."""
    from fasttalk_llm_microservice_amd.engine.guided import GuidedSpec

    spec = GuidedSpec.json_schema({"type": "object", "properties": {
        "city": {"type": "string", "maxLength": 8}, "n": {"type": "integer"}},
        "required": ["city", "n"]})
    prompts = _prompts()[:2]
    eng = _engine()

    def run(ask):
        params = [SamplingParams(temperature=0.0, max_tokens=40, guided=spec),
                  SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True, logprobs=ask)]
        return _run(eng, prompts, params)

    plain, _, _ = run(None)
    before = eng.metrics()["logprob_steps"]
    assert before == 0
    toks, lps, tap = run(5)
    assert toks[0] == plain[0] and toks[1] == plain[1]
    json.loads(eng.tokenizer.decode(toks[0]))
    assert lps[0] is None
    _check_against_tap(toks[1], lps[1], tap["r1"], 5)
    assert eng.metrics()["logprob_rows"] >= 12
    assert all(len(k) == 2 for k in eng.runner.graphs_split)
    with pytest.raises(Exception, match="guided"):
        eng.add_request("g", prompts[0], SamplingParams(max_tokens=4, guided=spec, logprobs=1))


def test_checked_build_passes_this_file():
    """The bounds-checked kernel build (FT_KERNEL_CHECKS=1: sampled id < V, want <= 20)
    runs the tests above in a child process without a violation."""
    env = dict(os.environ, FT_KERNEL_CHECKS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "not checked_build", os.path.abspath(__file__)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-2000:]
