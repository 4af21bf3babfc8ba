"""Prompt logprobs on the GPU (csrc/kernels/logprobs.hip, ft_prompt_logprobs): the kernel
against ``ops.reference.prompt_logprobs`` (ids and ranks exactly) and a float64
``log_softmax`` (values), rows built to break a rank count, and the engine -- whole,
chunked and queued prefill, the prefix cache, the batch-invariant plans -- checked
position by position against the raw logit taps."""
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
VOCABS = [128256, 1003]   # 1003: slices end inside an 8-id chunk (the tail chunk)


def _padded(x: torch.Tensor) -> torch.Tensor:
    """``x`` [rows, V] on the device as a view of a wider buffer (row stride a multiple
    of 8 and > V, the columns behind V filled with a huge value no result may pick up:
    it would win every top-N and push every rank up)."""
    rows, v = x.shape
    stride = (v + 7) // 8 * 8 + 64
    buf = torch.full((rows, stride), 3.0e38, dtype=x.dtype, device=DEV)
    buf[:, :v] = x.to(DEV)
    return buf[:, :v]


def _run_kernel(x: torch.Tensor, targets, want):
    """(out_lp, out_id, out_rank) of the kernel on the host; the outputs are pre-filled
    with a sentinel (rows that asked for nothing must keep it)."""
    rows = x.shape[0]
    out_lp = torch.full((rows, COLS), 123.0, dtype=torch.float32, device=DEV)
    out_id = torch.full((rows, COLS), -77, dtype=torch.int32, device=DEV)
    out_rank = torch.full((rows,), -5, dtype=torch.int32, device=DEV)
    ops.prompt_logprobs(_padded(x), torch.tensor(targets, dtype=torch.int32, device=DEV),
                        torch.tensor(want, dtype=torch.int32, device=DEV), out_lp, out_id, out_rank)
    torch.cuda.synchronize()
    return out_lp.cpu(), out_id.cpu(), out_rank.cpu()


def _check(x: torch.Tensor, targets, want, got_lp, got_id, got_rank, what=""):
    """Ids and ranks equal the reference exactly (the rank also a count done here);
    logprobs are within the bound the per-token logprob tests assert against a float64
    log_softmax of the same widened logits: 1e-4 absolute (about 50x the fp32 error of a
    tree sum of <= 131072 positive terms, one exp and one log at |lse| <~ 30), and from
    |logprob| = 512 on, where half an fp32 ulp alone is 3e-5, 2 fp32 ulps of the value
    (<= |v| 2^-22).  A -inf logit gives exactly -inf.  Rows with want -1 keep the sentinel
    in all three outputs."""
    xf = x.float()
    rows = xf.shape[0]
    ref_lp, ref_id, ref_rank = ref.prompt_logprobs(
        xf, targets, want, torch.full((rows, COLS), 123.0),
        torch.full((rows, COLS), -77, dtype=torch.int32), torch.full((rows,), -5, dtype=torch.int32))
    assert torch.equal(got_id, ref_id), (what, (got_id != ref_id).nonzero()[:8].tolist())
    assert torch.equal(got_rank, ref_rank), (what, got_rank.tolist(), ref_rank.tolist())
    lp64 = torch.log_softmax(xf.double(), dim=-1)
    worst = 0.0
    for r in range(rows):
        if want[r] < 0:
            assert bool((got_lp[r] == 123.0).all()) and bool((got_id[r] == -77).all()) \
                and got_rank[r] == -5, (what, r)
            continue
        assert got_rank[r] == 1 + int((xf[r] > xf[r, targets[r]]).sum()), (what, r)
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


def _random_case(rows, vocab, dtype):
    g = torch.Generator().manual_seed(rows * 13 + vocab)
    x = torch.randn(rows, vocab, generator=g) * 4
    if dtype == torch.float32:
        x[:, ::3] = x[:, ::3].bfloat16().float()   # a third of the fp32 row ties like bf16
    x = x.to(dtype)
    want = [(20, -1, 0, 1, 5)[r % 5] for r in range(rows)]
    rnd = torch.randint(0, vocab, (rows,), generator=g).tolist()
    low = x.float().argmin(dim=-1).tolist()
    high = x.float().argmax(dim=-1).tolist()
    targets = [(vocab - 1, 0, low[r], rnd[r], high[r])[(r + r // 5) % 5] for r in range(rows)]
    if rows >= 5:   # rows that asked: id 0, V - 1, the argmin, the argmax
        targets[0], targets[2], targets[3], targets[4] = 0, vocab - 1, low[3], high[4]
    return x, targets, want


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("vocab", VOCABS)
@pytest.mark.parametrize("rows", [1, 5, 64, 130])
def test_prompt_logprobs_match_reference(rows, vocab, dtype):
    x, targets, want = _random_case(rows, vocab, dtype)
    got = _run_kernel(x, targets, want)
    worst = _check(x, targets, want, *got, f"rows {rows} V {vocab} {dtype}")
    print(f"rows {rows} V {vocab} {dtype}: max |logprob - float64| {worst:.3e}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("vocab", VOCABS)
def test_rows_built_to_break_a_rank_count(vocab, dtype):
    g = torch.Generator().manual_seed(vocab)
    base = lambda: (torch.randn(vocab, generator=g) * 3).clamp(-20, 20).to(dtype).float()  # noqa: E731
    rows, targets, expect = [], [], []

    def add(row, target, rank=None):
        rows.append(row)
        targets.append(int(target))
        expect.append(rank)

    add(torch.full((vocab,), 1.25), vocab // 3, 1)                  # all equal
    add(torch.full((vocab,), 1.25), vocab - 1, 1)
    r = base()
    tied = torch.randperm(vocab, generator=g)[:41]
    r[tied[:40]] = 25.0
    r[tied[40]] = 24.875                                             # exact in bf16, just below
    add(r, tied[17], 1)                                              # one of the 40 maxima
    add(r.clone(), tied[40], 41)                                     # the id just below them
    r = base()
    r[5], r[vocab - 2] = -0.0, 0.0
    add(r, 5)                                                        # -0.0 ...
    add(r.clone(), vocab - 2)                                        # ... ranks as +0.0
    r = base()
    gone = torch.randperm(vocab, generator=g)[: vocab // 3]
    r[gone] = NEG_INF
    add(r, gone[0], 1 + vocab - vocab // 3)                          # a -inf target
    r = base()
    add(r, vocab - 1)                                                # the last partial chunk
    add(r.clone(), vocab - 3)
    r = base()
    r[vocab // 2] = 3.0e4
    add(r, vocab // 2, 1)                                            # maximum of 3e4
    add(r.clone(), 7)
    x = torch.stack(rows).to(dtype)
    want = [K] * len(rows)
    got_lp, got_id, got_rank = _run_kernel(x, targets, want)
    _check(x, targets, want, got_lp, got_id, got_rank, f"V {vocab} {dtype}")
    for i, e in enumerate(expect):
        if e is not None:
            assert got_rank[i] == e, (i, got_rank[i], e)
    assert got_rank[4] == got_rank[5]                                # the two zeros
    assert got_lp[6, 0] == NEG_INF
    assert got_lp[9, 0] == 0.0 and bool(torch.isfinite(got_lp[10]).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("vocab", VOCABS)
def test_ops_logprobs_is_unchanged_next_to_it(vocab, dtype):
    """The per-token op on the same inputs still returns what its reference returns, and
    -- rank aside -- what the new op returns."""
    x, targets, want = _random_case(64, vocab, dtype)
    out_lp = torch.full((64, COLS), 123.0, dtype=torch.float32, device=DEV)
    out_id = torch.full((64, COLS), -77, dtype=torch.int32, device=DEV)
    ops.logprobs(_padded(x), torch.tensor(targets, dtype=torch.int32, device=DEV),
                 torch.tensor(want, dtype=torch.int32, device=DEV), out_lp, out_id)
    torch.cuda.synchronize()
    ref_lp, ref_id = ref.token_logprobs(x.float(), targets, want, torch.full((64, COLS), 123.0),
                                        torch.full((64, COLS), -77, dtype=torch.int32))
    assert torch.equal(out_id.cpu(), ref_id)
    fin = torch.isfinite(ref_lp)
    assert bool(((out_lp.cpu() - ref_lp)[fin].abs() <= 1e-4).all())
    new_lp, new_id, _ = _run_kernel(x, targets, want)
    assert torch.equal(new_id, out_id.cpu()) and torch.equal(new_lp, out_lp.cpu())


# ------------------------------------------------------------------------------- engine
def _engine(**kw):
    base = dict(model="tiny", device="cuda", num_kv_blocks=256, max_model_len=512, max_num_seqs=8,
                graph_batch_sizes=(1, 2, 4, 8), enable_prefix_caching=False)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def _prompts(lens, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 120000, n).tolist() for n in lens]


def _drain(eng, outs):
    while eng.has_work():
        eng.step()
    return outs


def _run(eng, prompts, params, before=None):
    """({i: token ids}, {i: first event's prompt_logprobs}, {request id: {position: raw
    logits}}); ``before(eng)`` runs after the requests are added."""
    r = eng.runner
    r.plp_tap = []
    toks, plps, events = {}, {}, {}

    def on_output(o, i):
        toks.setdefault(i, []).extend(o.token_ids)
        events[i] = events.get(i, 0) + 1
        if events[i] == 1:
            plps[i] = o.prompt_logprobs
        else:
            assert o.prompt_logprobs is None, (i, events[i])

    for i, (p, sp) in enumerate(zip(prompts, params)):
        eng.add_request(f"r{i}", p, sp, on_output=lambda o, i=i: on_output(o, i))
    _drain(eng, None)
    tap = {}
    for rid, p0, raw in r.plp_tap:
        for k in range(raw.shape[0]):
            tap.setdefault(rid, {})[p0 + k] = raw[k]
    r.plp_tap = None
    return toks, plps, tap


def _check_against_tap(prompt, plp, taps, want):
    """Entry 0 is None; every other entry's id is the prompt token, and its alternatives,
    rank and logprobs are the reference's over the raw logits tapped at its position."""
    n = len(prompt)
    assert len(plp) == n and plp[0] is None
    assert sorted(taps) == list(range(n - 1))
    raw = torch.stack([taps[p] for p in range(n - 1)])
    got_lp = torch.tensor([[e[1]] + [a[1] for a in e[3]] + [0.0] * (K - len(e[3])) for e in plp[1:]])
    got_id = torch.tensor([[e[0]] + [a[0] for a in e[3]] + [-1] * (K - len(e[3])) for e in plp[1:]],
                          dtype=torch.int32)
    got_rank = torch.tensor([e[2] for e in plp[1:]], dtype=torch.int32)
    assert [e[0] for e in plp[1:]] == list(prompt[1:])
    assert all(len(e[3]) == want for e in plp[1:])
    return _check(raw, list(prompt[1:]), [want] * (n - 1), got_lp, got_id, got_rank)


LENS = [40, 9, 23, 17, 31, 12]
OUT = [6, 9, 5, 7, 4, 8]


@pytest.mark.parametrize("eager", [False, True], ids=["graphs", "eager"])
def test_engine_prompt_logprobs_against_the_raw_taps(eager):
    """Six concurrent requests of prompt lengths 9-40; three ask (0, 5 and 20
    alternatives).  LM-head slices of 16 rows: the 40-token prompt spans three."""
    prompts = _prompts(LENS)
    asks = [20, 0, 5, None, None, None]
    kw = [dict(temperature=0.0)] * 5 + [dict(temperature=0.8, seed=4)]
    params = [SamplingParams(max_tokens=n, ignore_eos=True, prompt_logprobs=a, **k)
              for n, a, k in zip(OUT, asks, kw)]
    eng = _engine(enforce_eager=eager)
    eng.runner.plp_slice_rows = 16
    toks, plps, tap = _run(eng, prompts, params)
    assert [len(toks[i]) for i in range(6)] == OUT
    for i in range(3):
        _check_against_tap(prompts[i], plps[i], tap[f"r{i}"], asks[i])
    assert all(plps[i] is None for i in range(3, 6))
    m = eng.metrics()
    assert m["prompt_logprob_steps"] > 0 and m["prompt_logprob_rows"] == sum(LENS[:3]) - 3
    if not eager:
        assert eng.runner.stats["graph_replays"] > 0
    assert all(len(k) == 2 for k in eng.runner.graphs)   # no new graph variants

    off = _engine(enforce_eager=eager)
    bare = [SamplingParams(max_tokens=n, ignore_eos=True, **k) for n, k in zip(OUT, kw)]
    same, none, _ = _run(off, prompts, bare)
    assert [same[i] for i in range(6)] == [toks[i] for i in range(6)]
    assert all(v is None for v in none.values())
    assert off.metrics()["prompt_logprob_steps"] == 0 and off.metrics()["prompt_logprob_rows"] == 0
    assert off.runner.d_plp is None and off.runner._plp_sync is None


def _chunked_run(invariant: bool, budget: int):
    """A 300-token prompt that asked, arriving while two sequences decode; ``budget``:
    the step's token budget (small: the prompt is prefilled in chunks queued behind the
    running steps).  Returns (engine, prompt, its entries, its taps, chunk count)."""
    eng = _engine(model="tiny-2k" if invariant else "tiny", batch_invariant=invariant,
                  max_num_batched_tokens=budget, prefill_chunk=min(budget, 96), max_model_len=1024)
    long_p = _prompts([300], seed=9)[0]
    dec = SamplingParams(temperature=0.0, max_tokens=48, ignore_eos=True)
    r = eng.runner
    r.plp_tap = []
    got = []
    for i, p in enumerate(_prompts([10, 14], seed=10)):
        eng.add_request(f"d{i}", p, dec)
    for _ in range(4):   # the two are decoding (queued graph steps) when the prompt arrives
        eng.step()
    eng.add_request("long", long_p, SamplingParams(temperature=0.0, max_tokens=3, ignore_eos=True,
                                                   prompt_logprobs=5), on_output=got.append)
    _drain(eng, None)
    tap, chunks = {}, 0
    for rid, p0, raw in r.plp_tap:
        if rid == "long":
            chunks += 1
            for k in range(raw.shape[0]):
                assert p0 + k not in tap   # no position is scored twice here (no preemption)
                tap[p0 + k] = raw[k]
    r.plp_tap = None
    assert got[0].prompt_logprobs is not None and all(o.prompt_logprobs is None for o in got[1:])
    return eng, long_p, got[0].prompt_logprobs, tap, chunks


@pytest.mark.parametrize("invariant", [False, True], ids=["default", "batch_invariant"])
def test_chunked_and_queued_prefill(invariant):
    """The prompt runs in >= 3 chunks, queued behind running steps (the mixed chain takes
    part).  Its entries are complete, in order, without duplicates and match the taps.
    Against the same prompt prefilled in ONE step the logprobs agree within the kernel
    tests' 1e-4 where the engine promises the same logits for a row whatever shares its
    step -- the batch-invariant plans; under the default plans the GEMM and attention
    tilings depend on the step's rows, the bf16 logits differ by their own rounding
    (printed), and only the ids are compared."""
    eng, prompt, plp, tap, chunks = _chunked_run(invariant, 112)
    assert chunks >= 3 and eng.runner.stats["mixed_ahead"] > 0
    _check_against_tap(prompt, plp, tap, 5)
    one, p1, plp1, tap1, chunks1 = _chunked_run(invariant, 2048)
    assert chunks1 == 1 and p1 == prompt
    _check_against_tap(prompt, plp1, tap1, 5)
    a = torch.tensor([e[1] for e in plp[1:]], dtype=torch.float64)
    b = torch.tensor([e[1] for e in plp1[1:]], dtype=torch.float64)
    print(f"invariant {invariant}: {chunks} chunks, max |logprob chunked - one step| "
          f"{(a - b).abs().max().item():.3e}")
    assert [e[0] for e in plp[1:]] == [e[0] for e in plp1[1:]]
    if invariant:
        assert bool(((a - b).abs() <= 1e-4).all())
        assert [e[2] for e in plp[1:]] == [e[2] for e in plp1[1:]]


def test_prefix_cache_on():
    """The prompt's blocks are cached by a request that does not ask; the one that asks
    computes every position all the same (num_cached_tokens 0); a third, plain request
    still hits the cache."""
    eng = _engine(enable_prefix_caching=True)
    p = _prompts([70], seed=12)[0]
    bare = SamplingParams(temperature=0.0, max_tokens=2, ignore_eos=True)
    ev = {k: [] for k in ("warm", "ask", "again")}
    eng.add_request("warm", p, bare, on_output=ev["warm"].append)
    _drain(eng, None)
    eng.runner.plp_tap = []
    eng.add_request("ask", p, SamplingParams(temperature=0.0, max_tokens=2, ignore_eos=True,
                                             prompt_logprobs=2), on_output=ev["ask"].append)
    _drain(eng, None)
    tap = {p0 + k: raw[k] for _, p0, raw in eng.runner.plp_tap for k in range(raw.shape[0])}
    eng.runner.plp_tap = None
    assert ev["ask"][0].num_cached_tokens == 0
    _check_against_tap(p, ev["ask"][0].prompt_logprobs, tap, 2)
    eng.add_request("again", p, bare, on_output=ev["again"].append)
    _drain(eng, None)
    assert ev["again"][0].num_cached_tokens == 64
    assert [t for o in ev["again"] for t in o.token_ids] == [t for o in ev["warm"] for t in o.token_ids]


def test_batch_invariant_engine_scores_the_right_hidden_rows():
    """Batch-invariant engine: the alternatives of entry j + 1 (ids and fp32 bits) equal
    the first-token ``logprobs=20`` alternatives of a request whose prompt is P[:j + 1]:
    the hidden row of position j reached the LM head."""
    eng = _engine(model="tiny-2k", batch_invariant=True, max_model_len=1024)
    assert eng.runner.model.invariant
    prompt = _prompts([48], seed=21)[0]
    got = []
    eng.add_request("p", prompt, SamplingParams(temperature=0.0, max_tokens=1, ignore_eos=True,
                                                prompt_logprobs=20), on_output=got.append)
    _drain(eng, None)
    plp = got[0].prompt_logprobs
    assert len(plp) == 48
    for j in (1, 7, 33):
        first = []
        eng.add_request(f"q{j}", prompt[:j + 1], SamplingParams(temperature=0.0, max_tokens=1,
                                                                 ignore_eos=True, logprobs=20),
                        on_output=first.append)
        _drain(eng, None)
        alts = first[0].logprobs[0][2]
        assert len(alts) == 20 and [a for a, _ in alts] == [a for a, _ in plp[j + 1][3]]
        assert np.array_equal(np.array([v for _, v in alts], np.float32).view(np.uint32),
                              np.array([v for _, v in plp[j + 1][3]], np.float32).view(np.uint32))


def test_checked_build_passes_this_file():
    """The bounds-checked kernel build (FT_KERNEL_CHECKS=1: target id < V, want <= 20)
    runs the tests above in a child process without a violation."""
    env = dict(os.environ, FT_KERNEL_CHECKS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "not checked_build", os.path.abspath(__file__)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-2000:]
