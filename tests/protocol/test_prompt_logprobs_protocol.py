"""``prompt_logprobs`` through the OpenAI facade on the CPU backend: the chat field, the
``/v1/completions`` endpoint (plain, streamed, ``echo`` + ``logprobs``, token-id
prompts) and every 400."""
import json

import pytest
from starlette.testclient import TestClient

from app.utils.config import Config
from fasttalk_llm_microservice_amd.engine.config import EngineConfig
from fasttalk_llm_microservice_amd.engine.engine import AsyncEngine, LLMEngine


@pytest.fixture(scope="module")
def engine():
    eng = AsyncEngine(LLMEngine(EngineConfig(model="tiny", device="cpu", num_kv_blocks=256,
                                             max_model_len=1024, max_num_seqs=8))).start()
    yield eng
    eng.shutdown()


@pytest.fixture()
def client(monkeypatch, engine):
    from app.core.websocket_server_vllm import WebSocketLLMServer

    for k, v in {"LLM_PROVIDER": "native", "ENABLE_PYDANTIC_AI": "false", "COMPUTE_DEVICE": "cpu",
                 "LLM_MAX_CONNECTIONS": "4"}.items():
        monkeypatch.setenv(k, v)
    return TestClient(WebSocketLLMServer(Config(), engine=engine).app)


CHAT = {"messages": [{"role": "user", "content": "hi there"}], "max_tokens": 4, "temperature": 0,
        "seed": 7, "ignore_eos": True}
TEXT = "The quick brown fox jumps over the lazy dog"
COMP = {"prompt": TEXT, "max_tokens": 5, "temperature": 0, "ignore_eos": True}


def _check_plp(plp, n_alt):
    assert plp[0] is None and len(plp) > 2
    for entry in plp[1:]:
        assert n_alt <= len(entry) <= n_alt + 1
        items = list(entry.items())
        assert all(set(v) == {"logprob", "rank", "decoded_token"} for _, v in items)
        assert all(str(int(k)) == k for k, _ in items)
        assert all(v["logprob"] <= 0.0 and v["rank"] >= 1 for _, v in items)
        tok, alts = items[0][1], [v for _, v in items[1:]]
        if len(entry) == n_alt:   # the prompt token is itself an alternative: listed once
            assert tok["rank"] <= n_alt
            others = sorted(set(range(1, n_alt + 1)) - {tok["rank"]})
        else:
            assert tok["rank"] > n_alt or n_alt == 0 or tok["logprob"] <= alts[-1]["logprob"]
            others = list(range(1, n_alt + 1))
        assert [a["rank"] for a in alts] == others
        assert [a["logprob"] for a in alts] == sorted((a["logprob"] for a in alts), reverse=True)


def test_chat_field_shape_and_absence(client):
    plain = client.post("/v1/chat/completions", json=CHAT)
    assert plain.status_code == 200 and "prompt_logprobs" not in plain.json()
    r = client.post("/v1/chat/completions", json=dict(CHAT, prompt_logprobs=3))
    assert r.status_code == 200
    body = r.json()
    assert len(body["prompt_logprobs"]) == body["usage"]["prompt_tokens"]
    _check_plp(body["prompt_logprobs"], 3)
    assert body["choices"][0]["message"] == plain.json()["choices"][0]["message"]
    assert set(body) - {"prompt_logprobs"} == set(plain.json())
    zero = client.post("/v1/chat/completions", json=dict(CHAT, prompt_logprobs=0)).json()
    assert all(len(e) == 1 for e in zero["prompt_logprobs"][1:])
    # the prompt token's entries do not depend on how many alternatives are asked
    for a, b in zip(zero["prompt_logprobs"][1:], body["prompt_logprobs"][1:]):
        (k, v), = a.items()
        assert b[k]["rank"] == v["rank"] and abs(b[k]["logprob"] - v["logprob"]) < 1e-4


@pytest.mark.parametrize("extra", [
    {"stream": True},
    {"tools": [{"type": "function", "function": {"name": "f", "parameters": {"type": "object"}}}]},
    {"response_format": {"type": "json_schema", "json_schema": {"schema": {"type": "object"}}}},
], ids=["stream", "tools", "json_schema"])
def test_chat_400_combinations(client, extra):
    r = client.post("/v1/chat/completions", json=dict(CHAT, prompt_logprobs=1, **extra))
    assert r.status_code == 400 and "prompt_logprobs" in r.json()["error"]["message"]


@pytest.mark.parametrize("bad", [-1, 21, 1.5, "2", True])
def test_chat_400_bad_values(client, bad):
    r = client.post("/v1/chat/completions", json=dict(CHAT, prompt_logprobs=bad))
    assert r.status_code == 400 and "prompt_logprobs" in r.json()["error"]["message"]


def test_400_on_a_tensor_parallel_engine(client, engine, monkeypatch):
    monkeypatch.setattr(engine.engine.cfg, "tp_size", 2)
    r = client.post("/v1/chat/completions", json=dict(CHAT, prompt_logprobs=1))
    assert r.status_code == 400 and "tensor parallelism" in r.json()["error"]["message"]
    r = client.post("/v1/completions", json=dict(COMP, prompt_logprobs=1))
    assert r.status_code == 400 and "tensor parallelism" in r.json()["error"]["message"]
    r = client.post("/v1/completions", json=dict(COMP, logprobs=1, echo=True))
    assert r.status_code == 400 and "tensor parallelism" in r.json()["error"]["message"]


# --------------------------------------------------------------------- /v1/completions
def test_plain_completion_and_the_sse_stream(client):
    r = client.post("/v1/completions", json=COMP)
    assert r.status_code == 200
    body = r.json()
    assert body["object"] == "text_completion"
    choice = body["choices"][0]
    assert choice["finish_reason"] == "length" and choice["logprobs"] is None
    assert "prompt_logprobs" not in choice
    assert body["usage"]["completion_tokens"] == 5 and isinstance(choice["text"], str)
    n_prompt = body["usage"]["prompt_tokens"]
    # BOS is prepended to a string prompt unless add_special_tokens is false
    r2 = client.post("/v1/completions", json=dict(COMP, add_special_tokens=False)).json()
    assert r2["usage"]["prompt_tokens"] == n_prompt - 1
    # the default max_tokens is 16
    r3 = client.post("/v1/completions", json={"prompt": TEXT, "temperature": 0, "ignore_eos": True})
    assert r3.json()["usage"]["completion_tokens"] == 16

    text, finish = [], None
    with client.stream("POST", "/v1/completions", json=dict(COMP, stream=True)) as s:
        assert s.status_code == 200
        lines = [ln for ln in s.iter_lines() if ln.startswith("data: ")]
    assert lines[-1] == "data: [DONE]"
    for ln in lines[:-1]:
        ev = json.loads(ln[6:])
        assert ev["object"] == "text_completion"
        text.append(ev["choices"][0]["text"])
        finish = ev["choices"][0]["finish_reason"] or finish
    assert "".join(text) == choice["text"] and finish == "length"


def test_completion_logprobs_without_echo(client):
    r = client.post("/v1/completions", json=dict(COMP, logprobs=2)).json()
    lp = r["choices"][0]["logprobs"]
    assert set(lp) == {"tokens", "token_logprobs", "top_logprobs", "text_offset"}
    assert len(lp["tokens"]) == len(lp["token_logprobs"]) == len(lp["top_logprobs"]) == \
        len(lp["text_offset"]) == 5
    assert "".join(lp["tokens"]) == r["choices"][0]["text"]
    assert lp["text_offset"][0] == 0 and lp["text_offset"] == sorted(lp["text_offset"])
    for tok, tlp, top in zip(lp["tokens"], lp["token_logprobs"], lp["top_logprobs"]):
        assert tlp <= 0.0 and 2 <= len(top) <= 3 and top[tok] == tlp   # greedy: the top one
        assert max(top.values()) == tlp


def test_echo_logprobs_with_max_tokens_zero_scores_the_prompt(client):
    r = client.post("/v1/completions", json=dict(COMP, echo=True, logprobs=1, max_tokens=0))
    assert r.status_code == 200
    body = r.json()
    choice, n = body["choices"][0], body["usage"]["prompt_tokens"]
    lp = choice["logprobs"]
    assert len(lp["tokens"]) == len(lp["token_logprobs"]) == len(lp["top_logprobs"]) == \
        len(lp["text_offset"]) == n
    assert lp["token_logprobs"][0] is None and lp["top_logprobs"][0] is None
    assert all(isinstance(v, float) and v <= 0.0 for v in lp["token_logprobs"][1:])
    assert all(1 <= len(t) <= 2 for t in lp["top_logprobs"][1:])
    assert choice["text"] == TEXT and choice["finish_reason"] == "length"
    assert body["usage"]["completion_tokens"] == 0 and body["usage"]["total_tokens"] == n
    # the tokens behind the BOS spell the prompt, and the offsets index into it
    assert "".join(lp["tokens"][1:]) == TEXT
    assert all(TEXT[o:].startswith(t) for o, t in zip(lp["text_offset"][1:], lp["tokens"][1:]))
    # with tokens to generate the arrays go on behind the prompt's
    more = client.post("/v1/completions", json=dict(COMP, echo=True, logprobs=1, max_tokens=3)).json()
    mlp = more["choices"][0]["logprobs"]
    assert len(mlp["tokens"]) == n + 3 and mlp["tokens"][:n] == lp["tokens"]
    assert more["choices"][0]["text"].startswith(TEXT) and more["usage"]["completion_tokens"] == 3
    for a, b in zip(mlp["token_logprobs"][1:n], lp["token_logprobs"][1:]):
        assert abs(a - b) < 1e-4
    # the same scores in vLLM's format
    plp = client.post("/v1/completions", json=dict(COMP, prompt_logprobs=1, max_tokens=1)).json()
    entries = plp["choices"][0]["prompt_logprobs"]
    assert len(entries) == n
    _check_plp(entries, 1)
    for e, v in zip(entries[1:], lp["token_logprobs"][1:]):
        assert abs(next(iter(e.values()))["logprob"] - v) < 1e-4


def test_token_id_prompts_are_used_as_they_are(client):
    ids = [11, 2022, 303, 44, 5005, 66]
    r = client.post("/v1/completions", json=dict(COMP, prompt=ids, prompt_logprobs=0, max_tokens=2))
    assert r.status_code == 200
    body = r.json()
    assert body["usage"]["prompt_tokens"] == len(ids)   # no BOS added
    plp = body["choices"][0]["prompt_logprobs"]
    assert plp[0] is None and [next(iter(e)) for e in plp[1:]] == [str(t) for t in ids[1:]]


@pytest.mark.parametrize("extra, word", [
    ({"prompt": ["a", "b"]}, "one prompt"),
    ({"prompt": [[1, 2], [3, 4]]}, "one prompt"),
    ({"prompt": None}, "prompt is required"),
    ({"prompt": []}, "prompt is required"),
    ({"prompt": [1, 10 ** 9]}, "token ids"),
    ({"n": 2}, "n above 1"),
    ({"best_of": 3}, "best_of above 1"),
    ({"suffix": "x"}, "suffix"),
    ({"max_tokens": 0}, "echo"),
    ({"max_tokens": -1}, "max_tokens"),
    ({"echo": "yes"}, "echo"),
    ({"logprobs": 21}, "logprobs"),
    ({"logprobs": True}, "logprobs"),
    ({"logprobs": -1}, "logprobs"),
    ({"prompt_logprobs": 21}, "prompt_logprobs"),
    ({"prompt_logprobs": "1"}, "prompt_logprobs"),
    ({"stream": True, "echo": True}, "stream"),
    ({"stream": True, "prompt_logprobs": 1}, "stream"),
    ({"min_p": 2.0}, "min_p"),
])
def test_completions_400(client, extra, word):
    r = client.post("/v1/completions", json=dict(COMP, **extra))
    assert r.status_code == 400, r.text
    assert word in r.json()["error"]["message"]
