"""``logprobs`` / ``top_logprobs`` through the OpenAI facade on the CPU backend: the
non-streaming and the streaming shape, token bytes, and the 400s."""
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


BODY = {"messages": [{"role": "user", "content": "hi"}], "max_tokens": 12, "temperature": 0,
        "seed": 7, "ignore_eos": True}


def _stream(client, body):
    """(chunks' choices, concatenated content) of a streamed completion."""
    choices, text = [], []
    with client.stream("POST", "/v1/chat/completions", json=dict(body, stream=True)) as r:
        assert r.status_code == 200
        for line in r.iter_lines():
            if not line.startswith("data: ") or line == "data: [DONE]":
                continue
            ch = json.loads(line[6:])["choices"][0]
            choices.append(ch)
            text.append(ch["delta"].get("content") or "")
    return choices, "".join(text)


def test_non_streaming_and_streaming_logprobs(client):
    body = dict(BODY, logprobs=True, top_logprobs=3)
    r = client.post("/v1/chat/completions", json=body)
    assert r.status_code == 200
    choice = r.json()["choices"][0]
    content = choice["logprobs"]["content"]
    assert len(content) == r.json()["usage"]["completion_tokens"] == 12
    raw = b""
    for item in content:
        assert set(item) == {"token", "logprob", "bytes", "top_logprobs"}
        assert item["token"] == bytes(item["bytes"]).decode("utf-8", errors="replace")
        assert item["logprob"] <= 0.0
        alts = item["top_logprobs"]
        assert len(alts) == 3 and all(set(a) == {"token", "logprob", "bytes"} for a in alts)
        assert [a["logprob"] for a in alts] == sorted((a["logprob"] for a in alts), reverse=True)
        assert alts[0]["logprob"] >= item["logprob"]
        # greedy: the sampled token is the most likely one
        assert alts[0]["bytes"] == item["bytes"] and alts[0]["logprob"] == item["logprob"]
        raw += bytes(item["bytes"])
    assert raw.decode("utf-8", errors="replace") == choice["message"]["content"]

    chunks, text = _stream(client, body)
    assert text == choice["message"]["content"]
    streamed = [it for ch in chunks for it in (ch.get("logprobs") or {}).get("content", [])]
    assert streamed == content
    # every content chunk carries the entries of its delta
    assert all("logprobs" in ch for ch in chunks if ch["delta"].get("content"))


def test_logprobs_without_alternatives(client):
    r = client.post("/v1/chat/completions", json=dict(BODY, logprobs=True)).json()
    content = r["choices"][0]["logprobs"]["content"]
    assert len(content) == 12 and all(it["top_logprobs"] == [] for it in content)


def test_without_the_fields_there_is_no_logprobs_key(client):
    r = client.post("/v1/chat/completions", json=BODY)
    assert r.status_code == 200 and "logprobs" not in r.text
    r = client.post("/v1/chat/completions", json=dict(BODY, logprobs=False))
    assert r.status_code == 200 and "logprobs" not in r.text
    chunks, _ = _stream(client, BODY)
    assert chunks and all(set(ch) == {"index", "delta", "finish_reason"} for ch in chunks)


@pytest.mark.parametrize("extra,word", [
    (dict(logprobs=True, top_logprobs=21), "top_logprobs"),
    (dict(top_logprobs=3), "logprobs"),
    (dict(logprobs=True, top_logprobs=2.5), "integer"),
    (dict(logprobs=True, top_logprobs="3"), "integer"),
    (dict(logprobs=True, top_logprobs=2, tools=[{"type": "function", "function": {
        "name": "get_current_time", "parameters": {"type": "object", "properties": {}}}}]), "tools"),
    (dict(logprobs=True, response_format={"type": "json_schema", "json_schema": {"schema": {
        "type": "object", "properties": {"n": {"type": "integer"}}, "required": ["n"]}}}), "json_schema"),
])
def test_bad_requests_are_400(client, extra, word):
    r = client.post("/v1/chat/completions", json=dict(BODY, **extra))
    assert r.status_code == 400, r.text
    err = r.json()["error"]
    assert err["type"] == "invalid_request_error" and word in err["message"]


def test_tensor_parallel_engines_refuse(client, engine):
    cfg = engine.engine.cfg
    old, cfg.tp_size = cfg.tp_size, 2
    try:
        r = client.post("/v1/chat/completions", json=dict(BODY, logprobs=True))
        assert r.status_code == 400 and "tensor parallelism" in r.json()["error"]["message"]
        assert client.post("/v1/chat/completions", json=BODY).status_code == 200
    finally:
        cfg.tp_size = old
