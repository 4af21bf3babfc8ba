"""min_p through the public interfaces on the CPU backend: the ``/ws/llm`` generation keys,
the OpenAI facade (vLLM's extension field), DEFAULT_MIN_P and what the remote providers
forward (vLLM: a body field, Ollama: ``options.min_p``)."""
import re

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


ENV = {"LLM_PROVIDER": "native", "ENABLE_PYDANTIC_AI": "false", "COMPUTE_DEVICE": "cpu",
       "LLM_MAX_CONNECTIONS": "4"}


@pytest.fixture()
def server(monkeypatch, engine):
    from app.core.websocket_server_vllm import WebSocketLLMServer

    for k, v in ENV.items():
        monkeypatch.setenv(k, v)
    return WebSocketLLMServer(Config(), engine=engine)


@pytest.fixture()
def spy(engine):
    """The SamplingParams of every request the handler hands the engine."""
    seen = []
    orig = engine.generate

    def generate(prompt_ids, params, request_id=None):
        seen.append(params)
        return orig(prompt_ids, params, request_id=request_id)

    engine.generate = generate
    yield seen
    engine.generate = orig


def _until_complete(ws):
    for _ in range(200):
        if ws.receive_json()["type"] == "response_complete":
            return
    raise AssertionError("no response_complete")


def test_ws_start_session_and_update_config(server, spy):
    c = TestClient(server.app)
    with c.websocket_connect("/ws/llm") as ws:
        sid = ws.receive_json()["session_id"]
        ws.send_json({"type": "start_session", "config": {"min_p": 1.5}})
        err = ws.receive_json()
        assert err["type"] == "error" and "min_p" in err["error"]["message"]
        assert not server.conversation_manager.has_session(sid)
        ws.send_json({"type": "start_session", "config": {
            "temperature": 0.9, "max_tokens": 4, "ignore_eos": True, "seed": 3, "min_p": 0.2}})
        assert ws.receive_json()["type"] == "session_configured"
        ws.send_json({"type": "user_message", "text": "Hello there"})
        _until_complete(ws)
        assert spy[-1].min_p == 0.2 and spy[-1].temperature == 0.9
        ws.send_json({"type": "update_config", "config": {"min_p": 0.05}})
        assert ws.receive_json()["type"] == "config_updated"
        ws.send_json({"type": "user_message", "text": "again"})
        _until_complete(ws)
        assert spy[-1].min_p == 0.05
        for bad in (True, -0.1, "x"):
            ws.send_json({"type": "update_config", "config": {"min_p": bad}})
            err = ws.receive_json()
            assert err["type"] == "error" and "min_p" in err["error"]["message"], bad
        ws.send_json({"type": "user_message", "text": "once more"})
        _until_complete(ws)
        assert spy[-1].min_p == 0.05


def test_default_min_p(monkeypatch, engine, spy):
    from app.core.websocket_server_vllm import WebSocketLLMServer

    for k, v in dict(ENV, DEFAULT_MIN_P="0.1").items():
        monkeypatch.setenv(k, v)
    cfg = Config()
    assert cfg.default_min_p == 0.1 and cfg.to_dict()["default_min_p"] == 0.1
    c = TestClient(WebSocketLLMServer(cfg, engine=engine).app)
    body = {"messages": [{"role": "user", "content": "hi"}], "max_tokens": 3}
    assert c.post("/v1/chat/completions", json=body).status_code == 200
    assert spy[-1].min_p == 0.1
    assert c.post("/v1/chat/completions", json=dict(body, min_p=0.4)).status_code == 200
    assert spy[-1].min_p == 0.4
    with c.websocket_connect("/ws/llm") as ws:
        ws.receive_json()
        ws.send_json({"type": "start_session", "config": {"max_tokens": 3}})
        assert ws.receive_json()["type"] == "session_configured"
        ws.send_json({"type": "user_message", "text": "Hello"})
        _until_complete(ws)
        assert spy[-1].min_p == 0.1
    monkeypatch.delenv("DEFAULT_MIN_P")
    assert Config().default_min_p == 0.0
    monkeypatch.setenv("DEFAULT_MIN_P", "1.5")
    with pytest.raises(ValueError, match="min_p"):
        Config()


def _norm(raw: bytes) -> bytes:
    raw = re.sub(rb"chatcmpl-[0-9a-f]{24}", b"chatcmpl-X", raw)
    return re.sub(rb'"created": ?\d+', b'"created":0', raw)


def test_facade_accepts_min_p_and_leaves_other_requests_alone(server, spy):
    c = TestClient(server.app)
    body = {"messages": [{"role": "user", "content": "hi"}], "max_tokens": 6, "temperature": 0.8,
            "seed": 11, "ignore_eos": True}
    r = c.post("/v1/chat/completions", json=dict(body, min_p=0.25))
    assert r.status_code == 200 and r.json()["usage"]["completion_tokens"] == 6
    assert spy[-1].min_p == 0.25
    for bad in (2, -0.5, True, "lots"):
        e = c.post("/v1/chat/completions", json=dict(body, min_p=bad))
        assert e.status_code == 400 and "min_p" in e.json()["error"]["message"], bad
    # without the field: the parameters and the bytes of a request that never heard of it
    n = len(spy)
    plain = c.post("/v1/chat/completions", json=body)
    assert plain.status_code == 200 and len(spy) == n + 1
    assert spy[-1].min_p == 0.0 and not spy[-1].has_penalties
    for same in (dict(body, min_p=None), dict(body, min_p=0)):
        again = c.post("/v1/chat/completions", json=same)
        assert _norm(again.content) == _norm(plain.content)
    with c.stream("POST", "/v1/chat/completions", json=dict(body, stream=True)) as s:
        sse = b"".join(s.iter_bytes())
    with c.stream("POST", "/v1/chat/completions", json=dict(body, stream=True, min_p=0)) as s:
        assert _norm(b"".join(s.iter_bytes())) == _norm(sse)
    assert sse.rstrip().endswith(b"data: [DONE]") and b"min_p" not in sse
    assert b"min_p" not in plain.content
    with c.stream("POST", "/v1/chat/completions",
                  json=dict(body, stream=True, min_p=0.25)) as s:
        assert b"data: [DONE]" in b"".join(s.iter_bytes())
    assert spy[-1].min_p == 0.25


def test_remote_providers_forward_min_p():
    from app.core.ollama_handler import OllamaHandler
    from app.core.vllm_handler import VLLMHandler, remote_penalties

    assert remote_penalties({"min_p": 0.05}) == {"min_p": 0.05}
    assert remote_penalties({"min_p": 0.0, "presence_penalty": 0.0}) == {}
    h = VLLMHandler.__new__(VLLMHandler)
    h.model = "m"
    msgs = [{"role": "user", "content": "x"}]
    body = h._params(msgs, 0.5, 8, None, None, None, penalties={"min_p": 0.05})
    assert body["min_p"] == 0.05
    assert "min_p" not in h._params(msgs, 0.5, 8, None, None, None, penalties={"min_p": 0.0})
    assert "min_p" not in h._params(msgs, 0.5, 8, None, None, None)

    sent = []

    class _Resp:
        def raise_for_status(self):
            pass

        def iter_content(self, chunk_size=None):
            yield b'{"message": {"content": "ok"}, "done": true}\n'

        def close(self):
            pass

    class _Session:
        def post(self, url, json=None, stream=False, timeout=None):  # noqa: A002
            sent.append(json)
            return _Resp()

    o = OllamaHandler("http://ollama:11434", "llama3.2:1b")
    o.session = _Session()
    assert "".join(o.generate_stream(msgs, penalties={"min_p": 0.1, "repetition_penalty": 1.0})) == "ok"
    assert sent[-1]["options"]["min_p"] == 0.1 and "repeat_penalty" not in sent[-1]["options"]
    "".join(o.generate_stream(msgs, penalties={"min_p": 0.0}))
    assert "min_p" not in sent[-1]["options"]
