"""Sampler penalties through the public interfaces on the CPU backend: the OpenAI facade
(``presence_penalty`` / ``frequency_penalty`` / ``logit_bias`` / vLLM's
``repetition_penalty``), the ``/ws/llm`` generation keys (with Ollama's ``repeat_penalty``),
the service defaults and what the remote providers forward."""
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
def server(monkeypatch, engine):
    from app.core.websocket_server_vllm import WebSocketLLMServer

    for k, v in {"LLM_PROVIDER": "native", "ENABLE_PYDANTIC_AI": "false", "COMPUTE_DEVICE": "cpu",
                 "LLM_MAX_CONNECTIONS": "4"}.items():
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


def test_facade_logit_bias_shapes_the_reply_and_bad_values_are_400(server, engine, spy):
    c = TestClient(server.app)
    tok = engine.engine.tokenizer.encode(" hello")[0]
    body = {"messages": [{"role": "user", "content": "hi"}], "max_tokens": 5, "temperature": 0,
            "ignore_eos": True, "logit_bias": {str(tok): 100}, "presence_penalty": 0.5,
            "repetition_penalty": 1.1}
    r = c.post("/v1/chat/completions", json=body).json()
    assert r["choices"][0]["message"]["content"] == " hello" * 5
    assert r["usage"]["completion_tokens"] == 5
    sp = spy[-1]
    assert sp.logit_bias == {tok: 100.0} and sp.presence_penalty == 0.5
    assert sp.repetition_penalty == 1.1 and sp.frequency_penalty == 0.0
    bad = c.post("/v1/chat/completions", json=dict(body, frequency_penalty=3))
    assert bad.status_code == 400 and "frequency_penalty" in bad.json()["error"]["message"]
    bad = c.post("/v1/chat/completions", json=dict(body, logit_bias={str(tok): 101}))
    assert bad.status_code == 400 and "logit_bias" in bad.json()["error"]["message"]
    plain = c.post("/v1/chat/completions", json={k: v for k, v in body.items() if k not in (
        "logit_bias", "presence_penalty", "repetition_penalty")})
    assert plain.status_code == 200 and not spy[-1].has_penalties


def test_ws_repeat_penalty_in_update_config_reaches_the_engine(server, spy):
    c = TestClient(server.app)
    with c.websocket_connect("/ws/llm") as ws:
        sid = ws.receive_json()["session_id"]
        # a refused start_session config leaves no half-made session behind
        ws.send_json({"type": "start_session", "config": {"frequency_penalty": -9}})
        err = ws.receive_json()
        assert err["type"] == "error" and "frequency_penalty" in err["error"]["message"]
        assert not server.conversation_manager.has_session(sid)
        ws.send_json({"type": "start_session", "config": {
            "temperature": 0.0, "max_tokens": 4, "ignore_eos": True, "frequency_penalty": 0.5}})
        assert ws.receive_json()["type"] == "session_configured"
        ws.send_json({"type": "update_config", "config": {"repeat_penalty": 1.25,
                                                          "logit_bias": {"11": -5}}})
        assert ws.receive_json()["type"] == "config_updated"
        ws.send_json({"type": "user_message", "text": "Hello there"})
        for _ in range(100):
            if ws.receive_json()["type"] == "response_complete":
                break
        sp = spy[-1]
        assert sp.repetition_penalty == 1.25 and sp.frequency_penalty == 0.5
        assert sp.presence_penalty == 0.0 and sp.logit_bias == {11: -5.0}
        ws.send_json({"type": "update_config", "config": {"presence_penalty": 7}})
        err = ws.receive_json()
        assert err["type"] == "error" and "presence_penalty" in err["error"]["message"]
        ws.send_json({"type": "user_message", "text": "again"})
        for _ in range(100):
            if ws.receive_json()["type"] == "response_complete":
                break
        assert spy[-1].presence_penalty == 0.0 and spy[-1].repetition_penalty == 1.25


def test_service_defaults(monkeypatch, engine, spy):
    from app.core.websocket_server_vllm import WebSocketLLMServer

    for k, v in {"LLM_PROVIDER": "native", "ENABLE_PYDANTIC_AI": "false", "COMPUTE_DEVICE": "cpu",
                 "DEFAULT_REPETITION_PENALTY": "1.15", "DEFAULT_FREQUENCY_PENALTY": "0.2"}.items():
        monkeypatch.setenv(k, v)
    cfg = Config()
    assert cfg.to_dict()["default_repetition_penalty"] == 1.15
    assert cfg.to_dict()["default_presence_penalty"] == 0.0
    c = TestClient(WebSocketLLMServer(cfg, engine=engine).app)
    r = c.post("/v1/chat/completions", json={"messages": [{"role": "user", "content": "hi"}],
                                             "max_tokens": 3, "presence_penalty": 1.0})
    assert r.status_code == 200
    sp = spy[-1]
    assert (sp.repetition_penalty, sp.presence_penalty, sp.frequency_penalty) == (1.15, 1.0, 0.2)
    monkeypatch.setenv("DEFAULT_PRESENCE_PENALTY", "2.5")
    with pytest.raises(ValueError, match="presence_penalty"):
        Config()


def test_remote_providers_forward_what_their_backend_understands():
    from app.core.vllm_handler import VLLMHandler, remote_penalties

    pen = {"repetition_penalty": 1.2, "presence_penalty": 0.0, "frequency_penalty": 0.4,
           "logit_bias": {5: 2.0}}
    assert remote_penalties(pen) == {"repetition_penalty": 1.2, "frequency_penalty": 0.4,
                                     "logit_bias": {"5": 2.0}}
    assert remote_penalties(None) == {}
    h = VLLMHandler.__new__(VLLMHandler)
    h.model = "m"
    body = h._params([{"role": "user", "content": "x"}], 0.5, 8, None, None, None, penalties=pen)
    assert body["repetition_penalty"] == 1.2 and body["logit_bias"] == {"5": 2.0}
    assert "presence_penalty" not in body
