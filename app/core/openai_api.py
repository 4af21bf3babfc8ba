"""OpenAI-compatible facade over the in-process engine (E1): ``GET /v1/models``,
``POST /v1/chat/completions`` (``stream`` via SSE, ``tools`` with server-side
hermes / llama3_json parsing like vLLM's ``--enable-auto-tool-choice``,
``tool_choice="required"`` or a named function -> JSON-schema guided decoding),
``POST /v1/completions`` (token scoring: ``echo`` + ``logprobs``, ``prompt_logprobs``),
``GET /health`` is on the main app.  Existing OpenAI/vLLM clients -- including
the reference's ``VLLMHandler`` / pydantic-ai agent -- can point their
``base_url`` at ``http://host:8000/v1``.
"""
from __future__ import annotations

import json
import time
import uuid
from typing import Any, Dict, List

from fastapi import Request
from fastapi.responses import JSONResponse, StreamingResponse


def _bad_request(msg: str):
    return JSONResponse({"error": {"message": msg, "type": "invalid_request_error"}},
                        status_code=400)


def _tp_size(handler) -> int:
    inner = getattr(handler.engine, "engine", handler.engine)
    return int(getattr(getattr(inner, "cfg", None), "tp_size", 1) or 1)


def _clip(lp: float) -> float:
    # JSON has no infinity: -inf goes out as -9999.0 (vLLM's convention)
    return lp if lp > -9999.0 else -9999.0


def _tok_str(tok_bytes, tid: int) -> str:
    b = tok_bytes[tid] if 0 <= tid < len(tok_bytes) else b""
    return b.decode("utf-8", errors="replace")


def prompt_logprobs_json(entries, tok_bytes, n: int) -> List[Any]:
    """vLLM's ``prompt_logprobs`` list of RequestOutput.prompt_logprobs: ``null`` for the
    first prompt token, then per token ``{"<token id>": {"logprob", "rank",
    "decoded_token"}}`` holding the prompt token (its counted rank) and the ``n`` most
    likely alternatives (rank = their 1-based position); a prompt token that is itself
    an alternative appears once, with its counted rank."""
    out: List[Any] = []
    for e in entries or ():
        if e is None:
            out.append(None)
            continue
        tid, lp, rank, alts = e
        d = {str(tid): {"logprob": _clip(lp), "rank": rank, "decoded_token": _tok_str(tok_bytes, tid)}}
        for pos, (a, alp) in enumerate(alts[:n], 1):
            if a != tid:
                d[str(a)] = {"logprob": _clip(alp), "rank": pos,
                             "decoded_token": _tok_str(tok_bytes, a)}
        out.append(d)
    return out


def register_openai_routes(app, handler) -> None:
    @app.get("/v1/models")
    async def models():
        return {"object": "list", "data": [{"id": handler.model, "object": "model",
                                             "created": int(time.time()), "owned_by": "fasttalk"}]}

    @app.post("/v1/chat/completions")
    async def chat_completions(request: Request):
        from fasttalk_llm_microservice_amd.engine.guided import GuidedSpec
        from fasttalk_llm_microservice_amd.engine.tool_parser import (StreamingToolCallParser,
                                                                       StreamingToolDetector,
                                                                       parse_tool_calls)

        try:
            body = await request.json()
        except Exception:
            return JSONResponse({"error": {"message": "invalid JSON body"}}, status_code=400)
        messages: List[Dict[str, Any]] = body.get("messages") or []
        if not messages:
            return JSONResponse({"error": {"message": "messages is required"}}, status_code=400)
        tools = body.get("tools") or None
        tool_choice = body.get("tool_choice", "auto")
        guided = None
        if tools and (tool_choice == "required" or isinstance(tool_choice, dict)):
            pick = tools
            if isinstance(tool_choice, dict):
                name = (tool_choice.get("function") or {}).get("name")
                pick = [t for t in tools if (t.get("function") or t).get("name") == name] or tools
            guided = GuidedSpec.tool_call(pick)
        rf = body.get("response_format") or {}
        if guided is None and rf.get("type") == "json_schema":
            guided = GuidedSpec.json_schema((rf.get("json_schema") or {}).get("schema") or {})
        stop = body.get("stop")
        if isinstance(stop, str):
            stop = [stop]
        kw = dict(temperature=body.get("temperature", 1.0), max_tokens=body.get("max_tokens")
                  or body.get("max_completion_tokens"), top_p=body.get("top_p"),
                  top_k=body.get("top_k"), stop=stop, tools=tools, guided=guided,
                  seed=body.get("seed"), ignore_eos=bool(body.get("ignore_eos", False)),
                  min_tokens=int(body.get("min_tokens") or 0))
        # presence_penalty / frequency_penalty / logit_bias, and vLLM's repetition_penalty
        # and min_p (it travels with the penalties)
        from fasttalk_llm_microservice_amd.engine.sampling_params import (pick_logprobs,
                                                                           pick_min_p,
                                                                           pick_penalties,
                                                                           pick_prompt_logprobs)

        def bad_request(msg: str):
            return JSONResponse({"error": {"message": msg, "type": "invalid_request_error"}},
                                status_code=400)

        try:
            pen = pick_penalties(body)
            pen.update(pick_min_p(body))
            kw["penalties"] = pen or None
            want_lp = pick_logprobs(body)
            want_plp = pick_prompt_logprobs(body)
        except (ValueError, TypeError) as e:
            return bad_request(str(e))
        if want_plp is not None:
            # vLLM's prompt_logprobs: every prompt token's logprob and rank.  Not streamed,
            # not with a grammar (its forced head joins the prompt) or tools, nor under TP.
            if body.get("stream"):
                return bad_request("prompt_logprobs are not supported with stream: true")
            if tools or guided is not None:
                return bad_request("prompt_logprobs are not supported with tools or "
                                   "response_format json_schema")
            if _tp_size(handler) > 1:
                return bad_request("prompt_logprobs are not supported with tensor parallelism yet")
            kw["prompt_logprobs"] = want_plp
        if pen.get("min_p"):
            inner = getattr(handler.engine, "engine", handler.engine)
            if int(getattr(getattr(inner, "cfg", None), "tp_size", 1) or 1) > 1:
                return bad_request("min_p is not supported with tensor parallelism yet")
        if want_lp is not None:
            # logprobs / top_logprobs: per-token logprobs over the raw logits.  Not with a
            # grammar (forced tokens have no sampled logit) nor tool parsing, nor under TP.
            if tools or guided is not None:
                return bad_request("logprobs are not supported with tools or response_format "
                                   "json_schema")
            inner = getattr(handler.engine, "engine", handler.engine)
            if int(getattr(getattr(inner, "cfg", None), "tp_size", 1) or 1) > 1:
                return bad_request("logprobs are not supported with tensor parallelism yet")
            kw["logprobs"] = want_lp
        tok_bytes = handler.tokenizer.id_to_bytes if want_lp is not None else None

        def lp_item(tid: int, lp: float) -> Dict[str, Any]:
            b = tok_bytes[tid] if 0 <= tid < len(tok_bytes) else b""
            # JSON has no infinity: -inf goes out as -9999.0 (vLLM's convention)
            return {"token": b.decode("utf-8", errors="replace"),
                    "logprob": lp if lp > -9999.0 else -9999.0, "bytes": list(b)}

        def lp_content(entries) -> List[Dict[str, Any]]:
            """OpenAI ``logprobs.content`` items of an event's RequestOutput.logprobs."""
            return [dict(lp_item(tid, lp), top_logprobs=[lp_item(a, alp) for a, alp in alts])
                    for tid, lp, alts in entries or ()]

        rid = f"chatcmpl-{uuid.uuid4().hex[:24]}"
        created = int(time.time())
        model = body.get("model") or handler.model

        def chunk(delta: Dict[str, Any], finish=None, lps=None) -> str:
            choice = {"index": 0, "delta": delta, "finish_reason": finish}
            if lps is not None:
                choice["logprobs"] = {"content": lps}
            return "data: " + json.dumps({"id": rid, "object": "chat.completion.chunk",
                                          "created": created, "model": model,
                                          "choices": [choice]}) + "\n\n"

        if body.get("stream"):
            async def gen():
                """With ``tools``, the first visible characters decide (like vLLM's
                auto tool choice): speech streams as ``content`` deltas at once; a
                tool call streams as ``tool_calls`` deltas -- id + name as soon as
                the name is complete, then argument fragments as they decode."""
                yield chunk({"role": "assistant", "content": ""})
                finish = "stop"
                det = StreamingToolDetector() if tools else None
                names = [(t.get("function") or t).get("name") for t in tools or []]
                tcp = StreamingToolCallParser(names) if tools else None
                any_call = False
                tool_text = []   # what the parser consumed, re-sent as content if no call
                # logprob entries not sent yet: an event without text (partial UTF-8) sends
                # no chunk, its entries go out with the next chunk or the final one
                held: List[Dict[str, Any]] = []
                async for out in handler.stream_events(messages, request_id=rid, **kw):
                    if out.finished:
                        finish = out.finish_reason
                    if want_lp is not None:
                        held += lp_content(out.logprobs)
                    if not out.text:
                        continue
                    if det is None:
                        if want_lp is not None:
                            yield chunk({"content": out.text}, lps=held)
                            held = []
                        else:
                            yield chunk({"content": out.text})
                        continue
                    mode, emit = det.feed(out.text)
                    if mode == "text":
                        if emit:
                            yield chunk({"content": emit})
                    elif mode == "tool":
                        held, det.buf = det.buf, ""   # the parser owns the tool text now
                        tool_text.append(held)
                        deltas = tcp.feed(held)
                        if deltas:
                            any_call = True
                            yield chunk({"tool_calls": deltas})
                if det is not None and det.mode is None and det.buf:
                    yield chunk({"content": det.buf})   # never became a tool call
                elif det is not None and det.mode == "tool" and not any_call and tool_text:
                    # looked like a call ('{', a tag) but no call of a requested tool
                    # came out of it: it was text (e.g. a JSON answer)
                    yield chunk({"content": "".join(tool_text)})
                if any_call:
                    finish = "tool_calls"
                yield chunk({}, finish if finish in ("stop", "length", "tool_calls") else "stop",
                            lps=held or None)
                yield "data: [DONE]\n\n"

            return StreamingResponse(gen(), media_type="text/event-stream")

        parts: List[str] = []
        n_prompt = n_out = 0
        finish = "stop"
        lp_all: List[Dict[str, Any]] = []
        plp = None
        async for out in handler.stream_events(messages, request_id=rid, **kw):
            if plp is None:
                plp = out.prompt_logprobs
            parts.append(out.text)
            n_out += len(out.token_ids)
            if want_lp is not None:
                lp_all += lp_content(out.logprobs)
            n_prompt = out.num_prompt_tokens or n_prompt
            if out.finished:
                finish = out.finish_reason
        text = "".join(parts)
        msg: Dict[str, Any] = {"role": "assistant", "content": text}
        if tools:
            calls, rest = parse_tool_calls(text)
            names = {(t.get("function") or t).get("name") for t in tools}
            if calls and all(c.name in names for c in calls):
                msg = {"role": "assistant", "content": rest or None,
                       "tool_calls": [c.to_openai() for c in calls]}
                finish = "tool_calls"
        choice = {"index": 0, "message": msg,
                  "finish_reason": finish if finish in ("stop", "length", "tool_calls") else "stop"}
        if want_lp is not None:
            choice["logprobs"] = {"content": lp_all}
        resp = {"id": rid, "object": "chat.completion", "created": created, "model": model,
                "choices": [choice],
                "usage": {"prompt_tokens": n_prompt, "completion_tokens": n_out,
                          "total_tokens": n_prompt + n_out}}
        if want_plp is not None:
            resp["prompt_logprobs"] = prompt_logprobs_json(plp, handler.tokenizer.id_to_bytes,
                                                           want_plp)
        return resp

    @app.post("/v1/completions")
    async def completions(request: Request):
        """Legacy text completions, for scoring: a string or token-id ``prompt``, ``echo`` +
        ``logprobs`` (lm-eval's loglikelihood requests), ``prompt_logprobs``."""
        from fasttalk_llm_microservice_amd.engine.sampling_params import (LOGPROBS_MAX,
                                                                           pick_min_p,
                                                                           pick_penalties,
                                                                           pick_prompt_logprobs)

        try:
            body = await request.json()
        except Exception:
            return JSONResponse({"error": {"message": "invalid JSON body"}}, status_code=400)
        if not isinstance(body, dict):
            return _bad_request("the body must be a JSON object")
        tok = handler.tokenizer
        tok_bytes = tok.id_to_bytes
        prompt = body.get("prompt")
        bos_added = False
        if isinstance(prompt, str):
            ids = tok.encode(prompt)
            if body.get("add_special_tokens", True) is not False:
                ids = [tok.bos_id] + list(ids)
                bos_added = True
            prompt_text = prompt
        elif isinstance(prompt, list) and prompt and \
                all(isinstance(t, int) and not isinstance(t, bool) for t in prompt):
            inner = getattr(handler.engine, "engine", handler.engine)
            vocab = int(getattr(getattr(inner, "model_cfg", None), "vocab_size", 0) or len(tok_bytes))
            if not all(0 <= t < vocab for t in prompt):
                return _bad_request(f"prompt token ids must be in [0, {vocab})")
            ids = list(prompt)
            prompt_text = tok.decode(ids)
        elif isinstance(prompt, list) and prompt:
            return _bad_request("one prompt per request: prompt must be a string or a list of "
                                "token ids")
        else:
            return _bad_request("prompt is required: a string or a list of token ids")
        for k in ("n", "best_of"):
            v = body.get(k)
            if v is not None and v != 1:
                return _bad_request(f"{k} above 1 is not supported")
        if body.get("suffix") is not None:
            return _bad_request("suffix is not supported")
        echo = body.get("echo", False)
        if not isinstance(echo, bool):
            return _bad_request("echo must be true or false")
        want_lp = body.get("logprobs")
        if want_lp is not None and (isinstance(want_lp, bool) or not isinstance(want_lp, int)
                                    or not 0 <= want_lp <= LOGPROBS_MAX):
            return _bad_request(f"logprobs must be an integer in 0..{LOGPROBS_MAX}")
        try:
            want_plp = pick_prompt_logprobs(body)
            pen = pick_penalties(body)
            pen.update(pick_min_p(body))
        except (ValueError, TypeError) as e:
            return _bad_request(str(e))
        max_tokens = body.get("max_tokens", 16)
        if isinstance(max_tokens, bool) or not isinstance(max_tokens, int) or max_tokens < 0:
            return _bad_request("max_tokens must be a non-negative integer")
        if max_tokens == 0 and not echo:
            return _bad_request("max_tokens: 0 is only allowed with echo")
        stream = bool(body.get("stream"))
        if stream and (echo or want_plp is not None):
            return _bad_request("echo and prompt_logprobs are not supported with stream: true")
        tp = _tp_size(handler) > 1
        if tp and want_lp is not None:
            return _bad_request("logprobs are not supported with tensor parallelism yet")
        if tp and (want_plp is not None or pen.get("min_p")):
            return _bad_request("prompt_logprobs and min_p are not supported with tensor "
                                "parallelism yet")
        # echo + logprobs: the arrays cover the prompt too, from the engine's prompt logprobs
        eng_plp = want_plp
        if echo and want_lp is not None:
            eng_plp = max(want_lp, want_plp or 0)
        stop = body.get("stop")
        if isinstance(stop, str):
            stop = [stop]
        kw = dict(temperature=body.get("temperature", 1.0), max_tokens=max(1, max_tokens),
                  top_p=body.get("top_p"), top_k=body.get("top_k"), stop=stop,
                  seed=body.get("seed"), ignore_eos=bool(body.get("ignore_eos", False)),
                  min_tokens=int(body.get("min_tokens") or 0), penalties=pen or None,
                  logprobs=want_lp, prompt_logprobs=eng_plp, prompt_ids=ids)
        rid = f"cmpl-{uuid.uuid4().hex[:24]}"
        created = int(time.time())
        model = body.get("model") or handler.model

        def legacy(entries, first_offset: int) -> Dict[str, Any]:
            """The legacy ``logprobs`` object of (token_id, logprob, alternatives) entries
            (None: a token without a logprob, the first of an echoed prompt)."""
            tokens, tlps, tops, offs = [], [], [], []
            off = first_offset
            for k, e in enumerate(entries):
                tid = e[0]
                piece = "" if (k == 0 and echo and bos_added) else _tok_str(tok_bytes, tid)
                tokens.append(_tok_str(tok_bytes, tid))
                offs.append(off)
                off += len(piece)
                if e[1] is None:
                    tlps.append(None)
                    tops.append(None)
                    continue
                tlps.append(_clip(e[1]))
                top = {_tok_str(tok_bytes, a): _clip(alp) for a, alp in e[2][:want_lp]}
                top.setdefault(_tok_str(tok_bytes, tid), _clip(e[1]))
                tops.append(top)
            return {"tokens": tokens, "token_logprobs": tlps, "top_logprobs": tops,
                    "text_offset": offs}

        def frame(text: str, finish=None, lps=None) -> str:
            return "data: " + json.dumps({"id": rid, "object": "text_completion", "created": created,
                                          "model": model,
                                          "choices": [{"index": 0, "text": text, "logprobs": lps,
                                                       "finish_reason": finish}]}) + "\n\n"

        if stream:
            async def gen():
                finish, off, held = "stop", 0, []
                async for out in handler.stream_events([], request_id=rid, **kw):
                    if out.finished:
                        finish = out.finish_reason
                    if want_lp is not None:
                        held += list(out.logprobs or ())
                    if not out.text:
                        continue
                    yield frame(out.text, lps=legacy(held, off) if want_lp is not None else None)
                    off += len(out.text)
                    held = []
                yield frame("", finish if finish in ("stop", "length") else "stop",
                            lps=legacy(held, off) if held else None)
                yield "data: [DONE]\n\n"

            return StreamingResponse(gen(), media_type="text/event-stream")

        parts: List[str] = []
        n_prompt, n_out, finish = len(ids), 0, "stop"
        gen_lps: List[Any] = []
        plp = None
        async for out in handler.stream_events([], request_id=rid, **kw):
            if plp is None:
                plp = out.prompt_logprobs
            parts.append(out.text)
            n_out += len(out.token_ids)
            gen_lps += list(out.logprobs or ())
            n_prompt = out.num_prompt_tokens or n_prompt
            if out.finished:
                finish = out.finish_reason
        text = "".join(parts)
        if max_tokens == 0:   # the engine ran one token to score the prompt: dropped
            text, n_out, gen_lps, finish = "", 0, [], "length"
        choice: Dict[str, Any] = {"index": 0, "text": (prompt_text + text) if echo else text,
                                  "logprobs": None,
                                  "finish_reason": finish if finish in ("stop", "length") else "stop"}
        if want_lp is not None:
            entries = list(gen_lps)
            if echo:
                head = [(ids[0], None, [])] + [(e[0], e[1], e[3]) for e in (plp or [])[1:]]
                entries = head + entries
            choice["logprobs"] = legacy(entries, 0)
        if want_plp is not None:
            choice["prompt_logprobs"] = prompt_logprobs_json(plp, tok_bytes, want_plp)
        return {"id": rid, "object": "text_completion", "created": created, "model": model,
                "choices": [choice],
                "usage": {"prompt_tokens": n_prompt, "completion_tokens": n_out,
                          "total_tokens": n_prompt + n_out}}
