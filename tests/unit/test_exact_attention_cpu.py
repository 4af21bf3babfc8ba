"""The attention section of ops/exact.py on the CPU: the operand design holds on every
case tests/test_attention_exact_gpu.py runs (exact formats, integer scores, one level per
channel, poison, the visibility condition), the comparison rejects every fault of the
mutation catalogue (the proof that the GPU assertion can fail), and an fp32 model of the
kernels' arithmetic stays inside the asserted tolerance."""
import dataclasses

import pytest
import torch

from fasttalk_llm_microservice_amd.ops import exact as E

ALL = E.attn_all_cases()


def _chunks(cases, n):
    size = -(-len(cases) // n)
    return [cases[i: i + size] for i in range(0, len(cases), size)]


def test_tables_cover_the_dispatchers():
    want = [(128, 1), (128, 2), (128, 3), (128, 4), (128, 8), (64, 1), (64, 2), (64, 4), (64, 8)]
    assert E.attn_instantiated("decode") == want
    assert E.attn_instantiated("prefill") == want
    assert len({c for c in ALL}) == len(ALL)
    # the long case needs more than 64 tiles per wave of a 512-wave grid
    long = [c for c in ALL if c.lens == E.ATTN_LONG_LENS][0]
    assert long.nkv * sum(-(-l // 16) for l in long.lens) > 64 * 512


@pytest.mark.parametrize("part", range(8))
def test_self_checks_and_visibility(part):
    """Every case of the tables: formats, scores, levels, poison, and every key (tile)
    carries at least 3 * 2**-7 of an output element."""
    for c in _chunks(ALL, 8)[part]:
        assert E.attn_self_check(E.attn_operands(c)) >= E.ATTN_MIN_SHARE, c.name


def test_visibility_condition_fires():
    with pytest.raises(AssertionError, match="visibility"):
        E.attn_operands(E.AttnCase("key", (4100,), 2, 2, 64))     # 65 keys per channel
    o = E.attn_operands(E.AttnCase("key", (2100,), 2, 2, 64))     # 33 per channel: v = 1 only
    assert o.v_max == 1
    with pytest.raises(AssertionError, match="e4m3"):
        E._f8_store(torch.tensor([17.0]), "x")


def _logical(c):
    return dataclasses.replace(c, block_size=16, q_pad=0)


MODEL_CASES = sorted({_logical(c) for c in ALL}, key=lambda c: c.name)


@pytest.mark.parametrize("part", range(8))
def test_arithmetic_model_within_tolerance(part):
    """The kernels' arithmetic in fp32 (16-key tiles in 8-tile ranges for decode, 64-key
    tiles in 4-tile ranges for prefill, deferred rescale at 8, bf16 P, online merge) agrees
    with RNE(fp64 reference) to one bf16 step on every case.  Levels, values and lengths do
    not depend on the block size or the q stride, so one layout per case is modelled."""
    for c in _chunks(MODEL_CASES, 8)[part]:
        o = E.attn_operands(c)
        dec = c.q_lens is None
        got = E.attn_model(o, 16 if dec else 64, 8 if dec else 4)
        E.assert_attn(o, got, E.attn_reference(o), c.name)
        if not dec and c.d == 128 and c.g == 4 and not c.kv8:      # the invariant mode's per-row ballot
            E.assert_attn(o, E.attn_model(o, 64, 16, per_row=True), E.attn_reference(o), c.name + " per row")


# ---------------------------------------------------------------------------------
# mutation catalogue
# ---------------------------------------------------------------------------------

def _decode_case(f, sc=False):
    c = E.AttnCase(f, E.ATTN_BASE_LENS, 8, 2, 128, 16, None, sc, sc)
    assert c in ALL
    return c


def _prefill_case(f, sc=False):
    c = E.attn_prefill_case(f, 4, 128, 16, sc, sc, q_pad=512 if sc else 0)
    assert c in ALL
    return c


def _jump_tile(o, seq, kvh, family):
    """First key of a 16-token tile whose maximum (head 0) lies above everything before
    it: by 10 levels or more in the tile family, by any amount in the key family (whose
    levels span 12)."""
    _, info = E.attn_reference(o, return_scores=True)
    s = info[(seq, kvh)][0][-1, 0]                       # last row, head 0: [L]
    need = 10 if family == "tile" else 1
    for t0 in range(16, len(s) - 15, 16):
        if float(s[t0: t0 + 16].max()) - float(s[:t0].max()) >= need:
            return t0
    raise AssertionError("no upward jump")


def _uneven_partial(o, seq, kvh):
    """(first key, 16) of a one-tile partial, past key 1024, whose maximum differs between
    every head and its neighbour: taking the neighbour's m is a fault only there (in the
    key family most longer ranges reach the top level for every head)."""
    _, info = E.attn_reference(o, return_scores=True)
    s = info[(seq, kvh)][0][-1]                          # last row: [g, L]
    for t0 in range(1024, s.shape[1] - 15, 16):
        mx = s[:, t0: t0 + 16].max(-1).values
        if bool((mx != torch.roll(mx, -1)).all()):
            return t0, 16
    raise AssertionError("no partial with uneven maxima")


def _mutants(o, seq, prefill):
    """(name, AttnMutation) for segment (seq, kv head 1) of ``o``."""
    M = E.AttnMutation
    L = o.case.lens[seq]
    kw = dict(seq=seq, kvh=1)
    out = [("drop key 0", M(drop=(0,), **kw)), ("drop key L-1", M(drop=(L - 1,), **kw)),
           ("drop first key of a 16-tile", M(drop=(1040,), **kw)),
           ("drop last key of a 16-tile", M(drop=(1055,), **kw)),
           ("drop first key of a 64-tile", M(drop=(1088,), **kw)),
           ("drop last key of a 64-tile", M(drop=(1151,), **kw)),
           ("duplicate a key", M(dup=(777,), **kw)),
           ("admit position L", M(admit_len=True, **kw)),
           ("admit an unreferenced block's key", M(admit_free=True, **kw)),
           # attention does not care about the order of fully visible keys: the swap shows
           # where one of the two blocks is cut by the length or the causal limit
           ("swap two table blocks", M(swap_blocks=(3, (L - 1) // o.case.block_size), **kw)),
           ("read kv head h + 1", M(read_kvh=0, **kw)),
           ("skip a whole tile", M(drop=tuple(range(1040, 1056)), **kw)),
           ("merge a partial with the neighbouring head's m", M(merge_m_from_head=_uneven_partial(o, seq, 1), **kw)),
           ("merge a partial twice", M(merge_twice=(1024, 128), **kw)),
           ("omit one rescale", M(skip_rescale_at=_jump_tile(o, seq, 1, o.case.family), **kw))]
    if o.k_scale is not None:
        out += [("wrong head's k_scale", M(k_scale_of=0, **kw)), ("wrong head's v_scale", M(v_scale_of=0, **kw))]
    if prefill:
        out += [("causal limit + 1", M(causal=1, **kw)), ("causal limit - 1", M(causal=-1, **kw)),
                ("fully masked partial with weight 1", M(masked_weight_one=True, **kw))]
    return out


@pytest.mark.parametrize("scales", [False, True])
@pytest.mark.parametrize("prefill", [False, True])
@pytest.mark.parametrize("family", E.ATTN_FAMILIES)
def test_mutation_catalogue(family, prefill, scales):
    """Every mutant moves some element of the fp64 reference by more than one bf16 step
    (what assert_attn rejects); the unmutated reference is accepted.  The scale mutants
    run on the fp8 case with per-head scales, the causal and masked-partial ones on
    prefill (decode has neither a causal limit nor a fully masked partial)."""
    c = _prefill_case(family, scales) if prefill else _decode_case(family, scales)
    o = E.attn_operands(c)
    seq = max(range(len(c.lens)), key=lambda i: c.lens[i])       # 2100 / 2048 tokens
    ref = E.attn_reference(o)
    assert E.assert_attn(o, E.attn_reference(o), ref, "unmutated") == 0.0
    for name, mut in _mutants(o, seq, prefill):
        got = E.attn_reference(o, mut)
        worst = int(E.bf16_ulp_diff(got, ref).max())
        assert worst > 1, f"{c.name}: mutant '{name}' is not rejected (max {worst} steps)"
        with pytest.raises(AssertionError, match=f"sequence {seq}"):
            E.assert_attn(o, got, ref, name)
        # the fault stays inside the mutated segment
        q0, q1 = int(o.q_start_loc[seq]), int(o.q_start_loc[seq + 1])
        d = E.bf16_ulp_diff(got, ref).view(-1, c.nkv, c.g * c.d)
        assert int(d[:q0].max() if q0 else 0) == 0 and int(d[q0:q1, 0].max()) == 0, name


def test_failure_message_names_the_tile():
    o = E.attn_operands(_decode_case("tile"))
    ref = E.attn_reference(o)
    got = E.attn_reference(o, E.AttnMutation(seq=9, kvh=1, dup=tuple(range(131 * 16, 131 * 16 + 4))))
    msg = E.explain_attn(o, got, ref)
    assert "sequence 9" in msg and "kv head 1" in msg and "131" in msg and "x its weight" in msg, msg
