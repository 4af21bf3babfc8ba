"""Decode and prefill attention against an fp64 reference on exactly predictable operands
(ops/exact.py, attention section): integer scores in log2 units, one-hot V, one score level
per output channel.  Every key (key family) or 16-token tile (tile family) carries at least
3 * 2**-7 of one output element and every element must lie within ONE bf16 step of the
reference, so a key dropped, read twice or let through a mask, a partial merged with the
wrong maximum, another head's scale or a misaligned dim pairing fails here, where random
data at 2 % cannot see it.  tests/unit/test_exact_attention_cpu.py shows on the CPU that
the operands meet the design on every case below and that the comparison rejects each of
those faults.  A failure names the sequence, heads, dim and the keys or tile concerned."""
import functools

import pytest
import torch

from fasttalk_llm_microservice_amd import ops
from fasttalk_llm_microservice_amd.ops import exact as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


@pytest.fixture(autouse=True)
def _native_loaded():
    ops.native()  # fail loudly if the extension is missing


@functools.lru_cache(maxsize=6)
def _case(case):
    """(operands on the GPU, reference): computed once per case and never written to."""
    o = E.attn_operands(case)
    return o.to(DEV), E.attn_reference(o)


def _kind(c):
    return ("fp8s" if c.scales else "fp8") if c.kv8 else "bf16"


def _bits(t):
    return t.view(torch.uint8) if t.dtype == torch.float8_e4m3fn else t.view(torch.int16)


class _Frozen:
    """Inputs a launch must leave bit-identical: the decode kernel takes the caches through
    non-const pointers."""

    def __init__(self, o):
        self.o = o
        self.saved = [_bits(o.k_cache).clone(), _bits(o.v_cache).clone(), o.block_tables.clone(),
                      o.seq_lens.clone(), o.q_start_loc.clone(), o.q_buf.view(torch.int16).clone()]

    def check(self, what):
        o = self.o
        now = [_bits(o.k_cache), _bits(o.v_cache), o.block_tables, o.seq_lens, o.q_start_loc,
               o.q_buf.view(torch.int16)]
        for name, a, b in zip(("k_cache", "v_cache", "block_tables", "seq_lens", "q_start_loc", "q"),
                              self.saved, now):
            assert torch.equal(a, b), f"{what}: the launch changed {name}"


# ---------------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------------

DECODE_PATHS = ("combine", "fused", "piece1", "piece8", "piece64")


def _decode(o, path, guard=False):
    """Runs one decode path; returns the bf16 output [B, nq d].  ``guard``: out, workspaces
    and tickets inside guarded allocations, inputs compared bit for bit afterwards."""
    c = o.case
    b, nq, nkv, d = len(c.lens), c.nq, c.nkv, c.d
    piece = int(path[5:]) if path.startswith("piece") else 0
    n_out, n_ml = ops.decode_workspace(b, nq, nkv, d, piece=piece,
                                       max_len=o.block_tables.shape[1] * c.block_size)
    if guard:
        frozen = _Frozen(o)
        g_out = E.guarded(b, nq * d, device=DEV)
        g_out.view.fill_(NAN)
        out = g_out.view
        g_to, g_ml = E.guarded_flat(n_out, device=DEV), E.guarded_flat(n_ml, device=DEV)
        tmp_out, tmp_ml = g_to.buf, g_ml.buf
        g_cnt = E.guarded_flat(max(1, b * nkv), tail=256, dtype=torch.int32, device=DEV)
        g_cnt.view.zero_()
        cnt = None if path == "combine" else g_cnt.buf
    else:
        out = torch.full((b, nq * d), NAN, device=DEV, dtype=torch.bfloat16)
        tmp_out = torch.full((n_out,), NAN, device=DEV)
        tmp_ml = torch.full((n_ml,), NAN, device=DEV)
        cnt = None if path == "combine" else ops.decode_counters(b, nkv, DEV)
    calls = 1 if path == "combine" else 3
    first = None
    for i in range(calls):
        if i:
            out.fill_(NAN)
        ops.decode_attention(out, o.q, o.k_cache, o.v_cache, o.block_tables, o.seq_lens, tmp_out,
                             tmp_ml, nq, nkv, d, E.ATTN_SCALE, counters=cnt, piece=piece,
                             k_scale=o.k_scale, v_scale=o.v_scale)
        if i == 0:
            first = out.clone()
        else:   # the tickets reset themselves: repeated calls agree bit for bit
            assert torch.equal(first.view(torch.int16), out.view(torch.int16)), \
                f"{c.name} {path}: call {i + 1} differs from call 1"
    torch.cuda.synchronize()
    if cnt is not None:
        assert int(cnt[: b * nkv].abs().sum()) == 0, f"{c.name} {path}: tickets must be left zero"
    if guard:
        what = f"{c.name} {path}"
        g_out.check(what + " out")
        g_to.check(what + " tmp_out")
        g_ml.check(what + " tmp_ml")
        g_cnt.check(what + " tickets")
        frozen.check(what)
    return out


def _check_decode(case, paths):
    o, ref = _case(case)
    for path in paths:
        got = _decode(o, path)
        E.assert_attn(o, got, ref, f"decode/{path}/{_kind(case)} {case.name}")
        # length-0 rows: exactly zero on every path
        empty = [i for i, l in enumerate(case.lens) if l == 0]
        assert bool((got[empty].float() == 0).all()), f"{case.name} {path}: an empty row is not zero"


@pytest.mark.parametrize("bs", E.ATTN_DECODE_BLOCKS)
@pytest.mark.parametrize("family", E.ATTN_FAMILIES)
@pytest.mark.parametrize("d,g", E.attn_instantiated("decode"))
def test_decode_base(d, g, family, bs):
    """Every instantiated (D, G), both families, every block size: lengths around tile and
    block edges in both orders and alone, on the fused-combine and the combine-kernel path.
    [2100] alone spreads one segment over 17 waves: the ticket merge runs 3 batches of 8."""
    cases = [c for c in E.attn_decode_base_cases()
             if (c.d, c.g, c.family, c.block_size) == (d, g, family, bs)]
    assert len(cases) == len(E.ATTN_DECODE_LENS)
    for c in cases:
        _check_decode(c, ("fused", "combine"))


@pytest.mark.parametrize("path", DECODE_PATHS)
@pytest.mark.parametrize("case", E.attn_decode_path_cases(), ids=lambda c: c.name)
def test_decode_paths(case, path):
    """Combine kernel, fused combine (3 calls into a NaN-filled out, bit-identical, tickets
    left zero) and piece mode (piece = 1: 132 pieces at L = 2100, many merge batches of 8)
    on bf16 and fp8 caches, without and with per-head power-of-two scales."""
    _check_decode(case, (path,))


@pytest.mark.parametrize("case", E.attn_decode_special_cases(), ids=lambda c: c.name)
def test_decode_special(case):
    """130 sequences (the prefix scan walks 64 at a time); 16 x 4100 tokens at nkv = 8 (a
    wave's range exceeds 64 tiles: the chunked block-index prefetch); nkv = 8 fused."""
    if case.lens == E.ATTN_LONG_LENS:   # the bf16 grid: one 2-wave workgroup per CU
        waves = ops.native().decode_waves() // 12 * 2
        assert case.nkv * sum(-(-l // 16) for l in case.lens) > 64 * waves
    _check_decode(case, ("fused", "combine"))


def test_decode_uninstantiated_pair_is_an_error():
    assert (128, 5) not in E.attn_instantiated("decode")
    o = E.attn_operands(E.AttnCase("tile", (40,), 10, 2, 128)).to(DEV)
    n_out, n_ml = ops.decode_workspace(1, 10, 2, 128)
    out = torch.zeros(1, 10 * 128, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="code -2"):
        ops.decode_attention(out, o.q, o.k_cache, o.v_cache, o.block_tables, o.seq_lens,
                             torch.zeros(n_out, device=DEV), torch.zeros(n_ml, device=DEV), 10, 2, 128,
                             E.ATTN_SCALE)


@pytest.mark.parametrize("path", ("combine", "fused", "piece8"))
@pytest.mark.parametrize("case", E.attn_decode_footprint_cases(), ids=lambda c: c.name)
def test_decode_footprint(path, case):
    """out inside a guarded strided allocation, q surrounded by NaN rows and columns,
    workspaces and tickets with guarded tails, caches / tables / lengths bit-identical."""
    o, ref = _case(case)
    assert o.q.stride(0) > case.nq * case.d and bool(torch.isnan(o.q_buf[0].float()).all())
    got = _decode(o, path, guard=True)
    E.assert_attn(o, got, ref, f"decode-footprint/{path}/{_kind(case)} {case.name}")


# ---------------------------------------------------------------------------------
# prefill
# ---------------------------------------------------------------------------------

PREFILL_MODES = ("unsplit", "split", "invariant")


def _prefill_plan(c, mode):
    tt = ops.prefill_tile_tokens(c.nq, c.nkv)
    assert tt == 256 // c.g
    if mode == "unsplit":
        tiles, comb = ops.build_prefill_tiles(c.q_lens, tt)
        assert not comb
    elif mode == "split":
        tiles, comb = ops.build_prefill_tiles(c.q_lens, tt, seq_lens=c.lens, nkv=c.nkv, num_cus=256,
                                              min_split_tiles=1)
        assert comb, "the plan split nothing"
        # at least one item lies wholly above its block's early rows: a fully masked partial
        masked = [it for it in tiles if it[3] >= 0 and
                  (it[2] >> 16) * ops.PREFILL_BK > c.lens[it[0]] - c.q_lens[it[0]] + it[1]]
        assert masked, "no split item is fully masked for its early rows"
    else:
        tiles, comb = ops.build_prefill_tiles(c.q_lens, tt, seq_lens=c.lens, nkv=c.nkv,
                                              fixed_chunk=ops.PREFILL_INV_CHUNK)
        assert comb and max(c.lens) > 1024, "the invariant plan needs a sequence above 1024 tokens"
    return tiles, comb


def _prefill(o, mode, guard=False):
    c = o.case
    nq, nkv, d = c.nq, c.nkv, c.d
    t = sum(c.q_lens)
    tiles, comb = _prefill_plan(c, mode)
    ti = torch.tensor(tiles, dtype=torch.int32, device=DEV).flatten()
    if guard:
        frozen = _Frozen(o)
        g_out = E.guarded(t, nq * d, device=DEV)
        g_out.view.fill_(NAN)
        out = g_out.view
    else:
        out = torch.full((t, nq * d), NAN, device=DEV, dtype=torch.bfloat16)
    kw = dict(k_scale=o.k_scale, v_scale=o.v_scale, invariant=(mode == "invariant"))
    args = (out, o.q, o.k_cache, o.v_cache, o.block_tables, o.seq_lens, o.q_start_loc, ti, len(tiles),
            nq, nkv, d, E.ATTN_SCALE)
    if comb:
        nparts = sum(cb[3] for cb in comb)
        n_po, n_pml = ops.prefill_partials(nkv, d, max_partials=nparts if guard else ops.PREFILL_MAX_PARTIALS)
        if guard:
            g_po, g_pml = E.guarded_flat(n_po, device=DEV), E.guarded_flat(n_pml, device=DEV)
            po, pml = g_po.buf, g_pml.buf
        else:
            po, pml = torch.full((n_po,), NAN, device=DEV), torch.full((n_pml,), NAN, device=DEV)
        cb = torch.tensor(comb, dtype=torch.int32, device=DEV).flatten()
        ops.prefill_attention(*args, po, pml, cb, len(comb), nparts, **kw)
    else:
        ops.prefill_attention(*args, **kw)
    torch.cuda.synchronize()
    if guard:
        what = f"{c.name} {mode}"
        g_out.check(what + " out")
        if comb:
            g_po.check(what + " part_o")
            g_pml.check(what + " part_ml")
        frozen.check(what)
    return out


@pytest.mark.parametrize("family", E.ATTN_FAMILIES)
@pytest.mark.parametrize("d,g", E.attn_instantiated("prefill"))
def test_prefill_base(d, g, family):
    """Every instantiated (D, G), both families: new tokens over cached prefixes whose ends
    land on and one past multiples of 8, 16, 64 and on block boundaries, query blocks past
    256 / G tokens; every query row is compared (row i sees positions <= prefix + i, and the
    later new tokens are real, heavy keys in the cache)."""
    case = [c for c in E.attn_prefill_base_cases() if (c.d, c.g, c.family) == (d, g, family)]
    assert len(case) == 1
    o, ref = _case(case[0])
    for mode in ("unsplit", "split"):
        E.assert_attn(o, _prefill(o, mode), ref, f"prefill/{mode}/bf16 {case[0].name}")


@pytest.mark.parametrize("mode", PREFILL_MODES)
@pytest.mark.parametrize("case", E.attn_prefill_path_cases(), ids=lambda c: c.name)
def test_prefill_paths(case, mode):
    """Unsplit, split-KV (with fully masked partials) and the invariant fixed-chunk plan on
    bf16 and fp8 caches, without and with per-head scales, block sizes 16 and 32, q read
    with a row stride out of a fused-QKV-shaped buffer."""
    o, ref = _case(case)
    assert o.q.stride(0) == (case.nq + 2 * case.nkv) * case.d + E.LEAD_COLS
    E.assert_attn(o, _prefill(o, mode), ref, f"prefill/{mode}/{_kind(case)} {case.name}")


def test_prefill_uninstantiated_pair_is_an_error():
    assert (128, 5) not in E.attn_instantiated("prefill")
    o = E.attn_operands(E.AttnCase("tile", (40,), 10, 2, 128, 16, (7,))).to(DEV)
    tiles, _ = ops.build_prefill_tiles([7], 256 // 5)
    ti = torch.tensor(tiles, dtype=torch.int32, device=DEV).flatten()
    out = torch.zeros(7, 10 * 128, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="code -2"):
        ops.prefill_attention(out, o.q, o.k_cache, o.v_cache, o.block_tables, o.seq_lens, o.q_start_loc,
                              ti, len(tiles), 10, 2, 128, E.ATTN_SCALE)


@pytest.mark.parametrize("mode", PREFILL_MODES)
@pytest.mark.parametrize("kind", [k for k, _, _ in E.ATTN_KINDS if k != "fp8"])
def test_prefill_footprint(mode, kind):
    case = [c for c in E.attn_prefill_path_cases()
            if (c.family, c.block_size, _kind(c)) == ("key", 16, kind)][0]
    o, ref = _case(case)
    assert bool(torch.isnan(o.q_buf[0].float()).all()) and bool(torch.isnan(o.q_buf[:, -1].float()).all())
    got = _prefill(o, mode, guard=True)
    E.assert_attn(o, got, ref, f"prefill-footprint/{mode}/{kind} {case.name}")
