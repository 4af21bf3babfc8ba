"""Per-head K / V scales of the fp8 (e4m3) KV cache: stored = clamp(x / scale, +-448),
x ~= stored * scale, one fp32 scale per kv head (and per layer in the model).

Writers (rope_kv.hip, fused_epilogue.hip slab_rope_kv) multiply by the host-computed
reciprocal before the clamp; readers (attn_decode.hip, attn_prefill.hip and their
combine kernels) fold K's scale into the softmax scale of the (sequence, kv head)
and apply V's once to the normalised output.  Scales differ per head and are not
all powers of two, so a head-index mix-up or a K / V swap shows.  Unit scales and
absent scales must give the same bits.  Model- and engine-level cases run weights
whose K / V are 1024x the random-init ones (q /= 1024, k *= 1024, v *= 1024,
o /= 1024: exact in bf16, the function is unchanged), which scale 1.0 clips."""
import numpy as np
import pytest
import torch

from fasttalk_llm_microservice_amd import ops
from fasttalk_llm_microservice_amd.engine import kv_calibrate
from fasttalk_llm_microservice_amd.engine.chat_template import ChatTemplate
from fasttalk_llm_microservice_amd.engine.config import EngineConfig
from fasttalk_llm_microservice_amd.engine.engine import LLMEngine
from fasttalk_llm_microservice_amd.engine.sampling_params import SamplingParams
from fasttalk_llm_microservice_amd.engine.tokenizer import get_tokenizer
from fasttalk_llm_microservice_amd.models import weights as W
from fasttalk_llm_microservice_amd.models.config import MODELS
from fasttalk_llm_microservice_amd.models.llama import AttnMeta, LlamaModel
from fasttalk_llm_microservice_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
F8 = torch.float8_e4m3fn
MAG = 64.0   # writer inputs: the existing fp8 tests' magnitudes x 64, well past +-448


def _close(a, b, atol, rtol=0.0, msg=""):
    a = a.float().cpu()
    b = b.float().cpu()
    err = (a - b).abs()
    tol = torch.as_tensor(atol).cpu() + rtol * b.abs()
    bad = (err > tol).sum().item()
    assert bad == 0, f"{msg}: {bad} elems out of tol, max err {err.max().item():.4g}"


@pytest.fixture(autouse=True)
def _native_loaded():
    ops.native()  # fail loudly if the extension is missing
    torch.manual_seed(0)


def _f8(x):
    return x.float().clamp(-448, 448).to(F8)


def _bytes(c):
    return c.view(torch.uint8)


def _reader_scales(nkv):
    """The attention tests' scales: all different, not all powers of two."""
    h = torch.arange(nkv, dtype=torch.float32)
    return (0.37 * (h + 1)).to(DEV), (2.0 ** (h % 4 - 1) * 1.1).to(DEV)


def _writer_scales(nkv):
    """The same per-head pattern lifted above absmax / 448 of the writers' inputs
    (N(0, (3 * 64)^2): 5.5 sigma / 448 = 2.36), so nothing may clip."""
    ks, vs = _reader_scales(nkv)
    return ks + 2.0, vs + 2.0


def _ones(nkv):
    return torch.ones(nkv, dtype=torch.float32, device=DEV)


def _zero_cache(nblocks, nkv, bs, d):
    return (torch.zeros(nblocks, nkv, bs, d, device=DEV).to(F8),
            torch.zeros(nblocks, nkv, d, bs, device=DEV).to(F8))


def _written(k, v, slots, bs):
    """[t, nkv, d] rows of K and V at ``slots`` (V blocks are transposed)."""
    s = slots.long()
    blk, off = s // bs, s % bs
    return k[blk, :, off, :].float(), v[blk, :, :, off].float()


def _check_dequant(stored, want, scale, atol_extra, msg):
    """stored * scale matches the unquantised value within e4m3's half-step: 1/16
    relative for normal numbers, half the subnormal step (2^-10) in stored units below
    2^-6; ``atol_extra`` covers the fp32 rounding of the value before the cast."""
    sc = scale.view(1, -1, 1).cpu()
    got = stored.cpu() * sc
    tol = sc * 2.0 ** -10 + atol_extra
    _close(got, want, atol=tol.expand_as(got), rtol=1.0 / 16 + 1e-5, msg=msg)


# ------------------------------------------------------------------------- 1. writers

@pytest.mark.parametrize("nq,nkv,d", [(32, 8, 128), (32, 8, 64), (8, 1, 128)])
def test_scaled_rope_kv_write(nq, nkv, d):
    t, bs, nblocks = 45, 16, 20
    qkv = (torch.randn(t, (nq + 2 * nkv) * d, device=DEV) * 3 * MAG).bfloat16()
    pos = torch.randint(0, 4000, (t,), device=DEV, dtype=torch.int32)
    cs = ref.rope_cos_sin(d, 8192, 500000.0, None, DEV)
    slots = torch.randperm(nblocks * bs, device=DEV)[:t].int()
    slots[3] = -1
    ks, vs = _writer_scales(nkv)
    k1, v1 = _zero_cache(nblocks, nkv, bs, d)
    k2, v2 = k1.clone(), v1.clone()
    q1, q2 = qkv.clone(), qkv.clone()
    ops.rope_kv_write(q1, pos, cs, slots, k1, v1, nq, nkv, d, k_scale=ks, v_scale=vs)
    ref.rope_kv_write(q2, pos, cs, slots, k2, v2, nq, nkv, d, k_scale=ks, v_scale=vs)
    _close(q1[:, : nq * d], q2[:, : nq * d], atol=2e-2 * MAG, rtol=1e-2, msg="q")
    # the existing tolerances (tests/test_kv_fp8_gpu.py): K one e4m3 step, V equal bytes
    _close(k1, k2, atol=2e-3, rtol=0.126, msg="k cache")
    assert (k1.float() != k2.float()).float().mean().item() < 0.01
    assert torch.equal(_bytes(v1), _bytes(v2))
    # dequantised cache vs the unquantised values
    keep = slots >= 0
    kq, vq = _written(k1, v1, slots[keep], bs)
    kv_in = qkv[keep].float()
    k_true = ref.apply_rope(kv_in[:, nq * d:(nq + nkv) * d].view(-1, nkv, d), pos[keep], cs)
    v_true = kv_in[:, (nq + nkv) * d:].view(-1, nkv, d)
    # 1e-3: fp32 rounding of the rotation (operands ~1e3, eps 1.2e-7, a few terms)
    _check_dequant(kq, k_true.cpu(), ks, 1e-3, "k dequantised")
    _check_dequant(vq, v_true.cpu(), vs, 0.0, "v dequantised")
    assert k1.float().abs().max().item() < 448 and v1.float().abs().max().item() < 448
    # control: the same input at scale 1.0 clips
    k3, v3 = _zero_cache(nblocks, nkv, bs, d)
    ops.rope_kv_write(qkv.clone(), pos, cs, slots, k3, v3, nq, nkv, d)
    assert k3.float().abs().max().item() == 448 and v3.float().abs().max().item() == 448


@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("nq,nkv,d", [(32, 8, 128), (32, 8, 64)])
def test_scaled_slab_rope_kv(nq, nkv, d, with_residual):
    t, bs, nblocks, splits, hidden, eps = 19, 16, 8, 4, 2048, 1e-5
    cols = (nq + 2 * nkv) * d
    parts = torch.randn(splits, t, cols, device=DEV) * MAG
    res = torch.randn(t, hidden, device=DEV).bfloat16() if with_residual else None
    pos = torch.randint(0, 4000, (t,), device=DEV, dtype=torch.int32)
    # the slab sum is N(0, 128^2): a few planted values (token 0 at position 0, so K is
    # not rotated) make sure the scale-1.0 control below has something past +-448
    pos[0] = 0
    parts[0, 0, nq * d: nq * d + 8] += 600.0
    parts[0, 0, (nq + nkv) * d: (nq + nkv) * d + 8] += 600.0
    cs = ref.rope_cos_sin(d, 8192, 500000.0, None, DEV)
    slots = torch.randperm(nblocks * bs, device=DEV)[:t].int()
    ks, vs = _writer_scales(nkv)
    k1, v1 = _zero_cache(nblocks, nkv, bs, d)
    k2, v2 = k1.clone(), v1.clone()
    q_out = torch.zeros(t, nq * d, device=DEV).bfloat16()
    kw = dict(residual=res, eps=eps) if with_residual else {}
    ops.slab_rope_kv(parts.flatten(), splits, t, cols, q_out, pos, cs, slots, k1, v1, nq, nkv, d,
                     k_scale=ks, v_scale=vs, **kw)
    full = parts.sum(0)
    if with_residual:
        full = full * torch.rsqrt(res.float().pow(2).mean(-1, keepdim=True) + eps)
    qkv = full.bfloat16()
    ref.rope_kv_write(qkv, pos, cs, slots, k2, v2, nq, nkv, d, k_scale=ks, v_scale=vs)
    _close(q_out, qkv[:, : nq * d], atol=3e-2 * MAG, rtol=2e-2, msg="q")
    # the existing 3e-2 (the reference rounds the slab sum to bf16 before RoPE) scaled by
    # the input magnitude, in stored units; then one e4m3 step
    atol = 3e-2 * MAG / min(ks.min().item(), vs.min().item())
    _close(k1, k2, atol=atol, rtol=0.126, msg="k")
    _close(v1, v2, atol=atol, rtol=0.126, msg="v")
    kq, vq = _written(k1, v1, slots, bs)
    k_true = ref.apply_rope(full[:, nq * d:(nq + nkv) * d].reshape(t, nkv, d), pos, cs)
    v_true = full[:, (nq + nkv) * d:].reshape(t, nkv, d)
    # 1e-3 as above, plus the order of the fp32 slab sum and rsqrt's last bit
    _check_dequant(kq, k_true.cpu(), ks, 2e-3, "k dequantised")
    _check_dequant(vq, v_true.cpu(), vs, 2e-3, "v dequantised")
    assert k1.float().abs().max().item() < 448 and v1.float().abs().max().item() < 448
    k3, v3 = _zero_cache(nblocks, nkv, bs, d)
    ops.slab_rope_kv(parts.flatten(), splits, t, cols, q_out, pos, cs, slots, k3, v3, nq, nkv, d,
                     **kw)
    assert k3.float().abs().max().item() == 448 and v3.float().abs().max().item() == 448


# --------------------------------------------------------------- attention test cases

def _alloc_cache(nblocks, nkv, bs, d, ks, vs):
    """fp8 caches holding f8(randn / scale[h]): the dequantised K / V are N(0, 1)."""
    k = _f8(torch.randn(nblocks, nkv, bs, d, device=DEV) / ks.view(1, -1, 1, 1))
    v = _f8(torch.randn(nblocks, nkv, d, bs, device=DEV) / vs.view(1, -1, 1, 1))
    return k, v


def _dequant(k, v, ks, vs):
    """What the kernels read, as fp32 caches: bf(k) * k_scale[h], bf(v) * v_scale[h]."""
    return (k.to(torch.bfloat16).float() * ks.view(1, -1, 1, 1),
            v.to(torch.bfloat16).float() * vs.view(1, -1, 1, 1))


def _random_tables(lens, bs, nblocks_total):
    perm = torch.randperm(nblocks_total).int()
    maxb = max((l + bs - 1) // bs for l in lens)
    bt = torch.zeros(len(lens), maxb, dtype=torch.int32)
    i = 0
    for b, l in enumerate(lens):
        n = (l + bs - 1) // bs
        bt[b, :n] = perm[i: i + n]
        i += n
    return bt


def _decode_setup(lens, nq, nkv, d, bs, ks, vs, piece=0):
    nblocks = sum((l + bs - 1) // bs for l in lens) + 4
    k, v = _alloc_cache(nblocks, nkv, bs, d, ks, vs)
    bt = _random_tables(lens, bs, nblocks).to(DEV)
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    q = torch.randn(len(lens), nq * d, device=DEV).bfloat16()
    n_out, n_ml = ops.decode_workspace(len(lens), nq, nkv, d, piece=piece, max_len=max(lens))
    return k, v, bt, sl, q, n_out, n_ml


def _decode_run(setup, nq, nkv, d, ks, vs, fused=True, piece=0, calls=2):
    k, v, bt, sl, q, n_out, n_ml = setup
    b = q.shape[0]
    tmp_out = torch.full((n_out,), float("nan"), device=DEV)
    tmp_ml = torch.full((n_ml,), float("nan"), device=DEV)
    out = torch.full((b, nq * d), float("nan"), device=DEV).bfloat16()
    cnt = ops.decode_counters(b, nkv, DEV) if (fused or piece) else None
    for _ in range(calls):
        first = out.clone()
        ops.decode_attention(out, q, k, v, bt, sl, tmp_out, tmp_ml, nq, nkv, d, d ** -0.5,
                             counters=cnt, piece=piece, k_scale=ks, v_scale=vs)
    if calls > 1:
        assert torch.equal(first, out)
    if cnt is not None:
        torch.cuda.synchronize()
        assert int(cnt.abs().sum()) == 0, "combine tickets must be left zeroed"
    return out


def _decode_case(lens, nq, nkv, d, bs=16, fused=True, piece=0, scales=None):
    ks, vs = scales if scales is not None else _reader_scales(nkv)
    setup = _decode_setup(lens, nq, nkv, d, bs, ks, vs, piece)
    out = _decode_run(setup, nq, nkv, d, ks, vs, fused, piece)
    k, v, bt, sl, q = setup[:5]
    b = len(lens)
    kd, vd = _dequant(k, v, ks, vs)
    expect = ref.paged_attention(q.view(b, nq, d), kd, vd, bt, sl,
                                 torch.arange(b + 1, dtype=torch.int32), d ** -0.5).view(b, nq * d)
    return out, expect


DEC_LENS = [1, 17, 255, 256, 257, 1000, 2100]


# ----------------------------------------------------------------- 3. decode attention

@pytest.mark.parametrize("nq,nkv,d", [(32, 8, 128), (64, 8, 128), (32, 8, 64), (8, 1, 128)])
@pytest.mark.parametrize("fused", [True, False])
def test_scaled_decode_attention(nq, nkv, d, fused):
    out, expect = _decode_case(DEC_LENS, nq, nkv, d, fused=fused)
    _close(out, expect, atol=2e-2, rtol=2e-2, msg="scaled fp8 decode attention")


def test_scaled_decode_attention_batch_invariant_pieces():
    out, expect = _decode_case([5, 600, 1500, 33], 32, 8, 128, piece=ops.DECODE_INV_PIECE)
    _close(out, expect, atol=2e-2, rtol=2e-2, msg="scaled fp8 decode attention (pieces)")


def test_scaled_decode_attention_block_size_32():
    out, expect = _decode_case(DEC_LENS, 32, 8, 128, bs=32)
    _close(out, expect, atol=2e-2, rtol=2e-2, msg="scaled fp8 decode attention bs=32")


@pytest.mark.parametrize("fused", [True, False])
def test_scaled_decode_attention_large_v_scale(fused):
    """The output is linear in v_scale: one head's scale x 8 scales that head's
    absolute tolerance by 8, nothing else."""
    nq, nkv, d, big = 32, 8, 128, 5
    ks, vs = _reader_scales(nkv)
    vs = vs.clone()
    vs[big] *= 8
    out, expect = _decode_case(DEC_LENS, nq, nkv, d, fused=fused, scales=(ks, vs))
    g = nq // nkv
    atol = torch.full((1, nq * d), 2e-2)
    atol[:, big * g * d:(big + 1) * g * d] *= 8
    _close(out, expect, atol=atol.expand(len(DEC_LENS), -1), rtol=2e-2, msg="v_scale x 8")


# ---------------------------------------------------------------- 4. prefill attention

def _prefill_setup(seqs, nq, nkv, d, split, bs, ks, vs):
    lens = [a + p for a, p in seqs]
    nblocks = sum((l + bs - 1) // bs for l in lens) + 4
    k, v = _alloc_cache(nblocks, nkv, bs, d, ks, vs)
    bt = _random_tables(lens, bs, nblocks).to(DEV)
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    qlens = [a for a, _ in seqs]
    qsl = torch.tensor([0] + list(torch.tensor(qlens).cumsum(0)), dtype=torch.int32)
    t = int(qsl[-1])
    q = torch.randn(t, nq * d, device=DEV).bfloat16()
    tiles, comb = ops.build_prefill_tiles(qlens, ops.prefill_tile_tokens(nq, nkv),
                                          seq_lens=lens if split else None, nkv=nkv, num_cus=256,
                                          min_split_tiles=1)
    assert bool(comb) == bool(split), comb
    return k, v, bt, sl, qsl, q, tiles, comb


def _prefill_run(setup, nq, nkv, d, ks, vs, invariant=False):
    k, v, bt, sl, qsl, q, tiles, comb = setup
    t = q.shape[0]
    ti = torch.tensor(tiles, dtype=torch.int32, device=DEV).flatten()
    out = torch.zeros(t, nq * d, device=DEV).bfloat16()
    scale = d ** -0.5
    if comb:
        n_po, n_pml = ops.prefill_partials(nkv, d)
        po = torch.full((n_po,), float("nan"), device=DEV)
        pml = torch.full((n_pml,), float("nan"), device=DEV)
        cb = torch.tensor(comb, dtype=torch.int32, device=DEV).flatten()
        ops.prefill_attention(out, q, k, v, bt, sl, qsl.to(DEV), ti, len(tiles), nq, nkv, d, scale,
                              po, pml, cb, len(comb), sum(c[3] for c in comb), invariant=invariant,
                              k_scale=ks, v_scale=vs)
    else:
        ops.prefill_attention(out, q, k, v, bt, sl, qsl.to(DEV), ti, len(tiles), nq, nkv, d, scale,
                              invariant=invariant, k_scale=ks, v_scale=vs)
    return out


def _prefill_case(seqs, nq, nkv, d, split, bs=16, invariant=False):
    ks, vs = _reader_scales(nkv)
    setup = _prefill_setup(seqs, nq, nkv, d, split, bs, ks, vs)
    out = _prefill_run(setup, nq, nkv, d, ks, vs, invariant)
    k, v, bt, sl, qsl, q = setup[:6]
    t = q.shape[0]
    kd, vd = _dequant(k, v, ks, vs)
    expect = ref.paged_attention(q.view(t, nq, d), kd, vd, bt, sl, qsl, d ** -0.5).view(t, nq * d)
    return out, expect


PF_SEQS = [(1, 0), (5, 0), (64, 0), (77, 33), (16, 300), (130, 1), (3, 500), (40, 23)]
PF_SPLIT_SEQS = [(100, 2900), (37, 4000), (64, 0), (130, 700), (3, 1500), (1, 63)]


@pytest.mark.parametrize("nq,nkv,d", [(32, 8, 128), (24, 8, 128), (32, 8, 64)])
@pytest.mark.parametrize("invariant", [False, True])
def test_scaled_prefill_attention(nq, nkv, d, invariant):
    out, expect = _prefill_case(PF_SEQS, nq, nkv, d, split=False, invariant=invariant)
    assert torch.isfinite(out.float()).all()
    _close(out, expect, atol=2e-2, rtol=2e-2, msg="scaled fp8 prefill attention")


@pytest.mark.parametrize("nq,nkv,d", [(32, 8, 128), (24, 8, 128), (32, 8, 64)])
def test_scaled_prefill_attention_split_kv(nq, nkv, d):
    out, expect = _prefill_case(PF_SPLIT_SEQS, nq, nkv, d, split=True)
    assert torch.isfinite(out.float()).all()
    _close(out, expect, atol=2e-2, rtol=2e-2, msg="scaled fp8 prefill attention split-KV")


# ------------------------------------------------- 2. unit scales are bit-identical

def test_unit_scales_match_absent_scales_writers():
    nq, nkv, d, bs, nblocks = 32, 8, 128, 16, 20
    one = _ones(nkv)
    cs = ref.rope_cos_sin(d, 8192, 500000.0, None, DEV)
    t = 45
    qkv = (torch.randn(t, (nq + 2 * nkv) * d, device=DEV) * 3).bfloat16()
    pos = torch.randint(0, 4000, (t,), device=DEV, dtype=torch.int32)
    slots = torch.randperm(nblocks * bs, device=DEV)[:t].int()
    slots[3] = -1
    ka, va = _zero_cache(nblocks, nkv, bs, d)
    kb, vb = _zero_cache(nblocks, nkv, bs, d)
    qa, qb = qkv.clone(), qkv.clone()
    ops.rope_kv_write(qa, pos, cs, slots, ka, va, nq, nkv, d)
    ops.rope_kv_write(qb, pos, cs, slots, kb, vb, nq, nkv, d, k_scale=one, v_scale=one)
    assert torch.equal(_bytes(ka), _bytes(kb)) and torch.equal(_bytes(va), _bytes(vb))
    assert torch.equal(qa, qb)
    t, splits, hidden, eps = 19, 4, 2048, 1e-5
    cols = (nq + 2 * nkv) * d
    parts = torch.randn(splits, t, cols, device=DEV)
    res = torch.randn(t, hidden, device=DEV).bfloat16()
    pos = torch.randint(0, 4000, (t,), device=DEV, dtype=torch.int32)
    slots = torch.randperm(nblocks * bs, device=DEV)[:t].int()
    for kw in ({}, dict(residual=res, eps=eps)):
        ka, va = _zero_cache(nblocks, nkv, bs, d)
        kb, vb = _zero_cache(nblocks, nkv, bs, d)
        qa = torch.zeros(t, nq * d, device=DEV).bfloat16()
        qb = qa.clone()
        ops.slab_rope_kv(parts.flatten(), splits, t, cols, qa, pos, cs, slots, ka, va, nq, nkv, d,
                         **kw)
        ops.slab_rope_kv(parts.flatten(), splits, t, cols, qb, pos, cs, slots, kb, vb, nq, nkv, d,
                         k_scale=one, v_scale=one, **kw)
        assert torch.equal(_bytes(ka), _bytes(kb)) and torch.equal(_bytes(va), _bytes(vb))
        assert torch.equal(qa, qb)


@pytest.mark.parametrize("fused,piece", [(True, 0), (False, 0), (True, ops.DECODE_INV_PIECE)])
def test_unit_scales_match_absent_scales_decode(fused, piece):
    nq, nkv, d = 32, 8, 128
    one = _ones(nkv)
    setup = _decode_setup(DEC_LENS, nq, nkv, d, 16, one, one, piece)
    a = _decode_run(setup, nq, nkv, d, None, None, fused, piece, calls=1)
    b = _decode_run(setup, nq, nkv, d, one, one, fused, piece, calls=1)
    assert torch.equal(a, b)


@pytest.mark.parametrize("split,invariant", [(False, False), (False, True), (True, False)])
def test_unit_scales_match_absent_scales_prefill(split, invariant):
    nq, nkv, d = 32, 8, 128
    one = _ones(nkv)
    setup = _prefill_setup(PF_SPLIT_SEQS if split else PF_SEQS, nq, nkv, d, split, 16, one, one)
    a = _prefill_run(setup, nq, nkv, d, None, None, invariant)
    b = _prefill_run(setup, nq, nkv, d, one, one, invariant)
    assert torch.equal(a, b)


def test_scale_argument_checks():
    nq, nkv, d, bs = 32, 8, 128, 16
    one = _ones(nkv)
    setup = _decode_setup([40], nq, nkv, d, bs, one, one)
    with pytest.raises(RuntimeError):   # wrong shape
        _decode_run(setup, nq, nkv, d, _ones(nkv + 1), one, calls=1)
    with pytest.raises(RuntimeError):   # wrong dtype
        _decode_run(setup, nq, nkv, d, one.double(), one, calls=1)
    k, v, bt, sl, q, n_out, n_ml = setup
    kb, vb = k.to(torch.bfloat16), v.to(torch.bfloat16)
    with pytest.raises(RuntimeError):   # scales with bf16 caches
        _decode_run((kb, vb, bt, sl, q, n_out, n_ml), nq, nkv, d, one, one, calls=1)


# ------------------------------------------------------------------- 5. model level

C = 1024.0   # a power of two: the weight transform is exact in bf16


def _outlier_layers(cfg):
    g = torch.Generator().manual_seed(3)
    layers = [W.random_full_layer(cfg, g, 0.02, torch.bfloat16) for _ in range(cfg.num_layers)]
    for L in layers:
        L["q"] = (L["q"].float() / C).bfloat16()
        L["k"] = (L["k"].float() * C).bfloat16()
        L["v"] = (L["v"].float() * C).bfloat16()
        L["o"] = (L["o"].float() / C).bfloat16()
    embed = (torch.randn(cfg.vocab_size, cfg.hidden_size, generator=g) * 0.02).bfloat16()
    return layers, embed


def _ckpt_scales(cfg):
    """Scales written into the tiny checkpoint: distinct per layer and head, around
    2 * absmax / 448 of these weights' K / V (absmax 2-4 x 1024)."""
    h = torch.arange(cfg.num_kv_heads, dtype=torch.float32)
    k = torch.stack([9.0 + li + 0.37 * (h + 1) for li in range(cfg.num_layers)])
    v = torch.stack([11.0 + li + 1.1 * 2.0 ** (h % 4 - 1) for li in range(cfg.num_layers)])
    return k, v


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    """{model: checkpoint dir} of the outlier weights; tiny's also carries scales."""
    out = {}
    for name in ("tiny", "tiny-2k"):
        cfg = MODELS[name]
        layers, embed = _outlier_layers(cfg)
        d = str(tmp_path_factory.mktemp(f"kvs-{name}"))
        scales = None
        if name == "tiny":
            k, v = _ckpt_scales(cfg)
            scales = {"k": list(k), "v": list(v)}
        W.save_hf_checkpoint(cfg, layers, embed, torch.ones(cfg.hidden_size).bfloat16(), None, d,
                             kv_scales=scales)
        out[name] = d
    return out


def _prefill_logits(m, T, kv):
    bs = 16
    nblk = max(8, -(-T // bs))
    dev = m.device
    ids = torch.arange(100, 100 + T, dtype=torch.int32, device=dev)
    tiles, _ = ops.build_prefill_tiles([T], ops.prefill_tile_tokens(m.nq, m.nkv))
    meta = AttnMeta(
        positions=torch.arange(T, dtype=torch.int32, device=dev),
        slot_mapping=torch.arange(T, dtype=torch.int32, device=dev),
        block_tables=torch.arange(nblk, dtype=torch.int32, device=dev)[None],
        seq_lens=torch.tensor([T], dtype=torch.int32, device=dev),
        logits_indices=torch.arange(T, device=dev),
        q_start_loc=torch.tensor([0, T], dtype=torch.int32, device=dev if dev.type == "cuda" else "cpu"),
        tile_info=torch.tensor(tiles, dtype=torch.int32, device=dev).flatten(),
        num_tiles=len(tiles))
    return m.compute_logits(m.forward(ids, meta, kv)).float().cpu()


def _cos_agree(a, b):
    cos = torch.nn.functional.cosine_similarity(a, b, dim=-1).min().item()
    agree = (a.argmax(-1) == b.argmax(-1)).float().mean().item()
    return cos, agree


@pytest.mark.parametrize("model", ["tiny-2k", "tiny"])
def test_model_calibrated_scales_recover_outlier_heads(model, ckpts):
    cfg = MODELS[model]
    T, bs = 200, 16
    nblk = max(8, -(-T // bs))
    c = LlamaModel(cfg, torch.device("cpu"), torch.float32, max_model_len=512)
    c.load_checkpoint(ckpts[model])
    kv = c.allocate_kv_cache(nblk, bs)
    truth = _prefill_logits(c, T, kv)
    absmax = min(min(k.abs().max().item(), v.abs().max().item()) for k, v in kv)
    assert absmax > 4 * 448, absmax    # precondition: scale 1.0 must clip heavily

    g = LlamaModel(cfg, torch.device("cuda"), torch.bfloat16, max_model_len=512)
    g.load_checkpoint(ckpts[model])
    # control: fp8 caches at scale 1.0
    cos1, _ = _cos_agree(_prefill_logits(g, T, g.allocate_kv_cache(nblk, bs, F8)), truth)
    print(f"{model}: scale one min cos {cos1:.4f}")
    assert cos1 < 0.9, cos1

    prompt = kv_calibrate.calibration_prompt_ids(ChatTemplate(get_tokenizer(None)),
                                                 vocab=cfg.vocab_size)
    assert len(prompt) >= 256
    ks, vs = kv_calibrate.calibrate(g, prompt)
    assert ks.min().item() > 1 and vs.min().item() > 1
    got = _prefill_logits(g, T, g.allocate_kv_cache(nblk, bs, F8))
    cos, agree = _cos_agree(got, truth)
    print(f"{model}: calibrated vs fp32-KV truth min cos {cos:.5f} argmax agreement {agree:.3f}")
    assert cos > 0.99, cos
    assert agree >= 0.7, agree

    c.set_kv_scales(ks, vs)       # the CPU reference over fp8 caches at the same scales
    same = _prefill_logits(c, T, c.allocate_kv_cache(nblk, bs, F8))
    cos8, agree8 = _cos_agree(got, same)
    print(f"{model}: calibrated vs CPU fp8 min cos {cos8:.5f} argmax agreement {agree8:.3f}")
    assert cos8 > 0.99, cos8
    assert agree8 >= 0.7, agree8


# ------------------------------------------------------------------------ 6. engine

def _engine(**kw):
    base = dict(model="tiny", device="cuda", num_kv_blocks=512, max_model_len=2048,
                max_num_seqs=16)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def test_engine_calibrate_graph_matches_eager(ckpts):
    rng = np.random.default_rng(0)
    prompts = [rng.integers(0, 120000, l).tolist() for l in [5, 17, 33, 64, 100]]
    sp = SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True)
    kw = dict(model="tiny-2k", weights=ckpts["tiny-2k"], kv_cache_dtype="fp8", kv_scales="calibrate")
    e1 = _engine(enforce_eager=False, **kw)
    info = e1.metrics()["kv_scales"]
    assert info["source"] == "calibrate"
    assert info["k_min"] > 1 and info["v_min"] > 1, info
    a = e1.generate(prompts, sp)
    assert e1.runner.stats.get("graph_replays", 0) > 0
    b = _engine(enforce_eager=True, **kw).generate(prompts, sp)
    assert a == b


def test_engine_reports_checkpoint_scales(ckpts):
    cfg = MODELS["tiny"]
    e = _engine(model="tiny", weights=ckpts["tiny"], kv_cache_dtype="fp8", kv_scales="auto")
    k, v = _ckpt_scales(cfg)
    m = e.runner.model
    assert torch.equal(torch.stack([s[0] for s in m.kv_scales]).cpu(), k)
    assert torch.equal(torch.stack([s[1] for s in m.kv_scales]).cpu(), v)
    assert torch.equal(torch.stack([s[2] for s in m.kv_scales]).cpu(), 1.0 / k)
    info = e.metrics()["kv_scales"]
    assert info["source"] == "checkpoint"
    assert info["k_min"] == k.min().item() and info["k_max"] == k.max().item()
    assert info["v_min"] == v.min().item() and info["v_max"] == v.max().item()
    out = e.generate([list(range(100, 140))], SamplingParams(temperature=0.0, max_tokens=8,
                                                             ignore_eos=True))
    assert len(out[0]) == 8
    # the same checkpoint with kv_scales="one" ignores them
    e1 = _engine(model="tiny", weights=ckpts["tiny"], kv_cache_dtype="fp8", kv_scales="one")
    assert e1.runner.model.kv_scales is None and e1.metrics()["kv_scales"]["source"] == "one"
