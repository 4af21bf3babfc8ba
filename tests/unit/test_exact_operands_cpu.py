"""ops/exact.py on the CPU: the exactness bound fires, the shipped parameter sets are
order-independent in fp32 (what tests/test_gemm_exact_gpu.py relies on, shown on the
reference side alone), bf16_ulp_diff and the guarded buffers behave."""
import pytest
import torch

from fasttalk_llm_microservice_amd.ops import exact as E
from fasttalk_llm_microservice_amd.ops import quant as Q


def test_bound_assertion_fires():
    E.int_operands(4, 16, 4096, x_max=7, w_max=15)
    with pytest.raises(AssertionError, match="exactness bound"):
        E.int_operands(8, 64, 14336, x_max=64, w_max=128)       # ~2**27 units
    with pytest.raises(AssertionError, match="exactness bound"):
        E.w4_int_operands(8, 64, 14336, x_max=16, n_scales=3)   # ~4e7 units of 2**-7
    E.w4_int_operands(8, 64, 14336, x_max=2, n_scales=3)
    with pytest.raises(AssertionError, match="bf16"):
        E.int_operands(2, 16, 64, x_max=300, w_max=1)           # 257 needs 9 bits
    x, w, _ = E.int_operands(2, 16, 64)
    with pytest.raises(AssertionError, match="integer multiple"):
        E.assert_exact_bound(x, w * 0.5, 2.0 ** -6)


def _shuffled_fp32(x, w, chunk, seed):
    """x w^T accumulated in fp32 over K chunks taken in a shuffled order."""
    k = x.shape[1]
    order = torch.randperm(k // chunk, generator=torch.Generator().manual_seed(seed)).tolist()
    acc = torch.zeros(x.shape[0], w.shape[0], dtype=torch.float32)
    for c in order:
        sl = slice(c * chunk, (c + 1) * chunk)
        acc = acc + x[:, sl].float() @ w[:, sl].float().t()
    return acc


@pytest.mark.parametrize("name", sorted(E.BF16_SETS))
def test_bf16_sets_are_order_independent(name):
    p = E.BF16_SETS[name]
    x, w, exact = E.int_operands(17, 48, **p, seed=3)
    for chunk, seed in ((64, 0), (256, 1), (512, 2)):
        acc = _shuffled_fp32(x, w, chunk, seed)
        assert torch.equal(acc.double(), exact)
    assert torch.equal((exact / 2.0 ** -p["w_shift"]).round(), exact / 2.0 ** -p["w_shift"])
    # a residual in the same units keeps fp32 exact
    res = E.int_residual(17, 48, w_shift=p["w_shift"])
    assert torch.equal((res.float() + exact.float()).double(), res.double() + exact)


@pytest.mark.parametrize("name", sorted(E.W4_SETS))
def test_w4_sets_are_order_independent(name):
    """The W4 kernels' arithmetic in fp32, groups in a shuffled order: acc = x (128 + q)
    per group, then s * (acc - (128 + z) * sum(x)) -- and the variant that subtracts the
    zero-point term after the loop."""
    p = E.W4_SETS[name]
    m, n = 9, 32
    x, q, z, s, exact = E.w4_int_operands(m, n, **p, seed=5)
    k = p["k"]
    groups = torch.randperm(k // 128, generator=torch.Generator().manual_seed(1)).tolist()
    fused = torch.zeros(m, n)
    main, zp = torch.zeros(m, n), torch.zeros(m, n)
    for g in groups:
        sl = slice(g * 128, (g + 1) * 128)
        xf = x[:, sl].float()
        acc = xf @ (128.0 + q[:, sl].float()).t()
        xs = xf.sum(-1, keepdim=True)
        sg, zg = s[:, g][None, :], 128.0 + z[:, g].float()[None, :]
        fused = fused + sg * (acc - zg * xs)
        main = main + sg * acc
        zp = zp + sg * zg * xs
    assert torch.equal(fused.double(), exact)
    assert torch.equal((main - zp).double(), exact)
    # pack / unpack keeps the operands (the GPU tests hand pack_w4 images to the kernels)
    q2, z2, s2 = Q.unpack_w4(Q.pack_w4(q, z, s))
    assert torch.equal(q2, q) and torch.equal(z2, z) and torch.equal(s2, s)
    assert torch.equal(Q.dequantize_w4(q, z, s).double(), E.w4_dequant_exact(q, z, s))


def test_onehot_operands_name_the_column():
    _, w, _ = E.int_operands(1, 32, 2048)
    ks = E.onehot_ks(2048, 512, 1024, 24)
    assert len(set(ks)) == 24 and all(0 <= v < 2048 for v in ks)
    for edge in (0, 7, 8, 15, 16, 63, 64, 511, 512, 1023, 1024, 2047):
        assert edge in ks
    x, exact = E.onehot_operands(24, ks, w)
    assert torch.equal(x.double() @ w.double().t(), exact)
    got = exact.clone()
    got[5, 3] += 1.0
    assert f"k = {ks[5]}" in E.explain_onehot(got, exact, ks)


def test_silu_operands_ranges():
    for eps in (None, 0.5):
        # (|x| <= 2 with the norm: mean(x^2) ~ 2, so eps = 0.5 moves the scale by ~10%)
        x, w, gate, up = E.silu_operands(33, 64, 2048, x_max=7 if eps is None else 2, seed=2,
                                         norm_eps=eps)
        rs = E.row_rms_scale(x, eps) if eps is not None else None
        g = gate * rs if rs is not None else gate
        assert float(g.abs().max()) < E.MAX_GATE and float(g.max()) >= 30 and float(g.min()) <= -30
        assert float((g[:, 4:].abs() <= 8).double().mean()) > 0.9
        ref = E.silu_ref(gate, up, rs)
        assert ref.dtype == torch.bfloat16 and torch.isfinite(ref.float()).all()
        # eps matters: the reference with the usual 1e-5 is far more than a step away
        if eps is not None:
            other = E.silu_ref(gate[:, 4:], up[:, 4:], E.row_rms_scale(x, 1e-5))
            d = E.bf16_ulp_diff(ref[:, 4:].contiguous(), other)
            assert float((d > 1).double().mean()) > 0.9     # (exact zeros stay zeros)


def _bf16_bits(*bits):
    return torch.tensor([b - 0x10000 if b >= 0x8000 else b for b in bits],
                        dtype=torch.int16).view(torch.bfloat16)


def test_bf16_ulp_diff():
    pz, nz = _bf16_bits(0x0000), _bf16_bits(0x8000)
    assert int(E.bf16_ulp_diff(pz, nz)) == 0
    # across a power of two: 0x3F7F is the bf16 just below 1.0 = 0x3F80
    assert int(E.bf16_ulp_diff(_bf16_bits(0x3F7F), _bf16_bits(0x3F81))) == 2
    # across the sign change: smallest positive and smallest negative subnormal
    assert int(E.bf16_ulp_diff(_bf16_bits(0x0001), _bf16_bits(0x8001))) == 2
    assert int(E.bf16_ulp_diff(_bf16_bits(0x8003), pz)) == 3
    a = torch.tensor([1.0, -2.0, 3.0]).bfloat16()
    assert E.bf16_ulp_diff(a, a.clone()).tolist() == [0, 0, 0]
    assert int(E.bf16_ulp_diff(_bf16_bits(0x7FC0), _bf16_bits(0x3F80))) >= 1 << 16
    with pytest.raises(AssertionError, match="more than one"):
        E.assert_ulp1(_bf16_bits(0x3F80, 0x3F82), _bf16_bits(0x3F81, 0x3F80), "demo")
    assert E.assert_ulp1(_bf16_bits(0x3F80, 0x3F80), _bf16_bits(0x3F81, 0x3F80), "demo") == 0.5


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_guarded_catches_pad_writes(dtype):
    fill = E.PAD_BF16 if dtype == torch.bfloat16 else E.NAN_F32
    g = E.guarded(5, 40, 16, 64, dtype, fill)
    assert g.view.shape == (5, 40) and g.view.stride(0) % 8 == 0 and g.view.data_ptr() % 16 == 0
    g.view.fill_(1.0)                      # the legitimate footprint
    g.check("clean")
    r0, c0 = g.region[0].start, g.region[1].start
    for r, c, what in ((r0 + 5, c0, "row pad below"), (r0 - 1, c0 + 39, "row pad above"),
                       (r0 + 4, c0 + 40, "column pad behind"), (r0, c0 - 1, "column pad in front")):
        g = E.guarded(5, 40, 16, 64, dtype, fill)
        g.buf[r, c] = 0.0
        with pytest.raises(AssertionError, match="outside the view"):
            g.check(what)
    # a NaN fill is compared by bit pattern, so an untouched NaN pad passes and a
    # different NaN does not
    g = E.guarded_from(torch.ones(3, 16, dtype=dtype))
    g.check("nan pad")
    assert torch.isnan(g.buf[0, 0]) and torch.equal(g.view, torch.ones(3, 16, dtype=dtype))
    g.buf[0, 0] = float("nan")
    with pytest.raises(AssertionError, match="outside the view"):
        g.check("other nan")


def test_guarded_flat_catches_tail_write():
    g = E.guarded_flat(100, tail=32)
    assert g.buf.numel() == 132 and g.buf.is_contiguous() and torch.isnan(g.buf).all()
    g.view.zero_()
    g.check("clean")
    g.buf[100] = 1.0
    with pytest.raises(AssertionError, match="outside the view"):
        g.check("tail")
    t = E.guarded_flat(8, tail=4, dtype=torch.int32, fill=0x5A5A5A5A)
    t.view.zero_()
    t.check("tickets")
    t.buf[11] = 0
    with pytest.raises(AssertionError, match="outside the view"):
        t.check("ticket tail")
