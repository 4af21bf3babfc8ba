"""Bit-exact tests of the GEMM family and its slab epilogues.

Operands are small integers times a power of two (ops/exact.py), so every partial sum
is exact in fp32 in any order: a kernel's output must EQUAL the fp64 product -- bf16
outputs its single RNE rounding, fp32 slabs its exact split -- whatever the tiling,
ring depth or split-K.  SiLU / norm epilogues cannot be exact; they are held to one
bf16 step of the fp64 reference of the exact sums (the device's exp, reciprocal and
rsqrt are good to a few fp32 ulps and SiLU's condition number is <= 1 + |g|, so for
|g| < 60 the fp32 value is within ~1e-5 of the truth: the bf16 output can differ from
RNE(reference) only next to a rounding tie, by one step).  Fused norms get eps = 0.5
on rows with mean(x^2) ~ 2, where a dropped or misplaced eps moves the result by ~10%.

Configurations come from the plans in models/llama.py and the instantiation lists in
ops, not from copies: a configuration added later is covered or fails loudly here.
Shapes are the smallest that reach every edge (two workgroups of columns plus a tail
where the kernel takes one, every split at least two K chunks and more chunks than the
ring is deep, uneven k-steps per wave), not the model's.

The footprint tests (``*_footprint``) embed every buffer in a guarded allocation: x
surrounded by NaN rows and columns, out / residual / workspace / tickets by a fixed bit
pattern that must survive the launch; every slab element must have been written.
(decode_block takes contiguous operands only, so its buffers are guarded by rows and
tails, not by columns.)
"""
import pytest
import torch

from fasttalk_llm_microservice_amd import ops
from fasttalk_llm_microservice_amd.models import llama as L
from fasttalk_llm_microservice_amd.ops import exact as E
from fasttalk_llm_microservice_amd.ops import quant as Q

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
EPS = 0.5
DECODE_ROWS = (1, 15, 16, 17, 33, 64)
PREFILL_ROWS = (65, 129, 300)
SLAB_SPLITS = (1, 2, 4, 5, 8)     # the consumers read slabs 4 at a time, clamped: 5 has a tail
_P = E.BF16_SETS["gemm"]
UNIT = 2.0 ** -_P["w_shift"]
_P4 = E.W4_SETS["gemm"]
UNIT4 = 2.0 ** _P4["s_exp"]
MAX_M, MAX_N, MAX_K = 300, 1040, _P["k"]


@pytest.fixture(autouse=True)
def _native_loaded():
    ops.native()  # fail loudly if the extension is missing


# ---------------------------------------------------------------------------------
# operands: one master set per family, computed once, sliced per case and never changed
# (a slice of operands inside the exactness bound is inside it too)
# ---------------------------------------------------------------------------------

_cache = {}


def _master():
    if "bf16" not in _cache:
        x, w, _ = E.int_operands(MAX_M, MAX_N, seed=11, device=DEV, **_P)
        res = E.int_residual(64, MAX_N, w_shift=_P["w_shift"], seed=12, device=DEV)
        _cache["bf16"] = (x, w, res)
    return _cache["bf16"]


def _case(m, n, k):
    """(x [m, k], w [n, k], exact fp64 [m, n]) on the GPU."""
    assert m <= MAX_M and n <= MAX_N and k <= MAX_K, (m, n, k)
    xm, wm, _ = _master()
    x, w = xm[:m, :k].contiguous(), wm[:n, :k].contiguous()
    return x, w, E.exact_product(x, w)


def _res0(m, n):
    return _master()[2][:m, :n].contiguous()


def _master4():
    if "w4" not in _cache:
        x, q, z, s, _ = E.w4_int_operands(MAX_M, MAX_N, seed=13, device=DEV, **_P4)
        _cache["w4"] = (x, q, z, s)
    return _cache["w4"]


def _case4(m, n, k):
    """(x, packed W4 weight, dequantized fp64 weights [n, k], exact)."""
    xm, qm, zm, sm = _master4()
    assert m <= xm.shape[0] and n <= qm.shape[0] and k <= qm.shape[1], (m, n, k)
    x = xm[:m, :k].contiguous()
    q, z, s = qm[:n, :k].contiguous(), zm[:n, :k // 128].contiguous(), sm[:n, :k // 128].contiguous()
    wd = E.w4_dequant_exact(q, z, s)
    return x, Q.pack_w4(q, z, s), wd, x.double() @ wd.t()


def _silu_case(m, inter, k, norm=False, il=1):
    """(x, packed interleaved gate_up image, fp64 reference h rounded once to bf16)."""
    key = ("silu", m, inter, k, norm)
    if key not in _cache:
        x, w, gate, up = E.silu_operands(m, inter, k, x_max=2 if norm else 7, seed=m + inter,
                                         norm_eps=EPS if norm else None, device=DEV)
        ref = E.silu_ref(gate, up, E.row_rms_scale(x, EPS) if norm else None)
        _cache[key] = (x, w, ref)
    x, w, ref = _cache[key]
    return x, ops.pack_weight(ops.interleave_gate_up(w, il)), ref


def _silu_case4(m, inter, k):
    key = ("silu4", m, inter, k)
    if key not in _cache:
        x, q, z, s, gate, up = E.w4_silu_operands(m, inter, k, seed=m + inter, device=DEV)
        il = ops.interleave_gate_up
        _cache[key] = (x, Q.pack_w4(il(q, 1), il(z, 1), il(s, 1)), E.silu_ref(gate, up))
    return _cache[key]


# ---------------------------------------------------------------------------------
# buffers and comparisons
# ---------------------------------------------------------------------------------

class Bufs:
    """The buffers of one launch; ``guard``: each inside a guarded allocation."""

    def __init__(self, guard):
        self.guard = guard
        self.guards = []

    def x(self, x):
        if not self.guard:
            return x
        return E.guarded_from(x, 16, 64).view       # NaN rows and columns around x

    def out(self, m, cols, init=None):
        if self.guard:
            g = E.guarded(m, cols, 16, 64, BF16, E.PAD_BF16, DEV)
            self.guards.append(("out / residual", g))
            t = g.view
        else:
            t = torch.empty(m, cols, dtype=BF16, device=DEV)
        if init is None:
            t.fill_(float("nan"))
        else:
            t.copy_(init)
        return t

    def ws(self, n):
        """fp32 workspace, all NaN: every slab element must be written by the launch."""
        g = E.guarded_flat(n, 4096 if self.guard else 0, device=DEV)
        self.guards.append(("workspace tail", g))
        return g.buf

    def tickets(self, n):
        g = E.guarded_flat(n, 64 if self.guard else 0, torch.int32, 0x5A5A5A5A, DEV)
        g.view.zero_()
        self.guards.append(("tickets", g))
        return g.buf

    def check(self):
        torch.cuda.synchronize()
        for what, g in self.guards:
            g.check(what)


def _eq(got, want, what):
    if torch.equal(got, want):
        return
    bad = (got != want) | torch.isnan(got.float())
    idx = tuple(int(v) for v in bad.nonzero()[0])
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at {idx}: "
                         f"got {float(got[idx])!r}, exact {float(want[idx])!r}")


def _eq_bf16(out, exact, what):
    _eq(out, exact.float().bfloat16(), what)


def _eq_slabs(ws, splits, m, n, exact, unit, what):
    s = ws[:splits * m * n].view(splits, m, n).double()
    assert bool(torch.isfinite(s).all()), f"{what}: slab elements left unwritten"
    units = s / unit
    assert torch.equal(units, units.round()), f"{what}: a slab element is no multiple of the unit"
    _eq(s.sum(0), exact, what)


def _onehot(m, k, chunk, k_slice, w):
    ks = E.onehot_ks(k, chunk, k_slice, m)
    x, exact = E.onehot_operands(m, ks, w)
    return x, exact, ks


def _eq_onehot(got, exact, ks, what):
    assert torch.equal(got.double(), exact), f"{what}: {E.explain_onehot(got, exact, ks)}"


# ---------------------------------------------------------------------------------
# ops.skinny_gemm  ("pk" u -3, "xc" -4, "xr" -5 / -7, SiLU -6 / -8)
# ---------------------------------------------------------------------------------

def _skinny_cfgs():
    s = set()
    for plan in (L.PACKED_PLAN, L.PACKED_PLAN_WIDE):
        for per in plan.values():
            s.update(tuple(c) for c in per.values())
    s.update((nt, -5, sp) for nt, sp in L.INV_PLAN.values())
    for nt, u in ops.SKINNY_CONFIGS:
        s.update({(nt, u, 1), (nt, u, 2)})
    for u in (-5, -7):
        for nt in (1, 2):
            s.update({(nt, u, 1), (nt, u, 2), (nt, u, 4)})
    s.update({(2, -6, 1), (2, -8, 1)})
    return sorted(s, key=lambda c: (-c[1], c[0], c[2]))


SKINNY = _skinny_cfgs()
SKINNY_STORE = [c for c in SKINNY if c[1] not in (-6, -8)]
SKINNY_SILU = [c for c in SKINNY if c[1] in (-6, -8)]


def _skinny_shape(nt, u, sp):
    """(N, K, K chunk): two workgroups of columns (three for pk, whose grid has no tail)
    plus a tail; per split three K chunks (pk: three rounds of its four waves plus one
    k-step, so the waves' step counts differ)."""
    if u == -3:
        return 48 * nt, (3 * 256 + 64) * sp, 256
    if u == -4:
        return 2 * 64 * nt + 64, 2 * 512 * sp, 512
    if u in (-5, -6, -7, -8):
        nw = 8 if u in (-7, -8) else 4
        kc = 512 if nt == 2 else 256
        tail = 32 if u in (-6, -8) else 16 * nt
        return 2 * nw * 16 * nt + tail, 3 * kc * sp, kc
    raise KeyError(f"skinny_gemm variant u = {u}: teach this test its tiling")


def _run_skinny(x, wp, m, n, nt, u, sp, guard=False):
    b = Bufs(guard)
    if sp == 1:
        out = b.out(m, n)
        ops.skinny_gemm(b.x(x), wp, out=out, nt=nt, u=u)
        return b, out, None
    ws = b.ws(sp * m * n)
    ops.skinny_gemm(b.x(x), wp, ws=ws, splits=sp, nt=nt, u=u)
    return b, None, ws


def _check_store(b, out, ws, sp, m, n, exact, unit, what):
    b.check()
    if ws is None:
        _eq_bf16(out, exact, what)
    else:
        _eq_slabs(ws, sp, m, n, exact, unit, what)


@pytest.mark.parametrize("m", DECODE_ROWS)
@pytest.mark.parametrize("nt,u,sp", SKINNY_STORE)
def test_skinny_gemm_exact(m, nt, u, sp):
    n, k, _ = _skinny_shape(nt, u, sp)
    assert L._cfg_fits((nt, u, sp), n, k)
    x, w, exact = _case(m, n, k)
    b, out, ws = _run_skinny(x, ops.pack_weight(w), m, n, nt, u, sp)
    _check_store(b, out, ws, sp, m, n, exact, UNIT, f"skinny_gemm nt {nt} u {u} splits {sp} m {m}")


@pytest.mark.parametrize("m", [65, 96, 100, 128])     # 16-row tile counts 5, 6, 7, 8
@pytest.mark.parametrize("nt,sp", [(1, 1), (2, 1), (2, 2)])
def test_skinny_gemm_xc_65_to_128_rows(m, nt, sp):
    """"xc" alone accepts 65..128 rows (its x chunk halves to 256 columns there)."""
    n, k, _ = _skinny_shape(nt, -4, sp)
    x, w, exact = _case(m, n, k)
    b, out, ws = _run_skinny(x, ops.pack_weight(w), m, n, nt, -4, sp)
    _check_store(b, out, ws, sp, m, n, exact, UNIT, f"skinny_gemm xc nt {nt} splits {sp} m {m}")


@pytest.mark.parametrize("m", DECODE_ROWS)
@pytest.mark.parametrize("nt,u,sp", SKINNY_SILU)
def test_skinny_gemm_silu_ulp(m, nt, u, sp):
    n, k, _ = _skinny_shape(nt, u, sp)
    x, wp, ref = _silu_case(m, n // 2, k)
    h = ops.skinny_gemm(x, wp, nt=nt, u=u)
    E.assert_ulp1(h, ref, f"skinny_gemm SiLU u {u} m {m}")


@pytest.mark.parametrize("nt,u,sp", [(2, -3, 2), (2, -4, 2), (1, -5, 2), (2, -5, 2), (2, -7, 2)])
def test_skinny_gemm_onehot(nt, u, sp):
    """One configuration per kernel template: y[i, :] == w[:, k_i] names a mis-read k."""
    m = 64
    n, k, chunk = _skinny_shape(nt, u, sp)
    _, w, _ = _case(1, n, k)
    x, exact, ks = _onehot(m, k, chunk, k // sp, w)
    _, _, ws = _run_skinny(x, ops.pack_weight(w), m, n, nt, u, sp)
    _eq_onehot(ws[:sp * m * n].view(sp, m, n).sum(0), exact, ks, f"skinny_gemm u {u} one-hot")
    out = ops.skinny_gemm(x, ops.pack_weight(w), nt=nt, u=u)
    _eq_onehot(out, exact, ks, f"skinny_gemm u {u} one-hot bf16")


@pytest.mark.parametrize("m", [17, 64])
@pytest.mark.parametrize("nt,u,sp", [(2, -3, 1), (2, -3, 2), (2, -4, 1), (2, -4, 2), (1, -5, 1),
                                     (2, -5, 2), (2, -7, 1), (1, -7, 2)])
def test_skinny_gemm_footprint(m, nt, u, sp):
    n, k, _ = _skinny_shape(nt, u, sp)
    x, w, exact = _case(m, n, k)
    b, out, ws = _run_skinny(x, ops.pack_weight(w), m, n, nt, u, sp, guard=True)
    _check_store(b, out, ws, sp, m, n, exact, UNIT, f"skinny_gemm guarded u {u} splits {sp} m {m}")


@pytest.mark.parametrize("m", [17, 64])
@pytest.mark.parametrize("u", [-6, -8])
def test_skinny_gemm_silu_footprint(m, u):
    n, k, _ = _skinny_shape(2, u, 1)
    x, wp, ref = _silu_case(m, n // 2, k)
    b = Bufs(True)
    h = b.out(m, n // 2)
    ops.skinny_gemm(b.x(x), wp, out=h, nt=2, u=u)
    b.check()
    E.assert_ulp1(h.contiguous(), ref, f"skinny_gemm SiLU guarded u {u} m {m}")


# ---------------------------------------------------------------------------------
# ops.pkr_gemm (fused decode layer GEMMs)
# ---------------------------------------------------------------------------------

def _pkr_cfgs():
    s = {tuple(c) for c in ops.PKR_CONFIGS}
    for per in L.FUSED_PLAN.values():
        s.update((c[0], c[1]) for c in per.values())
    return sorted(s)


PKR = _pkr_cfgs()
PKR_SILU = sorted(set(L._SILU_CONFIGS) | {(c[0], c[1]) for c in L.FUSED_PLAN["gu"].values()})
PKR_SPLITS = tuple(range(1, 9))
assert max(c[2] for per in L.FUSED_PLAN.values() for c in per.values()) <= PKR_SPLITS[-1]
assert L.MAX_FUSED_SPLITS <= PKR_SPLITS[-1]


def _pkr_rows(wn):
    return (33, 64) if wn else DECODE_ROWS      # the wave-split-N layout is for 33..64 rows


def _pkr_shape(nt, depth, sp, wn):
    """Three workgroups of columns (two with wn: 4 waves x nt tiles each).  Per split
    4 (depth + 1) + 1 k-steps: each of the four K-splitting waves walks more steps than
    the ring is deep (it wraps), wave 0 one more than the others."""
    return (2 * 64 * nt if wn else 48 * nt), (256 * (depth + 1) + 64) * sp, 256


def _pkr_params():
    return [pytest.param(nt, depth, sp, wn, m, id=f"nt{nt}-d{depth}-s{sp}-wn{int(wn)}-m{m}")
            for nt, depth in PKR for wn in (False, True) for sp in PKR_SPLITS
            for m in _pkr_rows(wn)]


def _pkr_store_exact(nt, depth, sp, wn, m, guard):
    n, k, _ = _pkr_shape(nt, depth, sp, wn)
    x, w, exact = _case(m, n, k)
    wp = ops.pack_weight(w)
    b = Bufs(guard)
    out, ws = (b.out(m, n), None) if sp == 1 else (None, b.ws(sp * m * n))
    ops.pkr_gemm(b.x(x), wp, out=out, ws=ws, splits=sp, nt=nt, depth=depth, wn=wn)
    _check_store(b, out, ws, sp, m, n, exact, UNIT, f"pkr store nt {nt} depth {depth} splits {sp}")


@pytest.mark.parametrize("nt,depth,sp,wn,m", _pkr_params())
def test_pkr_store_exact(nt, depth, sp, wn, m):
    _pkr_store_exact(nt, depth, sp, wn, m, guard=False)


def _pkr_resid_exact(nt, depth, sp, wn, m, guard):
    n, k, _ = _pkr_shape(nt, depth, sp, wn)
    x, w, exact = _case(m, n, k)
    wp = ops.pack_weight(w)
    res0 = _res0(m, n)
    b = Bufs(guard)
    ws = b.ws(sp * m * n) if sp > 1 else None
    tickets = b.tickets(n // (16 * nt))
    xg = b.x(x)
    outs = []
    for _ in range(3):
        if ws is not None:
            ws[:sp * m * n].fill_(float("nan"))      # every launch has to write every slab element
        res = b.out(m, n, init=res0)
        ops.pkr_gemm(xg, wp, "resid", residual=res, ws=ws, tickets=tickets, splits=sp, nt=nt,
                     depth=depth, wn=wn)
        outs.append(res)
    b.check()
    what = f"pkr resid nt {nt} depth {depth} splits {sp} wn {wn} m {m}"
    assert int(tickets[:n // (16 * nt)].abs().sum()) == 0, f"{what}: tickets not re-armed"
    _eq_bf16(outs[0], res0.double() + exact, what)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), f"{what}: relaunch differs"
    if ws is not None:
        # Deliberate: this pins that a resid launch leaves ALL ``splits`` slabs in the
        # workspace, the last arriver's included (it re-reads its own slab so the sum runs
        # in split order).  A rewrite that keeps the last slab in registers is legitimate;
        # it then has to relax this check to the slabs it still writes.
        _eq_slabs(ws, sp, m, n, exact, UNIT, what + " slabs")


@pytest.mark.parametrize("nt,depth,sp,wn,m", _pkr_params())
def test_pkr_resid_exact(nt, depth, sp, wn, m):
    """residual == bf16(res0 + x W^T): one rounding of the fp32 sum, bit-identical
    across three launches, tickets left zero."""
    _pkr_resid_exact(nt, depth, sp, wn, m, guard=False)


def _pkr_silu_norm_ulp(nt, depth, wn, m, guard):
    n, k, _ = _pkr_shape(nt, depth, 1, wn)
    x, wp, ref = _silu_case(m, n // 2, k, norm=True, il=nt // 2)
    b = Bufs(guard)
    h = b.out(m, n // 2)
    ops.pkr_gemm(b.x(x), wp, "silu", out=h, nt=nt, depth=depth, norm=True, eps=EPS, wn=wn)
    b.check()
    E.assert_ulp1(h.contiguous(), ref, f"pkr silu+norm nt {nt} depth {depth} wn {wn} m {m}")


@pytest.mark.parametrize("m,wn", [(m, wn) for wn in (False, True) for m in _pkr_rows(wn)])
@pytest.mark.parametrize("nt,depth", PKR_SILU)
def test_pkr_silu_norm_ulp(nt, depth, wn, m):
    """silu + norm, eps = 0.5.  (The kernel instantiates its SiLU epilogue only with
    the fused norm, so there is no plain ``silu`` variant to cover.)"""
    _pkr_silu_norm_ulp(nt, depth, wn, m, guard=False)


def test_pkr_plain_silu_is_not_built():
    """Documents the gap above: if a plain SiLU epilogue appears, cover it here."""
    x, wp, _ = _silu_case(16, 48, 832)
    with pytest.raises(RuntimeError, match="launch failed"):
        ops.pkr_gemm(x, wp, "silu", nt=2, depth=2, norm=False)
    torch.cuda.synchronize()


@pytest.mark.parametrize("wn", [False, True])
@pytest.mark.parametrize("epi", ["store", "resid"])
def test_pkr_onehot(epi, wn):
    nt, depth, sp, m = 2, 3, 2, 64
    n, k, chunk = _pkr_shape(nt, depth, sp, wn)
    _, w, _ = _case(1, n, k)
    x, exact, ks = _onehot(m, k, chunk, k // sp, w)
    wp = ops.pack_weight(w)
    ws = torch.full((sp * m * n,), float("nan"), device=DEV)
    if epi == "store":
        ops.pkr_gemm(x, wp, ws=ws, splits=sp, nt=nt, depth=depth, wn=wn)
        got = ws.view(sp, m, n).sum(0)
    else:
        got = torch.zeros(m, n, dtype=BF16, device=DEV)
        tickets = torch.zeros(n // (16 * nt), dtype=torch.int32, device=DEV)
        ops.pkr_gemm(x, wp, "resid", residual=got, ws=ws, tickets=tickets, splits=sp, nt=nt,
                     depth=depth, wn=wn)
    _eq_onehot(got, exact, ks, f"pkr {epi} wn {wn} one-hot")


_PKR_FOOT = [(2, 3, 1, False, 17), (2, 3, 4, False, 64), (4, 2, 8, True, 33), (1, 4, 2, False, 15),
             (4, 2, 1, True, 64)]


@pytest.mark.parametrize("nt,depth,sp,wn,m", _PKR_FOOT)
def test_pkr_store_footprint(nt, depth, sp, wn, m):
    _pkr_store_exact(nt, depth, sp, wn, m, guard=True)


@pytest.mark.parametrize("nt,depth,sp,wn,m", _PKR_FOOT)
def test_pkr_resid_footprint(nt, depth, sp, wn, m):
    _pkr_resid_exact(nt, depth, sp, wn, m, guard=True)


@pytest.mark.parametrize("nt,depth,wn,m", [(2, 4, False, 17), (4, 2, True, 33), (4, 3, False, 64)])
def test_pkr_silu_norm_footprint(nt, depth, wn, m):
    _pkr_silu_norm_ulp(nt, depth, wn, m, guard=True)


# ---------------------------------------------------------------------------------
# ops.packed_gemm (any M)
# ---------------------------------------------------------------------------------

# the tile configurations of csrc/kernels/packed_gemm.hip that tests/test_kernels_gpu.py
# lists (classic 0 1 2 5 6, phased 3, BK-32 ring 10..14) and whatever the plan adds
PG_CFGS = sorted({0, 1, 2, 3, 5, 6, 10, 11, 12, 13, 14} | {c for per in L.PG_PLAN.values()
                                                           for _, c, _ in per})
PG_SILU_CFGS = PG_CFGS      # (the model's gate_up picks cfg 2 with the SiLU epilogue too)
PG_N, PG_KSLICE = 528, 320       # 2 x 256 columns + 16; 5 BK-64 / 10 BK-32 chunks per split


def _pg_cases():
    s = {(c, sp) for per in L.PG_PLAN.values() for _, c, sp in per}
    s.update((c, sp) for c in PG_CFGS for sp in (1, 4))
    return sorted(s)


def _run_pg(x, wp, m, n, cfg, sp, guard):
    b = Bufs(guard)
    if sp == 1:
        out = b.out(m, n)
        ops.packed_gemm(b.x(x), wp, out=out, cfg=cfg)
        return b, out, None
    ws = b.ws(sp * m * n)
    ops.packed_gemm(b.x(x), wp, ws=ws, splits=sp, epi="slab", cfg=cfg)
    return b, None, ws


def _packed_gemm_exact(m, cfg, sp, guard):
    n, k = PG_N, PG_KSLICE * sp
    x, w, exact = _case(m, n, k)
    b, out, ws = _run_pg(x, ops.pack_weight(w), m, n, cfg, sp, guard)
    _check_store(b, out, ws, sp, m, n, exact, UNIT, f"packed_gemm cfg {cfg} splits {sp} m {m}")


@pytest.mark.parametrize("m", PREFILL_ROWS)
@pytest.mark.parametrize("cfg,sp", _pg_cases())
def test_packed_gemm_exact(m, cfg, sp):
    _packed_gemm_exact(m, cfg, sp, guard=False)


def _packed_gemm_silu_ulp(m, cfg, guard):
    inter, k = 272, PG_KSLICE
    x, wp, ref = _silu_case(m, inter, k)
    b = Bufs(guard)
    h = b.out(m, inter)
    ops.packed_gemm(b.x(x), wp, out=h, epi="silu", cfg=cfg)
    b.check()
    E.assert_ulp1(h.contiguous(), ref, f"packed_gemm SiLU cfg {cfg} m {m}")


@pytest.mark.parametrize("m", PREFILL_ROWS)
@pytest.mark.parametrize("cfg", PG_SILU_CFGS)
def test_packed_gemm_silu_ulp(m, cfg):
    _packed_gemm_silu_ulp(m, cfg, guard=False)


@pytest.mark.parametrize("cfg", [1, 3, 12])
def test_packed_gemm_onehot(cfg):
    m, n, sp = 129, PG_N, 2
    k = PG_KSLICE * sp
    _, w, _ = _case(1, n, k)
    x, exact, ks = _onehot(m, k, 64, k // sp, w)
    wp = ops.pack_weight(w)
    _eq_onehot(ops.packed_gemm(x, wp, cfg=cfg), exact, ks, f"packed_gemm cfg {cfg} one-hot")
    ws = torch.full((sp * m * n,), float("nan"), device=DEV)
    ops.packed_gemm(x, wp, ws=ws, splits=sp, epi="slab", cfg=cfg)
    _eq_onehot(ws.view(sp, m, n).sum(0), exact, ks, f"packed_gemm cfg {cfg} one-hot slabs")


@pytest.mark.parametrize("m", [65, 300])
@pytest.mark.parametrize("cfg,sp", [(1, 1), (1, 4), (3, 1), (3, 2), (12, 1), (12, 4), (6, 1)])
def test_packed_gemm_footprint(m, cfg, sp):
    _packed_gemm_exact(m, cfg, sp, guard=True)


@pytest.mark.parametrize("cfg", [1, 3, 12])
def test_packed_gemm_silu_footprint(cfg):
    _packed_gemm_silu_ulp(129, cfg, guard=True)


# ---------------------------------------------------------------------------------
# quant.w4_gemm (M <= 64): xr 0 register kernel, 1 "xr", 4 / 5 "mh"
# ---------------------------------------------------------------------------------

def _w4_cfgs():
    s = set()
    for per in L.W4_PLAN.values():
        s.update(tuple(c) for c in per.values())
    s.update(tuple(c) for c in L.W4_PLAN_MH.values())
    s.update(tuple(c) for c in L.W4_PLAN_WIDE.values())
    for xr in (0, 1):
        for nt in (1, 2, 4):
            s.update({(nt, 1, xr), (nt, 2, xr)})
    for xr in (4, 5):
        s.update({(2, 1, xr), (2, 2, xr), (2, 8, xr)})
    return sorted(s, key=lambda c: (c[2], c[0], c[1]))


def _w4_shape(nt, sp, xr):
    """(N, K, chunk): register kernel three workgroups, four waves x two 128-k groups
    plus one per split; xr two workgroups, three 512-k chunks per split; mh two
    128-column workgroups plus a 32-column tail, five 256-k chunks (ring 3 wraps)."""
    if xr == 0:
        return 48 * nt, (4 * 2 + 1) * 128 * sp, 128
    if xr == 1:
        return 2 * 64 * nt, 3 * 512 * sp, 512
    if xr in (4, 5):
        return 288, 5 * 256 * sp, 256
    raise KeyError(f"w4_gemm kernel xr = {xr}: teach this test its tiling")


def _w4_rows(xr):
    return DECODE_ROWS if xr == 0 else (17, 33, 64)      # the LDS kernels are built for > 16 rows


def _w4_params(cfgs):
    out = []
    for nt, sp, xr in cfgs:
        n, k, _ = _w4_shape(nt, sp, xr)
        assert L.w4_fits(xr, nt, sp, n, k), (nt, sp, xr, n, k)
        out += [pytest.param(nt, sp, xr, m, id=f"nt{nt}-s{sp}-xr{xr}-m{m}") for m in _w4_rows(xr)]
    return out


def _w4_gemm_exact(nt, sp, xr, m, guard):
    n, k, _ = _w4_shape(nt, sp, xr)
    x, W, _, exact = _case4(m, n, k)
    what = f"w4_gemm nt {nt} splits {sp} xr {xr} m {m}"
    b = Bufs(guard)
    xg = b.x(x)
    if sp == 1:
        out = b.out(m, n)
        Q.w4_gemm(xg, W, out=out, nt=nt, xr=xr)
    ws = b.ws(sp * m * n)
    Q.w4_gemm(xg, W, ws=ws, splits=sp, nt=nt, xr=xr)
    b.check()
    if sp == 1:
        _eq_bf16(out, exact, what)
    _eq_slabs(ws, sp, m, n, exact, UNIT4, what + " slabs")


@pytest.mark.parametrize("nt,sp,xr,m", _w4_params(_w4_cfgs()))
def test_w4_gemm_exact(nt, sp, xr, m):
    """bf16 store (one split) and fp32 slabs (every split count, one included)."""
    _w4_gemm_exact(nt, sp, xr, m, guard=False)


def _w4_gemm_silu_ulp(xr, m, guard):
    n, k, _ = _w4_shape(2, 1, xr)
    x, W, ref = _silu_case4(m, n // 2, k)
    b = Bufs(guard)
    h = b.out(m, n // 2)
    Q.w4_gemm(b.x(x), W, out=h, nt=2, xr=xr, silu=True)
    b.check()
    E.assert_ulp1(h.contiguous(), ref, f"w4_gemm SiLU xr {xr} m {m}")


@pytest.mark.parametrize("m", (17, 33, 64))
@pytest.mark.parametrize("xr", [1, 4, 5])
def test_w4_gemm_silu_ulp(xr, m):
    _w4_gemm_silu_ulp(xr, m, guard=False)


@pytest.mark.parametrize("nt,sp,xr", [(2, 2, 0), (2, 2, 1), (2, 2, 4), (2, 2, 5)])
def test_w4_gemm_onehot(nt, sp, xr):
    """y[i, :] == (q[:, k_i] - z) s: names the nibble that was mis-read."""
    m = 64
    n, k, chunk = _w4_shape(nt, sp, xr)
    _, W, wd, _ = _case4(1, n, k)
    x, exact, ks = _onehot(m, k, chunk, k // sp, wd)
    ws = torch.full((sp * m * n,), float("nan"), device=DEV)
    Q.w4_gemm(x, W, ws=ws, splits=sp, nt=nt, xr=xr)
    _eq_onehot(ws.view(sp, m, n).sum(0), exact, ks, f"w4_gemm xr {xr} one-hot")


@pytest.mark.parametrize("nt,sp,xr,m", [(2, 1, 0, 15), (4, 4, 0, 64), (2, 1, 1, 17), (2, 4, 1, 64),
                                        (2, 1, 4, 33), (2, 2, 4, 64), (2, 1, 5, 17), (2, 8, 5, 64)])
def test_w4_gemm_footprint(nt, sp, xr, m):
    _w4_gemm_exact(nt, sp, xr, m, guard=True)


@pytest.mark.parametrize("xr,m", [(1, 33), (4, 64), (5, 17)])
def test_w4_gemm_silu_footprint(xr, m):
    _w4_gemm_silu_ulp(xr, m, guard=True)


# ---------------------------------------------------------------------------------
# quant.w4_packed_gemm (any M)
# ---------------------------------------------------------------------------------

W4PG_CFGS = (0, 1, 2)
W4PG_KSLICE = 384                # three 128-k groups per split


def _w4pg_cases():
    s = {(c, sp) for per in L.W4PG_PLAN.values() for _, c, sp in per}
    assert {c for c, _ in s} <= set(W4PG_CFGS)
    s.update((c, sp) for c in W4PG_CFGS for sp in (1, 4))
    return sorted(s)


def _w4_packed_gemm_exact(m, n, cfg, sp, guard):
    k = W4PG_KSLICE * sp
    x, W, _, exact = _case4(m, n, k)
    what = f"w4_packed_gemm cfg {cfg} splits {sp} m {m} n {n}"
    b = Bufs(guard)
    xg = b.x(x)
    if sp == 1:
        out = b.out(m, n)
        Q.w4_packed_gemm(xg, W, out=out, cfg=cfg)
    ws = b.ws(sp * m * n)
    Q.w4_packed_gemm(xg, W, ws=ws, splits=sp, epi="slab", cfg=cfg)
    b.check()
    if sp == 1:
        _eq_bf16(out, exact, what)
    _eq_slabs(ws, sp, m, n, exact, UNIT4, what + " slabs")


@pytest.mark.parametrize("m", PREFILL_ROWS)
@pytest.mark.parametrize("n", [272, 528, 1040])
@pytest.mark.parametrize("cfg,sp", _w4pg_cases())
def test_w4_packed_gemm_exact(m, n, cfg, sp):
    _w4_packed_gemm_exact(m, n, cfg, sp, guard=False)


def _w4_packed_gemm_silu_ulp(m, cfg, guard):
    inter, k = 272, W4PG_KSLICE
    x, W, ref = _silu_case4(m, inter, k)
    b = Bufs(guard)
    h = b.out(m, inter)
    Q.w4_packed_gemm(b.x(x), W, out=h, epi="silu", cfg=cfg)
    b.check()
    E.assert_ulp1(h.contiguous(), ref, f"w4_packed_gemm SiLU cfg {cfg} m {m}")


@pytest.mark.parametrize("m", PREFILL_ROWS)
@pytest.mark.parametrize("cfg", W4PG_CFGS)
def test_w4_packed_gemm_silu_ulp(m, cfg):
    _w4_packed_gemm_silu_ulp(m, cfg, guard=False)


@pytest.mark.parametrize("cfg", W4PG_CFGS)
def test_w4_packed_gemm_onehot(cfg):
    m, n, sp = 129, 528, 2
    k = W4PG_KSLICE * sp
    _, W, wd, _ = _case4(1, n, k)
    x, exact, ks = _onehot(m, k, 128, k // sp, wd)
    ws = torch.full((sp * m * n,), float("nan"), device=DEV)
    Q.w4_packed_gemm(x, W, ws=ws, splits=sp, epi="slab", cfg=cfg)
    _eq_onehot(ws.view(sp, m, n).sum(0), exact, ks, f"w4_packed_gemm cfg {cfg} one-hot")


@pytest.mark.parametrize("cfg,sp,m", [(0, 1, 65), (0, 4, 300), (1, 1, 300), (2, 2, 129)])
def test_w4_packed_gemm_footprint(cfg, sp, m):
    _w4_packed_gemm_exact(m, 528, cfg, sp, guard=True)
    if sp == 1:
        _w4_packed_gemm_silu_ulp(m, cfg, guard=True)


# ---------------------------------------------------------------------------------
# slab consumers: ops.slab_store, ops.slab_silu, ops.row_rmsnorm
# ---------------------------------------------------------------------------------

SLAB_UNIT = 2.0 ** -11


def _int_slabs(splits, rows, cols, seed):
    """fp32 slabs of integers (|v| <= 2000) times 2**-11: sums of up to 8 need 14 bits,
    so the bf16 store really rounds; every partial sum is exact in fp32."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randint(-2000, 2001, (splits, rows, cols), generator=g).double() * SLAB_UNIT
    return s.float().to(DEV), s.sum(0).to(DEV)


def _slab_ws(b, slabs):
    ws = b.ws(slabs.numel())
    ws[:slabs.numel()].copy_(slabs.flatten())
    return ws


def _slab_store_exact(splits, guard):
    rows, cols = 37, 264
    slabs, total = _int_slabs(splits, rows, cols, splits)
    b = Bufs(guard)
    out = b.out(rows, cols)
    ops.slab_store(_slab_ws(b, slabs), splits, rows, cols, out)
    b.check()
    _eq_bf16(out, total, f"slab_store splits {splits}")


@pytest.mark.parametrize("splits", SLAB_SPLITS)
def test_slab_store_exact(splits):
    _slab_store_exact(splits, guard=True)


@pytest.mark.parametrize("splits", SLAB_SPLITS)
def test_row_rmsnorm_residual_exact(splits):
    """residual == bf16(res0 + sum of slabs) exactly; the normed row continues from that
    bf16 value: out = bf16(bf16(v inv) w) (the documented double rounding of
    row_add_rmsnorm).  With power-of-two norm weights the second rounding is exact, so
    out is within one step of bf16(v inv_fp64) w; eps = 0.5 on rows with mean(v^2) ~ 1."""
    rows, hidden = 5, 2048
    slabs, total = _int_slabs(splits, rows, hidden, 10 + splits)
    g = torch.Generator().manual_seed(20 + splits)
    res0 = (torch.randint(-128, 129, (rows, hidden), generator=g).double() * 2.0 ** -7).to(DEV)
    w = torch.pow(2.0, torch.randint(-1, 2, (hidden,), generator=g).double()).to(DEV)
    b = Bufs(True)
    out = b.out(rows, hidden)
    rg = E.guarded(rows, hidden, 16, 0, BF16, E.PAD_BF16, DEV, lead_cols=0)   # contiguous view
    rg.view.copy_(res0)
    assert rg.view.is_contiguous()
    ops.row_rmsnorm(out, w.to(BF16), EPS, rows, ws=_slab_ws(b, slabs), splits=splits,
                    residual=rg.view)
    b.check()
    rg.check("residual")
    v = (res0 + total).float().bfloat16()
    _eq(rg.view, v, f"row_rmsnorm residual splits {splits}")
    ref = ((v.double() * E.row_rms_scale(v, EPS)).to(BF16).double() * w).to(BF16)
    E.assert_ulp1(out.contiguous(), ref, f"row_rmsnorm out splits {splits}")


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("splits", SLAB_SPLITS)
def test_slab_silu_ulp(splits, interleaved):
    rows, inter = 23, 272
    g = torch.Generator().manual_seed(30 + splits)
    gate = torch.randint(-2048, 2049, (rows, inter), generator=g).double() * 2.0 ** -8   # +-8
    up = torch.randint(-2048, 2049, (rows, inter), generator=g).double() * 2.0 ** -8
    hot = torch.randint(30 * 256, 60 * 256, (rows, 4), generator=g).double() * 2.0 ** -8
    gate[:, :4] = hot * torch.tensor([1.0, -1.0, 1.0, -1.0], dtype=torch.float64)
    total = torch.cat([gate, up], dim=1)
    if interleaved:
        total = ops.interleave_gate_up(total.t().contiguous(), 1).t().contiguous()
    # split the totals into integer slabs: random parts, the last takes the remainder
    parts = torch.randint(-2000, 2001, (splits - 1, rows, 2 * inter), generator=g).double() * 2.0 ** -8
    slabs = torch.cat([parts, (total - parts.sum(0)).unsqueeze(0)]).float().to(DEV)
    assert torch.equal(slabs.double().sum(0).cpu(), total)
    b = Bufs(True)
    out = b.out(rows, inter)
    ops.slab_silu(_slab_ws(b, slabs), splits, rows, inter, out, interleaved=interleaved)
    b.check()
    E.assert_ulp1(out.contiguous(), E.silu_ref(gate, up).to(DEV),
                  f"slab_silu splits {splits} interleaved {interleaved}")


@pytest.mark.parametrize("sp", [2, 5])
def test_gemm_slabs_feed_consumers(sp):
    """The chain the engine runs: a split-K GEMM leaves slabs in a NaN-filled, guarded
    workspace; slab_store reads exactly those."""
    m = 33
    n, k, _ = _pkr_shape(2, 3, sp, False)
    x, w, exact = _case(m, n, k)
    b = Bufs(True)
    ws = b.ws(sp * m * n)
    ops.pkr_gemm(b.x(x), ops.pack_weight(w), ws=ws, splits=sp, nt=2, depth=3)
    out = b.out(m, n)
    ops.slab_store(ws, sp, m, n, out)
    b.check()
    _eq_bf16(out, exact, f"pkr slabs -> slab_store splits {sp}")


# ---------------------------------------------------------------------------------
# ops.decode_block: stage 1 exact, stage 3 adds exactly nothing
# ---------------------------------------------------------------------------------

BLOCK_H, BLOCK_KO, BLOCK_I = 4096, 4096, 14336    # the shape decode_block_plan accepts


@pytest.fixture(scope="module")
def block_layer():
    ops.native()
    plan = ops.decode_block_plan(BLOCK_H, BLOCK_KO, BLOCK_I)
    if plan is None:
        pytest.skip("decode block geometry does not fit this device")
    g = torch.Generator(device=DEV).manual_seed(5)
    p = dict(_P, k=BLOCK_KO)
    wo = (torch.randint(-p["w_max"], p["w_max"] + 1, (BLOCK_H, BLOCK_KO), device=DEV, generator=g)
          .double() * UNIT).to(BF16)
    attn = torch.randint(-p["x_max"], p["x_max"] + 1, (64, BLOCK_KO), device=DEV,
                         generator=g).to(BF16)
    E.assert_exact_bound(attn, wo, UNIT)
    wd = torch.randint(-15, 16, (BLOCK_H, BLOCK_I), device=DEV, generator=g).to(BF16)
    wgu = torch.zeros(2 * BLOCK_I, BLOCK_H, dtype=BF16, device=DEV)
    res0 = E.int_residual(64, BLOCK_H, w_shift=_P["w_shift"], seed=6, device=DEV)
    return dict(plan=plan, attn=attn, wo=wo, res0=res0, exact=E.exact_product(attn, wo),
                wo_pk=ops.pack_weight(wo), wgu_pk=ops.pack_weight(wgu), wd_pk=ops.pack_weight(wd))


@pytest.mark.parametrize("m", [1, 17, 33, 64])
def test_decode_block_stage1_exact(block_layer, m):
    """gate_up image all zeros: h == 0, so residual == bf16(res0 + attn Wo^T) -- one
    rounding of the exact sum (stage 1) to which the down projection adds exactly
    nothing (stage 3); counters left zero."""
    Lr = block_layer
    grid = Lr["plan"][3]
    ws = torch.full((ops.decode_block_ws_floats(BLOCK_H, m),), float("nan"), device=DEV)
    xg = torch.full(((grid // 2) * 2 * 4 * 256,), float("nan"), device=DEV)
    ctl = torch.zeros(ops.decode_block_ctl_words(), dtype=torch.int32, device=DEV)
    h = torch.full((64, BLOCK_I), float("nan"), dtype=BF16, device=DEV)
    res = Lr["res0"][:m].clone()
    ops.decode_block(Lr["attn"][:m].contiguous(), res, h, Lr["wo_pk"], Lr["wgu_pk"], Lr["wd_pk"],
                     ws, xg, ctl, EPS)
    torch.cuda.synchronize()
    assert int(ctl.abs().sum()) == 0, ctl.nonzero().flatten().tolist()
    _eq(h[:m], torch.zeros_like(h[:m]), f"decode_block h m {m}")
    _eq_bf16(res, Lr["res0"][:m].double() + Lr["exact"][:m], f"decode_block residual m {m}")


@pytest.mark.parametrize("m", [17, 64])
def test_decode_block_footprint(block_layer, m):
    """The same launch with every buffer guarded.  The binding takes contiguous operands
    (residual with exactly m rows), so the guards are rows and tails: attn between NaN
    rows, residual between pattern rows, h as m rows of a larger pattern-filled buffer
    (rows past m must stay untouched), pattern tails behind ws and ctl, and xg -- which
    the kernel takes but never uses -- untouched as a whole."""
    Lr = block_layer
    grid = Lr["plan"][3]
    ag = E.guarded(m, BLOCK_KO, 16, 0, BF16, E.NAN_BF16, DEV, lead_cols=0)
    ag.view.copy_(Lr["attn"][:m])
    rg = E.guarded(m, BLOCK_H, 16, 0, BF16, E.PAD_BF16, DEV, lead_cols=0)
    rg.view.copy_(Lr["res0"][:m])
    hg = E.guarded(m, BLOCK_I, 16, 0, BF16, E.PAD_BF16, DEV, lead_cols=0)
    hg.view.fill_(float("nan"))
    wsg = E.guarded_flat(ops.decode_block_ws_floats(BLOCK_H, m), 4096, device=DEV)
    xgg = E.guarded_flat(0, (grid // 2) * 2 * 4 * 256, device=DEV)
    cg = E.guarded_flat(ops.decode_block_ctl_words(), 64, torch.int32, 0x5A5A5A5A, DEV)
    cg.view.zero_()
    assert ag.view.is_contiguous() and rg.view.is_contiguous() and hg.view.is_contiguous()
    ops.decode_block(ag.view, rg.view, hg.view, Lr["wo_pk"], Lr["wgu_pk"], Lr["wd_pk"],
                     wsg.buf, xgg.buf, cg.buf, EPS)
    torch.cuda.synchronize()
    for what, g in (("attn", ag), ("residual", rg), ("h rows past m", hg), ("ws tail", wsg),
                    ("xg", xgg), ("ctl tail", cg)):
        g.check(f"decode_block {what} m {m}")
    assert int(cg.view.abs().sum()) == 0, cg.view.nonzero().flatten().tolist()
    _eq(hg.view, torch.zeros_like(hg.view), f"decode_block guarded h m {m}")
    _eq_bf16(rg.view, Lr["res0"][:m].double() + Lr["exact"][:m], f"decode_block guarded residual m {m}")
