"""Model runner: turns a :class:`ScheduledBatch` into device metadata, runs the
forward pass + sampler, returns sampled token ids.

Decode steps replay hipGraphs (``torch.cuda.CUDAGraph`` is hipGraph on ROCm),
one per (batch bucket, split bucket): the graph covers embedding -> 32 layers ->
final norm -> LM head -> sampler, with every input in static device buffers
that are refreshed by one pinned-host -> device copy per step.  Prefill steps
run eagerly (variable token counts) through the same HIP kernels.
"""
from __future__ import annotations

import contextlib
import logging
import math
import os
import time
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import ops
from ..models.config import ModelConfig
from ..models.llama import AttnMeta, LlamaModel
from ..parallel.comm import SINGLE, TPComm
from .config import EngineConfig
from .sampling_params import ln_min_p
from .scheduler import ScheduledBatch

log = logging.getLogger("fasttalk.engine.runner")


class DecodeBlockFault(RuntimeError):
    """A persistent decode-block launch gave up at a grid barrier: the step's rows
    (and the K/V they wrote) are garbage."""


class KernelCheckError(RuntimeError):
    """The bounds-checked kernel build (FT_KERNEL_CHECKS=1) caught an out-of-range
    index (block-table entry, KV slot, rotary position, token id) in a step."""

    CODES = {1: "block-table entry >= num_blocks", 2: "KV slot >= pool capacity",
             3: "position >= rotary table rows", 4: "input token id >= vocab",
             5: "sampled token id >= vocab", 6: "KV copy/swap block id >= num_blocks",
             7: "penalty slot >= max_num_seqs", 8: "penalty token id >= vocab",
             9: "logprob alternatives > 20", 10: "prompt-logprob target id >= vocab"}

    def __init__(self, word):
        count, code, ctx, value = (int(x) for x in word[:4])
        self.count, self.code, self.ctx, self.value = count, code, ctx, value
        super().__init__(f"kernel bounds check: {self.CODES.get(code, f'code {code}')} "
                         f"(row/token {ctx}, value {value}; {count} violation(s))")


class CommFault(RuntimeError):
    """A tensor-parallel collective of this step timed out (custom all-reduce spin
    budget): the step's tokens are discarded and the group now runs on RCCL."""


def _pow2_ceil(x: int) -> int:
    return 1 << max(0, (x - 1).bit_length())


def input_words(mb: int, max_blocks: int) -> int:
    return 10 * mb + mb * max_blocks


def pen_words(mb: int) -> int:
    """int32 words of a step's per-row penalty arrays: slot | rep | pres | freq.  They sit
    IN FRONT of the decode inputs in the staging image and the device buffer, so a step
    with a penalised row uploads them in the same copy (it starts 4 * mb words earlier)
    and a step without one uploads exactly what it always did."""
    return 4 * mb


def minp_words(mb: int) -> int:
    """fp32 words of a step's per-row ln(min_p) (-inf = off).  They sit between the penalty
    prefix and the decode inputs (pen | min_p | inputs): a step with a min_p row starts
    its one copy at them, a step with a penalised row at the penalty prefix as before
    (which then carries them along), any other step uploads exactly what it always did."""
    return mb


def _gkey(nb: int, pen: bool, mp: bool = False):
    """Key of a decode graph / split sampler graph variant: (bucket, pen), and (bucket,
    pen, True) for the variant whose sampler reads the ln(min_p) array."""
    return (nb, pen, True) if mp else (nb, pen)


def _pen_views(buf: torch.Tensor, mb: int):
    """(slots int32 [mb], rep, pres, freq f32 [mb]) views of the penalty prefix."""
    f = buf[mb:4 * mb].view(torch.float32)
    return buf[0:mb], f[0:mb], f[mb:2 * mb], f[2 * mb:3 * mb]


def _input_views(buf: torch.Tensor, mb: int, max_blocks: int):
    """(small int32 [6mb], f32 [2mb], seeds int64 [mb], block tables int32 [mb, max_blocks])
    views of one int32 buffer of input_words() elements."""
    return (buf[0:6 * mb], buf[6 * mb:8 * mb].view(torch.float32), buf[8 * mb:10 * mb].view(torch.int64),
            buf[10 * mb:].view(mb, max_blocks))


class _Uploader:
    """Eager (mixed decode + prefill) step inputs in ONE host -> device copy: the
    numpy arrays are packed into a pinned int32 image (64-B aligned fields, int64
    and float32 bit-cast) and come back as typed device views.  Two images
    alternate; an image is refilled only after its previous copy retired (event).
    Replaces ~15 pageable ``torch.from_numpy(a).to(dev)`` copies per step, each a
    blit launch with the GPU idle in front of it."""

    ALIGN = 16  # int32 words

    def __init__(self, device, pin: bool):
        self.device = device
        self.pin = pin
        self.host = [torch.zeros(0, dtype=torch.int32) for _ in range(2)]
        self.events = [None, None]
        self.dev = torch.zeros(0, dtype=torch.int32, device=device)
        self.k = 0

    def __call__(self, arrays):
        arrs = [np.ascontiguousarray(a) for a in arrays]
        offs, n = [], 0
        for a in arrs:
            offs.append(n)
            w = (a.nbytes + 3) // 4
            n += (w + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        n = max(n, self.ALIGN)
        k = self.k
        self.k ^= 1
        if self.events[k] is not None:
            self.events[k].synchronize()
        if self.host[k].numel() < n:
            self.host[k] = torch.zeros(2 * n, dtype=torch.int32, pin_memory=self.pin)
        if self.dev.numel() < n:
            # the old buffer may still feed queued kernels: the caching allocator only
            # reuses its memory after the stream has passed this point
            self.dev = torch.zeros(2 * n, dtype=torch.int32, device=self.device)
        hb = self.host[k].numpy().view(np.uint8)
        for a, o in zip(arrs, offs):
            hb[4 * o:4 * o + a.nbytes] = a.reshape(-1).view(np.uint8)
        self.dev[:n].copy_(self.host[k][:n], non_blocking=True)
        if self.pin:
            ev = self.events[k] or torch.cuda.Event()
            ev.record()
            self.events[k] = ev
        outs = []
        for a, o in zip(arrs, offs):
            w = (a.nbytes + 3) // 4
            v = self.dev[o:o + w]
            if a.dtype.itemsize == 8:
                v = v.view(torch.int64 if a.dtype.kind in "iu" else torch.float64)
            elif a.dtype == np.float32:
                v = v.view(torch.float32)
            elif a.dtype.itemsize != 4:
                raise TypeError(f"upload: unsupported dtype {a.dtype}")
            outs.append(v.view(a.shape) if a.ndim != 1 else v)
        return outs


class _LpHost:
    """Pinned host side of a step's per-token logprobs (SamplingParams.logprobs): the
    rows' ``want`` going up (-1 = the row did not ask) and the kernel's two result
    arrays [rows, 1 + 20] coming back.  ``n``: rows of the step it holds results of (0:
    none -- no row of the step asked)."""
    __slots__ = ("want", "lp", "ids", "n", "pin")

    def __init__(self, rows: int, pin: bool):
        self.pin = pin
        self.n = 0
        self._alloc(rows)

    def _alloc(self, rows: int):
        cols = 1 + ops.LOGPROBS_MAX
        self.want = torch.full((rows,), -1, dtype=torch.int32, pin_memory=self.pin)
        self.lp = torch.zeros(rows, cols, dtype=torch.float32, pin_memory=self.pin)
        self.ids = torch.zeros(rows, cols, dtype=torch.int32, pin_memory=self.pin)

    def stage(self, want: np.ndarray) -> int:
        n = len(want)
        if self.want.shape[0] < n:
            self._alloc(2 * n)
        self.want.numpy()[:n] = want
        self.n = n
        return n

    def take(self) -> Optional[list]:
        """Per row ``(token_id, logprob, [(alt_id, alt_logprob), ...])`` or None (the row
        did not ask); None when the step computed none.  Read after the step's event."""
        n, self.n = self.n, 0
        if not n:
            return None
        want = self.want.numpy()[:n].tolist()
        lp = self.lp.numpy()[:n].tolist()
        ids = self.ids.numpy()[:n].tolist()
        return [None if w < 0 else (ids[r][0], lp[r][0], list(zip(ids[r][1:1 + w], lp[r][1:1 + w])))
                for r, w in enumerate(want)]


class _PlpHost:
    """Pinned host side of a step's prompt logprobs (SamplingParams.prompt_logprobs): the
    three result arrays of ops.prompt_logprobs over the step's extra logits rows, and
    which prompt positions they belong to.  ``chunks``: per contributing prefill chunk
    ``(seq, epoch, first position, count, row offset)``; ``n``: rows held (0: none)."""
    __slots__ = ("lp", "ids", "rank", "want", "chunks", "n", "pin")

    def __init__(self, pin: bool):
        self.pin = pin
        self.n = 0
        self.want: list = []
        self.chunks: list = []
        self._alloc(0)

    def _alloc(self, rows: int):
        cols = 1 + ops.LOGPROBS_MAX
        self.lp = torch.zeros(rows, cols, dtype=torch.float32, pin_memory=self.pin and rows > 0)
        self.ids = torch.zeros(rows, cols, dtype=torch.int32, pin_memory=self.pin and rows > 0)
        self.rank = torch.zeros(rows, dtype=torch.int32, pin_memory=self.pin and rows > 0)

    def stage(self, want: np.ndarray, chunks: list) -> int:
        n = len(want)
        if self.lp.shape[0] < n:
            self._alloc(2 * n)
        self.want, self.chunks, self.n = want.tolist(), chunks, n
        return n

    def take(self) -> Optional[list]:
        """Per chunk ``(seq, epoch, first position, [(token_id, logprob, rank, [(alt_id,
        alt_logprob), ...]), ...])``, or None when the step scored no prompt position.
        Read after the step's event."""
        n, self.n = self.n, 0
        chunks, self.chunks = self.chunks, []
        if not n:
            return None
        lp = self.lp.numpy()[:n].tolist()
        ids = self.ids.numpy()[:n].tolist()
        rank = self.rank.numpy()[:n].tolist()
        out = []
        for seq, epoch, p0, cnt, off in chunks:
            ent = []
            for r in range(off, off + cnt):
                w = self.want[r]
                ent.append((ids[r][0], lp[r][0], rank[r], list(zip(ids[r][1:1 + w], lp[r][1:1 + w]))))
            out.append((seq, epoch, p0, ent))
        return out


class _Staging:
    """Pinned host mirror of the decode graph's device inputs + its output copy.
    int32 ``small`` fields: ids | pos | slots | seq_lens | top_k | steps."""

    def __init__(self, mb: int, max_blocks: int, pin: bool, gpu: bool):
        i32 = torch.int32
        # per-token logprobs: a pinned buffer of its own (not part of h_all, whose layout
        # and upload size stay as they are); lp_want: the staged step's array or None
        self.lp = _LpHost(mb, pin)
        self.lp_want: Optional[np.ndarray] = None
        # one pinned int32 image, laid out like the device inputs (_input_views), so a
        # step's inputs go up in ONE copy: small | f32 | seeds (int64) | block tables
        pw, mw = pen_words(mb), minp_words(mb)
        self.h_all = torch.zeros(pw + mw + input_words(mb, max_blocks), dtype=i32, pin_memory=pin)
        self.h_in = self.h_all[pw + mw:]
        self.h_pen = tuple(v.numpy() for v in _pen_views(self.h_all, mb))
        self.h_pen[0][:] = -1
        self.pen = False   # the staged step has a penalised row
        self.h_minp = self.h_all[pw:pw + mw].view(torch.float32).numpy()   # ln(min_p) per row
        self.h_minp[:] = -np.inf
        self.mp = False    # the staged step has a min_p row
        self.h_small, self.h_f32, self.h_seeds, self.h_bt = _input_views(self.h_in, mb, max_blocks)
        self.h_out = torch.zeros(mb, dtype=i32, pin_memory=pin)
        self.h_err = torch.zeros(1, dtype=i32, pin_memory=pin)  # TP collective error flag
        # pipelined row gather: [source rows | destination rows] (partial gathers)
        self.h_map = torch.zeros(2 * mb, dtype=torch.int64, pin_memory=pin)
        self.err_armed = False
        self.hs = self.h_small.numpy()
        self.hbt = self.h_bt.numpy()
        self.hf = self.h_f32.numpy()
        self.hseed = self.h_seeds.numpy()
        self.event = torch.cuda.Event() if gpu else None


class MixedHandle:
    """A queued mixed step's sampled ids (pinned host copy), completion event and
    ``mark``: an event recorded after MIXED_MARK_FRAC of its layers (the engine
    builds the step queued behind it once the GPU passes it).  They rotate; a
    handle is reused only after MIXED_HANDLES - 1 later mixed launches, more than
    the steps the engine keeps queued (ENGINE_PIPELINE_DEPTH + 1)."""
    __slots__ = ("host", "event", "mark", "n", "pending", "logits", "samp", "seqs", "lp", "plp",
                 "plp_job")

    def __init__(self, rows: int, pin: bool, gpu: bool):
        self.host = torch.zeros(rows, dtype=torch.int32, pin_memory=pin)
        self.lp = _LpHost(rows, pin)   # per-token logprobs of the step it holds
        self.event = torch.cuda.Event() if gpu else None
        self.mark = torch.cuda.Event() if gpu else None
        self.n = 0
        # deferred sampler (guided rows behind a queued step): the logits and the
        # device sampling arrays wait here for sample_launch
        self.pending = False
        self.logits = None
        self.samp = None
        self.seqs = None   # deferred sampler: its rows (their penalty slots are read then)
        # prompt logprobs of the step it holds (_PlpHost, made when a step first needs
        # one); plp_job: what _plp_launch needs, kept until the step's sampler is queued
        self.plp = None
        self.plp_job = None


MIXED_HANDLES = 4


class DecodeHandle:
    """A queued graph-replayed decode step.  ``pending``: only its forward pass is
    queued; its sampler waits for the allow-masks (``ModelRunner.sample_launch``)."""
    __slots__ = ("stage", "n", "nb", "pending", "seqs")

    def __init__(self, stage: "_Staging", n: int, nb: int, pending: bool = False, seqs=None):
        self.stage = stage
        self.n = n
        self.nb = nb
        self.pending = pending
        self.seqs = seqs   # deferred sampler: its rows (their penalty slots are read then)


class ModelRunner:
    def __init__(self, cfg: EngineConfig, model_cfg: ModelConfig, comm: TPComm = SINGLE,
                 device: Optional[str] = None):
        self.cfg = cfg
        self.mcfg = model_cfg
        self.comm = comm
        dev = device or cfg.resolved_device()
        if dev == "cuda":
            dev = f"cuda:{torch.cuda.current_device()}"
        self.device = torch.device(dev)
        self.is_gpu = self.device.type == "cuda"
        self.dtype = cfg.torch_dtype()
        self.bs = cfg.block_size
        self.max_model_len = min(cfg.max_model_len, model_cfg.max_position_embeddings)
        self.max_blocks_per_seq = (self.max_model_len + self.bs - 1) // self.bs

        t0 = time.time()
        self.model = LlamaModel(model_cfg, self.device, self.dtype, comm, self.max_model_len,
                                quantization=cfg.quantization,
                                w4_prefill=getattr(cfg, "w4_prefill", "auto"))
        if cfg.weights and cfg.weights != "random":
            self.model.load_checkpoint(cfg.weights)
        else:
            self.model.init_random(seed=cfg.seed)
        if self.is_gpu:
            torch.cuda.synchronize(self.device)
        # /stats: what the weights occupy, and (W4 engines on the GPU) how their
        # projections run above 64 rows
        self.weights_info = {
            "weights_resident_gb": round(self.model.weights_resident_bytes() / 1e9, 6)}
        w4_mode = self.model.w4_prefill_mode()
        if w4_mode is not None:
            self.weights_info["w4_prefill"] = w4_mode
        if self.model.quant == "fp8":   # only then: every other engine reports what it did
            self.weights_info["quantization"] = "fp8"
        if self.model.quant == "mxfp4":
            self.weights_info["quantization"] = "mxfp4"
        log.info("weights ready in %.1fs: %.3f GB resident%s%s%s", time.time() - t0,
                 self.weights_info["weights_resident_gb"],
                 f", W4 above 64 rows: {w4_mode}" if w4_mode else "",
                 ", quantization fp8 (e4m3 weights, per-channel scales; bench.py still labels "
                 "the dtype bf16)" if self.model.quant == "fp8" else "",
                 ", quantization mxfp4 (e2m1 weights, e8m0 scales per 32 k; bench.py still "
                 "labels the dtype bf16)" if self.model.quant == "mxfp4" else "")

        # batch-invariant numerics (cfg.batch_invariant): rows of a step up to the token
        # budget plus a decode row per sequence
        self.invariant = bool(getattr(cfg, "batch_invariant", False))
        if self.invariant:
            self.model.set_batch_invariant(max(cfg.max_num_batched_tokens, cfg.max_num_seqs)
                                           + cfg.max_num_seqs)
        self.kv_dtype = cfg.kv_torch_dtype(self.dtype)
        # fp8 KV scales (cfg.kv_scales): set on the model now -- after the weights, before
        # the pool exists and before any graph capture; calibration frees its small
        # temporary cache before the pool is sized
        from . import kv_calibrate

        t0 = time.time()
        src = kv_calibrate.resolve(cfg, model_cfg, self.model, self.kv_dtype, self.max_model_len)
        if self.is_gpu and src == "calibrate":
            # return the calibration prefill's temporary cache and activations before the
            # pool is sized from free memory; every other mode allocated nothing, and its
            # pool is sized exactly as it was before scales existed
            torch.cuda.synchronize(self.device)
            torch.cuda.empty_cache()
        self.kv_scale_info = self.model.kv_scale_summary()
        if self.kv_dtype == torch.float8_e4m3fn:
            i = self.kv_scale_info
            log.info("fp8 KV scales: source %s, K %.4g..%.4g, V %.4g..%.4g (%.2fs)", i["source"],
                     i["k_min"], i["k_max"], i["v_min"], i["v_max"], time.time() - t0)
        self.num_blocks = self._decide_num_blocks()
        self.kv = self.model.allocate_kv_cache(self.num_blocks, self.bs, self.kv_dtype)
        # FT_KERNEL_CHECKS=1: the bounds-checked kernel build validates every index it
        # is handed against the tensors of the launch (this pool's blocks, the rotary
        # table's rows, the vocab) and reports into this word, read after each step
        self.d_check: Optional[torch.Tensor] = None
        if self.is_gpu and getattr(ops.native(), "kernel_checks", False):
            self.d_check = torch.zeros(4, dtype=torch.int32, device=self.device)
            ops.native().set_kernel_checks(self.d_check)
            log.warning("FT_KERNEL_CHECKS: bounds-checked kernels (KV pool %d blocks x %d, "
                        "rotary rows %d, vocab %d)", self.num_blocks, self.bs,
                        self.model.cos_sin.shape[0], self.mcfg.vocab_size)
        # penalties: per-slot device state (ops.penalty_state), allocated after the KV pool
        # was sized, out of the reserve _decide_num_blocks keeps back -- the pool is the
        # size it was without them.  Single process only (the engine refuses penalties
        # under tensor parallelism), and nothing at all with cfg.penalties off.
        self.pen_slots = 0
        self.pen_active = False   # the engine has handed out a slot (else steps skip the row scan)
        self.pen_table = self.pen_bias_ids = self.pen_bias_vals = None
        if getattr(cfg, "penalties", True) and comm.world_size == 1:
            self.pen_slots = cfg.max_num_seqs
            self.pen_table, self.pen_bias_ids, self.pen_bias_vals = ops.penalty_state(
                self.pen_slots, model_cfg.vocab_size, self.device)
        # E6 host swap pool (--swap-space): capped at 2x the device pool, allocated
        # (pinned) on the first swap-out so an idle server does not pin host memory
        k0 = self.kv[0][0]
        self.kv_block_elems = k0.numel() // k0.shape[0]
        host_block_bytes = 2 * len(self.kv) * self.kv_block_elems * k0.element_size()
        self.num_host_blocks = min(int(cfg.swap_space_gb * (1 << 30)) // host_block_bytes,
                                   2 * self.num_blocks)
        self.host_kv = None
        self.swap_staging = None
        self.kv_ptrs = None
        nq, d = self.model.nq, self.model.d

        # -------- static decode buffers (graph inputs) --------
        self.graph_sizes = sorted(b for b in cfg.graph_batch_sizes if b <= cfg.max_num_seqs) or [1]
        if self.graph_sizes[-1] < cfg.max_num_seqs:
            self.graph_sizes.append(cfg.max_num_seqs)
        mb = self.graph_sizes[-1]
        self.max_decode_batch = mb
        dv = self.device
        i32 = torch.int32
        pin = self.is_gpu
        # Static graph inputs live in ONE device buffer whose layout mirrors a pinned
        # host staging image, so a decode step refreshes all its inputs with one async
        # H2D copy (each copy is a blit launch, and the GPU idled ~20 us in front of
        # each of the four it used to take: profiles/prof_driver_config_r02b.txt).
        # int32 fields: ids | pos | slots | seq_lens | top_k | steps, then temperature |
        # top_p (f32), seeds (int64), block tables
        # (the penalty prefix in front of them is uploaded only by steps that use it)
        pw, mw = pen_words(mb), minp_words(mb)
        self.d_all = torch.zeros(pw + mw + input_words(mb, self.max_blocks_per_seq), dtype=i32,
                                 device=dv)
        self.d_in = self.d_all[pw + mw:]
        self.d_pen = _pen_views(self.d_all, mb)
        self.d_pen[0].fill_(-1)
        # ln(min_p) per row (-inf = off): read only by the min_p graph variants
        self.d_minp = self.d_all[pw:pw + mw].view(torch.float32)
        self.d_minp.fill_(float("-inf"))
        self.mp_active = False   # the engine holds an unfinished request with min_p > 0
        self.d_small, self.d_f32, self.d_seeds, self.d_bt = _input_views(self.d_in, mb, self.max_blocks_per_seq)
        self.d_input_ids = self.d_small[0:mb]
        self.d_positions = self.d_small[mb:2 * mb]
        self.d_slots = self.d_small[2 * mb:3 * mb]
        self.d_seq_lens = self.d_small[3 * mb:4 * mb]
        self.d_top_k = self.d_small[4 * mb:5 * mb]
        self.d_steps = self.d_small[5 * mb:6 * mb]
        self.d_temp = self.d_f32[0:mb]
        self.d_top_p = self.d_f32[mb:2 * mb]
        self.d_out = torch.zeros(mb, dtype=i32, device=dv)
        self.d_map = torch.zeros(2 * mb, dtype=torch.int64, device=dv)
        # pinned staging sets: while decode step n runs, steps n+1 .. n+depth are
        # filled and queued behind it from the other sets (pipelined decode)
        nstg = max(2, int(getattr(cfg, "pipeline_depth", 1)) + 1)
        self.stg = [_Staging(mb, self.max_blocks_per_seq, pin, self.is_gpu) for _ in range(nstg)]
        self._mx_handles = [MixedHandle(mb, pin, self.is_gpu) for _ in range(MIXED_HANDLES)]
        # ENGINE_MIXED_CHAIN_AT: fraction of a queued mixed step's layers after which
        # its mark event is recorded (0: no mark, the next step is built at once).
        # 0.6: 5,751 / 5,782 / 5,694 vs 5,701-5,711 tok/s at 0.75, same p50 TTFT
        # (profiles/ab_sched_screen_r05.log)
        self.mixed_mark_frac = float(os.environ.get("ENGINE_MIXED_CHAIN_AT", "0.6"))
        self._mx_next = 0
        self._stg_next = 0
        self._upload = _Uploader(dv, pin) if self.is_gpu else None
        self.h_out = torch.zeros(mb, dtype=i32, pin_memory=pin)  # eager-step sampler output
        self.h_err = torch.zeros(1, dtype=i32, pin_memory=pin)
        # per-token logprobs (ops.logprobs, launched eagerly behind the sampler of steps in
        # which some row asked): the device side of a step's want / result arrays -- one
        # set: a step's results are copied out in stream order before the next launch
        # overwrites them -- and the pinned host side of synchronous eager steps
        self.lp_active = False   # the engine holds an unfinished request with logprobs
        self.d_lp_want = torch.full((mb,), -1, dtype=i32, device=dv)
        self.d_lp = torch.zeros(mb, 1 + ops.LOGPROBS_MAX, dtype=torch.float32, device=dv)
        self.d_lp_ids = torch.zeros(mb, 1 + ops.LOGPROBS_MAX, dtype=i32, device=dv)
        self._lp_sync = _LpHost(mb, pin)
        # prompt logprobs (ops.prompt_logprobs over extra logits rows of prefill chunks,
        # _plp_launch): nothing is allocated until a request asks
        self.plp_active = False   # the engine holds an unfinished request that asked
        self.plp_slice_rows = 512   # LM-head rows per slice
        self.plp_tap: Optional[list] = None   # tests: (request id, first position, raw logits)
        self.d_plp = None
        self._plp_sync: Optional[_PlpHost] = None
        self._plp_last: Optional[_PlpHost] = None
        self._lp_last = self._lp_sync   # where the last synchronous step's results are
        # TP rank 0 decides about collective faults; workers only follow its messages
        self.checks_comm = comm.world_size > 1 and comm.rank == 0
        # guided decoding (E19): the token allow-mask is a STATIC input of every
        # decode graph -- all-ones rows for unguided sequences -- so a batch with
        # one tool-calling session stays on the graph path (it only loses the
        # one-step-ahead pipelining: the next mask depends on this step's token)
        self.mask_words = (model_cfg.vocab_size + 31) // 32
        self.d_mask = torch.full((mb, self.mask_words), -1, dtype=i32, device=dv) if self.is_gpu else None
        self.h_mask = torch.full((mb, self.mask_words), -1, dtype=i32, pin_memory=pin) if self.is_gpu else None
        self._mask_rows = 0   # leading rows of d_mask that may hold a non-trivial mask
        self.d_logits_idx = torch.arange(mb, dtype=torch.int64, device=dv)
        # decode-attention partials: one slot per (sequence, kv head) + one per wave
        # of the kernel's grid (any step has at most max_num_seqs decode rows)
        self.max_decode_rows = max(mb, cfg.max_num_seqs)
        n_out, n_ml = ops.decode_workspace(self.max_decode_rows, nq, self.model.nkv, d,
                                           waves=None if self.is_gpu else 0,
                                           piece=ops.DECODE_INV_PIECE if self.invariant else 0,
                                           max_len=self.max_blocks_per_seq * self.bs)
        self.tmp_out = torch.empty(max(1, n_out), dtype=torch.float32, device=dv)
        self.tmp_ml = torch.empty(max(1, n_ml), dtype=torch.float32, device=dv)
        # split-KV prefill partials (ops.build_prefill_tiles): 128 slots = 128 MiB fp32
        # for Llama-3-8B; FT_PREFILL_SPLIT=0 keeps one workgroup per query block
        self.num_cus = torch.cuda.get_device_properties(dv).multi_processor_count if self.is_gpu else 256
        self.pf_part_o = self.pf_part_ml = None
        # batch-invariant plans cut every KV range at fixed pieces and never fall back
        # to an unsplit item: room for every query block of a full step (the budget's
        # 64-token blocks + a partial one per prompt) times the pieces of max_model_len
        self.pf_max_partials = ops.PREFILL_MAX_PARTIALS
        if self.invariant:
            pieces = -(-self.max_model_len // (ops.PREFILL_BK * ops.PREFILL_INV_CHUNK))
            qblocks = -(-cfg.max_num_batched_tokens // ops.prefill_tile_tokens(nq, self.model.nkv))
            self.pf_max_partials = max(ops.PREFILL_MAX_PARTIALS,
                                       (qblocks + cfg.max_num_seqs) * pieces)
        if self.is_gpu and (self.invariant or os.environ.get("FT_PREFILL_SPLIT", "1") == "1"):
            n_po, n_pml = ops.prefill_partials(self.model.nkv, d, self.pf_max_partials)
            self.pf_part_o = torch.empty(n_po, dtype=torch.float32, device=dv)
            self.pf_part_ml = torch.empty(n_pml, dtype=torch.float32, device=dv)
        # in-launch combine tickets (FT_DECODE_FUSED_COMBINE=0: separate combine kernel):
        # with the kernel at one workgroup per CU the last-arriver merge matches or beats
        # the combine kernel and saves a launch per layer (csrc/kernels/attn_decode.hip)
        self.dec_counters = ops.decode_counters(self.max_decode_rows, self.model.nkv, dv) \
            if self.is_gpu and (self.invariant or os.environ.get("FT_DECODE_FUSED_COMBINE", "1") == "1") \
            else None
        self._done_event = torch.cuda.Event() if self.is_gpu else None
        # persistent decode block: its sticky give-up word (ctl[2]) is copied to pinned
        # memory every BLOCK_CHECK_EVERY waits and read at the next check (never a sync)
        self._blk_host = torch.zeros(1, dtype=torch.int32, pin_memory=True) \
            if self.is_gpu and self.model.block else None
        self._blk_event = torch.cuda.Event() if self._blk_host is not None else None
        self._blk_armed = False
        self._blk_waits = 0
        # keyed (batch bucket, pen): pen = the sampler is wrapped in the penalty kernels;
        # (batch bucket, pen, True): the sampler also reads the ln(min_p) array (_gkey)
        self.graphs: Dict[Tuple[int, bool], torch.cuda.CUDAGraph] = {}
        # guided decoding, pipelined: per bucket a forward graph (-> logits) and a
        # sampler graph, so the next step's forward is queued before this step's
        # tokens are known and only its sampler waits for the grammar masks
        self.graphs_split: Dict[Tuple[int, bool], tuple] = {}
        self._fwd_logits: Dict[int, torch.Tensor] = {}
        self._pending_split: Optional["DecodeHandle"] = None   # forward queued, sampler not yet
        # ENGINE_GUIDED_PIPELINE=0: guided batches run one synchronous step at a time
        self.guided_pipeline = os.environ.get("ENGINE_GUIDED_PIPELINE", "1") != "0"
        self.graph_pool = None
        self.use_graphs = self.is_gpu and not cfg.enforce_eager and comm.graph_safe()
        # FT_FAULT_TP_STALL="<n>:<seconds>" (TP workers): before executing the n-th
        # decode graph message, stall until rank 0's custom all-reduce has run out of
        # spin budget (its error word is set; at most <seconds>) -- the fault test
        # of the collective timeout contract
        # "m<n>:<seconds>" stalls before the n-th eager (mixed / prefill) message instead
        stall = os.environ.get("FT_FAULT_TP_STALL", "") if comm.rank > 0 else ""
        self._stall_mixed = stall.startswith("m")
        stall = stall.lstrip("m")
        self._stall_at, self._stall_s = (int(stall.split(":")[0]), float(stall.split(":")[1])) \
            if stall else (None, 0.0)
        self._graph_msgs = 0
        self._mixed_msgs = 0
        # the first eager steps and graph warm-ups of a TP group wait for peers with a
        # long spin budget (every rank counts the same steps: same message order)
        self._warm_left = int(os.environ.get("ENGINE_TP_WARM_STEPS", "4")) \
            if comm.world_size > 1 else 0
        self._trace_tp = os.environ.get("FT_TP_TRACE", "0") == "1" and comm.world_size > 1
        self.stats = {"graph_replays": 0, "eager_decode": 0, "prefill_steps": 0, "captures": 0,
                      "penalty_steps": 0, "logprob_steps": 0, "logprob_rows": 0,
                      "prompt_logprob_steps": 0, "prompt_logprob_rows": 0,
                      "min_p_steps": 0}
        # tests: a list here collects every step's logits (fp32; eager steps on the host,
        # graph-replayed and mixed-ahead steps as stream-ordered device copies) -- TP-vs-TP=1
        # numerics are compared on logits, not on greedy tokens of random weights.  With
        # logits_tap_ids a list too, each entry gets the request ids of its rows.
        self.logits_tap: Optional[list] = None
        self.logits_tap_ids: Optional[list] = None
        self._tap_rows: Optional[list] = None
        self._graph_logits: Dict[Tuple[int, bool], torch.Tensor] = {}   # raw logits of each graph
        # FT_GPU_GAPS=1: timing events around every graph-replayed decode step, so
        # gap_summary() can report how long the GPU sat idle BETWEEN consecutive
        # decode steps (the host enqueued the next one late), without a profiler
        self._gaps = [] if self.is_gpu and os.environ.get("FT_GPU_GAPS", "0") == "1" else None
        self.bcast = None  # TP rank 0: parallel.shm_broadcast.ShmBroadcast writer

    # ------------------------------------------------------------------ memory
    # ------------------------------------------------------------------ host swap (E6)
    SWAP_CHUNK = 32  # blocks per gather/scatter launch (64 MiB of staging for 8B)

    def swap(self, swap_out, swap_in):
        """Copies preempted sequences' KV blocks device -> host (``swap_out``:
        (block, slot) pairs) and resumed ones host -> device (``swap_in``: (slot,
        block) pairs), in stream order before the step that follows."""
        if self.bcast is not None:
            self.bcast.send(("swap", (list(swap_out), list(swap_in)), None))
        self._swap(swap_out, swap_in)

    def _swap(self, swap_out, swap_in):
        nl = 2 * len(self.kv)
        be = self.kv_block_elems
        if self.host_kv is None:
            t0 = time.time()
            self.host_kv = torch.empty(self.num_host_blocks, nl * be, dtype=self.kv_dtype,
                                       pin_memory=self.is_gpu)
            self.swap_staging = torch.empty(self.SWAP_CHUNK, nl * be, dtype=self.kv_dtype,
                                            device=self.device)
            if self.is_gpu:
                self.kv_ptrs = torch.tensor([c.data_ptr() for kv in self.kv for c in kv],
                                            dtype=torch.int64, device=self.device)
            log.info("host KV swap pool: %d blocks (%.2f GiB) in %.2fs", self.num_host_blocks,
                     self.host_kv.numel() * self.host_kv.element_size() / (1 << 30),
                     time.time() - t0)
        for pairs, out in ((swap_out, True), (swap_in, False)):
            for c0 in range(0, len(pairs), self.SWAP_CHUNK):
                chunk = pairs[c0:c0 + self.SWAP_CHUNK]
                dev_blocks = [p[0] if out else p[1] for p in chunk]
                slots = [p[1] if out else p[0] for p in chunk]
                if min(dev_blocks) < 0 or max(dev_blocks) >= self.num_blocks or \
                        min(slots) < 0 or max(slots) >= self.num_host_blocks:
                    raise ValueError("swap block id out of range")
                ids = torch.tensor(dev_blocks, dtype=torch.int32, device=self.device)
                st = self.swap_staging[:len(chunk)]
                if not out:
                    for i, h in enumerate(slots):
                        st[i].copy_(self.host_kv[h], non_blocking=True)
                ops.kv_swap(self.kv, self.kv_ptrs, ids, st, to_staging=out)
                if out:
                    for i, h in enumerate(slots):
                        self.host_kv[h].copy_(st[i], non_blocking=True)
        self.stats["swap_blocks"] = self.stats.get("swap_blocks", 0) + len(swap_out) + len(swap_in)

    def _decide_num_blocks(self) -> int:
        cfg = self.cfg
        per_block = self.mcfg.num_layers * 2 * self.model.nkv * self.model.d * self.bs * \
            torch.tensor([], dtype=self.kv_dtype).element_size()
        if cfg.num_kv_blocks:
            n = cfg.num_kv_blocks
        elif self.is_gpu:
            free, total = torch.cuda.mem_get_info(self.device)
            reserve = 6 << 30  # activations (8k-token prefill), graphs, sampler workspace
            used = total - free
            if os.environ.get("ENGINE_KV_SIZING", "device") == "own":
                # several engines time-share this device (FT_BENCH_SHARED_GPU rehearsals):
                # count only this process's allocations, so the pool does not depend on
                # whether the other engines have sized theirs yet
                used = torch.cuda.memory_reserved(self.device)
            budget = int(total * cfg.gpu_memory_utilization) - used - reserve
            n = max(budget // per_block, 64)
        else:
            n = max(1024, (self.max_model_len // self.bs) * 4)
        n = self.comm.min_int(int(min(n, 4_000_000)))  # every TP rank holds the same pool
        log.info("KV cache: %d blocks x %d tokens = %d tokens (%.1f GiB, %s)", n, self.bs, n * self.bs,
                 n * per_block / 2**30, str(self.kv_dtype).replace("torch.", ""))
        return n

    # ------------------------------------------------------------------ helpers
    def _bucket(self, b: int) -> Optional[int]:
        for s in self.graph_sizes:
            if s >= b:
                return s
        return None

    # ------------------------------------------------------------------ execution
    @torch.inference_mode()
    def execute(self, batch: ScheduledBatch, masks: Optional[np.ndarray] = None) -> List[int]:
        """Runs one step; returns sampled ids for ``batch.sampled_seqs()`` in order.

        Decode-only steps replay a hipGraph; steps that carry prefill chunks run
        eagerly as one mixed forward pass (decode rows first)."""
        self._assert_no_pending_split("execute")
        self._plp_last = None
        if batch.has_prefill:
            if self._gaps is not None:
                self._gap_mark(True, "m")   # closed by _wait, right after the last launch
            return self._mixed(batch, masks)
        if not batch.decode_seqs:
            return []
        return self._decode(batch, masks)

    def _sampling_arrays(self, seqs):
        n = len(seqs)
        temp = np.empty(n, np.float32)
        topp = np.empty(n, np.float32)
        topk = np.empty(n, np.int32)
        seeds = np.empty(n, np.int64)
        steps = np.empty(n, np.int32)
        for i, s in enumerate(seqs):
            p = s.params
            temp[i] = p.temperature
            topp[i] = p.top_p
            topk[i] = p.top_k
            seeds[i] = p.seed
            steps[i] = s.num_output + s.inflight + 131 * s.preemptions
        return temp, topp, topk, seeds, steps

    # ------------------------------------------------------------------ penalties
    # INVARIANT: when a step that samples row r with slot s is launched, table[s] equals
    # the host's truth for that sequence (prompt tokens -> bit 15, output_ids -> counts)
    # plus the tokens sampled by its still-queued steps.  It holds because the slot is
    # seeded from host truth when the engine hands it out (pen_seed, stream-ordered
    # before the step), and every sampling step that carries the slot also runs
    # penalty_update on its sampled ids, in stream order, before the next step's
    # penalty_apply.  A row whose grammar is bound carries slot -1: nothing is applied
    # and nothing is counted (jump-forward tokens and dropped samples exist only then).
    def _pen_arrays(self, seqs):
        """(slot, rep, pres, freq) of a step's sampled rows, or None when no row holds
        a slot (the step then launches none of the penalty kernels)."""
        if self.pen_table is None or not self.pen_active:
            return None
        slot = None
        for i, s in enumerate(seqs):
            k = getattr(s, "pen_slot", -1)
            if k < 0 or (s.grammar is not None and not s.lazy):
                continue
            if slot is None:
                n = len(seqs)
                slot = np.full(n, -1, np.int32)
                rp = np.ones(n, np.float32)
                pr = np.zeros(n, np.float32)
                fr = np.zeros(n, np.float32)
            p = s.params
            slot[i] = k
            rp[i] = p.repetition_penalty
            pr[i] = p.presence_penalty
            fr[i] = p.frequency_penalty
        if slot is None:
            return None
        return slot, rp, pr, fr

    @torch.inference_mode()   # like every launch path: the uploader's buffers are made there
    def pen_seed(self, slot: int, prompt_ids, output_ids, bias: Optional[dict]):
        """Sets slot ``slot`` to a sequence's host truth: prompt tokens get bit 15, output
        tokens their (saturating) counts, ``bias`` (token id -> value) becomes the slot's
        bias list.  Queued in stream order: steps launched afterwards see it."""
        if self.pen_table is None:
            raise RuntimeError("penalties are off (EngineConfig.penalties)")
        vals: Dict[int, int] = {}
        for t in np.unique(np.asarray(prompt_ids, dtype=np.int64)).tolist():
            vals[t] = ops.PEN_PROMPT_BIT
        if len(output_ids):
            toks, cnt = np.unique(np.asarray(output_ids, dtype=np.int64), return_counts=True)
            for t, c in zip(toks.tolist(), cnt.tolist()):
                vals[t] = vals.get(t, 0) | min(int(c), ops.PEN_COUNT_MAX)
        n = len(vals)
        nb = ops.PEN_MAX_BIAS
        img = np.zeros(2 * n + 2 * nb, np.int32)
        img[:n] = list(vals.keys())
        img[n:2 * n] = list(vals.values())
        img[2 * n:2 * n + nb] = -1
        bv = img[2 * n + nb:].view(np.float32)
        for i, (t, b) in enumerate((bias or {}).items()):
            img[2 * n + i] = t
            bv[i] = b
        # pinned, asynchronous (the uploader's images): admissions do not stall the host
        # thread that keeps the decode pipeline fed
        d = self._upload([img])[0] if self.is_gpu else torch.from_numpy(img)
        ops.penalty_seed(self.pen_table, slot, d[:n], d[n:2 * n], self.pen_bias_ids,
                         self.pen_bias_vals, d[2 * n:2 * n + nb],
                         d[2 * n + nb:].view(torch.float32))

    def pen_read(self, slot: int) -> np.ndarray:
        """The table row of ``slot`` as uint16 (synchronises: tests / FT_PENALTY_VERIFY)."""
        if self.is_gpu:
            torch.cuda.synchronize(self.device)
        return self.pen_table[slot].cpu().numpy().view(np.uint16)

    def _minp_array(self, seqs) -> Optional[np.ndarray]:
        """ln(min_p) (fp32, -inf = off) of a step's sampled rows, or None when no row has
        min_p (the step then uploads and launches what it always did)."""
        if not self.mp_active:
            return None
        a = None
        for i, s in enumerate(seqs):
            v = s.params.min_p
            if v > 0.0 and s.params.temperature > 0.0:
                if a is None:
                    a = np.full(len(seqs), -np.inf, np.float32)
                a[i] = ln_min_p(v)
        return a

    def _pen_sample(self, logits, samp, dmask, pen, out=None):
        """The sampler over ``logits`` (raw: they are left untouched), wrapped in the
        penalty kernels when ``pen`` (device slot, rep, pres, freq) is given.  ``samp``:
        the five device sampling arrays, and the step's ln(min_p) array as a sixth when
        one of its rows has min_p."""
        temp, topp, topk, seeds, steps = samp[:5]
        mp = samp[5] if len(samp) > 5 else None
        if mp is not None:
            self.stats["min_p_steps"] += 1
        if pen is None:
            return ops.sample(logits, temp, topp, topk, seeds, steps, out=out, mask=dmask,
                              min_p=mp)
        self.stats["penalty_steps"] += 1
        slot, rp, pr, fr = pen
        pl = ops.penalty_apply(logits, slot, rp, pr, fr, self.pen_table, self.pen_bias_ids,
                               self.pen_bias_vals, out=torch.empty_like(logits))
        out = ops.sample(pl, temp, topp, topk, seeds, steps, out=out, mask=dmask, min_p=mp)
        ops.penalty_update(self.pen_table, slot, out[:logits.shape[0]])
        return out

    # ------------------------------------------------------------------ per-token logprobs
    # A logprob belongs to the step that sampled its token: nothing is kept between
    # steps.  A step in which some row asked launches ops.logprobs eagerly on the
    # step's stream right behind its sampler -- over the RAW logits (never
    # penalty_apply's output) and the sampled ids -- and copies the two result arrays
    # into the step's pinned _LpHost before the step's event is recorded, so the
    # collect finds them complete when the tokens are.  The decode graphs are not
    # touched; a step in which no row asked launches and uploads nothing new.
    def _lp_arrays(self, seqs) -> Optional[np.ndarray]:
        """``want`` (int32 per sampled row: alternatives asked, -1 = none) of a step, or
        None when no row asked."""
        if not self.lp_active:
            return None
        want = None
        for i, s in enumerate(seqs):
            k = s.params.logprobs
            if k is None:
                continue
            if want is None:
                want = np.full(len(seqs), -1, np.int32)
            want[i] = k
        return want

    def _lp_launch(self, hb: "_LpHost", want: np.ndarray, logits, sampled):
        """Queues the logprobs of a step: ``want`` up, the kernel over the raw ``logits``
        rows and their ``sampled`` ids, the results down into ``hb``."""
        n = hb.stage(want)
        if self.d_lp_want.shape[0] < n:   # (eager steps may sample more rows than a graph holds)
            dv, cols = self.device, 1 + ops.LOGPROBS_MAX
            self.d_lp_want = torch.full((2 * n,), -1, dtype=torch.int32, device=dv)
            self.d_lp = torch.zeros(2 * n, cols, dtype=torch.float32, device=dv)
            self.d_lp_ids = torch.zeros(2 * n, cols, dtype=torch.int32, device=dv)
        dw, dl, di = self.d_lp_want[:n], self.d_lp[:n], self.d_lp_ids[:n]
        dw.copy_(hb.want[:n], non_blocking=True)
        ops.logprobs(logits[:n], sampled[:n], dw, dl, di)
        hb.lp[:n].copy_(dl, non_blocking=True)
        hb.ids[:n].copy_(di, non_blocking=True)
        self.stats["logprob_steps"] += 1
        self.stats["logprob_rows"] += int((want >= 0).sum())

    # ------------------------------------------------------------------ prompt logprobs
    # A prefill chunk of a sequence that asked (SamplingParams.prompt_logprobs) names its
    # not yet scored prompt positions as extra logits rows BEHIND the step's sampled rows
    # (_mixed_host): the forward returns their hidden rows with the others, the sampler
    # sees only the sampled ones.  The LM head runs over the extra rows in slices of at
    # most plp_slice_rows (512 rows = 131 MB of bf16 logits at V = 128,256), each followed
    # by ops.prompt_logprobs with the NEXT prompt token as the row's target, on the
    # step's stream behind its sampler (behind the forward where it samples nothing).
    # The results come back into the step's pinned _PlpHost before its event.  A step
    # without such a row builds, uploads and launches exactly what it always did.
    def _plp_rows(self, pseqs, ntoks, starts, qsl, nd: int):
        """(rows, plp) of a step: the extra logits rows and ``{"targets", "want",
        "chunks"}``, or ([], None) when no chunk of it has an unscored position."""
        rows, tgt, want, chunks = [], [], [], []
        for i, (s, n, a) in enumerate(zip(pseqs, ntoks, starts)):
            if s.plp is None:
                continue
            if a is None:
                a = s.num_computed
            lo, hi = max(a, s.plp_next), min(a + n, s.prompt_len - 1)
            if hi <= lo:
                continue
            chunks.append((s, s.epoch, lo, hi - lo, len(rows)))
            base = nd + int(qsl[i]) - a
            rows += list(range(base + lo, base + hi))
            tgt.append(s.tokens[lo + 1:hi + 1])
            want += [s.params.prompt_logprobs] * (hi - lo)
        if not rows:
            return [], None
        return rows, {"targets": np.concatenate(tgt).astype(np.int32),
                      "want": np.asarray(want, np.int32), "chunks": chunks}

    @staticmethod
    def _plp_split(h, host, d_lrows):
        """(sampled rows, extra rows) of the forward's hidden rows ``h``.  The forward
        returns ALL rows in their natural order when as many rows are named as the step
        has tokens (it takes that for "every row"): with extra rows the names are then a
        permutation of the rows, which is applied here."""
        n = len(host["lrows"])
        if n == len(host["ids"]):
            h = h.index_select(0, d_lrows)
        ns = n - len(host["plp"]["want"])   # the sampled rows come first
        return h[:ns], h[ns:]

    def _plp_launch(self, hb: "_PlpHost", hidden, plp, d_tgt, d_want):
        """Queues a step's prompt logprobs: the LM head over ``hidden`` (the extra rows)
        slice by slice, ops.prompt_logprobs behind each, the results down into ``hb``."""
        n = hb.stage(plp["want"], plp["chunks"])
        if self.d_plp is None or self.d_plp[0].shape[0] < n:
            dv, cols = self.device, 1 + ops.LOGPROBS_MAX
            self.d_plp = (torch.zeros(2 * n, cols, dtype=torch.float32, device=dv),
                          torch.zeros(2 * n, cols, dtype=torch.int32, device=dv),
                          torch.zeros(2 * n, dtype=torch.int32, device=dv))
        dl, di, dr = (t[:n] for t in self.d_plp)
        step = max(1, int(self.plp_slice_rows))
        taps = [] if self.plp_tap is not None else None
        for o in range(0, n, step):
            m = min(step, n - o)
            logits = self.model.compute_logits(hidden[o:o + m])
            if taps is not None:
                taps.append(logits.float().cpu())
            ops.prompt_logprobs(logits, d_tgt[o:o + m], d_want[o:o + m], dl[o:o + m], di[o:o + m],
                                dr[o:o + m])
        hb.lp[:n].copy_(dl, non_blocking=True)
        hb.ids[:n].copy_(di, non_blocking=True)
        hb.rank[:n].copy_(dr, non_blocking=True)
        if taps is not None:
            raw = torch.cat(taps)
            for seq, _, p0, cnt, off in plp["chunks"]:
                self.plp_tap.append((seq.request_id, p0, raw[off:off + cnt]))
        self.stats["prompt_logprob_steps"] += 1
        self.stats["prompt_logprob_rows"] += n

    def take_prompt_logprobs(self, h=None) -> Optional[list]:
        """The prompt-logprob chunks of a collected step (``h``: its handle; None: the
        synchronous step ``execute`` just ran), or None when it scored no position."""
        hb = self._plp_last if h is None else getattr(h, "plp", None)
        return hb.take() if hb is not None else None

    def take_logprobs(self, h=None) -> Optional[list]:
        """The per-row logprob entries of a collected step (``h``: its handle; None: the
        synchronous step ``execute`` just ran), or None when no row of it asked."""
        hb = self._lp_last if h is None else (h.stage.lp if isinstance(h, DecodeHandle) else h.lp)
        return hb.take()

    def _mixed(self, batch: ScheduledBatch, masks) -> List[int]:
        host = self._mixed_host(batch)
        if self.bcast is not None:
            self.bcast.send(("mixed", host, masks))
        return self._mixed_run(host, masks)

    def _mixed_host(self, batch: ScheduledBatch) -> Dict[str, object]:
        """Host-side (numpy) inputs of an eager mixed decode+prefill step; this is
        also the message tensor-parallel workers receive."""
        dseqs = batch.decode_seqs
        pseqs = [s for s, n in zip(batch.prefill_seqs, batch.prefill_tokens) if n > 0]
        ntoks = [n for n in batch.prefill_tokens if n > 0]
        # chunk starts as scheduled (a chunk queued behind an in-flight chunk of the
        # same prompt starts after it; num_computed only moves in post_step)
        starts = [a for a, n in zip(batch.prefill_start or [None] * len(batch.prefill_seqs),
                                    batch.prefill_tokens) if n > 0]
        psamp = [sm for sm, n in zip(batch.prefill_sample, batch.prefill_tokens) if n > 0]
        bs = self.bs
        nd = len(dseqs)
        ids, pos, slots = [], [], []
        host: Dict[str, object] = {"nd": nd}
        # decode rows
        if nd:
            d_ids = np.empty(nd, np.int32)
            d_pos = np.empty(nd, np.int32)
            d_slot = np.empty(nd, np.int32)
            d_bt = np.zeros((nd, max(len(s.block_ids) for s in dseqs)), np.int32)
            for i, s in enumerate(dseqs):
                p = s.n_tokens - 1 + s.inflight   # queued ahead: ids come from the device
                d_ids[i] = s.last_token
                d_pos[i] = p
                d_slot[i] = s.block_ids[p // bs] * bs + p % bs
                d_bt[i, : len(s.block_ids)] = s.block_ids
            ids.append(d_ids)
            pos.append(d_pos)
            slots.append(d_slot)
            host["d_bt"] = d_bt
            host["d_sl"] = d_pos + 1
        # prefill rows
        seq_lens = np.empty(len(pseqs), np.int32)
        qsl = np.zeros(len(pseqs) + 1, np.int32)
        maxb = max([len(s.block_ids) for s in pseqs] or [1])
        bt = np.zeros((max(1, len(pseqs)), maxb), np.int32)
        for i, (s, n, a) in enumerate(zip(pseqs, ntoks, starts)):
            if a is None:
                a = s.num_computed
            ids.append(s.tokens[a:a + n])
            p = np.arange(a, a + n, dtype=np.int32)
            pos.append(p)
            blk = np.asarray(s.block_ids, dtype=np.int32)
            bt[i, : len(blk)] = blk
            slots.append(blk[p // bs] * bs + p % bs)
            seq_lens[i] = a + n
            qsl[i + 1] = qsl[i] + n
        tiles, combine = ops.build_prefill_tiles(
            ntoks, ops.prefill_tile_tokens(self.model.nq, self.model.nkv),
            seq_lens=seq_lens if self.pf_part_o is not None else None, nkv=self.model.nkv,
            num_cus=self.num_cus, max_partials=self.pf_max_partials,
            fixed_chunk=ops.PREFILL_INV_CHUNK if self.invariant else 0)
        # logits rows: every decode row + the last row of each prompt that completes
        lrows = list(range(nd)) + [nd + int(qsl[i + 1]) - 1 for i, sm in enumerate(psamp) if sm]
        host["plp"] = None
        if self.plp_active:   # prompt-logprob rows go behind the sampled rows
            xrows, host["plp"] = self._plp_rows(pseqs, ntoks, starts, qsl, nd)
            lrows += xrows
        host.update(ids=np.concatenate(ids).astype(np.int32), pos=np.concatenate(pos).astype(np.int32),
                    slots=np.concatenate(slots).astype(np.int32), lrows=np.asarray(lrows, np.int64),
                    bt=bt, seq_lens=seq_lens, qsl=qsl, tiles=np.asarray(tiles, np.int32).reshape(-1),
                    num_tiles=len(tiles), combine=np.asarray(combine, np.int32).reshape(-1),
                    num_combine=len(combine),
                    num_partials=sum(c[3] for c in combine))
        sseqs = dseqs + [s for s, sm in zip(pseqs, psamp) if sm]
        host["sampling"] = self._sampling_arrays(sseqs)
        host["pen"] = self._pen_arrays(sseqs)
        host["lp"] = self._lp_arrays(sseqs)
        host["minp"] = self._minp_array(sseqs)
        if self.logits_tap_ids is not None:
            self._tap_rows = [s.request_id for s in sseqs]
        return host

    def _long_waits(self):
        """Context: the custom collectives' first-steps spin budget while warm steps last."""
        if self._warm_left <= 0 or self.comm.custom is None:
            return contextlib.nullcontext()
        self._warm_left -= 1
        return self.comm.custom.long_waits()

    def _mixed_run(self, host: Dict[str, object], masks) -> List[int]:
        t0 = time.perf_counter() if self._trace_tp else 0.0
        with self._long_waits():
            out = self._mixed_run_inner(host, masks)
        if self._trace_tp:
            log.warning("TP trace rank %d: mixed step %d rows in %.1f ms", self.comm.rank,
                        len(host["ids"]), 1e3 * (time.perf_counter() - t0))
        return out

    def _mixed_run_inner(self, host: Dict[str, object], masks) -> List[int]:
        self.stats["prefill_steps"] += 1
        nd = host["nd"]
        qsl = host["qsl"]
        names = ["pos", "slots", "lrows", "bt", "seq_lens", "qsl", "tiles", "ids", "combine"]
        if nd:
            if nd > self.max_decode_rows:
                raise ValueError(f"{nd} decode rows exceed max_num_seqs {self.max_decode_rows}")
            names += ["d_bt", "d_sl"]
        plp = host.get("plp")
        if plp is not None:
            names += ["plp_t", "plp_w"]
            host["plp_t"], host["plp_w"] = plp["targets"], plp["want"]
        arrays = [host[k] for k in names]
        ns = len(host["lrows"]) - (len(plp["want"]) if plp is not None else 0)   # sampled rows
        has_logits = ns > 0
        self._plp_last = None
        pen = host.get("pen") if has_logits else None
        minp = host.get("minp") if has_logits else None
        if has_logits:
            arrays += list(host["sampling"])
            if masks is not None:
                arrays.append(masks)
            if minp is not None:   # same upload as the other sampling arrays
                arrays.append(minp)
            if pen is not None:
                arrays += list(pen)
        if self.is_gpu:
            dev = self._upload(arrays)
        else:
            dev = [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]
        d = dict(zip(names, dev))
        meta = AttnMeta(
            positions=d["pos"], slot_mapping=d["slots"], logits_indices=d["lrows"], num_decode=nd,
            block_tables=d["bt"], seq_lens=d["seq_lens"],
            q_start_loc=d["qsl"] if self.is_gpu else torch.from_numpy(qsl),
            tile_info=d["tiles"], num_tiles=host["num_tiles"])
        if host.get("num_combine", 0):
            meta.pf_part_o, meta.pf_part_ml = self.pf_part_o, self.pf_part_ml
            meta.pf_combine, meta.pf_num_combine = d["combine"], host["num_combine"]
            meta.pf_num_partials = host["num_partials"]
        if nd:
            meta.dec_block_tables = d["d_bt"]
            meta.dec_seq_lens = d["d_sl"]
            meta.tmp_out, meta.tmp_ml = self.tmp_out, self.tmp_ml
            meta.dec_counters = self.dec_counters
        h = self.model.forward(d["ids"], meta, self.kv)
        job = None
        if plp is not None:
            if self._plp_sync is None:
                self._plp_sync = _PlpHost(self.is_gpu)
            h, hx = self._plp_split(h, host, d["lrows"])
            job = (self._plp_sync, hx, plp, d["plp_t"], d["plp_w"])
            self._plp_last = self._plp_sync
        if not has_logits:
            if job is not None:   # a chunk that samples nothing still scores its positions
                self._plp_launch(*job)
            # a middle chunk of a chunked prefill samples nothing, but its all-reduces
            # wrote KV blocks that post_step commits to the prefix cache: check the
            # custom collectives' error word before anything is committed
            flag = self._arm_comm_check() if self.is_gpu else None
            if flag is not None:
                self.h_err.copy_(flag, non_blocking=True)
                self._wait()
                if int(self.h_err[0]):
                    self._comm_fault()
            elif job is not None and self.is_gpu:
                self._wait()
            return []
        k = len(names)
        samp = list(dev[k:k + 5])
        dmask = dev[k + 5] if masks is not None else None
        if minp is not None:
            samp.append(dev[k + 5 + (masks is not None)])
        dpen = dev[-4:] if pen is not None else None
        return self._sample(h, host["sampling"], masks, dev_sampling=samp, dev_mask=dmask,
                            dev_pen=dpen, lp_want=host.get("lp"), plp_job=job)

    def _wait(self, ev=None):
        """Block until the GPU work queued so far (or up to ``ev``) is done WITHOUT
        holding the GIL: a plain ``.cpu()`` / ``synchronize`` keeps the GIL for the
        whole step and starves the asyncio thread that streams to the WebSockets."""
        if ev is None:
            if self._gaps and self._gaps[-1][1] is None:
                self._gap_mark(False)
            ev = self._done_event
            ev.record()
        t0 = time.perf_counter()
        while not ev.query():
            time.sleep(0.0001)
        self.stats["wait_ms"] = self.stats.get("wait_ms", 0.0) + 1e3 * (time.perf_counter() - t0)
        if self.d_check is not None:
            self.kernel_check()
        if self._blk_host is not None:
            self._block_check()

    BLOCK_CHECK_EVERY = 64

    def _block_check(self):
        """Decode block give-up word: a grid barrier that timed out (a grid that was
        not fully resident) leaves garbage rows; the step fails loudly and the model
        falls back to the unfused layer (graphs recaptured on demand)."""
        self._blk_waits += 1
        if self._blk_armed and self._blk_event.query():
            self._blk_armed = False
            if int(self._blk_host[0]) and self.model.block_fault():
                self._blk_host = None
                self.graphs.clear()
                self._graph_logits.clear()
                self.graphs_split.clear()
                self._fwd_logits.clear()
                self._pending_split = None
                raise DecodeBlockFault("decode block grid barrier timed out; step discarded, "
                                       "unfused decode layer from now on")
        if not self._blk_armed and self._blk_waits % self.BLOCK_CHECK_EVERY == 0:
            self._blk_host.copy_(self.model.db_ctl[2:3], non_blocking=True)
            self._blk_event.record()
            self._blk_armed = True

    def kernel_check(self):
        """Checked build: raise KernelCheckError if a kernel has reported an out-of-range
        index since the last reset (the word is sticky until kernel_check_reset)."""
        if self.d_check is None:
            return
        w = self.d_check.cpu()
        if int(w[0]):
            # clear the sticky word as the error is raised: the serving loop fails the
            # affected requests and carries on, and later steps must not re-raise it
            self.d_check.zero_()
            raise KernelCheckError(w.tolist())

    def kernel_check_reset(self):
        if self.d_check is not None:
            self.d_check.zero_()

    def _sample(self, h, sampling, masks, dev_sampling=None, dev_mask=None, dev_pen=None,
                lp_want=None, plp_job=None) -> List[int]:
        logits = self.model.compute_logits(h)
        self._lp_sync.n = 0
        self._lp_last = self._lp_sync
        if self.logits_tap is not None:
            self._tap(logits.float().cpu())
        if dev_sampling is None:
            arrays = list(sampling) + ([masks] if masks is not None else [])
            if self.is_gpu:
                dev = self._upload(arrays)
            else:
                dev = [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]
            dev_sampling = dev[:5]
            dev_mask = dev[5] if masks is not None else None
        out = self._pen_sample(logits, dev_sampling, dev_mask, dev_pen)
        if lp_want is not None:
            self._lp_launch(self._lp_sync, lp_want, logits, out)
        if plp_job is not None:
            self._plp_launch(*plp_job)
        if not self.is_gpu:
            return out.tolist()
        n = out.shape[0]
        flag = self._arm_comm_check()
        if flag is not None:
            self.h_err.copy_(flag, non_blocking=True)
        if n <= self.h_out.shape[0]:
            self.h_out[:n].copy_(out, non_blocking=True)
            self._wait()
            host = self.h_out[:n]
        else:
            host = torch.empty(n, dtype=out.dtype, pin_memory=True)
            host.copy_(out, non_blocking=True)
            self._wait()
        if flag is not None and int(self.h_err[0]):
            self._comm_fault()
        return host.tolist()

    def _tap(self, logits: torch.Tensor):
        self.logits_tap.append(logits)
        if self.logits_tap_ids is not None:
            self.logits_tap_ids.append(self._tap_rows)
            self._tap_rows = None

    # ------------------------------------------------------------------ TP fault contract
    def _arm_comm_check(self) -> Optional[torch.Tensor]:
        """Queues the fold of every rank's collective error word into the device
        flag (eager steps; decode graphs carry it) and returns the flag, or None
        when this rank does not check (single GPU, workers, RCCL only)."""
        flag = self.comm.error_flag
        if flag is None or not self.checks_comm:
            return None
        self.comm.export_error()
        return flag

    def _comm_fault(self):
        """Rank 0 saw a timed-out custom collective: every rank drops to RCCL (in
        message order, so the collectives stay matched) and the step fails."""
        if self.bcast is not None:
            self.bcast.send(("comm_fault", None, None))
        self._drop_custom_collectives()
        raise CommFault("tensor-parallel all-reduce timed out waiting for a peer; "
                        "step discarded, group switched to RCCL")

    def _drop_custom_collectives(self):
        if self.is_gpu:
            torch.cuda.synchronize(self.device)  # no graph of the old kind still running
        self.comm.disable_custom("custom collective timed out")
        self.graphs.clear()  # they captured the custom kernels; recaptured on demand
        self._graph_logits.clear()
        self.graphs_split.clear()
        self._fwd_logits.clear()
        self._pending_split = None   # the in-flight step is discarded with its graphs
        if not self.comm.graph_safe():
            self.use_graphs = False
        for st in self.stg:
            st.err_armed = False
            st.h_err.zero_()

    def _decode(self, batch: ScheduledBatch, masks) -> List[int]:
        seqs = batch.decode_seqs
        n = len(seqs)
        bucket = self._bucket(n) if self.use_graphs else None
        if bucket is None:
            return self._decode_eager(seqs, masks)
        h = self.decode_launch(seqs, masks=masks)
        self._lp_last = h.stage.lp
        return self.decode_collect(h)

    def can_pipeline(self, n: int) -> bool:
        return self.use_graphs and self._bucket(n) is not None

    def can_defer_sample(self) -> bool:
        """Can a decode step be queued with its sampler deferred until its allow-masks
        are known (pipelined guided decoding)?  Single process only (TP workers replay
        whole steps from the broadcast)."""
        return self.use_graphs and self.guided_pipeline and self.bcast is None \
            and not self.checks_comm and self.d_mask is not None

    def decode_launch(self, seqs, ahead: int = 0, masks: Optional[np.ndarray] = None,
                      rowmap: Optional[List[int]] = None, defer_sample: bool = False
                      ) -> DecodeHandle:
        """Fills a staging set and queues a graph-replayed decode step (returns at
        once).  Positions are ``inflight`` tokens past each sequence's collected
        state (steps queued ahead of it); with ``ahead`` the input ids are the last
        queued step's sampled ids, copied device-to-device, so the host never waits
        between steps.  ``rowmap[i]`` (with ``ahead``): the row of that step that
        sequence i sat in (None: the same row).  ``defer_sample``: queue the forward
        pass only; ``sample_launch`` queues its sampler once the masks are known."""
        n = len(seqs)
        nb = self._bucket(n)
        st = self.stg[self._stg_next]
        self._stg_next = (self._stg_next + 1) % len(self.stg)
        maxblk = self._decode_fill(seqs, nb, st)
        # penalty arrays: into the staging prefix now, or (a deferred sampler) when the
        # sampler is queued -- whether a lazy grammar bound is known only then
        pa = None if defer_sample else self._pen_arrays(seqs)
        st.pen = pa is not None
        if pa is not None:
            self._pen_stage(st, pa, n, nb)
        # logprobs: launched behind the sampler, wherever that is queued (a deferred
        # sampler reads its rows again in sample_launch)
        st.lp.n = 0
        st.lp_want = None if defer_sample else self._lp_arrays(seqs)
        gather = None
        if ahead and rowmap is not None:
            gather = np.zeros(nb, dtype=np.int64)   # padding rows read row 0 (ignored)
            gather[:n] = rowmap   # -1: no queued step has the row, its id comes from the host
        self._assert_no_pending_split("decode_launch")
        if defer_sample:
            assert self.can_defer_sample()
            self._decode_enqueue(st, nb, n, from_device=bool(ahead), gather=gather, fwd_only=True)
            h = DecodeHandle(st, n, nb, pending=True, seqs=list(seqs))
            self._pending_split = h
            return h
        if self.bcast is not None:
            self.bcast.send(("graph", {"nb": nb, "n": n, "small": st.hs.copy(),
                                       "bt": st.hbt[:nb, :maxblk].copy(), "f32": st.hf.copy(),
                                       "seeds": st.hseed.copy(), "from_device": bool(ahead),
                                       "rowmap": gather}, masks))
        self._set_masks(masks, n)
        pen = st.pen
        self._decode_enqueue(st, nb, n, from_device=bool(ahead), gather=gather, pen=pen, mp=st.mp)
        gk = _gkey(nb, pen, st.mp)
        if self.logits_tap is not None and gk in self._graph_logits:
            # copied in stream order: the next queued replay overwrites the graph's logits
            if self.logits_tap_ids is not None:
                self._tap_rows = [s.request_id for s in seqs]
            self._tap(self._graph_logits[gk][:n].float().clone())
        return DecodeHandle(st, n, nb)

    @torch.inference_mode()
    def sample_launch(self, h, masks: Optional[np.ndarray]):
        """Queues the sampler of a step whose forward pass ``decode_launch(...,
        defer_sample=True)`` queued: its allow-masks go up, the sampler graph reads
        the forward graph's logits, the ids land in ``d_out`` (the next step's
        inputs) and in the staging set's pinned copy.  A mixed step's
        (``mixed_launch(..., defer_sample=True)``) eager sampler reads its held logits."""
        if isinstance(h, MixedHandle):
            assert h.pending
            pen = self._pen_arrays(h.seqs) if h.seqs is not None else None
            # (a min_p array went up with the step's sampling arrays: it is in h.samp)
            arrays = ([masks] if masks is not None else []) + list(pen or ())
            dev = []
            if arrays:
                dev = self._upload(arrays) if self.is_gpu else \
                    [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]
            dmask = dev[0] if masks is not None else None
            self._mixed_sample(h, h.logits, h.samp, dmask, dev[-4:] if pen is not None else None,
                               self._lp_arrays(h.seqs) if h.seqs is not None else None)
            return
        assert h.pending and self._pending_split is h
        self._set_masks(masks, h.n)
        st = h.stage
        # the rows' penalty slots as they stand now (a lazy grammar that bound meanwhile
        # has given its slot back): staged and uploaded with this sampler, not the forward
        pen = self._pen_arrays(h.seqs) if h.seqs is not None else None
        pw = pen_words(self.max_decode_batch)
        mw = minp_words(self.max_decode_batch) if st.mp else 0   # staged by _decode_fill
        if pen is not None:
            self._pen_stage(st, pen, h.n, h.nb)
            self.d_all[:pw + mw].copy_(st.h_all[:pw + mw], non_blocking=True)
            self.stats["penalty_steps"] += 1
        elif mw:
            self.d_all[pw:pw + mw].copy_(st.h_all[pw:pw + mw], non_blocking=True)
        if mw:
            self.stats["min_p_steps"] += 1
        key = _gkey(h.nb, pen is not None, st.mp)
        pair = self.graphs_split.get(key) or self._capture_split(h.nb, pen is not None, st.mp)
        pair[1].replay()
        self._pending_split = None
        want = self._lp_arrays(h.seqs) if h.seqs is not None else None
        if want is not None:   # before anything else can replay over the forward's logits
            self._lp_launch(st.lp, want, self._fwd_logits[h.nb], self.d_out)
        if self.logits_tap is not None and h.seqs is not None:
            if self.logits_tap_ids is not None:
                self._tap_rows = [s.request_id for s in h.seqs]
            self._tap(self._fwd_logits[h.nb][:h.n].float().clone())
        st.h_out[:h.n].copy_(self.d_out[:h.n], non_blocking=True)
        st.err_armed = False
        st.event.record()
        h.pending = False
        if self._gaps is not None:
            self._gap_mark(False)

    def discard_pending(self):
        """Forget a deferred-sample step whose sampler will never be queued (the
        engine dropped its in-flight steps after a failure)."""
        self._pending_split = None

    def _assert_no_pending_split(self, where: str):
        """A split step's logits (``_fwd_logits``) live in the graph pool every graph
        shares: nothing may be replayed or run between its forward and its sampler, or
        that work can overwrite them before they are sampled."""
        if self._pending_split is not None:
            raise RuntimeError(f"{where}: a deferred-sample decode step is pending; "
                               "sample_launch() must be queued first")

    def _set_masks(self, masks: Optional[np.ndarray], n: int):
        """Uploads the step's allow-masks into the graph's static mask rows (stream
        ordered before the replay); resets rows a previous guided step dirtied."""
        if self.d_mask is None:
            return
        if masks is None:
            if self._mask_rows:
                self.d_mask[:self._mask_rows].fill_(-1)
                self._mask_rows = 0
            return
        rows = max(n, self._mask_rows)
        hm = self.h_mask.numpy()
        hm[:n, : masks.shape[1]] = masks[:n]
        hm[n:rows] = -1
        self.d_mask[:rows].copy_(self.h_mask[:rows], non_blocking=True)
        self._mask_rows = n

    def decode_collect(self, h: DecodeHandle) -> List[int]:
        st = h.stage
        self._wait(st.event)
        if st.err_armed and int(st.h_err[0]):
            self._comm_fault()
        return st.h_out[:h.n].tolist()

    def step_done(self, h) -> bool:
        """Non-blocking: has the queued step behind handle ``h`` finished on the GPU?"""
        ev = h.stage.event if isinstance(h, DecodeHandle) else h.event
        return ev is None or ev.query()

    @torch.inference_mode()
    def mixed_launch(self, batch: ScheduledBatch, rowmap: Optional[List[int]],
                     masks: Optional[np.ndarray] = None, defer_sample: bool = False) -> "MixedHandle":
        """Queues a mixed (decode + prefill) step behind the queued step(s) without
        waiting (engine ``_speculate_mixed``): decode row i's input id is row
        ``rowmap[i]`` of the last queued step's sampled ids (``d_out``), gathered on
        the device; its position is ``inflight`` tokens ahead.  ``rowmap`` None:
        nothing is queued, the ids are the sequences' last tokens (host).  The
        sampled ids land in ``d_out`` (rows = ``batch.sampled_seqs()``) for the
        decode step queued next, and in a pinned host buffer for the collect.
        ``masks``: the sampled rows' allow-masks when they are known at launch;
        ``defer_sample``: they are not (guided rows whose grammar waits for the step
        queued ahead) -- the forward pass is queued now, the sampler by
        :meth:`sample_launch` once the engine has the masks.  Single process only
        (no TP broadcast)."""
        self._assert_no_pending_split("mixed_launch")
        if self._gaps is not None:
            self._gap_mark(True, "a")
        tp0 = time.perf_counter()
        host = self._mixed_host(batch)
        tp1 = time.perf_counter()
        nd = host["nd"]
        self.stats["prefill_steps"] += 1
        self.stats["mixed_ahead"] = self.stats.get("mixed_ahead", 0) + 1
        names = ["pos", "slots", "lrows", "bt", "seq_lens", "qsl", "tiles", "ids", "combine"]
        if nd:
            names += ["d_bt", "d_sl"]
        plp = host["plp"]
        if plp is not None:
            names += ["plp_t", "plp_w"]
            host["plp_t"], host["plp_w"] = plp["targets"], plp["want"]
        arrays = [host[k] for k in names] + list(host["sampling"])
        minp = host["minp"]
        # rowmap[i] < 0: row i's sequence has no queued step (it joined after the last
        # queued step was built); its id is its last token, already in host["ids"]
        rm = np.asarray(rowmap if rowmap is not None else [], dtype=np.int64)
        dst = np.nonzero(rm >= 0)[0].astype(np.int64)
        partial = nd and rowmap is not None and len(dst) < nd
        arrays.append(rm[dst] if nd and len(dst) else np.zeros(1, np.int64))
        arrays.append(dst if partial and len(dst) else np.zeros(1, np.int64))
        if masks is not None and not defer_sample:
            arrays.append(masks)
        if minp is not None:   # does not depend on the masks: also with a deferred sampler
            arrays.append(minp)
        # a deferred sampler reads its rows' penalty slots when it is queued (sample_launch):
        # whether a lazy grammar bound is known only then
        pen = None if defer_sample else host["pen"]
        if pen is not None:
            arrays += list(pen)
        if self.is_gpu:
            dev = self._upload(arrays)
        else:
            dev = [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]
        d = dict(zip(names, dev))
        tp2 = time.perf_counter()
        if nd and len(dst):
            src_t, dst_t = dev[len(names) + 5], dev[len(names) + 6]
            if partial:
                d["ids"].index_copy_(0, dst_t, self.d_out.index_select(0, src_t))
            else:
                torch.index_select(self.d_out, 0, src_t, out=d["ids"][:nd])
        tp3 = time.perf_counter()
        meta = AttnMeta(
            positions=d["pos"], slot_mapping=d["slots"], logits_indices=d["lrows"], num_decode=nd,
            block_tables=d["bt"], seq_lens=d["seq_lens"],
            q_start_loc=d["qsl"] if self.is_gpu else torch.from_numpy(host["qsl"]),
            tile_info=d["tiles"], num_tiles=host["num_tiles"])
        if host.get("num_combine", 0):
            meta.pf_part_o, meta.pf_part_ml = self.pf_part_o, self.pf_part_ml
            meta.pf_combine, meta.pf_num_combine = d["combine"], host["num_combine"]
            meta.pf_num_partials = host["num_partials"]
        if nd:
            meta.dec_block_tables = d["d_bt"]
            meta.dec_seq_lens = d["d_sl"]
            meta.tmp_out, meta.tmp_ml = self.tmp_out, self.tmp_ml
            meta.dec_counters = self.dec_counters
        mh = self._mx_handles[self._mx_next]
        self._mx_next = (self._mx_next + 1) % len(self._mx_handles)
        mh.plp_job = None   # (left by a deferred step whose sampler was never queued)
        nl = len(getattr(self.model, "layers", ()))
        if mh.mark is not None and nl and self.mixed_mark_frac > 0:
            self.model.mark_at = (min(nl - 1, int(self.mixed_mark_frac * nl)), mh.mark)
        try:
            h = self.model.forward(d["ids"], meta, self.kv)
        finally:
            self.model.mark_at = None
        if plp is not None:
            h, hx = self._plp_split(h, host, d["lrows"])
            if mh.plp is None:
                mh.plp = _PlpHost(self.is_gpu)
            dt, dw = d["plp_t"], d["plp_w"]
            if defer_sample:   # (views of the upload buffer, as the sampling arrays below)
                dt, dw = dt.clone(), dw.clone()
            mh.plp_job = (mh.plp, hx, plp, dt, dw)
        logits = self.model.compute_logits(h)
        if self.logits_tap is not None:
            self._tap(logits.float().cpu())   # taps are host tensors (tests)
        n = logits.shape[0]
        samp = list(dev[len(names):len(names) + 5])
        if minp is not None:
            samp.append(dev[len(names) + 7 + (masks is not None and not defer_sample)])
        if mh.host.shape[0] < n:
            mh.host = torch.zeros(2 * n, dtype=torch.int32, pin_memory=self.is_gpu)
        mh.n = n
        if defer_sample:
            # the sampling arrays are views into the shared upload buffer, which the
            # masks' upload (sample_launch) overwrites first: keep copies
            mh.pending, mh.logits, mh.samp = True, logits, [t.clone() for t in samp]
            mh.seqs = batch.sampled_seqs()
            self.stats["deferred_mixed"] = self.stats.get("deferred_mixed", 0) + 1
        else:
            dmask = dev[len(names) + 7] if masks is not None else None
            self._mixed_sample(mh, logits, samp, dmask, dev[-4:] if pen is not None else None,
                               host["lp"])
        if self._gaps is not None:
            self._gap_mark(False)
        tp4 = time.perf_counter()
        ml = self.stats.setdefault("mixed_launch_ms", {"host": 0.0, "upload": 0.0, "gather": 0.0,
                                                        "forward": 0.0, "n": 0})
        ml["host"] += 1e3 * (tp1 - tp0)
        ml["upload"] += 1e3 * (tp2 - tp1)
        ml["gather"] += 1e3 * (tp3 - tp2)
        ml["forward"] += 1e3 * (tp4 - tp3)
        ml["n"] += 1
        return mh

    def _mixed_sample(self, mh: "MixedHandle", logits, samp, dmask, pen=None, lp_want=None):
        self._pen_sample(logits, samp, dmask, pen, out=self.d_out[:mh.n])
        mh.lp.n = 0
        if lp_want is not None:
            self._lp_launch(mh.lp, lp_want, logits, self.d_out)
        if mh.plp is not None:
            mh.plp.n, mh.plp.chunks = 0, []
        if mh.plp_job is not None:
            job, mh.plp_job = mh.plp_job, None
            self._plp_launch(*job)
        mh.host[:mh.n].copy_(self.d_out[:mh.n], non_blocking=self.is_gpu)
        if mh.event is not None:
            mh.event.record()
        mh.pending, mh.logits, mh.samp, mh.seqs = False, None, None, None

    def mixed_collect(self, h: "MixedHandle") -> List[int]:
        if h.event is not None:
            self._wait(h.event)
        return h.host[:h.n].tolist()

    def _pen_stage(self, st: "_Staging", pen, n: int, nb: int):
        """Writes a step's penalty arrays into the prefix of a pinned staging set
        (padding rows: no slot)."""
        hslot, hrep, hpres, hfreq = st.h_pen
        hslot[:n], hrep[:n], hpres[:n], hfreq[:n] = pen
        hslot[n:nb] = -1

    def _decode_fill(self, seqs, nb: int, st: "_Staging") -> int:
        """Writes a decode step's inputs into a pinned staging set."""
        n = len(seqs)
        mb = self.max_decode_batch
        hs = st.hs
        ids = hs[0:mb]
        pos = hs[mb:2 * mb]
        slots = hs[2 * mb:3 * mb]
        sl = hs[3 * mb:4 * mb]
        bt = st.hbt
        bs = self.bs
        maxblk = 1
        for i, s in enumerate(seqs):
            p = s.n_tokens - 1 + s.inflight   # steps queued ahead of this one
            ids[i] = s.last_token  # replaced on the device when queued ahead
            pos[i] = p
            slots[i] = s.block_ids[p // bs] * bs + p % bs
            sl[i] = p + 1
            nbk = len(s.block_ids)
            bt[i, :nbk] = s.block_ids
            maxblk = max(maxblk, nbk)
        temp, topp, topk, seeds, steps = self._sampling_arrays(seqs)
        hs[4 * mb:4 * mb + n] = topk
        hs[5 * mb:5 * mb + n] = steps
        st.hf[:n] = temp
        st.hf[mb:mb + n] = topp
        st.hseed[:n] = seeds
        # ln(min_p): every step writes its rows' words (-inf = off), so a replay of the
        # min_p variant never sees a stale value
        st.h_minp[:nb] = -np.inf
        st.mp = False
        if self.mp_active:
            for i, s in enumerate(seqs):
                v = s.params.min_p
                if v > 0.0 and temp[i] > 0.0:
                    st.h_minp[i] = ln_min_p(v)
                    st.mp = True
        if nb > n:  # padding rows: no KV write, empty context (no attention work), greedy
            ids[n:nb] = 0
            pos[n:nb] = 0
            slots[n:nb] = -1
            sl[n:nb] = 0
            bt[n:nb, 0] = 0
            hs[4 * mb + n:4 * mb + nb] = 0
            hs[5 * mb + n:5 * mb + nb] = 0
            st.hf[n:nb] = 0.0
            st.hf[mb + n:mb + nb] = 1.0
        return maxblk

    def _gap_mark(self, start: bool, kind: str = "d"):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        if start:
            if self._gaps and self._gaps[-1][1] is None:   # an unclosed step: drop it
                self._gaps.pop()
            self._gaps.append([ev, None, kind])
        elif self._gaps and self._gaps[-1][1] is None:
            self._gaps[-1][1] = ev

    def gap_summary(self) -> Dict[str, float]:
        """FT_GPU_GAPS: idle GPU time between consecutive steps, by transition
        (d = graph-replayed decode, m = synchronous mixed step, a = mixed step
        queued ahead), and each kind's mean span from its first to its last
        launch (a mixed step's span includes any wait for the host's launches)."""
        if not self._gaps:
            return {}
        torch.cuda.synchronize(self.device)
        out: Dict[str, float] = {}
        busy: Dict[str, List[float]] = {}
        trans: Dict[str, List[float]] = {}
        prev = None
        for e0, e1, kind in self._gaps:
            if e1 is None:
                prev = None
                continue
            busy.setdefault(kind, []).append(e0.elapsed_time(e1))
            if prev is not None:
                trans.setdefault(prev[1] + kind, []).append(max(0.0, prev[0].elapsed_time(e0)))
            prev = (e1, kind)
        if not trans:
            return {}
        gaps = [g for v in trans.values() for g in v]
        out.update(idle_ms_total=round(sum(gaps), 1), idle_ms_per_step=round(sum(gaps) / len(gaps), 3),
                   idle_ms_max=round(max(gaps), 2), steps=sum(len(v) for v in busy.values()))
        for k, v in sorted(busy.items()):
            out[f"span_ms_{k}"] = round(sum(v) / len(v), 3)
            out[f"n_{k}"] = len(v)
        if "d" in busy:
            out["gpu_ms_per_step"] = out["span_ms_d"]
        for k, v in sorted(trans.items()):
            out[f"idle_ms_{k}"] = round(sum(v), 1)
            out[f"n_{k}"] = len(v)
        return out

    def _decode_enqueue(self, st: "_Staging", nb: int, n: int, from_device: bool = False,
                        gather: Optional[np.ndarray] = None, fwd_only: bool = False,
                        pen: bool = False, mp: bool = False):
        nw = 10 * self.max_decode_batch + nb * self.max_blocks_per_seq
        if self._gaps is not None:   # g: a split step, closed by its sampler (sample_launch)
            self._gap_mark(True, "g" if fwd_only else "d")
        if pen:   # the same copy, started at the penalty prefix (it carries the min_p words)
            pw = pen_words(self.max_decode_batch) + minp_words(self.max_decode_batch)
            self.d_all[:pw + nw].copy_(st.h_all[:pw + nw], non_blocking=True)
            self.stats["penalty_steps"] += 1
        elif mp and not fwd_only:   # the same copy, started at the min_p words
            pw, mw = pen_words(self.max_decode_batch), minp_words(self.max_decode_batch)
            self.d_all[pw:pw + mw + nw].copy_(st.h_all[pw:pw + mw + nw], non_blocking=True)
        else:
            self.d_in[:nw].copy_(st.h_in[:nw], non_blocking=True)
        if mp and not fwd_only:
            self.stats["min_p_steps"] += 1
        if from_device:  # the previous step's sampled ids feed this step
            if gather is None:
                self.d_input_ids[:nb].copy_(self.d_out[:nb])
            elif (gather >= 0).all():   # rows of the previous step, survivors only
                st.h_map[:nb].numpy()[:] = gather
                self.d_map[:nb].copy_(st.h_map[:nb], non_blocking=True)
                torch.index_select(self.d_out, 0, self.d_map[:nb], out=self.d_input_ids[:nb])
            else:   # gather < 0: a sequence with no queued step keeps its host id
                dst = np.nonzero(gather >= 0)[0]
                k = len(dst)
                if k:
                    hm = st.h_map.numpy()
                    hm[:k] = gather[dst]
                    hm[k:2 * k] = dst
                    self.d_map[:2 * k].copy_(st.h_map[:2 * k], non_blocking=True)
                    self.d_input_ids.index_copy_(0, self.d_map[k:2 * k],
                                                 self.d_out.index_select(0, self.d_map[:k]))
        if fwd_only:
            pair = self._split_any(nb)   # every variant of a bucket shares the forward graph
            if pair is None:
                pair = self._capture_split(nb, False)
            pair[0].replay()
            self.stats["graph_replays"] += 1
            self.stats["deferred_samples"] = self.stats.get("deferred_samples", 0) + 1
            return
        gk = _gkey(nb, pen, mp)
        g = self.graphs.get(gk)
        if g is None:
            g = self._capture(nb, pen, mp)
        g.replay()
        self.stats["graph_replays"] += 1
        if st.lp_want is not None:   # on the graph's raw logits, before the next replay overwrites them
            self._lp_launch(st.lp, st.lp_want, self._graph_logits[gk], self.d_out)
        st.h_out[:n].copy_(self.d_out[:n], non_blocking=True)
        flag = self.comm.error_flag if self.checks_comm else None
        st.err_armed = flag is not None
        if flag is not None:  # the graph folded the ranks' error words into it
            st.h_err.copy_(flag, non_blocking=True)
        st.event.record()
        if self._gaps is not None:
            self._gap_mark(False)

    # ------------------------------------------------------------------ TP workers
    @torch.inference_mode()
    def run_remote(self, msg) -> bool:
        """Executes one message broadcast by TP rank 0 (same kernels, same
        collectives, same order).  Returns False on ``stop``."""
        kind, host, masks = msg
        if kind == "stop":
            return False
        if kind == "mixed":
            self._mixed_msgs += 1
            if self._stall_mixed and self._mixed_msgs == self._stall_at:
                self._fault_stall()
            self._mixed_run(host, masks)
        elif kind == "graph":
            self._graph_msgs += 1
            if not self._stall_mixed and self._graph_msgs == self._stall_at:
                self._fault_stall()
            nb, n = host["nb"], host["n"]
            self._set_masks(masks, n)
            st = self.stg[0]
            st.hs[:] = host["small"]
            bt = host["bt"]
            st.hbt[:nb, :bt.shape[1]] = bt
            st.hf[:] = host["f32"]
            st.hseed[:] = host["seeds"]
            self._decode_enqueue(st, nb, n, from_device=host.get("from_device", False),
                                 gather=host.get("rowmap"))
            self._wait(st.event)
        elif kind == "warmup":
            self.warmup(host)
        elif kind == "swap":
            self._swap(*host)
        elif kind == "comm_fault":
            self._drop_custom_collectives()
        else:
            raise ValueError(f"unknown TP message {kind!r}")
        return True

    def _fault_stall(self):
        log.warning("FT_FAULT_TP_STALL: rank %d stalls", self.comm.rank)
        t_end = time.time() + self._stall_s
        while time.time() < t_end and not (self.comm.custom is not None
                                           and self.comm.custom.peer_error(0)):
            time.sleep(0.01)

    def _decode_meta(self, nb: int) -> AttnMeta:
        assert nb <= self.max_decode_rows
        return AttnMeta(positions=self.d_positions[:nb], slot_mapping=self.d_slots[:nb],
                        logits_indices=self.d_logits_idx[:nb], num_decode=nb,
                        dec_block_tables=self.d_bt[:nb], dec_seq_lens=self.d_seq_lens[:nb],
                        tmp_out=self.tmp_out, tmp_ml=self.tmp_ml, dec_counters=self.dec_counters)

    def _split_any(self, nb: int):
        return next((v for k, v in self.graphs_split.items() if k[0] == nb), None)

    def _graph_sample(self, logits, nb: int, pen: bool, mp: bool = False):
        """The sampler of a decode graph: with ``pen`` it is apply -> sample -> update,
        the penalties applied out of place so the graph's logits stay raw (logit taps);
        with ``mp`` the sampler reads the step's ln(min_p) array."""
        mask = self.d_mask[:nb] if self.d_mask is not None else None
        if pen:
            slot, rp, pr, fr = (t[:nb] for t in self.d_pen)
            logits = ops.penalty_apply(logits, slot, rp, pr, fr, self.pen_table, self.pen_bias_ids,
                                       self.pen_bias_vals, out=torch.empty_like(logits))
        ops.sample(logits, self.d_temp[:nb], self.d_top_p[:nb], self.d_top_k[:nb],
                   self.d_seeds[:nb], self.d_steps[:nb], out=self.d_out[:nb], mask=mask,
                   min_p=self.d_minp[:nb] if mp else None)
        if pen:
            ops.penalty_update(self.pen_table, slot, self.d_out[:nb])

    def _graph_body(self, nb: int, keep: bool = False, pen: bool = False, mp: bool = False):
        meta = self._decode_meta(nb)
        h = self.model.forward(self.d_input_ids[:nb], meta, self.kv)
        logits = self.model.compute_logits(h)
        if keep:   # graph-pool memory: holds each replay's logits until the next one
            self._graph_logits[_gkey(nb, pen, mp)] = logits
        self._graph_sample(logits, nb, pen, mp)
        if self.checks_comm:
            self.comm.export_error()

    @torch.inference_mode()
    def _capture_split(self, nb: int, pen: bool = False, mp: bool = False):
        """The forward graph (-> logits, held in ``_fwd_logits``) and the sampler graph
        of bucket ``nb`` for pipelined guided decoding, captured like ``_capture``.
        The ``pen`` / ``mp`` variants share the forward graph; only the sampler is captured
        again (with the penalty kernels around it, reading the ln(min_p) array).
        Nothing replays between a step's two halves (its sampler is queued before
        the next forward), so the pool may share their temporaries with every other
        graph; the logits stay allocated."""
        t0 = time.time()
        other = self._split_any(nb)
        if other is not None:
            # (a forward may be pending here: only the sampler runs, on its own logits)
            return self._capture_split_sampler(nb, pen, other[0], t0, mp)
        self._assert_no_pending_split("split-graph capture")
        saved = (self.d_slots[:nb].clone(), self.d_seq_lens[:nb].clone())
        self.d_slots[:nb].fill_(-1)
        self.d_seq_lens[:nb].fill_(0)
        psaved = self._pen_capture_begin(nb, pen)

        def fwd():
            h = self.model.forward(self.d_input_ids[:nb], self._decode_meta(nb), self.kv)
            return self.model.compute_logits(h)

        def samp(lg):
            self._graph_sample(lg, nb, pen, mp)

        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            samp(fwd())  # warm-up (allocator, lazy init)
        torch.cuda.current_stream(self.device).wait_stream(s)
        if self.graph_pool is None:
            self.graph_pool = torch.cuda.graph_pool_handle()
        gf = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gf, pool=self.graph_pool):
            lg = fwd()
        self._fwd_logits[nb] = lg
        gs = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gs, pool=self.graph_pool):
            samp(lg)
        self.d_slots[:nb].copy_(saved[0])
        self.d_seq_lens[:nb].copy_(saved[1])
        self._pen_capture_end(nb, psaved)
        self.graphs_split[_gkey(nb, pen, mp)] = (gf, gs)
        self.stats["captures"] += 1
        log.info("captured split decode graphs batch=%d pen=%d min_p=%d in %.2fs", nb, pen, mp,
                 time.time() - t0)
        return gf, gs

    def _capture_split_sampler(self, nb: int, pen: bool, gf, t0: float, mp: bool = False):
        lg = self._fwd_logits[nb]
        psaved = self._pen_capture_begin(nb, pen)
        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            self._graph_sample(lg, nb, pen, mp)  # warm-up (allocator)
        torch.cuda.current_stream(self.device).wait_stream(s)
        gs = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gs, pool=self.graph_pool):
            self._graph_sample(lg, nb, pen, mp)
        self._pen_capture_end(nb, psaved)
        self.graphs_split[_gkey(nb, pen, mp)] = (gf, gs)
        self.stats["captures"] += 1
        log.info("captured split sampler graph batch=%d pen=%d min_p=%d in %.2fs", nb, pen, mp,
                 time.time() - t0)
        return gf, gs

    def _pen_capture_begin(self, nb: int, pen: bool):
        """Warm-up and capture runs of a penalty graph must not touch any slot's state:
        every row's slot is -1 while they run (restored by _pen_capture_end)."""
        if not pen:
            return None
        saved = self.d_pen[0][:nb].clone()
        self.d_pen[0][:nb].fill_(-1)
        return saved

    def _pen_capture_end(self, nb: int, saved):
        if saved is not None:
            self.d_pen[0][:nb].copy_(saved)

    @torch.inference_mode()
    def _capture(self, nb: int, pen: bool = False, mp: bool = False):
        """Captures the decode graph of batch bucket ``nb``.  Always under
        inference mode, whichever path triggers it (pipelined launches run outside
        ``execute``): the CUDA generator's graph-safe RNG state is created by the
        first capture and must be of the same kind for every later one."""
        self._assert_no_pending_split("graph capture")
        t0 = time.time()
        # inputs must be valid for the warm-up/capture run: no KV writes, empty contexts
        saved = (self.d_slots[:nb].clone(), self.d_seq_lens[:nb].clone())
        self.d_slots[:nb].fill_(-1)
        self.d_seq_lens[:nb].fill_(0)
        psaved = self._pen_capture_begin(nb, pen)
        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s), self._long_waits():
            self._graph_body(nb, pen=pen, mp=mp)  # warm-up (allocator, lazy init)
        torch.cuda.current_stream(self.device).wait_stream(s)
        if self.graph_pool is None:
            self.graph_pool = torch.cuda.graph_pool_handle()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=self.graph_pool):
            self._graph_body(nb, keep=True, pen=pen, mp=mp)
        self.d_slots[:nb].copy_(saved[0])
        self.d_seq_lens[:nb].copy_(saved[1])
        self._pen_capture_end(nb, psaved)
        self.graphs[_gkey(nb, pen, mp)] = g
        self.stats["captures"] += 1
        log.info("captured decode graph batch=%d pen=%d min_p=%d in %.2fs", nb, pen, mp,
                 time.time() - t0)
        return g

    def _decode_eager(self, seqs, masks) -> List[int]:
        self.stats["eager_decode"] += 1
        from .scheduler import ScheduledBatch as _SB

        return self._mixed(_SB(list(seqs), [], [], []), masks)

    @staticmethod
    def _warm_split_graphs() -> bool:
        """Pre-capture the split (forward | sampler) graphs of pipelined guided decoding?
        Guided rows come from grammar-constrained tool calls or JSON-schema requests.
        ``ENGINE_WARM_SPLIT_GRAPHS`` decides when set; otherwise only a service with
        guided tool calls on (``AGENT_GUIDED_TOOL_CALLS``) pays for them at start-up, and
        any other deployment captures a bucket's pair on its first guided step."""
        env = os.environ.get("ENGINE_WARM_SPLIT_GRAPHS")
        if env is not None:
            return env.strip().lower() not in ("0", "false", "no", "off", "")
        return os.environ.get("AGENT_GUIDED_TOOL_CALLS", "false").strip().lower() == "true"

    def warmup(self, batch_sizes=None):
        """Pre-capture decode graphs (one per batch bucket, any context length) so
        serving never pays for a capture."""
        if not self.use_graphs:
            return
        if self.bcast is not None:
            self.bcast.send(("warmup", list(batch_sizes or self.graph_sizes), None))
        t0 = time.time()
        split = self.can_defer_sample() and self._warm_split_graphs()
        # ENGINE_PENALTIES_WARM=1: the penalty variants too (otherwise captured by the
        # first step of a bucket that carries a penalised row)
        pens = (False, True) if self.pen_table is not None and \
            os.environ.get("ENGINE_PENALTIES_WARM", "0") == "1" else (False,)
        for b in batch_sizes or self.graph_sizes:
            b = self._bucket(b)
            for pen in pens:
                if b is not None and (b, pen) not in self.graphs:
                    self._capture(b, pen)
                if b is not None and split and (b, pen) not in self.graphs_split:
                    self._capture_split(b, pen)
        log.info("decode graphs ready (%d + %d split) in %.1fs", len(self.graphs),
                 len(self.graphs_split), time.time() - t0)
