"""``LMM`` - drop-in for the reference's ``core.models.LMM`` on the ArAE decode path
(reference: core/models.py:32-99 constructor, :101-144 encode_cond, :204-319 generate).

Same constructor argument (``Options``), same checkpoint keys, same
``generate(conds, num_faces, resume_ids, tokenizer, max_new_tokens, clean)``
signature and return value ``(meshes, all_tokens)``.  Differences, all additive:
``B > 1`` is allowed (independent rows, per-row grammar state), ``min_new_tokens``
can be passed (benchmark rule: EOS suppressed until T).  ``forward`` / ``__call__`` score a batch the way the
reference's eval loop does (core/models.py:147-202 under ``model.eval()``, main.py:244-268); training mode (backward,
num-face dropout) and the image conditioner are not part of this path.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional

import numpy as np
import torch

from . import native
from .grammar import select_grammar
from .shape_opt import BuiltinGrammar, NativeShapeOPT
from .utils import quantize_num_faces
from .weights import dims_from_options

IGNORE_INDEX = -100           # F.cross_entropy's ignore_index: the reference's collate_fn writes it over cond tokens, BOS and padding
_INDEX_LIMIT = 2 ** 31 - 1    # er_score / er_prefill: B * S * max(intermediate_dim, 3 * hidden_dim, vocab) must stay below 2^31


def score_row_groups(batch: int, seq_len: int, dims, max_rows: int = 1023) -> List[tuple]:
    """Consecutive row ranges [(start, end), ...] that ``LMM.forward`` scores one ``er_score`` call at a time.  Rows are independent
    (causal attention, right padding), so a batch is cut wherever the 32-bit row indexing of the prefill (B * S * widest Linear
    output < 2^31) or the context's batch limit (``max_rows``) would be exceeded; every group but the last is full."""
    if batch <= 0 or seq_len <= 0:
        raise ValueError(f"batch {batch} / seq_len {seq_len} must be positive")
    width = max(dims.intermediate_dim, 3 * dims.hidden_dim, dims.vocab_size)
    per = _INDEX_LIMIT // (seq_len * width)
    if per < 1:
        raise ValueError(f"one row of {seq_len} positions exceeds the 32-bit index range of the prefill ({seq_len} x {width})")
    per = min(per, max_rows)
    return [(b, min(b + per, batch)) for b in range(0, batch, per)]


def prefix_leaders(conds) -> List[int]:
    """The grouping behind ``share_prefix``: leaders[b] = the first row whose ``conds`` entry is bit-equal to row b's (b itself when
    there is none before it).  ``conds`` is a tensor or array [B, ...]; equality is on the stored bits, so -0.0 and 0.0 differ and
    a NaN equals the same NaN.  A pure function of the host copy of ``conds``."""
    a = conds.detach().cpu().numpy() if isinstance(conds, torch.Tensor) else np.asarray(conds)
    first: Dict[bytes, int] = {}
    return [first.setdefault(np.ascontiguousarray(a[b]).tobytes(), b) for b in range(a.shape[0])]


def fork_plan(conds, resume_ids=None):
    """The plan behind ``fork_prefill``: ``(order, leader, n_leaders)`` for a batch whose rows are EQUAL when their ``conds`` entry and
    their ``resume_ids`` row are both bit-equal (as ``prefix_leaders``: -0.0 and 0.0 differ; one ``num_faces`` per call).  ``order`` is
    the stable permutation that puts each class's first row in front - the row at permuted place i is the caller's row ``order[i]``:
    first the classes' first rows in first-occurrence order (``n_leaders`` of them), then every other row in the caller's order.
    ``leader[i]`` is the permuted place of the first row of place i's class, so ``leader[i] == i`` below ``n_leaders`` and
    ``leader[i] < n_leaders`` behind: the table ``er_prefill_fork`` takes, and a valid ``er_set_prefix_groups`` table.  A pure function
    of the host copies; ``conds`` may be None (no conditioning: the rows are told apart by ``resume_ids`` alone, which then gives B)."""
    host = lambda t: None if t is None else (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t))
    c, r = host(conds), host(resume_ids)
    if c is None and r is None:
        raise ValueError("fork_plan: neither conds nor resume_ids")
    B = (c if c is not None else r).shape[0]
    if c is not None and r is not None and r.shape[0] != B:
        raise ValueError(f"fork_plan: {B} conds entries but {r.shape[0]} resume_ids rows")
    key = lambda b: (b"" if c is None else np.ascontiguousarray(c[b]).tobytes(), b"" if r is None else np.ascontiguousarray(r[b]).tobytes())
    place: Dict[tuple, int] = {}
    firsts, cls = [], []
    for b in range(B):
        k = key(b)
        if k not in place:
            place[k] = len(firsts)
            firsts.append(b)
        cls.append(place[k])
    is_first = set(firsts)
    rest = [b for b in range(B) if b not in is_first]
    order = firsts + rest
    return order, [cls[b] for b in order], len(firsts)


def cond_key(conds) -> bytes:
    """The stored bits of a ``conds`` batch with its shape and dtype: two batches are the same input to the point encoder exactly when
    their keys are equal (the comparison of ``prefix_leaders`` / ``fork_plan``: -0.0 and 0.0 differ, a NaN equals the same NaN)."""
    a = conds.detach().cpu().numpy() if isinstance(conds, torch.Tensor) else np.asarray(conds)
    return repr((a.shape, a.dtype.str)).encode() + b"|" + np.ascontiguousarray(a).tobytes()


def kept_prefix_len(num_cond_tokens: int, use_num_face_cond: bool) -> int:
    """Cache positions that depend on the cloud alone: ``encode_cond`` appends the face-count token BEHIND the conditioning tokens
    (core/models.py:134-141) and the decoder is causal, so everything before that token survives another face count."""
    return num_cond_tokens - 1 if use_num_face_cond else num_cond_tokens


class CondRecord:
    """What ``generate_ids(keep_cond=True)`` remembers of a prefill: the clouds' bits, the batch, the kept prefix length, and the decoder
    context with its reservation and ``cache_epoch`` right after that prefill.  ``usable`` says whether a later call may extend that
    prefix instead of running the full pass; any mismatch means the full pass (which records again).  Host data only."""

    def __init__(self):
        self.forget()

    def forget(self):
        self.key, self.batch, self.past, self.dec_id, self.reserved, self.epoch = None, 0, 0, None, (0, 0), -1

    def remember(self, conds, batch: int, past: int, dec_id: int, reserved, epoch: int):
        self.key, self.batch, self.past = cond_key(conds), int(batch), int(past)
        self.dec_id, self.reserved, self.epoch = dec_id, tuple(reserved), int(epoch)

    def usable(self, conds, batch: int, need_len: int, dec_id: int, reserved, epoch: int, queue_open: bool = False) -> bool:
        """``need_len``: positions the call will hold at most (prefix + new tokens + 1).  The context must be the recorded one, its
        reservation and cache untouched since (``cache_epoch``), no queue open, and the reservation must already fit."""
        if self.key is None or queue_open or conds is None:
            return False
        if dec_id != self.dec_id or tuple(reserved) != self.reserved or int(epoch) != self.epoch:
            return False
        if int(batch) != self.batch or self.reserved[0] != self.batch or self.reserved[1] < int(need_len) or self.past < 1:
            return False
        return cond_key(conds) == self.key


def fork_streams(order, row_streams=None) -> List[int]:
    """The Philox stream of every permuted place under ``fork_prefill``: the stream the caller's row ``order[i]`` would have had - its
    original index, or the caller's ``row_streams`` entry - so that sample-mode ids do not depend on the permutation."""
    if row_streams is not None and len(row_streams) != len(order):
        raise ValueError(f"row_streams has {len(row_streams)} entries for a batch of {len(order)}")
    return [int(o) if row_streams is None else int(row_streams[o]) for o in order]


class _QueueJob:
    """One job of ``LMM.generate_queue``: ``(conds, num_faces, resume_ids=None, stream=None, max_new_tokens=None)``."""

    def __init__(self, index: int, spec, default_budget: int):
        spec = tuple(spec)
        if not 2 <= len(spec) <= 5:
            raise ValueError(f"job {index}: (conds, num_faces[, resume_ids[, stream[, max_new_tokens]]]), got {len(spec)} fields")
        conds, num_faces, resume, stream, budget = spec + (None,) * (5 - len(spec))
        conds = torch.as_tensor(conds)
        self.conds = conds[None] if conds.dim() == 2 else conds
        if self.conds.dim() != 3 or self.conds.shape[0] != 1:
            raise ValueError(f"job {index}: conds must be [N, C] or [1, N, C], got {tuple(conds.shape)}")
        self.num_faces = int(num_faces)
        self.resume = None if resume is None else torch.as_tensor(resume).to("cpu", torch.long).reshape(1, -1)
        self.stream = index if stream is None else int(stream)
        self.budget = int(default_budget if budget is None else budget)
        if self.budget < 1:
            raise ValueError(f"job {index}: max_new_tokens={self.budget}")

    def input_key(self) -> tuple:
        """What decides the job's prefill, as bytes: two jobs with equal keys are repeats of one input (``fork_repeats``)."""
        c = self.conds.detach().cpu().numpy()
        return (c.dtype.str, c.shape, np.ascontiguousarray(c).tobytes(), self.num_faces,
                b"" if self.resume is None else self.resume.numpy().tobytes())


def queue_fork_split(keys) -> List[int]:
    """For the jobs of ONE admit call, by their ``input_key``: source[i] = the place in the call of the first job with job i's key (i
    itself for a job that is prefilled).  A pure host function; ``sum(source[i] != i)`` jobs are admitted by copy."""
    first: Dict[tuple, int] = {}
    return [first.setdefault(k, i) for i, k in enumerate(keys)]


class _QueueEngine:
    """The engine ``edgerunner_amd.queue.QueueScheduler`` drives: admissions are prefills into cache rows of the native context."""

    def __init__(self, lmm: "LMM", jobs: List[_QueueJob], logprobs: bool = False, fork_repeats: bool = False):
        self.lmm, self.jobs, self.dec = lmm, jobs, lmm.mesh_decoder
        # fork_repeats: inside one admit call a job whose input repeats an earlier job's is not prefilled: it starts as a copy of that
        # job's row (er_queue_admit_copy), taken before any step runs.  The prefilled job's pass is the one it would have had anyway.
        self.fork_repeats = fork_repeats
        self.forked = 0               # rows admitted by copy
        self.logprobs = logprobs      # take() then returns (ids, float32 [2, n]): the job's model / policy log-probs
        # exact mode: the jobs of one admit call that share a prefix length go through ONE forward pass (rows of a batched prefill
        # give the ids of their single runs, as LMM.generate's batches do).  Fast mode: one row per pass - the fp16-weight Linears of
        # the prefill pick their kernel by the row count of the pass, so only a one-row pass is bit-identical to the job run alone.
        # With log-probs kept, exact mode prefills one row per pass too: a batched prefill gives a job the ids of its single run but may
        # round its first logits differently in the last place, and the job's log-probs are promised bit for bit.
        self.rows_per_pass = 1 if lmm.precision != "fp32" or logprobs else 32      # fp16 and fp8 are both "fast mode" here

    def embeds(self, job: _QueueJob) -> torch.Tensor:
        """inputs_embeds [1, S, hidden] of the job, built exactly as LMM.generate_ids builds them for a batch of one."""
        opt, dec = self.lmm.opt, self.dec
        cond = self.lmm.encode_cond(job.conds, [job.num_faces])["cond_embeds"]
        ids = torch.full((1, 1), opt.bos_token_id, dtype=torch.long)
        if job.resume is not None:
            ids = torch.cat((ids, job.resume), dim=1)
        tok = dec.model.embd(ids)
        return torch.cat((cond, tok), dim=1) if cond is not None else tok

    def admit(self, slot0: int, job_ids) -> None:
        n = len(job_ids)
        source = queue_fork_split([self.jobs[j].input_key() for j in job_ids]) if self.fork_repeats else list(range(n))
        embeds = [self.embeds(self.jobs[j]) if source[i] == i else None for i, j in enumerate(job_ids)]
        i = 0
        while i < n:
            if embeds[i] is None:     # a repeat: its row is filled below, from its source's
                i += 1
                continue
            k = i + 1
            while k < n and k - i < self.rows_per_pass and embeds[k] is not None and embeds[k].shape[1] == embeds[i].shape[1]:
                k += 1
            part = [self.jobs[j] for j in job_ids[i:k]]
            self.dec.queue_admit(slot0 + i, torch.cat(embeds[i:k], dim=0), [p.stream for p in part], [p.budget for p in part])
            i = k
        for s in range(n):
            copies = [i for i in range(n) if source[i] == s and i != s]
            if copies:
                part = [self.jobs[job_ids[i]] for i in copies]
                self.dec.queue_admit_copy(slot0 + s, [slot0 + i for i in copies], [p.stream for p in part], [p.budget for p in part])
                self.forked += len(copies)

    def run(self):
        return self.dec.queue_run()

    def take(self, slot: int):
        cap = max(j.budget for j in self.jobs)
        lp = self.dec.queue_row_logprobs(slot, cap) if self.logprobs else None
        ids = self.dec.queue_take(slot, cap)
        return ids if lp is None else (ids, lp[:, : len(ids)].copy())


class _Embd:
    """``mesh_decoder.model.embd`` lookalike (core/models.py:228)."""

    def __init__(self, dec: NativeShapeOPT):
        self._dec = dec

    def __call__(self, input_ids):
        return self._dec.embd(input_ids)


class _DecoderModel:
    def __init__(self, dec):
        self.embd = _Embd(dec)


_KV8_RULE = ("kv_precision='fp8' (the e4m3 KV cache) goes with the fp16-activation precisions 'mxfp4', 'fp16' or 'fp8' only: exact mode (fp32 weights) keeps an fp32 cache. "
             "Use LMM(opt, device, precision='fp16', kv_precision='fp8'), or call .half() / .fp8() / .fp4() in module style.")


class LMM:
    def __init__(self, opt, device="cuda:0", precision: Optional[str] = "fp32", kv_precision: Optional[str] = None):
        """precision: 'fp32' = exact mode (fp32 weights + KV; greedy ids bit-exact vs the CPU path), 'fp16' = fast mode
        (decoder matrices and KV cache stored in fp16 like the reference's ``model.half()`` GPU path, fp32 accumulate),
        'fp8' = fast mode on a checkpoint whose q / k / v / out_proj / fc1 / fc2 matrices are rounded to e4m3 times a power of two
        per output row (csrc/er_w8.h; the single-row decode projections stream the bytes), 'mxfp4' = fp4 mode, fast mode on a checkpoint whose same six
        matrices are rounded to MXFP4 - e2m1 values times a power of two per block of 32 elements along a row (csrc/er_w4.h; the
        single-row qkv / fc1 / fc2 projections stream the nibbles where ``ER_W4_ROWS`` or the measured rule says so), or None = module style: fp32 until ``.half()`` is called, the native context being created on first use, so
        that the reference's ``LMM(opt)`` -> ``load_state_dict`` -> ``.half().eval().to(device)`` (infer.py:41-56)
        selects the fp16 context exactly as it selects fp16 storage there.

        kv_precision: None = the KV cache in the precision's own activation dtype (fp32 / fp16), 'fp8' = one e4m3 byte per cached
        element without a scale (kv8 mode: half the cache bytes of fp16; head_dim 96).  The byte cache goes with 'fp16', 'fp8' or 'mxfp4'
        weights only: with 'fp32', or in module style once ``.float()`` selects fp32, it raises ValueError."""
        self.opt = opt
        if precision not in (None, "fp32", "fp16", "fp8", "mxfp4"):      # fp4 mode is spelled by its format: the bare "fp4" stays refused
            raise ValueError(f"{precision!r}: 'fp32', 'fp16', 'fp8', 'mxfp4' (fp4 mode) or None" if precision == "fp4" else precision)
        if kv_precision not in (None, "fp8"):
            raise ValueError(f"kv_precision={kv_precision!r}: None (the cache follows precision) or 'fp8'")
        if kv_precision == "fp8" and precision == "fp32":
            raise ValueError(_KV8_RULE)
        self._kv8 = kv_precision == "fp8"
        if opt.cond_mode == "image":
            raise NotImplementedError("cond_mode='image' (CLIP conditioner) is outside the ArAE decode path")
        if opt.cond_mode == "point" and opt.point_encoder_mode not in ("embed", "downsample"):
            raise ValueError(f"point_encoder_mode={opt.point_encoder_mode!r}: 'embed' or 'downsample'")
        self.dims = dims_from_options(opt)
        if (self.dims.hidden_dim, self.dims.intermediate_dim) != (1536, 6144) or self.dims.hidden_dim // max(self.dims.num_heads, 1) not in (96, 64):
            # the decode kernels stream 1536-wide rows in whole 1536-element slices (csrc/k_gemv.h); the reference's generic
            # ShapeOPTConfig (core/transformer/modeling_opt.py:86-134; Options() default hidden_dim 1024) is not built - say so
            # here, with the option names, instead of from er_create
            raise NotImplementedError(
                f"decoder shape hidden_dim={self.dims.hidden_dim} / intermediate_dim={self.dims.intermediate_dim} / "
                f"num_heads={self.dims.num_heads} is not built: this library serves the ArAE / DiT presets' decoder "
                "(hidden_dim=1536, intermediate_dim=6144, head_dim 96 or 64). Use config_defaults['ArAE'] (or 'DiT'), "
                "or pass --hidden_dim 1536 --num_heads 16 --intermediate_dim 6144.")
        self.vocab_size = self.dims.vocab_size
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise native.NativeError("this LMM only runs on a HIP device (cuda:N); there is no CPU fallback")
        self._dtype = torch.float16 if precision in ("fp16", "fp8", "mxfp4") else torch.float32      # activations' storage: the KV cache, the prefill's operands
        self._w8 = precision == "fp8"
        self._w4 = precision == "mxfp4"
        self._dec: Optional[NativeShapeOPT] = None
        self._sources: List[tuple] = []        # (state_dict reference, strict) of every load_state_dict call, for re-creation
        self.training = False
        self._released = False                 # release_checkpoint() was called: the context cannot be re-created
        self.last_logprobs = None              # generate(output_logprobs=True): {"model", "policy"} float32 [B, n] on the device
        self.last_queue_logprobs = None        # generate_queue(output_logprobs=True): per job (model, policy) numpy arrays
        self._cond_record = CondRecord()       # generate_ids(keep_cond=True): the prefix a later call may extend
        self.last_prefill = None               # "full" | "extend": which prefill the last generate_ids call ran
        if precision is not None:
            self._materialize()

    # -- native context ------------------------------------------------------------------------
    @property
    def precision(self) -> str:
        return "mxfp4" if self._w4 else "fp8" if self._w8 else "fp16" if self._dtype == torch.float16 else "fp32"

    @property
    def kv_precision(self) -> Optional[str]:
        """'fp8' when the KV cache holds e4m3 bytes (kv8 mode), else None: the cache is stored in the precision's activation dtype."""
        return "fp8" if self._kv8 else None

    def _materialize(self):
        if self._kv8 and self._dtype != torch.float16:
            raise ValueError(_KV8_RULE)
        if self._released:
            raise native.NativeError("LMM: the checkpoint was released (release_checkpoint()) and the native context is gone; "
                                     "create a new LMM and load the checkpoint again")
        dec = NativeShapeOPT(self.dims, self.opt, self.device, weight_dtype="fp4" if self._w4 else "fp8" if self._w8 else self._dtype,
                             kv_dtype="fp8" if self._kv8 else self._dtype)
        dec.model = _DecoderModel(dec)
        for sd, strict in self._sources:
            dec.load_state_dict(sd, strict=strict)
        dec.direct_loads = False               # everything loaded so far is replayable from self._sources
        self._dec = dec
        return dec

    @property
    def mesh_decoder(self) -> NativeShapeOPT:
        """The native decoder context (created on first access in module style)."""
        return self._dec if self._dec is not None else self._materialize()

    # -- nn.Module-shaped conveniences so infer.py reads like the reference's ----------------
    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = False):
        """Returns (missing, unexpected) like nn.Module.load_state_dict.  The dict is kept by reference (no copy) so a
        later ``.half()`` / ``.float()`` can rebuild the native context in the other storage precision."""
        self._sources.append((sd, strict))
        self._cond_record.forget()
        if self._dec is not None:
            prev = self._dec.direct_loads
            out = self._dec.load_state_dict(sd, strict=strict)
            self._dec.direct_loads = prev
            return out
        from .weights import tensor_specs
        want = {k for k, _, _ in tensor_specs(self.dims)}
        have = {k for k, t in sd.items() if isinstance(t, torch.Tensor)}
        missing, unexpected = sorted(want - have), sorted(have - want)
        if strict and (missing or unexpected):
            raise native.NativeError(f"load_state_dict(strict=True): missing {missing[:5]}, unexpected {unexpected[:5]}")
        return missing, unexpected

    def release_checkpoint(self):
        """Drop the retained state_dict references (a full ArAE checkpoint is ~2.7 GB of host memory per rank) once the native
        context holds the weights.  ``.half()`` / ``.float()`` can no longer re-store them afterwards and fail loudly."""
        _ = self.mesh_decoder                  # make sure everything retained so far is on the device
        self._sources.clear()
        self._dec.direct_loads = True
        self._released = True
        return self

    def _cast(self, dtype, w8: bool = False, w4: bool = False):
        if self._kv8 and dtype != torch.float16:
            raise ValueError(_KV8_RULE)
        if dtype == self._dtype and w8 == self._w8 and w4 == self._w4:
            return self
        if self._dec is not None and self._dec.direct_loads:
            want = "mxfp4" if w4 else "fp8" if w8 else "fp16" if dtype == torch.float16 else "fp32"
            raise native.NativeError(
                f"LMM.{'fp4' if w4 else 'fp8' if w8 else 'half' if dtype == torch.float16 else 'float'}(): this context's weights were streamed directly into "
                f"the {self.precision} native context (mesh_decoder.load_state_iter / load_state_dict); they cannot be "
                f"re-stored. Create LMM(opt, device, precision='{want}') instead.")
        self._dtype, self._w8, self._w4 = dtype, w8, w4
        self._cond_record.forget()
        if self._dec is not None:            # rebuild lazily from the retained checkpoints in the new storage precision
            self._dec.close()
            self._dec = None
        return self

    def half(self):
        """The reference casts to fp16 here (infer.py:56): selects the fp16-storage context (fp32 accumulate)."""
        return self._cast(torch.float16)

    def fp8(self):
        """Selects the fp8 context: fast mode with the decoder matrices of every layer stored as e4m3 bytes times 2^e per row."""
        return self._cast(torch.float16, w8=True)

    def fp4(self):
        """Selects the fp4 context: fast mode with the decoder matrices of every layer stored as MXFP4 (e2m1 nibbles, one e8m0 scale
        byte per block of 32 along a row)."""
        return self._cast(torch.float16, w4=True)

    def float(self):
        return self._cast(torch.float32)

    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        """Sets the flag ``forward`` checks: there is no training path here, so a training-mode forward raises."""
        self.training = bool(mode)
        return self

    def to(self, device):
        d = torch.device(device)
        if d.type != "cuda":
            raise native.NativeError("this LMM only runs on a HIP device")
        if d.index is not None and self.device.index is not None and d.index != self.device.index:
            if self._dec is not None and self._dec.direct_loads:
                raise native.NativeError("LMM.to(): weights were streamed into the context of another device")
            if self._dec is not None:
                self._dec.close()
                self._dec = None
            self.device = d
        return self

    # -- conditioning -------------------------------------------------------------------------
    @torch.no_grad()
    def encode_cond(self, conds, num_faces):
        """core/models.py:101-144 (eval mode).  ``num_faces``: LongTensor[B] or list."""
        nf = num_faces.tolist() if isinstance(num_faces, torch.Tensor) else list(num_faces)
        buckets = [quantize_num_faces(int(n)) for n in nf]
        return {"cond_embeds": self.mesh_decoder.encode_cond(conds, buckets)}

    # -- scoring (the reference's eval-mode forward) --------------------------------------------------
    def __call__(self, data, step_ratio=1):
        return self.forward(data, step_ratio)

    @torch.no_grad()
    def forward(self, data, step_ratio=1):
        """core/models.py:147-202 in eval mode: ``data`` is the reference's batch (``collate_fn``: conds, tokens, labels, masks,
        num_faces, num_tokens).  Returns loss_ce (shifted cross entropy, mean over supervised positions), loss_kl (point mode:
        0.5 * sum of the latent mean squared over the batch), loss = loss_ce + kl_weight * loss_kl, logits float32 [B, S, V] on the
        device, and nll [B, S] (per-position -log p of the next label, 0 where ignored).  Logits at padded positions are not part
        of the contract.  Right padding only (what collate_fn produces); ``step_ratio`` is unused, as in the reference."""
        out = self.score(data)
        out.pop("pred")
        return out

    @torch.no_grad()
    def score(self, data) -> Dict[str, torch.Tensor]:
        """``forward`` plus ``pred`` [B, S] int32: the argmax of every position's logits (lowest index on ties), from the same kernel
        that computes ``nll``."""
        if self.training:
            raise NotImplementedError("LMM.forward in training mode (backward pass, num-face dropout) is not part of this path; "
                                      "call .eval() first")
        opt, d = self.opt, self.dims
        tokens = torch.as_tensor(data["tokens"]).to("cpu", torch.long)
        labels = torch.as_tensor(data["labels"]).to("cpu", torch.long)
        masks = torch.as_tensor(data["masks"]).to("cpu").bool()
        if tokens.dim() != 2 or labels.dim() != 2:
            raise ValueError(f"tokens {tuple(tokens.shape)} / labels {tuple(labels.shape)} must be [B, length]")
        B, S = labels.shape
        if tokens.shape[0] != B or S != d.num_cond_tokens + tokens.shape[1]:
            raise ValueError(f"labels {tuple(labels.shape)} do not cover the {d.num_cond_tokens} cond tokens + tokens "
                             f"{tuple(tokens.shape)}")
        if tuple(masks.shape) != (B, S):
            raise ValueError(f"masks {tuple(masks.shape)} do not match labels {tuple(labels.shape)}")
        lens = masks.sum(dim=1)
        if not torch.equal(masks, torch.arange(S)[None, :] < lens[:, None]):
            raise ValueError("masks must be ones followed by zeros in every row: only right padding (collate_fn's) is supported")
        if (labels[~masks] != IGNORE_INDEX).any():
            raise ValueError(f"labels must be {IGNORE_INDEX} wherever the mask is 0")
        sup = labels != IGNORE_INDEX
        if ((labels[sup] < 0) | (labels[sup] >= self.vocab_size)).any():
            raise ValueError(f"labels outside [0, {self.vocab_size}) that are not {IGNORE_INDEX}")
        conds = data.get("conds")
        num_faces = data["num_faces"]
        cond_embeds = self.encode_cond(conds, num_faces)["cond_embeds"]
        dec = self.mesh_decoder
        token_embeds = dec.model.embd(tokens)
        inputs_embeds = torch.cat((cond_embeds, token_embeds), dim=1) if d.num_cond_tokens else token_embeds
        dev = self.device
        logits = torch.empty((B, S, self.vocab_size), dtype=torch.float32, device=dev)
        nll = torch.empty((B, S), dtype=torch.float32, device=dev)
        pred = torch.empty((B, S), dtype=torch.int32, device=dev)
        groups = score_row_groups(B, S, d)
        for b0, b1 in groups:
            r = dec.score(inputs_embeds[b0:b1], labels[b0:b1], logits_out=logits[b0:b1], nll_out=nll[b0:b1], pred_out=pred[b0:b1])
            loss = r["loss"]
        if len(groups) > 1:      # the same fixed-order reduction over the whole batch (nll / pred come out bit-identical)
            from .kernels import score_rows
            with torch.cuda.device(dev):
                _, _, loss = score_rows(logits, labels.to(dev))
        results = {"loss_ce": loss[0]}
        total = loss[0]
        if d.cond_mode == "point":
            _, kl = dec.point_latent(conds)
            results["loss_kl"] = kl
            total = total + opt.kl_weight * kl
        results["loss"] = total
        results["logits"] = logits
        results["nll"] = nll
        results["pred"] = pred
        return results

    # -- generation ---------------------------------------------------------------------------
    @torch.no_grad()
    def generate_ids(self, conds, num_faces=1000, resume_ids=None, tokenizer=None, max_new_tokens=None,
                     min_new_tokens: int = 0, seed: Optional[int] = None, row_streams=None, share_prefix=False, *,
                     temperature: Optional[float] = None, top_p: Optional[float] = None, top_k: Optional[int] = None,
                     output_logprobs: bool = False, fork_prefill: bool = False, keep_cond: bool = False) -> torch.Tensor:
        """Everything of LMM.generate up to the HF call's return value (core/models.py:215-303).

        ``keep_cond=True``: after the prefill the model remembers a host copy of ``conds``, the batch and the cache positions that
        depend on the clouds alone (``kept_prefix_len``: num_cond_tokens - 1, the face-count token comes behind them).  A later call
        with ``keep_cond=True``, bit-equal ``conds`` (``cond_key``), the same batch, no queue open, the decoder's cache untouched in
        between (decoding does not count) and a reservation that already fits skips the point encoder and the cond positions: it runs
        ``prefill_extend`` over [face-count token, BOS, resume_ids ...] behind the kept prefix - another face count or another resume
        tail costs its few positions.  Anything else silently takes the full path and records again; ``.half()`` / ``.float()`` /
        ``load_state_dict`` and any re-reserve forget the record.  ``last_prefill`` says which path ran ("full" | "extend").  The extend
        path with ``fork_prefill=True`` or ``share_prefix`` raises NotImplementedError for now; a full-path call with them is fine.

        ``fork_prefill=True``: rows whose ``conds`` entry and ``resume_ids`` row are both bit-equal (``fork_plan``) are encoded and
        prefilled ONCE; the repeats start from a copy of that row's cache rows and last hidden state (``er_prefill_fork``), which is
        bit for bit what their own pass would have written next to that row.  Any batch size, precision and cache type.  Ids and
        ``last_logprobs`` come back in the caller's row order, and in sample mode a row draws from the stream it would have had
        (its index, or its ``row_streams`` entry).  The first rows of the classes are prefilled as a batch of their own, so their
        state is that of ``generate_ids`` on those rows alone (exact mode: the ids of the unforked call; fast mode: the GEMMs of the
        prefill pick their kernels by the row count of the pass).  With ``share_prefix`` the groups are the plan's classes (rows of one
        cloud whose ``resume_ids`` differ are then not grouped).  A batch without repeats takes the path of ``fork_prefill=False``.

        ``temperature`` / ``top_p`` / ``top_k`` (None: the reference's call, ``top_k=10`` in sample mode; ``top_k=0``: no top-k
        filter) shape the draw of sample mode as HF's warpers do; greedy mode accepts them and picks the same ids.
        ``output_logprobs=True`` leaves ``last_logprobs = {"model", "policy"}``, float32 [B, n] on the device for the n id columns
        returned: the model's log-softmax at the chosen id (``score``'s ``-nll``) and the id's log-probability in the distribution
        it was taken from (greedy: log-softmax of the grammar-masked row).  Otherwise ``last_logprobs`` is None.

        ``share_prefix=True``: rows whose ``conds`` entries are bit-equal (``prefix_leaders``) form a group, and every decode step reads
        the group's cond + BOS prefix (num_cond_tokens + 1 cache positions; one ``num_faces`` per call, so ``resume_ids`` may differ
        behind it) once from the first such row's cache instead of once per row (``er_set_prefix_groups``).  The tokens are those
        of ``share_prefix=False`` up to the rounding of a different summation order.  It acts on the batched decode path only: with
        B <= 4 and no ``ER_FORCE_BATCHED=1`` it has no effect.  ``share_prefix="mfma"`` is ``True`` with the prefix pass of this call on the
        matrix cores (``er_set_prefix_pass``; fast mode's fp16 cache only, ``NativeError`` otherwise) and is ignored where ``True`` is;
        ``True`` runs the pass the context is set to (``NativeShapeOPT.set_prefix_pass``, env ``ER_PREFIX_PASS``; the VALU pass by default)."""
        if share_prefix not in (False, True, None, "mfma", "valu"):
            raise ValueError(f"share_prefix must be a bool, 'valu' or 'mfma', got {share_prefix!r}")
        opt = self.opt
        B = conds.shape[0]
        max_new_tokens = opt.max_seq_length if max_new_tokens is None else max_new_tokens
        rec, dec = self._cond_record, self.mesh_decoder
        past = kept_prefix_len(opt.num_cond_tokens, self.dims.use_num_face_cond)
        n_resume = 0 if resume_ids is None else resume_ids.shape[1]
        extend = bool(keep_cond) and rec.usable(conds, B, opt.num_cond_tokens + 1 + n_resume + max_new_tokens + 1, id(dec), dec._reserved,
                                                dec.cache_epoch)
        if extend and (fork_prefill or share_prefix):
            raise NotImplementedError("generate_ids: keep_cond=True would extend the kept cond prefix here, which does not combine with "
                                      "fork_prefill / share_prefix yet; drop one of them for this call")
        fork = None
        if fork_prefill:
            order, leader, n_leaders = fork_plan(conds, resume_ids)
            if n_leaders < B:
                fork = (order, leader)
                row_streams = fork_streams(order, row_streams)
                first = torch.as_tensor(order[:n_leaders], dtype=torch.long)
                conds = conds[first.to(conds.device)]
                resume_ids = None if resume_ids is None else resume_ids[first.to(resume_ids.device)]
        N = conds.shape[0]                     # rows that are encoded and prefilled: B, or the leaders of a fork
        if extend:      # the positions behind the kept prefix: the face-count token (when the model has one), then BOS and the resume ids
            cond_embeds = dec.embed_num_face([quantize_num_faces(int(num_faces))] * N)[:, None, :] if self.dims.use_num_face_cond else None
        else:
            cond_embeds = self.encode_cond(conds, [num_faces] * N)["cond_embeds"]
        input_ids = torch.full((N, 1), opt.bos_token_id, dtype=torch.long)
        if resume_ids is not None:
            input_ids = torch.cat((input_ids, resume_ids.to("cpu", torch.long)), dim=1)
        tokens_embeds = self.mesh_decoder.model.embd(input_ids)
        inputs_embeds = torch.cat((cond_embeds, tokens_embeds), dim=1) if cond_embeds is not None else tokens_embeds
        fn = BuiltinGrammar(select_grammar(opt, tokenizer is not None), self.vocab_size, opt.eos_token_id)
        if fn.er_grammar == native.ER_GRAMMAR_NONE:
            print("[WARN] prefix_allowed_tokens_fn is not defined for meto backend:", opt.meto_backend)
            fn = None
        if num_faces < 0:
            num_tokens = torch.full((B,), -1, dtype=torch.long)
        else:
            num_tokens = torch.full((B,), num_faces * 4 + opt.num_cond_tokens, dtype=torch.long)
        kwargs = dict(inputs_embeds=inputs_embeds, num_tokens=num_tokens, pad_token_id=opt.pad_token_id,
                      bos_token_id=opt.bos_token_id, eos_token_id=opt.eos_token_id, max_new_tokens=max_new_tokens,
                      prefix_allowed_tokens_fn=fn, min_new_tokens=min_new_tokens, seed=seed, row_streams=row_streams)
        if fork is not None:
            kwargs["fork_leaders"] = fork[1]
        if extend:
            kwargs["extend_past"] = past
        if share_prefix and (B > 4 or os.environ.get("ER_FORCE_BATCHED", "")[:1] == "1"):
            kwargs["prefix_groups"] = (fork[1] if fork is not None else prefix_leaders(conds), opt.num_cond_tokens + 1)
            if isinstance(share_prefix, str):
                kwargs["prefix_pass"] = share_prefix
        if opt.generate_mode == "greedy":
            kwargs["num_beams"] = 1
        elif opt.generate_mode == "sample":
            kwargs["do_sample"] = True
            kwargs["top_k"] = 10 if top_k is None else top_k
        if temperature is not None:
            kwargs["temperature"] = temperature
        if top_p is not None:
            kwargs["top_p"] = top_p
        if top_k is not None and opt.generate_mode != "sample":
            kwargs["top_k"] = top_k          # checked like the others; greedy does not use it
        if output_logprobs:
            kwargs["output_logprobs"] = True
        self.last_logprobs = None
        rec.forget()                           # whatever happens in the call, the old record is not the cache's any more
        out = self.mesh_decoder.generate(**kwargs)
        self.last_logprobs = self.mesh_decoder.last_logprobs
        self.last_prefill = "extend" if extend else "full"
        if keep_cond and fork is None and not kwargs.get("prefix_groups"):      # every row holds its own cloud's prefix
            rec.remember(conds, B, past, id(dec), dec._reserved, dec.cache_epoch)
        if fork is not None:                   # back to the caller's row order: permuted place i holds the caller's row order[i]
            back = torch.empty(B, dtype=torch.long)
            back[torch.as_tensor(fork[0], dtype=torch.long)] = torch.arange(B)
            back = back.to(out.device)
            out = out[back]
            if self.last_logprobs is not None:
                self.last_logprobs = {k: v[back] for k, v in self.last_logprobs.items()}
        return out

    @torch.no_grad()
    def generate_queue(self, jobs, slots: int, tokenizer=None, max_new_tokens=None, min_new_tokens: int = 0,
                       seed: Optional[int] = None, clean=True, check_every: int = 0, *, temperature: Optional[float] = None,
                       top_p: Optional[float] = None, top_k: Optional[int] = None, output_logprobs: bool = False,
                       fork_repeats: bool = False):
        """Serves independent jobs from ``slots`` cache rows (continuous batching, ``er_queue_*``) -> ``(meshes, all_tokens)`` in job
        order, as ``generate`` returns them for one job each.  A job is ``(conds [N,3] or [1,N,3], num_faces, resume_ids=None,
        stream=None, max_new_tokens=None)``; clouds of different sizes, different face counts and resume lengths may be mixed.  A job
        leaves its slot when it emits EOS or reaches its budget and the next waiting job is prefilled into that slot, so - unlike a
        ``generate`` batch - no row rides on after its end.  ``all_tokens[j]`` has the job's own length (no PAD) with the resume
        prefix echoed; ``stream`` (default: the job's index) is the Philox stream of sample mode.  A job's ids are those of
        ``generate`` on that job alone (fp32; fp16: within one kernel class, slots <= 4 or slots > 4).  Afterwards
        ``last_queue_stats`` holds the ``er_queue_stats`` counters and ``last_queue_slots[j]`` the slot job j ran in.  The sampling
        controls and ``output_logprobs`` are those of ``generate_ids``; with ``output_logprobs=True`` ``last_queue_logprobs[j]`` is the
        pair (model, policy) of float32 numpy arrays over job j's generated tokens (its own length, the resume prefix not counted).
        ``fork_repeats=True``: jobs that are admitted together (one scheduler ``admit`` call) and whose (conds, num_faces, resume_ids)
        are bit-equal are prefilled once; the others start as copies of that job's row (``er_queue_admit_copy``) with their own stream
        and budget.  Every job's tokens and log-probs stay those of ``fork_repeats=False``; ``last_queue_stats["forked"]`` counts the
        rows admitted by copy (0 with the option off), ``last_queue_stats["admissions"]`` counts every job either way, and
        ``last_queue_admissions`` lists the scheduler's admit calls as (first slot, [job indices])."""
        from .meto import Engine, save_mesh
        from .queue import QueueScheduler
        opt = self.opt
        budget = opt.max_seq_length if max_new_tokens is None else int(max_new_tokens)
        jobs = [_QueueJob(j, spec, budget) for j, spec in enumerate(jobs)]
        self.last_queue_stats, self.last_queue_slots, self.last_queue_logprobs = {}, [], None
        self.last_queue_admissions = []        # the scheduler's admit calls in order: (first slot, [job indices])
        if not jobs:
            return [], []
        fn = BuiltinGrammar(select_grammar(opt, tokenizer is not None), self.vocab_size, opt.eos_token_id)
        if fn.er_grammar == native.ER_GRAMMAR_NONE:
            print("[WARN] prefix_allowed_tokens_fn is not defined for meto backend:", opt.meto_backend)
        do_sample = opt.generate_mode == "sample"
        if seed is None:      # as NativeShapeOPT._decode_device: the Philox key comes from torch's global CPU generator
            seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if do_sample else 0
        dec = self.mesh_decoder
        prefix = lambda j: opt.num_cond_tokens + 1 + (0 if j.resume is None else j.resume.shape[1])
        l_cap = max(prefix(j) + j.budget + 1 for j in jobs)
        dec.queue_begin(int(slots), l_cap, max(j.budget for j in jobs), min_new_tokens, do_sample, 10 if top_k is None else top_k,
                        fn.er_grammar, seed, check_every, 1.0 if temperature is None else temperature,
                        1.0 if top_p is None else top_p, output_logprobs)
        try:
            sched = QueueScheduler(int(slots))
            engine = _QueueEngine(self, jobs, output_logprobs, fork_repeats)
            ids = sched.serve(engine, len(jobs))
            if output_logprobs:
                self.last_queue_logprobs = [(lp[0], lp[1]) for _, lp in ids]
                ids = [i for i, _ in ids]
            self.last_queue_stats = dec.queue_stats()
            self.last_queue_stats["forked"] = engine.forked
            self.last_queue_slots = list(sched.slot_of)
            self.last_queue_admissions = [(s, list(j)) for s, j in sched.admissions]
        finally:
            dec.queue_end()
            dec.set_sampling()                 # the controls were the queue's: the context is back at its defaults
        meshes: List[Optional[object]] = []
        all_tokens: List[np.ndarray] = []
        for job, tokens in zip(jobs, ids):
            if job.resume is not None:
                tokens = np.concatenate((job.resume[0].numpy(), tokens), axis=0)
            if tokenizer is None or isinstance(tokenizer, Engine):
                meshes.append(save_mesh(tokens, opt, tokenizer=tokenizer, clean=clean))
            else:
                meshes.append(None)
            all_tokens.append(tokens)
        return meshes, all_tokens

    @torch.no_grad()
    def generate(self, conds, num_faces=1000, resume_ids=None, tokenizer=None, max_new_tokens=None, clean=True,
                 min_new_tokens: int = 0, seed: Optional[int] = None, row_streams=None, share_prefix=False, *,
                 temperature: Optional[float] = None, top_p: Optional[float] = None, top_k: Optional[int] = None,
                 output_logprobs: bool = False, fork_prefill: bool = False, keep_cond: bool = False):
        """-> (meshes, all_tokens) like core/models.py:204-319.  ``keep_cond``: see ``generate_ids``.  ``share_prefix``, ``fork_prefill``, the sampling controls and ``output_logprobs``
        (-> ``last_logprobs``, columns = the generated ids, without the resume prefix ``all_tokens`` echoes): see ``generate_ids``.  ``tokenizer`` is a
        ``edgerunner_amd.meto.Engine`` (or None for the 9-coordinate layout); each mesh is a
        ``edgerunner_amd.meto.Mesh`` - ``.vertices``, ``.faces``, ``.export(path)``, the members the reference's callers
        use of the trimesh objects it returns (trimesh itself is absent here); it still unpacks as ``v, f = mesh``."""
        output_ids = self.generate_ids(conds, num_faces, resume_ids, tokenizer, max_new_tokens, min_new_tokens, seed, row_streams, share_prefix,
                                       temperature=temperature, top_p=top_p, top_k=top_k, output_logprobs=output_logprobs,
                                       fork_prefill=fork_prefill, keep_cond=keep_cond)
        from .meto import Engine, save_mesh
        meshes: List[Optional[object]] = []
        all_tokens: List[np.ndarray] = []
        out = output_ids.detach().cpu().numpy()
        for b in range(out.shape[0]):
            tokens = out[b]
            if resume_ids is not None:
                tokens = np.concatenate((resume_ids[b].detach().cpu().numpy(), tokens), axis=0)
            # batch detokenize (core/models.py:315): a meto.Mesh instead of a trimesh object
            if tokenizer is None or isinstance(tokenizer, Engine):
                meshes.append(save_mesh(tokens, self.opt, tokenizer=tokenizer, clean=clean))
            else:
                meshes.append(None)      # opaque tokenizer marker (tests / benches): ids only
            all_tokens.append(tokens)
        return meshes, all_tokens
