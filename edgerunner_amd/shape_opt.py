"""``NativeShapeOPT`` - the MI355X-native stand-in for the reference's ``ShapeOPT``
(core/transformer/modeling_opt.py:429-550) at the seam ``LMM.generate`` uses:

    output_ids = self.mesh_decoder.generate(**kwargs)            core/models.py:303

It accepts the kwargs of core/models.py:286-301 (``inputs_embeds, num_tokens,
pad/bos/eos_token_id, max_new_tokens, prefix_allowed_tokens_fn, num_beams |
do_sample + top_k``) and returns the same ``LongTensor[B, T]`` of newly generated
ids.  All arithmetic runs in the HIP library behind the C ABI
(include/edgerunner_hip.h); this class only moves pointers.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Callable, Dict, Optional

import torch

from . import native
from .weights import ModelDims

_COND = {"none": native.ER_COND_NONE, "point": native.ER_COND_POINT, "point_latent": native.ER_COND_POINT_LATENT}
# storage dtypes of a context; "fp8" (or torch.float8_e4m3fn) = e4m3 bytes times 2^e per row for the six decoder matrices of a layer
# "fp4" = MXFP4 for the same matrices: e2m1 nibbles with an e8m0 scale byte per block of 32 along a row
_DT = {torch.float32: native.ER_F32, torch.float16: native.ER_F16, torch.bfloat16: native.ER_BF16, "fp8": native.ER_F8E4M3, "fp4": native.ER_F4E2M1}
if hasattr(torch, "float8_e4m3fn"):
    _DT[torch.float8_e4m3fn] = native.ER_F8E4M3


class BuiltinGrammar:
    """A ``prefix_allowed_tokens_fn`` the device understands.  Callable with the
    reference's signature (so host-side code can still use it) and tagged with the
    ``er_grammar`` enum the sampling-head kernel evaluates."""

    def __init__(self, er_grammar: int, vocab_size: int, eos_token_id: int = 2):
        from .grammar import as_callable
        self.er_grammar = er_grammar
        self._fn = as_callable(er_grammar, vocab_size, eos_token_id)

    def __call__(self, batch_id, input_ids):
        return self._fn(batch_id, input_ids) if self._fn is not None else None


_PE_MODES = {"embed": native.ER_PE_EMBED, "downsample": native.ER_PE_DOWNSAMPLE}


def point_encoder_mode_id(mode: str) -> int:
    if mode not in _PE_MODES:
        raise ValueError(f"point_encoder_mode={mode!r}: 'embed' or 'downsample'")
    return _PE_MODES[mode]


def check_clouds(points: torch.Tensor, dims) -> None:
    """The downsample encoder's preconditions on clouds [B, N, 3]: farthest point sampling picks point_latent_size points per cloud
    (the reference's ``.view(B, latent_size, 3)`` needs N >= point_latent_size) and its argmax needs finite coordinates.  The embed
    encoder reads any cloud, as before."""
    if getattr(dims, "point_encoder_mode", "embed") != "downsample":
        return
    if points.dim() != 3 or points.shape[-1] != 3:
        raise ValueError(f"point clouds must be [B, N, 3], got {tuple(points.shape)}")
    if points.shape[1] < dims.point_latent_size:
        raise ValueError(f"point_encoder_mode='downsample' samples point_latent_size={dims.point_latent_size} points per cloud; "
                         f"the clouds have {points.shape[1]} (use at least point_latent_size points, e.g. --point_num)")
    if not bool(torch.isfinite(points).all()):
        raise ValueError("point_encoder_mode='downsample': the point clouds hold non-finite coordinates")


def check_sampling(temperature, top_p, top_k) -> None:
    """The ranges ``er_set_sampling`` accepts, refused here with the argument's name."""
    import math
    if not (isinstance(temperature, (int, float)) and math.isfinite(temperature) and temperature > 0):
        raise ValueError(f"temperature={temperature!r}: a finite number > 0")
    if not (isinstance(top_p, (int, float)) and 0 < top_p <= 1):
        raise ValueError(f"top_p={top_p!r}: in (0, 1]")
    if int(top_k) != top_k or top_k < 0:
        raise ValueError(f"top_k={top_k!r}: an integer >= 0 (0: no top-k filter)")


class NativeShapeOPT:
    def __init__(self, dims: ModelDims, opt, device: torch.device, weight_dtype=torch.float32,
                 kv_dtype=torch.float32):
        if dims.cond_mode not in _COND:
            raise NotImplementedError(
                f"cond_mode={dims.cond_mode!r}: only the point / point_latent / none conditioners are on this path")
        self.dims, self.opt = dims, opt
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise native.NativeError("NativeShapeOPT needs a HIP device (cuda:N); there is no CPU fallback")
        self.lib = native.load_library()
        cfg = native.ErConfig(
            hidden_dim=dims.hidden_dim, num_heads=dims.num_heads, num_layers=dims.num_layers,
            intermediate_dim=dims.intermediate_dim, vocab_size=dims.vocab_size, max_positions=dims.max_positions,
            num_cond_tokens=dims.num_cond_tokens, point_hidden_dim=dims.point_hidden_dim,
            point_num_heads=dims.point_num_heads, point_latent_size=dims.point_latent_size,
            point_latent_dim=dims.point_latent_dim, point_freq_dim=dims.point_freq_dim,
            num_face_buckets=dims.num_face_buckets if dims.use_num_face_cond else 0,
            cond_mode=_COND[dims.cond_mode], pad_token_id=opt.pad_token_id, bos_token_id=opt.bos_token_id,
            eos_token_id=opt.eos_token_id, weight_dtype=_DT[weight_dtype], kv_dtype=_DT[kv_dtype], ln_eps=1e-5)
        self._ctx = C.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        native.check(self.lib.er_create(C.byref(cfg), idx, C.byref(self._ctx)), "er_create")
        if dims.cond_mode == "point":
            native.check(self.lib.er_set_point_encoder_mode(self._ctx, point_encoder_mode_id(dims.point_encoder_mode)),
                         "er_set_point_encoder_mode")
        self.stream = torch.cuda.Stream(device=self.device)
        self._reserved = (0, 0)
        # counts every call that rewrites the cache rows from position 0 (or may): what a caller that keeps a prefix for
        # ``prefill_extend`` compares to know that the prefix is still its own (LMM.generate_ids(keep_cond=True))
        self.cache_epoch = 0
        self.last_decode_ms = 0.0
        self.last_logprobs = None     # {"model", "policy"}: float32 [B, n] on the device after a generate(output_logprobs=True)
        # the prefix pass of the next grouping, as er_create read it (env ER_PREFIX_PASS; "mfma" holds on an fp16 cache only)
        self.prefix_pass = "mfma" if os.environ.get("ER_PREFIX_PASS") == "mfma" and kv_dtype == torch.float16 else "valu"
        self.direct_loads = False     # weights loaded on this object directly (LMM.half()/float() cannot replay them)

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx:
            self.lib.er_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- checkpoint --------------------------------------------------------------------------
    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = False):
        """Same keys as the reference checkpoint.  Returns the
        (missing, unexpected) lists like ``nn.Module.load_state_dict``."""
        self.direct_loads = True
        unexpected = []
        for key, t in sd.items():
            if not isinstance(t, torch.Tensor):
                continue
            self._load_one(key, t, unexpected)
        return self._finish_load(strict, unexpected)

    def load_state_iter(self, items, strict: bool = False):
        """Streaming variant (one tensor resident at a time)."""
        self.direct_loads = True
        unexpected = []
        for key, t in items:
            self._load_one(key, t, unexpected)
        return self._finish_load(strict, unexpected)

    def _load_one(self, key, t, unexpected):
        if native.load_tensor(self.lib.er_load_tensor, self._ctx, key, t) == 1:
            unexpected.append(key)

    def _finish_load(self, strict, unexpected):
        self.cache_epoch += 1                  # a cache written under other weights is nobody's prefix
        rc = self.lib.er_finalize_weights(self._ctx)
        missing = []
        if rc < 0:
            msg = self.lib.er_last_error().decode()
            if strict:
                raise native.NativeError(msg)
            missing.append(msg)
        if strict and unexpected:
            raise native.NativeError(f"unexpected keys: {unexpected[:5]}...")
        return missing, unexpected

    # -- plumbing ----------------------------------------------------------------------------
    def _enter(self):
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        return torch.cuda.stream(self.stream)

    def _exit(self):
        # inputs may have been allocated on the caller's stream: finish before they can be freed
        self.stream.synchronize()
        torch.cuda.current_stream(self.device).wait_stream(self.stream)

    def _sp(self):
        return C.c_void_p(self.stream.cuda_stream)

    def reserve(self, batch: int, max_len: int):
        native.check(self.lib.er_kv_reserve(self._ctx, batch, max_len), "er_kv_reserve")
        self._reserved = (batch, max_len)
        self.cache_epoch += 1

    # -- pieces of LMM.generate --------------------------------------------------------------
    def encode_cond(self, conds: Optional[torch.Tensor], face_buckets) -> torch.Tensor:
        d = self.dims
        B = len(face_buckets)
        n_points = 0
        if d.cond_mode != "none":
            conds = conds.to(self.device, torch.float32).contiguous()
            n_points = conds.shape[1]
            if d.cond_mode == "point":
                check_clouds(conds, d)
        with self._enter():
            out = torch.empty((B, d.num_cond_tokens, d.hidden_dim), dtype=torch.float32, device=self.device)
            native.check(self.lib.er_encode_cond(self._ctx, native.ptr(conds if d.cond_mode != "none" else None), B,
                                                 n_points, native.i32_array(face_buckets), native.ptr(out), self._sp()),
                         "er_encode_cond")
        self._exit()
        return out

    def embd(self, input_ids: torch.Tensor) -> torch.Tensor:
        ids = input_ids.detach().to("cpu", torch.int32).contiguous()
        B, R = ids.shape
        with self._enter():
            out = torch.empty((B, R, self.dims.hidden_dim), dtype=torch.float32, device=self.device)
            native.check(self.lib.er_embed_tokens(self._ctx, native.i32_array(ids.flatten().tolist()), B, R,
                                                  native.ptr(out), self._sp()), "er_embed_tokens")
        self._exit()
        return out

    def set_prefix_groups(self, prefix_groups=None):
        """``er_set_prefix_groups`` on the reserved batch: ``(leaders, prefix_len)`` with leaders[b] = the lowest row that shares row
        b's first prefix_len cache positions (b itself for a row of its own); None clears the groups."""
        if prefix_groups is None:
            native.check(self.lib.er_set_prefix_groups(self._ctx, None, 0, 0), "er_set_prefix_groups")
            return
        leaders, prefix_len = prefix_groups
        leaders = [int(v) for v in leaders]
        native.check(self.lib.er_set_prefix_groups(self._ctx, native.i32_array(leaders), len(leaders), int(prefix_len)),
                     "er_set_prefix_groups")

    def set_prefix_pass(self, prefix_pass: str):
        """``er_set_prefix_pass``: the kernel of the prefix pass under prefix groups, "valu" (the default) or "mfma" (the matrix-core
        pass: fp16 caches at head_dim 96, ER_ERR_UNSUPPORTED on any other context).  It takes effect at the next ``set_prefix_groups``."""
        if prefix_pass not in native.PREFIX_PASSES:
            raise ValueError(f"prefix_pass must be 'valu' or 'mfma', got {prefix_pass!r}")
        native.check(self.lib.er_set_prefix_pass(self._ctx, native.PREFIX_PASSES[prefix_pass]), "er_set_prefix_pass")
        self.prefix_pass = prefix_pass

    def prefill(self, inputs_embeds: torch.Tensor, max_new_tokens: int, prefix_groups=None, prefix_pass=None):
        """``prefix_groups``: None, or ``(leaders, prefix_len)`` as for set_prefix_groups - set (or cleared) after the lazy reserve and
        before the forward pass, which then checks on the device that the rows of a group hold the same prefix.  ``prefix_pass``
        ("valu" | "mfma"): the prefix pass of THIS grouping; the context's own setting (``set_prefix_pass``) is put back behind it."""
        x = inputs_embeds.to(self.device, torch.float32).contiguous()
        B, S, _ = x.shape
        self._reserve_and_group(B, S, max_new_tokens, prefix_groups, prefix_pass)
        with self._enter():
            native.check(self.lib.er_prefill(self._ctx, native.ptr(x), B, S, self._sp()), "er_prefill")
        self._exit()
        self.cache_epoch += 1

    def embed_num_face(self, buckets) -> torch.Tensor:
        """``er_embed_num_face``: rows of the embed_num_face table for ``buckets`` (``quantize_num_faces`` of the face counts) ->
        float32 [B, hidden] on the device: the token ``encode_cond`` appends behind the cloud's, without the point encoder."""
        buckets = [int(v) for v in buckets]
        with self._enter():
            out = torch.empty((len(buckets), self.dims.hidden_dim), dtype=torch.float32, device=self.device)
            native.check(self.lib.er_embed_num_face(self._ctx, native.i32_array(buckets), len(buckets), native.ptr(out), self._sp()),
                         "er_embed_num_face")
        self._exit()
        return out

    def prefill_extend(self, embeds_new: torch.Tensor, past_len: int):
        """``er_prefill_extend``: the forward pass over the ``embeds_new.shape[1]`` positions behind ``past_len`` cache positions that
        the last full or extending pass on this reservation wrote and that are kept.  The reservation is the caller's: the call never
        reserves (a new reservation has no past), so ``past_len + n_new`` plus what is to be decoded must fit the reserved length."""
        x = embeds_new.to(self.device, torch.float32).contiguous()
        B, n_new, _ = x.shape
        with self._enter():
            native.check(self.lib.er_prefill_extend(self._ctx, native.ptr(x), B, int(past_len), n_new, self._sp()), "er_prefill_extend")
        self._exit()
        self.cache_epoch += 1

    def _reserve_and_group(self, B, S, max_new_tokens, prefix_groups, prefix_pass):
        need = S + max_new_tokens + 1
        if self._reserved[0] != B or self._reserved[1] < need:
            self.reserve(B, need)
        if prefix_pass is None or prefix_groups is None:
            self.set_prefix_groups(prefix_groups)
        else:
            mine = self.prefix_pass
            self.set_prefix_pass(prefix_pass)
            try:
                self.set_prefix_groups(prefix_groups)
            finally:
                self.set_prefix_pass(mine)

    def prefill_fork(self, inputs_embeds: torch.Tensor, leaders, max_new_tokens: int, prefix_groups=None, prefix_pass=None):
        """``er_prefill_fork``: ``prefill`` for a batch of ``len(leaders)`` rows of which only the first ``inputs_embeds.shape[0]`` are
        distinct.  ``leaders`` is leaders-first (``leaders[b] == b`` for the rows that have embeds, the index of such a row behind them):
        the forward pass runs over the leaders alone and every other row receives its leader's cache rows and last hidden state as a
        copy.  ``prefix_groups`` / ``prefix_pass`` as for ``prefill``; groups must name the same leader table."""
        x = inputs_embeds.to(self.device, torch.float32).contiguous()
        n_leaders, S, _ = x.shape
        leaders = [int(v) for v in leaders]
        self._reserve_and_group(len(leaders), S, max_new_tokens, prefix_groups, prefix_pass)
        with self._enter():
            native.check(self.lib.er_prefill_fork(self._ctx, native.ptr(x), n_leaders, S, native.i32_array(leaders), len(leaders),
                                                  self._sp()), "er_prefill_fork")
        self._exit()
        self.cache_epoch += 1

    def logits(self) -> torch.Tensor:
        with self._enter():
            out = torch.empty((self._reserved[0], self.dims.vocab_size), dtype=torch.float32, device=self.device)
            native.check(self.lib.er_logits(self._ctx, native.ptr(out), self._sp()), "er_logits")
        self._exit()
        return out

    def score(self, inputs_embeds: torch.Tensor, labels: torch.Tensor, logits_out: Optional[torch.Tensor] = None,
              nll_out: Optional[torch.Tensor] = None, pred_out: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """ShapeOPT.forward(inputs_embeds, labels) in eval mode through ``er_score``: every layer over [B, S] positions, LN + lm_head
        over all of them, the shifted cross entropy.  ``labels`` int[B, S] as the reference's (unshifted, -100 = ignored).  The
        ``*_out`` tensors (contiguous, on the device) receive the results when given.  Returns nll [B, S], pred [B, S] (int32
        argmax), logits [B, S, V] or None (logits_out=False), loss float[2] = {mean NLL over supervised positions, count}.
        Leaves the cache as ``prefill`` does (positions [0, S))."""
        x = inputs_embeds.to(self.device, torch.float32).contiguous()
        B, S, _ = x.shape
        lab = labels.to(self.device, torch.int32).contiguous()
        if tuple(lab.shape) != (B, S):
            raise ValueError(f"labels {tuple(lab.shape)} do not match inputs_embeds [{B}, {S}]")
        if self._reserved[0] != B or self._reserved[1] < S + 1:
            self.reserve(B, S + 1)
        with self._enter():
            kw = dict(dtype=torch.float32, device=self.device)
            nll = nll_out if nll_out is not None else torch.empty((B, S), **kw)
            pred = pred_out if pred_out is not None else torch.empty((B, S), dtype=torch.int32, device=self.device)
            logits = None if logits_out is False else (logits_out if logits_out is not None
                                                        else torch.empty((B, S, self.dims.vocab_size), **kw))
            loss = torch.empty((2,), **kw)
            native.check(self.lib.er_score(self._ctx, native.ptr(x), native.ptr(lab), B, S, native.ptr(nll), native.ptr(pred),
                                           native.ptr(logits), native.ptr(loss), self._sp()), "er_score")
        self._exit()
        self.cache_epoch += 1
        return {"nll": nll, "pred": pred, "logits": logits, "loss": loss}

    def point_latent(self, conds: torch.Tensor):
        """PointEncoderEmbed's posterior.mode() [B, point_latent_size, point_latent_dim] and its kl() (0.5 * sum of squares over the
        whole batch, a 0-dim tensor) through ``er_point_latent``."""
        d = self.dims
        x = conds.to(self.device, torch.float32).contiguous()
        B, N = x.shape[0], x.shape[1]
        check_clouds(x, d)
        with self._enter():
            lat = torch.empty((B, d.point_latent_size, d.point_latent_dim), dtype=torch.float32, device=self.device)
            kl = torch.empty((1,), dtype=torch.float32, device=self.device)
            native.check(self.lib.er_point_latent(self._ctx, native.ptr(x), B, N, native.ptr(lat), native.ptr(kl), self._sp()),
                         "er_point_latent")
        self._exit()
        return lat, kl[0]

    def feed(self, ids):
        ids = [int(v) for v in (ids.flatten().tolist() if isinstance(ids, torch.Tensor) else ids)]
        with self._enter():
            native.check(self.lib.er_feed(self._ctx, native.i32_array(ids), self._sp()), "er_feed")
        self._exit()

    # -- the seam ----------------------------------------------------------------------------
    @torch.no_grad()
    def generate(self, inputs_embeds: torch.Tensor, num_tokens=None, pad_token_id=None, bos_token_id=None,
                 eos_token_id=None, max_new_tokens: Optional[int] = None,
                 prefix_allowed_tokens_fn: Optional[Callable] = None, num_beams: int = 1, do_sample: bool = False,
                 top_k: int = 50, min_new_tokens: int = 0, seed: Optional[int] = None, row_streams=None,
                 prefix_groups=None, temperature: float = 1.0, top_p: float = 1.0, output_logprobs: bool = False,
                 prefix_pass=None, fork_leaders=None, extend_past: Optional[int] = None, **unused) -> torch.Tensor:
        """Drop-in for ``ShapeOPT.generate`` as called at core/models.py:303.
        ``num_tokens`` is accepted and ignored exactly like the reference decoder
        ignores it (modeling_opt.py:324,467,546).  ``prefix_groups`` and ``prefix_pass`` go to ``prefill``.  ``fork_leaders``: a
        leaders-first table for a batch of ``len(fork_leaders)`` rows; ``inputs_embeds`` then holds the leaders only and the prefill is
        ``prefill_fork``.  ``extend_past``: ``inputs_embeds`` holds only the positions behind that many kept cache positions and
        the prefill is ``prefill_extend`` on the reservation as it stands (ValueError when it does not fit).

        ``temperature``, ``top_k`` (0: no top-k filter) and ``top_p`` act in sample mode, in the order of HF's warpers; greedy mode
        accepts them and picks the same ids.  ``output_logprobs=True`` leaves ``last_logprobs = {"model", "policy"}`` (float32
        [B, n] on the device, n = the id columns returned; ``er_set_sampling`` in include/edgerunner_hip.h defines both), otherwise
        ``last_logprobs`` is None.  With the defaults a call runs exactly the kernels it ran before the controls existed."""
        if num_beams != 1:
            raise NotImplementedError("beam search is not part of the reference's call (num_beams=1)")
        check_sampling(temperature, top_p, top_k)
        self.last_logprobs = None
        for name, got, want in (("pad", pad_token_id, self.opt.pad_token_id), ("bos", bos_token_id, self.opt.bos_token_id),
                                ("eos", eos_token_id, self.opt.eos_token_id)):
            if got is not None and got != want:
                raise ValueError(f"{name}_token_id={got} differs from the context's {want}")
        if max_new_tokens is None:
            max_new_tokens = self.opt.max_seq_length
        if extend_past is not None:
            if fork_leaders is not None or prefix_groups is not None:
                raise ValueError("extend_past combines with neither fork_leaders nor prefix_groups")
            B = inputs_embeds.shape[0]
            need = int(extend_past) + inputs_embeds.shape[1] + max_new_tokens + 1
            if self._reserved[0] != B or self._reserved[1] < need:
                raise ValueError(f"extend_past: the reservation {self._reserved} does not fit {B} rows of {need} positions")
            self.prefill_extend(inputs_embeds, extend_past)
        elif fork_leaders is None:
            B = inputs_embeds.shape[0]
            self.prefill(inputs_embeds, max_new_tokens, prefix_groups=prefix_groups, prefix_pass=prefix_pass)
        else:
            B = len(fork_leaders)
            self.prefill_fork(inputs_embeds, fork_leaders, max_new_tokens, prefix_groups=prefix_groups, prefix_pass=prefix_pass)
        # sample mode: the Philox stream of row b (default b; a sharding / batching caller passes global job indices)
        if row_streams is not None and len(row_streams) != B:
            raise ValueError(f"row_streams has {len(row_streams)} entries for a batch of {B}")
        arr = None if row_streams is None else (C.c_uint32 * B)(*[int(v) & 0xFFFFFFFF for v in row_streams])
        native.check(self.lib.er_set_row_streams(self._ctx, arr, B), "er_set_row_streams")
        if prefix_allowed_tokens_fn is None or isinstance(prefix_allowed_tokens_fn, BuiltinGrammar):
            grammar = native.ER_GRAMMAR_NONE if prefix_allowed_tokens_fn is None else prefix_allowed_tokens_fn.er_grammar
            return self._decode_device(B, max_new_tokens, min_new_tokens, do_sample, top_k, grammar, seed,
                                       temperature, top_p, output_logprobs)
        return self._decode_stepwise(B, max_new_tokens, min_new_tokens, do_sample, top_k, prefix_allowed_tokens_fn,
                                     temperature, top_p, output_logprobs)

    def set_sampling(self, temperature: float = 1.0, top_p: float = 1.0, top_k: Optional[int] = None, logprobs: bool = False):
        """``er_set_sampling``: sticky until the next call; all defaults restore the library's (``top_k=None`` leaves top-k to the
        decode parameters, 0 switches the filter off)."""
        check_sampling(temperature, top_p, 0 if top_k is None else top_k)
        if temperature == 1.0 and top_p == 1.0 and top_k is None and not logprobs:
            native.check(self.lib.er_set_sampling(self._ctx, None), "er_set_sampling")
            return
        s = native.ErSampling(temperature=float(temperature), top_p=float(top_p), top_k=int(top_k or 0),
                              top_k_set=0 if top_k is None else 1, logprobs=1 if logprobs else 0)
        native.check(self.lib.er_set_sampling(self._ctx, C.byref(s)), "er_set_sampling")

    def _decode_device(self, B, T, min_new, do_sample, top_k, grammar, seed, temperature=1.0, top_p=1.0, output_logprobs=False):
        # top_k > 0 travels in the decode parameters, as it always has; only "no filter" needs the controls' own field
        self.set_sampling(temperature, top_p, 0 if (do_sample and int(top_k) == 0) else None, output_logprobs)
        if seed is None:
            # the reference draws with torch.multinomial on the GLOBAL generator, which advances on every call:
            # repeated generate() calls give different samples and torch.manual_seed() reproduces a whole script.
            # Same contract here: the Philox key of this call is itself drawn from torch's global CPU generator.
            seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if do_sample else 0
        p = native.ErDecodeParams(mode=native.ER_SAMPLE if do_sample else native.ER_GREEDY, top_k=int(top_k),
                                  grammar=int(grammar), max_new_tokens=int(T), min_new_tokens=int(min_new),
                                  seed=int(seed) & 0xFFFFFFFFFFFFFFFF)
        n = C.c_int32(0)
        with self._enter():
            out = torch.empty((B, T), dtype=torch.int64, device=self.device)
            native.check(self.lib.er_decode(self._ctx, C.byref(p), native.ptr(out), C.byref(n), self._sp()), "er_decode")
        self._exit()
        ms = C.c_float(0)
        self.lib.er_last_decode_ms(self._ctx, C.byref(ms))
        self.last_decode_ms = float(ms.value)
        if output_logprobs:
            with self._enter():
                lp = torch.empty((2, B, n.value), dtype=torch.float32, device=self.device)
                native.check(self.lib.er_get_logprobs(self._ctx, native.ptr(lp[0]), native.ptr(lp[1]), n.value, n.value, self._sp()),
                             "er_get_logprobs")
            self._exit()
            self.last_logprobs = {"model": lp[0], "policy": lp[1]}
        return out[:, : n.value]

    def _decode_stepwise(self, B, T, min_new, do_sample, top_k, fn, temperature=1.0, top_p=1.0, output_logprobs=False):
        """Arbitrary host callable: logits come back every step (like the reference's
        host loop); the forward passes still run in the HIP library.  Temperature, top-k (0: none) and top-p mean what they mean
        to the device head, and the same two log-probs are kept."""
        eos, pad = self.opt.eos_token_id, self.opt.pad_token_id
        ids = torch.empty((B, 0), dtype=torch.long)
        unfinished = torch.ones(B, dtype=torch.long)
        lp_model, lp_policy = [], []
        for t in range(T):
            s = self.logits().float().cpu()
            raw_lsm = torch.log_softmax(s, dim=-1) if output_logprobs else None
            if t < min_new:
                s[:, eos] = -float("inf")
            mask = torch.full_like(s, -float("inf"))
            for b in range(B):
                allowed = fn(b, ids[b])
                if len(allowed) == 0:
                    raise ValueError(f"`prefix_allowed_tokens_fn` returned an empty list for batch ID {b}.")
                mask[b, allowed] = 0
            s = s + mask
            if do_sample:
                s = s / temperature
                if top_k > 0:
                    k = min(top_k, s.shape[-1])
                    kth = torch.topk(s, k)[0][..., -1, None]
                    s = s.masked_fill(s < kth, -float("inf"))
                if top_p < 1.0:      # TopPLogitsWarper, min_tokens_to_keep=1: keep while the mass strictly ahead is < top_p
                    srt, order = torch.sort(s, dim=-1, descending=True, stable=True)
                    probs = torch.softmax(srt, dim=-1)
                    drop = (probs.cumsum(dim=-1) - probs) >= top_p
                    drop[..., 0] = False
                    s = s.masked_fill(drop.scatter(-1, order, drop), -float("inf"))
                nxt = torch.multinomial(torch.softmax(s, dim=-1), 1).squeeze(1)
            else:
                nxt = torch.argmax(s, dim=-1)
            if output_logprobs:
                live = unfinished.float()
                lp_model.append(raw_lsm.gather(-1, nxt[:, None]).squeeze(1) * live)
                lp_policy.append(torch.log_softmax(s, dim=-1).gather(-1, nxt[:, None]).squeeze(1) * live)
            nxt = nxt * unfinished + pad * (1 - unfinished)
            ids = torch.cat([ids, nxt[:, None]], dim=-1)
            unfinished = unfinished & (nxt != eos).long()
            if unfinished.max() == 0 or t == T - 1:
                break
            self.feed(nxt)
        if output_logprobs:
            self.last_logprobs = {"model": torch.stack(lp_model, dim=1).to(self.device, torch.float32),
                                  "policy": torch.stack(lp_policy, dim=1).to(self.device, torch.float32)}
        return ids.to(self.device)

    # -- queue mode (continuous batching): thin bindings of er_queue_* -------------------------
    def queue_begin(self, slots: int, l_cap: int, max_new_tokens: int, min_new_tokens: int = 0, do_sample: bool = False,
                    top_k: int = 10, grammar: int = native.ER_GRAMMAR_NONE, seed: int = 0, check_every: int = 0,
                    temperature: float = 1.0, top_p: float = 1.0, output_logprobs: bool = False):
        """Reserves ``slots`` cache rows of ``l_cap`` positions and opens the queue on them (every row parked).  The sampling controls
        and ``output_logprobs`` are those of ``generate``; they hold for the whole queue (``queue_row_logprobs``)."""
        if self._reserved[0] != slots or self._reserved[1] < l_cap:
            self.reserve(slots, l_cap)
        self.set_sampling(temperature, top_p, 0 if (do_sample and int(top_k) == 0) else None, output_logprobs)
        p = native.ErDecodeParams(mode=native.ER_SAMPLE if do_sample else native.ER_GREEDY, top_k=int(top_k), grammar=int(grammar),
                                  max_new_tokens=int(max_new_tokens), min_new_tokens=int(min_new_tokens),
                                  seed=int(seed) & 0xFFFFFFFFFFFFFFFF)
        with self._enter():
            native.check(self.lib.er_queue_begin(self._ctx, C.byref(p), int(check_every), self._sp()), "er_queue_begin")
        self._exit()
        self.cache_epoch += 1

    def queue_admit(self, row0: int, inputs_embeds: torch.Tensor, stream_ids=None, budgets=None):
        """Prefills rows [row0, row0 + n) from ``inputs_embeds`` [n, S, hidden] in one forward pass and starts their jobs."""
        x = inputs_embeds.to(self.device, torch.float32).contiguous()
        n, S, _ = x.shape
        ids = None if stream_ids is None else (C.c_uint32 * n)(*[int(v) & 0xFFFFFFFF for v in stream_ids])
        bud = None if budgets is None else native.i32_array(budgets)
        if (ids is not None and len(stream_ids) != n) or (bud is not None and len(budgets) != n):
            raise ValueError(f"queue_admit: {n} rows need {n} stream ids / budgets")
        with self._enter():
            native.check(self.lib.er_queue_admit(self._ctx, int(row0), n, native.ptr(x), S, ids, bud, self._sp()), "er_queue_admit")
        self._exit()

    def queue_admit_copy(self, src_row: int, dst_rows, stream_ids=None, budgets=None):
        """``er_queue_admit_copy``: starts jobs in the free rows ``dst_rows`` as copies of the fresh job in ``src_row`` (admitted and
        not yet stepped): its cache rows and last hidden state, with stream ids and budgets of their own."""
        dst = [int(v) for v in dst_rows]
        n = len(dst)
        if (stream_ids is not None and len(stream_ids) != n) or (budgets is not None and len(budgets) != n):
            raise ValueError(f"queue_admit_copy: {n} rows need {n} stream ids / budgets")
        ids = None if stream_ids is None else (C.c_uint32 * n)(*[int(v) & 0xFFFFFFFF for v in stream_ids])
        bud = None if budgets is None else native.i32_array(budgets)
        with self._enter():
            native.check(self.lib.er_queue_admit_copy(self._ctx, int(src_row), native.i32_array(dst), n, ids, bud, self._sp()),
                         "er_queue_admit_copy")
        self._exit()

    def queue_run(self):
        """Replays the step until a job is done: the rows of all done jobs ([] when no row is occupied)."""
        rows = (C.c_int32 * max(1, self._reserved[0]))()
        n = C.c_int32(0)
        with self._enter():
            native.check(self.lib.er_queue_run(self._ctx, rows, C.byref(n), self._sp()), "er_queue_run")
        self._exit()
        return [int(rows[i]) for i in range(n.value)]

    def queue_take(self, row: int, capacity: int):
        """The finished job's ids (int64 numpy array of its own length, no PAD); the row is free afterwards."""
        import numpy as np
        buf = np.empty((max(1, int(capacity)),), dtype=np.int64)
        n = C.c_int32(0)
        native.check(self.lib.er_queue_take(self._ctx, int(row), buf.ctypes.data_as(C.POINTER(C.c_int64)), int(capacity), C.byref(n)),
                     "er_queue_take")
        return buf[: n.value].copy()

    def queue_row_logprobs(self, row: int, capacity: int):
        """(model, policy) float32 numpy arrays of the finished job in ``row``, of the job's own length; call it before ``queue_take``."""
        import numpy as np
        cap = max(1, int(capacity))
        buf = np.zeros((2, cap), dtype=np.float32)
        f32p = C.POINTER(C.c_float)
        native.check(self.lib.er_queue_row_logprobs(self._ctx, int(row), buf[0].ctypes.data_as(f32p), buf[1].ctypes.data_as(f32p), cap),
                     "er_queue_row_logprobs")
        return buf

    def queue_stats(self) -> Dict[str, float]:
        s = native.ErQueueCounters()
        native.check(self.lib.er_queue_stats(self._ctx, C.byref(s)), "er_queue_stats")
        return {n: (float if n.endswith("_ms") else int)(getattr(s, n)) for n, _ in native.ErQueueCounters._fields_}

    def queue_end(self):
        native.check(self.lib.er_queue_end(self._ctx), "er_queue_end")

    def plan(self):
        """Kernel selection of THIS context for its reserved cache (``er_ctx_plan``): dict of the ``er_decode_plan`` fields."""
        p = native.ErDecodePlan()
        native.check(self.lib.er_ctx_plan(self._ctx, C.byref(p)), "er_ctx_plan")
        return {n: int(getattr(p, n)) for n, _ in native.ErDecodePlan._fields_}

    def w8_streams(self):
        """fp8 mode: which projections the reserved shape's decode step streams as e4m3 bytes (``er_ctx_w8_streams``): dict of 0 / 1 for
        qkv, out_proj, fc1 and fc2.  All zero in the other precisions."""
        out = (C.c_int32 * 4)()
        native.check(self.lib.er_ctx_w8_streams(self._ctx, out), "er_ctx_w8_streams")
        return dict(zip(("qkv", "out_proj", "fc1", "fc2"), (int(v) for v in out)))

    def w4_streams(self):
        """fp4 mode: which projections the reserved shape's decode step streams as e2m1 nibbles (``er_ctx_w4_streams``): dict of 0 / 1 for
        qkv, out_proj, fc1 and fc2.  All zero in the other precisions."""
        out = (C.c_int32 * 4)()
        native.check(self.lib.er_ctx_w4_streams(self._ctx, out), "er_ctx_w4_streams")
        return dict(zip(("qkv", "out_proj", "fc1", "fc2"), (int(v) for v in out)))

    def w4_streams_batched(self):
        """fp4 mode: which projections the reserved shape's batched decode step (batch > 4) streams as e2m1 nibbles in their matrix-core
        forms (``er_ctx_w4_streams_batched``; ``ER_W4_BATCHED`` at creation: 0 / 1 / unset = the measured rule): dict of 0 / 1 for qkv,
        out_proj, fc1 and fc2.  All zero in the other precisions and for single-row shapes; ``w4_streams`` reports the row forms only."""
        out = (C.c_int32 * 4)()
        native.check(self.lib.er_ctx_w4_streams_batched(self._ctx, out), "er_ctx_w4_streams_batched")
        return dict(zip(("qkv", "out_proj", "fc1", "fc2"), (int(v) for v in out)))

    def mlp_nnz(self):
        """Live fc1 neurons per (layer, workgroup) that the fused single-row MLP counted in the last decode step (``er_mlp_nnz``):
        int32 [num_layers, 256], each 0 .. 24.  Raises unless the reserved shape runs the fused MLP (one row, ``ER_MLP_V`` on)."""
        import numpy as np
        n = int(self.dims.num_layers) * 256
        buf = np.empty((n,), dtype=np.int32)
        native.check(self.lib.er_mlp_nnz(self._ctx, buf.ctypes.data_as(C.POINTER(C.c_int32)), n), "er_mlp_nnz")
        return buf.reshape(-1, 256)

    # -- measurement -------------------------------------------------------------------------
    def profile_decode_kernels(self, repeats: int = 5, context_len: int = 0, use_graph: bool = False):
        """Per-kind average launch duration (HIP events on the launch stream) and algorithmic bytes per launch.
        context_len > 0: the attention kernels run over that many keys (default: the current context length);
        use_graph: the 24 launches of a kind are replayed from a hipGraph, as the generation loop does."""
        us = (C.c_float * native.ER_NUM_KERNEL_KINDS)()
        by = (C.c_double * native.ER_NUM_KERNEL_KINDS)()
        with self._enter():
            native.check(self.lib.er_profile_decode_kernels_at(self._ctx, repeats, int(context_len), 1 if use_graph else 0, us, by,
                                                               self._sp()), "er_profile")
        self._exit()
        return {self.lib.er_kernel_kind_name(k).decode(): {"avg_us": float(us[k]), "bytes": float(by[k])}
                for k in range(native.ER_NUM_KERNEL_KINDS)}
