#!/usr/bin/env python3
"""Drop-in for the reference's ``infer.py`` (point-conditioned ArAE inference) on MI355X.

    python infer.py ArAE --workspace out --resume model.safetensors --test_path mesh_or_dir \
        --generate_mode greedy --test_num_face 1000 --test_repeat 1 --seed 0

Same flags (``edgerunner_amd.options`` mirrors ``core/options.py``), same outputs
(``{name}_{i}_{n}f_tokens.npy`` = ids-3 cut at EOS, ``{name}_pc.obj``; reference infer.py:86-123).
Inputs: .obj/.ply meshes (surface-sampled to ``point_num`` points) or .npy point clouds [N,3].
Difference from the reference on MESH inputs: reference infer.py:86 first runs ``kiui.mesh_utils.clean_mesh(v, f, min_f=0, min_d=0,
remesh=False)`` (pymeshlab filters - both packages absent here and not restated) and samples with ``trimesh.sample``; this script
normalises the mesh as loaded and uses its own seeded area-weighted sampler, so the conditioning cloud is a different sample of the
same surface.  ``.npy`` clouds are passed through untouched (identical conditions for both code bases).  Meshes are written with
``mesh.export(...)`` on the ``edgerunner_amd.meto.Mesh`` objects generate() returns (reference infer.py:120 on trimesh objects).
``--cond_mode none`` (reference infer.py:96-97) generates from the face-count token alone, once per input path.
With torchrun (one process per GPU) the (file x repeat x num_face) jobs are sharded block-cyclically over ranks;
inside a rank, jobs with the same face count run as ONE batched generate() call (the B > 1 decode path streams the
weights once for all rows), and the generated token streams are all-gathered over RCCL at the end
(``{workspace}/tokens_all.npz`` on rank 0).

Reproducibility: in sample mode job j (its index in the reference's loop order) draws from the Philox stream
(--seed, step, j), whatever the world size, ER_INFER_BATCH or free memory made of the grouping.  In the fp16 (default) precision
the projections of calls with more than 4 rows run on the matrix cores and round differently from the 1..4-row kernels
(both within 1e-5 of the fp16-storage model), so a near-tie can still resolve differently when the grouping changes;
EDGERUNNER_PRECISION=fp32 with ER_INFER_BATCH <= 4 (or any fixed grouping) is bit-reproducible.

ER_INFER_QUEUE=1 serves the rank's jobs through ``LMM.generate_queue`` instead: one set of min(ER_INFER_BATCH, jobs) cache rows for
all face counts, a job leaves its row when it emits EOS and the next job is prefilled into that row, so no row rides on to the end
of the longest job of its call.  Same output files and ``tokens_all.npz``; the log line of a job carries its own token count and
the row it ran in.  Without the variable nothing changes.

ER_INFER_SHARE_PREFIX=1 passes ``share_prefix=True`` to the batched path's ``LMM.generate`` calls: the jobs of one call that come from
the same cloud (--test_repeat samples of one input) read their common cond + BOS prefix once per decode step instead of once per job
(calls of more than 4 jobs; see ``LMM.generate_ids``).  Same output files.  It cannot be combined with ER_INFER_QUEUE=1 (the queue's
rows change owners; groups in queue mode are not built): both together are refused at start.  Without the variable nothing changes.
ER_INFER_PREFIX_PASS=mfma beside it passes ``share_prefix="mfma"``: the shared prefix is read by the matrix-core prefix pass (fast mode's
fp16 cache only; ``LMM.generate_ids``).  Alone, or with any other value than ``mfma``, it does nothing.

ER_INFER_FORK_PREFILL=1 encodes and prefills every distinct input of a call once and starts its repeats (--test_repeat samples of one
cloud at one face count) from a copy of that row's cache (``LMM.generate(fork_prefill=True)``; in queue mode
``LMM.generate_queue(fork_repeats=True)``, for repeats that are admitted together).  Same output files; it combines with every other
variable here.  Without the variable nothing changes.

ER_INFER_KEEP_COND=1 orders the rank's calls so that the face counts of one set of clouds follow each other
(``edgerunner_amd.dist.group_jobs_keep_cond``) and passes ``keep_cond=True``: the first call of a set runs the point encoder and the full
prefill, the others prefill only the face-count token and BOS behind the kept cond positions (``LMM.generate_ids``).  Every call
reserves for --test-max-seq-length, so one reservation serves all face counts.  Same output files.  It cannot be combined with
ER_INFER_QUEUE=1, ER_INFER_SHARE_PREFIX=1 or ER_INFER_FORK_PREFILL=1 (refused at start).  Without the variable nothing changes.

ER_INFER_TEMPERATURE, ER_INFER_TOP_P and ER_INFER_TOP_K (0: no top-k filter) shape the draws of ``--generate_mode sample`` as HF's
warpers do, in that order; unset, the reference's TopK(10) at temperature 1 stays.  ER_INFER_LOGPROBS=1 writes
``{name}_{i}_{n}f_logprobs.npy`` beside every tokens file: float32 [n, 2], one row per token of the tokens file (cut at EOS the same way),
columns = the model's log-probability of the token and its log-probability under the distribution it was drawn from
(``LMM.generate_ids``); the log line of a job carries the sum of the model column.  Batch, queue and share-prefix mode alike.  A value
that does not parse or is out of range ends the run with the variable's name.  Without the variables nothing changes.
"""
from __future__ import annotations

import glob
import os
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from edgerunner_amd import dist as D  # noqa: E402
from edgerunner_amd import meshio  # noqa: E402
from edgerunner_amd.models import LMM  # noqa: E402
from edgerunner_amd.options import parse_cli  # noqa: E402
from edgerunner_amd.meto import get_tokenizer  # noqa: E402
from edgerunner_amd.utils import seed_everything, trim_tokens  # noqa: E402


def sampling_from_env(env=None) -> dict:
    """The keyword arguments ER_INFER_TEMPERATURE / ER_INFER_TOP_P / ER_INFER_TOP_K / ER_INFER_LOGPROBS add to ``LMM.generate`` and
    ``LMM.generate_queue`` ({} when none is set).  A bad value ends with SystemExit naming the variable."""
    env = os.environ if env is None else env
    out = {}

    def read(name, conv, ok, want):
        raw = env.get(name)
        if raw is None or raw == "":
            return None
        try:
            v = conv(raw)
        except ValueError:
            v = None
        if v is None or not ok(v):
            raise SystemExit(f"[ERROR] {name}={raw!r}: {want}")
        return v

    t = read("ER_INFER_TEMPERATURE", float, lambda v: np.isfinite(v) and v > 0, "a finite number > 0")
    p = read("ER_INFER_TOP_P", float, lambda v: 0 < v <= 1, "a number in (0, 1]")
    k = read("ER_INFER_TOP_K", int, lambda v: v >= 0, "an integer >= 0 (0: no top-k filter)")
    lp = read("ER_INFER_LOGPROBS", int, lambda v: v in (0, 1), "0 or 1")
    if t is not None:
        out["temperature"] = t
    if p is not None:
        out["top_p"] = p
    if k is not None:
        out["top_k"] = k
    if lp:
        out["output_logprobs"] = True
    return out


def load_points(opt, path):
    """One cloud per input path, reused for every repeat and face count (reference infer.py:84-92).  The surface
    sampler is seeded by (opt.seed, path) so that every rank - and a world-size-1 run - derives the same cloud."""
    if opt.cond_mode == "none":                      # reference infer.py:96-97: a [1, 0] dummy that only carries the batch size
        return np.zeros((0, 3), dtype=np.float32)
    if path.endswith(".npy"):
        return np.load(path).astype(np.float32).reshape(-1, 3)
    rng = np.random.default_rng([int(opt.seed) & 0xFFFFFFFF, zlib.crc32(os.path.basename(path).encode())])
    v, f = meshio.load_mesh(path)
    v = meshio.normalize_mesh(v, bound=0.95)
    return meshio.sample_surface(v, f, opt.point_num, rng).astype(np.float32)


def max_rows_per_call(opt, model, max_new_tokens, device) -> int:
    """How many independent jobs one generate() call carries: ER_INFER_BATCH (default 32 = one pass of the batched
    projections) - a fixed number, so the grouping does not depend on what else occupies the device.  Memory is only a guard:
    the rows' KV cache + prefill / encoder scratch must fit in the HBM that is free once the weights are resident (the native
    context is created here, before the measurement)."""
    d = model.dims
    esz = 4 if model.precision == "fp32" else 1 if model.kv_precision == "fp8" else 2      # fp16 and fp8 keep an fp16 cache unless EDGERUNNER_KV_PRECISION=fp8
    l_cap = d.num_cond_tokens + 2 + max_new_tokens
    kv_row = 2 * d.num_layers * d.hidden_dim * esz * l_cap
    scratch_row = (d.num_cond_tokens + 1) * (6 * d.hidden_dim + d.intermediate_dim) * 4
    if d.cond_mode == "point":                       # encoder scratch per sample at point_num points (K / V / x rows + the GEGLU buffers)
        scratch_row += (3 * opt.point_num + 14 * d.point_latent_size) * d.point_hidden_dim * 4
        if d.point_encoder_mode == "downsample":     # per-sample query rows (gathered, ln1, q_proj) and the sampling indices
            scratch_row += 3 * d.point_latent_size * d.point_hidden_dim * 4 + d.point_latent_size * 4
    _ = model.mesh_decoder                           # materialise the context: the weights are on the device from here on
    free, _total = torch.cuda.mem_get_info(device)
    cap = max(1, int(os.environ.get("ER_INFER_BATCH", "32")))
    fit = int(0.8 * free // (kv_row + scratch_row))
    if fit < 1:
        raise SystemExit(f"[ERROR] not enough free HBM for one job: {free / 2**30:.1f} GiB free, one row needs "
                         f"{(kv_row + scratch_row) / 2**30:.1f} GiB (lower --test_max_seq_length)")
    if fit < cap:
        print(f"[WARN] {free / 2**30:.1f} GiB free: {fit} jobs per call instead of {cap} (sample-mode results are unaffected, "
              "fp16 greedy near-ties may resolve differently - see the module docstring)")
    return min(cap, fit)


def main(argv=None):
    opt = parse_cli(argv)
    sampling = sampling_from_env()
    share_prefix = os.environ.get("ER_INFER_SHARE_PREFIX") == "1"
    fork_prefill = os.environ.get("ER_INFER_FORK_PREFILL") == "1"
    if share_prefix and os.environ.get("ER_INFER_PREFIX_PASS") == "mfma":
        share_prefix = "mfma"
    if share_prefix and os.environ.get("ER_INFER_QUEUE") == "1":
        raise SystemExit("[ERROR] ER_INFER_SHARE_PREFIX=1 and ER_INFER_QUEUE=1 cannot be combined: prefix groups are not built for queue mode")
    if share_prefix and os.environ.get("EDGERUNNER_KV_PRECISION") == "fp8":
        raise SystemExit("[ERROR] ER_INFER_SHARE_PREFIX=1 and EDGERUNNER_KV_PRECISION=fp8 cannot be combined: the shared-prefix kernels read fp32 and fp16 caches only")
    keep_cond = os.environ.get("ER_INFER_KEEP_COND") == "1"
    if keep_cond and (share_prefix or fork_prefill or os.environ.get("ER_INFER_QUEUE") == "1"):
        raise SystemExit("[ERROR] ER_INFER_KEEP_COND=1 cannot be combined with ER_INFER_QUEUE=1, ER_INFER_SHARE_PREFIX=1 or ER_INFER_FORK_PREFILL=1: "
                         "the prefill behind a kept cond prefix is built for plain batched calls")
    rank, world, local = D.init_process_group()
    seed_everything(opt.seed)
    if opt.cond_mode not in ("point", "none"):
        raise SystemExit("infer.py serves cond_mode='point' (ArAE preset) and 'none'; see infer_dit.py for the image -> point_latent path")
    if opt.cond_mode == "point" and opt.point_encoder_mode == "downsample" and opt.point_num < opt.point_latent_size:
        raise SystemExit(f"[ERROR] point_encoder_mode=downsample samples point_latent_size={opt.point_latent_size} points per cloud: "
                         f"--point_num {opt.point_num} is too small")
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device visible: this path has no CPU fallback")
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    # module style: storage precision follows .half() / .float(); EDGERUNNER_KV_PRECISION=fp8 stores the KV cache as e4m3 bytes (fp16 / fp8 weights only)
    model = LMM(opt, device, precision=None, kv_precision=os.environ.get("EDGERUNNER_KV_PRECISION") or None)
    if opt.resume is not None:
        if opt.resume.endswith("safetensors"):
            from safetensors.torch import load_file
            ckpt = load_file(opt.resume, device="cpu")
        else:
            ckpt = torch.load(opt.resume, map_location="cpu")
        model.load_state_dict(ckpt, strict=False)
        print(f"[INFO] Loaded checkpoint from {opt.resume}")
    else:
        from edgerunner_amd import weights as W
        print("[WARN] model randomly initialized, are you sane?")
        model.load_state_dict(W.make_state_dict(opt, opt.seed, "reference"), strict=True)
    # the reference runs fp16 on the GPU (infer.py:56,105): .half() selects the fp16-storage context (fp32 accumulate);
    # EDGERUNNER_PRECISION=fp32 keeps the exact mode (greedy ids bit-exact vs the CPU path), fp8 selects e4m3 row-scaled decoder matrices
    if os.environ.get("EDGERUNNER_PRECISION", "fp16") == "fp32":
        model = model.float().eval().to(device)
    elif os.environ.get("EDGERUNNER_PRECISION") == "fp8":
        model = model.fp8().eval().to(device)
    elif os.environ.get("EDGERUNNER_PRECISION") in ("fp4", "mxfp4"):      # MXFP4 decoder matrices (e2m1 nibbles, one e8m0 scale per block of 32); ER_W4_ROWS / ER_W4_BATCHED = 0 / 1 force the nibble kernels of the single-row / batched step off / on
        model = model.fp4().eval().to(device)
    else:
        model = model.half().eval().to(device)
    model.release_checkpoint()        # the weights are on the device in their final precision: drop the host copy (~2.7 GB per rank)
    ckpt = None

    tokenizer, _ = get_tokenizer(opt)

    assert opt.test_path is not None
    paths = sorted(glob.glob(os.path.join(opt.test_path, "*"))) if os.path.isdir(opt.test_path) else [opt.test_path]
    os.makedirs(opt.workspace, exist_ok=True)
    # the reference's serial loops (infer.py:99-101,136-137): path x repeat x num_face, here sharded block-cyclically over
    # ranks and, inside a rank, batched through the B > 1 decode path (rows are independent)
    jobs, mine, pc_owner = D.plan_jobs(paths, opt.test_repeat, opt.test_num_face, rank, world)
    clouds = {}
    for j in mine:
        path = jobs[j][0]
        if path not in clouds:
            clouds[path] = load_points(opt, path)
    for path in paths:                               # exactly one rank exports the cloud of a path
        if pc_owner[path] == rank and opt.cond_mode == "point":
            if path not in clouds:
                clouds[path] = load_points(opt, path)
            name = os.path.splitext(os.path.basename(path))[0]
            meshio.save_points_obj(f"{opt.workspace}/{name}_pc.obj", clouds[path])
    rows_max = max_rows_per_call(opt, model, opt.test_max_seq_length, device)
    local_streams = {}

    def save_job(j, mesh, tokens, note, logprobs=None):
        path, i, num_faces = jobs[j]
        name = os.path.splitext(os.path.basename(path))[0]
        toks = trim_tokens(tokens)
        filename = f"{name}_{i}" + (f"_{num_faces}f" if opt.use_num_face_cond else "")
        np.save(f"{opt.workspace}/{filename}_tokens.npy", toks)
        if logprobs is not None:      # (model, policy) over the generated ids: the rows of the tokens the file above holds
            lp = np.stack([np.asarray(logprobs[0], dtype=np.float32)[: len(toks)], np.asarray(logprobs[1], dtype=np.float32)[: len(toks)]], axis=1)
            np.save(f"{opt.workspace}/{filename}_logprobs.npy", lp)
            note = f"{note}, model log-prob {float(lp[:, 0].sum()):.4f}"
        if mesh is not None:
            mesh.export(f"{opt.workspace}/{filename}.ply")               # reference infer.py:120
        local_streams[j] = toks
        print(f"[INFO] Processing {path} --> {filename}.ply, {len(toks)} tokens, {note}")

    if os.environ.get("ER_INFER_QUEUE") == "1" and mine:
        # queue mode: all of the rank's jobs, whatever their face counts, share one set of cache rows; a job leaves its row at its
        # own EOS and the next job takes the row (LMM.generate_queue).  Stream id = global job index, as in the batched path.
        slots = min(rows_max, len(mine))
        specs = [(torch.from_numpy(clouds[jobs[j][0]]).float(), jobs[j][2], None, j) for j in mine]
        t0 = time.time()
        meshes, tokens = model.generate_queue(specs, slots, tokenizer=tokenizer, max_new_tokens=opt.test_max_seq_length,
                                              clean=True, seed=opt.seed, **({"fork_repeats": True} if fork_prefill else {}), **sampling)
        torch.cuda.synchronize()
        dt = time.time() - t0
        st = model.last_queue_stats
        qlp = model.last_queue_logprobs
        for r, j in enumerate(mine):
            save_job(j, meshes[r], tokens[r], f"{len(tokens[r])} generated, slot {model.last_queue_slots[r]} of {slots}",
                     None if qlp is None else qlp[r])
        print(f"[INFO] queue: {len(mine)} jobs on {slots} slots in {dt:.4f}s, {st['steps']} steps, {st['occupied_row_steps']} occupied / "
              f"{st['wait_row_steps']} waiting / {st['parked_row_steps']} parked row-steps, prefill {st['prefill_ms']:.1f} ms, "
              f"decode {st['decode_ms']:.1f} ms")
        mine_groups = []
    else:
        mine_groups = (D.group_jobs_keep_cond if keep_cond else D.group_jobs)(jobs, mine, lambda p: clouds[p].shape[0], rows_max)
    for num_faces, chunk in mine_groups:
        cond = torch.from_numpy(np.stack([clouds[jobs[j][0]] for j in chunk])).float().to(device)
        t0 = time.time()
        # sample mode: job j draws from the Philox stream (opt.seed, step, j) whatever rows share its call
        meshes, tokens = model.generate(cond, num_faces=num_faces, max_new_tokens=opt.test_max_seq_length,
                                        tokenizer=tokenizer, clean=True, seed=opt.seed, row_streams=list(chunk),
                                        **({"share_prefix": share_prefix} if share_prefix else {}),
                                        **({"fork_prefill": True} if fork_prefill else {}),
                                        **({"keep_cond": True} if keep_cond else {}), **sampling)
        torch.cuda.synchronize()
        dt = time.time() - t0
        blp = model.last_logprobs
        if blp is not None:
            blp = (blp["model"].cpu().numpy(), blp["policy"].cpu().numpy())
        for r, j in enumerate(chunk):
            save_job(j, meshes[r], tokens[r], f"time = {dt:.4f}s ({len(chunk)} jobs in this call)",
                     None if blp is None else (blp[0][r], blp[1][r]))
    # the one exchange of the sharded path: RCCL all-gather of the token streams (ids - 3, >= -3, so shift to >= 0)
    gathered = D.gather_token_streams([local_streams[j] + 3 for j in mine], len(jobs), device=device)
    if rank == 0:
        index = [f"{os.path.splitext(os.path.basename(p))[0]}_{i}" + (f"_{nf}f" if opt.use_num_face_cond else "")
                 for p, i, nf in jobs]
        np.savez(f"{opt.workspace}/tokens_all.npz", **{k: g - 3 for k, g in zip(index, gathered)})
        print(f"[INFO] {len(jobs)} jobs over {world} rank(s); token streams gathered into {opt.workspace}/tokens_all.npz")
    D.barrier()
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
