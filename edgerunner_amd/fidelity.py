"""Reconstruction fidelity: how close a generated mesh is to the point cloud it was conditioned on.

``fidelity(clouds, meshes)`` samples points on every mesh and measures nearest-neighbour distances to its cloud in both directions
on the device (csrc/k_fidelity.h: no distance matrix is stored), giving Chamfer L1 / L2, Hausdorff and precision / recall / F-score
at a threshold.  ``pair_workspace`` is the host side of ``fidelity.py``: which ``.ply`` candidates of an ``infer.py`` workspace
belong to which ``_pc.obj`` cloud.  There is no CPU path for the metrics themselves."""
from __future__ import annotations

import re
from typing import Dict, List, Optional, Sequence

import numpy as np

COORD_MAX = 8.0            # |coordinate| bound of the sampler's integer face weights (er_k_surface_sample)
MAX_FACES = 1 << 22


def pair_workspace(files: Sequence[str]) -> Dict[str, List[str]]:
    """File names of a workspace written by infer.py -> {name: its candidates}: every ``{name}_pc.obj`` is an input, and its
    candidates are the ``{name}_{i}.ply`` / ``{name}_{i}_{n}f.ply`` files, ordered by (i, n).  An input without a mesh keeps an
    empty list; a name that is a prefix of another name takes only its own files (``a_0.ply`` is of ``a``, ``a_1_0.ply`` of ``a_1``)."""
    names = sorted(f[:-len("_pc.obj")] for f in files if f.endswith("_pc.obj"))
    out = {}
    for name in names:
        pat = re.compile(re.escape(name) + r"_(\d+)(?:_(\d+)f)?\.ply")
        hits = []
        for f in files:
            m = pat.fullmatch(f)
            if m:
                hits.append((int(m.group(1)), int(m.group(2)) if m.group(2) else -1, f))
        out[name] = [f for _, _, f in sorted(hits)]
    return out


def face_weights(v, f):
    """The sampler's integer face weights llrint(area * 2^32), operation by operation as face_weight_kernel computes them (double
    arithmetic on the fp32 coordinates, every product and sum rounded on its own): the host and the device agree on which faces,
    and so which meshes, have area."""
    p = np.asarray(v, np.float32).astype(np.float64)[np.asarray(f, np.int64)]
    a, b = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    return np.rint((0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)) * 4294967296.0).astype(np.int64)


def mesh_arrays(mesh, where="mesh"):
    """(v [V,3] float32, f [F,3] int64) of a meto.Mesh or a (v, f) pair, validated (ValueError); None for a mesh that is None or
    has no faces or no area."""
    if mesh is None:
        return None
    v, f = (mesh.vertices, mesh.faces) if hasattr(mesh, "vertices") else mesh
    v = np.asarray(v, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(f).reshape(-1, 3)
    if f.shape[0] == 0:
        return None
    if f.shape[0] > MAX_FACES:
        raise ValueError(f"{where}: {f.shape[0]} faces (at most {MAX_FACES})")
    if not np.isfinite(v).all():
        raise ValueError(f"{where}: non-finite vertex coordinate")
    if v.size and np.abs(v).max() > COORD_MAX:
        raise ValueError(f"{where}: vertex coordinate outside [-{COORD_MAX:g}, {COORD_MAX:g}]")
    if not np.issubdtype(f.dtype, np.integer):
        raise ValueError(f"{where}: face indices are not integers")
    f = f.astype(np.int64)
    if f.min() < 0 or f.max() >= v.shape[0]:
        raise ValueError(f"{where}: face index outside [0, {v.shape[0]})")
    if not (face_weights(v, f) > 0).any():
        return None
    return v, f


def fidelity(clouds, meshes, n_samples: Optional[int] = None, tau: float = 0.02, seed: int = 0,
             streams: Optional[Sequence[int]] = None) -> List[Optional[dict]]:
    """clouds [B, N, 3] (array or tensor), meshes: B ``meto.Mesh`` objects or (vertices, faces) pairs -> per mesh a dict of
    kernels.FIDELITY_METRICS (a = the cloud, b = n_samples surface samples of the mesh; distances in the cloud's units), or None
    for a mesh that is None, has no faces or has zero area.  tau: the F-score threshold (0.02 = 1 % of the normalised cube's
    edge).  Sample i of mesh m draws from the Philox stream (seed, i, streams[m]); streams defaults to the position in the call, a
    caller that batches a longer list passes global indices so that a result does not depend on the batching.
    Raises ValueError for non-finite or out-of-range coordinates and for face indices outside the mesh."""
    import torch
    c = clouds if isinstance(clouds, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(clouds, dtype=np.float32)))
    if c.dim() != 3 or c.shape[2] != 3 or c.shape[1] < 1:
        raise ValueError(f"clouds must be [B, N >= 1, 3], got {tuple(c.shape)}")
    if len(meshes) != c.shape[0]:
        raise ValueError(f"{c.shape[0]} clouds but {len(meshes)} meshes")
    if streams is not None and len(streams) != len(meshes):
        raise ValueError("streams must name one stream per mesh")
    c = c.float()
    if not bool(torch.isfinite(c).all()):
        raise ValueError("clouds: non-finite coordinate")
    if float(c.abs().max()) > COORD_MAX:
        raise ValueError(f"clouds: coordinate outside [-{COORD_MAX:g}, {COORD_MAX:g}]")
    n = int(c.shape[1] if n_samples is None else n_samples)
    if n < 1:
        raise ValueError("n_samples must be positive")
    arrays = [mesh_arrays(m, f"mesh {i}") for i, m in enumerate(meshes)]
    keep = [i for i, a in enumerate(arrays) if a is not None]
    out: List[Optional[dict]] = [None] * len(meshes)
    if not keep:
        return out

    from . import kernels
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible: fidelity() has no CPU fallback")
    dev = c.device if c.is_cuda else torch.device("cuda", torch.cuda.current_device())
    voff = np.concatenate([[0], np.cumsum([arrays[i][0].shape[0] for i in keep])])
    foff = np.concatenate([[0], np.cumsum([arrays[i][1].shape[0] for i in keep])])
    v = torch.from_numpy(np.concatenate([arrays[i][0] for i in keep])).to(dev)
    f = torch.from_numpy(np.concatenate([arrays[i][1] for i in keep]).astype(np.int32)).to(dev)
    a = c.to(dev)
    if len(keep) != len(meshes):
        a = a[torch.as_tensor(keep, device=dev)]
    a = a.contiguous()
    sid = [int(streams[i]) if streams is not None else i for i in keep]
    b = kernels.surface_sample(v, f, voff.tolist(), foff.tolist(), n, seed=seed, stream_ids=sid, return_faces=False)
    d2_ab = kernels.nn_dist2(a, b, return_idx=False)
    d2_ba = kernels.nn_dist2(b, a, return_idx=False)
    m = kernels.fidelity_metrics(d2_ab, d2_ba, tau).cpu().numpy()
    for row, i in enumerate(keep):
        out[i] = {k: float(x) for k, x in zip(kernels.FIDELITY_METRICS, m[row])}
    return out
