"""Data side of the reference's eval loop (core/provider.py) in plain numpy: ``collate_fn`` (core/provider.py:469-541) and one
helper that turns a mesh file into the dataset item it pads (the fields ``ObjaverseDataset.__getitem__`` returns,
core/provider.py:250-309, in eval mode: no augmentation).  ``LMM.forward`` consumes what ``collate_fn`` returns."""
from __future__ import annotations

import os
import zlib
from typing import Dict, List, Optional

import numpy as np
import torch

from . import meshio
from .meto import tokenize_mesh


def collate_fn(batch: List[Dict], opt) -> Dict:
    """core/provider.py:469-541: pads (right) or truncates every item to the longest one, capped at ``opt.max_seq_length``.
    tokens = [BOS, coords, EOS, pad...]; labels = [-100 x (num_cond_tokens + 1), coords, EOS, -100...] (a truncated item has
    neither EOS token nor EOS label); masks = ones over cond + BOS + coords (+ EOS), zeros over the padding.
    One extension: a batch that mixes truncated and padded items makes the reference's np.stack raise (a truncated row is one
    position shorter: no EOS); here such rows get one more padding position (pad token, label -100, mask 0) instead."""
    C = opt.num_cond_tokens
    max_len = min(max(int(item["len"]) for item in batch), opt.max_seq_length)
    tokens, labels, masks, num_tokens = [], [], [], []
    for item in batch:
        coords = np.asarray(item["coords"])
        n = int(item["len"])
        if max_len >= n:
            pad = max_len - n
            tokens.append(np.concatenate([[opt.bos_token_id], coords, [opt.eos_token_id], np.full(pad, opt.pad_token_id)]))
            labels.append(np.concatenate([np.full(C + 1, -100), coords, [opt.eos_token_id], np.full(pad, -100)]))
            masks.append(np.concatenate([np.ones(C + 1 + n + 1), np.zeros(pad)]))
            num_tokens.append(C + 1 + n + 1)
        else:
            tokens.append(np.concatenate([[opt.bos_token_id], coords[:max_len]]))
            labels.append(np.concatenate([np.full(C + 1, -100), coords[:max_len]]))
            masks.append(np.ones(C + 1 + max_len))
            num_tokens.append(C + 1 + max_len)
    for rows, fill in ((tokens, opt.pad_token_id), (labels, -100), (masks, 0)):
        width = max(len(r) for r in rows)
        rows[:] = [np.concatenate([r, np.full(width - len(r), fill)]) for r in rows]
    return {
        "conds": torch.from_numpy(np.stack([np.asarray(item["cond"]) for item in batch], axis=0)).float(),
        "num_faces": torch.from_numpy(np.stack([item["num_faces"] for item in batch], axis=0)).long(),
        "num_tokens": torch.from_numpy(np.stack(num_tokens, axis=0)).long(),
        "azimuths": torch.from_numpy(np.stack([item.get("azimuth", 0) for item in batch], axis=0)).long(),
        "tokens": torch.from_numpy(np.stack(tokens, axis=0)).long(),
        "labels": torch.from_numpy(np.stack(labels, axis=0)).long(),
        "masks": torch.from_numpy(np.stack(masks, axis=0)).bool(),
        "paths": [item.get("path") for item in batch],
    }


def mesh_item(path: str, opt, tokenizer=None, rng: Optional[np.random.Generator] = None) -> Dict:
    """Dataset item of one mesh file (.obj / .ply) in eval mode: the mesh normalised to bound 0.95, ``opt.point_num`` surface
    points as the point condition (``cond_mode='point'``; an empty [0, 3] cloud otherwise), the model ids of
    ``tokenize_mesh`` as ``coords``.  The sampler is the one infer.py uses (seeded by ``opt.seed`` and the file name when no ``rng``
    is given), not trimesh's: the cloud is a different sample of the same surface than the reference would draw."""
    v, f = meshio.load_mesh(path)
    v = meshio.normalize_mesh(v, bound=0.95)
    if opt.cond_mode == "point":
        if rng is None:
            rng = np.random.default_rng([int(opt.seed) & 0xFFFFFFFF, zlib.crc32(os.path.basename(path).encode())])
        cond = meshio.sample_surface(v, f, opt.point_num, rng).astype(np.float32)
    else:
        cond = np.zeros((0, 3), dtype=np.float32)
    coords = np.asarray(tokenize_mesh(v, f, opt.discrete_bins, tokenizer), dtype=np.int64)
    if (coords - 3 < 0).any():                      # core/provider.py:288-290
        raise ValueError(f"{path}: invalid token range {coords.min() - 3} - {coords.max() - 3}")
    return {"cond": cond, "coords": coords, "len": int(coords.shape[0]), "num_faces": int(f.shape[0]), "path": path, "azimuth": 0}


# ------------------------------------------------------------------------------------ DiT pairs (core/provider_dit.py, eval branch)
DIT_IMAGE_SIZE = 512          # the reference dataset's renders are 512 x 512 (provider_dit.py:105); infer_dit.py resizes to it (:97)


def load_image(path: str) -> np.ndarray:
    """An image as float32 [H, W, 3] in [0, 1]: RGB / RGBA / grey files readable by PIL, or .npy arrays [H, W, 3|4] in [0, 1]; alpha is
    composited on white (reference infer_dit.py:93, provider_dit.py:116)."""
    if path.endswith(".npy"):
        a = np.load(path).astype(np.float32)
    else:
        from PIL import Image
        a = np.asarray(Image.open(path)).astype(np.float32) / 255.0
    if a.ndim == 2:
        a = np.repeat(a[..., None], 3, axis=-1)
    if a.shape[-1] == 4:
        a = a[..., :3] * a[..., 3:4] + (1 - a[..., 3:4])
    return a[..., :3]


def dit_item(image_path: str, shape_path: str, opt, rng: Optional[np.random.Generator] = None) -> Dict:
    """Dataset item of one (image, shape) pair as ``ObjaverseDataset.__getitem__`` of provider_dit.py:84-145 returns it in eval mode
    (azimuth 0, no augmentation): ``cond`` = the image [3, 512, 512] in [0, 1] (bilinearly resized like infer_dit.py), ``points`` =
    ``opt.point_num`` surface samples [N, 3] of the mesh normalised to bound 0.95, or a .npy cloud [N, 3] used as it is.  The surface
    sampler is meshio's (seeded by ``rng``), not trimesh's."""
    import torch.nn.functional as F
    img = torch.from_numpy(np.ascontiguousarray(load_image(image_path))).permute(2, 0, 1).unsqueeze(0).float()
    img = F.interpolate(img, (DIT_IMAGE_SIZE, DIT_IMAGE_SIZE), mode="bilinear", align_corners=False)[0]
    if shape_path.lower().endswith(".npy"):
        points = np.load(shape_path).astype(np.float32)
        if points.ndim != 2 or points.shape[1] != 3:
            raise ValueError(f"{shape_path}: a point cloud must be [N, 3], got {points.shape}")
    else:
        v, f = meshio.load_mesh(shape_path)
        v = meshio.normalize_mesh(v, bound=0.95)
        if rng is None:
            rng = np.random.default_rng([int(opt.seed) & 0xFFFFFFFF, zlib.crc32(os.path.basename(shape_path).encode())])
        points = meshio.sample_surface(v, f, opt.point_num, rng).astype(np.float32)
    return {"cond": img.contiguous(), "points": torch.from_numpy(np.ascontiguousarray(points)), "image_path": image_path,
            "shape_path": shape_path}


def collate_dit(batch: List[Dict]) -> Dict:
    """Stacks ``dit_item`` results into the batch ``MDiT.forward`` takes: cond [B, 3, 512, 512], points [B, N, 3] (every cloud of a
    batch must have the same N, as the reference's default collate requires)."""
    sizes = {tuple(item["points"].shape) for item in batch}
    if len(sizes) != 1:
        raise ValueError(f"point clouds of one batch must have the same shape, got {sorted(sizes)}")
    return {
        "cond": torch.stack([item["cond"] for item in batch], dim=0),
        "points": torch.stack([item["points"] for item in batch], dim=0),
        "paths": [(item["image_path"], item["shape_path"]) for item in batch],
    }
