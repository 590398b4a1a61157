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
