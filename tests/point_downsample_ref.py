"""CPU restatement of the downsample point encoder (core/transformer/point.py:129-169, PointEncoder) for the tests and the golden
generator - test infrastructure, never imported by the product package.

Farthest point sampling is torch_cluster.fps's CPU algorithm with random_start=False, restated here because torch_cluster is not
installed (and its random_start=True default is not deterministic):
  * sample 0 is point 0 of the cloud; dist[i] = d(p_i, p_0);
  * for k = 1 .. S-1: s_k = argmax(dist), lowest index on ties; dist = min(dist, d(p_i, p_{s_k}));
  * d(a, b) = (dx*dx + dy*dy) + dz*dz in fp32, each product and sum rounded on its own.
Already-selected points stay in the argmax with distance 0, so an all-equal cloud gives 0, 0, 0, ...  The rest of the encoder is
built from oracle/arae_oracle.py's pieces (point_embed, LayerNorm, attention, GEGLU) exactly as its PointEncoderEmbed restatement.
"""
import numpy as np
import torch
import torch.nn.functional as F


def _d2(p, c):
    """(dx*dx + dy*dy) + dz*dz in fp32 for points p [..., 3] and one point c [3]."""
    p = np.asarray(p, dtype=np.float32)
    c = np.asarray(c, dtype=np.float32)
    dx = p[..., 0] - c[0]
    dy = p[..., 1] - c[1]
    dz = p[..., 2] - c[2]
    return (dx * dx + dy * dy) + dz * dz


def fps(points, n_samples: int) -> np.ndarray:
    """points [B, N, 3] (or [N, 3]) -> int64 indices [B, n_samples] (or [n_samples]), 0-based within each cloud."""
    pts = np.asarray(points, dtype=np.float32)
    single = pts.ndim == 2
    if single:
        pts = pts[None]
    B, N, _ = pts.shape
    if not 1 <= n_samples <= N:
        raise ValueError(f"n_samples {n_samples} must lie in [1, {N}]")
    out = np.zeros((B, n_samples), dtype=np.int64)
    for b in range(B):
        p = pts[b]
        dist = _d2(p, p[0])
        for k in range(1, n_samples):
            s = int(np.argmax(dist))                 # first maximal index
            out[b, k] = s
            dist = np.minimum(dist, _d2(p, p[s]))
    return out[0] if single else out


def fps_bruteforce(points, n_samples: int):
    """The definition round by round with Python scalars (np.float32 arithmetic), for small clouds."""
    p = [tuple(np.float32(v) for v in row) for row in np.asarray(points, dtype=np.float32)]

    def d(a, b):
        dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
        return np.float32(np.float32(np.float32(dx * dx) + np.float32(dy * dy)) + np.float32(dz * dz))

    dist = [d(q, p[0]) for q in p]
    sel = [0]
    for _ in range(1, n_samples):
        best = 0
        for i in range(1, len(p)):
            if dist[i] > dist[best]:
                best = i
        sel.append(best)
        dist = [min(dist[i], d(p[i], p[best])) for i in range(len(p))]
    return sel


def torch_cluster_stub():
    """A stand-in ``torch_cluster`` module whose ``fps(src, batch, ratio)`` runs the restatement above and returns FLATTENED
    indices b * N + i, as torch_cluster does.  Clouds are the runs of equal values in ``batch``; ceil(N * ratio) samples each."""
    import math
    import types

    def _fps(src, batch=None, ratio=0.5, random_start=True, batch_size=None):
        src = src.detach().cpu()
        if batch is None:
            batch = torch.zeros(src.shape[0], dtype=torch.long)
        batch = batch.detach().cpu()
        out, start = [], 0
        for b in torch.unique_consecutive(batch).tolist():
            n = int((batch == b).sum())
            k = int(math.ceil(n * ratio))
            out.append(torch.from_numpy(fps(src[start:start + n].numpy(), k)) + start)
            start += n
        return torch.cat(out)

    mod = types.ModuleType("torch_cluster")
    mod.fps = _fps
    return mod


def encoder_downsample(sd, x, num_heads: int, idx):
    """PointEncoder.forward (point.py:143-169) at state_dict level: x [B, N, 3] -> latent mean [B, L, latent_dim] (DummyLatent: mode
    == mean).  idx [B, L] (0-based per cloud) = the FPS samples (``fps(x, L)``)."""
    import arae_oracle as O
    pe = "point_encoder"
    B = x.shape[0]
    c = O._ln(sd, f"{pe}.ln", O.point_embed(sd, x))                          # :150
    idx = torch.as_tensor(np.asarray(idx), dtype=torch.long)
    qpc = torch.stack([x[b, idx[b]] for b in range(B)])                       # pc_flattened[fps_indices].view(B, L, 3)
    q = O.point_embed(sd, qpc)                                                # :157, no ln
    a = f"{pe}.cross_att.att"
    xq = O._ln(sd, f"{pe}.cross_att.ln1", q)
    Nq, M = xq.shape[1], c.shape[1]
    hd = xq.shape[2] // num_heads
    qq = O._lin(sd, f"{a}.q_proj", xq).reshape(B, Nq, num_heads, hd)
    kk = O._lin(sd, f"{a}.k_proj", c).reshape(B, M, num_heads, hd)
    vv = O._lin(sd, f"{a}.v_proj", c).reshape(B, M, num_heads, hd)
    att = O.attention_naive(qq, kk, vv, causal=False)
    att = O._lin(sd, f"{a}.out_proj", att.reshape(B, Nq, -1))
    l = q + att
    u = O._lin(sd, f"{pe}.cross_att.mlp.net.0", O._ln(sd, f"{pe}.cross_att.ln2", l))
    xx, gates = u.chunk(2, dim=-1)
    l = l + O._lin(sd, f"{pe}.cross_att.mlp.net.2", xx * F.gelu(gates))
    return O._lin(sd, f"{pe}.linear", l)                                      # :165


def latent(sd, opt, x):
    """encoder_downsample with the restated FPS at opt.point_latent_size samples."""
    return encoder_downsample(sd, x, opt.point_num_heads, fps(x.float().numpy(), opt.point_latent_size))


def encode_cond(sd, opt, conds, num_faces):
    """core/models.py:101-144 (eval mode) with the downsample encoder."""
    import arae_oracle as O
    lat = latent(sd, opt, conds)
    cond = O._ln(sd, "norm_cond", O._lin(sd, "proj_cond", lat))
    if opt.use_num_face_cond:
        nf = F.embedding(O.quantize_num_faces(torch.as_tensor(num_faces)), sd["embed_num_face.weight"]).unsqueeze(1)
        cond = torch.cat((cond, nf), dim=1)
    return cond
