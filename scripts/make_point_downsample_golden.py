#!/usr/bin/env python3
"""Writes tests/golden/point_downsample.npz: the reference's own PointEncoder (core/transformer/point.py:129-169, the
point_encoder_mode='downsample' encoder) on two synthetic clouds, with seeded weights.

torch_cluster is not installed, so ``torch_cluster.fps`` is a stub that runs the project's restatement of farthest point sampling
(tests/point_downsample_ref.py: first sample = point 0, lowest index on ties) and returns flattened indices b * N + i as torch_cluster
does.  Everything after the sampling is the reference's code; the sampling itself is pinned to the restatement only (unpinned
against the real torch_cluster).  Needs the reference checkout (oracle/ref_stubs.py); CPU only.

    python scripts/make_point_downsample_golden.py [--out tests/golden/point_downsample.npz]
"""
import argparse
import dataclasses
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

N_POINTS = 4096
CLOUDS = (0, 5)
ROW_STRIDE = 8          # latent rows kept: every 8th of point_latent_size (the file stays small)
FINGERPRINT_KEYS = ("point_encoder.point_embed.mlp.weight", "point_encoder.cross_att.att.q_proj.weight",
                    "point_encoder.cross_att.mlp.net.0.weight", "point_encoder.linear.weight", "point_encoder.linear.bias")


def reference_encoder(opt, sd):
    import ref_stubs
    import point_downsample_ref as R
    ref_stubs.install()
    sys.modules["torch_cluster"] = R.torch_cluster_stub()
    from core.transformer.point import PointEncoder
    enc = PointEncoder(hidden_dim=opt.point_hidden_dim, num_heads=opt.point_num_heads, latent_size=opt.point_latent_size,
                       latent_dim=opt.point_latent_dim, gradient_checkpointing=False)
    pre = "point_encoder."
    enc.load_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}, strict=True)
    return enc.eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "point_downsample.npz"))
    args = ap.parse_args()
    from edgerunner_amd import weights as W
    from edgerunner_amd.options import config_defaults
    import point_downsample_ref as R
    opt = dataclasses.replace(config_defaults["ArAE"], num_layers=2, point_encoder_mode="downsample")
    sd = W.make_state_dict(opt, 0, "perturbed")
    assert "point_encoder.query_embed" not in sd
    enc = reference_encoder(opt, sd)
    pc = torch.cat([W.synthetic_point_cloud(i, N_POINTS) for i in CLOUDS])
    with torch.no_grad():
        lat = enc(pc).mode()
    idx = R.fps(pc.numpy(), opt.point_latent_size)
    rows = np.arange(0, opt.point_latent_size, ROW_STRIDE)
    # the restated encoder on the same samples agrees with the reference's modules
    with torch.no_grad():
        mine = R.encoder_downsample(sd, pc, opt.point_num_heads, idx)
    err = float((mine - lat).abs().max())
    print(f"restatement vs reference PointEncoder: max abs err {err:.3e}")
    assert err < 1e-4, err
    np.savez_compressed(
        args.out, points=pc.numpy().astype(np.float32), fps_idx=idx.astype(np.int32), rows=rows.astype(np.int32),
        latent_rows=lat[:, rows].numpy().astype(np.float32), kl=np.float64(0.5 * float((lat.double() ** 2).sum())),
        fingerprint_keys=np.array(FINGERPRINT_KEYS), fingerprints=np.array([W.fingerprint(sd[k]) for k in FINGERPRINT_KEYS]),
        seed=np.int64(0), style=np.array("perturbed"))
    print(f"wrote {args.out} ({os.path.getsize(args.out) / 1024:.0f} KB)")


if __name__ == "__main__":
    main()
