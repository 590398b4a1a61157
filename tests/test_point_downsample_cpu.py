"""The downsample point encoder without a GPU: the farthest-point-sampling restatement (tests/point_downsample_ref.py) against its
round-by-round definition and against the reference's PointEncoder, the construction path that used to refuse the mode, the
checkpoint contract, the C header and the sampling kernel's code generation."""
import dataclasses
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import point_downsample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def clouds():
    rng = np.random.default_rng(0)
    g = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    dup = rng.standard_normal((20, 3)).astype(np.float32)
    return {
        "random": (rng.standard_normal((40, 3)).astype(np.float32), 17),
        "grid_ties": (g, 27),                                    # exact ties every round, N == n_samples
        "duplicates": (np.concatenate([dup, dup, dup[:5]]), 30),
        "all_equal": (np.full((9, 3), 0.5, dtype=np.float32), 9),
        "n_equals_s": (rng.uniform(-1, 1, (16, 3)).astype(np.float32), 16),
        "one_sample": (rng.standard_normal((5, 3)).astype(np.float32), 1),
    }


@pytest.mark.parametrize("name", list(clouds()))
def test_fps_restatement_equals_bruteforce_definition(name):
    pts, S = clouds()[name]
    assert R.fps(pts, S).tolist() == R.fps_bruteforce(pts, S)


def test_fps_degenerate_and_batched():
    assert R.fps(np.zeros((6, 3), np.float32), 6).tolist() == [0] * 6
    a, b = clouds()["random"][0], clouds()["duplicates"][0][:40]
    both = R.fps(np.stack([a, b]), 12)
    assert both[0].tolist() == R.fps(a, 12).tolist() and both[1].tolist() == R.fps(b, 12).tolist()
    with pytest.raises(ValueError):
        R.fps(a, 41)


def test_torch_cluster_stub_returns_flattened_indices():
    pts = torch.from_numpy(np.stack([clouds()["random"][0], clouds()["random"][0][::-1].copy()]))
    stub = R.torch_cluster_stub()
    idx = stub.fps(pts.view(-1, 3), torch.arange(2).repeat_interleave(40), ratio=10 / 40)
    assert idx.tolist() == R.fps(pts[0].numpy(), 10).tolist() + (R.fps(pts[1].numpy(), 10) + 40).tolist()


def test_lmm_constructs_in_downsample_mode():
    """main refused point_encoder_mode='downsample' with NotImplementedError before any device work."""
    from edgerunner_amd.models import LMM
    from edgerunner_amd.options import config_defaults
    opt = dataclasses.replace(config_defaults["ArAE"], point_encoder_mode="downsample")
    m = LMM(opt, "cuda:0", precision=None)
    assert m.dims.point_encoder_mode == "downsample"
    from edgerunner_amd.weights import tensor_specs
    sd = {k: torch.zeros(1) for k, _, _ in tensor_specs(m.dims)}
    missing, unexpected = m.load_state_dict(sd, strict=True)             # module style: checked against the specs only
    assert not missing and not unexpected


def test_specs_drop_query_embed_only_in_downsample_mode():
    from edgerunner_amd import weights as W
    from edgerunner_amd.models_dit import point_encoder_keys
    from edgerunner_amd.options import config_defaults
    emb = config_defaults["ArAE"]
    ds = dataclasses.replace(emb, point_encoder_mode="downsample")
    se = W.tensor_specs(W.dims_from_options(emb))
    sds = W.tensor_specs(W.dims_from_options(ds))
    assert [s for s in se if s[0] != "point_encoder.query_embed"] == sds
    assert any(s[0] == "point_encoder.query_embed" for s in se)
    assert "point_encoder.query_embed" not in W.make_state_dict(dataclasses.replace(ds, num_layers=1), 0)
    assert point_encoder_keys(emb) - point_encoder_keys(ds) == {"point_encoder.query_embed"}
    assert point_encoder_keys(dataclasses.replace(config_defaults["DiT"], point_encoder_mode="downsample")) == point_encoder_keys(ds)


def test_header_declares_the_new_entries():
    from edgerunner_amd import native
    src = open(os.path.join(ROOT, "include", "edgerunner_hip.h")).read()
    for name in ("er_set_point_encoder_mode", "er_dit_set_point_encoder_mode", "er_k_fps"):
        assert re.search(rf"\bint {name}\(", src) and name in native.EXPORTS, name
    m = re.search(r"typedef enum \{ ER_PE_EMBED = (\d+), ER_PE_DOWNSAMPLE = (\d+) \}", src)
    assert m and (int(m.group(1)), int(m.group(2))) == (native.ER_PE_EMBED, native.ER_PE_DOWNSAMPLE)


def test_fps_kernels_use_no_lds_crossbar_and_no_fma():
    """The per-round reductions run on v_permlane*_swap + DPP (er_common.h), and the distance is rounded term by term."""
    from edgerunner_amd import build as B
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "fps.hip")
        with open(src, "w") as fh:
            fh.write(f'#include "{os.path.join(ROOT, "edgerunner_amd", "csrc", "k_fps.h")}"\n'
                     "template __global__ void er::fps_reg_kernel<8>(const float*, int, int, int32_t*);\n"
                     "template __global__ void er::fps_reg_kernel<16>(const float*, int, int, int32_t*);\n")
        out = os.path.join(tmp, "fps.s")
        flags = [f for f in B.FLAGS if f not in ("-shared", "-fPIC")]
        subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", "-o", out, src], check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL)
        text = open(out).read()
    bodies = dict(re.findall(r"\n(_Z[^\n:]*fps_(?:reg|global)_kernel[^\n:]*):\s*; @[^\n]*\n(.*?)s_endpgm", text, flags=re.S))
    assert len(bodies) >= 3, list(bodies)
    for name, body in bodies.items():
        assert "ds_bpermute" not in body, name
        assert "v_permlane32_swap" in body and "v_permlane16_swap" in body, name
        assert not re.search(r"\bv_(pk_)?fma\w*_f32|\bv_fmac_f32|\bv_mac_f32|\bv_mad_f32", body), name
    for m in re.finditer(r"\.amdhsa_kernel (\S*fps\S*)\n(.*?)\.end_amdhsa_kernel", text, flags=re.S):
        assert int(re.search(r"private_segment_fixed_size (\d+)", m.group(2)).group(1)) == 0, (m.group(1), "register spill")


def test_reference_point_encoder_with_stubbed_fps_matches_restatement():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_stubs
    if not ref_stubs.reference_available():
        pytest.skip("reference checkout not present")
    from edgerunner_amd import weights as W
    from edgerunner_amd.options import config_defaults
    ref_stubs.install()
    sys.modules["torch_cluster"] = R.torch_cluster_stub()
    from core.transformer.point import PointEncoder
    opt = dataclasses.replace(config_defaults["ArAE"], num_layers=1, point_encoder_mode="downsample", point_latent_size=64)
    sd = W.make_state_dict(opt, 1, "perturbed")
    enc = PointEncoder(hidden_dim=opt.point_hidden_dim, num_heads=opt.point_num_heads, latent_size=64,
                       latent_dim=opt.point_latent_dim, gradient_checkpointing=False)
    enc.load_state_dict({k[len("point_encoder."):]: v for k, v in sd.items() if k.startswith("point_encoder.")}, strict=True)
    pc = torch.cat([W.synthetic_point_cloud(i, 256) for i in (0, 1)])
    with torch.no_grad():
        want = enc.eval()(pc).mode()
        got = R.encoder_downsample(sd, pc, opt.point_num_heads, R.fps(pc.numpy(), 64))
    assert float((got - want).abs().max()) < 1e-5
