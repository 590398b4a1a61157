"""Checkpoint loading (csrc/er_weights.h) stores the same numbers whatever form they arrive in: fp32 from the host or from the device,
and values that are exactly bf16 (fp16) handed over in their own dtype or as .float(), give bit-identical outputs of the LMM (with a
point encoder, embed and downsample, exact and fp16 mode) and of MDiT (CLIP + attached point encoder, fp32 and fp16).  Also pinned:
element-count errors name the key, unknown keys come back as unexpected, and loading a tensor again gives the outputs of a context
that was loaded with the new values from the start.  Small shapes: one decoder / DiT layer, two CLIP layers."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_POINTS = 2304          # downsample needs n_points >= point_latent_size (2048)


def lmm_opt(mode):
    from edgerunner_amd.options import config_defaults
    return dataclasses.replace(config_defaults["ArAE"], num_layers=1, generate_mode="greedy", point_encoder_mode=mode,
                               dit_num_layers=1)


_SD = {}


def lmm_sd(mode):
    from edgerunner_amd import weights as W
    if ("lmm", mode) not in _SD:
        _SD["lmm", mode] = W.make_state_dict(lmm_opt(mode), 0, "perturbed")     # downsample: no query_embed
    return _SD["lmm", mode]


def dit_sd():
    from edgerunner_amd import weights as W
    if "dit" not in _SD:
        sd = dict(W.make_dit_state_dict(lmm_opt("embed"), 0, "perturbed"))
        sd.update(W.make_clip_state_dict(2, 0, "perturbed"))
        sd.update({k: v for k, v in lmm_sd("embed").items() if k.startswith("point_encoder.")})
        _SD["dit"] = sd
    return _SD["dit"]


def four_ways(sd):
    """(name, state_dict) pairs: fp32 host / fp32 device hold the same values; so do the bf16 and fp16 pairs (rounded once)."""
    bf = {k: v.to(torch.bfloat16) for k, v in sd.items()}
    hf = {k: v.to(torch.float16) for k, v in sd.items()}
    return [
        (("f32", "host"), sd),
        (("f32", "device"), {k: v.to(DEV) for k, v in sd.items()}),
        (("bf16", "device bf16"), {k: v.to(DEV) for k, v in bf.items()}),
        (("bf16", "host as f32"), {k: v.float() for k, v in bf.items()}),
        (("f16", "host f16"), hf),
        (("f16", "device as f32"), {k: v.float().to(DEV) for k, v in hf.items()}),
    ]


def cloud():
    from edgerunner_amd import weights as W
    return W.synthetic_point_cloud(3, N_POINTS).to(DEV)


def lmm_loaded(mode, precision, sd):
    from edgerunner_amd.models import LMM
    m = LMM(lmm_opt(mode), DEV, precision=precision)
    missing, unexpected = m.mesh_decoder.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    return m.mesh_decoder


def lmm_outputs(dec):
    """encode_cond, point_latent (+ KL) and the prefill's last logits of one cloud + six tokens"""
    pc = cloud()
    cond = dec.encode_cond(pc, [5])
    lat, kl = dec.point_latent(pc)
    ids = torch.tensor([[0, 7, 123, 400, 81, 9]])
    dec.prefill(torch.cat([cond, dec.embd(ids)], dim=1), 1)
    out = [cond, lat, kl, dec.logits()]
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


def dit_loaded(precision, sd):
    from edgerunner_amd.models_dit import MDiT
    m = MDiT(lmm_opt("embed"), DEV, clip_layers=2, precision=precision, point_encoder=True)
    missing, unexpected = m.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    return m


def dit_outputs(m):
    """encode_image, get_cond, one DiT forward and point_latent"""
    from edgerunner_amd import native
    gen = torch.Generator().manual_seed(11)
    img = torch.rand(1, 3, 224, 224, generator=gen).to(DEV)
    x = torch.randn(1, 2048, 64, generator=gen).to(DEV)
    hid = torch.empty((1, 257, 1280), device=DEV)
    torch.cuda.synchronize()
    native.check(m.lib.er_dit_encode_image(m._ctx, native.ptr(img), 1, 224, 224, native.ptr(hid), None), "er_dit_encode_image")
    torch.cuda.synchronize()
    cond = m.get_cond(img)
    out = [hid, cond, m.dit(x, cond, torch.tensor([417.0])), m.point_latent(cloud())]
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


def assert_same_per_value_set(results):
    by_values = {}
    for (vals, how), outs in results:
        if vals not in by_values:
            by_values[vals] = (how, outs)
            continue
        ref_how, ref = by_values[vals]
        for i, (a, b) in enumerate(zip(ref, outs)):
            assert torch.equal(a, b), f"{vals}: output {i} differs between '{ref_how}' and '{how}'"


@pytest.mark.parametrize("mode", ["embed", "downsample"])
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_lmm_same_values_any_dtype_any_memory(mode, precision):
    results = []
    for name, sd in four_ways(lmm_sd(mode)):
        dec = lmm_loaded(mode, precision, sd)
        results.append((name, lmm_outputs(dec)))
        dec.close()
    assert_same_per_value_set(results)


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_dit_same_values_any_dtype_any_memory(precision):
    results = []
    for name, sd in four_ways(dit_sd()):
        m = dit_loaded(precision, sd)
        results.append((name, dit_outputs(m)))
        m.close()
    assert_same_per_value_set(results)


def test_wrong_element_count_names_the_key():
    from edgerunner_amd import native
    from edgerunner_amd.models import LMM
    from edgerunner_amd.models_dit import MDiT
    dec = LMM(lmm_opt("embed"), DEV).mesh_decoder
    for key in ("point_encoder.point_embed.mlp.weight", "mesh_decoder.model.layers.0.self_attn.k_proj.weight"):
        with pytest.raises(native.NativeError, match=key.replace(".", r"\.") + ".*elements, expected"):
            dec.load_state_dict({key: torch.zeros(3, 5)})
    m = MDiT(lmm_opt("embed"), DEV, clip_layers=2, point_encoder=True)
    for key in ("dit.proj_in.weight", "image_encoder.vision_model.embeddings.patch_embedding.weight", "point_encoder.ln.bias"):
        with pytest.raises(native.NativeError, match=key.replace(".", r"\.") + ".*elements, expected"):
            m.load_state_dict({key: torch.zeros(7)})
    m.close()


def test_unknown_keys_are_unexpected():
    from edgerunner_amd.models import LMM
    from edgerunner_amd.models_dit import MDiT
    t = torch.zeros(4)
    dec = LMM(lmm_opt("downsample"), DEV).mesh_decoder
    _, unexpected = dec.load_state_dict({"no.such.key": t, "point_encoder.query_embed": t,
                                         "mesh_decoder.model.layers.1.fc1.bias": t})
    assert unexpected == ["no.such.key", "point_encoder.query_embed", "mesh_decoder.model.layers.1.fc1.bias"]
    m = MDiT(lmm_opt("embed"), DEV, clip_layers=0)          # no encoder attached, no image encoder
    _, unexpected = m.load_state_dict({"point_encoder.ln.weight": t, "image_encoder.vision_model.pre_layrnorm.weight": t,
                                       "dit.nothing": t})
    assert sorted(unexpected) == ["dit.nothing", "image_encoder.vision_model.pre_layrnorm.weight", "point_encoder.ln.weight"]
    m.close()


def changed(sd, keys):
    return {k: (sd[k] * 0.75 + 0.01).contiguous() for k in keys}


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_lmm_reload_equals_fresh_load(precision):
    sd = lmm_sd("embed")
    new = changed(sd, ["mesh_decoder.model.layers.0.self_attn.k_proj.weight", "mesh_decoder.model.layers.0.self_attn.v_proj.bias",
                       "mesh_decoder.lm_head.weight", "point_encoder.point_embed.mlp.weight", "point_encoder.query_embed"])
    dec = lmm_loaded("embed", precision, dict(sd, **new))
    fresh = lmm_outputs(dec)
    dec.close()
    dec = lmm_loaded("embed", precision, sd)
    before = lmm_outputs(dec)
    dec.load_state_dict({k: v.to(DEV) for k, v in new.items()})
    after = lmm_outputs(dec)
    dec.close()
    for i, (a, b) in enumerate(zip(fresh, after)):
        assert torch.equal(a, b), f"output {i}"
    assert not torch.equal(before[3], after[3])


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_dit_reload_equals_fresh_load(precision):
    sd = dit_sd()
    new = changed(sd, ["dit.layers.0.ff.net.0.weight", "dit.layers.0.attn1.qkv_proj.weight",
                       "image_encoder.vision_model.embeddings.patch_embedding.weight", "point_encoder.point_embed.mlp.weight"])
    m = dit_loaded(precision, dict(sd, **new))
    fresh = dit_outputs(m)
    m.close()
    m = dit_loaded(precision, sd)
    before = dit_outputs(m)
    m.load_state_dict(new)
    after = dit_outputs(m)
    m.close()
    for i, (a, b) in enumerate(zip(fresh, after)):
        assert torch.equal(a, b), f"output {i}"
    assert not torch.equal(before[2], after[2])
