"""Device memory comes back when a context is closed (csrc/er_devbuf.h: every buffer of the host layer is a member of its context
or a local of its entry point).  A cycle creates a 2-layer LMM, generates at B = 1 and B = 6 (the KV cache and both decode
workspaces are reserved, then reserved again for the other shape), scores one row and closes it; then the same with a 2-layer MDiT
that has a point encoder attached (eval loss from points, two sampler steps).  After one warm-up cycle the device's free memory is read;
after three more cycles it must be the same figure within one allocation granule.

GRANULE: ``torch.cuda.mem_get_info`` moves in steps of 2 MiB on the MI355X.  Measured with raw hipMalloc calls: 1 byte .. 64 KiB
move the figure by 0 (the runtime carves them out of a block it already holds), 1 MiB .. 2 MiB by 2 MiB, 2 MiB + 1 byte by 4 MiB, and
an idle process reads the same figure every time.  So the bound is 2 MiB, and a forgotten buffer of 1 MiB or more shows as three times
its rounded size.  The figure is device-wide: another process allocating on the same card during the test moves it too.

One thing besides the library moves the figure and is taken out first (``touch_stream_pool``): every LMM / MDiT takes the next
``torch.cuda.Stream`` of torch's pool of 32, and the first launch on each of them costs the HIP runtime 2 MiB that it keeps.  Without
that step the figure sank by 2 MiB per cycle for 15 cycles and then stood still for the next 25 (same with the library before and
after the buffers became members); with it, eight further cycles in either precision each read the warm-up figure again."""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRANULE = 2 << 20


def opt_small():
    from edgerunner_amd.options import config_defaults
    return dataclasses.replace(config_defaults["ArAE"], num_layers=2, generate_mode="greedy", dit_num_layers=2)


@pytest.fixture(scope="module")
def weights():
    from edgerunner_amd import weights as W
    opt = opt_small()
    sd_lmm = W.make_state_dict(opt, 0, "perturbed")
    sd_dit = dict(W.make_dit_state_dict(opt, 0, "perturbed"))
    sd_dit.update({k: v for k, v in sd_lmm.items() if k.startswith("point_encoder.")})
    return opt, sd_lmm, sd_dit


def clouds(n, points=512):
    from edgerunner_amd import weights as W
    return torch.cat([W.synthetic_point_cloud(i, points) for i in range(n)], dim=0)


def lmm_cycle(opt, sd, precision):
    from edgerunner_amd.models import LMM
    from edgerunner_amd.provider import collate_fn
    lmm = LMM(opt, DEV, precision=precision)
    lmm.load_state_dict(sd, strict=True)
    pc = clouds(6)
    _, one = lmm.generate(pc[:1].to(DEV), 1000, tokenizer=object(), max_new_tokens=8, min_new_tokens=8)
    _, six = lmm.generate(pc.to(DEV), 1000, tokenizer=object(), max_new_tokens=8, min_new_tokens=8)
    _, again = lmm.generate(pc[:1].to(DEV), 1000, tokenizer=object(), max_new_tokens=8, min_new_tokens=8)
    assert len(six) == 6 and np.array_equal(one[0], again[0])
    ids = np.asarray(one[0], dtype=np.int64)
    item = {"cond": pc[0].numpy(), "num_faces": 1000, "coords": ids, "len": len(ids), "azimuth": 0, "path": None}
    loss = float(lmm.forward(collate_fn([item], opt))["loss"])
    assert np.isfinite(loss)
    lmm.mesh_decoder.close()


def dit_cycle(opt, sd, precision):
    from edgerunner_amd.models_dit import MDiT
    m = MDiT(opt, DEV, clip_layers=0, precision=precision, point_encoder=True)
    m.load_state_dict(sd, strict=True)
    gen = torch.Generator().manual_seed(5)
    hid = torch.randn(2, 257, 1280, generator=gen)
    out = m.forward({"cond": hid, "points": clouds(2, 2048)}, generator=gen)
    assert np.isfinite(float(out["loss"]))
    lat = m.run(hid[:1], num_inference_steps=2, noise=torch.randn(1, opt.point_latent_size, opt.point_latent_dim, generator=gen))
    assert bool(torch.isfinite(lat).all())
    m.close()


def touch_stream_pool():
    """One launch on every stream torch can hand out, so that the runtime's per-stream memory exists before anything is measured."""
    x = torch.zeros(1024, device=DEV)
    seen = set()
    for _ in range(256):
        s = torch.cuda.Stream(device=DEV)
        if s.cuda_stream in seen:
            break
        seen.add(s.cuda_stream)
        with torch.cuda.stream(s):
            x.add_(1.0)
    torch.cuda.synchronize()


def free_bytes():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()          # torch's own cache is not what is measured
    return torch.cuda.mem_get_info(torch.device(DEV))[0]


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_closed_contexts_give_their_memory_back(weights, precision):
    opt, sd_lmm, sd_dit = weights

    def cycle():
        lmm_cycle(opt, sd_lmm, precision)
        dit_cycle(opt, sd_dit, precision)

    touch_stream_pool()
    cycle()                           # warm-up: the runtime's own one-time allocations (code objects, graph memory)
    warm = free_bytes()
    after = []
    for _ in range(3):
        cycle()
        after.append(free_bytes())
    print(f"{precision}: free after warm-up {warm}, after cycles 2..4 {after} (deltas {[warm - a for a in after]} bytes)")
    assert abs(warm - after[-1]) <= GRANULE, f"free memory moved by {warm - after[-1]} bytes over three create / run / close cycles"
