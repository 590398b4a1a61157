"""The decode plan of a context is the one its last ``er_kv_reserve`` stored with the memory of that shape (csrc/er_api.hip,
``DecodePlan`` in ``KvMem``).  ONE 2-layer context reserves five shapes in sequence - one row, five rows, one row with the batched
kernels forced, one row again with the switch removed, sixteen rows - and after every reserve

* ``er_ctx_plan`` equals ``er_plan_decode`` of that shape under the environment of that reserve, field for field (the step from the
  forced shape to the plain one is what tells a stored plan from one guessed back out of the context's flags), and
* eight greedy tokens from a fixed 4-token prefix are the ids of a fresh context that reserved only that shape: no kernel choice,
  stride or partial-buffer size of an earlier shape survives into the next.
"""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (batch, max_len, ER_FORCE_BATCHED) in the order the one context reserves them
SHAPES = [(1, 64, None), (5, 64, None), (1, 96, "1"), (1, 64, None), (16, 64, None)]
SWITCHES = ("ER_FORCE_BATCHED", "ER_BATCHED_VALU", "ER_XT", "ER_DECODE_V", "ER_ATTN_V_BATCHED", "ER_NO_GRAPH")


@pytest.fixture(scope="module")
def small():
    from edgerunner_amd import weights as W
    from edgerunner_amd.options import config_defaults
    opt = dataclasses.replace(config_defaults["ArAE"], num_layers=2, generate_mode="greedy")
    return opt, W.make_state_dict(opt, 0, "perturbed")


def make_decoder(small, precision):
    from edgerunner_amd.models import LMM
    opt, sd = small
    lmm = LMM(opt, DEV, precision=precision)
    lmm.load_state_dict(sd, strict=True)
    return lmm.mesh_decoder


def prefix_ids(batch, vocab):
    return torch.tensor([[(11 + 37 * b + 5 * j) % (vocab - 3) + 3 for j in range(4)] for b in range(batch)], dtype=torch.long)


def reserve_and_decode(dec, batch, max_len):
    dec.reserve(batch, max_len)
    plan = dec.plan()
    emb = dec.embd(prefix_ids(batch, dec.dims.vocab_size))
    ids = dec.generate(emb, max_new_tokens=8, min_new_tokens=8).cpu().numpy()
    assert dec._reserved == (batch, max_len), "generate() must run in the cache this test reserved"
    return plan, ids


def hypothetical_plan(dec, batch, max_len):
    from edgerunner_amd import native
    d = dec.dims
    p = native.ErDecodePlan()
    native.check(dec.lib.er_plan_decode(batch, d.num_heads, d.hidden_dim // d.num_heads, d.hidden_dim, max_len, p), "er_plan_decode")
    return {n: int(getattr(p, n)) for n, _ in native.ErDecodePlan._fields_}


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_reserved_shapes_keep_their_own_plan(small, precision, monkeypatch):
    from edgerunner_amd import native
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)

    def set_force(force):
        if force is None:
            monkeypatch.delenv("ER_FORCE_BATCHED", raising=False)
        else:
            monkeypatch.setenv("ER_FORCE_BATCHED", force)

    fresh = {}                       # one fresh context per distinct shape, each reserving only that shape
    for shape in dict.fromkeys(SHAPES):
        set_force(shape[2])
        dec = make_decoder(small, precision)
        fresh[shape] = reserve_and_decode(dec, shape[0], shape[1])
        dec.close()

    dec = make_decoder(small, precision)
    for step, shape in enumerate(SHAPES, 1):
        batch, max_len, force = shape
        set_force(force)
        plan, ids = reserve_and_decode(dec, batch, max_len)
        want = hypothetical_plan(dec, batch, max_len)
        print(f"{precision} shape {step} {shape}: plan {plan}")
        assert plan == want, f"shape {step} {shape}: er_ctx_plan {plan} != er_plan_decode {want}"
        assert plan == fresh[shape][0], f"shape {step} {shape}: plan differs from a fresh context's"
        assert ids.shape == (batch, 8)
        assert np.array_equal(ids, fresh[shape][1]), \
            f"shape {step} {shape}: ids {ids.tolist()} differ from a fresh context's {fresh[shape][1].tolist()}"
        if step == 3:
            assert plan["batched"] == 1, "ER_FORCE_BATCHED=1 at B = 1 runs the batched kernels"
        if step == 4:
            assert (plan["batched"], plan["decode_version"], plan["attn_kernel"]) == (0, 3, native.ER_ATTN_BALANCED), \
                "the forced shape before it must leave nothing behind"
    dec.close()
