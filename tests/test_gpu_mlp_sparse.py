"""The fused single-row MLP (csrc/k_mlp_sparse.h) against the two launches it replaces, bit for bit.

``er_k_mlp_sparse`` runs one layer's fused launch + finish launch on caller-owned operands; the reference is the decode step's own
fc1 (LayerNorm prologue, ReLU epilogue) followed by fc2 (bias + residual epilogue) through ``er_k_gemv_form``.  ``y`` and ``h1`` must
be EQUAL AS BIT PATTERNS, for fp32 and for fp16 weights.  All at the kernel's fixed widths 1536 / 6144.

Which neurons are alive is steered through b1 (the pre-activations of these inputs have a standard deviation of about 0.8, so a bias
of +4 / -4 decides the sign); every case checks on the REFERENCE f that the pattern it meant is the pattern it got, and that the
kernel's own count of live neurons per workgroup agrees with it.  Chain c = slice * 64 + lane owns the neurons
k(i) = slice * 1536 + (i // EPL * 64 + lane) * EPL + i % EPL, i = 0..23 (EPL = 4 for fp32 weights, 8 for fp16: csrc/er_mlp_map.h).

The end-to-end test runs a 2-layer model with ER_MLP_V=0 and ER_MLP_V=1: 48 greedy tokens must be the same ids and the logits
behind the last step the same bits."""
import dataclasses
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HID, INTER, CHAIN, WGS = 1536, 6144, 24, 256


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


@functools.lru_cache(maxsize=None)
def data(half):
    from edgerunner_amd import kernels
    d = SimpleNamespace()
    cast = (lambda t: t.half()) if half else (lambda t: t)
    d.w1, d.w2 = cast(rnd(INTER, HID, seed=201, scale=0.02)), cast(rnd(HID, INTER, seed=202, scale=0.02))
    d.b1, d.b2 = rnd(INTER, seed=203, scale=0.02), rnd(HID, seed=204, scale=0.02)
    d.x = rnd(1, HID, seed=205) * 2 + 0.3
    d.lw, d.lb = 1 + 0.1 * rnd(HID, seed=206), 0.05 * rnd(HID, seed=207)
    d.w2t = kernels.mlp_transpose(d.w2)
    torch.cuda.synchronize()
    assert torch.equal(d.w2t, d.w2.t().contiguous()), "er_k_mlp_transpose is not the transpose"
    return d


def neuron(epl, wg, i):
    return (wg >> 6) * HID + ((i // epl) * 64 + (wg & 63)) * epl + i % epl


def chain_neurons(half):
    """[256, 24] neuron ids: row c = the chain of workgroup c in chain order"""
    epl = 8 if half else 4
    return torch.tensor([[neuron(epl, c, i) for i in range(CHAIN)] for c in range(WGS)], device=DEV)


def reference(d, b1, half):
    """today's two launches: (h1, f, y)"""
    from edgerunner_amd import kernels, native
    r1 = kernels.gemv_form(native.ER_FORM_ROW, native.ER_EPI_RELU, d.w1, 1, x=d.x, bias=b1, ln=(d.lw, d.lb), nw=4, rw=2, return_xnorm=True)
    r2 = kernels.gemv_form(native.ER_FORM_ROW, native.ER_EPI_RESID, d.w2, 1, x=r1["y"], bias=d.b2, resid=r1["xnorm"], nw=4, rw=2)
    return r1["xnorm"].reshape(-1), r1["y"].reshape(-1), r2["y"].reshape(-1)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check(d, b1, half, want_alive=None):
    """run the fused pair, compare with the reference bit for bit; want_alive: bool [6144] the case meant to produce"""
    from edgerunner_amd import kernels
    h1, f, y = reference(d, b1, half)
    alive = f != 0
    if want_alive is not None:
        assert torch.equal(alive, want_alive), "the case's b1 did not produce the zero pattern it was built for"
    m = kernels.MlpSparse(d.w1, b1, d.w2t, d.b2, d.x, d.lw, d.lb)
    m.part.fill_(float("nan"))
    m.launch()
    torch.cuda.synchronize()
    assert not torch.isnan(m.part).any(), "a word of the partial block was not written"
    assert torch.equal(m.nnz.long(), alive[chain_neurons(half)].sum(1)), "live neurons per workgroup"
    assert same_bits(m.h1, h1), "h1 (LayerNorm row) differs from fc1's"
    assert same_bits(m.y, y), f"y differs from fc2's: max |diff| {(m.y - y).abs().max().item():.3e}"
    return alive


PREC = pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])


@PREC
def test_random_operands(half):
    d = data(half)
    alive = check(d, d.b1, half)
    z = 1.0 - alive.float().mean().item()
    print(f"zero fraction {z:.4f}")
    assert 0.4 < z < 0.6


@PREC
def test_no_zero_neuron(half):
    d = data(half)
    check(d, torch.full_like(d.b1, 4.0), half, torch.ones(INTER, dtype=torch.bool, device=DEV))


@PREC
def test_every_neuron_zero(half):
    from edgerunner_amd import kernels
    d = data(half)
    b1 = torch.full_like(d.b1, -4.0)
    check(d, b1, half, torch.zeros(INTER, dtype=torch.bool, device=DEV))
    m = kernels.MlpSparse(d.w1, b1, d.w2t, d.b2, d.x, d.lw, d.lb)
    m.launch()
    torch.cuda.synchronize()
    assert same_bits(m.y, (torch.zeros_like(d.b2) + d.b2) + m.h1), "all dead: y = ((0) + b2) + h1"


@PREC
@pytest.mark.parametrize("place", [0, 11, 12, 23])
def test_one_live_neuron_per_chain(half, place):
    d = data(half)
    want = torch.zeros(INTER, dtype=torch.bool, device=DEV)
    want[chain_neurons(half)[:, place]] = True
    check(d, torch.where(want, 4.0, -4.0).float(), half, want)


@PREC
def test_live_chain_between_dead_chains(half):
    d = data(half)
    ch = chain_neurons(half)
    b1 = d.b1.clone()
    c = 70                                    # slice 1, lane 6
    b1[ch[c]] = 4.0
    b1[ch[c - 1]] = -4.0
    b1[ch[c + 1]] = -4.0
    alive = check(d, b1, half)
    assert alive[ch[c]].all() and not alive[ch[c - 1]].any() and not alive[ch[c + 1]].any()


@PREC
def test_graph_replay_over_nan_partials(half):
    """the launch pair captured once, replayed twice over a partial block pre-filled with NaN"""
    from edgerunner_amd import kernels
    d = data(half)
    _, _, y = reference(d, d.b1, half)
    m = kernels.MlpSparse(d.w1, d.b1, d.w2t, d.b2, d.x, d.lw, d.lb)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.launch()                            # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m.launch()
    for _ in range(2):
        m.part.fill_(float("nan"))
        m.y.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert not torch.isnan(m.part).any()
        assert same_bits(m.y, y)


@pytest.fixture(scope="module")
def small():
    from edgerunner_amd import weights as W
    from edgerunner_amd.options import config_defaults
    opt = dataclasses.replace(config_defaults["ArAE"], num_layers=2, generate_mode="greedy")
    return opt, W.make_state_dict(opt, 0, "perturbed")


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_generation_is_unchanged_by_the_fused_mlp(small, precision, monkeypatch):
    from edgerunner_amd.models import LMM
    opt, sd = small
    got = {}
    for v in ("0", "1"):
        monkeypatch.setenv("ER_MLP_V", v)
        lmm = LMM(opt, DEV, precision=precision)
        lmm.load_state_dict(sd, strict=True)
        dec = lmm.mesh_decoder
        dec.reserve(1, 64)
        prefix = torch.tensor([[(11 + 5 * j) % (dec.dims.vocab_size - 3) + 3 for j in range(4)]], dtype=torch.long)
        ids = dec.generate(dec.embd(prefix), max_new_tokens=48, min_new_tokens=48).cpu().numpy()
        logits = dec.logits().clone()
        nnz = dec.mlp_nnz() if v == "1" else None
        torch.cuda.synchronize()
        got[v] = (ids, logits, nnz)
        dec.close()
    assert got["0"][0].shape == (1, 48)
    assert np.array_equal(got["0"][0], got["1"][0]), "greedy ids differ"
    assert same_bits(got["0"][1], got["1"][1]), "logits behind the last step differ"
    nnz = got["1"][2]
    assert nnz.shape == (2, 256) and nnz.min() >= 0 and nnz.max() <= CHAIN and nnz.sum() > 0
    print(f"{precision}: zero fraction per layer {[round(1 - float(n.sum()) / INTER, 4) for n in nnz]}")
