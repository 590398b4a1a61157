"""The fused MLP's finish launch (csrc/k_mlp_sparse.h, mlp_finish_kernel: 32 outputs per workgroup, the chain vectors read as whole
128-byte lines) through ``er_k_mlp_sparse`` against fc1 + fc2 of the row kernels, bit for bit.  The forms with 8 and 16 outputs per
workgroup and a write-through store of the chain vectors passed the same cases before they were dropped.

The reference is the one of tests/test_gpu_mlp_sparse.py: the decode step's own fc1 (LayerNorm prologue, ReLU epilogue) followed by fc2
(bias + residual epilogue) through ``er_k_gemv_form``; ``y`` and ``h1`` must be EQUAL AS BIT PATTERNS, for fp32 and for fp16 weights, at
the kernel's fixed widths 1536 / 6144.  A reference is computed once per (precision, case).

The finish adds the 64 chain values of a slice in the order of the row kernel's butterfly (chain index xor 32, 16, 8, 4, 2, 1), partly
as adds of a lane's own registers, partly across lanes (csrc/er_mlp_map.h).  The cases are chosen so that a wrong pairing or a wrong
chain address shows: chain vectors whose magnitudes differ by powers of two between 2^-12 and 2^12 (any other association rounds
differently), a single live chain per slice at the lanes where the pairing changes hands (0, 63, 31 | 32), nothing alive, and a block
of partial vectors that holds NaN or the previous launch's values when the pair runs."""
import functools
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HID, INTER, CHAIN, WGS = 1536, 6144, 24, 256

PREC = pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def neuron(epl, wg, i):
    return (wg >> 6) * HID + ((i // epl) * 64 + (wg & 63)) * epl + i % epl


@functools.lru_cache(maxsize=None)
def chain_neurons(half):
    """[256, 24] neuron ids: row c = the chain of workgroup c in chain order"""
    epl = 8 if half else 4
    return torch.tensor([[neuron(epl, c, i) for i in range(CHAIN)] for c in range(WGS)], device=DEV)


@functools.lru_cache(maxsize=None)
def data(half, scaled=False):
    """scaled: the fc2 weights of chain c (24 rows of W2T) times 2^e(c), e = -12 .. 12, far apart for neighbouring chains"""
    from edgerunner_amd import kernels
    d = SimpleNamespace()
    cast = (lambda t: t.half()) if half else (lambda t: t)
    w2 = rnd(HID, INTER, seed=212, scale=0.02)
    if scaled:
        e = (torch.arange(WGS, device=DEV) * 7) % 25 - 12
        col = torch.empty(INTER, device=DEV)
        col[chain_neurons(half).reshape(-1)] = torch.pow(2.0, e.float()).repeat_interleave(CHAIN)
        w2 = w2 * col
    d.w1, d.w2 = cast(rnd(INTER, HID, seed=211, scale=0.02)), cast(w2)
    d.b1, d.b2 = rnd(INTER, seed=213, scale=0.02), rnd(HID, seed=214, scale=0.02)
    d.x = rnd(1, HID, seed=215) * 2 + 0.3
    d.lw, d.lb = 1 + 0.1 * rnd(HID, seed=216), 0.05 * rnd(HID, seed=217)
    d.w2t = kernels.mlp_transpose(d.w2)
    torch.cuda.synchronize()
    assert torch.equal(d.w2t, d.w2.t().contiguous())
    return d


def bias_for(half, case):
    """b1 of a named case (the pre-activations have a standard deviation of about 0.8: +4 / -4 decides the sign)"""
    d = data(half)
    if case == "random":
        return d.b1
    if case == "other":
        return rnd(INTER, seed=301, scale=0.5)
    if case == "dead":
        return torch.full_like(d.b1, -4.0)
    kind, lane = case.split(":")
    assert kind == "lane"
    b1 = torch.full_like(d.b1, -4.0)
    for s in range(4):
        b1[chain_neurons(half)[s * 64 + int(lane)]] = 4.0
    return b1


@functools.lru_cache(maxsize=None)
def reference(half, scaled, case):
    """today's two row launches, once per (precision, weights, case): (h1, f, y)"""
    from edgerunner_amd import kernels, native
    d, b1 = data(half, scaled), bias_for(half, case)
    r1 = kernels.gemv_form(native.ER_FORM_ROW, native.ER_EPI_RELU, d.w1, 1, x=d.x, bias=b1, ln=(d.lw, d.lb), nw=4, rw=2, return_xnorm=True)
    r2 = kernels.gemv_form(native.ER_FORM_ROW, native.ER_EPI_RESID, d.w2, 1, x=r1["y"], bias=d.b2, resid=r1["xnorm"], nw=4, rw=2)
    torch.cuda.synchronize()
    return r1["xnorm"].reshape(-1).clone(), r1["y"].reshape(-1).clone(), r2["y"].reshape(-1).clone()


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check(half, case, scaled=False):
    """run the fused pair over a block of NaN, compare with the reference bit for bit"""
    from edgerunner_amd import kernels
    d, b1 = data(half, scaled), bias_for(half, case)
    h1, f, y = reference(half, scaled, case)
    alive = f != 0
    m = kernels.MlpSparse(d.w1, b1, d.w2t, d.b2, d.x, d.lw, d.lb)
    m.part.fill_(float("nan"))
    m.y.fill_(float("nan"))
    m.launch()
    torch.cuda.synchronize()
    assert not torch.isnan(m.part).any(), "a word of the partial block was not written"
    assert torch.equal(m.nnz.long(), alive[chain_neurons(half)].sum(1)), "live neurons per workgroup"
    assert same_bits(m.h1, h1), "h1 (LayerNorm row) differs from fc1's"
    assert same_bits(m.y, y), f"y differs from fc2's: max |diff| {(m.y - y).abs().max().item():.3e}"
    return alive, m


@PREC
def test_random_operands(half):
    alive, _ = check(half, "random")
    assert 0.4 < 1.0 - alive.float().mean().item() < 0.6


@PREC
def test_chains_scaled_by_powers_of_two(half):
    """chain vectors between 2^-12 and 2^12 times the usual size: the sum's association decides the low bits"""
    alive, m = check(half, "random", scaled=True)
    mag = m.part.abs().amax(1)
    assert mag.max() / mag[mag > 0].min() > 2.0 ** 16, "the chain vectors do not span the magnitudes the case was built for"


@PREC
def test_every_neuron_dead(half):
    alive, m = check(half, "dead")
    assert not alive.any()
    assert same_bits(m.y, (torch.zeros_like(m.h1) + data(half).b2) + m.h1), "all dead: y = ((0) + b2) + h1"


@PREC
@pytest.mark.parametrize("lane", [0, 63, 31, 32])
def test_one_live_chain_per_slice(half, lane):
    """lanes 31 | 32 differ in bit 5: the first level of the tree, an add of two of a lane's own registers"""
    alive, m = check(half, f"lane:{lane}")
    want = torch.zeros(INTER, dtype=torch.bool, device=DEV)
    for s in range(4):
        want[chain_neurons(half)[s * 64 + lane]] = True
    assert torch.equal(alive, want), "the case's b1 did not produce the zero pattern it was built for"
    live_rows = (m.part != 0).any(1).nonzero().reshape(-1).tolist()
    assert live_rows == [s * 64 + lane for s in range(4)]


@PREC
def test_graph_with_two_bias_patterns_reads_no_stale_line(half):
    """ONE captured graph: [pattern A into b1, launch pair, y out, pattern B into b1, launch pair, y out], replayed three times.  The
    block of partial vectors is never cleared in between: every finish must see the values of the fused launch right in front of it,
    not lines of the launch before."""
    from edgerunner_amd import kernels
    d = data(half)
    pa, pb = bias_for(half, "random"), bias_for(half, "other")
    ya, yb = reference(half, False, "random")[2], reference(half, False, "other")[2]
    assert not same_bits(ya, yb)
    b1 = pa.clone()
    m = kernels.MlpSparse(d.w1, b1, d.w2t, d.b2, d.x, d.lw, d.lb)
    out_a, out_b = torch.empty_like(m.y), torch.empty_like(m.y)

    def sequence():
        b1.copy_(pa)
        m.launch()
        out_a.copy_(m.y)
        b1.copy_(pb)
        m.launch()
        out_b.copy_(m.y)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sequence()                            # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sequence()
    for rep in range(3):
        out_a.fill_(float("nan"))
        out_b.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(out_a, ya), f"replay {rep}: pattern A"
        assert same_bits(out_b, yb), f"replay {rep}: pattern B"
