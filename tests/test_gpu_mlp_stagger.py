"""The fused single-row MLP's two half-chains (csrc/k_mlp_sparse.h: group A = places 0-11, group B = places 12-23 of a chain, each
half requesting only its live fc2 rows in blocks of four slots, csrc/er_mlp_map.h) through ``kernels.MlpSparse`` against fc1 + fc2 of
the row kernels (``kernels.gemv_form``), bit for bit.

``y`` and ``h1`` must be EQUAL AS BIT PATTERNS, ``nnz`` must be the reference's count of live neurons per chain, and the partial block,
pre-filled with NaN, must come back fully written; for fp32 and for fp16 weights, at the kernel's only shape (1536 / 6144).  Which
places of a chain are alive is steered through b1 = +4 / -4 (the pre-activations of these inputs have a standard deviation of about
0.8); every case checks on the REFERENCE f that the pattern it meant is the pattern it got.  The cases walk the live count of a half
over every block count (0, 1-4, 5-8, 9-12 live places = 0, 1, 2, 3 blocks) and both sides of every block edge, with the live places
at the start or at the end of the half, and once with every count of both halves in one grid."""
import functools
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HID, INTER, CHAIN, HALF, WGS = 1536, 6144, 24, 12, 256
COUNTS = [0, 1, 3, 4, 5, 8, 9, 11, 12]


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
def data(half):
    from edgerunner_amd import kernels
    d = SimpleNamespace()
    cast = (lambda t: t.half()) if half else (lambda t: t)
    d.w1, d.w2 = cast(rnd(INTER, HID, seed=301, scale=0.02)), cast(rnd(HID, INTER, seed=302, scale=0.02))
    d.b2 = rnd(HID, seed=304, scale=0.02)
    d.x = rnd(1, HID, seed=305) * 2 + 0.3
    d.lw, d.lb = 1 + 0.1 * rnd(HID, seed=306), 0.05 * rnd(HID, seed=307)
    d.w2t = kernels.mlp_transpose(d.w2)
    torch.cuda.synchronize()
    return d


def places(case):
    """bool [256, 24]: the live places of every chain"""
    kind, n = case
    p = torch.zeros(WGS, CHAIN, dtype=torch.bool)
    if kind == "first_start":
        p[:, :n] = True
    elif kind == "first_end":
        p[:, HALF - n:HALF] = True
    elif kind == "second_start":
        p[:, HALF:HALF + n] = True
    elif kind == "second_end":
        p[:, CHAIN - n:] = True
    elif kind == "mixed":                      # chain c: c mod 13 live places in the first half, 7c mod 13 in the second, at seeded places
        g = torch.Generator().manual_seed(977)
        for c in range(WGS):
            p[c, torch.randperm(HALF, generator=g)[:c % 13]] = True
            p[c, HALF + torch.randperm(HALF, generator=g)[:(7 * c) % 13]] = True
    else:
        raise ValueError(kind)
    return p.to(DEV)


@functools.lru_cache(maxsize=None)
def reference(half, case):
    """the two launches of the row kernels: (b1, want_alive [6144], h1, f, y); computed once per case and left unchanged"""
    from edgerunner_amd import kernels, native
    d = data(half)
    want = torch.zeros(INTER, dtype=torch.bool, device=DEV)
    want[chain_neurons(half)[places(case)]] = True
    b1 = torch.where(want, 4.0, -4.0).float()
    r1 = kernels.gemv_form(native.ER_FORM_ROW, native.ER_EPI_RELU, d.w1, 1, x=d.x, bias=b1, ln=(d.lw, d.lb), nw=4, rw=2, return_xnorm=True)
    r2 = kernels.gemv_form(native.ER_FORM_ROW, native.ER_EPI_RESID, d.w2, 1, x=r1["y"], bias=d.b2, resid=r1["xnorm"], nw=4, rw=2)
    torch.cuda.synchronize()
    f = r1["y"].reshape(-1)
    assert torch.equal(f != 0, want), "the case's b1 did not produce the zero pattern it was built for"
    return b1, want, r1["xnorm"].reshape(-1).clone(), f.clone(), r2["y"].reshape(-1).clone()


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def fused(half, case):
    from edgerunner_amd import kernels
    d = data(half)
    b1 = reference(half, case)[0]
    return kernels.MlpSparse(d.w1, b1, d.w2t, d.b2, d.x, d.lw, d.lb)


def verify(m, half, case):
    _, want, h1, _, y = reference(half, case)
    assert not torch.isnan(m.part).any(), "a word of the partial block was not written"
    assert torch.equal(m.nnz.long(), want[chain_neurons(half)].sum(1)), "live neurons per chain"
    assert same_bits(m.h1, h1), "h1 (LayerNorm row) differs from fc1's"
    assert same_bits(m.y, y), f"y differs from fc2's: max |diff| {(m.y - y).abs().max().item():.3e}"


def check(half, case):
    m = fused(half, case)
    m.part.fill_(float("nan"))
    m.launch()
    torch.cuda.synchronize()
    verify(m, half, case)


PREC = pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])


@PREC
@pytest.mark.parametrize("n", COUNTS)
def test_first_half_live_from_its_start(half, n):
    check(half, ("first_start", n))


@PREC
@pytest.mark.parametrize("n", COUNTS)
def test_second_half_live_from_its_start(half, n):
    check(half, ("second_start", n))


@PREC
@pytest.mark.parametrize("n", COUNTS)
def test_first_half_live_at_its_end(half, n):
    check(half, ("first_end", n))


@PREC
@pytest.mark.parametrize("n", COUNTS)
def test_second_half_live_at_its_end(half, n):
    check(half, ("second_end", n))


@PREC
def test_every_count_of_both_halves_in_one_grid(half):
    case = ("mixed", 0)
    p = places(case)
    a, b = p[:, :HALF].sum(1).cpu(), p[:, HALF:].sum(1).cpu()
    assert set(a.tolist()) == set(range(13)) and set(b.tolist()) == set(range(13)), "every live count of both halves"
    want = reference(half, case)[1]
    assert torch.equal(want[chain_neurons(half)].sum(1).cpu(), a + b)
    check(half, case)                          # nnz per chain included


@PREC
def test_group_a_all_live_group_b_all_dead(half):
    check(half, ("first_start", HALF))


@PREC
def test_group_a_all_dead_group_b_all_live(half):
    check(half, ("second_start", HALF))


@PREC
def test_mixed_counts_in_a_graph_replayed_over_nan(half):
    """the launch pair captured once, replayed twice over a partial block and a y pre-filled with NaN"""
    case = ("mixed", 0)
    m = fused(half, case)
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
        m.nnz.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        verify(m, half, case)
