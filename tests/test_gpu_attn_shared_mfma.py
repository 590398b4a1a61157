"""The matrix-core prefix pass of the shared-prefix decode attention (csrc/k_attn_shared_mfma.h) through its unit entry
``er_k_attn_shared_mfma`` (``kernels.attn_shared(prefix_pass="mfma")``): attn_prefix_mfma_kernel in front of the unchanged suffix / merge
launch.  H = 16, D = 96, fp16 cache; inputs, poisoning, the float64 reference and the bound are those of tests/test_gpu_attn_shared.py.

Wave w of a workgroup owns keys 32 w .. 32 w + 31 of a 128-key chunk and a row tile is 32 rows, so P runs below, at and above 32 and
128, odd and even, and the groups reach past one row tile."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_attn_shared import DEV, H, D, NAN16, LEADERS7, SUFFIX7, rnd, close, poison, reference  # noqa: E402

pytestmark = pytest.mark.gpu

ATOL, RTOL = 2e-6, 1e-5          # the project's bound for every decode attention kernel
PS = [1, 31, 32, 33, 127, 128, 129, 2049]
LEADERS40 = [0, 0, 0, 3, 4, 5] + [4] * 32 + [38, 38]      # a group of 33 = row 4 and rows 6..37: member m >= 1 is row 5 + m


@functools.lru_cache(maxsize=None)
def case(P):
    """The parity inputs for one P, computed once: seven rows in groups [0, 0, 2, 0, 2, 5, 0], suffixes 0 .. 130, every row's q at its
    own scale (a swapped row or head then misses the bound by far), the float64 reference, and both passes' outputs."""
    from edgerunner_amd import kernels as K
    B = len(LEADERS7)
    lens = [P + s for s in SUFFIX7]
    Lcap = (max(lens) + 63) // 64 * 64
    q = rnd(B, H * D, seed=190) * torch.tensor([0.75 + 0.125 * b for b in range(B)], device=DEV).view(B, 1)
    kc, vc = rnd(B, H, Lcap, D, seed=191).half(), rnd(B, H, Lcap, D, seed=192).half()
    ref = reference(q, kc, vc, LEADERS7, P, lens)
    poison(kc, vc, LEADERS7, P, lens)
    mfma = K.attn_shared(q, kc, vc, lens, LEADERS7, P, prefix_pass="mfma")
    valu = K.attn_shared(q, kc, vc, lens, LEADERS7, P, prefix_pass="valu")
    return lens, ref, mfma, valu


@pytest.mark.parametrize("P", PS)
def test_attn_shared_mfma_parity(P):
    lens, ref, out, _ = case(P)
    worst = (0.0, 0.0)
    for b in range(len(LEADERS7)):
        worst = max(worst, close(out[b], ref[b], ATOL, RTOL, f"mfma prefix pass row {b} (leader {LEADERS7[b]}) P {P} len {lens[b]}"),
                    key=lambda t: t[1])
    print(f"attn_shared mfma P={P}: max |err| {worst[0]:.3e}, max err / bound {worst[1]:.3f}")


@pytest.mark.parametrize("P", PS)
def test_attn_shared_mfma_agrees_with_the_valu_pass(P):
    """Both passes meet the bound against float64, so they are within twice the bound of each other."""
    _, ref, mfma, valu = case(P)
    err = (mfma.double() - valu.double()).abs().cpu()
    tol = 2 * (ATOL + RTOL * ref.abs().cpu())
    print(f"attn_shared mfma vs valu P={P}: max |diff| {float(err.max()):.3e}, max diff / bound {float((err / tol).max()):.3f}")
    assert not torch.isnan(mfma).any() and not (err > tol).any(), f"P {P}: first bad index {(err > tol).nonzero()[:1].tolist()}"


@pytest.fixture(scope="module")
def one_row():
    """The row under test: q, its prefix (P = 257) and its suffix (131 keys), Lcap 512."""
    P, S, Lcap = 257, 131, 512
    return (P, S, Lcap, rnd(1, H * D, seed=193), rnd(H, P, D, seed=194).half(), rnd(H, P, D, seed=195).half(),
            rnd(H, S, D, seed=196).half(), rnd(H, S, D, seed=197).half())


def run_placed(one_row, B, leaders, rows, seed):
    """The row under test as every row of `rows` (all of one group, whose leader holds the prefix); every other row gets its own q,
    prefix per group, suffix and length."""
    from edgerunner_amd import kernels as K
    P, S, Lcap, q1, kp, vp, ks, vs = one_row
    q = rnd(B, H * D, seed=seed)
    kc, vc = rnd(B, H, Lcap, D, seed=seed + 1).half(), rnd(B, H, Lcap, D, seed=seed + 2).half()
    lens = [P + (37 * b) % 200 for b in range(B)]
    for r in rows:
        q[r] = q1[0]
        kc[r, :, P:P + S], vc[r, :, P:P + S] = ks, vs
        lens[r] = P + S
    kc[leaders[rows[0]], :, :P], vc[leaders[rows[0]], :, :P] = kp, vp
    poison(kc, vc, leaders, P, lens)
    out = K.attn_shared(q, kc, vc, lens, leaders, P, prefix_pass="mfma")
    assert not torch.isnan(out).any()
    return out


def test_attn_shared_mfma_row_invariance_bits(one_row):
    """A row's output bits depend on its q, the prefix bits and its own suffix only: the same row as a singleton, as the follower of a
    pair, and as members 20, 31 and 32 of a group of 33 inside a batch of 40 that holds other groups - 31 is the last column of the
    group's first row tile, 32 the first (and only live) column of its second."""
    alone = run_placed(one_row, 1, [0], [0], seed=200)[0]
    pair = run_placed(one_row, 2, [0, 0], [1], seed=210)[1]
    big = [b for b in range(40) if LEADERS40[b] == 4]
    assert len(big) == 33 and (big[20], big[31], big[32]) == (25, 36, 37)
    out = run_placed(one_row, 40, LEADERS40, [25, 36, 37], seed=220)
    assert torch.equal(alone, pair), f"singleton vs follower of a pair: max diff {float((alone - pair).abs().max()):.3e}"
    for m, r in ((20, 25), (31, 36), (32, 37)):
        assert torch.equal(alone, out[r]), f"singleton vs member {m} of 33: max diff {float((alone - out[r]).abs().max()):.3e}"


@pytest.mark.parametrize("B", [7, 40])
def test_attn_shared_mfma_writes_tiled_image(B):
    """With out_xt the image equals xt_pack_image(out), rows the batch does not have are left alone, and out does not depend on out_xt."""
    from edgerunner_amd import kernels as K
    P = 65
    leaders = LEADERS7 if B == 7 else LEADERS40
    lens = [P + (29 * b) % 140 for b in range(B)]
    Lcap = (max(lens) + 63) // 64 * 64
    q = rnd(B, H * D, seed=230)
    kc, vc = rnd(B, H, Lcap, D, seed=231).half(), rnd(B, H, Lcap, D, seed=232).half()
    ref = reference(q, kc, vc, leaders, P, lens)
    poison(kc, vc, leaders, P, lens)
    img = torch.full(((B + 31) // 32, H * D // 4, 32, 8), NAN16, dtype=torch.int16, device=DEV).view(torch.float16)
    out = K.attn_shared(q, kc, vc, lens, leaders, P, out_xt=img, prefix_pass="mfma")
    plain = K.attn_shared(q, kc, vc, lens, leaders, P, prefix_pass="mfma")
    assert torch.equal(out, plain), "the row-major rows must not depend on out_xt"
    close(out, ref, ATOL, RTOL, "mfma prefix pass with out_xt")
    hi, lo = K.xt_unpack_image(K.xt_pack_image(out))
    rows = torch.arange(hi.shape[0], device=DEV) < B
    wh, wl = hi.view(torch.int16), lo.view(torch.int16)
    wh[~rows], wl[~rows] = NAN16, NAN16                           # rows the batch does not have: untouched
    gh, gl = K.xt_unpack_image(img)
    assert torch.equal(gh.view(torch.int16), wh) and torch.equal(gl.view(torch.int16), wl), "image != xt_pack(out), or a row >= B was written"


def test_attn_shared_mfma_refusals():
    """fp32 and byte caches are ER_ERR_UNSUPPORTED; the bad tables er_k_attn_shared refuses are refused here too."""
    from edgerunner_amd import kernels as K, native
    q = rnd(3, H * D, seed=240)
    kc, vc = rnd(3, H, 64, D, seed=241), rnd(3, H, 64, D, seed=242)
    for k, v in ((kc, vc), (kc.to(torch.uint8), vc.to(torch.uint8))):
        with pytest.raises(native.NativeError) as e:
            K.attn_shared(q, k, v, [9, 9, 9], [0, 0, 0], 8, prefix_pass="mfma")
        assert "(-5)" in str(e.value), str(e.value)
    kc, vc = kc.half(), vc.half()
    for leaders, P, lens in (([0, 2, 2], 8, [9, 9, 9]),        # leader[1] > 1
                             ([0, 0, 1], 8, [9, 9, 9]),        # a chain: row 1 is led by row 0
                             ([0, 0, 0], 0, [9, 9, 9]),        # prefix_len < 1
                             ([0, 0, 0], 8, [9, 7, 9])):       # a row shorter than the prefix
        with pytest.raises(native.NativeError):
            K.attn_shared(q, kc, vc, lens, leaders, P, prefix_pass="mfma")
    with pytest.raises(ValueError):
        K.attn_shared(q, kc, vc, [9, 9, 9], [0, 0, 0], 8, prefix_pass="tensor")
    out = K.attn_shared(q, kc, vc, [9, 9, 9], [0, 0, 0], 8, prefix_pass="mfma")      # the same table, well formed, runs
    assert not torch.isnan(out).any()
