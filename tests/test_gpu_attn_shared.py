"""The decode attention under prefix groups (csrc/k_attn_shared.h) through its unit entry ``er_k_attn_shared``: row b attends keys
[0, P) of its LEADER's cache slice and keys [P, len_b) of its own.  H = 16, D = 96, fp32 and fp16 cache, inputs drawn as
tests/test_gpu_kernels.py draws them; the bound is the one every decode attention kernel meets there."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H, D = 16, 96
NAN16 = 0x7E00


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def close(a, b, atol, rtol=0.0, what=""):
    a, b = a.double().cpu(), b.double().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol) | torch.isnan(a)
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} mismatches, max abs err {float(err.max()):.3e}, " \
                          f"first bad index {bad.nonzero()[0].tolist()}"
    return float(err.max()), float((err / tol).max())


def poison(kc, vc, leaders, P, lens):
    """NaN over every unused tail and over every follower's own [0, P): the leader's copy is what is read, and nothing else is."""
    for b, n in enumerate(lens):
        kc[b, :, n:] = float("nan")
        vc[b, :, n:] = float("nan")
        if leaders[b] != b:
            kc[b, :, :P] = float("nan")
            vc[b, :, :P] = float("nan")


def reference(q, kc, vc, leaders, P, lens):
    """float64 softmax attention over cat(leader prefix, own suffix), row by row (computed before the poisoning)."""
    out = []
    for b, n in enumerate(lens):
        k = torch.cat((kc[leaders[b], :, :P], kc[b, :, P:n]), dim=1).double()
        v = torch.cat((vc[leaders[b], :, :P], vc[b, :, P:n]), dim=1).double()
        w = torch.softmax(q[b].view(H, 1, D).double() @ k.transpose(1, 2) / math.sqrt(D), dim=-1)
        out.append((w @ v).reshape(H * D))
    return torch.stack(out)


LEADERS7 = [0, 0, 2, 0, 2, 5, 0]
SUFFIX7 = [0, 1, 2, 63, 64, 127, 130]


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 129, 2049])
def test_attn_shared_parity(P, half):
    """Seven rows in three groups (one of four rows, one of two, a singleton), suffixes from empty to more than one tile; P below, at
    and above the 64-key tile and the 128-key chunk, odd and even (the fp16 pair mapping starts tiles at even keys)."""
    from edgerunner_amd import kernels as K
    B = len(LEADERS7)
    lens = [P + s for s in SUFFIX7]
    Lcap = (max(lens) + 63) // 64 * 64
    q = rnd(B, H * D, seed=90)
    kc, vc = rnd(B, H, Lcap, D, seed=91), rnd(B, H, Lcap, D, seed=92)
    if half:
        kc, vc = kc.half(), vc.half()
    ref = reference(q, kc, vc, LEADERS7, P, lens)
    poison(kc, vc, LEADERS7, P, lens)
    out = K.attn_shared(q, kc, vc, lens, LEADERS7, P)
    worst = (0.0, 0.0)
    for b in range(B):
        worst = max(worst, close(out[b], ref[b], 2e-6, 1e-5, f"shared attn row {b} (leader {LEADERS7[b]}) P {P} len {lens[b]}"), key=lambda t: t[1])
    print(f"attn_shared P={P} {'fp16' if half else 'fp32'} cache: max |err| {worst[0]:.3e}, max err / bound {worst[1]:.3f}")


@pytest.fixture(scope="module", params=[False, True], ids=["f32", "f16"])
def one_row(request):
    """The row under test: q, its prefix (P = 257) and its suffix (131 keys), Lcap 512."""
    half = request.param
    P, S, Lcap = 257, 131, 512
    q = rnd(1, H * D, seed=93)
    kp, vp = rnd(H, P, D, seed=94), rnd(H, P, D, seed=95)
    ks, vs = rnd(H, S, D, seed=96), rnd(H, S, D, seed=97)
    if half:
        kp, vp, ks, vs = kp.half(), vp.half(), ks.half(), vs.half()
    return half, P, S, Lcap, q, kp, vp, ks, vs


def run_placed(one_row, B, leaders, row, twin=None, seed=100):
    """The row under test as row `row` of a batch of B (its group's leader holds the prefix; `twin`: a second row of the group with the
    same q and suffix); every other row gets its own q, prefix per group, suffix and length."""
    from edgerunner_amd import kernels as K
    half, P, S, Lcap, q1, kp, vp, ks, vs = one_row
    q = rnd(B, H * D, seed=seed)
    kc, vc = rnd(B, H, Lcap, D, seed=seed + 1), rnd(B, H, Lcap, D, seed=seed + 2)
    if half:
        kc, vc = kc.half(), vc.half()
    lens = [P + (37 * b) % 200 for b in range(B)]
    for r in (row,) + (() if twin is None else (twin,)):
        q[r] = q1[0]
        kc[r, :, P:P + S], vc[r, :, P:P + S] = ks, vs
        lens[r] = P + S
    kc[leaders[row], :, :P], vc[leaders[row], :, :P] = kp, vp
    poison(kc, vc, leaders, P, lens)
    out = K.attn_shared(q, kc, vc, lens, leaders, P)
    assert not torch.isnan(out).any()
    return out


def test_attn_shared_row_invariance_bits(one_row):
    """A row's output bits depend on its q, the prefix bits and its own suffix only: the same row as a singleton, as the follower in a
    group of 2, and as member 20 of a group of 33 inside a batch of 40 that holds other groups (33 rows cross any 16- or 32-row tile)."""
    alone = run_placed(one_row, 1, [0], 0)[0]
    pair = run_placed(one_row, 2, [0, 0], 1, seed=110)[1]
    # B = 40: rows 0..2 a group of three, row 3 a singleton, the group of 33 = row 4 and rows 6..37 (row 5 a singleton between them),
    # rows 38, 39 a pair; member 20 of the big group (counting its leader as member 0) is row 25
    leaders = [0, 0, 0, 3, 4, 5] + [4] * 32 + [38, 38]
    big = [b for b in range(40) if leaders[b] == 4]
    assert len(big) == 33 and big[20] == 25
    out = run_placed(one_row, 40, leaders, 25, twin=31, seed=120)
    assert torch.equal(alone, pair), f"singleton vs follower of a pair: max diff {float((alone - pair).abs().max()):.3e}"
    assert torch.equal(alone, out[25]), f"singleton vs member 20 of 33: max diff {float((alone - out[25]).abs().max()):.3e}"
    assert torch.equal(out[25], out[31]), "two rows of one group with equal q and equal suffix"


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("B", [7, 40])
def test_attn_shared_writes_tiled_image(B, half):
    """With out_xt the image holds hi = fp16(r), lo = fp16(r - hi) at the entries er_k_attn_stream_xt documents; rows the batch does not
    have are left alone."""
    from edgerunner_amd import kernels as K
    P = 65
    leaders = LEADERS7 if B == 7 else [0, 0, 0, 3, 4, 5] + [4] * 32 + [38, 38]
    lens = [P + (29 * b) % 140 for b in range(B)]
    Lcap = (max(lens) + 63) // 64 * 64
    q = rnd(B, H * D, seed=130)
    kc, vc = rnd(B, H, Lcap, D, seed=131), rnd(B, H, Lcap, D, seed=132)
    if half:
        kc, vc = kc.half(), vc.half()
    ref = reference(q, kc, vc, leaders, P, lens)
    poison(kc, vc, leaders, P, lens)
    img = torch.full(((B + 31) // 32, H * D // 4, 32, 8), NAN16, dtype=torch.int16, device=DEV).view(torch.float16)
    out = K.attn_shared(q, kc, vc, lens, leaders, P, out_xt=img)
    plain = K.attn_shared(q, kc, vc, lens, leaders, P)
    assert torch.equal(out, plain), "the row-major rows must not depend on out_xt"
    close(out, ref, 2e-6, 1e-5, "shared attn with out_xt")
    want = K.xt_pack_image(out)
    hi, lo = K.xt_unpack_image(want)
    rows = torch.arange(hi.shape[0], device=DEV) < B
    wh, wl = hi.view(torch.int16), lo.view(torch.int16)
    wh[~rows], wl[~rows] = NAN16, NAN16                           # rows the batch does not have: untouched
    gh, gl = K.xt_unpack_image(img)
    assert torch.equal(gh.view(torch.int16), wh) and torch.equal(gl.view(torch.int16), wl), "image != xt_pack(out), or a row >= B was written"


def test_attn_shared_refuses_bad_tables():
    from edgerunner_amd import kernels as K, native
    q = rnd(3, H * D, seed=140)
    kc, vc = rnd(3, H, 64, D, seed=141), rnd(3, H, 64, D, seed=142)
    for leaders, P, lens in (([0, 2, 2], 8, [9, 9, 9]),        # leader[1] > 1
                             ([0, 0, 1], 8, [9, 9, 9]),        # a chain: row 1 is led by row 0
                             ([0, 0, 0], 0, [9, 9, 9]),        # prefix_len < 1
                             ([0, 0, 0], 8, [9, 7, 9])):       # a row shorter than the prefix
        with pytest.raises(native.NativeError):
            K.attn_shared(q, kc, vc, lens, leaders, P)
