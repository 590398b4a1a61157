"""kv_fork_kernel (csrc/k_kv_fork.h) through its unit entry er_k_kv_fork: positions [0, len) of K and V, every layer and head, copied
from source rows to destination rows of caches full of random bytes - and nothing else written.  Shapes: 2 layers, 6 rows, 2 heads, 64
positions (one head's slab is 16 bytes .. 24 KB: below one lane round, below and above one piece of 4 x 256 x 16 bytes, with and without
a rest).  Pairs 0 -> {1, 3}, 2 -> {4}; row 5 is in no pair."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LAYERS, B, H, LCAP = 2, 6, 2, 64
SRC, DST = [0, 0, 2], [1, 3, 4]
SHAPES = [(96, 4), (96, 2), (96, 1), (64, 4)]          # (head_dim, element size)
LENS = [1, 31, 33, 64]
ER_ERR_INVALID = -1


def caches(head_dim, esz, seed):
    """K and V [layers, B, H, Lcap, D] in the dtype of that element size, every byte random (NaN patterns included: bytes are bytes)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    dtype = {4: torch.float32, 2: torch.float16, 1: torch.uint8}[esz]
    raw = torch.randint(0, 256, (2, LAYERS, B, H, LCAP, head_dim * esz), dtype=torch.uint8, generator=g).to(DEV)
    k, v = (raw[i].view(dtype).contiguous() for i in range(2))
    assert k.shape == (LAYERS, B, H, LCAP, head_dim) and k.element_size() == esz
    return k, v


def as_bytes(t):
    return t.view(torch.uint8)


def expected(before, length):
    """The cache the fork must leave: destinations' [0, length) from their sources, every other byte as before."""
    want = before.clone()
    for s, d in zip(SRC, DST):
        want[:, d, :, :length] = before[:, s, :, :length]
    return want


@pytest.mark.parametrize("length", LENS)
@pytest.mark.parametrize("head_dim,esz", SHAPES)
def test_fork_copies_the_slabs_and_nothing_else(head_dim, esz, length):
    from edgerunner_amd import kernels
    k, v = caches(head_dim, esz, 1000 * head_dim + 10 * esz + length)
    k0, v0 = k.clone(), v.clone()
    kernels.kv_fork(k, v, SRC, DST, length)
    torch.cuda.synchronize()
    for name, got, before in (("K", k, k0), ("V", v, v0)):
        gb, bb = as_bytes(got), as_bytes(before)
        for s, d in zip(SRC, DST):
            assert torch.equal(gb[:, d, :, :length], bb[:, s, :, :length]), f"{name}: row {d} [0, {length}) is not row {s}'s"
            assert torch.equal(gb[:, d, :, length:], bb[:, d, :, length:]), f"{name}: row {d} was written at or behind position {length}"
        for r in (0, 2, 5):
            assert torch.equal(gb[:, r], bb[:, r]), f"{name}: row {r} (a source / in no pair) changed"
        assert torch.equal(gb, as_bytes(expected(before, length)))


@pytest.mark.parametrize("head_dim,esz,length", [(96, 2, 33), (96, 1, 64), (64, 4, 31)])
def test_captured_launch_replays_the_same_bytes(head_dim, esz, length):
    from edgerunner_amd import kernels
    k, v = caches(head_dim, esz, 77 + length)
    k0, v0 = k.clone(), v.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        kernels.kv_fork(k, v, SRC, DST, length)          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager_k, eager_v = k.clone(), v.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        kernels.kv_fork(k, v, SRC, DST, length)
    for _ in range(2):
        k.copy_(k0)
        v.copy_(v0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(as_bytes(k), as_bytes(eager_k)) and torch.equal(as_bytes(v), as_bytes(eager_v))
    assert torch.equal(as_bytes(k), as_bytes(expected(k0, length)))


def test_more_destinations_than_one_launch_holds():
    """70 followers of one source and 70 sources of one follower each: the table is cut into launches of 64 groups / 64 destinations."""
    from edgerunner_amd import kernels
    g = torch.Generator(device="cpu").manual_seed(5)
    rows = 1 + 70 + 140
    raw = torch.randint(0, 256, (2, 1, rows, 1, 32, 64), dtype=torch.uint8, generator=g).to(DEV)
    k, v = raw[0].contiguous(), raw[1].contiguous()          # [1, rows, 1, 32, 64] bytes
    k0, v0 = k.clone(), v.clone()
    src = [0] * 70 + list(range(71, 141))
    dst = list(range(1, 71)) + list(range(141, 211))
    kernels.kv_fork(k, v, src, dst, 17)
    torch.cuda.synchronize()
    for got, before in ((k, k0), (v, v0)):
        want = before.clone()
        for s, d in zip(src, dst):
            want[:, d, :, :17] = before[:, s, :, :17]
        assert torch.equal(got, want)


def test_refusals_change_nothing():
    from edgerunner_amd import native
    lib = native.load_library()
    k, v = caches(96, 2, 3)
    k0, v0 = k.clone(), v.clone()
    st = native.stream_ptr(None)

    def call(src=SRC, dst=DST, length=32, esz=2, head_dim=96, batch=B, kc=k, vc=v):
        return lib.er_k_kv_fork(native.ptr(kc), native.ptr(vc), esz, LAYERS, batch, H, LCAP, head_dim, native.i32_array(src),
                                native.i32_array(dst), len(src), length, st)

    bad = {
        "a source outside the batch": dict(src=[6, 0, 2]),
        "a negative source": dict(src=[-1, 0, 2]),
        "a destination outside the batch": dict(dst=[1, 3, 6]),
        "a negative destination": dict(dst=[1, -2, 4]),
        "a destination that is also a source": dict(src=[0, 0, 2], dst=[1, 2, 4]),
        "a row copied onto itself": dict(src=[0], dst=[0]),
        "a destination named twice": dict(src=[0, 0, 2], dst=[1, 3, 1]),
        "len 0": dict(length=0),
        "len above l_cap": dict(length=LCAP + 1),
        "element size 3": dict(esz=3),
        "element size 8": dict(esz=8),
        "a slab that is not a multiple of 16 bytes": dict(head_dim=4, esz=2, length=1),
        "no pairs": dict(src=[], dst=[]),
    }
    for why, kw in bad.items():
        assert call(**kw) == ER_ERR_INVALID, why
        assert lib.er_last_error(), why
    torch.cuda.synchronize()
    assert torch.equal(as_bytes(k), as_bytes(k0)) and torch.equal(as_bytes(v), as_bytes(v0)), "a refused call wrote to the caches"
    assert call() == 0          # the same buffers, a good table
    torch.cuda.synchronize()
    assert torch.equal(as_bytes(k), as_bytes(expected(k0, 32)))
