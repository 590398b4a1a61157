"""Reconstruction fidelity on the GPU (csrc/k_fidelity.h) against its numpy restatement (tests/fidelity_ref.py): nearest-neighbour
distances and indices and surface samples bit for bit, the metrics within the bound of an N-term double sum (counts and maxima
exactly), then ``fidelity()`` and the ``fidelity.py`` script end to end on a cube."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fidelity_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32 = np.float32


def dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


def check_nn(a, b):
    """a [B,Na,3], b [B,Nb,3] numpy fp32: d2 and idx of the kernel == the restatement, bit for bit."""
    from edgerunner_amd import kernels
    d2, idx = kernels.nn_dist2(dev(a), dev(b))
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    for k in range(a.shape[0]):
        want_d2, want_idx = R.nn_dist2(a[k], b[k])
        assert np.array_equal(idx[k], want_idx), (k, np.flatnonzero(idx[k] != want_idx)[:8])
        assert np.array_equal(d2[k].view(np.uint32), want_d2.view(np.uint32)), k


# (1, 1, 1) .. (1, 1000, 1025): ragged sizes (below / across the 64-lane wave, the 256-key tile and the 1024-query block);
# (3, 257, 4097): batch strides with different content per entry; (2, 8192, 8192): the key-range split and its merge at the size
# fidelity.py uses
@pytest.mark.parametrize("B,Na,Nb", [(1, 1, 1), (1, 63, 65), (1, 1000, 1025), (3, 257, 4097), (2, 8192, 8192)])
def test_nn_dist2_matches_restatement(B, Na, Nb):
    rng = np.random.default_rng(1000 * B + Na + Nb)
    check_nn(rng.uniform(-1, 1, (B, Na, 3)).astype(F32), rng.uniform(-1, 1, (B, Nb, 3)).astype(F32))


@pytest.mark.parametrize("q", [1, 2, 4])
def test_nn_dist2_every_queries_per_lane_form(q, monkeypatch):
    """The launch picks 4, 2 or 1 queries per lane from the shape (the cases above run 1 and 2); ER_NN_Q forces each form on a
    shape with a ragged last query block and several key tiles."""
    monkeypatch.setenv("ER_NN_Q", str(q))
    rng = np.random.default_rng(7)
    check_nn(rng.uniform(-1, 1, (2, 1500, 3)).astype(F32), rng.uniform(-1, 1, (2, 700, 3)).astype(F32))


def test_nn_dist2_exact_ties_take_the_lowest_index():
    g = np.arange(16, dtype=F32)
    a = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(1, -1, 3)
    rng = np.random.default_rng(2)
    # half a cell along x: every interior point has two nearest keys at exactly 0.25 (the keys are shuffled, so the lower index
    # is on either side); half a cell along all three axes: eight at exactly 0.75
    for off in ([0.5, 0, 0], [0.5, 0.5, 0.5]):
        b = (a[0] + np.array(off, F32))[rng.permutation(a.shape[1])][None]
        want_d2, _ = R.nn_dist2(a[0], b[0])
        assert (want_d2 == F32(sum(x * x for x in off))).all()
        check_nn(a, b)


def test_nn_dist2_duplicates_and_same_buffer():
    from edgerunner_amd import kernels
    rng = np.random.default_rng(3)
    c = rng.uniform(-1, 1, (700, 3)).astype(F32)
    perm = rng.permutation(1400)
    b = np.concatenate([c, c])[perm][None]                    # every point occurs twice, at unrelated positions
    check_nn(rng.uniform(-1, 1, (1, 900, 3)).astype(F32), b)
    t = dev(b)
    d2, idx = kernels.nn_dist2(t, t)                            # a and b the same buffer: zeros, the first occurrence
    first = np.full(700, 1 << 30)
    np.minimum.at(first, perm % 700, np.arange(1400))           # lowest position of each original point
    assert not d2.cpu().numpy().any()
    assert np.array_equal(idx.cpu().numpy()[0], first[perm % 700])


def test_nn_dist2_rejects_bad_sizes():
    from edgerunner_amd import kernels, native
    a = torch.zeros((1, 4, 3), device=DEV)
    with pytest.raises(native.NativeError, match="er_k_nn_dist2"):
        kernels.nn_dist2(a, torch.zeros((1, 0, 3), device=DEV))


# ---------------------------------------------------------------------------------------------------------------- sampling
def sphere(n_lat=32, n_lon=64, radius=0.9):
    """A latitude / longitude sphere: 2 * n_lat * n_lon = 4096 faces, of which the 2 * n_lon at the poles have zero area."""
    th = np.linspace(0, np.pi, n_lat + 1)
    ph = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    v = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones_like(ph))], -1)
    v = (radius * v).reshape(-1, 3).astype(F32)
    f = []
    for i in range(n_lat):
        for j in range(n_lon):
            p, q = i * n_lon + j, i * n_lon + (j + 1) % n_lon
            f += [[p, p + n_lon, q + n_lon], [p, q + n_lon, q]]
    return v, np.asarray(f)


CUBE_V = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], F32)
CUBE_F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                   [1, 5, 7], [1, 7, 3]])
TRI = (np.array([[0.25, -0.5, 0.125], [0.75, 0.3, -0.9], [-0.6, 0.4, 0.7]], F32), np.array([[0, 1, 2]]))
N_S = 2048


def sample(meshes, n, seed, streams=None):
    from edgerunner_amd import kernels
    voff = np.concatenate([[0], np.cumsum([len(v) for v, _ in meshes])]).tolist()
    foff = np.concatenate([[0], np.cumsum([len(f) for _, f in meshes])]).tolist()
    pts, face = kernels.surface_sample(dev(np.concatenate([v for v, _ in meshes])),
                                       dev(np.concatenate([f for _, f in meshes]), torch.int32), voff, foff, n, seed=seed,
                                       stream_ids=streams)
    return pts.cpu().numpy(), face.cpu().numpy()


@pytest.fixture(scope="module")
def sphere_ref():
    v, f = sphere()
    return v, f, R.surface_sample(v, f, N_S, seed=11, stream=5)


def check_samples(got_pts, got_face, want):
    assert np.array_equal(got_face, want[1]), np.flatnonzero(got_face != want[1])[:8]
    assert np.array_equal(got_pts.view(np.uint32), want[0].view(np.uint32))


def test_sample_single_triangle():
    pts, face = sample([TRI], 1000, seed=0x1234567890)        # a seed with a high word
    check_samples(pts[0], face[0], R.surface_sample(*TRI, 1000, seed=0x1234567890, stream=0))


def test_sample_skips_the_degenerate_triangle():
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0]], F32)
    f = np.array([[0, 1, 2], [0, 1, 3]])
    pts, face = sample([(v, f)], 1000, seed=7)
    assert (face == 1).all()
    check_samples(pts[0], face[0], R.surface_sample(v, f, 1000, seed=7))


def test_sample_sphere(sphere_ref):
    v, f, want = sphere_ref
    pts, face = sample([(v, f)], N_S, seed=11, streams=[5])
    check_samples(pts[0], face[0], want)
    assert len(set(face[0].tolist())) > 1000                   # spread over the surface


def test_sample_ragged_batch_and_stream_independence(sphere_ref):
    v, f, want = sphere_ref
    pts, face = sample([TRI, (CUBE_V, CUBE_F), (v, f)], N_S, seed=11, streams=[9, 2, 5])
    check_samples(pts[0], face[0], R.surface_sample(*TRI, N_S, seed=11, stream=9))
    check_samples(pts[1], face[1], R.surface_sample(CUBE_V, CUBE_F, N_S, seed=11, stream=2))
    check_samples(pts[2], face[2], want)                       # the sphere alone (test_sample_sphere) and third of a batch
    pts2, face2 = sample([(v, f), TRI], N_S, seed=11, streams=[5, 9])
    assert np.array_equal(pts2[0], pts[2]) and np.array_equal(face2[0], face[2]) and np.array_equal(pts2[1], pts[0])
    pts3, _ = sample([TRI, TRI], 64, seed=11)                    # default stream ids: the position in the call
    assert np.array_equal(pts3[0], R.surface_sample(*TRI, 64, seed=11, stream=0)[0])
    assert np.array_equal(pts3[1], R.surface_sample(*TRI, 64, seed=11, stream=1)[0])


def test_sample_names_the_bad_mesh():
    from edgerunner_amd import native
    flat = (np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], F32), np.array([[0, 1, 2]]))
    outside = (CUBE_V, np.where(np.arange(36).reshape(12, 3) == 17, 8, CUBE_F))     # one index == the vertex count
    with pytest.raises(native.NativeError, match="mesh 1 has zero area"):
        sample([TRI, flat], 16, seed=0)
    with pytest.raises(native.NativeError, match="mesh 2 has a face index outside"):
        sample([TRI, TRI, outside], 16, seed=0)
    with pytest.raises(native.NativeError, match="mesh 1 has no faces"):
        sample([TRI, (CUBE_V, np.zeros((0, 3), np.int64)), TRI], 16, seed=0)


# ----------------------------------------------------------------------------------------------------------------- metrics
def test_metrics_match_restatement_and_repeat_bitwise():
    from edgerunner_amd import kernels
    rng = np.random.default_rng(4)
    B, Na, Nb, tau = 3, 8192, 5001, 0.5
    d2_ab = (rng.uniform(0, 1, (B, Na)) ** 2).astype(F32)
    d2_ba = (rng.uniform(0, 1.2, (B, Nb)) ** 2).astype(F32)
    d2_ab[:, ::7] = 0.25                                         # distance == tau exactly: not within
    d2_ba[1, 17] = 4.0                                           # the Hausdorff distance of entry 1, from the b side
    got = kernels.fidelity_metrics(dev(d2_ab), dev(d2_ba), tau)
    again = kernels.fidelity_metrics(dev(d2_ab), dev(d2_ba), tau)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))
    got = got.cpu().numpy()
    u = 2.0 ** -52
    for k in range(B):
        want = R.metrics(d2_ab[k], d2_ba[k], tau)
        g = dict(zip(kernels.FIDELITY_METRICS, got[k]))
        for name in kernels.FIDELITY_METRICS:
            print(k, name, g[name], want[name])
        # an N-term double sum against the exactly rounded one: N * 2^-52 relative.  The sum of two positive means that each
        # hold their bound holds the larger of the two, plus the rounding of the addition
        assert abs(g["mean_a2b"] - want["mean_a2b"]) <= Na * u * want["mean_a2b"]
        assert abs(g["mean_b2a"] - want["mean_b2a"]) <= Nb * u * want["mean_b2a"]
        assert abs(g["chamfer_l1"] - want["chamfer_l1"]) <= (max(Na, Nb) + 1) * u * want["chamfer_l1"]
        assert abs(g["chamfer_l2"] - want["chamfer_l2"]) <= (max(Na, Nb) + 1) * u * want["chamfer_l2"]
        assert g["hausdorff"] == want["hausdorff"]
        # count / N is one rounded division on both sides: equal quotients are equal counts
        assert g["recall"] == want["recall"] and g["precision"] == want["precision"] and g["fscore"] == want["fscore"]
    assert got[1][2] == 2.0


def test_metrics_fscore_is_zero_when_nothing_is_within():
    from edgerunner_amd import kernels
    got = kernels.fidelity_metrics(torch.ones((1, 5), device=DEV), torch.ones((1, 3), device=DEV), 0.5).cpu().numpy()[0]
    assert got.tolist() == [2.0, 2.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0]


# -------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def cube_cloud():
    # 8192 samples of the unit cube's surface (area 6) from another seed than fidelity() uses: 1365 points per unit area, so a
    # disc of radius 0.1 around a surface point holds 43 of them on average and is empty with probability e^-43
    pts, _ = sample([(CUBE_V, CUBE_F)], 8192, seed=99)
    return pts[0]


def test_fidelity_ranks_the_cube_above_its_shifted_copy(cube_cloud):
    from edgerunner_amd.fidelity import fidelity
    from edgerunner_amd.meto import Mesh
    shifted = cube_cloud + np.array([0.1, 0, 0], F32)
    res = fidelity(np.stack([cube_cloud, shifted, cube_cloud]), [Mesh(CUBE_V, CUBE_F), (CUBE_V, CUBE_F), None], tau=0.1, seed=0)
    same, off, none = res
    print(same, off)
    assert none is None
    assert same["chamfer_l1"] < off["chamfer_l1"]
    assert same["fscore"] == 1.0 and same["precision"] == 1.0 and same["recall"] == 1.0
    assert same["hausdorff"] < 0.1
    assert 0 < off["mean_a2b"] <= 0.1                            # every shifted point is 0.1 from a surface point
    # the result of a mesh does not depend on what shares its call, given its stream
    alone = fidelity(shifted[None], [(CUBE_V, CUBE_F)], tau=0.1, seed=0, streams=[1])
    assert alone[0] == off


def test_fidelity_script_names_the_cube_as_best(cube_cloud, tmp_path):
    from edgerunner_amd import meshio
    ws = tmp_path / "ws"
    ws.mkdir()
    meshio.save_points_obj(str(ws / "cube_pc.obj"), cube_cloud)
    meshio.save_ply(str(ws / "cube_0.ply"), CUBE_V + np.array([0.1, 0, 0], F32), CUBE_F)
    meshio.save_ply(str(ws / "cube_1.ply"), CUBE_V, CUBE_F)
    meshio.save_ply(str(ws / "cube_2.ply"), CUBE_V * F32(9), CUBE_F)        # outside the sampler's range: recorded, not fatal
    p = subprocess.run([sys.executable, os.path.join(ROOT, "fidelity.py"), "--workspace", str(ws), "--samples", "4096", "--tau", "0.1",
                        "--copy_best"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:]
    out = json.load(open(ws / "fidelity.json"))
    assert out["inputs"]["cube"]["best"] == "cube_1.ply" and out["inputs"]["cube"]["candidates"] == ["cube_0.ply", "cube_1.ply",
                                                                                                      "cube_2.ply"]
    assert set(out["files"]) == {"cube_0.ply", "cube_1.ply", "cube_2.ply"} and out["files"]["cube_2.ply"] is None
    assert list(out["errors"]) == ["cube_2.ply"] and "outside" in out["errors"]["cube_2.ply"]
    assert out["files"]["cube_1.ply"]["chamfer_l1"] < out["files"]["cube_0.ply"]["chamfer_l1"]
    assert out["files"]["cube_1.ply"]["fscore"] == 1.0
    assert (ws / "cube_best.ply").read_bytes() == (ws / "cube_1.ply").read_bytes()
