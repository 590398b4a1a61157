"""Reconstruction fidelity without a GPU: the entry points exist in the cross-compiled library, the numpy restatement
(tests/fidelity_ref.py, the oracle of tests/test_gpu_fidelity.py) is sane on cases with a closed form, the workspace pairing of
fidelity.py, and the host validation of ``fidelity()``."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fidelity_ref as R  # noqa: E402

F32 = np.float32


def test_entry_points_are_exported():
    from edgerunner_amd import build, native
    build.build(verbose=False)
    lib = native.load_library()
    for name in ("er_k_nn_dist2", "er_k_surface_sample", "er_k_fidelity_metrics"):
        assert name in native.EXPORTS and hasattr(lib, name), name


def random_mesh(rng, nv, nf):
    v = rng.uniform(-1, 1, (nv, 3)).astype(F32)
    f = np.stack([rng.permutation(nv)[:3] for _ in range(nf)])
    return v, f


def test_sampled_points_lie_in_their_triangles():
    rng = np.random.default_rng(0)
    v, f = random_mesh(rng, 40, 60)
    pts, face = R.surface_sample(v, f, 500, seed=3, stream=7)
    assert face.min() >= 0 and face.max() < len(f) and len(set(face.tolist())) > 20
    tri = v.astype(np.float64)[f[face]]
    e1, e2, d = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], pts.astype(np.float64) - tri[:, 0]
    # barycentric coordinates of the point by least squares: inside the triangle and on its plane within fp32 round-off of
    # coordinates of magnitude <= 1 (a few ulp of 2^-24 through three rounded operations per component)
    for k in range(len(pts)):
        uv, *_ = np.linalg.lstsq(np.stack([e1[k], e2[k]], 1), d[k], rcond=None)
        assert np.abs(np.stack([e1[k], e2[k]], 1) @ uv - d[k]).max() < 1e-6
        scale = 1e-6 / max(np.linalg.norm(e1[k]), np.linalg.norm(e2[k]))
        assert uv[0] >= -scale and uv[1] >= -scale and uv[0] + uv[1] <= 1 + scale


def test_zero_area_face_is_never_chosen():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [0.5, 0, 0]], F32)
    f = np.array([[0, 1, 3], [0, 1, 2], [1, 4, 3], [1, 1, 2]])       # collinear, real, collinear, repeated vertex
    assert [w > 0 for w in R.face_weights(v, f)] == [False, True, False, False]
    assert R.face_weights(v, f)[1] == 2 ** 31                        # area 0.5, exactly
    _, face = R.surface_sample(v, f, 2000, seed=1)
    assert set(face.tolist()) == {1}


def test_sampling_follows_the_areas_and_the_stream():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [3, 0, 0], [0, 3, 0]], F32)
    f = np.array([[0, 1, 2], [0, 3, 4]])                              # areas 0.5 and 4.5
    pts, face = R.surface_sample(v, f, 4000, seed=5)
    assert abs((face == 1).mean() - 0.9) < 0.02                       # 4 sigma of a binomial share at n = 4000 is 0.019
    pts2, face2 = R.surface_sample(v, f, 4000, seed=5)
    assert np.array_equal(pts, pts2) and np.array_equal(face, face2)
    _, face3 = R.surface_sample(v, f, 4000, seed=5, stream=1)
    assert not np.array_equal(face, face3)


def test_identical_clouds_give_zero_metrics():
    rng = np.random.default_rng(1)
    a = rng.uniform(-1, 1, (300, 3)).astype(F32)
    d2, idx = R.nn_dist2(a, a)
    assert not d2.any() and np.array_equal(idx, np.arange(300))
    m = R.metrics(d2, d2, 0.02)
    assert m["fscore"] == 1.0 and m["precision"] == 1.0 and m["recall"] == 1.0
    assert all(m[k] == 0.0 for k in ("chamfer_l1", "chamfer_l2", "hausdorff", "mean_a2b", "mean_b2a"))


def test_translated_lattice_has_the_closed_form():
    g = np.arange(6, dtype=F32)
    a = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    b = a + np.array([0.1, 0, 0], F32)
    d2_ab, idx_ab = R.nn_dist2(a, b)
    d2_ba, idx_ba = R.nn_dist2(b, a)
    # the nearest neighbour of a lattice point is its own translate (0.1 away; the next candidate is 0.9 away), both ways
    assert np.array_equal(idx_ab, np.arange(len(a))) and np.array_equal(idx_ba, np.arange(len(a)))
    # x + 0.1 rounds in fp32: the distance of point x is |fl(x + 0.1f) - x|, within one ulp of 5 (2^-21) of 0.1
    assert np.abs(np.sqrt(d2_ab.astype(np.float64)) - 0.1).max() < 2.0 ** -21
    m = R.metrics(d2_ab, d2_ba, 0.2)
    assert abs(m["mean_a2b"] - 0.1) < 2.0 ** -21 and abs(m["mean_b2a"] - 0.1) < 2.0 ** -21
    assert abs(m["chamfer_l1"] - 0.2) < 2.0 ** -20 and abs(m["chamfer_l2"] - 0.02) < 1e-6 and abs(m["hausdorff"] - 0.1) < 2.0 ** -21
    assert m["fscore"] == 1.0
    m = R.metrics(d2_ab, d2_ba, 0.05)
    assert m["precision"] == 0.0 and m["recall"] == 0.0 and m["fscore"] == 0.0


def test_metrics_counts_are_strict_and_use_the_fp32_threshold():
    d2 = np.array([0.0, 0.25, 1.0], F32)
    m = R.metrics(d2, d2[:2], 0.5)
    assert m["count_a"] == 1 and m["count_b"] == 1                    # sqrt(0.25) = 0.5 is not < 0.5
    assert m["recall"] == 1 / 3 and m["precision"] == 0.5 and m["hausdorff"] == 1.0
    assert m["mean_a2b"] == math.fsum([0.0, 0.5, 1.0]) / 3 and m["fscore"] == 2 * 0.5 * (1 / 3) / (0.5 + 1 / 3)


def test_host_face_weights_are_the_restatement():
    from edgerunner_amd.fidelity import face_weights
    rng = np.random.default_rng(5)
    v, f = random_mesh(rng, 50, 200)
    v[:5] *= F32(1e-6)                                                # some faces around the 2^-33 area boundary
    f[:20] = rng.integers(0, 5, (20, 3))
    assert face_weights(v, f).tolist() == R.face_weights(v, f)


def test_workspace_pairing():
    from edgerunner_amd.fidelity import pair_workspace
    files = ["chair_pc.obj", "chair_0.ply", "chair_1.ply", "chair_10.ply", "chair_2.ply", "chair_0_tokens.npy", "chair_best.ply",
             "table_pc.obj", "table_0_1000f.ply", "table_0_4000f.ply", "table_1_1000f.ply", "table_0_1000f_tokens.npy",
             "lamp_pc.obj", "lamp_0_tokens.npy",                                   # generated nothing that decodes to a mesh
             "a_pc.obj", "a_0.ply", "a_1_pc.obj", "a_1_0.ply", "a_1_1_500f.ply",   # "a" is a prefix of "a_1"
             "tokens_all.npz", "fidelity.json", "stray_0.ply"]
    got = pair_workspace(files)
    assert got == {"chair": ["chair_0.ply", "chair_1.ply", "chair_2.ply", "chair_10.ply"],
                   "table": ["table_0_1000f.ply", "table_0_4000f.ply", "table_1_1000f.ply"],
                   "lamp": [], "a": ["a_0.ply"], "a_1": ["a_1_0.ply", "a_1_1_500f.ply"]}
    assert pair_workspace(["x_0.ply"]) == {}


CUBE_V = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], F32)
CUBE_F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                   [1, 5, 7], [1, 7, 3]])


@pytest.mark.parametrize("case", ["nan_vertex", "inf_cloud", "far_cloud", "far_vertex", "index_high", "index_negative", "count"])
def test_fidelity_validates_before_it_touches_the_library(case, monkeypatch):
    from edgerunner_amd import fidelity as F, native

    def no_library(*a, **k):
        raise AssertionError("the library was loaded before validation finished")
    monkeypatch.setattr(native, "load_library", no_library)
    cloud = np.zeros((1, 16, 3), F32)
    v, f = CUBE_V.copy(), CUBE_F.copy()
    meshes = [(v, f)]
    if case == "nan_vertex":
        v[3, 1] = np.nan
    elif case == "inf_cloud":
        cloud[0, 2, 0] = np.inf
    elif case == "far_cloud":
        cloud[0, 2, 0] = 9.0
    elif case == "far_vertex":
        v[0, 0] = -8.5
    elif case == "index_high":
        f[5, 2] = 8
    elif case == "index_negative":
        f[0, 0] = -1
    else:
        meshes = [(v, f), (v, f)]
    with pytest.raises(ValueError):
        F.fidelity(cloud, meshes)


def test_fidelity_leaves_empty_meshes_out_without_a_device_call(monkeypatch):
    from edgerunner_amd import fidelity as F, native
    monkeypatch.setattr(native, "load_library", lambda *a, **k: (_ for _ in ()).throw(AssertionError("library loaded")))
    cloud = np.zeros((3, 16, 3), F32)
    flat = (np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], F32), np.array([[0, 1, 2]]))
    assert F.fidelity(cloud, [None, (CUBE_V, np.zeros((0, 3), np.int64)), flat]) == [None, None, None]
