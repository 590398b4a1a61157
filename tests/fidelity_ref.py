"""Numpy restatement of csrc/k_fidelity.h, operation by operation: the oracle of tests/test_fidelity_cpu.py and
tests/test_gpu_fidelity.py (nothing in the reference computes these quantities).

  nn_dist2:        fp32 (dx*dx + dy*dy) + dz*dz, every product and sum rounded on its own; the minimum over the packed key
                   (float bits << 32) | j, i.e. the smallest distance and on ties the lowest j.
  surface_sample:  face weights llrint(area * 2^32) as Python integers from double arithmetic on the fp32 coordinates, their
                   inclusive prefix sum, Philox4x32-10 words from kernels.philox4x32_10, mulhi64 on Python integers, the point in fp32.
  metrics:         distances sqrt((double)d2), means with math.fsum (exactly rounded), counts and maxima exact.
"""
import math

import numpy as np

from edgerunner_amd.kernels import FIDELITY_METRICS, philox4x32_10

SURF_TAG = 0x53555246
F32 = np.float32


def nn_dist2(a, b, chunk=512):
    """a [Na,3], b [Nb,3] fp32 -> (d2 [Na] fp32, idx [Na] int32)."""
    a = np.ascontiguousarray(a, F32)
    b = np.ascontiguousarray(b, F32)
    d2 = np.empty(a.shape[0], F32)
    idx = np.empty(a.shape[0], np.int32)
    bx, by, bz = b[None, :, 0], b[None, :, 1], b[None, :, 2]
    for lo in range(0, a.shape[0], chunk):
        q = a[lo:lo + chunk]
        dx, dy, dz = q[:, 0:1] - bx, q[:, 1:2] - by, q[:, 2:3] - bz
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == F32
        j = np.argmin(d, axis=1)                 # first occurrence of the minimum = the lowest j = the minimum of the packed key
        idx[lo:lo + chunk] = j
        d2[lo:lo + chunk] = d[np.arange(d.shape[0]), j]
    return d2, idx


def face_weights(v, f):
    """Exact integer weights of the faces: llrint(area * 2^32), area in double from the fp32 coordinates."""
    p = np.asarray(v, F32).astype(np.float64)[np.asarray(f, np.int64)]
    a, b = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    area = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
    return [int(x) for x in np.rint(area * 4294967296.0)]


def surface_sample(v, f, n, seed=0, stream=0):
    """One mesh: v [V,3] fp32, f [F,3] -> (points [n,3] fp32, faces [n] int32)."""
    v = np.asarray(v, F32)
    f = np.asarray(f, np.int64)
    cum, run = [], 0
    for w in face_weights(v, f):
        run += w
        cum.append(run)
    total = run
    assert 0 < total < 2 ** 63
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    face = np.empty(n, np.int32)
    u = np.empty(n, F32)
    w = np.empty(n, F32)
    for i in range(n):
        r = philox4x32_10((i, stream, SURF_TAG, 0), key)
        t = ((((r[0] << 32) | r[1]) * total) >> 64)
        lo, hi = 0, len(cum) - 1
        while lo < hi:                           # the smallest face with cum > t
            mid = (lo + hi) >> 1
            if cum[mid] > t:
                hi = mid
            else:
                lo = mid + 1
        face[i] = lo
        u[i] = F32(r[2] >> 8) * F32(2.0 ** -24)
        w[i] = F32(r[3] >> 8) * F32(2.0 ** -24)
    flip = (u + w) > F32(1.0)
    u = np.where(flip, F32(1.0) - u, u)[:, None]
    w = np.where(flip, F32(1.0) - w, w)[:, None]
    tri = f[face]
    p0, p1, p2 = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    pts = (p0 + u * (p1 - p0)) + w * (p2 - p0)
    assert pts.dtype == F32
    return pts, face


def metrics(d2_ab, d2_ba, tau):
    """d2_ab [Na], d2_ba [Nb] fp32 -> dict of FIDELITY_METRICS plus the exact counts (count_a, count_b within tau)."""
    tau = float(F32(tau))
    da = np.sqrt(np.asarray(d2_ab, F32).astype(np.float64))
    db = np.sqrt(np.asarray(d2_ba, F32).astype(np.float64))
    mean_ab, mean_ba = math.fsum(da) / len(da), math.fsum(db) / len(db)
    sq = math.fsum(np.asarray(d2_ab, F32).astype(np.float64)) / len(da) + math.fsum(np.asarray(d2_ba, F32).astype(np.float64)) / len(db)
    ca, cb = int((da < tau).sum()), int((db < tau).sum())
    p, r = cb / len(db), ca / len(da)
    vals = (mean_ab + mean_ba, sq, max(da.max(), db.max()), p, r, 2.0 * p * r / (p + r) if p + r > 0 else 0.0, mean_ab, mean_ba)
    out = dict(zip(FIDELITY_METRICS, (float(x) for x in vals)))
    out["count_a"], out["count_b"] = ca, cb
    return out
