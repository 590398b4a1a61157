"""kv8 mode (e4m3 byte KV cache) without a device: the QUAD lane mapping of csrc/er_kv8_map.h, the cache encoder of csrc/er_w8.h and the
plan rules of csrc/er_decode_plan.h enumerated on the host (tests/host/kv8_map_check.cpp, ASan + UBSan), and the Python surface."""
import dataclasses
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv8_ref  # noqa: E402

from edgerunner_amd import native  # noqa: E402

SPLIT2, STREAM = native.ER_ATTN_SPLIT2, native.ER_ATTN_STREAM


@pytest.fixture(scope="module")
def host():
    lines = kv8_ref.host_output()
    if lines is None:
        pytest.skip("no host C++ compiler")
    return lines


def test_quad_map_loads_every_byte_once_and_folds_every_output_once(host):
    # the program checks the properties itself and names the first one that fails; "ok" is printed behind all of them
    assert host[-1] == "kv8_map_check: ok"
    assert not [l for l in host if l.startswith("kv8_map_check:") and not l.endswith("ok")]


def test_kv8_encode_is_the_clamped_torch_cast_and_keeps_nan(host):
    v, got = kv8_ref.encode_sweep()
    # the sweep the GPU test builds in torch holds the same inputs (it takes its expected bytes from torch_kv8, proved equal below)
    assert sorted(set(kv8_ref.torch_sweep().view(torch.int32).tolist())) == sorted(set(v.view(torch.int32).tolist()))
    finite = torch.isfinite(v)
    # the sweep holds what it should: all 254 finite codes as inputs, ties, fp32 subnormals, the saturating values, NaNs
    codes = set(kv8_ref.torch_kv8(v[finite]).tolist())
    assert codes == set(range(256)) - {0x7F, 0xFF}
    tiny = v.abs() < 1.17549435e-38
    assert int((tiny & (v != 0)).sum()) >= 6 and int(torch.isnan(v).sum()) == 6 and int(torch.isinf(v).sum()) == 2
    want = kv8_ref.torch_kv8(v)
    bad = (got != want).nonzero().flatten().tolist()
    assert not bad, [(float(v[i]), int(got[i]), int(want[i])) for i in bad[:8]]
    by = {float(x): int(c) for x, c in zip(v[~torch.isnan(v)], got[~torch.isnan(v)])}
    for x in (448.0, 464.0, 1e6, float("inf")):
        assert by[x] == 0x7E and by[-x] == 0xFE, x
    assert by[1.0625] == 0x38                                    # the tie between 1.0 and 1.125 goes to the even code
    nan = torch.isnan(v)
    neg = v.view(torch.int32)[nan] < 0
    assert got[nan][~neg].tolist() == [0x7F] * 3 and got[nan][neg].tolist() == [0xFF] * 3
    bits = v.view(torch.int32)
    assert set(got[bits == 0].tolist()) == {0x00} and set(got[bits == -2 ** 31].tolist()) == {0x80}      # the sign of zero is kept


def test_plan_rules(host):
    rows = {(int(r[1]), int(r[2])): [int(x) for x in r[3:]] for r in (l.split() for l in host if l.startswith("P "))}
    for B in (1, 4, 5, 15, 16, 33):
        ver, kernel, merge, kv8, stream, v3 = rows[(B, 1)]
        assert kv8 == 1 and v3 == 0 and ver == 2, B               # never version 3
        if B <= 4:
            assert (kernel, merge, stream) == (SPLIT2, 1, 0), B   # version 2: split kernel + merge launch
        else:
            assert (kernel, merge, stream) == (STREAM, 0, 1), B   # every batched shape streams
    # the fp16 rules next to them are what they were: version 3 at one row, the round-1 split kernel below 16 rows
    assert rows[(1, 0)][:3] == [3, native.ER_ATTN_BALANCED, 0] and rows[(4, 0)][:3] == [2, SPLIT2, 1]
    assert rows[(5, 0)][:3] == [2, native.ER_ATTN_SPLIT1, 1] and rows[(15, 0)][:3] == [2, native.ER_ATTN_SPLIT1, 1]
    assert rows[(16, 0)][:3] == [2, STREAM, 0] and rows[(33, 0)][:3] == [2, STREAM, 0]
    assert all(r[3] == 0 for (b, k), r in rows.items() if k == 0)
    assert rows[(8, 2)][1:3] == [STREAM, 0]                       # ER_ATTN_V_BATCHED=1 cannot select a kernel that reads no bytes
    shared = {int(r[1]): int(r[2]) for r in (l.split() for l in host if l.startswith("S "))}
    assert set(shared) == {1, 4, 5, 15, 16, 33} and not any(shared.values())      # no prefix groups on a byte cache


def test_lmm_argument_validation():
    from edgerunner_amd.models import LMM
    from edgerunner_amd.options import config_defaults
    from edgerunner_amd.shape_opt import _DT
    opt = dataclasses.replace(config_defaults["ArAE"], num_layers=2)
    with pytest.raises(ValueError, match="kv_precision"):
        LMM(opt, "cuda:0", precision="fp32", kv_precision="fp8")
    with pytest.raises(ValueError, match="kv_precision"):
        LMM(opt, "cuda:0", precision="fp16", kv_precision="fp16")
    m = LMM(opt, "cuda:0", precision=None, kv_precision="fp8")            # module style: nothing is created yet
    assert m.kv_precision == "fp8" and m.precision == "fp32"
    with pytest.raises(ValueError, match="'fp16' or 'fp8' only"):
        m.float()
    with pytest.raises(ValueError, match="'fp16' or 'fp8' only"):
        m.mesh_decoder                                                      # fp32 until .half(): the context would be exact mode's
    assert m.half().precision == "fp16" and m.kv_precision == "fp8"
    assert m.fp8().precision == "fp8" and m.kv_precision == "fp8"
    with pytest.raises(ValueError, match="'fp16' or 'fp8' only"):
        m.float()
    assert m.precision == "fp8"                                            # a refused cast changes nothing
    plain = LMM(opt, "cuda:0", precision=None)
    assert plain.kv_precision is None and plain.half().kv_precision is None and plain.float().precision == "fp32"
    assert _DT["fp8"] == native.ER_F8E4M3 and "er_k_kv8_encode" in native.EXPORTS
