"""fp4 mode without a device: csrc/er_w4.h (e2m1 encode / decode, block exponent, canonical block) and csrc/er_w4_map.h (the streamed
copy) enumerated on the host under ASan + UBSan and compared with the torch restatement tests/w4_ref.py, the launch rule of
csrc/er_w4_rule.h, and the Python surface of the mode."""
import dataclasses
import importlib
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import w4_ref  # noqa: E402


def f32_of_bits(bits):
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(torch.float32)


@pytest.fixture(scope="module")
def host_lines():
    lines = w4_ref.host_lines()
    if lines is None:
        pytest.skip("no host C++ compiler")
    return lines


# ------------------------------------------------------------------ the format
def test_all_16_codes_decode_to_the_table(host_lines):
    codes, bits = zip(*host_lines["D"])
    assert list(codes) == list(range(16))
    want = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0])
    assert torch.equal(f32_of_bits(bits).view(torch.int32), want.view(torch.int32))      # bit for bit: code 8 is -0
    assert torch.equal(w4_ref.decode_table().view(torch.int32), want.view(torch.int32))


def test_encode_is_nearest_ties_to_even_and_saturates(host_lines):
    bits, codes = zip(*host_lines["E"])
    v = f32_of_bits(bits)
    got = torch.tensor(codes, dtype=torch.uint8)
    assert len(bits) > 100 and bool((v.abs() > 6).any()) and bool((v == 0).any()) and bool(((v != 0) & (v.abs() < 1.2e-38)).any())
    want = w4_ref.encode(v)
    bad = (got != want).nonzero().flatten().tolist()
    assert not bad, [(float(v[i]), int(got[i]), int(want[i])) for i in bad[:8]]
    by = {float(x): int(c) for x, c in zip(v, got) if x > 0 or (x == 0 and not torch.signbit(x))}
    # every tie goes to the even code, written out: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4
    assert [by[t] for t in (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)] == [0, 2, 2, 4, 4, 6, 6]
    up = lambda t: float(torch.nextafter(torch.tensor(t), torch.tensor(9.0)))
    down = lambda t: float(torch.nextafter(torch.tensor(t), torch.tensor(0.0)))
    assert [by[up(t)] for t in (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)] == [1, 2, 3, 4, 5, 6, 7]
    assert [by[down(t)] for t in (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)] == [0, 1, 2, 3, 4, 5, 6]
    sub = float(torch.tensor(1e-41, dtype=torch.float32))
    assert by[6.0] == by[up(6.0)] == by[8.0] == by[1e6] == 7 and by[0.0] == 0 and by[sub] == 0      # saturation, an fp32 subnormal
    neg = {float(x): int(c) for x, c in zip(v, got) if torch.signbit(x)}
    assert neg[-0.0] == 8 and neg[-sub] == 8 and neg[-1e6] == 15 and neg[-0.25] == 8 and neg[-0.75] == 10      # the sign of zero is kept
    # round trip on all codes (the host program checked pack / unpack of every pair too)
    assert w4_ref.encode(w4_ref.decode_table()).tolist() == list(range(16))


def test_block_exponent_is_the_smallest_admissible_one_in_every_binade(host_lines):
    bits, es = zip(*host_lines["X"])
    amax = f32_of_bits(bits)
    assert es[0] == -15 and float(amax[0]) == 0.0                                      # the zero block
    assert len(es) == 1 + 43 * 5 + 3
    assert list(es) == w4_ref.block_exponents(amax).tolist()
    a64 = amax.to(torch.float64)
    for a, e in zip(a64[1:].tolist(), es[1:]):
        assert -15 <= e <= 7
        if e > -15:
            assert a * 2.0 ** -(e - 1) > 6.0, (a, e)                                   # e - 1 would clip: e is the smallest
        if e < 7:
            assert a * 2.0 ** -e <= 6.0, (a, e)                                        # admissible unless the clamp holds it down
    by = {float(a): e for a, e in zip(amax, es)}
    assert by[1.0] == -2 and by[1.5] == -2 and by[float(torch.nextafter(torch.tensor(1.5), torch.tensor(2.0)))] == -1
    assert by[2.0 ** -30] == -15 and by[2.0 ** 12] == 7 and by[0.125] == -5


def test_every_value_in_the_clamp_range_is_an_fp16_number(host_lines):
    table = w4_ref.decode_table()
    for e in range(-15, 8):
        v = torch.ldexp(table, torch.tensor(e))
        assert torch.equal(v.to(torch.float16).to(torch.float32), v), e
    assert float(torch.ldexp(table, torch.tensor(7)).abs().max()) == 768.0
    if host_lines["H"]:                                                                # the host compiler has _Float16: the same, by the header
        assert len(host_lines["H"]) == 23 * 16 and all(ok == 1 for _, _, ok in host_lines["H"])


# ------------------------------------------------------------------ the quantiser: host program against the torch restatement
def test_reference_and_host_quantiser_agree_byte_for_byte(host_lines):
    w = w4_ref.crafted_matrix()
    assert w.shape == (8, 1536)
    nib, scales, e, w16 = w4_ref.quantize(w)
    assert torch.equal(w4_ref.host_quantize(w), w4_ref.canonical_block(nib, scales))
    assert e.min() >= -15 and e.max() <= 7
    assert int(e[1, 2]) == -15 and bool((nib[1, 32:48] == 0).all())                    # the zero block
    assert int(e[2, 1]) == 0 and int(nib[2, 20]) & 15 == 6                             # the outlier 5.0 -> 4 (a tie) = code 6 in the low nibble
    assert int(((nib[2, 16:32] & 0x77) != 0).sum()) == 1                               # ... and every other element of its block rounds to +-0
    assert int(e[3, 0]) == -7 and int(e[4, 0]) == -6                                   # amax on 6 * 2^-7 exactly, and one ulp above it
    assert int(nib[3, 2]) >> 4 == 7                                                    # ... which is code 7 (element 5: the high nibble of byte 2)
    assert nib[5, 0:4].tolist() == [0x20, 0x42, 0x64, 0xF6] and nib[5, 4:8].tolist() == [0xA8, 0xCA, 0xEC, 0x7E]      # the ties at e = 0, both signs
    assert int(nib[5, 8]) == 0x80                                                      # -0 keeps its sign (element 17)
    assert int(e[6, 3]) == -15 and int(e[7, 0]) == 7 and int(nib[7, 0]) & 15 == 7      # far below the clamp; beyond it: saturated
    deq = w4_ref.dequantize(nib, e)
    assert torch.equal(w16.float(), deq) and torch.equal(deq.to(torch.float16).float(), deq)
    rel = ((deq[0] - w[0]).norm() / w[0].norm()).item()
    assert rel < 0.2, rel                                                              # half a step of a 1-bit mantissa: at most 1/6 of the block maximum per element
    for dt in (torch.float16, torch.bfloat16):                                         # the rule reads the source values, whatever their dtype
        wd = w.to(dt)
        a, b = w4_ref.quantize(wd), w4_ref.quantize(wd.float())
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError):
        w4_ref.quantize(torch.tensor([[1.0] * 31 + [float("nan")]]))


def test_dequantized_state_dict_touches_the_six_decoder_matrices_only():
    sd = {"mesh_decoder.model.layers.0.self_attn.q_proj.weight": torch.randn(4, 32) * 0.02,
          "mesh_decoder.model.layers.0.self_attn.q_proj.bias": torch.randn(4),
          "mesh_decoder.model.layers.0.fc2.weight": torch.randn(4, 64),
          "mesh_decoder.lm_head.weight": torch.randn(4, 32),
          "point_encoder.cross_att.att.q_proj.weight": torch.randn(4, 32)}
    out = w4_ref.dequantized_state_dict(sd)
    changed = sorted(k for k in sd if not torch.equal(out[k], sd[k]))
    assert changed == ["mesh_decoder.model.layers.0.fc2.weight", "mesh_decoder.model.layers.0.self_attn.q_proj.weight"]


# ------------------------------------------------------------------ the streamed copy and the launch rule
@pytest.fixture(scope="module")
def map_lines():
    exe = w4_ref.host_exe("w4_map_check")
    if exe is None:
        pytest.skip("no host C++ compiler")
    res = subprocess.run([exe, "8", "1536", "8", "6144"], capture_output=True, text=True)
    assert res.returncode == 0 and "w4_map_check: ok" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
    return [l.split() for l in res.stdout.splitlines()]


def test_map_holds_every_element_once_with_its_scale_in_aligned_loads(map_lines):
    m = [[int(t) for t in l[1:]] for l in map_lines if l[0] == "M"]
    assert m == [[8, 1536, 6, 6 * 1088], [8, 6144, 24, 24 * 1088]]                     # 2 quads x 1 (4) slices x 3 loads; 1088 bytes per unit
    assert all(n * k // 2 + n * k // 32 == total for n, k, _, total in m)              # no padding: the copy has the canonical block's size
    exe = w4_ref.host_exe("w4_map_check")
    for bad in (["6", "1536"], ["8", "1024"]):                                         # N % 4 and K % 1536 are refused
        assert subprocess.run([exe] + bad, capture_output=True, text=True).returncode != 0


def test_launch_rule_over_projection_batch_and_knob(map_lines):
    QKV, OUT, FC1, FC2, HEAD = range(5)
    rule = {(int(p), int(b), int(k)): int(v) for _, p, b, k, v in (l for l in map_lines if l[0] == "R")}
    assert len(rule) == 5 * 6 * 3
    for proj in range(5):
        for B in range(6):
            assert rule[proj, B, 0] == 0                                               # ER_W4_ROWS=0: the fp16 copies everywhere
            assert rule[proj, B, 1] == int(proj in (QKV, FC1, FC2) and 1 <= B <= 4)    # =1: every row form that has a nibble kernel
            assert rule[proj, B, -1] <= rule[proj, B, 1]                               # the measured rule picks among those
    # the measured rule (profiles/w4_bench.json)
    measured = {(proj, B) for proj in range(5) for B in range(6) if rule[proj, B, -1]}
    assert measured == set(MEASURED_RULE)


# (projection, B) pairs whose nibble form measured faster than the fp16 form beyond the fp16 spread: qkv (0) at one row, fc1 (2) and
# fc2 (3) at every row count
MEASURED_RULE = ((0, 1),) + tuple((proj, B) for proj in (2, 3) for B in (1, 2, 3, 4))


# ------------------------------------------------------------------ the Python surface
def test_python_surface_names_the_mode():
    from edgerunner_amd import native
    from edgerunner_amd.models import LMM
    from edgerunner_amd.models_dit import MDiT
    from edgerunner_amd.options import config_defaults
    from edgerunner_amd.shape_opt import _DT, NativeShapeOPT
    opt = dataclasses.replace(config_defaults["ArAE"], num_layers=2)
    m = LMM(opt, "cuda:0", precision=None)
    assert m.fp4().precision == "mxfp4" and m.half().precision == "fp16" and m.fp4().fp8().precision == "fp8" and m.fp4().float().precision == "fp32"
    try:                                        # the name is accepted; without a device the context itself cannot be created
        assert LMM(opt, "cuda:0", precision="mxfp4").precision == "mxfp4"
    except native.NativeError:
        pass
    with pytest.raises(ValueError, match="mxfp4"):                                      # the bare name stays refused (tests/test_w8_cpu.py pins it) and names the spelling
        LMM(opt, "cuda:0", precision="fp4")
    with pytest.raises(ValueError):
        MDiT(dataclasses.replace(config_defaults["DiT"], num_layers=2), "cuda:0", precision="mxfp4")
    assert native.ER_F4E2M1 == 4 and _DT["fp4"] == 4 and hasattr(NativeShapeOPT, "w4_streams")
    for name in ("er_k_w4_quantize", "er_k_gemv_form_w4", "er_k_w4_cvt_probe", "er_ctx_w4_streams"):
        assert name in native.EXPORTS


def test_lmm_kv_precision_rules_under_fp4():
    from edgerunner_amd.models import LMM
    from edgerunner_amd.options import config_defaults
    opt = dataclasses.replace(config_defaults["ArAE"], num_layers=2)
    m = LMM(opt, "cuda:0", precision=None, kv_precision="fp8")                         # module style: nothing is created yet
    assert m.fp4().precision == "mxfp4" and m.kv_precision == "fp8"                      # the byte cache is allowed beside fp4 weights
    with pytest.raises(ValueError, match="kv_precision"):
        m.float()
    assert m.precision == "mxfp4"                                                      # a refused cast changes nothing
    with pytest.raises(ValueError, match="kv_precision"):
        LMM(opt, "cuda:0", precision="mxfp4", kv_precision="fp16")
    with pytest.raises(ValueError, match="kv_precision"):
        LMM(opt, "cuda:0", precision="mxfp4", kv_precision="fp4")                        # there is no 4-bit cache
    plain = LMM(opt, "cuda:0", precision=None)
    assert plain.fp4().kv_precision is None


@pytest.mark.parametrize("tool", ["infer", "score"])
def test_tools_take_the_mode_from_the_environment(tool, monkeypatch, tmp_path):
    """EDGERUNNER_PRECISION=fp4 (with and without EDGERUNNER_KV_PRECISION=fp8) reaches LMM.fp4() in infer.py and score.py; the run is cut
    where the weights would go to the device."""
    sys.path.insert(0, ROOT)
    mod = importlib.import_module(tool)
    from edgerunner_amd import weights as W
    from edgerunner_amd.models import LMM

    class Reached(Exception):
        pass

    seen = []

    def release(self):
        seen.append((self.precision, self.kv_precision))
        raise Reached

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(W, "make_state_dict", lambda *a, **k: {})
    monkeypatch.setattr(LMM, "load_state_dict", lambda self, sd, strict=False: ([], []))
    monkeypatch.setattr(LMM, "to", lambda self, *a, **k: self)
    monkeypatch.setattr(LMM, "release_checkpoint", release)
    for kv, name in ((None, "fp4"), ("fp8", "mxfp4")):                                   # the tools take either spelling
        monkeypatch.setenv("EDGERUNNER_PRECISION", name)
        if kv:
            monkeypatch.setenv("EDGERUNNER_KV_PRECISION", kv)
        else:
            monkeypatch.delenv("EDGERUNNER_KV_PRECISION", raising=False)
        with pytest.raises(Reached):
            mod.main(["ArAE", "--num_layers", "2", "--test_path", str(tmp_path), "--workspace", str(tmp_path)])
    assert seen == [("mxfp4", None), ("mxfp4", "fp8")]
