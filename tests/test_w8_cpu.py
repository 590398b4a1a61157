"""fp8 mode without a device: csrc/er_w8.h (encode, decode, row exponent) enumerated on the host under ASan + UBSan and compared with
torch's float8_e4m3fn cast, the properties of the reference quantiser (tests/w8_ref.py), and the Python surface of the mode."""
import dataclasses
import os
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import w8_ref  # noqa: E402


def f32_of_bits(bits):
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(torch.float32)


@pytest.fixture(scope="module")
def host_lines(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("w8") / "w8_check")
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, os.path.join(ROOT, "tests", "host", "w8_check.cpp")]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    elif "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]      # gcc links the runtimes dynamically by default: keep the program self-contained
    subprocess.run(cmd, check=True, cwd=ROOT)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "w8_check: ok" in out
    rows = [l.split() for l in out.splitlines() if l[:2] in ("D ", "E ", "X ")]
    return {k: [(int(r[1]), int(r[2])) for r in rows if r[0] == k] for k in "DEX"}


def test_decode_of_all_256_codes_is_torchs(host_lines):
    codes, bits = zip(*host_lines["D"])
    assert list(codes) == list(range(256))
    got = f32_of_bits(bits)
    want = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(torch.float8_e4m3fn).to(torch.float32)
    nan = torch.isnan(want)
    assert nan.nonzero().flatten().tolist() == [0x7F, 0xFF] and torch.isnan(got[nan]).all()
    assert torch.equal(got[~nan].view(torch.int32), want[~nan].view(torch.int32))      # bit for bit: -0 is 0x80


def test_encode_rounds_to_nearest_even_and_saturates_like_the_clamped_torch_cast(host_lines):
    bits, codes = zip(*host_lines["E"])
    v = f32_of_bits(bits)
    assert len(bits) > 1000 and bool((v.abs() > 448).any()) and bool((v == 0).any())
    want = v.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    got = torch.tensor(codes, dtype=torch.int32).to(torch.uint8)
    bad = (got != want).nonzero().flatten().tolist()
    assert not bad, [(float(v[i]), int(got[i]), int(want[i])) for i in bad[:8]]
    assert not bool(((got & 0x7F) == 0x7F).any()), "a NaN byte was produced"
    # the ties are in the set: a midpoint goes to the even neighbour
    lo, hi = torch.tensor(1.0), torch.tensor(1.125)
    mid = ((lo + hi) / 2).item()
    i = [float(x) for x in v].index(mid)
    assert got[i] == 0x38                                                            # 1.0 (mantissa 000), not 1.125 (001)


def test_row_exponent_rule_on_and_above_every_boundary(host_lines):
    bits, es = zip(*host_lines["X"])
    amax = f32_of_bits(bits)
    want = w8_ref.row_exponents(amax[:, None])
    assert list(es) == want.tolist()
    assert es[0] == -15 and float(amax[0]) == 0.0                                      # the zero row
    by = {float(a): e for a, e in zip(amax, es)}
    for e in range(-16, 9):
        on = 448.0 * 2.0 ** e
        above = float(torch.nextafter(torch.tensor(on, dtype=torch.float32), torch.tensor(float("inf"))))
        assert by[on] == min(max(e, -15), 7) and by[above] == min(max(e + 1, -15), 7), e


def crafted_rows(k=1536, seed=0, dtype=torch.float32):
    """fp32 rows whose crafted entries are numbers of `dtype`, the source type they will be cast to."""
    big = 6e4 if dtype == torch.float16 else 1e6                                       # beyond 448 * 2^7 either way
    g = torch.Generator().manual_seed(seed)
    gauss = torch.randn(k, generator=g) * 0.02
    rows = [gauss, torch.zeros(k), gauss.clone(), gauss.clone(), gauss * 1e-6, gauss.clone(), gauss.clone(), gauss.clone(), -gauss.abs()]
    rows[2][7] = 3e4                                                                   # e = 7
    rows[3][11] = big                                                                  # saturates
    rows[5][:] = 0.0
    rows[5][:16] = torch.tensor([1.0625, 1.1875, 1.3125, -1.0625, 0.00390625 * 1.5, 13.0, 15.0, 17.0] * 2)   # exact ties at e = -8 .. (amax 17)
    rows[5][16] = 1.75                                                                 # |max| 17 = 1.0625 * 2^4
    rows[6] = rows[6].clamp(-0.4, 0.4); rows[6][3] = 0.4375                           # 448 * 2^-10: exactly on a boundary
    rows[7] = rows[7].clamp(-0.4, 0.4); rows[7][3] = 0.4375 + 0.25 * torch.finfo(dtype).eps   # one ulp of dtype over it
    rows[8][5] = -0.0
    return torch.stack(rows)


def test_reference_quantiser_properties():
    w = crafted_rows()
    q, e, w16 = w8_ref.quantize_rows(w)
    assert e.min() >= -15 and e.max() <= 7
    assert e.tolist()[1] == -15 and e.tolist()[2] == 7 and e.tolist()[3] == 7 and e.tolist()[4] == -15
    assert e.tolist()[6] == -10 and e.tolist()[7] == -9
    assert not bool(((q & 0x7F) == 0x7F).any()), "NaN byte"
    deq = w8_ref.dequantize(q, e)
    assert torch.equal(deq.to(torch.float16).to(torch.float32), deq), "q * 2^e is not an fp16 number"
    assert torch.equal(w16.to(torch.float32), deq)
    q2, e2, _ = w8_ref.quantize_rows(deq)                                              # idempotent on its own output: the same model values
    assert torch.equal(w8_ref.dequantize(q2, e2), deq)                                 # (a row whose maximum rounded down a binade gets e - 1 and shifted codes)
    same = e2 == e
    assert int(same.sum()) >= 6 and torch.equal(q2[same], q[same])
    assert int(q[3, 11]) == 0x7E and int(q[8, 5]) == 0x80
    rel = ((deq[0] - w[0]).norm() / w[0].norm()).item()
    assert rel < 0.04, rel                                                             # half a step of a 3-bit mantissa: at most 2^-4 per element
    for dt in (torch.float16, torch.bfloat16):                                         # the rule reads the source values, whatever their dtype
        wd = crafted_rows(dtype=dt).to(dt)
        qd, ed, _ = w8_ref.quantize_rows(wd)
        qf, ef, _ = w8_ref.quantize_rows(wd.float())
        assert torch.equal(qd, qf) and torch.equal(ed, ef)
    with pytest.raises(ValueError):
        w8_ref.quantize_rows(torch.tensor([[1.0, float("nan")]]))


def test_dequantized_state_dict_touches_the_six_decoder_matrices_only():
    sd = {"mesh_decoder.model.layers.0.self_attn.q_proj.weight": torch.randn(4, 8) * 0.02,
          "mesh_decoder.model.layers.0.self_attn.q_proj.bias": torch.randn(4),
          "mesh_decoder.model.layers.0.fc2.weight": torch.randn(4, 8),
          "mesh_decoder.lm_head.weight": torch.randn(4, 8),
          "point_encoder.cross_att.att.q_proj.weight": torch.randn(4, 8)}
    out = w8_ref.dequantized_state_dict(sd)
    changed = sorted(k for k in sd if not torch.equal(out[k], sd[k]))
    assert changed == ["mesh_decoder.model.layers.0.fc2.weight", "mesh_decoder.model.layers.0.self_attn.q_proj.weight"]


def test_python_surface_names_the_mode():
    from edgerunner_amd import native
    from edgerunner_amd.models import LMM
    from edgerunner_amd.models_dit import MDiT
    from edgerunner_amd.options import config_defaults
    from edgerunner_amd.shape_opt import _DT
    opt = dataclasses.replace(config_defaults["ArAE"], num_layers=2)
    m = LMM(opt, "cuda:0", precision=None)
    assert m.fp8().precision == "fp8" and m.half().precision == "fp16" and m.fp8().float().precision == "fp32"
    with pytest.raises(ValueError):
        LMM(opt, "cuda:0", precision="fp4")
    try:                                        # the name is accepted; without a device the context itself cannot be created
        assert LMM(opt, "cuda:0", precision="fp8").precision == "fp8"
    except native.NativeError:
        pass
    with pytest.raises(ValueError):
        MDiT(dataclasses.replace(config_defaults["DiT"], num_layers=2), "cuda:0", precision="fp8")
    assert native.ER_F8E4M3 == 3 and _DT["fp8"] == 3
    for name in ("er_k_w8_quantize", "er_k_gemv_form_w8", "er_k_attn_outproj3_w8"):
        assert name in native.EXPORTS
