"""torch-CPU restatement of the fp4 mode's block quantiser (edgerunner_amd/csrc/er_w4.h: OCP MXFP4), by table lookup - no torch fp4 dtype:

    block   = 32 consecutive elements of a row
    e[blk]  = the smallest integer with amax(block) * 2^-e <= 6, clamped to [-15, 7]; a zero block gets -15; stored as the byte e + 127
    q       = the nearest of {0, 0.5, 1, 1.5, 2, 3, 4, 6} to clamp(|w| * 2^-e, 6), a tie going to the even code, with the sign of w
    value   = q * 2^e, an fp16 number
    packing = element 2 i in the low nibble of byte i, element 2 i + 1 in the high nibble

The exponent comes from ``torch.frexp`` (exponent and mantissa bits), never from a logarithm.  Also here: the two host programs
tests/host/w4_check.cpp and tests/host/w4_map_check.cpp, built with ASan + UBSan once per session (CPU suite only)."""
import functools
import os
import shutil
import subprocess
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_MIN, E_MAX, W4_MAX, BLOCK = -15, 7, 6.0, 32
MAGNITUDES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
# the six matrices of a decoder layer that fp4 mode quantises (q / k / v each on its own rows)
W4_SUFFIXES = tuple(f"self_attn.{p}.weight" for p in ("q_proj", "k_proj", "v_proj", "out_proj")) + ("fc1.weight", "fc2.weight")


def decode_table() -> torch.Tensor:
    """fp32 [16]: the value of every code (code 8 is -0)."""
    m = torch.tensor(MAGNITUDES, dtype=torch.float32)
    return torch.cat((m, -m))


def encode(v: torch.Tensor) -> torch.Tensor:
    """uint8 codes of fp32 / fp64 values: saturate at 6, nearest magnitude, ties to the even code, the sign bit of v (of -0 too)."""
    v = v.to(torch.float64)
    a = v.abs().clamp(max=W4_MAX)
    d = (a[..., None] - torch.tensor(MAGNITUDES, dtype=torch.float64)).abs()          # exact: fp32 and the table are fp64 numbers
    best = d.amin(dim=-1, keepdim=True)
    odd = torch.arange(8) % 2
    rank = torch.where(d == best, odd, torch.full_like(odd, 2))                        # among the nearest: an even code first
    code = rank.argmin(dim=-1)
    return (code + 8 * torch.signbit(v).to(torch.int64)).to(torch.uint8)


def block_exponents(amax: torch.Tensor) -> torch.Tensor:
    """int32: e of blocks with these maxima (finite, >= 0)."""
    amax = amax.to(torch.float64)
    m, x = torch.frexp(amax)                                                # amax = m * 2^x, m in [0.5, 1);  6 = 0.75 * 2^3
    e = x.to(torch.int64) - 3 + (m > 0.75).to(torch.int64)
    e = torch.where(amax == 0, torch.full_like(e, E_MIN), e)
    return e.clamp(E_MIN, E_MAX).to(torch.int32)


def quantize(w: torch.Tensor):
    """(nibbles uint8 [n, k / 2], scales uint8 [n, k / 32], e int32 [n, k / 32], w16 fp16 [n, k] = q * 2^e) of w [n, k]; raises on a
    non-finite value."""
    w = w.detach().to("cpu")
    n, k = w.shape
    assert k % BLOCK == 0
    if not bool(torch.isfinite(w.float()).all()):
        raise ValueError("non-finite source value")
    w64 = w.to(torch.float64).view(n, k // BLOCK, BLOCK)
    e = block_exponents(w64.abs().amax(dim=2))
    codes = encode(torch.ldexp(w64, (-e).to(torch.int64)[..., None])).view(n, k)       # exact: a power of two in fp64
    nib = codes[:, 0::2] | (codes[:, 1::2] << 4)
    return nib.contiguous(), (e + 127).to(torch.uint8), e, dequantize(nib, e).to(torch.float16)


def canonical_block(nib: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """uint8 [n * k / 2 + n * k / 32]: the nibble bytes row-major, then the scale bytes row-major."""
    return torch.cat((nib.reshape(-1), scales.reshape(-1)))


def dequantize(nib: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """fp32 [n, k] = q * 2^e from nibble bytes [n, k / 2] and block exponents [n, k / 32]."""
    n = nib.shape[0]
    codes = torch.stack((nib & 15, nib >> 4), dim=2).view(n, -1).long().cpu()
    vals = decode_table()[codes].view(n, -1, BLOCK)
    return torch.ldexp(vals, e.cpu().to(torch.int32)[..., None]).view(n, -1)


def dequantized_state_dict(sd):
    """The checkpoint an fp4 context computes on: every quantised decoder matrix replaced by its q * 2^e (fp32), the rest untouched."""
    out = {}
    for k, t in sd.items():
        if isinstance(t, torch.Tensor) and ".layers." in k and k.endswith(W4_SUFFIXES):
            nib, _, e, _ = quantize(t)
            out[k] = dequantize(nib, e)
        else:
            out[k] = t
    return out


def crafted_matrix(n=8, k=1536, seed=0):
    """fp32 [n, k]: Gaussian rows with a zero block, a block with one outlier, a block whose amax sits exactly on 6 * 2^e, exact ties,
    a -0 and a value beyond the clamp."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k, generator=g) * 0.02
    w[1, 64:96] = 0.0                                            # a zero block: e = -15
    w[2, 32:64] = w[2, 32:64].clamp(-0.01, 0.01); w[2, 40] = 5.0              # one outlier: everything else rounds to 0
    w[3, 0:32] = w[3, 0:32].clamp(-0.04, 0.04); w[3, 5] = 6.0 * 2.0 ** -7      # amax exactly on 6 * 2^-7 = 0.046875
    w[4, 0:32] = w[4, 0:32].clamp(-0.04, 0.04); w[4, 5] = float(torch.nextafter(torch.tensor(6.0 * 2.0 ** -7), torch.tensor(1.0)))
    w[5, 0:8] = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -6.0])    # every tie, at e = 0
    w[5, 8:16] = -w[5, 0:8]
    w[5, 16:32] = 0.0; w[5, 17] = -0.0
    w[6, 96:128] = w[6, 96:128] * 1e-8                           # far below the clamp: e = -15 and codes 0
    w[7, 0] = 3.0e4                                              # beyond 6 * 2^7: e = 7, saturates
    return w


@functools.lru_cache(maxsize=None)
def host_exe(name):
    """Path of tests/host/<name>.cpp built with ASan + UBSan (None: no host C++ compiler), as tests/kv8_ref.py builds its program."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    if cxx is None:
        return None
    exe = os.path.join(tempfile.mkdtemp(prefix="w4_"), name)
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, os.path.join(ROOT, "tests", "host", name + ".cpp")]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    elif "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]
    subprocess.run(cmd, check=True, cwd=ROOT)
    return exe


@functools.lru_cache(maxsize=None)
def host_lines():
    """stdout lines of w4_check without arguments, by their first letter: {"D": [(a, b), ...], "E": ..., "X": ..., "H": [(e, code, ok)]}."""
    exe = host_exe("w4_check")
    if exe is None:
        return None
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "w4_check: ok" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
    rows = [l.split() for l in res.stdout.splitlines() if l[:2] in ("D ", "E ", "X ", "H ")]
    return {k: [tuple(int(t) for t in r[1:]) for r in rows if r[0] == k] for k in "DEXH"}


def host_quantize(w: torch.Tensor) -> torch.Tensor:
    """The canonical block (uint8) the host program makes of the fp32 matrix w."""
    exe = host_exe("w4_check")
    d = tempfile.mkdtemp(prefix="w4q_")
    src, dst = os.path.join(d, "w.f32"), os.path.join(d, "w.blk")
    w.contiguous().numpy().astype("float32").tofile(src)
    subprocess.run([exe, src, str(w.shape[0]), str(w.shape[1]), dst], check=True)
    with open(dst, "rb") as f:
        return torch.frombuffer(bytearray(f.read()), dtype=torch.uint8)
