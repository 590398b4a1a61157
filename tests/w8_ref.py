"""torch-CPU restatement of the fp8 mode's row quantiser (edgerunner_amd/csrc/er_w8.h), with torch's own ``float8_e4m3fn`` cast:

    e[n]    = the smallest integer with amax(row n) * 2^-e <= 448, clamped to [-15, 7]; a zero row gets -15
    q[n][k] = e4m3fn(clamp(w * 2^-e, +-448)), round to nearest even (torch's cast does not saturate: the clamp comes first)
    value   = q * 2^e, an fp16 number

The exponent comes from ``torch.frexp`` (exponent and mantissa bits), never from a logarithm."""
import torch

E_MIN, E_MAX, W8_MAX = -15, 7, 448.0
# the six matrices of a decoder layer that fp8 mode quantises (q / k / v each on its own rows)
W8_SUFFIXES = tuple(f"self_attn.{p}.weight" for p in ("q_proj", "k_proj", "v_proj", "out_proj")) + ("fc1.weight", "fc2.weight")


def row_exponents(w: torch.Tensor) -> torch.Tensor:
    """int32 [n]: e of every row of w [n, k] (any float dtype; finite values)."""
    amax = w.detach().to("cpu", torch.float64).abs().amax(dim=1)          # fp32 / fp16 / bf16 are exact in fp64, and so is 448 * 2^e
    m, x = torch.frexp(amax)                                                # amax = m * 2^x, m in [0.5, 1);  448 = 0.875 * 2^9
    e = x.to(torch.int64) - 9 + (m > 0.875).to(torch.int64)
    e = torch.where(amax == 0, torch.full_like(e, E_MIN), e)
    return e.clamp(E_MIN, E_MAX).to(torch.int32)


def quantize_rows(w: torch.Tensor):
    """(q uint8 [n, k], e int32 [n], w16 fp16 [n, k] = q * 2^e) of w [n, k]; raises on a non-finite value."""
    w = w.detach().to("cpu")
    if not bool(torch.isfinite(w.float()).all()):
        raise ValueError("non-finite source value")
    e = row_exponents(w)
    scaled = torch.ldexp(w.to(torch.float64), (-e).to(torch.int64)[:, None])          # exact: a power of two in fp64
    q8 = scaled.clamp(-W8_MAX, W8_MAX).to(torch.float32).to(torch.float8_e4m3fn)       # |scaled| <= 448 is exact in fp32 unless it is far
    deq = torch.ldexp(q8.to(torch.float32), e[:, None])                                # below the e4m3 grid, where both roundings give 0
    return q8.view(torch.uint8), e, deq.to(torch.float16)


def dequantize(q: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """fp32 [n, k] = q * 2^e."""
    return torch.ldexp(q.view(torch.float8_e4m3fn).to(torch.float32), e.to(torch.int32)[:, None])


def dequantized_state_dict(sd):
    """The checkpoint an fp8 context computes on: every quantised decoder matrix replaced by its q * 2^e (fp32), the rest untouched."""
    out = {}
    for k, t in sd.items():
        if isinstance(t, torch.Tensor) and ".layers." in k and k.endswith(W8_SUFFIXES):
            q, e, _ = quantize_rows(t)
            out[k] = dequantize(q, e)
        else:
            out[k] = t
    return out
