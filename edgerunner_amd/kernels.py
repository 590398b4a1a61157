"""Torch-tensor wrappers over the single-kernel C-ABI entry points (``er_k_*``).
Used by the GPU unit tests and for debugging; the product path goes through
``NativeShapeOPT`` / ``er_decode``."""
from __future__ import annotations

import ctypes as C

import torch

from . import native


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def gemv(w, x, bias=None, ln_w=None, ln_b=None, resid=None, relu=False, eps=1e-5, return_xnorm=False):
    """y[b,n] = act(W x_b + bias) (+resid); LayerNorm(x) first when ln_w is given."""
    lib = native.load_library()
    B, K = x.shape
    N = w.shape[0]
    y = torch.empty((B, N), dtype=torch.float32, device=x.device)
    xn = torch.empty_like(x) if return_xnorm else None
    native.check(lib.er_k_gemv(native.ptr(w), native.ptr(bias), native.ptr(x), native.ptr(ln_w), native.ptr(ln_b),
                               native.ptr(resid), native.ptr(y), native.ptr(xn), B, N, K, int(relu), float(eps), _st()),
                 "er_k_gemv")
    return (y, xn) if return_xnorm else y


def attn_decode(q, k_cache, v_cache, lens, steps=4, variant=native.ER_ATTN_SPLIT2):
    """q [B,H*D] fp32; caches [B,H,Lcap,D] fp32, fp16 or e4m3 bytes (uint8 / float8_e4m3fn: ER_ATTN_SPLIT2 and ER_ATTN_STREAM, D = 96);
    lens: list[int] -> out [B,H*D].
    variant: native.ER_ATTN_SPLIT2 (single-row fallback), ER_ATTN_SPLIT1 (mid-size batches) or ER_ATTN_STREAM (B * heads >= 256)."""
    lib = native.load_library()
    B, H, Lcap, D = k_cache.shape
    out = torch.empty((B, H * D), dtype=torch.float32, device=q.device)
    native.check(lib.er_k_attn_decode(native.ptr(q), native.ptr(k_cache), native.ptr(v_cache), native.i32_array(lens),
                                      native.ptr(out), B, H, D, Lcap, steps, kv_type(k_cache), int(variant), _st()),
                 "er_k_attn_decode")
    return out


def kv_type(cache):
    """The kernels' cache type argument (kv_half) of a cache tensor: 0 = fp32, 1 = fp16, 2 = e4m3 bytes (uint8 or float8_e4m3fn)."""
    if cache.dtype == torch.float32:
        return 0
    if cache.dtype == torch.float16:
        return 1
    assert cache.dtype in (torch.uint8, torch.float8_e4m3fn), cache.dtype
    return 2


def kv8_encode(x):
    """The device encoder of the byte KV cache on an fp32 device tensor (``er_k_kv8_encode``): uint8 of x's shape, one e4m3fn byte per
    element - saturating at +-448, round to nearest even, the sign of zero and NaN kept (csrc/er_w8.h kv8_encode)."""
    assert x.dtype == torch.float32 and x.is_cuda
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    if x.numel():
        native.check(native.load_library().er_k_kv8_encode(native.ptr(x), native.ptr(out), x.numel(), _st()), "er_k_kv8_encode")
    return out


def kv_fork(k_cache, v_cache, src_rows, dst_rows, length):
    """``er_k_kv_fork`` in place on caches [layers, B, H, Lcap, D] of 4-, 2- or 1-byte elements: positions [0, length) of every layer
    and head of row src_rows[i] are copied to row dst_rows[i].  Enqueued on the current stream without blocking (capturable)."""
    assert k_cache.shape == v_cache.shape and k_cache.dtype == v_cache.dtype and k_cache.dim() == 5
    layers, B, H, Lcap, D = k_cache.shape
    assert len(src_rows) == len(dst_rows)
    native.check(native.load_library().er_k_kv_fork(native.ptr(k_cache), native.ptr(v_cache), k_cache.element_size(), layers, B, H, Lcap, D,
                                                    native.i32_array(src_rows), native.i32_array(dst_rows), len(src_rows), int(length),
                                                    _st()), "er_k_kv_fork")


def xt_pack_image(x):
    """The tiled hi | lo activation image of x [B, K] fp32 (K a multiple of 4), as the fast-mode matrix-core projections exchange
    it: a plain restatement of ``xt_entry`` / ``xt_pack`` in csrc/k_gemv.h.  Returns a half tensor [groups, K / 4, 32, 8]:
    entry (k4, b) of group b >> 5 is 8 halves = hi(x[b, 4 k4 .. 4 k4 + 3]), lo(the same four) with hi = half(x) and
    lo = half(x - float(hi)), both round-to-nearest-even; a group is K * 128 bytes, i.e. it starts K * 32 floats behind the previous
    one; rows the batch does not have are zero."""
    B, K = x.shape
    assert x.dtype == torch.float32 and K % 4 == 0
    G = (B + 31) // 32
    xp = torch.zeros((G * 32, K), dtype=torch.float32, device=x.device)
    xp[:B] = x
    hi = xp.half()
    lo = (xp - hi.float()).half()
    hi, lo = (t.view(G, 32, K // 4, 4).permute(0, 2, 1, 3) for t in (hi, lo))
    return torch.cat((hi, lo), dim=3).contiguous()


def xt_unpack_image(img, B=None):
    """Inverse of xt_pack_image: (hi, lo) as [B, K] half tensors (B None: every row of every group, 32 per group)."""
    G, K4, _, _ = img.shape
    hi, lo = (img[..., s].permute(0, 2, 1, 3).reshape(G * 32, K4 * 4) for s in (slice(0, 4), slice(4, 8)))
    n = G * 32 if B is None else B
    return hi[:n].contiguous(), lo[:n].contiguous()


def _i32_dev(values, device, hi, what):
    v = [int(t) for t in (values.tolist() if torch.is_tensor(values) else values)]
    assert all(0 <= t < hi for t in v), f"{what} outside [0, {hi})"      # the kernels index with these unchecked
    return torch.tensor(v, dtype=torch.int32, device=device)


def gemv_form(form, epilogue, w, B, *, x=None, bias=None, ln=None, embed=None, sk=None, resid=None, qkv=None, nw=4, rw=1, eps=1e-5,
              n=None, k=None, w_half=None, return_xnorm=False, prep_xt=False, prep_xt_image=None, xt_out_image=None, w8=None, w4=None):
    """One decode projection in one of the forms the decode step launches it in (``er_k_gemv_form``; native.ER_FORM_* / ER_EPI_*).
    w [n, k] fp32 or fp16 (None with ER_FORM_PREP).  The prologue is chosen by what is given:
      ln=(ln_w, ln_b) with x [B, k]            LayerNorm rows
      embed=(embd [V, k], posemb [P, k], tok, pos)   token + position rows (tok / pos: B ints)
      ln=... with sk=(part, bias [k], resid [B, k], slices)   LayerNorm over a deferred split-K finish
      none of them                             x itself - in the tiled forms (ER_FORM_NARROW*) x is xt_pack_image of the input
    qkv=(kcache, vcache, pos[, q_out]) for ER_EPI_QKV: caches [B, heads, l_cap, head_dim] fp32, fp16 or uint8 (e4m3 bytes) are written in place at
    pos[b].  prep_xt: also return the image the batched prologue launch writes (prep_xt_image: write into this one);
    xt_out_image: the image the tiled fc1 writes (allocated zeroed when the form needs one).
    w8=(q uint8 [n, k], wscale fp32 [n]): the row form or a matrix-core form (ER_FORM_MFMA, _MFMA_XT, _NARROW, _NARROW_DEFER) on e4m3 bytes
    and row scales in place of w (``er_k_gemv_form_w8``; gemv_form_w8).
    w4=(block uint8 [n * k / 2 + n * k / 32], n, k): the row form of qkv / fc1 / fc2, or a matrix-core form (ER_FORM_MFMA, _MFMA_XT, _NARROW,
    _NARROW_DEFER) of qkv / out_proj / fc1 / fc2, on a canonical MXFP4 block in place of w (``er_k_gemv_form_w4``; gemv_form_w4); nw / rw
    still name the fp16 row form a row launch stands in for.
    Returns a dict: y, xnorm, q, part (ER_FORM_NARROW_DEFER: [groups, k / 384 * 32 * n] raw block), prep_xt, xt_out - those the call produced."""
    lib = native.load_library()
    dev = (x if x is not None else (embed[0] if embed is not None else sk[0])).device
    if w is not None:
        n, k = w.shape
        w_half = w.dtype == torch.float16
    if w8 is not None:
        assert w is None and w8[0].dtype == torch.uint8 and w8[1].dtype == torch.float32 and w8[1].numel() == w8[0].shape[0]
        (n, k), w_half = w8[0].shape, True
    if w4 is not None:
        assert w is None and w8 is None and w4[0].dtype == torch.uint8 and w4[0].is_contiguous()
        n, k, w_half = int(w4[1]), int(w4[2]), True
        assert w4[0].numel() == n * k // 2 + n * k // 32
    a = native.ErKGemvFormArgs()
    keep = [w, x, bias, resid]
    a.w, a.bias, a.x, a.resid = (native.ptr(t).value for t in (w, bias, x, resid))
    a.w_half, a.batch, a.n, a.k, a.epilogue, a.form, a.nw, a.rw, a.eps = int(bool(w_half)), B, n, k, epilogue, form, nw, rw, eps
    pro = native.ER_PRO_NONE
    if ln is not None:
        pro = native.ER_PRO_LN
        a.ln_w, a.ln_b = native.ptr(ln[0]).value, native.ptr(ln[1]).value
    if embed is not None:
        pro = native.ER_PRO_EMBED
        embd, posemb, tok, pos = embed
        tok_d, pos_d = _i32_dev(tok, dev, embd.shape[0], "token"), _i32_dev(pos, dev, posemb.shape[0], "position")
        assert len(tok_d) == B and len(pos_d) == B and embd.shape[1] == k and posemb.shape[1] == k
        keep += [tok_d, pos_d]
        a.embd, a.posemb, a.tok, a.pos = (native.ptr(t).value for t in (embd, posemb, tok_d, pos_d))
    if sk is not None:
        pro = native.ER_PRO_LN_SK
        part, sk_bias, sk_resid, slices = sk
        groups = (B + 31) // 32
        assert part.numel() >= groups * slices * 32 * k and sk_resid.shape == (B, k) and sk_bias.numel() == k
        a.sk_part, a.sk_bias, a.sk_resid, a.sk_slices = native.ptr(part).value, native.ptr(sk_bias).value, native.ptr(sk_resid).value, slices
    a.prologue = pro
    if x is not None and pro in (native.ER_PRO_NONE, native.ER_PRO_LN):
        tiled = form in (native.ER_FORM_NARROW, native.ER_FORM_NARROW_DEFER)
        assert x.numel() * x.element_size() == ((B + 31) // 32 * 32 if tiled else B) * k * 4, "x does not hold B rows of k (tiled: whole groups)"
    out = {}
    if pro != native.ER_PRO_NONE and (return_xnorm or form == native.ER_FORM_PREP):
        out["xnorm"] = torch.empty((B, k), dtype=torch.float32, device=dev)
        a.xnorm_out = native.ptr(out["xnorm"]).value
    if prep_xt or prep_xt_image is not None:
        out["prep_xt"] = prep_xt_image if prep_xt_image is not None else torch.zeros(((B + 31) // 32, k // 4, 32, 8), dtype=torch.float16, device=dev)
        assert out["prep_xt"].numel() == (B + 31) // 32 * k * 64
        a.prep_xt_out = native.ptr(out["prep_xt"]).value
    if epilogue == native.ER_EPI_QKV and form != native.ER_FORM_PREP:
        kc, vc, pos = qkv[:3]
        _, heads, l_cap, hd = kc.shape
        assert kc.shape == vc.shape and kc.shape[0] == B and kc.dtype == vc.dtype and kc.dtype in (torch.float32, torch.float16, torch.uint8, torch.float8_e4m3fn)
        pos_d = _i32_dev(pos, dev, l_cap, "cache position")
        assert len(pos_d) == B
        out["q"] = qkv[3] if len(qkv) > 3 else torch.empty((B, heads * hd), dtype=torch.float32, device=dev)
        assert out["q"].shape == (B, heads * hd) and out["q"].dtype == torch.float32
        keep += [pos_d]
        a.pos = native.ptr(pos_d).value      # the decode step feeds the embedding and the cache append the same positions
        a.q_out, a.kcache, a.vcache = native.ptr(out["q"]).value, native.ptr(kc).value, native.ptr(vc).value
        a.kv_half, a.heads, a.head_dim, a.l_cap = kv_type(kc), heads, hd, l_cap
    elif form == native.ER_FORM_NARROW_DEFER:
        out["part"] = torch.empty(((B + 31) // 32, (k // 384) * 32 * n), dtype=torch.float32, device=dev)
        a.part_out = native.ptr(out["part"]).value
    elif form == native.ER_FORM_MFMA_XT and epilogue == native.ER_EPI_RELU:
        out["xt_out"] = xt_out_image if xt_out_image is not None else torch.zeros(((B + 31) // 32, n // 4, 32, 8), dtype=torch.float16, device=dev)
        assert out["xt_out"].numel() == (B + 31) // 32 * n * 64
        a.xt_out = native.ptr(out["xt_out"]).value
    elif form != native.ER_FORM_PREP:
        out["y"] = torch.empty((B, n), dtype=torch.float32, device=dev)
        a.y = native.ptr(out["y"]).value
    if w4 is not None:
        native.check(lib.er_k_gemv_form_w4(C.byref(a), native.ptr(w4[0]), _st()), "er_k_gemv_form_w4")
    elif w8 is not None:
        native.check(lib.er_k_gemv_form_w8(C.byref(a), native.ptr(w8[0]), native.ptr(w8[1]), _st()), "er_k_gemv_form_w8")
    else:
        native.check(lib.er_k_gemv_form(C.byref(a), _st()), "er_k_gemv_form")
    del keep
    return out


def gemv_form_w8(form, epilogue, q, wscale, B, **kw):
    """``gemv_form`` on the e4m3 bytes q [n, k] (uint8) and row scales wscale [n] of fp8 mode: the fp16 row shapes and the four
    matrix-core batched forms of qkv, out_proj, fc1 and fc2 (ER_FORM_VALU and ER_FORM_ROWS8 have no byte kernel and raise),
    bit-identical to ``gemv_form`` on the fp16 matrix q * wscale."""
    return gemv_form(form, epilogue, None, B, w8=(q, wscale), **kw)


_W8_SRC = {torch.float32: native.ER_F32, torch.float16: native.ER_F16, torch.bfloat16: native.ER_BF16}


def w8_quantize(w, device=None):
    """The fp8 weight loader's row quantiser on a matrix w [n, k] (fp32 / fp16 / bf16, host or device memory; ``er_k_w8_quantize``):
    returns (q uint8 [n, k], e int32 [n], w16 fp16 [n, k] = q * 2^e, wscale fp32 [n] = 2^e) on the device.  Raises on NaN / infinity."""
    assert w.dim() == 2 and w.dtype in _W8_SRC
    w = w.contiguous()
    dev = torch.device(device) if device is not None else (w.device if w.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    n, k = w.shape
    q = torch.empty((n, k), dtype=torch.uint8, device=dev)
    e = torch.empty((n,), dtype=torch.int32, device=dev)
    w16 = torch.empty((n, k), dtype=torch.float16, device=dev)
    ws = torch.empty((n,), dtype=torch.float32, device=dev)
    native.check(native.load_library().er_k_w8_quantize(native.ptr(w), _W8_SRC[w.dtype], 1 if w.is_cuda else 0, n, k, native.ptr(q), native.ptr(e),
                                                        native.ptr(w16), native.ptr(ws), _st()), "er_k_w8_quantize")
    return q, e, w16, ws


def gemv_form_w4(form, epilogue, block, n, k, B, **kw):
    """``gemv_form`` on the canonical MXFP4 block of a matrix [n, k] (uint8: n * k / 2 nibble bytes, then n * k / 32 e8m0 bytes;
    ``w4_quantize``): the row forms of qkv, fc1 and fc2 (n a multiple of 4; nw / rw name the fp16 row form the nibble kernel stands in
    for) and the four matrix-core batched forms of qkv, out_proj, fc1 and fc2 (any n; x, ``prep_xt``, ``xt_out_image`` and the deferred
    finish's ``part`` as for ``gemv_form_w8``) - ER_FORM_VALU, ER_FORM_ROWS8, the lm_head and an fp32 cache raise before any launch.
    Bit-identical to ``gemv_form`` on the fp16 matrix of the dequantised values."""
    return gemv_form(form, epilogue, None, B, w4=(block, n, k), **kw)


def w4_quantize(w, device=None):
    """The fp4 weight loader's block quantiser on a matrix w [n, k] (fp32 / fp16 / bf16, host or device memory, k a multiple of 32;
    ``er_k_w4_quantize``): returns (block uint8 = the canonical block, n * k / 2 nibble bytes then n * k / 32 e8m0 scale bytes,
    e int32 [n, k / 32], w16 fp16 [n, k] = q * 2^e) on the device.  Raises on NaN / infinity."""
    assert w.dim() == 2 and w.dtype in _W8_SRC and w.shape[1] % 32 == 0
    w = w.contiguous()
    dev = torch.device(device) if device is not None else (w.device if w.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    n, k = w.shape
    block = torch.empty((n * k // 2 + n * k // 32,), dtype=torch.uint8, device=dev)
    e = torch.empty((n, k // 32), dtype=torch.int32, device=dev)
    w16 = torch.empty((n, k), dtype=torch.float16, device=dev)
    native.check(native.load_library().er_k_w4_quantize(native.ptr(w), _W8_SRC[w.dtype], 1 if w.is_cuda else 0, n, k, native.ptr(block), native.ptr(e),
                                                        native.ptr(w16), _st()), "er_k_w4_quantize")
    return block, e, w16


def w4_block_parts(block, n, k):
    """(nibble bytes uint8 [n, k / 2], scale bytes uint8 [n, k / 32]) views of a canonical MXFP4 block."""
    return block[: n * k // 2].view(n, k // 2), block[n * k // 2:].view(n, k // 32)


def w4_cvt_probe(device=None):
    """What the hardware's scaled fp4 conversion makes of every byte (``er_k_w4_cvt_probe``): fp32 [23, 256, 4, 2] - block exponent
    -15 .. 7, byte value, byte select, (low nibble, high nibble)."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    out = torch.empty((23, 256, 4, 2), dtype=torch.float32, device=dev)
    native.check(native.load_library().er_k_w4_cvt_probe(native.ptr(out), _st()), "er_k_w4_cvt_probe")
    return out


def mlp_transpose(w2):
    """fc2.weight [1536, 6144] (fp32 or fp16) as the k-major copy [6144, 1536] the fused single-row MLP streams (``er_k_mlp_transpose``)."""
    assert w2.shape == (1536, 6144) and w2.dtype in (torch.float32, torch.float16)
    w2t = torch.empty((6144, 1536), dtype=w2.dtype, device=w2.device)
    native.check(native.load_library().er_k_mlp_transpose(native.ptr(w2), native.ptr(w2t), int(w2.dtype == torch.float16), _st()), "er_k_mlp_transpose")
    return w2t


class MlpSparse:
    """One layer's fused single-row MLP on fixed operands (``er_k_mlp_sparse``): ``launch()`` only enqueues the two launches on the
    current stream - no allocation, no synchronisation - so it can be captured into a graph.  Results: ``y``, ``h1`` (LN(x)),
    ``nnz`` (live neurons per workgroup); ``part`` is the scratch block of 256 chain vectors."""

    def __init__(self, w1, b1, w2t, b2, x, ln_w, ln_b, eps=1e-5):
        dev = x.device
        assert w1.shape == (6144, 1536) and w2t.shape == (6144, 1536) and w1.dtype == w2t.dtype and x.numel() == 1536
        self.keep = [w1, b1, w2t, b2, x, ln_w, ln_b]
        self.zero_row = torch.zeros(1536, dtype=torch.float32, device=dev)
        self.h1 = torch.empty(1536, dtype=torch.float32, device=dev)
        self.y = torch.empty(1536, dtype=torch.float32, device=dev)
        self.part = torch.empty((256, 1536), dtype=torch.float32, device=dev)
        self.nnz = torch.zeros(256, dtype=torch.int32, device=dev)
        a = self.args = native.ErKMlpSparseArgs()
        a.w1, a.b1, a.w2t, a.zero_row, a.b2, a.x, a.ln_w, a.ln_b, a.h1_out, a.y, a.part, a.nnz = (
            native.ptr(t).value for t in (w1, b1, w2t, self.zero_row, b2, x, ln_w, ln_b, self.h1, self.y, self.part, self.nnz))
        a.w_half, a.eps = int(w1.dtype == torch.float16), eps

    def launch(self):
        native.check(native.load_library().er_k_mlp_sparse(C.byref(self.args), _st()), "er_k_mlp_sparse")


def attn_stream_xt(q, k_cache, v_cache, lens, out_xt):
    """The streaming decode attention (head_dim 96) that also writes its rows into the tiled image out_xt (half
    [groups, heads * 24, 32, 8], xt_pack_image's layout; written in place) -> out [B, heads * 96]."""
    lib = native.load_library()
    B, H, Lcap, D = k_cache.shape
    assert D == 96 and out_xt.dtype == torch.float16 and out_xt.numel() == (B + 31) // 32 * H * D * 64
    out = torch.empty((B, H * D), dtype=torch.float32, device=q.device)
    native.check(lib.er_k_attn_stream_xt(native.ptr(q), native.ptr(k_cache), native.ptr(v_cache), native.i32_array(lens), native.ptr(out),
                                         native.ptr(out_xt), B, H, Lcap, int(k_cache.dtype == torch.float16), _st()), "er_k_attn_stream_xt")
    return out


def attn_shared(q, k_cache, v_cache, lens, leaders, prefix_len, out_xt=None, prefix_pass="valu"):
    """The decode attention under prefix groups (head_dim 96; er_set_prefix_groups): row b attends keys [0, prefix_len) of row
    leaders[b]'s cache slice and keys [prefix_len, lens[b]) of its own -> out [B, heads * 96].  out_xt (optional) as for attn_stream_xt.
    prefix_pass: "valu" (er_k_attn_shared) or "mfma" (er_k_attn_shared_mfma: the matrix-core prefix pass, fp16 caches only)."""
    if prefix_pass not in native.PREFIX_PASSES:
        raise ValueError(f"prefix_pass must be 'valu' or 'mfma', got {prefix_pass!r}")
    lib = native.load_library()
    B, H, Lcap, D = k_cache.shape
    assert D == 96 and len(lens) == B and len(leaders) == B
    if out_xt is not None:
        assert out_xt.dtype == torch.float16 and out_xt.numel() == (B + 31) // 32 * H * D * 64
    out = torch.empty((B, H * D), dtype=torch.float32, device=q.device)
    name = "er_k_attn_shared_mfma" if prefix_pass == "mfma" else "er_k_attn_shared"
    native.check(getattr(lib, name)(native.ptr(q), native.ptr(k_cache), native.ptr(v_cache), native.i32_array(lens),
                                    native.i32_array(leaders), int(prefix_len), native.ptr(out), native.ptr(out_xt), B, H, Lcap,
                                    int(k_cache.dtype == torch.float16), _st()), name)
    return out


def attn_extend(q, k_cache, v_cache, past_len, out=None):
    """The rows route of ``er_prefill_extend``'s attention (csrc/k_attn_extend.h; ``er_k_attn_extend``): q [B, n_new, heads * D] fp32,
    caches [B, heads, Lcap, D] fp32 / fp16 / uint8 (e4m3 bytes) holding positions [0, past_len + n_new) -> out [B, n_new, heads * D],
    query (b, t) over keys [0, past_len + t] of row b.  ``out``: a caller's buffer of that size (the tests put guards around it)."""
    lib = native.load_library()
    B, H, Lcap, D = k_cache.shape
    n_new = q.shape[1]
    assert q.shape == (B, n_new, H * D) and q.dtype == torch.float32 and q.is_contiguous() and v_cache.shape == k_cache.shape
    kv_half = {torch.float32: 0, torch.float16: 1, torch.uint8: 2}[k_cache.dtype]
    if out is None:
        out = torch.empty((B, n_new, H * D), dtype=torch.float32, device=q.device)
    assert out.numel() == B * n_new * H * D and out.dtype == torch.float32 and out.is_contiguous()
    native.check(lib.er_k_attn_extend(native.ptr(q), native.ptr(k_cache), native.ptr(v_cache), int(past_len), n_new, native.ptr(out), B, H,
                                      Lcap, D, kv_half, _st()), "er_k_attn_extend")
    return out


def attn_outproj3(q, k_cache, v_cache, length, wo, bo, resid):
    """Version-3 single-row path: y = Wo . attention(q, K[:length], V[:length]) + bo + resid.
    q [1536] fp32; caches [16,Lcap,96] fp32 or fp16; wo [1536,1536] fp32 or fp16."""
    lib = native.load_library()
    H, Lcap, D = k_cache.shape
    assert (H, D) == (16, 96)
    y = torch.empty((H * D,), dtype=torch.float32, device=q.device)
    native.check(lib.er_k_attn_outproj3(native.ptr(q), native.ptr(k_cache), native.ptr(v_cache), int(length), native.ptr(wo),
                                        native.ptr(bo), native.ptr(resid), native.ptr(y), Lcap,
                                        int(k_cache.dtype == torch.float16), int(wo.dtype == torch.float16), _st()),
                 "er_k_attn_outproj3")
    return y


def attn_outproj3_w8(q, k_cache, v_cache, length, wo_q, wo_scale, bo, resid):
    """``attn_outproj3`` with Wo as e4m3 bytes [1536, 1536] (uint8) and row scales [1536] (``er_k_attn_outproj3_w8``)."""
    lib = native.load_library()
    H, Lcap, D = k_cache.shape
    assert (H, D) == (16, 96) and wo_q.dtype == torch.uint8 and wo_q.shape == (H * D, H * D) and wo_scale.dtype == torch.float32 and wo_scale.numel() == H * D
    y = torch.empty((H * D,), dtype=torch.float32, device=q.device)
    native.check(lib.er_k_attn_outproj3_w8(native.ptr(q), native.ptr(k_cache), native.ptr(v_cache), int(length), native.ptr(wo_q),
                                           native.ptr(wo_scale), native.ptr(bo), native.ptr(resid), native.ptr(y), Lcap,
                                           int(k_cache.dtype == torch.float16), _st()), "er_k_attn_outproj3_w8")
    return y


def gemm(a, b, bias=None, resid=None, b_is_kn=False, relu=False, div=0.0, m=None, n=None, k=None):
    """C = A.op(B) with row strides taken from the (2-D, row-contiguous) tensors."""
    lib = native.load_library()
    M = a.shape[0] if m is None else m
    K = a.shape[1] if k is None else k
    N = (b.shape[1] if b_is_kn else b.shape[0]) if n is None else n
    c = torch.empty((M, N), dtype=torch.float32, device=a.device)
    native.check(lib.er_k_gemm(native.ptr(a), native.ptr(b), native.ptr(bias), native.ptr(resid), native.ptr(c), M, N, K,
                               a.stride(0), b.stride(0), c.stride(0), int(b_is_kn), int(relu), float(div), _st()),
                 "er_k_gemm")
    return c


def gemm_f16(a, w_half, bias=None, resid=None, relu=False):
    """C = relu?(fp16(A) . W^T + bias) (+resid) on the fp16-input MFMA path; a fp32 [M,K], w_half fp16 [N,K]."""
    lib = native.load_library()
    M, K = a.shape
    N = w_half.shape[0]
    c = torch.empty((M, N), dtype=torch.float32, device=a.device)
    native.check(lib.er_k_gemm_f16(native.ptr(a), native.ptr(w_half), native.ptr(bias), native.ptr(resid), native.ptr(c), M, N, K,
                                   a.stride(0), w_half.stride(0), c.stride(0), int(relu), _st()), "er_k_gemm_f16")
    return c


def gemm_hh(a, w_half, bias=None, resid=None, relu=False, return_half=False):
    """The same product through the LDS-DMA kernel (both operands fp16 in HBM; a is rounded to an fp16 copy first); K % 64 == 0.
    return_half: also return the epilogue's fp16 copy of the result."""
    lib = native.load_library()
    M, K = a.shape
    N = w_half.shape[0]
    c = torch.empty((M, N), dtype=torch.float32, device=a.device)
    c16 = torch.empty((M, N), dtype=torch.float16, device=a.device) if return_half else None
    native.check(lib.er_k_gemm_hh(native.ptr(a), native.ptr(w_half), native.ptr(bias), native.ptr(resid), native.ptr(c), native.ptr(c16),
                                  M, N, K, a.stride(0), w_half.stride(0), c.stride(0), int(relu), _st()), "er_k_gemm_hh")
    return (c, c16) if return_half else c


def gemm_hh_qkv(a, w_half, bias, rows_per_batch, force_tile=0):
    """Fused q/k/v projection through the LDS-DMA kernel: returns (qk16 [M, N] whose V third is left as allocated, V^T
    [M / rows_per_batch, heads, 64, rows_per_batch] in the key order of flash_attn_hh_kernel)."""
    lib = native.load_library()
    M, K = a.shape
    N = w_half.shape[0]
    heads = N // 192
    qk16 = torch.zeros((M, N), dtype=torch.float16, device=a.device)
    vt = torch.zeros((M // rows_per_batch, heads, 64, rows_per_batch), dtype=torch.float16, device=a.device)
    native.check(lib.er_k_gemm_hh_qkv(native.ptr(a.contiguous()), native.ptr(w_half.contiguous()), native.ptr(bias), native.ptr(qk16), native.ptr(vt),
                                      M, N, K, rows_per_batch, force_tile, _st()), "er_k_gemm_hh_qkv")
    return qk16, vt


def gemm_hh_geglu(a, w_half, bias, force_tile=0):
    """fp16(GEGLU(fp16(a) . W^T + b)) through the fused LDS-DMA kernel; w_half [2F, K] fp16 in checkpoint order (value rows, gate rows)."""
    lib = native.load_library()
    M, K = a.shape
    F = w_half.shape[0] // 2
    out = torch.empty((M, F), dtype=torch.float16, device=a.device)
    native.check(lib.er_k_gemm_hh_geglu(native.ptr(a.contiguous()), native.ptr(w_half.contiguous()), native.ptr(bias), native.ptr(out), M, F, K,
                                        force_tile, _st()), "er_k_gemm_hh_geglu")
    return out


def gemm_f16s(a, w_half, bias=None, resid=None, relu=False):
    """C = relu?(fp16(A) . W^T + bias) (+resid) on the fp16-input MFMA path; a fp32 [M,K], w_half fp16 [N,K]."""
    lib = native.load_library()
    M, K = a.shape
    N = w_half.shape[0]
    c = torch.empty((M, N), dtype=torch.float32, device=a.device)
    native.check(lib.er_k_gemm_f16s(native.ptr(a), native.ptr(w_half), native.ptr(bias), native.ptr(resid), native.ptr(c), M, N, K,
                                   a.stride(0), w_half.stride(0), c.stride(0), int(relu), _st()), "er_k_gemm_f16s")
    return c


def _rows_ptr(t):
    """Pointer of a 2-D tensor whose rows are contiguous (a view into a larger allocation is fine: the row stride is passed as ld)."""
    if t is None:
        return None
    assert t.dim() == 2 and t.stride(1) == 1, "rows must be contiguous"
    return t.data_ptr()


def gemm_epi(family, a, w, c, *, bias=None, resid=None, resid_mod=0, gate=None, gate_rows=0, c16=None, relu=False, div=0.0, force_tile=0):
    """One GEMM family with the whole plain epilogue (``er_k_gemm_epi``; native.ER_GEMM_F32 / F16 / F16S / HH), written in place:
      c[m][n] = resid[m % resid_mod if resid_mod else m][n] + gate[m // gate_rows][n] * relu?((a . w^T)[m][n] (/ div) + bias[n]),  c16 = fp16(c)
    a [M, K] fp32, w [N, K] fp32 (F32) or fp16, c [M, N] fp32 (None with c16), c16 [M, N] fp16 (HH only).  Every 2-D operand may be a
    view with contiguous rows into a larger tensor: its row stride is the ld the kernel gets (gate: gate_bstride; c and c16 share ldc).
    Which form runs is chosen as in the product: ER_GEMM_TILE, ER_GEMM_F32_DMA, ER_GEMM_STREAM, and force_tile for HH."""
    lib = native.load_library()
    f = native.ErKGemmEpiArgs()
    M, K = a.shape
    N = w.shape[0]
    out = c if c is not None else c16
    assert w.shape[1] == K and tuple(out.shape) == (M, N)
    assert c is None or c16 is None or c16.stride(0) == c.stride(0), "c and c16 share one row stride"
    f.a, f.w, f.resid, f.gate, f.c, f.c16 = (_rows_ptr(t) for t in (a, w, resid, gate, c, c16))
    f.bias = native.ptr(bias).value
    f.family, f.m, f.n, f.k, f.lda, f.ldb, f.ldc = family, M, N, K, a.stride(0), w.stride(0), out.stride(0)
    f.ldr = resid.stride(0) if resid is not None else 0
    f.resid_mod, f.gate_rows, f.gate_bstride = resid_mod, gate_rows, gate.stride(0) if gate is not None else 0
    f.relu, f.div, f.force_tile = int(relu), float(div), force_tile
    native.check(lib.er_k_gemm_epi(C.byref(f), _st()), "er_k_gemm_epi")


def flash_attn_f16(q, k, v, heads):
    """q [B,N,H*64], k/v [B,M,H*64] fp32 -> softmax(q k^T / 8) v, [B,N,H*64] (fp16 operands, fp32 accumulate)."""
    lib = native.load_library()
    B, N, _ = q.shape
    M = k.shape[1]
    o = torch.empty_like(q)
    native.check(lib.er_k_flash_attn_f16(native.ptr(q), native.ptr(k), native.ptr(v), native.ptr(o), B, heads, N, M, _st()),
                 "er_k_flash_attn_f16")
    return o


def flash_attn_hh(q, k, v, heads):
    """The same attention through the LDS-DMA kernel (fp16 q / k / v in HBM, V transposed per head; fp16 output widened to fp32)."""
    lib = native.load_library()
    B, N, _ = q.shape
    M = k.shape[1]
    o = torch.empty_like(q)
    native.check(lib.er_k_flash_attn_hh(native.ptr(q), native.ptr(k), native.ptr(v), native.ptr(o), B, heads, N, M, _st()),
                 "er_k_flash_attn_hh")
    return o


def flash_attn_f32(q, k, v, heads, causal=False):
    """q [B,N,H*D], k/v [B,M,H*D] fp32 -> softmax(q k^T / sqrt(D) [+ causal, key j <= i + M - N]) v in exact fp32 on the
    f32-input matrix cores, no score matrix in HBM (head_dim 64 or 96)."""
    lib = native.load_library()
    B, N, HD = q.shape
    M = k.shape[1]
    o = torch.empty_like(q)
    native.check(lib.er_k_flash_attn_f32(native.ptr(q), native.ptr(k), native.ptr(v), native.ptr(o), B, heads, N, M, HD // heads,
                                         int(causal), _st()), "er_k_flash_attn_f32")
    return o



def flash_attn_f16s(q, k, v, heads, causal=False):
    """The same attention for head_dim 96 on the fp16 matrix cores with hi/lo-split q and p; k / v must hold
    fp16-representable values (fast-mode prefix attention of batches)."""
    lib = native.load_library()
    B, N, HD = q.shape
    assert HD // heads == 96
    M = k.shape[1]
    o = torch.empty_like(q)
    native.check(lib.er_k_flash_attn_f16s(native.ptr(q), native.ptr(k), native.ptr(v), native.ptr(o), B, heads, N, M,
                                          int(causal), _st()), "er_k_flash_attn_f16s")
    return o

def layernorm(x, w, b, eps=1e-5):
    lib = native.load_library()
    y = torch.empty_like(x)
    native.check(lib.er_k_layernorm(native.ptr(x), native.ptr(w), native.ptr(b), native.ptr(y), x.shape[0], x.shape[1],
                                    float(eps), _st()), "er_k_layernorm")
    return y


def softmax_(s, cols, causal=False):
    """In place over s [rows, ld]: softmax of the first `cols` (or row+1 if causal) columns, zeros after."""
    lib = native.load_library()
    native.check(lib.er_k_softmax(native.ptr(s), s.shape[0], cols, s.stride(0), int(causal), _st()), "er_k_softmax")
    return s


def score_rows(logits, labels):
    """er_score's head on given logits [B, S, V] fp32 and labels int [B, S] -> (nll [B, S], pred [B, S] int32, loss [2] =
    {mean NLL over supervised positions, count})."""
    lib = native.load_library()
    B, S, V = logits.shape
    lab = labels.to(logits.device, torch.int32).contiguous()
    nll = torch.empty((B, S), dtype=torch.float32, device=logits.device)
    pred = torch.empty((B, S), dtype=torch.int32, device=logits.device)
    loss = torch.empty((2,), dtype=torch.float32, device=logits.device)
    native.check(lib.er_k_score_rows(native.ptr(logits), native.ptr(lab), B, S, V, native.ptr(nll), native.ptr(pred),
                                     native.ptr(loss), _st()), "er_k_score_rows")
    return nll, pred, loss


def dit_loss(pred, x0, eps, timesteps, pred_type=native.ER_PRED_V_PREDICTION, snr_gamma=None):
    """er_dit_loss's two loss kernels on given tensors [B, ...] fp32 (elements per sample a multiple of 4) -> (mse [B] unweighted,
    loss [1] = mean of w * mse); snr_gamma None = unweighted."""
    lib = native.load_library()
    B = pred.shape[0]
    n = pred[0].numel()
    args = [t.to(pred.device, torch.float32).contiguous().clone() for t in (pred, x0, eps)]     # fresh (aligned) blocks
    mse = torch.empty((B,), dtype=torch.float32, device=pred.device)
    loss = torch.empty((1,), dtype=torch.float32, device=pred.device)
    native.check(lib.er_k_dit_loss(*[native.ptr(t) for t in args], native.i32_array(torch.as_tensor(timesteps).flatten().tolist()), B, n,
                                   int(pred_type), float("nan") if snr_gamma is None else float(snr_gamma), native.ptr(mse),
                                   native.ptr(loss), _st()), "er_k_dit_loss")
    return mse, loss


def fps(points, n_samples):
    """Farthest point sampling of the downsample point encoder (csrc/k_fps.h) on clouds [B, N, 3] fp32 -> indices [B, n_samples]
    int32, 0-based within each cloud: sample 0 is point 0, then the argmax of the running min squared distance, lowest index on ties."""
    lib = native.load_library()
    x = points.to(torch.float32).contiguous()
    B, N = x.shape[0], x.shape[1]
    idx = torch.empty((B, n_samples), dtype=torch.int32, device=x.device)
    native.check(lib.er_k_fps(native.ptr(x), B, N, n_samples, native.ptr(idx), _st()), "er_k_fps")
    return idx


def nn_dist2(a, b, return_idx=True):
    """Nearest neighbour of every point of a [B, Na, 3] among b [B, Nb, 3] (csrc/k_fidelity.h; fp32, no distance matrix) ->
    (d2 [B, Na] fp32 = min_j (dx*dx + dy*dy) + dz*dz, idx [B, Na] int32 = the j that attains it, lowest j on ties)."""
    lib = native.load_library()
    a = a.to(torch.float32).contiguous()
    b = b.to(torch.float32).contiguous()
    B, Na, Nb = a.shape[0], a.shape[1], b.shape[1]
    d2 = torch.empty((B, Na), dtype=torch.float32, device=a.device)
    idx = torch.empty((B, Na), dtype=torch.int32, device=a.device) if return_idx else None
    native.check(lib.er_k_nn_dist2(native.ptr(a), native.ptr(b), B, Na, Nb, native.ptr(d2), native.ptr(idx), _st()), "er_k_nn_dist2")
    return (d2, idx) if return_idx else d2


def surface_sample(vertices, faces, vert_offsets, face_offsets, n_samples, seed=0, stream_ids=None, return_faces=True):
    """n_samples area-weighted surface samples of each mesh of a concatenated batch: vertices [sum V, 3] fp32 and faces [sum F, 3]
    int32 (indices local to their mesh) on the device, vert_offsets / face_offsets B + 1 host ints.  Sample i of mesh m draws
    Philox4x32-10(key = seed, counter = (i, stream_ids[m] or m, 0x53555246, 0)) -> (points [B, n_samples, 3] fp32, faces
    [B, n_samples] int32)."""
    lib = native.load_library()
    v = vertices.to(torch.float32).contiguous()
    f = faces.to(torch.int32).contiguous()
    B = len(vert_offsets) - 1
    assert len(face_offsets) == B + 1 and int(vert_offsets[B]) <= v.shape[0] and int(face_offsets[B]) <= f.shape[0]
    pts = torch.empty((B, n_samples, 3), dtype=torch.float32, device=v.device)
    fo = torch.empty((B, n_samples), dtype=torch.int32, device=v.device) if return_faces else None
    sid = None if stream_ids is None else (C.c_uint32 * B)(*[int(s) & 0xFFFFFFFF for s in stream_ids])
    native.check(lib.er_k_surface_sample(native.ptr(v), native.ptr(f), native.i32_array(vert_offsets), native.i32_array(face_offsets), B,
                                         int(n_samples), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), sid, native.ptr(pts),
                                         native.ptr(fo), _st()), "er_k_surface_sample")
    return (pts, fo) if return_faces else pts


FIDELITY_METRICS = ("chamfer_l1", "chamfer_l2", "hausdorff", "precision", "recall", "fscore", "mean_a2b", "mean_b2a")


def fidelity_metrics(d2_ab, d2_ba, tau):
    """d2_ab [B, Na] (reference cloud -> generated samples), d2_ba [B, Nb] (generated samples -> reference cloud), both squared
    distances in fp32 -> [B, 8] float64 in the order of FIDELITY_METRICS (fixed-order double sums: the same bits from run to run)."""
    lib = native.load_library()
    d2_ab = d2_ab.to(torch.float32).contiguous()
    d2_ba = d2_ba.to(torch.float32).contiguous()
    B, Na, Nb = d2_ab.shape[0], d2_ab.shape[1], d2_ba.shape[1]
    out = torch.empty((B, len(FIDELITY_METRICS)), dtype=torch.float64, device=d2_ab.device)
    native.check(lib.er_k_fidelity_metrics(native.ptr(d2_ab), native.ptr(d2_ba), B, Na, Nb, float(tau), native.ptr(out), _st()),
                 "er_k_fidelity_metrics")
    return out


def sample_head(logits, mode, grammar, step, last_tok, counter, unfinished, top_k=10, min_new=0, seed=0,
                eos=2, pad=0):
    """One sampling-head step. Returns (next_tok, counter, unfinished) lists."""
    lib = native.load_library()
    B, V = logits.shape
    p = native.ErDecodeParams(mode=mode, top_k=top_k, grammar=grammar, max_new_tokens=step + 1,
                              min_new_tokens=min_new, seed=seed)
    nt, co, uo = (C.c_int32 * B)(), (C.c_int32 * B)(), (C.c_int32 * B)()
    native.check(lib.er_k_sample_head(native.ptr(logits), C.byref(p), V, eos, pad, B, step, native.i32_array(last_tok),
                                      native.i32_array(counter), native.i32_array(unfinished), nt, co, uo, _st()),
                 "er_k_sample_head")
    return list(nt), list(co), list(uo)


def sample_head_ctl(logits, mode, grammar, step, last_tok, counter, unfinished, top_k=10, min_new=0, seed=0, eos=2, pad=0,
                    temperature=1.0, top_p=1.0, sampling_top_k=None):
    """One step of the sampling head with controls (``er_k_sample_head_ctl``).  ``top_k`` goes into ``er_decode_params`` as for
    ``sample_head``; ``sampling_top_k`` (None: unset) is ``er_sampling.top_k``, where 0 means no top-k filter.  Returns
    (next_tok, counter, unfinished, lp_model, lp_policy, n_kept) lists."""
    lib = native.load_library()
    B, V = logits.shape
    p = native.ErDecodeParams(mode=mode, top_k=top_k, grammar=grammar, max_new_tokens=step + 1,
                              min_new_tokens=min_new, seed=seed)
    s = native.ErSampling(temperature=float(temperature), top_p=float(top_p), top_k=int(sampling_top_k or 0),
                          top_k_set=0 if sampling_top_k is None else 1, logprobs=1)
    nt, co, uo, nk = (C.c_int32 * B)(), (C.c_int32 * B)(), (C.c_int32 * B)(), (C.c_int32 * B)()
    lm, lq = (C.c_float * B)(), (C.c_float * B)()
    native.check(lib.er_k_sample_head_ctl(native.ptr(logits), C.byref(p), C.byref(s), V, eos, pad, B, step, native.i32_array(last_tok),
                                          native.i32_array(counter), native.i32_array(unfinished), nt, co, uo, lm, lq, nk, _st()),
                 "er_k_sample_head_ctl")
    return list(nt), list(co), list(uo), list(lm), list(lq), list(nk)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., Random123) on the host: counter = 4 words, key = 2 words -> 4 words.
    The same rounds and constants as ``philox4x32_10`` in csrc/k_head.h."""
    M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
    c = [int(x) & 0xFFFFFFFF for x in counter]
    k = [int(x) & 0xFFFFFFFF for x in key]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k[0]) & 0xFFFFFFFF, p1 & 0xFFFFFFFF, ((p0 >> 32) ^ c[3] ^ k[1]) & 0xFFFFFFFF,
             p0 & 0xFFFFFFFF]
        k = [(k[0] + W0) & 0xFFFFFFFF, (k[1] + W1) & 0xFFFFFFFF]
    return c


def philox_uniform(seed: int, step: int, row: int) -> float:
    """Host replica of the device sampler's uniform draw (Philox4x32-10, key = seed,
    counter = (step, row, 0, 0), u = (x0 >> 8) * 2^-24)."""
    x = philox4x32_10((step, row, 0, 0), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return float(x[0] >> 8) / 16777216.0


# ---- the once-per-sample row, element-wise and K/V scatter kernels (er_k_* of csrc/k_rowops.h, k_dit.h, split_rows_f16_kernel).
# The caller owns every buffer - the tests put sentinels around them - so these take the tensors (or views: only the first element's
# address is passed, the strides are arguments) and the sizes as the C entries do, and enqueue on the current stream.
def _at(t):
    """Address of a tensor's or view's first element (None -> NULL); the layout behind it is the caller's argument."""
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())


def _rowop(name, *args):
    native.check(getattr(native.load_library(), name)(*args, _st()), name)


def softmax_batched_(s, rows, cols, ld, ld_pad, batch, batch_stride, causal=False, causal_off=0):
    _rowop("er_k_softmax_batched", _at(s), rows, cols, ld, ld_pad, batch, batch_stride, int(causal), causal_off)
    return s


def kv_scatter_(qkv, kcache, vcache, M, S, hidden, head_dim, l_cap, kv_bstride):
    """In place: qkv [M][3 * hidden] fp32; caches fp16, or uint8 for the e4m3 byte cache (first element of batch row 0)."""
    assert kcache.dtype == vcache.dtype and kcache.dtype in (torch.float16, torch.uint8)
    _rowop("er_k_kv_scatter", _at(qkv), _at(kcache), _at(vcache), 1 if kcache.dtype == torch.float16 else 2, M, S, hidden, head_dim,
           l_cap, kv_bstride)


def split_rows_f16_(x, hi, lo, rows, cols, ldx):
    _rowop("er_k_split_rows_f16", _at(x), _at(hi), _at(lo), rows, cols, ldx)


def add_pos_(emb, pos, out, B, S, Cc, pos0=0):
    _rowop("er_k_add_pos", _at(emb), _at(pos), _at(out), B, S, Cc, pos0)


def gather_rows_(table, ids, out, Cc, ldo):
    """ids: list of ints (host); table [rows][Cc] dense."""
    _rowop("er_k_gather_rows", _at(table), table.shape[0], native.i32_array(ids), _at(out), len(ids), Cc, ldo)


def point_embed_(pts, basis, out, M, F, ldo):
    _rowop("er_k_point_embed", _at(pts), _at(basis), _at(out), M, F, ldo)


def geglu_(u, out, rows, F):
    _rowop("er_k_geglu", _at(u), _at(out), rows, F)


def gelu_(x, y, n):
    _rowop("er_k_gelu", _at(x), _at(y), n)


def silu_(x, y, n):
    _rowop("er_k_silu", _at(x), _at(y), n)


def ln_modulate_(x, y, rows, rows_per_batch, cols, table, tvec, t_bstride, t_cstride, shift_idx, scale_idx, y16=None):
    _rowop("er_k_ln_modulate", _at(x), _at(y), rows, rows_per_batch, cols, _at(table), _at(tvec), t_bstride, t_cstride, shift_idx,
           scale_idx, _at(y16))


def adaln_gate_(table, tada, out, B, Cc, idx):
    _rowop("er_k_adaln_gate", _at(table), _at(tada), _at(out), B, Cc, idx)


def adaln_gate_all_(tables, tada, out, B, Cc):
    """tables: one device tensor [6][Cc] per layer."""
    ptrs = (C.c_void_p * len(tables))(*[t.data_ptr() for t in tables])
    _rowop("er_k_adaln_gate_all", C.cast(ptrs, C.c_void_p), _at(tada), _at(out), len(tables), B, Cc)


def timestep_embed_(t, out, B, half):
    _rowop("er_k_timestep_embed", _at(t), _at(out), B, half)


def ddim_cfg_step_(latents, pred, n, prediction_type, guidance, sa_t, sb_t, sa_p, sb_p):
    _rowop("er_k_ddim_cfg_step", _at(latents), _at(pred), n, prediction_type, float(guidance), float(sa_t), float(sb_t), float(sa_p),
           float(sb_p))


def clip_preprocess_(img, out, B, H, W, OUT):
    _rowop("er_k_clip_preprocess", _at(img), _at(out), B, H, W, OUT)


def clip_im2col_(px, a, B, S, P, lda):
    _rowop("er_k_clip_im2col", _at(px), _at(a), B, S, P, lda)


def clip_assemble_(patches, cls, pos, x, B, NP, Cc):
    _rowop("er_k_clip_assemble", _at(patches), _at(cls), _at(pos), _at(x), B, NP, Cc)
