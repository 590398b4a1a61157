"""Unit tests of the DiT sampler's and the CLIP front's row / element-wise kernels (csrc/k_dit.h), each through the launcher the
product calls.  References, gates and mutants: tests/rowops_ref.py, tests/test_rowops_ref_cpu.py; the kernels of csrc/k_rowops.h:
tests/test_gpu_rowops.py.

  kernel                          launcher                 product call sites                                 test
  ln_modulate_rows_kernel<16, 4>  dit_ln_mod               dit_forward_impl: norm1, norm2, norm_out           test_ln_modulate[4096-*], ..._rpw_env
  ln_modulate_rows_kernel<16, 1>  dit_ln_mod               (rows < 4096 or not in fours; ER_DIT_LN_RPW=1)     test_ln_modulate[4100-*, 5-*]
  adaln_gate_kernel               launch_adaln_gate        (unit entry only)                                  test_adaln_gate
  adaln_gate_all_kernel           launch_adaln_gate_all    dit_forward_impl                                   test_adaln_gate_all
  timestep_embed_kernel           launch_timestep_embed    dit_time_embed                                     test_timestep_embed
  silu_kernel                     launch_silu              dit_time_embed                                     test_silu_gelu[silu-*]
  gelu_kernel                     launch_gelu              er_dit_encode_image (in place)                     test_silu_gelu[gelu-*]
  ddim_cfg_step_kernel            launch_ddim_cfg_step     er_dit_sample (v-prediction)                       test_ddim_cfg_step[0-*]
  ddim_cfg_step_eps_kernel        launch_ddim_cfg_step     er_dit_sample (epsilon)                            test_ddim_cfg_step[1-*]
  clip_preprocess_kernel          launch_clip_preprocess   er_dit_encode_image                                test_clip_preprocess
  clip_im2col_kernel              launch_clip_im2col       er_dit_encode_image                                test_clip_im2col
  clip_assemble_kernel            launch_clip_assemble     er_dit_encode_image                                test_clip_assemble"""
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowops_ref as R  # noqa: E402
from test_gpu_rowops import DEV, Guarded, K, native_error  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}


def note(op, r, where):
    if r > WORST.get(op, (-1.0, ""))[0]:
        WORST[op] = (r, where)
    print(f"{op} {where}: worst err / gate {r:.3f}")


# ---------------------------------------------------------------------------------------------- ln_modulate
def run_ln_modulate(c, sh, sc, in_place, with_y16):
    """-> (y [rows, C] cpu, y16 or None); x, table and tvec are views into larger allocations (the others' rows are NaN)"""
    n = c.rows * c.C
    src = Guarded(n, torch.float32, c.x.to(DEV))
    dst = src if in_place else Guarded(n, torch.float32)
    y16 = Guarded(n, torch.float16) if with_y16 else None
    ta, tv = c.table_alloc.to(DEV), c.tvec_alloc.to(DEV)
    K().ln_modulate_(src.live, dst.live, c.rows, c.rpb, c.C, ta[1:], tv[1:], c.t_bstride, c.t_cstride, sh, sc, y16.live if with_y16 else None)
    torch.cuda.synchronize()
    assert dst.guards_intact() and src.guards_intact() and (y16 is None or y16.guards_intact())
    if not in_place:
        assert R.bits_equal(src.live.view(c.rows, c.C), c.x)
    return dst.live.view(c.rows, c.C).cpu(), (y16.live.view(c.rows, c.C).cpu() if with_y16 else None)


@pytest.mark.parametrize("in_place,with_y16", [(True, True), (False, False)])
@pytest.mark.parametrize("layout", ["layer", "out"])
@pytest.mark.parametrize("rows,rpb", [(4096, 2048), (4100, 2050), (5, 5)])
def test_ln_modulate(rows, rpb, layout, in_place, with_y16):
    """4096 rows in fours: the four-rows-per-wave kernel; 4100 = 2 x 2050 (rows_per_batch not in fours) and 5: one row per wave.
    Both table layouts with the indices the DiT layer (0, 1), (3, 4) and the output layer (0, 1) pass; y16 == y.half() bit for bit."""
    c = R.ln_mod_case(rows, rpb, layout, 200)
    for sh, sc in c.idx:
        y, y16 = run_ln_modulate(c, sh, sc, in_place, with_y16)
        r = R.check_rows(y, R.ln_modulate(c.x, rpb, c.table, c.tvec, sh, sc), R.ln_modulate(c.x, rpb, c.table, c.tvec, sh, sc, dt=torch.float32),
                         c.hard, R.TOL_LAYERNORM, f"ln_modulate {rows} {layout} ({sh}, {sc})")
        note("ln_modulate", r, f"{rows}/{rpb} {layout} ({sh}, {sc})")
        if with_y16:
            assert R.bits_equal(y16, y.half()), "y16 is y rounded to fp16"


RPW_CHILD = """
import sys, torch
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import rowops_ref as R
from test_gpu_dit_elementwise import run_ln_modulate
c = R.ln_mod_case(4096, 2048, "layer", 200)
torch.save(run_ln_modulate(c, 3, 4, True, True), {out!r})
"""


def test_ln_modulate_rpw_env_gives_equal_bits(tmp_path):
    """ER_DIT_LN_RPW=1 (read once per process: a child) sends the 4096-row case to the one-row-per-wave kernel: the same bits"""
    c = R.ln_mod_case(4096, 2048, "layer", 200)
    y, y16 = run_ln_modulate(c, 3, 4, True, True)
    out = str(tmp_path / "rpw1.pt")
    env = dict(os.environ, ER_DIT_LN_RPW="1")
    res = subprocess.run([sys.executable, "-c", RPW_CHILD.format(tests=os.path.join(ROOT, "tests"), root=ROOT, out=out)], env=env,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    y1, y16_1 = torch.load(out)
    assert R.bits_equal(y1, y) and R.bits_equal(y16_1, y16)


def test_ln_modulate_refusals():
    c = R.ln_mod_case(5, 5, "layer", 200)
    x, y = Guarded(5 * 1024, torch.float32, c.x.to(DEV)), Guarded(5 * 1024, torch.float32)
    ta, tv = c.table_alloc.to(DEV), c.tvec_alloc.to(DEV)
    for a in (dict(cols=512), dict(cols=1536), dict(rpb=2), dict(rows=0), dict(t_bstride=6 * 1024 + 2), dict(sh=-1)):
        p = dict(rows=5, rpb=5, cols=1024, t_bstride=6 * 1024, sh=0)
        p.update(a)
        with pytest.raises(native_error()):
            K().ln_modulate_(x.live, y.live, p["rows"], p["rpb"], p["cols"], ta[1:], tv[1:], p["t_bstride"], 1024, p["sh"], 1, None)
    torch.cuda.synchronize()
    assert bool(R.is_sentinel(y.all).all()), "a refused call writes nothing"


# ---------------------------------------------------------------------------------------------- adaLN gates
@pytest.mark.parametrize("B,C", [(3, 1024), (3, 100)])
def test_adaln_gate(B, C):
    """one fp32 add, bit for bit; 3 x 100 is no multiple of the 256-thread block"""
    table, tada = R.randn(210, 6, C), R.randn(211, B, 6, C)
    for idx in (2, 5, 0):
        out = Guarded(B * C, torch.float32)
        K().adaln_gate_(table.to(DEV), tada.to(DEV), out.live, B, C, idx)
        torch.cuda.synchronize()
        assert R.bits_equal(out.live.view(B, C), R.adaln_gate(table, tada, idx)) and out.guards_intact()
    with pytest.raises(native_error()):
        K().adaln_gate_(table.to(DEV), tada.to(DEV), out.live, B, C, 6)


@pytest.mark.parametrize("B,C", [(3, 1024), (3, 100)])
def test_adaln_gate_all(B, C):
    tables, tada = [R.randn(220 + i, 6, C) for i in range(2)], R.randn(223, B, 6, C)
    out = Guarded(2 * 2 * B * C, torch.float32)
    K().adaln_gate_all_([t.to(DEV) for t in tables], tada.to(DEV), out.live, B, C)
    torch.cuda.synchronize()
    assert R.bits_equal(out.live.view(2, 2, B, C), R.adaln_gate_all(tables, tada)) and out.guards_intact()


# ---------------------------------------------------------------------------------------------- timestep embedding
def test_timestep_embed():
    """t in {0, 0.5, 1, 500, 999}, half = 128: one gate per timestep (the small ones near 1e-7, 999 near 1e-4)"""
    t = torch.tensor([0.0, 0.5, 1.0, 500.0, 999.0])
    out = Guarded(5 * 256, torch.float32)
    K().timestep_embed_(t.to(DEV), out.live, 5, 128)
    torch.cuda.synchronize()
    assert out.guards_intact()
    got = out.live.view(5, 256).cpu()
    for i in range(5):
        r = R.check(got[i:i + 1], R.timestep_embed(t[i:i + 1], 128), R.timestep_embed(t[i:i + 1], 128, torch.float32), None, None,
                    f"timestep_embed t={float(t[i])}")
        note("timestep_embed", r, f"t={float(t[i])}")


# ---------------------------------------------------------------------------------------------- silu, gelu
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("values", ["grid", "randn"])
@pytest.mark.parametrize("n", [70001, 5000])
@pytest.mark.parametrize("op", ["silu", "gelu"])
def test_silu_gelu(op, n, values, in_place):
    """a thread per element: n is no multiple of the 256-thread block (the last block is partial); in place as the CLIP MLP runs gelu,
    and out of place as the time embedding runs silu"""
    x = R.ew_values(n, 230) if values == "grid" else R.randn(230, n)
    ref = R.silu if op == "silu" else R.gelu
    src = Guarded(n, torch.float32, x.to(DEV))
    dst = src if in_place else Guarded(n, torch.float32)
    (K().silu_ if op == "silu" else K().gelu_)(src.live, dst.live, n)
    torch.cuda.synchronize()
    assert dst.guards_intact() and src.guards_intact()
    if not in_place:
        assert R.bits_equal(src.live, x)
    note(op, R.check(dst.live.cpu(), ref(x), ref(x, torch.float32), None, None, f"{op} n={n} {values}"), f"n={n} {values}")


# ---------------------------------------------------------------------------------------------- DDIM + guidance
@pytest.mark.parametrize("n", [1000, 3 * 2048 * 64])
@pytest.mark.parametrize("ptype", [0, 1])
def test_ddim_cfg_step(ptype, n):
    """both prediction types at the first, a middle and the last step of the 6- and the 50-step schedule (epsilon divides by sa_t at its
    smallest at the first step), guidance 1, 7.5 and 0; latents updated in place, pred unchanged"""
    x, pred = R.randn(240, n), R.randn(241, 2 * n)
    pd = Guarded(2 * n, torch.float32, pred.to(DEV))
    for cname, sa_t, sb_t, sa_p, sb_p in R.ddim_coefficients():
        for g in (1.0, 7.5, 0.0):
            lat = Guarded(n, torch.float32, x.to(DEV))
            K().ddim_cfg_step_(lat.live, pd.live, n, ptype, g, sa_t, sb_t, sa_p, sb_p)
            torch.cuda.synchronize()
            assert lat.guards_intact()
            co = (sa_t, sb_t, sa_p, sb_p)
            r = R.check(lat.live.cpu(), R.ddim_step(x, pred, n, ptype, g, *co), R.ddim_step(x, pred, n, ptype, g, *co, dt=torch.float32),
                        None, None, f"ddim type {ptype} n={n} {cname} g={g}")
            note(f"ddim {'v' if ptype == 0 else 'eps'}", r, f"n={n} {cname} g={g}")
    assert pd.guards_intact() and R.bits_equal(pd.live, pred), "pred is read only"
    with pytest.raises(native_error()):
        K().ddim_cfg_step_(lat.live, pd.live, n, 2, 1.0, 1.0, 0.0, 1.0, 0.0)


# ---------------------------------------------------------------------------------------------- CLIP front
@pytest.mark.parametrize("H,W", [(14, 14), (28, 28), (61, 45), (1, 1)])
def test_clip_preprocess(H, W):
    """OUT = 28: up, identity (the normalised image to one rounding), down and non-square, a single pixel; B = 2"""
    B, OUT = 2, 28
    img = R.clip_image(B, H, W, 250)
    out = Guarded(B * 3 * OUT * OUT, torch.float32)
    K().clip_preprocess_(img.to(DEV), out.live, B, H, W, OUT)
    torch.cuda.synchronize()
    assert out.guards_intact()
    got = out.live.view(B, 3, OUT, OUT).cpu()
    note("clip_preprocess", R.check(got, R.clip_preprocess(img, OUT), R.clip_preprocess(img, OUT, torch.float32), None, None,
                                    f"clip_preprocess {H}x{W}"), f"{H}x{W}")
    if (H, W) == (OUT, OUT):
        mean = torch.tensor(R.CLIP_MEAN, dtype=torch.float32).double()[None, :, None, None]
        std = torch.tensor(R.CLIP_STD, dtype=torch.float32).double()[None, :, None, None]
        norm = (img.double() - mean) / std
        # one rounding of the quotient (the fp32 difference is exact or rounded once more: two ulps at the most)
        assert bool(((got.double() - norm).abs() <= 2 * R.ulp32(norm)).all()), "identity resize: the normalised image"


@pytest.mark.parametrize("S,P,lda", [(28, 14, 592), (8, 4, 48)])
def test_clip_im2col(S, P, lda):
    B = 2
    px = R.randn(260, B, 3, S, S)
    G = S // P
    out = Guarded(B * G * G * lda, torch.float32)
    K().clip_im2col_(px.to(DEV), out.live, B, S, P, lda)
    torch.cuda.synchronize()
    assert R.bits_equal(out.live.view(B * G * G, lda), R.clip_im2col(px, P, lda)) and out.guards_intact()
    with pytest.raises(native_error()):
        K().clip_im2col_(px.to(DEV), out.live, B, S, P, 3 * P * P - 4)


def test_clip_assemble():
    B, NP, C = 2, 4, 1280
    patches, cls, pos = R.randn(270, B, NP, C), R.randn(271, C), R.randn(272, NP + 1, C)
    out = Guarded(B * (NP + 1) * C, torch.float32)
    K().clip_assemble_(patches.to(DEV), cls.to(DEV), pos.to(DEV), out.live, B, NP, C)
    torch.cuda.synchronize()
    assert R.bits_equal(out.live.view(B, NP + 1, C), R.clip_assemble(patches, cls, pos)) and out.guards_intact()


def test_zz_worst_ratios():
    for op in sorted(WORST):
        print(f"rowops worst: {op:16s} {WORST[op][0]:.3f}  at {WORST[op][1]}")
    assert all(r <= 1.0 for r, _ in WORST.values())
