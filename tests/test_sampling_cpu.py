"""Sampling controls without a GPU: the float64 restatement the GPU tests measure against (tests/sampling_ref.py) keeps exactly
what HF's warpers keep, the header and the binding agree on the new entry points, and infer.py's environment variables parse."""
import importlib.util
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(0.7, 10, 0.9), (1.3, 0, 0.8), (1.0, 50, 0.5), (0.5, 0, 0.95), (2.0, 10, 1.0)]
NEW_ENTRIES = ("er_set_sampling", "er_get_logprobs", "er_queue_row_logprobs", "er_k_sample_head_ctl")


def test_kept_set_is_what_hf_warpers_keep():
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    rows, mismatches = 0, []
    for seed in range(300):
        logits = torch.randn(518, generator=torch.Generator().manual_seed(seed)) * 3
        for temperature, top_k, top_p in CONFIGS:
            x = TemperatureLogitsWarper(temperature)(None, logits[None].clone())
            if top_k > 0:
                x = TopKLogitsWarper(top_k)(None, x)
            if top_p < 1.0:
                x = TopPLogitsWarper(top_p, min_tokens_to_keep=1)(None, x)
            _, keep, _ = R.filtered(logits, temperature, top_k, top_p)
            rows += 1
            if not torch.equal(keep, torch.isfinite(x[0])):
                mismatches.append((seed, temperature, top_k, top_p, int(keep.sum()), int(torch.isfinite(x[0]).sum())))
    assert rows == 300 * len(CONFIGS) and not mismatches, mismatches[:10]


def test_restatement_on_a_row_with_a_closed_form():
    # probabilities 0.5, 0.25, 0.125, 0.125 at ids 3, 1, 0, 2: the masses ahead are 0, 0.5, 0.75 (id 0, lower id first) and 0.875 (id 2)
    logits = torch.log(torch.tensor([0.125, 0.25, 0.125, 0.5], dtype=torch.float64))
    _, keep, margin = R.filtered(logits, 1.0, 0, 0.8)
    assert keep.tolist() == [True, True, False, True] and abs(margin - 0.05) < 1e-12
    _, keep, _ = R.filtered(logits, 1.0, 0, 1e-6)
    assert keep.tolist() == [False, False, False, True], "the first candidate always stays"
    s, keep, _ = R.filtered(logits, 1.0, 2, 1.0)
    assert keep.tolist() == [False, True, False, True]
    lp = R.policy_logprobs(s, keep)
    assert abs(float(lp[3].exp()) - 2 / 3) < 1e-12 and lp[0] == -float("inf")
    assert R.pick(s, keep, 0.2)[0] == 1 and R.pick(s, keep, 0.5)[0] == 3      # ascending id: id 1 owns [0, 1/3)
    s, keep, _ = R.filtered(logits, 0.5, 0, 1.0)                                # temperature 0.5 squares the probabilities
    assert abs(float(R.policy_logprobs(s, keep)[3].exp()) - 0.25 / (0.25 + 0.0625 + 2 * 0.015625)) < 1e-12
    assert abs(float(R.model_logprobs(logits)[1].exp()) - 0.25) < 1e-12


def test_header_and_binding_agree_on_the_new_entry_points():
    from edgerunner_amd import native
    src = open(os.path.join(ROOT, "include", "edgerunner_hip.h")).read()
    for name in NEW_ENTRIES:
        assert re.search(rf"\bint {name}\(", src) and name in native.EXPORTS, name
    m = re.search(r"typedef struct \{([^}]*)\} er_sampling;", src)
    fields = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [n for n, _ in native.ErSampling._fields_]
    from edgerunner_amd import kernels
    assert callable(kernels.sample_head_ctl)


def test_library_exports_the_new_entry_points():
    from edgerunner_amd import build, native
    build.build(verbose=False)
    lib = native.load_library()
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
    assert lib.er_abi_version() == 1


def test_plain_unit_entry_refuses_what_it_cannot_handle():
    """er_k_sample_head shares er_k_sample_head_ctl's argument check, which runs before any HIP call (there is no GPU here: a HIP
    call would fail with ER_ERR_HIP): a vocabulary above ER_HEAD_MAX_VOCAB = 1088 and a null pointer are ER_ERR_INVALID by name.  So is
    top_k <= 0 in sample mode, as in er_decode: the shared k-th-largest piece reads it as "no threshold", which only er_sampling may
    ask for (er_k_sample_head_ctl)."""
    import ctypes as C
    from edgerunner_amd import build, native
    build.build(verbose=False)
    lib = native.load_library()
    B = 2
    p = native.ErDecodeParams(mode=1, top_k=10, grammar=0, max_new_tokens=1, min_new_tokens=0, seed=0)
    logits = (C.c_float * (B * 1089))()              # never read: the entry refuses first
    state = native.i32_array([0] * B)
    outs = [(C.c_int32 * B)() for _ in range(3)]
    calls = {"vocab 1089": (C.addressof(logits), C.byref(p), 1089, 2, 0, B, 0, state, state, state, *outs, None),
             "null last_tok": (C.addressof(logits), C.byref(p), 518, 2, 0, B, 0, None, state, state, *outs, None),
             "null logits": (None, C.byref(p), 518, 2, 0, B, 0, state, state, state, *outs, None)}
    p0 = native.ErDecodeParams(mode=1, top_k=0, grammar=0, max_new_tokens=1, min_new_tokens=0, seed=0)
    calls["top_k 0 in sample mode"] = (C.addressof(logits), C.byref(p0), 518, 2, 0, B, 0, state, state, state, *outs, None)
    for what, args in calls.items():
        assert lib.er_k_sample_head(*args) == -1, what                      # ER_ERR_INVALID
        assert lib.er_last_error().decode().startswith("er_k_sample_head:"), (what, lib.er_last_error())
    assert "top_k" in lib.er_last_error().decode()


def _infer():
    spec = importlib.util.spec_from_file_location("infer_under_test", os.path.join(ROOT, "infer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_infer_env_parsing():
    f = _infer().sampling_from_env
    assert f({}) == {}
    assert f({"ER_INFER_TEMPERATURE": "0.8", "ER_INFER_TOP_P": "0.9", "ER_INFER_TOP_K": "0", "ER_INFER_LOGPROBS": "1"}) == \
        {"temperature": 0.8, "top_p": 0.9, "top_k": 0, "output_logprobs": True}
    assert f({"ER_INFER_TOP_K": "50"}) == {"top_k": 50}
    assert f({"ER_INFER_LOGPROBS": "0", "ER_INFER_TOP_P": "1"}) == {"top_p": 1.0}
    for name, bad in (("ER_INFER_TEMPERATURE", "0"), ("ER_INFER_TEMPERATURE", "-1"), ("ER_INFER_TEMPERATURE", "nan"),
                      ("ER_INFER_TEMPERATURE", "inf"), ("ER_INFER_TEMPERATURE", "warm"), ("ER_INFER_TOP_P", "0"),
                      ("ER_INFER_TOP_P", "1.01"), ("ER_INFER_TOP_P", "x"), ("ER_INFER_TOP_K", "-1"), ("ER_INFER_TOP_K", "2.5"),
                      ("ER_INFER_LOGPROBS", "yes"), ("ER_INFER_LOGPROBS", "2")):
        with pytest.raises(SystemExit, match=name):
            f({name: bad})


def test_python_argument_checks_name_the_argument():
    from edgerunner_amd.shape_opt import check_sampling
    check_sampling(1.0, 1.0, 0)
    check_sampling(0.5, 0.3, 50)
    for args, name in (((0.0, 1.0, 10), "temperature"), ((float("nan"), 1.0, 10), "temperature"), ((float("inf"), 1.0, 10), "temperature"),
                       ((1.0, 0.0, 10), "top_p"), ((1.0, 1.5, 10), "top_p"), ((1.0, 1.0, -1), "top_k")):
        with pytest.raises(ValueError, match=name):
            check_sampling(*args)
