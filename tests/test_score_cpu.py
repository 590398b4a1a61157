"""Host side of teacher-forced scoring (LMM.forward): the numpy restatement of the reference's collate_fn, the row-grouping rule
of LMM.forward, and the dataset item built from a mesh file.  No GPU needed."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_stubs  # noqa: E402


def _opt(**kw):
    from edgerunner_amd.options import config_defaults
    return dataclasses.replace(config_defaults["ArAE"], **kw)


def _ragged_items(seed=0):
    rng = np.random.default_rng(seed)
    items = []
    for i, n in enumerate((7, 19, 12, 30)):
        items.append({"cond": rng.standard_normal((16, 3)).astype(np.float32), "num_faces": 100 * (i + 1), "len": n,
                      "coords": rng.integers(3, 518, n), "azimuth": 0, "path": f"m{i}.obj"})
    return items


def test_collate_fn_matches_reference_live():
    """core/provider.py:469-541 run live on the same ragged batch: padding, truncation at max_seq_length (the 30-token item), -100
    labels over the cond tokens and BOS."""
    if not ref_stubs.reference_available():
        pytest.skip("/root/reference not present")
    ref_stubs.install()
    import core.provider as rp
    from edgerunner_amd.provider import collate_fn
    # 64: every item padded; 5: every item truncated (a batch mixing both makes the reference's np.stack raise - see
    # test_collate_fn_layout for what the restatement does there)
    for max_seq in (64, 5):
        opt = _opt(max_seq_length=max_seq)
        items = _ragged_items()
        want = rp.collate_fn(items, opt)
        got = collate_fn(items, opt)
        assert sorted(got) == sorted(want)
        for k in want:
            if k == "paths":
                assert got[k] == want[k]
            else:
                assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (max_seq, k)


def test_collate_fn_layout():
    """What LMM.forward relies on: right padding, -100 labels wherever the mask is 0, truncated rows without EOS (one more padding
    position than the reference would give them: its np.stack cannot mix them with padded rows)."""
    from edgerunner_amd.provider import collate_fn
    opt = _opt(max_seq_length=24)
    items = _ragged_items()
    d = collate_fn(items, opt)
    C = opt.num_cond_tokens
    B, S = d["labels"].shape
    assert (B, S) == (4, C + 1 + 24 + 1)                 # the 30-token item is truncated to 24, no EOS
    assert d["tokens"].shape == (4, 1 + 24 + 1)
    lens = d["masks"].sum(1)
    assert torch.equal(d["masks"], torch.arange(S)[None] < lens[:, None])
    assert (d["labels"][~d["masks"]] == -100).all()
    assert (d["labels"][:, : C + 1] == -100).all()
    assert lens.tolist() == [C + 1 + 7 + 1, C + 1 + 19 + 1, C + 1 + 12 + 1, C + 1 + 24]
    assert d["labels"][0, C + 1 + 7].item() == opt.eos_token_id and d["labels"][3, -2].item() == items[3]["coords"][23]
    assert d["labels"][3, -1].item() == -100 and d["tokens"][3, -1].item() == opt.pad_token_id
    assert torch.equal(d["num_tokens"], lens)


def test_score_row_groups():
    from edgerunner_amd.models import score_row_groups
    from edgerunner_amd.weights import dims_from_options
    d = dims_from_options(_opt())
    width = max(d.intermediate_dim, 3 * d.hidden_dim, d.vocab_size)
    assert score_row_groups(3, 2100, d) == [(0, 3)]
    # the 32-bit bound of the prefill: B * S * width < 2^31
    S = 43011
    per = (2 ** 31 - 1) // (S * width)
    assert per == 8
    groups = score_row_groups(20, S, d)
    assert groups == [(0, 8), (8, 16), (16, 20)]
    for b0, b1 in groups:
        assert (b1 - b0) * S * width < 2 ** 31
    assert score_row_groups(9, S + 1000, d) == [(b, min(b + 7, 9)) for b in range(0, 9, 7)]
    # the context's batch limit
    assert score_row_groups(2000, 10, d) == [(0, 1023), (1023, 2000)]
    assert score_row_groups(5, 10, d, max_rows=2) == [(0, 2), (2, 4), (4, 5)]
    with pytest.raises(ValueError):
        score_row_groups(1, 2 ** 31 // width + 1, d)
    with pytest.raises(ValueError):
        score_row_groups(0, 10, d)


def _write_box(path, scale=1.0):
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) * scale
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    with open(path, "w") as fh:
        for p in v:
            fh.write(f"v {p[0]} {p[1]} {p[2]}\n")
        for q in quads:
            fh.write(f"f {q[0] + 1} {q[1] + 1} {q[2] + 1}\nf {q[0] + 1} {q[2] + 1} {q[3] + 1}\n")


def test_mesh_item_and_collate(tmp_path):
    from edgerunner_amd import meshio
    from edgerunner_amd.meto import get_tokenizer, tokenize_mesh
    from edgerunner_amd.provider import collate_fn, mesh_item
    opt = _opt(point_num=256)
    tok, _ = get_tokenizer(opt)
    p = str(tmp_path / "box.obj")
    _write_box(p, 0.5)
    it = mesh_item(p, opt, tok)
    v, f = meshio.load_mesh(p)
    want = tokenize_mesh(meshio.normalize_mesh(v, bound=0.95), f, opt.discrete_bins, tok)
    assert np.array_equal(it["coords"], want) and it["len"] == len(want) and it["num_faces"] == 12
    assert it["cond"].shape == (256, 3) and np.abs(it["cond"]).max() <= 0.95 + 1e-6
    assert np.array_equal(mesh_item(p, opt, tok)["cond"], it["cond"])          # seeded by (opt.seed, file name)
    d = collate_fn([it, it], opt)
    assert d["conds"].shape == (2, 256, 3) and d["labels"].shape == (2, opt.num_cond_tokens + it["len"] + 2)
