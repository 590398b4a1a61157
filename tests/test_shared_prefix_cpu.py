"""``prefix_leaders``: the grouping behind ``LMM.generate(share_prefix=True)`` - rows whose ``conds`` entries are bit-equal form a group
named by its first row.  A pure function of the host copy of ``conds``; the leaders it returns satisfy what ``er_set_prefix_groups``
asks of a table (0 <= leader[b] <= b, leader[leader[b]] == leader[b])."""
import numpy as np
import torch

from edgerunner_amd.models import prefix_leaders


def clouds(*seeds, n=64):
    return torch.stack([torch.randn(n, 3, generator=torch.Generator().manual_seed(s)) for s in seeds])


def valid_table(leaders):
    return all(0 <= l <= b and leaders[l] == l for b, l in enumerate(leaders))


def test_equal_clouds_form_one_group():
    assert prefix_leaders(clouds(7, 7, 7, 7)) == [0, 0, 0, 0]


def test_unequal_clouds_are_singletons():
    assert prefix_leaders(clouds(1, 2, 3)) == [0, 1, 2]


def test_interleaved_clouds():
    leaders = prefix_leaders(clouds(0, 0, 3, 0, 3, 4))
    assert leaders == [0, 0, 2, 0, 2, 5] and valid_table(leaders)
    leaders = prefix_leaders(clouds(5, 6, 5, 6, 7, 5, 6))
    assert leaders == [0, 1, 0, 1, 4, 0, 1] and valid_table(leaders)


def test_single_row():
    assert prefix_leaders(clouds(9)) == [0]


def test_equality_is_on_the_bits():
    c = clouds(2, 2, 2, 2)
    c[1, 10, 1] = torch.nextafter(c[1, 10, 1], torch.tensor(float("inf")))      # one ulp in one coordinate
    c[2, 0, 0], c[3, 0, 0] = 0.0, -0.0                                            # 0.0 == -0.0 as numbers, not as bits
    assert prefix_leaders(c) == [0, 1, 2, 3]
    d = clouds(4, 4)
    d[:, 3, 2] = float("nan")                                                     # the same NaN in both rows: still one group
    assert prefix_leaders(d) == [0, 0]


def test_numpy_and_latent_shaped_input():
    a = np.zeros((3, 8, 4), dtype=np.float32)
    a[1, 2, 3] = 1.0
    assert prefix_leaders(a) == [0, 1, 0]
    assert prefix_leaders(torch.from_numpy(a).double()) == [0, 1, 0]
