"""CPU: the host side of stem_conv2d_f16x3_gen_fwd's plans -- the get-only read-backs of the plan that ran ("fx3_ran_form",
"fx3_ran_split", "fx3_ran_mfma"), the workspace size under every forced form and split of tests/fx3_form_cases.py (the function is
host-only: this pins the split clamp without a GPU), and that case table itself (eligibility of every shape for the image-tile
form, split lists that reach the prologue cases of csrc/conv_f16x3_img.hip)."""
import numpy as np
import pytest

import conv_ref as ref
from fx3_form_cases import FORMS, SHAPES, cdiv, chunks, img_eligible_forced, live_taps, q_begins, s_eff, split_list, workspace_bytes

RAN = (b"fx3_ran_form", b"fx3_ran_split", b"fx3_ran_mfma")


@pytest.fixture(scope="module")
def lib():
    from spatiotemporalentropymodel_amd import _lib
    return _lib.hip()


def test_read_backs_are_get_only(lib):
    import torch
    for name in RAN:
        before = lib.stem_tuning_get(name)
        assert before >= 0 and (before == 0 or torch.cuda.is_available()), name          # 0 until the family's first launch in this process
        assert lib.stem_tuning_set(name, before + 1) != 0 and name in lib.stem_last_error() and b"get-only" in lib.stem_last_error()
        assert lib.stem_tuning_set(name, 0) != 0 and lib.stem_tuning_get(name) == before


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_workspace_bytes_under_forced_plans(lib, name, form):
    B, C, H, W, N, R, taps = SHAPES[name]
    n = chunks(C, R, taps)
    sel = dict(FORMS[form][0])
    old = {k: lib.stem_tuning_get(k.encode()) for k in list(sel) + ["fx3_split"]}
    try:
        for k, v in sel.items():
            assert lib.stem_tuning_set(k.encode(), v) == 0
        for s in (1, 2, 3, 5, n, n + 7):
            assert lib.stem_tuning_set(b"fx3_split", s) == 0
            got = int(lib.stem_conv2d_f16x3_gen_workspace_bytes(B, H, W, C, N, R, R, 1, R // 2, taps))
            assert got == workspace_bytes(B, H, W, N, n, s), (name, form, s, got)
            assert (got == 0) == (s_eff(n, s) == 1) and s_eff(n, s) <= min(s, n)
    finally:
        for k, v in old.items():
            lib.stem_tuning_set(k.encode(), v)


def test_every_shape_is_eligible_for_the_forced_image_tile_form():
    for name, (B, C, H, W, N, R, taps) in SHAPES.items():
        assert C % 32 == 0 and N % 4 == 0 and 0 <= taps < R * R, name
        assert img_eligible_forced(B, H, W, N, R), name
    assert not img_eligible_forced(2, 9, 11, 96, 3) and not img_eligible_forced(1, 13, 7, 160, 5)       # the half-tile rule
    assert img_eligible_forced(2, 11, 13, 96, 5)                                                         # 286 >= 256


def test_split_lists_reach_the_prologue_cases():
    """every 3x3 / 5x5 shape has a split that starts mid-slab (0 < q_begin % T < T - 1) and one that starts on a slab's last tap
    (q_begin % T == T - 1: the early store of the second halo); the first shape reaches the latter with s = 5 (cps = 4, q = 8)"""
    for name, (B, C, H, W, N, R, taps) in SHAPES.items():
        n, T = chunks(C, R, taps), live_taps(R, taps)
        splits = split_list(n)
        assert len({s_eff(n, s) for s in splits}) == len(splits) and splits[0] == 1 and s_eff(n, splits[-1]) == n, name
        assert s_eff(n, n + 7) == n
        if R == 1:
            continue
        starts = {q % T for s in splits for q in q_begins(n, s)[1:]}
        assert any(0 < t < T - 1 for t in starts), (name, starts)
        assert T - 1 in starts, (name, starts)
    n = chunks(64, 3, 0)
    assert 5 in split_list(n) and cdiv(n, 5) == 4 and q_begins(n, 5)[2] == 8 == live_taps(3, 0) - 1


def test_type_b_mask_is_type_a_plus_the_centre():
    for R in (3, 5):
        a, b = ref.mask_a(R, R), ref.mask_b(R, R)
        assert b.sum() == a.sum() + 1 and b[R // 2, R // 2] == 1 and a[R // 2, R // 2] == 0 and np.array_equal(b.reshape(-1)[:int(a.sum())], np.ones(int(a.sum())))
        assert not b[R // 2 + 1:].any() and not b[R // 2, R // 2 + 1:].any()
    assert ref.mask_b(3, 3).sum() == 5 and ref.mask_a(5, 5).sum() == 12
