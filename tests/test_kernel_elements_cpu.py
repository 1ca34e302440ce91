"""
The element-wise checkers of tests/kernel_elements.py without a GPU: float32 restatements of attn_kernel, dwconv3x3_kernel and
tta_scale_kernel pass at every shape and input class of tests/test_gpu_kernel_elements.py, and each planted mistake is caught on
the cases named here.  Shown before the GPU test is trusted.

Which inputs catch which mistake:
  attention
    padded_key_scores_0       'negative' (every real score below 0: the key left at 0 takes most of the softmax), N % 32 != 0.  On
                              Gaussian inputs its share falls with N, which is why that class alone is not enough.
    no_rescale_of_o           'ramp' (the running maximum rises in every step: every alpha is below 1), N > 32
    alpha_of_wrong_query      'gauss15', N > 32: the maximum of neighbouring queries rises in different steps
    scale_of_key_dim_64       every class; named on 'gauss075'
    tail_query_rows_stored    N % 16 != 0 with a second image: the rows land on the next image's first queries
    v_in_natural_key_order    every class with more than 4 keys; named on N = 32
  depthwise
    taps_transposed           maps with both sides above 1 (smooth input: the x and y neighbours differ)
    left_border_skips_the_right_tap   maps with W >= 2; invisible at (9, 1) and (1, 1), where x + 1 is outside anyway
    residual_added_before_silu, residual_rounded_first   act and res together -- the combination the suite never ran
    grp_off_ignored           the pe mapping (grp_off 64): the k slices are read instead of the v slices
    bias_of_the_next_channel_group    every case with more than 8 channels (every channel has its own bias); named on (1, 1)
  TTA input
    pad_value_0.5             every case (every case has pad elements), bit for bit
    no_half_pixel_offset      every case
    destination_flipped       pass 1: the mirrored row has its pad on the left.  (Mirroring the sw resized columns alone is the same
                              function: the sample positions are symmetric.)
    second_row_not_clamped    NOT caught, and cannot be: both scales are below 1, so the first neighbour is at most row h - 2 and the
                              clamp is never taken (test_tta_second_neighbour_clamp_is_never_taken).  It is listed, not claimed.
Truncation of P instead of rounding stays inside a worst-case bound and is not claimed either.
"""

import numpy as np
import pytest

import conv_probe as P
import kernel_elements as KE

DTYPES = ['bf16', 'fp16']

ATTN_NAMED = {
    'padded_key_scores_0': [('negative', 15, 1), ('negative', 33, 4), ('negative', 300, 4), ('negative', 1000, 1)],
    'no_rescale_of_o': [('ramp', 33, 1), ('ramp', 300, 4)],
    'alpha_of_wrong_query': [('gauss15', 300, 4)],
    'scale_of_key_dim_64': [('gauss075', 17, 1)],
    'tail_query_rows_stored': [('gauss075', 17, 4), ('negative', 15, 1)],
    'v_in_natural_key_order': [('gauss15', 32, 1)],
}
DW_NAMED = {            # (map, mapping, act, res)
    'taps_transposed': [((7, 9), 'c24', 1, 0), ((2, 2), 'c8', 1, 0)],
    'left_border_skips_the_right_tap': [((2, 2), 'c8', 1, 0), ((1, 9), 'c24_ld40', 1, 1)],
    'residual_added_before_silu': [((7, 9), 'c64', 1, 1), ((1, 9), 'c24_ld40', 1, 1)],
    'residual_rounded_first': [((15, 20), 'c64', 1, 1), ((7, 9), 'pe4', 0, 1)],
    'grp_off_ignored': [((7, 9), 'pe4', 0, 1), ((1, 1), 'pe4', 1, 1)],
    'bias_of_the_next_channel_group': [((1, 1), 'c24', 0, 0)],
}
TTA_NAMED = {           # (model stride, (h, w), pass)
    'pad_value_0.5': [(64, (64, 64), 1), (32, (192, 320), 2)],
    'no_half_pixel_offset': [(64, (64, 64), 2), (32, (96, 160), 1)],
    'destination_flipped': [(32, (96, 160), 1), (64, (128, 192), 1)],
}
MAPPING = {m[0]: m for m in KE.DW_MAPPINGS}


# ---- attention ----------------------------------------------------------------------------------------------------------------

def test_mfma_key_order_is_a_permutation_of_the_step():
    assert sorted(KE.MFMA_KEY_ORDER.tolist()) == list(range(32))
    assert KE.MFMA_KEY_ORDER[:8].tolist() == [0, 1, 2, 3, 16, 17, 18, 19]


@pytest.mark.parametrize('cls', KE.ATTN_CLASSES)
@pytest.mark.parametrize('dtype', DTYPES)
def test_faithful_attention_passes_and_the_classes_are_what_they_are_for(dtype, cls):
    for N in KE.ATTN_TOKENS:
        for heads in KE.ATTN_HEADS:
            qkv = KE.attention_input(cls, KE.ATTN_IMAGES, N, heads, dtype)
            assert P.is_storage(qkv, dtype)
            ref = KE.AttentionReference(qkv, heads, dtype)
            v = ref.verdict('{} {} N={} heads={}'.format(cls, dtype, N, heads), KE.emulated_attention(qkv, heads, dtype))
            assert v.over == 0 and v.size == KE.ATTN_IMAGES * N * heads * KE.HD, str(v)
            KE.assert_attention_class(cls, ref)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('mutant', KE.ATTN_MUTANTS)
def test_attention_mutant_is_caught(mutant, dtype):
    for cls, N, heads in ATTN_NAMED[mutant]:
        assert N in KE.ATTN_TOKENS and heads in KE.ATTN_HEADS
        qkv = KE.attention_input(cls, KE.ATTN_IMAGES, N, heads, dtype)
        ref = KE.AttentionReference(qkv, heads, dtype)
        v = ref.verdict(mutant, KE.emulated_attention(qkv, heads, dtype, mutant))
        assert v.over, '{} is not caught on {} N={} heads={} {}: {}'.format(mutant, cls, N, heads, dtype, v)
        print('\n{} {} {} N={} heads={}: {}'.format(mutant, dtype, cls, N, heads, v))


@pytest.mark.parametrize('dtype', DTYPES)
def test_unmasked_key_passes_the_old_bar_and_is_far_over_the_new_bound(dtype):
    """the planted padded key against the norm-wise bar of test_attention_kernel (max |d| < 2 unit_tol max |ref|, mean |d| <
    unit_tol / 4 mean |ref|) on Gaussian inputs, and against the bound on the designed class"""
    unit = 4e-3 if dtype == 'fp16' else 2e-2
    qkv = KE.attention_input('gauss15', 2, 300, 4, dtype)
    ref = KE.AttentionReference(qkv, 4, dtype)
    emax, emean = KE.norm_wise(KE.emulated_attention(qkv, 4, dtype, 'padded_key_scores_0'), ref.y)
    assert emax < 2 * unit and emean < unit / 4, (emax, emean)
    qkv = KE.attention_input('negative', 2, 300, 4, dtype)
    ref = KE.AttentionReference(qkv, 4, dtype)
    v = ref.verdict('unmasked key', KE.emulated_attention(qkv, 4, dtype, 'padded_key_scores_0'))
    assert v.worst > 25, str(v)


# ---- depthwise ----------------------------------------------------------------------------------------------------------------

def test_depthwise_cases_reach_the_grid_tail_and_a_full_grid():
    counts = {(hw, m[0]): KE.dw_threads(hw, m) for hw in KE.DW_MAPS for m in KE.DW_MAPPINGS}
    assert any(c % 256 == 0 for c in counts.values()), 'no case fills its last block'
    assert any(c % 256 and c > 256 for c in counts.values()) and any(c < 256 for c in counts.values())
    assert counts[(2, 2), 'pe4'] == 256 and counts[(15, 20), 'pe4'] % 256 == 0
    assert any(m[2] > m[1] and m[3] == m[1] for m in KE.DW_MAPPINGS), 'no plain case with ld_in > C'


@pytest.mark.parametrize('mapping', KE.DW_MAPPINGS, ids=lambda m: m[0])
@pytest.mark.parametrize('dtype', DTYPES)
def test_faithful_depthwise_passes(dtype, mapping):
    name, c, ld_in, grp, grp_stride, grp_off = mapping
    for hw in KE.DW_MAPS:
        a, w, b, r = KE.depthwise_case(hw, mapping, dtype)
        assert a.shape == (KE.DW_IMAGES, ld_in) + hw and P.is_storage(a, dtype) and P.is_storage(r, dtype)
        assert np.abs(a[1]).max() < np.abs(a[0]).max() / 16, 'the second image is not near zero'
        wr = P.round_storage(w, dtype)
        for act in (0, 1):
            for res in (0, 1):
                rr = r if res else None
                v = KE.depthwise_verdict('{} {} {} act={} res={}'.format(name, dtype, hw, act, res),
                                         KE.emulated_depthwise(a, w, b, rr, grp, grp_stride, grp_off, act, dtype),
                                         a, wr, b, rr, grp, grp_stride, grp_off, act, dtype)
                assert v.over == 0 and v.size == KE.DW_IMAGES * c * hw[0] * hw[1], str(v)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('mutant', KE.DW_MUTANTS)
def test_depthwise_mutant_is_caught(mutant, dtype):
    for hw, name, act, res in DW_NAMED[mutant]:
        assert hw in KE.DW_MAPS
        _, c, ld_in, grp, grp_stride, grp_off = MAPPING[name]
        a, w, b, r = KE.depthwise_case(hw, MAPPING[name], dtype)
        rr = r if res else None
        v = KE.depthwise_verdict(mutant, KE.emulated_depthwise(a, w, b, rr, grp, grp_stride, grp_off, act, dtype, mutant),
                                 a, P.round_storage(w, dtype), b, rr, grp, grp_stride, grp_off, act, dtype)
        assert v.over, '{} is not caught on {} {} act={} res={} {}: {}'.format(mutant, name, hw, act, res, dtype, v)
        print('\n{} {} {} {} act={} res={}: {}'.format(mutant, dtype, name, hw, act, res, v))


def test_left_border_mistake_is_invisible_on_a_one_column_map():
    """why (9, 1) alone would not do: there the tap at x + 1 is outside the map as well"""
    a, w, b, r = KE.depthwise_case((9, 1), MAPPING['c8'], 'bf16')
    same = KE.emulated_depthwise(a, w, b, None, 8, 8, 0, 1, 'bf16')
    assert np.array_equal(KE.emulated_depthwise(a, w, b, None, 8, 8, 0, 1, 'bf16', 'left_border_skips_the_right_tap'), same)


# ---- the TTA input ------------------------------------------------------------------------------------------------------------

def test_tta_cases_hold_what_they_are_for():
    """The four shapes; the stride-64 model takes the three that are multiples of 64, a stride-32 model all four.  By computation:
    an odd resized side (the image's edge inside a 2 x 2 space-to-depth cell) and a case with both sides even; a resized side that
    is a whole number of stride cells (the pad begins on a cell boundary) and sides that are not.  NO case is without padding on an
    axis, and none can be: int(h s) == ceil(h s / stride) stride needs h s to be a multiple of the stride, which 0.83 and 0.67 give for
    no h below 100 strides -- every case has pad elements on both axes, and the scaled input never outgrows the batch's buffer."""
    assert {hw for _, hw in KE.TTA_CASES} == set(KE.TTA_SHAPES) and {s for s, _ in KE.TTA_CASES} == {64, 32}
    assert [hw for s, hw in KE.TTA_CASES if s == 64] == [(64, 64), (128, 192), (192, 320)]
    geo = [(s, hw, KE.tta_geometry(*hw, p, stride=s)) for s, hw in KE.TTA_CASES for p in (1, 2)]
    assert any(g[0] % 2 or g[1] % 2 for _, _, g in geo) and any(g[0] % 2 == 0 and g[1] % 2 == 0 for _, _, g in geo)
    assert all(g[0] < g[2] and g[1] < g[3] for _, _, g in geo)
    assert any(g[0] % s == 0 or g[1] % s == 0 for s, _, g in geo) and any(g[0] % s and g[1] % s for s, _, g in geo)
    assert all(hw[0] % s == 0 and hw[1] % s == 0 and g[2] % s == 0 and g[3] % s == 0 and g[2] <= hw[0] and g[3] <= hw[1] for s, hw, g in geo)
    assert [g[4] for _, _, g in geo[:2]] == [True, False]
    assert not any(h * sc == int(h * sc) and int(h * sc) % 32 == 0 for h in range(32, 3200, 32) for sc in KE.TTA_SCALES.values())


def _case_id(case):
    return 's{}-{}x{}'.format(case[0], *case[1])


@pytest.mark.parametrize('case', KE.TTA_CASES, ids=_case_id)
@pytest.mark.parametrize('dtype', DTYPES)
def test_faithful_tta_passes_and_the_reference_is_scale_img(dtype, case):
    stride, hw = case
    imgs = KE.tta_images(2, *hw)
    assert all(im[:, :hw[1] // 2].mean() + 20 < im[:, hw[1] // 2:].mean() for im in imgs), 'no left-to-right asymmetry'
    x = KE.tta_input_tensor(imgs, dtype)
    for tta_pass in (1, 2):
        ref = KE.TtaReference(x, tta_pass, dtype, stride)
        assert np.abs(ref.y - KE.torch_scale_img(x, tta_pass, dtype, stride)).max() < 1e-14
        inner, pad = ref.verdicts('{} {} pass {}'.format(dtype, case, tta_pass), KE.emulated_tta(x, tta_pass, dtype, stride))
        assert inner.over == 0 and pad.over == 0 and pad.size > 0, (str(inner), str(pad))
        assert inner.size + pad.size == ref.y.size


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('mutant', sorted(TTA_NAMED))
def test_tta_mutant_is_caught(mutant, dtype):
    for stride, hw, tta_pass in TTA_NAMED[mutant]:
        assert (stride, hw) in KE.TTA_CASES
        x = KE.tta_input_tensor(KE.tta_images(2, *hw), dtype)
        ref = KE.TtaReference(x, tta_pass, dtype, stride)
        inner, pad = ref.verdicts(mutant, KE.emulated_tta(x, tta_pass, dtype, stride, mutant=mutant))
        assert inner.over or pad.over, '{} is not caught on {} pass {} {}'.format(mutant, hw, tta_pass, dtype)
        print('\n{} {} stride {} {} pass {}: {}; {}'.format(mutant, dtype, stride, hw, tta_pass, inner, pad))
        if mutant == 'pad_value_0.5':
            assert pad.over == pad.size and inner.over == 0


def test_tta_second_neighbour_clamp_is_never_taken():
    """f <= r (sh - 0.5) - 0.5 = h - 1 - (r - 1) / 2 < h - 1 for r = h / sh > 1: the first neighbour is at most row h - 2 at every
    shape and pass, so a kernel without the clamp of y1 (or x1) computes the same bits.  The clamp guards a scale of 1 or more,
    which mdhip_forward_tta never asks for; no input can show its absence."""
    assert set(KE.TTA_MUTANTS) - set(TTA_NAMED) == {'second_row_not_clamped'}
    for stride, hw in KE.TTA_CASES:
        x = KE.tta_input_tensor(KE.tta_images(2, *hw), 'bf16')
        for tta_pass in (1, 2):
            ref = KE.TtaReference(x, tta_pass, 'bf16', stride)
            assert ref.max_y0 <= hw[0] - 2 and ref.max_x0 <= hw[1] - 2
            assert np.array_equal(KE.emulated_tta(x, tta_pass, 'bf16', stride, mutant='second_row_not_clamped'),
                                  KE.emulated_tta(x, tta_pass, 'bf16', stride))
