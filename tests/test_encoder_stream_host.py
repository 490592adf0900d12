"""Host side of the encoder's streaming passes (tests/encoder_stream_oracle.py, csrc/encoder.hip): the bit-exact restatement of the top-down
blend holds the bound derived for the expression against fp64 bilinear interpolation and has ATen's NaN mask, and the forms
stemseg_hip_encoder_stream_forms reports are those of the predicates restated in Python -- no GPU needed."""
import numpy as np
import pytest

from tests import encoder_stream_oracle as eso


@pytest.mark.parametrize("shape", eso.UP2_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restated_blend_within_the_derived_bound_of_fp64(shape):
    fine, coarse = eso.up2_inputs(shape)
    got, ref, bound = eso.up2_restated(fine, coarse), eso.up2_fp64(fine, coarse), eso.up2_bound(fine, coarse)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print("[up2 restated] %s max|err| %.3e = %.2f x 2^-24 x scale, bound 6" % (shape, err, err / (bound / 6.0)))
    assert got.dtype == np.float32 and err <= bound


@pytest.mark.parametrize("where", ["coarse", "fine"])
@pytest.mark.parametrize("hw", [(2, 2), (4, 4), (6, 12), (8, 10)], ids=lambda s: "x".join(map(str, s)))
def test_restated_blend_nan_mask_is_atens(hw, where):
    """inf, -inf and NaN in border rows and columns of either map: NaN where fp64 ATen gives NaN (weight 0 x inf at column / row 0 included),
    the same infinities elsewhere."""
    fine, coarse = eso.up2_nonfinite_inputs(*hw, where)
    got, ref = eso.up2_restated(fine, coarse), eso.up2_fp64(fine, coarse)
    assert np.isnan(ref).any()
    for f in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(f(got), f(ref))
    if where == "coarse" and hw[1] >= 4:
        # an inf in coarse column 1 reaches output column 0 at weight 0
        hit = [i for i in range(coarse.shape[0]) if np.isinf(coarse[i, 0, :, 1]).any()]
        assert hit and all(np.isnan(got[i, 0, :, 0]).any() for i in hit)


SIZES = [(32, 32), (32, 64), (64, 96), (96, 160), (480, 864), (640, 1152), (608, 1952)]


@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_stream_forms_are_the_restated_predicates(hw, T):
    import ctypes
    from stemseg_amd import hip
    e = hip.EncoderDesc()
    e.struct_bytes = ctypes.sizeof(hip.EncoderDesc)
    for i, n in enumerate((3, 4, 6, 3)):
        e.blocks[i] = n
    e.T, e.H, e.W, e.out_channels, e.precision, e.n_clips = T, hw[0], hw[1], 256, hip.PRECISIONS["f16x3"], 1
    e.conv2_groups, e.width_per_group = 1, 64
    got = hip.encoder_stream_forms(e)
    assert got == eso.encoder_stream_forms(T, *hw)
    # every accepted size has a multiple-of-16 stem output: the max-pool takes the 16-byte form; no level's in-place add is scalar
    assert got[0] == eso.STREAM_VEC4 and eso.UP2_SCALAR not in got[4:]

