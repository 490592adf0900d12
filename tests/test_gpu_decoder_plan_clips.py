"""The decoders' planning clip count on the device (StemsegDecoderDesc.plan_clips; the host side is tests/test_decoder_plan_clips_host.py).

With ``plan_clips = 4`` every convolution of a decoder decides its split-K factor as if four clips shared the launch, whatever the call holds.
The K partition is a summation order, so what must hold is the rule the encoder's ``plan_frames`` follows: at ONE value of the constant, clip c
is the same bits alone and in any batch.  The small decoder here (in_channels 32, inter 64 / 64 / 32 / 32, 8 groups) runs at two shapes:

  * H4 x W4 = 16 x 24, where the scratch and chunk bounds, not the workgroup count, decide every factor (the plans at 0 and 4 agree);
  * 16 x 72, the first width in steps of 8 from 24 at which a factor moves while others stay split -- f16x3, T = 8: the seven stages
    split 8 / 16 / 16 / 4 / 8 / 4 / 2 ways at 0 and 8 / 16 / 16 / 4 / 8 / 2 / 1 at 4 (tests/test_decoder_plan_clips_host.py prints such tables):
    seven reduces against six, and the 4x stage takes its GroupNorm sums in the conv epilogue instead of the reduce.

The accuracy cases use the reference's widths (256 / 256 / 128 / 128, 32 groups: what the CPU oracle's GroupNorm is written for) at 24 x 40, where
the factors go from 16 / 16 / 16 / 4 / 8 / 4 / 2 to 4 / 8 / 16 / 2 / 4 / 2 / 1."""
import numpy as np
import pytest
import torch

from oracle import decoder as odec
from tests import synth

pytestmark = pytest.mark.gpu

CIN, INTER, GROUPS, H4 = 32, [64, 64, 32, 32], 8, 16
N_MAX = 5


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _small(which, T, seed=23):
    from stemseg_amd.modeling.embedding_decoder import SqueezingExpandDecoder as Emb
    from stemseg_amd.modeling.seediness_decoder import SqueezingExpandDecoder as Seed
    gn = lambda c: torch.nn.GroupNorm(GROUPS, c)     # noqa: E731
    m = Emb(CIN, INTER, 4, True, False, "xyff", NormType=gn, num_frames=T) if which == "embedding" else Seed(CIN, INTER, NormType=gn, num_frames=T)
    sd = synth.synth_state_dict([(k, v.shape) for k, v in m.state_dict().items()], seed, prefix="x.")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)).reshape(m.state_dict()[k].shape) for k, v in sd.items()})
    return m.cuda().eval()


def _levels(hip, n, T, W4, seed0=80, poison=None):
    """n clips' zero-haloed feature buffers (32x .. 4x), one allocation per level.  poison = (clip, level): one +inf in that map."""
    h32, w32 = H4 // 8, W4 // 8
    levels = [hip.alloc_padded_batch(n, CIN, T, h32 * s, w32 * s, "cuda") for s in (1, 2, 4, 8)]
    for c in range(n):
        feats = synth.synth_features(T, h32, w32, C=CIN, seed=seed0 + c)
        if poison is not None and poison[0] == c:
            feats[poison[1]][CIN // 2, T // 2, 1, 2] = np.inf
        for (bufs, g, _), f, s in zip(levels, feats, (1, 2, 4, 8)):
            hip.copy_to_volume(dev(f), 0, hip.padded_interior_view(bufs[c], g, CIN, T, h32 * s, w32 * s))
    return levels


def _single(m, levels, c, T, W4):
    return m.forward_single(([lv[0][c] for lv in levels], (T, H4, W4)), 2).clone()


def _batch(m, levels, n, T, W4):
    return m.forward_single(([lv[0][0] for lv in levels], (T, H4, W4)), 2, clip_batch=(n, [lv[2] for lv in levels])).clone()


def _reduces(hip, fn):
    """(result of fn(), split-K reduce launches it made): the library's per-tag launch counts, the reduce's own tag."""
    hip.profile_enable(True)
    hip.profile_read()
    try:
        out = fn()
        prof = hip.profile_read()
    finally:
        hip.profile_enable(False)
    return out, prof.get(hip.SPLITK_REDUCE_TAG, (0, 0, 0))[2]


# ------------------------------------------------------------------------------------------------ 1. batch invariance at plan_clips = 4
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("T,W4", [(4, 24), (8, 24), (8, 72)])
@pytest.mark.parametrize("which", ["embedding", "seediness"])
def test_clip_is_the_same_bits_alone_and_in_batches_of_2_4_5(hip, which, T, W4, precision):
    m = _small(which, T)
    m.precision, m.plan_clips = precision, 4
    levels = _levels(hip, N_MAX, T, W4)
    singles = [_single(m, levels, c, T, W4) for c in range(N_MAX)]
    assert singles[0].shape == ((6 if which == "embedding" else 1), T, H4, W4) and not torch.equal(singles[0], singles[1])
    assert all(bool(torch.isfinite(s).all()) for s in singles)
    for n in (2, 4, 5):
        batch = _batch(m, levels, n, T, W4)
        assert batch.shape[0] == n
        for c in range(n):
            assert torch.equal(batch[c], singles[c]), "%s %s T %d W4 %d: clip %d in a batch of %d differs from its single-clip call (%d values)" % (
                which, precision, T, W4, c, n, int((batch[c] != singles[c]).sum()))
    bad, where = m.check_workspaces()
    assert bad == 0, "guard words clobbered: %s" % (where,)


# ------------------------------------------------------------------------------------------------ 2. the field does what it says; 4. 0 == 1
def test_fewer_split_k_reduces_at_4_than_at_0_and_0_equals_1(hip):
    """16 x 72, T = 8, f16x3 (16 x 24 .. 16 x 64 change no factor): 7 of the 7 stages are split at plan_clips 0, 6 at 4 -- per decoder call, whatever
    the call's clip count."""
    T, W4 = 8, 72
    m = _small("embedding", T)
    m.precision = "f16x3"
    levels = _levels(hip, 4, T, W4)
    outs, counts = {}, {}
    for pc in (0, 1, 4):
        m.plan_clips = pc
        for n in (1, 4):
            outs[pc, n], counts[pc, n] = _reduces(hip, (lambda: _single(m, levels, 0, T, W4)) if n == 1 else (lambda: _batch(m, levels, 4, T, W4)[0].clone()))
    torch.cuda.synchronize()
    print("[plan_clips] split-K reduces per decoder call at 16 x 72, T = 8, f16x3: %s" % {k: v for k, v in sorted(counts.items())})
    for n in (1, 4):
        assert 0 < counts[4, n] < counts[0, n], counts
        assert counts[1, n] == counts[0, n]
        assert counts[0, n] == 7 and counts[4, n] == 6, counts
        assert torch.equal(outs[0, n], outs[1, n]), "plan_clips 0 and 1 differ"
    for pc in (0, 1, 4):
        assert torch.equal(outs[pc, 1], outs[pc, 4])
    # a round-off level move, not another function: the bound tests/test_gpu_parity.py holds the folded linear tail to against the step-by-step form
    rel = float(((outs[4, 1] - outs[0, 1]).abs() / outs[0, 1].abs().clamp(min=1.0)).max())
    print("[plan_clips] plan_clips 4 vs 0: max |diff| / max(1, |x|) %.3g" % rel)
    assert rel <= 2e-5


@pytest.mark.parametrize("which", ["embedding", "seediness"])
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_plan_clips_0_and_1_give_equal_outputs(hip, which, precision):
    for T, W4 in ((4, 24), (8, 24), (8, 72)):
        m = _small(which, T)
        m.precision = precision
        levels = _levels(hip, 2, T, W4)
        got = {}
        for pc in (0, 1):
            m.plan_clips = pc
            got[pc] = _batch(m, levels, 2, T, W4)
        assert torch.equal(got[0], got[1]), (which, precision, T, W4)


# ------------------------------------------------------------------------------------------------ 3. accuracy against the CPU oracle
def test_outputs_at_plan_clips_4_vs_the_oracle(hip):
    """The tolerance of the decoder golden tests for the same heads (tests/test_gpu_parity.py: max |error| <= 1e-3), T = 8, 24 x 40."""
    from stemseg_amd.modeling.embedding_decoder import SqueezingExpandDecoder as Emb
    from stemseg_amd.modeling.seediness_decoder import SqueezingExpandDecoder as Seed
    T, h32, w32 = 8, 3, 5
    gn = lambda c: torch.nn.GroupNorm(32, c)     # noqa: E731
    feats = synth.synth_features(T, h32, w32, seed=78)
    for name, m, prefix, ref_fn in (("embedding", Emb(256, [256, 256, 128, 128], 4, True, False, "xyff", NormType=gn, num_frames=T), "embedding_head.",
                                     lambda sd: odec.embedding_decoder(feats, sd, "xyff", True)),
                                    ("seediness", Seed(256, [256, 256, 128, 128], NormType=gn, num_frames=T), "seediness_head.",
                                     lambda sd: odec.seediness_decoder(feats, sd))):
        sd = synth.synth_state_dict([(k, v.shape) for k, v in m.state_dict().items()], 77, prefix=prefix)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)).reshape(m.state_dict()[k].shape) for k, v in sd.items()})
        m = m.cuda().eval()
        ref = ref_fn({prefix + k: v for k, v in sd.items()}).numpy()
        for precision in ("f16x3", "f32"):
            m.precision = precision
            for pc in (4, 0):
                m.plan_clips = pc
                out = m([dev(f)[None] for f in feats])[0].cpu().numpy()
                assert out.shape == ref.shape
                err = float(np.abs(out.astype(np.float64) - ref).max())
                print("[plan_clips] %s decoder %s plan_clips %d vs oracle: max |err| %.3e (max |ref| %.3g)" % (name, precision, pc, err, float(np.abs(ref).max())))
                if pc == 4:
                    assert err <= 1e-3


# ------------------------------------------------------------------------------------------------ 5. a non-finite input is not silent
@pytest.mark.parametrize("level", [0, 3])
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_inf_in_one_level_of_one_clip_raises_that_clips_flag(hip, level, precision):
    """Level 3 (the 4x stage) is un-split at plan_clips = 4 and 16 x 72: its GroupNorm sums come from the conv epilogue, where the split launch took
    them in the reduce; level 0 keeps the reduce.  Either way the poisoned clip's maps are non-finite and its neighbour's are untouched."""
    T, W4 = 8, 72
    m = _small("embedding", T)
    m.precision, m.plan_clips = precision, 4
    clean = _batch(m, _levels(hip, 2, T, W4), 2, T, W4)
    out = _batch(m, _levels(hip, 2, T, W4, poison=(1, level)), 2, T, W4)
    flags = [bool(hip.overflow_status([out[c].contiguous()]).any()) for c in range(2)]
    assert flags == [False, True], flags
    assert torch.equal(out[0], clean[0]) and bool(torch.isfinite(clean).all())
