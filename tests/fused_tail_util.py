"""Shared by tests/test_gpu_fused_tail.py, tests/test_gpu_fused_tail_blocks.py and tests/test_fused_tail_cases_host.py: backbones with synthetic
weights, one profiled encoder pass, the fuse_tail constants, and the tiny three-block-stage networks with their inputs (built on the CPU,
so that the validity of every GPU case -- dead-channel share, overflow positions -- is asserted without a GPU)."""
import numpy as np
import pytest
import torch

from tests import synth
from tests.bottleneck_ref import bottleneck_stages_f64

MEAN = torch.tensor([102.9801, 115.9465, 122.7717])[None, :, None, None]
R1 = 7 | 16          # fuse_tail bits 3-4 = 2: stage 3 on the one-wave-per-SIMD form (fused_tail_r1_kernel; also the default)
W16 = 7 | 8          # ... = 1: stage 3 on the 16-column form (fused_tail16_kernel), stage 2 on the 32-column form
FUSED_TAG = 19       # profile slot of the fused tail's launches (bottleneck_fused.hip)


def backbone(name, seed, cuda=True):
    from stemseg_amd.modeling.backbone import ResNetFPN
    bb = ResNetFPN(name).eval()
    sd = synth.synth_state_dict([(k, v.shape) for k, v in bb.state_dict().items()], seed, prefix="backbone.")
    bb.load_state_dict({k: torch.from_numpy(np.asarray(v)).reshape(bb.state_dict()[k].shape) for k, v in sd.items()})
    return (bb.cuda() if cuda else bb), sd


def run(hip, bb, x, fuse, precision="f16x3"):
    """One encoder pass -> (the four FPN maps, fused-tail launches of the pass)."""
    bb.fuse_tail, bb.precision = fuse, precision
    T, _, H, W = x.shape
    outs = [torch.full((256, T, H // s, W // s), float("nan"), device="cuda") for s in (4, 8, 16, 32)]
    hip.profile_enable(True)
    hip.profile_read()
    bb.run_backbone_into(x, [hip.dense_volume(o) for o in outs])
    prof = hip.profile_read()
    hip.profile_enable(False)
    return outs, (prof.get(FUSED_TAG, (0, 0, 0))[2])


def frames(T, H, W, seed, scale=1.0):
    return (torch.from_numpy(synth.synth_frames(T, H, W, seed=seed).astype(np.float32)).permute(0, 3, 1, 2) - MEAN) * scale


# ---- tiny networks: ONE stage of three blocks (two fused tails: block 0 -> 1 behind the projection shortcut, block 1 -> 2 behind the plain
# identity), one block in every other stage.  After a pass the workspace still holds, for that stage: B = block 1's output (the second tail's
# y), M1[stage] = block 2's conv1 output (the second tail's z, zero-haloed), Cst[stage] = the stage output.
TINY = {0: ("T-3111", (3, 1, 1, 1)), 1: ("T-1311", (1, 3, 1, 1)), 2: ("T-1131", (1, 1, 3, 1))}
SEED = 84
PLAN_FRAMES = 4096


def tiny_backbone(stage, stress=False, seed=SEED):
    """-> (ResNetFPN on the CPU with the three-block stage `stage` (0-2), its state dict as float32 numpy)."""
    from stemseg_amd.modeling import backbone as B
    name, blocks = TINY[stage]
    with pytest.MonkeyPatch.context() as mp:
        mp.setitem(B.STAGE_BLOCKS, name, blocks)
        bb = B.ResNetFPN(name).eval()
    sd = {k: np.asarray(synth.synth_param("backbone." + k, v.shape, seed)).reshape(v.shape).astype(np.float32) for k, v in bb.state_dict().items()}
    if stress:
        frozen_bn_like(sd, stage, seed)
    load(bb, sd)
    centre_last_bn1(bb, sd, stage, seed)
    bb.plan_frames = PLAN_FRAMES
    return bb, sd


def centre_last_bn1(bb, sd, stage, seed):
    """running_mean of block 2's bn1 := the mean of its conv1 output over a calibration clip (8 frames of 32 x 32), as training leaves it.  The
    synthetic 0.1-scale running_mean against all-positive inputs of a few hundred leaves 7-30 % of the conv1 channels below zero at every
    position (identically zero after the ReLU: nothing to measure); centred, a channel is dead only where all of a map's positions are."""
    import torch.nn.functional as F
    key = "body.layer%d.2." % (stage + 1)
    b = reference(bb, frames(8, 32, 32, seed + 7), stage)["B"].permute(1, 0, 2, 3)
    c = F.conv2d(b, torch.from_numpy(sd[key + "conv1.weight"]).double())
    sd[key + "bn1.running_mean"] = c.mean((0, 2, 3)).float().numpy()
    load(bb, sd)


def scale_network(sd, g):
    """The network whose every activation is g times the given one's on g times the frames: every FrozenBN shift (bias, running_mean) and
    FPN bias times g -- a ReLU network is positively homogeneous in (input, biases).  The dead channels stay the same channels."""
    out = dict(sd)
    for k in sd:
        if k.endswith(".running_mean") or k.endswith(".bias"):
            out[k] = (sd[k] * np.float32(g)).astype(np.float32)
    return out


def load(bb, sd):
    bb.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})


def frozen_bn_like(sd, stage, seed):
    """Statistics like a trained checkpoint's on the four FrozenBNs a stage's two fused tails fold in (bn3 of blocks 0-1: conv3; bn1 of blocks
    1-2: conv1) -- the recipe of test_split_modes_encoder_with_checkpoint_like_frozen_bn_statistics: running_var log-uniform over 1e-6 ... 1e2
    with the conv rows (and running_mean) scaled by sqrt(var), gamma log-uniform over 1e-4 ... 0.5 (bn3) / 3 (bn1): folded, per-output-channel
    weight scales over 4 orders of magnitude inside one layer.  bn1's beta is scaled by its gamma as well: relu(gamma * xhat + beta) with a
    negative beta of the synthetic 0.1 scale is identically zero for every gamma below ~0.02 -- a quarter of the channels would be dead and
    could not be measured; with beta * gamma a channel is its unit-gamma self times gamma, which is the per-channel range under test."""
    rs = np.random.RandomState(seed + 1000 * stage)
    layer = "body.layer%d." % (stage + 1)
    for blk, bn in ((0, "bn3"), (1, "bn3"), (1, "bn1"), (2, "bn1")):
        p = layer + "%d." % blk
        conv = p + bn.replace("bn", "conv") + ".weight"
        var = (10.0 ** rs.uniform(-6, 2, size=sd[p + bn + ".running_var"].shape)).astype(np.float32)
        gamma = (10.0 ** rs.uniform(-4, np.log10(0.5 if bn == "bn3" else 3.0), size=var.shape)).astype(np.float32)
        sd[p + bn + ".running_var"] = var
        sd[conv] = sd[conv] * np.sqrt(var)[:, None, None, None]
        sd[p + bn + ".running_mean"] = (sd[p + bn + ".running_mean"] * np.sqrt(var)).astype(np.float32)
        sd[p + bn + ".weight"] = gamma
        if bn == "bn1":
            sd[p + bn + ".bias"] = (sd[p + bn + ".bias"] * gamma).astype(np.float32)


def reference(bb, x, stage, folded=None):
    """fp64 reference of the three buffers as the workspace holds them (channel-major): dict(B=[C,T,h,w], M1=[mid,T,h,w], Cst=[C,T,h,w])."""
    r = bottleneck_stages_f64(bb, x, folded)
    first = stage                      # (one block per earlier stage)
    cm = lambda t: t.permute(1, 0, 2, 3).contiguous()
    return dict(B=cm(r["block_out"][first + 1]), M1=cm(r["conv1_out"][first + 2]), Cst=cm(r["block_out"][first + 2]), stage_in=cm(r["block_out"][first - 1] if first else r["stem"]))


def channel_scales(ref):
    """max |ref| per channel of a [C, ...] buffer."""
    return ref.reshape(ref.shape[0], -1).abs().amax(1)


def dead_share(ref):
    """share of a buffer's channels whose fp64 reference is identically zero (after the ReLU): they have no scale to measure against."""
    return float((channel_scales(ref) == 0).double().mean())


# ---- overflow through the tail: one output channel of block 1's bn3 raised until the block output B leaves the f16x3 range at SOME positions
F16X3_INF = 4 * 65520.0        # x / 4 rounds to fp16 infinity from here on (split_operand.h)
F16X3_MAX = 4 * 65504.0        # ... and is a finite fp16 number up to here; in between lies the rounding boundary


def overflow_network(stage, x, seed=SEED):
    """-> (bb, sd, channel, factor, over, inside, ref): block 1 of the three-block stage with bn3.weight[channel] multiplied by `factor`, chosen from
    the fp64 reference so that the channel's largest value in B is 8 x the f16x3 limit (2.1e6: far below fp32's 3.4e38); over / inside: bool
    [T,h,w] masks of the positions whose largest |B| over the channels is >= 4 x 65520 / <= 4 x 65504 (what lies between is left out)."""
    bb, sd = tiny_backbone(stage, seed=seed)
    key = "body.layer%d.1.bn3.weight" % (stage + 1)
    base = reference(bb, x, stage)["B"]
    # B[c] = relu(gamma[c] * u[c] + v[c]) and channel c of bn3 reaches B[c] alone: a pass with every gamma doubled gives gamma * u wherever both
    # values are past the ReLU; the channel raised is the one with the largest such term, the factor puts that value at 8 x the limit
    sd2 = dict(sd)
    sd2[key] = sd[key] * np.float32(2.0)
    load(bb, sd2)
    twice = reference(bb, x, stage)["B"]
    slope = torch.where((base > 0) & (twice > 0), twice - base, torch.zeros_like(base)).reshape(base.shape[0], -1)
    for channel in slope.amax(1).argsort(descending=True).tolist():        # the first channel that leaves positions of BOTH kinds (>= 5 % each)
        pos = int(slope[channel].argmax())
        b1, gu = float(base[channel].reshape(-1)[pos]), float(slope[channel, pos])
        assert b1 > 0 and gu > 0, (b1, gu)
        factor = float(np.float32(1.0 + (8 * F16X3_INF - b1) / gu))
        sd2[key] = sd[key].copy()
        sd2[key][channel] = sd[key][channel] * np.float32(factor)
        load(bb, sd2)
        ref = reference(bb, x, stage)
        col = ref["B"].abs().amax(0)
        over, inside = col >= F16X3_INF, col <= F16X3_MAX
        if min(int(over.sum()), int(inside.sum())) * 20 >= col.numel():
            return bb, sd2, channel, factor, over, inside, ref
    raise AssertionError("no channel of block 1 leaves positions over the f16x3 range and inside it")


# ---- what a pass leaves in the workspace
def tail_buffers(hip, bb, x, stage):
    """Copies of the three buffers after a pass of x [T,3,H,W] (on the device): dict(B=[C,T,h,w], Cst=[C,T,h,w], M1=[mid,T,h,w] (the interior),
    M1_halo = every other word of the M1[stage] slice as int32 bits: rows 0 and h + 1, column 0, columns w + 1 ... pitch - 1 of every plane,
    and the slack words behind the last plane)."""
    T, _, H, W = x.shape
    key = (T, H, W, x.device.index, bb.lane, None, int(bb.plan_frames))
    offs = (hip.C.c_int64 * 25)()
    hip.check(hip.lib().stemseg_hip_encoder_plan_offsets(hip.C.byref(bb._ws_desc[key]), offs))
    ws = bb._ws[key].view(torch.float32)
    h, w, C, mid = H >> (2 + stage), W >> (2 + stage), 256 << stage, 64 << stage
    V = T * h * w
    pitch = (w + 2 + 3) // 4 * 4                       # Padded2D (csrc/encoder.hip): [mid][T][h + 2][pitch] + 64 slack words, halo in h and w only
    g = dict(pitch=pitch, ts=(h + 2) * pitch, cs=T * (h + 2) * pitch, total=mid * T * (h + 2) * pitch + 64)
    m1 = ws[int(offs[8 + stage]):int(offs[8 + stage]) + g["total"]].clone()
    planes = m1[:mid * g["cs"]].view(mid, T, h + 2, g["pitch"])
    inside = torch.zeros(h + 2, g["pitch"], dtype=torch.bool, device=m1.device)
    inside[1:h + 1, 1:w + 1] = True
    halo = torch.cat([planes[:, :, ~inside].reshape(-1), m1[mid * g["cs"]:]]).view(torch.int32)
    assert halo.numel() == g["total"] - mid * V
    return dict(B=ws[int(offs[3]):int(offs[3]) + C * V].view(C, T, h, w).clone(), Cst=ws[int(offs[4 + stage]):int(offs[4 + stage]) + C * V].view(C, T, h, w).clone(),
                M1=planes[:, :, 1:h + 1, 1:w + 1].contiguous(), M1_halo=halo)
