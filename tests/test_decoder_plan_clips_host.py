"""The decoders' planning clip count (StemsegDecoderDesc.plan_clips) -- asked of the launch code itself, without a GPU.

``plan_ksplit`` (csrc/conv_igemm.h) splits a convolution over K until the PLANNED launch holds about 1.25 workgroups per CU (320 for the
eight-wave split-staged tiles).  The decoders plan on one clip and run the 4 clips of a step, so their small-map stages split 2 .. 16 ways
for nothing; ``plan_clips`` multiplies the planned workgroup count.  ``hip.conv3d_plan(..., plan_clips=)`` is the dry run of one stage as the
decoder launches it (zero temporal halo, GroupNorm sums, one clip's share of the decoder's split-K scratch), so the numbers below are the
library's own records:

  * the seven stages of a decoder at the flagship shape (T = 8, 480 x 864, f16x3) make 16 / 32 / 64 / 128 / 240 / 432 workgroups per clip and
    split 16 / 8 / 4 / 2 / 1 / 1 ways planned on one clip, 4 / 2 / 1 / 1 / 1 / 1 ways planned on four -- the arithmetic restated here;
  * nothing but the factor moves: the tile, the grid's x and y, the 16-byte forms;
  * plan_clips 0 and 1 are the entry without the argument, record for record;
  * un-split launches leave their GroupNorm sums per tile: at every level of the three workloads' shapes the statistics stay in the launch
    (no record falls back to the separate pass, no launch is refused for a full slot table);
  * the descriptor: the older size is accepted and sizes the same workspace, plan_clips moves no byte of it, a bad value is refused."""
import ctypes

import pytest

from tests import conv_cases as cc

CIN, INTER, GROUPS = 256, (256, 256, 128, 128), 32
WORKLOADS = {"davis": (120, 216), "ytvis": (96, 160), "kitti": (152, 488)}          # H4 x W4 of bench.py's three workloads (T = 8)
WG_TARGET = 320                                                                      # plan_ksplit: eight-wave split-staged tiles


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.lib()
    return h


def stages(H4, W4, T=8, cin=CIN, inter=INTER):
    """(name, Cin, Cout, T, H, W, one clip's split-K scratch in floats) of the seven 3x3x3 stages, as csrc/decoder.hip lays them out for T = 8."""
    c32, c16, c8, c4 = inter
    h, w = [H4 >> (3 - i) for i in range(4)], [W4 >> (3 - i) for i in range(4)]
    S = [k * c * T * h[i] * w[i] for i, (k, c) in enumerate(zip((16, 4, 4, 2), inter))]
    return [("32x conv 1", cin, c32, T, h[0], w[0], S[0]), ("32x conv 2", c32, c32, T // 2, h[0], w[0], S[0]), ("32x conv 3", c32, c32, T // 4, h[0], w[0], S[0]),
            ("16x conv 1", cin, c16, T, h[1], w[1], S[1]), ("16x conv 2", c16, c16, T // 2, h[1], w[1], S[1]),
            ("8x conv 1", cin, c8, T, h[2], w[2], S[2]), ("4x conv 1", cin, c4, T, h[3], w[3], S[3])]


def plan(hip, st, plan_clips, precision="f16x3", groups=GROUPS, **kw):
    _, ci, co, t, h, w, scratch = st
    case = cc.C("stage", "k3", ci, co, t, h, w, "?", scratch=scratch)
    return hip.conv3d_plan(cc.volume(hip, cc.in_geom(case), cc.BASE), cc.volume(hip, cc.out_geom(case), 2 * cc.BASE), 3, 0, (4 * cc.BASE, scratch),
                           dict(precision=precision), gn_groups=groups, zero_t_halo=True, plan_clips=plan_clips, **kw)


def expected_ksplit(wgs, nchunks, slabs, plan_clips):
    k = 1
    while 2 * k <= 16 and 2 * k <= nchunks and wgs * max(plan_clips, 1) * 2 * k <= WG_TARGET and 2 * k <= slabs:
        k *= 2
    return k


def test_symbol_exported_declared_and_bound(hip):
    import os
    raw = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stemseg_hip.h")).read()
    assert hasattr(raw, "stemseg_hip_conv3d_plan_clips") and "stemseg_hip_conv3d_plan_clips" in hip.SIGNATURES and "stemseg_hip_conv3d_plan_clips(" in header
    body = header[header.index("typedef struct StemsegDecoderDesc {"):header.index("} StemsegDecoderDesc;")]
    assert body.rstrip().endswith("int32_t reserved;            /* 0 */") and "int32_t plan_clips;" in body
    assert [n for n, _ in hip.DecoderDesc._fields_][-3:] == ["out_clip_stride", "plan_clips", "reserved"]
    assert hip.DecoderDesc.plan_clips.offset + 8 == ctypes.sizeof(hip.DecoderDesc)


def test_flagship_stages_split_as_the_arithmetic_says(hip):
    """Workgroup counts 16 / 32 / 64 / 128 / 240 / 432 per clip at planning counts 1 and 4."""
    seen = {}
    for st in stages(*WORKLOADS["davis"]):
        by_pc = {}
        for pc in (1, 4):
            (r,) = plan(hip, st, pc)
            print("%-11s plan_clips %d  %s" % (st[0], pc, cc.describe(r)))
            wgs = r["grid"][0]
            slabs = st[6] // (st[2] * st[3] * st[4] * st[5])
            assert r["ksplit"] == r["grid"][2] == expected_ksplit(wgs, r["nchunks"], slabs, pc), (st[0], pc, r)
            assert (r["reduce"] is not None) == (r["ksplit"] > 1)
            assert r["gn"] == ("split-K reduce" if r["ksplit"] > 1 else "tile epilogue")
            by_pc[pc] = r
        a, b = by_pc[1], by_pc[4]
        same = [k for k in a if k not in ("ksplit", "chunks_per_split", "grid", "reduce", "gn", "vec_epi")]
        assert all(a[k] == b[k] for k in same) and a["grid"][:2] == b["grid"][:2], "plan_clips moved more than the split-K factor: %s" % st[0]
        seen.setdefault(a["grid"][0], set()).add((a["ksplit"], b["ksplit"]))
    assert seen == {16: {(16, 4)}, 32: {(8, 2)}, 64: {(4, 1)}, 128: {(2, 1)}, 240: {(1, 1)}, 432: {(1, 1)}}, seen


@pytest.mark.parametrize("precision", ["f16x3", "bf16x6", "f32"])
def test_plan_clips_0_and_1_are_the_plans_without_it(hip, precision):
    for H4, W4 in list(WORKLOADS.values()) + [(16, 24), (16, 72)]:
        for st in stages(H4, W4):
            _, ci, co, t, h, w, scratch = st
            case = cc.C("stage", "k3", ci, co, t, h, w, "?", scratch=scratch)
            vin, vout = cc.volume(hip, cc.in_geom(case), cc.BASE), cc.volume(hip, cc.out_geom(case), 2 * cc.BASE)
            e = hip._conv_epilogue(dict(precision=precision))
            rec, n = (hip.ConvPlanRecord * 4)(), ctypes.c_int32(0)
            hip.check(hip.lib().stemseg_hip_conv3d_plan(ctypes.byref(vin), ctypes.c_void_p(1 << 20), ctypes.byref(vout), 3, 3, 3, 0, ctypes.c_void_p(4 * cc.BASE),
                                                        scratch, ctypes.byref(e), hip.PLAN_GN | hip.PLAN_ZERO_T_HALO, GROUPS, rec, 4, ctypes.byref(n)))
            old = [bytes(r) for r in rec[:n.value]]
            for pc in (0, 1):
                new = plan(hip, st, pc, precision)
                assert len(new) == len(old)
                for o, d in zip(old, new):
                    o = hip.ConvPlanRecord.from_buffer_copy(o)
                    assert all(getattr(o, k) == d[k] for k in ("ksplit", "chunks_per_split", "nchunks", "rows", "tw", "nt", "mt", "ck", "row0", "row1", "vec_epi"))
                    assert tuple(o.grid) == d["grid"]


@pytest.mark.parametrize("workload", sorted(WORKLOADS))
@pytest.mark.parametrize("inter,groups", [(INTER, 32), ((128, 128, 64, 64), 16)])
def test_groupnorm_sums_stay_in_the_launch_at_every_level(hip, workload, inter, groups):
    """gn_cap: an un-split launch takes one slot per tile (tiles_x . tiles_y . T), a split one gn_cpg per 256 outputs of a channel; the decoder's table
    holds GN_SLOT_CAP = 32768 per group.  A full table is an argument error of the plan call, a launch too large for it a 'separate pass' record."""
    for pc in (0, 4):
        for st in stages(*WORKLOADS[workload], inter=inter):
            for r in plan(hip, st, pc, groups=groups):
                assert r["gn"] in ("tile epilogue", "split-K reduce"), (workload, st[0], pc, r["gn"])
                if r["ksplit"] == 1:
                    assert r["grid"][0] // -(-st[2] // r["mt"]) <= 32768          # tiles_x . tiles_y . T: the grid's x without its output-channel blocks


def _desc(hip, **kw):
    d = hip.DecoderDesc()
    d.struct_bytes = ctypes.sizeof(hip.DecoderDesc)
    d.in_channels = 32
    for i, c in enumerate((64, 64, 32, 32)):
        d.inter[i] = c
    d.T, d.H4, d.W4, d.gn_groups, d.gn_eps, d.n_out = 8, 16, 24, 8, 1e-5, 6
    d.pool[0], d.pool[1], d.pool[2] = 1, 1, 0
    d.t_scale[0], d.t_scale[1], d.t_scale[2] = 1, 2, 2
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_descriptor_older_size_and_workspace(hip):
    l = hip.lib()
    want = l.stemseg_hip_decoder_workspace_bytes(ctypes.byref(_desc(hip)))
    assert want > 0
    for pc in (1, 4, 64):
        for n in (0, 4):
            assert l.stemseg_hip_decoder_workspace_bytes(ctypes.byref(_desc(hip, plan_clips=pc, n_clips=n))) == \
                l.stemseg_hip_decoder_workspace_bytes(ctypes.byref(_desc(hip, n_clips=n))), "plan_clips moved the workspace"
    # the descriptor as it was before the field: accepted, and whatever lies behind it is not read as a planning count
    assert l.stemseg_hip_decoder_workspace_bytes(ctypes.byref(_desc(hip, struct_bytes=hip.DecoderDesc.plan_clips.offset, plan_clips=-7))) == want
    for bad in (dict(plan_clips=-1), dict(plan_clips=4097), dict(struct_bytes=hip.DecoderDesc.plan_clips.offset + 4)):
        assert l.stemseg_hip_decoder_workspace_bytes(ctypes.byref(_desc(hip, **bad))) == 0, bad
        assert (b"plan_clips" in l.stemseg_hip_last_error()) or (b"ABI skew" in l.stemseg_hip_last_error())


def test_model_default_reaches_all_three_decoders():
    from stemseg_amd import config
    from stemseg_amd.modeling.inference_model import InferenceModel
    config.load_preset("ytvis")
    try:
        config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
        model = InferenceModel()
        m = model._model
        heads = [h for h in (m.embedding_head, m.seediness_head, m.semseg_head) if h is not None]
        assert m.semseg_head is not None and model.plan_clips == 4 and all(h.plan_clips == 4 for h in heads)
        assert all(h._desc(8, 16, 24, 2, [0]).plan_clips == 4 for h in heads)
        model.plan_clips = 1
        assert all(h.plan_clips == 1 and h._desc(8, 16, 24, 2, [0]).plan_clips == 1 for h in heads)
    finally:
        config.load_preset("defaults")
