"""CPU tests of the product's host-side logic against the reference-generated goldens, plus the C-ABI export
check.  No compute call goes through the GPU here; device ops of the chainer are replaced by the oracle twin."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import decoder as odec
from oracle import encoder as oenc
from tests import synth
from tests.conftest import ROOT
from tests.oracle_ops import OracleChainerOps


# ------------------------------------------------------------------------------------------------ C-ABI
def _header_functions():
    txt = open(os.path.join(ROOT, "include", "stemseg_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(stemseg_hip_\w+)\s*\(", txt)))


def test_cabi_library_exports_every_declared_symbol():
    from stemseg_amd import hip
    names = _header_functions()
    assert len(names) >= 20
    assert sorted(hip.SIGNATURES) == names, "ctypes binding and include/stemseg_hip.h disagree"
    assert os.path.exists(hip.LIB_PATH), "libstemseg_hip.so not built (python stem-seg_amd/build.py)"
    lib = ctypes.CDLL(hip.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n
    assert hip.lib().stemseg_hip_version() == hip.ABI_VERSION


def test_product_library_contains_no_packed_fp32_valu_instructions():
    """the round-3/4 lane differences were reproduced in round 5 with a kernel whose FMAs are v_pk_fma_f32 sharing a CU
    with the f16x3 128 x 128 1x1 convolution (wrong low halves in lanes 48..63; the same kernel with scalar v_fma_f32: clean).  The product
    library is therefore built without the packed-fp32 VALU instruction class; build.py writes what the device assembly holds."""
    import json
    from stemseg_amd import hip
    rep_path = os.path.splitext(hip.LIB_PATH)[0] + ".isa.json"
    if not os.path.exists(rep_path):
        pytest.skip("no ISA report next to the library (built elsewhere): python stem-seg_amd/build.py --force writes it")
    rep = json.load(open(rep_path))
    assert rep["no_packed_fp32_flag"] and rep["arch"] == "gfx950"
    assert all(v["assembly_found"] for v in rep["sources"].values())
    assert sum(v["kernels"] for v in rep["sources"].values()) >= 80
    assert sum(v["packed_fp32_valu_instructions"] for v in rep["sources"].values()) == 0, rep
    assert os.path.getmtime(rep_path) >= os.path.getmtime(hip.LIB_PATH) - 5.0, "stale ISA report"


def test_cabi_struct_sizes_and_argument_errors():
    from stemseg_amd import hip
    l = hip.lib()
    d = hip.DecoderDesc()
    d.struct_bytes = ctypes.sizeof(hip.DecoderDesc) - 4              # ABI skew must be rejected, not mis-read
    assert l.stemseg_hip_decoder_workspace_bytes(ctypes.byref(d)) == 0
    assert b"descriptor size mismatch" in l.stemseg_hip_last_error()
    d.struct_bytes = ctypes.sizeof(hip.DecoderDesc)
    d.in_channels, d.T, d.H4, d.W4, d.gn_groups, d.n_out = 256, 8, 24, 32, 32, 7
    for i, c in enumerate((256, 256, 128, 128)):
        d.inter[i] = c
    for i, (p, s) in enumerate(zip((1, 1, 0), (1, 2, 2))):
        d.pool[i], d.t_scale[i] = p, s
    nbytes = l.stemseg_hip_decoder_workspace_bytes(ctypes.byref(d))
    assert nbytes > 4 * 256 * 10 * 26 * 36
    # the clip batch (ABI 8): n_clips clip plans a fixed stride apart + ONE split-K area for all of them behind -- linear in n_clips, and the
    # strides the caller announces are checked
    d.input_layout = 2
    n1 = l.stemseg_hip_decoder_workspace_bytes(ctypes.byref(d))
    d.n_clips = 4
    for i, (h, w) in enumerate(((3, 4), (6, 8), (12, 16), (24, 32))):
        d.feat_clip_stride[i] = (hip.padded_geometry(256, 8, h, w)["total"] + 63) // 64 * 64
    n4 = l.stemseg_hip_decoder_workspace_bytes(ctypes.byref(d))
    d.n_clips = 2
    n2 = l.stemseg_hip_decoder_workspace_bytes(ctypes.byref(d))
    assert 0 < n1 < n2 < n4 and n4 - n2 == 2 * (n2 - n1) and (n2 - n1) % 1024 == 0
    d.feat_clip_stride[3] = 16                                        # clips would overlap
    assert l.stemseg_hip_decoder_workspace_bytes(ctypes.byref(d)) == 0 and b"feat_clip_stride" in l.stemseg_hip_last_error()
    d.feat_clip_stride[3] = (hip.padded_geometry(256, 8, 24, 32)["total"] + 63) // 64 * 64
    d.out_clip_stride = 8                                             # smaller than one clip's output
    assert l.stemseg_hip_decoder_workspace_bytes(ctypes.byref(d)) == 0 and b"out_clip_stride" in l.stemseg_hip_last_error()
    d.out_clip_stride, d.n_clips, d.input_layout = 0, 0, 0
    assert l.stemseg_hip_decoder_workspace_bytes(ctypes.byref(d)) == nbytes
    d.t_scale[0] = 2                                                  # inconsistent topology
    assert l.stemseg_hip_decoder_workspace_bytes(ctypes.byref(d)) == 0
    g = hip.padded_geometry(256, 8, 120, 216)
    assert g["pitch"] == 220 and g["ts"] == 122 * 220 and g["cs"] == 10 * 122 * 220 and g["interior"] == 122 * 220 + 220 + 1
    assert ctypes.sizeof(hip.ClusterMeta) == 4 + 4 + 8 + 8 + 64 * 8 * 4 * 2 + 64 * 4
    assert l.stemseg_hip_cluster_workspace_bytes(1000) >= 4000
    e = hip.EncoderDesc()
    e.struct_bytes = ctypes.sizeof(hip.EncoderDesc)
    for i, n in enumerate((3, 4, 23, 3)):
        e.blocks[i] = n
    e.T, e.H, e.W, e.out_channels, e.precision, e.n_clips = 32, 480, 864, 256, 0, 4
    assert l.stemseg_hip_encoder_workspace_bytes(ctypes.byref(e)) > 32 * 64 * 240 * 432 * 4
    e.n_clips = 3                                                     # 32 frames are not 3 whole clips
    assert l.stemseg_hip_encoder_workspace_bytes(ctypes.byref(e)) == 0 and b"whole clips" in l.stemseg_hip_last_error()
    e.n_clips, e.W = 4, 850                                           # frame size must be padded to multiples of 32
    assert l.stemseg_hip_encoder_workspace_bytes(ctypes.byref(e)) == 0
    # packed weight sizes per precision (pure host arithmetic): chunks x k-groups x planes x [half][Cout] 16-B pieces (+ the f16x3 per-output-channel scale vector)
    split3 = 64 * 7 * 3 * 2 * 128 * 16
    split2 = split3 // 3 * 2
    assert l.stemseg_hip_packed_weight_bytes_prec(128, 256, 27, hip.PRECISIONS["bf16x6"]) == split3
    assert l.stemseg_hip_packed_weight_bytes_prec(128, 256, 27, 1) == 0                       # (code 1, the retired two-term bf16 split)
    assert l.stemseg_hip_packed_weight_bytes_prec(128, 256, 27, hip.PRECISIONS["f16x3"]) == split2 + 8 * 128      # (two staged weight planes: hi, lo)
    assert l.stemseg_hip_packed_weight_bytes_prec(256, 1024, 1, hip.PRECISIONS["f16x3"]) == 32 * 2 * 2 * 2 * 256 * 16 + 8 * 256
    # 1x3x3: bf16x6 packs 8-channel chunks of five k-groups (two taps x 8 channels, the ninth tap beside a zero one), f16x3 16-channel chunks of
    # nine (one tap x 16 channels: no padded tap slot)
    assert l.stemseg_hip_packed_weight_bytes_prec(256, 256, 9, hip.PRECISIONS["bf16x6"]) == (256 // 8) * 3 * 5 * 2 * 256 * 16
    assert l.stemseg_hip_packed_weight_bytes_prec(256, 256, 9, hip.PRECISIONS["f16x3"]) == (256 // 16) * 2 * 9 * 2 * 256 * 16 + 8 * 256
    assert l.stemseg_hip_packed_weight_bytes_prec(128, 256, 27, hip.PRECISIONS["f32"]) == 0 and l.stemseg_hip_packed_weight_bytes_prec(128, 256, 27, 7) == 0
    assert sorted(hip.PRECISIONS) == sorted(hip.PRECISION_INFO) and hip.PRECISION_INFO["f16x3"]["operand_significand_bits"] == 22
    # encoder plan offsets (debugging aid): distinct offsets, the first buffer at 0, the last value = the workspace size in floats
    e.n_clips, e.W = 4, 864
    offs = (ctypes.c_int64 * 25)()
    assert l.stemseg_hip_encoder_plan_offsets(ctypes.byref(e), offs) == 0
    present = [o for o in offs if o >= 0]
    assert len(set(present)) == len(present) == 21 and min(present) == 0 and offs[24] == max(present) and \
        offs[24] * 4 == l.stemseg_hip_encoder_workspace_bytes(ctypes.byref(e))            # (no FO buffers: the clips of this pass do not overlap)
    # planning frames: the split-K scratch grows with T / plan_frames (a pass of more frames keeps the plan's K-partition), never shrinks
    base = l.stemseg_hip_encoder_workspace_bytes(ctypes.byref(e))
    e.plan_frames = 32
    assert l.stemseg_hip_encoder_workspace_bytes(ctypes.byref(e)) == base
    e.plan_frames = 8
    assert l.stemseg_hip_encoder_workspace_bytes(ctypes.byref(e)) == base + 3 * (32 << 20) * 4
    e.plan_frames = -1
    assert l.stemseg_hip_encoder_workspace_bytes(ctypes.byref(e)) == 0 and b"plan_frames" in l.stemseg_hip_last_error()
    e.plan_frames = 0
    # mask materialisation: the crop must fit the up-sampled mask (davis.py:91-96 raises the same way)
    rc = l.stemseg_hip_resample_instance_masks(ctypes.c_void_p(16), 24, 32, ctypes.c_float(4.0), 97, 128, 70, 100, ctypes.c_void_p(16), None)
    assert rc != 0 and b"should be <= padded dims" in l.stemseg_hip_last_error()


# ------------------------------------------------------------------------------------------------ small host functions
def test_windowing_table(golden):
    from stemseg_amd.inference.main import get_subsequence_frames
    g = golden("misc")
    for key in g["win__keys"]:
        key = str(key)
        _, ds, seq_len, T, ov = key.split("_")
        clips, padded = get_subsequence_frames(int(seq_len), int(T), ds, int(ov))
        assert np.array_equal(np.array(clips, np.int64), g[key]), key
        assert (padded if padded is not None else []) == g[key + "__padded"].astype(bool).tolist(), key


def test_embedding_utils(golden):
    from stemseg_amd.modeling import embedding_utils as eu
    g = golden("misc")
    for m, nd, nf in zip(g["modes"], g["modes__nb_dims"], g["modes__nb_free"]):
        m = str(m)
        assert eu.get_nb_embedding_dims(m) == nd and eu.get_nb_free_dims(m) == nf
        z = torch.zeros(1, int(nd), 3, 4, 6)
        assert np.array_equal(eu.add_spatiotemporal_offset(z, torch.tensor(1.0), m)[0].numpy(), g["offset_" + m])
    with pytest.raises(ValueError):
        eu.get_nb_embedding_dims("xyz")
    assert eu.get_nb_free_dims("bogus") == 0
    for key in [k for k in g.files if k.startswith("grid_") and k.endswith("_x")]:
        _, H, W, T, _ = key.split("_")
        t, y, x = eu.creat_spatiotemporal_grid(int(H), int(W), int(T), 1.0)
        assert t.shape == (int(T), int(H), int(W))
        assert np.array_equal(t[:, 0, 0].numpy(), g[key[:-2] + "_t"])
        assert np.array_equal(y[0, :, 0].numpy(), g[key[:-2] + "_y"])
        assert np.array_equal(x[0, 0, :].numpy(), g[key])


def test_resize_params_and_preprocessing(golden):
    from stemseg_amd import config
    from stemseg_amd.modeling import inference_model as im
    g = golden("misc")
    for w, h, mn, mx, nw, nh in g["resize_params"].tolist():
        got = im.compute_resize_params_2((w, h), mn, mx)
        assert (got[0], got[1]) == (nw, nh)
    assert im.pad_to_multiple_of_32(480, 854) == (480, 864) and im.pad_to_multiple_of_32(701, 1248) == (704, 1248)
    old = (config.cfg.INPUT.MIN_DIM, config.cfg.INPUT.MAX_DIM)
    try:
        config.cfg.INPUT.MIN_DIM, config.cfg.INPUT.MAX_DIM = 64, 96
        from oracle import pipeline as opipe          # (the product's preprocess_frames is a HIP launch: tests/test_gpu_parity.py)
        out, _ = opipe.preprocess_frames(g["preproc__in"][None], 64, 96)
        assert out.shape[1:] == g["preproc__out"].shape
        assert np.abs(out[0].numpy() - g["preproc__out"]).max() <= 1e-4
    finally:
        config.cfg.INPUT.MIN_DIM, config.cfg.INPUT.MAX_DIM = old


def test_registry_contract():
    from stemseg_amd.utils import GlobalRegistry
    from stemseg_amd.modeling.embedding_decoder import EMBEDDING_HEAD_REGISTRY, SqueezingExpandDecoder
    from stemseg_amd.modeling.seediness_decoder import SEEDINESS_HEAD_REGISTRY
    from stemseg_amd.modeling.backbone import BACKBONE_REGISTRY
    assert GlobalRegistry.get("EmbeddingHead") is EMBEDDING_HEAD_REGISTRY
    assert EMBEDDING_HEAD_REGISTRY["squeeze_expand_decoder"] is SqueezingExpandDecoder
    assert SEEDINESS_HEAD_REGISTRY["squeeze_expand_decoder"] is not SqueezingExpandDecoder
    assert "R-101-FPN" in BACKBONE_REGISTRY and "R-50-FPN" in BACKBONE_REGISTRY
    with pytest.raises(KeyError):
        EMBEDDING_HEAD_REGISTRY["nope"]
    with pytest.raises(AssertionError):
        EMBEDDING_HEAD_REGISTRY.add("squeeze_expand_decoder", object)
    r = GlobalRegistry.get("UnitTestRegistry")

    @r.add("thing")
    def thing():
        return 1
    assert r["thing"] is thing


# ------------------------------------------------------------------------------------------------ state-dict contracts
def _gn(c):
    return torch.nn.GroupNorm(32, c)


def test_decoder_state_dict_keys_match_reference_layout():
    from stemseg_amd.modeling.embedding_decoder import SqueezingExpandDecoder as Emb
    from stemseg_amd.modeling.seediness_decoder import SqueezingExpandDecoder as Seed
    for T in (4, 8, 16):
        e = Emb(256, [256, 256, 128, 128], 4, True, True, "xyff", NormType=_gn, num_frames=T)
        want = dict(odec.decoder_param_shapes("", mode="xyff", embedding_size=4, seediness_output=True))
        got = {k: tuple(v.shape) for k, v in e.state_dict().items()}
        assert got == {k: tuple(v) for k, v in want.items()}
        assert (e.embedding_size, e.variance_channels, e.seediness_channels) == (4, 2, 1)
    e = Emb(256, [256, 256, 128, 128], 3, True, False, "xyt", NormType=_gn, num_frames=8)
    assert (e.variance_channels, e.seediness_channels) == (3, 0) and "conv_seediness.weight" not in e.state_dict()
    s = Seed(256, [256, 256, 128, 128], NormType=_gn, num_frames=8)
    want = dict(odec.decoder_param_shapes("", kind="seediness"))
    assert {k: tuple(v.shape) for k, v in s.state_dict().items()} == {k: tuple(v) for k, v in want.items()}
    with pytest.raises(NotImplementedError):
        Emb(256, [256, 256, 128, 128], 4, True, True, "xyff", NormType=_gn, num_frames=7)


def test_decoder_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from stemseg_amd.modeling.seediness_decoder import SqueezingExpandDecoder as Seed
    s = Seed(256, [256, 256, 128, 128], NormType=_gn, num_frames=8)
    feats = [torch.zeros(1, 256, 8, 3 * k, 3 * k) for k in (1, 2, 4, 8)]
    with pytest.raises(RuntimeError, match="no MI355X visible"):
        s(feats)


def folded_forward_torch(f, blocks, x):
    """Test-only torch evaluation of ResNetFPN.folded_state() (conv + folded bias; no BN anywhere)."""
    import torch.nn.functional as F
    x = F.max_pool2d(F.relu(F.conv2d(x, *f["stem"], stride=2, padding=3)), 3, 2, 1)
    feats, i = [], 0
    for li, n in enumerate(blocks, 1):
        for bi in range(n):
            stride = 2 if (bi == 0 and li > 1) else 1
            out = F.relu(F.conv2d(x, *f["b%d.conv1" % i], stride=stride))
            out = F.relu(F.conv2d(out, *f["b%d.conv2" % i], padding=1))
            out = F.conv2d(out, *f["b%d.conv3" % i])
            idt = F.conv2d(x, *f["b%d.down" % i], stride=stride) if ("b%d.down" % i) in f else x
            x = F.relu(out + idt)
            i += 1
        feats.append(x)
    last = F.conv2d(feats[3], *f["fpn_inner4"])
    res = {32: F.conv2d(last, *f["fpn_layer4"], padding=1)}
    for k, s in ((3, 16), (2, 8), (1, 4)):
        last = F.conv2d(feats[k - 1], *f["fpn_inner%d" % k]) + F.interpolate(last, scale_factor=2, mode="bilinear", align_corners=False)
        res[s] = F.conv2d(last, *f["fpn_layer%d" % k], padding=1)
    return res


@pytest.mark.parametrize("btype", ["R-50-FPN", "R-101-FPN"])
def test_backbone_state_dict_and_bn_folding_vs_golden(golden, btype):
    """Reference key names load, and the FrozenBN-folded weights the HIP encoder consumes reproduce the reference
    encoder's outputs (evaluated here with plain torch convs -- the product's forward is HIP-only)."""
    from stemseg_amd.modeling.backbone import ResNetFPN
    g = golden("encoder")
    tag = btype.replace("-", "")
    H, W, seed, stride = g[tag + "__meta"].tolist()
    bb = ResNetFPN(btype).eval()
    want = dict(oenc.backbone_param_shapes(btype, prefix=""))
    assert {k: tuple(v.shape) for k, v in bb.state_dict().items()} == {k: tuple(v) for k, v in want.items()}
    sd = {k: torch.from_numpy(np.asarray(synth.synth_param("backbone." + k, v.shape, seed))).reshape(v.shape)
          for k, v in bb.state_dict().items()}
    bb.load_state_dict(sd)
    x = synth.synth_frames(2, H, W, seed=seed).astype(np.float32)
    x = torch.from_numpy(x).permute(0, 3, 1, 2) - torch.tensor([102.9801, 115.9465, 122.7717])[None, :, None, None]
    feats = folded_forward_torch(bb.folded_state(), bb.stage_blocks, x)
    for s in (4, 8, 16, 32):
        ref = g["%s_s%d" % (tag, s)]
        got = feats[s].contiguous().numpy().reshape(-1)[::stride]
        assert np.abs(got - ref).max() <= 2e-5 * max(1.0, float(np.abs(ref).max())), (btype, s)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no MI355X visible"):
            bb(x)


# ------------------------------------------------------------------------------------------------ chainer host logic
def _make_chainer(resize=1.0):
    from stemseg_amd.inference.clusterers import SequentialClustering
    from stemseg_amd.inference.online_chainer import OnlineChainer
    return OnlineChainer(SequentialClustering(0.5, 0.3, 0.8, 2, [0.3, 0.3], "cpu"), resize, ops=OracleChainerOps())


@pytest.mark.parametrize("tag", ["seq20_ov4", "seq14_ov6", "seq8_single"])
def test_chainer_bookkeeping_vs_golden(golden, tag):
    g = golden("chainer")
    emb, bw, sd, fg = g[tag + "__emb"], g[tag + "__bw"], g[tag + "__sd"], g[tag + "__fg"]
    clips = g[tag + "__subseqs"].tolist()
    dicts = [dict(frames=list(fr), embeddings=torch.from_numpy(emb[:, fr].copy()), bandwidths=torch.from_numpy(bw[:, fr].copy()),
                  seediness=torch.from_numpy(sd[:, fr].copy())) for fr in clips]
    (track, counts, life), mask_idxes, clip_labels, _, meta = _make_chainer().process(torch.from_numpy(fg), dicts)
    for t, l in enumerate(track):
        assert l.dtype == torch.int64
        assert np.array_equal(l.numpy(), g["%s_track_%02d" % (tag, t)]), (tag, t)
        ys, xs = np.nonzero(fg[t])
        assert np.array_equal(mask_idxes[t][0].numpy(), ys) and np.array_equal(mask_idxes[t][1].numpy(), xs)
    assert sorted(counts.items()) == [tuple(r) for r in g[tag + "__pt_counts"].tolist()]
    assert sorted(life.items()) == [tuple(r) for r in g[tag + "__lifetimes"].tolist()]
    for i in range(len(clips)):
        assert np.array_equal(torch.cat(clip_labels[i]).numpy(), g["%s_clip%d_labels" % (tag, i)]), (tag, i)
        assert meta[i]["instance_labels"] == g["%s_clip%d_instance_labels" % (tag, i)].tolist(), (tag, i)
    assert all(d["embeddings"] is None for d in dicts)       # reference clears the tensors (online_chainer.py:239)


def test_chainer_track_ids_beyond_500_vs_golden(golden):
    """48 clips with births and deaths in every clip: the reference's track ids reach 527 (online_chainer.py:43-49 hands out
    highest id + 1).  The association only ever looks at the ids present on the overlap frames (:304-308)."""
    fg, dicts, exp = synth.long_sequence_case(golden("chainer_long"), torch.from_numpy)
    top = synth.check_long_sequence(_make_chainer().process(torch.from_numpy(fg), dicts), exp)
    assert top > 500


def test_chainer_exact_cost_ties_follow_the_reference_id_order(golden):
    """tests/golden/chainer_ties.npz: a 12-clip sequence in which new instances have zero IoU with several unmatched old tracks --
    rectangular cost matrices full of exact 1.0 ties -- through the reference's chainer.  Which old track wins depends on the order
    the reference enumerates the ids in, list(set(unique().tolist()) - {-1}) (online_chainer.py:308-309): CPython set order, not
    ascending.  (tools/make_goldens.py asserts that the ascending order gives a different result on this sequence.)"""
    from stemseg_amd.inference import online_chainer as oc
    g = golden("chainer_ties")
    fg, dicts, exp = synth.tie_sequence_case(g, torch.from_numpy)
    synth.check_long_sequence(_make_chainer().process(torch.from_numpy(fg), dicts), exp)
    # the enumeration order itself
    assert oc.reference_id_order([2, 9], True) == list(set([-1, 2, 9]) - {-1}) and oc.reference_id_order([9, 2], False) == list(set([2, 9]))
    assert oc.reference_id_order([], True) == [] and sorted(oc.reference_id_order(range(1, 60), True)) == list(range(1, 60))
    # direct associate_clusters cases (ids up to 400 that collide in the set's hash table, with and without the outlier id)
    ch = _make_chainer()
    n_order_sensitive = 0
    for case in range(int(g["n_assoc"])):
        l1, l2 = g["assoc%02d_l1" % case].astype(np.int64), g["assoc%02d_l2" % case].astype(np.int64)
        got = ch.associate_clusters(torch.from_numpy(l1), torch.from_numpy(l2))[0]
        want = [tuple(r) for r in g["assoc%02d_pairs" % case].tolist()]
        assert [tuple(p) for p in got] == want, case
        ids1, ids2 = sorted(set(l1[l1 > 0].tolist())), sorted(set(l2[l2 > 0].tolist()))
        inter, ca, cb = OracleChainerOps().overlap_counts(torch.from_numpy(l1), torch.from_numpy(l2), ids1, ids2)
        n_order_sensitive += sorted(oc.association_from_counts(inter, ca, cb, ids1, ids2)[0]) != sorted(want)
    assert n_order_sensitive >= 3, "the golden must contain cases that an ascending enumeration gets wrong"


def test_chainer_resize_path(golden):
    g = golden("chainer")
    e = torch.from_numpy(g["resize__in"])
    sub = {"embeddings": e, "seediness": e[:1].clone(), "bandwidths": e[:2].clone()}
    _make_chainer(4.0).resize_tensors(sub)
    assert np.abs(sub["embeddings"].numpy() - g["resize__emb"]).max() <= 1e-6
    assert sub["seediness"].shape == (1, 2, 20, 28) and sub["bandwidths"].shape == (2, 2, 20, 28)


def test_fg_mask_and_clip_assembly_semantics(golden):
    """dedup rule of inference_model.py:137-138 for short videos: the LAST occurrence of a repeated frame wins."""
    g = golden("model_davis")
    sub = g["seq5__subseqs"].tolist()[0]
    assert sub == [0, 0, 0, 0, 1, 2, 3, 4] and g["seq5_c0_frames"].tolist() == [0, 1, 2, 3, 4]
    assert g["seq5_c0_emb"].shape[1] == 5


def test_instances_to_keep_and_mask_lut_vs_golden(golden):
    """Track selection for the writers (davis.py:57-66): stable sort by lifetime, outliers dropped, max_tracks cut -- vs the
    reference's own selection; and the label -> plane-index table the scatter kernel consumes."""
    from stemseg_amd.inference.output_utils import MaskMaterializer, instances_to_keep
    g = golden("masks")
    for name in g["__names"].tolist():
        max_tracks = int(g[name + "__dims"][7])
        life = dict(zip(g[name + "__lifetime_keys"].tolist(), g[name + "__lifetime_vals"].tolist()))
        keep = instances_to_keep(life, -1, max_tracks)
        assert keep == g[name + "__keep"].tolist()
        lut = MaskMaterializer(-1)._lut(keep, "cpu").tolist()
        assert lut[0] == 0                                            # slot of the outlier label (-1 + 1)
        for n, k in enumerate(keep):
            assert lut[k + 1] == n + 1
        assert sum(1 for v in lut if v) == len(keep)
    assert instances_to_keep({3: 5, 1: 5, -1: 9, 2: 7}, -1, 2) == [2, 3]      # ties keep the dict's order; outlier dropped


def test_linear_tail_matrices_reproduce_the_step_by_step_tail():
    """SqueezeExpandTrunk._linear_tail (the decoders' default since round 6): between the last GroupNorm + ReLU of every branch and the heads'
    activations the reference applies only linear maps -- trilinear up-sampling, concatenation, the bias-free 1x1x1 convs conv_16 / conv_8 / conv_4
    and the 1x1x1 heads (embedding_decoder.py:64-80,112-143) -- and 1x1x1 convs commute with up-sampling.  The four per-level matrices must
    reproduce that tail: here in torch on the CPU, fp64 (exact algebra) and fp32 (round-off), with temporal scales (1, 2, 2) as at T = 8."""
    import torch
    import torch.nn.functional as F
    from stemseg_amd.modeling.seediness_decoder import SqueezingExpandDecoder as Seed
    from stemseg_amd.modeling.embedding_decoder import SqueezingExpandDecoder as Emb
    torch.manual_seed(3)
    for make in (lambda: Seed(256, [64, 48, 32, 24], num_frames=8), lambda: Emb(256, [64, 48, 32, 24], 5, True, True, "xytff", num_frames=8)):
        m = make().eval()
        for prm in m.parameters():
            with torch.no_grad():
                prm.normal_(0, 0.3)
        c32, c16, c8, c4 = m.inter_channels
        m.fold_linear_tail = False          # (the dense [n_out, c4] head matrix, as the reference's heads hold it)
        m.fold_conv4 = False
        wh = m._head_spec()[0].detach()
        n_out = wh.shape[0]
        for dt, tol in ((torch.float64, 1e-11), (torch.float32, 2e-4)):
            x32 = torch.randn(1, c32, 2, 3, 5, dtype=dt)
            y16 = torch.randn(1, c16, 2, 6, 10, dtype=dt)
            y8 = torch.randn(1, c8, 4, 12, 20, dtype=dt)
            y4 = torch.randn(1, c4, 8, 24, 40, dtype=dt)
            up = lambda t, ts: F.interpolate(t, scale_factor=(ts, 2, 2), mode="trilinear", align_corners=False)
            x = up(x32, 1)
            x = F.conv3d(torch.cat((x, y16), 1), m.conv_16.weight.detach().to(dt))
            x = up(x, 2)
            x = F.conv3d(torch.cat((x, y8), 1), m.conv_8.weight.detach().to(dt))
            x = up(x, 2)
            x = F.conv3d(torch.cat((x, y4), 1), m.conv_4.weight.detach().to(dt))
            ref = F.conv3d(x, wh.to(dt).reshape(n_out, c4, 1, 1, 1))
            m32, m16, m8, m4 = [q.to(dt) for q in m._linear_tail(wh.double() if dt == torch.float64 else wh)]
            if dt == torch.float64:         # (the matrices are handed over in fp32; the algebra is checked on their fp64 values)
                w4 = m.conv_4.weight.detach().reshape(c4, c8 + c4).double(); w8 = m.conv_8.weight.detach().reshape(c8, c16 + c8).double()
                w16 = m.conv_16.weight.detach().reshape(c16, c32 + c16).double()
                a = wh.double() @ w4[:, :c8]; b = a @ w8[:, :c16]
                m4, m8, m16, m32 = wh.double() @ w4[:, c8:], a @ w8[:, c16:], b @ w16[:, c32:], b @ w16[:, :c32]
            lin = lambda mat, t: F.conv3d(t, mat.reshape(mat.shape[0], mat.shape[1], 1, 1, 1))
            z = up(lin(m32, x32), 1) + lin(m16, y16)
            z = up(z, 2) + lin(m8, y8)
            z = up(z, 2) + lin(m4, y4)
            err = float((z - ref).abs().max() / ref.abs().max())
            assert err <= tol, (type(m).__module__, dt, err)
