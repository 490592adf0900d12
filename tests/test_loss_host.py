"""CPU tests of the embedding loss: the torch oracle (tests/loss_oracle.py) against the golden values of the reference's own
EmbeddingLoss (tests/golden/embedding_loss.npz, written by tools/make_loss_goldens.py), the C-ABI of the three entry points (argument
errors are reported before any GPU call) and the public module's interface.

Bounds: both sides are fp32 restatements of one arithmetic in different summation orders, so the yardstick is that arithmetic's own
fp32-versus-fp64 spread on the fixtures (measured with the oracle in both precisions and with the golden values against the fp64
oracle): at most 1.4e-7 relative on a loss, 4.3e-6 of max|g| on an element of the total gradient.  Allowed: 4 x that."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import loss_oracle as LO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = LO.load_fixtures(os.path.join(ROOT, "tests", "golden", "embedding_loss.npz"))
LOSS_REL = 4 * 1.4e-7
GRAD_REL = 4 * 4.3e-6


def test_fixture_list_covers_the_quirks():
    assert sorted(FIXTURES) == sorted(LO.FIXTURE_CASES)
    f = FIXTURES["empty_middle"]["targets"][0]["masks"]
    cnt = f.reshape(f.shape[0], -1).sum(1)
    assert cnt[1] == 0 and cnt[0] > 0 and cnt[2] > 0                 # an empty instance in the middle: the index shift
    assert FIXTURES["sample_without_instances"]["targets"][0]["masks"].numel() == 0
    assert all(int(t["masks"].sum()) == 0 for t in FIXTURES["all_empty_batch"]["targets"])
    assert (FIXTURES["n2_overlap"]["targets"][0]["masks"].sum(0) > 1).any()
    assert FIXTURES["xyt"]["targets"][0]["ignore_masks"].any()
    assert len(FIXTURES["xyff_free_dims"]["stds"]) == 2 and FIXTURES["xytf_n2"]["x"].shape[0] == 2


@pytest.mark.parametrize("name", sorted(LO.FIXTURE_CASES))
def test_oracle_reproduces_reference(name):
    f = FIXTURES[name]
    for inputs in (f, None):                                          # the stored inputs, and the generator that made them
        if inputs is None:
            x, targets = LO.make_case(name)
            assert torch.equal(x, f["x"]) and all(torch.equal(a["masks"], b["masks"]) for a, b in zip(targets, f["targets"]))
            continue
        losses, grads = LO.losses_and_grads(f["x"], f["targets"], f["E"], f["stds"], torch.float32)
        total, gtotal = LO.total_of(losses, grads)
        ref = f["losses"]
        for got, want, what in zip([total] + list(losses), ref, ("total", "lovasz", "smoothness", "seediness")):
            print(name, what, got, want)
            assert abs(got - want) <= LOSS_REL * abs(want), (what, got, want)
        gmax = np.abs(f["grad"]).max()
        err = np.abs(gtotal - f["grad"]).max()
        print(name, "grad max-norm error / max|g|", err / max(gmax, 1e-30))
        assert err <= GRAD_REL * gmax


def test_zero_instance_batch_is_exactly_zero():
    f = FIXTURES["all_empty_batch"]
    assert not f["losses"].any() and not f["grad"].any()


# ------------------------------------------------------------------------------------------------ C-ABI
def _desc(hip, **over):
    d = hip.embedding_loss_desc(3, [], 2, 2, 4, 4)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_loss_symbols_exported_and_reject_bad_arguments():
    from stemseg_amd import hip
    names = ("stemseg_hip_embedding_loss_workspace_bytes", "stemseg_hip_embedding_loss_forward", "stemseg_hip_embedding_loss_backward")
    raw = ctypes.CDLL(hip.LIB_PATH)
    for n in names:
        assert hasattr(raw, n) and n in hip.SIGNATURES, n
    header = open(os.path.join(ROOT, "include", "stemseg_hip.h")).read()
    assert all(n + "(" in header for n in names)
    l = hip.lib()
    assert l.stemseg_hip_version() == 11
    ws = l.stemseg_hip_embedding_loss_workspace_bytes(ctypes.byref(_desc(hip)))
    assert ws > 0 and l.stemseg_hip_embedding_loss_workspace_bytes(ctypes.byref(_desc(hip, n_instances=4))) > ws
    for over, word in ((dict(struct_bytes=8), b"ABI skew"), (dict(embedding_size=0), b"embedding_size"), (dict(embedding_size=9), b"embedding_size"),
                       (dict(n_free_dims=3), b"n_free_dims"), (dict(n_instances=0), b"n_instances"), (dict(T=0), b"bad dims"),
                       (dict(T=4096, H=4096, W=2), b"voxels"), (dict(reserved=1), b"reserved")):
        assert l.stemseg_hip_embedding_loss_workspace_bytes(ctypes.byref(_desc(hip, **over))) == 0
        assert word in l.stemseg_hip_last_error(), (over, l.stemseg_hip_last_error())
    d = _desc(hip)
    fake = ctypes.c_void_p(256)
    fwd = lambda x=fake, m=fake, ig=fake, w=fake, nb=ws, out=fake, dd=d: l.stemseg_hip_embedding_loss_forward(
        ctypes.byref(dd), x, m, ig, w, nb, out, None, None)
    assert fwd(x=None) == -1 and b"null pointer" in l.stemseg_hip_last_error()
    assert fwd(out=None) == -1 and b"null pointer" in l.stemseg_hip_last_error()
    assert fwd(nb=ws - 1) == -1 and b"workspace too small" in l.stemseg_hip_last_error()
    assert fwd(w=ctypes.c_void_p(8)) == -1 and b"aligned" in l.stemseg_hip_last_error()
    assert fwd(dd=_desc(hip, struct_bytes=4)) == -1 and b"ABI skew" in l.stemseg_hip_last_error()
    bwd = lambda up=fake, total=1, batch=1, g=fake, nb=ws: l.stemseg_hip_embedding_loss_backward(
        ctypes.byref(d), fake, fake, fake, fake, nb, up, total, batch, g, None)
    assert bwd(up=None) == -1 and b"null pointer" in l.stemseg_hip_last_error()
    assert bwd(total=0) == -1 and b"total_instances" in l.stemseg_hip_last_error()
    assert bwd(batch=0) == -1 and b"batch_size" in l.stemseg_hip_last_error()
    assert bwd(nb=0) == -1 and b"workspace too small" in l.stemseg_hip_last_error()
    free = _desc(hip, embedding_size=4, n_free_dims=1)
    assert l.stemseg_hip_embedding_loss_workspace_bytes(ctypes.byref(free)) == 0 and b"free_dim_bandwidths" in l.stemseg_hip_last_error()


def test_isa_report_covers_the_loss_kernels():
    import json
    from stemseg_amd import hip
    rep = json.load(open(os.path.splitext(hip.LIB_PATH)[0] + ".isa.json"))["sources"]["embedding_loss.hip"]
    assert rep["assembly_found"] and rep["kernels"] >= 14 and rep["packed_fp32_valu_instructions"] == 0


# ------------------------------------------------------------------------------------------------ public module
def test_module_interface_and_output_keys(monkeypatch):
    from stemseg_amd.modeling import losses
    from stemseg_amd.modeling.losses import embedding_loss as mod
    from stemseg_amd.utils.constants import Loss, ModelOutput
    assert (ModelOutput.OPTIMIZATION_LOSSES, ModelOutput.OTHERS) == ("optimization_losses", "others")
    assert (Loss.EMBEDDING, Loss.LOVASZ_LOSS, Loss.VARIANCE_SMOOTHNESS, Loss.SEEDINESS_LOSS) == \
        ("embedding_loss", "lovasz_loss", "variance_smoothness_loss", "seediness_loss")
    with pytest.raises(AssertionError, match="does not match number of free dims"):
        losses.EmbeddingLoss(4, EMBEDDING_SIZE=4, NBR_FREE_DIMS=2, FREE_DIM_STDS=[0.3], **LO.DEFAULT_WEIGHTS)
    loss = losses.EmbeddingLoss(4, EMBEDDING_SIZE=4, NBR_FREE_DIMS=2, FREE_DIM_STDS=[0.3, 0.4], **LO.DEFAULT_WEIGHTS)
    assert loss.num_input_channels == 7 and loss.split_sizes == (4, 2, 1)
    assert torch.equal(loss.free_dim_bandwidths, 1. / torch.tensor([[0.3, 0.4]]) ** 2)
    with pytest.raises(AssertionError, match="Expected 7 channels"):
        loss(torch.zeros(1, 6, 2, 4, 4), [], {})
    # the combination and the keys, with the device function replaced by fixed components (no GPU here)
    comps = (torch.tensor(0.5), torch.tensor(0.25), torch.tensor(0.125))
    monkeypatch.setattr(mod.EmbeddingLossFunction, "apply", staticmethod(lambda *a: comps))
    monkeypatch.setattr(mod.hip, "require_gpu", lambda: 1)
    od = {}
    loss(torch.zeros(1, 7, 2, 4, 4), [{"masks": torch.zeros(1, 2, 4, 4, dtype=torch.uint8), "ignore_masks": torch.zeros(2, 4, 4, dtype=torch.bool)}], od)
    assert set(od) == {"optimization_losses", "others"} and set(od["optimization_losses"]) == {"embedding_loss"}
    assert set(od["others"]) == {"lovasz_loss", "variance_smoothness_loss", "seediness_loss"}
    assert float(od["optimization_losses"]["embedding_loss"]) == 0.5 + 10 * 0.25 + 0.125
    assert od["others"]["lovasz_loss"] is comps[0] and od["others"]["seediness_loss"] is comps[2]


def test_overlay_serves_the_reference_import_name():
    from stemseg_amd import overlay
    overlay.install()
    try:
        from stemseg.modeling.losses import EmbeddingLoss
        from stemseg_amd.modeling.losses import EmbeddingLoss as Ours
        assert EmbeddingLoss is Ours
    finally:
        overlay.uninstall()
