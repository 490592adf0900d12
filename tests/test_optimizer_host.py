"""Host side of the training package (no GPU): the chunk plan and the argument errors of csrc/optimizer.hip through the C-ABI, the state
dicts and refusals of DeviceSGD / DeviceAdam, the schedulers, ModelOutputManager, the step-interval arithmetic, create_optimizer,
configure_trainable and the pretrained-backbone restore of build_model."""
import copy
import ctypes as C
import math
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip
    hip.lib()
    return hip


# ------------------------------------------------------------------------------------------------ C-ABI
def test_symbols_header_and_chunk_constant(hip):
    header = open(os.path.join(ROOT, "include", "stemseg_hip.h")).read()
    raw = C.CDLL(hip.LIB_PATH)
    for n in ("stemseg_hip_opt_plan", "stemseg_hip_opt_sgd_step", "stemseg_hip_opt_adam_step", "stemseg_hip_opt_grad_norm"):
        assert hasattr(raw, n) and n in hip.SIGNATURES and n + "(" in header, n
    assert "#define STEMSEG_OPT_CHUNK %d " % hip.OPT_CHUNK in header
    assert hip.lib().stemseg_hip_version() == 11
    assert C.sizeof(hip.OptTensor) == 48 and C.sizeof(hip.OptChunk) == 8 and C.sizeof(hip.OptHyper) == 40


def test_chunk_plan_covers_every_element_once_and_never_straddles(hip):
    CH = hip.OPT_CHUNK
    sizes = [1, 3, CH - 1, CH, CH + 1, 2 * CH + 7]
    for order in (sizes, sizes[::-1], [2 * CH + 7], [1]):
        tensors, chunks = hip.opt_plan([(4096 * (i + 1), 4096 * (i + 1), 0, 0, n, 0) for i, n in enumerate(order)], 0)
        assert len(chunks) == sum(-(-n // CH) for n in order)
        seen = [np.zeros(n, np.int32) for n in order]
        last = (-1, -1)
        for c in chunks:
            assert 0 <= c.tensor < len(order) and (c.tensor, c.chunk) > last            # table order: tensors, then rising chunks
            last = (c.tensor, c.chunk)
            lo, hi = c.chunk * CH, min(order[c.tensor], (c.chunk + 1) * CH)
            assert lo < hi <= order[c.tensor]                                           # inside ONE tensor, never empty
            seen[c.tensor][lo:hi] += 1
        assert all((s == 1).all() for s in seen)
    # a tensor of no elements has no chunk
    _, chunks = hip.opt_plan([(4096, 4096, 0, 0, 0, 0), (8192, 8192, 0, 0, 5, 0)], 0)
    assert [(c.tensor, c.chunk) for c in chunks] == [(1, 0)]


def test_argument_errors_before_any_hip_call(hip):
    l = hip.lib()
    E = -1                                                              # STEMSEG_E_INVALID
    one = (hip.OptTensor * 1)()
    one[0].p, one[0].g, one[0].n = 4096, 4096, 8
    n = C.c_int64(0)
    assert l.stemseg_hip_opt_plan(None, 1, 0, None, 0, C.byref(n)) == E
    assert l.stemseg_hip_opt_plan(one, 0, 0, None, 0, C.byref(n)) == E and b"n_tensors" in l.stemseg_hip_last_error()
    assert l.stemseg_hip_opt_plan(one, 1, 3, None, 0, C.byref(n)) == E
    assert l.stemseg_hip_opt_plan(one, 1, 1, None, 0, C.byref(n)) == E and b"state" in l.stemseg_hip_last_error()
    assert l.stemseg_hip_opt_plan(one, 1, 0, None, 0, C.byref(n)) == 0 and n.value == 1
    small = (hip.OptChunk * 1)()
    one[0].n = hip.OPT_CHUNK + 1
    assert l.stemseg_hip_opt_plan(one, 1, 0, small, 1, C.byref(n)) == E                 # the table is too short: nothing past it is written
    one[0].n = -1
    assert l.stemseg_hip_opt_plan(one, 1, 0, None, 0, C.byref(n)) == E and b"negative" in l.stemseg_hip_last_error()
    one[0].n, one[0].flags = 8, 2
    assert l.stemseg_hip_opt_plan(one, 1, 0, None, 0, C.byref(n)) == E and b"unknown flag" in l.stemseg_hip_last_error()
    one[0].flags, one[0].p = 0, 4098
    assert l.stemseg_hip_opt_plan(one, 1, 0, None, 0, C.byref(n)) == E and b"aligned" in l.stemseg_hip_last_error()
    h = hip.opt_hyper(lr=0.1, momentum=0.9)
    t, c = 4096, 8192                                                   # never dereferenced: every call below fails its checks first
    for fn, extra in ((l.stemseg_hip_opt_sgd_step, ()), (l.stemseg_hip_opt_adam_step, (4096,))):
        args = lambda tt, nt, cc, nc, hh: (tt, nt, cc, nc, hh) + extra + (None, None)
        assert fn(*args(None, 1, c, 1, C.byref(h))) == E and b"null table" in l.stemseg_hip_last_error()
        assert fn(*args(t, 1, None, 1, C.byref(h))) == E
        assert fn(*args(t, 0, c, 1, C.byref(h))) == E and b"n_tensors" in l.stemseg_hip_last_error()
        assert fn(*args(t, -3, c, 1, C.byref(h))) == E
        assert fn(*args(t, 1, c, 0, C.byref(h))) == E and b"n_chunks" in l.stemseg_hip_last_error()
        assert fn(*args(t, 1, c, 1, None)) == E
        bad = hip.opt_hyper()
        bad.flags = 6
        assert fn(*args(t, 1, c, 1, C.byref(bad))) == E and b"unknown flag" in l.stemseg_hip_last_error()
        bad = hip.opt_hyper()
        bad.struct_bytes -= 4
        assert fn(*args(t, 1, c, 1, C.byref(bad))) == E and b"size mismatch" in l.stemseg_hip_last_error()
    assert l.stemseg_hip_opt_adam_step(t, 1, c, 1, C.byref(h), None, None, None) == E and b"tensor_scalars" in l.stemseg_hip_last_error()
    gn = l.stemseg_hip_opt_grad_norm
    assert gn(None, 1, c, 1, 4096, 4096, 1.0, 4096, 4096, 4096, None) == E
    assert gn(t, 0, c, 1, 4096, 4096, 1.0, 4096, 4096, 4096, None) == E
    assert gn(t, 1, c, 1, None, 4096, 1.0, 4096, 4096, 4096, None) == E and b"null pointer" in l.stemseg_hip_last_error()
    assert gn(t, 1, c, 1, 4096, 4096, float("nan"), 4096, 4096, 4096, None) == E and b"NaN" in l.stemseg_hip_last_error()
    assert gn(t, 1, c, 1, 4100, 4096, 1.0, 4096, 4096, 4096, None) == E and b"aligned" in l.stemseg_hip_last_error()


def test_hyper_parameters_round_like_torch_scalars(hip):
    h = hip.opt_hyper(lr=0.1, momentum=0.9, dampening=0.5, weight_decay=1e-4, nesterov=True, beta1=0.9, beta2=0.999, eps=1e-8)
    f = lambda v: float(np.float32(v))
    assert (h.lr, h.momentum, h.one_minus_dampening, h.weight_decay) == (f(0.1), f(0.9), f(0.5), f(1e-4))
    assert (h.one_minus_beta1, h.beta2, h.one_minus_beta2, h.eps) == (f(1 - 0.9), f(0.999), f(1 - 0.999), f(1e-8))
    assert h.flags == hip.OPT_NESTEROV and h.struct_bytes == C.sizeof(hip.OptHyper)


# ------------------------------------------------------------------------------------------------ the optimiser classes
def _params(seed=0, sizes=((3, 4), (5,), (2, 2, 2))):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in sizes]
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g)
    return ps


def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert sa["param_groups"] == sb["param_groups"] and sa["state"].keys() == sb["state"].keys()
    for k in sa["state"]:
        assert sa["state"][k].keys() == sb["state"][k].keys()
        for n, v in sa["state"][k].items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(sb["state"][k][n])), (k, n)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_state_dicts_round_trip_with_the_stock_classes(kind):
    from stemseg_amd.training import DeviceAdam, DeviceSGD
    stock_cls, dev_cls, kw = ((torch.optim.SGD, DeviceSGD, dict(lr=0.1, momentum=0.9, nesterov=True, weight_decay=1e-4)) if kind == "sgd" else
                              (torch.optim.Adam, DeviceAdam, dict(lr=0.01, weight_decay=1e-2)))
    assert issubclass(dev_cls, stock_cls)
    stock = stock_cls(_params(), **kw)
    stock.step()
    stock.step()                                                        # a real state: buffers, Adam's step count
    dev = dev_cls(_params(), **dict(kw, lr=0.5))
    dev.load_state_dict(copy.deepcopy(stock.state_dict()))              # stock -> device class (load_state_dict keeps the tensors it is given)
    _same_state(dev, stock)
    assert dev.param_groups[0]["lr"] == kw["lr"]
    back = stock_cls(_params(), **dict(kw, lr=0.7))
    back.load_state_dict(copy.deepcopy(dev.state_dict()))               # device class -> stock
    _same_state(back, stock)
    with torch.no_grad():
        for a, b in zip(stock.param_groups[0]["params"], back.param_groups[0]["params"]):
            b.copy_(a)                                                  # the same weights, gradients and state: the same next step
    stock.step()
    back.step()
    for a, b in zip(stock.param_groups[0]["params"], back.param_groups[0]["params"]):
        assert torch.equal(a, b)
    # a fresh device optimiser has the parents' empty state dict
    assert dev_cls(_params(), **kw).state_dict() == stock_cls(_params(), **kw).state_dict()


def test_refusals_name_the_offender():
    from stemseg_amd.training import DeviceAdam, DeviceSGD, grad_norm
    for cls, kw in ((DeviceSGD, dict(maximize=True)), (DeviceAdam, dict(maximize=True)), (DeviceAdam, dict(amsgrad=True)),
                    (DeviceSGD, dict(foreach=True)), (DeviceAdam, dict(foreach=True)), (DeviceSGD, dict(fused=True)),
                    (DeviceAdam, dict(capturable=True))):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            cls(_params(), lr=0.1, **kw)
    # ... and when the option arrives through a loaded state dict
    opt = DeviceSGD(_params(), lr=0.1)
    opt.param_groups[0]["maximize"] = True
    with pytest.raises(NotImplementedError, match="maximize"):
        opt.step()
    # CPU parameters at step()
    for opt in (DeviceSGD(_params(), lr=0.1, momentum=0.9), DeviceAdam(_params(), lr=0.1)):
        with pytest.raises(NotImplementedError, match="cpu"):
            opt.step()
        assert len(opt.state) == 0
    with pytest.raises(NotImplementedError, match="cpu"):
        grad_norm(_params())
    # non-fp32, non-contiguous, sparse
    p = torch.nn.Parameter(torch.randn(4, dtype=torch.float64))
    p.grad = torch.randn(4, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="float64"):
        DeviceSGD([p], lr=0.1).step()
    p = torch.nn.Parameter(torch.randn(4, 6).t())
    p.grad = torch.randn(6, 4)
    assert not p.is_contiguous()
    with pytest.raises(NotImplementedError, match="non-contiguous"):
        DeviceSGD([p], lr=0.1).step()
    p = torch.nn.Parameter(torch.randn(4, 3))
    p.grad = torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.tensor([1.0]), (4, 3))
    with pytest.raises(NotImplementedError, match="sparse"):
        DeviceAdam([p], lr=0.1).step()
    with pytest.raises(ValueError):
        grad_norm([torch.nn.Parameter(torch.zeros(3))])                 # no gradient anywhere


# ------------------------------------------------------------------------------------------------ schedulers
def test_exponential_lr_follows_its_closed_form_over_the_start():
    from stemseg_amd.training import ExponentialLR, create_lr_scheduler
    lr, factor, steps, start = 0.1, 0.01, 5, 3
    opt = torch.optim.SGD(_params(), lr=lr)
    sched = ExponentialLR(opt, factor, steps, start)
    gamma = factor ** (1.0 / steps)
    assert sched.get_last_lr() == [lr]
    for k in range(1, 12):
        opt.step()
        sched.step()
        want = lr * gamma ** max(0, k - start + 1)
        assert math.isclose(sched.get_last_lr()[0], want, rel_tol=1e-12), (k, sched.get_last_lr(), want)
        assert opt.param_groups[0]["lr"] == sched.get_last_lr()[0]
    assert math.isclose(lr * gamma ** steps, lr * factor, rel_tol=1e-12)           # decay_steps after the start: down by decay_factor
    # its state dict resumes the sequence
    opt2 = torch.optim.SGD(_params(), lr=lr)
    sched2 = ExponentialLR(opt2, factor, steps, start)
    opt2.load_state_dict(opt.state_dict())
    sched2.load_state_dict(sched.state_dict())
    opt.step(), sched.step(), opt2.step(), sched2.step()
    assert sched2.get_last_lr() == sched.get_last_lr()
    cfg = NS(LR_DECAY_TYPE="exponential", LR_EXP_DECAY_FACTOR=factor, LR_EXP_DECAY_STEPS=steps, LR_EXP_DECAY_START=start, OPTIMIZER="SGD", INITIAL_LR=lr)
    assert isinstance(create_lr_scheduler(torch.optim.SGD(_params(), lr=lr), cfg, lambda s: None), ExponentialLR)


def test_step_and_none_schedulers():
    from stemseg_amd.training import create_lr_scheduler
    base = dict(LR_DECAY_STEPS=[2, 4], LR_DECAY_FACTOR=0.1, OPTIMIZER="SGD", INITIAL_LR=1.0)
    for kind, want in (("step", [1.0, 0.1, 0.1, 0.01, 0.01]), ("none", [1.0] * 5)):
        opt = torch.optim.SGD(_params(), lr=1.0)
        sched = create_lr_scheduler(opt, NS(LR_DECAY_TYPE=kind, **base), lambda s: None)
        got = []
        for _ in range(5):
            opt.step()
            sched.step()
            got.append(sched.get_last_lr()[0])
        assert np.allclose(got, want, rtol=1e-12), (kind, got)
    with pytest.raises(ValueError, match="LR_DECAY_TYPE"):
        create_lr_scheduler(torch.optim.SGD(_params(), lr=1.0), NS(LR_DECAY_TYPE="cosine", **base), lambda s: None)


# ------------------------------------------------------------------------------------------------ the loop's helpers
def test_model_output_manager_divides_and_resets():
    from stemseg_amd.training import ModelOutputManager
    from stemseg_amd.utils.constants import ModelOutput
    mgr = ModelOutputManager(4)
    a = torch.tensor(2.0, requires_grad=True)
    out = lambda s: {ModelOutput.OPTIMIZATION_LOSSES: {"embedding_loss": a * s, "foreground": torch.tensor(1.0)},
                     ModelOutput.OTHERS: {"lovasz_loss": torch.tensor(8.0), "count": 6}}
    loss = mgr(out(1.0))
    assert loss.requires_grad and float(loss.detach()) == (2.0 + 1.0) / 4
    loss.backward()
    assert float(a.grad) == 0.25
    mgr(out(3.0))
    tensors, others = mgr.reset()
    assert {k: float(v) for k, v in tensors.items()} == {"embedding_loss": (2.0 + 6.0) / 4, "foreground": 0.5, "lovasz_loss": 4.0}
    assert not any(v.requires_grad for v in tensors.values()) and others == {"count": 3.0}
    assert mgr.reset() == ({}, {})
    assert ModelOutputManager(1, excluded_keys=("count",))(out(1.0)) is not None


def test_optimizer_step_interval_and_its_asserts():
    from stemseg_amd.training import optimizer_step_interval
    assert optimizer_step_interval(2, 1, True) == (2, 1)                 # the reference's defaults
    assert optimizer_step_interval(8, 2, True) == (4, 2)
    assert optimizer_step_interval(8, 2, True, num_gpus=2) == (2, 2)
    assert optimizer_step_interval(4, 4, True) == (1, 4)
    assert optimizer_step_interval(3, 4, False) == (1, 3)                # no accumulation: the batch in one go
    with pytest.raises(AssertionError, match="no multiple"):
        optimizer_step_interval(5, 2, True)
    with pytest.raises(AssertionError, match="number of GPUs"):
        optimizer_step_interval(1, 1, True, num_gpus=2)
    with pytest.raises(ValueError, match="does not fit"):
        optimizer_step_interval(5, 4, False)


def test_create_optimizer_picks_class_and_hyper_parameters():
    from stemseg_amd.training import DeviceAdam, DeviceSGD, create_optimizer
    model = torch.nn.Linear(3, 2)
    cfg = NS(OPTIMIZER="SGD", INITIAL_LR=0.02, MOMENTUM=0.8, WEIGHT_DECAY=3e-4, NESTEROV=True)
    said = []
    opt = create_optimizer(model, cfg, said.append)
    g = opt.param_groups[0]
    assert type(opt) is DeviceSGD and (g["lr"], g["momentum"], g["weight_decay"], g["nesterov"], g["dampening"]) == (0.02, 0.8, 3e-4, True, 0)
    assert [id(p) for p in g["params"]] == [id(p) for p in model.parameters()] and said
    assert type(create_optimizer(model, cfg, said.append, device_step=False)) is torch.optim.SGD
    cfg.OPTIMIZER = "adam"
    opt = create_optimizer(model, cfg, said.append)
    g = opt.param_groups[0]
    assert type(opt) is DeviceAdam and (g["lr"], g["weight_decay"], g["betas"], g["eps"]) == (0.02, 3e-4, (0.9, 0.999), 1e-8)
    assert type(create_optimizer(model, cfg, said.append, device_step=False)) is torch.optim.Adam
    cfg.OPTIMIZER = "lamb"
    with pytest.raises(ValueError, match="lamb"):
        create_optimizer(model, cfg, said.append)


def test_var_keys_to_str():
    from stemseg_amd.training import var_keys_to_str
    assert var_keys_to_str({"embedding_loss": 1.23456, "foreground": 0.5, "lr": 1e-3}) == "EmbL: 1.235 - FgL: 0.500 - LR: 1.00E-03"


def test_parser_has_the_reference_flags():
    from stemseg_amd.training.main import build_parser
    a = build_parser().parse_args(["--model_dir", "x", "--cfg", "ytvis", "--log_level", "debug"])
    assert (a.display_interval, a.summary_interval, a.save_interval, a.num_cpu_workers, a.ckpts_to_keep) == (5, 10, 10000, 8, 2)
    assert a.restore_session is None and a.initial_ckpt is None and not a.no_resume and not a.allow_multigpu and a.log_level == 10


# ------------------------------------------------------------------------------------------------ the model side
@pytest.fixture(scope="module")
def small_model():
    """kittimots preset, R-50, built on the CPU."""
    from stemseg_amd import config
    from stemseg_amd.modeling.model_builder import build_model
    try:
        config.load_preset("kittimots")
        config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
        yield build_model()
    finally:
        config.load_preset("defaults")


def _frozen_prefixes(freeze_at):
    return ("backbone.body.stem.",) + tuple("backbone.body.layer%d." % st for st in range(1, freeze_at))


@pytest.mark.parametrize("freeze_at", [2, 3, 4])
def test_configure_trainable_freeze_at_stage(small_model, freeze_at):
    from stemseg_amd import config
    from stemseg_amd.training import configure_trainable
    m = small_model
    cfg = config.make_cfg("kittimots")
    cfg.MODEL.BACKBONE.FREEZE_AT_STAGE = freeze_at
    for p in m.parameters():
        p.requires_grad_(False)
    m.train_decoders = m.train_fpn = m.train_body = False
    assert configure_trainable(m, cfg) is m
    trainable = {k for k, p in m.named_parameters() if p.requires_grad}
    want = {k for k, _ in m.named_parameters() if not k.startswith(_frozen_prefixes(freeze_at))}
    assert trainable == want
    assert trainable == set(m.decoder_parameters()) | set(m.fpn_parameters()) | set(m.body_parameters(freeze_at))
    assert (m.train_decoders, m.train_fpn, m.train_body, m.train_wide_head) == (True, True, True, False)
    assert m.body_freeze_at() == freeze_at and m.body_fpn_and_decoders_only_trainable(freeze_at)


def test_configure_trainable_freeze_backbone_and_refusal(small_model):
    from stemseg_amd import config
    from stemseg_amd.training import configure_trainable
    m = small_model
    cfg = config.make_cfg("kittimots")
    cfg.TRAINING.FREEZE_BACKBONE = True
    configure_trainable(m, cfg)
    assert {k for k, p in m.named_parameters() if p.requires_grad} == set(m.decoder_parameters())
    assert m.train_decoders and m.decoders_only_trainable() and not m.train_wide_head
    cfg.TRAINING.FREEZE_BACKBONE = False
    before = [p.requires_grad for p in m.parameters()], (m.train_decoders, m.train_fpn, m.train_body)
    for bad in (0, 1, 5):
        cfg.MODEL.BACKBONE.FREEZE_AT_STAGE = bad
        with pytest.raises(NotImplementedError, match="FREEZE_AT_STAGE"):
            configure_trainable(m, cfg)
        assert ([p.requires_grad for p in m.parameters()], (m.train_decoders, m.train_fpn, m.train_body)) == before     # refused before any change
    # the caller's own TRAINING section wins over the cfg's (the Trainer passes its FREEZE_BACKBONE)
    cfg.MODEL.BACKBONE.FREEZE_AT_STAGE = 2
    configure_trainable(m, cfg, freeze_backbone=True)
    assert {k for k, p in m.named_parameters() if p.requires_grad} == set(m.decoder_parameters()) and not m.train_fpn and not m.train_body
    configure_trainable(m, cfg, freeze_backbone=False)
    assert m.train_fpn and m.train_body and any(p.requires_grad for p in m.backbone.fpn.parameters())
    # a head wider than the fused heads kernel serves switches the wide path on
    narrow = m.semseg_head.out_channels
    try:
        from stemseg_amd import hip
        m.semseg_head.out_channels = hip.MAX_HEAD_OUT + 1
        cfg.MODEL.BACKBONE.FREEZE_AT_STAGE = 2
        assert configure_trainable(m, cfg).train_wide_head is True
    finally:
        m.semseg_head.out_channels = narrow
        m.train_wide_head = False


def test_build_model_restores_the_pretrained_backbone(small_model, tmp_path, monkeypatch):
    from stemseg_amd import config
    from stemseg_amd.modeling.model_builder import build_model
    monkeypatch.setenv("STEMSEG_MODELS_DIR", str(tmp_path))
    try:
        config.load_preset("kittimots")
        config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
        config.cfg.MODEL.BACKBONE.PRETRAINED_WEIGHTS = "backbone_r50.pth"
        with pytest.raises(ValueError, match="backbone_r50.pth"):
            build_model(restore_pretrained_backbone_wts=True)
        sd = {k: torch.full_like(v, 0.25) + torch.arange(v.numel(), dtype=v.dtype).reshape(v.shape) % 7
              for k, v in small_model.backbone.state_dict().items()}
        os.makedirs(tmp_path / "pretrained")
        torch.save(sd, tmp_path / "pretrained" / "backbone_r50.pth")
        said = []
        m = build_model(restore_pretrained_backbone_wts=True, logger=NS(info=said.append))
        got = m.backbone.state_dict()
        assert got.keys() == sd.keys() and all(torch.equal(got[k], sd[k]) for k in sd)
        assert said and "backbone_r50.pth" in said[0]
        # strict: a file with a key missing is refused
        sd.pop(next(iter(sd)))
        torch.save(sd, tmp_path / "pretrained" / "backbone_r50.pth")
        with pytest.raises(RuntimeError, match="Missing key"):
            build_model(restore_pretrained_backbone_wts=True)
        # the default path never looks at the file
        monkeypatch.delenv("STEMSEG_MODELS_DIR")
        assert build_model() is not None
    finally:
        config.load_preset("defaults")


def test_trainer_refuses_mixed_precision_and_a_process_group(tmp_path, monkeypatch):
    from stemseg_amd.training.main import Trainer
    args = NS(restore_session=None, initial_ckpt=None)
    cfg = NS(MIXED_PRECISION=True)
    with pytest.raises(NotImplementedError, match="apex"):
        Trainer(cfg, str(tmp_path), args, NS(info=print), model=object())
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    with pytest.raises(NotImplementedError, match="2 ranks"):
        Trainer(NS(MIXED_PRECISION=False), str(tmp_path), args, NS(info=print), model=object())


def test_training_logger_keeps_the_reference_state_keys(tmp_path):
    """What a reference checkpoint holds under 'logger' loads here and the other way round: the keys are its TrainingLogger's private
    attributes, name-mangled."""
    from stemseg_amd.training.main import TrainingLogger
    log = TrainingLogger(str(tmp_path / "logs"), num_iterations=100)
    log.start_timer()
    log.add_training_point(4, True, embedding_loss=1.5)
    state = log.state_dict()
    assert sorted(state) == ["_TrainingLogger__latest_iteration_num", "_TrainingLogger__latest_timestamp", "_TrainingLogger__pause_duration",
                             "_TrainingLogger__train_start_time", "total_iterations"]
    assert state["_TrainingLogger__latest_iteration_num"] == 4 and state["total_iterations"] == 100 and log.last_point == {"embedding_loss": 1.5, "iteration": 4}
    other = TrainingLogger(str(tmp_path / "logs2"))
    other.load_state_dict(dict(state, _TrainingLogger__train_start_time=state["_TrainingLogger__latest_timestamp"] - 8.0))
    left, per_iteration = other.compute_eta(as_string=False)
    assert abs(per_iteration - 2.0) < 1e-9 and abs(left - 192.0) < 1e-6          # 8 s for 4 iterations, 96 to go
    assert other.compute_eta()[0] == "0-00:03:12"
    with pytest.raises(KeyError, match="bogus"):
        other.load_state_dict({"bogus": 1})
