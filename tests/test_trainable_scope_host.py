"""Host test of which graph ``TrainingModel.forward`` builds (modeling/model_builder.py): the six switches x what requires a gradient -> the
backbone entry point that is called (with its freeze_at), the heads' call (plain, or ``forward_stacks_trainable`` with its ``full`` flag) and
``trainable_scope()``, or the refusal, word for word.  The kernels are replaced by recording stubs: no GPU, no library.  Every expectation is
a literal below; ``run_backbone`` and ``forward_embeddings_and_semseg`` called on their own have rows of their own."""
import contextlib
import itertools

import pytest
import torch

HEADS = ("embedding_head", "semseg_head")                  # (the kittimots preset has no seediness head)

# ---- the outcomes: (backbone entry point, the heads' call, trainable_scope()) ----
PLAIN = ("forward", "plain", (None, None))
TAIL = ("forward", ("stacks", False), ("tail", None))
DEC = ("forward", ("stacks", True), ("decoders", None))
FPN = ("forward_trainable_fpn", ("stacks", True), ("fpn", None))
BODY = {fa: (("forward_trainable_body", fa), ("stacks", True), ("body", fa)) for fa in (0, 1, 2, 3, 4)}
E_TAIL = ("TrainingModel.forward with gradients: the decoder and encoder backward passes are not implemented; call it under "
          "torch.no_grad() (validation), or use compute_losses for the loss gradients with respect to the head outputs")
E_DEC = ("TrainingModel.forward with train_decoders: the encoder backward pass is not implemented, and %d parameters outside the "
         "decoders require a gradient (%s, ...); freeze the backbone (TRAINING.FREEZE_BACKBONE)")
E_FPN = ("TrainingModel.forward with train_decoders and train_fpn: behind the FPN the encoder backward pass is not implemented, and "
         "%d parameters outside the decoders and the FPN require a gradient (%s, ...); the backbone's body must be frozen "
         "(requires_grad_(False) on backbone.body)")
E_BODY = ("TrainingModel.forward with train_decoders, train_fpn and train_body: the backward pass of the stem, the max-pool and layer1 is not "
          "implemented (MODEL.BACKBONE.FREEZE_AT_STAGE >= 2), and %d parameters there require a gradient (%s, ...); freeze them "
          "(requires_grad_(False) on backbone.body.stem and backbone.body.layer1)")
E_STEM = ("TrainingModel.forward with train_decoders, train_fpn, train_body and train_stem: %d parameters outside the decoders, the FPN and the "
          "body's convolution weights require a gradient (%s, ...)")
FPN0, L1, L2, L3, L4, STEM = ("backbone.fpn.fpn_inner1.weight", "backbone.body.layer1.0.downsample.0.weight", "backbone.body.layer2.0.downsample.0.weight",
                              "backbone.body.layer3.0.downsample.0.weight", "backbone.body.layer4.0.downsample.0.weight", "backbone.body.stem.conv1.weight")

_DEC = lambda k: k.split(".")[0] in HEADS
_FPN = lambda k: k.startswith("backbone.fpn.")
_LAYERS = lambda *sts: lambda k: any(k.startswith("backbone.body.layer%d." % st) for st in sts)
# what requires a gradient: name -> predicate on the state-dict key ("tail" and "tail1+layer3" are resolved against tail_parameters())
PATTERNS = {
    "none": lambda k: False,
    "tail": None,
    "decoders": _DEC,
    "fpn": _FPN,
    "dec+fpn": lambda k: _DEC(k) or _FPN(k),
    "+layer4": lambda k: _DEC(k) or _FPN(k) or _LAYERS(4)(k),
    "+layer2..4": lambda k: _DEC(k) or _FPN(k) or _LAYERS(2, 3, 4)(k),
    "+layer1": lambda k: _DEC(k) or _FPN(k) or _LAYERS(1, 2, 3, 4)(k),
    "+stem": lambda k: _DEC(k) or _FPN(k) or k.startswith("backbone.body."),
    "everything": lambda k: True,
    "tail1+layer3": None,
}

# the switches as four letters: d train_decoders, f train_fpn, b train_body, s train_stem ("-": off)
SWITCHES = ["".join(c if on else "-" for c, on in zip("dfbs", bits)) for bits in itertools.product((False, True), repeat=4)]

# pattern -> {switches: outcome}.  The counts: 16 FPN tensors, 53 body weights (1 + 10 + 13 + 19 + 10), 69 in the backbone.
FORWARD = {
    "none": {s: PLAIN for s in SWITCHES},
    "tail": {"----": TAIL, "---s": TAIL, "--b-": TAIL, "--bs": TAIL, "-f--": TAIL, "-f-s": TAIL, "-fb-": TAIL, "-fbs": TAIL,
             "d---": DEC, "d--s": DEC, "d-b-": DEC, "d-bs": DEC, "df--": DEC, "df-s": DEC, "dfb-": DEC, "dfbs": DEC},
    "decoders": {"----": E_TAIL, "---s": E_TAIL, "--b-": E_TAIL, "--bs": E_TAIL, "-f--": E_TAIL, "-f-s": E_TAIL, "-fb-": E_TAIL, "-fbs": E_TAIL,
                 "d---": DEC, "d--s": DEC, "d-b-": DEC, "d-bs": DEC, "df--": DEC, "df-s": DEC, "dfb-": DEC, "dfbs": DEC},
    "fpn": {"----": E_TAIL, "---s": E_TAIL, "--b-": E_TAIL, "--bs": E_TAIL, "-f--": E_TAIL, "-f-s": E_TAIL, "-fb-": E_TAIL, "-fbs": E_TAIL,
            "d---": E_DEC % (16, FPN0), "d--s": E_DEC % (16, FPN0), "d-b-": E_DEC % (16, FPN0), "d-bs": E_DEC % (16, FPN0),
            "df--": FPN, "df-s": FPN, "dfb-": FPN, "dfbs": FPN},
    "dec+fpn": {"----": E_TAIL, "---s": E_TAIL, "--b-": E_TAIL, "--bs": E_TAIL, "-f--": E_TAIL, "-f-s": E_TAIL, "-fb-": E_TAIL, "-fbs": E_TAIL,
                "d---": E_DEC % (16, FPN0), "d--s": E_DEC % (16, FPN0), "d-b-": E_DEC % (16, FPN0), "d-bs": E_DEC % (16, FPN0),
                "df--": FPN, "df-s": FPN, "dfb-": FPN, "dfbs": FPN},
    "+layer4": {"----": E_TAIL, "---s": E_TAIL, "--b-": E_TAIL, "--bs": E_TAIL, "-f--": E_TAIL, "-f-s": E_TAIL, "-fb-": E_TAIL, "-fbs": E_TAIL,
                "d---": E_DEC % (26, L4), "d--s": E_DEC % (26, L4), "d-b-": E_DEC % (26, L4), "d-bs": E_DEC % (26, L4),
                "df--": E_FPN % (10, L4), "df-s": E_FPN % (10, L4), "dfb-": BODY[4], "dfbs": BODY[4]},
    "+layer2..4": {"----": E_TAIL, "---s": E_TAIL, "--b-": E_TAIL, "--bs": E_TAIL, "-f--": E_TAIL, "-f-s": E_TAIL, "-fb-": E_TAIL, "-fbs": E_TAIL,
                   "d---": E_DEC % (58, L2), "d--s": E_DEC % (58, L2), "d-b-": E_DEC % (58, L2), "d-bs": E_DEC % (58, L2),
                   "df--": E_FPN % (42, L2), "df-s": E_FPN % (42, L2), "dfb-": BODY[2], "dfbs": BODY[2]},
    "+layer1": {"----": E_TAIL, "---s": E_TAIL, "--b-": E_TAIL, "--bs": E_TAIL, "-f--": E_TAIL, "-f-s": E_TAIL, "-fb-": E_TAIL, "-fbs": E_TAIL,
                "d---": E_DEC % (68, L1), "d--s": E_DEC % (68, L1), "d-b-": E_DEC % (68, L1), "d-bs": E_DEC % (68, L1),
                "df--": E_FPN % (52, L1), "df-s": E_FPN % (52, L1), "dfb-": E_BODY % (10, L1), "dfbs": BODY[1]},
    "+stem": {"----": E_TAIL, "---s": E_TAIL, "--b-": E_TAIL, "--bs": E_TAIL, "-f--": E_TAIL, "-f-s": E_TAIL, "-fb-": E_TAIL, "-fbs": E_TAIL,
              "d---": E_DEC % (69, STEM), "d--s": E_DEC % (69, STEM), "d-b-": E_DEC % (69, STEM), "d-bs": E_DEC % (69, STEM),
              "df--": E_FPN % (53, STEM), "df-s": E_FPN % (53, STEM), "dfb-": E_BODY % (11, STEM), "dfbs": BODY[0]},
    "everything": {"----": E_TAIL, "---s": E_TAIL, "--b-": E_TAIL, "--bs": E_TAIL, "-f--": E_TAIL, "-f-s": E_TAIL, "-fb-": E_TAIL, "-fbs": E_TAIL,
                   "d---": E_DEC % (69, STEM), "d--s": E_DEC % (69, STEM), "d-b-": E_DEC % (69, STEM), "d-bs": E_DEC % (69, STEM),
                   "df--": E_FPN % (53, STEM), "df-s": E_FPN % (53, STEM), "dfb-": E_BODY % (11, STEM), "dfbs": BODY[0]},
    "tail1+layer3": {"----": E_TAIL, "---s": E_TAIL, "--b-": E_TAIL, "--bs": E_TAIL, "-f--": E_TAIL, "-f-s": E_TAIL, "-fb-": E_TAIL, "-fbs": E_TAIL,
                     "d---": E_DEC % (19, L3), "d--s": E_DEC % (19, L3), "d-b-": E_DEC % (19, L3), "d-bs": E_DEC % (19, L3),
                     "df--": E_FPN % (19, L3), "df-s": E_FPN % (19, L3), "dfb-": BODY[3], "dfbs": BODY[3]},
}

# (pattern, switches, under no_grad, TRAINING.FREEZE_BACKBONE) -> outcome: no graph without gradients; a backbone frozen by the cfg takes the no-grad
# pass whatever the scope says
OTHER = [
    ("everything", "----", True, False, PLAIN),
    ("tail", "----", True, False, PLAIN),
    ("decoders", "d---", True, False, PLAIN),
    ("dec+fpn", "df--", True, False, PLAIN),
    ("+layer2..4", "dfb-", True, False, PLAIN),
    ("+stem", "dfbs", True, False, PLAIN),
    ("dec+fpn", "dfb-", False, True, ("forward", ("stacks", True), ("fpn", None))),
    ("+layer2..4", "dfb-", False, True, ("forward", ("stacks", True), ("body", 2))),
]

# run_backbone() on its own: (pattern, switches) -> the backbone entry point.  It refuses nothing: without a graph it can carry, the no-grad pass.
RUN_BACKBONE = [
    ("none", "dfbs", "forward"),
    ("tail", "----", "forward"),
    ("decoders", "dfb-", "forward"),
    ("fpn", "df--", "forward_trainable_fpn"),
    ("fpn", "d---", "forward"),
    ("dec+fpn", "dfb-", "forward_trainable_fpn"),
    ("+layer4", "df--", "forward"),
    ("+layer4", "dfb-", ("forward_trainable_body", 4)),
    ("+layer2..4", "dfbs", ("forward_trainable_body", 2)),
    ("tail1+layer3", "dfb-", ("forward_trainable_body", 3)),
    ("+layer1", "dfbs", ("forward_trainable_body", 1)),
    ("everything", "dfbs", ("forward_trainable_body", 0)),
]
# THE ONE DELIBERATE DIFFERENCE of the single scope decision: the three switches set and a trainable parameter the body's backward does not
# reach (layer1 or the stem without train_stem).  forward() has always refused this; run_backbone() on its own used to build a body graph at
# body_freeze_at() all the same, which left that parameter without a gradient.  With trainable_scope() it builds no graph.
RUN_BACKBONE_OUTSIDE = [
    ("+layer1", "dfb-", ("forward_trainable_body", 2), "forward"),
    ("everything", "dfb-", ("forward_trainable_body", 2), "forward"),
]

# forward_embeddings_and_semseg() on its own: (pattern, switches) -> the heads' call
HEADS_ALONE = [
    ("none", "dfbs", "plain"),
    ("tail", "----", ("stacks", False)),
    ("tail", "d---", ("stacks", True)),
    ("decoders", "----", "plain"),
    ("decoders", "d---", ("stacks", True)),
    ("fpn", "d---", "plain"),
    ("dec+fpn", "df--", ("stacks", True)),
    ("+layer4", "df--", "plain"),
    ("+layer2..4", "dfb-", ("stacks", True)),
    ("+layer1", "dfb-", "plain"),
    ("+layer1", "dfbs", ("stacks", True)),
    ("everything", "dfb-", "plain"),
    ("everything", "dfbs", ("stacks", True)),
]


class _Harness:
    """The kittimots R-50 model with every kernel-side call replaced by a recording stub."""

    def __init__(self):
        from stemseg_amd.modeling.model_builder import build_model
        self.m = m = build_model()
        self.named = dict(m.named_parameters())
        self.calls = []
        maps = lambda x: tuple(torch.zeros(x.shape[0], 1, 1, 1) for _ in range(4))
        m.resize_masks = lambda targets: targets
        m.compute_losses = lambda emb, sem, targets: {"embeddings": tuple(emb.shape), "semseg": tuple(sem.shape)}
        bb = m.backbone
        bb.forward = lambda x: self.calls.append(("backbone", "forward")) or maps(x)
        bb.forward_trainable_fpn = lambda x: self.calls.append(("backbone", "forward_trainable_fpn")) or maps(x)
        bb.forward_trainable_body = lambda x, freeze_at: self.calls.append(("backbone", ("forward_trainable_body", freeze_at))) or maps(x)
        for name in HEADS:
            self._stub_head(name, getattr(m, name))
        tail = list(m.tail_parameters())
        self.patterns = dict(PATTERNS)
        self.patterns["tail"] = lambda k: k in tail
        self.patterns["tail1+layer3"] = lambda k: k == tail[0] or k.startswith("backbone.body.layer3.")

    def _stub_head(self, name, head):
        out = lambda xs: torch.zeros(xs[0].shape[0], 2, xs[0].shape[2], 1, 1)
        head.forward = lambda xs: self.calls.append((name, "plain")) or out(xs)
        head.forward_stacks_trainable = lambda xs, full: self.calls.append((name, ("stacks", full))) or out(xs)

    def set(self, pattern, switches):
        m = self.m
        m.train_decoders, m.train_fpn, m.train_body, m.train_stem = (c != "-" for c in switches)
        for k, p in self.named.items():
            p.requires_grad_(bool(self.patterns[pattern](k)))
        del self.calls[:]

    def backbone_call(self):
        (call,) = [c for who, c in self.calls if who == "backbone"]
        return call

    def heads_call(self):
        calls = dict((who, c) for who, c in self.calls if who != "backbone")
        assert sorted(calls) == sorted(HEADS) and len(self.calls) - len(calls) <= 1, self.calls
        (call,) = set(calls.values())                                # both heads are called the same way
        return call

    def forward(self, pattern, switches):
        """-> the exception's text, or (backbone call, heads' call, trainable_scope())."""
        self.set(pattern, switches)
        try:
            out = self.m(torch.zeros(1, 8, 3, 32, 32), [])
        except NotImplementedError as e:
            assert not self.calls
            return str(e)
        assert out == {"embeddings": (1, 2, 8, 1, 1), "semseg": (1, 8, 2, 1, 1)}
        scope = tuple(self.m.trainable_scope()) if hasattr(self.m, "trainable_scope") else None
        return self.backbone_call(), self.heads_call(), scope


@pytest.fixture(scope="module")
def harness():
    from stemseg_amd import config
    try:
        config.load_preset("kittimots")
        config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
        yield _Harness()
    finally:
        config.load_preset("defaults")


def _expected(outcome, h):
    if isinstance(outcome, str) or hasattr(h.m, "trainable_scope"):
        return outcome
    return outcome[:2] + (None,)                       # (a tree without trainable_scope(): the calls alone)


def test_the_matrix_is_complete():
    assert len(SWITCHES) == 16 and set(FORWARD) == set(PATTERNS) and all(sorted(row) == sorted(SWITCHES) for row in FORWARD.values())


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_forward_builds_the_graph_of_the_scope_or_refuses(harness, pattern):
    got = {s: harness.forward(pattern, s) for s in SWITCHES}
    assert got == {s: _expected(FORWARD[pattern][s], harness) for s in SWITCHES}


def test_no_graph_under_no_grad_and_a_cfg_frozen_backbone_runs_without_one(harness):
    from stemseg_amd import config
    for pattern, switches, no_grad, frozen, outcome in OTHER:
        config.cfg.TRAINING.FREEZE_BACKBONE = frozen
        try:
            with torch.no_grad() if no_grad else contextlib.nullcontext():
                got = harness.forward(pattern, switches)
        finally:
            config.cfg.TRAINING.FREEZE_BACKBONE = False
        assert got == _expected(outcome, harness), (pattern, switches, no_grad, frozen)


def test_run_backbone_on_its_own(harness):
    h, new = harness, hasattr(harness.m, "trainable_scope")
    x = torch.zeros(1, 8, 3, 32, 32)
    for pattern, switches, call in RUN_BACKBONE + [(p, s, after if new else before) for p, s, before, after in RUN_BACKBONE_OUTSIDE]:
        h.set(pattern, switches)
        feats = h.m.run_backbone(x)
        assert list(feats) == [4, 8, 16, 32] and h.calls == [("backbone", call)], (pattern, switches, h.calls)
    h.set("+layer2..4", "dfb-")
    with torch.no_grad():
        h.m.run_backbone(x)
    assert h.calls == [("backbone", "forward")]


def test_forward_embeddings_and_semseg_on_its_own(harness):
    h = harness
    feats = {s: torch.zeros(8, 1, 1, 1) for s in (4, 8, 16, 32)}
    for pattern, switches, call in HEADS_ALONE:
        h.set(pattern, switches)
        emb, sem = h.m.forward_embeddings_and_semseg(feats, 1, 8)
        assert (tuple(emb.shape), tuple(sem.shape), h.heads_call()) == ((1, 2, 8, 1, 1), (1, 8, 2, 1, 1), call), (pattern, switches, h.calls)
    h.set("+layer2..4", "dfb-")
    with torch.no_grad():
        h.m.forward_embeddings_and_semseg(feats, 1, 8)
    assert h.heads_call() == "plain"


def test_a_parameter_outside_every_group_is_refused_in_the_wording_of_the_switches(harness):
    """On an R-50 the body holds convolution weights only, so with train_stem everything can be trainable; a parameter that belongs to no group
    (here one hung on the model) brings out the train_stem wording."""
    h = harness
    h.m.extra = torch.nn.Parameter(torch.zeros(1))
    try:
        h.named["extra"], h.patterns["extra"] = h.m.extra, lambda k: k == "extra" or k.startswith("backbone.body.layer4.")
        assert h.forward("extra", "dfbs") == E_STEM % (1, "extra")
        assert h.forward("extra", "dfb-") == E_BODY % (1, "extra")
        assert h.forward("extra", "df--") == E_FPN % (11, "extra")           # (the model's own parameter comes first)
    finally:
        del h.m.extra, h.named["extra"], h.patterns["extra"]
