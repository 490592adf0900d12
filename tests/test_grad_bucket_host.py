"""Host side of data-parallel training (no GPU): the four gradient-bucket entry points of csrc/optimizer.hip through the C-ABI (exports,
argument errors, the layout rule against its restatement), ``stemseg_amd.utils.distributed`` on real gloo groups of 2 and 3 ranks on the CPU,
and the Trainer's rank bookkeeping on a monkeypatched group.

Every spawned group is initialised with a 120 s timeout, and the parent ends the remaining ranks as soon as one exits non-zero."""
import ctypes as C
import datetime
import os
import queue
import sys
from types import SimpleNamespace as NS

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.conftest import ROOT

SIZES = [0, 1, 3, 4, 5, 16383, 16384, 16385, 40000]
E = -1                                                                  # STEMSEG_E_INVALID
NAMES = ("stemseg_hip_opt_bucket_plan", "stemseg_hip_opt_pack_grads", "stemseg_hip_opt_unpack_grads", "stemseg_hip_opt_reduce_ranks")


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip
    hip.lib()
    return hip


# ------------------------------------------------------------------------------------------------ C-ABI
def test_the_four_symbols_are_exported_bound_and_declared(hip):
    header = open(os.path.join(ROOT, "include", "stemseg_hip.h")).read()
    raw = C.CDLL(hip.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n) and n in hip.SIGNATURES and n + "(" in header, n
    assert "#define STEMSEG_OPT_MAX_WORLD %d" % hip.OPT_MAX_WORLD in header and hip.OPT_MAX_WORLD == 64
    assert hip.lib().stemseg_hip_version() == 11 and "#define STEMSEG_HIP_ABI_VERSION 11" in header


def _restated(sizes):
    offsets, at = [], 0
    for n in sizes:
        offsets.append(at)
        at += -(-n // 4) * 4
    return offsets, at


def test_bucket_plan_is_the_layout_rule(hip):
    orders = [SIZES, SIZES[::-1], sorted(SIZES, key=lambda n: (n % 4, n)), [SIZES[i] for i in (4, 0, 8, 2, 6, 1, 7, 3, 5)], [0], [5], [0, 0, 3, 0]]
    for order in orders:
        offsets, total = hip.opt_bucket_plan(order)
        assert (offsets, total) == _restated(order), order
        assert all(o % 4 == 0 for o in offsets) and total % 4 == 0
        # every slice and its padding lie in [0, total), and no two slices share an element
        ends = [o + -(-n // 4) * 4 for o, n in zip(offsets, order)]
        assert all(a <= b for a, b in zip(ends, offsets[1:])) and ends[-1] == total
    # offsets_host NULL: the total alone
    t = (hip.OptTensor * 3)()
    for d, n in zip(t, (5, 0, 16385)):
        d.n = n
    total = C.c_int64(-7)
    assert hip.lib().stemseg_hip_opt_bucket_plan(t, 3, None, C.byref(total)) == 0 and total.value == 8 + 0 + 16388


def test_argument_errors_before_any_hip_call(hip):
    l = hip.lib()
    err = lambda: l.stemseg_hip_last_error()
    one = (hip.OptTensor * 1)()
    one[0].n = 8
    off, total = (C.c_int64 * 1)(), C.c_int64(0)
    plan = l.stemseg_hip_opt_bucket_plan
    assert plan(None, 1, off, C.byref(total)) == E and plan(one, 1, off, None) == E
    assert plan(one, 0, off, C.byref(total)) == E and b"n_tensors" in err()
    assert plan(one, -2, off, C.byref(total)) == E
    one[0].n = -1
    assert plan(one, 1, off, C.byref(total)) == E and b"negative" in err()
    one[0].n = 8
    assert plan(one, 1, off, C.byref(total)) == 0 and (off[0], total.value) == (0, 8)

    CH = hip.OPT_CHUNK
    t, c, o, b = 4096, 8192, 12288, 16384                               # never dereferenced: every call below fails its checks first
    pack = lambda *a, scale=1.0: l.stemseg_hip_opt_pack_grads(*(a + (scale, None)))
    unpack = lambda *a: l.stemseg_hip_opt_unpack_grads(*(a + (None,)))
    for fn in (pack, unpack):
        assert fn(None, 1, c, 1, o, b, 8) == E and b"null table" in err()
        assert fn(t, 1, None, 1, o, b, 8) == E
        assert fn(t, 1, c, 1, None, b, 8) == E and b"null offsets or bucket" in err()
        assert fn(t, 1, c, 1, o, None, 8) == E
        assert fn(t, 0, c, 1, o, b, 8) == E and b"n_tensors" in err()
        assert fn(t, 1, c, 0, o, b, 8) == E and b"n_chunks" in err()
        assert fn(t + 4, 1, c, 1, o, b, 8) == E and b"aligned" in err()
        assert fn(t, 1, c, 1, o + 4, b, 8) == E and b"offsets must be 8-byte aligned" in err()
        for misaligned in (b + 4, b + 8):
            assert fn(t, 1, c, 1, o, misaligned, 8) == E and b"16-byte aligned" in err()
        # a total that cannot be the plan's: not a multiple of 4, not positive, more than the chunks hold, no more than fewer chunks would hold
        for n_tensors, n_chunks, bad in ((1, 1, 7), (1, 1, 0), (1, 1, -8), (1, 1, CH + 4), (1, 3, 2 * CH), (2, 5, 3 * CH)):
            assert fn(t, n_tensors, c, n_chunks, o, b, bad) == E and b"total" in err(), (n_tensors, n_chunks, bad)
    for scale in (float("inf"), float("-inf"), float("nan")):
        assert pack(t, 1, c, 1, o, b, 8, scale=scale) == E and b"not finite" in err()

    red = lambda g, world, total, bucket: l.stemseg_hip_opt_reduce_ranks(g, world, total, bucket, None)
    far = 1 << 30
    assert red(None, 2, 8, far) == E and red(b, 2, 8, None) == E and b"null pointer" in err()
    for world in (0, -1, 65):
        assert red(b, world, 8, far) == E and b"world" in err()
    assert red(b, 2, 0, far) == E and red(b, 2, -4, far) == E and b"total" in err()
    assert red(b + 2, 2, 8, far) == E and red(b, 2, 8, far + 1) == E and b"aligned" in err()
    assert red(b, 2, 8, b + 32) == E and b"inside" in err()             # the second rank's row
    # the wrapper holds the plan and asks for its total exactly
    tables = NS(total=16, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="plan's total is 16"):
        hip._bucket_args(tables, torch.zeros(12))


# ------------------------------------------------------------------------------------------------ utils.distributed on gloo
def _gloo_worker(rank, world, store, case, q):
    for p in (ROOT, os.path.join(ROOT, "stem-seg_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    dist.init_process_group("gloo", init_method="file://" + store, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    try:
        q.put((rank, globals()["_case_" + case](rank, world)))
    finally:
        dist.destroy_process_group()


def _spawn(world, case, store):
    """-> the ranks' results in rank order.  The ranks meet through the file ``store`` (no port to collide on); the first rank to exit
    non-zero ends the others and fails the test."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, str(store), case, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = []
    try:
        while len(got) < world:
            try:
                got.append(q.get(timeout=0.25))
            except queue.Empty:
                failed = [r for r, p in enumerate(procs) if p.exitcode not in (None, 0)]
                assert not failed, "rank %s exited with %s" % (failed, [procs[r].exitcode for r in failed])
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    return [r[1] for r in sorted(got)]


def _case_distributed(rank, world):
    from stemseg_amd.utils import distributed as D
    basics = (D.is_distributed(), D.get_world_size(), D.get_rank(), D.is_main_process(), D.get_device())
    # values exact in binary, so that the mean is exact whatever the order of the additions
    losses = {"zeta": torch.tensor(float(rank + 1)), "alpha": torch.tensor(0.25 * (rank + 1)), "mid": torch.tensor(-2.0 * rank)}
    mean = D.reduce_dict(dict(losses))
    total = D.reduce_dict(dict(losses), average=False)
    gathered = D.all_gather({"rank": rank, "payload": "x" * (1 + 1000 * rank)})             # pickles of unequal length
    D.synchronize()
    agreed = (D.any_rank(rank == world - 1), D.any_rank(False))            # a signal on the last rank alone; on none
    return dict(agreed=agreed, basics=basics, keys=list(mean), mean={k: float(v) for k, v in mean.items()}, total={k: float(v) for k, v in total.items()},
                gathered=gathered)


@pytest.mark.parametrize("world", [2, 3])
def test_utils_distributed_on_a_gloo_group(world, tmp_path):
    res = _spawn(world, "distributed", tmp_path / "rendezvous")
    ranks = range(world)
    for r, out in enumerate(res):
        assert out["basics"] == (True, world, r, r == 0, "cuda:%d" % r)
        assert out["agreed"] == (True, False)
        assert out["keys"] == ["alpha", "mid", "zeta"]                                       # sorted, the same on every rank
        assert out["gathered"] == [{"rank": k, "payload": "x" * (1 + 1000 * k)} for k in ranks]
    sums = {"alpha": sum(0.25 * (k + 1) for k in ranks), "mid": sum(-2.0 * k for k in ranks), "zeta": float(sum(k + 1 for k in ranks))}
    assert res[0]["total"] == sums
    assert res[0]["mean"] == {k: float(torch.tensor(v) / world) for k, v in sums.items()}
    # the average is taken on rank 0 only: the other ranks never divide
    for out in res[1:]:
        assert all(out["mean"][k] == out["total"][k] for k in sums)


def test_utils_distributed_without_a_group():
    from stemseg_amd.utils import distributed as D
    assert (D.is_distributed(), D.get_world_size(), D.get_rank(), D.is_main_process(), D.get_device()) == (False, 1, 0, True, "cuda:0")
    d = {"a": torch.tensor(1.0)}
    assert D.reduce_dict(d) is d and D.all_gather("x") == ["x"]
    D.synchronize()
    assert D.any_rank(True) is True and D.any_rank(0) is False


# ------------------------------------------------------------------------------------------------ the Trainer's rank bookkeeping
class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(3))

    def forward(self, image_seqs, targets):
        from stemseg_amd.utils.constants import Loss, ModelOutput
        return {ModelOutput.OPTIMIZATION_LOSSES: {Loss.EMBEDDING: (self.w * image_seqs).sum()}, ModelOutput.OTHERS: {}}


class _StubBucket(object):
    MODES = ("allreduce", "ordered")

    def __init__(self, named_parameters, process_group=None, mode="allreduce"):
        self.names, self.mode, self.calls = [k for k, _ in named_parameters], mode, []

    def reduce(self):
        self.calls.append("reduce")

    def broadcast_parameters(self, src=0, buffers=()):
        self.calls.append(("broadcast", src, len(list(buffers))))


def _fake_group(monkeypatch, rank, world):
    """A process group that exists only as answers to the questions the Trainer asks, on the CPU, around a one-parameter model.
    -> (TRAINING cfg, the list of collectives the Trainer asked for)."""
    from stemseg_amd import config
    from stemseg_amd.training import main
    from stemseg_amd.utils import distributed as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: world)
    monkeypatch.setattr(dist, "get_rank", lambda *a: rank)
    seen = []
    monkeypatch.setattr(D, "reduce_dict", lambda d, average=True: (seen.append("reduce_dict"), d)[1])
    monkeypatch.setattr(D, "synchronize", lambda: seen.append("synchronize"))
    monkeypatch.setattr(D, "any_rank", lambda flag: (seen.append("any_rank"), bool(flag))[1])
    monkeypatch.setattr(main, "GradBucket", _StubBucket)
    monkeypatch.setattr(main, "configure_trainable", lambda model, freeze_backbone=None: model)
    monkeypatch.setattr(main, "create_optimizer", lambda model, cfg, log, device_step=True: torch.optim.SGD(model.parameters(), lr=0.5))
    monkeypatch.setattr(main, "create_lr_scheduler", lambda opt, cfg, log: torch.optim.lr_scheduler.LambdaLR(opt, lambda it: 1.0))
    cfg = NS(**vars(config.make_cfg().TRAINING))
    cfg.BATCH_SIZE, cfg.MAX_SAMPLES_PER_GPU, cfg.ACCUMULATE_GRADIENTS, cfg.MAX_ITERATIONS, cfg.CLIP_GRADIENTS = 4, 1, True, 1000, False
    return cfg, seen


def _fake_trainer(monkeypatch, tmp_path, rank, world, **kw):
    from stemseg_amd.training import main
    cfg, seen = _fake_group(monkeypatch, rank, world)
    said = []
    t = main.Trainer(cfg, str(tmp_path / ("rank%d" % rank)), NS(restore_session=None, initial_ckpt=None), NS(info=said.append, debug=said.append),
                     model=_Tiny(), **kw)
    return t, seen, said


@pytest.mark.parametrize("rank", [0, 1])
def test_trainer_rank_bookkeeping_on_a_two_rank_group(monkeypatch, tmp_path, rank):
    t, seen, said = _fake_trainer(monkeypatch, tmp_path, rank, 2, data_parallel=True, reduce_mode="ordered")
    assert (t.num_gpus, t.local_rank, t.is_main_process) == (2, rank, rank == 0)
    assert t.bucket.mode == "ordered" and t.bucket.names == ["w"] and t.bucket.calls == [("broadcast", 0, 0)]
    # batch 4 at one sample per GPU: 4 sub-iterations on one GPU, 2 on each of two -> four batches are two steps
    t.data_loader = [(torch.full((3,), float(k)), [{}], [{}]) for k in range(4)]
    t.start(NS(save_interval=2, display_interval=1, summary_interval=1, ckpts_to_keep=1))
    assert t.elapsed_iterations == 2 and t.bucket.calls[1:] == ["reduce", "reduce"]
    # w = 1 - 0.5 * mean over the step's two batches, twice: (0 + 1) / 2 and (2 + 3) / 2
    assert torch.equal(t.model.w.detach(), torch.full((3,), 1.0 - 0.5 * 0.5 - 0.5 * 2.5))
    # per step the means and the ranks' agreement on a signal; the two barriers around the one regular checkpoint
    assert seen == ["reduce_dict", "any_rank", "reduce_dict", "synchronize", "synchronize", "any_rank"]
    here = tmp_path / ("rank%d" % rank)
    if rank == 0:
        assert sorted(os.listdir(here)) == ["000002.pth", "logs"] and t.logger.last_point["iteration"] == 2
    else:
        assert not here.exists() and t.logger is None, "a rank other than 0 wrote a file"
        assert t.backup_session() is None


class _FailingLoader(object):
    """Two good batches (one step at two ranks), then the error of a rank that meets a bad sample."""

    def __iter__(self):
        for k in range(2):
            yield torch.full((3,), float(k)), [{}], [{}]
        raise RuntimeError("bad sample")


@pytest.mark.parametrize("rank", [0, 1])
def test_a_failing_rank_saves_without_any_collective(monkeypatch, tmp_path, rank):
    """The other ranks may be anywhere when one rank fails, inside the gradient reduction included: the failure path of ``start`` runs no
    barrier and no other collective; rank 0 writes its emergency checkpoint alone, any other rank writes nothing, and the error itself
    travels on."""
    from stemseg_amd.training import main
    cfg, seen = _fake_group(monkeypatch, rank, 2)
    monkeypatch.setenv("STEMSEG_MODELS_DIR", str(tmp_path))
    monkeypatch.setattr(main, "build_model", lambda **kw: _Tiny())
    args = main.build_parser().parse_args(["--model_dir", "run", "--cfg", "kittimots", "--save_interval", "1000", "--log_level", "off"])
    with pytest.raises(RuntimeError, match="bad sample"):
        main.start(args, cfg, _FailingLoader(), data_parallel=True)
    assert seen == ["reduce_dict", "any_rank"], seen                   # the one completed step; nothing after the error
    files = sorted(f for f in os.listdir(tmp_path / "checkpoints" / cfg.MODE / "run") if f.endswith(".pth"))
    assert files == (["000001.pth"] if rank == 0 else [])


@pytest.mark.parametrize("rank", [0, 1])
def test_a_signal_ends_every_rank_at_the_same_step(monkeypatch, tmp_path, rank):
    """A signal seen by another rank (``any_rank`` answers True) ends this rank at the step too; one seen here between sub-iterations
    waits for the step, where the ranks look together."""
    from stemseg_amd.training import main
    from stemseg_amd.utils import distributed as D
    t, seen, _ = _fake_trainer(monkeypatch, tmp_path, rank, 2, data_parallel=True)
    monkeypatch.setattr(D, "any_rank", lambda flag: (seen.append(("any_rank", bool(flag))), True)[1])
    t.data_loader = [(torch.full((3,), float(k)), [{}], [{}]) for k in range(4)]
    with pytest.raises(main.InterruptException):
        t.start(NS(save_interval=1000, display_interval=1, summary_interval=1, ckpts_to_keep=1))
    assert t.elapsed_iterations == 1 and seen == ["reduce_dict", ("any_rank", False)]
    # the local flag alone: no exit between the sub-iterations of a step
    t2, seen2, _ = _fake_trainer(monkeypatch, tmp_path / "second", rank, 2, data_parallel=True)

    class Raised(object):
        is_interrupted = True
        start = stop = staticmethod(lambda: None)
    t2.interrupt_detector = Raised()
    t2.data_loader = [(torch.full((3,), float(k)), [{}], [{}]) for k in range(4)]
    with pytest.raises(main.InterruptException):
        t2.start(NS(save_interval=1000, display_interval=1, summary_interval=1, ckpts_to_keep=1))
    assert t2.elapsed_iterations == 1 and t2.bucket.calls[1:] == ["reduce"] and seen2 == ["reduce_dict", "any_rank"]


def test_trainer_keeps_its_refusal_and_names_the_switch(monkeypatch, tmp_path):
    with pytest.raises(NotImplementedError, match="3 ranks.*data_parallel=True"):
        _fake_trainer(monkeypatch, tmp_path, 0, 3)
    with pytest.raises(ValueError, match="reduce_mode"):
        _fake_trainer(monkeypatch, tmp_path, 0, 3, data_parallel=True, reduce_mode="ring")


def test_main_ignores_allow_multigpu_on_one_device(monkeypatch):
    """As in the reference: with one visible device the flag starts no process group."""
    from stemseg_amd import config
    from stemseg_amd.training import main
    called = []
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    monkeypatch.setattr(main, "init_distributed", lambda *a: called.append("init"))
    monkeypatch.setattr(main, "start", lambda args, cfg, data_loader=None, data_parallel=False: called.append(data_parallel))
    try:
        main.main(main.build_parser().parse_args(["--model_dir", "x", "--cfg", "kittimots", "--allow_multigpu"]))
        assert called == [False]
        monkeypatch.setattr(torch.cuda, "device_count", lambda: 4)
        monkeypatch.setattr(dist, "destroy_process_group", lambda *a: called.append("destroy"))
        main.main(main.build_parser().parse_args(["--model_dir", "x", "--cfg", "kittimots", "--allow_multigpu", "--local_rank", "2"]))
        assert called == [False, "init", True, "destroy"]
    finally:
        config.load_preset("defaults")
