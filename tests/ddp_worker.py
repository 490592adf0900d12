"""Worker of tests/test_gpu_ddp.py (run as a script, one process per rank): ``GradBucket`` and the data-parallel ``Trainer`` on a real
process group.  Rank, world size and rendezvous come from the environment (RANK, WORLD_SIZE, MASTER_ADDR, MASTER_PORT); under gloo every
rank computes on device 0, under nccl rank r on device r.  Tensors are written with ``torch.save`` into --out for the parent to compare on
the CPU; the worker itself asserts nothing but what only it can see."""
import argparse
import datetime
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "stem-seg_amd")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

SIZES = [0, 1, 3, 4, 5, 16383, 16384, 16385, 40000]
ABSENT_ON_RANK_1 = 6            # the synthetic parameter that has no gradient on rank 1 only
MODES = ("allreduce", "ordered")
PERTURB = 1e-3                  # rank r starts the Trainer legs from weights moved by r * PERTURB


def synthetic_grads(rank):
    """Normal-range values, 1e-4 .. 1e2 in magnitude, either sign; the parent restates them from the rank."""
    rng = np.random.default_rng(100 + rank)
    return [(10.0 ** rng.uniform(-4, 2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32) for n in SIZES]


def synthetic_params():
    rng = np.random.default_rng(5)
    return [rng.standard_normal(n).astype(np.float32) for n in SIZES]


def _synthetic_model(rank, absent=True):
    params = [torch.nn.Parameter(torch.from_numpy(v).cuda()) for v in synthetic_params()]
    for i, (p, g) in enumerate(zip(params, synthetic_grads(rank))):
        p.grad = None if (absent and rank == 1 and i == ABSENT_ON_RANK_1) else torch.from_numpy(g).cuda()
    return params


def case_synthetic(rank, world, out):
    from stemseg_amd.training import GradBucket
    for mode in MODES:
        params = _synthetic_model(rank)
        bucket = GradBucket([("t%d" % i, p) for i, p in enumerate(params)], mode=mode)
        assert bucket.world == world
        bucket.reduce()
        views = all(p.grad.numel() == 0 or p.grad.data_ptr() == bucket.bucket.data_ptr() + 4 * o for p, o in zip(params, bucket.offsets))
        torch.save({"bucket": bucket.bucket.cpu(), "offsets": bucket.offsets, "views": views}, os.path.join(out, "synthetic_%s_rank%d.pt" % (mode, rank)))


def case_world1(rank, world, out):
    """A group of one rank: the collectives run, the result is the local bits, and the step from the bucket is the step without a group."""
    from stemseg_amd.training import DeviceSGD, GradBucket
    res = {"backend": dist.get_backend()}
    plain = _synthetic_model(0, absent=False)
    DeviceSGD(plain, lr=0.1, momentum=0.9, nesterov=True).step()
    for mode in MODES:
        params = _synthetic_model(0, absent=False)
        bucket = GradBucket([("t%d" % i, p) for i, p in enumerate(params)], mode=mode)
        bucket.reduce()
        res[mode + "_bucket"], res[mode + "_offsets"] = bucket.bucket.cpu(), bucket.offsets
        res[mode + "_gathered"] = None if bucket.gathered is None else tuple(bucket.gathered.shape)
        DeviceSGD(params, lr=0.1, momentum=0.9, nesterov=True).step()
        torch.cuda.synchronize()
        res[mode + "_step_equal"] = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(params, plain))
    torch.save(res, os.path.join(out, "world1.pt"))


def _perturbed(initial, rank):
    return {k: (v + rank * PERTURB if v.is_floating_point() else v.clone()) for k, v in initial.items()}


def digest(named):
    """{name: SHA-256 of the tensor's bytes}: equal digests are equal bits, at a thousandth of the size."""
    return {k: hashlib.sha256(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest() for k, v in named.items()}


def case_trainer(rank, world, out):
    """World 2 on the kittimots R-50 model and the two batches of tests/test_gpu_trainer.py: batch size 2 at one sample per GPU is one
    sub-iteration per step, rank r trains on batch r.  Per mode one Trainer and one step; under "allreduce" also the second step of the
    same Trainer, the same step after a resume from rank 0's checkpoint, and one clipped step.  Written in full: what the parent computes
    with (the local gradients, and on rank 0 the reduced gradients and the parameters after the step); everything that is only compared
    for equal bits travels as SHA-256 digests."""
    from tests import test_gpu_trainer as TT
    from tests.test_gpu_body_backward import _inputs
    with TT._preset("kittimots"):
        m0 = TT._build()
        frames, raw = _inputs(m0, 8, 96, 128)
        initial = {k: v.detach().cpu().clone() for k, v in m0.state_dict().items()}
        del m0
        items = [TT._two_batches(frames, raw)[rank]]
        opts = argparse.Namespace(**dict(vars(TT.OPTS), save_interval=1))

        def trainer(tag, mode, **kw):
            model = TT._build(_perturbed(initial, rank))
            tr = TT._trainer(os.path.join(out, "rank%d" % rank, tag), model, TT._training_cfg(**kw.pop("cfg", {})), data_parallel=True, reduce_mode=mode, **kw)
            local, inner = [], tr.bucket.reduce

            def reduce():
                local.append({k: p.grad.detach().cpu().clone() for k, p in model.named_parameters() if p.grad is not None})
                inner()
            tr.bucket.reduce = reduce
            return tr, model, local, TT.Snapshot(tr)

        def run(tr):
            tr.data_loader = TT.Batches(items)
            tr.start(opts)
            torch.cuda.synchronize()

        res = {"initial": digest(initial), "rank": rank}
        clock = time.monotonic()
        for mode in MODES:
            tr, model, local, snap = trainer(mode, mode)
            res[mode] = leg = {"constructed": digest(model.state_dict()), "num_gpus": tr.num_gpus, "main": tr.is_main_process}
            run(tr)
            before = snap.taken[0]
            reduced, after = {k: v[1] for k, v in before.items() if v[1] is not None}, TT._named(model)
            leg["before"], leg["local_digest"], leg["reduced_digest"], leg["after_digest"] = (
                digest({k: v[0] for k, v in before.items()}), digest(local[0]), digest(reduced), digest(after))
            leg["iterations"], leg["reductions"] = tr.elapsed_iterations, len(local)
            if mode == "allreduce":
                leg["local"] = local[0]
            if rank == 0:
                leg["reduced"], leg["after"] = reduced, after
            print("DDP_WORKER rank %d: %s leg built, stepped and digested after %.1f s" % (rank, mode, time.monotonic() - clock))
            if mode != "allreduce":
                continue
            run(tr)                                                                        # the uninterrupted second step
            leg["after_second"], leg["iterations_second"] = digest(TT._named(model)), tr.elapsed_iterations
            ckpt = os.path.join(out, "rank0", mode, "000001.pth")                            # rank 0's, read by every rank
            tr2, model2, _, _ = trainer("resumed", mode, restore=ckpt)
            leg["resumed_iterations"] = tr2.elapsed_iterations
            run(tr2)
            leg["resumed_after_second"] = digest(TT._named(model2))
            trc, modelc, _, _ = trainer("clip", mode, cfg=dict(CLIP_GRADIENTS=True), max_norm=0.01)
            run(trc)
            leg["clip_norm"], leg["clip_after"] = trc.last_grad_norm.cpu(), digest(TT._named(modelc))
        print("DDP_WORKER rank %d: all legs after %.1f s" % (rank, time.monotonic() - clock))
        torch.save(res, os.path.join(out, "trainer_rank%d.pt" % rank))
        print("DDP_WORKER rank %d: results written after %.1f s" % (rank, time.monotonic() - clock))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True, choices=("synthetic", "world1", "trainer"))
    ap.add_argument("--backend", required=True, choices=("gloo", "nccl"))
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    from stemseg_amd import hip
    hip.require_gpu()
    rank, world, began = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), time.monotonic()
    device = rank if (a.backend == "nccl" and world > 1) else 0
    torch.cuda.set_device(device)
    kw = dict(device_id=torch.device("cuda", device)) if a.backend == "nccl" else {}
    dist.init_process_group(a.backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120), **kw)
    try:
        globals()["case_" + a.case](rank, world, a.out)
        torch.cuda.synchronize()
        dist.barrier()
    finally:
        dist.destroy_process_group()
    print("DDP_WORKER rank %d: done %.1f s after the imports" % (rank, time.monotonic() - began))


if __name__ == "__main__":
    main()
