"""What the training loop asks of ``torch.distributed``, under the reference's names (utils/distributed.py): every function answers for
"no process group" as for a group of one rank, so single-process code calls them unconditionally.

``any_rank`` is this project's addition (the ranks agree on a signal).  ``all_gather`` and ``reduce_dict`` carry small host-side values
(logged scalars, picklable records); the gradient traffic of training does not go through here but through ``training.optim.GradBucket``.  Tensors travel on the device under nccl and through the host under any
other backend, so both run on a gloo group as well.
"""
import pickle

import torch
import torch.distributed as dist


def is_distributed():
    return dist.is_available() and dist.is_initialized()


def get_world_size():
    return dist.get_world_size() if is_distributed() else 1


def get_rank():
    return dist.get_rank() if is_distributed() else 0


def is_main_process():
    return get_rank() == 0


def get_device():
    """The reference's launcher contract: rank r computes on cuda:r."""
    return "cuda:%d" % get_rank()


def synchronize():
    """A barrier over the group; nothing for one rank."""
    if get_world_size() > 1:
        dist.barrier()


def any_rank(flag):
    """True on every rank when ``flag`` is true on at least one: one small all-reduce (a collective: every rank calls it at the same
    point).  With one rank, ``bool(flag)``."""
    if get_world_size() == 1:
        return bool(flag)
    seen = torch.tensor([1 if flag else 0], dtype=torch.int32, device=_wire_device())
    dist.all_reduce(seen, op=dist.ReduceOp.MAX)
    return bool(seen.item())


def _wire_device():
    return torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")


def all_gather(data):
    """data: any picklable object -> [rank 0's, rank 1's, ...] on every rank.  The pickles may differ in length: the lengths are gathered
    first and every payload is padded to the longest."""
    world = get_world_size()
    if world == 1:
        return [data]
    dev = _wire_device()
    payload = torch.frombuffer(bytearray(pickle.dumps(data)), dtype=torch.uint8).to(dev)
    sizes = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
    dist.all_gather(sizes, torch.tensor([payload.numel()], dtype=torch.int64, device=dev))
    sizes = [int(s.item()) for s in sizes]
    padded = torch.zeros(max(sizes), dtype=torch.uint8, device=dev)
    padded[:payload.numel()] = payload
    parts = [torch.empty_like(padded) for _ in range(world)]
    dist.all_gather(parts, padded)
    return [pickle.loads(part[:size].cpu().numpy().tobytes()) for size, part in zip(sizes, parts)]


def reduce_dict(input_dict, average=True):
    """input_dict: {name: scalar tensor} with the same names on every rank -> a dict of the same names, sorted, whose values on rank 0
    are the sums (``average``: the means) over the ranks.  The other ranks' values are unspecified, as ``dist.reduce`` leaves them.  With
    one rank the input comes back as it is."""
    world = get_world_size()
    if world < 2:
        return input_dict
    with torch.no_grad():
        names = sorted(input_dict)
        values = torch.stack([input_dict[k].detach().reshape(()) for k in names])
        home = values.device
        values = values.to(_wire_device())
        dist.reduce(values, dst=0)
        if dist.get_rank() == 0 and average:
            values /= world
        values = values.to(home)
        return {k: v for k, v in zip(names, values)}
