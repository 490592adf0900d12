"""``DistributedSampler`` (the reference's data/distributed_data_sampler.py, itself torch's of that time): every rank gets
ceil(len / world) indices of one permutation that all ranks share -- seeded by the epoch -- the first indices repeated to fill up."""
import math

import torch
import torch.distributed as dist
from torch.utils.data.sampler import Sampler


class DistributedSampler(Sampler):
    def __init__(self, dataset, num_replicas=None, rank=None, shuffle=True):
        if (num_replicas is None or rank is None) and not dist.is_available():
            raise RuntimeError("Requires distributed package to be available")
        self.dataset = dataset
        self.num_replicas = dist.get_world_size() if num_replicas is None else num_replicas
        self.rank = dist.get_rank() if rank is None else rank
        self.epoch = 0
        self.shuffle = shuffle
        self.num_samples = int(math.ceil(len(dataset) / float(self.num_replicas)))
        self.total_size = self.num_samples * self.num_replicas

    def __iter__(self):
        n = len(self.dataset)
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.epoch)
            order = torch.randperm(n, generator=g).tolist()
        else:
            order = list(range(n))
        order += order[:self.total_size - n]
        assert len(order) == self.total_size
        first = self.rank * self.num_samples
        return iter(order[first:first + self.num_samples])

    def __len__(self):
        return self.num_samples

    def set_epoch(self, epoch):
        self.epoch = epoch
