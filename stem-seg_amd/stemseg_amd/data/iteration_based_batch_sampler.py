"""``IterationBasedBatchSampler`` (the reference's data/iteration_based_batch_sampler.py): runs over a batch sampler again and again until
``num_iterations`` batches are out, counting from ``start_iter`` -- how a resumed session skips what it has already seen."""
from torch.utils.data.sampler import BatchSampler


class IterationBasedBatchSampler(BatchSampler):
    def __init__(self, batch_sampler, num_iterations, start_iter=0):
        self.batch_sampler = batch_sampler
        self.num_iterations = num_iterations
        self.start_iter = start_iter

    def __iter__(self):
        done = self.start_iter
        while done <= self.num_iterations:
            sampler = self.batch_sampler.sampler
            if hasattr(sampler, "set_epoch"):          # (a DistributedSampler: another permutation for every pass)
                sampler.set_epoch(done)
            for batch in self.batch_sampler:
                done += 1
                if done > self.num_iterations:
                    return
                yield batch

    def __len__(self):
        return self.num_iterations
