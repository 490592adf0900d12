"""``ConcatDataset`` and ``SparseDataset`` (the reference's data/concat_dataset.py): ``total_samples`` indices over several datasets, each
given its weight's share -- a dataset that is larger than its share is thinned by a fixed shuffle, one that is smaller is repeated and
topped up with evenly spaced indices."""
import math
import random

import torch
from torch.utils.data import Dataset


class SparseDataset(Dataset):
    """The first ``num_samples`` entries of a shuffle of ``dataset`` under ``random.seed(42)`` (which, as in the reference, re-seeds the
    global generator)."""

    def __init__(self, dataset, num_samples):
        assert num_samples < len(dataset), "SparseDataset is only applicable when num_samples < len(dataset)"
        self.dataset, self.num_samples = dataset, num_samples
        random.seed(42)
        self.idxes = list(range(len(dataset)))
        random.shuffle(self.idxes)

    def __len__(self):
        return self.num_samples

    def __getitem__(self, index):
        return self.dataset[self.idxes[index]]


class ConcatDataset(Dataset):
    def __init__(self, datasets, total_samples, weights=None):
        if weights is None:
            weights = [1.0 / len(datasets)] * len(datasets)
        assert abs(sum(weights) - 1.0) < 1e-6, "Sum of weights is {}. Should be 1".format(sum(weights))
        self.id_mapping, self.samples_per_dataset = [], []
        for i, (weight, ds) in enumerate(zip(weights, datasets)):
            assert 0.0 < weight <= 1.0
            share = int(round(weight * total_samples))
            if share < len(ds):
                ds = SparseDataset(ds, share)
            whole = int(math.floor(share / float(len(ds))))
            idxes = list(range(len(ds))) * whole
            idxes += torch.linspace(0, len(ds) - 1, share - len(idxes)).round().long().tolist()
            self.id_mapping.extend((i, j) for j in idxes)
            self.samples_per_dataset.append(share)
        self.datasets, self.weights = datasets, weights          # (the thinned view only fixed the indices: a sample is read from the dataset itself)
        assert len(self.id_mapping) == total_samples

    def __len__(self):
        return len(self.id_mapping)

    def __getitem__(self, index):
        ds, sample = self.id_mapping[index]
        return self.datasets[ds][sample]
