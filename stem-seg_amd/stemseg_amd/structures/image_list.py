"""``ImageList`` under the reference's name (structures/image_list.py): a batch of clips zero-padded to one size that is a multiple of 32,
with every clip's size before the padding.  ``TrainingModel`` reads ``.tensors``; ``resize_masks`` reads ``max_size``."""
import math

import torch


class ImageList(object):
    def __init__(self, images_tensor, image_sizes, original_image_sizes=None):
        self.tensors = images_tensor                                  # [N, T, C, H, W]
        self.image_sizes = image_sizes                                # per clip (H, W) before the padding
        self.original_image_sizes = original_image_sizes              # per clip (W, H) of the files

    def to(self, *args, **kwargs):
        return type(self)(self.tensors.to(*args, **kwargs), self.image_sizes, self.original_image_sizes)

    def cuda(self):
        return type(self)(self.tensors.cuda(), self.image_sizes, self.original_image_sizes)

    def __len__(self):
        return self.num_seqs

    def __getitem__(self, index):
        return self.tensors[index]

    @property
    def num_seqs(self):
        return self.tensors.shape[0]

    @property
    def num_frames(self):
        return self.tensors.shape[1]

    @property
    def max_size(self):
        return self.tensors.shape[-2:]                                # (H, W) of the padded batch

    @staticmethod
    def padded_size(image_sizes):
        """(H, W) of the batch: the largest height and width, each rounded up to a multiple of 32."""
        return tuple(int(math.ceil(max(s[d] for s in image_sizes) / 32)) * 32 for d in (0, 1))

    @classmethod
    def from_image_sequence_list(cls, image_sequence_list, original_dims=None):
        """N clips, each a tensor [T, C, H_n, W_n] or T tensors [C, H_n, W_n] of one size -> the zero-padded batch."""
        clips = [c if torch.is_tensor(c) else torch.stack(list(c), 0) for c in image_sequence_list]
        lengths = sorted(set(c.shape[0] for c in clips))
        if len(lengths) != 1:
            raise ValueError("All sequences must contain the same number of images. Found {} and {}".format(lengths[0], lengths[1]))
        sizes = [tuple(c.shape[-2:]) for c in clips]
        ph, pw = cls.padded_size(sizes)
        batch = torch.zeros((len(clips), lengths[0], clips[0].shape[1], ph, pw), dtype=clips[0].dtype, device=clips[0].device)
        for n, (c, (h, w)) in enumerate(zip(clips, sizes)):
            batch[n, :, :, :h, :w] = c
        return cls(batch, sizes, original_dims)
