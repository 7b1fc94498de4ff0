"""Distortion masks of the eval-time beamformer -- drop-in for tssep/train/enhancer_distortion_mask.py.
Config objects: ``ClassicBF_np`` recognises them by type and hands a mode and an eps to the
segment-wise MVDR kernels, which form the distortion mask on the fly (csrc/mvdr.hip).  The numpy
``__call__`` is for standalone use; layout ``[mask, spk, ...]`` with one mask in, two out."""
import numpy as np


class OneMinus:
    """distortion = max(1 - mask, 0); one speaker."""
    kernel_mode = "one_minus"
    eps = 0.0

    def __call__(self, masks):
        assert masks.shape[0] == 1, masks.shape
        return np.concatenate([masks, np.maximum(1 - masks, 0)], axis=0)


class SumCrossTalker:
    """distortion of speaker k = max(sum of the other speakers' masks, eps)."""
    kernel_mode = "sum_cross_talker"

    def __init__(self, eps=0.0001):
        self.eps = eps

    def __call__(self, masks):
        assert masks.shape[0] == 1, masks.shape
        speakers = masks.shape[1]
        others = np.stack([np.sum(np.delete(masks, spk, axis=1), axis=1) for spk in range(speakers)], axis=1)
        return np.concatenate([masks, np.maximum(others, self.eps)], axis=0)
