"""Discretisation: estimated masks (or an explicit_vad activity) -> the segment table of the segment-wise beamformer.
This project's own step between the two halves (the reference's evaluation scripts are not part of its tree): threshold,
closing by dilation and erosion, runs, minimum length -- DESIGN 4.13; csrc/segments.hip through hip_ops.

    table = ActivitySegmenter(threshold=0.5, dilation=81, erosion=41, min_frames=8)(model(ex).mask[0])
    enh = ClassicBF_np()(masks, Observation, table, numpy_out=True)
"""
import torch

from .. import hip_ops as H
from ..configurable import Configurable


class ActivitySegmenter(Configurable):
    """masks [K, M, T, F] (mask index 0 is averaged over F) or an activity [K, T] (the vad_mask of an explicit_vad
    estimator; skips the averaging) -> int32 [S, 3] rows (speaker, start, end) on the device, sorted by speaker then
    start.  The defaults are neutral (no smoothing): the project claims no tuned values."""

    def __init__(self, threshold=0.5, dilation=1, erosion=1, min_frames=1):
        super().__init__()
        H.check_segment_params(dilation, erosion, min_frames)
        self.threshold = threshold
        self.dilation = dilation
        self.erosion = erosion
        self.min_frames = min_frames

    def activity(self, masks_or_activity):
        x = masks_or_activity
        if not isinstance(x, torch.Tensor) or x.dim() not in (2, 4):
            raise ValueError(f"masks [K, M, T, F] or an activity [K, T], got "
                             f"{tuple(x.shape) if hasattr(x, 'shape') else type(x)}")
        x = x.detach()
        if not x.is_cuda:
            x = x.to("cuda")
        if x.dim() == 4:
            return H.mask_activity(x)
        return x.to(torch.float32)

    def __call__(self, masks_or_activity, return_count=False):
        """One host synchronisation (the count becomes the table's length); return_count=True: (buffer, count), none."""
        return H.activity_segments(self.activity(masks_or_activity), self.threshold, self.dilation, self.erosion,
                                   self.min_frames, return_count=return_count)

    @staticmethod
    def intervals(table, K):
        """table -> per speaker a list of (s, e): a host read, for code that wants `dia` in the old form."""
        out = [[] for _ in range(K)]
        for k, s, e in table.cpu().tolist():
            out[k].append((s, e))
        return out
