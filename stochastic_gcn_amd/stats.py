"""Running statistics of the --gradvar bias / variance study (gcn/stats.py, gcn/train.py:241-276), kept on the device.

The reference's ``Stat`` appends every draw to a host list and reduces the list with np.mean / np.std (axis 0) at the
end: for S-Reddit's first layer (1204 x 128 floats) 1000 draws are ~616 MB per Stat, and every draw costs a
device-to-host copy and a synchronisation.  ``DeviceStat`` folds each draw into a running fp64 mean and sum of squared
deviations on the device instead (sgcn_moments_add_f32: one launch per draw, nothing on the host), and ``summary`` brings
the study's scalars back from one fixed-order reduction (sgcn_moments_summary_f64) and one 24-byte copy.
"""
import numpy as np
import torch

from . import ops


class DeviceStat(object):
    """``Stat`` of gcn/stats.py: ``add(v)``, ``mean()``, ``std()`` (np.std, ddof 0) and ``count``.

    ``add`` takes an fp32 device tensor, or a pair / list of equally shaped ones (a (mean, variance) prediction), kept
    stacked as np.mean(Stat.vals, axis=0) sees them.  Every later sample must have the first one's size.  ``mean()`` and
    ``std()`` are host fp64 arrays of the first sample's shape; the running state itself is ``mean_dev`` / ``m2_dev``."""

    def __init__(self):
        self.count = 0
        self.shape = None
        self.mean_dev = self.m2_dev = None

    def add(self, v):
        stacked = isinstance(v, (tuple, list))
        parts = list(v) if stacked else [v]
        if not parts or not all(isinstance(p, torch.Tensor) for p in parts):
            raise TypeError("DeviceStat.add takes a device tensor or a list of them")
        for p in parts:
            ops._flat(p, "sample")          # fp32, contiguous, in HBM
        k = int(parts[0].numel())
        if any(tuple(p.shape) != tuple(parts[0].shape) for p in parts):
            raise ValueError("DeviceStat.add: the parts of a stacked sample differ in shape")
        if k == 0:
            raise ValueError("DeviceStat.add: empty sample")
        n = k * len(parts)
        if self.mean_dev is None:
            self.mean_dev = torch.empty(n, dtype=torch.float64, device=parts[0].device)
            self.m2_dev = torch.empty_like(self.mean_dev)
            self.shape = ((len(parts),) if stacked else ()) + tuple(parts[0].shape)
        elif n != int(self.mean_dev.numel()):
            raise ValueError("DeviceStat.add: a sample of %d elements after samples of %d" % (n, self.mean_dev.numel()))
        for j, p in enumerate(parts):
            ops.moments_add(p, self.count, self.mean_dev[j * k:(j + 1) * k], self.m2_dev[j * k:(j + 1) * k])
        self.count += 1

    def _need(self):
        if self.count == 0:
            raise ValueError("DeviceStat: no samples")

    def mean(self):
        self._need()
        return self.mean_dev.cpu().numpy().reshape(self.shape)

    def std(self):
        self._need()
        return np.sqrt(self.m2_dev.cpu().numpy() / self.count).reshape(self.shape)


def summary(stat_a, stat_b=None):
    """(mean |a.mean()|, mean a.std(), mean |a.mean() - b.mean()|) -- the np.mean(...) scalars gcn/train.py:256-275
    prints -- as Python floats, from one reduction on the device and one copy.  The third is 0.0 without ``stat_b``."""
    stat_a._need()
    if stat_b is not None:
        stat_b._need()
        if stat_b.mean_dev.numel() != stat_a.mean_dev.numel():
            raise ValueError("summary: the two statistics differ in size")
    out = ops.moments_summary(stat_a.mean_dev, stat_a.m2_dev, stat_a.count,
                              None if stat_b is None else stat_b.mean_dev)
    a, s, b = out.cpu().tolist()
    return a, s, b
