"""What the per-env accumulators share on the host (EpisodeStats, HealthStats, ValueProbe, Timeline,
SpatialMaps): the tensor and layout-row checks of their constructors and calls, the decoding of
reduced rows, and the slice of an owner's envs (csrc/evx_reduce.h is the device side's share).
"""
from __future__ import annotations

import torch

from .env import _ptr


def need(name, t, n, dtype, device):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: a tensor is needed, not {type(t).__name__}")
    if t.dtype != dtype or t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{name}: needs {n} contiguous {dtype} elements, got {t.numel()} of {t.dtype}")
    if device is not None and t.device != device:
        raise ValueError(f"{name}: on {t.device}, the statistics are on {device}")


def check_rows(who, E, n_layouts, layout_idx, device, where="the statistics are") -> torch.device:
    """The layout-row arguments of a constructor: n_layouts rows (plus "all") over E envs whose
    layouts are layout_idx (int32 [E], or None with one layout) on ``device``, which is returned as
    a torch.device. Nothing is allocated."""
    if not 1 <= n_layouts <= 65535:
        raise ValueError(f"{who}: n_layouts must be 1..65535, not {n_layouts}")
    if n_layouts > 1 and layout_idx is None:
        raise ValueError(f"{who}: several layouts need layout_idx")
    device = torch.device(device)
    if layout_idx is not None:
        need("layout_idx", layout_idx, E, torch.int32, None)
        if layout_idx.device.type != device.type:
            raise ValueError(f"layout_idx: on {layout_idx.device}, {where} on {device}")
    return device


def as_mask(mask, E, device):
    """An env mask as the kernels read it: uint8 [E] (a bool tensor is converted), or None."""
    if mask is None:
        return None
    if isinstance(mask, torch.Tensor) and mask.dtype == torch.bool:
        mask = mask.to(torch.uint8)
    need("mask", mask, E, torch.uint8, device)
    return mask


def host_rows(rows, n_rows, words):
    """Reduced rows (int64 words, float64 sums as their bit patterns) copied to the host (this waits
    for the current stream): the [n_rows][words] lists read as int64 and as float64."""
    host = rows.cpu().view(n_rows, words)
    return host.tolist(), host.view(torch.float64).tolist()


class EnvSlice:
    """``n`` envs of an accumulator (the owner) from env ``lo``, such as a VecEnv.split part's own:
    the owner's buffers through offset pointers in a descriptor of the family's own.

    A family's slice class names the descriptor type, the owner's per-env arrays, its [E, K]
    episode tables (filled when the owner records: ``owner.record`` > 0) and the descriptor's fixed
    fields with the owner attribute each comes from, and adds its calls. The owner derives from
    its slice class, is its own slice of all envs and names the slice class as ``_part``."""

    _desc = None
    _per_env = ()
    _tables = ()
    _fixed = {}

    def __init__(self, owner, lo: int, n: int):
        self.owner, self.lo, self.E = owner, lo, n
        self.c = self._desc(E=n, **{field: getattr(owner, attr) for field, attr in self._fixed.items()})
        names = self._per_env + (self._tables if getattr(owner, "record", 0) else ())
        for name in names:
            setattr(self.c, name, _ptr(getattr(owner, name)[lo:lo + n]))

    def view(self, lo: int, n: int):
        """The slice object of envs [lo, lo + n): its calls touch only those."""
        lo, n = int(lo), int(n)
        if lo < 0 or n < 1 or lo + n > self.E:
            raise ValueError(f"view: envs [{lo}, {lo + n}) are not within 0..{self.E}")
        return self._part(self, lo, n)
