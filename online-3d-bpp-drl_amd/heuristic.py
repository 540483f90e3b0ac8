"""The lowest-top packing heuristic on the device (include/bpp_heuristic.h): per bin the placement whose
resulting top is lowest, then the one that leaves the smoothest surface, then the lowest index -- the baseline packer a checkpoint
is compared with.  One HIP kernel (`bpp_heuristic_act`), integer arithmetic throughout; there is no CPU fallback."""
import torch

from . import _lib
from ._front import obs_rows, stream_ptr

RULES = tuple(_lib.HEURISTIC_RULES)


def rule_id(rule):
    """BPP_HEUR_* of a rule's name."""
    try:
        return _lib.HEURISTIC_RULES[rule]
    except (KeyError, TypeError):
        raise ValueError("unknown heuristic rule %r (known: %s)" % (rule, ", ".join(RULES)))


def check_outputs(n, dev, out, top):
    """The (action, top) tensors of a call on n bins: `out` int64 [n] (allocated when None), `top` int32 [n] or None."""
    if out is None:
        out = torch.empty((n,), dtype=torch.int64, device=dev)
    elif not torch.is_tensor(out) or out.dtype != torch.int64 or out.numel() != n or out.device != dev or not out.is_contiguous():
        raise ValueError("out must be a contiguous int64 [n] tensor on the inputs' device")
    if top is not None and (not torch.is_tensor(top) or top.dtype != torch.int32 or top.numel() != n or top.device != dev
                            or not top.is_contiguous()):
        raise ValueError("top must be a contiguous int32 [n] tensor on the inputs' device")
    return out, top


def heuristic_act(obs, location_masks, container_size, enable_rotation=False, rule="lowest_top", out=None, top=None):
    """obs float32 [n, >= 4 A] (rows with unit inner stride: a storage slot or a column slice of a wider tensor will do) and
    location_masks float32 [n, M] on a HIP device -> int64 [n] actions on that device, enqueued on torch's current stream (no
    synchronisation, capturable into a graph).  rule: "lowest_top" (lowest top, smoothest surface, lowest index) or
    "lowest_top_plain" (lowest top, lowest index).  out: int64 [n] tensor to write into; top: int32 [n] tensor that receives the
    chosen top (-1 where the mask offers nothing placeable)."""
    W, L = int(container_size[0]), int(container_size[1])
    A = W * L
    M = A * (1 + int(bool(enable_rotation)))
    r = rule_id(rule)
    if not torch.is_tensor(obs) or not torch.is_tensor(location_masks):
        raise ValueError("obs and location_masks must be tensors")
    (n, stride), dev = obs_rows(obs, A, "heuristic_act"), obs.device
    if location_masks.device != dev:
        raise RuntimeError("heuristic_act needs its tensors on a HIP device")
    if location_masks.dtype != torch.float32 or tuple(location_masks.shape) != (n, M) or not location_masks.is_contiguous():
        raise ValueError("location_masks must be a contiguous float32 [n, M = %d] tensor" % M)
    out, top = check_outputs(n, dev, out, top)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().bpp_heuristic_act(obs.data_ptr(), stride, location_masks.data_ptr(), n, W, L, int(bool(enable_rotation)), r,
                                                out.data_ptr(), top.data_ptr() if top is not None else None, stream_ptr(dev)))
    return out
