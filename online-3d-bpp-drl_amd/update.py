"""a2c_loss -- the loss of the reference's A2C update (acktr/algo/acktr_pipeline.py:45-92, acktr=False) and its gradients with
respect to the three network outputs as ONE native call (include/bpp_update.h).

    out = bpp_amd.a2c_loss(logits, values, pred_mask, location_masks, action, returns)
    optimizer.zero_grad()
    out.backward()                      # the kernel's gradients enter autograd at the network outputs
    value_loss, action_loss = out.value_loss, out.action_loss        # 0-dim device tensors, no sync

Every coefficient of the total is known before the backward pass starts, so the kernel that computes the five terms writes
d loss / d logits, d loss / d values and d loss / d pred_mask in the same pass; `backward()` only hands them to autograd.  The
terms are sums in double in a fixed order: the same bits on every run.
"""
import torch

from . import _lib
from ._front import NativeLoss, dense_f32, dense_i64, loss_buffers, stream_ptr

_CACHE = {}     # (device, E, M) -> workspace and gradient buffers: static addresses for a captured region


class A2CLoss(NativeLoss):
    """Result of a2c_loss: `terms` float32 [6] on the device = (value_loss, action_loss, dist_entropy, prob_loss, graph_loss,
    loss), each also a 0-dim view by name; `rows` float32 [E, 5] = per-row (adv^2, -adv logp, entropy, bad mass, squared mask
    error) when asked for; backward() sends the gradients into the graph the network outputs hang on.  The gradient buffers
    belong to a cache per (device, E, M): the next a2c_loss of the same shape overwrites them, so call backward() first."""
    TERMS = _lib.A2C_TERMS


def a2c_loss(logits, values, pred_mask, location_masks, action, returns, value_loss_coef=0.5, entropy_coef=0.01, invalid_coef=2.0,
             mask_coef=5.0, rows=False):
    """logits [E, M], values [E] / [E, 1] / [T, N, 1] and pred_mask [E, M] or None: the network's outputs, still attached to the
    autograd graph; location_masks [E, M] (or [T, N, M]), action int64 [E] / [E, 1] / [T, N, 1], returns like values -> A2CLoss.
    The default coefficients are the reference's (mask_coef: its `force = 0.5 * 10`).  Only enqueues on the current stream."""
    for t in (logits, values, location_masks, action, returns) + ((pred_mask,) if pred_mask is not None else ()):
        if not torch.is_tensor(t):
            raise ValueError("a2c_loss takes tensors")
        if t.device.type != "cuda":
            raise RuntimeError("a2c_loss needs its tensors on a HIP device")
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError("logits must be [E, M]")
    dev = logits.device
    E, M = (int(v) for v in logits.shape)
    x = dense_f32(logits, (E, M), "logits", dev)
    v = dense_f32(values, (E,), "values", dev)
    m = dense_f32(location_masks, (E, M), "location_masks", dev)
    r = dense_f32(returns, (E,), "returns", dev)
    p = dense_f32(pred_mask, (E, M), "pred_mask", dev) if pred_mask is not None else None
    a = dense_i64(action, E, "action", dev)
    buf = loss_buffers(_CACHE, _lib.lib().bpp_a2c_loss_workspace, dev, E, M, pred_mask=p is not None)
    terms = torch.empty(6, dtype=torch.float32, device=dev)
    row_terms = torch.empty((E, 5), dtype=torch.float32, device=dev) if rows else None
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().bpp_a2c_loss(x.data_ptr(), m.data_ptr(), a.data_ptr(), v.data_ptr(), r.data_ptr(),
                                           p.data_ptr() if p is not None else None, float(value_loss_coef), float(entropy_coef),
                                           float(invalid_coef), float(mask_coef), buf["grad_logits"].data_ptr(),
                                           buf["grad_values"].data_ptr(), buf["grad_pred_mask"].data_ptr() if p is not None else None,
                                           row_terms.data_ptr() if rows else None, terms.data_ptr(), buf["workspace"].data_ptr(), E, M,
                                           stream_ptr(dev)))
    outputs, grads = [logits, values], [buf["grad_logits"], buf["grad_values"]]
    if p is not None:
        outputs.append(pred_mask)
        grads.append(buf["grad_pred_mask"])
    return A2CLoss(terms, row_terms, outputs, grads, dict(logits=x, values=v, pred_mask=p, location_masks=m, action=a, returns=r))
