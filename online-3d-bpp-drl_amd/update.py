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
import ctypes

import torch

from . import _lib

_CACHE = {}     # (device, E, M) -> workspace and gradient buffers: static addresses for a captured region


def _buffers(dev, E, M):
    key = (dev, E, M)
    buf = _CACHE.get(key)
    if buf is None:
        n = int(_lib.lib().bpp_a2c_loss_workspace(E, M))
        buf = _CACHE[key] = {"workspace": torch.empty((n + 7) // 8, dtype=torch.float64, device=dev),
                             "grad_logits": torch.empty((E, M), dtype=torch.float32, device=dev),
                             "grad_values": torch.empty(E, dtype=torch.float32, device=dev), "grad_pred_mask": None}
    return buf


class A2CLoss(object):
    """Result of a2c_loss: `terms` float32 [6] on the device = (value_loss, action_loss, dist_entropy, prob_loss, graph_loss,
    loss), each also a 0-dim view by name; `rows` float32 [E, 5] = per-row (adv^2, -adv logp, entropy, bad mass, squared mask
    error) when asked for; backward() sends the gradients into the graph the network outputs hang on.  The gradient buffers
    belong to a cache per (device, E, M): the next a2c_loss of the same shape overwrites them, so call backward() first."""

    def __init__(self, terms, rows, outputs, grads, inputs):
        self.terms, self.rows = terms, rows
        self.inputs = inputs            # the dense tensors the kernel reads (views of the caller's wherever those are dense)
        self._outputs, self._grads = outputs, grads

    @property
    def grad_logits(self):
        return self._grads[0]

    @property
    def grad_values(self):
        return self._grads[1]

    @property
    def grad_pred_mask(self):
        return self._grads[2] if len(self._grads) > 2 else None

    def backward(self):
        pairs = [(t, g.view(t.shape)) for t, g in zip(self._outputs, self._grads) if t.requires_grad]
        if not pairs:
            raise RuntimeError("none of logits, values and pred_mask requires grad")
        torch.autograd.backward([t for t, _ in pairs], [g for _, g in pairs])


for _i, _name in enumerate(_lib.A2C_TERMS):
    setattr(A2CLoss, _name, property(lambda self, _i=_i: self.terms[_i]))


def _f32(t, shape, what, dev):
    """The dense float32 tensor the kernel reads: `t` detached, viewed as `shape`."""
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise ValueError("%s must be a float32 tensor" % what)
    if t.device != dev:
        raise ValueError("%s is on %s, the logits on %s" % (what, t.device, dev))
    n = 1
    for s in shape:
        n *= s
    if t.numel() != n:
        raise ValueError("%s has %d elements, expected %s" % (what, t.numel(), "x".join(str(s) for s in shape)))
    return t.detach().reshape(shape).contiguous()


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
    x = _f32(logits, (E, M), "logits", dev)
    v = _f32(values, (E,), "values", dev)
    m = _f32(location_masks, (E, M), "location_masks", dev)
    r = _f32(returns, (E,), "returns", dev)
    p = _f32(pred_mask, (E, M), "pred_mask", dev) if pred_mask is not None else None
    if action.dtype != torch.int64 or action.device != dev or action.numel() != E:
        raise ValueError("action must be an int64 tensor of E entries on the logits' device")
    a = action.reshape(E).contiguous()
    buf = _buffers(dev, E, M)
    if p is not None and buf["grad_pred_mask"] is None:
        buf["grad_pred_mask"] = torch.empty((E, M), dtype=torch.float32, device=dev)
    terms = torch.empty(6, dtype=torch.float32, device=dev)
    row_terms = torch.empty((E, 5), dtype=torch.float32, device=dev) if rows else None
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(_lib.lib().bpp_a2c_loss(x.data_ptr(), m.data_ptr(), a.data_ptr(), v.data_ptr(), r.data_ptr(),
                                           p.data_ptr() if p is not None else None, float(value_loss_coef), float(entropy_coef),
                                           float(invalid_coef), float(mask_coef), buf["grad_logits"].data_ptr(),
                                           buf["grad_values"].data_ptr(), buf["grad_pred_mask"].data_ptr() if p is not None else None,
                                           row_terms.data_ptr() if rows else None, terms.data_ptr(), buf["workspace"].data_ptr(), E, M,
                                           stream))
    outputs, grads = [logits, values], [buf["grad_logits"], buf["grad_values"]]
    if p is not None:
        outputs.append(pred_mask)
        grads.append(buf["grad_pred_mask"])
    return A2CLoss(terms, row_terms, outputs, grads, dict(logits=x, values=v, pred_mask=p, location_masks=m, action=a, returns=r))
