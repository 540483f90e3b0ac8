"""What every torch front-end of a native call needs, stated once: the calling thread's current HIP stream, the
checks of the tensors a kernel reads in place, the grown-to-largest workspace with its in-capture rule, and the result class of
the fused losses."""
import ctypes

import torch

RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def raw_stream(dev):
    """The calling thread's current HIP stream on `dev` as an int (0: the default stream), what torch.cuda.Stream.cuda_stream
    holds: the raw handle straight from torch's stream table where this torch has it -- a third of the cost of building a
    torch.cuda.Stream object per call."""
    if RAW_STREAM is not None and dev.index is not None:
        return RAW_STREAM(dev.index)
    return torch.cuda.current_stream(dev).cuda_stream


def stream_ptr(dev):
    """raw_stream(dev) as the c_void_p the native calls take (spelled out: this is on every lock-step's path)."""
    if RAW_STREAM is not None and dev.index is not None:
        return ctypes.c_void_p(RAW_STREAM(dev.index))
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def dense_f32(t, shape, what, dev):
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


def dense_i64(t, n, what, dev):
    """The dense int64 [n] tensor the kernel reads."""
    if not torch.is_tensor(t) or t.dtype != torch.int64 or t.device != dev or t.numel() != n:
        raise ValueError("%s must be an int64 tensor of %d entries on the logits' device" % (what, n))
    return t.reshape(n).contiguous()


def obs_rows(obs, A, who):
    """(n, floats between two rows) of an obs the native calls take: float32 [n, >= 4 A] on a HIP device, rows with unit inner
    stride; `who`: the subject of the wrong-device error."""
    if not torch.is_tensor(obs) or obs.dtype != torch.float32 or obs.dim() != 2 or obs.shape[0] < 1:
        raise ValueError("obs must be a float32 [n, 4 A] tensor with n >= 1")
    if obs.device.type != "cuda":
        raise RuntimeError("%s needs its tensors on a HIP device" % who)
    n = int(obs.shape[0])
    if obs.shape[1] < 4 * A or obs.stride(1) != 1 or (n > 1 and obs.stride(0) < 4 * A):
        raise ValueError("obs rows must be contiguous and hold 4 A = %d floats" % (4 * A))
    return n, int(obs.stride(0)) if n > 1 else int(obs.shape[1])


class Workspace(dict):
    """key -> tensor, grown to the largest request.  Inside a stream capture take() hands out a tensor of the call's own from
    the graph's memory pool and leaves the dict alone: a captured call keeps its workspace for as long as the graph lives, and
    no eager call ever writes into memory the replays use."""

    def take(self, key, need, dtype, dev):
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():     # (not asked for a CPU dev: it would initialise the runtime)
            return torch.empty(need, dtype=dtype, device=dev)
        ws = self.get(key)
        if ws is None or ws.numel() < need:
            ws = self[key] = torch.empty(need, dtype=dtype, device=dev)
        return ws


class NativeLoss(object):
    """Result of a fused loss call: `terms` float32 on the device, each also a 0-dim view under its name in the class's TERMS;
    `rows` the per-row terms when asked for; `inputs` the dense tensors the kernel reads (views of the caller's wherever those
    are dense); backward() sends the kernel's gradients into the graph the network outputs hang on."""
    TERMS = ()

    def __init__(self, terms, rows, outputs=None, grads=None, inputs=None):
        self.terms, self.rows, self.inputs = terms, rows, inputs
        self._outputs, self._grads = outputs, grads

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        for i, name in enumerate(cls.TERMS):
            setattr(cls, name, property(lambda self, i=i: self.terms[i]))

    @property
    def grad_logits(self):
        return self._grads[0] if self._grads else None

    @property
    def grad_values(self):
        return self._grads[1] if self._grads else None

    @property
    def grad_pred_mask(self):
        return self._grads[2] if self._grads and len(self._grads) > 2 else None

    def backward(self):
        pairs = [(t, g.view(t.shape)) for t, g in zip(self._outputs, self._grads) if t.requires_grad]
        if not pairs:
            raise RuntimeError("none of logits, values and pred_mask requires grad")
        torch.autograd.backward([t for t, _ in pairs], [g for _, g in pairs])


def loss_buffers(cache, workspace_bytes, dev, B, M, pred_mask=False):
    """cache[(dev, B, M)]: the workspace (`workspace_bytes(B, M)` bytes) and the gradient buffers of a fused loss on B rows of M
    logits -- static addresses for a captured region.  pred_mask: the call also writes d loss / d pred_mask."""
    key = (dev, B, M)
    buf = cache.get(key)
    if buf is None:
        n = int(workspace_bytes(B, M))
        buf = cache[key] = {"workspace": torch.empty((n + 7) // 8, dtype=torch.float64, device=dev),
                            "grad_logits": torch.empty((B, M), dtype=torch.float32, device=dev),
                            "grad_values": torch.empty(B, dtype=torch.float32, device=dev), "grad_pred_mask": None}
    if pred_mask and buf["grad_pred_mask"] is None:
        buf["grad_pred_mask"] = torch.empty((B, M), dtype=torch.float32, device=dev)
    return buf
