"""K-FAC for the reference's ACKTR path (acktr/algo/kfac.py:90-258, `--algorithm acktr`, main.py:104-110): the Kronecker factors from
ONE native call each (include/bpp_kfac.h), the rest of the optimiser in plain torch on the factors' device.

    optimizer = bpp_amd.KFACOptimizer(net)              # splits every bias into a module of its own, hooks the layers
    ...
    if optimizer.steps % optimizer.Ts == 0:             # the sampled-Fisher pass of acktr_pipeline.py:68-84
        net.zero_grad()
        optimizer.acc_stats = True
        fisher_loss.backward(retain_graph=True)
        optimizer.acc_stats = False
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()

A factor is scale * X^T X over the rows X the reference builds: for a Conv2d input the im2col patches, which the kernel forms
in LDS and never writes (the reference materialises all of them: 576 floats per output position for a 3x3/64-channel layer);
for a conv grad-output the [B][OC][OH*OW] tensor read in place; for a Linear the [B][D] matrix.  `fast_cnn` is not offered: the
reference never enables it.
"""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._front import Workspace, raw_stream

PATCH, ROWS, NCHW = _lib.KFAC_PATCH, _lib.KFAC_ROWS, _lib.KFAC_NCHW
_LAYOUTS = {"patch": PATCH, "rows": ROWS, "nchw": NCHW, PATCH: PATCH, ROWS: ROWS, NCHW: NCHW}
_WORKSPACE = Workspace()    # (device, stream) -> float64 tensor, grown to the largest request; a captured call takes its own


def _pair(v):
    return (int(v), int(v)) if not isinstance(v, (tuple, list)) else (int(v[0]), int(v[1]))


def factor_geometry(src, layout, kernel_size=(1, 1), stride=(1, 1), padding=(0, 0)):
    """(layout id, geom list for bpp_kfac_factor, D, R, positions per sample) of a source tensor; ValueError on a shape that
    does not fit the layout."""
    if layout not in _LAYOUTS:
        raise ValueError("unknown layout %r (patch, rows or nchw)" % (layout,))
    layout = _LAYOUTS[layout]
    if not torch.is_tensor(src) or src.dtype != torch.float32:
        raise ValueError("src must be a float32 tensor")
    if src.numel() == 0:
        raise ValueError("src is empty")
    if layout == PATCH:
        if src.dim() != 4:
            raise ValueError("a patch source is [B, C, H, W]")
        (kh, kw), (sh, sw), (ph, pw) = _pair(kernel_size), _pair(stride), _pair(padding)
        B, C, H, W = (int(v) for v in src.shape)
        if min(kh, kw, sh, sw) < 1 or min(ph, pw) < 0 or kh > H + 2 * ph or kw > W + 2 * pw:
            raise ValueError("kernel %s, stride %s, padding %s do not fit a %dx%d image" % ((kh, kw), (sh, sw), (ph, pw), H, W))
        oh, ow = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
        return layout, [B, C, H, W, kh, kw, sh, sw, ph, pw], C * kh * kw, B * oh * ow, oh * ow
    if layout == ROWS:
        if src.dim() != 2:
            raise ValueError("a rows source is [R, D]")
        R, D = (int(v) for v in src.shape)
        return layout, [R, D], D, R, 1
    if src.dim() < 3:
        raise ValueError("an nchw source is [B, D, ...]")
    B, D = int(src.shape[0]), int(src.shape[1])
    S = src.numel() // (B * D)
    return layout, [B, D, S], D, B * S, S


def factor_scale(kind, batch, positions=1):
    """The product of the reference's scalings for a factor, in double (include/bpp_kfac.h): kind = 'conv_a' (kfac.py:38, :45),
    'conv_g' (:57, :62-63), 'linear_a' (:45) or 'linear_g' (:62-63; a bias gradient summed over space alike)."""
    batch, positions = float(batch), float(positions)
    if kind == "conv_a":
        return 1.0 / (batch * positions * positions)
    if kind == "conv_g":
        return batch * positions
    if kind == "linear_a":
        return 1.0 / batch
    if kind == "linear_g":
        return batch
    raise ValueError("unknown factor kind %r" % (kind,))


def _check_m(m, D, dev):
    if not torch.is_tensor(m) or m.dtype != torch.float32 or tuple(m.shape) != (D, D) or not m.is_contiguous():
        raise ValueError("m must be a dense float32 [%d, %d] tensor" % (D, D))
    if m.device != dev:
        raise ValueError("m is on %s, src on %s" % (m.device, dev))


def kfac_factor(src, layout, m, stat_decay, first, scale, kernel_size=(1, 1), stride=(1, 1), padding=(0, 0)):
    """m <- running average of scale * X^T X (bpp_kfac_factor): src the float32 device tensor the rows X are read from in
    `layout` ('patch': [B, C, H, W] with kernel_size / stride / padding, 'rows': [R, D], 'nchw': [B, D, ...]), m float32 [D, D]
    on the same device, updated in place and returned; first: m is set to the factor before the update (kfac.py:159-162).
    Only enqueues on the current stream; inside a stream capture the call takes a workspace of its own from the graph's pool.
    The result is symmetric bit for bit and the same bits on every run."""
    layout, geom, D, R, _ = factor_geometry(src, layout, kernel_size, stride, padding)
    if src.device.type != "cuda":
        raise RuntimeError("kfac_factor needs its tensors on a HIP device")
    _check_m(m, D, src.device)
    if not 0.0 < float(stat_decay) < 1.0:
        raise ValueError("stat_decay must lie in (0, 1)")
    dev = src.device
    x = src.detach().contiguous()
    g = _lib.kfac_geom(geom)
    with torch.cuda.device(dev):
        stream = raw_stream(dev)
        need = (int(_lib.lib().bpp_kfac_factor_workspace(layout, g)) + 7) // 8
        ws = _WORKSPACE.take((dev, stream), need, torch.float64, dev)
        _lib.check(_lib.lib().bpp_kfac_factor(x.data_ptr(), layout, g, m.data_ptr(), float(scale), float(stat_decay), int(bool(first)),
                                              ws.data_ptr(), ctypes.c_void_p(stream)))
    return m


def factor_rows(src, layout, kernel_size=(1, 1), stride=(1, 1), padding=(0, 0)):
    """The rows X of a factor as a dense [R, D] tensor in plain torch (unfold -> contiguous): what the native kernel never
    builds.  The factor routine for CPU tensors and the baseline of tools/bench_kfac.py."""
    layout, geom, D, R, _ = factor_geometry(src, layout, kernel_size, stride, padding)
    src = src.detach()
    if layout == PATCH:
        cols = F.unfold(src, _pair(kernel_size), padding=_pair(padding), stride=_pair(stride))       # [B, D, OH * OW]
        return cols.transpose(1, 2).contiguous().view(R, D)
    if layout == ROWS:
        return src.contiguous()
    return src.reshape(geom[0], D, geom[2]).transpose(1, 2).contiguous().view(R, D)


def torch_factor(src, layout, m, stat_decay, first, scale, kernel_size=(1, 1), stride=(1, 1), padding=(0, 0)):
    """kfac_factor in plain torch, on whatever device src lives: the routine KFACOptimizer uses for CPU tensors."""
    rows = factor_rows(src, layout, kernel_size, stride, padding)
    _check_m(m, rows.shape[1], src.device)
    aa = (rows.t() @ rows) * float(scale)
    if first:
        m.copy_(aa)
    m.mul_(stat_decay / (1.0 - stat_decay)).add_(aa).mul_(1.0 - stat_decay)
    return m


class AddBias(nn.Module):
    """A bias as a layer of its own, parameter `_bias` [n, 1]: the shape and name the reference's checkpoints carry."""

    def __init__(self, bias):
        super().__init__()
        self._bias = nn.Parameter(bias.unsqueeze(1))

    def forward(self, x):
        return x + self._bias.t().view((1, -1) if x.dim() == 2 else (1, -1, 1, 1))


class SplitBias(nn.Module):
    """`module` without its bias, followed by `add_bias`."""

    def __init__(self, module):
        super().__init__()
        self.module = module
        self.add_bias = AddBias(module.bias.data)
        self.module.bias = None

    def forward(self, x):
        return self.add_bias(self.module(x))


def split_biases(model):
    """Replace every child that owns a bias by SplitBias(child), recursively; the parameter names become
    `<child>.module.weight` and `<child>.add_bias._bias`, which main.py:70-75 maps back to `<child>.weight` / `<child>.bias`."""
    for name, child in model.named_children():
        if getattr(child, "bias", None) is not None:
            model._modules[name] = SplitBias(child)
        else:
            split_biases(child)
    return model


def plain_state_dict(state):
    """A state dict saved from a bias-split model under the names and shapes of the unsplit one (main.py:70-75,
    acktr/model_loader.py:26-32)."""
    out = {}
    for k, v in state.items():
        k = k.replace("module.", "").replace("add_bias.", "").replace("_bias", "bias")
        out[k] = v.squeeze(dim=-1) if v.dim() <= 3 else v
    return out


def _kind(module):
    if isinstance(module, nn.Conv2d):
        return "conv"
    if isinstance(module, nn.Linear):
        return "linear"
    if module.__class__.__name__ == "AddBias":
        return "bias"
    return None


class KFACOptimizer(torch.optim.Optimizer):
    """The reference's KFACOptimizer (kfac.py:90-258) with the factor statistics from bpp_kfac_factor.

    Public surface as there: `acc_stats`, `steps`, `Ts`, `Tf`, `step()`, `zero_grad()`, and `m_aa` / `m_gg` / `Q_a` / `Q_g` /
    `d_a` / `d_g` keyed by module.  A-statistics are taken in a forward-pre hook while gradients are enabled and
    `steps % Ts == 0`, G-statistics in a full backward hook while `acc_stats` is set; at `steps == 0` a factor replaces its
    running average before the update.  Every `Tf` steps the factors are decomposed with torch.linalg.eigh (eigenvalues
    <= 1e-6 set to 0); each step preconditions the gradients on both sides and takes one SGD-with-momentum step.
    `fast_cnn` is not offered: the reference never enables it.

    One difference: nu = min(1, sqrt(kl_clip / vg_sum)) stays a device tensor, where the reference's math.sqrt of a tensor
    waits for the device once per update.

    factor_fn: a routine with kfac_factor's signature that replaces it; default kfac_factor for device tensors and
    torch_factor (plain torch) for CPU tensors."""

    def __init__(self, model, lr=0.25, momentum=0.9, stat_decay=0.99, kl_clip=0.001, damping=1e-2, weight_decay=0, Ts=1, Tf=10,
                 factor_fn=None):
        split_biases(model)
        super().__init__(model.parameters(), dict())
        self.model = model
        self.factor_fn = factor_fn
        self.modules, self._kinds = [], {}
        self.steps = 0
        self.acc_stats = False
        self.m_aa, self.m_gg = {}, {}
        self.Q_a, self.Q_g = {}, {}
        self.d_a, self.d_g = {}, {}
        self.momentum, self.stat_decay = momentum, stat_decay
        self.lr, self.kl_clip, self.damping, self.weight_decay = lr, kl_clip, damping, weight_decay
        self.Ts, self.Tf = Ts, Tf
        self.eigh_on_host = False
        for module in model.modules():
            kind = _kind(module)
            if kind is None:
                continue
            if kind != "bias" and module.bias is not None:
                raise ValueError("a %s still owns its bias: every bias must be a layer of its own" % module.__class__.__name__)
            self.modules.append(module)
            self._kinds[module] = kind
            module.register_forward_pre_hook(self._save_input)
            module.register_full_backward_hook(self._save_grad_output)
        self.optim = torch.optim.SGD(model.parameters(), lr=self.lr * (1 - self.momentum), momentum=self.momentum)

    def _factor(self, store, module, src, layout, scale, **conv):
        D = factor_geometry(src, layout, **conv)[2]
        m = store.get(module)
        if m is None or m.device != src.device:
            m = store[module] = torch.zeros((D, D), dtype=torch.float32, device=src.device)
        fn = self.factor_fn or (kfac_factor if src.device.type == "cuda" else torch_factor)
        fn(src, layout, m, self.stat_decay, self.steps == 0, scale, **conv)

    def _save_input(self, module, inputs):
        if not (torch.is_grad_enabled() and self.steps % self.Ts == 0):
            return
        x, kind = inputs[0].detach(), self._kinds[module]
        if kind == "conv":
            conv = dict(kernel_size=module.kernel_size, stride=module.stride, padding=module.padding)
            positions = factor_geometry(x, "patch", **conv)[4]
            self._factor(self.m_aa, module, x.contiguous(), "patch", factor_scale("conv_a", x.shape[0], positions), **conv)
        elif kind == "linear":
            if x.dim() != 2:
                raise ValueError("the input of a Linear must be [B, D]")
            self._factor(self.m_aa, module, x.contiguous(), "rows", factor_scale("linear_a", x.shape[0]))
        else:                                           # the constant [[1]] through the same running average (kfac.py:39-45)
            m = self.m_aa.get(module)
            if m is None or self.steps == 0:
                m = self.m_aa[module] = torch.ones((1, 1), dtype=torch.float32, device=x.device)
            m.mul_(self.stat_decay / (1.0 - self.stat_decay)).add_(1.0).mul_(1.0 - self.stat_decay)

    def _save_grad_output(self, module, grad_input, grad_output):
        if not self.acc_stats:
            return
        g, kind = grad_output[0].detach(), self._kinds[module]
        B = g.shape[0]
        if kind == "conv":
            g = g.contiguous()
            self._factor(self.m_gg, module, g, "nchw", factor_scale("conv_g", B, g.numel() // (B * g.shape[1])))
        else:
            if g.dim() > 2:                             # a conv bias: its gradient summed over space (kfac.py:59-60)
                g = g.reshape(B, g.shape[1], -1).sum(-1)
            self._factor(self.m_gg, module, g.contiguous(), "rows", factor_scale("linear_g", B))

    def _eigh(self, m):
        if not self.eigh_on_host:
            try:
                return torch.linalg.eigh(m)
            except RuntimeError:
                if m.device.type == "cpu":
                    raise
                self.eigh_on_host = True              # no symmetric eigensolver on this device: decompose a host copy from now on
        d, q = torch.linalg.eigh(m.cpu())
        return d.to(m.device), q.to(m.device)

    def step(self):
        params = [p for group in self.param_groups for p in group["params"]]
        if self.weight_decay > 0:
            for p in params:
                p.grad.add_(p.detach(), alpha=self.weight_decay)
        la = self.damping + self.weight_decay
        refresh = self.steps % self.Tf == 0
        updates = {}
        for module in self.modules:
            own = list(module.parameters())
            if len(own) != 1:
                raise ValueError("a K-FAC layer must own exactly one parameter")
            p = own[0]
            if refresh:
                for d_store, q_store, m in ((self.d_g, self.Q_g, self.m_gg[module]), (self.d_a, self.Q_a, self.m_aa[module])):
                    d, q = self._eigh(m)
                    d_store[module], q_store[module] = d * (d > 1e-6).to(d.dtype), q.to(self.m_gg[module].device)
                self.d_a[module] = self.d_a[module].to(self.m_gg[module].device)
            q_g, q_a, d_g, d_a = self.Q_g[module], self.Q_a[module], self.d_g[module], self.d_a[module]
            grad = p.grad.detach()
            mat = grad.reshape(grad.shape[0], -1)
            v = q_g @ ((q_g.t() @ mat @ q_a) / (d_g.unsqueeze(1) * d_a.unsqueeze(0) + la)) @ q_a.t()
            updates[p] = v.view_as(grad)
        vg_sum = 0
        for p in params:
            vg_sum = vg_sum + (updates[p] * p.grad.detach() * self.lr * self.lr).sum()
        nu = torch.clamp(torch.sqrt(self.kl_clip / vg_sum), max=1.0)
        for p in params:
            p.grad.copy_(updates[p])
            p.grad.mul_(nu)
        self.optim.step()
        self.steps += 1
