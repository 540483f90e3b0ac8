"""PPO -- the reference's third algorithm (acktr/algo/ppo.py:34-95) on the masked head of acktr/distributions.py:71-101
(include/bpp_ppo.h).

    agent = bpp_amd.PPO(net, clip_param=0.1, ppo_epoch=4, num_mini_batch=32, value_loss_coef=0.5, entropy_coef=0.01, lr=7e-4, eps=1e-5,
                        max_grad_norm=0.5)
    value_loss, action_loss, dist_entropy = agent.update(rollouts)          # rollouts: bpp_amd.RolloutStorage

One mini-batch is ONE native call: `ppo_loss` evaluates the masked head on the mini-batch's logits, forms the clipped surrogate and
the clipped value loss and writes the gradients at the network's outputs in the same pass.  Feasibility masks, actions, old values,
returns, old log-probabilities and advantages are read in place in the rollout's slabs through the mini-batch's row indices: the only
thing gathered per mini-batch is the observation rows the network reads (bpp_gather_rows).

`ppo_loss_torch` states the same expressions in plain torch on any device and dtype: the path of a CPU storage (an explicit twin,
not a fallback -- ppo_loss itself refuses tensors that are not on a HIP device) and the baseline of tools/bench_ppo.py.
"""
import torch

from . import _lib
from ._front import NativeLoss, dense_f32, dense_i64, loss_buffers, stream_ptr

_CACHE = {}     # (device, B, M) -> workspace and gradient buffers: static addresses for a captured region
PROB_EPS = 1.1920928955078125e-7        # torch.finfo(float32).eps: the clamp of probs_to_logits the kernels use


class PPOLoss(NativeLoss):
    """Result of ppo_loss / ppo_loss_torch: `terms` [7] = (value_loss, action_loss, dist_entropy, prob_loss, graph_loss, loss,
    clip_fraction), detached, each also a 0-dim view by name; `rows` [B, 7] = per-row (value term, action term, entropy, bad mass,
    squared mask error, ratio, clipped flag) when asked for; backward() sends the gradients into the graph the network outputs hang
    on.  The native gradient buffers belong to a cache per (device, B, M): the next ppo_loss of the same shape overwrites them, so
    call backward() first."""

    TERMS = _lib.PPO_TERMS

    def __init__(self, terms, rows, outputs=None, grads=None, inputs=None, total=None):
        NativeLoss.__init__(self, terms, rows, outputs, grads, inputs)
        self._total = total

    def backward(self):
        if self._total is not None:     # ppo_loss_torch: autograd of the expressions
            self._total.backward()
        else:
            NativeLoss.backward(self)


def ppo_loss(logits, values, pred_mask, location_masks, action, value_preds, returns, old_log_probs, advantages, indices=None,
             clip_param=0.2, value_loss_coef=0.5, entropy_coef=0.01, invalid_coef=0.0, mask_coef=0.0, use_clipped_value_loss=True,
             rows=False):
    """logits [B, M], values [B] / [B, 1] and pred_mask [B, M] or None: the network's outputs on a mini-batch, still attached to the
    autograd graph.  location_masks [E, M] (or [T, N, M]), action int64, value_preds, returns, old_log_probs and advantages of E
    entries each: the rollout, read in place at rows `indices` (int64 [B]; None = rows 0 .. B - 1) -> PPOLoss.  An index outside
    [0, E) makes that row's gradients and the terms NaN.  Only enqueues on the current stream."""
    for t in (logits, values, location_masks, action, value_preds, returns, old_log_probs, advantages) + \
            tuple(t for t in (pred_mask, indices) if t is not None):
        if not torch.is_tensor(t):
            raise ValueError("ppo_loss takes tensors")
        if t.device.type != "cuda":
            raise RuntimeError("ppo_loss needs its tensors on a HIP device (ppo_loss_torch states it for any other)")
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError("logits must be [B, M]")
    if not float(clip_param) >= 0.0:
        raise ValueError("clip_param must be >= 0")
    dev = logits.device
    B, M = (int(v) for v in logits.shape)
    if location_masks.numel() % M or location_masks.numel() < M:
        raise ValueError("location_masks must be [E, M]")
    E = location_masks.numel() // M
    x = dense_f32(logits, (B, M), "logits", dev)
    v = dense_f32(values, (B,), "values", dev)
    p = dense_f32(pred_mask, (B, M), "pred_mask", dev) if pred_mask is not None else None
    m = dense_f32(location_masks, (E, M), "location_masks", dev)
    vp, r, old, adv = (dense_f32(t, (E,), what, dev) for t, what in ((value_preds, "value_preds"), (returns, "returns"),
                                                                      (old_log_probs, "old_log_probs"), (advantages, "advantages")))
    a = dense_i64(action, E, "action", dev)
    idx = dense_i64(indices, B, "indices", dev) if indices is not None else None
    if idx is None and B > E:
        raise ValueError("without indices the mini-batch is rows 0 .. B - 1 of the rollout: B > E")
    buf = loss_buffers(_CACHE, _lib.lib().bpp_ppo_loss_workspace, dev, B, M, pred_mask=p is not None)
    terms = torch.empty(7, dtype=torch.float32, device=dev)
    row_terms = torch.empty((B, 7), dtype=torch.float32, device=dev) if rows else None
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().bpp_ppo_loss(
            x.data_ptr(), v.data_ptr(), p.data_ptr() if p is not None else None, idx.data_ptr() if idx is not None else None,
            m.data_ptr(), a.data_ptr(), vp.data_ptr(), r.data_ptr(), old.data_ptr(), adv.data_ptr(), float(clip_param),
            float(value_loss_coef), float(entropy_coef), float(invalid_coef), float(mask_coef), int(bool(use_clipped_value_loss)),
            buf["grad_logits"].data_ptr(), buf["grad_values"].data_ptr(), buf["grad_pred_mask"].data_ptr() if p is not None else None,
            row_terms.data_ptr() if rows else None, terms.data_ptr(), buf["workspace"].data_ptr(), B, E, M, stream_ptr(dev)))
    outputs, grads = [logits, values], [buf["grad_logits"], buf["grad_values"]]
    if p is not None:
        outputs.append(pred_mask)
        grads.append(buf["grad_pred_mask"])
    return PPOLoss(terms, row_terms, outputs, grads,
                   dict(logits=x, values=v, pred_mask=p, location_masks=m, action=a, value_preds=vp, returns=r, old_log_probs=old,
                        advantages=adv, indices=idx))


def masked_head_torch(logits, mask, action):
    """acktr/distributions.py:71-101 in torch expressions: (log-probability of `action` [B], entropy [B], invalid mass [B])."""
    lx = torch.softmax(logits - (1.0 - mask) * 14.0, dim=-1) + 1e-5
    p = lx / lx.sum(-1, keepdim=True)
    logc = torch.log(torch.clamp(p, PROB_EPS, 1.0 - PROB_EPS))
    logp = logc.gather(-1, action.reshape(-1, 1))[:, 0]
    return logp, -(p * logc).sum(-1), (torch.softmax(logits, dim=-1) * (1.0 - mask)).sum(-1)


def ppo_loss_torch(logits, values, pred_mask, location_masks, action, value_preds, returns, old_log_probs, advantages, indices=None,
                   clip_param=0.2, value_loss_coef=0.5, entropy_coef=0.01, invalid_coef=0.0, mask_coef=0.0, use_clipped_value_loss=True,
                   rows=False):
    """ppo_loss in plain torch expressions (ppo.py:60-80 on masked_head_torch), on any device and dtype; backward() is autograd's."""
    B, M = (int(v) for v in logits.shape)
    E = location_masks.numel() // M
    m, a = location_masks.reshape(E, M), action.reshape(E)
    vp, r, old, adv = (t.reshape(E) for t in (value_preds, returns, old_log_probs, advantages))
    if indices is not None:
        m, a, vp, r, old, adv = (t[indices] for t in (m, a, vp, r, old, adv))
    else:
        m, a, vp, r, old, adv = (t[:B] for t in (m, a, vp, r, old, adv))
    v = values.reshape(B)
    logp, ent, bad = masked_head_torch(logits, m, a)
    ratio = torch.exp(logp - old)
    surr1 = ratio * adv
    surr2 = torch.clamp(ratio, 1.0 - clip_param, 1.0 + clip_param) * adv
    action_rows = -torch.min(surr1, surr2)
    if use_clipped_value_loss:
        value_pred_clipped = vp + (v - vp).clamp(-clip_param, clip_param)
        value_rows = 0.5 * torch.max((v - r).pow(2), (value_pred_clipped - r).pow(2))
    else:
        value_rows = 0.5 * (r - v).pow(2)
    sq = ((pred_mask - m) ** 2).sum(-1) if pred_mask is not None else torch.zeros_like(ent)
    value_loss, action_loss, dist_entropy = value_rows.mean(), action_rows.mean(), ent.mean()
    prob_loss, graph_loss = bad.sum() / float(B * M), sq.sum() / float(B * M)
    total = value_loss * value_loss_coef + action_loss - dist_entropy * entropy_coef
    if invalid_coef:
        total = total + prob_loss * invalid_coef
    if mask_coef and pred_mask is not None:
        total = total + graph_loss * mask_coef
    clipped = ((ratio < 1.0 - clip_param) | (ratio > 1.0 + clip_param)).to(ratio.dtype)
    terms = torch.stack([value_loss, action_loss, dist_entropy, prob_loss, graph_loss, total, clipped.mean()]).detach()
    row_terms = torch.stack([value_rows, action_rows, ent, bad, sq, ratio, clipped], dim=1).detach() if rows else None
    return PPOLoss(terms, row_terms, total=total)


def normalized_advantages(returns, value_preds):
    """(adv - mean) / (std + 1e-5) of adv = returns - value_preds over all E elements (ppo.py:34-36): float32 tensors of one shape
    on a HIP device -> (advantages of that shape, stats float64 [2] = mean and unbiased std).  The two sums are taken in double in an
    order fixed by E alone (include/bpp_ppo.h): the same bits on every run."""
    dev = returns.device
    if dev.type != "cuda":
        raise RuntimeError("normalized_advantages needs its tensors on a HIP device")
    E = returns.numel()
    r, vp = dense_f32(returns, (E,), "returns", dev), dense_f32(value_preds, (E,), "value_preds", dev)
    L = _lib.lib()
    adv = torch.empty(tuple(returns.shape), dtype=torch.float32, device=dev)
    stats = torch.empty(2, dtype=torch.float64, device=dev)
    ws = torch.empty((int(L.bpp_ppo_advantages_workspace(E)) + 7) // 8 or 1, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.bpp_ppo_advantages(r.data_ptr(), vp.data_ptr(), adv.data_ptr(), stats.data_ptr(), E, ws.data_ptr(), stream_ptr(dev)))
    return adv, stats


def gather_rows(src, indices, out=None):
    """src[indices] for a float32 [rows, len] tensor on a HIP device whose rows are dense (any row stride) and int64 indices [B]:
    one bpp_gather_rows.  An index outside [0, rows) gives a row of NaN."""
    dev = src.device
    if dev.type != "cuda":
        raise RuntimeError("gather_rows needs its tensors on a HIP device")
    if src.dtype != torch.float32 or src.dim() != 2 or src.stride(1) != 1 or src.stride(0) < src.shape[1]:
        raise ValueError("src must be float32 [rows, len] with dense rows")
    B = int(indices.numel())
    idx = dense_i64(indices, B, "indices", dev)
    rows, n = (int(v) for v in src.shape)
    if out is None:
        out = torch.empty((B, n), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().bpp_gather_rows(src.data_ptr(), int(src.stride(0)), rows, idx.data_ptr(), B, n, out.data_ptr(), stream_ptr(dev)))
    return out


class MiniBatch(object):
    """One item of RolloutStorage.feed_forward_generator.  Unpacks into the reference's eight fields in its order (obs_batch,
    recurrent_hidden_states_batch, actions_batch, value_preds_batch, return_batch, masks_batch, old_action_log_probs_batch,
    adv_targ); `indices` is the int64 device tensor of the rows, `location_masks_batch` the rows' feasibility masks.  Every field is
    gathered when it is first read: an update through RolloutStorage.ppo_loss reads obs_batch and indices only."""
    FIELDS = ("obs_batch", "recurrent_hidden_states_batch", "actions_batch", "value_preds_batch", "return_batch", "masks_batch",
              "old_action_log_probs_batch", "adv_targ")

    def __init__(self, storage, indices, advantages):
        self._storage, self.indices, self._advantages, self._got = storage, indices, advantages, {}

    def _field(self, name):
        if name not in self._got:
            st, idx = self._storage, self.indices
            T, N = st.num_steps, st.num_envs
            if name == "obs_batch":
                flat = st.obs[:-1].view(T * N, -1)
                if flat.is_cuda and flat.dtype == torch.float32:
                    got = gather_rows(flat, idx).view((idx.numel(),) + tuple(st.obs.shape[2:]))
                else:
                    got = st.obs[:-1].view((T * N,) + tuple(st.obs.shape[2:]))[idx]
            elif name == "adv_targ":
                got = None if self._advantages is None else self._advantages.view(-1, 1)[idx]
            else:
                src = {"recurrent_hidden_states_batch": st.recurrent_hidden_states[:-1], "actions_batch": st.actions,
                       "value_preds_batch": st.value_preds[:-1], "return_batch": st.returns[:-1], "masks_batch": st.masks[:-1],
                       "old_action_log_probs_batch": st.action_log_probs, "location_masks_batch": st.location_masks[:-1]}[name]
                got = src.reshape(T * N, src.shape[-1])[idx]
            self._got[name] = got
        return self._got[name]

    def __iter__(self):
        return iter([self._field(n) for n in self.FIELDS])

    def __len__(self):
        return len(self.FIELDS)

    def __getitem__(self, i):
        return self._field(self.FIELDS[i])


for _name in MiniBatch.FIELDS + ("location_masks_batch",):
    setattr(MiniBatch, _name, property(lambda self, _name=_name: self._field(_name)))


class PPO(object):
    """acktr/algo/ppo.py with its constructor and Adam.  net(obs) -> (logits, values, pred_mask) is the examples' convention
    (pred_mask may be None); invalid_coef and mask_coef weigh the two optional terms of acktr_pipeline.py and default to 0, which
    is ppo.py exactly.  update(rollouts) takes a bpp_amd.RolloutStorage whose returns are computed: on a HIP device every
    mini-batch is one bpp_gather_rows and one bpp_ppo_loss around the network, on the CPU the same expressions in torch."""

    def __init__(self, net, clip_param, ppo_epoch, num_mini_batch, value_loss_coef, entropy_coef, lr=None, eps=None, max_grad_norm=None,
                 use_clipped_value_loss=True, invalid_coef=0.0, mask_coef=0.0):
        self.actor_critic = self.net = net
        self.clip_param, self.ppo_epoch, self.num_mini_batch = clip_param, int(ppo_epoch), int(num_mini_batch)
        self.value_loss_coef, self.entropy_coef, self.invalid_coef, self.mask_coef = value_loss_coef, entropy_coef, invalid_coef, mask_coef
        self.max_grad_norm, self.use_clipped_value_loss = max_grad_norm, use_clipped_value_loss
        self.optimizer = torch.optim.Adam(net.parameters(), lr=lr, eps=eps)

    def update(self, rollouts, generator=None):
        """ppo.py:34-95: returns (value_loss, action_loss, dist_entropy), each the mean over ppo_epoch * num_mini_batch mini-batches.
        The means are accumulated on the rollouts' device; the only host read is the one that returns them."""
        advantages = rollouts.normalized_advantages()
        acc = None
        for _ in range(self.ppo_epoch):
            for batch in rollouts.feed_forward_generator(advantages, self.num_mini_batch, generator=generator):
                logits, values, pred_mask = self.net(batch.obs_batch)
                out = rollouts.ppo_loss(logits, values, pred_mask if self.mask_coef else None, batch, advantages, clip_param=self.clip_param,
                                        value_loss_coef=self.value_loss_coef, entropy_coef=self.entropy_coef, invalid_coef=self.invalid_coef,
                                        mask_coef=self.mask_coef, use_clipped_value_loss=self.use_clipped_value_loss)
                self.optimizer.zero_grad()
                out.backward()
                if self.max_grad_norm is not None:
                    torch.nn.utils.clip_grad_norm_(self.net.parameters(), self.max_grad_norm)
                self.optimizer.step()
                acc = out.terms[:3].clone() if acc is None else acc + out.terms[:3]
        # the reference's divisor (ppo.py:89), also where T * N // num_mini_batch leaves room for one mini-batch more
        return tuple((acc / (self.ppo_epoch * self.num_mini_batch)).tolist())
