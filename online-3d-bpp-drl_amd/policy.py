"""The CNNPro policy of the reference (acktr/model.py:265-323 with dist.linear, acktr/distributions.py:72) for inference as ONE
native call (include/bpp_policy.h): the five 3x3 layers and the 1x1 head convolutions inside the LDS of a
workgroup, the Linear layers as products over 64 bins, float32 on the matrix cores.

    policy = bpp_amd.NativePolicy.from_checkpoint(path, side=10, n_actions=env.action_space.n).to("cuda:0")
    value, logits, pred = policy(obs)                   # the callable ReorderSearch, MultiBinPacker and MCTSearch take
    value, action, log_prob = policy.act(obs, env.location_masks, deterministic=True)

Sides above 15 (20 x 20 pallets, up to 22) take the one-image form of the trunk kernel (include/bpp_policy_one_image.h):
`NativePolicy(20, 400, form="auto")`; where both forms accept a side they give the same bits.

NativePolicy is inference only; `refresh(module)` repacks the weights after an optimizer step.  A bin's outputs are the same bits
whatever batch it is evaluated in.  CPU tensors go through torch_forward, the same layers in plain torch.

Training (include/bpp_policy_train.h): TrainablePolicy is the same network as an nn.Module whose five 3x3 layers
and 1x1 head convolutions run forward and backward through the native trunk kernels (policy_trunk, an autograd Function); its
Linear layers are torch, or with heads="native" the native head kernels (include/bpp_policy_heads_train.h; DESIGN.md 3.18;
policy_heads, a second autograd Function), so that nothing of the network runs in torch.

    net = bpp_amd.TrainablePolicy(10, env.action_space.n).to("cuda:0")
    value, logits, pred = net(obs); loss.backward(); optimizer.step(); policy.refresh(net)
"""
import ctypes

import torch
import torch.nn.functional as F

from . import _lib
from ._front import Workspace, obs_rows, raw_stream, stream_ptr
from .masks import masked_act

HEADS = ("value", "logits", "pred")
TRUNK = tuple("base.share.%d" % i for i in (0, 2, 4, 6, 8))
HIDDEN_STEP, MAX_HIDDEN = 32, 512                    # what bpp_policy_forward accepts (include/bpp_policy.h)
MAX_SIDE = _lib.POLICY_FORMS["two_images"][2]        # the same: 15
MAX_SIDE_ONE_IMAGE = _lib.POLICY_FORMS["one_image"][2]      # what bpp_policy_forward_one_image accepts (include/bpp_policy_one_image.h): 22
FORMS = tuple(_lib.POLICY_FORMS) + ("auto",)         # auto: two images up to MAX_SIDE, one image above
_WORKSPACE = Workspace()    # (device, stream, geom) -> float32 tensor, grown to the largest n asked for


def layer_shapes(side, hidden, n_actions):
    """[(name, weight shape)] of every layer in the order of the packed blob (include/bpp_policy.h); the three 1x1 head
    convolutions share one matrix there."""
    A = side * side
    return ([(TRUNK[0], (64, 4, 3, 3))] + [(name, (64, 64, 3, 3)) for name in TRUNK[1:]] +
            [("base.actor.0", (8, 64, 1, 1)), ("base.mask.0", (8, 64, 1, 1)), ("base.critic.0", (4, 64, 1, 1)),
             ("base.actor.3", (hidden, 8 * A)), ("dist.linear", (n_actions, hidden)), ("base.mask.3", (hidden, 8 * A)),
             ("base.mask.5", (n_actions, hidden)), ("base.critic.3", (hidden, 4 * A)), ("base.critic_linear", (1, hidden))])


def plain_weights(state, side, hidden, n_actions, device=None):
    """{name.weight / name.bias: float32 tensor} under the reference's Policy.state_dict() names and shapes, from any of: those
    names; the K-FAC-split checkpoint form (`<layer>.module.weight`, `<layer>.add_bias._bias` [C, 1]; main.py:66-76); the
    output of kfac.plain_state_dict.  device: where every tensor is moved to (the entries of `state` may lie on different
    devices); None leaves them where they are.  ValueError for a missing layer or a wrong size."""
    seen = {}
    for k, v in state.items():
        seen[k.replace("module.", "").replace("add_bias.", "").replace("_bias", "bias")] = v
    out = {}
    for name, shape in layer_shapes(side, hidden, n_actions):
        for suffix, want in ((".weight", shape), (".bias", shape[:1])):
            if name + suffix not in seen:
                raise ValueError("the state dict has no %s%s" % (name, suffix))
            v = seen[name + suffix].detach().to(device=device, dtype=torch.float32)
            n = 1
            for d in want:
                n *= d
            if v.numel() != n:
                raise ValueError("%s%s has %d elements, the network needs %r" % (name, suffix, v.numel(), tuple(want)))
            out[name + suffix] = v.reshape(want)
    return out


def pack_weights(weights, side, hidden, n_actions):
    """The float32 blob bpp_policy_forward reads, from plain_weights' output: every matrix [k][oc] (weight.view(OC, -1)
    transposed) followed by its bias, in layer_shapes' order."""
    parts = []
    names = [n for n, _ in layer_shapes(side, hidden, n_actions)]

    def put(ws, bs):
        w = torch.cat([x.reshape(x.shape[0], -1) for x in ws], 0)
        parts.extend([w.t().contiguous().reshape(-1), torch.cat([b.reshape(-1) for b in bs], 0)])

    for name in names[:5]:
        put([weights[name + ".weight"]], [weights[name + ".bias"]])
    put([weights[n + ".weight"] for n in names[5:8]], [weights[n + ".bias"] for n in names[5:8]])
    for name in names[8:]:
        put([weights[name + ".weight"]], [weights[name + ".bias"]])
    return torch.cat([p.to(torch.float32) for p in parts], 0).contiguous()


def unpack_weights(blob, side, hidden, n_actions):
    """pack_weights backwards: plain tensors per layer."""
    out, at = {}, 0
    shapes = layer_shapes(side, hidden, n_actions)

    def take(group):
        nonlocal at
        oc = sum(s[0] for _, s in group)
        k = 1
        for d in group[0][1][1:]:
            k *= d
        w = blob[at:at + k * oc].reshape(k, oc).t()
        b = blob[at + k * oc:at + (k + 1) * oc]
        at += (k + 1) * oc
        c = 0
        for name, s in group:
            out[name + ".weight"] = w[c:c + s[0]].reshape(s).contiguous()
            out[name + ".bias"] = b[c:c + s[0]].contiguous()
            c += s[0]

    for g in [shapes[i:i + 1] for i in range(5)] + [shapes[5:8]] + [shapes[i:i + 1] for i in range(8, len(shapes))]:
        take(g)
    if at != blob.numel():
        raise ValueError("the blob has %d floats, the network %d" % (blob.numel(), at))
    return out


def torch_forward(weights, obs, want=HEADS):
    """(value [n], logits [n, M], pred [n, M]) of CNNPro + dist.linear in plain torch, in the dtype and on the device of
    `weights` (plain_weights' names), None for a head not in `want`: what NativePolicy computes for CPU tensors, and what the
    tests and tools/bench_policy.py compare against."""
    w = weights
    dt = w[TRUNK[0] + ".weight"].dtype
    A = w["base.actor.3.weight"].shape[1] // 8
    side = int(round(A ** 0.5))
    x = obs.to(dt)[:, :4 * A].reshape(-1, 4, side, side)       # CNNPro.forward, acktr/model.py:315-316
    for name in TRUNK:
        x = F.relu(F.conv2d(x, w[name + ".weight"], w[name + ".bias"], padding=1))

    def head(name):
        h = F.relu(F.conv2d(x, w[name + ".0.weight"], w[name + ".0.bias"])).flatten(1)
        return F.relu(F.linear(h, w[name + ".3.weight"], w[name + ".3.bias"]))

    value = logits = pred = None
    if "value" in want:
        value = F.linear(head("base.critic"), w["base.critic_linear.weight"], w["base.critic_linear.bias"]).reshape(-1)
    if "logits" in want:
        logits = F.linear(head("base.actor"), w["dist.linear.weight"], w["dist.linear.bias"])
    if "pred" in want:
        pred = F.relu(F.linear(head("base.mask"), w["base.mask.5.weight"], w["base.mask.5.bias"]))
    return value, logits, pred


def resolve_form(form, side):
    """"two_images" or "one_image": what `form` (one of FORMS) means at this side."""
    if form not in FORMS:
        raise ValueError("form must be one of %r" % (FORMS,))
    if form == "auto":
        return "two_images" if int(side) <= MAX_SIDE else "one_image"
    return form


def max_side(form):
    """The largest side NativePolicy / policy_forward accept under `form`: that of the form it comes to at the largest side."""
    return _lib.POLICY_FORMS[resolve_form(form, MAX_SIDE_ONE_IMAGE)][2]


def forward_info(geom, n, L=None, form="two_images"):
    """bpp_policy_forward_info as a dict (_lib.POLICY_INFO), or bpp_policy_forward_one_image_info (_lib.POLICY_ONE_IMAGE_INFO)
    where `form` comes to "one_image" at this side."""
    symbols, names, _ = _lib.POLICY_FORMS[resolve_form(form, geom[0])]
    return _lib.info_dict(symbols[3], names, 8, _lib.kfac_geom(geom), int(n), L=L)


def policy_forward(obs, weights, geom, want=HEADS, form="two_images"):
    """(value [n], logits [n, M], pred [n, M]) from bpp_policy_forward, None for a head not in `want`: obs float32 [n, >= 4 A]
    on a HIP device with contiguous rows (a view of a storage's rows will do), weights the packed blob on the same device,
    geom = (S, H, M).  Only enqueues on the current stream.

    form (one of FORMS): "two_images" is bpp_policy_forward (S <= 15); "one_image" is bpp_policy_forward_one_image (S <= 22: one
    LDS image per bin, the same blob, workspace and bits); "auto" takes two images up to S = 15 and one image above.

    The workspace is kept per (device, stream, geom) and grown to the largest n asked for.  Inside a stream capture the call
    takes a workspace of its own from the graph's memory pool, as its outputs are, so a captured call keeps its workspace for as
    long as the graph lives.  Make one call before capturing: the first call per device opts the kernels in to more than
    64 KiB of LDS, which is no stream operation and should not happen first inside a capture."""
    S, H, M = (int(v) for v in geom)
    want = tuple(want)
    if not want or any(h not in HEADS for h in want):
        raise ValueError("want must name at least one of %r" % (HEADS,))
    symbols = _lib.POLICY_FORMS[resolve_form(form, S)][0]
    n, stride = obs_rows(obs, S * S, "policy_forward")
    dev = obs.device
    g = _lib.kfac_geom((S, H, M))
    L = _lib.lib()
    forward, workspace, weights_floats, info = (getattr(L, name) for name in symbols)
    floats = int(weights_floats(g))
    if floats == 0:
        _lib.check(info(g, n, (ctypes.c_int32 * 8)()))
    if (not torch.is_tensor(weights) or weights.dtype != torch.float32 or weights.device != dev or not weights.is_contiguous()
            or weights.numel() != floats):
        raise ValueError("weights must be the packed float32 blob of %d floats on %s" % (floats, dev))
    with torch.cuda.device(dev):
        stream = raw_stream(dev)
        ws = _WORKSPACE.take((dev, stream, (S, H, M)), (int(workspace(g, n)) + 3) // 4, torch.float32, dev)
        value = torch.empty(n, dtype=torch.float32, device=dev) if "value" in want else None
        logits = torch.empty((n, M), dtype=torch.float32, device=dev) if "logits" in want else None
        pred = torch.empty((n, M), dtype=torch.float32, device=dev) if "pred" in want else None
        ptr = [t.data_ptr() if t is not None else None for t in (value, logits, pred)]
        _lib.check(forward(obs.data_ptr(), stride, n, g, weights.data_ptr(), ptr[0], ptr[1], ptr[2], ws.data_ptr(), ctypes.c_void_p(stream)))
    return value, logits, pred


class NativePolicy:
    """The reference's Policy(CNNPro) for inference: holds the packed weights, `policy(obs) -> (value [n], logits [n, M],
    pred [n, M])`, the contract of the searches' `policy` argument.  side: the pallet side S (the image is S x S), n_actions: S * S
    or 2 S * S, hidden: 256 in the reference, form: one of FORMS -- "two_images" (bpp_policy_forward, S <= 15), "one_image"
    (bpp_policy_forward_one_image, S <= 22: 20 x 20 pallets) or "auto" (two images up to 15, one above); the weights, act() and
    the outputs' bits do not depend on it.  What the native call refuses is refused here, wherever the tensors live: a side whose
    LDS images per bin do not fit under the form (S > 15 with two images, S > 22 with one), a hidden size that is no multiple of
    32 or above 512."""

    def __init__(self, side, n_actions, hidden=256, device=None, form="two_images"):
        self.side, self.n_actions, self.hidden, self.form = int(side), int(n_actions), int(hidden), form
        most = max_side(form)
        if self.n_actions not in (self.side ** 2, 2 * self.side ** 2):
            raise ValueError("n_actions must be side^2 or 2 side^2")
        if not 1 <= self.side <= most:
            raise ValueError("side must lie in 1 .. %d: the LDS images of a bin must fit (form=%r)" % (most, form))
        if self.hidden < 1 or self.hidden % HIDDEN_STEP or self.hidden > MAX_HIDDEN:
            raise ValueError("hidden must be a multiple of %d, at most %d" % (HIDDEN_STEP, MAX_HIDDEN))
        self.geom = (self.side, self.hidden, self.n_actions)
        floats = sum(s[0] * (1 + _numel(s[1:])) for _, s in layer_shapes(*self._dims()))
        self.weights = torch.zeros(floats, dtype=torch.float32, device=device)
        self._plain = None

    def _dims(self):
        return self.side, self.hidden, self.n_actions

    @property
    def device(self):
        return self.weights.device

    def to(self, device):
        self.weights = self.weights.to(device)
        self._plain = None
        return self

    def load_state_dict(self, state):
        """Pack a state dict in any of the three forms plain_weights takes; its tensors may lie on any devices."""
        blob = pack_weights(plain_weights(state, *self._dims(), device=self.weights.device), *self._dims())
        if blob.numel() != self.weights.numel():
            raise ValueError("packed %d floats, expected %d" % (blob.numel(), self.weights.numel()))
        self.weights.copy_(blob)
        self._plain = None
        return self

    def refresh(self, module_or_state):
        """Repack after an optimizer step: a module (its state_dict()) or a state dict."""
        state = module_or_state.state_dict() if hasattr(module_or_state, "state_dict") else module_or_state
        return self.load_state_dict(state)

    @classmethod
    def from_checkpoint(cls, path, side, n_actions, hidden=256, device=None, form="two_images"):
        """A reference checkpoint: the (state_dict, ob_rms) pair main.py:186-191 saves.  Observation statistics are refused."""
        state, ob_rms = torch.load(path, map_location="cpu", weights_only=False)
        if ob_rms is not None:
            raise ValueError("checkpoint carries observation statistics (VecNormalize ob=True); the BPP checkpoints do not")
        return cls(side, n_actions, hidden, device=device, form=form).load_state_dict(state)

    def unpack(self):
        """{name.weight / name.bias: tensor} of every layer under the reference's names, from the blob."""
        if self._plain is None:
            self._plain = unpack_weights(self.weights, *self._dims())
        return self._plain

    def __call__(self, obs, want=HEADS):
        if obs.device != self.weights.device:
            raise ValueError("obs is on %s, the weights on %s" % (obs.device, self.weights.device))
        obs = obs.reshape(obs.shape[0], -1) if obs.dim() != 2 else obs
        if obs.device.type != "cuda":
            with torch.no_grad():
                return torch_forward(self.unpack(), obs.to(torch.float32), want)
        return policy_forward(obs if obs.dtype == torch.float32 else obs.to(torch.float32), self.weights, self.geom, want, self.form)

    def act(self, obs, location_masks, deterministic=False, **sampler):
        """Policy.act (acktr/model.py:57-68): (value [n, 1], action int64 [n, 1], action_log_probs [n, 1]); the forward, then
        bpp_amd.masked_act on its logits (`sampler`: its seed / step / counter / out arguments)."""
        value, logits, _ = self(obs, want=("value", "logits"))
        action, logp = masked_act(logits, location_masks, deterministic=deterministic, **sampler)
        return value.reshape(-1, 1), action, logp


# ------------------------------------------------------------------------------------------------- training (bpp_policy_train.h)
HEAD_CONVS = ("base.actor.0", "base.mask.0", "base.critic.0")
TRUNK_PARAMETERS = tuple(n + k for n in TRUNK + HEAD_CONVS for k in (".weight", ".bias"))        # the order policy_trunk takes
TRUNK_FLOATS, TRUNK_BWD_FLOATS = _lib.POLICY_TRUNK_FLOATS, _lib.POLICY_TRUNK_BWD_FLOATS


def pack_trunk(weights):
    """The first 151 380 floats of pack_weights' blob -- share.0 .. share.8 and the head convolutions, all that the trunk
    kernels read -- from plain tensors under the reference's names."""
    parts = []
    for names in [(n,) for n in TRUNK] + [HEAD_CONVS]:
        w = torch.cat([weights[n + ".weight"].reshape(weights[n + ".weight"].shape[0], -1) for n in names], 0)
        parts.extend([w.t().reshape(-1), torch.cat([weights[n + ".bias"].reshape(-1) for n in names], 0)])
    return torch.cat([p.to(torch.float32) for p in parts], 0).contiguous()


def pack_trunk_backward(weights):
    """The float32 blob `weights_bwd` of bpp_policy_trunk_backward, from plain tensors under the reference's names: per layer
    share.2 .. share.8 the matrix [k' = oc * 9 + i' * 3 + j'][c] = W[oc][c][2 - i'][2 - j'], then the head convolutions [h][c]."""
    parts = [weights[n + ".weight"].flip(2, 3).permute(0, 2, 3, 1).reshape(-1) for n in TRUNK[1:]]
    parts += [weights[n + ".weight"].reshape(-1) for n in HEAD_CONVS]
    return torch.cat([p.to(torch.float32) for p in parts], 0).contiguous()


def unpack_trunk_gradient(gw):
    """{name: gradient in torch's shape} from bpp_policy_trunk_backward's grad_weights [151 380]: [OC][C][3][3] is a view of
    [k][oc] transposed."""
    out, at = {}, 0
    for names, c, taps in [((n,), 4 if n == TRUNK[0] else 64, 3) for n in TRUNK] + [(HEAD_CONVS, 64, 1)]:
        oc = 64 if taps == 3 else 20
        k = c * taps * taps
        w, b = gw[at:at + k * oc].reshape(k, oc).t(), gw[at + k * oc:at + (k + 1) * oc]
        at += (k + 1) * oc
        o = 0
        for n in names:
            m = 64 if taps == 3 else (4 if n == HEAD_CONVS[2] else 8)
            out[n + ".weight"], out[n + ".bias"] = w[o:o + m].reshape(m, c, taps, taps), b[o:o + m]
            o += m
    return out


def trunk_backward_info(geom, n, L=None):
    """bpp_policy_trunk_backward_info as a dict (_lib.POLICY_TRAIN_INFO)."""
    return _lib.info_dict("bpp_policy_trunk_backward_info", _lib.POLICY_TRAIN_INFO, 8, _lib.kfac_geom(geom), int(n), L=L)


def _check_obs(obs, S):
    """_front.obs_rows for the trunk's calls."""
    return obs_rows(obs, S * S, "the native trunk")


def trunk_forward_train(obs, blob, geom, feat=None, acts=None):
    """(feat [n, 20 A], acts [5, n, 64, S, S]) from bpp_policy_trunk_forward_train: obs as policy_forward takes it, blob the
    packed weights (pack_trunk's 151 380 floats, or the whole blob of pack_weights).  feat / acts: buffers to write into.  Only
    enqueues on the current stream."""
    S, H, M = (int(v) for v in geom)
    n, stride = _check_obs(obs, S)
    dev, A = obs.device, S * S
    if not torch.is_tensor(blob) or blob.dtype != torch.float32 or blob.device != dev or not blob.is_contiguous() or blob.numel() < TRUNK_FLOATS:
        raise ValueError("the weights must be a packed float32 blob of at least %d floats on %s" % (TRUNK_FLOATS, dev))
    feat = torch.empty((n, 20 * A), dtype=torch.float32, device=dev) if feat is None else feat
    acts = torch.empty((5, n, 64, S, S), dtype=torch.float32, device=dev) if acts is None else acts
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().bpp_policy_trunk_forward_train(obs.data_ptr(), stride, n, _lib.kfac_geom((S, H, M)), blob.data_ptr(), feat.data_ptr(),
                                                             acts.data_ptr(), stream_ptr(dev)))
    return feat, acts


def trunk_backward(obs, geom, blob_bwd, feat, acts, grad_feat, grads=None, grad_weights=None, workspace=None):
    """(grads [5 n 64 A + n 20 A] flat: G_1 .. G_5 then gf', grad_weights [151 380]) from bpp_policy_trunk_backward.  grads /
    grad_weights / workspace: buffers to use (workspace: float32, at least bpp_policy_trunk_backward_workspace bytes)."""
    S, H, M = (int(v) for v in geom)
    n, stride = _check_obs(obs, S)
    dev, A = obs.device, S * S
    g = _lib.kfac_geom((S, H, M))
    L = _lib.lib()
    for name, t, numel in (("blob_bwd", blob_bwd, TRUNK_BWD_FLOATS), ("feat", feat, n * 20 * A), ("acts", acts, 5 * n * 64 * A),
                           ("grad_feat", grad_feat, n * 20 * A)):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous() or t.numel() != numel:
            raise ValueError("%s must be a contiguous float32 tensor of %d elements on %s" % (name, numel, dev))
    need = int(L.bpp_policy_trunk_backward_workspace(g, n))
    if need == 0:
        _lib.check(L.bpp_policy_trunk_backward_info(g, n, (ctypes.c_int32 * 8)()))
    grads = torch.empty(n * (5 * 64 + 20) * A, dtype=torch.float32, device=dev) if grads is None else grads
    grad_weights = torch.empty(TRUNK_FLOATS, dtype=torch.float32, device=dev) if grad_weights is None else grad_weights
    workspace = torch.empty(need // 4, dtype=torch.float32, device=dev) if workspace is None else workspace
    with torch.cuda.device(dev):
        _lib.check(L.bpp_policy_trunk_backward(obs.data_ptr(), stride, n, g, blob_bwd.data_ptr(), feat.data_ptr(), acts.data_ptr(),
                                               grad_feat.data_ptr(), grads.data_ptr(), grad_weights.data_ptr(), workspace.data_ptr(),
                                               workspace.numel() * 4, stream_ptr(dev)))
    return grads, grad_weights


class _TrunkBuffers:
    """What one (n, device, side) needs between a forward and its backward passes, and both blobs with the parameter versions
    they were packed from."""

    def __init__(self):
        self.versions = self.blob = self.blob_bwd = self.acts = self.grads = self.workspace = None
        self.forwards = 0


_TRUNK_BUFFERS = {}     # (n, device, side) -> _TrunkBuffers: policy_trunk's default cache (a module brings its own)


def clear_trunk_buffers():
    """Release what policy_trunk's default cache holds (activations, gradients, workspace, blobs of every batch size seen)."""
    _TRUNK_BUFFERS.clear()


class _PolicyTrunk(torch.autograd.Function):
    @staticmethod
    def forward(ctx, obs, side, cache, keep, *params):
        S = int(side)
        if len(params) != len(TRUNK_PARAMETERS):
            raise ValueError("policy_trunk takes the %d tensors of TRUNK_PARAMETERS" % len(TRUNK_PARAMETERS))
        n = int(obs.shape[0])
        key = (n, obs.device, S)
        buf = cache.get(key)
        if buf is None:
            buf = cache[key] = _TrunkBuffers()
        versions = tuple((p.data_ptr(), p._version) for p in params)
        if buf.versions != versions:
            plain = {name: p.detach() for name, p in zip(TRUNK_PARAMETERS, params)}
            buf.blob, buf.blob_bwd, buf.versions = pack_trunk(plain), pack_trunk_backward(plain), versions
        geom = (S, HIDDEN_STEP, S * S)          # H and M do not enter the trunk
        if not keep:                                # nothing will be differentiated: the kept activations stay as they are
            return trunk_forward_train(obs, buf.blob, geom)[0]
        if buf.acts is None:
            A = S * S
            need = int(_lib.lib().bpp_policy_trunk_backward_workspace(_lib.kfac_geom(geom), n))
            buf.acts = torch.empty((5, n, 64, S, S), dtype=torch.float32, device=obs.device)
            buf.grads = torch.empty(n * (5 * 64 + 20) * A, dtype=torch.float32, device=obs.device)
            buf.workspace = torch.empty(max(1, need // 4), dtype=torch.float32, device=obs.device)
        feat, _ = trunk_forward_train(obs, buf.blob, geom, acts=buf.acts)
        ctx.save_for_backward(obs, feat)
        buf.forwards += 1
        ctx.buf, ctx.geom, ctx.blob_bwd, ctx.stamp = buf, geom, buf.blob_bwd, buf.forwards
        return feat

    @staticmethod
    def backward(ctx, grad_feat):
        obs, feat = ctx.saved_tensors
        buf = ctx.buf
        if buf.forwards != ctx.stamp:
            raise RuntimeError("policy_trunk: another forward of the same batch size has overwritten the activations of this graph")
        _, gw = trunk_backward(obs, ctx.geom, ctx.blob_bwd, feat, buf.acts, grad_feat.contiguous(), grads=buf.grads, workspace=buf.workspace)
        named = unpack_trunk_gradient(gw)
        return (None,) * 4 + tuple(named[name] if ctx.needs_input_grad[4 + i] else None for i, name in enumerate(TRUNK_PARAMETERS))


def policy_trunk(obs, trunk_parameters, side, cache=None):
    """feat [n, 20 A] = the head features of CNNPro's trunk (five 3x3 layers, three 1x1 head convolutions, all with ReLU) for
    obs float32 [n, >= 4 A] on a HIP device, differentiable with respect to trunk_parameters: the 16 tensors of TRUNK_PARAMETERS
    (a dict under those names, or a sequence in that order), in torch's shapes.  Forward and backward are the native calls of
    include/bpp_policy_train.h; no gradient is computed with respect to obs, and an obs that requires one is refused.

    The activations of a forward are kept per (n, device, side) until the next differentiable forward of the same key:
    backward passes over one graph may be repeated (retain_graph=True) and give the same bits, a backward after a newer such
    forward is refused.  A forward under no_grad, or with no parameter that requires grad, keeps nothing and disturbs nothing.
    The buffers (activations 5 n 64 A floats, gradients slightly more, the workspace, both blobs, re-packed when a parameter's
    version changes) live in `cache`, a dict the caller owns -- TrainablePolicy gives its own, so they go with the module; the
    default is one dict for the process, which clear_trunk_buffers() empties.  Callers with different parameters that share a
    cache re-pack the blobs at every alternation: give each its own."""
    if torch.is_tensor(obs) and obs.requires_grad:
        raise ValueError("policy_trunk computes no gradient with respect to obs: pass obs.detach()")
    if isinstance(trunk_parameters, dict):
        trunk_parameters = [trunk_parameters[name] for name in TRUNK_PARAMETERS]
    S = int(side)
    if not 1 <= S <= MAX_SIDE:
        raise ValueError("side must lie in 1 .. %d: the two LDS images of a bin must fit" % MAX_SIDE)
    obs = obs.reshape(obs.shape[0], -1) if obs.dim() != 2 else obs
    _check_obs(obs, S)
    keep = torch.is_grad_enabled() and any(p.requires_grad for p in trunk_parameters)
    return _PolicyTrunk.apply(obs, S, _TRUNK_BUFFERS if cache is None else cache, keep, *trunk_parameters)


# ------------------------------------------------------------------------------- training of the heads (bpp_policy_heads_train.h)
HEAD_LINEARS = ("base.actor.3", "dist.linear", "base.mask.3", "base.mask.5", "base.critic.3", "base.critic_linear")    # the blob's order
HEAD_PARAMETERS = tuple(n + k for n in HEAD_LINEARS for k in (".weight", ".bias"))               # the order policy_heads takes
HEADS_MODES = ("torch", "native")


def pack_heads(weights):
    """pack_weights' blob from float 151 380 on -- the six Linear layers, all that the head kernels read -- from plain tensors
    under the reference's names: every matrix [k][oc], its bias behind it."""
    parts = []
    for n in HEAD_LINEARS:
        parts.extend([weights[n + ".weight"].t().reshape(-1), weights[n + ".bias"].reshape(-1)])
    return torch.cat([p.to(torch.float32) for p in parts], 0).contiguous()


def pack_heads_backward(weights):
    """The float32 blob `weights_bwd` of bpp_policy_heads_backward, from plain tensors under the reference's names: the six
    matrices in torch's own [out][in] layout, per head (actor, mask, critic) the second Linear in front of the first."""
    order = (HEAD_LINEARS[1], HEAD_LINEARS[0], HEAD_LINEARS[3], HEAD_LINEARS[2], HEAD_LINEARS[5], HEAD_LINEARS[4])
    return torch.cat([weights[n + ".weight"].to(torch.float32).reshape(-1) for n in order], 0).contiguous()


def unpack_heads_gradient(gw, side, hidden, n_actions):
    """{name: gradient in torch's shape} from bpp_policy_heads_backward's grad_weights: [out][in] is a view of [k][oc]
    transposed."""
    out, at = {}, 0
    for name, (oc, k) in layer_shapes(side, hidden, n_actions)[8:]:
        out[name + ".weight"], out[name + ".bias"] = gw[at:at + k * oc].reshape(k, oc).t(), gw[at + k * oc:at + (k + 1) * oc]
        at += (k + 1) * oc
    if at != gw.numel():
        raise ValueError("grad_weights has %d floats, the six Linear layers %d" % (gw.numel(), at))
    return out


def heads_backward_info(geom, n, L=None):
    """bpp_policy_heads_backward_info as a dict (_lib.POLICY_HEADS_TRAIN_INFO)."""
    return _lib.info_dict("bpp_policy_heads_backward_info", _lib.POLICY_HEADS_TRAIN_INFO, 8, _lib.kfac_geom(geom), int(n), L=L)


def _heads_tensor(name, t, numel, dev):
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous() or t.numel() != numel:
        raise ValueError("%s must be a contiguous float32 tensor of %d elements on %s" % (name, numel, dev))
    return t


def _check_feat(feat, A):
    if not torch.is_tensor(feat) or feat.dtype != torch.float32 or feat.dim() != 2 or feat.shape[0] < 1 or feat.shape[1] != 20 * A:
        raise ValueError("feat must be a float32 [n, 20 A] tensor with n >= 1")
    if feat.device.type != "cuda":
        raise RuntimeError("the native heads need their tensors on a HIP device")
    if not feat.is_contiguous():
        raise ValueError("feat must be contiguous")
    return int(feat.shape[0])


def heads_forward_train(feat, blob, geom, value=None, logits=None, pred=None, hidden=None):
    """(value [n], logits [n, M], pred [n, M], hidden [3, n, H]) from bpp_policy_heads_forward_train: feat float32 [n, 20 A] as
    trunk_forward_train wrote it, blob the whole packed blob of pack_weights (only the floats from 151 380 on are read).
    value / logits / pred / hidden: buffers to write into.  Only enqueues on the current stream."""
    S, H, M = (int(v) for v in geom)
    n = _check_feat(feat, S * S)
    dev = feat.device
    g = _lib.kfac_geom((S, H, M))
    L = _lib.lib()
    floats = int(L.bpp_policy_one_image_weights_floats(g))
    if floats == 0:
        _lib.check(L.bpp_policy_heads_backward_info(g, n, (ctypes.c_int32 * 8)()))
    _heads_tensor("blob", blob, floats, dev)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)      # noqa: E731
    value = new(n) if value is None else _heads_tensor("value", value, n, dev)
    logits = new(n, M) if logits is None else _heads_tensor("logits", logits, n * M, dev)
    pred = new(n, M) if pred is None else _heads_tensor("pred", pred, n * M, dev)
    hidden = new(3, n, H) if hidden is None else _heads_tensor("hidden", hidden, 3 * n * H, dev)
    with torch.cuda.device(dev):
        _lib.check(L.bpp_policy_heads_forward_train(feat.data_ptr(), n, g, blob.data_ptr(), value.data_ptr(), logits.data_ptr(), pred.data_ptr(),
                                                    hidden.data_ptr(), stream_ptr(dev)))
    return value, logits, pred, hidden


def heads_backward(feat, hidden, pred, grad_value, grad_logits, grad_pred, geom, blob_bwd, grad_feat=None, grad_hidden=None,
                   grad_out_mask=None, grad_weights=None, workspace=None):
    """(grad_feat [n, 20 A], grad_hidden [3, n, H], grad_out_mask [n, M], grad_weights) from bpp_policy_heads_backward.
    grad_value [n] / grad_logits [n, M] / grad_pred [n, M]: None for a head that contributes nothing (zeros are written for it).
    The other keyword arguments: buffers to use (workspace: float32, at least bpp_policy_heads_backward_workspace bytes)."""
    S, H, M = (int(v) for v in geom)
    n = _check_feat(feat, S * S)
    dev, A = feat.device, S * S
    g = _lib.kfac_geom((S, H, M))
    L = _lib.lib()
    need = int(L.bpp_policy_heads_backward_workspace(g, n))
    if need == 0:
        _lib.check(L.bpp_policy_heads_backward_info(g, n, (ctypes.c_int32 * 8)()))
    if grad_value is None and grad_logits is None and grad_pred is None:
        raise ValueError("at least one of grad_value, grad_logits and grad_pred must be given")
    floats = int(L.bpp_policy_one_image_weights_floats(g)) - TRUNK_FLOATS
    for name, t, numel in (("hidden", hidden, 3 * n * H), ("pred", pred, n * M), ("grad_value", grad_value, n), ("grad_logits", grad_logits, n * M),
                           ("grad_pred", grad_pred, n * M), ("blob_bwd", blob_bwd, int(L.bpp_policy_heads_backward_weights_floats(g))),
                           ("grad_feat", grad_feat, n * 20 * A), ("grad_hidden", grad_hidden, 3 * n * H), ("grad_out_mask", grad_out_mask, n * M),
                           ("grad_weights", grad_weights, floats)):
        if t is not None or name in ("hidden", "pred", "blob_bwd"):
            _heads_tensor(name, t, numel, dev)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)      # noqa: E731
    grad_feat = new(n, 20 * A) if grad_feat is None else grad_feat
    grad_hidden = new(3, n, H) if grad_hidden is None else grad_hidden
    grad_out_mask = new(n, M) if grad_out_mask is None else grad_out_mask
    grad_weights = new(floats) if grad_weights is None else grad_weights
    workspace = new(max(1, need // 4)) if workspace is None else workspace
    if not torch.is_tensor(workspace) or workspace.dtype != torch.float32 or workspace.device != dev or not workspace.is_contiguous():
        raise ValueError("workspace must be a contiguous float32 tensor on %s" % dev)
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    with torch.cuda.device(dev):
        _lib.check(L.bpp_policy_heads_backward(feat.data_ptr(), hidden.data_ptr(), pred.data_ptr(), ptr(grad_value), ptr(grad_logits), ptr(grad_pred),
                                               n, g, blob_bwd.data_ptr(), grad_feat.data_ptr(), grad_hidden.data_ptr(), grad_out_mask.data_ptr(),
                                               grad_weights.data_ptr(), workspace.data_ptr(), workspace.numel() * 4, stream_ptr(dev)))
    return grad_feat, grad_hidden, grad_out_mask, grad_weights


class _HeadsBuffers:
    """What one (n, device, side, H, M) needs between a forward and its backward passes, and both blobs with the parameter
    versions they were packed from."""

    def __init__(self):
        self.versions = self.blob = self.blob_bwd = self.hidden = self.grad_hidden = self.grad_out_mask = self.workspace = None
        self.forwards = 0


_HEADS_BUFFERS = {}     # (n, device, side, H, M) -> _HeadsBuffers: policy_heads' default cache (a module brings its own)


def clear_heads_buffers():
    """Release what policy_heads' default cache holds."""
    _HEADS_BUFFERS.clear()


class _PolicyHeads(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, geom, cache, keep, *params):
        S, H, M = geom
        n, dev = int(feat.shape[0]), feat.device
        ctx.set_materialize_grads(False)            # an output that takes no part reaches the backward as None: that head's NULL
        key = (n, dev, S, H, M)
        buf = cache.get(key)
        if buf is None:
            buf = cache[key] = _HeadsBuffers()
        versions = tuple((p.data_ptr(), p._version) for p in params)
        if buf.versions != versions:
            plain = {name: p.detach() for name, p in zip(HEAD_PARAMETERS, params)}
            tail = pack_heads(plain)
            if buf.blob is None:                    # the trunk's part of the blob is never read by the head kernels
                buf.blob = torch.zeros(TRUNK_FLOATS + tail.numel(), dtype=torch.float32, device=dev)
            buf.blob[TRUNK_FLOATS:] = tail
            buf.blob_bwd, buf.versions = pack_heads_backward(plain), versions
        if not keep:                                # nothing will be differentiated: the kept hidden vectors stay as they are
            return heads_forward_train(feat, buf.blob, geom)[:3]
        if buf.hidden is None:
            need = int(_lib.lib().bpp_policy_heads_backward_workspace(_lib.kfac_geom(geom), n))
            buf.hidden = torch.empty((3, n, H), dtype=torch.float32, device=dev)
            buf.grad_hidden = torch.empty((3, n, H), dtype=torch.float32, device=dev)
            buf.grad_out_mask = torch.empty((n, M), dtype=torch.float32, device=dev)
            buf.workspace = torch.empty(max(1, need // 4), dtype=torch.float32, device=dev)
        value, logits, pred, _ = heads_forward_train(feat, buf.blob, geom, hidden=buf.hidden)
        ctx.save_for_backward(feat, pred)
        buf.forwards += 1
        ctx.buf, ctx.geom, ctx.blob_bwd, ctx.stamp = buf, geom, buf.blob_bwd, buf.forwards
        return value, logits, pred

    @staticmethod
    def backward(ctx, grad_value, grad_logits, grad_pred):
        feat, pred = ctx.saved_tensors
        buf = ctx.buf
        if buf.forwards != ctx.stamp:
            raise RuntimeError("policy_heads: another forward of the same batch size has overwritten the hidden vectors of this graph")
        dense = lambda g: None if g is None else g.to(torch.float32).contiguous()      # noqa: E731
        grad_feat, _, _, gw = heads_backward(feat, buf.hidden, pred, dense(grad_value), dense(grad_logits), dense(grad_pred), ctx.geom, ctx.blob_bwd,
                                             grad_hidden=buf.grad_hidden, grad_out_mask=buf.grad_out_mask, workspace=buf.workspace)
        named = unpack_heads_gradient(gw, *ctx.geom)
        return (grad_feat if ctx.needs_input_grad[0] else None, None, None, None) + tuple(
            named[name] if ctx.needs_input_grad[4 + i] else None for i, name in enumerate(HEAD_PARAMETERS))


def policy_heads(feat, head_parameters, side, n_actions, hidden, cache=None):
    """(value [n], logits [n, M], pred [n, M]) = the six Linear layers of CNNPro's three heads on feat float32 [n, 20 A] on a
    HIP device (what policy_trunk returns), differentiable with respect to feat and to head_parameters: the 12 tensors of
    HEAD_PARAMETERS (a dict under those names, or a sequence in that order), in torch's shapes.  Forward and backward are the
    native calls of include/bpp_policy_heads_train.h; the backward hands grad_feat on to whatever produced feat.

    policy_trunk's rules hold: the hidden vectors of a forward are kept per (n, device, side) until the next differentiable
    forward of the same key; backward passes over one graph may be repeated and give the same bits, a backward after a newer
    such forward is refused; a forward under no_grad, or with nothing that requires grad, keeps nothing.  The buffers and both
    blobs (re-packed when a parameter's version changes) live in `cache`, a dict the caller owns; the default is one dict for
    the process, which clear_heads_buffers() empties.  An output that takes no part in the loss contributes zeros."""
    if isinstance(head_parameters, dict):
        head_parameters = [head_parameters[name] for name in HEAD_PARAMETERS]
    head_parameters = list(head_parameters)
    if len(head_parameters) != len(HEAD_PARAMETERS):
        raise ValueError("policy_heads takes the %d tensors of HEAD_PARAMETERS" % len(HEAD_PARAMETERS))
    geom = (int(side), int(hidden), int(n_actions))
    if not 1 <= geom[0] <= MAX_SIDE_ONE_IMAGE:
        raise ValueError("side must lie in 1 .. %d" % MAX_SIDE_ONE_IMAGE)
    _check_feat(feat, geom[0] ** 2)
    for name, p in zip(HEAD_PARAMETERS, head_parameters):
        if not torch.is_tensor(p) or p.device != feat.device:
            raise ValueError("%s is on %s, feat on %s" % (name, getattr(p, "device", None), feat.device))
    keep = torch.is_grad_enabled() and (feat.requires_grad or any(p.requires_grad for p in head_parameters))
    return _PolicyHeads.apply(feat, geom, _HEADS_BUFFERS if cache is None else cache, keep, *head_parameters)


class TrainablePolicy(torch.nn.Module):
    """The reference's Policy(CNNPro) for training: parameters under the reference's names (`base.share.0.weight` ...
    `dist.linear.bias`), the trunk and the head convolutions through policy_trunk.  heads="torch" (the default): the Linear
    layers in torch; heads="native": through policy_heads, so that nothing of the network runs in torch.
    forward(obs) -> (value [n], logits [n, M], pred [n, M]) as NativePolicy returns them.  On CPU tensors the forward is
    torch_forward on the same parameters (no native code, for inspection only)."""

    def __init__(self, side, n_actions, hidden=256, heads="torch"):
        super().__init__()
        if heads not in HEADS_MODES:
            raise ValueError("heads must be one of %r" % (HEADS_MODES,))
        NativePolicy(side, n_actions, hidden)                 # its refusals
        self._trunk_cache = {}                                # policy_trunk's buffers, per batch size: released with the module
        self._heads_cache, self._last = {}, None              # policy_heads' buffers; the keys of the last differentiable forward
        self.heads = heads
        self.side, self.n_actions, self.hidden = int(side), int(n_actions), int(hidden)
        relu = torch.nn.init.calculate_gain("relu")
        for name, shape in layer_shapes(self.side, self.hidden, self.n_actions):
            at = self
            for part in name.split("."):                      # plain containers: only the names matter
                if part not in at._modules:
                    at.add_module(part, torch.nn.Module())
                at = at._modules[part]
            w = torch.empty(shape)
            torch.nn.init.orthogonal_(w, gain=0.01 if name == "dist.linear" else relu)     # acktr/model.py:268, distributions.py:65
            at.weight, at.bias = torch.nn.Parameter(w), torch.nn.Parameter(torch.zeros(shape[0]))

    def named_weights(self):
        """{reference name: parameter}"""
        return dict(self.named_parameters())

    def release_buffers(self):
        """Drop the activations, gradients and workspaces kept for the batch sizes seen so far (21 GB at n = 65 536)."""
        self._trunk_cache.clear()
        self._heads_cache.clear()
        self._last = None

    def kept(self):
        """The dense tensors the last differentiable forward (and its backward, once it has run) left on the device, as views of
        the module's buffers, None before such a forward: `acts` [5, n, 64, S, S] and `grads` (flat: G_1 .. G_5 [n, 64, A] each,
        then the masked head gradient [n, 20 A]) of the trunk -- the sources of BPP_KFAC_PATCH and BPP_KFAC_NCHW -- and, with
        heads="native", `hidden` [3, n, H], `grad_hidden` [3, n, H] and `grad_out_mask` [n, M], which with the gradients at
        logits and value are the BPP_KFAC_ROWS sources of the six Linear layers.  This is what a K-FAC hook-up of the native
        network will read; nothing uses it yet."""
        if self._last is None:
            return None
        trunk, heads = (c.get(k) for c, k in zip((self._trunk_cache, self._heads_cache), self._last))
        out = dict(acts=trunk.acts, grads=trunk.grads) if trunk is not None else {}
        if heads is not None:
            out.update(hidden=heads.hidden, grad_hidden=heads.grad_hidden, grad_out_mask=heads.grad_out_mask)
        return out

    def load_state_dict(self, state, strict=True, assign=False):
        """A state dict in any of the three forms plain_weights takes (the reference's names, the K-FAC-split checkpoint form,
        kfac.plain_state_dict's output), not only this module's own.  Every layer must be there whatever `strict` says
        (ValueError otherwise, as NativePolicy.load_state_dict raises); strict=True also refuses a key that names no layer.
        Returns nn.Module's (missing_keys, unexpected_keys) result; `assign` is not supported."""
        if assign:
            raise ValueError("TrainablePolicy.load_state_dict copies into its parameters: assign=True is not supported")
        plain = plain_weights(state, self.side, self.hidden, self.n_actions)
        known = {k.replace("module.", "").replace("add_bias.", "").replace("_bias", "bias"): k for k in state}
        unexpected = [k for name, k in known.items() if name not in plain]
        if strict and unexpected:
            raise RuntimeError("unexpected key(s) in state_dict: %s" % ", ".join(sorted(unexpected)))
        with torch.no_grad():
            for name, p in self.named_weights().items():
                p.copy_(plain[name].to(p.device))
        return torch.nn.modules.module._IncompatibleKeys([], unexpected)

    def forward(self, obs):
        w = self.named_weights()
        obs = obs.reshape(obs.shape[0], -1) if obs.dim() != 2 else obs
        if obs.device.type != "cuda":
            return torch_forward(w, obs.to(torch.float32))
        A = self.side ** 2
        feat = policy_trunk(obs if obs.dtype == torch.float32 else obs.to(torch.float32), w, self.side, cache=self._trunk_cache)
        if feat.requires_grad:
            n = int(feat.shape[0])
            self._last = ((n, feat.device, self.side), (n, feat.device, self.side, self.hidden, self.n_actions))
        if self.heads == "native":
            return policy_heads(feat, w, self.side, self.n_actions, self.hidden, cache=self._heads_cache)

        def head(name, lo, hi):
            return F.relu(F.linear(feat[:, lo * A:hi * A], w[name + ".3.weight"], w[name + ".3.bias"]))

        value = F.linear(head("base.critic", 16, 20), w["base.critic_linear.weight"], w["base.critic_linear.bias"]).reshape(-1)
        logits = F.linear(head("base.actor", 0, 8), w["dist.linear.weight"], w["dist.linear.bias"])
        pred = F.relu(F.linear(head("base.mask", 8, 16), w["base.mask.5.weight"], w["base.mask.5.bias"]))
        return value, logits, pred


def _numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n
