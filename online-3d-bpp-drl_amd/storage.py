"""RolloutStorage -- the reference's rollout buffer (acktr/storage.py) held in [rows][N] slabs, with the returns computed by
ONE native call (include/bpp_rollout.h) and, on the device, filled by the step kernel itself.

Same attribute names, shapes and dtypes as the reference's class, so `ACKTR.update(rollouts)` and `Policy.evaluate_actions`
take it unchanged: obs [T+1,N,*], recurrent_hidden_states, rewards [T,N,1], value_preds, returns, action_log_probs, actions
(int64), masks, bad_masks, location_masks [T+1,N,M], num_steps, step.  rewards[t], masks[t], ... are contiguous [N,1] views.

Zero-copy path (a storage on the env's device): slot t + 1 of the storage IS the output set of lock-step t --
`storage.reset(env)` lets the reset write observation and mask into slot 0, `storage.step(env, actions, value, log_prob)`
enqueues one lock-step whose bpp_step_out points into the slabs (obs[t+1], location_masks[t+1], rewards[t], and the per-step
done / counter / ratio / ep_ret / ep_len rows), and `env.rollout_uniform_sets(..., sets=storage.output_sets())` lets the
pipelined driver do the same for T lock-steps.  No environment output is copied.  `masks` rows written this way are derived
from the step kernel's `done` bytes inside compute_returns (masks[t+1] = done[t] ? 0 : 1): they are valid after that call,
which is where the reference's update reads them.

A storage on the CPU takes the reference's insert() path and the host entry point of the same native recurrence: an explicit
twin, not a fallback -- a storage on a device without the library's kernels does not exist.
"""
import torch

from . import _lib
from ._front import stream_ptr
from .vec_env import StepTensors

_SMALL = (("rewards", torch.float32), ("done", torch.uint8), ("counter", torch.int32), ("ratio", torch.float64),
          ("ep_ret", torch.float64), ("ep_len", torch.int32))


class RolloutStorage(object):
    def __init__(self, num_steps, env_or_num_envs, obs_shape, action_space, recurrent_hidden_state_size=1, device=None):
        env = None if isinstance(env_or_num_envs, int) else env_or_num_envs
        N = int(env_or_num_envs) if env is None else int(env.num_envs)
        T = int(num_steps)
        if T < 1 or N < 1:
            raise ValueError("num_steps and the number of bins must be >= 1")
        if action_space.__class__.__name__ != "Discrete":
            raise ValueError("RolloutStorage holds the packing environment's Discrete actions")
        if device is None:
            device = env.device if env is not None else "cpu"
        self.num_steps, self.num_envs, self.step_index = T, N, 0
        M = int(action_space.n)           # one mask entry per action (acktr/storage.py:27-32 for both rotation settings)
        z = dict(device=torch.device(device))
        # every per-bin scalar lives in a [rows][N] slab; the small outputs of the step kernel have T + 1 rows, row s written
        # by the lock-step (or reset) whose output set is slot s -- the public views start at row 1
        self._slabs = {"obs": torch.zeros((T + 1, N) + tuple(obs_shape), **z),
                       "location_masks": torch.zeros((T + 1, N, M), **z),
                       "recurrent_hidden_states": torch.zeros((T + 1, N, int(recurrent_hidden_state_size)), **z),
                       "value_preds": torch.zeros((T + 1, N), **z), "returns": torch.zeros((T + 1, N), **z),
                       "action_log_probs": torch.zeros((T, N), **z), "actions": torch.zeros((T, N), dtype=torch.int64, **z),
                       "masks": torch.ones((T + 1, N), **z), "bad_masks": torch.ones((T + 1, N), **z)}
        for name, dtype in _SMALL:
            self._slabs[name] = torch.zeros((T + 1, N), dtype=dtype, **z)
        self._from_done = [False] * T      # row t of the current rollout: written by a lock-step (done bytes) / by insert() (masks)
        self._bind()

    # ------------------------------------------------------------------ views
    def _bind(self):
        s = self._slabs
        self.device = s["obs"].device
        self.obs, self.location_masks, self.recurrent_hidden_states = s["obs"], s["location_masks"], s["recurrent_hidden_states"]
        for name in ("value_preds", "returns", "action_log_probs", "actions", "masks", "bad_masks"):
            setattr(self, name, s[name].unsqueeze(-1))
        self.rewards = s["rewards"][1:].unsqueeze(-1)
        # the infos of every lock-step of the rollout, [T][N]: one scan per update instead of one per step (main.py:159-162)
        self.done, self.counter, self.ratio = s["done"][1:], s["counter"][1:], s["ratio"][1:]
        self.ep_ret, self.ep_len = s["ep_ret"][1:], s["ep_len"][1:]
        self._slots = None

    @property
    def step(self):
        """The reference's `step` attribute (the row the next insert / lock-step fills) -- and, called with an env, the
        zero-copy lock-step: see lockstep()."""
        return _Step(self)

    @step.setter
    def step(self, value):
        self.step_index = int(value) % self.num_steps

    def _slot(self, k):
        """(StepTensors, bpp_step_out) whose buffers are slot k of the slabs."""
        if self.device.type != "cuda":
            raise RuntimeError("the step kernel writes into a storage on its own device; a CPU storage is filled with insert()")
        if self._slots is None:
            s = self._slabs
            self._slots = []
            for j in range(self.num_steps + 1):
                res = StepTensors(obs=s["obs"][j], mask=s["location_masks"][j], reward=s["rewards"][j].unsqueeze(-1), done=s["done"][j],
                                  counter=s["counter"][j], ratio=s["ratio"][j], ep_ret=s["ep_ret"][j], ep_len=s["ep_len"][j])
                out = _lib.StepOut(*[getattr(res, f).data_ptr() for f in ("obs", "mask", "reward", "done", "counter", "ratio", "ep_ret", "ep_len")])
                self._slots.append((res, out))
        return self._slots[k]

    def _check_env(self, env):
        if env.num_envs != self.num_envs or env.device != self.device:
            raise ValueError("the env has %d bins on %s, the storage %d on %s" % (env.num_envs, env.device, self.num_envs, self.device))
        if tuple(self.obs.shape[2:]) != (env.obs_len,) or self.location_masks.shape[2] != env.act_len:
            raise ValueError("the storage's observation / mask rows do not have the env's lengths")

    # ------------------------------------------------------------------ zero-copy path
    def reset(self, env):
        """env.reset() whose observation and mask land in slot 0; returns obs[0].  Starts a rollout at row 0."""
        self._check_env(env)
        self.step_index = 0
        return env.reset(out=self._slot(0))

    def lockstep(self, env, actions, value=None, action_log_prob=None):
        """ONE lock-step of `env` whose outputs are row `step` of the storage (obs[step+1], location_masks[step+1],
        rewards[step], done / counter / ratio / ep_ret / ep_len[step]): nothing the environment produces is copied.  The
        caller's actions int64 [N] or [N,1], value and action_log_prob [N,1] are recorded in actions / value_preds /
        action_log_probs[step].  Returns the StepTensors of the slot; never synchronises."""
        self._check_env(env)
        t = self.step_index
        self._slabs["actions"][t].copy_(actions.reshape(-1))
        if value is not None:
            self._slabs["value_preds"][t].copy_(value.reshape(-1))
        if action_log_prob is not None:
            self._slabs["action_log_probs"][t].copy_(action_log_prob.reshape(-1))
        res = env.step_tensors(actions, out=self._slot(t + 1))
        self._from_done[t] = True
        self.step_index = (t + 1) % self.num_steps
        return res

    def output_sets(self):
        """Slots 1 .. T as the `sets` of BppVecEnv.rollout_uniform_sets: with these T sets lock-step t of the driver lands in
        slot t + 1.  The rollout they fill starts at row 0 and takes its masks from the done bytes.  The slots stay the
        storage's: after the driver's call slot T is the env's current result (its location_masks), but never the env's own
        output set -- a later env.reset() or env.step_tensors() without out= writes the env's buffers, not the slabs."""
        sets = [self._slot(j) for j in range(1, self.num_steps + 1)]
        self._from_done = [True] * self.num_steps
        self.step_index = 0
        return sets

    # ------------------------------------------------------------------ the reference's surface (acktr/storage.py)
    def to(self, device):
        self._slabs = {k: v.to(device) for k, v in self._slabs.items()}
        self._bind()

    def insert(self, obs, recurrent_hidden_states, actions, action_log_probs, value_preds, rewards, masks, bad_masks, location_masks):
        t = self.step_index
        self.obs[t + 1].copy_(obs)
        self.recurrent_hidden_states[t + 1].copy_(recurrent_hidden_states)
        self.actions[t].copy_(actions)
        self.action_log_probs[t].copy_(action_log_probs)
        self.value_preds[t].copy_(value_preds)
        self.rewards[t].copy_(rewards)
        self.masks[t + 1].copy_(masks)
        self.bad_masks[t + 1].copy_(bad_masks)
        self.location_masks[t + 1].copy_(location_masks)
        self._from_done[t] = False
        self.step_index = (t + 1) % self.num_steps

    def after_update(self):
        self.obs[0].copy_(self.obs[-1])
        self.recurrent_hidden_states[0].copy_(self.recurrent_hidden_states[-1])
        self.masks[0].copy_(self.masks[-1])
        self.bad_masks[0].copy_(self.bad_masks[-1])
        self.location_masks[0].copy_(self.location_masks[-1])

    def compute_returns(self, next_value, use_gae, gamma, gae_lambda, use_proper_time_limits=True, advantages=False):
        """The reference's compute_returns, bit for bit, as one native call: bpp_compute_returns on the current stream of a
        device storage, bpp_compute_returns_host for a CPU storage.  advantages=True: also returns the [T,N,1] tensor
        returns[:-1] - value_preds[:-1]."""
        s, T, N, dev = self._slabs, self.num_steps, self.num_envs, self.device
        nv = next_value.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        if nv.numel() != N:
            raise ValueError("next_value must hold one value per bin")
        if any(self._from_done) and not all(self._from_done):      # a rollout filled both ways: finish the masks, then read them
            for t, d in enumerate(self._from_done):
                if d:
                    s["masks"][t + 1].copy_((s["done"][t + 1] == 0).to(torch.float32))     # any nonzero byte is done, as in the kernel
                    self._from_done[t] = False
        done = self.done.data_ptr() if all(self._from_done) else None
        adv = torch.empty((T, N), dtype=torch.float32, device=dev) if advantages else None
        # the variants without proper time limits never read bad_masks
        args = [self.rewards.data_ptr(), s["value_preds"].data_ptr(), nv.data_ptr(), done, s["masks"].data_ptr(),
                s["bad_masks"].data_ptr() if use_proper_time_limits else None, s["returns"].data_ptr(),
                adv.data_ptr() if adv is not None else None, T, N, int(bool(use_gae)), int(bool(use_proper_time_limits)),
                float(gamma), float(gae_lambda)]
        if dev.type == "cuda":
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().bpp_compute_returns(*args, stream_ptr(dev)))
        elif dev.type == "cpu":
            _lib.check(_lib.lib().bpp_compute_returns_host(*args))
        else:
            raise RuntimeError("RolloutStorage.compute_returns runs on a HIP device or on the CPU, not on %s" % dev)
        return adv.unsqueeze(-1) if adv is not None else None

    def a2c_loss(self, logits, values, pred_mask, **coefs):
        """The loss of the reference's update on this rollout and its gradients in one native call (update.a2c_loss): logits
        [T*N, M], values [T*N, 1] or [T, N, 1] and pred_mask [T*N, M] or None are the network's outputs on obs[:-1];
        location_masks[:-1], actions and returns[:-1] are handed over as views of the slabs, nothing is copied."""
        from .update import a2c_loss
        s, T, N = self._slabs, self.num_steps, self.num_envs
        return a2c_loss(logits, values, pred_mask, s["location_masks"][:-1].view(T * N, -1), s["actions"].view(T * N),
                        s["returns"][:-1].view(T * N), **coefs)


    # ------------------------------------------------------------------ PPO (acktr/algo/ppo.py; include/bpp_ppo.h)
    def normalized_advantages(self):
        """[T, N, 1]: (adv - adv.mean()) / (adv.std() + 1e-5) of adv = returns[:-1] - value_preds[:-1] (ppo.py:34-36).  A device
        storage: one native call (bpp_ppo_advantages), the same bits on every run.  A CPU storage: these torch expressions in the
        slabs' dtype."""
        s = self._slabs
        if self.device.type == "cuda":
            from .ppo import normalized_advantages
            return normalized_advantages(s["returns"][:-1], s["value_preds"][:-1])[0].unsqueeze(-1)
        adv = s["returns"][:-1] - s["value_preds"][:-1]
        return ((adv - adv.mean()) / (adv.std() + 1e-5)).unsqueeze(-1)

    def feed_forward_generator(self, advantages, num_mini_batch=None, mini_batch_size=None, generator=None):
        """The reference's generator (acktr/storage.py:113-149): mini-batches of rows of [:-1] in the order of
        BatchSampler(SubsetRandomSampler(range(T * N)), mini_batch_size, drop_last=True) -- torch.randperm(T * N) on the CPU cut
        into chunks, the remainder dropped, so the same torch seed gives the same mini-batches.  Each item is a ppo.MiniBatch."""
        from .ppo import MiniBatch
        num_steps, num_processes = self.num_steps, self.num_envs
        batch_size = num_processes * num_steps
        if mini_batch_size is None:
            assert batch_size >= num_mini_batch, (
                "PPO requires the number of processes ({}) * number of steps ({}) = {} to be greater than or equal to the number of "
                "PPO mini batches ({}).".format(num_processes, num_steps, num_processes * num_steps, num_mini_batch))
            mini_batch_size = batch_size // num_mini_batch
        perm = torch.randperm(batch_size, generator=generator).to(self.device)
        for i in range(batch_size // mini_batch_size):
            yield MiniBatch(self, perm[i * mini_batch_size:(i + 1) * mini_batch_size], advantages)

    def ppo_loss(self, logits, values, pred_mask, batch, advantages, **kw):
        """The loss of one PPO mini-batch and its gradients (ppo.ppo_loss): logits [B, M], values [B, 1] and pred_mask [B, M] or
        None are the network's outputs on batch.obs_batch; the slabs and batch.indices are handed over as they are, nothing of the
        rollout is gathered.  A CPU storage states the same in torch (ppo.ppo_loss_torch)."""
        from .ppo import ppo_loss, ppo_loss_torch
        s, T, N = self._slabs, self.num_steps, self.num_envs
        fn = ppo_loss if self.device.type == "cuda" else ppo_loss_torch
        return fn(logits, values, pred_mask, s["location_masks"][:-1].view(T * N, -1), s["actions"].view(T * N),
                  s["value_preds"][:-1].view(T * N), s["returns"][:-1].view(T * N), s["action_log_probs"].view(T * N),
                  advantages.reshape(T * N), indices=batch.indices if batch is not None else None, **kw)


class _Step(int):
    """`storage.step`: the reference's integer attribute -- and callable, `storage.step(env, actions, value, action_log_prob)`
    being the zero-copy lock-step (RolloutStorage.lockstep)."""

    def __new__(cls, storage):
        self = int.__new__(cls, storage.step_index)
        self._storage = storage
        return self

    def __call__(self, env, actions, value=None, action_log_prob=None):
        return self._storage.lockstep(env, actions, value, action_log_prob)
