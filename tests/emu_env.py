"""TEST INFRASTRUCTURE ONLY -- EmuVecEnv: the product's branch surface (bpp_amd.branch.BranchOps: step_bins, observe_bins,
clone_bins, preview, the id checks and the per-n output sets, all inherited) over the emulated library, so that the CPU
tests run bpp_amd.ReorderSearch, MCTSearch and MultiBinPacker themselves.  The bins are an emu.OracleEnv's; everything
the product code touches is a torch CPU tensor that shares memory with its numpy arrays, and the emulated library takes
host pointers behind the same C ABI."""
import ctypes

import numpy as np
import torch

from bpp_amd import _lib
from bpp_amd.branch import BranchOps
from bpp_amd.vec_env import StepTensors

KEYS = ("obs", "mask", "reward", "done", "counter", "ratio", "ep_ret", "ep_len")


def bind(emu):
    """The emulated library with the branch and search entry points bound, once: bpp_batch and bpp_stream are the front-end's
    classes (the OracleEnv's structs are passed), bpp_step_out the product's (BranchOps._branch_out builds it)."""
    L = emu.lib()
    if not getattr(L, "_bpp_search_bound", False):
        _lib.bind_branch(L, emu.Batch, None, emu.Stream)
        _lib.bind_reorder(L, emu.Batch)
        _lib.bind_multibin(L, emu.Batch)
        _lib.bind_mcts(L, emu.Batch)
        L._bpp_search_bound = True
    return L


def torch_policy(policy):
    """A numpy policy, obs [n, 4A] -> (value, logits[, pred]) arrays or None, as the tensor policy the search classes take."""
    def wrapped(obs):
        out = tuple(None if t is None else torch.from_numpy(np.ascontiguousarray(t)) for t in policy(obs.numpy()))
        return out + (None,) * (3 - len(out))
    return wrapped


class EmuVecEnv(BranchOps):
    """What BranchOps and the search classes require (see BranchOps) over emu.OracleEnv(pool or stream), reset on construction;
    plus look-alikes of BppVecEnv.step_tensors / sample_feasible / location_masks for full-batch warm-up steps."""
    device = torch.device("cpu")
    compute_mask = True

    def __init__(self, emu, size, num_envs, pool=None, stream=None, rotation=False):
        self.emu, self.lib = emu, bind(emu)
        self.oracle = o = emu.OracleEnv(pool, size, rotation, num_envs, stream=stream)
        self.num_envs = self.E = o.E
        self.W, self.L, self.H, self.A, self.M, self.obs_len, self.can_rotate = o.W, o.L, o.H, o.A, o.M, 4 * o.A, bool(o.rotation)
        self.state = torch.from_numpy(o.state.view(np.int32).reshape(o.E, 12))
        self.pool, self.hmap, self.ep_acc = torch.from_numpy(o.pool), torch.from_numpy(o.hmap), torch.from_numpy(o.ep_acc)
        self._batch_ref, self._stream = ctypes.byref(o._b), o.stream
        self._serial = 0
        self.reset()

    _first_reset = property(lambda self: self.oracle._first)

    def _stepped(self):
        self.oracle._after_steps(1)

    def _stream_ptr(self):
        return None

    def _on_device(self):
        pass

    def reset(self):
        self._serial += 1
        return torch.from_numpy(self.oracle.reset()[0])

    @property
    def location_masks(self):
        return torch.from_numpy(self.oracle.out["mask"])

    def sample_feasible(self, seed, step):
        return torch.from_numpy(self.emu.sample_feasible(self.oracle.out["mask"], seed, step))

    def step_tensors(self, actions):
        """One full-batch lock-step (OracleEnv.step); the result's tensors are views of the OracleEnv's output arrays."""
        out = self.oracle.step(torch.as_tensor(actions).numpy(), copy=False)
        self._serial += 1
        return StepTensors(**{k: torch.from_numpy(out[k].reshape(-1, 1) if k == "reward" else out[k]) for k in KEYS})

    def heightmaps(self):
        return self.hmap.view(self.E, self.W, self.L).to(torch.int32)
