"""The torch front-end glue of the native calls (online-3d-bpp-drl_amd/_front.py) on the CPU: the tensor checks
with their exact texts, the grown-to-largest workspace and the shared result class of the fused losses.  No device is touched: a
tensor that has to pass for one on a HIP device is a CPU tensor whose `device` says cuda:0."""
import pytest
import torch

import bpp_amd
from bpp_amd import _front as front
from bpp_amd import _lib

HIP0 = torch.device("cuda", 0)


class OnHip(torch.Tensor):
    """A CPU tensor that reports cuda:0 as its device: shapes and strides are real, nothing is launched."""
    device = property(lambda self: HIP0)


def on_hip(t):
    return t.as_subclass(OnHip)


def refusal(exc, fn, *args):
    with pytest.raises(exc) as e:
        fn(*args)
    return str(e.value)


def test_dense_f32_views_dense_inputs_copies_strided_ones_and_refuses_with_its_texts():
    cpu = torch.device("cpu")
    for src, shape in ((torch.randn(5, 1, requires_grad=True), (5,)), (torch.randn(2, 3, 1, requires_grad=True), (6,))):
        got = front.dense_f32(src, shape, "values", cpu)
        assert tuple(got.shape) == shape and not got.requires_grad and got.data_ptr() == src.data_ptr()
        assert torch.equal(got, src.detach().reshape(shape))
    base = torch.randn(6, 2)
    got = front.dense_f32(base[:, 0], (6,), "returns", cpu)
    assert got.is_contiguous() and got.data_ptr() != base.data_ptr() and torch.equal(got, base[:, 0])
    assert refusal(ValueError, front.dense_f32, torch.zeros(6, dtype=torch.float64), (6,), "returns", cpu) == "returns must be a float32 tensor"
    assert refusal(ValueError, front.dense_f32, [0.0] * 6, (6,), "returns", cpu) == "returns must be a float32 tensor"
    assert refusal(ValueError, front.dense_f32, torch.zeros(6), (2, 4), "pred_mask", cpu) == "pred_mask has 6 elements, expected 2x4"
    assert refusal(ValueError, front.dense_f32, torch.zeros(6), (6,), "values", HIP0) == "values is on cpu, the logits on cuda:0"


def test_dense_i64_views_dense_inputs_copies_strided_ones_and_refuses_with_its_text():
    cpu = torch.device("cpu")
    src = torch.arange(6).reshape(2, 3, 1)
    got = front.dense_i64(src, 6, "action", cpu)
    assert tuple(got.shape) == (6,) and got.data_ptr() == src.data_ptr() and torch.equal(got, torch.arange(6))
    base = torch.arange(12).reshape(6, 2)
    got = front.dense_i64(base[:, 1], 6, "indices", cpu)
    assert got.is_contiguous() and got.data_ptr() != base[:, 1].data_ptr() and torch.equal(got, base[:, 1])
    text = "action must be an int64 tensor of 6 entries on the logits' device"
    for bad, dev in ((torch.zeros(6, dtype=torch.int32), cpu), (torch.zeros(5, dtype=torch.int64), cpu), (torch.zeros(6, dtype=torch.int64), HIP0),
                     ([0] * 6, cpu)):
        assert refusal(ValueError, front.dense_i64, bad, 6, "action", dev) == text


def test_obs_rows_returns_the_row_stride_and_refuses_in_the_order_of_its_checks():
    A = 4
    assert front.obs_rows(on_hip(torch.zeros(1, 20)), A, "who") == (1, 20)
    one_of_wider = on_hip(torch.zeros(3, 64)[1:2, 8:48])              # n = 1: the stride between rows is never used, the length is
    assert one_of_wider.stride(0) == 64 and front.obs_rows(one_of_wider, A, "who") == (1, 40)
    view = on_hip(torch.zeros(3, 64)[:, 8:48])
    assert tuple(view.shape) == (3, 40) and not view.is_contiguous()
    assert front.obs_rows(view, A, "who") == (3, 64)
    whole = "obs must be a float32 [n, 4 A] tensor with n >= 1"
    for bad in (torch.zeros(2, 16, dtype=torch.float64), torch.zeros(16), torch.zeros(0, 16), [[0.0] * 16]):
        assert refusal(ValueError, front.obs_rows, bad, A, "who") == whole                 # before the device is looked at
    rows = "obs rows must be contiguous and hold 4 A = 16 floats"
    for bad in (torch.zeros(2, 15), torch.zeros(2, 32)[:, ::2], torch.zeros(40).as_strided((2, 16), (15, 1))):
        assert refusal(ValueError, front.obs_rows, on_hip(bad), A, "who") == rows
        assert "HIP device" in refusal(RuntimeError, front.obs_rows, bad, A, "who")         # on the CPU the device comes first
    assert refusal(RuntimeError, front.obs_rows, torch.zeros(2, 16), A, "the_caller") == "the_caller needs its tensors on a HIP device"


def test_workspace_grows_to_the_largest_request_per_key():
    cpu = torch.device("cpu")
    ws = front.Workspace()
    first = ws.take("a", 8, torch.float32, cpu)
    assert first.numel() == 8 and first.dtype == torch.float32 and ws["a"] is first
    assert ws.take("a", 4, torch.float32, cpu) is first
    grown = ws.take("a", 16, torch.float32, cpu)
    assert grown is not first and grown.numel() == 16 and ws["a"] is grown and ws["a"].numel() == 16
    other = ws.take("b", 2, torch.float64, cpu)
    assert other is not grown and other.dtype == torch.float64 and ws["a"] is grown and set(ws) == {"a", "b"}
    assert isinstance(bpp_amd.policy._WORKSPACE, front.Workspace) and isinstance(bpp_amd.kfac._WORKSPACE, front.Workspace)


@pytest.mark.parametrize("cls,names", [(bpp_amd.A2CLoss, _lib.A2C_TERMS), (bpp_amd.PPOLoss, _lib.PPO_TERMS)], ids=["a2c", "ppo"])
def test_native_loss_names_its_terms_and_hands_the_given_gradients_to_autograd(cls, names):
    assert issubclass(cls, front.NativeLoss) and cls.TERMS == names
    terms = torch.arange(len(names), dtype=torch.float32) + 0.5
    a, b = torch.randn(3, 2, requires_grad=True), torch.randn(3, 1, requires_grad=True)
    ga, gb = torch.randn(6), torch.randn(3)
    loss = cls(terms, None, (a * 1, b * 1), [ga, gb], dict(logits=a))
    for i, name in enumerate(names):
        got = getattr(loss, name)
        assert got.dim() == 0 and got.data_ptr() == terms[i].data_ptr() and got.item() == terms[i].item()
    assert loss.terms is terms and loss.rows is None and loss.inputs == dict(logits=a)
    assert loss.grad_logits is ga and loss.grad_values is gb and loss.grad_pred_mask is None
    assert cls(terms, None, (a, b, a), [ga, gb, ga]).grad_pred_mask is ga
    loss.backward()
    assert torch.equal(a.grad, ga.view(3, 2)) and torch.equal(b.grad, gb.view(3, 1))
    frozen = cls(terms, None, (a.detach(), b.detach()), [ga, gb])
    assert refusal(RuntimeError, frozen.backward) == "none of logits, values and pred_mask requires grad"
