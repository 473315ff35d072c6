"""The shared-gradient rule of the training Functions (train_ops.SharedGrad: several autograd nodes write one gradient buffer, the last
backward to run hands it out) and the key of StackParamsFn's segment-table cache, with no library behind them: plain objects and
CPU tensors."""
import pytest
import torch

from instancediff_amd.train_ops import SharedGrad, stack_params_key


def test_the_last_of_three_leaves_hands_the_buffer_out():
    like = torch.zeros(3, 4)
    sg = SharedGrad()
    for _ in range(3):
        sg.enter()
    handed, bufs = [], []
    for i in range(3):
        buf, held = sg.leave(like)
        assert held == (i > 0)                     # the first backward writes, the later ones accumulate
        assert buf.shape == like.shape and buf.dtype == like.dtype
        bufs.append(buf)
        handed.append(sg.result())
    assert bufs[0] is bufs[1] is bufs[2]           # one buffer for the group
    assert handed[0] is None and handed[1] is None and handed[2] is bufs[0]
    assert sg.pending == 0 and sg.buf is None      # nothing kept alive behind the backward


def test_a_leave_without_an_enter_raises_and_the_object_stays_usable():
    like = torch.zeros(2, 2)
    sg = SharedGrad()
    for _ in range(3):
        sg.enter()
    for _ in range(3):
        sg.leave(like)
        sg.result()
    with pytest.raises(RuntimeError, match="retain_graph / double backward"):
        sg.leave(like)
    assert sg.pending == 0 and sg.buf is None
    sg.enter()                                     # a fresh forward / backward pair works again
    buf, held = sg.leave(like)
    assert not held and sg.result() is buf


def test_an_enter_while_a_buffer_is_held_raises():
    like = torch.zeros(2, 2)
    sg = SharedGrad()
    sg.enter()
    sg.leave(like)                                 # a backward that stopped between taking the buffer and handing it out
    with pytest.raises(RuntimeError, match="still held"):
        sg.enter()


def test_stack_params_key_tells_sizes_and_splits_apart():
    base = torch.zeros(32)
    other = torch.zeros(32)
    half = base[:16]
    assert half.data_ptr() == base.data_ptr()
    assert stack_params_key(2, 1, (base, other)) == stack_params_key(2, 1, (base, other))
    # equal addresses, another numel: what the caching allocator hands out after a reload
    assert stack_params_key(2, 1, (base, other)) != stack_params_key(2, 1, (half, other[:16]))
    assert stack_params_key(2, 1, (base, other)) != stack_params_key(2, 1, (half, other))
    # the same tensors under another L / nk split
    four = tuple(torch.zeros(8) for _ in range(4))
    assert stack_params_key(2, 2, four) != stack_params_key(4, 1, four)
    assert stack_params_key(2, 2, four) != stack_params_key(1, 4, four)
