"""DeviceOps' view of the Lloyd state on the device: lloyd_clear and the pinned state copy address
the struct's words by name (gdd._lib.LloydState), not by byte offset."""
import numpy as np
import pytest
import torch

from gdd import _lib
from gdd.sharded import DeviceOps

pytestmark = pytest.mark.gpu
WORDS = ("stop_at", "reason", "iter", "changed", "done")


def _words(ctx):
    st = _lib.LloydState.from_buffer_copy(ctx.state.cpu().numpy().tobytes())
    return [getattr(st, w) for w in WORDS], list(st.pad)


def test_clear_and_state_copy_use_the_named_words():
    ops = DeviceOps("cuda:0")
    ctx = ops.lloyd_begin(64, 3, 4, 1, 64, 1)
    assert ctx.state.numel() == 64
    fill = np.arange(101, 117, dtype=np.int32)  # sixteen distinct non-zero words
    ctx.state.copy_(torch.from_numpy(fill.view(np.uint8)))
    ctx.labels_old.fill_(9)
    assert ops.lloyd_state_end(ops.lloyd_state_begin(ctx)) == (101, 102, 103, 105)  # done, not changed
    ops.lloyd_clear(ctx, True)  # a resume after a relocation keeps the labels-changed flag
    assert _words(ctx) == ([0, 0, 0, 104, 105], list(range(106, 117)))
    assert bool((ctx.labels_old == 9).all())
    assert ops.lloyd_state_end(ops.lloyd_state_begin(ctx)) == (0, 0, 0, 105)
    ops.lloyd_clear(ctx, False)
    assert _words(ctx) == ([0, 0, 0, 0, 105], list(range(106, 117)))
    assert ctx.labels_old.shape == (64,) and bool((ctx.labels_old == -1).all())
