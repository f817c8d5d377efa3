"""gdd.sharded's host structure without a process group or a device: the chunk schedule and the state
read one chunk behind (run_chunks), the per-mode iteration bodies' order of calls, the typed Lloyd
state (gdd._lib.LloydState against the library and the tests' stand-ins), and the small shared
helpers. Fake ops record every call and replay a scripted state."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gdd import _lib, sharded  # noqa: E402


class ScheduleOps:
    """The two state calls of the chunk driver: `states[c]` is what the copy begun after chunk c holds
    (default: no stop). The log is shared with the mode that records the iterations."""

    def __init__(self, log, states=None):
        self.log, self.states, self.begun = log, states or {}, 0

    def lloyd_state_begin(self, ctx):
        c = self.begun
        self.begun += 1
        self.log.append(("begin", c))
        return c

    def lloyd_state_end(self, handle):
        self.log.append(("end", handle))
        return self.states.get(handle, (0, 0, 0, 0))


class ScheduleMode:
    def __init__(self, states=None):
        self.log = []
        self.ops, self.ctx = ScheduleOps(self.log, states), object()

    def iteration(self, C_old, C_new, i, first):
        self.log.append(("it", i, C_old, C_new, bool(first)))

    def update(self, C_old, C_new, i, resumed):  # the driver calls it only to resume after a relocation
        assert resumed is True
        self.log.append(("resume", i, C_old, C_new))


CB = ("C0", "C1")


def _run(mode, it0=0, resume=False, first_e=0, max_iter=15):
    return sharded.run_chunks(mode, CB, it0, resume, first_e, max_iter)


def _chunks(log):
    """Iterations enqueued before each state copy."""
    sizes, cur = [], 0
    for ev in log:
        if ev[0] in ("it", "resume"):
            cur += 1
        elif ev[0] == "begin":
            sizes.append(cur)
            cur = 0
    assert cur == 0  # every chunk ends with its state copy
    return sizes


@pytest.mark.parametrize("max_iter,want", [(1, [1]), (2, [2]), (3, [2, 1]), (6, [2, 4]), (7, [2, 4, 1]),
                                           (15, [2, 4, 8, 1]), (30, [2, 4, 8, 8, 8])])
def test_chunk_sizes_double_to_eight_and_stop_at_max_iter(max_iter, want):
    mode = ScheduleMode()
    assert _run(mode, max_iter=max_iter) == (0, 0, 0, max_iter)  # no stop: sklearn's loop end
    assert _chunks(mode.log) == want
    assert [ev[1] for ev in mode.log if ev[0] == "it"] == list(range(max_iter))


def test_chunk_sizes_restart_from_two_at_it0():
    mode = ScheduleMode()
    assert _run(mode, it0=5, first_e=5, max_iter=12) == (0, 0, 0, 12)
    assert _chunks(mode.log) == [2, 4, 1]
    assert [ev[1] for ev in mode.log if ev[0] == "it"] == list(range(5, 12))


def test_state_is_read_one_chunk_behind():
    mode = ScheduleMode()
    _run(mode, max_iter=15)
    kinds = [ev[:2] if ev[0] != "it" else ("it", ev[1]) for ev in mode.log]
    assert kinds == ([("it", 0), ("it", 1), ("begin", 0)]
                     + [("it", i) for i in range(2, 6)] + [("begin", 1), ("end", 0)]
                     + [("it", i) for i in range(6, 14)] + [("begin", 2), ("end", 1)]
                     + [("it", 14), ("begin", 3), ("end", 2), ("end", 3)])
    # iteration i reads C[i % 2] and writes C[(i + 1) % 2]; only iteration first_e is a first E-step
    for ev in mode.log:
        if ev[0] == "it":
            assert ev[2:] == (CB[ev[1] % 2], CB[(ev[1] + 1) % 2], ev[1] == 0)


@pytest.mark.parametrize("chunk", [0, 1, 2, 3])
def test_a_stop_in_chunk_c_returns_its_words_after_chunk_c_plus_one(chunk):
    st = (2 * 4 + 2, 2, 4, 5)  # (stop_at, reason, iter, done): distinct words
    mode = ScheduleMode({chunk: st})
    assert _run(mode, max_iter=15) == st
    # chunk c's copy is waited for once chunk c+1 (if any) is enqueued and its copy begun; nothing after
    sizes = [2, 4, 8, 1]
    assert _chunks(mode.log) == sizes[:chunk + 2]
    assert mode.log[-1] == ("end", chunk)
    assert [ev for ev in mode.log if ev[0] == "end"] == [("end", c) for c in range(chunk + 1)]


def test_it0_at_max_iter_reads_no_state():
    mode = ScheduleMode({0: (1, 1, 1, 1)})
    assert _run(mode, it0=7, resume=True, first_e=8, max_iter=7) == (0, 0, 0, 7)
    assert mode.log == []


def test_resume_body_runs_once_at_it0():
    mode = ScheduleMode()
    assert _run(mode, it0=3, resume=True, first_e=4, max_iter=10) == (0, 0, 0, 10)
    assert [ev[:2] for ev in mode.log if ev[0] in ("it", "resume")] == \
        [("resume", 3)] + [("it", i) for i in range(4, 10)]
    assert mode.log[0] == ("resume", 3, "C1", "C0")
    assert [ev[1] for ev in mode.log if ev[0] == "it" and ev[4]] == [4]  # the fresh E-step after it
    assert _chunks(mode.log) == [2, 4, 1]
    fresh = ScheduleMode()
    _run(fresh, it0=3, resume=False, first_e=3, max_iter=10)
    assert not [ev for ev in fresh.log if ev[0] == "resume"]


# ---------------------------------------------------------------------------------------------------
# the modes' bodies: today's order of calls per iteration
# ---------------------------------------------------------------------------------------------------
class RecordingOps:
    """Every primitive a mode calls, recorded as (name, args); lloyd_begin hands out real buffers."""

    def __init__(self):
        self.calls = []

    def lloyd_begin(self, n, dim, k, world, m, fw):
        self.calls.append(("lloyd_begin", (n, dim, k, world, m, fw)))
        return SimpleNamespace(n=n, dim=dim, k=k, labels=torch.zeros(world * m, dtype=torch.int32),
                               parts=torch.zeros(world * k * fw), wsum=torch.zeros(k))

    def lloyd_reduce_begin(self, ctx):
        self.calls.append(("lloyd_reduce_begin", ()))
        ctx.rbuf = torch.zeros(ctx.k * (ctx.dim + 1) + 1, dtype=torch.int64)

    def __getattr__(self, name):
        if not name.startswith("lloyd_"):
            raise AttributeError(name)
        return lambda ctx, *args: self.calls.append((name, args))


@pytest.fixture
def collectives(monkeypatch):
    """gdd.sharded's collectives replaced by recorders appending to the ops' call list."""
    def install(ops):
        monkeypatch.setattr(sharded, "all_gather_slots",
                            lambda buf, m, group=None: ops.calls.append(("all_gather_slots", (buf, m, group))))
        monkeypatch.setattr(sharded, "all_reduce_sum",
                            lambda buf, group=None: ops.calls.append(("all_reduce_sum", (buf, group))))
    return install


def _mode(cls, collectives, rank=1, world=2, n=9, dim=5, k=3):
    ops = RecordingOps()
    collectives(ops)
    X = torch.zeros(n, dim)
    mode = cls(ops, X, k, rank, world, "grp", 0.25)
    setup, ops.calls[:] = list(ops.calls), []
    return mode, ops, X, setup


def test_rows_body_order(collectives):
    mode, ops, X, setup = _mode(sharded._Rows, collectives)
    assert setup == [("lloyd_begin", (9, 5, 3, 2, 5, 1))] and mode.name == "rows"
    mode.iteration("Cold", "Cnew", 6, True)
    assert [c[0] for c in ops.calls] == ["lloyd_estep", "all_gather_slots", "lloyd_mstep", "lloyd_update"]
    estep, gather, mstep, update = (c[1] for c in ops.calls)
    assert estep == (X, "Cold", 5, 9, True, 6)  # rank 1 of 2: rows [5, 9), m = 5
    assert gather[0] is mode.ctx.labels and gather[1:] == (5, "grp")
    assert mstep == (X, 0, 5, "Cnew", 6)  # all columns, straight into the next centres
    assert update == (None, 5, "Cnew", "Cold", 0.25, 6)
    ops.calls[:] = []
    mode.update("Cold", "Cnew", 6, True)
    assert ops.calls == [("lloyd_update", (None, 5, "Cnew", "Cold", 0.25, 6))]
    ops.calls[:] = []
    mode.gather_labels()
    mode.gather_sums("Cnew")
    assert ops.calls == []  # the labels are already whole, the sums already in C_new
    assert mode.labels.shape == (9,) and mode.labels.data_ptr() == mode.ctx.labels.data_ptr()


def test_column_split_body_order(collectives):
    mode, ops, X, setup = _mode(sharded._RowsCols, collectives)
    assert setup == [("lloyd_begin", (9, 5, 3, 2, 5, 3))] and mode.name == "rows"  # fw = ceil(5 / 2)
    mode.iteration("Cold", "Cnew", 2, False)
    assert [c[0] for c in ops.calls] == ["lloyd_estep", "all_gather_slots", "lloyd_mstep",
                                         "all_gather_slots", "lloyd_update"]
    estep, gather, mstep, gather2, update = (c[1] for c in ops.calls)
    assert estep == (X, "Cold", 5, 9, False, 2)
    assert gather[0] is mode.ctx.labels and gather[1:] == (5, "grp")
    assert mstep[:3] == (X, 3, 5) and mstep[4] == 2  # rank 1's columns [3, 5)
    assert mstep[3].shape == (3, 3) and mstep[3].data_ptr() == mode.ctx.parts[9:].data_ptr()  # its own slot
    assert gather2[0] is mode.ctx.parts and gather2[1:] == (9, "grp")  # k * fw elements per slot
    assert update[0] is mode.ctx.parts and update[1:] == (3, "Cnew", "Cold", 0.25, 2)
    ops.calls[:] = []
    mode.update("Cold", "Cnew", 2, True)
    assert ops.calls == [("lloyd_update", (None, 3, "Cnew", "Cold", 0.25, 2))]
    # before a relocation the sums are assembled from the slices
    mode.ctx.parts.copy_(torch.arange(18.0))
    C_new = torch.zeros(3, 5)
    mode.gather_labels()
    assert ops.calls[1:] == []  # the labels are whole after every iteration
    mode.gather_sums(C_new)
    want = np.concatenate([np.arange(9.0).reshape(3, 3), np.arange(9.0, 15.0).reshape(3, 2)], 1)
    assert np.array_equal(C_new.numpy(), want)


def test_reduce_body_order(collectives):
    mode, ops, X, setup = _mode(sharded._Reduce, collectives)
    assert [c[0] for c in setup] == ["lloyd_begin", "lloyd_reduce_begin", "lloyd_reduce_exponents"]
    assert setup[0][1] == (9, 5, 3, 2, 5, 1) and setup[2][1] == (X,) and mode.name == "reduce"
    mode.iteration("Cold", "Cnew", 4, False)
    assert [c[0] for c in ops.calls] == ["lloyd_estep", "lloyd_reduce_local", "all_reduce_sum",
                                         "lloyd_reduce_update"]
    estep, local, reduce, update = (c[1] for c in ops.calls)
    assert estep == (X, "Cold", 5, 9, False, 4)
    assert local == (X, 5, 9, 4)
    assert reduce[0] is mode.ctx.rbuf and reduce[1] == "grp"
    assert update == (False, "Cnew", "Cold", 0.25, 4)
    ops.calls[:] = []
    mode.update("Cold", "Cnew", 4, True)
    assert ops.calls == [("lloyd_reduce_update", (True, "Cnew", "Cold", 0.25, 4))]
    # each rank holds its own rows' labels: one all-gather before a relocation or a strict stop's labels
    ops.calls[:] = []
    mode.gather_labels()
    mode.gather_sums("Cnew")
    assert [c[0] for c in ops.calls] == ["all_gather_slots"]
    assert ops.calls[0][1][0] is mode.ctx.labels and ops.calls[0][1][1:] == (5, "grp")


# ---------------------------------------------------------------------------------------------------
# the typed state
# ---------------------------------------------------------------------------------------------------
WORDS = ("stop_at", "reason", "iter", "changed", "done")


def test_lloyd_state_layout():
    S = _lib.LloydState
    assert ctypes.sizeof(S) == 64
    assert [getattr(S, w).offset for w in WORDS] == [0, 4, 8, 12, 16]
    assert all(getattr(S, w).size == 4 for w in WORDS)
    assert [f[0] for f in S._fields_] == list(WORDS) + ["pad"] and S.pad.offset == 20
    st = S.from_buffer_copy(np.arange(1, 17, dtype=np.int32).tobytes())
    assert st.driver_words() == (1, 2, 3, 5)  # done, not the changed word


@pytest.mark.parametrize("standin", ["OracleOps", "ReduceOps"])
def test_standins_keep_the_struct(standin):
    import reduce_util
    ops = getattr(reduce_util, standin)()
    ctx = ops.lloyd_begin(8, 2, 2, 1, 8, 1)
    assert isinstance(ctx.state, _lib.LloydState)
    for i, w in enumerate(WORDS):
        setattr(ctx.state, w, 10 + i)
    assert ops.lloyd_state_end(ops.lloyd_state_begin(ctx)) == (10, 11, 12, 14)
    ops.lloyd_clear(ctx, True)
    assert [getattr(ctx.state, w) for w in WORDS] == [0, 0, 0, 13, 14]
    ctx.labels_old.fill_(5)
    ops.lloyd_clear(ctx, False)
    assert [getattr(ctx.state, w) for w in WORDS] == [0, 0, 0, 0, 14]
    assert bool((ctx.labels_old == -1).all())


# ---------------------------------------------------------------------------------------------------
# small shared helpers
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn,switch", [("propagation_shards_pay", "GDD_SHARD_PROP"),
                                       ("lloyd_rows_pay", "GDD_SHARD_LLOYD")])
def test_switches_force_both_size_models_alike(monkeypatch, fn, switch):
    small = dict(propagation_shards_pay=(100, 300, 8), lloyd_rows_pay=(100, 8, 4))[fn]
    pay = getattr(sharded, fn)
    monkeypatch.delenv(switch, raising=False)
    assert not pay(*small, 8) and not pay(*small, 1)
    monkeypatch.setenv(switch, "1")
    assert pay(*small, 8) and not pay(*small, 1)  # one rank never splits
    monkeypatch.setenv(switch, "0")
    assert not pay(*small, 8)
    assert sharded._forced(switch, 8) is False
    monkeypatch.delenv(switch)
    assert sharded._forced(switch, 8) is None and sharded._forced(switch, 1) is False


def test_best_of_inits_rule_and_auto():
    from gdd.kmeans import better_init, n_init_of
    assert n_init_of("auto") == 1 and n_init_of(10) == 10 and n_init_of("3") == 3
    a = np.array([0, 0, 1, 2])
    best = (a, 5.0)
    assert better_init(9.0, a, None, 3)  # the first init
    assert not better_init(5.0, np.array([1, 1, 0, 2]), best, 3)  # not lower
    assert not better_init(4.0, np.array([2, 2, 0, 1]), best, 3)  # lower, but the same clustering renamed
    assert better_init(4.0, np.array([0, 1, 1, 2]), best, 3)


def test_reduce_with_column_split_is_refused_at_construction():
    with pytest.raises(ValueError, match="split_columns"):
        sharded.ShardedKMeans(n_clusters=4, split_columns=True, mstep="reduce")
