"""TrainStep.step()'s host side without a GPU: the order of its effects, how the tensor-fed and the batcher-fed step bind
their fixed input buffers, the refusals of the two ways in, and the log it returns.  The constructor needs the GPU, so
the object is made with __new__ and given the attributes the step reads; the step body, the optimizer launch and
everything around them are stubs that record their calls.  use_graph=False throughout: a capture is GPU work."""
import types

import pytest
import torch

from hypernerf_torch_amd import machine
from hypernerf_torch_amd.training import TrainStep


class _Model:
    def __init__(self, calls):
        self._calls = calls

    @property
    def training(self):
        self._calls.append("model.training")
        return True


class _Batcher:
    """next_rows / views / launch of datasets.RayBatcher: `sizes` in turn, views of two fixed buffers."""

    def __init__(self, calls, sizes, batch_size):
        self.calls, self.sizes, self.k = calls, list(sizes), 0
        self.rays, self.rgbs = torch.zeros(batch_size, 9), torch.zeros(batch_size, 3)

    def next_rows(self):
        self.calls.append("next_rows")
        rows = self.sizes[self.k % len(self.sizes)]
        self.k += 1
        return rows

    def views(self, rows):
        self.calls.append(("views", rows))
        return self.rays[:rows], self.rgbs[:rows]

    def launch(self, rows):
        self.calls.append(("gather", rows))


def make_step(monkeypatch, batcher_sizes=None, clip=None, occupancy=True, background=False, lr=5e-4):
    calls = []
    ts = TrainStep.__new__(TrainStep)
    # what the constructor leaves behind, as far as step() reads it
    ts.model = _Model(calls)
    ts.use_graph, ts.dp, ts.sync, ts.world = False, False, None, 1
    ts.background_loss = object() if background else None
    ts.distortion_loss = None
    ts.clip = clip
    ts.occupancy = types.SimpleNamespace(before_step=lambda: calls.append("before_step")) if occupancy else None
    ts.optimizer = types.SimpleNamespace(sync_hyper=lambda: calls.append("sync_hyper"), param_groups=[{"lr": lr}])
    ts.arena = types.SimpleNamespace(bump=lambda: calls.append("bump"))
    ts.batcher = None if batcher_sizes is None else _Batcher(calls, batcher_sizes, max(batcher_sizes))
    # the step's own state (a name that one of the two ways in does not read is harmless)
    ts._graph = ts._graph_state = ts._batched_state = None
    ts._rays = ts._rgbs = ts._rng = ts._bg_rng = ts._batched_bg_rng = None
    ts._log, ts._batched, ts._batched_rng = {}, {}, {}
    seen = []

    def forward_backward():
        calls.append("forward_backward")
        seen.append((ts._rays, ts._rgbs, ts._rng, ts._bg_rng))
        ts._log = {"train/loss": ts._rays.sum(), "train/psnr": torch.tensor(20.0)}

    ts._forward_backward = forward_backward
    ts._optimizer_step = lambda: calls.append("optimizer_step")
    monkeypatch.setattr(machine, "note_parameters_changed", lambda: calls.append("note_parameters_changed"))
    return ts, calls, seen


def batch(rows, fill=1.0, cols=9):
    return torch.full((rows, cols), fill), torch.full((rows, 3), fill / 2)


TAIL = ["forward_backward", "optimizer_step", "bump", "note_parameters_changed"]


def test_tensor_fed_step_runs_its_effects_in_order(monkeypatch):
    ts, calls, _ = make_step(monkeypatch)
    ts.step(*batch(8))
    assert calls == ["model.training", "sync_hyper", "before_step"] + TAIL
    del calls[:]
    ts.step(*batch(8))                                   # and so does every later step
    assert calls == ["model.training", "sync_hyper", "before_step"] + TAIL
    ts, calls, _ = make_step(monkeypatch, occupancy=False)
    ts.step(*batch(8))
    assert calls == ["model.training", "sync_hyper"] + TAIL


def test_batcher_fed_step_gathers_ahead_of_the_body(monkeypatch):
    ts, calls, seen = make_step(monkeypatch, batcher_sizes=(8, 8, 5))
    for rows in (8, 8, 5):
        del calls[:]
        ts.step()
        assert calls == ["next_rows", ("views", rows), "model.training", "sync_hyper", "before_step", ("gather", rows)] + TAIL
        rays, rgbs = seen[-1][:2]
        assert rays.shape == (rows, 9) and rays.data_ptr() == ts.batcher.rays.data_ptr()         # the batcher's own buffers
        assert rgbs.shape == (rows, 3) and rgbs.data_ptr() == ts.batcher.rgbs.data_ptr()
        assert ts._rays is rays and ts._rng is None and ts._bg_rng is None


def test_tensor_buffers_are_owned_and_copied_into_in_place(monkeypatch):
    ts, _, seen = make_step(monkeypatch)
    rays, rgbs = batch(8, 1.0)
    ts.step(rays, rgbs, rng={"t_rand": torch.full((8, 4), 0.25)})
    b_rays, b_rgbs, b_rng = ts._rays, ts._rgbs, ts._rng
    assert b_rays is not rays and b_rgbs is not rgbs and torch.equal(b_rays, rays) and torch.equal(b_rgbs, rgbs)
    assert set(b_rng) == {"t_rand"} and ts._bg_rng is None
    t_rand = b_rng["t_rand"]
    rays.fill_(7.0)                                      # the caller's tensor is its own again
    assert float(b_rays[0, 0]) == 1.0
    rays2, rgbs2 = batch(8, 3.0)
    ts.step(rays2, rgbs2, rng={"t_rand": torch.full((8, 4), 0.75)})
    assert ts._rays is b_rays and ts._rgbs is b_rgbs and ts._rng is b_rng and ts._rng["t_rand"] is t_rand
    assert torch.equal(b_rays, rays2) and torch.equal(b_rgbs, rgbs2) and float(t_rand[0, 0]) == 0.75
    assert seen[0][0] is seen[1][0] and seen[0][2] is seen[1][2]          # what the body read both times


def test_tensor_buffers_are_cloned_anew_when_the_inputs_change_form(monkeypatch):
    ts, _, _ = make_step(monkeypatch, background=True)
    t = {"t_rand": torch.zeros(8, 4)}
    bg = {"bg_u": torch.full((6, 2), 0.5), "bg_n": torch.full((6, 3), -1.0)}
    ts.step(*batch(8))
    first = ts._rays
    ts.step(*batch(12))                                  # another row count
    assert ts._rays is not first and ts._rays.shape == (12, 9) and ts._rgbs.shape == (12, 3)
    second = ts._rays
    ts.step(*batch(12, cols=8))                          # the same rows, another width
    assert ts._rays is not second and ts._rays.shape == (12, 8)
    ts.step(*batch(8))
    plain = ts._rays
    ts.step(*batch(8), rng=t)                            # rng: not given -> given
    assert ts._rays is not plain and set(ts._rng) == {"t_rand"} and ts._bg_rng is None
    with_rng = ts._rays
    ts.step(*batch(8), rng=dict(t, **bg))                # background draws: not given -> given
    assert ts._rays is not with_rng and set(ts._rng) == {"t_rand"} and set(ts._bg_rng) == {"bg_u", "bg_n"}
    assert ts._bg_rng["bg_u"] is not bg["bg_u"] and torch.equal(ts._bg_rng["bg_n"], bg["bg_n"])
    with_bg, bg_u = ts._rays, ts._bg_rng["bg_u"]
    ts.step(*batch(8), rng=dict(t, bg_u=torch.full((6, 2), 0.125), bg_n=bg["bg_n"]))
    assert ts._rays is with_bg and ts._bg_rng["bg_u"] is bg_u and float(bg_u[0, 0]) == 0.125      # unchanged form: in place
    ts.step(*batch(8), rng=bg)                           # rng: given -> not given (the background draws stay)
    assert ts._rays is not with_bg and ts._rng is None and set(ts._bg_rng) == {"bg_u", "bg_n"}
    only_bg = ts._rays
    ts.step(*batch(8))                                   # background draws: given -> not given
    assert ts._rays is not only_bg and ts._rng is None and ts._bg_rng is None


def test_batcher_keeps_one_rng_buffer_set_per_row_count(monkeypatch):
    ts, _, seen = make_step(monkeypatch, batcher_sizes=(8, 5), background=True)

    def draws(rows, value, keys=("t_rand",)):
        return {k: torch.full((rows, 4), value) for k in keys}

    ts.step(rng=draws(8, 0.1))
    full = ts._rng
    ts.step(rng=draws(5, 0.2))
    short = ts._rng
    assert full is not short and full["t_rand"].shape == (8, 4) and short["t_rand"].shape == (5, 4)
    ts.step(rng=draws(8, 0.3))
    ts_full_again = ts._rng
    ts.step(rng=draws(5, 0.4))
    assert ts_full_again is full and ts._rng is short                     # one set per row count, copied into in place
    assert float(full["t_rand"][0, 0]) == pytest.approx(0.3) and float(short["t_rand"][0, 0]) == pytest.approx(0.4)
    ts.step(rng=draws(8, 0.5, keys=("t_rand", "u")))                      # another key set: that row count's set is replaced
    assert ts._rng is not full and set(ts._rng) == {"t_rand", "u"}
    ts.step(rng=draws(5, 0.6))
    assert ts._rng is short                                               # ... and only that one
    ts.step()                                                             # no draws: nothing bound
    assert ts._rng is None and ts._bg_rng is None
    ts.step(rng=draws(5, 0.7))
    assert ts._rng is short
    # the background draws: ONE pair of buffers for every row count
    bg = {"bg_u": torch.full((6, 2), 0.5), "bg_n": torch.full((6, 3), -1.0)}
    ts.step(rng=dict(draws(8, 0.8, keys=("t_rand", "u")), **bg))
    pair = ts._bg_rng
    assert set(pair) == {"bg_u", "bg_n"} and pair["bg_u"] is not bg["bg_u"] and set(ts._rng) == {"t_rand", "u"}
    ts.step(rng={"bg_u": torch.full((6, 2), 0.25), "bg_n": bg["bg_n"]})   # 5 rows, no per-ray draws
    assert ts._bg_rng is pair and float(pair["bg_u"][0, 0]) == 0.25 and ts._rng is None
    ts.step()
    assert ts._bg_rng is None
    ts.step(rng=bg)
    assert ts._bg_rng is pair and float(pair["bg_u"][0, 0]) == 0.5
    assert seen[-1][3] is pair                                            # what the body read


def test_the_two_ways_in_refuse_each_other(monkeypatch):
    ts, calls, _ = make_step(monkeypatch, batcher_sizes=(8,))
    rays, rgbs = batch(8)
    for args in ((rays, rgbs), (rays, None), (None, rgbs)):
        with pytest.raises(ValueError, match="takes no rays"):
            ts.step(*args)
    plain, plain_calls, _ = make_step(monkeypatch)
    for args in ((), (rays,), (None, rgbs)):
        with pytest.raises(ValueError, match="needs rays and rgbs"):
            plain.step(*args)
    assert calls == [] and plain_calls == []             # refused before anything ran


def test_returned_log_is_a_clone_with_lr(monkeypatch):
    ts, _, _ = make_step(monkeypatch, lr=2.5e-4)
    log = ts.step(*batch(8))
    assert set(log) == {"train/loss", "train/psnr", "lr"} and log["lr"] == 2.5e-4
    assert float(log["train/loss"]) == 72.0 and float(log["train/psnr"]) == 20.0
    assert log["train/loss"] is not ts._log["train/loss"] and "lr" not in ts._log
    log["train/loss"].fill_(-1.0)
    log["train/psnr"] = None
    assert float(ts._log["train/loss"]) == 72.0 and float(ts._log["train/psnr"]) == 20.0
    bt, _, _ = make_step(monkeypatch, batcher_sizes=(8,), lr=1e-3)
    log = bt.step()
    assert set(log) == {"train/loss", "train/psnr", "lr"} and log["lr"] == 1e-3
    log["train/loss"].fill_(-1.0)
    assert float(bt._log["train/loss"]) == 0.0


@pytest.mark.parametrize("batcher_sizes", [None, (8,)])
def test_grad_norm_is_logged_exactly_with_a_norm_clip(monkeypatch, batcher_sizes):
    norm = torch.tensor(3.5)
    for clip, logged in ((None, False), (types.SimpleNamespace(max_norm=None, total_norm=norm), False),
                         (types.SimpleNamespace(max_norm=1.0, total_norm=norm), True)):
        ts, _, _ = make_step(monkeypatch, batcher_sizes=batcher_sizes, clip=clip)
        log = ts.step(*(() if batcher_sizes else batch(8)))
        assert ("train/grad_norm" in log) == logged
        if logged:
            assert float(log["train/grad_norm"]) == 3.5 and log["train/grad_norm"] is not norm     # cloned with the rest
