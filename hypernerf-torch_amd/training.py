"""The training step of the reference's Lightning system as one replayable GPU program
(reference: train.py:96-114 `forward` with its chunk loop, 146-163 `training_step`, 116-131 `configure_optimizers`;
optimizer / scheduler from utils.get_optimizer / get_scheduler, utils/__init__.py:23-59).

`TrainStep(model, lr=...)` owns what NeRFSystem owns around the model — loss, optimizer, LR schedule — laid out the
MI355X way: parameters and gradients in a `ParamArena`, `ArenaAdam` (one kernel for all parameters, hyper-parameters
and step counter on the device), the whole step (prepare_ray_dict -> model per chunk -> MSE -> backward -> Adam)
captured once into a HIP graph and replayed on fixed input buffers.  With torch.distributed initialised the initial
parameters are broadcast from rank 0 (what Lightning's DDP wrapper does), rays are expected pre-sharded per rank,
the gradient buffer is SUM-all-reduced in place between the captured forward+backward and the optimizer step —
optionally in two buckets, the first in flight while the weight gradients of the second are still being computed
(dist.GradSync, `overlap_grad_sync=True`) — and the 1/world of the mean is folded into the Adam kernel.
`step(rays, rgbs)` returns the log the reference's training_step records: {'train/loss', 'train/psnr', 'lr'}
(device scalars, no host sync).  `background_loss=losses.BackgroundLoss(...)` adds HyperNeRF's background regularization
to every step (and 'train/background_loss' to the log); without it the step is launch for launch the one above.
`distortion_loss=losses.DistortionLoss(...)` adds Mip-NeRF 360's distortion loss on the rendered levels' compositing
weights (and 'train/distortion_loss'): one launch per level behind the compositing launches, back-propagated together
with the MSE in ONE traversal (functional.backward_all); without it the step is launch for launch the one above.
`clip_grad_norm=` / `clip_grad_value=` clip the gradient buffer in two HIP launches right before every optimizer launch
(optim.GradClip: by value, then by global norm; Lightning's gradient_clip_val / gradient_clip_algorithm) and
`clip_grad_norm` adds 'train/grad_norm' (the norm before clipping) to the log; without them nothing is allocated or launched.
`occupancy=TrainOccupancy(...)` clips the step's rays to per-frame occupancy grids inside the captured step (one
hn_occ_clip_batch launch at its head; 'train/occupancy_hit' and 'train/occupancy_span' in the log) and keeps the grids
current between replays; without it the step is launch for launch the one above.  One GPU only.
"""
from __future__ import annotations

import contextlib
from typing import Dict, NamedTuple, Optional, Sequence, Union

import torch
import torch.distributed as dist

from . import functional as F
from . import machine
from . import optim as _optim          # FUSE_REDUCE is read where a TrainStep is built: tests rebind it on the module
from .arena import ParamArena
from .dist import GradSync, collective_capturable
from .graphs import GraphedStep
from .hypernerf import model_utils
from .losses import MSELoss, psnr
from .ops.occupancy.train import TrainOccupancy
from .optim import OPTIMIZERS, ArenaAdam, GradClip, MultiStepLR, check_clip_args, get_scheduler, make_optimizer

_EXTRA = {'nerf_alpha': None, 'warp_alpha': None, 'hyper_alpha': None, 'hyper_sheet_alpha': None}


class _Program(NamedTuple):
    """A captured step.  `run`: the whole step as ONE GraphedStep, or the data-parallel step in three pieces as
    (fwd_bwd, held) — a graph up to the first weight-gradient bucket and the graph of the held bucket (or None), with an
    eager all-reduce and the optimizer behind them (TrainStep._run).  `log`: the log tensors that capture wrote, which
    every replay overwrites."""
    run: Union[GraphedStep, tuple]
    log: Dict[str, torch.Tensor]


class TrainStep:
    def __init__(self, model: torch.nn.Module, lr: float = 5e-4, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, use_graph: bool = True, group=None, chunk: int = 32 * 1024,
                 decay_step: Optional[Sequence[int]] = None, decay_gamma: float = 0.1, overlap_grad_sync: bool = False,
                 hparams=None, force_dp: bool = False, capture_collective: bool = True, optimizer: str = "adam",
                 momentum: float = 0.9, batcher=None, background_loss=None, clip_grad_norm: Optional[float] = None,
                 clip_grad_value: Optional[float] = None, distortion_loss=None, occupancy=None):
        # the optimizer of the reference's get_optimizer (utils/__init__.py:23-41): hparams.optimizer (and
        # hparams.momentum for 'sgd') when hparams carries one, the keywords otherwise; lr / eps / weight_decay always
        # from the keywords.  Checked before any device work.
        if hparams is not None and getattr(hparams, "optimizer", None):
            optimizer = hparams.optimizer
            momentum = getattr(hparams, "momentum", momentum)
        if optimizer not in OPTIMIZERS:
            raise ValueError('optimizer not recognized!')
        clipping = clip_grad_norm is not None or clip_grad_value is not None
        if clipping:
            check_clip_args(clip_grad_norm, clip_grad_value, "TrainStep(clip_grad_norm=, clip_grad_value=)")
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        if occupancy is not None:
            if not isinstance(occupancy, TrainOccupancy):
                raise ValueError(f"TrainStep(occupancy=): expected a TrainOccupancy, got {type(occupancy).__name__}")
            if self.world > 1 or (bool(force_dp) and dist.is_available() and dist.is_initialized()):
                # sized, not built: the replicas are bit-identical, so every rank could refresh on its own and get the
                # same grids — but nothing of it has run on two GPUs
                raise ValueError("TrainStep(occupancy=): not available under data parallelism")
            if occupancy.model is not model:
                raise ValueError("TrainStep(occupancy=): the TrainOccupancy was built for another model")
        self.model = model
        self.arena = ParamArena(model.parameters())
        self.group = group
        self.use_graph = use_graph
        self.chunk = int(chunk)          # rays per model call (train.py:108-111); the default exceeds any batch size
        self.sync: Optional[GradSync] = None
        # force_dp: take the data-parallel code path (broadcast, gradient all-reduce, Adam behind it) in a ONE-rank
        # group too — a one-GPU box can then run the captured RCCL all-reduce (tests, bench.py --force-dp)
        self.dp = self.world > 1 or (bool(force_dp) and dist.is_available() and dist.is_initialized())
        self.capture_collective = bool(capture_collective)
        self.dp_graph = None             # how the N>1 step runs: "one graph" | "three pieces (<why>)"
        if self.dp:
            # replicas must start identical (Lightning DDP broadcasts module state from rank 0 at wrap time)
            dist.broadcast(self.arena.data, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
            self.arena.bump()
            # one all-reduce of the flat gradient buffer, or (overlap_grad_sync=True) two buckets with the first in
            # flight while the second is still being computed — off by default, see dist.GradSync
            self.sync = GradSync(self.arena, model, group, overlap=overlap_grad_sync)
        # hn_adam_step: one launch for all parameters, clears the gradient buffer on the way out, graph-capturable
        # (on one GPU it is part of the captured step; with N>1 it follows the gradient all-reduce and scales the
        # summed gradient by 1/world itself)
        # Opt-in, off by default (HN_FUSE_REDUCE=1, optim.FUSE_REDUCE): without a collective between backward and the
        # optimizer (one GPU) and without clipping, the launch that completes the gradient also applies the update
        # (hn_mlp_wgrad_reduce_adam: no gradient write-back, no second pass over the arena)
        if optimizer == "adam":
            self.optimizer = ArenaAdam(self.arena, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, zero_grad=True,
                                       grad_scale=1.0 / self.world,
                                       fuse_reduce=(not self.dp) and _optim.FUSE_REDUCE and not clipping)
        else:
            # SGD / RAdam / Ranger: one launch of their own after the gradient is complete (no fused reduce); betas at
            # the class defaults, as get_optimizer passes none
            self.optimizer = make_optimizer(optimizer, self.arena, lr=lr, eps=eps, weight_decay=weight_decay,
                                            momentum=momentum, zero_grad=True, grad_scale=1.0 / self.world)
        # optim.GradClip or None: value clip, then global-norm clip of the (all-reduced) gradient buffer, right before
        # every optimizer launch (_optimizer_step).  The fused reduce + Adam launch never materialises the gradient, so
        # a clipped step always takes the two-launch form (fuse_reduce above)
        self.clip = (GradClip(self.arena, max_norm=clip_grad_norm, clip_value=clip_grad_value,
                              grad_scale=1.0 / self.world) if clipping else None)
        # 'steplr' of the reference (utils/__init__.py:43-46): stepped once per epoch by the caller (`epoch_end`)
        self.scheduler = MultiStepLR(self.optimizer, decay_step, decay_gamma) if decay_step else None
        # any scheduler of the reference's get_scheduler (utils/__init__.py:43-59): `hparams` carries lr_scheduler
        # ('steplr' | 'cosine' | 'poly') and its arguments, warmup_epochs / warmup_multiplier for the warm-up wrapper
        if hparams is not None and getattr(hparams, "lr_scheduler", None):
            self.scheduler = get_scheduler(hparams, self.optimizer)
        self.loss_fn = MSELoss()
        # losses.BackgroundLoss or None: a term of its own ahead of the ray chunks (_forward_backward_body)
        self.background_loss = background_loss
        self._bg_rng: Optional[Dict[str, torch.Tensor]] = None   # its injected draws, split off `rng` (_split_rng)
        # losses.DistortionLoss or None: a term on every ray chunk's compositing weights (_forward_backward_body)
        self.distortion_loss = distortion_loss
        # TrainOccupancy or None: one clip launch at the head of the step body; its schedule runs in step(), ahead of the
        # replay.  With it the distortion loss normalises depth over each ray's CLIPPED interval (the model's z).
        self.occupancy = occupancy
        # batcher (datasets.RayBatcher): step() takes no tensors; the batch is gathered on the device by the first
        # launch of the step's graph (eager and data-parallel steps: by a launch of its own ahead of the step)
        self.batcher = batcher
        self._rays = self._rgbs = None                         # the fixed buffers the step body reads (_bind_*)
        self._rng: Optional[Dict[str, torch.Tensor]] = None    # ... of injected random draws (tests)
        self._log: Dict[str, torch.Tensor] = {}                # ... and writes: the log of the step that ran last
        # the captured programs by key (step()).  The tensor-fed step keeps ONE (its binder drops it together with the
        # buffers it was captured on); a batcher one per key: the full batch and the epoch's short last one
        self._batched: Dict[tuple, _Program] = {}
        self._graph = None          # _Program.run of the step that ran last, None once that program was dropped
        self._graph_state = None    # (precision, model.training) the programs were captured under
        self._batched_rng: Dict[int, Dict[str, torch.Tensor]] = {}       # the batcher's rng buffers per row count
        self._batched_bg_rng: Optional[Dict[str, torch.Tensor]] = None   # ... and its background draws, for all row counts

    # ---- the step body (what gets captured) ---------------------------------------------------
    def _forward_backward(self):
        with (self.sync.splitting() if self.sync is not None else contextlib.nullcontext()):
            self._forward_backward_body()

    def _forward_backward_body(self):
        b = self._rays.shape[0]
        loss_sum, dist_sum, psnr_in = None, None, []
        # rows the model renders: the step's rays, or (occupancy=) each clipped to its frame's occupied cells, then
        # rendered with the original directions as view directions, as inference.render_image does
        rows, clip = self._rays, None
        if self.occupancy is not None:
            clip = self.occupancy.clip(self._rays)
            rows = clip['rays']
        dl = self.distortion_loss
        bg = None
        if self.background_loss is not None:
            # a term of its own, handled exactly like a non-last ray chunk: back-propagated at once (its activations are
            # freed before the first chunk runs) and its held weight-gradient jobs launched now — only the LAST ray
            # chunk's held jobs overlap the all-reduce
            loss_bg = self.background_loss(self.model, rng=self._bg_rng)
            F.backward(loss_bg, self.background_loss.weight)
            F.flush_held_wgrads()
            bg = loss_bg.detach()
        # the reference renders `chunk` rays at a time and concatenates the results before the loss
        # (train.py:108-114); mean((rgb-gt)^2) over the batch = sum over chunks of (rays in chunk / B) x chunk mean,
        # so every chunk is back-propagated on its own (its activations are freed before the next chunk runs)
        for i in range(0, b, self.chunk):
            rays, rgbs = rows[i:i + self.chunk], self._rgbs[i:i + self.chunk]
            kw = {} if self._rng is None else {'rng': {k: v[i:i + self.chunk] for k, v in self._rng.items()}}
            ray_dict = model_utils.prepare_ray_dict(rays)
            if clip is not None:
                ray_dict['viewdirs'] = clip['viewdirs'][i:i + self.chunk]
            results = self.model(ray_dict, dict(_EXTRA), **kw)
            w = rays.shape[0] / b
            # the term's forward launches (one per level, right behind the compositing launches) write the gradient for
            # the root they are about to get
            terms = dl.per_level(self.model, results, root=dl.weight * w) if dl is not None else []
            loss = self.loss_fn(results, rgbs)
            if dl is None:
                F.backward(loss, w)      # into arena.grad (zeroed by the previous Adam launch); cached root gradient = w
            else:
                # ONE traversal: the compositing kernels and the MLP machines run backward once, with the gradients of
                # both losses
                F.backward_all([(loss, w)] + [(t, dl.weight * w) for t in terms])
            if i + self.chunk < b:
                F.flush_held_wgrads()        # only the LAST chunk's held jobs overlap with the all-reduce (a held
                                             # job keeps its chunk's activation stash alive)
            typ = 'fine' if 'fine' in results else 'coarse'
            with torch.no_grad():
                loss_sum = loss.detach() * w if loss_sum is None else loss_sum + loss.detach() * w
                psnr_in.append(results[typ]['rgb'].detach())
                if dl is not None:
                    d = terms[0].detach()
                    for t in terms[1:]:
                        d = d + t.detach()
                    d = d if w == 1.0 else d * w
                    dist_sum = d if dist_sum is None else dist_sum + d
        with torch.no_grad():
            pred = psnr_in[0] if len(psnr_in) == 1 else torch.cat(psnr_in, 0)
            self._log = {'train/loss': loss_sum, 'train/psnr': psnr(pred, self._rgbs)}
            if bg is not None:
                self._log['train/background_loss'] = bg          # unweighted
            if dist_sum is not None:
                self._log['train/distortion_loss'] = dist_sum    # unweighted
            if clip is not None:
                self._log['train/occupancy_hit'] = clip['hit_count'].to(torch.float32) / b      # the share of rays clipped to cells
                self._log['train/occupancy_span'] = clip['affine'][:, 1].mean()                 # the mean share of [near, far] kept

    def _optimizer_step(self):
        if self.clip is not None:
            self.clip.apply()
        self.optimizer.step()

    def _with_grad_norm(self, log):
        """'train/grad_norm': the norm before clipping, what clip_grad_norm_ returns (a device scalar the clip's launch
        overwrites every step: cloned with the rest of the log)."""
        if self.clip is not None and self.clip.max_norm is not None:
            log['train/grad_norm'] = self.clip.total_norm.clone()
        return log

    def _whole(self):
        self._forward_backward()
        self._optimizer_step()

    def _whole_dp(self):
        """forward + backward | ONE in-place SUM all-reduce of the gradient buffer | Adam, as one capturable program
        (RCCL's kernel is enqueued on the capturing stream like any launch): one graph replay per step, no host in
        the loop between backward and the optimizer (reference: Lightning DDP's reduce inside backward,
        train.py:224-229)."""
        self._forward_backward()
        F.flush_held_wgrads()
        self.arena.all_reduce_sum(self.group, force=True)
        self._optimizer_step()

    def _state(self):
        """Parameters, gradient buffer and every tensor of the optimizer's state (step counter, moments, momentum /
        slow buffers)."""
        o = self.optimizer
        opt = (o.exp_avg, o.exp_avg_sq, o.step_count) if isinstance(o, ArenaAdam) else tuple(o.state_tensors())
        return (self.arena.data, self.arena.grad) + opt

    def _snapshot(self):
        return [t.clone() for t in self._state()]

    def _restore(self, snap):
        with torch.no_grad():
            for dst, src in zip(self._state(), snap):
                dst.copy_(src)
        self.arena.bump()

    def _capture(self, fn, warmup_fn=None):
        """Warm-up runs + capture execute `fn` (the warm-up runs: `warmup_fn` when given) for real; parameters,
        gradient buffer and optimizer state are put back afterwards so that the first step() applies exactly ONE
        update (and, with N>1, all-reduces ONE gradient)."""
        snap = self._snapshot()
        try:
            g = GraphedStep(fn, warmup=2, warmup_fn=warmup_fn)
        finally:
            self._restore(snap)
        return g

    def _capture_data_parallel(self):
        """Two graphs: forward + backward up to the first weight-gradient bucket | the held bucket (None when the
        model offers no split).  The warm-up runs execute both; the capture of the first leaves exactly one pass's
        held jobs behind, which the capture of the second consumes."""
        snap = self._snapshot()
        F.flush_held_wgrads()
        g1 = GraphedStep(self._forward_backward, warmup=2, mutates_params=False,
                         warmup_fn=lambda: (self._forward_backward(), F.flush_held_wgrads()))
        g2 = (GraphedStep(F.flush_held_wgrads, warmup=0, pool=g1.graph.pool(), mutates_params=False)
              if F.held_wgrads() else None)
        self._restore(snap)
        return g1, g2

    def _capture_dp(self):
        """The N>1 step as ONE graph when the collective can be captured (RCCL, single all-reduce); otherwise — gloo,
        the two-bucket overlap, or a capture that raised — graph | eager all-reduce | eager Adam, in this process
        (never a re-exec)."""
        why = None
        if self.sync.split is not None:
            why = "two overlapped buckets"
        elif not self.capture_collective:
            why = "capture_collective=False"
        elif not collective_capturable(self.group):
            why = f"backend {dist.get_backend(self.group)} stages through the host"
        else:
            g = None
            try:
                g = self._capture(self._whole_dp)
            except Exception as e:      # noqa: BLE001 (whatever the runtime says about capturing the collective)
                why = f"capturing the all-reduce raised {type(e).__name__}: {str(e)[:120]}"
                # a capture that died part-way may have queued weight-gradient shares whose stashes belong to the
                # abandoned graph's pool: they must never be launched
                F.drop_pending_wgrads()
            # every rank takes the SAME form of the step (a rank replaying one graph next to a rank issuing an eager
            # all-reduce would still match collective for collective, but time and behave differently): agree on it
            ok = torch.tensor([1.0 if g is not None else 0.0], device=self.arena.data.device)
            if self.world > 1:
                dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=self.group)
            if float(ok.item()) > 0.5:
                self.dp_graph = "one graph: forward + backward + all-reduce + Adam"
                return g
            if g is not None:
                why = "another rank could not capture the all-reduce"
                g = None
        self.dp_graph = f"three pieces: graph | eager all-reduce | Adam ({why})"
        return self._capture_data_parallel()

    def _whole_batched(self, rows: int):
        self.batcher.launch(rows)
        self._whole()

    def _capture_batched(self, rows: int):
        """The step of `rows` rays as one graph, hn_ray_batch first.  Each warm-up run gathers the epoch's first
        `rows` rays (cursor reset to 0: never past the permutation); the device state is put back with the optimizer
        state, so the first replay reads the batch that is due."""
        b = self.batcher
        state = b.state.clone()

        def warm():
            b.state.zero_()
            self._whole_batched(rows)
        try:
            return self._capture(lambda: self._whole_batched(rows), warmup_fn=warm)
        finally:
            b.state.copy_(state)

    def _capture_step(self, rows: int) -> _Program:
        """The step on the buffers bound now, captured in the form this TrainStep runs."""
        if self.dp:
            run = self._capture_dp()
        elif self.batcher is not None:
            run = self._capture_batched(rows)
        else:
            run = self._capture(self._whole)
        return _Program(run, self._log)

    def _run(self, run):
        """One step: ONE replay of a whole-step graph, or `run` = (fwd_bwd, held) in three pieces — a captured program's
        two graphs, or the eager step's uncaptured functions."""
        if isinstance(run, GraphedStep):
            return run()
        fwd_bwd, held = run
        fwd_bwd()
        if self.dp:
            self.sync.reduce(held, force=True)   # all-reduce(bucket 0) || held weight gradients, then all-reduce(bucket 1)
        self._optimizer_step()

    # ---- binding the step's inputs ----------------------------------------------------------------
    _BG_KEYS = ('bg_u', 'bg_n')

    def _split_rng(self, rng):
        """`rng` of step() -> (the per-ray draws of NerfModel.forward or None, the background loss's draws or None): the
        second never reaches the model and is never sliced per chunk."""
        if rng is None or not any(k in rng for k in self._BG_KEYS):
            return rng, None
        if self.background_loss is None:
            raise ValueError("step(rng=...): 'bg_u' / 'bg_n' given to a TrainStep without background_loss")
        if not all(k in rng for k in self._BG_KEYS):
            raise ValueError("step(rng=...): 'bg_u' and 'bg_n' come together")
        rest = {k: v for k, v in rng.items() if k not in self._BG_KEYS}
        return (rest or None), {k: rng[k] for k in self._BG_KEYS}

    @staticmethod
    def _fill(bufs, draws):
        """`draws` copied into the fixed buffers `bufs` in place; without buffers (None), owned clones become them."""
        if bufs is None:
            return {k: v.clone() for k, v in draws.items()}
        for k, v in draws.items():
            bufs[k].copy_(v)
        return bufs

    def _drop_programs(self, rng_rows: Optional[int] = None):
        """Forget the captured programs: all of them, or only those of `rng_rows` rows that read per-ray draws."""
        self._batched = {} if rng_rows is None else {key: prog for key, prog in self._batched.items()
                                                     if not (key[0] == rng_rows and key[1])}
        self._graph = None

    def _bind_tensors(self, rays, rgbs, rng):
        """The caller's tensors into owned buffers: copied in place while the shape of `rays` stays and `rng` / the
        background draws stay given or not given; otherwise cloned anew, and the program captured on the old ones goes."""
        rng, bg_rng = self._split_rng(rng)
        if (self._rays is None or self._rays.shape != rays.shape or (rng is None) != (self._rng is None)
                or (bg_rng is None) != (self._bg_rng is None)):
            self._rays, self._rgbs = rays.clone(), rgbs.clone()
            self._rng = self._bg_rng = None
            self._drop_programs()
        else:
            self._rays.copy_(rays)
            self._rgbs.copy_(rgbs)
        self._rng = None if rng is None else self._fill(self._rng, rng)
        self._bg_rng = None if bg_rng is None else self._fill(self._bg_rng, bg_rng)

    def _bind_batch(self, rng):
        """The batcher's next batch: views of its buffers, one set of rng buffers per row count — replaced, with that row
        count's programs that read it, when the key set of `rng` changes — and one pair of background buffers for all."""
        rows = self.batcher.next_rows()              # host bookkeeping only; the cursor itself lives on the device
        self._rays, self._rgbs = self.batcher.views(rows)
        rng, bg_rng = self._split_rng(rng)
        if bg_rng is not None:
            self._batched_bg_rng = self._fill(self._batched_bg_rng, bg_rng)
        self._bg_rng = None if bg_rng is None else self._batched_bg_rng
        if rng is not None:
            bufs = self._batched_rng.get(rows)
            if bufs is None or set(bufs) != set(rng):
                bufs = None
                self._drop_programs(rng_rows=rows)
            self._batched_rng[rows] = self._fill(bufs, rng)
        self._rng = None if rng is None else self._batched_rng[rows]

    # ---- public -----------------------------------------------------------------------------------
    def step(self, rays: Optional[torch.Tensor] = None, rgbs: Optional[torch.Tensor] = None,
             rng: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """rays (B, 8|9), rgbs (B, 3) on the GPU; B must stay the same from call to call when graphs are on.
        `rng` optionally supplies the random draws of NerfModel.forward ('t_rand', 'u', 'noise_coarse', 'noise_fine',
        one row per ray) instead of torch's generator: parity runs against the CPU oracle share the draws this way.
        With a background loss, `rng` may also carry its draws 'bg_u' (batch_size, 2) and 'bg_n' (batch_size, 3).
        With a batcher, step() takes no rays / rgbs: the next batch of the batcher's epoch is gathered on the device
        (an epoch that ran out starts the next one); `rng` rows then match that batch's size."""
        if self.batcher is not None:
            if rays is not None or rgbs is not None:
                raise ValueError("TrainStep(batcher=...): step() takes no rays / rgbs")
            self._bind_batch(rng)
        elif rays is None or rgbs is None:
            raise ValueError("step() needs rays and rgbs (or a TrainStep built with batcher=...)")
        else:
            self._bind_tensors(rays, rgbs, rng)
        # what a captured graph froze besides the shapes: the precision mode and whether the model trains / evaluates
        state = (F.get_precision(), self.model.training)
        if self._graph_state != state:
            self._graph_state = state
            self._drop_programs()
        self.optimizer.sync_hyper()      # a replayed Adam launch reads lr & co. from device memory
        if self.occupancy is not None:
            self.occupancy.before_step()     # the refresh that is due, on the host side of the graph
        rows = self._rays.shape[0]
        if self.batcher is not None and (self.dp or not self.use_graph):
            # only the one-GPU graph holds the gather (_capture_batched); otherwise it runs on its own, ahead of the step
            self.batcher.launch(rows)
        if not self.use_graph:
            self._run((self._forward_backward, F.flush_held_wgrads))
        else:
            # what names a program: the rows and whether per-ray / background draws are injected, of the buffers bound above
            key = (rows, self._rng is not None, self._bg_rng is not None)
            prog = self._batched.get(key)
            if prog is None:
                prog = self._batched[key] = self._capture_step(rows)
            self._graph, self._log = prog.run, prog.log
            self._run(prog.run)
        # a replay updates the parameters without running any Python: tell the weight packers (an eval forward
        # after this must repack — see machine.MlpRunner.pack)
        self.arena.bump()
        machine.note_parameters_changed()
        log = self._with_grad_norm({k: v.clone() for k, v in self._log.items()})     # graph outputs are overwritten by the next replay
        log['lr'] = self.optimizer.param_groups[0]['lr']
        return log

    def epoch_end(self):
        """Advance the LR schedule by one epoch (Lightning steps the scheduler of configure_optimizers per epoch); with
        a batcher, end its epoch too: the next step() draws a new order (for the epoch a set_epoch() call in between
        names, else the next one)."""
        if self.scheduler is not None:
            self.scheduler.step()
        if self.batcher is not None:
            self.batcher.end_epoch()

