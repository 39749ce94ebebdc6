"""Training driver with the reference's ``utils/train_utils.py`` surface (TrainConfig, count_parameters,
init_lr_scheduler, prepare_data_loaders, run_train_model, simple_train_model) plus the explicit
``train_step`` the north star asks for — the loop body of utils/train_utils.py:128-148:

    lr = get_lr(step) -> zero_grad -> loss, _ = model(inputs, labels, date_info) -> backward
    (-> DP gradient mean) -> clip_grad_value_(1.0) -> AdamW.step()

MI355X-first implementation: all trainable parameters live in ONE flat fp32 arena (params, grads, Adam
moments), so clip + AdamW + zero_grad is a single HBM-bound kernel launch (fk_adamw_step) and the data-parallel
gradient exchange is a handful of large contiguous RCCL all-reduces issued from autograd hooks while the
backward is still running (one process per GPU, torch.distributed 'nccl' = RCCL over xGMI).  No accelerate /
wandb dependency (accelerate's DDP wrapping, utils/train_utils.py:97-101,122, is what GradSync replaces, and its loader
sharding what ShardedLoader does).
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from pathlib import Path
from typing import Callable, List, Optional

import torch

from .. import engine as E
from .. import kernels as K


@dataclass
class TrainConfig():
    exp_name: str = 'default'

    batch_size: int = 256
    grad_accum: int = 1

    p_augs: float = 0.0

    learning_rate: float = 1e-3
    weight_decay: float = 1e-5

    max_steps: int = 100_000
    eval_interval: int = 1_000

    use_scheduler: bool = True
    warmup_iters: int = 2_000
    lr_decay_iters: int = 50_000

    num_workers: int = 3
    pin_memory: bool = True

    grad_clip: float = 1.0
    grad_clip_norm: float = 0.0          # > 0: clip the global gradient norm (clip_grad_norm_) instead of the values; needs grad_clip = 0
    mixed_precision: bool = True

    visualize_predictions: bool = False


def count_parameters(model):
    n_trainable = sum(p.numel() for p in model.parameters() if p.requires_grad)
    n_total = sum(p.numel() for p in model.parameters())
    print(f"Total: {n_total/1e6:.2f}M, Trainable: {n_trainable/1e6:.2f}M")
    return n_total, n_trainable


def init_lr_scheduler(config) -> Callable[[int], float]:
    """linear warm-up to lr over warmup_iters, cosine to lr/10 at lr_decay_iters, constant after
    (utils/train_utils.py:49-72)."""
    lr, warm, decay = config.learning_rate, config.warmup_iters, config.lr_decay_iters
    min_lr = lr / 10
    constant = not config.use_scheduler

    def get_lr(it):
        if constant:
            return lr
        if it < warm:
            return lr * it / warm
        if it > decay:
            return min_lr
        ratio = (it - warm) / (decay - warm)
        assert 0 <= ratio <= 1
        return min_lr + 0.5 * (1.0 + math.cos(math.pi * ratio)) * (lr - min_lr)

    return get_lr


def prepare_data_loaders(train_dataset, val_dataset, config):
    batch_size = config.batch_size // config.grad_accum
    mk = lambda ds, shuffle: torch.utils.data.DataLoader(ds, batch_size=batch_size, shuffle=shuffle,
                                                         num_workers=config.num_workers, pin_memory=config.pin_memory)
    return mk(train_dataset, True), mk(val_dataset, False)


# ------------------------------------------------------------------------------------------------ arena + optimizer
def _unique_trainable(model) -> List[torch.nn.Parameter]:
    seen, out = set(), []
    for p in model.parameters():
        if p.requires_grad and id(p) not in seen:
            seen.add(id(p))
            out.append(p)
    return out


class ParamArena:
    """Flat fp32 storage for all trainable parameters (+ grads): every Parameter becomes a view into ``flat``
    and its ``.grad`` a view into ``grad`` (tensors padded to 16 bytes so vector kernels stay aligned)."""

    def __init__(self, model: torch.nn.Module):
        self.params = _unique_trainable(model)
        assert self.params, "model has no trainable parameters"
        dev = self.params[0].device
        self.offsets, off = [], 0
        for p in self.params:
            assert p.dtype == torch.float32 and p.device == dev, "parameters must be fp32 masters on one device"
            self.offsets.append(off)
            off += (p.numel() + 3) // 4 * 4
        self.numel = off
        self.flat = torch.zeros(off, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(off, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, o in zip(self.params, self.offsets):
                view = self.flat[o:o + p.numel()].view(p.shape)
                view.copy_(p.data)
                p.data = view
                p.grad = self.grad[o:o + p.numel()].view(p.shape)
                p._fk_arena = True          # engine.wgrad may accumulate weight gradients straight into the arena
        E.bump_weight_epoch()

    def rebind_grads(self):
        """(re)attach .grad views, e.g. after someone called zero_grad(set_to_none=True)."""
        for p, o in zip(self.params, self.offsets):
            if p.grad is None or p.grad.data_ptr() != self.grad.data_ptr() + 4 * o:
                g = self.grad[o:o + p.numel()].view(p.shape)
                if p.grad is not None:
                    g.copy_(p.grad)
                p.grad = g


class GradSync:
    """Data-parallel gradient exchange (what accelerate's DDP wrap does implicitly in the reference,
    utils/train_utils.py:122,139): contiguous buckets of the flat grad arena are all-reduced (SUM; the mean's
    1/world is folded into the optimizer kernel) as soon as every parameter of the bucket has its gradient,
    asynchronously on the process group's communication stream, so the exchange overlaps the remaining backward."""

    def __init__(self, arena: ParamArena, group=None, bucket_bytes: int = 8 << 20, always: bool = False, measure: bool = False,
                 register: bool = True):
        import torch.distributed as dist
        self.dist, self.group, self.arena = dist, group, arena
        # measure=True: bracket the wait for the buckets in finish() with timestamps on the compute stream (HIP events; wall clock for
        # CPU tensors) -> exposed_ms_mean(): how long the step sat waiting for the exchange after its last backward kernel
        self.measure, self._exposed = measure, []
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        self.enabled = True
        # always=True: issue the collectives also in a one-rank group (identity) — how the RCCL path is rehearsed on a one-GPU box
        self.active = self.world > 1 or (always and dist.is_available() and dist.is_initialized())
        self.buckets: List[tuple] = []           # (start, end, n_params)
        self.bucket_of: List[int] = []
        cap = max(1, bucket_bytes // 4)
        start, count = 0, 0
        for i, (p, o) in enumerate(zip(arena.params, arena.offsets)):
            end = o + (p.numel() + 3) // 4 * 4
            if count and end - start > cap:
                self.buckets.append((start, o, count))
                start, count = o, 0
            self.bucket_of.append(len(self.buckets))
            count += 1
        self.buckets.append((start, arena.numel, count))
        self._pending = [0] * len(self.buckets)
        self._launched = [False] * len(self.buckets)
        self._works = []
        if self.active:
            # replicas start from rank 0's parameters: what wrapping the model in DDP does in the reference
            # (accelerator.prepare, utils/train_utils.py:122) — identical seeds are not relied upon
            self.broadcast_parameters()
            if register:                                       # (FusedAdamW calls on_grad from its own per-parameter hook instead: one
                for i, p in enumerate(arena.params):           # Python hook per parameter costs ~5 us of host time per backward)
                    hook = self._make_hook(self.bucket_of[i])
                    p.register_post_accumulate_grad_hook(hook)     # also fires when engine.wgrad wrote the gradient itself

    def _mark(self):
        if self.arena.grad.is_cuda:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            return ev
        import time
        return time.perf_counter()

    def exposed_ms_mean(self, last: Optional[int] = None) -> float:
        """mean over the last `last` measured steps (all by default) of the compute stream's wait for the exchange, in ms; call after
        a device synchronisation"""
        pairs = self._exposed[-last:] if last else self._exposed
        if not pairs:
            return 0.0
        ms = [a.elapsed_time(b) if hasattr(a, "elapsed_time") else (b - a) * 1e3 for a, b in pairs]
        return sum(ms) / len(ms)

    def broadcast_parameters(self, src: int = 0):
        """Every rank takes the master parameters of group rank `src` (one collective over the flat arena)."""
        if self.active:
            gsrc = self.dist.get_global_rank(self.group, src) if self.group is not None else src
            self.dist.broadcast(self.arena.flat, src=gsrc, group=self.group)
            E.bump_weight_epoch()

    def on_grad(self, i: int) -> None:
        """parameter i of the arena has its gradient: counts towards its bucket, which goes out when complete"""
        if not (self.active and self.enabled):
            return
        b = self.bucket_of[i]
        self._pending[b] += 1
        if self._pending[b] == self.buckets[b][2]:
            self._launch(b)

    def _make_hook(self, b: int):
        def hook(_param):
            if not self.enabled:
                return
            self._pending[b] += 1
            if self._pending[b] == self.buckets[b][2]:
                self._launch(b)
        return hook

    def _launch(self, b: int):
        s, e, _ = self.buckets[b]
        self._launched[b] = True
        side = E.wgrad_stream()
        if side is not None:
            # the bucket may hold gradients produced on the weight-gradient stream AND on the main stream: order the
            # collective after both by issuing it from the side stream once that has caught up with the main one
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                w = self.dist.all_reduce(self.arena.grad[s:e], op=self.dist.ReduceOp.SUM, group=self.group, async_op=True)
        else:
            w = self.dist.all_reduce(self.arena.grad[s:e], op=self.dist.ReduceOp.SUM, group=self.group, async_op=True)
        self._works.append(w)

    def finish(self) -> float:
        """Launch whatever has not gone out (unused parameters), wait for all buckets; returns the factor that turns
        the summed gradient into the DDP mean."""
        if self.active and self.enabled:
            for b in range(len(self.buckets)):
                if not self._launched[b]:
                    self._launch(b)
            side = E.wgrad_stream()
            t0 = self._mark() if self.measure else None
            for w in self._works:
                if side is not None:
                    with torch.cuda.stream(side):
                        w.wait()
                else:
                    w.wait()
            if self.measure:
                if side is not None:
                    torch.cuda.current_stream().wait_stream(side)
                self._exposed.append((t0, self._mark()))
        self._works.clear()
        self._pending = [0] * len(self.buckets)
        self._launched = [False] * len(self.buckets)
        return 1.0 / self.world if self.enabled else 1.0


def decay_groups(model: torch.nn.Module, weight_decay: float) -> List[dict]:
    """The two parameter groups of the reference's GPT.configure_optimizers (models/gpt2_model.py:286-298): trainable tensors with
    dim() >= 2 (matmul weights, embeddings) decayed, the rest (biases, norm weights) not; a tied tensor appears once.  Frozen parameters
    are in neither group.  Low-rank adapters (`lora_A` / `lora_B`, GPT.add_lora) are not decayed: decay would pull the correction B A
    to zero, i.e. back to the pre-trained weight, at a rate unrelated to the decay of the weight they correct."""
    ps = _unique_trainable(model)
    lora = {id(p) for n, p in model.named_parameters() if n.endswith(('.lora_A', '.lora_B'))}
    decayed = [p for p in ps if p.dim() >= 2 and id(p) not in lora]
    return [{'params': decayed, 'weight_decay': weight_decay},
            {'params': [p for p in ps if p.dim() < 2 or id(p) in lora], 'weight_decay': 0.0}]


def adamw_tables(offsets, sizes, group_of, touched, lag, t: int, max_slots: int = K.ADAMW_MAX_SLOTS):
    """The launches of one grouped update, from the arena layout (element offset and size of each parameter, in arena order), the
    group index of each parameter, which parameters received a gradient, how many steps each has sat out (None: none ever did) and the
    optimizer's step count t (including this step).  A pure function: nothing is modified.

    Returns a list of (segments, slots), one entry per launch: segments = [(begin, end, slot)] sorted by begin, edges multiples of 4,
    adjacent parameters of equal slot merged; slots = [(group, step)], step = t - lag being the parameter's own bias-correction count.
    A parameter without a gradient is in no segment (torch.optim.AdamW: `if p.grad is None: continue`).  A launch carries at most
    max_slots slots: the distinct (group, step) pairs are numbered in order of first appearance, and launch k takes the segments of
    pairs k * max_slots .. (k + 1) * max_slots - 1 -- one launch unless many parameters have sat out different numbers of steps."""
    keys, merged = {}, []                               # (group, step) -> number; [(begin, end, number)]
    for i, (o, n) in enumerate(zip(offsets, sizes)):
        if not touched[i]:
            continue
        key = (int(group_of[i]), int(t) - (0 if lag is None else int(lag[i])))
        k = keys.setdefault(key, len(keys))
        e = o + (n + 3) // 4 * 4
        if merged and merged[-1][1] == o and merged[-1][2] == k:
            merged[-1] = (merged[-1][0], e, k)
        else:
            merged.append((o, e, k))
    order = list(keys)
    launches = []
    for first in range(0, len(order), max_slots):
        segs = [(b, e, k - first) for b, e, k in merged if first <= k < first + max_slots]
        launches.append((segs, order[first:first + max_slots]))
    return launches


class FusedAdamW:
    """torch.optim.AdamW semantics (betas .9/.999, eps 1e-8, decoupled decay, utils/train_utils.py:117-119) + clip_grad_value_ (:142),
    as one kernel over the arena.  Without `param_groups` every parameter is in one group, as in the reference's training loop.

    param_groups: a list of dicts with `params` and any of `weight_decay`, `betas`, `eps`, `lr`, `lr_scale` (the rest comes from the
    constructor's arguments); trainable parameters that no dict lists form a last, default group.  train_step / GraphedTrainStep set
    each group's lr to the schedule's value times its `lr_scale`.  The arena keeps model.parameters() order whatever the groups are.
    grad_clip_norm > 0: torch.nn.utils.clip_grad_norm_ (global L2 norm over the parameters that received a gradient, after the
    data-parallel mean) instead of the value clip; `last_grad_norm` is then a one-element device tensor holding the norm of the last
    step (reading it synchronises; the optimizer never does).  Groups or the norm clip take fk_adamw_step_groups: one launch for the
    whole arena (two with the norm), driven by a segment table that is uploaded only when its content changes."""

    def __init__(self, model: torch.nn.Module, lr: float = 1e-3, weight_decay: float = 1e-2, betas=(0.9, 0.999),
                 eps: float = 1e-8, grad_clip: Optional[float] = None, group=None, bucket_bytes: int = 8 << 20,
                 overlap_wgrad: Optional[bool] = None, sync_always: bool = False, param_groups: Optional[List[dict]] = None,
                 grad_clip_norm: Optional[float] = None):
        if (grad_clip or 0.0) > 0 and (grad_clip_norm or 0.0) > 0:
            raise ValueError("grad_clip (clip_grad_value_) and grad_clip_norm (clip_grad_norm_) are alternatives: set one of them")
        if param_groups is not None:                      # checked before the arena takes the parameters over
            param_groups = [dict(g) for g in param_groups]
            trainable, listed = {id(p) for p in _unique_trainable(model)}, set()
            for gi, g in enumerate(param_groups):
                g['params'] = list(g['params'])
                for p in g['params']:
                    if id(p) not in trainable:
                        raise ValueError(f"param_groups[{gi}] lists a tensor {tuple(p.shape)} that is not a trainable parameter of the model")
                    if id(p) in listed:
                        raise ValueError(f"param_groups[{gi}] lists a parameter {tuple(p.shape)} that is already in a group")
                    listed.add(id(p))
        self.arena = ParamArena(model)
        if overlap_wgrad is None:
            overlap_wgrad = os.environ.get("FK_WGRAD_STREAM", "0") == "1"        # off by default: see engine.py (no speed-up with one-block-per-CU grids)
        if overlap_wgrad and self.arena.flat.is_cuda and E.wgrad_stream() is None:
            E.enable_wgrad_stream(True)
        self.m = torch.zeros_like(self.arena.flat)
        self.v = torch.zeros_like(self.arena.flat)
        if param_groups is None:
            self.param_groups = [dict(params=self.arena.params, lr=lr, weight_decay=weight_decay, betas=betas, eps=eps)]
            self._group_of = [0] * len(self.arena.params)
        else:
            rest = [p for p in self.arena.params if id(p) not in listed]
            self.param_groups = []
            for g in param_groups + ([dict(params=rest)] if rest else []):
                scale = float(g.get('lr_scale', 1.0))
                self.param_groups.append({**g, 'lr': g.get('lr', lr * scale), 'weight_decay': g.get('weight_decay', weight_decay),
                                          'betas': tuple(g.get('betas', betas)), 'eps': g.get('eps', eps), 'lr_scale': scale})
            where = {id(p): gi for gi, g in enumerate(self.param_groups) for p in g['params']}
            self._group_of = [where[id(p)] for p in self.arena.params]
        self.grad_clip = grad_clip
        self.grad_clip_norm = grad_clip_norm
        self.last_grad_norm: Optional[torch.Tensor] = None      # device scalar, set by a norm-clipped step
        self._tables = {}                # (touched, lag) -> [(segments, [(group, -lag)])]: the launches of adamw_tables at t = 0
        self._seg_dev = {}               # segments -> their device table
        self._sumsq = None               # (partials, norm) device buffers of the norm clip
        self.t = 0
        # torch.optim.AdamW leaves a parameter alone whose .grad is None (after the reference's zero_grad(set_to_none=True),
        # utils/train_utils.py:134, that is a parameter the backward never reached): no decay, no moment update, its own step count.
        # The arena's gradients are never None, so "was reached" is recorded by a post-accumulate-grad hook per parameter (it also
        # fires when engine.wgrad / engine.norm_bwd wrote the gradient into the arena themselves).
        self._touched = [False] * len(self.arena.params)
        self._lag: Optional[List[int]] = None       # per parameter: optimizer steps it sat out (None: no parameter ever did)
        self.sync = GradSync(self.arena, group, bucket_bytes, always=sync_always, register=False)
        for i, p in enumerate(self.arena.params):
            p.register_post_accumulate_grad_hook(self._make_touch_hook(i))

    def _make_touch_hook(self, i: int):
        if self.sync.active:
            def hook(_param):                  # one hook per parameter serves both: "reached by the backward" and the bucket's readiness
                self._touched[i] = True
                self.sync.on_grad(i)
        else:
            def hook(_param):
                self._touched[i] = True
        return hook

    def mark_touched(self, flags=None) -> None:
        """Declare which parameters received a gradient since the last step() when the gradients were not produced by an eager
        backward (a replayed hipGraph, a hand-written arena.grad): `flags` is a sequence of booleans, None = all of them."""
        n = len(self.arena.params)
        self._touched = [True] * n if flags is None else [bool(f) for f in flags]
        assert len(self._touched) == n

    def zero_grad(self, set_to_none: bool = True):
        self.arena.grad.zero_()
        self.arena.rebind_grads()
        self._touched = [False] * len(self.arena.params)

    def _update_ranges(self):
        """[(start, end, t)] element ranges of the arena to update with bias-correction step t: one range in the usual case (every
        parameter reached by the backward, none ever skipped); otherwise maximal runs of adjacent reached parameters with equal
        step counts.  Parameters the backward did not reach are left out (torch.optim.AdamW: `if p.grad is None: continue`)."""
        a = self.arena
        if all(self._touched) and self._lag is None:
            return [(0, a.numel, self.t)]
        if self._lag is None:
            self._lag = [0] * len(a.params)
        out = []
        for i, (p, o) in enumerate(zip(a.params, a.offsets)):
            if not self._touched[i]:
                self._lag[i] += 1
                continue
            e, t = o + (p.numel() + 3) // 4 * 4, self.t - self._lag[i]
            if out and out[-1][1] == o and out[-1][2] == t:
                out[-1] = (out[-1][0], e, t)
            else:
                out.append((o, e, t))
        return out

    def step(self):
        """clip + AdamW + zero_grad over the arena: ONE launch when every parameter received a gradient since the last step (every
        model of the reference, every step); a parameter that did not is skipped like torch.optim.AdamW skips `grad is None` — no
        weight decay, no moment decay, its bias-correction count does not advance (utils/train_utils.py:117-119,134,143)."""
        g = self.param_groups[0]
        a = self.arena
        p0, p1 = a.params[0], a.params[-1]
        if p0.data_ptr() != a.flat.data_ptr() + 4 * a.offsets[0] or p1.data_ptr() != a.flat.data_ptr() + 4 * a.offsets[-1]:
            raise RuntimeError("parameters no longer live in the optimizer's arena (model.to() / .float() after constructing "
                               "FusedAdamW?): build the optimizer after the model is on its final device")
        self.arena.rebind_grads()
        scale = self.sync.finish()
        side = E.wgrad_stream()
        if side is not None:
            torch.cuda.current_stream().wait_stream(side)      # join the weight-gradient stream before the update
        if not any(self._touched):
            # torch.optim.AdamW is a silent no-op when every .grad is None, and so is this; but here the usual way to get there is a
            # gradient that did not come from an eager backward (arena.grad written by hand, a replayed graph, gradients produced before
            # load_state_dict re-created the hooks) — say so instead of silently leaving the parameters alone.
            import warnings
            warnings.warn("FusedAdamW.step(): no parameter was reached by a backward since the last step, so nothing is updated; "
                          "if the gradients were written into arena.grad directly (or by a replayed graph), call mark_touched() first",
                          RuntimeWarning, stacklevel=2)
        self.t += 1
        if len(self.param_groups) == 1 and not (self.grad_clip_norm or 0.0) > 0:
            for s0, s1, t in self._update_ranges():
                K.adamw_step_(a.flat[s0:s1], a.grad[s0:s1], self.m[s0:s1], self.v[s0:s1], t, g['lr'], g['betas'][0], g['betas'][1],
                              g['eps'], g['weight_decay'], clip=self.grad_clip or 0.0, grad_scale=scale, zero_grad=True)
        else:
            self._step_groups(scale)
        self._touched = [False] * len(a.params)
        E.bump_weight_epoch()
        E.refresh_shadows(self.arena.params)       # every weight shadow re-packed from the new masters in one launch

    def _device_table(self, segs) -> torch.Tensor:
        key = tuple(segs)
        tab = self._seg_dev.get(key)
        if tab is None:                                   # a new table (first step, or the set of reached parameters changed): upload it
            if len(self._seg_dev) >= 8:
                self._seg_dev.clear()
            tab = self._seg_dev[key] = K.adamw_segments(segs, self.arena.flat.device)
        return tab

    def _step_groups(self, scale: float) -> None:
        """The grouped update: per launch of adamw_tables one fk_adamw_step_groups over the whole arena (one launch unless more than 16
        (group, step) pairs are alive), preceded by one fk_grad_sumsq when the global norm is clipped.  The per-step numbers (learning
        rates, bias-correction steps, the 1/world scale) travel by value with the launch; the device table only changes when the set
        of reached parameters or their lags change, so a steady-state step uploads nothing and never synchronises."""
        a = self.arena
        if self._lag is None and not all(self._touched):
            self._lag = [0] * len(a.params)
        key = (tuple(self._touched), None if self._lag is None else tuple(self._lag))
        launches = self._tables.get(key)
        if launches is None:
            if len(self._tables) >= 8:
                self._tables.clear()
            launches = self._tables[key] = adamw_tables(a.offsets, [p.numel() for p in a.params], self._group_of, self._touched, self._lag, 0)
        if self._lag is not None:                         # a parameter without a gradient sits this step out
            self._lag = [l + (not tch) for l, tch in zip(self._lag, self._touched)]
        max_norm = float(self.grad_clip_norm or 0.0)
        partials = norm = None
        if max_norm > 0 and launches:
            if self._sumsq is None:
                self._sumsq = (torch.empty(K.GRAD_SUMSQ_BLOCKS, dtype=torch.float32, device=a.flat.device),
                               torch.zeros(1, dtype=torch.float32, device=a.flat.device))
            partials, norm = self._sumsq
            # the norm is over every reached parameter: the one launch's own table, or the union of the launches' tables
            cover = launches[0][0] if len(launches) == 1 else sorted((b, e, 0) for segs, _ in launches for b, e, _ in segs)
            K.grad_sumsq_(a.grad, self._device_table(cover), partials)
        for segs, slots in launches:
            hyper = []
            for gi, neg_lag in slots:
                g = self.param_groups[gi]
                hyper.append((g['lr'], g['betas'][0], g['betas'][1], g['eps'], g['weight_decay'], self.t + neg_lag))
            K.adamw_step_groups_(a.flat, a.grad, self.m, self.v, self._device_table(segs), hyper, clip=self.grad_clip or 0.0,
                                 grad_scale=scale, zero_grad=True, max_norm=max_norm, partials=partials, norm_out=norm)
        if norm is not None:
            self.last_grad_norm = norm

    def state_dict(self):
        return dict(t=self.t, m=self.m, v=self.v, lag=None if self._lag is None else list(self._lag),
                    param_groups=[{k: v for k, v in g.items() if k != 'params'} for g in self.param_groups])

    def load_state_dict(self, sd):
        """Resume: step count, both moment arenas and the hyper-parameters (the parameters themselves travel with the model)."""
        assert sd["m"].numel() == self.m.numel() and sd["v"].numel() == self.v.numel(), "optimizer state of another model"
        self.t = int(sd["t"])
        self._lag = None if sd.get("lag") is None else [int(x) for x in sd["lag"]]
        self.m.copy_(sd["m"].to(self.m.device))
        self.v.copy_(sd["v"].to(self.v.device))
        for g, src in zip(self.param_groups, sd.get("param_groups", [])):
            g.update({k: v for k, v in src.items() if k != 'params'})


def enable_fused_head_loss(model: torch.nn.Module, on: bool = True) -> int:
    """Training loops that only use the loss (the reference's run_train_model discards the second output of model(...),
    utils/train_utils.py:138-139) can let the vocabulary heads skip the [rows, 50257] logits: sets `fuse_head_loss` on every sub-module
    that implements it (GPT, the notebook CE BrainFormer); their forward then returns (loss, None).  Returns how many were switched."""
    n = 0
    for m in model.modules():
        if type(m).__name__ in ("GPT", "BrainFormerCE"):
            m.fuse_head_loss = on
            n += 1
    return n


# ------------------------------------------------------------------------------------------------ the step
# What grad_accum > 1 means.  The reference wraps the step in `with accelerator.accumulate(model)` but zeroes the gradients BEFORE the
# forward (utils/train_utils.py:133-134), and accelerate's optimizer wrapper executes zero_grad() and step() only on "sync" micro-steps.
# So on a sync micro-step the gradients of the earlier micro-batches are wiped before the forward, and the update uses the gradient of
# THAT micro-batch alone, scaled by 1 / grad_accum (accelerator.backward divides the loss); the other micro-batches only contribute their
# logged loss.  tests/golden/train_accum.npz pins this against the reference's own loop running under accelerate.
#   "reference": reproduce exactly that (default: a drop-in gives the reference's numbers).  The backward of a non-sync micro-step
#                cannot influence anything, so only its forward runs (the loss is logged, :147).
#   "sum":       what the construct is meant to do: gradients of all grad_accum micro-batches summed (each loss / grad_accum), one
#                update — equal to one step on the concatenated batch for a mean-reduced loss.
ACCUMULATE = "reference"


class GradAccumulation:
    """accelerate's GradientState as the reference drives it (Accelerator(gradient_accumulation_steps=k), utils/train_utils.py:98,133):
    a micro-step is a sync step when it is the k-th since the last reset, or the last batch of the loader — which also resets the
    count (accelerate's sync_with_dataloader default)."""

    def __init__(self, grad_accum: int):
        self.k, self.count = max(1, int(grad_accum)), 0

    def sync(self, end_of_loader: bool = False) -> bool:
        if end_of_loader:
            self.count = 0
            return True
        self.count += 1
        return self.count % self.k == 0


def train_step(model, batch, optimizer: FusedAdamW, step: int, cfg: TrainConfig, scheduler=None,
               micro_step: int = 0, sync: Optional[bool] = None, accumulate: Optional[str] = None):
    """One iteration of the reference's hot loop (utils/train_utils.py:128-148): lr = get_lr(step) -> zero_grad -> forward ->
    backward (-> DP gradient mean) -> clip_grad_value_ -> AdamW.step().  With cfg.grad_accum > 1 call it once per micro-batch;
    `sync` says whether this micro-step ends an accumulation window (default: micro_step == grad_accum - 1; run_train_model passes
    accelerate's rule incl. the end of the loader), `accumulate` picks the semantics (module default ACCUMULATE, see above).
    Returns the un-scaled loss of this micro-batch (what the reference logs)."""
    get_lr = scheduler or init_lr_scheduler(cfg)
    lr = get_lr(step)
    for g in optimizer.param_groups:
        g['lr'] = lr * g.get('lr_scale', 1.0)
    inputs, labels, date_info = batch
    k = max(1, cfg.grad_accum)
    mode = accumulate or ACCUMULATE
    assert mode in ("reference", "sum"), mode
    last = (micro_step == k - 1) if sync is None else bool(sync)
    optimizer.sync.enabled = last
    if k > 1 and mode == "reference":
        if not last:
            with torch.no_grad():
                loss, _ = model(inputs, labels, date_info=date_info)
            return loss.detach()
        optimizer.zero_grad()             # :134 on a sync micro-step: whatever was accumulated is dropped
    loss, _ = model(inputs, labels, date_info=date_info)
    (loss / k if k > 1 else loss).backward()
    if last:
        optimizer.step()
    return loss.detach()


class GraphedTrainStep:
    """The hot loop's forward + backward captured ONCE as a hipGraph and replayed per batch; the update (whose learning
    rate changes every step) runs eagerly after each replay.  For the small configurations (gpt2-nano, SimpleMAE B=32)
    a step is ~300 launches of a few microseconds each and the Python/ctypes launch path, not the GPU, sets the step
    time; replaying a graph removes it.  Requirements: static batch shape, grad_accum == 1, a forward without host-side
    randomness.  With the weight-gradient side stream on (FusedAdamW(overlap_wgrad=True)) the dW GEMMs become a parallel
    branch of the graph.  Same numbers as ``train_step``: the captured kernels are the ones the eager step launches.
    Data parallel: no collective is captured — warm-up and capture run with the exchange switched off — and the gradient
    hooks do not fire on replay, so after each replay GradSync.finish() all-reduces the whole arena (every bucket, SUM, the
    1/world in the AdamW kernel) before the eager update.  That exchange is exposed (it does not overlap the backward as in
    ``train_step``); with two ranks each bucket is a + b either way, so the result is the eager step's bit for bit."""

    def __init__(self, model, batch, optimizer: FusedAdamW, cfg: TrainConfig, scheduler=None, warmup: int = 2):
        if cfg.grad_accum != 1:
            raise RuntimeError("GraphedTrainStep needs grad_accum == 1")
        self.model, self.optimizer, self.cfg = model, optimizer, cfg
        self.get_lr = scheduler or init_lr_scheduler(cfg)
        self.static = tuple(t.clone() if torch.is_tensor(t) else t for t in batch)
        if len(self.static) == 3 and self.static[2] is not None:
            # date_info is part of the static batch: int64 [B] on the device whatever form it came in (tensor on any device, Python int),
            # so that the captured kernels read a buffer which every call copies into
            self.static = (*self.static[:2], self._days(batch[2]).clone())
        optimizer.sync.enabled = False
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):                  # warm-up off the default stream: workspaces, shadows, autotune
            for _ in range(warmup):
                self._fwd_bwd()
        cur.wait_stream(side)
        optimizer.zero_grad()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss = self._fwd_bwd()
        self._touched = list(optimizer._touched)       # which parameters the captured backward reaches (hooks do not run on replay)
        optimizer.zero_grad()                          # capture recorded the launches, it did not run them

    def _fwd_bwd(self):
        inputs, labels, date_info = self.static
        loss, _ = self.model(inputs, labels, date_info=date_info)
        loss.backward()
        side = E.wgrad_stream()
        if side is not None:                            # join the weight-gradient branch: a captured graph must end on one stream
            torch.cuda.current_stream().wait_stream(side)
        return loss.detach()

    def _days(self, date_info):
        return E.day_ids(date_info, self.static[0].shape[0], self.static[0].device)

    def __call__(self, batch, step: int):
        if len(self.static) == 3 and torch.is_tensor(self.static[2]) and len(batch) == 3:
            if batch[2] is None:
                raise RuntimeError("GraphedTrainStep was captured with date_info, got None (use -1 for an unknown session)")
            batch = (*batch[:2], self._days(batch[2]))
        for dst, src in zip(self.static, batch):
            if torch.is_tensor(dst):
                if dst.shape != src.shape:
                    raise RuntimeError(f"GraphedTrainStep was captured for {tuple(dst.shape)}, got {tuple(src.shape)}")
                dst.copy_(src, non_blocking=True)
        lr = self.get_lr(step)
        for g in self.optimizer.param_groups:
            g['lr'] = lr * g.get('lr_scale', 1.0)
        self.graph.replay()
        self.optimizer.mark_touched(self._touched)
        self.optimizer.sync.enabled = True             # no bucket went out during the replay: finish() exchanges all of them
        self.optimizer.step()
        return self.loss


def _dist_info():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def init_distributed():
    """The process group of a data-parallel run -> (rank, world, created).  A default group that already exists is used as is
    (created False).  Otherwise, with WORLD_SIZE > 1 in the environment (torchrun, accelerate.notebook_launcher(...,
    num_processes=N)): the rank binds its GPU (LOCAL_RANK) before any other GPU call and creates the default group (created True:
    the caller destroys it), RCCL's defaults being those of bench.dp_env (NCCL_MAX_NCHANNELS=8, HSA_ENABLE_IPC_MODE_LEGACY=0 unless
    set).  Backend: $FK_DIST_BACKEND, else "nccl" (= RCCL); FK_DIST_BACKEND=gloo lets two ranks share one
    GPU, which RCCL refuses.  WORLD_SIZE unset or 1: (0, 1, False) without creating a group or touching the GPU."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size(), False
    if int(os.environ.get("WORLD_SIZE") or 1) <= 1:
        return 0, 1, False
    # set before set_device: the HSA runtime reads its variables when it starts, which set_device makes it do
    os.environ.setdefault("NCCL_MAX_NCHANNELS", "8")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
    torch.cuda.set_device(device)
    backend = os.environ.get("FK_DIST_BACKEND", "nccl")
    dist.init_process_group(backend, device_id=device if backend == "nccl" else None)
    return dist.get_rank(), dist.get_world_size(), True


def shard_batch(batch, rank: int, world: int):
    """accelerate ``split_batches=True`` (utils/train_utils.py:100): the loader batch is the GLOBAL batch and rank r
    gets the r-th contiguous slice."""
    if world == 1:
        return batch
    n = batch[0].shape[0]
    assert n % world == 0, f"global batch {n} not divisible by world size {world}"
    k = n // world
    return tuple(t[rank * k:(rank + 1) * k] if torch.is_tensor(t) else t for t in batch)


def _n_samples(batch) -> int:
    for x in batch:
        if torch.is_tensor(x) and x.dim() > 0:
            return x.shape[0]
    for x in batch:
        if isinstance(x, (list, tuple)):
            return len(x)
    raise ValueError("a batch needs a tensor or a list with one entry per sample")


def _per_sample(x, n: int) -> bool:
    """tensors and lists whose leading length is the batch's sample count are split; anything else (None, constants) is shared"""
    return (torch.is_tensor(x) and x.dim() > 0 and x.shape[0] == n) or (isinstance(x, (list, tuple)) and len(x) == n)


def _append_samples(x, first, idx: List[int], n: int):
    """field x of an n-sample batch followed by samples `idx` of the same field of the epoch's first batch"""
    if not _per_sample(x, n):
        return x
    if torch.is_tensor(x):
        return torch.cat([x, first[torch.tensor(idx, device=first.device)].to(x.device)])
    out = list(x) + [first[i] for i in idx]
    return tuple(out) if isinstance(x, tuple) else out


def _batch_crc(batch) -> int:
    import zlib
    crc = 0
    for x in batch:
        if torch.is_tensor(x):
            crc = zlib.crc32(x.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy(), crc)
        elif isinstance(x, (list, tuple)):
            crc = zlib.crc32(repr(list(x)).encode(), crc)
    return crc


def _check_same_batch(batch) -> None:
    """every rank holds the same global batch, else raise (one all-reduce of a CRC-32 of its bytes)"""
    import torch.distributed as dist
    c = _batch_crc(batch)
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
    t = torch.tensor([c, -c], dtype=torch.int64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    hi, lo = int(t[0]), -int(t[1])
    if hi != lo:
        raise RuntimeError(f"rank {dist.get_rank()}: the ranks' loaders yield different global batches (CRC-32 {c:#010x}, group "
                           f"min {lo:#010x} max {hi:#010x}); every rank must draw the same shuffled order (same seed, same draws from "
                           f"the CPU generator before each epoch)")


class ShardedLoader:
    """accelerate's ``prepare(loader)`` with ``split_batches=True, even_batches=True`` (utils/train_utils.py:100,122), done on the
    host.  The wrapped loader yields GLOBAL batches, the same ones in the same order on every rank (same seed, same draws from the
    CPU generator: the order a one-process run sees); rank r takes the r-th contiguous slice of each and copies only that slice to
    `device` (non_blocking: asynchronous when the loader pins memory).  A batch smaller than the global batch (an epoch's last) is
    first completed with the epoch's first samples, cycled if the epoch has fewer (accelerate's BatchSamplerShard).  The global
    batch is the loader's (or its batch sampler's) `batch_size`, else the size of each epoch's first batch.  With a process group,
    a checksum of each epoch's first global batch is compared across the ranks, and a mismatch raises instead of training on
    misaligned shards.  World 1: the loader's batches as they come, moved to `device`.  rank / world default to the process
    group's."""

    def __init__(self, loader, rank: Optional[int] = None, world: Optional[int] = None, device=None):
        import torch.distributed as dist
        r, w = _dist_info()
        self.loader, self.device = loader, device
        self.rank = r if rank is None else int(rank)
        self.world = w if world is None else int(world)
        assert 0 <= self.rank < self.world, (self.rank, self.world)
        self.check = self.world > 1 and dist.is_available() and dist.is_initialized()
        bs = getattr(loader, "batch_size", None)
        if bs is None:                                   # a DataLoader built from a batch_sampler
            bs = getattr(getattr(loader, "batch_sampler", None), "batch_size", None)
        self.batch_size = bs if isinstance(bs, int) else None
        if self.world > 1 and self.batch_size is not None and self.batch_size % self.world:
            raise ValueError(f"split_batches: the global batch ({self.batch_size}) must be a multiple of the world size ({self.world})")

    def __len__(self):
        return len(self.loader)

    def _to_device(self, batch):
        if self.device is None:
            return batch
        return tuple(x.to(self.device, non_blocking=True) if torch.is_tensor(x) else x for x in batch)

    def __iter__(self):
        if self.world == 1:
            for batch in self.loader:
                yield self._to_device(tuple(batch))
            return
        first, B = None, self.batch_size
        for batch in self.loader:
            batch = tuple(batch)
            n = _n_samples(batch)
            if first is None:
                first, B = batch, B or n
                if B % self.world:
                    raise ValueError(f"split_batches: the global batch ({B}) must be a multiple of the world size ({self.world})")
                if self.check:
                    _check_same_batch(batch)
            if n > B:
                raise ValueError(f"a batch of {n} samples from a loader whose global batch is {B}")
            if n < B:
                idx = [i % _n_samples(first) for i in range(B - n)]
                batch = tuple(_append_samples(x, f, idx, n) for x, f in zip(batch, first))
            k = B // self.world
            lo = self.rank * k
            yield self._to_device(tuple(x[lo:lo + k] if _per_sample(x, B) else x for x in batch))


def mean_val_loss(losses) -> float:
    """The validation loss of run_train_model from the per-batch losses of this rank's shards: each batch's loss averaged across
    the ranks (all-reduce), then the batches' mean — for a mean-reduced loss on equal shards the one-process value, so the best
    checkpoint does not depend on the world size."""
    v = torch.stack([x.detach().float().reshape(()) for x in losses])
    world = _dist_info()[1]
    if world > 1:
        import torch.distributed as dist
        dist.all_reduce(v, op=dist.ReduceOp.SUM)
        v = v / world
    return float(v.mean())


def save_model(model, path) -> None:
    """safetensors checkpoint with the reference's key names (utils/train_utils.py:172).  Parameters are views into the
    flat arena, which safetensors refuses to serialise as-is (shared storage), so tensors are cloned first."""
    import safetensors.torch
    sd = {k: v.detach().clone().contiguous() for k, v in model.state_dict().items() if v is not None}
    safetensors.torch.save_file(sd, str(path))


def _adapted(model):
    """the module that carries the adapters: the GPT itself, or the `llm_model` of a Franky"""
    for m in model.modules():
        if callable(getattr(m, "lora_state_dict", None)) and callable(getattr(m, "add_lora", None)):
            return m
    raise TypeError("the model has no GPT with add_lora / lora_state_dict")


def save_lora(model, path) -> None:
    """The adapters alone (GPT.lora_state_dict) as safetensors; rank, alpha and targets travel in the file's metadata."""
    import safetensors.torch
    gpt = _adapted(model)
    cfg = gpt.lora_config()
    if cfg is None:
        raise RuntimeError("the model has no adapters (add_lora first)")
    sd = {k: v.detach().clone().contiguous() for k, v in gpt.lora_state_dict().items()}
    meta = {"lora_rank": str(cfg["rank"]), "lora_alpha": repr(cfg["alpha"]), "lora_targets": ",".join(cfg["targets"])}
    safetensors.torch.save_file(sd, str(path), metadata=meta)


def load_lora(model, path) -> dict:
    """Read a save_lora file into the model: adds the adapters with the file's rank, alpha and targets when the model has none (a model
    that has some must have the same), then copies the tensors.  Returns dict(rank, alpha, targets)."""
    import safetensors
    import safetensors.torch
    gpt = _adapted(model)
    with safetensors.safe_open(str(path), framework="pt") as f:
        meta = f.metadata() or {}
    cfg = dict(rank=int(meta["lora_rank"]), alpha=float(meta["lora_alpha"]), targets=tuple(meta["lora_targets"].split(",")))
    if gpt.lora_config() is None:
        gpt.add_lora(rank=cfg["rank"], alpha=cfg["alpha"], targets=cfg["targets"])
    elif gpt.lora_config() != cfg:
        raise ValueError(f"the file's adapters {cfg} differ from the model's {gpt.lora_config()}")
    gpt.load_lora_state_dict(safetensors.torch.load_file(str(path)))
    return cfg


def run_train_model(model, datasets, config, project_name='transformer', save_folder=Path('logs'), logger=None):
    """Same contract as the reference (utils/train_utils.py:93-185): trains until max_steps, evaluates every eval_interval and
    saves the best model as safetensors.  Data parallel when launched one process per GPU (torchrun, or
    accelerate.notebook_launcher(run_train_model, args, num_processes=N)): init_distributed() creates the process group and it is
    destroyed on return (a group the caller made is used and left alone); the loaders' global batches are split on the host
    (ShardedLoader: accelerate's split_batches=True, even_batches=True); every rank evaluates its shard of each validation batch
    and the losses are averaged across the ranks (mean_val_loss), so the validation loss and the best checkpoint do not depend on
    the world size; rank 0 alone prints, logs and writes the checkpoint, and the ranks meet at a barrier after each evaluation."""
    import torch.distributed as dist
    rank, world, created = init_distributed()
    try:
        return _train_loop(model, datasets, config, save_folder, logger, rank, world)
    finally:
        if created:
            dist.destroy_process_group()


def _train_loop(model, datasets, config, save_folder, logger, rank: int, world: int):
    import safetensors.torch
    import torch.distributed as dist
    torch.manual_seed(42)
    device = torch.device('cuda', int(os.environ.get('LOCAL_RANK', 0)))
    torch.cuda.set_device(device)
    E.set_compute_dtype('bf16' if config.mixed_precision else 'fp32')
    save_folder = Path(save_folder) / config.exp_name
    if rank == 0:
        save_folder.mkdir(parents=True, exist_ok=True)
    train_dataset, val_dataset = datasets
    train_loader, val_loader = prepare_data_loaders(train_dataset, val_dataset, config)
    train_loader, val_loader = ShardedLoader(train_loader, rank, world, device), ShardedLoader(val_loader, rank, world, device)
    model.to(device).float()
    optimizer = FusedAdamW(model, lr=config.learning_rate, weight_decay=config.weight_decay, grad_clip=config.grad_clip,
                           grad_clip_norm=getattr(config, 'grad_clip_norm', 0.0))
    scheduler = init_lr_scheduler(config)
    overall_step, best_val = 0, float('inf')
    accum = GradAccumulation(config.grad_accum)
    done = False
    while not done:
        n_batches = len(train_loader)
        for i_batch, batch in enumerate(train_loader):
            loss = train_step(model, batch, optimizer, overall_step, config, scheduler,
                              sync=accum.sync(end_of_loader=i_batch == n_batches - 1))
            overall_step += 1
            if rank == 0:
                print('*', end='')
                if logger is not None:
                    log = {'train/loss': float(loss), 'lr': optimizer.param_groups[0]['lr']}
                    if optimizer.last_grad_norm is not None:          # float(loss) has synchronised already
                        log['train/grad_norm'] = float(optimizer.last_grad_norm)
                    logger(log, overall_step)
            if overall_step % config.eval_interval == 0:
                model.eval()
                with torch.no_grad():
                    mean_val = mean_val_loss([model(inputs, labels, date_info)[0] for inputs, labels, date_info in val_loader])
                if rank == 0:
                    print(f"overall_steps {overall_step}: {float(loss)}")
                    print(f"val loss: {mean_val}")
                    if logger is not None:
                        logger({'val/loss': mean_val}, overall_step)
                if mean_val < best_val:                 # the same value on every rank (all-reduced)
                    best_val = mean_val
                    if rank == 0:
                        path = save_folder / f"step_{overall_step}_loss_{mean_val:.4f}.safetensors"
                        save_model(model, path)
                        print('saved model: ', path.name)
                if world > 1:
                    dist.barrier()                      # no rank runs ahead of rank 0's checkpoint
                model.train()
            if overall_step > config.max_steps:
                if rank == 0:
                    print('Complete training')
                done = True
                break
    return model


def simple_train_model(model, datasets, config, project_name='transformer'):
    """Single-process variant (utils/train_utils.py:189-260): no gradient clipping."""
    cfg = TrainConfig(**{**config.__dict__, 'grad_clip': 0.0, 'grad_clip_norm': 0.0})
    return run_train_model(model, datasets, cfg, project_name, Path('logs'))
