"""Counterpart of /root/reference/train.py (train :77-131, eval :12-74) for the MI355X pipeline.

`train()` / `eval()` keep the reference signatures.  The step itself is the fused path
    forward (HIP) -> WeightedBCE fwd+bwd on the un-materialised x8 logits (HIP) -> backward (HIP)
    -> [RCCL all-reduce of the flat fp32 gradient buffer, bucketed per ConvBlock and overlapped with
       the rest of backward] -> fused Adam-amsgrad on the flat parameter buffer (HIP)
with the reference's semantics: Adam(lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=True)
(train.py:85), `lr *= 0.997` after every 200th iteration (train.py:108-110), checkpoint dict keys
{'iterations', 'model', 'optimizer'} (train.py:123-128).

Data parallelism (one process per GPU, torch.distributed backend "nccl" == RCCL over xGMI): each
rank runs the same step on its shard of the global batch; gradients are averaged with one
all-reduce per bucket issued as soon as the bucket's last gradient kernel has been enqueued, so
the collective of block i overlaps the backward kernels of blocks i-1..0.  BatchNorm statistics are
per rank (the torch DDP convention); optimizer state is replicated.
"""
from __future__ import annotations

import json
import math
import os
from time import time
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib as L
from .utils.metric_utils import calculate_metrics, calculate_metrics_device, f_score  # noqa: F401

LR_DECAY_FREQ = 200      # train.py:80
LR_DECAY = 0.997         # train.py:110


# ----------------------------------------------------------------------------------------------
# flat parameter / gradient storage
# ----------------------------------------------------------------------------------------------
class FlatParams:
    """All trainable parameters of a model as views of ONE fp32 buffer (and their gradients as views
    of another), in nn.Module.parameters() order, each start padded to 4 floats.  The per-block
    slices [start, end) are the all-reduce buckets."""

    def __init__(self, model: torch.nn.Module, n_buckets: Optional[int] = None, grads: bool = True):
        """n_buckets: how many all-reduce buckets the per-group slices are merged into (None: $SED_DDP_BUCKETS, default 2;
        0: one bucket per top-level group, the round-1 layout kept for A/B runs; 1: a single flat all-reduce).
        grads=False: no gradient buffer (a mean teacher's parameters are never differentiated)."""
        named = list(model.named_parameters())
        if not named:
            raise ValueError("model has no parameters")
        dev = named[0][1].device
        self.names = [n for n, _ in named]
        self.offsets: Dict[str, int] = {}
        off = 0
        for n, p in named:
            self.offsets[n] = off
            off += (p.numel() + 3) // 4 * 4
        self.numel = off
        self.p = torch.zeros(off, dtype=torch.float32, device=dev)
        self.g = torch.zeros(off, dtype=torch.float32, device=dev) if grads else None
        self.P: Dict[str, torch.Tensor] = {}
        self.G: Dict[str, torch.Tensor] = {}
        for n, p in named:
            o = self.offsets[n]
            view = self.p[o:o + p.numel()].view(p.shape)
            view.copy_(p.data)
            p.data = view                      # the nn.Parameter now aliases the flat buffer
            self.P[n] = view
            if grads:
                self.G[n] = self.g[o:o + p.numel()].view(p.shape)
        self.model = model
        self.groups = self._make_buckets()
        if n_buckets is None:
            n_buckets = int(os.environ.get("SED_DDP_BUCKETS", "2"))
        self.buckets = self._merge_buckets(self.groups, n_buckets)

    def _make_buckets(self) -> List[tuple]:
        """(start, end) per top-level group in BACKWARD completion order: event_fc first (after att_fc on a model with the
        attention head), then conv_blocks.N-1 ... conv_blocks.0."""
        groups: Dict[str, List[int]] = {}
        order: List[str] = []
        for n in self.names:
            key = ".".join(n.split(".")[:2]) if n.startswith("conv_blocks.") else n.split(".")[0]
            if key not in groups:
                groups[key] = [self.offsets[n], 0]
                order.append(key)
            numel = int(np.prod(self.P[n].shape))
            groups[key][1] = self.offsets[n] + (numel + 3) // 4 * 4
        return [(k, groups[k][0], groups[k][1]) for k in reversed(order)]

    @staticmethod
    def _merge_buckets(groups, n_buckets: int, head_share: float = 0.85):
        """Merge the per-group slices (backward completion order, contiguous in the flat buffer) into at most `n_buckets`
        all-reduces.  The gradient buffer is 2.3 MB: every collective is latency-bound, so fewer is better; two
        keep the overlap -- the head bucket (late layers, >= 85 % of the elements) goes out while the first blocks' backward
        still runs, the small tail bucket is the only exposed one.  Each entry: (keys, start, end); a bucket is ready when
        the LAST of its keys is."""
        if n_buckets <= 0 or n_buckets >= len(groups):
            return [((k,), s, e) for (k, s, e) in groups]
        total = sum(e - s for _, s, e in groups)
        if n_buckets == 1:
            cuts = [len(groups)]
        else:
            acc, cut = 0, len(groups) - 1
            for i, (_, s, e) in enumerate(groups[:-1]):
                acc += e - s
                if acc >= head_share * total:
                    cut = i + 1
                    break
            cuts = [cut, len(groups)]
            # (more than two buckets: split the head evenly by group count)
            if n_buckets > 2 and cut > 1:
                step = max(1, cut // (n_buckets - 1))
                cuts = sorted(set(list(range(step, cut, step))[: n_buckets - 2] + [cut, len(groups)]))
        out, lo = [], 0
        for hi in cuts:
            part = groups[lo:hi]
            if part:
                out.append((tuple(k for k, _, _ in part), min(s for _, s, _ in part), max(e for _, _, e in part)))
            lo = hi
        return out

    def aliased(self) -> bool:
        """False once something (e.g. model.to()) replaced the parameter storages."""
        for n, p in self.model.named_parameters():
            if p.data_ptr() != self.P[n].data_ptr():
                return False
        return True

    def tensor_dict(self) -> Dict[str, torch.Tensor]:
        d = dict(self.P)
        d.update({n: b for n, b in self.model.named_buffers()})
        return d


def data_parallel_enabled(group=None) -> bool:
    """True when the trainer runs its collectives on `group`: a process group of more than one rank, or any initialised group
    under SED_DDP_FORCE=1 (test hook: the collectives then run on a world-size-1 group too, so that one GPU can execute the RCCL
    path -- librccl, async handles, stream ordering -- tests/test_gpu_ddp.py)."""
    import torch.distributed as dist
    force = os.environ.get("SED_DDP_FORCE", "0") == "1"
    return dist.is_available() and dist.is_initialized() and (dist.get_world_size(group) > 1 or force)


class GradAllReducer:
    """Bucketed, overlapped gradient averaging over torch.distributed (RCCL on the GPU box, gloo
    in the CPU tests).  No-op for world_size 1.  `buckets`: [(keys, start, end)] from FlatParams (a bare (key, start, end)
    triple is accepted as a one-key bucket)."""

    def __init__(self, flat_g: torch.Tensor, buckets, group=None):
        import torch.distributed as dist
        self.dist = dist
        self.enabled = data_parallel_enabled(group)
        self.world = dist.get_world_size(group) if self.enabled else 1
        self.rank = dist.get_rank(group) if self.enabled else 0
        self.flat_g, self.group = flat_g, group
        self.buckets = [((k,) if isinstance(k, str) else tuple(k), s, e) for (k, s, e) in buckets]
        self._bucket_of = {k: i for i, (keys, _, _) in enumerate(self.buckets) for k in keys}
        self._waiting = [set(keys) for keys, _, _ in self.buckets]
        self.pending = []
        self.issued = []           # bucket indices in issue order of the current step (tests / traces)
        # bench.py --gpus N: set to a list to have finish() bracket its waits with two events on the current stream -- the time the
        # compute stream spends blocked on the collectives after the backward's last kernel = the EXPOSED communication of the step
        self.exposed_events = None

    def bucket_ready(self, key: str):
        """Call right after the kernels producing group `key` have been enqueued; the all-reduce of the bucket the group
        belongs to is issued (async) once all of its groups are ready."""
        if key not in self._bucket_of:
            raise KeyError(key)
        if not self.enabled:
            return
        i = self._bucket_of[key]
        self._waiting[i].discard(key)
        if not self._waiting[i]:
            _, s, e = self.buckets[i]
            self.issued.append(i)
            self.pending.append(self.dist.all_reduce(self.flat_g[s:e], op=self.dist.ReduceOp.SUM,
                                                     group=self.group, async_op=True))

    def finish(self) -> float:
        """Wait for every bucket; returns the factor the optimizer must apply (1/world)."""
        if self.enabled:
            for i, w in enumerate(self._waiting):      # a group nobody reported (model without that layer type): flush
                if w and i not in self.issued:
                    _, s, e = self.buckets[i]
                    self.issued.append(i)
                    self.pending.append(self.dist.all_reduce(self.flat_g[s:e], op=self.dist.ReduceOp.SUM,
                                                             group=self.group, async_op=True))
        ev = None
        if self.exposed_events is not None and self.pending:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        for w in self.pending:
            w.wait()
        if ev is not None:
            ev[1].record()
            self.exposed_events.append(ev)
        self.pending = []
        self.issued = []
        self._waiting = [set(keys) for keys, _, _ in self.buckets]
        return 1.0 / self.world


class BnSync:
    """SyncBN plumbing handed to the engine: in-place SUM all-reduce of a small fp32 row, ordered after the kernels already
    enqueued on the current stream (torch.distributed's synchronous collectives have exactly that stream semantics)."""

    def __init__(self, dist, group, world):
        self.dist, self.group, self.world = dist, group, int(world)
        self.calls = 0             # collectives issued so far (bench.py reports them per step)

    def all_reduce(self, t: torch.Tensor):
        self.calls += 1
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group)


def seed_all_ranks(seed: Optional[int] = None, group=None) -> Optional[int]:
    """Identical host RNG state (random, numpy, torch) on every data-parallel rank.  The dataset classes shuffle with the
    global RNGs like the reference's do (spectograms_dataset.py:53,176-185; waveform_dataset.py split/shuffle): ranks that
    draw different train/val splits or start-index permutations would train on each other's validation files and the
    rank-sharded index ranges would overlap.  With seed=None rank 0 draws one and broadcasts it.  Single process: seeds
    only if a seed is given."""
    import random
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dev = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
        t = torch.tensor([seed if seed is not None else random.getrandbits(31)], dtype=torch.int64, device=dev)
        dist.broadcast(t, src=0, group=group)
        seed = int(t.item())
    if seed is not None:
        random.seed(seed)
        np.random.seed(seed % (2 ** 32))
        torch.manual_seed(seed)
    return seed


def reseed_rank(seed: Optional[int], rank: int) -> None:
    """Rank-specific host RNG streams AFTER the rank-identical draws (train/val split, start-index permutation) are done:
    the datasets draw their augmentation decisions (mix-in partners, noise, gains) from the global numpy RNG in
    __getitem__ / device_batch, and with identical streams every rank would make the same draws at every step -- the
    augmentation diversity of the global batch would shrink by the world size against the reference's single process
    (spectograms_dataset.py:71-73,112-135).  Parameters are broadcast from rank 0 in FusedTrainer anyway."""
    import random
    if seed is None:
        return
    s = int(seed) + 1000003 * (int(rank) + 1)
    random.seed(s)
    np.random.seed(s % (2 ** 32))
    torch.manual_seed(s)


def sharded_batch_indices(n: int, batch_size: int, rank: int = 0, world_size: int = 1):
    """Index lists of one epoch for rank `rank`: idx = step*B_global + rank*B_local + i of the dataset's own order (SURVEY 8e;
    the reference builds its DataLoader without shuffle and without drop_last, main.py:125).  One process keeps the short tail
    batch like DataLoader does.  With world_size > 1 every rank must hold the same number of samples per step (the 1/world
    gradient average and SyncBN's `count * world` assume it), so the ragged tail of the LAST global batch is filled by wrapping
    to the start of the table -- the same rule on every rank; no sample is left out of an epoch and len() is
    ceil(n / B_global) at every world size (a few samples at the head are seen twice instead).
    TRAIN LOADERS ONLY: a metric / evaluation loop over a wrapped epoch would count the head samples twice -- the validation samplers
    of the datasets (get_validation_sampler) walk whole files on every rank and do not come through here; the waveform path's
    WaveformBatchLoader drops its ragged tail instead (multiples of 8 frames per rank)."""
    B, g = int(batch_size), int(batch_size) * int(world_size)
    if n <= 0:
        return
    if world_size == 1:
        for base in range(0, n, B):
            yield list(range(base, min(base + B, n)))
        return
    for base in range(0, n, g):
        lo = base + rank * B
        yield [(lo + i) % n for i in range(B)]


class ShardedBatchLoader:
    """DataLoader stand-in for map-style datasets under data parallel (sharded_batch_indices above)."""

    def __init__(self, dataset, batch_size: int, rank: int = 0, world_size: int = 1):
        self.dataset, self.batch_size, self.rank, self.world_size = dataset, int(batch_size), int(rank), int(world_size)

    def __len__(self):
        g = self.batch_size * self.world_size
        return (len(self.dataset) + g - 1) // g

    def indices(self):
        return sharded_batch_indices(len(self.dataset), self.batch_size, self.rank, self.world_size)

    def __iter__(self):
        for idx in self.indices():
            items = [self.dataset[i] for i in idx]
            yield tuple(torch.stack([torch.as_tensor(it[k]) for it in items]) for k in range(len(items[0])))


# ----------------------------------------------------------------------------------------------
# the fused optimizer + step
# ----------------------------------------------------------------------------------------------
def check_optimizer_options(weight_decay=0.0, decoupled_weight_decay=False, amsgrad=True, max_grad_norm=None):
    """Validate the optimizer options of FusedTrainer / FusedAdamAmsgrad (host only, before any device work).  Returns
    (weight_decay, decoupled, amsgrad, max_grad_norm or None, ext): `ext` is False when every option has the reference's value
    (Adam, amsgrad=True, no decay, no clipping) -- the trainer then launches exactly the reference step's kernels."""
    wd = float(weight_decay)
    if not (0.0 <= wd < float("inf")):
        raise ValueError(f"weight_decay must be finite and >= 0 (got {weight_decay!r})")
    mgn = None
    if max_grad_norm is not None:
        mgn = float(max_grad_norm)
        if not (0.0 < mgn < float("inf")):
            raise ValueError(f"max_grad_norm must be finite and > 0, or None for no clipping (got {max_grad_norm!r})")
    dec, ams = bool(decoupled_weight_decay), bool(amsgrad)
    return wd, dec, ams, mgn, (wd != 0.0 or not ams or mgn is not None)


# ---- learning-rate schedules and parameter groups (this build only; the kernels are csrc/sed_optim.hip) -------------------------
TILE4 = L.OPT_TILE4              # float4s per tile of the grouped step, SED_OPT_TILE4
MAX_GROUPS = L.OPT_MAX_GROUPS    # SED_OPT_MAX_GROUPS
SCHEDULE_KINDS = tuple(L.SCHED_KINDS)


def _is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


class LRSchedule:
    """Linear warm-up over the first `warmup` steps times a decay d(s) of the 1-based step s (lr_at is the definition):
        const    1
        step     gamma^floor((s - 1) / every)                          (the reference's rule in closed form: every=200, gamma=0.997)
        cosine   floor + (1 - floor) (1 + cos(pi u)) / 2,  u = clamp((s - warmup) / (total - warmup), 0, 1)
        linear   floor + (1 - floor) (1 - u)
        invsqrt  sqrt(max(warmup, 1) / max(s, warmup, 1))              (Noam's rule after the warm-up)
    Validated here, on the host, before anything else happens."""

    def __init__(self, kind: str, warmup: int = 0, total: int = 0, every: int = LR_DECAY_FREQ, gamma: float = LR_DECAY,
                 floor: float = 0.0):
        if kind not in SCHEDULE_KINDS:
            raise ValueError(f"lr schedule kind must be one of {', '.join(SCHEDULE_KINDS)} (got {kind!r})")
        for name, v in (("warmup", warmup), ("total", total), ("every", every)):
            if not _is_int(v) or not -2 ** 31 < v < 2 ** 31:
                raise ValueError(f"lr schedule: {name} is a number of steps, an integer (got {v!r})")
        if warmup < 0:
            raise ValueError(f"lr schedule: warmup must be >= 0 (got {warmup})")
        if kind in ("cosine", "linear") and total <= warmup:
            raise ValueError(f"lr schedule: {kind} needs total > warmup (got total={total}, warmup={warmup})")
        if kind == "step" and every < 1:
            raise ValueError(f"lr schedule: step needs every >= 1 (got {every})")
        g, f = float(gamma), float(floor)
        if not (0.0 < g < float("inf")):
            raise ValueError(f"lr schedule: gamma must be finite and > 0 (got {gamma!r})")
        if not (0.0 <= f <= 1.0):
            raise ValueError(f"lr schedule: floor must lie in [0, 1] (got {floor!r})")
        self.kind, self.warmup, self.total, self.every, self.gamma, self.floor = kind, int(warmup), int(total), int(every), g, f

    def as_dict(self) -> dict:
        return {"kind": self.kind, "warmup": self.warmup, "total": self.total, "every": self.every, "gamma": self.gamma,
                "floor": self.floor}

    def __repr__(self):
        return "LRSchedule(" + ", ".join(f"{k}={v!r}" for k, v in self.as_dict().items()) + ")"


def lr_at(base_lr: float, s: int, schedule: LRSchedule) -> float:
    """The learning rate of the 1-based step s in float64: base_lr * w(s) * d(s), w(s) = min(1, s / warmup) (1 without warm-up).
    The device evaluates the same expressions in double (adam_groups_hyper_kernel); this one is for logging and for the tests."""
    s = int(s)
    if s < 1:
        raise ValueError(f"steps are 1-based (got {s})")
    W, kind = schedule.warmup, schedule.kind
    w = min(1.0, s / W) if W > 0 else 1.0
    d = 1.0
    if kind == "step":
        d = schedule.gamma ** float((s - 1) // schedule.every)
    elif kind in ("cosine", "linear"):
        u = min(1.0, max(0.0, (s - W) / (schedule.total - W)))
        shape = 0.5 * (1.0 + math.cos(math.pi * u)) if kind == "cosine" else 1.0 - u
        d = schedule.floor + (1.0 - schedule.floor) * shape
    elif kind == "invsqrt":
        d = math.sqrt(max(W, 1) / max(s, W, 1))
    return float(base_lr) * w * d


def selector_matches(selector, name: str) -> bool:
    """A selector is a callable name -> bool, or a list of name prefixes matched at dot boundaries: 'conv_blocks.1' takes
    'conv_blocks.1.conv1.weight' and not 'conv_blocks.10.conv1.weight'."""
    if callable(selector):
        return bool(selector(name))
    for pre in selector:
        pre = pre.rstrip(".")
        if name == pre or name.startswith(pre + "."):
            return True
    return False


def resolve_param_groups(names, param_groups, weight_decay: float = 0.0):
    """param_groups -> (specs, assignment): specs[g] = (lr_scale, weight_decay, frozen) with g = 0 the unmatched remainder (scale 1,
    the trainer's decay) and g = i + 1 the i-th given group; assignment[k] = the group of names[k], the first match.  Host only:
    refuses a selector that matches nothing, a negative or non-finite scale or decay, more than 64 groups and everything frozen."""
    names = list(names)
    specs = [(1.0, float(np.float32(weight_decay)), False)]
    given = list(param_groups or [])
    if len(given) + 1 > MAX_GROUPS:
        raise ValueError(f"at most {MAX_GROUPS} parameter groups, the unmatched remainder included (got {len(given)} + 1)")
    for i, pg in enumerate(given):
        if not isinstance(pg, dict) or "params" not in pg:
            raise ValueError(f"param_groups[{i}] must be a dict with a 'params' selector")
        extra = set(pg) - {"params", "lr_scale", "weight_decay", "frozen"}
        if extra:
            raise ValueError(f"param_groups[{i}]: unknown keys {sorted(extra)} (params, lr_scale, weight_decay, frozen)")
        sel = pg["params"]
        if not callable(sel) and (isinstance(sel, str) or not all(isinstance(s, str) for s in sel)):
            raise ValueError(f"param_groups[{i}]: 'params' is a list of name prefixes or a callable name -> bool")
        scale = float(pg.get("lr_scale", 1.0))
        wd = pg.get("weight_decay")
        wd = float(weight_decay) if wd is None else float(wd)
        if not (0.0 <= scale < float("inf")):
            raise ValueError(f"param_groups[{i}]: lr_scale must be finite and >= 0 (got {pg.get('lr_scale')!r})")
        if not (0.0 <= wd < float("inf")):
            raise ValueError(f"param_groups[{i}]: weight_decay must be finite and >= 0 (got {pg.get('weight_decay')!r})")
        # (the group table is fp32, as a float argument of the C ABI is: the specs carry the values the device multiplies with)
        specs.append((float(np.float32(scale)), float(np.float32(wd)), bool(pg.get("frozen", False))))
    assignment, hit = [], [False] * len(given)
    for n in names:
        g = 0
        for i, pg in enumerate(given):
            if selector_matches(pg["params"], n):
                g, hit[i] = i + 1, True
                break
        assignment.append(g)
    # (a group whose every match was taken by an earlier group is as empty as one that matches nothing)
    for i, h in enumerate(hit):
        if not h:
            raise ValueError(f"param_groups[{i}]: the selector matches no parameter that an earlier group has not taken")
    if all(specs[g][2] for g in assignment):
        raise ValueError("every parameter is frozen: there is nothing to train")
    return specs, assignment


def no_decay_groups(model) -> list:
    """The usual AdamW split as a param_groups list: every parameter with ndim <= 1 -- biases, BatchNorm / LayerNorm weight and bias,
    PCEN's vectors -- gets weight_decay 0; the rest stays in the remainder with the trainer's weight_decay."""
    names = [n for n, p in model.named_parameters() if p.ndim <= 1]
    return [{"params": names, "weight_decay": 0.0}] if names else []


def check_tiles(tiles, groups, flat, assignment) -> None:
    """Validate a tile table against the layout (what sed_adam_groups_step cannot do on the host): int32 (NT, 4) rows
    {start4, count4, group, 0}, ascending, covering [0, numel / 4) exactly, 1 <= count4 <= TILE4, no tile across a parameter, every
    tile in its parameter's group; groups float32 (NG, 4), 1 <= NG <= MAX_GROUPS."""
    tiles, groups = np.asarray(tiles), np.asarray(groups)
    if tiles.dtype != np.int32 or tiles.ndim != 2 or tiles.shape[1] != 4 or tiles.shape[0] < 1:
        raise ValueError("tile table must be int32 (NT, 4) with NT >= 1")
    if groups.dtype != np.float32 or groups.ndim != 2 or groups.shape[1] != 4 or not 1 <= groups.shape[0] <= MAX_GROUPS:
        raise ValueError(f"group table must be float32 (NG, 4) with 1 <= NG <= {MAX_GROUPS}")
    if flat.numel % 4:
        raise ValueError("the flat buffer's length must be a multiple of 4")
    if len(assignment) != len(flat.names):
        raise ValueError("one group index per parameter")
    bounds = []                       # (first float4, one past the last, group) per parameter, in buffer order
    for n, g in zip(flat.names, assignment):
        o, k = flat.offsets[n], int(flat.P[n].numel())
        if o % 4:
            raise ValueError(f"parameter {n} does not start on a float4")
        if not 0 <= int(g) < groups.shape[0]:
            raise ValueError(f"parameter {n}: group {g} outside the group table")
        if k:
            bounds.append((o // 4, (o + k + 3) // 4, int(g), n))
    pos, bi = 0, 0
    for t, (s4, c4, g, z) in enumerate(tiles.tolist()):
        if s4 != pos:
            raise ValueError(f"tile {t}: starts at float4 {s4}, expected {pos} (tiles ascend and cover the buffer without gaps)")
        if not 1 <= c4 <= TILE4:
            raise ValueError(f"tile {t}: count4 {c4} outside 1..{TILE4}")
        if z != 0:
            raise ValueError(f"tile {t}: the fourth word must be 0")
        while bi < len(bounds) and bounds[bi][1] <= s4:
            bi += 1
        if bi == len(bounds) or s4 < bounds[bi][0] or s4 + c4 > bounds[bi][1]:
            raise ValueError(f"tile {t}: [{s4}, {s4 + c4}) crosses a parameter boundary")
        if g != bounds[bi][2]:
            raise ValueError(f"tile {t}: group {g}, but parameter {bounds[bi][3]} is in group {bounds[bi][2]}")
        pos = s4 + c4
    if pos != flat.numel // 4:
        raise ValueError(f"the tiles cover {pos} float4s of {flat.numel // 4}")


def build_tiles(flat, assignment, specs=None):
    """The two tables of the grouped step for a FlatParams layout, as numpy arrays: tiles int32 (NT, 4) = {start4, count4, group, 0}
    -- every parameter cut into runs of at most TILE4 float4s, its padding lanes included -- and groups float32 (NG, 4) =
    {lr_scale, weight_decay, frozen, 0}.  assignment: one group index per parameter in flat.names order; specs: (lr_scale,
    weight_decay, frozen) per group (None: max(assignment) + 1 groups of (1, 0, False)).  Checked with check_tiles before return."""
    assignment = [int(g) for g in assignment]
    if len(assignment) != len(flat.names):
        raise ValueError("one group index per parameter")
    if specs is None:
        specs = [(1.0, 0.0, False)] * (max(assignment) + 1)
    if not 1 <= len(specs) <= MAX_GROUPS:
        raise ValueError(f"1..{MAX_GROUPS} groups (got {len(specs)})")
    if min(assignment) < 0 or max(assignment) >= len(specs):
        raise ValueError("group index outside the group table")
    rows = []
    for n, g in zip(flat.names, assignment):
        s4, c4 = flat.offsets[n] // 4, (int(flat.P[n].numel()) + 3) // 4
        while c4 > 0:
            c = min(c4, TILE4)
            rows.append((s4, c, g, 0))
            s4, c4 = s4 + c, c4 - c
    tiles = np.asarray(rows, dtype=np.int32).reshape(-1, 4)
    groups = np.asarray([(float(s), float(w), 1.0 if f else 0.0, 0.0) for s, w, f in specs], dtype=np.float32).reshape(-1, 4)
    check_tiles(tiles, groups, flat, assignment)
    return tiles, groups


def grouped_param_groups(template: dict, specs, assignment, next_lr: float, base_lr: float) -> list:
    """state_dict()'s 'param_groups' on the grouped path, torch's multi-group layout: one dict per NON-EMPTY group in group order,
    `template`'s keys (betas, eps, amsgrad, ...) with 'params' = the indices in model.parameters() order, 'lr' = next_lr * lr_scale,
    'initial_lr' = base_lr * lr_scale, the group's 'weight_decay', and 'lr_scale' / 'frozen'."""
    out = []
    for gi, (scale, wd, frozen) in enumerate(specs):
        idx = [i for i, g in enumerate(assignment) if g == gi]
        if idx:
            out.append(dict(template, lr=next_lr * scale, initial_lr=base_lr * scale, weight_decay=wd if wd != 0.0 else 0,
                            lr_scale=scale, frozen=frozen, params=idx))
    return out


def state_index_map(state_groups, own_groups) -> dict:
    """{id in the state: index in model.parameters() order} for a multi-group optimizer state, matched by POSITION as
    torch.optim.Optimizer.load_state_dict does: the k-th parameter of the j-th group of the state is the k-th of the j-th own group.
    A torch optimizer numbers its parameters group after group, this trainer in model.parameters() order; both load.  Refuses
    another number of groups or of parameters in a group."""
    if [len(g["params"]) for g in state_groups] != [len(g["params"]) for g in own_groups]:
        raise ValueError("optimizer state does not have this trainer's parameter groups "
                         f"(sizes {[len(g['params']) for g in state_groups]}, expected {[len(g['params']) for g in own_groups]})")
    return {int(a): int(b) for sg, og in zip(state_groups, own_groups) for a, b in zip(sg["params"], og["params"])}


def check_group_options(model, lr, lr_schedule=None, param_groups=None, weight_decay=0.0):
    """Validate lr_schedule / param_groups of FusedTrainer / train() (host only, before the model is touched).  Returns None when
    both are None -- the step then launches exactly what it always did -- else (schedule, specs, assignment); without a schedule
    the groups run the reference's decay as LRSchedule('step', every=200, gamma=0.997)."""
    if lr_schedule is None and param_groups is None:
        return None
    if lr_schedule is not None and not isinstance(lr_schedule, LRSchedule):
        raise TypeError(f"lr_schedule must be an LRSchedule or None (got {type(lr_schedule).__name__})")
    if not math.isfinite(float(lr)):
        raise ValueError(f"lr must be finite (got {lr!r})")
    specs, assignment = resolve_param_groups([n for n, _ in model.named_parameters()], param_groups, weight_decay)
    eng = getattr(model, "engine", None)
    if eng is not None and not hasattr(eng, "adam_groups_step"):
        raise RuntimeError(f"lr_schedule / param_groups need an engine with the grouped optimizer step ({type(model).__name__} has "
                           "none)")
    return lr_schedule if lr_schedule is not None else LRSchedule("step"), specs, assignment


def check_weak_options(weak_pooling=None, weak_weight=1.0, weak_only=False, model=None):
    """Validate the weak-label options of FusedTrainer / train() (host only, before any device work).  Returns None when
    weak_pooling is None -- the step then launches exactly what it always did -- else the (mode, weight, only) triple of
    CnnEngine.loss_and_grad."""
    if weak_pooling is None:
        if weak_only:
            raise ValueError("weak_only needs a weak_pooling (max, mean, linear or exp)")
        return None
    from .engine import check_clip_pooling
    check_clip_pooling(weak_pooling, model)           # 'att': the attention pooling, on a model with the attention head
    w = float(weak_weight)
    if not (0.0 < w < float("inf")):
        raise ValueError(f"weak_weight must be finite and > 0 (got {weak_weight!r})")
    if model is not None and not hasattr(model, "conv_blocks"):
        raise ValueError(f"the weak-label loss pools frame probabilities over time: {type(model).__name__} has no time axis in "
                         "its output (use Cnn_AvgPooling / Crnn_AvgPooling)")
    return weak_pooling, w, bool(weak_only)


def check_semi_options(mean_teacher=False, ema_decay=0.999, consistency_weight=2.0, consistency_rampup=0, model=None):
    """Validate the mean-teacher options of FusedTrainer / train() (host only, before any device work).  Returns None when
    mean_teacher is off -- the step then launches exactly what it always did -- else (ema_decay, consistency_weight,
    consistency_rampup)."""
    if not mean_teacher:
        return None
    d, w = float(ema_decay), float(consistency_weight)
    if not (0.0 <= d < 1.0):
        raise ValueError(f"ema_decay must lie in [0, 1) (got {ema_decay!r})")
    if not (0.0 <= w < float("inf")):
        raise ValueError(f"consistency_weight must be finite and >= 0 (got {consistency_weight!r})")
    if isinstance(consistency_rampup, bool) or int(consistency_rampup) != consistency_rampup or consistency_rampup < 0:
        raise ValueError(f"consistency_rampup is a number of steps, an integer >= 0 (got {consistency_rampup!r})")
    if model is not None:
        if not hasattr(model, "conv_blocks"):
            raise ValueError(f"the mean teacher compares frame probabilities over time: {type(model).__name__} has no time axis in "
                             "its output (use Cnn_AvgPooling / Crnn_AvgPooling)")
        if getattr(getattr(model, "engine", None), "head", "fc") == "none":
            raise ValueError("the mean teacher needs a model with a classification head")
    return d, w, int(consistency_rampup)


def check_frontend_options(model, graph=False, group=None, mean_teacher=False):
    """Refuse what a model with a front-end layer (Cnn_AvgPooling(frontend=PCEN(...))) does not train under: a captured graph, a
    process group and the mean teacher.  Returns the layer, or None for a model without one -- the step then launches exactly
    what it always did."""
    fe = getattr(model, "frontend", None)
    if fe is None:
        return None
    if graph:
        raise RuntimeError("graph=True does not capture a front-end layer (PCEN): build the trainer with graph=False")
    if data_parallel_enabled(group):
        raise RuntimeError("a front-end layer (PCEN) trains in a single process: its backward takes the input gradient, which "
                           "the data-parallel path (and SyncBN) does not provide")
    if mean_teacher:
        raise RuntimeError("mean_teacher does not take a model with a front-end layer (PCEN) yet")
    return fe


def ema_factor(n: int, ema_decay: float) -> float:
    """The teacher's EMA factor after the n-th step (n = 1, 2, ...): min(1 - 1/n, ema_decay), so the first update copies the
    student and the early teacher is the plain average of the students so far."""
    return min(1.0 - 1.0 / n, float(ema_decay))


def consistency_weight_at(n: int, weight: float, rampup: int) -> float:
    """The consistency weight at step n (n = 1, 2, ...): weight * exp(-5 (1 - min(n, R)/R)^2) for R = rampup > 0 (the sigmoid
    ramp-up of Tarvainen and Valpola 2017), constant for R = 0."""
    if rampup <= 0:
        return float(weight)
    return float(weight) * math.exp(-5.0 * (1.0 - min(n, rampup) / rampup) ** 2)


def check_state_amsgrad(group, amsgrad: bool):
    """Refuse an optimizer state whose amsgrad flag is not the trainer's: the max_exp_avg_sq buffers exist on one side only."""
    got = bool(group.get("amsgrad", False))
    if amsgrad and not got:
        raise ValueError("the fused optimizer is Adam with amsgrad=True (train.py:85)")
    if got and not amsgrad:
        raise ValueError("optimizer state has amsgrad=True but this trainer was built with amsgrad=False: "
                         "build it with amsgrad=True to resume from this state")


# The mean teacher's dropout seed is the student's XOR this constant (the 64-bit golden-ratio constant): its training-mode forward
# draws masks of its own.  With a process group, rank r uses seed + r.
TEACHER_DROPOUT_SEED_XOR = 0x9E3779B97F4A7C15


def _dropout_engine(model):
    """the model's engine when it drops (Csa_AvgPooling with sa_dropout > 0), else None"""
    eng = getattr(model, "engine", None)
    return eng if eng is not None and getattr(eng, "sa_dropout", 0.0) > 0.0 else None


class FusedTrainer:
    """Owns the flat buffers, the Adam state and the step counter for one model."""

    def __init__(self, model, lr: float, recall_factor: float = 5.0, betas=(0.9, 0.999), eps: float = 1e-8,
                 group=None, graph: bool = False, sync_bn: bool = False, n_buckets: Optional[int] = None,
                 weight_decay: float = 0.0, decoupled_weight_decay: bool = False, amsgrad: bool = True,
                 max_grad_norm: Optional[float] = None, weak_pooling: Optional[str] = None, weak_weight: float = 1.0,
                 weak_only: bool = False, mean_teacher: bool = False, ema_decay: float = 0.999, consistency_weight: float = 2.0,
                 consistency_rampup: int = 0, teacher_augment=None, lr_schedule: Optional["LRSchedule"] = None,
                 param_groups: Optional[list] = None):
        """graph=True (single process): after two eager steps per input shape the whole step -- forward, loss, backward,
        Adam-amsgrad with its step counter, learning rate and bias corrections in device memory -- is captured into a HIP
        graph and replayed.  For the reference's own small shapes (T = 30 crops, batch 4: ~90 launches of a few microseconds
        each) the eager step is bound by launch overhead, not by the GPU.

        weight_decay / decoupled_weight_decay / amsgrad: torch.optim.Adam(weight_decay=, amsgrad=) or, decoupled,
        torch.optim.AdamW.  max_grad_norm: torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm) between backward and the
        step, computed on the device from the averaged gradient -- every rank reduces the same all-reduced buffer with
        grad_scale = 1/world in the same fixed order, so all ranks get the same factor without another collective.  A
        non-finite norm propagates as in torch (the step is not skipped).  With all four at their defaults the step launches
        what it always did; any option switches to sed_grad_norm / sed_adam_step_ex.

        weak_pooling: None, or max / mean / linear / exp -- train from clip-level labels (csrc/sed_weak.hip) -- or att on a model
        built with attention=True (the learned attention pooling, csrc/sed_attn.hip; it also trains att_fc): the frame
        probabilities are pooled over time and WeightedBCE is taken against the clip label, times weak_weight.  weak_only=False
        adds it to the strong loss, with the clip label taken from the (B, T, K) target on the device; weak_only=True trains on it
        alone, and the target may be (B, K).  None launches nothing new.

        A model built with frontend=PCEN(...) brings its layer: the step runs the layer's forward, the engine's forward with
        keep_for_grad, the losses, the engine's backward with need_dx, then sed_pcen_bwd on the input gradient into
        flat.G['frontend.*'] (a fixed layer, trainable=False: its forward only).  The layer's parameters sit in the flat buffer like
        the others.  Refused with graph=True, a process group or mean_teacher.

        mean_teacher: keep self.teacher, a copy of the model whose parameters are an exponential moving average of the
        student's (csrc/sed_semi.hip), with its own engine, plans and flat parameter buffer.  Every step the teacher runs a
        training-mode forward on teacher_augment(x) (a callable, None: x itself) and the student is pulled towards its frame
        probabilities and, with a weak_pooling, its pooled clip probabilities: MSE terms over all clips times
        consistency_weight, ramped up over the first consistency_rampup steps (consistency_weight_at).  After the optimizer step
        teacher <- a_n teacher + (1 - a_n) student, a_n = ema_factor(n, ema_decay).  self.last_consistency is a device (2,)
        tensor, the frame and clip terms of the last step.  Single process, eager steps only.

        lr_schedule: None, or an LRSchedule -- linear warm-up, then const / step / cosine / linear / invsqrt decay.  param_groups:
        None, or a list of {"params": selector, "lr_scale": 1.0, "weight_decay": None, "frozen": False}; a selector is a list of
        name prefixes matched against named_parameters() at dot boundaries, or a callable name -> bool; the first match wins, the
        unmatched parameters form group 0 (scale 1, the trainer's weight_decay), weight_decay None inherits the trainer's
        (no_decay_groups(model) is the usual AdamW split).  A frozen group's parameters and optimizer state keep their bits and its
        gradients are left out of the clipping norm, as torch does for a parameter without a gradient; its backward still runs, and
        the BatchNorm running statistics of a frozen block still follow the training-mode forwards, as in torch (model.eval() with
        the eval-mode backward pins them).  With both None the trainer does what it always did.  With either given, eager and
        graph=True steps alike run sed_grad_norm_groups (if clipping) and sed_adam_groups_step: the step counter, the schedule's
        learning rate and every group's scalars live in device memory and the host keeps no second copy of the schedule.
        param_groups without a schedule run the reference's decay as LRSchedule("step", every=200, gamma=0.997): the closed form
        lr * 0.997^floor((s - 1) / 200) in float64, NOT claimed bit-equal to the legacy path's fp32 recurrence lr *= 0.997.
        trainer.lr is then lr_at(base_lr, step_count + 1, schedule), the next step's rate as before, and trainer.last_lr the device
        view of the rate the last step used.  Works under a process group (every rank applies the same elementwise step to the same
        all-reduced buffer; only world size 1 is exercised), with label kinds, weak pooling, the mean teacher (the EMA runs over the
        whole buffer), a PCEN front-end, the M5 engine and all four precisions.  FusedAdamAmsgrad does not take these options."""
        self._grouped = check_group_options(model, lr, lr_schedule, param_groups, weight_decay)
        self.semi = check_semi_options(mean_teacher, ema_decay, consistency_weight, consistency_rampup, model)
        # every refusal comes before the teacher is made and before the model's parameters move into the flat buffer: a refused
        # constructor leaves the model as it found it
        if graph and self.semi is not None:
            raise RuntimeError("graph=True does not capture the mean teacher (its weights change on the host's schedule)")
        if self.semi is not None and data_parallel_enabled(group):
            raise RuntimeError("mean_teacher is the single-process path (the teacher's BatchNorm statistics and the order of "
                               "the EMA across ranks are not defined yet)")
        self.teacher = self.teacher_flat = self.last_consistency = None
        self.teacher_augment = teacher_augment
        (self.weight_decay, self.decoupled_weight_decay, self.amsgrad, self.max_grad_norm,
         self._opt_ext) = check_optimizer_options(weight_decay, decoupled_weight_decay, amsgrad, max_grad_norm)
        self.weak = check_weak_options(weak_pooling, weak_weight, weak_only, model)
        self.frontend = check_frontend_options(model, graph, group, self.semi is not None)
        self.model = model
        self.engine = model.engine
        self.use_graph = bool(graph)
        self._graphs = {}           # input-shape key -> (graph, static x, static y, loss buffer)
        self._eager_seen = {}
        if not next(model.parameters()).is_cuda:
            raise RuntimeError("FusedTrainer needs the model on the GPU (model.to('cuda')); there is no CPU path")
        if self.semi is not None:           # before the student's parameters become views of its flat buffer
            self.teacher = model.clone_without_engines()
            for p in self.teacher.parameters():
                p.requires_grad_(False)
        self.flat = FlatParams(model, n_buckets)
        self.m = torch.zeros_like(self.flat.p)
        self.v = torch.zeros_like(self.flat.p)
        self.vmax = torch.zeros_like(self.flat.p) if self.amsgrad else None
        self._lr = self.base_lr = float(lr)
        self.lr_schedule = self.group_specs = self.group_of = self.last_lr = None
        self.betas, self.eps = betas, eps
        self.recall_factor = float(recall_factor)
        # clipping workspace, allocated once: fp64 partial sums, out = [norm, clip factor]; last_grad_norm is a view of out
        self._gn_partial = self._gn_out = self._coef = self.last_grad_norm = None
        if self._grouped is not None:
            # the grouped step: tile and group tables, the per-group scalars, the schedule's three floats and the step counter,
            # all in device memory for eager and captured steps alike
            dev = self.flat.p.device
            self.lr_schedule, self.group_specs, self.group_of = self._grouped
            tiles, groups = build_tiles(self.flat, self.group_of, self.group_specs)
            self._tiles, self._groups = torch.from_numpy(tiles).to(dev), torch.from_numpy(groups).to(dev)
            self._gh = torch.zeros(len(self.group_specs), 4, dtype=torch.float32, device=dev)
            self.hyper = torch.zeros(4, dtype=torch.float32, device=dev)
            self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
            self.last_lr = self.hyper[0:1]              # device (1,), the learning rate the last step used; no sync
        if self.max_grad_norm is not None:
            dev = self.flat.p.device
            nparts = L.lib().sed_grad_norm_nparts(self.flat.numel) if self._grouped is None else self._tiles.shape[0]
            self._gn_partial = torch.zeros(nparts, dtype=torch.float64, device=dev)
            self._gn_out = torch.tensor([0.0, 1.0], dtype=torch.float32, device=dev)
            self._coef = self._gn_out[1:2]
            self.last_grad_norm = self._gn_out[0:1]     # device (1,), norm of the last step's averaged gradient; no sync
        self.step_count = 0
        self.reducer = GradAllReducer(self.flat.g, self.flat.buckets, group)
        if self.teacher is not None:
            self.teacher_flat = FlatParams(self.teacher, grads=False)
        deng = _dropout_engine(model)
        if deng is not None:
            seed = deng.sa_dropout_seed
            if self.reducer.enabled:        # every rank its own masks
                seed = (seed + self.reducer.rank) & 0xFFFFFFFFFFFFFFFF
                deng.set_drop_state([seed & 0xFFFFFFFF, seed >> 32] + deng.drop_state_words()[2:])
            if self.teacher is not None:
                ts = seed ^ TEACHER_DROPOUT_SEED_XOR
                self.teacher.engine.set_drop_state([ts & 0xFFFFFFFF, ts >> 32, 0, 0])
        self.sync_bn = bool(sync_bn) and self.reducer.enabled
        if self.reducer.enabled:
            # replicas start from rank 0's parameters and BatchNorm buffers (the DDP constructor's broadcast): identical
            # seeds are not something to rely on
            self.reducer.dist.broadcast(self.flat.p, src=0, group=group)
            for _, b in model.named_buffers():
                if b.is_floating_point():
                    self.reducer.dist.broadcast(b, src=0, group=group)
        if self.sync_bn:
            if not hasattr(self.engine, "bn_sync"):
                raise RuntimeError("sync_bn is implemented for the spectrogram models (Cnn_AvgPooling / Crnn_AvgPooling)")
            self.engine.bn_sync = BnSync(self.reducer.dist, group, self.reducer.world)
        if self.use_graph:
            if self.reducer.enabled:
                raise RuntimeError("graph=True is the single-process path (the gradient collectives are not captured)")
            if not hasattr(self.engine, "adam_step_dev"):
                raise RuntimeError("graph=True needs an engine with a device-scalar optimizer step (Cnn_AvgPooling / Crnn_AvgPooling)")
            if self._grouped is None:
                dev = self.flat.p.device
                # (the extended device step keeps this step's learning rate in a fourth slot, sed_hip.h)
                self.hyper = torch.tensor([self.lr, 0.0, 0.0] + ([self.lr] if self._opt_ext else []), dtype=torch.float32, device=dev)
                self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)

    @property
    def lr(self) -> float:
        """The learning rate of the NEXT step: the host's scalar on the default path, lr_at(base_lr, step_count + 1, schedule) --
        float64, for logging -- with lr_schedule / param_groups (the device computes its own from the step counter)."""
        if self._grouped is None:
            return self._lr
        return lr_at(self.base_lr, self.step_count + 1, self.lr_schedule)

    @lr.setter
    def lr(self, value: float):
        if self._grouped is not None:
            raise AttributeError("with lr_schedule / param_groups the learning rate follows the schedule from base_lr")
        self._lr = float(value)

    def _groups_step(self, scale: float):
        """the grouped path's optimizer launches, eager or captured: [norm over the non-frozen tiles,] hyper kernel + update"""
        if self.max_grad_norm is not None:
            self.engine.grad_norm_groups(self.flat.g, self._tiles, self._groups, self._gn_partial, self._gn_out, scale,
                                         self.max_grad_norm)
        self.engine.adam_groups_step(self.flat.p, self.flat.g, self.m, self.v, self.vmax, self._tiles, self._groups, self._gh,
                                     self.hyper, self.step_dev, self.base_lr, self.lr_schedule, grad_scale=scale, betas=self.betas,
                                     eps=self.eps, decoupled=self.decoupled_weight_decay, coef=self._coef)

    def _check_alias(self):
        if not self.flat.aliased():
            raise RuntimeError("model parameters were re-allocated after FusedTrainer was built "
                               "(e.g. model.to()); build the trainer after moving the model")

    def forward_backward(self, x: torch.Tensor, y: torch.Tensor, kind: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One forward + loss + backward; gradients land in flat.g; returns the device loss (1,).
        kind: None, or an integer (B,) device tensor of label kinds -- 0 strong, 1 weak, 2 unlabelled (CnnEngine.loss_and_grad)."""
        self._check_alias()
        eng = self.engine
        if kind is not None:
            if self.use_graph:
                raise RuntimeError("graph=True does not take label kinds (the selections are made by torch comparisons per step)")
            if not hasattr(self.model, "conv_blocks"):
                raise ValueError(f"label kinds select clips of frame-wise targets: {type(self.model).__name__} has none")
        teacher_pre = teacher_att = None
        if self.teacher is not None:        # first: the teacher's forward, in training mode like the student's
            if not self.teacher_flat.aliased():
                raise RuntimeError("the teacher's parameters were re-allocated after FusedTrainer was built")
            self.teacher.train()
            xt = x if self.teacher_augment is None else self.teacher_augment(x)
            tplan = self.teacher.engine.forward(xt, self.teacher_flat.tensor_dict(), training=True)
            teacher_pre, teacher_att = tplan.pre, tplan.att
            self.teacher._nbt_pending += 1
            self.teacher._fwd_serial += 1
        P = self.flat.tensor_dict()
        self.model.train()
        fe = self.frontend
        fe_train = fe is not None and fe.trainable
        if fe is None:
            plan = eng.forward(x, P, training=True)
        else:
            eng._tag = ""
            x_raw = x.float() if x.dim() == 4 else x.float().unsqueeze(1)
            fe_theta = fe.theta()
            x = fe.run_forward(x_raw, fe_theta, launch=eng._k)
            plan = eng.forward(x, P, training=True, keep_for_grad=True) if fe_train else eng.forward(x, P, training=True)
        self.model._nbt_pending += 1
        self.model._fwd_serial += 1
        if kind is not None or teacher_pre is not None:
            cw = None if self.semi is None else consistency_weight_at(self.step_count + 1, self.semi[1], self.semi[2])
            loss = eng.loss_and_grad(plan, y, self.recall_factor, weak=self.weak, kind=kind, teacher_pre=teacher_pre, consistency=cw,
                                     teacher_att=teacher_att)
            if teacher_pre is not None:
                self.last_consistency = plan.consistency
        elif self.weak is None:
            loss = eng.loss_and_grad(plan, y, self.recall_factor)
        else:
            loss = eng.loss_and_grad(plan, y, self.recall_factor, weak=self.weak)
        if not fe_train:
            eng.backward(plan, P, self.flat.G, on_group_done=self.reducer.bucket_ready)
            return loss
        eng.backward(plan, P, self.flat.G, on_group_done=self.reducer.bucket_ready, need_dx=True)
        eng._tag = ""
        _, dtheta = fe.run_backward(x_raw, fe_theta, plan.dx_in, need_dx=False, need_dtheta=True, launch=eng._k)
        from .models.frontend_layers import PARAM_NAMES
        for i, n in enumerate(PARAM_NAMES):
            self.flat.G["frontend." + n].copy_(dtheta[i])
        self.reducer.bucket_ready("frontend")        # the last group in backward-completion order
        return loss

    def optimizer_step(self):
        scale = self.reducer.finish()
        self.step_count += 1
        if self._grouped is not None:
            self._groups_step(scale)
        elif not self._opt_ext:
            self.engine.adam_step(self.flat.p, self.flat.g, self.m, self.v, self.vmax, self.lr, self.step_count,
                                  grad_scale=scale, betas=self.betas, eps=self.eps)
        else:
            # after finish(): the norm is taken over the all-reduced buffer, the same bits on every rank
            if self.max_grad_norm is not None:
                self.engine.grad_norm(self.flat.g, self._gn_partial, self._gn_out, scale, self.max_grad_norm)
            self.engine.adam_step_ex(self.flat.p, self.flat.g, self.m, self.v, self.vmax, self.lr, self.step_count,
                                     grad_scale=scale, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay,
                                     decoupled=self.decoupled_weight_decay, coef=self._coef)
        if self.teacher is not None:
            self.engine._k("sed_ema_update", self.engine.lib.sed_ema_update, L.ptr(self.teacher_flat.p), L.ptr(self.flat.p),
                           self.flat.numel, ema_factor(self.step_count, self.semi[0]), torch.cuda.current_stream().cuda_stream)
        if self._grouped is None and self.step_count % LR_DECAY_FREQ == 0:       # train.py:108-110 (after that iteration's step)
            self.lr *= LR_DECAY

    def _step_dev(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """forward + loss + backward + optimizer step with device-resident scalars: kernel launches only (capturable)."""
        loss = self.forward_backward(x, y)
        if self._grouped is not None:
            self._groups_step(1.0)
            return loss
        if not self._opt_ext:
            self.engine.adam_step_dev(self.flat.p, self.flat.g, self.m, self.v, self.vmax, self.hyper, self.step_dev, 1.0,
                                      LR_DECAY, LR_DECAY_FREQ, betas=self.betas, eps=self.eps)
            return loss
        if self.max_grad_norm is not None:
            self.engine.grad_norm(self.flat.g, self._gn_partial, self._gn_out, 1.0, self.max_grad_norm)
        self.engine.adam_step_ex_dev(self.flat.p, self.flat.g, self.m, self.v, self.vmax, self.hyper, self.step_dev, 1.0,
                                     LR_DECAY, LR_DECAY_FREQ, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay,
                                     decoupled=self.decoupled_weight_decay, coef=self._coef)
        return loss

    def _host_mirror(self):
        self.step_count += 1
        if self._grouped is None and self.step_count % LR_DECAY_FREQ == 0:
            self.lr *= LR_DECAY

    def train_step(self, x: torch.Tensor, y: torch.Tensor, kind: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Returns the device loss buffer (1,) of this shape's plan: valid until the next step (clone to keep)."""
        if not self.use_graph:
            loss = self.forward_backward(x, y) if kind is None else self.forward_backward(x, y, kind)
            self.optimizer_step()
            return loss
        if kind is not None:
            raise RuntimeError("graph=True does not take label kinds (the selections are made by torch comparisons per step)")
        key = (tuple(x.shape), tuple(y.shape))
        ent = self._graphs.get(key)
        if ent is None:
            seen = self._eager_seen.get(key, 0)
            if seen < 2:            # eager: allocates the plan, the descriptor tables, sets kernel attributes
                self._eager_seen[key] = seen + 1
                loss = self._step_dev(x, y)
                self._host_mirror()
                return loss
            xs, ys = torch.empty_like(x), torch.empty_like(y)
            xs.copy_(x); ys.copy_(y)
            nbt, ser = self.model._nbt_pending, self.model._fwd_serial
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                loss = self._step_dev(xs, ys)
            self.model._nbt_pending, self.model._fwd_serial = nbt, ser     # (capture does not execute the step)
            ent = self._graphs[key] = (g, xs, ys, loss)
        else:
            ent[1].copy_(x); ent[2].copy_(y)
        self._check_alias()
        self.model.train()
        self.model._nbt_pending += 1
        self.model._fwd_serial += 1
        ent[0].replay()
        self._host_mirror()
        return ent[3]

    def _sync_host_scalars(self):
        """graph mode keeps the authoritative step counter / learning rate on the device; the grouped path keeps the counter there
        in every mode, and the learning rate is a function of it: only the counter is read."""
        if self._grouped is not None:
            self.step_count = int(self.step_dev.item())
        elif self.use_graph and self._graphs:
            self.step_count = int(self.step_dev.item())
            self.lr = float(self.hyper[0].item())

    def state_dict(self):
        """torch.optim.Adam(amsgrad=True).state_dict() layout (what the reference saves under checkpoint['optimizer'],
        train.py:123-126): {'state': {i: {'step', 'exp_avg', 'exp_avg_sq', 'max_exp_avg_sq'}}, 'param_groups': [...]}, the
        parameters numbered in model.parameters() order -- loadable into torch.optim.Adam and back into this trainer.
        The param group carries the trainer's weight_decay / amsgrad / decoupled_weight_decay (load a decoupled one into
        torch.optim.AdamW); without amsgrad there is no 'max_exp_avg_sq'.  max_grad_norm is not optimizer state.

        With lr_schedule / param_groups the layout is torch's multi-group one: one entry per non-empty group in group order (the
        unmatched remainder first), 'params' the indices in model.parameters() order, 'lr' that group's rate for the next step,
        'initial_lr' = base_lr * lr_scale, its 'weight_decay', plus 'lr_scale' and 'frozen'; no 'state' entries for frozen
        parameters; a top-level 'lr_schedule' dict.  It loads into torch.optim.Adam / AdamW built with the same groups."""
        self._sync_host_scalars()
        state = {}
        for i, n in enumerate(self.flat.names):
            if self._grouped is not None and self.group_specs[self.group_of[i]][2]:
                continue                    # frozen: torch keeps no state for a parameter that never had a gradient
            o, shp = self.flat.offsets[n], self.flat.P[n].shape
            k = self.flat.P[n].numel()
            state[i] = {"step": torch.tensor(float(self.step_count)),
                        "exp_avg": self.m[o:o + k].view(shp).clone(),
                        "exp_avg_sq": self.v[o:o + k].view(shp).clone()}
            if self.amsgrad:
                state[i]["max_exp_avg_sq"] = self.vmax[o:o + k].view(shp).clone()
        group = {"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps,
                 "weight_decay": self.weight_decay if self.weight_decay != 0.0 else 0, "amsgrad": self.amsgrad,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "decoupled_weight_decay": self.decoupled_weight_decay, "params": list(range(len(self.flat.names)))}
        sd = {"state": state, "param_groups": [group]}
        if self._grouped is not None:
            sd["param_groups"] = grouped_param_groups(group, self.group_specs, self.group_of, self.lr, self.base_lr)
            sd["lr_schedule"] = dict(self.lr_schedule.as_dict(), base_lr=self.base_lr)
        if self.teacher is not None:        # the mean teacher's parameters and BatchNorm buffers
            sd["teacher"] = {k: v.clone() for k, v in self.teacher.state_dict().items()}
        deng = _dropout_engine(self.model)
        if deng is not None:                # the four uint32 words (seed_lo, seed_hi, step, 0) the next training forward draws from
            sd["dropout_state"] = torch.tensor(deng.drop_state_words(), dtype=torch.int64)
            if self.teacher is not None:
                sd["teacher_dropout_state"] = torch.tensor(self.teacher.engine.drop_state_words(), dtype=torch.int64)
        return sd

    def load_state_dict(self, sd, teacher=None):
        """Resume from state_dict() output or from a torch.optim.Adam / AdamW state_dict of the same model whose amsgrad flag
        is this trainer's.  lr, betas and eps come from the state; weight decay, its kind and max_grad_norm stay as the
        trainer was built.  The mean teacher is restored from `teacher` (a checkpoint of train() keeps it beside the optimizer
        state: trainer.load_state_dict(ck['optimizer'], teacher=ck.get('teacher'))), else from sd['teacher'], else -- a state
        from before the teacher -- it starts as a copy of the student as the model is now.

        With lr_schedule / param_groups the state must have this trainer's group structure (as many groups, as many parameters in
        each: its own state_dict() or that of a torch optimizer built with the same groups, matched by position as torch does,
        state_index_map); the base learning rate, the scales, the decays and the SCHEDULE are the trainer's, not the state's
        (sd['lr_schedule'] and the groups' 'lr' are not read): only betas, eps, the moments and the step counter are restored, the
        counter on the device too."""
        groups = sd["param_groups"]
        grouped = getattr(self, "_grouped", None) is not None
        if grouped:
            ids = state_index_map(groups, grouped_param_groups({}, self.group_specs, self.group_of, 0.0, 0.0))
            sd = dict(sd, state={ids[k]: st for k, st in sd["state"].items()})
        elif len(groups) != 1 or len(groups[0]["params"]) != len(self.flat.names):
            raise ValueError("optimizer state does not match this model's parameter list")
        for g in groups:
            check_state_amsgrad(g, self.amsgrad)
        if not grouped:
            self.lr = float(groups[0]["lr"])
        self.betas, self.eps = tuple(groups[0]["betas"]), float(groups[0]["eps"])
        step = 0
        for i, n in enumerate(self.flat.names):
            o, k = self.flat.offsets[n], self.flat.P[n].numel()
            st = sd["state"].get(i)
            if st is None:
                self.m[o:o + k].zero_(); self.v[o:o + k].zero_()
                if self.amsgrad:
                    self.vmax[o:o + k].zero_()
                continue
            self.m[o:o + k].copy_(st["exp_avg"].reshape(-1))
            self.v[o:o + k].copy_(st["exp_avg_sq"].reshape(-1))
            if self.amsgrad:
                self.vmax[o:o + k].copy_(st["max_exp_avg_sq"].reshape(-1))
            step = max(step, int(float(st["step"])))
        self.step_count = step
        if self.teacher is not None:
            if teacher is not None or "teacher" in sd:
                self.teacher.load_state_dict(teacher if teacher is not None else sd["teacher"])
            else:                           # a checkpoint from before the teacher: it starts as a copy of the student
                self.teacher.load_state_dict(self.model.state_dict())
        deng = _dropout_engine(self.model)
        if deng is not None:                # a state without it starts at step 0 with the seed the engine has
            for eng, key in ((deng, "dropout_state"), (self.teacher.engine if self.teacher is not None else None, "teacher_dropout_state")):
                if eng is None:
                    continue
                words = [int(v) for v in sd[key].tolist()] if key in sd else eng.drop_state_words()[:2] + [0, 0]
                eng.set_drop_state(words)
        if grouped:
            self.step_dev.fill_(step)
        elif self.use_graph:
            self.hyper[0] = self.lr
            self.step_dev.fill_(step)


class FusedAdamAmsgrad:
    """torch.optim-like facade over the fused kernel for code that calls loss.backward() itself
    (gradients in p.grad): zero_grad() / step().  The four optimizer options are FusedTrainer's; lr_schedule / param_groups are
    not offered here (set param_groups[0]["lr"] between steps for a schedule)."""

    def __init__(self, model, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 decoupled_weight_decay: bool = False, amsgrad: bool = True, max_grad_norm: Optional[float] = None):
        (self.weight_decay, self.decoupled_weight_decay, self.amsgrad, self.max_grad_norm,
         self._opt_ext) = check_optimizer_options(weight_decay, decoupled_weight_decay, amsgrad, max_grad_norm)
        self.flat = FlatParams(model)
        self.model = model
        self.m = torch.zeros_like(self.flat.p)
        self.v = torch.zeros_like(self.flat.p)
        self.vmax = torch.zeros_like(self.flat.p) if self.amsgrad else None
        self.param_groups = [{"lr": float(lr)}]
        self.betas, self.eps, self.step_count = betas, eps, 0
        self._gn_partial = self._gn_out = self._coef = self.last_grad_norm = None
        if self.max_grad_norm is not None:
            dev = self.flat.p.device
            self._gn_partial = torch.zeros(L.lib().sed_grad_norm_nparts(self.flat.numel), dtype=torch.float64, device=dev)
            self._gn_out = torch.tensor([0.0, 1.0], dtype=torch.float32, device=dev)
            self._coef, self.last_grad_norm = self._gn_out[1:2], self._gn_out[0:1]

    def zero_grad(self):
        for p in self.model.parameters():
            p.grad = None

    def step(self):
        self.flat.g.zero_()
        for n, p in self.model.named_parameters():
            if p.grad is not None:
                self.flat.G[n].copy_(p.grad)
        self.step_count += 1
        if self._opt_ext:
            st = torch.cuda.current_stream().cuda_stream
            if self.max_grad_norm is not None:
                L.check(L.lib().sed_grad_norm(L.ptr(self.flat.g), self.flat.numel, 1.0, self.max_grad_norm,
                                              L.ptr(self._gn_partial), self._gn_partial.numel(), L.ptr(self._gn_out), st),
                        "grad_norm")
            L.check(L.lib().sed_adam_step_ex(L.ptr(self.flat.p), L.ptr(self.flat.g), L.ptr(self.m), L.ptr(self.v),
                                             L.ptr(self.vmax), self.flat.numel, float(self.param_groups[0]["lr"]),
                                             float(self.betas[0]), float(self.betas[1]), float(self.eps), self.step_count, 1.0,
                                             self.weight_decay, int(self.decoupled_weight_decay), L.ptr(self._coef), st),
                    "adam_step_ex")
            return
        L.check(L.lib().sed_adam_amsgrad_step(L.ptr(self.flat.p), L.ptr(self.flat.g), L.ptr(self.m), L.ptr(self.v),
                                              L.ptr(self.vmax), self.flat.numel, float(self.param_groups[0]["lr"]),
                                              float(self.betas[0]), float(self.betas[1]), float(self.eps),
                                              self.step_count, 1.0, torch.cuda.current_stream().cuda_stream),
                "adam_amsgrad_step")


# ----------------------------------------------------------------------------------------------
# reference-signature loops
# ----------------------------------------------------------------------------------------------
def eval(model, dataloader, criterion, outputs_dir, iteration, device, limit_val_samples=None):
    """train.py:12-74 minus the matplotlib figures: whole recordings, batch 1, running-stat BN,
    sigmoid, 21-threshold metrics.  Returns (losses, recall_sets, precision_sets, APs)."""
    losses, recal_sets, precision_sets, APs = [], [], [], []
    val_sampler = dataloader.dataset.get_validation_sampler(max_validate_num=limit_val_samples)
    for idx, (inp, target, file_name) in enumerate(val_sampler):
        model.eval()
        with torch.no_grad():
            output = model(inp.to(device).float())
        loss = criterion(output, target.to(device).float())
        output = output[0] if inp.dim() == 4 else output
        target = target[0] if inp.dim() == 4 else target.reshape(-1, 1)
        # sigmoid + the 21-threshold counting stay on the device (sed_metric_counts)
        recal_vals, precision_vals, AP = calculate_metrics_device(output, target.to(device).float(), raw_logits=True)
        losses.append(loss.item())
        recal_sets.append(recal_vals)
        precision_sets.append(precision_vals)
        APs.append(AP)
    return losses, recal_sets, precision_sets, APs


def eval_events(model, dataloader, device, *, threshold, low_threshold, median_window, max_gap, min_len, seg_frames,
                collar_frames, limit_val_samples=None):
    """Event-level validation (this build only): every recording of the validation sampler is run like eval() does, its
    probabilities are decoded into events ON THE DEVICE (utils.event_utils.decode_events: median_window / max_gap / min_len /
    seg_frames / collar_frames in frames, threshold / low_threshold on the probability), the reference events are the runs of the
    target, and both are scored over the first min(frames) frames: segment-based counts on the device, summed there; event-based
    (collar) matching on the host, for which each recording costs ONE device-to-host copy, of its two event lists.
    Returns a dict of plain numbers (JSON-ready): segment_f1, segment_error_rate, event_f1 (micro averages), their per-class lists,
    the counts behind them and the numbers of predicted / reference events."""
    from .utils.event_utils import (decode_events, event_based_metrics, events_from_targets, events_to_host,
                                    metrics_from_segment_counts, segment_counts_device)
    val_sampler = dataloader.dataset.get_validation_sampler(max_validate_num=limit_val_samples)
    seg_counts, pred_all, ref_all = None, [], []
    for idx, (inp, target, file_name) in enumerate(val_sampler):
        model.eval()
        with torch.no_grad():
            output = model(inp.to(device).float())
        output = output[0] if inp.dim() == 4 else output
        target = (target[0] if inp.dim() == 4 else target.reshape(-1, 1)).to(device).float()
        n = min(output.shape[0], target.shape[0])
        pred = decode_events(torch.sigmoid(output[:n]), threshold=threshold, low_threshold=low_threshold,
                             median_window=median_window, max_gap=max_gap, min_len=min_len)
        ref = events_from_targets(target[:n])
        c = segment_counts_device(pred.decisions, target[:n], seg_frames)
        seg_counts = c if seg_counts is None else seg_counts + c
        pe, re_ = events_to_host(pred, ref)
        pe[:, 0] = idx                       # (recording, class, onset, offset): events of different recordings never match
        re_[:, 0] = idx
        pred_all.append(pe)
        ref_all.append(re_)
    if seg_counts is None:
        raise RuntimeError("the validation sampler produced no recording")
    seg = metrics_from_segment_counts(seg_counts.cpu().numpy())
    pred_all, ref_all = np.concatenate(pred_all), np.concatenate(ref_all)
    evm = event_based_metrics(pred_all, ref_all, collar_frames)
    return {"segment_f1": seg["micro"]["f1"], "segment_error_rate": seg["micro"]["error_rate"],
            "segment_precision": seg["micro"]["precision"], "segment_recall": seg["micro"]["recall"],
            "segment_f1_per_class": [c["f1"] for c in seg["per_class"]],
            "segment_error_rate_per_class": [c["error_rate"] for c in seg["per_class"]],
            "segment_counts": seg["counts"].tolist(),
            "event_f1": evm["micro"]["f1"], "event_precision": evm["micro"]["precision"], "event_recall": evm["micro"]["recall"],
            "event_f1_per_class": {int(k): v["f1"] for k, v in evm["per_class"].items()},
            "event_counts": [evm["micro"]["tp"], evm["micro"]["fp"], evm["micro"]["fn"]],
            "n_pred_events": int(len(pred_all)), "n_ref_events": int(len(ref_all))}


def check_ranking_options(clip_pooling=None, model=None):
    """Validate eval_ranking's clip_pooling (host only): None, or max / mean / linear / exp on a model with a time axis, or att
    on one with the attention head."""
    if clip_pooling is None:
        return None
    from .engine import check_clip_pooling
    check_clip_pooling(clip_pooling, model)
    if model is not None and not hasattr(model, "conv_blocks"):
        raise ValueError(f"clip pooling pools frame probabilities over time: {type(model).__name__} has no time axis in its "
                         "output (use Cnn_AvgPooling / Crnn_AvgPooling)")
    return clip_pooling


def eval_ranking(model, dataloader, device, *, clip_pooling=None, limit_val_samples=None):
    """Corpus-level rank metrics of the validation set (this build only): every recording of the validation sampler is run like
    eval() does, its frame probabilities -- the sigmoid of sed_metric_counts, the one eval() uses -- and its targets are appended
    ON THE DEVICE to a utils.ranking_utils.RankingAccumulator over the first min(frames) frames, and one sort + scan at the end
    gives per-class AP, ROC-AUC, d' and the best-F1 threshold over all recordings; the host receives 68 bytes per class.
    clip_pooling (max / mean / linear / exp, or att on a model with the attention head): a second accumulator takes one element per recording and class, CnnEngine.clip_probs
    of the whole recording against the clip label (the target's maximum over the scored frames); its result sits under 'clip'.
    Returns the JSON-ready dict of metrics_from_rank_counts plus 'n_recordings'."""
    from .utils.metric_utils import metric_counts_device
    from .utils.ranking_utils import RankingAccumulator
    check_ranking_options(clip_pooling, model)
    val_sampler = dataloader.dataset.get_validation_sampler(max_validate_num=limit_val_samples)
    frames, clips, count = None, None, 0
    for idx, (inp, target, file_name) in enumerate(val_sampler):
        model.eval()
        inp = inp.to(device).float()
        with torch.no_grad():
            output = model(inp)
        output = output[0] if inp.dim() == 4 else output
        target = (target[0] if inp.dim() == 4 else target.reshape(-1, 1)).to(device).float()
        probs = metric_counts_device(output, target, raw_logits=True, return_probs=True)[3]
        if frames is None:
            frames = RankingAccumulator(probs.shape[1], probs.device)
            clips = RankingAccumulator(probs.shape[1], probs.device) if clip_pooling is not None else None
        frames.update(probs, target)
        if clips is not None:        # the plan of the forward just run still holds its logits
            plan = model.engine.plan(inp.shape[0], inp.shape[2], inp.shape[3], inp.device)
            clip = model.engine.clip_probs(plan, clip_pooling)[:1]
            clips.update(clip, target[:probs.shape[0]].max(dim=0, keepdim=True)[0])
        count += 1
    if frames is None:
        raise RuntimeError("the validation sampler produced no recording")
    res = frames.compute()
    res["n_recordings"] = count
    if clips is not None:
        res["clip"] = clips.compute()
        res["clip"]["pooling"] = clip_pooling
    return res


def check_psds_options(scenario=1, thresholds=None, median_window=1, model=None):
    """Validate eval_psds's options (host only): scenario 1, 2 or a dict, 1..64 thresholds, an odd median window in frames, and a
    model with a time axis.  Returns the checked scenario."""
    from .utils.event_utils import MAX_MEDIAN_WINDOW
    from .utils.psds_utils import check_thresholds, resolve_scenario
    s = resolve_scenario(scenario)
    check_thresholds(thresholds)
    w = int(median_window)
    if w < 1 or w > MAX_MEDIAN_WINDOW or w % 2 == 0:
        raise ValueError(f"median window must be odd, 1..{MAX_MEDIAN_WINDOW} frames (got {median_window})")
    if model is not None and not hasattr(model, "conv_blocks"):
        raise ValueError(f"PSDS scores events along time: {type(model).__name__} has no time axis in its output (use "
                         "Cnn_AvgPooling / Crnn_AvgPooling)")
    return s


def eval_psds(model, dataloader, device, *, scenario=1, thresholds=None, median_window=1, fps, limit_val_samples=None):
    """The polyphonic sound detection score of the validation set (this build only): every recording of the validation sampler is
    run like eval() does, its frame probabilities -- the sigmoid of sed_metric_counts, the one eval_ranking takes -- and its targets
    go ON THE DEVICE through utils.psds_utils.PsdsAccumulator (median_window frames of median filter, then one sed_psds_counts per
    recording for the whole threshold sweep), and one copy of the integer counts at the end gives the score.  scenario: 1 or 2 (the
    DCASE task-4 settings) or a dict; thresholds: None = 50 from 0.01 to 0.99; fps: the model's output frames per second.
    Returns {'psds', 'classes_scored', 'best_macro_f1', 'best_macro_f1_threshold', 'scenario', 'n_recordings'} (JSON-ready)."""
    from .utils.metric_utils import metric_counts_device
    from .utils.psds_utils import PsdsAccumulator
    check_psds_options(scenario, thresholds, median_window, model)
    val_sampler = dataloader.dataset.get_validation_sampler(max_validate_num=limit_val_samples)
    acc, count = None, 0
    for idx, (inp, target, file_name) in enumerate(val_sampler):
        model.eval()
        inp = inp.to(device).float()
        with torch.no_grad():
            output = model(inp)
        output = output[0] if inp.dim() == 4 else output
        target = (target[0] if inp.dim() == 4 else target.reshape(-1, 1)).to(device).float()
        probs = metric_counts_device(output, target, raw_logits=True, return_probs=True)[3]
        if acc is None:
            acc = PsdsAccumulator(probs.shape[1], probs.device, thresholds=thresholds, scenario=scenario,
                                  median_window=median_window)
        acc.update(probs, target)
        count += 1
    if acc is None:
        raise RuntimeError("the validation sampler produced no recording")
    res = acc.compute(fps)
    return {"psds": res["psds"], "classes_scored": res["classes_scored"], "best_macro_f1": res["best_macro_f1"],
            "best_macro_f1_threshold": res["best_macro_f1_threshold"],
            "scenario": scenario if not isinstance(scenario, dict) else "custom", "n_recordings": count}


def summarize_validation(val_losses, recal_sets, precision_sets, APs):
    """ProgressPlotter.report_validation_metrics (utils/common.py:46-56): F-scores of the
    validation-AVERAGED precision/recall curves, including the swapped-argument call convention."""
    r = np.mean(recal_sets, axis=0)
    p = np.mean(precision_sets, axis=0)
    return {"val_loss": float(np.mean(val_losses)), "AP": float(np.mean(APs)),
            "max_f1": float(np.max(f_score(p, r, precision_importance_factor=1))),
            "max_f5": float(np.max(f_score(p, r, precision_importance_factor=5)))}


def train(model, data_loader, criterion, num_steps, lr, log_freq, outputs_dir, device, *, weight_decay=0.0,
          decoupled_weight_decay=False, amsgrad=True, max_grad_norm=None, event_eval=None, batch_augment=None,
          weak_pooling=None, weak_weight=1.0, weak_only=False, mean_teacher=False, ema_decay=0.999, consistency_weight=2.0,
          consistency_rampup=0, teacher_augment=None, eval_teacher=False, ranking_eval=None, psds_eval=None, lr_schedule=None,
          param_groups=None):
    """train.py:77-131.  `criterion` must be this package's WeightedBCE(multi_frame=True) (its
    recall_factor feeds the fused loss kernel).  The keyword-only optimizer options are FusedTrainer's (this build only; their
    defaults are the reference's Adam(amsgrad=True) without decay or clipping).  event_eval: None, or the keyword arguments of
    eval_events (threshold ... collar_frames): the periodic evaluation then also logs that dict; None launches nothing new.
    batch_augment: None, or a callable (features, labels) -> (features, labels) applied to every device batch before the step
    (dataset.spectogram.augment.LogMelAugment for loaders that hand plain log-mel tensors over); validation never sees it.
    weak_pooling / weak_weight / weak_only: FusedTrainer's weak-label options.  A utils.common.WeakBCE as `criterion` is shorthand
    for weak_only=True with its pooling and recall_factor; the loader may then hand (B, K) clip labels over.
    The loader yields (features, labels) or (features, labels, kind), kind the (B,) label kinds of FusedTrainer.train_step.
    mean_teacher ... teacher_augment: FusedTrainer's mean-teacher options; eval_teacher=True runs every periodic evaluation on
    trainer.teacher.  Checkpoints carry the teacher's state under 'teacher', beside 'optimizer' (resume with
    trainer.load_state_dict(ck['optimizer'], teacher=ck['teacher'])).  batch_augment does not see the kinds: an augmentation that
    mixes clips (mixup) must not be combined with them.  ranking_eval: None, or the keyword arguments of eval_ranking ({} or
    {'clip_pooling': ...}): the periodic evaluation then also logs that dict under 'ranking' (the teacher's with eval_teacher);
    None launches nothing new.  psds_eval: None, or the keyword arguments of eval_psds ({'fps': ...} and optionally scenario,
    thresholds, median_window): the periodic evaluation then also logs that dict under 'psds' (the teacher's with eval_teacher);
    None launches nothing new.  lr_schedule / param_groups: FusedTrainer's (an LRSchedule; a list of group dicts, e.g.
    no_decay_groups(model)); both None keep the reference's step decay and single group."""
    from .utils.common import WeakBCE, WeightedBCE
    check_optimizer_options(weight_decay, decoupled_weight_decay, amsgrad, max_grad_norm)
    check_group_options(model, lr, lr_schedule, param_groups, weight_decay)
    if isinstance(criterion, WeakBCE):
        if weak_pooling is not None and weak_pooling != criterion.pooling:
            raise ValueError(f"criterion pools with {criterion.pooling!r} but weak_pooling={weak_pooling!r}")
        weak_pooling, weak_only = criterion.pooling, True
    check_weak_options(weak_pooling, weak_weight, weak_only, model)
    check_semi_options(mean_teacher, ema_decay, consistency_weight, consistency_rampup, model)
    check_frontend_options(model, mean_teacher=mean_teacher)
    if eval_teacher and not mean_teacher:
        raise ValueError("eval_teacher needs mean_teacher")
    if ranking_eval is not None:
        if set(ranking_eval) - {"clip_pooling"}:
            raise ValueError(f"ranking_eval takes clip_pooling only (got {sorted(ranking_eval)})")
        check_ranking_options(ranking_eval.get("clip_pooling"), model)
    if psds_eval is not None:
        if set(psds_eval) - {"scenario", "thresholds", "median_window", "fps"} or "fps" not in psds_eval:
            raise ValueError(f"psds_eval takes fps and optionally scenario, thresholds, median_window (got {sorted(psds_eval)})")
        if not float(psds_eval["fps"]) > 0:
            raise ValueError(f"psds_eval: fps must be > 0 (got {psds_eval['fps']})")
        check_psds_options(psds_eval.get("scenario", 1), psds_eval.get("thresholds"), psds_eval.get("median_window", 1), model)
    if mean_teacher and data_parallel_enabled():
        raise RuntimeError("mean_teacher is the single-process path (the teacher's BatchNorm statistics and the order of the EMA "
                           "across ranks are not defined yet)")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("the MI355X training path needs device='cuda' (there is no CPU path)")
    print("Training:")
    print("\t- Using device: ", device)
    os.makedirs(os.path.join(outputs_dir, "checkpoints"), exist_ok=True)
    model.to(dev)
    # the fused step computes WeightedBCE (utils/common.py:11-30) itself: honour exactly that criterion, refuse anything else
    if not isinstance(criterion, (WeightedBCE, WeakBCE)):
        raise TypeError("train() runs the fused WeightedBCE loss kernel: pass this package's WeightedBCE "
                        f"(got {type(criterion).__name__}); other criteria would be silently ignored")
    wants_multi = hasattr(model, "conv_blocks")       # spectrogram models: frame-wise targets; M5: one label per frame
    if isinstance(criterion, WeightedBCE) and bool(criterion.multi_frame) != wants_multi:
        raise ValueError(f"{type(model).__name__} trains with WeightedBCE(multi_frame={wants_multi}) (main.py:44,71)")
    trainer = FusedTrainer(model, lr, recall_factor=criterion.recall_factor,
                           sync_bn=os.environ.get("SED_SYNC_BN", "0") == "1", weight_decay=weight_decay,
                           decoupled_weight_decay=decoupled_weight_decay, amsgrad=amsgrad, max_grad_norm=max_grad_norm,
                           weak_pooling=weak_pooling, weak_weight=weak_weight, weak_only=weak_only, mean_teacher=mean_teacher,
                           ema_decay=ema_decay, consistency_weight=consistency_weight, consistency_rampup=consistency_rampup,
                           teacher_augment=teacher_augment, lr_schedule=lr_schedule, param_groups=param_groups)
    eval_model = trainer.teacher if eval_teacher else model
    rank0 = (not trainer.reducer.enabled) or trainer.reducer.dist.get_rank() == 0
    log_path = os.path.join(outputs_dir, "progress.jsonl")
    losses: List[float] = []
    iterations, epoch = 0, 0
    t0 = time()
    world = trainer.reducer.world
    while iterations < num_steps:
        seen = 0
        for item in data_loader:
            batch_features, event_labels = item[0], item[1]
            kind = item[2].to(dev, non_blocking=True) if len(item) > 2 else None
            seen += 1
            batch_features = batch_features.to(dev, non_blocking=True).float()
            event_labels = event_labels.to(dev, non_blocking=True).float()
            if batch_augment is not None:
                batch_features, event_labels = batch_augment(batch_features, event_labels)
            loss = trainer.train_step(batch_features, event_labels) if kind is None else \
                trainer.train_step(batch_features, event_labels, kind)
            losses.append(loss.clone())              # device scalars (the step's loss buffer is reused): no host sync
            iterations += 1
            if iterations % log_freq == 0:
                host_losses = [float(l) for l in torch.stack([l.reshape(()) for l in losses]).cpu()]
                losses = []
                im_sec = iterations * data_loader.batch_size * world / (time() - t0)      # whole job, all ranks
                rec = {"epoch": epoch, "step": iterations, "train_loss": float(np.mean(host_losses)),
                       "im_sec": im_sec, "lr": trainer.lr}
                if hasattr(data_loader.dataset, "get_validation_sampler"):
                    rec.update(summarize_validation(*eval(eval_model, data_loader, criterion, outputs_dir,
                                                          iteration=iterations, device=dev, limit_val_samples=3)))
                    if event_eval is not None:
                        rec.update(eval_events(eval_model, data_loader, dev, limit_val_samples=3, **event_eval))
                    if ranking_eval is not None:
                        rec["ranking"] = eval_ranking(eval_model, data_loader, dev, limit_val_samples=3, **ranking_eval)
                    if psds_eval is not None:
                        rec["psds"] = eval_psds(eval_model, data_loader, dev, limit_val_samples=3, **psds_eval)
                if rank0:
                    print(f"epoch: {epoch}, step: {iterations}, loss: {host_losses[-1]:.2f}, "
                          f"im/sec: {im_sec:.1f}, lr: {trainer.lr:.8f}")
                    with open(log_path, "a") as f:
                        f.write(json.dumps(rec) + "\n")
                    ck = {"iterations": iterations, "model": model.state_dict(), "optimizer": trainer.state_dict()}
                    if trainer.teacher is not None:
                        ck["teacher"] = ck["optimizer"].pop("teacher")
                    torch.save(ck,
                               os.path.join(outputs_dir, "checkpoints", f"iteration_{iterations}.pth"))
            if iterations == num_steps:
                break
        if seen == 0:
            raise RuntimeError("the data loader produced no batch in a whole epoch (dataset smaller than "
                               "batch_size x world_size?): training cannot make progress")
        epoch += 1
    return trainer
