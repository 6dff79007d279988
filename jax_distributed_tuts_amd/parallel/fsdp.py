"""FSDP / ZeRO-3 parameter sharding (reference param_sharding.py:58-397).

Reference mechanism (flax):
  * ``shard_params`` (param_sharding.py:58-125): per leaf, skip if already
    sharded on the axis, keep replicated if ``size <= min_weight_size``, else
    shard the first dim in descending-size order that divides evenly.
  * ``gather_arr_mean_grads`` (:129-142): custom-VJP all_gather whose backward
    is reduce-scatter / N -- where FSDP's gradient averaging happens.
  * ``shard_module_params`` (:179-191): ``nn.map_variables`` gathering on read,
    sharding on write.
  * ``sync_gradients`` (:293-322): pmean over the mesh axes a grad is NOT
    sharded on (replicated leaves).
  * Adam moments mirror the Partitioned boxes: optimizer state is sharded.

MI355X engine (``FSDPTrainer``): each rank owns a LOCAL flat buffer (shards +
replicated leaves) with its own fp32 master, AdamW moments and bf16 shadow;
a FULL flat buffer holds the gathered bf16 weights and full fp32 grads.
Per minibatch (faithful to the reference) the bf16 SHADOW shards are
all-gathered (half the bytes of gathering fp32 -- cast-then-gather equals
gather-then-cast), the same explicit fwd/bwd kernels as DP run on the full
buffer, and full grads are reduce-scattered (SUM) into the local grad buffer.
Replicated leaves + the 4 metric scalars form the contiguous tail of the local
grad buffer: ONE all-reduce (``sync_gradients`` + ``synch_metrics``).  The
1/N of reduce-scatter-mean and pmean and the 1/n_mb of accumulation are one
scale inside the fused AdamW.  Flags ``gather_once``/``scatter_once`` gather
once per step / reduce-scatter once per step (identical maths, 4x fewer
collectives) -- documented optimisations, off by default.
"""
from __future__ import annotations

import logging
import math
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.distributed as dist

from ..comm import collectives as C
from ..models.mlp import MLP, loss_and_grad
from ..ops import kernels as K
from ..runtime.dist import Mesh
from ..utils import rng as R
from ..utils.flat import FlatParams, ParamSpec, N_METRIC_SLOTS
from ..utils.profiling import named_scope
from ..utils.train_state import AdamW, Batch, TrainState
from .step_program import CapturedStep, hw_queues, mb_streams

log = logging.getLogger("jdt.fsdp")


# ---------------------------------------------------------------------------- sharding metadata
@dataclass
class Partitioned:
    """Analogue of ``flax.linen.Partitioned``: a (local) value plus per-dim mesh
    axis names (None = not sharded on that dim) and the global shape."""

    value: Optional[torch.Tensor]
    names: Tuple[Optional[str], ...]
    global_shape: Tuple[int, ...] = ()

    @property
    def shard_dim(self) -> Optional[int]:
        for i, n in enumerate(self.names):
            if n is not None:
                return i
        return None


def shard_rule(shape: Sequence[int], names: Sequence[Optional[str]], axis_name: str, axis_size: int,
               min_weight_size: int, path: str = "") -> Tuple[Optional[int], Tuple[Optional[str], ...]]:
    """The per-leaf decision of param_sharding.py:82-118 (with bug B5 fixed).

    Returns (dim to shard or None, new names)."""
    names = tuple(names) if names else (None,) * len(shape)
    if axis_name in names:
        log.warning("Parameter %s with names %s already sharded on axis %s.", path, names, axis_name)
        return None, names
    size = int(np.prod(shape))
    if size <= min_weight_size:
        log.info("Parameter %s with shape %s and size %d is too small to shard, size %d.", path, tuple(shape), size,
                 min_weight_size)
        return None, names
    for i in np.argsort(np.asarray(shape))[::-1]:
        i = int(i)
        if shape[i] % axis_size == 0 and names[i] is None:
            return i, names[:i] + (axis_name,) + names[i + 1:]
    log.warning("Could not shard %s with shape %s and names %s on axis %s, no suitable axis found", path,
                tuple(shape), names, axis_name)
    return None, names


def shard_params(params: Dict[str, torch.Tensor | Partitioned], mesh: Optional[Mesh], axis_name: str,
                 min_weight_size: int = 2 ** 18) -> Dict[str, torch.Tensor | Partitioned]:
    """param_sharding.py:58-125: full (replicated) leaves -> this rank's shard."""
    with named_scope("shard_params"):
        n = C.axis_size(mesh, axis_name)
        idx = C.axis_index(mesh, axis_name)
        out = {}
        for path, x in params.items():
            if isinstance(x, Partitioned):
                value, names, gshape = x.value, x.names, x.global_shape
            else:
                value, names, gshape = x, (None,) * x.dim(), tuple(x.shape)
            d, new_names = shard_rule(tuple(value.shape), names, axis_name, n, min_weight_size, path)
            if d is None:
                out[path] = x
                continue
            split = value.shape[d] // n
            local = value.narrow(d, idx * split, split).clone()
            out[path] = Partitioned(local, new_names, tuple(gshape))
        return out


class _GatherMeanGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mesh, axis_name, dim):
        ctx.mesh, ctx.axis, ctx.dim = mesh, axis_name, dim
        return C.all_gather(x, mesh, axis_name, dim=dim).clone()

    @staticmethod
    def backward(ctx, g):
        n = C.axis_size(ctx.mesh, ctx.axis)
        out = C.psum_scatter(g.contiguous(), ctx.mesh, ctx.axis, dim=ctx.dim)
        return out / n, None, None, None


def gather_arr_mean_grads(x: torch.Tensor, mesh: Optional[Mesh], axis_name: str, dim: int) -> torch.Tensor:
    """param_sharding.py:129-142: all-gather fwd, reduce-scatter-mean bwd (autograd)."""
    return _GatherMeanGrad.apply(x, mesh, axis_name, dim)


def gather_params(params: Dict[str, torch.Tensor | Partitioned], mesh: Optional[Mesh], axis_name: str):
    """param_sharding.py:146-175."""
    with named_scope("gather_params"):
        out = {}
        for path, p in params.items():
            if isinstance(p, Partitioned) and axis_name in p.names:
                d = p.names.index(axis_name)
                v = gather_arr_mean_grads(p.value, mesh, axis_name, d)
                names = p.names[:d] + (None,) + p.names[d + 1:]
                out[path] = Partitioned(v, names, p.global_shape) if any(n is not None for n in names) else v
            else:
                out[path] = p
        return out


def sync_gradients(grads: Dict[str, torch.Tensor | Partitioned], mesh: Optional[Mesh],
                   axis_names: Sequence[str]) -> Dict[str, torch.Tensor | Partitioned]:
    """param_sharding.py:293-322: pmean each grad over the axes it is NOT sharded on
    (a Partitioned grad sharded on every axis is already averaged by C22)."""
    with named_scope("sync_grad"):
        for path, g in grads.items():
            if isinstance(g, Partitioned):
                repl = [a for a in axis_names if a not in g.names]
                for a in repl:
                    C.pmean_(g.value, mesh, a)
            else:
                for a in axis_names:
                    C.pmean_(g, mesh, a)
        return grads


class ShardedModule(torch.nn.Module):
    """``shard_module_params`` (param_sharding.py:179-191) for arbitrary torch
    modules: parameters are replaced by their local shards (registered as
    parameters ``<name>__shard``); forward gathers them through
    :func:`gather_arr_mean_grads` and calls the wrapped module functionally, so
    autograd produces reduce-scatter-mean gradients on the shards."""

    def __init__(self, module: torch.nn.Module, mesh: Optional[Mesh], axis_name: str,
                 min_weight_size: int = 2 ** 18):
        super().__init__()
        self.inner = module
        self.mesh, self.axis_name = mesh, axis_name
        full = {n: p.detach() for n, p in module.named_parameters()}
        sharded = shard_params(full, mesh, axis_name, min_weight_size)
        self.meta: Dict[str, Tuple[Tuple[Optional[str], ...], Tuple[int, ...]]] = {}
        self.local = torch.nn.ParameterDict()
        for n, v in sharded.items():
            key = n.replace(".", "__")
            if isinstance(v, Partitioned):
                self.local[key] = torch.nn.Parameter(v.value)
                self.meta[n] = (v.names, v.global_shape)
            else:
                self.local[key] = torch.nn.Parameter(v.clone())
        for n, _ in list(module.named_parameters()):
            mod, attr = self._owner(n)
            delattr(mod, attr)
            setattr(mod, attr, torch.zeros(0))

    def _owner(self, name):
        parts = name.split(".")
        mod = self.inner
        for p in parts[:-1]:
            mod = getattr(mod, p)
        return mod, parts[-1]

    def gathered(self) -> Dict[str, torch.Tensor]:
        params = {}
        for key, v in self.local.items():
            n = key.replace("__", ".")
            if n in self.meta:
                names, gshape = self.meta[n]
                params[n] = Partitioned(v, names, gshape)
            else:
                params[n] = v
        return gather_params(params, self.mesh, self.axis_name)

    def forward(self, *args, **kw):
        params = self.gathered()
        return torch.func.functional_call(self.inner, params, args, kw)

    def partitioned_grads(self) -> Dict[str, torch.Tensor | Partitioned]:
        out = {}
        for key, v in self.local.items():
            n = key.replace("__", ".")
            g = v.grad if v.grad is not None else torch.zeros_like(v)
            out[n] = Partitioned(g, self.meta[n][0], self.meta[n][1]) if n in self.meta else g
        return out


def shard_module_params(module: torch.nn.Module, mesh: Optional[Mesh], axis_name: str,
                        min_weight_size: int = 2 ** 18) -> ShardedModule:
    return ShardedModule(module, mesh, axis_name, min_weight_size)


# ---------------------------------------------------------------------------- engine
@dataclass
class FSDPConfig:
    num_minibatches: int = 4
    min_weight_size: int = 2 ** 18
    axis: str = "data"
    gather_once: bool = False
    scatter_once: bool = False
    fused_kernels: bool = False   # classifier: whole-step fused kernels on the gathered buffer (implies *_once)
    comm: str = "auto"            # "auto" | "xgmi" | "rccl": N>1 gather / reduce-scatter transport
    # the reference's per-minibatch schedule (gather / fwd+bwd / reduce-scatter every
    # minibatch) on the fused per-layer md kernels (parallel/fused_stage.py) instead of
    # the generic GEMM chain, where the model and the collectives allow (GPU, tutorial
    # MLP shapes, N = 1 or every sharded leaf on the xGMI kernels)
    fused_loop: bool = True
    # N = 1 (every shard the whole leaf, no per-minibatch collective): minibatch i of the
    # fused loop on stream i % loop_streams with its own grad set, as DPConfig.loop_streams
    # (0 = auto: 2 for models of >= 3 layers, else 1)
    loop_streams: int = field(default_factory=lambda: int(os.environ.get("JDT_LOOP_STREAMS", "0")))


class ShardedFlatParams:
    """Local (sharded) + full (gathered) flat buffers for an explicit-backward model."""

    def __init__(self, specs: Sequence[ParamSpec], mesh: Optional[Mesh], axis: str, min_weight_size: int, device):
        self.mesh, self.axis = mesh, axis
        n = C.axis_size(mesh, axis)
        self.n = n
        self.global_specs = list(specs)
        self.part: Dict[str, Partitioned] = {}
        sharded, repl = [], []
        for s in specs:
            d, names = shard_rule(s.shape, (None,) * len(s.shape), axis, n, min_weight_size, s.name)
            if d is None:
                repl.append(ParamSpec(s.name, s.shape, s.init))
                self.part[s.name] = Partitioned(None, names, tuple(s.shape))
            else:
                lshape = tuple(s.shape[i] // n if i == d else s.shape[i] for i in range(len(s.shape)))
                sharded.append(ParamSpec(s.name, lshape, s.init))
                self.part[s.name] = Partitioned(None, names, tuple(s.shape))
        self.sharded_names = [s.name for s in sharded]
        self.repl_names = [s.name for s in repl]
        # local buffer: sharded leaves first, then replicated leaves, then metric slots
        self.local = FlatParams(sharded + repl, device=device)
        self.full = FlatParams(specs, device=device, metric_slots=0)
        self.repl_start = self.local.offsets[repl[0].name][0] if repl else self.local.metric_off
        self.xg = None  # comm/xgmi.XgmiComm: direct xGMI segmented gather / reduce-scatter (attach_xgmi)
        self._xg_names: List[str] = []

    def attach_xgmi(self, comm) -> None:
        """Route the dim-0 sharded leaves (and the replicated tail's all-reduce)
        through ONE segmented xGMI kernel per collective instead of one RCCL call
        per leaf; leaves the kernel cannot move stay on RCCL."""
        from ..comm.xgmi import XgmiComm

        self.xg = comm
        # dim 0, or dim 1 of a 2-D leaf (the reference rule shards a square weight along
        # its last dim): both are layouts of the segmented kernel
        self._xg_names = [n for n in self.sharded_names
                          if (self.part[n].shard_dim == 0 or (self.part[n].shard_dim == 1
                                                                and self.full.s(n).dim() == 2))
                          and XgmiComm.segment_ok(self.full.s(n), self.local.s(n), self.n)
                          and XgmiComm.segment_ok(self.full.g(n), self.local.g(n), self.n)]

    def global_num_params(self) -> int:
        return sum(int(math.prod(s.shape)) for s in self.global_specs)

    def num_params(self) -> int:
        return self.global_num_params()

    def init_(self, seed: int):
        """Full init with the same seed on every rank, then keep this rank's shard
        (param_sharding.py:227-288 semantics)."""
        tmp = FlatParams(self.global_specs, device="cpu", with_grad=False, with_shadow=False, metric_slots=0)
        tmp.init_(seed)
        idx = C.axis_index(self.mesh, self.axis)
        for name, pt in self.part.items():
            full = tmp.p(name)
            d = pt.shard_dim
            if d is None:
                self.local.p(name).copy_(full)
            else:
                split = full.shape[d] // self.n
                self.local.p(name).copy_(full.narrow(d, idx * split, split))
        self.local.sync_shadow()
        self.gather()
        return self

    # ------------------------------------------------------------------ comm
    def gather(self):
        """all-gather bf16 shadow shards -> full shadow (X05); replicated: local copy."""
        with named_scope("gather_params"):
            if self.xg is not None and self._xg_names:
                self.xg.all_gather_segments([(self.full.s(n), self.local.s(n)) for n in self._xg_names])
            for name in self.sharded_names:
                if self.xg is not None and name in self._xg_names:
                    continue
                d = self.part[name].shard_dim
                C.all_gather(self.local.s(name), self.mesh, self.axis, dim=d, out=self.full.s(name))
            for name in self.repl_names:
                self.full.s(name).copy_(self.local.s(name))

    def scatter_grads(self, accumulate: bool, zero_full: bool = True, with_replicated: bool = False) -> bool:
        """full fp32 grads -> reduce-scatter SUM into local grads (X06); replicated
        grads copied into the local tail.  Full grads are zeroed.

        ``with_replicated`` (the step's last scatter): on the xGMI path the local tail
        (replicated leaves' grads + metric slots, i.e. sync_replicated's all-reduce)
        rides in the same launch as an all-reduce segment -- one collective per step
        fewer.  Returns True if it did (then skip sync_replicated)."""
        fold = (with_replicated and not accumulate and self.xg is not None and bool(self._xg_names)
                and len(self._xg_names) < 16 and (self.local.grad.numel() - self.repl_start) % 4 == 0
                and self.repl_start % 4 == 0)
        with named_scope("scatter_grads"):
            if fold:
                for name in self.repl_names:
                    self.local.g(name).copy_(self.full.g(name))
                self.xg.reduce_scatter_segments([(self.full.g(n), self.local.g(n)) for n in self._xg_names],
                                                accumulate=False, allreduce=[self.local.grad[self.repl_start:]])
            elif self.xg is not None and self._xg_names:
                self.xg.reduce_scatter_segments([(self.full.g(n), self.local.g(n)) for n in self._xg_names],
                                                accumulate=accumulate)
            for name in self.sharded_names:
                if self.xg is not None and name in self._xg_names:
                    continue
                d = self.part[name].shard_dim
                if accumulate:
                    tmp = C.psum_scatter(self.full.g(name), self.mesh, self.axis, dim=d)
                    self.local.g(name).add_(tmp)
                else:
                    C.psum_scatter(self.full.g(name), self.mesh, self.axis, dim=d, out=self.local.g(name))
            for name in self.repl_names:
                if fold:
                    continue  # copied before the launch
                if accumulate:
                    self.local.g(name).add_(self.full.g(name))
                else:
                    self.local.g(name).copy_(self.full.g(name))
            if zero_full:
                self.full.grad.zero_()
        return fold

    def sync_replicated(self):
        """sync_gradients for replicated leaves + synch_metrics: ONE all-reduce of the tail."""
        with named_scope("sync_grad"):
            if self.xg is not None:
                self.xg.all_reduce_(self.local.grad[self.repl_start:])
            else:
                C.psum_(self.local.grad[self.repl_start:], self.mesh, self.axis)


def init_fsdp(model: MLP, tx, seed: int, device, mesh: Optional[Mesh], axis: str = "data",
              min_weight_size: int = 2 ** 18) -> TrainState:
    sp = ShardedFlatParams(model.param_specs(), mesh, axis, min_weight_size, device).init_(seed)
    st = TrainState(step=0, apply_fn=model, params=sp.local, tx=tx, opt_state=tx.init(sp.local),
                    rng=R.PRNGKey(seed))
    st.extra["sharded"] = sp
    return st


class _LoopView:
    """The parameter view of the fused per-minibatch FSDP loop: bf16 weights from the
    gathered full shadow, gradients of the SHARDED leaves into the full fp32 buffer
    (reduce-scattered after every minibatch, gather_arr_mean_grads), gradients of the
    replicated leaves and the metric slots straight into the local buffer -- they
    accumulate over the minibatches and are all-reduced once per step
    (sync_gradients), exactly the reference's split (param_sharding.py:129-142,
    343-367).  At N = 1 every shard is the whole leaf: everything is local."""

    def __init__(self, sp: ShardedFlatParams):
        self.sp = sp
        self.one = sp.n == 1
        self.master = sp.local.master

    def s(self, name):
        # replicated leaves: the local bf16 shadow, which the optimizer keeps current (the
        # per-minibatch all-gather moves only the sharded leaves, so the full buffer's copy
        # of a replicated leaf is only as fresh as the last sp.gather())
        return self.sp.local.s(name) if (self.one or name in self.sp.repl_names) else self.sp.full.s(name)

    def g(self, name):
        return self.sp.local.g(name) if (self.one or name in self.sp.repl_names) else self.sp.full.g(name)

    @property
    def metrics_slot(self):
        return self.sp.local.metrics_slot

    @property
    def grad(self):
        """The buffer every g() view lives in -- only at N = 1 (grad sets, FusedMLPStage)."""
        assert self.one, "private grad sets need every gradient in one local buffer (N = 1)"
        return self.sp.local.grad


class FSDPTrainer(CapturedStep):
    scope = "train_step_fsdp"

    def __init__(self, state: TrainState, mesh: Optional[Mesh], cfg: FSDPConfig = FSDPConfig()):
        CapturedStep.__init__(self)
        self.state, self.mesh, self.cfg = state, mesh, cfg
        self.sp: ShardedFlatParams = state.extra["sharded"]
        self.model: MLP = state.apply_fn
        self.metrics = torch.zeros(N_METRIC_SLOTS, dtype=torch.float32, device=self.sp.local.master.device)
        self.world = C.axis_size(mesh, cfg.axis)
        # one device and no collective to issue: gather / reduce-scatter are identities and
        # the step is the DP engine on the local buffer (a Mesh(unit_groups=True) keeps the
        # N > 1 schedule, RCCL calls included, on one GPU)
        self._n1 = not (self.world > 1 or C.active(mesh, cfg.axis))
        self.fused = None
        self._txx = None          # the one-launch step's tile exchange (_tile_exchange)
        self._plan = None         # the fused step collective's arguments (_fsdp_plan) ...
        self._staged = False      # ... and whether the engine writes into its staging buffer
        self._full_fresh = True   # init_fsdp gathered the full shadow
        self._loop_engine = None
        self._loop_tried = False
        self._loop_streams = None
        self._shard_full = None   # the loop engine's full-grad ranges of the sharded leaves
        if self.world > 1 and self.sp.local.master.is_cuda and self.sp.xg is None:
            from ..comm.xgmi import create_for

            xg = create_for(mesh, cfg.axis, self.sp.full.grad.numel(), self.sp.local.master.device, cfg.comm)
            if xg is not None:
                self.sp.attach_xgmi(xg)
        from ..utils.checkpoint import bind_trainer

        bind_trainer(state, self)

    def invalidate(self):
        """After a checkpoint restore: drop the fused engine and captured graphs."""
        self._loop_engine = None
        self._loop_tried = False
        self.fused = None
        self._drop_graphs()
        self._plan = None
        self._full_fresh = False

    @property
    def one_launch(self) -> bool:
        """N > 1 step as one run-ahead launch with the in-kernel sharded exchange."""
        return getattr(self.fused, "fsdp_tx", False)

    def _tile_exchange(self, batch: Batch):
        """(TileExchange, ranks sharing this GPU) for the N > 1 FSDP step without a
        separate collective launch, or (None, 1).  2-layer classifier: ONE run-ahead launch
        per step (csrc/mlp_fused.hip FX); deep classifier (JDT_FSDP_DEEP_FX, default 1): one backward
        launch per hidden layer, each sending its tiles' partials to the row owners, which
        apply the sharded AdamW and hand the values back (csrc/mlp_deep.hip md_bwd FX).
        Both need AdamW, the reference's dim-0 shards of every kernel and bias (the head
        bias replicated) with whole 16-unit column blocks per rank, not deterministic, every
        rank's grid co-resident with the grids of the ranks sharing its GPU -- agreed by
        all ranks (collective).  JDT_FSDP_AHEAD=0: the forward / backward / fused FSDP
        collective step."""
        if not (self.world > 1 and batch.inputs.is_cuda and os.environ.get("JDT_FSDP_AHEAD", "1") == "1"):
            return None, 1
        from ..comm import tile_exchange as TX
        from ..runtime.dist import ranks_per_gpu
        from ..utils.train_state import AdamW
        from .fused_mlp import FusedMLPDeep, deterministic, md_ahead_ok, mlp2_chunk, supported, supported_deep

        sp, W, dev = self.sp, self.world, batch.inputs.device
        share = ranks_per_gpu()
        dims = {n: sp.part[n].shard_dim for n in sp.part}
        names = list(getattr(self.model, "names", ()))

        def dim_ok(name, d):
            # dim-0 shards (the head bias replicated); a square hidden kernel also dim 1
            layer, leaf = name.split("/")
            if layer == names[-1] and leaf == "bias":
                return d is None
            if leaf == "kernel" and layer not in (names[0], names[-1]):
                return d in (0, 1)
            return d == 0

        base = (bool(names) and set(dims) == {f"{n}/{leaf}" for n in names for leaf in ("kernel", "bias")}
                and all(dim_ok(n, d) for n, d in dims.items()) and isinstance(self.state.tx, AdamW)
                and not deterministic())
        if supported(self.model, batch.size, dev):
            K, H = self.model.dims[0], self.model.dims[1]
            kc = mlp2_chunk(K)
            # the kernel's partial stores reach a W1 chunk's first and last owner only
            # (tile_exchange.fx_owner_span); W must divide both sharded dims
            local = (base and K % W == 0 and H % (16 * W) == 0 and TX.fx_owner_span(W, K, kc) <= 2
                     and TX.ahead_tx_ok(batch.size, H, share, K))
            tiles = (H // 16) * (K // kc)
        elif supported_deep(self.model, batch.size, dev):
            # layer 0 (784 rows, 112-row chunks) and the 512-row layers (64-row chunks)
            # default on: 88 vs 111 us per step against the step collective at 2 ranks
            # sharing the GPU (profiles/r5_autotune_validation.txt, session 12)
            local = (base and os.environ.get("JDT_FSDP_DEEP_FX", "1") == "1"
                     and os.environ.get("JDT_MLP2_AHEAD", "1") == "1" and 784 % W == 0 and 512 % (16 * W) == 0
                     and TX.fx_owner_span(W, 784, 112) <= 2 and TX.fx_owner_span(W, 512, 64) <= 2
                     and bool(md_ahead_ok(batch.size)) and TX.deep_fx_ok(batch.size, share))
            tiles = FusedMLPDeep.tx_tiles(self.model.L - 1)
        else:
            local, tiles = False, 0
        tx, share = TX.renew_for(self._txx, self.mesh, self.cfg.axis, dev, tiles, local)
        self._txx = tx or self._txx   # (no agreement: the old one stays, for close())
        return tx, share

    def _fsdp_plan(self):
        """Arguments of the fused FSDP step collective (comm/xgmi.py ``fsdp_plan``), or
        None when it does not apply: every sharded leaf must move on the segmented xGMI
        kernel, AdamW, <= 16 segments (JDT_FSDP_FUSED_COMM=0 turns it off)."""
        if self._plan is not None:
            return self._plan
        from ..utils.train_state import AdamW

        sp, st = self.sp, self.state
        if (sp.xg is None or len(sp._xg_names) != len(sp.sharded_names) or not isinstance(st.tx, AdamW)
                or len(sp.sharded_names) + len(sp.repl_names) + 1 > 16
                or os.environ.get("JDT_FSDP_FUSED_COMM", "1") == "0"):
            return None
        tx, o = st.tx, st.opt_state
        self._staged = False
        self._plan = sp.xg.fsdp_plan(
            [(sp.full.g(n), sp.local.g(n), sp.full.s(n)) for n in sp.sharded_names],
            [(sp.full.g(n), sp.local.g(n), sp.full.s(n)) for n in sp.repl_names],
            sp.local.metrics_slot, grad_base=sp.local.grad, p=sp.local.master, m=o["m"], v=o["v"],
            shadow=sp.local.shadow, running=self.metrics, lr=tx.learning_rate, b1=tx.b1, b2=tx.b2, eps=tx.eps,
            wd=tx.weight_decay, grad_scale=1.0 / (self.cfg.num_minibatches * self.world), step=o["count"],
            ticket=o["ticket"])
        return self._plan

    def _stage_producer(self):
        """The fused engine writes its gradients straight into the collective's staging
        buffer (packed FSDP layout, step-parity half): the step's collective skips its
        staging copy -- the FSDP form of DP's staged bucket (JDT_FSDP_STAGED=0: off)."""
        if (self._staged or self._plan is None or self.fused is None
                or not hasattr(self.fused, "set_fsdp_stage") or os.environ.get("JDT_FSDP_STAGED", "1") == "0"):
            return
        sp = self.sp
        leaves = ([(n, self.sp.part[n].global_shape, self.sp.part[n].shard_dim) for n in sp.sharded_names]
                  + [(n, self.sp.part[n].global_shape, None) for n in sp.repl_names])
        lay = sp.xg.fsdp_stage_layout(self._plan, leaves)
        sp.xg.stage_clear()   # packed positions no producer writes (segment padding) reduce to zero
        self.fused.set_fsdp_stage(lay, lay["base"], lay["half"], lay["slice"], self.world)
        self._plan[1].staged = 1
        self._staged = True

    @property
    def comm_backend(self) -> str:
        if self._n1:
            return "none"
        if self.sp.xg is not None:
            return "xgmi"
        from ..runtime.dist import backend_name

        return backend_name()

    @property
    def xgmi_status(self) -> str:
        from ..comm.xgmi import status

        return status(self.sp.xg, self.world, self.sp.local.master.device, self.cfg.comm)

    def _fused_step(self, batch: Batch) -> bool:
        """gather bf16 shards once -> mlp2_fwd/mlp2_bwd on the full buffer (mode 0:
        plain-stored full grads + metric slots) -> reduce-scatter -> sharded AdamW."""
        if not self.cfg.fused_kernels:
            return False
        sp = self.sp
        if self.fused is None:
            from .fused_mlp import make_engine

            if self._n1:
                # one device: every shard is the whole leaf (param_sharding.py:89-113 at
                # N=1) and the gather / reduce-scatter are identities, so the step is the
                # DP engine on the local buffer with AdamW in the backward epilogue
                self.fused = make_engine(self.state, self.mesh, self.cfg.axis, self.cfg.num_minibatches,
                                         batch.size, self.metrics, batch.inputs.device)
            else:
                tx, share = self._tile_exchange(batch)
                if tx is not None:
                    # ONE launch per step: each tile's partial gradients go to their rows'
                    # owners, which apply the sharded AdamW and hand the updated values back
                    # (csrc/mlp_fused.hip FX); no separate collective
                    self.fused = make_engine(self.state, self.mesh, self.cfg.axis, self.cfg.num_minibatches,
                                             batch.size, self.metrics, batch.inputs.device, params=sp.full,
                                             fuse_opt=True, tx=tx, ranks_on_gpu=share, opt_params=sp.local)
                else:
                    self.fused = make_engine(self.state, self.mesh, self.cfg.axis, self.cfg.num_minibatches,
                                             batch.size, self.metrics, batch.inputs.device, params=sp.full,
                                             mslot=sp.local.metrics_slot, fuse_opt=False)
            if self.fused is None:
                self.cfg.fused_kernels = False
                return False
        if self._n1:
            self.fused.forward_backward(batch)
            if not self.fused.fuse_opt:
                self.state.tx.update(sp.local, self.state.opt_state, 1.0 / self.cfg.num_minibatches, zero_grad=False)
                with named_scope("synch_metrics"):
                    K.metrics_fold_(self.metrics, sp.local.metrics_slot)
            return True
        if self.one_launch:
            if not self._full_fresh:
                sp.gather()
                self._full_fresh = True
            self.fused.forward_backward(batch)   # the run-ahead launch with the in-kernel exchange
            return True
        plan = self._fsdp_plan()
        if plan is not None:
            # ONE collective launch: reduce-scatter + sharded AdamW + replicated all-reduce
            # + metrics fold + the next step's bf16 all-gather (xg_fsdp_kernel); the full
            # shadow the forward reads was gathered by the previous step's launch
            if not self._full_fresh:
                sp.gather()
                self._full_fresh = True
            self._stage_producer()
            self.fused.forward_backward(batch)
            with named_scope("scatter_update_gather"):
                sp.xg.fsdp_step(plan)
            return True
        sp.gather()
        self.fused.forward_backward(batch)
        if not sp.scatter_grads(accumulate=False, zero_full=False, with_replicated=True):
            sp.sync_replicated()
        self.state.tx.update(sp.local, self.state.opt_state, 1.0 / (self.cfg.num_minibatches * self.world),
                             zero_grad=False)
        with named_scope("synch_metrics"):
            K.metrics_fold_(self.metrics, sp.local.metrics_slot)
        return True

    @property
    def _batch_engines(self):
        return (self.fused, self._loop_engine)

    # ------------------------------------------------------------------ hipGraph
    @property
    def capturable(self) -> bool:
        """N=1, every collective of the step an xGMI kernel, or RCCL (which enqueues on
        the capturing stream; reference: the step under one jit, param_sharding.py:370-379).
        Only a gloo group's host-side collectives keep the step eager."""
        from ..runtime.dist import collectives_capturable

        if self.sp.local.master.device.type != "cuda":
            return False
        return (self._n1 or (self.sp.xg is not None and len(self.sp._xg_names) == len(self.sp.sharded_names))
                or collectives_capturable())

    def capture(self, batch: Batch, steps_per_graph: int = 1):
        """Record the whole step (gather, fwd/bwd, reduce-scatter, replicated
        all-reduce, sharded AdamW, metrics fold) as a hipGraph; with
        ``steps_per_graph`` > 1 also a graph of that many consecutive steps."""
        assert self.capturable and batch.inputs.is_cuda
        if not self._full_fresh:   # the fused step collective keeps the full shadow current
            self.sp.gather()
            self._full_fresh = True

        # N = 1 on the fused engine with AdamW in its epilogue: one run-ahead launch per
        # step (the DP engine's schedule, fused_mlp.AheadGraphs)
        def ahead():
            ok = (self._n1 or self.one_launch) and getattr(self.fused, "ahead_ok", False)
            return self.fused if ok else None

        # (False: a collective refused stream capture, the step stays eager)
        return self._capture(lambda: self._eager_step(batch), batch, steps_per_graph, ahead)

    def _fused_loop(self, mb: int, seed: int):
        """FusedMLPStage (one stage = the whole classifier) on the _LoopView: minibatch
        i, layer l draws dropout stream (i << 16) + (l << 1) at the step counter -- the
        generic loop's masks below."""
        if not self._loop_tried:
            self._loop_tried = True
            from .fused_stage import FusedMLPStage, stage_supported

            sp = self.sp
            dev = sp.local.master.device
            coll_ok = self._n1 or (sp.xg is not None and len(sp._xg_names) == len(sp.sharded_names))
            if self.cfg.fused_loop and coll_ok and stage_supported(self.model, mb, dev):
                k = min(int(self.cfg.loop_streams) or (2 if self.model.L >= 3 else 1), hw_queues())
                self._loop_engine = FusedMLPStage(self.model, _LoopView(sp), self.cfg.num_minibatches, mb,
                                                  self.state.step_tensor, seed,
                                                  n_sets=min(k, self.cfg.num_minibatches) if self._n1 else 1)
                # sharded leaves' full-grad range (zeroed after each minibatch's reduce-scatter)
                offs = sorted((sp.full.offsets[n][0], sp.full.g(n).numel()) for n in sp.sharded_names)
                self._shard_full = [sp.full.grad[o:o + n] for o, n in offs]
        return self._loop_engine

    def _eager_step(self, batch: Batch):
        """train_step_fsdp (param_sharding.py:343-367): one step of device work (no host
        counters, so it can be captured)."""
        if self._fused_step(batch):
            return
        st, sp, cfg = self.state, self.sp, self.cfg
        rng = R.fold_rng_over_axis(st.rng, self.mesh, cfg.axis)
        seed = rng & 0xFFFFFFFF
        n_mb = cfg.num_minibatches
        mb = batch.size // n_mb
        eng = self._fused_loop(mb, seed) if batch.inputs.is_cuda else None
        if eng is not None:
            # param_sharding.py's schedule on the md kernels: per minibatch gather the bf16
            # shards, forward + CE + backward, reduce-scatter the sharded leaves' grads
            # into the local shards (replicated leaves accumulate locally); then ONE
            # all-reduce of the local tail (replicated grads + metric slots), AdamW
            k = eng.n_sets   # > 1 only at N = 1: no collective inside the loop
            on = mb_streams(self._loop_streams, k, batch.inputs.device)
            self._loop_streams = on.side or self._loop_streams
            on.fork()
            for i in range(n_mb):
                if not self._n1 and (i == 0 or not cfg.gather_once):
                    sp.xg.all_gather_segments([(sp.full.s(n), sp.local.s(n)) for n in sp._xg_names])
                with on(i):
                    eng.forward(i, batch.inputs[i * mb:(i + 1) * mb])
                    eng.backward(i, labels=batch.labels[i * mb:(i + 1) * mb])
                if not self._n1 and (not cfg.scatter_once or i == n_mb - 1):
                    with named_scope("scatter_grads"):
                        sp.xg.reduce_scatter_segments([(sp.full.g(n), sp.local.g(n)) for n in sp._xg_names],
                                                      accumulate=True)
                        for t in self._shard_full:
                            t.zero_()
            on.join()
            if k > 1:
                eng.merge()
            if not self._n1:
                sp.sync_replicated()
            st.tx.update(sp.local, st.opt_state, 1.0 / (n_mb * self.world))
            with named_scope("synch_metrics"):
                K.metrics_fold_(self.metrics, sp.local.metrics_slot)
            return
        for i in range(n_mb):
            if i == 0 or not cfg.gather_once:
                sp.gather()
            loss_and_grad(self.model, sp.full, batch.inputs[i * mb:(i + 1) * mb], batch.labels[i * mb:(i + 1) * mb],
                          train=True, seed=seed, offset=i << 16, step=st.step_tensor, grad_scale=1.0 / mb,
                          metrics=sp.local.metrics_slot)
            if not cfg.scatter_once:
                sp.scatter_grads(accumulate=True)
        if not (cfg.scatter_once and sp.scatter_grads(accumulate=False, with_replicated=True)):
            sp.sync_replicated()
        st.tx.update(sp.local, st.opt_state, 1.0 / (n_mb * self.world))
        with named_scope("synch_metrics"):
            K.metrics_fold_(self.metrics, sp.local.metrics_slot)

    def finalize(self):
        if self.fused is not None and (self._n1 or self.one_launch):
            self.fused.finalize()  # bf16 shadow parity of the in-epilogue AdamW
        if self.one_launch:
            # the owners updated the local fp32 masters in-kernel; their bf16 local shards
            # (what a later gather() moves) are refreshed from them
            self.sp.local.sync_shadow()
        if self.sp.xg is not None:
            self.sp.xg.raise_if_error()

    def close(self):
        """Release the IPC-mapped exchange buffers (tile exchange inboxes, the shards' xGMI
        context) and the captured graphs (see DataParallelTrainer.close; collective)."""
        from ..runtime.dist import quiesce_and_close

        quiesce_and_close(self.sp.local.master.device, self._txx, self.sp.xg)
        self._txx = self.sp.xg = None
        self.invalidate()

    def full_params(self) -> Dict[str, torch.Tensor]:
        """Gather the fp32 masters (for checks / checkpoints)."""
        out = {}
        for name, pt in self.sp.part.items():
            v = self.sp.local.p(name)
            d = pt.shard_dim
            out[name] = v.clone() if d is None else C.all_gather(v.contiguous(), self.mesh, self.cfg.axis, dim=d).clone()
        return out
