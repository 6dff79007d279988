"""The trainers' shared captured-step program (parallel/step_program.py) on the CPU:
the replay arithmetic of ``run_steps``, the static-batch bookkeeping, and that the
three real trainers define every attribute in ``__init__``."""
import types

import pytest
import torch

from jax_distributed_tuts_amd.parallel.step_program import CapturedStep
from jax_distributed_tuts_amd.utils.train_state import Batch


class _Graph:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def replay(self):
        self.log.append(self.name)


class _Ahead:
    def __init__(self, log):
        self.log = log

    def replay(self, S):
        self.log.append(S)


class _Engine:
    ahead_primed = True


class _Program(CapturedStep):
    """The shared base with counting "graphs" and a fake state."""

    def __init__(self, multi=None, ahead=False):
        super().__init__()
        self.state = types.SimpleNamespace(step=0)
        self.log, self.eager, self.engine = [], 0, _Engine()
        self._static = _batch(0)
        self.graph = ("one", _Graph(self.log, "g1"))
        if multi:
            self.multi = (multi, _Graph(self.log, "gm"))
        if ahead:
            self._ahead = _Ahead(self.log)

    def _eager_step(self, batch):
        self.eager += 1

    @property
    def _batch_engines(self):
        return (self.engine,)


def _batch(seed, rows=8):
    g = torch.Generator().manual_seed(seed)
    return Batch(torch.randn(rows, 4, generator=g), torch.randint(0, 10, (rows,), generator=g))


def test_run_steps_multi_then_single():
    p = _Program(multi=3)
    p.run_steps(p._static, 7)
    assert p.log == ["gm", "gm", "g1"] and p.state.step == 7 and p.eager == 0


def test_run_steps_ahead_graphs():
    p = _Program(multi=3, ahead=True)
    p.run_steps(p._static, 7)
    assert p.log == [3, 3, 1] and p.state.step == 7


def test_run_steps_without_multi():
    p = _Program()
    p.run_steps(p._static, 7)
    assert p.log == ["g1"] * 7 and p.state.step == 7


def test_uncaptured_steps_run_eagerly():
    p = _Program()
    p._drop_graphs()
    assert p.graph is None and p.multi is None and p._ahead is None
    p.run_steps(_batch(1), 3)   # no graph: any batch
    assert p.log == [] and p.eager == 3 and p.state.step == 3


def test_static_batch():
    p = _Program(multi=2)
    b, other = p._static, _batch(1)
    with pytest.raises(ValueError, match="set_batch"):
        p.step(other)
    with pytest.raises(ValueError, match="set_batch"):
        p.run_steps(other, 4)
    assert p.log == [] and p.state.step == 0
    p.step(Batch(b.inputs, b.labels))   # the captured storage under another Batch object
    assert p.log == ["g1"]
    p.set_batch(other)
    assert torch.equal(b.inputs, other.inputs) and torch.equal(b.labels, other.labels)
    assert p._static is b and p.engine.ahead_primed is False
    with pytest.raises(ValueError, match="shapes"):
        p.set_batch(_batch(2, rows=4))


# ----------------------------------------------------------------------------- the real trainers
def _dp():
    from jax_distributed_tuts_amd.models.mlp import Classifier
    from jax_distributed_tuts_amd.parallel.dp import DataParallelTrainer, DPConfig, init_dp
    from jax_distributed_tuts_amd.utils.train_state import adamw

    return DataParallelTrainer(init_dp(Classifier(), adamw(1e-3), 69, "cpu"), None, DPConfig(4, "loop"))


def _fsdp():
    from jax_distributed_tuts_amd.models.mlp import Classifier
    from jax_distributed_tuts_amd.parallel.fsdp import FSDPConfig, FSDPTrainer, init_fsdp
    from jax_distributed_tuts_amd.utils.train_state import adamw

    return FSDPTrainer(init_fsdp(Classifier(), adamw(1e-3), 69, "cpu", None), None, FSDPConfig())


def _gpipe():
    from pipeline_parallel import pp_mlp_dims
    from jax_distributed_tuts_amd.models.mlp import MLP
    from jax_distributed_tuts_amd.parallel.pipeline import GPipeTrainer, PipeConfig, init_stage_params, mlp_stage
    from jax_distributed_tuts_amd.utils import rng as R
    from jax_distributed_tuts_amd.utils.config import dp_config
    from jax_distributed_tuts_amd.utils.train_state import TrainState, adamw

    cfg = dp_config()
    dims = pp_mlp_dims(cfg, 3)
    stage = mlp_stage(dims, 1, 0)
    P = init_stage_params(stage, MLP(dims).param_specs(), cfg.seed, "cpu")
    st = TrainState.create(apply_fn=stage, params=P, tx=adamw(1e-3), rng=R.PRNGKey(cfg.seed))
    return GPipeTrainer(st, None, PipeConfig(4))


@pytest.fixture(scope="module")
def mnist_batch():
    from data_paral import synthetic_batch
    from jax_distributed_tuts_amd.utils.config import dp_config

    return synthetic_batch(dp_config(), 70)


@pytest.mark.parametrize("make", [_dp, _fsdp, _gpipe])
def test_invalidate_drops_the_captured_program(make):
    tr = make()
    assert tr.graph is None and tr.multi is None and tr._ahead is None and tr._static is None
    tr.graph, tr.multi, tr._ahead = ("one", "stale"), (4, "stale"), "stale"
    tr.invalidate()
    assert tr.graph is None and tr.multi is None and tr._ahead is None


@pytest.mark.parametrize("make", [_dp, _fsdp, _gpipe])
def test_every_attribute_is_set_in_init(make, mnist_batch):
    tr = make()
    at_init = set(vars(tr))
    tr.step(mnist_batch)
    tr.invalidate()
    tr.step(mnist_batch)
    assert set(vars(tr)) - at_init == set()
    assert tr.state.step == 2
