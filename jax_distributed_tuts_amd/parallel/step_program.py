"""The captured step program shared by the three trainers (DP, FSDP, GPipe).

A trainer's step is recorded once as a hipGraph (``capture_graph``), optionally with
an S-step variant -- S sequential steps in one graph, or the run-ahead graphs of a
whole-step fused engine (``fused_mlp.AheadGraphs``) -- and then replayed:
``run_steps(batch, n)`` = n // S multi-step replays + n % S single ones.
``CapturedStep`` owns that state (``graph``, ``multi``, ``_ahead``, ``_static``) and
nothing else; what a trainer records, and which engine may run ahead, stay with the
trainer.  Also here: the stream plumbing of the per-minibatch schedules
(``hw_queues``, ``_MbStreams``, ``mb_streams``).
"""
from __future__ import annotations

import contextlib
import logging
import os
from typing import Optional

import torch

from ..utils.profiling import replay_scope
from ..utils.train_state import Batch, check_static_batch, load_static_batch


def hw_queues() -> int:
    """HIP hardware queues per process (GPU_MAX_HW_QUEUES; HIP's default is 4), the cap
    on concurrent-stream schedules.  ``JDT_HWQ_CAP=0`` lifts the cap (diagnosis of the
    more-streams-than-queues case, tools/sessions/gpu_r4_hwq.sh)."""
    if os.environ.get("JDT_HWQ_CAP", "1") == "0":
        return 1 << 10
    try:
        return max(1, int(os.environ.get("GPU_MAX_HW_QUEUES", "4")))
    except ValueError:
        return 4


class _MbStreams:
    """``with on(i)``: run work item i on stream i % k (item 0, k, 2k, ... on the main
    stream); ``fork``: the side streams wait for the main stream's work so far;
    ``join``: the main stream waits for the side streams.  ``main=None``: one stream."""

    def __init__(self, main, side):
        self.main, self.side = main, side or []

    def fork(self):
        for s in self.side:
            s.wait_stream(self.main)

    def join(self):
        for s in self.side:
            self.main.wait_stream(s)

    def __call__(self, i: int):
        k = len(self.side) + 1
        return torch.cuda.stream(self.side[i % k - 1]) if (self.side and i % k) else contextlib.nullcontext()


def mb_streams(have, k: int, device) -> _MbStreams:
    """The k-stream schedule on ``device``'s current stream.  Its k - 1 side streams
    are ``have`` when that already is such a list (the owner keeps ``.side`` across
    steps: a captured graph replays on them), else new ones; k <= 1: one stream."""
    if k <= 1:
        return _MbStreams(None, None)
    if have is None or len(have) != k - 1:
        have = [torch.cuda.Stream(device) for _ in range(k - 1)]
    return _MbStreams(torch.cuda.current_stream(device), have)


def capture_graph(body, pool=None) -> Optional[torch.cuda.CUDAGraph]:
    """``body`` recorded into a hipGraph, or None if a collective in it refused stream
    capture (the caller then keeps that collective eager).  RCCL collectives enqueue
    on the capturing stream and are recorded like kernels."""
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g, pool=pool):
            body()
    except RuntimeError as e:
        logging.getLogger(__name__).warning("step capture with the collective inside failed (%s); "
                                            "running the collective eagerly between graphs", e)
        torch.cuda.synchronize()
        return None
    return g


class CapturedStep:
    """Mixin of a trainer with ``state`` (a TrainState) and ``_eager_step(batch)`` (one
    step's device work, no host counter).

    ``graph``: None, or a tuple whose [0] names its form ("one": the whole step in
    graph[1]) and whose [1] is a graph; ``multi``: None or (S, S-step graph);
    ``_ahead``: None or the AheadGraphs both of them came from; ``_static``: the batch
    the graphs read."""

    scope = "train_step"    # the replays' profiler range (utils.profiling.replay_scope)

    def __init__(self):
        self.graph = self.multi = self._ahead = self._static = None

    def _drop_graphs(self):
        self.graph = self.multi = self._ahead = None

    @property
    def _batch_engines(self) -> tuple:
        """The engines whose run-ahead forward a new batch makes stale (``set_batch``)."""
        return ()

    # ------------------------------------------------------------------ capture
    def _capture(self, body, batch: Batch, steps_per_graph: int = 1, ahead=None, multi_body=None) -> bool:
        """Record ``body`` (one step on ``batch``) as the 1-step graph; False if a
        collective in it refused capture.  ``ahead()`` (evaluated after that capture,
        which may have built the engine) is an engine that can run ahead, or None: with
        one, the graphs are its AheadGraphs; without, ``steps_per_graph`` > 1 records
        that many bodies -- or ``multi_body()``, when given and it returns True -- into a
        second graph in the same pool."""
        self._static = batch
        self._drop_graphs()
        g = capture_graph(body)
        if g is None:
            return False
        self.graph = ("one", g)
        S = int(steps_per_graph)
        eng = ahead() if ahead is not None else None
        if eng is not None:
            from .fused_mlp import AheadGraphs

            self._ahead = AheadGraphs(eng, batch, S, pool=g.pool())
            if S > 1:
                self.multi = (S, self._ahead.graph(S))
        elif S > 1:
            gm = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gm, pool=g.pool()):
                if not (multi_body is not None and multi_body()):
                    for _ in range(S):
                        body()
            self.multi = (S, gm)
        return True

    # ------------------------------------------------------------------ replay
    def _replay(self, S: int = 1):
        """One replay of the S-step program (S = 1, or multi's S)."""
        with replay_scope(self.scope, S):
            if self._ahead is not None:
                self._ahead.replay(S)
            else:
                (self.graph if S == 1 else self.multi)[1].replay()

    def step(self, batch: Batch):
        if self.graph is not None:
            check_static_batch(self._static, batch)
            self._replay()
        else:
            self._eager_step(batch)
        self.state.step += 1

    def run_steps(self, batch: Batch, n: int):
        """n training steps; with a multi-step graph, n // S replays of it plus
        single-step replays for the remainder."""
        if self.graph is not None and self.multi is not None:
            check_static_batch(self._static, batch)
            S = self.multi[0]
            for _ in range(n // S):
                self._replay(S)
            self.state.step += (n // S) * S
            n %= S
        for _ in range(n):
            self.step(batch)

    def set_batch(self, batch: Batch):
        """New data for captured graphs: copied into the captured batch tensors (the
        run-ahead schedule's next forward, computed from the old contents, is redone)."""
        if self._static is not None:
            load_static_batch(self._static, batch, self._batch_engines)
