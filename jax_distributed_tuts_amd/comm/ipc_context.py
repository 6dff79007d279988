"""The lifecycle of a comm context whose device buffers the peers map over IPC.

``XgmiComm`` (comm/xgmi.py), ``XgmiP2P`` (comm/p2p.py) and ``TileExchange``
(comm/tile_exchange.py) are built and torn down by one protocol, collective over
their process group:

  build     every rank creates its buffers and exports their IPC handles, the handles
            are all-gathered, every rank maps its peers' buffers, and the ranks agree
            (MIN all-reduce) that all of it worked everywhere -- ``_handshake``;
  teardown  every rank unmaps its peers' buffers, a barrier, then every rank releases
            its own: no peer mapping outlives the pages it resolves to
            (comm/csrc/ipc_pool.hip) -- ``close``.

The subclasses keep what is theirs: argument checks, self-tests, kernel entry points.
"""
from __future__ import annotations

import contextlib
import ctypes
import logging
from ctypes import c_void_p

import torch
import torch.distributed as dist

log = logging.getLogger(__name__)

HANDLE_BYTES = 64   # sizeof(hipIpcMemHandle_t)


def agree(group, ok: bool, device) -> bool:
    """AND of ``ok`` over ``group`` (collective; on the device for nccl, else on the CPU)."""
    t = torch.tensor([1 if ok else 0], dtype=torch.int32,
                     device=device if dist.get_backend(group) == "nccl" else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MIN, group=group)
    return bool(int(t.item()))


def ipc_teardown_barrier(group):
    """The barrier between the two phases of a comm context's teardown: every rank of
    ``group`` has closed its mappings of the peers' buffers before any rank releases its
    own (a gloo group's barrier runs on the host; nccl's on the device)."""
    if group is None or not dist.is_initialized():
        return
    if dist.get_backend(group) == "nccl":
        from ..runtime.dist import device

        dist.barrier(group=group, device_ids=[device().index])
    else:
        dist.barrier(group=group)


class IpcContext:
    """``group`` / ``rank`` / ``world`` / ``device``, the native context ``ctx`` (null
    when closed) and ``ok``.  Subclasses provide ``_unmap()`` and ``_destroy()``."""

    def __init__(self, group, rank: int, world: int, device):
        self.group, self.rank, self.world, self.device = group, rank, world, device
        self.ctx = c_void_p()
        self.ok = False

    def _agree(self, ok: bool) -> bool:
        return agree(self.group, ok, self.device)

    def _on_device(self):
        dev = torch.device(self.device)
        return torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()

    def _handshake(self, create, open_, n_handles: int, tag: str) -> bool:
        """``create(handles_out)`` (sets ``self.ctx``) and ``open_(all_handles)`` return 0
        on success; each exports / takes ``n_handles`` 64-byte handles per rank, rank-major.
        True on every rank iff both worked on every rank."""
        h = (ctypes.c_char * (n_handles * HANDLE_BYTES))()
        with self._on_device():
            rc = create(h)
        objs = [None] * self.world
        dist.all_gather_object(objs, bytes(h) if rc == 0 else None, group=self.group)
        good = all(o is not None for o in objs)
        if good:
            allh = b"".join(objs)
            with self._on_device():
                rc = open_(ctypes.create_string_buffer(allh, len(allh)))
            good = rc == 0
            if not good:
                log.warning("%s: hipIpcOpenMemHandle failed on rank %d (rc %d)", tag, self.rank, rc)
        else:
            log.warning("%s: buffer export failed on some rank (rank %d rc %d)", tag, self.rank, rc)
        return self._agree(good)

    def _finish(self, good: bool):
        """The constructor's end: ``ok``, or the context closed again (collective: the
        verdict is the same on every rank)."""
        self.ok = good
        if not good:
            self.close()

    def close(self, collective: bool = True):
        """Two-phase teardown (collective over the context's group).
        ``collective=False`` (garbage collection): one phase, this rank only."""
        if self.ctx:
            if collective:
                self._unmap()
                ipc_teardown_barrier(self.group)
            # (one phase: exported buffers go back with no barrier -- the open finding on ipc_pool.hip's GC path)
            self._destroy()
            self.ctx = c_void_p()
        self.ok = False
