"""Autoregressive generation for the transformer LM: a KV cache, a prefill through the
training forward and a decode step of one token per sequence.

Cache layout: per layer K and V are ``[B, H, seq_len, 64]`` bf16 (a head's keys are
contiguous 128-byte rows), ``tokens`` is ``int32 [B, seq_len]`` and ``pos`` is a device
``int32[1]``: the number of tokens already in the cache, which is also the index of the
token the next step processes.  Every kernel of a step reads ``pos`` from memory and the
sampler -- the step's last launch -- advances it, so one captured step replays for every
token without host bookkeeping.  A step past the end of the cache writes nothing.

Prefill convention: ``prefill(prompt)`` runs the training forward once over the prompt
padded to ``seq_len`` (causal attention makes rows < P independent of the padding),
copies rows < P of every layer's k / v into the cache and sets ``pos = P - 1``: the first
decode step re-processes the last prompt token (rewriting cache row P - 1 with its own
k / v) and samples token P from it.

Out of scope: ragged prompt lengths within a batch, top-k / top-p and beam search,
sequences longer than ``seq_len`` (the learned positions end there), multi-GPU or
pipeline-split generation, and head dims other than 64 on the HIP path.
"""
from __future__ import annotations

from typing import Optional

import torch

from .models.transformer import TransformerConfig, TransformerLM
from .ops import kernels as K
from .parallel.step_program import capture_graph
from .utils.flat import FlatParams


class KVCache:
    """Per-layer K / V ``[B, H, seq_len, Dh]`` bf16, ``tokens`` int32 ``[B, seq_len]``, the
    device position word ``pos`` int32[1] and ``o``, the decode step's attention output
    ``[B, d_model]`` bf16 (one buffer, reused layer after layer)."""

    def __init__(self, cfg: TransformerConfig, batch: int, device):
        H, Dh = cfg.n_heads, cfg.d_model // cfg.n_heads
        mk = lambda: torch.zeros(batch, H, cfg.seq_len, Dh, dtype=torch.bfloat16, device=device)  # noqa: E731
        self.k = [mk() for _ in range(cfg.n_layers)]
        self.v = [mk() for _ in range(cfg.n_layers)]
        self.tokens = torch.zeros(batch, cfg.seq_len, dtype=torch.int32, device=device)
        self.pos = torch.zeros(1, dtype=torch.int32, device=device)
        # attention output of the layer in flight (a step past the end leaves it as it is)
        self.o = torch.zeros(batch, cfg.d_model, dtype=torch.bfloat16, device=device)


class Generator:
    """Generation with a full (un-split) ``TransformerLM`` and its parameters ``P`` for a
    fixed batch of ``batch`` sequences on ``device``."""

    def __init__(self, model: TransformerLM, P: FlatParams, batch: int, device):
        if not (model.has_embed and model.has_head and list(model.layers) == list(range(model.cfg.n_layers))):
            raise ValueError("Generator needs the full model (embedding, every layer and the head): "
                             "pipeline-split stages cannot generate")
        self.model, self.P, self.batch, self.device = model, P, int(batch), torch.device(device)
        self.kv = KVCache(model.cfg, self.batch, self.device)
        self.x = torch.zeros(self.batch, model.cfg.d_model, dtype=torch.bfloat16, device=self.device)
        self.temperature, self.seed = 0.0, 0
        self.logits: Optional[torch.Tensor] = None   # the last step's logits [B, vocab]
        self._graphs: dict = {}                      # (temperature, seed) -> (graph, its logits)

    # ------------------------------------------------------------------ prefill
    def prefill(self, prompt: torch.Tensor):
        """``prompt`` int [B, P], 1 <= P <= seq_len: fills cache rows < P and sets pos = P - 1."""
        c = self.model.cfg
        if prompt.dim() != 2 or prompt.shape[0] != self.batch or not 1 <= prompt.shape[1] <= c.seq_len:
            raise ValueError(f"prompt must be [{self.batch}, 1..{c.seq_len}], got {tuple(prompt.shape)}")
        if int(prompt.min()) < 0 or int(prompt.max()) >= c.vocab_size:
            raise ValueError(f"prompt token outside [0, {c.vocab_size})")
        B, Pn, H, Dh = self.batch, prompt.shape[1], c.n_heads, c.d_model // c.n_heads
        kv = self.kv
        kv.tokens.zero_()
        kv.tokens[:, :Pn] = prompt.to(device=self.device, dtype=torch.int32)
        _, cache = self.model.forward(self.P, kv.tokens)
        for l, bc in zip(self.model.layers, cache.blocks):
            qkv = bc.qkv.view(B, c.seq_len, 3, H, Dh)
            kv.k[l][:, :, :Pn] = qkv[:, :Pn, 1].permute(0, 2, 1, 3)
            kv.v[l][:, :, :Pn] = qkv[:, :Pn, 2].permute(0, 2, 1, 3)
        kv.pos.fill_(Pn - 1)

    # ------------------------------------------------------------------ one step
    def step(self, sample: bool = True) -> torch.Tensor:
        """One decode step at position ``pos``; returns its logits [B, vocab].  ``sample``:
        the sampler writes ``tokens[:, pos + 1]`` and advances ``pos`` (temperature / seed:
        the attributes of that name).  ``sample=False`` (teacher forcing): ``tokens`` is left
        alone and ``pos`` advances by a torch op."""
        kv, P = self.kv, self.P
        K.embed_decode(kv.tokens, P.s("embed/wte"), P.s("embed/wpe"), kv.pos, out=self.x)
        self.logits = self.model.decode_step(P, kv, self.x)
        if sample:
            K.sample_tokens(self.logits, kv.tokens, kv.pos, temperature=self.temperature, seed=self.seed)
        else:
            kv.pos.add_(1)
        return self.logits

    def _replay(self):
        """The sampling step as a graph replay (captured on first use per sampler setting;
        one stream, no parallel branches).  The eager step before the capture is a real
        step: it also creates every lazily allocated workspace outside the capture."""
        key = (self.temperature, self.seed)
        ent = self._graphs.get(key)
        if ent is None:
            eager = self.step()
            torch.cuda.synchronize(self.device)
            g = capture_graph(self.step)   # records only: nothing runs, pos and the cache stay
            self._graphs[key] = (g, self.logits)
            self.logits = eager
            return
        g, logits = ent
        if g is None:   # the capture was refused: stay eager
            self.step()
            return
        g.replay()
        self.logits = logits

    # ------------------------------------------------------------------ generate
    def generate(self, prompt: torch.Tensor, max_new_tokens: int, temperature: float = 0.0, seed: int = 0,
                 capture: bool = True) -> torch.Tensor:
        """``prompt`` int [B, P] -> int32 [B, P + max_new_tokens] (the prompt, then the new
        tokens).  ``temperature == 0``: greedy; otherwise softmax(logits / T) sampling from
        Philox stream ``seed``.  ``capture`` (GPU only): the decode step is captured into a
        graph once and replayed per token."""
        c = self.model.cfg
        Pn = prompt.shape[1] if prompt.dim() == 2 else 0
        if max_new_tokens < 0 or Pn + max_new_tokens > c.seq_len:
            raise ValueError(f"prompt length {Pn} + max_new_tokens {max_new_tokens} exceeds seq_len {c.seq_len} "
                             "(the learned positions end there)")
        self.prefill(prompt)
        self.temperature, self.seed = float(temperature), int(seed)
        graph = capture and self.device.type == "cuda"
        for _ in range(max_new_tokens):
            if graph:
                self._replay()
            else:
                self.step()
        return self.kv.tokens[:, :Pn + max_new_tokens].clone()
