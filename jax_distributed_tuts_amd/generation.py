"""Autoregressive generation for the transformer LM: a KV cache, a prefill through the
training forward or in chunks straight into the cache, and a decode step of one token per
sequence.

Cache layout: per layer K and V are ``[B, H, seq_len, 64]`` bf16 (a head's keys are
contiguous 128-byte rows; "FP8 cache" below: 64-byte rows and a scale), ``tokens`` is ``int32 [B, seq_len]`` and ``pos`` is a device
``int32[1]``: the number of tokens already in the cache, which is also the index of the
token the next step processes.  Every kernel of a step reads ``pos`` from memory and the
sampler -- the step's last launch -- advances it, so one captured step replays for every
token without host bookkeeping.  A step past the end of the cache writes nothing.

Prefill convention: ``prefill(prompt)`` runs the training forward once over the prompt
padded to ``seq_len`` (causal attention makes rows < P independent of the padding),
copies rows < P of every layer's k / v into the cache and sets ``pos = P - 1``: the first
decode step re-processes the last prompt token (rewriting cache row P - 1 with its own
k / v) and samples token P from it.  With ``seq_len > 128`` the forward runs over the prompt
padded to the next multiple of 128 only (``Generator.prefill_rows``), not over the whole cache.

Long caches: the decode attention is one launch up to 128 cache rows and, for ``128 < seq_len
<= 32768``, a split-KV pair of launches (one workgroup per 128-key chunk, then a combine;
``KVCache.split_ws`` holds the partials).  Both read ``pos`` on the device and their grids
depend on the cache's shape only, so the captured step replays at every depth.

Ragged batches: ``prefill(prompt, prompt_lens)`` / ``generate(..., prompt_lens=, eos_id=)``
switch the cache to its per-row state, ``pos_rows`` int32[B] and ``end`` int32[B] (one past
the last token index a row may hold).  The same kernels then read ``pos[b]``; the sampler
advances row b while ``pos[b] + 1 < end[b]`` and, for a drawn ``eos_id``, sets ``end[b]`` to
the row's length, which finishes it: its later steps re-process the same token (the same
bits) and sample nothing, so the captured step still replays without host bookkeeping.
The sampler can also be restricted to the top-k / top-p set (``ops.kernels.sample_tokens``).

Appending to the cache: ``advance`` pushes a block of tokens already in ``tokens`` through the
blocks in slices of at most ``chunk`` rows -- ``embed_append``, then ``TransformerLM.append_chunk``
with ``ops.kernels.attention_append`` (csrc/attn_append.hip: causal attention of C new query
rows against the cache in the cache's own layout, one launch per layer) -- with no backward
cache and no logits it does not need.  ``prefill(prompt, chunk=c)`` (``generate(...,
prefill_chunk=c)``) fills the cache that way instead of through the training forward, and leaves
the same position.  ``extend(tokens)`` appends to a live cache: a second turn after a generation,
teacher forcing a block of tokens, or scoring a continuation (``logits=True``).  The bits a
token's attention output gets do not depend on how the tokens were cut into calls or slices.

Split append (``Generator(..., split_append=True)``, opt-in): a slice of a few rows against a deep
cache is, in the one launch, a handful of workgroups that each walk the whole cache below their
query tile.  The split pair of launches gives every 512-key span of absolute cache rows a
workgroup of its own per query tile and folds the spans' partials in a combine launch, the way
the split-KV decode does for one query; ``KVCache.append_ws`` holds the partials, ``advance``
sizes it for its largest slice before the loop (from ``n`` and ``chunk``: the position is not read)
and every layer reuses it.  The caches are bit for bit the one launch's, tokens below row 512 get
its bits, and the bits of a deeper token still do not depend on how the tokens were cut.

Beam search: ``beam_search(prompt [G, P], n, num_beams=W)`` on a generator of batch G * W keeps W
hypotheses per prompt; batch row g * W + j is beam slot j of group g, and the position is the shared
one.  A step is the decode step above followed by two launches of csrc/beam.hip instead of the
sampler: ``ops.kernels.beam_topw`` (per row: fp32 log-softmax and the W largest logits, or the single
candidate of a finished beam) and ``ops.kernels.beam_reorder`` (per group the W best of the
candidates by score, then source slot, then rank; then every layer's cache rows 0..pos and
``tokens[:, 0..pos]`` of the new slots become their parents', permuted in place, the new tokens go to
``tokens[:, pos + 1]`` and ``pos`` advances).  The beam state (``BeamState``) lives on the device and
both launches read ``pos`` there, so the captured beam step replays for every token too.

Speculative decoding: ``Generator(..., draft=(draft_model, draft_P))`` and ``generate(..., speculative=k)``
emit up to k + 1 tokens per verify pass.  The draft is a second ``Generator`` (a full ``TransformerLM`` of
the same vocabulary and ``seq_len``, any depth or width) whose ``KVCache.tokens`` IS the target's tensor.
A round (``spec_step(k)``): k greedy per-row draft steps write draft i straight to ``tokens[b, dpos + 1]``;
``ops.kernels.spec_count`` turns the number drafted into the row's ``count`` = 1 + drafts; one more draft
step without sampling caches the last draft's row; then ``verify``: ``embed_append`` and
``append_chunk(count=count, head=True)`` score the C = k + 1 tokens from ``pos`` on in one append slice,
``ops.kernels.spec_judge`` (csrc/spec.hip, one workgroup per logits row) decides per draft and
``ops.kernels.spec_commit`` keeps the longest agreed prefix plus one token of the target's own, advances
``pos_rows`` / ``end`` and sets the drafter's position back to the target's.  Greedy stays greedy and
sampling stays softmax sampling under the same top-k / top-p filter: the drafts are deterministic, a
point mass, so "accept d with probability p(d), else redraw from p without d" is the exact rule.  All of
a round's state (``SpecState``, the per-row cache state) is read on the device, so one captured round
replays with no host bookkeeping.  Invariant: rejected drafts leave their k / v rows in both caches at
rows >= ``pos``; those rows are rewritten before they are read, because the next round (or step) appends
from ``pos``.  ``verify(count)`` is the round without the drafter, for drafts the caller wrote into
``kv.tokens``: the hook for other drafters.

FP8 cache (``Generator(..., kv_dtype="fp8")``, opt-in; bf16 is untouched): K and V are stored as OCP e4m3
bytes with one fp32 scale per cache row -- the 64 values of one (batch, head, token) of K or of V -- so a
row takes 68 bytes against 128 (``KVCache.k`` / ``.v`` uint8 ``[B, H, seq_len, 64]``, ``.k_scale`` /
``.v_scale`` fp32 ``[B, H, seq_len]``).  The format (``ops.kernels.kv_quantize`` is its definition, and the
cache bytes are reproducible bit for bit on any device): ``amax = max |x|``, ``e = floor(log2(amax))``
taken from amax's exponent bits and clamped to [-120, 127] (7 for a zero row), ``scale = 2^(e - 7)``,
``q = e4m3fn(x * 2^(7 - e))`` rounded to nearest even.  The scale is a power of two, so the product is exact,
the row's largest scaled magnitude lies in [128, 256) -- nothing reaches 448, no saturation -- and the
dequantized ``float(q) * scale`` is exact in fp32 and exactly a bf16, within ``amax / 16`` of ``x``.
Semantics: attention always sees the dequantized row.  The decode step quantizes the token's k / v, writes
them and uses them as they will be read back; the append kernel does the same for the keys of its own
chunk.  So the invariant above survives: the bits of token t's attention output depend only on ``(q_t,
K[0..t], V[0..t])``, not on how the tokens were cut into calls.  The one exception is the default
``prefill`` through the training forward: there the prompt rows attend over unquantized bf16 keys and only
the cache is quantized (one launch of ``ops.kernels.kv_cache_fill`` per layer in the place of the two
permute-copies) -- the usual arrangement; ``prefill(chunk=)`` has no such exception.  ``prefill`` in both
forms, ``advance``, ``extend``, ``step`` and ``generate`` (shared and per-row positions, sampler filters, EOS,
capture) run on an FP8 cache of up to 32768 rows through the ``_fp8`` launchers of csrc/attn_decode.hip and
csrc/attn_append.hip, with the bf16 path's launches, chunks and workspaces; ``split_append=True``,
``draft=`` and ``beam_begin`` / ``beam_search`` raise ``ValueError``.

Out of scope: FP8 caches with beams, speculative decoding or split append, per-channel or per-tensor
scales, e5m2, FP8 MFMA for Q K^T, quantized weights, sampled drafts with a q / p ratio test, n-gram / prompt-lookup or tree drafters (``verify``
is the hook for them), speculative beams, continuing speculation after ``extend``, a draft with another
vocabulary, adapting k per row or per round, beams over ragged prompts (per-row positions), diverse or
constrained beam search, a beam cache that re-routes through an indirection table instead of copying,
sharing the prompt's cache rows between the beams of a group, repetition penalties, sequences longer than ``seq_len`` (the
learned positions end there), multi-GPU or pipeline-split generation, paged or compacted
caches, ``generate()`` continuing a live cache, split append as the default, a span size chosen
per shape (the spans are absolute so that the cut does not change the bits), removing finished
rows from the batch, and head dims other than 64 or caches past 32768 rows on the HIP path.
Chunked prefill is opt-in: the default ``prefill`` is still the training forward.
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import torch

from .models.transformer import TransformerConfig, TransformerLM
from .ops import kernels as K
from .parallel.step_program import capture_graph
from .utils.flat import FlatParams


KV_DTYPES = ("bf16", "fp8")


class KVCache:
    """Per-layer K / V ``[B, H, seq_len, Dh]`` bf16, ``tokens`` int32 ``[B, seq_len]``, the
    device position word ``pos`` int32[1] and ``o``, the decode step's attention output
    ``[B, d_model]`` bf16 (one buffer, reused layer after layer).  The per-row state is
    ``pos_rows`` int32[B] and ``end`` int32[B] (one past the last token index a row may hold);
    ``per_row`` says which position tensor is live (``live_pos``): ``pos`` by default.
    ``split_ws``: the split-KV decode attention's partials, fp32 ``[B * H, ceil(seq_len / 128),
    66]`` (one buffer, reused layer after layer), or ``None`` when ``seq_len <= 128``.
    ``append_ws``: the split-KV append attention's partials, flat fp32 of at least
    ``ops.kernels.attention_append_ws_floats(B, H, C, seq_len)`` words for the largest slice size C
    appended so far (one buffer, reused layer after layer), or ``None``: ``append_chunk`` then runs the
    one-launch kernel.  Only ``Generator(split_append=True)`` allocates it, on first use and again
    when a larger slice needs more.  Size: 16.5 KiB (64 rows x 66 words) per (batch x head, 64-row
    query tile, 512-key span) -- 8.3 MiB at B = 1, H = 8, chunk 64 and ``seq_len`` 32768, and it
    scales with the chunk and the batch.
    ``kv_dtype="fp8"``: ``k`` / ``v`` are uint8 (e4m3 bytes, 64 per row) and ``k_scale`` / ``v_scale`` hold
    per layer the rows' scales, fp32 ``[B, H, seq_len]`` initialised to 1 -- 68 bytes per row against 128.
    ``"bf16"``: ``k_scale`` / ``v_scale`` are ``None``."""

    def __init__(self, cfg: TransformerConfig, batch: int, device, kv_dtype: str = "bf16"):
        if kv_dtype not in KV_DTYPES:
            raise ValueError(f"kv_dtype must be one of {KV_DTYPES}, got {kv_dtype!r}")
        H, Dh = cfg.n_heads, cfg.d_model // cfg.n_heads
        self.kv_dtype = kv_dtype
        fp8 = kv_dtype == "fp8"
        if fp8 and Dh != K.KV_ROW:
            raise ValueError(f"an FP8 cache needs head dim {K.KV_ROW} (the quantized row), got {Dh}")
        mk = lambda: torch.zeros(batch, H, cfg.seq_len, Dh, dtype=torch.uint8 if fp8 else torch.bfloat16,  # noqa: E731
                                 device=device)
        self.k = [mk() for _ in range(cfg.n_layers)]
        self.v = [mk() for _ in range(cfg.n_layers)]
        # FP8: one fp32 power-of-two scale per cache row (1: the scale of a zero row)
        sc = lambda: torch.ones(batch, H, cfg.seq_len, dtype=torch.float32, device=device)  # noqa: E731
        self.k_scale = [sc() for _ in range(cfg.n_layers)] if fp8 else None
        self.v_scale = [sc() for _ in range(cfg.n_layers)] if fp8 else None
        self.tokens = torch.zeros(batch, cfg.seq_len, dtype=torch.int32, device=device)
        self.pos = torch.zeros(1, dtype=torch.int32, device=device)
        self.pos_rows = torch.zeros(batch, dtype=torch.int32, device=device)
        self.end = torch.full((batch,), cfg.seq_len, dtype=torch.int32, device=device)
        self.per_row = False
        # attention output of the layer in flight (a step past the end leaves it as it is)
        self.o = torch.zeros(batch, cfg.d_model, dtype=torch.bfloat16, device=device)
        self.split_ws: Optional[torch.Tensor] = None
        if cfg.seq_len > K.AD_CHUNK_ROWS:
            chunks = (cfg.seq_len + K.AD_CHUNK_ROWS - 1) // K.AD_CHUNK_ROWS
            self.split_ws = torch.zeros(batch * H, chunks, K.AD_SLOT_FLOATS, dtype=torch.float32, device=device)
        self.append_ws: Optional[torch.Tensor] = None
        self._history_ptrs = None

    @property
    def live_pos(self) -> torch.Tensor:
        return self.pos_rows if self.per_row else self.pos

    def cache_bytes(self) -> int:
        """Bytes of every layer's K and V with their scales: 2 * L * B * H * seq_len * 128 for bf16, * 68 for FP8."""
        ts = self.k + self.v + (self.k_scale or []) + (self.v_scale or [])
        return sum(t.numel() * t.element_size() for t in ts)

    def history_ptrs(self):
        """``ops.kernels.cache_ptr_table`` of every layer's K, then V: the table the beam reorder's one
        launch walks.  Built on first use and kept (the cache tensors are never reallocated)."""
        if self._history_ptrs is None:
            self._history_ptrs = K.cache_ptr_table(self.k + self.v)
        return self._history_ptrs


class BeamState:
    """The device state of a beam search over ``batch`` = G * W rows: per slot ``score`` (fp32, the sum
    of the chosen tokens' log-probabilities), ``done`` and ``length`` (int32, generated tokens), the
    last step's ``parent`` (the slot 0..W-1 of the same group whose history the slot continues) and
    ``token``, and the stage-1 candidate scratch ``cand`` = (token int32 [B, 8], score fp32 [B, 8])."""

    def __init__(self, batch: int, W: int, device):
        self.W, self.G, self.eos_id = W, batch // W, -1
        i32 = lambda: torch.zeros(batch, dtype=torch.int32, device=device)  # noqa: E731
        self.score = torch.zeros(batch, dtype=torch.float32, device=device)
        self.done, self.length, self.parent, self.token = i32(), i32(), i32(), i32()
        self.cand = (torch.full((batch, K.BEAM_MAX_W), -1, dtype=torch.int32, device=device),
                     torch.full((batch, K.BEAM_MAX_W), float("-inf"), dtype=torch.float32, device=device))

    def reset(self, eos_id: int):
        """Slot 0 of each group at score 0, the others at -inf: the first step fans out from one beam."""
        self.eos_id = eos_id
        self.score.fill_(float("-inf"))
        self.score.view(self.G, self.W)[:, 0] = 0.0
        for t in (self.done, self.length, self.parent, self.token):
            t.zero_()


class SpecState:
    """The device state of speculative rounds of ``k`` drafts over ``batch`` rows: ``count`` (tokens a row
    appends this round: 1 + its drafts; 0: the row sits the round out), ``n_drafted``, the judge's
    scratch ``acc`` / ``repl`` int32 [B, k + 1], and the counters ``drafted`` / ``accepted`` / ``emitted``
    (sums over the rounds since ``reset``) and ``last_accept`` (drafts kept in the row's last round)."""

    def __init__(self, batch: int, k: int, device):
        self.k, self.C = k, k + 1
        i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=device)  # noqa: E731
        self.count, self.n_drafted = i32(batch), i32(batch)
        self.acc, self.repl = i32(batch, self.C), i32(batch, self.C)
        self.drafted, self.accepted, self.emitted, self.last_accept = i32(batch), i32(batch), i32(batch), i32(batch)

    def reset(self):
        for t in (self.drafted, self.accepted, self.emitted, self.last_accept):
            t.zero_()


SPEC_CHECK_ROUNDS = 4   # speculative generate reads "every row finished" on the host this often (untuned)


class Generator:
    """Generation with a full (un-split) ``TransformerLM`` and its parameters ``P`` for a
    fixed batch of ``batch`` sequences on ``device``.  ``split_append`` (opt-in): everything that
    appends to the cache -- ``prefill(chunk=)``, ``extend``, ``generate(prefill_chunk=)``,
    ``beam_search(prefill_chunk=)`` -- runs the split-KV append attention (``KVCache.append_ws``
    holds its partials) instead of the one-launch kernel.  ``draft`` = (draft_model, draft_P): the
    drafter of speculative decoding, a full ``TransformerLM`` of the same ``vocab_size`` and
    ``seq_len`` (``self.draft`` is its ``Generator``; its ``kv.tokens`` is this one's tensor).
    ``kv_dtype="fp8"`` (opt-in): the cache is quantized (``KVCache``, the module docstring has the
    format and the semantics); ``prefill`` in both forms, ``advance``, ``extend``, ``step`` and
    ``generate`` work as on a bf16 cache, while ``split_append=True``, ``draft=`` and ``beam_begin`` /
    ``beam_search`` raise ``ValueError``."""

    def __init__(self, model: TransformerLM, P: FlatParams, batch: int, device, split_append: bool = False,
                 draft=None, kv_dtype: str = "bf16"):
        if not (model.has_embed and model.has_head and list(model.layers) == list(range(model.cfg.n_layers))):
            raise ValueError("Generator needs the full model (embedding, every layer and the head): "
                             "pipeline-split stages cannot generate")
        if kv_dtype == "fp8" and split_append:
            raise ValueError("kv_dtype='fp8' does not support split_append=True (the split append launchers take "
                             "bf16 caches only)")
        if kv_dtype == "fp8" and draft is not None:
            raise ValueError("kv_dtype='fp8' does not support draft= (speculative decoding runs on bf16 caches only)")
        self.model, self.P, self.batch, self.device = model, P, int(batch), torch.device(device)
        self.kv_dtype = kv_dtype
        self.kv = KVCache(model.cfg, self.batch, self.device, kv_dtype=kv_dtype)
        self.split_append = bool(split_append)
        self.x =torch.zeros(self.batch, model.cfg.d_model, dtype=torch.bfloat16, device=self.device)
        self.temperature, self.seed = 0.0, 0
        self.top_k, self.top_p, self.eos_id = 0, 1.0, -1
        self.logits: Optional[torch.Tensor] = None   # the last step's logits [B, vocab]
        self.lengths: Optional[torch.Tensor] = None  # int32 [B]: the final lengths of the last generate
        self.prefill_rows = 0                        # rows per sequence the last prefill's forward ran over
        self._prefill_models: dict = {}              # rows -> the model at that seq_len (same parameters)
        self._chunk_bufs: dict = {}                  # chunk size -> advance's embedded rows [B * chunk, d_model]
        self._live = False                           # a prefill has run: extend may append
        # (temperature, seed) -> (graph, its logits); any other sampler setting or the
        # per-row mode: (temperature, seed, top_k, top_p, eos_id, per_row); the beam step: ("beam", W, eos_id)
        self._graphs: dict = {}
        self.beam: Optional[BeamState] = None        # the live beam search's state (beam_begin)
        self._beam_states: dict = {}                 # W -> BeamState (kept: a captured step holds its pointers)
        self.beam_scores: Optional[torch.Tensor] = None    # fp32 [G, W]: the last beam_search's ranking scores
        self.beam_logprobs: Optional[torch.Tensor] = None  # fp32 [G, W]: its raw log-probability sums
        self.beam_steps = 0                          # steps the last beam_search ran
        self.draft: Optional[Generator] = None       # the drafter (speculative decoding)
        self._draft_sync = False                     # the draft's cache and position follow the target's
        self._spec_states: dict = {}                 # k -> SpecState (kept: a captured round holds its pointers)
        self.spec_rounds = 0                         # rounds the last speculative generate ran
        self.spec_drafted: Optional[torch.Tensor] = None    # int32 [B]: drafts it proposed per row,
        self.spec_accepted: Optional[torch.Tensor] = None   # ... drafts kept
        self.spec_emitted: Optional[torch.Tensor] = None    # ... and tokens emitted
        if draft is not None:
            dm, dP = draft
            dc = getattr(dm, "cfg", None)
            if not isinstance(dm, TransformerLM) or (dc.vocab_size, dc.seq_len) != (model.cfg.vocab_size,
                                                                                   model.cfg.seq_len):
                raise ValueError("the draft must be a TransformerLM with the target's vocab_size and seq_len")
            self.draft = Generator(dm, dP, self.batch, self.device, split_append=split_append)
            self.draft.kv.tokens = self.kv.tokens    # one tensor: the drafts land where the verify pass reads them

    # ------------------------------------------------------------------ prefill
    def prefill(self, prompt: torch.Tensor, prompt_lens: Optional[torch.Tensor] = None, *,
                chunk: Optional[int] = None):
        """``prompt`` int [B, P], 1 <= P <= seq_len: fills cache rows < P and sets pos = P - 1.

        ``chunk`` (>= 1): chunked prefill -- instead of the training forward, the first P - 1
        tokens (per row: len_b - 1) go through ``advance`` in slices of at most ``chunk`` rows
        straight into the cache: no backward cache, no logits, no permute-copies.  It fills cache
        rows < P - 1 (the decode step writes row P - 1 itself), leaves the same position and
        leaves ``prefill_rows`` at 0.  ``None``: the path described below.

        ``prompt_lens`` (int [B], each in 1..P): ``prompt`` is right-padded, tokens at or past
        a row's length are ignored, and the per-row state becomes live: ``pos_rows[b] =
        len_b - 1``, ``end[b] = seq_len``.  Cache rows >= len_b of row b are never read before
        the decode step writes them.

        ``seq_len > 128``: the forward runs over ``prefill_rows`` = P rounded up to a multiple of
        128 (at most ``seq_len``) rows per sequence: a model of that ``seq_len`` on the same
        parameters (the embedding reads only the first ``prefill_rows`` rows of ``wpe``)."""
        c = self.model.cfg
        if chunk is not None and int(chunk) < 1:
            raise ValueError(f"chunk must be >= 1, got {chunk}")
        if prompt.dim() != 2 or prompt.shape[0] != self.batch or not 1 <= prompt.shape[1] <= c.seq_len:
            raise ValueError(f"prompt must be [{self.batch}, 1..{c.seq_len}], got {tuple(prompt.shape)}")
        B, Pn, H, Dh = self.batch, prompt.shape[1], c.n_heads, c.d_model // c.n_heads
        prompt = prompt.to(device=self.device, dtype=torch.int32)
        lens = None
        if prompt_lens is not None:
            lens = torch.as_tensor(prompt_lens).to(device=self.device)
            if lens.shape != (B,) or lens.dtype.is_floating_point or int(lens.min()) < 1 or int(lens.max()) > Pn:
                raise ValueError(f"prompt_lens must be {B} integers in 1..{Pn}, got {lens.tolist()}")
            lens = lens.to(torch.int32)
            prompt = prompt * (torch.arange(Pn, device=self.device)[None] < lens[:, None])   # padding -> token 0
        if int(prompt.min()) < 0 or int(prompt.max()) >= c.vocab_size:
            raise ValueError(f"prompt token outside [0, {c.vocab_size})")
        kv = self.kv
        kv.tokens.zero_()
        kv.tokens[:, :Pn] = prompt
        self._live = True
        self._draft_sync = False
        if chunk is not None:
            self.prefill_rows = 0
            kv.per_row = lens is not None
            kv.live_pos.zero_()
            if kv.per_row:
                kv.end.fill_(c.seq_len)
            self.advance(lens.cpu() - 1 if kv.per_row else Pn - 1, chunk=int(chunk))
            return
        model, Sp = self.model, c.seq_len
        if c.seq_len > K.AD_CHUNK_ROWS:
            Sp = min(-(-Pn // K.AD_CHUNK_ROWS) * K.AD_CHUNK_ROWS, c.seq_len)
            if Sp != c.seq_len:
                model = self._prefill_models.get(Sp)
                if model is None:
                    model = self._prefill_models[Sp] = TransformerLM(dataclasses.replace(c, seq_len=Sp))
        self.prefill_rows = Sp
        _, cache = model.forward(self.P, kv.tokens if Sp == c.seq_len else kv.tokens[:, :Sp].contiguous())
        for l, bc in zip(self.model.layers, cache.blocks):
            if kv.k_scale is not None:   # FP8: one quantizing launch per layer instead of the two copies
                K.kv_cache_fill(bc.qkv, kv.k[l], kv.v[l], kv.k_scale[l], kv.v_scale[l], Pn, Sp)
                continue
            qkv = bc.qkv.view(B, Sp, 3, H, Dh)
            kv.k[l][:, :, :Pn] = qkv[:, :Pn, 1].permute(0, 2, 1, 3)
            kv.v[l][:, :, :Pn] = qkv[:, :Pn, 2].permute(0, 2, 1, 3)
        kv.per_row = lens is not None
        if kv.per_row:
            kv.pos_rows.copy_(lens - 1)
            kv.end.fill_(c.seq_len)
        else:
            kv.pos.fill_(Pn - 1)

    # ------------------------------------------------------------------ append
    def advance(self, n, *, chunk: int, logits: bool = False) -> Optional[torch.Tensor]:
        """Process the ``n`` tokens already in ``kv.tokens`` at positions pos..pos+n-1 (their k / v
        go to the cache) and add ``n`` to the position, in slices of at most ``chunk`` rows:
        ``embed_append``, ``TransformerLM.append_chunk``, ``live_pos += slice count``.  ``n``: an
        int or, per-row mode only, an int tensor [B] (slice j of row b then holds
        ``clamp(n_b - j * chunk, 0, chunk)`` tokens).  The position is never read on the host: the
        counts come from ``n``, and the caller answers for ``pos + n <= seq_len`` (a slice that would
        pass the end of the cache writes nothing, but the position still advances).  With
        ``split_append`` set, ``kv.append_ws`` is first made to hold the largest slice's partials.

        ``logits=True``: returns the logits [B, vocab] of each row's last processed token (a row
        with nothing to process: of a zero vector); their block outputs are gathered before
        ``ln_f`` / the head, so the head runs at M = B."""
        kv, P, c, B = self.kv, self.P, self.model.cfg, self.batch
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError(f"chunk must be >= 1, got {chunk}")
        if isinstance(n, torch.Tensor) and n.dim() > 0:
            if not kv.per_row:
                raise ValueError("a per-row n needs the per-row cache state (prefill with prompt_lens)")
            nb = [int(v) for v in n.tolist()]
            if len(nb) != B:
                raise ValueError(f"n must be an int or {B} integers, got {nb}")
        else:
            nb = [int(n)] * B
        if min(nb) < 0:
            raise ValueError(f"n must be >= 0, got {nb}")
        uniform = min(nb) == max(nb)
        pos = kv.live_pos
        x = self._chunk_bufs.get(chunk)
        if x is None:   # once per chunk size, zero-initialised: rows past a count stay finite
            x = self._chunk_bufs[chunk] = torch.zeros(B * chunk, c.d_model, dtype=torch.bfloat16, device=self.device)
        last = torch.zeros(B, c.d_model, dtype=torch.bfloat16, device=self.device) if logits else None
        if self.split_append and max(nb) > 0:
            # the largest slice's partials; an outgrown buffer is replaced, a larger one is kept
            need = K.attention_append_ws_floats(B, c.n_heads, min(chunk, max(nb)), c.seq_len)
            if kv.append_ws is None or kv.append_ws.numel() < need:
                kv.append_ws = torch.empty(need, dtype=torch.float32, device=self.device)
                self._drop_spec_graphs()
        for lo in range(0, max(nb), chunk):
            C = min(chunk, max(nb) - lo)
            cnt = [min(max(v - lo, 0), C) for v in nb]
            count = None if uniform else torch.tensor(cnt, dtype=torch.int32, device=self.device)
            xs = x[:B * C]
            K.embed_append(kv.tokens, P.s("embed/wte"), P.s("embed/wpe"), pos, C, count=count, out=xs)
            h = self.model.append_chunk(P, kv, xs, C, count=count)
            if logits:
                ends = [(b, b * C + v - lo - 1) for b, v in enumerate(nb) if lo < v <= lo + C]
                if ends:
                    dst = torch.tensor([b for b, _ in ends], device=self.device)
                    src = torch.tensor([r for _, r in ends], device=self.device)
                    last[dst] = h[src]
            if uniform:
                pos.add_(C)
            else:
                pos.add_(count)
        if logits:
            self.logits = self.model.lm_head(P, last)
            return self.logits
        return None

    def extend(self, tokens: torch.Tensor, lens: Optional[torch.Tensor] = None, *, chunk: int = 64,
               logits: bool = False) -> Optional[torch.Tensor]:
        """Append ``tokens`` int [B, n] to a live cache (a second turn after a generation, teacher
        forcing a block, scoring a continuation): they are written at pos + 1 .. pos + n and
        ``advance(n)`` processes the n tokens from pos on, so ``pos`` again indexes the last, not yet
        processed, token and ``step`` / ``extend`` can follow.  ``lens`` (int [B], each in 0..n;
        per-row caches only): ``tokens`` is right-padded and row b appends its first ``lens[b]``
        tokens.  In per-row mode every row's ``end`` is set back to ``seq_len``.  ``logits=True``:
        the logits [B, vocab] of each row's last processed token, the one at the new pos - 1 (they
        predict the last token given).  Reads the position on the host once, to check the bounds.

        Raises ``ValueError`` before any prefill, for ``lens`` on a shared-position cache and when a
        row would pass ``seq_len``."""
        kv, c, B = self.kv, self.model.cfg, self.batch
        if not self._live:
            raise ValueError("extend needs a live cache: call prefill (or generate) first")
        if int(chunk) < 1:
            raise ValueError(f"chunk must be >= 1, got {chunk}")
        if lens is not None and not kv.per_row:
            raise ValueError("lens needs the per-row cache state (prefill with prompt_lens)")
        if tokens.dim() != 2 or tokens.shape[0] != B:
            raise ValueError(f"tokens must be [{B}, n], got {tuple(tokens.shape)}")
        n = tokens.shape[1]
        tokens = tokens.to(device=self.device, dtype=torch.int32)
        if lens is None:
            nb = [n] * B
        else:
            lt = torch.as_tensor(lens)
            if lt.shape != (B,) or lt.dtype.is_floating_point or int(lt.min()) < 0 or int(lt.max()) > n:
                raise ValueError(f"lens must be {B} integers in 0..{n}, got {lt.tolist()}")
            nb = [int(v) for v in lt.tolist()]
            tokens = tokens * (torch.arange(n, device=self.device)[None] < lt.to(self.device)[:, None])
        if n and (int(tokens.min()) < 0 or int(tokens.max()) >= c.vocab_size):
            raise ValueError(f"token outside [0, {c.vocab_size})")
        pv = kv.live_pos.tolist() if kv.per_row else kv.live_pos.tolist() * B
        for b, (p, v) in enumerate(zip(pv, nb)):
            if p < 0 or p + v > c.seq_len - 1:
                raise ValueError(f"row {b}: position {p} + {v} new tokens passes seq_len {c.seq_len} "
                                 f"(the learned positions end there)")
        for b, (p, v) in enumerate(zip(pv, nb)):
            kv.tokens[b, p + 1:p + 1 + v] = tokens[b, :v]
        if kv.per_row:
            kv.end.fill_(c.seq_len)
        self._draft_sync = False   # the target moves on without the draft
        return self.advance(torch.tensor(nb) if kv.per_row else n, chunk=chunk, logits=logits)

    # ------------------------------------------------------------------ one step
    def step(self, sample: bool = True) -> torch.Tensor:
        """One decode step at position ``pos``; returns its logits [B, vocab].  ``sample``:
        the sampler writes ``tokens[:, pos + 1]`` and advances ``pos`` (temperature / seed /
        top_k / top_p / eos_id: the attributes of that name).  ``sample=False`` (teacher
        forcing): ``tokens`` is left alone and ``pos`` advances by a torch op.  Per-row mode:
        ``pos`` is ``kv.pos_rows``, and a row at its ``end`` neither samples nor advances."""
        kv, P = self.kv, self.P
        pos = kv.live_pos
        self._draft_sync = False   # a plain step moves the target without its draft
        K.embed_decode(kv.tokens, P.s("embed/wte"), P.s("embed/wpe"), pos, out=self.x)
        self.logits = self.model.decode_step(P, kv, self.x)
        if not sample:
            pos.add_(1)
        elif kv.per_row:
            K.sample_tokens(self.logits, kv.tokens, pos, temperature=self.temperature, seed=self.seed, end=kv.end,
                            eos_id=self.eos_id, top_k=self.top_k, top_p=self.top_p)
        else:
            K.sample_tokens(self.logits, kv.tokens, pos, temperature=self.temperature, seed=self.seed,
                            top_k=self.top_k, top_p=self.top_p)
        return self.logits

    def _graph_key(self):
        key = (self.temperature, self.seed)
        if self.kv.per_row or self.top_k != 0 or self.top_p != 1.0 or self.eos_id >= 0:
            key += (self.top_k, self.top_p, self.eos_id, self.kv.per_row)
        return key

    def _replay(self, step=None, key=None):
        """The sampling step as a graph replay (captured on first use per sampler setting;
        one stream, no parallel branches).  The eager step before the capture is a real
        step: it also creates every lazily allocated workspace outside the capture.
        ``step`` / ``key``: another step function and its graph key (the beam step)."""
        step = self.step if step is None else step
        key = self._graph_key() if key is None else key
        ent = self._graphs.get(key)
        if ent is None:
            eager = step()
            torch.cuda.synchronize(self.device)
            g = capture_graph(step)   # records only: nothing runs, pos and the cache stay
            self._graphs[key] = (g, self.logits)
            self.logits = eager
            return
        g, logits = ent
        if g is None:   # the capture was refused: stay eager
            step()
            return
        g.replay()
        self.logits = logits

    # ------------------------------------------------------------------ speculative decoding
    def _spec_state(self, k: int) -> SpecState:
        """The checks common to ``spec_step`` / ``verify`` and the state of rounds of ``k`` drafts (made
        on first use, with the round's workspaces, so that nothing is allocated under a capture)."""
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= K.SPEC_MAX_DRAFTS:
            raise ValueError(f"speculative k must be an int in 1..{K.SPEC_MAX_DRAFTS}, got {k!r}")
        if not self._live:
            raise ValueError("speculative decoding needs a live cache: call prefill (or generate) first")
        if not self.kv.per_row:
            raise ValueError("speculative decoding needs the per-row cache state (prefill with prompt_lens)")
        st = self._spec_states.get(k)
        if st is None:
            st = self._spec_states[k] = SpecState(self.batch, k, self.device)
        c, C = self.model.cfg, k + 1
        if C not in self._chunk_bufs:
            self._chunk_bufs[C] = torch.zeros(self.batch * C, c.d_model, dtype=torch.bfloat16, device=self.device)
        if self.split_append:
            need = K.attention_append_ws_floats(self.batch, c.n_heads, C, c.seq_len)
            if self.kv.append_ws is None or self.kv.append_ws.numel() < need:
                self.kv.append_ws = torch.empty(need, dtype=torch.float32, device=self.device)
                self._drop_spec_graphs()
        return st

    def _drop_spec_graphs(self):
        """A captured round holds ``kv.append_ws``' pointer: a replaced buffer retires those graphs."""
        for gen in (self, self.draft):
            if gen is not None:
                gen._graphs = {key: v for key, v in gen._graphs.items() if key[0] != "spec"}

    def _verify(self, st: SpecState, dpos=None, dend=None) -> torch.Tensor:
        kv, P = self.kv, self.P
        x = self._chunk_bufs[st.C]
        K.embed_append(kv.tokens, P.s("embed/wte"), P.s("embed/wpe"), kv.pos_rows, st.C, count=st.count, out=x)
        self.logits = self.model.append_chunk(P, kv, x, st.C, count=st.count, head=True)
        K.spec_judge(self.logits, kv.tokens, kv.pos_rows, kv.end, st.count, st.acc, st.repl,
                     temperature=self.temperature, seed=self.seed, top_k=self.top_k, top_p=self.top_p)
        K.spec_commit(st.acc, st.repl, kv.tokens, kv.pos_rows, kv.end, st.count, st.drafted, st.accepted, st.emitted,
                      st.last_accept, eos_id=self.eos_id, dpos=dpos, dend=dend)
        return self.logits

    def verify(self, count: torch.Tensor, k: Optional[int] = None) -> torch.Tensor:
        """A speculative round without the drafter.  Row b's ``count[b] - 1`` drafts are already in
        ``kv.tokens[b, pos + 1 ..]``; ``count`` (int [B], each 0 or 1..k + 1) is copied into the round's
        state and the C = k + 1 tokens from ``pos`` on go through ``embed_append``, ``append_chunk(count=,
        head=True)``, ``spec_judge`` and ``spec_commit`` (temperature / seed / top_k / top_p / eos_id: the
        attributes of that name).  A row whose count would pass ``end`` or the cache sits the round out
        (see ``ops.kernels.spec_judge``).  ``k`` defaults to ``max(count) - 1`` (read on the host).  Returns
        the round's logits [B * C, vocab]: row b * C + i predicts token index pos_before + i + 1.
        ``self.spec_state(k)`` holds ``acc`` / ``repl`` / ``last_accept`` and the counters.  The draft
        generator, if any, is not told: ``spec_step`` refuses to go on after a ``verify``."""
        count = torch.as_tensor(count)
        if count.shape != (self.batch,) or count.dtype.is_floating_point:
            raise ValueError(f"count must be {self.batch} integers, got {tuple(count.shape)} {count.dtype}")
        if k is None:
            k = max(int(count.max()) - 1, 1)
        st = self._spec_state(k)
        st.count.copy_(count.to(device=self.device, dtype=torch.int32))
        self._draft_sync = False
        return self._verify(st)

    def spec_state(self, k: int) -> SpecState:
        """The ``SpecState`` of rounds of ``k`` drafts (``verify`` / ``spec_step`` create it)."""
        return self._spec_states[k]

    def spec_step(self, k: int) -> torch.Tensor:
        """One speculative round of up to ``k`` drafts per row (eager or under a capture; needs ``draft``
        in sync with the target: a speculative ``generate`` brings it there, ``extend`` / ``prefill`` /
        ``verify`` / ``step`` take it away).  k greedy per-row draft steps bounded by the draft's ``end`` (a draft
        equal to ``eos_id`` ends a row's drafting), ``spec_count``, one more draft step without sampling
        (the draft cache then holds the row of the last draft too), then the verify pass, whose commit
        sets the draft's position and end back to the target's.  Returns the verify logits
        [B * (k + 1), vocab]."""
        if self.draft is None:
            raise ValueError("spec_step needs a draft model: Generator(..., draft=(model, P))")
        st = self._spec_state(k)
        if not self._draft_sync:
            raise ValueError("the draft is not in sync with the target (extend / prefill / verify / step moved the target "
                             "alone): start again with generate(..., speculative=k)")
        d, kv = self.draft, self.kv
        d.temperature, d.eos_id = 0.0, self.eos_id
        for _ in range(k):
            d.step()
        torch.sub(d.kv.pos_rows, kv.pos_rows, out=st.n_drafted)
        K.spec_count(kv.pos_rows, kv.end, st.n_drafted, k, self.model.cfg.seq_len, out=st.count)
        d.step(sample=False)
        return self._verify(st, d.kv.pos_rows, d.kv.end)

    def _generate_spec(self, prompt, max_new_tokens, k, graph, prompt_lens, pad_id, prefill_chunk):
        c, kv, d = self.model.cfg, self.kv, self.draft
        if d is None:
            raise ValueError("speculative decoding needs a draft model: Generator(..., draft=(model, P))")
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= K.SPEC_MAX_DRAFTS:
            raise ValueError(f"speculative must be an int in 1..{K.SPEC_MAX_DRAFTS}, got {k!r}")
        Pn = prompt.shape[1] if prompt.dim() == 2 else 0
        if prompt_lens is None:
            prompt_lens = torch.full((self.batch,), Pn, dtype=torch.int32)
        lens = torch.as_tensor(prompt_lens)
        longest = int(lens.max()) if lens.numel() else 0
        if max_new_tokens < 0 or longest + max_new_tokens > c.seq_len:
            raise ValueError(f"longest prompt {longest} + max_new_tokens {max_new_tokens} exceeds seq_len "
                             f"{c.seq_len} (the learned positions end there)")
        self.prefill(prompt, lens, chunk=prefill_chunk)
        d.prefill(prompt, lens, chunk=prefill_chunk)   # the same tokens into the shared tensor again
        kv.end.copy_(kv.pos_rows + 1 + max_new_tokens)
        d.kv.pos_rows.copy_(kv.pos_rows)
        d.kv.end.copy_((kv.end.clamp(max=c.seq_len) - 1).clamp(min=0))
        st = self._spec_state(k)
        st.reset()
        self._draft_sync = True
        step = lambda: self.spec_step(k)  # noqa: E731
        key = ("spec", k, self.temperature, self.seed, self.top_k, self.top_p, self.eos_id)
        self.spec_rounds = 0
        for r in range(1, max_new_tokens + 1):   # every round emits a token per unfinished row
            if graph:
                self._replay(step, key)
            else:
                step()
            self.spec_rounds = r
            # a host read serialises the replay loop: look only every SPEC_CHECK_ROUNDS rounds
            if r % SPEC_CHECK_ROUNDS == 0 and r < max_new_tokens and bool((kv.pos_rows + 1 >= kv.end).all()):
                break
        self.spec_drafted, self.spec_accepted, self.spec_emitted = (t.clone() for t in (st.drafted, st.accepted,
                                                                                         st.emitted))
        self.lengths = kv.pos_rows + 1
        out = kv.tokens[:, :longest + max_new_tokens].clone()
        out[torch.arange(out.shape[1], device=self.device)[None] >= self.lengths[:, None]] = pad_id
        return out

    # ------------------------------------------------------------------ generate
    def generate(self, prompt: torch.Tensor, max_new_tokens: int, temperature: float = 0.0, seed: int = 0,
                 capture: bool = True, *, prompt_lens: Optional[torch.Tensor] = None, top_k: int = 0,
                 top_p: float = 1.0, eos_id: Optional[int] = None, pad_id: int = 0,
                 prefill_chunk: Optional[int] = None, speculative: Optional[int] = None) -> torch.Tensor:
        """``prompt`` int [B, P] -> int32 [B, P + max_new_tokens] (the prompt, then the new
        tokens).  ``temperature == 0``: greedy; otherwise softmax(logits / T) sampling from
        Philox stream ``seed``, restricted to the ``top_k`` largest logits (0: off) and, of
        those, the smallest head of probability mass >= ``top_p`` (1.0: off); ties at a
        threshold are kept.  ``capture`` (GPU only): the decode step is captured into a graph
        once per sampler setting and replayed per token.  ``prefill_chunk``: ``prefill``'s ``chunk``
        (chunked prefill into the cache; ``None``: through the training forward).

        ``prompt_lens`` (int [B], each in 1..P; ``prompt`` right-padded) or ``eos_id`` select the
        per-row mode: row b starts at its own length len_b and may grow to len_b +
        max_new_tokens; a row that emits ``eos_id`` stops there (the EOS is its last token)
        while the others go on, and the loop ends early once every row has finished (checked
        every 16 steps).  Returns int32 [B, max(len) + max_new_tokens] with ``pad_id`` at and
        past each row's final length; ``self.lengths`` (int32 [B]) holds those lengths.

        ``speculative`` = k in 1..15 (needs ``draft``): speculative rounds of up to k greedy drafts per
        row (``spec_step``) instead of decode steps; always the per-row mode and its ragged return
        format, the output distribution is the plain one's.  Both models are prefilled
        (``prefill_chunk`` for both), ``capture`` captures one round per (k, sampler setting), the loop
        ends once every row has finished (read every ``SPEC_CHECK_ROUNDS`` rounds, an untuned constant)
        and after at most ``max_new_tokens`` rounds.  Sets ``spec_rounds`` and ``spec_drafted`` /
        ``spec_accepted`` / ``spec_emitted`` (int32 [B])."""
        c = self.model.cfg
        Pn = prompt.shape[1] if prompt.dim() == 2 else 0
        if top_k < 0 or not 0.0 < top_p <= 1.0:
            raise ValueError(f"top_k must be >= 0 and top_p in (0, 1], got top_k={top_k} top_p={top_p}")
        self.temperature, self.seed = float(temperature), int(seed)
        self.top_k, self.top_p = int(top_k), float(top_p)
        self.eos_id = -1 if eos_id is None else int(eos_id)
        graph = capture and self.device.type == "cuda"
        run = self._replay if graph else self.step
        if speculative is not None:
            if self.eos_id >= c.vocab_size or (eos_id is not None and self.eos_id < 0):
                raise ValueError(f"eos_id {eos_id} outside [0, {c.vocab_size})")
            return self._generate_spec(prompt, max_new_tokens, speculative, graph, prompt_lens, pad_id, prefill_chunk)
        if prompt_lens is None and eos_id is None:
            if max_new_tokens < 0 or Pn + max_new_tokens > c.seq_len:
                raise ValueError(f"prompt length {Pn} + max_new_tokens {max_new_tokens} exceeds seq_len "
                                 f"{c.seq_len} (the learned positions end there)")
            self.prefill(prompt, chunk=prefill_chunk)
            for _ in range(max_new_tokens):
                run()
            self.lengths = torch.full((self.batch,), Pn + max_new_tokens, dtype=torch.int32, device=self.device)
            return self.kv.tokens[:, :Pn + max_new_tokens].clone()
        if self.eos_id >= c.vocab_size or (eos_id is not None and self.eos_id < 0):
            raise ValueError(f"eos_id {eos_id} outside [0, {c.vocab_size})")
        if prompt_lens is None:
            prompt_lens = torch.full((self.batch,), Pn, dtype=torch.int32)
        lens = torch.as_tensor(prompt_lens)
        longest = int(lens.max()) if lens.numel() else 0
        if max_new_tokens < 0 or longest + max_new_tokens > c.seq_len:
            raise ValueError(f"longest prompt {longest} + max_new_tokens {max_new_tokens} exceeds seq_len "
                             f"{c.seq_len} (the learned positions end there)")
        self.prefill(prompt, lens, chunk=prefill_chunk)
        kv = self.kv
        kv.end.copy_(kv.pos_rows + 1 + max_new_tokens)
        for i in range(1, max_new_tokens + 1):
            run()
            # a host read serialises the replay loop: look only every 16 steps
            if self.eos_id >= 0 and i % 16 == 0 and i < max_new_tokens and bool((kv.pos_rows + 1 >= kv.end).all()):
                break
        self.lengths = kv.pos_rows + 1
        out = kv.tokens[:, :longest + max_new_tokens].clone()
        out[torch.arange(out.shape[1], device=self.device)[None] >= self.lengths[:, None]] = pad_id
        return out

    # ------------------------------------------------------------------ beam search
    def beam_begin(self, prompt: torch.Tensor, num_beams: int, eos_id: Optional[int] = None,
                   prefill_chunk: Optional[int] = None) -> BeamState:
        """Start a beam search: ``prompt`` int [G, P] with G * num_beams == batch is repeated over each
        group's slots and prefilled (shared position, pos = P - 1), and the beam state is reset.
        Returns the ``BeamState`` (also ``self.beam``); ``beam_step`` runs the steps."""
        if self.kv_dtype == "fp8":
            raise ValueError("kv_dtype='fp8' does not support beam search (the cache reorder moves bf16 rows only)")
        c, W = self.model.cfg, int(num_beams)
        if not 1 <= W <= K.BEAM_MAX_W:
            raise ValueError(f"num_beams must be in 1..{K.BEAM_MAX_W}, got {num_beams}")
        if self.batch % W:
            raise ValueError(f"num_beams {W} does not divide the generator's batch {self.batch}")
        if prompt.dim() != 2 or prompt.shape[0] * W != self.batch:
            raise ValueError(f"prompt must be [{self.batch // W}, P] for {W} beams on a batch of {self.batch}, "
                             f"got {tuple(prompt.shape)}")
        if W > c.vocab_size:
            raise ValueError(f"num_beams {W} exceeds the vocabulary {c.vocab_size}")
        eos = -1 if eos_id is None else int(eos_id)
        if eos >= c.vocab_size or (eos_id is not None and eos < 0):
            raise ValueError(f"eos_id {eos_id} outside [0, {c.vocab_size})")
        self.prefill(prompt.repeat_interleave(W, dim=0), chunk=prefill_chunk)
        st = self._beam_states.get(W)
        if st is None:
            st = self._beam_states[W] = BeamState(self.batch, W, self.device)
        st.reset(eos)
        self.beam = st
        return st

    def beam_step(self) -> torch.Tensor:
        """One beam step at position ``pos``: the decode step, then ``beam_topw`` and ``beam_reorder``
        (which writes ``tokens[:, pos + 1]`` and advances ``pos``).  Returns the step's logits
        [B, vocab]; ``self.beam.parent`` / ``.token`` hold the step's choice."""
        kv, P, st = self.kv, self.P, self.beam
        if st is None or kv.per_row:
            raise ValueError("beam_step needs a beam search in progress: call beam_begin first")
        K.embed_decode(kv.tokens, P.s("embed/wte"), P.s("embed/wpe"), kv.pos, out=self.x)
        self.logits = self.model.decode_step(P, kv, self.x)
        K.beam_topw(self.logits, st.score, st.done, kv.pos, st.W, st.eos_id, seq_len=self.model.cfg.seq_len,
                    out=st.cand)
        K.beam_reorder(st.cand, kv.k, kv.v, kv.tokens, st.score, st.done, st.length, st.parent, st.token, kv.pos,
                       st.W, st.eos_id, ptrs=kv.history_ptrs() if self.device.type == "cuda" else None)
        return self.logits

    def beam_search(self, prompt: torch.Tensor, max_new_tokens: int, num_beams: int = 1, *,
                    eos_id: Optional[int] = None, length_penalty: float = 0.0, pad_id: int = 0,
                    capture: bool = True, prefill_chunk: Optional[int] = None) -> torch.Tensor:
        """``prompt`` int [G, P] -> int32 [G, num_beams, P + max_new_tokens]: per prompt the
        ``num_beams`` hypotheses the search ends with, best first.  The generator's batch must be
        G * num_beams.  A hypothesis that emits ``eos_id`` is finished (the EOS is its last token, its
        score stops changing) and keeps competing; the loop ends early once every slot is finished
        (checked every 16 steps).  Ranking: ``score / max(length, 1) ** length_penalty`` with ``length``
        the generated tokens (0.0: the raw sum of log-probabilities), stable.  ``pad_id`` fills
        positions at and past each hypothesis' final length.  Sets ``beam_scores`` (the ranking
        scores) and ``beam_logprobs`` (the raw sums), fp32 [G, W], and ``lengths`` (int32 [G, W],
        prompt included).  ``capture`` (GPU only): the beam step is captured once per
        (num_beams, eos_id) and replayed per token."""
        c = self.model.cfg
        Pn = prompt.shape[1] if prompt.dim() == 2 else 0
        if max_new_tokens < 0 or Pn + max_new_tokens > c.seq_len:
            raise ValueError(f"prompt length {Pn} + max_new_tokens {max_new_tokens} exceeds seq_len "
                             f"{c.seq_len} (the learned positions end there)")
        st = self.beam_begin(prompt, num_beams, eos_id=eos_id, prefill_chunk=prefill_chunk)
        G, W = st.G, st.W
        graph = capture and self.device.type == "cuda"
        key = ("beam", W, st.eos_id)
        self.beam_steps = 0
        for i in range(1, max_new_tokens + 1):
            if graph:
                self._replay(self.beam_step, key)
            else:
                self.beam_step()
            self.beam_steps = i
            # a host read serialises the replay loop: look only every 16 steps
            if st.eos_id >= 0 and i % 16 == 0 and i < max_new_tokens and bool(st.done.all()):
                break
        raw, length = st.score.view(G, W), st.length.view(G, W)
        rank = raw / length.clamp(min=1).to(torch.float32) ** float(length_penalty)
        order = torch.sort(rank, dim=1, descending=True, stable=True).indices
        self.beam_scores, self.beam_logprobs = rank.gather(1, order), raw.gather(1, order)
        self.lengths = (Pn + length).gather(1, order).to(torch.int32)
        out = self.kv.tokens[:, :Pn + max_new_tokens].view(G, W, -1)
        out = out.gather(1, order[:, :, None].expand(-1, -1, out.shape[2]))   # a copy, best first
        out[torch.arange(out.shape[2], device=self.device)[None, None] >= self.lengths[:, :, None]] = pad_id
        return out
