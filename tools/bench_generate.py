"""Decode-step timing of KV-cache generation (jax_distributed_tuts_amd/generation.py) for the
default TransformerConfig at B = 1 and B = 16: us per decode step and tokens/s, launched
eagerly against one captured step replayed per token, plus the kernel-launcher calls per step.

    python tools/bench_generate.py [--steps 100] [--temperature 0.0] [--ragged] [--seq-len N] [--prompt-len P]
                                   [--prefill-chunk N[,N...]] [--split-append] [--beams W[,W...]]
                                   [--speculative K[,K...]] [--kv-dtype bf16,fp8]

Each figure: ``--steps`` decode steps after a 16-token prefill, timed with events around the
whole loop (prefill excluded), median of 5 runs.  ``--seq-len N`` > 128 builds the LM with an
N-row cache and prefills ``N - steps - 1`` tokens, so the timed steps attend at depth (split-KV
decode attention); ``--prompt-len`` overrides that, e.g. 16 for a shallow position in a deep
cache, and ``--batch`` the batch sizes.  ``--ragged`` adds, at B = 16 and a sampling
temperature (``--temperature``, or 0.8 when that is 0): the uniform batch with the top-k /
top-p sampler (k = 50, p = 0.9), and a ragged batch (prompt lengths 1..16, per-row positions)
with the plain and with the filtered sampler.  ``--prefill-chunk 64,256,1024`` adds, per batch
size, the time and the peak memory of one prefill of the same prompt through the training forward
and through chunked prefill at each chunk size (``prefill_lines``); with ``--split-append`` each chunk
line is followed by a ``chunk N split`` line, the same prefill through the split-KV append attention
of ``Generator(..., split_append=True)``.  ``--beams 4,8`` adds, per batch
size G (then the number of prompts) and beam count W, the beam step of ``Generator.beam_search`` on G x W
rows beside the plain sampled step at the same batch and depth (``beam_lines``).  ``--speculative 2,4,8``
adds, per batch size and draft count K, the captured speculative round of ``Generator.spec_step`` beside
the plain captured step of the main line: us per round, tokens per round and hence us per token, for the
target itself as the draft (acceptance near 1: the ceiling on tokens per round, at the full cost of K + 1
target-sized draft steps) and for a 1-layer draft with fresh weights (acceptance near 0: one token per
round, the worst case) (``spec_lines``).  ``--kv-dtype bf16,fp8`` prints the main line once per cache dtype
(``Generator(..., kv_dtype=)``), each with the bytes its K / V caches and their scales hold; the extra
lines above are bf16-only and follow the bf16 line.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jax_distributed_tuts_amd.generation import Generator  # noqa: E402
from jax_distributed_tuts_amd.models.transformer import TransformerConfig, TransformerLM  # noqa: E402
from jax_distributed_tuts_amd.ops import _lib  # noqa: E402
from jax_distributed_tuts_amd.ops import kernels as K  # noqa: E402
from jax_distributed_tuts_amd.utils.flat import FlatParams  # noqa: E402

PROMPT = 16


class _CountingLib:
    """The kernel library with every launcher call counted (setters / planners / size queries are not)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if "_set_" in name or name.endswith(("_eligible", "_size", "_bytes", "_plan")):
            return fn

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)

        return counted


def launches_per_step(gen, step=None):
    real = _lib.lib
    proxy = _CountingLib(real())
    _lib.lib = lambda: proxy
    try:
        (step or gen.step)()
    finally:
        _lib.lib = real
    return proxy.calls


def timed(run, reset, steps):
    ts = []
    for _ in range(5):
        reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            run()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / steps)
    return sorted(ts)[2]


def prefill_lines(model, P, B, dev, prompt, chunks, reps=5, split_append=False):
    """One line per prefill path -- the training forward, then chunked prefill at each chunk size:
    the time of one ``prefill`` (host clock around a call that ends in a device synchronise,
    median of ``reps`` after a warm-up call that also makes every allocation and GEMM tile
    choice) and the peak of ``torch.cuda.max_memory_allocated`` during the timed calls, beside
    what was allocated before them (parameters, the KV cache and the path's persistent buffers).
    ``split_append``: after each ``chunk N`` line a ``chunk N split`` line, the same prefill from a
    ``Generator(..., split_append=True)`` (the split-KV append attention)."""
    cfg = model.cfg
    paths = [(None, False)]
    for c in chunks:
        paths += [(c, False)] + ([(c, True)] if split_append else [])
    for chunk, split in paths:
        gen = Generator(model, P, B, dev, split_append=split)
        gen.prefill(prompt, chunk=chunk)
        torch.cuda.synchronize(dev)
        held = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            gen.prefill(prompt, chunk=chunk)
            torch.cuda.synchronize(dev)
            ts.append((time.perf_counter() - t0) * 1e3)
        peak = torch.cuda.max_memory_allocated(dev)
        ts.sort()
        path = "training forward" if chunk is None else f"chunk {chunk:4d}" + (" split" if split else "")
        print(f"prefill  B={B:2d} S={cfg.seq_len} P={prompt.shape[1]} {path:>16}: {ts[len(ts) // 2]:9.2f} ms "
              f"(min {ts[0]:.2f}, max {ts[-1]:.2f}) | {B * prompt.shape[1] / ts[len(ts) // 2] * 1e3:10.0f} tokens/s | "
              f"peak {peak / 2 ** 20:8.1f} MiB ({(peak - held) / 2 ** 20:8.1f} MiB above the {held / 2 ** 20:.1f} MiB "
              f"held between calls)", flush=True)
        del gen


def beam_lines(model, P, G, dev, beams, steps, temperature, depth):
    """Per beam count W, on a generator of G x W rows: us per beam step (decode step + ``beam_topw`` +
    ``beam_reorder``), eager and captured, with its launcher calls; the select + reorder launches alone
    (the step's own candidates and position, eager, so launch-bound at small caches); the share of
    slots that changed parent per step (what the reorder has to move); and the plain sampled step of
    the same generator at the same batch and depth."""
    cfg = model.cfg
    for W in beams:
        B = G * W
        gen = Generator(model, P, B, dev)
        prompt = torch.randint(0, cfg.vocab_size, (G, PROMPT), generator=torch.Generator().manual_seed(1))
        prompt = prompt.to(torch.int32).to(dev)
        gen.beam_search(prompt, 2, W, capture=True)   # warm-up + the step capture
        graph = gen._graphs[("beam", W, -1)][0]
        reset = lambda: gen.beam_begin(prompt, W)  # noqa: E731
        reset()
        calls = launches_per_step(gen, gen.beam_step)
        t_e = timed(gen.beam_step, reset, steps)
        st, kv = gen.beam, gen.kv
        reset()
        moved = torch.zeros((), dtype=torch.int64, device=dev)
        own = torch.arange(B, device=dev) % W
        for _ in range(steps):
            gen.beam_step()
            moved += (st.parent != own).sum()

        def tail():
            K.beam_topw(gen.logits, st.score, st.done, kv.pos, W, -1, seq_len=cfg.seq_len, out=st.cand)
            K.beam_reorder(st.cand, kv.k, kv.v, kv.tokens, st.score, st.done, st.length, st.parent, st.token, kv.pos,
                           W, -1, ptrs=kv.history_ptrs())

        def reset_tail():
            reset()
            gen.beam_step()   # logits and a spread-out beam state to select from

        t_t = timed(tail, reset_tail, steps - 1)
        line = (f"beam     G={G:2d} W={W} B={B:3d}{depth}: eager {t_e:7.1f} us/step")
        if graph is not None:
            line += f" | captured {timed(graph.replay, reset, steps):7.1f} us/step"
        line += (f" | select + reorder alone, eager {t_t:6.1f} us | {float(moved) / (steps * B):.2f} of the slots "
                 f"change parent per step | {sum(calls.values())} launcher calls/step: "
                 + ", ".join(f"{k[4:]} x{v}" for k, v in sorted(calls.items())))
        print(line, flush=True)
        wide = prompt.repeat_interleave(W, 0)
        gen.generate(wide, 2, temperature=temperature, capture=True)
        pgraph = gen._graphs[(float(temperature), 0)][0]
        preset = lambda: gen.prefill(wide)  # noqa: E731
        line = f"  plain step B={B:3d} T={temperature}{depth}: eager {timed(gen.step, preset, steps):7.1f} us/step"
        if pgraph is not None:
            line += f" | captured {timed(pgraph.replay, preset, steps):7.1f} us/step"
        print(line, flush=True)
        del gen, graph, pgraph, reset, preset


def spec_lines(model, P, B, dev, ks, steps, temperature, depth, t_plain):
    """Per draft count k and draft -- the target itself, then a 1-layer LM with fresh weights: us per
    captured speculative round (k + 1 draft steps, the count, the verify append pass, judge, commit),
    the tokens a row emits per round (from the device counters over the timed number of rounds) and
    the resulting us per token beside the plain captured step's ``t_plain``; and the launcher calls
    of one round.  Rounds per run: ``steps // (k + 1)``, so no row reaches its end while timed."""
    cfg = model.cfg
    small = TransformerLM(TransformerConfig(seq_len=cfg.seq_len, n_layers=1))
    drafts = (("self", (model, P)), ("1-layer", (small, FlatParams(small.param_specs(), device=dev).init_(1))))
    prompt = torch.randint(0, cfg.vocab_size, (B, PROMPT), generator=torch.Generator().manual_seed(1))
    prompt = prompt.to(torch.int32).to(dev)
    for k in ks:
        rounds = max(steps // (k + 1), 1)
        for name, draft in drafts:
            gen = Generator(model, P, B, dev, draft=draft)
            gen.generate(prompt, 2 * (k + 1), temperature=temperature, speculative=k, capture=True)   # warm-up + capture
            graph = gen._graphs[("spec", k, float(temperature), 0, 0, 1.0, -1)][0]
            st = gen.spec_state(k)

            def reset():
                gen.generate(prompt, 0, temperature=temperature, speculative=k)   # both prefills, in sync, no round
                gen.kv.end.fill_(min(PROMPT + steps + 2, cfg.seq_len))
                gen.draft.kv.end.copy_(gen.kv.end - 1)

            step = lambda: gen.spec_step(k)  # noqa: E731
            reset()
            calls = launches_per_step(gen, step)
            run = graph.replay if graph is not None else step
            t_r = timed(run, reset, rounds)
            reset()
            for _ in range(rounds):
                run()
            per_round = float(st.emitted.sum()) / (B * rounds)
            acc, dr = int(st.accepted.sum()), int(st.drafted.sum())
            print(f"spec     B={B:2d} T={temperature}{depth} k={k:2d} draft={name:>7}: "
                  f"{'captured' if graph is not None else 'eager'} {t_r:8.1f} us/round | {per_round:5.2f} tokens/round "
                  f"(accepted / drafted {acc} / {dr}) | {t_r / per_round:7.1f} us/token (plain captured step "
                  f"{t_plain:7.1f}) | {sum(calls.values())} launcher calls/round: "
                  + ", ".join(f"{c[4:]} x{v}" for c, v in sorted(calls.items())), flush=True)
            del gen, graph, st, reset, step, run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--speculative", default=None, metavar="K[,K...]",
                    help="extra lines per batch size: the captured speculative round with K drafts, for the target "
                         "as its own draft and for a fresh 1-layer draft, beside the plain captured step")
    ap.add_argument("--beams", default=None, metavar="W[,W...]",
                    help="extra lines per batch size G: the beam step on G x W rows, eager and captured, beside "
                         "the plain sampled step at the same batch")
    ap.add_argument("--prefill-chunk", default=None, metavar="N[,N...]",
                    help="extra lines per batch size: the time and peak memory of one prefill through the "
                         "training forward and through chunked prefill at each of these chunk sizes")
    ap.add_argument("--split-append", action="store_true",
                    help="with --prefill-chunk: after each chunk line, the same prefill with the split-KV append "
                         "attention (Generator(split_append=True))")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--temperature", type=float, default=0.0)
    ap.add_argument("--ragged", action="store_true", help="extra lines: top-k / top-p and a ragged B = 16 batch")
    ap.add_argument("--seq-len", type=int, default=128, help="cache rows; > 128: the prompt is seq_len - steps - 1")
    ap.add_argument("--prompt-len", type=int, default=None, help="override the prompt length")
    ap.add_argument("--batch", default="1,16", help="comma-separated batch sizes of the main lines")
    ap.add_argument("--kv-dtype", default="bf16", metavar="bf16[,fp8]",
                    help="comma-separated KV cache dtypes: the main line once per dtype, with the cache's bytes")
    a = ap.parse_args()
    dtypes = a.kv_dtype.split(",")
    dev = torch.device("cuda", 0)
    cfg = TransformerConfig(seq_len=a.seq_len)
    global PROMPT
    if a.prompt_len is not None:
        PROMPT = a.prompt_len
    elif a.seq_len > 128:
        PROMPT = a.seq_len - a.steps - 1
    assert PROMPT >= 1 and PROMPT + a.steps <= cfg.seq_len
    model = TransformerLM(cfg)
    P = FlatParams(model.param_specs(), device=dev).init_(0)
    for B, kv_dtype in ((int(v), t) for v in a.batch.split(",") for t in dtypes):
        gen = Generator(model, P, B, dev, kv_dtype=kv_dtype)
        prompt = torch.randint(0, cfg.vocab_size, (B, PROMPT), generator=torch.Generator().manual_seed(1))
        prompt = prompt.to(torch.int32).to(dev)
        gen.generate(prompt, 2, temperature=a.temperature, capture=True)   # warm-up + the step capture
        graph = gen._graphs[(float(a.temperature), 0)][0]
        reset = lambda: gen.prefill(prompt)  # noqa: E731
        reset()
        calls = launches_per_step(gen)
        t_e = timed(gen.step, reset, a.steps)
        depth = f" S={a.seq_len} P={PROMPT}" if a.seq_len != 128 or a.prompt_len is not None else ""
        line = (f"generate B={B:2d} T={a.temperature}{depth} kv={kv_dtype:>4}: eager {t_e:7.1f} us/step "
                f"({B / t_e * 1e6:9.0f} tokens/s)")
        t_g = float("nan")
        if graph is not None:
            t_g = timed(graph.replay, reset, a.steps)
            line += f" | captured {t_g:7.1f} us/step ({B / t_g * 1e6:9.0f} tokens/s)"
        print(line + f" | cache {gen.kv.cache_bytes() / 2 ** 20:8.2f} MiB | {sum(calls.values())} launcher calls/step: "
              + ", ".join(f"{k[4:]} x{v}" for k, v in sorted(calls.items())), flush=True)
        if kv_dtype != "bf16":   # the extra lines below run on bf16 caches
            del gen, graph, reset
            continue
        if a.speculative:
            spec_lines(model, P, B, dev, [int(v) for v in a.speculative.split(",")], a.steps, a.temperature, depth, t_g)
        if a.prefill_chunk:
            del gen, graph, reset
            prefill_lines(model, P, B, dev, prompt, [int(v) for v in a.prefill_chunk.split(",")],
                          split_append=a.split_append)
        if a.beams:
            beam_lines(model, P, B, dev, [int(v) for v in a.beams.split(",")], a.steps, a.temperature, depth)
    if not a.ragged:
        return
    B, T = 16, a.temperature or 0.8
    prompt = torch.randint(0, cfg.vocab_size, (B, PROMPT), generator=torch.Generator().manual_seed(1))
    prompt = prompt.to(torch.int32).to(dev)
    for lens in (None, torch.arange(1, B + 1)):
        for top_k, top_p in ((0, 1.0), (50, 0.9)):
            if lens is None and top_k == 0:
                continue   # the uniform batch with the plain sampler: the lines above
            gen = Generator(model, P, B, dev)
            gen.generate(prompt, 2, temperature=T, capture=True, prompt_lens=lens, top_k=top_k, top_p=top_p)
            graph = gen._graphs[gen._graph_key()][0]
            reset = lambda: gen.prefill(prompt, lens)  # noqa: E731  (end = seq_len: no row finishes in the loop)
            t_e = timed(gen.step, reset, a.steps)
            line = (f"generate B={B:2d} T={T} {'ragged ' if lens is not None else 'uniform'} top_k={top_k:2d} "
                    f"top_p={top_p}: eager {t_e:7.1f} us/step")
            if graph is not None:
                t_g = timed(graph.replay, reset, a.steps)
                line += f" | captured {t_g:7.1f} us/step ({B / t_g * 1e6:9.0f} tokens/s)"
            print(line, flush=True)


if __name__ == "__main__":
    main()
