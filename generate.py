"""Autoregressive generation with the tutorial's transformer LM on one device
(jax_distributed_tuts_amd/generation.py: KV cache, prefill through the training forward,
one captured decode step replayed per token).

    python generate.py --prompt-len 16 --max-new-tokens 32            # untrained weights
    python generate.py --train-steps 200 --temperature 0.8 --seed 3   # train on lm_batch first
    python generate.py --restore ckpt_dir                             # weights of a checkpoint
    python generate.py --batch 3 --prompt-lens 5,16,9 --temperature 0.8 --top-k 50 --top-p 0.9 --eos-id 7
    python generate.py --seq-len 1024 --prompt-len 900 --max-new-tokens 100   # a 1024-row KV cache
    python generate.py --seq-len 1024 --prompt-len 900 --prefill-chunk 256    # chunked prefill into the cache
    python generate.py --seq-len 4096 --prompt-len 4000 --prefill-chunk 64 --split-append   # split-KV append
    python generate.py --beams 4 --length-penalty 1.0 --eos-id 7              # beam search, 4 hypotheses per prompt
    python generate.py --train-steps 200 --speculative 4 --draft-layers 1     # speculative decoding, 4 drafts per round
    python generate.py --seq-len 4096 --prompt-len 4000 --kv-dtype fp8        # FP8 KV cache: 68 bytes per row, not 128

Runs the HIP kernels on a GPU and the torch reference paths on CPU tensors when none is
present.  The prompt is the first ``--prompt-len`` tokens of ``lm_batch``'s sequences;
``--prompt-lens`` gives every sequence its own length (ragged prompts), ``--top-k`` /
``--top-p`` restrict the sampler and ``--eos-id`` ends a sequence at that token.  Each row is
printed up to its own final length.  ``--seq-len`` builds the LM with that many learned
positions (default 128); up to 32768 the decode attention stays on the HIP kernels (split-KV
past 128 cache rows).  ``--prefill-chunk N`` fills the cache through the append kernels in slices
of N prompt rows instead of one pass of the training forward; ``--split-append`` (only with
``--prefill-chunk``) runs them through the split-KV append attention, meant for small N and deep
caches.  ``--beams W`` (1..8) runs a beam search
instead of sampling: ``--batch`` prompts with W hypotheses each (a generator of batch * W rows), printed
best first with their scores, ranked by ``log-probability / length ** --length-penalty``.
``--speculative K`` (1..15; not with ``--beams``) decodes speculatively: a draft LM of ``--draft-layers``
layers (default 1; the same width, vocabulary and ``--seq-len``, trained for the same ``--train-steps`` on
the same batch) proposes K greedy tokens per round and the target scores them in one append pass; the
output distribution is the plain decoder's.  The run also prints the rounds and accepted / drafted.
``--kv-dtype fp8`` stores the cache as e4m3 bytes with one power-of-two fp32 scale per (layer, head, token) row of
K and of V (68 bytes against 128); attention then sees the dequantized rows.  Not with ``--beams``,
``--speculative`` or ``--split-append``.
Not covered: FP8 caches with beams, speculative decoding or split append, per-channel or per-tensor scales,
e5m2, FP8 MFMA for Q K^T, quantized weights, sampled, n-gram or tree drafters, speculative beams, beams over ragged prompts, diverse or constrained beam search, repetition penalties,
sequences past ``seq_len``, caches longer than 32768 rows or head dims other than 64 on the HIP path,
multi-GPU or pipeline-split generation.
"""
from __future__ import annotations

import argparse
import time

import torch

from jax_distributed_tuts_amd.generation import Generator
from jax_distributed_tuts_amd.models.transformer import TransformerConfig
from jax_distributed_tuts_amd.parallel.pipeline_lm import build_lm_pipeline, lm_batch
from jax_distributed_tuts_amd.utils.train_state import Batch


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--train-steps", type=int, default=0, help="AdamW steps on lm_batch before generating")
    ap.add_argument("--restore", default=None, metavar="DIR", help="load a utils.checkpoint directory first")
    ap.add_argument("--prompt-len", type=int, default=16)
    ap.add_argument("--max-new-tokens", type=int, default=32)
    ap.add_argument("--temperature", type=float, default=0.0, help="0: greedy")
    ap.add_argument("--seed", type=int, default=0, help="sampling seed (Philox stream)")
    ap.add_argument("--top-k", type=int, default=0, help="sample from the k largest logits only (0: off)")
    ap.add_argument("--top-p", type=float, default=1.0, help="nucleus sampling mass in (0, 1] (1: off)")
    ap.add_argument("--eos-id", type=int, default=None, help="a sequence that emits this token stops there")
    ap.add_argument("--prompt-lens", default=None, metavar="L0,L1,...",
                    help="one prompt length per sequence (ragged prompts); overrides --prompt-len")
    ap.add_argument("--model-seed", type=int, default=0, help="parameter initialisation seed")
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--seq-len", type=int, default=128, help="learned positions == rows of the KV cache")
    ap.add_argument("--eager", action="store_true", help="launch every decode step eagerly (no graph replay)")
    ap.add_argument("--prefill-chunk", type=int, default=None, metavar="N",
                    help="chunked prefill: the prompt goes into the cache in slices of N rows "
                         "(default: one pass of the training forward)")
    ap.add_argument("--split-append", action="store_true",
                    help="with --prefill-chunk: the chunked prefill runs the split-KV append attention "
                         "(one workgroup per 512-key span of the cache and a combine launch)")
    ap.add_argument("--beams", type=int, default=0, metavar="W",
                    help="beam search with W hypotheses per prompt (1..8) instead of sampling")
    ap.add_argument("--length-penalty", type=float, default=0.0, metavar="A",
                    help="beam ranking: log-probability / generated length ** A (0: the raw log-probability)")
    ap.add_argument("--speculative", type=int, default=0, metavar="K",
                    help="speculative decoding: K greedy drafts per round (1..15) from a small draft LM")
    ap.add_argument("--draft-layers", type=int, default=1, metavar="L",
                    help="with --speculative: layers of the draft LM (trained like the target)")
    ap.add_argument("--kv-dtype", choices=("bf16", "fp8"), default="bf16",
                    help="the KV cache's storage: bf16, or fp8 (e4m3 bytes and one fp32 scale per row)")
    args = ap.parse_args(argv)
    if args.kv_dtype == "fp8" and (args.beams or args.speculative or args.split_append):
        ap.error("--kv-dtype fp8 does not combine with --beams, --speculative or --split-append")
    if args.speculative and args.beams:
        ap.error("--speculative and --beams exclude each other: there are no speculative beams")
    if args.speculative and not 1 <= args.speculative <= 15:
        ap.error("--speculative K needs K in 1..15")
    if args.split_append and args.prefill_chunk is None:
        ap.error("--split-append needs --prefill-chunk N: only the chunked prefill appends to the cache")
    return args


def beam_main(args, tr, prompt, dev):
    if args.prompt_lens or args.temperature or args.top_k or args.top_p != 1.0:
        raise SystemExit("--beams is a deterministic search over prompts of one length: it takes none of "
                         "--prompt-lens, --temperature, --top-k, --top-p")
    W = args.beams
    gen = Generator(tr.state.apply_fn, tr.state.params, args.batch * W, dev, split_append=args.split_append)
    sync = (lambda: torch.cuda.synchronize(dev)) if dev.type == "cuda" else (lambda: None)
    kw = dict(eos_id=args.eos_id, length_penalty=args.length_penalty, capture=not args.eager,
              prefill_chunk=args.prefill_chunk)
    out = gen.beam_search(prompt, args.max_new_tokens, W, **kw)   # first call: allocations and the step capture
    sync()
    t0 = time.perf_counter()
    out = gen.beam_search(prompt, args.max_new_tokens, W, **kw)
    sync()
    dt = time.perf_counter() - t0
    lengths, scores, raw = gen.lengths.cpu().tolist(), gen.beam_scores.cpu().tolist(), gen.beam_logprobs.cpu().tolist()
    for g, beams in enumerate(out.cpu().tolist()):
        for r, row in enumerate(beams):
            print(f"[generate] group {g} beam {r}: score {scores[g][r]:.4f} (log-probability {raw[g][r]:.4f}, "
                  f"{lengths[g][r] - args.prompt_len} new): {' '.join(str(t) for t in row[:lengths[g][r]])}")
    print(f"[generate] device={dev} groups={args.batch} beams={W} prompt={args.prompt_len} new={args.max_new_tokens} "
          f"length_penalty={args.length_penalty} eos_id={args.eos_id} "
          f"{'eager' if args.eager or dev.type != 'cuda' else 'captured'}: {gen.beam_steps} beam steps, "
          f"{gen.beam_steps / dt:.1f} steps/s ({dt * 1e3:.2f} ms with the prefill)")


def main(args):
    dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    if dev.type == "cuda":
        torch.cuda.set_device(dev)
    tr, cfg = build_lm_pipeline(None, dev, cfg=TransformerConfig(seq_len=args.seq_len), seed=args.model_seed)
    if args.restore:
        from jax_distributed_tuts_amd.utils.checkpoint import restore

        restore(tr.state, args.restore)
    data = lm_batch(cfg, global_batch=max(16, args.batch), seed=1)
    trainers = [tr]
    if args.speculative:   # the draft: the same LM with fewer layers, trained the same way
        dcfg = TransformerConfig(seq_len=args.seq_len, n_layers=args.draft_layers)
        trainers.append(build_lm_pipeline(None, dev, cfg=dcfg, seed=args.model_seed + 1)[0])
    if args.train_steps:
        batch = Batch(data.inputs[:16].to(dev), data.labels[:16].to(dev))
        for t in trainers:
            for _ in range(args.train_steps):
                t.step(batch)
            if hasattr(t, "finalize"):
                t.finalize()
    lens = None
    if args.prompt_lens:
        lens = torch.tensor([int(v) for v in args.prompt_lens.split(",")])
        if lens.numel() != args.batch:
            raise SystemExit(f"--prompt-lens needs one length per sequence ({args.batch}), got {lens.numel()}")
        args.prompt_len = int(lens.max())
    prompt = data.inputs[:args.batch, :args.prompt_len].contiguous().to(dev)
    if args.beams:
        return beam_main(args, tr, prompt, dev)
    draft = (trainers[1].state.apply_fn, trainers[1].state.params) if args.speculative else None
    gen = Generator(tr.state.apply_fn, tr.state.params, args.batch, dev, split_append=args.split_append, draft=draft,
                    kv_dtype=args.kv_dtype)
    sync = (lambda: torch.cuda.synchronize(dev)) if dev.type == "cuda" else (lambda: None)
    kw = dict(temperature=args.temperature, seed=args.seed, capture=not args.eager, prompt_lens=lens,
              top_k=args.top_k, top_p=args.top_p, eos_id=args.eos_id, prefill_chunk=args.prefill_chunk)
    if args.speculative:
        kw["speculative"] = args.speculative
    out = gen.generate(prompt, args.max_new_tokens, **kw)   # first call: allocations and the step capture
    sync()
    t0 = time.perf_counter()
    out = gen.generate(prompt, args.max_new_tokens, **kw)
    sync()
    dt = time.perf_counter() - t0
    lengths = gen.lengths.cpu().tolist()
    for b, row in enumerate(out.cpu().tolist()):
        print(f"[generate] seq {b}: {' '.join(str(t) for t in row[:lengths[b]])}")
    n = sum(lengths) - (int(lens.sum()) if lens is not None else args.batch * args.prompt_len)   # new tokens
    print(f"[generate] device={dev} batch={args.batch} prompt={args.prompt_lens or args.prompt_len} "
          f"new={args.max_new_tokens} temperature={args.temperature} top_k={args.top_k} top_p={args.top_p} "
          f"eos_id={args.eos_id} kv_dtype={args.kv_dtype} ({gen.kv.cache_bytes() / 2 ** 20:.2f} MiB) {'eager' if args.eager or dev.type != 'cuda' else 'captured'}: "
          f"{n / dt:.1f} tokens/s ({dt * 1e3:.2f} ms with the prefill)")
    if args.speculative:
        acc, dr = int(gen.spec_accepted.sum()), int(gen.spec_drafted.sum())
        print(f"[generate] speculative k={args.speculative} draft_layers={args.draft_layers}: {gen.spec_rounds} rounds, "
              f"{n / max(gen.spec_rounds, 1):.2f} tokens per round over the batch, accepted / drafted = {acc} / {dr}")


if __name__ == "__main__":
    main(parse_args())
